"""The ambient occlusion integrator on the GPU (device/ao.inl; ambientocclusion.cpp:29-74), checked without the CPU checker: open and closed
scenes whose answer is known exactly, the weight's structure, the dumped rays against the pinned generator and a numpy restatement of the
sampling, the occlusion bits against the ray service and the exact-arithmetic classifier, the counts against an analytic solid angle,
statistics, determinism and the invariances every pipeline here keeps."""
import ctypes as C

import numpy as np
import pytest

import ao_helpers as H
import exact_rays as X
import oracle_binding as ob
from pearray_amd import _cabi as abi
from pearray_amd import backend, scene

pytestmark = pytest.mark.gpu
F = np.float32
W, HGT = 96, 64
EPS32 = 2.0 ** -24
EYE, TARGET = (0.0, -3.0, 2.0), (0.0, 0.0, 0.0)
FLOOR = [[-2, -2, 0], [2, -2, 0], [2, 2, 0], [-2, 2, 0]]
# One ulp-scale margin for a rebuilt unit direction: the hemisphere sample (a square root, two products), the tangent-space sum (three products,
# two sums) and the normalisation (three squares, two sums, a root, a division) are about a dozen roundings of values <= 1, and they do not all
# line up: 8 half-ulps of 1.
UNIT_ULPS = 8 * EPS32
# ... and what the backend's shared fp32 sin / cos of 2 pi u (pr_sincos_2pi) differs from numpy's sin / cos of fl(2 pi) * u: measured over all
# 2^23 arguments k / 2^23 at most 7 * 2^-24 for the sine and 6.25 * 2^-24 for the cosine (the test measures it again on its own arguments)
SINCOS_BOUND = 8 * EPS32
# frame_occluded / frame_open against weight: the open frame is fl(w * sum_k cie_k), the occluded one fl(w * sum_k fl(weight * cie_k)).  The one multiply
# the weight adds rounds each (non-negative) term by <= 2^-24 relative; the three additions of the sum and the multiply by w round on either side
# (<= 4 * 2^-24 each): to first order the ratio is within (1 + 4 + 4) * 2^-24 of the weight, 10 * 2^-24 with room for the second order.
WEIGHT_RTOL = 10 * EPS32


def rel_l2(a, b):
    return float(np.sqrt(((a.astype(np.float64) - b) ** 2).sum()) / max(np.sqrt((b.astype(np.float64) ** 2).sum()), 1e-30))


def render(sc, iterations=1, instrument=False, aovs=(), tiles=None, calls=None):
    ctx = backend.RenderContext(sc, device=0)
    if instrument:
        ctx.setInstrumentation(True)
    if aovs:
        ctx.enableAOVs(aovs)
    if tiles is not None:
        ctx.setTiles(tiles)
    for n in (calls or [iterations]):
        ctx.render(n)
    ctx.waitForFinish()
    return ctx


def floor_scene(n, occluder=None, sampler=abi.SAMPLER_RANDOM, filt=abi.FILTER_BLOCK, radius=0, floor=FLOOR, eye=EYE):
    b, white = H.builder(W, HGT, n, eye, TARGET, sampler=sampler, filt=filt, radius=radius)
    H.quad(b, white, floor, toward=eye)
    if occluder is not None:
        H.quad(b, white, occluder)
    return b.build()


def box_scene(n, **kw):
    """A floor and a box floating above it (no contact anywhere), seen from above."""
    b, white = H.builder(W, HGT, n, EYE, TARGET, **kw)
    H.quad(b, white, FLOOR, toward=EYE)
    for q in H.box_quads((-0.5, -0.5, 0.3), (0.5, 0.5, 1.0)):
        H.quad(b, white, q, away=(0, 0, 0.65))   # outward normals
    return b.build()


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------------
AO_PRC = """(scene :render_width 48 :render_height 32 :camera 'c'
  (sampler :slot 'aa' :type 'random' :sample_count 4) (filter :type 'block' :radius 0)
  (integrator :type 'ao' :sample_count 32)
  (camera :name 'c' :type 'standard' :width 1 :height 0.667 :local_direction [0,0,-1] :local_up [0,1,0] :local_right [1,0,0] :transform [1,0,0,0, 0,1,0,0.6, 0,0,1,4, 0,0,0,1])
  (material :name 'm' :type 'diffuse' :albedo 0.8)
  %s
)"""
MESH_LIKE = AO_PRC % """(mesh :name 'floor' (attribute :type 'p' [-3,0,-3],[3,0,-3],[3,0,3],[-3,0,3]) (faces [0,3,2],[0,2,1]))
  (mesh :name 'pyramid' (attribute :type 'p' [-0.7,0.2,-0.7],[0.7,0.2,-0.7],[0.7,0.2,0.7],[-0.7,0.2,0.7],[0,1.4,0])
     (attribute :type 'n' [-0.6,0.5,-0.6],[0.6,0.5,-0.6],[0.6,0.5,0.6],[-0.6,0.5,0.6],[0,1,0]) (faces [0,4,1],[1,4,2],[2,4,3],[3,4,0],[0,1,2],[0,2,3]))
  (entity :name 'f' :type 'mesh' :mesh 'floor' :materials 'm')
  (entity :name 'p' :type 'mesh' :mesh 'pyramid' :materials 'm')"""
SPHERE_LIKE = AO_PRC % """(entity :name 'f' :type 'plane' :x_axis [6,0,0] :y_axis [0,0,-6] :centering true :materials 'm')
  (entity :name 's' :type 'sphere' :radius 0.6 :materials 'm' :transform [1,0,0,0, 0,1,0,0.9, 0,0,1,0, 0,0,0,1])"""


def test_an_ao_scene_renders():
    assert hasattr(backend.RenderContext, "enableAmbientOcclusion")
    sc = scene.PrcScene(source=MESH_LIKE)
    assert (sc.integrator, sc.ao_sample_count) == (abi.INTEGRATOR_AO, 32)
    ctx = render(sc, 2)
    xyz, smp, fb = ctx.output()
    assert ctx.ao_sample_count == 32 and ctx.pipelineInfo()["mode"] == 0
    assert np.isfinite(xyz).all() and xyz.max() > 0 and smp.max() == 2 and not fb.any()
    assert ctx.aoCounts().max() > 0 and ctx.aoCounts().max() <= 64


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------------
def sphere_scene(n, inner):
    b, white = H.builder(W, HGT, n, (0, -4, 0.5), (0, 0, 0))
    b.add_sphere(white, radius=1.0)
    if inner:   # inside the sphere: hidden from the camera, below every tangent plane
        H.quad(b, white, [[-0.2, -0.2, 0], [0.2, -0.2, 0], [0.2, 0.2, 0], [-0.2, 0.2, 0]])
    return b.build()


def plane_scene(n, below):
    b, white = H.builder(W, HGT, n, EYE, TARGET)
    b.add_plane(white, x_axis=(1, 0, 0), y_axis=(0, 1, 0), width=4.0, height=4.0, centering=True)
    if below:   # under the plane's middle: hidden from the camera by the plane, below every hemisphere
        H.quad(b, white, [[-0.5, -0.5, -1], [0.5, -0.5, -1], [0.5, 0.5, -1], [-0.5, 0.5, -1]])
    return b.build()


@pytest.mark.parametrize("make", [plane_scene, sphere_scene])
@pytest.mark.parametrize("n", [1, 10, 32])
def test_open_scene_weight_is_exactly_one(make, n):
    a, b = render(make(n, False), 3), render(make(n, True), 3)
    xa, sa, _ = a.output()
    xb, sb, _ = b.output()
    assert not a.aoCounts().any() and not b.aoCounts().any()
    assert np.array_equal(xa, xb) and np.array_equal(sa, sb)   # nothing occludes in either: weight 1 bit for bit
    hit = sa > 0   # at least one of the pixel's three (jittered) samples hit; the others added nothing
    assert 0 < hit.sum() < hit.size and (xa[hit] > 0).all() and not xa[~hit].any()
    assert (sa[a.primaryHits()[0] != abi.INVALID_ID] > 0).all()
    # `direct` in the same light-less scene leaves the same sample counts (none for a miss) and the same primary hits.  One iteration: the first
    # camera sample of a pixel is the same draw under both integrators, later ones are not (a hit spends 2 N numbers of the pixel's stream here)
    a1, d1 = render(make(n, False), 1), render(make(0, False), 1)
    assert np.array_equal(a1.output()[1], d1.output()[1]) and all(np.array_equal(x, y) for x, y in zip(a1.primaryHits(), d1.primaryHits()))
    assert not a1.output()[1][a1.primaryHits()[0] == abi.INVALID_ID].any() and not d1.output()[0].any()


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 10])
def test_closed_scene_is_black(n):
    b, white = H.builder(W, HGT, n, (0, 0, 0), (0, 1, 0))
    for q in H.box_quads((-1, -1, -1), (1, 1, 1)):
        H.quad(b, white, q, toward=(0, 0, 0))   # inward normals: the hemispheres lie inside the box
    ctx = render(b.build(), 3)
    xyz, smp, _ = ctx.output()
    assert (ctx.aoCounts() == 3 * n).all() and not xyz.any() and (smp == 3).all()


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------------
OCCLUDER = [[-1, 0.5, 1.5], [1, 0.5, 1.5], [1, 2, 1.5], [-1, 2, 1.5]]   # above the far half of the floor, above the camera's view


@pytest.mark.parametrize("n", [1, 10, 32])
def test_weight_structure(n):
    aovs = ("position",)
    o, f = render(floor_scene(n, OCCLUDER), aovs=aovs), render(floor_scene(n), aovs=aovs)
    # same camera samples and wavelengths in both: the random budget does not depend on what the rays find
    assert all(np.array_equal(a, b) for a, b in zip(o.primaryHits(), f.primaryHits())) and np.array_equal(o.aov("position"), f.aov("position"))
    hit = f.primaryHits()[0] != abi.INVALID_ID
    assert (f.primaryHits()[0][hit] == 0).all()   # the occluder is not in view
    k = o.aoCounts()
    assert not f.aoCounts().any() and k[hit].max() > 0 and k.max() <= n
    want = (F(1) - k.astype(F) / F(n)).astype(np.float64)
    xo, xf = o.output()[0].astype(np.float64), f.output()[0].astype(np.float64)
    assert (xf[hit] > 0).all()
    ratio = xo[hit] / xf[hit]
    assert (np.abs(ratio - want[hit][:, None]) <= WEIGHT_RTOL * want[hit][:, None]).all(), np.abs(ratio - want[hit][:, None]).max()


# ---- 5, 6, 7, 11 ------------------------------------------------------------------------------------------------------------------------
def entity_scene(kind, n):
    if kind == "box":
        return box_scene(n)
    b, white = H.builder(W, HGT, n, EYE, TARGET)
    H.quad(b, white, FLOOR, toward=EYE)
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = (0, 0, 0.8)
    if kind == "sphere":
        b.add_sphere(white, radius=0.5, transform=T)
    elif kind == "quadric":
        b.add_cylinder(white, radius=0.4, height=0.8, transform=T)
    else:   # a tent with vertex normals that are not the face normals
        p = [[-0.6, -0.6, 0.3], [0.6, -0.6, 0.3], [0.6, 0.6, 0.3], [-0.6, 0.6, 0.3], [0, 0, 1.2]]
        nr = np.asarray([[-1, -1, 0.5], [1, -1, 0.5], [1, 1, 0.5], [-1, 1, 0.5], [0, 0, 1]], dtype=np.float64)
        b.add_mesh(p, [[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4], [0, 2, 1], [0, 3, 2]], white, normals=(nr / np.linalg.norm(nr, axis=1)[:, None]).astype(np.float32))
    return b.build()


def check_dump(ctx, n):
    """Checks 5 and 7 on a context rendered for one instrumented iteration with the frame AOVs; returns (origins, directions, bits) of the hit pixels."""
    state, org, direction, occ = ctx.aoSamples()
    hit = ctx.primaryHits()[0] != abi.INVALID_ID
    assert hit.any() and (state[hit] != 0).all() and not state[~hit].any() and not org[~hit].any() and not direction[~hit].any() and not occ[~hit].any()
    assert np.array_equal(occ.sum(-1).astype(np.uint32), ctx.aoCounts())   # 7: the counts plane is the sum of the dumped bits
    lib = ob.load()
    u = np.empty((int(hit.sum()), 2 * n), dtype=F)
    for i, s0 in enumerate(state[hit]):
        s = C.c_uint64(int(s0))
        for j in range(2 * n):
            u[i, j] = lib.orc_pcg_next_float(C.byref(s))
    u1, u2 = u[:, 0::2], u[:, 1::2]
    N, Nx, Ny, P = (ctx.aov(a)[hit][:, None, :] for a in ("normal", "tangent", "bitangent", "position"))
    phi = F(2) * F(np.pi) * u2
    ds, dc = H.sincos_2pi32(u2)
    measured = max(np.abs(ds - np.sin(phi)).max(), np.abs(dc - np.cos(phi)).max())
    assert measured <= SINCOS_BOUND, measured / EPS32
    want = H.from_tangent_space32(N, Nx, Ny, H.uniform_hemi32(u1, u2))
    d = direction[hit]
    assert np.abs(d - want).max() <= UNIT_ULPS + SINCOS_BOUND, np.abs(d - want).max() / EPS32
    # the UNIFORM hemisphere: the cosine to the normal is u1 itself -- where the entity's frame is orthonormal (interpolated vertex normals are not unit
    # vectors, and the frame built around one is skewed: mesh.cpp:229-243 as restated in geometry_point)
    dot3 = lambda a, b: np.abs((a.astype(np.float64) * b).sum(-1))[:, 0]   # noqa: E731
    ortho = np.maximum(np.maximum(dot3(N, Nx), dot3(N, Ny)), dot3(Nx, Ny)) <= 4 * EPS32
    assert ortho.mean() > 0.5
    assert np.abs((d.astype(np.float64) * N).sum(-1) - u1)[ortho].max() <= UNIT_ULPS + SINCOS_BOUND
    assert np.array_equal(org[hit], H.safe_position32(np.broadcast_to(P, d.shape), d, np.broadcast_to(N, d.shape)))
    return org[hit].reshape(-1, 3), d.reshape(-1, 3), occ[hit].reshape(-1)


FRAME_AOVS = ("normal", "tangent", "bitangent", "position")


@pytest.mark.parametrize("kind,n", [("box", 1), ("box", 10), ("box", 32), ("sphere", 10), ("quadric", 10), ("normals", 10)])
def test_ray_dump_against_the_pinned_generator_and_the_ray_service(monkeypatch, kind, n):
    dumps = []
    for width in ("4", "6"):
        monkeypatch.setenv("PRGPU_BVH_WIDTH", width)
        ctx = render(entity_scene(kind, n), instrument=True, aovs=FRAME_AOVS)
        if kind in ("box", "normals"):   # (a floor and one analytic primitive make a tree of three leaves: it has no six-wide form)
            assert ctx.pipelineInfo()["bvh_width"] == int(width)
        org, d, occ = check_dump(ctx, n)
        # 6: the ray service answers every dumped ray alike
        assert np.array_equal(ctx.traceShadowRays(org, d, H.PR_EPSILON, np.inf), occ)
        assert 0 < occ.mean() < 1
        dumps.append((org, d, occ, ctx.output()[0]))
    assert all(np.array_equal(a, b) for a, b in zip(dumps[0], dumps[1]))   # 10: both widths give the same rays, bits and frame
    if kind == "box" and n == 10:   # 6: a subset under the exact-arithmetic occlusion rule
        org, d, occ = (a[:6000] for a in dumps[0][:3])
        tris, ent, prim = H.world_triangles(entity_scene(kind, n))
        geo = X.Geometry(tris, ent, prim)
        cls = X.classify(org, d, geo.tris, margin=geo.delta(org))
        undecided = X.check_any(geo, cls, org, np.float64(H.PR_EPSILON), np.inf, occ, label="ao")
        assert undecided <= 0.02, undecided


def test_the_ray_record_needs_instrumentation_and_other_refusals():
    lib = abi.load()
    ctx = backend.RenderContext(box_scene(4), device=0)
    with pytest.raises(abi.PrgpuError, match="error -4"):
        ctx.enableLPE(["C.*"])
    ch = (abi.OutputChannel * 1)(abi.OutputChannel(0, abi.CHANNEL_SPECTRAL, 0, abi.TONE_SRGB, b"", b"C.*"))
    assert lib.prgpu_outputs_enable(ctx._h, ch, 1) == -4 and b"ambient occlusion" in lib.prgpu_last_error()
    ctx.render(1)
    ctx.waitForFinish()
    assert lib.prgpu_download_ao_samples(ctx._h, None, None, None, None) == -1 and b"instrumentation" in lib.prgpu_last_error()
    d = backend.RenderContext(box_scene(0), device=0)
    assert lib.prgpu_enable_ambient_occlusion(d._h, 0) == -1
    d.render(1)
    assert lib.prgpu_enable_ambient_occlusion(d._h, 8) == -1 and b"before the first iteration" in lib.prgpu_last_error()
    assert lib.prgpu_download_ao_counts(d._h, (C.c_uint32 * (W * HGT))()) == -1


# ---- 8 ----------------------------------------------------------------------------------------------------------------------------------
def test_counts_follow_the_solid_angle_of_a_ceiling():
    n, iters = 32, 16
    x0, x1, y0, y1, z = -0.6, 0.8, -0.5, 0.5, 1.5
    ceiling = [[x0, y0, z], [x1, y0, z], [x1, y1, z], [x0, y1, z]]
    big = [[-3, -3, 0], [3, -3, 0], [3, 3, 0], [-3, 3, 0]]
    ctx = render(floor_scene(n, ceiling, sampler=abi.SAMPLER_UNIFORM, floor=big, eye=(0.0, -3.0, 1.0)), iters, aovs=("position",))
    ent = ctx.primaryHits()[0]
    hit = ent != abi.INVALID_ID
    assert hit.sum() > 1000 and (ent[hit] == 0).all()   # the ceiling is out of view: every hit lies on the floor, the whole rectangle above its horizon
    smp = ctx.output()[1]
    assert (smp[hit] == iters).all()
    P = ctx.aov("position")[hit].astype(np.float64) / iters   # the uniform sampler: every sample of a pixel hits the same point
    p = H.rect_solid_angle(P, x0, x1, y0, y1, z) / (2 * np.pi)
    trials = float(n * iters)
    k = ctx.aoCounts()[hit].astype(np.float64)
    assert (np.abs(k - trials * p) <= 5 * np.sqrt(trials * p * (1 - p)) + 1).all(), np.abs(k - trials * p).max()
    assert abs(k.sum() - (trials * p).sum()) <= 5 * np.sqrt((trials * p * (1 - p)).sum())
    assert not ctx.aoCounts()[~hit].any()


# ---- 9, 13 ------------------------------------------------------------------------------------------------------------------------------
def check_statistics(ctx, direct, n):
    st, sd = ctx.statistics(), direct.statistics()
    smp = ctx.output()[1]
    hits, samples = int(smp.sum()), ctx.width * ctx.height * ctx.iterations_done
    assert st["shadow_rays"] == hits * n and st["entity_hits"] == hits and st["camera_depth"] == hits
    assert st["background_hits"] == samples - hits and st["bounce_rays"] == 0 and 0 < hits < samples
    # as `direct` reports them for the same film and iterations -- whose bounce rays are camera rays too (RenderTileSession.cpp:64-74), and AO has none
    assert st["camera_rays"] == sd["camera_rays"] - sd["bounce_rays"] == samples
    for key in ("primary_rays", "pixel_samples"):
        assert st[key] == sd[key] == samples, key
    assert int(ctx.aoCounts().sum()) <= hits * n
    tc = ctx.traceCounters()
    assert tc["rays_any"] == hits * n and tc["rays_closest"] == samples


@pytest.mark.parametrize("n", [1, 10, 32])
def test_statistics(n):
    check_statistics(render(box_scene(n), 3), render(box_scene(0), 3), n)


@pytest.mark.parametrize("source", [MESH_LIKE, SPHERE_LIKE])
def test_example_shaped_scenes(source):
    sc = scene.PrcScene(source=source)   # no force_direct: the scene file's own integrator
    assert not sc.warnings and (sc.integrator, sc.ao_sample_count) == (abi.INTEGRATOR_AO, 32)
    ctx = backend.RenderContext(sc, device=0)
    ctx.setInstrumentation(True)
    ctx.render(4)
    ctx.waitForFinish()
    check_statistics(ctx, render(scene.PrcScene(source=source.replace("(integrator :type 'ao' :sample_count 32)", "")), 4), 32)
    state, org, direction, occ = ctx.aoSamples()
    hit = state != 0
    assert np.array_equal(ctx.traceShadowRays(org[hit].reshape(-1, 3), direction[hit].reshape(-1, 3), H.PR_EPSILON, np.inf), occ[hit].reshape(-1))
    assert 0 < occ[hit].mean() < 1 and np.isfinite(ctx.output()[0]).all()


# ---- 10 ---------------------------------------------------------------------------------------------------------------------------------
def test_determinism_and_chunking():
    a, b = render(box_scene(10), 5), render(box_scene(10), 5)
    c = render(box_scene(10), calls=[1] * 5)
    for other in (b, c):
        assert all(np.array_equal(x, y) for x, y in zip(a.output(), other.output())) and np.array_equal(a.aoCounts(), other.aoCounts())
    assert a.output()[0].max() > 0


@pytest.mark.parametrize("filt,radius", [(abi.FILTER_BLOCK, 0), (abi.FILTER_MITCHELL, 1)])
def test_complementary_tiles_sum_to_the_frame(filt, radius):
    kw = dict(filt=filt, radius=radius)
    whole = render(box_scene(10, **kw), 3)
    left = render(box_scene(10, **kw), 3, tiles=[(0, 0, 40, HGT)])
    right = render(box_scene(10, **kw), 3, tiles=[(40, 0, W, HGT)])
    total = left.output()[0] + right.output()[0]
    if radius == 0:
        assert np.array_equal(total, whole.output()[0])
    else:
        assert rel_l2(total, whole.output()[0]) <= 1e-5
    assert np.array_equal(left.aoCounts() + right.aoCounts(), whole.aoCounts())
    assert np.array_equal(left.output()[1] + right.output()[1], whole.output()[1])


def test_a_multi_tap_filter_moves_the_film_sum_no_more_than_it_does_for_direct():
    block, mitchell = render(box_scene(10), 4), render(box_scene(10, filt=abi.FILTER_MITCHELL, radius=1), 4)
    xb, xm = block.output()[0].astype(np.float64), mitchell.output()[0].astype(np.float64)
    assert np.isfinite(xm).all() and np.array_equal(block.output()[1], mitchell.output()[1]) and np.array_equal(block.aoCounts(), mitchell.aoCounts())

    def wall(filt, radius):   # the same filter swap on a `direct` render of an emissive wall filling most of the view
        b, white = H.builder(W, HGT, 0, EYE, TARGET, filt=filt, radius=radius)
        H.quad(b, white, FLOOR, toward=EYE, emission=b.diffuse_emission(b.illuminant_d65()))
        return render(b.build(), 4).output()[0].astype(np.float64)
    wb, wm = wall(abi.FILTER_BLOCK, 0), wall(abi.FILTER_MITCHELL, 1)
    moved = abs(wm.sum() - wb.sum()) / wb.sum()
    assert abs(xm.sum() - xb.sum()) / xb.sum() <= moved, (abs(xm.sum() - xb.sum()) / xb.sum(), moved)
