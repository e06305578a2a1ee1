"""Disk entities on the GPU (disk.cpp, geometry/Disk.h; device/pr_device.h disk_hit and disk_light_sample), checked without the CPU checker, which does
not know them: against exact arithmetic (tests/exact_disk.py, with margins counted from disk_hit's operations), against closed forms and float64 quadratures of
what the reference's code computes, and against mesh scenes whose fragments perform the same fp32 operations.

Comparison kinds: bits where both sides perform the same fp32 operations; RTOL = 64 u of tests/test_gpu_vf.py where a scalar is applied on one side before
and on the other after the CIE sum; the project's 2 % + 1e-3 (tests/test_oracle_render.py:94) for Monte Carlo block means whose standard error is computed
beforehand, in float64, from the estimator's second moment and held to <= 0.4 %, so that 2 % is five standard errors."""
import numpy as np
import pytest

import ao_helpers as H
import exact_disk as D
import test_exact_rays as E
from pearray_amd import _cabi as abi
from pearray_amd import backend, scene
from test_exact_disk import rays_at
from test_gpu_vf import U, RTOL, aov_ids, close, finish, hits_of, render, s520, worst

pytestmark = pytest.mark.gpu
F = np.float32
INV = abi.INVALID_ID

# ---- the three disks ------------------------------------------------------------------------------------------------------------------------
ROT = np.asarray([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]])   # orthonormal in exact arithmetic (a 3-4-5 construction)


def xform(linear, t):
    T = np.eye(4, dtype=F)
    T[:3, :3], T[:3, 3] = np.asarray(linear, dtype=F), t
    return T


# (transform, LOCAL radius, linear scale): axis-parallel; turned by an exact pi about x; a general rotation times 2; and, for the ray service only, a tilted
# disk far from the origin (|c| = 80 r: half an ulp of its centre, 1.9e-6, is what its placeholder box is inflated by, so its rim leans on pad_box)
DISKS = [(xform(np.eye(3), (-4.0, 0.0, 1.0)), 1.0, 1.0), (xform(np.diag([1.0, -1.0, -1.0]), (0.5, 0.25, 2.0)), 0.75, 1.0), (xform(2.0 * ROT, (5.0, -1.0, 1.5)), 0.6, 2.0),
         (xform(ROT.T, (40.5, -37.25, 12.0)), 0.5, 1.0)]


def frame(T):
    """(centre, unit normal, e1, e2) in float64 of the disk the device holds for the transform T."""
    n = D.normal32(T).astype(np.float64)
    nh = n / np.linalg.norm(n)
    e1 = np.cross(nh, [0.0, 1.0, 0.0] if abs(nh[1]) < 0.9 else [1.0, 0.0, 0.0])
    e1 /= np.linalg.norm(e1)
    return D.centre32(T).astype(np.float64), nh, e1, np.cross(nh, e1)


def backdrop(k):
    """The triangle half a (local) radius beside disk k's plane, on its lower side, that covers the square the rays are aimed at, as float32 vertices."""
    T, r, scale = DISKS[k]
    c, nh, e1, e2 = frame(T)
    s = 1.5 * scale * r
    base = c - 0.5 * r * nh * np.sign(nh[2])
    return np.asarray([base - s * e1 - s * e2, base + 3 * s * e1 - s * e2, base - s * e1 + 3 * s * e2], dtype=F)


def add_three_disks(b, materials=None, emission=None, count=3):
    """Entities 0 .. count - 1: the first `count` disks; count .. 2 count - 1: their backdrops (untransformed meshes).  Returns the reference's view:
    (disks, triangles, entity, primitive)."""
    materials = materials or [b.lambert(b.spectrum_const(0.5))] * (2 * count)
    for k, (T, r, _) in enumerate(DISKS[:count]):
        assert b.add_disk(materials[k], radius=r, transform=T, emission=emission if k == 1 else None) == k
    tris = [backdrop(k) for k in range(count)]
    for k, p in enumerate(tris):
        assert b.add_mesh(p, [[0, 1, 2]], materials[count + k]) == count + k
    return ([(k, D.centre32(T), D.normal32(T), F(r)) for k, (T, r, _) in enumerate(DISKS[:count])], np.asarray(tris, dtype=np.float64), list(range(count, 2 * count)), [0] * count)


# ---- 1: the ray service against exact arithmetic ---------------------------------------------------------------------------------------------
def service_scene():
    b = scene.SceneBuilder(8, 8)
    return b, add_three_disks(b, count=len(DISKS))


@pytest.fixture(scope="module")
def service_case():
    """20 000 seeded rays, a quarter aimed at each disk: at points uniform in the bounding square of the TRANSFORMED disk (half side scale x r, so that the scaled
    disk's ring between its local and its scaled radius is aimed at too), from origins 0.1 .. 3 r off the disk's plane on either side."""
    rng = np.random.default_rng(20240)
    org, direction, aimed = [], [], []
    for k, (T, r, scale) in enumerate(DISKS):
        c, nh, e1, e2 = frame(T)
        o, d = rays_at(c, e1, e2, nh, r, 5000, rng, spread=scale)
        org.append(o), direction.append(d), aimed.append(np.full(len(o), k))
    org, direction, aimed = np.concatenate(org), np.concatenate(direction), np.concatenate(aimed)
    disks, tris, te, tp = service_scene()[1]
    return org, direction, aimed, D.candidates(org, direction, disks, tris, te, tp), disks


@pytest.mark.parametrize("width", ["4", "6"])
@pytest.mark.parametrize("split", ["0", "1"])
def test_the_ray_service_is_held_to_the_exact_reference(monkeypatch, service_case, split, width):
    """R1 - R4 and R6 of tests/exact_rays.py on disks and the triangles behind them (tests/exact_disk.py, check_closest / check_any), on four- and six-wide
    trees; PRGPU_TRACE_SPLIT=1 asks for the split service kernel, which has no disk form and must hand the scene to the plain one."""
    monkeypatch.setenv("PRGPU_TRACE_SPLIT", split)
    monkeypatch.setenv("PRGPU_BVH_WIDTH", width)
    org, direction, aimed, cand, disks = service_case
    g = backend.RenderContext(service_scene()[0].build())
    try:
        assert g.pipelineInfo()["bvh_width"] == int(width)
        hit = g.traceRays(org, direction, 1e-4, np.inf)
        tmin = float(F(1e-4))
        s = D.check_closest(cand, tmin, np.inf, hit, label="closest width %s" % width)
        print("closest", s)
        ent, prim, u, v, t = hit
        on_disk = ent < len(DISKS)
        assert on_disk.sum() > 4500 and (ent[~on_disk] != INV).sum() > 5000 and all((ent == k).sum() > 400 for k in range(len(DISKS)))   # (the scaled disk is a quarter of its square, seen from one side)
        assert not u[on_disk].any() and not v[on_disk].any() and not prim[on_disk].any()         # u = v = 0, primitive id 0
        assert s["undecided"] <= 0.01 and s["undecided_disk"] <= 0.01, s
        # the scaled disk is hit inside its LOCAL radius only: the rays aimed at its ring out to the scaled radius pass through
        tab = D.classify(org, direction, [disks[2][1]], [disks[2][2]], [disks[2][3]])
        r2 = float(disks[2][3])
        ring = (aimed == 2) & (tab.rho[:, 0] > 1.01 * r2) & (tab.rho[:, 0] < 2.0 * r2)
        assert ring.sum() > 1500 and (ent[ring] != 2).all() and (ent[(aimed == 2) & (tab.rho[:, 0] < 0.99 * r2) & (tab.t[:, 0] > 0)] != INV).all()
        # occlusion windows a margin either side of the reported distance
        near = np.where(ent != INV, t.astype(np.float64), 1.0)
        far = np.full(len(near), np.inf)
        for lo, hi in ((np.full(len(near), tmin), near * 1.01 + 0.001), (np.full(len(near), tmin), near * 0.99 + 0.001), (near * 0.99, far), (near * 1.01, far)):
            lo32, hi32 = lo.astype(F), hi.astype(F)
            occ = g.traceShadowRays(org, direction, lo32, hi32)
            sa = D.check_any(cand, lo32.astype(np.float64), hi32.astype(np.float64), occ, label="any width %s" % width)
            print("any", sa)
            assert sa["undecided"] <= 0.01, sa
    finally:
        g.close()


# ---- 2: the path kernel's primary hits and AOVs, in every pipeline ----------------------------------------------------------------------------
CW, CH = 79, 59
CAM_EYE = (0.5, -8.0, 7.5)
CAM = dict(width=1.3, height=1.3 * CH / CW, local_direction=(0, 0.8, -0.6), local_up=(0, 0.6, 0.8), local_right=(1, 0, 0))
AOVS = ("position", "normal", "entity_id", "material_id", "emission_id")


def camera_scene(integ=None, mono=False):
    """The three disks and their backdrops under the lens-less perspective camera with the `uniform` sampler and a single-tap filter: one known ray per
    pixel (tests/test_exact_rays.py, input 8).  Every entity has a material of its own; disk 1 is emissive."""
    b = scene.SceneBuilder(CW, CH)
    s = b.settings
    s.aa_sampler, s.aa_samples, s.filter, s.filter_radius = abi.SAMPLER_UNIFORM, 1, abi.FILTER_BLOCK, 0
    mats = [b.lambert(b.spectrum_const(0.3 + 0.1 * k)) for k in range(6)]
    geo = add_three_disks(b, mats, emission=b.diffuse_emission(b.spectrum_const(1.0)))
    T = np.eye(4, dtype=F)
    T[:3, 3] = CAM_EYE
    b.set_camera(T, near=1e-6, **CAM)
    return finish(b, integ, mono=mono), geo


@pytest.fixture(scope="module")
def camera_case():
    y, x = np.meshgrid(np.arange(CH, dtype=np.float64), np.arange(CW, dtype=np.float64), indexing="ij")
    nx, ny = 2 * (x / CW - 0.5), -2 * (y / CH - 0.5)
    d = (nx[..., None] * (0.5 * CAM["width"]) * np.asarray(CAM["local_right"], dtype=np.float64) + ny[..., None] * (0.5 * CAM["height"]) * np.asarray(CAM["local_up"], dtype=np.float64)
         + np.asarray(CAM["local_direction"], dtype=np.float64))
    n = CW * CH
    org, direction = np.broadcast_to(np.asarray(CAM_EYE, dtype=F), (n, 3)).copy(), E._unit32(d.reshape(n, 3))
    disks, tris, te, tp = camera_scene()[1]
    return org, direction, D.candidates(org, direction, disks, tris, te, tp, extra_ulps=E.CAMERA_ULPS)


PIPELINES = [dict(PRGPU_MODE="persistent", PRGPU_PP_KERNEL="throughput"), dict(PRGPU_MODE="persistent", PRGPU_PP_KERNEL="latency"), dict(PRGPU_MODE="lockstep"),
             dict(PRGPU_MODE="streaming")]


def test_primary_hits_and_aovs_in_every_pipeline(monkeypatch, camera_case):
    """The primary-hit plane under R1, R2 (by id) and R4; the AOVs on disk pixels; the same frame and planes, bit for bit, from the persistent, lockstep and streaming
    pipelines.  The second leg asks for the persistent kernel's latency organisation: the shipped build holds it for variant rows 1 and 4 only (Makefile,
    PL_VARIANTS), so there the library falls back to the throughput kernel and the leg repeats the first; a build with `make PL_VARIANTS="1 2 3 4 5"` runs
    device/path_wave.inl with disks here and must give the same bits.  The kernels that ran are printed."""
    org, direction, cand = camera_case
    frames = []
    for env in PIPELINES:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ctx = render(camera_scene()[0], 1, aovs=AOVS)
        frames.append((ctx.output(), ctx.primaryHits(), [ctx.aov(a) for a in AOVS], ctx.pipelineInfo()))
        ctx.close()
        for k in env:
            monkeypatch.delenv(k)
    print("pipelines:", [(f[3]["mode"], f[3]["kernel"]) for f in frames])
    assert frames[0][3]["kernel"] == "throughput" and frames[1][3]["kernel"] in ("throughput", "latency") and frames[0][3]["mode"] == frames[1][3]["mode"] and len({f[3]["mode"] for f in frames}) == 3
    for other in frames[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(frames[0][0], other[0])) and all(np.array_equal(a, b) for a, b in zip(frames[0][1], other[1]))
        assert all(np.array_equal(a, b) for a, b in zip(frames[0][2], other[2]))
    (xyz, smp, fb), (ent, prim), planes, _ = frames[0]
    ent, prim = ent.reshape(-1), prim.reshape(-1)
    s = D.check_closest(cand, 1e-6, np.inf, (ent, prim, None, None, None), label="primary hits")
    print("primary", s)
    assert s["undecided"] <= 0.01 and all((ent == k).sum() > 30 for k in range(6)), (s, [(ent == k).sum() for k in range(6)])
    assert (smp.reshape(-1)[ent != INV] == 1).all() and np.isfinite(xyz).all() and xyz.max() > 0   # (a camera ray that leaves this light-less scene adds no sample)
    pos, nrm, eid, mid, emid = (p.reshape(len(ent), -1) for p in planes)
    on = ent < 3
    assert not prim[on].any()
    assert np.array_equal(aov_ids(eid[:, 0])[ent != INV], ent[ent != INV].astype(np.uint64)) and np.array_equal(aov_ids(mid[:, 0])[ent != INV], ent[ent != INV].astype(np.uint64))
    assert (aov_ids(emid[:, 0])[ent == 1] == 0).all() and (aov_ids(emid[:, 0])[on & (ent != 1)] == INV).all()
    # the normal: N = normalize(normalMatrix (0, 0, 1)), NOT flipped towards the viewer -- exact where the matrix is a signed permutation
    assert np.array_equal(nrm[ent == 0], np.tile(F([0, 0, 1]), ((ent == 0).sum(), 1))) and np.array_equal(nrm[ent == 1], np.tile(F([0, 0, -1]), ((ent == 1).sum(), 1)))
    n2 = D.normal32(DISKS[2][0]).astype(np.float64)
    assert np.abs(nrm[ent == 2].astype(np.float64) - n2 / np.linalg.norm(n2)).max() <= 4 * U
    # the position: o + t d with the kernel's own t and d, i.e. within the candidate's tolerance plus the camera's and two roundings of o + t d
    rays = np.nonzero(on)[0]
    row = D.lookup(cand, rays, ent[rays], prim[rays])
    assert (row >= 0).all()
    want = org[rays].astype(np.float64) + cand.t[row][:, None] * direction[rays].astype(np.float64)
    room = cand.tol[row] + (E.CAMERA_ULPS + 4) * U * np.maximum(cand.t[row], np.abs(org[rays]).max(1))
    off = np.linalg.norm(pos[rays].astype(np.float64) - want, axis=1)
    print("position: largest share of the allowance %.3f" % (off / room).max())
    assert (off <= room).all() and room.max() < 1e-3


# ---- 3: ambient occlusion ---------------------------------------------------------------------------------------------------------------------
W, HGT = 80, 60
EYE, TARGET = (0.0, -3.0, 2.0), (0.0, 0.0, 0.0)


def test_ao_of_a_lone_disk_is_unoccluded_and_weighs_exactly_one():
    """The hemisphere stands on the shading normal (0, 0, 1): no ray can meet the disk again, the weight is 1 - 0 / n = 1 -- in mono the frame's one value,
    and the value a lone mesh quad gives, whose weight is 1 for the same reason."""
    def make(kind):
        b, white = H.builder(W, HGT, 4, EYE, TARGET)
        if kind == "disk":
            b.add_disk(white, radius=1.0)
        else:
            H.quad(b, white, [[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], toward=EYE)
        return finish(b, None, mono=True)
    d, q = render(make("disk")), render(make("quad"))
    hit = hits_of(d)
    assert 500 < hit.sum() < hits_of(q).sum() and not d.aoCounts().any() and not q.aoCounts().any()
    (xd, sd, fd), (xq, sq, _) = d.output(), q.output()
    assert not fd.any() and not xd[~hit].any() and (sd[hit] == 1).all()
    wd, wq = np.unique(xd[hit]), np.unique(xq[hits_of(q)])
    assert len(wd) == 1 and wd[0] > 0 and np.array_equal(wd, wq)


def over_floor(n):
    b, white = H.builder(W, HGT, n, EYE, TARGET)
    floor = np.asarray([[-2, -2, 0], [2, -2, 0], [2, 2, 0], [-2, 2, 0]], dtype=F)
    H.quad(b, white, floor, toward=EYE)
    T = xform(np.eye(3), (0.0, 0.2, 0.6))
    b.add_disk(white, radius=0.8, transform=T)
    tris = np.asarray([floor[[0, 1, 2]], floor[[0, 2, 3]]], dtype=np.float64)
    return b.build(), ([(1, D.centre32(T), D.normal32(T), F(0.8))], tris, [0, 0], [0, 1])


def test_ao_rays_of_a_disk_over_a_floor_replay_through_the_ray_service_and_match_the_reference():
    sc, (disks, tris, te, tp) = over_floor(4)
    ctx = backend.RenderContext(sc, device=0)
    ctx.setInstrumentation(True)
    ctx.render(1)
    ctx.waitForFinish()
    state, org, direction, occ = ctx.aoSamples()
    hit = hits_of(ctx)
    ent = ctx.primaryHits()[0]
    assert (state[hit] != 0).all() and not state[~hit].any() and (ent == 0).sum() > 500 and (ent == 1).sum() > 300
    assert np.array_equal(occ.sum(-1).astype(np.uint32), ctx.aoCounts())
    o, d, bits = org[hit].reshape(-1, 3), direction[hit].reshape(-1, 3), occ[hit].reshape(-1)
    assert np.array_equal(ctx.traceShadowRays(o, d, H.PR_EPSILON, np.inf), bits)
    assert 0.02 < bits.mean() < 0.9 and not occ[ent == 1].any() and occ[ent == 0].any()        # the disk shadows the floor and nothing shadows the disk
    cand = D.candidates(o, d, disks, tris, te, tp)
    s = D.check_any(cand, np.float64(H.PR_EPSILON), np.inf, bits, label="ao")
    print("ao", s)
    assert s["undecided"] <= 0.02, s


# ---- 4: visual feedback -----------------------------------------------------------------------------------------------------------------------
def vf_scene(integ):
    """A floor (entity 0), an emissive disk (1) and a tilted disk (2) with materials 0, 1, 0, in mono."""
    b, white = H.builder(W, HGT, 0, (0.0, -4.0, 3.0), (0, 0, 0.3))
    grey = b.lambert(b.spectrum_const(0.4))
    H.quad(b, white, [[-2, -2, 0], [2, -2, 0], [2, 2, 0], [-2, 2, 0]], toward=(0, 0, 5))
    b.add_disk(grey, radius=0.7, transform=xform(np.eye(3), (-0.9, 0.0, 0.8)), emission=b.diffuse_emission(b.illuminant_d65()))
    b.add_disk(white, radius=0.5, transform=xform(ROT.T, (1.0, 0.2, 0.9)))
    return finish(b, integ, mono=True)


@pytest.fixture(scope="module")
def vf_anchor():
    a = render(vf_scene(("ao", 1)))
    free = hits_of(a) & (a.aoCounts() == 0)
    w = np.unique(a.output()[0][free])
    assert free.sum() > 500 and len(w) == 1 and w[0] > 0
    return float(w[0]), a


@pytest.mark.parametrize("mode", ["colored_entity_id", "colored_material_id", "colored_emission_id", "colored_primitive_id"])
def test_vf_id_modes_colour_disks_by_id_modulo_23(vf_anchor, mode):
    w, a = vf_anchor
    v = render(vf_scene(("vf", mode, False)), aovs=("entity_id", "material_id", "emission_id"))
    xv, sv, fv = v.output()
    hit = hits_of(v)
    ent, prim = v.primaryHits()
    assert np.array_equal(sv, a.output()[1]) and all(np.array_equal(p, q) for p, q in zip(a.primaryHits(), v.primaryHits())) and not fv.any()
    assert all((ent == k).sum() > 100 for k in range(3)) and not prim[(ent == 1) | (ent == 2)].any() and set(np.unique(prim[ent == 0])) == {0, 1}
    ids = {"colored_entity_id": aov_ids(v.aov("entity_id")), "colored_material_id": aov_ids(v.aov("material_id")), "colored_emission_id": aov_ids(v.aov("emission_id")),
           "colored_primitive_id": prim.astype(np.uint64)}[mode]
    if mode == "colored_entity_id":
        assert np.array_equal(ids[hit], ent[hit].astype(np.uint64))
    if mode == "colored_material_id":
        assert np.array_equal(ids[hit], np.asarray([0, 1, 0], dtype=np.uint64)[ent[hit]])
    if mode == "colored_emission_id":
        assert (ids[ent == 1] == 0).all() and (ids[hit & (ent != 1)] == INV).all()
    row = (ids % 23).astype(np.int64)
    want = np.asarray([float(s520(k)) for k in range(23)])[row] * w
    assert not xv[~hit].any() and (xv[hit][:, 0] == xv[hit][:, 1]).all() and (xv[hit][:, 0] == xv[hit][:, 2]).all()
    print("%s on disks against upsample(colour[id %% 23], 520) x ao: worst %.2f u" % (mode, worst(xv[hit][:, 0], want[hit])))
    assert close(xv[hit][:, 0], want[hit]).all()


def head_on_disk(integ, back=False):
    """tests/test_gpu_vf.py's head-on scene with a disk for the quad: N = (0, 0, 1) from either side (both faces are hit, the normal is not flipped)."""
    b = scene.SceneBuilder(W, HGT)
    s = b.settings
    s.aa_sampler, s.aa_samples, s.filter, s.filter_radius, s.mapper = abi.SAMPLER_RANDOM, 64, abi.FILTER_BLOCK, 0, abi.MAPPER_RANDOM
    T = np.eye(4, dtype=F)
    T[2, 3] = -3.0 if back else 3.0
    b.set_camera(T, width=2.0, height=2.0 * HGT / W, local_direction=(0, 0, 1 if back else -1), local_right=(1, 0, 0), local_up=(0, 1, 0), ortho=True)
    b.add_disk(b.lambert(b.spectrum_const(0.8)), radius=0.55)
    return finish(b, integ)


def test_vf_inside_and_ndotv_from_front_and_back():
    f = {}
    for key, integ, back in (("inside", ("vf", "inside", False), False), ("ndotv", ("vf", "ndotv"), False), ("inside_back", ("vf", "inside", True), True),
                             ("ndotv_back", ("vf", "ndotv"), True)):
        ctx = render(head_on_disk(integ, back), 2, aovs=("normal", "view"))
        xyz, smp, fb = ctx.output()
        hit = hits_of(ctx)
        assert 400 < hit.sum() < hit.size and not fb.any() and not xyz[smp == 0].any() and (xyz[smp > 0] > 0).all()
        n, v = ctx.aov("normal"), ctx.aov("view")
        assert np.array_equal(n[..., 2], smp.astype(F)) and np.array_equal(v[..., 2], smp.astype(F) * F(1 if back else -1)) and not n[..., :2].any() and not v[..., :2].any()
        f[key] = (xyz, smp)
    assert all(np.array_equal(f[k][1], f["inside"][1]) for k in f)
    # front: N.V = -1, `inside` False = red, `ndotv` green x 1; back: N.V = +1, `inside` True = green (x |N.V| = 1), `ndotv` red x 1 -- bits
    assert np.array_equal(f["inside_back"][0], f["ndotv"][0]) and np.array_equal(f["ndotv_back"][0], f["inside"][0]) and not np.array_equal(f["inside"][0], f["ndotv"][0])


def test_vf_parameter_on_a_disk_is_zero_zero_t(camera_case):
    """w (r 0 + g 0 + b t): the reported t is within the candidate's tolerance of the exact one (tests/exact_disk.py), the colour factor within RTOL."""
    org, direction, cand = camera_case
    a, v = render(camera_scene(("ao", 1), mono=True)[0]), render(camera_scene(("vf", "parameter", False), mono=True)[0])
    ent, prim = (p.reshape(-1) for p in v.primaryHits())
    free = (hits_of(a) & (a.aoCounts() == 0)).reshape(-1)
    w = np.unique(a.output()[0].reshape(-1, 3)[free])
    assert len(w) == 1 and free.sum() > 200
    rays = np.nonzero(ent < 3)[0]
    row = D.lookup(cand, rays, ent[rays], prim[rays])
    assert (row >= 0).all() and len(rays) > 100
    bl = float(s520(abi.VF_COLOR_BLUE))
    want, room = float(w[0]) * bl * cand.t[row], float(w[0]) * bl * cand.tol[row]
    got = v.output()[0].reshape(-1, 3)[rays]
    dev = np.abs(got[:, 0].astype(np.float64) - want)
    print("parameter on disks: largest share of the allowance %.3f" % (dev / (RTOL * want + room)).max())
    assert (dev <= RTOL * want + room).all() and (got[:, 0] == got[:, 1]).all() and (got[:, 0] == got[:, 2]).all() and room.max() < 1e-4 * want.max()


# ---- 5: an emissive disk seen directly -----------------------------------------------------------------------------------------------------------
def test_an_emissive_disk_seen_head_on_equals_an_emissive_quad_bit_for_bit():
    """Black material, constant emission, the orthographic head-on camera, the `uniform` sampler: on the pixels whose ray meets the disk, the fragment is that of
    a mesh quad with the same material and emission -- BITS.  The operations coincide: the camera ray and the pixel's wavelengths do not depend on the
    scene; handleDirectHit at the camera vertex takes the unweighted branch (the camera counts as a delta vertex, direct.cpp:369-377), so neither the light's
    area nor its pdf enters; N is (0, 0, 1) exactly on both (the quad has no vertex normals: normalize((0, 0, 1.44f))), hence N.V = -1; the radiance node
    is the same; the black material ends the path with zero-valued fragments on both."""
    def make(kind):
        b = scene.SceneBuilder(W, HGT)
        s = b.settings
        s.aa_sampler, s.aa_samples, s.filter, s.filter_radius = abi.SAMPLER_UNIFORM, 1, abi.FILTER_BLOCK, 0
        T = np.eye(4, dtype=F)
        T[2, 3] = 3.0
        b.set_camera(T, width=2.0, height=2.0 * HGT / W, local_direction=(0, 0, -1), local_right=(1, 0, 0), local_up=(0, 1, 0), ortho=True)
        black, ems = b.lambert(b.spectrum_const(0.0)), b.diffuse_emission(b.illuminant_d65())
        if kind == "disk":
            b.add_disk(black, radius=0.55, emission=ems)
        else:
            b.add_mesh([[-0.6, -0.6, 0], [0.6, -0.6, 0], [0.6, 0.6, 0], [-0.6, 0.6, 0]], [[0, 1, 2], [0, 2, 3]], black, emission=ems)
        return b.build()
    d, q = render(make("disk")), render(make("quad"))
    hd, hq = hits_of(d), hits_of(q)
    assert 400 < hd.sum() < hq.sum() and not (hd & ~hq).any()
    (xd, sd, _), (xq, sq, _) = d.output(), q.output()
    assert np.array_equal(xd[hd], xq[hd]) and np.array_equal(sd[hd], sq[hd]) and (xd[hd] > 0).all() and not xd[~hd].any()
    # ... and the disk's pixels are those whose centre lies inside the radius
    y, x = np.meshgrid(np.arange(HGT), np.arange(W), indexing="ij")
    rho = np.hypot(2.0 * (x / W - 0.5), -2.0 * (y / HGT - 0.5) * (HGT / W))
    assert hd[rho < 0.55 - 1e-5].all() and not hd[rho > 0.55 + 1e-5].any()


# ---- 6, 7: radiometry -------------------------------------------------------------------------------------------------------------------------
RW = 40
SPP = 4096
BLOCKS = ((20, 20), (25, 20))        # 5 x 5 pixels around the axis and around the lateral offset 0.5 (pixel p is centred on x = 0.1 p - 2)


def floor_scene(scale=1.0, **settings):
    """The floor of test_analytic_form_factor (4 x 4, albedo 1, vertex normals) under a disk of R = 1 at h = 1 that faces down through an exact pi rotation about
    x (times `scale`), unit emission, black material; an orthographic camera between the two looks down."""
    b = scene.SceneBuilder(RW, RW)
    s = b.settings
    s.aa_sampler, s.aa_samples, s.filter, s.filter_radius = abi.SAMPLER_MJITT, SPP, abi.FILTER_BLOCK, 0
    for k, v in settings.items():
        setattr(s, k, v)
    b.add_mesh([[-2, -2, 0], [2, -2, 0], [2, 2, 0], [-2, 2, 0]], [[0, 1, 2], [0, 2, 3]], b.lambert(b.spectrum_const(1.0)), normals=[[0, 0, 1]] * 4)
    b.add_disk(b.lambert(b.spectrum_const(0.0)), radius=1.0, transform=xform(scale * np.diag([1.0, -1.0, -1.0]), (0.0, 0.0, 1.0)), emission=b.diffuse_emission(b.spectrum_const(1.0)))
    T = np.eye(4, dtype=F)
    T[2, 3] = 0.5
    b.set_camera(T, width=4.0, height=4.0, local_direction=(0, 0, -1), local_right=(1, 0, 0), local_up=(0, 1, 0), ortho=True)
    return b.build()


def block_offsets(px, py):
    """Lateral offsets from the axis of 2 x 2 points in each of the block's 5 x 5 pixels (pixel p covers x in [0.1 p - 2.05, 0.1 p - 1.95)), as (distinct
    offsets, how often each occurs): the midpoint rule on a quarter pixel is off by a 96th of 0.05^2 E'' / E, below 0.01 % here."""
    sub = (np.arange(2) + 0.5) / 2 - 0.5
    xs = (0.1 * (np.arange(px - 2, px + 3)[:, None] + sub[None, :]) - 2.0).reshape(-1)
    ys = (0.1 * (np.arange(py - 2, py + 3)[:, None] + sub[None, :]) - 2.0).reshape(-1)
    return np.unique(np.round(np.hypot(xs[:, None], ys[None, :]).reshape(-1), 12), return_counts=True)


def block_expectation(px, py, moments):
    """(mean of the expectation over the block, relative standard error of the block mean of 25 pixels x SPP samples); moments(a) = (E X, E X^2) of one sample."""
    a, count = block_offsets(px, py)
    m = np.asarray([moments(x) for x in a], dtype=np.float64)
    m1, m2 = (m * count[:, None]).sum(0) / count.sum()
    return float(m1), float(np.sqrt(max(m2 - m1 * m1, 0.0) / (25 * SPP)) / m1)


def block_mean(ctx, px, py):
    xyz, smp, _ = ctx.output()
    assert (smp[py - 2:py + 3, px - 2:px + 3] == SPP).all()
    return float(xyz[py - 2:py + 3, px - 2:px + 3, 1].astype(np.float64).mean())


def hold(name, ctx, moments):
    for px, py in BLOCKS:
        want, se = block_expectation(px, py, moments)
        got = block_mean(ctx, px, py)
        print("%s block (%d, %d): rendered %.5f expected %.5f (%+.2f %%), standard error %.3f %%" % (name, px, py, got, want, 100 * (got / want - 1), 100 * se))
        assert se <= 0.004, se                                                # computed from the formula, not from the frame
        assert abs(got - want) < 0.02 * want + 1e-3, (name, px, py, got, want)


def test_radiometry_nee_only_follows_the_references_linear_radius_sampler():
    """(a) max_ray_depth 1, direct 0 (test_analytic_form_factor's settings): X = R^2 G(x, y(u, v)) with y at radius R v -- 0.6427 under the axis where an
    area-uniform sampler gives the form factor 0.5.  Standard errors of the block means: 0.125 % (axis), 0.157 % (offset 0.5)."""
    ctx = render(floor_scene(max_ray_depth=1, direct=0), SPP)
    hold("nee", ctx, lambda a: (D.nee_linear_radius(a, 1.0, 1.0), D.nee_linear_radius(a, 1.0, 1.0, moment=2)))
    assert abs(block_mean(ctx, 20, 20) - D.form_factor(0.0, 1.0, 1.0)) > 0.2 * D.form_factor(0.0, 1.0, 1.0)   # ... and NOT the area-uniform value


def test_radiometry_bsdf_sampling_alone_gives_the_form_factor():
    """(b) nee off, so that only a bounce finds the light (deeper vertices add nothing: the disk is black, the floor sees nothing else): a cosine-distributed direction meets the disk (weight: the albedo, 1) or nothing -- a Bernoulli variable with mean F(a), the
    closed-form form factor; geometry and emission alone.  Standard errors: sqrt((1 - F) / (F n)) = 0.319 % (axis), 0.361 % (offset 0.5)."""
    ctx = render(floor_scene(nee=0), SPP)
    hold("bsdf", ctx, lambda a: (float(D.form_factor(a, 1.0, 1.0)),) * 2)


def test_radiometry_of_the_default_integrator_nee_plus_mis():
    """(c) direct.cpp with its defaults at the floor point x, one light, selection probability 1, Russian roulette 1 below the soft depth, hero factor
    and wavelength pdfs cancelling for constant spectra.  G = cos cos' / d^2, pA = 1 / worldSurfaceArea = 1 / (pi R^2) the CLAIMED area pdf.
      light sample (direct.cpp:250-330): y = y(u, v); p_l = pA d^2 / cos' (IS::toSolidAngle of the claimed pdf), p_b = cos / pi (the Lambert pdf of the same
        direction); the contribution is Le (1 / pi) cos / p_l times the balance weight p_l / (p_l + p_b):  X_l = (1 / pi) cos / (p_l + p_b) = G / (pi pA + G).
        Its expectation is over the ACTUAL distribution of y (uniform in (u, v), radius linear in v), not over the claimed one.
      bsdf sample (direct.cpp:369-409): a cosine-distributed direction; where it meets the disk (the LOCAL radius) the emission counts with the weight
        p_b / (p_l' + p_b), p_l' = pA d^2 / cos' from sampleParameterPointPDF() = mPDF_Cache (disk.cpp:87):  X_b = (G / pi) / (pA + G / pi) = G / (pi pA + G),
        and E[X_b^k] = (1 / pi) int_disk G X_b^k dA.
    The frame's expectation is E[X_l] + E[X_b], its per-sample variance Var X_l + Var X_b (independent draws).  Standard errors: 0.124 % and 0.150 %."""
    ctx = render(floor_scene(), SPP)

    def moments(a):   # E[(X_l + X_b)^2] = E X_l^2 + E X_b^2 + 2 E X_l E X_b
        el, eb, ml, mb = D.mis_terms(a, 1.0, 1.0)
        return el + eb, ml + mb + 2 * el * eb
    hold("mis", ctx, moments)


def test_the_radius_quirk_rays_hit_the_local_radius_and_light_samples_the_scaled_one():
    """disk.cpp:70 hands Embree the LOCAL radius, sampleParameterPoint sends its points through the whole transform and the area is |det M| pi R^2
    (IEntity.h:70, ITransformable.cpp:14): under a x2 scale the primary hits cover the disc of radius R, while the NEE-only floor value is the quadrature
    with samples on the disc of radius 2 R and pdf_A = 1 / (8 pi R^2).  Standard errors: 0.265 % and 0.268 %."""
    ctx = render(floor_scene(scale=2.0, max_ray_depth=1, direct=0), SPP)
    hold("nee x2", ctx, lambda a: tuple(D.nee_linear_radius(a, 1.0, 1.0, area_scale=8.0, sample_scale=2.0, moment=k) for k in (1, 2)))
    # seen from above, orthographically, with one ray per pixel centre
    b = scene.SceneBuilder(W, HGT)
    s = b.settings
    s.aa_sampler, s.aa_samples, s.filter, s.filter_radius = abi.SAMPLER_UNIFORM, 1, abi.FILTER_BLOCK, 0
    T = np.eye(4, dtype=F)
    T[2, 3] = 3.0
    b.set_camera(T, width=4.0, height=4.0 * HGT / W, local_direction=(0, 0, -1), local_right=(1, 0, 0), local_up=(0, 1, 0), ortho=True)
    b.add_disk(b.lambert(b.spectrum_const(0.5)), radius=0.7, transform=xform(2.0 * np.eye(3), (0.0, 0.0, 0.0)))
    hit = hits_of(render(b.build()))
    y, x = np.meshgrid(np.arange(HGT), np.arange(W), indexing="ij")
    rho = np.hypot(4.0 * (x / W - 0.5), -4.0 * (y / HGT - 0.5) * (HGT / W))
    assert hit[rho < 0.7 - 1e-5].all() and not hit[rho > 0.7 + 1e-5].any() and 300 < hit.sum() < 0.5 * (rho < 1.4).sum()


# ---- 8: housekeeping ----------------------------------------------------------------------------------------------------------------------------
def lit_scene(filt=abi.FILTER_BLOCK, radius=0):
    b, white = H.builder(W, HGT, 0, EYE, TARGET, filt=filt, radius=radius, spp=8)
    H.quad(b, white, [[-2, -2, 0], [2, -2, 0], [2, 2, 0], [-2, 2, 0]], toward=(0, 0, 5))
    b.add_disk(white, radius=0.5, transform=xform(ROT.T, (0.6, 0.3, 0.5)))
    b.add_disk(b.lambert(b.spectrum_const(0.0)), radius=0.6, transform=xform(np.diag([1.0, -1.0, -1.0]), (-0.3, 0.0, 1.2)), emission=b.diffuse_emission(b.illuminant_d65()))
    return b.build()


def test_determinism_and_call_chunking():
    a, b, c = render(lit_scene(), 5), render(lit_scene(), 5), render(lit_scene(), calls=[1] * 5)
    for other in (b, c):
        assert all(np.array_equal(x, y) for x, y in zip(a.output(), other.output()))
        assert a.statistics() == other.statistics()
    assert a.output()[0].max() > 0 and a.output()[1].max() == 5


def test_complementary_tiles_sum_to_the_frame():
    whole, left, right = render(lit_scene(), 3), render(lit_scene(), 3, tiles=[(0, 0, 33, HGT)]), render(lit_scene(), 3, tiles=[(33, 0, W, HGT)])
    assert np.array_equal(left.output()[0] + right.output()[0], whole.output()[0]) and np.array_equal(left.output()[1] + right.output()[1], whole.output()[1])
    assert whole.output()[0].max() > 0


def test_statistics():
    ctx = render(lit_scene(), 3)
    st = ctx.statistics()
    samples = W * HGT * 3
    assert st["primary_rays"] == st["pixel_samples"] == samples and st["camera_rays"] == st["primary_rays"] + st["bounce_rays"] and st["light_rays"] == 0
    assert 0 < st["entity_hits"] and 0 < st["background_hits"] and st["shadow_rays"] > 0 and st["bounce_rays"] > 0
    assert ctx.pipelineInfo()["kernel"] == "throughput"


def test_refusals():
    lib = abi.load()
    for what in ("radius", "two"):
        b = scene.SceneBuilder(8, 8)
        m = b.lambert(b.spectrum_const(0.5))
        if what == "two":
            e = b.add_mesh([[0, 0, 0]] * 3, [[0, 1, 2], [0, 1, 2]], m)
            b.entities[e].kind, b.entities[e].radius = abi.ENTITY_DISK, 1.0
        else:
            b.add_disk(m, radius=1e-7)
        with pytest.raises(abi.PrgpuError, match="error -1"):
            backend.RenderContext(b.build(), device=0)
        assert b"disk entity" in lib.prgpu_last_error()
