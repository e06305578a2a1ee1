"""The visual feedback integrator on the GPU (device/vf.inl; visualfeedback.cpp:108-250), checked without the CPU checker.  Every fragment is a known
colour times a quantity the backend already exposes: the AOV planes (ids, normal, view), the exact-arithmetic ray reference (tests/exact_rays.py)
and the `ao` frame of an open scene, whose weight is exactly 1.

u = 2^-24.  Two kinds of comparison, nothing looser:
  * bits, where both sides perform the same fp32 operations;
  * RTOL = 64 u relative, where one side multiplies by a scalar before the CIE sum of fragment_value and the other after it (or in numpy).  The
    count, in fragment_value (render.hip): a fragment's XYZ component is w * sum_k (radiance_k * cie_k) -- the products with mis, importance and
    hero factor are by 1 or 0 and exact --, i.e. 1 rounding per (non-negative) term, 3 for the sum (the first addition is to 0), 1 for w: 5
    relative roundings; a scalar applied to the radiance first adds 1 per term: 6; the running mean over three iterations (fold_iteration) adds
    3 on either side.  Both sides together: at most (6 + 3) + (5 + 3) = 17 u to first order, and 64 >= 2 x 17.  In mono (one wavelength, no CIE sum)
    the device's w * s against numpy's is 1 rounding.
  * where N.V is rebuilt in float64 from the normal and view AOV planes, 4 u x |unweighted value| absolute in addition: the device's fp32 dot
    product of two unit vectors is three products and two sums, each within u / 2 of a partial sum bounded by 1 (Cauchy-Schwarz): < 3 u."""
import ctypes as C

import numpy as np
import pytest

import ao_helpers as H
import exact_rays as X
import test_exact_rays as E
from pearray_amd import _cabi as abi
from pearray_amd import backend, scene

pytestmark = pytest.mark.gpu
F = np.float32
W, HGT = 80, 60
U = 2.0 ** -24
RTOL = 64 * U
EYE, TARGET = (0.0, -3.0, 2.0), (0.0, 0.0, 0.0)
M = abi.VF_MODES


# ---- helpers ---------------------------------------------------------------------------------------------------------------------------
def render(sc, iterations=1, aovs=(), tiles=None, calls=None):
    ctx = backend.RenderContext(sc, device=0)
    if aovs:
        ctx.enableAOVs(aovs)
    if tiles is not None:
        ctx.setTiles(tiles)
    for n in (calls or [iterations]):
        ctx.render(n)
    ctx.waitForFinish()
    return ctx


def finish(b, integ, mono=False):
    """integ: None (`direct`), ("ao", n) or ("vf", mode[, weighting]); mono: :spectral_domain 520"""
    if mono:
        b.settings.spectral_start = b.settings.spectral_end = 520.0
        b.settings.spectral_mono = 1
    if integ and integ[0] == "ao":
        b.ambient_occlusion(integ[1])
    elif integ:
        b.visual_feedback(*integ[1:])
    return b.build()


def close(a, b, extra=0.0):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) <= RTOL * np.abs(b) + extra


def worst(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(all="ignore"):
        return float(np.nanmax(np.where(b != 0, np.abs(a - b) / np.abs(b), 0.0)) / U) if a.size else 0.0


def colour_rgb(k):
    rgb = (C.c_float * 3)()
    assert abi.load().prgpu_visual_feedback_color(k, rgb) == 0
    return [rgb[0], rgb[1], rgb[2]]


def upsample32(coeffs, wl=520.0):
    """upsample() of pr_device.h (SpectralUpsampler.h:45-49) in float32, in its operand order"""
    p, wl = [F(c) for c in coeffs], F(wl)
    x = (p[0] * wl + p[1]) * wl + p[2]
    return (F(0.5) * x) * (F(1) / np.sqrt(x * x + F(1))) + F(0.5)


_S520 = {}


def s520(k):
    """colour row k (prgpu_visual_feedback_color) at 520 nm: float32, from prgpu_rgb_to_coeffs"""
    if k not in _S520:
        _S520[k] = upsample32(scene.rgb_to_coeffs(colour_rgb(k)))
    return _S520[k]


def hits_of(ctx):
    return ctx.primaryHits()[0] != abi.INVALID_ID


# ---- 1: head-on plane ------------------------------------------------------------------------------------------------------------------
def head_on(integ, back=False):
    """An orthographic camera on the z axis looking at an axis-parallel quad in the plane z = 0 whose normal is +z: from z = 3 (front) or z = -3."""
    b = scene.SceneBuilder(W, HGT)
    s = b.settings
    s.aa_sampler, s.aa_samples, s.filter, s.filter_radius, s.mapper = abi.SAMPLER_RANDOM, 64, abi.FILTER_BLOCK, 0, abi.MAPPER_RANDOM
    T = np.eye(4, dtype=np.float32)
    T[2, 3] = -3.0 if back else 3.0
    b.set_camera(T, width=2.0, height=2.0 * HGT / W, local_direction=(0, 0, 1 if back else -1), local_right=(1, 0, 0), local_up=(0, 1, 0), ortho=True)
    # no vertex normals: N = normalize((p1 - p0) x (p2 - p0)) = normalize((0, 0, 0.96f)) = (0, 0, 1) exactly
    b.add_mesh([[-0.6, -0.4, 0], [0.6, -0.4, 0], [0.6, 0.4, 0], [-0.6, 0.4, 0]], [[0, 1, 2], [0, 2, 3]], b.lambert(b.spectrum_const(0.8)))
    return finish(b, integ)


@pytest.fixture(scope="module")
def head_on_frames():
    out = {}
    for key, integ, back in (("inside_w", ("vf", "inside", True), False), ("inside", ("vf", "inside", False), False), ("ndotv", ("vf", "ndotv"), False),
                             ("ray_direction", ("vf", "ray_direction", True), False), ("inside_back", ("vf", "inside", True), True), ("ndotv_back", ("vf", "ndotv"), True)):
        ctx = render(head_on(integ, back), 3, aovs=("normal", "view"))
        xyz, smp, fb = ctx.output()
        hit = hits_of(ctx)
        assert 0 < hit.sum() < hit.size and not fb.any() and (smp[hit] > 0).all() and not xyz[smp == 0].any() and (xyz[smp > 0] > 0).all()
        # N.V = -1 (front) / +1 (back) exactly: the planes hold smp x (0, 0, 1) and smp x (0, 0, -/+1)
        n, v = ctx.aov("normal"), ctx.aov("view")
        assert np.array_equal(n[..., 2], smp.astype(F)) and np.array_equal(v[..., 2], smp.astype(F) * F(1 if back else -1)) and not n[..., :2].any() and not v[..., :2].any()
        out[key] = (xyz, smp)
    return out


def test_head_on_weighting_is_the_identity(head_on_frames):
    assert np.array_equal(head_on_frames["inside_w"][0], head_on_frames["inside"][0])   # weight = |-1|: bits


def test_head_on_front_and_back_swap_the_colours_bit_for_bit(head_on_frames):
    f = head_on_frames
    assert all(np.array_equal(f[k][1], f["inside"][1]) for k in f)                      # the same samples hit in every render
    # front: `inside` is False = red, `ndotv` green x 1; back: `inside` True = green, `ndotv` red x 1
    assert np.array_equal(f["inside_back"][0], f["ndotv"][0]) and np.array_equal(f["ndotv_back"][0], f["inside"][0])
    assert not np.array_equal(f["inside"][0], f["ndotv"][0])
    red, green = f["inside"][0][f["inside"][1] > 0].astype(np.float64).sum(0), f["ndotv"][0][f["ndotv"][1] > 0].astype(np.float64).sum(0)
    assert red[0] > red[1] and green[1] > green[0]                                      # X dominates a red film, Y a green one


def test_head_on_ray_direction_is_half_red_plus_half_green(head_on_frames):
    f = head_on_frames
    want = 0.5 * (f["inside"][0].astype(np.float64) + f["ndotv"][0].astype(np.float64))   # direction (0, 0, -1) -> (1/2, 1/2, 0)
    got = f["ray_direction"][0]
    print("ray_direction against (inside + ndotv) / 2: worst %.2f u" % worst(got, want))
    assert close(got, want).all()


# ---- 2: anchor against `ao` in mono mode -----------------------------------------------------------------------------------------------
def open_scene(kind, integ):
    if kind == "sphere":
        b, white = H.builder(W, HGT, 0, (0, -4, 0.5), (0, 0, 0))
        b.add_sphere(white, radius=1.0)
    else:
        b, white = H.builder(W, HGT, 0, EYE, TARGET)
        b.add_plane(white, x_axis=(1, 0, 0), y_axis=(0, 1, 0), width=4.0, height=4.0, centering=True)
    return finish(b, integ, mono=True)


@pytest.mark.parametrize("kind", ["plane", "sphere"])
def test_inside_against_the_ao_frame_of_an_open_scene(kind):
    a, v = render(open_scene(kind, ("ao", 4))), render(open_scene(kind, ("vf", "inside", False)))
    (xa, sa, fa), (xv, sv, fv) = a.output(), v.output()
    assert not a.aoCounts().any() and not fa.any() and not fv.any()
    assert np.array_equal(sa, sv) and all(np.array_equal(p, q) for p, q in zip(a.primaryHits(), v.primaryHits()))
    hit = hits_of(v)
    assert 0 < hit.sum() < hit.size and (sv[hit] == 1).all() and not xa[~hit].any() and not xv[~hit].any()
    s = s520(abi.VF_COLOR_RED)   # seen from outside / above: front faces, False
    assert 0 < s < 1 and (xa[hit] > 0).all()
    print("inside / ao against upsample(red, 520): worst %.2f u" % worst(xv[hit], float(s) * xa[hit].astype(np.float64)))
    assert close(xv[hit], float(s) * xa[hit].astype(np.float64)).all()


# ---- 3: id modes -----------------------------------------------------------------------------------------------------------------------
BOX_EYE = (0.0, -4.0, 3.0)
EMISSIVE = 7


def boxes_scene(integ):
    """25 boxes, entities 0 .. 24, on a 5 x 5 grid; materials alternate, entity 7 alone is emissive."""
    b, white = H.builder(W, HGT, 0, BOX_EYE, (0, 0, 0))
    grey = b.lambert(b.spectrum_const(0.4))
    ems = b.diffuse_emission(b.illuminant_d65())
    pos = np.asarray([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], dtype=np.float64) * 0.3
    faces = [[0, 2, 3, 1], [4, 5, 7, 6], [0, 1, 5, 4], [2, 6, 7, 3], [0, 4, 6, 2], [1, 3, 7, 5]]
    for e in range(25):
        off = np.asarray([(e % 5) * 0.5 - 1.15, (e // 5) * 0.5 - 1.15, 0.0])
        assert b.add_mesh((pos + off).astype(np.float32), faces, (white, grey)[e % 2], emission=ems if e == EMISSIVE else None) == e
    return finish(b, integ, mono=True)


def aov_ids(plane):
    """an id AOV of one iteration back as integers ((float)PR_INVALID_ID is 2^32)"""
    v = plane.astype(np.float64)
    return np.where(v >= 2.0 ** 32, float(abi.INVALID_ID), v).astype(np.uint64)


@pytest.fixture(scope="module")
def boxes_anchor():
    """The unit frame: the `ao` render where no occlusion ray hit anything (weight 1 - 0 / 1 = 1 exactly) -- one value w on all those pixels."""
    a = render(boxes_scene(("ao", 1)))
    xa, sa, _ = a.output()
    hit = hits_of(a)
    free = hit & (a.aoCounts() == 0)
    assert free.sum() > 100
    w = np.unique(xa[free])
    assert len(w) == 1 and w[0] > 0
    return float(w[0]), a


@pytest.mark.parametrize("mode", ["colored_entity_id", "colored_material_id", "colored_emission_id", "colored_displace_id", "colored_primitive_id"])
def test_id_modes_colour_by_id_modulo_23(boxes_anchor, mode):
    w, a = boxes_anchor
    v = render(boxes_scene(("vf", mode, False)), aovs=("entity_id", "material_id", "emission_id"))
    xv, sv, fv = v.output()
    assert np.array_equal(sv, a.output()[1]) and all(np.array_equal(p, q) for p, q in zip(a.primaryHits(), v.primaryHits())) and not fv.any()
    hit = hits_of(v)
    ent, prim = v.primaryHits()
    assert np.array_equal(aov_ids(v.aov("entity_id"))[hit], ent[hit].astype(np.uint64)) and set(np.unique(ent[hit])) == set(range(25))
    ids = {"colored_entity_id": aov_ids(v.aov("entity_id")), "colored_material_id": aov_ids(v.aov("material_id")), "colored_emission_id": aov_ids(v.aov("emission_id")),
           "colored_displace_id": np.full(ent.shape, abi.INVALID_ID, dtype=np.uint64), "colored_primitive_id": prim.astype(np.uint64)}[mode]
    row = (ids % 23).astype(np.int64)
    if mode == "colored_material_id":
        assert set(np.unique(ids[hit])) == {0, 1} and np.array_equal(ids[hit], ent[hit] % 2)
    if mode == "colored_emission_id":   # absent: PR_INVALID_ID, 0xFFFFFFFF % 23 = 11
        assert (ids[hit & (ent != EMISSIVE)] == abi.INVALID_ID).all() and (row[hit & (ent != EMISSIVE)] == 11).all() and (ids[hit & (ent == EMISSIVE)] == 0).all()
    if mode == "colored_displace_id":
        assert (row == 11).all()
    if mode == "colored_primitive_id":
        assert ids[hit].max() == 11 and len(np.unique(ids[hit])) >= 4   # twelve triangles per box, top and two sides in view
    want = np.asarray([float(s520(k)) for k in range(23)])[row] * w
    assert not xv[~hit].any() and (xv[hit][:, 0] == xv[hit][:, 1]).all() and (xv[hit][:, 0] == xv[hit][:, 2]).all()   # mono: X = Y = Z
    print("%s against upsample(colour[id %% 23], 520) x ao: worst %.2f u" % (mode, worst(xv[hit][:, 0], want[hit])))
    assert close(xv[hit][:, 0], want[hit]).all()
    if mode == "colored_entity_id":   # 0 and 23, 1 and 24 share a colour; neighbours in the table do not
        val = lambda e: np.unique(xv[ent == e])   # noqa: E731
        assert len(val(0)) == 1 and np.array_equal(val(0), val(23)) and np.array_equal(val(1), val(24)) and not np.array_equal(val(0), val(1))
        assert len({float(val(e)[0]) for e in range(23)}) == 23


# ---- 4: weighting and ndotv at general angles ------------------------------------------------------------------------------------------
def tilted_scene(integ, backdrop=None):
    """A sphere, a tilted quad that faces the camera and one that faces away from it; backdrop: instead, ONE big quad across the whole view that
    faces the camera ("front") or away ("back") -- same film, camera, sampler and seed, hence the same wavelengths in every pixel."""
    b, white = H.builder(W, HGT, 0, EYE, TARGET)
    if backdrop:
        big = [[-9, 3, -9], [9, 3, -9], [9, 3, 9], [-9, 3, 9]]
        H.quad(b, white, big, **({"toward": EYE} if backdrop == "front" else {"away": EYE}))
    else:
        T = np.eye(4, dtype=np.float32)
        T[:3, 3] = (-0.9, 0.2, 0.5)
        b.add_sphere(white, radius=0.5, transform=T)
        H.quad(b, white, [[-0.2, -0.5, 0.1], [0.7, -0.3, -0.2], [0.8, 0.6, 0.5], [-0.1, 0.4, 0.8]], toward=EYE)
        H.quad(b, white, [[0.9, -0.6, 0.0], [1.6, -0.2, 0.1], [1.5, 0.5, 0.9], [0.8, 0.1, 0.8]], away=EYE)
    return finish(b, integ)


@pytest.fixture(scope="module")
def tilted():
    """N.V per pixel in float64 from the AOV planes, the hit mask, and the green / red unit frames of the film."""
    ctx = render(tilted_scene(("vf", "inside", False)), aovs=("normal", "view"))
    hit = hits_of(ctx)
    n, v = ctx.aov("normal").astype(np.float64), ctx.aov("view").astype(np.float64)
    ndv = (n * v).sum(-1)
    certain = hit & (np.abs(ndv) > 4 * U)   # (the sign of a float64 N.V within the fp32 dot product's error of zero says nothing)
    assert 0 < hit.sum() < hit.size and certain.sum() > 0.99 * hit.sum() and (ndv[certain] < 0).sum() > 200 and (ndv[certain] > 0).sum() > 50
    green, red = (render(tilted_scene(("vf", "inside", False), backdrop=k)).output()[0] for k in ("back", "front"))
    assert (green > 0).all() and (red > 0).all() and not np.array_equal(green, red)
    return ctx, ndv, certain, green, red


def test_inside_at_general_angles_is_red_in_front_and_green_behind(tilted):
    ctx, ndv, certain, green, red = tilted
    want = np.where((ndv < 0)[..., None], red, green)
    assert np.array_equal(ctx.output()[0][certain], want[certain])   # the same fp32 operations on the same wavelengths: bits


@pytest.mark.parametrize("mode", ["colored_entity_id", "ray_direction"])
def test_weighting_multiplies_by_the_cosine(tilted, mode):
    _, ndv, certain, _, _ = tilted
    xu, xw = (render(tilted_scene(("vf", mode, wt))).output()[0].astype(np.float64) for wt in (False, True))
    want = np.abs(ndv)[..., None] * xu
    print("%s weighted against |N.V| x unweighted: worst %.2f u" % (mode, worst(xw[certain], want[certain])))
    assert (xu[certain] > 0).all() and close(xw[certain], want[certain], extra=4 * U * xu[certain]).all()
    assert not xw[~hits_of(tilted[0])].any()


def test_ndotv_is_the_cosine_times_the_facing_colour_and_never_weighted(tilted):
    _, ndv, certain, green, red = tilted
    xn, xn_w = (render(tilted_scene(("vf", "ndotv", wt))).output()[0] for wt in (False, True))
    assert np.array_equal(xn, xn_w)
    colour = np.where((ndv < 0)[..., None], green, red).astype(np.float64)   # the OPPOSITE colour of `inside`: green in front
    want = np.abs(ndv)[..., None] * colour
    print("ndotv against |N.V| x colour frame: worst %.2f u" % worst(xn[certain], want[certain]))
    assert close(xn[certain], want[certain], extra=4 * U * colour[certain]).all()


# ---- 5: ray_direction and parameter in mono 520 ----------------------------------------------------------------------------------------
def test_ray_direction_from_the_view_plane():
    def make(integ):
        b, white = H.builder(W, HGT, 0, EYE, TARGET)
        H.quad(b, white, [[-2, -2, 0], [2, -2, 0], [2, 2, 0], [-2, 2, 0]], toward=EYE)
        return finish(b, integ, mono=True)
    a, v = render(make(("ao", 1))), render(make(("vf", "ray_direction", False)), aovs=("view",))
    hit = hits_of(v)
    assert 0 < hit.sum() < hit.size and not a.aoCounts().any()
    w = np.unique(a.output()[0][hit])
    assert len(w) == 1
    d = v.aov("view")[hit]
    r, g, bl = s520(abi.VF_COLOR_RED), s520(abi.VF_COLOR_GREEN), s520(abi.VF_COLOR_BLUE)
    rad = (r * (F(0.5) * (d[:, 0] + F(1))) + g * (F(0.5) * (d[:, 1] + F(1)))) + bl * (F(0.5) * (d[:, 2] + F(1)))   # visualfeedback.cpp:165-169 in float32
    assert rad.dtype == F
    got = v.output()[0][hit]
    print("ray_direction against the float32 restatement: worst %.2f u" % worst(got[:, 0], float(w[0]) * rad.astype(np.float64)))
    assert close(got[:, 0], float(w[0]) * rad.astype(np.float64)).all() and (got[:, 0] == got[:, 1]).all() and (got[:, 0] == got[:, 2]).all()
    assert len(np.unique(got[:, 0])) > 0.5 * hit.sum()   # (a direction per pixel, not one value)


def test_parameter_against_the_exact_intersection():
    """One large right-angled triangle, the lens-less perspective camera and the `uniform` sampler: one known ray per pixel, restated as
    tests/test_exact_rays.py restates it (float64, rounded; the device's own direction is within CAMERA_ULPS of it, which Geometry adds to DELTA).
    The frame is w (r u + g v + b t).  Rule R2 of tests/exact_rays.py bounds the reported t by TAU + the slide along the plane around the exact
    plane distance, and the point the reported (u, v) describe by DELTA + TAU around o + t d, hence by DELTA + 2 TAU + slide around the exact
    pierce point; the legs p1 - p0 and p2 - p0 are orthogonal, so u = (P - p0) . e1 / |e1|^2 moves by at most that distance / |e1| (v: / |e2|)."""
    Wp, Hp = 79, 59
    eye = (0.1, -3.0, 0.4)
    p = np.asarray([[-2.5, 0.5, -1.5], [2.5, 0.5, -1.5], [-2.5, 0.5, 2.5]], dtype=np.float32)   # e1 = (5, 0, 0), e2 = (0, 0, 4)
    cam = dict(width=1.6, height=1.6 * Hp / Wp, local_direction=(0, 1, 0), local_up=(0, 0, 1), local_right=(1, 0, 0))

    def make(integ):
        b = scene.SceneBuilder(Wp, Hp)
        s = b.settings
        s.aa_sampler, s.aa_samples, s.filter, s.filter_radius = abi.SAMPLER_UNIFORM, 1, abi.FILTER_BLOCK, 0
        b.add_mesh(p, [[0, 1, 2]], b.lambert(b.spectrum_const(0.5)))
        T = np.eye(4, dtype=np.float32)
        T[:3, 3] = eye
        b.set_camera(T, near=1e-6, **cam)
        return finish(b, integ, mono=True)
    y, x = np.meshgrid(np.arange(Hp, dtype=np.float64), np.arange(Wp, dtype=np.float64), indexing="ij")
    nx, ny = 2 * (x / Wp - 0.5), -2 * (y / Hp - 0.5)
    d = nx[..., None] * (0.5 * cam["width"]) * np.array([1.0, 0, 0]) + ny[..., None] * (0.5 * cam["height"]) * np.array([0, 0, 1.0]) + np.array([0, 1.0, 0])
    n = Wp * Hp
    org, direction = np.broadcast_to(np.asarray(eye, dtype=np.float32), (n, 3)).astype(np.float64), E._unit32(d.reshape(n, 3)).astype(np.float64)
    geo = X.Geometry(p.astype(np.float64)[None], [0], [0], extra_ulps=E.CAMERA_ULPS)
    cls = X.classify(org, direction, geo.tris, margin=geo.delta(org))
    tmin, tmax = np.full(n, 1e-6), np.full(n, np.inf)
    Q = X.qualifying(geo, cls, org, tmin, tmax)
    rays = cls.ray[Q]
    assert 0.2 * n < len(rays) < 0.9 * n and len(np.unique(rays)) == len(rays)

    a, v = render(make(("ao", 1))), render(make(("vf", "parameter", False)))
    hit = hits_of(v).reshape(-1)
    assert hit[rays].all() and not a.aoCounts().any()                                   # R1: every clear hit is reported
    assert hit.sum() - len(rays) <= 0.05 * hit.sum()                                    # ... and nearly every reported hit is a clear one
    w = np.unique(a.output()[0].reshape(n, 3)[hit])
    assert len(w) == 1
    w = float(w[0])
    t, u_, v_ = cls.t[Q], cls.u[Q], cls.v[Q]
    Mx = X.ray_extent(org, geo.extent)[rays]
    tau = X._tau(t, Mx)
    dt = tau + geo.slide(Mx, cls.sin_phi[Q])
    dpoint = geo.delta(org)[rays] + tau + dt
    r, g, bl = (float(s520(k)) for k in (abi.VF_COLOR_RED, abi.VF_COLOR_GREEN, abi.VF_COLOR_BLUE))
    want = w * (r * u_ + g * v_ + bl * t)
    room = w * (r * dpoint / 5.0 + g * dpoint / 4.0 + bl * dt)
    got = v.output()[0].reshape(n, 3)[rays]
    dev = np.abs(got[:, 0].astype(np.float64) - want)
    print("parameter: worst deviation %.3g of an allowed %.3g; largest share of the allowance %.3f" % (dev.max(), room.max(), (dev / (RTOL * want + room)).max()))
    assert (dev <= RTOL * np.abs(want) + room).all() and (got[:, 0] == got[:, 1]).all() and (got[:, 0] == got[:, 2]).all()
    assert room.max() < 1e-4 * want.max() and u_.max() - u_.min() > 0.3 and v_.max() - v_.min() > 0.3   # the allowance is small against what varies


# ---- 6: statistics ---------------------------------------------------------------------------------------------------------------------
def stats_scene(integ):
    b, white = H.builder(W, HGT, 0, EYE, TARGET, sampler=abi.SAMPLER_UNIFORM)   # no random numbers in the camera sample: `ao` and `vf` trace the same rays in every iteration
    H.quad(b, white, [[-2, -2, 0], [2, -2, 0], [2, 2, 0], [-2, 2, 0]], toward=EYE)
    for q in H.box_quads((-0.5, -0.5, 0.3), (0.5, 0.5, 1.0)):
        H.quad(b, white, q, away=(0, 0, 0.65))
    return finish(b, integ)


def test_statistics():
    iters = 3
    v, a = render(stats_scene(("vf", "colored_entity_id")), iters), render(stats_scene(("ao", 4)), iters)
    st, sa = v.statistics(), a.statistics()
    samples = W * HGT * iters
    hits = int(v.output()[1].sum())
    assert 0 < hits < samples and st["entity_hits"] == hits and st["background_hits"] == samples - hits
    assert st["entity_hits"] + st["background_hits"] == samples
    assert st["camera_depth"] == samples                       # every shading group, background ones included (visualfeedback.cpp:243)
    assert sa["camera_depth"] == hits                          # ... which `ao` does not (ambientocclusion.cpp:34)
    assert st["shadow_rays"] == 0 and st["bounce_rays"] == 0 and sa["shadow_rays"] == 4 * hits
    for key in ("camera_rays", "light_rays", "primary_rays", "monochrome_rays", "pixel_samples", "entity_hits", "background_hits", "light_depth"):
        assert st[key] == sa[key], key
    assert st["camera_rays"] == st["primary_rays"] == st["pixel_samples"] == samples
    tc = v.traceCounters()
    assert tc["rays_closest"] == samples and tc["rays_any"] == 0


# ---- 7: plumbing -----------------------------------------------------------------------------------------------------------------------
def plumbing_scene(mode="colored_primitive_id", **kw):
    b, white = H.builder(W, HGT, 0, EYE, TARGET, **kw)
    H.quad(b, white, [[-2, -2, 0], [2, -2, 0], [2, 2, 0], [-2, 2, 0]], toward=EYE)
    for q in H.box_quads((-0.5, -0.5, 0.3), (0.5, 0.5, 1.0)):
        H.quad(b, white, q, away=(0, 0, 0.65))
    return finish(b, ("vf", mode, True))


def test_determinism_and_chunking():
    a, b, c = render(plumbing_scene(), 5), render(plumbing_scene(), 5), render(plumbing_scene(), calls=[1] * 5)
    for other in (b, c):
        assert all(np.array_equal(x, y) for x, y in zip(a.output(), other.output()))
    assert a.output()[0].max() > 0 and a.output()[1].max() == 5 and a.pipelineInfo()["mode"] == 0


@pytest.mark.parametrize("filt,radius", [(abi.FILTER_BLOCK, 0), (abi.FILTER_MITCHELL, 1)])
def test_complementary_tiles_sum_to_the_frame(filt, radius):
    kw = dict(filt=filt, radius=radius)
    whole = render(plumbing_scene(**kw), 3)
    left = render(plumbing_scene(**kw), 3, tiles=[(0, 0, 33, HGT)])
    right = render(plumbing_scene(**kw), 3, tiles=[(33, 0, W, HGT)])
    total = left.output()[0] + right.output()[0]
    if radius == 0:
        assert np.array_equal(total, whole.output()[0])
    else:   # the bound tests/test_gpu_ao.py holds `ao` to
        rel = float(np.sqrt(((total.astype(np.float64) - whole.output()[0]) ** 2).sum()) / np.sqrt((whole.output()[0].astype(np.float64) ** 2).sum()))
        assert rel <= 1e-5, rel
    assert np.array_equal(left.output()[1] + right.output()[1], whole.output()[1]) and whole.output()[0].max() > 0


def test_both_bvh_widths_give_the_same_frame(monkeypatch):
    frames = []
    for width in ("4", "6"):
        monkeypatch.setenv("PRGPU_BVH_WIDTH", width)
        ctx = render(plumbing_scene("parameter"), 2)
        assert ctx.pipelineInfo()["bvh_width"] == int(width)
        frames.append(ctx.output())
    assert all(np.array_equal(x, y) for x, y in zip(*frames)) and frames[0][0].max() > 0


VF_PRC = """(scene :render_width 48 :render_height 32 :camera 'c'
  (sampler :slot 'aa' :type 'random' :sample_count 4) (filter :type 'block' :radius 0)
  (integrator :type 'visual_feedback' %s)
  (camera :name 'c' :type 'standard' :width 1 :height 0.667 :local_direction [0,0,-1] :local_up [0,1,0] :local_right [1,0,0] :transform [1,0,0,0, 0,1,0,0.6, 0,0,1,4, 0,0,0,1])
  (material :name 'm' :type 'diffuse' :albedo 0.8)
  (entity :name 'f' :type 'plane' :x_axis [6,0,0] :y_axis [0,0,-6] :centering true :materials 'm')
  (entity :name 's' :type 'sphere' :radius 0.6 :materials 'm' :transform [1,0,0,0, 0,1,0,0.9, 0,0,1,0, 0,0,0,1])
)"""


def test_a_vf_scene_file_renders_with_its_own_integrator():
    assert hasattr(backend.RenderContext, "enableVisualFeedback")
    sc = scene.PrcScene(source=VF_PRC % ":mode 'NdotV' :weighting false")   # no force_direct
    assert not sc.warnings and (sc.integrator, sc.vf_mode, sc.vf_weighting) == (abi.INTEGRATOR_VF, M["ndotv"], False)
    ctx = backend.RenderContext(sc, device=0)
    ctx.setTiming(True)
    ctx.render(2)
    ctx.waitForFinish()
    xyz, smp, fb = ctx.output()
    assert (ctx.vf_mode, ctx.vf_weighting) == (M["ndotv"], False) and ctx.pipelineInfo()["mode"] == 0
    assert np.isfinite(xyz).all() and xyz.max() > 0 and smp.max() == 2 and not fb.any() and not xyz[smp == 0].any()
    assert ctx.kernelTime("vf")[1] == 2 and ctx.kernelTime("ao")[1] == 0 and ctx.kernelTime("shade")[1] == 0
    ent = ctx.primaryHits()[0]
    assert set(np.unique(ent)) == {0, 1, abi.INVALID_ID}
    # a missing :mode is colored_entity_id: two entities, two colours (weighted by a cosine that varies over the sphere)
    d = render(scene.PrcScene(source=VF_PRC % ":weighting false"), 1)
    assert d.vf_mode == M["colored_entity_id"]
    x, e = d.output()[0], d.primaryHits()[0]
    assert len(np.unique(x[e == 0], axis=0)) > 1 and not x[e == abi.INVALID_ID].any()   # (full spectrum: the colour's XYZ follows the pixel's wavelengths)


# ---- 8: refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    lib = abi.load()
    ctx = backend.RenderContext(plumbing_scene(), device=0)
    with pytest.raises(abi.PrgpuError, match="error -4"):
        ctx.enableLPE(["C.*"])
    assert b"visual feedback" in lib.prgpu_last_error()
    ch = (abi.OutputChannel * 1)(abi.OutputChannel(0, abi.CHANNEL_SPECTRAL, 0, abi.TONE_SRGB, b"", b"C.*"))
    assert lib.prgpu_outputs_enable(ctx._h, ch, 1) == -4 and b"visual feedback" in lib.prgpu_last_error()
    assert lib.prgpu_enable_ambient_occlusion(ctx._h, 4) == -1 and b"visual feedback" in lib.prgpu_last_error()          # ao after vf
    assert lib.prgpu_enable_visual_feedback(ctx._h, M["inside"], 1) == -1 and b"already" in lib.prgpu_last_error()      # twice
    ctx.render(1)
    ctx.waitForFinish()
    assert ctx.output()[0].max() > 0

    b, white = H.builder(W, HGT, 0, EYE, TARGET)
    H.quad(b, white, [[-2, -2, 0], [2, -2, 0], [2, 2, 0], [-2, 2, 0]], toward=EYE)
    plain = b.build()
    d = backend.RenderContext(plain, device=0)
    for bad in (len(abi.VF_MODE_NAMES), 11, 0xFFFFFFFF):                                                                # outside the enum
        assert lib.prgpu_enable_visual_feedback(d._h, bad, 1) == -1 and b"mode" in lib.prgpu_last_error()
    d.render(1)
    assert lib.prgpu_enable_visual_feedback(d._h, M["inside"], 1) == -1 and b"before the first iteration" in lib.prgpu_last_error()

    a = backend.RenderContext(plain, device=0)
    a.enableAmbientOcclusion(4)
    assert lib.prgpu_enable_visual_feedback(a._h, M["inside"], 1) == -1 and b"ambient occlusion" in lib.prgpu_last_error()   # vf after ao
    with pytest.raises(abi.PrgpuError, match="error -1"):
        a.enableVisualFeedback("inside")

    e = backend.RenderContext(plain, device=0)
    e.enableLPE(["C.*"])
    assert lib.prgpu_enable_visual_feedback(e._h, M["inside"], 1) == -1 and b"light path expressions" in lib.prgpu_last_error()
