"""The Oren-Nayar, null, blend and add materials (PRGPU_MAT_OREN_NAYAR .. PRGPU_MAT_ADD; device/render.hip: oren_nayar_calc, vertex_eval, shade_vertex)
on the GPU, checked against closed forms: the CPU checker does not know these materials.

Common set-up: one quad [-1, 1]^2 in the plane z = 0, with vertex normals (so that its tangent frame is orthonormal), under an orthographic camera, the `uniform` sampler, a block filter of radius 0 and a mono spectral
domain.  Every value is the RATIO of the frame to the frame of the same scene with a Lambert albedo of 1 (same seed, same random numbers), over the quad's
pixels.  Tolerance 1e-5 relative + 1e-6 absolute unless said otherwise: the two frames differ by a few dozen fp32 roundings of 6e-8 each, any error of
formula is at least 1e-2.

 1  Oren-Nayar eval: one distant light, next event estimation, depth limit 1, a view 45 degrees off the normal and three light directions off the view's
    plane: s > 0 with t = NdotL, s > 0 with t = NdotV, s < 0 with t = 1.  The ratio is albedo (A + B s / t) in float64 from the known V and L.
 2  Oren-Nayar sample, head-on, constant environment, no next event estimation, depth limit 2: s is exactly 0, every pixel is albedo A.
 3  ... at 45 degrees: the mean over the quad against a float64 quadrature, within 6 standard errors.  The variance is at most (range / 2)^2 with
    range = B albedo (1 + sin 45): s / t lies in [-sin 45, 1].  6 standard errors must stay below a third of the distance between the quadrature with and
    without the B term; both are proportional to B albedo, so the condition is N >= (9 (1 + sin 45) / d)^2 with d = that distance / (B albedo) = 0.0488:
    N >= 89 500.  A 64 x 64 film wholly on the quad at 16 samples per pixel has 65 536, so this test takes 32 (N = 131 072).
 4  Blend and add eval in the set-up of 1: (1 - f) a + f b resp. a + b for two Lambert children (f = 1.7 is clamped to 1), with an Oren-Nayar child, and with
    a delta-only first child (mirror, null): f b resp. b.
 5  Blend and add sample in the set-up of 2, one sample per pixel: every pixel is (1 - f) a or f b (add: a or b), and the share of the first value is within
    6 binomial standard deviations of 1 - f (add: 0.5): 0.043 for f = 0.3 and 4096 pixels.
 6  Null: a null quad between the camera and the Lambert quad, depth limit 3, gives the frame of the scene without it to 1e-6 relative.  (The null quad is
    0.12 wide and 100 above the other: a bounce ray that came back up through it would need a fourth vertex; 3e-7 of them do.)  blend(null, Lambert a, f)
    alone: pixels are (1 - f) 1, straight through to the environment, or f a.
 7  Every pipeline renders a Cornell box that uses all four kinds, a blend with a principled child and one with a glass child, to the same frame, bit for bit.
 8  Light path expressions: the planes of diffuse reflection and specular transmission / reflection sum to the main plane in the scenes of 5 and 6.

Nested combinators (a blend or add as a child) are refused by name; no test pins that refusal, on purpose (tests/test_mix_material_loader.py)."""
import numpy as np
import pytest

import image_files as imf
from pearray_amd import _cabi as abi
from pearray_amd import backend, scene

pytestmark = pytest.mark.gpu
F = np.float32
WAVELENGTHS = (450.0, 550.0, 650.0)
EPS = 1.1920929e-07                                   # PR_EPSILON
S45 = float(np.sin(np.pi / 4))
A_RGB, B_RGB = (0.8, 0.45, 0.2), (0.15, 0.35, 0.75)   # two `refl` colours whose spectra differ at every wavelength used here
LIGHTS = {"t is NdotL": (0.4, 0.3, 0.866), "t is NdotV": (0.7, 0.5, 0.51), "s is negative": (-0.5, 0.6, 0.62)}


def unit32(v):
    """the fp32 vector the scene holds, normalised in float64"""
    v = np.float64(F(v))
    return v / np.linalg.norm(v)


def quad_scene(n, wl, material, tilt=0.0, light=None, depth=2, spp=1, extent=2.5, null_in_front=False):
    """material(b) -> material index of the quad.  light: a direction = one distant light with next event estimation, None = a constant environment of
    radiance 1 without it.  tilt: the angle between the view and the normal, in the xz plane.  Returns the builder."""
    b = scene.SceneBuilder(n, n)
    s = b.settings
    s.aa_sampler, s.aa_samples, s.filter, s.filter_radius = abi.SAMPLER_UNIFORM, spp, abi.FILTER_BLOCK, 0
    s.spectral_start = s.spectral_end = wl
    s.spectral_mono = 1
    s.max_ray_depth = depth
    if light is None:
        s.nee = 0
        b.environment_light(b.spectrum_const(1.0))
    else:
        s.nee = 1
        b.distant_light(b.spectrum_const(1.0), direction=tuple(float(x) for x in light))
    mat = material(b)
    up = [[0, 0, 1]] * 4          # vertex normals: the tangent frame of a mesh WITHOUT them is two edges of the triangle (mesh.cpp:229-250), not orthogonal
    b.add_mesh([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], [[0, 1, 2], [0, 2, 3]], mat, normals=up)
    if null_in_front:
        h = 0.06
        b.add_mesh([[-h, -h, 100], [h, -h, 100], [h, h, 100], [-h, h, 100]], [[0, 1, 2], [0, 2, 3]], b.null(), normals=up)
    sn, cs = float(F(np.sin(tilt))), float(F(np.cos(tilt)))
    T = np.eye(4, dtype=F)
    T[:3, 3] = (103.0 * sn, 0.0, 103.0 * cs)          # the camera sits on the side of +x and looks back along (-sin, 0, -cos)
    b.set_camera(T, width=extent, height=extent, local_direction=(-sn, 0.0, -cs), local_right=(cs, 0.0, -sn), local_up=(0.0, 1.0, 0.0), ortho=True)
    return b


def view_vector(tilt):
    return unit32((float(F(np.sin(tilt))), 0.0, float(F(np.cos(tilt)))))


def frame(b, lpe=None):
    ctx = backend.RenderContext(b.build(), device=0)
    if lpe:
        ctx.enableLPE(lpe)
    ctx.start()
    ctx.waitForFinish()
    xyz, smp, fb = ctx.output()
    ent = ctx.primaryHits()[0].reshape(ctx.height, ctx.width)
    info = ctx.pipelineInfo()
    planes = [np.float64(ctx.lpe(k)) for k in range(len(lpe or []))]
    ctx.close()
    assert not (fb & 0x7).any(), "NaN / Inf / negative feedback bits"
    return np.float64(xyz), ent, info, planes


_REFERENCE = {}


def reference(n, wl, **kw):
    """the frame with a Lambert albedo of 1: computed once per set-up and left unchanged"""
    key = (n, wl, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _REFERENCE:
        _REFERENCE[key] = frame(quad_scene(n, wl, lambda b: b.lambert(b.spectrum_const(1.0)), **kw))[:2]
    return _REFERENCE[key]


def ratio(n, wl, material, lpe=None, top_variant=True, **kw):
    """(ratio to the albedo-1 frame [n, n], mask of the quad's pixels, builder, expression planes as ratios)"""
    ref, ref_ent = reference(n, wl, **{k: v for k, v in kw.items() if k != "null_in_front"})
    b = quad_scene(n, wl, material, **kw)
    got, ent, info, planes = frame(b, lpe)
    assert info["mode"] == 2 and info["kernel"] == "throughput" and info["variant"] == (5 if top_variant else info["variant"]), info
    on = ref_ent == 0
    assert on.sum() > 0.3 * n * n and np.array_equal(ent != abi.INVALID_ID, on)
    ch = int(np.argmax(ref[on].mean(0)))
    assert (ref[..., ch][on] > 0).all()
    with np.errstate(all="ignore"):
        return np.where(on, got[..., ch] / ref[..., ch], 0.0), on, b, [np.where(on, p[..., ch] / ref[..., ch], 0.0) for p in planes]


def check(label, got, want, on, rtol=1e-5, atol=1e-6):
    want = np.broadcast_to(np.float64(want), got.shape)
    err = np.abs(got - want)[on]
    room = (rtol * np.abs(want) + atol)[on]
    print("%s: %d pixels, worst deviation %.3g (allowed there %.3g), values %.6g .. %.6g" % (label, on.sum(), err.max(), room[err.argmax()], want[on].min(), want[on].max()))
    assert (err <= room).all(), (label, float((err / room).max()))


def same(a, b):
    """expression planes against the main plane: the same fragments, folded by the same arithmetic; 1e-6 relative leaves room for nothing but roundings"""
    return bool((np.abs(a - b) <= 1e-6 * np.abs(b)).all())


def albedo_at(b, spectrum, wl):
    """the value of a (refl r g b) node at `wl`, as the device evaluates it (fp32)"""
    s = b.spectra[spectrum]
    assert s.kind == abi.SPEC_PARAMETRIC
    return float(imf.upsample32(np.array([s.p[0], s.p[1], s.p[2]], F), wl))


def oren_nayar(albedo, sigma, V, L):
    """OrenNayarMaterial::calc (orennayar.cpp:29-47) in float64; V, L unit vectors in the frame of the normal +z"""
    r2 = np.float64(F(sigma)) ** 2
    if not r2 > EPS:
        return albedo
    ndl, ndv = max(0.0, L[2]), V[2]
    s = -ndl * ndv + float(np.dot(V, L))
    t = 1.0 if s < EPS else max(ndl, ndv)
    A = 1 - 0.5 * r2 / (r2 + 0.33) + 0.17 * albedo * r2 / (r2 + 0.13)
    B = 0.45 * r2 / (r2 + 0.09)
    return albedo * (A + B * s / t)


# ---- 1: Oren-Nayar, next event estimation ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wl", WAVELENGTHS)
@pytest.mark.parametrize("case", sorted(LIGHTS))
def test_oren_nayar_eval(case, wl):
    V, L = view_vector(np.pi / 4), unit32(LIGHTS[case])
    s = -L[2] * V[2] + float(np.dot(V, L))
    assert {"t is NdotL": s > 0.1 and L[2] > V[2] + 0.1, "t is NdotV": s > 0.1 and L[2] < V[2] - 0.1, "s is negative": s < -0.1}[case]
    for sigma in (0.0, 0.5, 1.0):
        node = {}

        def material(b):
            node["albedo"] = b.refl(*A_RGB)
            return b.oren_nayar(node["albedo"], sigma)
        got, on, b, _ = ratio(32, wl, material, tilt=np.pi / 4, light=LIGHTS[case], depth=1)
        a = albedo_at(b, node["albedo"], wl)
        want = oren_nayar(a, sigma, V, L)
        check("oren-nayar eval, %s, sigma %g, %g nm" % (case, sigma, wl), got, want, on)


# ---- 2: Oren-Nayar, sampled, head-on -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.0, 0.5, 1.0])
def test_oren_nayar_sample_head_on(sigma):
    node = {}

    def material(b):
        node["albedo"] = b.refl(*A_RGB)
        return b.oren_nayar(node["albedo"], sigma)
    got, on, b, _ = ratio(32, 550.0, material)
    a = albedo_at(b, node["albedo"], 550.0)
    r2 = np.float64(F(sigma)) ** 2
    A = 1 - 0.5 * r2 / (r2 + 0.33) + 0.17 * a * r2 / (r2 + 0.13)
    assert sigma == 0.0 or abs(A - 1) > 0.05
    check("oren-nayar sample head-on, sigma %g" % sigma, got, a * A, on)


# ---- 3: Oren-Nayar, sampled, oblique -------------------------------------------------------------------------------------------------------------------
def oren_nayar_quadrature(albedo, sigma, V, with_b, n=1024):
    """the integral of albedo (A + B s / t) cos / pi over the upper hemisphere: midpoint rule in (cos^2, phi), where cos / pi is the measure"""
    u = (np.arange(n) + 0.5) / n
    U, P = np.meshgrid(u, 2 * np.pi * u, indexing="ij")
    ct, st = np.sqrt(U), np.sqrt(1 - U)
    L = np.stack([st * np.cos(P), st * np.sin(P), ct], -1)
    r2 = np.float64(F(sigma)) ** 2
    s = -ct * V[2] + L @ V
    t = np.where(s < EPS, 1.0, np.maximum(ct, V[2]))
    A = 1 - 0.5 * r2 / (r2 + 0.33) + 0.17 * albedo * r2 / (r2 + 0.13)
    B = 0.45 * r2 / (r2 + 0.09)
    return float((albedo * (A + (B * s / t if with_b else 0.0 * s))).mean()), B


def test_oren_nayar_sample_oblique():
    sigma, n, spp = 1.0, 64, 32
    node = {}

    def material(b):
        node["albedo"] = b.refl(*A_RGB)
        return b.oren_nayar(node["albedo"], sigma)
    got, on, b, _ = ratio(n, 550.0, material, tilt=np.pi / 4, spp=spp, extent=1.3)
    assert on.all()
    a = albedo_at(b, node["albedo"], 550.0)
    V = view_vector(np.pi / 4)
    full, B = oren_nayar_quadrature(a, sigma, V, True)
    without = oren_nayar_quadrature(a, sigma, V, False)[0]
    assert abs(full - oren_nayar_quadrature(a, sigma, V, True, 512)[0]) < 1e-5
    N = n * n * spp
    se = 0.5 * B * a * (1 + S45) / np.sqrt(N)
    print("oren-nayar sample oblique: mean %.6f, quadrature %.6f (without the B term %.6f), N = %d, 6 standard errors %.6f, a third of the distance %.6f"
          % (got.mean(), full, without, N, 6 * se, abs(full - without) / 3))
    assert 6 * se <= abs(full - without) / 3
    assert abs(got.mean() - full) <= 6 * se


# ---- 4: blend and add, next event estimation ---------------------------------------------------------------------------------------------------------------
def two_children(first, second, combine):
    """material(b) for ratio(): first(b), second(b) -> (material index, value(wl, b) in float64); combine(b, m1, m2) -> the quad's material"""
    made = {}

    def material(b):
        made["1"], made["2"] = first(b), second(b)
        return combine(b, made["1"][0], made["2"][0])
    return material, made


def lambert(rgb):
    def make(b):
        node = b.refl(*rgb)
        return b.lambert(node), lambda wl, b: albedo_at(b, node, wl)
    return make


def rough_diffuse(rgb, sigma, V, L):
    def make(b):
        node = b.refl(*rgb)
        return b.oren_nayar(node, sigma), lambda wl, b: oren_nayar(albedo_at(b, node, wl), sigma, V, L)
    return make


NEE = dict(tilt=np.pi / 4, light=LIGHTS["t is NdotL"], depth=1)


@pytest.mark.parametrize("wl", WAVELENGTHS)
@pytest.mark.parametrize("f", [0.0, 0.3, 1.0, 1.7])
def test_blend_eval_of_two_lambert_children(f, wl):
    material, made = two_children(lambert(A_RGB), lambert(B_RGB), lambda b, m1, m2: b.blend(m1, m2, f))
    got, on, b, _ = ratio(32, wl, material, **NEE)
    a, c = made["1"][1](wl, b), made["2"][1](wl, b)
    assert abs(a - c) > 0.05
    fc = min(1.0, max(0.0, float(F(f))))
    check("blend eval f %g at %g nm" % (f, wl), got, (1 - fc) * a + fc * c, on)


@pytest.mark.parametrize("wl", WAVELENGTHS)
def test_add_eval_of_two_lambert_children(wl):
    material, made = two_children(lambert(A_RGB), lambert(B_RGB), lambda b, m1, m2: b.add(m1, m2))
    got, on, b, _ = ratio(32, wl, material, **NEE)
    check("add eval at %g nm" % wl, got, made["1"][1](wl, b) + made["2"][1](wl, b), on)


@pytest.mark.parametrize("kind", ["blend", "add"])
def test_eval_with_an_oren_nayar_child(kind):
    V, L = view_vector(np.pi / 4), unit32(NEE["light"])
    f = 0.3
    material, made = two_children(lambert(A_RGB), rough_diffuse(B_RGB, 0.5, V, L), lambda b, m1, m2: b.blend(m1, m2, f) if kind == "blend" else b.add(m1, m2))
    got, on, b, _ = ratio(32, 550.0, material, **NEE)
    a, c = made["1"][1](550.0, b), made["2"][1](550.0, b)
    ff = float(F(f))
    check(kind + " eval with an oren-nayar child", got, (1 - ff) * a + ff * c if kind == "blend" else a + c, on)


@pytest.mark.parametrize("kind", ["blend", "add"])
@pytest.mark.parametrize("delta", ["mirror", "null"])
def test_eval_with_a_delta_only_first_child(delta, kind):
    def first(b):
        return (b.mirror() if delta == "mirror" else b.null()), None
    f = 0.3
    material, made = two_children(first, lambert(B_RGB), lambda b, m1, m2: b.blend(m1, m2, f) if kind == "blend" else b.add(m1, m2))
    got, on, b, _ = ratio(32, 550.0, material, **NEE)
    c = made["2"][1](550.0, b)
    check("%s eval, %s first" % (kind, delta), got, float(F(f)) * c if kind == "blend" else c, on)


# ---- 5, 8: blend and add, sampled -----------------------------------------------------------------------------------------------------------------------------
def two_valued(label, got, on, first, second, p_first):
    """every pixel of `on` is `first` or `second` (1e-5 relative + 1e-6); the share of `first` is within 6 binomial standard deviations of p_first"""
    assert abs(first - second) > 0.01
    is_first = np.abs(got - first) <= 1e-5 * abs(first) + 1e-6
    is_second = np.abs(got - second) <= 1e-5 * abs(second) + 1e-6
    N = int(on.sum())
    share = is_first[on].mean()
    room = 6 * np.sqrt(p_first * (1 - p_first) / N)
    print("%s: %d pixels, values %.6g / %.6g, share of the first %.4f (expected %.4f, allowed +- %.4f), other values: %d" % (label, N, first, second, share, p_first, room, (on & ~is_first & ~is_second).sum()))
    assert (is_first | is_second)[on].all(), label
    assert abs(share - p_first) <= room, label
    return is_first


LPE_PLANES = ["C<R,D>L", "C<T,S>L", "C<R,S>L"]


@pytest.mark.parametrize("kind,f", [("blend", 0.3), ("blend", 0.75), ("add", None)])
def test_sampling_picks_one_child_per_vertex(kind, f):
    material, made = two_children(lambert(A_RGB), lambert(B_RGB), lambda b, m1, m2: b.blend(m1, m2, f) if kind == "blend" else b.add(m1, m2))
    got, on, b, planes = ratio(64, 550.0, material, extent=1.3, lpe=LPE_PLANES)
    assert on.all() and on.sum() == 4096
    a, c = made["1"][1](550.0, b), made["2"][1](550.0, b)
    if kind == "blend":
        ff = float(F(f))
        two_valued("blend sample f %g" % f, got, on, (1 - ff) * a, ff * c, 1 - ff)
    else:
        two_valued("add sample", got, on, a, c, 0.5)
    # 8: both children scatter by diffuse reflection
    assert same(planes[0], got) and not planes[1].any() and not planes[2].any()


# ---- 6, 8: null ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_null_surface_passes_the_ray_on():
    kw = dict(depth=3, extent=0.1)
    ref, ref_ent = reference(64, 550.0, **kw)
    got, ent, info, planes = frame(quad_scene(64, 550.0, lambda b: b.lambert(b.spectrum_const(1.0)), null_in_front=True, **kw), lpe=["C<T,S><R,D>L", "C<R,D>L"])
    assert info["variant"] == 5 and (ref_ent == 0).all() and (ent == 1).all()          # every camera ray meets the null quad first
    err = np.abs(got - ref)
    print("null in front: worst relative deviation %.3g" % (err / np.maximum(np.abs(ref), 1e-30)).max())
    assert ref.min() > 0 and (err <= 1e-6 * np.abs(ref)).all()
    assert same(planes[0], got) and not planes[1].any()                        # 8: specular transmission, then diffuse reflection


@pytest.mark.parametrize("f", [0.3, 0.6])
def test_blend_of_null_and_lambert_is_a_cut_out(f):
    def first(b):
        return b.null(), None
    material, made = two_children(first, lambert(A_RGB), lambda b, m1, m2: b.blend(m1, m2, f))
    got, on, b, planes = ratio(64, 550.0, material, depth=3, extent=1.3, lpe=LPE_PLANES)
    assert on.all()
    ff = float(F(f))
    through = two_valued("blend(null, lambert) f %g" % f, got, on, 1 - ff, ff * made["2"][1](550.0, b), 1 - ff)
    # 8: the planes partition the main plane: straight through is specular transmission, the rest diffuse reflection
    assert same(planes[0] + planes[1] + planes[2], got) and not planes[2].any()
    assert np.array_equal(planes[1] != 0, through) and np.array_equal(planes[0] != 0, ~through)


# ---- 7: every pipeline ------------------------------------------------------------------------------------------------------------------------------------------------
PIPELINES = [dict(PRGPU_MODE="persistent", PRGPU_PP_KERNEL="throughput"), dict(PRGPU_MODE="persistent", PRGPU_PP_KERNEL="latency"), dict(PRGPU_MODE="lockstep"),
             dict(PRGPU_MODE="streaming")]


def cornell():
    """The Cornell box with an Oren-Nayar floor and back wall, a cut-out ceiling, an add of paint and metal on one wall, a blend with a principled child and a
    blend with a glass child on the boxes, and a null material that nothing uses.  The glass has a constant index: behind a Sellmeier index the path collapses
    to its hero wavelength, and next event estimation on such a path is flagged NaN and dropped (direct.cpp:321) with or without a blend"""
    b = scene.SceneBuilder(64, 64)
    b.settings.aa_sampler, b.settings.aa_samples = abi.SAMPLER_MJITT, 4
    b.settings.max_ray_depth = 8

    def paint(rgb):
        return lambda bb: bb.lambert(bb.refl(*rgb))
    over = {
        "floor": lambda bb: bb.oren_nayar(bb.refl(0.7, 0.7, 0.7), 0.6),
        "backWall": lambda bb: bb.oren_nayar(bb.checkerboard(bb.refl(0.7, 0.7, 0.7), bb.refl(0.2, 0.2, 0.6), 4.0), 1.0),
        "ceiling": lambda bb: bb.blend(bb.null(), paint((0.7, 0.7, 0.7))(bb), 0.8),
        "leftWall": lambda bb: bb.add(paint((0.5, 0.1, 0.1))(bb), bb.rough_conductor(0.3, specularity=bb.spectrum_const(0.4))),
        "shortBox": lambda bb: bb.blend(paint((0.2, 0.6, 0.3))(bb), bb.principled(base=bb.refl(0.3, 0.4, 0.8), roughness=0.4, metallic=0.3, clearcoat=0.5), 0.4),
        "tallBox": lambda bb: bb.blend(bb.dielectric(bb.spectrum_const(1.5)), bb.oren_nayar(bb.refl(0.8, 0.8, 0.3), 0.5), 0.5),
    }
    scene._cornell_into(b, material_override=over)
    b.null()
    return b.build()


def test_every_pipeline_renders_the_same_frame(monkeypatch):
    """The second leg asks for the latency organisation: the shipped build holds it for variant rows 1 and 4 only (Makefile, PL_VARIANTS), so this scene (top
    row) falls back to the throughput kernel there."""
    out = []
    for env in PIPELINES:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ctx = backend.RenderContext(cornell(), device=0)
        ctx.start()
        ctx.waitForFinish()
        out.append((ctx.output(), ctx.statistics(), ctx.pipelineInfo()))
        ctx.close()
        for k in env:
            monkeypatch.delenv(k)
    (xyz, smp, fb), stats, info = out[0]
    print("pipelines:", [(i["mode"], i["kernel"], i["variant"]) for _, _, i in out], stats)
    assert info["mode"] == 2 and info["kernel"] == "throughput" and len({i["mode"] for _, _, i in out}) == 3
    assert all(i["variant"] == 5 for _, _, i in out)
    assert np.isfinite(xyz).all() and xyz.max() > 0 and not (fb & 0x7).any()
    assert stats["shadow_rays"] > 1000 and stats["bounce_rays"] > 3000
    for (o, st, i), env in zip(out[1:], PIPELINES[1:]):
        assert all(np.array_equal(x, y) for x, y in zip(o, (xyz, smp, fb))), env
        assert st == stats, (env, st, stats)
