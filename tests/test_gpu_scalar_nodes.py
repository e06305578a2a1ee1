"""Scalar nodes on scalar material parameters (PRGPU_SPEC_SCALAR_IMAGE .. PRGPU_SPEC_SCALAR_COS, PRGPU_MATF_NODE_*; device/render.hip: scalar_image_eval,
scalar_run, scalar_resolve) on the GPU, checked without the CPU checker, which does not know them.  The harness is that of tests/test_gpu_image_texture.py
(the offset quad, its float64 uv, `frame`, `check`) and tests/test_gpu_mix_materials.py (the Oren-Nayar closed form).

1, 2  The value probe.  An Oren-Nayar quad with vertex normals, seen head-on by an orthographic camera under a constant environment of radiance 1, without next
      event estimation, depth limit 2, the `uniform` sampler, a block filter of radius 0, mono at 550 nm.  Head-on s is exactly 0, so the ratio of the frame to
      the frame of the same scene with a Lambert albedo of 1 is albedo (1 - 0.5 r / (r + 0.33) + 0.17 albedo r / (r + 0.13)), r = sigma^2 (orennayar.cpp:29-47;
      the third term is the interreflection share the material adds to A): the frame reads sigma^2 back.  With `:roughness` a scalar node every pixel is held
      to that closed form of the float64 restatement of the node at the ray's uv: 1e-5 relative + 1e-6 absolute -- the two frames differ by a dozen fp32
      roundings, |dA / d sigma| < 1, and a wrong texel, wrap, weight or operator is O(0.01) or more.  Pixels whose uv lies within 1e-3 texel of a texel
      boundary are left out (the uv of a hit is good to a few 1e-6); they must be at most 1 % of the quad's.
      The probe reads sigma^2: `neg` and `abs` alone could not be told from the identity, so they sit in two-operator trees where the sign matters.
3     The closures read the resolved value: a 2 x 2 `closest` texture on a quad that fills the film; each quadrant of the frame, sample counts included, equals
      bit for bit the same quadrant of the scene that holds that texel's number, the float32 k / 255 the reader produces (the two rows and two columns along the texel boundaries are left out: a sample
      is splatted where it lands, which may be the neighbouring pixel).
4     A Cornell-style box whose materials take 1 x 1 scalar textures renders the frame, the sample counts and the statistics of the box with the numbers, bit
      for bit, in every pipeline.
5     Such a scene runs the top row of the variant table; the one with numbers the row it always ran."""
import numpy as np
import pytest

import image_files as imf
import test_gpu_image_texture as ti
import test_gpu_mix_materials as tm
from pearray_amd import _cabi as abi
from pearray_amd import backend, scene

pytestmark = pytest.mark.gpu
F = np.float32
N = 64
WL = 550.0
ALBEDO = 0.5
RNG = np.random.RandomState(11)
GREY = {(4, 4): RNG.randint(0, 256, size=(4, 4, 1)), (5, 3): RNG.randint(0, 256, size=(3, 5, 1))}      # (W, H) -> [H, W, 1]
GREY[(4, 4)][1, 2] = 0
GREY[(4, 4)][2, 1] = 255
GREY[(4, 4)][0, 0], GREY[(4, 4)][3, 3] = 126, 129          # either side of one half: `round` tells them apart
SMOOTH = F(0.1) + F(0.7) * F(RNG.rand(4, 4))              # [0.1, 0.8]: every operator of the second test stays inside [0, 1] over it, or over ...
RAISED = F(1.0) + F(1.7) * F(RNG.rand(4, 4))              # ... [1, 2.7], for `log`


@pytest.fixture(scope="module")
def maps(tmp_path_factory):
    """{name: float32 [H, W] as prgpu_image_load_scalar returns it from a file written here}"""
    d = tmp_path_factory.mktemp("scalar_maps")
    out = {}
    for (w, h), s in GREY.items():
        out[(w, h, "png")] = scene.load_scalar_image(imf.write(d / ("g%dx%d.png" % (w, h)), imf.encode_png(s, 0, 8)))[0]
        out[(w, h, "pfm")] = scene.load_scalar_image(imf.write(d / ("g%dx%d.pfm" % (w, h)), imf.encode_pfm(F(s[:, :, 0]) / F(300.0), little=(w == 4))))[0]
        assert out[(w, h, "png")].shape == out[(w, h, "pfm")].shape == (h, w) and np.array_equal(out[(w, h, "png")], F(s[:, :, 0]) / F(255))
    for name, values in (("smooth", SMOOTH), ("negative", -SMOOTH), ("raised", RAISED)):
        out[name] = scene.load_scalar_image(imf.write(d / (name + ".pfm"), imf.encode_pfm(values)))[0]
        assert np.array_equal(out[name], values)
    return out


def probe_scene(material, extent=2.5, uv=(0.0, 1.0)):
    """ti.quad_scene's quad (offset from the film's grid by ti.DX, ti.DY, texture coordinates `uv` .. from corner to corner) with vertex normals and
    tm.quad_scene's settings (depth limit 2, no next event estimation, a constant environment) on an N x N film.  material(b) -> material index.
    Returns (builder, u, v, inside): the float64 texture coordinates under every pixel's ray."""
    b = scene.SceneBuilder(N, N)
    s = b.settings
    s.aa_sampler, s.aa_samples, s.filter, s.filter_radius, s.nee = abi.SAMPLER_UNIFORM, 1, abi.FILTER_BLOCK, 0, 0
    s.spectral_start = s.spectral_end = WL
    s.spectral_mono = 1
    s.max_ray_depth = 2
    b.environment_light(b.spectrum_const(1.0))
    x0, y0 = F(-1 + ti.DX), F(-1 + ti.DY)
    x1, y1 = F(x0 + F(2)), F(y0 + F(2))
    lo, hi = uv
    b.add_mesh([[x0, y0, 0], [x1, y0, 0], [x1, y1, 0], [x0, y1, 0]], [[0, 1, 2], [0, 2, 3]], material(b), normals=[[0, 0, 1]] * 4,
               uvs=[[lo, lo], [hi, lo], [hi, hi], [lo, hi]])
    gy, gx = np.meshgrid(np.arange(N, dtype=np.float64), np.arange(N, dtype=np.float64), indexing="ij")
    nx, ny = 2 * (gx / N - 0.5), -2 * (gy / N - 0.5)
    T = np.eye(4, dtype=F)
    T[2, 3] = 3.0
    b.set_camera(T, width=extent, height=extent, local_direction=(0, 0, -1), local_right=(1, 0, 0), local_up=(0, 1, 0), ortho=True)
    fu, fv = (0.5 * extent * nx - np.float64(x0)) / 2, (0.5 * extent * ny - np.float64(y0)) / 2
    inside = (fu > 0) & (fu < 1) & (fv > 0) & (fv < 1)
    return b, lo + (hi - lo) * fu, lo + (hi - lo) * fv, inside


_REFERENCE = {}


def probe(roughness, extent=2.5, uv=(0.0, 1.0)):
    """(ratio of the frame with Oren-Nayar roughness(b) to the albedo-1 Lambert frame, builder, u, v, on).  The Lambert frame is rendered once per set-up."""
    key = (extent, uv)
    if key not in _REFERENCE:
        _REFERENCE[key] = ti.frame(probe_scene(lambda b: b.lambert(b.spectrum_const(1.0)), extent, uv)[0])[:2]
    ref, ref_ent = _REFERENCE[key]
    b, u, v, inside = probe_scene(lambda b: b.oren_nayar(b.spectrum_const(ALBEDO), roughness(b)), extent, uv)
    got, ent, info = ti.frame(b)
    assert info["mode"] == 2 and info["kernel"] == "throughput" and info["variant"] == 5, info
    on = ent == 0
    assert np.array_equal(on, inside) and np.array_equal(ent, ref_ent) and on.sum() > 0.3 * N * N
    ch = int(np.argmax(ref[on].mean(0)))
    assert (ref[..., ch][on] > 0).all() and np.array_equal(got[~on], ref[~on])
    with np.errstate(all="ignore"):
        return np.where(on, got[..., ch] / ref[..., ch], 0.0), b, u, v, on


def closed_form(sigma):
    """albedo (A + B s / t) of orennayar.cpp:29-47 at s = 0, in float64, of the float64 sigma"""
    r2 = np.float64(sigma) ** 2
    a = np.float64(F(ALBEDO))
    return np.where(r2 > tm.EPS, a * (1 - 0.5 * r2 / (r2 + 0.33) + 0.17 * a * r2 / (r2 + 0.13)), a)


def decided(u, v, on, *grids):
    """the quad's pixels whose uv is at least 1e-3 texel away from every texel boundary of the (W, H) grids; the others are at most 1 % of them"""
    near = np.zeros(on.shape, bool)
    for w, h in grids:
        near |= imf.boundary_distance(u, v, w, h) < 1e-3
    print("within 1e-3 texel of a boundary: %d of %d pixels" % ((on & near).sum(), on.sum()))
    assert (on & near).sum() <= 0.01 * on.sum()
    return on & ~near


# ---- 1: the value of a scalar texture --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,kind", [(4, 4, "png"), (5, 3, "png"), (5, 3, "pfm"), (4, 4, "pfm")])
def test_closest_texel_values(maps, w, h, kind):
    values = maps[(w, h, kind)]
    got, b, u, v, on = probe(lambda b: b.scalar_image(values, "closest"))
    want = closed_form(imf.lookup_closest(np.float64(values), 0.0, u, v))
    assert len(np.unique(np.round(want[on], 5))) >= h * w // 2            # the frame tells texels apart
    ti.check("closest %dx%d %s" % (w, h, kind), got, want, decided(u, v, on, (w, h)))


@pytest.mark.parametrize("wrap", [("black", "black"), ("clamp", "clamp"), ("periodic", "periodic"), ("mirror", "mirror"), ("mirror", "clamp"), ("periodic", "black")])
def test_wrap_modes(maps, wrap):
    values = maps[(5, 3, "png")]
    got, b, u, v, on = probe(lambda b: b.scalar_image(values, "closest", wrap), extent=2.25, uv=(-1.0, 2.0))
    assert u[on].min() < -0.95 and u[on].max() > 1.95 and v[on].min() < -0.95 and v[on].max() > 1.95
    modes = tuple(scene.SceneBuilder.IMAGE_WRAPS[m] for m in wrap)
    sigma = imf.lookup_closest(np.float64(values), 0.0, u, v, modes)
    outside = on & ((u < 0) | (u > 1) | (v < 0) | (v > 1))
    assert outside.sum() > 4 * (on & ~outside).sum() and (wrap[0] != "black" or (sigma[on & (u < 0)] == 0.0).all())      # `black` is 0
    ti.check("wrap %s / %s" % wrap, got, closed_form(sigma), decided(u, v, on, (5, 3)))


@pytest.mark.parametrize("wrap,uv", [("black", (0.0, 1.0)), ("mirror", (-1.0, 2.0)), ("periodic", (-1.0, 2.0)), ("clamp", (-1.0, 2.0))])
def test_bilinear_blends_the_four_values_in_the_stated_order(maps, wrap, uv):
    """(v00 (1 - fx) + v10 fx)(1 - fy) + (v01 (1 - fx) + v11 fx) fy around s W - 0.5, every index wrapped on its own: no texel boundary decides anything,
    so no pixel is left out."""
    values = maps[(4, 4, "png")]
    got, b, u, v, on = probe(lambda b: b.scalar_image(values, "bilinear", wrap), extent=2.5 if uv[0] == 0 else 2.25, uv=uv)
    m = scene.SceneBuilder.IMAGE_WRAPS[wrap]
    sigma = imf.lookup_bilinear(np.float64(values), 0.0, u, v, (m, m))
    assert np.abs(closed_form(sigma)[on] - closed_form(imf.lookup_closest(np.float64(values), 0.0, u, v, (m, m)))[on]).max() > 0.02      # a closest lookup in its place fails
    ti.check("bilinear %s" % wrap, got, closed_form(sigma), on)


# ---- 2: the device operators ------------------------------------------------------------------------------------------------------------------------
C32 = lambda c: np.float64(F(c))
half_away = lambda x: np.sign(x) * np.floor(np.abs(x) + 0.5)
OPERATORS = {  # name -> (texture, tree(b, tex) -> ScalarNode, the same in float64 of the float64 texel value)
    "add": ("smooth", lambda b, t: b.scalar_op("add", t, 0.15), lambda x: x + C32(0.15)),
    "sub": ("smooth", lambda b, t: b.scalar_op("sub", t, 0.05), lambda x: x - C32(0.05)),
    "mul": ("smooth", lambda b, t: b.scalar_op("mul", t, 0.9), lambda x: x * C32(0.9)),
    "div": ("smooth", lambda b, t: b.scalar_op("div", t, 1.25), lambda x: x / C32(1.25)),
    "div, the texture below": ("raised", lambda b, t: b.scalar_op("div", 0.9, t), lambda x: C32(0.9) / x),
    "neg": ("smooth", lambda b, t: b.scalar_op("add", b.scalar_op("neg", t), 0.9), lambda x: -x + C32(0.9)),
    "abs": ("smooth", lambda b, t: b.scalar_op("add", b.scalar_op("abs", b.scalar_op("sub", t, 0.45)), 0.2), lambda x: np.abs(x - C32(0.45)) + C32(0.2)),
    "max": ("smooth", lambda b, t: b.scalar_op("max", t, 0.45), lambda x: np.maximum(x, C32(0.45))),
    "min": ("smooth", lambda b, t: b.scalar_op("min", t, 0.45), lambda x: np.minimum(x, C32(0.45))),
    "sqrt": ("smooth", lambda b, t: b.scalar_op("sqrt", t), np.sqrt),
    "pow": ("smooth", lambda b, t: b.scalar_op("pow", t, 1.7), lambda x: np.power(x, C32(1.7))),
    "floor": ((4, 4, "png"), lambda b, t: b.scalar_op("floor", t), np.floor),
    "ceil": ((4, 4, "png"), lambda b, t: b.scalar_op("ceil", t), np.ceil),
    "round": ((4, 4, "png"), lambda b, t: b.scalar_op("round", t), half_away),
    "exp": ("negative", lambda b, t: b.scalar_op("exp", t), np.exp),
    "log": ("raised", lambda b, t: b.scalar_op("log", t), np.log),
    "sin": ("smooth", lambda b, t: b.scalar_op("sin", t), np.sin),
    "cos": ("smooth", lambda b, t: b.scalar_op("cos", t), np.cos),
}


@pytest.mark.parametrize("name", sorted(OPERATORS))
def test_every_device_operator(maps, name):
    assert {n.split(",")[0] for n in OPERATORS} == {n for n, (k, _) in abi.SCALAR_OPS.items() if k is not None} - {"subtract", "multiply", "divide", "negate"}      # all 17
    key, tree, f64 = OPERATORS[name]
    values = maps[key]
    got, b, u, v, on = probe(lambda b: tree(b, b.scalar_image(values, "closest")))
    with np.errstate(all="ignore"):          # (off the quad the lookup is the black texel's 0)
        sigma = np.where(on, f64(imf.lookup_closest(np.float64(values), 0.0, u, v)), 0.0)
    assert sigma[on].min() >= 0.0 and sigma[on].max() <= 1.0 and len(np.unique(np.round(closed_form(sigma)[on], 5))) >= 2
    ti.check(name, got, closed_form(sigma), decided(u, v, on, values.shape[::-1]))


def test_a_tree_of_depth_three_over_two_textures(maps):
    """(mul (add T (min P 0.5)) (sqrt (sub 1 T))): T 4 x 4, P 5 x 3 bilinear; the right operand of the root needs the stack the left one does"""
    t_values, p_values = maps["smooth"], maps[(5, 3, "png")]

    def tree(b):
        t, p = b.scalar_image(t_values, "closest"), b.scalar_image(p_values, "bilinear", "clamp")
        return b.scalar_op("mul", b.scalar_op("add", t, b.scalar_op("min", p, 0.5)), b.scalar_op("sqrt", b.scalar_op("sub", 1.0, t)))
    got, b, u, v, on = probe(tree)
    t = imf.lookup_closest(np.float64(t_values), 0.0, u, v)
    p = imf.lookup_bilinear(np.float64(p_values), 0.0, u, v, (1, 1))
    sigma = (t + np.minimum(p, 0.5)) * np.sqrt(1.0 - t)
    assert sigma[on].min() >= 0.0 and sigma[on].max() <= 1.0
    ti.check("depth-3 tree", got, closed_form(sigma), decided(u, v, on, (4, 4)))


# ---- 3: the closures read the resolved value, bit for bit ------------------------------------------------------------------------------------------------
TEXELS = np.array([[26, 77], [128, 204]])          # k of k / 255, rows top-down
CLOSURES = {  # name -> material(b, value): value is a ScalarNode or the number
    "rough conductor": lambda b, x: b.rough_conductor(x, specularity=b.refl(0.9, 0.7, 0.4)),
    "rough dielectric": lambda b, x: b.rough_dielectric(x, ior=b.spectrum_const(1.5)),
    "principled roughness": lambda b, x: b.principled(base=b.refl(0.3, 0.5, 0.8), roughness=x, metallic=0.4, clearcoat=0.5),
    "roughness_x beside a numeric roughness_y": lambda b, x: b.rough_conductor(x, roughness_y=0.35),
    "principled metallic": lambda b, x: b.principled(base=b.refl(0.8, 0.5, 0.3), roughness=0.3, metallic=x, sheen=0.5),
}


def filled_film(material):
    """one quad [-1, 1]^2 that fills the film of an orthographic camera, alone under a constant environment: a pixel depends on its own first hit only;
    the texel boundaries u = v = 0.5 fall between pixels 31 and 32"""
    b = scene.SceneBuilder(N, N)
    s = b.settings
    s.aa_samples, s.filter, s.filter_radius, s.max_ray_depth = 4, abi.FILTER_BLOCK, 0, 4
    b.environment_light(b.illuminant_d65())
    b.add_mesh([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], [[0, 1, 2], [0, 2, 3]], material(b), normals=[[0, 0, 1]] * 4, uvs=[[0, 0], [1, 0], [1, 1], [0, 1]])
    T = np.eye(4, dtype=F)
    T[2, 3] = 3.0
    b.set_camera(T, width=2.0, height=2.0, local_direction=(0, 0, -1), local_right=(1, 0, 0), local_up=(0, 1, 0), ortho=True)
    ctx = backend.RenderContext(b.build(), device=0)
    ctx.start()
    ctx.waitForFinish()
    xyz, smp, fb = ctx.output()
    info = ctx.pipelineInfo()
    ctx.close()
    assert not (fb & 0x7).any()
    return np.asarray(xyz).reshape(N, N, 3), np.asarray(smp).reshape(N, N), info


@pytest.mark.parametrize("name", sorted(CLOSURES))
def test_the_closures_read_the_resolved_value_bit_for_bit(name):
    values = F(TEXELS) / F(255)
    xyz, smp, info = filled_film(lambda b: CLOSURES[name](b, b.scalar_image(values, "closest")))
    assert info["variant"] == 5 and np.isfinite(xyz).all() and xyz.max() > 0 and smp.max() == 4
    # a sample is splatted where it lands, up to half a pixel from its own pixel's centre: rows and columns 31 and 32 see both texels and are left out
    h = N // 2
    first = None
    for r in range(2):
        for c in range(2):
            ref_xyz, ref_smp, ref_info = filled_film(lambda b: CLOSURES[name](b, float(values[r, c])))
            assert ref_info["variant"] == 4                                                                     # 5: the row with numbers is the one it always was
            q = (slice(r * (h + 1), r * (h + 1) + h - 1), slice(c * (h + 1), c * (h + 1) + h - 1))
            assert np.array_equal(xyz[q], ref_xyz[q]) and np.array_equal(smp[q], ref_smp[q]), (name, r, c)
            if first is None:
                first = ref_xyz
            else:
                assert not np.array_equal(first[q], ref_xyz[q]), (name, r, c)                                   # the value matters to the closure


# ---- 4: uniform textures in every pipeline ----------------------------------------------------------------------------------------------------------------
def cornell(textured):
    """ti.cornell's box: its rough conductor, a rough glass, its principled card, an Oren-Nayar floor and a blend(Lambert, rough conductor) card take their
    scalars from 1 x 1 `closest` scalar textures, or are given the same float32 numbers"""
    b = scene.SceneBuilder(N, N)
    b.settings.aa_samples = 1
    b.settings.max_ray_depth = 8

    def scalar(k):   # wrap 'clamp': the box's corners are hit at u = 1 exactly, which `black` puts outside
        value = F(k) / F(255)
        return b.scalar_image(F([[value]]), "closest", "clamp") if textured else float(value)
    T = np.eye(4, dtype=F)
    T[:3, 3] = (0, -3.4, 1)
    b.set_camera(T, width=0.8, height=0.8, local_direction=(0, 1, 0), local_right=(1, 0, 0), local_up=(0, 0, 1))
    UV = [[0, 0], [1, 0], [1, 1], [0, 1]]

    def quad(p, mat, emission=None):
        b.add_mesh(p, [[0, 1, 2], [0, 2, 3]], mat, uvs=UV, emission=emission)
    grey, red, green = b.lambert(b.refl(0.7, 0.7, 0.7)), b.lambert(b.refl(0.7, 0.1, 0.1)), b.lambert(b.refl(0.1, 0.7, 0.1))
    quad([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], b.oren_nayar(b.refl(0.7, 0.7, 0.7), scalar(150)))      # floor
    quad([[-1, -1, 2], [-1, 1, 2], [1, 1, 2], [1, -1, 2]], grey)              # ceiling
    quad([[-1, 1, 0], [1, 1, 0], [1, 1, 2], [-1, 1, 2]], grey)                # back
    quad([[-1, -1, 0], [-1, 1, 0], [-1, 1, 2], [-1, -1, 2]], red)
    quad([[1, -1, 0], [1, -1, 2], [1, 1, 2], [1, 1, 0]], green)
    quad([[-0.3, -0.3, 1.98], [0.3, -0.3, 1.98], [0.3, 0.3, 1.98], [-0.3, 0.3, 1.98]], grey, emission=b.diffuse_emission(b.spectrum_const(12.0)))
    metal = b.rough_conductor(scalar(64), specularity=b.refl(0.95, 0.9, 0.8), roughness_y=scalar(110))
    disney = b.principled(base=b.refl(0.2, 0.3, 0.8), roughness=scalar(102), metallic=scalar(77), clearcoat=scalar(128), clearcoat_gloss=scalar(200), sheen=scalar(40))
    glass = b.rough_dielectric(scalar(51), ior=b.spectrum_const(1.5))
    card = b.blend(b.lambert(b.refl(0.8, 0.6, 0.2)), b.rough_conductor(scalar(90)), 0.4)
    quad([[-0.8, 0.6, 0.1], [-0.2, 0.8, 0.1], [-0.2, 0.8, 1.1], [-0.8, 0.6, 1.1]], metal)
    quad([[0.2, 0.8, 0.1], [0.8, 0.5, 0.1], [0.8, 0.5, 1.0], [0.2, 0.8, 1.0]], disney)
    quad([[-0.4, -0.2, 0.2], [0.4, -0.2, 0.2], [0.4, -0.1, 0.9], [-0.4, -0.1, 0.9]], glass)
    quad([[0.45, -0.5, 0.0], [0.9, -0.3, 0.0], [0.9, -0.3, 0.6], [0.45, -0.5, 0.6]], card)
    return b.build()


def test_uniform_textures_render_the_numeric_scene_bit_for_bit_in_every_pipeline(monkeypatch):
    """The second leg asks for the persistent kernel's latency organisation: the shipped build holds it for variant rows 1 and 4 only, so these scenes (top
    row: Oren-Nayar, blend) fall back to the throughput kernel there, as an image scene does."""
    ran = []
    for env in ti.PIPELINES:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        out = []
        for textured in (True, False):
            ctx = backend.RenderContext(cornell(textured), device=0)
            ctx.render(1)
            ctx.waitForFinish()
            out.append((ctx.output(), ctx.statistics(), ctx.pipelineInfo()))
            ctx.close()
        for k in env:
            monkeypatch.delenv(k)
        (a, sa, ia), (r, sr, ir) = out
        ran.append((ia["mode"], ia["kernel"], ir["kernel"]))
        assert all(np.array_equal(x, y) for x, y in zip(a, r)), env
        assert sa == sr and sa["shadow_rays"] > 1000 and sa["bounce_rays"] > 3000, (env, sa, sr)
        assert np.isfinite(a[0]).all() and a[0].max() > 0
    print("pipelines:", ran)
    assert len({m for m, _, _ in ran}) == 3 and ran[0][1] == "throughput"


# ---- 5: the variant row -------------------------------------------------------------------------------------------------------------------------------------
def test_a_scalar_node_scene_runs_the_top_row_and_a_numeric_one_the_row_it_ran():
    def info_of(material):
        b = scene.SceneBuilder(16, 16)
        b.settings.aa_samples = 1
        b.add_mesh([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], [[0, 1, 2], [0, 2, 3]], material(b), uvs=[[0, 0], [1, 0], [1, 1], [0, 1]],
                   emission=b.diffuse_emission(b.spectrum_const(1.0)))
        T = np.eye(4, dtype=F)
        T[2, 3] = 3.0
        b.set_camera(T, width=2.0, height=2.0, local_direction=(0, 0, -1), local_right=(1, 0, 0), local_up=(0, 1, 0))
        return ti.frame(b)[2]
    assert info_of(lambda b: b.rough_conductor(0.3))["variant"] == 4
    assert info_of(lambda b: b.rough_conductor(b.scalar_image(F([[0.3]]))))["variant"] == 5
    assert info_of(lambda b: b.rough_conductor(b.scalar_op("mul", b.scalar_image(F([[0.6]])), 0.5)))["variant"] == 5
    unused = lambda b: (b.scalar_image(F([[0.3]])), b.rough_conductor(0.3))[1]          # a node no material binds asks for nothing
    assert info_of(unused)["variant"] == 4
