"""Spectral expression nodes (PRGPU_SPEC_ADD .. PRGPU_SPEC_PEAK, include/prgpu.h; device/render.hip expr_eval) on the GPU, checked without the CPU
checker, which does not know them.

Values: the quad harness of tests/test_gpu_image_texture.py -- a 16 x 16 film, an orthographic camera over one quad, a constant environment, no next
event estimation, a mono spectral domain: the frame over the frame of the same scene with albedo 1 is the albedo, here an expression, restated in numpy
float32 in the reference's operand order.  Tolerance 1e-5 relative + 1e-6 absolute, the project's own for this harness (DESIGN.md sections 2.6, 2.7): the
two renders differ by about a dozen fp32 roundings, a wrong operand order or formula is O(0.1).  Worst measured deviation: DESIGN.md section 2.8.

As a light the expression is an environment's or an emission's radiance; in hero mode the blackbody is held against a 1 nm table of its own float64 values,
and the default `spd` mapper (whose histogram the HOST evaluator fills) against the `random` one.  Every pipeline renders a Cornell-style scene whose
spectra are all wrapped in exact identities to the frame, bit for bit, of the plain scene."""
import numpy as np
import pytest

import image_files as imf
from test_gpu_image_texture import DX, DY, PIPELINES, check, frame, quad_scene, textured_over_plain
from test_spectral_expr_loader import T_LIGHT, half_blackbody_table, interpolation_bound
from pearray_amd import _cabi as abi
from pearray_amd import backend, scene

pytestmark = pytest.mark.gpu
F = np.float32
WAVELENGTHS = (450.0, 550.0, 650.0)
N, EXTENT = 16, 2.5
RGB_A, RGB_B = (0.8, 0.7, 0.9), (0.3, 0.2, 0.4)          # A in about (0.65, 0.95), B in about (0.15, 0.45): A > B everywhere (asserted)


# ---- the reference, restated: fp32, the operand order of SpectralMathNode.cpp:67-96,128,188-194 --------------------------------------------------
def op32(name, a, b=None, p0=None, p1=None):
    one, two, half = F(1), F(2), F(0.5)
    if name == "smul": return a * b
    if name == "sadd": return a + b
    if name == "ssub": return a - b
    if name == "sdiv": return a / b
    if name == "sneg": return -a
    if name == "sabs": return np.abs(a)
    if name == "smax": return np.maximum(a, b)
    if name == "smin": return np.minimum(a, b)
    if name == "sburn": return one - (one - a) / (b + one)
    if name == "sscreen": return one - (one - a) * (one - b)
    if name == "sdodge": return a / ((one - b) + one)
    if name == "soverlay": return a * (a + two * b * (one - a))
    if name == "ssoftlight": return ((one - a) * b + (one - (one - a) * (one - b))) * a
    if name == "shardlight": return np.where(b <= half, two * b * a, one - (one - two * (b - half)) * (one - a))
    if name == "sblend": return a * (one - F(p0)) + b * F(p0)
    if name == "sbrightnesscontrast": return np.maximum((one + F(p1)) * a + (F(p0) - F(p1) * half), F(0))
    raise KeyError(name)


def planck64(wl_nm, t):
    c, h, kb = 299792458.0, 6.62607004081e-34, 1.3806485279e-23
    lam = np.float64(wl_nm) * 1e-9
    return (2 * h * c * c / lam ** 5) / np.expm1(h * c / (kb * lam * t))


def blackbody32(wl, t):
    """the node's fp32 value: float(Planck in double at the fp32 wavelength) times the fp32 normalisation 1 / float(Planck at Wien's peak)"""
    nm = np.float64(F(wl) * F(1e-9)) * 1e9
    norm = F(1) / F(planck64(np.float64(F(F(2.897771955e6) / F(t)) * F(1e-9)) * 1e9, float(F(t))))
    return F(planck64(nm, float(F(t)))) * norm


def refl32(rgb, wl):
    return imf.upsample32(np.array(scene.rgb_to_coeffs(rgb), F)[None, :], wl)[0]


class Expr:
    """An expression written once: built into a SceneBuilder and evaluated in numpy float32.  ("refl", rgb) | ("const", v) | ("peak", w, r) | ("blackbody", T) |
    (operator name, operands ..., [parameters])"""

    def __init__(self, tree):
        self.tree = tree

    def build(self, b, tree=None, memo=None):
        tree = self.tree if tree is None else tree
        memo = {} if memo is None else memo
        if id(tree) in memo:            # the same tuple object twice: one node, used twice
            return memo[id(tree)]
        head = tree[0]
        if head == "refl":
            node = b.refl(*tree[1])
        elif head == "const":
            node = b.spectrum_const(tree[1])
        elif head == "peak":
            node = b.spectrum_peak(tree[1], tree[2])
        elif head == "blackbody":
            node = b.spectrum_blackbody(tree[1])
        elif head == "sblend":
            x, y = self.build(b, tree[2], memo), self.build(b, tree[3], memo)
            node = b.spectrum_op(head, tree[1], x, y)
        elif head == "sbrightnesscontrast":
            node = b.spectrum_op(head, self.build(b, tree[1], memo), tree[2], tree[3])
        else:
            node = b.spectrum_op(head, *[self.build(b, t, memo) for t in tree[1:]])
        memo[id(tree)] = node
        return node

    def value(self, wl, tree=None):
        tree = self.tree if tree is None else tree
        head = tree[0]
        if head == "refl": return refl32(tree[1], wl)
        if head == "const": return F(tree[1])
        if head == "peak": return np.maximum(F(0), F(1) - np.abs(F(wl) - F(tree[1])) / F(tree[2]))
        if head == "blackbody": return blackbody32(wl, tree[1])
        if head == "sblend": return op32(head, self.value(wl, tree[2]), self.value(wl, tree[3]), p0=tree[1])
        if head == "sbrightnesscontrast": return op32(head, self.value(wl, tree[1]), p0=tree[2], p1=tree[3])
        return op32(head, *[self.value(wl, t) for t in tree[1:]])


A, B = ("refl", RGB_A), ("refl", RGB_B)


def c(v):
    return ("const", v)


BINARY = ["smul", "sadd", "ssub", "sdiv", "smax", "smin", "sburn", "sscreen", "sdodge", "soverlay", "ssoftlight", "shardlight"]
NON_COMMUTATIVE = ["ssub", "sdiv", "sburn", "sdodge", "soverlay", "ssoftlight", "shardlight"]
# two refl operands (sdiv with the smaller one on top, so that the value stays below 1.5; the unary ones on a difference, whose sign they show)
ON_TWO = {name: (name, B, A) if name == "sdiv" else (name, A, B) for name in BINARY}
ON_TWO.update({"sneg": ("sneg", ("ssub", B, A)), "sabs": ("sabs", ("ssub", B, A)), "sblend": ("sblend", 0.3, A, B), "sblend beyond 1": ("sblend", 1.25, B, A),
               "sbrightnesscontrast": ("sbrightnesscontrast", A, 0.1, 0.2), "sbrightnesscontrast clamps": ("sbrightnesscontrast", ("smul", B, c(0.01)), -0.5, 0.4)})
# a refl against a constant, in both positions where the order matters; hardlight on both sides of its 0.5
AGAINST_A_CONSTANT = {"%s refl const" % n: (n, A, c({"ssub": 0.1, "sadd": 0.25}.get(n, 0.75))) for n in BINARY}
AGAINST_A_CONSTANT.update({"%s const refl" % n: (n, c(1.2 if n == "ssub" else 0.25), A) for n in NON_COMMUTATIVE})
AGAINST_A_CONSTANT.update({"shardlight low const": ("shardlight", A, c(0.4)), "sblend refl const": ("sblend", 0.3, A, c(0.5)), "sblend const refl": ("sblend", 0.3, c(0.5), A)})


def render_ratio(expr, wl):
    got, _, _, _, on = textured_over_plain(N, EXTENT, wl, lambda b: expr.build(b))
    return got, on


def run_cases(cases, wl):
    worst = 0.0
    for label, tree in sorted(cases.items()):
        e = Expr(tree)
        want = np.float64(e.value(wl))
        assert 0 < want <= 1.5 or "clamps" in label, (label, want)
        got, on = render_ratio(e, wl)
        check("%s at %g nm" % (label, wl), got, np.full(got.shape, want), on)
        worst = max(worst, float(np.abs(got[on] - want).max() / (1e-5 * abs(want) + 1e-6)))
    print("worst deviation at %g nm: %.3f of the allowance" % (wl, worst))


# ---- 1: every operator -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wl", WAVELENGTHS)
def test_every_operator_on_two_refl_operands(wl):
    a, b = refl32(RGB_A, wl), refl32(RGB_B, wl)
    assert 0.1 < b < 0.5 < a < 1.0
    assert set(t[0] for t in ON_TWO.values()) == set(abi.SPEC_OPS)
    run_cases(ON_TWO, wl)


@pytest.mark.parametrize("wl", WAVELENGTHS)
def test_every_binary_operator_against_a_constant_in_both_positions(wl):
    run_cases(AGAINST_A_CONSTANT, wl)


# ---- 2, 3: the two leaves ----------------------------------------------------------------------------------------------------------------------
def test_peak_as_an_albedo():
    for wl, want in zip(WAVELENGTHS, (1.0 / 6, 1.0, 1.0 / 6)):
        e = Expr(("peak", 550.0, 120.0))
        assert abs(float(e.value(wl)) - want) < 1e-7
        got, on = render_ratio(e, wl)
        check("peak 550 +- 120 at %g nm" % wl, got, np.full(got.shape, want), on)


@pytest.mark.parametrize("t", [3000.0, 6500.0])
def test_blackbody_as_an_albedo(t):
    for wl in WAVELENGTHS:
        e = Expr(("blackbody", t))
        want = np.float64(e.value(wl))
        assert 0.05 < want <= 1.0 and abs(want - planck64(wl, t) / planck64(2.897771955e6 / t, t)) < 1e-6
        got, on = render_ratio(e, wl)
        check("blackbody %g K at %g nm" % (t, wl), got, np.full(got.shape, want), on)


# ---- 4: nesting --------------------------------------------------------------------------------------------------------------------------------
def left_deep_chain():
    tree = A
    for i in range(16):          # sixteen operators, the value kept inside (0.3, 1.2)
        tree = [("smul", tree, c(0.9)), ("sadd", tree, B), ("ssub", tree, c(0.2)), ("sdiv", tree, c(1.25)), ("sscreen", tree, c(0.1)), ("smax", tree, c(0.35)),
                ("sblend", 0.4, tree, A), ("sabs", tree)][i % 8]
    return tree


def balanced_tree():
    """eight leaves under seven binary operators: exactly PRGPU_EXPR_MAX_STACK entries"""
    leaves = [A, B, c(0.5), ("peak", 550.0, 400.0), B, c(0.25), A, ("blackbody", 5000.0)]
    level1 = [("sadd", leaves[0], leaves[1]), ("smul", leaves[2], leaves[3]), ("ssub", leaves[6], leaves[4]), ("smin", leaves[5], leaves[7])]
    return ("soverlay", ("sscreen", level1[0], level1[1]), ("sburn", level1[2], level1[3]))


def shared_node():
    n = ("sadd", B, ("smul", A, c(0.25)))           # ONE tuple object: Expr.build makes one node of it
    return ("smul", n, ("ssub", c(1.5), n))


@pytest.mark.parametrize("label,tree", [("a left-deep chain of 16 operators", left_deep_chain()), ("a balanced tree at the stack bound", balanced_tree()),
                                        ("a right-deep chain", ("ssub", c(1.0), ("smul", c(0.5), ("sadd", B, ("sdiv", B, ("sadd", A, c(0.5))))))),
                                        ("a node used twice", shared_node())])
def test_nesting(label, tree):
    e = Expr(tree)
    b = scene.SceneBuilder(8, 8)
    root = e.build(b)
    if "balanced" in label:
        assert len(b.spectra) == 13 and root == 12      # six distinct leaves (A and B are used twice each) under seven operators
    if "twice" in label:
        assert len(b.spectra) == 8           # B, A, 0.25, smul, sadd, 1.5, ssub, smul: thirteen were the shared node built twice
    for wl in WAVELENGTHS:
        want = np.float64(e.value(wl))
        assert 0 < want <= 1.5, (label, wl, want)
        got, on = render_ratio(e, wl)
        check("%s at %g nm" % (label, wl), got, np.full(got.shape, want), on)


# ---- as a light ----------------------------------------------------------------------------------------------------------------------------------


def lit_quad(n, wl=None, env=None, emission=None, mapper=None, spp=1):
    """the quad of the harness with albedo 1 under the environment env(b) (none: no environment), optionally emitting emission(b); mono at `wl`, or hero
    wavelengths over the default domain"""
    b = scene.SceneBuilder(n, n)
    s = b.settings
    s.aa_sampler, s.aa_samples, s.filter, s.filter_radius, s.nee = abi.SAMPLER_UNIFORM, spp, abi.FILTER_BLOCK, 0, 0
    if wl is not None:
        s.spectral_start = s.spectral_end = wl
        s.spectral_mono = 1
    if mapper is not None:
        s.mapper = mapper
    if env is not None:
        b.environment_light(env(b))
    x0, y0 = F(-1 + DX), F(-1 + DY)
    x1, y1 = F(x0 + F(2)), F(y0 + F(2))
    mat = b.lambert(b.spectrum_const(1.0))
    b.add_mesh([[x0, y0, 0], [x1, y0, 0], [x1, y1, 0], [x0, y1, 0]], [[0, 1, 2], [0, 2, 3]], mat, uvs=[[0, 0], [1, 0], [1, 1], [0, 1]],
               emission=None if emission is None else b.diffuse_emission(emission(b)))
    T = np.eye(4, dtype=F)
    T[2, 3] = 3.0
    b.set_camera(T, width=EXTENT, height=EXTENT, local_direction=(0, 0, -1), local_right=(1, 0, 0), local_up=(0, 1, 0), ortho=True)
    return b


def lamp(b):
    return b.spectrum_op("smul", b.spectrum_blackbody(T_LIGHT), b.spectrum_const(0.5))


@pytest.mark.parametrize("wl", WAVELENGTHS)
def test_an_expression_as_radiance_of_an_environment_and_of_an_emission(wl):
    want = np.float64(blackbody32(wl, T_LIGHT) * F(0.5))
    ref, ref_ent, _ = frame(lit_quad(N, wl, env=lambda b: b.spectrum_const(1.0)))
    on = ref_ent == 0
    ch = int(np.argmax(ref[on].mean(0)))
    assert on.sum() > 0.3 * N * N and (ref[..., ch] > 0).all()
    env, ent, info = frame(lit_quad(N, wl, env=lamp))
    assert np.array_equal(ent, ref_ent) and info["variant"] == 5
    everywhere = np.ones_like(on)
    check("environment at %g nm" % wl, env[..., ch] / ref[..., ch], np.full(on.shape, want), everywhere)     # the quad (albedo 1) and the background alike
    ems, ent, info = frame(lit_quad(N, wl, emission=lamp))
    assert np.array_equal(ent, ref_ent) and info["variant"] == 5 and (ems[~on] == 0).all()
    check("emission at %g nm" % wl, ems[..., ch] / ref[..., ch], np.full(on.shape, want), on)


def render_hero(b, iterations=16):
    ctx = backend.RenderContext(b.build(), device=0)
    ctx.enableVariance()
    ctx.render(iterations)
    ctx.waitForFinish()
    xyz = np.float64(ctx.output()[0])
    var = np.float64(ctx.variance()[1])
    info = ctx.pipelineInfo()
    info["on"] = ctx.primaryHits()[0].reshape(ctx.height, ctx.width) == 0      # the quad's pixels
    ctx.close()
    return xyz, var, info


def test_hero_wavelengths_blackbody_against_its_own_table_and_spd_against_random():
    """Interpolation bound: max |f''| / (8 f) per 1 nm cell, 3.5e-5 for 3200 K over 360 .. 830 nm; tests/test_spectral_expr_loader.py derives it and proves on
    the CPU that the fp32 restatement of the table lookup stays inside it.  The frames -- sums of radiance times positive weights at the same wavelengths -- then
    agree to that bound plus 4e-6 for the roundings of the sixteen-iteration mean."""
    bound = interpolation_bound(T_LIGHT)
    table = half_blackbody_table(T_LIGHT)

    a, var_a, info = render_hero(lit_quad(32, env=lamp, mapper=abi.MAPPER_RANDOM, spp=16))
    assert info["variant"] == 5
    b, _, _ = render_hero(lit_quad(32, env=lambda bb: bb.spectrum_table(360.0, 830.0, [float(v) for v in table]), mapper=abi.MAPPER_RANDOM, spp=16))
    assert (b > 0).all()
    err = np.abs(a - b) / b
    print("blackbody against its table: worst relative difference %.3g (bound %.3g)" % (err.max(), bound + 4e-6))
    assert err.max() <= bound + 4e-6 and err.max() > 0
    # The default mapper draws its wavelengths from a histogram the HOST evaluator fills with the light's power.  Importance sampling is unbiased under any
    # positive pdf, so this does not hold the histogram to the device's VALUES (the sky-albedo test of tests/test_spectral_expr_loader.py holds the host
    # evaluator to them); it shows that the host evaluates the expression to a usable density -- a histogram that were zero, NaN or negative where the lamp
    # shines would move the mean or blow the variance up.  The mean is taken over the QUAD's pixels:
    # a camera ray that leaves the scene is splatted without the wavelength pdf (IntegratorUtils.h:38, restated in shade_vertex and listed among the quirks of
    # DESIGN.md section 8), so the background's pixels depend on the mapper by design -- over the whole frame the two means are 0.587 and 1.245 on an MI355X.
    s, var_s, info_s = render_hero(lit_quad(32, env=lamp, spp=16))
    on = info["on"].copy()
    on[1:] &= info["on"][:-1]          # without the quad's rim, whose pixels the sixteen sub-pixel positions share with the background
    on[:-1] &= info["on"][1:]
    on[:, 1:] &= info["on"][:, :-1]
    on[:, :-1] &= info["on"][:, 1:]
    on[0] = on[-1] = on[:, 0] = on[:, -1] = False
    assert info_s["variant"] == 5 and np.array_equal(info["on"], info_s["on"]) and on.sum() > 0.3 * on.size
    n = int(on.sum())
    for ch in range(3):
        se = np.sqrt(var_a[..., ch][on].mean() / (16 * n) + var_s[..., ch][on].mean() / (16 * n))
        diff = abs(a[..., ch][on].mean() - s[..., ch][on].mean())
        print("channel %d: random %.6g spd %.6g, difference %.3g = %.2f standard errors" % (ch, a[..., ch][on].mean(), s[..., ch][on].mean(), diff, diff / se))
        assert se > 0 and diff <= 6 * se


# ---- every pipeline, bit for bit -------------------------------------------------------------------------------------------------------------------
COLOURS = {"red": (0.57, 0.012, 0.02), "green": (0.02, 0.51, 0.045), "grey": (0.46, 0.46, 0.46), "blue": (0.03, 0.08, 0.64), "tint": (0.87, 0.96, 0.83)}
IDENTITIES = ["smul smul", "sadd 0", "sblend 0", "smax x x", "sneg sneg", "sdiv 1"]


def cornell(wrapped):
    """The Cornell-style scene of test_gpu_image_texture.py (Lambert walls, an area light, a rough conductor, a principled and a glass card), its colours as
    (refl r g b) -- or every spectrum, the emission and the glass's index too, wrapped in one of six exact identities"""
    b = scene.SceneBuilder(64, 64)
    b.settings.aa_samples = 1
    b.settings.max_ray_depth = 8
    count = [0]

    def wrap(x):
        if not wrapped:
            return x
        op, cst = b.spectrum_op, b.spectrum_const
        which = IDENTITIES[count[0] % len(IDENTITIES)]
        count[0] += 1
        return {"smul smul": lambda: op("smul", op("smul", x, cst(1.0)), cst(1.0)), "sadd 0": lambda: op("sadd", x, cst(0.0)),
                "sblend 0": lambda: op("sblend", 0.0, x, b.refl(0.9, 0.1, 0.4)), "smax x x": lambda: op("smax", x, x),
                "sneg sneg": lambda: op("sneg", op("sneg", x)), "sdiv 1": lambda: op("sdiv", x, cst(1.0))}[which]()

    def colour(name):
        return wrap(b.refl(*COLOURS[name]))
    T = np.eye(4, dtype=F)
    T[:3, 3] = (0, -3.4, 1)
    b.set_camera(T, width=0.8, height=0.8, local_direction=(0, 1, 0), local_right=(1, 0, 0), local_up=(0, 0, 1))
    UV = [[0, 0], [1, 0], [1, 1], [0, 1]]

    def quad(p, mat, emission=None):
        b.add_mesh(p, [[0, 1, 2], [0, 2, 3]], mat, uvs=UV, emission=emission)
    grey, red, green = b.lambert(colour("grey")), b.lambert(colour("red")), b.lambert(colour("green"))
    quad([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], grey)
    quad([[-1, -1, 2], [-1, 1, 2], [1, 1, 2], [1, -1, 2]], grey)
    quad([[-1, 1, 0], [1, 1, 0], [1, 1, 2], [-1, 1, 2]], grey)
    quad([[-1, -1, 0], [-1, 1, 0], [-1, 1, 2], [-1, -1, 2]], red)
    quad([[1, -1, 0], [1, -1, 2], [1, 1, 2], [1, 1, 0]], green)
    quad([[-0.3, -0.3, 1.98], [0.3, -0.3, 1.98], [0.3, 0.3, 1.98], [-0.3, 0.3, 1.98]], grey, emission=b.diffuse_emission(wrap(b.spectrum_const(12.0))))
    metal = b.rough_conductor(0.25, specularity=colour("tint"))
    disney = b.principled(base=colour("blue"), roughness=0.4, metallic=0.3, clearcoat=0.5)
    glass = b.dielectric(wrap(b.spectrum_const(1.5)), transmission=colour("tint"))
    quad([[-0.8, 0.6, 0.1], [-0.2, 0.8, 0.1], [-0.2, 0.8, 1.1], [-0.8, 0.6, 1.1]], metal)
    quad([[0.2, 0.8, 0.1], [0.8, 0.5, 0.1], [0.8, 0.5, 1.0], [0.2, 0.8, 1.0]], disney)
    quad([[-0.4, -0.2, 0.2], [0.4, -0.2, 0.2], [0.4, -0.1, 0.9], [-0.4, -0.1, 0.9]], glass)
    if wrapped:
        assert count[0] == 8 and {IDENTITIES[i % 6] for i in range(count[0])} == set(IDENTITIES)      # five colours (tint twice), the emission, the glass's index
    return b.build()


def rendered(sc):
    ctx = backend.RenderContext(sc, device=0)
    ctx.render(1)
    ctx.waitForFinish()
    out = (ctx.output(), ctx.statistics(), ctx.pipelineInfo())
    ctx.close()
    return out


def test_exact_identities_change_nothing_in_any_pipeline(monkeypatch):
    """(As in test_gpu_image_texture.py: the shipped build holds the latency organisation for variant rows 1 and 4, so the second leg runs the throughput
    kernel of the top row unless the library was built with PL_VARIANTS="1 2 3 4 5".)"""
    ran = []
    for env in PIPELINES:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        (a, sa, ia), (r, sr, ir) = rendered(cornell(True)), rendered(cornell(False))
        for k in env:
            monkeypatch.delenv(k)
        ran.append((ia["mode"], ia["kernel"], ia["variant"], ir["variant"]))
        assert all(np.array_equal(x, y) for x, y in zip(a, r)), env
        assert sa == sr and sa["shadow_rays"] > 1000 and sa["bounce_rays"] > 3000, (env, sa, sr)
        assert np.isfinite(a[0]).all() and a[0].max() > 0
    print("pipelines:", ran)
    assert len({m for m, _, _, _ in ran}) == 3 and all(v == 5 for _, _, v, _ in ran)


# ---- hero collapse -----------------------------------------------------------------------------------------------------------------------------------
def test_a_spectral_varying_expression_as_index_collapses_to_the_hero_wavelength():
    """(smul (lookup_index 'bk7') 1) is NodeFlag::SpectralVarying as its operand is (SpectralMathNode.cpp:41): the path through the glass goes on with its hero
    wavelength alone, exactly as under the bare index -- the frame, the sample counts and the statistics (monochrome rays among them) are the same"""
    out = []
    for wrapped in (False, True):
        def glass(bb):
            index = bb.lookup_index("bk7")
            return bb.dielectric(bb.spectrum_op("smul", index, bb.spectrum_const(1.0)) if wrapped else index)
        b = scene.SceneBuilder(64, 64)          # the Cornell box with glass boxes (scene.cornell_glassy)
        b.settings.aa_sampler, b.settings.aa_samples = abi.SAMPLER_MJITT, 2
        scene._cornell_into(b, material_override={"shortBox": glass, "tallBox": glass})
        out.append(rendered(b.build()))
    (r, sr, ir), (a, sa, ia) = out
    assert ia["variant"] == 5 and ir["variant"] < 5
    assert all(np.array_equal(x, y) for x, y in zip(a, r))
    assert sa == sr and sa["monochrome_rays"] > 1000, (sa, sr)


# ---- a product of two leaves runs the code it ran, whatever its record's unused fields hold -----------------------------------------------------------
def test_unused_fields_of_a_product_record_are_ignored_in_the_top_row():
    """table_offset / table_count / wl_start / wl_end mean nothing on a MUL, and a caller of the C interface may leave anything there.  The top row's kernels
    read a root's program through those fields of the device's copy, so the scene zeroes them on every record that is no root -- also in a scene that has no
    expression and sits in the top row for another reason (here: a null material nothing uses).  The values chosen would, taken for a program, name one word,
    0, i.e. node 0, the environment's constant 1: the frame would be the albedo-1 frame instead of the product's."""
    wl = 550.0

    def albedo(stale):
        def make(b):
            b.spectrum_table(400.0, 700.0, [0.0, 0.0])          # the first table value: bits 0
            b.null()
            node = b.smul(b.refl(*RGB_A), b.refl(*RGB_B))
            if stale:
                s = b.spectra[node]
                s.table_offset, s.table_count, s.wl_start, s.wl_end = 0, 1, 1.0, 3.0
            return node
        return make
    frames = [frame(quad_scene(N, EXTENT, wl, albedo(stale))[0]) for stale in (False, True)]
    (clean, ent, info), (stale, ent_s, info_s) = frames
    assert info["variant"] == info_s["variant"] == 5 and np.array_equal(ent, ent_s)
    assert np.array_equal(clean, stale)
    got, on = render_ratio(Expr(("smul", A, B)), wl)
    ref = frame(quad_scene(N, EXTENT, wl, lambda b: b.spectrum_const(1.0))[0])[0]
    ch = int(np.argmax(ref[on].mean(0)))
    check("a product with stale fields", stale[..., ch] / ref[..., ch], np.full(on.shape, np.float64(refl32(RGB_A, wl) * refl32(RGB_B, wl))), on)
