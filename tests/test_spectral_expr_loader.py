"""Spectral expression nodes (PRGPU_SPEC_ADD .. PRGPU_SPEC_PEAK, include/prgpu.h) on the host: what the .prc loader parses
(inline forms and `(node ...)` blocks, defaults, the reference's quirks), SceneBuilder's records against the loader's, what the loader and
prgpu_scene_create's validation refuse -- the validation runs before any device call, so a refusal needs no GPU -- and the host evaluator.

The host evaluator is reached through the one place the library exposes it: a `sky` light's ground `:albedo` is evaluated by the loader at the eleven
band wavelengths of the sky model, 320 + 40 k nm (prgpu_prc_sky_info).  400 nm is one of them; 550 and 700 nm are not, 560 and 680 / 720 nm stand in
for them.  The host has ONE evaluator: expr_eval_at and spectrum_leaf_at of host/spectral_expr.h, over the arithmetic the kernels compile too
(device/node_math.h), which this test holds to float64.  Its other caller (host/setup.cpp: light power, the spd histogram) is not reachable without
a device; tests/test_gpu_spectral_expr.py renders under the `spd` mapper, whose histogram that caller fills, against the `random` one: that shows a
usable density, not its values (importance sampling is unbiased under any positive pdf).  spectral_range() of the new kinds (union / pass-through /
unbounded) has no observable on either side and is covered by reading only."""
import ctypes as C
import math

import numpy as np
import pytest

import image_files as imf
from pearray_amd import _cabi as abi
from pearray_amd import backend, scene

F = np.float32
SCENE = """(scene :render_width 8 :render_height 8
  (camera :name 'c' :type 'standard')
  %s
  (mesh :name 'q' (attribute :type 'p' [0,0,0],[1,0,0],[0,1,0]) (attribute :type 't' [0,0],[1,0],[0,1]) (faces [0,1,2]))
  (entity :name 'e' :type 'mesh' :mesh 'q' :materials 'm')
)"""
_KEEP = []   # a description points into its PrcScene: the scenes of this module stay alive

BINARY = {"sadd": abi.SPEC_ADD, "ssub": abi.SPEC_SUB, "smul": abi.SPEC_MUL, "sdiv": abi.SPEC_DIV, "smax": abi.SPEC_MAX, "smin": abi.SPEC_MIN,
          "sburn": abi.SPEC_BURN, "sscreen": abi.SPEC_SCREEN, "sdodge": abi.SPEC_DODGE, "soverlay": abi.SPEC_OVERLAY, "ssoftlight": abi.SPEC_SOFTLIGHT,
          "shardlight": abi.SPEC_HARDLIGHT}
UNARY = {"sneg": abi.SPEC_NEG, "sabs": abi.SPEC_ABS}
# every operator as an inline form over the operands A and B
FORMS = {**{k: "(%s A B)" % k for k in BINARY}, **{k: "(%s A)" % k for k in UNARY}, "sblend": "(sblend 0.25 A B)", "sbrightnesscontrast": "(sbrightnesscontrast A 0.1 0.2)"}
KINDS = {**BINARY, **UNARY, "sblend": abi.SPEC_BLEND, "sbrightnesscontrast": abi.SPEC_BRIGHTNESS_CONTRAST}


def load(blocks):
    _KEEP.append(scene.PrcScene(source=SCENE % blocks))
    return _KEEP[-1]


def material(albedo, before=""):
    return load("%s (material :name 'm' :type 'diffuse' :albedo %s)" % (before, albedo))


def record(m):
    return C.string_at(C.addressof(m), C.sizeof(m))


def refused(blocks, code, needle):
    with pytest.raises(abi.PrgpuError) as e:
        load(blocks)
    assert e.value.args[1] == code and needle in e.value.args[0], e.value.args


def form(name, a="(refl 0.2 0.5 0.7)", b="(refl 0.6 0.3 0.1)"):
    return FORMS[name].replace("A", a).replace("B", b)


# ---- parsing -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FORMS))
def test_every_operator_parses_inline(name):
    d = material(form(name)).desc
    n = d.spectra[d.materials[0].albedo]
    assert n.kind == KINDS[name]
    assert d.spectra[n.lhs].kind == abi.SPEC_PARAMETRIC and n.lhs < d.materials[0].albedo
    if name in UNARY or name == "sbrightnesscontrast":
        assert n.rhs == abi.INVALID_ID
    else:
        assert d.spectra[n.rhs].kind == abi.SPEC_PARAMETRIC and n.lhs < n.rhs < d.materials[0].albedo and record(d.spectra[n.lhs]) != record(d.spectra[n.rhs])
    assert tuple(n.p) == {"sblend": (0.25, 0, 0, 0), "sbrightnesscontrast": (F(0.1), F(0.2), 0, 0)}.get(name, (0, 0, 0, 0))
    assert (n.table_offset, n.table_count, n.wl_start, n.wl_end) == (0, 0, 0.0, 0.0)


@pytest.mark.parametrize("name", sorted(FORMS) + ["blackbody", "peak", "triangle_peak"])
def test_every_operator_parses_inline_on_an_emission_a_light_and_a_checkerboard_operand(name):
    text = {"blackbody": "(blackbody 3200)", "peak": "(peak 550 120)", "triangle_peak": "(triangle_peak 550 120)"}.get(name) or form(name)
    want = {"blackbody": abi.SPEC_BLACKBODY, "peak": abi.SPEC_PEAK, "triangle_peak": abi.SPEC_PEAK}.get(name) or KINDS[name]
    s = load("(material :name 'm' :type 'diffuse' :albedo (checkerboard 0.5 %s 4)) (emission :name 'e' :type 'standard' :radiance %s)"
             "(light :name 'l' :type 'env' :radiance %s :background %s)" % (text, text, text, text))
    d = s.desc
    checker = d.spectra[d.materials[0].albedo]
    roots = [checker.rhs, d.emissions[0].radiance, d.lights[0].radiance, d.lights[0].background]
    assert checker.kind == abi.SPEC_CHECKER and len(set(roots)) == 4 and not s.warnings, s.warnings
    for r in roots:          # four nodes of their own, the same record but for the operands' indices
        assert d.spectra[r].kind == want and tuple(d.spectra[r].p) == tuple(d.spectra[roots[0]].p)


@pytest.mark.parametrize("name", sorted(FORMS) + ["blackbody", "peak", "triangle_peak"])
def test_a_node_block_declares_a_name_for_every_user(name):
    """(node :name N :type T p0 p1 ...): the block's positional parameters are the inline form's; a material, an emission, an environment light and a
    checkerboard operand then use the name as a string -- and all four get the ONE node"""
    params = {"blackbody": "3200", "peak": "550 120", "triangle_peak": "550 120"}.get(name) or form(name)[len(name) + 2:-1]
    blocks = ("(node :name 'N' :type '%s' %s)"
              "(material :name 'm' :type 'diffuse' :albedo 'N') (material :name 'c' :type 'diffuse' :albedo (checkerboard 'N' 0.5 4))"
              "(emission :name 'e' :type 'standard' :radiance 'N') (light :name 'l' :type 'env' :radiance 'N')" % (name.upper() if name == "sadd" else name, params))
    s = load(blocks)
    d = s.desc
    node = d.materials[0].albedo
    want = {"blackbody": abi.SPEC_BLACKBODY, "peak": abi.SPEC_PEAK, "triangle_peak": abi.SPEC_PEAK}.get(name) or KINDS[name]
    assert d.spectra[node].kind == want and not s.warnings, s.warnings
    checker = d.spectra[d.materials[1].albedo]
    assert checker.kind == abi.SPEC_CHECKER and checker.lhs == node
    assert d.emissions[0].radiance == node and d.lights[0].radiance == node


def test_accepted_inline_types_declare_names_too():
    blocks = ("(node :name 'a' :type 'refl' 0.2 0.5 0.7) (node :name 'i' :type 'illuminant' 'D65') (node :name 'g' :type 'lookup_index' 'bk7')"
              "(node :name 's' :type 'spectrum' :start 400 :end 700 0.1 0.9) (node :name 'k' :type 'checkerboard' 'a' 'i' 3)"
              "(node :name 'p' :type 'smul' 'a' 'i')"
              "(material :name 'm' :type 'diffuse' :albedo 'k') (material :name 'x' :type 'glass' :index 'g' :specularity 'p' :transmission 's')")
    d = load(blocks).desc
    assert [d.spectra[i].kind for i in range(6)] == [abi.SPEC_PARAMETRIC, abi.SPEC_TABLE, abi.SPEC_SELLMEIER, abi.SPEC_TABLE, abi.SPEC_CHECKER, abi.SPEC_MUL]
    assert (d.spectra[4].lhs, d.spectra[4].rhs) == (0, 1) and (d.spectra[5].lhs, d.spectra[5].rhs) == (0, 1)
    m, x = d.materials[0], d.materials[1]
    assert m.albedo == 4 and (x.ior, x.albedo, x.transmission) == (2, 5, 3)


def test_defaults():
    d = material("(sadd (sblend) (smul (blackbody) (sdiv (peak) (sbrightnesscontrast (sneg)))))").desc
    by_kind = {d.spectra[i].kind: d.spectra[i] for i in range(d.n_spectra)}
    blend = by_kind[abi.SPEC_BLEND]
    assert blend.p[0] == 0.5 and (d.spectra[blend.lhs].kind, d.spectra[blend.lhs].p[0], d.spectra[blend.rhs].p[0]) == (abi.SPEC_CONST, 0.0, 0.0)   # :316, lookupSpectralNode's 0
    assert by_kind[abi.SPEC_BLACKBODY].p[0] == 6500.0 and tuple(by_kind[abi.SPEC_PEAK].p)[:2] == (520.0, 2.0)
    bc, neg = by_kind[abi.SPEC_BRIGHTNESS_CONTRAST], by_kind[abi.SPEC_NEG]
    assert tuple(bc.p) == (0, 0, 0, 0) and bc.lhs < d.n_spectra and d.spectra[neg.lhs].kind == abi.SPEC_CONST and d.spectra[neg.lhs].p[0] == 0.0
    one = material("(ssub 0.75)").desc      # a missing second operand
    n = one.spectra[one.materials[0].albedo]
    assert (one.spectra[n.lhs].p[0], one.spectra[n.rhs].p[0]) == (0.75, 0.0)


def test_a_numeric_temperature_is_always_peak_normalised():
    """BlackbodyNode.cpp:106-109 builds ConstBlackbodyNode<true> in both branches: the second parameter changes nothing"""
    recs = [record(material(a).desc.spectra[0]) for a in ("(blackbody 3200)", "(blackbody 3200 true)", "(blackbody 3200 false)")]
    assert recs[0] == recs[1] == recs[2]
    n = _KEEP[-1].desc.spectra[0]
    assert n.p[0] == 3200.0 and n.p[1] > 0 and abs(planck32(2.897771955e6 / 3200.0, 3200.0) * n.p[1] - 1) < 1e-6


def test_an_unknown_operand_name_warns_and_is_the_default():
    s = material("(sadd 'nowhere' 0.25)")
    d = s.desc
    n = d.spectra[d.materials[0].albedo]
    assert d.spectra[n.lhs].kind == abi.SPEC_CONST and d.spectra[n.lhs].p[0] == 0.0        # the operand's default, not the albedo's
    assert len(s.warnings) == 1 and "unknown node 'nowhere'" in s.warnings[0] and "default value used" in s.warnings[0]
    s = material("'nowhere'")
    assert s.desc.spectra[s.desc.materials[0].albedo].p[0] == 1.0 and len(s.warnings) == 1   # a parameter's own default stays what it was (lambert.cpp: albedo 1)
    s = material("(checkerboard (sadd 'nowhere' 0.5) 'nowhere')")                            # ... and so does a checkerboard operand's after an expression
    d = s.desc
    assert d.spectra[d.spectra[d.materials[0].albedo].rhs].p[0] == F(0.2) and len(s.warnings) == 2


@pytest.mark.parametrize("blocks,needle", [
    ("(node :name 'n' :type 'sadd' 1 2) (node :name 'n' :type 'smul' 1 2)", "already exists"),
    ("(node :type 'sadd' 1 2)", "without a name"),
    ("(node :name 'n' 1 2)", "no type given"),
])
def test_node_blocks_without_a_name_or_type_and_duplicates_are_errors(blocks, needle):
    refused(blocks + "(material :name 'm' :type 'diffuse')", -1, needle)


def test_other_node_types_keep_their_message():
    for t in ("perlin", "expr", "sciex"):
        refused("(node :name 'n' :type '%s') (material :name 'm' :type 'diffuse')" % t, -4, "not supported by this backend yet")
    refused("(material :name 'm' :type 'diffuse' :albedo (perlin 1 2))", -4, "perlin")


# ---- records -----------------------------------------------------------------------------------------------------------------------------
def test_scene_builder_assembles_the_loaders_records():
    text = ("(sadd (ssub (sdiv (refl 0.2 0.5 0.7) 2) (smul (smul (illum 1 2 3) 0.5) (blackbody 3200)))"
            " (smax (smin (sneg (sabs 0.5)) (peak 600 40)) (sburn (sscreen 0.1 0.2) (sdodge (soverlay 0.3 0.4) (ssoftlight (shardlight 0.5 0.6)"
            " (sblend 0.3 (sbrightnesscontrast 0.7 0.1 -0.2) (triangle_peak)))))))")
    d = material(text).desc
    b = scene.SceneBuilder(8, 8)
    c, op = b.spectrum_const, b.spectrum_op
    left = op("ssub", op("sdiv", b.refl(0.2, 0.5, 0.7), c(2)), op("smul", b.smul(b.illum(1, 2, 3), c(0.5)), b.spectrum_blackbody(3200)))
    low = op("smin", op("sneg", op("sabs", c(0.5))), b.spectrum_peak(600, 40))
    screen = op("sscreen", c(0.1), c(0.2))
    overlay = op("soverlay", c(0.3), c(0.4))
    hard = op("shardlight", c(0.5), c(0.6))
    blend = op("sblend", 0.3, op("sbrightnesscontrast", c(0.7), 0.1, -0.2), b.spectrum_peak())
    root = op("sadd", left, op("smax", low, op("sburn", screen, op("sdodge", overlay, op("ssoftlight", hard, blend)))))
    assert d.n_spectra == len(b.spectra) == root + 1 == d.materials[0].albedo + 1
    for i in range(d.n_spectra):
        assert record(d.spectra[i]) == record(b.spectra[i]), (i, d.spectra[i].kind)
    assert {d.spectra[i].kind for i in range(d.n_spectra)} >= set(range(abi.SPEC_ADD, abi.SPEC_PEAK + 1))
    for t in (1000.0, 2854.0, 6500.0, 12000.5):
        assert record(material("(blackbody %r)" % t).desc.spectra[0]) == record(b.spectra[b.spectrum_blackbody(t)]), t


def test_a_product_of_two_leaves_is_the_record_it_was():
    d = material("(smul (refl 0.2 0.5 0.7) (illuminant 'D65'))").desc
    assert d.n_spectra == 3 and [d.spectra[i].kind for i in range(3)] == [abi.SPEC_PARAMETRIC, abi.SPEC_TABLE, abi.SPEC_MUL]
    n = d.spectra[2]
    assert (n.lhs, n.rhs, tuple(n.p), n.table_offset, n.table_count, n.wl_start, n.wl_end) == (0, 1, (0, 0, 0, 0), 0, 0, 0.0, 0.0)
    b = scene.SceneBuilder(8, 8)
    b.smul(b.refl(0.2, 0.5, 0.7), b.illuminant_d65())
    assert all(record(d.spectra[i]) == record(b.spectra[i]) for i in range(3))
    assert max(d.spectra[i].kind for i in range(3)) <= abi.SPEC_IMAGE          # nothing in the description asks for the expression evaluator


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("expr,needle", [
    ("(sblend (refl 1 1 1) 0.2 0.3)", "factor"), ("(sbrightnesscontrast 0.5 (refl 1 1 1) 0.1)", "brightness"), ("(sbrightnesscontrast 0.5 0.1 (sadd 1 2))", "contrast"),
    ("(blackbody (sadd 1 2))", "temperature"), ("(peak (refl 1 1 1) 2)", "wavelength"), ("(triangle_peak 520 (refl 1 1 1))", "radius"),
])
def test_dynamic_forms_stay_refused(expr, needle):
    refused("(material :name 'm' :type 'diffuse' :albedo %s)" % expr, -4, needle)


@pytest.mark.parametrize("name", sorted(FORMS))
def test_no_uv_dependent_node_below_a_math_node(name, tmp_path):
    refused("(material :name 'm' :type 'diffuse' :albedo %s)" % form(name, a="(checkerboard 0.2 0.8)"), -4, "a checkerboard inside " + name)
    path = imf.write(tmp_path / "t.png", imf.encode_png(np.full((1, 1, 3), 128), 2, 8))
    texture = "(texture :name 't' :file '%s' :type 'color')" % path
    refused(texture + "(material :name 'm' :type 'diffuse' :albedo %s)" % form(name, a="'t'"), -4, "an image texture inside " + name)
    if name not in UNARY and name != "sbrightnesscontrast":
        refused(texture + "(material :name 'm' :type 'diffuse' :albedo %s)" % form(name, b="'t'"), -4, "an image texture inside " + name)


def balanced(depth, leaf=iter(range(1, 1000))):
    return "0.%03d" % next(leaf) if depth == 0 else "(sadd %s %s)" % (balanced(depth - 1), balanced(depth - 1))


def test_the_stack_bound():
    """A balanced tree of depth k needs k + 1 entries (leaf 1, one more wherever both operands need the same)"""
    d = material(balanced(abi.EXPR_MAX_STACK - 1)).desc
    assert d.n_spectra == 2 ** abi.EXPR_MAX_STACK - 1
    refused("(material :name 'm' :type 'diffuse' :albedo %s)" % balanced(abi.EXPR_MAX_STACK), -4, "PRGPU_EXPR_MAX_STACK")
    chain = "0.5"
    for i in range(16):     # a chain is two entries deep whichever side it grows on
        chain = "(sadd %s 0.25)" % chain if i % 2 else "(ssub 0.125 %s)" % chain
    assert material(chain).desc.n_spectra == 33


def test_the_program_length_bound():
    def chain(n):
        text = "0.5"
        for _ in range(n):
            text = "(sadd %s 0.25)" % text
        return text
    assert material(chain((abi.EXPR_MAX_PROGRAM - 1) // 2)).desc.n_spectra == abi.EXPR_MAX_PROGRAM - 1      # 31 operators: 63 words
    refused("(material :name 'm' :type 'diffuse' :albedo %s)" % chain(abi.EXPR_MAX_PROGRAM // 2), -4, "PRGPU_EXPR_MAX_PROGRAM")
    # a shared node counts once per path to it: a named chain of 20 operators (41 words) used twice, beside a tree that needs three entries
    nodes = ("(node :name 'c' :type 'sadd' %s 0.25) (node :name 't' :type 'sadd' (sadd 0.1 0.2) (sadd 0.3 0.4)) (node :name 'x' :type 'sadd' 't' 'c')" % chain(19))
    assert material("'x'", before=nodes).desc.n_spectra == 41 + 7 + 1
    refused(nodes + "(node :name 'y' :type 'sadd' 'x' 'c') (material :name 'm' :type 'diffuse' :albedo 'y')", -4, "PRGPU_EXPR_MAX_PROGRAM")


def one_triangle(spectra):
    b = scene.SceneBuilder(8, 8)
    albedo = spectra(b)
    b.add_mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 1, 2]], b.lambert(albedo))
    return b


def hand_made(kind, lhs=0, rhs=0, p=()):
    def spectra(b):
        b.spectrum_const(0.5)
        return b._add_spec(kind=kind, lhs=lhs, rhs=rhs, p=list(p))
    return spectra


def deep(b):
    leaves = [b.spectrum_const(0.1 * i) for i in range(2 ** abi.EXPR_MAX_STACK)]
    while len(leaves) > 1:
        leaves = [b.spectrum_op("sadd", leaves[i], leaves[i + 1]) for i in range(0, len(leaves), 2)]
    return leaves[0]


def long(b):
    node = b.spectrum_const(0.5)
    for _ in range(abi.EXPR_MAX_PROGRAM // 2):
        node = b.spectrum_op("sadd", node, b.spectrum_const(0.25))
    return node


@pytest.mark.parametrize("label,spectra,code,needle", [
    ("an operand that is the node itself", hand_made(abi.SPEC_ADD, 0, 1), -1, "operands must precede"),
    ("an operand behind the node", hand_made(abi.SPEC_NEG, 2, abi.INVALID_ID), -1, "operands must precede"),
    ("a forward operand of a blend", hand_made(abi.SPEC_BLEND, 5, 0, (0.5,)), -1, "operands must precede"),
    ("a temperature of zero", hand_made(abi.SPEC_BLACKBODY, p=(0.0, 1.0)), -1, "temperature must be positive"),
    ("a negative temperature", hand_made(abi.SPEC_BLACKBODY, p=(-300.0, 1.0)), -1, "temperature must be positive"),
    ("a radius of zero", hand_made(abi.SPEC_PEAK, p=(520.0, 0.0)), -1, "radius must be positive"),
    ("a negative radius", hand_made(abi.SPEC_PEAK, p=(520.0, -2.0)), -1, "radius must be positive"),
    ("an infinite factor", hand_made(abi.SPEC_BLEND, 0, 0, (float("inf"),)), -1, "parameters must be finite"),
    ("a NaN contrast", hand_made(abi.SPEC_BRIGHTNESS_CONTRAST, 0, abi.INVALID_ID, (0.1, float("nan"))), -1, "parameters must be finite"),
    ("a NaN temperature", hand_made(abi.SPEC_BLACKBODY, p=(float("nan"), 1.0)), -1, "parameters must be finite"),
    ("a kind past the last one", hand_made(abi.SPEC_PEAK + 1), -1, "unknown spectrum kind"),
    ("a checkerboard below a math node", lambda b: b.spectrum_op("sadd", b.checkerboard(b.spectrum_const(0.2), b.spectrum_const(0.8)), b.spectrum_const(0.1)), -4, "a checkerboard inside"),
    ("an image below a math node", lambda b: b.spectrum_op("sneg", b.image_texture(np.full((1, 1, 3), 0.5, F))), -4, "an image texture inside"),
    ("a stack one over the bound", deep, -4, "PRGPU_EXPR_MAX_STACK"),
    ("a program over the bound", long, -4, "PRGPU_EXPR_MAX_PROGRAM"),
])
def test_validation_refuses(label, spectra, code, needle):
    """prgpu_scene_create validates the description before it selects a device (prgpu_api.hip), so these return without one"""
    b = one_triangle(spectra)
    with pytest.raises(abi.PrgpuError) as e:
        backend.RenderContext(b.build(), device=0)
    assert ("prgpu error %d:" % code) in str(e.value) and needle in str(e.value), (label, str(e.value))


# ---- the host evaluator --------------------------------------------------------------------------------------------------------------------
BANDS = [320.0 + 40.0 * k for k in range(11)]          # 400 nm is band 2, 560 nm band 6, 680 / 720 nm bands 9 / 10


def planck64(wl, t):
    c, h, kb = 299792458.0, 6.62607004081e-34, 1.3806485279e-23
    lam = np.float64(wl) * 1e-9
    return (2 * h * c * c / lam ** 5) / np.expm1(h * c / (kb * lam * t))


def planck32(wl, t):
    return float(F(planck64(float(F(F(wl) * F(1e-9))) * 1e9, float(F(t)))))


def blackbody64(wl, t):
    """the node's value in float64: Planck's law over its value at Wien's peak"""
    return planck64(wl, t) / planck64(2.897771955e6 / t, t)


def albedo_at_the_bands(expr):
    s = load("(light :name 'sky' :type 'sky' :albedo %s :azimuth_resolution 8 :elevation_resolution 4) (material :name 'm' :type 'diffuse')" % expr)
    (_, _, _, albedo), = s.sky_params().values()
    return np.array(albedo)


@pytest.mark.parametrize("t", [3000.0, 6500.0])
def test_host_blackbody(t):
    got = albedo_at_the_bands("(blackbody %g)" % t)
    want = np.array([blackbody64(w, t) for w in BANDS])
    print("blackbody %g K: worst relative deviation %.3g" % (t, np.abs(got / want - 1).max()))
    assert (np.abs(got - want) <= 1e-6 * want).all()        # three float roundings (value, norm, their product): 2e-7
    assert 0 < got.min() and got.max() <= 1.0 + 1e-6 and (np.argmax(got) == (10 if t == 3000.0 else 3))   # 6500 K peaks at 446 nm


def test_host_peak():
    got = albedo_at_the_bands("(peak 550 120)")
    want = np.array([max(0.0, 1 - abs(w - 550.0) / 120.0) for w in BANDS])
    assert np.abs(got - want).max() <= 2e-7 and got[0] == 0.0 and got[6] == float(F(1) - F(10) / F(120))


def test_host_nested_expression():
    """(sblend 0.25 (smul (smul refl 0.5) (blackbody 4000)) (sdiv (peak 500 300) (sadd refl 1))) against float64"""
    rgb = (0.2, 0.5, 0.7)
    got = albedo_at_the_bands("(sblend 0.25 (smul (smul (refl %g %g %g) 0.5) (blackbody 4000)) (sdiv (peak 500 300) (sadd (refl %g %g %g) 1)))" % (rgb + rgb))
    co = np.array(scene.rgb_to_coeffs(rgb), F)[None, :]
    refl = np.array([np.float64(imf.upsample32(co, w)[0]) for w in BANDS])
    peak = np.array([max(0.0, 1 - abs(w - 500.0) / 300.0) for w in BANDS])
    bb = np.array([blackbody64(w, 4000.0) for w in BANDS])
    want = (refl * 0.5 * bb) * 0.75 + (peak / (refl + 1)) * 0.25
    print("nested expression: worst deviation %.3g" % np.abs(got - want).max())
    assert np.abs(got - want).max() <= 1e-6          # eight fp32 roundings of values below 1
    assert np.ptp(want) > 0.1


# ---- the blackbody against a 1 nm table of itself: the bound tests/test_gpu_spectral_expr.py holds two frames to, proved here without a GPU ----------
T_LIGHT = 3200.0


def blackbody32(wl, t):
    """the node's fp32 value: float(Planck in double at the fp32 wavelength) times the fp32 normalisation 1 / float(Planck at Wien's peak)"""
    nm = np.float64(F(wl) * F(1e-9)) * 1e9
    norm = F(1) / F(planck64(np.float64(F(F(2.897771955e6) / F(t)) * F(1e-9)) * 1e9, float(F(t))))
    return F(planck64(nm, float(F(t)))) * norm


def interpolation_bound(t, lo=360, hi=830):
    """Linear interpolation of f between samples 1 nm apart is off by at most max |f''| / 8 inside a cell.  Relative to f: the largest, over the cells, of
    max |f''| (second differences on a 0.05 nm grid) / 8 over min f of the cell."""
    fine = np.arange(lo, hi + 1e-9, 0.05)
    f = planck64(fine, t) / planck64(2.897771955e6 / t, t) * 0.5
    second = np.abs(np.diff(f, 2)) / 0.05 ** 2
    worst = 0.0
    for k in range((len(fine) - 1) // 20):
        worst = max(worst, second[max(0, 20 * k - 1):20 * k + 20].max() / 8 / f[20 * k:20 * k + 21].min())
    return worst


def half_blackbody_table(t, lo=360, hi=830):
    """0.5 blackbody(t) at every nanometre of lo .. hi, float64 values rounded to the fp32 a TABLE node holds"""
    grid = np.arange(lo, hi + 1, dtype=np.float64)
    return F(planck64(grid, t) / planck64(2.897771955e6 / t, t) * 0.5)


def test_the_fp32_table_lookup_stays_inside_the_interpolation_bound():
    """For 3200 K over 360 .. 830 nm, max |f''| / (8 f) per 1 nm cell is 3.5e-5, at the blue end (f'' / f is about (c2 / (lambda T) - 5)(c2 / (lambda T) - 6) /
    lambda^2 there).  The numpy restatement -- fp32 table, fp32 interpolation as equidistant_lookup does it, against the fp32 node -- stays inside that
    bound plus 1e-6 of fp32 rounding at every half nanometre, where the interpolation error is largest."""
    bound = interpolation_bound(T_LIGHT)
    assert 1e-5 < bound < 4e-5, bound
    table = half_blackbody_table(T_LIGHT)
    mid = F(np.arange(360.5, 830, 1.0))
    k = np.int32(np.floor(mid - F(360)))
    t = (mid - F(360)) - F(k)
    interp = table[k] * (F(1) - t) + table[k + 1] * t
    node = np.array([blackbody32(w, T_LIGHT) * F(0.5) for w in mid])
    err = np.abs(np.float64(interp) - node) / node
    print("table against node: worst relative difference %.3g (bound %.3g)" % (err.max(), bound))
    assert (err <= bound + 1e-6).all() and err.max() > 0.1 * bound          # and the bound is not idle: the blue end comes close to it
