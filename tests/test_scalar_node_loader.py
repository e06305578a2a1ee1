"""Scalar nodes (include/prgpu.h, PRGPU_SPEC_SCALAR_IMAGE .. PRGPU_SPEC_SCALAR_COS and the PRGPU_MATF_NODE_* bits) on the host:
the scalar mode of the image reader, `(texture :type 'scalar')` blocks, inline scalar math groups and `(node ...)` blocks of the scalar types in the .prc
loader, the records SceneBuilder.scalar_image / scalar_op assemble, constant folding, the defaults of lookupScalarNode, and what the loader, SceneBuilder
and prgpu_scene_create's validation refuse -- the validation runs before any device call, so a refusal needs no GPU.  The images are written here."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import image_files as imf
from pearray_amd import _cabi as abi
from pearray_amd import backend, scene

F = np.float32
HEAD = """(scene :render_width 8 :render_height 8 :camera 'cam'
  (camera :name 'cam' :type 'standard' :position [0, 0, 3])
  (mesh :name 'quad' (attribute :type 'p' [-1,-1,0],[1,-1,0],[1,1,0],[-1,1,0]) (attribute :type 't' [0,0],[1,0],[1,1],[0,1]) (faces [0,1,2],[0,2,3]))
"""
GREY = np.array([[[0], [255], [7]], [[128], [64], [200]]])                                   # 3 x 2, one channel
RGB = np.array([[[10, 200, 30], [250, 1, 2]], [[90, 80, 70], [0, 255, 255]]])                # 2 x 2: R differs from G and B everywhere
_KEEP = []   # a description points into its PrcScene: the scenes of this module stay alive


def load(tmp_path, body, **kw):
    sc = scene.PrcScene(source=HEAD + body + "\n)", include_dir=str(tmp_path), **kw)
    sc.warnings = [w for w in sc.warnings if "the scene has no entities" not in w]
    _KEEP.append(sc)
    return sc


def refused(tmp_path, body, code, needle):
    with pytest.raises(abi.PrgpuError) as e:
        load(tmp_path, body)
    assert e.value.args[1] == code and needle in e.value.args[0], e.value.args


def record(x):
    return C.string_at(C.addressof(x), C.sizeof(x))


def tables(d):
    return np.ctypeslib.as_array(d.spectral_tables, shape=(d.n_spectral_table_values,)).copy()


@pytest.fixture
def files(tmp_path):
    imf.write(tmp_path / "tex.png", imf.encode_png(GREY, 0, 8))
    imf.write(tmp_path / "col.png", imf.encode_png(RGB, 2, 8))
    return tmp_path


TEX = "(texture :name 'tex' :file 'tex.png' :type 'scalar' :interpolation 'closest')"


# ---- the reader's scalar mode ----------------------------------------------------------------------------------------------------------------
def test_the_scalar_mode_reads_the_first_channel_as_it_is(tmp_path):
    g8, ch = scene.load_scalar_image(imf.write(tmp_path / "g8.png", imf.encode_png(GREY, 0, 8)))
    assert ch == 1 and g8.dtype == F and np.array_equal(g8, F(GREY[:, :, 0]) / F(255))
    linear = scene.load_image(str(tmp_path / "g8.png"))[0][:, :, 0]
    assert not np.array_equal(g8, linear) and np.array_equal(linear[0, :2], g8[0, :2])       # not linearised (0 and 1 are fixed points)
    wide = GREY * 257 + np.array([[[0], [0], [3]], [[1], [100], [5]]])                        # 16 bit samples that are no multiple of 257
    g16, ch = scene.load_scalar_image(imf.write(tmp_path / "g16.png", imf.encode_png(wide, 0, 16)))
    assert ch == 1 and np.array_equal(g16, F(wide[:, :, 0]) / F(65535))
    r, ch = scene.load_scalar_image(imf.write(tmp_path / "rgb.png", imf.encode_png(RGB, 2, 8)))
    assert ch == 3 and r.shape == (2, 2) and np.array_equal(r, F(RGB[:, :, 0]) / F(255))      # an RGB file gives its R channel
    ga, ch = scene.load_scalar_image(imf.write(tmp_path / "ga.png", imf.encode_png(np.concatenate([GREY, 255 - GREY], 2), 4, 8)))
    assert ch == 2 and np.array_equal(ga, g8)                                                # grey + alpha: the grey
    values = F([[0.25, -1.5, 3.0], [1e-3, 0.5, 7.25]])
    for little in (True, False):
        p, ch = scene.load_scalar_image(imf.write(tmp_path / "s.pfm", imf.encode_pfm(values, little=little)))
        assert ch == 1 and np.array_equal(p, values)                                         # a PFM float as it is, rows top-down
    colour = np.stack([values, values + 1, values + 2], 2)
    p, ch = scene.load_scalar_image(imf.write(tmp_path / "c.pfm", imf.encode_pfm(colour)))
    assert ch == 3 and np.array_equal(p, values)
    lib = abi.load()
    w, h = C.c_uint32(), C.c_uint32()
    assert lib.prgpu_image_load_scalar(os.fsencode(str(tmp_path / "nope.png")), C.byref(w), C.byref(h), None, None) == -5
    assert lib.prgpu_image_load_scalar(None, C.byref(w), C.byref(h), None, None) == -1


# ---- a scalar texture block --------------------------------------------------------------------------------------------------------------------
def test_a_scalar_texture_block_yields_a_scalar_image_node(files):
    sc = load(files, """(texture :name 'tex' :file 'tex.png' :type 'scalar' :interpolation 'bi' :wrap ['mirror', 'clamp'])
        (material :name 'm' :type 'roughconductor' :roughness 'tex')
        (entity :name 'q' :type 'mesh' :mesh 'quad' :materials 'm')""")
    assert sc.warnings == []
    d = sc.desc
    m = d.materials[0]
    assert m.flags == abi.MATF_NODE_ROUGHNESS_X and m.roughness_x == m.roughness_y
    n = d.spectra[int(m.roughness_x)]
    assert n.kind == abi.SPEC_SCALAR_IMAGE == 32 and (n.lhs, n.rhs) == (3, 2) and list(n.p)[:3] == [1.0, 3.0, 1.0] and n.table_count == 3 * 2 + 1
    assert np.array_equal(tables(d)[n.table_offset:n.table_offset + n.table_count], np.append(F(GREY[:, :, 0]).reshape(-1) / F(255), F(0)))
    # an RGB file: its R channel
    d = load(files, "(texture :name 'r' :file 'col.png' :type 'scalar') (material :name 'm' :type 'orennayar' :roughness 'r')").desc
    n = d.spectra[0]
    assert n.kind == abi.SPEC_SCALAR_IMAGE and np.array_equal(tables(d)[n.table_offset:n.table_offset + 4], F(RGB[:, :, 0]).reshape(-1) / F(255))
    # NOT the reference's: a scalar texture that no scalar parameter and no scalar node names stays refused, as tests/test_texture_loader.py pins it
    refused(files, TEX, -4, "scalar textures are not supported")
    refused(files, TEX + "(material :name 'm' :type 'diffuse' :albedo 'tex')", -4, "nothing names this one")      # (a spectral parameter takes its default)
    assert load(files, TEX + "(node :name 'n' :type 'mul' 'tex' 0.5)").desc.n_spectra == 3                        # a scalar node names it
    refused(files, TEX + TEX, -1, "already exists")
    refused(files, "(texture :name 's' :file 'nope.png' :type 'scalar')", -5, "nope.png")


# ---- .prc against SceneBuilder ----------------------------------------------------------------------------------------------------------------
def same_description(d, b):
    assert d.n_spectra == len(b.spectra) and d.n_materials == len(b.materials)
    for i in range(d.n_spectra):
        assert record(d.spectra[i]) == record(b.spectra[i]), ("node", i, d.spectra[i].kind, b.spectra[i].kind)
    for i in range(d.n_materials):
        assert record(d.materials[i]) == record(b.materials[i]), ("material", i)
    assert np.array_equal(tables(d), F(b.tables))


def test_scene_builder_assembles_the_loaders_records(files):
    principled = ("roughness", "diffuse_transmission", "specular_transmission", "specular_tint", "anisotropic", "flatness", "metallic", "sheen", "sheen_tint",
                  "clearcoat", "clearcoat_gloss")
    d = load(files, TEX + """(texture :name 'bi' :file 'col.png' :type 'scalar' :interpolation 'bilinear' :wrap 'periodic')
        (material :name 'a' :type 'roughconductor' :roughness 'tex')
        (material :name 'b' :type 'roughmetal' :roughness_x 'tex' :roughness_y 'bi')
        (material :name 'c' :type 'roughglass' :roughness_x 0.25 :roughness_y 'tex')
        (material :name 'd' :type 'conductor' :roughness 'bi')
        (material :name 'e' :type 'glass' :roughness 'tex' :vndf false)
        (material :name 'f' :type 'orennayar' :albedo 0.5 :roughness 'tex')
        (material :name 'g' :type 'principled' %s)
        (material :name 'h' :type 'roughconductor' :roughness (mul 'tex' 0.5))
        (node :name 'half' :type 'add' (min 'bi' 0.75) (neg (sqrt 'tex')))
        (material :name 'i' :type 'orennayar' :roughness 'half')
        (material :name 'j' :type 'principled' :metallic 'half' :subsurface (pow 'tex' 2))
        (entity :name 'q' :type 'mesh' :mesh 'quad' :materials 'a')""" % " ".join(":%s '%s'" % (k, "tex" if i % 2 else "bi") for i, k in enumerate(principled))).desc
    b = scene.SceneBuilder(8, 8)
    c = b.spectrum_const
    tex = b.scalar_image(F(GREY[:, :, 0]) / F(255), "closest")
    bi = b.scalar_image(F(RGB[:, :, 0]) / F(255), "bilinear", "periodic")
    b.rough_conductor(tex)
    b.rough_conductor(tex, roughness_y=bi)
    b.rough_dielectric(0.25, roughness_y=tex)
    b.rough_conductor(bi)
    b.rough_dielectric(tex, vndf=False)
    b.oren_nayar(c(0.5), tex)
    b.principled(**{k: (tex if i % 2 else bi) for i, k in enumerate(principled)})
    eta, k, spec = c(1.2), c(2.605), c(1.0)                      # the loader reads the spectral parameters first, then the roughness
    b.rough_conductor(b.scalar_op("mul", tex, 0.5), eta=eta, k=k, specularity=spec)
    half = b.scalar_op("add", b.scalar_op("min", bi, 0.75), b.scalar_op("neg", b.scalar_op("sqrt", tex)))
    b.oren_nayar(c(1.0), half)
    base, ior = c(0.8), c(1.55)
    b.principled(base=base, ior=ior, metallic=half, flatness=b.scalar_op("pow", tex, 2))
    same_description(d, b)
    m = d.materials
    assert m[1].flags == abi.MATF_NODE_ROUGHNESS_X | abi.MATF_NODE_ROUGHNESS_Y | abi.MATF_ANISOTROPIC and m[2].flags == abi.MATF_NODE_ROUGHNESS_Y | abi.MATF_ANISOTROPIC
    assert m[6].flags == abi.MATF_HAS_TRANSMISSION | abi.MATF_NODE_ROUGHNESS_X | (0x3FF * abi.MATF_NODE_PRINCIPLED)      # the key's presence, as before
    assert m[8].roughness_x == m[9].principled[5] == half.id and d.spectra[half.id].kind == abi.SPEC_SCALAR_ADD      # one node, two users
    assert (m[9].flags, m[9].principled[4]) == (abi.MATF_NODE_PRINCIPLED << 5 | abi.MATF_NODE_PRINCIPLED << 4, d.n_spectra - 1)


def test_a_scene_without_scalar_nodes_is_the_description_it_was(files):
    """no bit, no new kind: numbers stay numbers, folded trees included"""
    d = load(files, """(material :name 'a' :type 'roughconductor' :roughness (mul 0.5 0.5) :roughness_y 0.125)
        (material :name 'p' :type 'principled' :roughness 0.3 :metallic (sub 1 0.75))""").desc
    b = scene.SceneBuilder(8, 8)
    b.rough_conductor(b.scalar_op("mul", 0.5, 0.5), roughness_y=0.125)
    b.principled(roughness=0.3, metallic=b.scalar_op("sub", 1, 0.75))
    same_description(d, b)
    assert d.materials[0].flags == abi.MATF_ANISOTROPIC and d.materials[0].roughness_x == 0.25 and d.materials[1].principled[5] == 0.25
    assert max(d.spectra[i].kind for i in range(d.n_spectra)) == abi.SPEC_CONST


# ---- folding ------------------------------------------------------------------------------------------------------------------------------------
A, B = 0.6, 0.3
FOLDS = {  # name -> (text of the operands, the float64 value of the float32 operands, exact in float32?)
    "add": ("A B", lambda a, b: F(a) + F(b), True), "sub": ("A B", lambda a, b: F(a) - F(b), True), "subtract": ("A B", lambda a, b: F(a) - F(b), True),
    "mul": ("A B", lambda a, b: F(a) * F(b), True), "multiply": ("A B", lambda a, b: F(a) * F(b), True), "div": ("A B", lambda a, b: F(a) / F(b), True),
    "divide": ("A B", lambda a, b: F(a) / F(b), True), "neg": ("A", lambda a, b: -F(a), True), "negate": ("A", lambda a, b: -F(a), True),
    "sin": ("A", lambda a, b: math.sin(a), False), "cos": ("A", lambda a, b: math.cos(a), False), "tan": ("A", lambda a, b: math.tan(a), False),
    "asin": ("A", lambda a, b: math.asin(a), False), "acos": ("A", lambda a, b: math.acos(a), False), "atan": ("A", lambda a, b: math.atan(a), False),
    "sinh": ("A", lambda a, b: math.sinh(a), False), "cosh": ("A", lambda a, b: math.cosh(a), False), "tanh": ("A", lambda a, b: math.tanh(a), False),
    "asinh": ("A", lambda a, b: math.asinh(a), False), "acosh": ("2.5", lambda a, b: math.acosh(2.5), False), "atanh": ("A", lambda a, b: math.atanh(a), False),
    "exp": ("A", lambda a, b: math.exp(a), False), "log": ("A", lambda a, b: math.log(a), False), "abs": ("-0.75", lambda a, b: F(0.75), True),
    "sqrt": ("A", lambda a, b: np.sqrt(F(a)), True), "cbrt": ("A", lambda a, b: float(a) ** (1.0 / 3.0), False), "ceil": ("A", lambda a, b: F(1), True),
    "floor": ("2.5", lambda a, b: F(2), True), "round": ("2.5", lambda a, b: F(3), True), "atan2": ("A B", lambda a, b: math.atan2(a, b), False),
    "max": ("A B", lambda a, b: F(a), True), "min": ("A B", lambda a, b: F(b), True),
}


def ulps(x, y):
    return abs(int(F(x).view(np.int32)) - int(F(y).view(np.int32)))


@pytest.mark.parametrize("name", sorted(FOLDS))
def test_every_operator_folds_over_constants(files, name):
    """All 32 names of ScalarMathNode.cpp: the record is the number's -- no node, no bit -- in the loader and in SceneBuilder.  The arithmetic ones, sqrt and
    the roundings are exact in float32; the transcendental ones may differ from the correctly rounded value by one ulp (libm's float functions)."""
    assert len(FOLDS) == 32 and set(FOLDS) <= set(abi.SCALAR_OPS)
    text, value, exact = FOLDS[name]
    a, b = float(F(A)), float(F(B))
    want = F(value(a, b))
    d = load(files, "(material :name 'm' :type 'orennayar' :roughness (%s %s))" % (name, text.replace("A", repr(A)).replace("B", repr(B)))).desc
    m = d.materials[0]
    plain = load(files, "(material :name 'm' :type 'orennayar' :roughness %r)" % float(m.roughness_x)).desc.materials[0]
    assert m.flags == 0 and d.n_spectra == 1 and record(m) == record(plain)
    operands = [float(x) if x not in "AB" else (A if x == "A" else B) for x in text.split()]
    built = F(scene.SceneBuilder(8, 8).scalar_op(name, *operands))
    print("%s: loader %r, builder %r, float64 %r" % (name, float(m.roughness_x), float(built), float(want)))
    for got in (F(m.roughness_x), built):
        assert ulps(got, want) <= (0 if exact else 1), (name, float(got), float(want))


def test_pow_and_nested_trees_fold_too(files):
    m = load(files, "(material :name 'm' :type 'roughconductor' :roughness (add (mul 2 0.25) (neg (pow 0.5 2))) :roughness_y (max (floor 0.9) (min 0.25 7)))").desc.materials[0]
    assert (m.flags, m.roughness_x, m.roughness_y) == (abi.MATF_ANISOTROPIC, 0.25, 0.25)


# ---- defaults: lookupScalarNode (SceneLoadContext.cpp:236-266) --------------------------------------------------------------------------------------
def test_operands_that_name_no_scalar_node_are_the_default(files):
    colour = "(texture :name 'col' :file 'col.png' :type 'color' :interpolation 'bi')"
    sc = load(files, "(material :name 'm' :type 'orennayar' :roughness (add 'nope' 0.375))")
    assert (sc.desc.materials[0].flags, sc.desc.materials[0].roughness_x) == (0, 0.375)
    assert len(sc.warnings) == 1 and "unknown node 'nope'" in sc.warnings[0] and "default value used" in sc.warnings[0]
    sc = load(files, colour + "(material :name 'm' :type 'orennayar' :roughness (add 'col' 0.375))")
    assert (sc.desc.materials[0].flags, sc.desc.materials[0].roughness_x) == (0, 0.375)
    assert len(sc.warnings) == 1 and "'col'" in sc.warnings[0] and "not a scalar node" in sc.warnings[0] and "default value used" in sc.warnings[0]
    sc = load(files, "(material :name 'm' :type 'orennayar' :roughness (add 0.375))")                  # a missing operand: 0
    assert (sc.desc.materials[0].flags, sc.desc.materials[0].roughness_x, sc.warnings) == (0, 0.375, [])
    sc = load(files, TEX + "(material :name 'm' :type 'orennayar' :roughness (max 'tex'))")             # ... beside a texture: the constant leaf 0
    d = sc.desc
    n = d.spectra[int(d.materials[0].roughness_x)]
    assert n.kind == abi.SPEC_SCALAR_MAX and d.spectra[n.lhs].kind == abi.SPEC_SCALAR_IMAGE and (d.spectra[n.rhs].kind, d.spectra[n.rhs].p[0]) == (abi.SPEC_CONST, 0.0)
    sc = load(files, "(material :name 'm' :type 'orennayar' :roughness (refl 1 1 1))")                  # a node that is not scalar: the parameter's default
    assert (sc.desc.materials[0].flags, sc.desc.materials[0].roughness_x) == (0, 0.5) and "not a scalar node" in sc.warnings[0]
    # NOT the reference's: on a material's own parameter a string that names no scalar node stays an error (a mistyped roughness map would render as the default)
    refused(files, "(material :name 'm' :type 'roughconductor' :roughness 'nope')", -4, "must be a number")
    refused(files, colour + "(material :name 'm' :type 'principled' :metallic 'col')", -4, "must be a number")


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------
def balanced(depth):
    return "'tex'" if depth == 0 else "(add %s %s)" % (balanced(depth - 1), balanced(depth - 1))


def chain(n):
    text = "'tex'"
    for _ in range(n):
        text = "(add %s 'tex')" % text
    return text


def test_the_loader_refuses_by_name(files):
    rough = "(material :name 'm' :type 'roughconductor' :roughness %s)"
    refused(files, TEX + rough % "(tanh 'tex')", -4, "a dynamic 'tanh'")
    refused(files, TEX + rough % "(add 0.5 (atan2 'tex' 2))", -4, "a dynamic 'atan2'")
    mix = "(material :name 'a' :type 'diffuse') (material :name 'b' :type 'mirror') (material :name 'm' :type 'blend' :material1 'a' :material2 'b' :factor %s)"
    refused(files, TEX + mix % "'tex'", -4, ":factor")
    refused(files, TEX + mix % "(mul 'tex' 0.5)", -4, ":factor")
    refused(files, TEX + "(material :name 'm' :type 'diffuse' :albedo (smul (div 'tex' 2) 0.5))", -4, "a scalar node ('div') where a spectrum is expected")
    refused(files, TEX + "(material :name 'm' :type 'diffuse' :albedo (sblend (mul 'tex' 2) 0.5 0.25))", -4, "factor")
    refused(files, TEX + "(material :name 'm' :type 'diffuse' :albedo (blackbody (mul 'tex' 6500)))", -4, "temperature")
    refused(files, TEX + "(material :name 'm' :type 'diffuse' :albedo (peak 550 (mul 'tex' 40)))", -4, "radius")
    for t in ("perlin", "noise", "expr"):
        refused(files, TEX + rough % ("(%s 'tex')" % t), -4, "'%s'" % t)
    refused(files, TEX + rough % "'tex'" + "(entity :name 'b' :type 'sphere' :material 'm')", -4, "scalar textures on sphere entities")
    leaf = "(material :name 'l' :type 'diffuse')" + rough % "'tex'"
    refused(files, TEX + leaf + "(material :name 'x' :type 'blend' :material1 'l' :material2 'm') (entity :name 'b' :type 'sphere' :material 'x')", -4, "sphere entities")
    # the two bounds of the device evaluator: a balanced tree of depth 4 needs 5 entries; 32 operators over 33 leaves are 65 words
    assert load(files, TEX + rough % balanced(abi.EXPR_MAX_STACK - 1)).desc.n_spectra == 1 + 3 + (2 ** (abi.EXPR_MAX_STACK - 1) - 1)
    refused(files, TEX + rough % balanced(abi.EXPR_MAX_STACK), -4, "PRGPU_EXPR_MAX_STACK")
    assert load(files, TEX + rough % chain((abi.EXPR_MAX_PROGRAM - 1) // 2)).desc.n_spectra == 1 + 3 + (abi.EXPR_MAX_PROGRAM - 1) // 2
    refused(files, TEX + rough % chain(abi.EXPR_MAX_PROGRAM // 2), -4, "PRGPU_EXPR_MAX_PROGRAM")
    refused(files, TEX + "(node :name 'tex' :type 'add' 1 2)", -1, "already exists")


def test_scene_builder_refuses_the_same():
    b = scene.SceneBuilder(8, 8)
    tex = b.scalar_image(F([[0.5]]))
    with pytest.raises(ValueError, match="a dynamic 'tanh'"):
        b.scalar_op("tanh", tex)
    level = [tex] * 2 ** abi.EXPR_MAX_STACK
    with pytest.raises(ValueError, match="PRGPU_EXPR_MAX_STACK"):
        while len(level) > 1:
            level = [b.scalar_op("add", level[i], level[i + 1]) for i in range(0, len(level), 2)]
    node = tex
    with pytest.raises(ValueError, match="PRGPU_EXPR_MAX_PROGRAM"):
        for _ in range(abi.EXPR_MAX_PROGRAM // 2):
            node = b.scalar_op("add", node, tex)


def one_triangle(material):
    b = scene.SceneBuilder(8, 8)
    b.add_mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 1, 2]], material(b), uvs=[[0, 0], [1, 0], [0, 1]])
    return b


def sphere_with(material):
    b = scene.SceneBuilder(8, 8)
    b.add_sphere(material(b))
    return b


def forward_operand(b):
    b.spectrum_const(0.5)
    return b.oren_nayar(b.spectrum_const(0.5), scene.ScalarNode(b._add_spec(kind=abi.SPEC_SCALAR_NEG, lhs=3, rhs=abi.INVALID_ID)))


def too_deep(b):
    tex = b.scalar_image(F([[0.5]])).id
    level = [tex] * 2 ** abi.EXPR_MAX_STACK
    while len(level) > 1:
        level = [b._add_spec(kind=abi.SPEC_SCALAR_ADD, lhs=level[i], rhs=level[i + 1]) for i in range(0, len(level), 2)]
    return b.oren_nayar(b.spectrum_const(0.5), scene.ScalarNode(level[0]))


def too_long(b):
    tex = node = b.scalar_image(F([[0.5]])).id
    for _ in range(abi.EXPR_MAX_PROGRAM // 2):
        node = b._add_spec(kind=abi.SPEC_SCALAR_ADD, lhs=node, rhs=tex)
    return b.oren_nayar(b.spectrum_const(0.5), scene.ScalarNode(node))


def blend_with_a_bound_factor(b):
    m = b.blend(b.lambert(b.spectrum_const(0.5)), b.mirror(), 0.5)
    b.materials[m].roughness_x = float(b.scalar_image(F([[0.5]])).id)
    b.materials[m].flags = abi.MATF_NODE_ROUGHNESS_X
    return m


def bit_on_a_lambert(b):
    m = b.lambert(b.spectrum_const(0.5))
    b.materials[m].roughness_x = float(b.scalar_image(F([[0.5]])).id)
    b.materials[m].flags = abi.MATF_NODE_ROUGHNESS_X
    return m


def short_table(b):
    tex = b.scalar_image(F([[0.5, 0.25]]))
    b.spectra[tex.id].lhs = 3                      # a width the table does not hold
    return b.oren_nayar(b.spectrum_const(0.5), tex)


@pytest.mark.parametrize("label,scene_of,code,needle", [
    ("a scalar kind on albedo", lambda: one_triangle(lambda b: b.lambert(b.scalar_image(F([[0.5]])).id)), -4, "where a spectrum is expected"),
    ("a scalar kind on a conductor's k", lambda: one_triangle(lambda b: b.conductor(k=b.scalar_image(F([[0.5]])).id)), -4, "where a spectrum is expected"),
    ("a scalar kind below a spectral operator", lambda: one_triangle(lambda b: b.lambert(b.spectrum_op("sadd", b.scalar_image(F([[0.5]])).id, b.spectrum_const(1.0)))), -4,
     "where a spectrum is expected"),
    ("a scalar kind as an emission", lambda: one_triangle(lambda b: (b.diffuse_emission(b.scalar_image(F([[0.5]])).id), b.lambert(b.spectrum_const(0.5)))[1]), -4,
     "where a spectrum is expected"),
    ("a binding to an index past the array", lambda: one_triangle(lambda b: b.oren_nayar(b.spectrum_const(0.5), scene.ScalarNode(999))), -1, "index of a node"),
    ("a binding to a spectral node", lambda: one_triangle(lambda b: b.oren_nayar(b.spectrum_const(0.5), scene.ScalarNode(0))), -1, "must name a scalar node"),
    ("an operand behind the operator", lambda: one_triangle(forward_operand), -1, "operands must precede"),
    ("a spectral operand of a scalar operator",
     lambda: one_triangle(lambda b: b.oren_nayar(b.refl(0.2, 0.4, 0.6), scene.ScalarNode(b._add_spec(kind=abi.SPEC_SCALAR_ABS, lhs=0, rhs=abi.INVALID_ID)))), -1, "where a scalar is expected"),
    ("a constant operand that is not finite",
     lambda: one_triangle(lambda b: b.oren_nayar(b.spectrum_const(float("inf")), scene.ScalarNode(b._add_spec(kind=abi.SPEC_SCALAR_ABS, lhs=0, rhs=abi.INVALID_ID)))), -1, "must be finite"),
    ("a stack one over the bound", lambda: one_triangle(too_deep), -4, "PRGPU_EXPR_MAX_STACK"),
    ("a program over the bound", lambda: one_triangle(too_long), -4, "PRGPU_EXPR_MAX_PROGRAM"),
    ("a bit on a field the kind does not read", lambda: one_triangle(bit_on_a_lambert), -1, "does not read"),
    ("a node on a blend's factor", lambda: one_triangle(blend_with_a_bound_factor), -4, "factor"),
    ("a table shorter than the image", lambda: one_triangle(short_table), -1, "W H + 1 floats"),
    ("a scalar texture on a sphere entity", lambda: sphere_with(lambda b: b.rough_conductor(b.scalar_image(F([[0.5]])))), -4, "sphere entities"),
])
def test_validation_refuses(label, scene_of, code, needle):
    with pytest.raises(abi.PrgpuError) as e:
        backend.RenderContext(scene_of().build(), device=0)
    assert ("prgpu error %d:" % code) in str(e.value) and needle in str(e.value), (label, str(e.value))


def test_a_scalar_image_below_a_scalar_operator_passes_validation_unlike_the_spectral_case():
    """up to the device: whatever comes back is not the validation's refusal of the description"""
    b = one_triangle(lambda b: b.oren_nayar(b.spectrum_const(0.5), b.scalar_op("mul", b.scalar_image(F([[0.5, 0.25]])), 0.5)))
    try:
        backend.RenderContext(b.build(), device=0).close()
    except abi.PrgpuError as e:
        assert ("prgpu error %d:" % -2) in str(e) or ("prgpu error %d:" % -3) in str(e), str(e)      # no device here


# ---- the reference's own example ---------------------------------------------------------------------------------------------------------------------
REFERENCE_EXAMPLES = "/root/reference/examples"


@pytest.mark.skipif(not os.path.isdir(REFERENCE_EXAMPLES), reason="the reference checkout is not on this machine")
def test_the_reference_example_with_roughness_maps_loads():
    sc = scene.PrcScene(path=os.path.join(REFERENCE_EXAMPLES, "cornellbox_substrate.prc"))
    d = sc.desc
    bound = [d.materials[i] for i in range(d.n_materials) if d.materials[i].flags & abi.MATF_NODE_MASK]
    assert sorted(m.kind for m in bound) == [abi.MAT_ROUGH_CONDUCTOR, abi.MAT_PRINCIPLED]                 # Metal-roughness, Wood-roughness
    assert all(m.flags & abi.MATF_NODE_ROUGHNESS_X and d.spectra[int(m.roughness_x)].kind == abi.SPEC_SCALAR_IMAGE for m in bound)
    assert any("'Metal-albedo'" in w and "default value used" in w for w in sc.warnings)                  # never declared: the reference's default
