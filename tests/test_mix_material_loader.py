"""The Oren-Nayar, null, blend and add materials (PRGPU_MAT_OREN_NAYAR .. PRGPU_MAT_ADD, include/prgpu.h) on the host: the .prc loader's type names,
fields and defaults, SceneBuilder's records against the loader's, and what prgpu_scene_create's validation refuses -- it runs before any device
call, so a refusal needs no GPU.

A blend or add as the CHILD of a blend or add is refused by name (PRGPU_EUNSUPPORTED) in the loader, in SceneBuilder and in the validation.  No test
here pins that refusal, on purpose: the reference nests these materials, and a pinned refusal is what a later change that builds nesting would have
to break."""
import ctypes as C

import numpy as np
import pytest

from pearray_amd import _cabi as abi
from pearray_amd import backend, scene

SCENE = """(scene :render_width 8 :render_height 8
  (camera :name 'c' :type 'standard')
  %s
  (mesh :name 'q' (attribute :type 'p' [0,0,0],[1,0,0],[0,1,0]) (faces [0,1,2]))
  (entity :name 'e' :type 'mesh' :mesh 'q' :materials '%s')
)"""


_KEEP = []   # a description points into its PrcScene: the scenes of this module stay alive


def load(materials, used):
    _KEEP.append(scene.PrcScene(source=SCENE % (materials, used)))
    return _KEEP[-1]


def record(m):
    return C.string_at(C.addressof(m), C.sizeof(m))


def const_value(desc, spectrum):
    s = desc.spectra[spectrum]
    assert s.kind == abi.SPEC_CONST
    return s.p[0]


@pytest.mark.parametrize("name", ["orennayar", "oren", "rough"])
def test_oren_nayar_type_names_fields_and_defaults(name):
    d = load("(material :name 'a' :type '%s') (material :name 'b' :type '%s' :albedo (refl 0.2 0.5 0.7) :roughness 0.25)" % (name, name), "b").desc
    a, b = d.materials[0], d.materials[1]
    assert a.kind == b.kind == abi.MAT_OREN_NAYAR == 7
    assert const_value(d, a.albedo) == 1.0 and a.roughness_x == 0.5                       # orennayar.cpp:103-104
    assert d.spectra[b.albedo].kind == abi.SPEC_PARAMETRIC and b.roughness_x == 0.25
    for m in (a, b):
        assert (m.two_sided, m.ior, m.transmission, m.thin, m.k, m.flags, m.roughness_y) == (0, 0, 0, 0, 0, 0, 0.0) and not any(m.principled)


def test_oren_nayar_reads_albedo_under_that_key_only():
    """create() looks `albedo` up (orennayar.cpp:103); the `base` and `diffuse` of the plugin's specification are never read"""
    d = load("(material :name 'a' :type 'orennayar' :base (refl 0.2 0.5 0.7) :diffuse 0.25)", "a").desc
    assert const_value(d, d.materials[0].albedo) == 1.0


def test_oren_nayar_takes_a_checkerboard_albedo():
    d = load("(material :name 'a' :type 'oren' :albedo (checkerboard 0.25 0.75 4))", "a").desc
    assert d.spectra[d.materials[0].albedo].kind == abi.SPEC_CHECKER


def test_a_string_roughness_is_refused():
    with pytest.raises(abi.PrgpuError) as e:
        load("(material :name 'a' :type 'orennayar' :roughness 'tex')", "a")
    assert e.value.args[1] == -4 and "must be a number" in e.value.args[0], e.value.args


def test_null_loads():
    d = load("(material :name 'n' :type 'null')", "n").desc
    m = d.materials[0]
    assert m.kind == abi.MAT_NULL == 8 and m.albedo < d.n_spectra
    assert (m.two_sided, m.ior, m.transmission, m.thin, m.k, m.flags, m.roughness_x, m.roughness_y) == (0, 0, 0, 0, 0, 0, 0.0, 0.0)


@pytest.mark.parametrize("name,kind", [("blend", 9), ("mix", 9), ("add", 10)])
def test_combinators_resolve_two_earlier_names_to_their_indices(name, kind):
    mats = ("(material :name 'x' :type 'diffuse') (material :name 'first' :type 'mirror') (material :name 'second' :type 'orennayar')"
            "(material :name 'c' :type '%s' :material1 'second' :material2 'first')" % name)
    d = load(mats, "c").desc
    m = d.materials[3]
    assert m.kind == kind and (kind == abi.MAT_BLEND) == (name != "add")
    assert (m.two_sided, m.thin) == (2, 1)                                                    # material1, material2 (include/prgpu.h)
    assert m.roughness_x == (0.5 if kind == abi.MAT_BLEND else 0.0) and m.albedo < d.n_spectra   # blend.cpp:149: factor 0.5
    assert (m.ior, m.transmission, m.k, m.flags, m.roughness_y) == (0, 0, 0, 0, 0.0)
    assert np.ctypeslib.as_array(d.tri_material, shape=(1,))[0] == 3


def test_a_factor_arrives_as_given():
    """1.7 is clamped where the reference clamps it, at evaluation (blend.cpp:54,109; render.hip), not in the description"""
    mats = "(material :name 'a' :type 'diffuse') (material :name 'b' :type 'null') (material :name 'c' :type 'blend' :material1 'a' :material2 'b' :factor %s)"
    assert load(mats % "1.7", "c").desc.materials[2].roughness_x == np.float32(1.7)
    assert load(mats % "-0.25", "c").desc.materials[2].roughness_x == np.float32(-0.25)
    assert load(mats % "0", "c").desc.materials[2].roughness_x == 0.0


@pytest.mark.parametrize("name", ["blend", "add"])
@pytest.mark.parametrize("key", ["material1", "material2"])
def test_an_unknown_child_is_named(name, key):
    other = "material2" if key == "material1" else "material1"
    mats = "(material :name 'a' :type 'diffuse') (material :name 'c' :type '%s' :%s 'nowhere' :%s 'a')" % (name, key, other)
    with pytest.raises(abi.PrgpuError) as e:
        load(mats, "c")
    assert e.value.args[1] == -1 and "'nowhere'" in e.value.args[0], e.value.args


def test_a_child_declared_later_is_unknown():
    mats = "(material :name 'a' :type 'diffuse') (material :name 'c' :type 'blend' :material1 'a' :material2 'late') (material :name 'late' :type 'diffuse')"
    with pytest.raises(abi.PrgpuError) as e:
        load(mats, "c")
    assert e.value.args[1] == -1 and "'late'" in e.value.args[0], e.value.args


def test_ward_stays_refused_and_the_message_lists_the_new_types():
    with pytest.raises(abi.PrgpuError) as e:
        load("(material :name 'w' :type 'ward')", "w")
    msg = e.value.args[0]
    assert e.value.args[1] == -4 and "material type 'ward'" in msg
    for word in ("orennayar", "null", "blend", "add"):
        assert word in msg.split("is not supported")[1], msg


ALL_FOUR = """(material :name 'paper' :type 'orennayar' :albedo (refl 0.7 0.6 0.5) :roughness 0.8)
  (material :name 'hole' :type 'null')
  (material :name 'paint' :type 'diffuse' :albedo (refl 0.1 0.3 0.8))
  (material :name 'foil' :type 'conductor' :roughness 0.2)
  (material :name 'cutout' :type 'blend' :material1 'hole' :material2 'paper' :factor 0.3)
  (material :name 'coat' :type 'add' :material1 'paint' :material2 'foil')
  (material :name 'half' :type 'mix' :material1 'paint' :material2 'paper')"""


def test_scene_builder_assembles_the_loaders_records():
    d = load(ALL_FOUR, "half").desc
    b = scene.SceneBuilder(8, 8)
    paper = b.oren_nayar(b.refl(0.7, 0.6, 0.5), 0.8)
    hole = b.null()
    paint = b.lambert(b.refl(0.1, 0.3, 0.8))
    foil = b.rough_conductor(0.2)
    cutout = b.blend(hole, paper, 0.3)
    coat = b.add(paint, foil)
    half = b.blend(paint, paper)
    assert (paper, hole, paint, foil, cutout, coat, half) == tuple(range(7)) and d.n_materials == 7
    kinds = [d.materials[i].kind for i in range(7)]
    assert kinds == [abi.MAT_OREN_NAYAR, abi.MAT_NULL, abi.MAT_LAMBERT, abi.MAT_ROUGH_CONDUCTOR, abi.MAT_BLEND, abi.MAT_ADD, abi.MAT_BLEND]
    assert d.n_spectra == len(b.spectra)
    for i in range(7):
        assert record(d.materials[i]) == record(b.materials[i]), i
    for i in range(d.n_spectra):
        assert record(d.spectra[i]) == record(b.spectra[i]), i


def test_scene_builder_refuses_a_child_that_is_not_there_yet():
    b = scene.SceneBuilder(8, 8)
    a = b.lambert(b.spectrum_const(0.5))
    with pytest.raises(ValueError):
        b.blend(a, 1)
    with pytest.raises(ValueError):
        b.add(-1, a)


def one_triangle(material):
    """(builder, index of the material the triangle uses): materials 0 and 1 are Lambert, `material(b)` appends the one under test"""
    b = scene.SceneBuilder(8, 8)
    b.lambert(b.spectrum_const(0.5))
    b.lambert(b.spectrum_const(0.25))
    spec = b.spectrum_const(1.0)
    b.materials.append(material(spec))
    b.add_mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 1, 2]], 2)
    return b


@pytest.mark.parametrize("label,material,needle", [
    ("a forward child", lambda s: abi.Material(abi.MAT_BLEND, s, 0, 0, 0, 3, 0, 0, 0.5, 0.0), "smaller index"),
    ("itself as a child", lambda s: abi.Material(abi.MAT_ADD, s, 2, 0, 0, 1, 0, 0, 0.0, 0.0), "smaller index"),
    ("an infinite factor", lambda s: abi.Material(abi.MAT_BLEND, s, 0, 0, 0, 1, 0, 0, float("inf"), 0.0), "factor must be finite"),
    ("a NaN factor", lambda s: abi.Material(abi.MAT_BLEND, s, 0, 0, 0, 1, 0, 0, float("nan"), 0.0), "factor must be finite"),
    ("a NaN roughness", lambda s: abi.Material(abi.MAT_OREN_NAYAR, s, 0, 0, 0, 0, 0, 0, float("nan"), 0.0), "roughness must be finite"),
    ("a kind past the last one", lambda s: abi.Material(11, s, 0, 0, 0, 0, 0), "unknown material kind"),
])
def test_validation_refuses(label, material, needle):
    """prgpu_scene_create validates the description before it selects a device (prgpu_api.hip), so these return without one"""
    b = one_triangle(material)
    with pytest.raises(abi.PrgpuError) as e:
        backend.RenderContext(b.build(), device=0)
    code = -4 if needle in ("unknown material kind", "smaller index") else -1   # a forward reference is a description this backend does not take, not a malformed one
    assert ("prgpu error %d:" % code) in str(e.value) and needle in str(e.value), (label, str(e.value))
