"""The visual feedback integrator's host side without a GPU: the .prc loader accepts `(integrator :type 'vf' ...)` under its six names and
reports it (prgpu_prc_integrator, prgpu_prc_visual_feedback), the mode lookup follows the reference's table -- a missing :mode is
colored_entity_id (visualfeedback.cpp:50,291-301), names are case-insensitive --, the modes that are not built and unknown names are
refused by name, force_direct behaves as before, and the entry points check their arguments."""
import ctypes as C

import numpy as np
import pytest

from pearray_amd import _cabi as abi
from pearray_amd import scene

SOURCE = """(scene :render_width 8 :render_height 8
  (camera :name 'c' :type 'standard')
  (material :name 'm' :type 'diffuse')
  (mesh :name 'q' (attribute :type 'p' [0,0,0],[1,0,0],[0,1,0]) (faces [0,1,2]))
  %s
  (entity :name 'e' :type 'mesh' :mesh 'q' :materials 'm')
)"""
ALIASES = ("vf", "visual", "feedback", "visual_feedback", "visualfeedback", "debug")   # visualfeedback.cpp:331


def load(block, options=None):
    """(return code, handle) of prgpu_prc_load_string"""
    h = C.c_void_p()
    rc = abi.load().prgpu_prc_load_string((SOURCE % block).encode(), None, options, C.byref(h))
    return rc, h


def vf_of(block):
    """(kind, mode, weighting) as the library reports them; the PrcScene wrapper must carry the same"""
    lib = abi.load()
    rc, h = load(block)
    assert rc == 0, lib.prgpu_prc_last_error()
    kind, count, mode, weighting = C.c_uint32(99), C.c_uint32(99), C.c_uint32(99), C.c_int(99)
    assert lib.prgpu_prc_integrator(h, C.byref(kind), C.byref(count)) == 0 and count.value == 0
    assert lib.prgpu_prc_visual_feedback(h, C.byref(mode), C.byref(weighting)) == 0
    assert lib.prgpu_prc_visual_feedback(h, None, None) == 0
    lib.prgpu_prc_free(h)
    s = scene.PrcScene(source=SOURCE % block)
    assert (s.integrator, s.vf_mode, s.vf_weighting) == (kind.value, mode.value, bool(weighting.value)) and not s.warnings
    return kind.value, mode.value, weighting.value


def test_the_constants_follow_the_header():
    assert abi.INTEGRATOR_VF == 2 and len(abi.VF_MODE_NAMES) == 9
    assert [abi.VF_MODES[n] for n in ("colored_entity_id", "colored_displace_id", "ray_direction", "parameter", "inside", "ndotv")] == [0, 3, 5, 6, 7, 8]


@pytest.mark.parametrize("alias", ALIASES + ("VF", "Visual_Feedback"))
def test_every_type_alias_loads_as_vf(alias):
    assert vf_of("(integrator :type '%s' :mode 'inside')" % alias) == (abi.INTEGRATOR_VF, abi.VF_MODES["inside"], 1)


def test_a_missing_mode_is_colored_entity_id_not_parameter():
    # the table's last row is { "", ColoredEntityID } and the loop's end test never fires (visualfeedback.cpp:50,296): the plugin specification's
    # default `parameter` (:345) is not what the reference runs
    assert vf_of("(integrator :type 'vf')") == (abi.INTEGRATOR_VF, abi.VF_MODES["colored_entity_id"], 1)
    assert vf_of("(integrator :type 'vf' :mode '')")[1] == abi.VF_MODES["colored_entity_id"]


@pytest.mark.parametrize("name", abi.VF_MODE_NAMES)
def test_every_built_mode_by_name(name):
    assert vf_of("(integrator :type 'vf' :mode '%s')" % name)[1] == abi.VF_MODES[name]
    assert vf_of("(integrator :type 'vf' :mode '%s')" % name.upper())[1] == abi.VF_MODES[name]


def test_mode_names_are_case_insensitive_and_weighting_is_a_bool():
    assert vf_of("(integrator :type 'vf' :mode 'NdotV')")[1:] == (abi.VF_MODES["ndotv"], 1)
    assert vf_of("(integrator :type 'vf' :mode 'inside' :weighting false)")[1:] == (abi.VF_MODES["inside"], 0)
    assert vf_of("(integrator :type 'vf' :mode 'inside' :weighting true)")[1:] == (abi.VF_MODES["inside"], 1)


@pytest.mark.parametrize("mode", ["colored_ray_id", "validate_material", "nonsense", "Validate_Material"])
def test_modes_that_are_not_built_and_unknown_ones_are_refused_by_name(mode):
    lib = abi.load()
    rc, h = load("(integrator :type 'vf' :mode '%s')" % mode)
    assert rc == -4 and not h.value
    assert mode.lower().encode() in lib.prgpu_last_error() and mode.lower().encode() in lib.prgpu_prc_last_error()
    with pytest.raises(abi.PrgpuError) as e:
        scene.PrcScene(source=SOURCE % ("(integrator :type 'vf' :mode '%s')" % mode))
    assert e.value.args[1] == -4 and mode.lower() in e.value.args[0]


def test_force_direct_keeps_replacing_it_with_direct():
    s = scene.PrcScene(source=SOURCE % "(integrator :type 'vf' :mode 'colored_ray_id')", force_direct=True)   # (not even its mode is looked at)
    assert s.integrator == abi.INTEGRATOR_DIRECT and s.vf_mode is None
    assert len(s.warnings) == 1 and s.warnings[0].endswith(": integrator 'vf' replaced by 'direct' with default parameters (force_direct)"), s.warnings
    assert abi.load().prgpu_prc_visual_feedback(s._h, None, None) == -1


def test_other_scenes_are_not_vf():
    lib = abi.load()
    mode, weighting = C.c_uint32(77), C.c_int(77)
    for block in ("", "(integrator :type 'direct')", "(integrator :type 'ao' :sample_count 3)"):
        s = scene.PrcScene(source=SOURCE % block)
        assert s.integrator != abi.INTEGRATOR_VF and s.vf_mode is None
        assert lib.prgpu_prc_visual_feedback(s._h, C.byref(mode), C.byref(weighting)) == -1 and (mode.value, weighting.value) == (77, 77)
    assert lib.prgpu_prc_visual_feedback(None, C.byref(mode), C.byref(weighting)) == -1
    # a later block replaces an earlier one, in either direction
    assert scene.PrcScene(source=SOURCE % "(integrator :type 'vf') (integrator :type 'direct')").integrator == abi.INTEGRATOR_DIRECT
    assert scene.PrcScene(source=SOURCE % "(integrator :type 'ao') (integrator :type 'debug' :mode 'ndotv')").vf_mode == abi.VF_MODES["ndotv"]


def test_the_refusal_of_other_integrators_lists_vf():
    with pytest.raises(abi.PrgpuError) as e:
        scene.PrcScene(source=SOURCE % "(integrator :type 'vcm')")
    assert e.value.args[1] == -4 and "integrator 'vcm'" in e.value.args[0] and "visual_feedback" in e.value.args[0]


def test_entry_points_check_their_arguments_without_a_gpu():
    lib = abi.load()
    assert lib.prgpu_enable_visual_feedback(None, 0, 1) == -1 and b"null" in lib.prgpu_last_error()
    rgb = (C.c_float * 3)()
    assert lib.prgpu_visual_feedback_color(26, rgb) == -1 and lib.prgpu_visual_feedback_color(0, None) == -1


def test_the_colour_table():
    lib = abi.load()
    rows = np.zeros((26, 3), dtype=np.float32)
    for k in range(26):
        assert lib.prgpu_visual_feedback_color(k, rows[k].ctypes.data_as(C.POINTER(C.c_float))) == 0
    assert np.array_equal(rows[abi.VF_COLOR_GREEN], [0, 1, 0]) and np.array_equal(rows[abi.VF_COLOR_RED], [1, 0, 0]) and np.array_equal(rows[abi.VF_COLOR_BLUE], [0, 0, 1])
    # sRandomColors (visualfeedback.cpp:56-80): every triple holds 0.45 and 0.1125 and one value between them; all 23 differ; spot values
    r = rows[:23]
    assert (r.max(1) == np.float32(0.45)).all() and (r.min(1) == np.float32(0.1125)).all() and len({tuple(x) for x in r}) == 23
    assert np.array_equal(r[0], np.asarray([0.45, 0.37663, 0.1125], np.float32)) and np.array_equal(r[11], np.asarray([0.45, 0.288587, 0.1125], np.float32))
    assert np.array_equal(r[22], np.asarray([0.1125, 0.317935, 0.45], np.float32))


def test_the_scene_builder_carries_the_integrator():
    b = scene.SceneBuilder(8, 8)
    b.add_mesh(np.asarray([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), [[0, 1, 2]], b.lambert(b.spectrum_const(0.8)))
    assert (b.build().integrator, b.build().vf_mode) == (abi.INTEGRATOR_DIRECT, None)
    b.visual_feedback("NdotV", weighting=False)
    assert (b.build().integrator, b.build().vf_mode, b.build().vf_weighting) == (abi.INTEGRATOR_VF, abi.VF_MODES["ndotv"], False)
    b.visual_feedback(abi.VF_MODES["parameter"])
    assert (b.build().vf_mode, b.build().vf_weighting) == (abi.VF_MODES["parameter"], True)
