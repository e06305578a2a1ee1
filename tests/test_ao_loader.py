"""The ambient occlusion integrator's host side without a GPU: the .prc loader accepts `(integrator :type 'ao' ...)` and reports it
(prgpu_prc_integrator), force_direct and the refused integrators behave as before, the entry points check their arguments, and the
analytic helper the GPU tests measure the occlusion against agrees with a Monte-Carlo estimate."""
import ctypes as C

import numpy as np
import pytest

import ao_helpers as H
from pearray_amd import _cabi as abi
from pearray_amd import scene

SOURCE = """(scene :render_width 8 :render_height 8
  (camera :name 'c' :type 'standard')
  (material :name 'm' :type 'diffuse')
  (mesh :name 'q' (attribute :type 'p' [0,0,0],[1,0,0],[0,1,0]) (faces [0,1,2]))
  %s
  (entity :name 'e' :type 'mesh' :mesh 'q' :materials 'm')
)"""


def integrator_of(block, **options):
    s = scene.PrcScene(source=SOURCE % block, **options)
    kind, count = C.c_uint32(99), C.c_uint32(99)
    assert abi.load().prgpu_prc_integrator(s._h, C.byref(kind), C.byref(count)) == 0
    assert (s.integrator, s.ao_sample_count) == (kind.value, count.value)   # PrcScene carries what the library reports
    return kind.value, count.value, s


def test_an_ao_block_loads_and_is_reported():
    h = C.c_void_p()
    lib = abi.load()
    assert lib.prgpu_prc_load_string((SOURCE % "(integrator :type 'ao' :sample_count 32)").encode(), None, None, C.byref(h)) == 0, lib.prgpu_prc_last_error()
    kind, count = C.c_uint32(), C.c_uint32()
    assert lib.prgpu_prc_integrator(h, C.byref(kind), C.byref(count)) == 0 and (kind.value, count.value) == (abi.INTEGRATOR_AO, 32)
    assert lib.prgpu_prc_integrator(h, None, None) == 0 and lib.prgpu_prc_integrator(None, C.byref(kind), C.byref(count)) == -1
    lib.prgpu_prc_free(h)


@pytest.mark.parametrize("block,want", [("(integrator :type 'occlusion' :sample_count 3)", 3), ("(integrator :type 'AMBIENT_OCCLUSION' :sample_count 1)", 1),
                                        ("(integrator :type 'ao')", 10), ("(integrator :type 'Ao' :max_ray_depth 2)", 10)])
def test_aliases_and_the_default_sample_count(block, want):
    kind, count, s = integrator_of(block)
    assert (kind, count) == (abi.INTEGRATOR_AO, want) and not s.warnings
    ref = abi.default_settings(8, 8)   # the `direct` parameters keep their defaults
    assert (s.settings.max_ray_depth, s.settings.soft_max_ray_depth, s.settings.nee, s.settings.mis) == (ref.max_ray_depth, ref.soft_max_ray_depth, ref.nee, ref.mis)


def test_direct_scenes_report_direct():
    assert integrator_of("")[:2] == (abi.INTEGRATOR_DIRECT, 0)
    assert integrator_of("(integrator :type 'direct' :max_ray_depth 5)")[:2] == (abi.INTEGRATOR_DIRECT, 0)


def test_force_direct_keeps_replacing_it_with_direct():
    kind, count, s = integrator_of("(integrator :type 'ao' :sample_count 32)", force_direct=True)
    assert (kind, count) == (abi.INTEGRATOR_DIRECT, 0)
    assert len(s.warnings) == 1 and s.warnings[0].endswith(": integrator 'ao' replaced by 'direct' with default parameters (force_direct)"), s.warnings


def test_other_integrators_stay_refused_and_a_zero_sample_count_is_invalid():
    for kind in ("vcm", "bidi", "ppm"):
        with pytest.raises(abi.PrgpuError) as e:
            scene.PrcScene(source=SOURCE % ("(integrator :type '%s')" % kind))
        assert e.value.args[1] == -4 and ("integrator '%s'" % kind) in e.value.args[0] and "ambient_occlusion" in e.value.args[0]
    with pytest.raises(abi.PrgpuError) as e:
        scene.PrcScene(source=SOURCE % "(integrator :type 'ao' :sample_count 0)")
    assert e.value.args[1] == -1 and "sample_count" in e.value.args[0]


def test_entry_points_check_their_arguments_without_a_gpu():
    lib = abi.load()
    assert lib.prgpu_enable_ambient_occlusion(None, 8) == -1 and b"null" in lib.prgpu_last_error()
    assert lib.prgpu_download_ao_counts(None, None) == -1
    assert lib.prgpu_download_ao_samples(None, None, None, None, None) == -1


def test_the_scene_builder_carries_the_integrator():
    b, white = H.builder(8, 8, 0, (0, -3, 1), (0, 0, 0))
    H.quad(b, white, [[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]])
    assert (b.build().integrator, b.build().ao_sample_count) == (abi.INTEGRATOR_DIRECT, 0)
    b.ambient_occlusion(7)
    assert (b.build().integrator, b.build().ao_sample_count) == (abi.INTEGRATOR_AO, 7)


@pytest.mark.parametrize("point", [(0.0, 0.0, 0.0), (0.0, 0.0, 0.7), (0.9, -0.4, 0.0), (2.5, 1.5, 0.3)])   # under the centre (twice), off-axis inside, outside the footprint
def test_the_rectangle_solid_angle_against_monte_carlo(point):
    x0, x1, y0, y1, z = -0.6, 0.8, -0.5, 0.5, 1.5
    omega = float(H.rect_solid_angle(np.array(point), x0, x1, y0, y1, z))
    rng = np.random.default_rng(20240607)
    n = 2_000_000
    u1, phi = rng.random(n), 2 * np.pi * rng.random(n)   # uniform hemisphere around +z: cos(theta) uniform
    st = np.sqrt(1 - u1 * u1)
    t = (z - point[2]) / np.maximum(u1, 1e-300)
    hx, hy = point[0] + t * st * np.cos(phi), point[1] + t * st * np.sin(phi)
    p_mc = float(((hx >= x0) & (hx <= x1) & (hy >= y0) & (hy <= y1)).mean())
    p = omega / (2 * np.pi)
    assert 0 < p < 1 and abs(p_mc - p) <= 5 * np.sqrt(p * (1 - p) / n), (p, p_mc)


def test_the_solid_angle_under_the_centre_of_a_square():
    for a, h in ((0.5, 1.0), (2.0, 0.25), (1.0, 1.0)):
        assert abs(float(H.rect_solid_angle(np.zeros(3), -a, a, -a, a, h)) - 4 * np.arcsin(a * a / (a * a + h * h))) < 1e-14
