"""Disk entities on the host side, without a GPU: the .prc loader accepts `(entity :type 'disk' ...)` (disk.cpp:112-123: `:name`, `:radius` default 1,
`:material`, `:emission`, the transform) inside `(scene ...)` and in includes and describes it like a sphere -- kind PRGPU_ENTITY_DISK, the LOCAL radius, one
placeholder triangle --, other entity types are still refused, and SceneBuilder.add_disk assembles the same description."""
import ctypes as C

import numpy as np
import pytest

from pearray_amd import _cabi as abi
from pearray_amd import scene
from test_prc_loader import arr, struct_bytes

SOURCE = """(scene :render_width 8 :render_height 8
  (camera :name 'c' :type 'standard')
  (emission :name 'lamp' :type 'standard' :radiance 2)
  (material :name 'm' :type 'diffuse' :albedo 0.5)
  (material :name 'k' :type 'diffuse' :albedo 0)
  (mesh :name 'q' (attribute :type 'p' [0,0,0],[1,0,0],[0,1,0]) (faces [0,1,2]))
  (entity :name 'e' :type 'mesh' :mesh 'q' :materials 'm')
  %s
)"""
T = [1, 0, 0, 0.5, 0, -1, 0, 0.25, 0, 0, -1, 2, 0, 0, 0, 1]   # an exact pi rotation about x and a translation
DISKS = ("(entity :name 'd0' :type 'disk' :material 'm')"
         "(entity :name 'd1' :type 'disk' :radius 0.75 :material 'k' :emission 'lamp' :transform %s)" % str(T))


def check_disks(d):
    assert d.n_entities == 3 and d.n_triangles == 3 and d.n_vertices == 9
    e0, e1, e2 = d.entities[0], d.entities[1], d.entities[2]
    assert e0.kind == abi.ENTITY_MESH
    assert (e1.kind, e1.radius, e1.first_tri, e1.n_tris, e1.emission) == (abi.ENTITY_DISK, 1.0, 1, 1, abi.INVALID_ID)        # the default radius
    assert (e2.kind, e2.radius, e2.first_tri, e2.n_tris, e2.emission) == (abi.ENTITY_DISK, 0.75, 2, 1, 0)
    assert list(e1.transform) == np.eye(4).reshape(-1).tolist() and list(e2.transform) == [float(v) for v in T]
    assert arr(d.tri_material, 3, np.uint32).tolist() == [0, 0, 1]
    assert not arr(d.positions, 27, np.float32)[9:].any()                                                                      # the placeholders
    assert arr(d.indices, 9, np.uint32).tolist() == list(range(9))
    assert d.spectra[d.emissions[0].radiance].p[0] == 2.0 and d.spectra[d.materials[1].albedo].p[0] == 0.0


def test_a_disk_loads():
    assert abi.ENTITY_DISK == 4
    s = scene.PrcScene(source=SOURCE % DISKS)
    assert not s.warnings
    check_disks(s.desc)


def test_a_disk_loads_through_an_include(tmp_path):
    (tmp_path / "disks.inc").write_text(DISKS)
    s = scene.PrcScene(source=SOURCE % "(include 'disks.inc')", include_dir=str(tmp_path))
    check_disks(s.desc)


def test_other_entity_types_are_still_refused_and_the_message_lists_disk():
    for kind in ("subdiv", "curve", "disc"):
        with pytest.raises(abi.PrgpuError) as e:
            scene.PrcScene(source=SOURCE % ("(entity :name 'x' :type '%s' :material 'm')" % kind))
        assert e.value.args[1] == -4 and "entity type '%s' is not supported" % kind in e.value.args[0] and "disk" in e.value.args[0].split("is not supported")[1]


@pytest.mark.parametrize("radius", ["0", "-1", "1e-7"])
def test_a_radius_that_is_not_above_epsilon_is_refused(radius):
    """Disk::isValid (Disk.h:28-31) needs |radius| > PR_EPSILON, and the light's pdf is 0 unless radius > PR_EPSILON (disk.cpp:26)."""
    with pytest.raises(abi.PrgpuError) as e:
        scene.PrcScene(source=SOURCE % ("(entity :name 'x' :type 'disk' :radius %s :material 'm')" % radius))
    assert e.value.args[1] == -1 and "disk :radius" in e.value.args[0]
    ok = scene.PrcScene(source=SOURCE % "(entity :name 'x' :type 'disk' :radius 2e-7 :material 'm')")
    assert ok.desc.entities[1].radius == np.float32(2e-7)


def test_an_unknown_emission_is_refused_as_for_a_sphere():
    with pytest.raises(abi.PrgpuError) as e:
        scene.PrcScene(source=SOURCE % "(entity :name 'x' :type 'disk' :emission 'nope')")
    assert e.value.args[1] == -1 and "unknown emission" in e.value.args[0]


def test_the_scene_builder_assembles_the_same_arrays():
    loaded = scene.PrcScene(source=SOURCE % DISKS)   # (owns the description)
    d = loaded.desc
    b = scene.SceneBuilder(8, 8)
    lamp = b.diffuse_emission(b.spectrum_const(2.0))
    m, k = b.lambert(b.spectrum_const(0.5)), b.lambert(b.spectrum_const(0.0))
    b.add_mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 1, 2]], m)
    assert b.add_disk(m) == 1
    assert b.add_disk(k, radius=0.75, transform=np.asarray(T, dtype=np.float32).reshape(4, 4), emission=lamp) == 2
    w = b.build().desc
    for f in ("n_vertices", "n_triangles", "n_entities", "n_materials", "n_emissions", "n_spectra"):
        assert getattr(d, f) == getattr(w, f), f
    assert np.array_equal(arr(d.positions, 27, np.float32), arr(w.positions, 27, np.float32)) and np.array_equal(arr(d.indices, 9, np.uint32), arr(w.indices, 9, np.uint32))
    assert np.array_equal(arr(d.tri_material, 3, np.uint32), arr(w.tri_material, 3, np.uint32))
    for name, n in (("entities", 3), ("materials", 2), ("emissions", 1), ("spectra", d.n_spectra)):
        for i in range(n):
            assert struct_bytes(getattr(d, name)[i]) == struct_bytes(getattr(w, name)[i]), (name, i)


def test_the_description_is_validated_without_a_gpu():
    """prgpu_scene_create validates before it touches a device: two placeholder triangles, or a radius that is not above epsilon, are EINVAL."""
    lib = abi.load()
    for what in ("two", "radius", "nan"):
        b = scene.SceneBuilder(8, 8)
        m = b.lambert(b.spectrum_const(0.5))
        if what == "two":
            e = b.add_mesh([[0, 0, 0]] * 3, [[0, 1, 2], [0, 1, 2]], m)
            b.entities[e].kind, b.entities[e].radius = abi.ENTITY_DISK, 1.0
        else:
            b.add_disk(m, radius=1e-7 if what == "radius" else float("nan"))
        h = C.c_void_p()
        assert lib.prgpu_scene_create(C.byref(b.build().desc), 0, C.byref(h)) == -1 and b"disk entity" in lib.prgpu_last_error(), what
