"""The leaves of the BVH (pearray_amd/csrc/device/bvh.hip, PRGPU_BVH_LEAF=auto|3|1): `3` collapses a radix subtree of up to three triangles into one
128-byte leaf, `1` makes every triangle a single 64-byte leaf (pr_device.h: the third record kind; an analytic sphere or disk keeps a 128-byte leaf
of one), `auto` prices both.  Which records a ray visits never reaches a result -- a hit is argmin (t, primitive id) over the primitives that pass the
watertight test -- so every id and every frame must be the CPU checker's bit for bit under either policy, on four- and on six-wide trees."""
import ctypes as C

import numpy as np
import pytest

import oracle_binding as ob
import test_exact_rays as E
import test_gpu_bvh_width as W
import test_gpu_exact_rays as G
import test_gpu_parity as P
from pearray_amd import _cabi as abi
from pearray_amd import backend, scene
from test_gpu_parity import assert_parity, render_both

pytestmark = pytest.mark.gpu
POLICIES = ["3", "1"]
WIDTHS = ["4", "6"]


@pytest.fixture(params=POLICIES)
def leaf(request, monkeypatch):
    monkeypatch.setenv("PRGPU_BVH_LEAF", request.param)
    return request.param


@pytest.fixture(params=WIDTHS)
def width(request, monkeypatch):
    monkeypatch.setenv("PRGPU_BVH_WIDTH", request.param)
    return request.param


def _rays(n, seed, lo, hi, towards=None):
    rng = np.random.default_rng(seed)
    org = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3))
    if towards is not None:      # half of them aimed at points of the geometry
        k = rng.integers(0, len(towards), n // 2)
        d[: n // 2] = towards[k] - org[: n // 2]
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return org, d


def _ids_against_brute_force(sc, org, d, shadow=True):
    g, o = backend.RenderContext(sc), ob.OracleScene(sc)
    try:
        got, want = g.traceRays(org, d, 1e-4, np.inf), o.trace_closest(org, d, 1e-4, np.inf, brute=True)
        for x, y in zip(got, want):
            assert np.array_equal(x, y)
        if shadow:
            rng = np.random.default_rng(3)
            dist = np.where(want[0] != abi.INVALID_ID, want[4] * rng.choice([0.5, 1.0, 2.0], len(org)), 5.0).astype(np.float32)
            assert np.array_equal(g.traceShadowRays(org, d, 1e-4, dist), o.trace_any(org, d, 1e-4, dist, brute=True))
        return got
    finally:
        g.close(); o.close()


def _mesh_scene(pos, faces, w=32, h=32, spp=2):
    b = scene.SceneBuilder(w, h)
    b.settings.aa_samples = spp
    b.add_mesh(np.asarray(pos, dtype=np.float32), np.asarray(faces, dtype=np.uint32), b.lambert(b.spectrum_const(0.5)), emission=b.diffuse_emission(b.spectrum_const(2.0)))
    return b.build()


def _fan(n):
    """n separate triangles in front of the default camera, spread so that the radix tree has something to split"""
    rng = np.random.default_rng(40 + n)
    c = rng.uniform([-0.8, -0.8, 2.5], [0.8, 0.8, 3.5], (n, 3))
    tri = np.array([[-0.3, -0.3, 0.0], [0.3, -0.3, 0.0], [0.0, 0.3, 0.0]])
    pos = (c[:, None, :] + tri[None]).reshape(-1, 3)
    return pos, np.arange(3 * n).reshape(n, 3)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_tiny_scenes(leaf, width, monkeypatch, n):
    """The n <= 3 path (one record, one leaf -- under policy 1 only n = 1 takes it) and the first real splits."""
    pos, faces = _fan(n)
    sc = _mesh_scene(pos, faces)
    for split in ("1", "0"):
        monkeypatch.setenv("PRGPU_TRACE_SPLIT", split)
        org, d = _rays(2000, n, [-1, -1, 0], [1, 1, 2], towards=pos)
        _ids_against_brute_force(sc, org, d)
    g, o = render_both(sc, iters=2)
    assert_parity(g, o, exact=True)
    g.close(); o.close()


def test_ties(leaf, width, monkeypatch):
    """Two coincident triangles and two that share an edge sit in different leaves under policy 1: the lower index wins on equal t, and a ray
    through the shared edge hits exactly one of the two."""
    a = np.array([[-1.0, -1.0, 3.0], [1.0, -1.0, 3.0], [1.0, 1.0, 3.0]])
    b = np.array([[-1.0, -1.0, 3.0], [1.0, 1.0, 3.0], [-1.0, 1.0, 3.0]])     # shares the diagonal with a
    far = np.array([[3.0, 3.0, 5.0], [4.0, 3.0, 5.0], [3.0, 4.0, 5.0]])
    pos = np.concatenate([a, a, b, far, far + 1.0])          # triangles 0 and 1 coincide; 0 / 1 and 2 share an edge
    sc = _mesh_scene(pos, np.arange(15).reshape(5, 3))
    rng = np.random.default_rng(8)
    s = rng.uniform(-1, 1, 400)
    on_edge = np.stack([s, s, np.full_like(s, 3.0)], axis=1)                  # points of the shared diagonal
    inside = np.stack([rng.uniform(0.1, 0.9, 400), rng.uniform(-0.9, -0.1, 400), np.full(400, 3.0)], axis=1)    # inside a (and its twin)
    tgt = np.concatenate([on_edge, inside])
    org = (tgt + rng.uniform([-0.5, -0.5, -3.5], [0.5, 0.5, -2.0], tgt.shape)).astype(np.float32)
    d = tgt - org
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    for split in ("1", "0"):
        monkeypatch.setenv("PRGPU_TRACE_SPLIT", split)
        ent, prim, u, v, t = _ids_against_brute_force(sc, org, d)
        assert (prim[400:] == 0).all()                        # the twin with the lower index
        hit = ent[:400] != abi.INVALID_ID
        assert hit.all() and np.isin(prim[:400], (0, 2)).all()   # exactly one of the two neighbours (the service reports one hit per ray), never the twin


DISK_T = np.eye(4, dtype=np.float32); DISK_T[:3, 3] = (-1.2, 0.1, 2.6)
DISK_R = 0.4


def _mixed_scene(with_disk, w=32, h=32):
    """About 200 triangles in the middle (entity 0), a sphere to the right (1) and -- listed last, so that the other ids do not move -- a disk to the left (2),
    nearer than everything a ray towards it could hit behind it."""
    b = scene.SceneBuilder(w, h)
    b.settings.aa_samples = 2
    m = b.lambert(b.spectrum_const(0.5))
    pos, faces = scene.triangle_soup(200, seed=7, size=0.15, lo=(-0.5, -0.9, 3.0), hi=(0.5, 0.9, 4.0))
    b.add_mesh(pos, faces, m, emission=b.diffuse_emission(b.spectrum_const(1.0)))
    T = np.eye(4, dtype=np.float32); T[:3, 3] = (1.2, 0.2, 3.0)
    b.add_sphere(m, radius=0.4, transform=T)
    if with_disk:
        b.add_disk(m, radius=DISK_R, transform=DISK_T)
    return b.build(), np.asarray(pos, dtype=np.float64)


def test_mixed_kinds_in_one_wave_step(leaf, width):
    """A sphere, a disk and 200 triangles in one tree: under policy 1 the analytic primitives keep 128-byte leaves between the single ones, and a bundle of
    64 rays spread over the three has lanes at either kind of leaf in the same step.  The CPU checker knows no disks: a ray that clearly hits the disk
    (exact classification of tests/exact_disk.py; nothing lies in front of the disk) must report it, a ray that clearly misses it must report what the
    checker's exhaustive test finds in the same scene without the disk."""
    import exact_disk as D
    sc, pos = _mixed_scene(True)
    without, _ = _mixed_scene(False)
    rng = np.random.default_rng(23)
    on_disk = DISK_T[:3, 3][None] + np.concatenate([rng.uniform(-0.5, 0.5, (300, 2)), np.zeros((300, 1))], axis=1)
    on_sphere = np.array([[1.2, 0.2, 3.0]]) + rng.uniform(-0.45, 0.45, (300, 3))
    org, d = _rays(64 * 40, 17, [-0.2, -0.2, 0.0], [0.2, 0.2, 0.5], towards=np.concatenate([pos, on_disk, on_sphere]))
    perm = rng.permutation(len(org))      # every bundle of 64 holds rays towards all three
    org, d = org[perm], d[perm]
    tab = D.classify(org, d, [D.centre32(DISK_T)], [D.normal32(DISK_T)], [np.float32(DISK_R)])
    t, rho = tab.t[:, 0], tab.rho[:, 0]
    hits_disk = (t > 1e-3) & (rho < 0.99 * DISK_R)
    misses_disk = ~(t > 0) | (rho > 1.01 * DISK_R)
    assert hits_disk.sum() > 100 and (hits_disk | misses_disk).mean() > 0.99
    g, o = backend.RenderContext(sc), ob.OracleScene(without)
    try:
        got, want = g.traceRays(org, d, 1e-4, np.inf), o.trace_closest(org, d, 1e-4, np.inf, brute=True)
        assert (got[0][hits_disk] == 2).all() and (got[1][hits_disk] == 0).all()
        assert np.allclose(got[4][hits_disk], t[hits_disk], rtol=1e-5)
        for x, y in zip(got, want):
            assert np.array_equal(x[misses_disk], y[misses_disk])
        kinds = set(np.unique(got[0][got[0] != abi.INVALID_ID]).tolist())
        assert kinds == {0, 1, 2}, kinds                          # the mesh, the sphere and the disk were all hit
        occ = g.traceShadowRays(org, d, 1e-4, 100.0)
        assert np.array_equal(occ[misses_disk], o.trace_any(org, d, 1e-4, np.full(len(org), 100.0, dtype=np.float32), brute=True)[misses_disk]) and occ[hits_disk].all()
    finally:
        g.close(); o.close()
    g, o = render_both(without, iters=2)       # (the sphere between single leaves, in the path kernel)
    assert_parity(g, o, exact=True)
    g.close(); o.close()


@pytest.mark.parametrize("n", [2, 4])
def test_the_last_unit_of_the_record_array_is_a_single_leaf(leaf, monkeypatch, n):
    """By construction: under policy 1 a mesh of two triangles is the root record (unit 0, unit 1 its pad) and ONE child group of two single leaves, units 2 and 3
    of an array of four units (bvh.hip: n_units = 2 + the group sizes, a group rounded up to an even count) -- the last unit of the allocation is a single leaf,
    with nothing behind it.  Four triangles in two well separated pairs: the radix root's two children hold two each, the four-wide collapse pulls the four
    grandchildren into the root record, units 2 .. 5 of six.  The builder's structure check passes (the scene is created; k_validate bounds every single leaf
    by the array's end) and the ids are exact.  (Policy 3 builds one 128-byte leaf or two there: the same rays, the same answers.)"""
    monkeypatch.setenv("PRGPU_BVH_WIDTH", "4")
    tri = np.array([[-0.3, -0.3, 0.0], [0.3, -0.3, 0.0], [0.0, 0.3, 0.0]])
    centres = np.array([[-0.6, -0.6, 2.5], [-0.5, -0.5, 2.7], [0.6, 0.6, 3.3], [0.5, 0.5, 3.5]])[:n] if n == 4 else np.array([[-0.5, -0.5, 2.5], [0.5, 0.5, 3.5]])
    pos = (centres[:, None, :] + tri[None]).reshape(-1, 3)
    sc = _mesh_scene(pos, np.arange(3 * n).reshape(n, 3))
    for split in ("1", "0"):
        monkeypatch.setenv("PRGPU_TRACE_SPLIT", split)
        org, d = _rays(4000, n, [-1, -1, 0], [1, 1, 2], towards=pos)
        _ids_against_brute_force(sc, org, d)


def test_class_byte_two_queue_variant(leaf, width):
    """The material class travels in the leaf record (float 31 of a 128-byte leaf, float 10 of a single leaf) to the shade queues of the two-queue variant."""
    g, o = render_both(scene.cornell_rough(64, 36, spp=2), iters=2)
    assert_parity(g, o, exact=True)
    g.close(); o.close()


def test_c5_fixture_under_single_leaves(monkeypatch):
    monkeypatch.setenv("PRGPU_BVH_LEAF", "1")
    g, o = render_both(P._complex_c5(160, 90, 1), iters=1)
    assert_parity(g, o, exact=True)
    g.close(); o.close()


def test_deep_chain_under_single_leaves(monkeypatch):
    """The deep chain of test_gpu_bvh_width.py is deeper still with one triangle per leaf: it is rendered exactly by a tree that fits the traversal
    stack, or refused with the tree's bound and the stack's capacity in the message -- never walked with a stack it can overflow."""
    monkeypatch.setenv("PRGPU_BVH_LEAF", "1")
    lib = abi.load()
    sc = W._deep_chain_scene(duplicates=2000)
    for w in ("4", "6", "auto"):
        monkeypatch.setenv("PRGPU_BVH_WIDTH", w)
        h = C.c_void_p()
        rc = lib.prgpu_scene_create(C.byref(sc.desc), 0, C.byref(h))
        if rc != 0:
            assert b"stack" in lib.prgpu_last_error() and b"80" in lib.prgpu_last_error(), lib.prgpu_last_error()
            continue
        lib.prgpu_scene_destroy(h)
        g, o = render_both(sc, iters=2)
        assert 0 < g.pipelineInfo()["bvh_stack_bound"] <= 80, g.pipelineInfo()
        assert_parity(g, o, exact=True)
        g.close(); o.close()


@pytest.mark.parametrize("name", E.CASES)
def test_the_exact_reference_inputs(leaf, width, monkeypatch, name):
    for split in ("1", "0"):
        monkeypatch.setenv("PRGPU_TRACE_SPLIT", split)
        G.run_on_device(name, "leaf=%s split=%s" % (leaf, split))


@pytest.mark.parametrize("name", E.CAMERA_CASES)
def test_the_exact_reference_primary_hits(leaf, width, name):
    G.render_on_device(name, "leaf=%s" % leaf)


def test_axis_parallel_and_grazing_rays(leaf, width):
    """(The other adversarial inputs of tests/test_gpu_parity.py spend ten seconds and more each on the checker's side, too long for a case of this module: they
    run under policy 1 when the whole suite is run with PRGPU_BVH_LEAF=1 exported; the rays aimed at vertices and edges, the closed meshes and the windows are
    in the exact-reference inputs above.)"""
    P.test_axis_aligned_and_grazing_rays()


def test_deep_traversal_stacks(leaf, width, monkeypatch):
    """One triangle per leaf makes the tree deeper: the LDS window of the stack spills earlier, and the entries come back."""
    P.test_deep_traversal_stacks_spill_and_come_back(monkeypatch, "0")


def test_auto_builds_one_of_the_two_and_the_frame_does_not_depend_on_it(monkeypatch):
    b = scene.SceneBuilder(64, 64)
    b.settings.aa_samples = 2
    b.add_mesh(*scene.triangle_soup(2000, seed=5, size=0.1, lo=(-0.9, -0.9, 2.0), hi=(0.9, 0.9, 4.0)), b.lambert(b.spectrum_const(0.5)), emission=b.diffuse_emission(b.spectrum_const(1.0)))
    sc = b.build()
    frames, leaf_bytes = {}, {}
    for policy in ("3", "1", "auto"):
        monkeypatch.setenv("PRGPU_BVH_LEAF", policy)
        g = backend.RenderContext(sc)
        g.render(2); g.waitForFinish()
        frames[policy] = (g.output(), g.statistics())
        leaf_bytes[policy] = g.traceCounters()["leaf_bytes"]
        g.close()
    assert leaf_bytes["3"] == 128 and leaf_bytes["1"] == 64 and leaf_bytes["auto"] in (64, 128), leaf_bytes
    for policy in ("1", "auto"):
        assert frames[policy][1] == frames["3"][1]
        for x, y in zip(frames[policy][0], frames["3"][0]):
            assert np.array_equal(x, y)


def _counting_scene(with_sphere):
    """Twelve flat right triangles over a 3 x 3 grid of unit cells (three cells hold two, at different depths), each covering the half x + y < 1 of its cell, so
    that a ray along +z through the cell's point (0.75, 0.75) crosses the triangle's BOX and misses the triangle; optionally a unit sphere far to the right, whose
    box such a ray crosses at (0.75, 0.75) from its centre, 1.06 radii away from it.  Returns the scene and the primitives' boxes (lo, hi, is_sphere)."""
    b = scene.SceneBuilder(16, 16)
    b.settings.aa_samples = 1
    m = b.lambert(b.spectrum_const(0.5))
    pos, boxes = [], []
    for k in range(12):
        x0, y0, z = -1.5 + (k % 3), -1.5 + ((k // 3) % 3), 3.0 + 0.25 * k
        pos += [[x0, y0, z], [x0 + 1.0, y0, z], [x0, y0 + 1.0, z]]
        boxes.append(((x0, y0), (x0 + 1.0, y0 + 1.0), False))
    b.add_mesh(np.asarray(pos, dtype=np.float32), np.arange(36, dtype=np.uint32).reshape(12, 3), m, emission=b.diffuse_emission(b.spectrum_const(1.0)))
    if with_sphere:
        T = np.eye(4, dtype=np.float32); T[:3, 3] = (4.0, 0.0, 4.0)
        b.add_sphere(m, radius=1.0, transform=T)
        boxes.append(((3.0, -1.0), (5.0, 1.0), True))
    return b.build(), boxes


@pytest.mark.parametrize("with_sphere", [False, True], ids=["triangles", "mixed"])
@pytest.mark.parametrize("split", ["1", "0"])
def test_leaf_counters_equal_a_brute_force_walk(monkeypatch, with_sphere, split):
    """Ten fixed rays along +z that hit NOTHING: such a ray is never pruned (its limit stays infinite, an occlusion ray never ends early), so it fetches exactly
    the leaves whose boxes it crosses, whatever the order of the walk -- and those are counted here by an exhaustive test of the ray against every primitive's box,
    with no tree.  Every ray passes every box face at a distance of 0.25 or more, four times what the quantised child boxes add (a grid step is at most 1 / 127 of a record's
    extent, the scene is 6.5 wide), so the count does not depend on the quantisation either.  Under policy 1 `leaf_bytes` is 64 and the leaf counters equal that count, a
    128-byte leaf (the sphere's) counting as two records; the same rays as occlusion rays count the same into `leaves_any`."""
    monkeypatch.setenv("PRGPU_BVH_LEAF", "1")
    monkeypatch.setenv("PRGPU_TRACE_SPLIT", split)
    sc, boxes = _counting_scene(with_sphere)
    cells = [(-1.5 + i + 0.75, -1.5 + j + 0.75) for j in range(3) for i in range(3)]
    points = cells + [(4.75, 0.75) if with_sphere else (2.75, 2.75)]          # the sphere's box beside the sphere; or past everything
    g = backend.RenderContext(sc)
    try:
        assert g.traceCounters()["leaf_bytes"] == 64
        crossed_any = 0
        for px, py in points:
            want = 0
            for (lx, ly), (hx, hy), is_sphere in boxes:
                assert min(abs(px - lx), abs(px - hx), abs(py - ly), abs(py - hy)) >= 0.249           # nowhere near a face
                if lx < px < hx and ly < py < hy:
                    want += 2 if is_sphere else 1
            org, d = np.array([[px, py, 0.0]], dtype=np.float32), np.array([[0.0, 0.0, 1.0]], dtype=np.float32)
            a = g.traceCounters()
            ent = g.traceRays(org, d, 1e-4, np.inf)[0]
            b = g.traceCounters()
            occ = g.traceShadowRays(org, d, 1e-4, 100.0)
            c = g.traceCounters()
            assert ent[0] == abi.INVALID_ID and not occ[0]
            assert b["leaves_closest"] - a["leaves_closest"] == want, (px, py, want)
            assert c["leaves_any"] - b["leaves_any"] == want, (px, py, want)
            assert b["nodes_closest"] - a["nodes_closest"] >= 1 and b["rays_closest"] - a["rays_closest"] == 1 and c["rays_any"] - b["rays_any"] == 1
            crossed_any += want
        assert crossed_any == (12 + 2 if with_sphere else 12)        # every triangle's box once (two in three cells), the sphere's as two records
    finally:
        g.close()
    monkeypatch.setenv("PRGPU_BVH_LEAF", "3")
    g = backend.RenderContext(sc)
    assert g.traceCounters()["leaf_bytes"] == 128
    g.close()


def test_an_unknown_leaf_policy_is_refused(monkeypatch):
    monkeypatch.setenv("PRGPU_BVH_LEAF", "2")
    sc = scene.cornell_box(8, 8, spp=1)
    h = C.c_void_p()
    assert abi.load().prgpu_scene_create(C.byref(sc.desc), 0, C.byref(h)) == -1 and b"PRGPU_BVH_LEAF" in abi.load().prgpu_last_error()
