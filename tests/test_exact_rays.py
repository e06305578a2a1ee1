"""The exact ray / triangle reference (tests/exact_rays.py): its own unit tests, and THE CPU CHECKER HELD TO IT.

Every traversal test of the suite compares the HIP kernels with the checker (oracle/pr_oracle.cpp), whose ray / triangle test is the same fp32
statement sequence as the device's: a mistake both share passes all of them.  Here the checker's `trace_closest` (exhaustive loop and BVH) and
`trace_any` answer the inputs below and are held to rules R1 - R6 of exact_rays.py against an arithmetic that shares nothing with them.
tests/test_gpu_exact_rays.py runs the same inputs and rules through the ray service on the device.

Inputs (all generated, seeded, fp32): 1 `soup` (30 000-triangle soup inside a box of 12 wall triangles, a second entity; 20 000 random rays),
2 `aimed` (the same scene, 5 000 rays aimed at vertices and edge points), 3 closed meshes for the watertightness rule (icosphere of 1 280 faces,
axis-aligned cube, rotated cube; each as it is, far from the origin at scale 300 and at scale 1e-3; rays from inside at every vertex, at three
points of every edge, and 1 ulp beside), 4 `axes` (fans of triangles on all six half-axes: every dominant axis and sign, ties, axis-parallel rays,
negative zeros), 5 `windings` (both windings, coincident triangles), 6 `window` (clear hits of input 1 with the window's ends 4 tau either side of
the exact distance), 7 `transformed` (a soup under a rotation and non-uniform scale), 8 `camera-*` (the primary-hit plane of one rendered iteration,
camera inside the icosphere and inside the soup's box, `uniform` sampler and single-tap filter: one known ray per pixel, R4 and R5).

Measured on the build host: this module 70 - 75 s (39 tests) next to the parent suite's 81 s -- over the half-again it was meant to stay within; nearly
all of it is the exact classification of the eighteen inputs, computed once each, and the numpy rule checks of the two checker runs per input."""
import numpy as np
import pytest

import exact_rays as X
import oracle_binding as ob
from pearray_amd import scene

INVALID = 0xFFFFFFFF
FAR_OFFSET, FAR_SCALE = (3.0e4, 1.0e4, -2.0e4), 300.0


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
class Case:
    """One input: meshes (positions, faces, 4 x 4 transform or None), rays with their windows, the distances of the occlusion queries, which rays
    must hit whatever the margins (R5), and whether the ray set is `random` (R4's cap) or `adversarial` (must be mostly non-clear)."""

    def __init__(self, name, meshes, org, direction, tmin, tmax, distance, must_hit=None, kind="other", any_must_be=None):
        self.name, self.meshes, self.kind = name, meshes, kind
        self.org, self.direction = np.ascontiguousarray(org, dtype=np.float32), np.ascontiguousarray(direction, dtype=np.float32)
        n = len(self.org)
        self.tmin = np.ascontiguousarray(np.broadcast_to(np.asarray(tmin, dtype=np.float32), (n,)))
        self.tmax = np.ascontiguousarray(np.broadcast_to(np.asarray(tmax, dtype=np.float32), (n,)))
        self.distance = np.ascontiguousarray(np.broadcast_to(np.asarray(distance, dtype=np.float32), (n,)))
        self.must_hit, self.any_must_be = must_hit, any_must_be
        self._geo = self._cls = None

    def build_scene(self):
        b = scene.SceneBuilder(8, 8)
        b.settings.aa_samples = 1
        for pos, faces, M in self.meshes:
            kw = {} if M is None else dict(transform=M)
            b.add_mesh(pos, faces, b.lambert(b.spectrum_const(0.5)), **kw)
        return b.build()

    def geometry(self):
        if self._geo is None:
            tris, ent, prim = [], [], []
            for e, (pos, faces, M) in enumerate(self.meshes):
                P = np.asarray(pos, dtype=np.float32).astype(np.float64)
                if M is not None:
                    M64 = np.asarray(M, dtype=np.float32).astype(np.float64).reshape(4, 4)
                    P = P @ M64[:3, :3].T + M64[:3, 3]
                f = np.asarray(faces, dtype=np.int64)
                tris.append(P[f]); ent.append(np.full(len(f), e)); prim.append(np.arange(len(f)))
            self._geo = X.Geometry(np.concatenate(tris), np.concatenate(ent), np.concatenate(prim), transformed=any(M is not None for _, _, M in self.meshes))
        return self._geo

    def classification(self):
        if self._cls is None:
            geo = self.geometry()
            self._cls = X.classify(self.org, self.direction, geo.tris, margin=geo.delta(self.org))
        return self._cls


def _unit32(v):
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def _walls():
    c = np.array([[x, y, z] for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (0.0, 2.0)], dtype=np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    faces = np.array([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], dtype=np.uint32)
    return c, faces


def _soup_meshes():
    pos, faces = scene.triangle_soup(30_000, seed=3)
    return [(pos, faces, None), _walls() + (None,)]


def input_soup():
    rng = np.random.default_rng(1)
    n = 20_000
    org = rng.random((n, 3)) * [1.9, 1.9, 1.85] + [-0.95, -0.95, 0.05]
    return Case("soup", _soup_meshes(), org, _unit32(rng.normal(size=(n, 3))), 1e-4, np.inf, rng.uniform(0.05, 2.5, n), kind="random")


def input_aimed():
    pos, faces = _soup_meshes()[0][:2]
    rng = np.random.default_rng(99)
    n = 5_000
    tri = rng.integers(0, len(faces), n)
    P = pos[faces[tri]].astype(np.float64)
    w = rng.random((n, 1))
    target = np.where(rng.random((n, 1)) < 0.7, P[:, 0], P[:, 1] * w + P[:, 2] * (1 - w))
    org = (rng.random((n, 3)) * [1.9, 1.9, 1.85] + [-0.95, -0.95, 0.05]).astype(np.float32)
    d = target - org.astype(np.float64)
    return Case("aimed", _soup_meshes(), org, _unit32(d), 1e-4, np.inf, np.linalg.norm(d, axis=1) * rng.uniform(0.5, 1.5, n), kind="adversarial")


def icosphere(levels=3):
    """20 x 4^levels faces; every vertex normalised in fp32 (no lattice structure)."""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(x, dtype=np.float64) for x in v]
    for _ in range(levels):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                mid[k] = len(v)
                v.append((v[a] + v[b]) / 2)
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    v = np.asarray(v, dtype=np.float32)
    v = v / np.sqrt((v * v).sum(1, dtype=np.float32))[:, None].astype(np.float32)
    return v.astype(np.float32), np.asarray(f, dtype=np.uint32)


def cube(rotated):
    c = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)], dtype=np.float64)
    if rotated:                                  # Rodrigues about (1, 2, 3) by sqrt(2) rad
        k = np.array([1.0, 2.0, 3.0]) / 14.0 ** 0.5
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        a = 2.0 ** 0.5
        c = c @ (np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K).T
    return c.astype(np.float32), _walls()[1]


def input_closed(shape, placement):
    pos, faces = icosphere() if shape == "icosphere" else cube(shape == "rotated_cube")
    offset, scale = {"unit": ((0.0, 0.0, 0.0), 1.0), "far": (FAR_OFFSET, FAR_SCALE), "tiny": ((0.0, 0.0, 0.0), 1e-3)}[placement]
    M = None
    if placement != "unit":
        M = np.eye(4, dtype=np.float32) * np.float32(scale); M[3, 3] = 1.0; M[:3, 3] = offset
    case = Case("tmp", [(pos, faces, M)], np.zeros((1, 3)), np.ones((1, 3)), 0, 1, 1)
    W = case.geometry().tris                                                                  # world triangles, float64
    inside = np.array([0.1, -0.2, 0.15]) if shape == "icosphere" else np.zeros(3)               # (the cubes: from the centre, so that rays lie in symmetry planes)
    o32 = (np.asarray(offset, dtype=np.float64) + scale * inside).astype(np.float32)
    edges = np.concatenate([W[:, [0, 1]], W[:, [1, 2]], W[:, [2, 0]]])
    targets = np.concatenate([W.reshape(-1, 3)] + [edges[:, 0] * (1 - s) + edges[:, 1] * s for s in (0.25, 0.5, 0.75)])
    targets = np.unique(targets, axis=0)
    d = _unit32(targets - o32.astype(np.float64))
    variants = [d]
    for axis in range(3):
        for to in (np.inf, -np.inf):
            e = d.copy()
            e[:, axis] = np.nextafter(d[:, axis], np.float32(to))
            variants.append(e)
    rng = np.random.default_rng(len(faces))                                                    # ... and at 300 points well inside faces: clear rays, for R1, R3, R4 and R6
    w = rng.dirichlet((4, 4, 4), 300)
    interior = (w[:, :, None] * W[rng.integers(0, len(W), 300)]).sum(1)
    d = np.concatenate(variants + [_unit32(interior - o32.astype(np.float64))])
    n = len(d)
    return Case("%s-%s" % (shape, placement), [(pos, faces, M)], np.broadcast_to(o32, (n, 3)), d, 1e-4 * scale, np.inf, 10.0 * scale,
                must_hit=np.ones(n, dtype=bool), kind="closed", any_must_be=True)


def input_axes():
    """Six fans of eight triangles, one on every half-axis at distance 2.5, each tilted against its axis (so that no ray meets one head-on), the
    hub of each EXACTLY on the axis.  Rays from around the origin at points inside the fans: every dominant axis and sign; rays along the axes
    through the hubs (a vertex shared by eight triangles; the other two components +0 and -0); exact ties |dx| = |dy| (= |dz|)."""
    rng = np.random.default_rng(44)
    pos, faces = [], []
    frames = []
    for axis in range(3):
        for sign in (1.0, -1.0):
            hub = np.zeros(3); hub[axis] = 2.5 * sign
            n = np.zeros(3); n[axis] = sign; n[(axis + 1) % 3] = 0.3; n[(axis + 2) % 3] = -0.2
            n /= np.linalg.norm(n)
            s = np.cross(n, np.eye(3)[(axis + 1) % 3]); s /= np.linalg.norm(s)
            t = np.cross(n, s)
            base = len(pos)
            pos.append(hub)
            for k in range(8):
                a = 2 * np.pi * k / 8 + 0.1
                pos.append(hub + 1.2 * (np.cos(a) * s + np.sin(a) * t))
            faces += [(base, base + 1 + k, base + 1 + (k + 1) % 8) for k in range(8)]
            frames.append((hub, s, t))
    pos = np.asarray(pos, dtype=np.float32)
    faces = np.asarray(faces, dtype=np.uint32)
    org, d, must = [], [], []
    for hub, s, t in frames:                       # random origins near the centre, at random points well inside the fan
        m = 1500
        o = rng.uniform(-0.3, 0.3, (m, 3)).astype(np.float32)
        r, a = 0.6 * np.sqrt(rng.random((m, 1))), rng.uniform(0, 2 * np.pi, (m, 1))
        target = hub + r * (np.cos(a) * s + np.sin(a) * t)
        target[: m // 10] = hub                      # a tenth of them at the hub itself
        target[m // 10: m // 5] = hub + rng.random((m // 5 - m // 10, 1)) * 0.6 * 1.2 * (np.cos(0.1) * s + np.sin(0.1) * t)   # ... and along a spoke
        org.append(o); d.append(_unit32(target - o.astype(np.float64))); must.append(np.ones(m, dtype=bool))
    z = np.zeros(3, dtype=np.float32)
    for axis in range(3):
        for sign in (1.0, -1.0):
            for z1 in (0.0, -0.0):
                for z2 in (0.0, -0.0):
                    e = np.empty(3, dtype=np.float32); e[axis] = sign; e[(axis + 1) % 3] = z1; e[(axis + 2) % 3] = z2
                    org.append(z[None]); d.append(e[None]); must.append(np.ones(1, dtype=bool))
    h, q = np.float32(0.70710677), np.float32(0.57735026)
    ties = [(sx * h, sy * h, 0.0) for sx in (1, -1) for sy in (1, -1)] + [(sx * h, 0.0, sz * h) for sx in (1, -1) for sz in (1, -1)] \
        + [(0.0, sy * h, sz * h) for sy in (1, -1) for sz in (1, -1)] + [(sx * q, sy * q, sz * q) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    ties = np.asarray(ties, dtype=np.float32)
    for _ in range(60):                            # the tied directions, each from two units before a point well inside the fan it heads for (not required to hit)
        o = np.empty((len(ties), 3))
        for k, e in enumerate(ties.astype(np.float64)):
            axis = int(np.nonzero(e)[0][0])
            hub, s, t = frames[2 * axis + (0 if e[axis] > 0 else 1)]
            r, a = 0.6 * np.sqrt(rng.random()), rng.uniform(0, 2 * np.pi)
            o[k] = hub + r * (np.cos(a) * s + np.sin(a) * t) - 2.0 * e
        org.append(o.astype(np.float32)); d.append(ties); must.append(np.zeros(len(ties), dtype=bool))
    org, d, must = np.concatenate(org), np.concatenate(d), np.concatenate(must)
    c = Case("axes", [(pos, faces, None)], org, d, 1e-4, np.inf, 6.0, must_hit=must)
    c.tied = np.arange(len(org) - 60 * len(ties), len(org))                                    # (test_the_tied_directions_meet_the_fans)
    return c


def input_windings():
    """The same triangle in both vertex orders (apart, so that each is met alone), and pairs of exactly coincident triangles: R4's lower index wins."""
    rng = np.random.default_rng(8)
    T = np.array([[-1.0, -1.0, 0.0], [1.2, -0.8, 0.1], [-0.2, 1.1, -0.1]])
    pos, faces = [], []
    for k, (order, z) in enumerate((((0, 1, 2), 1.0), ((0, 2, 1), 2.0), ((0, 1, 2), 3.0), ((0, 1, 2), 3.0), ((1, 2, 0), 4.0), ((1, 2, 0), 4.0), ((2, 1, 0), 5.0))):
        pos.append(T + [0, 0, z]); faces.append([3 * k + i for i in order])
    pos, faces = np.concatenate(pos).astype(np.float32), np.asarray(faces, dtype=np.uint32)
    n = 6000
    target = np.concatenate([rng.uniform(-0.6, 0.6, (n, 2)), rng.uniform(0.9, 5.1, (n, 1))], 1)
    org = np.concatenate([rng.uniform(-2, 2, (n, 2)), np.where(rng.random((n, 1)) < 0.5, rng.uniform(-1, 0.5, (n, 1)), rng.uniform(5.5, 7, (n, 1)))], 1).astype(np.float32)
    # windows that start between the layers, so that every layer is the nearest for some rays
    tmin = np.where(rng.random(n) < 0.5, 1e-4, rng.uniform(0.5, 4.0, n))
    return Case("windings", [(pos, faces, None)], org, _unit32(target - org.astype(np.float64)), tmin, np.inf, rng.uniform(1.0, 8.0, n))


def input_transformed():
    pos, faces = scene.triangle_soup(3000, seed=11, size=0.08, lo=(-1, -1, -1), hi=(1, 1, 1))
    k = np.array([2.0, -1.0, 0.5]) / np.linalg.norm([2.0, -1.0, 0.5])
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(1.1) * K + (1 - np.cos(1.1)) * K @ K
    M = np.eye(4, dtype=np.float32)
    M[:3, :3] = (R @ np.diag([1.5, 0.7, 2.2])).astype(np.float32)
    M[:3, 3] = (0.4, -0.3, 5.0)
    rng = np.random.default_rng(17)
    n = 8000
    org = (rng.uniform(-2.5, 2.5, (n, 3)) + [0.4, -0.3, 5.0]).astype(np.float32)
    target = rng.uniform(-1, 1, (n, 3)) @ M[:3, :3].astype(np.float64).T + [0.4, -0.3, 5.0]
    return Case("transformed", [(pos, faces, M)], org, _unit32(target - org.astype(np.float64)), 1e-4, np.inf, rng.uniform(0.5, 6.0, n), kind="random")


def input_window():
    """Clear hits of input 1 at exact distance t*: the window's far end at t* + 4 tau (reported) and t* - 4 tau (that triangle is outside), the near
    end likewise.  Same rays as input 1, so its classification is reused (the window is no part of it)."""
    base = case("soup")
    geo, cls = base.geometry(), base.classification()
    n = len(base.org)
    Q = X.qualifying(geo, cls, base.org, base.tmin.astype(np.float64), base.tmax.astype(np.float64))
    tstar = np.full(n, np.inf)
    np.minimum.at(tstar, cls.ray[Q], cls.t[Q])
    src = np.nonzero(np.isfinite(tstar))[0][:2500]
    t = tstar[src]
    tau = X.TAU_ULPS * X.EPS32 * np.maximum(t, X.ray_extent(base.org[src], geo.extent))
    src4 = np.concatenate([src] * 4)
    tmin = np.concatenate([np.full(len(src), 1e-4)] * 2 + [t - 4 * tau, t + 4 * tau])
    tmax = np.concatenate([t + 4 * tau, t - 4 * tau] + [np.full(len(src), np.inf)] * 2)
    c = Case("window", base.meshes, base.org[src4], base.direction[src4], np.maximum(tmin, 0), tmax, np.where(np.isfinite(tmax), tmax + 0.001, 10.0))
    c._geo = geo
    c._cls = cls.take(src4)
    return c


CLOSED = ["%s-%s" % (s, p) for s in ("icosphere", "cube", "rotated_cube") for p in ("unit", "far", "tiny")]
CASES = ["soup", "aimed"] + CLOSED + ["axes", "windings", "window", "transformed"]
_cache = {}


def case(name):
    """The input of that name with its exact classification, computed once per session."""
    if name not in _cache:
        if name in CLOSED:
            _cache[name] = input_closed(*name.rsplit("-", 1))
        elif name.startswith("camera-"):
            _cache[name] = input_camera(name.split("-")[1])
        else:
            _cache[name] = globals()["input_" + name]()
    return _cache[name]


def hold_to_the_rules(c, closest, occluded, label=""):
    """R1 - R6 and the caps for one tracer: closest(org, dir, tmin, tmax) -> (entity, prim, u, v, t), occluded(org, dir, tmin, distance) -> bool."""
    geo, cls = c.geometry(), c.classification()
    label = "%s %s" % (c.name, label)
    s = X.check_closest(geo, cls, c.org, c.direction, c.tmin.astype(np.float64), c.tmax.astype(np.float64), closest(c.org, c.direction, c.tmin, c.tmax),
                        must_hit=c.must_hit, label=label)
    occ = occluded(c.org, c.direction, c.tmin, c.distance)
    s["any_undecided"] = X.check_any(geo, cls, c.org, c.tmin.astype(np.float64), c.distance.astype(np.float64), occ, label=label)
    if c.any_must_be is not None:
        assert (occ == c.any_must_be).all(), "%s: occlusion query from inside a closed surface" % label
    print(label, s)
    # the caps: conditions on the reference and the inputs alone
    assert s["coplanar_skipped"] <= 0.001, (label, s)
    if c.kind == "random":
        assert s["r4_skipped"] <= 0.01, (label, s)
    if c.kind == "adversarial":
        assert s["non_clear"] >= 0.30, (label, s)
    return s


# ---- the reference's own tests --------------------------------------------------------------------------------------------------------------
F = np.float32
TRI = np.array([[[0, 0, 1], [1, 0, 1], [0, 1, 1]], [[1, 1, 1], [0, 1, 1], [1, 0, 1]]], dtype=np.float32)      # two triangles sharing the edge (1,0,1)-(0,1,1)


def _kinds(o, d, tris=TRI):
    cls = X.classify(np.asarray([o], dtype=F), np.asarray([d], dtype=F), tris)
    return {int(k): (int(x), float(t)) for k, x, t in zip(cls.tri, cls.kind, cls.t) if x > 0}       # (kind 0: near, not met)


def test_hand_built_cases():
    assert _kinds((0.25, 0.25, 0), (0, 0, 1)) == {0: (2, 1.0)}                                   # inside the first
    assert _kinds((0.75, 0.75, 0), (0, 0, 1)) == {1: (2, 1.0)}
    assert _kinds((0.5, 0.5, 0), (0, 0, 2)) == {0: (1, 0.5), 1: (1, 0.5)}                          # on the shared edge: touched on both, inside neither
    assert _kinds((0, 0, 0), (0, 0, 1)) == {0: (1, 1.0)}                                           # through a vertex
    assert _kinds((1, 0, 0), (0, 0, 1)) == {0: (1, 1.0), 1: (1, 1.0)}                              # through a shared vertex
    assert _kinds((2, 2, 0), (0, 0, 1)) == {}
    assert _kinds((-1, 0, 1), (1, 0, 0)) == {}                                                     # along an edge, in the plane: det == 0, never a hit
    assert _kinds((0.25, 0.25, 2), (0, 0, 1)) == {0: (2, -1.0)}                                    # the LINE is classified; the window belongs to the rules
    assert _kinds((0.25, 0.25, 0), (0, 0, 1), TRI[:, ::-1]) == {0: (2, 1.0)}                       # either winding
    deg = np.array([[[0, 0, 1], [1, 1, 1], [2, 2, 1]]], dtype=F)
    assert _kinds((1, 1, 0), (0, 0, 1), deg) == {}                                                 # a degenerate triangle is never pierced
    cls = X.classify(np.array([[0.25, 0.5, 0]], dtype=F), np.array([[0, 0, 1]], dtype=F), TRI[:1])
    assert (cls.u[0], cls.v[0]) == (0.25, 0.5)                                                     # P = (1 - u - v) p0 + u p1 + v p2


def test_coordinates_one_ulp_apart_are_told_apart():
    e = F(2.0 ** -23)
    one, up = F(1), F(1) + e
    tri = np.array([[[one, 0, 1], [up, 1, 1], [3, 0.5, 1]]], dtype=F)                              # an edge from x = 1 to x = 1 + 2^-23
    x_mid = F(1) + e                                                                               # at y = 0.5 the edge is at x = 1 + 2^-24: between two floats
    assert _kinds((one, 0.5, 0), (0, 0, 1), tri) == {}
    assert _kinds((x_mid, 0.5, 0), (0, 0, 1), tri) == {0: (2, 1.0)}
    assert _kinds((up, 1, 0), (0, 0, 1), tri) == {0: (1, 1.0)}
    assert X.classify(np.array([[one, 0.5, 0]], dtype=F), np.array([[0, 0, 1]], dtype=F), tri, margin=1e-6).kind.tolist() == [0]     # ... but near


def test_a_float64_zero_that_is_not_an_exact_zero():
    """fp32 values with short mantissas whose combination needs more than 53 bits: the ray from (2^-60, 0.5, 0) along (1, 0, 1) meets the plane z = 1
    at x = 1 + 2^-60, a hair inside the edge x = 1 of the triangle.  In float64 p0 - o rounds to (1, -0.5, 1) and the edge function is 0; the filter
    must know that it does not know, and the integers decide: strictly inside; ON the edge with the origin at x = 0; outside at x = -2^-60."""
    tri = np.array([[[1, 0, 1], [2, 0, 1], [1, 1, 1]]], dtype=F)
    d = np.array([[1, 0, 1]], dtype=np.float64)
    for x, kind in ((2.0 ** -60, 2), (0.0, 1), (-2.0 ** -60, 0)):
        o = np.array([[x, 0.5, 0]], dtype=F).astype(np.float64)
        E, B = X.pairs64(o, d, tri.astype(np.float64))[:2]
        assert (E[0] == 0.0).any() and (np.abs(E[0]) <= B[0]).any(), (E, B)
        e = X.exact_pair(o[0], d[0], *tri[0].astype(np.float64))
        assert (min(abs(v) for v in e[:3]) == 0) == (x == 0.0)
        k, t, u, v, n_exact = X.classify_pairs(o, d, tri.astype(np.float64))
        assert (int(k[0]), n_exact) == (kind, 1)
        assert abs(t[0] - 1.0) < 1e-15


def test_the_filter_agrees_with_all_exact():
    rng = np.random.default_rng(5)
    n = 3000
    P = rng.uniform(-1, 1, (n, 3, 3)).astype(F)
    o = rng.uniform(-1, 1, (n, 3)).astype(F)
    w = rng.dirichlet((1, 1, 1), n)
    w[: n // 3, 0] = 0; w[: n // 6, 1] = 0                                                          # a third aimed at an edge, a sixth at a vertex
    w /= w.sum(1, keepdims=True)
    target = (w[:, :, None] * P.astype(np.float64)).sum(1)
    d = _unit32(target - o)
    d[n // 2:] = _unit32(rng.normal(size=(n - n // 2, 3)))
    o64, d64, P64 = o.astype(np.float64), d.astype(np.float64), P.astype(np.float64)
    a = X.classify_pairs(o64, d64, P64)
    b = X.classify_pairs(o64, d64, P64, force_exact=True)
    assert b[4] == n and a[4] < n // 2
    assert np.array_equal(a[0], b[0])
    hit = b[0] > 0
    assert hit.sum() > n // 5
    for x, y in zip(a[1:4], b[1:4]):
        assert np.allclose(x[hit], y[hit], rtol=2.0 ** -39, atol=2.0 ** -39)
    # stage 1 loses no pair that stages 2 and 3 would keep
    r, k = X.candidate_pairs(o, d, P, 0.0)
    kept = set(zip(r.tolist(), k.tolist()))
    assert all((i, i) in kept for i in np.nonzero(hit)[0])
    every = X.classify_pairs(np.repeat(o64[:60], 60, 0), np.repeat(d64[:60], 60, 0), np.tile(P64[:60], (60, 1, 1)))[0].reshape(60, 60)
    assert all((i, j) in kept for i, j in zip(*np.nonzero(every > 0)))
    assert len(kept) < n * n // 4


def test_the_margins_hold_twice_over_for_an_fp32_restatement_of_the_watertight_test():
    """The rules' constants are bounds argued from the operation count; here they are checked against the exact reference on the CPU, with a numpy
    restatement of the fp32 statement sequence (not the checker, not the kernel) on the candidate pairs of inputs 1, 2, 3 (icosphere far away) and 7:
    a wrong accept / reject happens only within DELTA / 2 of an edge, an accepted pair's t is within TAU / 2 (+ the slide along the plane) of the exact
    one, its barycentrics are above -BARY_SLACK / 2."""
    for name in ("soup", "aimed", "icosphere-far", "transformed"):
        c = case(name)
        geo, cls = c.geometry(), c.classification()
        o, d, P = c.org[cls.ray].astype(np.float64), c.direction[cls.ray].astype(np.float64), geo.tris[cls.tri]
        ok, t, u, v = X.woop32(o, d, P.astype(F).astype(np.float64))     # (transformed entities: the fp32 world vertices are within TRANSFORM_ULPS of these)
        M = X.ray_extent(o, geo.extent)
        delta = geo.delta_ulps * X.EPS32 * M
        wrong_reject = (cls.kind == 2) & ~ok
        wrong_accept = (cls.kind == 0) & ok
        assert (cls.edge_dist[wrong_reject] <= delta[wrong_reject] / 2).all(), (name, (cls.edge_dist[wrong_reject] / delta[wrong_reject]).max())
        assert (cls.dist[wrong_accept] <= delta[wrong_accept] / 2).all(), (name, (cls.dist[wrong_accept] / delta[wrong_accept]).max())
        both = ok & (cls.kind == 2)
        slide = geo.slide(M, cls.sin_phi)
        both &= np.isfinite(slide)
        tau = X.TAU_ULPS * X.EPS32 * np.maximum(np.abs(cls.t), M)
        excess = np.abs(t.astype(np.float64) - cls.t)[both] / (tau + slide)[both]
        assert excess.max() <= 0.5, (name, excess.max())
        w = np.minimum(np.minimum(u, v), 1 - u.astype(np.float64) - v)[ok]
        assert w.min() >= -X.BARY_SLACK / 2, (name, w.min())
        print(name, "pairs", len(ok), "wrong rejects", int(wrong_reject.sum()), "wrong accepts", int(wrong_accept.sum()), "worst t error / (tau + slide)", excess.max(), "lowest weight", w.min())


# ---- the checker against the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("brute", [True, False], ids=["exhaustive", "bvh"])
@pytest.mark.parametrize("name", CASES)
def test_the_checker_is_held_to_the_exact_reference(name, brute):
    c = case(name)
    o = ob.OracleScene(c.build_scene())
    if brute and len(c.org) > 6000:            # the exhaustive loop: every k-th ray of the large sets, so that every kind of ray in them is there
        c = _subset(c, np.arange(0, len(c.org), -(-len(c.org) // 6000)))
    hold_to_the_rules(c, lambda *a: o.trace_closest(*a, brute=brute), lambda *a: o.trace_any(*a, brute=brute), "checker brute=%s" % brute)
    o.close()


def _subset(c, rays):
    """The rays `rays` of a case, with the rows of its classification."""
    h = Case(c.name, c.meshes, c.org[rays], c.direction[rays], c.tmin[rays], c.tmax[rays], c.distance[rays], None if c.must_hit is None else c.must_hit[rays], c.kind, c.any_must_be)
    h._geo = c.geometry()
    h._cls = c.classification().take(rays)
    return h


def test_the_tied_directions_meet_the_fans():
    """Input 4's exact ties |dx| = |dy| (= |dz|) are not required to hit; a good share of them must all the same have a CLEAR hit, or they test nothing."""
    c = case("axes")
    t = _subset(c, c.tied)
    clear = X.clear_rays(t.geometry(), t.classification(), t.org.astype(np.float64), t.tmin.astype(np.float64), t.tmax.astype(np.float64))[0]
    assert clear.mean() > 0.2, clear.mean()
    for k in range(len(c.tied) // 60):                                                         # every tied direction, for some origin
        assert clear[k::len(c.tied) // 60].any(), k


def test_the_closed_meshes_have_clear_rays_too():
    for name in CLOSED:
        c = case(name)
        clear = X.clear_rays(c.geometry(), c.classification(), c.org.astype(np.float64), c.tmin.astype(np.float64), c.tmax.astype(np.float64))[0]
        assert clear[-300:].mean() > 0.9, (name, clear[-300:].mean())


# ---- input 8: the path kernel's primary rays ------------------------------------------------------------------------------------------------
# The perspective camera without a lens (oracle and device: d = normalize(right nx + up ny + dir), nx = 2 (px / W - 0.5), ny = -2 (py / H - 0.5), right and up
# scaled by half the sensor's width and height) with the `uniform` sampler (every sample at the pixel's 0.5, 0.5, and px = x + 0.5 - 0.5 = x) and a
# single-tap filter sends ONE known ray per pixel.  It is restated here in float64 and rounded: the kernel's own fp32 direction differs by the roundings of
# nx (3), of two products and two sums per component (4) and of the normalisation (3) -- <= 10 x 2^-24 relative per component, i.e. the line is up to
# sqrt(3) x 10 x 2^-24 x t beside the restated one at distance t <= the scene's diagonal 2 sqrt(3) M: 60 x 2^-24 x M more in DELTA (Geometry's extra_ulps).
CAMERA_ULPS = 60.0
CAMERA_CASES = ["camera-icosphere", "camera-soup"]


def input_camera(what):
    from pearray_amd import _cabi as abi
    W, H = 95, 63                                  # (odd: no pixel on the axes of the sensor)
    if what == "icosphere":
        meshes, eye, closed = [icosphere() + (None,)], (0.1, -0.2, 0.15), True
    else:
        meshes, eye, closed = _soup_meshes(), (0.0, 0.75, 1.0), True                            # (inside the box of walls: every pixel hits something)
    T = np.eye(4, dtype=np.float32); T[:3, 3] = eye
    cam = dict(width=1.6, height=1.6 * H / W, local_direction=(0, 1, 0), local_up=(0, 0, 1), local_right=(1, 0, 0))
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    nx, ny = 2 * (x / W - 0.5), -2 * (y / H - 0.5)
    d = nx[..., None] * (0.5 * cam["width"]) * np.array([1.0, 0, 0]) + ny[..., None] * (0.5 * cam["height"]) * np.array([0, 0, 1.0]) + np.array([0, 1.0, 0])
    n = W * H
    c = Case("camera-" + what, meshes, np.broadcast_to(np.asarray(eye, dtype=np.float32), (n, 3)), _unit32(d.reshape(n, 3)), 1e-6, np.inf, 1.0,
             must_hit=np.ones(n, dtype=bool) if closed else None, kind="random")
    geo = c.geometry()
    c._geo = X.Geometry(geo.tris, geo.entity, geo.prim, extra_ulps=CAMERA_ULPS)

    def build_scene():
        b = scene.SceneBuilder(W, H)
        s = b.settings
        s.aa_sampler, s.aa_samples, s.filter, s.filter_radius = abi.SAMPLER_UNIFORM, 1, abi.FILTER_BLOCK, 0
        for pos, faces, _ in meshes:
            b.add_mesh(pos, faces, b.lambert(b.spectrum_const(0.5)))
        b.set_camera(T, near=1e-6, **cam)
        return b.build()
    c.build_scene = build_scene
    return c


def hold_primary_hits_to_the_rules(c, ent, prim, label=""):
    s = X.check_identity(c.geometry(), c.classification(), c.org, c.tmin.astype(np.float64), c.tmax.astype(np.float64), ent, prim, must_hit=c.must_hit, label="%s %s" % (c.name, label))
    print(c.name, label, s)
    # (not the 1 % of a random ray set: DELTA is 76 ulp here instead of 16, and the slide of obliquely seen soup triangles grows with it -- 1.1 % on the soup,
    # a figure of the reference and the input alone, computed before any kernel ran; twice the random sets' cap)
    assert s["r4_skipped"] <= 0.02 and s["clear"] > 0.95, s
    return s


@pytest.mark.parametrize("name", CAMERA_CASES)
def test_the_checkers_primary_hits_are_held_to_the_exact_reference(name):
    c = case(name)
    o = ob.OracleScene(c.build_scene())
    o.render(1, threads=4)
    hold_primary_hits_to_the_rules(c, *o.primary_hits(), label="checker")
    o.close()
