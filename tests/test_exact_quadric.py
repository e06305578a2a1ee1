"""tests/exact_quadric.py without a GPU: (a) the numpy float32 restatements of sphere_hit and quadric_hit stay inside the margins counted from their operations,
on every input family; (b) the CPU checker -- which the device equals bit for bit -- is held to R1 - R4 and R6 (exact_disk.check_closest / check_any) on the same
families: tree walk and brute force, closest hit and occlusion, and the quadric callbacks alone.

A FAMILY is one surface configuration with its near rays (aimed at its bounds from 0.2 - 3 sizes away, at the silhouette, from inside, from on the surface, with
scaled directions, around the asymptotic cone) or its far rays; the caps are the issue's: per scene at most 1 % of the near and 2 % of the far rays undecided
for the analytic surface, per family more than 25 % clear hits and more than 10 % certain misses of it.  Origins ON a quadric have scenes of their own under each kind of transform
(`*-surface`: surface_rays and the comment above SURFACE_SCALE say how they are chosen, by geometry alone; every ray drawn is counted).  Every analytic entity e has a backdrop triangle (e + 1)
on one side and a loose triangle (e + 2) before part of the other, so that nearest-first across kinds is exercised both ways."""
import ctypes as C

import numpy as np
import pytest

import exact_disk as D
import exact_quadric as Q
import exact_rays as X
import oracle_binding as ob
from oracle_binding import f32
from pearray_amd import scene

F = np.float32
TMIN = float(F(1e-4))
ROT = np.asarray([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]])   # orthonormal in exact arithmetic (a 3-4-5 construction)
FAR_DIAGONALS = 20.0                                                            # the far family's distance: see DESIGN.md section 4 for the shares at 20 and at 50


def xform(linear, t):
    T = np.eye(4, dtype=F)
    T[:3, :3], T[:3, 3] = np.asarray(linear, dtype=F), t
    return T


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def sphere_dirs(rng, n):
    return unit(rng.normal(size=(n, 3)))


def triangles_about(centre, size):
    """The backdrop (0.8 sizes below the centre, covering +-0.7 sizes) and the loose triangle (0.7 sizes above, before part of the surface), fp32 vertices."""
    c, s = np.asarray(centre, dtype=np.float64), float(size)
    back = np.asarray([c + [-0.7 * s, -0.7 * s, -0.8 * s], c + [2.1 * s, -0.7 * s, -0.8 * s], c + [-0.7 * s, 2.1 * s, -0.8 * s]], dtype=F)
    loose = np.asarray([c + [-0.5 * s, -0.5 * s, 0.7 * s], c + [0.6 * s, -0.3 * s, 0.7 * s], c + [0.0, 0.5 * s, 0.7 * s]], dtype=F)
    return back, loose


# ---- spheres -----------------------------------------------------------------------------------------------------------------------------------
# (name, transform, LOCAL radius): unit scale near the origin; a non-uniform transform (sphere_r = the mean column norm); radius 1e-3; |c| = 80 r; two that overlap
SPHERES = [("unit", xform(np.eye(3), (0.25, -0.5, 0.75)), 1.0), ("scaled", xform(np.diag([1.5, 0.75, 1.25]), (8.0, 0.5, -0.25)), 0.8),
           ("tiny", xform(np.eye(3), (-4.0, 1.0, 0.5)), 1e-3), ("far", xform(np.eye(3), (30.5, -22.25, 12.0)), 0.5),
           ("pair-a", xform(np.eye(3), (0.0, 8.0, 0.0)), 1.0), ("pair-b", xform(np.eye(3), (0.75, 8.5, 0.25)), 0.8)]


def sphere_rays(c, r, n, rng):
    """Near rays of one sphere (c, r in float64): see the module docstring; returns org, direction (fp32)."""
    k = n // 8
    w = sphere_dirs(rng, 4 * k)
    e1 = unit(np.cross(w, np.where(np.abs(w[:, :1]) < 0.9, [[1.0, 0, 0]], [[0, 1.0, 0]])))
    e2 = np.cross(w, e1)
    ab = rng.uniform(-1.0, 1.0, (4 * k, 2))                                        # the bounding square, seen along w
    ring = unit(rng.normal(size=(k, 2))) * (1.0 + rng.uniform(-1e-3, 1e-3, (k, 1)))
    ab[3 * k:] = ring                                                               # a quarter of these: the silhouette ring r (1 +- 1e-3)
    target = c + r * (ab[:, :1] * e1 + ab[:, 1:] * e2)
    org = [target - w * (r * rng.uniform(1.2, 4.0, (4 * k, 1)))]                      # 0.2 - 3 r beyond the sphere's extent
    d = [w]
    org.append(c + r * 0.9 * sphere_dirs(rng, k) * rng.uniform(0, 1, (k, 1)) ** (1 / 3)), d.append(sphere_dirs(rng, k))            # inside
    on = (c + r * sphere_dirs(rng, 2 * k)).astype(F).astype(np.float64)               # ON the surface, as fp32 roundings of surface points: both ways
    org.append(on), d.append(sphere_dirs(rng, 2 * k))
    m = n - 7 * k
    w2 = sphere_dirs(rng, m)                                                          # head-on with the rest
    org.append(c - w2 * (r * rng.uniform(1.2, 4.0, (m, 1))) + r * rng.uniform(-1, 1, (m, 3)) * 0.7), d.append(w2)
    org, d = np.concatenate(org).astype(F), np.concatenate(d).astype(F)
    scale = rng.choice([1.0, 1.0, 0.5, 3.0], len(d)).astype(F)                        # half the directions of length 0.5 or 3
    return org, d * scale[:, None]


def sphere_scene():
    """(builder, spheres for the reference, triangles, their entity ids, their primitive ids, families [(name, org, direction)])."""
    b = scene.SceneBuilder(8, 8)
    m = b.lambert(b.spectrum_const(0.5))
    rng = np.random.default_rng(7001)
    spheres, tris, te, fam = [], [], [], []
    for name, T, r in SPHERES:
        e = b.add_sphere(m, r, transform=T)
        c, rw = D.centre32(T), Q.sphere_r32(T, r)
        spheres.append((e, c, rw))
        for p in triangles_about(c, 2.0 * float(rw)):
            te.append(b.add_mesh(p, [[0, 1, 2]], m))
            tris.append(p)
        fam.append((name,) + sphere_rays(c.astype(np.float64), float(rw), 3300, rng))
    return b, spheres, np.asarray(tris, dtype=np.float64), te, [0] * len(te), fam


# ---- quadrics ----------------------------------------------------------------------------------------------------------------------------------
# (name, ten coefficients, box min, box max): the four of tests/test_quadrics.py's QUADRIC_SCENE (the cylinder and the cone through the loader's own
# parametrisation, see quadric_table), one with all ten coefficients, and two for the linear branch
QUADRICS = [("ellipsoid", [1, 2, 4, 0, 0, 0, 0, 0, 0, -0.25], (-0.6, -0.6, -0.6), (0.6, 0.6, 0.6)),
            ("hyperboloid", [4, 4, -1, 0, 0, 0, 0, 0, 0, -0.04], (-0.4, -0.4, -0.5), (0.4, 0.4, 0.5)),
            ("cylinder", dict(kind="cylinder", radius=0.5, height=1.2), None, None),
            ("cone", dict(kind="cone", radius=0.6, height=1.5, center_on=False), None, None),
            ("general", [1, 2, 3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, -1.0], (-1, -1, -1), (1, 1, 1)),
            ("plane", [0, 0, 0, 0, 0, 0, 0, 0, 1, -2], (-1, -1, 1), (1, 1, 3)),
            ("parabolic", [1, 0, 0, 0, 0, 0, 0, -1, 0, 0], (-1, -0.5, -1), (1, 1, 1))]
PERMUTE = np.asarray([[0.0, 0, 1], [1, 0, 0], [0, 1, 0]])
# the linear part of every entity's transform, per scene: identity; exactly invertible in fp32 (a permutation of the axes times powers of two, dyadic
# translations); general (the 3-4-5 rotation times a non-uniform scale)
LINEAR = dict(identity=np.eye(3), exact=PERMUTE @ np.diag([1.0, 0.5, 0.25]), general=ROT @ np.diag([1.5, 0.7, 1.2]))


def quadric_centre(kind, k):
    """A 3 x 3 grid: dyadic where the transform is exactly invertible."""
    return (2.5 * (k % 3) - 2.5, 2.5 * (k // 3) - 2.5, 0.0) if kind != "general" else (5.3 * (k % 3) - 5.1, 4.7 * (k // 3) - 4.9, 0.37)


def local_surface_points(p, lo, hi, n, rng):
    """n points of the surface inside the box, float64: a root of Q along random chords of the box."""
    out = []
    while sum(len(x) for x in out) < n:
        a, b = rng.uniform(lo, hi, (4 * n, 3)), rng.uniform(lo, hi, (4 * n, 3))
        qa, qb, qc = Q.coefficients(p, a.T, (b - a).T)
        with np.errstate(all="ignore"):
            disc = qb * qb - 4 * qa * qc
            s = np.where(np.abs(qa) > 1e-12, (-qb - np.sqrt(disc)) / (2 * qa), -qc / qb)
        ok = np.isfinite(s) & (s > 0) & (s < 1)
        out.append((a + (b - a) * s[:, None])[ok])
    return np.concatenate(out)[:n]


def quadric_rays(H, T, name, n, rng):
    """Near and far rays of one held quadric H under the transform T: (org, direction, far mask), fp32, unit directions.  (Origins ON the surface: surface_rays.)"""
    T64 = np.asarray(T, dtype=F).astype(np.float64)
    M, t = T64[:3, :3], T64[:3, 3]
    to_world = lambda x: x @ M.T + t                                                  # noqa: E731
    lo, hi, p = H.lo.astype(np.float64), H.hi.astype(np.float64), H.p.astype(np.float64)
    diag = float(np.linalg.norm(H.whi.astype(np.float64) - H.wlo.astype(np.float64)))
    k = 2 * n // 11
    org, d = [], []
    aimed = rng.uniform(lo, hi, (4 * k, 3))                                            # at the local box, from 0.2 - 3 diagonals away; the last k, the far family: at the
    aimed[3 * k:] = 0.5 * (lo + hi) + 1.125 * (aimed[3 * k:] - 0.5 * (lo + hi))         # box grown by an eighth, from FAR_DIAGONALS x as far
    aimed = to_world(aimed)
    w = sphere_dirs(rng, 4 * k)
    dist = rng.uniform(0.2, 3.0, (4 * k, 1)) * diag
    dist[3 * k:] *= FAR_DIAGONALS
    org.append(aimed - w * dist), d.append(w)
    org.append(to_world(rng.uniform(lo, hi, (k, 3)))), d.append(sphere_dirs(rng, k))   # origins inside the box
    m = n - 5 * k
    special = None
    if name in ("hyperboloid", "cone"):                                                # around the asymptotic cone A (x^2 + y^2) + C z^2 = 0: a changes sign
        phi = np.arctan(np.sqrt(-p[2] / p[0])) + rng.uniform(-0.05, 0.05, m)
        psi = rng.uniform(0, 2 * np.pi, m)
        special = np.stack([np.sin(phi) * np.cos(psi), np.sin(phi) * np.sin(psi), np.cos(phi) * rng.choice([-1.0, 1.0], m)], 1)
    if name == "parabolic":                                                            # a = dx^2 either side of PR_EPSILON: |dx| up to 6e-4
        psi = rng.uniform(0, 2 * np.pi, m)
        special = np.stack([rng.uniform(-6e-4, 6e-4, m), np.cos(psi), np.sin(psi)], 1)
    if special is not None:
        wd = unit(special @ M.T)
        org.append(to_world(rng.uniform(lo, hi, (m, 3))) - wd * rng.uniform(0.2, 3.0, (m, 1)) * diag), d.append(wd)
    else:
        w2 = sphere_dirs(rng, m)
        org.append(to_world(rng.uniform(lo, hi, (m, 3))) - w2 * rng.uniform(0.2, 3.0, (m, 1)) * diag), d.append(w2)
    org, d = np.concatenate(org).astype(F), np.concatenate(d)
    far = np.zeros(len(org), dtype=bool)
    far[3 * k:4 * k] = True
    return org, unit(d).astype(F), far


def surface_rays(H, T, n, rng):
    """Origins ON the surface (fp32 roundings of surface points inside the box), directions both ways, chosen by geometry alone and every one counted: within 60
    degrees of the normal, and with a chord to the line's other intersection no longer than half the world box's diagonal (|b / a| for a unit direction; a far root
    much farther than that cannot lie in the box, and fp32's -b +- root over 2a is good to u |b / a|)."""
    T64 = np.asarray(T, dtype=F).astype(np.float64)
    M, t = T64[:3, :3], T64[:3, 3]
    lo, hi, p = H.lo.astype(np.float64), H.hi.astype(np.float64), H.p.astype(np.float64)
    diag = float(np.linalg.norm(H.whi.astype(np.float64) - H.wlo.astype(np.float64)))
    x = local_surface_points(p, lo, hi, 8 * n, rng)
    nrm = unit(np.stack(Q.gradient(p, x.T), 1))
    tang = unit(np.cross(nrm, sphere_dirs(rng, len(x))))
    cos = rng.uniform(0.5, 1.0, (len(x), 1)) * rng.choice([-1.0, 1.0], (len(x), 1))
    dl = cos * nrm + np.sqrt(1 - cos * cos) * tang
    dl = dl / np.linalg.norm(dl @ M.T, axis=1, keepdims=True)                          # the local direction of a unit world direction
    qa, qb, _ = Q.coefficients(p, x.T, dl.T)
    with np.errstate(all="ignore"):
        keep = np.abs(qb / qa) <= 0.5 * diag
    assert keep.sum() >= n
    x, dl = x[keep][:n], dl[keep][:n]
    # every third origin stands 5e-7 BEFORE the surface along its ray, as a secondary ray's does whose origin carries an error: the near root, half of INT_EPS
    # ahead, is still "behind" and the far root is due -- which only the threshold INT_EPS itself (not 0, not PR_EPSILON) tells
    dw = unit(dl @ M.T)
    back = np.where(np.arange(n) % 3 == 0, 5e-7, 0.0)[:, None]
    return (x @ M.T + t - back * dw).astype(F), dw.astype(F), np.zeros(n, dtype=bool)


def quadric_table(b, e):
    off = b.entities[e].params
    v = [F(x) for x in b.tables[off:off + 16]]
    return v[:10], v[10:13], v[13:16]


# The scenes of the on-surface origins: every quadric AT the origin (they overlap: the nearest of several surfaces is what a traversal reports anyway), the general
# transform an eighth of its size, so that world coordinates stay below 1 / 4.  There the roundings of the local origin (4 u of coordinates < 0.25) and of c stay a
# tenth of INT_EPS = 1e-6 and the rule "the far root when the near one is <= INT_EPS" is decided; at coordinates of 2.5 or 5 the origin's own grid is not finer than
# INT_EPS and nothing is pinned.
# Two surfaces change there, for reasons of geometry: the plane is left out (from a point on a plane the line meets it nowhere else: no family with hits), and the
# quadric with all ten coefficients is a quarter of its size (x -> 4 x: the same surface, box +-0.25) -- at full size its c is a sum of ten terms of size 1 to 3 whose
# roundings, over |b| ~ 2, come to half of INT_EPS before doubling; a quarter the size, b is four times as large.
SURFACE_SCALE = dict(identity=1.0, exact=1.0, general=0.125)
SURFACE_SHRINK = 4.0


def surface_quadrics():
    out = []
    for name, p, lo, hi in QUADRICS:
        if name == "general":
            k = SURFACE_SHRINK
            p, lo, hi = [v * k * k for v in p[:6]] + [v * k for v in p[6:9]] + p[9:], tuple(v / k for v in lo), tuple(v / k for v in hi)
        if name != "plane":
            out.append((name, p, lo, hi))
    return out


def quadric_scene(kind):
    """(builder, quadrics for the reference, triangles, entity ids, primitive ids, families [(name, org, direction, far mask)])."""
    b = scene.SceneBuilder(8, 8)
    m = b.lambert(b.spectrum_const(0.5))
    base, on_surface = kind.split("-")[0], kind.endswith("-surface")
    rng = np.random.default_rng(dict(identity=7101, exact=7102, general=7103)[base] + (10 if on_surface else 0))
    quadrics, tris, te, fam = [], [], [], []
    for k, (name, p, lo, hi) in enumerate(surface_quadrics() if on_surface else QUADRICS):
        T = xform(LINEAR[base] * SURFACE_SCALE[base], (0.0, 0.0, 0.0)) if on_surface else xform(LINEAR[base], quadric_centre(base, k))
        if isinstance(p, dict):
            args = dict(p)
            e = (b.add_cylinder if args.pop("kind") == "cylinder" else b.add_cone)(m, transform=T, **args)
        else:
            e = b.add_quadric(m, p, lo, hi, transform=T)
        H = Q.HeldQuadric(T, *quadric_table(b, e))
        quadrics.append((e, H))
        wc, size = 0.5 * (H.wlo.astype(np.float64) + H.whi.astype(np.float64)), float(np.linalg.norm(H.whi.astype(np.float64) - H.wlo.astype(np.float64)))
        if not on_surface:
            for tri in triangles_about(wc, size):
                te.append(b.add_mesh(tri, [[0, 1, 2]], m))
                tris.append(tri)
        fam.append((name,) + (surface_rays(H, T, 1400, rng) if on_surface else quadric_rays(H, T, name, 2850, rng)))
    if on_surface:                                                                     # one backdrop and one loose triangle about the cluster
        wlo, whi = np.min([q[1].wlo for q in quadrics], 0).astype(np.float64), np.max([q[1].whi for q in quadrics], 0).astype(np.float64)
        for tri in triangles_about(0.5 * (wlo + whi), float(np.linalg.norm(whi - wlo))):
            te.append(b.add_mesh(tri, [[0, 1, 2]], m))
            tris.append(tri)
    return b, quadrics, np.asarray(tris, dtype=np.float64), te, [0] * len(te), fam


# ---- the cases, built once -----------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name):
        self.name = name
        if name == "spheres":
            self.builder, self.spheres, self.tris, self.te, self.tp, fam = sphere_scene()
            self.quadrics = []
            fam = [f + (np.zeros(len(f[1]), dtype=bool),) for f in fam]
        else:
            self.builder, self.quadrics, self.tris, self.te, self.tp, fam = quadric_scene(name)
            self.spheres = []
        self.org, self.direction = np.concatenate([f[1] for f in fam]), np.concatenate([f[2] for f in fam])
        self.far = np.concatenate([f[3] for f in fam])
        self.family = np.concatenate([np.full(len(f[1]), k) for k, f in enumerate(fam)])
        self.names = [f[0] for f in fam]
        self.analytic = [s[0] for s in self.spheres] + [q[0] for q in self.quadrics]
        self.n = len(self.org)
        assert self.n <= 20000
        self.min_hits = (50, -1) if name.endswith("-surface") else (200, 50)       # reported hits asked of every analytic entity / triangle (few on-surface rays leave the cluster upwards)
        self._tri = D.candidates(self.org, self.direction, [], self.tris, self.te, self.tp)
        self._closest, self._tables = {}, {}

    def candidates(self, tmin=TMIN, tmax=np.inf, any_hit=False, surfaces_only=False):
        tri = [self._tri.ray, self._tri.entity, self._tri.prim, self._tri.t, self._tri.tol, self._tri.clear]
        parts = [Q._sphere_rows(self.org.astype(np.float64), self.direction.astype(np.float64), self.spheres, np.broadcast_to(np.asarray(tmin, dtype=np.float64), (self.n,)), 0.0),
                 Q._quadric_rows(self.org.astype(np.float64), self.direction.astype(np.float64), self.quadrics, np.broadcast_to(np.asarray(tmin, dtype=np.float64), (self.n,)),
                                 np.broadcast_to(np.asarray(tmax, dtype=np.float64), (self.n,)), any_hit, tables=self._tables)]
        rows = [p[0] for p in parts] + ([] if surfaces_only else [tri])
        return D.Candidates(self.n, *(np.concatenate([r[k] for r in rows]) for k in range(6)), parts[0][1] | parts[1][1])

    def subset(self, pick):
        """The same scene with the rays `pick` only."""
        sub = Case.__new__(Case)
        sub.__dict__.update(self.__dict__)
        sub.org, sub.direction, sub.far, sub.family, sub.n = self.org[pick], self.direction[pick], self.far[pick], self.family[pick], len(pick)
        sub._tri = D.candidates(sub.org, sub.direction, [], self.tris, self.te, self.tp)
        sub._closest, sub._tables = {}, {}
        return sub

    def closest(self):
        """The candidates of the default window, cached: spheres with tmin = TMIN."""
        if "c" not in self._closest:
            self._closest["c"] = self.candidates()
        return self._closest["c"]

    def shares(self, cand, tmin=TMIN, tmax=np.inf):
        """Per family and near / far: the analytic surface's clear hits, certain misses and undecided rays; asserts the caps, returns the printed line."""
        sure, possible = D._window(cand, np.full(self.n, tmin), np.broadcast_to(np.asarray(tmax, dtype=np.float64), (self.n,)))
        mine = cand.entity == np.asarray(self.analytic)[self.family[cand.ray]]           # the family's OWN surface
        hit, near = np.zeros(self.n, dtype=bool), np.zeros(self.n, dtype=bool)
        hit[cand.ray[mine & cand.clear & sure]] = True
        near[cand.ray[mine & possible]] = True
        und = near & ~hit
        out, bad = [], []
        for far, cap in ((False, 0.01), (True, 0.02)):
            sel = self.far == far
            if not sel.any():
                continue
            out.append("%s %s: undecided %.4f" % (self.name, "far" if far else "near", und[sel].mean()))
            bad += [out[-1]] if und[sel].mean() > cap else []
            for k, nm in enumerate(self.names):
                s = sel & (self.family == k)
                out.append("  %-12s clear hits %.3f certain misses %.3f undecided %.4f" % (nm, hit[s].mean(), (~near)[s].mean(), und[s].mean()))
                bad += [out[-1]] if not (hit[s].mean() > 0.25 and (~near)[s].mean() > 0.10) else []
        print("\n".join(out))
        assert not bad, bad
        return "%s: caps hold" % self.name


CASES = ["spheres", "identity", "exact", "general", "identity-surface", "exact-surface", "general-surface"]
_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]


def nearest_clear(cand, n):
    """Per ray the t of the nearest clear candidate (inf: none) -- the `exact t` the tmax windows stand 1 % either side of."""
    return X._segment_min(np.where(cand.clear & (cand.t > TMIN), cand.t, np.inf), cand.ray, n)


def occlusion_windows(near, tmin):
    """test_gpu_disk.py's: (tmin, distance) pairs a margin either side of the reported distance, fp32."""
    far, lo = np.full(len(near), np.inf), np.full(len(near), tmin)
    return [(a.astype(F), b.astype(F)) for a, b in ((lo, near * 1.01 + 0.001), (lo, near * 0.99 + 0.001), (near * 0.99, far), (near * 1.01, far))]


def hold_any(c, trace_any, tmin32, dist32, label):
    cand = c.candidates(tmin=tmin32.astype(np.float64), tmax=dist32.astype(np.float64) - 0.001, any_hit=True)
    sa = D.check_any(cand, tmin32.astype(np.float64), dist32.astype(np.float64), trace_any(c.org, c.direction, tmin32, dist32), label=label)
    # not vacuous: the share left to neither clause is 3.0 % at most, in the sphere scene -- the rays about the sphere of radius 1e-3, where a window 1 % of 2e-3
    # beside the reported distance is as narrow as the slide exact_rays allows the neighbouring triangles at coordinates of 4; 0.2 % in the quadric scenes
    assert sa["undecided"] <= 0.035, (label, sa)
    return sa


# ---- the reference against itself ------------------------------------------------------------------------------------------------------------------
def test_exact_decisions_on_hand_made_rays():
    from fractions import Fraction as Fr
    c, r = F([0, 0, 5]), F(1)
    assert Q.exact_ray_sphere(F([0, 0, 0]), F([0, 0, 1]), c, r) == (1, Fr(4), Fr(6))
    assert Q.exact_ray_sphere(F([0, 0, 0]), F([0, 0, 2]), c, r) == (1, Fr(2), Fr(3))                       # a direction of length 2 halves t
    assert Q.exact_ray_sphere(F([1, 0, 0]), F([0, 0, 1]), c, r) == (0, Fr(5), Fr(5))                       # exactly grazing
    assert Q.exact_ray_sphere(np.nextafter(F(1), F(2)) * F([1, 0, 0]), F([0, 0, 1]), c, r)[0] == -1        # one ulp outside
    assert Q.exact_ray_sphere(np.nextafter(F(1), F(0)) * F([1, 0, 0]), F([0, 0, 1]), c, r)[0] == 1
    sg, tf, tb = Q.exact_ray_sphere(F([0, 0, 5]), F([0.6, 0, 0.8]), c, r)                                  # from the centre: -+ r / |d|
    assert sg == 1 and abs(float(tb) - 1.0) < 1e-7 and tf == -tb
    assert abs(Q._sqrt_fraction(Fr(2)) ** 2 - 2) < Fr(1, 1 << 90)
    # the unit sphere as a quadric, identity: the local parameter is the world's
    H = Q.HeldQuadric(np.eye(4), [1, 1, 1, 0, 0, 0, 0, 0, 0, -1], (-1, -1, -1), (1, 1, 1))
    entry, ext, a, b, cc, disc = Q._exact_quadric(F([0.25, 0, -3]), F([0.0625, 0.125, 1]), H)
    assert a == Fr(261, 256) and disc > 0 and entry > 2 - Fr(1, 1000) and entry < 2
    assert np.array_equal(H.wlo, H.lo) and np.array_equal(H.inv.reshape(3, 4)[:, :3], np.eye(3, dtype=F))
    assert Q.sphere_r32(np.diag([2.0, 2.0, 2.0, 1.0]), 0.5) == F(1) and abs(float(Q.sphere_r32(xform(np.diag([1.5, 0.75, 1.25]), (0, 0, 0)), 0.8)) - 0.8 * 3.5 / 3) < 1e-7


def test_the_float64_pass_agrees_with_the_exact_stage():
    rng = np.random.default_rng(5)
    c = case("general")
    pick = rng.choice(c.n, 300, replace=False)
    o, d = c.org[pick], c.direction[pick]
    for ent, H in c.quadrics[:5]:
        fast, exact = Q.classify_quadric(o, d, H), Q.classify_quadric(o, d, H, force_exact=True)
        assert exact.n_exact == 300 and fast.n_exact < 30
        ok = fast.ok & exact.ok
        for f in ("entry", "exit", "a", "b", "c"):
            x, y = getattr(fast, f)[ok], getattr(exact, f)[ok]
            fin = np.isfinite(x) & np.isfinite(y)
            assert np.abs(x[fin] - y[fin]).max() <= 2.0 ** -40 * max(1.0, np.abs(y[fin]).max()), f
        assert np.array_equal(np.sign(fast.disc[ok]), np.sign(exact.disc[ok]))
    s = case("spheres")
    o, d = s.org[::40], s.direction[::40]
    cs, rs = [x[1] for x in s.spheres], [x[2] for x in s.spheres]
    fast, exact = Q.classify_spheres(o, d, cs, rs), Q.classify_spheres(o, d, cs, rs, force_exact=True)
    assert np.array_equal(fast.s2 > 0, exact.s2 > 0)
    hit = exact.s2 > 0
    assert np.allclose(fast.proj[hit], exact.proj[hit], rtol=2.0 ** -40, atol=2.0 ** -45) and np.allclose(fast.td[hit], exact.td[hit], rtol=2.0 ** -30, atol=2.0 ** -45)


# ---- (a) the fp32 statement sequences inside their margins -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_the_fp32_statement_sequences_stay_inside_their_margins(name):
    """sphere32 / quadric32 (numpy float32 restatements of device/pr_device.h -- a check of the margins, not a reference) against each surface's own rows: where
    the surface is clear inside the window the restatement reports it, within tol; where it has no row the restatement reports nothing; the worst |t32 - t| / tol."""
    c = case(name)
    cand = c.candidates(surfaces_only=True)
    o, d = c.org, c.direction
    worst = {}
    for ent, kind, what in [(s[0], "s", s) for s in c.spheres] + [(q[0], "q", q) for q in c.quadrics]:
        for tmax in (np.inf, None):
            limit = np.full(c.n, np.inf)
            mine = cand.entity == ent
            if tmax is None:                                                           # a window that ends 1 % before or after the exact t
                t_ref = np.full(c.n, np.inf)
                t_ref[cand.ray[mine & cand.clear]] = cand.t[mine & cand.clear]
                limit = np.where(np.isfinite(t_ref), t_ref * np.where(np.arange(c.n) % 2 == 0, 0.99, 1.01), np.inf).astype(F).astype(np.float64)
            if kind == "s":
                ok, t32 = Q.sphere32(o, d, what[1], what[2], TMIN, limit)
            else:
                ok, t32, _, _ = Q.quadric32(o, d, what[1], TMIN, limit)
            sub = D.Candidates(c.n, cand.ray[mine], cand.entity[mine], cand.prim[mine], cand.t[mine], cand.tol[mine], cand.clear[mine], cand.undecided_disk)
            hit = (np.where(ok, ent, D.INVALID).astype(np.uint32), np.where(ok, 0, D.INVALID).astype(np.uint32), None, None, np.where(ok, t32, np.inf))
            D.check_closest(sub, TMIN, limit, hit, label="%s entity %d restated" % (name, ent))
            row = D.lookup(sub, np.nonzero(ok)[0], np.full(ok.sum(), ent), np.zeros(ok.sum(), dtype=np.int64))
            fin = (row >= 0) & sub.clear[np.maximum(row, 0)]
            ratio = np.abs(t32[ok][fin].astype(np.float64) - sub.t[row[fin]]) / sub.tol[row[fin]]
            worst[ent] = max(worst.get(ent, 0.0), float(ratio.max()) if len(ratio) else 0.0)
    print("%s: worst |t32 - t| / tol per entity %s" % (name, {k: round(v, 3) for k, v in worst.items()}))
    assert max(worst.values()) < 1.0
    print(c.shares(c.closest()))


# ---- (b) the checker held to the rules --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracles():
    made = {}

    def get(name):
        if name not in made:
            made[name] = ob.OracleScene(case(name).builder.build())
        return made[name]
    return get


@pytest.mark.parametrize("brute", [False, True])
@pytest.mark.parametrize("name", CASES)
def test_the_checker_is_held_to_the_rules(oracles, name, brute):
    c, o = case(name), oracles(name)
    cand = c.closest()
    hit = o.trace_closest(c.org, c.direction, TMIN, np.inf, brute=brute)
    s = D.check_closest(cand, TMIN, np.inf, hit, label="%s closest" % name)
    ent, prim, u, v, t = hit
    on = np.isin(ent, c.analytic)
    assert not u[on].any() and not v[on].any() and not prim[on].any()
    assert all((ent == e).sum() > c.min_hits[0] for e in c.analytic) and all((ent == e).sum() > c.min_hits[1] for e in c.te), np.bincount(ent[ent != D.INVALID])
    print("%s closest %s" % (name, s))
    # the window's end 1 % before and after the exact t
    t_ref = nearest_clear(cand, c.n)
    for scale in (0.99, 1.01):
        limit = np.where(np.isfinite(t_ref), t_ref * scale, np.inf).astype(F)
        D.check_closest(cand, TMIN, limit.astype(np.float64), o.trace_closest(c.org, c.direction, TMIN, limit, brute=brute), label="%s closest, tmax x %.2f" % (name, scale))
    near = np.where(ent != D.INVALID, t.astype(np.float64), 1.0)
    for lo32, hi32 in occlusion_windows(near, TMIN):
        sa = hold_any(c, lambda *a: o.trace_any(*a, brute=brute), lo32, hi32, "%s any" % name)
        print("%s any %s" % (name, sa))


@pytest.mark.parametrize("name", CASES[1:])
def test_the_quadric_callbacks_alone_are_held_to_the_rules(oracles, name):
    """orc_quadric_closest / orc_quadric_occluded: the callbacks without the tree and without triangles, on every eighth ray."""
    c, o = case(name), oracles(name)
    lib = ob.load()
    pick = np.arange(0, c.n, 8)
    ent, t, occ = np.empty(len(pick), dtype=np.uint32), np.empty(len(pick), dtype=F), np.empty(len(pick), dtype=bool)
    tt = C.c_float()
    for k, i in enumerate(pick):
        ent[k] = lib.orc_quadric_closest(o.h, f32(*c.org[i]), f32(*c.direction[i]), F(TMIN), np.inf, C.byref(tt))
        t[k] = tt.value
        occ[k] = lib.orc_quadric_occluded(o.h, f32(*c.org[i]), f32(*c.direction[i]), F(TMIN), 1e30) != 0
    sub = c.subset(pick)
    cand = sub.candidates(surfaces_only=True)
    prim = np.where(ent != D.INVALID, 0, D.INVALID).astype(np.uint32)
    print(name, D.check_closest(cand, TMIN, np.inf, (ent, prim, None, None, np.where(ent != D.INVALID, t, np.inf)), label="%s callback" % name))
    any_c = sub.candidates(tmin=TMIN, tmax=1e30, any_hit=True, surfaces_only=True)
    print(name, D.check_any(any_c, TMIN, 1e30 + 0.001, occ, label="%s occlusion callback" % name))
    assert 0.2 < occ.mean() < 0.95 and (occ & (ent == D.INVALID)).sum() > 20                  # the unbounded surface behind the box occludes


def test_the_rules_catch_wrong_answers():
    """The rules fail on answers that break them, one ray at a time: a clear hit dropped, a distance 1e-4 off, a hit where the ray comes near nothing
    (profiles/exact_quadric_mutations.log has the mutants of the code itself)."""
    c = case("identity")
    cand = c.closest()
    n = c.n
    first = np.full(n, -1, dtype=np.int64)
    rows = np.nonzero(cand.clear & (cand.t > TMIN + cand.tol))[0]
    first[cand.ray[rows][::-1]] = rows[::-1]
    has = first >= 0
    ent = np.where(has, cand.entity[np.maximum(first, 0)], D.INVALID).astype(np.uint32)
    prim = np.where(has, cand.prim[np.maximum(first, 0)], D.INVALID).astype(np.uint32)
    t = np.where(has, cand.t[np.maximum(first, 0)], np.inf)
    und = np.zeros(n, dtype=bool)
    und[cand.ray[~cand.clear]] = True
    keep = ~und                                                                            # (the reference's own answer is only known where nothing is undecided)
    ok_hit = (np.where(keep, ent, D.INVALID).astype(np.uint32), np.where(keep, prim, D.INVALID).astype(np.uint32), None, None, np.where(keep, t, np.inf))
    good = [k for k in np.nonzero(keep & has & np.isin(ent, c.analytic))[0][:50]]
    assert len(good) == 50
    for wrong in ("missed", "t", "phantom"):
        e2, p2, t2 = ok_hit[0].copy(), ok_hit[1].copy(), ok_hit[4].copy()
        k = good[7]
        if wrong == "missed":
            e2[k] = p2[k] = D.INVALID
        elif wrong == "t":
            t2[k] = t[k] * (1 + 1e-4)
        else:
            k = np.nonzero(keep & ~has)[0][0]
            e2[k], p2[k], t2[k] = c.analytic[0], 0, 1.0
        only = np.zeros(n, dtype=bool)
        only[k] = True
        rows = only[cand.ray]
        one = D.Candidates(n, cand.ray[rows], cand.entity[rows], cand.prim[rows], cand.t[rows], cand.tol[rows], cand.clear[rows], only)
        h = tuple(None if x is None else np.where(only, x, np.asarray(D.INVALID if x.dtype == np.uint32 else np.inf).astype(x.dtype)) for x in (e2, p2, None, None, t2))
        with pytest.raises(AssertionError):
            D.check_closest(one, TMIN, np.inf, h)
