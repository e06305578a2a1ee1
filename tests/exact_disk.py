"""Exact-arithmetic reference for ray / disk queries, the rules a traversal has to satisfy against it, and float64 quadratures for the radiometry of a
disk light (TEST INFRASTRUCTURE ONLY, beside tests/exact_rays.py, which is imported and not changed: plain numpy and Python integers, no product import).

A disk is (c, n, r): the points x of the plane n . (x - c) = 0 with |x - c| < r; n need not be a unit vector.  For fp32 (or float64) inputs

    den = d . n        num = (c - o) . n        t = num / den                 (den == 0: the ray lies in or beside the plane, never a hit)
    q   = o + t d - c  = (num d - den (c - o)) / den
    inside  <=>  |q|^2 < r^2  <=>  |num d - den (c - o)|^2 - r^2 den^2 < 0

are all rationals: exact_ray_disk() evaluates them with Python integers (a float is an integer x 2^-1074) and returns t as a Fraction and the SIGN of
|q|^2 - r^2.  classify() evaluates the same expressions in float64 for many rays -- a rounding of 2^-53 where the rules below work with margins of
2^-24 -- and sends every pair whose float64 value is within 2^-30 (relative) of a decision to the exact stage.

The margins come from the operation count of the fp32 statement sequence under test (device/pr_device.h, disk_hit), u = 2^-24, first order, doubled:

    den = (dx nx + dy ny) + dz nz        each term passes 3 roundings: |err| <= 3 u sum |d_i n_i| <= 3 u |d| |n| = 3 u |den| / cos(phi)
    c0  = c - o                          1 rounding per component
    num = (c0x nx + c0y ny) + c0z nz     3 more: |err| <= 4 u |c0| |n|, and |num| = h |n| with h the origin's distance from the plane
    t   = num / den                      1 more
    => |dt| <= u (3 t / cos(phi) + 4 D / cos(phi) + t) <= 8 u max(t, D) / cos(phi),      D = |c - o|, cos(phi) = |d . n| / (|d| |n|), |d| = 1

    TAU(t, D, phi) = T_ULPS u max(t, D) / cos(phi),  T_ULPS = 16 (twice the count)

    q   = d t - c0                       per component 1 rounding of d_i t, the rounding c0_i carries, 1 of the difference: <= u (t + D + rho), rho = |q|,
                                         on top of |d| dt from t
    q . q < r r                          3 roundings of the sum (1.5 u rho as a distance), 1 of r r (0.5 u r)
    => the fp32 decision can differ from the exact one only when |rho - r| <= TAU + u (t + D + 2.5 rho + 0.5 r) <= TAU + 5 u max(t, D, r) near the rim

    RIM(t, D, phi, r) = TAU + RIM_ULPS u max(t, D, r),  RIM_ULPS = 10 (twice the count)

A ray whose exact pierce point is farther than RIM inside the rim and whose exact t is TAU inside the window MUST be reported; one farther than RIM outside
the rim, or TAU outside the window, MUST NOT; between them the ray is UNDECIDED (ties on the rim and at the window's ends are not pinned, DESIGN.md
section 4)."""
from fractions import Fraction

import numpy as np

import exact_rays as X

EPS32 = X.EPS32
T_ULPS = 16.0
RIM_ULPS = 10.0
INVALID = X.INVALID
F = np.float32


# ---- the fp32 inputs as the library derives them from an entity's transform -------------------------------------------------------------------
def normal32(T):
    """normalMatrix * (0, 0, 1) in float32 as host/setup.cpp computes it from the 4x4 transform: column 2 of cofactor / det, the operations in its order."""
    m = np.asarray(T, dtype=F).reshape(4, 4)
    a, b, c, dd, ee, f, g, h, i = (m[0, 0], m[0, 1], m[0, 2], m[1, 0], m[1, 1], m[1, 2], m[2, 0], m[2, 1], m[2, 2])
    cof0, cof1, cof2 = ee * i - f * h, f * g - dd * i, dd * h - ee * g
    cof5, cof8 = b * g - a * h, a * ee - b * dd
    det = (a * cof0 + b * cof1) + c * cof2
    out = np.asarray([cof2 / det, cof5 / det, cof8 / det])
    assert out.dtype == F
    return out


def centre32(T):
    return np.asarray(T, dtype=F).reshape(4, 4)[:3, 3].copy()


# ---- exact --------------------------------------------------------------------------------------------------------------------------------
def exact_ray_disk(o, d, c, n, r):
    """(t, sign): t = the exact plane distance as a Fraction (None when d . n == 0), sign = -1 / 0 / +1 of |o + t d - c|^2 - r^2 (inside / on / outside)."""
    o, d, c, n = ([X._int(v) for v in x] for x in (o, d, c, n))
    r = X._int(r)
    c0 = [c[k] - o[k] for k in range(3)]
    den = sum(d[k] * n[k] for k in range(3))
    if den == 0:
        return None, 1
    num = sum(c0[k] * n[k] for k in range(3))
    # q den = num d - den c0 (inputs on the common scale S = 2^1074, both products on S^3): |q|^2 - r^2 has the sign of |q den|^2 - r^2 den^2 (S^6)
    qd = [num * d[k] - den * c0[k] for k in range(3)]
    s = sum(v * v for v in qd) - r * r * den * den
    return Fraction(num, den), (s > 0) - (s < 0)


class DiskTable:
    """Per (ray, disk): t (float64, the exact value rounded once where the exact stage ran), rho = |o + t d - c|, sign of rho - r, cos(phi), D; nan / +1
    where d . n == 0.  Arrays of shape [n_rays, n_disks]."""

    def __init__(self, t, rho, sign, cos_phi, D, n_exact):
        self.t, self.rho, self.sign, self.cos_phi, self.D, self.n_exact = t, rho, sign, cos_phi, D, n_exact


def classify(org, direction, centres, normals, radii, force_exact=False):
    o, d = X._as64(org, (-1, 3)), X._as64(direction, (-1, 3))
    C, N, R = X._as64(centres, (-1, 3)), X._as64(normals, (-1, 3)), X._as64(radii, (-1,))
    c0 = C[None] - o[:, None]                                   # [rays, disks, 3]
    den = (d[:, None] * N[None]).sum(-1)
    num = (c0 * N[None]).sum(-1)
    with np.errstate(all="ignore"):
        t = num / den
        q = d[:, None] * t[..., None] - c0
        rho = np.sqrt((q * q).sum(-1))
        cos_phi = np.abs(den) / (np.linalg.norm(d, axis=1)[:, None] * np.linalg.norm(N, axis=1)[None])
    D = np.linalg.norm(c0, axis=-1)
    sign = np.where(rho < R[None], -1, 1)
    # float64 cannot be trusted where the decision is closer than 2^-30 relative, or den is within its own rounding of zero
    todo = ~np.isfinite(t) | (np.abs(rho - R[None]) <= 2.0 ** -30 * np.maximum(R[None], rho)) | (cos_phi <= 2.0 ** -30) | force_exact
    idx = np.argwhere(todo)
    for i, k in idx:
        te, se = exact_ray_disk(o[i], d[i], C[k], N[k], R[k])
        sign[i, k] = se
        t[i, k] = np.nan if te is None else float(te)
    return DiskTable(t, rho, sign, cos_phi, D, len(idx))


def tau(t, D, cos_phi):
    with np.errstate(all="ignore"):
        return T_ULPS * EPS32 * np.maximum(np.abs(t), D) / cos_phi


def rim(t, D, cos_phi, r):
    return tau(t, D, cos_phi) + RIM_ULPS * EPS32 * np.maximum(np.maximum(np.abs(t), D), r)


def disk32(o, d, c, n, r, tmin, limit):
    """disk_hit of device/pr_device.h restated in numpy float32, row-wise (for checking the margins on the CPU, not a reference): accepted, t."""
    o, d, c, n = (np.asarray(x, dtype=F) for x in (o, d, c, n))
    r, tmin, limit = F(r), F(tmin), F(limit)
    with np.errstate(all="ignore"):
        den = (d[:, 0] * n[0] + d[:, 1] * n[1]) + d[:, 2] * n[2]
        c0 = c[None] - o
        t = ((c0[:, 0] * n[0] + c0[:, 1] * n[1]) + c0[:, 2] * n[2]) / den
        q = d * t[:, None] - c0
        ok = (den != 0) & (t > tmin) & (t <= limit) & (((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) < r * r)
    return ok, t


# ---- candidates: what a ray may or must report, disks and triangles alike -----------------------------------------------------------------------
class Candidates:
    """Rows (ray, entity, prim, t, tol, clear): a surface the ray meets or may meet.  clear: the reference decides that it is hit (a disk farther than RIM
    inside its rim; a triangle that qualifies under R1 of tests/exact_rays.py, window not yet applied); tol: how far the reported t may be from t."""

    def __init__(self, n_rays, ray, entity, prim, t, tol, clear, undecided_disk):
        order = np.lexsort((t, ray))
        self.n_rays = n_rays
        self.ray, self.entity, self.prim, self.t, self.tol, self.clear = (np.asarray(a)[order] for a in (ray, entity, prim, t, tol, clear))
        self.undecided_disk = undecided_disk                     # per ray: some disk's rim band holds the pierce point


def candidates(org, direction, disks, tris=None, tri_entity=None, tri_prim=None, extra_ulps=0.0):
    """disks: list of (entity id, centre, normal, radius) as the device holds them (fp32 values); tris: world-space triangles of untransformed meshes.
    extra_ulps: as X.Geometry's (rays the caller knows only up to a rounding, the camera's): widens the triangles' DELTA, and for the disks TAU and RIM by
    extra_ulps u max(t, D) / cos(phi) -- a direction off by e moves the pierce point by e t along the plane and t by e t tan(phi) <= e t / cos(phi)."""
    o = X._as64(org, (-1, 3))
    n = len(o)
    tab = classify(org, direction, [k[1] for k in disks], [k[2] for k in disks], [k[3] for k in disks])
    R = np.asarray([float(k[3]) for k in disks])[None]
    with np.errstate(all="ignore"):
        extra = extra_ulps * EPS32 * np.maximum(np.abs(tab.t), tab.D) / tab.cos_phi
        rm, tl = rim(tab.t, tab.D, tab.cos_phi, R) + extra, tau(tab.t, tab.D, tab.cos_phi) + extra
        met = np.isfinite(tab.t) & np.isfinite(rm) & (tab.rho <= R + rm)
        clear = met & (tab.rho < R - rm) & (tab.sign < 0)
    ri, di = np.nonzero(met)
    ray, ent, prim = [ri], [np.asarray([disks[k][0] for k in di], dtype=np.int64)], [np.zeros(len(ri), dtype=np.int64)]
    t, tol, clr = [tab.t[ri, di]], [tl[ri, di]], [clear[ri, di]]
    undecided = (met & ~clear).any(1) | (~np.isfinite(rm) & np.isfinite(tab.t)).any(1)
    if tris is not None and len(tris):
        geo = X.Geometry(tris, tri_entity, tri_prim, extra_ulps=extra_ulps)
        cls = X.classify(org, direction, geo.tris, margin=geo.delta(o))
        M = X.ray_extent(o, geo.extent)[cls.ray]
        tol_t = X._tau(cls.t, M) + geo.slide(M, cls.sin_phi)
        q = (cls.kind == 2) & (cls.edge_dist >= geo.delta_ulps * EPS32 * M * (1 + 2.0 ** -30)) & np.isfinite(tol_t)
        ray.append(cls.ray), ent.append(geo.entity[cls.tri]), prim.append(geo.prim[cls.tri]), t.append(cls.t), tol.append(tol_t), clr.append(q)
    return Candidates(n, *(np.concatenate(a) for a in (ray, ent, prim, t, tol, clr)), undecided)


def lookup(cand, rays, entity, prim):
    """Row of the candidate (ray, entity, prim) for each triple, -1 where the ray has no such candidate."""
    key = lambda r, e, p: (np.asarray(r, dtype=np.int64) << 40) | (np.asarray(e, dtype=np.int64) << 20) | np.asarray(p, dtype=np.int64)   # noqa: E731
    ck = key(cand.ray, cand.entity, cand.prim)
    order = np.argsort(ck, kind="stable")
    hk = key(rays, entity, prim)
    if not len(ck):
        return np.full(len(hk), -1, dtype=np.int64)
    pos = np.minimum(np.searchsorted(ck[order], hk), len(ck) - 1)
    return np.where(ck[order][pos] == hk, order[pos], -1)


def _window(cand, tmin, tmax):
    """(surely inside, possibly inside) the window, per row.  A row without a finite t or tolerance is possible and never sure."""
    with np.errstate(invalid="ignore"):
        sure = (cand.t >= tmin[cand.ray] + cand.tol) & (cand.t <= tmax[cand.ray] - cand.tol)
        possible = ~((cand.t < tmin[cand.ray] - cand.tol) | (cand.t > tmax[cand.ray] + cand.tol))
    return sure, possible


def check_closest(cand, tmin, tmax, hit, label=""):
    """The rules of tests/exact_rays.py on the candidate table, for a closest-hit answer (entity, prim, u, v, t); u, v may be None (ids and t only), t too.
    R1 no clear hit missed, R3 nearest first, R2 no phantom (the reported surface is a candidate, its t within tol of the reported one and in the window;
    u = v = 0 on disks is the caller's), R4 a clear ray reports the clear surface.  Returns the shares."""
    n = cand.n_rays
    tmin = np.broadcast_to(np.asarray(tmin, dtype=np.float64), (n,))
    tmax = np.broadcast_to(np.asarray(tmax, dtype=np.float64), (n,))
    ent, prim, _, _, ht = hit
    ent, prim = np.asarray(ent).reshape(-1), np.asarray(prim).reshape(-1)
    is_hit = ent != INVALID
    sure, possible = _window(cand, tmin, tmax)
    must = cand.clear & sure
    bound = X._segment_min(np.where(must, cand.t + cand.tol, np.inf), cand.ray, n)
    has = np.isfinite(bound)
    bad = has & ~is_hit
    assert not bad.any(), "%s R1: ray %d has a clear hit but reports none" % (label, np.nonzero(bad)[0][0])
    if ht is not None:
        ht = np.asarray(ht, dtype=np.float64).reshape(-1)
        bad = has & is_hit & ~(ht <= bound)
        assert not bad.any(), "%s R1/R3: ray %d reports t = %r beyond a clear hit's bound %r" % (label, np.nonzero(bad)[0][0], ht[bad][0], bound[bad][0])
    # R2: the reported surface among the ray's candidates
    h = np.nonzero(is_hit)[0]
    row = lookup(cand, h, ent[h], prim[h])
    found = row >= 0
    assert found.all(), "%s R2: ray %d reports (%d, %d), which it does not come near" % (label, h[~found][0], ent[h][~found][0], prim[h][~found][0])
    assert possible[row].all(), "%s R2: ray %d reports a surface outside its window" % (label, h[~possible[row]][0])
    if ht is not None:
        with np.errstate(invalid="ignore"):
            bad = np.isfinite(cand.tol[row]) & np.isfinite(cand.t[row]) & ~(np.abs(ht[h] - cand.t[row]) <= cand.tol[row])
        assert not bad.any(), "%s R2: ray %d reports t = %r, exact %r, allowed %r" % (label, h[bad][0], ht[h][bad][0], cand.t[row][bad][0], cand.tol[row][bad][0])
    # R4: identity on clear rays -- the nearest clear candidate, when every other possible one lies beyond its bound
    first = np.full(n, -1, dtype=np.int64)
    rows = np.nonzero(must)[0]
    first[cand.ray[rows][::-1]] = rows[::-1]                      # rows are sorted by (ray, t): the nearest clear one wins
    with np.errstate(invalid="ignore"):
        rival = possible & (np.arange(len(cand.ray)) != first[cand.ray]) & ~(cand.t - cand.tol > bound[cand.ray])
    rivals = np.zeros(n, dtype=np.int64)
    np.add.at(rivals, cand.ray, rival)
    clear_ray = (first >= 0) & (rivals == 0) & np.isfinite(bound)
    # (a clear candidate that is not the nearest by t alone but whose bound is the smallest would make `bound` someone else's: then it counts as a rival)
    want_e, want_p = cand.entity[np.maximum(first, 0)], cand.prim[np.maximum(first, 0)]
    bad = clear_ray & ~(is_hit & (ent.astype(np.int64) == want_e) & (prim.astype(np.int64) == want_p))
    assert not bad.any(), "%s R4: clear ray %d reports (%d, %d), expected (%d, %d)" % (label, np.nonzero(bad)[0][0], ent[bad][0], prim[bad][0], want_e[bad][0], want_p[bad][0])
    nothing = np.ones(n, dtype=bool)
    nothing[cand.ray[possible]] = False
    bad = nothing & is_hit
    assert not bad.any(), "%s R2: ray %d comes near nothing in its window but reports a hit" % (label, np.nonzero(bad)[0][0])
    return dict(rays=n, hits=float(is_hit.mean()), clear=float(clear_ray.mean()), with_clear_hit=float(has.mean()), miss_certain=float(nothing.mean()),
                undecided=float(1.0 - (clear_ray | nothing).mean()), undecided_disk=float(cand.undecided_disk.mean()))


def check_any(cand, tmin, distance, occluded, label=""):
    """R6: occluded when a clear candidate lies surely inside (tmin, distance - 0.001]; free when no candidate possibly does.  Returns the undecided share."""
    n = cand.n_rays
    tmin = np.broadcast_to(np.asarray(tmin, dtype=np.float64), (n,))
    tmax = np.broadcast_to(np.asarray(distance, dtype=np.float64), (n,)) - 0.001
    occluded = np.asarray(occluded, dtype=bool).reshape(-1)
    sure, possible = _window(cand, tmin, tmax)
    must, may = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    must[cand.ray[cand.clear & sure]] = True
    may[cand.ray[possible]] = True
    bad = must & ~occluded
    assert not bad.any(), "%s R6: ray %d has a clear occluder but is reported free" % (label, np.nonzero(bad)[0][0])
    bad = ~may & occluded
    assert not bad.any(), "%s R6: ray %d has nothing in its window but is reported occluded" % (label, np.nonzero(bad)[0][0])
    return dict(rays=n, occluded=float(occluded.mean()), must=float(must.mean()), undecided=float((may & ~must).mean()))


# ---- radiometry: a disk light of radius R, parallel to a floor at height h, unit radiance, Lambert floor of albedo 1 ---------------------------
def form_factor(a, h, R):
    """Differential element to a parallel, coaxial-offset disk (a: lateral offset of the element from the axis; e.g. Howell's catalogue B-12):
    F = 1/2 [1 - (h^2 + a^2 - R^2) / sqrt((h^2 + a^2 + R^2)^2 - 4 R^2 a^2)].  This is the radiance a unit-albedo Lambert element reflects under a unit-radiance disk."""
    a, h, R = np.asarray(a, dtype=np.float64), float(h), float(R)
    z = h * h + a * a
    return 0.5 * (1.0 - (z - R * R) / np.sqrt((z + R * R) ** 2 - 4.0 * R * R * a * a))


def _gauss(n):
    x, w = np.polynomial.legendre.leggauss(n)
    return 0.5 * (x + 1.0), 0.5 * w


def _G_uv(a, h, Rs, nu=64, nv=64):
    """G(x, y(u, v)) = cos cos' / d^2 on the Gauss-Legendre grid of [0, 1]^2 for the floor point (a, 0, 0) and y = (Rs v cos 2 pi u, Rs v sin 2 pi u, h),
    with the weights: the reference's surfacePoint (Disk.h:19-26), radius LINEAR in v.  Rs: the radius the samples reach (the scaled one)."""
    u, wu = _gauss(nu)
    v, wv = _gauss(nv)
    uu, vv = np.meshgrid(u, v, indexing="ij")
    x, y = Rs * vv * np.cos(2 * np.pi * uu) - a, Rs * vv * np.sin(2 * np.pi * uu)
    d2 = x * x + y * y + h * h
    return h * h / (d2 * d2), wu[:, None] * wv[None, :]


def nee_linear_radius(a, h, R, area_scale=1.0, sample_scale=1.0, moment=1):
    """E[X^moment] of the NEE-only estimator as the reference's code yields it: X = f / pdf with the CLAIMED pdf_A = 1 / (area_scale pi R^2) at points drawn by
    y = M (R v cos 2 pi u, R v sin 2 pi u, 0), (u, v) uniform: X = (1 / pi) G / pdf_A = area_scale R^2 G(x, y(u, v)).  area_scale = |det M| (IEntity.h:70),
    sample_scale = the linear scale of M.  On the axis and unscaled: (R / 2) [R / (h^2 + R^2) + atan(R / h) / h]."""
    G, w = _G_uv(float(a), float(h), float(R) * sample_scale)
    return float((((area_scale * R * R) * G) ** moment * w).sum())


def nee_uniform(a, h, R):
    """What an area-uniform sampler with the same pdf gives: the true form factor (for telling the two samplers apart)."""
    return float(form_factor(a, h, R))


def _G_disk(a, h, R, nr=64, nphi=128):
    """G on a polar Gauss grid over the disk of radius R (the LOCAL one, which rays hit), with area weights."""
    s, ws = _gauss(nr)
    p, wp = _gauss(nphi)
    ss, pp = np.meshgrid(R * s, 2 * np.pi * p, indexing="ij")
    x, y = ss * np.cos(pp) - a, ss * np.sin(pp)
    d2 = x * x + y * y + h * h
    return h * h / (d2 * d2), (R * ws)[:, None] * (2 * np.pi * wp)[None, :] * ss


def mis_terms(a, h, R):
    """The default integrator (NEE + MIS, balance heuristic) on the floor point, derived in tests/test_gpu_disk.py: returns (E light term, E bsdf term,
    second moment light term, second moment bsdf term).  With P = pi pdf_A = 1 / R^2:
      light sample   X_l = G / (P + G)            at y(u, v), (u, v) uniform
      bsdf sample    X_b = G / (P + G) on the disk, 0 beside it; the direction is cosine distributed: E[X_b^k] = (1 / pi) int_disk G (G / (P + G))^k dA."""
    P = 1.0 / (R * R)
    G, w = _G_uv(float(a), float(h), float(R))
    xl = G / (P + G)
    Gd, wd = _G_disk(float(a), float(h), float(R))
    xb = Gd / (P + Gd)
    return float((xl * w).sum()), float((Gd * xb * wd).sum() / np.pi), float((xl * xl * w).sum()), float((Gd * xb * xb * wd).sum() / np.pi)
