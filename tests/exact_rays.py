"""Exact-arithmetic reference for ray / triangle queries, and the rules a traversal has to satisfy against it (TEST INFRASTRUCTURE ONLY:
plain numpy and Python integers, no checker, no product import).

Every finite binary floating-point number is a rational, so for fp32 (or float64) rays and triangles it is DECIDABLE which triangles
a ray's line pierces, where, and with which barycentrics.  With a = p0 - o, b = p1 - o, c = p2 - o and [x, y, z] = x . (y x z):

    E0 = [d, b, c]   E1 = [d, c, a]   E2 = [d, a, b]          the signed edge functions (edge p1p2, p2p0, p0p1)
    det = E0 + E1 + E2 = d . ((p1 - p0) x (p2 - p0))           t = [a, b, c] / det     u = E1 / det     v = E2 / det

so that o + t d = (1 - u - v) p0 + u p1 + v p2.  The line pierces the triangle strictly inside iff E0, E1, E2 are all > 0 or all < 0
(either winding), touches its boundary iff at least one is zero, not all are, and the others have one sign; det == 0 is never a hit.

classify() decides this in three stages, none of which has a tolerance of its own:

 1. all ray x triangle pairs, float64, in Pluecker form: E = d . (q x r) + (o x d) . (r - q) for the edge q -> r, i.e. a dot product of six
    per-ray with six per-edge numbers, one matrix product per edge.  Error: for fp32 inputs the products in q x r and o x d are exact in float64
    and each component costs 1 rounding; float64 inputs with long mantissas (transformed vertices) round the two products as well: 2 per component;
    r - q: 1; each of the six products: 1; the sum of six terms in whatever order: 5; the division of the edge's row by its length and of the ray's by
    |d| (both only scale the row, for the margin below): 2.  At most 12 roundings, each relative to ABSOLUTE terms -- |q_i r_j| + |q_j r_i|, |q| + |r|
    for the edge's row (its entries may cancel, their errors do not), the ray's own for its row -- whose sum is bounded (Cauchy-Schwarz) by |ray row| x
    |absolute edge row|: |error| <= 16 x 2^-53 x that product (16 rather than 12 pays for the rounding of the norms themselves, for the cancellation in
    o x d, which is relative to the same |ray row| up to sqrt 2, and for gamma_n = n u / (1 - n u)).  A pair is DROPPED only when, beyond
    that bound plus the caller's margin (a distance: rows are scaled so that E is a distance times sin(d, edge) <= distance), one edge
    function is certainly positive and another certainly negative beyond the margin -- the line then passes the triangle farther than the margin.
 2. the survivors (few per ray), float64, as plain triple products with a = p0 - o etc.: a - o: 1 rounding per component; y x z: product 1,
    difference 1; times x: 1; the sum of three: 2 -- 6 roundings on the sum S of the six absolute products |x_i y_j z_k|, and S itself is
    evaluated with <= 5 roundings of its own: |error| <= 8 x 2^-53 x S (static filter; 8 >= 6 (1 + 6u) / (1 - 6u) with room).  A sign that this
    bound decides is final.
 3. every pair with an undecided sign (|E| <= bound), and every pair whose t the float64 pass cannot certify to 2^-40 relative, is re-evaluated
    with Python integers (a float is an integer x 2^-1074): exact signs, exact t, u, v as fractions, rounded once to float64.

The rules R1 - R6 (check_closest / check_any) hold a kernel's answers to that classification with margins derived from the operation count
of the fp32 kernel, see DELTA_ULPS, TAU_ULPS, BARY_SLACK and COPLANAR_RAD below."""
from fractions import Fraction

import numpy as np

U53 = 2.0 ** -53
EPS32 = 2.0 ** -24          # unit roundoff of fp32
INVALID = 0xFFFFFFFF

# ---- the margins of the rules ------------------------------------------------------------------------------------------------------
# M = the largest absolute coordinate among the ray's origin and the scene's vertices.
#
# DELTA = DELTA_ULPS x 2^-24 x M: how far (perpendicular to the ray) the line an fp32 watertight test effectively tests may lie from the
# exact one.  The test forms p - o (1 rounding of a value <= 2M), one product with |S| <= 1 (1 rounding, and S itself carries the rounding of
# its division: 1 more on a value <= 2M) and one subtraction (1) per sheared coordinate: <= 4 roundings of magnitude <= 2M x 2^-24 each, i.e.
# 8 x 2^-24 x M per sheared coordinate; the edge functions that follow are relative-error operations on these coordinates (their zero case is
# re-evaluated in double).  Two coordinates -> sqrt(2) x 8 < 16 with the factor 2 of safety over the one-coordinate figure the rules ask for.
DELTA_ULPS = 16.0
# A transformed entity's world vertices are three products and three sums in fp32 per coordinate, of which the reference's float64 transform
# has none: <= 3 x 2^-24 x M per coordinate (the last two sums round values <= M, the products are smaller), sqrt(3) x that as a distance.
TRANSFORM_ULPS = 3.0 * np.sqrt(3.0)
# TAU = TAU_ULPS x 2^-24 x max(t, M): the rounding of t = T / det.  Az = Sz x (p - o)_kz: 2 roundings + Sz's own; T = (U Az + V Bz) + W Cz: 3
# products and 2 sums; det: 2 sums; the quotient as a reciprocal and a product: 2 -- about 8 relative roundings on values bounded by max(t, M)
# once U, V, W are taken as the barycentric weights they are (non-negative, so the sums do not cancel).  The shear's perturbation of the pierce
# point moves t by up to DELTA / tan(angle to the plane) ON TOP of TAU (Geometry.slide), which is why R2's comparison is skipped below COPLANAR_RAD.
TAU_ULPS = 8.0
# u = V / det, v = W / det with U, V, W of one sign in fp32: each is >= 0 up to the rounding of the reciprocal and the product (2 x 2^-24) --
# only 1 - u - v can go below zero, by the rounding of det's two sums and of u, v: <= 6 x 2^-24 < 2^-21.  2^-20 is twice that.
BARY_SLACK = 2.0 ** -20
# R2 compares the reported t with the exact PLANE distance of the reported triangle.  A ray that is displaced by DELTA sideways moves along a
# plane it meets at angle phi by DELTA / tan(phi): with phi >= 1e-3 rad that is <= 1000 DELTA = 1.6e4 x 2^-24 x M, far beyond TAU -- so the
# comparison that IS made uses TAU + DELTA / tan(phi), and so does R1's bound on the reported distance; the cut-off only removes rays where even that bound is vacuous (> 1e-3 M).
COPLANAR_RAD = 1e-3


def _as64(x, shape):
    a = np.ascontiguousarray(x, dtype=np.float64).reshape(shape)
    assert np.isfinite(a).all()
    return a


def scene_extent(tris):
    return float(np.abs(np.asarray(tris, dtype=np.float64)).max())


def ray_extent(org, tris_extent):
    return np.maximum(np.abs(np.asarray(org, dtype=np.float64)).max(axis=1), tris_extent)


# ---- stage 3: exact ---------------------------------------------------------------------------------------------------------------
_SCALE = 1 << 1074


def _int(x):
    n, d = float(x).as_integer_ratio()      # d is a power of two <= 2^1074
    return n * (_SCALE // d)


def _triple(x, y, z):
    return (x[0] * (y[1] * z[2] - y[2] * z[1]) + x[1] * (y[2] * z[0] - y[0] * z[2]) + x[2] * (y[0] * z[1] - y[1] * z[0]))


def exact_pair(o, d, p0, p1, p2):
    """(E0, E1, E2, det, T) as Python integers on one common scale: signs, and t = T / det, u = E1 / det, v = E2 / det, exact."""
    o, d, p0, p1, p2 = ([_int(c) for c in x] for x in (o, d, p0, p1, p2))
    a, b, c = ([p[i] - o[i] for i in range(3)] for p in (p0, p1, p2))
    e0, e1, e2 = _triple(d, b, c), _triple(d, c, a), _triple(d, a, b)
    return e0, e1, e2, e0 + e1 + e2, _triple(a, b, c)


def exact_kind(e0, e1, e2):
    """2 = pierced strictly inside, 1 = touched on an edge or a vertex, 0 = neither (a degenerate triangle, det == 0, is never hit)."""
    pos, neg = (e0 > 0) + (e1 > 0) + (e2 > 0), (e0 < 0) + (e1 < 0) + (e2 < 0)
    if pos and neg:
        return 0
    if pos == 3 or neg == 3:
        return 2
    return 1 if (pos or neg) else 0        # all three zero: det == 0


def _ratio(n, d):
    return float(Fraction(n, d))           # one rounding of the exact quotient


# ---- stage 2: float64 triple products with a static bound ------------------------------------------------------------------------------
def _triple64(x, y, z):
    """[x, y, z] and the sum of its six absolute products, row-wise."""
    p = [x[:, 0] * y[:, 1] * z[:, 2], x[:, 0] * y[:, 2] * z[:, 1], x[:, 1] * y[:, 2] * z[:, 0],
         x[:, 1] * y[:, 0] * z[:, 2], x[:, 2] * y[:, 0] * z[:, 1], x[:, 2] * y[:, 1] * z[:, 0]]
    val = (x[:, 0] * (y[:, 1] * z[:, 2] - y[:, 2] * z[:, 1]) + x[:, 1] * (y[:, 2] * z[:, 0] - y[:, 0] * z[:, 2])
           + x[:, 2] * (y[:, 0] * z[:, 1] - y[:, 1] * z[:, 0]))
    s = np.abs(p[0]) + np.abs(p[1]) + np.abs(p[2]) + np.abs(p[3]) + np.abs(p[4]) + np.abs(p[5])
    return val, 8.0 * U53 * s


def pairs64(o, d, P):
    """Float64 pass over explicit pairs (row i: ray o[i], d[i] against triangle P[i], 3 x 3): E (n x 3), det, T and their error bounds."""
    a, b, c = P[:, 0] - o, P[:, 1] - o, P[:, 2] - o
    e0, b0 = _triple64(d, b, c)
    e1, b1 = _triple64(d, c, a)
    e2, b2 = _triple64(d, a, b)
    det, bd = _triple64(d, P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    bd = bd + 2.0 * U53 * np.abs(det)      # P1 - P0 is a difference of INPUTS here, rounded like a - o: already in the 8
    T, bt = _triple64(a, b, c)
    return np.stack([e0, e1, e2], 1), np.stack([b0, b1, b2], 1), det, bd, T, bt


def line_triangle_distance(o, d, P):
    """Float64 distance between the LINE o + s d and triangle P (row-wise; 0 is NOT decided here -- callers know from the exact signs whether
    the line meets the triangle): the smallest distance between the line and the three edge segments, in the plane perpendicular to d."""
    dn = d / np.linalg.norm(d, axis=1, keepdims=True)
    best = np.full(len(o), np.inf)
    for i, j in ((1, 2), (2, 0), (0, 1)):
        w, e = P[:, i] - o, P[:, j] - P[:, i]
        w = w - (w * dn).sum(1, keepdims=True) * dn
        e = e - (e * dn).sum(1, keepdims=True) * dn
        ee = (e * e).sum(1)
        s = np.clip(-(w * e).sum(1) / np.where(ee > 0, ee, 1.0), 0.0, 1.0)
        best = np.minimum(best, np.linalg.norm(w + s[:, None] * e, axis=1))
    return best


def plane_angle_sine(d, P):
    """sin of the angle between the ray and the triangle's plane (float64; 0 for a degenerate triangle)."""
    N = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    with np.errstate(all="ignore"):
        s = np.abs((N * d).sum(1)) / (np.linalg.norm(N, axis=1) * np.linalg.norm(d, axis=1))
    return np.where(np.isfinite(s), s, 0.0)


def line_edge_distances(o, d, P):
    """Float64 distances between the line and the three edge LINES (edge i opposite vertex i), n x 3: |E_i| / |d x e_i|; inf for a zero edge."""
    out = np.empty((len(o), 3))
    for k, (i, j) in enumerate(((1, 2), (2, 0), (0, 1))):
        e = P[:, j] - P[:, i]
        n = np.cross(d, e)
        nn = np.linalg.norm(n, axis=1)
        out[:, k] = np.where(nn > 0, np.abs(((P[:, i] - o) * n).sum(1)) / np.where(nn > 0, nn, 1.0), np.inf)
    return out


# ---- stage 1: all pairs ----------------------------------------------------------------------------------------------------------------
def candidate_pairs(org, direction, tris, margin, chunk_elems=6_000_000):
    """Indices (ray, tri) of every pair whose line passes the triangle within `margin` (per ray, a distance) -- a superset: pairs are dropped only
    on certain signs beyond the margin and the float64 error bound (module docstring, stage 1)."""
    o, d, P = _as64(org, (-1, 3)), _as64(direction, (-1, 3)), _as64(tris, (-1, 3, 3))
    margin = np.broadcast_to(np.asarray(margin, dtype=np.float64), (len(o),))
    dl = np.linalg.norm(d, axis=1)
    assert (dl > 0).all()
    R = np.concatenate([d, np.cross(o, d)], 1) / dl[:, None]            # rows: (d, o x d) / |d|
    Rn = np.linalg.norm(R, axis=1)
    L, Ln_max = [], 0.0
    for i, j in ((1, 2), (2, 0), (0, 1)):
        q, r = P[:, i], P[:, j]
        e = r - q
        el = np.linalg.norm(e, axis=1)
        row = np.concatenate([np.cross(q, r), e], 1) / np.where(el > 0, el, 1.0)[:, None]
        aq, ar = np.abs(q), np.abs(r)              # the bound is on the ABSOLUTE products (float64 vertices: q x r rounds, and may cancel)
        mag = np.concatenate([aq[:, [1, 2, 0]] * ar[:, [2, 0, 1]] + aq[:, [2, 0, 1]] * ar[:, [1, 2, 0]], aq + ar], 1) / np.where(el > 0, el, 1.0)[:, None]
        Ln_max = max(Ln_max, float(np.linalg.norm(mag, axis=1).max()))
        L.append(np.ascontiguousarray(row.T))
    thr = (16.0 * U53 * Ln_max) * Rn * (1.0 + 2.0 ** -20) + margin * (1.0 + 2.0 ** -20)
    rows = max(1, chunk_elems // max(len(P), 1))
    out_r, out_t = [], []
    for s in range(0, len(o), rows):
        G0, G1, G2 = R[s:s + rows] @ L[0], R[s:s + rows] @ L[1], R[s:s + rows] @ L[2]
        lo = np.minimum(np.minimum(G0, G1), G2)
        hi = np.maximum(np.maximum(G0, G1), G2)
        th = thr[s:s + rows, None]
        keep = ~((lo < -th) & (hi > th))
        r, t = np.nonzero(keep)
        out_r.append(r + s)
        out_t.append(t)
    return np.concatenate(out_r), np.concatenate(out_t)


class Classification:
    """Sparse table of the (ray, triangle) pairs the reference has something to say about, sorted by ray:
    kind 2 pierced strictly inside / 1 touched / 0 near (within the margin, not met); t, u, v exact values rounded to float64 (nan for kind 0
    pairs whose exact det is 0); edge_dist = the smallest distance between the ray's line and the triangle's three edge lines (kind 2), dist =
    distance between line and triangle (0 for kinds 1, 2); n_exact = pairs that went through the integer stage."""

    def __init__(self, n_rays, ray, tri, kind, t, u, v, edge_dist, dist, sin_phi, n_exact):
        order = np.lexsort((tri, ray))
        self.n_rays = n_rays
        self.ray, self.tri, self.kind = ray[order], tri[order], kind[order]
        self.t, self.u, self.v, self.edge_dist, self.dist, self.sin_phi = t[order], u[order], v[order], edge_dist[order], dist[order], sin_phi[order]
        self.n_exact = n_exact

    def take(self, rays):
        """The table of the ray set `rays` (indices into this one's rays, repeats allowed)."""
        lo, hi = np.searchsorted(self.ray, rays), np.searchsorted(self.ray, np.asarray(rays) + 1)
        idx = np.concatenate([np.arange(a, b) for a, b in zip(lo, hi)]) if len(rays) else np.zeros(0, dtype=np.int64)
        ray = np.repeat(np.arange(len(rays)), hi - lo)
        return Classification(len(rays), ray, self.tri[idx], self.kind[idx], self.t[idx], self.u[idx], self.v[idx], self.edge_dist[idx], self.dist[idx], self.sin_phi[idx], 0)

    def of_ray(self, r):
        lo, hi = np.searchsorted(self.ray, [r, r + 1])
        return slice(lo, hi)


def classify_pairs(o, d, P, force_exact=False):
    """kind, t, u, v, n_exact for explicit pairs (stages 2 and 3)."""
    E, B, det, bd, T, bt = pairs64(o, d, P)
    n = len(o)
    decided = (np.abs(E) > B).all(1) & (np.abs(det) > bd)
    pos, neg = (E > 0).sum(1), (E < 0).sum(1)
    kind = np.where(decided, np.where((pos == 3) | (neg == 3), 2, 0), -1)
    with np.errstate(all="ignore"):
        t, u, v = T / det, E[:, 1] / det, E[:, 2] / det
        # certified relative error of the float64 quotient: (bt + |t| bd) / (|det| - bd), + the division's own rounding
        terr = (bt + np.abs(t) * bd) / (np.abs(det) - bd) + U53 * np.abs(t)
        uerr = (B[:, 1] + np.abs(u) * bd) / (np.abs(det) - bd) + (B[:, 2] + np.abs(v) * bd) / (np.abs(det) - bd)
        poor = ~(terr <= 2.0 ** -40 * np.abs(t)) | ~(uerr <= 2.0 ** -40)
    todo = np.nonzero((kind < 0) | (poor & (kind == 2)) | force_exact)[0]
    for i in todo:
        e0, e1, e2, de, Te = exact_pair(o[i], d[i], P[i, 0], P[i, 1], P[i, 2])
        kind[i] = exact_kind(e0, e1, e2)
        if de != 0:
            t[i], u[i], v[i] = _ratio(Te, de), _ratio(e1, de), _ratio(e2, de)
        else:
            t[i] = u[i] = v[i] = np.nan
    return kind, t, u, v, len(todo)


def classify(org, direction, tris, margin=0.0, force_exact=False):
    """Exact classification of fp32 (or float64) rays against world-space triangles (n x 3 x 3); `margin` (scalar or per ray) also keeps the
    triangles the line passes within that distance (kind 0), which R2, R4 and R6 need.  The ray's window is NOT applied here."""
    o, d, P = _as64(org, (-1, 3)), _as64(direction, (-1, 3)), _as64(tris, (-1, 3, 3))
    margin = np.ascontiguousarray(np.broadcast_to(np.asarray(margin, dtype=np.float64), (len(o),)))
    r, k = candidate_pairs(o, d, P, margin)
    kind, t, u, v, n_exact = classify_pairs(o[r], d[r], P[k], force_exact)
    dist = np.where(kind > 0, 0.0, line_triangle_distance(o[r], d[r], P[k]))
    keep = (kind > 0) | (dist <= margin[r])
    edge = line_edge_distances(o[r], d[r], P[k]).min(1)
    sin_phi = plane_angle_sine(d[r], P[k])
    return Classification(len(o), r[keep], k[keep], kind[keep], t[keep], u[keep], v[keep], edge[keep], dist[keep], sin_phi[keep], n_exact)


# ---- a numpy restatement of the fp32 statement sequence (for checking the margins on the CPU, not a reference) ------------------------------
def woop32(o, d, P):
    """The watertight test as fp32 kernels state it (Woop, Benthin, Wald 2013), row-wise in numpy float32: accepted, t, u, v."""
    f = np.float32
    o, d, P = o.astype(f), d.astype(f), P.astype(f)
    n = len(o)
    ad = np.abs(d)
    kz = np.zeros(n, dtype=np.int64)
    kz[ad[:, 1] > ad[:, 0]] = 1
    kz[ad[:, 2] > ad[np.arange(n), kz]] = 2
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    neg = d[np.arange(n), kz] < 0
    kx, ky = np.where(neg, ky, kx), np.where(neg, kx, ky)
    ar = np.arange(n)
    with np.errstate(all="ignore"):
        Sx, Sy, Sz = d[ar, kx] / d[ar, kz], d[ar, ky] / d[ar, kz], f(1) / d[ar, kz]
        A, B, C = P[:, 0] - o, P[:, 1] - o, P[:, 2] - o
        Ax, Ay = A[ar, kx] - Sx * A[ar, kz], A[ar, ky] - Sy * A[ar, kz]
        Bx, By = B[ar, kx] - Sx * B[ar, kz], B[ar, ky] - Sy * B[ar, kz]
        Cx, Cy = C[ar, kx] - Sx * C[ar, kz], C[ar, ky] - Sy * C[ar, kz]
        U, V, W = Cx * By - Cy * Bx, Ax * Cy - Ay * Cx, Bx * Ay - By * Ax
        z = (U == 0) | (V == 0) | (W == 0)
        g = np.float64
        U = np.where(z, (Cx.astype(g) * By - Cy.astype(g) * Bx).astype(f), U)
        V = np.where(z, (Ax.astype(g) * Cy - Ay.astype(g) * Cx).astype(f), V)
        W = np.where(z, (Bx.astype(g) * Ay - By.astype(g) * Ax).astype(f), W)
        rej = ((U < 0) | (V < 0) | (W < 0)) & ((U > 0) | (V > 0) | (W > 0))
        det = (U + V) + W
        rej |= det == 0
        T = (U * (Sz * A[ar, kz]) + V * (Sz * B[ar, kz])) + W * (Sz * C[ar, kz])
        rcp = f(1) / det
        return ~rej, T * rcp, V * rcp, W * rcp


# ---- the rules -------------------------------------------------------------------------------------------------------------------------
class Geometry:
    """World-space triangles (float64, n x 3 x 3) of a scene with the (entity, primitive) id of each, and the margins' scale."""

    def __init__(self, tris, entity, prim, transformed=False, extra_ulps=0.0):
        self.tris = _as64(tris, (-1, 3, 3))
        self.entity, self.prim = np.asarray(entity, dtype=np.int64), np.asarray(prim, dtype=np.int64)
        self.extent = scene_extent(self.tris)
        # extra_ulps: a displacement of the tested line that is not the triangle test's (rays the caller knows only up to a rounding), as the transform's is
        self.delta_ulps = DELTA_ULPS + (TRANSFORM_ULPS if transformed else 0.0) + extra_ulps
        # exact duplicates (same vertices in the same order): the lowest index stands for all of them
        _, first, inverse = np.unique(self.tris.reshape(len(self.tris), 9), axis=0, return_index=True, return_inverse=True)
        self.canonical = first[inverse.reshape(-1)]
        self.lookup = {(int(e), int(p)): i for i, (e, p) in enumerate(zip(self.entity, self.prim))}

    def delta(self, org):
        return self.delta_ulps * EPS32 * ray_extent(org, self.extent)

    def slide(self, org_extent, sin_phi):
        """How far t moves when the tested line is DELTA beside the exact one and the vertices a transform's rounding beside theirs: the pierce point
        slides along the plane by DELTA / tan(phi), and a plane displaced by e is met e / sin(phi) earlier or later.  inf below COPLANAR_RAD."""
        with np.errstate(all="ignore"):
            tan_phi = sin_phi / np.sqrt(np.maximum(1.0 - sin_phi * sin_phi, 1e-300))
            s = DELTA_ULPS * EPS32 * org_extent / tan_phi + (self.delta_ulps - DELTA_ULPS) * EPS32 * org_extent / sin_phi
        return np.where(sin_phi >= np.sin(COPLANAR_RAD), s, np.inf)

    def index_of(self, ent, prim):
        return np.array([self.lookup.get((int(e), int(p)), -1) for e, p in zip(ent, prim)], dtype=np.int64)


def _tau(t, M):
    return TAU_ULPS * EPS32 * np.maximum(np.abs(t), M)


def _segment_min(values, seg_ray, n_rays, fill=np.inf):
    out = np.full(n_rays, fill)
    np.minimum.at(out, seg_ray, values)
    return out


def qualifying(geo, cls, org, tmin, tmax):
    """R1's set: pierced strictly inside, >= DELTA from its three edges, exact t in [tmin + tau', tmax - tau'] with tau' = tau + the slide along the
    plane -- the same bound R1 then puts on the reported distance: a kernel whose t may legitimately be tau' off must not be asked for a hit that it may
    legitimately see outside the window.  Mask over cls's rows."""
    M = ray_extent(org, geo.extent)[cls.ray]
    tau = _tau(cls.t, M) + geo.slide(M, cls.sin_phi)
    delta = geo.delta_ulps * EPS32 * M
    with np.errstate(invalid="ignore"):
        return (cls.kind == 2) & (cls.edge_dist >= delta * (1 + 2.0 ** -30)) & (cls.t >= tmin[cls.ray] + tau) & (cls.t <= tmax[cls.ray] - tau)


def clear_rays(geo, cls, org, tmin, tmax):
    """R4's clear rays.  A triangle can be the one reported only if its fp32 distance can be <= R1's bound, i.e. if its exact t less tau and less its slide
    is; the ray is clear when exactly one triangle (up to exact duplicates) can, and that one qualifies.  This is the rule's "one qualifying triangle within
    2 tau of the nearest, nothing else met or near there" with every triangle's own margin instead of a common 2 tau.  Returns the mask, the nearest exact t
    met in the window (inf: nothing met -- not R4's population) and the expected entity / primitive."""
    n = cls.n_rays
    M = ray_extent(org, geo.extent)
    Q = qualifying(geo, cls, org, tmin, tmax)
    tau_c = _tau(cls.t, M[cls.ray])
    slide_c = geo.slide(M[cls.ray], cls.sin_phi)
    bound = _segment_min(np.where(Q, cls.t + tau_c + slide_c, np.inf), cls.ray, n)
    with np.errstate(invalid="ignore"):
        in_window = (cls.t >= tmin[cls.ray] - tau_c) & (cls.t <= tmax[cls.ray] + tau_c) | ~np.isfinite(cls.t)
        around = in_window & ~(cls.t - tau_c - slide_c > bound[cls.ray])        # (no finite t, or below COPLANAR_RAD: around)
        nearest = _segment_min(np.where(in_window & (cls.kind > 0), cls.t, np.inf), cls.ray, n)
    canon = geo.canonical[cls.tri]
    first_q = np.full(n, -1, dtype=np.int64)
    qa = Q & around
    first_q[cls.ray[qa][::-1]] = canon[qa][::-1]
    others = np.zeros(n, dtype=np.int64)
    np.add.at(others, cls.ray, around & (canon != first_q[cls.ray]))
    clear = (first_q >= 0) & (others == 0) & np.isfinite(nearest)
    return clear, nearest, geo.entity[np.maximum(first_q, 0)], geo.prim[np.maximum(first_q, 0)]


def check_identity(geo, cls, org, tmin, tmax, ent, prim, must_hit=None, label=""):
    """R4 and R5 alone, for answers that carry ids only (the path kernel's primary-hit plane)."""
    o = _as64(org, (-1, 3))
    n = len(o)
    tmin = np.broadcast_to(np.asarray(tmin, dtype=np.float64), (n,))
    tmax = np.broadcast_to(np.asarray(tmax, dtype=np.float64), (n,))
    ent, prim = np.asarray(ent).reshape(-1), np.asarray(prim).reshape(-1)
    is_hit = ent != INVALID
    if must_hit is not None:
        assert not (must_hit & ~is_hit).any(), "%s R5: ray %d into a closed surface leaks" % (label, np.nonzero(must_hit & ~is_hit)[0][0])
    clear, nearest, want_e, want_p = clear_rays(geo, cls, o, tmin, tmax)
    bad = clear & ~(is_hit & (ent.astype(np.int64) == want_e) & (prim.astype(np.int64) == want_p))
    assert not bad.any(), "%s R4: clear ray %d reports (%d, %d), expected (%d, %d)" % (
        label, np.nonzero(bad)[0][0], ent[bad][0], prim[bad][0], want_e[bad][0], want_p[bad][0])
    met = np.isfinite(nearest)
    return dict(rays=n, hits=float(is_hit.mean()), r4_skipped=float(1.0 - clear[met].mean()) if met.any() else 0.0, clear=float(clear.mean()))


def check_closest(geo, cls, org, direction, tmin, tmax, hit, must_hit=None, label=""):
    """R1 - R5 for a closest-hit answer `hit` = (entity, prim, u, v, t).  Returns the shares the caps are stated on; raises AssertionError with
    the first offending ray otherwise."""
    o, d = _as64(org, (-1, 3)), _as64(direction, (-1, 3))
    n = len(o)
    tmin = np.broadcast_to(np.asarray(tmin, dtype=np.float64), (n,))
    tmax = np.broadcast_to(np.asarray(tmax, dtype=np.float64), (n,))
    ent, prim, hu, hv, ht = (np.asarray(x) for x in hit)
    is_hit = ent != INVALID
    ht64 = ht.astype(np.float64)
    M = ray_extent(o, geo.extent)
    delta = geo.delta(o)

    def fail(rule, idx, extra=""):
        r = int(idx)
        s = cls.of_ray(r)
        raise AssertionError("%s %s: ray %d o=%r d=%r window=(%r, %r) reported=(%r, %r, u=%r, v=%r, t=%r) exact=%s %s" % (
            label, rule, r, org[r].tolist(), direction[r].tolist(), float(tmin[r]), float(tmax[r]), int(ent[r]), int(prim[r]), float(hu[r]), float(hv[r]),
            float(ht[r]), list(zip(cls.tri[s].tolist(), cls.kind[s].tolist(), cls.t[s].tolist(), cls.edge_dist[s].tolist(), cls.dist[s].tolist())), extra))

    # R1 no miss + R3 nearest: every qualifying triangle bounds the reported distance from above
    Q = qualifying(geo, cls, o, tmin, tmax)
    tau_c = _tau(cls.t, M[cls.ray])
    slide_c = geo.slide(M[cls.ray], cls.sin_phi)
    bound = _segment_min(np.where(Q, cls.t + tau_c + slide_c, np.inf), cls.ray, n)
    has_q = np.isfinite(bound)
    bad = has_q & ~is_hit
    if bad.any():
        fail("R1 (a clear hit is missed)", np.nonzero(bad)[0][0])
    bad = has_q & is_hit & ~(ht64 <= bound)
    if bad.any():
        fail("R1/R3 (a nearer clear hit exists)", np.nonzero(bad)[0][0])
    # R5 watertight
    if must_hit is not None and (must_hit & ~is_hit).any():
        fail("R5 (a ray into a closed surface leaks)", np.nonzero(must_hit & ~is_hit)[0][0])
    # R2 no phantom
    h = np.nonzero(is_hit)[0]
    k = geo.index_of(ent[h], prim[h])
    if (k < 0).any():
        fail("R2 (unknown entity / primitive id)", h[np.nonzero(k < 0)[0][0]])
    oh, dh, Ph = o[h], d[h], geo.tris[k]
    kind, tk, _, _, _ = classify_pairs(oh, dh, Ph)
    dist = np.where(kind > 0, 0.0, line_triangle_distance(oh, dh, Ph))
    bad = ~(dist <= delta[h])
    if bad.any():
        fail("R2 (the reported triangle is farther than DELTA from the ray)", h[np.nonzero(bad)[0][0]], "distance %r delta %r" % (dist[bad][0], delta[h][bad][0]))
    sin_phi = plane_angle_sine(dh, Ph)
    coplanar = ~(sin_phi >= np.sin(COPLANAR_RAD))
    tau_h = _tau(ht64[h], M[h])
    slide = geo.slide(M[h], sin_phi)
    with np.errstate(all="ignore"):
        bad = ~coplanar & ~(np.abs(ht64[h] - tk) <= tau_h + slide)
    if bad.any():
        i = np.nonzero(bad)[0][0]
        fail("R2 (reported t is not the plane distance of the reported triangle)", h[i], "plane t %r tau %r slide %r" % (tk[i], tau_h[i], slide[i]))
    bad = ~((ht64[h] >= tmin[h] - tau_h) & (ht64[h] <= tmax[h] + tau_h))
    if bad.any():
        fail("R2 (reported t outside the window)", h[np.nonzero(bad)[0][0]])
    u64, v64 = hu[h].astype(np.float64), hv[h].astype(np.float64)
    bad = ~((u64 >= -BARY_SLACK) & (v64 >= -BARY_SLACK) & (1.0 - u64 - v64 >= -BARY_SLACK))
    if bad.any():
        fail("R2 (barycentrics outside the triangle)", h[np.nonzero(bad)[0][0]])
    point = (1.0 - u64 - v64)[:, None] * Ph[:, 0] + u64[:, None] * Ph[:, 1] + v64[:, None] * Ph[:, 2]
    off = np.linalg.norm(point - (oh + ht64[h, None] * dh), axis=1)
    # (no slide here: u, v and t come from the same weights, so the point they describe and o + t d differ by the sheared residual alone)
    bad = ~(off <= delta[h] + tau_h)
    if bad.any():
        i = np.nonzero(bad)[0][0]
        fail("R2 (u, v do not describe the point o + t d: u / v swapped or of another vertex order?)", h[i], "off by %r" % off[i])
    clear, nearest, want_e, want_p = clear_rays(geo, cls, o, tmin, tmax)
    bad = clear & ~(is_hit & (ent.astype(np.int64) == want_e) & (prim.astype(np.int64) == want_p))
    if bad.any():
        r = np.nonzero(bad)[0][0]
        fail("R4 (a clear ray reports another triangle)", r, "expected entity %d prim %d" % (want_e[r], want_p[r]))
    return dict(rays=n, hits=float(is_hit.mean()), with_clear_hit=float(has_q.mean()), r4_skipped=float(1.0 - clear[np.isfinite(nearest)].mean()) if np.isfinite(nearest).any() else 0.0,
                non_clear=float(1.0 - clear.mean()), coplanar_skipped=float(coplanar.sum() / max(n, 1)))


def check_any(geo, cls, org, tmin, distance, occluded, label=""):
    """R6 for an occlusion answer: true when a triangle qualifies inside [tmin + tau, distance - 0.001 - tau]; false when nothing is pierced,
    touched or within DELTA inside [tmin - tau, distance - 0.001 + tau].  (The occlusion query tests (tmin, distance - 0.001].)
    Returns the share of rays neither clause decides."""
    o = _as64(org, (-1, 3))
    n = len(o)
    tmin = np.broadcast_to(np.asarray(tmin, dtype=np.float64), (n,))
    tmax = np.broadcast_to(np.asarray(distance, dtype=np.float64), (n,)) - 0.001
    occluded = np.asarray(occluded, dtype=bool)
    M = ray_extent(o, geo.extent)
    Q = qualifying(geo, cls, o, tmin, tmax)
    must = np.zeros(n, dtype=bool)
    must[cls.ray[Q]] = True
    tau_c = _tau(cls.t, M[cls.ray])
    with np.errstate(invalid="ignore"):
        possible = ~((cls.t < tmin[cls.ray] - tau_c) | (cls.t > tmax[cls.ray] + tau_c))     # (no finite t: possible)
    may = np.zeros(n, dtype=bool)
    may[cls.ray[possible]] = True
    bad = must & ~occluded
    assert not bad.any(), "%s R6: ray %d has a clear occluder but is reported free" % (label, np.nonzero(bad)[0][0])
    bad = ~may & occluded
    assert not bad.any(), "%s R6: ray %d has nothing within DELTA in its window but is reported occluded" % (label, np.nonzero(bad)[0][0])
    return float((may & ~must).mean())
