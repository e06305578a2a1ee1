"""Exact-arithmetic reference for ray / sphere and ray / quadric queries (TEST INFRASTRUCTURE ONLY, beside tests/exact_rays.py and tests/exact_disk.py, which are
imported and not changed: plain numpy, Python integers and fractions, no product import, no checker).  Rows go to exact_disk.Candidates, so that
exact_disk.check_closest / check_any hold a traversal to R1 - R4 and R6 on spheres, quadrics and the triangles around them alike.

fp32 inputs are rationals.  A float64 pass evaluates the expressions below for many rays (a rounding of 2^-53 where the margins are counted in 2^-24); every
(ray, surface) pair whose float64 value lies within 2^-30 (relative) of a decision goes to the exact stage: Python integers / Fractions for the coefficients and
the SIGN of the discriminant, math.isqrt on integers scaled by 2^(2 x 96) for the root's value -- 96 bits below the leading one, more than any margin, so that
"root <= bound" is the comparison of two rationals that differ from the true ones by less than 2^-90 relative.

SPHERE (c, r) as the device holds them: c the fp32 translation, r = sphere_r32().  For any non-zero d, with c0 = c - o:

    proj = c0 . d / |d|^2      perp = c0 - d proj      l^2 = |perp|^2      s2 = r^2 - l^2      td = sqrt(s2) / |d|      t-+ = proj -+ td
    required: the smallest root in (tmin, limit]; from inside, or with the front root behind tmin, the back root; u = v = 0, prim = 0.

Roundings of sphere_hit (device/pr_device.h), u = 2^-24, D = |c0|, l = |perp|, first order:

    rd2 = 1 / d.d            3 (positive sum) + 1                               4 u relative
    c0 = c - o               1 per component
    projC0 = dot(c0, d) rd2  3 + 1 (c0) on sum |c0_i d_i| <= D |d|, 1 + 4 (rd2)  |err| <= 4 u D / |d| + 5 u |proj| <= 9 u D / |d|
    perp = c0 - d projC0     per component u |d_i proj| + u |c0_i| + u |perp_i|; the error of projC0 moves perp ALONG d, perpendicular to perp: second order in l^2
    l2 = dot(perp, perp)     3 relative                                         |err l2| <= 2 l u (2 D + l) + 3 u l^2 = u (4 l D + 5 l^2)
    r2 = r r                 1                                                  u r^2      => |err s2| <= u (r^2 + 4 l D + 5 l^2) =: DS2     (grows like u D l)
    td = sqrt((r2 - l2) rd2) 1 + 1 + 4 (rd2) under the root, 1 of the root      |err td| <= DS2 / (2 sqrt(s2) |d|) + 4 u td
    t = projC0 -+ td         1                                                  u |t|

    GRAZE = 2 DS2:                |s2| <= GRAZE is undecided (l2 <= r2 may fall either way)
    TOL_S(t) = 2 u (9 D / |d| + 4 td + |t|) + min(GRAZE / (2 sqrt(s2)), sqrt(GRAZE)) / |d|       (|sqrt x' - sqrt x| <= sqrt |x' - x| always)

QUADRIC.  The surface is what the device holds: p[10], the local box lo / hi (grown by BBOX_EPS in fp32), the fp32 inverse rows inv, the fp32 world box
wlo / whi and the transform rows m (HeldQuadric restates host/setup.cpp in numpy float32, in its order).  With L0 = inv (o, 1) and ld = inv_lin d taken EXACTLY
from the held inv, the local parameter is the world parameter by construction: the inverse's own rounding needs no margin in t.

    per axis k: the slab values (lo_k - L0_k) / ld_k, (hi_k - L0_k) / ld_k; entry = max(PR_EPSILON, max_k min), exit = min_k max
    P = L0 + entry ld;  a, b, c of Q(P + s ld) = a s^2 + b s + c;  disc = b^2 - 4 a c;  s1 = (-b - sqrt disc) / 2a, s2 = (-b + sqrt disc) / 2a
    |a| <= PR_EPSILON: s = -c / b (whatever a is: the linear branch's regime is the exact a = 0 and its neighbourhood)
    else disc < 0: none; else s = s1 when s1 > INT_EPS, s2 otherwise                 hit iff s >= INT_EPS
    closest: T = entry + s <= exit, [tmin, tmax] overlaps the world box, |M (ld T)| in [tmin, tmax]
    occlusion: the world box overlap and a root s >= INT_EPS -- clipped neither to the exit nor to the window (quadric.cpp:222-230, kept)

The root rule is Quadric.h:61-64 restated: for a > 0 it is "the smallest root beyond INT_EPS past the entry"; for a < 0 the division by 2a turns the order round,
s1 is the LARGER root, and the larger root is the answer whenever it lies beyond INT_EPS.

Roundings of quadric_hit / quadric_roots (S_x = the sum of the absolute terms of x).  The table gives the COUNT and the closed bound it implies; the code (class Err)
accumulates the same roundings operation by operation in the device's order -- u |result| per sum, product and quotient, the operands' bounds carried along -- and
leaves out the operations that are exact in binary floating point whatever their size: a sum with an exact zero, a product with an exact zero or power of two.  That
is what makes the identity and the exactly invertible transforms as sharp as they are (1 x + 0 y + 0 z - 2^k costs one rounding, not four):

    L0_k: ((i0 ox + i1 oy) + i2 oz) + i3    4        dL0_k <= 4 u (|inv_k| . |o| + |i3|)            ld_k: 3       dld_k <= 3 u |inv_k| . |d|
    slab value v = (1 / ld_k) (lo_k - L0_k)  3 relative, and the errors of L0, ld:                    dv <= |v| (dld_k / |ld_k| + 3 u) + dL0_k / |ld_k|
    P_k = L0_k + ld_k entry                  2        dP_k <= u (|ld_k| entry + |P_k|) + dL0_k + dld_k entry
        (the error of entry ITSELF moves P along ld and s by the opposite amount: T = entry + s does not see it; only the decisions on s and exit do)
    a  2 products + 5 sums = 7    da <= 7 u S_a + |dQ''(ld)| . dld
    b  2 products (or product, sum, product) + 8 sums = 10    db <= 10 u S_b + |grad Q(P)| . dld + |Q''(ld)| . dP
    c  2 products + 9 sums = 11   dc <= 11 u S_c + |grad Q(P)| . dP          (the entry point's rounding, through |grad Q|)
    disc = b b - 4 a c   3        ddisc <= u (b^2 + 4 |a c| + |disc|) + 2 |b| db + 4 (|a| dc + |c| da)
    root = sqrt(disc) 1; -b -+ root 1; / (2 a) 1; t += entry 1

    GRAZE_Q = 2 ddisc:  |disc| <= GRAZE_Q is undecided
    sensitivity   (s^2 da + |s| db + dc) / sqrt(disc)                            (implicit differentiation of a s^2 + b s + c = 0; blows up at grazing)
              or  (db + min(ddisc' / (2 sqrt disc), sqrt ddisc')) / |2a| + |s| da / |a|   (the formula's own propagation, ddisc' the propagated part; blows up as a -> 0)
    cancellation  u ((b^2 + 4 |a c| + |disc|) / (2 sqrt disc) + sqrt disc + |-b -+ sqrt disc|) / |2a| + u |s|
    TOL_Q(s) = 2 (min of the two sensitivities + cancellation);   TOL_T = TOL_Q + 2 u |T| + (| |M ld| - 1 | + 10 u) T
        (the last term: the window is tested on |M (ld' T)| -- 5 roundings -- where the rules test T; the families' quadric rays have |d| = 1 up to fp32)
    linear: TOL_Q(s) = 2 ((dc + |s| db) / |b| + u |s|)

A ray is UNDECIDED for a surface when the discriminant lies within GRAZE of 0, the pierce parameter within TOL of exit (plus exit's own error) or of the world box's
entry or exit, s within TOL (plus entry's error) of INT_EPS, |a| within 2 da of PR_EPSILON, a sphere's front root within TOL_S of tmin -- and only then.  Outside
those bands the surface MUST be reported (clear) or MUST NOT (no row).  Window ends are exact_disk._window's, through the row's tol."""
import math
from fractions import Fraction

import numpy as np

import exact_disk as D
import exact_rays as X

U = X.EPS32
F = np.float32
PR_EPSILON = float(F(1.1920929e-07))
INT_EPS = float(F(1e-6))
BBOX_EPS = F(1e-4)
ROOT_BITS = 96


# ---- the fp32 values the library holds ---------------------------------------------------------------------------------------------------------
def sphere_r32(T, radius):
    """sphere_r of host/setup.cpp: radius x the mean column norm of the linear part, in float32 and in its order."""
    m = np.asarray(T, dtype=F).reshape(4, 4)
    n = [np.sqrt((m[0, j] * m[0, j] + m[1, j] * m[1, j]) + m[2, j] * m[2, j]) for j in range(3)]
    r = F(radius) * (((n[0] + n[1]) + n[2]) / F(3))
    assert r.dtype == F
    return r


class HeldQuadric:
    """p[10], lo / hi (grown), inv[12], wlo / whi, m[12] as fp32 arrays: host/setup.cpp entity_tables restated in numpy float32."""

    def __init__(self, T, params, box_min, box_max):
        M = np.asarray(T, dtype=F).reshape(4, 4)
        m = M[:3].reshape(12).copy()
        a, b, c, dd, ee, f, g, h, i = m[0], m[1], m[2], m[4], m[5], m[6], m[8], m[9], m[10]
        cof = [ee * i - f * h, f * g - dd * i, dd * h - ee * g, c * h - b * i, a * i - c * g, b * g - a * h, b * f - c * ee, c * dd - a * f, a * ee - b * dd]
        det = (a * cof[0] + b * cof[1]) + c * cof[2]
        nm = [k / det for k in cof]
        self.p = np.asarray(params, dtype=F)
        assert self.p.shape == (10,)
        self.lo = np.asarray(box_min, dtype=F) - BBOX_EPS
        self.hi = np.asarray(box_max, dtype=F) + BBOX_EPS
        inv = np.zeros(12, dtype=F)
        for r in range(3):
            for c2 in range(3):
                inv[4 * r + c2] = nm[3 * c2 + r]
            inv[4 * r + 3] = -((inv[4 * r] * m[3] + inv[4 * r + 1] * m[7]) + inv[4 * r + 2] * m[11])
        wlo, whi = np.full(3, np.inf, dtype=F), np.full(3, -np.inf, dtype=F)
        for corner in range(8):
            cc = [self.hi[k] if corner & (1 << k) else self.lo[k] for k in range(3)]
            for r in range(3):
                w = ((m[4 * r] * cc[0] + m[4 * r + 1] * cc[1]) + m[4 * r + 2] * cc[2]) + m[4 * r + 3]
                wlo[r], whi[r] = min(wlo[r], w), max(whi[r], w)
        self.inv, self.wlo, self.whi, self.m = inv, wlo, whi, m
        assert all(x.dtype == F for x in (self.p, self.lo, self.hi, self.inv, self.wlo, self.whi, self.m))


# ---- the quadric's polynomial, for floats, arrays and Fractions alike ----------------------------------------------------------------------------
def coefficients(p, o, d):
    A, B, C, Dq, E, Fq, G, H, I, J = p
    ox, oy, oz = o
    dx, dy, dz = d
    a = A * dx * dx + B * dy * dy + C * dz * dz + Dq * dx * dy + E * dx * dz + Fq * dy * dz
    b = (2 * A * ox * dx + 2 * B * oy * dy + 2 * C * oz * dz + Dq * (ox * dy + oy * dx) + E * (ox * dz + oz * dx) + Fq * (oy * dz + oz * dy)
         + G * dx + H * dy + I * dz)
    c = A * ox * ox + B * oy * oy + C * oz * oz + Dq * ox * oy + E * ox * oz + Fq * oy * oz + G * ox + H * oy + I * oz + J
    return a, b, c


def gradient(p, x):
    A, B, C, Dq, E, Fq, G, H, I, _ = p
    return (2 * A * x[0] + Dq * x[1] + E * x[2] + G, Dq * x[0] + 2 * B * x[1] + Fq * x[2] + H, E * x[0] + Fq * x[1] + 2 * C * x[2] + I)


def _sqrt_fraction(x):
    """sqrt of a non-negative Fraction to ROOT_BITS bits below its leading one, as a Fraction (math.isqrt on scaled integers)."""
    if x == 0:
        return Fraction(0)
    n, d = x.numerator, x.denominator
    shift = max(0, ROOT_BITS - (n.bit_length() - d.bit_length()) // 2 + 2)
    return Fraction(math.isqrt((n << (2 * shift)) // d), 1 << shift)


# ---- spheres -------------------------------------------------------------------------------------------------------------------------------
def exact_ray_sphere(o, d, c, r):
    """(sign of r^2 - l^2, t_front, t_back): the sign exact; the roots Fractions good to ROOT_BITS bits (None when the sign is negative)."""
    o, d, c = ([Fraction(float(v)) for v in x] for x in (o, d, c))
    r = Fraction(float(r))
    c0 = [c[k] - o[k] for k in range(3)]
    dd, p, c2 = sum(v * v for v in d), sum(c0[k] * d[k] for k in range(3)), sum(v * v for v in c0)
    disc = p * p - dd * (c2 - r * r)                              # = |d|^2 (r^2 - l^2)
    if disc < 0:
        return -1, None, None
    root = _sqrt_fraction(disc)
    return (1 if disc > 0 else 0), (p - root) / dd, (p + root) / dd


class SphereTable:
    """Per (ray, sphere), arrays [n_rays, n_spheres]: proj, td (0 where s2 < 0), s2 = r^2 - l^2 (its sign exact where the exact stage ran), l, D = |c - o|, |d|."""

    def __init__(self, proj, td, s2, l, dist, dl, n_exact):
        self.proj, self.td, self.s2, self.l, self.D, self.dl, self.n_exact = proj, td, s2, l, dist, dl, n_exact


def classify_spheres(org, direction, centres, radii, force_exact=False):
    o, d = X._as64(org, (-1, 3)), X._as64(direction, (-1, 3))
    C, R = X._as64(centres, (-1, 3)), X._as64(radii, (-1,))
    c0 = C[None] - o[:, None]
    dd = (d * d).sum(1)[:, None]
    proj = (c0 * d[:, None]).sum(-1) / dd
    perp = c0 - d[:, None] * proj[..., None]
    l2 = (perp * perp).sum(-1)
    s2 = R[None] ** 2 - l2
    l, dist, dl = np.sqrt(l2), np.linalg.norm(c0, axis=-1), np.sqrt(dd)
    td = np.sqrt(np.maximum(s2, 0.0)) / dl
    todo = (np.abs(s2) <= 2.0 ** -30 * (R[None] ** 2 + 4 * l * dist + 5 * l2)) | force_exact
    idx = np.argwhere(todo)
    for i, k in idx:
        sg, tf, tb = exact_ray_sphere(o[i], d[i], C[k], R[k])
        if sg < 0:
            s2[i, k], td[i, k] = -abs(s2[i, k]) if s2[i, k] != 0 else -np.finfo(np.float64).tiny, 0.0
        else:
            td[i, k], proj[i, k] = float((tb - tf) / 2), float((tb + tf) / 2)
            s2[i, k] = td[i, k] ** 2 * dd[i, 0]
    return SphereTable(proj, td, s2, l, dist, np.broadcast_to(dl, proj.shape), len(idx))


def sphere_graze(tab, R):
    return 2.0 * U * (R ** 2 + 4 * tab.l * tab.D + 5 * tab.l ** 2)


def sphere_tol(tab, R, t):
    g = sphere_graze(tab, R)
    with np.errstate(all="ignore"):
        root = np.minimum(g / (2.0 * np.sqrt(np.maximum(tab.s2, 0.0))), np.sqrt(g))
    return 2.0 * U * (9.0 * tab.D / tab.dl + 4.0 * tab.td + np.abs(t)) + root / tab.dl


def sphere32(o, d, c, r, tmin, limit):
    """sphere_hit of device/pr_device.h restated in numpy float32, row-wise (for checking the margins on the CPU, not a reference): accepted, t."""
    o, d, c = (np.asarray(x, dtype=F) for x in (o, d, c))
    r = F(r)
    tmin, limit = np.broadcast_to(np.asarray(tmin, dtype=F), (len(o),)), np.broadcast_to(np.asarray(limit, dtype=F), (len(o),))
    with np.errstate(all="ignore"):
        rd2 = F(1) / ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        c0 = c[None] - o
        proj = ((c0[:, 0] * d[:, 0] + c0[:, 1] * d[:, 1]) + c0[:, 2] * d[:, 2]) * rd2
        perp = c0 - d * proj[:, None]
        l2 = (perp[:, 0] * perp[:, 0] + perp[:, 1] * perp[:, 1]) + perp[:, 2] * perp[:, 2]
        r2 = r * r
        td = np.sqrt((r2 - l2) * rd2)
        tf, tb = proj - td, proj + td
        front, back = (tf > tmin) & (tf <= limit), (tb > tmin) & (tb <= limit)
        ok = (l2 <= r2) & (front | back)
    return ok, np.where(front, tf, tb)


def _sphere_rows(o, d, spheres, tmin, extra_ulps):
    """Rows of the spheres [(entity, centre, radius)]: the required root given tmin, see the module docstring.  extra_ulps: the caller knows d only up to
    extra_ulps u relative -- the line is up to extra_ulps u max(t, D) beside the restated one: on l (through l^2's error, 2 l x that) and on t alike."""
    n = len(o)
    if not spheres:
        return [np.zeros(0, dtype=np.int64)] * 3 + [np.zeros(0)] * 2 + [np.zeros(0, dtype=bool)], np.zeros(n, dtype=bool)
    R = np.asarray([float(s[2]) for s in spheres])[None]
    tab = classify_spheres(o, d, [s[1] for s in spheres], R[0])
    tf, tb = tab.proj - tab.td, tab.proj + tab.td
    side = extra_ulps * U * np.maximum(np.maximum(np.abs(tf), np.abs(tb)), tab.D / tab.dl)          # in t; x |d| as a distance
    graze = sphere_graze(tab, R) + 2.0 * tab.l * side * tab.dl
    with np.errstate(all="ignore"):
        widen = np.minimum(2.0 * tab.l * side * tab.dl / (2.0 * np.sqrt(np.maximum(tab.s2, 0.0))), np.sqrt(2.0 * tab.l * side * tab.dl)) / tab.dl + side
    tol_f, tol_b = sphere_tol(tab, R, tf) + widen, sphere_tol(tab, R, tb) + widen
    lo = tmin[:, None]
    met = tab.s2 >= -graze
    decided = tab.s2 > graze
    front, back = decided & (tf > lo + tol_f), decided & (tf < lo - tol_f)
    t = np.where(front, tf, np.where(back, tb, tab.proj))
    tol = np.where(front, tol_f, np.where(back, tol_b, tab.td + np.maximum(tol_f, tol_b)))
    clear = front | back
    ri, si = np.nonzero(met)
    ent = np.asarray([spheres[k][0] for k in si], dtype=np.int64)
    return [ri, ent, np.zeros(len(ri), dtype=np.int64), t[ri, si], tol[ri, si], clear[ri, si]], (met & ~clear).any(1)


# ---- quadrics --------------------------------------------------------------------------------------------------------------------------------
class QuadricTable:
    """Per ray, for one held quadric, float64 (the exact values rounded once where the exact stage ran): entry (T0), exit, their error bounds, a, b, c, disc at
    P = L0 + T0 ld and the FIRST-ORDER error bounds da, db, dc, ddisc (ddisc_p: its propagated part), the world box's interval w0, w1 and g = |M ld|."""
    FIELDS = "entry exit dentry dexit a b c disc da db dc ddisc ddisc_p w0 w1 mw g ok".split()

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _exact_quadric(o, d, Q):
    """entry, exit, a, b, c, disc as Fractions (None, ... when some ld_k is zero: the slab test is then the caller's)."""
    fr = lambda x: [Fraction(float(v)) for v in x]                # noqa: E731
    o, d, inv, p, lo, hi = fr(o), fr(d), fr(Q.inv), fr(Q.p), fr(Q.lo), fr(Q.hi)
    L0 = [inv[4 * k] * o[0] + inv[4 * k + 1] * o[1] + inv[4 * k + 2] * o[2] + inv[4 * k + 3] for k in range(3)]
    ld = [inv[4 * k] * d[0] + inv[4 * k + 1] * d[1] + inv[4 * k + 2] * d[2] for k in range(3)]
    if any(v == 0 for v in ld):
        return None
    va, vb = [(lo[k] - L0[k]) / ld[k] for k in range(3)], [(hi[k] - L0[k]) / ld[k] for k in range(3)]
    entry = max(Fraction(PR_EPSILON), max(min(x, y) for x, y in zip(va, vb)))
    ext = min(max(x, y) for x, y in zip(va, vb))
    P = [L0[k] + ld[k] * entry for k in range(3)]
    a, b, c = coefficients(p, P, ld)
    return entry, ext, a, b, c, b * b - 4 * a * c


class Err:
    """A float64 value with a first-order bound on the error its fp32 evaluation carries: running error analysis, one rounding u |result| per operation, none
    where the operation is exact in binary floating point whatever its operands' size: a sum with an exact zero, a product with an exact zero or power of two."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v, self.e = np.asarray(v, dtype=np.float64), np.asarray(e, dtype=np.float64)

    @staticmethod
    def of(x):
        return x if isinstance(x, Err) else Err(x)

    def _free(self):
        return (self.e == 0) & (np.abs(np.frexp(self.v)[0]) == 0.5) | self._zero()

    def _zero(self):
        return (self.e == 0) & (self.v == 0)

    def __mul__(self, y):
        y = Err.of(y)
        v = self.v * y.v
        return Err(v, np.abs(self.v) * y.e + np.abs(y.v) * self.e + np.where(self._free() | y._free(), 0.0, U * np.abs(v)))

    __rmul__ = __mul__

    def __add__(self, y):
        y = Err.of(y)
        v = self.v + y.v
        return Err(v, self.e + y.e + np.where(self._zero() | y._zero(), 0.0, U * np.abs(v)))

    __radd__ = __add__

    def __neg__(self):
        return Err(-self.v, self.e)

    def __sub__(self, y):
        return self + (-Err.of(y))

    def __rsub__(self, y):
        return Err.of(y) + (-self)

    def inverse(self):
        v = 1.0 / self.v
        return Err(v, np.abs(v) * self.e / np.abs(self.v) + U * np.abs(v))


def _device_coefficients(p, o, d):
    """a, b, c in quadric_roots' order of operations (device/pr_device.h), for Err operands."""
    A, B, C, Dq, E, Fq, G, H, I, J = p
    ox, oy, oz = o
    dx, dy, dz = d
    a = ((((A * dx * dx + B * dy * dy) + C * dz * dz) + Dq * dx * dy) + E * dx * dz) + Fq * dy * dz
    b = ((((((((2.0 * A * ox * dx + 2.0 * B * oy * dy) + 2.0 * C * oz * dz) + Dq * (ox * dy + oy * dx)) + E * (ox * dz + oz * dx)) + Fq * (oy * dz + oz * dy)) + G * dx) + H * dy) + I * dz)
    c = ((((((((A * ox * ox + B * oy * oy) + C * oz * oz) + Dq * ox * oy) + E * ox * oz) + Fq * oy * oz) + G * ox) + H * oy) + I * oz) + J
    return a, b, c


def classify_quadric(org, direction, Q, force_exact=False, extra_ulps=0.0):
    """extra_ulps: the caller knows each component of d only up to extra_ulps u |d| (the camera's rays): an input error that the running analysis carries into
    every bound, the slab values' included."""
    o, d = X._as64(org, (-1, 3)), X._as64(direction, (-1, 3))
    n = len(o)
    inv = Q.inv.astype(np.float64).reshape(3, 4)
    p = [Err(np.full(n, float(v))) for v in Q.p]
    lo, hi, M = Q.lo.astype(np.float64), Q.hi.astype(np.float64), Q.m.astype(np.float64).reshape(3, 4)[:, :3]
    ar = np.arange(n)
    with np.errstate(all="ignore"):
        dlen = np.linalg.norm(d, axis=1)
        col = lambda x, k: Err(x[:, k], extra_ulps * U * dlen if x is d else 0.0)               # noqa: E731
        row = lambda k, j: Err(np.full(n, inv[k, j]))                                           # noqa: E731
        L0 = [((row(k, 0) * col(o, 0) + row(k, 1) * col(o, 1)) + row(k, 2) * col(o, 2)) + row(k, 3) for k in range(3)]
        ld = [(row(k, 0) * col(d, 0) + row(k, 1) * col(d, 1)) + row(k, 2) * col(d, 2) for k in range(3)]
        va, vb = [ld[k].inverse() * (Err(np.full(n, lo[k])) - L0[k]) for k in range(3)], [ld[k].inverse() * (Err(np.full(n, hi[k])) - L0[k]) for k in range(3)]
        va_v, vb_v, va_e, vb_e = (np.stack([x.v for x in va], 1), np.stack([x.v for x in vb], 1), np.stack([x.e for x in va], 1), np.stack([x.e for x in vb], 1))
        near, far = np.minimum(va_v, vb_v), np.maximum(va_v, vb_v)
        dnear, dfar = np.where(va_v <= vb_v, va_e, vb_e), np.where(va_v <= vb_v, vb_e, va_e)
        kn, kf = np.argmax(near, 1), np.argmin(far, 1)
        entry, ext = near[ar, kn], far[ar, kf]
        dentry, dexit = np.where(entry > PR_EPSILON, dnear[ar, kn], 0.0), dfar[ar, kf]
        entry = np.maximum(entry, PR_EPSILON)
        # (the error of entry ITSELF is not P's: it moves P along ld and the root by the opposite amount)
        P = [L0[k] + ld[k] * Err(entry) for k in range(3)]
        a, b, c = _device_coefficients(p, P, ld)
        (a, da), (b, db), (c, dc) = (a.v, a.e), (b.v, b.e), (c.v, c.e)
        Sa, _, Sc = coefficients(np.abs(Q.p.astype(np.float64)), [np.abs(x.v) for x in P], [np.abs(x.v) for x in ld])
        disc = b * b - 4.0 * a * c
        ddisc_p = 2.0 * np.abs(b) * db + 4.0 * (np.abs(a) * dc + np.abs(c) * da)
        ddisc = U * (b * b + 4.0 * np.abs(a * c) + np.abs(disc)) + ddisc_p
        # the world box's interval along the ray (float64; its own fp32 evaluation: a difference and a quotient per value)
        wa, wb = (Q.wlo.astype(np.float64) - o) / d, (Q.whi.astype(np.float64) - o) / d
        inside = (o >= Q.wlo) & (o <= Q.whi)
        wa, wb = np.where(d == 0, np.where(inside, -np.inf, np.inf), wa), np.where(d == 0, np.where(inside, np.inf, -np.inf), wb)
        w0, w1 = np.minimum(wa, wb).max(1), np.maximum(wa, wb).min(1)
        mw = 4.0 * U * np.maximum(np.abs(np.where(np.isfinite(wa), wa, 0.0)), np.abs(np.where(np.isfinite(wb), wb, 0.0))).max(1)
        ldv = np.stack([x.v for x in ld], 1)
        g = np.linalg.norm(ldv @ M.T, axis=1)
        ok = (ldv != 0).all(1) & np.isfinite(entry) & np.isfinite(ext)
        root = np.sqrt(np.maximum(disc, 0.0))
        s_any = (np.abs(b) + root) / np.abs(2.0 * a)
        todo = ok & ((np.abs(disc) <= 2.0 ** -30 * (b * b + 4.0 * np.abs(a * c))) | (np.abs(np.abs(a) - PR_EPSILON) <= 2.0 ** -30 * np.maximum(Sa, PR_EPSILON))
                     | (np.abs(c) <= 2.0 ** -30 * Sc) | (np.abs(entry + s_any - ext) <= 2.0 ** -30 * np.abs(ext)) | force_exact)
    idx = np.nonzero(todo)[0]
    for i in idx:
        e = _exact_quadric(o[i], d[i], Q)
        if e is None:
            ok[i] = False
            continue
        entry[i], ext[i], a[i], b[i], c[i] = (float(v) for v in e[:5])
        disc[i] = float(e[5])
        if disc[i] == 0.0 and e[5] != 0:
            disc[i] = math.copysign(np.finfo(np.float64).tiny, e[5])
    return QuadricTable(entry=entry, exit=ext, dentry=dentry, dexit=dexit, a=a, b=b, c=c, disc=disc, da=da, db=db, dc=dc, ddisc=ddisc, ddisc_p=ddisc_p,
                        w0=w0, w1=w1, mw=mw, g=g, ok=ok, n_exact=len(idx))


def quadric_decide(tab):
    """From the table: per ray `linear` (+1 surely, -1 surely not, 0 undecided), the two roots s1, s2 (nan where there is none or the branch is linear), the
    linear root, their tolerances, and `real` (+1 disc surely > 0, -1 surely < 0, 0 grazing)."""
    a, b, c, disc = tab.a, tab.b, tab.c, tab.disc
    with np.errstate(all="ignore"):
        linear = np.where(np.abs(a) < PR_EPSILON - 2.0 * tab.da, 1, np.where(np.abs(a) > PR_EPSILON + 2.0 * tab.da, -1, 0))
        real = np.where(disc > 2.0 * tab.ddisc, 1, np.where(disc < -2.0 * tab.ddisc, -1, 0))
        root = np.sqrt(np.maximum(disc, 0.0))
        q = -0.5 * (b + np.where(b >= 0, root, -root))            # the stable pair: q / a and c / q
        ra, rb = q / a, c / q
        s1, s2 = np.where(b >= 0, ra, rb), np.where(b >= 0, rb, ra)   # s1 = (-b - root) / 2a, s2 = (-b + root) / 2a

        def tol(s, num):
            cancel = U * ((b * b + 4.0 * np.abs(a * c) + np.abs(disc)) / (2.0 * root) + root + np.abs(num)) / np.abs(2.0 * a) + U * np.abs(s)
            implicit = (s * s * tab.da + np.abs(s) * tab.db + tab.dc) / root
            formula = (tab.db + np.minimum(tab.ddisc_p / (2.0 * root), np.sqrt(tab.ddisc_p))) / np.abs(2.0 * a) + np.abs(s) * tab.da / np.abs(a)
            return 2.0 * (np.fmin(implicit, formula) + cancel)
        tol1, tol2 = tol(s1, -b - root), tol(s2, -b + root)
        sl = -c / b
        tol_l = 2.0 * ((tab.dc + np.abs(sl) * tab.db) / np.abs(b) + U * np.abs(sl))
    return linear, real, s1, tol1, s2, tol2, sl, tol_l


def quadric32(o, d, Q, tmin, tmax, any_hit=False):
    """quadric_hit of device/pr_device.h restated in numpy float32, row-wise (for checking the margins on the CPU, not a reference): accepted, t, and the
    intermediate (a, entry) for the tests' own bookkeeping."""
    o, d = np.asarray(o, dtype=F), np.asarray(d, dtype=F)
    n = len(o)
    tmin, tmax = np.broadcast_to(np.asarray(tmin, dtype=F), (n,)), np.broadcast_to(np.asarray(tmax, dtype=F), (n,))
    i, p, m = Q.inv, Q.p, Q.m
    with np.errstate(all="ignore"):
        t0, t1 = tmin.copy(), tmax.copy()
        cull = np.zeros(n, dtype=bool)
        for k in range(3):
            z = d[:, k] == 0
            cull |= z & ((o[:, k] < Q.wlo[k]) | (o[:, k] > Q.whi[k]))
            wa, wb = (Q.wlo[k] - o[:, k]) / d[:, k], (Q.whi[k] - o[:, k]) / d[:, k]
            t0, t1 = np.where(z, t0, np.fmax(t0, np.fmin(wa, wb))), np.where(z, t1, np.fmin(t1, np.fmax(wa, wb)))
        cull |= ~(t0 <= t1)
        L = [((i[4 * k] * o[:, 0] + i[4 * k + 1] * o[:, 1]) + i[4 * k + 2] * o[:, 2]) + i[4 * k + 3] for k in range(3)]
        ld = [(i[4 * k] * d[:, 0] + i[4 * k + 1] * d[:, 1]) + i[4 * k + 2] * d[:, 2] for k in range(3)]
        smin, smax = lambda x, y: np.where(y < x, y, x), lambda x, y: np.where(x < y, y, x)      # noqa: E731   std::min / std::max
        entry = ext = None
        for k in range(3):
            ik = F(1) / ld[k]
            va, vb = ik * (Q.lo[k] - L[k]), ik * (Q.hi[k] - L[k])
            entry = smin(va, vb) if entry is None else smax(smin(va, vb), entry)
            ext = smax(va, vb) if ext is None else smin(smax(va, vb), ext)
        entry = smax(np.full(n, F(1.1920929e-07)), entry)
        entry = np.where(entry < 0, F(0), entry)
        ox, oy, oz = (L[k] + ld[k] * entry for k in range(3))
        dx, dy, dz = ld
        A, B, C, Dq, E, Fq, G, H, I, J = p
        two, four = F(2), F(4)
        a = ((((A * dx * dx + B * dy * dy) + C * dz * dz) + Dq * dx * dy) + E * dx * dz) + Fq * dy * dz
        b = ((((((((two * A * ox * dx + two * B * oy * dy) + two * C * oz * dz) + Dq * (ox * dy + oy * dx)) + E * (ox * dz + oz * dx)) + Fq * (oy * dz + oz * dy)) + G * dx) + H * dy) + I * dz)
        c = ((((((((A * ox * ox + B * oy * oy) + C * oz * oz) + Dq * ox * oy) + E * ox * oz) + Fq * oy * oz) + G * ox) + H * oy) + I * oz) + J
        disc = b * b - four * a * c
        root = np.sqrt(disc)
        qu1, qu2 = (-b - root) / (two * a), (-b + root) / (two * a)
        qu = np.where(qu1 <= F(1e-6), qu2, qu1)
        t = np.where(np.abs(a) <= F(1.1920929e-07), -c / b, np.where(disc < 0, F(np.inf), qu))
        ok = ~cull & (t < np.inf) & (t >= F(1e-6))
        if any_hit:
            return ok, t, a, entry
        t = t + entry
        ok &= ~(t > ext)
        w = [(m[4 * k] * (dx * t) + m[4 * k + 1] * (dy * t)) + m[4 * k + 2] * (dz * t) for k in range(3)]
        gt = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
        ok &= (gt >= tmin) & (gt <= tmax)
    assert t.dtype == F and a.dtype == F
    return ok, t, a, entry


def _pick(tab):
    """The closest-hit rule on a table: (T, tol_T, state) with state +1 the surface MUST be reported at T (window apart), 0 undecided, -1 MUST NOT."""
    linear, real, s1, tol1, s2, tol2, sl, tol_l = quadric_decide(tab)
    n = len(tab.a)
    with np.errstate(all="ignore"):
        m1, m2, ml = tol1 + 2.0 * tab.dentry, tol2 + 2.0 * tab.dentry, tol_l + 2.0 * tab.dentry
        # quadratic branch: s1 when it is beyond INT_EPS, s2 otherwise
        first, second = s1 > INT_EPS + m1, s1 < INT_EPS - m1
        s_q = np.where(first, s1, s2)
        tol_q = np.where(first, tol1, tol2)
        st_q = np.where(first, 1, np.where(second, np.where(s2 > INT_EPS + m2, 1, np.where(s2 < INT_EPS - m2, -1, 0)), 0))
        # (s1 undecided against INT_EPS: a miss all the same when neither root can be reported)
        st_q = np.where((st_q == 0) & (np.fmax(s1 + m1, s2 + m2) < INT_EPS), -1, st_q)
        st_q = np.where(real > 0, st_q, np.where(real < 0, -1, 0))
        st_l = np.where(sl > INT_EPS + ml, 1, np.where(sl < INT_EPS - ml, -1, 0))
        st_l = np.where(np.isfinite(tol_l), st_l, 0)
        state = np.where(linear > 0, st_l, np.where(linear < 0, st_q, 0))
        s = np.where(linear > 0, sl, s_q)
        tol = np.where(linear > 0, tol_l, tol_q)
        T = s + tab.entry
        tol_T = tol + 2.0 * U * np.abs(T) + (np.abs(tab.g - 1.0) + 10.0 * U) * np.abs(T)
        # the clip at the exit, then the world box
        me = tol_T + 2.0 * tab.dexit
        hit = state > 0
        state = np.where(hit & (T > tab.exit + me), -1, np.where(hit & ~(T < tab.exit - me), 0, state))
        # (an undecided root that lies beyond the exit whichever it is: a miss)
        lowest = np.where(linear > 0, sl - ml, np.where(linear < 0, np.fmin(s1 - m1, s2 - m2), -np.inf))
        state = np.where((state == 0) & (real != 0) & (linear != 0) & (tab.entry + np.fmax(lowest, INT_EPS) > tab.exit + 2.0 * tab.dexit + 4.0 * U * np.abs(tab.exit)), -1, state)
        hit = state > 0
        state = np.where(hit & ~((T >= tab.w0 + tab.mw) & (T <= tab.w1 - tab.mw)), 0, state)
        state = np.where(tab.ok & (np.isfinite(tol_T) | (state < 0)), state, np.where(tab.ok, np.minimum(state, 0), 0))
        # a ray that surely passes beside the local box (s >= INT_EPS > 0 puts T beyond an exit that lies before the entry), or beside the world box: a miss
        state = np.where(tab.ok & (tab.entry - 2.0 * tab.dentry > tab.exit + 2.0 * tab.dexit), -1, state)
        state = np.where(tab.w0 - tab.mw > tab.w1 + tab.mw, -1, state)
    assert state.shape == (n,)
    return T, np.where(state > 0, tol_T, np.inf), state


def _occlusion(tab, tmin, tmax):
    """The occlusion rule: state +1 MUST be reported occluded, 0 undecided, -1 MUST NOT."""
    linear, real, s1, tol1, s2, tol2, sl, tol_l = quadric_decide(tab)
    with np.errstate(all="ignore"):
        big = np.where(tab.a > 0, s2, s1)
        mb = np.where(tab.a > 0, tol2, tol1) + 2.0 * tab.dentry
        st_q = np.where(big > INT_EPS + mb, 1, np.where(big < INT_EPS - mb, -1, 0))
        st_q = np.where(real > 0, st_q, np.where(real < 0, -1, 0))
        ml = tol_l + 2.0 * tab.dentry
        st_l = np.where(np.isfinite(tol_l), np.where(sl > INT_EPS + ml, 1, np.where(sl < INT_EPS - ml, -1, 0)), 0)
        state = np.where(linear > 0, st_l, np.where(linear < 0, st_q, 0))
        state = np.where(tab.ok, state, 0)
        lo, hi = np.maximum(tmin, tab.w0), np.minimum(tmax, tab.w1)
        over = np.where(lo + tab.mw <= hi - tab.mw, 1, np.where(lo - tab.mw > hi + tab.mw, -1, 0))
    return np.where((state < 0) | (over < 0), -1, np.where((state > 0) & (over > 0), 1, 0))


def _quadric_rows(o, d, quadrics, tmin, tmax, any_hit, extra_ulps=0.0, tables=None):
    """Rows of the quadrics [(entity, HeldQuadric)].  Closest: t = T, the window is the rules'.  Occlusion: the answer does not depend on where in the window the
    root lies, so the row stands AT the window's start (t = tmin + tol, tol = the world box's margin): sure and possible there, or absent."""
    n = len(o)
    rows, undecided = [[] for _ in range(6)], np.zeros(n, dtype=bool)
    for ent, Q in quadrics:
        tab = tables[ent] if tables is not None and ent in tables else classify_quadric(o, d, Q, extra_ulps=extra_ulps)
        if tables is not None:
            tables[ent] = tab
        if any_hit:
            state = _occlusion(tab, tmin, tmax)
            tol = tab.mw + 2.0 * U * np.abs(tmin)
            T = tmin + tol
        else:
            T, tol, state = _pick(tab)
        keep = np.nonzero(state >= 0)[0]
        undecided[state == 0] = True
        for k, v in enumerate((keep, np.full(len(keep), ent, dtype=np.int64), np.zeros(len(keep), dtype=np.int64), T[keep], tol[keep], state[keep] > 0)):
            rows[k].append(v)
    if not quadrics:
        return [np.zeros(0, dtype=np.int64)] * 3 + [np.zeros(0)] * 2 + [np.zeros(0, dtype=bool)], undecided
    return [np.concatenate(r) for r in rows], undecided


# ---- candidates ------------------------------------------------------------------------------------------------------------------------------
def candidates(org, direction, spheres=(), quadrics=(), tris=None, tri_entity=None, tri_prim=None, tmin=1e-4, tmax=np.inf, any_hit=False, extra_ulps=0.0):
    """exact_disk.Candidates for a scene of spheres [(entity, centre, radius)], quadrics [(entity, HeldQuadric)] and world-space triangles of untransformed
    meshes (through X.Geometry / X.classify, as exact_disk.candidates does).  tmin (scalar or per ray) chooses a sphere's root; any_hit: the rows of the quadrics
    follow the occlusion callback for the window (tmin, tmax], tmax = distance - 0.001 as the caller of check_any states it.  extra_ulps: as exact_disk's, for
    spheres and triangles; for the quadrics it is an input error of d that the running error analysis carries into every bound (classify_quadric)."""
    o, d = X._as64(org, (-1, 3)), X._as64(direction, (-1, 3))
    n = len(o)
    tmin = np.broadcast_to(np.asarray(tmin, dtype=np.float64), (n,))
    tmax = np.broadcast_to(np.asarray(tmax, dtype=np.float64), (n,))
    srows, s_und = _sphere_rows(o, d, list(spheres), tmin, extra_ulps)
    qrows, q_und = _quadric_rows(o, d, list(quadrics), tmin, tmax, any_hit, extra_ulps)
    parts = [srows, qrows]
    if tris is not None and len(tris):
        c = D.candidates(org, direction, [], tris, tri_entity, tri_prim, extra_ulps=extra_ulps)
        parts.append([c.ray, c.entity, c.prim, c.t, c.tol, c.clear])
    return D.Candidates(n, *(np.concatenate([p[k] for p in parts]) for k in range(6)), s_und | q_und)
