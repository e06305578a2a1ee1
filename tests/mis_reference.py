"""A float64 model of one vertex of the `direct` integrator -- next event estimation plus one bounce that may find the light, combined by multiple importance
sampling -- for materials that are trees of blend / add over Lambert, Oren-Nayar, null and mirror leaves (TEST INFRASTRUCTURE ONLY: plain numpy, no product
import, no checker).  It restates the rules of the reference's direct.cpp, blend.cpp, add.cpp, orennayar.cpp, environment.cpp and mesh.cpp in words of its own:

  path pdf      after a bounce the path pdf is (pdf the material's `sample` reports) x (roulette probability of the vertex); the weight `sample` reports multiplies
                the throughput and is NOT divided by the roulette probability.
  light sample  contribution = radiance x (weight of `eval`) / p_light, times  t(p_light) / (t(p_light) + t(p_eval x roulette)), with t the identity (`balance`) or
                the square (`power`).  The roulette probability here is the path length's, whether or not the material is delta-only.
  bounce        a bounce that finds a light counts its radiance times  t(path pdf) / (t(path pdf) + t(p_light of that direction)); after a delta bounce the radiance
                counts in full.
  mono          (one wavelength per sample) the weights are formed over four lanes of which three are masked: the light sample of a non-delta light becomes NaN and is
                dropped (its pixel gets the NaN feedback bit), the bounce keeps a quarter: both sums of the denominator run over four lanes, the numerator over one.
  blend         f = the factor clamped to [0, 1].  eval: weight and pdf are (1 - f) x1 + f x2; when one child is delta-only the other child's weight AND pdf are scaled
                by that child's probability.  sample: one number picks child 1 with probability 1 - f; weight and pdf are scaled by the probability of the child picked.
  add           eval: weight w1 + w2, pdf (p1 + p2) / 2; when one child is delta-only the other's pdf is halved and its weight kept.  sample: one number picks a child
                with probability 1/2; the pdf is halved, the weight kept.
  nesting       both rules call themselves on a child that is a blend / add, so the factors compound from the root down; a blend / add is delta-only when both children are.
  Lambert       eval weight a cos / pi, pdf cos / pi; sample: cosine hemisphere on the viewer's side, weight a.
  Oren-Nayar    eval weight a (A + B s / t) cos / pi with cos = max(0, N.L), pdf cos / pi; sample: cosine hemisphere around +N (not flipped), weight a (A + B s / t).
  null, mirror  delta-only: sample passes the ray straight on resp. mirrors it about N, weight 1, pdf 1.
  environment   a constant environment draws its light samples from the cosine hemisphere around its +z ONLY, but claims |z| / pi for every direction.
  mesh light    a point uniform on a face picked uniformly; claimed area pdf 1 / (faces x area of that face).  For the rectangle of two equal triangles used here that is
                the uniform distribution and its true density 1 / A; as a solid angle p = d^2 / (A cos').  A bounce that meets it is charged 1 / (world area), the same.

Everything is written recursively over the Python tree; nothing here knows the flattened leaf table of the library.

A material is  ("lambert", a) | ("oren", a, sigma) | "null" | "mirror" | ("blend", m1, m2, f) | ("add", m1, m2).  The shading frame is the world frame: N = +z.

Rule switches (keywords, off by default; each is a plausible WRONG rule, there to prove that a test can tell it from the right one):
  sample_pdf_unscaled   (a)  `sample` of a blend / add reports the leaf's pdf without the selection probabilities
  blend_weight_unscaled (b1) `sample` of a blend does not scale the weight          add_weight_halved (b2) `sample` of an add halves the weight
  innermost_only        (c)  the pdf `sample` reports carries the innermost level's selection probability only
  one_sided_pdf_unscaled(d)  `eval` of a form with a delta-only child leaves the other child's pdf as it is
  add_pdf_not_halved    (e)  `eval` of an add of two children reports p1 + p2
  no_clamp              (f)  the factor is used as given"""
import numpy as np

F = np.float32
EPS = 1.1920929e-07
SWITCHES = ("sample_pdf_unscaled", "blend_weight_unscaled", "add_weight_halved", "innermost_only", "one_sided_pdf_unscaled", "add_pdf_not_halved", "no_clamp")


def _sw(sw):
    assert all(k in SWITCHES for k in sw), sw
    return sw


def kind(tree):
    return tree if isinstance(tree, str) else tree[0]


def delta_only(tree):
    k = kind(tree)
    if k in ("null", "mirror"):
        return True
    if k in ("blend", "add"):
        return delta_only(tree[1]) and delta_only(tree[2])
    return False


def factor(tree, **sw):
    """the blend factor as the scene holds it (fp32), clamped"""
    f = float(F(tree[3]))
    return f if sw.get("no_clamp") else min(1.0, max(0.0, f))


def oren_nayar_term(a, sigma, V, L):
    """a (A + B s / t) for unit V and L [..., 3] in the frame of N = +z; the albedo alone when sigma^2 is not above epsilon"""
    r2 = float(F(sigma)) ** 2
    L = np.asarray(L, dtype=np.float64)
    if not r2 > EPS:
        return np.full(L.shape[:-1], float(a))
    ndl, ndv = np.maximum(0.0, L[..., 2]), V[2]
    s = -ndl * ndv + L @ V
    t = np.where(s < EPS, 1.0, np.maximum(ndl, ndv))
    A = 1 - 0.5 * r2 / (r2 + 0.33) + 0.17 * a * r2 / (r2 + 0.13)
    B = 0.45 * r2 / (r2 + 0.09)
    return a * (A + B * s / t)


# ---- eval ------------------------------------------------------------------------------------------------------------------------------------------
def eval(tree, V, L, **sw):   # noqa: A001 (the reference's name)
    """(weight, pdf, delta-only) of the material for the viewer V and the light directions L [..., 3]; weight includes the cosine"""
    _sw(sw)
    L = np.asarray(L, dtype=np.float64)
    k = kind(tree)
    zero = np.zeros(L.shape[:-1])
    if k in ("null", "mirror"):
        return zero, zero, True
    if k == "lambert":      # two-sided, and the viewer is above: the light must be too
        c = np.maximum(0.0, L[..., 2]) / np.pi
        return float(tree[1]) * c, c, False
    if k == "oren":
        c = np.maximum(0.0, L[..., 2]) / np.pi
        return oren_nayar_term(float(tree[1]), tree[2], V, L) * c, c, False
    d1, d2 = delta_only(tree[1]), delta_only(tree[2])
    if d1 and d2:
        return zero, zero, True
    if k == "blend":
        f = factor(tree, **sw)
        if d1 or d2:
            w, p, d = eval(tree[2] if d1 else tree[1], V, L, **sw)
            q = f if d1 else 1 - f
            return w * q, (p if sw.get("one_sided_pdf_unscaled") else p * q), d
        (w1, p1, _), (w2, p2, _) = eval(tree[1], V, L, **sw), eval(tree[2], V, L, **sw)
        return (1 - f) * w1 + f * w2, (1 - f) * p1 + f * p2, False
    assert k == "add", tree
    if d1 or d2:
        w, p, d = eval(tree[2] if d1 else tree[1], V, L, **sw)
        return w, (p if sw.get("one_sided_pdf_unscaled") else 0.5 * p), d
    (w1, p1, _), (w2, p2, _) = eval(tree[1], V, L, **sw), eval(tree[2], V, L, **sw)
    return w1 + w2, (p1 + p2 if sw.get("add_pdf_not_halved") else 0.5 * (p1 + p2)), False


# ---- sample ----------------------------------------------------------------------------------------------------------------------------------------
def descend(tree, **sw):
    """[(leaf, probability that `sample` ends in it, factor on the pdf it reports, factor on the weight it reports)], leaves in tree order.  Under the right
    rules the first two factors are the same number."""
    _sw(sw)
    k = kind(tree)
    if k not in ("blend", "add"):
        return [(tree, 1.0, 1.0, 1.0)]
    out = []
    for child, side in ((tree[1], 0), (tree[2], 1)):
        if k == "blend":
            f = factor(tree, **sw)
            sel = f if side else 1 - f
            prob = min(1.0, max(0.0, sel))              # (a number below an unclamped 1 - f is a probability all the same)
            wf = 1.0 if sw.get("blend_weight_unscaled") else sel
        else:
            sel = prob = 0.5
            wf = 0.5 if sw.get("add_weight_halved") else 1.0
        for leaf, p, s, m in descend(child, **sw):
            inner = kind(child) in ("blend", "add")
            scale = 1.0 if sw.get("sample_pdf_unscaled") else (s if (sw.get("innermost_only") and inner) else sel * s)
            out.append((leaf, prob * p, scale, wf * m))
    return out


def leaves(tree, **sw):
    """[(leaf, selection product s_i, weight product m_i)] of `sample`, under the right rules"""
    return [(leaf, s, m) for leaf, _, s, m in descend(tree, **sw)]


# ---- the integrator's constants -------------------------------------------------------------------------------------------------------------------------
def rr_probability(path_length, soft_depth, factor_=0.9):
    """the roulette probability of a vertex: 1 below the soft depth (and for path length 0), then 0.9^(length - soft depth), 0 once that is at most 1e-4"""
    if path_length == 0 or path_length < soft_depth:
        return 1.0
    p = float(F(min(1.0, float(F(factor_)) ** (path_length - soft_depth))))
    return 0.0 if p <= 1e-4 else p


def mis_term(x, mis):
    assert mis in ("balance", "power")
    return x * x if mis == "power" else x


# ---- lights: quadrature nodes ---------------------------------------------------------------------------------------------------------------------------
def _midpoints(n):
    return (np.arange(n) + 0.5) / n


def _gauss(n):
    x, w = np.polynomial.legendre.leggauss(n)
    return 0.5 * (x + 1.0), 0.5 * w


def _cos_hemisphere(n):
    """directions of the cosine-weighted upper hemisphere (midpoints in cos^2 and the azimuth) and their probabilities"""
    U, P = np.meshgrid(_midpoints(n), 2 * np.pi * _midpoints(2 * n), indexing="ij")
    ct, st = np.sqrt(U), np.sqrt(1 - U)
    L = np.stack([st * np.cos(P), st * np.sin(P), ct], -1).reshape(-1, 3)
    return L, np.full(len(L), 1.0 / len(L))


class ConstantEnvironment:
    """unit radiance from every direction; samples its +z hemisphere only and claims |z| / pi everywhere.  The floor's normal is its +z."""
    exact = True                # every node carries the same value for Lambert leaves seen head-on

    def light_samples(self, point, n):
        """(L, probability of the node, claimed solid-angle pdf, radiance)"""
        L, w = _cos_hemisphere(n)
        return L, w, np.abs(L[:, 2]) / np.pi, np.ones(len(L))

    def bounce_nodes(self, point, n):
        """the cosine hemisphere around N as (L, probability, claimed light pdf of L, radiance met along L)"""
        L, w = _cos_hemisphere(n)
        return L, w, np.abs(L[:, 2]) / np.pi, np.ones(len(L))

    def along(self, point, direction):
        """radiance a delta bounce meets"""
        return 1.0


class QuadLight:
    """a rectangle [-hx, hx] x [-hy, hy] at height h that faces down, unit radiance, black; nothing else is lit"""
    exact = False

    def __init__(self, hx, hy, h):
        self.hx, self.hy, self.h = float(hx), float(hy), float(h)
        self.area = 4.0 * self.hx * self.hy

    def _nodes(self, point, n):
        g, w = _gauss(n)
        X, Y = np.meshgrid(self.hx * (2 * g - 1), self.hy * (2 * g - 1), indexing="ij")
        W = (w[:, None] * w[None, :]).reshape(-1)
        d = np.stack([X.reshape(-1) - point[0], Y.reshape(-1) - point[1], np.full(X.size, self.h)], -1)
        d2 = (d * d).sum(-1)
        L = d / np.sqrt(d2)[:, None]
        return L, W, d2

    def light_samples(self, point, n):
        L, W, d2 = self._nodes(point, n)
        return L, W, d2 / (self.area * L[:, 2]), np.ones(len(L))

    def bounce_nodes(self, point, n):
        """directions that meet the rectangle, with the probability the cosine hemisphere gives their node: cos cos' / (pi d^2) dA; the rest of the hemisphere
        meets nothing and is left out (its value is 0)"""
        L, W, d2 = self._nodes(point, n)
        return L, W * self.area * L[:, 2] * L[:, 2] / (np.pi * d2), d2 / (self.area * L[:, 2]), np.ones(len(L))

    def along(self, point, direction):
        if not direction[2] > 0:
            return 0.0
        t = self.h / direction[2]
        return 1.0 if abs(point[0] + t * direction[0]) < self.hx and abs(point[1] + t * direction[1]) < self.hy else 0.0


# ---- the estimator ------------------------------------------------------------------------------------------------------------------------------------
def _leaf_sample(leaf, V, L):
    """(integral weight, pdf) the leaf's `sample` reports for the cosine-hemisphere direction L"""
    c = np.maximum(0.0, L[..., 2]) / np.pi
    if kind(leaf) == "lambert":
        return np.full(L.shape[:-1], float(leaf[1])), c
    assert kind(leaf) == "oren", leaf
    return oren_nayar_term(float(leaf[1]), leaf[2], V, L), c


def _delta_direction(leaf, V):
    return -V if leaf == "null" else np.asarray([-V[0], -V[1], V[2]])


def strategies(tree, light, point, V, mis="balance", rr=1.0, mono=False, n=32, **sw):
    """One sample of each strategy at the floor point `point` seen from V, as lists of (value, probability): the light sample's and the bounce's.  Probabilities
    that do not add up to 1 leave the rest at value 0.  In mono the light sample is dropped (value 0; flagged NaN by the integrator)."""
    V = np.asarray(V, dtype=np.float64)
    point = np.asarray(point, dtype=np.float64)
    quarter = 0.25 if mono else 1.0
    light_values = (np.zeros(0), np.zeros(0))
    if not delta_only(tree) and not mono:
        L, w, pl, le = light.light_samples(point, n)
        wt, p, d = eval(tree, V, L, **sw)
        ok = (p > 0) & (pl > 0) & (not d)
        with np.errstate(all="ignore"):
            x = np.where(ok, le * wt / pl * mis_term(pl, mis) / (mis_term(pl, mis) + mis_term(p * rr, mis)), 0.0)
        light_values = (x, w)
    survive = 1.0 if delta_only(tree) else rr            # a delta-only material is never ended by the roulette
    vals, probs = [], []
    for leaf, prob, scale, m in descend(tree, **sw):
        if prob <= 0:
            continue
        if kind(leaf) in ("null", "mirror"):
            vals.append(np.asarray([m * light.along(point, _delta_direction(leaf, V))]))
            probs.append(np.asarray([survive * prob]))
            continue
        L, w, pl, le = light.bounce_nodes(point, n)
        iw, p = _leaf_sample(leaf, V, L)
        path = p * scale * survive
        with np.errstate(all="ignore"):
            x = np.where(path > 0, m * iw * le * quarter * mis_term(path, mis) / (mis_term(path, mis) + mis_term(pl, mis)), 0.0)
        vals.append(x)
        probs.append(survive * prob * w)
    return light_values, (np.concatenate(vals), np.concatenate(probs))


def moments(tree, light, point, V, **kw):
    """dict(light=(E X, E X^2), bounce=(E X, E X^2), sample=(E, E of the square) of their sum: the two are drawn independently)"""
    (xl, wl), (xb, wb) = strategies(tree, light, point, V, **kw)
    l1, l2, b1, b2 = float((xl * wl).sum()), float((xl * xl * wl).sum()), float((xb * wb).sum()), float((xb * xb * wb).sum())
    return dict(light=(l1, l2), bounce=(b1, b2), sample=(l1 + b1, l2 + b2 + 2 * l1 * b1))


def _distinct(x, w):
    """the distinct values of x (to 1e-12 relative) with their total probabilities, zero-probability entries dropped"""
    out = []
    for v, p in sorted(zip(x.tolist(), w.tolist())):
        if p <= 0:
            continue
        if out and abs(v - out[-1][0]) <= 1e-12 * max(1.0, abs(v)):
            out[-1][1] += p
        else:
            out.append([v, p])
    return [(v, p) for v, p in out]


def exact_values(tree, light, V, **kw):
    """For set-ups in which a sample takes finitely many values (the constant environment, head-on, Lambert and Oren-Nayar leaves): the light sample's value
    (None in mono or for a delta-only tree) and the bounce's [(value, probability)]; a roulette below 1 leaves the remaining probability at value 0."""
    assert light.exact
    (xl, wl), (xb, wb) = strategies(tree, light, (0.0, 0.0, 0.0), V, n=4, **kw)
    nee = _distinct(xl, wl)
    assert len(nee) <= 1, nee
    return (nee[0][0] if nee else None), _distinct(xb, wb)


# ---- block means on a film ---------------------------------------------------------------------------------------------------------------------------
def floor_points(n, extent, px, py, half, tilt=0.0, sub=2):
    """Floor points (z = 0) under `sub` x `sub` midpoints of each pixel of the (2 half + 1)^2 block around pixel (px, py) of an n x n film of an orthographic camera
    of width = height = `extent` that looks at the origin, tilted by `tilt` from the normal in the xz plane.  Pixel p covers film positions [p - 0.5, p + 0.5) / n - 0.5
    (the sample position has half a pixel taken off before it is normalised); a film offset x lies over the floor at x / cos(tilt)."""
    s = (np.arange(sub) + 0.5) / sub - 0.5
    fx = (extent * ((np.arange(px - half, px + half + 1)[:, None] + s[None, :]) / n - 0.5)).reshape(-1) / np.cos(tilt)
    fy = -(extent * ((np.arange(py - half, py + half + 1)[:, None] + s[None, :]) / n - 0.5)).reshape(-1)
    X, Y = np.meshgrid(fx, fy, indexing="ij")
    return np.stack([X.reshape(-1), Y.reshape(-1), np.zeros(X.size)], -1)


def block_moments(tree, light, points, V, n=24, **kw):
    """(E, E of the square) of one sample whose floor point is uniform over `points`"""
    m = np.asarray([moments(tree, light, p, V, n=n, **kw)["sample"] for p in points])
    return float(m[:, 0].mean()), float(m[:, 1].mean())


def block_expectation(tree, light, film, V, tilt=0.0, quick=False, **kw):
    """film = (n, extent, px, py, half).  Returns (expectation of the block mean, second moment of one sample, quadrature error): the error is the difference to
    the same computation at half the step, on the light and within the pixels.  quick: the half-step computation alone, no error (for comparing two rules)."""
    coarse = block_moments(tree, light, floor_points(*film, tilt=tilt, sub=1), V, n=16, **kw)
    if quick:
        return coarse[0], coarse[1], None
    fine = block_moments(tree, light, floor_points(*film, tilt=tilt, sub=2), V, n=32, **kw)
    return fine[0], fine[1], abs(fine[0] - coarse[0])


# ---- the cases of tests/test_gpu_mix_mis.py (kept here so that tests/test_mis_reference.py can weigh them on a machine without a GPU) ------------------
L1, L2, L3 = (("lambert", float(F(x))) for x in (0.8, 0.6, 0.4))
ROUGH = ("oren", float(F(0.7)), 0.5)
MATERIALS = {
    "blend(L1, L2, 0.3)": ("blend", L1, L2, 0.3),
    "blend(L1, L2, 1.7)": ("blend", L1, L2, 1.7),
    "add(L1, L2)": ("add", L1, L2),
    "blend(blend(L1, L2, 0.25), L3, 0.4)": ("blend", ("blend", L1, L2, 0.25), L3, 0.4),
    "add(blend(L1, L2, 0.25), L3)": ("add", ("blend", L1, L2, 0.25), L3),
    "blend(null, L1, 0.4)": ("blend", "null", L1, 0.4),
    "add(mirror, L1)": ("add", "mirror", L1),
    "blend(null, blend(null, L1, 0.5), 0.5)": ("blend", "null", ("blend", "null", L1, 0.5), 0.5),
    "blend(L3, add(L1, oren-nayar), 0.3)": ("blend", L3, ("add", L1, ROUGH), 0.3),
    "oren-nayar at 45 degrees": ROUGH,
}
HEAD_ON = [k for k in MATERIALS if k != "oren-nayar at 45 degrees"]          # the exact tier: a constant environment seen along the normal
MONO_SETUPS = [("balance", 4), ("power", 4), ("balance", 0)]                  # (MIS mode, soft depth): soft depth 0 puts the roulette at 0.9 on the first vertex
HERO_SETUPS = ["balance", "power"]
EXACT_RTOL, EXACT_ATOL = 1e-5, 1e-6

# the statistical tier: the floor [-1, 1]^2 under a 2 x 2 lamp one unit above it, a 40 x 40 film 2 wide (pixel 0.05), 5 x 5 pixel blocks under the lamp's centre and 0.5 beside it
LAMP = (1.0, 1.0, 1.0)
FILM_N, FILM_EXTENT, BLOCK_HALF = 40, 2.0, 2
BLOCKS = ((20, 20), (30, 20))
SPP = 4096
VIEW_45 = float(np.pi / 4)


def view(tilt):
    """the viewer's direction as the scene holds it: fp32 sine and cosine, normalised in float64"""
    v = np.asarray([float(F(np.sin(tilt))), 0.0, float(F(np.cos(tilt)))])
    return v / np.linalg.norm(v)


def tilt_of(name):
    return VIEW_45 if name == "oren-nayar at 45 degrees" else 0.0


HERO_SECOND_MOMENT = 1.25   # E c^2 as the power table takes it, from above: the GPU test and the checker anchor measure their own (1.15 .. 1.16) and assert that it is below this


def statistical_case(tree, tilt, block, hero_second_moment=1.0, **kw):
    """(expectation of the block mean, standard error of the block mean, quadrature error) of the material under the lamp; keywords as strategies() takes them
    (hero mode, `balance`, roulette 1 by default).  hero_second_moment: E c^2 of the factor c (mean 1) by which the wavelengths of a sample scale the Y of a
    constant spectrum; c is independent of the rest.  1 in mono."""
    e, m2, err = block_expectation(tree, QuadLight(*LAMP), (FILM_N, FILM_EXTENT, block[0], block[1], BLOCK_HALF), view(tilt), tilt=tilt, **kw)
    n = (2 * BLOCK_HALF + 1) ** 2 * SPP
    return e, float(np.sqrt(max(hero_second_moment * m2 - e * e, 0.0) / n)), err
