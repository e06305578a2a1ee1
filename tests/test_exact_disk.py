"""tests/exact_disk.py against itself and against closed forms, without a GPU: the exact ray / disk decision on hand-made cases and against its float64
pass, the fp32 restatement of disk_hit inside the margins derived from its operation count, the candidate rules on answers built from the reference
itself, and the radiometric quadratures against their closed forms."""
from fractions import Fraction

import numpy as np
import pytest

import exact_disk as D
import exact_rays as X

F = np.float32


def rays_at(c, e1, e2, nh, r, n, rng, spread=1.0):
    """Rays aimed at points uniform in the square of half side spread * r around c in the disk's plane, from origins at least 0.1 r off it."""
    a, b = rng.uniform(-spread * r, spread * r, (2, n))
    target = c + a[:, None] * e1 + b[:, None] * e2
    off = rng.uniform(-2, 2, (2, n))
    g = rng.uniform(0.1, 3.0, n) * rng.choice([-1.0, 1.0], n)
    org = (target + r * (off[0][:, None] * e1 + off[1][:, None] * e2 + g[:, None] * nh)).astype(F)
    d = target - org
    return org, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)


def test_exact_decisions_on_hand_made_rays():
    c, n, r = F([0, 0, 1]), F([0, 0, 2]), F(1)                                          # (the normal is not a unit vector)
    t, s = D.exact_ray_disk(F([0.5, 0, 3]), F([0, 0, -1]), c, n, r)
    assert (t, s) == (Fraction(2), -1)
    assert D.exact_ray_disk(F([1, 0, 3]), F([0, 0, -1]), c, n, r) == (Fraction(2), 0)     # exactly on the rim
    assert D.exact_ray_disk(F([1, 0, 3]), F([0, 0, -0.5]), c, n, r) == (Fraction(4), 0)
    assert D.exact_ray_disk(np.nextafter(F(1), F(2)) * F([1, 0, 0]) + F([0, 0, 3]), F([0, 0, -1]), c, n, r)[1] == 1   # one ulp outside
    assert D.exact_ray_disk(np.nextafter(F(1), F(0)) * F([1, 0, 0]) + F([0, 0, 3]), F([0, 0, -1]), c, n, r)[1] == -1  # one ulp inside
    assert D.exact_ray_disk(F([0, 0, 3]), F([1, 0, 0]), c, n, r) == (None, 1)              # parallel to the plane
    assert D.exact_ray_disk(F([0, 0, 1]), F([1, 0, 0]), c, n, r) == (None, 1)              # ... and inside it
    t, s = D.exact_ray_disk(F([0, 0, -1]), F([0, 0, -1]), c, n, r)                         # behind the origin: t < 0, the window is the caller's
    assert (t, s) == (Fraction(-2), -1)
    t, s = D.exact_ray_disk(F([-0.3, 0.1, 0]), F([0.6, 0, 0.8]), c, n, r)
    assert t == Fraction(1) / Fraction(float(F(0.8))) and s == -1


def test_the_float64_pass_agrees_with_the_exact_stage():
    rng = np.random.default_rng(5)
    c, n, r = F([0.3, -0.2, 1.1]), F([0.2, -0.4, 1.3]), F(0.8)
    nh = n.astype(np.float64) / np.linalg.norm(n.astype(np.float64))
    e1 = np.cross(nh, [1.0, 0, 0]); e1 /= np.linalg.norm(e1)
    e2 = np.cross(nh, e1)
    org, d = rays_at(c.astype(np.float64), e1, e2, nh, float(r), 400, rng, spread=1.5)
    fast, exact = D.classify(org, d, [c], [n], [r]), D.classify(org, d, [c], [n], [r], force_exact=True)
    assert exact.n_exact == 400 and fast.n_exact < 10
    assert np.array_equal(fast.sign, exact.sign) and np.allclose(fast.t, exact.t, rtol=2.0 ** -45, atol=0)
    assert 0.2 < (exact.sign < 0).mean() < 0.8


def test_the_fp32_statement_sequence_stays_inside_its_margins():
    """disk_hit restated in numpy float32 against the exact table: its decision differs only inside RIM, its t by at most TAU -- on 60 000 rays, for an
    axis-parallel, an exactly turned and a generally turned disk with coordinates around 1 and around 40."""
    rng = np.random.default_rng(11)
    worst_t = worst_rim = 0.0
    for c, n, r in ((F([0, 0, 1]), F([0, 0, 1]), F(1)), (F([40.5, -37.25, 12]), F([0, 0, -1]), F(0.5)), (F([0.3, -0.2, 1.1]), F([0.2, -0.4, 1.3]), F(0.8)),
                    (F([-33.1, 20.7, 5.3]), F([0.7, 0.1, -0.2]), F(2.5))):
        nh = n.astype(np.float64) / np.linalg.norm(n.astype(np.float64))
        e1 = np.cross(nh, [1.0, 0, 0]); e1 /= np.linalg.norm(e1)
        e2 = np.cross(nh, e1)
        org, d = rays_at(c.astype(np.float64), e1, e2, nh, float(r), 15000, rng, spread=1.2)
        ok, t32 = D.disk32(org, d, c, n, r, 1e-4, np.inf)
        tab = D.classify(org, d, [c], [n], [r])
        t, rho, cos_phi, Dd = tab.t[:, 0], tab.rho[:, 0], tab.cos_phi[:, 0], tab.D[:, 0]
        tau, rim = D.tau(t, Dd, cos_phi), D.rim(t, Dd, cos_phi, float(r))
        front = t > 1e-3
        assert front.all() and (np.abs(t32 - t) <= tau).all()
        inside, outside = rho < float(r) - rim, rho > float(r) + rim
        assert ok[inside].all() and not ok[outside].any()
        assert (~inside & ~outside).mean() < 0.002 and 0.3 < inside.mean() < 0.8
        worst_t, worst_rim = max(worst_t, float((np.abs(t32 - t) / tau).max())), max(worst_rim, float(rim.max() / float(r)))
    print("largest |t32 - t| / TAU %.3f, widest rim band %.2e r" % (worst_t, worst_rim))
    assert worst_t < 0.5                                                                   # (the count is doubled: half of TAU is never used)


def test_normal32_restates_the_host():
    assert np.array_equal(D.normal32(np.eye(4)), F([0, 0, 1]))
    assert np.array_equal(D.normal32(np.diag([1.0, -1.0, -1.0, 1.0])), F([0, 0, -1]))
    assert np.array_equal(D.normal32(np.diag([2.0, 2.0, 2.0, 1.0])), F([0, 0, 0.5]))     # (M^-1)^T: a scale shortens the normal, which nothing minds
    T = np.eye(4)
    T[:3, :3] = 2.0 * np.asarray([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]])
    got = D.normal32(T.astype(F)).astype(np.float64)
    want = np.linalg.inv(T.astype(F).astype(np.float64)[:3, :3]).T[:, 2]
    assert np.allclose(got, want, rtol=8 * 2.0 ** -24, atol=2.0 ** -24)


def test_the_rules_pass_the_reference_and_catch_wrong_answers():
    rng = np.random.default_rng(3)
    c, n, r = F([0, 0, 1]), F([0, 0, 1]), F(1)
    tri = np.asarray([[[-4, -4, 0.5], [4, -4, 0.5], [0, 6, 0.5]]], dtype=np.float64)       # behind the disk for rays from above
    org, d = rays_at(c.astype(np.float64), np.asarray([1.0, 0, 0]), np.asarray([0, 1.0, 0]), np.asarray([0, 0, 1.0]), 1.0, 3000, rng, spread=1.3)
    cand = D.candidates(org, d, [(0, c, n, r)], tri, [1], [0])
    # the reference's own answer: the nearest candidate in front, disks decided by the exact sign
    ent, prim, t = np.full(3000, D.INVALID, dtype=np.uint32), np.full(3000, D.INVALID, dtype=np.uint32), np.full(3000, np.inf)
    tab = D.classify(org, d, [c], [n], [r])
    for k in range(len(cand.ray)):
        i = cand.ray[k]
        met = (tab.sign[i, 0] < 0) if cand.entity[k] == 0 else bool(cand.clear[k])
        if met and 1e-4 < cand.t[k] < t[i]:
            ent[i], prim[i], t[i] = cand.entity[k], cand.prim[k], cand.t[k]
    s = D.check_closest(cand, 1e-4, np.inf, (ent, prim, None, None, t))
    assert s["undecided"] < 0.01 and s["clear"] > 0.9 and s["undecided_disk"] < 0.005, s
    assert (ent == 0).sum() > 500 and (ent == 1).sum() > 500                               # both orders of disk and triangle occur
    hit_disk = np.nonzero(ent == 0)[0]
    for wrong in ("missed", "far", "phantom", "t"):
        e2, p2, t2 = ent.copy(), prim.copy(), t.copy()
        k = hit_disk[7]
        if wrong == "missed":
            e2[k] = p2[k] = D.INVALID
        elif wrong == "far":                                                              # the triangle behind, reported instead of the disk
            k = next(i for i in hit_disk if ((cand.ray == i) & (cand.entity == 1)).any())
            row = np.nonzero((cand.ray == k) & (cand.entity == 1))[0][0]
            e2[k], p2[k], t2[k] = 1, 0, cand.t[row]
        elif wrong == "phantom":
            k = np.nonzero(ent == D.INVALID)[0][0]
            e2[k], p2[k], t2[k] = 0, 0, 1.0
        else:
            t2[k] = t[k] * (1 + 1e-4)
        with pytest.raises(AssertionError):
            D.check_closest(cand, 1e-4, np.inf, (e2, p2, None, None, t2))
    # occlusion windows a margin either side of the nearest hit
    near = np.where(np.isfinite(t), t, 1.0)
    for scale, want in ((1.01, True), (0.99, False)):
        occ = np.isfinite(t) & want
        s = D.check_any(cand, 1e-4, near * scale + 0.001, occ)
        assert s["undecided"] < 0.01, s
    with pytest.raises(AssertionError):
        D.check_any(cand, 1e-4, near * 1.01 + 0.001, np.zeros(3000, dtype=bool))
    with pytest.raises(AssertionError):
        D.check_any(cand, 1e-4, near * 0.99 + 0.001, np.isfinite(t))


def test_the_form_factor_on_the_axis_and_far_away():
    for h, R in ((1.0, 1.0), (0.5, 2.0), (3.0, 0.25)):
        assert abs(D.form_factor(0.0, h, R) - R * R / (h * h + R * R)) < 1e-15
    assert abs(D.form_factor(50.0, 1.0, 1.0) - 1.0 / 50.0 ** 4) < 1e-9                    # ~ cos cos' A / (pi d^2) = h^2 pi R^2 / (pi d^4)
    # against the plain area quadrature of G / pi over the disk
    for a in (0.0, 0.5, 1.7):
        G, w = D._G_disk(a, 1.0, 1.0)
        assert abs(float((G * w).sum()) / np.pi - D.form_factor(a, 1.0, 1.0)) < 1e-12


def test_the_linear_radius_sampler_against_its_closed_form():
    for h, R in ((1.0, 1.0), (0.7, 1.3)):
        want = 0.5 * R * (R / (h * h + R * R) + np.arctan(R / h) / h)
        assert abs(D.nee_linear_radius(0.0, h, R) - want) < 1e-12
    got, true = D.nee_linear_radius(0.0, 1.0, 1.0), D.nee_uniform(0.0, 1.0, 1.0)
    assert abs(got - 0.6427) < 5e-5 and true == 0.5 and abs(got / true - 1.285) < 1e-3    # 28 % apart: a test at 2 % tells the samplers apart
    # a x2 scale: |det| = 8 in the area, samples on the disc of radius 2 R
    assert abs(D.nee_linear_radius(0.0, 1.0, 1.0, area_scale=8.0, sample_scale=2.0) - 4.0 * (0.2 + np.arctan(2.0) / 2.0)) < 1e-12


def test_the_mis_terms_sum_between_the_two_pure_estimators_and_weights_add_up():
    """w_l + w_b = 1 pointwise, so with an area-uniform sampler the two terms would add up to F; with the reference's sampler the light term is biased
    like the NEE-only estimator, less so: the sum lies between F and the NEE-only value."""
    for a in (0.0, 0.5):
        el, eb, ml, mb = D.mis_terms(a, 1.0, 1.0)
        lo, hi = D.form_factor(a, 1.0, 1.0), D.nee_linear_radius(a, 1.0, 1.0)
        assert lo < el + eb < hi and el > 0 and eb > 0 and ml > el * el and mb > eb * eb
