"""tests/mis_reference.py, the float64 model behind tests/test_gpu_mix_mis.py, held on a machine without a GPU:

 1  against closed forms (1e-12): seen along the normal under the constant environment, p_light = p_leaf = cos / pi, so for a tree of Lambert leaves with `eval`
    coefficients c_i (weight) and b_i (pdf) and `sample` products s_i (selection) and m_i (weight), albedos a_i, roulette r:
      light sample   sum a_i c_i / (1 + r sum b_i)                    (`balance`)      sum a_i c_i / (1 + (r sum b_i)^2)                       (`power`)
      bounce         a_i m_i r s_i / (1 + r s_i) with probability r s_i               a_i m_i (r s_i)^2 / (1 + (r s_i)^2) with probability r s_i
    a quarter of the bounce in mono, where the light sample is dropped.
 2  against the CPU checker, which is a second implementation of direct.cpp for the materials it knows: plain Lambert (two- and one-sided) and a mirror, in the
    very scenes of tests/test_gpu_mix_mis.py -- mono under the constant environment, every pixel at 1e-5 (+ 1e-6), both MIS modes, roulette at 1 and at 0.9; hero under
    the environment, the ratio of the frame with the bounce to the frame without it per pixel (the factors of the wavelengths cancel in it, also the squared one of
    `power`); and block means under the lamp within 6 standard errors + the quadrature error, hero `balance` (light sample and bounce) and mono in both modes with
    the roulette at 1 and at 0.9.
 3  the power of the GPU file's cases: for every rule switch of the model at least one case moves by more than 100 tolerances (exact tier) or 3 (statistical)."""
import numpy as np
import pytest

import mis_reference as R
import oracle_binding as ob
import test_gpu_mix_mis as G

F = np.float32
ENV, HEAD = R.ConstantEnvironment(), R.view(0.0)


# ---- 1: closed forms ----------------------------------------------------------------------------------------------------------------------------------------
A1, A2, A3 = R.L1[1], R.L2[1], R.L3[1]
F3, F4 = float(F(0.3)), float(F(0.4))
# name: (eval terms [(a, c, b)], sample terms of the Lambert leaves [(a, s, m)], of the delta leaves [(s, m)]) -- by hand from the rules, factors as fp32
CLOSED = {
    "blend(L1, L2, 0.3)": ([(A1, 1 - F3, 1 - F3), (A2, F3, F3)], [(A1, 1 - F3, 1 - F3), (A2, F3, F3)], []),
    "blend(L1, L2, 1.7)": ([(A2, 1.0, 1.0)], [(A2, 1.0, 1.0)], []),
    "add(L1, L2)": ([(A1, 1.0, 0.5), (A2, 1.0, 0.5)], [(A1, 0.5, 1.0), (A2, 0.5, 1.0)], []),
    "blend(blend(L1, L2, 0.25), L3, 0.4)": ([(A1, (1 - F4) * 0.75, (1 - F4) * 0.75), (A2, (1 - F4) * 0.25, (1 - F4) * 0.25), (A3, F4, F4)],
                                            [(A1, (1 - F4) * 0.75, (1 - F4) * 0.75), (A2, (1 - F4) * 0.25, (1 - F4) * 0.25), (A3, F4, F4)], []),
    "add(blend(L1, L2, 0.25), L3)": ([(A1, 0.75, 0.375), (A2, 0.25, 0.125), (A3, 1.0, 0.5)], [(A1, 0.375, 0.75), (A2, 0.125, 0.25), (A3, 0.5, 1.0)], []),
    "blend(null, L1, 0.4)": ([(A1, F4, F4)], [(A1, F4, F4)], [(1 - F4, 1 - F4)]),
    "add(mirror, L1)": ([(A1, 1.0, 0.5)], [(A1, 0.5, 1.0)], [(0.5, 1.0)]),
    "blend(null, blend(null, L1, 0.5), 0.5)": ([(A1, 0.25, 0.25)], [(A1, 0.25, 0.25)], [(0.5, 0.5), (0.25, 0.25)]),
}


@pytest.mark.parametrize("rr", [1.0, float(F(0.9))])
@pytest.mark.parametrize("mis", ["balance", "power"])
@pytest.mark.parametrize("name", sorted(CLOSED))
def test_closed_forms_head_on_under_the_constant_environment(name, mis, rr):
    ev, sa, de = CLOSED[name]
    t = (lambda x: x * x) if mis == "power" else (lambda x: x)
    for mono, quarter in ((False, 1.0), (True, 0.25)):
        nee, bounce = R.exact_values(R.MATERIALS[name], ENV, HEAD, mis=mis, rr=rr, mono=mono)
        if mono:
            assert nee is None
        else:
            assert abs(nee - sum(a * c for a, c, _ in ev) / (1 + t(rr * sum(b for _, _, b in ev)))) <= 1e-12
        # a Lambert leaf: weighted against the light; a delta leaf: the environment in full, times its weight product
        want = sorted([(quarter * a * m * t(rr * s) / (1 + t(rr * s)), rr * s) for a, s, m in sa] + [(m, rr * s) for s, m in de])
        assert len(bounce) == len(want) and all(abs(v - w) <= 1e-12 and abs(p - q) <= 1e-12 for (v, p), (w, q) in zip(sorted(bounce), want)), (bounce, want)


def test_the_issues_figure_and_the_delta_leaves():
    nee, bounce = R.exact_values(R.MATERIALS["blend(L1, L2, 0.3)"], ENV, HEAD)
    assert abs(nee - 0.37) < 1e-7 and abs(sum(v * p for v, p in bounce) - 0.17387) < 1e-5 and abs(nee + sum(v * p for v, p in bounce) - 0.54387) < 1e-5
    # a delta leaf counts the environment in full, times its weight product: blend scales it, add does not; a delta-only tree is never ended by the roulette
    _, b = R.exact_values(R.MATERIALS["blend(null, L1, 0.4)"], ENV, HEAD, rr=0.9, mono=True)
    assert any(abs(v - (1 - float(F(0.4)))) < 1e-12 and abs(p - 0.9 * (1 - float(F(0.4)))) < 1e-12 for v, p in b)
    _, b = R.exact_values(R.MATERIALS["add(mirror, L1)"], ENV, HEAD, mono=True)
    assert any(abs(v - 1.0) < 1e-12 and abs(p - 0.5) < 1e-12 for v, p in b)
    _, b = R.exact_values("mirror", ENV, HEAD, rr=0.9)
    assert b == [(1.0, 1.0)]
    assert R.leaves(R.MATERIALS["add(blend(L1, L2, 0.25), L3)"]) == [(R.L1, 0.375, 0.75), (R.L2, 0.125, 0.25), (R.L3, 0.5, 1.0)]
    assert R.rr_probability(1, 4) == 1.0 and R.rr_probability(1, 0) == float(F(0.9)) and R.rr_probability(0, 0) == 1.0 and abs(R.rr_probability(3, 1) - 0.81) < 1e-6


# ---- 2: the checker ---------------------------------------------------------------------------------------------------------------------------------------------
def checker(b, spp=1, tiles=None):
    o = ob.OracleScene(b.build())
    if tiles:
        o.set_tiles(tiles)
    o.render(spp, threads=8)
    xyz, smp, fb = o.output()
    ent = o.primary_hits()[0].reshape(o.height, o.width)
    o.close()
    return np.float64(xyz), smp, fb, ent


ANCHORS = {"lambert": ("lambert", 0.5), "one-sided lambert": ("lambert", 0.5, False), "mirror": "mirror"}


@pytest.mark.parametrize("soft", [4, 0])
@pytest.mark.parametrize("mis", ["balance", "power"])
@pytest.mark.parametrize("name", sorted(ANCHORS))
def test_checker_mono_head_on_every_pixel(name, mis, soft):
    """mono, the wavelength pdf is 1 and the frame holds the raw value: the model's bounce value itself, or 0 where the roulette ended the path"""
    tree = ANCHORS[name][:2] if name != "mirror" else "mirror"
    rr = R.rr_probability(1, soft)
    xyz, smp, fb, ent = checker(G.environment_scene(ANCHORS[name], True, mis, soft, 2, n=32))
    on = ent == 0
    assert on.all()
    _, values = R.exact_values(tree, ENV, HEAD, mis=mis, rr=rr, mono=True)
    assert len(values) == 1
    v, p = values[0]
    got = xyz[..., 1]
    hit = np.abs(got - v) <= 1e-5 * v + 1e-6
    print("%s %s soft %d: model %.7f with probability %.3f; frame %.7f .. %.7f on %.3f of the pixels, 0 elsewhere" % (name, mis, soft, v, p, got[hit].min(), got[hit].max(), hit.mean()))
    assert (hit | (got == 0)).all() and abs(hit.mean() - p) <= 6 * np.sqrt(p * (1 - p) / hit.size)
    assert ((fb & 7)[on] == (0 if name == "mirror" else 1)).all()            # the dropped light sample; a delta-only material takes none


@pytest.mark.parametrize("soft", [4, 0])
@pytest.mark.parametrize("mis", ["balance", "power"])
def test_checker_hero_head_on_bounce_over_light_sample(mis, soft):
    """hero: (light sample + bounce) / (light sample) per pixel.  Both frames draw the same numbers up to the end of the first vertex."""
    rr = R.rr_probability(1, soft)
    tree = ANCHORS["lambert"]
    with_bounce = checker(G.environment_scene(tree, False, mis, soft, 2, n=32))
    alone = checker(G.environment_scene(tree, False, mis, soft, 1, n=32))
    assert not with_bounce[2].any() and not alone[2].any() and (alone[0][..., 1] > 0).all()
    q = with_bounce[0][..., 1] / alone[0][..., 1]
    nee, bounce = R.exact_values(tree, ENV, HEAD, mis=mis, rr=rr)
    want = 1 + bounce[0][0] / nee
    hit = np.abs(q - want) <= 1e-5 * want + 1e-6
    ended = np.abs(q - 1) <= 1e-6
    print("%s soft %d: model ratio %.7f; frame %.7f .. %.7f on %.3f of the pixels" % (mis, soft, want, q[hit].min(), q[hit].max(), hit.mean()))
    assert (hit | ended).all() and abs(hit.mean() - rr) <= 6 * np.sqrt(rr * (1 - rr) / hit.size)


TILES = [(px - R.BLOCK_HALF, py - R.BLOCK_HALF, px + R.BLOCK_HALF + 1, py + R.BLOCK_HALF + 1) for px, py in R.BLOCKS]


@pytest.fixture(scope="module")
def checker_hero_factor():
    """tests/test_gpu_mix_mis.py's hero anchor, on the checker"""
    def render(b, spp):
        xyz, smp, fb, ent = checker(b, spp)
        assert not fb.any()
        return xyz, ent == 0
    return G.hero_anchor(render)[1]


@pytest.mark.parametrize("mono,mis,soft", [(False, "balance", 4), (True, "balance", 4), (True, "power", 4), (True, "balance", 0), (True, "power", 0)])
def test_checker_block_means_under_the_lamp(mono, mis, soft, checker_hero_factor):
    rr = R.rr_probability(1, soft)
    xyz, smp, fb, ent = checker(G.lamp_scene(R.L1, mono=mono, mis=mis, soft=soft), spp=R.SPP, tiles=TILES)
    for (px, py), (x0, y0, x1, y1) in zip(R.BLOCKS, TILES):
        assert (ent[y0:y1, x0:x1] == 0).all() and (smp[y0:y1, x0:x1] == R.SPP).all()
        want, se, err = R.statistical_case(R.L1, 0.0, (px, py), hero_second_moment=1.0 if mono else checker_hero_factor, mis=mis, rr=rr, mono=mono)
        got = float(xyz[y0:y1, x0:x1, 1].mean())
        print("lambert 0.8 %s %s soft %d block (%d, %d): checker %.5f model %.5f, deviation %.3g allowed %.3g (standard error %.3f %%, quadrature %.1e)"
              % ("mono" if mono else "hero", mis, soft, px, py, got, want, abs(got - want), 6 * se + err, 100 * se / want, err))
        assert abs(got - want) <= 6 * se + err


# ---- 3: the power of the GPU file's cases ------------------------------------------------------------------------------------------------------------------------
def exact_movement(right, wrong):
    """how far the wrong rule's values lie from the right rule's, in tolerances: a value the right rule does not have counts by its distance to the nearest it has"""
    if not wrong or not right:
        return 0.0 if len(wrong) == len(right) else np.inf
    return max(min(abs(w - v) / (R.EXACT_RTOL * abs(v) + R.EXACT_ATOL) for v in right) for w in wrong)


def test_every_rule_switch_moves_a_case_of_the_gpu_file():
    table = {s: {} for s in R.SWITCHES}
    for name in R.HEAD_ON:
        tree = R.MATERIALS[name]
        for mis, soft in R.MONO_SETUPS:
            kw = dict(mis=mis, rr=R.rr_probability(1, soft), mono=True)
            right = [v for v, _ in R.exact_values(tree, ENV, HEAD, **kw)[1]]
            for s in R.SWITCHES:
                table[s]["mono %s soft %d: %s" % (mis, soft, name)] = ("exact", exact_movement(right, [v for v, _ in R.exact_values(tree, ENV, HEAD, **kw, **{s: True})[1]]))
        for mis in R.HERO_SETUPS:
            right = [R.exact_values(tree, ENV, HEAD, mis=mis)[0]]
            for s in R.SWITCHES:
                table[s]["hero %s depth 1: %s" % (mis, name)] = ("exact", exact_movement(right, [R.exact_values(tree, ENV, HEAD, mis=mis, **{s: True})[0]]))
    for name, tree in R.MATERIALS.items():
        for block in R.BLOCKS:
            want, se, err = R.statistical_case(tree, R.tilt_of(name), block, hero_second_moment=R.HERO_SECOND_MOMENT)
            assert se <= 0.004 * want, (name, block, se / want)
            base = R.statistical_case(tree, R.tilt_of(name), block, quick=True)[0]
            for s in R.SWITCHES:
                moved = R.statistical_case(tree, R.tilt_of(name), block, quick=True, **{s: True})[0]
                table[s]["lamp block %s: %s" % (block, name)] = ("statistical", abs(moved - base) / (6 * se + err))
    cases = list(next(iter(table.values())))
    print("movement in tolerances (exact tier: needs > 100; statistical tier: needs > 3); '.' = none")
    print("%-72s" % "case" + "".join("%10s" % s[:9] for s in R.SWITCHES))
    for c in cases:
        print("%-72s" % c + "".join("%10s" % ("." if table[s][c][1] == 0 else "%.3g" % table[s][c][1]) for s in R.SWITCHES))
    for s in R.SWITCHES:
        caught = [c for c in cases if table[s][c][1] > (100 if table[s][c][0] == "exact" else 3)]
        print("%s: caught by %d cases, e.g. %s" % (s, len(caught), caught[:3]))
        assert caught, s
        assert {table[s][c][0] for c in caught} == {"exact", "statistical"}, s   # ... in either tier
