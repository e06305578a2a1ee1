"""Next event estimation and multiple importance sampling through blend, add, nested and Oren-Nayar materials (device/render.hip: vertex_eval's weight and
pdf sums, shade_vertex's mix_weight / mix_pdf products), against tests/mis_reference.py, a float64 restatement of the estimator written recursively over the
material tree.  The CPU checker does not know these materials; tests/test_mis_reference.py anchors the model on it where it does (plain Lambert), holds it to
closed forms, and shows that every plausible wrong rule (a forgotten selection factor on the pdf, a scaled weight, a level that does not compound, ...) moves a
case of THIS file by more than 100 tolerances (exact tier) or 3 (statistical tier).

The harness is that of tests/test_gpu_mix_materials.py, imported unchanged: the quad [-1, 1]^2 with vertex normals, the orthographic camera, a block filter of
radius 0.  The materials are those of mis_reference.MATERIALS: Lambert leaves 0.8 / 0.6 / 0.4, an Oren-Nayar leaf (albedo 0.7, sigma 0.5), null and mirror.

Exact tier (1e-5 relative + 1e-6, that file's; a constant environment of radiance 1 WITH next event estimation, seen along the normal, one sample per pixel, 64 x 64,
every value the RATIO of a pixel to the same pixel of the Lambert-albedo-1 frame of the same set-up):
  mono   depth limit 2.  The light sample of every pixel is NaN and dropped (the model's `mono` rule), so every pixel of the quad carries the NaN feedback bit and
         no other; what remains is the bounce, weighted against the light's pdf with the pdf the material's `sample` reported.  Every ratio is one of the model's
         values and each value's share is within 6 binomial standard deviations.  `balance`, `power`, and `balance` with the roulette at 0.9 on the first vertex: both
         frames draw the roulette from the same number, so the paths it ends are the same pixels and are 0 in both; their share is held like a value's.
  hero   constant spectra, depth limit 1: the frame is the light sample alone.  A vertex draws its light sample BEFORE its roulette and material numbers
         (shade_vertex: handleNEE, then handleScattering), so with one sample per pixel the light direction is that of the Lambert-albedo-1 frame whatever the
         tree draws afterwards, and every pixel's ratio is the model's ONE value: eval's weight over 1 + eval's pdf coefficient.  `balance` and `power`.

Statistical tier (hero mode, constant spectra, `balance`, Y): the floor under a 2 x 2 lamp (an emissive mesh quad, black, facing down) one unit above it; a
40 x 40 film 2 wide under the multi-jittered sampler at 4096 samples per pixel; 5 x 5 pixel blocks under the lamp's centre and 0.5 beside it.  The block mean
against the model's expectation within 6 standard errors + the model's quadrature error.  The standard error comes from the model's second moments, never
from the frame, and is asserted to be at most 0.4 %.  The hero wavelengths scale the Y of a constant spectrum by a factor c per sample that is independent of the
path.  Its mean must be 1 -- it cancels in expectation, as tests/test_gpu_disk.py states -- but its spread is not small, so its second moment enters the
standard error: Var(c X) = E c^2 E X^2 - (E X)^2.  Both are measured ONCE on the anchor, a Lambert-albedo-1 quad under the constant environment without next event
estimation, where every sample is c: E c^2 from 64 x 64 samples, the mean from 1024 per pixel, held to 1 within 6 of its standard errors.
Measured on an MI355X: anchor mean 0.99971 over 4 194 304 samples (allowed 1 +- 0.00114), E c^2 = 1.1521, a spread of 39 % per sample, 0.12 % on a block mean of
102 400 samples -- inside standard errors of 0.16 .. 0.24 % and tolerances of 0.99 .. 1.47 % of the expectation.  Worst deviations measured there: mono 0.034 of
the allowed 1e-5 + 1e-6 and 0.18 of a share's allowance (0.3664 for 0.375, +- 0.0479); hero 5.7e-7 (0.042 of the allowed); block means 0.40 % where 1.16 % is allowed (0.35 of it).

One nested case of the statistical tier renders to the same frame, sample counts and statistics, bit for bit, in all four pipelines.

Not held: the ORDER of the draws across levels (no statistic sees it)."""
import numpy as np
import pytest

import mis_reference as R
import test_gpu_mix_materials as mm
from pearray_amd import _cabi as abi
from pearray_amd import backend

pytestmark = pytest.mark.gpu
F = np.float32
WL = 550.0
ONE = ("lambert", 1.0)


# ---- scenes (tests/test_mis_reference.py renders the Lambert ones with the CPU checker) ------------------------------------------------------------------
def material_of(tree):
    """material(b) for mm.quad_scene: the tree of mis_reference as materials of the builder, constant spectra"""
    def build(b, t):
        k = R.kind(t)
        if k == "lambert":
            return b.lambert(b.spectrum_const(t[1]), two_sided=t[2] if len(t) > 2 else True)
        if k == "oren":
            return b.oren_nayar(b.spectrum_const(t[1]), t[2])
        if k in ("null", "mirror"):
            return b.null() if k == "null" else b.mirror()
        c1, c2 = build(b, t[1]), build(b, t[2])
        return b.blend(c1, c2, t[3]) if k == "blend" else b.add(c1, c2)
    return lambda b: build(b, tree)


def integrator(b, mono, mis, soft, nee=True):
    s = b.settings
    s.nee, s.mis, s.soft_max_ray_depth = int(nee), {"balance": abi.MIS_BALANCE, "power": abi.MIS_POWER}[mis], soft
    if not mono:
        d = abi.default_settings(1, 1)
        s.spectral_mono, s.spectral_start, s.spectral_end = 0, d.spectral_start, d.spectral_end
    return b


def environment_scene(tree, mono, mis="balance", soft=4, depth=2, nee=True, n=64, spp=1):
    """the quad under the constant environment, seen along the normal, one sample per pixel"""
    return integrator(mm.quad_scene(n, WL, material_of(tree), depth=depth, extent=1.3, spp=spp), mono, mis, soft, nee)


ANCHOR_SPP = 1024


def hero_anchor(render):
    """The factor c by which a sample's wavelengths scale the Y of a constant spectrum, on the Lambert-albedo-1 quad under the constant environment WITHOUT next
    event estimation, hero mode, where every sample is c: its second moment from 4096 samples (one per pixel), its mean from ANCHOR_SPP per pixel.  The mean must be
    1 within 6 of its standard errors.  render(builder, spp) -> (xyz, mask of the quad's pixels).  Returns (mean, E c^2 / mean^2, standard error of the mean)."""
    xyz, on = render(environment_scene(ONE, False, nee=False), 1)
    c = np.float64(xyz[..., 1][on])
    m2 = float((c * c).mean())
    xyz, on = render(environment_scene(ONE, False, nee=False, spp=ANCHOR_SPP), ANCHOR_SPP)
    m1 = float(np.float64(xyz[..., 1][on]).mean())
    se = np.sqrt(max(m2 - m1 * m1, 0.0) / (c.size * ANCHOR_SPP))
    print("hero anchor: mean of %d samples %.5f (allowed 1 +- %.5f), second moment of %d samples %.5f: a spread of %.1f %% per sample"
          % (c.size * ANCHOR_SPP, m1, 6 * se, c.size, m2, 100 * np.sqrt(max(m2 - m1 * m1, 0.0))))
    assert abs(m1 - 1.0) <= 6 * se and m2 / (m1 * m1) <= R.HERO_SECOND_MOMENT
    return m1, m2 / (m1 * m1), se


def lamp_scene(tree, tilt=0.0, mono=False, mis="balance", soft=4, spp=R.SPP):
    """the quad under the lamp of mis_reference.LAMP and nothing else; the camera sits between the two (0.9 from the origin) and looks down at `tilt`"""
    b = mm.quad_scene(R.FILM_N, WL, material_of(tree), tilt=tilt, depth=2, spp=spp, extent=R.FILM_EXTENT)
    b.lights.clear()                                                           # (the harness adds an environment; this scene has none)
    b.settings.aa_sampler = abi.SAMPLER_MJITT
    hx, hy, h = R.LAMP
    b.add_mesh([[-hx, -hy, h], [hx, -hy, h], [hx, hy, h], [-hx, hy, h]], [[0, 2, 1], [0, 3, 2]], b.lambert(b.spectrum_const(0.0)), normals=[[0, 0, -1]] * 4,
               emission=b.diffuse_emission(b.spectrum_const(1.0)))
    sn, cs = float(F(np.sin(tilt))), float(F(np.cos(tilt)))
    T = np.eye(4, dtype=F)
    T[:3, 3] = (0.9 * sn, 0.0, 0.9 * cs)
    b.set_camera(T, width=R.FILM_EXTENT, height=R.FILM_EXTENT, local_direction=(-sn, 0.0, -cs), local_right=(cs, 0.0, -sn), local_up=(0.0, 1.0, 0.0), ortho=True)
    return integrator(b, mono, mis, soft)


def frame(b, nan_expected=False, top_variant=True):
    """mm.frame with the feedback this file expects: with nan_expected every pixel whose camera ray meets the quad carries the NaN bit and no other, every other
    pixel none; without it no pixel carries any.  Returns (xyz float64, mask of the quad's pixels)."""
    ctx = backend.RenderContext(b.build(), device=0)
    ctx.start()
    ctx.waitForFinish()
    xyz, smp, fb = ctx.output()
    ent = ctx.primaryHits()[0].reshape(ctx.height, ctx.width)
    info = ctx.pipelineInfo()
    ctx.close()
    on = ent == 0
    assert info["mode"] == 2 and info["kernel"] == "throughput" and (not top_variant or info["variant"] == 5), info
    if nan_expected:
        assert ((fb & 0x7)[on] == 0x1).all() and not (fb & 0x7)[~on].any(), "the NaN feedback bit on the quad's pixels, and nothing else"
    else:
        assert not (fb & 0x7).any(), "NaN / Inf / negative feedback bits"
    return np.float64(xyz), on, smp


_REFERENCE = {}


def reference(key, make):
    """the Lambert-albedo-1 frame of a set-up: computed once and left unchanged"""
    if key not in _REFERENCE:
        _REFERENCE[key] = make()
        _REFERENCE[key][0].setflags(write=False)
    return _REFERENCE[key]


def ratios(tree, mono, mis, soft, depth):
    """(ratio of the tree's frame to the Lambert-albedo-1 frame per pixel of the quad, mask of pixels at which that frame is not 0)"""
    ref, on, _ = reference(("env", mono, mis, soft, depth), lambda: frame(environment_scene(ONE, mono, mis, soft, depth), nan_expected=mono, top_variant=False))
    got, on2, _ = frame(environment_scene(tree, mono, mis, soft, depth), nan_expected=mono)
    assert np.array_equal(on, on2) and on.all() and on.sum() == 4096
    ch = 1
    lit = ref[..., ch] > 0
    assert not got[..., ch][~lit].any()                                        # where the roulette ended the albedo-1 path it ended this one
    with np.errstate(all="ignore"):
        return np.where(lit, got[..., ch] / ref[..., ch], 0.0), lit


def close_to(got, v):
    return np.abs(got - v) <= R.EXACT_RTOL * abs(v) + R.EXACT_ATOL


# ---- exact tier, mono: the bounce ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mis,soft", R.MONO_SETUPS)
@pytest.mark.parametrize("name", R.HEAD_ON)
def test_mono_every_pixel_is_one_of_the_models_bounce_values(name, mis, soft):
    rr = R.rr_probability(1, soft)
    assert rr == (1.0 if soft else float(F(0.9)))
    kw = dict(mis=mis, rr=rr, mono=True)
    env, V = R.ConstantEnvironment(), R.view(0.0)
    _, unit = R.exact_values(ONE, env, V, **kw)
    assert len(unit) == 1 and abs(unit[0][1] - rr) < 1e-12
    nee, values = R.exact_values(R.MATERIALS[name], env, V, **kw)
    assert nee is None
    values = [(v / unit[0][0], p / rr) for v, p in values]                    # as ratios, and as shares of the paths the roulette let through
    got, lit = ratios(R.MATERIALS[name], True, mis, soft, 2)
    n_all, n = lit.size, int(lit.sum())
    room = 6 * np.sqrt(rr * (1 - rr) / n_all)
    print("%s, mono, %s, roulette %.3g: %d of %d pixels lit (expected share %.4f, allowed +- %.4f)" % (name, mis, rr, n, n_all, rr, room))
    assert abs(n / n_all - rr) <= room
    left, worst, rows = lit.copy(), 0.0, []
    for v, p in values:
        m = lit & close_to(got, v)
        if m.any():
            worst = max(worst, float((np.abs(got[m] - v) / (R.EXACT_RTOL * abs(v) + R.EXACT_ATOL)).max()))
        left &= ~m
        rows.append((v, m.sum() / n, p, 6 * np.sqrt(p * (1 - p) / n)))
    print("  other values: %d; worst deviation %.3g of the allowed; " % (left.sum(), worst) + "; ".join("value %.6g share %.4f (expected %.4f, allowed +- %.4f)" % r for r in rows))
    assert all(abs(x[0] - y[0]) > 100 * (R.EXACT_RTOL * abs(x[0]) + R.EXACT_ATOL) for k, x in enumerate(values) for y in values[k + 1:])
    assert not left.any(), (name, got[left][:4])
    for v, share, p, allowed in rows:
        assert abs(share - p) <= allowed, (name, v, share, p)


# ---- exact tier, hero: the light sample -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mis", R.HERO_SETUPS)
@pytest.mark.parametrize("name", R.HEAD_ON)
def test_hero_depth_one_every_pixel_is_the_models_light_sample(name, mis):
    env, V = R.ConstantEnvironment(), R.view(0.0)
    unit = R.exact_values(ONE, env, V, mis=mis)[0]
    want = R.exact_values(R.MATERIALS[name], env, V, mis=mis)[0] / unit
    got, lit = ratios(R.MATERIALS[name], False, mis, 4, 1)
    assert lit.all()
    err = np.abs(got - want)
    room = R.EXACT_RTOL * abs(want) + R.EXACT_ATOL
    print("%s, hero, %s, depth 1: %d pixels, value %.6g, worst deviation %.3g (allowed %.3g)" % (name, mis, lit.sum(), want, err.max(), room))
    assert (err <= room).all()


# ---- statistical tier ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hero_factor():
    """hero_anchor() on the GPU, once"""
    return hero_anchor(lambda b, spp: frame(b, top_variant=False)[:2])


def block_mean(xyz, smp, px, py, spp):
    h = R.BLOCK_HALF
    assert (smp[py - h:py + h + 1, px - h:px + h + 1] == spp).all()
    return float(xyz[py - h:py + h + 1, px - h:px + h + 1, 1].mean())


def hold(name, tree, tilt, xyz, smp, c2):
    for block in R.BLOCKS:
        want, se, err = R.statistical_case(tree, tilt, block, hero_second_moment=c2)
        got = block_mean(xyz, smp, block[0], block[1], R.SPP)
        room = 6 * se + err
        print("%s block %s: rendered %.5f expected %.5f, deviation %.3g (%+.2f %%) allowed %.3g (%.2f %%): standard error %.3f %%, quadrature %.1e" %
              (name, block, got, want, abs(got - want), 100 * (got / want - 1), room, 100 * room / want, 100 * se / want, err))
        assert se <= 0.004 * want, (name, block, se / want)                  # from the model, not from the frame
        assert abs(got - want) <= room, (name, block, got, want)


@pytest.mark.parametrize("name", list(R.MATERIALS))
def test_block_means_under_the_lamp_follow_the_model(name, hero_factor):
    xyz, on, smp = frame(lamp_scene(R.MATERIALS[name], tilt=R.tilt_of(name)))
    hold(name, R.MATERIALS[name], R.tilt_of(name), xyz, smp, hero_factor[1])


def test_the_lambert_anchor_under_the_lamp(hero_factor):
    """plain Lambert, which the CPU checker renders too (tests/test_mis_reference.py holds the model to the checker there)"""
    xyz, on, smp = frame(lamp_scene(R.L1), top_variant=False)
    hold("lambert 0.8", R.L1, 0.0, xyz, smp, hero_factor[1])


# ---- every pipeline -------------------------------------------------------------------------------------------------------------------------------------------------
def test_every_pipeline_renders_the_same_nested_frame_under_the_lamp(monkeypatch):
    out = []
    for env in mm.PIPELINES:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ctx = backend.RenderContext(lamp_scene(R.MATERIALS["add(blend(L1, L2, 0.25), L3)"], spp=64).build(), device=0)
        ctx.start()
        ctx.waitForFinish()
        out.append((ctx.output(), ctx.statistics(), ctx.pipelineInfo()))
        ctx.close()
        for k in env:
            monkeypatch.delenv(k)
    (xyz, smp, fb), stats, info = out[0]
    print("pipelines:", [(i["mode"], i["kernel"], i["variant"]) for _, _, i in out], stats)
    assert info["mode"] == 2 and info["kernel"] == "throughput" and len({i["mode"] for _, _, i in out}) == 3
    assert all(i["variant"] == 5 for _, _, i in out)
    assert np.isfinite(xyz).all() and xyz.max() > 0 and not (fb & 0x7).any()
    assert stats["shadow_rays"] > 1000 and stats["bounce_rays"] > 3000
    for (o, st, i), env in zip(out[1:], mm.PIPELINES[1:]):
        assert all(np.array_equal(x, y) for x, y in zip(o, (xyz, smp, fb))), env
        assert st == stats, (env, st, stats)
