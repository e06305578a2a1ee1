"""Nested blend / add materials on the GPU (device/render.hip: vertex_eval walks the flattened row of a tree, shade_vertex descends it to sample), against
closed forms, in the set-ups of tests/test_gpu_mix_materials.py, whose harness this file imports unchanged: one quad under an orthographic camera, a mono
spectral domain, every value the RATIO of the frame to the frame with a Lambert albedo of 1.  Tolerance: that file's 1e-5 relative + 1e-6 absolute -- the
flattened coefficients add at most four roundings of 6e-8, any error of rule is at least 1e-2.  The Lambert leaves L1, L2, L3 have the constant albedos
0.8, 0.6, 0.4.

 4  Eval (one distant light at 45 degrees, next event estimation, depth limit 1): blend(blend(L1, L2, f1), L3, f2) = (1 - f2)((1 - f1) 0.8 + f1 0.6) + f2 0.4
    for three pairs of factors (one clamped from above, one from below), add(add(L1, L2), L3) = 1.8, add(blend(L1, L2, 0.25), L3) = 1.15,
    blend(add(L1, L2), L3, 0.4) = 1.0, and a tree with an Oren-Nayar leaf against that file's float64 formula.
 5  One-sided forms: blend(null, blend(L1, mirror, 0.25), 0.4) = 0.4 0.75 0.8; blend(blend(null, mirror, 0.3), L1, 0.4) = 0.4 0.8;
    add(mirror, add(null, L1)) = 0.8.
 6  Sampling (constant environment, no next event estimation, depth limit 2, one sample per pixel): every pixel of blend(blend(L1, L2, 0.25), L3, 0.4) is
    0.45 0.8, 0.15 0.6 or 0.4 0.4, with shares within 6 binomial standard deviations of 0.45 / 0.15 / 0.40 (computed from the pixel count: about 0.047 /
    0.034 / 0.046 on 4096); add(add(L1, L2), L3): 0.8 / 0.6 / 0.4 with shares 0.25 / 0.25 / 0.5.
 7  A root that is delta-only one level down: blend(null, blend(null, L1, 0.5), 0.5) alone: pixels 0.5 (through the root's null), 0.25 (through the inner
    one) or 0.25 0.8, shares 0.5 / 0.25 / 0.25.  Then blend(null, blend(null, mirror, 0.5), 0.5), delta-only through two levels, on a small quad in front of
    the Lambert quad (depth limit 3): a pixel whose path took a null branch is the frame without the quad times 0.5 resp. 0.25, a pixel whose path took the
    mirror is 0.25 of the environment; the shares of the three selection products 0.5 / 0.25 / 0.25.
 8  Light path expressions partition the main plane in the scenes of 6 and 7.
 9  A Cornell box with a depth-3 tree (principled and Sellmeier-glass leaves), a sub-tree with two parents and a depth-one blend renders to the same frame,
    sample counts and statistics, bit for bit, in every pipeline.  (pipelineInfo does not expose the shade class of a triangle.)

Not pinned here: the pdf a sampled level contributes (observable only through multiple importance sampling at a later vertex: tests/test_gpu_mix_mis.py
holds it) and the order of the draws across levels, which no statistic sees; both restate blend.cpp:104-122 / add.cpp:92-110."""
import numpy as np
import pytest

import test_gpu_mix_materials as mm
from pearray_amd import _cabi as abi
from pearray_amd import backend, scene

pytestmark = pytest.mark.gpu
F = np.float32
L1, L2, L3 = (float(F(x)) for x in (0.8, 0.6, 0.4))   # as the scene holds them


def const_lambert(albedo):
    return lambda b: (b.lambert(b.spectrum_const(albedo)), lambda wl, bb: albedo)


def plain(name):
    return lambda b: ({"null": b.null, "mirror": b.mirror}[name](), None)


def tree(spec):
    """material(b) for ratio(): spec is ("blend", spec, spec, f), ("add", spec, spec) or a leaf maker; a leaf maker used twice is one material"""
    def material(b):
        made = {}

        def build(s):
            if not isinstance(s, tuple):
                if s not in made:
                    made[s] = s(b)[0]
                return made[s]
            c1, c2 = build(s[1]), build(s[2])
            return b.blend(c1, c2, s[3]) if s[0] == "blend" else b.add(c1, c2)
        return build(spec)
    return material


def clamp(f):
    return min(1.0, max(0.0, float(F(f))))


A, B, C = const_lambert(L1), const_lambert(L2), const_lambert(L3)
NULL, MIRROR = plain("null"), plain("mirror")


# ---- 4: eval ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wl", mm.WAVELENGTHS)
@pytest.mark.parametrize("f1,f2", [(0.25, 0.4), (1.7, 0.4), (0.25, -0.25)])
def test_eval_of_a_blend_of_a_blend(f1, f2, wl):
    got, on, _, _ = mm.ratio(32, wl, tree(("blend", ("blend", A, B, f1), C, f2)), **mm.NEE)
    g1, g2 = clamp(f1), clamp(f2)
    mm.check("blend(blend(L1, L2, %g), L3, %g) at %g nm" % (f1, f2, wl), got, (1 - g2) * ((1 - g1) * L1 + g1 * L2) + g2 * L3, on)


@pytest.mark.parametrize("wl", mm.WAVELENGTHS)
@pytest.mark.parametrize("label,spec,want", [
    ("add(add(L1, L2), L3)", ("add", ("add", A, B), C), 1.8),
    ("add(blend(L1, L2, 0.25), L3)", ("add", ("blend", A, B, 0.25), C), 1.15),
    ("blend(add(L1, L2), L3, 0.4)", ("blend", ("add", A, B), C, 0.4), 1.0),
])
def test_eval_of_mixed_trees(label, spec, want, wl):
    got, on, _, _ = mm.ratio(32, wl, tree(spec), **mm.NEE)
    mm.check("%s at %g nm" % (label, wl), got, want, on)


def test_eval_with_an_oren_nayar_leaf_two_levels_down():
    V, L = mm.view_vector(np.pi / 4), mm.unit32(mm.NEE["light"])
    made = {}

    def material(b):
        made["on"] = mm.rough_diffuse(mm.B_RGB, 0.5, V, L)(b)
        l1, l3 = b.lambert(b.spectrum_const(L1)), b.lambert(b.spectrum_const(L3))
        return b.blend(l3, b.add(l1, made["on"][0]), 0.3)
    got, on, b, _ = mm.ratio(32, 550.0, material, **mm.NEE)
    rough = made["on"][1](550.0, b)
    f = float(F(0.3))
    assert abs(rough - mm.albedo_at(b, b.materials[made["on"][0]].albedo, 550.0)) > 0.01   # the leaf is not a Lambert term in disguise
    mm.check("blend(L3, add(L1, oren-nayar), 0.3)", got, (1 - f) * L3 + f * (L1 + rough), on)


# ---- 5: one-sided forms ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wl", mm.WAVELENGTHS)
@pytest.mark.parametrize("label,spec,want", [
    ("blend(null, blend(L1, mirror, 0.25), 0.4)", ("blend", NULL, ("blend", A, MIRROR, 0.25), 0.4), float(F(0.4)) * 0.75 * L1),
    ("blend(blend(null, mirror, 0.3), L1, 0.4)", ("blend", ("blend", NULL, MIRROR, 0.3), A, 0.4), float(F(0.4)) * L1),
    ("add(mirror, add(null, L1))", ("add", MIRROR, ("add", NULL, A)), L1),
])
def test_eval_of_one_sided_forms(label, spec, want, wl):
    got, on, _, _ = mm.ratio(32, wl, tree(spec), **mm.NEE)
    mm.check("%s at %g nm" % (label, wl), got, want, on)


# ---- 6, 8: sampling ------------------------------------------------------------------------------------------------------------------------------------
def multi_valued(label, got, on, values, shares):
    """mm.two_valued for any number of values: every pixel of `on` is one of `values` (1e-5 relative + 1e-6), none is left over, and each share is within 6
    binomial standard deviations of its expectation.  Returns the masks."""
    assert all(abs(x - y) > 0.01 for k, x in enumerate(values) for y in values[k + 1:])
    N = int(on.sum())
    masks = [np.abs(got - v) <= 1e-5 * abs(v) + 1e-6 for v in values]
    left = on & ~np.logical_or.reduce(masks)
    rows = []
    for v, p, m in zip(values, shares, masks):
        rows.append((v, m[on].mean(), p, 6 * np.sqrt(p * (1 - p) / N)))
    print("%s: %d pixels, other values: %d; " % (label, N, left.sum()) + "; ".join("value %.6g share %.4f (expected %.4f, allowed +- %.4f)" % r for r in rows))
    assert not left.any(), label
    for v, share, p, room in rows:
        assert abs(share - p) <= room, (label, v)
    return masks


def test_sampling_a_blend_of_a_blend_picks_one_leaf_per_vertex():
    got, on, _, planes = mm.ratio(64, 550.0, tree(("blend", ("blend", A, B, 0.25), C, 0.4)), extent=1.3, lpe=mm.LPE_PLANES)
    assert on.all() and on.sum() == 4096
    f1, f2 = float(F(0.25)), float(F(0.4))
    multi_valued("blend(blend(L1, L2, 0.25), L3, 0.4) sample", got, on, [(1 - f2) * (1 - f1) * L1, (1 - f2) * f1 * L2, f2 * L3], [0.45, 0.15, 0.40])
    assert mm.same(planes[0], got) and not planes[1].any() and not planes[2].any()      # 8: every leaf scatters by diffuse reflection


def test_sampling_an_add_of_an_add_picks_one_leaf_per_vertex():
    got, on, _, planes = mm.ratio(64, 550.0, tree(("add", ("add", A, B), C)), extent=1.3, lpe=mm.LPE_PLANES)
    assert on.all() and on.sum() == 4096
    multi_valued("add(add(L1, L2), L3) sample", got, on, [L1, L2, L3], [0.25, 0.25, 0.5])
    assert mm.same(planes[0], got) and not planes[1].any() and not planes[2].any()


# ---- 7, 8: delta-only below the root ----------------------------------------------------------------------------------------------------------------------
def test_a_cut_out_of_a_cut_out():
    got, on, _, planes = mm.ratio(64, 550.0, tree(("blend", NULL, ("blend", NULL, A, 0.5), 0.5)), depth=3, extent=1.3, lpe=mm.LPE_PLANES)
    assert on.all()
    root, inner, leaf = multi_valued("blend(null, blend(null, L1, 0.5), 0.5)", got, on, [0.5, 0.25, 0.25 * L1], [0.5, 0.25, 0.25])
    # 8: straight through either null is specular transmission, the leaf reflects diffusely
    assert mm.same(planes[0] + planes[1] + planes[2], got) and not planes[2].any()
    assert np.array_equal(planes[1] != 0, root | inner) and np.array_equal(planes[0] != 0, leaf)


def test_a_root_that_is_delta_only_through_two_levels():
    kw = dict(depth=3, extent=0.1)
    ref, ref_ent = mm.reference(64, 550.0, **kw)
    b = mm.quad_scene(64, 550.0, lambda bb: bb.lambert(bb.spectrum_const(1.0)), **kw)
    front = b.blend(b.null(), b.blend(b.null(), b.mirror(), 0.5), 0.5)
    assert backend.mix_leaves(b.build(), front) == {"leaves": [], "delta_only": True, "symbol_leaf": None, "flag_leaf": None}
    h = 0.06                                                     # that file's null quad, with this material
    b.add_mesh([[-h, -h, 100], [h, -h, 100], [h, h, 100], [-h, h, 100]], [[0, 1, 2], [0, 2, 3]], front, normals=[[0, 0, 1]] * 4)
    got, ent, info, planes = mm.frame(b, lpe=["C<T,S><R,D>L", "C<R,S>L"])
    assert info["variant"] == 5 and (ref_ent == 0).all() and (ent == 1).all()          # every camera ray meets the small quad first
    ch = int(np.argmax(ref.mean((0, 1))))
    r, g = ref[..., ch], got[..., ch]
    assert r.min() > 0
    through, bounced = planes[0][..., ch] != 0, planes[1][..., ch] != 0
    assert not (through & bounced).any() and (through | bounced).all()
    assert mm.same(planes[0] + planes[1], got)                                          # 8
    q = g / r
    half, quarter = through & (np.abs(q - 0.5) <= 1e-5 * 0.5 + 1e-6), through & (np.abs(q - 0.25) <= 1e-5 * 0.25 + 1e-6)   # the frame without the quad, times the selection product
    N = q.size
    print("delta-only through two levels: %d pixels, root null %.4f, inner null %.4f, mirror %.4f (expected 0.5 / 0.25 / 0.25, allowed +- %.4f / %.4f)"
          % (N, half.mean(), quarter.mean(), bounced.mean(), 6 * np.sqrt(0.25 / N), 6 * np.sqrt(0.1875 / N)))
    assert np.array_equal(half | quarter, through)
    # the mirror sends the ray back up into the environment of radiance 1, which is what the albedo-1 frame shows too: 0.25 of it
    assert (np.abs(q[bounced] - 0.25) <= 1e-5 * 0.25 + 1e-6).all()
    assert abs(half.mean() - 0.5) <= 6 * np.sqrt(0.25 / N)
    assert abs(quarter.mean() - 0.25) <= 6 * np.sqrt(0.1875 / N) and abs(bounced.mean() - 0.25) <= 6 * np.sqrt(0.1875 / N)


# ---- 9: every pipeline ------------------------------------------------------------------------------------------------------------------------------------
def cornell():
    """The Cornell box with a depth-3 tree on the short box -- blend(add(S, principled), Sellmeier glass) over the shared sub-tree S = blend(paint,
    Oren-Nayar) --, add(S, rough conductor) on the tall box, and a depth-one cut-out ceiling."""
    b = scene.SceneBuilder(64, 64)
    b.settings.aa_sampler, b.settings.aa_samples = abi.SAMPLER_MJITT, 4
    b.settings.max_ray_depth = 8
    shared = {}

    def S(bb):
        if "S" not in shared:
            shared["S"] = bb.blend(bb.lambert(bb.refl(0.2, 0.6, 0.3)), bb.oren_nayar(bb.refl(0.8, 0.8, 0.3), 0.5), 0.5)
        return shared["S"]
    over = {
        "ceiling": lambda bb: bb.blend(bb.null(), bb.lambert(bb.refl(0.7, 0.7, 0.7)), 0.8),
        "shortBox": lambda bb: bb.blend(bb.add(S(bb), bb.principled(base=bb.refl(0.3, 0.4, 0.8), roughness=0.4, metallic=0.3, clearcoat=0.5)),
                                        bb.dielectric(bb.lookup_index("bk7")), 0.3),
        "tallBox": lambda bb: bb.add(S(bb), bb.rough_conductor(0.3, specularity=bb.spectrum_const(0.4))),
    }
    scene._cornell_into(b, material_override=over)
    trees = [i for i, m in enumerate(b.materials) if m.kind in (abi.MAT_BLEND, abi.MAT_ADD)]
    built = b.build()
    extents = sorted(b._mix_extent(i) for i in trees)
    assert extents == [(1, 2), (1, 2), (2, 3), (2, 3), (3, 4)], extents
    assert sum(1 for m in b.materials if shared["S"] in (m.two_sided, m.thin) and m.kind in (abi.MAT_BLEND, abi.MAT_ADD)) == 2
    return built


def test_every_pipeline_renders_the_same_nested_frame(monkeypatch):
    out = []
    for env in mm.PIPELINES:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ctx = backend.RenderContext(cornell(), device=0)
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
    assert np.isfinite(xyz).all() and xyz.max() > 0
    assert stats["shadow_rays"] > 1000 and stats["bounce_rays"] > 3000
    for (o, st, i), env in zip(out[1:], mm.PIPELINES[1:]):
        assert all(np.array_equal(x, y) for x, y in zip(o, (xyz, smp, fb))), env
        assert st == stats, (env, st, stats)
