"""Nested blend / add materials on the host (include/prgpu.h, PRGPU_MIX_MAX_DEPTH / PRGPU_MIX_MAX_LEAVES; csrc/host/mix_tree.h): a blend or add may name
a blend or add declared earlier as a child.  No GPU is needed: the loader and SceneBuilder are host code, prgpu_mix_leaves returns the flattened tree
the device reads without a device, and prgpu_scene_create validates before it selects one.

 1  The loader keeps kinds, child indices and factors of nested trees as written, and SceneBuilder assembles byte-identical records.
 2  prgpu_mix_leaves against a recursive restatement, in float64, of the rules of blend.cpp / add.cpp: which leaves eval reaches,
    their weight and pdf coefficients (4 ulp of fp32: the library forms the products in fp32 from the root down, one rounding per level and one for
    1 - f), the delta-only bit, the leaf whose scattering type the root reports and the leaf whose delta flag it reports.
 3  The two bounds, in the loader, in SceneBuilder and in the validation of a hand-built description."""
import ctypes as C

import numpy as np
import pytest

from pearray_amd import _cabi as abi
from pearray_amd import backend, scene

F = np.float32
SCENE = """(scene :render_width 8 :render_height 8
  (camera :name 'c' :type 'standard')
  %s
  (mesh :name 'q' (attribute :type 'p' [0,0,0],[1,0,0],[0,1,0]) (faces [0,1,2]))
  (entity :name 'e' :type 'mesh' :mesh 'q' :materials '%s')
)"""
_KEEP = []   # a description points into its PrcScene: the scenes of this module stay alive


def load(materials, used):
    _KEEP.append(scene.PrcScene(source=SCENE % (materials, used)))
    return _KEEP[-1]


def record(m):
    return C.string_at(C.addressof(m), C.sizeof(m))


# ---- 1: records ------------------------------------------------------------------------------------------------------------------------------
NESTED = """(material :name 'a' :type 'diffuse' :albedo (refl 0.8 0.2 0.2))
  (material :name 'b' :type 'orennayar' :albedo (refl 0.2 0.8 0.2) :roughness 0.4)
  (material :name 'c' :type 'diffuse' :albedo (refl 0.2 0.2 0.8))
  (material :name 'ab' :type 'blend' :material1 'a' :material2 'b' :factor 0.25)
  (material :name 'abc' :type 'mix' :material1 'ab' :material2 'c' :factor 0.4)
  (material :name 'a+b' :type 'add' :material1 'a' :material2 'b')
  (material :name 'a+b+c' :type 'add' :material1 'a+b' :material2 'c')
  (material :name 'hole' :type 'null')
  (material :name 'paint' :type 'diffuse' :albedo (refl 0.1 0.3 0.8))
  (material :name 'foil' :type 'conductor' :roughness 0.2)
  (material :name 'coat' :type 'add' :material1 'paint' :material2 'foil')
  (material :name 'cutout' :type 'blend' :material1 'hole' :material2 'coat' :factor 0.3)
  (material :name 'twice' :type 'blend' :material1 'ab' :material2 'a+b' :factor 0.5)"""


def test_the_loader_keeps_nested_trees_as_written():
    d = load(NESTED, "cutout").desc
    assert d.n_materials == 13
    m = d.materials
    want = {3: (abi.MAT_BLEND, 0, 1, 0.25), 4: (abi.MAT_BLEND, 3, 2, 0.4), 5: (abi.MAT_ADD, 0, 1, 0.0), 6: (abi.MAT_ADD, 5, 2, 0.0),
            10: (abi.MAT_ADD, 8, 9, 0.0), 11: (abi.MAT_BLEND, 7, 10, 0.3), 12: (abi.MAT_BLEND, 3, 5, 0.5)}   # 3 and 5 each have two parents
    for i, (kind, c1, c2, f) in want.items():
        assert (m[i].kind, m[i].two_sided, m[i].thin) == (kind, c1, c2), i
        assert m[i].roughness_x == F(f), i
    assert np.ctypeslib.as_array(d.tri_material, shape=(1,))[0] == 11


def test_scene_builder_assembles_the_loaders_nested_records():
    d = load(NESTED, "cutout").desc
    b = scene.SceneBuilder(8, 8)
    a = b.lambert(b.refl(0.8, 0.2, 0.2))
    bb = b.oren_nayar(b.refl(0.2, 0.8, 0.2), 0.4)
    c = b.lambert(b.refl(0.2, 0.2, 0.8))
    ab = b.blend(a, bb, 0.25)
    abc = b.blend(ab, c, 0.4)
    apb = b.add(a, bb)
    apbc = b.add(apb, c)
    hole = b.null()
    paint = b.lambert(b.refl(0.1, 0.3, 0.8))
    foil = b.rough_conductor(0.2)
    coat = b.add(paint, foil)
    cutout = b.blend(hole, coat, 0.3)
    twice = b.blend(ab, apb, 0.5)
    assert (a, bb, c, ab, abc, apb, apbc, hole, paint, foil, coat, cutout, twice) == tuple(range(13))
    assert d.n_spectra == len(b.spectra)
    for i in range(13):
        assert record(d.materials[i]) == record(b.materials[i]), i
    for i in range(d.n_spectra):
        assert record(d.spectra[i]) == record(b.spectra[i]), i


# ---- 2: the flattened tree ------------------------------------------------------------------------------------------------------------------------
DELTA_KINDS = (abi.MAT_DIELECTRIC, abi.MAT_CONDUCTOR, abi.MAT_MIRROR, abi.MAT_NULL)


def delta_only(mats, i):
    m = mats[i]
    if m.kind not in (abi.MAT_BLEND, abi.MAT_ADD):
        return m.kind in DELTA_KINDS
    return delta_only(mats, m.two_sided) and delta_only(mats, m.thin)


def restated(mats, i, a=1.0, b=1.0, symbol=True, flag=True):
    """[(leaf, a, b, is the symbol leaf, is the flag leaf)] of IMaterial::eval below material i, float64 products"""
    m = mats[i]
    if m.kind not in (abi.MAT_BLEND, abi.MAT_ADD):
        return [(i, a, b, symbol, flag)]
    add = m.kind == abi.MAT_ADD
    f = min(1.0, max(0.0, float(m.roughness_x)))
    d1, d2 = delta_only(mats, m.two_sided), delta_only(mats, m.thin)
    k1 = (a, b * 0.5) if add else (a * (1 - f), b * (1 - f))
    k2 = (a, b * 0.5) if add else (a * f, b * f)
    if d1 and d2:                     # form All
        return []
    if not d1 and not d2:             # form None: both children, no flag, the symbol from child 1 unless a blend leans to child 2
        first = add or f <= 0.5
        return restated(mats, m.two_sided, *k1, symbol and first, False) + restated(mats, m.thin, *k2, symbol and not first, False)
    if d1:                            # form First
        return restated(mats, m.thin, *k2, symbol, flag)
    return restated(mats, m.two_sided, *k1, symbol, flag)


def ulps(got, want):
    want32 = F(want)
    return abs(float(got) - float(want)) / float(np.spacing(abs(want32))) if want32 != 0 else (0.0 if got == 0 else np.inf)


def compare(b, root, label):
    got = backend.mix_leaves(b.build(), root)
    want = restated(b.materials, root)
    assert [l[0] for l in got["leaves"]] == [w[0] for w in want], (label, got, want)
    for (_, ga, gb), (_, wa, wb, _, _) in zip(got["leaves"], want):
        assert ulps(ga, wa) <= 4 and ulps(gb, wb) <= 4, (label, ga, wa, gb, wb)
    assert got["delta_only"] == delta_only(b.materials, root), label
    sym = [k for k, w in enumerate(want) if w[3]]
    flg = [k for k, w in enumerate(want) if w[4]]
    assert len(sym) <= 1 and len(flg) <= 1 and len(sym) == (1 if want else 0), label
    assert got["symbol_leaf"] == (sym[0] if sym else None), (label, got, sym)
    assert got["flag_leaf"] == (flg[0] if flg else None), (label, got, flg)
    return got


def builder():
    """a builder with one triangle, and its stock of plain materials: two diffuse, one Oren-Nayar, a rough conductor, and the four delta-only kinds"""
    b = scene.SceneBuilder(8, 8)
    p = {"a": b.lambert(b.spectrum_const(0.8)), "b": b.lambert(b.spectrum_const(0.6)), "o": b.oren_nayar(b.spectrum_const(0.4), 0.5), "r": b.rough_conductor(0.3),
         "null": b.null(), "mirror": b.mirror(), "glass": b.dielectric(b.spectrum_const(1.5)), "metal": b.conductor()}
    b.add_mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 1, 2]], p["a"])
    return b, p


FACTORS = (0.0, 0.3, 1.0, 1.7, -0.25)
# (child 1, child 2) of a combinator by its form
FORMS = {"None": ("a", "b"), "First": ("null", "b"), "Second": ("a", "mirror"), "All": ("glass", "null")}


@pytest.mark.parametrize("inner_form", sorted(FORMS))
@pytest.mark.parametrize("root_form", sorted(FORMS))
def test_every_form_at_the_root_and_one_level_down(root_form, inner_form):
    """the root's form is set by its OTHER child and by whether the inner combinator is delta-only; the inner one sits on either side"""
    for root_kind in ("blend", "add"):
        for inner_kind in ("blend", "add"):
            for inner_side in (1, 2):
                for f in FACTORS:
                    b, p = builder()
                    i1, i2 = (p[k] for k in FORMS[inner_form])
                    inner = b.blend(i1, i2, 0.3 if root_kind == "blend" else f) if inner_kind == "blend" else b.add(i1, i2)
                    other = p[FORMS[root_form][2 - inner_side]]      # the root's other child: plain, delta-only or not as the root's form says
                    c1, c2 = (inner, other) if inner_side == 1 else (other, inner)
                    root = b.blend(c1, c2, f) if root_kind == "blend" else b.add(c1, c2)
                    compare(b, root, (root_kind, root_form, inner_kind, inner_form, inner_side, f))
                    if root_kind == "add" and inner_kind == "add":
                        break   # no factor anywhere: one pass


def test_coefficients_of_the_issue_examples():
    b, p = builder()
    inner = b.blend(p["a"], p["b"], 0.25)
    got = compare(b, b.blend(inner, p["o"], 0.4), "blend(blend(a, b, .25), o, .4)")
    assert [l[0] for l in got["leaves"]] == [p["a"], p["b"], p["o"]]
    for (_, ga, gb), want in zip(got["leaves"], (0.6 * 0.75, 0.6 * 0.25, 0.4)):
        assert abs(ga - want) < 1e-6 and ga == gb
    got = compare(b, b.add(b.add(p["a"], p["b"]), p["o"]), "add(add(a, b), o)")
    assert [(float(x), float(y)) for _, x, y in got["leaves"]] == [(1.0, 0.25), (1.0, 0.25), (1.0, 0.5)]


def test_depth_one_coefficients_are_the_two_child_arithmetic():
    """a product with 1 and a scaling by a half: (1 - f, f) and (1, 0.5) exactly, f clamped"""
    for f in FACTORS:
        b, p = builder()
        got = compare(b, b.blend(p["a"], p["o"], f), f)
        fc = F(min(1.0, max(0.0, float(F(f)))))
        assert [(x, y) for _, x, y in got["leaves"]] == [(F(1) - fc, F(1) - fc), (fc, fc)]
    b, p = builder()
    got = compare(b, b.add(p["mirror"], p["o"]), "add, first delta-only")
    assert got["leaves"] == [(p["o"], F(1), F(0.5))] and got["flag_leaf"] == 0 and got["symbol_leaf"] == 0


def test_a_root_that_is_delta_only_through_two_levels():
    b, p = builder()
    root = b.blend(p["null"], b.blend(p["null"], p["mirror"], 0.5), 0.5)
    got = compare(b, root, "blend(null, blend(null, mirror))")
    assert got == {"leaves": [], "delta_only": True, "symbol_leaf": None, "flag_leaf": None}
    got = compare(b, b.add(b.add(p["glass"], p["metal"]), root), "add(add(glass, metal), ...)")
    assert got["delta_only"] and not got["leaves"]
    assert not compare(b, b.blend(p["null"], b.blend(p["null"], p["a"], 0.5), 0.5), "one diffuse leaf two levels down")["delta_only"]


def test_a_shared_child_counts_once_per_path():
    b, p = builder()
    M = b.blend(p["a"], p["b"], 0.3)
    got = compare(b, b.blend(M, M, 0.7), "blend(M, M)")
    assert [l[0] for l in got["leaves"]] == [p["a"], p["b"], p["a"], p["b"]]
    assert abs(sum(float(l[1]) for l in got["leaves"]) - 1.0) < 1e-6


def test_the_symbol_leaf_on_both_sides_of_a_half():
    for f, side in ((0.5, 0), (float(np.nextafter(F(0.5), F(1))), 1), (0.3, 0), (0.75, 1)):
        b, p = builder()
        left, right = b.blend(p["a"], p["b"], f), b.blend(p["o"], p["r"], f)
        got = compare(b, b.blend(left, right, f), f)
        assert got["symbol_leaf"] == (3 if side else 0), (f, got)          # f > 0.5 leans to child 2 at both levels
        got = compare(b, b.add(left, right), f)
        assert got["symbol_leaf"] == (1 if side else 0), (f, got)          # an add reports child 1, the blend below it leans
        assert got["flag_leaf"] is None


def test_the_flag_leaf_needs_a_chain_of_one_sided_forms():
    b, p = builder()
    got = compare(b, b.blend(p["null"], b.blend(p["a"], p["mirror"], 0.25), 0.4), "blend(null, blend(a, mirror))")
    assert got["leaves"][0][0] == p["a"] and got["flag_leaf"] == 0 and got["symbol_leaf"] == 0 and len(got["leaves"]) == 1
    for label, make in (("a None form at the root", lambda: b.blend(p["b"], b.blend(p["a"], p["mirror"], 0.25), 0.4)),
                        ("a None form below", lambda: b.blend(p["null"], b.blend(p["a"], p["b"], 0.25), 0.4)),
                        ("an add of two", lambda: b.add(p["glass"], b.add(p["a"], p["o"])))):
        assert compare(b, make(), label)["flag_leaf"] is None, label


def test_a_plain_material_is_one_leaf():
    b, p = builder()
    for name, m in p.items():
        got = backend.mix_leaves(b.build(), m)
        assert got == {"leaves": [(m, F(1), F(1))], "delta_only": name in ("null", "mirror", "glass", "metal"), "symbol_leaf": 0, "flag_leaf": 0}, name


def test_mix_leaves_refuses_what_scene_creation_refuses():
    b, p = builder()
    sc = b.build()
    with pytest.raises(abi.PrgpuError) as e:
        backend.mix_leaves(sc, len(b.materials))
    assert "prgpu error -1:" in str(e.value)
    b, p = builder()
    b.materials.append(abi.Material(abi.MAT_BLEND, 0, p["a"], 0, 0, len(b.materials) + 1, 0, 0, 0.5, 0.0))
    with pytest.raises(abi.PrgpuError) as e:
        backend.mix_leaves(b.build(), len(b.materials) - 1)
    assert "prgpu error -4:" in str(e.value) and "smaller index" in str(e.value)


# ---- 3: bounds ----------------------------------------------------------------------------------------------------------------------------------------
def chain(depth):
    """(material text, name of the root): `depth` blends, each over the one before and a fresh diffuse leaf"""
    text = ["(material :name 'l0' :type 'diffuse')"]
    root = "l0"
    for k in range(1, depth + 1):
        text.append("(material :name 'l%d' :type 'diffuse') (material :name 'c%d' :type '%s' :material1 '%s' :material2 'l%d')" % (k, k, "blend" if k % 2 else "add", root, k))
        root = "c%d" % k
    return " ".join(text), root


def tree(leaves):
    """(material text, name of the root): pairs combined level by level -- balanced for a power of two; an odd one out joins the root"""
    text = ["(material :name 'l%d' :type 'diffuse')" % k for k in range(leaves)]
    level, n = ["l%d" % k for k in range(leaves)], 0
    while len(level) > 1:
        nxt = []
        for k in range(0, len(level) - 1, 2):
            text.append("(material :name 't%d' :type '%s' :material1 '%s' :material2 '%s')" % (n, "add" if n % 2 else "mix", level[k], level[k + 1]))
            nxt.append("t%d" % n)
            n += 1
        if len(level) % 2:
            nxt.append(level[-1])
        level = nxt
    return " ".join(text), level[0]


def build_like(desc, root):
    """the loader's material array through SceneBuilder's own calls"""
    b = scene.SceneBuilder(8, 8)
    for i in range(root + 1):
        m = desc.materials[i]
        if m.kind == abi.MAT_BLEND:
            assert b.blend(m.two_sided, m.thin, m.roughness_x) == i
        elif m.kind == abi.MAT_ADD:
            assert b.add(m.two_sided, m.thin) == i
        else:
            assert b.lambert(b.spectrum_const(1.0)) == i
    return b


def by_hand(records):
    """a description whose material array was written without SceneBuilder's checks: [(kind, child 1, child 2)] or None for a diffuse leaf"""
    b = scene.SceneBuilder(8, 8)
    spec = b.spectrum_const(1.0)
    for r in records:
        b.materials.append(abi.Material(abi.MAT_LAMBERT, spec, 1, 0, abi.INVALID_ID, 0, 0) if r is None else abi.Material(r[0], spec, r[1], 0, 0, r[2], 0, 0, 0.5, 0.0))
    b.add_mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 1, 2]], len(records) - 1)
    return b


def records_of(desc):
    return [((m.kind, m.two_sided, m.thin) if m.kind in (abi.MAT_BLEND, abi.MAT_ADD) else None) for m in (desc.materials[i] for i in range(desc.n_materials))]


@pytest.mark.parametrize("label,make,extent", [("a chain of depth 4", lambda: chain(abi.MIX_MAX_DEPTH), (4, 5)), ("a balanced tree of 8 leaves", lambda: tree(abi.MIX_MAX_LEAVES), (3, 8))])
def test_trees_at_the_bounds_load(label, make, extent):
    text, root = make()
    d = load(text, root).desc
    rid = d.n_materials - 1
    b = build_like(d, rid)
    assert b._mix_extent(rid) == extent
    for i in range(d.n_materials):
        assert (d.materials[i].kind, d.materials[i].two_sided, d.materials[i].thin) == (b.materials[i].kind, b.materials[i].two_sided, b.materials[i].thin), i
    assert len(backend.mix_leaves(d, rid)["leaves"]) == extent[1]
    # the validation of a hand-built description passes the tree: without a GPU the call gets as far as choosing a device (-2), with one it succeeds
    try:
        backend.RenderContext(by_hand(records_of(d)).build(), device=0).close()
    except abi.PrgpuError as e:
        assert "prgpu error -2:" in str(e), str(e)


@pytest.mark.parametrize("label,make,needle", [("a chain of depth 5", lambda: chain(abi.MIX_MAX_DEPTH + 1), "PRGPU_MIX_MAX_DEPTH"),
                                               ("a tree of 9 leaves", lambda: tree(abi.MIX_MAX_LEAVES + 1), "PRGPU_MIX_MAX_LEAVES")])
def test_trees_beyond_the_bounds_are_refused_by_name(label, make, needle):
    text, root = make()
    with pytest.raises(abi.PrgpuError) as e:                       # the loader
        load(text, root)
    assert e.value.args[1] == -4 and needle in e.value.args[0], e.value.args
    # the same array minus its root loads; SceneBuilder refuses the root
    inner, _ = make()
    cut = inner.rindex("(material")
    d = load(inner[:cut], "l0").desc
    b = build_like(d, d.n_materials - 1)
    last = [s for s in inner[cut:].replace("'", " ").split()]
    name_to_id = {}
    for i, chunk in enumerate(inner.split("(material")[1:]):
        name_to_id[chunk.split("'")[1]] = i
    c1, c2 = name_to_id[last[last.index(":material1") + 1]], name_to_id[last[last.index(":material2") + 1]]
    with pytest.raises(ValueError, match=needle):
        b.blend(c1, c2)
    with pytest.raises(ValueError, match=needle):
        b.add(c1, c2)
    # a hand-built record: refused by prgpu_scene_create's validation, before a device is chosen, and by prgpu_mix_leaves
    recs = records_of(d) + [(abi.MAT_ADD, c1, c2)]
    hb = by_hand(recs)
    with pytest.raises(abi.PrgpuError) as e:
        backend.RenderContext(hb.build(), device=0)
    assert "prgpu error -4:" in str(e.value) and needle in str(e.value), str(e.value)
    with pytest.raises(abi.PrgpuError) as e:
        backend.mix_leaves(hb.build(), len(recs) - 1)
    assert "prgpu error -4:" in str(e.value) and needle in str(e.value), str(e.value)
