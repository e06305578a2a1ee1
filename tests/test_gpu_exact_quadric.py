"""Analytic spheres and quadric entities on the GPU (device/pr_device.h: sphere_hit, quadric_roots, quadric_bounds_hit, quadric_hit), held to the exact-arithmetic
reference of tests/exact_quadric.py WITHOUT the CPU checker: the ray service on the families of tests/test_exact_quadric.py (R1 - R4 and R6 of
exact_disk.check_closest / check_any, four- and six-wide trees, the plain and the split service kernel), and the primary hits of one camera scene in every pipeline
and integrator."""
import numpy as np
import pytest

import exact_disk as D
import exact_quadric as Q
import test_exact_quadric as T
import test_exact_rays as E
from pearray_amd import _cabi as abi
from pearray_amd import backend, scene
from test_gpu_vf import U, aov_ids, finish, render

pytestmark = pytest.mark.gpu
F = np.float32
INV = abi.INVALID_ID
TMIN = T.TMIN


# ---- 1: the ray service ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", ["4", "6"])
@pytest.mark.parametrize("split", ["0", "1"])
@pytest.mark.parametrize("name", T.CASES)
def test_the_ray_service_is_held_to_the_exact_reference(monkeypatch, name, split, width):
    """traceRays / traceShadowRays on the CPU families' scenes; occlusion windows a margin either side of the reported distance; the window's end 1 % before and
    after the exact t.  The undecided shares are those tests/test_exact_quadric.py caps (the same candidates); the rules' own are printed."""
    monkeypatch.setenv("PRGPU_TRACE_SPLIT", split)
    monkeypatch.setenv("PRGPU_BVH_WIDTH", width)
    c = T.case(name)
    cand = c.closest()
    g = backend.RenderContext(c.builder.build())
    try:
        assert g.pipelineInfo()["bvh_width"] == int(width)
        hit = g.traceRays(c.org, c.direction, TMIN, np.inf)
        s = D.check_closest(cand, TMIN, np.inf, hit, label="%s closest width %s split %s" % (name, width, split))
        print("closest", s)
        ent, prim, u, v, t = hit
        on = np.isin(ent, c.analytic)
        assert not u[on].any() and not v[on].any() and not prim[on].any()                  # u = v = 0, primitive id 0
        assert all((ent == e).sum() > c.min_hits[0] for e in c.analytic) and all((ent == e).sum() > c.min_hits[1] for e in c.te)
        t_ref = T.nearest_clear(cand, c.n)
        for scale in (0.99, 1.01):
            limit = np.where(np.isfinite(t_ref), t_ref * scale, np.inf).astype(F)
            D.check_closest(cand, TMIN, limit.astype(np.float64), g.traceRays(c.org, c.direction, TMIN, limit), label="%s closest, tmax x %.2f" % (name, scale))
        near = np.where(ent != INV, t.astype(np.float64), 1.0)
        for lo32, hi32 in T.occlusion_windows(near, TMIN):
            sa = T.hold_any(c, g.traceShadowRays, lo32, hi32, "%s any width %s split %s" % (name, width, split))
            print("any", sa)                                                               # (hold_any asserts the share left to neither clause)
    finally:
        g.close()


# ---- 2: the path kernels' primary hits ---------------------------------------------------------------------------------------------------------------
CW, CH = 79, 59
LOOK, UP, RIGHT = np.asarray([0.0, 0.8, -0.6]), np.asarray([0.0, 0.6, 0.8]), np.asarray([1.0, 0.0, 0.0])
FAR_C = np.asarray([30.5, -22.25, 12.0])                                                     # the far sphere: |c| = 80 r
CAM_EYE = tuple(float(F(v)) for v in FAR_C - 6.0 * LOOK)
CAM = dict(width=1.3, height=1.3 * CH / CW, local_direction=tuple(LOOK), local_up=tuple(UP), local_right=tuple(RIGHT))
AOVS = ("position", "entity_id")
# (quadric of T.QUADRICS, linear part, place on the view plane through the far sphere: right, up)
PLACED = [(0, "identity", -2.6, 1.45), (1, "general", 2.6, 1.45), (2, "exact", -2.6, -1.4), (3, "general", 0.0, -1.4), (4, "identity", 2.6, -1.4)]


def camera_scene(integ=None):
    """Entity 0: the far sphere; 1: a sphere of radius 1e-3 two centimetres before the eye; 2 - 6: the five quadrics; 7: a backdrop behind everything."""
    b = scene.SceneBuilder(CW, CH)
    s = b.settings
    s.aa_sampler, s.aa_samples, s.filter, s.filter_radius = abi.SAMPLER_UNIFORM, 1, abi.FILTER_BLOCK, 0
    mats = [b.lambert(b.spectrum_const(0.3 + 0.05 * k)) for k in range(8)]
    spheres, quadrics = [], []
    for k, (Tm, r) in enumerate(((T.xform(np.eye(3), FAR_C + 1.45 * UP), 0.5), (T.xform(np.eye(3), np.asarray(CAM_EYE) + 0.02 * (LOOK + 0.1 * RIGHT - 0.15 * UP)), 1e-3))):
        assert b.add_sphere(mats[k], r, transform=Tm) == k
        spheres.append((k, D.centre32(Tm), Q.sphere_r32(Tm, r)))
    for q, kind, a, up in PLACED:
        name, p, lo, hi = T.QUADRICS[q]
        Tm = T.xform(T.LINEAR[kind] if kind != "exact" else T.PERMUTE @ np.diag([2.0, 1.0, 2.0]), FAR_C + a * RIGHT + up * UP)
        if isinstance(p, dict):
            args = dict(p)
            e = (b.add_cylinder if args.pop("kind") == "cylinder" else b.add_cone)(mats[len(quadrics) + 2], transform=Tm, **args)
        else:
            e = b.add_quadric(mats[len(quadrics) + 2], p, lo, hi, transform=Tm)
        quadrics.append((e, Q.HeldQuadric(Tm, *T.quadric_table(b, e))))
    back = np.asarray([FAR_C + 4.0 * LOOK - 30.0 * RIGHT - 20.0 * UP, FAR_C + 4.0 * LOOK + 30.0 * RIGHT - 20.0 * UP, FAR_C + 4.0 * LOOK + 40.0 * UP], dtype=F)
    te = b.add_mesh(back, [[0, 1, 2]], mats[7])
    Tc = np.eye(4, dtype=F)
    Tc[:3, 3] = CAM_EYE
    b.set_camera(Tc, near=1e-6, **CAM)
    return finish(b, integ), (spheres, quadrics, np.asarray([back], dtype=np.float64), [te], [0])


@pytest.fixture(scope="module")
def camera_case():
    y, x = np.meshgrid(np.arange(CH, dtype=np.float64), np.arange(CW, dtype=np.float64), indexing="ij")
    nx, ny = 2 * (x / CW - 0.5), -2 * (y / CH - 0.5)
    d = nx[..., None] * (0.5 * CAM["width"]) * RIGHT + ny[..., None] * (0.5 * CAM["height"]) * UP + LOOK
    n = CW * CH
    org, direction = np.broadcast_to(np.asarray(CAM_EYE, dtype=F), (n, 3)).copy(), E._unit32(d.reshape(n, 3))
    spheres, quadrics, tris, te, tp = camera_scene()[1]
    return org, direction, Q.candidates(org, direction, spheres, quadrics, tris, te, tp, tmin=1e-6, extra_ulps=E.CAMERA_ULPS)


PIPELINES = [(dict(PRGPU_MODE="persistent"), None), (dict(PRGPU_MODE="lockstep"), None), (dict(PRGPU_MODE="streaming"), None), ({}, ("ao", 1)),
             ({}, ("vf", "colored_entity_id", False))]


def test_primary_hits_in_every_pipeline(monkeypatch, camera_case):
    """One known ray per pixel (tests/test_exact_rays.py, input 8, restated in float64 with CAMERA_ULPS of room): the primary-hit plane of the persistent, lockstep
    and streaming path kernels and of the `ao` and `vf` pipelines under R1, R2 (by id) and R4; the position AOV of the path kernels at the exact point."""
    org, direction, cand = camera_case
    first = None
    for env, integ in PIPELINES:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ctx = render(camera_scene(integ)[0], 1, aovs=AOVS if integ is None else ())
        ent, prim = (a.reshape(-1) for a in ctx.primaryHits())
        info = ctx.pipelineInfo()
        planes = [ctx.aov(a) for a in AOVS] if integ is None else None
        ctx.close()
        for k in env:
            monkeypatch.delenv(k)
        label = "primary hits %s %s" % (env.get("PRGPU_MODE", info["mode"]), integ[0] if integ else "direct")
        s = D.check_closest(cand, 1e-6, np.inf, (ent, prim, None, None, None), label=label)
        print(label, s)
        assert s["undecided"] <= 0.02 and all((ent == k).sum() > 12 for k in range(8)), (s, [(ent == k).sum() for k in range(8)])
        assert not prim[ent < 7].any()
        if first is None:
            first = (ent, prim)
        assert np.array_equal(first[0], ent) and np.array_equal(first[1], prim), label
        if planes is None:
            continue
        pos, eid = (p.reshape(len(ent), -1) for p in planes)
        assert np.array_equal(aov_ids(eid[:, 0])[ent != INV], ent[ent != INV].astype(np.uint64))
        # the position: o + t d with the kernel's own t and d -- within the row's tolerance plus the camera's and the roundings of o + t d, whose o is 30 units out
        rays = np.nonzero(ent < 7)[0]
        row = D.lookup(cand, rays, ent[rays], prim[rays])
        assert (row >= 0).all()
        fin = np.isfinite(cand.tol[row])
        want = org[rays].astype(np.float64) + cand.t[row][:, None] * direction[rays].astype(np.float64)
        room = cand.tol[row] + (E.CAMERA_ULPS + 4) * U * np.maximum(cand.t[row], np.abs(org[rays]).max(1))
        off = np.linalg.norm(pos[rays].astype(np.float64) - want, axis=1)
        print("position: largest share of the allowance %.3f on %d pixels" % ((off / room)[fin].max(), fin.sum()))
        assert fin.sum() > 400 and (off[fin] <= room[fin]).all() and np.median(room[fin]) < 1e-3
