"""The ray service on device memory (prgpu_trace_closest_device / prgpu_trace_any_device; RenderContext.traceRaysDevice / traceShadowRaysDevice):
the same answers as the host entry points, every batch shape, every optional output, the hit's shading geometry against a float64 restatement of
the reference's provideGeometryPoint (tests/geometry_point_ref.py) and against the bits a pipeline commits to its AOV planes, stream order with
torch, refused rays, refused pointers, and a render that is left undisturbed.  tests/test_ray_service_device_args.py holds what needs no device.

Batches are a few thousand rays; the exact classification of an input of tests/test_exact_rays.py is computed once per session (E.case)."""
import ctypes as C

import numpy as np
import pytest
import torch  # before pearray_amd: the library then finds the HIP runtime torch has loaded

import geometry_point_ref as G
import test_exact_rays as E
from pearray_amd import _cabi as abi
from pearray_amd import backend, scene

pytestmark = pytest.mark.gpu
INVALID = 0xFFFFFFFF
EINVAL = -1


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda:0")


def host(t):
    """a result tensor as numpy; the int32 tensors of ids as the uint32 they hold"""
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


def device_closest(g, **kw):
    """the device path as a tracer numpy in, numpy out: (entity, prim, u, v, t), more with geometry / count_invalid"""
    def closest(org, direction, tmin, tmax):
        return tuple(host(x) for x in g.traceRaysDevice(dev(org), dev(direction), dev(tmin), dev(tmax), **kw))
    return closest


def device_any(g):
    def occluded(org, direction, tmin, distance):
        return host(g.traceShadowRaysDevice(dev(org), dev(direction), dev(tmin), dev(distance)))
    return occluded


# ---- 1. the same answers as the host path ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", ["4", "6"])
@pytest.mark.parametrize("split", ["1", "0"])
@pytest.mark.parametrize("name", ["aimed", "cube-unit", "windings", "axes", "icosphere-far"])
def test_the_device_path_answers_what_the_host_path_answers(monkeypatch, name, split, width):
    monkeypatch.setenv("PRGPU_TRACE_SPLIT", split)
    monkeypatch.setenv("PRGPU_BVH_WIDTH", width)
    c = E.case(name)
    g = backend.RenderContext(c.build_scene())
    try:
        closest, occluded = device_closest(g), device_any(g)
        want = g.traceRays(c.org, c.direction, c.tmin, c.tmax)
        got = closest(c.org, c.direction, c.tmin, c.tmax)
        for field, x, y in zip(backend.RayHits._fields, got, want):
            assert x.dtype == y.dtype and np.array_equal(x, y), (name, field)
        assert np.array_equal(occluded(c.org, c.direction, c.tmin, c.distance), g.traceShadowRays(c.org, c.direction, c.tmin, c.distance)), name
        if name in ("aimed", "windings"):   # the exact reference judges the new path directly
            E.hold_to_the_rules(c, closest, occluded, "device tensors split=%s width=%s" % (split, width))
    finally:
        g.close()


# ---- the scene of tests 3 - 5: one entity of every kind ---------------------------------------------------------------------------------------
def rot(axis, degrees):
    a = np.radians(degrees)
    c, s = np.cos(a), np.sin(a)
    m = np.eye(4)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    return m


def place(x, y, *more):
    m = np.eye(4)
    m[:3, 3] = (x, y, 0.0)
    for k in more:
        m = m @ k
    return m.astype(np.float32)


def grid(n, half, height):
    """(n + 1)^2 vertices over [-half, half]^2 with z = height(x, y), 2 n^2 triangles"""
    xs = np.linspace(-half, half, n + 1)
    x, y = [a.ravel() for a in np.meshgrid(xs, xs, indexing="ij")]
    pos = np.stack([x, y, height(x, y)], axis=-1).astype(np.float32)
    idx = lambda i, j: i * (n + 1) + j  # noqa: E731
    faces = [f for i in range(n) for j in range(n) for f in ((idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)))]
    return pos, np.asarray(faces, dtype=np.uint32)


class GeometryScene:
    """A mesh with vertex normals and uvs under a rotation and the non-uniform scale (1, 2, 0.5), a mesh without normals (an area light), a plane, a
    sphere, a disk and a cone, side by side in the plane z = 0 and facing +z; with `backdrop` a quad behind them that fills a camera's view.
    Entity e has material e.  Conditioning (what keeps the counted tolerance of test 4 below 1e-5): the patch is shallow (its vertex normals, the
    analytic ones of z = 0.08 (x^2 + y^2), stay within 6 degrees of the axis, so the Gram-Schmidt step of tangentFromUV removes little), its uv map
    is axis-aligned with determinant 0.25, far from the PR_EPSILON fallback; rays come from above at no more than about 20 degrees to the axis,
    so every normal they meet has N.z > 0.1 (frame_duff's copysign flips at 0); the cone is hit in the lower half of its height, away from its apex,
    where its gradient vanishes, and it stands at the ORIGIN: its normal goes through invTransform() * P, whose cancellation at a centre 3 away
    costs 2^-22 of absolute error that the gradient multiplies (counted: 8e-5 for a cone of radius 0.5 at (2.5, -1.5), which is ill-conditioned)."""
    KINDS = ("mesh-uv", "mesh-flat", "plane", "sphere", "disk", "cone")
    CENTRES = [(-2.5, 1.6), (0.0, 2.0), (2.5, 1.6), (-2.5, -1.6), (0.0, -2.0), (0.0, 0.0)]   # the cone at the origin: see the class's text

    def __init__(self, backdrop=False, film=8):
        b = scene.SceneBuilder(film, film)
        b.settings.aa_samples = 1
        mats = [b.lambert(b.spectrum_const(0.1 * (k + 2))) for k in range(7)]
        self.transform = [place(*self.CENTRES[0], rot(2, 30.0), np.diag([1.0, 2.0, 0.5, 1.0])), place(*self.CENTRES[1], rot(0, 20.0)),
                          place(*self.CENTRES[2], rot(1, 15.0)), place(*self.CENTRES[3]), place(*self.CENTRES[4], rot(0, 25.0)),
                          place(*self.CENTRES[5])]
        self.pos_uv, self.faces_uv = grid(4, 0.6, lambda x, y: 0.08 * (x * x + y * y))
        n = np.stack([-0.16 * self.pos_uv[:, 0], -0.16 * self.pos_uv[:, 1], np.ones(len(self.pos_uv))], axis=-1)
        self.nrm_uv = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float32)
        self.uv_uv = np.stack([0.5 * self.pos_uv[:, 0] + 0.5, 0.5 * self.pos_uv[:, 1] + 0.5], axis=-1).astype(np.float32)
        self.pos_flat, self.faces_flat = grid(2, 0.8, lambda x, y: 0.3 * x * y)
        self.emission = b.diffuse_emission(b.smul(b.illuminant_d65(), b.illum(4, 4, 4)))
        self.plane_x, self.plane_y = np.float32([1.5, 0, 0]), np.float32([0, 1.0, 0])
        self.sphere_radius, self.disk_radius, self.cone_radius, self.cone_height = 0.6, 0.7, 1.0, 1.0
        b.add_mesh(self.pos_uv, self.faces_uv, mats[0], normals=self.nrm_uv, uvs=self.uv_uv, transform=self.transform[0])
        b.add_mesh(self.pos_flat, self.faces_flat, mats[1], emission=self.emission, transform=self.transform[1])
        b.add_plane(mats[2], width=1.5, height=1.0, centering=True, transform=self.transform[2])
        b.add_sphere(mats[3], radius=self.sphere_radius, transform=self.transform[3])
        b.add_disk(mats[4], radius=self.disk_radius, transform=self.transform[4])
        b.add_cone(mats[5], radius=self.cone_radius, height=self.cone_height, transform=self.transform[5])
        self.cone_parameters = [float(v) for v in b.tables[-16:-6]]
        if backdrop:
            b.add_mesh([[-20, -20, -2], [20, -20, -2], [20, 20, -2], [-20, 20, -2]], [[0, 1, 2, 3]], mats[6])
            b.set_camera(place(0.0, 0.0) + np.float32([[0, 0, 0, 0.25], [0, 0, 0, -0.5], [0, 0, 0, 9.0], [0, 0, 0, 0]]), local_direction=(0, 0, -1))
        self.camera_origin, self.near, self.far = np.float32([0.25, -0.5, 9.0]), np.float32(1e-6), np.float32(np.inf)
        self.scene = b.build()

    def targets(self, rng, per_entity):
        """world-space points spread over the six entities (local points through the entity's transform)"""
        out = []
        for e, kind in enumerate(self.KINDS):
            a, c = rng.uniform(-1, 1, per_entity), rng.uniform(-1, 1, per_entity)
            if kind == "mesh-uv":
                p = np.stack([0.55 * a, 0.55 * c, 0.08 * ((0.55 * a) ** 2 + (0.55 * c) ** 2)], -1)
            elif kind == "mesh-flat":
                p = np.stack([0.75 * a, 0.75 * c, 0.3 * (0.75 * a) * (0.75 * c)], -1)
            elif kind == "plane":
                p = np.stack([0.7 * a, 0.45 * c, 0 * a], -1)
            elif kind == "sphere":
                r = 0.75 * self.sphere_radius * np.sqrt(np.abs(a))
                p = np.stack([r * np.cos(np.pi * c), r * np.sin(np.pi * c), np.sqrt(self.sphere_radius ** 2 - r * r)], -1)
            elif kind == "disk":
                r = 0.9 * self.disk_radius * np.sqrt(np.abs(a))
                p = np.stack([r * np.cos(np.pi * c), r * np.sin(np.pi * c), 0 * a], -1)
            else:   # the cone's mantle: radius rho at height z = h / 2 - rho h / r, between 0.5 and 0.95 of the base radius
                rho = self.cone_radius * (0.5 + 0.45 * np.abs(a))
                p = np.stack([rho * np.cos(np.pi * c), rho * np.sin(np.pi * c), self.cone_height * (0.5 - rho / self.cone_radius)], -1)
            m = self.transform[e].astype(np.float64)
            out.append(p @ m[:3, :3].T + m[:3, 3])
        return np.concatenate(out)

    def rays(self, n=2000, seed=7, stray=40):
        """n seeded rays from above, aimed at the targets; the last `stray` of them point away from everything"""
        rng = np.random.default_rng(seed)
        per = (n - stray) // 6
        tgt = self.targets(rng, per)
        tgt = np.concatenate([tgt, tgt[: n - stray - len(tgt)]])
        org = tgt + np.stack([rng.uniform(-1.2, 1.2, len(tgt)), rng.uniform(-1.2, 1.2, len(tgt)), rng.uniform(4.0, 6.0, len(tgt))], -1)
        d = tgt - org
        up = np.stack([rng.uniform(-1, 1, stray), rng.uniform(-1, 1, stray), np.ones(stray)], -1)
        org = np.concatenate([org, rng.uniform(-3, 3, (stray, 3)) + [0, 0, 5]]).astype(np.float32)
        d = np.concatenate([d, up])
        return org, (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)

    # the float64 restatement, per kind: (N, Nx, Ny, UV or None) as G's bounded values for the rays `sel` of a batch
    def reference(self, kind, prim, u, v, position):
        e = self.KINDS.index(kind)
        k = len(prim)
        if kind == "mesh-uv":
            f = self.faces_uv[prim]
            N, Nx, Ny, UV, det = G.mesh_point(self.transform[e], self.pos_uv[f], self.nrm_uv[f], self.uv_uv[f], u, v)
            assert (det.v > 0.01).all()   # far from PR_EPSILON: tangentFromUV never falls back to Tangent::frame here
            return N, Nx, Ny, UV
        if kind == "mesh-flat":
            f = self.faces_flat[prim]
            N, Nx, Ny, UV, _ = G.mesh_point(self.transform[e], self.pos_flat[f], None, None, u, v)
            return N, Nx, Ny, UV
        if kind == "plane":
            return tuple(G.plane_point(self.transform[e], None, self.plane_x, self.plane_y, k)) + (None,)
        if kind == "sphere":
            N, Nx, Ny, nz = G.sphere_point(self.transform[e], position)
        elif kind == "disk":
            N, Nx, Ny, nz = G.disk_point(self.transform[e], k)
        else:
            N, Nx, Ny, nz = G.quadric_point(self.transform[e], self.cone_parameters, position)
        assert (nz > 0.1).all(), kind   # frame_duff's sign is decided far from its flip (the counted error of N.z is below 1e-5)
        return N, Nx, Ny, None


@pytest.fixture(scope="module")
def geo():
    return GeometryScene()


@pytest.fixture(scope="module")
def geo_answers(geo):
    """the 2 000 rays of tests 3 and 4 and the device's full answer for them, computed once"""
    org, d = geo.rays()
    g = backend.RenderContext(geo.scene)
    try:
        r = g.traceRaysDevice(dev(org), dev(d), 1e-4, float("inf"), geometry=True)
        return org, d, {f: host(x) for f, x in zip(r._fields, r)}
    finally:
        g.close()


# ---- 2. batch shape ---------------------------------------------------------------------------------------------------------------------------
def test_every_batch_shape_answers_the_leading_slice_of_the_full_batch():
    """A lone lane, one wave +- 1, one block +- 1, a ragged tail; in this order on one context, so that the scratch grows batch by batch
    (geometry is asked for: that is what uses it), and once more after reserveRays(1000), when nothing grows."""
    c = E.case("aimed")
    sc = c.build_scene()
    g = backend.RenderContext(sc)
    full = device_closest(g, geometry=True)(c.org[:1000], c.direction[:1000], c.tmin[:1000], c.tmax[:1000])
    full_any = device_any(g)(c.org[:1000], c.direction[:1000], c.tmin[:1000], c.distance[:1000])
    g.close()
    assert (full[0] != INVALID).sum() > 500
    g = backend.RenderContext(sc)
    try:
        for reserved in (False, True):
            if reserved:
                g.reserveRays(1000)
            for n in (0, 1, 63, 64, 65, 255, 256, 257, 1000):
                got = device_closest(g, geometry=True)(c.org[:n], c.direction[:n], c.tmin[:n], c.tmax[:n])
                assert len(got) == 12
                for field, x, y in zip(backend.RayGeometry._fields, got, full):
                    assert len(x) == n and np.array_equal(x, y[:n], equal_nan=True), (n, reserved, field)
                assert np.array_equal(device_any(g)(c.org[:n], c.direction[:n], c.tmin[:n], c.distance[:n]), full_any[:n]), (n, reserved)
    finally:
        g.close()


# ---- 3. optional outputs ----------------------------------------------------------------------------------------------------------------------
def test_every_output_may_be_null_and_the_others_do_not_change(geo, geo_answers):
    org, d, want = geo_answers
    n = len(org)
    lib = abi.load()
    t_org, t_dir, t_tmin, t_tmax = dev(org), dev(d), dev(np.full(n, 1e-4)), dev(np.full(n, np.inf))
    rays = abi.Rays(n, t_org.data_ptr(), t_dir.data_ptr(), t_tmin.data_ptr(), t_tmax.data_ptr())
    fields = [f for f, _ in abi.Hits._fields_]
    shape = {"position": (n, 3), "normal": (n, 3), "tangent": (n, 3), "bitangent": (n, 3), "uv": (n, 2), "invalid": (1,)}
    integer = ("entity", "prim", "material", "emission", "invalid")
    g = backend.RenderContext(geo.scene)
    try:
        for left_out in [None] + fields:
            out = {f: torch.full(shape.get(f, (n,)), 77, dtype=torch.int32 if f in integer else torch.float32, device="cuda:0") for f in fields}
            out["invalid"].zero_()
            hits = abi.Hits(**{f: (None if f == left_out else out[f].data_ptr()) for f in fields})
            torch.cuda.synchronize()   # the call runs on the scene's own stream: the tensors are ready, and waitForFinish ends it
            abi.check(lib.prgpu_trace_closest_device(g._h, C.byref(rays), C.byref(hits)))
            g.waitForFinish()
            for f in fields:
                if f == left_out:
                    assert (out[f] == (0 if f == "invalid" else 77)).all(), f   # (nothing wrote through another pointer into it either)
                elif f == "invalid":
                    assert int(out[f][0]) == 0
                else:
                    assert np.array_equal(host(out[f]), want[f]), (left_out, f)
    finally:
        g.close()


# ---- 4. geometry against float64 --------------------------------------------------------------------------------------------------------------
def test_the_geometry_of_every_entity_kind_against_the_float64_restatement(geo, geo_answers):
    """normal, tangent and bitangent (and the uv mesh's uv) within the tolerance tests/geometry_point_ref.py counts from the fp32 statement sequence
    of each branch, per ray and component: every fp32 operation adds one rounding u = 2^-24 of its result to the propagated first-order error of its
    operands, and the sum is doubled.  For this scene the count comes out below 1e-5 everywhere (asserted); a scene for which it does not is
    ill-conditioned and is to be replaced, not the tolerance widened.  Everything else is exact."""
    org, d, a = geo_answers
    ent, prim, t = a["entity"], a["prim"], a["t"]
    hit = ent != INVALID
    for e, kind in enumerate(geo.KINDS):   # before anything else: the rays do reach every kind
        assert (ent == e).sum() >= 100, kind
    plane_tri = geo_plane_triangle(geo, org, d, ent)
    assert (plane_tri == 0).sum() >= 20 and (plane_tri == 1).sum() >= 20
    assert (~hit).sum() >= 20
    # position: org + dir * t in fp32, in that order
    position = org + d * t[:, None]
    assert position.dtype == np.float32 and np.array_equal(a["position"][hit], position[hit])
    # ids
    assert np.array_equal(a["material"][hit], ent[hit])   # entity e carries material e
    assert np.array_equal(a["emission"][hit], np.where(ent[hit] == 1, np.uint32(geo.emission), np.uint32(INVALID)))
    assert (prim[hit & (ent >= 2)] == 0).all() and (prim[ent == 0] < len(geo.faces_uv)).all() and (prim[ent == 1] < len(geo.faces_flat)).all()
    # misses
    for f in ("position", "normal", "tangent", "bitangent", "uv"):
        assert (a[f][~hit] == 0).all(), f
    assert (a["material"][~hit] == INVALID).all() and (a["emission"][~hit] == INVALID).all() and (prim[~hit] == INVALID).all()
    # vectors and uv
    worst = 0.0
    for e, kind in enumerate(geo.KINDS):
        sel = ent == e
        N, Nx, Ny, UV = geo.reference(kind, prim[sel], a["u"][sel], a["v"][sel], a["position"][sel])
        for name, w in (("normal", N), ("tangent", Nx), ("bitangent", Ny)):
            tol, err = G.tolerance(w), np.abs(a[name][sel].astype(np.float64) - G.values(w))
            print("%-9s %-9s counted tolerance <= %.3g, largest error %.3g" % (kind, name, tol.max(), err.max()))
            assert tol.max() < 1e-5, (kind, name, tol.max())
            assert (err <= tol).all(), (kind, name, float((err - tol).max()))
            worst = max(worst, tol.max())
        if kind == "mesh-uv":
            tol, err = G.tolerance(UV), np.abs(a["uv"][sel].astype(np.float64) - G.values(UV))
            assert tol.max() < 1e-5 and (err <= tol).all(), (kind, "uv", float(err.max()))
        elif kind == "mesh-flat":
            assert np.array_equal(a["uv"][sel], np.stack([a["u"][sel], a["v"][sel]], -1))
        elif kind == "plane":
            first = (plane_tri == 0)[sel]
            u, v = a["u"][sel], a["v"][sel]
            assert np.array_equal(a["uv"][sel][first], np.stack([u, v], -1)[first])
            assert np.array_equal(a["uv"][sel][~first], np.stack([np.float32(1) - u, np.float32(1) - v], -1)[~first])
        else:
            assert (a["uv"][sel] == 0).all(), kind
    # the quirk that is part of the contract: a quadric's normal is the normal matrix times a unit gradient, not normalised again
    assert np.abs(np.linalg.norm(a["normal"][ent == 5].astype(np.float64), axis=-1) - 1).max() < 1e-5   # (a rotation: it happens to be of unit length here)


def geo_plane_triangle(geo, org, d, ent):
    """0 / 1: which triangle of the plane's quad (v0, v1, v3) / (v2, v3, v1) a ray that hit the plane went through; -1 for the other rays.  In float64,
    from the ray and the quad alone: with s, r the hit's coordinates along the x and the y axis, the first triangle is s + r < 1."""
    m = geo.transform[2].astype(np.float64)
    x, y = m[:3, :3] @ geo.plane_x.astype(np.float64), m[:3, :3] @ geo.plane_y.astype(np.float64)
    p0 = m[:3, :3] @ (-0.5 * geo.plane_x.astype(np.float64) - 0.5 * geo.plane_y.astype(np.float64)) + m[:3, 3]
    nrm = np.cross(x, y)
    o, dd = org.astype(np.float64), d.astype(np.float64)
    with np.errstate(all="ignore"):
        tt = ((p0 - o) @ nrm) / (dd @ nrm)
    q = o + dd * tt[:, None] - p0
    s, r = (q @ x) / (x @ x), (q @ y) / (y @ y)   # (x and y are orthogonal)
    out = np.where(s + r < 1.0, 0, 1)
    # no ray of the batch runs along the diagonal: the device's quad has world-space corners rounded to fp32 (coordinates below 4: the diagonal moves
    # by less than 4 * 2^-24 * 2 = 5e-7 of the quad's unit square), and its triangle test is exact for the corners and the ray it is given
    assert (np.abs(s + r - 1.0)[ent == 2] > 1e-5).all()
    return np.where(ent == 2, out, -1)


# ---- 5. the pipelines commit the same bits ----------------------------------------------------------------------------------------------------
def test_a_render_commits_the_same_bits_to_its_aov_planes(monkeypatch):
    monkeypatch.setenv("PRGPU_MODE", "persistent")
    gs = GeometryScene(backdrop=True, film=32)
    g = backend.RenderContext(gs.scene)
    try:
        g.enableAOVs(abi.AOV_NAMES)
        g.render(1)
        g.waitForFinish()
        samples = g.output()[1]
        planes = {k: g.aov(k) for k in abi.AOV_NAMES}
        one = samples == 1
        assert one.mean() >= 0.9
        view = np.ascontiguousarray(planes["view"][one])
        n = len(view)
        r = g.traceRaysDevice(dev(np.broadcast_to(gs.camera_origin, (n, 3))), dev(view), float(gs.near), float(gs.far), geometry=True)
        a = {f: host(x) for f, x in zip(r._fields, r)}
        assert (a["entity"] != INVALID).all() and len(np.unique(a["entity"])) == 7   # every kind and the backdrop are in view
        for plane, field in (("position", "position"), ("normal", "normal"), ("normal_g", "normal"), ("tangent", "tangent"), ("bitangent", "bitangent")):
            # a plane holds 0 + value, the sum the pipeline makes into its zeroed plane: that turns a -0 (frame_duff's -sign * N.x at N.x = 0) into +0
            assert np.array_equal(planes[plane][one].view(np.uint32), (np.float32(0) + a[field]).view(np.uint32)), plane
        for plane, field in (("entity_id", "entity"), ("material_id", "material"), ("emission_id", "emission")):
            assert np.array_equal(planes[plane][one], a[field].astype(np.float32)), plane
        ent, prim = g.primaryHits()
        assert np.array_equal(ent[one], a["entity"]) and np.array_equal(prim[one], a["prim"])
    finally:
        g.close()


# ---- 6. stream order with torch ---------------------------------------------------------------------------------------------------------------
def test_the_call_is_ordered_with_the_torch_stream_it_is_made_on():
    c = E.case("cube-unit")
    g = backend.RenderContext(c.build_scene())
    try:
        ent, _, _, _, t = g.traceRays(c.org, c.direction, c.tmin, c.tmax)   # test 1's synchronised answers
        hit = ent != INVALID
        assert hit.any()
        want = int(t.view(np.int32).astype(np.int64)[hit].sum())   # the bits of t over the hits: a sum whose order does not matter
        want_occluded = int(g.traceShadowRays(c.org, c.direction, c.tmin, c.distance).sum())
        half_org, half_dir = dev(c.org * np.float32(0.5)), dev(c.direction * np.float32(0.5))
        tmin, tmax, dist = dev(c.tmin), dev(c.tmax), dev(c.distance)
        torch.cuda.synchronize()
        with torch.cuda.stream(torch.cuda.Stream()):
            org, direction = half_org + half_org, half_dir * 2.0   # the rays are made on this stream (x / 2 * 2 is exact), and nothing waits for them
            r = g.traceRaysDevice(org, direction, tmin, tmax)
            got = (r.t.view(torch.int32).to(torch.int64) * (r.entity != -1)).sum()   # reduced by torch on the same stream, at once
            got_occluded = g.traceShadowRaysDevice(org, direction, tmin, dist).sum()
            got, got_occluded = int(got.item()), int(got_occluded.item())
        assert got == want and got_occluded == want_occluded
        assert np.array_equal(g.traceRays(c.org, c.direction, c.tmin, c.tmax)[4], t)   # and the host path after it, back on the scene's own stream
    finally:
        g.close()


# ---- 7. refused rays --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", ["1", "0"])
def test_a_ray_with_a_negative_or_nan_tmin_is_a_miss_and_is_counted(monkeypatch, split):
    monkeypatch.setenv("PRGPU_TRACE_SPLIT", split)
    c = E.case("aimed")
    n = 200
    org, d, tmax, dist = c.org[:n], c.direction[:n], c.tmax[:n], c.distance[:n]
    bad = np.array([0, 63, 64, 199, 100, 128, 7])
    tmin = c.tmin[:n].copy()
    tmin[bad] = [-1.0, np.nan, -1.0, np.nan, -np.inf, -1e-30, np.nan]
    good = np.ones(n, bool)
    good[bad] = False
    g = backend.RenderContext(c.build_scene())
    try:
        clean = device_closest(g)(org, d, c.tmin[:n], tmax)
        clean_any = device_any(g)(org, d, c.tmin[:n], dist)
        assert (clean[0][bad] != INVALID).sum() >= 4 and clean_any[bad].sum() >= 2   # the refused rays would have had something to hit
        ent, prim, u, v, t, invalid = device_closest(g, count_invalid=True)(org, d, tmin, tmax)
        assert invalid.tolist() == [7]
        assert (ent[bad] == INVALID).all() and (prim[bad] == INVALID).all() and (u[bad] == 0).all() and (v[bad] == 0).all() and np.array_equal(t[bad], tmax[bad])
        for x, y in zip((ent, prim, u, v, t), clean):
            assert np.array_equal(x[good], y[good])
        r = g.traceRaysDevice(dev(org), dev(d), dev(tmin), dev(tmax), geometry=True)   # no counter: misses all the same, and no geometry for them
        assert (host(r.entity)[bad] == INVALID).all() and (host(r.normal)[bad] == 0).all() and (host(r.material)[bad] == INVALID).all()
        occ, invalid = g.traceShadowRaysDevice(dev(org), dev(d), dev(tmin), dev(dist), count_invalid=True)
        occ = host(occ)
        assert host(invalid).tolist() == [7] and not occ[bad].any() and np.array_equal(occ[good], clean_any[good])
        with pytest.raises(abi.PrgpuError, match="tmin must not be negative"):   # the host path still refuses the batch
            g.traceRays(org, d, tmin, tmax)
    finally:
        g.close()


# ---- 8. pointers ------------------------------------------------------------------------------------------------------------------------------
def test_a_host_pointer_is_refused_by_field_name_and_the_context_lives_on():
    c = E.case("cube-unit")
    n = 64
    lib = abi.load()
    g = backend.RenderContext(c.build_scene())
    try:
        t = {k: dev(a[:n]) for k, a in (("org", c.org), ("dir", c.direction), ("tmin", c.tmin), ("tmax", c.tmax))}
        out = torch.zeros((n, 3), dtype=torch.float32, device="cuda:0")
        occ = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
        on_host = np.zeros((n, 3), dtype=np.float32)
        torch.cuda.synchronize()
        rays = abi.Rays(n, on_host.ctypes.data, t["dir"].data_ptr(), t["tmin"].data_ptr(), t["tmax"].data_ptr())
        assert lib.prgpu_trace_closest_device(g._h, C.byref(rays), C.byref(abi.Hits())) == EINVAL
        assert b"prgpu_trace_closest_device: org is not device memory" in lib.prgpu_last_error()
        assert lib.prgpu_trace_any_device(g._h, C.byref(rays), C.c_void_p(occ.data_ptr()), None) == EINVAL
        assert b"prgpu_trace_any_device: org is not device memory" in lib.prgpu_last_error()
        rays.org = t["org"].data_ptr()
        assert lib.prgpu_trace_closest_device(g._h, C.byref(rays), C.byref(abi.Hits(position=out.data_ptr(), normal=on_host.ctypes.data))) == EINVAL
        assert b"prgpu_trace_closest_device: normal is not device memory" in lib.prgpu_last_error()
        assert lib.prgpu_trace_any_device(g._h, C.byref(rays), C.c_void_p(on_host.ctypes.data), None) == EINVAL
        assert b"prgpu_trace_any_device: occluded is not device memory" in lib.prgpu_last_error()
        rays.n = 0   # the check comes first in the function: an empty batch does not pass a host pointer either
        assert lib.prgpu_trace_closest_device(g._h, C.byref(rays), C.byref(abi.Hits(uv=on_host.ctypes.data))) == EINVAL and b": uv is not" in lib.prgpu_last_error()
        g.waitForFinish()
        assert (out == 0).all() and (occ == 0).all()   # nothing was enqueued by a refused call
        for x, y in zip(device_closest(g)(c.org, c.direction, c.tmin, c.tmax), g.traceRays(c.org, c.direction, c.tmin, c.tmax)):
            assert np.array_equal(x, y)
    finally:
        g.close()


# ---- 9. the render is undisturbed -------------------------------------------------------------------------------------------------------------
def test_a_batch_between_two_render_calls_leaves_the_frame_as_it_would_have_been():
    sc = scene.cornell_box(48, 40, spp=2)
    a = backend.RenderContext(sc)
    b = backend.RenderContext(sc)
    try:
        a.render(2)
        a.waitForFinish()
        b.render(1)
        rng = np.random.default_rng(5)
        org = (rng.uniform(-0.8, 0.8, (1000, 3)) + [0.0, 0.0, 1.0]).astype(np.float32)   # inside the box, which spans [-1, 1] x [-1, 1] x [0, 2]
        d = rng.normal(size=(1000, 3))
        r = b.traceRaysDevice(dev(org), dev(d / np.linalg.norm(d, axis=-1, keepdims=True)), 1e-3, float("inf"), geometry=True)
        assert (host(r.entity) != INVALID).mean() > 0.75 and np.isfinite(host(r.normal)).all()   # (the box is open towards the camera)
        b.render(1)
        b.waitForFinish()
        for x, y in zip(a.output(), b.output()):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        sa, sb = a.statistics(), b.statistics()
        assert sa == sb, (sa, sb)
    finally:
        a.close()
        b.close()
