"""Shared by tests/test_ao_loader.py and tests/test_gpu_ao.py: the analytic occlusion probability of a rectangle, restatements of the
integrator's arithmetic in numpy, and small scenes."""
import numpy as np

from pearray_amd import _cabi as abi
from pearray_amd import scene

PR_EPSILON = np.float32(1.1920928955078125e-7)   # config/Constants.inl:4: the occlusion rays' MinT


def rect_solid_angle(point, x0, x1, y0, y1, z):
    """Solid angle (float64) of the axis-aligned rectangle [x0, x1] x [y0, y1] in the plane at height `z`, seen from `point` ([..., 3]) below or
    above it: the sum of the four signed corner terms G(x, y) = atan(x y / (h sqrt(x^2 + y^2 + h^2))) with the corners taken relative to
    the point's foot on the plane and h its distance to it.  Under the centre of a square of half side a this is 4 asin(a^2 / (a^2 + h^2))."""
    p = np.asarray(point, dtype=np.float64)
    h = np.abs(z - p[..., 2])

    def G(x, y):
        return np.arctan2(x * y, h * np.sqrt(x * x + y * y + h * h))

    ax0, ax1, ay0, ay1 = x0 - p[..., 0], x1 - p[..., 0], y0 - p[..., 1], y1 - p[..., 1]
    return (G(ax1, ay1) - G(ax0, ay1)) - (G(ax1, ay0) - G(ax0, ay0))


def look_at(eye, target, up=(0, 0, 1)):
    eye, target = np.asarray(eye, dtype=np.float64), np.asarray(target, dtype=np.float64)
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    T = np.eye(4, dtype=np.float32)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = right, np.cross(right, fwd), fwd, eye
    return T


def builder(width, height, n, eye, target, up=(0, 0, 1), sampler=abi.SAMPLER_RANDOM, filt=abi.FILTER_BLOCK, radius=0, spp=64, fov=0.8):
    """A light-less scene with the AO integrator at `n` samples (0: `direct`); returns (builder, white material)."""
    b = scene.SceneBuilder(width, height)
    s = b.settings
    s.aa_sampler, s.aa_samples, s.filter, s.filter_radius, s.mapper = sampler, spp, filt, radius, abi.MAPPER_RANDOM
    b.set_camera(look_at(eye, target, up), width=fov, height=fov * height / width)
    if n:
        b.ambient_occlusion(n)
    return b, b.lambert(b.spectrum_const(0.8))


def quad(b, mat, corners, toward=None, away=None, **kw):
    """Two triangles over four corners given in order around the quad, with the face normal as vertex normals: the integrator takes its
    hemisphere around the shading normal as the entity gives it (no flip towards the viewer), and a mesh without normals gets the triangle's
    edges as its tangent frame (mesh.cpp:205-250), which is not orthonormal.  toward / away: a point the normal faces / faces away from."""
    c = np.asarray(corners, dtype=np.float64)
    n = np.cross(c[1] - c[0], c[3] - c[0])
    n /= np.linalg.norm(n)
    if (toward is not None and np.dot(np.asarray(toward) - c[0], n) < 0) or (away is not None and np.dot(np.asarray(away) - c[0], n) > 0):
        n = -n
    return b.add_mesh(c.astype(np.float32), [[0, 1, 2], [0, 2, 3]], mat, normals=np.tile(n.astype(np.float32), (4, 1)), **kw)


def box_quads(lo, hi):
    """The six faces of an axis-aligned box as corner lists."""
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    return [[[x0, y0, z0], [x1, y0, z0], [x1, y1, z0], [x0, y1, z0]], [[x0, y0, z1], [x1, y0, z1], [x1, y1, z1], [x0, y1, z1]],
            [[x0, y0, z0], [x1, y0, z0], [x1, y0, z1], [x0, y0, z1]], [[x0, y1, z0], [x1, y1, z0], [x1, y1, z1], [x0, y1, z1]],
            [[x0, y0, z0], [x0, y1, z0], [x0, y1, z1], [x0, y0, z1]], [[x1, y0, z0], [x1, y1, z0], [x1, y1, z1], [x1, y0, z1]]]


def world_triangles(sc):
    """(triangles float64 [n, 3, 3], entity, primitive) of a scene whose entities are untransformed meshes."""
    d = sc.desc
    pos = np.ctypeslib.as_array(d.positions, shape=(d.n_vertices * 3,)).reshape(-1, 3).astype(np.float64)
    idx = np.ctypeslib.as_array(d.indices, shape=(d.n_triangles * 3,)).reshape(-1, 3)
    ent, prim = np.zeros(d.n_triangles, np.int64), np.zeros(d.n_triangles, np.int64)
    for e in range(d.n_entities):
        E = d.entities[e]
        assert E.kind == abi.ENTITY_MESH and np.array_equal(np.asarray(list(E.transform), dtype=np.float32).reshape(4, 4), np.eye(4, dtype=np.float32))
        ent[E.first_tri:E.first_tri + E.n_tris] = e
        prim[E.first_tri:E.first_tri + E.n_tris] = np.arange(E.n_tris)
    return pos[idx], ent, prim


F = np.float32


def uniform_hemi32(u1, u2, sincos=None):
    """Sampling::hemi (base/math/Sampling.h:23-29) in float32; sincos: the (sin, cos) of 2 pi u2 to use instead of numpy's."""
    u1, u2 = np.asarray(u1, dtype=F), np.asarray(u2, dtype=F)
    sin_theta = np.sqrt(np.maximum(F(0), F(1) - u1 * u1))
    phi = F(2) * F(np.pi) * u2
    s, c = (np.sin(phi), np.cos(phi)) if sincos is None else sincos
    return np.stack([sin_theta * c.astype(F), sin_theta * s.astype(F), u1], axis=-1)


def from_tangent_space32(N, Nx, Ny, v):
    """Tangent::fromTangentSpace (base/math/Tangent.h:9-14) in float32, normalised as there."""
    w = (N * v[..., 2:3] + Ny * v[..., 1:2]) + Nx * v[..., 0:1]
    return (w / np.sqrt(((w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1]) + w[..., 2] * w[..., 2]))[..., None]).astype(F)


def safe_position32(P, d, N):
    """Transform::safePosition (base/math/Transform.h:13-32) in float32: offset along the normal on the ray's side, then one float outwards."""
    P, d, N = (np.asarray(a, dtype=F) for a in (P, d, N))
    k = (np.abs(N[..., 0]) * F(0.0001) + np.abs(N[..., 1]) * F(0.0001)) + np.abs(N[..., 2]) * F(0.0001)
    off = N * k[..., None]
    neg = ((d[..., 0] * N[..., 0] + d[..., 1] * N[..., 1]) + d[..., 2] * N[..., 2]) < 0
    off = np.where(neg[..., None], -off, off).astype(F)
    p = (P + off).astype(F)
    return np.where(off > 0, np.nextafter(p, F(np.inf)), np.where(off < 0, np.nextafter(p, F(-np.inf)), p)).astype(F)


def sincos_2pi32(u):
    """The backend's shared fp32 sin / cos of 2 pi u (pr_device.h, pr_sincos_2pi: exact quadrant reduction, minimax polynomials), restated
    operation for operation: returns (sin, cos)."""
    u = np.asarray(u, dtype=F)
    k = np.floor(u * F(4) + F(0.5))
    x = F(6.28318530717958647692) * (u - F(0.25) * k)
    x2 = x * x
    ps = (F(-1.9515295891e-4) * x2 + F(8.3321608736e-3)) * x2 + F(-1.6666654611e-1)
    sn = (ps * x2) * x + x
    pc = (F(2.443315711809948e-5) * x2 + F(-1.388731625493765e-3)) * x2 + F(4.166664568298827e-2)
    cs = (pc * x2) * x2 + (F(1) - F(0.5) * x2)
    q = k.astype(np.int64) & 3
    s = np.where(q == 0, sn, np.where(q == 1, cs, np.where(q == 2, -sn, -cs)))
    c = np.where(q == 0, cs, np.where(q == 1, -sn, np.where(q == 2, -cs, sn)))
    return s.astype(F), c.astype(F)
