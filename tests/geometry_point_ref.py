"""IEntity::provideGeometryPoint of the five entity kinds restated in float64, with the bound an fp32 evaluation of the same statements is held to.

Written from the reference's text, not from the device's geometry_point:
    mesh     entities/mesh.cpp:205-250 (provideGeometryPointLocal, then normalMatrix() * {N, Nx, Ny}, each normalised), Face::interpolateNormals /
             interpolateUVs, Face::tangentFromUV (geometry/Face.h:80-98), and for a mesh without normals Embree's dPdu = v1 - v0, dPdv = v2 - v0
    plane    entities/plane.cpp:206-238: N = normalMatrix() * normal, Nx = linear * xAxis, Ny = linear * yAxis, each normalised; UV = query.UV
    sphere   entities/sphere.cpp:126-141: N = (P - transform * 0).normalized(), Tangent::frame
    disk     entities/disk.cpp:89-102: N = (normalMatrix() * (0, 0, 1)).normalized(), Tangent::frame
    quadric  entities/quadric.cpp:95-108: N = normalMatrix() * Quadric::normal(parameters, invTransform() * P) -- not normalised again --, Tangent::frame
    Tangent::frame = frame_duff (math/Tangent.h:50-73), both tangents normalised; normalMatrix() = linear().inverse().transpose().

THE BOUND.  Every value is a pair (float64 value, bound on the error of its fp32 evaluation), carried through the statements by class B: an fp32
operation on operands a, b with errors ea, eb returns a result whose error is at most the propagated first-order error (|b| ea + |a| eb for a product,
ea + eb for a sum, ...) plus ONE rounding u |result|, u = 2^-24 -- the count of the fp32 statement sequence, taken operation by operation instead
of in closed form, because the conditioning differs per ray (how far the interpolated normal is from unit length, how much of the tangent the
Gram-Schmidt step removes, which way the non-uniform scale stretches the vector).  The inputs -- vertex data, transform entries, quadric parameters,
and a ray's (u, v, position) as the device reports them -- are fp32 numbers and carry no error.  As tests/exact_disk.py does with its margins, the
first-order count is DOUBLED before anything is held to it (tolerance()).  The float64 arithmetic of the values themselves rounds at 2^-53, nine
orders below.  The one discontinuity, frame_duff's copysign(1, N.z), is the caller's to keep away from: frame() reports |N.z| so that a test can assert
the scene never comes near it."""
import numpy as np

U = 2.0 ** -24


class B:
    """float64 value(s) `v` with a bound `e` on the error of their fp32 evaluation"""
    __array_ufunc__ = None   # numpy arrays leave the arithmetic to this class

    def __init__(self, v, e=None):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.zeros_like(self.v) if e is None else np.asarray(e, dtype=np.float64)

    @staticmethod
    def lift(x):
        return x if isinstance(x, B) else B(np.float64(np.float32(x)))   # a literal of the statement: an fp32 constant

    @staticmethod
    def rounded(v, e):
        return B(v, e + U * np.abs(v))

    def __add__(self, o):
        o = B.lift(o)
        return B.rounded(self.v + o.v, self.e + o.e)

    __radd__ = __add__

    def __sub__(self, o):
        o = B.lift(o)
        return B.rounded(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return B.lift(o) - self

    def __mul__(self, o):
        o = B.lift(o)
        return B.rounded(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = B.lift(o)
        v = self.v / o.v
        return B.rounded(v, (self.e + np.abs(v) * o.e) / np.abs(o.v))

    def __rtruediv__(self, o):
        return B.lift(o) / self

    def __neg__(self):
        return B(-self.v, self.e)

    def sqrt(self):
        v = np.sqrt(self.v)
        return B.rounded(v, self.e / (2.0 * v))


def vec(a):
    """[..., 3] fp32 numbers -> a 3-vector of B"""
    a = np.asarray(a, dtype=np.float32).astype(np.float64)
    return [B(a[..., 0]), B(a[..., 1]), B(a[..., 2])]


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def sub(a, b):
    return [a[k] - b[k] for k in range(3)]


def scaled(a, s):
    return [a[k] * s for k in range(3)]


def normalized(a):
    n = dot(a, a).sqrt()
    return [a[k] / n for k in range(3)]


def mat3(m, a):
    """m: 3 x 3 of B (or of fp32 numbers), row-major"""
    return [(m[3 * r] * a[0] + m[3 * r + 1] * a[1]) + m[3 * r + 2] * a[2] for r in range(3)]


def linear(transform):
    t = np.asarray(transform, dtype=np.float32).astype(np.float64).reshape(4, 4)
    return [B(t[r, c]) for r in range(3) for c in range(3)], [B(t[r, 3]) for r in range(3)]


def normal_matrix(transform, normalised_after=True):
    """linear().inverse().transpose(): cofactors over the determinant, as Eigen inverts a 3 x 3.  normalised_after: the product with this matrix
    is normalised before anything else is done with it, so an error of the determinant -- one factor common to all nine entries -- cancels
    exactly and is not counted (the division's own rounding is); the quadric's normal is NOT normalised after and counts it."""
    (a, b, c, d, e, f, g, h, i), _ = linear(transform)
    cof = [e * i - f * h, f * g - d * i, d * h - e * g, c * h - b * i, a * i - c * g, b * g - a * h, b * f - c * e, c * d - a * f, a * e - b * d]
    det = (a * cof[0] + b * cof[1]) + c * cof[2]
    if normalised_after:
        det = B(det.v)
    return [k / det for k in cof]


def frame(N):
    """Tangent::frame: frame_duff, both tangents normalised.  Also returns |N.z| (the sign below flips at 0)."""
    sign = np.copysign(1.0, N[2].v)
    a = -1.0 / (B(sign) + N[2])
    b = N[0] * N[1] * a
    Nx = [1.0 + B(sign) * N[0] * N[0] * a, B(sign) * b, -(B(sign) * N[0])]
    Ny = [b, B(sign) + N[1] * N[1] * a, -N[1]]
    return normalized(Nx), normalized(Ny), np.abs(N[2].v)


def mesh_point(transform, p, n, uv, u, v):
    """p, n, uv: the hit triangles' vertex positions [k, 3, 3], normals (None: a mesh without) and uvs [k, 3, 2] (None: without); u, v: [k].
    Returns N, Nx, Ny, UV (B vectors) and the determinant of tangentFromUV (None without uvs: the caller asserts it is far from PR_EPSILON)."""
    u, v = B(np.asarray(u, np.float32)), B(np.asarray(v, np.float32))
    P = [vec(np.asarray(p)[:, k]) for k in range(3)]
    w = 1.0 - u - v
    det = None
    if uv is not None:
        t = np.asarray(uv, dtype=np.float32).astype(np.float64)
        T = [[B(t[:, k, 0]), B(t[:, k, 1])] for k in range(3)]
        UV = [(T[1][c] * u + T[2][c] * v) + T[0][c] * w for c in range(2)]
    else:
        UV = [u, v]
    if n is not None:
        Nv = [vec(np.asarray(n)[:, k]) for k in range(3)]
        N = [(Nv[1][c] * u + Nv[2][c] * v) + Nv[0][c] * w for c in range(3)]
        if uv is not None:   # Face::tangentFromUV
            dp1, dp2 = sub(P[1], P[0]), sub(P[2], P[0])
            du1, dv1, du2, dv2 = T[1][0] - T[0][0], T[1][1] - T[0][1], T[2][0] - T[0][0], T[2][1] - T[0][1]
            det = dv2 * du1 - dv1 * du2
            Nx = [(dp1[c] * dv2 - dp2[c] * dv1) / det for c in range(3)]
            Nx = sub(Nx, scaled(N, dot(N, Nx)))
            Nx = normalized(Nx)
            Ny = cross(N, Nx)
        else:   # Tangent::unnormalized_frame
            sign = np.copysign(1.0, N[2].v)
            a = -1.0 / (B(sign) + N[2])
            b = N[0] * N[1] * a
            Nx = [1.0 + B(sign) * N[0] * N[0] * a, B(sign) * b, -(B(sign) * N[0])]
            Ny = [b, B(sign) + N[1] * N[1] * a, -N[1]]
    else:
        Nx, Ny = sub(P[1], P[0]), sub(P[2], P[0])
        N = cross(Nx, Ny)
    nm = normal_matrix(transform)
    return normalized(mat3(nm, N)), normalized(mat3(nm, Nx)), normalized(mat3(nm, Ny)), UV, det


def plane_point(transform, origin, x_axis, y_axis, k):
    """the plane's cached frame, the same for each of k hits"""
    lin, _ = linear(transform)
    x, y = vec(x_axis), vec(y_axis)
    N = normalized(mat3(normal_matrix(transform), normalized(cross(x, y))))
    out = [N, normalized(mat3(lin, x)), normalized(mat3(lin, y))]
    return [[B(np.full(k, c.v), np.full(k, c.e)) for c in w] for w in out]


def sphere_point(transform, position):
    _, t = linear(transform)   # transform * (0, 0, 0)
    N = normalized(sub(vec(position), t))
    Nx, Ny, nz = frame(N)
    return N, Nx, Ny, nz


def disk_point(transform, k):
    N = normalized(mat3(normal_matrix(transform), [B(0.0), B(0.0), B(1.0)]))
    Nx, Ny, nz = frame(N)
    return [[B(np.full(k, c.v), np.full(k, c.e)) for c in w] for w in (N, Nx, Ny)] + [nz]


def quadric_point(transform, parameters, position):
    """Quadric::gradient (geometry/Quadric.h:91-110) at invTransform() * P"""
    nm = normal_matrix(transform, normalised_after=False)
    _, t = linear(transform)
    P = vec(position)
    inv = [nm[3 * c + r] for r in range(3) for c in range(3)]   # linear^-1 = normalMatrix^T
    it = [-((inv[3 * r] * t[0] + inv[3 * r + 1] * t[1]) + inv[3 * r + 2] * t[2]) for r in range(3)]   # Transformf::inverse: -linear^-1 * translation
    L = [((inv[3 * r] * P[0] + inv[3 * r + 1] * P[1]) + inv[3 * r + 2] * P[2]) + it[r] for r in range(3)]
    A, Bq, Cq, D, E, F, G, H, I = [B(np.float64(np.float32(q))) for q in parameters[:9]]
    grad = [((2.0 * A * L[0] + D * L[1]) + E * L[2]) + G, ((D * L[0] + 2.0 * Bq * L[1]) + F * L[2]) + H, ((E * L[0] + F * L[1]) + 2.0 * Cq * L[2]) + I]
    N = mat3(nm, normalized(grad))
    Nx, Ny, nz = frame(N)
    return N, Nx, Ny, nz


def values(w):
    return np.stack([c.v for c in w], axis=-1)


def tolerance(w):
    """per component: the first-order count, doubled"""
    return 2.0 * np.stack([c.e for c in w], axis=-1)
