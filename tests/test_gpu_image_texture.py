"""Image textures on material parameters (PRGPU_SPEC_IMAGE, include/prgpu.h; device/render.hip image_eval) on the GPU, checked without the CPU
checker, which does not know them.

1 - 4, 6: an orthographic (or perspective) camera looks at one quad under a constant environment of radiance 1, without next event estimation, with the
`uniform` sampler, a single-tap filter and a mono spectral domain: the frame is the albedo under every ray times the frame of the same scene with albedo 1
(same seed, same random numbers).  The ratio must be upsample(c(texel), wavelength) -- restated in numpy float32 (tests/image_files.py) -- of the texel a
float64 restatement of the ray's uv selects.  Tolerance 1e-5 relative + 1e-6 absolute: the two renders differ by about a dozen fp32 roundings (7e-7), any
indexing error is O(0.1).  Bilinear: 1e-4 absolute, derived: the hit's uv carries a few 1e-6 of barycentric rounding, times 4 texels per unit, times a spectrum
range <= 1; a wrong weight or order is O(0.1).
5: every closure reads the image: a Cornell-style scene whose materials take 1 x 1 `closest` images gives the frame, bit for bit, of the same scene with
(refl r g b) of those pixels, in every pipeline."""
import numpy as np
import pytest

import image_files as imf
from pearray_amd import _cabi as abi
from pearray_amd import backend, scene

pytestmark = pytest.mark.gpu
F = np.float32
WAVELENGTHS = (450.0, 550.0, 650.0)
DX, DY = 0.00625, 1.0 / 96        # the quad's offset from the film's grid: keeps every ray off the texel boundaries (checked, not assumed: `clear`)
RNG = np.random.RandomState(5)
SAMPLES = {(4, 4): RNG.randint(0, 256, size=(4, 4, 3)), (5, 3): RNG.randint(0, 256, size=(3, 5, 3))}      # (W, H) -> [H, W, 3]
SAMPLES[(4, 4)][1, 2] = 0          # a black pixel, a white one and one below the linearisation threshold
SAMPLES[(4, 4)][2, 1] = 255
SAMPLES[(5, 3)][0, 4] = (3, 9, 200)


@pytest.fixture(scope="module")
def images(tmp_path_factory):
    """{(W, H, 'png' | 'pfm'): linear rgb [H, W, 3] as prgpu_image_load returns it from a file written here}"""
    d = tmp_path_factory.mktemp("textures")
    out = {}
    for (w, h), s in SAMPLES.items():
        out[(w, h, "png")] = scene.load_image(imf.write(d / ("t%dx%d.png" % (w, h)), imf.encode_png(s, 2, 8)))[0]
        out[(w, h, "pfm")] = scene.load_image(imf.write(d / ("t%dx%d.pfm" % (w, h)), imf.encode_pfm(F(s) / F(300.0), little=(w == 4))))[0]
        assert out[(w, h, "png")].shape == out[(w, h, "pfm")].shape == (h, w, 3)
    for k, rgb in (("red", (200, 30, 40)), ("green", (40, 190, 60)), ("grey", (180, 180, 180)), ("blue", (50, 80, 210)), ("tint", (240, 250, 235))):
        out[k] = scene.load_image(imf.write(d / (k + ".png"), imf.encode_png(np.array(rgb).reshape(1, 1, 3), 2, 8)))[0]
    return out


def spectra_of(b, node, wl):
    """([H, W] fp32 spectra at `wl` of the texels of image node `node` of builder `b`, that of its black texel)"""
    n = b.spectra[node]
    t = np.array(b.tables[n.table_offset:n.table_offset + n.table_count], F).reshape(-1, 4)
    s = imf.upsample32(t[:, :3], wl)
    return s[:-1].reshape(n.rhs, n.lhs), s[-1]


def quad_scene(n, extent, wl, albedo, uv=(0.0, 1.0), plane=False, eye=None):
    """One quad [x0, x0 + 2] x [y0, y0 + 2] in the plane z = 0 (x0 = -1 + DX, y0 = -1 + DY) with texture coordinates `uv` .. from corner to corner -- or a
    plane entity of the same place -- seen on an n x n film by an orthographic camera of extent `extent` at z = 3, or by a perspective camera at `eye` looking
    at the origin.  albedo(b) -> spectrum id.  Returns (scene, u, v, inside): the float64 texture coordinates under every pixel's ray."""
    b = scene.SceneBuilder(n, n)
    s = b.settings
    s.aa_sampler, s.aa_samples, s.filter, s.filter_radius, s.nee = abi.SAMPLER_UNIFORM, 1, abi.FILTER_BLOCK, 0, 0
    s.spectral_start = s.spectral_end = wl
    s.spectral_mono = 1
    b.environment_light(b.spectrum_const(1.0))
    x0, y0 = F(-1 + DX), F(-1 + DY)
    x1, y1 = F(x0 + F(2)), F(y0 + F(2))
    mat = b.lambert(albedo(b))
    if plane:   # its own uv: (along y_axis, along x_axis) in units of the sides, on both triangles (plane.cpp:214)
        T = np.eye(4, dtype=F)
        T[:3, 3] = (x0, y0, 0)
        b.add_plane(mat, width=2.0, height=2.0, transform=T)
    else:
        lo, hi = uv
        b.add_mesh([[x0, y0, 0], [x1, y0, 0], [x1, y1, 0], [x0, y1, 0]], [[0, 1, 2], [0, 2, 3]], mat, uvs=[[lo, lo], [hi, lo], [hi, hi], [lo, hi]])
    gy, gx = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    nx, ny = 2 * (gx / n - 0.5), -2 * (gy / n - 0.5)          # the `uniform` sampler's one ray per pixel (render.hip, camera rays)
    T = np.eye(4, dtype=F)
    if eye is None:
        T[2, 3] = 3.0
        b.set_camera(T, width=extent, height=extent, local_direction=(0, 0, -1), local_right=(1, 0, 0), local_up=(0, 1, 0), ortho=True)
        X, Y = 0.5 * extent * nx, 0.5 * extent * ny
    else:       # perspective.cpp:45-82: d = right (w / 2) nx + up (h / 2) ny + direction from the eye; the plane z = 0
        eye = np.asarray(eye, np.float64)
        fwd = -eye / np.linalg.norm(eye)
        right = np.cross(fwd, [0.0, 0.0, 1.0])
        right /= np.linalg.norm(right)
        up = np.cross(right, fwd)
        T[:3, 3] = eye
        b.set_camera(T, width=extent, height=extent, local_direction=tuple(F(fwd)), local_right=tuple(F(right)), local_up=tuple(F(up)))
        d = (0.5 * extent) * (nx[..., None] * np.float64(F(right)) + ny[..., None] * np.float64(F(up))) + np.float64(F(fwd))
        t = -eye[2] / d[..., 2]
        X, Y = eye[0] + t * d[..., 0], eye[1] + t * d[..., 1]
    fu, fv = (X - np.float64(x0)) / 2, (Y - np.float64(y0)) / 2
    inside = (fu > 0) & (fu < 1) & (fv > 0) & (fv < 1)
    if plane:
        return b, fv, fu, inside
    return b, uv[0] + (uv[1] - uv[0]) * fu, uv[0] + (uv[1] - uv[0]) * fv, inside


def frame(b):
    ctx = backend.RenderContext(b.build(), device=0)
    ctx.render(1)
    ctx.waitForFinish()
    xyz, smp, _ = ctx.output()
    ent = ctx.primaryHits()[0].reshape(ctx.height, ctx.width)
    info = ctx.pipelineInfo()
    ctx.close()
    return np.float64(xyz).reshape(ent.shape + (3,)), ent, info


_REFERENCE = {}


def check(label, got, want, on, rtol=1e-5, atol=1e-6):
    err = np.abs(got - want)[on]
    room = (rtol * np.abs(want) + atol)[on]
    print("%s: %d pixels, worst deviation %.3g (allowed there %.3g), values %.3g .. %.3g" % (label, on.sum(), err.max(), room[err.argmax()], want[on].min(), want[on].max()))
    assert (err <= room).all(), (label, float((err / room).max()))


def textured_over_plain(n, extent, wl, albedo, share=0.3, **kw):
    """(ratio of the textured frame to the albedo-1 frame [n, n], builder of the textured scene, u, v, on): `on` = the quad's pixels, which must be the ones
    the float64 restatement puts inside it"""
    key = (n, extent, wl, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _REFERENCE:
        _REFERENCE[key] = frame(quad_scene(n, extent, wl, lambda b: b.spectrum_const(1.0), **kw)[0])
    ref, ref_ent, _ = _REFERENCE[key]
    b, u, v, inside = quad_scene(n, extent, wl, albedo, **kw)
    tex, ent, info = frame(b)
    assert info["kernel"] == "throughput"
    on = ent == 0
    assert np.array_equal(on, inside) and np.array_equal(ent, ref_ent) and on.sum() > share * n * n
    ch = int(np.argmax(ref[on].mean(0)))
    assert (ref[..., ch][on] > 0).all() and np.array_equal(tex[~on], ref[~on])          # the background does not change
    with np.errstate(all="ignore"):
        return np.where(on, tex[..., ch] / ref[..., ch], 0.0), b, u, v, on


# ---- 1: texel values, closest -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wl", WAVELENGTHS)
@pytest.mark.parametrize("w,h,kind", [(4, 4, "png"), (5, 3, "png"), (5, 3, "pfm"), (4, 4, "pfm")])
def test_closest_texel_values(images, w, h, kind, wl):
    node = {}

    def albedo(b):
        node["id"] = b.image_texture(images[(w, h, kind)], interpolation="closest")
        return node["id"]
    got, b, u, v, on = textured_over_plain(40, 2.5, wl, albedo)          # 32 pixels across the quad
    clear = imf.boundary_distance(u, v, w, h)[on].min()
    print("nearest texel boundary: %.4f texel" % clear)
    assert clear > 0.01                                                 # (the uv of a hit is good to a few 1e-6)
    spectra, black = spectra_of(b, node["id"], wl)
    assert spectra.shape == (h, w) and len(np.unique(spectra)) >= h * w - 1
    check("closest %dx%d %s at %g nm" % (w, h, kind, wl), got, imf.lookup_closest(spectra, black, u, v), on)


# ---- 2: wraps ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wrap", [("black", "black"), ("clamp", "clamp"), ("periodic", "periodic"), ("mirror", "mirror"), ("mirror", "clamp"), ("periodic", "black")])
def test_wrap_modes(images, wrap):
    node = {}

    def albedo(b):
        node["id"] = b.image_texture(images[(5, 3, "png")], interpolation="closest", wrap=wrap)
        return node["id"]
    got, b, u, v, on = textured_over_plain(96, 2.25, 550.0, albedo, uv=(-1.0, 2.0))
    assert u[on].min() < -0.95 and u[on].max() > 1.95 and v[on].min() < -0.95 and v[on].max() > 1.95
    clear = imf.boundary_distance(u, v, 5, 3)[on].min()
    print("nearest texel boundary: %.4f texel" % clear)
    assert clear > 0.003
    spectra, black = spectra_of(b, node["id"], 550.0)
    modes = tuple(scene.SceneBuilder.IMAGE_WRAPS[m] for m in wrap)
    want = imf.lookup_closest(spectra, black, u, v, modes)
    outside = on & ((u < 0) | (u > 1) | (v < 0) | (v > 1))
    assert outside.sum() > 4 * (on & ~outside).sum() and (wrap[0] != "black" or (want[on & (u < 0)] == np.float64(black)).all())
    check("wrap %s / %s" % wrap, got, want, on)


# ---- 3: bilinear ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wl", WAVELENGTHS)
@pytest.mark.parametrize("wrap,uv", [("black", (0.0, 1.0)), ("mirror", (-1.0, 2.0)), ("periodic", (-1.0, 2.0)), ("clamp", (-1.0, 2.0))])
def test_bilinear_blends_the_four_spectra_in_the_stated_order(images, wl, wrap, uv):
    """Worst deviation measured on an MI355X: recorded in DESIGN.md section 2.6."""
    node = {}

    def albedo(b):
        node["id"] = b.image_texture(images[(4, 4, "png")], interpolation="bilinear", wrap=wrap)
        return node["id"]
    got, b, u, v, on = textured_over_plain(40 if uv[0] == 0 else 96, 2.5 if uv[0] == 0 else 2.25, wl, albedo, uv=uv)
    spectra, black = spectra_of(b, node["id"], wl)
    m = scene.SceneBuilder.IMAGE_WRAPS[wrap]
    want = imf.lookup_bilinear(spectra, black, u, v, (m, m))
    assert np.abs(want[on] - imf.lookup_closest(spectra, black, u, v, (m, m))[on]).max() > 0.1          # a closest lookup in its place fails
    check("bilinear %s at %g nm" % (wrap, wl), got, want, on, rtol=0.0, atol=1e-4)


# ---- 4: a plane entity, and an oblique perspective view ------------------------------------------------------------------------------------------
def test_a_plane_entity_uses_its_own_uv_on_both_triangles(images):
    node = {}

    def albedo(b):
        node["id"] = b.image_texture(images[(5, 3, "png")], interpolation="closest")
        return node["id"]
    got, b, u, v, on = textured_over_plain(40, 2.5, 550.0, albedo, plane=True)
    assert (on & (u + v < 0.9)).sum() > 300 and (on & (u + v > 1.1)).sum() > 300            # both triangles of the quad
    clear = imf.boundary_distance(u, v, 5, 3)[on].min()
    print("nearest texel boundary: %.4f texel" % clear)
    assert clear > 0.003
    spectra, black = spectra_of(b, node["id"], 550.0)
    check("plane entity", got, imf.lookup_closest(spectra, black, u, v), on)


def test_an_oblique_perspective_view(images):
    node = {}

    def albedo(b):
        node["id"] = b.image_texture(images[(5, 3, "png")], interpolation="closest", wrap="periodic")
        return node["id"]
    got, b, u, v, on = textured_over_plain(96, 0.6, 550.0, albedo, share=0.25, uv=(-1.0, 2.0), eye=(2.1, -3.3, 2.6))
    undecided = on & (imf.boundary_distance(u, v, 5, 3) < 1e-3)
    print("undecided: %.3f %% of %d pixels" % (100.0 * undecided.sum() / on.sum(), on.sum()))
    assert undecided.sum() <= 0.02 * on.sum()
    spectra, black = spectra_of(b, node["id"], 550.0)
    check("oblique view", got, imf.lookup_closest(spectra, black, u, v, (2, 2)), on & ~undecided)


# ---- 5: every closure reads the image, bit for bit -------------------------------------------------------------------------------------------------
PIPELINES = [dict(PRGPU_MODE="persistent", PRGPU_PP_KERNEL="throughput"), dict(PRGPU_MODE="persistent", PRGPU_PP_KERNEL="latency"), dict(PRGPU_MODE="lockstep"),
             dict(PRGPU_MODE="streaming")]


def cornell(images, textured):
    """A box of Lambert walls under an area light with a rough conductor, a principled and a glass card in it; every colour is a 1 x 1 `closest` image, or
    (refl r g b) of the pixel prgpu_image_load returned for it"""
    b = scene.SceneBuilder(64, 64)
    b.settings.aa_samples = 1
    b.settings.max_ray_depth = 8

    def colour(name):   # wrap 'clamp': the box's corners are hit at u = 1 exactly (the floor's edge under the right wall lies on the film's diagonal), which `black` puts outside
        return b.image_texture(images[name], interpolation="closest", wrap="clamp") if textured else b.refl(*[float(c) for c in images[name][0, 0]])
    T = np.eye(4, dtype=F)
    T[:3, 3] = (0, -3.4, 1)
    b.set_camera(T, width=0.8, height=0.8, local_direction=(0, 1, 0), local_right=(1, 0, 0), local_up=(0, 0, 1))
    UV = [[0, 0], [1, 0], [1, 1], [0, 1]]

    def quad(p, mat, emission=None):
        b.add_mesh(p, [[0, 1, 2], [0, 2, 3]], mat, uvs=UV, emission=emission)
    grey, red, green = b.lambert(colour("grey")), b.lambert(colour("red")), b.lambert(colour("green"))
    quad([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], grey)              # floor
    quad([[-1, -1, 2], [-1, 1, 2], [1, 1, 2], [1, -1, 2]], grey)              # ceiling
    quad([[-1, 1, 0], [1, 1, 0], [1, 1, 2], [-1, 1, 2]], grey)                # back
    quad([[-1, -1, 0], [-1, 1, 0], [-1, 1, 2], [-1, -1, 2]], red)
    quad([[1, -1, 0], [1, -1, 2], [1, 1, 2], [1, 1, 0]], green)
    quad([[-0.3, -0.3, 1.98], [0.3, -0.3, 1.98], [0.3, 0.3, 1.98], [-0.3, 0.3, 1.98]], grey, emission=b.diffuse_emission(b.spectrum_const(12.0)))
    metal = b.rough_conductor(0.25, specularity=colour("tint"))
    disney = b.principled(base=colour("blue"), roughness=0.4, metallic=0.3, clearcoat=0.5)
    glass = b.dielectric(b.spectrum_const(1.5), transmission=colour("tint"))
    quad([[-0.8, 0.6, 0.1], [-0.2, 0.8, 0.1], [-0.2, 0.8, 1.1], [-0.8, 0.6, 1.1]], metal)
    quad([[0.2, 0.8, 0.1], [0.8, 0.5, 0.1], [0.8, 0.5, 1.0], [0.2, 0.8, 1.0]], disney)
    quad([[-0.4, -0.2, 0.2], [0.4, -0.2, 0.2], [0.4, -0.1, 0.9], [-0.4, -0.1, 0.9]], glass)
    return b.build()


def test_every_closure_reads_the_image_bit_for_bit_in_every_pipeline(monkeypatch, images):
    """The second leg asks for the persistent kernel's latency organisation: the shipped build holds it for variant rows 1 and 4 only (Makefile, PL_VARIANTS), so
    an image scene (top row) falls back to the throughput kernel there; a build with `make PL_VARIANTS="1 2 3 4 5"` runs device/path_wave.inl with images."""
    ran = []
    for env in PIPELINES:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        out = []
        for textured in (True, False):
            ctx = backend.RenderContext(cornell(images, textured), device=0)
            ctx.render(1)
            ctx.waitForFinish()
            out.append((ctx.output(), ctx.statistics(), ctx.pipelineInfo()))
            ctx.close()
        for k in env:
            monkeypatch.delenv(k)
        (a, sa, ia), (r, sr, ir) = out
        ran.append((ia["mode"], ia["kernel"], ir["kernel"]))
        assert all(np.array_equal(x, y) for x, y in zip(a, r)), env
        assert sa == sr and sa["shadow_rays"] > 1000 and sa["bounce_rays"] > 3000, (env, sa, sr)
        assert np.isfinite(a[0]).all() and a[0].max() > 0
    print("pipelines:", ran)
    assert len({m for m, _, _ in ran}) == 3 and ran[0][1] == "throughput"


# ---- 6: an image behind a checkerboard, and a checkerboard of two images -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["image_and_constant", "two_images", "nested"])
def test_an_image_behind_a_checkerboard(images, case):
    node = {}

    def albedo(b):
        node["a"] = b.image_texture(images[(5, 3, "png")], interpolation="closest")
        node["b"] = b.image_texture(images[(4, 4, "pfm")], interpolation="closest")
        node["c"] = b.spectrum_const(0.25)
        if case == "image_and_constant":
            return b.checkerboard(node["a"], node["c"], 3.0)
        if case == "two_images":
            return b.checkerboard(node["a"], node["b"], 3.0)
        return b.checkerboard(b.checkerboard(node["b"], node["c"], 3.0), node["a"], 3.0, 2.0)
    got, b, u, v, on = textured_over_plain(40, 2.5, 550.0, albedo)
    sa, ba = spectra_of(b, node["a"], 550.0)
    sb, bb = spectra_of(b, node["b"], 550.0)
    va, vb, vc = imf.lookup_closest(sa, ba, u, v), imf.lookup_closest(sb, bb, u, v), np.full(u.shape, np.float64(F(0.25)))
    cell = lambda su, sv: (np.floor(u * su) + np.floor(v * sv)) % 2 == 0          # CheckerboardNode.cpp:26-48: the even cells take the second operand
    clear = min(imf.boundary_distance(u, v, 5, 3)[on].min(), imf.boundary_distance(u, v, 4, 4)[on].min(), imf.boundary_distance(u, 1 - v, 3, 3)[on].min(),
                imf.boundary_distance(u, 1 - v, 3, 2)[on].min())
    assert clear > 0.005
    if case == "image_and_constant":
        want = np.where(cell(3, 3), vc, va)
    elif case == "two_images":
        want = np.where(cell(3, 3), vb, va)
    else:
        want = np.where(cell(3, 2), va, np.where(cell(3, 3), vc, vb))
    assert 0.3 < cell(3, 3)[on].mean() < 0.7
    check("checkerboard: " + case, got, want, on)
