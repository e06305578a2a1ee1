"""`(texture :name N :file F :type T ...)` blocks of the .prc loader (parser/TextureParser.cpp) and SceneBuilder.image_texture: the
PRGPU_SPEC_IMAGE node they yield (include/prgpu.h), its texel table, the option spellings, and the refusals.  The images are written
here (tests/image_files.py).  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from pearray_amd import _cabi as abi
from pearray_amd import scene

import image_files as imf

HEAD = """(scene :render_width 8 :render_height 8 :camera 'cam'
  (camera :name 'cam' :type 'standard' :position [0, 0, 3])
  (mesh :name 'quad' (attribute :type 'p' [-1,-1,0],[1,-1,0],[1,1,0],[-1,1,0]) (attribute :type 't' [0,0],[1,0],[1,1],[0,1]) (faces [0,1,2],[0,2,3]))
"""
SAMPLES = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [7, 7, 7]],
                    [[10, 20, 30], [200, 100, 50], [0, 0, 0], [128, 128, 128], [255, 0, 0]],
                    [[1, 2, 3], [250, 251, 252], [90, 80, 70], [7, 7, 7], [60, 160, 220]]])     # 5 x 3, two colours twice


def load(tmp_path, body, **kw):
    sc = scene.PrcScene(source=HEAD + body + "\n)", include_dir=str(tmp_path), **kw)
    sc.warnings = [w for w in sc.warnings if "the scene has no entities" not in w]      # (most scenes here declare no entity)
    return sc


def refused(tmp_path, body):
    with pytest.raises(abi.PrgpuError) as e:
        load(tmp_path, body)
    return e.value.args[1], e.value.args[0]


@pytest.fixture
def png(tmp_path):
    imf.write(tmp_path / "tex.png", imf.encode_png(SAMPLES, 2, 8))
    return tmp_path


def image_nodes(d):
    return [d.spectra[i] for i in range(d.n_spectra) if d.spectra[i].kind == abi.SPEC_IMAGE]


def tables(d):
    return np.ctypeslib.as_array(d.spectral_tables, shape=(d.n_spectral_table_values,)).copy()


def test_a_texture_block_and_a_material_yield_an_image_node(png):
    sc = load(png, """(texture :name 'tex' :file 'tex.png' :type 'color' :interpolation 'closest' :wrap ['periodic', 'mirror'])
        (material :name 'm' :type 'diffuse' :albedo (spectrum :start 400 :end 700 0.1 0.5 0.9))
        (material :name 't' :type 'diffuse' :albedo 'tex')
        (entity :name 'q' :type 'mesh' :mesh 'quad' :materials 't')""")
    assert sc.warnings == []
    d = sc.desc
    n = d.spectra[d.materials[1].albedo]
    assert n.kind == abi.SPEC_IMAGE == 7 and (n.lhs, n.rhs) == (5, 3) and list(n.p)[:3] == [0.0, 2.0, 3.0]
    assert n.table_offset % 4 == 0 and n.table_count == 4 * (5 * 3 + 1) and n.table_offset + n.table_count <= d.n_spectral_table_values
    # the texels: rgb_to_coeffs of the linearised pixels, rows top-down, the fourth float 0, the black texel last
    rgb, _, _ = scene.load_image(str(png / "tex.png"))
    texels = tables(d)[n.table_offset:n.table_offset + n.table_count].reshape(-1, 4)
    want = np.array([scene.rgb_to_coeffs(p) for p in rgb.reshape(-1, 3)] + [scene.rgb_to_coeffs((0, 0, 0))], np.float32)
    assert np.array_equal(texels[:, :3], want) and not texels[:, 3].any()
    assert np.array_equal(texels[-1, :3], texels[7, :3])            # pixel (1, 2) is black too
    assert not np.array_equal(texels[0, :3], texels[1, :3])


def test_the_path_is_relative_to_the_file_that_holds_the_block(tmp_path):
    os.makedirs(tmp_path / "sub" / "img")
    imf.write(tmp_path / "sub" / "img" / "g.pfm", imf.encode_pfm(np.full((2, 3), 0.25, np.float32)))
    imf.write(tmp_path / "sub" / "inc.prc", b"(texture :name 'g' :filename 'img/g.pfm' :type 'grayscale' :interpolation 'bi')\n")
    imf.write(tmp_path / "scene.prc", (HEAD + "(include 'sub/inc.prc') (material :name 't' :type 'mirror' :specularity 'g'))").encode())
    sc = scene.PrcScene(path=str(tmp_path / "scene.prc"))
    n, = image_nodes(sc.desc)
    assert (n.lhs, n.rhs) == (3, 2) and list(n.p)[:3] == [1.0, 0.0, 0.0] and sc.desc.materials[0].albedo == sc.desc.n_spectra - 1
    texels = tables(sc.desc)[n.table_offset:n.table_offset + n.table_count].reshape(-1, 4)
    assert np.array_equal(texels[0, :3], np.float32(scene.rgb_to_coeffs((0.25, 0.25, 0.25))))    # PFM: not linearised


@pytest.mark.parametrize("wrap,want", [("'black'", (0, 0)), ("'clamp'", (1, 1)), ("'Periodic'", (2, 2)), ("'MIRROR'", (3, 3)), ("'repeat'", (0, 0)),
                                       ("['clamp']", (1, 0)), ("['mirror', 'clamp']", (3, 1)), ("['clamp', 'nonsense', 'mirror']", (1, 0)),
                                       ("['periodic', 'periodic', 'clamp', 'clamp']", (2, 2)), (None, (0, 0)), ("3", (0, 0))])
def test_every_wrap_spelling(png, wrap, want):
    sc = load(png, "(texture :name 'tex' :file 'tex.png' :type 'color' :interpolation 'bilinear'%s)" % ("" if wrap is None else " :wrap " + wrap))
    n, = image_nodes(sc.desc)
    assert (n.p[1], n.p[2]) == want and sc.warnings == []


@pytest.mark.parametrize("interp,want,warns", [("'closest'", 0, None), ("'bi'", 1, None), ("'bilinear'", 1, None), ("'Bilinear'", 1, None),
                                               ("'bicubic'", 1, "bicubic"), (None, 1, "smart bicubic"), ("'cubic'", 1, "smart bicubic")])
def test_every_interpolation_spelling(png, interp, want, warns):
    sc = load(png, "(texture :name 'tex' :file 'tex.png' :type 'spectral' :mip 'trilinear' :anisotropic 8 :blur 0%s)" % ("" if interp is None else " :interpolation " + interp))
    n, = image_nodes(sc.desc)
    assert n.p[0] == want
    if warns is None:
        assert sc.warnings == []
    else:
        assert len(sc.warnings) == 1 and warns in sc.warnings[0] and "bilinear is used" in sc.warnings[0]


def test_a_missing_type_means_color_with_a_warning(png):
    sc = load(png, "(texture :name 'tex' :file 'tex.png' :interpolation 'closest')")
    assert len(image_nodes(sc.desc)) == 1 and len(sc.warnings) == 1 and "assuming color" in sc.warnings[0]


def test_every_spectral_parameter_resolves_a_texture_name(png):
    sc = load(png, """(texture :name 'tex' :file 'tex.png' :type 'color' :interpolation 'closest')
        (material :name 'a' :type 'diffuse' :albedo 'tex') (material :name 'b' :type 'diffuse' :base 'tex') (material :name 'c' :type 'diffuse' :diffuse 'tex')
        (material :name 'd' :type 'mirror' :specularity 'tex')
        (material :name 'e' :type 'glass' :index 'tex' :transmission 'tex')
        (material :name 'f' :type 'conductor' :eta 'tex' :k 'tex')
        (material :name 'g' :type 'principled' :base 'tex')
        (material :name 'h' :type 'diffuse' :albedo (checkerboard 'tex' (checkerboard 0.5 'tex' 3) 2 4))""")
    d = sc.desc
    tex = [i for i in range(d.n_spectra) if d.spectra[i].kind == abi.SPEC_IMAGE]
    assert len(tex) == 1 and sc.warnings == []                       # one node, shared by every user
    t = tex[0]
    m = d.materials
    assert [m[i].albedo for i in range(4)] == [t] * 4
    assert (m[4].ior, m[4].transmission) == (t, t) and (m[5].ior, m[5].k) == (t, t) and m[6].albedo == t
    outer = d.spectra[m[7].albedo]
    assert outer.kind == abi.SPEC_CHECKER and outer.lhs == t and d.spectra[outer.rhs].kind == abi.SPEC_CHECKER and d.spectra[outer.rhs].rhs == t


def test_an_unknown_name_keeps_the_default_value_warning(png):
    sc = load(png, "(texture :name 'tex' :file 'tex.png' :type 'color' :interpolation 'bi') (material :name 'a' :type 'diffuse' :albedo 'text')")
    assert len(sc.warnings) == 1 and "unknown node 'text'" in sc.warnings[0] and "default value used" in sc.warnings[0]
    n = sc.desc.spectra[sc.desc.materials[0].albedo]
    assert n.kind == abi.SPEC_CONST and n.p[0] == 1.0


@pytest.mark.parametrize("body,code,needle", [
    ("(texture :name 's' :file 'tex.png' :type 'scalar')", -4, "scalar textures are not supported"),
    ("(texture :name 's' :file 'tex.png' :type 'color' :blur 0.5)", -4, ":blur"),
    ("(texture :name 's' :file 'tex.png' :type 'color' :blur [0, 0.1])", -4, ":blur"),
    ("(texture :name 's' :file 'nope.png' :type 'color')", -5, "nope.png"),
    ("(texture :name 's' :type 'color')", -1, "filename"),
    ("(texture :file 'tex.png' :type 'color')", -1, "without a name"),
    ("(texture :name 's' :file 'tex.png' :type 'normal')", -1, "no known type"),
    ("(texture :name 's' :file 'tex.png' :type 'color') (texture :name 's' :file 'tex.png' :type 'color')", -1, "already exists"),
    ("(texture :name 's' :file 'tex.png' :type 'color') (material :name 'm' :type 'diffuse' :albedo (smul 's' 0.5))", -4, "inside smul"),
    ("(texture :name 's' :file 'tex.png' :type 'color') (emission :name 'e' :type 'diffuse' :radiance 's')", -4, "emissions"),
    ("(texture :name 's' :file 'tex.png' :type 'color') (emission :name 'e' :type 'diffuse' :radiance (checkerboard 1 's'))", -4, "emissions"),
    ("(texture :name 's' :file 'tex.png' :type 'color') (light :name 'l' :type 'env' :radiance 's')", -4, "infinite lights"),
    ("(texture :name 's' :file 'tex.png' :type 'color') (material :name 'm' :type 'diffuse' :albedo 's') (entity :name 'b' :type 'sphere' :material 'm')", -4, "sphere entities"),
    ("(texture :name 's' :file 'tex.png' :type 'color') (material :name 'g' :type 'glass' :roughness 's')", -4, "must be a number"),
    ("(texture :name 's' :file 'tex.png' :type 'color') (material :name 'g' :type 'principled' :metallic 's')", -4, "must be a number"),
    ("(node :name 'n' :type 'perlin')", -4, "not supported by this backend yet"),
])
def test_refusals(png, body, code, needle):
    got, msg = refused(png, body)
    assert got == code and needle in msg, msg


def test_a_damaged_image_is_refused_with_the_readers_code(tmp_path):
    data = imf.encode_png(SAMPLES, 2, 8)
    imf.write(tmp_path / "cut.png", data[:-20])
    imf.write(tmp_path / "adam7.png", imf.encode_png(SAMPLES, 2, 8, interlace=1))
    imf.write(tmp_path / "neg.pfm", imf.encode_pfm(np.full((1, 1, 3), -0.5, np.float32)))
    assert refused(tmp_path, "(texture :name 's' :file 'cut.png' :type 'color')")[0] == -5
    assert refused(tmp_path, "(texture :name 's' :file 'adam7.png' :type 'color')")[0] == -4
    assert refused(tmp_path, "(texture :name 's' :file 'neg.pfm' :type 'color')")[0] == -1


def test_scene_builder_assembles_the_same_description(png):
    sc = load(png, """(material :name 'w' :type 'diffuse' :albedo (spectrum :start 400 :end 700 0.1 0.5 0.9))
        (texture :name 'tex' :file 'tex.png' :type 'color' :interpolation 'closest' :wrap ['clamp', 'mirror'])
        (texture :name 'lin' :file 'tex.png' :type 'color' :interpolation 'bi')""")
    rgb, _, _ = scene.load_image(str(png / "tex.png"))
    b = scene.SceneBuilder(8, 8)
    b.spectrum_table(400.0, 700.0, [0.1, 0.5, 0.9])                 # three floats: the texels that follow are padded to a multiple of four
    ids = [b.image_texture(rgb, interpolation="closest", wrap=("clamp", "mirror")), b.image_texture(rgb)]
    d = sc.desc
    assert d.n_spectra == len(b.spectra) == 3 and ids == [1, 2]
    for i in range(3):
        assert C.string_at(C.addressof(d.spectra[i]), C.sizeof(abi.Spectrum)) == C.string_at(C.addressof(b.spectra[i]), C.sizeof(abi.Spectrum)), i
    assert d.spectra[1].table_offset == 4 and d.spectra[2].table_offset == 4 + 64
    assert np.array_equal(tables(d), np.array(b.tables, np.float32))
