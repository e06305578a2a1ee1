"""The reader of the image files `(texture ...)` blocks name (csrc/host/image_reader.cpp; C ABI prgpu_image_load): PNG through zlib's
inflate and PFM, against the arrays this file encodes itself (tests/image_files.py, tools/fuzz_image.py: zlib + struct), the
linearisation against a float64 restatement of RGBConverter::linearize, and the refusals."""
import ctypes as C
import struct

import numpy as np
import pytest

from pearray_amd import _cabi as abi
from pearray_amd import scene

import image_files as imf

RNG = np.random.RandomState(3)


def load_code(path, pixels=False):
    """(return code, width, height) of the size query, or of the full read into a buffer for at most 64 pixels"""
    lib = abi.load()
    w, h = C.c_uint32(), C.c_uint32()
    buf = (C.c_float * 192)() if pixels else None
    return lib.prgpu_image_load(str(path).encode(), C.byref(w), C.byref(h), None, None, buf), w.value, h.value


def samples(h, w, colour_type, depth):
    hi = 4 if colour_type == 3 else (1 << depth)
    s = RNG.randint(0, hi, size=(h, w, imf.CHANNELS[colour_type]))
    s[0, 0] = 0                                             # both ends of the range, and a sample below the linearisation threshold
    s[-1, -1] = hi - 1
    s[0, -1] = min(hi - 1, 7 if depth == 8 else 2000)
    return s


PALETTE = np.array([[0, 0, 0], [255, 128, 9], [10, 200, 255], [255, 255, 255]])


@pytest.mark.parametrize("colour_type,depth", [(0, 8), (0, 16), (2, 8), (2, 16), (3, 8), (4, 8), (4, 16), (6, 8), (6, 16)])
def test_png_round_trip_of_every_colour_type_and_depth(tmp_path, colour_type, depth):
    s = samples(3, 5, colour_type, depth)                   # 5 x 3: a W / H swap cannot pass
    pal = PALETTE if colour_type == 3 else None
    path = imf.write(tmp_path / "a.png", imf.encode_png(s, colour_type, depth, palette=pal, trns=b"\x00\x40" if colour_type == 3 else None))
    rgb, channels, linearised = scene.load_image(path)
    assert rgb.shape == (3, 5, 3) and linearised
    assert channels == {0: 1, 2: 3, 3: 3, 4: 2, 6: 4}[colour_type]
    want = imf.png_rgb64(s, colour_type, depth, pal)
    assert np.allclose(rgb, want, rtol=1e-6, atol=0), np.abs(rgb / np.maximum(want, 1e-300) - 1).max()
    assert load_code(path) == (0, 5, 3)


@pytest.mark.parametrize("row_filter", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("colour_type,depth", [(2, 8), (6, 16), (0, 8)])
def test_png_every_row_filter(tmp_path, row_filter, colour_type, depth):
    s = samples(4, 6, colour_type, depth)
    path = imf.write(tmp_path / "f.png", imf.encode_png(s, colour_type, depth, filters=row_filter))
    rgb, _, _ = scene.load_image(path)
    assert np.allclose(rgb, imf.png_rgb64(s, colour_type, depth), rtol=1e-6, atol=0)


def test_png_split_idat_chunks_and_unknown_ancillary_chunks(tmp_path):
    s = samples(9, 11, 2, 8)
    whole = imf.encode_png(s, 2, 8)
    split = imf.encode_png(s, 2, 8, idat_split=7, extra=[(b"tEXt", b"Comment\0split"), (b"gAMA", struct.pack(">I", 45455))])
    assert split.count(b"IDAT") > 5
    a, _, _ = scene.load_image(imf.write(tmp_path / "whole.png", whole))
    b, _, _ = scene.load_image(imf.write(tmp_path / "split.png", split))
    assert np.array_equal(a, b) and np.allclose(a, imf.png_rgb64(s, 2, 8), rtol=1e-6, atol=0)


@pytest.mark.parametrize("little", [True, False])
def test_pfm_of_either_byte_order_and_its_row_order(tmp_path, little):
    img = RNG.rand(3, 5, 3).astype(np.float32) * 4          # taken as linear: values above 1 stay
    rgb, channels, linearised = scene.load_image(imf.write(tmp_path / "a.pfm", imf.encode_pfm(img, little=little)))
    assert channels == 3 and not linearised
    assert np.array_equal(rgb, img)                          # rows top-down although the file's run bottom-up
    grey = RNG.rand(4, 2).astype(np.float32)
    rgb, channels, _ = scene.load_image(imf.write(tmp_path / "g.pfm", imf.encode_pfm(grey, little=little, scale=3.0)))
    assert channels == 1 and np.array_equal(rgb, np.repeat(grey[:, :, None], 3, axis=2))


def test_linearisation_matches_a_float64_restatement(tmp_path):
    s8 = np.arange(256).reshape(16, 16, 1)                   # every 8-bit value: 0 .. 10 lie below the threshold (the quadratic toe)
    rgb, _, _ = scene.load_image(imf.write(tmp_path / "g8.png", imf.encode_png(s8, 0, 8)))
    x = np.float32(s8[:, :, 0]) / np.float32(255)
    want = imf.linearise64(x)
    assert np.allclose(rgb[:, :, 0], want, rtol=1e-6, atol=0)
    toe = x <= 0.04045
    assert toe.sum() == 11 and np.allclose(rgb[:, :, 0][toe], np.float64(x[toe]) ** 2 / 12.92, rtol=1e-6, atol=0)   # x / 12.92 * x, not x / 12.92
    s16 = np.array([0, 1, 100, 2650, 2651, 2652, 30000, 65535]).reshape(1, 8, 1)      # around the threshold 0.04045 * 65535 = 2650.9
    rgb, _, _ = scene.load_image(imf.write(tmp_path / "g16.png", imf.encode_png(s16, 0, 16)))
    assert np.allclose(rgb[0, :, 0], imf.linearise64(np.float32(s16[0, :, 0]) / np.float32(65535)), rtol=1e-6, atol=0)


def test_refusals(tmp_path):
    s = samples(4, 4, 2, 8)
    good = imf.encode_png(s, 2, 8)
    assert load_code(imf.write(tmp_path / "ok.png", good))[0] == 0
    # interlaced: a valid PNG this reader does not decode
    assert load_code(imf.write(tmp_path / "adam7.png", imf.encode_png(s, 2, 8, interlace=1)))[0] == -4
    assert b"interlaced" in abi.load().prgpu_last_error()
    # truncated: inside the header chunk, inside the data, and without its end chunk
    for cut in (4, 20, len(good) - 30, len(good) - 12):
        assert load_code(imf.write(tmp_path / "cut.png", good[:cut]), pixels=True)[0] == -5, cut
    assert load_code(imf.write(tmp_path / "cut.png", good[:20]))[0] == -5          # (the size query needs the header chunk only)
    lib = abi.load()
    w, h = C.c_uint32(), C.c_uint32()
    buf = (C.c_float * 48)()
    # a wrong checksum, of the data and of the header
    i = good.index(b"IDAT")
    bad = bytearray(good); bad[i + 6] ^= 0x10
    assert lib.prgpu_image_load(imf.write(tmp_path / "crc.png", bytes(bad)).encode(), C.byref(w), C.byref(h), None, None, buf) == -1
    assert b"checksum" in lib.prgpu_last_error()
    bad = bytearray(good); bad[17] ^= 1
    assert load_code(imf.write(tmp_path / "crc2.png", bytes(bad)))[0] == -1
    # a damaged stream under a right checksum, and a row filter that does not exist
    raw = b"".join(bytes([9 if y == 2 else 0]) + s[y].astype(np.uint8).tobytes() for y in range(4))
    import zlib
    head = imf.fuzz_image.PNG_MAGIC + imf.chunk(b"IHDR", struct.pack(">IIBBBBB", 4, 4, 8, 2, 0, 0, 0))
    for body in (zlib.compress(raw), zlib.compress(raw[:-5]), zlib.compress(raw + b"abc"), zlib.compress(raw)[:-6], b"\x00\x01\x02"):
        f = imf.write(tmp_path / "z.png", head + imf.chunk(b"IDAT", body) + imf.chunk(b"IEND", b""))
        assert lib.prgpu_image_load(f.encode(), C.byref(w), C.byref(h), None, None, buf) == -1
    # sizes: a side of 4097 (either one), an empty image; 4096 passes the size query
    for wh, code in (((4097, 1), -1), ((1, 4097), -1), ((0, 3), -1), ((3, 0), -1), ((0x80000000, 0x80000000), -1), ((4096, 4096), 0)):
        f = imf.write(tmp_path / "size.png", imf.fuzz_image.PNG_MAGIC + imf.chunk(b"IHDR", struct.pack(">IIBBBBB", wh[0], wh[1], 8, 2, 0, 0, 0)))
        assert load_code(f)[0] == code, wh
    for header, code in ((b"PF\n4097 1\n-1\n", -1), (b"PF\n0 1\n-1\n", -1), (b"PF\n2 2\n0\n", -1), (b"PF\n2 2\n-1\n" + bytes(47), -5), (b"PF\n2 2\n-1\n" + bytes(48), 0)):
        f = imf.write(tmp_path / "size.pfm", header)
        rc = lib.prgpu_image_load(f.encode(), C.byref(w), C.byref(h), None, None, buf)
        assert rc == code, header
    # a palette index past the palette, bit depths below 8, a missing file, neither format
    f = imf.write(tmp_path / "pal.png", imf.encode_png(np.full((2, 2, 1), 3), 3, 8, palette=PALETTE[:3]))
    assert lib.prgpu_image_load(f.encode(), C.byref(w), C.byref(h), None, None, buf) == -1
    f = imf.write(tmp_path / "d4.png", imf.fuzz_image.PNG_MAGIC + imf.chunk(b"IHDR", struct.pack(">IIBBBBB", 4, 4, 4, 0, 0, 0, 0)))
    assert load_code(f)[0] == -4
    assert load_code(tmp_path / "missing.png")[0] == -5
    assert load_code(imf.write(tmp_path / "x.jpg", b"\xff\xd8\xff\xe0" + bytes(64)))[0] == -4
    assert lib.prgpu_image_load(None, C.byref(w), C.byref(h), None, None, None) == -1
