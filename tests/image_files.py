"""What the image-texture tests share: the PNG / PFM encoders of tools/fuzz_image.py (zlib + struct, nothing else), restatements of the
reader's sample conversion and of the device's texel lookup (include/prgpu.h, PRGPU_SPEC_IMAGE), and the spectrum of a texel."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("fuzz_image", os.path.join(ROOT, "tools", "fuzz_image.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


fuzz_image = _tool()
encode_png, encode_pfm, chunk, CHANNELS = fuzz_image.encode_png, fuzz_image.encode_pfm, fuzz_image.chunk, fuzz_image.CHANNELS


def write(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return str(path)


def linearise64(x):
    """RGBConverter::linearize (spectral/RGBConverter.cpp:53-58) in float64 -- the toe is x / 12.92 * x, a quirk the reader keeps"""
    x = np.asarray(x, np.float64)
    return np.where(x <= np.float64(np.float32(0.04045)), x / 12.92 * x, np.power((x + 0.055) / 1.055, 2.4))


def png_rgb64(samples, colour_type, depth, palette=None):
    """The float64 linear RGB [H, W, 3] the reader must return for integer samples [H, W, C]: grey replicated, alpha dropped, a palette looked up"""
    s = np.asarray(samples)
    if colour_type == 3:
        v = np.asarray(palette)[s[:, :, 0]] / 255.0
    else:
        v = s[:, :, :3] if CHANNELS[colour_type] >= 3 else np.repeat(s[:, :, :1], 3, axis=2)
        v = v / (255.0 if depth == 8 else 65535.0)
    return linearise64(np.float32(v))      # (the reader divides in fp32)


def upsample32(c, wl):
    """upsample() of pr_device.h in numpy float32: c = the three coefficients [..., 3], wl a wavelength"""
    c = np.asarray(c, np.float32)
    wl = np.float32(wl)
    x = (c[..., 0] * wl + c[..., 1]) * wl + c[..., 2]
    return (np.float32(0.5) * x) * (np.float32(1.0) / np.sqrt(x * x + np.float32(1.0))) + np.float32(0.5)


def wrap_index(i, n, mode):
    """One texel index under a wrap mode (0 black, 1 clamp, 2 periodic, 3 mirror); -1 = the black texel.  Integer arrays."""
    i = np.asarray(i, np.int64)
    if mode == 1:
        return np.clip(i, 0, n - 1)
    if mode == 2:
        return np.mod(i, n)
    if mode == 3:
        r = np.mod(i, 2 * n)
        return np.where(r >= n, 2 * n - 1 - r, r)
    return np.where((i < 0) | (i >= n), -1, i)


def lookup_closest(spectra, black, u, v, wraps=(0, 0)):
    """Expected value at uv (float64 arrays) of a closest lookup: spectra [H, W] of the texels, `black` that of the black texel"""
    h, w = spectra.shape
    s, t = np.asarray(u, np.float64), 1.0 - np.asarray(v, np.float64)
    i = wrap_index(np.floor(s * w), w, wraps[0])
    j = wrap_index(np.floor(t * h), h, wraps[1])
    out = spectra[np.maximum(j, 0), np.maximum(i, 0)].astype(np.float64)
    return np.where((i < 0) | (j < 0), np.float64(black), out)


def boundary_distance(u, v, w, h):
    """distance, in texels, of uv from the nearest texel boundary of a closest lookup"""
    s, t = np.asarray(u, np.float64) * w, (1.0 - np.asarray(v, np.float64)) * h
    return np.minimum(np.abs(s - np.round(s)), np.abs(t - np.round(t)))


def lookup_bilinear(spectra, black, u, v, wraps=(0, 0)):
    """Expected value of a bilinear lookup: the float64 blend, in the device's order, of the four fp32 spectra"""
    h, w = spectra.shape
    x = np.asarray(u, np.float64) * w - 0.5
    y = (1.0 - np.asarray(v, np.float64)) * h - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0

    def tex(i, j):
        i, j = wrap_index(i, w, wraps[0]), wrap_index(j, h, wraps[1])
        val = spectra[np.maximum(j, 0), np.maximum(i, 0)].astype(np.float64)
        return np.where((i < 0) | (j < 0), np.float64(black), val)
    return (tex(x0, y0) * (1 - fx) + tex(x0 + 1, y0) * fx) * (1 - fy) + (tex(x0, y0 + 1) * (1 - fx) + tex(x0 + 1, y0 + 1) * fx) * fy
