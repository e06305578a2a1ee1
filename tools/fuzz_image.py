#!/usr/bin/env python3
"""Fuzz the image reader of (texture ...) blocks (host/image_reader.cpp: PNG through zlib's inflate, PFM) under AddressSanitizer +
UndefinedBehaviorSanitizer, the way tools/fuzz_loader.py fuzzes the scene readers.

`make -C pearray_amd/csrc san` builds the reader (plain C++, no device code) into build_san/prc_san; `prc_san --image -` calls
prgpu_image_load on every path it reads from stdin (the size query, then the pixels).  This script encodes its own seed files -- PNGs of
every colour type, both bit depths, every row filter, split IDAT chunks, a palette with tRNS; PFMs of both kinds and byte orders --
derives truncations and byte mutations of them with a FIXED seed (the checksums of a mutated PNG are repaired for half the mutants, so
that mutations reach the chunk parsers, the inflate stream and the filters and do not all end at the first CRC), and feeds the lot to
the driver.  A finding = the driver dies (the sanitizers abort); a clean run = one status line per input, each 0 or a negative error code.

  python tools/fuzz_image.py [--n 400] [--seed 7] [--keep DIR]     -> prints a summary, exit code 1 on a finding
tests/test_fuzz_image.py runs it in the CPU suite.  encode_png / encode_pfm are also what the texture tests write their images with."""
import argparse
import os
import random
import struct
import subprocess
import sys
import tempfile
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pearray_amd", "csrc")
DRIVER = os.path.join(CSRC, "build_san", "prc_san")
PNG_MAGIC = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}   # samples per pixel of a PNG colour type


def chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def filter_row(ft, row, prev, bpp):
    """One scanline (bytes) under PNG row filter `ft` (0 none, 1 sub, 2 up, 3 average, 4 Paeth); `prev` is the unfiltered row above (zeros for the first)."""
    out = bytearray(len(row))
    for i, x in enumerate(row):
        a = row[i - bpp] if i >= bpp else 0
        b = prev[i]
        c = prev[i - bpp] if i >= bpp else 0
        out[i] = (x - (0, a, b, (a + b) >> 1, _paeth(a, b, c))[ft]) & 0xFF
    return bytes(out)


def encode_png(samples, colour_type, depth=8, filters=None, idat_split=0, palette=None, trns=None, interlace=0, extra=()):
    """samples: integer array [H, W, CHANNELS[colour_type]] (palette indices for type 3); filters: one row filter for all rows, or one per row
    (default: row y uses y % 5); idat_split: cut the compressed stream into IDAT chunks of that many bytes (0: one chunk);
    palette: [N, 3] uint8 (type 3); trns: bytes of a tRNS chunk; extra: (tag, data) chunks put before the first IDAT."""
    samples = np.asarray(samples)
    h, w, c = samples.shape
    assert c == CHANNELS[colour_type] and depth in (8, 16)
    data = samples.astype(">u2" if depth == 16 else "u1")
    bpp = c * depth // 8
    if filters is None:
        filters = [y % 5 for y in range(h)]
    elif isinstance(filters, int):
        filters = [filters] * h
    raw, prev = b"", bytes(w * bpp)
    for y in range(h):
        row = data[y].tobytes()
        raw += bytes([filters[y]]) + filter_row(filters[y], row, prev, bpp)
        prev = row
    z = zlib.compress(raw, 6)
    out = PNG_MAGIC + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, colour_type, 0, 0, interlace))
    if palette is not None:
        out += chunk(b"PLTE", np.asarray(palette, np.uint8).tobytes())
    if trns is not None:
        out += chunk(b"tRNS", bytes(trns))
    for tag, d in extra:
        out += chunk(tag, d)
    step = idat_split or len(z)
    for i in range(0, len(z), step):
        out += chunk(b"IDAT", z[i:i + step])
    return out + chunk(b"IEND", b"")


def encode_pfm(image, little=True, scale=1.0):
    """image: float array [H, W, 3] (`PF`) or [H, W] / [H, W, 1] (`Pf`), rows top-down; the file's rows run bottom-up and the sign of the
    scale tells the byte order."""
    image = np.asarray(image, np.float32)
    if image.ndim == 2:
        image = image[:, :, None]
    h, w, c = image.shape
    assert c in (1, 3)
    head = "%s\n%d %d\n%g\n" % ("PF" if c == 3 else "Pf", w, h, -abs(scale) if little else abs(scale))
    return head.encode() + image[::-1].astype("<f4" if little else ">f4").tobytes()


def seeds():
    rng = np.random.RandomState(11)
    out = {}
    for ct in (0, 2, 3, 4, 6):
        for depth in ((8,) if ct == 3 else (8, 16)):
            hi = 5 if ct == 3 else (1 << depth)
            s = rng.randint(0, hi, size=(6, 7, CHANNELS[ct]))
            pal = rng.randint(0, 256, size=(5, 3)) if ct == 3 else None
            out["t%d_d%d.png" % (ct, depth)] = encode_png(s, ct, depth, palette=pal, trns=b"\x00\x80" if ct == 3 else None, idat_split=40 if ct == 2 else 0)
    out["rgb_l.pfm"] = encode_pfm(rng.rand(4, 5, 3), little=True)
    out["rgb_b.pfm"] = encode_pfm(rng.rand(4, 5, 3), little=False)
    out["grey_l.pfm"] = encode_pfm(rng.rand(3, 2), little=True, scale=2.5)
    return out


def repair_png(data):
    """Recompute the checksum of every chunk whose length field still fits the file (the rest of the file is kept as it is)."""
    if not data.startswith(PNG_MAGIC):
        return data
    out, pos = bytearray(data[:8]), 8
    while len(data) - pos >= 12:
        n = struct.unpack(">I", data[pos:pos + 4])[0]
        if n > len(data) - pos - 12:
            break
        body = data[pos + 4:pos + 8 + n]
        out += data[pos:pos + 4] + body + struct.pack(">I", zlib.crc32(body) & 0xFFFFFFFF)
        pos += 12 + n
    return bytes(out) + data[pos:]


def mutate(data, rng):
    """One mutant: a truncation, byte flips, a deleted or duplicated span, a 32-bit field set to an edge value, or (PNG) damage INSIDE the
    inflated stream: the scanlines are unpacked, mutated and packed again."""
    b = bytearray(data)
    kind = rng.randrange(6)
    if kind == 0 and len(b) > 1:
        return bytes(b[:rng.randrange(len(b))])
    if kind == 1:
        for _ in range(1 + rng.randrange(4)):
            b[rng.randrange(len(b))] = rng.randrange(256)
        return bytes(b)
    if kind == 2 and len(b) > 4:
        i = rng.randrange(len(b) - 1)
        return bytes(b[:i] + b[min(len(b), i + 1 + rng.randrange(16)):])
    if kind == 3 and len(b) > 4:
        i = rng.randrange(len(b) - 1)
        j = min(len(b), i + 1 + rng.randrange(32))
        return bytes(b[:j] + b[i:j] * (1 + rng.randrange(3)) + b[j:])
    if kind == 4 and len(b) >= 4:
        i = rng.randrange(len(b) - 3)
        b[i:i + 4] = struct.pack(rng.choice("<>") + "I", rng.choice([0, 1, 4096, 4097, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 65536]))
        return bytes(b)
    i = data.find(b"IDAT")
    if i >= 4 and data.startswith(PNG_MAGIC):      # (the seed's first IDAT chunk alone: a split stream then ends early, which is a case too)
        n = struct.unpack(">I", data[i - 4:i])[0]
        try:
            raw = bytearray(zlib.decompressobj().decompress(data[i + 4:i + 4 + n]))
        except zlib.error:
            raw = bytearray()
        if raw:
            for _ in range(1 + rng.randrange(3)):
                raw[rng.randrange(len(raw))] = rng.randrange(256)
            if rng.random() < 0.3:
                raw = raw[:rng.randrange(len(raw))] if rng.random() < 0.5 else raw + raw[:rng.randrange(64)]
            return data[:i - 4] + chunk(b"IDAT", zlib.compress(bytes(raw))) + data[i + 8 + n:]
    return bytes(b)


def run(n=400, seed=7, keep=None, timeout=600):
    subprocess.check_call(["make", "-C", CSRC, "san"], stdout=subprocess.DEVNULL)   # (nothing to do when the driver is up to date)
    rng = random.Random(seed)
    tmp = keep or tempfile.mkdtemp(prefix="image_fuzz_")
    os.makedirs(tmp, exist_ok=True)
    files = seeds()
    paths = []
    for name, data in sorted(files.items()):
        paths.append(os.path.join(tmp, name))
        with open(paths[-1], "wb") as f:
            f.write(data)
    names = sorted(files)
    for k in range(n):
        name = names[k % len(names)]
        m = files[name]
        for _ in range(1 + rng.randrange(2)):
            m = mutate(m, rng)
        if rng.random() < 0.5:
            m = repair_png(m)
        paths.append(os.path.join(tmp, "m%04d_%s" % (k, name)))
        with open(paths[-1], "wb") as f:
            f.write(m)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:allocator_may_return_null=1:max_allocation_size_mb=2048", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([DRIVER, "--image", "-"], input=("\n".join(paths) + "\n").encode(), capture_output=True, env=env, timeout=timeout)
    lines = [l for l in p.stdout.decode("ascii", "replace").split("\n") if l]
    codes = {}
    for l in lines[len(files):]:
        codes[l.split()[0]] = codes.get(l.split()[0], 0) + 1
    finding = p.returncode != 0 or len(lines) != len(paths)
    report = {"inputs": len(paths), "answered": len(lines), "seeds": len(files), "seed_codes": sorted({l.split()[0] for l in lines[:len(files)]}),
              "status_codes": codes, "driver_exit": p.returncode, "seed": seed, "first_unanswered": paths[len(lines)] if len(lines) < len(paths) else None,
              "stderr_tail": p.stderr.decode("utf-8", "replace")[-3000:] if finding else ""}
    if not keep and not finding:
        import shutil
        shutil.rmtree(tmp, ignore_errors=True)
    return finding, report


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=400)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--keep", default=None)
    a = ap.parse_args()
    bad, rep = run(a.n, a.seed, a.keep)
    print(rep)
    sys.exit(1 if bad else 0)
