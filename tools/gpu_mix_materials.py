#!/usr/bin/env python3
"""What the Oren-Nayar / null / blend / add materials cost: a Cornell-style box
  lambert      Lambert walls and blocks -- no such material in the scene: the scene runs the variant row without light path expressions,
  lambert/top  the same, plus one null material nothing uses: the scene runs the TOP variant row, as every scene with one of the four kinds does,
  orennayar    Oren-Nayar walls (roughness 0.6), Lambert blocks,
  blend        Lambert walls, blocks of blend(Lambert, rough conductor, 0.5): two closure evaluations per next event estimation,
  nested       the same with every such blend wrapped once more, blend(null, blend(Lambert, rough conductor, 0.5), 1): what one more level costs alone
               -- the same two leaves with the same coefficients, a sample draws one more number and takes one more step down.  (Factor 1, not 0:
               a factor of 0 is material1 alone, blend.cpp:109, which would turn the blocks into null surfaces and time another scene.)
rendered in ONE process, alternating, `--repeats` times `--iters` iterations each after a warm-up, timed with the host clock around work
that ends in a device synchronise.  Prints ms per iteration (median, min .. max over the repeats) and the ratio to `lambert`.

    python tools/gpu_mix_materials.py [--size 512 --spp 128 --iters 16 --repeats 5] [--kinds lambert,blend] [--out profiles/mix_nesting_cost.log]

`--kinds` leaves scenes out (`lambert` always runs: it is the unit of the ratios) -- a library from before nested trees refuses `nested`.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pearray_amd import _cabi as abi  # noqa: E402
from pearray_amd import backend, scene  # noqa: E402

F = np.float32
WALLS = {  # name: (corners, colour)
    "floor": ([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], (0.7, 0.7, 0.65)),
    "ceiling": ([[-1, -1, 2], [-1, 1, 2], [1, 1, 2], [1, -1, 2]], (0.7, 0.7, 0.65)),
    "back": ([[-1, 1, 0], [1, 1, 0], [1, 1, 2], [-1, 1, 2]], (0.7, 0.7, 0.65)),
    "left": ([[-1, -1, 0], [-1, 1, 0], [-1, 1, 2], [-1, -1, 2]], (0.6, 0.1, 0.1)),
    "right": ([[1, -1, 0], [1, -1, 2], [1, 1, 2], [1, 1, 0]], (0.15, 0.5, 0.15)),
}
UP = {"floor": (0, 0, 1), "ceiling": (0, 0, -1), "back": (0, -1, 0), "left": (1, 0, 0), "right": (-1, 0, 0)}


def box(size, spp, kind):
    b = scene.SceneBuilder(size, size)
    b.settings.aa_samples = spp
    T = np.eye(4, dtype=F)
    T[:3, 3] = (0, -3.4, 1)
    b.set_camera(T, width=0.8, height=0.8, local_direction=(0, 1, 0), local_right=(1, 0, 0), local_up=(0, 0, 1))
    for name, (p, colour) in WALLS.items():   # vertex normals towards the room: an orthonormal tangent frame, and the side Oren-Nayar lights
        mat = b.oren_nayar(b.refl(*colour), 0.6) if kind == "orennayar" else b.lambert(b.refl(*colour))
        b.add_mesh(p, [[0, 1, 2], [0, 2, 3]], mat, normals=[UP[name]] * 4)
    if kind == "lambert/top":
        b.null()
    white = b.lambert(b.refl(0.7, 0.7, 0.65))
    b.add_mesh([[-0.3, -0.3, 1.98], [0.3, -0.3, 1.98], [0.3, 0.3, 1.98], [-0.3, 0.3, 1.98]], [[0, 1, 2], [0, 2, 3]], white,
               emission=b.diffuse_emission(b.smul(b.illuminant_d65(), b.illum(17, 12, 4))))
    block = b.blend(white, b.rough_conductor(0.25), 0.5) if kind in ("blend", "nested") else white
    if kind == "nested":
        block = b.blend(b.null(), block, 1.0)
    for cx, cy, h in ((-0.35, 0.3, 1.2), (0.35, -0.2, 0.6)):   # two blocks
        r = 0.3
        c = [[cx - r, cy - r], [cx + r, cy - r], [cx + r, cy + r], [cx - r, cy + r]]
        for k in range(4):
            (x0, y0), (x1, y1) = c[k], c[(k + 1) % 4]
            b.add_mesh([[x0, y0, 0], [x1, y1, 0], [x1, y1, h], [x0, y0, h]], [[0, 1, 2], [0, 2, 3]], block)
        b.add_mesh([[x, y, h] for x, y in c], [[0, 1, 2], [0, 2, 3]], block)
    return b.build()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--spp", type=int, default=128)
    ap.add_argument("--iters", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the result lines to this file")
    ap.add_argument("--kinds", default=None, help="comma-separated subset of the scenes")
    a = ap.parse_args()
    kinds = ("lambert", "lambert/top", "orennayar", "blend", "nested")
    if a.kinds:
        kinds = tuple(k for k in kinds if k == "lambert" or k in a.kinds.split(","))
    ctxs = {}
    for k in kinds:
        ctxs[k] = backend.RenderContext(box(a.size, a.spp, k), device=0)
        ctxs[k].render(2)            # warm-up: code objects, the pipeline's calibration launches
        ctxs[k].waitForFinish()
    times = {k: [] for k in kinds}
    for _ in range(a.repeats):       # alternating: a drift of the shared machine touches every kind alike
        for k in kinds:
            t0 = time.perf_counter()
            ctxs[k].render(a.iters)
            ctxs[k].waitForFinish()
            times[k].append((time.perf_counter() - t0) * 1e3 / a.iters)
    base = float(np.median(times["lambert"]))
    lines = ["# tools/gpu_mix_materials.py: %dx%d, %d iterations x %d repeats per kind, library %s" % (a.size, a.size, a.iters, a.repeats, os.path.basename(abi.LIB_PATH))]
    for k in kinds:
        info = ctxs[k].pipelineInfo()
        xyz = ctxs[k].output()[0]
        lines.append("%-11s %.3f ms/iteration (median; %.3f .. %.3f)  x%.3f of lambert  kernel %s  variant row %d  mean Y %.5f"
                     % (k, float(np.median(times[k])), min(times[k]), max(times[k]), float(np.median(times[k])) / base, info["kernel"], info["variant"],
                        float(xyz.reshape(-1, 3)[:, 1].mean())))
        ctxs[k].close()
    for line in lines:
        print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
