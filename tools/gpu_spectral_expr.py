#!/usr/bin/env python3
"""What spectral expression nodes cost: a 512 x 512 Cornell-style box
  plain       (refl r g b) albedos -- no expression in the scene: the scene runs the variant row without light path expressions,
  plain/top   the same, plus one material nothing uses whose albedo is an expression: the scene runs the TOP variant row, as every scene
              with an expression root does, and evaluates no program,
  two ops     every wall's albedo is (smul (sadd refl 0) 1): a program of five words per evaluation,
  depth 4     every wall's albedo is a balanced tree of seven operators over eight leaves that gives the same value: fifteen words, the full
              operand stack.
One call: this process starts no GPU work itself; every variant runs in a child process of its own under its own time limit (`--limit`
seconds), one after the other, and the first child that fails ends the run.  A child renders `--repeats` times `--iters` iterations after a
warm-up, timed with the host clock around work that ends in a device synchronise.  Prints ms per iteration as median (min .. max) and the
ratio to `plain`.

    python tools/gpu_spectral_expr.py [--size 512 --spp 128 --iters 16 --repeats 5 --limit 120] [--out profiles/spectral_expr_cost.log]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F = np.float32
KINDS = ("plain", "plain/top", "two ops", "depth 4")
WALLS = {  # name: (corners, colour)
    "floor": ([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], (0.7, 0.7, 0.65)),
    "ceiling": ([[-1, -1, 2], [-1, 1, 2], [1, 1, 2], [1, -1, 2]], (0.7, 0.7, 0.65)),
    "back": ([[-1, 1, 0], [1, 1, 0], [1, 1, 2], [-1, 1, 2]], (0.7, 0.7, 0.65)),
    "left": ([[-1, -1, 0], [-1, 1, 0], [-1, 1, 2], [-1, -1, 2]], (0.6, 0.1, 0.1)),
    "right": ([[1, -1, 0], [1, -1, 2], [1, 1, 2], [1, 1, 0]], (0.15, 0.5, 0.15)),
}


def albedo(b, colour, kind):
    x, op, c = b.refl(*colour), b.spectrum_op, b.spectrum_const
    if kind == "two ops":
        return op("smul", op("sadd", x, c(0.0)), c(1.0))
    if kind == "depth 4":   # ((x + 0) * (1 max 1)) + ((0 * x) - (0 min 1)): x again, through eight leaves and all four stack entries
        left = op("smul", op("sadd", x, c(0.0)), op("smax", c(1.0), c(1.0)))
        right = op("ssub", op("smul", c(0.0), b.refl(*colour)), op("smin", c(0.0), c(1.0)))
        return op("sadd", left, right)
    return x


def box(size, spp, kind):
    from pearray_amd import scene
    b = scene.SceneBuilder(size, size)
    b.settings.aa_samples = spp
    T = np.eye(4, dtype=F)
    T[:3, 3] = (0, -3.4, 1)
    b.set_camera(T, width=0.8, height=0.8, local_direction=(0, 1, 0), local_right=(1, 0, 0), local_up=(0, 0, 1))
    for name, (p, colour) in WALLS.items():
        b.add_mesh(p, [[0, 1, 2], [0, 2, 3]], b.lambert(albedo(b, colour, kind)))
    if kind == "plain/top":
        b.lambert(b.spectrum_op("sadd", b.refl(0.5, 0.5, 0.5), b.spectrum_const(0.0)))
    white = b.lambert(b.refl(0.7, 0.7, 0.65))
    b.add_mesh([[-0.3, -0.3, 1.98], [0.3, -0.3, 1.98], [0.3, 0.3, 1.98], [-0.3, 0.3, 1.98]], [[0, 1, 2], [0, 2, 3]], white,
               emission=b.diffuse_emission(b.smul(b.illuminant_d65(), b.illum(17, 12, 4))))
    for cx, cy, h in ((-0.35, 0.3, 1.2), (0.35, -0.2, 0.6)):   # two blocks
        r = 0.3
        c = [[cx - r, cy - r], [cx + r, cy - r], [cx + r, cy + r], [cx - r, cy + r]]
        for k in range(4):
            (x0, y0), (x1, y1) = c[k], c[(k + 1) % 4]
            b.add_mesh([[x0, y0, 0], [x1, y1, 0], [x1, y1, h], [x0, y0, h]], [[0, 1, 2], [0, 2, 3]], white)
        b.add_mesh([[x, y, h] for x, y in c], [[0, 1, 2], [0, 2, 3]], white)
    return b.build()


def child(a):
    from pearray_amd import _cabi as abi
    from pearray_amd import backend
    ctx = backend.RenderContext(box(a.size, a.spp, a.kind), device=0)
    ctx.render(2)            # warm-up: code objects, the pipeline's calibration launches
    ctx.waitForFinish()
    times = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        ctx.render(a.iters)
        ctx.waitForFinish()
        times.append((time.perf_counter() - t0) * 1e3 / a.iters)
    info = ctx.pipelineInfo()
    xyz = ctx.output()[0]
    ctx.close()
    print(json.dumps({"kind": a.kind, "times": times, "kernel": info["kernel"], "variant": info["variant"], "mean_y": float(xyz.reshape(-1, 3)[:, 1].mean()),
                      "library": os.path.basename(abi.LIB_PATH)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--spp", type=int, default=128)
    ap.add_argument("--iters", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--limit", type=int, default=120, help="seconds a variant's process may take")
    ap.add_argument("--kind", default=None, help="(internal) run this one variant in this process")
    ap.add_argument("--out", default=None, help="append the result lines to this file")
    a = ap.parse_args()
    if a.kind is not None:
        return child(a)
    results = []
    for k in KINDS:
        cmd = [sys.executable, os.path.abspath(__file__), "--kind", k, "--size", str(a.size), "--spp", str(a.spp), "--iters", str(a.iters), "--repeats", str(a.repeats)]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            sys.exit("variant '%s' did not finish within %d s: stopping" % (k, a.limit))
        if done.returncode != 0:
            sys.exit("variant '%s' ended with status %d: stopping\n%s" % (k, done.returncode, done.stderr[-2000:]))
        results.append(json.loads(done.stdout.strip().splitlines()[-1]))
    base = float(np.median(results[0]["times"]))
    lines = ["# tools/gpu_spectral_expr.py: %dx%d, %d iterations x %d repeats per variant, one process each, library %s" % (a.size, a.size, a.iters, a.repeats, results[0]["library"])]
    for r in results:
        t = r["times"]
        lines.append("%-10s %.3f ms/iteration (median; %.3f .. %.3f)  x%.3f of plain  kernel %s  variant row %d  mean Y %.5f"
                     % (r["kind"], float(np.median(t)), min(t), max(t), float(np.median(t)) / base, r["kernel"], r["variant"], r["mean_y"]))
    for line in lines:
        print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
