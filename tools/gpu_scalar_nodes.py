#!/usr/bin/env python3
"""What a scalar node on `:roughness` costs: a Cornell-style box whose five walls are rough conductors with
  numeric   a number -- no scalar node in the scene: it runs the variant row without light path expressions,
  top       the same numbers, plus one material nothing uses that binds a scalar node: the scene runs the TOP variant row, as every
            scalar-node scene does,
  closest   a 256 x 256 scalar texture each, closest texel,
  bilinear  the same maps, bilinear,
  tree      (min (add (mul map 0.5) 0.05) 0.6): three operators over each map, closest.
One call runs all five, each in a process of its own, one after the other: a warm-up, then `--repeats` times `--iters` iterations timed with
the host clock around work that ends in a device synchronise.  Prints ms per iteration (median, min .. max over the repeats) and the ratio
to `numeric` of the same call -- figures of different calls do not compare.  The maps are generated here from a seed.

    python tools/gpu_scalar_nodes.py [--size 512 --spp 128 --iters 16 --repeats 5] [--out profiles/scalar_nodes_cost.log]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

F = np.float32
KINDS = ("numeric", "top", "closest", "bilinear", "tree")
WALLS = {  # name: (corners, mean roughness)
    "floor": ([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], 0.35),
    "ceiling": ([[-1, -1, 2], [-1, 1, 2], [1, 1, 2], [1, -1, 2]], 0.5),
    "back": ([[-1, 1, 0], [1, 1, 0], [1, 1, 2], [-1, 1, 2]], 0.25),
    "left": ([[-1, -1, 0], [-1, 1, 0], [-1, 1, 2], [-1, -1, 2]], 0.4),
    "right": ([[1, -1, 0], [1, -1, 2], [1, 1, 2], [1, 1, 0]], 0.3),
}


def box(size, spp, kind):
    from pearray_amd import scene
    b = scene.SceneBuilder(size, size)
    b.settings.aa_samples = spp
    T = np.eye(4, dtype=F)
    T[:3, 3] = (0, -3.4, 1)
    b.set_camera(T, width=0.8, height=0.8, local_direction=(0, 1, 0), local_right=(1, 0, 0), local_up=(0, 0, 1))
    rng = np.random.RandomState(9)
    for name, (p, mean) in WALLS.items():
        if kind in ("numeric", "top"):
            roughness = mean
        else:
            values = F(mean) * (F(0.5) + rng.rand(256, 256).astype(F))
            roughness = b.scalar_image(values, interpolation="bilinear" if kind == "bilinear" else "closest", wrap="periodic")
            if kind == "tree":
                roughness = b.scalar_op("min", b.scalar_op("add", b.scalar_op("mul", roughness, 0.5), 0.05), 0.6)
        b.add_mesh(p, [[0, 1, 2], [0, 2, 3]], b.rough_conductor(roughness, specularity=b.refl(0.9, 0.8, 0.6)), uvs=[[0, 0], [1, 0], [1, 1], [0, 1]])
    if kind == "top":
        b.rough_conductor(b.scalar_image(F([[0.5]])))          # on no triangle
    white = b.lambert(b.refl(0.7, 0.7, 0.65))
    b.add_mesh([[-0.3, -0.3, 1.98], [0.3, -0.3, 1.98], [0.3, 0.3, 1.98], [-0.3, 0.3, 1.98]], [[0, 1, 2], [0, 2, 3]], white, uvs=[[0, 0], [1, 0], [1, 1], [0, 1]],
               emission=b.diffuse_emission(b.smul(b.illuminant_d65(), b.illum(17, 12, 4))))
    for cx, cy, h in ((-0.35, 0.3, 1.2), (0.35, -0.2, 0.6)):   # two blocks
        r = 0.3
        c = [[cx - r, cy - r], [cx + r, cy - r], [cx + r, cy + r], [cx - r, cy + r]]
        for k in range(4):
            (x0, y0), (x1, y1) = c[k], c[(k + 1) % 4]
            b.add_mesh([[x0, y0, 0], [x1, y1, 0], [x1, y1, h], [x0, y0, h]], [[0, 1, 2], [0, 2, 3]], white, uvs=[[0, 0], [1, 0], [1, 1], [0, 1]])
        b.add_mesh([[x, y, h] for x, y in c], [[0, 1, 2], [0, 2, 3]], white, uvs=[[0, 0], [1, 0], [1, 1], [0, 1]])
    return b.build()


def one_kind(a):
    """the child: one variant in this process; a JSON line with its times"""
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
    print(json.dumps({"kind": a.kind, "times": times, "kernel": info["kernel"], "variant": info["variant"], "mean_y": float(xyz.reshape(-1, 3)[:, 1].mean())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--spp", type=int, default=128)
    ap.add_argument("--iters", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the result lines to this file")
    ap.add_argument("--kind", default=None, choices=KINDS, help="(what the tool starts itself with: one variant in this process)")
    a = ap.parse_args()
    if a.kind:
        return one_kind(a)
    results = {}
    for k in KINDS:          # one process per variant, one after the other; a child that fails ends the call: nothing more is started on the GPU
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--kind", k, "--size", str(a.size), "--spp", str(a.spp), "--iters", str(a.iters), "--repeats", str(a.repeats)],
                           stdout=subprocess.PIPE, timeout=240)
        if p.returncode != 0:
            print("variant %s ended with status %d: stopping" % (k, p.returncode), flush=True)
            return p.returncode
        results[k] = json.loads(p.stdout.decode().strip().splitlines()[-1])
    base = float(np.median(results["numeric"]["times"]))
    lines = ["# tools/gpu_scalar_nodes.py: %dx%d, %d iterations x %d repeats per variant, one process each; ratios to `numeric` of this call" % (a.size, a.size, a.iters, a.repeats)]
    for k in KINDS:
        r = results[k]
        lines.append("%-9s %.3f ms/iteration (median; %.3f .. %.3f)  x%.3f of numeric  kernel %s  variant row %d  mean Y %.5f"
                     % (k, float(np.median(r["times"])), min(r["times"]), max(r["times"]), float(np.median(r["times"])) / base, r["kernel"], r["variant"], r["mean_y"]))
    for line in lines:
        print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
