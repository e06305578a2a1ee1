#!/usr/bin/env python3
"""The visual feedback integrator's time per iteration, by kernel family (HIP events, prgpu_set_timing), for every mode on two scenes: a mesh
scene (a tessellated sphere over a floor) and a C4-like one (the Cornell box with a triangle soup).  A measurement, not a benchmark: one
process, a warm-up, then `--iters` timed iterations per mode.

    python tools/gpu_vf.py [--width 512 --height 512 --iters 8 --soup 200000] [--out profiles/vf_ms_per_iteration.log]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pearray_amd import _cabi as abi  # noqa: E402
from pearray_amd import backend, scene  # noqa: E402

FAMILIES = ("raygen", "trace_closest", "vf", "resolve")


def measure(name, make, iters, out):
    for mode in abi.VF_MODE_NAMES:
        sc = make()
        sc.integrator, sc.vf_mode, sc.vf_weighting = abi.INTEGRATOR_VF, abi.VF_MODES[mode], True
        ctx = backend.RenderContext(sc, device=0)
        ctx.render(2)   # warm-up
        ctx.waitForFinish()
        ctx.setTiming(True)
        ctx.render(iters)
        ctx.waitForFinish()
        ms = {f: ctx.kernelTime(f) for f in FAMILIES}
        assert all(n == iters for _, n in ms.values())
        line = "%-6s %dx%d %-22s %s  sum %.3f ms per iteration  hits %.3f" % (
            name, ctx.width, ctx.height, mode, "  ".join("%s %.3f" % (f, ms[f][0] / iters) for f in FAMILIES), sum(t for t, _ in ms.values()) / iters,
            ctx.statistics()["entity_hits"] / float(ctx.statistics()["camera_depth"]))
        print(line, flush=True)
        if out:
            out.write(line + "\n")
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--soup", type=int, default=200000)
    ap.add_argument("--out", default=None, help="append the result lines to this file")
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else None
    if out:
        out.write("# tools/gpu_vf.py: ms per iteration by kernel family (HIP events), %d timed iterations after a warm-up\n" % a.iters)
    measure("mesh", lambda: scene.sphere_light(a.width, a.height, spp=64), a.iters, out)
    measure("soup", lambda: scene.cornell_soup(a.width, a.height, spp=64, n_triangles=a.soup), a.iters, out)


if __name__ == "__main__":
    main()
