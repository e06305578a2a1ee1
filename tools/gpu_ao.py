#!/usr/bin/env python3
"""Occlusion kernel of the ambient occlusion integrator against the ray service on the IDENTICAL rays, in one process.

For a mesh scene (a tessellated sphere over a floor, like examples/mesh.prc) and a C4-like one (the Cornell box with a triangle soup):
render AO with instrumentation on, take the dumped rays of the last iteration, then time
  * the occlusion kernel (kernel family "ao") over plain iterations, which build the same kind of rays in the lanes, and
  * prgpu_trace_any (family "trace_any") on the dumped rays, which reads them from memory,
and print both in Mrays/s with their ratio.  Which counting scheme the library was built with (one atomic per hit and wave step, or one
per occluded ray: `make EXTRA=-DPR_AO_FOLD=0 B=build_ao0 LIB=libprgpu_ao0.so`, then PRGPU_LIBRARY=.../libprgpu_ao0.so) is the A/B this
probe is run twice for.

    python tools/gpu_ao.py [--width 512 --height 512 --samples 32 --iters 8 --soup 200000] [--out profiles/ao_occlusion_vs_service.log]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pearray_amd import _cabi as abi  # noqa: E402
from pearray_amd import backend, scene  # noqa: E402


def mesh_scene(w, h, n):
    sc = scene.sphere_light(w, h, spp=64)   # a 16 k-triangle sphere with vertex normals over a floor (its lamp plays no part)
    sc.integrator, sc.ao_sample_count = abi.INTEGRATOR_AO, n
    return sc


def soup_scene(w, h, n, tris):
    sc = scene.cornell_soup(w, h, spp=64, n_triangles=tris)
    sc.integrator, sc.ao_sample_count = abi.INTEGRATOR_AO, n
    return sc


def measure(name, sc, iters, out):
    ctx = backend.RenderContext(sc, device=0)
    n = ctx.ao_sample_count
    ctx.setInstrumentation(True)
    ctx.render(1)
    ctx.waitForFinish()
    state, org, direction, occ = ctx.aoSamples()
    hit = state != 0
    org, direction, occ = org[hit].reshape(-1, 3), direction[hit].reshape(-1, 3), occ[hit].reshape(-1)
    ctx.setInstrumentation(False)
    ctx.render(2)   # warm-up of the plain kernel
    ctx.waitForFinish()
    ctx.setTiming(True)
    before = ctx.statistics()["shadow_rays"]
    ctx.render(iters)
    ctx.waitForFinish()
    ao_ms, ao_launches = ctx.kernelTime("ao")
    ao_rays = ctx.statistics()["shadow_rays"] - before
    tmin = np.float32(1.1920928955078125e-7)
    same = np.array_equal(ctx.traceShadowRays(org, direction, tmin, np.inf), occ)   # (also the service's warm-up)
    t0, l0 = ctx.kernelTime("trace_any")
    for _ in range(iters):
        ctx.traceShadowRays(org, direction, tmin, np.inf)
    t1, l1 = ctx.kernelTime("trace_any")
    ao_rate, svc_rate = ao_rays / ao_ms / 1e3, len(org) * (l1 - l0) / (t1 - t0) / 1e3
    line = ("%-6s %dx%d N=%d  rays/iteration %d  occluded %.3f  bits equal %s  ao %.1f Mrays/s (%d launches, %.3f ms each)  "
            "trace_any %.1f Mrays/s (%d launches, %.3f ms each)  ratio %.3f  bvh width %d"
            % (name, ctx.width, ctx.height, n, len(org), float(occ.mean()), same, ao_rate, ao_launches, ao_ms / max(1, ao_launches), svc_rate, l1 - l0,
               (t1 - t0) / max(1, l1 - l0), ao_rate / svc_rate, ctx.pipelineInfo()["bvh_width"]))
    print(line, flush=True)
    if out:
        out.write(line + "\n")
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--soup", type=int, default=200000)
    ap.add_argument("--out", default=None, help="append the result lines to this file")
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else None
    if out:
        out.write("# tools/gpu_ao.py: library %s\n" % os.path.basename(abi.LIB_PATH))
    measure("mesh", mesh_scene(a.width, a.height, a.samples), a.iters, out)
    measure("soup", soup_scene(a.width, a.height, a.samples, a.soup), a.iters, out)


if __name__ == "__main__":
    main()
