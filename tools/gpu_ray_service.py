"""Ray service (prgpu_trace_closest, the IArchive surface) on the C4 scene: Mrays/s of its kernel variants on the same incoherent rays, with
records per ray, wave steps and lane utilisation, and a check that every variant returns the same hits.
usage: python tools/gpu_ray_service.py [million rays]     variants: split traversal (default), classic (PRGPU_TRACE_SPLIT=0).
       python tools/gpu_ray_service.py device             the host entry point against the one on device memory (below; profiles/ray_service_device.log)
(PRGPU_TRACE_TWO_RAYS=1 selected round 4's two-rays-per-lane experiment: profiles/r04_two_rays_per_lane.{log,patch}; the kernel is not in the tree.)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
DEVICE = sys.argv[1:2] == ["device"]
if DEVICE:
    import torch
from pearray_amd import backend, scene

N = 8 << 20 if DEVICE else int(float(sys.argv[1]) * 1e6) if len(sys.argv) > 1 else 8_000_000
sc = scene.cornell_soup(1920, 1080, spp=4, n_triangles=1_000_000)
rng = np.random.default_rng(11)
org = np.stack([rng.uniform(-0.9, 0.9, N), rng.uniform(-0.9, 0.9, N), rng.uniform(0.1, 1.8, N)], 1).astype(np.float32)
d = rng.normal(size=(N, 3)); d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def device_probe():
    """Wall time per batch of n incoherent rays, three ways in one process: prgpu_trace_closest on host arrays (nine allocations, four uploads,
    a synchronise, five downloads, nine frees per batch), prgpu_trace_closest_device on tensors that are resident (the answers stay on the
    device too), and the same with the hit's geometry.  Every batch ends in ONE synchronise; one warm-up round, then five rounds that alternate
    the three in a rotating order; median and min .. max.  The geometry kernel alone comes from the library's HIP events (prgpu_kernel_time_ms("geometry")),
    measured in a second pass with timing on, so that the events are not in the wall times."""
    g = backend.RenderContext(sc)
    t_org, t_dir = torch.from_numpy(org).cuda(), torch.from_numpy(d).cuda()
    g.reserveRays(N)
    print("ray service, host arrays against device tensors: 1 M-triangle scene, incoherent rays, wall ms per batch (one synchronise each), median [min .. max] of 5")
    for n in (4 << 10, 256 << 10, 8 << 20):
        o_h, d_h, o_d, d_d = org[:n], d[:n], t_org[:n], t_dir[:n]
        tmin_d, tmax_d = torch.full((n,), 1e-4, device="cuda"), torch.full((n,), float("inf"), device="cuda")

        def host_path():
            g.traceRays(o_h, d_h, 1e-4, np.inf)

        def device_path():
            g.traceRaysDevice(o_d, d_d, tmin_d, tmax_d)

        def device_geometry():
            g.traceRaysDevice(o_d, d_d, tmin_d, tmax_d, geometry=True)
        ways = (("host arrays", host_path), ("device tensors", device_path), ("device tensors + geometry", device_geometry))
        ms = {name: [] for name, _ in ways}
        for rep in range(6):   # round 0 warms up; the order within a round rotates, so that no way always runs behind the same neighbour
            for name, fn in ways[rep % 3:] + ways[:rep % 3]:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if rep:
                    ms[name].append((time.perf_counter() - t0) * 1e3)
        g.setTiming(True)
        k0, g0 = g.kernelTime("trace_closest"), g.kernelTime("geometry")
        for _ in range(5):
            device_geometry()
        torch.cuda.synchronize()
        k1, g1 = g.kernelTime("trace_closest"), g.kernelTime("geometry")
        g.setTiming(False)
        for name, _ in ways:
            v = np.sort(ms[name])
            print("n = %8d  %-26s %9.3f ms [%9.3f .. %9.3f]  %8.1f Mrays/s" % (n, name, np.median(v), v[0], v[-1], n / np.median(v) / 1e3), flush=True)
        print("n = %8d  kernels alone (HIP events, mean of 5): traversal %.3f ms, geometry %.3f ms = %.0f Mrays/s"
              % (n, (k1[0] - k0[0]) / 5, (g1[0] - g0[0]) / 5, n / max((g1[0] - g0[0]) / 5, 1e-9) / 1e3), flush=True)
    a = g.traceRays(org[:1 << 20], d[:1 << 20], 1e-4, np.inf)
    b = g.traceRaysDevice(t_org[:1 << 20], t_dir[:1 << 20], 1e-4, float("inf"))
    print("same answers on the first 1 Mi rays:", all(np.array_equal(x, y.cpu().numpy().view(x.dtype)) for x, y in zip(a, b)))
    g.close()


if DEVICE:
    device_probe()
    sys.exit(0)
ref = None
for name, env in (("split traversal (default)", {}), ("classic, one ray per lane", {"PRGPU_TRACE_SPLIT": "0"})):
    for k in ("PRGPU_TRACE_SPLIT", "PRGPU_TRACE_TWO_RAYS"):
        os.environ.pop(k, None)
    os.environ.update(env)
    g = backend.RenderContext(sc)
    g.setTiming(True)
    g.traceRays(org[:1 << 20], d[:1 << 20], 1e-4, np.inf)     # warm-up
    a, (ms0, n0) = g.traceCounters(), g.kernelTime("trace_closest")
    res = g.traceRays(org, d, 1e-4, np.inf)
    b, (ms1, n1) = g.traceCounters(), g.kernelTime("trace_closest")
    ms = ms1 - ms0
    recs = b["nodes_closest"] - a["nodes_closest"] + b["leaves_closest"] - a["leaves_closest"]
    steps = b["wave_steps_closest"] - a["wave_steps_closest"]
    same = "reference" if ref is None else str(all(np.array_equal(x, y) for x, y in zip(ref, res)))
    ref = ref or res
    print("%-28s %5.2f ms for %.1f M rays = %6.0f Mrays/s | %.1f inner + %.1f leaf records per ray, %.2f M wave steps, records per lane-step %.3f | same hits: %s"
          % (name, ms, N / 1e6, N / ms / 1e3, (b["nodes_closest"] - a["nodes_closest"]) / N, (b["leaves_closest"] - a["leaves_closest"]) / N, steps / 1e6,
             recs / max(64 * steps, 1), same), flush=True)
    g.close()
