"""128-byte leaves of up to three triangles against single-triangle 64-byte leaves (PRGPU_BVH_LEAF) over the scenes of tools/gpu_bvh_width.py:
scene creation time, ms per iteration, Msamples/s and inner / leaf records per closest and per occlusion ray under `3`, `1` and `auto`.  With
PRGPU_DEBUG_COUNTERS set the library prints the builder's prices and the instrumented kernel's time split (leaf steps, inner steps) to stderr after
each row: ticks per record of either kind = share of the wave time / records (device/bvh.hip, LEAF3_STEP_COST and LEAF1_STEP_COST).
usage: PRGPU_DEBUG_COUNTERS=1 python tools/gpu_bvh_leaf.py [scene ...] 2>&1     (GPU box; profiles/r06_single_leaf_ab.log)"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
from pearray_amd import backend
from gpu_bvh_width import SCENES


def run(sc, policy, iters=16):
    os.environ["PRGPU_BVH_LEAF"] = policy
    t = time.time()
    ctx = backend.RenderContext(sc)
    create_s = time.time() - t
    ctx.render(8); ctx.waitForFinish()
    best = 1e30
    for _ in range(3):
        t = time.time(); ctx.render(iters); ctx.waitForFinish()
        best = min(best, (time.time() - t) / iters * 1e3)
    a = ctx.traceCounters()
    ctx.setInstrumentation(True); ctx.render(4); ctx.waitForFinish(); ctx.setInstrumentation(False)
    sys.stdout.flush()
    b = ctx.traceCounters()     # (prints the time split of the instrumented launch under PRGPU_DEBUG_COUNTERS)
    d = {k: b[k] - a[k] for k in ("rays_closest", "rays_any", "nodes_closest", "nodes_any", "leaves_closest", "leaves_any")}
    rc, ra = max(d["rays_closest"], 1), max(d["rays_any"], 1)
    px = sc.desc.settings.width * sc.desc.settings.height
    row = dict(policy=policy, leaf_bytes=b["leaf_bytes"], create_s=create_s, ms=best, msamples=px / best / 1e3, inner_c=d["nodes_closest"] / rc, leaf_c=d["leaves_closest"] / rc,
               inner_a=d["nodes_any"] / ra, leaf_a=d["leaves_any"] / ra, width=ctx.pipelineInfo()["bvh_width"])
    ctx.close()
    return row


if __name__ == "__main__":
    print("%-9s %-5s | %9s | %8s %9s | %5s | %22s | %22s | %8s" % ("scene", "leaf", "leaf bytes", "ms/iter", "Msample/s", "width", "closest: inner, leaf", "occlusion: inner, leaf", "create s"))
    for name in (sys.argv[1:] or list(SCENES)):
        sc = SCENES[name]()
        rows = {}
        for policy in ("3", "1", "auto"):
            r = rows[policy] = run(sc, policy)
            print("%-9s %-5s | %9d | %8.3f %9.1f | %5d | %10.2f %10.2f  | %10.2f %10.2f  | %8.2f" % (name, policy, r["leaf_bytes"], r["ms"], r["msamples"], r["width"], r["inner_c"], r["leaf_c"],
                                                                                               r["inner_a"], r["leaf_a"], r["create_s"]), flush=True)
        print("%-9s single leaves against today's: time x %.3f; `auto` built %d-byte leaves and is %+.1f %% against `3`" % (name, rows["1"]["ms"] / rows["3"]["ms"], rows["auto"]["leaf_bytes"],
                                                                                                                         100.0 * (rows["auto"]["ms"] / rows["3"]["ms"] - 1.0)), flush=True)
