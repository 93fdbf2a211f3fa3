"""Measurements of the device BVH build: one object added per frame, the host builder against the device build, the two
arms alternated in one process; then unedited frames on either tree.  Prints the figures and writes them to OUT (default
bvh_device_build_measure.txt in the working directory; the recorded run is profiles/bvh_device_build_measure.txt).
    python tools/bvh_build_measure.py [N ...] [OUT]        (default N: 10000 100000 1000000)"""
import os
import sys
import time

import numpy as np
import torch  # noqa: F401  (one HIP runtime)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from path_trace_golang_amd import capi, hip, synth  # noqa: E402

ARGS = sys.argv[1:]
OUT = open(ARGS.pop() if ARGS and not ARGS[-1].isdigit() else "bvh_device_build_measure.txt", "w")
SIZES = [int(a) for a in ARGS] or [10 ** 4, 10 ** 5, 10 ** 6]
W, H, SPP, DEPTH = 1920, 1080, 16, 8


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    OUT.write(line + "\n")
    OUT.flush()


def frame(ctx, flat, seed, img):
    t0 = time.perf_counter()
    st = hip.render(flat, hip.RenderConfig(W, H, SPP, DEPTH, seed), img, ctx=ctx)
    return (time.perf_counter() - t0) * 1e3, st


def added(n, frames):
    t0 = time.perf_counter()
    flat = hip.FlatScene(synth.make_scene(n + frames, 4))
    total = flat.c.num_objects
    say("# %d objects: scene made and flattened in %.1f s (Python, not part of any figure)" % (n, time.perf_counter() - t0))
    img = np.zeros((H, W, 4), np.uint8)
    flat.c.num_objects = total - frames  # the last `frames` objects come in one per frame
    with capi.Context(ndev=1) as host, capi.Context(ndev=1) as dev:
        hip.set_bvh_build(dev, "device")
        arms = (("host", host), ("device", dev))
        for name, ctx in arms:
            for k in range(3):  # the build, then unchanged frames (warm code objects, grown buffers)
                ms, st = frame(ctx, flat, 1 + k, img)
            b = hip.bvh_build_stats(ctx)
            say("warm frame  %-6s wall %8.2f ms  device %8.2f ms  trace %8.2f ms | tree: builder %d nodes %d depth %d stack %d figure %.6g"
                % (name, ms, st["device_ms"], st["trace_ms"], b["builder"], b["nodes"], b["depth"], b["stack_need"], b["cost"]))
        rows = {"host": [], "device": []}
        for f in range(frames):
            flat.c.num_objects += 1
            for name, ctx in arms if f % 2 == 0 else arms[::-1]:
                ms, st = frame(ctx, flat, 10 + f, img)
                b = hip.bvh_build_stats(ctx)
                rows[name].append((ms, st["device_ms"], st["trace_ms"], b["prepare_ms"], b["device_ms"], b["builder"], b["upload_ms"], b["readback_ms"]))
        for name in ("host", "device"):
            a = np.array(rows[name])
            say("add one %-6s n=%d frames=%d  wall ms median %.2f min %.2f max %.2f | frame device ms median %.2f | trace ms median %.2f | "
                "preparation wall ms median %.2f | build device ms median %.3f | build upload wall ms median %.2f | build readback wall ms median %.2f | builder %s"
                % (name, n, frames, np.median(a[:, 0]), a[:, 0].min(), a[:, 0].max(), np.median(a[:, 1]), np.median(a[:, 2]), np.median(a[:, 3]),
                   np.median(a[:, 4]), np.median(a[:, 6]), np.median(a[:, 7]), sorted(set(int(x) for x in a[:, 5]))))
            say("   wall per frame:", " ".join("%.1f" % x for x in a[:, 0]))
        # unedited frames afterwards: what each tree costs to trace (the same scene and seeds in both arms, alternated)
        un = {"host": [], "device": []}
        for k in range(4):
            for name, ctx in arms if k % 2 == 0 else arms[::-1]:
                ms, st = frame(ctx, flat, 50 + k, img)
                un[name].append((ms, st["device_ms"], st["trace_ms"]))
        for name in ("host", "device"):
            a = np.array(un[name])
            say("unedited %-6s n=%d  wall ms median %.2f | frame device ms median %.2f | trace ms median %.2f"
                % (name, n, np.median(a[:, 0]), np.median(a[:, 1]), np.median(a[:, 2])))
        bh, bd = hip.bvh_build_stats(host), hip.bvh_build_stats(dev)
    with capi.Context(ndev=1) as fig:  # the host-built tree's figure: computed only with the refit on, so taken outside the timed arms
        hip.set_bvh_refit(fig, float("inf"))
        frame(fig, flat, 1, img)
        host_cost = hip.bvh_refit_stats(fig)["cost_built"]
    say("trees n=%d  host: nodes %d depth %d stack %d figure %.6g | device: nodes %d depth %d stack %d figure %.6g (x%.3f)" % (
        n, bh["nodes"], bh["depth"], bh["stack_need"], host_cost, bd["nodes"], bd["depth"], bd["stack_need"], bd["cost"], bd["cost"] / host_cost))


if __name__ == "__main__":
    say("# 1080p, 16 spp, depth 8, one device; wall = host clock around hip.render (ends in a synchronise)")
    for n in SIZES:
        added(n, 6 if n < 10 ** 6 else 4)
    say("# done")
