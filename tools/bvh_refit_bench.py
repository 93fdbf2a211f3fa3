"""Measurements of the BVH refit: drag of one object per frame, refit on against off, arms alternated in one process;
trace time on a refitted tree against a rebuilt one.  Prints the figures and writes them to OUT (default bvh_refit_measure.txt in the
working directory; the recorded run is profiles/bvh_refit_measure.txt).
    python tools/bvh_refit_bench.py [all | drag | degrade | big] [OUT]"""
import math
import os
import sys
import time

import numpy as np
import torch  # noqa: F401  (one HIP runtime)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from path_trace_golang_amd import capi, hip, synth  # noqa: E402

OUT = open(sys.argv[2] if len(sys.argv) > 2 else "bvh_refit_measure.txt", "w")
OBJ = np.dtype([("type", "<i4"), ("material", "<i4"), ("position", "<f8", 3), ("size", "<f8", 3)])
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


def drag(n, frames):
    t0 = time.perf_counter()
    sc = synth.make_scene(n, 4)
    flat = hip.FlatScene(sc)
    objs = np.frombuffer(flat.objects, dtype=OBJ)
    say("# %d objects: scene made and flattened in %.1f s (Python, not part of any figure)" % (n, time.perf_counter() - t0))
    img = np.zeros((H, W, 4), np.uint8)
    free = len(objs) - 7
    with capi.Context(ndev=1) as off, capi.Context(ndev=1) as on:
        hip.set_bvh_refit(on, math.inf)
        for ctx in (off, on):
            for k in range(3):  # the build, then unchanged frames (warm code objects, grown buffers)
                ms, st = frame(ctx, flat, 1 + k, img)
            say("warm frame  %-5s wall %8.2f ms  device %8.2f ms  trace %8.2f ms" % ("on" if ctx is on else "off", ms, st["device_ms"], st["trace_ms"]))
        rows = {"off": [], "on": []}
        for f in range(frames):
            objs["position"][free][0] += 0.01  # one object dragged by a little
            for name, ctx in (("off", off), ("on", on)) if f % 2 == 0 else (("on", on), ("off", off)):
                ms, st = frame(ctx, flat, 10 + f, img)
                rs = hip.bvh_refit_stats(ctx)
                rows[name].append((ms, st["device_ms"], st["trace_ms"], rs["refit_ms"], rs["last_action"], rs["cost_now"] / rs["cost_built"] if rs["cost_built"] else 0.0))
        for name in ("off", "on"):
            a = np.array(rows[name])
            say("drag %-3s n=%d frames=%d  wall ms median %.2f min %.2f max %.2f | device ms median %.2f | trace ms median %.2f | refit device ms median %.3f | action %s | figure ratio %.6f"
                % (name, n, frames, np.median(a[:, 0]), a[:, 0].min(), a[:, 0].max(), np.median(a[:, 1]), np.median(a[:, 2]), np.median(a[:, 3]),
                   sorted(set(int(x) for x in a[:, 4])), a[-1, 5]))
            say("   wall per frame:", " ".join("%.1f" % x for x in a[:, 0]))
        # unchanged scene: what a frame costs when the preparation does nothing (the host share of the arms above is wall minus this)
        for name, ctx in (("off", off), ("on", on)):
            t = [frame(ctx, flat, 50 + k, img)[0] for k in range(3)]
            say("unchanged %-3s wall ms %s" % (name, " ".join("%.2f" % x for x in t)))
    return sc


def degrade(n):
    """Trace time on a refitted tree against a rebuilt one, the same scene and seed in both."""
    sc = synth.make_scene(n, 4)
    flat = hip.FlatScene(sc)
    objs = np.frombuffer(flat.objects, dtype=OBJ)
    base = objs.copy()
    img = np.zeros((H, W, 4), np.uint8)
    rng = np.random.default_rng(9)
    free = np.arange(5, len(objs))

    def compare(tag, on):
        ms_on = [frame(on, flat, 70 + k, img) for k in range(3)]
        ratio = hip.bvh_refit_stats(on)
        with capi.Context(ndev=1) as fresh:
            ms_off = [frame(fresh, flat, 70 + k, img) for k in range(3)]
        t_on = np.median([s["trace_ms"] for _, s in ms_on[1:]])
        t_off = np.median([s["trace_ms"] for _, s in ms_off[1:]])
        d_on = np.median([s["device_ms"] for _, s in ms_on[1:]])
        d_off = np.median([s["device_ms"] for _, s in ms_off[1:]])
        say("degrade n=%d %-28s figure ratio %.4f | trace ms refitted %.2f rebuilt %.2f (x%.3f) | device ms refitted %.2f rebuilt %.2f | refits %d builds %d"
            % (n, tag, ratio["cost_now"] / ratio["cost_built"], t_on, t_off, t_on / t_off, d_on, d_off, ratio["refits"], ratio["builds"]))

    with capi.Context(ndev=1) as on:
        hip.set_bvh_refit(on, math.inf)
        frame(on, flat, 1, img)
        step = 0
        for target in (1, 8, 64):
            while step < target:
                objs["position"][free[-3]][0] += 0.25
                step += 1
                if step < target:
                    frame(on, flat, 2, img)
            compare("%d drag steps of 0.25" % target, on)
    for share in (0.01, 0.1, 1.0):
        objs[:] = base
        with capi.Context(ndev=1) as on:
            hip.set_bvh_refit(on, math.inf)
            frame(on, flat, 1, img)
            pick = rng.choice(free, max(1, int(share * len(free))), replace=False)
            d = rng.standard_normal((len(pick), 3))
            d /= np.linalg.norm(d, axis=1)[:, None]
            size = np.maximum(objs["size"][pick].max(axis=1), 1e-3)
            objs["position"][pick] += d * size[:, None]
            compare("%g %% moved by their size" % (100 * share), on)


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    say("# 1080p, 16 spp, depth 8, one device; wall = host clock around hip.render (ends in a synchronise)")
    if which in ("all", "drag"):
        drag(10 ** 4, 10)
        drag(10 ** 5, 10)
    if which in ("all", "degrade"):
        degrade(10 ** 5)
    if which in ("all", "big"):
        drag(10 ** 6, 4)
    say("# done")
