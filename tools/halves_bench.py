"""Cost of the half-buffer sums and of the pair filter on the MI355X: gpu_showcase at 1920x1080, depth 8, one process.

  collect    frames of --spp samples with moments on, halves off and on alternated, --reps each after one warm-up of each: ms per
             frame and the time inside halves_kernel (libptcore's PTCORE_VERBOSE note at pt_end) in the same run.
  pair       on the last halves frame (k = --k feature samples): pt_atrous_halves at the defaults, --reps calls (pt_halves_stats.atrous_ms
             = the call's launches, and the call's wall time, which adds the gathers), pt_atrous on the same frame beside it, then one
             pair call each with 0 .. 5 iterations: the differences are the times of the single atrous_pair_kernel launches at steps
             1, 2, 4, 8, 16, and the 0-iteration call is the pair prep + the combine.
  use        a frame of --cap samples with halves on and its pt_atrous_halves figure; then hip.render to that figure as the
             filtered_noise target (cap --cap, steps of --step): frame time with the checks in it, the samples taken, and noise
             against noise_model at the stop.  Neither figure sees the bias the filter adds.

    python tools/halves_bench.py [--skip collect,pair,use] [--out profiles/halves_bench.jsonl]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

NOTE = re.compile(r"halves_kernel ([0-9.]+) ms in (\d+) launches")


def main() -> None:
    import numpy as np
    import torch  # noqa: F401  (one HIP runtime with torch, see capi.py)

    os.environ["PTCORE_VERBOSE"] = "1"  # read when the frame ends
    from moments_bench import Stderr
    from path_trace_golang_amd import build, capi, hip, scene

    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cap", type=int, default=1024)
    ap.add_argument("--step", type=int, default=64)
    ap.add_argument("--skip", default="", help="comma list of parts to skip: collect, pair, use")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    skip = set(x for x in a.skip.split(",") if x)
    build.build_core()
    L = capi.load()
    full = scene.load(os.path.join(ROOT, "scenes", "gpu_showcase.json"))
    sc = hip.FlatScene(full)
    W, H = a.width, a.height
    img = np.zeros((H, W, 4), np.uint8)
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def frame(ctx, halves, k=0, spp=None):
        hip.set_moments(ctx, True)
        hip.set_adaptive(ctx, None)
        hip.set_features(ctx, k)
        hip.set_halves(ctx, halves)
        pc = hip.pt_config(hip.RenderConfig(W, H, spp or a.spp, a.depth, 1))
        st = capi.PtStats()
        with Stderr() as err:
            t0 = time.perf_counter()
            capi.check(L.pt_render(ctx.handle, C.byref(sc.c), C.byref(pc), img.ctypes.data_as(C.c_void_p), int(img.strides[0]), None, None, None,
                                   C.byref(st)))
            ms = (time.perf_counter() - t0) * 1e3
        row = {"ms": ms, "device_ms": st.device_ms, "trace_ms": st.trace_ms, "resolve_ms": st.resolve_ms, "spp_chunk": st.spp_chunk,
               "samples": st.samples, "halves": halves}
        m = NOTE.search(err.text)
        if m:
            row.update(halves_ms=float(m.group(1)), halves_launches=int(m.group(2)))
        return row

    def pair(ctx, iterations=5):
        t0 = time.perf_counter()
        st = hip.atrous_halves(ctx, hip.AtrousConfig(iterations=iterations))
        st["wall_ms"] = (time.perf_counter() - t0) * 1e3
        return st

    with capi.Context(ndev=1) as ctx:
        if "collect" not in skip:
            for rep in range(a.reps + 1):
                for on in (False, True):
                    r = frame(ctx, on)
                    r.update(part="collect", rep=rep)
                    if rep > 0:
                        emit(r)
            off = sorted(r["ms"] for r in rows if r["part"] == "collect" and not r["halves"])
            on = [r for r in rows if r["part"] == "collect" and r["halves"]]
            emit({"part": "collect", "summary": True, "spp": a.spp, "ms_off": off, "ms_on": sorted(r["ms"] for r in on),
                  "ratio_of_medians": float(np.median([r["ms"] for r in on]) / np.median(off)),
                  "halves_ms": sorted(r.get("halves_ms", -1.0) for r in on), "halves_launches": on[0].get("halves_launches")})
        if "pair" not in skip:
            frame(ctx, True, a.k)
            pair(ctx)  # warm-up: allocates the planes
            hip.atrous(ctx, hip.AtrousConfig(), img)
            for rep in range(a.reps):
                r = pair(ctx)
                r.update(part="pair", kind="defaults", rep=rep + 1, width=W, height=H, k=a.k)
                emit(r)
                t0 = time.perf_counter()
                s1 = hip.atrous(ctx, hip.AtrousConfig(), img)
                emit({"part": "pair", "kind": "pt_atrous beside it", "rep": rep + 1, "atrous_ms": s1["atrous_ms"],
                      "wall_ms": (time.perf_counter() - t0) * 1e3, "noise_after": s1["noise_after"]})
            per = [pair(ctx, t)["atrous_ms"] for t in range(6)]
            emit({"part": "pair", "kind": "by iterations", "atrous_ms": per, "fixed_ms": per[0],
                  "kernel_ms_by_step": {str(1 << t): per[t + 1] - per[t] for t in range(5)}})
        if "use" not in skip:
            cfg = hip.RenderConfig(W, H, a.cap, a.depth, 1)
            ac = hip.AtrousConfig(features=a.k)
            target = None
            for rep in range(3):  # the first two frames size the buffers of the cap-sized frame (the second one grows them)
                r = frame(ctx, True, a.k, a.cap)
                p = pair(ctx)
                target = p["noise"]
                if rep > 1:
                    emit({"part": "use", "kind": "cap frame", "cap": a.cap, "frame_ms": r["ms"], "noise": p["noise"], "noise_model": p["noise_model"],
                          "pair_ms": p["atrous_ms"], "pair_wall_ms": p["wall_ms"]})
            for rep in range(2):
                t0 = time.perf_counter()
                st = hip.render(sc, cfg, img, ctx=ctx, atrous=ac, filtered_noise=target, noise_step=a.step)
                ms = (time.perf_counter() - t0) * 1e3
                emit({"part": "use", "kind": "to the target", "rep": rep, "target": target, "cap": a.cap, "step": a.step, "k": a.k, "total_ms": ms,
                      "spp_done": st["spp_done"], "samples": st["samples"], "filtered_noise": st["filtered_noise"], "noise_model": st["noise_model"],
                      "noise_unfiltered": st["noise"], "noise_after": st["atrous"]["noise_after"], "atrous_ms": st["atrous"]["atrous_ms"]})
            hip.set_halves(ctx, False)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
