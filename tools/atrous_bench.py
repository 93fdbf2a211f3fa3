"""Cost of the first-hit feature planes and of the a-trous filter on the MI355X: gpu_showcase at 1920x1080, depth 8,
one process.

  features   frames of --spp samples with moments on, features off and k = --k alternated, --reps each after one warm-up of each:
             ms per frame and the time inside feature_kernel (libptcore's PTCORE_VERBOSE note at pt_end) in the same run.
  filter     on the last k = --k frame: pt_atrous at the defaults, --reps calls (pt_atrous_stats.atrous_ms = the filter's launches,
             and the call's wall time, which adds the gathers and the copies out), then one call each with 0 .. 5 iterations: the
             differences are the times of the single atrous_kernel launches at steps 1, 2, 4, 8, 16, and the 0-iteration call is
             prep + the two noise reductions + finish.
  use        an adaptive frame (cap --cap, --step samples per step) at a block target --loosen times the one recorded in
             profiles/adaptive_bench.jsonl, with k = --k, then pt_atrous: wall time of both and noise_after, beside the recorded
             adaptive frame at the tight target.

    python tools/atrous_bench.py [--out profiles/atrous_bench.jsonl]
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

NOTE = re.compile(r"feature_kernel ([0-9.]+) ms in (\d+) launches")


def recorded_adaptive():
    """(target, ms, noise) of the adaptive frame recorded in profiles/adaptive_bench.jsonl."""
    with open(os.path.join(ROOT, "profiles", "adaptive_bench.jsonl")) as f:
        for line in f:
            r = json.loads(line)
            if r.get("part") == "gain" and r.get("kind") == "adaptive":
                return r["target"], r["ms"], r["noise"]
    raise SystemExit("profiles/adaptive_bench.jsonl holds no adaptive gain row")


def main() -> None:
    import numpy as np
    import torch  # noqa: F401  (one HIP runtime with torch, see capi.py)

    os.environ["PTCORE_VERBOSE"] = "1"  # read when the frame ends
    from adaptive_bench import Stderr
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
    ap.add_argument("--loosen", type=float, default=2.0)
    ap.add_argument("--skip", default="", help="comma list of parts to skip: features, filter, use")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    skip = set(x for x in a.skip.split(",") if x)
    build.build_core()
    L = capi.load()
    sc = hip.FlatScene(scene.load(os.path.join(ROOT, "scenes", "gpu_showcase.json")))
    W, H = a.width, a.height
    img = np.zeros((H, W, 4), np.uint8)
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def frame(ctx, k):
        hip.set_moments(ctx, True)
        hip.set_adaptive(ctx, None)
        hip.set_features(ctx, k)
        pc = hip.pt_config(hip.RenderConfig(W, H, a.spp, a.depth, 1))
        st = capi.PtStats()
        with Stderr() as err:
            t0 = time.perf_counter()
            capi.check(L.pt_render(ctx.handle, C.byref(sc.c), C.byref(pc), img.ctypes.data_as(C.c_void_p), int(img.strides[0]), None, None, None,
                                   C.byref(st)))
            ms = (time.perf_counter() - t0) * 1e3
        row = {"ms": ms, "device_ms": st.device_ms, "trace_ms": st.trace_ms, "raygen_ms": st.raygen_ms, "resolve_ms": st.resolve_ms,
               "spp_chunk": st.spp_chunk, "samples": st.samples, "k": k}
        m = NOTE.search(err.text)
        if m:
            row.update(feature_ms=float(m.group(1)), feature_launches=int(m.group(2)))
        return row

    def filtered(ctx, iterations=5):
        t0 = time.perf_counter()
        st = hip.atrous(ctx, hip.AtrousConfig(iterations=iterations), img)
        st["wall_ms"] = (time.perf_counter() - t0) * 1e3
        return st

    with capi.Context(ndev=1) as ctx:
        if "features" not in skip:
            for rep in range(a.reps + 1):
                for k in (0, a.k):
                    r = frame(ctx, k)
                    r.update(part="features", rep=rep)
                    if rep > 0:
                        emit(r)
            off = sorted(r["ms"] for r in rows if r["part"] == "features" and r["k"] == 0)
            on = [r for r in rows if r["part"] == "features" and r["k"] == a.k]
            emit({"part": "features", "summary": True, "spp": a.spp, "k": a.k, "ms_off": off, "ms_on": sorted(r["ms"] for r in on),
                  "ratio_of_medians": float(np.median([r["ms"] for r in on]) / np.median(off)),
                  "feature_ms": sorted(r.get("feature_ms", -1.0) for r in on), "feature_launches": on[0].get("feature_launches")})
        if "filter" not in skip:
            frame(ctx, a.k)
            filtered(ctx)  # warm-up: allocates the filter's planes
            for rep in range(a.reps):
                r = filtered(ctx)
                r.update(part="filter", kind="defaults", rep=rep + 1, width=W, height=H, k=a.k)
                emit(r)
            per = [filtered(ctx, t)["atrous_ms"] for t in range(6)]
            emit({"part": "filter", "kind": "by iterations", "atrous_ms": per, "fixed_ms": per[0],
                  "kernel_ms_by_step": {str(1 << t): per[t + 1] - per[t] for t in range(5)}})
        if "use" not in skip:
            target, rec_ms, rec_noise = recorded_adaptive()
            loose = target * a.loosen
            for rep in range(3):  # the first two frames size the buffers of the cap-sized frame (the second one grows them)
                hip.set_moments(ctx, True)
                hip.set_features(ctx, a.k)
                hip.set_adaptive(ctx, loose, 0, a.step)
                pc = hip.pt_config(hip.RenderConfig(W, H, a.cap, a.depth, 1))
                st = capi.PtStats()
                t0 = time.perf_counter()
                capi.check(L.pt_render(ctx.handle, C.byref(sc.c), C.byref(pc), img.ctypes.data_as(C.c_void_p), int(img.strides[0]), None, None,
                                       None, C.byref(st)))
                frame_ms = (time.perf_counter() - t0) * 1e3
                f = filtered(ctx)
                state = hip.adaptive_state(ctx)
                if rep > 1:
                    emit({"part": "use", "target": loose, "cap": a.cap, "step": a.step, "k": a.k, "frame_ms": frame_ms, "atrous_wall_ms": f["wall_ms"],
                          "atrous_ms": f["atrous_ms"], "total_ms": frame_ms + f["wall_ms"], "samples": st.samples, "noise_unfiltered": f["noise_before"],
                          "noise_after": f["noise_after"], "state": state, "recorded_adaptive": {"target": target, "ms": rec_ms, "noise": rec_noise}})
            hip.set_adaptive(ctx, None)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
