"""What adaptive sampling by the filtered frame's pooled noise costs and buys on the MI355X: gpu_showcase at 1920x1080,
depth 8, cap --cap, steps of --step, one process, buffers warm.

  truth      a frame of --truth samples of another seed, rendered on the same device: the reference of every relative MSE below
             (per-pixel squared error over max(reference luminance, 0.01)^2, averaged: section 3.11's normalisation).
  uniform    the plain frame of --cap samples with the filter: the parent's way of rendering it, the yardstick of the frame times.
  frame      the parent's other mode, filtered_noise= (section 3.12), to the figure the uniform frame ends with: every sample, and its checks.
  rule       filtered_adaptive=T for T = --factors x the uniform frame's measured noise, pool 1, and pool 0 and 2 at the middle factor:
             total time, the time inside the checks (libptcore's PTCORE_VERBOSE notes at pt_end: checks_ms = gathers, pair filter and
             block map on devices[0]; keep_ms = keep_from_map_kernel + compact_kernel; the count stamp and the map's copies through the host
             are in neither, only in the frame's total),
             samples, counts, relative MSE of the filtered image.
  equal      at the samples each rule frame took: section 3.10's own-noise rule with its target bisected to the same total (within 3 %),
             and the uniform frame of the nearest sample count; relative MSE of both filtered images.
  The modes are alternated --reps times.

    python tools/filtered_adaptive_bench.py [--out profiles/filtered_adaptive_bench.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

NOTE = re.compile(r"filtered block checks[^\n]*? ([0-9.]+) ms in (\d+) launches")
KEEP = re.compile(r"adaptive check ([0-9.]+) ms in (\d+) launches")  # keep_from_map_kernel + compact_kernel, the slowest device's


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
    ap.add_argument("--cap", type=int, default=1024)
    ap.add_argument("--step", type=int, default=64)
    ap.add_argument("--truth", type=int, default=16384)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--factors", default="1.25,1.5,2.0")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build.build_core()
    sc = hip.FlatScene(scene.load(os.path.join(ROOT, "scenes", "gpu_showcase.json")))
    W, H = a.width, a.height
    img = np.zeros((H, W, 4), np.uint8)
    mean = np.zeros((H, W, 3))
    ac = hip.AtrousConfig(features=a.k)
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def rel_mse(m, ref):
        den = np.maximum(ref.sum(axis=2) / 3.0, 0.01)
        return float(np.mean(((m - ref) ** 2).mean(axis=2) / (den * den)))

    def run(ctx, spp, **kw):
        """One frame through hip.render with the filter; the row of its times, samples and relative MSE against the truth."""
        with Stderr() as err:
            t0 = time.perf_counter()
            st = hip.render(sc, hip.RenderConfig(W, H, spp, a.depth, 1), img, ctx=ctx, atrous=ac, noise_step=a.step, **kw)
            ms = (time.perf_counter() - t0) * 1e3
        hip.atrous(ctx, ac, None, mean)
        row = {"total_ms": ms, "device_ms": st["device_ms"], "samples": st["samples"], "spp_done": st["spp_done"],
               "spp_mean": st["samples"] / float(W * H), "rel_mse": rel_mse(mean, truth), "atrous_ms": st["atrous"]["atrous_ms"]}
        if "adaptive" in st:
            row.update(active_blocks=st["adaptive"]["active_blocks"], blocks=st["adaptive"]["blocks"], spp_min=st["adaptive"]["spp_min"])
        if "block_checks" in st:
            row["block_checks"] = st["block_checks"]
        if "filtered_noise" in st:
            row.update(filtered_noise=st["filtered_noise"], noise_model=st["noise_model"])
        m = NOTE.search(err.text)
        if m:
            row.update(checks_ms=float(m.group(1)), checks_timed=int(m.group(2)))
            k = KEEP.search(err.text)
            if k:
                row.update(keep_ms=float(k.group(1)))
        return row

    with capi.Context(ndev=1) as ctx:
        acc = np.zeros((H, W, 3))
        t0 = time.perf_counter()
        hip.render(sc, hip.RenderConfig(W, H, a.truth, a.depth, 2), img, None, acc, ctx=ctx)
        truth = acc / float(a.truth)
        del acc
        emit({"part": "truth", "spp": a.truth, "seed": 2, "ms": (time.perf_counter() - t0) * 1e3, "width": W, "height": H, "depth": a.depth})
        for _ in range(2):  # the first two frames size the buffers of the cap-sized frame (the second one grows them)
            run(ctx, a.cap)
        run(ctx, a.cap, halves=True)
        figure = hip.atrous_halves(ctx, ac)["noise"]
        targets = [float(f) * figure for f in a.factors.split(",")]
        mid = targets[len(targets) // 2]
        modes = [("uniform", a.cap, {}), ("frame", a.cap, dict(filtered_noise=figure))]
        modes += [("rule", a.cap, dict(filtered_adaptive=t, pool=1)) for t in targets]
        modes += [("rule", a.cap, dict(filtered_adaptive=mid, pool=p)) for p in (0, 2)]
        for _, spp, kw in modes:  # warm: the rule's buffers, the halves planes
            run(ctx, spp, **kw)
        took = {}
        for rep in range(a.reps):
            for name, spp, kw in modes:
                r = run(ctx, spp, **kw)
                r.update(part=name, rep=rep, cap=a.cap, step=a.step, k=a.k, **{k: v for k, v in kw.items()}, uniform_figure=figure)
                emit(r)
                if name == "rule":
                    took[(kw["filtered_adaptive"], kw["pool"])] = r["samples"]
        for (t, pool), samples in took.items():
            # section 3.10's own rule at the same samples: bisect its target (more samples for a smaller one)
            lo, hi, best = 0.0, 4.0, None
            for _ in range(12):
                tgt = 0.5 * (lo + hi)
                r = run(ctx, a.cap, noise=tgt, adaptive=True)
                if best is None or abs(r["samples"] - samples) < abs(best["samples"] - samples):
                    best = dict(r, own_target=tgt)
                if abs(r["samples"] - samples) <= 0.03 * samples:
                    break
                lo, hi = (tgt, hi) if r["samples"] > samples else (lo, tgt)
            best.update(part="equal", kind="own-noise rule", filtered_adaptive=t, pool=pool, rule_samples=samples,
                        within_3_percent=abs(best["samples"] - samples) <= 0.03 * samples)
            emit(best)
            n = max(4, int(round(samples / float(W * H))))
            r = run(ctx, n)
            r.update(part="equal", kind="uniform", filtered_adaptive=t, pool=pool, rule_samples=samples)
            emit(r)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
