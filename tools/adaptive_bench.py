"""Cost and gain of adaptive sampling on the MI355X: gpu_showcase at 1920x1080, depth 8, one process.

  overhead   plain frames with moments on and adaptive frames with target 0 and min_spp = the frame's samples (every block
             stays active to the end -- target 0 alone would stop the blocks of constant colour, whose noise is exactly 0 --
             so both trace the same samples) alternated, --reps each after one warm-up of each: ms per frame, resolve_kernel's add
             (pt_stats.resolve_ms) and the time of the per-step check (block_noise_kernel + compact_kernel, libptcore's
             PTCORE_VERBOSE note at pt_end) in the same run.
  gain       the frame noise of the plain --ref-spp frame is the target; then, cap --cap and --step samples per step, the
             frame-level stop (pt_noise_estimate after every step) against the adaptive stop: wall time, samples traced, the
             histogram of the per-block counts, and per step the active blocks and the wall time (late steps are small
             launches).

    python tools/adaptive_bench.py [--out profiles/adaptive_bench.jsonl]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NOTE = re.compile(r"adaptive check ([0-9.]+) ms in (\d+) launches")


class Stderr:
    """Redirects the process's stderr (the library writes to fd 2) into a file while active; .text afterwards."""

    def __enter__(self):
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        sys.stderr.flush()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *a):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode("utf-8", "replace")
        self.tmp.close()


def main() -> None:
    import numpy as np
    import torch  # noqa: F401  (one HIP runtime with torch, see capi.py)

    os.environ["PTCORE_VERBOSE"] = "1"  # read when the frame ends
    from path_trace_golang_amd import build, capi, hip, scene

    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--spp", type=int, default=1024, help="overhead part: samples per frame")
    ap.add_argument("--overhead-step", type=int, default=64, help="overhead part: samples per step of both kinds of frame")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cap", type=int, default=1024)
    ap.add_argument("--step", type=int, default=64)
    ap.add_argument("--ref-spp", type=int, default=256)
    ap.add_argument("--skip", default="", help="comma list of parts to skip: overhead, gain")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    skip = set(x for x in a.skip.split(",") if x)
    build.build_core()
    L = capi.load()
    sc = hip.FlatScene(scene.load(os.path.join(ROOT, "scenes", "gpu_showcase.json")))
    W, H = a.width, a.height
    img = np.zeros((H, W, 4), np.uint8)
    counts = np.zeros((H, W), np.uint32)
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def stepped(ctx, cap, step, adaptive_target=None, frame_target=None, min_spp=0):
        """One pt_begin ... pt_end frame in steps of `step`: plain with moments, adaptive, or with the frame-level stop."""
        hip.set_moments(ctx, True)
        hip.set_adaptive(ctx, adaptive_target, min_spp, step)
        pc = hip.pt_config(hip.RenderConfig(W, H, cap, a.depth, 1))
        st = capi.PtStats()
        nz = capi.PtNoise()
        done, steps, excl = C.c_int32(0), [], 0.0
        with Stderr() as err:
            t0 = time.perf_counter()
            capi.check(L.pt_begin(ctx.handle, C.byref(sc.c), C.byref(pc)))
            while done.value < cap:
                before, ts = done.value, time.perf_counter()
                capi.check(L.pt_step(ctx.handle, step, C.byref(done)))
                if done.value == before:
                    break
                rec = {"done": done.value, "ms": (time.perf_counter() - ts) * 1e3}
                if adaptive_target is not None:  # (a small read-back for the record: its time is taken out of the frame's)
                    tq = time.perf_counter()
                    rec["active_after"] = hip.adaptive_state(ctx)["active_blocks"]
                    excl += time.perf_counter() - tq
                steps.append(rec)
                if frame_target is not None:
                    capi.check(L.pt_noise_estimate(ctx.handle, C.byref(nz)))
                    if done.value >= 2 and nz.noise <= frame_target:
                        break
            capi.check(L.pt_read(ctx.handle, img.ctypes.data_as(C.c_void_p), int(img.strides[0]), None))
            capi.check(L.pt_end(ctx.handle, C.byref(st)))
            ms = (time.perf_counter() - t0 - excl) * 1e3
        row = {"ms": ms, "device_ms": st.device_ms, "trace_ms": st.trace_ms, "raygen_ms": st.raygen_ms, "resolve_ms": st.resolve_ms,
               "resolve_launches": st.resolve_launches, "spp_chunk": st.spp_chunk, "samples": st.samples, "segments": st.segments,
               "spp_done": done.value, "noise": hip.noise_estimate(ctx)["noise"], "steps": steps}
        m = NOTE.search(err.text)
        if m:
            row.update(check_ms=float(m.group(1)), check_launches=int(m.group(2)))
        if adaptive_target is not None:
            row["state"] = hip.adaptive_state(ctx)
            hip.read_sample_counts(ctx, counts)
            v, c = np.unique(counts[::8, ::8], return_counts=True)
            row["block_histogram"] = {int(k): int(n) for k, n in zip(v, c)}
        return row

    with capi.Context(ndev=1) as ctx:
        if "overhead" not in skip:
            for rep in range(a.reps + 1):
                for kind in ("plain+moments", "adaptive target 0"):
                    r = stepped(ctx, a.spp, a.overhead_step, adaptive_target=0.0 if kind.startswith("adaptive") else None, min_spp=a.spp)
                    r.pop("steps")
                    r.update(part="overhead", kind=kind, rep=rep)
                    if rep > 0:
                        emit(r)
            plain = sorted(r["ms"] for r in rows if r.get("kind") == "plain+moments")
            adap = [r for r in rows if r.get("kind") == "adaptive target 0"]
            emit({"part": "overhead", "summary": True, "spp": a.spp, "step": a.overhead_step, "ms_plain": plain,
                  "ms_adaptive": sorted(r["ms"] for r in adap), "ratio_of_medians": float(np.median([r["ms"] for r in adap]) / np.median(plain)),
                  "check_ms": sorted(r.get("check_ms", -1.0) for r in adap), "resolve_ms": sorted(r["resolve_ms"] for r in adap),
                  "check_launches": adap[0].get("check_launches"), "resolve_launches": adap[0]["resolve_launches"]})
        if "gain" not in skip:
            ref = stepped(ctx, a.ref_spp, a.ref_spp)
            target = ref["noise"]
            emit({"part": "gain", "kind": "plain reference", "spp": a.ref_spp, "ms": ref["ms"], "samples": ref["samples"], "noise": target})
            for rep in range(2):  # the first pair warms the buffers of the cap-sized frame up
                for kind in ("frame stop", "adaptive"):
                    r = stepped(ctx, a.cap, a.step, adaptive_target=target if kind == "adaptive" else None,
                                frame_target=target if kind == "frame stop" else None)
                    r.update(part="gain", kind=kind, rep=rep, target=target, cap=a.cap, step=a.step)
                    if rep > 0:
                        emit(r)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
