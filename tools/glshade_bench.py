"""GL shading cost on the MI355X: gpu_showcase at 1920x1080, 4 passes (16 paths each), depth 8, GL shading off (the CPU
engine at 4 spp) and on alternated in one process, three frames each (after one warm-up of each).  Prints one JSON line
per frame and a summary line: ms per frame (off / on), gl_ms from pt_shading_last_stats, paths / segments / shadow rays
per second of gl_trace_kernel time, and the kernel's VGPRs, scratch and waves per SIMD (tools/kernel_regs.py).

    python tools/glshade_bench.py [--passes 4] [--out profiles/r06_glshade_bench.jsonl] [--no-regs]
"""
from __future__ import annotations

import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernel_resources() -> dict:
    """gl_trace_kernel's line of tools/kernel_regs.py (a device-only compile; no GPU needed)."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py")], capture_output=True, text=True,
                         check=True).stdout
    line = next(ln for ln in out.splitlines() if "gl_trace_kernel" in ln)
    m = re.search(r"vgpr\s+(\d+) \(<=(\d+) waves/SIMD\) sgpr\s+(\d+) spill v(\d+) s(\d+) lds\s+(\d+) scratch (\d+)", line)
    keys = ("vgpr", "waves_per_simd", "sgpr", "vgpr_spill", "sgpr_spill", "lds", "scratch")
    return dict(zip(keys, (int(v) for v in m.groups()))) if m else {"line": line}


def main() -> None:
    import numpy as np
    import torch  # noqa: F401  (one HIP runtime with torch, see capi.py)

    from path_trace_golang_amd import build, capi, hip, scene

    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-regs", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build.build_core()
    sc = scene.load(os.path.join(ROOT, "scenes", "gpu_showcase.json"))
    img = np.zeros((a.height, a.width, 4), np.uint8)
    cfg = hip.RenderConfig(a.width, a.height, a.passes, a.depth, 1)
    rows = []
    with capi.Context(ndev=1) as ctx:
        for rep in range(a.reps + 1):
            for shading in ("cpu", "gl"):
                t0 = time.perf_counter()
                st = hip.render(sc, cfg, img, ctx=ctx, shading=shading)
                ms = (time.perf_counter() - t0) * 1e3
                gst = hip.shading_last_stats(ctx)
                row = {"rep": rep, "shading": shading, "ms": ms, "device_ms": st["device_ms"], "trace_ms": st["trace_ms"],
                       "resolve_ms": st["resolve_ms"], "samples": st["samples"], "segments": st["segments"],
                       **{"gl_" + k if not k.startswith("gl") else k: v for k, v in gst.items()}}
                if shading == "gl" and gst["gl_ms"] > 0:
                    s = gst["gl_ms"] * 1e-3
                    row.update(paths_per_s=gst["paths"] / s, segments_per_s=gst["segments"] / s,
                               shadow_rays_per_s=gst["shadow_rays"] / s)
                if rep > 0:
                    rows.append(row)
                print(json.dumps(row), flush=True)
    off = [r for r in rows if r["shading"] == "cpu"]
    on = [r for r in rows if r["shading"] == "gl"]
    med = lambda k: float(np.median([r[k] for r in on]))  # noqa: E731
    summ = {"summary": True, "scene": "gpu_showcase", "width": a.width, "height": a.height, "passes": a.passes, "depth": a.depth,
            "ms_off": sorted(r["ms"] for r in off), "ms_on": sorted(r["ms"] for r in on), "gl_ms": sorted(r["gl_ms"] for r in on),
            "paths": on[0]["gl_paths"], "segments": on[0]["gl_segments"], "shadow_rays": on[0]["gl_shadow_rays"],
            "probe_rays": on[0]["gl_probe_rays"], "paths_per_s": med("paths_per_s"), "segments_per_s": med("segments_per_s"),
            "shadow_rays_per_s": med("shadow_rays_per_s")}
    if not a.no_regs:
        summ["gl_trace_kernel"] = kernel_resources()
    print(json.dumps(summ), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
            f.write(json.dumps(summ) + "\n")


if __name__ == "__main__":
    main()
