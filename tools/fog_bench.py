"""Fog cost on the MI355X: gpu_showcase at 1920x1080, depth 8, fog off and fog on alternated in one process, three
frames each (after one warm-up of each).  Prints one JSON line per frame and a summary line:
  ms per frame (off / on), fog_ms and launches from pt_fog_last_stats, shadow rays per second of fog_kernel time,
  and the fog kernel's algorithmic FP64 rate against the FP64 vector peak (fp64_ops() below).

    python tools/fog_bench.py [--spp 16] [--out profiles/r05_fog_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# FP64 vector peak of the MI355X without fused multiply-add (39.3 Tflop/s, the unfused peak bench.py uses); every
# operation below counts 1 -- the kernel is built without contraction.
FP64_PEAK = 39.3e12


def fp64_ops(st: dict, nobj_kinds: dict, nlights: int) -> float:
    """Algorithmic FP64 operations of one frame's fog_kernel, from its counters.  Per shadow ray, per object tested (the
    object loop is left early only when a whole wave is occluded, so every object is counted: an upper bound on the
    work issued): sphere 19 (+ sqrt and two divisions when the discriminant is >= 0, counted as 1 each), plane 9,
    box 18.  Per light sample before the occlusion test 40 (sphere sampling with sin/cos polynomials ~25, distance,
    direction, cosine); per unoccluded light 30 (phase, geometry, contribution).  Per march step 25 (+ 3 octaves x 30
    for the noise, exp 20).  Divisions and square roots are counted as one operation, which understates their cost."""
    per_ray = 19 * nobj_kinds.get("sphere", 0) + 9 * nobj_kinds.get("plane", 0) + 18 * nobj_kinds.get("box", 0)
    draws = st["draws"] / 2  # light samples
    return st["shadow_rays"] * (per_ray + 30) + draws * 40 + st["steps"] * (25 + 90 + 20)


def main() -> None:
    import numpy as np
    import torch  # noqa: F401  (one HIP runtime with torch, see capi.py)

    from path_trace_golang_amd import build, capi, hip, scene

    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build.build_core()
    sc = scene.load(os.path.join(ROOT, "scenes", "gpu_showcase.json"))
    kinds = {}
    for o in sc.objects:
        k = "sphere" if o.type in ("sphere", "sphere_light") else o.type
        kinds[k] = kinds.get(k, 0) + 1
    nlights = sum(1 for o in sc.objects if o.type in ("sphere", "sphere_light") and "light" in o.material_id)
    img = np.zeros((a.height, a.width, 4), np.uint8)
    cfg = hip.RenderConfig(a.width, a.height, a.spp, a.depth, 1)
    rows = []
    with capi.Context(ndev=1) as ctx:
        for rep in range(a.reps + 1):
            for fog in (False, True):
                t0 = time.perf_counter()
                st = hip.render(sc, cfg, img, ctx=ctx, fog=fog)
                ms = (time.perf_counter() - t0) * 1e3
                fst = hip.fog_last_stats(ctx)
                row = {"rep": rep, "fog": fog, "ms": ms, "device_ms": st["device_ms"], "trace_ms": st["trace_ms"],
                       "segments": st["segments"], **{"fog_" + k if not k.startswith("fog") else k: v for k, v in fst.items()}}
                if fog and fst["fog_ms"] > 0:
                    ops = fp64_ops({"shadow_rays": fst["shadow_rays"], "draws": fst["draws"], "steps": fst["steps"]}, kinds, nlights)
                    row["shadow_rays_per_s"] = fst["shadow_rays"] / (fst["fog_ms"] * 1e-3)
                    row["fp64_ops"] = ops
                    row["fp64_rate"] = ops / (fst["fog_ms"] * 1e-3)
                    row["fp64_frac"] = row["fp64_rate"] / FP64_PEAK
                if rep > 0:
                    rows.append(row)
                print(json.dumps(row), flush=True)
    off = [r["ms"] for r in rows if not r["fog"]]
    on = [r for r in rows if r["fog"]]
    summ = {"summary": True, "scene": "gpu_showcase", "width": a.width, "height": a.height, "spp": a.spp, "depth": a.depth,
            "ms_off": sorted(off), "ms_on": sorted(r["ms"] for r in on), "fog_ms": sorted(r["fog_ms"] for r in on),
            "shadow_rays": on[0]["fog_shadow_rays"], "shadow_rays_per_s": float(np.median([r["shadow_rays_per_s"] for r in on])),
            "fp64_frac": float(np.median([r["fp64_frac"] for r in on])), "objects": kinds, "lights": nlights}
    print(json.dumps(summ), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
            f.write(json.dumps(summ) + "\n")


if __name__ == "__main__":
    main()
