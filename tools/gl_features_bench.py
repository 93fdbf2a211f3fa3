"""What the first-hit features of a GL-shaded frame cost on the MI355X (pt_set_shading_features).

  showcase   gpu_showcase at 1920x1080, 4 passes, depth 8 (gl_trace_kernel + gl_feature_kernel)
  walk       the 1 901-object synthetic scene of tools/glshade_walk_bench.py with 4 lights, the same frame, on the BVH path
             (gl_bvh_kernel + gl_feature_bvh_kernel)

For each scene: frames with moments on and k = 0, 1, 4 feature passes alternated, --reps each after one warm-up of each, as
tools/glshade_bench.py alternates its arrangements.  Per frame the wall time, the GL kernel time (pt_shading_last_stats) and the time
inside the feature kernel (EV_FEATURE: libptcore's PTCORE_VERBOSE note at pt_end); the summary gives the medians and the feature
kernel's share of the GL kernel time.  Every frame must give the same image bytes and the same GL counters: features do not disturb
the radiance.  One JSON line per frame and one summary line per scene.

    python tools/gl_features_bench.py [--scenes showcase,walk] [--out profiles/gl_features_bench.jsonl]
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

NOTE = re.compile(r"gl_feature(?:_bvh)?_kernel ([0-9.]+) ms in (\d+) launches")
GLC = ("paths", "segments", "shadow_rays", "probe_rays", "draws")
KS = (0, 1, 4)


def main() -> None:
    import numpy as np
    import torch  # noqa: F401  (one HIP runtime with torch, see capi.py)

    os.environ["PTCORE_VERBOSE"] = "1"  # read when the frame ends
    from adaptive_bench import Stderr
    from glshade_walk_bench import make_scene
    from path_trace_golang_amd import build, capi, hip, scene

    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="showcase,walk")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--objects", type=int, default=1900)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build.build_core()
    cfg = hip.RenderConfig(a.width, a.height, a.passes, a.depth, 1)
    img = np.zeros((a.height, a.width, 4), np.uint8)
    m2 = np.zeros((a.height, a.width, 3))
    out = []

    def emit(row):
        out.append(row)
        print(json.dumps(row), flush=True)

    for name in [s for s in a.scenes.split(",") if s]:
        walk = name == "walk"
        sc = make_scene(a.objects, 4) if walk else scene.load(os.path.join(ROOT, "scenes", "gpu_showcase.json"))
        rows, first = [], None
        with capi.Context(ndev=1) as ctx:
            for rep in range(a.reps + 1):
                for k in KS:
                    with Stderr() as err:
                        t0 = time.perf_counter()
                        st = hip.render(sc, cfg, img, ctx=ctx, shading="gl", shading_walk=walk, shading_features=True, moments=m2, features=k)
                        ms = (time.perf_counter() - t0) * 1e3
                    gst = hip.shading_last_stats(ctx)
                    row = {"scene": name, "objects": len(sc.objects), "rep": rep, "k": k, "ms": ms, "device_ms": st["device_ms"], "gl_ms": gst["gl_ms"],
                           "gl_launches": gst["gl_launches"], **{c: gst[c] for c in GLC}, "image": int(np.bitwise_xor.reduce(img.view(np.uint32), axis=None))}
                    m = NOTE.search(err.text)
                    row.update(feature_ms=float(m.group(1)) if m else 0.0, feature_launches=int(m.group(2)) if m else 0)
                    first = first or (img.copy(), tuple(gst[c] for c in GLC))
                    row["same_frame"] = bool(np.array_equal(img, first[0])) and tuple(gst[c] for c in GLC) == first[1]
                    if rep > 0:
                        rows.append(row)
                        emit(row)
        med = lambda k, key: float(np.median([r[key] for r in rows if r["k"] == k]))  # noqa: E731
        summ = {"summary": True, "scene": name, "objects": len(sc.objects), "width": a.width, "height": a.height, "passes": a.passes, "depth": a.depth,
                "same_frame": all(r["same_frame"] for r in rows), **{c: rows[0][c] for c in GLC}}
        for k in KS:
            summ["k%d" % k] = {"ms": med(k, "ms"), "gl_ms": med(k, "gl_ms"), "feature_ms": med(k, "feature_ms"),
                               "feature_launches": int(med(k, "feature_launches")), "feature_share_of_gl": med(k, "feature_ms") / med(k, "gl_ms"),
                               "ms_over_k0": med(k, "ms") / med(0, "ms")}
        emit(summ)
    if a.out:
        with open(a.out, "w") as f:
            for r in out:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
