"""GL shading on the BVH path on the MI355X (pt_set_shading_walk): what the per-lane walk costs.

  compare   the largest synthetic scene the PTCORE_SCAN=uniform plan accepts, 4 lights, 1920x1080, 1 pass, depth 8:
            A = the linear gl_trace_kernel on a uniform context, B = gl_bvh_kernel on a default context with the walk, alternated,
            three frames each after one warm-up of each; the GL kernel milliseconds of pt_shading_last_stats and their ratio.
  walk      gl_bvh_kernel alone on a scene of --objects objects with 8 lights: GL ms per frame, paths, segments and shadow rays per
            second, node visits per query of each kind, the share of queries sent to the plain loop, the deepest stack.

Prints one JSON line per frame and a summary line; every frame of a mode must give the same GL counters, and in `compare` A and B
must give the same image bytes.  One mode per process: run each under its own time limit.

    python tools/glshade_walk_bench.py compare [--out profiles/gl_walk_compare.json]
    python tools/glshade_walk_bench.py walk --objects 10000
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GLC = ("paths", "segments", "shadow_rays", "probe_rays", "draws")


def make_scene(n: int, lights: int, room: float = 40.0):
    """synth.make_scene(n) with light_every chosen for `lights` lights."""
    from path_trace_golang_amd import synth

    n_free = max(1, n - 4)
    sc = synth.make_scene(n, seed=1, room=room, light_every=max(1, -(-n_free // lights)))
    have = sum(1 for o in sc.objects if o.type == "sphere_light")
    assert have == lights, (have, lights)
    return sc


def context(env):
    from path_trace_golang_amd import capi

    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)  # read at pt_create
    try:
        return capi.Context(ndev=1)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def frame(ctx, sc, cfg, img, walk):
    from path_trace_golang_amd import hip

    t0 = time.perf_counter()
    st = hip.render(sc, cfg, img, ctx=ctx, shading="gl", shading_walk=walk)
    ms = (time.perf_counter() - t0) * 1e3
    gst = hip.shading_last_stats(ctx)
    row = {"ms": ms, "device_ms": st["device_ms"], "gl_ms": gst["gl_ms"], "gl_launches": gst["gl_launches"], **{k: gst[k] for k in GLC}}
    if gst["gl_ms"] > 0:
        for k in ("paths", "segments", "shadow_rays"):
            row[k + "_per_s"] = gst[k] / (gst["gl_ms"] * 1e-3)
    if walk:
        try:
            ws = hip.shading_walk_stats(ctx)
        except Exception:  # the scene was not on the BVH path: gl_trace_kernel ran
            ws = None
        if ws:
            nq = ws["closest_walked"] + ws["closest_plain"] + ws["shadow_walked"] + ws["shadow_plain"]
            row.update(ws, visits_per_closest=ws["closest_visits"] / max(1, ws["closest_walked"]),
                       visits_per_shadow=ws["shadow_visits"] / max(1, ws["shadow_walked"]),
                       plain_share=(ws["closest_plain"] + ws["shadow_plain"]) / max(1, nq))
    return row


def main() -> None:
    import numpy as np
    import torch  # noqa: F401  (one HIP runtime with torch, see capi.py)

    from path_trace_golang_amd import build, capi, hip

    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["compare", "walk"])
    ap.add_argument("--objects", type=int, default=10000)
    ap.add_argument("--lights", type=int, default=None)
    ap.add_argument("--passes", type=int, default=1)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build.build_core()
    cfg = hip.RenderConfig(a.width, a.height, a.passes, a.depth, 1)
    img = {k: np.zeros((a.height, a.width, 4), np.uint8) for k in "AB"}
    rows = []
    keys = ("visits_per_closest", "visits_per_shadow", "plain_share", "deepest_stack")
    if a.mode == "compare":
        lights = a.lights or 4
        A = context({"PTCORE_SCAN": "uniform"})
        sc = None
        for n in range(2000, 100, -100):  # the uniform plan stages the world in LDS: the largest count of this ladder it accepts
            sc = make_scene(n, lights)
            try:
                hip.render(sc, hip.RenderConfig(16, 16, 1, 1, 1), np.zeros((16, 16, 4), np.uint8), ctx=A, shading="gl")
                break
            except capi.PtError as e:
                print(json.dumps({"objects": n, "refused": str(e)}), flush=True)
        B = context({})
        for rep in range(a.reps + 1):
            for name, ctx, walk in (("A", A, False), ("B", B, True)):
                row = dict(rep=rep, arrangement=name, objects=len(sc.objects), lights=lights, **frame(ctx, sc, cfg, img[name], walk))
                print(json.dumps(row), flush=True)
                if rep > 0:
                    rows.append(row)
        A.close()
        B.close()
        same = bool(np.array_equal(img["A"], img["B"]))
        fa = sorted(r["gl_ms"] for r in rows if r["arrangement"] == "A")
        fb = sorted(r["gl_ms"] for r in rows if r["arrangement"] == "B")
        cnt = {tuple(r[k] for k in GLC) for r in rows}
        last = [r for r in rows if r["arrangement"] == "B"][-1]
        summ = {"summary": True, "mode": "compare", "objects": len(sc.objects), "lights": lights, "width": a.width, "height": a.height,
                "passes": a.passes, "depth": a.depth, "gl_ms_linear": fa, "gl_ms_walk": fb, "walk_over_linear": float(np.median(fb) / np.median(fa)),
                "images_equal": same, "counters_equal": len(cnt) == 1, **{k: rows[0][k] for k in GLC}, **{k: last.get(k) for k in keys}}
    else:
        lights = a.lights or 8
        sc = make_scene(a.objects, lights)
        with context({}) as ctx:
            for rep in range(a.reps + 1):
                row = dict(rep=rep, objects=len(sc.objects), lights=lights, **frame(ctx, sc, cfg, img["B"], True))
                print(json.dumps(row), flush=True)
                if rep > 0:
                    rows.append(row)
        cnt = {tuple(r[k] for k in GLC) for r in rows}
        summ = {"summary": True, "mode": "walk", "objects": len(sc.objects), "lights": lights, "width": a.width, "height": a.height,
                "passes": a.passes, "depth": a.depth, "gl_ms": sorted(r["gl_ms"] for r in rows), "ms": sorted(r["ms"] for r in rows),
                **{k: rows[0][k] for k in GLC}, **{k + "_per_s": float(np.median([r[k + "_per_s"] for r in rows])) for k in ("paths", "segments", "shadow_rays")},
                **{k: rows[0].get(k) for k in keys}, "counters_equal": len(cnt) == 1}
    print(json.dumps(summ), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
            f.write(json.dumps(summ) + "\n")


if __name__ == "__main__":
    main()
