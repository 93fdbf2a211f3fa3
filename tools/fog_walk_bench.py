"""Volumetric fog on the BVH path on the MI355X (pt_set_fog_walk): what the wave-shared walks cost.

  compare   the largest synthetic scene the PTCORE_SCAN=uniform plan accepts, 4 lights, 1920x1080, 4 spp, depth 8:
            A = the linear fog_kernel on a uniform context, B = fog_bvh_kernel on a default context with the walk, alternated,
            three frames each after one warm-up of each; the fog kernel milliseconds of pt_fog_last_stats and their ratio.
  walk      fog_bvh_kernel alone on a scene of --objects objects with 8 lights: fog ms per frame, shadow rays per second, node visits
            per shadow turn, the share of turns sent to the plain loop.

Prints one JSON line per frame and a summary line; every frame of a mode must give the same fog counters, and in `compare` A and B
must give the same image bytes.  One mode per process: run each under its own time limit.

    python tools/fog_walk_bench.py compare [--out profiles/fog_walk_compare.json]
    python tools/fog_walk_bench.py walk --objects 10000
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FOG = dict(density=0.05, scatter=0.8, g=0.3, hetero_strength=0.4, noise_scale=2.0, noise_octaves=2, affect_sky=True, gpu_volumetric=True)


def make_scene(n: int, lights: int, room: float = 40.0):
    """synth.make_scene(n) with light_every chosen for `lights` lights and a fog block."""
    from path_trace_golang_amd import scene, synth

    n_free = max(1, n - 4)
    sc = synth.make_scene(n, seed=1, room=room, light_every=max(1, -(-n_free // lights)))
    sc.fog = scene.Fog(color=scene.Color(0.85, 0.88, 0.95), **FOG)
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
    st = hip.render(sc, cfg, img, ctx=ctx, fog=True, fog_walk=walk)
    ms = (time.perf_counter() - t0) * 1e3
    fst = hip.fog_last_stats(ctx)
    row = {"ms": ms, "device_ms": st["device_ms"], "trace_ms": st["trace_ms"], "fog_ms": fst["fog_ms"], "fog_launches": fst["fog_launches"],
           "shadow_rays": fst["shadow_rays"], "fog_draws": fst["draws"], "steps": fst["steps"]}
    if fst["fog_ms"] > 0:
        row["shadow_rays_per_s"] = fst["shadow_rays"] / (fst["fog_ms"] * 1e-3)
    if walk:
        try:
            ws = hip.fog_walk_stats(ctx)
        except Exception:  # the scene was not on the BVH path: fog_kernel ran
            ws = None
        if ws:
            turns = ws["shadow_walked"] + ws["shadow_plain"]
            row.update(ws, visits_per_turn=ws["node_visits"] / max(1, ws["shadow_walked"]), plain_share=ws["shadow_plain"] / max(1, turns))
    return row


def main() -> None:
    import numpy as np
    import torch  # noqa: F401  (one HIP runtime with torch, see capi.py)

    from path_trace_golang_amd import build, capi, hip

    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["compare", "walk"])
    ap.add_argument("--objects", type=int, default=10000)
    ap.add_argument("--lights", type=int, default=None)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build.build_core()
    cfg = hip.RenderConfig(a.width, a.height, a.spp, a.depth, 1)
    img = {k: np.zeros((a.height, a.width, 4), np.uint8) for k in "AB"}
    rows = []
    if a.mode == "compare":
        lights = a.lights or 4
        A = context({"PTCORE_SCAN": "uniform"})
        sc = None
        for n in range(2000, 100, -100):  # the uniform plan stages the world in LDS: the largest count of this ladder it accepts
            sc = make_scene(n, lights)
            try:
                hip.render(sc, hip.RenderConfig(16, 16, 1, 1, 1), np.zeros((16, 16, 4), np.uint8), ctx=A, fog=True)
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
        fa = sorted(r["fog_ms"] for r in rows if r["arrangement"] == "A")
        fb = sorted(r["fog_ms"] for r in rows if r["arrangement"] == "B")
        cnt = {(r["shadow_rays"], r["fog_draws"], r["steps"]) for r in rows}
        summ = {"summary": True, "mode": "compare", "objects": len(sc.objects), "lights": lights, "width": a.width, "height": a.height, "spp": a.spp,
                "depth": a.depth, "fog_ms_linear": fa, "fog_ms_walk": fb, "walk_over_linear": float(np.median(fb) / np.median(fa)),
                "images_equal": same, "counters_equal": len(cnt) == 1, "shadow_rays": rows[0]["shadow_rays"],
                "visits_per_turn": rows[-1].get("visits_per_turn"), "plain_share": rows[-1].get("plain_share")}
    else:
        lights = a.lights or 8
        sc = make_scene(a.objects, lights)
        with context({}) as ctx:
            for rep in range(a.reps + 1):
                row = dict(rep=rep, objects=len(sc.objects), lights=lights, **frame(ctx, sc, cfg, img["B"], True))
                print(json.dumps(row), flush=True)
                if rep > 0:
                    rows.append(row)
        cnt = {(r["shadow_rays"], r["fog_draws"], r["steps"]) for r in rows}
        summ = {"summary": True, "mode": "walk", "objects": len(sc.objects), "lights": lights, "width": a.width, "height": a.height, "spp": a.spp,
                "depth": a.depth, "fog_ms": sorted(r["fog_ms"] for r in rows), "ms": sorted(r["ms"] for r in rows),
                "shadow_rays": rows[0]["shadow_rays"], "shadow_rays_per_s": float(np.median([r["shadow_rays_per_s"] for r in rows])),
                "visits_per_turn": rows[0]["visits_per_turn"], "plain_share": rows[0]["plain_share"], "deepest_stack": rows[0]["deepest_stack"],
                "counters_equal": len(cnt) == 1}
    print(json.dumps(summ), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
            f.write(json.dumps(summ) + "\n")


if __name__ == "__main__":
    main()
