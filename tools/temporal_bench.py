"""Cost of the temporal accumulation on the MI355X: gpu_showcase at 1920x1080, depth 8, one process, buffers warm.

  atrous     the yardstick: a frame of --spp samples with k = --k, then pt_atrous at the defaults, --reps calls after one warm-up
             (pt_atrous_stats.atrous_ms and the call's wall time).  Runs with any libptcore.so that has pt_atrous (PTCORE_LIB), so
             the parent commit's library measures it on the same box.
  temporal   two frames of a sideways camera move (1 % of the distance to the target), seeds 1 and 2; after each pt_temporal with
             the default filter.  The pair is repeated --reps times after one warm-up pair, the history reset before each pair, so every
             timed call of the second frame reprojects the first: pt_temporal_stats.temporal_ms (all launches), the time inside
             temporal_kernel (libptcore's PTCORE_VERBOSE note), the call's wall time, and the kernel's achieved bytes per second
             on the bytes each pixel has to move once (--bytes-per-pixel) against --hbm-peak.
             --clip GAMMA runs it with the history clip (pt_temporal_set_clip; 0 = off, the default) and adds
             clipped and clipped / reprojected to every row; a library without the entry point runs with 0 only.
             --motion runs it with displaced reprojection (pt_temporal_set_motion): in the second frame one sphere
             and one box of the scene stand 0.08 further along x, the frames record object ids, the table of all 27 objects goes in
             front of the second pt_temporal, and every row gains moved and moved_reprojected.  Without the flag nothing of it is
             touched, so the parent commit's library measures the same calls.

    python tools/temporal_bench.py --part atrous|temporal [--clip GAMMA] [--motion] [--out FILE]
"""
from __future__ import annotations

import argparse
import copy
import ctypes as C
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

NOTE = re.compile(r"temporal_kernel ([0-9.]+) ms")
# per pixel, each once: S 24 + Q 24 + three feature sums 72 read; the previous history 96 read (the four taps of neighbouring lanes
# are the same words); the new history 96 + colour 24 + variance 8 + guide 64 written
BYTES_PER_PIXEL = 24 + 24 + 72 + 96 + 96 + 24 + 8 + 64


def main() -> None:
    import numpy as np
    import torch  # noqa: F401  (one HIP runtime with torch, see capi.py)

    os.environ["PTCORE_VERBOSE"] = "1"
    from adaptive_bench import Stderr
    from path_trace_golang_amd import capi, hip, scene

    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("atrous", "temporal"), required=True)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--clip", type=float, default=0.0, help="gamma of the history clip; 0 = off")
    ap.add_argument("--motion", action="store_true", help="displaced reprojection: two objects moved, the table of 27 passed")
    ap.add_argument("--bytes-per-pixel", type=int, default=BYTES_PER_PIXEL)
    ap.add_argument("--hbm-peak", type=float, default=8.0e12, help="bytes per second")
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = capi.load()
    W, H = a.width, a.height
    base = scene.load(os.path.join(ROOT, "scenes", "gpu_showcase.json"))
    moved = copy.deepcopy(base)
    p, t, u = (np.array(v.as_list()) for v in (base.camera.position, base.camera.target, base.camera.up))
    right = np.cross(t - p, u)
    q = p + right / np.linalg.norm(right) * (0.01 * np.linalg.norm(t - p))
    moved.camera.position = scene.Vec3(float(q[0]), float(q[1]), float(q[2]))
    delta = None
    if a.motion:
        for i in (8, 15):  # the rough copper sphere and the white box
            moved.objects[i].position.x += 0.08
        delta = hip.scene_motion(base, moved)
        assert delta is not None and delta.shape == (27, 3)
    flats = [hip.FlatScene(base), hip.FlatScene(moved)]
    img = np.zeros((H, W, 4), np.uint8)
    rows = []

    def emit(row):
        row.update(lib=os.environ.get("PTCORE_LIB", "in-tree"), tag=a.tag, width=W, height=H, spp=a.spp)
        rows.append(row)
        print(json.dumps(row), flush=True)

    def frame(ctx, i):
        hip.set_moments(ctx, True)
        hip.set_features(ctx, a.k)
        if a.motion:
            hip.set_object_ids(ctx, True)
        pc = hip.pt_config(hip.RenderConfig(W, H, a.spp, a.depth, 1 + i))
        capi.check(L.pt_render(ctx.handle, C.byref(flats[i].c), C.byref(pc), img.ctypes.data_as(C.c_void_p), int(img.strides[0]), None, None, None, None))

    with capi.Context(ndev=1) as ctx:
        if a.part == "atrous":
            frame(ctx, 0)
            for rep in range(a.reps + 1):
                t0 = time.perf_counter()
                st = hip.atrous(ctx, hip.AtrousConfig(), img)
                st.update(part="atrous", rep=rep, wall_ms=(time.perf_counter() - t0) * 1e3)
                if rep > 0:
                    emit(st)
        else:
            if a.clip != 0.0 or capi.has("pt_temporal_set_clip"):
                hip.temporal_set_clip(ctx, a.clip)
            for rep in range(a.reps + 1):
                hip.temporal_reset(ctx)
                for i in (0, 1):
                    frame(ctx, i)
                    if a.motion and i == 1:
                        hip.temporal_set_motion(ctx, delta)
                    with Stderr() as err:
                        t0 = time.perf_counter()
                        st = hip.temporal(ctx, hip.TemporalConfig(), hip.AtrousConfig(), img)
                        wall = (time.perf_counter() - t0) * 1e3
                    m = NOTE.search(err.text)
                    st.update(part="temporal", rep=rep, frame=i, wall_ms=wall, kernel_ms=float(m.group(1)) if m else -1.0, clip=a.clip)
                    if capi.has("pt_temporal_clip_stats"):
                        st["clipped"] = hip.temporal_clip_stats(ctx)["clipped"]
                        st["clipped_fraction"] = st["clipped"] / max(st["reprojected"], 1)
                    if a.motion:
                        st.update(hip.temporal_motion_stats(ctx))
                    if m:
                        st["kernel_bytes_per_s"] = a.bytes_per_pixel * W * H / (st["kernel_ms"] * 1e-3)
                        st["kernel_fraction_of_hbm_peak"] = st["kernel_bytes_per_s"] / a.hbm_peak
                    if rep > 0:
                        emit(st)
    if a.out:
        with open(a.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
