"""Cost of the second moments on the MI355X: gpu_showcase at 1920x1080, depth 8, moments off and on alternated in one
process, three frames each (after one warm-up of each).  Prints one JSON line per frame and a summary line:
  ms per frame (off / on), resolve_kernel's time (pt_stats.resolve_ms, the yardstick: it streams the same radiance
  records), moments_kernel's time and launches (libptcore's PTCORE_VERBOSE note at pt_end, read back from stderr), and
  the time of one pt_noise_estimate call on the finished frame.

    python tools/moments_bench.py [--spp 1024] [--out profiles/moments_bench.jsonl]
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

NOTE = re.compile(r"moments_kernel ([0-9.]+) ms in (\d+) launches \(resolve_kernel ([0-9.]+) ms in (\d+)\)")


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
    ap.add_argument("--spp", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build.build_core()
    sc = hip.FlatScene(scene.load(os.path.join(ROOT, "scenes", "gpu_showcase.json")))
    img = np.zeros((a.height, a.width, 4), np.uint8)
    m2 = np.zeros((a.height, a.width, 3))
    cfg = hip.RenderConfig(a.width, a.height, a.spp, a.depth, 1)
    rows = []
    with capi.Context(ndev=1) as ctx:
        for rep in range(a.reps + 1):
            for on in (False, True):
                with Stderr() as err:
                    t0 = time.perf_counter()
                    # the frame alone: the moments are read and the noise is estimated outside the timed part
                    hip.set_moments(ctx, on)
                    st = capi.PtStats()
                    pc = hip.pt_config(cfg)
                    capi.check(capi.load().pt_render(ctx.handle, C.byref(sc.c), C.byref(pc), img.ctypes.data_as(C.c_void_p),
                                                     int(img.strides[0]), None, None, None, C.byref(st)))
                    ms = (time.perf_counter() - t0) * 1e3
                row = {"rep": rep, "moments": on, "ms": ms, "device_ms": st.device_ms, "trace_ms": st.trace_ms,
                       "resolve_ms": st.resolve_ms, "resolve_launches": st.resolve_launches, "spp_chunk": st.spp_chunk,
                       "segments": st.segments}
                if on:
                    m = NOTE.search(err.text)
                    if not m:
                        raise RuntimeError("no moments_kernel note on stderr: %r" % err.text[-400:])
                    row.update(moments_ms=float(m.group(1)), moments_launches=int(m.group(2)))
                    row["moments_over_resolve"] = row["moments_ms"] / row["resolve_ms"]
                    t0 = time.perf_counter()
                    nz = hip.noise_estimate(ctx)
                    row["noise_estimate_ms"] = (time.perf_counter() - t0) * 1e3
                    t0 = time.perf_counter()
                    hip.read_moments(ctx, m2)
                    row["read_moments_ms"] = (time.perf_counter() - t0) * 1e3
                    row.update(noise=nz["noise"], bad_pixels=nz["bad_pixels"])
                if rep > 0:
                    rows.append(row)
                print(json.dumps(row), flush=True)
    off = [r for r in rows if not r["moments"]]
    on = [r for r in rows if r["moments"]]
    summ = {"summary": True, "scene": "gpu_showcase", "width": a.width, "height": a.height, "spp": a.spp, "depth": a.depth,
            "ms_off": sorted(r["ms"] for r in off), "ms_on": sorted(r["ms"] for r in on),
            "resolve_ms_off": sorted(r["resolve_ms"] for r in off), "resolve_ms_on": sorted(r["resolve_ms"] for r in on),
            "moments_ms": sorted(r["moments_ms"] for r in on),
            "moments_over_resolve": float(np.median([r["moments_over_resolve"] for r in on])),
            "noise_estimate_ms": sorted(r["noise_estimate_ms"] for r in on),
            "read_moments_ms": sorted(r["read_moments_ms"] for r in on), "noise": on[0]["noise"]}
    print(json.dumps(summ), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
            f.write(json.dumps(summ) + "\n")


if __name__ == "__main__":
    main()
