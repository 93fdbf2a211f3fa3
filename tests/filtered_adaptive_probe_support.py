"""Builds and loads tests/filtered_adaptive_probe.hip: block_err_kernel, block_pool_kernel and keep_from_map_kernel (with
compact_kernel behind it) of csrc/pt_kernels.h, through the product's own launch sequences of csrc/pt_filter_launch.h
(test_filtered_adaptive_probe_cpu.py compiles it anywhere; test_filtered_adaptive_probe_gpu.py runs it).

The probe is compiled with the library's compiler and exactly its flags (path_trace_golang_amd.build.HIPCC, HIP_FLAGS), into a
temporary directory, never into the tree."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import adaptive_support as ad
import filtered_adaptive_support as fa
from adaptive_probe_support import RES, SENTINEL
from fog_support import CSRC, ROOT, ptr

SOURCE = os.path.join(ROOT, "tests", "filtered_adaptive_probe.hip")
SYMBOLS = ("probe_block_map", "probe_keep_from_map")

_dir = None
_lib = None


def compile_probe() -> str:
    """Path of the probe's shared library (built once per process)."""
    global _dir
    from path_trace_golang_amd import build

    if _dir is None:
        _dir = tempfile.mkdtemp(prefix="faprobe_")
    out = os.path.join(_dir, "libfilteredadaptiveprobe.so")
    if not os.path.exists(out):
        r = subprocess.run([build.HIPCC, *build.HIP_FLAGS, "-shared", "-I", CSRC, "-I", os.path.join(ROOT, "include"), SOURCE, "-o", out],
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("filtered adaptive probe does not compile:\n%s\n%s" % (r.stdout, r.stderr))
    return out


def load():
    """The probe, loaded after torch so that the process keeps one HIP runtime (as conftest.gpu_ctx does for libptcore.so)."""
    global _lib
    if _lib is None:
        import torch  # noqa: F401

        L = C.CDLL(compile_probe())
        vp = C.c_void_p
        L.probe_block_map.argtypes = [vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_double, vp, vp, vp, vp, vp]
        L.probe_keep_from_map.argtypes = [vp, C.c_int64, C.c_int64, vp, vp, C.c_int32, vp, vp, vp, vp, vp, vp]
        for s in SYMBOLS:
            getattr(L, s).restype = C.c_int
        _lib = L
    return _lib


def block_map(mean, err, bad, pool: int, target: float) -> dict:
    """block_err_kernel and block_pool_kernel on the device: the dict of filtered_adaptive_support.host_blocks."""
    mean, err, bad = (np.ascontiguousarray(a, np.float64) for a in (mean, err, bad))
    h, w = err.shape
    g = fa.grid(w, h)
    r = dict(s=np.zeros(g), k=np.zeros(g, np.uint32), pooled=np.zeros(g), own=np.zeros(g), stop=np.zeros(g, np.uint8))
    rc = load().probe_block_map(ptr(mean), ptr(err), ptr(bad), w, h, int(pool), float(target), *(ptr(r[n]) for n in ("s", "k", "pooled", "own", "stop")))
    if rc != 0:
        raise RuntimeError("probe_block_map: status %d" % rc)
    return r


def geom5(w: int, h: int, shard_index: int, shard_count: int) -> np.ndarray:
    return np.array([w, h, (w + 31) // 32, shard_index, shard_count], np.int32)


def shard_slots(w: int, h: int, shard_index: int, shard_count: int) -> int:
    return len(range(shard_index, ((w + 31) // 32) * ((h + 31) // 32), shard_count)) * 1024


def keep_from_map(active, w, h, shard_index, shard_count, n, pooled=None, stop=None) -> dict:
    """keep_from_map_kernel and compact_kernel on the device: dict(blk_spp, keep, noise, next, res)."""
    active = np.ascontiguousarray(active, np.uint32)
    ns = shard_slots(w, h, shard_index, shard_count)
    r = dict(blk_spp=np.zeros(ns // 64, np.uint32), keep=np.zeros(active.size, np.uint32), noise=np.zeros(active.size),
             next=np.zeros(active.size, np.uint32), res=np.zeros(1, RES))
    p = np.ascontiguousarray(pooled, np.float64) if pooled is not None else None
    s = np.ascontiguousarray(stop, np.uint8) if stop is not None else None
    g = geom5(w, h, shard_index, shard_count)
    rc = load().probe_keep_from_map(ptr(active), active.size, ns, ptr(p) if p is not None else None, ptr(s) if s is not None else None, int(n),
                                    ptr(g), *(ptr(r[k]) for k in ("blk_spp", "keep", "noise", "next", "res")))
    if rc != 0:
        raise RuntimeError("probe_keep_from_map: status %d" % rc)
    r["res"] = r["res"][0]
    return r


def keep_reference(order, ns: int, n: int, pooled=None, stop=None) -> dict:
    """What the two kernels leave for the list `order` (rows of adaptive_support.block_order): blk_spp = n in the listed blocks and
    the sentinel elsewhere; keep and noise from the map at the block's place in the frame's grid (all kept and +inf without a map);
    the next list = the kept entries in order, then the sentinel; nact and the largest noise among the kept (0 with none)."""
    blk, by, bx = order[:, 0], order[:, 1], order[:, 2]
    spp = np.full(ns // 64, SENTINEL, np.uint32)
    spp[blk] = n
    if pooled is None:
        keep, noise = np.ones(len(blk), np.uint32), np.full(len(blk), np.inf)
    else:
        keep, noise = (1 - np.asarray(stop)[by, bx]).astype(np.uint32), np.asarray(pooled)[by, bx].astype(np.float64)
    kept = keep != 0
    nxt = np.full(len(blk), SENTINEL, np.uint32)
    nxt[:int(kept.sum())] = blk[kept]
    return dict(blk_spp=spp, keep=keep, noise=noise, next=nxt, nact=int(kept.sum()), worst=float(noise[kept].max()) if kept.any() else 0.0)


# (width, height, shard index, shard count): one device and shard 1 of 3 at 70 x 45; 293 x 253 on one device: 1 184 blocks, so
# compact_kernel behind the new keep[] walks more than one strip of 1 024 entries
LISTS = ((70, 45, 0, 1), (70, 45, 1, 3), (293, 253, 0, 1), (293, 253, 2, 3))
