"""Builds and loads tests/device_probe.hip: the routines of csrc/pt_math.h, pt_fog.h and pt_glshade.h one at a time on the
gfx950 device (test_device_probe_cpu.py compiles it anywhere; test_device_math_gpu.py runs it).

The probe is compiled with the library's compiler and exactly its flags (path_trace_golang_amd.build.HIPCC, HIP_FLAGS --
which include -ffp-contract=off), into a temporary directory, never into the tree."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from fog_support import CSRC, ROOT, ptr

SOURCE = os.path.join(ROOT, "tests", "device_probe.hip")
SYMBOLS = ("probe_device_count", "probe_unary", "probe_binary", "probe_sincos", "probe_streams", "probe_hash31",
           "probe_volume_noise", "probe_inscatter_many", "probe_pass_many")
U_SIN, U_TAN, U_EXP, U_POW5, U_SQRT_OUTLINE, U_SQRT_INLINE = range(6)
B_MIN, B_MAX, B_PHASE_HG = range(3)

_dir = None
_lib = None


def compile_probe() -> str:
    """Path of the probe's shared library (built once per process)."""
    global _dir
    from path_trace_golang_amd import build

    if _dir is None:
        _dir = tempfile.mkdtemp(prefix="devprobe_")
    out = os.path.join(_dir, "libdeviceprobe.so")
    if not os.path.exists(out):
        r = subprocess.run([build.HIPCC, *build.HIP_FLAGS, "-shared", "-I", CSRC, SOURCE, "-o", out], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("device probe does not compile:\n%s\n%s" % (r.stdout, r.stderr))
    return out


def load():
    """The probe, loaded after torch so that the process keeps one HIP runtime (as conftest.gpu_ctx does for libptcore.so)."""
    global _lib
    if _lib is None:
        import torch  # noqa: F401

        L = C.CDLL(compile_probe())
        vp = C.c_void_p
        L.probe_device_count.argtypes = [C.POINTER(C.c_int)]
        L.probe_unary.argtypes = [C.c_int, vp, vp, C.c_int64]
        L.probe_binary.argtypes = [C.c_int, vp, vp, vp, C.c_int64]
        L.probe_sincos.argtypes = [vp, vp, vp, C.c_int64]
        L.probe_streams.argtypes = [vp, C.c_int32, vp, vp, C.c_int64]
        L.probe_hash31.argtypes = [vp, vp, C.c_int64]
        L.probe_volume_noise.argtypes = [vp, vp, vp, C.c_int64]
        L.probe_inscatter_many.argtypes = [vp, vp, C.c_int32, C.c_int64, vp, vp, vp, vp]
        L.probe_pass_many.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, vp, C.c_int64, vp, vp, vp]
        for s in SYMBOLS:
            getattr(L, s).restype = C.c_int
        _lib = L
    return _lib


def _ok(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError("%s: HIP status %d" % (what, rc))


def _f64(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float64)


def unary(which: int, x) -> np.ndarray:
    x = _f64(x)
    out = np.empty_like(x)
    _ok(load().probe_unary(which, ptr(x), ptr(out), x.size), "probe_unary(%d)" % which)
    return out


def binary(which: int, a, b) -> np.ndarray:
    a, b = _f64(a), _f64(b)
    assert a.shape == b.shape
    out = np.empty_like(a)
    _ok(load().probe_binary(which, ptr(a), ptr(b), ptr(out), a.size), "probe_binary(%d)" % which)
    return out


def sincos(x):
    x = _f64(x)
    s, c = np.empty_like(x), np.empty_like(x)
    _ok(load().probe_sincos(ptr(x), ptr(s), ptr(c), x.size), "probe_sincos")
    return s, c


def streams(keys: np.ndarray, ndraw: int):
    """(state0 u64 [n], draws f64 [n, ndraw]) for keys u64 [n, 3] = (seed, pixel, sample)."""
    keys = np.ascontiguousarray(keys, np.uint64)
    n = keys.shape[0]
    s0 = np.zeros(n, np.uint64)
    out = np.zeros((n, ndraw), np.float64)
    _ok(load().probe_streams(ptr(keys), ndraw, ptr(s0), ptr(out), n), "probe_streams")
    return s0, out


def hash31(p) -> np.ndarray:
    p = _f64(p)
    out = np.empty(p.shape[0])
    _ok(load().probe_hash31(ptr(p), ptr(out), p.shape[0]), "probe_hash31")
    return out


def volume_noise(fog, p) -> np.ndarray:
    p = _f64(p)
    out = np.empty(p.shape[0])
    _ok(load().probe_volume_noise(C.byref(fog), ptr(p), ptr(out), p.shape[0]), "probe_volume_noise")
    return out


def inscatter(scene_c, fog, depth: int, rays: np.ndarray, keys: np.ndarray):
    """(radiance f64 [n, 3], counters u32 [n, 3]) of fog_inscatter on the device; `scene_c` is a pt_scene (or the oracle's
    scene struct, which has its layout: test_scene_layouts_are_shared)."""
    n = rays.shape[0]
    L = np.zeros((n, 3))
    cnt = np.zeros((n, 3), np.uint32)
    _ok(load().probe_inscatter_many(C.byref(scene_c), C.byref(fog), depth, n, ptr(rays), ptr(keys), ptr(L), ptr(cnt)),
        "probe_inscatter_many")
    return L, cnt


def passes(flat_scene, ex, w, h, depth, seed, jobs: np.ndarray, fog=None):
    """(radiance f64 [n, 3], counters u64 [n, 8]) of gl_pass on the device (the layout of glshade_support.host_passes)."""
    jobs = np.ascontiguousarray(jobs, np.int32)
    n = jobs.shape[0]
    out = np.zeros((n, 3))
    cnt = np.zeros((n, 8), np.uint64)
    _ok(load().probe_pass_many(C.byref(flat_scene.c), C.cast(ex, C.c_void_p), w, h, depth, seed,
                               C.byref(fog) if fog is not None else None, n, ptr(jobs), ptr(out), ptr(cnt)), "probe_pass_many")
    return out, cnt
