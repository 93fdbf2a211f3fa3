"""Helpers of the temporal accumulation tests (test_temporal_cpu.py, test_temporal_gpu.py): builds tests/temporal_reference.c -- the
independent CPU restatement of pt_temporal's model against the oracle -- and a host build of csrc/pt_temporal.h, loads both with
ctypes, and makes the camera sequences (scene documents with the camera moved sideways) and their oracle-side inputs once each."""
from __future__ import annotations

import copy
import ctypes as C
import json
import os
import subprocess

import numpy as np

import atrous_support as at
from conftest import scene_path
from fog_support import CFLAGS, CSRC, CXXFLAGS, ORACLE, ROOT, ptr

T_DEFAULTS = dict(alpha=0.2, tol_z=0.1, n_min=0.9, tol_a=0.05, max_len=32)
OPEN = dict(tol_z=1e9, n_min=-2.0, tol_a=1e9)  # every in-frame tap with history passes

# The host build of pt_temporal.h: the product's per-pixel functions looped over a frame the way pt_temporal launches its kernels
# (temporal_kernel's body, the filter's iterations, the finish), with the two sets of history planes it swaps.
SHIM = r"""
#include <cmath>
#include <cstring>
#include <vector>
#include "pt_temporal.h"
namespace {
struct State {
    std::vector<double> hist[2];
    int cur = 0, W = 0, H = 0;
    bool valid = false;
    ptd::DevCamera cam{};
};
ptd::DevCamera camera(const double *c) {  // ora_camera_setup's 22 doubles
    ptd::DevCamera d{};
    for (int k = 0; k < 3; k++) {
        d.origin[k] = c[k]; d.lower_left[k] = c[3 + k]; d.horizontal[k] = c[6 + k]; d.vertical[k] = c[9 + k];
        d.u[k] = c[12 + k]; d.v[k] = c[15 + k];
    }
    d.lens_radius = c[21];
    return d;
}
}
extern "C" {
void *shim_new() { return new State(); }
void shim_free(void *s) { delete static_cast<State *>(s); }
void shim_reset(void *s) { static_cast<State *>(s)->valid = false; }
int shim_read(void *sp, double *mean, double *var, int32_t *len) {
    State &s = *static_cast<State *>(sp);
    if (!s.valid) return 0;
    const size_t np = (size_t)s.W * s.H;
    const double *h = s.hist[s.cur].data();
    const int32_t *hl = reinterpret_cast<const int32_t *>(h + (size_t)PTT_LH * np);
    for (size_t i = 0; i < np; i++) {
        for (int k = 0; k < 3; k++) mean[3 * i + k] = h[(size_t)k * np + i];
        var[i] = h[(size_t)PTT_VAR * np + i];
        len[i] = hl[2 * i];
    }
    return 1;
}
void shim_frame(void *sp, int32_t W, int32_t H, const double *S, const double *Q, const uint32_t *cnt, uint32_t n, const double *fn,
                const double *fa, const double *fd, const double *cam22, const double *tcfg, int32_t T, const double *sig, double *mean,
                double *var, uint8_t *rgba, double *noise, uint64_t *counts, double *place) {
    State &s = *static_cast<State *>(sp);
    const size_t np = (size_t)W * (size_t)H;
    const bool have = s.valid && s.W == W && s.H == H;
    for (int k = 0; k < 2; k++) s.hist[k].resize((size_t)PTT_PLANES * np);
    ptt::Config Cf;
    Cf.alpha = tcfg[0]; Cf.tol_z = tcfg[1]; Cf.n_min = tcfg[2]; Cf.tol_a = tcfg[3]; Cf.max_len = (int32_t)tcfg[4];
    Cf.have_history = have;
    ptt::View V;
    V.cam = camera(cam22);
    V.inv_width = 1.0 / (double)(W - 1);
    V.inv_height = 1.0 / (double)(H - 1);
    V.W = W; V.H = H;
    const double *hd = s.hist[s.cur].data();
    double *ho = s.hist[s.cur ^ 1].data();
    std::vector<double> col[2] = {std::vector<double>(3 * np), std::vector<double>(3 * np)};
    std::vector<double> v[2] = {std::vector<double>(np), std::vector<double>(np)};
    std::vector<pta::Guide> g(np);
    double before = 0;
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    for (int32_t y = 0; y < H; y++)
        for (int32_t x = 0; x < W; x++) {
            const size_t i = (size_t)y * W + x;
            double c[3], vi;
            pta::prep_pixel(S + 3 * i, Q + 3 * i, cnt ? cnt[i] : n, fn + 3 * i, fa + 3 * i, fd + 3 * i, c, vi, g[i]);
            const bool hit = fd[3 * i + 1] > 0.0;
            int32_t len;
            const ptt::Status st = ptt::blend_pixel(Cf, V, s.cam, hd, reinterpret_cast<const int32_t *>(hd + (size_t)PTT_LH * np), x, y, c, vi,
                                                    g[i], hit, &col[0][3 * i], v[0][i], len);
            ptt::store_history(ho, reinterpret_cast<int32_t *>(ho + (size_t)PTT_LH * np), np, i, &col[0][3 * i], v[0][i], len, g[i], hit);
            before += pta::noise_term(c, vi);
            counts[0] += st == ptt::ST_REPROJECTED;
            counts[1] += st == ptt::ST_DISOCCLUDED;
            counts[2] += st == ptt::ST_BAD;
            counts[3] += (uint64_t)len;
            if (place) {
                double fx, fy, zexp;
                place[2 * i] = place[2 * i + 1] = NAN;
                if (have && st != ptt::ST_BAD && ptt::reproject(V, s.cam, x, y, hit, g[i].z, fx, fy, zexp)) { place[2 * i] = fx; place[2 * i + 1] = fy; }
            }
        }
    s.cur ^= 1; s.valid = true; s.W = W; s.H = H; s.cam = V.cam;
    auto figure = [&](int k) {
        double t = 0;
        for (size_t i = 0; i < np; i++) t += pta::noise_term(&col[k][3 * i], v[k][i]);
        return std::sqrt(t / (double)np);
    };
    noise[0] = std::sqrt(before / (double)np);
    noise[1] = figure(0);
    int cur = 0;
    if (T >= 0) {
        pta::Params P;
        std::memset(&P, 0, sizeof P);
        P.sigma_l = sig[0]; P.sigma_n = sig[1]; P.sigma_z = sig[2]; P.sigma_a = sig[3];
        P.iterations = T;
        P.n_on = sig[1] > 0; P.z_on = sig[2] > 0; P.a_on = sig[3] > 0;
        for (int32_t t = 0; t < T; t++, cur ^= 1)
            for (int32_t y = 0; y < H; y++)
                for (int32_t x = 0; x < W; x++) {
                    const size_t i = (size_t)y * W + x;
                    pta::filter_pixel(P, W, H, x, y, 1 << t, col[cur].data(), v[cur].data(), g.data(), &col[cur ^ 1][3 * i], v[cur ^ 1][i]);
                }
    }
    noise[2] = figure(cur);
    for (size_t i = 0; i < np; i++) {
        for (int k = 0; k < 3; k++) mean[3 * i + k] = col[cur][3 * i + k];
        var[i] = v[cur][i];
        const uint32_t p = pta::finish_pack(&col[cur][3 * i]);
        std::memcpy(rgba + 4 * i, &p, 4);
    }
}
}
"""

_libs = {}
_cache = {}
_vp = C.c_void_p
_FRAME_ARGS = [_vp, C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp, _vp, _vp, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]


def reference():
    """temporal_reference.c linked against oracle/libptoracle.so."""
    if "ref" not in _libs:
        from oracle import ora

        ora.lib()
        out = os.path.join(at._build_dir(), "libtemporalref.so")
        subprocess.run(["gcc", *CFLAGS, "-shared", "-I", ORACLE, os.path.join(ROOT, "tests", "temporal_reference.c"), "-o", out,
                        "-L", ORACLE, "-Wl,-rpath," + ORACLE, "-lptoracle", "-lm"], check=True, capture_output=True)
        L = C.CDLL(out)
        L.tr_new.restype = _vp
        L.tr_free.argtypes = [_vp]
        L.tr_reset.argtypes = [_vp]
        L.tr_read.argtypes = [_vp, _vp, _vp, _vp]
        L.tr_frame.argtypes = _FRAME_ARGS
        L.tr_sums.argtypes = [_vp, _vp, _vp, _vp]
        _libs["ref"] = L
    return _libs["ref"]


def product_host():
    """csrc/pt_temporal.h built for the host with g++."""
    if "shim" not in _libs:
        d = at._build_dir()
        src = os.path.join(d, "temporal_shim.cpp")
        with open(src, "w") as f:
            f.write(SHIM)
        out = os.path.join(d, "libtemporalshim.so")
        subprocess.run(["g++", *CXXFLAGS, "-shared", "-I", CSRC, src, "-o", out], check=True, capture_output=True)
        L = C.CDLL(out)
        L.shim_new.restype = _vp
        L.shim_free.argtypes = [_vp]
        L.shim_reset.argtypes = [_vp]
        L.shim_read.argtypes = [_vp, _vp, _vp, _vp]
        L.shim_frame.argtypes = _FRAME_ARGS
        _libs["shim"] = L
    return _libs["shim"]


class Accumulator:
    """One history, on the restatement (kind "ref") or on the host build of the product's header (kind "host")."""

    def __init__(self, kind: str):
        L = reference() if kind == "ref" else product_host()
        self.kind = kind
        pre = "tr_" if kind == "ref" else "shim_"
        self._new, self._free, self._reset, self._read, self._frame = (getattr(L, pre + n) for n in ("new", "free", "reset", "read", "frame"))
        self.h = self._new()

    def close(self):
        if self.h:
            self._free(self.h)
            self.h = None

    __del__ = close

    def reset(self):
        self._reset(self.h)

    def read(self, w: int, h: int):
        """(mean, var, len) of the stored history, or None when it is empty."""
        mean, var, ln = np.zeros((h, w, 3)), np.zeros((h, w)), np.zeros((h, w), np.int32)
        return (mean, var, ln) if self._read(self.h, ptr(mean), ptr(var), ptr(ln)) else None

    def frame(self, S, Q, n, feats, cam, counts=None, filter=None, **tcfg) -> dict:
        """One frame: S, Q raw sums [H, W, 3], n the count (counts: uint32 [H, W] per pixel), feats the three feature sums, cam =
        camera_of(...); filter = None (no filter) or a dict over atrous_support.DEFAULTS."""
        t = dict(T_DEFAULTS, **tcfg)
        S = np.ascontiguousarray(S, np.float64)
        Q = np.ascontiguousarray(Q, np.float64)
        H, W = S.shape[:2]
        cnt = np.ascontiguousarray(counts, np.uint32) if counts is not None else None
        f = [np.ascontiguousarray(a, np.float64) for a in feats]
        cam = np.ascontiguousarray(cam, np.float64)
        camarg = np.ascontiguousarray(cam[:12]) if self.kind == "ref" else cam
        tc = np.array([t["alpha"], t["tol_z"], t["n_min"], t["tol_a"], float(t["max_len"])], np.float64)
        fc = dict(at.DEFAULTS, **filter) if filter is not None else None
        sig = np.array([fc[k] for k in ("sigma_l", "sigma_n", "sigma_z", "sigma_a")] if fc else [1.0, 0, 0, 0], np.float64)
        mean, var = np.zeros((H, W, 3)), np.zeros((H, W))
        rgba = np.zeros((H, W, 4), np.uint8)
        noise = np.zeros(3)
        cnts = np.zeros(4, np.uint64)
        place = np.zeros((H, W, 2))
        self._frame(self.h, W, H, ptr(S), ptr(Q), ptr(cnt) if cnt is not None else None, int(n), ptr(f[0]), ptr(f[1]), ptr(f[2]),
                    ptr(camarg), ptr(tc), int(fc["iterations"]) if fc else -1, ptr(sig), ptr(mean), ptr(var), ptr(rgba), ptr(noise),
                    ptr(cnts), ptr(place))
        hist = self.read(W, H)
        return dict(mean=mean, var=var, rgba=rgba, noise_before=float(noise[0]), noise_blended=float(noise[1]), noise_after=float(noise[2]),
                    reprojected=int(cnts[0]), disoccluded=int(cnts[1]), bad_pixels=int(cnts[2]), mean_len=float(cnts[3]) / (W * H),
                    place=place, hist_mean=hist[0], hist_var=hist[1], hist_len=hist[2])


def assert_same_frame(a: dict, b: dict, tag="") -> None:
    """Two runs of one frame agree: the output and the stored history bit for bit, the figures to 1e-9, the counts exactly."""
    for k in ("mean", "var", "hist_mean", "hist_var"):
        assert at.same_bits(a[k], b[k]), (tag, k, int(np.count_nonzero(~np.isclose(a[k], b[k], rtol=0, atol=0, equal_nan=True))))
    assert np.array_equal(a["hist_len"], b["hist_len"]), (tag, "len", int(np.count_nonzero(a["hist_len"] != b["hist_len"])))
    assert np.array_equal(a["rgba"], b["rgba"]), (tag, "rgba", int(np.count_nonzero(a["rgba"] != b["rgba"])))
    for k in ("noise_before", "noise_blended", "noise_after", "mean_len"):
        assert abs(a[k] - b[k]) <= 1e-9 * max(1.0, abs(b[k])), (tag, k, a[k], b[k])
    for k in ("reprojected", "disoccluded", "bad_pixels"):
        assert a[k] == b[k], (tag, k, a[k], b[k])


# ---------------------------------------------------------------- camera sequences
def moved_doc(name: str, f: float, step: float = 0.01) -> dict:
    """The shipped scene's document with the camera moved sideways (along forward x up) by f * step * |target - position|."""
    key = ("doc", name)
    if key not in _cache:
        with open(scene_path(name), "r", encoding="utf-8") as fh:
            _cache[key] = json.load(fh)
    doc = copy.deepcopy(_cache[key])
    cam = doc["camera"]
    p, t, u = (np.array([cam[k]["x"], cam[k]["y"], cam[k]["z"]], np.float64) for k in ("position", "target", "up"))
    fwd = t - p
    dist = float(np.linalg.norm(fwd))
    right = np.cross(fwd, u)
    right = right / np.linalg.norm(right)
    p = p + right * (f * step * dist)
    cam["position"] = {"x": float(p[0]), "y": float(p[1]), "z": float(p[2])}
    return doc


def ora_scene(name: str, f: float, step: float = 0.01):
    """The oracle scene of moved_doc, kept alive for the session (atrous_support.ref_features caches by id(scene))."""
    from oracle import ora

    key = ("ora", name, float(f), step)
    if key not in _cache:
        _cache[key] = ora.Scene(moved_doc(name, f, step))
    return _cache[key]


def product_scene(name: str, f: float, step: float = 0.01):
    from path_trace_golang_amd import scene

    return scene.Scene.decode(moved_doc(name, f, step))


def camera_of(sc, w: int, h: int) -> np.ndarray:
    """ora_camera_setup: origin, lower_left, horizontal, vertical, u, v, w, lens radius (22 doubles)."""
    from oracle import ora

    out = np.zeros(22)
    ora.lib().ora_camera_setup(C.byref(sc.c.camera), w, h, out.ctypes.data_as(C.POINTER(C.c_double)))
    return out


def oracle_frame(name: str, f: float, w: int, h: int, spp: int, depth: int, seed: int, k: int = 4, step: float = 0.01) -> dict:
    """A frame's inputs from oracle samples only: dict(S, Q, feats, cam), computed once."""
    from oracle import ora

    key = ("frame", name, float(f), w, h, spp, depth, seed, k, step)
    if key not in _cache:
        sc = ora_scene(name, f, step)
        cfg = ora.OraConfig(w, h, spp, depth, seed, 1, 0)
        S, Q = np.zeros((h, w, 3)), np.zeros((h, w, 3))
        reference().tr_sums(C.byref(sc.c), C.byref(cfg), ptr(S), ptr(Q))
        S.setflags(write=False)
        Q.setflags(write=False)
        _cache[key] = dict(S=S, Q=Q, feats=at.ref_features(sc, w, h, spp, depth, seed, k), cam=camera_of(sc, w, h), n=spp)
    return _cache[key]


def run_sequence(kind: str, frames, filter=None, **tcfg):
    """Every frame of `frames` (dicts of oracle_frame) through one Accumulator: the list of its results."""
    acc = Accumulator(kind)
    try:
        return [acc.frame(f["S"], f["Q"], f["n"], f["feats"], f["cam"], f.get("counts"), filter, **tcfg) for f in frames]
    finally:
        acc.close()


def temporal_config(**kw):
    from path_trace_golang_amd import hip

    return hip.TemporalConfig(**dict(T_DEFAULTS, **kw))


def gpu_frame(ctx, tcfg, filter, w: int, h: int) -> dict:
    """pt_temporal on ctx's frame and pt_temporal_read after it: the dict of Accumulator.frame (without `place`) plus the stats."""
    from path_trace_golang_amd import hip

    img, mean, var = np.zeros((h, w, 4), np.uint8), np.zeros((h, w, 3)), np.zeros((h, w))
    st = hip.temporal(ctx, tcfg, filter, img, mean, var)
    hm, hv, hl = np.zeros((h, w, 3)), np.zeros((h, w)), np.zeros((h, w), np.int32)
    hip.temporal_read(ctx, hm, hv, hl)
    return dict(st, mean=mean, var=var, rgba=img, hist_mean=hm, hist_var=hv, hist_len=hl)
