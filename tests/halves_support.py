"""Helpers of the half-buffer tests (test_halves_cpu.py, test_halves_gpu.py): a host build of the pair functions of
csrc/pt_atrous.h, looped the way pt_atrous_halves launches its kernels (pair prep, T ping-pong pair iterations over the plane
layout, combine); the reference -- atrous_support.ref_filter, the independent restatement of the filter, on each half as a frame
of its own, and the combine restated here in plain floats; and the half sums of the oracle's samples."""
from __future__ import annotations

import ctypes as C
import math
import os
import subprocess

import numpy as np

import atrous_support as at
from fog_support import CSRC, CXXFLAGS, ptr

SHIM = r"""
#include <cmath>
#include <cstring>
#include <vector>
#include "pt_atrous.h"
extern "C" void shim_pair(int32_t W, int32_t H, const double *SA, const double *QA, const double *SB, const double *QB, const uint32_t *cnt,
                          uint32_t n, const double *fn, const double *fa, const double *fd, int32_t T, const double *sig, double *mean,
                          double *err, double *half_means, double *noise, uint64_t *bad) {
    const size_t np = (size_t)W * (size_t)H;
    const bool feat = fn && fa && fd;
    std::vector<double> guide(PTA_GUIDE_PLANES * np), col[2] = {std::vector<double>(6 * np), std::vector<double>(6 * np)};
    std::vector<double> var[2] = {std::vector<double>(2 * np), std::vector<double>(2 * np)};
    for (size_t i = 0; i < np; i++)
        pta::prep_pair_pixel(SA + 3 * i, QA + 3 * i, SB + 3 * i, QB + 3 * i, cnt ? cnt[i] : n, feat ? fn + 3 * i : nullptr,
                             feat ? fa + 3 * i : nullptr, feat ? fd + 3 * i : nullptr, np, i, guide.data(), col[0].data(), var[0].data());
    pta::Params P;
    std::memset(&P, 0, sizeof P);
    P.sigma_l = sig[0]; P.sigma_n = sig[1]; P.sigma_z = sig[2]; P.sigma_a = sig[3];
    P.iterations = T;
    P.n_on = feat && sig[1] > 0; P.z_on = feat && sig[2] > 0; P.a_on = feat && sig[3] > 0;
    int cur = 0;
    for (int32_t t = 0; t < T; t++, cur ^= 1)
        for (int32_t y = 0; y < H; y++)
            for (int32_t x = 0; x < W; x++) {
                const size_t i = (size_t)y * W + x;
                double c[6], v[2];
                pta::filter_pair_pixel(P, W, H, x, y, 1 << t, col[cur].data(), var[cur].data(), guide.data(), c, v);
                for (int k = 0; k < 6; k++) col[cur ^ 1][(size_t)k * np + i] = c[k];
                var[cur ^ 1][i] = v[0];
                var[cur ^ 1][np + i] = v[1];
            }
    double sum = 0, model = 0;
    *bad = 0;
    for (size_t i = 0; i < np; i++) {
        const double *c = col[cur].data();
        const double fA[3] = {c[i], c[np + i], c[2 * np + i]}, fB[3] = {c[3 * np + i], c[4 * np + i], c[5 * np + i]};
        double e2, em;
        *bad += pta::combine_pixel(fA, fB, var[cur][i], var[cur][np + i], (int)guide[(size_t)PTA_GUIDE_BAD * np + i], mean + 3 * i, err[i], e2, em);
        sum += e2;
        model += em;
        for (int k = 0; k < 3; k++) { half_means[3 * i + k] = fA[k]; half_means[3 * (np + i) + k] = fB[k]; }
    }
    noise[0] = std::sqrt(sum / (double)np);
    noise[1] = std::sqrt(model / (double)np);
}
"""

_lib = None
_vp = C.c_void_p


def product_host():
    """The pair functions of csrc/pt_atrous.h built for the host with g++."""
    global _lib
    if _lib is None:
        d = at._build_dir()
        src = os.path.join(d, "halves_shim.cpp")
        with open(src, "w") as f:
            f.write(SHIM)
        out = os.path.join(d, "libhalvesshim.so")
        subprocess.run(["g++", *CXXFLAGS, "-shared", "-I", CSRC, src, "-o", out], check=True, capture_output=True)
        _lib = C.CDLL(out)
        _lib.shim_pair.argtypes = [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp, C.c_int32, _vp, _vp, _vp, _vp,
                                   _vp, _vp]
    return _lib


def host_pair(SA, QA, SB, QB, n, counts=None, feats=None, **cfg) -> dict:
    """One run of the host build: dict(mean, err, half_means, noise, noise_model, bad_pixels)."""
    c = dict(at.DEFAULTS, **cfg)
    a = [np.ascontiguousarray(x, np.float64) for x in (SA, QA, SB, QB)]
    H, W = a[0].shape[:2]
    cnt = np.ascontiguousarray(counts, np.uint32) if counts is not None else None
    f = [np.ascontiguousarray(x, np.float64) for x in feats] if feats is not None else [None] * 3
    sig = np.array([c["sigma_l"], c["sigma_n"], c["sigma_z"], c["sigma_a"]], np.float64)
    mean, err, hm, noise = np.zeros((H, W, 3)), np.zeros((H, W)), np.zeros((2, H, W, 3)), np.zeros(2)
    bad = C.c_uint64(0)
    p = lambda x: ptr(x) if x is not None else None
    product_host().shim_pair(W, H, *(ptr(x) for x in a), p(cnt), int(n), p(f[0]), p(f[1]), p(f[2]), int(c["iterations"]), ptr(sig),
                             ptr(mean), ptr(err), ptr(hm), ptr(noise), C.byref(bad))
    return dict(mean=mean, err=err, half_means=hm, noise=float(noise[0]), noise_model=float(noise[1]), bad_pixels=bad.value)


def half_counts(n, counts=None):
    """(nA, nB) of the model: scalars for a uniform n, uint32 [H, W] arrays for per-pixel counts."""
    if counts is None:
        return (int(n) + 1) // 2, int(n) // 2
    c = np.asarray(counts, np.uint32)
    return (c + 1) // 2, c // 2


def ref_pair(SA, QA, SB, QB, n, counts=None, feats=None, **cfg) -> dict:
    """The reference: at.ref_filter on each half as a frame of its own, and the combine pixel by pixel in plain Python floats."""
    nA, nB = half_counts(n, counts)
    if counts is None:
        ra = at.ref_filter(SA, QA, nA, None, feats, **cfg)
        rb = at.ref_filter(SB, QB, nB, None, feats, **cfg)
    else:
        ra = at.ref_filter(SA, QA, 0, nA, feats, **cfg)
        rb = at.ref_filter(SB, QB, 0, nB, feats, **cfg)
    fA, fB, vA, vB = ra["mean"], rb["mean"], ra["var"], rb["var"]
    H, W = vA.shape
    mean, err = np.zeros((H, W, 3)), np.zeros((H, W))
    total = model = 0.0
    bad = 0
    fin = lambda v: not (math.isnan(v) or math.isinf(v))
    for y in range(H):
        for x in range(W):
            a = [float(v) for v in fA[y, x]]
            b = [float(v) for v in fB[y, x]]
            m = [(a[k] + b[k]) * 0.5 for k in range(3)]
            d = [(a[k] - b[k]) * 0.5 for k in range(3)]
            e = (d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) / 3.0
            l = (m[0] + m[1] + m[2]) / 3.0
            den = 0.01 if l < 0.01 else l
            e2 = e / (den * den)
            em = ((float(vA[y, x]) + float(vB[y, x])) * 0.25) / (den * den)
            mean[y, x] = m
            err[y, x] = e
            half_bad = not (all(fin(v) for v in a) and fin(float(vA[y, x])) and all(fin(v) for v in b) and fin(float(vB[y, x])))
            if half_bad or not fin(e2):
                bad += 1
                continue
            total += e2
            if fin(em):
                model += em
    np_ = H * W
    return dict(mean=mean, err=err, half_means=np.stack([fA, fB]), noise=math.sqrt(total / np_), noise_model=math.sqrt(model / np_),
                bad_pixels=bad)


def assert_same_pair(a: dict, b: dict, tag="") -> None:
    """Two pair runs agree: half_means, mean and err bit for bit, the two figures to 1e-9, the bad pixels."""
    for k in ("half_means", "mean", "err"):
        assert at.same_bits(a[k], b[k]), (tag, k, int(np.count_nonzero(~np.isclose(a[k], b[k], rtol=0, atol=0, equal_nan=True))))
    for k in ("noise", "noise_model"):
        assert abs(a[k] - b[k]) <= 1e-9 * max(1.0, abs(b[k])), (tag, k, a[k], b[k])
    assert a["bad_pixels"] == b["bad_pixels"], (tag, a["bad_pixels"], b["bad_pixels"])


def half_sums(l: np.ndarray):
    """(SA, QA, SB, QB) of per-sample radiances l [H, W, n, 3]: the sums of moments_support.sums over the even- and the
    odd-indexed samples, each added in sample order from zero."""
    import moments_support as ms

    SA, QA = ms.sums(l[:, :, 0::2])
    SB, QB = ms.sums(l[:, :, 1::2])
    return SA, QA, SB, QB


def figure(var: np.ndarray, ref_mean: np.ndarray) -> float:
    """A per-pixel variance [H, W] (already averaged over the channels) as the frame figure sqrt(mean(var / max(l, 0.01)^2)), l the
    luminance of ref_mean."""
    den = np.maximum(ref_mean.sum(axis=2) / 3.0, 0.01)
    return float(np.sqrt(np.mean(var / (den * den))))


def gpu_pair(ctx, cfg, w: int, h: int) -> dict:
    """pt_atrous_halves on ctx's frame: the dict of host_pair plus the stats."""
    from path_trace_golang_amd import hip

    mean, err, hm = np.zeros((h, w, 3)), np.zeros((h, w)), np.zeros((2, h, w, 3))
    st = hip.atrous_halves(ctx, cfg, mean, err, hm)
    return dict(st, mean=mean, err=err, half_means=hm)


def read_halves(ctx, w: int, h: int):
    from path_trace_golang_amd import hip

    out = tuple(np.full((h, w, 3), -7.0) for _ in range(4))
    hip.read_halves(ctx, *out)
    return out


STOP_SCENE, STOP_DEPTH, STOP_SEED, STOP_CAP, STOP_STEP, STOP_K = "example_simple", 4, 1, 32, 4, 4
_stop = None


def stop_case() -> dict:
    """The stop rule restated on the oracle's samples (40 x 24, cap 32, step 4, k = 4, default sigmas): figures = the measured noise
    after every step, target = a T halfway between the figure of the fourth check and the smallest one before it, count = the
    samples at the first check at or below T.  Computed once."""
    global _stop
    if _stop is None:
        import moments_support as ms

        smp = ms.samples(STOP_SCENE, STOP_DEPTH, STOP_SEED, STOP_CAP)
        feats = at.ref_features(STOP_SCENE, ms.W, ms.H, STOP_CAP, STOP_DEPTH, STOP_SEED, STOP_K)  # k = 4 <= the first check's count
        figures = [ref_pair(*half_sums(smp[:, :, :done]), done, None, feats)["noise"] for done in range(STOP_STEP, STOP_CAP + 1, STOP_STEP)]
        target = 0.5 * (figures[3] + min(figures[:3]))
        count = next((STOP_STEP * (i + 1) for i, f in enumerate(figures) if f <= target), STOP_CAP)
        _stop = dict(figures=figures, target=target, count=count)
    return _stop
