"""Helpers of the a-trous tests (test_atrous_cpu.py, test_atrous_gpu.py): builds tests/atrous_reference.c -- the independent
CPU restatement of the feature planes and of the filter against the oracle -- and a host build of csrc/pt_atrous.h, loads both
with ctypes, and derives the oracle-side inputs (sums, features) of the shipped scenes once per (scene, seed)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from fog_support import CFLAGS, CSRC, CXXFLAGS, ORACLE, ROOT, ptr

DEFAULTS = dict(iterations=5, sigma_l=4.0, sigma_n=0.1, sigma_z=0.1, sigma_a=0.2)

# The host build of pt_atrous.h: the product's per-pixel functions, looped over a frame the way pt_atrous's kernels are
# launched (prep, T ping-pong iterations, finish), and first_hit over a list of rays with the world converted the way
# scene_to_world (ptcore.hip) converts it.
SHIM = r"""
#include <cmath>
#include <cstring>
#include <vector>
#include "pt_atrous.h"
extern "C" {
void shim_filter(int32_t W, int32_t H, const double *S, const double *Q, const uint32_t *cnt, uint32_t n, const double *fn,
                 const double *fa, const double *fd, int32_t T, const double *sig, double *mean, double *var, uint8_t *rgba,
                 double *noise, uint64_t *bad) {
    const size_t np = (size_t)W * (size_t)H;
    const bool feat = fn && fa && fd;
    std::vector<double> col[2] = {std::vector<double>(3 * np), std::vector<double>(3 * np)};
    std::vector<double> v[2] = {std::vector<double>(np), std::vector<double>(np)};
    std::vector<pta::Guide> g(np);
    *bad = 0;
    for (size_t i = 0; i < np; i++) {
        pta::prep_pixel(S + 3 * i, Q + 3 * i, cnt ? cnt[i] : n, feat ? fn + 3 * i : nullptr, feat ? fa + 3 * i : nullptr,
                        feat ? fd + 3 * i : nullptr, &col[0][3 * i], v[0][i], g[i]);
        *bad += g[i].bad != 0.0;
    }
    pta::Params P;
    std::memset(&P, 0, sizeof P);
    P.sigma_l = sig[0]; P.sigma_n = sig[1]; P.sigma_z = sig[2]; P.sigma_a = sig[3];
    P.iterations = T;
    P.n_on = feat && sig[1] > 0; P.z_on = feat && sig[2] > 0; P.a_on = feat && sig[3] > 0;
    auto figure = [&](int k) {
        double s = 0;
        for (size_t i = 0; i < np; i++) s += pta::noise_term(&col[k][3 * i], v[k][i]);
        return std::sqrt(s / (double)np);
    };
    noise[0] = figure(0);
    int cur = 0;
    for (int32_t t = 0; t < T; t++, cur ^= 1)
        for (int32_t y = 0; y < H; y++)
            for (int32_t x = 0; x < W; x++) {
                const size_t i = (size_t)y * W + x;
                pta::filter_pixel(P, W, H, x, y, 1 << t, col[cur].data(), v[cur].data(), g.data(), &col[cur ^ 1][3 * i], v[cur ^ 1][i]);
            }
    noise[1] = figure(cur);
    for (size_t i = 0; i < np; i++) {
        for (int k = 0; k < 3; k++) mean[3 * i + k] = col[cur][3 * i + k];
        var[i] = v[cur][i];
        const uint32_t p = pta::finish_pack(&col[cur][3 * i]);
        std::memcpy(rgba + 4 * i, &p, 4);
    }
}
void shim_first_hit_many(const pt_scene *sc, int64_t n, const double *rays, double *out) {
    std::vector<ptd::DevObj> objs;
    std::vector<ptd::DevMat> mats((size_t)sc->num_materials + 1);
    std::memset(mats.data(), 0, mats.size() * sizeof(ptd::DevMat));
    for (int32_t i = 0; i < sc->num_materials; i++) {  // the albedo of convertMaterial (materials.go:28-55): every type but emissive
        const pt_material &m = sc->materials[i];
        if (m.type != PT_MAT_EMISSIVE)
            for (int k = 0; k < 3; k++) mats[(size_t)i].albedo[k] = m.albedo[k];
    }
    for (int32_t i = 0; i < sc->num_objects; i++) {
        const pt_object &o = sc->objects[i];
        ptd::DevObj d = {};
        if (o.type == PT_OBJ_SPHERE || o.type == PT_OBJ_SPHERE_LIGHT) {
            d.kind = ptd::KIND_SPHERE;
            for (int k = 0; k < 3; k++) d.a[k] = o.position[k];
            d.radius = o.size[0];
            d.radius_sq = d.radius * d.radius;
            d.inv_radius = 1.0 / d.radius;
        } else if (o.type == PT_OBJ_PLANE) {
            d.kind = ptd::KIND_PLANE;
            for (int k = 0; k < 3; k++) d.a[k] = o.position[k];
            d.b[1] = 1;
        } else if (o.type == PT_OBJ_BOX) {
            d.kind = ptd::KIND_BOX;
            for (int k = 0; k < 3; k++) { d.a[k] = o.position[k] - o.size[k] * 0.5; d.b[k] = o.position[k] + o.size[k] * 0.5; }
        } else {
            continue;
        }
        d.mat = (o.material >= 0 && o.material < sc->num_materials) ? o.material : sc->num_materials;
        objs.push_back(d);
    }
    for (int64_t i = 0; i < n; i++) {
        double *r = out + 8 * i;
        for (int k = 0; k < 8; k++) r[k] = 0;
        double nn[3], a[3], dist;
        if (pta::first_hit(objs.data(), mats.data(), (int32_t)objs.size(), rays + 6 * i, rays + 6 * i + 3, nn, a, dist)) {
            r[0] = 1;
            for (int k = 0; k < 3; k++) { r[1 + k] = nn[k]; r[4 + k] = a[k]; }
            r[7] = dist;
        }
    }
}
}
"""

_dir = None
_libs = {}
_cache = {}


def _build_dir() -> str:
    global _dir
    if _dir is None:
        _dir = tempfile.mkdtemp(prefix="atroustest_")
    return _dir


_vp = C.c_void_p
_FILTER_ARGS = [C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp]


def reference():
    """atrous_reference.c linked against oracle/libptoracle.so."""
    if "ref" not in _libs:
        from oracle import ora

        ora.lib()  # builds oracle/libptoracle.so when missing
        out = os.path.join(_build_dir(), "libatrousref.so")
        subprocess.run(["gcc", *CFLAGS, "-shared", "-I", ORACLE, os.path.join(ROOT, "tests", "atrous_reference.c"), "-o", out,
                        "-L", ORACLE, "-Wl,-rpath," + ORACLE, "-lptoracle", "-lm"], check=True, capture_output=True)
        L = C.CDLL(out)
        L.ar_filter.argtypes = _FILTER_ARGS
        L.ar_features.argtypes = [_vp, _vp, C.c_int32, _vp, _vp, _vp, _vp]
        L.ar_first_hit_many.argtypes = [_vp, C.c_int64, _vp, _vp]
        _libs["ref"] = L
    return _libs["ref"]


def product_host():
    """csrc/pt_atrous.h built for the host with g++."""
    if "shim" not in _libs:
        d = _build_dir()
        src = os.path.join(d, "atrous_shim.cpp")
        with open(src, "w") as f:
            f.write(SHIM)
        out = os.path.join(d, "libatrousshim.so")
        subprocess.run(["g++", *CXXFLAGS, "-shared", "-I", CSRC, src, "-o", out], check=True, capture_output=True)
        L = C.CDLL(out)
        L.shim_filter.argtypes = _FILTER_ARGS
        L.shim_first_hit_many.argtypes = [_vp, C.c_int64, _vp, _vp]
        _libs["shim"] = L
    return _libs["shim"]


def _filter(fn, S, Q, n, counts=None, feats=None, **cfg):
    """One filter run through `fn` (ar_filter or shim_filter): dict(mean, var, rgba, noise_before, noise_after, bad_pixels)."""
    c = dict(DEFAULTS, **cfg)
    S = np.ascontiguousarray(S, np.float64)
    Q = np.ascontiguousarray(Q, np.float64)
    H, W = S.shape[:2]
    cnt = np.ascontiguousarray(counts, np.uint32) if counts is not None else None
    f = [np.ascontiguousarray(a, np.float64) for a in feats] if feats is not None else [None] * 3
    sig = np.array([c["sigma_l"], c["sigma_n"], c["sigma_z"], c["sigma_a"]], np.float64)
    mean = np.zeros((H, W, 3))
    var = np.zeros((H, W))
    rgba = np.zeros((H, W, 4), np.uint8)
    noise = np.zeros(2)
    bad = C.c_uint64(0)
    p = lambda a: ptr(a) if a is not None else None
    fn(W, H, ptr(S), ptr(Q), p(cnt), int(n), p(f[0]), p(f[1]), p(f[2]), int(c["iterations"]), ptr(sig), ptr(mean), ptr(var),
       ptr(rgba), ptr(noise), C.byref(bad))
    return dict(mean=mean, var=var, rgba=rgba, noise_before=float(noise[0]), noise_after=float(noise[1]), bad_pixels=bad.value)


def ref_filter(S, Q, n, counts=None, feats=None, **cfg):
    return _filter(reference().ar_filter, S, Q, n, counts, feats, **cfg)


def host_filter(S, Q, n, counts=None, feats=None, **cfg):
    return _filter(product_host().shim_filter, S, Q, n, counts, feats, **cfg)


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    """Bit equality of two float64 arrays, any NaN equal to any NaN (the payload of a NaN is not part of the model)."""
    a = np.ascontiguousarray(a, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all(nan | (a.view(np.uint64) == b.view(np.uint64))))


def assert_same_run(a: dict, b: dict, tag="") -> None:
    """Two filter runs agree: mean, var and rgba bit for bit, the noise figures to 1e-9 (the order of that sum is the reduction's)."""
    for k in ("mean", "var"):
        assert same_bits(a[k], b[k]), (tag, k, int(np.count_nonzero(~(np.isclose(a[k], b[k], rtol=0, atol=0, equal_nan=True)))))
    assert np.array_equal(a["rgba"], b["rgba"]), (tag, "rgba", int(np.count_nonzero(a["rgba"] != b["rgba"])))
    for k in ("noise_before", "noise_after"):
        assert abs(a[k] - b[k]) <= 1e-9 * max(1.0, abs(b[k])), (tag, k, a[k], b[k])
    if "bad_pixels" in a and "bad_pixels" in b:
        assert a["bad_pixels"] == b["bad_pixels"], (tag, a["bad_pixels"], b["bad_pixels"])


def ora_scene_of(path_or_name: str):
    """An oracle scene by shipped name or by file path (cached)."""
    from oracle import ora

    from conftest import scene_path

    path = path_or_name if os.path.sep in path_or_name or path_or_name.endswith(".json") else scene_path(path_or_name)
    if ("scene", path) not in _cache:
        _cache[("scene", path)] = ora.Scene.load(path)
    return _cache[("scene", path)]


def ref_features(scene, w: int, h: int, spp: int, depth: int, seed: int, k: int, counts=None):
    """(normal, albedo, depth) float64 [H, W, 3]: the oracle-derived feature sums of a frame; counts (uint32 [H, W]) = the
    samples each pixel holds in an adaptive frame (None: spp everywhere).  `scene` = shipped name, path or ora.Scene."""
    from oracle import ora

    sc = ora_scene_of(scene) if isinstance(scene, str) else scene
    key = ("feat", id(sc), w, h, spp, depth, seed, k, None if counts is None else counts.tobytes())
    if key not in _cache:
        cfg = ora.OraConfig(w, h, spp, depth, seed, 1, 0)
        cnt = np.ascontiguousarray(counts, np.uint32) if counts is not None else None
        out = [np.zeros((h, w, 3)) for _ in range(3)]
        reference().ar_features(C.byref(sc.c), C.byref(cfg), k, ptr(cnt) if cnt is not None else None, *(ptr(a) for a in out))
        for a in out:
            a.setflags(write=False)
        _cache[key] = tuple(out)
    return _cache[key]


def oracle_inputs(name: str, spp: int = 16, depth: int = 4, seed: int = 1, k: int = 4):
    """The filter's inputs for a shipped scene at moments_support's 40 x 24 from oracle samples only: (S, Q, feats)."""
    import moments_support as ms

    key = ("inputs", name, spp, depth, seed, k)
    if key not in _cache:
        S, Q = ms.sums(ms.samples(name, depth, seed, spp))
        _cache[key] = (S, Q, ref_features(name, ms.W, ms.H, spp, depth, seed, k))
    return _cache[key]


def relative_mse(mean: np.ndarray, ref_mean: np.ndarray) -> float:
    """Per-pixel squared error (mean over the channels) over max(reference mean luminance, 0.01)^2, averaged over the frame:
    the normalisation of pt_noise_estimate."""
    den = np.maximum(ref_mean.sum(axis=2) / 3.0, 0.01)
    return float(np.mean(((mean - ref_mean) ** 2).mean(axis=2) / (den * den)))


def atrous_config(**kw):
    from path_trace_golang_amd import hip

    c = dict(DEFAULTS, **kw)
    return hip.AtrousConfig(c["iterations"], c["sigma_l"], c["sigma_n"], c["sigma_z"], c["sigma_a"])


def gpu_run(ctx, cfg, w: int, h: int) -> dict:
    """pt_atrous on ctx's frame: the dict of _filter plus the stats."""
    from path_trace_golang_amd import hip

    img = np.zeros((h, w, 4), np.uint8)
    mean = np.zeros((h, w, 3))
    var = np.zeros((h, w))
    st = hip.atrous(ctx, cfg, img, mean, var)
    return dict(st, mean=mean, var=var, rgba=img)
