"""Helpers of the fog tests (test_fog_cpu.py, test_fog_gpu.py): builds tests/fog_reference.c -- the independent CPU
restatement of the fog model against the oracle -- and a host build of csrc/pt_fog.h, and loads both with ctypes."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(ROOT, "oracle")
CSRC = os.path.join(ROOT, "path_trace_golang_amd", "csrc")
# the oracle Makefile's flags: Go never fuses multiply-add, no fast-math
CFLAGS = ["-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fno-unsafe-math-optimizations"]
CXXFLAGS = ["-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]

# The host build of pt_fog.h: the product's term for one (ray, stream key) at a time.  The world is converted here the
# way scene_to_world (ptcore.hip) converts it; the light list, the parameters and the term are pt_fog.h's own.
SHIM = r"""
#include <vector>
#include "pt_fog.h"
extern "C" {
void shim_sin_many(const double *x, double *out, int64_t n) { for (int64_t i = 0; i < n; i++) out[i] = ptm::go_sin(x[i]); }
void shim_hash31_many(const double *p, double *out, int64_t n) {
    for (int64_t i = 0; i < n; i++) out[i] = ptf::hash31(p[3 * i], p[3 * i + 1], p[3 * i + 2]);
}
void shim_noise_many(const pt_fog *raw, const double *p, double *out, int64_t n) {
    const ptf::FogParams q = ptf::fog_resolve(*raw);
    for (int64_t i = 0; i < n; i++) out[i] = ptf::volume_noise(q, p[3 * i], p[3 * i + 1], p[3 * i + 2]);
}
void shim_phase_many(const double *ct, const double *g, double *out, int64_t n) {
    for (int64_t i = 0; i < n; i++) out[i] = ptf::phase_hg(ct[i], g[i]);
}
void shim_resolve_flat(const pt_fog *raw, double out[13]) {
    ptf::FogParams p = ptf::fog_resolve(*raw);
    double v[13] = {p.density, p.scatter, p.sigma_s, p.sigma_a, p.g, p.hetero, p.noise_scale, p.color[0], p.color[1], p.color[2],
                    (double)p.octaves, (double)p.affect_sky, (double)p.volumetric};
    for (int i = 0; i < 13; i++) out[i] = v[i];
}
void shim_sky(const pt_fog *raw, pt_sky *sky) {
    ptf::FogParams p = ptf::fog_resolve(*raw);
    if (!ptf::fog_sky_applies(p)) return;
    for (double *c : {sky->background, sky->color, sky->horizon, sky->zenith}) ptf::fog_sky_rewrite(p, c);
}
void shim_inscatter_many(const pt_scene *sc, const pt_fog *raw, int32_t max_depth, int64_t n, const double *rays,
                         const uint64_t *keys, double *L, uint32_t *cnt) {
    ptf::FogParams p = ptf::fog_resolve(*raw);
    std::vector<ptd::DevObj> objs;
    std::vector<ptf::FogLight> lights;
    for (int32_t i = 0; i < sc->num_objects; i++) {
        const pt_object &o = sc->objects[i];
        ptd::DevObj d = {};
        if (o.type == PT_OBJ_SPHERE || o.type == PT_OBJ_SPHERE_LIGHT) {
            d.kind = ptd::KIND_SPHERE;
            for (int k = 0; k < 3; k++) d.a[k] = o.position[k];
            d.radius = o.size[0];
            d.radius_sq = d.radius * d.radius;
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
        objs.push_back(d);
        ptf::FogLight l;
        if (ptf::fog_light_of(*sc, i, l)) lights.push_back(l);
    }
    for (int64_t i = 0; i < n; i++) {
        ptf::FogCount c = {0u, 0u, 0u};
        double *out = L + 3 * i;
        out[0] = out[1] = out[2] = 0;
        if (ptf::fog_volumetric(p, max_depth)) {
            const uint64_t rs = ptm::stream_init(ptm::seed_key(keys[3 * i] ^ PTF_STREAM_SALT), keys[3 * i + 1], keys[3 * i + 2]);
            ptf::fog_inscatter(p, objs.data(), (int32_t)objs.size(), lights.data(), (int32_t)lights.size(), rays + 6 * i,
                               rays + 6 * i + 3, rs, c, out);
        }
        cnt[3 * i] = c.shadow_rays; cnt[3 * i + 1] = c.draws; cnt[3 * i + 2] = c.steps;
    }
}
}
"""

_dir = None
_libs = {}


def _build_dir() -> str:
    global _dir
    if _dir is None:
        _dir = tempfile.mkdtemp(prefix="fogtest_")
    return _dir


def reference():
    """fog_reference.c linked against oracle/libptoracle.so."""
    if "ref" not in _libs:
        from oracle import ora

        ora.lib()  # builds oracle/libptoracle.so when missing
        out = os.path.join(_build_dir(), "libfogref.so")
        subprocess.run(["gcc", *CFLAGS, "-shared", "-I", ORACLE, os.path.join(ROOT, "tests", "fog_reference.c"), "-o", out,
                        "-L", ORACLE, "-Wl,-rpath," + ORACLE, "-lptoracle", "-lm"], check=True, capture_output=True)
        L = C.CDLL(out)
        _vp = C.c_void_p
        L.fr_sin_many.argtypes = [_vp, _vp, C.c_int64]
        L.fr_resolve_flat.argtypes = [_vp, _vp]
        L.fr_sky.argtypes = [_vp, _vp]
        L.fr_inscatter_many.argtypes = [_vp, _vp, C.c_int32, C.c_int64, _vp, _vp, _vp, _vp]
        L.fr_render.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp]
        L.fr_render.restype = C.c_int
        L.fr_hash31_many.argtypes = [_vp, _vp, C.c_int64]
        L.fr_noise_many.argtypes = [_vp, _vp, _vp, C.c_int64]
        L.fr_phase_many.argtypes = [_vp, _vp, _vp, C.c_int64]
        L.fr_ora_unary_many.argtypes = [C.c_int, _vp, _vp, C.c_int64]
        L.fr_ora_binary_many.argtypes = [C.c_int, _vp, _vp, _vp, C.c_int64]
        L.fr_ora_streams.argtypes = [_vp, C.c_int32, _vp, _vp, C.c_int64]
        _libs["ref"] = L
    return _libs["ref"]


def product_host():
    """csrc/pt_fog.h built for the host with g++."""
    if "shim" not in _libs:
        d = _build_dir()
        src = os.path.join(d, "fog_shim.cpp")
        with open(src, "w") as f:
            f.write(SHIM)
        out = os.path.join(d, "libfogshim.so")
        subprocess.run(["g++", *CXXFLAGS, "-shared", "-I", CSRC, src, "-o", out], check=True, capture_output=True)
        L = C.CDLL(out)
        _vp = C.c_void_p
        L.shim_sin_many.argtypes = [_vp, _vp, C.c_int64]
        L.shim_resolve_flat.argtypes = [_vp, _vp]
        L.shim_sky.argtypes = [_vp, _vp]
        L.shim_inscatter_many.argtypes = [_vp, _vp, C.c_int32, C.c_int64, _vp, _vp, _vp, _vp]
        L.shim_hash31_many.argtypes = [_vp, _vp, C.c_int64]
        L.shim_noise_many.argtypes = [_vp, _vp, _vp, C.c_int64]
        L.shim_phase_many.argtypes = [_vp, _vp, _vp, C.c_int64]
        _libs["shim"] = L
    return _libs["shim"]


def ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def fog_struct(**kw):
    """A PtFog (the raw scene.Fog fields) from keyword arguments."""
    from path_trace_golang_amd import capi

    f = capi.PtFog()
    for k, v in kw.items():
        if k == "color":
            f.color[:] = list(v)
        else:
            setattr(f, k, v)
    return f


def fog_of_scene(doc_fog: dict):
    """The PtFog of a scene file's "fog" object, through the package's own scene loader and flattening."""
    from path_trace_golang_amd import hip, scene

    return hip.pt_fog(scene.Fog.decode(doc_fog))


def reference_render(ora_scene, w, h, spp, depth, seed, fog):
    """fr_render: (rgba uint8 [H,W,4], accum f64 [H,W,3], stats dict)."""
    from oracle import ora

    L = reference()
    cfg = ora.OraConfig(w, h, spp, depth, seed, 1, 0)
    rgba = np.zeros((h, w, 4), np.uint8)
    acc = np.zeros((h, w, 3), np.float64)
    st = np.zeros(5, np.uint64)
    L.fr_render(C.byref(ora_scene.c), C.byref(cfg), C.byref(fog), ptr(rgba), ptr(acc), ptr(st))
    return rgba, acc, dict(zip(("segments", "draws", "shadow_rays", "fog_draws", "steps"), (int(v) for v in st)))
