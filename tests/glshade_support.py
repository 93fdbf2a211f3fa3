"""Helpers of the GL-shading tests (test_glshade_cpu.py, test_glshade_gpu.py): builds tests/glshade_reference.c -- the
independent CPU restatement of GL shading against the oracle -- and a host build of csrc/pt_glshade.h, and loads both with
ctypes."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from fog_support import CFLAGS, CSRC, CXXFLAGS, ORACLE, ROOT, ptr

# The host build of pt_glshade.h: the product's pass sum for one job at a time, on the tables frame_open (ptcore.hip) builds
# from the same calls.  The fog term's CPU world is converted the way scene_to_world converts it (as in fog_support.py).
SHIM = r"""
#include <cstddef>
#include <vector>
#include "pt_glshade.h"
extern "C" {
void shim_material(const pt_material *m, const pt_gl_material *x, double out[19]) {
    ptg::GlMat g = ptg::gl_material(*m, *x);
    double v[19] = {(double)g.type, g.rough, g.ior, g.smoothness, g.reflectivity, g.albedo[0], g.albedo[1], g.albedo[2],
                    g.emit[0], g.emit[1], g.emit[2], g.absorption[0], g.absorption[1], g.absorption[2], g.absorption_scale,
                    g.tint[0], g.tint[1], g.tint[2], 0};
    for (int i = 0; i < 19; i++) out[i] = v[i];
}
int shim_sizes(int32_t out[4]) {
    out[0] = (int32_t)sizeof(pt_gl_material); out[1] = (int32_t)sizeof(pt_shading); out[2] = (int32_t)sizeof(pt_shading_stats);
    out[3] = PT_ABI_VERSION;
    return 4;
}
void shim_pass_many(const pt_scene *sc, const pt_gl_material *ex, int32_t w, int32_t h, int32_t depth, uint64_t seed,
                    const pt_fog *fog, int64_t n, const int32_t *jobs, double *out, uint64_t *cnt) {
    const int32_t nmat = sc->num_materials;
    std::vector<ptg::GlMat> mats((size_t)(nmat > 0 ? nmat : 1), ptg::GlMat{});
    for (int32_t i = 0; i < nmat; i++) mats[(size_t)i] = ptg::gl_material(sc->materials[i], ex[i]);
    std::vector<ptg::GlObj> objs;
    std::vector<int32_t> lights;
    for (int32_t i = 0; i < sc->num_objects; i++) {
        objs.push_back(ptg::gl_object(sc->objects[i], nmat));
        if (ptg::gl_is_light(*sc, i)) lights.push_back(i);
    }
    ptg::GlScene S = {};
    S.objs = objs.data(); S.mats = mats.data(); S.lights = lights.data();
    S.nobj = (int32_t)objs.size(); S.nlight = (int32_t)lights.size();
    pt_sky sky = sc->sky;
    std::vector<ptd::DevObj> fobjs;
    std::vector<ptf::FogLight> flights;
    if (fog) {
        S.fog = ptf::fog_resolve(*fog);
        if (ptf::fog_sky_applies(S.fog))
            for (double *c : {sky.background, sky.color, sky.horizon, sky.zenith}) ptf::fog_sky_rewrite(S.fog, c);
        S.fog_on = ptf::fog_volumetric(S.fog, depth) ? 1 : 0;
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
            fobjs.push_back(d);
            ptf::FogLight l;
            if (ptf::fog_light_of(*sc, i, l)) flights.push_back(l);
        }
        S.fog_objs = fobjs.data(); S.fog_nobj = (int32_t)fobjs.size();
        S.fog_lights = flights.data(); S.fog_nlight = (int32_t)flights.size();
    }
    S.sky = ptg::gl_sky(sky);
    S.cam = ptg::gl_camera(sc->camera, w, h);
    S.max_depth = depth; S.width = w; S.height = h;
    const uint64_t key = ptm::seed_key(seed ^ PTG_STREAM_SALT), fkey = ptm::seed_key(seed ^ PTF_STREAM_SALT);
    for (int64_t i = 0; i < n; i++) {
        ptg::GlCount c = {0u, 0u, 0u, 0u, 0u};
        ptf::FogCount f = {0u, 0u, 0u};
        ptg::gl_pass(S, key, fkey, jobs[3 * i], jobs[3 * i + 1], (uint32_t)jobs[3 * i + 2], c, f, out + 3 * i);
        uint64_t v[8] = {c.paths, c.segments, c.shadow_rays, c.probe_rays, c.draws, f.shadow_rays, f.draws, f.steps};
        for (int k = 0; k < 8; k++) cnt[8 * i + k] = v[k];
    }
}
}
"""

COUNTERS = ("paths", "segments", "shadow_rays", "probe_rays", "draws", "fog_shadow_rays", "fog_draws", "fog_steps")

_dir = None
_libs = {}


def _build_dir() -> str:
    global _dir
    if _dir is None:
        _dir = tempfile.mkdtemp(prefix="glshadetest_")
    return _dir


def reference():
    """glshade_reference.c (with fog_reference.c inside) linked against oracle/libptoracle.so."""
    if "ref" not in _libs:
        from oracle import ora

        ora.lib()  # builds oracle/libptoracle.so when missing
        out = os.path.join(_build_dir(), "libglshaderef.so")
        subprocess.run(["gcc", *CFLAGS, "-shared", "-I", ORACLE, "-I", os.path.join(ROOT, "tests"),
                        os.path.join(ROOT, "tests", "glshade_reference.c"), "-o", out, "-L", ORACLE,
                        "-Wl,-rpath," + ORACLE, "-lptoracle", "-lm"], check=True, capture_output=True)
        L = C.CDLL(out)
        _vp = C.c_void_p
        L.gr_material.argtypes = [_vp, _vp, _vp]
        L.gr_pass_many.argtypes = [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, _vp, C.c_int64, _vp, _vp, _vp]
        L.gr_render.argtypes = [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, _vp, _vp, _vp, _vp]
        _libs["ref"] = L
    return _libs["ref"]


def product_host():
    """csrc/pt_glshade.h built for the host with g++."""
    if "shim" not in _libs:
        d = _build_dir()
        src = os.path.join(d, "glshade_shim.cpp")
        with open(src, "w") as f:
            f.write(SHIM)
        out = os.path.join(d, "libglshadeshim.so")
        subprocess.run(["g++", *CXXFLAGS, "-shared", "-I", CSRC, src, "-o", out], check=True, capture_output=True)
        L = C.CDLL(out)
        _vp = C.c_void_p
        L.shim_material.argtypes = [_vp, _vp, _vp]
        L.shim_sizes.argtypes = [_vp]
        L.shim_pass_many.argtypes = [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, _vp, C.c_int64, _vp, _vp, _vp]
        _libs["shim"] = L
    return _libs["shim"]


def extras(sc):
    """The scene's pt_gl_material table, through the package's own flattening."""
    from path_trace_golang_amd import hip

    return hip.gl_materials(sc)


def _fogp(fog):
    return C.byref(fog) if fog is not None else None


def ref_passes(ora_scene, ex, w, h, depth, seed, jobs: np.ndarray, fog=None):
    """(radiance f64 [n,3], counters u64 [n,8]) of the restatement for int32 jobs [n,3] = (x, y, pass)."""
    jobs = np.ascontiguousarray(jobs, np.int32)
    n = jobs.shape[0]
    out = np.zeros((n, 3), np.float64)
    cnt = np.zeros((n, 8), np.uint64)
    reference().gr_pass_many(C.byref(ora_scene.c), C.cast(ex, C.c_void_p), w, h, depth, seed, _fogp(fog), n, ptr(jobs), ptr(out),
                             ptr(cnt))
    return out, cnt


def host_passes(flat_scene, ex, w, h, depth, seed, jobs: np.ndarray, fog=None):
    """The same from the host build of pt_glshade.h (flat_scene: hip.FlatScene)."""
    jobs = np.ascontiguousarray(jobs, np.int32)
    n = jobs.shape[0]
    out = np.zeros((n, 3), np.float64)
    cnt = np.zeros((n, 8), np.uint64)
    product_host().shim_pass_many(C.byref(flat_scene.c), C.cast(ex, C.c_void_p), w, h, depth, seed, _fogp(fog), n, ptr(jobs),
                                  ptr(out), ptr(cnt))
    return out, cnt


def reference_render(ora_scene, ex, w, h, passes, depth, seed, fog=None):
    """gr_render: (rgba uint8 [H,W,4], accum f64 [H,W,3], stats dict)."""
    rgba = np.zeros((h, w, 4), np.uint8)
    acc = np.zeros((h, w, 3), np.float64)
    st = np.zeros(8, np.uint64)
    reference().gr_render(C.byref(ora_scene.c), C.cast(ex, C.c_void_p), w, h, passes, depth, seed, _fogp(fog), ptr(rgba), ptr(acc),
                          ptr(st))
    return rgba, acc, dict(zip(COUNTERS, (int(v) for v in st)))


# ---------------------------------------------------------------- synthetic scenes (JSON documents)
def _v(x, y, z):
    return {"x": x, "y": y, "z": z}


def _c(r, g, b):
    return {"r": r, "g": g, "b": b}


def _mat(id_, type_, albedo=(0.7, 0.7, 0.7), **kw):
    m = {"id": id_, "type": type_, "albedo": _c(*albedo), "rough": 0, "ior": 1.5, "emit": _c(0, 0, 0), "power": 0,
         "absorption": _c(0, 0, 0)}
    for k, v in kw.items():
        m[k] = _c(*v) if k in ("emit", "absorption", "tint") else v
    return m


def _obj(id_, type_, pos, size, mat):
    return {"id": id_, "type": type_, "position": _v(*pos), "size": _v(*size), "material_id": mat}


def _doc(objects, materials, sky=None, aperture=0.0, fov=50, aspect=0):
    return {"name": "synthetic", "camera": {"position": _v(0, 2.5, 9), "target": _v(0, 1, 0), "up": _v(0, 1, 0), "fov": fov,
                                             "aperture": aperture, "focus_dist": 0, "aspect_ratio": aspect},
            "objects": objects, "materials": materials, "background": _c(0.2, 0.25, 0.3),
            "sky": sky if sky is not None else {"type": "gradient", "horizon": _c(0.8, 0.85, 0.9), "zenith": _c(0.3, 0.4, 0.7)}}


def synthetic_docs() -> dict:
    """Scenes for the corners the shipped ones miss: the 8-light subset rule, the object / material edge cases, glass
    absorption and tint, metals with smoothness / reflectivity set."""
    many = [_mat("floor", "lambert", (0.6, 0.6, 0.55)), _mat("red", "lambert", (0.8, 0.2, 0.2)),
            _mat("rough", "metal", (0.9, 0.8, 0.6), rough=0.4)]
    objs = [_obj("floor", "plane", (0, 0, 0), (0, 0, 0), "floor"), _obj("s1", "sphere", (-1, 1, 0), (1, 1, 1), "red"),
            _obj("s2", "sphere", (1.2, 0.8, 0.5), (0.8, 0, 0), "rough")]
    for i in range(12):
        many.append(_mat("l%d" % i, "emissive", emit=(1.0, 0.8 + 0.01 * i, 0.6), power=3.0 + i))
        objs.append(_obj("lamp%d" % i, "sphere_light" if i % 2 else "sphere", (-3.3 + 0.6 * i, 3.5 + 0.1 * (i % 3), -1 + 0.2 * i),
                         (0.15, 0, 0), "l%d" % i))
    twelve = _doc(objs, many)

    edge_m = [_mat("first", "lambert", (0.5, 0.6, 0.7)), _mat("glow", "emissive", emit=(2, 2, 1.5), power=4),
              _mat("boxglow", "emissive", emit=(1, 0.5, 0.2), power=5), _mat("dim", "emissive", emit=(0.5, 0.5, 0.5), power=0),
              _mat("weird", "velvet", (0.3, 0.9, 0.3))]
    edge_o = [_obj("floor", "plane", (0, 0, 0), (0, 0, 0), "first"),
              _obj("nomat", "sphere", (-1.5, 1, 0), (1, 0, 0), "does-not-exist"),
              _obj("torus", "torus", (1.5, 1, -0.5), (0.9, 0.4, 0), "weird"),
              _obj("boxlight", "box", (0, 3.5, -1), (1.5, 0.2, 1.5), "boxglow"),
              _obj("sun", "sphere_light", (2.5, 4, 2), (0.4, 0, 0), "glow"),
              _obj("dimlamp", "sphere", (-2.5, 3, 1), (0.3, 0, 0), "dim"),
              _obj("cube", "box", (0.2, 0.5, 1.5), (1, 1, 1), "weird")]
    edge = _doc(edge_o, edge_m, sky={"type": "solid", "color": _c(0.4, 0.5, 0.6)}, aperture=0.2, aspect=1.5)

    glass_m = [_mat("floor", "lambert", (0.7, 0.7, 0.7)), _mat("lamp", "emissive", emit=(3, 3, 3), power=2),
               _mat("green", "dielectric", (1, 1, 1), ior=1.5, absorption=(0.5, 0.1, 0.8), absorption_scale=0.3,
                    tint=(0.6, 1.0, 0.7)),
               _mat("plain", "dielectric", (1, 1, 1), ior=1.33, absorption=(0.2, 0.2, 0.05)),
               _mat("dense", "dielectric", (1, 1, 1), ior=2.4, absorption=(1.5, 0.4, 0.2), absorption_scale=1.0)]
    glass_o = [_obj("floor", "plane", (0, 0, 0), (0, 0, 0), "floor"), _obj("lamp", "sphere", (0, 5, 1), (0.8, 0, 0), "lamp"),
               _obj("gbox", "box", (-1.3, 0.8, 0), (1.4, 1.6, 1.2), "green"), _obj("gball", "sphere", (1.2, 1, 0.3), (1, 0, 0), "plain"),
               _obj("gem", "sphere", (0.1, 0.5, 2), (0.5, 0, 0), "dense"), _obj("slab", "box", (0, 0.3, 3), (3, 0.6, 0.4), "dense")]
    glass = _doc(glass_o, glass_m)

    metal_m = [_mat("floor", "lambert", (0.5, 0.5, 0.5)), _mat("lamp", "emissive", emit=(4, 3.5, 3), power=3),
               _mat("brushed", "metal", (0.9, 0.85, 0.8), rough=0.2, smoothness=0.35, reflectivity=0.7),
               _mat("oldstyle", "metal", (0.8, 0.8, 0.9), rough=0.6),
               _mat("polished", "metal", (0.95, 0.9, 0.8), rough=0.0, smoothness=1.0, reflectivity=1.4),
               _mat("mirror", "mirror", (0.9, 0.9, 0.9), reflectivity=0.5),
               _mat("neg", "metal", (0.7, 0.7, 0.7), rough=0.3, smoothness=-0.5, reflectivity=-1.0)]
    metal_o = [_obj("floor", "plane", (0, 0, 0), (0, 0, 0), "floor"), _obj("lamp", "sphere", (0, 4.5, 2), (0.7, 0, 0), "lamp"),
               _obj("lampbox", "box", (3, 3, -2), (1, 1, 1), "lamp"),
               _obj("m1", "sphere", (-2, 1, 0), (1, 0, 0), "brushed"), _obj("m2", "sphere", (0, 1, -0.5), (1, 0, 0), "oldstyle"),
               _obj("m3", "box", (2, 1, 0), (1.5, 2, 1.5), "polished"), _obj("m4", "box", (0, 1.5, -3), (6, 3, 0.3), "mirror"),
               _obj("m5", "sphere", (1, 0.4, 2), (0.4, 0, 0), "neg")]
    metal = _doc(metal_o, metal_m, sky=None)
    return {"twelve_lights": twelve, "edge": edge, "glass": glass, "metal": metal}


def scene_pair(doc: dict, tmp_dir: str, name: str):
    """(scene.Scene, hip.FlatScene, ora.Scene) of a document, the package's scene through its own loader."""
    import json

    from oracle import ora
    from path_trace_golang_amd import hip, scene

    p = os.path.join(tmp_dir, name + ".json")
    with open(p, "w") as f:
        json.dump(doc, f)
    sc = scene.load(p)
    return sc, hip.FlatScene(sc), ora.Scene(doc)
