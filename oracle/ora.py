"""ctypes harness for the CPU oracle -- TEST INFRASTRUCTURE ONLY.

Loads oracle/libptoracle.so (built by oracle/Makefile) and feeds it scene JSON
decoded the way Go's encoding/json fills scene.Scene (internal/scene/scene.go,
internal/scene/io.go:10-22): missing keys are zero values, keys match
case-insensitively, `"sky": null` leaves Sky nil.  Nothing under
path_trace_golang_amd/ imports this module.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get("PTORACLE_LIB") or os.path.join(_HERE, "libptoracle.so")  # PTORACLE_LIB: a sanitizer build (oracle/Makefile)


class OraMaterial(C.Structure):
    _fields_ = [("type", C.c_int32), ("_pad", C.c_int32), ("albedo", C.c_double * 3), ("rough", C.c_double),
                ("ior", C.c_double), ("emit", C.c_double * 3), ("power", C.c_double),
                ("absorption", C.c_double * 3), ("smoothness", C.c_double)]


class OraObject(C.Structure):
    _fields_ = [("type", C.c_int32), ("material", C.c_int32), ("position", C.c_double * 3),
                ("size", C.c_double * 3)]


class OraCamera(C.Structure):
    _fields_ = [("position", C.c_double * 3), ("target", C.c_double * 3), ("up", C.c_double * 3),
                ("fov", C.c_double), ("aperture", C.c_double), ("focus_dist", C.c_double),
                ("aspect_ratio", C.c_double)]


class OraSky(C.Structure):
    _fields_ = [("sky_type", C.c_int32), ("_pad", C.c_int32), ("background", C.c_double * 3),
                ("color", C.c_double * 3), ("horizon", C.c_double * 3), ("zenith", C.c_double * 3)]


class OraScene(C.Structure):
    _fields_ = [("camera", OraCamera), ("sky", OraSky), ("nmaterials", C.c_int32), ("nobjects", C.c_int32),
                ("materials", C.POINTER(OraMaterial)), ("objects", C.POINTER(OraObject))]


class OraConfig(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("spp", C.c_int32), ("max_depth", C.c_int32),
                ("seed", C.c_uint64), ("workers", C.c_int32), ("_pad", C.c_int32)]


class OraPostConfig(C.Structure):
    _fields_ = [("tonemap", C.c_int32), ("denoise", C.c_int32), ("sigma_s", C.c_double), ("sigma_r", C.c_double),
                ("smooth", C.c_int32), ("smooth_radius", C.c_int32), ("smooth_strength", C.c_double)]


class OraStats(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("segments", C.c_uint64), ("exit_scans", C.c_uint64),
                ("draws", C.c_uint64), ("seconds", C.c_double), ("workers", C.c_int32), ("_pad", C.c_int32)]


def build(force: bool = False) -> str:
    """Compile the oracle if the .so is missing or older than its sources."""
    srcs = [os.path.join(_HERE, f) for f in ("pt_oracle.c", "pt_oracle.h", "Makefile")]
    stale = force or not os.path.exists(_LIB_PATH) or any(
        os.path.getmtime(s) > os.path.getmtime(_LIB_PATH) for s in srcs)
    if stale:
        subprocess.run(["make", "-C", _HERE, "libptoracle.so"], check=True, capture_output=True)
    return _LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(_LIB_PATH)
        dp = C.POINTER(C.c_double)
        L.ora_render.restype = C.c_int
        L.ora_render.argtypes = [C.POINTER(OraScene), C.POINTER(OraConfig), C.c_void_p, C.c_int32, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.POINTER(OraStats)]
        L.ora_render_window.restype = C.c_int
        L.ora_render_window.argtypes = [C.POINTER(OraScene), C.POINTER(OraConfig), C.c_int32, C.c_int32, C.c_int32,
                                        C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.POINTER(OraStats)]
        L.ora_sample.restype = None
        L.ora_sample.argtypes = [C.POINTER(OraScene), C.POINTER(OraConfig), C.c_int32, C.c_int32, C.c_int32, dp,
                                 C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        u32p = C.POINTER(C.c_uint32)
        L.ora_primary_ray.restype = None
        L.ora_primary_ray.argtypes = [C.POINTER(OraScene), C.POINTER(OraConfig), C.c_int32, C.c_int32, C.c_int32, dp, dp]
        L.ora_sample_ray.restype = None
        L.ora_sample_ray.argtypes = [C.POINTER(OraScene), C.POINTER(OraConfig), C.c_int32, C.c_int32, C.c_int32, dp, dp, dp,
                                     u32p, u32p]
        L.ora_sample_rays.restype = None
        L.ora_sample_rays.argtypes = [C.POINTER(OraScene), C.POINTER(OraConfig), C.c_int32, C.c_int32, C.c_int32, C.c_int64,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        for name in ("ora_sin", "ora_cos", "ora_tan", "ora_exp"):
            f = getattr(L, name)
            f.restype = C.c_double
            f.argtypes = [C.c_double]
        for name in ("ora_pow", "ora_min", "ora_max"):
            f = getattr(L, name)
            f.restype = C.c_double
            f.argtypes = [C.c_double, C.c_double]
        L.ora_stream_init.restype = C.c_uint64
        L.ora_stream_init.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64]
        L.ora_stream_next.restype = C.c_double
        L.ora_stream_next.argtypes = [C.POINTER(C.c_uint64)]
        L.ora_hit.restype = C.c_int
        L.ora_hit.argtypes = [C.c_int32, dp, dp, C.c_double, dp, dp, C.c_double, C.c_double, dp]
        L.ora_convert_material.restype = None
        L.ora_convert_material.argtypes = [C.POINTER(OraMaterial), dp]
        L.ora_material_derived.restype = None
        L.ora_material_derived.argtypes = [C.POINTER(OraMaterial), dp]
        u64p, vp = C.POINTER(C.c_uint64), C.c_void_p
        L.ora_scatter_step.restype = C.c_int
        L.ora_scatter_step.argtypes = [C.POINTER(OraMaterial), dp, dp, dp, u64p, dp, u32p]
        L.ora_exit_step.restype = None
        L.ora_exit_step.argtypes = [C.POINTER(OraMaterial), dp, dp, dp, dp]
        L.ora_roulette_step.restype = C.c_int
        L.ora_roulette_step.argtypes = [C.c_int32, dp, u64p, u32p]
        L.ora_scatter_steps.restype = None
        L.ora_scatter_steps.argtypes = [C.c_int64, vp, vp, vp, vp, vp, vp, vp, vp]
        L.ora_exit_steps.restype = None
        L.ora_exit_steps.argtypes = [C.c_int64, vp, vp, vp, vp, vp, vp, vp]
        L.ora_roulette_steps.restype = None
        L.ora_roulette_steps.argtypes = [C.c_int64, vp, vp, vp, vp, vp, vp]
        L.ora_hits.restype = None
        L.ora_hits.argtypes = [C.c_int64, vp, vp, vp, vp, vp, C.c_double, C.c_double, vp, vp]
        L.ora_reflects.restype = None
        L.ora_reflects.argtypes = [C.c_int64, vp, vp, vp]
        L.ora_camera_setup.restype = None
        L.ora_camera_setup.argtypes = [C.POINTER(OraCamera), C.c_int32, C.c_int32, dp]
        L.ora_post_process.restype = None
        L.ora_post_process.argtypes = [C.POINTER(OraPostConfig), C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                       C.c_int32]
        L.ora_aces_tonemap.restype = C.c_float
        L.ora_aces_tonemap.argtypes = [C.c_float]
        L.ora_finish_pixel.restype = None
        L.ora_finish_pixel.argtypes = [dp, C.c_int32, C.POINTER(C.c_uint8)]
        _lib = L
    return _lib


# ---------------------------------------------------------------- scene JSON

_MAT_TYPES = {"lambert": 0, "metal": 1, "dielectric": 2, "emissive": 3, "mirror": 4}
_OBJ_TYPES = {"sphere": 0, "plane": 1, "box": 2, "sphere_light": 3}


def _get(d, key, default=None):
    """encoding/json matches keys case-insensitively (exact match preferred)."""
    if not isinstance(d, dict):
        return default
    if key in d:
        v = d[key]
    else:
        v = default
        for k, vv in d.items():
            if isinstance(k, str) and k.lower() == key.lower():
                v = vv
                break
    return default if v is None else v


def _num(d, key):
    return float(_get(d, key, 0.0))


def _vec(d, key, names):
    sub = _get(d, key, {})
    return [_num(sub, n) for n in names]


class Scene:
    """Owns the ctypes arrays behind an OraScene."""

    def __init__(self, doc: dict):
        self.doc = doc
        mats = _get(doc, "materials", []) or []
        objs = _get(doc, "objects", []) or []
        self._mats = (OraMaterial * max(1, len(mats)))()
        ids = {}
        for i, m in enumerate(mats):
            om = self._mats[i]
            # unknown type strings fall to convertMaterial's default branch (lambert)
            om.type = _MAT_TYPES.get(_get(m, "type", ""), 0)
            om.albedo[:] = _vec(m, "albedo", "rgb")
            om.rough = _num(m, "rough")
            om.ior = _num(m, "ior")
            om.emit[:] = _vec(m, "emit", "rgb")
            om.power = _num(m, "power")
            om.absorption[:] = _vec(m, "absorption", "rgb")
            om.smoothness = _num(m, "smoothness")
            ids[_get(m, "id", "")] = i  # map assignment: the last duplicate id wins (objects.go:227-229)
        self._objs = (OraObject * max(1, len(objs)))()
        for i, o in enumerate(objs):
            oo = self._objs[i]
            oo.type = _OBJ_TYPES.get(_get(o, "type", ""), -1)
            oo.material = ids.get(_get(o, "material_id", ""), -1)
            oo.position[:] = _vec(o, "position", "xyz")
            oo.size[:] = _vec(o, "size", "xyz")
        sc = OraScene()
        cam = _get(doc, "camera", {})
        sc.camera.position[:] = _vec(cam, "position", "xyz")
        sc.camera.target[:] = _vec(cam, "target", "xyz")
        sc.camera.up[:] = _vec(cam, "up", "xyz")
        sc.camera.fov = _num(cam, "fov")
        sc.camera.aperture = _num(cam, "aperture")
        sc.camera.focus_dist = _num(cam, "focus_dist")
        sc.camera.aspect_ratio = _num(cam, "aspect_ratio")
        sky = _get(doc, "sky", None)
        sc.sky.background[:] = _vec(doc, "background", "rgb")
        if isinstance(sky, dict):
            t = _get(sky, "type", "")
            sc.sky.sky_type = 1 if t == "gradient" else 2 if t == "solid" else 0
            sc.sky.color[:] = _vec(sky, "color", "rgb")
            sc.sky.horizon[:] = _vec(sky, "horizon", "rgb")
            sc.sky.zenith[:] = _vec(sky, "zenith", "rgb")
        else:
            sc.sky.sky_type = 0
        sc.nmaterials = len(mats)
        sc.nobjects = len(objs)
        sc.materials = C.cast(self._mats, C.POINTER(OraMaterial))
        sc.objects = C.cast(self._objs, C.POINTER(OraObject))
        self.c = sc

    @classmethod
    def load(cls, path: str) -> "Scene":
        with open(path, "r", encoding="utf-8") as f:
            return cls(json.load(f))


def render(scene: Scene, width: int, height: int, spp: int, depth: int, seed: int = 1, workers: int = 0,
           window=None, want=("rgba", "accum", "nseg", "ndraw")):
    """Returns dict(rgba uint8[H,W,4], accum f64[H,W,3], nseg u32[H,W], ndraw u32[H,W], stats)."""
    L = lib()
    cfg = OraConfig(width, height, spp, depth, seed, workers, 0)
    rgba = np.zeros((height, width, 4), np.uint8) if "rgba" in want else None
    accum = np.zeros((height, width, 3), np.float64) if "accum" in want else None
    nseg = np.zeros((height, width), np.uint32) if "nseg" in want else None
    ndraw = np.zeros((height, width), np.uint32) if "ndraw" in want else None
    st = OraStats()

    def p(a):
        return a.ctypes.data_as(C.c_void_p) if a is not None else None

    if window is None:
        L.ora_render(C.byref(scene.c), C.byref(cfg), p(rgba), width * 4, p(accum), p(nseg), p(ndraw), C.byref(st))
    else:
        x0, y0, x1, y1 = window
        L.ora_render_window(C.byref(scene.c), C.byref(cfg), x0, y0, x1, y1, p(rgba), width * 4, p(accum), p(nseg),
                            p(ndraw), C.byref(st))
    return {"rgba": rgba, "accum": accum, "nseg": nseg, "ndraw": ndraw,
            "stats": {"samples": st.samples, "segments": st.segments, "exit_scans": st.exit_scans,
                      "draws": st.draws, "seconds": st.seconds, "workers": st.workers}}


def sample(scene: Scene, width: int, height: int, spp: int, depth: int, seed: int, x: int, y: int, s: int):
    L = lib()
    cfg = OraConfig(width, height, spp, depth, seed, 1, 0)
    out = (C.c_double * 3)()
    a, b = C.c_uint32(), C.c_uint32()
    L.ora_sample(C.byref(scene.c), C.byref(cfg), x, y, s, out, C.byref(a), C.byref(b))
    return list(out), a.value, b.value


def primary_ray(scene: Scene, width: int, height: int, spp: int, depth: int, seed: int, x: int, y: int, s: int):
    """The ray sample_once traces for (x, y, s): (origin, direction) as two lists."""
    L = lib()
    cfg = OraConfig(width, height, spp, depth, seed, 1, 0)
    o, d = (C.c_double * 3)(), (C.c_double * 3)()
    L.ora_primary_ray(C.byref(scene.c), C.byref(cfg), x, y, s, o, d)
    return list(o), list(d)


def sample_ray(scene: Scene, width: int, height: int, spp: int, depth: int, seed: int, x: int, y: int, s: int, orig, dir_):
    """`sample` with the primary ray replaced by (orig, dir_) after the camera draws."""
    L = lib()
    cfg = OraConfig(width, height, spp, depth, seed, 1, 0)
    d3 = C.c_double * 3
    out = d3()
    a, b = C.c_uint32(), C.c_uint32()
    L.ora_sample_ray(C.byref(scene.c), C.byref(cfg), x, y, s, d3(*orig), d3(*dir_), out, C.byref(a), C.byref(b))
    return list(out), a.value, b.value


def sample_rays(scene: Scene, width: int, height: int, spp: int, depth: int, seed: int, rays):
    """A whole frame of chosen primary rays: rays float64 [width*height*spp, 6] (origin, direction), the ray of pixel (x, y),
    sample s at (y*width + x)*spp + s.  Returns (rgb f64 [n, 3], nseg u32 [n], ndraw u32 [n]), one row per sample."""
    L = lib()
    rays = np.ascontiguousarray(rays, dtype=np.float64)
    n = width * height * spp
    assert rays.shape == (n, 6)
    cfg = OraConfig(width, height, spp, depth, seed, 1, 0)
    rgb = np.zeros((n, 3))
    nseg = np.zeros(n, np.uint32)
    ndraw = np.zeros(n, np.uint32)
    L.ora_sample_rays(C.byref(scene.c), C.byref(cfg), 0, 0, 0, n, rays.ctypes.data, rgb.ctypes.data,
                      nseg.ctypes.data, ndraw.ctypes.data)
    return rgb, nseg, ndraw


def hit(kind: int, a, b, radius, orig, dir_, tmin, tmax):
    L = lib()
    d3 = C.c_double * 3
    out = (C.c_double * 8)()
    ok = L.ora_hit(kind, d3(*a), d3(*b), radius, d3(*orig), d3(*dir_), tmin, tmax, out)
    return bool(ok), {"t": out[0], "p": [out[1], out[2], out[3]], "n": [out[4], out[5], out[6]],
                      "front": bool(out[7])}


# ---------------------------------------------------------------- the surface step, one call or one table at a time

def material_array(mats):
    """A ctypes array of OraMaterial from OraMaterial structs (copied)."""
    arr = (OraMaterial * max(1, len(mats)))()
    for i, m in enumerate(mats):
        C.memmove(C.byref(arr[i]), C.byref(m), C.sizeof(OraMaterial))
    return arr


def scatter_step(mat, rec, orig, dir_, state: int):
    """renderer.go:308-311 on the record `hit` returned.  mat: an OraMaterial or None (the zero material).  Returns dict(ok,
    emitted, att, orig, dir, state, draws)."""
    L = lib()
    d3 = C.c_double * 3
    h = (C.c_double * 8)(rec["t"], *rec["p"], *rec["n"], float(rec["front"]))
    out = (C.c_double * 12)()
    st, nd = C.c_uint64(state), C.c_uint32()
    ok = L.ora_scatter_step(C.byref(mat) if mat is not None else None, h, d3(*orig), d3(*dir_), C.byref(st), out, C.byref(nd))
    return {"ok": bool(ok), "emitted": list(out[0:3]), "att": list(out[3:6]), "orig": list(out[6:9]), "dir": list(out[9:12]),
            "state": st.value, "draws": nd.value}


def exit_step(mat, entry, exit_p, att, orig):
    """renderer.go:352-370; exit_p None = no exit found.  Returns (att, orig) afterwards."""
    L = lib()
    d3 = C.c_double * 3
    a, o = d3(*att), d3(*orig)
    L.ora_exit_step(C.byref(mat) if mat is not None else None, d3(*entry), d3(*exit_p) if exit_p is not None else None, a, o)
    return list(a), list(o)


def roulette_step(depth: int, att, state: int):
    """renderer.go:375-393.  Returns (ended 0 / 1 / 2, att afterwards, state afterwards, draws)."""
    L = lib()
    a = (C.c_double * 3)(*att)
    st, nd = C.c_uint64(state), C.c_uint32()
    e = L.ora_roulette_step(depth, a, C.byref(st), C.byref(nd))
    return e, list(a), st.value, nd.value


def hits(kind, a, b, radius, rays, tmin, tmax):
    """n cases of `hit`, one object each.  Returns (ok i32 [n], out f64 [n, 8] = t, p, normal, frontFace)."""
    L = lib()
    kind = np.ascontiguousarray(kind, np.int32)
    a, b, radius, rays = (np.ascontiguousarray(x, np.float64) for x in (a, b, radius, rays))
    n = len(kind)
    assert a.shape == (n, 3) and b.shape == (n, 3) and radius.shape == (n,) and rays.shape == (n, 6)
    out, ok = np.zeros((n, 8)), np.zeros(n, np.int32)
    L.ora_hits(n, kind.ctypes.data, a.ctypes.data, b.ctypes.data, radius.ctypes.data, rays.ctypes.data, tmin, tmax, out.ctypes.data,
               ok.ctypes.data)
    return ok, out


def reflects(v, nrm):
    """reflectVec on n pairs: f64 [n, 3]."""
    L = lib()
    v, nrm = np.ascontiguousarray(v, np.float64), np.ascontiguousarray(nrm, np.float64)
    assert v.shape == nrm.shape and v.shape[1:] == (3,)
    out = np.zeros_like(v)
    L.ora_reflects(len(v), v.ctypes.data, nrm.ctypes.data, out.ctypes.data)
    return out


def scatter_steps(mats, mat, hits, rays, states):
    """n cases of scatter_step: mats a material_array, mat int32 [n] (-1: the zero material), hits f64 [n, 8], rays f64 [n, 6],
    states u64 [n].  Returns dict(ok i32 [n], out f64 [n, 12] = emitted, att, orig, dir; state u64 [n]; draws u32 [n])."""
    L = lib()
    mat = np.ascontiguousarray(mat, np.int32)
    hits = np.ascontiguousarray(hits, np.float64)
    rays = np.ascontiguousarray(rays, np.float64)
    st = np.array(states, np.uint64)
    n = len(mat)
    assert hits.shape == (n, 8) and rays.shape == (n, 6) and st.shape == (n,)
    out, ok, nd = np.zeros((n, 12)), np.zeros(n, np.int32), np.zeros(n, np.uint32)
    L.ora_scatter_steps(n, C.addressof(mats), mat.ctypes.data, hits.ctypes.data, rays.ctypes.data, st.ctypes.data, out.ctypes.data,
                        ok.ctypes.data, nd.ctypes.data)
    return {"ok": ok, "out": out, "state": st, "draws": nd}


def exit_steps(mats, mat, rays, t, best, att):
    """n cases of exit_step on the scattered rays f64 [n, 6], the exit hit (t f64 [n], best i32 [n], < 0: none) and att f64 [n, 3].
    Returns (att, orig) afterwards, f64 [n, 3] each."""
    L = lib()
    mat = np.ascontiguousarray(mat, np.int32)
    rays = np.ascontiguousarray(rays, np.float64)
    t = np.ascontiguousarray(t, np.float64)
    best = np.ascontiguousarray(best, np.int32)
    a = np.array(att, np.float64)
    n = len(mat)
    assert rays.shape == (n, 6) and t.shape == (n,) and best.shape == (n,) and a.shape == (n, 3)
    o = np.zeros((n, 3))
    L.ora_exit_steps(n, C.addressof(mats), mat.ctypes.data, rays.ctypes.data, t.ctypes.data, best.ctypes.data, a.ctypes.data, o.ctypes.data)
    return a, o


def roulette_steps(depth, att, T, states):
    """n cases of roulette_step and the step to the next level.  Returns dict(ended i32 [n]: 0 goes on, 1 maxAtt < 1e-6, 2 the
    draw, 3 depth reached 0; att, T f64 [n, 3]; state u64 [n]; draws u32 [n])."""
    L = lib()
    depth = np.ascontiguousarray(depth, np.int32)
    a, tt, st = np.array(att, np.float64), np.array(T, np.float64), np.array(states, np.uint64)
    n = len(depth)
    assert a.shape == (n, 3) and tt.shape == (n, 3) and st.shape == (n,)
    e, nd = np.zeros(n, np.int32), np.zeros(n, np.uint32)
    L.ora_roulette_steps(n, depth.ctypes.data, a.ctypes.data, tt.ctypes.data, st.ctypes.data, e.ctypes.data, nd.ctypes.data)
    return {"ended": e, "att": a, "T": tt, "state": st, "draws": nd}


def post_process(img, tonemap=False, denoise=False, sigma_s=1.0, sigma_r=0.15, smooth=False, smooth_radius=2,
                 smooth_strength=0.5, accum=None, spp=1):
    """In-place CPU restatement of the reference GPU backend's post passes on img (uint8 [H, W, 4])."""
    L = lib()
    cfg = OraPostConfig(int(tonemap), int(denoise), sigma_s, sigma_r, int(smooth), smooth_radius, smooth_strength)
    h, w = img.shape[0], img.shape[1]
    L.ora_post_process(C.byref(cfg), accum.ctypes.data_as(C.c_void_p) if accum is not None else None, spp,
                       img.ctypes.data_as(C.c_void_p), int(img.strides[0]), w, h)
