"""Helpers of the GL feature tests (test_gl_features_cpu.py, test_gl_features_gpu.py; pt_set_shading_features).

  * reference(): tests/gl_features_reference.c (with glshade_reference.c inside) linked against the oracle; ref_features(case, ...)
    gives glf_features' planes and ids, computed once per (case, passes, k); ref_classes(...) what the first hits were.
  * shim(): a host build of csrc/pt_gl_features.h.  It is glwalk_support's shim -- the product's GL tables, trees and bounds as
    frame_open builds them -- with one more entry point, so the features run over the loop (ptg::LinearWorld) or over the tree
    (ptg::TreeWorld) on exactly the tables the walk tests use.
  * the cases: the five shipped scenes, scenes of fuzz_support.py (host_fuzz_case, trimmed below the BVH path for the GPU), and
    glwalk_support's room.  A case is glwalk_support's dict: name, doc, sc, ora, cfg = (w, h, passes, depth, seed).
"""
from __future__ import annotations

import ctypes as C
import json
import os
import subprocess

import numpy as np

import glshade_support as gs
import glwalk_support as gw
from fog_support import CFLAGS, CSRC, CXXFLAGS, ORACLE, ROOT, ptr
from fuzz_support import host_fuzz_case, trim_to_limits

SHIPPED = ("example_simple", "gpu_showcase", "metal_glass_room", "test_comprehensive", "test_scene")
W, H, PASSES, DEPTH, SEED = 40, 24, 3, 3, 1  # two tiles wide, ragged right and bottom edges, out-of-frame lanes
KS = (1, 2, 5)
N_FUZZ = 32
FUZZ_W, FUZZ_H = 24, 16

EXTRA = r"""
#include "pt_gl_features.h"
extern "C" {
// The planes ([H][W][3] each) and ids of a frame of `passes` passes with k feature passes, by ptg::feature_pass over the loop
// (tree = 0) or over the tree (tree = 1); wc [7]: the tree policy's counters.
void gf_features(void *h, int32_t passes, int32_t k, uint64_t seed, int32_t tree, double *fn, double *fa, double *fd, int32_t *ids, uint64_t *wc) {
    Walk *K = static_cast<Walk *>(h);
    const uint64_t key = ptm::seed_key(seed ^ PTG_STREAM_SALT);
    const int32_t take = k < passes ? k : passes;
    int stack[PT_BVH_STACK];
    for (int32_t y = 0; y < K->S.height; y++)
        for (int32_t x = 0; x < K->S.width; x++) {
            const size_t i = (size_t)y * (size_t)K->S.width + (size_t)x;
            double f[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            int32_t id = -1;
            for (int32_t p = 0; p < take; p++) {
                int32_t pid = -1;
                if (tree) {
                    ptg::WalkCount w = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
                    const ptg::TreeWorld world{K->objs.data(), K->S.nobj, K->F, K->T.nodes.data(), K->T.objs.data(), K->plane_idx.data(), stack, 1, w};
                    ptg::feature_pass(K->S, world, key, x, y, (uint32_t)p, f, &pid);
                    add(wc, w);
                } else {
                    ptg::feature_pass(K->S, key, x, y, (uint32_t)p, f, &pid);
                }
                if (p == 0) id = pid;
            }
            for (int q = 0; q < 3; q++) { fn[3 * i + q] = f[q]; fa[3 * i + q] = f[3 + q]; fd[3 * i + q] = f[6 + q]; }
            ids[i] = id;
        }
}
}
"""

_libs = {}
_refs = {}
_cases = {}


def reference():
    """gl_features_reference.c linked against oracle/libptoracle.so."""
    if "ref" not in _libs:
        from oracle import ora

        ora.lib()
        out = os.path.join(gs._build_dir(), "libglfeatref.so")
        r = subprocess.run(["gcc", *CFLAGS, "-Wall", "-Wextra", "-Wno-unused-function", "-shared", "-I", ORACLE, "-I", os.path.join(ROOT, "tests"),
                            os.path.join(ROOT, "tests", "gl_features_reference.c"), "-o", out, "-L", ORACLE, "-Wl,-rpath," + ORACLE,
                            "-lptoracle", "-lm"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        L = C.CDLL(out)
        vp = C.c_void_p
        L.glf_features.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, vp, vp, vp, vp]
        L.glf_classes.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, vp]
        L.gr_render.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, vp, vp, vp, vp]
        _libs["ref"] = L
    return _libs["ref"]


def shim():
    """csrc/pt_gl_features.h built for the host with g++, beside glwalk_support's shim of the tables and trees."""
    if "shim" not in _libs:
        d = gs._build_dir()
        src = os.path.join(d, "glfeat_shim.cpp")
        with open(src, "w") as f:
            f.write(gw.SHIM + EXTRA)
        out = os.path.join(d, "libglfeatshim.so")
        r = subprocess.run(["g++", *CXXFLAGS, "-Wall", "-Wextra", "-shared", "-I", CSRC, src, "-o", out], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        L = C.CDLL(out)
        vp = C.c_void_p
        L.gw_open.restype = vp
        L.gw_open.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int32]
        L.gw_close.argtypes = [vp]
        L.gw_info.argtypes = [vp, vp, vp]
        L.gf_features.argtypes = [vp, C.c_int32, C.c_int32, C.c_uint64, C.c_int32, vp, vp, vp, vp, vp]
        _libs["shim"] = L
    return _libs["shim"]


def _planes(w, h):
    return [np.zeros((h, w, 3)) for _ in range(3)], np.full((h, w), -9, np.int32)


def ref_features(case, passes=None, k=1):
    """(fn, fa, fd, ids) of glf_features for the case's frame with `passes` passes done; read-only, computed once."""
    w, h, p, _, seed = case["cfg"]
    p = p if passes is None else passes
    key = (case["name"], w, h, p, k, seed)
    if key not in _refs:
        (fn, fa, fd), ids = _planes(w, h)
        reference().glf_features(C.byref(case["ora"].c), C.cast(gs.extras(case["sc"]), C.c_void_p), w, h, p, k, seed, ptr(fn), ptr(fa), ptr(fd), ptr(ids))
        for a in (fn, fa, fd, ids):
            a.setflags(write=False)
        _refs[key] = (fn, fa, fd, ids)
    return _refs[key]


CLASSES = ("paths", "sphere", "plane", "box", "back_face", "miss")


def ref_classes(case, passes=None, k=1):
    """What the first hits of that frame's feature paths were (from the reference alone)."""
    w, h, p, _, seed = case["cfg"]
    out = np.zeros(6, np.uint64)
    reference().glf_classes(C.byref(case["ora"].c), C.cast(gs.extras(case["sc"]), C.c_void_p), w, h, p if passes is None else passes, k, seed, ptr(out))
    return dict(zip(CLASSES, (int(v) for v in out)))


def host_features(case, passes=None, k=1, tree=False):
    """(fn, fa, fd, ids, walk counters, tree built) of the host build of pt_gl_features.h."""
    from path_trace_golang_amd import hip

    w, h, p, depth, seed = case["cfg"]
    L = shim()
    flat, ex = hip.FlatScene(case["sc"]), gs.extras(case["sc"])
    hd = L.gw_open(C.byref(flat.c), C.cast(ex, C.c_void_p), w, h, depth)
    try:
        info = np.zeros(6, np.int32)
        L.gw_info(hd, ptr(info), ptr(np.zeros(4)))
        (fn, fa, fd), ids = _planes(w, h)
        wc = np.zeros(7, np.uint64)
        assert not tree or info[0], "no tree was built for this scene"
        L.gf_features(hd, p if passes is None else passes, k, seed, 1 if tree else 0, ptr(fn), ptr(fa), ptr(fd), ptr(ids), ptr(wc))
    finally:
        L.gw_close(hd)
    return fn, fa, fd, ids, dict(zip(gw.WALK_COUNTERS, (int(v) for v in wc))), bool(info[0])


def same_planes(a, b):
    """Bit equality of (fn, fa, fd, ids) tuples (the first four entries)."""
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64)) for x, y in zip(a[:3], b[:3])) \
        and np.array_equal(a[3], b[3])


# ---------------------------------------------------------------- cases
def shipped_case(name, w=W, h=H, passes=PASSES, depth=DEPTH, seed=SEED):
    key = ("shipped", name, w, h, passes, depth, seed)
    if key not in _cases:
        with open(os.path.join(ROOT, "scenes", name + ".json")) as f:
            doc = json.load(f)
        c = gw._case(name, doc, (w, h, passes, depth, seed))
        c["name"] = "%s@%dx%dx%d-d%d-s%d" % (name, w, h, passes, depth, seed)
        _cases[key] = c
    return _cases[key]


def fuzz_case(i, w=FUZZ_W, h=FUZZ_H, passes=2, gpu=False):
    """Scene i of fuzz_support.host_fuzz_case (1 .. 150 random objects, GL extras, a light count from its table) without its fog
    block; gpu=True trims it below the BVH path (128 of a kind), where gl_trace_kernel renders it."""
    key = ("fuzz", i, w, h, passes, gpu)
    if key not in _cases:
        doc = host_fuzz_case(i)["doc"]
        doc.pop("fog", None)
        if gpu:
            trim_to_limits(doc)
        c = gw._case("glf-fuzz%d%s" % (i, "g" if gpu else ""), doc, (w, h, passes, DEPTH, 300 + i))
        c["name"] += "@%dx%dx%d" % (w, h, passes)
        _cases[key] = c
    return _cases[key]


def room_case(passes=PASSES):
    """glwalk_support's room (341 objects: on the BVH path) at its own 33 x 20."""
    return gw.with_cfg(gw.room_case(), passes=passes, depth=DEPTH, seed=SEED)


def back_face_case():
    """A camera inside a large lambert sphere, looking at a box through a glass ball: every ray that reaches the shell hits its inside."""
    def make():
        V, RGB = gw.V, gw.RGB
        mats = [{"id": "shell", "type": "lambert", "albedo": RGB(0.5, 0.55, 0.6)}, {"id": "red", "type": "lambert", "albedo": RGB(0.8, 0.2, 0.2)},
                {"id": "lamp", "type": "emissive", "albedo": RGB(0.2, 0.3, 0.4), "emit": RGB(1, 0.9, 0.7), "power": 6.0}]
        objs = [{"id": "shell", "type": "sphere", "position": V(0, 0, 0), "size": V(30, 0, 0), "material_id": "shell"},
                {"id": "cube", "type": "box", "position": V(0, 1, 0), "size": V(1.5, 1.5, 1.5), "material_id": "red"},
                {"id": "lamp", "type": "sphere_light", "position": V(2, 4, 1), "size": V(0.5, 0, 0), "material_id": "lamp"}]
        doc = {"name": "glf-inside", "camera": {"position": V(0, 2, 8), "target": V(0, 1, 0), "up": V(0, 1, 0), "fov": 60},
               "materials": mats, "objects": objs, "background": RGB(0.1, 0.1, 0.1)}
        return gw._case("glf-inside", doc, (W, H, PASSES, DEPTH, SEED))
    key = ("inside",)
    if key not in _cases:
        _cases[key] = make()
    return _cases[key]


# ---------------------------------------------------------------- the GPU side
def gl_reference(case, passes=None):
    """(rgba, accum, stats) of gr_render for the case with `passes` passes, computed once."""
    return gw.reference(case if passes is None else gw.with_cfg(case, passes=passes))


def read_planes(ctx, w, h, ids=True):
    """(fn, fa, fd, ids) of ctx's open or last frame (ids None when not asked for)."""
    from path_trace_golang_amd import hip

    (fn, fa, fd), idp = _planes(w, h)
    for a in (fn, fa, fd):
        a.fill(-7.0)
    hip.read_features(ctx, fn, fa, fd)
    if ids:
        hip.read_object_ids(ctx, idp)
    return fn, fa, fd, (idp if ids else None)


def tonemapped(mean):
    """ora_post_process(tonemap = 1) of a mean at spp 1: GL's finish as the oracle states it."""
    from oracle import ora

    h, w = mean.shape[:2]
    img = np.zeros((h, w, 4), np.uint8)
    ora.post_process(img, tonemap=True, accum=np.ascontiguousarray(mean, np.float64), spp=1)
    return img


# ---------------------------------------------------------------- quality, on the CPU
def quality(name, w=80, h=48, passes=4, ref_passes=512, depth=8, k=1, **cfg):
    """What the default filter does to a GL frame of a shipped scene, through the host builds alone: the frame's pass sums from
    glshade_reference.c (S = their sum, Q = the sum of their squares, in pass order), the features of pt_gl_features.h's host build,
    the filter of pt_atrous.h's host build, against a `ref_passes`-pass frame of gr_render with another seed.  Returns the relative
    MSE (atrous_support.relative_mse) of the unfiltered and of the filtered mean, their ratio and the two noise figures."""
    import atrous_support as at

    case = shipped_case(name, w, h, passes, depth, SEED)
    jobs = np.array([(x, y, p) for y in range(h) for x in range(w) for p in range(passes)], np.int32)
    out, _ = gs.ref_passes(case["ora"], gs.extras(case["sc"]), w, h, depth, SEED, jobs)
    per = out.reshape(h, w, passes, 3)
    S, Q = np.zeros((h, w, 3)), np.zeros((h, w, 3))
    for p in range(passes):
        S = S + per[:, :, p]
        Q = Q + per[:, :, p] * per[:, :, p]
    feats = host_features(case, k=k)[:3]
    run = at.host_filter(S, Q, passes, None, feats, **cfg)
    truth = gs.reference_render(case["ora"], gs.extras(case["sc"]), w, h, ref_passes, depth, SEED + 7)[1] / float(ref_passes)
    before, after = at.relative_mse(S / float(passes), truth), at.relative_mse(run["mean"], truth)
    return dict(scene=name, width=w, height=h, passes=passes, ref_passes=ref_passes, depth=depth, k=k, rel_mse_unfiltered=before,
                rel_mse_filtered=after, ratio=after / before, noise_before=run["noise_before"], noise_after=run["noise_after"],
                bad_pixels=run["bad_pixels"])
