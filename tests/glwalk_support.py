"""The scenes of the GL walk tests (test_glshade_walk_cpu.py, test_glshade_walk_gpu.py) and a host build of csrc/pt_gl_walk.h.

A case is a dict: name, doc (the scene file's document), sc (the product's Scene), ora (the oracle's), cfg = (w, h, passes, depth,
seed).  reference(case) renders it with tests/glshade_reference.c (glshade_support.reference_render: a loop over all objects) once
per process.

The shim builds the product's own tables -- gl_material / gl_object / gl_is_light as frame_open calls them, ptd::scene_to_world,
ptbvh::build_scene_trees, ptbvh::world_bound / frame_bounds for origin_bound, dir_floor and clip_bound -- and exposes pass sums
with the tree policy (ptg::TreeWorld), the queries a pass makes (a recording policy around ptg::LinearWorld), single closest /
occluded queries with both policies, the walk's counters and ptg::walk_scene_check.

Every scene that must keep both "sent to the plain loop" counters at zero is closed by a large sphere around the origin (DOME):
the planes are infinite, a ray that grazes one is hit hundreds of units out, beyond clip_bound = 3.5 scene sizes, and its next
segment would take the plain loop.  Inside the dome every hit point, hence every later origin, lies within the scene bound."""
from __future__ import annotations

import copy
import ctypes as C
import json
import os
import subprocess

import numpy as np

import glshade_support as gs
from fog_support import CSRC, CXXFLAGS, ptr
from fuzz_support import count_kinds, random_doc, random_gl_extras, set_lights
from ray_inject_support import scene_bound

V = lambda x, y, z: {"x": float(x), "y": float(y), "z": float(z)}  # noqa: E731
RGB = lambda r, g, b: {"r": float(r), "g": float(g), "b": float(b)}  # noqa: E731
DOME_RADIUS = 60.0
LINEAR_COUNTS = (1000, 800, 600, 400, 300)
FUZZ_COUNTS = (300, 450, 700)
FUZZ_LIGHTS = (0, 1, 8, 9, 12)
FUZZ_FRAMES = ((33, 20), (20, 33))
N_FUZZ = 8
WALK_COUNTERS = ("closest_walked", "closest_plain", "shadow_walked", "shadow_plain", "closest_visits", "shadow_visits", "deepest_stack")

SHIM = r"""
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>
#include "pt_bvh.h"
#include "pt_convert.h"
#include "pt_glshade.h"
#include "pt_gl_walk.h"

namespace {
struct Walk {
    std::vector<pt_object> raw;
    std::vector<ptg::GlMat> mats;
    std::vector<ptg::GlObj> objs;
    std::vector<int32_t> lights, plane_idx;
    std::vector<ptd::DevObj> world;
    std::vector<ptd::DevMat> dmats;
    ptbvh::SceneTrees T;
    ptd::DevFrame F;
    ptg::GlScene S;
    bool built = false;
};
// the queries of a pass, as the model asks them: kind (0 closest, 1 occluded), ro, rd, tmin, tmax, skip
struct RecordingWorld {
    ptg::LinearWorld lin;
    std::vector<double> *q;
    int32_t closest(const double ro[3], const double rd[3], double tmin, double tmax_start, int32_t skip, double &t_hit) const {
        const double r[11] = {0, ro[0], ro[1], ro[2], rd[0], rd[1], rd[2], tmin, tmax_start, (double)skip, 0};
        q->insert(q->end(), r, r + 11);
        return lin.closest(ro, rd, tmin, tmax_start, skip, t_hit);
    }
    bool occluded(const double ro[3], const double rd[3], double tmax) const {
        const double r[11] = {1, ro[0], ro[1], ro[2], rd[0], rd[1], rd[2], 0.001, tmax, -1, 0};
        q->insert(q->end(), r, r + 11);
        return lin.occluded(ro, rd, tmax);
    }
};
void add(uint64_t *out, const ptg::WalkCount &c) {
    const uint32_t v[6] = {c.closest_walked, c.closest_plain, c.shadow_walked, c.shadow_plain, c.closest_visits, c.shadow_visits};
    for (int k = 0; k < 6; k++) out[k] += v[k];
    if (c.deepest > out[6]) out[6] = c.deepest;
}
}  // namespace

extern "C" {
void *gw_open(const pt_scene *sc, const pt_gl_material *ex, int32_t w, int32_t h, int32_t depth) {
    Walk *K = new Walk;
    const int32_t nmat = sc->num_materials;
    K->raw.assign(sc->objects, sc->objects + sc->num_objects);
    K->mats.assign((size_t)(nmat > 0 ? nmat : 1), ptg::GlMat{});
    for (int32_t i = 0; i < nmat; i++) K->mats[(size_t)i] = ptg::gl_material(sc->materials[i], ex[i]);
    for (int32_t i = 0; i < sc->num_objects; i++) {
        K->objs.push_back(ptg::gl_object(sc->objects[i], nmat));
        if (ptg::gl_is_light(*sc, i)) K->lights.push_back(i);
    }
    ptd::scene_to_world(*sc, K->world, K->dmats);
    for (size_t i = 0; i < K->world.size(); i++)
        if ((K->world[i].kind & 0xff) == ptd::KIND_PLANE) K->plane_idx.push_back((int32_t)i);
    K->built = ptbvh::build_scene_trees(K->world, false, PT_BVH_STACK, K->T);
    std::memset(&K->F, 0, sizeof K->F);
    ptbvh::frame_bounds(ptbvh::world_bound(K->world), K->F);
    K->F.n_plane = (int32_t)K->plane_idx.size();
    K->F.bvh_root = K->built ? K->T.root : -1;
    K->F.bvh_stack = PT_BVH_STACK;
    K->F.nobj = (int32_t)K->world.size();
    ptg::GlScene &S = K->S;
    S = ptg::GlScene{};
    S.objs = K->objs.data(); S.mats = K->mats.data(); S.lights = K->lights.data();
    S.nobj = (int32_t)K->objs.size(); S.nlight = (int32_t)K->lights.size();
    S.sky = ptg::gl_sky(sc->sky);
    S.cam = ptg::gl_camera(sc->camera, w, h);
    S.max_depth = depth; S.width = w; S.height = h;
    return K;
}
void gw_close(void *h) { delete static_cast<Walk *>(h); }
// {built, nodes of the main tree, records of the main tree, stack_need, planes, world objects}; bounds = {origin_bound, dir_floor, clip_bound, margin}
void gw_info(void *h, int32_t out[6], double bounds[4]) {
    Walk *K = static_cast<Walk *>(h);
    const int32_t v[6] = {K->built ? 1 : 0, K->T.main_nodes, K->T.main_objs, K->T.stack_need, K->F.n_plane, K->F.nobj};
    for (int k = 0; k < 6; k++) out[k] = v[k];
    bounds[0] = K->F.origin_bound; bounds[1] = K->F.dir_floor; bounds[2] = K->F.clip_bound; bounds[3] = K->F.margin;
}
int32_t gw_check(void *h, char *why, int32_t cap) {
    Walk *K = static_cast<Walk *>(h);
    std::string w;
    const bool ok = ptg::walk_scene_check(K->raw.data(), (int32_t)K->raw.size(), K->objs.data(), K->T.nodes.data(), K->T.main_nodes, K->T.objs.data(),
                                          K->T.main_objs, K->plane_idx.data(), (int32_t)K->plane_idx.size(), w);
    std::strncpy(why, w.c_str(), (size_t)cap - 1);
    why[cap - 1] = 0;
    return ok ? 1 : 0;
}
// pass sums with the tree policy: out [n][3], cnt [n][5] (paths, segments, shadow rays, probe rays, draws), wc [7] summed (the last: max)
void gw_pass_many(void *h, uint64_t seed, int64_t n, const int32_t *jobs, double *out, uint64_t *cnt, uint64_t *wc) {
    Walk *K = static_cast<Walk *>(h);
    const uint64_t key = ptm::seed_key(seed ^ PTG_STREAM_SALT), fkey = ptm::seed_key(seed ^ PTF_STREAM_SALT);
    int stack[PT_BVH_STACK];
    for (int64_t i = 0; i < n; i++) {
        ptg::GlCount c = {0u, 0u, 0u, 0u, 0u};
        ptg::WalkCount w = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
        ptf::FogCount f = {0u, 0u, 0u};
        const ptg::TreeWorld world{K->objs.data(), K->S.nobj, K->F, K->T.nodes.data(), K->T.objs.data(), K->plane_idx.data(), stack, 1, w};
        ptg::gl_pass(K->S, world, key, fkey, jobs[3 * i], jobs[3 * i + 1], (uint32_t)jobs[3 * i + 2], c, f, out + 3 * i);
        const uint64_t v[5] = {c.paths, c.segments, c.shadow_rays, c.probe_rays, c.draws};
        for (int k = 0; k < 5; k++) cnt[5 * i + k] = v[k];
        add(wc, w);
    }
}
// the queries of those passes with the loop over all objects: returns their number; q (when not null) receives [count][11]; out / cnt as above
int64_t gw_record(void *h, uint64_t seed, int64_t n, const int32_t *jobs, double *q, int64_t cap, double *out, uint64_t *cnt) {
    Walk *K = static_cast<Walk *>(h);
    const uint64_t key = ptm::seed_key(seed ^ PTG_STREAM_SALT), fkey = ptm::seed_key(seed ^ PTF_STREAM_SALT);
    std::vector<double> rec;
    const RecordingWorld world{ptg::LinearWorld{K->objs.data(), K->S.nobj}, &rec};
    for (int64_t i = 0; i < n; i++) {
        ptg::GlCount c = {0u, 0u, 0u, 0u, 0u};
        ptf::FogCount f = {0u, 0u, 0u};
        ptg::gl_pass(K->S, world, key, fkey, jobs[3 * i], jobs[3 * i + 1], (uint32_t)jobs[3 * i + 2], c, f, out + 3 * i);
        const uint64_t v[5] = {c.paths, c.segments, c.shadow_rays, c.probe_rays, c.draws};
        for (int k = 0; k < 5; k++) cnt[5 * i + k] = v[k];
    }
    const int64_t m = (int64_t)(rec.size() / 11);
    if (q && m <= cap) std::memcpy(q, rec.data(), rec.size() * sizeof(double));
    return m;
}
// queries q [n][11] with both policies: idx [n][2] (loop, tree; occluded: 0 / 1), t [n][2]; wc [7] of the tree policy
void gw_queries(void *h, int64_t n, const double *q, int32_t *idx, double *t, uint64_t *wc) {
    Walk *K = static_cast<Walk *>(h);
    int stack[PT_BVH_STACK];
    const ptg::LinearWorld lin{K->objs.data(), K->S.nobj};
    for (int64_t i = 0; i < n; i++) {
        const double *r = q + 11 * i;
        ptg::WalkCount w = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
        const ptg::TreeWorld tree{K->objs.data(), K->S.nobj, K->F, K->T.nodes.data(), K->T.objs.data(), K->plane_idx.data(), stack, 1, w};
        if (r[0] == 0) {
            idx[2 * i] = lin.closest(r + 1, r + 4, r[7], r[8], (int32_t)r[9], t[2 * i]);
            idx[2 * i + 1] = tree.closest(r + 1, r + 4, r[7], r[8], (int32_t)r[9], t[2 * i + 1]);
        } else {
            idx[2 * i] = lin.occluded(r + 1, r + 4, r[8]) ? 1 : 0;
            idx[2 * i + 1] = tree.occluded(r + 1, r + 4, r[8]) ? 1 : 0;
            t[2 * i] = t[2 * i + 1] = 0.0;
        }
        add(wc, w);
    }
}
// closest queries whose winning t is shared: out = {two spheres, two boxes, a sphere and a box, two planes} (queries counted once per kind)
void gw_tie_census(void *h, int64_t n, const double *q, int64_t out[4]) {
    Walk *K = static_cast<Walk *>(h);
    const ptg::LinearWorld lin{K->objs.data(), K->S.nobj};
    for (int64_t i = 0; i < n; i++) {
        const double *r = q + 11 * i;
        if (r[0] != 0) continue;
        double tw;
        if (lin.closest(r + 1, r + 4, r[7], r[8], (int32_t)r[9], tw) < 0) continue;
        int kinds[3] = {0, 0, 0};
        for (int32_t j = 0; j < K->S.nobj; j++) {
            double t;
            if (j != (int32_t)r[9] && ptg::hit_t(K->objs[(size_t)j], r + 1, r + 4, r[7], r[8], t) && t == tw) kinds[K->objs[(size_t)j].type]++;
        }
        if (kinds[ptg::GT_SPHERE] >= 2) out[0]++;
        if (kinds[ptg::GT_BOX] >= 2) out[1]++;
        if (kinds[ptg::GT_SPHERE] >= 1 && kinds[ptg::GT_BOX] >= 1) out[2]++;
        if (kinds[ptg::GT_PLANE] >= 2) out[3]++;
    }
}
}
"""

_lib = None
_cases = {}
_refs = {}


def shim():
    """csrc/pt_gl_walk.h (with pt_glshade.h, pt_bvh.h, pt_convert.h) built for the host with g++."""
    global _lib
    if _lib is None:
        d = gs._build_dir()
        src = os.path.join(d, "glwalk_shim.cpp")
        with open(src, "w") as f:
            f.write(SHIM)
        out = os.path.join(d, "libglwalkshim.so")
        r = subprocess.run(["g++", *CXXFLAGS, "-Wall", "-Wextra", "-shared", "-I", CSRC, src, "-o", out], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        L = C.CDLL(out)
        vp = C.c_void_p
        L.gw_open.restype = vp
        L.gw_open.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int32]
        L.gw_close.argtypes = [vp]
        L.gw_info.argtypes = [vp, vp, vp]
        L.gw_check.restype = C.c_int32
        L.gw_check.argtypes = [vp, C.c_char_p, C.c_int32]
        L.gw_pass_many.argtypes = [vp, C.c_uint64, C.c_int64, vp, vp, vp, vp]
        L.gw_record.restype = C.c_int64
        L.gw_record.argtypes = [vp, C.c_uint64, C.c_int64, vp, vp, C.c_int64, vp, vp]
        L.gw_queries.argtypes = [vp, C.c_int64, vp, vp, vp, vp]
        L.gw_tie_census.argtypes = [vp, C.c_int64, vp, vp]
        _lib = L
    return _lib


class Host:
    """The product's tables and trees of a case on the host (w, h, depth: the camera and the model's depth)."""

    def __init__(self, case, depth=None):
        from path_trace_golang_amd import hip

        w, h, _, d, _ = case["cfg"]
        self.case = case
        self.flat = hip.FlatScene(case["sc"])
        self.ex = gs.extras(case["sc"])
        self.h = shim().gw_open(C.byref(self.flat.c), C.cast(self.ex, C.c_void_p), w, h, d if depth is None else depth)

    def close(self):
        if self.h:
            shim().gw_close(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def info(self):
        out = np.zeros(6, np.int32)
        b = np.zeros(4)
        shim().gw_info(self.h, ptr(out), ptr(b))
        return dict(zip(("built", "main_nodes", "main_objs", "stack_need", "planes", "world"), (int(v) for v in out))), \
            dict(zip(("origin_bound", "dir_floor", "clip_bound", "margin"), (float(v) for v in b)))

    def check(self):
        buf = C.create_string_buffer(512)
        ok = shim().gw_check(self.h, buf, 512)
        return bool(ok), buf.value.decode()

    def passes(self, seed, jobs):
        """(radiance [n,3], counters [n,5], walk counters dict) of the tree policy."""
        jobs = np.ascontiguousarray(jobs, np.int32)
        n = jobs.shape[0]
        out, cnt, wc = np.zeros((n, 3)), np.zeros((n, 5), np.uint64), np.zeros(7, np.uint64)
        shim().gw_pass_many(self.h, seed, n, ptr(jobs), ptr(out), ptr(cnt), ptr(wc))
        return out, cnt, dict(zip(WALK_COUNTERS, (int(v) for v in wc)))

    def record(self, seed, jobs):
        """(queries [m,11], radiance [n,3], counters [n,5]) of the loop over all objects."""
        jobs = np.ascontiguousarray(jobs, np.int32)
        n = jobs.shape[0]
        out, cnt = np.zeros((n, 3)), np.zeros((n, 5), np.uint64)
        m = shim().gw_record(self.h, seed, n, ptr(jobs), None, 0, ptr(out), ptr(cnt))
        q = np.zeros((max(m, 1), 11))
        assert shim().gw_record(self.h, seed, n, ptr(jobs), ptr(q), m, ptr(out), ptr(cnt)) == m
        return q[:m], out, cnt

    def queries(self, q):
        """(idx [n,2], t [n,2], walk counters): column 0 the loop, column 1 the tree policy."""
        q = np.ascontiguousarray(q, np.float64)
        n = q.shape[0]
        idx, t, wc = np.zeros((n, 2), np.int32), np.zeros((n, 2)), np.zeros(7, np.uint64)
        shim().gw_queries(self.h, n, ptr(q), ptr(idx), ptr(t), ptr(wc))
        return idx, t, dict(zip(WALK_COUNTERS, (int(v) for v in wc)))

    def tie_census(self, q):
        q = np.ascontiguousarray(q, np.float64)
        out = np.zeros(4, np.int64)
        shim().gw_tie_census(self.h, q.shape[0], ptr(q), ptr(out))
        return dict(zip(("sphere_sphere", "box_box", "sphere_box", "plane_plane"), (int(v) for v in out)))


def closest_query(ro, rd, tmin=0.001, tmax=1e20, skip=-1):
    return [0.0, *ro, *rd, tmin, tmax, float(skip), 0.0]


def shadow_query(ro, rd, tmax):
    return [1.0, *ro, *rd, 0.001, tmax, -1.0, 0.0]


# ---------------------------------------------------------------- cases
def _case(name, doc, cfg):
    from oracle import ora
    from path_trace_golang_amd import scene

    doc = json.loads(json.dumps(doc))
    return {"name": name, "doc": doc, "sc": scene.Scene.decode(doc), "ora": ora.Scene(doc), "cfg": tuple(cfg)}


def _cached(name, make):
    if name not in _cases:
        _cases[name] = make()
    return _cases[name]


def kinds(case):
    return count_kinds(case["doc"])


def with_cfg(case, **kw):
    """The case with another frame: w, h, passes, depth, seed by name (its reference is cached under a name of its own)."""
    w, h, p, d, s = case["cfg"]
    cfg = (kw.get("w", w), kw.get("h", h), kw.get("passes", p), kw.get("depth", d), kw.get("seed", s))
    if cfg == case["cfg"]:
        return case
    c = dict(case)
    c["cfg"] = cfg
    c["name"] = "%s@%dx%dx%d-d%d-s%d" % ((case["name"].split("@")[0],) + cfg)
    return c


def reference(case, fog=None):
    """(rgba, accum, stats) of gr_render for the case, computed once."""
    key = case["name"] + ("+fog" if fog is not None else "")
    if key not in _refs:
        w, h, passes, depth, seed = case["cfg"]
        _refs[key] = gs.reference_render(case["ora"], gs.extras(case["sc"]), w, h, passes, depth, seed, fog)
    return _refs[key]


def frame_jobs(case, step=1):
    """Every step-th pixel of the case's frame, every pass: int32 [n, 3] = (x, y, pass)."""
    w, h, passes, _, _ = case["cfg"]
    pix = [(x, y) for y in range(h) for x in range(w)][::step]
    return np.array([(x, y, p) for p in range(passes) for x, y in pix], np.int32)


def _dome(mat):
    return {"id": "dome", "type": "sphere", "position": V(0, 0, 0), "size": V(DOME_RADIUS, 0, 0), "material_id": mat}


LAMP = {"id": "gw-lamp", "type": "emissive", "albedo": RGB(0, 0, 0), "emit": RGB(1.0, 0.85, 0.6), "power": 9.0}


def threshold_case():
    """129 spheres, a plane and 2 sphere lights: one sphere more than the grouped scan takes, the smallest tree.  The 129th sphere is
    the dome.  40 x 24: ragged blocks."""
    def make():
        mats = [{"id": "floor", "type": "lambert", "albedo": RGB(0.7, 0.7, 0.7)}, {"id": "ball", "type": "lambert", "albedo": RGB(0.3, 0.5, 0.7)},
                {"id": "steel", "type": "metal", "albedo": RGB(0.8, 0.8, 0.85), "rough": 0.3}, dict(LAMP),
                {"id": "sky", "type": "lambert", "albedo": RGB(0.5, 0.6, 0.8)}]
        objs = [{"id": "ground", "type": "plane", "position": V(0, 0, 0), "size": V(0, 0, 0), "material_id": "floor"}]
        for i in range(128):  # three layers of a 7 x 7 grid, the last 19 dropped
            gx, gz, gy = i % 7, (i // 7) % 7, i // 49
            objs.append({"id": "s%d" % i, "type": "sphere", "position": V(-3 + gx, 0.4 + 1.1 * gy, -3 + gz), "size": V(0.3 + 0.02 * (i % 5), 0, 0),
                         "material_id": "steel" if i % 6 == 0 else "ball"})
        objs.append(_dome("sky"))
        for i, p in enumerate(((-1.5, 4.5, 1.0), (2.5, 1.6, 2.5))):
            objs.append({"id": "l%d" % i, "type": "sphere_light", "position": V(*p), "size": V(0.25, 0, 0), "material_id": "gw-lamp"})
        doc = {"name": "gl-walk-threshold", "camera": {"position": V(0.5, 2.5, 9), "target": V(0, 1.2, 0), "up": V(0, 1, 0), "fov": 55},
               "materials": mats, "objects": objs, "background": RGB(0.05, 0.05, 0.08)}
        return _case("threshold", doc, (40, 24, 2, 8, 5))
    return _cached("threshold", make)


def _room_doc(dome=True):
    """About 400 objects with every material kind (synth.make_scene: lambert, metal rough 0.2 and 0, dielectric, mirror, emissive), plus:
    glass spheres and glass boxes with objects inside them, a rough metal slab facing a light (the reflect-direction probe fires),
    an emissive box (a light GL does not sample) and, with `dome`, the closing sphere."""
    from path_trace_golang_amd import synth

    doc = synth.make_scene(400, seed=3, room=8.0, light_every=100).encode()
    doc["materials"].append({"id": "brushed", "type": "metal", "albedo": RGB(0.9, 0.85, 0.8), "rough": 0.45})
    doc["materials"].append({"id": "shell", "type": "lambert", "albedo": RGB(0.4, 0.45, 0.5)})
    doc["materials"].append({"id": "green-glass", "type": "dielectric", "albedo": RGB(1, 1, 1), "ior": 1.5, "absorption": RGB(0.5, 0.1, 0.8),
                             "absorption_scale": 0.3, "tint": RGB(0.6, 1.0, 0.7)})
    add = doc["objects"].append
    add({"id": "gball", "type": "sphere", "position": V(-1.2, 1.2, 1.5), "size": V(0.9, 0, 0), "material_id": "green-glass"})
    add({"id": "gball-core", "type": "sphere", "position": V(-1.2, 1.2, 1.5), "size": V(0.35, 0, 0), "material_id": "red"})
    add({"id": "gbox", "type": "box", "position": V(1.4, 0.9, 1.2), "size": V(1.6, 1.6, 1.4), "material_id": "glass"})
    add({"id": "gbox-core", "type": "box", "position": V(1.4, 0.8, 1.2), "size": V(0.5, 0.5, 0.5), "material_id": "gold"})
    add({"id": "gbox-pearl", "type": "sphere", "position": V(1.7, 1.3, 1.4), "size": V(0.2, 0, 0), "material_id": "blue"})
    add({"id": "slab", "type": "box", "position": V(0.0, 0.15, 2.4), "size": V(2.5, 0.3, 1.2), "material_id": "brushed"})
    add({"id": "slab-lamp", "type": "sphere_light", "position": V(0.0, 2.2, 2.2), "size": V(0.3, 0, 0), "material_id": "lamp"})
    add({"id": "glowbox", "type": "box", "position": V(-2.5, 2.5, 0.0), "size": V(0.4, 0.4, 0.4), "material_id": "lamp"})
    if dome:
        add(_dome("shell"))
    return doc


def room_case():
    return _cached("room", lambda: _case("room", _room_doc(), (33, 20, 2, 8, 7)))


def far_case():
    """The room without its dome seen from 10 units beyond clip_bound = 3.5 x the scene bound on +z, through a pinhole: every primary
    ray starts outside the range the walk was analysed for (the plain loop), every later segment inside it (the walk)."""
    def make():
        doc = _room_doc(dome=False)
        b = scene_bound(doc)
        cam = doc["camera"]
        cam["position"] = V(0.0, cam["position"]["y"], 3.5 * b + 10.0)
        cam["aperture"] = 0.0
        cam["fov"] = 25.0
        return _case("far", doc, (33, 20, 2, 3, 7))
    return _cached("far", make)


TIE_SPHERE = ((-2.0, 1.0, 0.0), 0.8)            # the same sphere twice: lambert first, emissive second -- GL draws the emission
TIE_BOX = ((2.0, 1.0, 0.0), (1.4, 1.6, 1.2))    # the same box twice: the first one's material shows
TIE_TANGENT_BOX = ((0.0, 1.0, -1.0), (2.0, 2.0, 2.0))  # [-1, 1] x [0, 2] x [-2, 0]; the sphere inside touches its face z = 0 at (0, 1, 0)
TIE_TANGENT_SPHERE = ((0.0, 1.0, -1.0), 1.0)
TIE_TANGENT_RAY = ((0.0, 1.0, 9.0), (0.0, 0.0, -1.0))  # box entry 9 / 1 = 9; sphere: hb = -10, c = 99, disc = 1, (10 - 1) / 1 = 9
TIE_HALL = ((0.0, 6.0, 4.0), (24.0, 14.0, 24.0))  # the large glass box the camera sits in: every ray from inside hits it at tmin


def ties_case():
    """The tie constructions, padded beyond 128 spheres, inside the dome."""
    def make():
        mats = [{"id": "floor", "type": "lambert", "albedo": RGB(0.6, 0.6, 0.6)}, {"id": "floor2", "type": "lambert", "albedo": RGB(0.9, 0.3, 0.3)},
                {"id": "matte", "type": "lambert", "albedo": RGB(0.3, 0.6, 0.4)}, dict(LAMP),
                {"id": "chalk", "type": "lambert", "albedo": RGB(0.8, 0.8, 0.7)}, {"id": "ink", "type": "lambert", "albedo": RGB(0.1, 0.1, 0.3)},
                {"id": "hall", "type": "dielectric", "albedo": RGB(1, 1, 1), "ior": 1.3},
                {"id": "steel", "type": "metal", "albedo": RGB(0.8, 0.8, 0.85), "rough": 0.35},
                {"id": "shell", "type": "lambert", "albedo": RGB(0.4, 0.45, 0.5)}]
        objs = [{"id": "ground", "type": "plane", "position": V(0, 0, 0), "size": V(0, 0, 0), "material_id": "floor"},
                {"id": "ground-again", "type": "plane", "position": V(0, 0, 0), "size": V(0, 0, 0), "material_id": "floor2"},
                {"id": "twin-a", "type": "sphere", "position": V(*TIE_SPHERE[0]), "size": V(TIE_SPHERE[1], 0, 0), "material_id": "matte"},
                {"id": "twin-b", "type": "sphere", "position": V(*TIE_SPHERE[0]), "size": V(TIE_SPHERE[1], 0, 0), "material_id": "gw-lamp"},
                {"id": "cube-a", "type": "box", "position": V(*TIE_BOX[0]), "size": V(*TIE_BOX[1]), "material_id": "chalk"},
                {"id": "cube-b", "type": "box", "position": V(*TIE_BOX[0]), "size": V(*TIE_BOX[1]), "material_id": "ink"},
                {"id": "case", "type": "box", "position": V(*TIE_TANGENT_BOX[0]), "size": V(*TIE_TANGENT_BOX[1]), "material_id": "chalk"},
                {"id": "kernel", "type": "sphere", "position": V(*TIE_TANGENT_SPHERE[0]), "size": V(TIE_TANGENT_SPHERE[1], 0, 0), "material_id": "steel"},
                {"id": "hall", "type": "box", "position": V(*TIE_HALL[0]), "size": V(*TIE_HALL[1]), "material_id": "hall"},
                {"id": "lamp", "type": "sphere_light", "position": V(0.5, 4.5, 3.0), "size": V(0.4, 0, 0), "material_id": "gw-lamp"}]
        for i in range(130):  # the padding: a ring of small spheres, every fifth a rough metal
            a = 2 * np.pi * i / 130
            objs.append({"id": "p%d" % i, "type": "sphere", "position": V(5.0 * np.cos(a), 0.3 + 0.02 * (i % 7), 5.0 * np.sin(a) - 1.0),
                         "size": V(0.12 + 0.01 * (i % 4), 0, 0), "material_id": "steel" if i % 5 == 0 else "matte"})
        objs.append(_dome("shell"))
        doc = {"name": "gl-walk-ties", "camera": {"position": V(0.0, 1.0, 9.0), "target": V(0, 1.0, 0), "up": V(0, 1, 0), "fov": 50},
               "materials": mats, "objects": objs, "background": RGB(0.05, 0.05, 0.08)}
        return _case("ties", doc, (33, 20, 2, 8, 3))
    return _cached("ties", make)


TIE_HALL_INDEX = 8  # "hall" in the object list: what a path that has entered the hall skips (GL's currentGlassObject)


def tie_rays(case):
    """Queries aimed at the constructions of the ties scene, asked as a path inside the hall asks them (skip = the hall; without it
    the hall answers every query at tmin): the tangent ray, rays through both twins from several sides (also from inside them),
    along the coplanar planes' normal; then each closest query again with `skip` set to the object the loop answered."""
    hall = TIE_HALL_INDEX
    assert case["doc"]["objects"][hall]["id"] == "hall"
    cq = lambda ro, rd, **kw: closest_query(ro, rd, skip=kw.pop("skip", hall), **kw)  # noqa: E731
    q = [cq(*TIE_TANGENT_RAY), cq((0.0, 1.0, 9.0), (0.0, 0.0, -2.0)), cq((0.0, 1.0, 3.0), (0.0, 0.0, -1.0)),
         cq(*TIE_TANGENT_RAY, tmax=9.0),  # tmax_start at the shared t: the sphere is accepted at <=, the box is not at <
         cq(*TIE_TANGENT_RAY, skip=-1),   # nothing skipped: the hall at tmin
         shadow_query(TIE_TANGENT_RAY[0], TIE_TANGENT_RAY[1], 9.0)]
    for c in (TIE_SPHERE[0], TIE_BOX[0]):
        c = np.array(c)
        for d in ((0, 0, -1), (1, 0, 0), (0, -1, 0), (0.6, -0.3, -0.7), (-0.2, 0.9, 0.1)):
            d = np.array(d, float)
            for back in (6.0, 2.5, 0.0):  # from outside, from nearby, from the centre
                q.append(cq(tuple(c - d * back), tuple(d)))
                q.append(shadow_query(tuple(c - d * back), tuple(d), 4.0))
    q.append(cq((1.0, 3.0, 5.0), (0.0, -1.0, 0.0)))   # the two planes, head on
    q.append(cq((1.0, 3.0, 5.0), (0.3, -0.5, -0.2)))
    q.append(cq((1.0, 3.0, 5.0), (0.0, -1.0, 0.0), tmax=3.0))  # tmax_start at the planes' t: both accepted at <=
    with Host(case) as hst:
        idx, _, _ = hst.queries(np.array(q))
    for row, (win, _) in zip(list(q), idx):
        if row[0] == 0 and win >= 0:
            q.append(row[:9] + [float(win), 0.0])  # the winner itself skipped
    return np.array(q)


def fuzz_case(i):
    """Random geometry i: fuzz_support.random_doc untrimmed (overlapping, nested, coincident objects, several planes, boxes without
    a volume, missing material ids) at 300 / 450 / 700 objects with 0 / 1 / 8 / 9 / 12 lights and random GL extras, inside the dome."""
    def make():
        rng = np.random.default_rng([4711, i])
        doc = random_doc(rng, FUZZ_COUNTS[i % 3])
        random_gl_extras(doc, rng)
        set_lights(doc, FUZZ_LIGHTS[i % 5], kind="sphere" if i % 2 else "sphere_light", seed=i)
        doc["materials"].append({"id": "shell", "type": "lambert", "albedo": RGB(0.4, 0.45, 0.5)})
        doc["objects"].append(_dome("shell"))
        w, h = FUZZ_FRAMES[i % 2]
        return _case("fuzz%d" % i, doc, (w, h, 1 + i % 2, (1, 3, 8, 12)[i % 4], 200 + i))
    return _cached("fuzz%d" % i, make)


def unknown_type_case():
    """The room with a torus: GL draws it as a sphere, the device world drops it."""
    def make():
        doc = _room_doc()
        doc["objects"].insert(7, {"id": "torus", "type": "torus", "position": V(0.5, 1.0, 1.0), "size": V(0.6, 0.2, 0), "material_id": "red"})
        return _case("unknown", doc, (33, 20, 1, 3, 7))
    return _cached("unknown", make)


UNKNOWN_INDEX = 7


def negative_box_case():
    """The room with a box of negative width in front of the camera: bmin > bmax on x, which no ray can hit."""
    def make():
        doc = _room_doc()
        doc["objects"].insert(5, {"id": "inside-out", "type": "box", "position": V(0.0, 1.5, 3.0), "size": V(-2.0, 1.5, 1.0), "material_id": "red"})
        return _case("negbox", doc, (33, 20, 1, 3, 7))
    return _cached("negbox", make)


def linear_case(n):
    """About n objects and 4 lights: what gl_trace_kernel under PTCORE_SCAN=uniform and gl_bvh_kernel both render."""
    def make():
        from path_trace_golang_amd import synth

        doc = synth.make_scene(n, seed=11, room=12.0, light_every=0).encode()
        for i in range(4):
            a = 2 * np.pi * i / 4 + 0.3
            doc["objects"].append({"id": "ring%d" % i, "type": "sphere_light", "position": V(3.5 * np.cos(a), 6.0 + 0.3 * (i % 3), 3.5 * np.sin(a)),
                                   "size": V(0.3, 0, 0), "material_id": "lamp"})
        return _case("linear%d" % n, doc, (32, 18, 1, 3, 13))
    return _cached("linear%d" % n, make)


def small_case():
    """27 objects: far below the BVH path."""
    def make():
        from path_trace_golang_amd import synth

        return _case("small", synth.make_scene(26, seed=2, room=8.0, light_every=9).encode(), (32, 18, 1, 3, 3))
    return _cached("small", make)


def moved(case, ids=("gball", "gbox-core", "slab-lamp"), by=(0.25, 0.1, -0.2)):
    """The case with three of its objects moved (the topology stays: what pt_set_bvh_refit refits)."""
    doc = copy.deepcopy(case["doc"])
    hit = 0
    for o in doc["objects"]:
        if o["id"] in ids:
            for k, dv in zip("xyz", by):
                o["position"][k] += dv
            hit += 1
    assert hit == len(ids)
    return _case(case["name"].split("@")[0] + "-moved", doc, case["cfg"])
