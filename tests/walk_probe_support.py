"""The queries of test_walk_probe_cpu.py / test_walk_probe_gpu.py: arbitrary rays -- the classes of ray_inject_support.py on the
341-object scene rescaled by 2^k -- asked of the fog's wave-shared any-hit walk (csrc/pt_fog_walk.h) and of GL shading's per-lane
walks (csrc/pt_gl_walk.h), with the plain loops of tests/glshade_reference.c (gr_queries) and tests/fog_reference.c
(fr_occluded_many) as the reference; the device probe tests/walk_probe.hip, built like roulette_probe_support.compile_probe builds
its own; and the stand-alone host program tests/walk_host_probe.cpp.

Every class of ray_inject_support.classes() is 64 waves of 64 rays.  WAVES keeps 13 of them, every fifth (832 rays per class: the
classes repeat their rays to fill a frame, so a stride keeps every part of a class, and 13 waves of stride 5 keep every odd kind and
every lane position of the mixed class), so that the reference's side of one scale stays within a few seconds.  No class and no
scale is cut.  One more wave of edge origins (edge_origins) is added to "far origins".

From a ray the tables below make 11 GL queries and 4 fog shadow rays (queries_of).  Lane i of the GL launch is query i: the eleven
queries of a ray are neighbours, so every wave mixes kinds, tmin / tmax and skip."""
from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

import glshade_support as gs
import glwalk_support as gw
import ray_inject_support as S
import scaled_scene_support as X
from fog_support import CSRC, ROOT, ptr

SOURCE = os.path.join(ROOT, "tests", "walk_probe.hip")
HOST_SOURCE = os.path.join(ROOT, "tests", "walk_host_probe.cpp")
# the product's routines the probe calls (a CPU test holds the source to this list)
PRODUCT = ("ptg::TreeWorld", "world.closest", "world.occluded", "ptg::WalkCount", "ptg::walk_scene_check", "ptg::gl_object", "scene_to_world",
           "ptbvh::build_scene_trees", "ptbvh::world_bound", "ptbvh::frame_bounds", "ptf::make_fray", "ptk::wave_walk_coop", "ptk::wave_any_hit(",
           "ptk::wave_any_hit_plain")
K = tuple(k for k in X.K if k < 120)   # 120 and 130 leave the BVH path (the world goes to the plain loop)
assert K == (-140, -40, -4, -3, 40, 60, 61, 64, 90, 96, 97, 119)
CLASSES = ("length", "components", "near geometry", "far origins", "mixed")
WAVES = tuple(range(0, S.NWAVES, 5))     # 13 waves of every class
RAYS_PER_CLASS = 64 * len(WAVES)         # 832
SCALED_SCENES = ("bvh", "bvh-noplanes")
PTF_TMAX = 40.0
GL_PER_RAY, FOG_PER_RAY = 11, 4
DBL_MAX = float(np.finfo(np.float64).max)
MASKS = ("full", "lane 0", "lane 37", "lane 63", "alternating", "lanes 0..31", "empty")
FRAME_K = (-3, 40)                      # the frame-level item's scales
WALK_COUNT = ("closest_walked", "closest_plain", "shadow_walked", "shadow_plain", "closest_visits", "shadow_visits", "deepest")

_dir = None
_lib = None
_cache = {}


def _tmp():
    global _dir
    if _dir is None:
        _dir = tempfile.mkdtemp(prefix="walkprobe_")
    return _dir


# ---------------------------------------------------------------- scenes
def case_of(scene_name: str, k: int = 0):
    """A glwalk_support case: the 341-object scene times 2^k, with its plane or without ("bvh-noplanes"); "ties", "fuzz0" unscaled."""
    key = ("case", scene_name, k)
    if key not in _cache:
        if scene_name == "ties":
            _cache[key] = gw.ties_case()
        elif scene_name.startswith("fuzz"):
            _cache[key] = gw.fuzz_case(int(scene_name[4:]))
        else:
            doc = X.doc_of("bvh", k)
            if scene_name == "bvh-noplanes":
                doc = X.without_planes(doc)
            _cache[key] = gw._case("%s@k%d" % (scene_name, k), doc, (33, 20, 1, 3, 7))
    return _cache[key]


FRAME_MOVED = ((1, (0.25, 0.1, -0.2)), (4, (-0.2, 0.0, 0.3)), (7, (0.1, -0.25, 0.2)))  # (object, displacement at k = 0)


def frame_case(k: int, moved: bool = False):
    """The 341-object scene times 2^k as a 33 x 20 frame of 1 pass at depth 3; `moved`: three of its objects displaced (the
    topology stays: what a refit takes)."""
    key = ("frame", k, moved)
    if key not in _cache:
        doc = X.scaled_doc(S.scene_doc("bvh"), k)
        if moved:
            for i, by in FRAME_MOVED:
                for c, dv in zip("xyz", by):
                    doc["objects"][i]["position"][c] += dv * 2.0 ** k
        _cache[key] = gw._case("frame@k%d%s" % (k, "-moved" if moved else ""), doc, (33, 20, 1, 3, 7))
    return _cache[key]


def scene_list(k: int):
    """(scene name, k) pairs of one parameter of the tests: the scaled scenes at k; at k = 0 (no listed scale) the two tie scenes."""
    return [(s, k) for s in SCALED_SCENES] if k != 0 else [("ties", 0), ("fuzz0", 0)]


def families(scene_name: str, k: int):
    return X.families(k) if scene_name in SCALED_SCENES else ("unit",)


def band_walks(scene_name: str, k: int, family: str) -> bool:
    """Does a ray of ordinary length walk at this scale?  Unit directions do at every k; directions scaled with the scene have
    d.d = 4^k a0, inside walk_ok's (1e-29, 1e29) for |k| <= 48.  (Outside it only strays of the "length" and "mixed" classes walk,
    whose own factor happens to undo the scale.)"""
    return family == "unit" or scene_name not in SCALED_SCENES or 1e-29 < 4.0 ** k < 1e29


def host_info(case):
    """(counts, bounds) of the host build's tables (gw_info): bounds are read from here, never recomputed."""
    key = ("info", case["name"])
    if key not in _cache:
        with gw.Host(case) as h:
            _cache[key] = h.info()
    return _cache[key]


def kinds_of(case):
    """Per object index: 0 sphere, 1 plane, 2 box; the last entry (index -1) is 'miss' = 3."""
    code = {"sphere": 0, "sphere_light": 0, "plane": 1, "box": 2}
    return np.array([code[o["type"]] for o in case["doc"]["objects"]] + [3])


# ---------------------------------------------------------------- rays
def class_waves(name: str) -> np.ndarray:
    """[13][64][6]: the kept waves of a class, lane by lane as the device would hold them."""
    key = ("waves", name)
    if key not in _cache:
        tab = S.classes()[name].reshape(S.H, S.W, 6)
        ys, xs = np.mgrid[0:S.H, 0:S.W]
        by_wave = np.zeros((S.NWAVES, 64, 6))
        by_wave[S.wave_of(xs, ys), S.lane_of(xs, ys)] = tab
        _cache[key] = np.ascontiguousarray(by_wave[list(WAVES)])
    return _cache[key]


def edge_origins(bounds: dict, scale: float) -> np.ndarray:
    """[64][6], directions of unit length: per axis and sign an origin component at clip_bound, at 0.99 * (double)origin_bound and at
    the neighbours of each one ulp in and out (36 rays; then the same again towards other targets), the other components inside the
    scene, aimed at the scene."""
    rng = np.random.default_rng(108)
    lim = 0.99 * float(np.float64(np.float32(bounds["origin_bound"])))
    combos = [(axis, sgn, float(S.ulps(base, u))) for base in (bounds["clip_bound"], lim) for axis in range(3) for sgn in (1.0, -1.0) for u in (-1, 0, 1)]
    tg = S._targets(rng, 64) * scale
    out = np.zeros((64, 6))
    with np.errstate(all="ignore"):
        for j in range(64):
            axis, sgn, v = combos[j % len(combos)]
            o = np.array([0.5, 2.0, 0.75]) * scale
            o[axis] = sgn * v
            d = tg[j] - o
            out[j, 0:3], out[j, 3:6] = o, d / np.sqrt(d @ d)
    return out


def rays_of(case, k: int, family: str):
    """(rays [n][6] in waves of 64, {class: slice}) of a scene at a scale in a family."""
    key = ("rays", case["name"], k, family)
    if key not in _cache:
        _, bounds = host_info(case)
        parts, where, at = [], {}, 0
        for name in CLASSES:
            r = X.scaled_rays(class_waves(name).reshape(-1, 6), k, family)
            if name == "far origins":
                e = edge_origins(bounds, 2.0 ** k)
                if family == "similar":
                    with np.errstate(all="ignore"):
                        e[:, 3:6] *= 2.0 ** k
                r = np.concatenate([r, e])
            parts.append(r)
            where[name] = slice(at, at + len(r))
            at += len(r)
        rays = np.ascontiguousarray(np.concatenate(parts))
        assert len(rays) % 64 == 0
        rays.setflags(write=False)
        _cache[key] = (rays, where)
    return _cache[key]


def walk_ok(bounds: dict, ro, rd) -> np.ndarray:
    """ptg::walk_ok restated: 1e-29 < d.d < 1e29, every |origin component| within clip_bound and 0.99 * (double)origin_bound."""
    lim = 0.99 * float(np.float64(np.float32(bounds["origin_bound"])))
    with np.errstate(all="ignore"):
        a = rd[:, 0] * rd[:, 0] + rd[:, 1] * rd[:, 1] + rd[:, 2] * rd[:, 2]
        ok = (a > 1e-29) & (a < 1e29)
        for c in range(3):
            ok &= (np.abs(ro[:, c]) <= bounds["clip_bound"]) & (np.abs(ro[:, c]) <= lim)
    return ok


def lane_passes(bounds: dict, ro, rd) -> np.ndarray:
    """What wave_walk_coop asks of a lane that holds a ray: tame (1e-100 <= a <= 1e100, the origin within clip_bound) and
    bvh_ray_trusted without a clip (1e-29 < a < 1e29, |o + d * 0| within 0.99 origin_bound)."""
    lim = 0.99 * float(np.float64(np.float32(bounds["origin_bound"])))
    with np.errstate(all="ignore"):
        a = rd[:, 0] * rd[:, 0] + rd[:, 1] * rd[:, 1] + rd[:, 2] * rd[:, 2]
        ok = (a >= 1e-100) & (a <= 1e100) & (a > 1e-29) & (a < 1e29)
        for c in range(3):
            ok &= (np.abs(ro[:, c]) <= bounds["clip_bound"]) & (np.abs(ro[:, c] + rd[:, c] * 0.0) <= lim)
    return ok


def mask_lanes(name: str) -> np.ndarray:
    lane = np.arange(64)
    return {"full": lane >= 0, "lane 0": lane == 0, "lane 37": lane == 37, "lane 63": lane == 63, "alternating": lane % 2 == 0,
            "lanes 0..31": lane < 32, "empty": lane < 0}[name]


# ---------------------------------------------------------------- the reference
def _ref():
    L = gs.reference()
    if not getattr(L, "_walk_probe", False):
        vp = C.c_void_p
        L.gr_queries.restype = None
        L.gr_queries.argtypes = [vp, vp, C.c_int64, vp, vp, vp]
        L.fr_occluded_many.restype = None
        L.fr_occluded_many.argtypes = [vp, C.c_int64, vp, vp]
        L._walk_probe = True
    return L


def ref_queries(case, q):
    """gr_queries: (idx i32 [n], t f64 [n]) of the loop over all objects of tests/glshade_reference.c."""
    q = np.ascontiguousarray(q, np.float64)
    n = len(q)
    idx, t = np.zeros(n, np.int32), np.zeros(n)
    _ref().gr_queries(C.byref(case["ora"].c), C.cast(gs.extras(case["sc"]), C.c_void_p), n, ptr(q), ptr(idx), ptr(t))
    return idx, t


def ref_occluded(case, rays7):
    """fr_occluded_many: blocked i32 [n] of the shadow test of tests/fog_reference.c."""
    rays7 = np.ascontiguousarray(rays7, np.float64)
    out = np.zeros(len(rays7), np.int32)
    _ref().fr_occluded_many(C.byref(case["ora"].c), len(rays7), ptr(rays7), ptr(out))
    return out


def _row(kind, rays, tmin, tmax, skip):
    n = len(rays)
    q = np.zeros((n, 11))
    q[:, 0] = kind
    q[:, 1:7] = rays
    q[:, 7] = tmin
    q[:, 8] = tmax
    q[:, 9] = skip
    return q


def queries_of(case, rays):
    """dict(q [11 n][11] GL queries, ray by ray; fog [4 n][7] shadow rays, turn by turn (turn j = rays with the j-th tmax); idx0, t0:
    the reference's first hit of every ray in (0.001, MaxFloat64): in the unit family t goes with 2^k and passes the model's 1e20
    from k = 64 on, where a first hit within 1e20 would leave only misses).  Per ray:
      closest (0.001, 1e20), (0.001, PTF_TMAX), (0.001, MaxFloat64), tmax = t0 and its neighbours one ulp down and up, skip = the
      reference's winner; occluded with tmax = t0, its neighbours, 0.0009; the fog's shadow rays with the same four."""
    n = len(rays)
    idx0, t0 = ref_queries(case, _row(0, rays, 0.001, DBL_MAX, -1))
    with np.errstate(all="ignore"):
        dn, up = np.nextafter(t0, -np.inf), np.nextafter(t0, np.inf)
    per = [_row(0, rays, 0.001, 1e20, -1), _row(0, rays, 0.001, PTF_TMAX, -1), _row(0, rays, 0.001, DBL_MAX, -1), _row(0, rays, 0.001, t0, -1), _row(0, rays, 0.001, dn, -1),
           _row(0, rays, 0.001, up, -1), _row(0, rays, 0.001, 1e20, idx0), _row(1, rays, 0.001, t0, -1), _row(1, rays, 0.001, dn, -1),
           _row(1, rays, 0.001, up, -1), _row(1, rays, 0.001, 0.0009, -1)]
    assert len(per) == GL_PER_RAY
    q = np.ascontiguousarray(np.stack(per, axis=1).reshape(GL_PER_RAY * n, 11))
    fog = np.concatenate([np.concatenate([rays, np.broadcast_to(np.asarray(tm, float), (n,))[:, None]], axis=1) for tm in (t0, dn, up, 0.0009)])
    return dict(q=q, fog=np.ascontiguousarray(fog), idx0=idx0, t0=t0)


def table(scene_name: str, k: int, family: str):
    """Everything the tests of one (scene, k, family) share, computed once and left unchanged: the rays, the queries, the reference's
    answers (gl_idx, gl_t of gr_queries; fog_blocked of fr_occluded_many), the numpy predicates."""
    key = ("table", scene_name, k, family)
    if key not in _cache:
        case = case_of(scene_name, k)
        info, bounds = host_info(case)
        rays, where = rays_of(case, k, family)
        Q = queries_of(case, rays)
        if scene_name == "ties":  # the tie constructions' own queries, behind the table's
            Q["q"] = np.ascontiguousarray(np.concatenate([Q["q"], gw.tie_rays(case)]))
        gl_idx, gl_t = ref_queries(case, Q["q"])
        T = dict(case=case, info=info, bounds=bounds, rays=rays, where=where, q=Q["q"], fog=Q["fog"], idx0=Q["idx0"], t0=Q["t0"], gl_idx=gl_idx, gl_t=gl_t,
                 fog_blocked=ref_occluded(case, Q["fog"]), ok=walk_ok(bounds, Q["q"][:, 1:4], Q["q"][:, 4:7]), ray_ok=walk_ok(bounds, rays[:, 0:3], rays[:, 3:6]),
                 fog_pass=lane_passes(bounds, Q["fog"][:, 0:3], Q["fog"][:, 3:6]))
        for v in T.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[key] = T
    return _cache[key]


def same_t(a, b) -> np.ndarray:
    """t equal bit for bit; two NaNs count as equal whatever their sign and payload (IEEE 754 leaves those of an invalid operation's
    result to the implementation, and the host and the device differ there)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def host_answers(T):
    """The host build of ptg::TreeWorld on the table's queries (gw_queries): (idx [n][2], t [n][2], deepest) with column 0 the
    product's loop, column 1 its tree policy.  Walked / plain per query: the queries numpy's walk_ok accepts and the others go in
    two calls, and the tree policy must have walked every query of the first and none of the second."""
    q, ok = T["q"], T["ok"]
    idx, t = np.zeros((len(q), 2), np.int32), np.zeros((len(q), 2))
    deepest = 0
    with gw.Host(T["case"]) as h:
        for sel, walked in ((ok, True), (~ok, False)):
            if not sel.any():
                continue
            i, tt, wc = h.queries(q[sel])
            idx[sel], t[sel] = i, tt
            n = int(np.count_nonzero(sel))
            got = (wc["closest_walked"] + wc["shadow_walked"], wc["closest_plain"] + wc["shadow_plain"])
            assert got == ((n, 0) if walked else (0, n)), (T["case"]["name"], "walk_ok restated disagrees with the host build", walked, n, wc)
            deepest = max(deepest, wc["deepest_stack"])
    return idx, t, deepest


def report_line(what, scene_name, k, family, T, walked, disagreements) -> str:
    kinds = kinds_of(T["case"])[T["gl_idx"][T["q"][:, 0] == 0]]
    return ("walk probe: %-10s on %-12s k %4d [%s] %-7s: %d GL queries + %d fog rays, walked %d / plain %d, closest hits %d sphere / %d box / %d plane / "
            "%d miss, blocked %d GL / %d fog, disagreements %d"
            % (what, scene_name, k, X.band(k), family, len(T["q"]), len(T["fog"]), int(walked), len(T["q"]) - int(walked),
               *(int(np.count_nonzero(kinds == c)) for c in (0, 2, 1, 3)), int(np.count_nonzero(T["gl_idx"][T["q"][:, 0] == 1])),
               int(np.count_nonzero(T["fog_blocked"])), disagreements))


# ---------------------------------------------------------------- the stand-alone host program
def deep_scene_rows():
    """(objects [n][7] = type, position, size; ...) of the deepest-tree case: bvh_build_support's "geometric ratio 2" world (300 spheres at
    x = 2^(i - 200), radius x / 4) as scene objects, type 0 = sphere."""
    import bvh_build_support as bb

    w = bb.special_world("geometric ratio 2")
    rows = np.zeros((len(w), 7))
    rows[:, 1:4] = w["a"]
    rows[:, 4] = w["radius"]
    return rows


def deep_queries(rows):
    """Closest and occluded queries along the chain and across it, from inside and outside."""
    rng = np.random.default_rng(109)
    q = []
    far = float(rows[:, 1].max()) * 1.5
    for i in range(0, len(rows), 7):
        c, r = rows[i, 1:4], rows[i, 4]
        for o, d in (((far, 0.0, 0.0), (-1.0, 0.0, 0.0)), ((-far, 0.0, 0.0), (1.0, 0.0, 0.0)), (tuple(c + np.array([0.0, 3.0 * r, 0.0])), (0.0, -1.0, 0.0)),
                     (tuple(c), tuple(rng.normal(size=3))), ((far, 0.5 * r, 0.0), tuple(S._unit(c - np.array([far, 0.5 * r, 0.0]))))):
            q.append(gw.closest_query(o, d))
            q.append(gw.shadow_query(o, d, 2.0 * far))
    return np.array(q)


def build_host(flags=(), name="walk_host_probe"):
    exe = os.path.join(_tmp(), name)
    cxx = os.environ.get("CXX") or shutil.which("g++") or "g++"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fno-fast-math", *flags, "-I" + CSRC,
                    HOST_SOURCE, "-o", exe], check=True)  # (the walks' `#pragma unroll` is the device compiler's)
    return exe


def _hex(a):
    return " ".join("%016x" % int(v) for v in np.asarray(a, np.float64).view(np.uint64))


def run_host(exe, rows, q):
    """dict(info = [built, stack_need, deepest, walked, plain], idx i32 [n][2], t f64 [n][2]): the loop and the tree policy."""
    text = "%d %d\n" % (len(rows), len(q)) + "".join("%d %s\n" % (int(r[0]), _hex(r[1:7])) for r in rows) + "".join(_hex(r[:10]) + "\n" for r in q)
    r = subprocess.run([exe], input=text, check=True, capture_output=True, text=True)
    assert r.stderr == "", r.stderr  # a sanitizer report goes there
    lines = r.stdout.split("\n")[:-1]
    info = [int(v) for v in lines[0].split()]
    body = [ln.split() for ln in lines[1:]]
    assert len(body) == len(q)
    idx = np.array([[int(w[0]), int(w[1])] for w in body], np.int32)
    t = np.array([[int(w[2], 16), int(w[3], 16)] for w in body], np.uint64).view(np.float64)
    return dict(info=info, idx=idx, t=t)


# ---------------------------------------------------------------- the device probe
def compile_probe() -> str:
    from path_trace_golang_amd import build

    out = os.path.join(_tmp(), "libwalkprobe.so")
    if not os.path.exists(out):
        r = subprocess.run([build.HIPCC, *build.HIP_FLAGS, "-shared", "-I", CSRC, "-I", os.path.join(ROOT, "tests"), SOURCE, "-o", out],
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("walk probe does not compile:\n%s\n%s" % (r.stdout, r.stderr))
    return out


def load():
    """The probe, loaded after torch so that the process keeps one HIP runtime (as conftest.gpu_ctx does for libptcore.so)."""
    global _lib
    if _lib is None:
        import torch  # noqa: F401

        L = C.CDLL(compile_probe())
        vp, i64 = C.c_void_p, C.c_int64
        L.wp_guard.restype = i64
        L.wp_guard.argtypes = []
        L.wp_open.restype = vp
        L.wp_open.argtypes = [vp, vp]
        L.wp_close.restype = None
        L.wp_close.argtypes = [vp]
        L.wp_info.restype = None
        L.wp_info.argtypes = [vp, vp, vp]
        L.wp_gl_queries.restype = C.c_int
        L.wp_gl_queries.argtypes = [vp, i64, vp, vp, vp, vp]
        L.wp_fog_turns.restype = C.c_int
        L.wp_fog_turns.argtypes = [vp, i64, vp, vp, vp, vp]
        _lib = L
    return _lib


class Device:
    """A case's tables on the device, built by the probe on the host as gw_open builds them."""

    def __init__(self, case):
        from path_trace_golang_amd import hip

        self.flat = hip.FlatScene(case["sc"])
        self.ex = gs.extras(case["sc"])
        self.h = load().wp_open(C.byref(self.flat.c), C.cast(self.ex, C.c_void_p))
        if not self.h:
            raise RuntimeError("wp_open failed")

    def __enter__(self):
        return self

    def __exit__(self, *a):
        if self.h:
            load().wp_close(self.h)
            self.h = None

    def info(self):
        out, b = np.zeros(9, np.int32), np.zeros(4)
        load().wp_info(self.h, ptr(out), ptr(b))
        names = ("built", "main_nodes", "main_objs", "stack_need", "planes", "world", "bvh_stack", "gl_ok", "nodes")
        return dict(zip(names, (int(v) for v in out))), dict(zip(("origin_bound", "dir_floor", "clip_bound", "margin"), (float(v) for v in b)))

    def gl_queries(self, q):
        """(idx i32 [n], t f64 [n], wc u32 [n][7] = WALK_COUNT per lane)."""
        L = load()
        q = np.ascontiguousarray(q, np.float64)
        n, g = len(q), int(L.wp_guard())
        idx, t, wc = np.zeros(n + g, np.int32), np.zeros(n + g, np.uint64), np.zeros((n + g, 7), np.uint32)
        rc = L.wp_gl_queries(self.h, n, ptr(q), ptr(idx), ptr(t), ptr(wc))
        if rc != 0:
            raise RuntimeError("wp_gl_queries: status %d" % rc)
        for a in (idx, t, wc):
            assert np.all(a[n:].view(np.uint8) == 0xFF), "guard words were written"
        return idx[:n], t[:n].view(np.float64), wc[:n]

    def fog_turns(self, rays7, active):
        """(blocked i32 [n], waves u32 [n / 64][3] = coop, visits, deepest; 0xFFFFFFFF where a wave wrote nothing)."""
        L = load()
        rays7 = np.ascontiguousarray(rays7, np.float64)
        active = np.ascontiguousarray(active, np.uint8)
        n, g = len(rays7), int(L.wp_guard())
        assert n % 64 == 0 and len(active) == n
        blocked, waves = np.zeros(n + g, np.int32), np.zeros((n // 64 + g, 3), np.uint32)
        rc = L.wp_fog_turns(self.h, n // 64, ptr(rays7), ptr(active), ptr(blocked), ptr(waves))
        if rc != 0:
            raise RuntimeError("wp_fog_turns: status %d" % rc)
        for a, m in ((blocked, n), (waves, n // 64)):
            assert np.all(a[m:].view(np.uint8) == 0xFF), "guard words were written"
        return blocked[:n], waves[:n // 64]
