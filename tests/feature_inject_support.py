"""Injected rays for feature_bvh_kernel (csrc/pt_feature_walk.h), shared by test_feature_inject_cpu.py and
test_feature_inject_gpu.py: the classes of ray_inject_support.py and its named case, the walk's own classification restated on
the inputs, the layout that lets the walk see a class's rays, the oracle's per-ray records and ids, and the comparison.

The walk is taken by a wave (one 8 x 8 block of one sample) only when NONE of its 64 rays is odd, where a ray is odd unless
    1e-29 < a < 1e29  and  max |origin component| <= 3.5 B          (a = d.d in FP64, B the scene bound; NaN fails both)
-- `tame` with F.clip_bound and bvh_ray_trusted with the no-clip Clip, as the kernel's header comment and DESIGN 3.11a state them.
One odd lane sends the whole wave to scan_uniform.  In ray_inject_support's own layout the classes that hold the degenerate rays
(zero and denormal direction components, whose FP32 reciprocals make infinite and NaN slab parameters) have an odd lane in nearly
every wave, so those rays would never be walked: walk_layout puts a class's non-odd rows first, wave by wave."""
from __future__ import annotations

import ctypes as C

import numpy as np

import ray_inject_support as S

NAMED = "beside a core"
CLASS_NAMES = ("length", "components", "near geometry", "far origins", "incoherent", "mixed", NAMED)
# whole waves the walk must take after walk_layout: floor(non-odd rows / 64) of the tables as they are (test_feature_inject_cpu.py)
MIN_WALKED = {"components": 56, "mixed": 55, "far origins": 22, "length": 1, "near geometry": 64, "incoherent": 64, NAMED: 64}
DEPTH = 2
LAYOUTS = ("original", "walk")

_cache = {}


def named_table() -> np.ndarray:
    """The named case for this kernel: the four rays of S.NAMED_RAYS, each followed by the ray from the same origin the other way.
    The named rays start at the scene's edge and all hit after passing beside many cores; turned round they leave the scene, so the
    table also holds misses and both senses of every axis.  Every wave holds all eight, eight times."""
    named = np.array(S.NAMED_RAYS[NAMED], float)
    away = named.copy()
    away[:, 3:6] = -away[:, 3:6]
    eight = np.stack([named, away], axis=1).reshape(8, 6)
    return S.to_table(np.tile(eight, (S.W * S.H // 8, 1)))


def tables() -> dict:
    """{name: [W*H][6]} the six classes and the named case, in ray_inject_support's layout.  Read-only."""
    if "tables" not in _cache:
        t = dict(S.classes())
        t[NAMED] = named_table()
        for a in t.values():
            a.setflags(write=False)
        _cache["tables"] = t
    return _cache["tables"]


def walk_odd(rays, bound=S.BOUND) -> np.ndarray:
    """[n] bool: the rays that keep their wave off the shared walk."""
    rays = np.asarray(rays, np.float64).reshape(-1, 6)
    a = S.dir_a(rays)
    with np.errstate(all="ignore"):
        ok = (a > 1e-29) & (a < 1e29) & (S.omax(rays) <= 3.5 * bound)  # a comparison with NaN is false: odd
    return ~ok


def odd_waves(table, bound=S.BOUND) -> int:
    """Waves of a [W*H][6] table that hold at least one odd ray."""
    return len(np.unique(S.waves_of_table(table)[walk_odd(table, bound)]))


def walk_layout(rays, bound=S.BOUND):
    """A 4096-row class laid out for the walk: a stable partition, the non-odd rows first and the odd rows last, placed wave by
    wave (row k is lane k % 64 of wave k // 64) through S.to_table, so at most one wave mixes the two.  Returns (table, the
    number of waves that must take the plain scan: those holding an odd row, counted from the predicate on the table)."""
    rays = np.asarray(rays, np.float64).reshape(S.W * S.H, 6)
    odd = walk_odd(rays, bound)
    order = np.concatenate([np.flatnonzero(~odd), np.flatnonzero(odd)])
    table = S.to_table(rays[order])
    return table, odd_waves(table, bound)


def laid_out(name: str, layout: str):
    """(table, expected plain waves) of a class in one of LAYOUTS.  Cached, read-only."""
    key = ("laid", name, layout)
    if key not in _cache:
        t = tables()[name]
        out = (t, odd_waves(t)) if layout == "original" else walk_layout(t)
        out[0].setflags(write=False)
        _cache[key] = out
    return _cache[key]


# ---------------------------------------------------------------- the oracle's side
def ora_scene(doc, key=None):
    """ora.Scene of a document, kept alive under `key`."""
    from oracle import ora

    if key is None:
        return ora.Scene(doc)
    if ("osc", key) not in _cache:
        _cache[("osc", key)] = ora.Scene(doc)
    return _cache[("osc", key)]


def oracle_records(osc, rays, key=None) -> dict:
    """The oracle's first hit of every ray: rec [n][8] = (hit, normal[3], albedo[3], t |d|) by tests/atrous_reference.c, ids and
    tie [n] by tests/object_ids_reference.c (tie: another object's hit lies within 1e-9 of the winner's).  Cached under `key`."""
    import atrous_support as at
    import temporal_motion_support as tm

    if key is not None and ("rec", key) in _cache:
        return _cache[("rec", key)]
    rays = np.ascontiguousarray(rays, np.float64)
    rec = np.zeros((len(rays), 8))
    at.reference().ar_first_hit_many(C.byref(osc.c), len(rays), at.ptr(rays), at.ptr(rec))
    ids, tie = tm.oracle_ids_of_rays(osc, rays)
    out = dict(rec=rec, ids=ids, tie=tie, nonfinite=~np.all(np.isfinite(rec), axis=1))
    for a in out.values():
        a.setflags(write=False)
    if key is not None:
        _cache[("rec", key)] = out
    return out


def expected_planes(rec, w: int, h: int, spp: int):
    """(normal, albedo, depth) [h][w][3] of a frame whose (pixel, sample) records are rec [(y*w + x)*spp + s][8]: the sums as the
    kernel keeps them, from zero, one sample after the other in FP64."""
    rec = np.asarray(rec).reshape(h, w, spp, 8)
    n, a, d = np.zeros((h, w, 3)), np.zeros((h, w, 3)), np.zeros((h, w, 3))
    with np.errstate(all="ignore"):
        for s in range(spp):
            r = rec[:, :, s]
            hit = r[..., 0] != 0
            n = np.where(hit[..., None], n + r[..., 1:4], n)
            a = np.where(hit[..., None], a + r[..., 4:7], a)
            d[..., 0] = np.where(hit, d[..., 0] + r[..., 7], d[..., 0])
            d[..., 1] = np.where(hit, d[..., 1] + 1.0, d[..., 1])
            d[..., 2] = d[..., 2] + 1.0
    return n, a, d


def _bits_differ(a, b):
    """Elementwise: not the same bits (any NaN equals any NaN)."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return ~((np.isnan(a) & np.isnan(b)) | (a.view(np.uint64) == b.view(np.uint64)))


def compare_frame(f: dict, o: dict, rays, tag) -> dict:
    """A 1-spp frame f (feats, ids; h x w = the table's order) against the oracle's records o of the same table, every ray.  Rows
    whose record is finite: normal, albedo, depth[0] (= t |d|), depth[1] (= the hit flag) bit for bit, depth[2] == 1, the id equal
    (tied rows included).  Rows whose record holds a NaN or an infinity: the same hit flag, the same id, non-finite values in the
    same fields.  Returns the counts a report line needs."""
    n = len(o["ids"])
    want = expected_planes(o["rec"], n, 1, 1)
    got = [np.asarray(p).reshape(1, n, 3) for p in f["feats"]]
    ids = np.asarray(f["ids"]).reshape(-1)
    nf = o["nonfinite"]
    assert np.all(got[2][0, :, 2] == 1.0), (tag, "samples", np.flatnonzero(got[2][0, :, 2] != 1.0)[:8].tolist())
    bad = np.flatnonzero(got[2][0, :, 1] != o["rec"][:, 0])
    assert len(bad) == 0, (tag, "hit flags differ at rows", bad[:8].tolist(), _hex(rays, bad[:4]))
    bad = np.flatnonzero(ids != o["ids"])
    assert len(bad) == 0, (tag, "ids differ at rows", bad[:8].tolist(), ids[bad[:8]].tolist(), o["ids"][bad[:8]].tolist(), _hex(rays, bad[:4]))
    for name, g, w_ in zip(("normal", "albedo", "depth"), got, want):
        diff = _bits_differ(g[0], w_[0]).any(axis=1)
        bad = np.flatnonzero(diff & ~nf)  # a finite record is never excused
        assert len(bad) == 0, (tag, name, "differs at rows", bad[:8].tolist(), g[0][bad[:4]].tolist(), w_[0][bad[:4]].tolist(), _hex(rays, bad[:4]))
        bad = np.flatnonzero((np.isfinite(g[0]) != np.isfinite(w_[0])).any(axis=1) & nf)
        assert len(bad) == 0, (tag, name, "non-finite fields differ at rows", bad[:8].tolist(), g[0][bad[:4]].tolist(), w_[0][bad[:4]].tolist())
    return dict(rays=n, hits=int(np.count_nonzero(o["rec"][:, 0])), ties=int(np.count_nonzero(o["tie"])), nonfinite=int(np.count_nonzero(nf)))


def planes_differ(got, want) -> list:
    """Per plane, the number of values whose bits differ (any NaN equals any NaN)."""
    return [int(np.count_nonzero(_bits_differ(g, w_))) for g, w_ in zip(got, want)]


def edited_doc(doc: dict, count: int = 40, seed: int = 23):
    """(a copy of doc with `count` of its filler objects -- those after the probes -- moved by up to half a unit per axis and
    resized by a factor in 0.5 .. 1.5 per size component, the indices).  Types and materials stay: a refit takes it."""
    import copy

    rng = np.random.default_rng(seed)
    out = copy.deepcopy(doc)
    idx = np.sort(rng.choice(np.arange(len(S.PROBES), len(doc["objects"])), count, replace=False))
    for i in idx:
        o = out["objects"][int(i)]
        for k in "xyz":
            o["position"][k] = float(o["position"][k] + rng.uniform(-0.5, 0.5))
            o["size"][k] = float(o["size"][k] * rng.uniform(0.5, 1.5))
    return out, [int(i) for i in idx]


def _hex(rays, rows):
    return [[float.hex(float(v)) for v in rays[int(i)]] for i in rows]


def report_line(what, counts: dict, stats: dict) -> str:
    return ("feature walk, injected: %-34s %d rays, %d hits, %d ties, %d non-finite rows, walked %d, plain %d, node visits %d, deepest stack %d"
            % (what, counts["rays"], counts["hits"], counts["ties"], counts["nonfinite"], stats["walked"], stats["plain"],
               stats["node_visits"], stats["deepest_stack"]))


# ---------------------------------------------------------------- the GPU's side
ENV_KEYS = ("PTCORE_SCAN", "PTCORE_SPLIT_ROUNDS", "PTCORE_TAIL", "PTCORE_PIPELINE", "PTCORE_PRIMARY", "PTCORE_DEBUG_DROP")


def context_with(env: dict):
    """A context created with exactly `env` of the variables pt_create reads ({}: the default context)."""
    import os

    from path_trace_golang_amd import capi

    old = {k: os.environ.get(k) for k in ENV_KEYS}
    try:
        for k in ENV_KEYS:
            os.environ.pop(k, None)
        os.environ.update(env)
        return capi.Context(ndev=1)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def render_features(ctx, sc, rays, w=S.W, h=S.H, spp=1, depth=DEPTH, k=1, chunk=0, seed=S.SEED) -> dict:
    """One frame on ctx with `rays` as its primary rays, the feature walk, k feature samples and the object ids on:
    dict(img, feats = (normal, albedo, depth), ids, stats = pt_feature_walk_stats).  The table is cleared before returning."""
    from path_trace_golang_amd import hip

    img, acc, m2 = np.zeros((h, w, 4), np.uint8), np.zeros((h, w, 3)), np.zeros((h, w, 3))
    ctx.set_primary_rays(rays)
    try:
        hip.render(sc, hip.RenderConfig(w, h, spp, depth, seed, chunk), img, None, acc, ctx=ctx, moments=m2, features=k, object_ids=True,
                   feature_walk=True)
    finally:
        ctx.set_primary_rays(None)
    feats = tuple(np.full((h, w, 3), -7.0) for _ in range(3))
    hip.read_features(ctx, *feats)
    ids = np.full((h, w), -9, np.int32)
    hip.read_object_ids(ctx, ids)
    return dict(img=img, feats=feats, ids=ids, stats=hip.feature_walk_stats(ctx))


def assert_walk_stats(stats: dict, waves: int, plain: int, tag) -> None:
    """`waves` (wave, sample) pairs in the frame, `plain` of them holding an odd ray."""
    walked = waves - plain
    assert (stats["plain"], stats["walked"]) == (plain, walked), (tag, stats, plain, walked)
    if walked > 0:
        assert stats["node_visits"] > walked and 1 <= stats["deepest_stack"] < 96, (tag, stats)
