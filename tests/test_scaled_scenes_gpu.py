"""Rescaled scenes through every scan form, against the oracle ray by ray ("Scale of the geometry").

The scenes and ray tables of ray_inject_support.py with every length times 2^k (scaled_scene_support.py; test_scaled_scenes_cpu.py
shows that they reach the geometry at every scale) put B = max(1, largest |coordinate|) on either side of every constant the FP32
bounds rest on: the floor B >= 1, the FP32 squares at 2^64, the 1e30 cut, the 1e37 rule, FLT_MAX.  Per (scene, k):
  G1  the default context, every table in the similar family and (k >= -4) the unit family, held to ora_sample_ray in both builds
  G2  the self-checking context of the scene: pt_debug_scan_mismatches must not move (and does under PTCORE_DEBUG_DROP at k = 60)
  G3  a 64 x 48 frame of the scaled scene's own camera
and on the 341-object scene at the scales of WALKER_K
  G4  the wavefront (sorted), walk32 and PTCORE_PRIMARY=lane forms, a device-built tree, a refitted tree
  G5  the feature walk's records and ids, in both layouts.
Every comparison is the suite's own (injected_vs_oracle, render_vs_oracle, compare_frame); nothing is skipped or widened."""
import math
import os

import numpy as np
import pytest

import feature_inject_support as fi
import ray_inject_support as S
import scaled_scene_support as X
from conftest import render_vs_oracle

pytestmark = pytest.mark.gpu

CASES = [(s, k) for s in X.SCENES for k in X.K]
WALKER_TABLES = ("incoherent", "near geometry")
ENV_KEYS = fi.ENV_KEYS + ("PTCORE_WF_SORT",)
FORMS = {"wavefront, sorted": {"PTCORE_PIPELINE": "wavefront", "PTCORE_WF_SORT": "1"}, "walk32": {"PTCORE_PIPELINE": "walk32"},
         "primary pass off": {"PTCORE_PRIMARY": "lane"}}

_cache = {}


def _context_with(env):
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


@pytest.fixture(scope="module")
def contexts(gpu_ctx):
    out = {"default": gpu_ctx}
    for mode in S.VERIFY_MODE.values():
        out[mode] = _context_with({"PTCORE_SCAN": mode})
    for name, env in FORMS.items():
        out[name] = _context_with(env)
    yield out
    for name, c in out.items():
        if name != "default":
            c.close()


def _scene(scene_name, k, edited=False):
    from path_trace_golang_amd import scene

    key = ("scene", scene_name, k, edited)
    if key not in _cache:
        doc = X.scaled_doc(fi.edited_doc(S.scene_doc(scene_name))[0], k) if edited else X.doc_of(scene_name, k)
        _cache[key] = (doc, scene.Scene.decode(doc))
    return _cache[key]


def _oracle(oracle, scene_name, k, table_name, family, edited=False):
    doc, _ = _scene(scene_name, k, edited)
    return S.oracle_frame(oracle, doc, X.rays_of(table_name, k, family), key=("scaled", scene_name, k, table_name, family, edited))


def _mismatches(ctx):
    from path_trace_golang_amd import capi

    return capi.load().pt_debug_scan_mismatches(ctx.handle)


def _report(oracle, what, scene_name, k, table_name, family, delta="n/a", edited=False):
    doc, _ = _scene(scene_name, k, edited)
    rays = X.rays_of(table_name, k, family)
    key = ("ids", scene_name, k, table_name, family, edited)
    if key not in _cache:
        _cache[key] = S.first_hits(oracle, doc, rays)
    o = _oracle(oracle, scene_name, k, table_name, family, edited)
    print(X.report_line("%s, %s, %s" % (what, table_name, family), scene_name, k, rays, _cache[key], int(o["nseg"].sum()), delta))


def _tables(k, names=X.TABLES):
    return [(t, f) for t in names for f in X.families(k)]


# ---------------------------------------------------------------- G1
@pytest.mark.parametrize("scene_name,k", CASES)
def test_default_context_matches_the_oracle_ray_by_ray(contexts, oracle, scene_name, k):
    _, sc = _scene(scene_name, k)
    for table_name, family in _tables(k):
        o = _oracle(oracle, scene_name, k, table_name, family)
        S.injected_vs_oracle(contexts["default"], sc, o, X.rays_of(table_name, k, family), tag=(scene_name, k, table_name, family))
        _report(oracle, "default", scene_name, k, table_name, family)


# ---------------------------------------------------------------- G2
@pytest.mark.parametrize("scene_name,k", CASES)
def test_verify_contexts_count_nothing(contexts, oracle, scene_name, k):
    """Every scan of every scaled ray by the culled strategy and by the plain loop: no candidate wrongly culled, even where the
    pixel would survive it.  (In the plain-loop band there is no culled strategy: the counter has nothing to count.)"""
    _, sc = _scene(scene_name, k)
    mode = S.VERIFY_MODE[scene_name]
    ctx = contexts[mode]
    start = _mismatches(ctx)
    for table_name, family in _tables(k):
        before = _mismatches(ctx)
        S.injected_vs_oracle(ctx, sc, _oracle(oracle, scene_name, k, table_name, family), X.rays_of(table_name, k, family),
                             tag=(mode, k, table_name, family))
        _report(oracle, mode, scene_name, k, table_name, family, _mismatches(ctx) - before)
    assert _mismatches(ctx) - start == 0, (mode, k, _mismatches(ctx) - start)


def test_the_mismatch_counter_moves_on_a_scaled_scene(oracle):
    """Negative control at k = 60: with the first eight candidate bits of every group cleared (PTCORE_DEBUG_DROP, read when the scene
    is prepared) the checker must count lost hits on the scaled scene too; without the knob it counts nothing."""
    k = 60
    _, sc = _scene("bitmask", k)
    deltas = {}
    for drop in ("0xff", None):
        ctx = _context_with({"PTCORE_SCAN": "verify"})
        old = os.environ.get("PTCORE_DEBUG_DROP")
        try:
            if drop is None:
                os.environ.pop("PTCORE_DEBUG_DROP", None)
            else:
                os.environ["PTCORE_DEBUG_DROP"] = drop
            before = _mismatches(ctx)
            for family in X.FAMILIES:
                S.render_injected(ctx, sc, X.rays_of("incoherent", k, family), stats=False)
            deltas[drop] = _mismatches(ctx) - before
        finally:
            if old is None:
                os.environ.pop("PTCORE_DEBUG_DROP", None)
            else:
                os.environ["PTCORE_DEBUG_DROP"] = old
            ctx.close()
    print("scaled scenes: negative control on bitmask k %d [%s], scan-mismatch deltas with / without PTCORE_DEBUG_DROP=0xff: %d / %d"
          % (k, X.band(k), deltas["0xff"], deltas[None]))
    assert deltas["0xff"] > 0 and deltas[None] == 0, deltas


# ---------------------------------------------------------------- G3
@pytest.mark.parametrize("scene_name,k", CASES)
def test_camera_frame_matches_the_oracle(contexts, oracle, scene_name, k):
    """The scaled scene's own camera: primary rays of the similar family by construction, bounces of unit length from scaled origins."""
    doc, sc = _scene(scene_name, k)
    w, h, spp, depth = 64, 48, 2, 6
    o = oracle.render(oracle.Scene(doc), w, h, spp, depth, seed=S.SEED)
    out = render_vs_oracle(contexts["default"], sc, o, w, h, spp, depth, S.SEED, tag=(scene_name, k))
    hit = int(np.count_nonzero(o["nseg"] > spp))
    print("scaled scenes: camera frame on %-8s k %4d [%s]: %d rays, %d pixels with a bounce, %d non-finite sums, %d segments, %d exit scans"
          % (scene_name, k, X.band(k), w * h * spp, hit, int(np.count_nonzero(~np.isfinite(o["accum"]).all(axis=2))),
             out["shipping"][4]["segments"], out["shipping"][4]["exit_scans"]))
    assert 0 < hit < w * h  # the camera sees the scene and the sky at every scale


# ---------------------------------------------------------------- G4
@pytest.mark.parametrize("k", X.WALKER_K)
@pytest.mark.parametrize("form", list(FORMS))
def test_other_walkers_match_the_same_oracle_output(contexts, oracle, form, k):
    _, sc = _scene("bvh", k)
    for table_name, family in _tables(k, WALKER_TABLES):
        S.injected_vs_oracle(contexts[form], sc, _oracle(oracle, "bvh", k, table_name, family), X.rays_of(table_name, k, family),
                             tag=(form, k, table_name, family))
        _report(oracle, form, "bvh", k, table_name, family)


@pytest.mark.parametrize("k", X.WALKER_K)
def test_device_built_tree_gives_the_host_built_frame(contexts, oracle, k):
    from path_trace_golang_amd import capi, hip

    _, sc = _scene("bvh", k)
    with capi.Context(ndev=1) as ctx:
        hip.set_bvh_build(ctx, 1)
        for table_name, family in _tables(k, WALKER_TABLES):
            rays = X.rays_of(table_name, k, family)
            out = S.injected_vs_oracle(ctx, sc, _oracle(oracle, "bvh", k, table_name, family), rays, tag=("device build", k, table_name, family))
            host = S.render_injected(contexts["default"], sc, rays, stats=False)
            dev = out["shipping"]
            assert np.array_equal(dev[0], host[0]) and dev[1].tobytes() == host[1].tobytes(), (k, table_name, family)
            assert all(dev[4][key] == host[4][key] for key in ("samples", "segments", "exit_scans", "draws")), (k, table_name, family)
            _report(oracle, "device-built tree", "bvh", k, table_name, family)
        st = hip.bvh_build_stats(ctx)
        four = (st["host_builds"], st["device_builds"], st["builder"], st["last_fallback"])
        print("scaled scenes: device build on bvh k %4d [%s]: host builds %d, device builds %d, builder %d, fallback %d, nodes %d, depth %d, stack need %d"
              % ((k, X.band(k)) + four + (st["nodes"], st["depth"], st["stack_need"])))
        if X.band(k) == "plain loop":  # no tree at all: neither builder ran
            assert four == (0, 0, capi.PT_BVH_BUILDER_NONE, capi.PT_BVH_BUILD_FALLBACK_NOT_BVH), st
        else:  # the device built it, or fell back for the reason it states
            assert four == (0, 1, capi.PT_BVH_BUILDER_DEVICE, capi.PT_BVH_BUILD_FALLBACK_NONE) or \
                four == (1, 1, capi.PT_BVH_BUILDER_HOST, capi.PT_BVH_BUILD_FALLBACK_STACK), st
            assert st["nodes"] > 0 and 0 < st["stack_need"]


@pytest.mark.parametrize("k", X.WALKER_K)
def test_refit_of_the_scaled_edited_scene(oracle, k):
    """The scaled scene, then the scaled edit of it (40 objects moved and resized) with the refit on: one build and one refit up to
    k = 119; at k = 120 the edited world is on the plain loop and prepares in full, for the 1e37 rule."""
    from path_trace_golang_amd import capi, hip

    _, sc = _scene("bvh", k)
    edoc, esc = _scene("bvh", k, edited=True)
    assert S.scene_bound(edoc) == max(1.0, X.coordinate(k))  # the edit stays inside the bound: the tables' classification holds
    ctx = fi.context_with({})
    try:
        hip.set_bvh_refit(ctx, math.inf)
        S.render_injected(ctx, sc, X.rays_of("incoherent", k, "similar"), stats=False)
        st = hip.bvh_refit_stats(ctx)
        assert (st["builds"], st["refits"], st["last_build_reason"]) == (1, 0, capi.PT_BVH_REASON_FIRST), st
        for table_name, family in _tables(k, WALKER_TABLES):
            S.injected_vs_oracle(ctx, esc, _oracle(oracle, "bvh", k, table_name, family, edited=True), X.rays_of(table_name, k, family),
                                 tag=("refit", k, table_name, family))
            st = hip.bvh_refit_stats(ctx)
            if X.band(k) == "plain loop":
                assert (st["builds"], st["refits"], st["last_build_reason"]) == (2, 0, capi.PT_BVH_REASON_NONFINITE), st
            else:
                assert (st["builds"], st["refits"]) == (1, 1), st
            _report(oracle, "refitted tree", "bvh", k, table_name, family, edited=True)
        changed = int(np.count_nonzero(_cache[("ids", "bvh", k, "incoherent", "similar", True)] !=
                                       S.first_hits(oracle, _scene("bvh", k)[0], X.rays_of("incoherent", k, "similar"))))
        assert changed > 50, changed  # the edit is seen: rays whose winner is another object than before
    finally:
        ctx.close()


# ---------------------------------------------------------------- G5
def _render_features(ctx, sc, rays):
    """fi.render_features; on the plain loop, where the linear feature pass runs and pt_feature_walk_stats has nothing to report
    (PT_ERR_STATE), the same frame with zero counters."""
    from path_trace_golang_amd import capi, hip

    try:
        return fi.render_features(ctx, sc, rays)
    except capi.PtError as e:
        assert e.code == capi.PT_ERR_STATE and "did not run the walk" in str(e), e
    feats = tuple(np.full((S.H, S.W, 3), -7.0) for _ in range(3))
    hip.read_features(ctx, *feats)
    ids = np.full((S.H, S.W), -9, np.int32)
    hip.read_object_ids(ctx, ids)
    return dict(feats=feats, ids=ids, stats=dict(walked=0, plain=0, node_visits=0, deepest_stack=0))


@pytest.mark.parametrize("k", X.WALKER_K)
def test_feature_walk_records_match_the_oracle(oracle, k):
    """Normal, albedo, distance, hit flag and id of every scaled ray, bit for bit against tests/atrous_reference.c and
    tests/object_ids_reference.c, in the tables' own layout and in the walk's.  The split between walked and plain waves is what
    walk_odd says with the bound as it is at that scale (infinite in the keep-all band, where 0.99 origin_bound is what is left);
    on the plain loop (k = 120) there is no tree to walk and the split is only reported."""
    doc, sc = _scene("bvh", k)
    osc = fi.ora_scene(doc, key=("scaled", "bvh", k))
    ctx = fi.context_with({})
    try:
        for table_name, family in _tables(k):
            for layout, (table, plain) in X.walk_layouts(X.rays_of(table_name, k, family), k).items():
                tag = (k, table_name, family, layout)
                o = fi.oracle_records(osc, table)
                f = _render_features(ctx, sc, table)
                counts = fi.compare_frame(f, o, table, tag)
                print("scaled scenes: " + fi.report_line("bvh k %d [%s] %s, %s, %s layout (predicted plain %d)" % (k, X.band(k), table_name, family, layout, plain),
                                                         counts, f["stats"]))
                if X.band(k) != "plain loop":
                    fi.assert_walk_stats(f["stats"], S.NWAVES, plain, tag)
                    # a NaN or an infinity excuses odd rows only: no ray the walk took
                    assert not np.any(o["nonfinite"] & ~X.walk_odd(table, k)), tag
                assert 0 < counts["hits"] < counts["rays"], tag
    finally:
        ctx.close()
