"""T6 - T10: whole frames with pt_set_bvh_refit, at the sizes of test_bvh_gpu.py.  A frame rendered on a refitted tree
is the oracle's frame of the moved scene and, bit for bit, the frame of a context that rebuilds; the stats say what was built and
what was refitted and why; a tree that degrades past the bound serves one frame; every edit that is no move builds in full."""
import copy
import math

import numpy as np
import pytest

import atrous_support as at
import bvh_refit_support as rs
import temporal_support as ts
from conftest import render_vs_oracle

pytestmark = pytest.mark.gpu

INF = math.inf
_cache = {}


@pytest.fixture(autouse=True, scope="module")
def _built(gpu_ctx):
    return gpu_ctx


def _scene(n, seed=4):
    from path_trace_golang_amd import synth

    if (n, seed) not in _cache:
        _cache[(n, seed)] = synth.make_scene(n, seed)
    return _cache[(n, seed)]


def _oracle(oracle, sc, w, h, spp, depth, seed):
    return oracle.render(oracle.Scene(sc.encode()), w, h, spp, depth, seed=seed)


def _plain(ctx, sc, w, h, spp, depth, seed):
    from path_trace_golang_amd import hip

    img, acc = np.zeros((h, w, 4), np.uint8), np.zeros((h, w, 3))
    st = hip.render(sc, hip.RenderConfig(w, h, spp, depth, seed), img, None, acc, ctx=ctx)
    return img, acc, st


def _drag(sc, step, count=3):
    """sc with `count` of its free objects (spheres and boxes among them) moved by `step` x a small offset each."""
    idx = rs.finite_indices(sc)
    pick = [idx[3], idx[len(idx) // 2], idx[-2]][:count]
    return rs.moved_scene(sc, {i: (0.45 * step, 0.2 * step, -0.3 * step) for i in pick})


# ---------------------------------------------------------------- T6
@pytest.mark.parametrize("n,w,h,spp,depth", [(300, 64, 48, 4, 6), (3000, 48, 32, 2, 5)])
def test_t6_a_refitted_frame_is_the_oracles_and_a_rebuilding_contexts(oracle, n, w, h, spp, depth):
    from path_trace_golang_amd import capi, hip

    sc = _scene(n)
    moved = _drag(sc, 1.0)
    o = _oracle(oracle, moved, w, h, spp, depth, 4)
    with capi.Context(ndev=1) as ctx:
        hip.set_bvh_refit(ctx, INF)
        _plain(ctx, sc, w, h, spp, depth, 4)
        st0 = hip.bvh_refit_stats(ctx)
        assert (st0["builds"], st0["refits"], st0["last_action"], st0["last_build_reason"]) == (1, 0, 1, capi.PT_BVH_REASON_FIRST)
        assert st0["cost_built"] > 0 and st0["cost_now"] == st0["cost_built"]
        out = render_vs_oracle(ctx, moved, o, w, h, spp, depth, 4, tag="refit, %d objects" % n)
        st = hip.bvh_refit_stats(ctx)
        assert (st["builds"], st["refits"]) == (1, 1) and st["last_action"] == 0  # (the second of the two builds of the kernels: unchanged)
        assert st["cost_now"] > 0 and st["refit_ms"] > 0
        # the figure is the host restatement's
        r = hip.bvh_refit_check(sc, moved)
        assert r["reason"] == 0 and abs(st["cost_now"] / st["cost_built"] * 1000 - r["cost_ratio_x1000"]) <= 1
    with capi.Context(ndev=1) as fresh:
        img, acc, _ = _plain(fresh, moved, w, h, spp, depth, 4)
        stf = hip.bvh_refit_stats(fresh)
        assert (stf["builds"], stf["refits"], stf["last_build_reason"]) == (1, 0, capi.PT_BVH_REASON_FIRST)
    assert np.array_equal(out["shipping"][0], img) and np.array_equal(out["shipping"][1], acc, equal_nan=True)


def test_t6_a_six_frame_drag(oracle):
    from path_trace_golang_amd import capi, hip

    sc = _scene(300)
    w, h, spp, depth = 64, 48, 4, 6
    with capi.Context(ndev=1) as ctx, capi.Context(ndev=1) as off:
        hip.set_bvh_refit(ctx, INF)
        for f in range(6):
            cur = _drag(sc, float(f))
            a = _plain(ctx, cur, w, h, spp, depth, 10 + f)
            b = _plain(off, cur, w, h, spp, depth, 10 + f)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1], equal_nan=True), f
            for k in ("samples", "segments", "exit_scans", "draws"):
                assert a[2][k] == b[2][k], (f, k)
            if f in (1, 5):
                o = _oracle(oracle, cur, w, h, spp, depth, 10 + f)
                assert np.array_equal(a[0], o["rgba"]) and a[2]["segments"] == o["stats"]["segments"], f
        st, sto = hip.bvh_refit_stats(ctx), hip.bvh_refit_stats(off)
        assert (st["builds"], st["refits"], st["last_action"]) == (1, 5, 2)
        assert (sto["builds"], sto["refits"], sto["last_build_reason"]) == (6, 0, capi.PT_BVH_REASON_OFF)


def test_t6_the_verifying_scan_finds_no_mismatch_on_a_refitted_tree(oracle, monkeypatch):
    from path_trace_golang_amd import capi, hip

    monkeypatch.setenv("PTCORE_SCAN", "verify_bvh")
    sc = _scene(300)
    moved = _drag(sc, 1.0)
    w, h, spp, depth = 64, 48, 4, 6
    o = _oracle(oracle, moved, w, h, spp, depth, 4)
    with capi.Context(ndev=1) as ctx:
        hip.set_bvh_refit(ctx, INF)
        _plain(ctx, sc, w, h, spp, depth, 4)
        before = capi.load().pt_debug_scan_mismatches(ctx.handle)
        img, acc, st = _plain(ctx, moved, w, h, spp, depth, 4)
        assert capi.load().pt_debug_scan_mismatches(ctx.handle) == before
        assert hip.bvh_refit_stats(ctx)["refits"] == 1
    assert np.array_equal(img, o["rgba"]) and st["segments"] == o["stats"]["segments"]


# ---------------------------------------------------------------- T7
def test_t7_a_tree_degraded_past_the_bound_serves_one_frame(oracle):
    from path_trace_golang_amd import capi, hip

    sc = _scene(300, 3)
    tele = rs.teleported(sc)
    w, h, spp, depth = 64, 48, 4, 6
    o = _oracle(oracle, tele, w, h, spp, depth, 4)
    with capi.Context(ndev=1) as ctx:
        hip.set_bvh_refit(ctx, 1.5)
        _plain(ctx, sc, w, h, spp, depth, 4)
        render_vs_oracle(ctx, tele, o, w, h, spp, depth, 4, tag="teleport", forms=("shipping",))
        st = hip.bvh_refit_stats(ctx)
        assert (st["builds"], st["refits"], st["last_action"]) == (1, 1, 2)
        assert st["cost_now"] / st["cost_built"] > 1.5
        render_vs_oracle(ctx, tele, o, w, h, spp, depth, 4, tag="rebuilt", forms=("shipping",))
        st = hip.bvh_refit_stats(ctx)
        assert (st["builds"], st["refits"], st["last_action"], st["last_build_reason"]) == (2, 1, 1, capi.PT_BVH_REASON_GROWTH)
        assert st["cost_now"] == st["cost_built"]
        render_vs_oracle(ctx, tele, o, w, h, spp, depth, 4, tag="settled", forms=("shipping",))
        assert hip.bvh_refit_stats(ctx)["builds"] == 2 and hip.bvh_refit_stats(ctx)["last_action"] == 0
    with capi.Context(ndev=1) as ctx:
        hip.set_bvh_refit(ctx, INF)
        _plain(ctx, sc, w, h, spp, depth, 4)
        for tag in ("teleport", "again"):
            render_vs_oracle(ctx, tele, o, w, h, spp, depth, 4, tag=tag, forms=("shipping",))
        st = hip.bvh_refit_stats(ctx)
        assert (st["builds"], st["refits"]) == (1, 1) and st["cost_now"] / st["cost_built"] > 1.5


# ---------------------------------------------------------------- T8
def test_t8_edits_that_are_no_moves_build_in_full(oracle):
    from path_trace_golang_amd import capi, hip

    sc = _scene(300)
    idx = rs.finite_indices(sc)
    sphere = next(i for i in idx if sc.objects[i].type == "sphere")
    lambert = next(i for i in idx if sc.objects[i].material_id in ("red", "green", "blue"))
    kind = copy.deepcopy(sc)
    kind.objects[sphere].type = "box"
    kind.objects[sphere].size.y = kind.objects[sphere].size.z = kind.objects[sphere].size.x
    swap = copy.deepcopy(sc)
    swap.objects[lambert].material_id = "glass"
    more = copy.deepcopy(sc)
    more.objects.append(copy.deepcopy(sc.objects[sphere]))
    more.objects[-1].id = "one-more"
    more.objects[-1].position.y += 1.0
    huge = copy.deepcopy(sc)
    huge.objects[sphere].position.x = 1e38
    w, h, spp, depth = 64, 48, 4, 6
    edits = (("kind", kind, capi.PT_BVH_REASON_CHANGED), ("material", swap, capi.PT_BVH_REASON_CHANGED),
             ("one more", more, capi.PT_BVH_REASON_CHANGED), ("1e38", huge, capi.PT_BVH_REASON_NONFINITE))
    with capi.Context(ndev=1) as ctx, capi.Context(ndev=1) as off:
        hip.set_bvh_refit(ctx, INF)
        for k, (name, edit, reason) in enumerate(edits):
            _plain(ctx, sc, w, h, spp, depth, 4)
            _plain(off, sc, w, h, spp, depth, 4)
            o = _oracle(oracle, edit, w, h, spp, depth, 4)
            render_vs_oracle(ctx, edit, o, w, h, spp, depth, 4, tag=name, forms=("shipping",))
            st = hip.bvh_refit_stats(ctx)
            assert (st["refits"], st["last_action"], st["last_build_reason"]) == (0, 1, reason), (name, st)
            assert st["builds"] == 2 * (k + 1), (name, st)
            _plain(off, edit, w, h, spp, depth, 4)
        sto = hip.bvh_refit_stats(off)
        assert (sto["builds"], sto["refits"]) == (2 * len(edits), 0)  # every frame of `off` changed the scene


def test_setting_rules():
    from path_trace_golang_amd import capi, hip

    with capi.Context(ndev=1) as ctx:
        with pytest.raises(capi.PtError) as e:
            hip.bvh_refit_stats(ctx)
        assert e.value.code == capi.PT_ERR_STATE
        for bad in (math.nan, -1.0, 0.5, 0.999):
            with pytest.raises(capi.PtError) as e:
                hip.set_bvh_refit(ctx, bad)
            assert e.value.code == capi.PT_ERR_INVALID, bad
        for good in (1.0, 2.0, INF, 0.0):
            hip.set_bvh_refit(ctx, good)
        L = capi.load()
        sc = hip.FlatScene(_scene(40))
        cfg = hip.pt_config(hip.RenderConfig(32, 32, 1, 2, 1))
        capi.check(L.pt_begin(ctx.handle, capi.C.byref(sc.c), capi.C.byref(cfg)))
        assert L.pt_set_bvh_refit(ctx.handle, 2.0) == capi.PT_ERR_STATE
        capi.check(L.pt_end(ctx.handle, capi.C.byref(capi.PtStats())))
        st = hip.bvh_refit_stats(ctx)  # a small scene: not on the hierarchy path, a build with the feature off
        assert (st["builds"], st["refits"], st["last_build_reason"]) == (1, 0, capi.PT_BVH_REASON_FIRST)


# ---------------------------------------------------------------- T9
def test_t9_two_virtual_devices_refit_their_own_copies():
    from path_trace_golang_amd import capi, hip

    sc = _scene(300)
    moved = _drag(sc, 1.0)
    w, h, spp, depth = 96, 64, 2, 6
    outs = []
    for devs in ([0], [0, 0]):
        with capi.Context(devices=devs) as ctx:
            hip.set_bvh_refit(ctx, INF)
            _plain(ctx, sc, w, h, spp, depth, 2)
            img, acc, st = _plain(ctx, moved, w, h, spp, depth, 2)
            rst = hip.bvh_refit_stats(ctx)
            assert (rst["builds"], rst["refits"]) == (1, 1)
            outs.append((img, acc, st["segments"], rst["cost_now"], rst["cost_built"]))
    a, b = outs
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1], equal_nan=True) and a[2:] == b[2:]


# ---------------------------------------------------------------- T10
def test_t10_features_ids_and_the_accumulated_frame_on_a_refitted_tree():
    from path_trace_golang_amd import capi, hip

    sc = _scene(300)
    idx = rs.finite_indices(sc)
    sphere = next(i for i in idx if sc.objects[i].type == "sphere")
    box = next(i for i in idx if sc.objects[i].type == "box")
    w, h, spp, depth = 64, 48, 4, 4
    tcfg, flt = ts.temporal_config(), at.atrous_config()

    def run(refit):
        frames = []
        with capi.Context(ndev=1) as ctx:
            if refit:
                hip.set_bvh_refit(ctx, INF)
            prev = None
            for f in range(3):
                cur = rs.moved_scene(sc, {sphere: (0.3 * f, 0.0, 0.1 * f), box: (-0.2 * f, 0.1 * f, 0.0)})
                img, acc, m2 = np.zeros((h, w, 4), np.uint8), np.zeros((h, w, 3)), np.zeros((h, w, 3))
                delta = hip.scene_motion(prev, cur) if prev is not None else None
                st = hip.render(cur, hip.RenderConfig(w, h, spp, depth, 20 + f), img, None, acc, ctx=ctx, moments=m2, features=4,
                                object_ids=True, feature_walk=True, atrous=flt, temporal=tcfg, temporal_motion=delta)
                feats = tuple(np.zeros((h, w, 3)) for _ in range(3))
                hip.read_features(ctx, *feats)
                ids = np.zeros((h, w), np.int32)
                hip.read_object_ids(ctx, ids)
                hm, hv, hl = np.zeros((h, w, 3)), np.zeros((h, w)), np.zeros((h, w), np.int32)
                hip.temporal_read(ctx, hm, hv, hl)
                frames.append(dict(img=img, acc=acc, m2=m2, feats=feats, ids=ids, hist=(hm, hv, hl), t=st["temporal"]))
                prev = cur
            rst = hip.bvh_refit_stats(ctx)
        return frames, rst

    on, rst_on = run(True)
    off, rst_off = run(False)
    assert (rst_on["builds"], rst_on["refits"]) == (1, 2) and (rst_off["builds"], rst_off["refits"]) == (3, 0)
    assert on[2]["t"]["moved"] > 0  # the dragged objects are in view
    for f, (a, b) in enumerate(zip(on, off)):
        assert np.array_equal(a["img"], b["img"]) and at.same_bits(a["acc"], b["acc"]) and at.same_bits(a["m2"], b["m2"]), f
        assert all(at.same_bits(x, y) for x, y in zip(a["feats"], b["feats"])) and np.array_equal(a["ids"], b["ids"]), f
        assert at.same_bits(a["hist"][0], b["hist"][0]) and at.same_bits(a["hist"][1], b["hist"][1]) and np.array_equal(a["hist"][2], b["hist"][2]), f
        ta, tb = dict(a["t"]), dict(b["t"])
        ta.pop("temporal_ms"), tb.pop("temporal_ms")
        assert ta == tb, (f, ta, tb)
