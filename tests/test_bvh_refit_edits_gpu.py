"""Whole frames on a tree refitted after edits that are no translations: ptbvh::refit_reason accepts every edit that keeps
each object's kind and material and every coordinate below 1e37, so resized spheres and boxes, negative and zero radii, a moved plane
and moved and resized dielectrics (the second tree, the one the exit search walks) all keep the tree of the last full build -- with the
scan choice, the LDS plan and has_glass of that build, new radius_sq / inv_radius in the records the device copies, and new plane
fields from build_broad.  For every edit of rs.edited_scenes, at the sizes of T6: the refitted frame is the oracle's and, bit for bit, a
fresh context's; the verifying scan counts no mismatch; a chain of all edits in one context equals a rebuilding context frame by frame."""
import math

import numpy as np
import pytest

import atrous_support as at
import bvh_refit_support as rs
from conftest import render_vs_oracle

pytestmark = pytest.mark.gpu

INF = math.inf
N, SEED = 300, 4
W, H, SPP, DEPTH = 64, 48, 4, 6
_cache = {}


@pytest.fixture(autouse=True, scope="module")
def _built(gpu_ctx):
    return gpu_ctx


def _base():
    from path_trace_golang_amd import synth

    if "sc" not in _cache:
        _cache["sc"] = synth.make_scene(N, SEED)
        _cache["edits"] = dict(rs.edited_scenes(_cache["sc"]))
        assert tuple(_cache["edits"]) == rs.EDITS
    return _cache["sc"]


def _edit(name):
    _base()
    return _cache["edits"][name]


def _oracle(oracle, name, seed=SEED):
    """The oracle's frame of an edit (None: the scene itself).  Computed once."""
    key = ("oracle", name, seed)
    if key not in _cache:
        sc = _base() if name is None else _edit(name)
        _cache[key] = oracle.render(oracle.Scene(sc.encode()), W, H, SPP, DEPTH, seed=seed)
    return _cache[key]


def _plain(ctx, sc, seed=SEED):
    from path_trace_golang_amd import hip

    img, acc = np.zeros((H, W, 4), np.uint8), np.zeros((H, W, 3))
    st = hip.render(sc, hip.RenderConfig(W, H, SPP, DEPTH, seed), img, None, acc, ctx=ctx)
    return img, acc, st


def _same(a, b):
    return (np.array_equal(a[0], b[0]) and at.same_bits(a[1], b[1])
            and all(a[2][k] == b[2][k] for k in ("samples", "segments", "exit_scans", "draws")))


@pytest.mark.parametrize("name", rs.EDITS)
def test_a_frame_refitted_after_the_edit_is_the_oracles_and_a_fresh_contexts(oracle, name):
    from path_trace_golang_amd import capi, hip

    sc, edit = _base(), _edit(name)
    o = _oracle(oracle, name)
    with capi.Context(ndev=1) as ctx:
        hip.set_bvh_refit(ctx, INF)
        _plain(ctx, sc)
        st0 = hip.bvh_refit_stats(ctx)
        assert (st0["builds"], st0["refits"], st0["last_build_reason"]) == (1, 0, capi.PT_BVH_REASON_FIRST)
        out = render_vs_oracle(ctx, edit, o, W, H, SPP, DEPTH, SEED, tag="refit, " + name)
        st = hip.bvh_refit_stats(ctx)
        assert (st["builds"], st["refits"]) == (1, 1) and st["refit_ms"] > 0, (name, st)
        r = hip.bvh_refit_check(sc, edit)  # the figure is the host restatement's
        assert r["reason"] == 0 and abs(st["cost_now"] / st["cost_built"] * 1000 - r["cost_ratio_x1000"]) <= 1, (name, st, r)
    with capi.Context(ndev=1) as fresh:
        img, acc, stf = _plain(fresh, edit)
        rf = hip.bvh_refit_stats(fresh)
        assert (rf["builds"], rf["refits"]) == (1, 0)
    got = out["shipping"]
    assert np.array_equal(got[0], img) and at.same_bits(got[1], acc), (name, int(np.count_nonzero(got[1] != acc)))
    for k in ("samples", "segments", "exit_scans", "draws"):
        assert got[4][k] == stf[k], (name, k)
    base = _oracle(oracle, None)
    assert not np.array_equal(o["rgba"], base["rgba"]), name  # the edit is in view
    if name == rs.DIELECTRIC_EDIT:  # the second tree was refitted and walked
        assert o["stats"]["exit_scans"] > 0 and o["stats"]["exit_scans"] != base["stats"]["exit_scans"]
    print("refit after an edit: %-28s %d rays, %d segments, %d exit scans (unedited: %d, %d), figure ratio x1000 %d, refit %.3f ms"
          % (name, W * H * SPP, o["stats"]["segments"], o["stats"]["exit_scans"], base["stats"]["segments"], base["stats"]["exit_scans"],
             r["cost_ratio_x1000"], st["refit_ms"]))


def test_the_verifying_scan_finds_no_mismatch_after_any_edit(oracle, monkeypatch):
    from path_trace_golang_amd import capi, hip

    monkeypatch.setenv("PTCORE_SCAN", "verify_bvh")  # read by pt_create
    sc = _base()
    L = capi.load()
    with capi.Context(ndev=1) as ctx:
        hip.set_bvh_refit(ctx, INF)
        for k, name in enumerate(rs.EDITS):
            _plain(ctx, sc)
            before = L.pt_debug_scan_mismatches(ctx.handle)
            img, acc, st = _plain(ctx, _edit(name))
            delta = L.pt_debug_scan_mismatches(ctx.handle) - before
            o = _oracle(oracle, name)
            assert delta == 0, (name, delta)
            assert np.array_equal(img, o["rgba"]) and st["segments"] == o["stats"]["segments"] and st["exit_scans"] == o["stats"]["exit_scans"], name
            rst = hip.bvh_refit_stats(ctx)
            assert (rst["builds"], rst["refits"]) == (1, 2 * k + 1), (name, rst)  # the edit, and back to sc before the next one
            print("refit after an edit, verify_bvh: %-28s scan-mismatch delta %d" % (name, delta))


def test_a_chain_of_every_edit_equals_a_rebuilding_context_frame_by_frame(oracle):
    from path_trace_golang_amd import capi, hip

    sc = _base()
    chain = [(None, sc)] + [(name, _edit(name)) for name in rs.EDITS] + [(None, sc)]
    with capi.Context(ndev=1) as ctx, capi.Context(ndev=1) as off:
        hip.set_bvh_refit(ctx, INF)
        frames = []
        for k, (name, cur) in enumerate(chain):
            a, b = _plain(ctx, cur), _plain(off, cur)
            assert _same(a, b), (k, name)
            o = _oracle(oracle, name)
            assert np.array_equal(a[0], o["rgba"]) and a[2]["segments"] == o["stats"]["segments"], (k, name)
            frames.append(a)
        assert _same(frames[-1], frames[0])  # back at sc: nothing accumulated
        st, sto = hip.bvh_refit_stats(ctx), hip.bvh_refit_stats(off)
        assert (st["builds"], st["refits"]) == (1, len(rs.EDITS) + 1), st
        assert st["cost_now"] == st["cost_built"]
        assert (sto["builds"], sto["refits"]) == (len(chain), 0)


def test_two_virtual_devices_refit_their_own_copies_after_the_dielectric_edit():
    from path_trace_golang_amd import capi, hip

    sc, edit = _base(), _edit(rs.DIELECTRIC_EDIT)
    outs = []
    for devs in ([0], [0, 0]):
        with capi.Context(devices=devs) as ctx:
            hip.set_bvh_refit(ctx, INF)
            _plain(ctx, sc)
            img, acc, st = _plain(ctx, edit)
            rst = hip.bvh_refit_stats(ctx)
            assert (rst["builds"], rst["refits"]) == (1, 1) and st["num_devices"] == len(devs)
            outs.append((img, acc, st["segments"], st["exit_scans"], rst["cost_now"], rst["cost_built"]))
    a, b = outs
    assert np.array_equal(a[0], b[0]) and at.same_bits(a[1], b[1]) and a[2:] == b[2:] and a[3] > 0
