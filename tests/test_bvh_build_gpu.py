"""B7: whole frames with pt_set_bvh_build, 64 x 48 at 4 spp and depth 8.  A frame rendered on a device-built tree is the
oracle's frame by the bar of test_bvh_gpu.py and, bit for bit, the frame of a context that builds on the host; the verifying scan
finds no mismatch; the stats say who built the tree and why; a refit, the feature walk, the object ids and a second device take the
device-built tree as they take the host's."""
import copy
import math

import numpy as np
import pytest

import atrous_support as at
import bvh_refit_support as rs
from conftest import render_vs_oracle

pytestmark = pytest.mark.gpu

W, H, SPP, DEPTH = 64, 48, 4, 8
_cache = {}


@pytest.fixture(autouse=True, scope="module")
def _built(gpu_ctx):
    return gpu_ctx


def _scene(kind="plain"):
    from path_trace_golang_amd import synth

    if "plain" not in _cache:
        _cache["plain"] = synth.make_scene(300, 4)
    if kind == "glass" and "glass" not in _cache:
        sc = copy.deepcopy(_cache["plain"])
        for i in rs.finite_indices(sc, ("sphere", "box"))[::6]:
            sc.objects[i].material_id = "glass"
        assert len(rs.dielectric_indices(sc)) >= 20
        _cache["glass"] = sc
    return _cache[kind]


def _oracle(oracle, sc, seed=4):
    return oracle.render(oracle.Scene(sc.encode()), W, H, SPP, DEPTH, seed=seed)


def _plain(ctx, sc, seed=4, **kw):
    from path_trace_golang_amd import hip

    img, acc = np.zeros((H, W, 4), np.uint8), np.zeros((H, W, 3))
    st = hip.render(sc, hip.RenderConfig(W, H, SPP, DEPTH, seed), img, None, acc, ctx=ctx, **kw)
    return img, acc, st


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1], equal_nan=True) and all(
        a[2][k] == b[2][k] for k in ("samples", "segments", "exit_scans", "draws"))


@pytest.mark.parametrize("kind", ["plain", "glass"])
def test_b7_a_device_built_frame_is_the_oracles_and_a_host_building_contexts(oracle, kind):
    from path_trace_golang_amd import capi, hip

    sc = _scene(kind)
    o = _oracle(oracle, sc)
    with capi.Context(ndev=1) as ctx:
        hip.set_bvh_build(ctx, "device")
        out = render_vs_oracle(ctx, sc, o, W, H, SPP, DEPTH, 4, tag="device build, " + kind)
        st = hip.bvh_build_stats(ctx)
        assert (st["host_builds"], st["device_builds"], st["builder"], st["last_fallback"]) == (0, 1, capi.PT_BVH_BUILDER_DEVICE, 0), st
        assert st["nodes"] > 0 and st["depth"] > 0 and 0 < st["stack_need"] < 96 and st["cost"] > 0 and st["device_ms"] > 0 and st["prepare_ms"] > 0
        assert st["upload_ms"] > 0 and st["readback_ms"] > 0 and st["prepare_ms"] >= st["upload_ms"] + st["readback_ms"]  # (parts of it)
        chk = hip.bvh_build_check(sc)  # the host restatement builds the same tree
        assert (chk["nodes"], chk["depth"], chk["stack_need"]) == (st["nodes"], st["depth"], st["stack_need"])
        assert (chk["not_reached_once"], chk["objects_outside"], chk["children_outside"], chk["faults"]) == (0, 0, 0, 0)
    with capi.Context(ndev=1) as host:
        ref = _plain(host, sc)
        sth = hip.bvh_build_stats(host)
        assert (sth["host_builds"], sth["device_builds"], sth["builder"], sth["device_ms"], sth["upload_ms"]) == (1, 0, capi.PT_BVH_BUILDER_HOST, 0.0, 0.0)  # never set
    img, acc, _, _, stf = out["shipping"]
    assert _same((img, acc, stf), ref)


def test_b7_the_verifying_scan_finds_no_mismatch(oracle, monkeypatch):
    from path_trace_golang_amd import capi, hip

    monkeypatch.setenv("PTCORE_SCAN", "verify_bvh")
    sc = _scene("glass")
    o = _oracle(oracle, sc)
    with capi.Context(ndev=1) as ctx:
        hip.set_bvh_build(ctx, 1)
        before = capi.load().pt_debug_scan_mismatches(ctx.handle)
        img, acc, st = _plain(ctx, sc)
        assert capi.load().pt_debug_scan_mismatches(ctx.handle) == before
        assert hip.bvh_build_stats(ctx)["builder"] == capi.PT_BVH_BUILDER_DEVICE
    assert np.array_equal(img, o["rgba"]) and st["segments"] == o["stats"]["segments"]


def _edits(sc):
    """A chain of topology edits, each applied to the one before: one object added, 150 added, one removed, a material changed, a
    sphere turned to glass."""
    idx = rs.finite_indices(sc)
    sphere = next(i for i in idx if sc.objects[i].type == "sphere")
    one = copy.deepcopy(sc)
    one.objects.append(copy.deepcopy(sc.objects[sphere]))
    one.objects[-1].id = "one-more"
    one.objects[-1].position.y += 1.0
    yield "one added", one
    many = copy.deepcopy(one)
    rng = np.random.default_rng(9)
    for k in range(150):
        o = copy.deepcopy(sc.objects[idx[k % len(idx)]])
        o.id = "more-%d" % k
        o.position.x += float(rng.uniform(-2, 2))
        o.position.y += float(rng.uniform(0.2, 2))
        o.position.z += float(rng.uniform(-2, 2))
        many.objects.append(o)
    yield "150 added", many
    fewer = copy.deepcopy(many)
    del fewer.objects[idx[5]]
    yield "one removed", fewer
    lambert = next(i for i in rs.finite_indices(fewer) if fewer.objects[i].material_id in ("red", "green", "blue"))
    mat = copy.deepcopy(fewer)
    mat.objects[lambert].material_id = "green" if mat.objects[lambert].material_id != "green" else "red"
    yield "a material changed", mat
    glass = copy.deepcopy(mat)
    s2 = next(i for i in rs.finite_indices(glass) if glass.objects[i].type == "sphere" and glass.objects[i].material_id != "glass")
    glass.objects[s2].material_id = "glass"
    yield "a sphere turned to glass", glass


def test_b7_a_chain_of_topology_edits(oracle):
    from path_trace_golang_amd import capi, hip

    sc = _scene("plain")
    with capi.Context(ndev=1) as ctx:
        hip.set_bvh_build(ctx, "device")
        _plain(ctx, sc)
        for k, (name, edit) in enumerate(_edits(sc)):
            o = _oracle(oracle, edit, 5 + k)
            out = render_vs_oracle(ctx, edit, o, W, H, SPP, DEPTH, 5 + k, tag=name, forms=("shipping",))
            st = hip.bvh_build_stats(ctx)
            assert (st["device_builds"], st["host_builds"], st["builder"]) == (2 + k, 0, capi.PT_BVH_BUILDER_DEVICE), (name, st)
            with capi.Context(ndev=1) as fresh:
                img, acc, _, _, stf = out["shipping"]
                assert _same((img, acc, stf), _plain(fresh, edit, 5 + k)), name
                assert hip.bvh_build_stats(fresh)["device_builds"] == 0


def test_b7_a_refit_keeps_the_device_built_topology(oracle):
    from path_trace_golang_amd import capi, hip

    sc = _scene("glass")
    idx = rs.finite_indices(sc)
    moved = rs.moved_scene(sc, {i: (0.45, 0.2, -0.3) for i in (idx[3], idx[len(idx) // 2], idx[-2])})
    o = _oracle(oracle, moved)
    with capi.Context(ndev=1) as ctx:
        hip.set_bvh_build(ctx, "device")
        hip.set_bvh_refit(ctx, math.inf)
        _plain(ctx, sc)
        built = hip.bvh_build_stats(ctx)
        render_vs_oracle(ctx, moved, o, W, H, SPP, DEPTH, 4, tag="refit of a device-built tree", forms=("shipping",))
        rst, st = hip.bvh_refit_stats(ctx), hip.bvh_build_stats(ctx)
        assert (rst["builds"], rst["refits"]) == (1, 1) and rst["refit_ms"] > 0
        assert rst["cost_built"] == built["cost"] > 0 and rst["cost_now"] > 0  # the base figure is the device-built tree's
        assert (st["device_builds"], st["host_builds"], st["builder"]) == (1, 0, capi.PT_BVH_BUILDER_DEVICE)
    with capi.Context(ndev=1) as host:  # a host-built tree of the same scene has another figure: the trees differ
        hip.set_bvh_refit(host, math.inf)
        _plain(host, sc)
        assert hip.bvh_refit_stats(host)["cost_built"] != built["cost"]


def test_b7_an_outgrown_tree_is_rebuilt_by_the_selected_builder(oracle):
    from path_trace_golang_amd import capi, hip

    sc = _scene("plain")
    tele = rs.teleported(sc)
    o = _oracle(oracle, tele)
    with capi.Context(ndev=1) as ctx:
        hip.set_bvh_build(ctx, "device")
        hip.set_bvh_refit(ctx, 1.5)
        _plain(ctx, sc)
        _plain(ctx, tele)
        rst = hip.bvh_refit_stats(ctx)
        assert rst["refits"] == 1 and rst["cost_now"] / rst["cost_built"] > 1.5
        render_vs_oracle(ctx, tele, o, W, H, SPP, DEPTH, 4, tag="rebuilt", forms=("shipping",))
        rst, st = hip.bvh_refit_stats(ctx), hip.bvh_build_stats(ctx)
        assert (rst["builds"], rst["last_build_reason"]) == (2, capi.PT_BVH_REASON_GROWTH)
        assert (st["device_builds"], st["host_builds"]) == (2, 0)


def test_b7_features_and_object_ids_on_a_device_built_tree():
    from path_trace_golang_amd import capi, hip

    sc = _scene("glass")

    def run(mode):
        with capi.Context(ndev=1) as ctx:
            hip.set_bvh_build(ctx, mode)
            img, acc, m2 = np.zeros((H, W, 4), np.uint8), np.zeros((H, W, 3)), np.zeros((H, W, 3))
            hip.render(sc, hip.RenderConfig(W, H, SPP, DEPTH, 7), img, None, acc, ctx=ctx, moments=m2, features=4, object_ids=True,
                       feature_walk=True)
            feats = tuple(np.zeros((H, W, 3)) for _ in range(3))
            hip.read_features(ctx, *feats)
            ids = np.zeros((H, W), np.int32)
            hip.read_object_ids(ctx, ids)
            return img, acc, m2, feats, ids, hip.bvh_build_stats(ctx)["builder"]

    a, b = run("device"), run("host")
    assert (a[5], b[5]) == (2, 1)
    assert np.array_equal(a[0], b[0]) and at.same_bits(a[1], b[1]) and at.same_bits(a[2], b[2])
    assert all(at.same_bits(x, y) for x, y in zip(a[3], b[3])) and np.array_equal(a[4], b[4])
    assert (a[4] >= 0).any()


def test_b7_two_virtual_devices_render_with_the_tree_the_first_built():
    from path_trace_golang_amd import capi, hip

    sc = _scene("glass")
    outs = []
    for devs in ([0], [0, 0]):
        with capi.Context(devices=devs) as ctx:
            hip.set_bvh_build(ctx, "device")
            w, h = 96, 64
            img, acc = np.zeros((h, w, 4), np.uint8), np.zeros((h, w, 3))
            st = hip.render(sc, hip.RenderConfig(w, h, 2, DEPTH, 2), img, None, acc, ctx=ctx)
            bst = hip.bvh_build_stats(ctx)
            assert (bst["device_builds"], bst["host_builds"]) == (1, 0)
            outs.append((img, acc, st["segments"], bst["nodes"], bst["cost"]))
    a, b = outs
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1], equal_nan=True) and a[2:] == b[2:]


def test_b7_walk32_falls_back_to_the_host_builder(oracle, monkeypatch):
    from path_trace_golang_amd import capi, hip

    monkeypatch.setenv("PTCORE_PIPELINE", "walk32")
    sc = _scene("plain")
    o = _oracle(oracle, sc)
    with capi.Context(ndev=1) as ctx:
        hip.set_bvh_build(ctx, "device")
        render_vs_oracle(ctx, sc, o, W, H, SPP, DEPTH, 4, tag="walk32", forms=("shipping",))
        st = hip.bvh_build_stats(ctx)
        assert (st["host_builds"], st["device_builds"], st["builder"], st["last_fallback"]) == (
            1, 0, capi.PT_BVH_BUILDER_HOST, capi.PT_BVH_BUILD_FALLBACK_WALK32)


def test_b7_mode_rules_and_mode_0_after_mode_1():
    from path_trace_golang_amd import capi, hip, synth

    sc = _scene("plain")
    with capi.Context(ndev=1) as ctx:
        with pytest.raises(capi.PtError) as e:
            hip.bvh_build_stats(ctx)
        assert e.value.code == capi.PT_ERR_STATE
        L = capi.load()
        for bad in (-1, 2, 7):
            assert L.pt_set_bvh_build(ctx.handle, bad) == capi.PT_ERR_INVALID
        hip.set_bvh_build(ctx, "device")
        small = hip.FlatScene(synth.make_scene(40, 4))
        cfg = hip.pt_config(hip.RenderConfig(32, 32, 1, 2, 1))
        capi.check(L.pt_begin(ctx.handle, capi.C.byref(small.c), capi.C.byref(cfg)))
        assert L.pt_set_bvh_build(ctx.handle, 0) == capi.PT_ERR_STATE
        capi.check(L.pt_end(ctx.handle, capi.C.byref(capi.PtStats())))
        st = hip.bvh_build_stats(ctx)  # a small scene: no tree at all
        assert (st["host_builds"], st["device_builds"], st["builder"], st["last_fallback"]) == (0, 0, 0, capi.PT_BVH_BUILD_FALLBACK_NOT_BVH)
        _plain(ctx, sc)
        assert hip.bvh_build_stats(ctx)["device_builds"] == 1
        hip.set_bvh_build(ctx, "host")
        name, edit = next(_edits(sc))
        _plain(ctx, edit)
        st = hip.bvh_build_stats(ctx)
        assert (st["host_builds"], st["device_builds"], st["builder"], st["last_fallback"]) == (1, 1, capi.PT_BVH_BUILDER_HOST, 0)
