"""B8: whole frames with pt_set_bvh_build at the edges of the device build, 64 x 48 at 4 spp and depth 8, by the bar of
test_bvh_build_gpu.py.  The deepest tree that still fits the traversal stack (bvh_build_support.deep_scene(1): a stack of 89 of 96) is
built on the device and walked; a tree one step too deep (deep_scene(DEEP_TIES)) is built on the device, found too deep and rebuilt
by the host (PT_BVH_BUILD_FALLBACK_STACK), and the context goes on building on the device afterwards; scenes of 1024 and 1025 finite
objects sit on a tile of the sort and the scans.  What the deep scenes are is asserted without a GPU by
test_bvh_build_reference_cpu.py (R3)."""
import numpy as np
import pytest

import bvh_build_reference as ref
import bvh_build_support as bs
import bvh_refit_support as rs
from conftest import render_vs_oracle

pytestmark = pytest.mark.gpu

W, H, SPP, DEPTH = 64, 48, 4, 8


@pytest.fixture(autouse=True, scope="module")
def _built(gpu_ctx):
    return gpu_ctx


def _oracle(oracle, sc, seed=4):
    return oracle.render(oracle.Scene(sc.encode()), W, H, SPP, DEPTH, seed=seed)


def _plain(ctx, sc, seed=4):
    from path_trace_golang_amd import hip

    img, acc = np.zeros((H, W, 4), np.uint8), np.zeros((H, W, 3))
    st = hip.render(sc, hip.RenderConfig(W, H, SPP, DEPTH, seed), img, None, acc, ctx=ctx)
    return img, acc, st


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1], equal_nan=True) and all(
        a[2][k] == b[2][k] for k in ("samples", "segments", "exit_scans", "draws"))


def _reference_figures(sc):
    """(nodes, depth, stack_need) of the scene's two trees by the Python reference."""
    main, glass = ref.build_once(sc.name, bs.scene_world(sc))
    return main["n_nodes"] + glass["n_nodes"], max(main["depth"], glass["depth"]), max(main["stack_need"], glass["stack_need"])


def _stats(ctx):
    from path_trace_golang_amd import hip

    st = hip.bvh_build_stats(ctx)
    return (st["host_builds"], st["device_builds"], st["builder"], st["last_fallback"]), st


def _device_and_host_frames(oracle, sc, tag):
    """`sc` rendered by a device-building context (held to the oracle) and by a host-building one: the same frame, bit for bit."""
    from path_trace_golang_amd import capi, hip

    o = _oracle(oracle, sc)
    with capi.Context(ndev=1) as ctx:
        hip.set_bvh_build(ctx, "device")
        out = render_vs_oracle(ctx, sc, o, W, H, SPP, DEPTH, 4, tag=tag)
        four, st = _stats(ctx)
    with capi.Context(ndev=1) as host:
        frame = _plain(host, sc)
        assert _stats(host)[0] == (1, 0, capi.PT_BVH_BUILDER_HOST, 0)
    img, acc, _, _, stf = out["shipping"]
    assert _same((img, acc, stf), frame), tag
    return four, st


def test_b8_the_deepest_tree_that_fits_is_built_and_walked_on_the_device(oracle):
    from path_trace_golang_amd import capi

    sc = bs.deep_scene(1)
    nodes, depth, need = _reference_figures(sc)
    assert 80 <= need < bs.PT_BVH_STACK
    four, st = _device_and_host_frames(oracle, sc, "deep, fits")
    assert four == (0, 1, capi.PT_BVH_BUILDER_DEVICE, 0), st
    assert (st["nodes"], st["depth"], st["stack_need"]) == (nodes, depth, need)


def test_b8_the_verifying_scan_finds_no_mismatch_on_the_deepest_tree(oracle, monkeypatch):
    from path_trace_golang_amd import capi, hip

    monkeypatch.setenv("PTCORE_SCAN", "verify_bvh")
    sc = bs.deep_scene(1)
    o = _oracle(oracle, sc)
    with capi.Context(ndev=1) as ctx:
        hip.set_bvh_build(ctx, "device")
        before = capi.load().pt_debug_scan_mismatches(ctx.handle)
        img, acc, st = _plain(ctx, sc)
        assert capi.load().pt_debug_scan_mismatches(ctx.handle) == before
        assert hip.bvh_build_stats(ctx)["builder"] == capi.PT_BVH_BUILDER_DEVICE
    assert np.array_equal(img, o["rgba"]) and st["segments"] == o["stats"]["segments"]


def test_b8_a_tree_too_deep_falls_back_to_the_host_and_the_context_goes_on(oracle):
    from path_trace_golang_amd import capi, hip, synth

    deep = bs.deep_scene(bs.DEEP_TIES)
    assert _reference_figures(deep)[2] >= bs.PT_BVH_STACK  # the Morton-order tree does not fit
    plain = synth.make_scene(300, 4)
    o_deep, o_plain = _oracle(oracle, deep), _oracle(oracle, plain, 5)
    fallback = capi.PT_BVH_BUILD_FALLBACK_STACK
    with capi.Context(ndev=1) as ctx:
        hip.set_bvh_build(ctx, "device")
        render_vs_oracle(ctx, deep, o_deep, W, H, SPP, DEPTH, 4, tag="too deep")
        four, st = _stats(ctx)
        assert four == (1, 0, capi.PT_BVH_BUILDER_HOST, fallback), st
        assert 0 < st["stack_need"] < bs.PT_BVH_STACK and st["device_ms"] > 0  # the host's tree is in use; the device did build one
        render_vs_oracle(ctx, plain, o_plain, W, H, SPP, DEPTH, 5, tag="device again", forms=("shipping",))
        four, st = _stats(ctx)
        assert four == (1, 1, capi.PT_BVH_BUILDER_DEVICE, 0), st
        render_vs_oracle(ctx, deep, o_deep, W, H, SPP, DEPTH, 4, tag="too deep again", forms=("shipping",))
        four, st = _stats(ctx)
        assert four == (2, 1, capi.PT_BVH_BUILDER_HOST, fallback), st


@pytest.mark.parametrize("n", [1024, 1025])
def test_b8_scenes_on_a_tile_boundary(oracle, n):
    from path_trace_golang_amd import capi, synth

    sc = synth.make_scene(n, 6)
    assert len(rs.finite_indices(sc)) + 4 == n == len(bs.scene_world(sc)) and sum(o.type == "plane" for o in sc.objects) == 1
    assert len(rs.dielectric_indices(sc)) >= 20
    nodes, depth, need = _reference_figures(sc)
    four, st = _device_and_host_frames(oracle, sc, "n=%d" % n)
    assert four == (0, 1, capi.PT_BVH_BUILDER_DEVICE, 0), st
    assert (st["nodes"], st["depth"], st["stack_need"]) == (nodes, depth, need)
