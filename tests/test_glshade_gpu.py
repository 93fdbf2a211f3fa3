"""GL shading on the MI355X (pt_set_shading, gl_trace_kernel): whole-frame parity with the independent CPU restatement
tests/glshade_reference.c on the shipped and synthetic scenes (also with gpu_showcase's fog block), invariance to chunking,
progressive steps, shards and device count, the GL finish, that off is off, and the refusals.  Every test uses contexts of
its own, so the shared session context never carries a shading model."""
from __future__ import annotations

import ctypes as C
import json

import numpy as np
import pytest

import glshade_support as gs
from conftest import render_vs_oracle, scene_path

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, scope="module")
def _torch_before_libptcore():
    # the shard test hands torch device memory to the C ABI: torch's HIP runtime must be loaded before libptcore.so
    import torch  # noqa: F401


W, H, PASSES, DEPTH, SEED = 40, 24, 2, 8, 11  # 40 x 24: ragged 32 x 32 tiles
SHIPPED = ["example_simple", "gpu_showcase", "metal_glass_room", "test_comprehensive", "test_scene"]


def _close(acc, ref, depth=DEPTH):  # the fog tests' bar
    rel = np.abs(acc - ref) / np.maximum(np.abs(ref), 1e-300)
    return float(np.max(rel)) <= 4 * depth * 2.0 ** -52


def _shipped(name):
    from oracle import ora
    from path_trace_golang_amd import scene

    with open(scene_path(name)) as f:
        doc = json.load(f)
    return scene.load(scene_path(name)), ora.Scene(doc)


def _render(ctx, sc, w=W, h=H, passes=PASSES, depth=DEPTH, seed=SEED, chunk=0, flags=0, fog=False):
    from path_trace_golang_amd import hip

    img = np.zeros((h, w, 4), np.uint8)
    acc = np.zeros((h, w, 3))
    st = hip.render(sc, hip.RenderConfig(w, h, passes, depth, seed, chunk, flags), img, None, acc, ctx=ctx, fog=fog, shading="gl")
    return img, acc, st, hip.shading_last_stats(ctx)


def _check(tag, sc, o, w=W, h=H, passes=PASSES, depth=DEPTH, fog=False):
    from path_trace_golang_amd import capi, hip

    ref_img, ref_acc, ref_st = gs.reference_render(o, gs.extras(sc), w, h, passes, depth, SEED,
                                                   hip.pt_fog(sc.fog) if fog else None)
    with capi.Context(ndev=1) as ctx:
        img, acc, st, gst = _render(ctx, sc, w, h, passes, depth, fog=fog)
        fst = hip.fog_last_stats(ctx)
    assert np.array_equal(img, ref_img), (tag, int(np.count_nonzero(img != ref_img)))
    assert _close(acc, ref_acc, depth), tag
    bit_equal = np.array_equal(acc.view(np.uint64), ref_acc.view(np.uint64))
    print("%s: accum bit-equal to the restatement: %s" % (tag, bit_equal))
    assert (gst["paths"], gst["segments"], gst["shadow_rays"], gst["probe_rays"], gst["draws"]) == \
        (ref_st["paths"], ref_st["segments"], ref_st["shadow_rays"], ref_st["probe_rays"], ref_st["draws"]), tag
    assert (st["samples"], st["segments"], st["draws"]) == (ref_st["paths"], ref_st["segments"], ref_st["draws"])
    assert gst["gl_launches"] >= 1 and gst["gl_ms"] > 0 and st["trace_ms"] == pytest.approx(gst["gl_ms"])
    if fog:
        assert (fst["shadow_rays"], fst["draws"], fst["steps"]) == \
            (ref_st["fog_shadow_rays"], ref_st["fog_draws"], ref_st["fog_steps"]) and ref_st["fog_steps"] > 0
    return img, acc


@pytest.mark.parametrize("name", SHIPPED)
def test_gl_parity_with_restatement_on_the_shipped_scenes(name):
    sc, o = _shipped(name)
    _check(name, sc, o)
    if name == "gpu_showcase":
        _check(name + " depth 80", sc, o, depth=80)


@pytest.mark.parametrize("name", ["twelve_lights", "edge", "glass", "metal"])
def test_gl_parity_with_restatement_on_synthetic_scenes(name, tmp_path):
    sc, _, o = gs.scene_pair(gs.synthetic_docs()[name], str(tmp_path), name)
    _check(name, sc, o, w=33, h=20, passes=2, depth=6)


def test_gl_with_the_fog_block_matches_restatement():
    sc, o = _shipped("gpu_showcase")
    sc.fog.affect_sky = True  # volumetric and the sky blend together
    img, _ = _check("gpu_showcase fog", sc, o, fog=True)
    sc2, _ = _shipped("gpu_showcase")
    from path_trace_golang_amd import capi

    with capi.Context(ndev=1) as ctx:
        plain, _, _, _ = _render(ctx, sc2)
    assert not np.array_equal(img, plain)


def test_gl_finish_is_post_process_tonemap_of_accum():
    from path_trace_golang_amd import capi, hip

    sc, _ = _shipped("test_scene")
    with capi.Context(ndev=1) as ctx:
        img, acc, _, _ = _render(ctx, sc, passes=3)
        post = np.zeros_like(img)
        hip.post_process(post, hip.PostConfig(tonemap=True), acc, 3, ctx=ctx)
    assert np.array_equal(img, post)


def test_gl_is_invariant_to_chunks_steps_shards_and_devices():
    import torch

    from path_trace_golang_amd import capi, hip

    sc, _ = _shipped("metal_glass_room")
    passes = 5
    L = capi.load()
    with capi.Context(ndev=1) as ctx:
        ref_img, ref_acc, ref_st, ref_gl = _render(ctx, sc, passes=passes)
        for chunk in (1, 2, 3):
            img, acc, st, gst = _render(ctx, sc, passes=passes, chunk=chunk)
            assert np.array_equal(img, ref_img) and np.array_equal(acc, ref_acc), chunk
            assert gst["shadow_rays"] == ref_gl["shadow_rays"] and st["segments"] == ref_st["segments"]
        # progressive: steps of 1, 3, rest, with pt_read in between
        flat = hip.FlatScene(sc)
        cfg = hip.pt_config(hip.RenderConfig(W, H, passes, DEPTH, SEED))
        hip.set_shading(ctx, "gl", sc)
        capi.check(L.pt_begin(ctx.handle, C.byref(flat.c), C.byref(cfg)))
        done = C.c_int32(0)
        img = np.zeros((H, W, 4), np.uint8)
        acc = np.zeros((H, W, 3))
        for n in (1, 3, passes):
            capi.check(L.pt_step(ctx.handle, n, C.byref(done)))
            capi.check(L.pt_read(ctx.handle, img.ctypes.data_as(C.c_void_p), W * 4, acc.ctypes.data_as(C.c_void_p)))
            post = np.zeros_like(img)
            hip.post_process(post, hip.PostConfig(tonemap=True), acc, done.value, ctx=None)
            assert np.array_equal(img, post), done.value  # the GL finish of a partial frame too
        st = capi.PtStats()
        capi.check(L.pt_end(ctx.handle, C.byref(st)))
        assert done.value == passes
        assert np.array_equal(img, ref_img) and np.array_equal(acc, ref_acc)
        # device entry point: 3 shards, gathered back to back and untiled on the device
        dev = torch.device("cuda", 0)
        ntl = C.c_int32(0)
        tiles, taccs, paths = [], [], 0
        for k in range(3):
            capi.check(L.pt_shard_tiles(W, H, C.byref(capi.PtShard(k, 3)), C.byref(ntl), None, None))
            t = torch.zeros(max(1, ntl.value) * 4096, dtype=torch.uint8, device=dev)
            a = torch.zeros(max(1, ntl.value) * 3072, dtype=torch.float64, device=dev)
            capi.check(L.pt_render_tiles_device(ctx.handle, C.byref(flat.c), C.byref(cfg), C.byref(capi.PtShard(k, 3)),
                                                C.c_void_p(t.data_ptr()), C.c_void_p(a.data_ptr()), None, None))
            paths += hip.shading_last_stats(ctx)["paths"]
            tiles.append(t[:ntl.value * 4096])
            taccs.append(a[:ntl.value * 3072])
        hip.set_shading(ctx, "cpu")
        dimg = torch.zeros(H * W * 4, dtype=torch.uint8, device=dev)
        dacc = torch.zeros(H * W * 3, dtype=torch.float64, device=dev)
        gt, ga = torch.cat(tiles), torch.cat(taccs)
        capi.check(L.pt_untile_device(ctx.handle, W, H, 3, 0, C.c_void_p(gt.data_ptr()), C.c_void_p(ga.data_ptr()),
                                      C.c_void_p(dimg.data_ptr()), W * 4, C.c_void_p(dacc.data_ptr()), None))
        torch.cuda.synchronize()
        assert np.array_equal(dimg.cpu().numpy().reshape(H, W, 4), ref_img)
        assert np.array_equal(dacc.cpu().numpy().reshape(H, W, 3), ref_acc)
        assert paths == ref_gl["paths"] == 16 * W * H * passes
    # two devices in one context (ordinal 0 listed twice works on any box), and two real ones when visible
    with capi.Context(devices=[0, 0]) as ctx2:
        img, acc, _, gst = _render(ctx2, sc, passes=passes)
    assert np.array_equal(img, ref_img) and np.array_equal(acc, ref_acc) and gst["gl_launches"] >= 2
    if capi.device_count() >= 2:
        with capi.Context(devices=[0, 1]) as ctx3:
            img, acc, _, _ = _render(ctx3, sc, passes=passes)
        assert np.array_equal(img, ref_img) and np.array_equal(acc, ref_acc)


def test_off_is_off(oracle):
    from path_trace_golang_amd import capi, hip

    sc, o = _shipped("metal_glass_room")
    w, h, spp, depth, seed = 32, 24, 2, 6, 3
    ref = oracle.render(o, w, h, spp, depth, seed)
    with capi.Context(ndev=1) as ctx:
        _render(ctx, sc)
        hip.set_shading(ctx, "cpu")  # pt_set_shading(NULL)
        render_vs_oracle(ctx, sc, ref, w, h, spp, depth, seed, tag="after pt_set_shading(NULL)")
        assert hip.shading_last_stats(ctx)["gl_launches"] == 0
    with capi.Context(ndev=1) as ctx:  # never called: plain pt_render
        L = capi.load()
        flat = hip.FlatScene(sc)
        cfg = hip.pt_config(hip.RenderConfig(w, h, spp, depth, seed))
        img = np.zeros((h, w, 4), np.uint8)
        acc = np.zeros((h, w, 3))
        st = capi.PtStats()
        capi.check(L.pt_render(ctx.handle, C.byref(flat.c), C.byref(cfg), img.ctypes.data_as(C.c_void_p), w * 4,
                               acc.ctypes.data_as(C.c_void_p), None, None, C.byref(st)))
        assert np.array_equal(img, ref["rgba"])
        assert hip.shading_last_stats(ctx)["gl_launches"] == 0


def test_refusals_leave_the_context_usable(tmp_path):
    from path_trace_golang_amd import capi, hip, synth

    big = synth.make_scene(400, seed=3)
    assert sum(1 for o in big.objects if o.type in ("sphere", "sphere_light")) > 128
    sc, _ = _shipped("test_scene")
    L = capi.load()
    with capi.Context(ndev=1) as ctx:
        with pytest.raises(capi.PtError) as e:
            _render(ctx, big, w=32, h=32, passes=1, depth=3)
        assert e.value.code == capi.PT_ERR_INVALID and "BVH" in str(e.value)
        with pytest.raises(capi.PtError) as e:
            _render(ctx, sc, flags=capi.PT_FLAG_PIXEL_STATS)
        assert e.value.code == capi.PT_ERR_INVALID
        # a material table of the wrong length
        arr = hip.gl_materials(sc)
        s = capi.PtShading(capi.PT_SHADING_GL, len(sc.materials) - 1, C.cast(arr, C.POINTER(capi.PtGlMaterial)))
        capi.check(L.pt_set_shading(ctx.handle, C.byref(s)))
        flat = hip.FlatScene(sc)
        cfg = hip.pt_config(hip.RenderConfig(W, H, 1, DEPTH, SEED))
        img = np.zeros((H, W, 4), np.uint8)
        rc = L.pt_render(ctx.handle, C.byref(flat.c), C.byref(cfg), img.ctypes.data_as(C.c_void_p), W * 4, None, None, None, None)
        assert rc == capi.PT_ERR_INVALID and b"material" in L.pt_last_error()
        assert not img.any()  # nothing launched, nothing written
        # still usable: a GL render and a CPU-engine render
        img, acc, st, gst = _render(ctx, sc, passes=1)
        assert gst["paths"] == 16 * W * H and img.any()
        hip.set_shading(ctx, "cpu")
        img2 = np.zeros((H, W, 4), np.uint8)
        st2 = hip.render(sc, hip.RenderConfig(W, H, 1, DEPTH, SEED), img2, ctx=ctx)
        assert st2["samples"] == W * H
