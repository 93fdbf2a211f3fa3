"""Fog on the MI355X (pt_set_fog, fog_kernel): parity with the independent CPU restatement tests/fog_reference.c on the
shipped fog scenes, a light behind an occluder and a thin-lens camera, in both kernel builds; fog off is the fog-off
image bit for bit; affect_sky alone; invariance to chunking, progressive steps, shards and device count; refusal on the
BVH path.  Every test uses contexts of its own, so the shared session context never carries a fog block."""
from __future__ import annotations

import copy
import ctypes as C
import json
import os

import numpy as np
import pytest

import fog_support as fs
from conftest import scene_path

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, scope="module")
def _torch_before_libptcore():
    # the shard test hands torch device memory to the C ABI: torch's HIP runtime must be loaded before libptcore.so
    import torch  # noqa: F401


W, H, SPP, DEPTH, SEED = 96, 54, 4, 8, 5


def _doc(name):
    with open(scene_path(name)) as f:
        return json.load(f)


def _occluder_doc():
    """One emissive sphere above a box that shadows part of the fogged room from it."""
    return {
        "name": "fog-occluder",
        "camera": {"position": {"x": 0, "y": 2, "z": 9}, "target": {"x": 0, "y": 1.5, "z": 0}, "up": {"x": 0, "y": 1, "z": 0},
                   "fov": 60},
        "materials": [
            {"id": "floor", "type": "lambert", "albedo": {"r": 0.7, "g": 0.7, "b": 0.7}},
            {"id": "block", "type": "lambert", "albedo": {"r": 0.3, "g": 0.4, "b": 0.6}},
            {"id": "lamp", "type": "emissive", "emit": {"r": 1.0, "g": 0.9, "b": 0.7}, "power": 4.0},
        ],
        "objects": [
            {"type": "plane", "position": {"x": 0, "y": 0, "z": 0}, "material_id": "floor"},
            {"type": "box", "position": {"x": 0, "y": 3.5, "z": 0}, "size": {"x": 3, "y": 0.3, "z": 3}, "material_id": "block"},
            {"type": "sphere_light", "position": {"x": 0.3, "y": 6, "z": 0.2}, "size": {"x": 0.6, "y": 0.6, "z": 0.6},
             "material_id": "lamp"},
            {"type": "sphere", "position": {"x": -2, "y": 1, "z": 1}, "size": {"x": 1, "y": 1, "z": 1}, "material_id": "block"},
        ],
        "background": {"r": 0.05, "g": 0.05, "b": 0.08},
        "fog": {"density": 0.15, "color": {"r": 0.9, "g": 0.9, "b": 1.0}, "scatter": 0.8, "g": 0.3, "hetero_strength": 0.5,
                "noise_scale": 2.0, "noise_octaves": 2, "affect_sky": True, "gpu_volumetric": True},
    }


def _lens_doc():
    d = copy.deepcopy(_doc("gpu_showcase"))
    d["camera"]["aperture"] = 0.15
    d["camera"]["focus_dist"] = 0  # focus on the target
    return d


def _scenes(doc, tmp_path, name):
    from oracle import ora

    from path_trace_golang_amd import scene

    p = tmp_path / (name + ".json")
    p.write_text(json.dumps(doc))
    return scene.load(str(p)), ora.Scene(doc)


def _render(ctx, sc, fog, w=W, h=H, spp=SPP, depth=DEPTH, seed=SEED, chunk=0, flags=0):
    from path_trace_golang_amd import hip

    img = np.zeros((h, w, 4), np.uint8)
    acc = np.zeros((h, w, 3))
    st = hip.render(sc, hip.RenderConfig(w, h, spp, depth, seed, chunk, flags), img, None, acc, ctx=ctx, fog=fog)
    return img, acc, st, hip.fog_last_stats(ctx)


def _close(acc, ref, depth=DEPTH):
    rel = np.abs(acc - ref) / np.maximum(np.abs(ref), 1e-300)
    return float(np.max(rel)) <= 4 * depth * 2.0 ** -52


CASES = ["gpu_showcase", "test_scene", "occluder", "thin_lens"]


@pytest.mark.parametrize("case", CASES)
def test_fog_parity_with_reference(case, tmp_path):
    from path_trace_golang_amd import capi

    doc = _occluder_doc() if case == "occluder" else _lens_doc() if case == "thin_lens" else _doc(case)
    sc, oc = _scenes(doc, tmp_path, case)
    fog = fs.fog_of_scene(doc["fog"])
    ref_img, ref_acc, ref_st = fs.reference_render(oc, W, H, SPP, DEPTH, SEED, fog)
    assert ref_st["shadow_rays"] > 0 and ref_st["steps"] > 0
    with capi.Context(ndev=1) as ctx:
        off_img, _, off_st, off_fog = _render(ctx, sc, False)
        assert off_fog["fog_launches"] == 0
        for flags in (capi.PT_FLAG_PIXEL_STATS, 0):
            img, acc, st, fst = _render(ctx, sc, True, flags=flags)
            assert np.array_equal(img, ref_img), (case, flags, int(np.count_nonzero(img != ref_img)))
            assert _close(acc, ref_acc), case
            assert (st["segments"], st["draws"]) == (off_st["segments"], off_st["draws"]) == (ref_st["segments"], ref_st["draws"])
            assert (fst["shadow_rays"], fst["draws"], fst["steps"]) == (ref_st["shadow_rays"], ref_st["fog_draws"], ref_st["steps"])
            assert fst["fog_launches"] >= 1 and fst["fog_ms"] > 0
        assert not np.array_equal(img, off_img)  # the fog is visible


def test_fog_off_is_off(tmp_path):
    from path_trace_golang_amd import capi, hip, scene

    sc = scene.load(scene_path("gpu_showcase"))
    flat = hip.FlatScene(sc)  # a FlatScene carries no fog block: hip.render leaves the context's setting to the calls below
    L = capi.load()

    def plain(ctx):
        img = np.zeros((H, W, 4), np.uint8)
        acc = np.zeros((H, W, 3))
        st = capi.PtStats()
        cfg = hip.pt_config(hip.RenderConfig(W, H, SPP, DEPTH, SEED))
        capi.check(L.pt_render(ctx.handle, C.byref(flat.c), C.byref(cfg), img.ctypes.data_as(C.c_void_p), W * 4,
                               acc.ctypes.data_as(C.c_void_p), None, None, C.byref(st)))
        return img, acc, (st.segments, st.draws, st.exit_scans), hip.fog_last_stats(ctx)

    with capi.Context(ndev=1) as ctx:
        base = plain(ctx)  # a context that never saw fog
    with capi.Context(ndev=1) as ctx:
        hip.set_fog(ctx, sc.fog)
        fogged = plain(ctx)
        hip.set_fog(ctx, None)
        after = plain(ctx)
        quiet = copy.deepcopy(sc.fog)
        quiet.gpu_volumetric = False
        quiet.affect_sky = False
        hip.set_fog(ctx, quiet)
        inert = plain(ctx)
    assert not np.array_equal(fogged[0], base[0])
    for other in (after, inert):
        assert np.array_equal(other[0], base[0])
        assert np.array_equal(other[1].view(np.uint64), base[1].view(np.uint64))
        assert other[2] == base[2]
        assert other[3]["fog_launches"] == 0 and other[3]["shadow_rays"] == 0


def test_affect_sky_only_matches_oracle_on_the_rewritten_sky(tmp_path):
    from path_trace_golang_amd import capi

    doc = _doc("test_scene")
    doc["fog"] = {"density": 0.01, "color": {"r": 0.9, "g": 0.6, "b": 0.3}, "affect_sky": True, "gpu_volumetric": False}
    doc["sky"] = {"type": "gradient", "horizon": {"r": 0.9, "g": 0.9, "b": 1.0}, "zenith": {"r": 0.2, "g": 0.4, "b": 0.9},
                  "color": {"r": 0.5, "g": 0.5, "b": 0.5}}
    sc, oc = _scenes(doc, tmp_path, "sky")
    fog = fs.fog_of_scene(doc["fog"])
    ref_img, ref_acc, ref_st = fs.reference_render(oc, W, H, SPP, DEPTH, SEED, fog)
    assert ref_st["steps"] == 0
    with capi.Context(ndev=1) as ctx:
        off_img, _, _, _ = _render(ctx, sc, False)
        img, acc, st, fst = _render(ctx, sc, True)
    assert fst["fog_launches"] == 0
    assert np.array_equal(img, ref_img) and _close(acc, ref_acc)
    assert (st["segments"], st["draws"]) == (ref_st["segments"], ref_st["draws"])
    assert not np.array_equal(img, off_img)  # the sky is seen and changed


def test_fog_is_invariant_to_chunks_steps_shards_and_devices():
    import torch

    from path_trace_golang_amd import capi, hip, scene, tiling

    sc = scene.load(scene_path("test_scene"))
    spp = 5
    with capi.Context(ndev=1) as ctx:
        ref_img, ref_acc, ref_st, ref_fog = _render(ctx, sc, True, spp=spp, chunk=0)
        for chunk in (1, 3):
            img, acc, st, fst = _render(ctx, sc, True, spp=spp, chunk=chunk)
            assert np.array_equal(img, ref_img) and np.array_equal(acc, ref_acc), chunk
            assert fst["shadow_rays"] == ref_fog["shadow_rays"] and fst["draws"] == ref_fog["draws"]
        # progressive: uneven steps, then pt_read
        L = capi.load()
        flat = hip.FlatScene(sc)
        cfg = hip.pt_config(hip.RenderConfig(W, H, spp, DEPTH, SEED))
        hip.set_fog(ctx, sc.fog)
        capi.check(L.pt_begin(ctx.handle, C.byref(flat.c), C.byref(cfg)))
        done = C.c_int32(0)
        for n in (1, 3, 7):
            capi.check(L.pt_step(ctx.handle, n, C.byref(done)))
        img = np.zeros((H, W, 4), np.uint8)
        acc = np.zeros((H, W, 3))
        capi.check(L.pt_read(ctx.handle, img.ctypes.data_as(C.c_void_p), W * 4, acc.ctypes.data_as(C.c_void_p)))
        st = capi.PtStats()
        capi.check(L.pt_end(ctx.handle, C.byref(st)))
        assert done.value == spp
        assert np.array_equal(img, ref_img) and np.array_equal(acc, ref_acc)
        assert hip.fog_last_stats(ctx)["shadow_rays"] == ref_fog["shadow_rays"]
        # device entry point: shards {0,2} and {1,2}, untiled on the host
        dev = torch.device("cuda", 0)
        stride = tiling.max_shard_tiles(W, H, 2)
        tiles, taccs, shadow = [], [], 0
        for k in range(2):
            t = torch.zeros(stride * 4096, dtype=torch.uint8, device=dev)
            a = torch.zeros(stride * 3072, dtype=torch.float64, device=dev)
            sh = capi.PtShard(k, 2)
            capi.check(L.pt_render_tiles_device(ctx.handle, C.byref(flat.c), C.byref(cfg), C.byref(sh), C.c_void_p(t.data_ptr()),
                                                C.c_void_p(a.data_ptr()), None, None))
            shadow += hip.fog_last_stats(ctx)["shadow_rays"]  # collected lazily: waits for the render
            tiles.append(t.cpu().numpy())
            taccs.append(a.cpu().numpy())
        hip.set_fog(ctx, None)
        img = tiling.untile([x.reshape(stride, 32, 32, 4) for x in tiles], W, H, 2, 4, np.uint8, stride)
        acc = tiling.untile([x.reshape(stride, 32, 32, 3) for x in taccs], W, H, 2, 3, np.float64, stride)
        assert np.array_equal(img, ref_img) and np.array_equal(acc, ref_acc)
        assert shadow == ref_fog["shadow_rays"]
    # two devices in one context (ordinal 0 listed twice works on any box)
    with capi.Context(devices=[0, 0]) as ctx2:
        img, acc, st, fst = _render(ctx2, sc, True, spp=spp)
    assert np.array_equal(img, ref_img) and np.array_equal(acc, ref_acc)
    assert fst["shadow_rays"] == ref_fog["shadow_rays"] and fst["fog_launches"] >= 2


def test_wavefront_pipeline_gives_the_same_fog_bytes():
    from path_trace_golang_amd import capi, scene

    sc = scene.load(scene_path("gpu_showcase"))
    with capi.Context(ndev=1) as ctx:
        ref = _render(ctx, sc, True)
    old = os.environ.get("PTCORE_PIPELINE")
    os.environ["PTCORE_PIPELINE"] = "wavefront"  # read at pt_create
    try:
        with capi.Context(ndev=1) as ctx:
            got = _render(ctx, sc, True)
    finally:
        if old is None:
            del os.environ["PTCORE_PIPELINE"]
        else:
            os.environ["PTCORE_PIPELINE"] = old
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    assert got[3]["shadow_rays"] == ref[3]["shadow_rays"]


def test_bvh_scene_refuses_volumetric_fog_but_takes_affect_sky():
    from path_trace_golang_amd import capi, scene, synth

    sc = synth.make_scene(400, seed=3)
    assert sum(1 for o in sc.objects if o.type in ("sphere", "sphere_light")) > 128
    sc.fog = scene.Fog(density=0.05, color=scene.Color(0.8, 0.8, 0.9), affect_sky=True, gpu_volumetric=True)
    with capi.Context(ndev=1) as ctx:
        with pytest.raises(capi.PtError) as e:
            _render(ctx, sc, True, w=32, h=32, spp=1, depth=3)
        assert e.value.code == capi.PT_ERR_INVALID and "BVH" in str(e.value)
        sc.fog.gpu_volumetric = False
        img, acc, st, fst = _render(ctx, sc, True, w=32, h=32, spp=1, depth=3)
        assert fst["fog_launches"] == 0 and st["samples"] == 32 * 32
