"""GL shading on the BVH path on the MI355X (pt_set_shading_walk, gl_bvh_kernel): whole-frame parity with the independent CPU
restatement tests/glshade_reference.c -- rgba byte-equal, accum at the GL tests' bar, the counters equal -- on the scenes of
glwalk_support.py (test_glshade_walk_cpu.py shows on the host that they reach what they are for, and that none of those that must
not takes the plain loop); invariance to chunking, progressive steps, shards, device count, who built the tree and a refit; the
linear gl_trace_kernel itself (PTCORE_SCAN=uniform) on the device; and the switch's own rules.  Every test uses contexts of its own."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import pytest

import glwalk_support as gw

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, scope="module")
def _torch_before_libptcore():
    import torch  # noqa: F401  (one HIP runtime in the process, as in test_glshade_gpu.py)


def _ctx(env=None, **kw):
    """A context of its own, made under `env` (PTCORE_* variables are read at pt_create)."""
    from path_trace_golang_amd import capi

    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return capi.Context(**(kw or {"ndev": 1}))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _render(ctx, case, walk=True, chunk=0, flags=0, passes=None, fog=False, shading="gl", **kw):
    """(img, accum, pt_stats, pt_shading_last_stats) of one frame of the case's cfg = (w, h, passes, depth, seed)."""
    from path_trace_golang_amd import hip

    w, h, p, depth, seed = case["cfg"]
    p = p if passes is None else passes
    img, acc = np.zeros((h, w, 4), np.uint8), np.zeros((h, w, 3))
    st = hip.render(case["sc"], hip.RenderConfig(w, h, p, depth, seed, chunk, flags), img, None, acc, ctx=ctx, fog=fog, shading=shading,
                    shading_walk=walk, **kw)
    return img, acc, st, hip.shading_last_stats(ctx)


GLC = ("paths", "segments", "shadow_rays", "probe_rays", "draws")


def _same(a, b):
    """Two frames bit-equal in rgba, accum and the five GL counters."""
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64)) and all(a[3][k] == b[3][k] for k in GLC)


def _parity(ctx, case, tag="", fog=None, **kw):
    """A frame of `case` with the walk against the reference, at the bar of test_glshade_gpu.py; returns the frame and the walk's
    counters, which must account for every query the model made."""
    from path_trace_golang_amd import hip

    ref_img, ref_acc, ref_st = gw.reference(case, fog)
    depth = case["cfg"][3]
    got = _render(ctx, case, fog=fog is not None, **kw)
    img, acc, st, gst = got
    ws = hip.shading_walk_stats(ctx)
    assert np.array_equal(img, ref_img), (case["name"], tag, int(np.count_nonzero(img != ref_img)))
    rel = np.abs(acc - ref_acc) / np.maximum(np.abs(ref_acc), 1e-300)
    assert float(np.max(rel)) <= 4 * depth * 2.0 ** -52, (case["name"], tag, float(np.max(rel)))
    print("%s %s: accum bit-equal to the restatement: %s; walk %s" % (case["name"], tag, np.array_equal(acc.view(np.uint64), ref_acc.view(np.uint64)), ws))
    assert tuple(gst[k] for k in GLC) == tuple(ref_st[k] for k in GLC), (case["name"], tag)
    assert (st["samples"], st["segments"], st["draws"]) == (ref_st["paths"], ref_st["segments"], ref_st["draws"])
    assert gst["gl_launches"] >= 1 and gst["gl_ms"] > 0 and st["trace_ms"] == pytest.approx(gst["gl_ms"])
    assert ws["closest_walked"] + ws["closest_plain"] == gst["segments"] + gst["probe_rays"], ws
    assert ws["shadow_walked"] + ws["shadow_plain"] == gst["shadow_rays"], ws
    return got, ws


# ---------------------------------------------------------------- 1. the smallest tree, a ragged frame, both builds of the BVH scan
def test_threshold_scene_is_refused_without_the_switch_and_matches_the_reference_with_it():
    from path_trace_golang_amd import capi

    case = gw.threshold_case()
    assert gw.kinds(case) == (131, 0, 1) and case["cfg"][:3] == (40, 24, 2)
    for env in ({}, {"PTCORE_SCAN": "verify_bvh"}):
        with _ctx(env) as ctx:
            with pytest.raises(capi.PtError) as e:
                _render(ctx, case, walk=False)
            assert e.value.code == capi.PT_ERR_INVALID and "GL shading is not available for scenes on the BVH path" in str(e.value)
            _, ws = _parity(ctx, case, tag=str(env), chunk=1)
            assert ws["closest_plain"] == 0 and ws["shadow_plain"] == 0 and ws["shadow_walked"] > 0 and ws["deepest_stack"] >= 1, ws
            assert ws["closest_visits"] >= ws["closest_walked"] > 0 and ws["shadow_visits"] > 0, ws


# ---------------------------------------------------------------- 2. the room and the tie constructions, shallow and deep
@pytest.mark.parametrize("depth", [1, 8])
@pytest.mark.parametrize("name", ["room", "ties"])
def test_room_and_ties_match_the_reference(name, depth):
    case = gw.with_cfg(gw.room_case() if name == "room" else gw.ties_case(), depth=depth)
    assert case["cfg"][:2] == (33, 20)
    with _ctx() as ctx:
        (img, _, _, gst), ws = _parity(ctx, case)
    assert ws["closest_plain"] == 0 and ws["shadow_plain"] == 0, ws
    if name == "room" and depth == 8:
        assert gst["probe_rays"] > 0 and gst["shadow_rays"] > 0 and len(np.unique(img[..., :3].reshape(-1, 3), axis=0)) > 50


def test_far_camera_takes_the_plain_loop_for_what_starts_outside_and_the_walk_for_the_rest():
    case = gw.far_case()
    assert case["cfg"][3] == 3
    with _ctx() as ctx:
        _, ws = _parity(ctx, case)
    assert min(ws["closest_walked"], ws["closest_plain"], ws["shadow_walked"], ws["shadow_plain"]) > 0, ws
    assert ws["closest_plain"] >= 16 * 33 * 20 * case["cfg"][2]  # every primary ray at the least


@pytest.mark.parametrize("i", range(gw.N_FUZZ))
def test_random_geometry_matches_the_reference(i):
    case = gw.fuzz_case(i)
    with _ctx() as ctx:
        _, ws = _parity(ctx, case)
    assert ws["closest_plain"] == 0 and ws["shadow_plain"] == 0, ws


def test_negative_size_box_is_accepted_and_an_unknown_type_is_refused_by_name():
    from path_trace_golang_amd import capi

    with _ctx() as ctx:
        with pytest.raises(capi.PtError) as e:
            _render(ctx, gw.unknown_type_case())
        assert e.value.code == capi.PT_ERR_INVALID and "object %d is of unknown type" % gw.UNKNOWN_INDEX in str(e.value), str(e.value)
        with pytest.raises(capi.PtError):  # asked once per scene: the cached answer is the same
            _render(ctx, gw.unknown_type_case())
        _parity(ctx, gw.negative_box_case())  # the context goes on


# ---------------------------------------------------------------- 3. invariance
def test_room_is_invariant_to_chunks_steps_shards_devices_device_build_and_refit():
    import torch

    from path_trace_golang_amd import capi, hip, tiling

    case = gw.with_cfg(gw.room_case(), passes=3, depth=4)
    sc, (w, h, passes, depth, seed) = case["sc"], case["cfg"]
    with _ctx() as ctx:
        one = _render(ctx, case)
        ws1 = hip.shading_walk_stats(ctx)
        assert one[3]["shadow_rays"] > 0
        for chunk in (1, 2):
            assert _same(_render(ctx, case, chunk=chunk), one), chunk
            assert hip.shading_walk_stats(ctx) == ws1
        # progressive: uneven steps, then pt_read
        L = capi.load()
        flat = hip.FlatScene(sc)
        pc = hip.pt_config(hip.RenderConfig(w, h, passes, depth, seed))
        hip.set_shading(ctx, "gl", sc)
        hip.set_shading_walk(ctx, True)
        capi.check(L.pt_begin(ctx.handle, C.byref(flat.c), C.byref(pc)))
        assert L.pt_set_shading_walk(ctx.handle, 0) == capi.PT_ERR_STATE  # not while a frame is open
        done = C.c_int32(0)
        for n in (1, 2, 5):
            capi.check(L.pt_step(ctx.handle, n, C.byref(done)))
        img, acc = np.zeros((h, w, 4), np.uint8), np.zeros((h, w, 3))
        capi.check(L.pt_read(ctx.handle, img.ctypes.data_as(C.c_void_p), w * 4, acc.ctypes.data_as(C.c_void_p)))
        capi.check(L.pt_end(ctx.handle, C.byref(capi.PtStats())))
        assert done.value == passes
        assert _same((img, acc, None, hip.shading_last_stats(ctx)), one)
        # device entry point: 3 shards, untiled on the host; the counters add up
        dev = torch.device("cuda", 0)
        stride = tiling.max_shard_tiles(w, h, 3)
        tiles, taccs, counts = [], [], np.zeros(5, np.int64)
        for k in range(3):
            t = torch.zeros(stride * 4096, dtype=torch.uint8, device=dev)
            a = torch.zeros(stride * 3072, dtype=torch.float64, device=dev)
            sh = capi.PtShard(k, 3)
            capi.check(L.pt_render_tiles_device(ctx.handle, C.byref(flat.c), C.byref(pc), C.byref(sh), C.c_void_p(t.data_ptr()),
                                                C.c_void_p(a.data_ptr()), None, None))
            gst = hip.shading_last_stats(ctx)  # collected lazily: waits for the render
            counts += np.array([gst[k2] for k2 in GLC])
            tiles.append(t.cpu().numpy())
            taccs.append(a.cpu().numpy())
        img = tiling.untile([x.reshape(stride, 32, 32, 4) for x in tiles], w, h, 3, 4, np.uint8, stride)
        acc = tiling.untile([x.reshape(stride, 32, 32, 3) for x in taccs], w, h, 3, 3, np.float64, stride)
        assert np.array_equal(img, one[0]) and np.array_equal(acc.view(np.uint64), one[1].view(np.uint64))
        assert tuple(int(c) for c in counts) == tuple(one[3][k] for k in GLC)
        hip.set_shading(ctx, "cpu")
    with _ctx(devices=[0, 0]) as ctx2:  # two devices in one context (ordinal 0 listed twice works on any box)
        two = _render(ctx2, case)
        assert _same(two, one) and two[3]["gl_launches"] >= 2
        assert hip.shading_walk_stats(ctx2) == ws1  # summed over the devices, the deepest stack their largest
    if capi.device_count() >= 2:
        with _ctx(devices=[0, 1]) as ctx2b:
            assert _same(_render(ctx2b, case), one)
    with _ctx() as ctx3:  # the tree built on the device
        assert _same(_render(ctx3, case, bvh_build="device"), one)
        assert hip.bvh_build_stats(ctx3)["device_builds"] >= 1
    # a refitted tree: three objects moved under bvh_refit=1.25, against a fresh context's frame of the moved scene
    moved = gw.moved(case)
    with _ctx() as ctx4:
        _render(ctx4, case, bvh_refit=1.25)
        refit = _render(ctx4, moved, bvh_refit=1.25)
        assert hip.bvh_refit_stats(ctx4)["last_action"] == 2  # it was a refit
    with _ctx() as ctx5:
        fresh = _render(ctx5, moved)
    assert _same(refit, fresh) and not np.array_equal(fresh[1], one[1])


# ---------------------------------------------------------------- 4. the linear kernel on the device
def test_walk_equals_the_linear_gl_kernel_on_the_device():
    from path_trace_golang_amd import capi, hip

    case = None
    with _ctx({"PTCORE_SCAN": "uniform"}) as ctx:
        for n in gw.LINEAR_COUNTS:  # the uniform plan may refuse a count for LDS: step down until one is accepted
            case = gw.linear_case(n)
            try:
                a = _render(ctx, case)  # (the switch is on and ignored: this is no BVH scan)
                break
            except capi.PtError as e:
                assert n != gw.LINEAR_COUNTS[-1], str(e)
        print("linear count accepted:", n)
        assert a[3]["shadow_rays"] > 0 and a[3]["gl_launches"] >= 1
        with pytest.raises(capi.PtError):
            hip.shading_walk_stats(ctx)  # gl_trace_kernel ran
    with _ctx() as ctx:
        b = _render(ctx, case)
        ws = hip.shading_walk_stats(ctx)
        assert ws["closest_walked"] > 0 and ws["shadow_walked"] > 0
    assert _same(a, b)


# ---------------------------------------------------------------- 5. switch hygiene
def test_switch_rules():
    from path_trace_golang_amd import capi, hip

    small, big = gw.small_case(), gw.with_cfg(gw.threshold_case(), passes=1, depth=3)
    assert len(small["sc"].objects) == 27
    L = capi.load()
    out = (C.c_uint64 * 7)()
    with _ctx() as ctx:
        # ignored off the BVH path
        off = _render(ctx, small, walk=False)
        on = _render(ctx, small, walk=True)
        assert _same(on, off) and on[3]["shadow_rays"] > 0
        assert L.pt_shading_walk_stats(ctx.handle, out) == capi.PT_ERR_STATE
        # on, then off: the refusal is back, and the stats say no walk ran
        walked = _render(ctx, big)
        assert hip.shading_walk_stats(ctx)["closest_walked"] > 0
        with pytest.raises(capi.PtError) as e:
            _render(ctx, big, walk=False)
        assert e.value.code == capi.PT_ERR_INVALID and "BVH" in str(e.value)
        assert L.pt_shading_walk_stats(ctx.handle, out) == capi.PT_ERR_STATE
        assert _same(_render(ctx, small, walk=False), off)  # the context goes on
        # a CPU-engine frame of the big scene ignores the switch
        cpu = _render(ctx, big, shading="cpu")
        assert cpu[2]["samples"] == 40 * 24 and L.pt_shading_walk_stats(ctx.handle, out) == capi.PT_ERR_STATE
        # the combinations that stay refused, each by its own message, the context usable after each
        refusals = (
            (dict(flags=capi.PT_FLAG_PIXEL_STATS), "PT_FLAG_PIXEL_STATS"),
            (dict(features=2), "features"),
            (dict(noise=0.5, noise_step=1, adaptive=True), "adaptive"),
        )
        for kw, word in refusals:
            with pytest.raises((capi.PtError, ValueError, RuntimeError)) as e:
                _render(ctx, big, **kw)
            assert word in str(e.value), (word, str(e.value))
            assert _same(_render(ctx, big), walked), word
        # injected primary rays
        w, h = big["cfg"][:2]
        rays = np.tile(np.array([0.0, 2.0, 9.0, 0.0, 0.0, -1.0]), (w * h, 1))
        ctx.set_primary_rays(rays)
        with pytest.raises(capi.PtError) as e:
            _render(ctx, big)
        assert "injected primary rays" in str(e.value)
        ctx.set_primary_rays(None)
        assert _same(_render(ctx, big), walked)


def test_fog_with_gl_on_the_bvh_path():
    """gpu_volumetric is refused (fog_march's shadow tests loop over all objects), with or without pt_set_fog_walk; affect_sky alone is
    accepted and equals the reference: the far scene has no dome, so the rewritten sky is seen."""
    import copy

    from path_trace_golang_amd import capi, hip, scene

    base = gw.far_case()
    doc = copy.deepcopy(base["doc"])
    doc["fog"] = {"density": 0.08, "color": {"r": 0.9, "g": 0.9, "b": 1.0}, "scatter": 0.8, "g": 0.3, "hetero_strength": 0.0, "noise_scale": 2.0,
                  "noise_octaves": 2, "affect_sky": True, "gpu_volumetric": True}
    vol = gw._case("far-fog-vol", doc, base["cfg"])
    doc2 = copy.deepcopy(doc)
    doc2["fog"]["gpu_volumetric"] = False
    sky = gw._case("far-fog-sky", doc2, base["cfg"])
    assert isinstance(vol["sc"], scene.Scene) and vol["sc"].fog is not None
    with _ctx() as ctx:
        for fog_walk in (False, True):
            with pytest.raises(capi.PtError) as e:
                _render(ctx, vol, fog=True, **({"fog_walk": True} if fog_walk else {}))
            assert e.value.code == capi.PT_ERR_INVALID and "gpu_volumetric is not available with GL shading on the BVH path" in str(e.value)
        (img, _, _, _), ws = _parity(ctx, sky, fog=hip.pt_fog(sky["sc"].fog))
        plain = _render(ctx, base)
        assert not np.array_equal(img, plain[0]) and ws["closest_walked"] > 0
