"""Volumetric fog on the BVH path on the MI355X (pt_set_fog_walk, fog_bvh_kernel).

Every frame here is held to tests/fog_reference.c (fog_support.reference_render, a linear scan that takes any object count) at the
bar of test_fog_gpu.py::test_fog_parity_with_reference: rgba byte-equal, accum within 4 * depth * 2^-52 relative, segments and
draws those of the fog-off frame and of the reference, (shadow rays, fog draws, march steps) those of the reference.  The scenes:
the smallest tree (129 spheres) on a ragged frame; a small synthetic room with a light only the ground plane hides and a light
inside a box, on every pipeline a BVH context has; the same room seen from outside 3.5 scene bounds, where march points start beyond
clip_bound and turns take the plain loop; 0, 1 and 9 lights; the fuzz generator's overlapping, nested and coincident geometry
untrimmed; chunks, progressive steps, shards, two devices, a device-built and a refitted tree; an adaptive frame pixel by pixel;
the linear fog_kernel itself (PTCORE_SCAN=uniform) on the device; and the switch's own rules.  Every test uses contexts of its own.
CPU-side checks of what these scenes reach: tests/test_fog_walk_cpu.py."""
from __future__ import annotations

import copy
import ctypes as C
import os

import numpy as np
import pytest

import fog_walk_support as fw

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, scope="module")
def _torch_before_libptcore():
    import torch  # noqa: F401  (one HIP runtime in the process, as in test_fog_gpu.py)


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


def _render(ctx, sc, cfg, fog=True, walk=True, chunk=0, flags=0, spp=None, **kw):
    """(img, accum, pt_stats, pt_fog_last_stats) of one frame of cfg = (w, h, spp, depth, seed)."""
    from path_trace_golang_amd import hip

    w, h, s, depth, seed = cfg
    s = s if spp is None else spp
    img, acc = np.zeros((h, w, 4), np.uint8), np.zeros((h, w, 3))
    st = hip.render(sc, hip.RenderConfig(w, h, s, depth, seed, chunk, flags), img, None, acc, ctx=ctx, fog=fog, fog_walk=walk, **kw)
    return img, acc, st, hip.fog_last_stats(ctx)


def _fogc(fst):
    return fst["shadow_rays"], fst["draws"], fst["steps"]


def _same(a, b):
    """Two frames bit-equal in rgba, accum and the three fog counters."""
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64)) and _fogc(a[3]) == _fogc(b[3])


def _parity(ctx, case, tag="", off=None, **kw):
    """A frame of `case` with the walk against the reference, at the bar of test_fog_parity_with_reference; returns the frame."""
    ref_img, ref_acc, ref_st = fw.reference(case)
    depth = case["cfg"][3]
    if off is None:
        off = _render(ctx, case["sc"], case["cfg"], fog=False, walk=False)
    got = _render(ctx, case["sc"], case["cfg"], **kw)
    img, acc, st, fst = got
    assert np.array_equal(img, ref_img), (case["name"], tag, int(np.count_nonzero(img != ref_img)))
    nan = np.isnan(ref_acc)
    assert np.array_equal(np.isnan(acc), nan), (case["name"], tag)
    rel = np.abs(acc[~nan] - ref_acc[~nan]) / np.maximum(np.abs(ref_acc[~nan]), 1e-300)
    assert rel.size == 0 or float(rel.max()) <= 4 * depth * 2.0 ** -52, (case["name"], tag, float(rel.max()))
    assert (st["segments"], st["draws"]) == (off[2]["segments"], off[2]["draws"]) == (ref_st["segments"], ref_st["draws"]), (case["name"], tag)
    assert _fogc(fst) == (ref_st["shadow_rays"], ref_st["fog_draws"], ref_st["steps"]), (case["name"], tag)
    assert fst["fog_launches"] >= 1 and fst["fog_ms"] > 0
    return got


# ---------------------------------------------------------------- 1. the smallest tree, a ragged frame, both kernel builds
def test_threshold_scene_is_refused_without_the_switch_and_matches_the_reference_with_it():
    from path_trace_golang_amd import capi, hip

    case = fw.threshold_case()
    assert fw.kinds(case)[0] == 131 and case["cfg"][:2] == (40, 24)
    with _ctx() as ctx:
        with pytest.raises(capi.PtError) as e:
            _render(ctx, case["sc"], case["cfg"], walk=False, chunk=2)
        assert e.value.code == capi.PT_ERR_INVALID and "BVH" in str(e.value)
        off = _render(ctx, case["sc"], case["cfg"], fog=False, walk=False)
        for flags in (capi.PT_FLAG_PIXEL_STATS, 0):
            _parity(ctx, case, tag=flags, off=off, chunk=2, flags=flags)
            ws = hip.fog_walk_stats(ctx)
            assert ws["shadow_walked"] > 0 and ws["shadow_plain"] == 0 and ws["deepest_stack"] >= 1, ws
            assert ws["primary_walked"] > 0 and ws["primary_plain"] == 0 and ws["node_visits"] >= ws["shadow_walked"], ws


# ---------------------------------------------------------------- 2. the synthetic room on every pipeline of a BVH context
PIPELINES = {"default": {}, "lane": {"PTCORE_PRIMARY": "lane"}, "wavefront": {"PTCORE_PIPELINE": "wavefront"},
             "walk32": {"PTCORE_PIPELINE": "walk32"}}


def test_room_matches_the_reference_on_every_pipeline_and_the_pipelines_agree():
    case = fw.room_case()
    frames = {}
    for name, env in PIPELINES.items():
        with _ctx(env) as ctx:
            frames[name] = _parity(ctx, case, tag=name)
    for name in PIPELINES:
        assert _same(frames[name], frames["default"]), name


# ---------------------------------------------------------------- 3. a camera outside clip_bound: turns on the plain loop
def test_far_camera_marches_across_clip_bound_and_takes_the_plain_loop_there():
    from path_trace_golang_amd import hip

    case = fw.far_case()
    x = fw.far_crossing(case)
    assert x["first_point"] > x["clip_bound"] > x["last_point"], x  # the centre pixel's march starts outside and ends inside
    with _ctx() as ctx:
        _parity(ctx, case)
        ws = hip.fog_walk_stats(ctx)
        assert ws["shadow_walked"] > 0 and ws["shadow_plain"] > 0 and ws["primary_plain"] > 0, ws
        _parity(ctx, fw.room_case(), tag="inside")
        ws = hip.fog_walk_stats(ctx)
        assert ws["shadow_plain"] == 0 and ws["primary_plain"] == 0 and ws["shadow_walked"] > 0, ws


# ---------------------------------------------------------------- 4. light counts
@pytest.mark.parametrize("nlight", [0, 1, 9])
def test_light_counts(nlight):
    case = fw.lights_case(nlight)
    _, _, ref_st = fw.reference(case)
    assert ref_st["steps"] > 0 and (ref_st["shadow_rays"] > 0) == (nlight > 0)
    with _ctx() as ctx:
        _parity(ctx, case)


# ---------------------------------------------------------------- 5. random geometry, untrimmed
@pytest.mark.parametrize("i", range(len(fw.FUZZ_SEEDS)))
def test_random_geometry_matches_the_reference(i):
    case = fw.fuzz_case(i)
    ns, nb, _ = fw.kinds(case)
    assert ns > 128 or nb > 128, (ns, nb)
    with _ctx() as ctx:
        _parity(ctx, case)


# ---------------------------------------------------------------- 6. invariance
def test_walk_is_invariant_to_chunks_steps_shards_devices_device_build_and_refit():
    import torch

    from path_trace_golang_amd import capi, hip, tiling

    case = fw.room_case()
    sc, (w, h, _, depth, seed) = case["sc"], case["cfg"]
    spp = 5
    cfg5 = (w, h, spp, depth, seed)
    with _ctx() as ctx:
        one = _render(ctx, sc, cfg5)
        assert one[3]["shadow_rays"] > 0
        for chunk in (1, 3):
            assert _same(_render(ctx, sc, cfg5, chunk=chunk), one), chunk
        # progressive: uneven steps, then pt_read
        L = capi.load()
        flat = hip.FlatScene(sc)
        pc = hip.pt_config(hip.RenderConfig(w, h, spp, depth, seed))
        hip.set_fog(ctx, sc.fog)
        hip.set_fog_walk(ctx, True)
        capi.check(L.pt_begin(ctx.handle, C.byref(flat.c), C.byref(pc)))
        assert L.pt_set_fog_walk(ctx.handle, 0) == capi.PT_ERR_STATE  # not while a frame is open
        done = C.c_int32(0)
        for n in (1, 3, 7):
            capi.check(L.pt_step(ctx.handle, n, C.byref(done)))
        img, acc = np.zeros((h, w, 4), np.uint8), np.zeros((h, w, 3))
        capi.check(L.pt_read(ctx.handle, img.ctypes.data_as(C.c_void_p), w * 4, acc.ctypes.data_as(C.c_void_p)))
        capi.check(L.pt_end(ctx.handle, C.byref(capi.PtStats())))
        assert done.value == spp
        assert _same((img, acc, None, hip.fog_last_stats(ctx)), one)
        # device entry point: shards {0,2} and {1,2}, untiled on the host; the counters add up
        dev = torch.device("cuda", 0)
        stride = tiling.max_shard_tiles(w, h, 2)
        tiles, taccs, counts = [], [], np.zeros(3, np.int64)
        for k in range(2):
            t = torch.zeros(stride * 4096, dtype=torch.uint8, device=dev)
            a = torch.zeros(stride * 3072, dtype=torch.float64, device=dev)
            sh = capi.PtShard(k, 2)
            capi.check(L.pt_render_tiles_device(ctx.handle, C.byref(flat.c), C.byref(pc), C.byref(sh), C.c_void_p(t.data_ptr()),
                                                C.c_void_p(a.data_ptr()), None, None))
            counts += np.array(_fogc(hip.fog_last_stats(ctx)))  # collected lazily: waits for the render
            tiles.append(t.cpu().numpy())
            taccs.append(a.cpu().numpy())
        img = tiling.untile([x.reshape(stride, 32, 32, 4) for x in tiles], w, h, 2, 4, np.uint8, stride)
        acc = tiling.untile([x.reshape(stride, 32, 32, 3) for x in taccs], w, h, 2, 3, np.float64, stride)
        assert np.array_equal(img, one[0]) and np.array_equal(acc.view(np.uint64), one[1].view(np.uint64))
        assert tuple(int(c) for c in counts) == _fogc(one[3])
    with _ctx(devices=[0, 0]) as ctx2:  # two devices in one context (ordinal 0 listed twice works on any box)
        two = _render(ctx2, sc, cfg5)
        assert _same(two, one) and two[3]["fog_launches"] >= 2
        ws = hip.fog_walk_stats(ctx2)
        assert ws["shadow_walked"] > 0 and ws["shadow_plain"] == 0
    with _ctx() as ctx3:  # the tree built on the device
        assert _same(_render(ctx3, sc, cfg5, bvh_build="device"), one)
        assert hip.bvh_build_stats(ctx3)["device_builds"] >= 1
    # a refitted tree: three objects moved under bvh_refit=1.25, against a fresh context's frame of the moved scene
    moved = copy.deepcopy(sc)
    for k, d in ((7, (0.3, 0.1, -0.2)), (60, (-0.25, 0.2, 0.15)), (200, (0.1, -0.05, 0.3))):
        p = moved.objects[k].position
        p.x, p.y, p.z = p.x + d[0], p.y + d[1], p.z + d[2]
    with _ctx() as ctx4:
        _render(ctx4, sc, cfg5, bvh_refit=1.25)
        refit = _render(ctx4, moved, cfg5, bvh_refit=1.25)
        assert hip.bvh_refit_stats(ctx4)["last_action"] == 2  # it was a refit
    with _ctx() as ctx5:
        fresh = _render(ctx5, moved, cfg5)
    assert _same(refit, fresh) and not np.array_equal(fresh[1], one[1])


# ---------------------------------------------------------------- 7. adaptive frames
def test_adaptive_frame_holds_each_pixel_of_the_plain_frame_of_its_own_count():
    from path_trace_golang_amd import hip

    case = fw.room_case()
    sc, (w, h, _, depth, seed) = case["sc"], case["cfg"]
    with _ctx() as ctx:
        counts = np.zeros((h, w), np.uint32)
        ad = _render(ctx, sc, (w, h, 6, depth, seed), noise=fw.ADAPTIVE_TARGET, noise_step=2, adaptive=True, min_spp=2, counts=counts)
        assert hip.fog_walk_stats(ctx)["shadow_walked"] > 0
        assert set(np.unique(counts).tolist()) <= {2, 4, 6} and len(np.unique(counts)) >= 2, np.unique(counts)  # blocks did stop early
        for n in (2, 4, 6):
            plain = _render(ctx, sc, (w, h, n, depth, seed))
            m = counts == n
            assert np.array_equal(ad[1][m].view(np.uint64), plain[1][m].view(np.uint64)), n


# ---------------------------------------------------------------- 8. the linear kernel on the device
def test_walk_equals_the_linear_fog_kernel_on_the_device():
    from path_trace_golang_amd import capi, hip

    case = None
    with _ctx({"PTCORE_SCAN": "uniform"}) as ctx:
        for n in fw.LINEAR_COUNTS:  # the uniform plan may refuse a count for LDS: step down until one is accepted
            case = fw.linear_case(n)
            try:
                a = _render(ctx, case["sc"], case["cfg"], walk=False)
                break
            except capi.PtError as e:
                assert n != fw.LINEAR_COUNTS[-1], str(e)
        assert n == fw.LINEAR_COUNT_ACCEPTED, n  # the count recorded in fog_walk_support
        assert a[3]["shadow_rays"] > 0 and a[3]["fog_launches"] >= 1
        with pytest.raises(capi.PtError):
            hip.fog_walk_stats(ctx)  # today's fog_kernel ran
    with _ctx() as ctx:
        b = _render(ctx, case["sc"], case["cfg"])
        assert hip.fog_walk_stats(ctx)["shadow_walked"] > 0
    assert _same(a, b)


# ---------------------------------------------------------------- 9. switch hygiene
def test_switch_is_ignored_off_the_bvh_path_and_turning_it_off_restores_the_refusal():
    from path_trace_golang_amd import capi, hip

    small, big = fw.small_case(), fw.threshold_case()
    assert len(small["sc"].objects) == 27
    with _ctx() as ctx:
        off = _render(ctx, small["sc"], small["cfg"], walk=False)
        on = _render(ctx, small["sc"], small["cfg"], walk=True)
        assert _same(on, off) and on[3]["shadow_rays"] > 0
        out = (C.c_uint64 * 6)()
        assert capi.load().pt_fog_walk_stats(ctx.handle, out) == capi.PT_ERR_STATE
        _render(ctx, big["sc"], big["cfg"], spp=1)
        assert hip.fog_walk_stats(ctx)["shadow_walked"] > 0
        with pytest.raises(capi.PtError) as e:
            _render(ctx, big["sc"], big["cfg"], walk=False, spp=1)
        assert e.value.code == capi.PT_ERR_INVALID and "BVH" in str(e.value)
        assert capi.load().pt_fog_walk_stats(ctx.handle, out) == capi.PT_ERR_STATE
        again = _render(ctx, small["sc"], small["cfg"], walk=False)  # the context goes on
        assert _same(again, off)
        with pytest.raises(capi.PtError) as e:  # GL shading on the BVH path stays refused, with the walk on too
            _render(ctx, big["sc"], big["cfg"], walk=True, spp=1, shading="gl")
        assert e.value.code == capi.PT_ERR_INVALID and "GL shading" in str(e.value)
        assert capi.load().pt_fog_walk_stats(ctx.handle, out) == capi.PT_ERR_STATE  # refused first: no walk frame was opened
        assert _same(_render(ctx, small["sc"], small["cfg"], walk=False), off)
