"""First-hit features and the a-trous filter for GL-shaded frames on the MI355X (pt_set_shading_features; gl_feature_kernel,
gl_feature_bvh_kernel, atrous_finish_gl_kernel).  The planes and ids against tests/gl_features_reference.c bit for bit --
every k, every chunking, between two pt_steps, on the BVH path with a host-built, a device-built and a refitted tree --, the radiance
sums and GL's counters undisturbed, pt_atrous and pt_atrous_halves on such a frame against tests/atrous_reference.c fed the frame's own
sums, GL's finish of the filtered mean, and what stays refused.  40 x 24: two tiles wide, ragged right and bottom edges, lanes
outside the frame.  (test_gl_features_cpu.py shows from the reference alone that these scenes hold every class of first hit.)"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import atrous_support as at
import gl_features_support as gf
import glwalk_support as gw
import halves_support as hs

pytestmark = pytest.mark.gpu

GLC = ("paths", "segments", "shadow_rays", "probe_rays", "draws")


@pytest.fixture(autouse=True, scope="module")
def _torch_before_libptcore():
    import torch  # noqa: F401  (one HIP runtime in the process, as in test_glshade_gpu.py)


@pytest.fixture(scope="module")
def ctx():
    from path_trace_golang_amd import capi

    with capi.Context(ndev=1) as c:
        yield c


def _frame(ctx, case, k=0, on=True, chunk=0, passes=None, ids=None, **kw):
    """One GL frame of the case: dict(img, acc, m2, st = pt_stats, gst = pt_shading_last_stats)."""
    from path_trace_golang_amd import hip

    w, h, p, depth, seed = case["cfg"]
    p = p if passes is None else passes
    img, acc, m2 = np.zeros((h, w, 4), np.uint8), np.zeros((h, w, 3)), np.zeros((h, w, 3))
    st = hip.render(case["sc"], hip.RenderConfig(w, h, p, depth, seed, chunk), img, None, acc, ctx=ctx, shading="gl", moments=m2,
                    features=k, object_ids=bool(k) if ids is None else ids, shading_features=on, **kw)
    return dict(img=img, acc=acc, m2=m2, st=st, gst=hip.shading_last_stats(ctx))


def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _same_frame(a, b):
    return np.array_equal(a["img"], b["img"]) and _bits(a["acc"], b["acc"]) and _bits(a["m2"], b["m2"]) and all(a["gst"][k] == b["gst"][k] for k in GLC)


def _case(name):
    return gf.fuzz_case(int(name[4:]), gf.W, gf.H, gf.PASSES, gpu=True) if name.startswith("fuzz") else gf.shipped_case(name)


# ---------------------------------------------------------------- 1. planes and ids, sums undisturbed
@pytest.mark.parametrize("name", ["gpu_showcase", "test_scene", "fuzz2", "fuzz3"])
def test_planes_and_ids_equal_the_reference_and_the_sums_are_undisturbed(ctx, name):
    case = _case(name)
    w, h, passes, depth, _ = case["cfg"]
    assert (w, h, passes, depth) == (40, 24, 3, 3)
    ref_img, ref_acc, ref_st = gf.gl_reference(case)
    off = _frame(ctx, case, on=False)  # today's frame
    zero = _frame(ctx, case, k=0, on=True)  # the switch on, nothing asked for
    assert _same_frame(zero, off)
    for k in gf.KS:
        ref = gf.ref_features(case, k=k)
        for chunk in (1, 2, 0):
            fr = _frame(ctx, case, k=k, chunk=chunk)
            got = gf.read_planes(ctx, w, h)
            tag = (name, k, chunk)
            assert gf.same_planes(ref, got), (tag, [int(np.count_nonzero(a != b)) for a, b in zip(ref, got)])
            assert np.all(got[2][..., 2] == 16 * min(k, passes)), tag
            # the radiance: the frame without features, and the reference's
            assert _same_frame(fr, off), tag
            print(tag, "accum bit-equal to gr_render:", _bits(fr["acc"], ref_acc), "max rel",
                  float(np.max(np.abs(fr["acc"] - ref_acc) / np.maximum(np.abs(ref_acc), 1e-300))))
            assert np.array_equal(fr["img"], ref_img), (tag, int(np.count_nonzero(fr["img"] != ref_img)))
            assert _bits(fr["acc"], ref_acc), tag
            assert tuple(fr["gst"][c] for c in GLC) == tuple(ref_st[c] for c in GLC), tag
    assert int(np.count_nonzero(gf.ref_features(case, k=1)[3] >= 0)) > 50  # (ids were compared, and they are not all misses)


def test_planes_between_two_steps(ctx):
    from path_trace_golang_amd import capi, hip

    case = gf.shipped_case("gpu_showcase")
    sc, (w, h, passes, depth, seed) = case["sc"], case["cfg"]
    L = capi.load()
    flat = hip.FlatScene(sc)
    pc = hip.pt_config(hip.RenderConfig(w, h, passes, depth, seed, 1))
    hip.set_shading(ctx, "gl", sc)
    hip.set_shading_features(ctx, True)
    hip.set_moments(ctx, True)
    hip.set_halves(ctx, False)
    hip.set_features(ctx, 5)
    hip.set_object_ids(ctx, True)
    capi.check(L.pt_begin(ctx.handle, C.byref(flat.c), C.byref(pc)))
    try:
        assert L.pt_set_shading_features(ctx.handle, 0) == capi.PT_ERR_STATE  # not while a frame is open
        assert b"pt_set_shading_features while a frame is open" in L.pt_last_error()
        done = C.c_int32(0)
        capi.check(L.pt_step(ctx.handle, 1, C.byref(done)))
        got = gf.read_planes(ctx, w, h)
        assert gf.same_planes(gf.ref_features(case, passes=1, k=5), got) and np.all(got[2][..., 2] == 16)
        capi.check(L.pt_step(ctx.handle, 2, C.byref(done)))
        got = gf.read_planes(ctx, w, h)
        assert done.value == 3 and gf.same_planes(gf.ref_features(case, passes=3, k=5), got) and np.all(got[2][..., 2] == 48)
        img, acc = np.zeros((h, w, 4), np.uint8), np.zeros((h, w, 3))
        capi.check(L.pt_read(ctx.handle, img.ctypes.data_as(C.c_void_p), w * 4, acc.ctypes.data_as(C.c_void_p)))
    finally:
        capi.check(L.pt_end(ctx.handle, C.byref(capi.PtStats())))
    ref_img, ref_acc, _ = gf.gl_reference(case)
    assert np.array_equal(img, ref_img) and _bits(acc, ref_acc)
    hip.set_object_ids(ctx, False)
    hip.set_features(ctx, 0)
    hip.set_shading(ctx, "cpu")


# ---------------------------------------------------------------- 2. the BVH path
def test_bvh_path_planes_ids_and_walk_stats():
    from path_trace_golang_amd import capi, hip

    case = gf.room_case()
    w, h = case["cfg"][:2]
    ns, nb, _ = gw.kinds(case)
    assert (w, h) == (33, 20) and ns > 128 and nb > 128
    ref = gf.ref_features(case, k=2)
    ref_img, ref_acc, _ = gf.gl_reference(case)
    with capi.Context(ndev=1) as c1:
        plain = _frame(c1, case, on=False, shading_walk=True)
        ws0 = hip.shading_walk_stats(c1)
        for chunk in (0, 1):
            fr = _frame(c1, case, k=2, chunk=chunk, shading_walk=True)
            assert gf.same_planes(ref, gf.read_planes(c1, w, h)), chunk
            assert _same_frame(fr, plain) and hip.shading_walk_stats(c1) == ws0, chunk  # the GL pass's counters alone
        assert np.array_equal(plain["img"], ref_img) and _bits(plain["acc"], ref_acc)
        # without pt_set_shading_walk the scene stays refused, and the context goes on
        with pytest.raises(capi.PtError) as e:
            _frame(c1, case, k=2, shading_walk=False)
        assert e.value.code == capi.PT_ERR_INVALID and "GL shading is not available for scenes on the BVH path" in str(e.value)
        assert _same_frame(_frame(c1, case, k=2, shading_walk=True), plain)
        assert gf.same_planes(ref, gf.read_planes(c1, w, h))
    with capi.Context(ndev=1) as c2:  # the tree built on the device
        fr = _frame(c2, case, k=2, shading_walk=True, bvh_build="device")
        assert hip.bvh_build_stats(c2)["device_builds"] >= 1
        assert gf.same_planes(ref, gf.read_planes(c2, w, h)) and _same_frame(fr, plain)
    moved = gw.moved(gw.room_case())  # a refitted tree: three objects moved
    moved = gw.with_cfg(moved, passes=case["cfg"][2], depth=case["cfg"][3], seed=case["cfg"][4])
    with capi.Context(ndev=1) as c3:
        _frame(c3, case, k=2, shading_walk=True, bvh_refit=1.25)
        _frame(c3, moved, k=2, shading_walk=True, bvh_refit=1.25)
        assert hip.bvh_refit_stats(c3)["last_action"] == 2  # it was a refit
        got = gf.read_planes(c3, w, h)
    mref = gf.ref_features(moved, k=2)
    assert gf.same_planes(mref, got) and not gf.same_planes(mref, ref)


# ---------------------------------------------------------------- 3. the filter
@pytest.mark.parametrize("k", [1, 0])
def test_atrous_on_a_gl_frame_equals_the_reference(ctx, k):
    case = gf.shipped_case("gpu_showcase")
    w, h, passes, _, _ = case["cfg"]
    fr = _frame(ctx, case, k=k)
    feats = gf.ref_features(case, k=1)[:3] if k else None
    if k:
        assert gf.same_planes(gf.ref_features(case, k=1), gf.read_planes(ctx, w, h))
    for it in (0, 1, 5):
        ref = at.ref_filter(fr["acc"], fr["m2"], passes, None, feats, iterations=it)
        got = at.gpu_run(ctx, at.atrous_config(iterations=it), w, h)
        tag = (k, it)
        for key in ("mean", "var"):
            assert at.same_bits(got[key], ref[key]), (tag, key, int(np.count_nonzero(got[key] != ref[key])))
        assert got["bad_pixels"] == ref["bad_pixels"] == 0, tag
        for key in ("noise_before", "noise_after"):
            print(tag, key, got[key], ref[key])
            assert abs(got[key] - ref[key]) <= 1e-9 * max(1.0, abs(ref[key])), (tag, key, got[key], ref[key])
        assert np.array_equal(got["rgba"], gf.tonemapped(ref["mean"])), (tag, int(np.count_nonzero(got["rgba"] != gf.tonemapped(ref["mean"]))))
        if it == 0:
            assert np.array_equal(got["rgba"], fr["img"]), tag  # pt_read's image of the frame
        else:
            assert not np.array_equal(got["mean"], fr["acc"] / passes), tag  # it filtered
    again = _frame(ctx, case, k=k)  # a pure read: the next frame is the same frame
    assert _same_frame(again, fr)


def test_atrous_halves_on_a_gl_frame_equals_the_reference(ctx):
    case = gf.shipped_case("gpu_showcase")
    w, h = case["cfg"][:2]
    fr = _frame(ctx, case, k=1, passes=4, halves=True)
    feats = gf.ref_features(case, passes=4, k=1)
    assert gf.same_planes(feats, gf.read_planes(ctx, w, h))
    SA, QA, SB, QB = hs.read_halves(ctx, w, h)
    assert np.allclose(SA + SB, fr["acc"], rtol=1e-12, atol=0)  # the halves are the frame's own passes
    for it in (0, 5):
        ref = hs.ref_pair(SA, QA, SB, QB, 4, None, feats[:3], iterations=it)
        got = hs.gpu_pair(ctx, at.atrous_config(iterations=it), w, h)
        hs.assert_same_pair(got, ref, tag=str(it))
    ref0 = hs.ref_pair(SA, QA, SB, QB, 4, None, None, iterations=5)  # the feature terms were on
    assert not at.same_bits(ref0["mean"], ref["mean"])


# ---------------------------------------------------------------- 4. what stays refused
def test_refusals_leave_the_context_usable(ctx):
    from path_trace_golang_amd import capi, hip

    case = gf.shipped_case("test_scene")
    w, h = case["cfg"][:2]
    good = _frame(ctx, case, k=1)
    ref = gf.ref_features(case, k=1)

    def still_good():
        assert _same_frame(_frame(ctx, case, k=1), good) and gf.same_planes(ref, gf.read_planes(ctx, w, h))

    # pt_temporal on such a frame: its projection is the CPU camera's
    with pytest.raises(capi.PtError) as e:
        hip.temporal(ctx, None, None, np.zeros((h, w, 4), np.uint8))
    assert e.value.code == capi.PT_ERR_STATE and "GL shading" in str(e.value) and "pt_temporal" in str(e.value), str(e.value)
    still_good()
    # adaptive sampling with GL shading
    with pytest.raises((capi.PtError, ValueError)) as e:
        _frame(ctx, case, k=1, noise=0.5, noise_step=1, adaptive=True)
    assert "adaptive sampling: not available with GL shading" in str(e.value), str(e.value)
    still_good()
    # with the switch off everything is refused as before, by the pinned messages
    with pytest.raises(capi.PtError) as e:
        _frame(ctx, case, k=1, on=False)
    assert e.value.code == capi.PT_ERR_INVALID and "features: not available with GL shading (pt_set_shading), where a sample is a pass of 16 paths" in str(e.value)
    _frame(ctx, case, on=False)
    with pytest.raises(capi.PtError) as e:
        hip.atrous(ctx, None, np.zeros((h, w, 4), np.uint8))
    assert e.value.code == capi.PT_ERR_STATE and "not available for a frame rendered with GL shading (pt_set_shading)" in str(e.value)
    still_good()
    # object ids without features
    with pytest.raises(capi.PtError) as e:
        _frame(ctx, case, k=0, ids=True)
    assert e.value.code == capi.PT_ERR_INVALID and "object ids: the frame needs features on" in str(e.value)
    still_good()
    # a CPU-model frame on the same context ignores the switch
    from oracle import ora

    img, acc = np.zeros((h, w, 4), np.uint8), np.zeros((h, w, 3))
    hip.render(case["sc"], hip.RenderConfig(w, h, 2, 3, 1), img, None, acc, ctx=ctx, shading_features=True)
    cpu = ora.render(case["ora"], w, h, 2, 3, seed=1, want=("rgba",))
    assert np.array_equal(img, cpu["rgba"])
    still_good()
