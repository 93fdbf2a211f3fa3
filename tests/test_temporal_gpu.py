"""Temporal accumulation on the MI355X (pt_temporal, temporal_kernel and the a-trous kernels behind it).  The reference
is the restatement tests/temporal_reference.c, fed the context's own accum, m2, counts and features of every frame and the oracle's
camera (ora_camera_setup) of the moved scene.  Frames are small (40 x 24: two tiles, ragged, 2 x 3 blocks of the kernel; 37 x 21).
Every comparison runs with contexts of its own."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import adaptive_support as ad
import atrous_support as at
import temporal_support as ts
from moments_support import H, W

pytestmark = pytest.mark.gpu

SPP = 16
SCENES = [("example_simple", 4), ("gpu_showcase", 8), ("metal_glass_room", 6)]  # glass, emitters; the last two have a thin lens


@pytest.fixture(autouse=True, scope="module")
def _built(gpu_ctx):
    return gpu_ctx


def _frame(ctx, name, f, w, h, spp, depth, k=4, **kw):
    """Frame f of the sequence (the camera moved by f steps, seed 1 + f) on ctx with moments on and k feature samples: the inputs
    the restatement takes -- dict(S, Q, n, feats, cam) -- read back from the context."""
    from path_trace_golang_amd import hip

    img, acc, m2 = np.zeros((h, w, 4), np.uint8), np.zeros((h, w, 3)), np.zeros((h, w, 3))
    hip.render(ts.product_scene(name, f), hip.RenderConfig(w, h, spp, depth, 1 + f), img, None, acc, ctx=ctx, moments=m2, features=k, **kw)
    feats = None
    if k > 0:
        feats = tuple(np.zeros((h, w, 3)) for _ in range(3))
        hip.read_features(ctx, *feats)
    return dict(S=acc, Q=m2, n=spp, feats=feats, cam=ts.camera_of(ts.ora_scene(name, f), w, h), img=img)


def _check(ctx, ref, fr, w, h, flt, tag, counts=None, **tcfg):
    """pt_temporal on ctx's frame against the restatement's next frame."""
    got = ts.gpu_frame(ctx, ts.temporal_config(**tcfg), at.atrous_config(**flt) if flt is not None else None, w, h)
    want = ref.frame(fr["S"], fr["Q"], fr["n"], fr["feats"], fr["cam"], counts, flt, **tcfg)
    ts.assert_same_frame(got, want, tag)
    T = flt.get("iterations", 5) if flt is not None else 0
    assert got["iterations"] == T and got["launches"] == (T + 4 if flt is not None else 3) and got["temporal_ms"] > 0
    return got


# ---------------------------------------------------------------- 1. sequences against the restatement
@pytest.mark.parametrize("name,depth", SCENES)
def test_moving_sequences_match_the_restatement(name, depth):
    from path_trace_golang_amd import capi, hip

    ref = ts.Accumulator("ref")
    with capi.Context(ndev=1) as ctx:
        for f in range(3):
            fr = _frame(ctx, name, f, W, H, SPP, depth)
            got = _check(ctx, ref, fr, W, H, dict(), (name, f))
            nz = hip.noise_estimate(ctx)
            assert abs(got["noise_before"] - nz["noise"]) <= 1e-9 * max(1.0, nz["noise"])
            assert got["bad_pixels"] == 0
            if f == 0:
                assert got["reprojected"] == 0 and got["disoccluded"] == 0 and np.all(got["hist_len"] == 1)
            else:
                assert got["reprojected"] > W * H // 2 and got["reprojected"] + got["disoccluded"] == W * H
                assert got["hist_len"].max() == f + 1 and got["noise_blended"] < got["noise_before"]
    ref.close()


def test_an_odd_size_and_no_filter_match_the_restatement():
    from path_trace_golang_amd import capi

    name, depth = "metal_glass_room", 6
    for (w, h), flt in (((37, 21), dict()), ((W, H), None)):
        ref = ts.Accumulator("ref")
        with capi.Context(ndev=1) as ctx:
            for f in range(3):
                got = _check(ctx, ref, _frame(ctx, name, f, w, h, SPP, depth), w, h, flt, (w, h, flt, f))
            if flt is None:  # the output is the stored history
                assert at.same_bits(got["mean"], got["hist_mean"]) and at.same_bits(got["var"], got["hist_var"])
                assert got["noise_after"] == got["noise_blended"]
        ref.close()


def test_an_adaptive_second_frame_matches_the_restatement():
    from path_trace_golang_amd import capi, hip

    name, depth, _, cap, step, _, target = ad.CASE
    ref = ts.Accumulator("ref")
    with capi.Context(ndev=1) as ctx:
        _check(ctx, ref, _frame(ctx, name, 0, W, H, SPP, depth), W, H, dict(), "first")
        img, acc, m2, counts, _, _, st = ad.render_adaptive(ctx, ts.product_scene(name, 1), W, H, cap, depth, 2, target, step, 2, features=4)
        assert len(np.unique(counts)) >= 3 and counts.min() >= 2
        feats = tuple(np.zeros((H, W, 3)) for _ in range(3))
        hip.read_features(ctx, *feats)
        fr = dict(S=acc, Q=m2, n=0, feats=feats, cam=ts.camera_of(ts.ora_scene(name, 1), W, H))
        got = _check(ctx, ref, fr, W, H, dict(), "adaptive", counts=counts)
        assert got["reprojected"] > W * H // 2
    ref.close()


# ---------------------------------------------------------------- 2. a pure read of the frame
def test_a_call_between_two_steps_changes_nothing_and_is_not_repeated():
    from path_trace_golang_amd import capi, hip

    name, depth = "gpu_showcase", 8
    L = capi.load()
    flat = hip.FlatScene(ts.product_scene(name, 0))
    pc = hip.pt_config(hip.RenderConfig(W, H, SPP, depth, 1))
    out = {}
    for preview in (False, True):
        with capi.Context(ndev=1) as ctx:
            hip.set_moments(ctx, True)
            hip.set_features(ctx, 4)
            capi.check(L.pt_begin(ctx.handle, C.byref(flat.c), C.byref(pc)))
            done = C.c_int32(0)
            capi.check(L.pt_step(ctx.handle, 8, C.byref(done)))
            if preview:
                first = ts.gpu_frame(ctx, None, hip.AtrousConfig(), W, H)
                assert first["reprojected"] == 0 and np.all(first["hist_len"] == 1)
                # the same frame at the same count: it would be blended into itself
                assert L.pt_temporal(ctx.handle, None, None, None, 0, None, None, None) == capi.PT_ERR_STATE
                assert b"already accumulated" in L.pt_last_error()
                again = tuple(np.zeros(s, t) for s, t in (((H, W, 3), np.float64), ((H, W), np.float64), ((H, W), np.int32)))
                hip.temporal_read(ctx, *again)
                assert at.same_bits(again[0], first["hist_mean"]) and at.same_bits(again[1], first["hist_var"]) and np.array_equal(again[2], first["hist_len"])
            capi.check(L.pt_step(ctx.handle, SPP, C.byref(done)))
            assert done.value == SPP
            if preview:  # after the next step the call is valid again, and finds the 8-sample state of every pixel at its own place
                second = ts.gpu_frame(ctx, None, hip.AtrousConfig(), W, H)
                assert second["reprojected"] + second["disoccluded"] == W * H and second["reprojected"] > W * H * 3 // 4
            img, acc, m2 = np.zeros((H, W, 4), np.uint8), np.zeros((H, W, 3)), np.zeros((H, W, 3))
            capi.check(L.pt_read(ctx.handle, img.ctypes.data_as(C.c_void_p), W * 4, acc.ctypes.data_as(C.c_void_p)))
            st = capi.PtStats()
            capi.check(L.pt_end(ctx.handle, C.byref(st)))
            hip.read_moments(ctx, m2)
            out[preview] = (img, acc, m2, st.as_dict())
    a, b = out[False], out[True]
    assert np.array_equal(a[0], b[0]) and at.same_bits(a[1], b[1]) and at.same_bits(a[2], b[2])
    for key in ("samples", "segments", "exit_scans", "draws", "trace_launches"):
        assert a[3][key] == b[3][key], key


# ---------------------------------------------------------------- 3. refusals
def test_refusals_leave_the_context_usable_and_the_history_unchanged():
    from path_trace_golang_amd import capi, hip

    name, depth = "example_simple", 4
    L = capi.load()
    st = capi.PtTemporalStats()

    def call(ctx, cfg=None, flt=None):
        return L.pt_temporal(ctx.handle, C.byref(cfg) if cfg is not None else None, C.byref(flt) if flt is not None else None, None, 0,
                             None, None, C.byref(st))

    def history(ctx):
        a = (np.zeros((H, W, 3)), np.zeros((H, W)), np.zeros((H, W), np.int32))
        hip.temporal_read(ctx, *a)
        return a

    def same(a, b):
        return at.same_bits(a[0], b[0]) and at.same_bits(a[1], b[1]) and np.array_equal(a[2], b[2])

    ref = ts.Accumulator("ref")
    with capi.Context(ndev=1) as ctx:
        # before any frame; reading an empty history
        assert call(ctx) == capi.PT_ERR_STATE and L.pt_last_error()
        assert L.pt_temporal_read(ctx.handle, None, None, None) == capi.PT_ERR_STATE and b"empty" in L.pt_last_error()
        _check(ctx, ref, _frame(ctx, name, 0, W, H, SPP, depth), W, H, dict(), "first")
        kept = history(ctx)
        # bad arguments
        d = ts.T_DEFAULTS
        for bad in (dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=float("nan")), dict(max_len=0), dict(tol_z=-1.0), dict(tol_a=-1.0),
                    dict(tol_z=float("nan")), dict(n_min=float("nan")), dict(tol_a=float("nan"))):
            c = dict(d, **bad)
            cfg = capi.PtTemporalConfig(c["alpha"], c["tol_z"], c["n_min"], c["tol_a"], c["max_len"], 0)
            assert call(ctx, cfg) == capi.PT_ERR_INVALID and L.pt_last_error(), bad
        for bad in (dict(iterations=7), dict(sigma_l=0.0), dict(sigma_n=-0.1)):
            c = dict(at.DEFAULTS, **bad)
            assert call(ctx, None, capi.PtAtrousConfig(c["iterations"], 0, c["sigma_l"], c["sigma_n"], c["sigma_z"], c["sigma_a"])) == capi.PT_ERR_INVALID
        buf = np.zeros((H, W, 4), np.uint8)
        assert L.pt_temporal(ctx.handle, None, None, buf.ctypes.data_as(C.c_void_p), W * 4 - 1, None, None, None) == capi.PT_ERR_INVALID
        assert same(history(ctx), kept)
        # features off
        _frame(ctx, name, 1, W, H, SPP, depth, k=0)
        assert call(ctx) == capi.PT_ERR_STATE and b"features off" in L.pt_last_error()
        assert same(history(ctx), kept)
        # moments off
        hip.render(ts.product_scene(name, 1), hip.RenderConfig(W, H, SPP, depth, 2), buf, ctx=ctx)
        assert call(ctx) == capi.PT_ERR_STATE and b"moments off" in L.pt_last_error()
        # one sample per pixel: no variance
        _frame(ctx, name, 1, W, H, 1, depth)
        assert call(ctx) == capi.PT_ERR_STATE and b"2 samples" in L.pt_last_error()
        assert same(history(ctx), kept)
        # GL shading
        sc = ts.product_scene(name, 1)
        hip.render(sc, hip.RenderConfig(W, H, 2, depth, 2), buf, ctx=ctx, shading="gl", moments=np.zeros((H, W, 3)))
        assert call(ctx) == capi.PT_ERR_STATE and b"GL shading" in L.pt_last_error()
        assert same(history(ctx), kept)
        # ... and the context goes on where the history stood: the second frame of the sequence against the restatement
        got = _check(ctx, ref, _frame(ctx, name, 1, W, H, SPP, depth), W, H, dict(), "after the refusals")
        assert got["reprojected"] > W * H // 2 and got["hist_len"].max() == 2
    ref.close()


# ---------------------------------------------------------------- 4. the history's size, reset, and hip.render
def test_a_size_change_and_a_reset_start_a_new_history():
    from path_trace_golang_amd import capi, hip

    name, depth = "example_simple", 4
    ref = ts.Accumulator("ref")
    with capi.Context(ndev=1) as ctx:
        _check(ctx, ref, _frame(ctx, name, 0, W, H, SPP, depth), W, H, dict(), "40 x 24")
        got = _check(ctx, ref, _frame(ctx, name, 1, 37, 21, SPP, depth), 37, 21, dict(), "37 x 21")
        assert got["reprojected"] == 0 and got["disoccluded"] == 0 and np.all(got["hist_len"] == 1) and got["mean_len"] == 1.0
        got = _check(ctx, ref, _frame(ctx, name, 2, 37, 21, SPP, depth), 37, 21, dict(), "37 x 21 again")
        assert got["reprojected"] > 0
        got = _check(ctx, ref, _frame(ctx, name, 3, W, H, SPP, depth), W, H, dict(), "40 x 24 again")  # a larger frame after a smaller one
        assert got["reprojected"] == 0 and np.all(got["hist_len"] == 1)
        hip.temporal_reset(ctx)
        ref.reset()
        assert capi.load().pt_temporal_read(ctx.handle, None, None, None) == capi.PT_ERR_STATE
        got = _check(ctx, ref, _frame(ctx, name, 4, W, H, SPP, depth), W, H, dict(), "after the reset")
        assert got["reprojected"] == 0 and np.all(got["hist_len"] == 1)
    ref.close()


def test_render_with_temporal_returns_the_accumulated_image():
    from path_trace_golang_amd import capi, hip

    name, depth = "example_simple", 4
    ref = ts.Accumulator("ref")
    with capi.Context(ndev=1) as ctx:
        for f in range(2):
            img, acc, m2 = np.zeros((H, W, 4), np.uint8), np.zeros((H, W, 3)), np.zeros((H, W, 3))
            st = hip.render(ts.product_scene(name, f), hip.RenderConfig(W, H, SPP, depth, 1 + f), img, None, acc, ctx=ctx, moments=m2,
                            temporal=hip.TemporalConfig(), atrous=hip.AtrousConfig(iterations=3))
            feats = tuple(np.zeros((H, W, 3)) for _ in range(3))
            hip.read_features(ctx, *feats)  # k = 4 came with the argument
            want = ref.frame(acc, m2, SPP, feats, ts.camera_of(ts.ora_scene(name, f), W, H), None, dict(iterations=3))
            assert np.array_equal(img, want["rgba"]) and "atrous" not in st
            assert st["temporal"]["iterations"] == 3 and st["temporal"]["reprojected"] == want["reprojected"]
        assert st["temporal"]["reprojected"] > W * H // 2
        plain = np.zeros((H, W, 4), np.uint8)
        st = hip.render(ts.product_scene(name, 1), hip.RenderConfig(W, H, SPP, depth, 2), plain, ctx=ctx)
        assert "temporal" not in st and not np.array_equal(plain, img)  # off again without the argument
    ref.close()


# ---------------------------------------------------------------- 5. more than one device, and past the clamp
def test_three_virtual_devices_give_the_history_of_one():
    """pt_temporal gathers its inputs to devices[0] first: a moving sequence on three virtual devices (40 x 24 is two tiles, so the
    third holds none) against the one-device context and against the restatement."""
    from path_trace_golang_amd import capi

    name, depth = "metal_glass_room", 6
    ref = ts.Accumulator("ref")
    with capi.Context(ndev=1) as one, capi.Context(devices=[0, 0, 0]) as three:
        for f in range(3):
            fr1 =_frame(one, name, f, W, H, SPP, depth)
            fr3 = _frame(three, name, f, W, H, SPP, depth)
            assert at.same_bits(fr1["S"], fr3["S"]) and at.same_bits(fr1["Q"], fr3["Q"])
            assert all(at.same_bits(x, y) for x, y in zip(fr1["feats"], fr3["feats"]))
            a = ts.gpu_frame(one, ts.temporal_config(), at.atrous_config(), W, H)
            b = _check(three, ref, fr3, W, H, dict(), ("three devices", f))
            ts.assert_same_frame(a, b, ("one device vs three", f))
            for k in ("noise_before", "noise_blended", "noise_after", "mean_len"):  # devices[0] runs the kernels over the gathered planes: the same tree
                assert a[k] == b[k], (f, k)
        assert b["reprojected"] > W * H // 2 and b["hist_len"].max() == 3
    ref.close()


def test_eight_frames_pass_the_clamp_and_reach_the_exponential_regime():
    """example_simple at 37 x 21, 8 spp, alpha = 0.5, max_len = 3: from the fourth frame on len' is cut to 3, and alpha > 1 / (L + 1)
    holds wherever L >= 2 -- the product's own pt_temporal against the restatement, frame by frame."""
    from path_trace_golang_amd import capi

    name, depth, w, h, spp = "example_simple", 4, 37, 21, 8
    tcfg = dict(alpha=0.5, max_len=3)
    ref = ts.Accumulator("ref")
    with capi.Context(ndev=1) as ctx:
        for f in range(8):
            got = _check(ctx, ref, _frame(ctx, name, f, w, h, spp, depth), w, h, dict(), (name, f), **tcfg)
            assert got["hist_len"].max() == min(f + 1, 3) and got["bad_pixels"] == 0
            if f > 0:
                assert got["reprojected"] > w * h // 2 and got["reprojected"] + got["disoccluded"] == w * h
        assert np.count_nonzero(got["hist_len"] == 3) > w * h // 2
    ref.close()
