"""The history clip of pt_temporal on the MI355X (step 7a of csrc/pt_temporal.h).  The reference of every comparison
is the restatement tests/temporal_clip_reference.c.  Rendered frames: pt_temporal after pt_temporal_set_clip, fed the context's own
sums and features (37 x 21: ragged, 2 x 3 blocks of the kernel).  The kernel by itself: tests/temporal_clip_probe.hip launches
temporal_kernel with C.clip_gamma set on the synthetic sequences of test_temporal_clip_cpu.py."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import atrous_support as at
import denoise_probe_support as dp
import temporal_clip_support as tc
import temporal_support as ts

pytestmark = pytest.mark.gpu

W, H, SPP = 37, 21, 16
SCENES = [("test_scene", 4), ("metal_glass_room", 6)]
FILTERS = (None, dict())


@pytest.fixture(autouse=True, scope="module")
def _built(gpu_ctx):
    return gpu_ctx


def _frame(ctx, name, f, depth):
    """Frame f of the moving sequence (seed 1 + f) on ctx with moments on and 4 feature samples: the inputs the restatement takes,
    read back from the context."""
    from path_trace_golang_amd import hip

    img, acc, m2 = np.zeros((H, W, 4), np.uint8), np.zeros((H, W, 3)), np.zeros((H, W, 3))
    hip.render(ts.product_scene(name, f), hip.RenderConfig(W, H, SPP, depth, 1 + f), img, None, acc, ctx=ctx, moments=m2, features=4)
    feats = tuple(np.zeros((H, W, 3)) for _ in range(3))
    hip.read_features(ctx, *feats)
    return dict(S=acc, Q=m2, n=SPP, feats=feats, cam=ts.camera_of(ts.ora_scene(name, f), W, H))


def _gpu(ctx, flt):
    """pt_temporal on ctx's frame (the context's gamma), the history read back and pt_temporal_clip_stats."""
    from path_trace_golang_amd import hip

    got = ts.gpu_frame(ctx, ts.temporal_config(), at.atrous_config(**flt) if flt is not None else None, W, H)
    got["clip"] = hip.temporal_clip_stats(ctx)
    got["clipped"] = got["clip"]["clipped"]
    return got


def _history(ctx):
    from path_trace_golang_amd import hip

    a = (np.zeros((H, W, 3)), np.zeros((H, W)), np.zeros((H, W), np.int32))
    hip.temporal_read(ctx, *a)
    return a


def _same_history(a, b):
    return at.same_bits(a[0], b[0]) and at.same_bits(a[1], b[1]) and np.array_equal(a[2], b[2])


# ---------------------------------------------------------------- 1. rendered frames
@pytest.mark.parametrize("devices", [None, [0, 0, 0]], ids=["one device", "three virtual devices"])
@pytest.mark.parametrize("name,depth", SCENES)
def test_rendered_sequences_match_the_restatement(name, depth, devices):
    from path_trace_golang_amd import capi, hip

    for flt in FILTERS:
        ref = tc.ClipAccumulator("ref")
        with (capi.Context(devices=devices) if devices else capi.Context(ndev=1)) as ctx:
            hip.temporal_set_clip(ctx, tc.GAMMA)
            for f in range(3):
                fr = _frame(ctx, name, f, depth)
                got = _gpu(ctx, flt)
                want = ref.frame(fr["S"], fr["Q"], fr["n"], fr["feats"], fr["cam"], None, flt, tc.GAMMA)
                tc.assert_same_frame(got, want, (name, devices, flt, f))
                assert got["clip"] == dict(gamma=tc.GAMMA, clipped=want["clipped"], reprojected=want["reprojected"])
                print(name, flt, f, "clipped %d of %d" % (want["clipped"], want["reprojected"]))
                if f > 0:
                    assert got["reprojected"] > W * H // 2
                    if name == "test_scene":
                        assert 0 < got["clipped"] < got["reprojected"]
        ref.close()


def test_gamma_zero_after_a_set_and_back_is_a_context_that_never_called_the_setter():
    from path_trace_golang_amd import capi, hip

    name, depth = "test_scene", 4
    L = capi.load()
    ref = tc.ClipAccumulator("ref")
    with capi.Context(ndev=1) as plain, capi.Context(ndev=1) as ctx:
        assert L.pt_temporal_clip_stats(ctx.handle, C.byref(capi.PtTemporalClipStats())) == capi.PT_ERR_STATE and b"empty" in L.pt_last_error()
        hip.temporal_set_clip(ctx, tc.GAMMA)
        hip.temporal_set_clip(ctx, 0.0)
        for f in range(3):
            _frame(plain, name, f, depth)
            fr = _frame(ctx, name, f, depth)
            a = ts.gpu_frame(plain, ts.temporal_config(), at.atrous_config(), W, H)
            b = _gpu(ctx, dict())
            ts.assert_same_frame(b, a, ("set and back", f))
            assert b["clip"] == dict(gamma=0.0, clipped=0, reprojected=a["reprojected"])
            tc.assert_same_frame(b, ref.frame(fr["S"], fr["Q"], fr["n"], fr["feats"], fr["cam"], None, dict(), 0.0), ("gamma 0", f))
        # gamma may change between frames of one history: the fourth frame runs clipped on the unclipped history
        hip.temporal_set_clip(ctx, tc.GAMMA)
        fr = _frame(ctx, name, 3, depth)
        got = _gpu(ctx, dict())
        tc.assert_same_frame(got, ref.frame(fr["S"], fr["Q"], fr["n"], fr["feats"], fr["cam"], None, dict(), tc.GAMMA), "gamma changed")
        assert got["clip"]["gamma"] == tc.GAMMA and got["clipped"] > 0
    ref.close()


def test_a_refused_setter_call_leaves_the_context_and_the_history_as_they_were():
    from path_trace_golang_amd import capi, hip

    name, depth = "metal_glass_room", 6
    L = capi.load()
    ref = tc.ClipAccumulator("ref")
    with capi.Context(ndev=1) as ctx:
        hip.temporal_set_clip(ctx, tc.GAMMA)
        for f in range(2):
            fr = _frame(ctx, name, f, depth)
            got = _gpu(ctx, None)
            tc.assert_same_frame(got, ref.frame(fr["S"], fr["Q"], fr["n"], fr["feats"], fr["cam"], None, None, tc.GAMMA), f)
        kept, stats = _history(ctx), hip.temporal_clip_stats(ctx)
        for bad in (float("nan"), -1.0, float("inf"), -float("inf"), -1e-300):
            assert L.pt_temporal_set_clip(ctx.handle, bad) == capi.PT_ERR_INVALID and b"gamma" in L.pt_last_error(), bad
            with pytest.raises(capi.PtError):
                hip.temporal_set_clip(ctx, bad)
        assert L.pt_temporal_clip_stats(ctx.handle, None) == capi.PT_ERR_INVALID and L.pt_last_error()
        assert _same_history(_history(ctx), kept) and hip.temporal_clip_stats(ctx) == stats
        # ... and gamma is still 2.5: the third frame against the restatement
        fr = _frame(ctx, name, 2, depth)
        got = _gpu(ctx, None)
        tc.assert_same_frame(got, ref.frame(fr["S"], fr["Q"], fr["n"], fr["feats"], fr["cam"], None, None, tc.GAMMA), "after the refusals")
        assert got["clip"]["gamma"] == tc.GAMMA
        hip.temporal_reset(ctx)
        assert L.pt_temporal_clip_stats(ctx.handle, C.byref(capi.PtTemporalClipStats())) == capi.PT_ERR_STATE
    ref.close()


def test_render_with_temporal_clip_returns_the_clipped_image():
    from path_trace_golang_amd import capi, hip

    name, depth = "test_scene", 4
    ref = tc.ClipAccumulator("ref")
    with capi.Context(ndev=1) as ctx:
        for f in range(2):
            img, acc, m2 = np.zeros((H, W, 4), np.uint8), np.zeros((H, W, 3)), np.zeros((H, W, 3))
            st = hip.render(ts.product_scene(name, f), hip.RenderConfig(W, H, SPP, depth, 1 + f), img, None, acc, ctx=ctx, moments=m2,
                            temporal=hip.TemporalConfig(), atrous=hip.AtrousConfig(iterations=3), temporal_clip=tc.GAMMA)
            feats = tuple(np.zeros((H, W, 3)) for _ in range(3))
            hip.read_features(ctx, *feats)
            want = ref.frame(acc, m2, SPP, feats, ts.camera_of(ts.ora_scene(name, f), W, H), None, dict(iterations=3), tc.GAMMA)
            assert np.array_equal(img, want["rgba"])
            assert st["temporal"]["clipped"] == want["clipped"] and st["temporal"]["reprojected"] == want["reprojected"]
        assert st["temporal"]["clipped"] > 0
    ref.close()


# ---------------------------------------------------------------- 2. the kernel by itself
PROBE_GAMMAS = (1e-6, 0.5, 2.5, 1e300)
PROBE_FILTERS = (dict(iterations=0), dict(iterations=3), None)


def _probe_against_the_restatement(key, frames):
    ran = 0
    for gamma in PROBE_GAMMAS:
        for flt in PROBE_FILTERS:
            want = tc.reference_run(key, frames, flt, gamma)
            got = tc.run_sequence("gpu", frames, flt, gamma)
            for k, (x, y) in enumerate(zip(got, want)):
                tc.assert_same_frame(x, y, (key, gamma, flt, k))
                assert not np.isnan(x["hist_var"][y["hist_len"] > 0]).any()  # nothing of the 0xFF fill is left where a pixel is good
            ran += 1
            if gamma == 1e-6:
                assert all(o["clipped"] > 0 for o in got[1:])
    return ran


@pytest.mark.parametrize("name", ["sideways", "sideways 33 x 9", "sideways 97 x 71"])
def test_the_kernel_on_the_moving_walls(name):
    """70 x 37, 33 x 9 and 97 x 71: four frames of the sideways move, every gamma with a filter of 0 and of 3 iterations and without
    one, against the restatement: output, history and len bit for bit, counts exactly, figures to 1e-9."""
    frames = dp.sequence(name)[:4]
    assert _probe_against_the_restatement(name, frames) == 12
    all_clipped = tc.reference_run(name, frames, None, 1e-6)
    none_clipped = tc.reference_run(name, frames, None, 1e300)
    assert all(o["clipped"] == o["reprojected"] > 0 for o in all_clipped[1:]) and all(o["clipped"] == 0 for o in none_clipped)


def test_the_kernel_on_the_planted_special_cases():
    """The frames of test_every_case_of_the_clip_on_synthetic_frames: zero variance on both sides, c_r exactly on a bound, s <= 0
    through prep's clamp, bad pixels beside clipped ones; per-pixel counts."""
    assert _probe_against_the_restatement("planted", tc.planted_frames()) == 12


def test_the_probe_refuses_what_the_setter_refuses():
    fr = dp.sequence("sideways 33 x 9")[0]
    acc = tc.ClipAccumulator("gpu")
    for bad in (float("nan"), -1.0, float("inf")):
        with pytest.raises(RuntimeError, match="status -7"):
            acc.frame(fr["S"], fr["Q"], fr["n"], fr["feats"], fr["cam"], None, None, bad)
    assert acc.read(33, 9) is None
    acc.close()
