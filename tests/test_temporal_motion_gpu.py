"""Displaced reprojection on the MI355X (pt_temporal_set_motion, pt_temporal_motion_stats, step 4a in temporal_kernel).
Rendered sequences: one sphere and one box moved per frame, with and without the camera moving; pt_temporal with the table against
the host build of csrc/pt_temporal.h fed the context's own sums, features and ids -- the comparison test_temporal_clip_gpu.py makes.
The kernel by itself: tests/temporal_motion_probe.hip launches temporal_kernel on planted index planes and tables."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import atrous_support as at
import denoise_probe_support as dp
import temporal_motion_support as tm
import temporal_support as ts

pytestmark = pytest.mark.gpu

W, H, SPP, DEPTH = 37, 21, 16, 4
FILTERS = (None, dict())


@pytest.fixture(autouse=True, scope="module")
def _built(gpu_ctx):
    return gpu_ctx


def _product_scene(doc):
    from path_trace_golang_amd import scene

    return scene.Scene.decode(doc)


def _frame(ctx, name, f, cam, w=W, h=H):
    """Frame f of the moving sequence (seed 1 + f) on ctx with moments, 4 feature samples and object ids: the inputs the host build
    takes, read back from the context, and the table against frame f - 1."""
    from oracle import ora
    from path_trace_golang_amd import hip

    doc = tm.motion_doc(name, f, cam=cam)
    img, acc, m2 = np.zeros((h, w, 4), np.uint8), np.zeros((h, w, 3)), np.zeros((h, w, 3))
    hip.render(_product_scene(doc), hip.RenderConfig(w, h, SPP, DEPTH, 1 + f), img, None, acc, ctx=ctx, moments=m2, features=4, object_ids=True)
    feats = tuple(np.zeros((h, w, 3)) for _ in range(3))
    hip.read_features(ctx, *feats)
    ids = np.full((h, w), -9, np.int32)
    hip.read_object_ids(ctx, ids)
    osc = ora.Scene(doc)
    assert np.array_equal(ids, tm.oracle_ids(osc, w, h, 1 + f)[0])
    delta = tm.doc_delta(tm.motion_doc(name, f - 1, cam=cam), doc) if f > 0 else None
    return dict(S=acc, Q=m2, n=SPP, feats=feats, cam=ts.camera_of(osc, w, h), ids=ids, delta=delta, doc=doc)


def _gpu(ctx, flt, w=W, h=H):
    """pt_temporal on ctx's frame, the history read back, pt_temporal_clip_stats and pt_temporal_motion_stats."""
    from path_trace_golang_amd import hip

    got = ts.gpu_frame(ctx, ts.temporal_config(), at.atrous_config(**flt) if flt is not None else None, w, h)
    got["clipped"] = hip.temporal_clip_stats(ctx)["clipped"]
    got["motion"] = hip.temporal_motion_stats(ctx)
    got["moved"], got["moved_reprojected"] = got["motion"]["moved"], got["motion"]["moved_reprojected"]
    return got


def _history(ctx, w=W, h=H):
    from path_trace_golang_amd import hip

    a = (np.zeros((h, w, 3)), np.zeros((h, w)), np.zeros((h, w), np.int32))
    hip.temporal_read(ctx, *a)
    return a


def _same_history(a, b):
    return at.same_bits(a[0], b[0]) and at.same_bits(a[1], b[1]) and np.array_equal(a[2], b[2])


# ---------------------------------------------------------------- 1. rendered sequences
@pytest.mark.parametrize("gamma", [0.0, tm.GAMMA])
@pytest.mark.parametrize("name,cam,devices", [("example_simple", 0.0, None), ("metal_glass_room", 1.0, None), ("example_simple", 1.0, [0, 0, 0])],
                         ids=["objects", "objects and camera, thin lens", "objects and camera, three virtual devices"])
def test_rendered_sequences_match_the_host_build(name, cam, devices, gamma):
    from path_trace_golang_amd import capi, hip

    for flt in FILTERS:
        host = tm.MotionAccumulator("host")
        with (capi.Context(devices=devices) if devices else capi.Context(ndev=1)) as ctx:
            hip.temporal_set_clip(ctx, gamma)
            for f in range(3):
                fr = _frame(ctx, name, f, cam)
                if f > 0:
                    hip.temporal_set_motion(ctx, fr["delta"])
                got = _gpu(ctx, flt)
                want = host.frame(fr["S"], fr["Q"], fr["n"], fr["feats"], fr["cam"], None, flt, gamma, fr["ids"] if f > 0 else None, fr["delta"])
                tm.assert_same_frame(got, want, (name, cam, devices, gamma, flt, f))
                assert got["motion"] == dict(objects=len(fr["delta"]) if f > 0 else 0, moved=want["moved"], moved_reprojected=want["moved_reprojected"])
                print(name, cam, flt, gamma, f, "moved %d, %d of them reprojected, %d reprojected" % (want["moved"], want["moved_reprojected"], want["reprojected"]))
                if f > 0:
                    assert got["reprojected"] > W * H // 2 and 0 < got["moved_reprojected"] <= got["moved"]
        host.close()


def test_the_table_is_one_shot_and_a_zero_table_is_no_table():
    from path_trace_golang_amd import capi, hip

    name, cam = "example_simple", 0.0
    host = tm.MotionAccumulator("host")
    with capi.Context(ndev=1) as ctx, capi.Context(ndev=1) as plain:
        hip.temporal_set_clip(ctx, tm.GAMMA)
        hip.temporal_set_clip(plain, tm.GAMMA)
        # a table with the history empty is consumed: frame 0 runs as a first frame, frame 1 without a table
        fr = _frame(ctx, name, 0, cam)
        hip.temporal_set_motion(ctx, np.full((19, 3), 0.5))
        got = _gpu(ctx, None)
        tm.assert_same_frame(got, host.frame(fr["S"], fr["Q"], fr["n"], fr["feats"], fr["cam"], None, None, tm.GAMMA, fr["ids"], np.full((19, 3), 0.5)), 0)
        assert got["motion"]["objects"] == 19 and got["moved"] > 0 and got["moved_reprojected"] == 0 and got["reprojected"] == 0
        fr = _frame(ctx, name, 1, cam)
        got = _gpu(ctx, None)
        tm.assert_same_frame(got, host.frame(fr["S"], fr["Q"], fr["n"], fr["feats"], fr["cam"], None, None, tm.GAMMA), "consumed")
        assert got["motion"] == dict(objects=0, moved=0, moved_reprojected=0)
        # a zero table: the bits of a context that never heard of motion (object ids off there)
        for f in range(2):
            doc = tm.motion_doc(name, f, cam=cam)
            img, acc, m2 = np.zeros((H, W, 4), np.uint8), np.zeros((H, W, 3)), np.zeros((H, W, 3))
            hip.render(_product_scene(doc), hip.RenderConfig(W, H, SPP, DEPTH, 1 + f), img, None, acc, ctx=plain, moments=m2, features=4)
            want = ts.gpu_frame(plain, ts.temporal_config(), at.atrous_config(), W, H)
        hip.temporal_reset(ctx)
        for f in range(2):
            _frame(ctx, name, f, cam)
            hip.temporal_set_motion(ctx, np.zeros((19, 3)))
            got = _gpu(ctx, dict())
        ts.assert_same_frame(got, want, "zero table")
        assert got["motion"] == dict(objects=19, moved=0, moved_reprojected=0)
        # NULL and 0 clear a pending table
        fr = _frame(ctx, name, 2, cam)
        hip.temporal_set_motion(ctx, fr["delta"])
        hip.temporal_set_motion(ctx, None)
        assert _gpu(ctx, None)["motion"]["objects"] == 0
        # after pt_temporal_reset nothing of the last table is left
        fr = _frame(ctx, name, 3, cam)
        hip.temporal_set_motion(ctx, fr["delta"])
        hip.temporal_reset(ctx)
        with pytest.raises(capi.PtError):
            hip.temporal_motion_stats(ctx)  # the history is empty
        got = _gpu(ctx, None)
        assert got["motion"] == dict(objects=0, moved=0, moved_reprojected=0) and got["reprojected"] == 0
    host.close()


def test_every_refusal_leaves_the_context_the_history_and_the_table_as_they_were(oracle):
    import moments_support as ms
    from conftest import render_vs_oracle
    from path_trace_golang_amd import capi, hip

    name, cam = "example_simple", 0.0
    L = capi.load()
    host = tm.MotionAccumulator("host")
    dp_ = C.POINTER(C.c_double)
    with capi.Context(ndev=1) as ctx:
        assert L.pt_temporal_motion_stats(ctx.handle, C.byref(capi.PtTemporalMotionStats())) == capi.PT_ERR_STATE and b"empty" in L.pt_last_error()
        for f in range(2):
            fr = _frame(ctx, name, f, cam)
            if f:
                hip.temporal_set_motion(ctx, fr["delta"])
            got = _gpu(ctx, None)
            tm.assert_same_frame(got, host.frame(fr["S"], fr["Q"], fr["n"], fr["feats"], fr["cam"], None, None, 0.0, fr["ids"] if f else None, fr["delta"]), f)
        kept, stats = _history(ctx), hip.temporal_motion_stats(ctx)
        # the setter's refusals: the pending table (set here, good) survives them
        fr = _frame(ctx, name, 2, cam)
        hip.temporal_set_motion(ctx, fr["delta"])
        for bad in (float("nan"), float("inf"), -float("inf")):
            d = fr["delta"].copy()
            d[7, 1] = bad
            assert L.pt_temporal_set_motion(ctx.handle, d.ctypes.data_as(dp_), len(d)) == capi.PT_ERR_INVALID and b"finite" in L.pt_last_error(), bad
        assert L.pt_temporal_set_motion(ctx.handle, fr["delta"].ctypes.data_as(dp_), -1) == capi.PT_ERR_INVALID
        assert L.pt_temporal_motion_stats(ctx.handle, None) == capi.PT_ERR_INVALID
        # pt_temporal's: the table's length against the scene's
        hip.temporal_set_motion(ctx, fr["delta"][:18])
        assert L.pt_temporal(ctx.handle, None, None, None, 0, None, None, None) == capi.PT_ERR_INVALID and b"18 objects" in L.pt_last_error()
        hip.temporal_set_motion(ctx, fr["delta"])
        # ... a frame without object ids (the table stays pending through the refusal, and through the next frame)
        doc = tm.motion_doc(name, 2, cam=cam)
        img = np.zeros((H, W, 4), np.uint8)
        hip.render(_product_scene(doc), hip.RenderConfig(W, H, SPP, DEPTH, 3), img, ctx=ctx, moments=np.zeros((H, W, 3)), features=4)
        assert L.pt_temporal(ctx.handle, None, None, None, 0, None, None, None) == capi.PT_ERR_STATE and b"object ids off" in L.pt_last_error()
        assert _same_history(_history(ctx), kept) and hip.temporal_motion_stats(ctx) == stats
        # the frame again with ids: the pending table is used now, against the host build
        fr = _frame(ctx, name, 2, cam)
        got = _gpu(ctx, None)
        tm.assert_same_frame(got, host.frame(fr["S"], fr["Q"], fr["n"], fr["feats"], fr["cam"], None, None, 0.0, fr["ids"], fr["delta"]), "after the refusals")
        assert got["motion"]["objects"] == 19 and got["moved_reprojected"] > 0
        # an oracle-exact frame afterwards
        hip.set_object_ids(ctx, False)
        hip.set_features(ctx, 0)
        hip.set_moments(ctx, False)
        sc = _product_scene(tm.motion_doc(name, 0))
        render_vs_oracle(ctx, sc, oracle.render(ms.ora_scene(name), W, H, 3, DEPTH, seed=5), W, H, 3, DEPTH, 5, tag="at the end")
    host.close()


def test_render_with_temporal_motion_returns_the_displaced_image():
    from oracle import ora
    from path_trace_golang_amd import capi, hip

    name, cam = "example_simple", 1.0
    host = tm.MotionAccumulator("host")
    with capi.Context(ndev=1) as ctx:
        prev = None
        for f in range(3):
            doc = tm.motion_doc(name, f, cam=cam)
            sc = _product_scene(doc)
            delta = hip.scene_motion(prev, sc) if prev is not None else None
            img, acc, m2 = np.zeros((H, W, 4), np.uint8), np.zeros((H, W, 3)), np.zeros((H, W, 3))
            st = hip.render(sc, hip.RenderConfig(W, H, SPP, DEPTH, 1 + f), img, None, acc, ctx=ctx, moments=m2, temporal=hip.TemporalConfig(),
                            atrous=hip.AtrousConfig(iterations=3), temporal_clip=tm.GAMMA, temporal_motion=delta)
            feats = tuple(np.zeros((H, W, 3)) for _ in range(3))
            hip.read_features(ctx, *feats)
            ids = np.zeros((H, W), np.int32)
            if delta is not None:
                hip.read_object_ids(ctx, ids)
            want = host.frame(acc, m2, SPP, feats, ts.camera_of(ora.Scene(doc), W, H), None, dict(iterations=3), tm.GAMMA, ids if delta is not None else None, delta)
            assert np.array_equal(img, want["rgba"])
            if delta is not None:
                assert st["temporal"]["objects"] == 19 and st["temporal"]["moved"] == want["moved"] > 0
                assert st["temporal"]["moved_reprojected"] == want["moved_reprojected"] > 0
            else:
                assert "moved" not in st["temporal"]
            prev = sc
    host.close()


# ---------------------------------------------------------------- 2. the kernel by itself
PW, PH = 70, 37
TABLE = np.array([[100.0, 0.0, 0.0],        # 0: carries P outside the previous view
                  [0.0, 0.0, -10.0],        # 1: ... behind the previous camera (it stands at z = 5 and looks down -z)
                  [1e300, -1e300, 1e300],   # 2: huge and finite
                  [0.12, 0.0, 0.0],         # 3 and 4: three quarters of a pixel at the wall, opposite ways
                  [-0.12, 0.0, 0.0],
                  [0.0, 0.0, 0.0]])         # 5: in the table and not moved


def planted():
    """The first two frames of the "unmoved" wall sequence (70 x 37; the wall fills columns 16-53 of rows 6-30, the sky the rest)
    with an index plane for the second: columns 0-15, the sky's, claim object 3; 16-19 object 7 of a table of 6; 20-25 object 0, 26-31
    object 1, 32-37 object 2; 38-69 objects 3 and 4 in alternating columns (both in every wave); rows 26-36 object 5; row 8 nothing
    (-1)."""
    f0, f1 = (dict(f) for f in dp.sequence("unmoved")[:2])
    ids = np.full((PH, PW), -1, np.int32)
    ids[:, 0:16] = 3
    ids[:, 16:20] = 7
    ids[:, 20:26] = 0
    ids[:, 26:32] = 1
    ids[:, 32:38] = 2
    ids[:, 38:70:2] = 3
    ids[:, 39:70:2] = 4
    ids[26:, :] = 5
    ids[8, :] = -1
    f1["ids"], f1["delta"] = ids, TABLE
    return [f0, f1]


@pytest.mark.parametrize("gamma", [0.0, tm.GAMMA])
def test_the_kernel_on_the_planted_index_plane(gamma):
    frames = planted()
    ids = frames[1]["ids"]
    none = tm.restate_sequence(frames, gamma, motion="none")[-1]
    want = tm.restate_sequence(frames, gamma)[-1]
    for flt in (None, dict(iterations=3)):
        host = tm.run_sequence("host", frames, flt, gamma)
        got = tm.run_sequence("gpu", frames, flt, gamma)
        for k, (a, b) in enumerate(zip(got, host)):
            tm.assert_same_frame(a, b, (gamma, flt, k))
            assert not np.isnan(a["hist_var"][b["hist_len"] > 0]).any()  # nothing of the 0xFF fill is left where a pixel is good
        if flt is None:
            tm.assert_same_model(host[-1], want, (gamma, "host build against the restatement"))
    good_hit = (frames[1]["feats"][2][..., 1] > 0) & (want["hist_len"] > 0)
    assert good_hit.sum() > 900  # the wall's 38 x 25 pixels less the planted bad ones
    # outside the table, -1 and the zero row: the undisplaced path
    same = np.isin(ids, (-1, 7, 5)) | ~good_hit
    assert all((good_hit & (ids == o)).sum() > 16 for o in (-1, 7, 5)) and (~good_hit & (ids == 3)).sum() > 100
    assert at.same_bits(want["place"][same], none["place"][same]) and at.same_bits(want["mean"][same], none["mean"][same])
    # out of the previous view, behind the previous camera, huge: disoccluded, every one
    lost = np.isin(ids, (0, 1, 2)) & good_hit
    assert all((good_hit & (ids == o)).sum() > 50 for o in (0, 1, 2)) and np.isnan(want["place"][lost]).all() and (want["hist_len"][lost] == 1).all()
    assert np.isfinite(none["place"][lost]).all()
    # opposite deltas side by side in one wave: each lands its own way
    for o, sign in ((3, -1.0), (4, 1.0)):
        sel = (ids == o) & good_hit
        shift = want["place"][sel][:, 0] - none["place"][sel][:, 0]
        assert sel.sum() > 50 and np.all(sign * shift > 0.5) and np.all(sign * shift < 1.0), (o, shift.min(), shift.max())
    assert want["moved"] == int((np.isin(ids, (0, 1, 2, 3, 4)) & good_hit).sum())
    assert 0 < want["moved_reprojected"] <= int((np.isin(ids, (3, 4)) & good_hit).sum())


def test_a_zero_table_against_null_pointers_on_the_kernel():
    frames = [dict(f) for f in dp.sequence("sideways")[:3]]
    for f in frames[1:]:
        f["ids"] = (np.arange(PW * PH, dtype=np.int32).reshape(PH, PW) % 9) - 2  # -2 .. 6 against a table of 5
        f["delta"] = np.zeros((5, 3))
    for flt in (None, dict(iterations=3)):
        zero = tm.run_sequence("gpu", frames, flt, tm.GAMMA, motion="zero")
        none = tm.run_sequence("gpu", frames, flt, tm.GAMMA, motion="none")
        for k, (a, b) in enumerate(zip(zero, none)):
            tm.assert_same_frame(a, b, (flt, k))
            assert a["moved"] == 0
        assert none[-1]["reprojected"] > PW * PH // 2


def test_the_probe_refuses_what_the_setter_refuses():
    fr = dp.sequence("sideways 33 x 9")[0]
    ids = np.zeros((9, 33), np.int32)
    acc = tm.MotionAccumulator("gpu")
    for bad in (float("nan"), float("inf"), -float("inf")):
        d = np.zeros((4, 3))
        d[2, 1] = bad
        with pytest.raises(RuntimeError, match="status -8"):
            acc.frame(fr["S"], fr["Q"], fr["n"], fr["feats"], fr["cam"], None, None, 0.0, ids, d)
    with pytest.raises(RuntimeError, match="status -8"):
        acc.frame(fr["S"], fr["Q"], fr["n"], fr["feats"], fr["cam"], None, None, 0.0, ids, np.zeros((4, 3)), ndelta=-1)
    with pytest.raises(RuntimeError, match="status -9"):
        acc.frame(fr["S"], fr["Q"], fr["n"], fr["feats"], fr["cam"], None, None, 0.0, None, np.zeros((4, 3)))
    assert acc.read(33, 9) is None
    # NULL or 0 is a call without a table
    a = acc.frame(fr["S"], fr["Q"], fr["n"], fr["feats"], fr["cam"], None, None, 0.0, ids, np.zeros((4, 3)), ndelta=0)
    assert a["moved"] == 0 and acc.read(33, 9) is not None
    acc.close()
