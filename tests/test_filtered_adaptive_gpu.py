"""Adaptive sampling by the filtered frame's pooled noise on the MI355X (pt_set_adaptive_filtered, block_err_kernel,
block_pool_kernel, keep_from_map_kernel).  The yardstick is filtered_adaptive_support.predict -- the restatement of
the pair filter and of the block rule -- fed with plain frames of the same context at every check's count: the counts plane is
exact and both figures are bit for bit after every step, since every sum of the model has a stated order.  On the committed case
the counts are also the map predicted from the oracle's samples on the CPU.  Then self-consistency (every block bit-equal to the
plain frame of its count), invariance under chunk size, scan form, stepping and device count, the refusals, and the rule off.

Frames of at most 70 x 45, cap 32, step 8, k = 4."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import adaptive_support as ad
import atrous_support as at
import filtered_adaptive_support as fa
import halves_support as hs
from adaptive_support import bits
from conftest import scene_path
from moments_support import H, W

pytestmark = pytest.mark.gpu

CAP, STEP, DEPTH, SEED, K = 32, 8, 4, 1, 4
BIG = (ad.GATHER_W, ad.GATHER_H)  # 70 x 45: six tiles, ragged on both edges


@pytest.fixture(autouse=True, scope="module")
def _built(gpu_ctx):
    return gpu_ctx


def _scene(name):
    from path_trace_golang_amd import scene

    return scene.load(scene_path(name))


def plain_frames(ctx, sc, w, h, depth=DEPTH, seed=SEED, chunk=0, **kw):
    """{n: dict(rgba, accum, m2, halves)} of the plain frames of ctx at every check's count, and their feature sums."""
    from path_trace_golang_amd import hip

    out, feats = {}, None
    for n in range(STEP, CAP + 1, STEP):
        img, acc, m2 = np.zeros((h, w, 4), np.uint8), np.zeros((h, w, 3)), np.zeros((h, w, 3))
        hip.render(sc, hip.RenderConfig(w, h, n, depth, seed, chunk), img, None, acc, ctx=ctx, moments=m2, halves=True, features=K, **kw)
        out[n] = dict(rgba=img, accum=acc, m2=m2, halves=hs.read_halves(ctx, w, h))
        if feats is None:
            feats = tuple(np.zeros((h, w, 3)) for _ in range(3))
            hip.read_features(ctx, *feats)
    return out, feats


def run_rule(ctx, sc, w, h, target, pool=1, chunk=0, min_spp=0, stepped=True, depth=DEPTH, seed=SEED, **kw):
    """One frame with the rule on through hip.render.  stepped: the host steps pt_begin / pt_step / pt_read itself and after every step
    the counts, the figures and the plain finish are recorded (the last record follows pt_end); else pt_render steps inside."""
    from path_trace_golang_amd import capi, hip

    img, acc, m2 = np.zeros((h, w, 4), np.uint8), np.zeros((h, w, 3)), np.zeros((h, w, 3))
    counts = np.full((h, w), 0xFFFFFFFF, np.uint32)
    steps = []

    def progress():
        c = np.zeros((h, w), np.uint32)
        hip.read_sample_counts(ctx, c)
        pooled, own = np.full(fa.grid(w, h), -1.0), np.full(fa.grid(w, h), -1.0)
        try:
            checks = hip.read_block_figures(ctx, pooled, own)
        except capi.PtError as e:
            assert e.code == capi.PT_ERR_STATE
            checks = 0
        steps.append(dict(counts=c, rgba=img.copy(), pooled=pooled, own=own, checks=checks, state=hip.adaptive_state(ctx)))

    st = hip.render(sc, hip.RenderConfig(w, h, CAP, depth, seed, chunk), img, progress if stepped else None, acc, ctx=ctx, moments=m2,
                    atrous=hip.AtrousConfig(), filtered_adaptive=target, pool=pool, noise_step=STEP, min_spp=min_spp, counts=counts, **kw)
    return dict(filtered=img, accum=acc, m2=m2, counts=counts, steps=steps, st=st, halves=hs.read_halves(ctx, w, h))


def predicted(frames, feats, target, pool=1, min_spp=0):
    return fa.predict({n: f["halves"] for n, f in frames.items()}, feats, target, STEP, min_spp, CAP, pool)


def splitting_target(frames, feats, pool=1):
    """A target that stops some blocks at the second check and not others: the median pooled figure of the plain 16-sample frame."""
    r = hs.ref_pair(*frames[2 * STEP]["halves"], 2 * STEP, None, feats)
    h, w = r["err"].shape
    return float(np.median(fa.restate_blocks(r["mean"], r["err"], np.zeros((h, w)), pool, 0.0)["pooled"]))


@pytest.fixture(scope="module")
def small(_built):
    """The committed case's frame, 40 x 24: one context, its plain frames and feature sums (read-only)."""
    from path_trace_golang_amd import capi

    with capi.Context(ndev=1) as ctx:
        sc = _scene(fa.CASE[0])
        frames, feats = plain_frames(ctx, sc, W, H)
        yield ctx, sc, frames, feats


@pytest.fixture(scope="module")
def big(_built):
    """70 x 45 on one device: plain frames, feature sums, the splitting target, the prediction and the rule's frame."""
    from path_trace_golang_amd import capi

    w, h = BIG
    with capi.Context(ndev=1) as ctx:
        sc = _scene("example_simple")
        frames, feats = plain_frames(ctx, sc, w, h)
        target = splitting_target(frames, feats)
        yield dict(ctx=ctx, sc=sc, frames=frames, feats=feats, target=target, pred=predicted(frames, feats, target),
                   got=run_rule(ctx, sc, w, h, target))


def check_against(pred, got, w, h, target, min_spp=0):
    """The counts plane and pt_read_block_figures after every step, pt_adaptive_state at the end, against the predictor."""
    hist = pred["history"]
    steps = got["steps"]
    assert len(steps) == len(hist) + 1  # one record per check, and the one after pt_end
    decided = 0
    for i, (rec, want) in enumerate(zip(steps, hist)):
        n = STEP * (i + 1)
        assert np.array_equal(rec["counts"], ad.expand(want, w, h)), (n, rec["counts"][::8, ::8].tolist(), want.tolist())
        if n >= max(min_spp, 4):
            decided += 1
            pooled, own = pred["figures"][n]
            assert at.same_bits(rec["pooled"], pooled), (n, "pooled", float(np.abs(rec["pooled"] - pooled).max()))
            assert at.same_bits(rec["own"], own), (n, "own", float(np.abs(rec["own"] - own).max()))
        assert rec["checks"] == decided, (n, rec["checks"])
    assert np.array_equal(got["counts"], ad.expand(pred["counts"], w, h))
    a = got["st"]["adaptive"]
    assert a["active_blocks"] == int(pred["active"].sum()) and a["samples"] == pred["samples"] == got["st"]["samples"]
    assert a["worst_active"] == pred["worst"]  # the largest P_B among the active blocks, the same bits
    assert got["st"]["block_checks"] == decided
    ad.check_state(got["st"], got["counts"], CAP)


# ---------------------------------------------------------------- 1. counts and figures against the predictor
def test_the_case_is_the_frame_predicted_from_the_oracle(small):
    ctx, sc, frames, feats = small
    name, depth, seed, cap, step, min_spp, k, pool = fa.CASE
    assert (depth, seed, cap, step, k) == (DEPTH, SEED, CAP, STEP, K)
    got = run_rule(ctx, sc, W, H, fa.CASE_TARGET, pool, min_spp=min_spp)
    assert got["counts"][::8, ::8].tolist() == fa.CASE_MAP  # the map computed on the CPU from the oracle's samples
    assert got["st"]["samples"] == fa.CASE_SAMPLES and got["st"]["adaptive"]["active_blocks"] == fa.CASE_ACTIVE
    pred = predicted(frames, feats, fa.CASE_TARGET, pool, min_spp)
    assert pred["by_neighbours"].any()  # a block the pool alone kept alive, on the device's frames too
    check_against(pred, got, W, H, fa.CASE_TARGET, min_spp)


@pytest.mark.parametrize("pool", [0, 2, 4])
def test_other_pool_radii_against_the_predictor(small, pool):
    ctx, sc, frames, feats = small
    target = splitting_target(frames, feats, pool)
    pred = predicted(frames, feats, target, pool)
    assert (pred["counts"] < CAP).any()
    check_against(pred, run_rule(ctx, sc, W, H, target, pool), W, H, target)


def test_a_ragged_frame_of_six_tiles_against_the_predictor(big):
    w, h = BIG
    pred = big["pred"]
    assert (pred["counts"] < CAP).any() and pred["active"].any() and np.unique(pred["counts"]).size >= 3
    check_against(pred, big["got"], w, h, big["target"])


def test_min_spp_delays_the_first_decision(small):
    ctx, sc, frames, feats = small
    pred = predicted(frames, feats, fa.CASE_TARGET, 1, 20)
    got = run_rule(ctx, sc, W, H, fa.CASE_TARGET, 1, min_spp=20)
    assert got["steps"][0]["checks"] == 0 and got["steps"][1]["checks"] == 0 and got["steps"][2]["checks"] == 1
    assert np.isinf(got["steps"][0]["state"]["worst_active"])  # no figure before the first decision
    check_against(pred, got, W, H, fa.CASE_TARGET, 20)


# ---------------------------------------------------------------- 2. self-consistency
def test_every_block_is_the_plain_frame_of_its_count(big):
    """adaptive_support.check_self_consistent's property with the new rule, the four half sums included; the image is pt_atrous on
    the full sums with the per-pixel counts."""
    from path_trace_golang_amd import hip

    w, h = BIG
    got, frames = big["got"], big["frames"]
    counts = got["counts"]
    assert counts.min() >= STEP and counts.max() == CAP
    plain = got["steps"][-1]["rgba"]  # pt_read's finish of the frame as it ended
    for n in sorted(int(v) for v in np.unique(counts)):
        sel = counts == n
        f = frames[n]
        assert np.array_equal(plain[sel], f["rgba"][sel]), ("rgba", n)
        assert np.array_equal(bits(got["accum"])[sel], bits(f["accum"])[sel]), ("accum", n)
        assert np.array_equal(bits(got["m2"])[sel], bits(f["m2"])[sel]), ("m2", n)
        for k, name in enumerate(("SA", "QA", "SB", "QB")):
            assert np.array_equal(bits(got["halves"][k])[sel], bits(f["halves"][k])[sel]), (name, n)
    ref = at.ref_filter(got["accum"], got["m2"], 0, counts, big["feats"])
    mean = np.zeros((h, w, 3))
    img = np.zeros((h, w, 4), np.uint8)
    hip.atrous(big["ctx"], hip.AtrousConfig(), img, mean)  # the frame is still the rule's: the last one finished on the context
    assert at.same_bits(mean, ref["mean"]) and np.array_equal(img, got["filtered"])


# ---------------------------------------------------------------- 3. invariance
@pytest.mark.parametrize("chunk", [3, 5])
def test_the_chunk_size_changes_nothing(big, chunk):
    w, h = BIG
    got = run_rule(big["ctx"], big["sc"], w, h, big["target"], chunk=chunk)
    assert got["st"]["spp_chunk"] == chunk
    check_against(big["pred"], got, w, h, big["target"])
    assert np.array_equal(bits(got["accum"]), bits(big["got"]["accum"]))


def test_pt_render_steps_to_the_same_frame(big):
    w, h = BIG
    got = run_rule(big["ctx"], big["sc"], w, h, big["target"], stepped=False)
    assert np.array_equal(got["counts"], big["got"]["counts"]) and np.array_equal(got["filtered"], big["got"]["filtered"])
    assert np.array_equal(bits(got["accum"]), bits(big["got"]["accum"]))
    assert got["st"]["adaptive"] == big["got"]["st"]["adaptive"] and got["st"]["block_checks"] == big["got"]["st"]["block_checks"]


def test_three_devices_decide_what_one_decides(big):
    """devices = [0, 0, 0] at 70 x 45: the six tiles go 2, 2, 2, so a window spans blocks owned by different devices; the map
    reaches every device by the same path."""
    from path_trace_golang_amd import capi

    w, h = BIG
    with capi.Context(devices=[0, 0, 0]) as ctx:
        got = run_rule(ctx, big["sc"], w, h, big["target"])
    assert got["st"]["num_devices"] == 3
    check_against(big["pred"], got, w, h, big["target"])
    for k in ("accum", "m2", "filtered"):
        assert np.array_equal(got[k].view(np.uint8), big["got"][k].view(np.uint8)), k


def test_the_split_and_the_all_in_one_form_decide_the_same(monkeypatch):
    """metal_glass_room (glass: split rounds and the nested tail by default) against PTCORE_SPLIT_ROUNDS=0, pinhole, 40 x 24."""
    import copy

    from path_trace_golang_amd import capi

    sc = copy.deepcopy(_scene("metal_glass_room"))
    sc.camera.aperture = 0.0
    with capi.Context(ndev=1) as ctx:
        frames, feats = plain_frames(ctx, sc, W, H, depth=6)
        target = splitting_target(frames, feats)
        pred = predicted(frames, feats, target)
        a = run_rule(ctx, sc, W, H, target, depth=6)
        assert a["st"]["trace_split_launches"] > 0
    monkeypatch.setenv("PTCORE_SPLIT_ROUNDS", "0")
    with capi.Context(ndev=1) as ctx:  # read by pt_create
        b = run_rule(ctx, sc, W, H, target, depth=6)
        assert b["st"]["trace_split_launches"] == 0
    assert (pred["counts"] < CAP).any()
    check_against(pred, a, W, H, target)
    check_against(pred, b, W, H, target)
    assert np.array_equal(bits(a["accum"]), bits(b["accum"]))


# ---------------------------------------------------------------- 4. refusals
def test_refusals_leave_the_context_usable(small):
    from path_trace_golang_amd import capi, hip

    ctx, sc, frames, feats = small
    L = capi.load()
    flat = hip.FlatScene(sc)
    pc = hip.pt_config(hip.RenderConfig(W, H, CAP, DEPTH, SEED))
    img = np.zeros((H, W, 4), np.uint8)
    dp = C.POINTER(C.c_double)
    pooled = np.zeros(fa.grid(W, H))

    def usable():
        got = run_rule(ctx, sc, W, H, fa.CASE_TARGET, stepped=False)
        assert got["counts"][::8, ::8].tolist() == fa.CASE_MAP

    def good(pool=1, **kw):
        return capi.PtAdaptiveFiltered(hip.AtrousConfig(**kw).c(), pool, 0)

    # the rule without an adaptive frame: refused before anything is launched
    hip.set_adaptive(ctx, None)
    hip.set_adaptive_filtered(ctx, None, 1)
    for call in (lambda: L.pt_begin(ctx.handle, C.byref(flat.c), C.byref(pc)),
                 lambda: L.pt_render(ctx.handle, C.byref(flat.c), C.byref(pc), img.ctypes.data_as(C.c_void_p), W * 4, None, None, None, None)):
        assert call() == capi.PT_ERR_INVALID and b"pt_set_adaptive first" in L.pt_last_error()
    assert L.pt_step(ctx.handle, 1, None) == capi.PT_ERR_STATE  # no frame was opened
    usable()
    # bad arguments: the pool, and pt_atrous's own refusals of the filter
    for bad, text in ((good(5), b"pool must be 0..4"), (good(-1), b"pool must be 0..4"), (good(sigma_l=0.0), b"sigma_l must be > 0"),
                      (good(sigma_n=-1.0), b"sigma_l must be > 0"), (good(sigma_z=float("nan")), b"sigma_l must be > 0"),
                      (good(iterations=7), b"iterations must be 0..6")):
        assert L.pt_set_adaptive_filtered(ctx.handle, C.byref(bad)) == capi.PT_ERR_INVALID and text in L.pt_last_error(), text
    usable()  # (a refused setting leaves the one in force)
    # GL shading: the refusal of adaptive frames, as it was
    hip.set_adaptive(ctx, fa.CASE_TARGET, 0, STEP)
    hip.set_adaptive_filtered(ctx, None, 1)
    hip.set_shading(ctx, "gl", sc)
    assert L.pt_begin(ctx.handle, C.byref(flat.c), C.byref(pc)) == capi.PT_ERR_STATE and b"GL shading" in L.pt_last_error()
    hip.set_shading(ctx, "cpu")
    usable()
    # inside an open frame
    hip.set_adaptive(ctx, fa.CASE_TARGET, 0, STEP)
    hip.set_adaptive_filtered(ctx, None, 1)
    capi.check(L.pt_begin(ctx.handle, C.byref(flat.c), C.byref(pc)))
    f = good()
    assert L.pt_set_adaptive_filtered(ctx.handle, C.byref(f)) == capi.PT_ERR_STATE
    assert L.pt_set_adaptive_filtered(ctx.handle, None) == capi.PT_ERR_STATE
    assert L.pt_read_block_figures(ctx.handle, pooled.ctypes.data_as(dp), None, None) == capi.PT_ERR_STATE  # no step yet
    capi.check(L.pt_step(ctx.handle, 2, None))
    assert L.pt_read_block_figures(ctx.handle, pooled.ctypes.data_as(dp), None, None) == capi.PT_ERR_STATE  # 2 samples: nothing decided
    assert b"no check of the frame has decided yet" in L.pt_last_error()
    capi.check(L.pt_step(ctx.handle, 6, None))
    n = C.c_int32(0)
    capi.check(L.pt_read_block_figures(ctx.handle, pooled.ctypes.data_as(dp), None, C.byref(n)))
    assert n.value == 1 and np.all(pooled > 0)
    capi.check(L.pt_end(ctx.handle, None))
    # after a plain frame, and after an adaptive frame without the rule
    hip.set_adaptive_filtered(ctx, on=False)
    hip.set_adaptive(ctx, None)
    hip.set_moments(ctx, True)
    pc8 = hip.pt_config(hip.RenderConfig(W, H, 8, DEPTH, SEED))
    capi.check(L.pt_render(ctx.handle, C.byref(flat.c), C.byref(pc8), img.ctypes.data_as(C.c_void_p), W * 4, None, None, None, None))
    assert L.pt_read_block_figures(ctx.handle, pooled.ctypes.data_as(dp), None, None) == capi.PT_ERR_STATE
    assert b"adaptive sampling off" in L.pt_last_error()
    hip.set_adaptive(ctx, 0.25, 0, STEP)
    capi.check(L.pt_render(ctx.handle, C.byref(flat.c), C.byref(pc8), img.ctypes.data_as(C.c_void_p), W * 4, None, None, None, None))
    assert L.pt_read_block_figures(ctx.handle, pooled.ctypes.data_as(dp), None, None) == capi.PT_ERR_STATE
    assert b"the rule off" in L.pt_last_error()
    hip.set_adaptive(ctx, None)
    usable()


# ---------------------------------------------------------------- 5. the rule off
def test_a_context_that_set_and_cleared_the_rule_renders_the_adaptive_frame_it_did():
    from path_trace_golang_amd import capi, hip

    name, depth, seed, cap, step, min_spp, target = ad.CASE
    sc = _scene(name)
    with capi.Context(ndev=1) as ctx:
        ref = ad.render_adaptive(ctx, sc, W, H, cap, depth, seed, target, step, min_spp)
    with capi.Context(ndev=1) as ctx:
        run_rule(ctx, sc, W, H, fa.CASE_TARGET, stepped=False)
        hip.set_adaptive_filtered(ctx, on=False)
        ctx._filtered_adaptive_on = False
        got = ad.render_adaptive(ctx, sc, W, H, cap, depth, seed, target, step, min_spp)
        halves_off = capi.load().pt_read_halves(ctx.handle, None, None, None, None)
    assert np.array_equal(got[3][::8, ::8], np.asarray(ad.CASE_MAP, np.uint32))  # section 3.10's own rule and its committed map
    for a, b in zip(ref[:4], got[:4]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert got[6]["adaptive"] == ref[6]["adaptive"] and got[6]["samples"] == ref[6]["samples"] == ad.CASE_SAMPLES
    assert halves_off == capi.PT_ERR_STATE  # the frame collected no half sums: nothing of the rule is left
