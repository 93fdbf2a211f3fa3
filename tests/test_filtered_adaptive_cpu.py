"""Adaptive sampling by the filtered frame's pooled noise (pt_set_adaptive_filtered; the model in csrc/pt_atrous.h,
BLOCKS), without a GPU: the host build of the new PT_HD functions against the plain-Python restatement of steps 2 to 4 on planted
planes, bit for bit; the whole rule predicted from the oracle's per-sample radiances on the committed case; and the surface -- the
entry points, their refusals without a device, hip.render's refusals and the environment parsing."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

import adaptive_support as ad
import atrous_support as at
import filtered_adaptive_support as fa
import halves_support as hs
from moments_support import H, W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pt_set_adaptive_filtered", "pt_read_block_figures")


# ---------------------------------------------------------------- steps 2 to 4: the restatement against the host build
def test_the_planted_planes_hold_what_no_rendered_frame_gives():
    for w, h in fa.GRIDS:
        mean, err, bad = fa.planted(w, h)
        l = mean.sum(axis=2) / 3.0
        assert np.isnan(err).any() and np.isposinf(err).any() and np.isneginf(err).any(), (w, h)
        assert (bad == 1).any() and (bad == 2).any() and (bad == 3).any()  # bad in half A only, in half B only, in both
        assert (l < 0.01).any() and (l < 0).any() and (l == 0).any() and np.isnan(l).any()
    mean, err, bad = fa.planted(37, 21)
    assert np.all(bad[16:, 32:] == 3)  # the last block: 5 x 5 pixels, every one bad


@pytest.mark.parametrize("pool", fa.POOLS)
@pytest.mark.parametrize("w,h", fa.GRIDS)
def test_the_restatement_and_the_host_build_agree_bit_for_bit(w, h, pool):
    mean, err, bad = fa.planted(w, h)
    nby, nbx = fa.grid(w, h)
    free = fa.restate_blocks(mean, err, bad, pool, 0.0)
    target = float(np.median(free["pooled"]))  # some blocks at or below it (the median itself: the <= of the rule), some above
    want = fa.restate_blocks(mean, err, bad, pool, target)
    got = fa.host_blocks(mean, err, bad, pool, target)
    fa.assert_same_blocks(got, want, (w, h, pool))
    assert want["stop"].any() and (nby * nbx == 1 or not want["stop"].all() or np.unique(want["pooled"]).size == 1)
    # k_B: the block's pixels inside the frame, bad ones included
    inside = np.zeros((nby * 8, nbx * 8), np.uint32)
    inside[:h, :w] = 1
    assert np.array_equal(want["k"], inside.reshape(nby, 8, nbx, 8).sum(axis=(1, 3)))
    assert np.all(np.isfinite(want["s"])) and np.all(want["s"] >= 0) and np.all(np.isfinite(want["pooled"]))
    if nby * nbx > 1:  # the block whose every pixel is bad
        assert want["s"][-1, -1] == 0.0 and want["k"][-1, -1] > 0 and want["own"][-1, -1] == 0.0
    if pool == 0 or nby * nbx == 1:  # every window is the block itself
        assert at.same_bits(want["pooled"], want["own"])
    if pool >= max(nby, nbx) - 1:  # every window is the whole grid: one figure, whatever the block
        assert np.unique(want["pooled"].view(np.uint64)).size == 1


def test_a_window_is_summed_rows_first_from_zero():
    """The order of step 3 matters in the last bit: a window summed in another order gives other bits somewhere on the 97 x 71 grid."""
    mean, err, bad = fa.planted(97, 71)
    r = fa.restate_blocks(mean, err, bad, 2, 0.0)
    s, k = r["s"], r["k"].astype(np.float64)
    nby, nbx = s.shape
    other = np.zeros_like(s)
    for by in range(nby):
        for bx in range(nbx):
            ys, xs = range(max(0, by - 2), min(nby, by + 3)), range(max(0, bx - 2), min(nbx, bx + 3))
            ss = 0.0
            for x in xs:  # columns first
                for y in ys:
                    ss = ss + float(s[y, x])
            other[by, bx] = np.sqrt(ss / sum(float(k[y, x]) for y in ys for x in xs))
    assert np.allclose(other, r["pooled"], rtol=1e-14, atol=0) and not at.same_bits(other, r["pooled"])


def test_the_term_is_the_one_the_frame_figure_adds():
    """noise^2 * pixels of pt_atrous_halves' model = the sum of every block's s_B (to the rounding of the two orders), on a frame
    with bad pixels: the block rule and the frame rule count the same pixels."""
    smp = __import__("moments_support").samples("example_simple", 4, 1, 8)
    SA, QA, SB, QB = (np.array(a) for a in hs.half_sums(smp))
    SA[3, 5, 1] = np.nan  # bad in half A only
    QB[10, 20, 0] = np.inf
    r = hs.host_pair(SA, QA, SB, QB, 8, None, None)
    bad = np.zeros((H, W))
    bad[3, 5], bad[10, 20] = 1.0, 2.0
    b = fa.host_blocks(r["mean"], r["err"], bad, 0, 0.0)
    assert r["bad_pixels"] == 2
    assert abs(float(b["s"].sum()) - r["noise"] ** 2 * W * H) <= 1e-12 * float(b["s"].sum())


def test_the_header_states_the_model():
    text = open(os.path.join(ROOT, "path_trace_golang_amd", "csrc", "pt_atrous.h")).read()
    head = text[:text.index("#pragma once")]
    assert head.index("HALVES") < head.index("BLOCKS (pt_set_adaptive_filtered")
    assert "DO keep each other alive" in head and "rows top to bottom and left to right" in head
    # (that block_term is combine_pixel's own term is checked in numbers, in test_the_term_is_the_one_the_frame_figure_adds)


# ---------------------------------------------------------------- the whole rule on the case, from the oracle's samples
@pytest.fixture(scope="module")
def case(oracle):
    frames, feats = fa.case_frames()
    name, depth, seed, cap, step, min_spp, k, pool = fa.CASE
    return fa.predict(frames, feats, fa.CASE_TARGET, step, min_spp, cap, pool), frames, feats


def test_the_case_stops_some_blocks_and_neighbours_keep_one_alive(case):
    r, frames, feats = case
    cap = fa.CASE[3]
    assert r["counts"].tolist() == fa.CASE_MAP
    assert r["samples"] == fa.CASE_SAMPLES and int(r["active"].sum()) == fa.CASE_ACTIVE
    assert (r["counts"] < cap).any() and r["active"].any()  # the rule stops some blocks and not others
    assert r["by_neighbours"].any()                         # own <= target < pooled at some check: kept alive by the pool alone
    assert r["margin"] > 1e-3                               # no decision rides on the last bits
    assert r["worst"] > fa.CASE_TARGET
    assert sorted(r["figures"]) == [8, 16, 24, 32]


def test_the_case_judged_block_by_block_is_another_frame(case):
    """pool = 0 on the same samples: the blocks the pool kept alive stop earlier -- the pool is what the rule adds."""
    r, frames, feats = case
    name, depth, seed, cap, step, min_spp, k, pool = fa.CASE
    own = fa.predict(frames, feats, fa.CASE_TARGET, step, min_spp, cap, 0)
    assert not own["by_neighbours"].any()
    assert np.all(own["counts"][r["by_neighbours"]] <= r["counts"][r["by_neighbours"]]) and own["counts"].tolist() != fa.CASE_MAP


def test_the_host_build_of_the_pair_filter_predicts_the_same_frame(case):
    """The predictor with halves_support.host_pair (the product's functions on the host) in place of the restatement: the same
    counts and the same figures bit for bit -- what the GPU test relies on when it feeds the predictor with device frames."""
    r, frames, feats = case
    name, depth, seed, cap, step, min_spp, k, pool = fa.CASE
    h = fa.predict(frames, feats, fa.CASE_TARGET, step, min_spp, cap, pool, pair=hs.host_pair)
    assert h["counts"].tolist() == fa.CASE_MAP
    for n in r["figures"]:
        assert at.same_bits(h["figures"][n][0], r["figures"][n][0]) and at.same_bits(h["figures"][n][1], r["figures"][n][1]), n


def test_a_min_spp_above_the_first_check_delays_the_first_decision(case):
    r, frames, feats = case
    name, depth, seed, cap, step, _, k, pool = fa.CASE
    late = fa.predict(frames, feats, fa.CASE_TARGET, step, 20, cap, pool)
    assert sorted(late["figures"]) == [24, 32] and late["counts"].min() >= 24


# ---------------------------------------------------------------- does the rule pay?  ("Measured on the CPU")
def test_the_truth_fixtures_are_the_oracles_own_frames(oracle):
    """A window of every committed 8 192-spp frame, rendered again: the same bits."""
    from oracle import ora

    S = fa.STUDY
    for name in fa.STUDY_SCENES:
        truth = fa.study_truth(name)
        assert truth.shape == (S["h"], S["w"], 3) and truth.dtype == np.float64
        x0, y0, x1, y1 = 36, 20, 44, 24
        r = ora.render(at.ora_scene_of(name), S["w"], S["h"], S["truth_spp"], S["depth"], seed=S["truth_seed"], window=(x0, y0, x1, y1), want=("accum",))
        assert at.same_bits(r["accum"][y0:y1, x0:x1] / float(S["truth_spp"]), truth[y0:y1, x0:x1]), name


@pytest.mark.parametrize("name", fa.STUDY_SCENES)
def test_the_study_gives_the_committed_figures(oracle, name):
    """The table of DESIGN 3.12a recomputed from the oracle's samples: three ways of spending the same samples, pool 0, 1 and 2."""
    S = fa.STUDY
    cap_frame, rows = fa.STUDY_TABLE[name]
    close = lambda a, b: abs(a - b) <= 1e-6 * abs(b)
    full = fa.study_uniform(name, S["w"] * S["h"] * S["cap"])
    assert full["spp"] == S["cap"] and close(full["rel_mse"], cap_frame)
    for pool in fa.STUDY_POOLS:
        target, samples, rule, own_target, own_samples, own, uniform_spp, uniform = rows[pool]
        r = fa.study_rule(name, target, pool)
        print(name, pool, r["samples"], r["share"], r["rel_mse"])
        assert r["samples"] == samples and 0.4 <= r["share"] <= 0.6, (pool, r["samples"], r["share"])
        assert close(r["rel_mse"], rule), (pool, r["rel_mse"], rule)
        o = fa.study_own(name, own_target)
        assert o["samples"] == own_samples and abs(own_samples - samples) <= 0.03 * samples, (pool, o["samples"])
        assert close(o["rel_mse"], own), (pool, o["rel_mse"], own)
        u = fa.study_uniform(name, samples)
        assert u["spp"] == uniform_spp and close(u["rel_mse"], uniform), (pool, u)


def test_the_shipped_pool_is_what_the_table_says():
    """Best on the most scenes: pool 0 and pool 1 tie at two scenes each, pool 2 has one; on a tie the default stays 1.  And the table's
    plain words: at equal samples the rule (pool 1) beats the uniform frame on three scenes and loses on two."""
    from path_trace_golang_amd import hip
    import inspect

    wins = {p: 0 for p in fa.STUDY_POOLS}
    beats_uniform, beats_own = [], []
    for name, (_, rows) in fa.STUDY_TABLE.items():
        wins[min(fa.STUDY_POOLS, key=lambda p: rows[p][2])] += 1
        if rows[1][2] < rows[1][7]:
            beats_uniform.append(name)
        if rows[1][2] < rows[1][5]:
            beats_own.append(name)
    assert wins == {0: 2, 1: 2, 2: 1}
    assert inspect.signature(hip.render).parameters["pool"].default == 1 and inspect.signature(hip.set_adaptive_filtered).parameters["pool"].default == 1
    assert beats_uniform == ["example_simple", "metal_glass_room", "test_scene"]
    assert beats_own == ["gpu_showcase", "metal_glass_room", "test_comprehensive", "test_scene"]


# ---------------------------------------------------------------- the surface
def test_entry_points_are_declared_exported_and_bound():
    from path_trace_golang_amd import build, capi

    build.build_core()
    lib = capi.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptcore.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pt_[a-z_0-9]+)\s*\(", text))
    bound = {name for name, _, _ in capi.SYMBOLS}
    for sym in ENTRY_POINTS:
        assert sym in declared, sym
        assert hasattr(lib, sym), sym
        assert sym in bound and capi.has(sym) and sym in capi.ADDITIVE, sym
    assert re.search(r"\}\s*pt_adaptive_filtered\s*;", text)
    assert lib.pt_abi_version() == 4  # additive: the version stays
    assert C.sizeof(capi.PtAdaptiveFiltered) == C.sizeof(capi.PtAtrousConfig) + 8


def test_null_arguments_are_refused_with_a_message():
    from path_trace_golang_amd import capi

    lib = capi.load()
    f = capi.PtAdaptiveFiltered()
    for call in (lambda: lib.pt_set_adaptive_filtered(None, C.byref(f)), lambda: lib.pt_set_adaptive_filtered(None, None),
                 lambda: lib.pt_read_block_figures(None, None, None, None)):
        assert call() == capi.PT_ERR_INVALID
        assert lib.pt_last_error()


def test_the_go_binding_is_kept_in_step():
    go = open(os.path.join(ROOT, "go", "internal", "engine", "hip", "hip.go")).read()
    for sym in ENTRY_POINTS:
        assert "C." + sym + "(" in go, sym
    assert "func SetFilteredAdaptive(" in go and "func ReadBlockFigures(" in go and "C.pt_adaptive_filtered" in go


def test_render_refuses_what_the_rule_excludes_before_it_touches_the_library():
    from path_trace_golang_amd import hip

    img = np.zeros((8, 8, 4), np.uint8)
    cfg = hip.RenderConfig(8, 8, 8, 2, 1)
    f = hip.AtrousConfig()
    for kw, text in ((dict(filtered_adaptive=0.1), "needs the filter"),
                     (dict(filtered_adaptive=0.1, atrous=f, noise=0.1), "one stop rule per frame"),
                     (dict(filtered_adaptive=0.1, atrous=f, noise=0.1, adaptive=True), "one stop rule per frame"),
                     (dict(filtered_adaptive=0.1, atrous=f, filtered_noise=0.1), "one stop rule per frame"),
                     (dict(filtered_adaptive=0.1, atrous=f, shading="gl"), "GL shading"),
                     (dict(filtered_adaptive=0.1, atrous=f, pool=5), "pool must be 0..4"),
                     (dict(filtered_adaptive=0.1, atrous=f, pool=-1), "pool must be 0..4")):
        with pytest.raises(ValueError, match=text):
            hip.render(None, cfg, img, **kw)
    # the refusals that were there keep their words
    with pytest.raises(ValueError, match=r"^filtered_noise excludes noise= and adaptive=True: one stop rule per frame$"):
        hip.render(None, cfg, img, atrous=f, filtered_noise=0.1, noise=0.1)
    with pytest.raises(ValueError, match=r"^filtered_noise needs the filter whose output it measures \(atrous=\)$"):
        hip.render(None, cfg, img, filtered_noise=0.1)


def test_the_environment_is_parsed_like_the_other_targets():
    from path_trace_golang_amd import hip

    E = "PATHTRACER_GPU_"
    assert hip.filtered_adaptive_from_env({}) == (None, 1)
    assert hip.filtered_adaptive_from_env({E + "FILTERED_ADAPTIVE": "0.05"}) == (0.05, 1)
    assert hip.filtered_adaptive_from_env({E + "FILTERED_ADAPTIVE": "0.05", E + "POOL": "0"}) == (0.05, 0)
    assert hip.filtered_adaptive_from_env({E + "FILTERED_ADAPTIVE": "0.05", E + "POOL": "4"}) == (0.05, 4)
    for bad in ("5", "-1", "x", ""):
        assert hip.filtered_adaptive_from_env({E + "FILTERED_ADAPTIVE": "0.05", E + "POOL": bad}) == (0.05, 1)
    for bad in ("0", "-1", "nan", "x", ""):
        assert hip.filtered_adaptive_from_env({E + "FILTERED_ADAPTIVE": bad})[0] is None
