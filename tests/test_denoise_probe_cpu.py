"""The probe of the filter, pair-filter and temporal kernels (tests/denoise_probe.hip) without a GPU: it
cross-compiles for gfx950 with the library's flags against the unchanged pt_kernels.h and exports what test_denoise_probe_gpu.py
calls.  Every case that test runs on the device runs here through the host build of the product's headers and through the C
restatement, which must agree; and the conditions that keep the GPU tests from being vacuous -- that the inputs hold every special
pixel where the blocks and waves meet, that the temporal sequences reach every reason a history tap is rejected for, every frame
edge, the clamp of len' and both sides of alpha > 1 / (L + 1) -- are asserted on the restatement's results alone."""
from __future__ import annotations

import os
import re
import subprocess

import numpy as np
import pytest

import adaptive_probe_support as ap
import atrous_support as at
import denoise_probe_support as dp
import halves_support as hv
import temporal_support as ts
from fog_support import CSRC

SHAPE_IDS = ["%dx%d" % s for s in dp.SHAPES]


def test_probe_compiles_for_gfx950_with_the_library_flags():
    from path_trace_golang_amd import build

    assert "-ffp-contract=off" in build.HIP_FLAGS and "--offload-arch=gfx950" in build.HIP_FLAGS
    lib = dp.compile_probe()
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (\w+)", syms))
    assert set(dp.SYMBOLS) <= exported, sorted(set(dp.SYMBOLS) - exported)
    with open(lib, "rb") as f:
        blob = f.read()
    assert b"gfx950" in blob
    for kernel in dp.KERNELS:
        assert kernel.encode() in blob, kernel


def test_probe_source_launches_the_product_kernels_and_has_no_inline_assembly():
    def code_of(path):
        with open(path) as f:
            return re.sub(r"//.*", "", f.read())

    with open(dp.SOURCE) as f:
        src = f.read()
    code = code_of(dp.SOURCE)
    assert "asm" not in code and "__global__" not in code
    assert '#include "pt_kernels.h"' in src and '#include "probe_common.h"' in src
    # The probe runs the product's launch sequence itself: the header ptcore.hip includes holds the filter's launches, its iteration
    # loop and the two grids of a frame, and neither the probe nor ptcore.hip has a copy of any of them.
    assert '#include "pt_filter_launch.h"' in src
    header = code_of(os.path.join(CSRC, "pt_filter_launch.h"))
    core = code_of(os.path.join(CSRC, "ptcore.hip"))
    assert '#include "pt_filter_launch.h"' in core and "asm" not in header and "__global__" not in header
    grids = ("(npix + PT_BLOCK - 1) / PT_BLOCK", "((W + 31) / 32), (unsigned)((H + 7) / 8)")
    for text in grids + ("A.step = 1 << t",):
        assert header.count(text) == 1, text
    for where, text in (("probe", code), ("ptcore.hip", core)):
        for kernel in ("atrous_kernel", "atrous_pair_kernel", "atrous_noise_kernel", "atrous_finish_kernel"):
            assert not re.search(r"\b%s\b" % kernel, text), (where, kernel)        # not launched, not even named
        for expr in grids + ("(np + PT_BLOCK - 1) / PT_BLOCK", "+ 7) / 8", "1 << t"):
            assert expr not in text, (where, expr)
    for name in dp.KERNELS:
        assert "ptk::" + name in code or "ptk::" + name in header, name
    for name in ("ptk::AtrousPrepArgs", "ptk::AtrousArgs", "ptk::AtrousPairPrepArgs", "ptk::AtrousPairArgs", "ptk::HalvesCombineArgs",
                 "ptk::TemporalArgs", "ptk::NoisePartial", "ptk::HalvesPartial", "ptk::TemporalPartial"):
        assert name in code or name in header, name
    for name in ("ptl::filter_sequence", "ptl::pair_iterations", "ptl::filter_params", "ptl::noise_figures", "ptl::halves_figures",
                 "ptl::temporal_figures", "ptl::grid_1d", "ptl::grid_2d"):
        assert name in code and name in core, name
    assert "1.0 / (double)(W - 1)" in code


def test_the_shared_header_leaves_the_adaptive_probe_compiling():
    with open(ap.SOURCE) as f:
        src = f.read()
    assert '#include "probe_common.h"' in src and "struct Buf" not in src and "#define PROBE_TRY" not in src
    lib = ap.compile_probe()
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    assert set(ap.SYMBOLS) <= set(re.findall(r"\bT (\w+)", syms))


# ---------------------------------------------------------------- the filter and the pair filter
@pytest.mark.parametrize("size", dp.SHAPES, ids=SHAPE_IDS)
def test_specials_lie_where_blocks_waves_and_taps_meet(size):
    w, h = size
    S, Q, n, feats, places = dp.special_inputs(w, h, 7 * w + h)
    where = [p for _, p in places]
    kinds = [k for k, _ in places]
    assert sorted(kinds) == sorted(dp.BAD_KINDS + dp.GOOD_KINDS) and len(set(where)) == len(where) == 11
    bad = {p for k, p in places if k in dp.BAD_KINDS}
    assert (0, 0) in bad and (h - 1, w - 1) in bad                               # a frame corner, the last pixel
    if w >= 32 and h >= 8:
        assert any(x in (31, 32) and y in (7, 8) for y, x in where)               # a corner of the 32 x 8 blocks
        assert any(x in (31, 32) and y in (7, 8) for y, x in bad)
    if w * h > 255:
        assert any(y * w + x in (255, 256) for y, x in bad)                       # an end of a 256-thread block
    # one interior bad pixel whose 5 x 5 neighbours at step 1 include another special
    yi, xi = h // 2, w // 2
    assert (yi, xi) in bad and any((y, x) != (yi, xi) and abs(y - yi) <= 2 and abs(x - xi) <= 2 for y, x in where)
    if w * h > 256:                                                               # bad pixels in other waves than the first of a block
        assert any((y * w + x) % 256 >= 64 for y, x in bad)
    # the values: what the kinds say, and nothing else is non-finite
    nonfinite = ~(np.isfinite(S).all(axis=2) & np.isfinite(Q).all(axis=2))
    assert {tuple(p) for p in np.argwhere(nonfinite).tolist()} == bad and dp.planted_bad(w, h) == 5
    with np.errstate(all="ignore"):
        c = S / n[..., None]
        m = Q / n[..., None] - c * c
    d = dict((k, p) for k, p in places)
    assert np.all(S[d["var0_black"]] == 0) and np.all(m[d["var0_black"]] == 0) and np.all(m[d["var0"]] == 0) and np.all(c[d["var0"]] == 3.0)
    assert sum(1 for k, p in places if k == "Q0" and np.all(m[p] < 0)) == 2
    assert sum(1 for k, p in places if k == "h0" and feats[2][p][1] == 0) == 2
    assert np.isnan(S[d["nan_S"]]).any() and np.isposinf(S[d["posinf_S"]]).any() and np.isneginf(S[d["neginf_S"]]).any()
    assert np.isposinf(Q[d["inf_Q"]]).any() and np.isfinite(S[d["inf_Q"]]).all() and np.isnan(Q[d["nan_Q"]]).any()
    assert int(n.min()) >= 2 and int(n.max()) <= 64 and len(np.unique(n)) > 8
    # the pair variant: bad in half A only, in half B only and in both
    SA, QA, SB, QB, n2, _, info = dp.special_pair_inputs(w, h, 7 * w + h)
    badA = ~(np.isfinite(SA).all(axis=2) & np.isfinite(QA).all(axis=2))
    badB = ~(np.isfinite(SB).all(axis=2) & np.isfinite(QB).all(axis=2))
    assert len(info["both"]) == 2 and len(info["a_only"]) == 1 and len(info["b_only"]) == 2 and int(n2.min()) >= 4
    assert all(badA[p] and badB[p] for p in info["both"]) and all(badA[p] and not badB[p] for p in info["a_only"])
    assert all(badB[p] and not badA[p] for p in info["b_only"]) and int((badA | badB).sum()) == 5


def test_the_shapes_and_cases_are_the_ones_named():
    assert dp.SHAPES == ((37, 21), (97, 71), (130, 2), (2, 130), (33, 9), (64, 16)) and dp.ALL_ITERATIONS == ((37, 21), (97, 71))
    assert (97 + 31) // 32 == 4 and (71 + 7) // 8 == 9 and (97 * 71 + 255) // 256 == 27 and 97 * 71 % 256 != 0
    assert 64 * 16 % 256 == 0 and 64 % 32 == 0 and 16 % 8 == 0
    for w, h in dp.SHAPES:
        cases = dp.filter_cases(w, h)
        assert {c[0] for c in cases} == ({0, 1, 5, 6} if (w, h) in dp.ALL_ITERATIONS else {6})
        assert {c[1] for c in cases} == {0, 4, 5} and {c[2] for c in cases} == {True, False} and {c[3] for c in cases} == {True, False}
        assert len(cases) == (36 if (w, h) in dp.ALL_ITERATIONS else 10)
    assert dp.CONFIGS[4] == dict(sigma_n=0.0, sigma_z=0.0, sigma_a=0.0) and dp.CONFIGS[5]["sigma_n"] == 2.0 and dp.CONFIGS[0] == {}


@pytest.mark.parametrize("size", dp.SHAPES, ids=SHAPE_IDS)
def test_host_build_equals_the_restatement_on_every_filter_case(size):
    w, h = size
    _, _, _, _, places = dp.shape_inputs(w, h)
    bad = [p for k, p in places if k in dp.BAD_KINDS]
    for case in dp.filter_cases(w, h):
        ref = dp.run_filter_case("ref", w, h, case)
        at.assert_same_run(dp.run_filter_case("host", w, h, case), ref, (size, case))
        assert ref["bad_pixels"] == dp.planted_bad(w, h) == len(bad)
        t0 = dp.run_filter_case("ref", w, h, (0,) + case[1:]) if (0,) + case[1:] in dp.filter_cases(w, h) else None
        for p in bad:  # a bad pixel passes through: not finite, and its bytes are the finish of its own mean
            assert not (np.isfinite(ref["mean"][p]).all() and np.isfinite(ref["var"][p]))
            if t0 is not None:
                assert np.array_equal(ref["rgba"][p], t0["rgba"][p]) and at.same_bits(ref["mean"][p], t0["mean"][p])
            with np.errstate(all="ignore"):
                v = np.sqrt(ref["mean"][p]) * 255.999
            want = [0 if np.isnan(x) else int(min(max(x, 0.0), 255.999)) for x in v.tolist()] + [255]
            assert ref["rgba"][p].tolist() == want, (size, case, p)
        good = np.ones((h, w), bool)
        for p in bad:
            good[p] = False
        assert np.isfinite(ref["mean"][good]).all() and np.isfinite(ref["var"][good]).all()


@pytest.mark.parametrize("size", dp.SHAPES, ids=SHAPE_IDS)
def test_host_build_equals_the_restatement_on_every_pair_case(size):
    w, h = size
    info = dp.shape_inputs(w, h, pair=True)[-1]
    for case in dp.filter_cases(w, h):
        ref = dp.run_filter_case("ref", w, h, case, pair=True)
        hv.assert_same_pair(dp.run_filter_case("host", w, h, case, pair=True), ref, (size, case))
        assert ref["bad_pixels"] == 5
        fA, fB = ref["half_means"]
        for p in info["a_only"]:  # the good half of a pixel that is bad in one half stays finite (the bad half may have a finite mean and
            assert np.isfinite(fB[p]).all()  # an infinite variance)
        for p in info["b_only"]:
            assert np.isfinite(fA[p]).all()
        assert not np.isfinite(fA[info["a_only"][0]]).all() and not np.isfinite(fB[info["b_only"][1]]).all()


def test_step_32_taps_count_across_block_rows_and_columns_at_97_x_71():
    """At 97 x 71 the sixth iteration (step 32) of the wide-sigma configuration has taps that lie in another block row and another
    block column, on good pixels, with a weight that matters; so has the configuration without features."""
    w, h = 97, 71
    counts = {case: dp.step32_taps(w, h, case) for case in dp.filter_cases(w, h) if case[0] == 6 and case[3]}
    print(counts)
    assert all(c[1] in (0, 4, 5) for c in counts)
    assert all(v > 100 for c, v in counts.items() if c[1] == 5), counts
    # and the taps change the result: the sixth iteration is not the fifth
    for case in counts:
        five = dp.run_filter_case("ref", w, h, (5,) + case[1:])
        six = dp.run_filter_case("ref", w, h, case)
        assert int(np.count_nonzero(five["mean"] != six["mean"])) > w * h


# ---------------------------------------------------------------- the temporal sequences
def test_the_sequences_and_configurations_are_the_ones_named():
    assert set(dp.SEQUENCES) == {"unmoved", "sideways", "sideways, up = x", "sideways 33 x 9", "sideways 97 x 71", "rotation", "dolly",
                                 "field of view", "turn", "through the wall", "jump", "edge", "resize"}
    assert dp.TCONFIGS == ({}, dict(alpha=0.5, max_len=3), dict(alpha=0.0, tol_z=1e9, n_min=-2.0, tol_a=1e9), dict(alpha=1.0),
                           dict(tol_z=0.0, tol_a=0.0, n_min=1.0))
    assert dp.FILTERS == (dict(iterations=3), None, dict(iterations=0), dict(iterations=6))
    sizes = {name: [(f["w"], f["h"]) for f in dp.sequence(name)] for name in dp.SEQUENCES}
    assert sizes["sideways 33 x 9"] == [(33, 9)] * 8 and sizes["sideways 97 x 71"] == [(97, 71)] * 8 and sizes["unmoved"] == [(70, 37)] * 8
    assert sizes["resize"] == [(70, 37)] * 2 + [(33, 9)] * 2 + [(70, 37)] * 4 and [f["reset"] for f in dp.sequence("resize")].count(True) == 1
    assert len(sizes["turn"]) == 4 and len(sizes["through the wall"]) == 5 and len(sizes["rotation"]) == 8
    for name in dp.SEQUENCES:
        for f in dp.sequence(name):
            nonfinite = ~(np.isfinite(f["S"]).all(axis=2) & np.isfinite(f["Q"]).all(axis=2))
            assert {tuple(p) for p in np.argwhere(nonfinite).tolist()} == set(f["bad"]) and len(set(f["bad"])) == 3
            assert f["cam"].shape == (22,) and f["feats"][2][..., 2].min() == 4.0
    # the second wall is nearer and covers part of the view; a third of the first wall's normals are tilted past n_min
    fr = dp.sequence("sideways")[0]
    fn, _, fd = fr["feats"]
    hit = fd[..., 1] > 0
    z = np.where(hit, fd[..., 0] / np.where(hit, fd[..., 1], 1.0), 0.0)
    assert 0.1 < np.mean(z[hit] < 4.0) < 0.6 and 0.05 < np.mean(~hit) < 0.75
    nz = np.abs(fn[..., 2][hit] / fd[..., 1][hit])
    assert 0.2 < np.mean(nz < 0.9) < 0.45 and np.all((np.abs(nz - 0.8) < 1e-12) | (np.abs(nz - 1.0) < 1e-12))


_classes = {}


@pytest.mark.parametrize("name", dp.SEQUENCES)
def test_host_build_equals_the_restatement_on_every_sequence(name):
    frames = dp.sequence(name)
    for ci, tcfg in enumerate(dp.TCONFIGS):
        for fi, flt in enumerate(dp.FILTERS):
            ref, ref_hist = dp.run_frames("ref", frames, flt, **tcfg)
            host, host_hist = dp.run_frames("host", frames, flt, **tcfg)
            for k, (a, b) in enumerate(zip(host, ref)):
                ts.assert_same_frame(a, b, (name, tcfg, flt, k))
            assert at.same_bits(host_hist[0], ref_hist[0]) and at.same_bits(host_hist[1], ref_hist[1]) and np.array_equal(host_hist[2], ref_hist[2])
            for k, r in enumerate(ref):
                npix = frames[k]["w"] * frames[k]["h"]
                assert r["bad_pixels"] == 3
                if dp.has_history(frames, k):
                    assert r["reprojected"] + r["disoccluded"] + r["bad_pixels"] == npix, (name, tcfg, k)
                else:
                    assert r["reprojected"] == 0 and r["disoccluded"] == 0 and r["mean_len"] * npix == npix - 3
            if fi == 0 and ci in (0, 1):  # the tap classes, for test_the_sequences_reach_every_tap_class
                rows = []
                for k in range(1, len(frames)):
                    if dp.has_history(frames, k):
                        c = dp.classify(frames[k - 1], frames[k], ref[k - 1], ref[k], **tcfg)
                        assert c["reprojected"] == ref[k]["reprojected"], (name, tcfg, k)  # the classification is the restatement's
                        c["good"] = frames[k]["w"] * frames[k]["h"] - 3
                        rows.append(c)
                _classes[(name, ci)] = rows


def test_the_sequences_reach_every_tap_class():
    for name in dp.SEQUENCES:  # (a run of this test alone computes what the test above leaves)
        for ci in (0, 1):
            if (name, ci) not in _classes:
                frames = dp.sequence(name)
                ref, _ = dp.run_frames("ref", frames, dp.FILTERS[0], **dp.TCONFIGS[ci])
                _classes[(name, ci)] = [dict(dp.classify(frames[k - 1], frames[k], ref[k - 1], ref[k], **dp.TCONFIGS[ci]),
                                             good=frames[k]["w"] * frames[k]["h"] - 3) for k in range(1, len(frames)) if dp.has_history(frames, k)]
    default = [c for (name, ci), rows in _classes.items() if ci == 0 for c in rows]
    short = [c for (name, ci), rows in _classes.items() if ci == 1 for c in rows]
    total = {k: sum(c[k] for c in default) for k in default[0]}
    print(total)
    for reason in dp.REASONS:  # a tap rejected for each single reason
        assert total[reason] > 0, reason
    for k in ("sole tol_z", "sole n_min", "sole tol_a"):  # ... and for each tolerance, taps that fail nothing else
        assert total[k] > 0, k
    assert total["small sw"] > 0  # 0 < sw <= 0.01: the "edge" sequence puts 0.005 of a pixel inside the frame
    for k in ("x0 = -1", "y0 = -1", "x0 = W - 1", "y0 = H - 1"):
        assert total[k] > 0, k
    assert sum(c["clamped"] for c in short) > 0 and total["clamped"] == 0                # max_len = 3 clamps, 32 does not
    assert any(c["alpha above"] > 0 and c["alpha not above"] > 0 for c in default)         # alpha > 1 / (L + 1) true and false in one frame
    assert any(c["alpha above"] > 0 and c["alpha not above"] > 0 for c in short)
    assert any(c["reprojected"] == 0 for c in default)                                   # every good pixel disoccluded, the history valid
    assert any(c["reprojected"] == c["good"] for c in default)                           # every good pixel reprojected
    assert all(c["reprojected"] == 0 for c in _classes[("turn", 0)]) and len(_classes[("turn", 0)]) == 3
    assert any(c["reprojected"] == 0 for c in _classes[("through the wall", 0)])
    assert all(c["reprojected"] == c["good"] for c in _classes[("unmoved", 0)][:3])
    assert any(c["len"] > 0 for c in _classes[("unmoved", 0)][3:])                       # a tap on a pixel that was bad
    lens = max(f["hist_len"].max() for f in dp.run_frames("ref", dp.sequence("sideways"), None)[0])
    assert lens == 8
