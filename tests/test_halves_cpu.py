"""Half-buffer sums and the measured noise of the filtered frame on CPU: the host build of the pair functions of
csrc/pt_atrous.h against the existing restatement of the filter run on each half, bit for bit; the calibration of the measured figure
against the across-seed truth on the five shipped scenes and the stop rule's count, both from oracle samples only; and the surface
(symbols, struct layout, argument refusals, off by default, environment, flags).  No compute calls on a device here."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

import atrous_support as at
import halves_support as hv
import moments_support as ms
from conftest import ROOT, SCENE_NAMES

ENTRY_POINTS = ("pt_set_halves", "pt_read_halves", "pt_atrous_halves")


def random_halves(w, h, seed):
    """The four sums of a frame with counts 4..64 and, per half, every special case denoise_probe_support.random_inputs names: pixels
    with var = 0, with Q/n < c^2, with NaN and infinite sums -- in both halves, in half A only and in half B only -- and the
    feature planes of that function (pixels whose feature samples all missed, smooth regions and edges in every guide)."""
    from denoise_probe_support import random_inputs

    r = np.random.default_rng(seed)
    _, _, _, feats = random_inputs(w, h, seed)
    n = r.integers(4, 65, (h, w)).astype(np.uint32)
    base = np.where(np.arange(w)[None, :, None] < w // 2, 0.2, 1.5) + 0.3 * r.random((h, w, 3))
    out = []
    for nh in ((n + 1) // 2, n // 2):
        nh = nh.astype(np.float64)[..., None]
        mean = base * (1 + 0.4 * r.standard_normal((h, w, 3)))
        S = mean * nh
        Q = (mean * mean + (0.5 * base * r.random((h, w, 3))) ** 2 * nh) * nh
        out += [S, Q]
    SA, QA, SB, QB = out
    nA, nB = (n + 1) // 2, n // 2
    for S, Q, nh in ((SA, QA, nA), (SB, QB, nB)):
        S[1, 2] = 0.0; Q[1, 2] = 0.0                        # var = 0 exactly, l = 0
        S[3, 5] = 3.0 * nh[3, 5]; Q[3, 5] = 9.0 * nh[3, 5]  # var = 0 exactly
        Q[4, 7] = 0.0; Q[h - 1, w - 1] = 0.0                # Q/n < c^2: counts as 0
    SA[6, 9, 1] = np.nan; SB[6, 9, 0] = np.inf              # bad in both halves
    QA[0, 0, 0] = np.nan; QB[0, 0, 2] = np.nan
    SA[7, 11, 0] = np.inf                                   # bad in half A only
    QA[8, 13, 2] = np.inf                                   # (var infinite, mean finite)
    SB[h - 2, w - 3, 2] = -np.inf                           # bad in half B only
    QB[10, 17, 1] = np.nan
    QB[4, 8] = 0.0                                          # Q/n < c^2 in half B only
    return SA, QA, SB, QB, n, feats


BAD = 6  # the pixels above that are bad in either half
CONFIGS = [dict(), dict(sigma_n=0.0, sigma_z=0.0, sigma_a=0.0), dict(sigma_l=0.5, sigma_n=2.0, sigma_z=1.0, sigma_a=5.0), dict(sigma_z=0.0)]


@pytest.mark.parametrize("size", [(40, 24), (37, 21)])
def test_host_build_equals_the_restatement_on_each_half(size):
    w, h = size
    SA, QA, SB, QB, n, feats = random_halves(w, h, 7 * w + h)
    runs = 0
    for T in (0, 1, 5, 6):  # steps 16 and 32 reach past a 24-row frame
        for i, cfg in enumerate(CONFIGS):
            if T in (1, 6) and i > 1:
                continue
            for counts in (n, None):
                for f in (feats, None):
                    if f is None and i > 1:
                        continue
                    a = hv.host_pair(SA, QA, SB, QB, 9, counts, f, iterations=T, **cfg)  # uniform: nA = 5, nB = 4
                    b = hv.ref_pair(SA, QA, SB, QB, 9, counts, f, iterations=T, **cfg)
                    hv.assert_same_pair(a, b, (size, T, cfg, counts is None, f is None))
                    assert a["bad_pixels"] == BAD
                    runs += 1
    assert runs >= 40


def test_a_pixel_bad_in_one_half_keeps_the_other_half_filtered():
    w, h = 40, 24
    SA, QA, SB, QB, n, feats = random_halves(w, h, 3)
    run = hv.host_pair(SA, QA, SB, QB, 0, n, feats)
    t0 = hv.host_pair(SA, QA, SB, QB, 0, n, feats, iterations=0)
    fA, fB = run["half_means"]
    assert not np.isfinite(fA[7, 11]).all() and np.isfinite(fB[7, 11]).all()
    assert np.isfinite(fA[h - 2, w - 3]).all() and not np.isfinite(fB[h - 2, w - 3]).all()
    assert not at.same_bits(fB[7, 11], t0["half_means"][1][7, 11])  # half B of that pixel was filtered, not passed through
    assert at.same_bits(fA[7, 11], t0["half_means"][0][7, 11])      # half A passed through
    # T = 0: the halves are the half means, and their mean is the mean of the two
    nA, nB = hv.half_counts(0, n)
    with np.errstate(all="ignore"):
        assert at.same_bits(t0["half_means"][0], SA / nA[..., None].astype(np.float64))
        assert at.same_bits(t0["half_means"][1], SB / nB[..., None].astype(np.float64))
    # identical halves: err is exactly zero and the mean is the half
    same = hv.host_pair(SA, QA, SA, QA, 10, None, feats)
    good = np.isfinite(same["mean"]).all(axis=2)
    assert np.all(same["err"][good] == 0.0) and same["noise"] == 0.0 and same["noise_model"] > 0.0
    assert at.same_bits(same["mean"][good], same["half_means"][0][good])


# ---------------------------------------------------------------- calibration, from oracle samples only
SEEDS = range(1, 17)


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_measured_figure_is_closer_to_the_truth_than_the_propagated_one(name, oracle):
    """40 x 24, 16 spp, depth 4, k = 4, default sigmas, seeds 1..16.  truth = the across-seed variance of the two-halves mean,
    truth_full that of the full-sums filter's output, both as frame figures with l from an 8 192-spp frame of seed 8."""
    spp, depth = 16, 4
    l = oracle.render(ms.ora_scene(name), ms.W, ms.H, 8192, depth, seed=8, want=("accum",))["accum"] / 8192.0
    pair, full, noise, after, errs = [], [], [], [], []
    for seed in SEEDS:
        smp = ms.samples(name, depth, seed, spp)
        feats = at.ref_features(name, ms.W, ms.H, spp, depth, seed, 4)
        S, Q = ms.sums(smp)
        rf = at.ref_filter(S, Q, spp, None, feats)
        rp = hv.host_pair(*hv.half_sums(smp), spp, None, feats)
        assert rp["bad_pixels"] == 0
        pair.append(rp["mean"]); full.append(rf["mean"]); noise.append(rp["noise"]); after.append(rf["noise_after"]); errs.append(rp["err"])
    truth = hv.figure(np.var(np.stack(pair), axis=0, ddof=1).mean(axis=2), l)
    truth_full = hv.figure(np.var(np.stack(full), axis=0, ddof=1).mean(axis=2), l)
    m_noise, m_after = float(np.mean(noise)), float(np.mean(after))
    by_ref = hv.figure(np.mean(np.stack(errs), axis=0), l)  # err over the reference's l instead of the frame's own: not what `noise` reports
    print("| %s | %.4f | %.4f | %.2f | %.4f | %.4f (%.3f ... %.3f) | %.2f | %.4f | %.2f |"
          % (name, truth_full, m_after, m_after / truth_full, truth, m_noise, min(noise), max(noise), m_noise / truth, by_ref, by_ref / truth))
    assert abs(math.log(m_noise / truth)) < abs(math.log(m_after / truth_full)), (name, m_noise, truth, m_after, truth_full)


# ---------------------------------------------------------------- the stop rule, from oracle samples only
def test_stop_rule_restated_on_the_oracle_samples(oracle):
    case = hv.stop_case()
    print("figures per step:", ["%.6f" % f for f in case["figures"]], "T = %.6f" % case["target"], "stops at", case["count"])
    assert all(abs(f - case["target"]) >= 1e-6 for f in case["figures"])
    assert 4 < case["count"] < hv.STOP_CAP  # neither the first check nor the cap
    assert case["figures"][case["count"] // hv.STOP_STEP - 1] <= case["target"]
    assert all(f > case["target"] for f in case["figures"][: case["count"] // hv.STOP_STEP - 1])


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
    assert re.search(r"\}\s*pt_halves_stats\s*;", text)
    assert lib.pt_abi_version() == 4  # additive: the version stays


def test_null_and_bad_arguments_are_refused_with_a_message():
    from path_trace_golang_amd import capi, hip

    lib = capi.load()
    st = capi.PtHalvesStats()
    for call in (lambda: lib.pt_set_halves(None, 1), lambda: lib.pt_read_halves(None, None, None, None, None),
                 lambda: lib.pt_atrous_halves(None, None, None, None, None, C.byref(st))):
        assert call() == capi.PT_ERR_INVALID
        assert lib.pt_last_error()
    with pytest.raises(ValueError):
        hip.atrous_halves(None, None, mean=np.zeros((4, 4, 3), np.float32))
    with pytest.raises(ValueError):
        hip.atrous_halves(None, None, mean=np.zeros((4, 4, 3)), err=np.zeros((4, 5)))
    with pytest.raises(ValueError):
        hip.read_halves(None, np.zeros((4, 4)))


def test_struct_layout_in_c99_and_in_ctypes(tmp_path):
    from path_trace_golang_amd import build, capi

    lib = build.build_core()
    S = capi.PtHalvesStats
    assert C.sizeof(S) == 48
    src = tmp_path / "consumer.c"
    src.write_text(r'''
#include <stddef.h>
#include <stdio.h>
#include "ptcore.h"
int main(void) {
    typedef void (*fn_t)(void);
    fn_t fns[] = {(fn_t)pt_set_halves, (fn_t)pt_read_halves, (fn_t)pt_atrous_halves};
    pt_halves_stats s;
    int rc = pt_atrous_halves(0, 0, 0, 0, 0, &s) + 10 * pt_set_halves(0, 1) + 100 * pt_read_halves(0, 0, 0, 0, 0);
    printf("%d %d %d %d %d %d %d %d %d\n", (int)sizeof s, (int)offsetof(pt_halves_stats, launches), (int)offsetof(pt_halves_stats, iterations),
           (int)offsetof(pt_halves_stats, noise), (int)offsetof(pt_halves_stats, noise_model), (int)offsetof(pt_halves_stats, bad_pixels),
           (int)offsetof(pt_halves_stats, spp_min), rc, (int)(sizeof fns / sizeof fns[0]));
    return 0;
}
''')
    exe = tmp_path / "consumer"
    libdir = os.path.dirname(lib)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe), "-L", libdir, "-lptcore", "-Wl,-rpath," + libdir], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [48, S.launches.offset, S.iterations.offset, S.noise.offset, S.noise_model.offset, S.bad_pixels.offset, S.spp_min.offset,
                   111 * capi.PT_ERR_INVALID, 3]
    assert (S.atrous_ms.offset, S.launches.offset, S.iterations.offset, S.noise.offset, S.noise_model.offset, S.bad_pixels.offset,
            S.spp_min.offset) == (0, 8, 12, 16, 24, 32, 40)


def test_off_is_the_default_and_the_stop_rules_exclude_each_other():
    from path_trace_golang_amd import engine, hip

    assert hip.filtered_noise_from_env({}) is None
    for fn in (hip.render, engine.render_into):
        assert inspect.signature(fn).parameters["filtered_noise"].default is None
    img = np.zeros((4, 4, 4), np.uint8)
    cfg = hip.RenderConfig(4, 4, 8, 2, 1)
    with pytest.raises(ValueError, match="atrous="):
        hip.render(None, cfg, img, ctx=object(), filtered_noise=0.1)
    with pytest.raises(ValueError, match="excludes noise= and adaptive=True"):
        hip.render(None, cfg, img, ctx=object(), atrous=hip.AtrousConfig(), filtered_noise=0.1, noise=0.2)
    with pytest.raises(ValueError, match="excludes noise= and adaptive=True"):
        hip.render(None, cfg, img, ctx=object(), atrous=hip.AtrousConfig(), filtered_noise=0.1, noise=0.2, adaptive=True)


def test_filtered_noise_from_env():
    from path_trace_golang_amd import hip

    assert hip.filtered_noise_from_env({"PATHTRACER_GPU_FILTERED_NOISE": "0.25"}) == 0.25
    for v in ("0", "-1", "x", "", "nan", "inf"):
        assert hip.filtered_noise_from_env({"PATHTRACER_GPU_FILTERED_NOISE": v}) is None


def test_render_help_lists_the_filtered_noise_flag():
    from path_trace_golang_amd import build

    build.build_host()
    exe = os.path.join(ROOT, "path_trace_golang_amd", "render")
    r = subprocess.run([exe, "-h"], capture_output=True, text=True)
    assert r.returncode == 0 and "  -filtered-noise float\n" in r.stderr
    bad = subprocess.run([exe, "-filtered-noise", "low"], capture_output=True, text=True)
    assert bad.returncode == 2 and 'invalid value "low" for flag -filtered-noise' in bad.stderr


def test_host_layer_and_go_source_have_the_switch():
    hpp = open(os.path.join(ROOT, "path_trace_golang_amd", "csrc", "host", "engine.hpp")).read()
    cpp = open(os.path.join(ROOT, "path_trace_golang_amd", "csrc", "host", "engine.cpp")).read()
    assert "void SetFilteredNoise(double target" in hpp
    for name in ("pt_set_halves", "pt_atrous_halves", "PATHTRACER_GPU_FILTERED_NOISE"):
        assert name in cpp, name
    go = open(os.path.join(ROOT, "go", "internal", "engine", "hip", "hip.go")).read()
    for name in ("C.pt_set_halves", "C.pt_atrous_halves", "C.pt_halves_stats", "PATHTRACER_GPU_FILTERED_NOISE"):
        assert name in go, name
    main = open(os.path.join(ROOT, "go", "cmd", "render", "main.go")).read()
    assert 'flag.Float64("filtered-noise"' in main
