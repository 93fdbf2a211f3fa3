"""The history clip of pt_temporal on CPU (step 7a of csrc/pt_temporal.h): the new restatement
(tests/temporal_clip_reference.c) against the old one at gamma = 0 and against the host build of the product's header at every gamma,
bit for bit; a NumPy statement of step 7a applied to the restatement's own reprojected values on synthetic frames that hold every case
the step distinguishes; the quality of the clipped, blended and filtered frame on the shipped scenes at two camera speeds; and the
surface (symbols, the struct's layout, argument refusals, environment, host sources).  No compute calls on a device here."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import atrous_support as at
import denoise_probe_support as dp
import temporal_clip_support as tc
import temporal_support as ts
from conftest import ROOT

ENTRY_POINTS = ("pt_temporal_set_clip", "pt_temporal_clip_stats")
SPP, DEPTH, K = 16, 4, 4
GAMMAS = (0.0, 0.5, 2.5, 1e300)


def sequence(name, w, h, frames, moving=True, step=0.01):
    """Frame f of a sequence: the camera moved by f steps (or not at all), seed 1 + f (test_temporal_cpu.py's)."""
    return [ts.oracle_frame(name, f if moving else 0, w, h, SPP, DEPTH, 1 + f, K, step=step) for f in range(frames)]


# ---------------------------------------------------------------- 1. the restatements and the host build
@pytest.mark.parametrize("moving", [True, False], ids=["moving", "static"])
@pytest.mark.parametrize("size", [(40, 24), (37, 21)])
@pytest.mark.parametrize("name", ["example_simple", "metal_glass_room"])
def test_gamma_zero_is_the_restatement_without_the_clip(name, size, moving, oracle):
    w, h = size
    frames = sequence(name, w, h, 3, moving)
    for alpha in (0.0, 0.2):
        for flt in (dict(), None, dict(iterations=2, sigma_z=0.0)):
            old = ts.run_sequence("ref", frames, flt, alpha=alpha)
            new = tc.run_sequence("ref", frames, flt, 0.0, alpha=alpha)
            for i, (x, y) in enumerate(zip(new, old)):
                ts.assert_same_frame(x, y, (name, size, moving, alpha, flt, i))
                assert x["clipped"] == 0
                assert at.same_bits(x["place"], y["place"])
            assert new[2]["reprojected"] > w * h // 2


@pytest.mark.parametrize("size", [(40, 24), (37, 21)])
@pytest.mark.parametrize("name", ["example_simple", "metal_glass_room", "test_scene"])
def test_host_build_equals_the_restatement(name, size, oracle):
    w, h = size
    frames = sequence(name, w, h, 3)
    for gamma in GAMMAS:
        for flt in (dict(), None):
            a = tc.run_sequence("host", frames, flt, gamma)
            b = tc.run_sequence("ref", frames, flt, gamma)
            for i, (x, y) in enumerate(zip(a, b)):
                tc.assert_same_frame(x, y, (name, size, gamma, flt, i))
                assert x["bad_pixels"] == 0 and x["clipped"] <= x["reprojected"]
            assert a[0]["clipped"] == 0 and a[2]["reprojected"] > w * h // 2
            if gamma == 0.0:
                assert a[1]["clipped"] == 0 and a[2]["clipped"] == 0
            if name == "test_scene" and gamma == 2.5:  # the comparison on the device (test_temporal_clip_gpu.py) means something
                for r in a[1:]:
                    print(name, size, "clipped %d of %d" % (r["clipped"], r["reprojected"]))
                    assert 0 < r["clipped"] < r["reprojected"]
    # a smaller gamma clips no fewer pixels of the first frame with a history (later frames see different histories)
    second = [tc.run_sequence("ref", frames, None, g)[1]["clipped"] for g in (1e300, 2.5, 0.5)]
    assert second[0] <= second[1] <= second[2]


# ---------------------------------------------------------------- 2. synthetic frames: step 7a in NumPy on the restatement's own c_r
BLOCK_A, BLOCK_B, BLOCK_C, planted_frames = tc.BLOCK_A, tc.BLOCK_B, tc.BLOCK_C, tc.planted_frames


def check_frame_against_numpy(fr, res, gamma, tag):
    """Step 7a and the blend of step 8 in NumPy, from the restatement's c_r, var_r and a, against what the restatement stored.
    Returns (rep, below, above, half, c_i, var_i, clipped c_r)."""
    ci, var_i = tc.prep_frame(fr)
    cr, var_r, a = res["repro"][..., :3], res["repro"][..., 3], res["repro"][..., 4]
    rep = np.isfinite(a)
    assert int(np.count_nonzero(rep)) == res["reprojected"], tag
    if gamma > 0:
        crc, below, above, half = tc.clip_numpy(gamma, ci, var_i, cr, var_r)
    else:
        crc, below, above, half = cr, np.zeros(cr.shape, bool), np.zeros(cr.shape, bool), np.zeros(a.shape)
    changed = rep & (below | above).any(axis=2)
    assert int(np.count_nonzero(changed)) == res["clipped"], (tag, int(np.count_nonzero(changed)), res["clipped"])
    want = tc.blend_numpy(ci, crc, np.where(rep, a, 0.0))
    assert at.same_bits(res["hist_mean"][rep], want[rep]), (tag, "blend of the clipped history")
    assert at.same_bits(res["hist_mean"][~rep], ci[~rep]), (tag, "the frame passes through")
    with np.errstate(all="ignore"):
        vwant = ((1 - a) * (1 - a)) * var_r + (a * a) * var_i
    assert at.same_bits(res["hist_var"][rep], vwant[rep]), (tag, "var_r is not clipped")
    return rep, below, above, half, ci, var_i, crc


def test_every_case_of_the_clip_on_synthetic_frames():
    frames = planted_frames()
    gamma = 0.5
    out = tc.run_sequence("ref", frames, None, gamma)
    fr, res = frames[1], out[1]
    rep, below, above, half, ci, var_i, crc = check_frame_against_numpy(fr, res, gamma, "planted")
    cr, var_r = res["repro"][..., :3], res["repro"][..., 3]
    lo_px, hi_px = rep & below.any(axis=2) & ~above.any(axis=2), rep & above.any(axis=2) & ~below.any(axis=2)
    some = rep & (below | above).any(axis=2) & ~(below | above).all(axis=2)
    print("lo only %d, hi only %d, some channels only %d, clipped %d of %d" % (np.count_nonzero(lo_px), np.count_nonzero(hi_px),
                                                                             np.count_nonzero(some), res["clipped"], res["reprojected"]))
    assert lo_px.any() and hi_px.any() and some.any()
    assert 0 < res["clipped"] < res["reprojected"]
    # A: var_i = var_r = 0 and c_r != c_i: the history becomes the frame exactly
    assert rep[BLOCK_A] and var_i[BLOCK_A] == 0.0 and var_r[BLOCK_A] == 0.0 and half[BLOCK_A] == 0.0
    assert np.all(ci[BLOCK_A] == 2.0) and np.all(np.abs(cr[BLOCK_A] - 3.0) < 1e-9)
    assert at.same_bits(res["hist_mean"][BLOCK_A], ci[BLOCK_A]) and res["hist_var"][BLOCK_A] == 0.0
    # B: c_r lies exactly on hi (and on lo): neither changed nor counted
    assert rep[BLOCK_B] and half[BLOCK_B] == 0.0 and np.all(cr[BLOCK_B] == ci[BLOCK_B] + half[BLOCK_B])
    assert not below[BLOCK_B].any() and not above[BLOCK_B].any()
    # C: s <= 0 through prep's clamp (Q / n < c^2) and a history of zero variance
    n = float(fr["n"])
    assert np.all(fr["Q"][BLOCK_C] / n < ci[BLOCK_C] * ci[BLOCK_C]) and var_i[BLOCK_C] == 0.0 and var_r[BLOCK_C] == 0.0
    assert rep[BLOCK_C] and not (var_i[BLOCK_C] + var_r[BLOCK_C] > 0) and at.same_bits(res["hist_mean"][BLOCK_C], ci[BLOCK_C])
    assert (below[BLOCK_C] | above[BLOCK_C]).any()
    # a bad pixel beside a clipped one: it passes through with len' = 0, its neighbour is clipped all the same
    clipped = rep & (below | above).any(axis=2)
    beside = 0
    for (y, x) in fr["bad"]:
        assert not rep[y, x] and res["hist_len"][y, x] == 0 and at.same_bits(res["hist_mean"][y, x], ci[y, x])
        beside += sum(1 for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0)) if 0 <= y + dy < 37 and 0 <= x + dx < 70 and clipped[y + dy, x + dx])
    assert beside > 0 and res["bad_pixels"] == 3
    # the host build agrees on these frames too
    host = tc.run_sequence("host", frames, None, gamma)
    for x, y in zip(host, out):
        tc.assert_same_frame(x, y, "planted, host")


@pytest.mark.parametrize("name", ["sideways", "sideways 33 x 9", "sideways 97 x 71"])
def test_all_clipped_none_clipped_and_numpy_on_the_moving_walls(name):
    frames = dp.sequence(name)[:4]
    off = tc.run_sequence("ref", frames, None, 0.0)
    for gamma in (1e-6, 0.5, 2.5, 1e300):
        out = tc.reference_run(name, frames, None, gamma)
        for k in range(1, len(frames)):
            check_frame_against_numpy(frames[k], out[k], gamma, (name, gamma, k))
            assert out[k]["reprojected"] > 0
        if gamma == 1e-6:  # every reprojected pixel is clipped
            assert all(o["clipped"] == o["reprojected"] for o in out[1:]), [(o["clipped"], o["reprojected"]) for o in out]
        if gamma == 1e300:  # none is, and every bit is gamma = 0's
            for k, (x, y) in enumerate(zip(out, off)):
                assert x["clipped"] == 0
                tc.assert_same_frame(x, y, (name, "1e300 against 0", k))
        if gamma in (0.5, 2.5):
            assert all(0 < o["clipped"] < o["reprojected"] for o in out[1:]), [(o["clipped"], o["reprojected"]) for o in out]
    check_frame_against_numpy(frames[1], off[1], 0.0, (name, "off"))


def test_a_nan_half_changes_nothing():
    """The comparisons are written so that a NaN half changes nothing.  The C ABI refuses an infinite gamma; the model does not need
    to: on the planted frames s = 0 in the three blocks, so half = inf * 0 is a NaN there and infinite everywhere else, and every bit
    is gamma = 0's."""
    frames = planted_frames()
    off = tc.run_sequence("ref", frames, None, 0.0)
    assert off[1]["reprojected"] > 0
    for kind in ("ref", "host"):
        for x, y in zip(tc.run_sequence(kind, frames, None, float("inf")), off):
            tc.assert_same_frame(x, y, kind)
    ci = np.array([[1.0, 2.0, 3.0]])
    out, below, above, half = tc.clip_numpy(float("inf"), ci, np.array([0.0]), np.array([[9.0, -9.0, 3.0]]), np.array([0.0]))
    assert np.isnan(half).all() and not below.any() and not above.any() and np.array_equal(out, [[9.0, -9.0, 3.0]])


# ---------------------------------------------------------------- 3. quality, from oracle samples only
QUALITY_FRAMES = 6


@pytest.mark.parametrize("step", [0.01, 0.03])
@pytest.mark.parametrize("name", ["example_simple", "metal_glass_room", "gpu_showcase", "test_comprehensive", "test_scene"])
def test_clipped_history_then_filter(name, step, oracle):
    """DESIGN 3.13's set-up (40 x 24, 16 spp, depth 4, k = 4, six frames, seeds 1 + f, defaults everywhere; relative MSE of the last
    frame against a 4096-spp oracle frame of the last camera, seed 977) with the camera moved sideways by `step` of its distance to the
    target per frame; the clip off and at the recommended gamma.  test_scene, which the history made worse, must gain on the filter
    alone and on the unclipped history; the other scenes must still gain on the filter alone and may lose at most a twentieth against
    the unclipped history."""
    w, h = 40, 24
    frames = sequence(name, w, h, QUALITY_FRAMES, step=step)
    last = frames[-1]
    truth = oracle.render(ts.ora_scene(name, QUALITY_FRAMES - 1, step), w, h, 4096, DEPTH, seed=977, want=("accum",))["accum"] / 4096.0
    e_alone = at.relative_mse(at.ref_filter(last["S"], last["Q"], SPP, None, last["feats"])["mean"], truth)
    off = tc.run_sequence("ref", frames, dict(), 0.0)[-1]
    on = tc.run_sequence("ref", frames, dict(), tc.GAMMA)[-1]
    e_off, e_on = at.relative_mse(off["mean"], truth), at.relative_mse(on["mean"], truth)
    print("| %s | %.2f | %.3f | %.3f | %.3f | %.3f | %.2f |" % (name, step, e_alone, e_off, e_on, e_on / e_off, on["clipped"] / max(on["reprojected"], 1)))
    assert e_on < e_alone, (name, step, e_on, e_alone)
    if name == "test_scene":
        assert e_on < e_off, (name, step, e_on, e_off)
    else:
        assert e_on <= 1.05 * e_off, (name, step, e_on, e_off)


# ---------------------------------------------------------------- 4. the surface
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
    assert re.search(r"struct\s+pt_temporal_clip_stats\s*\{", text)
    assert lib.pt_abi_version() == 4  # additive: the version stays


def test_null_and_bad_arguments_are_refused_with_a_message():
    from path_trace_golang_amd import capi, hip

    lib = capi.load()
    st = capi.PtTemporalClipStats()
    for call in (lambda: lib.pt_temporal_set_clip(None, 2.5), lambda: lib.pt_temporal_clip_stats(None, C.byref(st))):
        assert call() == capi.PT_ERR_INVALID
        assert lib.pt_last_error()
    with pytest.raises(ValueError):
        hip.render(None, hip.RenderConfig(4, 4, 2, 2, 1), np.zeros((4, 4, 4), np.uint8), temporal_clip=2.5)  # without temporal=


def test_struct_layout_in_c99_and_in_ctypes(tmp_path):
    from path_trace_golang_amd import build, capi

    lib = build.build_core()
    S = capi.PtTemporalClipStats
    assert C.sizeof(S) == 24
    assert C.sizeof(capi.PtTemporalConfig) == 40 and C.sizeof(capi.PtTemporalStats) == 72  # no existing struct changed size
    src = tmp_path / "consumer.c"
    src.write_text(r'''
#include <stddef.h>
#include <stdio.h>
#include "ptcore.h"
int main(void) {
    typedef void (*fn_t)(void);
    fn_t fns[] = {(fn_t)pt_temporal_set_clip, (fn_t)pt_temporal_clip_stats};
    struct pt_temporal_clip_stats s;
    int rc = pt_temporal_set_clip(0, 2.5) + 10 * pt_temporal_clip_stats(0, &s);
    printf("%d %d %d %d\n", (int)sizeof s, (int)offsetof(struct pt_temporal_clip_stats, gamma),
           (int)offsetof(struct pt_temporal_clip_stats, clipped), (int)offsetof(struct pt_temporal_clip_stats, reprojected));
    printf("%d %d %d %d\n", rc, (int)(sizeof fns / sizeof fns[0]), (int)sizeof(pt_temporal_config), (int)sizeof(pt_temporal_stats));
    return 0;
}
''')
    exe = tmp_path / "consumer"
    libdir = os.path.dirname(lib)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe), "-L", libdir, "-lptcore", "-Wl,-rpath," + libdir], check=True)
    lines = [[int(x) for x in l.split()] for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert lines[0] == [24] + [getattr(S, n).offset for n in ("gamma", "clipped", "reprojected")]
    assert lines[0] == [24, 0, 8, 16]
    assert lines[1] == [11 * capi.PT_ERR_INVALID, 2, 40, 72]
    # ... and C++ sees the struct beside the function of the same name
    cpp = tmp_path / "consumer.cpp"
    cpp.write_text('#include "ptcore.h"\nint main() { struct pt_temporal_clip_stats s; return pt_temporal_clip_stats(nullptr, &s) == 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(cpp), "-o", str(tmp_path / "cpp"),
                    "-L", libdir, "-lptcore", "-Wl,-rpath," + libdir], check=True)


def test_the_environment_variable_and_the_arguments():
    from path_trace_golang_amd import engine, hip

    assert tc.GAMMA == 2.5 and "RECOMMENDED: 2.5" in open(os.path.join(ROOT, "include", "ptcore.h")).read()
    assert hip.temporal_clip_from_env({}) == 0.0  # unset means off
    for v, want in (("2.5", 2.5), ("0", 0.0), ("", 0.0), ("3", 3.0), ("1e-3", 1e-3), ("nan", 0.0), ("-1", 0.0), ("inf", 0.0), ("on", 0.0)):
        assert hip.temporal_clip_from_env({"PATHTRACER_GPU_TEMPORAL_CLIP": v}) == want, v
    for fn in (hip.render, engine.render_into):
        assert inspect.signature(fn).parameters["temporal_clip"].default is None  # the context's setting, which is off unless asked for
    assert "temporal_clip_from_env" in inspect.getsource(engine.render_into)
    # the existing switch is what it was
    assert engine.temporal_setup({}) == (None, None, None)
    assert engine.temporal_setup({"PATHTRACER_GPU_TEMPORAL_CLIP": "2.5"}) == (None, None, None)


def test_host_layers_and_go_source_have_the_calls():
    hpp = open(os.path.join(ROOT, "path_trace_golang_amd", "csrc", "host", "engine.hpp")).read()
    cpp = open(os.path.join(ROOT, "path_trace_golang_amd", "csrc", "host", "engine.cpp")).read()
    assert "SetTemporalClip(" in hpp and "TemporalClipStats(" in hpp
    for name in ("pt_temporal_set_clip", "pt_temporal_clip_stats", "PATHTRACER_GPU_TEMPORAL_CLIP"):
        assert name in cpp, name
    go = open(os.path.join(ROOT, "go", "internal", "engine", "hip", "hip.go")).read()
    for name in ("C.pt_temporal_set_clip(", "C.pt_temporal_clip_stats(", "C.struct_pt_temporal_clip_stats", "func SetTemporalClip(",
                 "func TemporalClipStats(", "PATHTRACER_GPU_TEMPORAL_CLIP"):
        assert name in go, name
    bench = open(os.path.join(ROOT, "tools", "temporal_bench.py")).read()
    assert "--clip" in bench
    py = open(os.path.join(ROOT, "path_trace_golang_amd", "hip.py")).read()
    assert "PATHTRACER_GPU_TEMPORAL_CLIP" in py


def test_the_old_probe_and_the_old_shim_compile_unedited_and_give_the_bits_of_gamma_zero(oracle):
    """tests/denoise_probe.hip zero-fills TemporalArgs and temporal_support's shim default-constructs ptt::Config: neither names
    clip_gamma, both must still build, and the shim must give the new restatement's gamma = 0 bits."""
    assert "clip_gamma" not in ts.SHIM and "clip_gamma" not in open(dp.SOURCE).read()
    frames = sequence("test_scene", 37, 21, 3)
    a = ts.run_sequence("host", frames, dict())
    b = tc.run_sequence("ref", frames, dict(), 0.0)
    for i, (x, y) in enumerate(zip(a, b)):
        ts.assert_same_frame(x, y, i)
    dp.compile_probe()
