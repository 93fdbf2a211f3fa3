"""Temporal accumulation on CPU: the host build of csrc/pt_temporal.h against the restatement
(tests/temporal_reference.c), bit for bit, on camera sequences made from oracle samples; the properties of the model (an unmoved
camera lands on its own pixel, alpha = 0 with open tolerances is the running mean, a NaN does not spread, reset and a size change
empty the history); the quality of the blended-and-filtered frame against the filter alone on the shipped scenes; and the surface
(symbols, struct layouts, argument refusals, environment, host sources).  No compute calls on a device here."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import atrous_support as at
import temporal_support as ts
from conftest import ROOT

ENTRY_POINTS = ("pt_temporal", "pt_temporal_read", "pt_temporal_reset")
SPP, DEPTH, K = 16, 4, 4


def sequence(name, w, h, frames, moving=True):
    """Frame f of a sequence: the camera moved by f steps (or not at all), seed 1 + f."""
    return [ts.oracle_frame(name, f if moving else 0, w, h, SPP, DEPTH, 1 + f, K) for f in range(frames)]


# ---------------------------------------------------------------- the host build against the restatement
@pytest.mark.parametrize("moving", [True, False], ids=["moving", "static"])
@pytest.mark.parametrize("size", [(40, 24), (37, 21)])
@pytest.mark.parametrize("name", ["example_simple", "metal_glass_room"])
def test_host_build_equals_the_restatement(name, size, moving, oracle):
    w, h = size
    frames = sequence(name, w, h, 3, moving)
    if name == "metal_glass_room":
        assert frames[0]["cam"][21] > 0  # a thin lens
    for alpha in (0.0, 0.2):
        for flt in (dict(), None, dict(iterations=2, sigma_z=0.0)):
            a = ts.run_sequence("host", frames, flt, alpha=alpha)
            b = ts.run_sequence("ref", frames, flt, alpha=alpha)
            for i, (x, y) in enumerate(zip(a, b)):
                ts.assert_same_frame(x, y, (name, size, moving, alpha, flt, i))
                assert x["bad_pixels"] == 0
            assert a[0]["reprojected"] == 0 and a[0]["disoccluded"] == 0 and np.all(a[0]["hist_len"] == 1)
            assert a[2]["reprojected"] > w * h // 2 and a[2]["hist_len"].max() == 3
            if flt is None:  # the output is the stored history
                assert at.same_bits(a[2]["mean"], a[2]["hist_mean"]) and a[2]["noise_after"] == a[2]["noise_blended"]
            else:           # ... which is kept before the filter
                assert not at.same_bits(a[2]["mean"], a[2]["hist_mean"])


@pytest.mark.parametrize("name", ["example_simple", "metal_glass_room"])
def test_an_unmoved_camera_lands_on_its_own_pixel(name, oracle):
    for w, h in ((40, 24), (37, 21)):
        frames = sequence(name, w, h, 2, moving=False)
        for kind in ("host", "ref"):
            r = ts.run_sequence(kind, frames)[1]
            hit = frames[1]["feats"][2][..., 1] > 0
            assert hit.any() and ((~hit).any() or name != "example_simple")  # pixels that hit and, outside the closed room, pixels that see the sky
            yy, xx = np.mgrid[0:h, 0:w]
            assert np.all(np.abs(r["place"][..., 0] - xx) <= 1e-9) and np.all(np.abs(r["place"][..., 1] - yy) <= 1e-9), (name, kind)


def _neighbourhood_max(a):
    """Per pixel the largest value of `a` ([H, W] or [H, W, 3]) over its 3 x 3 neighbourhood (edge pixels repeated)."""
    h, w = a.shape[:2]
    p = np.pad(a, ((1, 1), (1, 1)) + ((0, 0),) * (a.ndim - 2), mode="edge")
    return np.max(np.stack([p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy in (-1, 0, 1) for dx in (-1, 0, 1)]), axis=0)


@pytest.mark.parametrize("name", ["metal_glass_room", "gpu_showcase"])
def test_alpha_zero_with_open_tolerances_is_the_running_mean(name, oracle):
    """Static camera, alpha = 0, tolerances opened, F = 4 frames of seeds 1..4: a = 1 / (len + 1) makes the history the running
    mean.  The scenes are the two whose every pixel hits in every frame: `hit_h == hit_i` is not a tolerance, so on a silhouette
    against the sky, where the feature samples of two seeds disagree about the hit, a pixel starts again by the model's own rule.
    "1e-12 relative" is relative to the largest magnitude in the pixel's 3 x 3 neighbourhood over the F frames: an unmoved camera
    lands within d <= 1e-9 of a pixel of its own pixel (the test above), not on it, and a bilinear tap d away mixes in d times the
    neighbour -- next to a pixel a hundred times brighter, or for a channel that is exactly 0, the pixel's own value is no scale."""
    w, h, F = 40, 24, 4
    frames = sequence(name, w, h, F, moving=False)
    assert all(np.all(f["feats"][2][..., 1] > 0) for f in frames)
    per_mean = np.stack([f["S"] / SPP for f in frames])
    per_var = np.stack([at.ref_filter(f["S"], f["Q"], SPP, None, f["feats"], iterations=0)["var"] for f in frames])
    want_mean, want_var = per_mean.mean(axis=0), per_var.sum(axis=0) / F ** 2
    scale_mean, scale_var = _neighbourhood_max(np.abs(per_mean).max(axis=0)), _neighbourhood_max(per_var.max(axis=0))
    for kind in ("host", "ref"):
        last = ts.run_sequence(kind, frames, None, alpha=0.0, **ts.OPEN)[-1]
        assert last["bad_pixels"] == 0 and np.all(last["hist_len"] == F) and last["reprojected"] == w * h and last["mean_len"] == F
        em, ev = np.abs(last["mean"] - want_mean) / scale_mean, np.abs(last["var"] - want_var) / scale_var
        print(name, kind, "mean %.3g var %.3g" % (em.max(), ev.max()))
        assert em.max() <= 1e-12 and ev.max() <= 1e-12, (name, kind, em.max(), ev.max())


def test_a_nan_passes_through_and_does_not_spread(oracle):
    w, h = 40, 24
    frames = [dict(f) for f in sequence("example_simple", w, h, 3)]
    S = frames[1]["S"].copy()
    S[11, 17, 1] = np.nan
    frames[1]["S"] = S
    for kind in ("host", "ref"):
        out = ts.run_sequence(kind, frames, dict(), **ts.OPEN)
        mid, nxt = out[1], out[2]
        assert mid["bad_pixels"] == 1 and mid["hist_len"][11, 17] == 0 and np.isnan(mid["mean"][11, 17, 1])
        assert at.same_bits(mid["mean"][11, 17], (S / SPP)[11, 17])  # passed through
        rest = np.ones((h, w), bool)
        rest[11, 17] = False
        for r in (mid, nxt):
            assert np.isfinite(r["mean"][rest]).all() and np.isfinite(r["var"][rest]).all() and np.isfinite(r["hist_mean"][rest]).all()
        assert np.isfinite(nxt["mean"]).all() and nxt["bad_pixels"] == 0  # nothing read from the bad tap
        assert nxt["hist_len"].min() >= 1


def test_reset_and_a_size_change_empty_the_history(oracle):
    a = sequence("example_simple", 40, 24, 2)
    b = sequence("example_simple", 37, 21, 2)
    for kind in ("host", "ref"):
        acc = ts.Accumulator(kind)
        assert acc.read(40, 24) is None
        run = lambda f: acc.frame(f["S"], f["Q"], f["n"], f["feats"], f["cam"])
        run(a[0])
        assert run(a[1])["reprojected"] > 0
        r = run(b[0])  # another size
        assert r["reprojected"] == 0 and r["disoccluded"] == 0 and np.all(r["hist_len"] == 1)
        assert run(b[1])["reprojected"] > 0
        acc.reset()
        assert acc.read(37, 21) is None
        r = run(b[0])
        assert r["reprojected"] == 0 and np.all(r["hist_len"] == 1)
        acc.close()


# ---------------------------------------------------------------- quality, from oracle samples only
QUALITY_FRAMES = 6


@pytest.mark.parametrize("name", ["example_simple", "metal_glass_room", "gpu_showcase", "test_comprehensive", "test_scene"])
def test_history_then_filter_beats_the_filter_alone(name, oracle):
    """40 x 24, 16 spp, depth 4, k = 4, six frames, the camera moved sideways by 1 % of its distance to the target per frame, seeds
    1 + f, defaults everywhere; relative MSE against a 4096-spp oracle frame of the last camera.  test_scene is printed, not
    asserted: one frame of its sequence holds a firefly, which an exponential history keeps for several frames."""
    w, h = 40, 24
    frames = sequence(name, w, h, QUALITY_FRAMES)
    last = frames[-1]
    truth = oracle.render(ts.ora_scene(name, QUALITY_FRAMES - 1), w, h, 4096, DEPTH, seed=977, want=("accum",))["accum"] / 4096.0
    alone = at.ref_filter(last["S"], last["Q"], SPP, None, last["feats"])
    out = ts.run_sequence("ref", frames, dict())[-1]
    e_raw = at.relative_mse(last["S"] / SPP, truth)
    e_alone = at.relative_mse(alone["mean"], truth)
    e_blend = at.relative_mse(out["hist_mean"], truth)
    e_both = at.relative_mse(out["mean"], truth)
    print("| %s | %.3f | %.3f | %.3f | %.3f | %.2f | %.2f |" % (name, e_raw, e_alone, e_blend, e_both, out["reprojected"] / (w * h), out["mean_len"]))
    if name != "test_scene":
        assert e_both < e_alone, (name, e_both, e_alone)


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
    assert re.search(r"\}\s*pt_temporal_config\s*;", text) and re.search(r"\}\s*pt_temporal_stats\s*;", text)
    assert lib.pt_abi_version() == 4  # additive: the version stays


def test_null_and_bad_arguments_are_refused_with_a_message():
    from path_trace_golang_amd import capi, hip

    lib = capi.load()
    st = capi.PtTemporalStats()
    for call in (lambda: lib.pt_temporal(None, None, None, None, 0, None, None, C.byref(st)),
                 lambda: lib.pt_temporal_read(None, None, None, None), lambda: lib.pt_temporal_reset(None)):
        assert call() == capi.PT_ERR_INVALID
        assert lib.pt_last_error()
    with pytest.raises(ValueError):
        hip.temporal(None, None, None, np.zeros((4, 4, 3), np.uint8))
    with pytest.raises(ValueError):
        hip.temporal(None, None, None, None, mean=np.zeros((4, 4, 3), np.float32))
    with pytest.raises(ValueError):
        hip.temporal(None, None, None, np.zeros((4, 4, 4), np.uint8), var=np.zeros((4, 5)))
    with pytest.raises(ValueError):
        hip.temporal_read(None, length=np.zeros((4, 4), np.int64))
    with pytest.raises(ValueError):
        hip.temporal_read(None, np.zeros((4, 4, 3)), np.zeros((4, 5)))


def test_struct_layouts_in_c99_and_in_ctypes(tmp_path):
    from path_trace_golang_amd import build, capi

    lib = build.build_core()
    Cf, S = capi.PtTemporalConfig, capi.PtTemporalStats
    assert C.sizeof(Cf) == 40 and C.sizeof(S) == 72
    src = tmp_path / "consumer.c"
    src.write_text(r'''
#include <stddef.h>
#include <stdio.h>
#include "ptcore.h"
int main(void) {
    typedef void (*fn_t)(void);
    fn_t fns[] = {(fn_t)pt_temporal, (fn_t)pt_temporal_read, (fn_t)pt_temporal_reset};
    pt_temporal_stats s;
    int rc = pt_temporal(0, 0, 0, 0, 0, 0, 0, &s) + 10 * pt_temporal_read(0, 0, 0, 0) + 100 * pt_temporal_reset(0);
    printf("%d %d %d %d %d %d %d\n", (int)sizeof(pt_temporal_config), (int)offsetof(pt_temporal_config, alpha),
           (int)offsetof(pt_temporal_config, tol_z), (int)offsetof(pt_temporal_config, n_min), (int)offsetof(pt_temporal_config, tol_a),
           (int)offsetof(pt_temporal_config, max_len), (int)offsetof(pt_temporal_config, reserved));
    printf("%d %d %d %d %d %d %d %d %d %d %d\n", (int)sizeof s, (int)offsetof(pt_temporal_stats, temporal_ms),
           (int)offsetof(pt_temporal_stats, launches), (int)offsetof(pt_temporal_stats, iterations),
           (int)offsetof(pt_temporal_stats, reprojected), (int)offsetof(pt_temporal_stats, disoccluded),
           (int)offsetof(pt_temporal_stats, bad_pixels), (int)offsetof(pt_temporal_stats, mean_len),
           (int)offsetof(pt_temporal_stats, noise_before), (int)offsetof(pt_temporal_stats, noise_blended),
           (int)offsetof(pt_temporal_stats, noise_after));
    printf("%d %d\n", rc, (int)(sizeof fns / sizeof fns[0]));
    return 0;
}
''')
    exe = tmp_path / "consumer"
    libdir = os.path.dirname(lib)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe), "-L", libdir, "-lptcore", "-Wl,-rpath," + libdir], check=True)
    lines = [[int(x) for x in l.split()] for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert lines[0] == [40] + [getattr(Cf, n).offset for n in ("alpha", "tol_z", "n_min", "tol_a", "max_len", "reserved")]
    assert lines[0] == [40, 0, 8, 16, 24, 32, 36]
    names = ("temporal_ms", "launches", "iterations", "reprojected", "disoccluded", "bad_pixels", "mean_len", "noise_before",
             "noise_blended", "noise_after")
    assert lines[1] == [72] + [getattr(S, n).offset for n in names]
    assert lines[1] == [72, 0, 8, 12, 16, 24, 32, 40, 48, 56, 64]
    assert lines[2] == [111 * capi.PT_ERR_INVALID, 3]


def test_config_defaults_and_the_environment_switch():
    from path_trace_golang_amd import engine, hip

    c = hip.TemporalConfig()
    assert (c.alpha, c.max_len, c.tol_z, c.n_min, c.tol_a) == (0.2, 32, 0.1, 0.9, 0.05)
    cc = hip.TemporalConfig(0.5, 8, 0.2, 0.8, 0.1).c()
    assert (cc.alpha, cc.tol_z, cc.n_min, cc.tol_a, cc.max_len, cc.reserved) == (0.5, 0.2, 0.8, 0.1, 8, 0)
    assert hip.TemporalConfig.from_env({}) is None
    for v in ("0", "", "off", "2"):
        assert hip.TemporalConfig.from_env({"PATHTRACER_GPU_TEMPORAL": v}) is None
    for v in ("1", "true", "ON", "yes"):
        assert hip.TemporalConfig.from_env({"PATHTRACER_GPU_TEMPORAL": v}) == hip.TemporalConfig()
    for fn in (hip.render, engine.render_into):
        assert inspect.signature(fn).parameters["temporal"].default is None  # off unless asked for
    assert engine.temporal_setup({}) == (None, None, None)
    t, a, k = engine.temporal_setup({"PATHTRACER_GPU_TEMPORAL": "1"})
    assert t == hip.TemporalConfig() and a == hip.AtrousConfig() and k == 4  # moments come with the filter
    t, a, k = engine.temporal_setup({"PATHTRACER_GPU_TEMPORAL": "1", "PATHTRACER_GPU_FEATURES": "8", "PATHTRACER_GPU_ATROUS_ITERS": "3"})
    assert k == 8 and a.iterations == 3


def test_the_one_shot_cli_has_no_temporal_flag():
    from path_trace_golang_amd import build

    build.build_host()
    r = subprocess.run([os.path.join(ROOT, "path_trace_golang_amd", "render"), "-h"], capture_output=True, text=True)
    assert r.returncode == 0 and "temporal" not in r.stderr  # one frame, no history


def test_host_layer_and_go_source_have_the_calls():
    hpp = open(os.path.join(ROOT, "path_trace_golang_amd", "csrc", "host", "engine.hpp")).read()
    cpp = open(os.path.join(ROOT, "path_trace_golang_amd", "csrc", "host", "engine.cpp")).read()
    assert "void SetTemporal(" in hpp and "Temporal(" in hpp
    for name in ("pt_temporal", "pt_temporal_reset", "PATHTRACER_GPU_TEMPORAL"):
        assert name in cpp, name
    go = open(os.path.join(ROOT, "go", "internal", "engine", "hip", "hip.go")).read()
    for name in ("C.pt_temporal(", "C.pt_temporal_reset(", "C.pt_temporal_config", "C.pt_temporal_stats", "func SetTemporal(", "func Temporal(",
                 "PATHTRACER_GPU_TEMPORAL"):
        assert name in go, name
