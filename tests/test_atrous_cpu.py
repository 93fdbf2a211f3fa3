"""Feature planes and the a-trous filter on CPU: the host build of csrc/pt_atrous.h against the independent
restatement tests/atrous_reference.c, bit for bit, on random inputs and on oracle-derived inputs; the model's properties; what the
filter does to the noise and to the relative error of the five shipped scenes, from oracle samples only; and the surface (struct
sizes, flags, environment variables, argument refusals, off by default).  No compute calls on a device here."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import atrous_support as at
import moments_support as ms
from conftest import ROOT, SCENE_NAMES
from denoise_probe_support import CONFIGS, random_inputs

ENTRY_POINTS = ("pt_set_features", "pt_read_features", "pt_atrous")


@pytest.mark.parametrize("size", [(40, 24), (37, 21)])
def test_host_build_equals_the_restatement_on_random_inputs(size):
    w, h = size
    S, Q, n, feats = random_inputs(w, h, 7 * w + h)
    for T in (0, 1, 5, 6):  # steps 16 and 32 reach past a 24-row frame
        for i, cfg in enumerate(CONFIGS):
            if T in (1, 6) and i not in (0, 4):
                continue
            for counts in (n, None):
                for f in (feats, None):
                    if f is None and i not in (0, 4):
                        continue
                    a = at.host_filter(S, Q, 9, counts, f, iterations=T, **cfg)
                    b = at.ref_filter(S, Q, 9, counts, f, iterations=T, **cfg)
                    at.assert_same_run(a, b, (size, T, cfg, counts is None, f is None))
                    assert a["bad_pixels"] == 5


def test_bad_pixels_pass_through_and_never_spread():
    w, h = 40, 24
    S, Q, n, feats = random_inputs(w, h, 3)
    run = at.host_filter(S, Q, 0, n, feats)
    c0 = at.host_filter(S, Q, 0, n, feats, iterations=0)
    bad = ~(np.isfinite(c0["mean"]).all(axis=2) & np.isfinite(c0["var"]))
    assert int(bad.sum()) == 5 == run["bad_pixels"]
    assert at.same_bits(run["mean"][bad], c0["mean"][bad]) and at.same_bits(run["var"][bad], c0["var"][bad])
    assert np.isfinite(run["mean"][~bad]).all() and np.isfinite(run["var"][~bad]).all()
    # the good pixels are what they are in a frame where the bad ones hold other non-finite sums
    S2 = S.copy()
    S2[bad] = -np.inf
    run2 = at.host_filter(S2, Q, 0, n, feats)
    assert at.same_bits(run["mean"][~bad], run2["mean"][~bad]) and at.same_bits(run["var"][~bad], run2["var"][~bad])


def test_t0_is_the_mean_and_a_constant_image_is_unchanged():
    w, h = 37, 21
    S, Q, n, feats = random_inputs(w, h, 11)
    r0 = at.host_filter(S, Q, 0, n, feats, iterations=0)
    with np.errstate(all="ignore"):
        assert at.same_bits(r0["mean"], S / n[..., None].astype(np.float64))
    # a constant image with zero variance is unchanged bit for bit, whatever the constant
    r = np.random.default_rng(2)
    nn = np.full((h, w), 8, np.uint32)
    for c in (np.array([0.3, 1.7, 0.05]), np.array([0.25, 2.0, 0.5]), r.random(3) * 3, r.random(3) * 1e-3, np.zeros(3)):
        Sc = np.broadcast_to(c * 8.0, (h, w, 3)).copy()
        Qc = np.broadcast_to((c * 8.0) ** 2 / 8.0, (h, w, 3)).copy()
        flat = at.host_filter(Sc, Qc, 8, nn, None, iterations=0)
        assert np.all(flat["var"] == 0.0) and at.same_bits(flat["mean"], np.broadcast_to(c, (h, w, 3)))
        for T in (1, 5, 6):
            for run in (at.host_filter, at.ref_filter):
                got = run(Sc, Qc, 8, nn, None, iterations=T)
                assert at.same_bits(got["mean"], flat["mean"]) and np.all(got["var"] == 0.0) and np.array_equal(got["rgba"], flat["rgba"])


def test_first_hit_of_the_host_build_equals_the_oracle(oracle):
    """pt_atrous.h's first_hit (the feature kernel's body) against ora_hit over the object list, on the primary rays of three
    shipped scenes and on rays from inside and behind the objects."""
    from path_trace_golang_amd import hip, scene

    for name in ("example_simple", "gpu_showcase", "test_comprehensive"):
        from conftest import scene_path

        osc = at.ora_scene_of(name)
        flat = hip.FlatScene(scene.load(scene_path(name)))
        rays = [sum(oracle.primary_ray(osc, ms.W, ms.H, 4, 4, 1, x, y, s), []) for y in range(0, ms.H, 2) for x in range(0, ms.W, 3)
                for s in range(2)]
        r = np.random.default_rng(5)
        for _ in range(300):  # origins among the objects, any direction: back faces, inside hits, misses
            rays.append(list(r.uniform(-3, 3, 3) + (0, 1.5, 0)) + list(r.standard_normal(3)))
        rays = np.ascontiguousarray(rays, np.float64)
        a = np.zeros((len(rays), 8))
        b = np.zeros((len(rays), 8))
        at.product_host().shim_first_hit_many(C.byref(flat.c), len(rays), at.ptr(rays), at.ptr(a))
        at.reference().ar_first_hit_many(C.byref(osc.c), len(rays), at.ptr(rays), at.ptr(b))
        assert at.same_bits(a, b), (name, int(np.count_nonzero(a != b)))
        assert 0 < int(a[:, 0].sum()) < len(rays)


# ---------------------------------------------------------------- the five shipped scenes, from oracle samples only
_measured = {}


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_filter_lowers_noise_and_relative_error_on_the_shipped_scenes(name, oracle):
    S, Q, feats = at.oracle_inputs(name)  # 40 x 24, 16 spp, depth 4, seed 1, k = 4
    got = at.host_filter(S, Q, 16, None, feats)
    ref = at.ref_filter(S, Q, 16, None, feats)
    at.assert_same_run(got, ref, name)
    truth = oracle.render(ms.ora_scene(name), ms.W, ms.H, 8192, 4, seed=8, want=("accum",))["accum"] / 8192.0
    before, after = at.relative_mse(S / 16.0, truth), at.relative_mse(ref["mean"], truth)
    plain = float(np.mean((ref["mean"] - truth) ** 2) / np.mean((S / 16.0 - truth) ** 2))
    print("%s: noise %.4f -> %.4f, relative MSE %.5f -> %.5f (ratio %.3f), plain MSE ratio %.3f"
          % (name, ref["noise_before"], ref["noise_after"], before, after, after / before, plain))
    assert ref["noise_after"] < ref["noise_before"]
    assert after < before
    assert abs(ref["noise_before"] - ms.noise_restated(S, Q, 16)["noise"]) <= 1e-9


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
    assert re.search(r"\}\s*pt_atrous_config\s*;", text) and re.search(r"\}\s*pt_atrous_stats\s*;", text)
    assert lib.pt_abi_version() == 4  # additive: the version stays


def test_null_and_bad_arguments_are_refused_with_a_message():
    from path_trace_golang_amd import capi

    lib = capi.load()
    st = capi.PtAtrousStats()
    for call in (lambda: lib.pt_set_features(None, 4), lambda: lib.pt_read_features(None, None, None, None),
                 lambda: lib.pt_atrous(None, None, None, 0, None, None, C.byref(st))):
        assert call() == capi.PT_ERR_INVALID
        assert lib.pt_last_error()


def test_struct_sizes_in_c99_and_in_ctypes(tmp_path):
    from path_trace_golang_amd import build, capi

    lib = build.build_core()
    assert C.sizeof(capi.PtAtrousConfig) == 40 and C.sizeof(capi.PtAtrousStats) == 40
    src = tmp_path / "consumer.c"
    src.write_text(r'''
#include <stddef.h>
#include <stdio.h>
#include "ptcore.h"
int main(void) {
    typedef void (*fn_t)(void);
    fn_t fns[] = {(fn_t)pt_set_features, (fn_t)pt_read_features, (fn_t)pt_atrous};
    pt_atrous_config c = {5, 0, 4.0, 0.1, 0.1, 0.2};
    pt_atrous_stats s;
    int rc = pt_atrous(0, &c, 0, 0, 0, 0, &s) + 10 * pt_set_features(0, 4);
    printf("%d %d %d %d %d %d %d %d %d\n", (int)sizeof c, (int)offsetof(pt_atrous_config, sigma_l), (int)offsetof(pt_atrous_config, sigma_a),
           (int)sizeof s, (int)offsetof(pt_atrous_stats, iterations), (int)offsetof(pt_atrous_stats, noise_before),
           (int)offsetof(pt_atrous_stats, bad_pixels), rc, (int)(sizeof fns / sizeof fns[0]));
    return 0;
}
''')
    exe = tmp_path / "consumer"
    libdir = os.path.dirname(lib)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe), "-L", libdir, "-lptcore", "-Wl,-rpath," + libdir], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    K, S = capi.PtAtrousConfig, capi.PtAtrousStats
    assert out == [40, K.sigma_l.offset, K.sigma_a.offset, 40, S.iterations.offset, S.noise_before.offset, S.bad_pixels.offset,
                   11 * capi.PT_ERR_INVALID, 3]
    assert (K.sigma_l.offset, K.sigma_a.offset, S.iterations.offset, S.noise_before.offset, S.bad_pixels.offset) == (8, 32, 12, 16, 32)


def test_off_is_the_default():
    from path_trace_golang_amd import engine, hip

    assert hip.AtrousConfig.from_env({}) is None and hip.features_from_env({}) is None
    for fn in (hip.render, engine.render_into):
        p = inspect.signature(fn).parameters
        assert p["atrous"].default is None and p["features"].default in (None, 0)
    c = hip.AtrousConfig()
    assert (c.iterations, c.sigma_l, c.sigma_n, c.sigma_z, c.sigma_a, c.features) == (5, 4.0, 0.1, 0.1, 0.2, None)


def test_atrous_config_from_env():
    from path_trace_golang_amd import hip

    for v in ("1", "true", "ON", "Yes"):
        assert hip.AtrousConfig.from_env({"PATHTRACER_GPU_ATROUS": v}) is not None
    for v in ("0", "", "atrous", "2"):
        assert hip.AtrousConfig.from_env({"PATHTRACER_GPU_ATROUS": v}) is None
    c = hip.AtrousConfig.from_env({"PATHTRACER_GPU_ATROUS": "1", "PATHTRACER_GPU_ATROUS_ITERS": "3", "PATHTRACER_GPU_FEATURES": "8"})
    assert (c.iterations, c.features) == (3, 8)
    for v in ("-1", "7", "x", "1.5"):
        assert hip.AtrousConfig.from_env({"PATHTRACER_GPU_ATROUS": "1", "PATHTRACER_GPU_ATROUS_ITERS": v}).iterations == 5
    for v in ("-1", "x", "1.5"):
        assert hip.features_from_env({"PATHTRACER_GPU_FEATURES": v}) is None
    assert hip.features_from_env({"PATHTRACER_GPU_FEATURES": "0"}) == 0


def test_scene_allows_features_follows_the_bvh_threshold():
    from conftest import scene_path
    from path_trace_golang_amd import hip, scene, synth

    sc = scene.load(scene_path("example_simple"))
    assert hip.scene_allows_features(sc) and hip.scene_allows_features(hip.FlatScene(sc))
    assert not hip.scene_allows_features(sc, shading="gl")
    big = synth.make_scene(300)
    assert not hip.scene_allows_features(big) and not hip.scene_allows_features(hip.FlatScene(big))


def test_render_help_lists_the_atrous_flags():
    from path_trace_golang_amd import build

    build.build_host()
    exe = os.path.join(ROOT, "path_trace_golang_amd", "render")
    r = subprocess.run([exe, "-h"], capture_output=True, text=True)
    assert r.returncode == 0
    assert "  -atrous\n" in r.stderr and "  -atrous-iters int\n" in r.stderr and "  -features int\n" in r.stderr
    bad = subprocess.run([exe, "-atrous-iters", "many"], capture_output=True, text=True)
    assert bad.returncode == 2 and 'invalid value "many" for flag -atrous-iters' in bad.stderr
    bad = subprocess.run([exe, "-atrous=maybe"], capture_output=True, text=True)
    assert bad.returncode == 2 and 'invalid boolean value "maybe" for -atrous' in bad.stderr


def test_host_layer_and_go_source_have_the_switches():
    hpp = open(os.path.join(ROOT, "path_trace_golang_amd", "csrc", "host", "engine.hpp")).read()
    cpp = open(os.path.join(ROOT, "path_trace_golang_amd", "csrc", "host", "engine.cpp")).read()
    assert "void SetAtrous(bool on, int iterations" in hpp and "AtrousFromEnv" in hpp and "void SetFeatures(int k" in hpp
    for name in ("pt_set_features", "pt_atrous", "PATHTRACER_GPU_ATROUS", "PATHTRACER_GPU_FEATURES"):
        assert name in cpp, name
    go = open(os.path.join(ROOT, "go", "internal", "engine", "hip", "hip.go")).read()
    for name in ("C.pt_set_features", "C.pt_atrous", "C.pt_atrous_config{", "PATHTRACER_GPU_ATROUS", "PATHTRACER_GPU_FEATURES"):
        assert name in go, name
    main = open(os.path.join(ROOT, "go", "cmd", "render", "main.go")).read()
    assert 'flag.Bool("atrous"' in main and 'flag.Int("atrous-iters"' in main and 'flag.Int("features"' in main
