"""Second moments and the noise target on CPU: the C-ABI surface (declared, exported, bound, NULL arguments refused, pt_noise
of 40 bytes for C and for ctypes), the NumPy statement of the metric against an independent restatement on the oracle's
moments, the CLI's two flags and the two environment variables.  No compute calls on a device here."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np

import moments_support as ms
from conftest import ROOT

ENTRY_POINTS = ("pt_set_moments", "pt_read_moments", "pt_noise_estimate")


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
        assert sym in bound and capi.has(sym), sym
    assert re.search(r"\}\s*pt_noise\s*;", text)
    assert lib.pt_abi_version() == 4  # additive: the version stays


def test_null_arguments_are_invalid_with_a_message():
    from path_trace_golang_amd import capi

    lib = capi.load()
    nz = capi.PtNoise()
    buf = (C.c_double * 3)()
    for call in (lambda: lib.pt_set_moments(None, 1), lambda: lib.pt_read_moments(None, buf),
                 lambda: lib.pt_noise_estimate(None, C.byref(nz))):
        assert call() == capi.PT_ERR_INVALID
        assert lib.pt_last_error()


def test_pt_noise_is_40_bytes_in_c99_and_in_ctypes(tmp_path):
    from path_trace_golang_amd import build, capi

    lib = build.build_core()
    assert C.sizeof(capi.PtNoise) == 40
    src = tmp_path / "consumer.c"
    src.write_text(r'''
#include <stddef.h>
#include <stdio.h>
#include "ptcore.h"
int main(void) {
    typedef void (*fn_t)(void);
    fn_t fns[] = {(fn_t)pt_set_moments, (fn_t)pt_read_moments, (fn_t)pt_noise_estimate};
    pt_noise n;
    int rc = pt_noise_estimate(0, &n);
    printf("%d %d %d %d %d\n", (int)sizeof(pt_noise), (int)offsetof(pt_noise, pixels), (int)offsetof(pt_noise, spp), rc,
           (int)(sizeof fns / sizeof fns[0]));
    return 0;
}
''')
    exe = tmp_path / "consumer"
    libdir = os.path.dirname(lib)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe), "-L", libdir, "-lptcore", "-Wl,-rpath," + libdir], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [40, capi.PtNoise.pixels.offset, capi.PtNoise.spp.offset, capi.PT_ERR_INVALID, 3]
    assert (capi.PtNoise.pixels.offset, capi.PtNoise.spp.offset) == (16, 32)


def test_noise_estimate_host_equals_the_restatement_on_oracle_moments(oracle):
    from path_trace_golang_amd import hip

    n = 32
    l = ms.samples("example_simple", 4, 1, n)
    S, Q = ms.sums(l)
    # the sample list is the oracle's frame: summed in sample order it is ora.render's accum, bit for bit
    o = oracle.render(ms.ora_scene("example_simple"), ms.W, ms.H, n, 4, seed=1, want=("accum",))
    assert np.array_equal(S.view(np.uint64), o["accum"].view(np.uint64))
    got = hip.noise_estimate_host(S, Q, n)
    want = ms.noise_restated(S, Q, n)
    assert got["pixels"] == want["pixels"] == ms.W * ms.H and got["bad_pixels"] == want["bad_pixels"] == 0 and got["spp"] == n
    assert got["max_pixel"] == want["max_pixel"]  # per pixel the same IEEE operations
    # the two differ only in the order of the 960 adds of the frame sum: 960 * 2^-53 relative at the most, halved by the root
    assert abs(got["noise"] - want["noise"]) <= 960 * 2.0 ** -53 * want["noise"]
    assert 0 < want["noise"] < 10
    # fewer than two samples: no variance estimate
    one = hip.noise_estimate_host(S, Q, 1)
    assert math.isinf(one["noise"]) and one["noise"] > 0
    # a pixel whose sums are not finite contributes nothing and is counted
    Sb, Qb = S.copy(), Q.copy()
    Sb[3, 5, 1] = np.nan
    Qb[7, 39, 0] = np.inf
    bad = hip.noise_estimate_host(Sb, Qb, n)
    wantb = ms.noise_restated(Sb, Qb, n)
    assert bad["bad_pixels"] == wantb["bad_pixels"] == 2 and bad["pixels"] == 960
    assert abs(bad["noise"] - wantb["noise"]) <= 960 * 2.0 ** -53 * wantb["noise"]


def test_render_help_lists_the_noise_flags():
    from path_trace_golang_amd import build

    build.build_host()
    r = subprocess.run([os.path.join(ROOT, "path_trace_golang_amd", "render"), "-h"], capture_output=True, text=True)
    assert r.returncode == 0
    assert "  -noise float\n" in r.stderr and "  -noise-step int\n" in r.stderr
    bad = subprocess.run([os.path.join(ROOT, "path_trace_golang_amd", "render"), "-noise", "loud"], capture_output=True, text=True)
    assert bad.returncode == 2 and 'invalid value "loud" for flag -noise' in bad.stderr


def test_noise_config_from_env():
    from path_trace_golang_amd import hip

    c = hip.NoiseConfig.from_env({})
    assert (c.target, c.step, c.enabled) == (0.0, 16, False)
    c = hip.NoiseConfig.from_env({"PATHTRACER_GPU_NOISE": "0.05", "PATHTRACER_GPU_NOISE_STEP": "8"})
    assert (c.target, c.step, c.enabled) == (0.05, 8, True)
    c = hip.NoiseConfig.from_env({"PATHTRACER_GPU_NOISE": "quiet", "PATHTRACER_GPU_NOISE_STEP": "0"})
    assert (c.target, c.step, c.enabled) == (0.0, 16, False)
    c = hip.NoiseConfig.from_env({"PATHTRACER_GPU_NOISE": "-1", "PATHTRACER_GPU_NOISE_STEP": "x"})
    assert (c.target, c.step) == (0.0, 16)
    c = hip.NoiseConfig.from_env({"PATHTRACER_GPU_NOISE": "inf"})
    assert not c.enabled


def test_go_source_has_the_loop_and_the_flags():
    go = open(os.path.join(ROOT, "go", "internal", "engine", "hip", "hip.go")).read()
    for name in ("C.pt_set_moments", "C.pt_noise_estimate", "C.pt_noise", "PATHTRACER_GPU_NOISE", "PATHTRACER_GPU_NOISE_STEP"):
        assert name in go, name
    main = open(os.path.join(ROOT, "go", "cmd", "render", "main.go")).read()
    assert 'flag.Float64("noise"' in main and 'flag.Int("noise-step"' in main
