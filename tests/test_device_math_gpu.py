"""The shared headers on the device, routine by routine (tests/device_probe.hip): pt_math.h's Go routines, square roots and
sample streams against the oracle and numpy's correctly rounded sqrt; pt_fog.h's hash, noise, phase function and the whole
in-scatter term, pt_glshade.h's pass sum, against the independent restatements and the g++ host builds.

pt_fog.h and pt_glshade.h promise that the gfx950 build gives the bits of the host build.  The device takes other paths
(a hand-written v_rsq_f64 refinement for the root, the ldexp builtin, a ballot to leave the shadow loops, the compiler's
device division and floor), so that promise is checked here on the uint64 view of every result: no tolerance.  The one
thing not compared is the payload of a NaN -- Go's math.NaN(), C's NAN and a propagated operand differ in it and nothing
reads it: where the reference is NaN the device must give NaN."""
from __future__ import annotations

import ctypes as C
import json
import math
import time

import numpy as np
import pytest

import device_probe_support as dp
import fog_support as fs
import glshade_support as gs
from conftest import scene_path
from test_fog_cpu import FOG_TABLE, _rays, fuzz_scene, sin_range_arguments, sin_special_arguments

pytestmark = pytest.mark.gpu

ORA_SIN, ORA_COS, ORA_TAN, ORA_EXP = range(4)
ORA_POW, ORA_MIN, ORA_MAX = range(3)
LIM = 2.0 ** 29
MAXF = 1.7976931348623157e308


@pytest.fixture(autouse=True, scope="module")
def _probe():
    L = dp.load()  # torch first, then the probe: one HIP runtime in the process
    n = C.c_int(0)
    assert L.probe_device_count(C.byref(n)) == 0 and n.value >= 1, "the gpu-marked tests must run on the GPU box"


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(got, want):
    """Bit-equal, or NaN where the reference is NaN."""
    return (_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))


def _check(what, got, want, *operands):
    ok = _same(got, want)
    bad = np.flatnonzero(~ok.reshape(ok.shape[0], -1).all(1))
    print("%s: %d results, %d differ" % (what, ok.shape[0], bad.size))
    assert bad.size == 0, (what, bad.size, [np.asarray(o)[bad[:5]] for o in operands], np.asarray(got)[bad[:5]],
                           np.asarray(want)[bad[:5]])


def _ora1(which, x):
    x = np.ascontiguousarray(x, np.float64)
    out = np.empty_like(x)
    fs.reference().fr_ora_unary_many(which, fs.ptr(x), fs.ptr(out), x.size)
    return out


def _ora2(which, a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    out = np.empty_like(a)
    fs.reference().fr_ora_binary_many(which, fs.ptr(a), fs.ptr(b), fs.ptr(out), a.size)
    return out


def _around(values, ulps=3):
    """Every value with its neighbours up to `ulps` away on both sides."""
    out = []
    for v in values:
        lo = hi = np.float64(v)
        out.append(lo)
        for _ in range(ulps):
            lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
            out += [lo, hi]
    return np.array(out, np.float64)


# ---------------------------------------------------------------- pt_math.h

def test_go_sin_and_sincos_pos_on_the_device_equal_the_oracle():
    x = np.concatenate([sin_range_arguments(), sin_special_arguments()])
    assert x.size >= 1_000_000
    got = dp.unary(dp.U_SIN, x)
    _check("go_sin", got, _ora1(ORA_SIN, x), x)
    assert math.copysign(1.0, got[np.flatnonzero(_bits(x) == _bits(np.array([-0.0]))[0])[0]]) == -1.0  # -0 keeps its sign
    # the branch Go leaves to Payne-Hanek is not restated: NaN from 2^29 on, for the infinities and for NaN
    out_of_range = np.array([LIM, -LIM, np.nextafter(LIM, np.inf), 1e10, -1e300, MAXF, np.inf, -np.inf, np.nan])
    assert np.all(np.isnan(dp.unary(dp.U_SIN, out_of_range)))
    # one reduction serves both: sin and cos of the non-negative arguments
    xp = np.abs(x)
    s, c = dp.sincos(xp)
    _check("sincos_pos sin", s, _ora1(ORA_SIN, xp), xp)
    _check("sincos_pos cos", c, _ora1(ORA_COS, xp), xp)


def test_go_tan_on_the_device_equals_the_oracle():
    rng = np.random.default_rng(71)
    half_pi = np.arange(0, 400) * (math.pi / 2)
    parts = [
        rng.uniform(0.0, math.pi / 2, 300_000),                                          # tan(fov / 2): the camera set-up
        rng.uniform(-LIM, LIM, 300_000),
        np.sign(rng.uniform(-1, 1, 300_000)) * np.exp2(rng.uniform(-60, 29, 300_000)),  # every binade
        rng.uniform(-3000.0, 3000.0, 150_000),                                           # every octant, -1/y in half of them
        # both sides of zz > 1e-14: |z| around 1e-7 next to the zeros and the poles
        np.concatenate([half_pi[:, None] + s * np.exp2(rng.uniform(-26, -20, (400, 40))) for s in (1.0, -1.0)]).ravel(),
        np.exp2(rng.uniform(-30, -18, 20_000)),
        sin_special_arguments(),
    ]
    x = np.concatenate(parts)
    x = x[np.abs(x) < LIM]
    assert x.size >= 1_000_000
    _check("go_tan", dp.unary(dp.U_TAN, x), _ora1(ORA_TAN, x), x)
    assert np.all(np.isnan(dp.unary(dp.U_TAN, np.array([LIM, -LIM, 1e300, np.inf, -np.inf, np.nan]))))


def test_go_exp_on_the_device_equals_the_oracle():
    rng = np.random.default_rng(72)
    over, under, near = 7.09782712893383973096e+02, -7.45133219101941108420e+02, 2.0 ** -28
    ln2 = math.log(2.0)
    parts = [
        rng.uniform(-746.0, 710.0, 600_000),
        np.sign(rng.uniform(-1, 1, 250_000)) * np.exp2(rng.uniform(-40, 9.5, 250_000)),  # every binade up to 724
        rng.uniform(-745.5, -707.0, 100_000),                                            # subnormal results
        rng.uniform(-0.5 * ln2, 0.5 * ln2, 50_000),                                      # k = 0
        rng.uniform(-40.0, 0.0, 100_000),                                                # -sigma_t * t of the march
        _around([over, under, near, -near, 0.5 * ln2, -0.5 * ln2, 1.5 * ln2, -1.5 * ln2, 709.0, -745.0, -708.0, -708.5, 1.0, -1.0]),
        (np.arange(-1075, 1025)[:, None] * ln2 + np.array([-1e-9, 0.0, 1e-9])).ravel(),  # the rounding of k, |k| large
        np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 710.0, 1000.0, -746.0, -1000.0, MAXF, -MAXF]),
    ]
    x = np.concatenate(parts)
    assert x.size >= 1_000_000
    got, want = dp.unary(dp.U_EXP, x), _ora1(ORA_EXP, x)
    _check("go_exp", got, want, x)
    sub = (want > 0) & (want < 2.2250738585072014e-308)
    assert np.count_nonzero(sub) > 10_000 and np.count_nonzero(want == np.inf) > 0 and np.count_nonzero(want == 0) > 0


def test_go_pow5_min_max_on_the_device_equal_the_oracle():
    rng = np.random.default_rng(73)
    x = np.concatenate([np.array([0.0, 1.0, np.nan, 2.0, 2.0 ** -53]), _around([1.0, 0.5, 2.0 ** -53], 3), np.exp2(rng.uniform(-53, 1, 200_000)),
                        rng.uniform(0.0, 2.0, 200_000)])
    x = x[~(x < 2.0 ** -53) | (x == 0)]  # go_pow5's domain: 0 or >= 2^-53 (what 1 - cos(theta) can be)
    _check("go_pow5", dp.unary(dp.U_POW5, x), _ora2(ORA_POW, x, np.full_like(x, 5.0)), x)
    v = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, MAXF, -MAXF, 2.2250738585072014e-308])
    a, b = [m.ravel() for m in np.meshgrid(v, v)]
    _check("go_min", dp.binary(dp.B_MIN, a, b), _ora2(ORA_MIN, a, b), a, b)
    _check("go_max", dp.binary(dp.B_MAX, a, b), _ora2(ORA_MAX, a, b), a, b)


def test_f_sqrt_on_the_device_is_correctly_rounded():
    rng = np.random.default_rng(74)
    k = rng.integers(1, 1 << 26, 50_000).astype(np.float64)
    sq = k * k  # exact squares below 2^52
    parts = [
        rng.integers(1, 0x7ff0000000000000, 1_000_000, dtype=np.uint64).view(np.float64),  # every positive binade, subnormals too
        np.exp2(rng.uniform(-770, -764, 100_000)),                                         # both sides of the short form's 2^-767
        _around([2.0 ** -767, 2.0 ** -766, 2.0 ** -768, 2.2250738585072014e-308, 1.0, 2.0, 4.0, np.nextafter(MAXF, 0.0, dtype=np.float64) * 0.99], 3),
        rng.integers(1, 1 << 52, 50_000, dtype=np.uint64).view(np.float64),                # subnormals
        sq, np.nextafter(sq, 0.0), np.nextafter(sq, np.inf),
        sq * 2.0 ** -600, np.nextafter(sq * 2.0 ** -600, 0.0), np.nextafter(sq * 2.0 ** -600, np.inf),
        np.array([0.0, -0.0, np.inf, MAXF, 5e-324, -5e-324, -1.0, -2.0 ** -767, -MAXF, -np.inf, np.nan]),
    ]
    x = np.concatenate(parts)
    assert np.count_nonzero(x > 0) >= 1_000_000
    with np.errstate(invalid="ignore"):
        want = np.sqrt(x)
    for which, name in ((dp.U_SQRT_OUTLINE, "f_sqrt<true>"), (dp.U_SQRT_INLINE, "f_sqrt<false>")):
        _check(name, dp.unary(which, x), want, x)


def test_sample_streams_on_the_device_equal_the_oracle():
    rng = np.random.default_rng(75)
    n, ndraw = 10_000, 64
    keys = np.stack([rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64),
                     rng.integers(0, 1 << 28, n, dtype=np.uint64), rng.integers(0, 1 << 31, n, dtype=np.uint64)], axis=1)
    keys[0] = (0, 0, 0)
    keys[1] = (2 ** 64 - 1, 2 ** 28 - 1, 2 ** 31 - 1)
    keys[2] = (1, 0, 2 ** 31 - 1)
    keys[3] = (1, 2 ** 28 - 1, 0)
    keys = np.ascontiguousarray(keys)
    s0, draws = dp.streams(keys, ndraw)
    r0, ref = np.zeros(n, np.uint64), np.zeros((n, ndraw))
    fs.reference().fr_ora_streams(fs.ptr(keys), ndraw, fs.ptr(r0), fs.ptr(ref), n)
    assert np.array_equal(s0, r0)
    _check("stream_next", draws, ref, keys)
    assert 0.0 <= draws.min() and draws.max() < 1.0 and np.unique(draws).size > n * ndraw * 0.999


# ---------------------------------------------------------------- pt_fog.h piece by piece

def _fog_points(rng, n):
    """Points whose hash argument (about 2000 |p|) runs from tiny to far beyond the 2^29 guard, and the non-finite ones."""
    p = rng.normal(size=(n, 3)) * np.exp2(rng.uniform(-12, 26, (n, 1)))
    p[:6] = [[np.inf, 0, 0], [0, -np.inf, 1], [np.nan, 1, 1], [0, 0, 0], [-0.0, -0.0, -0.0], [1e300, 1e300, 1e300]]
    return np.ascontiguousarray(p)


def test_hash_noise_and_phase_on_the_device_equal_host_build_and_restatement():
    rng = np.random.default_rng(76)
    n = 300_000
    p = np.concatenate([_fog_points(rng, n), rng.uniform(-12.0, 12.0, (n, 3))])  # and the positions a march visits
    m = p.shape[0]
    got = dp.hash31(p)
    host, ref = np.empty(m), np.empty(m)
    fs.product_host().shim_hash31_many(fs.ptr(p), fs.ptr(host), m)
    fs.reference().fr_hash31_many(fs.ptr(p), fs.ptr(ref), m)
    _check("hash31 vs restatement", got, ref, p)
    _check("hash31 vs host build", got, host, p)
    guarded = np.count_nonzero(ref == 0.5)
    assert m // 25 < guarded < m // 2 and np.all((ref >= 0) & (ref < 1))  # both sides of the guard
    for name in ("octaves_0", "octaves_1", "octaves_7", "noise_scale_0", "huge_noise_scale", "hetero_1.5"):
        fog = fs.fog_struct(**FOG_TABLE[name])
        got = dp.volume_noise(fog, p)
        fs.product_host().shim_noise_many(C.byref(fog), fs.ptr(p), fs.ptr(host), m)
        fs.reference().fr_noise_many(C.byref(fog), fs.ptr(p), fs.ptr(ref), m)
        _check("volume_noise %s vs restatement" % name, got, ref, p)
        _check("volume_noise %s vs host build" % name, got, host, p)
    g = np.concatenate([rng.uniform(-0.9, 0.9, n), np.repeat([0.9, -0.9, 0.0, 0.3], 1000)])
    ct = np.concatenate([rng.uniform(-1.0, 1.0, n), np.tile([1.0, -1.0, 0.0, np.nextafter(1.0, 0.0)], 1000)])
    got = dp.binary(dp.B_PHASE_HG, ct, g)
    host, ref = np.empty(g.size), np.empty(g.size)
    fs.product_host().shim_phase_many(fs.ptr(ct), fs.ptr(g), fs.ptr(host), g.size)
    fs.reference().fr_phase_many(fs.ptr(ct), fs.ptr(g), fs.ptr(ref), g.size)
    _check("phase_hg vs restatement", got, ref, ct, g)
    _check("phase_hg vs host build", got, host, ct, g)


# ---------------------------------------------------------------- the in-scatter term and the GL pass, per ray and per job

def _doc(name):
    with open(scene_path(name)) as f:
        return json.load(f)


def _check_terms(tag, scene_c, fog, depth, rays, keys):
    n = rays.shape[0]
    Lr, cr = np.zeros((n, 3)), np.zeros((n, 3), np.uint32)
    fs.reference().fr_inscatter_many(C.byref(scene_c), C.byref(fog), depth, n, fs.ptr(rays), fs.ptr(keys), fs.ptr(Lr), fs.ptr(cr))
    Ld, cd = dp.inscatter(scene_c, fog, depth, rays, keys)
    bad = np.flatnonzero(~_same(Ld, Lr).all(1) | (cd != cr).any(1))
    assert bad.size == 0, (tag, bad.size, rays[bad[:3]], keys[bad[:3]], Ld[bad[:3]], Lr[bad[:3]], cd[bad[:3]], cr[bad[:3]])
    return int(np.count_nonzero(np.any(Lr != 0, axis=1))), cr.sum(0).astype(np.int64)


def test_inscatter_term_on_the_device_equals_the_restatement(tmp_path):
    from oracle import ora

    t0 = time.time()
    total = nonzero = 0
    counts = np.zeros(3, np.int64)
    # the rays, keys and fog blocks of test_inscatter_term_matches_reference_bit_for_bit
    for scene_name in ("gpu_showcase", "test_scene"):
        oc = ora.Scene.load(scene_path(scene_name))
        rng = np.random.default_rng(11 if scene_name == "gpu_showcase" else 12)
        blocks = [("scene", fs.fog_of_scene(_doc(scene_name)["fog"]))] + [(k, fs.fog_struct(**v)) for k, v in sorted(FOG_TABLE.items())]
        per = 50_000 // len(blocks) + 1
        for name, fog in blocks:
            rays, keys = _rays(oc, per, rng, 8)
            nz, c = _check_terms((scene_name, name), oc.c, fog, 8, rays, keys)
            total, nonzero, counts = total + per, nonzero + nz, counts + c
    shipped = total
    # the generator's scenes: 1..150 objects, 0 / 1 / 8 / 9 / 12 lights, random fog blocks
    scenes = 24
    for i in range(scenes):
        case, sc, flat, oc, fog = fuzz_scene(i, tmp_path)
        rays, keys = _rays(oc, 600, np.random.default_rng([31, i]), 8)
        nz, c = _check_terms(("random", i), oc.c, fog, case["depth"], rays, keys)
        total, nonzero, counts = total + 600, nonzero + nz, counts + c
    print("fog_inscatter on the device: %d rays (%d on 2 shipped scenes x 16 fog blocks, %d on %d random scenes), %d non-zero "
          "terms, %d shadow rays, %d draws, %d march steps, all bit-equal to the restatement, %.0f s"
          % (total, shipped, total - shipped, scenes, nonzero, counts[0], counts[1], counts[2], time.time() - t0))
    assert scenes >= 20 and total >= 50_000
    assert nonzero > total // 4 and counts[0] > total and counts[2] > total  # the comparison is not over zeros


def _jobs(n, w, h, passes, seed):  # test_glshade_cpu._jobs
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, w, n), rng.integers(0, h, n), rng.integers(0, passes, n)], 1).astype(np.int32)


def _check_passes(tag, sc, flat, o, w, h, depth, seed, jobs, fog=None):
    ex = gs.extras(sc)
    a, ca = gs.ref_passes(o, ex, w, h, depth, seed, jobs, fog)
    b, cb = dp.passes(flat, ex, w, h, depth, seed, jobs, fog)
    bad = np.flatnonzero(~_same(b, a).all(1) | (ca != cb).any(1))
    assert bad.size == 0, (tag, bad.size, jobs[bad[:3]], a[bad[:3]], b[bad[:3]], ca[bad[:3]], cb[bad[:3]])
    return ca.sum(0)


def test_gl_pass_on_the_device_equals_the_restatement(tmp_path):
    from oracle import ora
    from path_trace_golang_amd import hip, scene
    from test_glshade_cpu import FUZZ_H, FUZZ_JOBS, FUZZ_PASSES, FUZZ_W, SEED, SHIPPED

    t0 = time.time()
    totals = np.zeros(8, np.uint64)
    n = with_fog = 0
    # the jobs of test_host_build_equals_restatement_on_the_shipped_scenes ...
    for name in SHIPPED:
        sc = scene.load(scene_path(name))
        flat, o = hip.FlatScene(sc), ora.Scene(_doc(name))
        fog = hip.pt_fog(sc.fog) if sc.fog is not None else None
        for depth, k in ((8, 9000), (3, 3000), (1, 3000)):
            totals += _check_passes((name, depth), sc, flat, o, 64, 36, depth, SEED, _jobs(k, 64, 36, 6, depth), fog)
            n, with_fog = n + k, with_fog + (k if fog is not None else 0)
        if name == "gpu_showcase":
            totals += _check_passes((name, 80, "fog"), sc, flat, o, 64, 36, 80, SEED, _jobs(1500, 64, 36, 4, 80), fog)
            totals += _check_passes((name, 80), sc, flat, o, 64, 36, 80, SEED, _jobs(1500, 64, 36, 4, 81))
            n, with_fog = n + 3000, with_fog + 1500
    # ... of test_host_build_equals_restatement_on_synthetic_scenes ...
    for name in ("twelve_lights", "edge", "glass", "metal"):
        sc, flat, o = gs.scene_pair(gs.synthetic_docs()[name], str(tmp_path), name)
        for depth, k in ((1, 2000), (3, 3000), (8, 5000), (80, 2000)):
            totals += _check_passes((name, depth), sc, flat, o, 48, 32, depth, SEED, _jobs(k, 48, 32, 5, depth + 7))
            n += k
    fixed = n
    # ... and the generator's scenes, half of them with their fog block
    scenes = 24
    for i in range(scenes):
        case, sc, flat, o, fog = fuzz_scene(i, tmp_path)
        jobs = _jobs(FUZZ_JOBS, FUZZ_W, FUZZ_H, FUZZ_PASSES, 500 + i)
        totals += _check_passes(("random", i), sc, flat, o, FUZZ_W, FUZZ_H, case["depth"], SEED, jobs, fog if case["fog"] else None)
        n, with_fog = n + FUZZ_JOBS, with_fog + (FUZZ_JOBS if case["fog"] else 0)
    print("gl_pass on the device: %d jobs (%d on 9 fixed scenes, %d on %d random scenes; %d with a fog block), %d paths, %d segments, "
          "%d shadow rays, %d probe rays, %d draws, %d fog shadow rays, %d fog steps, all bit-equal to the restatement, %.0f s"
          % (n, fixed, n - fixed, scenes, with_fog, totals[0], totals[1], totals[2], totals[3], totals[4], totals[5], totals[7],
             time.time() - t0))
    assert scenes >= 20 and n >= 30_000 and 0 < with_fog < n
    assert totals[0] == 16 * n and totals[1] > totals[0] and totals[2] > 0 and totals[3] > 0 and totals[5] > 0 and totals[7] > 0
