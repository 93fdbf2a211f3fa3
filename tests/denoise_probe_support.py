"""Builds and loads tests/denoise_probe.hip: the kernels of the a-trous filter, of the pair filter and of the temporal accumulation
(csrc/pt_kernels.h) launched on frames no renderer made (test_denoise_probe_cpu.py compiles it anywhere and
checks the inputs below on the CPU; test_denoise_probe_gpu.py runs it).

The probe is compiled with the library's compiler and exactly its flags (path_trace_golang_amd.build.HIPCC, HIP_FLAGS), into a
temporary directory, never into the tree.  Also here, so that they can be checked without a device: the inputs of the GPU tests --
frames of sums with every special value placed where the kernels' blocks, waves and taps meet, and a synthetic world of one or two
walls seen by look-at cameras for the temporal sequences -- the list of cases, and a NumPy classification of the history taps of a
frame.  The reference of every GPU comparison is the C restatement (atrous_reference.c, temporal_reference.c), never the host build
of the header under test."""
from __future__ import annotations

import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np

import atrous_support as at
import halves_support as hv
import temporal_support as ts
from fog_support import CSRC, ROOT, ptr

SOURCE = os.path.join(ROOT, "tests", "denoise_probe.hip")
SYMBOLS = ("probe_filter", "probe_pair", "probe_temporal_new", "probe_temporal_free", "probe_temporal_reset", "probe_temporal_read",
           "probe_temporal_frame")
KERNELS = ("atrous_prep_kernel", "atrous_noise_kernel", "atrous_kernel", "atrous_finish_kernel", "atrous_pair_prep_kernel",
           "atrous_pair_kernel", "halves_combine_kernel", "temporal_kernel")

_dir = None
_lib = None


def compile_probe() -> str:
    """Path of the probe's shared library (built once per process)."""
    global _dir
    from path_trace_golang_amd import build

    if _dir is None:
        _dir = tempfile.mkdtemp(prefix="dnprobe_")
    out = os.path.join(_dir, "libdenoiseprobe.so")
    if not os.path.exists(out):
        r = subprocess.run([build.HIPCC, *build.HIP_FLAGS, "-shared", "-I", CSRC, SOURCE, "-o", out], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("denoise probe does not compile:\n%s\n%s" % (r.stdout, r.stderr))
    return out


def load():
    """The probe, loaded after torch so that the process keeps one HIP runtime (as conftest.gpu_ctx does for libptcore.so)."""
    global _lib
    if _lib is None:
        import torch  # noqa: F401

        L = C.CDLL(compile_probe())
        vp = C.c_void_p
        L.probe_filter.argtypes = at._FILTER_ARGS
        L.probe_pair.argtypes = [C.c_int32, C.c_int32, vp, vp, vp, vp, vp, C.c_uint32, vp, vp, vp, C.c_int32, vp, vp, vp, vp, vp, vp]
        L.probe_temporal_new.restype = vp
        L.probe_temporal_new.argtypes = []
        L.probe_temporal_free.argtypes = [vp]
        L.probe_temporal_free.restype = None
        L.probe_temporal_reset.argtypes = [vp]
        L.probe_temporal_reset.restype = None
        L.probe_temporal_read.argtypes = [vp, vp, vp, vp, vp]
        L.probe_temporal_frame.argtypes = ts._FRAME_ARGS
        for s in ("probe_filter", "probe_pair", "probe_temporal_read", "probe_temporal_frame"):
            getattr(L, s).restype = C.c_int
        _lib = L
    return _lib


def _ok(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError("%s: status %d" % (what, rc))


# ---------------------------------------------------------------- the three entry points as the host builds' callers see them
def gpu_filter(S, Q, n, counts=None, feats=None, **cfg) -> dict:
    """probe_filter: the dict of atrous_support.host_filter."""
    L = load()
    return at._filter(lambda *a: _ok(L.probe_filter(*a), "probe_filter"), S, Q, n, counts, feats, **cfg)


def gpu_pair(SA, QA, SB, QB, n, counts=None, feats=None, **cfg) -> dict:
    """probe_pair: the dict of halves_support.host_pair."""
    c = dict(at.DEFAULTS, **cfg)
    a = [np.ascontiguousarray(x, np.float64) for x in (SA, QA, SB, QB)]
    H, W = a[0].shape[:2]
    cnt = np.ascontiguousarray(counts, np.uint32) if counts is not None else None
    f = [np.ascontiguousarray(x, np.float64) for x in feats] if feats is not None else [None] * 3
    sig = np.array([c["sigma_l"], c["sigma_n"], c["sigma_z"], c["sigma_a"]], np.float64)
    mean, err, hm, noise = np.zeros((H, W, 3)), np.zeros((H, W)), np.zeros((2, H, W, 3)), np.zeros(2)
    bad = C.c_uint64(0)
    p = lambda x: ptr(x) if x is not None else None
    _ok(load().probe_pair(W, H, *(ptr(x) for x in a), p(cnt), int(n), p(f[0]), p(f[1]), p(f[2]), int(c["iterations"]), ptr(sig), ptr(mean),
                          ptr(err), ptr(hm), ptr(noise), C.byref(bad)), "probe_pair")
    return dict(mean=mean, err=err, half_means=hm, noise=float(noise[0]), noise_model=float(noise[1]), bad_pixels=bad.value)


class GpuAccumulator(ts.Accumulator):
    """temporal_support.Accumulator on the probe's device history (kind "gpu"): the same frame / read / reset / close."""

    def __init__(self):
        L = load()
        self.kind = "gpu"
        self._new, self._free, self._reset = L.probe_temporal_new, L.probe_temporal_free, L.probe_temporal_reset
        self._frame = lambda *a: _ok(L.probe_temporal_frame(*a), "probe_temporal_frame")
        self._read = L.probe_temporal_read
        self.h = self._new()

    def read(self, w: int, h: int):
        mean, var, ln = np.zeros((h, w, 3)), np.zeros((h, w)), np.zeros((h, w), np.int32)
        valid = C.c_int32(-1)
        _ok(self._read(self.h, ptr(mean), ptr(var), ptr(ln), C.byref(valid)), "probe_temporal_read")
        return (mean, var, ln) if valid.value else None


def accumulator(kind: str):
    return GpuAccumulator() if kind == "gpu" else ts.Accumulator(kind)


# ---------------------------------------------------------------- filter inputs
def random_inputs(w, h, seed):
    """Sums of a frame with every special case the model names: counts 2..64, pixels with var = 0, with Q/n < c^2, with NaN and
    infinite sums, pixels whose feature samples all missed (h = 0), smooth regions and edges in every guide."""
    r = np.random.default_rng(seed)
    n = r.integers(2, 65, (h, w)).astype(np.uint32)
    base = np.where(np.arange(w)[None, :, None] < w // 2, 0.2, 1.5) + 0.3 * r.random((h, w, 3))
    mean = base * (1 + 0.4 * r.standard_normal((h, w, 3)))
    S = mean * n[..., None]
    Q = (mean * mean + (0.5 * base * r.random((h, w, 3))) ** 2 * n[..., None]) * n[..., None]
    S[1, 2] = 0.0; Q[1, 2] = 0.0                      # var = 0 exactly, l = 0
    S[3, 5] = 3.0 * n[3, 5]; Q[3, 5] = 9.0 * n[3, 5]  # var = 0 exactly
    Q[4, 7] = 0.0; Q[h - 1, w - 1] = 0.0              # Q/n < c^2: counts as 0
    S[6, 9, 1] = np.nan
    S[7, 11, 0] = np.inf
    Q[8, 13, 2] = np.inf                              # var infinite, mean finite
    Q[0, 0, 0] = np.nan
    S[h - 2, w - 3, 2] = -np.inf
    k = 4.0
    hits = r.integers(0, 5, (h, w)).astype(np.float64)
    hits[2, 2] = 0; hits[5, 20] = 0
    nrm = r.standard_normal((h, w, 3))
    nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
    nrm[:, : w // 3] = (0.0, 1.0, 0.0)
    fn = nrm * hits[..., None]
    fa = np.where(np.arange(h)[:, None, None] < h // 2, 0.8, 0.1) * r.random((h, w, 3)) * hits[..., None]
    fd = np.stack([hits * (2.0 + 5.0 * r.random((h, w))), hits, np.full((h, w), k)], axis=2)
    return S, Q, n, (fn, fa, fd)


# the configurations of test_atrous_cpu.py; the probe's cases use [0], [4] (every feature term off) and [5] (wide sigmas)
CONFIGS = [dict(), dict(sigma_n=0.0), dict(sigma_z=0.0), dict(sigma_a=0.0), dict(sigma_n=0.0, sigma_z=0.0, sigma_a=0.0),
           dict(sigma_l=0.5, sigma_n=2.0, sigma_z=1.0, sigma_a=5.0)]

BAD_KINDS = ("nan_S", "posinf_S", "neginf_S", "inf_Q", "nan_Q")           # the pixel is bad
GOOD_KINDS = ("var0_black", "var0", "Q0", "Q0", "h0", "h0")               # var = 0 with l = 0, var = 0, Q/n < c^2, no feature sample hit


def special_places(w, h, seed):
    """[(kind, (y, x))]: where special_inputs plants its specials, by rule.  The five bad kinds go on (0, 0), on the last pixel, next to
    a corner of the kernels' 32 x 8 blocks (column 32 or 31, row 7, where the shape has them), on linear index 256 or 255 (the first
    or last lane of a 256-thread block) and on the middle pixel; the good kinds next to the middle pixel (inside its 5 x 5 taps of
    step 1), on (8, 31), on linear index 255, on the two other corners, and at seeded places.  A place taken twice is replaced by a
    seeded free one.  A frame of fewer than eleven pixels gets as many as fit."""
    r = np.random.default_rng(1000003 * seed + 7919 * w + h)
    npix = w * h
    lin = lambda i: (i // w, i % w)
    xe = 32 if w > 32 else (31 if w == 32 else w // 2)
    ye = 7 if h >= 8 else h // 2
    yi, xi = h // 2, w // 2
    rule = [(0, 0), (h - 1, w - 1), (ye, xe), lin(256) if npix > 256 else lin(255) if npix > 255 else lin(npix // 3), (yi, xi)]
    rule.append((yi - 1 if yi >= 1 else yi + 1, xi + 2 if xi + 2 < w else max(xi - 1, 0)))
    if h > 8 and w >= 32:
        rule.append((8, 31))
    if npix > 256:
        rule.append(lin(255))
    rule += [(0, w - 1), (h - 1, 0)]
    kinds = BAD_KINDS + GOOD_KINDS
    free = [lin(int(i)) for i in r.permutation(npix)]
    taken, out = set(), []
    for k, kind in enumerate(kinds[:npix]):
        p = rule[k] if k < len(rule) and rule[k] not in taken else next(q for q in free if q not in taken and q not in rule)
        taken.add(p)
        out.append((kind, (int(p[0]), int(p[1]))))
    return out


def _noisy_sums(r, base, n):
    """(S, Q) around `base` [h, w, 3] for the counts n [h, w]: the recipe of random_inputs."""
    nn = n.astype(np.float64)[..., None]
    mean = base * (1 + 0.4 * r.standard_normal(base.shape))
    return mean * nn, (mean * mean + (0.5 * base * r.random(base.shape)) ** 2 * nn) * nn


def _plant(S, Q, n, kind, y, x):
    if kind == "nan_S":
        S[y, x, 1] = np.nan
    elif kind == "posinf_S":
        S[y, x, 0] = np.inf
    elif kind == "neginf_S":
        S[y, x, 2] = -np.inf
    elif kind == "inf_Q":
        Q[y, x, 2] = np.inf   # var infinite, mean finite
    elif kind == "nan_Q":
        Q[y, x, 0] = np.nan
    elif kind == "var0_black":
        S[y, x] = 0.0; Q[y, x] = 0.0
    elif kind == "var0":
        S[y, x] = 3.0 * n[y, x]; Q[y, x] = 9.0 * n[y, x]
    elif kind == "Q0":
        Q[y, x] = 0.0


def _base(r, w, h):
    return np.where(np.arange(w)[None, :, None] < w // 2, 0.2, 1.5) + 0.3 * r.random((h, w, 3))


def _features(r, w, h, places):
    hits = r.integers(0, 5, (h, w)).astype(np.float64)
    for kind, (y, x) in places:
        if kind == "h0":
            hits[y, x] = 0
        elif hits[y, x] == 0:
            hits[y, x] = 2  # the other specials keep a guide
    nrm = r.standard_normal((h, w, 3))
    nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
    nrm[:, : max(w // 3, 1)] = (0.0, 1.0, 0.0)
    fn = nrm * hits[..., None]
    fa = np.where(np.arange(h)[:, None, None] < h // 2, 0.8, 0.1) * r.random((h, w, 3)) * hits[..., None]
    fd = np.stack([hits * (2.0 + 5.0 * r.random((h, w))), hits, np.full((h, w), 4.0)], axis=2)
    return fn, fa, fd


def special_inputs(w, h, seed):
    """random_inputs for any w, h >= 2, the specials at special_places: (S, Q, n, feats, places)."""
    assert w >= 2 and h >= 2
    r = np.random.default_rng(seed)
    places = special_places(w, h, seed)
    n = r.integers(2, 65, (h, w)).astype(np.uint32)
    S, Q = _noisy_sums(r, _base(r, w, h), n)
    for kind, (y, x) in places:
        _plant(S, Q, n, kind, y, x)
    return S, Q, n, _features(r, w, h, places), places


def special_pair_inputs(w, h, seed):
    """The four half sums with counts 4..64 and the places of special_inputs: (SA, QA, SB, QB, n, feats, info).  The good specials are in
    both halves; of the five bad places the first and the last are bad in both halves, the second and the fourth in half B only, the
    third in half A only.  info = dict(both, a_only, b_only: lists of (y, x))."""
    assert w >= 2 and h >= 2
    r = np.random.default_rng(seed + 1)
    places = special_places(w, h, seed)
    n = r.integers(4, 65, (h, w)).astype(np.uint32)
    nA, nB = (n + 1) // 2, n // 2
    base = _base(r, w, h)
    SA, QA = _noisy_sums(r, base, nA)
    SB, QB = _noisy_sums(r, base, nB)
    info = dict(both=[], a_only=[], b_only=[])
    k = 0
    for kind, (y, x) in places:
        if kind in BAD_KINDS:
            where = ("both", "b_only", "a_only", "b_only", "both")[k]
            if where != "b_only":
                _plant(SA, QA, nA, kind, y, x)
            if where != "a_only":
                _plant(SB, QB, nB, BAD_KINDS[(k + 2) % 5], y, x)  # another kind than half A's
            info[where].append((y, x))
            k += 1
        else:
            _plant(SA, QA, nA, kind, y, x)
            _plant(SB, QB, nB, kind, y, x)
    return SA, QA, SB, QB, n, _features(r, w, h, places), info


SHAPES = ((37, 21), (97, 71), (130, 2), (2, 130), (33, 9), (64, 16))
ALL_ITERATIONS = ((37, 21), (97, 71))  # iterations 0, 1, 5, 6; the other shapes run 6 only
UNIFORM_N = 9                          # the count of the runs without per-pixel counts (halves: nA = 5, nB = 4)


def filter_cases(w, h):
    """[(T, config index, per-pixel counts?, features?)] of one shape: CONFIGS[0], [4] and [5], with and without features, with the
    per-pixel counts and with n = 9.  Pruned like test_host_build_equals_the_restatement_on_random_inputs -- the wide-sigma
    configuration only with features -- except that it runs at 5 and 6 iterations, not at 0 and 1: at 0 no configuration is read,
    and its wide sigmas are there for the taps of steps 16 and 32."""
    out = []
    for T in ((0, 1, 5, 6) if (w, h) in ALL_ITERATIONS else (6,)):
        for i in (0, 4, 5):
            if i == 5 and T in (0, 1):
                continue
            for per_pixel in (True, False):
                for with_feats in (True, False):
                    if i == 5 and not with_feats:
                        continue
                    out.append((T, i, per_pixel, with_feats))
    return out


_inputs = {}
_ref = {}


def shape_inputs(w, h, pair=False):
    key = (w, h, pair)
    if key not in _inputs:
        _inputs[key] = (special_pair_inputs if pair else special_inputs)(w, h, 7 * w + h)
    return _inputs[key]


def run_filter_case(kind, w, h, case, pair=False):
    """One case of filter_cases through `kind`: "ref" (the restatement; computed once per process), "host" or "gpu"."""
    T, i, per_pixel, with_feats = case
    key = (w, h, case, pair)
    if kind == "ref" and key in _ref:
        return _ref[key]
    inp = shape_inputs(w, h, pair)
    sums, n, feats = inp[:-3], inp[-3], inp[-2]
    fn = {("ref", False): at.ref_filter, ("host", False): at.host_filter, ("gpu", False): gpu_filter,
          ("ref", True): hv.ref_pair, ("host", True): hv.host_pair, ("gpu", True): gpu_pair}[(kind, pair)]
    out = fn(*sums, UNIFORM_N, n if per_pixel else None, feats if with_feats else None, iterations=T, **CONFIGS[i])
    if kind == "ref":
        _ref[key] = out
    return out


def planted_bad(w, h) -> int:
    return sum(1 for kind, _ in special_places(w, h, 7 * w + h) if kind in BAD_KINDS)


# ---------------------------------------------------------------- the synthetic world of the temporal sequences
def _unit(v):
    v = np.asarray(v, np.float64)
    return v / math.sqrt(float(v @ v))


def look_at(pos, target, up, vfov, w, h):
    """The 22 doubles of ora_camera_setup for a pinhole camera at `pos` looking at `target`: origin, lower_left, horizontal, vertical,
    u, v, w, lens radius 0; the image plane at distance 1."""
    pos, target = np.asarray(pos, np.float64), np.asarray(target, np.float64)
    half_h = math.tan(math.radians(vfov) / 2.0)
    half_w = half_h * w / h
    ww = _unit(pos - target)
    u = _unit(np.cross(np.asarray(up, np.float64), ww))
    v = np.cross(ww, u)
    ll = pos - half_w * u - half_h * v - ww
    return np.concatenate([pos, ll, 2.0 * half_w * u, 2.0 * half_h * v, u, v, ww, [0.0]])


WALL_X, WALL_Y = 3.0, 2.0             # the first wall: z = 0, |x| <= 3, |y| <= 2
WALL2 = (1.5, -0.2, 1.4, -1.2, 0.6)   # the second: z, x from .. to, y from .. to -- nearer to a camera on the +z side
CELL, STRIPE = 0.5, 0.7
TILT = (0.6, 0.0, 0.8)                # the tilted normal: 0.8 against (0, 0, 1), below the default n_min of 0.9
LIGHT = _unit((0.3, 0.5, 0.8))


def centre_rays(cam, w, h):
    """d [h, w, 3] of pt_temporal.h step 3, in its order of evaluation."""
    org, ll, hor, ver = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    x, y = np.arange(w, dtype=np.float64)[None, :, None], np.arange(h, dtype=np.float64)[:, None, None]
    u = (x + 0.5) * (1.0 / float(w - 1))
    v = ((float(h - 1) - y) + 0.5) * (1.0 / float(h - 1))
    return ((ll + hor * u) + ver * v) - org


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def wall_frame(cam, w, h, seed, n=8, second_wall=False, bad_seed=None):
    """A frame of the world as `cam` sees it: dict(S, Q, n, feats, cam, bad) like temporal_support.oracle_frame.  A checker wall at
    z = 0 whose normals are tilted in every third horizontal stripe, optionally a second, nearer wall with the same pattern, the sky
    where a centre ray leaves both; k = 4 feature sums with 1..4 of the samples hitting; S and Q noisy around the analytic radiance;
    three bad pixels (a NaN sum, an infinite sum, a NaN square sum) at places seeded by bad_seed (default: seed)."""
    cam = np.ascontiguousarray(cam, np.float64)
    r = np.random.default_rng(seed)
    d = centre_rays(cam, w, h)
    o = cam[0:3]
    t = np.full((h, w), np.inf)
    with np.errstate(all="ignore"):
        walls = [(0.0, -WALL_X, WALL_X, -WALL_Y, WALL_Y)] + ([WALL2] if second_wall else [])
        for wz, x0, x1, y0, y1 in walls:
            tt = (wz - o[2]) / d[..., 2]
            px, py = o[0] + d[..., 0] * tt, o[1] + d[..., 1] * tt
            ok = (tt > 1e-9) & (px >= x0) & (px <= x1) & (py >= y0) & (py <= y1) & (tt < t)
            t = np.where(ok, tt, t)
    hit = np.isfinite(t)
    ts_ = np.where(hit, t, 0.0)
    px, py = o[0] + d[..., 0] * ts_, o[1] + d[..., 1] * ts_
    dlen = np.sqrt(_dot(d, d))
    z = ts_ * dlen
    side = np.where(d[..., 2] < 0, 1.0, -1.0)[..., None]   # face forward
    tilted = (np.floor((py + 10.0) / STRIPE) % 3 == 0)[..., None]
    N = np.where(tilted, np.array(TILT), np.array((0.0, 0.0, 1.0))) * side
    light = np.abs(_dot(N, LIGHT[None, None]))[..., None]
    odd = ((np.floor((px + 10.0) / CELL) + np.floor((py + 10.0) / CELL)) % 2 == 1)[..., None]
    A = np.where(odd, np.array((0.8, 0.7, 0.6)), np.array((0.2, 0.3, 0.4)))
    sky = np.array((0.4, 0.6, 0.9)) * (0.5 + 0.5 * (d[..., 1] / dlen))[..., None] + 0.1
    L = np.where(hit[..., None], A * (0.25 + 0.75 * light), sky)
    mean = L * (1 + 0.15 * r.standard_normal((h, w, 3)))
    S = mean * n
    Q = (mean * mean + (0.4 * L * r.random((h, w, 3))) ** 2 * n) * n
    hits = np.where(hit, r.integers(1, 5, (h, w)), 0).astype(np.float64)
    fn = np.where(hit[..., None], N, 0.0) * hits[..., None]
    fa = np.where(hit[..., None], A, 0.0) * hits[..., None]
    fd = np.stack([z * hits, hits, np.full((h, w), 4.0)], axis=2)
    rb = np.random.default_rng(977 + (seed if bad_seed is None else bad_seed))
    bad = [(int(i) // w, int(i) % w) for i in rb.choice(w * h, 3, replace=False)]
    S[bad[0][0], bad[0][1], 1] = np.nan
    S[bad[1][0], bad[1][1], 0] = np.inf
    Q[bad[2][0], bad[2][1], 2] = np.nan
    return dict(S=S, Q=Q, n=n, feats=(fn, fa, fd), cam=cam, bad=bad, w=w, h=h)


POS, TARGET, UP, FOV = np.array((0.3, 0.2, 5.0)), np.array((0.1, 0.0, 0.0)), (0.0, 1.0, 0.0), 60.0


def _rot_y(v, deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return np.array((c * v[0] + s * v[2], v[1], -s * v[0] + c * v[2]))


def _sideways(w, h, up, frames=8, step=0.02):
    fwd = TARGET - POS
    right = _unit(np.cross(fwd, np.asarray(up, np.float64)))
    dist = math.sqrt(float(fwd @ fwd))
    return [wall_frame(look_at(POS + right * (f * step * dist), TARGET, up, FOV, w, h), w, h, 100 + f, second_wall=True) for f in range(frames)]


def _make_sequence(name):
    w, h = 70, 37
    if name == "unmoved":  # the bad pixels stay where they are for four frames, then move: all reprojected, then a few taps on len_h = 0
        cam = look_at(POS, TARGET, UP, FOV, w, h)
        return [wall_frame(cam, w, h, 200 + f, bad_seed=0 if f < 4 else f) for f in range(8)]
    if name == "sideways":
        return _sideways(w, h, UP)
    if name == "sideways, up = x":
        return _sideways(w, h, (1.0, 0.0, 0.0))
    if name == "sideways 33 x 9":
        return _sideways(33, 9, UP)
    if name == "sideways 97 x 71":
        return _sideways(97, 71, UP)
    if name == "rotation":  # 4 degrees per frame about the vertical through the camera
        return [wall_frame(look_at(POS, POS + _rot_y(TARGET - POS, 4.0 * f), UP, FOV, w, h), w, h, 300 + f) for f in range(8)]
    if name == "dolly":  # 8 % nearer per frame
        return [wall_frame(look_at(TARGET + (POS - TARGET) * 0.92 ** f, TARGET, UP, FOV, w, h), w, h, 400 + f) for f in range(6)]
    if name == "field of view":  # 60 -> 25 degrees
        return [wall_frame(look_at(POS, TARGET, UP, 60.0 - 7.0 * f, w, h), w, h, 500 + f) for f in range(6)]
    if name == "turn":  # 180 degrees every frame
        return [wall_frame(look_at(POS, TARGET if f % 2 == 0 else POS + (POS - TARGET), UP, FOV, w, h), w, h, 600 + f) for f in range(4)]
    if name == "through the wall":  # the camera keeps looking at the wall's middle and ends behind it
        return [wall_frame(look_at(np.array((0.3, 0.2, z)), TARGET, UP, FOV, w, h), w, h, 700 + f) for f, z in enumerate((5.0, 3.0, 1.0, -1.0, -3.0))]
    if name == "jump":  # sideways by three frame widths at the wall, and back; camera and target move together
        cam0 = look_at(POS, TARGET, UP, FOV, w, h)
        jump = 3.0 * math.sqrt(float(cam0[6:9] @ cam0[6:9])) * 5.0 * _unit(cam0[6:9])
        return [wall_frame(look_at(POS + jump * (f % 2), TARGET + jump * (f % 2), UP, FOV, w, h), w, h, 800 + f) for f in range(5)]
    if name == "edge":  # straight at the wall from 2 away (it fills the frame), moved by 0.995 pixel per frame: to the right twice, then back
        pos, tgt = np.array((0.0, 0.0, 2.0)), np.zeros(3)
        cam0 = look_at(pos, tgt, UP, FOV, w, h)
        pitch = math.sqrt(float(cam0[6:9] @ cam0[6:9])) * 2.0 / (w - 1)
        out = []
        for f, k in enumerate((0, 1, 2, 1, 0)):
            sh = np.array((0.995 * pitch * k, 0.0, 0.0))
            out.append(wall_frame(look_at(pos + sh, tgt + sh, UP, FOV, w, h), w, h, 900 + f))
        return out
    if name == "resize":  # 70 x 37 -> 33 x 9 -> 70 x 37, and one reset
        out = []
        for f, (ww, hh) in enumerate(((70, 37), (70, 37), (33, 9), (33, 9), (70, 37), (70, 37), (70, 37), (70, 37))):
            fr = wall_frame(look_at(POS + np.array((0.03 * f, 0.0, 0.0)), TARGET, UP, FOV, ww, hh), ww, hh, 1000 + f, second_wall=True)
            fr["reset"] = f == 6
            out.append(fr)
        return out
    raise KeyError(name)


SEQUENCES = ("unmoved", "sideways", "sideways, up = x", "sideways 33 x 9", "sideways 97 x 71", "rotation", "dolly", "field of view", "turn",
             "through the wall", "jump", "edge", "resize")
TCONFIGS = (dict(), dict(alpha=0.5, max_len=3), dict(alpha=0.0, **ts.OPEN), dict(alpha=1.0), dict(tol_z=0.0, tol_a=0.0, n_min=1.0))
FILTERS = (dict(iterations=3), None, dict(iterations=0), dict(iterations=6))
_seq = {}


def sequence(name):
    """The frames of a sequence (made once)."""
    if name not in _seq:
        _seq[name] = _make_sequence(name)
    return _seq[name]


def run_frames(kind, frames, filter=None, **tcfg):
    """Every frame through one accumulator of `kind` ("ref", "host" or "gpu"); a frame with reset = True resets it first.  Returns
    (results, the history read after the last frame)."""
    acc = accumulator(kind)
    try:
        out = []
        for f in frames:
            if f.get("reset"):
                acc.reset()
                assert acc.read(f["w"], f["h"]) is None
            out.append(acc.frame(f["S"], f["Q"], f["n"], f["feats"], f["cam"], None, filter, **tcfg))
        return out, acc.read(frames[-1]["w"], frames[-1]["h"])
    finally:
        acc.close()


def has_history(frames, k) -> bool:
    """Whether frame k of the sequence finds a history: not the first, not after a reset, not at another size."""
    return k > 0 and not frames[k].get("reset") and (frames[k]["w"], frames[k]["h"]) == (frames[k - 1]["w"], frames[k - 1]["h"])


# ---------------------------------------------------------------- what the history taps of a frame did
REASONS = ("outside", "len", "hit", "weight", "tol_z", "n_min", "tol_a")


def _guides(fr):
    fn, fa, fd = fr["feats"]
    hh = fd[..., 1]
    den = np.where(hh != 0, hh, 1.0)[..., None]
    on = (hh != 0)[..., None]
    return np.where(on, fn / den, 0.0), np.where(on, fa / den, 0.0), np.where(hh != 0, fd[..., 0] / den[..., 0], 0.0), hh > 0


def classify(prev, cur, res_prev, res_cur, **tcfg):
    """The taps of frame `cur` on the history frame `prev` left, from the restatement's results alone: its `place` (fx, fy) of `cur`
    and its stored len of `prev`; the guide planes and zexp are prepped here as pt_temporal.h writes them.  Returns counts: the taps
    rejected first by each of REASONS (in the kernel's order of tests) and, for the three tolerances, those that fail nothing else
    ("sole tol_z", ...); pixels with 0 < sw <= 0.01; with x0 = -1, y0 = -1, x0 = W - 1, y0 = H - 1; reprojected pixels, those whose
    len' the clamp cut, and those with alpha > 1 / (L + 1) and with alpha <= 1 / (L + 1)."""
    c = dict(ts.T_DEFAULTS, **tcfg)
    w, h = cur["w"], cur["h"]
    cam, camh = cur["cam"], prev["cam"]
    Ni, Ai, zi, hiti = _guides(cur)
    Nh, Ah, zh, hith = _guides(prev)
    lenh = res_prev["hist_len"]
    fx, fy = res_cur["place"][..., 0], res_cur["place"][..., 1]
    found = np.isfinite(fx) & np.isfinite(fy)
    d = centre_rays(cam, w, h)
    with np.errstate(all="ignore"):
        s = zi / np.sqrt(_dot(d, d))
        q = (cam[0:3] + d * s[..., None]) - camh[0:3]
        zexp = np.where(hiti, np.sqrt(_dot(q, q)), 0.0)
    fx0, fy0 = np.where(found, fx, 0.0), np.where(found, fy, 0.0)
    x0, y0 = np.floor(fx0).astype(np.int64), np.floor(fy0).astype(np.int64)
    ax, ay = fx0 - x0, fy0 - y0
    out = {k: 0 for k in REASONS}
    out.update({"sole " + k: 0 for k in REASONS[4:]})
    sw = np.zeros((h, w))
    L = np.full((h, w), 2 ** 31 - 1, np.int64)
    for dy in (0, 1):
        for dx in (0, 1):
            xj, yj = x0 + dx, y0 + dy
            inside = (xj >= 0) & (xj < w) & (yj >= 0) & (yj < h)
            xc, yc = np.clip(xj, 0, w - 1), np.clip(yj, 0, h - 1)
            wt = (ax if dx else 1.0 - ax) * (ay if dy else 1.0 - ay)
            lok = lenh[yc, xc] > 0
            hok = hith[yc, xc] == hiti
            wok = wt > 0.0
            with np.errstate(all="ignore"):
                zok = ~hiti | (np.abs(zh[yc, xc] - zexp) <= c["tol_z"] * zexp)
                nok = ~hiti | (_dot(Ni, Nh[yc, xc]) >= c["n_min"])
                da = Ai - Ah[yc, xc]
                aok = ~hiti | ((da[..., 0] * da[..., 0] + da[..., 1] * da[..., 1]) + da[..., 2] * da[..., 2] <= c["tol_a"] * c["tol_a"])
            tests = (inside, lok, hok, wok, zok, nok, aok)
            alive = found.copy()
            for name, t in zip(REASONS, tests):
                out[name] += int(np.count_nonzero(alive & ~t))
                alive &= t
            pre = found & inside & lok & hok & wok
            out["sole tol_z"] += int(np.count_nonzero(pre & ~zok & nok & aok))
            out["sole n_min"] += int(np.count_nonzero(pre & zok & ~nok & aok))
            out["sole tol_a"] += int(np.count_nonzero(pre & zok & nok & ~aok))
            sw = sw + np.where(alive, wt, 0.0)
            L = np.where(alive, np.minimum(L, lenh[yc, xc]), L)
    rep = found & (sw > 0.01)
    out["small sw"] = int(np.count_nonzero(found & (sw > 0.0) & ~rep))
    out["x0 = -1"] = int(np.count_nonzero(found & (x0 == -1)))
    out["y0 = -1"] = int(np.count_nonzero(found & (y0 == -1)))
    out["x0 = W - 1"] = int(np.count_nonzero(found & (x0 == w - 1)))
    out["y0 = H - 1"] = int(np.count_nonzero(found & (y0 == h - 1)))
    out["reprojected"] = int(np.count_nonzero(rep))
    out["clamped"] = int(np.count_nonzero(rep & (L + 1 > c["max_len"])))
    r = 1.0 / (L + 1.0)
    out["alpha above"] = int(np.count_nonzero(rep & (c["alpha"] > r)))
    out["alpha not above"] = int(np.count_nonzero(rep & ~(c["alpha"] > r)))
    return out


def step32_taps(w, h, case):
    """How many (good pixel, diagonal tap at step 32) pairs of a 6-iteration case enter the sum with a weight that matters: the tap is
    in the frame, both pixels are good and pen <= 30 (the issue's bound is PTA_PEN_CUT = 745.2; a weight of e^-30 still moves the
    last bits of the sums, one of e^-700 does not).  From the restatement's state after five iterations.  At step 32 every tap with
    dx != 0 and dy != 0 lies in another block column (32 wide) and another block row (8 high)."""
    T, i, per_pixel, with_feats = case
    assert T == 6
    S, Q, n, feats, _ = shape_inputs(w, h)
    cfg = dict(at.DEFAULTS, **CONFIGS[i])
    st = at.ref_filter(S, Q, UNIFORM_N, n if per_pixel else None, feats if with_feats else None, iterations=5, **CONFIGS[i])
    c, var = st["mean"], st["var"]
    good = np.isfinite(c).all(axis=2) & np.isfinite(var)
    fr = dict(feats=feats)
    N, A, z, _ = _guides(fr) if with_feats else (np.zeros((h, w, 3)), np.zeros((h, w, 3)), np.zeros((h, w)), None)
    l = (c[..., 0] + c[..., 1] + c[..., 2]) / 3.0
    count = 0
    with np.errstate(all="ignore"):
        for dy in (-64, -32, 32, 64):
            for dx in (-64, -32, 32, 64):
                ys, xs = np.mgrid[max(0, -dy):min(h, h - dy), max(0, -dx):min(w, w - dx)]
                if ys.size == 0:
                    continue
                yj, xj = ys + dy, xs + dx
                pen = np.abs(l[ys, xs] - l[yj, xj]) / (cfg["sigma_l"] * np.sqrt(var[ys, xs]) + 1e-8)
                if with_feats and cfg["sigma_n"] > 0:
                    pen = pen + np.maximum(1.0 - _dot(N[ys, xs], N[yj, xj]), 0.0) / cfg["sigma_n"]
                if with_feats and cfg["sigma_z"] > 0:
                    pen = pen + np.abs(z[ys, xs] - z[yj, xj]) / (cfg["sigma_z"] * np.maximum(z[ys, xs], 1e-8))
                if with_feats and cfg["sigma_a"] > 0:
                    da = A[ys, xs] - A[yj, xj]
                    pen = pen + _dot(da, da) / (cfg["sigma_a"] * cfg["sigma_a"])
                count += int(np.count_nonzero(good[ys, xs] & good[yj, xj] & (pen <= 30.0)))
    return count
