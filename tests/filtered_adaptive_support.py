"""Helpers of the filtered-adaptive tests (test_filtered_adaptive_cpu.py, test_filtered_adaptive_gpu.py; DESIGN 3.12a, the model in
csrc/pt_atrous.h BLOCKS): a host build of the block functions of csrc/pt_atrous.h looped the way block_err_kernel and block_pool_kernel
run them; the restatement of steps 2 to 4 in plain Python floats, independent of that code; planted planes no rendered frame gives;
and the predictor of a whole frame with the rule on from the plain frames of its checks."""
from __future__ import annotations

import ctypes as C
import math
import os
import subprocess

import numpy as np

import adaptive_support as ad
import atrous_support as at
import halves_support as hs
from fog_support import CSRC, CXXFLAGS, ptr

SHIM = r"""
#include <cmath>
#include <vector>
#include "pt_atrous.h"
extern "C" void shim_blocks(int32_t W, int32_t H, const double *mean, const double *err, const double *bad, int32_t pool, double target,
                            double *s, uint32_t *k, double *pooled, double *own, uint8_t *stop) {
    const int32_t nbx = (W + 7) / 8, nby = (H + 7) / 8;
    for (int32_t by = 0; by < nby; by++)
        for (int32_t bx = 0; bx < nbx; bx++) {
            double lane[64];
            uint32_t kk = 0;
            for (int p = 0; p < 64; p++) {  // block_err_kernel: one lane per pixel, zeros outside the frame
                const int32_t x = bx * 8 + (p & 7), y = by * 8 + (p >> 3);
                lane[p] = 0.0;
                if (x >= W || y >= H) continue;
                const size_t i = (size_t)y * W + x;
                lane[p] = pta::block_term(mean + 3 * i, err[i], (int)bad[i]);
                kk++;
            }
            for (int off = 32; off > 0; off >>= 1) {  // its xor butterfly
                double next[64];
                for (int p = 0; p < 64; p++) next[p] = lane[p] + lane[p ^ off];
                for (int p = 0; p < 64; p++) lane[p] = next[p];
            }
            s[(size_t)by * nbx + bx] = lane[0];
            k[(size_t)by * nbx + bx] = kk;
        }
    for (int32_t by = 0; by < nby; by++)
        for (int32_t bx = 0; bx < nbx; bx++) {  // block_pool_kernel: one lane per block
            const size_t b = (size_t)by * nbx + bx;
            pooled[b] = pta::pool_block(s, k, nbx, nby, bx, by, pool, own[b]);
            stop[b] = pooled[b] <= target ? 1 : 0;
        }
}
"""

_lib = None
_vp = C.c_void_p

GRIDS = ((37, 21), (97, 71), (8, 8), (130, 2))  # ragged on both edges; several rows and columns; one block; a strip two pixels high
POOLS = (0, 1, 2, 4)                             # 4 reaches past the 37 x 21 grid (5 x 3 blocks) on every side


def product_host():
    """The block functions of csrc/pt_atrous.h built for the host with g++."""
    global _lib
    if _lib is None:
        d = at._build_dir()
        src = os.path.join(d, "blocks_shim.cpp")
        with open(src, "w") as f:
            f.write(SHIM)
        out = os.path.join(d, "libblocksshim.so")
        subprocess.run(["g++", *CXXFLAGS, "-shared", "-I", CSRC, src, "-o", out], check=True, capture_output=True)
        _lib = C.CDLL(out)
        _lib.shim_blocks.argtypes = [C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_int32, C.c_double, _vp, _vp, _vp, _vp, _vp]
    return _lib


def grid(w: int, h: int):
    return (h + 7) // 8, (w + 7) // 8


def host_blocks(mean, err, bad, pool: int, target: float) -> dict:
    """Steps 2 to 4 by the host build: dict(s, k, pooled, own, stop), each [nby, nbx]."""
    mean, err, bad = (np.ascontiguousarray(a, np.float64) for a in (mean, err, bad))
    h, w = err.shape
    g = grid(w, h)
    r = dict(s=np.zeros(g), k=np.zeros(g, np.uint32), pooled=np.zeros(g), own=np.zeros(g), stop=np.zeros(g, np.uint8))
    product_host().shim_blocks(w, h, ptr(mean), ptr(err), ptr(bad), int(pool), float(target), *(ptr(r[n]) for n in ("s", "k", "pooled", "own", "stop")))
    return r


def _finite(v: float) -> bool:
    return not (math.isnan(v) or math.isinf(v))


def restate_blocks(mean, err, bad, pool: int, target: float) -> dict:
    """Steps 2 to 4 of the model, pixel by pixel and block by block in plain Python floats."""
    h, w = err.shape
    nby, nbx = grid(w, h)
    s = [[0.0] * nbx for _ in range(nby)]
    k = [[0] * nbx for _ in range(nby)]
    for by in range(nby):
        for bx in range(nbx):
            lane = [0.0] * 64
            for p in range(64):
                y, x = by * 8 + (p >> 3), bx * 8 + (p & 7)
                if y >= h or x >= w:
                    continue
                k[by][bx] += 1
                m = [float(v) for v in mean[y, x]]
                l = (m[0] + m[1] + m[2]) / 3.0
                den = 0.01 if l < 0.01 else l
                e2 = float(err[y, x]) / (den * den)
                if int(bad[y, x]) == 0 and _finite(e2):
                    lane[p] = e2
            for off in (32, 16, 8, 4, 2, 1):
                lane = [lane[p] + lane[p ^ off] for p in range(64)]
            s[by][bx] = lane[0]
    r = dict(s=np.array(s), k=np.array(k, np.uint32), pooled=np.zeros((nby, nbx)), own=np.zeros((nby, nbx)), stop=np.zeros((nby, nbx), np.uint8))
    for by in range(nby):
        for bx in range(nbx):
            ss, kk = 0.0, 0
            for y in range(by - pool, by + pool + 1):
                if y < 0 or y >= nby:
                    continue
                for x in range(bx - pool, bx + pool + 1):
                    if x < 0 or x >= nbx:
                        continue
                    ss = ss + s[y][x]
                    kk += k[y][x]
            P = math.sqrt(ss / kk)
            r["pooled"][by, bx] = P
            r["own"][by, bx] = math.sqrt(s[by][bx] / k[by][bx])
            r["stop"][by, bx] = 1 if P <= target else 0
    return r


def assert_same_blocks(a: dict, b: dict, tag="") -> None:
    """Two runs of steps 2 to 4 agree: the sums and both figures bit for bit, the pixel counts and the flags."""
    for n in ("s", "pooled", "own"):
        assert at.same_bits(a[n], b[n]), (tag, n, a[n].tolist(), b[n].tolist())
    assert np.array_equal(a["k"], b["k"]), (tag, "k")
    assert np.array_equal(a["stop"], b["stop"]), (tag, "stop")


def planted(w: int, h: int, seed: int = 7):
    """(mean [h, w, 3], err [h, w], bad [h, w] as the guide's plane: 0, 1, 2 or 3) with what no rendered frame gives: NaN, +inf and -inf
    errs, pixels bad in half A only and in half B only, luminances below 0.01 (zero and negative ones too), and one block -- the last of
    the grid -- whose every pixel is bad (s_B = 0 with k_B > 0)."""
    rng = np.random.default_rng(seed + 1000 * w + h)
    mean = rng.uniform(0.02, 2.0, (h, w, 3))
    err = rng.uniform(0.0, 0.05, (h, w)) ** 2
    bad = np.zeros((h, w))
    n = w * h
    flat = list(rng.permutation(n))

    def pick(m):  # the next m pixels of the permutation: no pixel is planted twice
        idx = [flat.pop() for _ in range(m)]
        return np.unravel_index(idx, (h, w))

    m = max(1, n // 40)
    err[pick(m)] = np.nan
    err[pick(m)] = np.inf
    err[pick(m)] = -np.inf
    bad[pick(m)] = 1.0
    bad[pick(m)] = 2.0
    bad[pick(m)] = 3.0
    mean[pick(m)] = rng.uniform(0.0005, 0.0095, (m, 3))
    mean[pick(m)] = rng.uniform(-0.004, -0.001, (m, 3))
    mean[pick(m)] = 0.0
    mean[pick(1)] = np.nan
    nby, nbx = grid(w, h)
    if nby * nbx > 1:
        bad[(nby - 1) * 8:, (nbx - 1) * 8:] = 3.0
    return mean, err, bad


# ---------------------------------------------------------------- the whole rule, from the plain frames of its checks
def compose(frames: dict, counts: np.ndarray, w: int, h: int):
    """The four half sums of the adaptive state whose blocks hold `counts` [nby, nbx] samples: every pixel from the plain frame of its
    count.  frames = {n: (SA, QA, SB, QB)}.  Returns (SA, QA, SB, QB, per-pixel counts)."""
    px = ad.expand(counts, w, h)
    out = [np.zeros((h, w, 3)) for _ in range(4)]
    for n in np.unique(px):
        sel = px == n
        for i in range(4):
            out[i][sel] = frames[int(n)][i][sel]
    return (*out, px)


def predict(frames: dict, feats, target: float, step: int, min_spp: int, cap: int, pool: int, pair=None, **cfg) -> dict:
    """A frame with the rule on, from plain ones: frames = {n: (SA, QA, SB, QB)} at n = step, 2 * step, ..., cap, feats the feature
    sums of any of them (or None).  At each check the state is composed from the per-block counts, `pair` (halves_support.ref_pair,
    the restatement of the pair filter) runs on it and restate_blocks applies the rule.  Returns counts [nby, nbx], figures
    {n: (pooled, own)} of the checks that decided, active [nby, nbx], by_neighbours (blocks some check kept although
    own <= target < pooled), stopped_in_window (blocks that stopped at a check while some block of the grid stayed active), worst (the
    largest pooled figure among the active blocks of the last check that decided, 0 with none), history (the counts after every
    check, in order) and samples."""
    pair = pair or hs.ref_pair
    h, w = next(iter(frames.values()))[0].shape[:2]
    nby, nbx = grid(w, h)
    checks = list(range(step, cap, step)) + [cap]
    assert sorted(frames) == checks
    counts = np.zeros((nby, nbx), np.int64)
    active = np.ones((nby, nbx), bool)
    by_neighbours = np.zeros((nby, nbx), bool)
    figures = {}
    margin = np.inf
    worst = 0.0
    history = []
    for n in checks:
        counts[active] = n
        if n >= max(min_spp, 4):
            SA, QA, SB, QB, px = compose(frames, counts, w, h)
            r = pair(SA, QA, SB, QB, n, px, feats, **cfg)
            assert r["bad_pixels"] == 0  # (a rendered frame has none: the bad mask is all zeros)
            b = restate_blocks(r["mean"], r["err"], np.zeros((h, w)), pool, target)
            figures[n] = (b["pooled"], b["own"])
            if target > 0:
                margin = min(margin, float(np.min(np.abs(b["pooled"][active] - target) / target)))
            by_neighbours |= active & (b["own"] <= target) & (b["pooled"] > target)
            active = active & ~(b["pooled"] <= target)
            worst = float(b["pooled"][active].max()) if active.any() else 0.0
        history.append(counts.copy())
        if not active.any():
            break
    return {"history": history, "counts": counts, "figures": figures, "active": active, "by_neighbours": by_neighbours, "margin": margin, "worst": worst,
            "samples": int(ad.expand(counts, w, h).astype(np.uint64).sum())}


# scene, depth, seed, cap, step, min_spp, k, pool: example_simple at 40 x 24 = 3 x 5 blocks, the default filter.  CASE_TARGET was picked on
# the CPU from the oracle's samples (test_filtered_adaptive_cpu.py checks what it was picked for): some blocks stop and others do
# not, and at least one block is kept alive only by its neighbours.
CASE = ("example_simple", 4, 1, 32, 8, 0, 4, 1)
CASE_TARGET = 0.25  # the nearest (block, check) is 3.8e-3 of the target away
CASE_MAP = [[24, 16, 24, 16, 32], [32, 24, 32, 16, 16], [32, 32, 32, 24, 32]]
CASE_SAMPLES = 24576  # of 30720
CASE_ACTIVE = 5


def case_frames():
    """The oracle's side of CASE: ({n: (SA, QA, SB, QB)} at every check's count, the feature sums of the first k samples)."""
    import moments_support as ms

    name, depth, seed, cap, step, _, k, _ = CASE
    l = ms.samples(name, depth, seed, cap)
    feats = at.ref_features(name, ms.W, ms.H, cap, depth, seed, k)
    return {n: hs.half_sums(l[:, :, :n]) for n in range(step, cap + 1, step)}, feats


# ---------------------------------------------------------------- does the rule pay?  The CPU study of DESIGN 3.12a, oracle samples only
# The five shipped scenes at 80 x 48 (10 x 6 blocks), cap 64, step 8, k = 4, the default filter, depth 4, seed 1.  Truth: the oracle's
# 8 192-spp frame of seed 2, kept under tests/golden/ (study_truth recomputes it when asked).  Figure: relative MSE of pt_atrous's model
# (atrous_support.ref_filter, every pixel with its own count), section 3.11's normalisation.
STUDY = dict(w=80, h=48, cap=64, step=8, k=4, depth=4, seed=1, truth_spp=8192, truth_seed=2)
STUDY_SCENES = ("example_simple", "gpu_showcase", "metal_glass_room", "test_comprehensive", "test_scene")
STUDY_POOLS = (0, 1, 2)
_study = {}


def study_truth_path(name: str) -> str:
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "filtered_adaptive_truth_%s.npy" % name)


def study_truth(name: str, recompute: bool = False) -> np.ndarray:
    """The mean of the oracle's 8 192-spp frame of seed 2, float64 [48, 80, 3]: the committed fixture, or the oracle's own run."""
    if not recompute:
        return np.load(study_truth_path(name))
    from oracle import ora

    r = ora.render(at.ora_scene_of(name), STUDY["w"], STUDY["h"], STUDY["truth_spp"], STUDY["depth"], seed=STUDY["truth_seed"], want=("accum",))
    return r["accum"] / float(STUDY["truth_spp"])


def study_inputs(name: str) -> dict:
    """Per scene, once: the oracle's per-sample radiances l [48, 80, 64, 3], the half sums and the full sums at every check's count,
    and the feature sums of the first k samples."""
    if name not in _study:
        import moments_support as ms
        from oracle import ora

        w, h, cap, step, depth, seed = (STUDY[k] for k in ("w", "h", "cap", "step", "depth", "seed"))
        sc = at.ora_scene_of(name)
        l = np.empty((h, w, cap, 3))
        for y in range(h):
            for x in range(w):
                for s in range(cap):
                    l[y, x, s] = ora.sample(sc, w, h, cap, depth, seed, x, y, s)[0]
        l.setflags(write=False)
        _study[name] = dict(l=l, halves={n: hs.half_sums(l[:, :, :n]) for n in range(step, cap + 1, step)},
                            sums={n: ms.sums(l[:, :, :n]) for n in range(1, cap + 1)},
                            feats=at.ref_features(name, w, h, cap, depth, seed, STUDY["k"]))
    return _study[name]


def study_filtered_mse(name: str, counts: np.ndarray) -> float:
    """Relative MSE against the truth of the filtered image of the frame whose blocks hold `counts` [nby, nbx] samples."""
    d = study_inputs(name)
    w, h = STUDY["w"], STUDY["h"]
    px = ad.expand(counts, w, h)
    S, Q = np.zeros((h, w, 3)), np.zeros((h, w, 3))
    for n in np.unique(px):
        sel = px == n
        S[sel], Q[sel] = d["sums"][int(n)][0][sel], d["sums"][int(n)][1][sel]
    return at.relative_mse(at.ref_filter(S, Q, 0, px, d["feats"])["mean"], study_truth(name))


def study_rule(name: str, target: float, pool: int) -> dict:
    """The new rule on the scene: dict(samples, share of the cap's samples, rel_mse, counts)."""
    d = study_inputs(name)
    r = predict(d["halves"], d["feats"], target, STUDY["step"], 0, STUDY["cap"], pool)
    full = STUDY["w"] * STUDY["h"] * STUDY["cap"]
    return dict(samples=r["samples"], share=r["samples"] / float(full), rel_mse=study_filtered_mse(name, r["counts"]), counts=r["counts"])


def study_own(name: str, target: float) -> dict:
    """Section 3.10's own-noise rule at `target` on the same samples (hip.adaptive_plan_host, min_spp 0)."""
    from path_trace_golang_amd import hip

    counts = hip.adaptive_plan_host(study_inputs(name)["l"], target, STUDY["step"], 0, STUDY["cap"])
    return dict(samples=int(ad.expand(counts, STUDY["w"], STUDY["h"]).astype(np.uint64).sum()), rel_mse=study_filtered_mse(name, counts))


def study_uniform(name: str, samples: int) -> dict:
    """The uniform frame of the sample count nearest to `samples` in all."""
    n = max(2, min(STUDY["cap"], int(round(samples / float(STUDY["w"] * STUDY["h"])))))
    nby, nbx = grid(STUDY["w"], STUDY["h"])
    return dict(spp=n, samples=n * STUDY["w"] * STUDY["h"], rel_mse=study_filtered_mse(name, np.full((nby, nbx), n, np.int64)))


# The study's committed figures (test_filtered_adaptive_cpu.py recomputes them): per scene the relative MSE of the full 64-spp
# frame, then per pool (target of the rule, its samples, its relative MSE, the own-noise rule's bisected target, its samples and relative MSE,
# the uniform frame's sample count and relative MSE).  The rule's target is chosen per scene and pool so that it takes 48 - 52 % of the cap.
STUDY_TABLE = {
    "example_simple": (0.03605184181826101, {
        0: (0.08593, 119296, 0.04657557848204109, 0.316406, 118784, 0.04496268719937229, 31, 0.060705147207957125),
        1: (0.1719, 120320, 0.05240298877983189, 0.3125, 120832, 0.044552954478203524, 31, 0.060705147207957125),
        2: (0.1875, 120832, 0.0650777961335461, 0.3125, 120832, 0.044552954478203524, 31, 0.060705147207957125),
    }),
    "gpu_showcase": (0.050008502952093914, {
        0: (0.375, 124928, 0.11157151979168932, 0.507812, 124416, 0.10153589089129539, 33, 0.09324391522959506),
        1: (0.4062, 123392, 0.0985221156130825, 0.507812, 124416, 0.10153589089129539, 32, 0.09661811938512206),
        2: (0.4062, 125952, 0.09573312956516501, 0.503906, 124928, 0.10156676228770171, 33, 0.09324391522959506),
    }),
    "metal_glass_room": (0.014771950608132463, {
        0: (0.2188, 124928, 0.019690366893590924, 0.398438, 124416, 0.019370782333425908, 33, 0.02292688688968721),
        1: (0.2188, 125952, 0.019076811505737198, 0.397462, 125952, 0.019131402911046605, 33, 0.02292688688968721),
        2: (0.2344, 124928, 0.020345963652787267, 0.398438, 124416, 0.019370782333425908, 33, 0.02292688688968721),
    }),
    "test_comprehensive": (0.060525749863994206, {
        0: (0.4062, 122368, 0.09790855216039382, 0.648438, 121344, 0.13726525755232194, 32, 0.10023200591740104),
        1: (0.4219, 124416, 0.10297481741900191, 0.642578, 124928, 0.12143267359307816, 32, 0.10023200591740104),
        2: (0.4219, 124928, 0.09899821764626722, 0.640625, 125952, 0.12104175672221791, 33, 0.09616432699209508),
    }),
    "test_scene": (0.11888195464705814, {
        0: (0.1875, 122368, 0.15091598826704625, 0.4375, 121344, 0.15541683902518047, 32, 0.16541380401968628),
        1: (0.2578, 121344, 0.15038420111425105, 0.4375, 121344, 0.15541683902518047, 32, 0.16541380401968628),
        2: (0.2852, 124416, 0.15783854566221991, 0.429688, 124416, 0.1533316654263913, 32, 0.16541380401968628),
    }),
}
