"""Helpers of the adaptive-sampling tests (test_adaptive_cpu.py, test_adaptive_gpu.py): the case the issue fixes, a plain-Python
restatement of the block rule on per-sample radiances (independent of hip.adaptive_plan_host), and the self-consistency check
that needs no oracle: every block of an adaptive frame is bit-equal to the same block of a plain frame of the block's count.
For test_adaptive_scale_gpu.py and the probe of the two check kernels (adaptive_probe_support.py): the NumPy statement of
block_noise_kernel's arithmetic in its own order (pixel_e2, butterfly), the order of a device's active list (block_order) and
the predictor of an adaptive frame from the plain frames of its checks (predict)."""
from __future__ import annotations

import math

import numpy as np

from moments_support import H, W

# scene, depth, seed, cap, step, min_spp, target: example_simple at 40 x 24 = 3 x 5 blocks of 8 x 8
CASE = ("example_simple", 4, 1, 64, 8, 0, 0.25)
CASE_MAP = [[48, 32, 16, 24, 40], [64, 64, 48, 64, 64], [40, 64, 32, 32, 40]]
CASE_SAMPLES = 43008  # of 61440


def plan_restated(l: np.ndarray, target: float, step: int, min_spp: int, cap: int):
    """The block rule of include/ptcore.h, block by block and pixel by pixel in plain Python floats.  l = [H, W, >= cap, 3].
    Returns (counts [nby][nbx], checks): checks = every (by, bx, done, b) the rule looked at, in order."""
    h, w = l.shape[0], l.shape[1]
    nby, nbx = (h + 7) // 8, (w + 7) // 8
    counts = [[0] * nbx for _ in range(nby)]
    checks = []
    for by in range(nby):
        for bx in range(nbx):
            pix = [(y, x) for y in range(by * 8, min(by * 8 + 8, h)) for x in range(bx * 8, min(bx * 8 + 8, w))]
            S = {p: [0.0, 0.0, 0.0] for p in pix}
            Q = {p: [0.0, 0.0, 0.0] for p in pix}
            done = 0
            while done < cap:
                n = min(step, cap - done)
                for s in range(done, done + n):
                    for (y, x) in pix:
                        for c in range(3):
                            v = float(l[y, x, s, c])
                            S[(y, x)][c] += v
                            Q[(y, x)][c] += v * v
                done += n
                counts[by][bx] = done
                if done < max(min_spp, 2):
                    continue
                total = 0.0
                for p in pix:
                    m = [S[p][c] / done for c in range(3)]
                    d = [Q[p][c] / done - m[c] * m[c] for c in range(3)]
                    v = [(0.0 if dc < 0.0 else dc) / (done - 1) for dc in d]
                    den = (m[0] + m[1] + m[2]) / 3.0
                    den = 0.01 if den < 0.01 else den
                    e2 = ((v[0] + v[1] + v[2]) / 3.0) / (den * den)
                    if not (math.isnan(e2) or math.isinf(e2)):
                        total += e2
                b = math.sqrt(total / len(pix))
                checks.append((by, bx, done, b))
                if b <= target:
                    break
    return counts, checks


def expand(block_counts, w: int = W, h: int = H) -> np.ndarray:
    """Block counts [nby][nbx] as the per-pixel plane pt_read_sample_counts returns, uint32 [h, w]."""
    a = np.asarray(block_counts, np.uint32)
    return np.repeat(np.repeat(a, 8, axis=0), 8, axis=1)[:h, :w].copy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def render_adaptive(ctx, sc, w, h, cap, depth, seed, target, step, min_spp=0, chunk=0, flags=0, progress=None, **kw):
    """One adaptive frame through hip.render: (img, acc, m2, counts, nseg, ndraw, st)."""
    from path_trace_golang_amd import hip

    img = np.zeros((h, w, 4), np.uint8)
    acc = np.zeros((h, w, 3))
    m2 = np.zeros((h, w, 3))
    counts = np.full((h, w), 0xFFFFFFFF, np.uint32)
    nseg = np.zeros((h, w), np.uint32) if flags else None
    ndraw = np.zeros((h, w), np.uint32) if flags else None
    st = hip.render(sc, hip.RenderConfig(w, h, cap, depth, seed, chunk, flags), img, progress, acc, nseg, ndraw, ctx=ctx, moments=m2,
                    noise=target, noise_step=step, adaptive=True, min_spp=min_spp, counts=counts, **kw)
    return img, acc, m2, counts, nseg, ndraw, st


def check_state(st: dict, counts: np.ndarray, cap: int):
    """pt_adaptive_state and pt_stats of a frame against its counts plane."""
    h, w = counts.shape
    blocks = ((h + 7) // 8) * ((w + 7) // 8)
    a = st["adaptive"]
    total = int(counts.astype(np.uint64).sum())
    assert a["blocks"] == blocks
    assert a["samples"] == total and st["samples"] == total  # pt_adaptive_state.samples and pt_stats.samples
    assert a["spp_min"] == int(counts.min()) and a["spp_max"] == int(counts.max()) == st["spp_done"]
    assert 0 <= a["active_blocks"] <= blocks
    if a["active_blocks"]:
        assert a["spp_max"] == cap  # the frame went on until no block was active, or to the cap
        assert a["worst_active"] > 0
    else:
        assert a["worst_active"] == 0
    # a block's pixels share one count
    blk = counts[::8, ::8]
    assert np.array_equal(expand(blk, w, h), counts)


def check_self_consistent(ctx, sc, w, h, cap, depth, seed, target, step, min_spp=0, chunk=0, min_distinct=2, **kw):
    """An adaptive frame on ctx, then for each distinct count n a plain n-sample frame of the same context: the blocks that hold n
    samples are bit-equal in rgba, accum and m2.  Returns (counts, st)."""
    from path_trace_golang_amd import hip

    img, acc, m2, counts, _, _, st = render_adaptive(ctx, sc, w, h, cap, depth, seed, target, step, min_spp, chunk, **kw)
    assert counts.min() >= 1 and counts.max() <= cap  # zeros nowhere inside the frame
    check_state(st, counts, cap)
    distinct = sorted(set(int(v) for v in np.unique(counts)))
    assert len(distinct) >= min_distinct, distinct
    for n in distinct:
        pi = np.zeros((h, w, 4), np.uint8)
        pa = np.zeros((h, w, 3))
        pm = np.zeros((h, w, 3))
        hip.render(sc, hip.RenderConfig(w, h, n, depth, seed, chunk), pi, None, pa, ctx=ctx, moments=pm, **kw)
        sel = counts == n
        assert np.array_equal(img[sel], pi[sel]), ("rgba", n)
        assert np.array_equal(bits(acc)[sel], bits(pa)[sel]), ("accum", n)
        assert np.array_equal(bits(m2)[sel], bits(pm)[sel]), ("m2", n)
    return counts, st


# ---------------------------------------------------------------- the gather check (one tile map, one gather)
GATHER_W, GATHER_H, GATHER_SPP = 70, 45, 8  # 3 x 2 tiles, ragged on both edges; 6 tiles = 2, 2, 1, 1 on four devices, none for the seventh
GATHER_PLANES = ("rgba", "accum", "nseg", "ndraw", "m2", "ad_rgba", "ad_accum", "ad_nseg", "ad_ndraw", "ad_m2", "ad_counts")
_gather_ref = []


def gather_frames(ctx, sc=None) -> dict:
    """Every plane a context gathers, of two frames of the case's scene at 70 x 45 with pixel stats and moments on: a plain frame of 8
    samples, and the case's adaptive frame (its cap, step and target), whose blocks must end with different counts and some of them
    active.  Also the pt_noise_estimate fields of both ("noise", "ad_noise") and the adaptive frame's pt_adaptive_state ("ad_state")."""
    from conftest import scene_path
    from path_trace_golang_amd import capi, hip, scene

    name, depth, seed, cap, step, min_spp, target = CASE
    w, h = GATHER_W, GATHER_H
    sc = sc or scene.load(scene_path(name))
    d = {"rgba": np.zeros((h, w, 4), np.uint8), "accum": np.zeros((h, w, 3)), "m2": np.zeros((h, w, 3)),
         "nseg": np.zeros((h, w), np.uint32), "ndraw": np.zeros((h, w), np.uint32)}
    hip.render(sc, hip.RenderConfig(w, h, GATHER_SPP, depth, seed, 0, capi.PT_FLAG_PIXEL_STATS), d["rgba"], None, d["accum"], d["nseg"],
               d["ndraw"], ctx=ctx, moments=d["m2"])
    d["noise"] = hip.noise_estimate(ctx)
    (d["ad_rgba"], d["ad_accum"], d["ad_m2"], d["ad_counts"], d["ad_nseg"], d["ad_ndraw"], st) = render_adaptive(
        ctx, sc, w, h, cap, depth, seed, target, step, min_spp, flags=capi.PT_FLAG_PIXEL_STATS)
    d["ad_noise"] = hip.noise_estimate(ctx)
    d["ad_state"] = st["adaptive"]
    # the target stops some blocks and not others
    assert d["ad_counts"].min() < cap and 0 < d["ad_state"]["active_blocks"] < d["ad_state"]["blocks"] == 54, d["ad_state"]
    assert d["nseg"].min() > 0 and np.all(d["m2"] >= 0) and np.any(d["m2"] > 0)
    return d


def gather_reference() -> dict:
    """gather_frames of a one-device context that gathers by itself (no PTCORE_GATHER), made once per process and read-only."""
    import os

    from path_trace_golang_amd import capi

    if not _gather_ref:
        assert "PTCORE_GATHER" not in os.environ
        with capi.Context(ndev=1) as ctx:
            d = gather_frames(ctx)
        for k in GATHER_PLANES:
            d[k].setflags(write=False)
        _gather_ref.append(d)
    return _gather_ref[0]


def assert_same_planes(got: dict, ref: dict, tag=""):
    for k in GATHER_PLANES:
        a, b = got[k], ref[k]
        assert a.dtype == b.dtype and a.shape == b.shape, (tag, k)
        assert np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b), (tag, k)


# ---------------------------------------------------------------- the check in NumPy, and frames whose lists outgrow a wave and a strip
def pixel_e2(acc, m2, n: int) -> np.ndarray:
    """pixel_e2 of csrc/pt_kernels.h with its operations in its order, elementwise over acc, m2 = [3, ...] (n >= 2): bit-equal to the
    device by IEEE arithmetic.  A NaN or infinite e2 comes back as 0."""
    nn, n1 = float(n), float(n - 1)
    msum, vsum = 0.0, 0.0
    with np.errstate(all="ignore"):
        for c in range(3):
            m = acc[c] / nn
            d = m2[c] / nn - m * m
            d = np.where(d < 0.0, 0.0, d)  # (a NaN stays a NaN)
            msum = msum + m
            vsum = vsum + d / n1
        den = msum / 3.0
        den = np.where(den < 0.01, 0.01, den)
        e2 = (vsum / 3.0) / (den * den)
        bad = ~((e2 - e2) == 0.0)
    return np.where(bad, 0.0, e2)


def butterfly(e2: np.ndarray) -> np.ndarray:
    """Lane 0's value after the xor butterfly of block_noise_kernel over [..., 64] lanes (zeros in the lanes outside the frame)."""
    idx = np.arange(64)
    s = np.array(e2, np.float64)
    for off in (32, 16, 8, 4, 2, 1):
        s = s + s[..., idx ^ off]
    return s[..., 0]


def block_order(w: int, h: int, shard_index: int, shard_count: int) -> np.ndarray:
    """The blocks of one device that have a pixel inside the frame, in the order of its first active list: tile
    t = shard_index + lt * shard_count, then sub-block sb = 0..15.  int64 [n, 3]: (blk = lt * 16 + sb, by, bx), by and bx being
    the block's row and column in the frame's 8 x 8 grid."""
    ntx, nty = (w + 31) // 32, (h + 31) // 32
    out = []
    for lt, t in enumerate(range(shard_index, ntx * nty, shard_count)):
        ty, tx = divmod(t, ntx)
        for sb in range(16):
            by, bx = ty * 4 + (sb >> 2), tx * 4 + (sb & 3)
            if by * 8 < h and bx * 8 < w:
                out.append((lt * 16 + sb, by, bx))
    return np.asarray(out, np.int64).reshape(-1, 3)


def block_noise_map(acc: np.ndarray, m2: np.ndarray, n: int) -> np.ndarray:
    """b of every 8 x 8 block of a plain n-sample frame (acc, m2 = [h, w, 3]) as block_noise_kernel computes it, [nby, nbx]."""
    h, w = acc.shape[:2]
    nby, nbx = (h + 7) // 8, (w + 7) // 8
    e2 = np.zeros((nby * 8, nbx * 8))
    inside = np.zeros((nby * 8, nbx * 8), bool)
    inside[:h, :w] = True
    if n >= 2:
        e2[:h, :w] = pixel_e2(np.moveaxis(acc, 2, 0), np.moveaxis(m2, 2, 0), n)

    def lanes(a):  # [nby, nbx, 64], lane p = row * 8 + column inside the block
        return a.reshape(nby, 8, nbx, 8).transpose(0, 2, 1, 3).reshape(nby, nbx, 64)

    k = lanes(inside).sum(axis=2)
    return np.sqrt(butterfly(lanes(e2)) / k) if n >= 2 else np.full((nby, nbx), np.inf)


def predict(frames: dict, target: float, step: int, min_spp: int, cap: int, ndev: int = 1) -> dict:
    """An adaptive frame from plain ones.  frames = {n: (acc, m2)} of the plain frames at n = step, 2 * step, ..., cap.  Returns
    counts [nby, nbx], noise {n: [nby, nbx]}, lists {device: [the (by, bx) rows of its list after each check]}, margin (the
    smallest relative distance of a deciding (block, check) from the target), worst (the largest noise among the blocks the
    last check kept, 0 with none), active (their number) and samples."""
    h, w = next(iter(frames.values()))[0].shape[:2]
    nby, nbx = (h + 7) // 8, (w + 7) // 8
    checks = list(range(step, cap, step)) + [cap]
    assert sorted(frames) == checks
    counts = np.zeros((nby, nbx), np.int64)
    active = np.ones((nby, nbx), bool)
    noise, after = {}, []
    margin = np.inf
    for n in checks:
        counts[active] = n
        noise[n] = b = block_noise_map(frames[n][0], frames[n][1], n)
        if n >= max(min_spp, 2):
            margin = min(margin, float(np.min(np.abs(b[active] - target) / target))) if active.any() and target > 0 else margin
            active = active & ~(b <= target)
        after.append(active.copy())
        if not active.any():
            break
    lists = {}
    for d in range(ndev):
        order = block_order(w, h, d, ndev)
        lists[d] = [order[a[order[:, 1], order[:, 2]]][:, 1:] for a in after]
    last = noise[max(noise)]
    return {"counts": counts, "noise": noise, "lists": lists, "margin": margin, "worst": float(last[active].max()) if active.any() else 0.0,
            "active": int(active.sum()), "samples": int(expand(counts, w, h).astype(np.uint64).sum()), "checks": checks[:len(after)]}


# scene, width, height, depth, seed, cap, step, min_spp: example_simple at 293 x 253 = 32 rows of 37 blocks in 8 rows of 10 tiles, both edges cut.
# SCALE_LISTS: the list lengths after the checks at 8, 16, 24 and 32 samples per (target, devices), device by device, computed from
# the oracle's per-sample radiances on the CPU (the nearest (block, check) is 2.9e-4 of the target away at 0.30, 3.9e-5 at 0.45).
SCALE = ("example_simple", 293, 253, 4, 1, 32, 8, 0)
SCALE_LISTS = {(0.30, 1): [[1035, 801, 599, 439]],
               (0.30, 3): [[364, 289, 216, 153], [348, 282, 206, 157], [323, 230, 177, 129]],
               (0.45, 3): [[265, 114, 60, 35], [257, 98, 51, 34], [209, 89, 38, 32]]}


def scale_frames(ctx, sc=None) -> dict:
    """{n: (rgba, accum, m2)} of the plain frames of SCALE at every check's count, rendered on ctx."""
    from conftest import scene_path
    from path_trace_golang_amd import hip, scene

    name, w, h, depth, seed, cap, step, _ = SCALE
    sc = sc or scene.load(scene_path(name))
    out = {}
    for n in range(step, cap + 1, step):
        img = np.zeros((h, w, 4), np.uint8)
        acc = np.zeros((h, w, 3))
        m2 = np.zeros((h, w, 3))
        hip.render(sc, hip.RenderConfig(w, h, n, depth, seed), img, None, acc, ctx=ctx, moments=m2)
        for a in (img, acc, m2):
            a.setflags(write=False)
        out[n] = (img, acc, m2)
    return out
