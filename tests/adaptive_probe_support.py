"""Builds and loads tests/adaptive_probe.hip: compact_kernel and block_noise_kernel of csrc/pt_kernels.h (the adaptive check,
DESIGN 3.10), each launched by itself on lists of any length (test_adaptive_probe_cpu.py compiles it anywhere and checks the
references below on the CPU; test_adaptive_probe_gpu.py runs it).

The probe is compiled with the library's compiler and exactly its flags (path_trace_golang_amd.build.HIPCC, HIP_FLAGS), into a
temporary directory, never into the tree.  Also here: the NumPy references of the two kernels and the inputs of the GPU tests,
so that both can be checked without a device."""
from __future__ import annotations

import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np

import adaptive_support as ad
from fog_support import CSRC, ROOT, ptr

SOURCE = os.path.join(ROOT, "tests", "adaptive_probe.hip")
SYMBOLS = ("probe_compact", "probe_block_noise")
SENTINEL = 0xFFFFFFFF  # what the probe's output buffers hold before the launch
FSUM_BOUND = 8 * 2.0 ** -53  # b against math.fsum: six levels of additions of non-negative terms, a division, halved by the root,
#                              plus the root's and the reference's own roundings

_dir = None
_lib = None


def compile_probe() -> str:
    """Path of the probe's shared library (built once per process)."""
    global _dir
    from path_trace_golang_amd import build

    if _dir is None:
        _dir = tempfile.mkdtemp(prefix="adprobe_")
    out = os.path.join(_dir, "libadaptiveprobe.so")
    if not os.path.exists(out):
        r = subprocess.run([build.HIPCC, *build.HIP_FLAGS, "-shared", "-I", CSRC, SOURCE, "-o", out], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("adaptive probe does not compile:\n%s\n%s" % (r.stdout, r.stderr))
    return out


def load():
    """The probe, loaded after torch so that the process keeps one HIP runtime (as conftest.gpu_ctx does for libptcore.so)."""
    global _lib
    if _lib is None:
        import torch  # noqa: F401

        L = C.CDLL(compile_probe())
        vp = C.c_void_p
        L.probe_compact.argtypes = [vp, vp, vp, C.c_int64, vp, vp]
        L.probe_block_noise.argtypes = [vp, vp, C.c_int64, vp, C.c_int64, C.c_int32, C.c_int32, C.c_double, vp, vp, vp, vp]
        for s in SYMBOLS:
            getattr(L, s).restype = C.c_int
        _lib = L
    return _lib


def _ok(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError("%s: status %d" % (what, rc))


RES = np.dtype([("nact", np.uint32), ("reserved", np.uint32), ("worst", np.float64)])  # ptk::AdaptResult


# ---------------------------------------------------------------- compact_kernel
def compact(active, keep, noise):
    """compact_kernel on the device: (next uint32 [nact], res: one RES record)."""
    active, keep = np.ascontiguousarray(active, np.uint32), np.ascontiguousarray(keep, np.uint32)
    noise = np.ascontiguousarray(noise, np.float64)
    assert active.shape == keep.shape == noise.shape and active.ndim == 1
    nxt = np.zeros(active.size, np.uint32)
    res = np.zeros(1, RES)
    _ok(load().probe_compact(ptr(active), ptr(keep), ptr(noise), active.size, ptr(nxt), ptr(res)), "probe_compact")
    return nxt, res[0]


def compact_reference(active, keep, noise):
    """(next, nact, worst): the kept entries in order, then the sentinel; their number; their largest noise, 0.0 with none."""
    kept = np.asarray(keep) != 0
    c = int(kept.sum())
    nxt = np.full(len(active), SENTINEL, np.uint32)
    nxt[:c] = np.asarray(active)[kept]
    return nxt, c, float(np.max(np.asarray(noise)[kept])) if c else 0.0


def ascending_list(rng, n: int) -> np.ndarray:
    """n strictly ascending uint32 with a gap of at least 2 between neighbours, the last one 2^32 - 2."""
    gaps = rng.integers(2, max(3, (2 ** 32 - 2) // n), n, dtype=np.int64)
    a = np.cumsum(gaps)
    a += (2 ** 32 - 2) - a[-1]
    assert a[0] >= 0 and np.all(np.diff(a) >= 2)
    return a.astype(np.uint32)


COMPACT_LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 1088, 2047, 2048, 2049, 3071, 4097, 32400)


def compact_cases(n: int):
    """[(name, active, keep, noise)] for a list of n entries: every keep pattern that makes sense at that length."""
    rng = np.random.default_rng(1000 + n)
    active = ascending_list(rng, n)
    noise = rng.uniform(0.01, 4.0, n)
    i = np.arange(n)
    tail = (n - 1) // 1024 * 1024  # where the last strip begins
    pats = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "first": i == 0, "last": i == n - 1, "every second": i % 2 == 0,
            "every second, odd": i % 2 == 1}
    if n > 1023:
        pats["entry 1023"] = i == 1023
    if n > 1024:
        pats["entry 1024"] = i == 1024
        pats["first strip only"] = (i < 1024) & (rng.random(n) < 0.5)
        pats["last strip only"] = (i >= tail) & ((rng.random(n) < 0.5) | (i == tail))
    if n >= 64:
        pats["lane 63 of each wave"] = i % 64 == 63
    for p in (0.02, 0.5, 0.98):
        pats["random %.2f" % p] = rng.random(n) < p
    out = [(name, active, k.astype(np.uint32), noise) for name, k in pats.items()]
    k = rng.random(n) < 0.5
    out.append(("values other than 1", active, np.where(k, rng.choice(np.array([2, 256, 0x80000000, 0xFFFFFFFF], np.uint32), n), 0).astype(np.uint32),
                noise))
    if n >= 2:  # a dropped entry holds the largest noise
        k = rng.random(n) < 0.5
        j = int(rng.integers(0, n))
        k[j] = False
        k[(j + 1) % n] = True
        nz = noise.copy()
        nz[j] = 1e300
        out.append(("largest noise dropped", active, k.astype(np.uint32), nz))
    k = rng.random(n) < 0.5  # a kept +inf: the noise of a check at n < 2
    j = int(rng.integers(0, n))
    k[j] = True
    nz = noise.copy()
    nz[j] = np.inf
    out.append(("kept inf", active, k.astype(np.uint32), nz))
    return out


# ---------------------------------------------------------------- block_noise_kernel
GEOMETRIES = ((8, 8, 0, 1), (9, 9, 0, 1), (40, 24, 0, 1), (37, 21, 0, 1), (293, 253, 1, 3))  # (w, h, shard_index, shard_count)
SAMPLE_COUNTS = (1, 2, 8, 64)


def geom5(w, h, si, sc):
    return np.array([w, h, (w + 31) // 32, si, sc], np.int32)


def shard_slots(w, h, si, sc) -> int:
    ntx, nty = (w + 31) // 32, (h + 31) // 32
    return len(range(si, ntx * nty, sc)) * 1024


def slot_inside(w, h, si, sc) -> np.ndarray:
    """bool [nslots / 64, 64]: whether the frame holds the pixel of slot blk * 64 + p (block_pixel of csrc/pt_kernels.h)."""
    ntx = (w + 31) // 32
    nb = shard_slots(w, h, si, sc) // 64
    blk, p = np.arange(nb)[:, None], np.arange(64)[None, :]
    lt, sb = blk >> 4, blk & 15
    t = si + lt * sc
    ty, tx = t // ntx, t % ntx
    x = tx * 32 + (sb & 3) * 8 + (p & 7)
    y = ty * 32 + (sb >> 2) * 8 + (p >> 3)
    return (x < w) & (y < h)


def block_noise(acc, m2, active, n, decide, target, geom):
    """block_noise_kernel on the device: (blk_spp uint32 [nslots / 64], keep uint32 [nact], noise float64 [nact])."""
    acc, m2 = np.ascontiguousarray(acc, np.float64), np.ascontiguousarray(m2, np.float64)
    active = np.ascontiguousarray(active, np.uint32)
    geom = np.ascontiguousarray(geom, np.int32)
    nslots = acc.shape[1]
    assert acc.shape == m2.shape == (3, nslots) and geom.shape == (5,)
    spp = np.zeros(nslots // 64, np.uint32)
    keep = np.zeros(active.size, np.uint32)
    noise = np.zeros(active.size, np.float64)
    _ok(load().probe_block_noise(ptr(acc), ptr(m2), nslots, ptr(active), active.size, n, decide, target, ptr(geom), ptr(spp), ptr(keep),
                                 ptr(noise)), "probe_block_noise")
    return spp, keep, noise


def block_noise_reference(acc, m2, active, n, decide, target, inside):
    """(blk_spp, keep, noise) as the kernel must write them, bit for bit: pixel_e2 in its order over the lanes inside the frame
    (nothing outside is read), the xor butterfly, b = sqrt(sum / k)."""
    nb = inside.shape[0]
    active = np.asarray(active, np.int64)
    ins = inside[active]
    if n >= 2:
        a = np.where(ins[None], acc.reshape(3, nb, 64)[:, active], 0.0)  # the lanes outside the frame: never read, e2 = 0
        q = np.where(ins[None], m2.reshape(3, nb, 64)[:, active], 0.0)
        e2 = np.where(ins, ad.pixel_e2(a, q, n), 0.0)
        b = np.sqrt(ad.butterfly(e2) / ins.sum(axis=1))
    else:
        b = np.full(active.size, np.inf)
    spp = np.full(nb, SENTINEL, np.uint32)
    spp[active] = n
    keep = np.where(b <= target, 0, 1).astype(np.uint32) if decide else np.ones(active.size, np.uint32)
    return spp, keep, b


def block_noise_fsum(acc, m2, active, n, inside):
    """b of every listed block from math.fsum of its pixels' e2: the exactly rounded sum, then one division and one root."""
    nb = inside.shape[0]
    a, q = acc.reshape(3, nb, 64), m2.reshape(3, nb, 64)
    out = []
    for blk in np.asarray(active, np.int64):
        ins = inside[blk]
        e2 = ad.pixel_e2(a[:, blk][:, ins], q[:, blk][:, ins], n)
        out.append(math.sqrt(math.fsum(e2.tolist()) / int(ins.sum())))
    return np.array(out)


def block_noise_inputs(w, h, si, sc, n):
    """(acc, m2 [3, nslots], inside [nblocks, 64], all_bad: the block whose pixels are all bad, or None) of a shard after n samples:
    sums of seeded gamma samples, with pixels that are all zero, dim pixels (the 0.01 clamp with a variance), m2 a hair below
    S^2 / n (the negative-d clamp), NaN and infinite sums, one block of nothing else where the shard has more than one block, and a
    NaN in every slot outside the frame."""
    rng = np.random.default_rng(7 * w + 13 * h + 101 * si + n)
    ns = shard_slots(w, h, si, sc)
    inside = slot_inside(w, h, si, sc)
    l = rng.gamma(0.6, 0.8, (n, 3, ns)) * rng.uniform(0.05, 2.0, (1, 1, ns))
    kind = rng.random(ns)
    l[:, :, kind < 0.05] = 0.0                      # all-zero pixels
    l[:, :, (kind >= 0.05) & (kind < 0.10)] *= 1e-3   # dim pixels: mean below 0.01
    acc = np.zeros((3, ns))
    m2 = np.zeros((3, ns))
    for s in range(n):  # in sample order, like the kernels
        acc = acc + l[s]
        m2 = m2 + l[s] * l[s]
    hair = (kind >= 0.10) & (kind < 0.15)
    m2[:, hair] = (acc[:, hair] * acc[:, hair] / n) * (1.0 - 2.0 ** -40)
    for lo, hi, v, plane in ((0.15, 0.17, np.nan, acc), (0.17, 0.19, np.inf, acc), (0.19, 0.20, -np.inf, acc), (0.20, 0.21, np.inf, m2),
                             (0.21, 0.22, np.nan, m2)):
        sel = np.nonzero((kind >= lo) & (kind < hi))[0]
        plane[rng.integers(0, 3, sel.size), sel] = v
    blocks = np.nonzero(inside.any(axis=1))[0]
    all_bad = None
    if blocks.size > 1:
        all_bad = int(blocks[blocks.size // 2])
        acc[:, all_bad * 64:all_bad * 64 + 64] = np.nan
    out = ~inside.reshape(-1)
    acc[:, out] = np.nan
    m2[:, out] = np.nan
    return acc, m2, inside, all_bad


def block_noise_lists(w, h, si, sc):
    """{name: active list}: every block with a pixel inside the frame; a sparse random subset whose length is no multiple of 4 (the
    last workgroup of four waves is partly filled); the last block alone (9 x 9: the corner block with one pixel)."""
    rng = np.random.default_rng(w * 1000 + h)
    full = ad.block_order(w, h, si, sc)[:, 0].astype(np.uint32)
    lists = {"all": full, "single": full[-1:]}
    if full.size >= 4:
        m = max(3, full.size // 3)
        m += 1 if m % 4 == 0 else 0
        lists["sparse"] = np.sort(rng.choice(full, m, replace=False))
        assert lists["sparse"].size % 4 != 0
    return lists


def block_noise_targets(b: np.ndarray):
    """0, huge, exactly one block's b (equality stops it) and the double below it (keeps it)."""
    ok = b[np.isfinite(b) & (b > 0)]
    t = [0.0, 1e300]
    if ok.size:
        one = float(np.sort(ok)[ok.size // 2])
        t += [one, float(np.nextafter(one, 0.0))]
    return t
