"""The probe of the adaptive check's two kernels (tests/adaptive_probe.hip) without a GPU: it cross-compiles for gfx950 with the
library's flags against the unchanged pt_kernels.h and exports what test_adaptive_probe_gpu.py calls.  Also the references that
test holds the kernels to, checked here against plain-Python restatements of the same operations (no NumPy in them), and the
inputs of the GPU tests: that they contain what their names promise."""
from __future__ import annotations

import math
import re
import subprocess

import numpy as np
import pytest

import adaptive_probe_support as ap
import adaptive_support as ad


def test_probe_compiles_for_gfx950_with_the_library_flags():
    from path_trace_golang_amd import build

    assert "-ffp-contract=off" in build.HIP_FLAGS and "--offload-arch=gfx950" in build.HIP_FLAGS
    lib = ap.compile_probe()
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (\w+)", syms))
    assert set(ap.SYMBOLS) <= exported, sorted(set(ap.SYMBOLS) - exported)
    with open(lib, "rb") as f:
        blob = f.read()
    assert b"gfx950" in blob
    for kernel in (b"compact_kernel", b"block_noise_kernel"):
        assert kernel in blob, kernel


def test_probe_source_launches_the_product_kernels_and_has_no_inline_assembly():
    with open(ap.SOURCE) as f:
        src = f.read()
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code
    assert '#include "pt_kernels.h"' in src
    # the product's kernels and argument records, not copies of them
    for name in ("ptk::compact_kernel", "ptk::block_noise_kernel", "ptk::CompactArgs", "ptk::BlockNoiseArgs", "ptk::AdaptResult"):
        assert name in code, name
    assert "__global__" not in code
    # the product's own grid expressions (dev_adaptive_check, ptcore.hip)
    assert "dim3(1), dim3(PT_COMPACT_BLOCK)" in code and "dim3((A.nact * 64u + PT_BLOCK - 1) / PT_BLOCK), dim3(PT_BLOCK)" in code
    assert ap.RES.itemsize == 16 and ap.RES.fields["worst"][1] == 8


# ---------------------------------------------------------------- compact_kernel's reference and inputs
@pytest.mark.parametrize("n", [1, 2, 65, 1025, 4097])
def test_compact_reference_equals_a_plain_loop(n):
    for name, active, keep, noise in ap.compact_cases(n):
        want, worst = [], 0.0
        for a, k, b in zip(active.tolist(), keep.tolist(), noise.tolist()):
            if k != 0:
                want.append(a)
                worst = b if b > worst else worst
        nxt, c, w = ap.compact_reference(active, keep, noise)
        assert c == len(want) and nxt[:c].tolist() == want and np.all(nxt[c:] == ap.SENTINEL), (n, name)
        assert w == worst and (c > 0 or w == 0.0), (n, name)


def test_compact_cases_hold_what_the_names_say():
    names = set()
    for n in ap.COMPACT_LENGTHS:
        cases = ap.compact_cases(n)
        for name, active, keep, noise in cases:
            names.add(name)
            assert active.dtype == np.uint32 and keep.dtype == np.uint32 and len(active) == len(keep) == len(noise) == n
            a = active.astype(np.int64)
            assert np.all(np.diff(a) >= 2) and a[-1] == 2 ** 32 - 2 and np.all(noise > 0)
        d = {name: (keep, noise) for name, _, keep, noise in cases}
        assert d["all"][0].all() and not d["none"][0].any() and np.flatnonzero(d["first"][0]).tolist() == [0]
        assert np.flatnonzero(d["last"][0]).tolist() == [n - 1]
        if n > 1024:
            assert np.flatnonzero(d["entry 1023"][0]).tolist() == [1023] and np.flatnonzero(d["entry 1024"][0]).tolist() == [1024]
            k = np.flatnonzero(d["first strip only"][0])
            assert k.size > 64 and k.max() < 1024
            k = np.flatnonzero(d["last strip only"][0])
            assert k.size > 0 and k.min() >= (n - 1) // 1024 * 1024
        if n >= 64:
            assert np.flatnonzero(d["lane 63 of each wave"][0]).tolist() == list(range(63, n, 64))
        k, _ = d["values other than 1"]
        assert n < 8 or (set(k.tolist()) - {0, 1} and 0 in k)
        if n >= 2:
            k, nz = d["largest noise dropped"]
            assert k[np.argmax(nz)] == 0 and k.any()
        k, nz = d["kept inf"]
        assert np.isinf(nz).sum() == 1 and k[np.argmax(nz)] != 0
    assert ap.COMPACT_LENGTHS == (1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 1088, 2047, 2048, 2049, 3071, 4097, 32400)
    assert {"all", "none", "first", "last", "entry 1023", "entry 1024", "every second", "lane 63 of each wave", "first strip only",
            "last strip only", "random 0.02", "random 0.50", "random 0.98", "values other than 1", "largest noise dropped",
            "kept inf"} <= names


# ---------------------------------------------------------------- block_noise_kernel's reference and inputs
def _block_python(acc, m2, blk, inside, n):
    """b of one block in plain Python floats: pixel_e2's operations per lane, the butterfly on a list, one division, one root."""
    lanes = []
    for p in range(64):
        if not inside[blk, p]:
            lanes.append(0.0)
            continue
        slot = blk * 64 + p
        msum, vsum = 0.0, 0.0
        for c in range(3):
            m = float(acc[c, slot]) / float(n)
            d = float(m2[c, slot]) / float(n) - m * m
            if d < 0.0:
                d = 0.0
            msum += m
            vsum += d / float(n - 1)
        den = msum / 3.0
        if den < 0.01:
            den = 0.01
        e2 = (vsum / 3.0) / (den * den)
        lanes.append(0.0 if (math.isnan(e2) or math.isinf(e2)) else e2)
    s = lanes
    for off in (32, 16, 8, 4, 2, 1):
        s = [s[i] + s[i ^ off] for i in range(64)]
    return math.sqrt(s[0] / int(inside[blk].sum()))


@pytest.mark.parametrize("geom", ap.GEOMETRIES, ids=lambda g: "%dx%d_%dof%d" % g)
def test_block_noise_reference_equals_plain_python_and_fsum(geom):
    worst = 0.0
    for n in ap.SAMPLE_COUNTS:
        acc, m2, inside, all_bad = ap.block_noise_inputs(*geom, n)
        nb = inside.shape[0]
        assert acc.shape == m2.shape == (3, nb * 64) == (3, ap.shard_slots(*geom))
        assert np.isnan(acc[:, ~inside.reshape(-1)]).all() and np.isnan(m2[:, ~inside.reshape(-1)]).all()
        lists = ap.block_noise_lists(*geom)
        assert lists["all"].tolist() == [b for b in range(nb) if inside[b].any()] and len(lists["single"]) == 1
        for lname, active in lists.items():
            assert np.all(np.diff(active.astype(np.int64)) > 0)
            spp, keep, b = ap.block_noise_reference(acc, m2, active, n, int(n >= 2), 0.3, inside)
            assert np.all(spp[active] == n) and np.all(np.delete(spp, active) == ap.SENTINEL)
            if n < 2:
                assert np.all(np.isinf(b)) and np.all(keep == 1)
                continue
            assert np.all(np.isfinite(b)) and np.all(b >= 0)
            sub = active if len(active) <= 24 else active[:: len(active) // 24]
            for blk in sub.tolist():
                want = _block_python(acc, m2, blk, inside, n)
                i = int(np.flatnonzero(active == blk)[0])
                assert b[i] == want, (geom, n, lname, blk)
                assert keep[i] == (0 if want <= 0.3 else 1)
            f = ap.block_noise_fsum(acc, m2, active, n, inside)
            rel = np.abs(b - f) / np.where(f > 0, f, 1.0)
            assert np.all(rel <= ap.FSUM_BOUND) and np.all((f > 0) | (b == 0)), (geom, n, lname, rel.max())
            worst = max(worst, float(rel.max()))
            if all_bad is not None and all_bad in active.tolist():
                assert b[active.tolist().index(all_bad)] == 0.0
            # equality stops a block, the double below keeps it
            t = ap.block_noise_targets(b)
            assert len(t) == 4 and t[2] in b.tolist()
            at = b == t[2]
            assert np.all(ap.block_noise_reference(acc, m2, active, n, 1, t[2], inside)[1][at] == 0)
            assert np.all(ap.block_noise_reference(acc, m2, active, n, 1, t[3], inside)[1][at] == 1)
            assert np.all(ap.block_noise_reference(acc, m2, active, n, 0, 1e300, inside)[1] == 1)
            assert np.all(ap.block_noise_reference(acc, m2, active, n, 1, 1e300, inside)[1] == 0)
    print("largest relative distance of the restated b from fsum: %.3g (bound %.3g)" % (worst, ap.FSUM_BOUND))


def test_block_noise_inputs_hold_every_pixel_case():
    geom = ap.GEOMETRIES[-1]
    for n in (2, 64):
        acc, m2, inside, all_bad = ap.block_noise_inputs(*geom, n)
        ins = inside.reshape(-1)
        a, q = acc[:, ins], m2[:, ins]
        with np.errstate(all="ignore"):
            m = a / n
            d = q / n - m * m
        assert np.any(np.all(a == 0, axis=0) & np.all(q == 0, axis=0))                       # all zero
        assert np.any((m.sum(axis=0) / 3 < 0.01) & (m.sum(axis=0) > 0) & np.all(d > 0, axis=0))  # dim, with a variance
        assert np.any(np.all((d < 0) & (d > -1e-6), axis=0))                                    # a hair below
        assert np.isnan(a).any() and np.isposinf(a).any() and np.isneginf(a).any() and np.isposinf(q).any() and np.isnan(q).any()
        assert all_bad is not None and inside[all_bad].all() and np.isnan(acc[:, all_bad * 64:all_bad * 64 + 64]).all()
    # the geometries: the one-block frame, the corner block with one pixel, cut edges, a shard of three
    assert int(ap.slot_inside(9, 9, 0, 1)[5].sum()) == 1 and ap.block_noise_lists(9, 9, 0, 1)["single"].tolist() == [5]
    assert ap.GEOMETRIES == ((8, 8, 0, 1), (9, 9, 0, 1), (40, 24, 0, 1), (37, 21, 0, 1), (293, 253, 1, 3)) and ap.SAMPLE_COUNTS == (1, 2, 8, 64)
    for g in ap.GEOMETRIES:
        ls = ap.block_noise_lists(*g)
        assert "sparse" not in ls or (len(ls["sparse"]) % 4 != 0 and len(ls["sparse"]) < len(ls["all"]))
    assert "sparse" in ap.block_noise_lists(*ap.GEOMETRIES[-1]) and len(ap.block_noise_lists(*ap.GEOMETRIES[-1])["all"]) > 64


# ---------------------------------------------------------------- the list order and the predictor of test_adaptive_scale_gpu.py
@pytest.mark.parametrize("w,h,count", [(40, 24, 1), (37, 21, 2), (293, 253, 1), (293, 253, 3), (293, 253, 7)])
def test_block_order_is_the_tile_map(w, h, count):
    from path_trace_golang_amd import tiling

    seen = set()
    for k in range(count):
        order = ad.block_order(w, h, k, count)
        inside = ap.slot_inside(w, h, k, count)
        assert order[:, 0].tolist() == [b for b in range(inside.shape[0]) if inside[b].any()]  # ascending: the host's first list
        tiles = tiling.shard_tiles(w, h, k, count)
        for blk, by, bx in order.tolist():
            x0, y0, x1, y1 = tiling.tile_rect(w, h, tiles[blk >> 4])
            sb = blk & 15
            assert (x0 + (sb & 3) * 8, y0 + (sb >> 2) * 8) == (bx * 8, by * 8) and bx * 8 < x1 and by * 8 < y1
            assert (by, bx) not in seen
            seen.add((by, bx))
    assert len(seen) == ((h + 7) // 8) * ((w + 7) // 8)
    if (w, h) == (293, 253):
        assert len(seen) == 1184 and (w + 31) // 32 * ((h + 31) // 32) == 80


def test_predict_equals_the_restated_plan_on_synthetic_samples():
    """predict works on the frames' sums; plan_restated on per-sample radiances, in plain Python.  Same maps, and the lists follow."""
    rng = np.random.default_rng(5)
    h, w, cap, step = 21, 37, 32, 8
    shape = ad.expand(np.arange(15).reshape(3, 5), w, h) * 0.2 + 0.15  # a noise level of its own for every block
    l = rng.gamma(shape[:, :, None, None], 0.6, (h, w, cap, 3)) * rng.uniform(0.2, 3.0, (h, w, 1, 1))
    frames = {}
    for n in range(step, cap + 1, step):
        S = np.zeros((h, w, 3))
        Q = np.zeros((h, w, 3))
        for s in range(n):
            S = S + l[:, :, s]
            Q = Q + l[:, :, s] * l[:, :, s]
        frames[n] = (S, Q)
    target = float(np.median(ad.block_noise_map(*frames[16], 16))) * 1.001  # about half of the blocks stop by 16 samples
    want, checks = ad.plan_restated(l, target, step, 0, cap)
    for ndev in (1, 2):
        p = ad.predict(frames, target, step, 0, cap, ndev)
        assert p["counts"].tolist() == want and len(set(np.unique(p["counts"]).tolist())) >= 3
        for by, bx, done, b in checks:  # the butterfly's sum and the plain loop's differ by roundings only
            assert abs(p["noise"][done][by, bx] - b) <= ap.FSUM_BOUND * b
        assert p["margin"] > 1e-6 and p["samples"] == int(ad.expand(want, w, h).astype(np.uint64).sum())
        total = 0
        for i, n in enumerate(p["checks"]):
            rows = [r for d in range(ndev) for r in map(tuple, p["lists"][d][i].tolist())]
            assert sorted(rows) == sorted((by, bx) for by in range(3) for bx in range(5) if want[by][bx] > n or (n == cap and p["noise"][n][by, bx] > target))
            total = len(rows)
        assert total == p["active"] and (p["worst"] > target) == (total > 0)
    # min_spp: no decision before it
    p = ad.predict(frames, 1e9, step, 20, cap)
    assert np.all(p["counts"] == 24) and p["active"] == 0 and p["worst"] == 0.0
