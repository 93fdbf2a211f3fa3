"""block_err_kernel, block_pool_kernel and keep_from_map_kernel on the MI355X through tests/filtered_adaptive_probe.hip, which calls
the product's own launch sequences: the planted planes and grids of test_filtered_adaptive_cpu.py (NaN and infinite errs, pixels
bad in one half, luminances below 0.01, a block whose every pixel is bad), bit for bit against the plain-Python restatement; and
active lists of one device and of one shard of three, one of them longer than a strip of compact_kernel.  The only place where
frames no rendered scene gives reach the new kernels."""
from __future__ import annotations

import numpy as np
import pytest

import adaptive_support as ad
import filtered_adaptive_probe_support as fp
import filtered_adaptive_support as fa
from adaptive_support import bits

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, scope="module")
def _built(gpu_ctx):
    return gpu_ctx


@pytest.mark.parametrize("w,h", fa.GRIDS)
def test_the_block_map_kernels_equal_the_restatement(w, h):
    mean, err, bad = fa.planted(w, h)
    for pool in fa.POOLS:
        target = float(np.median(fa.restate_blocks(mean, err, bad, pool, 0.0)["pooled"]))
        for t in (target, 0.0, np.inf):  # the median (some stop, the block at the median by the rule's <=), nothing stops, everything
            want = fa.restate_blocks(mean, err, bad, pool, t)
            got = fp.block_map(mean, err, bad, pool, t)  # (every output was 0xFF bytes before the launch)
            fa.assert_same_blocks(got, want, (w, h, pool, t))
        assert want["stop"].all()


@pytest.mark.parametrize("w,h,si,sc", fp.LISTS, ids=lambda v: str(v))
def test_keep_from_map_and_the_compaction_behind_it(w, h, si, sc):
    order = ad.block_order(w, h, si, sc)
    ns = fp.shard_slots(w, h, si, sc)
    nby, nbx = fa.grid(w, h)
    rng = np.random.default_rng(w * 7 + si)
    pooled = rng.uniform(0.01, 2.0, (nby, nbx))
    lists = {"every block": order, "every third": order[::3], "one": order[-1:]}
    stops = {"random": (rng.random((nby, nbx)) < 0.5).astype(np.uint8), "none": np.zeros((nby, nbx), np.uint8),
             "all": np.ones((nby, nbx), np.uint8)}
    if w > 200:
        assert len(order) > (1024 if sc == 1 else 256)
    for lname, lst in lists.items():
        for sname, stop in {**stops, "no map": None}.items():
            tag = (lname, sname)
            n = 24
            want = fp.keep_reference(lst, ns, n, None if stop is None else pooled, stop)
            got = fp.keep_from_map(lst[:, 0], w, h, si, sc, n, None if stop is None else pooled, stop)
            assert np.array_equal(got["blk_spp"], want["blk_spp"]), tag  # n in the listed blocks, untouched elsewhere
            assert np.array_equal(got["keep"], want["keep"]), tag
            assert np.array_equal(bits(got["noise"]), bits(want["noise"])), tag
            c = want["nact"]
            assert int(got["res"]["nact"]) == c and int(got["res"]["reserved"]) == 0, tag
            assert np.array_equal(got["next"][:c], want["next"][:c]) and np.all(got["next"][c:] == fp.SENTINEL), tag
            assert bits(np.float64(got["res"]["worst"])) == bits(np.float64(want["worst"])), tag


def test_bad_arguments_are_refused_before_anything_is_launched():
    order = ad.block_order(70, 45, 0, 1)
    L = fp.load()
    from fog_support import ptr

    out = fp.keep_reference(order, fp.shard_slots(70, 45, 0, 1), 8)
    act = np.array([6 * 16], np.uint32)  # a block of a seventh tile: the frame has six
    g = fp.geom5(70, 45, 0, 1)
    res = np.zeros(1, fp.RES)
    bufs = [np.zeros(7 * 16, np.uint32), np.zeros(1, np.uint32), np.zeros(1), np.zeros(1, np.uint32), res]
    assert L.probe_keep_from_map(ptr(act), 1, 7 * 1024, None, None, 8, ptr(g), *(ptr(b) for b in bufs)) == -2
    assert L.probe_keep_from_map(ptr(act), 1, 1000, None, None, 8, ptr(g), *(ptr(b) for b in bufs)) == -1
    assert out["nact"] == len(order)
