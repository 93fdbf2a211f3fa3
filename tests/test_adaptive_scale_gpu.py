"""Adaptive frames whose active lists outgrow one wave and one strip of compact_kernel: example_simple at 293 x 253,
1184 blocks of 8 x 8 in 80 tiles, both edges cut.  On one device the first check reads 1184 entries and writes more than 1024, the
second reads those; on three devices the lists run from a few hundred down to below one wave.

The reference never touches the adaptive kernels: adaptive_support.predict applies the block rule in NumPy to the plain frames at
8, 16, 24 and 32 samples of the same context (the plain kernels are pinned to the oracle elsewhere) and gives the count map and
every device's list after every check.  The preconditions -- no (block, check) within 1e-6 of the target, lists on both sides of
64 and 1024 -- are asserted on that prediction, and its list lengths are those computed from the oracle's per-sample radiances."""
from __future__ import annotations

import numpy as np
import pytest

import adaptive_support as ad
from adaptive_probe_support import FSUM_BOUND
from adaptive_support import bits
from conftest import scene_path

pytestmark = pytest.mark.gpu

NAME, W, H, DEPTH, SEED, CAP, STEP, MIN_SPP = ad.SCALE
PLANES = ("rgba", "accum", "m2", "counts", "nseg", "ndraw")


@pytest.fixture(autouse=True, scope="module")
def _built(gpu_ctx):
    return gpu_ctx


@pytest.fixture(scope="module")
def scene(_built):
    from path_trace_golang_amd import scene as scn

    return scn.load(scene_path(NAME))


def _adaptive_planes(ctx, sc, target, chunk=0):
    from path_trace_golang_amd import capi

    img, acc, m2, counts, nseg, ndraw, st = ad.render_adaptive(ctx, sc, W, H, CAP, DEPTH, SEED, target, STEP, MIN_SPP, chunk,
                                                               flags=capi.PT_FLAG_PIXEL_STATS)
    return dict(zip(PLANES, (img, acc, m2, counts, nseg, ndraw))), st


@pytest.fixture(scope="module")
def one_device(scene):
    """On one context of one device: the plain frames, the predictions for both targets and one, three and seven devices, and the
    adaptive frames of both targets with every plane a context gathers (the per-pixel counters included).  Read-only."""
    from path_trace_golang_amd import capi

    with capi.Context(ndev=1) as ctx:
        frames = ad.scale_frames(ctx, scene)
        planes = {t: _adaptive_planes(ctx, scene, t) for t in (0.30, 0.45)}
    sums = {n: (f[1], f[2]) for n, f in frames.items()}
    pred = {(t, k): ad.predict(sums, t, STEP, MIN_SPP, CAP, k) for t in (0.30, 0.45) for k in (1, 3, 7)}
    for p, _ in planes.values():
        for a in p.values():
            a.setflags(write=False)
    return frames, pred, planes


def _lengths(p):
    return [[len(rows) for rows in p["lists"][d]] for d in sorted(p["lists"])]


def _check_against_the_prediction(p, planes, st, target):
    counts = planes["counts"]
    want = ad.expand(p["counts"], W, H)
    assert np.array_equal(counts, want), int(np.count_nonzero(counts != want))
    a = st["adaptive"]
    assert (a["blocks"], a["active_blocks"], a["samples"]) == (1184, p["active"], p["samples"]) and st["samples"] == p["samples"]
    assert (a["spp_min"], a["spp_max"]) == (int(p["counts"].min()), CAP)
    print("target %.2f: worst_active %.17g, predicted %.17g" % (target, a["worst_active"], p["worst"]))
    assert p["worst"] > target and abs(a["worst_active"] - p["worst"]) <= FSUM_BOUND * p["worst"]


def test_the_predictions_are_what_the_case_needs(one_device):
    """The preconditions, on the reference side only."""
    frames, pred, _ = one_device
    for (t, k), want in ad.SCALE_LISTS.items():
        assert _lengths(pred[(t, k)]) == want, (t, k, _lengths(pred[(t, k)]))
    for key, p in pred.items():
        print("target %.2f, %d devices: nearest (block, check) %.3g of the target away; lists %s" % (*key, p["margin"], _lengths(p)))
        assert p["margin"] > 1e-6 and p["checks"] == [8, 16, 24, 32]
        assert sorted(set(np.unique(p["counts"]).tolist())) == [8, 16, 24, 32]
        assert np.array_equal(p["counts"], pred[(key[0], 1)]["counts"])  # the map does not know the device count
    # one device: a check whose incoming list is longer than one strip keeps entries on both sides of position 1024
    p = pred[(0.30, 1)]
    order = [tuple(r) for r in ad.block_order(W, H, 0, 1)[:, 1:].tolist()]
    incoming = [order] + [[tuple(r) for r in rows.tolist()] for rows in p["lists"][0]]
    assert len(order) == 1184
    long_lists, both_sides = 0, 0
    for before, after in zip(incoming, incoming[1:]):
        if len(before) > 1024:
            pos = [before.index(r) for r in after]
            assert pos == sorted(pos)
            long_lists += 1
            both_sides += min(pos) < 1024 <= max(pos)
    assert both_sides >= 1
    assert long_lists == 2 and len(incoming[1]) > 1024  # the first check writes more than one strip, the second reads it
    # three devices: some device stays between one wave and one strip at every check; at 0.45 some list ends within one wave
    assert any(all(65 <= n <= 1023 for n in dev) for dev in _lengths(pred[(0.30, 3)]))
    assert any(dev[-1] <= 64 for dev in _lengths(pred[(0.45, 3)])) and all(dev[0] > 64 for dev in _lengths(pred[(0.45, 3)]))
    assert any(dev[-1] <= 64 for dev in _lengths(pred[(0.30, 7)]))


def test_one_device_holds_the_predicted_map_and_lists(scene, one_device):
    """The counts plane equals the predicted map; every block is bit-equal in rgba, accum and m2 to the plain frame of its count;
    pt_adaptive_state's active blocks and samples are the prediction's, worst_active the largest predicted noise among the kept."""
    from path_trace_golang_amd import capi

    frames, pred, planes = one_device
    with capi.Context(ndev=1) as ctx:
        counts, st = ad.check_self_consistent(ctx, scene, W, H, CAP, DEPTH, SEED, 0.30, STEP, MIN_SPP, min_distinct=4)
    p = pred[(0.30, 1)]
    _check_against_the_prediction(p, {"counts": counts}, st, 0.30)
    # the frame with the per-pixel counters on (the other build of the kernels), against the plain frames of the fixture
    got, st = planes[0.30]
    _check_against_the_prediction(p, got, st, 0.30)
    for n, (img, acc, m2) in frames.items():
        sel = got["counts"] == n
        assert sel.any() and np.array_equal(got["rgba"][sel], img[sel]), n
        assert np.array_equal(bits(got["accum"])[sel], bits(acc)[sel]) and np.array_equal(bits(got["m2"])[sel], bits(m2)[sel]), n
    _check_against_the_prediction(pred[(0.45, 1)], planes[0.45][0], planes[0.45][1], 0.45)


@pytest.mark.parametrize("target", [0.30, 0.45])
@pytest.mark.parametrize("k", [3, 7])
def test_virtual_devices_gather_the_one_device_frame(scene, one_device, k, target):
    from path_trace_golang_amd import capi

    _, pred, planes = one_device
    with capi.Context(devices=[0] * k) as ctx:
        got, st = _adaptive_planes(ctx, scene, target)
    assert st["num_devices"] == k
    ref, rst = planes[target]
    for name in PLANES:
        a, b = got[name], ref[name]
        assert a.dtype == b.dtype and np.array_equal(bits(a) if a.dtype == np.float64 else a, bits(b) if b.dtype == np.float64 else b), name
    _check_against_the_prediction(pred[(target, k)], got, st, target)
    for key in ("samples", "segments", "draws"):
        assert st[key] == rst[key], key
    assert st["adaptive"] == rst["adaptive"]


def test_one_device_in_chunks_of_three(scene, one_device):
    from path_trace_golang_amd import capi

    _, pred, planes = one_device
    with capi.Context(ndev=1) as ctx:
        counts, st = ad.check_self_consistent(ctx, scene, W, H, CAP, DEPTH, SEED, 0.30, STEP, MIN_SPP, chunk=3, min_distinct=4)
        got, gst = _adaptive_planes(ctx, scene, 0.30, chunk=3)
    assert st["spp_chunk"] == 3 and gst["spp_chunk"] == 3
    _check_against_the_prediction(pred[(0.30, 1)], {"counts": counts}, st, 0.30)
    ref, _ = planes[0.30]
    for name in PLANES:
        a, b = got[name], ref[name]
        assert np.array_equal(bits(a) if a.dtype == np.float64 else a, bits(b) if b.dtype == np.float64 else b), name
