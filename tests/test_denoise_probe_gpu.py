"""The kernels of the a-trous filter, of the pair filter and of the temporal accumulation on the MI355X, on inputs no rendered frame
gives (tests/denoise_probe.hip): non-finite and degenerate pixels where the blocks and waves meet, frames of
4 x 9 blocks and frames two pixels thin, cameras that roll, turn, dolly, zoom, pass through a wall and jump.  Every case of
test_denoise_probe_cpu.py runs on the device against the C restatement ("ref"), never against the host build of the header: planes,
history, len and rgba bit for bit, counts exactly, figures to 1e-9.  That the inputs reach what they are meant to reach is asserted
in the CPU test, on the restatement alone."""
from __future__ import annotations

import numpy as np
import pytest

import atrous_support as at
import denoise_probe_support as dp
import halves_support as hv
import temporal_support as ts

pytestmark = pytest.mark.gpu

SHAPE_IDS = ["%dx%d" % s for s in dp.SHAPES]


@pytest.fixture(autouse=True, scope="module")
def _probe(gpu_ctx):
    return dp.load()


@pytest.mark.parametrize("size", dp.SHAPES, ids=SHAPE_IDS)
def test_filter_kernels_match_the_restatement_on_special_inputs(size):
    w, h = size
    _, _, _, _, places = dp.shape_inputs(w, h)
    bad = [p for k, p in places if k in dp.BAD_KINDS]
    for case in dp.filter_cases(w, h):
        got = dp.run_filter_case("gpu", w, h, case)
        want = dp.run_filter_case("ref", w, h, case)
        at.assert_same_run(got, want, (size, case))
        assert got["bad_pixels"] == len(bad) == 5
        for p in bad:  # the 8-bit image of a bad pixel is the restatement's
            assert np.array_equal(got["rgba"][p], want["rgba"][p]), (size, case, p)
        assert np.all(got["rgba"][..., 3] == 255)


@pytest.mark.parametrize("size", dp.SHAPES, ids=SHAPE_IDS)
def test_pair_kernels_match_the_restatement_on_special_inputs(size):
    w, h = size
    for case in dp.filter_cases(w, h):
        got = dp.run_filter_case("gpu", w, h, case, pair=True)
        want = dp.run_filter_case("ref", w, h, case, pair=True)
        hv.assert_same_pair(got, want, (size, case))
        assert got["bad_pixels"] == 5


@pytest.mark.parametrize("name", dp.SEQUENCES)
def test_temporal_kernel_matches_the_restatement_on_synthetic_sequences(name):
    frames = dp.sequence(name)
    for tcfg in dp.TCONFIGS:
        for flt in dp.FILTERS:
            want, want_hist = dp.run_frames("ref", frames, flt, **tcfg)
            got, got_hist = dp.run_frames("gpu", frames, flt, **tcfg)
            for k, (a, b) in enumerate(zip(got, want)):
                ts.assert_same_frame(a, b, (name, tcfg, flt, k))
                npix = frames[k]["w"] * frames[k]["h"]
                if dp.has_history(frames, k):
                    assert a["reprojected"] + a["disoccluded"] + a["bad_pixels"] == npix
                    if a["reprojected"] == 0:  # every good pixel disoccluded: len' is 1 everywhere good and 0 on the bad pixels
                        isbad = np.zeros((frames[k]["h"], frames[k]["w"]), bool)
                        for p in frames[k]["bad"]:
                            isbad[p] = True
                        assert np.all(a["hist_len"][~isbad] == 1) and np.all(a["hist_len"][isbad] == 0)
            # the probe's read of the stored history is the restatement's tr_read
            assert at.same_bits(got_hist[0], want_hist[0]) and at.same_bits(got_hist[1], want_hist[1]) and np.array_equal(got_hist[2], want_hist[2])
    if name in ("turn", "through the wall"):
        assert any(r["reprojected"] == 0 for r in want[1:])


def test_the_probe_refuses_bad_arguments_before_launching():
    import ctypes as C

    L = dp.load()
    S, Q, n, feats, _ = dp.shape_inputs(33, 9)
    out = (np.zeros((9, 33, 3)), np.zeros((9, 33)), np.zeros((9, 33, 4), np.uint8), np.zeros(2))
    bad = C.c_uint64(0)
    sig = np.array([4.0, 0.1, 0.1, 0.2])
    p = at.ptr
    args = lambda **kw: [kw.get("w", 33), 9, p(S), p(Q), None, kw.get("n", 9), None, None, None, kw.get("T", 5), p(kw.get("sig", sig)), p(out[0]), p(out[1]),
                         p(out[2]), p(out[3]), C.byref(bad)]
    assert L.probe_filter(*args()) == 0
    assert L.probe_filter(*args(w=0)) == -1 and L.probe_filter(*args(T=7)) == -1 and L.probe_filter(*args(T=-1)) == -1
    assert L.probe_filter(*args(n=1)) == -5 and L.probe_filter(*args(sig=np.array([0.0, 0.1, 0.1, 0.2]))) == -4
    a = args()
    a[6] = p(feats[0])  # one feature plane without the others
    assert L.probe_filter(*a) == -3
    a = args()
    a[11] = None
    assert L.probe_filter(*a) == -2
    acc = dp.GpuAccumulator()
    assert acc.read(33, 9) is None
    fr = dp.sequence("sideways 33 x 9")[0]
    with pytest.raises(RuntimeError, match="status -6"):
        acc.frame(fr["S"], fr["Q"], fr["n"], fr["feats"], fr["cam"], None, None, alpha=1.5)
    with pytest.raises(RuntimeError, match="status -5"):
        acc.frame(fr["S"], fr["Q"], 1, fr["feats"], fr["cam"])
    assert acc.read(33, 9) is None  # a refused frame leaves the history as it was
    acc.close()
