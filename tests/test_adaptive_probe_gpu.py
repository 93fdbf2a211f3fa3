"""compact_kernel and block_noise_kernel on the MI355X, each by itself through tests/adaptive_probe.hip, on active lists that
straddle a wave (64), the workgroup (1024 entries: one strip) and several strips, up to the 32 400 blocks of a 1080p frame: the
lengths no frame of the suite reaches.  Everything is exact: compact_kernel against NumPy's boolean selection, block_noise_kernel
bit for bit against the NumPy statement of its operations in their order (adaptive_probe_support.py, itself checked against plain
Python in test_adaptive_probe_cpu.py), and its b within 8 * 2^-53 relative of math.fsum over the block's pixels."""
from __future__ import annotations

import numpy as np
import pytest

import adaptive_probe_support as ap
from adaptive_support import bits

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, scope="module")
def _built(gpu_ctx):
    return gpu_ctx


@pytest.mark.parametrize("n", ap.COMPACT_LENGTHS)
def test_compact_kernel_equals_numpy(n):
    """next = the kept entries in order, the sentinel behind them; res = (their number, 0, the largest noise among them)."""
    for name, active, keep, noise in ap.compact_cases(n):
        want, c, worst = ap.compact_reference(active, keep, noise)
        nxt, res = ap.compact(active, keep, noise)
        tag = (n, name)
        assert int(res["nact"]) == c and int(res["reserved"]) == 0, (tag, res)
        assert np.array_equal(nxt[:c], want[:c]), (tag, int(np.flatnonzero(nxt[:c] != want[:c])[0]))
        assert np.all(nxt[c:] == ap.SENTINEL), (tag, "written behind the new list")
        assert bits(np.float64(res["worst"])) == bits(np.float64(worst)), (tag, float(res["worst"]), worst)


@pytest.mark.parametrize("n", ap.SAMPLE_COUNTS)
@pytest.mark.parametrize("geom", ap.GEOMETRIES, ids=lambda g: "%dx%d_%dof%d" % g)
def test_block_noise_kernel_equals_its_restatement(geom, n):
    """Per list (every block, a sparse one that leaves the last workgroup partly filled, a single block) and per target (0, huge,
    one block's own b, the double below it): noise bit-equal, keep as the rule says, blk_spp = n for the listed blocks and
    untouched elsewhere.  decide = (n >= 2), the host's invariant; n = 1 gives +inf and keeps everything."""
    acc, m2, inside, all_bad = ap.block_noise_inputs(*geom, n)
    g5 = ap.geom5(*geom)
    decide = int(n >= 2)
    worst = 0.0
    for lname, active in ap.block_noise_lists(*geom).items():
        b = ap.block_noise_reference(acc, m2, active, n, decide, 0.0, inside)[2]
        fs = ap.block_noise_fsum(acc, m2, active, n, inside) if n >= 2 else None
        for target in ap.block_noise_targets(b):
            tag = (geom, n, lname, target)
            wspp, wkeep, wb = ap.block_noise_reference(acc, m2, active, n, decide, target, inside)
            spp, keep, noise = ap.block_noise(acc, m2, active, n, decide, target, g5)
            assert np.array_equal(bits(noise), bits(wb)), (tag, int(np.flatnonzero(bits(noise) != bits(wb))[0]))
            assert np.array_equal(keep, wkeep), tag
            assert np.array_equal(spp, wspp), tag  # n in the listed blocks, the sentinel everywhere else
            if n < 2:
                assert np.all(np.isposinf(noise)) and np.all(keep == 1), tag
                continue
            rel = np.abs(noise - fs) / np.where(fs > 0, fs, 1.0)
            assert np.all(rel <= ap.FSUM_BOUND) and np.all((fs > 0) | (noise == 0)), (tag, float(rel.max()))
            worst = max(worst, float(rel.max()))
            if all_bad is not None and all_bad in active.tolist():
                i = active.tolist().index(all_bad)
                assert noise[i] == 0.0 and keep[i] == 0, tag  # nothing but bad pixels: stops at any target >= 0
        if n >= 2:
            t = ap.block_noise_targets(b)
            assert len(t) == 4 and np.any(b == t[2])  # the equality case was there
    print("%dx%d shard %d of %d, n = %d: largest relative distance of b from fsum %.3g (bound %.3g)" % (*geom, n, worst, ap.FSUM_BOUND))
