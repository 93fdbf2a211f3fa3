"""What the frames of test_edge_materials_gpu.py must be for that test to mean something, checked with the oracle alone.
conftest.render_vs_oracle accepts equal NaNs but not equal infinities (inf - inf), so every sum must be finite or NaN -- infinities
are the probe's business, which compares them bit for bit -- and the edge materials must really be on the paths: every set makes
exit scans, and draws at least 10 % more or fewer random numbers than the same scene with everyday materials."""
from __future__ import annotations

import numpy as np
import pytest

import edge_materials_support as em


@pytest.mark.parametrize("large", [False, True], ids=["small", "large"])
def test_edge_material_frames_are_comparable_and_differ_from_ordinary_ones(oracle, large):
    base = em.oracle_frame(oracle, "ordinary", large)
    assert np.isfinite(base["accum"]).all()
    for name in em.SET_NAMES:
        o = em.oracle_frame(oracle, name, large)
        acc = o["accum"]
        assert not np.isinf(acc).any(), name
        st = o["stats"]
        change = st["draws"] / base["stats"]["draws"] - 1.0
        print("%-10s %s: segments %d exit scans %d draws %d (%+.0f %% against ordinary materials), NaN sums %d"
              % (name, "large" if large else "small", st["segments"], st["exit_scans"], st["draws"], 100 * change, np.isnan(acc).sum()))
        assert st["exit_scans"] >= 1, name
        assert abs(change) >= 0.10, (name, change)
    assert np.isnan(em.oracle_frame(oracle, em.NONFINITE, large)["accum"]).any()


def test_scenes_take_the_paths_they_are_meant_for():
    assert len(em.objects(False)) == 7 and len(em.objects(True)) == 147   # beyond 128 spheres: the hierarchy
    assert len(em.SET_NAMES) == 7
    for name in em.SETS:
        assert set(em.SETS[name]) == set(em.SLOTS), name
