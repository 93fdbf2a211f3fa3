"""The roulette step that reads the roulette table (csrc/pt_kernels.h: roulette_table_advance, and roulette_step's choice between it
and roulette_advance) on the MI355X, one lane per case (tests/roulette_probe.hip), on the full case table of
shade_probe_support.roulette_table(): depths above and inside the roulette range, attenuations around 1e-6 and 0.95, non-finite ones,
and the cases whose draw equals the survival probability or lies one ulp beside it.  Every case's record is built by the product's
roulette_record from its attenuation.  Reference: oracle.roulette_steps, the code rayColorOpt runs.  `finished`, the depth, T, the
stream state and both draw counters are compared on their bits (a NaN where the reference has a NaN), with the records read through
LDS and from global memory, STATS off and on, in two lane layouts, and once more with every third lane sent through roulette_advance
behind the wave's ballot."""
from __future__ import annotations

import numpy as np
import pytest

import roulette_probe_support as rp
import shade_probe_support as sp

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, scope="module")
def _probe(gpu_ctx):
    return rp.load()


@pytest.fixture(scope="module")
def reference(oracle):
    R = sp.roulette_table()
    ref = oracle.roulette_steps(R["depth"], R["att"], R["T"], R["state"])
    for a in ref.values():
        a.setflags(write=False)
    return R, ref


def _want(R, ref):
    ended = ref["ended"] != 0
    return dict(finished=ended.astype(np.int32), depth=np.where(np.isin(ref["ended"], (1, 2)), R["depth"], R["depth"] - 1).astype(np.int32),
                T=ref["T"], state=ref["state"], draws=ref["draws"].astype(np.int32))


def _differs(dev, ref):
    d = ~sp.same(dev, ref) if np.asarray(ref).dtype.kind == "f" else np.asarray(dev) != np.asarray(ref)
    return d.reshape(len(d), -1).any(axis=1)


def _run_all(R, ref, mixed):
    n = R["n"]
    want = _want(R, ref)
    key = ref["ended"] * 100 + np.minimum(R["depth"], 4)
    orders = dict(table=np.arange(n), sorted=np.argsort(key, kind="stable"))
    total = 0
    for stats in (False, True):
        for lds in (False, True):
            for name, o in orders.items():
                inv = np.empty(n, np.int64)
                inv[o] = np.arange(n)
                got = rp.gpu_table_step(R["depth"][o], R["att"][o], R["T"][o], R["state"][o], stats, lds, mixed)
                I, F, S = got["I"][inv], got["F"][inv], got["S"][inv]
                dev = dict(finished=I[:, 0], depth=I[:, 1], T=F, state=S, draws=I[:, 3])
                bad = np.zeros(n, bool)
                for k in want:
                    bad |= _differs(dev[k], want[k])
                bad |= I[:, 4] != (I[:, 3] if stats else 0)
                used = I[:, 2]
                assert used.min() == (0 if mixed else 1) and used.max() == 1
                print("roulette table step stats=%d lds=%d mixed=%d %s order: %d cases, %d without a record, differ %d"
                      % (stats, lds, mixed, name, n, int((used == 0).sum()), int(bad.sum())))
                for i in np.flatnonzero(bad)[:5]:
                    print("  case %d depth %d att %s T %s state %x: device %s | reference %s" % (
                        i, R["depth"][i], R["att"][i], R["T"][i], R["state"][i],
                        {k: (v[i] if v.dtype.kind != "f" else sp.bits(v[i])) for k, v in dev.items()},
                        {k: (v[i] if v.dtype.kind != "f" else sp.bits(v[i])) for k, v in want.items()}))
                total += int(bad.sum())
    return total


def test_every_class_of_the_table_is_reached(reference):
    R, ref = reference
    cl = sp.roulette_classes(R, ref)
    counts = {k: int(v.sum()) for k, v in cl.items()}
    print("roulette table: %d cases %s" % (R["n"], counts))
    assert set(counts) == set(sp.ROULETTE_CLASSES) and all(v > 0 for v in counts.values()), counts
    assert R["n"] % 64 != 0 and R["n"] > 4 * 256   # more than one block, a partly filled last wave


def test_table_step_matches_the_reference(reference):
    R, ref = reference
    assert _run_all(R, ref, mixed=False) == 0


def test_step_with_lanes_that_have_no_record_matches_the_reference(reference):
    R, ref = reference
    assert _run_all(R, ref, mixed=True) == 0
