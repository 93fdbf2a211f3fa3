"""The roulette table's host builder (csrc/pt_convert.h: roulette_record, roulette_table) against the oracle's own roulette step, on
any machine: a stand-alone g++ -ffp-contract=off build of the header (tests/roulette_table_probe.cpp) over the attenuation triples of
the surface-step probe's roulette table and the edge values the table must get right (-0.0, 1e-6 and 0.95 with their neighbours, a
denormal, infinities, a NaN in each position).  Reference: oracle.roulette_steps at depth 3 with T = (1, 1, 1), so that a
survivor's T is the divided attenuation itself.  Bit for bit, a NaN where the reference has a NaN; no tolerance."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import roulette_probe_support as rp
import shade_probe_support as sp


@pytest.fixture(scope="module")
def host_exe():
    return rp.build_host()


@pytest.fixture(scope="module")
def table(host_exe):
    t = rp.triples()
    rec, tab = rp.run_host(host_exe, t["att"])
    return t, rec, tab


def _draws(oracle, states):
    L = oracle.lib()
    return np.array([L.ora_stream_next(C.byref(C.c_uint64(int(s)))) for s in states])


def test_triples_hold_what_the_issue_lists():
    t = rp.triples()
    a = t["att"]
    R = sp.roulette_table()
    have = {sp.bits(x).tobytes() for x in a}
    assert {sp.bits(x).tobytes() for x in R["att"]} <= have
    flat = sp.bits(a).ravel()
    for v in (-0.0, 1e-6, sp.down(1e-6), sp.up(1e-6), 0.95, sp.down(0.95), sp.up(0.95), 5e-324):
        assert (flat == sp.bits(np.array([v]))[0]).any(), v
    inf, nan = np.isinf(a) & (a > 0), np.isnan(a)
    assert (inf.sum(axis=1) == 1).any() and inf.all(axis=1).any()
    assert all((nan[:, k] & (nan.sum(axis=1) == 1)).any() for k in range(3))
    assert t["at_prob"].sum() >= 440 and (t["state"] == rp.SURVIVOR_STATE).sum() == len(a) // 2


def test_records_equal_the_reference_step_at_depth_three(oracle, table):
    t, rec, _ = table
    n = len(t["att"])
    ref = oracle.roulette_steps(np.full(n, 3, np.int32), t["att"], np.ones((n, 3)), t["state"])
    prob, q = rec[:, 0], rec[:, 1:4]
    ended_rec = sp.bits(prob) == sp.bits(np.array([rp.ENDED]))[0]
    # ended without a draw <=> the record says so, and then nothing was drawn
    assert np.array_equal(ref["ended"] == 1, ended_rec)
    assert np.all(ref["draws"][ended_rec] == 0) and np.all(ref["draws"][~ended_rec] == 1)
    # the draw against the stored probability decides like the reference's (xi > NaN is false, as there)
    xi = _draws(oracle, t["state"])
    with np.errstate(invalid="ignore"):
        dies = ~ended_rec & (xi > prob)
    assert np.array_equal(ref["ended"] == 2, dies)
    # a survivor's T = 1 * (att / rrProb): the stored quotients
    alive = ~ended_rec & ~dies
    assert np.array_equal(ref["ended"] == 0, alive)
    bad = ~sp.same(q[alive], ref["T"][alive]).all(axis=1)
    print("roulette_record: %d triples, %d ended, %d die at the draw, %d survive; quotients that differ: %d"
          % (n, ended_rec.sum(), dies.sum(), alive.sum(), bad.sum()))
    assert bad.sum() == 0
    # every triple survives once (its SURVIVOR_STATE twin), so every stored quotient was compared
    surv = t["state"] == rp.SURVIVOR_STATE
    assert np.array_equal(alive[surv], ~ended_rec[surv])
    assert np.isnan(prob).any() and (prob == 0.95).any() and ((prob > 1e-6) & (prob < 0.95)).any() and (prob == 1e-6).any()


def test_probability_is_exact_at_the_draw(oracle, table):
    """The draw-at-probability cases: the attenuation's maximum is the case's own next draw, or one ulp to either side.  The record's
    probability is that maximum itself, and the reference ends exactly the cases whose maximum is one ulp below the draw."""
    t, rec, _ = table
    sel = t["at_prob"]
    xi = _draws(oracle, t["state"][sel])
    mx = t["att"][sel].max(axis=1)
    prob = rec[sel, 0]
    small = mx < 1e-6
    assert np.array_equal(sp.bits(prob[~small]), sp.bits(np.minimum(mx[~small], 0.95)))
    ref = oracle.roulette_steps(np.full(sel.sum(), 3, np.int32), t["att"][sel], np.ones((sel.sum(), 3)), t["state"][sel])
    below = (mx < xi) & ~small & (mx < 0.95)
    assert below.sum() > 100 and (mx == xi).sum() > 100 and (mx > xi).sum() > 100
    assert np.array_equal(ref["ended"] == 2, (xi > prob) & ~small) and np.all((ref["ended"] == 2)[below])


def test_table_has_one_record_per_material_and_the_unit_record(table):
    t, rec, tab = table
    assert tab.shape == (4, 4)
    assert np.array_equal(sp.bits(tab[:3]), sp.bits(rec[:3]))
    unit = np.array([0.95, 1.0 / 0.95, 1.0 / 0.95, 1.0 / 0.95])
    assert np.array_equal(sp.bits(tab[3]), sp.bits(unit))


def test_probe_is_clean_under_asan_and_ubsan(table):
    """Host code on the CPU: the same program once more with the sanitizers, run stand-alone."""
    t, rec, tab = table
    exe = rp.build_host(["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "roulette_table_probe_san")
    rec2, tab2 = rp.run_host(exe, t["att"])
    assert np.array_equal(sp.bits(rec), sp.bits(rec2)) and np.array_equal(sp.bits(tab), sp.bits(tab2))
