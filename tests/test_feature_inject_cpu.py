"""The injected-ray tables of feature_inject_support.py hold what test_feature_inject_gpu.py needs of them (no GPU): the walk's
predicate gives the counts the tables were laid out for, walk_layout is a stable partition that leaves at most one mixed wave, every
class has whole waves for the walk to take, and -- through the oracle alone -- every table holds hits, misses and rays whose winner
is tied with another object, and every record with a NaN or an infinity belongs to an odd ray."""
import numpy as np
import pytest

import feature_inject_support as fi
import ray_inject_support as S

# odd rays, and waves holding one, of the tables in ray_inject_support's layout
ODD_TODAY = {"length": (3999, 63), "components": (470, 62), "near geometry": (0, 0), "far origins": (2626, 45), "incoherent": (0, 0),
             "mixed": (560, 64), fi.NAMED: (0, 0)}


def test_the_predicate_is_the_walks():
    B = S.BOUND
    ok = [0.1, 2.0, -3.0, 0.0, 0.0, 1.0]

    def odd(**kw):
        r = np.array(ok, float)
        for k, v in kw.items():
            r[int(k[1:])] = v
        return bool(fi.walk_odd(r[None, :])[0])

    assert not odd()
    # a = d.d strictly inside (1e-29, 1e29)
    assert odd(c5=np.sqrt(1e-29) * (1 - 1e-9)) and not odd(c5=np.sqrt(1e-29) * (1 + 1e-9))
    assert odd(c5=np.sqrt(1e29) * (1 + 1e-9)) and not odd(c5=np.sqrt(1e29) * (1 - 1e-9))
    assert odd(c5=0.0) and odd(c5=1e200) and odd(c5=1e-200) and odd(c5=np.inf) and odd(c5=np.nan) and odd(c3=np.nan)
    # zero and denormal components next to an ordinary one are NOT odd: these are the rays the walk must see
    assert not odd(c3=0.0, c4=-0.0) and not odd(c3=5e-324, c4=-5e-324)
    # the origin: every |component| <= 3.5 B, the bound included
    for c in ("c0", "c1", "c2"):
        assert not odd(**{c: 3.5 * B}) and not odd(**{c: -3.5 * B}) and odd(**{c: np.nextafter(3.5 * B, np.inf)}) and odd(**{c: -4.0 * B})
        assert odd(**{c: np.nan}) and odd(**{c: np.inf}) and odd(**{c: -np.inf})
    assert not fi.walk_odd(np.array([ok]), bound=1.0)[0] and fi.walk_odd(np.array([ok]), bound=0.5)[0]  # 3 <= 3.5, 3 > 1.75


def test_the_tables_as_they_are_keep_the_degenerate_rays_off_the_walk():
    t = fi.tables()
    assert tuple(t) == fi.CLASS_NAMES
    for name, table in t.items():
        odd = fi.walk_odd(table)
        assert (int(odd.sum()), fi.odd_waves(table)) == ODD_TODAY[name], (name, int(odd.sum()), fi.odd_waves(table))
        assert fi.laid_out(name, "original")[1] == ODD_TODAY[name][1]
    # the components class: the rays with a zero or denormal component sit in waves that hold an odd ray, nearly all of them
    c = t["components"]
    degenerate = (np.abs(c[:, 3:6]) < 2.0 ** -1022).any(axis=1) & ~fi.walk_odd(c)
    wv = S.waves_of_table(c)
    in_odd_wave = np.isin(wv, np.unique(wv[fi.walk_odd(c)]))
    assert degenerate.sum() > 2000 and np.count_nonzero(degenerate & ~in_odd_wave) < 0.05 * degenerate.sum()


@pytest.mark.parametrize("name", fi.CLASS_NAMES)
def test_walk_layout_is_a_stable_partition_with_one_mixed_wave_at_most(name):
    src = fi.tables()[name]
    table, plain = fi.walk_layout(src)
    assert table.shape == (S.W * S.H, 6) and table.dtype == np.float64
    # back to wave order: row k = lane k % 64 of wave k // 64
    ys, xs = np.mgrid[0:S.H, 0:S.W]
    pos = (S.wave_of(xs, ys) * 64 + S.lane_of(xs, ys)).reshape(-1)
    seq = np.zeros_like(table)
    seq[pos] = table
    odd = fi.walk_odd(seq)
    n_ok = int(np.count_nonzero(~odd))
    assert not odd[:n_ok].any() and odd[n_ok:].all()
    src_odd = fi.walk_odd(src)
    assert seq[:n_ok].tobytes() == src[~src_odd].tobytes() and seq[n_ok:].tobytes() == src[src_odd].tobytes()  # stable, nothing lost
    per_wave = odd.reshape(S.NWAVES, 64).sum(axis=1)
    assert np.count_nonzero((per_wave > 0) & (per_wave < 64)) <= 1
    assert plain == int(np.count_nonzero(per_wave > 0)) == S.NWAVES - n_ok // 64
    assert S.NWAVES - plain >= fi.MIN_WALKED[name], (name, S.NWAVES - plain)
    assert n_ok // 64 == S.NWAVES - (ODD_TODAY[name][0] + 63) // 64
    assert fi.laid_out(name, "walk")[1] == plain and fi.laid_out(name, "walk")[0].tobytes() == table.tobytes()


def test_the_degenerate_component_rays_are_walked_after_the_layout():
    table, plain = fi.laid_out("components", "walk")
    wv = S.waves_of_table(table)
    walked = ~np.isin(wv, np.unique(wv[fi.walk_odd(table)]))
    d = table[:, 3:6]
    assert np.count_nonzero(walked & (d == 0).any(axis=1)) >= 1000             # infinite FP32 reciprocals, NaN slab parameters
    assert np.count_nonzero(walked & ((d != 0) & (np.abs(d) < 2.0 ** -1022)).any(axis=1)) >= 500  # denormal: flushed or infinite
    assert np.count_nonzero(walked & (np.count_nonzero(d, axis=1) == 1)) >= 256  # exactly axis-parallel


@pytest.mark.parametrize("name", fi.CLASS_NAMES)
def test_the_oracles_records_hold_hits_misses_and_ties(oracle, name):
    osc = fi.ora_scene(S.scene_doc("bvh"), key="bvh")
    for layout in fi.LAYOUTS:
        table, _ = fi.laid_out(name, layout)
        o = fi.oracle_records(osc, table, key=("bvh", name, layout))
        hits = int(np.count_nonzero(o["rec"][:, 0]))
        assert 0 < hits < len(table), (name, layout, hits)
        assert np.array_equal(o["rec"][:, 0] != 0, o["ids"] >= 0)  # the two restatements agree on what is hit
        ties = int(np.count_nonzero(o["tie"]))
        assert ties > 0 or name == fi.NAMED, (name, layout, ties)
        # a record with a NaN or an infinity comes from an odd ray, which the walk never takes
        assert not np.any(o["nonfinite"] & ~fi.walk_odd(table)), (name, layout)
        print("%-14s %-8s: %d hits, %d ties, %d non-finite records" % (name, layout, hits, ties, int(o["nonfinite"].sum())))
    a, b = (fi.oracle_records(osc, fi.laid_out(name, lay)[0], key=("bvh", name, lay)) for lay in fi.LAYOUTS)
    assert sorted(a["ids"].tolist()) == sorted(b["ids"].tolist())  # the same rays in another order


def test_the_named_table_holds_the_named_rays_and_their_reverses(oracle):
    """S.NAMED_RAYS all hit (that is what they are kept for), so on their own they would never show a walk that invents a hit."""
    osc = fi.ora_scene(S.scene_doc("bvh"), key="bvh")
    named = np.array(S.NAMED_RAYS[fi.NAMED], float)
    table = fi.tables()[fi.NAMED]
    rows = {r.tobytes() for r in table}
    assert len(rows) == 8 and all(r.tobytes() in rows for r in named)
    ids = fi.oracle_records(osc, table, key=("bvh", fi.NAMED, "original"))["ids"]
    is_named = np.array([r.tobytes() in {q.tobytes() for q in named} for r in table])
    assert np.all(ids[is_named] >= 0) and np.all(ids[~is_named] < 0) and is_named.sum() == len(table) // 2
    assert len(np.unique(ids[is_named])) == 4


def test_expected_planes_add_the_samples_in_order():
    rec = np.zeros((2 * 1 * 3, 8))
    rec[0] = [1, 0.1, 0.2, 0.3, 0.5, 0.5, 0.5, 1e16]
    rec[1] = [0, 9, 9, 9, 9, 9, 9, 9]  # a miss adds nothing but the sample
    rec[2] = [1, 0.7, -0.2, 0.0, 0.25, 0.5, 1.0, 1.0]
    rec[3] = [1, -0.0, 0.0, -1.0, 0.0, 0.0, 0.0, np.inf]
    n, a, d = fi.expected_planes(rec, 2, 1, 3)
    assert n[0, 0].tolist() == [0.1 + 0.7, 0.2 + -0.2, 0.3 + 0.0] and a[0, 0].tolist() == [0.75, 1.0, 1.5]
    assert d[0, 0].tolist() == [1e16 + 1.0, 2.0, 3.0] and d[0, 0, 0] == 1e16  # FP64, in order
    assert n[0, 1].tolist() == [0.0, 0.0, -1.0] and not np.signbit(n[0, 1, 0]) and d[0, 1].tolist() == [np.inf, 1.0, 3.0]
