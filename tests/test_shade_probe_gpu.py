"""The surface step of the trace kernels on the MI355X, one lane per case (tests/shade_probe.hip): shade_hit in its four
instantiations, outward_normal, reflect_vec, glass_kernel's own sequence, exit_post and roulette_advance against the oracle's step
functions -- the code rayColorOpt runs -- on the tables of shade_probe_support.py.  Everything is compared on the uint64 view, a NaN
where the reference has a NaN, no tolerance anywhere.  Every table runs in two lane layouts (table order: neighbouring lanes differ
in material type and branch; sorted by type and branch: whole waves are coherent, as in glass_kernel), which must agree bit for
bit, lane by lane, and with the material table in LDS and in global memory.  That the tables reach what they are meant to reach is
asserted in test_shade_probe_cpu.py, on the reference alone."""
from __future__ import annotations

import numpy as np
import pytest

import shade_probe_support as sp

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, scope="module")
def _probe(gpu_ctx):
    return sp.load()


def _hex(x):
    return " ".join("%016x" % v for v in np.atleast_1d(sp.bits(x)).ravel())


def _report(what, bad, operands, dev, ref):
    """The first five cases that differ: operands, device bits, reference bits."""
    for i in np.flatnonzero(bad)[:5]:
        print("  %s case %d" % (what, i))
        for k, v in operands.items():
            print("    %-8s %s" % (k, v[i] if v[i].dtype.kind != "f" else "%s  [%s]" % (v[i], _hex(v[i]))))
        for k in dev:
            print("    %-8s device %s | reference %s" % (k, _hex(dev[k][i]) if dev[k].dtype.kind == "f" else dev[k][i],
                                                      _hex(ref[k][i]) if ref[k].dtype.kind == "f" else ref[k][i]))


def _differs(dev, ref, where=None):
    """bool [n]: a row of dev differs from ref (floats: sp.same; integers: equality), only where `where` says the item is defined."""
    d = ~sp.same(dev, ref) if np.asarray(ref).dtype.kind == "f" else np.asarray(dev) != np.asarray(ref)
    d = d.reshape(len(d), -1).any(axis=1)
    return d if where is None else d & where


def _both_layouts(n, key, run):
    """run(order) in table order and sorted by key; the sorted run is brought back to table order and must equal the other bit for
    bit, lane by lane.  Returns the table-order result."""
    lay = sp.layouts(n, key)
    a = run(lay["table"])
    b = run(lay["sorted"])
    inv = np.empty(n, np.int64)
    inv[lay["sorted"]] = np.arange(n)
    for k in a:
        x, y = a[k], b[k][inv]
        assert np.array_equal(x.view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), "the lane layouts disagree on " + k
    return a


def _shade_reference(T, ref):
    ok = ref["ok"] != 0
    diel = T["typ"] == sp.DIELECTRIC
    return dict(finished=(~ok).astype(np.int32), exit=(ok & diel & ref["front"]).astype(np.int32), term=ref["out"][:, 0:3],
                att=ref["out"][:, 3:6], origin=ref["out"][:, 6:9], dir=ref["out"][:, 9:12], state=ref["state"],
                draws=ref["draws"].astype(np.int32)), ok


def _check_shade(what, T, sel, stats, glass, sequence=False):
    """The cases `sel` of the table through shade_hit<stats, glass> (or glass_kernel's sequence): both layouts, LDS and global."""
    M, ref = sp.materials(), sp.reference()
    want, ok = _shade_reference(T, ref)
    want, ok = {k: v[sel] for k, v in want.items()}, ok[sel]
    n = len(sel)
    assert n % 64 != 0
    key = T["typ"][sel] * 16 + ref["branch"][sel]
    total = 0
    for lds in ((True,) if sequence else (True, False)):
        def run(order):
            i = sel[order]
            return sp.gpu_shade(M["arr"], T["objs"][i], T["t"][i], T["ray"][i], T["state"][i], stats, glass, lds, sequence)

        got = _both_layouts(n, key, run)
        I, F = got["I"], got["F"]
        dev = dict(finished=I[:, 0], exit=I[:, 1], term=F[:, 0:3], att=F[:, 3:6], origin=F[:, 6:9], dir=F[:, 9:12], state=got["S"],
                   draws=I[:, 3])
        bad = np.zeros(n, bool)
        for k in ("finished", "exit", "state", "draws"):
            bad |= _differs(dev[k], want[k])
        bad |= _differs(dev["term"], want["term"], ~ok)   # the path ends with `emitted`
        for k in ("att", "origin", "dir"):                # the scattered ray, where there is one
            bad |= _differs(dev[k], want[k], ok)
        bad |= (I[:, 2] != np.where(want["exit"] != 0, T["mat"][sel], -1)) if not sequence else (I[:, 2] != T["mat"][sel])
        bad |= I[:, 4] != (I[:, 3] if stats else 0)       # j_draw follows c_draw in the STATS builds only
        count = {name: int((ref["branch"][sel] == b).sum()) for b, name in enumerate(sp.BRANCHES)}
        print("%s stats=%d %s: %d cases %s, differ %d" % (what, stats, "LDS" if lds else "global", n, {k: v for k, v in count.items() if v},
                                                          bad.sum()))
        if bad.any():
            _report(what, bad, dict(object=T["objs"][sel], t=T["t"][sel], ray=T["ray"][sel], state=T["state"][sel]), dev, want)
        total += int(bad.sum())
    return total


def test_shade_hit_with_glass_matches_the_reference():
    T = sp.cases()
    sel = np.arange(T["n"])
    assert sum(_check_shade("shade_hit<GLASS>", T, sel, stats, True) for stats in (False, True)) == 0


def test_shade_hit_without_glass_matches_the_reference():
    T = sp.cases()
    sel = np.flatnonzero(T["typ"] != sp.DIELECTRIC)   # its callers never pass a dielectric hit
    if len(sel) % 64 == 0:
        sel = sel[:-1]
    assert sum(_check_shade("shade_hit<!GLASS>", T, sel, stats, False) for stats in (False, True)) == 0


def test_glass_kernel_sequence_matches_the_reference():
    T = sp.cases()
    sel = np.flatnonzero(T["typ"] == sp.DIELECTRIC)
    if len(sel) % 64 == 0:
        sel = sel[:-1]
    assert sum(_check_shade("glass sequence", T, sel, stats, True, sequence=True) for stats in (False, True)) == 0


def test_outward_normal_and_reflect_vec_match_the_reference(oracle):
    T = sp.cases()
    n = T["n"]
    front = T["hit"][:, 7] != 0
    want = np.where(front[:, None], T["hit"][:, 4:7], -T["hit"][:, 4:7])   # setFaceNormal negates on a back face (objects.go:17-24)
    got = _both_layouts(n, T["kind"] * 2 + front, lambda o: dict(n=sp.gpu_normal(T["objs"][o], T["hit"][o, 1:4])))["n"]
    bad = _differs(got, want)
    print("outward_normal: %d cases %s, differ %d" % (n, {k: int((T["kind"] == v).sum()) for k, v in (("sphere", 0), ("plane", 1), ("box", 2))},
                                                      bad.sum()))
    if bad.any():
        _report("outward_normal", bad, dict(object=T["objs"], p=T["hit"][:, 1:4]), dict(n=got), dict(n=want))
    v, nrm = sp.reflect_table()
    wantr = oracle.reflects(v, nrm)
    gotr = _both_layouts(len(v), np.isnan(wantr).any(axis=1), lambda o: dict(r=sp.gpu_reflect(v[o], nrm[o])))["r"]
    badr = _differs(gotr, wantr)
    print("reflect_vec: %d cases, %d with a NaN, %d with an infinity, differ %d"
          % (len(v), np.isnan(wantr).any(axis=1).sum(), np.isinf(wantr).any(axis=1).sum(), badr.sum()))
    if badr.any():
        _report("reflect_vec", badr, dict(v=v, n=nrm), dict(r=gotr), dict(r=wantr))
    assert bad.sum() == 0 and badr.sum() == 0


def test_exit_post_matches_the_reference(oracle):
    E, M = sp.exit_table(), sp.materials()
    n = E["n"]
    want_att, want_o = oracle.exit_steps(M["arr"], E["mat"], E["ray"], E["tmax"], E["best"], E["att"])

    def run(o):
        att, org = sp.gpu_exit(M["arr"], E["mat"][o], E["best"][o], E["tmax"][o], E["ray"][o], E["att"][o])
        return dict(att=np.ascontiguousarray(att), origin=np.ascontiguousarray(org))

    got = _both_layouts(n, (E["best"] >= 0) * 1000 + E["mat"], run)
    bad = _differs(got["att"], want_att) | _differs(got["origin"], want_o)
    print("exit_post: %d cases, no exit %d, absorbing %d, differ %d"
          % (n, (E["best"] < 0).sum(), ((E["best"] >= 0) & np.any(want_att != 1.0, axis=1)).sum(), bad.sum()))
    if bad.any():
        _report("exit_post", bad, dict(mat=E["mat"], best=E["best"], tmax=E["tmax"], ray=E["ray"]), got, dict(att=want_att, origin=want_o))
    assert bad.sum() == 0


def test_roulette_advance_matches_the_reference(oracle):
    R = sp.roulette_table()
    n = R["n"]
    ref = oracle.roulette_steps(R["depth"], R["att"], R["T"], R["state"])
    cl = sp.roulette_classes(R, ref)
    ended = ref["ended"] != 0
    want = dict(finished=ended.astype(np.int32), depth=np.where(np.isin(ref["ended"], (1, 2)), R["depth"], R["depth"] - 1).astype(np.int32),
                T=ref["T"], state=ref["state"], draws=ref["draws"].astype(np.int32))
    total = 0
    for stats in (False, True):
        def run(o):
            return sp.gpu_roulette(R["depth"][o], R["att"][o], R["T"][o], R["state"][o], stats)

        got = _both_layouts(n, ref["ended"] * 100 + np.minimum(R["depth"], 4), run)
        I = got["I"]
        dev = dict(finished=I[:, 0], depth=I[:, 1], T=got["F"], state=got["S"], draws=I[:, 3])
        bad = np.zeros(n, bool)
        for k in want:   # T: the product T * att formed in C for a path that goes on, untouched for one the roulette ended
            bad |= _differs(dev[k], want[k])
        bad |= I[:, 4] != (I[:, 3] if stats else 0)
        print("roulette_advance stats=%d: %d cases %s, differ %d" % (stats, n, {k: int(v.sum()) for k, v in cl.items()}, bad.sum()))
        if bad.any():
            _report("roulette_advance", bad, dict(depth=R["depth"], att=R["att"], T=R["T"], state=R["state"]), dev, want)
        total += int(bad.sum())
    assert total == 0
