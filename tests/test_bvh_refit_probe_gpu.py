"""T5: the product's refit kernels and level sequence (csrc/pt_bvh_refit.h through tests/bvh_refit_probe.hip) against the host build
of the same header (tests/bvh_refit_probe.cpp): nodes, object records, the exact boxes and the figure, byte for byte, on the cases of
test_bvh_refit_cpu.py -- among them level ranges that end in the middle of a wave and a tree of one object."""
import struct

import numpy as np
import pytest

import bvh_refit_support as rs

pytestmark = pytest.mark.gpu

CASES = [(n, d) for n in rs.SIZES for d in rs.DIELECTRICS]


def _same(dev, host, tag):
    assert np.array_equal(dev["nodes"], host["nodes"]), (tag, "nodes", int(np.count_nonzero(dev["nodes"] != host["nodes"])))
    assert np.array_equal(dev["objs"], host["objs"]), (tag, "records")
    assert dev["box"].tobytes() == host["box"].tobytes(), (tag, "node_box")
    assert dev["area"].tobytes() == host["area"].tobytes(), (tag, "a[q]")


def test_the_bit_routines_agree_with_the_host():
    """nextafterf on the bits, the conversion and the rounding of one axis, on the device and on the host."""
    rng = np.random.default_rng(4)
    n = 4096
    lo = np.concatenate([rng.uniform(-50, 50, n - 8), [np.nan, 0.0, -1e300, 0.0, -0.0, 1e-46, -3.4e38, 3.3e38]])
    hi = lo + np.concatenate([10.0 ** rng.uniform(-9, 3, n - 8), [1.0, np.inf, 2e300, 1.0, 0.0, 1e-46, 1.0, 1e37]])
    m = np.concatenate([10.0 ** rng.uniform(-5, 1, n - 8), [0.1, 0.1, 0.1, np.inf, 1e-46, 0.0, 1e30, 1e36]])
    arg = np.ascontiguousarray(np.stack([lo, hi, m], axis=1))
    out = np.zeros((n, 4), np.uint32)
    assert rs.gpu().rpg_bits(rs.ptr(arg), rs.ptr(out), n) == 0
    L = rs.host()
    two = (rs.C.c_uint32 * 2)()
    for i in range(n):
        L.rp_encode_axis(float(lo[i]), float(hi[i]), float(m[i]), two)
        want = (two[0], two[1], L.rp_h_word(two[1], i & 255), L.rp_next_up(two[0]))
        assert tuple(int(v) for v in out[i]) == want, (i, lo[i], hi[i], m[i])


@pytest.mark.parametrize("n,ndiel", CASES)
def test_t5_the_device_refit_equals_the_host_restatement(n, ndiel):
    w = rs.world_of(n, ndiel)
    t = rs.Tree(w)
    built = t.state()
    counts = np.diff(built["levels"])
    if n >= 300:  # a level range that is no multiple of 16 nodes ends in the middle of a wave
        assert np.any(counts % 16 != 0)
    # the world unchanged: the built bytes
    cost = t.refit(w)
    host = t.state()
    dev = rs.gpu_refit(built, w, t.margin, t.main_nodes)
    _same(dev, host, "unchanged")
    assert np.array_equal(dev["nodes"], t.built)
    assert struct.pack("<d", dev["cost"]) == struct.pack("<d", cost)
    # every move, each from the state the one before left on the device (nothing accumulates: the host refits from its own)
    state = dev
    for name, wm in rs.moves(w):
        cost = t.refit(wm)
        host = t.state()
        state = rs.gpu_refit(state, wm, t.margin, t.main_nodes)
        _same(state, host, name)
        assert struct.pack("<d", state["cost"]) == struct.pack("<d", cost), name
        assert t.check(wm) == dict(objects_outside=0, children_outside=0, bytes_differ=0, topology_changed=0, records_differ=0), name
    t.close()


def test_t5_the_device_refit_equals_the_host_restatement_after_every_resize():
    """The edits that are no translations (rs.resizes: radius, radius_sq and inv_radius change in the records the device copies, box
    extents, negative and zero radii, the dielectrics of the second tree), each from the state the one before left on the device."""
    w = rs.world_of(300, 7)
    t = rs.Tree(w)
    assert t.n_objs == t.main_objs + 7
    state = t.state()
    built_objs = state["objs"].copy()
    figures = []
    for name, wm in rs.resizes(w):
        cost = t.refit(wm)
        host = t.state()
        state = rs.gpu_refit(state, wm, t.margin, t.main_nodes)
        _same(state, host, name)
        assert struct.pack("<d", state["cost"]) == struct.pack("<d", cost), (name, state["cost"], cost)
        assert t.check(wm) == dict(objects_outside=0, children_outside=0, bytes_differ=0, topology_changed=0, records_differ=0), name
        changed = (state["objs"].reshape(-1, rs.OBJ_BYTES) != built_objs.reshape(-1, rs.OBJ_BYTES)).any(axis=1)
        figures.append(cost)
        print("refit probe, %-34s figure %.6f, %d of %d records changed" % (name, cost, int(changed.sum()), len(changed)))
    assert np.array_equal(state["nodes"], t.built) and np.array_equal(state["objs"], built_objs)
    assert figures[0] > figures[-1] > figures[1]  # grown > built > shrunk
    t.close()


def test_t5_a_tree_of_more_than_one_cost_block():
    """20 000 objects: more than 4096 nodes, so the figure adds block sums."""
    w = rs.world_of(20000, 7)
    t = rs.Tree(w)
    assert t.main_nodes > 4096
    built = t.state()
    name, wm = next(iter(rs.moves(w)))
    cost = t.refit(wm)
    dev = rs.gpu_refit(built, wm, t.margin, t.main_nodes)
    _same(dev, t.state(), name)
    assert struct.pack("<d", dev["cost"]) == struct.pack("<d", cost)
    t.close()
