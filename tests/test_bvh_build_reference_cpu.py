"""R1 - R3: the host restatement of the device BVH build (csrc/pt_bvh_build.h through tests/bvh_build_probe.cpp) against
tests/bvh_build_reference.py, a statement of the same build that shares no code with it: Morton keys bit by bit, a stable argsort, a
top-down radix tree over key << 32 | position, boxes by range reduction, a breadth-first collapse on lists.  Every comparison is
exact.  R1: every world of B2 and every world added for the boundaries of the kernels (bvh_build_support.NEW_CASE_NAMES).  R2: what
each new world is chosen for, so that an edit to a world cannot make its case vacuous.  R3: the two deep scenes of
test_bvh_build_edges_gpu.py keep those conditions with their large spheres, and the oracle sees the spheres.  No GPU.

bvh_build_support.DEEP_TIES = 26 is the smallest number of equal keys in front of the chain of deep_keys() for which the
Morton-order tree needs PT_BVH_STACK = 96 entries or more (found with bs.Trees(...).fits; 1 ... 25 give 89 ... 95, 26 gives 96)."""
from __future__ import annotations

import math

import numpy as np
import pytest

import bvh_build_reference as ref
import bvh_build_support as bs
from fog_support import ptr

ALL_NAMES = bs.CASE_NAMES + bs.NEW_CASE_NAMES


def reference(name: str):
    """(main tree, dielectric tree) of a named world by the reference, computed once."""
    return ref.build_once(name, bs.case_world(name))


def assert_tree_equals_reference(got: dict, want: dict, tag):
    assert ref.differences(got, want) == [], tag


# ---------------------------------------------------------------- R1
@pytest.mark.parametrize("name", ALL_NAMES)
def test_r1_host_restatement_equals_the_reference(name):
    w = bs.case_world(name)
    t = bs.Trees(w)
    main, glass = ref.build_once(name, w)
    assert_tree_equals_reference(t.tree(0), main, (name, "main"))
    assert_tree_equals_reference(t.tree(1), glass, (name, "dielectric"))
    assert (t.main_nodes, t.main_objs, t.n_nodes, t.n_objs) == (main["n_nodes"], main["n"], main["n_nodes"] + glass["n_nodes"], main["n"] + glass["n"])
    assert t.depth == max(main["depth"], glass["depth"]), name
    assert t.stack_need == max(main["stack_need"], glass["stack_need"]), name
    assert t.fits == (t.stack_need < bs.PT_BVH_STACK)
    t.close()


def test_r1_the_reference_tree_is_a_tree():
    """The reference's own invariants on one world with ties: every node but the root has one parent, a node's range is its
    children's ranges side by side, and the ranges of the leaves are the positions."""
    m = reference("duplicates over the seams")[0]
    n = m["n"]
    assert m["parent"][0] == -1 and np.count_nonzero(m["parent"] < 0) == 1
    assert sorted(m["child"].ravel().tolist()) == list(range(1, 2 * n - 1))
    l, r = m["child"][:, 0], m["child"][:, 1]
    assert np.array_equal(m["first"][:n - 1], m["first"][l]) and np.array_equal(m["last"][:n - 1], m["last"][r])
    assert np.array_equal(m["last"][l] + 1, m["first"][r])
    assert sorted(m["order"].tolist()) == list(range(n))


# ---------------------------------------------------------------- R2
def tiles_of(positions, tile=1024):
    return set((np.asarray(positions) // tile).tolist())


def test_r2_the_boundary_sizes_sit_on_the_boundaries():
    assert {255, 256, 257} <= set(bs.BOUNDARY_SIZES)  # a block of 256 lanes
    assert {1023, 1024, 1025} <= set(bs.BOUNDARY_SIZES)  # a sort, scan and reduction tile of 1024
    assert {4095, 4096, 4097} <= set(bs.BOUNDARY_SIZES)  # a sort block of four tiles
    fifth = [n for n in bs.BOUNDARY_SIZES if -(-n // 1024) == 5]
    assert fifth and all(256 * -(-n // 1024) > 1024 for n in fifth) and 256 * 4 <= 1024  # the [digit][tile] table: two scan blocks from the fifth tile on
    for n in bs.BOUNDARY_SIZES:
        w = bs.case_world("n=%d diel=7" % n)
        assert len(w) == n and np.count_nonzero(w["kind"] & 0x100) == 7


def test_r2_one_centroid_is_the_tie_breaks_alone():
    w = bs.case_world("one centroid, 5000")
    m = reference("one centroid, 5000")[0]
    assert m["n"] == 5000 and len(np.unique(m["keys"])) == 1
    assert np.array_equal(m["sorted"], np.arange(5000))  # ties stay in position order, over five tiles and two sort blocks
    assert m["depth"] <= math.ceil(math.log2(5000)) == 13  # balanced by position up to position 4999
    t = bs.Trees(w)
    assert t.depth <= 13 and t.fits
    t.close()


def test_r2_a_line_has_few_digits_per_pass():
    keys = reference("a line, 5000")[0]["keys"]
    assert len(keys) == 5000 and len(np.unique(keys)) == 5000  # distinct keys ...
    # ... whose bits are those of one axis: a digit of 8 key bits holds 2 or 3 of them, so a pass sees at most 8 digits of 256
    assert all(len(np.unique((keys >> np.uint64(8 * p)) & np.uint64(255))) <= 8 for p in range(8))


def test_r2_three_centroids_fill_every_tile_and_come_out_as_three_progressions():
    w = bs.case_world("three centroids interleaved, 4500")
    lo, hi = ref.object_boxes(w)
    keys = ref.keys_of(ref.centroids(lo, hi))  # in position order
    m = reference("three centroids interleaved, 4500")[0]
    assert len(np.unique(keys)) == 3
    for key in np.unique(keys):
        at = np.flatnonzero(keys == key)
        assert tiles_of(at) == {0, 1, 2, 3, 4} and tiles_of(at, 4096) == {0, 1}  # the key enters from every tile and both sort blocks
        run = np.flatnonzero(m["keys"] == key)
        assert len(run) == 1500 and len(tiles_of(run)) >= 2  # its run of the output spans tiles
    assert tiles_of(np.flatnonzero(m["keys"] == m["keys"][-1]), 4096) == {0, 1}  # ... and the last run both sort blocks
    assert np.array_equal(m["sorted"], np.concatenate([np.arange(2, 4500, 3), np.arange(0, 4500, 3), np.arange(1, 4500, 3)]))


def test_r2_the_duplicates_lie_over_the_seams():
    w = bs.case_world("duplicates over the seams")
    copies = np.array(bs.SEAM_COPIES)
    assert len(w) == 5000 and len(copies) == 122
    assert tiles_of(copies) == {0, 1, 3, 4} and tiles_of(copies, 4096) == {0, 1}  # both sides of position 1024 and of 4096
    body = w[["a", "b", "radius"]]
    same = np.flatnonzero(body == body[copies[0]])
    assert set(copies.tolist()) < set(same.tolist()) and len(same) == 123  # the copies and the object they are copies of
    m = reference("duplicates over the seams")[0]
    run = np.flatnonzero(m["keys"] == m["keys"][np.flatnonzero(m["sorted"] == copies[0])[0]])
    assert len(run) >= 123 and run[0] <= 1023 and run[-1] >= 1024  # equal keys on both sides of sorted position 1024: clz(i ^ j) above bit 9
    assert np.all(np.diff(m["sorted"][run]) > 0)  # ... in position order


def sah_fits(w) -> bool:
    w = np.ascontiguousarray(w)
    return bs.host().bp_sah_bytes(ptr(w), len(w), None) > 0


def test_r2_the_deep_worlds_are_as_designed():
    for name, ties in ((bs.DEEP_FITS, 1), (bs.DEEP_TOO_DEEP, bs.DEEP_TIES)):
        m = reference(name)[0]
        assert np.array_equal(m["keys"], np.array(bs.deep_keys(ties), np.uint64)), name  # the sorted keys are the designed ones
        assert len(bs.deep_keys(ties)) == ties + 240
    fit, deep = reference(bs.DEEP_FITS), reference(bs.DEEP_TOO_DEEP)
    assert 80 <= max(t["stack_need"] for t in fit) < bs.PT_BVH_STACK  # the deepest stack any test walks
    assert max(t["stack_need"] for t in deep) >= bs.PT_BVH_STACK
    t = bs.Trees(bs.case_world(bs.DEEP_FITS))
    assert t.fits and t.stack_need >= 80
    t.close()
    t = bs.Trees(bs.case_world(bs.DEEP_TOO_DEEP))
    assert not t.fits and t.stack_need >= bs.PT_BVH_STACK
    t.close()
    assert sah_fits(bs.case_world(bs.DEEP_TOO_DEEP))  # the host builder's tree of the same world fits: the fallback has somewhere to go


def test_r2_no_smaller_number_of_ties_is_too_deep():
    for ties in range(1, bs.DEEP_TIES):
        t = bs.Trees(bs.special_world("deep, %d" % ties))
        assert t.fits, ties
        t.close()


# ---------------------------------------------------------------- R3
W, H, SPP, DEPTH = 64, 48, 4, 8  # test_bvh_build_edges_gpu.py


def assert_library_builds_the_reference_tree(sc):
    """The library's own conversion of the scene and its host restatement (pt_debug_bvh_build_check) give the figures the reference
    gives on bs.scene_world(sc): what B8 compares a device build's stats with."""
    from path_trace_golang_amd import hip

    main, glass = ref.build_once(sc.name, bs.scene_world(sc))
    chk = hip.bvh_build_check(sc)
    assert (chk["nodes"], chk["objects"]) == (main["n_nodes"] + glass["n_nodes"], main["n"] + glass["n"])
    assert (chk["depth"], chk["stack_need"]) == (max(main["depth"], glass["depth"]), max(main["stack_need"], glass["stack_need"]))
    assert (chk["not_reached_once"], chk["objects_outside"], chk["children_outside"], chk["faults"]) == (0, 0, 0, 0)


@pytest.mark.parametrize("n", [1024, 1025])
def test_r3_the_tile_boundary_scenes(n):
    from path_trace_golang_amd import synth

    sc = synth.make_scene(n, 6)
    w = bs.scene_world(sc)
    assert len(w) == n and np.count_nonzero(w["kind"] & 0x100) >= 20 and sum(o.type == "plane" for o in sc.objects) == 1
    assert_library_builds_the_reference_tree(sc)


@pytest.mark.parametrize("ties", [1, bs.DEEP_TIES])
def test_r3_the_deep_scenes_keep_their_conditions_and_show_their_spheres(oracle, ties):
    sc, bare = bs.deep_scene(ties), bs.deep_scene(ties, big=False)
    w = bs.scene_world(sc)
    assert len(w) == ties + 240 + len(bs.DEEP_BIG) and np.count_nonzero(w["kind"] & 0x100) >= 20
    main, glass = ref.build_once(sc.name, w)
    chain = np.array(bs.deep_keys(ties), np.uint64)
    assert np.array_equal(main["keys"][np.isin(main["sorted"], np.arange(len(chain)))], chain)  # the large spheres move no key of the chain
    t = bs.Trees(w)
    assert_tree_equals_reference(t.tree(0), main, (ties, "main"))
    assert_tree_equals_reference(t.tree(1), glass, (ties, "dielectric"))
    need = max(main["stack_need"], glass["stack_need"])
    assert t.stack_need == need
    if ties == 1:
        assert t.fits and 80 <= need < bs.PT_BVH_STACK
    else:
        assert not t.fits and need >= bs.PT_BVH_STACK and sah_fits(w)
    t.close()
    assert_library_builds_the_reference_tree(sc)
    a = oracle.render(oracle.Scene(sc.encode()), W, H, SPP, DEPTH, seed=4)["rgba"]
    b = oracle.render(oracle.Scene(bare.encode()), W, H, SPP, DEPTH, seed=4)["rgba"]
    differ = np.count_nonzero(np.any(a != b, axis=2))
    assert differ >= 0.10 * W * H, differ  # something is on screen
