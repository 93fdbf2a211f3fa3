"""B6: the product's build kernels and launch sequence (tests/bvh_build_probe.hip) against the host restatement of the same
header (tests/bvh_build_probe.cpp), byte for byte at every stage: sorted keys and order, the binary tree's children and parents, its
boxes, the wide nodes, `order`, the records and the level table -- on B2's worlds and on 20 000 objects, where every kernel and every
scan runs more than one block and the sort more than one tile.

The host restatement is a second compile of the device's own functions, so every stage of the device is also held to
tests/bvh_build_reference.py directly (keys, order, children, parents, boxes, node words, payload bytes, slot boxes, `order`, levels):
the sort, the scans and the level kernels have no other statement.  The worlds on the boundaries of the kernels
(bvh_build_support.NEW_CASE_NAMES: a block, a tile, a sort block, a fifth tile; ties over the seams; the deep chains) are built twice in
the process, and the second build's bytes are the first's."""
from __future__ import annotations

import numpy as np
import pytest

import bvh_build_reference as ref
import bvh_build_support as bs

pytestmark = pytest.mark.gpu

STAGES = ("keys", "sorted", "child", "parent", "box", "nodes", "order", "levels")


def compare(world: np.ndarray, name: str, twice: bool = False):
    t = bs.Trees(world)
    finite, glass = bs.object_lists(world)
    host_main, host_glass = t.tree(0), t.tree(1)
    want_main, want_glass = ref.build_once(name, world)
    dev_main = bs.gpu_tree(world, finite, t.margin, 0, 0)
    for k in STAGES:
        assert np.array_equal(dev_main[k].view(np.uint8), host_main[k].view(np.uint8)), (name, "main", k)
    assert ref.differences(dev_main, want_main) == [], (name, "main")
    dev_glass = None
    if len(glass):
        dev_glass = bs.gpu_tree(world, glass, t.margin, t.main_nodes, t.main_objs)
        for k in STAGES:
            assert np.array_equal(dev_glass[k].view(np.uint8), host_glass[k].view(np.uint8)), (name, "dielectric", k)
        assert ref.differences(dev_glass, want_glass) == [], (name, "dielectric")
    assert (want_main["n_nodes"], want_main["n"]) == (t.main_nodes, t.main_objs)
    # both trees together are what the host restatement hands a render
    a = t.arrays()
    nodes = np.concatenate([dev_main["nodes"]] + ([dev_glass["nodes"]] if dev_glass else []))
    order = np.concatenate([dev_main["order"]] + ([dev_glass["order"]] if dev_glass else []))
    assert np.array_equal(nodes, a["nodes"]), name
    assert np.array_equal(bs.gpu_objs(order, world), a["objs"]), name
    if twice:  # nothing of a build depends on what the build before left behind, or on the order its lanes ran in
        again = [bs.gpu_tree(world, finite, t.margin, 0, 0)] + ([bs.gpu_tree(world, glass, t.margin, t.main_nodes, t.main_objs)] if len(glass) else [])
        for first, second, which in zip([dev_main, dev_glass], again, ("main", "dielectric")):
            for k in STAGES:
                assert np.array_equal(second[k].view(np.uint8), first[k].view(np.uint8)), (name, which, k, "second build")
    t.close()
    return dev_main


@pytest.mark.parametrize("name", bs.CASE_NAMES)
def test_b6_device_equals_host(name):
    compare(bs.case_world(name), name)


@pytest.mark.parametrize("name", bs.NEW_CASE_NAMES)
def test_b6_device_equals_host_and_reference_on_the_boundaries(name):
    """What each world is there for is asserted, without a GPU, by test_bvh_build_reference_cpu.py (R2)."""
    compare(bs.case_world(name), name, twice=True)


def test_b6_twenty_thousand_objects_run_every_kernel_in_several_blocks():
    sizes = bs.gpu_sizes()
    n = bs.LARGE
    assert sizes == dict(sort_tile=1024, scan_tile=1024, reduce_tile=1024, sort_passes=8)
    assert n > 4 * sizes["sort_tile"]  # the sort: more than one block of four tiles
    assert 256 * -(-n // sizes["sort_tile"]) > sizes["scan_tile"]  # its histogram scan: more than one block
    assert n > sizes["reduce_tile"] and n > 256  # the centroid reduction; keys, radix tree and boxes: one lane per object
    m = compare(bs.large_world(), "large")
    widths = np.diff(m["levels"])
    assert widths.max() > sizes["scan_tile"]  # the collapse: a level's scan in more than one block (its kernels then too)
    ends = m["levels"][1:]
    assert np.any((4 * widths) % 64 != 0) and np.any(ends % 64 != 0)  # some level's quads end in the middle of a wave
