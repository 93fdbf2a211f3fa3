"""The device BVH build restated plainly, in numpy and Python only: nothing here includes, calls or is compiled from csrc/.
The host restatement (tests/bvh_build_probe.cpp) and the device (tests/bvh_build_probe.hip) are held to it by
test_bvh_build_reference_cpu.py and test_bvh_build_probe_gpu.py.

The statement differs from the product's in form wherever it can:
  keys      bit by bit, not by magic masks;
  sort      np.argsort(kind="stable");
  tree      top-down over key << 32 | position (a range splits at the highest bit in which its ends differ), not Karras' search per node;
  boxes     min / max over a node's leaf range, not a bottom-up walk with visit counters;
  collapse  lists of slots, breadth-first;
  the slot boxes are not re-encoded (the refit's tests hold the encoder): they are decoded from the node bytes and must contain the
  exact boxes."""
from __future__ import annotations

import math

import numpy as np

KIND_SPHERE, KIND_BOX = 0, 2
NODE_BYTES = 128
EMPTY_CENTRE = np.float32(3.0e38)  # an empty slot is a far-away point: centre 3e38, half extent 0
UNBOUNDED_H = 0x7f7fff00  # the half extent word of a slab that constrains nothing (payload byte off)


# ---------------------------------------------------------------- keys
def py_scale(cmin: float, cmax: float) -> float:
    e = cmax - cmin
    if not (e > 0.0) or not math.isfinite(e):
        return 0.0
    s = 2097152.0 / e
    return s if math.isfinite(s) else 0.0


def py_quantise(c: float, cmin: float, scale: float) -> int:
    if not math.isfinite(c):
        c = 0.0
    t = (c - cmin) * scale
    if not (t > 0.0):
        return 0
    if t >= 2097151.0:
        return 2097151
    return int(t)


def py_morton(qx: int, qy: int, qz: int) -> int:
    key = 0
    for b in range(21):
        key |= ((qx >> b) & 1) << (3 * b + 2) | ((qy >> b) & 1) << (3 * b + 1) | ((qz >> b) & 1) << (3 * b)
    return key


def object_boxes(world: np.ndarray):
    """lo [n, 3], hi [n, 3]: a sphere's centre -+ |radius|, a box's min / max of a and b; an axis with a NaN bound is unbounded."""
    sphere = ((world["kind"] & 0xff) == KIND_SPHERE)[:, None]
    r = np.abs(world["radius"])[:, None]
    with np.errstate(invalid="ignore"):
        lo = np.where(sphere, world["a"] - r, np.minimum(world["a"], world["b"]))
        hi = np.where(sphere, world["a"] + r, np.maximum(world["a"], world["b"]))
    bad = np.isnan(lo) | np.isnan(hi)
    return np.where(bad, -np.inf, lo), np.where(bad, np.inf, hi)


def centroids(lo: np.ndarray, hi: np.ndarray) -> np.ndarray:
    with np.errstate(invalid="ignore", over="ignore"):
        c = 0.5 * (lo + hi)
    return np.where(np.isfinite(c), c, 0.0)


def keys_of(cen: np.ndarray) -> np.ndarray:
    """[n] uint64: the Morton key of every centroid on the grid of their own min / max."""
    cmin = [float(cen[:, k].min()) for k in range(3)]
    scale = [py_scale(cmin[k], float(cen[:, k].max())) for k in range(3)]
    return np.array([py_morton(*(py_quantise(float(c[k]), cmin[k], scale[k]) for k in range(3))) for c in cen], np.uint64)


# ---------------------------------------------------------------- the binary tree
def radix_tree(sorted_keys):
    """child [n - 1, 2], parent [2 n - 1], first [2 n - 1], last [2 n - 1] of the binary radix tree over the sorted keys, top-down.
    Internal node i has id i, sorted leaf k id n - 1 + k, the root id 0; first / last are a node's range of sorted leaves."""
    n = len(sorted_keys)
    aug = [(int(k) << 32) | i for i, k in enumerate(sorted_keys)]
    child = np.full((max(n - 1, 0), 2), -1, np.int32)
    parent = np.full(2 * n - 1, -1, np.int32)
    first, last = np.zeros(2 * n - 1, np.int64), np.zeros(2 * n - 1, np.int64)
    for k in range(n):
        first[n - 1 + k] = last[n - 1 + k] = k
    todo = [(0, n - 1, 0)] if n > 1 else []  # (a, b, id): iterative, the deepest trees are 95 levels deep
    while todo:
        a, b, me = todo.pop()
        bit = (aug[a] ^ aug[b]).bit_length() - 1
        lo, hi = a, b  # aug[lo] has the bit 0, aug[hi] has it 1 (sorted: the zeros come first)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if (aug[mid] >> bit) & 1:
                hi = mid
            else:
                lo = mid
        g = lo  # the last of the range with that bit 0
        left = n - 1 + a if a == g else g
        right = n - 1 + b if g + 1 == b else g + 1
        child[me] = (left, right)
        parent[left] = parent[right] = me
        first[me], last[me] = a, b
        if a != g:
            todo.append((a, g, g))  # a left child takes its range's last index
        if g + 1 != b:
            todo.append((g + 1, b, g + 1))  # a right child its first
    return child, parent, first, last


def range_boxes(leaf_lo, leaf_hi, first, last) -> np.ndarray:
    """box [2 n - 1, 6]: min / max of the exact object boxes over every node's leaf range."""
    n = len(leaf_lo)
    box = np.zeros((2 * n - 1, 6))
    box[n - 1:, :3], box[n - 1:, 3:] = leaf_lo, leaf_hi
    for i in range(n - 1):
        box[i, :3] = leaf_lo[first[i]:last[i] + 1].min(axis=0)
        box[i, 3:] = leaf_hi[first[i]:last[i] + 1].max(axis=0)
    return box


# ---------------------------------------------------------------- the collapse
def area_of(b) -> float:
    dx, dy, dz = float(b[3]) - float(b[0]), float(b[4]) - float(b[1]), float(b[5]) - float(b[2])
    if not (dx >= 0 and dy >= 0 and dz >= 0):
        return 0.0
    a = 2 * (dx * dy + dy * dz + dz * dx)  # (Python floats: IEEE doubles, inf * 0 is NaN without an exception)
    return math.inf if math.isnan(a) else a


def gather(n: int, child, box, b: int) -> list:
    """The binary nodes in the slots of the wide node made from binary node b, in slot order."""
    if b >= n - 1:
        return [b]  # a tree of one object
    slots = [int(child[b][0]), int(child[b][1])]
    for _ in range(2):
        pick, best = -1, -1.0
        for k, s in enumerate(slots):
            if s >= n - 1:
                continue
            a = area_of(box[s])
            if a > best:  # the first of equals wins
                pick, best = k, a
        if pick < 0:
            break
        s = slots[pick]
        slots[pick] = int(child[s][0])
        slots.append(int(child[s][1]))
    return slots


def collapse(n: int, child, box, leaf_object, is_box, node_off: int, obj_off: int) -> dict:
    """Breadth-first from binary node 0.  slots [nn, 4] (-1: empty), node_base, obj_base, meta [nn], order [n], levels."""
    slots, node_base, obj_base, meta, order, levels = [], [], [], [], [], []
    cur, placed = [0], 0
    while cur:
        start = len(slots)
        levels.append(start)
        nxt = []
        for b in cur:
            sl = gather(n, child, box, b)
            node_base.append(node_off + start + len(cur) + len(nxt))
            obj_base.append(obj_off + placed)
            ranks = intm = objm = boxm = 0
            ni = no = 0
            for s, id_ in enumerate(sl):
                if id_ >= n - 1:
                    obj = int(leaf_object[id_ - (n - 1)])
                    ranks |= no << (2 * s)
                    objm |= 1 << s
                    if is_box[obj]:
                        boxm |= 1 << s
                    no += 1
                    order.append(obj)
                else:
                    ranks |= ni << (2 * s)
                    intm |= 1 << s
                    ni += 1
                    nxt.append(id_)
            placed += no
            meta.append(ranks | intm << 8 | objm << 12 | boxm << 16)
            slots.append(sl + [-1] * (4 - len(sl)))
        cur = nxt
    levels.append(len(slots))
    return dict(slots=np.array(slots, np.int32).reshape(-1, 4), node_base=np.array(node_base, np.int32), obj_base=np.array(obj_base, np.int32),
                meta=np.array(meta, np.uint32), order=np.array(order, np.int32), levels=np.array(levels, np.int32))


def stack_need(node_base, meta, node_off: int) -> int:
    """The deepest stack a walk of the tree needs: a node with k internal children leaves k - 1 entries below the child it walks,
    so its need is k - 1 plus the largest need among those children (0 without any)."""
    nn = len(meta)
    need = [0] * nn
    for q in range(nn - 1, -1, -1):
        k = bin((int(meta[q]) >> 8) & 0xf).count("1")
        if k:
            first = int(node_base[q]) - node_off
            need[q] = k - 1 + max(need[first:first + k])
    return need[0] if nn else 0


# ---------------------------------------------------------------- one tree, both trees
def build_tree(world: np.ndarray, finite, node_off: int = 0, obj_off: int = 0) -> dict:
    """Every stage of the tree of the objects `finite` (world indices, in that order) of `world`."""
    finite = np.asarray(finite, np.int64)
    n = len(finite)
    if n == 0:
        return dict(n=0, depth=0, stack_need=0, n_nodes=0)
    lo, hi = object_boxes(world[finite])
    keys = keys_of(centroids(lo, hi))
    order = np.argsort(keys, kind="stable")
    skeys = keys[order]
    child, parent, first, last = radix_tree(skeys)
    box = range_boxes(lo[order], hi[order], first, last)
    is_box = (world["kind"] & 0xff) == KIND_BOX
    c = collapse(n, child, box, finite[order], is_box, node_off, obj_off)
    return dict(n=n, keys=skeys, sorted=order.astype(np.int32), child=child, parent=parent, box=box, first=first, last=last,
                n_nodes=len(c["meta"]), depth=len(c["levels"]) - 1, stack_need=stack_need(c["node_base"], c["meta"], node_off), **c)


def object_lists(world: np.ndarray):
    """World indices of the finite objects (no planes in these worlds) and of the dielectric ones among them."""
    finite = np.arange(len(world))
    return finite, finite[(world["kind"] & 0x100) != 0]


def build(world: np.ndarray):
    """(main tree, dielectric tree): the second behind the first in both arrays."""
    finite, glass = object_lists(world)
    main = build_tree(world, finite)
    return main, build_tree(world, glass, main["n_nodes"], main["n"])


_trees = {}


def build_once(name: str, world: np.ndarray):
    """build(world), computed once per name and shared by the tests that need it (read-only)."""
    if name not in _trees:
        _trees[name] = build(world)
        for t in _trees[name]:
            for v in t.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
    return _trees[name]


# ---------------------------------------------------------------- a built tree against the reference
STAGES = ("keys", "sorted", "child", "parent", "box", "slots", "node_base", "obj_base", "meta", "order", "levels")


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def differences(got: dict, want: dict) -> list:
    """The stages in which a built tree `got` (the arrays the probes hand out: keys, sorted, child, parent, box, nodes, order, levels,
    and slots where the builder can say them) is not the reference tree `want`, bit for bit; [] when it is.  node_base, obj_base and
    meta are read from the node bytes, once from their words and once from the low bytes of the half extents; "slot boxes" says that
    some slot's decoded box does not contain the exact box of its binary node, or that an empty slot is not the far-away point."""
    if got["n"] != want["n"]:
        return ["n"]
    if want["n"] == 0:
        return []
    have = dict(got)
    have["node_base"], have["obj_base"], have["meta"] = node_words(got["nodes"])
    bad = [k for k in STAGES if k in have and not same_bits(have[k], want[k].astype(have[k].dtype))]
    words = (want["node_base"].astype(np.uint32), want["obj_base"].astype(np.uint32), want["meta"] & np.uint32(0xffffff))
    if len(got["nodes"]) != want["n_nodes"] * NODE_BYTES or not all(np.array_equal(a, b) for a, b in zip(payload_words(got["nodes"]), words)):
        bad.append("payload bytes")
    if slot_box_faults(got["nodes"], want):
        bad.append("slot boxes")
    return bad


# ---------------------------------------------------------------- what a node's bytes say
def node_words(nodes: np.ndarray):
    """node_base, obj_base, meta [nn] of node bytes."""
    w = np.ascontiguousarray(nodes).reshape(-1, NODE_BYTES)[:, 96:108].copy().view(np.uint32)
    return w[:, 0].astype(np.int32), w[:, 1].astype(np.int32), w[:, 2].copy()


def payload_words(nodes: np.ndarray):
    """node_base, obj_base, meta (24 bits) [nn] as the low bytes of the twelve half extents carry them: byte s of word k in h[k][s]."""
    h = np.ascontiguousarray(nodes).reshape(-1, NODE_BYTES)[:, 48:96].copy().view(np.uint32).reshape(-1, 3, 4)
    w = np.zeros((len(h), 3), np.uint32)
    for s in range(4):
        w |= (h[:, :, s] & 0xff) << np.uint32(8 * s)
    return w[:, 0], w[:, 1], w[:, 2]


def slot_boxes(nodes: np.ndarray):
    """c [nn, 3, 4] float32 and h [nn, 3, 4] float32 with the payload byte masked off, and the masked words themselves."""
    raw = np.ascontiguousarray(nodes).reshape(-1, NODE_BYTES)
    c = raw[:, 0:48].copy().view(np.float32).reshape(-1, 3, 4)
    hw = raw[:, 48:96].copy().view(np.uint32).reshape(-1, 3, 4) & np.uint32(0xffffff00)
    return c, hw.view(np.float32), hw


def slot_box_faults(nodes: np.ndarray, ref: dict) -> int:
    """How many slots of `nodes` do not hold what the reference tree `ref` says: an occupied slot's decoded [c - h, c + h] must contain
    the exact box of its binary node (an unbounded axis: centre 0 and the largest half extent), an empty one is the far-away point."""
    c, h, hw = slot_boxes(nodes)
    if len(c) != ref["n_nodes"]:
        return abs(len(c) - ref["n_nodes"]) + 1
    c64, h64 = c.astype(np.float64), h.astype(np.float64)
    faults = 0
    for q in range(len(c)):
        for s in range(4):
            b = int(ref["slots"][q][s])
            if b < 0:
                faults += not (np.all(c[q, :, s] == EMPTY_CENTRE) and np.all(hw[q, :, s] == 0))
                continue
            for k in range(3):
                lo, hi = ref["box"][b][k], ref["box"][b][3 + k]
                if math.isinf(lo) or math.isinf(hi):
                    ok = c[q, k, s] == 0 and hw[q, k, s] == UNBOUNDED_H
                else:
                    ok = c64[q, k, s] - h64[q, k, s] <= lo and c64[q, k, s] + h64[q, k, s] >= hi
                faults += not ok
    return faults
