"""The device BVH build's shared header on the host: the key routines against a Python restatement (B1), the invariants
of the Morton-order trees on every size and on the worlds made to break the radix tree, the tie-break and the collapse (B2), the host
builder's bytes against digests recorded from the commit before (B3: the shared gather rule changed nothing), and the stand-alone probe under the sanitizers (B4).  No GPU."""
from __future__ import annotations

import hashlib
import json
import math
import os
import subprocess

import numpy as np
import pytest

import bvh_build_support as bs
import bvh_refit_support as rs
from bvh_build_reference import py_morton, py_quantise, py_scale  # B1's Python restatement of the key routines lives with the rest of it
from fog_support import ptr

RAYS = 20000


# ---------------------------------------------------------------- B1
def axis_values(cmin: float, cmax: float, seed: int) -> np.ndarray:
    """4096 values of one axis: the ends, one ulp inside each, a non-finite centroid, and the rest spread over the extent."""
    rng = np.random.default_rng(seed)
    v = cmin + (cmax - cmin) * rng.uniform(0.0, 1.0, 4096)
    v[:6] = [cmin, cmax, np.nextafter(cmin, cmax), np.nextafter(cmax, cmin), np.inf, np.nan]
    return np.ascontiguousarray(np.clip(v, cmin, cmax) if math.isfinite(cmin) else v)


@pytest.mark.parametrize("cmin,cmax", [(-3.0, 5.0), (0.0, 1e36), (-1e36, 1e36), (2.5, 2.5), (0.0, 5e-324), (-1e-3, 1e-3), (1.0, 1.0 + 2 ** -40)])
def test_b1_quantise_matches_python(cmin, cmax):
    L = bs.host()
    scale = L.bp_key_scale(cmin, cmax)
    assert scale == py_scale(cmin, cmax)
    if cmax == cmin or cmax == 5e-324:
        assert scale == 0.0  # extent 0, and an extent whose quotient is not finite
    v = axis_values(cmin, cmax, 3)
    v[4:6] = [np.inf, np.nan]
    out = np.zeros(len(v), np.uint32)
    L.bp_quantise(ptr(v), len(v), cmin, scale, ptr(out))
    want = np.array([py_quantise(float(x), cmin, scale) for x in v], np.uint32)
    assert np.array_equal(out, want)
    assert out.max() <= 2097151
    if scale > 0.0:
        assert out[0] == 0 and out[1] == 2097151


def test_b1_interleave_matches_python():
    rng = np.random.default_rng(5)
    q = rng.integers(0, 1 << 21, (4096, 3), dtype=np.uint32)
    q[:4] = [[0, 0, 0], [2097151, 2097151, 2097151], [2097151, 0, 0], [0, 0, 2097151]]
    q = np.ascontiguousarray(q)
    out = np.zeros(len(q), np.uint64)
    bs.host().bp_morton(ptr(q), len(q), ptr(out))
    want = np.array([py_morton(int(a), int(b), int(c)) for a, b, c in q], np.uint64)
    assert np.array_equal(out, want)
    assert int(out.max()) < 1 << 63
    assert int(out[2]) == sum(1 << (3 * b + 2) for b in range(21))  # x is the highest bit of every triple


# ---------------------------------------------------------------- B2
@pytest.fixture(scope="module", params=bs.CASE_NAMES)
def built(request):
    t = bs.Trees(bs.case_world(request.param))
    yield request.param, t
    t.close()


def test_b2_invariants(built):
    name, t = built
    n = len(t.world)
    nd = int(((t.world["kind"] & 0x100) != 0).sum())
    chk = t.check()
    assert chk["objects"] == n + nd == t.n_objs and t.main_objs == n
    assert chk["not_reached_once"] == 0, name
    assert chk["objects_outside"] == 0 and chk["children_outside"] == 0, name
    assert chk["faults"] == 0, name  # consecutive children and objects, increasing levels, a refit to the same world changes no byte
    a = t.arrays()
    assert np.all(np.diff(a["levels"]) > 0) and a["levels"][0] == 0 and a["levels"][-1] == t.n_nodes
    meta = a["nodes"].reshape(-1, rs.NODE_BYTES)[:, 104:108].copy().view(np.uint32)[:, 0]
    assert np.all(((meta >> 8) & 0xf) & ((meta >> 12) & 0xf) == 0)  # a slot is internal, an object or empty: four at the most
    assert t.refit_same() == 0


def test_b2_rays_find_the_linear_winner(built):
    name, t = built
    bad, hits = t.rays(RAYS, 17)
    assert bad == 0, name
    if len(t.world) >= 17 and name != "geometric ratio 2":
        assert hits > 0


def test_b2_equal_keys_give_a_balanced_tree():
    t = bs.Trees(bs.special_world("one centroid"))
    m = t.tree(0)
    assert len(np.unique(m["keys"])) == 1
    assert np.array_equal(m["sorted"], np.arange(300))  # ties stay in position order
    # 300 leaves balanced by position are a binary tree of ceil(log2 300) = 9 levels, and a wide level spans one binary level at the
    # least; without the tie-break equal keys would chain, a level per object
    assert t.depth <= 9
    t.close()


def test_b2_geometric_spacing_fits_the_stack():
    """x = 2^(i - 200): the top 21 objects take a cell of their own on the key's 21 bits and peel off one per binary level, the other
    279 share cell 0 and are balanced by position.  The stack need is far below the limit, so the product builds this on the device."""
    t = bs.Trees(bs.special_world("geometric ratio 2"))
    assert t.fits and t.stack_need < bs.PT_BVH_STACK
    assert t.stack_need <= 3 * (21 + 9)  # at most three entries left per level of at most 21 + ceil(log2 279) binary levels
    t.close()
    tight = bs.Trees(bs.special_world("geometric ratio 2"), stack_limit=2)  # ... and the limit is what decides
    assert not tight.fits
    tight.close()


# ---------------------------------------------------------------- B3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bvh_sah_build_digests.json")


def sah_digest(world) -> dict:
    """Nodes as built (payload bytes in place), records and level table of ptbvh::build_scene_trees on `world`, as a SHA-256."""
    t = rs.Tree(world)
    st = t.state()
    h = hashlib.sha256()
    for part in (t.built.tobytes(), st["objs"].tobytes(), st["levels"].astype("<i4").tobytes()):
        h.update(part)
    out = dict(nodes=t.n_nodes, records=t.n_objs, sha256=h.hexdigest())
    t.close()
    return out


def test_b3_host_builder_bytes_are_the_parents():
    """tests/golden/bvh_sah_build_digests.json holds, per (n, dielectrics) of rs.SIZES x rs.DIELECTRICS, the digest of what
    ptbvh::build_scene_trees gave on rs.world_of(n, dielectrics) BEFORE its gather rule and stack loop moved into shared functions
    (recorded from the commit before the device build, with this function's recipe).  The builder must still give those bytes."""
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted("%d/%d" % (n, nd) for n in rs.SIZES for nd in rs.DIELECTRICS)
    for n in rs.SIZES:
        for nd in rs.DIELECTRICS:
            assert sah_digest(rs.world_of(n, nd)) == golden["%d/%d" % (n, nd)], (n, nd)


def test_b3_this_probes_build_of_the_host_builder_agrees():
    """The same bytes through this probe's compile of pt_bvh.h (nodes, then records)."""
    L = bs.host()
    for n in rs.SIZES:
        w = np.ascontiguousarray(rs.world_of(n, 7))
        size = L.bp_sah_bytes(ptr(w), n, None)
        got = np.zeros(size, np.uint8)
        L.bp_sah_bytes(ptr(w), n, ptr(got))
        t = rs.Tree(w)
        assert np.array_equal(got, np.concatenate([t.built, t.state()["objs"]]))
        t.close()


# ---------------------------------------------------------------- B4
def test_b4_standalone_probe_under_sanitizers(tmp_path):
    exe = bs.standalone(("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"), "bvh_build_probe_san")
    files = []
    for i, (name, w) in enumerate(list(bs.cases()) + [(name, bs.case_world(name)) for name in bs.NEW_CASE_NAMES]):
        p = tmp_path / ("world%02d.bin" % i)
        np.ascontiguousarray(w).tofile(p)
        files.append(str(p))
    r = subprocess.run([exe, *files], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr  # a sanitizer report goes to stderr
    assert r.stdout.count("failed 0") == len(files)
