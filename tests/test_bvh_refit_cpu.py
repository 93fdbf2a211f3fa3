"""The BVH refit on the host: csrc/pt_bvh_refit.h is the one statement of a slot's bits, called by the builder, by the
scene preparation's payload step and by the refit.  Here its host build (tests/bvh_refit_probe.cpp) is held to: a refit to the same
world changes no byte; a refit after a move holds every object, keeps the topology, equals a fresh encode and finds the linear
scan's winner for 20 000 rays; the same after resizes, negative and zero radii and edited dielectrics (T2b), which the rule accepts
as it accepts moves; edits of kind, material or count are refused with their reason; the quality figure has the shape it states."""
import math
import struct
import subprocess

import numpy as np
import pytest

import bvh_refit_support as rs

CASES = [(n, d) for n in rs.SIZES for d in rs.DIELECTRICS]


def _scene(n, seed=3):
    from path_trace_golang_amd import synth

    return synth.make_scene(n, seed)


# ---------------------------------------------------------------- the bit routines
def _f32(bits):
    return struct.unpack("<f", struct.pack("<I", bits))[0]


def _bits(f):
    return struct.unpack("<I", struct.pack("<f", f))[0]


def test_next_up_is_nextafterf_towards_plus_infinity():
    L = rs.host()
    for f in (0.0, -0.0, 1.0, -1.0, 1.5e-45, -1.5e-45, 3.4028235e38, -3.4028235e38, 1.17549435e-38, -1.17549435e-38, 0.1, -0.1, 16777216.0):
        b = _bits(f)
        with np.errstate(over="ignore"):
            want = _bits(float(np.nextafter(np.float32(_f32(b)), np.float32(np.inf))))
        assert L.rp_next_up(b) == want, (f, hex(L.rp_next_up(b)), hex(want))


def test_round_up_is_the_smallest_float_not_below():
    L = rs.host()
    rng = np.random.default_rng(1)
    vals = list(rng.uniform(-1e3, 1e3, 200)) + list(10.0 ** rng.uniform(-44, 38, 200)) + [0.0, 1.0, 1.0 + 2.0 ** -40, 2.0 ** -149, 2.0 ** -150,
                                                                                           3.4028235e38, 3.5e38]
    for v in vals:
        f = np.float32(_f32(L.rp_round_up(float(v))))
        assert float(f) >= v, v
        if np.isfinite(f):
            assert float(np.nextafter(f, np.float32(-np.inf))) < v, v


def test_axis_encoding_holds_the_inflated_interval_and_falls_back():
    L = rs.host()
    out = (rs.C.c_uint32 * 2)()
    rng = np.random.default_rng(2)
    for _ in range(500):
        lo = float(rng.uniform(-50, 50))
        hi = lo + float(10.0 ** rng.uniform(-6, 2))
        m = float(10.0 ** rng.uniform(-4, 0))
        L.rp_encode_axis(lo, hi, m, out)
        c, h = _f32(out[0]), _f32(out[1])
        assert c - h <= lo - m and c + h >= hi + m
        w = _f32(L.rp_h_word(out[1], 0xAB))
        assert L.rp_h_word(out[1], 0xAB) & 0xff == 0xAB and w >= h and w <= h * (1 + 2.0 ** -14)
    for lo, hi, m in ((math.nan, 1.0, 0.1), (0.0, math.inf, 0.1), (-1e300, 1e300, 0.1), (0.0, 1.0, math.inf)):
        L.rp_encode_axis(lo, hi, m, out)
        assert (out[0], out[1]) == (0, 0x7f800000), (lo, hi, m)
    assert L.rp_h_word(0x7f800000, 0x12) == 0x7f7fff12 and L.rp_h_word(0x7fc00000, 0) == 0x7f7fff00 and L.rp_h_word(0x7f7fff01, 0) == 0x7f7fff00


# ---------------------------------------------------------------- T1
@pytest.mark.parametrize("n,ndiel", CASES)
def test_t1_refit_to_the_same_world_changes_no_byte(n, ndiel):
    w = rs.world_of(n, ndiel)
    t = rs.Tree(w)
    assert t.n_objs == n + min(ndiel, len(range(0, n, 3))) and t.main_objs == n
    before = t.state()
    assert np.array_equal(before["nodes"], t.built)
    t.refit(w)
    after = t.state()
    assert np.array_equal(after["nodes"], t.built), int(np.count_nonzero(after["nodes"] != t.built))
    assert np.array_equal(after["objs"], before["objs"])
    assert t.check(w) == dict(objects_outside=0, children_outside=0, bytes_differ=0, topology_changed=0, records_differ=0)
    assert after["levels"][0] == 0 and after["levels"][-1] == t.n_nodes and np.all(np.diff(after["levels"]) > 0)
    t.close()


def test_t1_a_tree_of_one_object_holds_it_in_slot_0():
    t = rs.Tree(rs.world_of(1, 0))
    s = t.state()
    meta = int(np.frombuffer(s["nodes"].tobytes(), np.uint32)[26])  # node 0: node_base, obj_base, meta at bytes 96..107
    assert t.n_nodes == 1 and (meta >> 12) & 0xf == 1 and (meta >> 8) & 0xf == 0
    t.close()


@pytest.mark.parametrize("n", [17, 300, 3000])
def test_t1_the_library_check_reports_zeros_for_an_unchanged_scene(n):
    from path_trace_golang_amd import hip

    sc = _scene(n)
    r = hip.bvh_refit_check(sc, sc)
    assert r["nodes"] > 0 and r["objects"] >= n
    assert (r["reason"], r["objects_outside"], r["children_outside"], r["bytes_differ"], r["topology_changed"]) == (0, 0, 0, 0, 0)
    assert r["cost_ratio_x1000"] == 1000


# ---------------------------------------------------------------- T2
@pytest.mark.parametrize("n,ndiel", [(17, 1), (300, 7), (3000, 7)])
def test_t2_a_refit_after_a_move_holds_its_objects_and_equals_a_fresh_encode(n, ndiel):
    w = rs.world_of(n, ndiel)
    t = rs.Tree(w)
    m0 = t.margin
    margins = []
    for name, wm in rs.moves(w):
        t.refit(wm)
        margins.append(t.margin)
        assert t.check(wm) == dict(objects_outside=0, children_outside=0, bytes_differ=0, topology_changed=0, records_differ=0), name
    assert margins[2] > 2 * m0 and margins[3] < margins[2], margins
    t.refit(w)  # nothing accumulates: back at the built world the bytes are the built ones
    assert np.array_equal(t.state()["nodes"], t.built)
    t.close()


def test_t2_the_tree_finds_the_linear_scans_winner_after_every_move():
    w = rs.world_of(300, 7)
    t = rs.Tree(w)
    bad, hits = t.rays(w, 20000, 1)
    assert bad == 0 and hits > 2000
    for k, (name, wm) in enumerate(rs.moves(w)):
        t.refit(wm)
        bad, hits = t.rays(wm, 20000, 100 + k)
        assert bad == 0 and hits > 200, (name, bad, hits)
    t.close()


def test_t2_a_stale_tree_is_caught_by_the_same_checks():
    """The checks can fail: the built tree against a moved world, without the refit."""
    w = rs.world_of(300, 7)
    t = rs.Tree(w)
    name, wm = list(rs.moves(w))[1]
    c = t.check(wm)
    assert c["objects_outside"] > 0 and c["bytes_differ"] > 0 and c["records_differ"] > 0
    assert t.rays(wm, 20000, 9)[0] > 0
    t.close()


def test_the_probe_runs_stand_alone_and_under_the_sanitizers():
    for flags, name in (((), "bvh_refit_probe"), (("-fsanitize=address,undefined", "-fno-sanitize-recover=all"), "bvh_refit_probe_san")):
        r = subprocess.run([rs.standalone(flags, name), "300"], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "" and "failed 0" in r.stdout, (name, r.stdout, r.stderr)


def test_t2_the_library_check_on_moved_scenes():
    from path_trace_golang_amd import hip

    sc = _scene(300)
    idx = rs.finite_indices(sc)
    moved = rs.moved_scene(sc, {i: (0.3, 0.1, -0.2) for i in idx[::5]})
    r = hip.bvh_refit_check(sc, moved)
    assert (r["reason"], r["objects_outside"], r["children_outside"], r["bytes_differ"], r["topology_changed"]) == (0, 0, 0, 0, 0)
    assert 500 < r["cost_ratio_x1000"] < 2000  # a fifth of the objects by a third of a unit: the same tree, a little looser or tighter


# ---------------------------------------------------------------- T2b: edits that are no translations, and that the rule accepts
ZEROS = dict(objects_outside=0, children_outside=0, bytes_differ=0, topology_changed=0, records_differ=0)


def test_t2b_the_resizes_are_what_they_say():
    w = rs.world_of(300, 7)
    steps = list(rs.resizes(w))
    assert tuple(name for name, _ in steps) == rs.RESIZES
    sph, box, die = (w["kind"] & 0xff) == rs.KIND_SPHERE, (w["kind"] & 0xff) == rs.KIND_BOX, (w["kind"] & 0x100) != 0
    assert sph.sum() > 100 and box.sum() > 50 and die.sum() == 7 and (die & sph).any() and (die & box).any()
    for name, wm in steps:
        assert np.array_equal(wm["kind"], w["kind"]) and np.array_equal(wm["mat"], w["mat"]), name  # what refit_reason holds on to
        r = wm["radius"][sph]
        with np.errstate(divide="ignore"):
            assert np.array_equal(wm["radius_sq"][sph], r * r) and np.array_equal(wm["inv_radius"][sph], 1.0 / r), name
        assert not wm[box]["radius"].any() and np.all(wm["b"][box] >= wm["a"][box]), name
    by = dict(steps)
    assert np.allclose(by[rs.RESIZES[0]]["radius"][sph], 1.7 * w["radius"][sph]) and np.array_equal(by[rs.RESIZES[0]][box], w[box])
    assert np.allclose(by[rs.RESIZES[1]]["radius"][sph], 0.01 * w["radius"][sph])
    ext, ext0 = by[rs.RESIZES[2]]["b"][box] - by[rs.RESIZES[2]]["a"][box], w["b"][box] - w["a"][box]
    assert np.allclose(ext, ext0 * [2.5, 0.2, 1.0]) and np.allclose(by[rs.RESIZES[2]]["a"][box] + 0.5 * ext, w["a"][box] + 0.5 * ext0)
    assert np.count_nonzero(by[rs.RESIZES[3]]["radius"] < 0) == 2 and np.count_nonzero(by[rs.RESIZES[3]] != w) == 2
    zero = by[rs.RESIZES[4]]
    assert np.count_nonzero(sph & (zero["radius"] == 0)) == 2 and np.count_nonzero(np.isinf(zero["inv_radius"])) == 2
    d = by[rs.RESIZES[5]]
    assert np.array_equal(d[~die], w[~die]) and np.all(d[die] != w[die])
    assert np.allclose(d["a"][die & sph], w["a"][die & sph] + rs.DIELECTRIC_MOVE) and np.allclose(d["radius"][die & sph], 1.3 * w["radius"][die & sph])
    assert np.allclose(d["b"][die & box] - d["a"][die & box], 1.3 * (w["b"][die & box] - w["a"][die & box]))
    assert by[rs.RESIZES[6]].tobytes() == w.tobytes()


@pytest.mark.parametrize("n,ndiel", [(17, 1), (300, 7), (3000, 7)])
def test_t2b_a_refit_after_a_resize_holds_its_objects_and_equals_a_fresh_encode(n, ndiel):
    w = rs.world_of(n, ndiel)
    t = rs.Tree(w)
    assert t.n_objs > t.main_objs  # a second tree, of the dielectrics
    for name, wm in rs.resizes(w):
        t.refit(wm)
        assert t.check(wm) == ZEROS, (name, t.check(wm))
    assert np.array_equal(t.state()["nodes"], t.built)  # the last step is the built world: the built bytes
    t.close()


@pytest.mark.parametrize("n,ndiel,least", [(17, 1, 2000), (300, 7, 3000), (3000, 7, 3000)])
def test_t2b_the_tree_finds_the_linear_scans_winner_after_every_resize(n, ndiel, least):
    """`least`: of 20 000 rays from inside the world's bounds at least this many hit something after every step -- also with every
    sphere at a hundredth of its size, where the boxes (two objects in five) still stand."""
    w = rs.world_of(n, ndiel)
    t = rs.Tree(w)
    for k, (name, wm) in enumerate(rs.resizes(w)):
        t.refit(wm)
        bad, hits = t.rays(wm, 20000, 200 + k)
        assert bad == 0 and hits > least, (name, bad, hits)
    t.close()


def test_t2b_a_stale_tree_is_caught_after_a_resize():
    """The checks can fail: the built tree against the world with every sphere grown, without the refit."""
    w = rs.world_of(300, 7)
    t = rs.Tree(w)
    name, wm = next(iter(rs.resizes(w)))
    c = t.check(wm)
    assert c["objects_outside"] > 0 and c["bytes_differ"] > 0 and c["records_differ"] > 0
    assert t.rays(wm, 20000, 9)[0] > 0
    t.close()


def test_t2b_the_library_check_on_every_edited_scene():
    from path_trace_golang_amd import hip

    sc = _scene(300, 4)
    edits = list(rs.edited_scenes(sc))
    assert tuple(name for name, _ in edits) == rs.EDITS and len(rs.dielectric_indices(sc)) >= 10
    ratios = {}
    for name, edit in edits:
        assert [o.type for o in edit.objects] == [o.type for o in sc.objects] and [o.material_id for o in edit.objects] == [o.material_id for o in sc.objects]
        assert edit.encode() != sc.encode(), name
        r = hip.bvh_refit_check(sc, edit)
        assert (r["reason"], r["objects_outside"], r["children_outside"], r["bytes_differ"], r["topology_changed"]) == (0, 0, 0, 0, 0), (name, r)
        ratios[name] = r["cost_ratio_x1000"]
    print("figure ratios x1000:", ratios)
    assert ratios["plane lowered"] == 1000  # the plane is in no tree
    assert ratios["spheres grown"] > 1000 > ratios["spheres shrunk"] and ratios["radii negated"] == 1000 and ratios["radii zero"] < 1000


# ---------------------------------------------------------------- T3
def test_t3_edits_that_are_no_moves_report_their_reason():
    import copy

    from path_trace_golang_amd import capi, hip

    sc = _scene(300)
    idx = rs.finite_indices(sc)
    sphere = next(i for i in idx if sc.objects[i].type == "sphere")
    lambert = next(i for i in idx if sc.objects[i].material_id in ("red", "green", "blue"))

    kind = copy.deepcopy(sc)
    kind.objects[sphere].type = "box"
    kind.objects[sphere].size.y = kind.objects[sphere].size.z = kind.objects[sphere].size.x
    swap = copy.deepcopy(sc)
    swap.objects[lambert].material_id = "glass"
    more = copy.deepcopy(sc)
    more.objects.append(copy.deepcopy(sc.objects[sphere]))
    more.objects[-1].id = "one-more"
    huge = copy.deepcopy(sc)
    huge.objects[sphere].position.x = 1e38
    for name, edit, reason in (("kind", kind, capi.PT_BVH_REASON_CHANGED), ("material", swap, capi.PT_BVH_REASON_CHANGED),
                               ("one more", more, capi.PT_BVH_REASON_CHANGED), ("1e38", huge, capi.PT_BVH_REASON_NONFINITE)):
        r = hip.bvh_refit_check(sc, edit)
        assert r["reason"] == reason, (name, r)
        # ... and the full build of the edited scene that takes the refit's place is sound
        assert (r["objects_outside"], r["children_outside"], r["bytes_differ"], r["topology_changed"]) == (0, 0, 0, 0), (name, r)


# ---------------------------------------------------------------- T4
@pytest.mark.parametrize("n", [5, 300, 3000, 20000])
def test_t4_the_figure_is_the_fixed_shape_sum(n):
    w = rs.world_of(n, 7)
    t = rs.Tree(w)
    cost = t.refit(w)
    s = t.state()
    assert struct.pack("<d", cost) == struct.pack("<d", rs.python_cost(s["area"][:t.main_nodes]))
    assert cost > 0 and (n < 20000 or t.main_nodes > 4096)  # the largest case spans more than one block
    a = s["area"][:t.main_nodes]
    assert struct.pack("<d", float(rs.host().rp_cost_of(rs.ptr(np.ascontiguousarray(a)), len(a)))) == struct.pack("<d", cost)
    t.close()


def test_t4_the_teleported_scene_degrades_past_the_bound_t7_uses():
    from path_trace_golang_amd import hip

    sc = _scene(300)
    r = hip.bvh_refit_check(sc, rs.teleported(sc))
    assert r["reason"] == 0 and (r["objects_outside"], r["children_outside"], r["bytes_differ"], r["topology_changed"]) == (0, 0, 0, 0)
    assert r["cost_ratio_x1000"] > 1500, r
