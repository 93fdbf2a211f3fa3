"""The fog and GL tree walks ray by ray, without a GPU: the host build of ptg::TreeWorld (csrc/pt_gl_walk.h, through glwalk_support's
gw_queries) on every table of walk_probe_support.py -- the ray classes of ray_inject_support.py on the 341-object scene at every scale
of DESIGN 9 that stays on the BVH path, directions scaled with the scene and left at unit length -- against gr_queries of
tests/glshade_reference.c, bit for bit; and that the tables are what the device probe's tests need them to be (the conditions below
are asserted from the reference and numpy alone).  The stand-alone host program walks the deepest tree under ASan and UBSan."""
from __future__ import annotations

import numpy as np
import pytest

import walk_probe_support as wp


def test_the_probe_calls_the_product():
    with open(wp.SOURCE) as f:
        src = f.read()
    for name in wp.PRODUCT:
        assert name in src, name
    for word in ("walk_slab", "slab_recips", "walk_closest(", "walk_occluded(", "hit_t(", "hit_object(", "asm"):
        assert word not in src, word  # no traversal and no intersection code of its own
    for header in ('#include "pt_gl_walk.h"', '#include "pt_fog_walk.h"', '#include "probe_common.h"'):
        assert header in src, header
    with open(wp.HOST_SOURCE) as f:
        host = f.read()
    assert "ptg::TreeWorld" in host and "int stack[PT_BVH_STACK]" in host


def test_the_scales_stay_on_the_bvh_path_and_the_tables_are_whole_waves():
    assert wp.RAYS_PER_CLASS == 832 and len(wp.CLASSES) == 5
    kinds = wp.S.class_mixed()[1]
    assert {kinds[w] for w in wp.WAVES} == set(wp.S.ODD_KINDS)  # every odd kind of the mixed class is kept
    for k in wp.K:
        for name in wp.SCALED_SCENES:
            info, bounds = wp.host_info(wp.case_of(name, k))
            assert info["built"] == 1 and info["world"] == 341 and info["planes"] == (1 if name == "bvh" else 0), (name, k, info)
            assert 1 <= info["stack_need"] < 96
            assert bounds["clip_bound"] < 0.99 * bounds["origin_bound"] or np.isinf(bounds["clip_bound"]), (k, bounds)  # clip_bound binds
        for fam in wp.X.families(k):
            rays, where = wp.rays_of(wp.case_of("bvh", k), k, fam)
            assert len(rays) == 5 * wp.RAYS_PER_CLASS + 64 and where["far origins"].stop - where["far origins"].start == wp.RAYS_PER_CLASS + 64


def _edge_sides(T):
    """The edge origins of a table on either side of walk_ok."""
    sl = T["where"]["far origins"]
    ok = T["ray_ok"][sl][-64:]
    return int(np.count_nonzero(ok)), int(np.count_nonzero(~ok))


def _conditions(scene_name, k, fam, T):
    """What the table must hold for the GPU comparison to mean something; from the reference and numpy alone."""
    tag = (scene_name, k, fam)
    q, ok = T["q"], T["ok"]
    if not wp.band_walks(scene_name, k, fam):
        # a direction scaled with the scene has d.d = 4^k a0 outside (1e-29, 1e29): nothing of ordinary length walks.  What does walk
        # are strays of the classes that vary |d| by many binades, whose own factor happens to undo 2^k; every other query takes the
        # plain loop, which is a tested path too (the comparison leaves no query out)
        sl_ok = T["ray_ok"].copy()
        for name in ("length", "mixed"):
            sl_ok[T["where"][name]] = False
        assert not sl_ok.any(), tag
        print("walk probe: %s k %d %s: d.d = 4^k a0 is outside (1e-29, 1e29), no ray of ordinary length may walk; %d of %d queries (strays of the "
              "length and mixed classes) walk, the rest take the plain loop" % (tag + (int(np.count_nonzero(ok)), len(q))))
        return False
    assert ok.any(), tag
    closest, shadow = q[:, 0] == 0, q[:, 0] == 1
    kinds = wp.kinds_of(T["case"])[T["gl_idx"]]
    # GL's sphere test refuses disc < 1e-8, an absolute bound, and disc = a r^2 - (a |oc|^2 - hb^2) <= a r^2.  A ray of ordinary length
    # has a = 4^k (directions scaled with the scene) or 1, the largest sphere r = 1.5 * 2^k: where a r^2 < 1e-8 (k <= -7 scaled, k <= -14
    # at unit length) no sphere can answer such a ray
    r_max = max(abs(o["size"]["x"]) for o in T["case"]["doc"]["objects"] if o["type"] in ("sphere", "sphere_light"))
    a_family = 4.0 ** k if (fam == "similar" and scene_name in wp.SCALED_SCENES) else 1.0
    sphere_can = a_family * r_max * r_max >= 1e-8
    if not sphere_can:
        print("walk probe: %s k %d %s: a r^2 < 1e-8 for rays of ordinary length and every sphere: GL's disc < 1e-8 lets no sphere answer them" % tag)
    for code, what in ((0, "sphere"), (2, "box"), (3, "miss")):
        if code == 0 and not sphere_can:
            continue
        assert np.any(ok & closest & (kinds == code)), (tag, "no walked closest query with the answer", what)
    blocked = T["gl_idx"] == 1
    assert np.any(ok & shadow & ~blocked), (tag, "no walked occluded query that is not blocked")
    # what the planes and what the finite objects do to an occluded query: the same query in the scene without its planes, and the
    # plane test of the reference on the numbers (|d_y| >= 1e-6, t = (p_y - o_y) / d_y in [0.001, tmax])
    bare = wp.case_of("bvh-noplanes", k) if scene_name in wp.SCALED_SCENES else None
    if bare is not None:
        sel = np.flatnonzero(ok & shadow)
        by_finite = wp.ref_queries(bare, q[sel])[0] == 1
        planes_y = [o["position"]["y"] for o in T["case"]["doc"]["objects"] if o["type"] == "plane"]
        by_plane = np.zeros(len(sel), bool)
        with np.errstate(all="ignore"):
            for py in planes_y:
                t = (py - q[sel, 2]) / q[sel, 5]
                by_plane |= (np.abs(q[sel, 5]) >= 1e-6) & (t >= 0.001) & (t <= q[sel, 8])
        assert np.array_equal(by_finite | by_plane, blocked[sel]), tag  # the two parts make the whole
        assert np.any(by_finite & ~by_plane), (tag, "no walked occluded query blocked by a finite object alone")
        # (GL's plane test refuses |d_y| < 1e-6, an absolute bound: directions scaled by 2^k with k <= -20 never meet a plane)
        if planes_y and (2.0 ** k if fam == "similar" else 1.0) >= 1e-6:
            assert np.any(by_plane & ~by_finite), (tag, "no walked occluded query blocked by a plane alone")
    if scene_name in wp.SCALED_SCENES and fam == "unit" and k >= 60:
        floor = T["bounds"]["dir_floor"]
        with np.errstate(all="ignore"):
            low = np.any(np.abs(T["rays"][:, 3:6]) < floor, axis=1)
        hits = np.isin(wp.kinds_of(T["case"])[T["idx0"]], (0, 2))
        assert np.any(T["ray_ok"] & low & hits), (tag, "no walked ray with a component below dir_floor hits a finite object")
        with np.errstate(all="ignore"):
            f32 = np.abs(T["rays"][:, 3:6].astype(np.float32))
        tiny = np.any((f32 > 0) & (f32 < np.float32(floor)), axis=1)
        print("walk probe: %s k %d %s: %d walked rays below dir_floor = %.3g hit a finite object, %d of them with a non-zero FP32 component"
              % (scene_name, k, fam, np.count_nonzero(T["ray_ok"] & low & hits), floor, np.count_nonzero(T["ray_ok"] & tiny & hits)))
        if k >= 61:  # (B = 2^61 on: a component of 2^-60 is below the floor, pt_bvh.h)
            assert np.any(T["ray_ok"] & tiny & hits), tag
    return True


@pytest.mark.parametrize("k", wp.K + (0,))
def test_host_walk_equals_the_reference_loop_and_the_tables_are_not_hollow(k):
    for scene_name, kk in wp.scene_list(k):
        for fam in wp.families(scene_name, kk):
            T = wp.table(scene_name, kk, fam)
            walks = _conditions(scene_name, kk, fam, T)
            idx, t, deepest = wp.host_answers(T)  # (asserts walked / plain per query against numpy's walk_ok)
            assert deepest <= T["info"]["stack_need"], (scene_name, kk, fam, deepest, T["info"])
            if walks:
                assert deepest >= 1
                inside, outside = _edge_sides(T)
                if np.isfinite(T["bounds"]["clip_bound"]):
                    assert inside >= 12 and outside >= 12, (scene_name, kk, fam, inside, outside)  # the edge origins straddle the bound
            bad = 0
            for col, what in ((0, "the product's loop"), (1, "the tree policy")):
                wrong = np.flatnonzero((idx[:, col] != T["gl_idx"]) | ~wp.same_t(t[:, col], T["gl_t"]))
                bad += len(wrong)
                assert len(wrong) == 0, (scene_name, kk, fam, what, len(wrong), [(int(i), T["q"][i].tolist(), int(idx[i, col]), int(T["gl_idx"][i]),
                                                                                 float(t[i, col]), float(T["gl_t"][i])) for i in wrong[:3]])
            print(wp.report_line("host", scene_name, kk, fam, T, np.count_nonzero(T["ok"]), bad))


def test_ties_table_holds_every_kind_of_tie():
    T = wp.table("ties", 0, "unit")
    with wp.gw.Host(T["case"]) as h:
        census = h.tie_census(T["q"])
    assert min(census.values()) > 0, census


@pytest.mark.parametrize("k", wp.FRAME_K)
def test_the_reference_frames_of_the_frame_level_item_trace_past_the_first_hit(k):
    """The frame-level item of test_walk_probe_gpu.py compares whole frames at these scales; a frame whose paths end at their first
    hit and cast no shadow ray would ask the walk nothing beyond primary rays."""
    for moved in (False, True):
        case = wp.frame_case(k, moved)
        _, _, st = wp.gw.reference(case)
        assert st["segments"] > st["paths"] and st["shadow_rays"] > 0, (k, moved, st)


def test_host_program_on_the_deepest_tree_plain_and_under_the_sanitizers():
    rows = wp.deep_scene_rows()
    q = wp.deep_queries(rows)
    assert len(rows) == 300
    plain = wp.run_host(wp.build_host(), rows, q)
    built, stack_need, deepest, walked, plain_n = plain["info"]
    assert built == 1 and walked == len(q) and plain_n == 0, plain["info"]
    assert 8 <= deepest <= stack_need < 96, plain["info"]  # a deep tree, walked to the bottom
    assert np.array_equal(plain["idx"][:, 0], plain["idx"][:, 1]) and np.all(wp.same_t(plain["t"][:, 0], plain["t"][:, 1]))
    assert np.count_nonzero(plain["idx"][q[:, 0] == 0, 0] >= 0) > 10 and np.count_nonzero(plain["idx"][q[:, 0] == 1, 0] == 1) > 10
    san = wp.run_host(wp.build_host(("-fsanitize=address,undefined", "-fno-sanitize-recover=all"), "walk_host_probe_san"), rows, q)  # stderr must be empty
    assert san["info"] == plain["info"] and np.array_equal(san["idx"], plain["idx"]) and np.all(wp.same_t(san["t"], plain["t"]))
