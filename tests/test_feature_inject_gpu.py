"""Injected rays through feature_bvh_kernel (csrc/pt_feature_walk.h), record by record against the oracle.

The kernel's walk is the function primary_bvh_kernel calls (csrc/pt_wave_walk.h), and test_feature_walk_gpu.py feeds it camera rays:
coherent waves of unit directions.  Here the seven tables of feature_inject_support.py -- direction lengths over 1200 binades, zero and denormal components,
origins on the geometry and around every bound, incoherent waves, waves with one odd lane, exactly axis-parallel rays beside many
cores -- go through it on the 341-object scene of ray_inject_support.py, in their own layout (one odd lane in most waves: the plain
scan) and in walk_layout (the degenerate rays in whole waves: the walk).  Every ray's normal, albedo, distance, hit flag and id is the
oracle's (tests/atrous_reference.c, tests/object_ids_reference.c), bit for bit, tied rows included; a record with a NaN or an infinity
must have the oracle's hit flag, id and non-finite fields.  pt_feature_walk_stats must say what the layout says.  No tolerance."""
import math

import numpy as np
import pytest

import feature_inject_support as fi
import ray_inject_support as S

pytestmark = pytest.mark.gpu

_cache = {}


@pytest.fixture(scope="module")
def ctx(gpu_ctx):
    c = fi.context_with({})
    yield c
    c.close()


def _scene(key="bvh", doc=None):
    """(doc, product scene, oracle scene) under `key`."""
    from path_trace_golang_amd import scene

    if key not in _cache:
        doc = doc if doc is not None else S.scene_doc("bvh")
        assert S.scene_bound(doc) == S.BOUND
        _cache[key] = (doc, scene.Scene.decode(doc), fi.ora_scene(doc, key=key))
    return _cache[key]


def _default_frame(ctx, name, layout):
    """The default context's frame of a table, held to the oracle; (frame, counts).  Rendered once per (class, layout)."""
    key = ("frame", name, layout)
    if key not in _cache:
        _, sc, osc = _scene()
        table, plain = fi.laid_out(name, layout)
        o = fi.oracle_records(osc, table, key=("bvh", name, layout))
        f = fi.render_features(ctx, sc, table)
        counts = fi.compare_frame(f, o, table, (name, layout))
        fi.assert_walk_stats(f["stats"], S.NWAVES, plain, (name, layout))
        _cache[key] = (f, counts)
    return _cache[key]


# ---------------------------------------------------------------- A4
@pytest.mark.parametrize("layout", fi.LAYOUTS)
@pytest.mark.parametrize("name", fi.CLASS_NAMES)
def test_every_class_matches_the_oracle_record_by_record(ctx, oracle, name, layout):
    table, plain = fi.laid_out(name, layout)
    f, counts = _default_frame(ctx, name, layout)
    print(fi.report_line("%s, %s layout" % (name, layout), counts, f["stats"]))
    if layout == "walk":
        assert S.NWAVES - plain >= fi.MIN_WALKED[name]
    # the rows a NaN or an infinity excuses are odd rays, all of them: no ray the walk took is excused
    o = fi.oracle_records(_scene()[2], table, key=("bvh", name, layout))
    assert not np.any(o["nonfinite"] & ~fi.walk_odd(table))
    assert counts["nonfinite"] == {"length": 153, "far origins": 126, "mixed": 127}.get(name, 0)
    assert 0 < counts["hits"] < counts["rays"] and (counts["ties"] > 0 or name == fi.NAMED)


# ---------------------------------------------------------------- A5
RW, RH, RSPP = 33, 31, 3


def _ragged_check(ctx, rays, plain, tag):
    _, sc, osc = _scene()
    o = fi.oracle_records(osc, rays)
    want = fi.expected_planes(o["rec"], RW, RH, RSPP)
    want_ids = o["ids"].reshape(RH, RW, RSPP)[:, :, 0]
    waves = ((RW + 7) // 8) * ((RH + 7) // 8) * RSPP
    for chunk in (2, 0):
        f = fi.render_features(ctx, sc, rays, RW, RH, RSPP, k=RSPP, chunk=chunk)
        assert fi.planes_differ(f["feats"], want) == [0, 0, 0], (tag, chunk, fi.planes_differ(f["feats"], want))
        assert np.array_equal(f["ids"], want_ids), (tag, chunk, int(np.count_nonzero(f["ids"] != want_ids)))
        fi.assert_walk_stats(f["stats"], waves, plain, (tag, chunk))
        counts = dict(rays=len(rays), hits=int(np.count_nonzero(o["rec"][:, 0])), ties=int(np.count_nonzero(o["tie"])),
                      nonfinite=int(np.count_nonzero(o["nonfinite"])))
        print(fi.report_line("%s, chunk %d" % (tag, chunk), counts, f["stats"]))
    assert np.all(want[2][..., 2] == RSPP) and 0 < want[2][..., 1].sum() < RW * RH * RSPP and counts["ties"] > 0


def test_three_samples_on_a_ragged_frame_add_up_in_sample_order(ctx, oracle):
    """33 x 31 pixels (edge waves hold lanes outside the frame), three independent rays per pixel, chunks of two and one chunk: the
    planes are the oracle's records added in sample order, the ids those of sample 0.  Then sample 1 of one block becomes odd."""
    rays = S.indexing_rays(RW, RH, RSPP)
    assert not fi.walk_odd(rays).any()
    _ragged_check(ctx, rays, 0, "33x31x3")
    odd = rays.copy().reshape(RH, RW, RSPP, 6)
    blk = odd[16:24, 8:16, 1]             # one whole 8 x 8 block, sample 1
    blk[0:4, :, 3:6] *= 1e20              # a = 1e40
    blk[4:6, :, 3:6] *= 1e-20             # a = 1e-40
    blk[6:8, :, 0:3] = blk[6:8, :, 0:3] - blk[6:8, :, 3:6] * (30.0 * S.BOUND)  # origins thirty scene sizes away, looking the same way
    odd = np.ascontiguousarray(odd.reshape(-1, 6))
    mask = fi.walk_odd(odd).reshape(RH, RW, RSPP)
    assert mask.sum() == 64 and mask[16:24, 8:16, 1].all()
    _ragged_check(ctx, odd, 1, "33x31x3, one block's sample 1 odd")


# ---------------------------------------------------------------- A6
@pytest.mark.parametrize("env", [{"PTCORE_PIPELINE": "wavefront"}, {"PTCORE_PRIMARY": "lane"}, {"PTCORE_SCAN": "verify_bvh"}],
                         ids=["wavefront", "primary_lane", "verify_bvh"])
def test_the_other_trace_forms_give_the_default_contexts_planes(ctx, oracle, env):
    _, sc, osc = _scene()
    other = fi.context_with(env)
    try:
        for name in ("components", "incoherent"):
            table, plain = fi.laid_out(name, "walk")
            want, counts = _default_frame(ctx, name, "walk")
            f = fi.render_features(other, sc, table)
            assert fi.planes_differ(f["feats"], want["feats"]) == [0, 0, 0] and np.array_equal(f["ids"], want["ids"]), (env, name)
            fi.compare_frame(f, fi.oracle_records(osc, table, key=("bvh", name, "walk")), table, (env, name))
            fi.assert_walk_stats(f["stats"], S.NWAVES, plain, (env, name))
            print(fi.report_line("%s, walk layout, %s" % (name, "=".join(*env.items())), counts, f["stats"]))
    finally:
        other.close()


# ---------------------------------------------------------------- A7
def test_a_refitted_tree_gives_the_oracles_records_of_the_edited_scene(oracle):
    from path_trace_golang_amd import hip

    doc, sc, _ = _scene()
    edit, idx = fi.edited_doc(doc)
    assert len(idx) == 40 and min(idx) >= len(S.PROBES)
    kinds = {doc["objects"][i]["type"] for i in idx}
    assert {"sphere", "box"} <= kinds
    assert all(edit["objects"][i]["type"] == doc["objects"][i]["type"] and edit["objects"][i]["material_id"] == doc["objects"][i]["material_id"]
               and edit["objects"][i]["position"] != doc["objects"][i]["position"] and edit["objects"][i]["size"] != doc["objects"][i]["size"]
               for i in idx)
    _, esc, eosc = _scene("bvh, edited", edit)  # (the bound is still B: the tables' classification holds)
    refit = fi.context_with({})
    try:
        hip.set_bvh_refit(refit, math.inf)
        fi.render_features(refit, sc, None)
        st = hip.bvh_refit_stats(refit)
        assert (st["builds"], st["refits"]) == (1, 0)
        changed = 0
        for name in ("incoherent", "components"):
            table, plain = fi.laid_out(name, "walk")
            o = fi.oracle_records(eosc, table, key=("bvh, edited", name, "walk"))
            f = fi.render_features(refit, esc, table)
            counts = fi.compare_frame(f, o, table, ("refitted", name))
            fi.assert_walk_stats(f["stats"], S.NWAVES, plain, ("refitted", name))
            st = hip.bvh_refit_stats(refit)
            assert (st["builds"], st["refits"]) == (1, 1), st
            changed += int(np.count_nonzero(o["ids"] != fi.oracle_records(_scene()[2], table, key=("bvh", name, "walk"))["ids"]))
            print(fi.report_line("%s, walk layout, refitted tree" % name, counts, f["stats"]))
        assert changed > 50  # the edit is seen: rays whose winner is another object than before
    finally:
        refit.close()
