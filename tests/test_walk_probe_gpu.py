"""The fog and GL tree walks ray by ray on the MI355X: tests/walk_probe.hip calls the product's own routines (ptg::TreeWorld of
csrc/pt_gl_walk.h with the lane's LDS stack column; wave_walk_coop, wave_any_hit and wave_any_hit_plain of csrc/pt_fog_walk.h) on the
tables of walk_probe_support.py and every answer is held to the plain loops of tests/glshade_reference.c and tests/fog_reference.c,
exactly: the product's headers claim the loop's bits.  test_walk_probe_cpu.py shows without a GPU that the tables reach what they
are for.  One frame-level item renders the rescaled scene through the library, because the probe's tree is built on the host."""
from __future__ import annotations

import numpy as np
import pytest

import walk_probe_support as wp

pytestmark = pytest.mark.gpu
GLC = ("paths", "segments", "shadow_rays", "probe_rays", "draws")


@pytest.mark.parametrize("k", wp.K + (0,))
def test_gl_queries_equal_the_reference_loop(k):
    """probe_gl_queries, one launch per (scene, family): index, t and the blocked flag equal gr_queries for every query; walked /
    plain per query equals the host build's (= numpy's walk_ok, which wp.host_answers holds the host build to); the deepest stack of
    every lane is within stack_need; a walked query visits between 1 node and all of them."""
    for scene_name, kk in wp.scene_list(k):
        with wp.Device(wp.case_of(scene_name, kk)) as dev:
            info, bounds = dev.info()
            for fam in wp.families(scene_name, kk):
                T = wp.table(scene_name, kk, fam)
                tag = (scene_name, kk, fam)
                assert info["built"] == 1 and info["gl_ok"] == 1 and bounds == T["bounds"], (tag, info, bounds)
                assert all(info[n] == T["info"][n] for n in ("main_nodes", "main_objs", "stack_need", "planes", "world")), (tag, info, T["info"])
                assert info["bvh_stack"] == max(4, (info["stack_need"] + 1 + 3) // 4 * 4)
                idx, t, wc = dev.gl_queries(T["q"])
                q, ok = T["q"], T["ok"]
                closest = q[:, 0] == 0
                wrong = np.flatnonzero((idx != T["gl_idx"]) | ~wp.same_t(t, T["gl_t"]))
                walked = np.where(closest, wc[:, 0], wc[:, 2])
                plain = np.where(closest, wc[:, 1], wc[:, 3])
                print(wp.report_line("device", scene_name, kk, fam, T, np.count_nonzero(walked), len(wrong)))
                assert len(wrong) == 0, (tag, len(wrong), [(int(i), q[i].tolist(), int(idx[i]), int(T["gl_idx"][i]), float(t[i]), float(T["gl_t"][i]))
                                                           for i in wrong[:3]])
                assert np.array_equal(walked, ok.astype(np.uint32)) and np.array_equal(plain, (~ok).astype(np.uint32)), \
                    (tag, "walked / plain per lane", int(np.count_nonzero(walked != ok)))
                host_idx, host_t, _ = wp.host_answers(T)  # (walked / plain of the host build = ok, or it fails there)
                assert np.array_equal(idx, host_idx[:, 1]) and np.all(wp.same_t(t, host_t[:, 1])), tag
                assert np.all(np.where(closest, wc[:, 2] + wc[:, 3] + wc[:, 5], wc[:, 0] + wc[:, 1] + wc[:, 4]) == 0), tag  # nothing of the other kind
                assert int(wc[:, 6].max()) <= info["stack_need"], (tag, int(wc[:, 6].max()), info)
                assert np.all(wc[~ok, 4:7] == 0), tag
                visits = np.where(closest, wc[:, 4], wc[:, 5])
                assert int(visits.max()) <= info["main_nodes"], (tag, int(visits.max()), info)
                # (an occluded query that a plane answers returns before the tree)
                must_visit = ok & (closest | (T["gl_idx"] == 0))
                assert np.all(visits[must_visit] >= 1), tag
                if wp.band_walks(scene_name, kk, fam):
                    assert int(wc[:, 6].max()) >= 1 and np.count_nonzero(walked) > 1000, tag


def _masked(T):
    """The table's fog turns under every lane mask, back to back: (rays [7 m][7], active u8 [7 m], {mask: slice})."""
    n = len(T["fog"])
    rays = np.ascontiguousarray(np.tile(T["fog"], (len(wp.MASKS), 1)))
    active = np.concatenate([np.tile(wp.mask_lanes(m), n // 64) for m in wp.MASKS]).astype(np.uint8)
    return rays, active, {m: slice(j * n, (j + 1) * n) for j, m in enumerate(wp.MASKS)}


@pytest.mark.parametrize("k", wp.K + (0,))
def test_fog_turns_equal_the_reference_loop_under_every_lane_mask(k):
    """probe_fog_turns, one launch per (scene, family) with every mask: an active lane's `blocked` equals fr_occluded_many and its
    answer in the full wave, an idle lane reports blocked, a wave's coop equals "every active lane passes" of numpy's restatement of
    wave_walk_coop, a wave without an active lane writes nothing but blocked, the wave's deepest stack is within stack_need."""
    for scene_name, kk in wp.scene_list(k):
        with wp.Device(wp.case_of(scene_name, kk)) as dev:
            info, _ = dev.info()
            for fam in wp.families(scene_name, kk):
                T = wp.table(scene_name, kk, fam)
                tag = (scene_name, kk, fam)
                rays, active, where = _masked(T)
                blocked, waves = dev.fog_turns(rays, active)
                n = len(T["fog"])
                full = blocked[where["full"]]
                bad_total = 0
                for m in wp.MASKS:
                    sl = where[m]
                    act = active[sl] != 0
                    b = blocked[sl]
                    wrong = np.flatnonzero(act & (b != T["fog_blocked"]))
                    bad_total += len(wrong)
                    assert len(wrong) == 0, (tag, m, len(wrong), [(int(i), T["fog"][i].tolist(), int(b[i]), int(T["fog_blocked"][i])) for i in wrong[:3]])
                    assert np.array_equal(b[act], full[act]), (tag, m)
                    assert np.all(b[~act] == 1), (tag, m)
                    w = waves[sl.start // 64:sl.stop // 64]
                    if m == "empty":
                        assert np.all(w == 0xFFFFFFFF), (tag, m)  # the wave returned before its outputs
                        continue
                    coop = np.all((T["fog_pass"] | ~act).reshape(-1, 64), axis=1)
                    assert np.array_equal(w[:, 0], coop.astype(np.uint32)), (tag, m, int(np.count_nonzero(w[:, 0] != coop)))
                    assert np.all(w[~coop, 1:3] == 0), (tag, m)
                    assert int(w[:, 2].max()) <= info["stack_need"] and int(w[:, 1].max()) <= info["main_nodes"], (tag, m, info)
                    if m == "full":
                        # the mixed class: a wave that holds one odd ray reports coop = 0 and still answers every lane (above)
                        mixed = T["where"]["mixed"]
                        mw = coop[mixed.start // 64:mixed.stop // 64]
                        if wp.band_walks(scene_name, kk, fam):
                            assert np.count_nonzero(~mw) >= 6 and np.count_nonzero(coop) >= 10, (tag, int(np.count_nonzero(~mw)), int(np.count_nonzero(coop)))
                            assert int(w[:, 1].max()) >= 1 and int(w[:, 2].max()) >= 1, tag  # the tree was walked, and more than one child deep
                print("walk probe: fog        on %-12s k %4d %-7s: %d rays x %d masks, full waves coop %d / plain %d, blocked %d, disagreements %d"
                      % (scene_name, kk, fam, n, len(wp.MASKS), int(np.count_nonzero(waves[:n // 64, 0] == 1)), int(np.count_nonzero(waves[:n // 64, 0] == 0)),
                         int(np.count_nonzero(full)), bad_total))


# ---------------------------------------------------------------- the frame-level item: the tree built and refitted on the device
@pytest.fixture(scope="module")
def _torch_before_libptcore():
    import torch  # noqa: F401  (one HIP runtime in the process, as in test_glshade_walk_gpu.py)


def _render(ctx, case, **kw):
    from path_trace_golang_amd import hip

    w, h, p, depth, seed = case["cfg"]
    img, acc = np.zeros((h, w, 4), np.uint8), np.zeros((h, w, 3))
    hip.render(case["sc"], hip.RenderConfig(w, h, p, depth, seed, 0, 0), img, None, acc, ctx=ctx, shading="gl", shading_walk=True, **kw)
    return img, hip.shading_last_stats(ctx)


def _holds(case, got, tag):
    ref_img, _, ref_st = wp.gw.reference(case)
    img, gst = got
    assert np.array_equal(img, ref_img), (tag, int(np.count_nonzero(img != ref_img)))
    assert tuple(gst[c] for c in GLC) == tuple(ref_st[c] for c in GLC), (tag, gst, ref_st)


@pytest.mark.parametrize("k", wp.FRAME_K)
def test_scaled_frames_with_a_device_built_and_a_refitted_tree_equal_the_reference(k, _torch_before_libptcore):
    from path_trace_golang_amd import capi, hip

    case, moved = wp.frame_case(k), wp.frame_case(k, moved=True)
    assert case["cfg"] == (33, 20, 1, 3, 7)
    with capi.Context(ndev=1) as ctx:
        _holds(case, _render(ctx, case, bvh_build="device"), ("device build", k))
        assert hip.bvh_build_stats(ctx)["device_builds"] >= 1
        ws = hip.shading_walk_stats(ctx)
        assert ws["closest_walked"] > 0 and ws["shadow_walked"] > 0, ws
    with capi.Context(ndev=1) as ctx:
        _render(ctx, case, bvh_refit=1.25)
        got = _render(ctx, moved, bvh_refit=1.25)
        assert hip.bvh_refit_stats(ctx)["last_action"] == 2  # it was a refit
        _holds(moved, got, ("refit", k))
