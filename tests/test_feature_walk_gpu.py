"""First-hit features on the BVH path on the MI355X (pt_set_feature_walk, feature_bvh_kernel / feature_bvh_adaptive_kernel,
pt_feature_walk_stats).  The references are those of the linear kernel's tests: the oracle through
tests/atrous_reference.c (planes) and tests/object_ids_reference.c (ids), feature_kernel itself on the scenes both kernels can take,
the restatements of the filter and of the accumulation downstream.  Frames are 40 x 24 (two tiles, the second ragged) and 37 x 21
(waves that hold out-of-frame lanes), 6 samples at depth 3 unless a case needs steps.  Every test turns the walk on, so none passes
without it."""
from __future__ import annotations

import ctypes as C
import json

import numpy as np
import pytest

import adaptive_support as ad
import atrous_support as at
import temporal_motion_support as tm
import temporal_support as ts
from conftest import render_vs_oracle, scene_path
from moments_support import H, W

pytestmark = pytest.mark.gpu

SPP, DEPTH = 6, 3
NOBJ = 300  # more than 128 spheres: the hierarchy, with several node levels, glass, emitters and a thin lens
_cache = {}


@pytest.fixture(autouse=True, scope="module")
def _built(gpu_ctx):
    return gpu_ctx


def _big():
    """(product scene, oracle scene) of synth.make_scene(NOBJ); the oracle scene is kept alive (ref_features caches by its id)."""
    if "big" not in _cache:
        from oracle import ora
        from path_trace_golang_amd import synth

        sc = synth.make_scene(NOBJ)
        _cache["big"] = (sc, ora.Scene(sc.encode()))
    return _cache["big"]


def _shipped(name):
    from oracle import ora
    from path_trace_golang_amd import scene

    if name not in _cache:
        with open(scene_path(name), "r", encoding="utf-8") as fh:
            doc = json.load(fh)
        _cache[name] = (scene.Scene.decode(doc), ora.Scene(doc), doc)
    return _cache[name]


def _frame(ctx, sc, w, h, spp, depth, k, seed=1, chunk=0, walk=True, **kw):
    """One frame with moments, k feature samples and object ids on: dict(img, accum, m2, feats, ids, st)."""
    from path_trace_golang_amd import hip

    img, acc, m2 = np.zeros((h, w, 4), np.uint8), np.zeros((h, w, 3)), np.zeros((h, w, 3))
    st = hip.render(sc, hip.RenderConfig(w, h, spp, depth, seed, chunk), img, None, acc, ctx=ctx, moments=m2, features=k, object_ids=k > 0,
                    feature_walk=walk, **kw)
    out = dict(img=img, accum=acc, m2=m2, st=st, feats=None, ids=None)
    if k > 0:
        out["feats"] = tuple(np.full((h, w, 3), -7.0) for _ in range(3))
        hip.read_features(ctx, *out["feats"])
        out["ids"] = np.full((h, w), -9, np.int32)
        hip.read_object_ids(ctx, out["ids"])
    return out


def _same_feats(a, b):
    return all(at.same_bits(x, y) for x, y in zip(a, b))


def _diffs(a, b):
    return [int(np.count_nonzero(np.ascontiguousarray(x).view(np.uint64) != np.ascontiguousarray(y).view(np.uint64))) for x, y in zip(a, b)]


def _waves(w, h):
    """8 x 8 blocks with a pixel inside a w x h frame: the waves that take part in a feature pass."""
    return ((w + 7) // 8) * ((h + 7) // 8)


# ---------------------------------------------------------------- 1. against the oracle on a real tree
@pytest.mark.parametrize("k,size", [(1, (W, H)), (4, (W, H)), (40, (W, H)), (4, (37, 21))])
def test_planes_and_ids_match_the_oracle_on_a_tree(k, size):
    from path_trace_golang_amd import capi, hip

    w, h = size
    sc, osc = _big()
    assert sc.camera.aperture > 0 and sum(1 for o in sc.objects) >= NOBJ
    with capi.Context(ndev=1) as ctx:
        f = _frame(ctx, sc, w, h, SPP, DEPTH, k)
        stats = hip.feature_walk_stats(ctx)
        plain = _frame(ctx, sc, w, h, SPP, DEPTH, 0, walk=False)
    want = at.ref_features(osc, w, h, SPP, DEPTH, 1, k)
    assert _diffs(f["feats"], want) == [0, 0, 0], (k, size, _diffs(f["feats"], want))
    assert np.all(f["feats"][2][..., 2] == min(k, SPP)) and f["feats"][2][..., 1].max() > 0
    ids, tie = tm.oracle_ids(osc, w, h, 1)
    assert not tie.any() and np.array_equal(f["ids"], ids), int(np.count_nonzero(f["ids"] != ids))
    assert len(np.unique(ids)) > 4 and ids.max() < len(sc.objects)
    print("feature walk, k = %d, %d x %d: %s" % (k, w, h, stats))
    # every wave walks every feature sample (camera rays are tame), visits more than the root, and pushes at least once
    assert stats["walked"] == _waves(w, h) * min(k, SPP) and stats["plain"] == 0
    assert stats["node_visits"] > stats["walked"] and 1 <= stats["deepest_stack"] < 96
    assert np.array_equal(f["img"], plain["img"]) and at.same_bits(f["accum"], plain["accum"])  # the frame itself is untouched


# ---------------------------------------------------------------- 2. against the linear kernel
@pytest.mark.parametrize("name,depth", [("gpu_showcase", 8), ("metal_glass_room", 6)])
def test_the_walk_gives_the_planes_of_the_linear_kernel(monkeypatch, name, depth):
    from path_trace_golang_amd import capi, hip

    sc, osc, _ = _shipped(name)
    with capi.Context(ndev=1) as linear:  # the default scan: feature_kernel (the walk's setting is ignored there)
        a = _frame(linear, sc, W, H, SPP, depth, 4, walk=False)
        monkeypatch.setenv("PTCORE_SCAN", "bvh")  # read by pt_create
        with capi.Context(ndev=1) as walked:
            b = _frame(walked, sc, W, H, SPP, depth, 4)
            stats = hip.feature_walk_stats(walked)
        with pytest.raises(capi.PtError, match="did not run the walk"):
            hip.feature_walk_stats(linear)
    assert stats["walked"] == _waves(W, H) * 4 and stats["plain"] == 0
    assert _diffs(a["feats"], b["feats"]) == [0, 0, 0] and np.array_equal(a["ids"], b["ids"])
    assert _same_feats(b["feats"], at.ref_features(osc, W, H, SPP, depth, 1, 4))
    assert np.array_equal(a["img"], b["img"])


# ---------------------------------------------------------------- 3. invariance, bit for bit
INV_SPP, INV_K = 16, 6  # chunks of 3 and 5 cut the six feature samples at different places


@pytest.fixture(scope="module")
def inv_ref(_built):
    from path_trace_golang_amd import capi

    sc, osc = _big()
    with capi.Context(ndev=1) as ctx:
        f = _frame(ctx, sc, W, H, INV_SPP, DEPTH, INV_K)
    assert _same_feats(f["feats"], at.ref_features(osc, W, H, INV_SPP, DEPTH, 1, INV_K))
    assert _same_feats(f["feats"], at.ref_features(osc, W, H, SPP, DEPTH, 1, INV_K))  # ... which are case 1's: the first six samples
    return f


@pytest.mark.parametrize("chunk", [3, 5])
def test_planes_do_not_depend_on_the_chunk(inv_ref, chunk):
    from path_trace_golang_amd import capi

    with capi.Context(ndev=1) as ctx:
        f = _frame(ctx, _big()[0], W, H, INV_SPP, DEPTH, INV_K, chunk=chunk)
    assert f["st"]["spp_chunk"] == chunk and _same_feats(f["feats"], inv_ref["feats"]) and np.array_equal(f["ids"], inv_ref["ids"])
    assert np.array_equal(f["img"], inv_ref["img"]) and at.same_bits(f["m2"], inv_ref["m2"])


@pytest.mark.parametrize("step", [1, 7])
def test_planes_do_not_depend_on_the_steps(inv_ref, step):
    from path_trace_golang_amd import capi, hip

    sc, osc = _big()
    L = capi.load()
    flat = hip.FlatScene(sc)
    pc = hip.pt_config(hip.RenderConfig(W, H, INV_SPP, DEPTH, 1))
    feats = tuple(np.zeros((H, W, 3)) for _ in range(3))
    ids = np.full((H, W), -9, np.int32)
    with capi.Context(ndev=1) as ctx:
        hip.set_moments(ctx, True)
        hip.set_feature_walk(ctx, True)
        hip.set_features(ctx, INV_K)
        hip.set_object_ids(ctx, True)
        capi.check(L.pt_begin(ctx.handle, C.byref(flat.c), C.byref(pc)))
        done = C.c_int32(0)
        while done.value < INV_SPP:
            capi.check(L.pt_step(ctx.handle, step, C.byref(done)))
            if done.value == step:  # between steps the planes hold the samples done so far
                hip.read_features(ctx, *feats)
                assert _same_feats(feats, at.ref_features(osc, W, H, min(step, INV_SPP), DEPTH, 1, INV_K))
                hip.read_object_ids(ctx, ids)
                assert np.array_equal(ids, inv_ref["ids"])
        capi.check(L.pt_end(ctx.handle, None))
        hip.read_features(ctx, *feats)
        stats = hip.feature_walk_stats(ctx)
    assert _same_feats(feats, inv_ref["feats"]) and stats["walked"] == _waves(W, H) * INV_K


@pytest.mark.parametrize("env", [{"PTCORE_PIPELINE": "wavefront"}, {"PTCORE_PIPELINE": "walk32"}, {"PTCORE_PRIMARY": "lane"},
                                 {"PTCORE_SCAN": "verify_bvh"}], ids=["wavefront", "walk32", "primary_lane", "verify_bvh"])
def test_planes_do_not_depend_on_the_trace_form(monkeypatch, inv_ref, env):
    from path_trace_golang_amd import capi

    for key, v in env.items():
        monkeypatch.setenv(key, v)
    with capi.Context(ndev=1) as ctx:  # read by pt_create
        f = _frame(ctx, _big()[0], W, H, INV_SPP, DEPTH, INV_K)
    assert _same_feats(f["feats"], inv_ref["feats"]) and np.array_equal(f["ids"], inv_ref["ids"]) and np.array_equal(f["img"], inv_ref["img"])


def test_four_virtual_devices_give_the_planes_of_one(inv_ref):
    from path_trace_golang_amd import capi, hip

    sc, osc = _big()
    w, h = ad.GATHER_W, ad.GATHER_H  # 70 x 45: 6 tiles = 2, 2, 1, 1
    with capi.Context(devices=[0, 0, 0, 0]) as four:
        small = _frame(four, sc, W, H, INV_SPP, DEPTH, INV_K)  # two tiles: two of the devices hold none
        s_small = hip.feature_walk_stats(four)
        f = _frame(four, sc, w, h, SPP, DEPTH, 4)
        stats = hip.feature_walk_stats(four)
        assert f["st"]["num_devices"] == 4
    assert _same_feats(small["feats"], inv_ref["feats"]) and np.array_equal(small["ids"], inv_ref["ids"])
    assert s_small["walked"] == _waves(W, H) * INV_K
    assert _same_feats(f["feats"], at.ref_features(osc, w, h, SPP, DEPTH, 1, 4))
    assert np.array_equal(f["ids"], tm.oracle_ids(osc, w, h, 1)[0])
    assert stats["walked"] == _waves(w, h) * 4 and stats["plain"] == 0  # summed over the devices


# ---------------------------------------------------------------- 4. adaptive
def test_adaptive_blocks_hold_the_features_of_their_own_count():
    from path_trace_golang_amd import capi, hip

    sc, osc = _big()
    cap, step, k = 24, 8, 40
    with capi.Context(ndev=1) as ctx:
        # the target: the median block noise of the plain 8-sample frame, so that about half the blocks stop at the first check
        plain = _frame(ctx, sc, W, H, step, DEPTH, 0, walk=False)
        target = float(np.median(ad.block_noise_map(plain["accum"], plain["m2"], step)))
        hip.set_feature_walk(ctx, True)
        img, acc, m2, counts, _, _, st = ad.render_adaptive(ctx, sc, W, H, cap, DEPTH, 1, target, step, 0, features=k, object_ids=True,
                                                            feature_walk=True)
        feats = tuple(np.zeros((H, W, 3)) for _ in range(3))
        hip.read_features(ctx, *feats)
        ids = np.full((H, W), -9, np.int32)
        hip.read_object_ids(ctx, ids)
        stats = hip.feature_walk_stats(ctx)
    print("adaptive counts:", sorted(set(int(v) for v in np.unique(counts))), stats)
    assert len(np.unique(counts)) >= 2 and counts.min() >= step and counts.max() <= cap  # blocks stopped at different counts
    assert np.array_equal(feats[2][..., 2], np.minimum(k, counts).astype(np.float64))  # min(k, n) feature samples
    assert _diffs(feats, at.ref_features(osc, W, H, cap, DEPTH, 1, k, counts=counts)) == [0, 0, 0]
    assert np.array_equal(ids, tm.oracle_ids(osc, W, H, 1)[0])
    blocks = counts[::8, ::8].astype(np.int64)  # one wave per 8 x 8 block and sample it holds
    assert stats["walked"] == int(blocks.sum()) and stats["plain"] == 0


# ---------------------------------------------------------------- 5. the fallback: waves that hold an odd ray take the plain scan
def _injected(doc, spp):
    """A [W*H*spp][6] table of rays from the camera towards the scene's objects, with odd rays (the classification of
    primary_bvh_kernel: a direction whose squared length is outside 1e-29 .. 1e29, an origin beyond 3.5 scene sizes) in chosen 8 x 8
    blocks and samples; and the mask of the odd rows."""
    import ray_inject_support as ri

    bound = ri.scene_bound(doc)
    cam = doc["camera"]["position"]
    o = np.array([cam["x"], cam["y"], cam["z"]], float)
    centres = np.array([[ob["position"][a] for a in "xyz"] for ob in doc["objects"] if ob["type"] != "plane"], float)
    rng = np.random.default_rng(7)
    rays = np.zeros((H, W, spp, 6))
    for y in range(H):
        for x in range(W):
            for s in range(spp):
                c = centres[(y * W + x + 3 * s) % len(centres)] + rng.uniform(-0.3, 0.3, 3)
                d = c - o
                rays[y, x, s] = np.concatenate([o, d / np.linalg.norm(d)])
    rays[0:8, 0:8, 0, 3:6] *= 1e20        # a whole wave of long directions (a = 1e40), sample 0
    rays[0:8, 8:16, 1, 3:6] *= 1e-20      # ... of short ones (a = 1e-40), sample 1
    far = rays[8:16, 16:24, 0]            # ... of origins thirty scene sizes away, still aimed at the scene
    far[..., 0:3] = far[..., 0:3] - far[..., 3:6] * (30.0 * bound)
    rays[18, 35, 1, 3:6] *= 1e20          # one odd lane in a wave of the ragged tile
    rays[23, 39, 0, 3:6] *= 1e-20         # ... and the frame's last pixel
    table = np.ascontiguousarray(rays.reshape(W * H * spp, 6))
    a = ri.dir_a(table)
    odd = ~((a > 1e-29) & (a < 1e29)) | (ri.omax(table) > 3.5 * bound)
    return table, odd.reshape(H, W, spp)


def test_waves_with_an_odd_ray_take_the_plain_scan(monkeypatch):
    from path_trace_golang_amd import capi, hip

    name, depth, spp = "gpu_showcase", 4, 2
    sc, osc, doc = _shipped(name)
    table, odd = _injected(doc, spp)
    pairs = {(y // 8, x // 8, s) for y, x, s in zip(*np.nonzero(odd))}
    assert len(pairs) == 5 and int(odd.sum()) == 3 * 64 + 2
    with capi.Context(ndev=1) as linear:
        monkeypatch.setenv("PTCORE_SCAN", "bvh")  # read by pt_create
        with capi.Context(ndev=1) as walked:
            for ctx in (linear, walked):
                ctx.set_primary_rays(table)
            try:
                a = _frame(linear, sc, W, H, spp, depth, spp, walk=False)
                b = _frame(walked, sc, W, H, spp, depth, spp)
                stats = hip.feature_walk_stats(walked)
            finally:
                for ctx in (linear, walked):
                    ctx.set_primary_rays(None)
    print("injected rays:", stats)
    assert _diffs(a["feats"], b["feats"]) == [0, 0, 0] and np.array_equal(a["ids"], b["ids"])
    assert stats["plain"] == len(pairs) and stats["walked"] == _waves(W, H) * spp - len(pairs)
    want, tie = tm.oracle_ids_of_rays(osc, table.reshape(H * W, spp, 6)[:, 0])
    keep = ~tie & ~odd[..., 0].reshape(-1)  # (the oracle's ids for the rays the walk took)
    assert keep.sum() > W * H * 0.7 and len(np.unique(want[keep])) > 4
    assert np.array_equal(b["ids"].reshape(-1)[keep], want[keep])


# ---------------------------------------------------------------- 6. downstream: the filter, the accumulation, the motion table
def test_the_filter_takes_the_feature_terms_on_a_hierarchy_scene():
    from path_trace_golang_amd import capi, hip

    sc, osc = _big()
    assert not hip.scene_allows_features(sc) and hip.scene_allows_features(sc, feature_walk=True)
    with capi.Context(ndev=1) as ctx:
        f = _frame(ctx, sc, W, H, SPP, DEPTH, 0, walk=False)
        img = np.zeros((H, W, 4), np.uint8)
        st = hip.render(sc, hip.RenderConfig(W, H, SPP, DEPTH, 1), img, ctx=ctx, atrous=hip.AtrousConfig(), feature_walk=True)
        assert hip.feature_walk_stats(ctx)["walked"] == _waves(W, H) * 4  # k = 4: hip.render's choice where the scene allows features
        without = np.zeros((H, W, 4), np.uint8)
        hip.render(sc, hip.RenderConfig(W, H, SPP, DEPTH, 1), without, ctx=ctx, atrous=hip.AtrousConfig())
    feats = at.ref_features(osc, W, H, SPP, DEPTH, 1, 4)
    want = at.ref_filter(f["accum"], f["m2"], SPP, None, feats)
    assert np.array_equal(img, want["rgba"]) and st["atrous"]["iterations"] == 5
    assert np.array_equal(without, at.ref_filter(f["accum"], f["m2"], SPP, None, None)["rgba"]) and not np.array_equal(img, without)


def test_two_accumulated_frames_match_the_restatement_and_take_a_motion_table():
    from path_trace_golang_amd import capi, hip

    sc, osc = _big()
    cam = ts.camera_of(osc, W, H)
    ref = ts.Accumulator("ref")
    tcfg, flt = ts.temporal_config(), at.atrous_config()
    with capi.Context(ndev=1) as ctx:
        f0 = _frame(ctx, sc, W, H, SPP, DEPTH, 4, seed=1)
        got = ts.gpu_frame(ctx, tcfg, flt, W, H)
        ts.assert_same_frame(got, ref.frame(f0["accum"], f0["m2"], SPP, f0["feats"], cam, None, dict()), "frame 0")
        # the second frame through hip.render's temporal=: the restatement's frame
        f1 = _frame(ctx, sc, W, H, SPP, DEPTH, 4, seed=2, atrous=flt, temporal=tcfg)
        hm, hv, hl = np.zeros((H, W, 3)), np.zeros((H, W)), np.zeros((H, W), np.int32)
        hip.temporal_read(ctx, hm, hv, hl)
        # ... and a third with a motion table (object ids on, nothing moved): accepted
        f2 = _frame(ctx, sc, W, H, SPP, DEPTH, 4, seed=3, atrous=flt, temporal=tcfg, temporal_motion=np.zeros((len(sc.objects), 3)))
    want = ref.frame(f1["accum"], f1["m2"], SPP, f1["feats"], cam, None, dict())
    ref.close()
    t = f1["st"]["temporal"]
    assert f2["st"]["temporal"]["objects"] == len(sc.objects) and f2["st"]["temporal"]["moved"] == 0
    assert t["reprojected"] == want["reprojected"] and t["reprojected"] > W * H // 2
    assert np.array_equal(f1["img"], want["rgba"]), int(np.count_nonzero(f1["img"] != want["rgba"]))
    assert at.same_bits(hm, want["hist_mean"]) and at.same_bits(hv, want["hist_var"]) and np.array_equal(hl, want["hist_len"])


# ---------------------------------------------------------------- 7. state rules
PARENT_REFUSAL = ("features: not available for scenes on the BVH path (more than 128 spheres or 128 boxes): a linear scan per feature sample")


def test_state_rules_and_every_refusal_leaves_a_usable_context(oracle):
    from path_trace_golang_amd import capi, hip

    L = capi.load()
    sc, osc = _big()
    o = oracle.render(osc, W, H, 4, DEPTH, seed=1)
    flat = hip.FlatScene(sc)
    pc = hip.pt_config(hip.RenderConfig(W, H, 4, DEPTH, 1))
    out = (C.c_uint64 * 4)(7, 7, 7, 7)
    img = np.zeros((H, W, 4), np.uint8)
    with capi.Context(ndev=1) as ctx:
        assert L.pt_feature_walk_stats(ctx.handle, out) == capi.PT_ERR_STATE  # no frame yet
        assert L.pt_feature_walk_stats(ctx.handle, None) == capi.PT_ERR_INVALID
        # the walk off: the refusal as it was, word for word
        hip.set_moments(ctx, True)
        hip.set_features(ctx, 2)
        assert L.pt_begin(ctx.handle, C.byref(flat.c), C.byref(pc)) == capi.PT_ERR_INVALID
        assert L.pt_last_error().decode() == PARENT_REFUSAL
        render_vs_oracle(ctx, sc, o, W, H, 4, DEPTH, 1, tag="after the refusal", forms=("shipping",))
        # the walk on: accepted; the setter is refused while the frame is open
        hip.set_feature_walk(ctx, True)
        hip.set_moments(ctx, True)
        hip.set_features(ctx, 2)  # (hip.render said its own settings)
        capi.check(L.pt_begin(ctx.handle, C.byref(flat.c), C.byref(pc)))
        assert L.pt_set_feature_walk(ctx.handle, 0) == capi.PT_ERR_STATE and b"frame is open" in L.pt_last_error()
        capi.check(L.pt_step(ctx.handle, 4, None))
        capi.check(L.pt_feature_walk_stats(ctx.handle, out))  # readable in the open frame
        assert out[0] == _waves(W, H) * 2 and out[1] == 0
        capi.check(L.pt_end(ctx.handle, None))
        # a frame with the walk on and features off runs no walk, and says so; nothing is written
        for i in range(4):
            out[i] = 7
        hip.render(sc, hip.RenderConfig(W, H, 4, DEPTH, 1), img, ctx=ctx, feature_walk=True)
        assert np.array_equal(img, o["rgba"])
        assert L.pt_feature_walk_stats(ctx.handle, out) == capi.PT_ERR_STATE and b"did not run the walk" in L.pt_last_error()
        assert list(out) == [7, 7, 7, 7]
        # GL shading is refused with the walk on: for the hierarchy scene by the shading's own rule, for a small one by the features'
        with pytest.raises(capi.PtError, match="GL shading"):
            hip.render(sc, hip.RenderConfig(W, H, 1, DEPTH, 1), img, ctx=ctx, shading="gl", features=2, feature_walk=True)
        small = _shipped("gpu_showcase")[0]
        with pytest.raises(capi.PtError, match="features: not available with GL shading"):
            hip.render(small, hip.RenderConfig(W, H, 1, DEPTH, 1), img, ctx=ctx, shading="gl", features=2, feature_walk=True)
        assert L.pt_feature_walk_stats(ctx.handle, out) == capi.PT_ERR_STATE
        hip.set_shading(ctx, "cpu")
        # ... and the context is usable: the oracle's frame, the oracle's planes
        hip.set_moments(ctx, False)
        hip.set_features(ctx, 0)
        render_vs_oracle(ctx, sc, o, W, H, 4, DEPTH, 1, tag="at the end", forms=("shipping",))
        f = _frame(ctx, sc, W, H, 4, DEPTH, 2)
        assert _same_feats(f["feats"], at.ref_features(osc, W, H, 4, DEPTH, 1, 2)) and np.array_equal(f["img"], o["rgba"])
        # turned off again, the refusal is back
        hip.set_feature_walk(ctx, False)
        hip.set_moments(ctx, True)
        hip.set_features(ctx, 2)
        assert L.pt_begin(ctx.handle, C.byref(flat.c), C.byref(pc)) == capi.PT_ERR_INVALID and L.pt_last_error().decode() == PARENT_REFUSAL
