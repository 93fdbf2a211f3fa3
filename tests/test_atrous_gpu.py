"""First-hit feature planes and the a-trous filter on the MI355X (pt_set_features, feature_kernel, pt_atrous and its kernels;
DESIGN 3.11).  The features' reference is the oracle (ora_primary_ray, ora_hit, ora_convert_material through
tests/atrous_reference.c); the filter's reference is the same file's restatement of the model, fed the context's own accum, m2,
counts and features.  Frames are small (40 x 24: two tiles, ragged; 37 x 21; 70 x 45 for the gather).  Every comparison runs
with contexts of its own."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import adaptive_support as ad
import atrous_support as at
import moments_support as ms
from conftest import ROOT, render_vs_oracle, scene_path
from moments_support import H, W

pytestmark = pytest.mark.gpu

SPP = 16
FEATURE_SCENES = [("example_simple", 4), ("gpu_showcase", 8), ("metal_glass_room", 6)]  # glass, emitters; the last two have a thin lens


@pytest.fixture(autouse=True, scope="module")
def _built(gpu_ctx):
    return gpu_ctx


def _scene(name):
    from path_trace_golang_amd import scene

    return scene.load(scene_path(name))


def _frame(ctx, sc, w, h, spp, depth, k, seed=1, chunk=0, **kw):
    """One frame with moments on and k feature samples: dict(img, accum, m2, feats (normal, albedo, depth) or None, st)."""
    from path_trace_golang_amd import hip

    img = np.zeros((h, w, 4), np.uint8)
    acc = np.zeros((h, w, 3))
    m2 = np.zeros((h, w, 3))
    st = hip.render(sc, hip.RenderConfig(w, h, spp, depth, seed, chunk), img, None, acc, ctx=ctx, moments=m2, features=k, **kw)
    feats = None
    if k > 0:
        feats = tuple(np.full((h, w, 3), -7.0) for _ in range(3))
        hip.read_features(ctx, *feats)
    return dict(img=img, accum=acc, m2=m2, feats=feats, st=st)


def _same_feats(a, b):
    return all(at.same_bits(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------- 1. features against the oracle
@pytest.mark.parametrize("name,depth", FEATURE_SCENES)
def test_features_match_the_oracle(name, depth):
    from path_trace_golang_amd import capi

    sc = _scene(name)
    if name != "example_simple":
        assert sc.camera.aperture > 0  # a thin lens: the rays come from the lens-pool ray generation
    with capi.Context(ndev=1) as ctx:
        for k in (4, 16, 40):
            got = _frame(ctx, sc, W, H, SPP, depth, k)["feats"]
            want = at.ref_features(name, W, H, SPP, depth, 1, k)
            for plane, g, w_ in zip(("normal", "albedo", "depth"), got, want):
                diff = int(np.count_nonzero(np.ascontiguousarray(g).view(np.uint64) != np.ascontiguousarray(w_).view(np.uint64)))
                assert diff == 0, (name, k, plane, diff)
            assert np.all(got[2][..., 2] == min(k, SPP))            # feature samples taken
            assert np.all(got[2][..., 1] <= got[2][..., 2]) and got[2][..., 1].max() > 0
            n = np.linalg.norm(got[0], axis=2)
            assert np.all(n <= got[2][..., 1] + 1e-9)              # a sum of h unit normals


# ---------------------------------------------------------------- 2. invariance, bit for bit
INV = ("metal_glass_room", 6, 6)  # scene, depth, k: chunks of 3 and 5 cut the six feature samples at different places


@pytest.fixture(scope="module")
def inv_ref(_built):
    from path_trace_golang_amd import capi

    name, depth, k = INV
    with capi.Context(ndev=1) as ctx:
        f = _frame(ctx, _scene(name), W, H, SPP, depth, k)
    assert _same_feats(f["feats"], at.ref_features(name, W, H, SPP, depth, 1, k))
    return f


@pytest.mark.parametrize("chunk", [3, 5])
def test_features_do_not_depend_on_the_chunk(inv_ref, chunk):
    from path_trace_golang_amd import capi

    name, depth, k = INV
    with capi.Context(ndev=1) as ctx:
        f = _frame(ctx, _scene(name), W, H, SPP, depth, k, chunk=chunk)
    assert f["st"]["spp_chunk"] == chunk and _same_feats(f["feats"], inv_ref["feats"])
    assert np.array_equal(f["img"], inv_ref["img"]) and at.same_bits(f["m2"], inv_ref["m2"])


@pytest.mark.parametrize("step", [1, 7])
def test_features_do_not_depend_on_the_steps(inv_ref, step):
    from path_trace_golang_amd import capi, hip

    name, depth, k = INV
    L = capi.load()
    flat = hip.FlatScene(_scene(name))
    pc = hip.pt_config(hip.RenderConfig(W, H, SPP, depth, 1))
    feats = tuple(np.zeros((H, W, 3)) for _ in range(3))
    with capi.Context(ndev=1) as ctx:
        hip.set_moments(ctx, True)
        hip.set_features(ctx, k)
        capi.check(L.pt_begin(ctx.handle, C.byref(flat.c), C.byref(pc)))
        assert L.pt_set_features(ctx.handle, 2) == capi.PT_ERR_STATE  # refused while a frame is open
        done = C.c_int32(0)
        while done.value < SPP:
            capi.check(L.pt_step(ctx.handle, step, C.byref(done)))
            if done.value == step:  # between steps the planes hold the samples done so far
                hip.read_features(ctx, *feats)
                assert _same_feats(feats, at.ref_features(name, W, H, min(step, SPP), depth, 1, k))
        capi.check(L.pt_end(ctx.handle, None))
        hip.read_features(ctx, *feats)
    assert _same_feats(feats, inv_ref["feats"])


@pytest.mark.parametrize("env", [{"PTCORE_PIPELINE": "wavefront"}, {"PTCORE_SCAN": "uniform"}], ids=["wavefront", "uniform"])
def test_features_do_not_depend_on_the_trace_form(monkeypatch, inv_ref, env):
    from path_trace_golang_amd import capi

    name, depth, k = INV
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    with capi.Context(ndev=1) as ctx:  # both are read by pt_create
        f = _frame(ctx, _scene(name), W, H, SPP, depth, k)
    assert _same_feats(f["feats"], inv_ref["feats"]) and np.array_equal(f["img"], inv_ref["img"])


def _filter_against_restatement(ctx, f, w, h, n, counts=None, tag="", configs=(dict(), dict(iterations=0), dict(iterations=6, sigma_z=0.0))):
    """pt_atrous on ctx's frame f against the restatement fed f's own planes, for several configurations."""
    out = None
    for cfg in configs:
        got = at.gpu_run(ctx, at.atrous_config(**cfg), w, h)
        want = at.ref_filter(f["accum"], f["m2"], n, counts, f["feats"], **cfg)
        at.assert_same_run(got, want, (tag, cfg))
        assert got["iterations"] == cfg.get("iterations", 5) and got["launches"] == got["iterations"] + 4 and got["atrous_ms"] > 0
        out = out or got
    return out


def test_four_virtual_devices_give_the_planes_and_the_filter_of_one():
    from path_trace_golang_amd import capi

    name, depth, k = "example_simple", 4, 4
    w, h = ad.GATHER_W, ad.GATHER_H  # 70 x 45: 6 tiles = 2, 2, 1, 1
    sc = _scene(name)
    with capi.Context(ndev=1) as one, capi.Context(devices=[0, 0, 0, 0]) as four:
        a = _frame(one, sc, w, h, 8, depth, k)
        b = _frame(four, sc, w, h, 8, depth, k)
        assert b["st"]["num_devices"] == 4
        assert _same_feats(a["feats"], b["feats"]) and at.same_bits(a["accum"], b["accum"]) and at.same_bits(a["m2"], b["m2"])
        ra = at.gpu_run(one, None, w, h)
        rb = _filter_against_restatement(four, b, w, h, 8, tag="four devices")
    at.assert_same_run(ra, rb, "one device vs four")
    assert ra["noise_after"] == rb["noise_after"]  # the filter runs on devices[0] over the gathered planes: the same tree


def test_adaptive_blocks_hold_the_features_of_their_own_count():
    from path_trace_golang_amd import capi, hip

    name, depth, seed, cap, step, min_spp, target = ad.CASE
    k = 40
    sc = _scene(name)
    with capi.Context(ndev=1) as ctx:
        hip.set_features(ctx, k)
        img, acc, m2, counts, _, _, st = ad.render_adaptive(ctx, sc, W, H, cap, depth, seed, target, step, min_spp, features=k)
        assert counts.tolist() == ad.expand(ad.CASE_MAP).tolist()
        feats = tuple(np.zeros((H, W, 3)) for _ in range(3))
        hip.read_features(ctx, *feats)
        assert np.array_equal(feats[2][..., 2], np.minimum(k, counts).astype(np.float64))  # min(k, n) feature samples
        assert _same_feats(feats, at.ref_features(name, W, H, cap, depth, seed, k, counts=counts))
        for n in sorted(set(int(v) for v in np.unique(counts))):  # ... and the planes of the plain n-sample frame
            plain = _frame(ctx, sc, W, H, n, depth, k, seed)["feats"]
            sel = counts == n
            assert all(at.same_bits(a[sel], b[sel]) for a, b in zip(feats, plain)), n


# ---------------------------------------------------------------- 3. the filter against the restatement
@pytest.mark.parametrize("size", [(40, 24), (37, 21)])
@pytest.mark.parametrize("name,depth", FEATURE_SCENES)
def test_filter_matches_the_restatement(name, depth, size):
    from path_trace_golang_amd import capi, hip

    w, h = size
    with capi.Context(ndev=1) as ctx:
        f = _frame(ctx, _scene(name), w, h, SPP, depth, 4)
        got = _filter_against_restatement(ctx, f, w, h, SPP, tag=(name, size))
        nz = hip.noise_estimate(ctx)
    assert abs(got["noise_before"] - nz["noise"]) <= 1e-9 * max(1.0, nz["noise"])
    assert got["noise_after"] < got["noise_before"] and got["bad_pixels"] == 0


def test_filter_matches_the_restatement_on_a_fogged_frame():
    from path_trace_golang_amd import capi

    sc = _scene("gpu_showcase")
    assert sc.fog is not None and sc.fog.gpu_volumetric
    with capi.Context(ndev=1) as ctx:
        plain = _frame(ctx, sc, W, H, SPP, 8, 4)
        f = _frame(ctx, sc, W, H, SPP, 8, 4, fog=True)
        assert not np.array_equal(f["accum"], plain["accum"]) and _same_feats(f["feats"], plain["feats"])  # fog changes L, not the first hit
        _filter_against_restatement(ctx, f, W, H, SPP, tag="fog")


def test_filter_matches_the_restatement_on_an_adaptive_frame():
    from path_trace_golang_amd import capi, hip

    name, depth, seed, cap, step, min_spp, target = ad.CASE
    sc = _scene(name)
    with capi.Context(ndev=1) as ctx:
        img, acc, m2, counts, _, _, st = ad.render_adaptive(ctx, sc, W, H, cap, depth, seed, target, step, min_spp, features=4)
        assert len(np.unique(counts)) >= 3
        feats = tuple(np.zeros((H, W, 3)) for _ in range(3))
        hip.read_features(ctx, *feats)
        f = dict(accum=acc, m2=m2, feats=feats)
        got = _filter_against_restatement(ctx, f, W, H, 0, counts=counts, tag="adaptive")
        nz = hip.noise_estimate(ctx)
    assert abs(got["noise_before"] - nz["noise"]) <= 1e-9 * max(1.0, nz["noise"])


def test_filter_runs_without_features_on_a_hierarchy_scene():
    from path_trace_golang_amd import capi, hip, synth

    sc = synth.make_scene(300)
    L = capi.load()
    flat = hip.FlatScene(sc)
    with capi.Context(ndev=1) as ctx:
        # k > 0 is refused for a scene on the BVH path, and the context stays usable
        hip.set_moments(ctx, True)
        hip.set_features(ctx, 4)
        pc = hip.pt_config(hip.RenderConfig(W, H, 4, 3, 1))
        assert L.pt_begin(ctx.handle, C.byref(flat.c), C.byref(pc)) == capi.PT_ERR_INVALID and b"BVH" in L.pt_last_error()
        f = _frame(ctx, sc, W, H, 4, 3, 0)
        assert L.pt_read_features(ctx.handle, None, None, None) == capi.PT_ERR_STATE
        _filter_against_restatement(ctx, f, W, H, 4, tag="300 objects")
        # hip.render chooses k = 0 by itself there
        img = np.zeros((H, W, 4), np.uint8)
        st = hip.render(sc, hip.RenderConfig(W, H, 4, 3, 1), img, ctx=ctx, atrous=hip.AtrousConfig())
        want = at.ref_filter(f["accum"], f["m2"], 4, None, None)
    assert np.array_equal(img, want["rgba"]) and st["atrous"]["iterations"] == 5


# ---------------------------------------------------------------- 4. consistency
def test_a_preview_between_two_steps_changes_nothing():
    from path_trace_golang_amd import capi, hip

    name, depth = "gpu_showcase", 8
    sc = _scene(name)
    L = capi.load()
    flat = hip.FlatScene(sc)
    pc = hip.pt_config(hip.RenderConfig(W, H, SPP, depth, 1))
    out = {}
    for preview in (False, True):
        with capi.Context(ndev=1) as ctx:
            hip.set_moments(ctx, True)
            hip.set_features(ctx, 4)
            capi.check(L.pt_begin(ctx.handle, C.byref(flat.c), C.byref(pc)))
            done = C.c_int32(0)
            capi.check(L.pt_step(ctx.handle, 1, C.byref(done)))
            if preview:  # one sample per pixel: no variance yet
                assert L.pt_atrous(ctx.handle, None, None, 0, None, None, None) == capi.PT_ERR_STATE and b"2 samples" in L.pt_last_error()
            capi.check(L.pt_step(ctx.handle, 6, C.byref(done)))
            if preview:
                mid = at.gpu_run(ctx, None, W, H)
                acc7, m27 = np.zeros((H, W, 3)), np.zeros((H, W, 3))
                capi.check(L.pt_read(ctx.handle, None, 0, acc7.ctypes.data_as(C.c_void_p)))
                hip.read_moments(ctx, m27)
                feats = tuple(np.zeros((H, W, 3)) for _ in range(3))
                hip.read_features(ctx, *feats)
                at.assert_same_run(mid, at.ref_filter(acc7, m27, 7, None, feats), "preview at 7 samples")
            capi.check(L.pt_step(ctx.handle, SPP, C.byref(done)))
            img, acc, m2 = np.zeros((H, W, 4), np.uint8), np.zeros((H, W, 3)), np.zeros((H, W, 3))
            capi.check(L.pt_read(ctx.handle, img.ctypes.data_as(C.c_void_p), W * 4, acc.ctypes.data_as(C.c_void_p)))
            st = capi.PtStats()
            capi.check(L.pt_end(ctx.handle, C.byref(st)))
            hip.read_moments(ctx, m2)
            out[preview] = (img, acc, m2, st.as_dict(), at.gpu_run(ctx, None, W, H))
    a, b = out[False], out[True]
    assert np.array_equal(a[0], b[0]) and at.same_bits(a[1], b[1]) and at.same_bits(a[2], b[2])
    for key in ("samples", "segments", "exit_scans", "draws", "trace_launches"):
        assert a[3][key] == b[3][key], key
    at.assert_same_run(a[4], b[4], "final filter")


def test_the_same_image_through_render_and_through_the_cli(tmp_path):
    from PIL import Image

    from path_trace_golang_amd import capi, hip

    name, depth = "example_simple", 4
    sc = _scene(name)
    with capi.Context(ndev=1) as ctx:
        f = _frame(ctx, sc, W, H, SPP, depth, 4)
        direct = at.gpu_run(ctx, at.atrous_config(iterations=3), W, H)
        img = np.zeros((H, W, 4), np.uint8)
        st = hip.render(sc, hip.RenderConfig(W, H, SPP, depth, 1), img, ctx=ctx, atrous=hip.AtrousConfig(iterations=3))
        plain = np.zeros((H, W, 4), np.uint8)
        st_plain = hip.render(sc, hip.RenderConfig(W, H, SPP, depth, 1), plain, ctx=ctx)
    assert np.array_equal(img, direct["rgba"]) and st["atrous"]["noise_after"] == direct["noise_after"] and "noise" in st
    assert np.array_equal(plain, f["img"]) and "atrous" not in st_plain and not np.array_equal(plain, img)  # off again without the argument
    out = str(tmp_path / "o.png")
    r = subprocess.run([os.path.join(ROOT, "path_trace_golang_amd", "render"), "-headless", "-gpu", "-scene", scene_path(name), "-out", out,
                        "-width", str(W), "-height", str(H), "-spp", str(SPP), "-depth", str(depth), "-seed", "1", "-atrous",
                        "-atrous-iters", "3"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "a-trous filter: 3 iterations, 4 feature samples per pixel" in r.stderr, r.stderr
    im = Image.open(out)
    assert im.size == (W, H) and np.array_equal(np.array(im.convert("RGB")), direct["rgba"][..., :3])


# ---------------------------------------------------------------- 5. state rules
def test_state_rules_and_every_refusal_leaves_a_usable_context(oracle):
    from path_trace_golang_amd import capi, hip

    L = capi.load()
    name, depth, n, seed = "test_comprehensive", 6, 3, 5
    sc = _scene(name)
    o = oracle.render(ms.ora_scene(name), W, H, n, depth, seed=seed)
    flat = hip.FlatScene(sc)
    st = capi.PtAtrousStats()
    buf = np.zeros((H, W, 3))
    p = buf.ctypes.data_as(C.POINTER(C.c_double))

    def atrous(ctx, cfg=None):
        return L.pt_atrous(ctx.handle, C.byref(cfg) if cfg is not None else None, None, 0, None, None, C.byref(st))

    with capi.Context(ndev=1) as ctx:
        # before any frame, then after a frame with moments off
        for _ in range(2):
            assert atrous(ctx) == capi.PT_ERR_STATE and L.pt_last_error()
            assert L.pt_read_features(ctx.handle, p, None, None) == capi.PT_ERR_STATE and L.pt_last_error()
            render_vs_oracle(ctx, sc, o, W, H, n, depth, seed, tag="after a refusal")
        assert atrous(ctx) == capi.PT_ERR_STATE and b"moments off" in L.pt_last_error()
        # moments on, features off: the filter runs, the planes are refused
        _frame(ctx, sc, W, H, n, depth, 0, seed)
        assert atrous(ctx) == capi.PT_OK and st.iterations == 5
        assert L.pt_read_features(ctx.handle, p, None, None) == capi.PT_ERR_STATE and b"features off" in L.pt_last_error()
        # bad arguments
        assert L.pt_set_features(ctx.handle, -1) == capi.PT_ERR_INVALID
        for bad in (dict(iterations=7), dict(iterations=-1), dict(sigma_l=0.0), dict(sigma_l=float("nan")), dict(sigma_n=-0.1),
                    dict(sigma_z=float("nan")), dict(sigma_a=-1.0)):
            c = dict(at.DEFAULTS, **bad)
            cfg = capi.PtAtrousConfig(c["iterations"], 0, c["sigma_l"], c["sigma_n"], c["sigma_z"], c["sigma_a"])
            assert atrous(ctx, cfg) == capi.PT_ERR_INVALID and L.pt_last_error(), bad
        assert L.pt_atrous(ctx.handle, None, buf.ctypes.data_as(C.c_void_p), W * 4 - 1, None, None, None) == capi.PT_ERR_INVALID
        assert atrous(ctx) == capi.PT_OK
        # one sample: no variance
        _frame(ctx, sc, W, H, 1, depth, 0, seed)
        assert atrous(ctx) == capi.PT_ERR_STATE
        # GL shading: a frame with k > 0 is refused; a GL frame refuses both reads
        hip.set_features(ctx, 4)
        hip.set_moments(ctx, True)
        hip.set_shading(ctx, "gl", sc)
        pc = hip.pt_config(hip.RenderConfig(W, H, n, depth, seed))
        assert L.pt_begin(ctx.handle, C.byref(flat.c), C.byref(pc)) == capi.PT_ERR_INVALID and b"GL shading" in L.pt_last_error()
        hip.set_features(ctx, 0)
        img = np.zeros((H, W, 4), np.uint8)
        capi.check(L.pt_render(ctx.handle, C.byref(flat.c), C.byref(pc), img.ctypes.data_as(C.c_void_p), W * 4, None, None, None, None))
        assert atrous(ctx) == capi.PT_ERR_STATE and b"GL shading" in L.pt_last_error()
        assert L.pt_read_features(ctx.handle, p, None, None) == capi.PT_ERR_STATE
        hip.set_shading(ctx, "cpu")
        # ... and the context still renders the CPU engine's frame, with everything off
        hip.set_moments(ctx, False)
        render_vs_oracle(ctx, sc, o, W, H, n, depth, seed, tag="at the end")


def test_tiles_device_neither_collects_nor_fails():
    import torch

    from path_trace_golang_amd import capi, hip

    sc = _scene("example_simple")
    flat = hip.FlatScene(sc)
    L = capi.load()
    pc = hip.pt_config(hip.RenderConfig(W, H, 4, 4, 1))
    with capi.Context(ndev=1) as ctx:
        hip.set_moments(ctx, True)
        hip.set_features(ctx, 4)
        tiles = torch.zeros(2 * 4096, dtype=torch.uint8, device=torch.device("cuda", 0))
        st = capi.PtStats()
        capi.check(L.pt_render_tiles_device(ctx.handle, C.byref(flat.c), C.byref(pc), None, C.c_void_p(tiles.data_ptr()), None, None, C.byref(st)))
        assert st.samples == W * H * 4 and int(tiles.sum().item()) > 0
        assert L.pt_read_features(ctx.handle, None, None, None) == capi.PT_ERR_STATE
        assert L.pt_atrous(ctx.handle, None, None, 0, None, None, None) == capi.PT_ERR_STATE
