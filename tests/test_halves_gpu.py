"""Half-buffer sums and the pair filter on the MI355X (pt_set_halves, halves_kernel, pt_atrous_halves and its kernels; DESIGN
3.12).  The sums' reference is the oracle's per-sample radiances; the pair filter's reference is tests/atrous_reference.c's
restatement of the filter run on each half, fed the context's own planes, and the combine restated in halves_support.  Frames
are small (40 x 24: two tiles, ragged; 37 x 21; 70 x 45 for the gather).  Every comparison runs with contexts of its own."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import adaptive_support as ad
import atrous_support as at
import halves_support as hv
import moments_support as ms
from conftest import ROOT, render_vs_oracle, scene_path
from moments_support import H, W

pytestmark = pytest.mark.gpu

SPP = 16
SCENES = [("example_simple", 4), ("metal_glass_room", 6), ("gpu_showcase", 8)]  # the last two have a thin lens
PLANES = ("SA", "QA", "SB", "QB")


@pytest.fixture(autouse=True, scope="module")
def _built(gpu_ctx):
    return gpu_ctx


def _scene(name):
    from path_trace_golang_amd import scene

    return scene.load(scene_path(name))


def _frame(ctx, sc, w, h, spp, depth, k=0, seed=1, chunk=0, **kw):
    """One frame with halves on and k feature samples: dict(img, accum, m2, halves (SA, QA, SB, QB), feats or None, st)."""
    from path_trace_golang_amd import hip

    img = np.zeros((h, w, 4), np.uint8)
    acc = np.zeros((h, w, 3))
    m2 = np.zeros((h, w, 3))
    st = hip.render(sc, hip.RenderConfig(w, h, spp, depth, seed, chunk), img, None, acc, ctx=ctx, moments=m2, features=k, halves=True, **kw)
    feats = None
    if k > 0:
        feats = tuple(np.full((h, w, 3), -7.0) for _ in range(3))
        hip.read_features(ctx, *feats)
    return dict(img=img, accum=acc, m2=m2, halves=hv.read_halves(ctx, w, h), feats=feats, st=st)


def _same_halves(a, b, sel=None):
    return all(at.same_bits(x if sel is None else x[sel], y if sel is None else y[sel]) for x, y in zip(a, b))


# ---------------------------------------------------------------- 1. the sums against the oracle
@pytest.mark.parametrize("name,depth", SCENES)
def test_half_sums_match_the_oracle(name, depth):
    from path_trace_golang_amd import capi

    n = 24
    sc = _scene(name)
    if name != "example_simple":
        assert sc.camera.aperture > 0
    want = hv.half_sums(ms.samples(name, depth, 1, n))
    with capi.Context(ndev=1) as ctx:
        f = _frame(ctx, sc, W, H, n, depth, chunk=5)
        one = _frame(ctx, sc, W, H, 1, depth)
        two = _frame(ctx, sc, W, H, 2, depth)
    assert f["st"]["spp_chunk"] == 5
    for plane, got, ref in zip(PLANES, f["halves"], want):
        bound = (4 * depth if plane[0] == "S" else 8 * depth + n // 2) * 2.0 ** -52
        rel = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)
        print("%s %s: max rel err %.3g (bound %.3g)" % (name, plane, rel.max(), bound))
        assert np.all(rel <= bound), (name, plane, float(rel.max()))
    # the halves add up to the frame's own sums (one rounding per add)
    assert np.allclose(f["halves"][0] + f["halves"][2], f["accum"], rtol=2 * n * 2.0 ** -53, atol=0)  # n - 1, n / 2 - 1 and one more add
    # a 1-sample frame: the sample is half A's; a 2-sample frame: the second one is half B's
    SA, QA, SB, QB = one["halves"]
    assert at.same_bits(SA, one["accum"]) and at.same_bits(QA, one["accum"] * one["accum"]) and at.same_bits(QA, one["m2"])
    assert not SB.any() and not QB.any()
    SA, QA, SB, QB = two["halves"]
    assert at.same_bits(SA, one["accum"]) and at.same_bits(QB, SB * SB) and SB.any()


# ---------------------------------------------------------------- 2. invariance, bit for bit, against one reference run
INV = ("metal_glass_room", 6)


@pytest.fixture(scope="module")
def inv_ref(_built):
    from path_trace_golang_amd import capi

    name, depth = INV
    with capi.Context(ndev=1) as ctx:
        f = _frame(ctx, _scene(name), W, H, SPP, depth)
    assert all(p.any() for p in f["halves"])
    return f


@pytest.mark.parametrize("chunk", [3, 5])
def test_half_sums_do_not_depend_on_the_chunk(inv_ref, chunk):
    from path_trace_golang_amd import capi

    name, depth = INV
    with capi.Context(ndev=1) as ctx:
        f = _frame(ctx, _scene(name), W, H, SPP, depth, chunk=chunk)  # a chunk starts on an odd sample
    assert f["st"]["spp_chunk"] == chunk and _same_halves(f["halves"], inv_ref["halves"])
    assert np.array_equal(f["img"], inv_ref["img"]) and at.same_bits(f["m2"], inv_ref["m2"])


@pytest.mark.parametrize("step", [1, 7])
def test_half_sums_do_not_depend_on_the_steps(inv_ref, step):
    from path_trace_golang_amd import capi, hip

    name, depth = INV
    L = capi.load()
    sc = _scene(name)
    flat = hip.FlatScene(sc)
    pc = hip.pt_config(hip.RenderConfig(W, H, SPP, depth, 1))
    with capi.Context(ndev=1) as ctx:
        mid = _frame(ctx, sc, W, H, 2 * step, depth)["halves"]
        hip.set_halves(ctx, True)
        capi.check(L.pt_begin(ctx.handle, C.byref(flat.c), C.byref(pc)))
        assert L.pt_set_halves(ctx.handle, 0) == capi.PT_ERR_STATE  # refused while a frame is open
        done = C.c_int32(0)
        while done.value < SPP:
            capi.check(L.pt_step(ctx.handle, step, C.byref(done)))
            if done.value == 2 * step:  # between steps the planes hold the samples done so far
                assert _same_halves(hv.read_halves(ctx, W, H), mid)
        capi.check(L.pt_end(ctx.handle, None))
        assert _same_halves(hv.read_halves(ctx, W, H), inv_ref["halves"])


@pytest.mark.parametrize("env", [{"PTCORE_PIPELINE": "wavefront"}, {"PTCORE_SCAN": "uniform"}], ids=["wavefront", "uniform"])
def test_half_sums_do_not_depend_on_the_trace_form(monkeypatch, inv_ref, env):
    from path_trace_golang_amd import capi

    name, depth = INV
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    with capi.Context(ndev=1) as ctx:  # both are read by pt_create
        f = _frame(ctx, _scene(name), W, H, SPP, depth)
    assert _same_halves(f["halves"], inv_ref["halves"]) and np.array_equal(f["img"], inv_ref["img"])


def test_four_virtual_devices_give_the_sums_and_the_pair_filter_of_one():
    from path_trace_golang_amd import capi

    name, depth, k = "example_simple", 4, 4
    w, h = ad.GATHER_W, ad.GATHER_H  # 70 x 45: 6 tiles = 2, 2, 1, 1
    sc = _scene(name)
    with capi.Context(ndev=1) as one, capi.Context(devices=[0, 0, 0, 0]) as four:
        a = _frame(one, sc, w, h, 8, depth, k)
        b = _frame(four, sc, w, h, 8, depth, k)
        assert b["st"]["num_devices"] == 4 and _same_halves(a["halves"], b["halves"])
        ra = hv.gpu_pair(one, None, w, h)
        rb = hv.gpu_pair(four, None, w, h)
    hv.assert_same_pair(ra, rb, "one device vs four")
    assert ra["noise"] == rb["noise"] and ra["noise_model"] == rb["noise_model"]  # devices[0], the gathered planes: the same tree


def test_fog_changes_all_four_sums():
    from path_trace_golang_amd import capi

    sc = _scene("gpu_showcase")
    assert sc.fog is not None and sc.fog.gpu_volumetric
    with capi.Context(ndev=1) as ctx:
        plain = _frame(ctx, sc, W, H, SPP, 8, 4)
        f = _frame(ctx, sc, W, H, SPP, 8, 4, fog=True)
        for a, b in zip(f["halves"], plain["halves"]):
            assert not np.array_equal(a, b)
        S, Q = f["halves"][0] + f["halves"][2], f["halves"][1] + f["halves"][3]  # the record the frame's sum adds: after the fog term
        assert np.allclose(S, f["accum"], rtol=2 * SPP * 2.0 ** -53, atol=0) and np.allclose(Q, f["m2"], rtol=2 * SPP * 2.0 ** -53, atol=0)
        _pair_against_restatement(ctx, f, W, H, SPP, tag="fog", configs=(dict(),))


# ---------------------------------------------------------------- 3. the pair filter against the restatement
CONFIGS = (dict(), dict(iterations=0), dict(iterations=6, sigma_z=0.0))


def _pair_against_restatement(ctx, f, w, h, n, counts=None, tag="", configs=CONFIGS):
    """pt_atrous_halves on ctx's frame f against the restatement fed f's own planes, for several configurations."""
    out = None
    for cfg in configs:
        got = hv.gpu_pair(ctx, at.atrous_config(**cfg), w, h)
        want = hv.ref_pair(*f["halves"], n, counts, f["feats"], **cfg)
        hv.assert_same_pair(got, want, (tag, cfg))
        T = cfg.get("iterations", 5)
        assert got["iterations"] == T and got["launches"] == T + 2 and got["atrous_ms"] > 0
        assert got["spp_min"] == (n if counts is None else int(counts.min()))
        out = out or got
    return out


@pytest.mark.parametrize("size", [(40, 24), (37, 21)])
@pytest.mark.parametrize("name,depth", SCENES)
def test_pair_filter_matches_the_restatement(name, depth, size):
    from path_trace_golang_amd import capi

    w, h = size
    sc = _scene(name)
    with capi.Context(ndev=1) as ctx:
        f = _frame(ctx, sc, w, h, SPP, depth, 4)
        got = _pair_against_restatement(ctx, f, w, h, SPP, tag=(name, size))
        full = at.gpu_run(ctx, None, w, h)  # pt_atrous on the same frame is untouched by the pair run
        at.assert_same_run(full, at.ref_filter(f["accum"], f["m2"], SPP, None, f["feats"]), (name, size, "pt_atrous beside it"))
        f0 = _frame(ctx, sc, w, h, SPP, depth, 0)  # features off: the three feature terms are off whatever the sigmas
        assert f0["feats"] is None and _same_halves(f0["halves"], f["halves"])
        _pair_against_restatement(ctx, f0, w, h, SPP, tag=(name, size, "k = 0"), configs=(dict(),))
    assert got["bad_pixels"] == 0 and 0 < got["noise_model"] and 0 < got["noise"]
    print("%s %s: noise %.4f measured, %.4f propagated; pt_atrous noise_after %.4f" % (name, size, got["noise"], got["noise_model"], full["noise_after"]))


# ---------------------------------------------------------------- 4. adaptive frames
ADAPT = ("example_simple", 4, 1, 35, 7, 7, 0.3)  # scene, depth, seed, cap, step, min_spp, target: blocks stop at 7, 14, 21, ...


def test_adaptive_blocks_hold_the_half_sums_of_their_own_count():
    from path_trace_golang_amd import capi, hip

    name, depth, seed, cap, step, min_spp, target = ADAPT
    sc = _scene(name)
    plan, _ = ad.plan_restated(ms.samples(name, depth, seed, cap), target, step, min_spp, cap)
    want = ad.expand(plan)
    distinct = sorted(set(int(v) for v in np.unique(want)))
    assert len(distinct) >= 3 and any(n & 1 for n in distinct) and min(distinct) >= 4, distinct  # odd counts: nA != nB
    with capi.Context(ndev=1) as ctx:
        img, acc, m2, counts, _, _, st = ad.render_adaptive(ctx, sc, W, H, cap, depth, seed, target, step, min_spp, features=4, halves=True)
        assert counts.tolist() == want.tolist()
        halves = hv.read_halves(ctx, W, H)
        feats = tuple(np.zeros((H, W, 3)) for _ in range(3))
        hip.read_features(ctx, *feats)
        got = _pair_against_restatement(ctx, dict(halves=halves, feats=feats), W, H, 0, counts=counts, tag="adaptive")
        assert got["spp_min"] == min(distinct)
        for n in distinct:  # every block's four sums are those of the plain frame of its own count
            plain = _frame(ctx, sc, W, H, n, depth, 0, seed)["halves"]
            assert _same_halves(halves, plain, counts == n), n


def test_a_block_stopped_below_four_samples_refuses_the_pair_filter():
    from path_trace_golang_amd import capi, hip

    name, depth, seed = "example_simple", 4, 1
    sc = _scene(name)
    L = capi.load()
    with capi.Context(ndev=1) as ctx:
        img, acc, m2, counts, _, _, st = ad.render_adaptive(ctx, sc, W, H, 12, depth, seed, 1e9, 3, 0, halves=True)  # every block stops at 3
        assert counts.min() == 3
        assert L.pt_atrous_halves(ctx.handle, None, None, None, None, None) == capi.PT_ERR_STATE
        assert b"at least 4 samples" in L.pt_last_error() and b"count is 3" in L.pt_last_error()
        hv.read_halves(ctx, W, H)  # the sums themselves are readable
        hip.set_adaptive(ctx, None)
        f = _frame(ctx, sc, W, H, SPP, depth, 4)
        _pair_against_restatement(ctx, f, W, H, SPP, tag="after the refusal", configs=(dict(),))


# ---------------------------------------------------------------- 5. the stop rule
def _stop_render(ctx, sc, **kw):
    from path_trace_golang_amd import hip

    img = np.zeros((H, W, 4), np.uint8)
    st = hip.render(sc, hip.RenderConfig(W, H, hv.STOP_CAP, hv.STOP_DEPTH, hv.STOP_SEED), img, ctx=ctx, atrous=hip.AtrousConfig(), **kw)
    return img, st


def test_render_stops_at_the_count_the_restatement_predicts(tmp_path, oracle):
    from PIL import Image

    from path_trace_golang_amd import capi, hip

    case = hv.stop_case()
    sc = _scene(hv.STOP_SCENE)
    with capi.Context(ndev=1) as ctx:
        img, st = _stop_render(ctx, sc, filtered_noise=case["target"], noise_step=hv.STOP_STEP)
        assert st["spp_done"] == case["count"], (st["spp_done"], case)
        k = case["count"] // hv.STOP_STEP - 1
        assert abs(st["filtered_noise"] - case["figures"][k]) <= 1e-9 and st["filtered_noise"] <= case["target"] and st["noise_model"] > 0
        plain = np.zeros((H, W, 4), np.uint8)
        sp = hip.render(sc, hip.RenderConfig(W, H, case["count"], hv.STOP_DEPTH, hv.STOP_SEED), plain, ctx=ctx, atrous=hip.AtrousConfig())
        assert np.array_equal(img, plain) and "filtered_noise" not in sp  # the filtered image of a plain frame of that count; off again
        capped, sc_ = _stop_render(ctx, sc, filtered_noise=1e-9, noise_step=hv.STOP_STEP)
        assert sc_["spp_done"] == hv.STOP_CAP and abs(sc_["filtered_noise"] - case["figures"][-1]) <= 1e-9
        assert capi.load().pt_read_halves(ctx.handle, None, None, None, None) == capi.PT_OK
        hip.render(sc, hip.RenderConfig(W, H, 4, hv.STOP_DEPTH, hv.STOP_SEED), plain, ctx=ctx)
        assert capi.load().pt_read_halves(ctx.handle, None, None, None, None) == capi.PT_ERR_STATE  # halves are off without the argument
    out = str(tmp_path / "o.png")
    r = subprocess.run([os.path.join(ROOT, "path_trace_golang_amd", "render"), "-headless", "-gpu", "-scene", scene_path(hv.STOP_SCENE), "-out", out,
                        "-width", str(W), "-height", str(H), "-spp", str(hv.STOP_CAP), "-depth", str(hv.STOP_DEPTH), "-seed", str(hv.STOP_SEED),
                        "-atrous", "-filtered-noise", repr(case["target"]), "-noise-step", str(hv.STOP_STEP)],
                       capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "%d of at most %d spp (filtered noise" % (case["count"], hv.STOP_CAP) in r.stderr, r.stderr
    im = Image.open(out)
    assert im.size == (W, H) and np.array_equal(np.array(im.convert("RGB")), img[..., :3])


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
            hip.set_halves(ctx, True)
            hip.set_features(ctx, 4)
            capi.check(L.pt_begin(ctx.handle, C.byref(flat.c), C.byref(pc)))
            done = C.c_int32(0)
            capi.check(L.pt_step(ctx.handle, 3, C.byref(done)))
            if preview:  # three samples per pixel: half B has no variance yet
                assert L.pt_atrous_halves(ctx.handle, None, None, None, None, None) == capi.PT_ERR_STATE and b"4 samples" in L.pt_last_error()
            capi.check(L.pt_step(ctx.handle, 4, C.byref(done)))
            if preview:
                mid = hv.gpu_pair(ctx, None, W, H)
                feats = tuple(np.zeros((H, W, 3)) for _ in range(3))
                hip.read_features(ctx, *feats)
                hv.assert_same_pair(mid, hv.ref_pair(*hv.read_halves(ctx, W, H), 7, None, feats), "preview at 7 samples")
            capi.check(L.pt_step(ctx.handle, SPP, C.byref(done)))
            img, acc, m2 = np.zeros((H, W, 4), np.uint8), np.zeros((H, W, 3)), np.zeros((H, W, 3))
            capi.check(L.pt_read(ctx.handle, img.ctypes.data_as(C.c_void_p), W * 4, acc.ctypes.data_as(C.c_void_p)))
            st = capi.PtStats()
            capi.check(L.pt_end(ctx.handle, C.byref(st)))
            hip.read_moments(ctx, m2)
            out[preview] = (img, acc, m2, st.as_dict(), hv.read_halves(ctx, W, H), hv.gpu_pair(ctx, None, W, H))
    a, b = out[False], out[True]
    assert np.array_equal(a[0], b[0]) and at.same_bits(a[1], b[1]) and at.same_bits(a[2], b[2]) and _same_halves(a[4], b[4])
    for key in ("samples", "segments", "exit_scans", "draws", "trace_launches", "resolve_launches"):
        assert a[3][key] == b[3][key], key
    hv.assert_same_pair(a[5], b[5], "final pair filter")


# ---------------------------------------------------------------- 6. state rules
def test_state_rules_and_every_refusal_leaves_a_usable_context(oracle):
    from path_trace_golang_amd import capi, hip

    L = capi.load()
    name, depth, n, seed = "test_comprehensive", 6, 5, 5
    sc = _scene(name)
    o = oracle.render(ms.ora_scene(name), W, H, n, depth, seed=seed)
    flat = hip.FlatScene(sc)
    st = capi.PtHalvesStats()
    buf = np.zeros((H, W, 3))
    p = buf.ctypes.data_as(C.POINTER(C.c_double))

    def pair(ctx, cfg=None):
        return L.pt_atrous_halves(ctx.handle, C.byref(cfg) if cfg is not None else None, None, None, None, C.byref(st))

    def plain(ctx, spp, **kw):
        img = np.zeros((H, W, 4), np.uint8)
        return hip.render(sc, hip.RenderConfig(W, H, spp, depth, seed), img, ctx=ctx, **kw)

    with capi.Context(ndev=1) as ctx:
        # before any frame, then after a frame with everything off
        for _ in range(2):
            assert pair(ctx) == capi.PT_ERR_STATE and L.pt_last_error()
            assert L.pt_read_halves(ctx.handle, p, None, None, None) == capi.PT_ERR_STATE and L.pt_last_error()
            render_vs_oracle(ctx, sc, o, W, H, n, depth, seed, tag="after a refusal")
        # moments on, halves off: both are refused by name
        plain(ctx, n, moments=np.zeros((H, W, 3)))
        assert pair(ctx) == capi.PT_ERR_STATE and b"halves off" in L.pt_last_error()
        assert L.pt_read_halves(ctx.handle, p, None, None, None) == capi.PT_ERR_STATE and b"halves off" in L.pt_last_error()
        # halves on: moments are collected whether or not pt_set_moments asked
        hip.set_moments(ctx, False)
        hip.set_halves(ctx, True)
        img = np.zeros((H, W, 4), np.uint8)
        pc = hip.pt_config(hip.RenderConfig(W, H, n, depth, seed))
        capi.check(L.pt_render(ctx.handle, C.byref(flat.c), C.byref(pc), img.ctypes.data_as(C.c_void_p), W * 4, None, None, None, None))
        assert L.pt_read_moments(ctx.handle, p) == capi.PT_OK and L.pt_read_halves(ctx.handle, p, None, None, p) == capi.PT_OK
        assert pair(ctx) == capi.PT_OK and st.iterations == 5 and st.spp_min == n
        # bad arguments
        for bad in (dict(iterations=7), dict(iterations=-1), dict(sigma_l=0.0), dict(sigma_l=float("nan")), dict(sigma_n=-0.1),
                    dict(sigma_z=float("nan")), dict(sigma_a=-1.0)):
            c = dict(at.DEFAULTS, **bad)
            cfg = capi.PtAtrousConfig(c["iterations"], 0, c["sigma_l"], c["sigma_n"], c["sigma_z"], c["sigma_a"])
            assert pair(ctx, cfg) == capi.PT_ERR_INVALID and L.pt_last_error(), bad
        assert pair(ctx) == capi.PT_OK
        # three samples: half B has one, no variance
        pc3 = hip.pt_config(hip.RenderConfig(W, H, 3, depth, seed))
        capi.check(L.pt_render(ctx.handle, C.byref(flat.c), C.byref(pc3), img.ctypes.data_as(C.c_void_p), W * 4, None, None, None, None))
        assert pair(ctx) == capi.PT_ERR_STATE and b"count is 3" in L.pt_last_error()
        # GL shading: the sums are collected, the pair filter is refused
        hip.set_shading(ctx, "gl", sc)
        capi.check(L.pt_render(ctx.handle, C.byref(flat.c), C.byref(pc), img.ctypes.data_as(C.c_void_p), W * 4, None, None, None, None))
        assert pair(ctx) == capi.PT_ERR_STATE and b"GL shading" in L.pt_last_error()
        assert L.pt_read_halves(ctx.handle, p, None, None, None) == capi.PT_OK
        hip.set_shading(ctx, "cpu")
        # ... and the context still renders the CPU engine's frame, with everything off
        hip.set_halves(ctx, False)
        render_vs_oracle(ctx, sc, o, W, H, n, depth, seed, tag="at the end")
        assert L.pt_read_halves(ctx.handle, p, None, None, None) == capi.PT_ERR_STATE


def test_tiles_device_neither_collects_nor_fails():
    import torch

    from path_trace_golang_amd import capi, hip

    sc = _scene("example_simple")
    flat = hip.FlatScene(sc)
    L = capi.load()
    pc = hip.pt_config(hip.RenderConfig(W, H, 4, 4, 1))
    with capi.Context(ndev=1) as ctx:
        hip.set_halves(ctx, True)
        tiles = torch.zeros(2 * 4096, dtype=torch.uint8, device=torch.device("cuda", 0))
        st = capi.PtStats()
        capi.check(L.pt_render_tiles_device(ctx.handle, C.byref(flat.c), C.byref(pc), None, C.c_void_p(tiles.data_ptr()), None, None, C.byref(st)))
        assert st.samples == W * H * 4 and int(tiles.sum().item()) > 0
        assert L.pt_read_halves(ctx.handle, None, None, None, None) == capi.PT_ERR_STATE
        assert L.pt_atrous_halves(ctx.handle, None, None, None, None, None) == capi.PT_ERR_STATE
