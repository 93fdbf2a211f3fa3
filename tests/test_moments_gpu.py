"""Second moments, the frame noise figure and the render-until-noise-target mode on the MI355X (pt_set_moments,
moments_kernel, noise_kernel).  The reference is the oracle's per-sample radiances (moments_support.samples):
their squares summed in sample order are Q, and the metric of include/ptcore.h computed from S and Q is the noise.  The
frame is 40 x 24: two tiles, the second 8 pixels wide, both cut in height, so every block row has out-of-frame slots.
Every test that switches moments on uses a context of its own."""
from __future__ import annotations

import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import moments_support as ms
from conftest import ROOT, SCENE_NAMES, render_vs_oracle, scene_path
from moments_support import H, W

pytestmark = pytest.mark.gpu

DEPTHS = {"example_simple": 4, "test_scene": 5, "metal_glass_room": 6, "gpu_showcase": 8, "test_comprehensive": 6}


@pytest.fixture(autouse=True, scope="module")
def _built(gpu_ctx):
    return gpu_ctx


def _scene(name):
    from path_trace_golang_amd import scene

    return scene.load(scene_path(name))


def _render(ctx, sc, spp, depth, seed=1, chunk=0, flags=0, want_moments=True, **kw):
    from path_trace_golang_amd import hip

    img = np.zeros((H, W, 4), np.uint8)
    acc = np.zeros((H, W, 3))
    m2 = np.full((H, W, 3), -1.0) if want_moments else None
    st = hip.render(sc, hip.RenderConfig(W, H, spp, depth, seed, chunk, flags), img, None, acc, ctx=ctx, moments=m2, **kw)
    return img, acc, m2, st


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---------------------------------------------------------------- 1. moments against the oracle
@pytest.mark.parametrize("name,depth", [("example_simple", 4), ("metal_glass_room", 6), ("gpu_showcase", 8)])
def test_moments_match_the_oracle(oracle, name, depth):
    from path_trace_golang_amd import capi, hip

    n, seed = 24, 1
    S, Q = ms.sums(ms.samples(name, depth, seed, n))
    o = oracle.render(ms.ora_scene(name), W, H, n, depth, seed=seed)
    assert np.array_equal(_bits(S), _bits(o["accum"]))  # the sample list is the oracle's frame
    sc = _scene(name)
    bound = (8 * depth + n) * 2.0 ** -52
    got = {}
    with capi.Context(ndev=1) as ctx:
        for flags in (capi.PT_FLAG_PIXEL_STATS, 0):
            img, acc, m2, st = _render(ctx, sc, n, depth, seed, chunk=5, flags=flags)  # 5 does not divide 24
            rel = np.abs(m2 - Q) / np.maximum(np.abs(Q), 1e-300)
            print("%s flags %d: m2 max rel err %.3g (bound %.3g), bit-equal %s" % (name, flags, rel.max(), bound,
                                                                                 np.array_equal(_bits(m2), _bits(Q))))
            assert np.all(rel <= bound), (name, flags, float(rel.max()))
            assert st["spp_done"] == n and st["spp_chunk"] == 5
            got[flags] = m2
        assert np.array_equal(_bits(got[0]), _bits(got[capi.PT_FLAG_PIXEL_STATS]))
        # rgba, accum and the totals of a frame with moments on still meet the project's bar ...
        hip.set_moments(ctx, True)
        out = {}
        for form, flags in (("stats", capi.PT_FLAG_PIXEL_STATS), ("shipping", 0)):
            img = np.zeros((H, W, 4), np.uint8)
            acc = np.zeros((H, W, 3))
            nseg = np.zeros((H, W), np.uint32) if flags else None
            ndraw = np.zeros((H, W), np.uint32) if flags else None
            m2 = np.zeros((H, W, 3))
            st = hip.render(sc, hip.RenderConfig(W, H, n, depth, seed, 5, flags), img, None, acc, nseg, ndraw, ctx=ctx, moments=m2)
            for k in ("samples", "segments", "exit_scans", "draws"):
                assert st[k] == o["stats"][k], (name, form, k)
            if flags:
                assert np.array_equal(nseg, o["nseg"]) and np.array_equal(ndraw, o["ndraw"])
            assert np.array_equal(img, o["rgba"])
            assert np.all(np.abs(acc - o["accum"]) <= 4 * depth * 2.0 ** -52 * np.maximum(np.abs(o["accum"]), 1e-300))
            out[form] = acc
        assert np.array_equal(_bits(out["stats"]), _bits(out["shipping"]))
        # ... and so does the frame after it with moments off (conftest.render_vs_oracle switches them off: no argument)
        render_vs_oracle(ctx, sc, o, W, H, n, depth, seed, chunk=5, tag=name)


# ---------------------------------------------------------------- 2. one sample is exact
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_one_sample_is_the_square_of_accum(name):
    from path_trace_golang_amd import capi

    with capi.Context(ndev=1) as ctx:
        img, acc, m2, st = _render(ctx, _scene(name), 1, DEPTHS[name])
    assert np.array_equal(_bits(m2), _bits(np.multiply(acc, acc)))
    assert np.any(m2 > 0)


def test_one_sample_with_the_fog_block_is_the_square_of_the_fogged_accum():
    from path_trace_golang_amd import capi, hip

    sc = _scene("gpu_showcase")
    assert sc.fog is not None and sc.fog.gpu_volumetric
    with capi.Context(ndev=1) as ctx:
        _, plain, _, _ = _render(ctx, sc, 1, 8)
        _, acc, m2, _ = _render(ctx, sc, 1, 8, fog=True)
        fst = hip.fog_last_stats(ctx)
    assert fst["fog_launches"] >= 1 and fst["shadow_rays"] > 0 and not np.array_equal(acc, plain)
    assert np.array_equal(_bits(m2), _bits(np.multiply(acc, acc)))  # the squares are taken after fog_kernel's add


# ---------------------------------------------------------------- 3. GL mode is exact
def test_gl_mode_moments_are_those_of_the_pass_sums():
    import glshade_support as gs
    from path_trace_golang_amd import capi, hip

    depth, seed, passes = 3, 1, 3
    sc = _scene("gpu_showcase")
    jobs = np.array([(x, y, p) for y in range(H) for x in range(W) for p in range(passes)], np.int32)
    l, _ = gs.host_passes(hip.FlatScene(sc), gs.extras(sc), W, H, depth, seed, jobs)
    l = l.reshape(H, W, passes, 3)
    want = (l[:, :, 0] * l[:, :, 0] + l[:, :, 1] * l[:, :, 1]) + l[:, :, 2] * l[:, :, 2]
    with capi.Context(ndev=1) as ctx:
        img, acc, m2, st = _render(ctx, sc, passes, depth, seed, chunk=2, shading="gl")
    assert st["spp_chunk"] == 2
    assert np.array_equal(_bits(acc), _bits((l[:, :, 0] + l[:, :, 1]) + l[:, :, 2]))
    assert np.array_equal(_bits(m2), _bits(want))


# ---------------------------------------------------------------- 4. invariance, bit for bit
INV = ("metal_glass_room", 6, 24)  # glass: split rounds, nested tail, exit scans


@pytest.fixture(scope="module")
def inv_ref(_built):
    from path_trace_golang_amd import capi, hip

    name, depth, n = INV
    with capi.Context(ndev=1) as ctx:
        img, acc, m2, st = _render(ctx, _scene(name), n, depth)
        nz = hip.noise_estimate(ctx)
    for a in (img, acc, m2):
        a.setflags(write=False)
    return img, acc, m2, nz


@pytest.mark.parametrize("chunk", [0, 1, 5])
def test_moments_do_not_depend_on_the_chunk(inv_ref, chunk):
    from path_trace_golang_amd import capi

    name, depth, n = INV
    with capi.Context(ndev=1) as ctx:
        img, acc, m2, st = _render(ctx, _scene(name), n, depth, chunk=chunk)
    assert chunk == 0 or st["spp_chunk"] == chunk
    assert np.array_equal(img, inv_ref[0]) and np.array_equal(_bits(acc), _bits(inv_ref[1]))
    assert np.array_equal(_bits(m2), _bits(inv_ref[2]))


def test_moments_do_not_depend_on_the_steps(inv_ref):
    from path_trace_golang_amd import capi, hip

    name, depth, n = INV
    L = capi.load()
    sc = _scene(name)
    flat = hip.FlatScene(sc)
    pc = hip.pt_config(hip.RenderConfig(W, H, n, depth, 1))
    with capi.Context(ndev=1) as ctx:
        hip.set_moments(ctx, True)
        capi.check(L.pt_begin(ctx.handle, C.byref(flat.c), C.byref(pc)))
        m2 = np.zeros((H, W, 3))
        assert L.pt_read_moments(ctx.handle, m2.ctypes.data_as(C.POINTER(C.c_double))) == capi.PT_ERR_STATE  # no step yet
        done, step = C.c_int32(0), 1
        while done.value < n:  # steps of 1, 2, 3, ... samples
            capi.check(L.pt_step(ctx.handle, step, C.byref(done)))
            step += 1
        hip.read_moments(ctx, m2)  # between pt_begin and pt_end
        inside = hip.noise_estimate(ctx)
        capi.check(L.pt_end(ctx.handle, None))
        after = np.zeros((H, W, 3))
        hip.read_moments(ctx, after)  # and after pt_end, until the next frame opens
        assert hip.noise_estimate(ctx) == inside
    assert done.value == n and step > 6
    assert np.array_equal(_bits(m2), _bits(inv_ref[2])) and np.array_equal(_bits(after), _bits(inv_ref[2]))
    assert inside == inv_ref[3]


@pytest.mark.parametrize("env", [{"PTCORE_PIPELINE": "wavefront"}, {"PTCORE_SCAN": "bvh"}], ids=["wavefront", "bvh"])
def test_moments_do_not_depend_on_the_trace_form(monkeypatch, inv_ref, env):
    from path_trace_golang_amd import capi

    name, depth, n = INV
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with capi.Context(ndev=1) as ctx:  # both are read by pt_create
        img, acc, m2, st = _render(ctx, _scene(name), n, depth)
    assert np.array_equal(img, inv_ref[0])
    assert np.array_equal(_bits(m2), _bits(inv_ref[2]))


def test_moments_on_two_virtual_devices(inv_ref):
    from path_trace_golang_amd import capi, hip

    name, depth, n = INV
    with capi.Context(devices=[0, 0]) as ctx:
        img, acc, m2, st = _render(ctx, _scene(name), n, depth)
        nz = hip.noise_estimate(ctx)
    assert st["num_devices"] == 2
    assert np.array_equal(img, inv_ref[0]) and np.array_equal(_bits(acc), _bits(inv_ref[1]))
    assert np.array_equal(_bits(m2), _bits(inv_ref[2]))
    ref = inv_ref[3]
    assert abs(nz["noise"] - ref["noise"]) <= 1e-12 * ref["noise"]  # the partials are added in another order there
    assert (nz["max_pixel"], nz["pixels"], nz["bad_pixels"], nz["spp"]) == (ref["max_pixel"], 960, 0, n)


@pytest.mark.parametrize("ndev", [4, 7], ids=["2+2+1+1 tiles", "a device without a tile"])
def test_uneven_shards_gather_the_planes_of_one_device(ndev):
    """70 x 45 = 6 tiles over 4 and over 7 virtual devices (peer copies of unequal length, and none at all from the seventh): every
    plane a context gathers -- rgba, the sums, the counters, the second moments, the sample counts of an adaptive frame -- has the
    bits of the one-device context's."""
    import adaptive_support as ad
    from path_trace_golang_amd import capi

    ref = ad.gather_reference()
    with capi.Context(devices=[0] * ndev) as ctx:
        got = ad.gather_frames(ctx)
    ad.assert_same_planes(got, ref, ndev)
    assert got["ad_state"]["active_blocks"] == ref["ad_state"]["active_blocks"] and got["ad_state"]["samples"] == ref["ad_state"]["samples"]


# ---------------------------------------------------------------- 5. the noise figure
def test_noise_estimate_matches_the_host_formula(inv_ref):
    from path_trace_golang_amd import capi, hip

    name, depth, n = INV
    sc = _scene(name)
    with capi.Context(ndev=1) as ctx:
        img, acc, m2, st = _render(ctx, sc, n, depth)
        a = hip.noise_estimate(ctx)
        b = hip.noise_estimate(ctx)
        assert st["noise"] == a["noise"]
        _, acc1, m21, st1 = _render(ctx, sc, 1, depth)
        one = hip.noise_estimate(ctx)
    host = hip.noise_estimate_host(acc, m2, n)
    print("noise %.17g (host %.17g), max pixel %.6g" % (a["noise"], host["noise"], a["max_pixel"]))
    assert abs(a["noise"] - host["noise"]) <= 1e-9 * host["noise"]
    assert abs(a["max_pixel"] - host["max_pixel"]) <= 1e-9 * host["max_pixel"]
    assert a["pixels"] == 960 and a["bad_pixels"] == 0 and a["spp"] == n
    assert a == b and math.copysign(1, a["noise"]) == 1 and a == inv_ref[3]  # the same bits every time
    assert math.isinf(one["noise"]) and one["noise"] > 0 and one["spp"] == 1 and math.isinf(st1["noise"])
    # against the oracle's moments the figure is as close as the sums are
    S, Q = ms.sums(ms.samples(name, depth, 1, n))
    want = hip.noise_estimate_host(S, Q, n)
    assert abs(a["noise"] - want["noise"]) <= 1e-9 * want["noise"]


# ---------------------------------------------------------------- 6. the stop rule
STOP = ("example_simple", 4, 1, 64, 8)  # scene, depth, seed, cap, step


@pytest.fixture(scope="module")
def stop_case(_built):
    from path_trace_golang_amd import hip

    name, depth, seed, cap, step = STOP
    l = ms.samples(name, depth, seed, cap)
    noise = {}
    for n in range(step, cap + 1, step):
        S, Q = ms.sums(l[:, :, :n])
        noise[n] = hip.noise_estimate_host(S, Q, n)["noise"]
    target = math.sqrt(noise[24] * noise[32])
    # precondition: no checkpoint within 1e-6 relative of the target, and 32 is the first one at or below it
    assert all(abs(v - target) > 1e-6 * target for v in noise.values()), noise
    assert all(noise[n] > target for n in (8, 16, 24)) and noise[32] < target, noise
    return target, noise


def _oracle_frame(oracle, n):
    name, depth, seed, _, _ = STOP
    return oracle.render(ms.ora_scene(name), W, H, n, depth, seed=seed, want=("rgba", "accum"))


@pytest.mark.parametrize("which,want_spp", [("between", 32), ("zero", 64), ("huge", 8)])
def test_render_stops_at_the_noise_target(oracle, stop_case, which, want_spp):
    from path_trace_golang_amd import capi, hip

    name, depth, seed, cap, step = STOP
    target = {"between": stop_case[0], "zero": 0.0, "huge": 1e9}[which]
    sc = _scene(name)
    calls = []
    with capi.Context(ndev=1) as ctx:
        img = np.zeros((H, W, 4), np.uint8)
        acc = np.zeros((H, W, 3))
        st = hip.render(sc, hip.RenderConfig(W, H, cap, depth, seed), img, None, acc, ctx=ctx, noise=target, noise_step=step)
        img_p = np.zeros((H, W, 4), np.uint8)
        st_p = hip.render(sc, hip.RenderConfig(W, H, cap, depth, seed), img_p, lambda: calls.append(1), ctx=ctx, noise=target,
                          noise_step=step)
        if which == "zero":
            plain = np.zeros((H, W, 4), np.uint8)
            plain_acc = np.zeros((H, W, 3))
            hip.render(sc, hip.RenderConfig(W, H, cap, depth, seed), plain, None, plain_acc, ctx=ctx)
            assert np.array_equal(img, plain) and np.array_equal(_bits(acc), _bits(plain_acc))
    o = _oracle_frame(oracle, want_spp)
    assert st["spp_done"] == want_spp and st["samples"] == 960 * want_spp
    assert np.array_equal(img, o["rgba"])
    assert np.all(np.abs(acc - o["accum"]) <= 4 * depth * 2.0 ** -52 * np.maximum(np.abs(o["accum"]), 1e-300))
    assert abs(st["noise"] - stop_case[1][want_spp]) <= 1e-9 * stop_case[1][want_spp]
    assert st_p["spp_done"] == want_spp and np.array_equal(img_p, o["rgba"]) and len(calls) == want_spp // step + 1


@pytest.mark.parametrize("which,want_spp", [("between", 32), ("zero", 64), ("huge", 8)])
def test_cli_stops_at_the_noise_target(tmp_path, oracle, stop_case, which, want_spp):
    from PIL import Image

    name, depth, seed, cap, step = STOP
    target = {"between": repr(stop_case[0]), "zero": "0", "huge": "1e9"}[which]
    out = str(tmp_path / "o.png")
    r = subprocess.run([os.path.join(ROOT, "path_trace_golang_amd", "render"), "-headless", "-gpu", "-scene", scene_path(name),
                        "-out", out, "-width", str(W), "-height", str(H), "-spp", str(cap), "-depth", str(depth), "-seed",
                        str(seed), "-noise", target, "-noise-step", str(step)], capture_output=True, text=True, cwd=ROOT,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    if which != "zero":
        assert "rendered %dx%d, %d of at most %d spp (noise " % (W, H, want_spp, cap) in r.stderr, r.stderr
    o = _oracle_frame(oracle, want_spp)
    im = Image.open(out)
    assert im.size == (W, H) and np.array_equal(np.array(im.convert("RGB")), o["rgba"][..., :3])


# ---------------------------------------------------------------- 7. two seeds
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_two_seeds_differ_by_what_the_moments_predict(name):
    """Seeds 1 and 2 at n = 32: the squared difference of the two means and the sum of the two variance-of-the-mean
    estimates both have expectation 2 sigma^2 / n per pixel and channel, so their ratio over the frame tends to 1.  The
    oracle alone gives 1.037 / 0.961 / 1.045 / 1.141 / 0.969 on the five scenes; over 20 seed pairs it stayed within
    0.906 - 1.146."""
    from path_trace_golang_amd import capi

    n, depth = 32, DEPTHS[name]
    sc = _scene(name)
    mean, var = [], []
    with capi.Context(ndev=1) as ctx:
        for seed in (1, 2):
            _, acc, m2, _ = _render(ctx, sc, n, depth, seed)
            m = acc / n
            mean.append(m)
            var.append(np.maximum(m2 / n - m * m, 0.0) / (n - 1))
    R = float(np.sum((mean[0] - mean[1]) ** 2) / np.sum(var[0] + var[1]))
    print("%s: R = %.4f" % (name, R))
    assert 0.8 <= R <= 1.25, R


# ---------------------------------------------------------------- 8. state
def test_reads_need_a_frame_with_moments_and_off_is_off(oracle):
    from path_trace_golang_amd import capi, hip

    L = capi.load()
    name, depth, n, seed = "test_comprehensive", 6, 3, 5
    sc = _scene(name)
    o = oracle.render(ms.ora_scene(name), W, H, n, depth, seed=seed)
    buf = np.zeros((H, W, 3))
    p = buf.ctypes.data_as(C.POINTER(C.c_double))
    nz = capi.PtNoise()
    with capi.Context(ndev=1) as ctx, capi.Context(ndev=1) as fresh:
        # no frame yet, then a frame with moments off: PT_ERR_STATE with a message, and the context stays usable
        for _ in range(2):
            assert L.pt_read_moments(ctx.handle, p) == capi.PT_ERR_STATE and L.pt_last_error()
            assert L.pt_noise_estimate(ctx.handle, C.byref(nz)) == capi.PT_ERR_STATE and L.pt_last_error()
            render_vs_oracle(ctx, sc, o, W, H, n, depth, seed, tag="moments off")
        assert L.pt_read_moments(ctx.handle, p) == capi.PT_ERR_STATE and b"moments off" in L.pt_last_error()
        # NULL outputs on a live context
        assert L.pt_read_moments(ctx.handle, None) == capi.PT_ERR_INVALID
        assert L.pt_noise_estimate(ctx.handle, None) == capi.PT_ERR_INVALID
        # a frame with moments on, then a call without the arguments: the frame of a fresh context, and no moments to read
        _, _, m2, _ = _render(ctx, sc, n, depth, seed)
        assert np.any(m2 > 0)
        a = _render(ctx, sc, n, depth, seed, want_moments=False)
        b = _render(fresh, sc, n, depth, seed, want_moments=False)
        assert "noise" not in a[3] and "spp_done" not in a[3]
        assert np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))
        for k in ("samples", "segments", "exit_scans", "draws"):
            assert a[3][k] == b[3][k] == o["stats"][k]
        assert L.pt_read_moments(ctx.handle, p) == capi.PT_ERR_STATE
        # pt_set_moments is refused while a frame is open
        flat = hip.FlatScene(sc)
        pc = hip.pt_config(hip.RenderConfig(W, H, n, depth, seed))
        capi.check(L.pt_begin(ctx.handle, C.byref(flat.c), C.byref(pc)))
        assert L.pt_set_moments(ctx.handle, 1) == capi.PT_ERR_STATE
        capi.check(L.pt_end(ctx.handle, None))
