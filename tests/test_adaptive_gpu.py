"""Adaptive sampling on the MI355X (pt_set_adaptive, block_noise_kernel, compact_kernel and the adaptive forms of ray generation,
resolve, moments, fog and noise).  The reference of the main case is the oracle: the count map predicted from its
per-sample radiances (adaptive_support.CASE, preconditions in test_adaptive_cpu.py) must come back exactly, and every block must
hold the oracle's n-sample pixels.  Where the oracle is slow or absent the check is self-consistency: a block that stopped at n
is bit-equal to the same block of a plain n-sample frame of the same context.

No frame here has more than 54 blocks on a device.  Lists longer than one wave and one strip of compact_kernel are in
test_adaptive_scale_gpu.py (frames of 1184 blocks) and test_adaptive_probe_gpu.py (the two check kernels by themselves, through
tests/adaptive_probe.hip, built by adaptive_probe_support.py)."""
from __future__ import annotations

import copy
import ctypes as C

import numpy as np
import pytest

import adaptive_support as ad
import moments_support as ms
from adaptive_support import bits
from conftest import render_vs_oracle, scene_path
from moments_support import H, W

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, scope="module")
def _built(gpu_ctx):
    return gpu_ctx


def _scene(name):
    from path_trace_golang_amd import scene

    return scene.load(scene_path(name))


@pytest.fixture(scope="module")
def case_ref(_built, oracle):
    """The oracle's side of the case: per distinct count n its n-sample frame and second moments (computed once, read-only)."""
    name, depth, seed, cap, step, min_spp, target = ad.CASE
    l = ms.samples(name, depth, seed, cap)
    ref = {}
    for n in sorted({n for row in ad.CASE_MAP for n in row}):
        o = oracle.render(ms.ora_scene(name), W, H, n, depth, seed=seed)
        _, Q = ms.sums(l[:, :, :n])
        for a in (o["rgba"], o["accum"], o["nseg"], o["ndraw"], Q):
            a.setflags(write=False)
        ref[n] = (o, Q)
    want = ad.expand(ad.CASE_MAP)
    want.setflags(write=False)
    return ref, want


def _check_against_the_oracle(case_ref, img, acc, m2, counts, nseg, ndraw):
    ref, want = case_ref
    depth = ad.CASE[1]
    assert np.array_equal(counts, want), counts[::8, ::8].tolist()
    assert counts.min() > 0  # zeros nowhere inside the frame
    for n, (o, Q) in ref.items():
        sel = want == n
        assert np.array_equal(img[sel], o["rgba"][sel]), ("rgba", n)
        rel = np.abs(acc[sel] - o["accum"][sel]) / np.maximum(np.abs(o["accum"][sel]), 1e-300)
        rel2 = np.abs(m2[sel] - Q[sel]) / np.maximum(np.abs(Q[sel]), 1e-300)
        print("n = %2d: accum max rel err %.3g (bound %.3g), m2 max rel err %.3g (bound %.3g)"
              % (n, rel.max(), 4 * depth * 2.0 ** -52, rel2.max(), (8 * depth + n) * 2.0 ** -52))
        assert np.all(rel <= 4 * depth * 2.0 ** -52), ("accum", n)
        assert np.all(rel2 <= (8 * depth + n) * 2.0 ** -52), ("m2", n)
        if nseg is not None:
            assert np.array_equal(nseg[sel], o["nseg"][sel]) and np.array_equal(ndraw[sel], o["ndraw"][sel]), ("nseg / ndraw", n)


# ---------------------------------------------------------------- 1. the case, against the oracle
@pytest.mark.parametrize("form", ["stats", "shipping", "stepped"])
def test_the_case_matches_the_oracle_block_by_block(case_ref, form):
    """stats / shipping: through pt_render (which steps internally), both builds of the kernels; stepped: the host steps
    pt_begin / pt_step / pt_read itself (hip.render with a progress callback)."""
    from path_trace_golang_amd import capi

    name, depth, seed, cap, step, min_spp, target = ad.CASE
    calls = []
    with capi.Context(ndev=1) as ctx:
        img, acc, m2, counts, nseg, ndraw, st = ad.render_adaptive(
            ctx, _scene(name), W, H, cap, depth, seed, target, step, min_spp, flags=capi.PT_FLAG_PIXEL_STATS if form == "stats" else 0,
            progress=(lambda: calls.append(1)) if form == "stepped" else None)
    _check_against_the_oracle(case_ref, img, acc, m2, counts, nseg, ndraw)
    assert st["samples"] == ad.CASE_SAMPLES
    ad.check_state(st, counts, cap)
    a = st["adaptive"]
    assert (a["blocks"], a["active_blocks"], a["samples"], a["spp_min"], a["spp_max"]) == (15, 3, ad.CASE_SAMPLES, 16, 64)
    assert a["worst_active"] > target
    assert st["segments"] == sum(int(o["nseg"][case_ref[1] == n].sum()) for n, (o, _) in case_ref[0].items())
    assert st["draws"] == sum(int(o["ndraw"][case_ref[1] == n].sum()) for n, (o, _) in case_ref[0].items())
    if form == "stepped":
        assert len(calls) == cap // step + 1


def test_the_case_through_the_c_abi(case_ref):
    """pt_set_adaptive + pt_render directly, and the reads after pt_end."""
    from path_trace_golang_amd import capi, hip

    name, depth, seed, cap, step, min_spp, target = ad.CASE
    L = capi.load()
    flat = hip.FlatScene(_scene(name))
    pc = hip.pt_config(hip.RenderConfig(W, H, cap, depth, seed))
    img = np.zeros((H, W, 4), np.uint8)
    acc = np.zeros((H, W, 3))
    m2 = np.zeros((H, W, 3))
    counts = np.zeros((H, W), np.uint32)
    st = capi.PtStats()
    a = capi.PtAdaptive(target, min_spp, step)
    with capi.Context(ndev=1) as ctx:
        capi.check(L.pt_set_adaptive(ctx.handle, C.byref(a)))  # (implies moments for the frame)
        capi.check(L.pt_render(ctx.handle, C.byref(flat.c), C.byref(pc), img.ctypes.data_as(C.c_void_p), W * 4,
                               acc.ctypes.data_as(C.c_void_p), None, None, C.byref(st)))
        hip.read_sample_counts(ctx, counts)
        hip.read_moments(ctx, m2)
        state = hip.adaptive_state(ctx)
        nz = hip.noise_estimate(ctx)
        assert L.pt_set_adaptive(ctx.handle, None) == capi.PT_OK
        assert hip.adaptive_state(ctx) == state  # the last frame stays readable until the next one opens
    _check_against_the_oracle(case_ref, img, acc, m2, counts, None, None)
    assert st.samples == ad.CASE_SAMPLES and state["samples"] == ad.CASE_SAMPLES and state["active_blocks"] == 3
    host = _noise_per_pixel(acc, m2, counts)
    assert abs(nz["noise"] - host) <= 1e-9 * host and nz["spp"] == 64 and nz["pixels"] == W * H and nz["bad_pixels"] == 0


def _noise_per_pixel(acc, m2, counts):
    """The NumPy form of pt_noise_estimate with every pixel's own n."""
    n = counts.astype(np.float64)[..., None]
    m = acc / n
    v = np.maximum(m2 / n - m * m, 0.0) / (n - 1.0)
    den = np.maximum(m.sum(axis=2) / 3.0, 0.01)
    e2 = (v.sum(axis=2) / 3.0) / (den * den)
    return float(np.sqrt(np.where(np.isfinite(e2), e2, 0.0).sum() / e2.size))


# ---------------------------------------------------------------- 2. target 0 and a huge target
def test_target_zero_is_the_plain_frame_and_a_huge_target_stops_at_the_first_check():
    from path_trace_golang_amd import capi, hip

    name, depth, seed, cap, step, min_spp, _ = ad.CASE
    sc = _scene(name)
    with capi.Context(ndev=1) as ctx:
        img, acc, m2, counts, _, _, st = ad.render_adaptive(ctx, sc, W, H, cap, depth, seed, 0.0, step)
        pi = np.zeros((H, W, 4), np.uint8)
        pa = np.zeros((H, W, 3))
        pm = np.zeros((H, W, 3))
        pst = hip.render(sc, hip.RenderConfig(W, H, cap, depth, seed), pi, None, pa, ctx=ctx, moments=pm)
        assert np.array_equal(img, pi) and np.array_equal(bits(acc), bits(pa)) and np.array_equal(bits(m2), bits(pm))
        assert np.all(counts == cap) and st["adaptive"]["active_blocks"] == 15
        for k in ("samples", "segments", "exit_scans", "draws"):
            assert st[k] == pst[k], k
        assert st["noise"] == pst["noise"]  # the adaptive noise kernel with every n equal is the plain one, bit for bit
        _, _, _, counts, _, _, st = ad.render_adaptive(ctx, sc, W, H, cap, depth, seed, 1e9, step)
        assert np.all(counts == step) and st["adaptive"]["active_blocks"] == 0 and st["samples"] == W * H * step
        _, _, _, counts, _, _, st = ad.render_adaptive(ctx, sc, W, H, cap, depth, seed, 1e9, step, min_spp=20)
        assert np.all(counts == 24)  # the first check at or past min_spp
        _, _, _, counts, _, _, st = ad.render_adaptive(ctx, sc, W, H, cap, depth, seed, 1e9, 1)
        assert np.all(counts == 2)   # one sample gives no variance estimate


def test_the_check_and_the_frame_noise_share_one_metric():
    """block_noise_kernel (through compact_kernel: pt_adaptive_state's worst_active) and noise_kernel (pt_noise_estimate's max_pixel)
    against noise_estimate_host's per-pixel e2 of the frame's own sums, after each of two steps of a frame whose blocks all stay
    active (target 0): the largest block noise, and the largest pixel.  The tolerance is test_noise_estimate_matches_the_host_formula's."""
    from path_trace_golang_amd import capi, hip

    name, depth, seed, _, step, min_spp, _ = ad.CASE
    w, h = ad.GATHER_W, ad.GATHER_H
    L = capi.load()
    flat = hip.FlatScene(_scene(name))
    pc = hip.pt_config(hip.RenderConfig(w, h, 2 * step, depth, seed))
    img = np.zeros((h, w, 4), np.uint8)
    acc = np.zeros((h, w, 3))
    m2 = np.zeros((h, w, 3))
    done = C.c_int32(0)
    with capi.Context(ndev=1) as ctx:
        hip.set_adaptive(ctx, 0.0, min_spp, step)
        capi.check(L.pt_begin(ctx.handle, C.byref(flat.c), C.byref(pc)))
        for k in (1, 2):
            capi.check(L.pt_step(ctx.handle, step, C.byref(done)))
            n = done.value
            assert n == k * step
            capi.check(L.pt_read(ctx.handle, img.ctypes.data_as(C.c_void_p), w * 4, acc.ctypes.data_as(C.c_void_p)))
            hip.read_moments(ctx, m2)
            state = hip.adaptive_state(ctx)
            nz = hip.noise_estimate(ctx)
            assert state["active_blocks"] == state["blocks"] == 54 and nz["bad_pixels"] == 0
            block, pixel = [], []
            for y in range(0, h, 8):
                for x in range(0, w, 8):
                    b = hip.noise_estimate_host(acc[y:y + 8, x:x + 8], m2[y:y + 8, x:x + 8], n)  # noise = sqrt(sum of e2 / the block's pixels)
                    block.append(b["noise"])
                    pixel.append(b["max_pixel"])
            print("n = %d: worst_active %.17g (host %.17g), max_pixel %.17g (host %.17g)" % (n, state["worst_active"], max(block),
                                                                                             nz["max_pixel"], max(pixel)))
            assert max(block) > 0 and abs(state["worst_active"] - max(block)) <= 1e-9 * max(block)
            assert abs(nz["max_pixel"] - max(pixel)) <= 1e-9 * max(pixel)
        capi.check(L.pt_end(ctx.handle, None))


# ---------------------------------------------------------------- 3. self-consistency
@pytest.mark.parametrize("chunk", [3, 5])
def test_the_map_does_not_depend_on_the_chunk(case_ref, chunk):
    from path_trace_golang_amd import capi

    name, depth, seed, cap, step, min_spp, target = ad.CASE
    with capi.Context(ndev=1) as ctx:
        counts, st = ad.check_self_consistent(ctx, _scene(name), W, H, cap, depth, seed, target, step, min_spp, chunk=chunk, min_distinct=4)
    assert st["spp_chunk"] == chunk
    assert np.array_equal(counts, case_ref[1])


def test_two_virtual_devices(case_ref):
    from path_trace_golang_amd import capi

    name, depth, seed, cap, step, min_spp, target = ad.CASE
    with capi.Context(devices=[0, 0]) as ctx:
        counts, st = ad.check_self_consistent(ctx, _scene(name), W, H, cap, depth, seed, target, step, min_spp, min_distinct=4)
    assert st["num_devices"] == 2
    assert np.array_equal(counts, case_ref[1])


def _median_block_noise(ctx, sc, w, h, n, depth, seed, **kw):
    """A target that splits the frame's blocks: the median of their own noise after n samples (a plain frame of ctx)."""
    from path_trace_golang_amd import hip

    img = np.zeros((h, w, 4), np.uint8)
    acc = np.zeros((h, w, 3))
    m2 = np.zeros((h, w, 3))
    hip.render(sc, hip.RenderConfig(w, h, n, depth, seed), img, None, acc, ctx=ctx, moments=m2, **kw)
    m = acc / n
    v = np.maximum(m2 / n - m * m, 0.0) / (n - 1)
    den = np.maximum(m.sum(axis=2) / 3.0, 0.01)
    e2 = (v.sum(axis=2) / 3.0) / (den * den)
    e2 = np.where(np.isfinite(e2), e2, 0.0)
    b = [float(np.sqrt(e2[y:y + 8, x:x + 8].mean())) for y in range(0, h, 8) for x in range(0, w, 8)]
    return float(np.median(b))


@pytest.mark.parametrize("lens", [True, False], ids=["thin lens", "pinhole"])
@pytest.mark.parametrize("w,h", [(W, H), (37, 21)], ids=["40x24", "37x21"])
def test_ragged_frames_with_and_without_the_thin_lens(lens, w, h):
    """metal_glass_room (aperture 0.1, glass: split rounds and the nested tail); 37 x 21 cuts the last block column and row."""
    from path_trace_golang_amd import capi

    sc = copy.deepcopy(_scene("metal_glass_room"))
    assert sc.camera.aperture > 0
    if not lens:
        sc.camera.aperture = 0.0
    with capi.Context(ndev=1) as ctx:
        target = _median_block_noise(ctx, sc, w, h, 8, 6, 1)
        ad.check_self_consistent(ctx, sc, w, h, 24, 6, 1, target, 4)


def test_the_fog_block():
    from path_trace_golang_amd import capi, hip

    sc = _scene("gpu_showcase")
    assert sc.fog is not None and sc.fog.gpu_volumetric
    with capi.Context(ndev=1) as ctx:
        target = _median_block_noise(ctx, sc, W, H, 8, 8, 1, fog=True)
        ad.check_self_consistent(ctx, sc, W, H, 24, 8, 1, target, 4, fog=True)
        fst = hip.fog_last_stats(ctx)
    assert fst["fog_launches"] >= 1 and fst["shadow_rays"] > 0


@pytest.mark.parametrize("nobj", [65, 300], ids=["grouped scan", "hierarchy"])
def test_grouped_and_hierarchy_scenes(nobj):
    """65 objects: the grouped candidate masks; 300: the hierarchy with its wave-cooperative primary pass (cap 16, step 4)."""
    from path_trace_golang_amd import capi, synth

    sc = synth.make_scene(nobj, 4)
    with capi.Context(ndev=1) as ctx:
        target = _median_block_noise(ctx, sc, W, H, 8, 5, 1)
        ad.check_self_consistent(ctx, sc, W, H, 16, 5, 1, target, 4)


# ---------------------------------------------------------------- 4. progressive use
EARLY_TARGET = 0.55  # on the oracle's samples every block of the case is at or below it by 24 samples (nearest check 2 % away)


def test_reading_between_steps_changes_nothing_and_a_finished_frame_adds_nothing(case_ref):
    from path_trace_golang_amd import capi, hip

    name, depth, seed, cap, step, min_spp, target = ad.CASE
    L = capi.load()
    sc = _scene(name)
    flat = hip.FlatScene(sc)
    img = np.zeros((H, W, 4), np.uint8)
    acc = np.zeros((H, W, 3))
    m2 = np.zeros((H, W, 3))

    def frame(ctx, tgt, cap_, read_every_step):
        hip.set_adaptive(ctx, tgt, min_spp, step)
        pc = hip.pt_config(hip.RenderConfig(W, H, cap_, depth, seed))
        capi.check(L.pt_begin(ctx.handle, C.byref(flat.c), C.byref(pc)))
        counts = np.zeros((H, W), np.uint32)
        assert L.pt_read_sample_counts(ctx.handle, counts.ctypes.data_as(C.POINTER(C.c_uint32))) == capi.PT_ERR_STATE  # no step yet
        done, seen = C.c_int32(0), []
        for _ in range(cap_ // step + 2):  # two steps more than the frame can take
            capi.check(L.pt_step(ctx.handle, step, C.byref(done)))
            seen.append(done.value)
            if read_every_step:
                capi.check(L.pt_read(ctx.handle, img.ctypes.data_as(C.c_void_p), W * 4, acc.ctypes.data_as(C.c_void_p)))
                hip.read_sample_counts(ctx, counts)
                hip.noise_estimate(ctx)
                assert counts.max() == done.value
        capi.check(L.pt_read(ctx.handle, img.ctypes.data_as(C.c_void_p), W * 4, acc.ctypes.data_as(C.c_void_p)))
        hip.read_sample_counts(ctx, counts)
        hip.read_moments(ctx, m2)
        nz = hip.noise_estimate(ctx)
        state = hip.adaptive_state(ctx)
        st = capi.PtStats()
        capi.check(L.pt_end(ctx.handle, C.byref(st)))
        return counts, seen, img.copy(), acc.copy(), m2.copy(), nz, state, st

    with capi.Context(ndev=1) as ctx:
        a = frame(ctx, target, cap, True)
        b = frame(ctx, target, cap, False)
        # a frame whose blocks all stop before the cap: the steps after the last stop add nothing and return the last value
        early = frame(ctx, EARLY_TARGET, cap, False)
    assert np.array_equal(a[0], case_ref[1]) and np.array_equal(b[0], case_ref[1])
    assert a[1] == b[1] == [8, 16, 24, 32, 40, 48, 56, 64, 64, 64]
    assert np.array_equal(a[2], b[2]) and np.array_equal(bits(a[3]), bits(b[3])) and np.array_equal(bits(a[4]), bits(b[4]))
    assert a[5] == b[5] and a[6] == b[6] and a[7].samples == b[7].samples == ad.CASE_SAMPLES
    host = _noise_per_pixel(a[3], a[4], a[0])
    assert abs(a[5]["noise"] - host) <= 1e-9 * host and a[5]["spp"] == 64
    counts, seen, _, acc_e, m2_e, nz, state, st = early
    want, checks = ad.plan_restated(ms.samples(name, depth, seed, cap), EARLY_TARGET, step, min_spp, cap)
    want = np.asarray(want)
    # the preconditions of this part: every block stops before the cap, and no check is within 1e-6 of the target
    assert want.max() < cap and min(abs(b - EARLY_TARGET) / EARLY_TARGET for _, _, _, b in checks) > 1e-6
    assert np.array_equal(counts, ad.expand(want))
    last = int(want.max())
    assert seen == list(range(step, last + 1, step)) + [last] * (cap // step + 2 - last // step)
    assert state["active_blocks"] == 0 and state["worst_active"] == 0 and state["spp_max"] == last
    assert st.samples == int(counts.sum()) == state["samples"]
    host = _noise_per_pixel(acc_e, m2_e, counts)
    assert abs(nz["noise"] - host) <= 1e-9 * host and nz["spp"] == last


# ---------------------------------------------------------------- 5. refusals and state
def test_refusals_leave_the_context_usable(oracle, monkeypatch):
    from path_trace_golang_amd import capi, hip

    L = capi.load()
    name, depth, n, seed = "example_simple", 4, 3, 5
    sc = _scene(name)
    o = oracle.render(ms.ora_scene(name), W, H, n, depth, seed=seed)
    flat = hip.FlatScene(sc)
    pc = hip.pt_config(hip.RenderConfig(W, H, n, depth, seed))
    img = np.zeros((H, W, 4), np.uint8)
    counts = np.zeros((H, W), np.uint32)
    pcounts = counts.ctypes.data_as(C.POINTER(C.c_uint32))
    st = capi.PtAdaptiveState()

    def refused(ctx, what):
        for call in (lambda: L.pt_begin(ctx.handle, C.byref(flat.c), C.byref(pc)),
                     lambda: L.pt_render(ctx.handle, C.byref(flat.c), C.byref(pc), img.ctypes.data_as(C.c_void_p), W * 4, None, None, None, None)):
            assert call() == capi.PT_ERR_STATE
            assert what in L.pt_last_error(), L.pt_last_error()
        assert L.pt_step(ctx.handle, 1, None) == capi.PT_ERR_STATE  # no frame was opened

    with capi.Context(ndev=1) as ctx:
        # nothing to read before a frame, nor after a frame that was not adaptive
        assert L.pt_adaptive_state(ctx.handle, C.byref(st)) == capi.PT_ERR_STATE and L.pt_last_error()
        render_vs_oracle(ctx, sc, o, W, H, n, depth, seed, tag="before")
        assert L.pt_read_sample_counts(ctx.handle, pcounts) == capi.PT_ERR_STATE
        hip.set_moments(ctx, True)
        capi.check(L.pt_render(ctx.handle, C.byref(flat.c), C.byref(pc), img.ctypes.data_as(C.c_void_p), W * 4, None, None, None, None))
        assert L.pt_adaptive_state(ctx.handle, C.byref(st)) == capi.PT_ERR_STATE and b"adaptive sampling off" in L.pt_last_error()
        assert L.pt_adaptive_state(ctx.handle, None) == capi.PT_ERR_INVALID and L.pt_read_sample_counts(ctx.handle, None) == capi.PT_ERR_INVALID
        # bad arguments
        for bad in (capi.PtAdaptive(-1.0, 0, 8), capi.PtAdaptive(float("nan"), 0, 8), capi.PtAdaptive(0.1, -1, 8)):
            assert L.pt_set_adaptive(ctx.handle, C.byref(bad)) == capi.PT_ERR_INVALID
        # GL shading together with adaptive
        hip.set_adaptive(ctx, 0.25, 0, 8)
        hip.set_shading(ctx, "gl", sc)
        refused(ctx, b"GL shading")
        hip.set_shading(ctx, "cpu")
        # injected primary rays together with adaptive
        ctx.set_primary_rays(np.zeros((W * H * n, 6)) + 1.0)
        refused(ctx, b"injected primary rays")
        ctx.set_primary_rays(None)
        # the device entry point neither adapts nor fails
        import torch

        ntl = C.c_int32(0)
        capi.check(L.pt_shard_tiles(W, H, None, C.byref(ntl), None, None))
        tiles = torch.zeros((ntl.value, 32, 32, 4), dtype=torch.uint8, device="cuda:0")
        capi.check(L.pt_render_tiles_device(ctx.handle, C.byref(flat.c), C.byref(pc), None, C.c_void_p(tiles.data_ptr()), None, None,
                                            C.byref(capi.PtStats())))
        assert L.pt_read_sample_counts(ctx.handle, pcounts) == capi.PT_ERR_STATE
        assert np.array_equal(tiles[0, :H, :32].cpu().numpy(), o["rgba"][:, :32])
        # pt_set_adaptive is refused while a frame is open, and the frame it would have changed is an adaptive one
        capi.check(L.pt_begin(ctx.handle, C.byref(flat.c), C.byref(pc)))
        assert L.pt_set_adaptive(ctx.handle, None) == capi.PT_ERR_STATE
        capi.check(L.pt_step(ctx.handle, n, None))
        capi.check(L.pt_adaptive_state(ctx.handle, C.byref(st)))
        assert (st.blocks, st.spp_max) == (15, n)
        capi.check(L.pt_end(ctx.handle, None))
        hip.set_adaptive(ctx, None)
        render_vs_oracle(ctx, sc, o, W, H, n, depth, seed, tag="after")
    # the wavefront and walk32 pipelines have no adaptive job map: refused cleanly
    for form in ("wavefront", "walk32"):
        monkeypatch.setenv("PTCORE_PIPELINE", form)
        with capi.Context(ndev=1) as ctx:  # read by pt_create
            hip.set_adaptive(ctx, 0.25, 0, 8)
            refused(ctx, b"PTCORE_PIPELINE")
            hip.set_adaptive(ctx, None)
            render_vs_oracle(ctx, sc, o, W, H, n, depth, seed, tag=form)
