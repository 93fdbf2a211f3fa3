"""Chosen primary rays through every scan form that ships, compared with the oracle ray by ray.

Frames only ever feed the trace kernels a camera's rays and what the bounces make of them: waves of 64 near-identical rays,
directions of length about 1, origins inside the scene.  pt_debug_set_primary_rays (include/ptcore.h) overwrites the ray
planes after ray generation, so the six classes of ray_inject_support.py -- direction lengths over 1200 binades, degenerate
components, origins on and a few ulps off the geometry, origins around every bound the kernels switch on, incoherent waves,
and waves in which ONE lane is odd -- go through the shipped kernels untouched: split, nested and all-in-one trace_kernel,
glass_kernel, the grouped scan, primary_bvh_kernel with the hierarchy's loop behind it, the wavefront and walk32 pipelines.
Every ray is compared with ora_sample_ray (oracle/pt_oracle.c): counts and the 8-bit pixel equal, the FP64 sum within
4 * depth * 2^-52; no ray is skipped.  The self-checking contexts must count no disagreement between the culled scan and the
plain loop, except under PTCORE_DEBUG_DROP, where they must."""
import ctypes as C
import os

import numpy as np
import pytest

import ray_inject_support as S

pytestmark = pytest.mark.gpu

# contexts by what pt_create reads from the environment
FORMS = {"split rounds 0": {"PTCORE_SPLIT_ROUNDS": "0"}, "split rounds 3": {"PTCORE_SPLIT_ROUNDS": "3"},
         "tail trip": {"PTCORE_TAIL": "trip"}, "wavefront": {"PTCORE_PIPELINE": "wavefront"}, "walk32": {"PTCORE_PIPELINE": "walk32"},
         "primary pass off": {"PTCORE_PRIMARY": "lane"}}
# the scenes on which a form is another code path than the default (frame_open in csrc/ptcore.hip)
FORM_SCENES = {"split rounds 0": ("bitmask", "grouped"), "split rounds 3": ("bitmask", "grouped"), "tail trip": ("bitmask", "grouped"),
               "wavefront": ("bitmask", "bvh"), "walk32": ("bvh",), "primary pass off": ("bvh",)}
ENV_KEYS = ("PTCORE_SCAN", "PTCORE_SPLIT_ROUNDS", "PTCORE_TAIL", "PTCORE_PIPELINE", "PTCORE_PRIMARY", "PTCORE_DEBUG_DROP")


def _context_with(env):
    from path_trace_golang_amd import capi

    old = {k: os.environ.get(k) for k in ENV_KEYS}
    try:
        for k in ENV_KEYS:
            os.environ.pop(k, None)
        os.environ.update(env)
        return capi.Context(ndev=1)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def contexts(gpu_ctx):
    out = {"default": gpu_ctx}
    for mode in S.VERIFY_MODE.values():
        out[mode] = _context_with({"PTCORE_SCAN": mode})
    for name, env in FORMS.items():
        out[name] = _context_with(env)
    yield out
    for name, c in out.items():
        if name != "default":
            c.close()


_SCENES = {}


def _scene(name):
    from path_trace_golang_amd import scene

    if name not in _SCENES:
        doc = S.scene_doc(name)
        _SCENES[name] = (doc, scene.Scene.decode(doc))
    return _SCENES[name]


def _oracle(oracle, scene_name, class_name):
    doc, _ = _scene(scene_name)
    return S.oracle_frame(oracle, doc, S.classes()[class_name], key=(scene_name, class_name))


def _mismatches(ctx):
    from path_trace_golang_amd import capi

    return capi.load().pt_debug_scan_mismatches(ctx.handle)


def _report(oracle, scene_name, class_name, where, delta):
    doc, _ = _scene(scene_name)
    rays = S.classes()[class_name]
    ids = S.first_hits(oracle, doc, rays)
    fin = S.is_finite(rays)
    o = _oracle(oracle, scene_name, class_name)
    print("injected rays: %-13s on %-10s [%s]: %d rays, %d hit / %d miss / %d non-finite, %d segments, scan-mismatch delta %s"
          % (class_name, scene_name, where, len(rays), np.count_nonzero(fin & (ids >= 0)), np.count_nonzero(fin & (ids < 0)),
             np.count_nonzero(~fin), int(o["nseg"].sum()), delta))


# class 5 on the small scene first, then every class on every scene
DEFAULT_CASES = [("bitmask", "incoherent")] + [(s, c) for s in S.SCENE_NAMES for c in ("length", "components", "near geometry", "far origins", "incoherent", "mixed")
                                               if (s, c) != ("bitmask", "incoherent")]


@pytest.mark.parametrize("scene_name,class_name", DEFAULT_CASES)
def test_default_context_matches_the_oracle_ray_by_ray(contexts, oracle, scene_name, class_name):
    _, sc = _scene(scene_name)
    o = _oracle(oracle, scene_name, class_name)
    S.injected_vs_oracle(contexts["default"], sc, o, S.classes()[class_name], tag=(scene_name, class_name))
    _report(oracle, scene_name, class_name, "default, both builds", "n/a")


@pytest.mark.parametrize("scene_name", list(S.SIZE_CLASSES))
def test_verify_contexts_count_nothing(contexts, oracle, scene_name):
    """Every scan of every injected ray by the culled strategy AND by the reference's plain loop: no disagreement, and the frame
    (rendered from the plain loop's answers) is the oracle's."""
    _, sc = _scene(scene_name)
    mode = S.VERIFY_MODE[scene_name]
    ctx = contexts[mode]
    for class_name, rays in S.classes().items():
        before = _mismatches(ctx)
        S.injected_vs_oracle(ctx, sc, _oracle(oracle, scene_name, class_name), rays, tag=(mode, class_name))
        delta = _mismatches(ctx) - before
        _report(oracle, scene_name, class_name, mode, delta)
        assert delta == 0, (mode, class_name, delta)


@pytest.mark.parametrize("form", list(FORMS))
def test_other_forms_match_the_same_oracle_output(contexts, oracle, form):
    for scene_name in FORM_SCENES[form]:
        _, sc = _scene(scene_name)
        for class_name, rays in S.classes().items():
            S.injected_vs_oracle(contexts[form], sc, _oracle(oracle, scene_name, class_name), rays, tag=(form, scene_name, class_name))
            _report(oracle, scene_name, class_name, form, "n/a")


@pytest.mark.parametrize("form", ["walk32", "wavefront", "default"])
def test_named_axis_parallel_rays_beside_a_core(contexts, oracle, form):
    """The rays the FP32 walk of walk32 got wrong (NAMED_RAYS in ray_inject_support.py): two zero direction components, whose NaN
    slab parameters made every core ahead of the ray count as pierced, wherever it lay sideways."""
    doc, sc = _scene("bvh")
    rays = S.named_table("beside a core")
    o = S.oracle_frame(oracle, doc, rays, key=("bvh", "beside a core"))
    S.injected_vs_oracle(contexts[form], sc, o, rays, tag=(form, "beside a core"))


@pytest.mark.parametrize("scene_name", list(S.SIZE_CLASSES))
def test_ragged_frame_three_samples_chunk_two(contexts, oracle, scene_name):
    """The table's indexing, (y*w + x)*spp + s: 33 x 31 pixels (edge tiles with jobs outside the frame), three samples in chunks
    of two (a chunk that starts at sample 2), an independent ray per sample."""
    doc, sc = _scene(scene_name)
    w, h, spp = 33, 31, 3
    rays = S.indexing_rays(w, h, spp)
    o = S.oracle_frame(oracle, doc, rays, w, h, spp, key=(scene_name, "indexing"))
    S.injected_vs_oracle(contexts["default"], sc, o, rays, w, h, spp, chunk=2, tag=(scene_name, "33x31x3, chunk 2"))
    S.injected_vs_oracle(contexts["default"], sc, o, rays, w, h, spp, chunk=0, tag=(scene_name, "33x31x3, one chunk"), forms=("shipping",))


def _camera_rays(oracle, doc, w, h, spp):
    osc = oracle.Scene(doc)
    return np.array([sum(oracle.primary_ray(osc, w, h, spp, S.DEPTH, S.SEED, x, y, s), []) for y in range(h) for x in range(w) for s in range(spp)])


def _same(a, b):
    return (np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
            and all(a[4][k] == b[4][k] for k in ("samples", "segments", "exit_scans", "draws")))


@pytest.mark.parametrize("scene_name", list(S.SIZE_CLASSES))
def test_injecting_the_cameras_own_rays_changes_nothing(contexts, oracle, scene_name):
    """Identity: the rays ora_primary_ray reports, injected, give the frame, the sums and the counts of the same render without a
    table, byte for byte -- in one call and stepped -- and after clearing the table the next frame is the ordinary one."""
    from path_trace_golang_amd import capi, hip

    doc, sc = _scene(scene_name)
    ctx = contexts["default"]
    w, h, spp = 33, 31, 3
    rays = _camera_rays(oracle, doc, w, h, spp)
    plain = S.render_injected(ctx, sc, None, w, h, spp, chunk=2)
    assert plain[4]["segments"] > w * h * spp
    assert _same(S.render_injected(ctx, sc, rays, w, h, spp, chunk=2), plain)
    for stats in (True, False):  # a table of other rays in between; then cleared: the ordinary frame again
        other = S.render_injected(ctx, sc, S.indexing_rays(w, h, spp), w, h, spp, chunk=2, stats=stats)
        assert other[1].tobytes() != plain[1].tobytes()
    assert _same(S.render_injected(ctx, sc, None, w, h, spp, chunk=2), plain)
    # stepped with pt_step, one sample at a time (chunks of one, two ... as the cadence cuts them)
    L = capi.load()
    flat = hip.FlatScene(sc)
    pc = hip.pt_config(hip.RenderConfig(w, h, spp, S.DEPTH, S.SEED, 2, 0))
    frames = []
    for table in (rays, None):
        ctx.set_primary_rays(table)
        try:
            img, acc, done = np.zeros((h, w, 4), np.uint8), np.zeros((h, w, 3)), C.c_int32(0)
            capi.check(L.pt_begin(ctx.handle, C.byref(flat.c), C.byref(pc)))
            try:
                for want in (1, 2, 3):
                    capi.check(L.pt_step(ctx.handle, 1, C.byref(done)))
                    assert done.value == want
                capi.check(L.pt_read(ctx.handle, img.ctypes.data_as(C.c_void_p), w * 4, acc.ctypes.data_as(C.c_void_p)))
            finally:
                st = capi.PtStats()
                capi.check(L.pt_end(ctx.handle, C.byref(st)))
            frames.append((img, acc, st.segments, st.draws))
        finally:
            ctx.set_primary_rays(None)
    for img, acc, seg, draws in frames:
        assert np.array_equal(img, plain[0]) and acc.tobytes() == plain[1].tobytes()
        assert (seg, draws) == (plain[4]["segments"], plain[4]["draws"])


def test_the_mismatch_counter_moves_when_candidates_are_dropped(oracle):
    """Negative control: with the first eight candidate bits of every group cleared (PTCORE_DEBUG_DROP, read when the scene is
    prepared), the culled scan of the incoherent class loses real hits and the checker must say so; the same run without the knob
    counts nothing."""
    _, sc = _scene("bitmask")
    rays = S.classes()["incoherent"]
    deltas = {}
    for drop in ("0xff", None):
        ctx = _context_with({"PTCORE_SCAN": "verify"})
        old = os.environ.get("PTCORE_DEBUG_DROP")
        try:
            if drop is None:
                os.environ.pop("PTCORE_DEBUG_DROP", None)
            else:
                os.environ["PTCORE_DEBUG_DROP"] = drop
            before = _mismatches(ctx)
            S.render_injected(ctx, sc, rays, stats=False)
            deltas[drop] = _mismatches(ctx) - before
        finally:
            if old is None:
                os.environ.pop("PTCORE_DEBUG_DROP", None)
            else:
                os.environ["PTCORE_DEBUG_DROP"] = old
            ctx.close()
    print("injected rays: negative control, scan-mismatch deltas with / without PTCORE_DEBUG_DROP=0xff: %d / %d" % (deltas["0xff"], deltas[None]))
    assert deltas["0xff"] > 0 and deltas[None] == 0, deltas


def test_refusals_leave_the_context_usable(contexts, oracle):
    """A table of the wrong size, fog on and GL shading on: each returns its status without launching anything, and the next frame
    on the same context is right."""
    from path_trace_golang_amd import capi, hip, scene as scn

    L = capi.load()
    doc, sc = _scene("bitmask")
    ctx = contexts["default"]
    rays = S.classes()["incoherent"]
    o = _oracle(oracle, "bitmask", "incoherent")
    flat = hip.FlatScene(sc)
    img = np.zeros((S.H, S.W, 4), np.uint8)

    def frame(w=S.W, h=S.H, spp=1):
        pc = hip.pt_config(hip.RenderConfig(w, h, spp, S.DEPTH, S.SEED, 0, 0))
        return L.pt_render(ctx.handle, C.byref(flat.c), C.byref(pc), img.ctypes.data_as(C.c_void_p), S.W * 4, None, None, None, None)

    def still_right():
        S.injected_vs_oracle(ctx, sc, o, rays, tag="after a refusal", forms=("shipping",))

    try:
        hip.set_fog(ctx, None)
        hip.set_shading(ctx, "cpu")
        # the wrong n: one ray short, one sample too many, a smaller frame
        ctx.set_primary_rays(rays[:-1])
        assert frame() == capi.PT_ERR_INVALID and b"4095 rays" in L.pt_last_error() and b"4096" in L.pt_last_error()
        ctx.set_primary_rays(rays)
        assert frame(spp=2) == capi.PT_ERR_INVALID and frame(w=32) == capi.PT_ERR_INVALID
        assert frame() == capi.PT_OK and np.array_equal(img, o["rgba"])
        still_right()
        # fog on
        ctx.set_primary_rays(rays)
        fog = scn.Fog()
        hip.set_fog(ctx, fog)
        assert frame() == capi.PT_ERR_STATE and b"fog" in L.pt_last_error()
        hip.set_fog(ctx, None)
        assert frame() == capi.PT_OK and np.array_equal(img, o["rgba"])
        still_right()
        # GL shading on
        ctx.set_primary_rays(rays)
        hip.set_shading(ctx, "gl", sc)
        assert frame() == capi.PT_ERR_STATE and b"GL shading" in L.pt_last_error()
        hip.set_shading(ctx, "cpu")
        assert frame() == capi.PT_OK and np.array_equal(img, o["rgba"])
        still_right()
        # while a frame is open the table cannot change
        pc = hip.pt_config(hip.RenderConfig(S.W, S.H, 1, S.DEPTH, S.SEED, 0, 0))
        ctx.set_primary_rays(rays)
        capi.check(L.pt_begin(ctx.handle, C.byref(flat.c), C.byref(pc)))
        assert L.pt_debug_set_primary_rays(ctx.handle, None, 0) == capi.PT_ERR_STATE
        capi.check(L.pt_end(ctx.handle, None))
    finally:
        hip.set_fog(ctx, None)
        hip.set_shading(ctx, "cpu")
        ctx.set_primary_rays(None)
    # several devices in the context (the one GPU twice): refused too
    with capi.Context(devices=[0, 0]) as two:
        two.set_primary_rays(rays)
        pc = hip.pt_config(hip.RenderConfig(S.W, S.H, 1, S.DEPTH, S.SEED, 0, 0))
        assert L.pt_render(two.handle, C.byref(flat.c), C.byref(pc), img.ctypes.data_as(C.c_void_p), S.W * 4, None, None, None, None) == capi.PT_ERR_STATE
        two.set_primary_rays(None)
        assert L.pt_render(two.handle, C.byref(flat.c), C.byref(pc), img.ctypes.data_as(C.c_void_p), S.W * 4, None, None, None, None) == capi.PT_OK
    plain = S.render_injected(ctx, sc, None, stats=False)
    assert np.array_equal(img, plain[0])
