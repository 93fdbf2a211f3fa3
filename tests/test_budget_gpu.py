"""Job-buffer budget (PTCORE_L_BUDGET_MB, DESIGN 8 "Passes per frame"): the samples per pass follow from it, the frame does not
(ordered accumulation); a device that cannot give the budget halves the pass until the buffers fit and keeps that size for the
frames that follow instead of trying the full budget again on every frame.  The per-pass memory plan behind it (pass_plan in
csrc/ptcore.hip: what a job and a queue entry cost in each form of the loop) is pinned through pt_stats.spp_chunk."""
import numpy as np
import pytest

from conftest import scene_path

pytestmark = pytest.mark.gpu


def _frames(monkeypatch, budget_mb, name, w, h, spp, depth, seed, n=1):
    from path_trace_golang_amd import capi, hip, scene

    if budget_mb is None:
        monkeypatch.delenv("PTCORE_L_BUDGET_MB", raising=False)
    else:
        monkeypatch.setenv("PTCORE_L_BUDGET_MB", str(budget_mb))
    sc = hip.FlatScene(scene.load(scene_path(name)))
    out = []
    with capi.Context(ndev=1) as ctx:  # the budget is read by pt_create
        for _ in range(n):
            img = np.zeros((h, w, 4), np.uint8)
            acc = np.zeros((h, w, 3))
            st = hip.render(sc, hip.RenderConfig(w, h, spp, depth, seed), img, None, acc, ctx=ctx)
            out.append((st, img, acc))
    return out


def test_the_frame_does_not_depend_on_the_budget(monkeypatch):
    name, w, h, spp, depth = "test_scene", 320, 180, 48, 8
    (st_a, img_a, acc_a), = _frames(monkeypatch, None, name, w, h, spp, depth, 5)
    (st_b, img_b, acc_b), = _frames(monkeypatch, 64, name, w, h, spp, depth, 5)
    assert st_a["spp_chunk"] == spp and 1 <= st_b["spp_chunk"] <= 4  # 64 MiB hold about three samples of every pixel slot
    assert st_b["trace_launches"] > st_a["trace_launches"]
    assert st_a["segments"] == st_b["segments"] and st_a["draws"] == st_b["draws"]
    assert np.array_equal(img_a, img_b)
    assert np.array_equal(acc_a, acc_b)  # same additions in the same order, whatever the pass size


def test_a_budget_beyond_the_device_halves_the_pass_once(monkeypatch, capfd):
    # 3840x2160: 8.36 M pixel slots x 128 spp x 310 B of job buffers (rays, radiance, two path-state queues) = 331 GB, more than
    # the 288 GB of an MI355X; half of it fits (a quarter, an eighth ... on a device that someone else is using too)
    from path_trace_golang_amd import capi, hip, scene

    name, w, h, spp, depth = "gpu_showcase", 3840, 2160, 128, 8
    monkeypatch.setenv("PTCORE_VERBOSE", "1")
    monkeypatch.setenv("PTCORE_L_BUDGET_MB", "400000")
    sc = hip.FlatScene(scene.load(scene_path(name)))
    big = []
    with capi.Context(ndev=1) as ctx:
        for frame in range(2):
            capfd.readouterr()
            img = np.zeros((h, w, 4), np.uint8)
            acc = np.zeros((h, w, 3))
            st = hip.render(sc, hip.RenderConfig(w, h, spp, depth, 3), img, None, acc, ctx=ctx)
            halvings = capfd.readouterr().err.count("short of memory")
            if frame == 0:
                assert halvings >= 1 and st["spp_chunk"] == spp >> halvings
            else:
                assert halvings == 0 and st["spp_chunk"] == big[0][0]["spp_chunk"]  # starts from the size that fitted
            big.append((st, img, acc))
    monkeypatch.delenv("PTCORE_VERBOSE")
    (st_ref, img_ref, acc_ref), = _frames(monkeypatch, None, name, w, h, spp, depth, 3)
    for st, img, acc in big:
        assert st["segments"] == st_ref["segments"]
        assert np.array_equal(img, img_ref)
        assert np.array_equal(acc, acc_ref)


def test_a_context_grows_its_job_buffers_on_the_second_frame_of_one_shape(monkeypatch):
    """pt_render with library defaults (what a Go host calls once per frame, gpu.go:2534-2546): the first frame of a shape is cut
    into the passes 48 GiB of job buffers allow, the second frame of the SAME shape takes the 160 GiB size by itself when the device
    has it free -- fewer passes, the same pixels; another shape starts small again; PTCORE_AUTO_GROW=0 or an explicit
    PTCORE_L_BUDGET_MB keep the size fixed."""
    from conftest import scene_path
    from path_trace_golang_amd import capi, hip, scene

    sc = scene.load(scene_path("test_scene"))
    w, h, spp, depth = 1920, 1080, 320, 1  # 2.07 M pixel slots x 320 spp x 310 B = 206 GB of job buffers for one pass
    monkeypatch.delenv("PTCORE_L_BUDGET_MB", raising=False)
    monkeypatch.delenv("PTCORE_AUTO_GROW", raising=False)
    frames = []
    with capi.Context(ndev=1) as ctx:
        for _ in range(3):
            img = np.zeros((h, w, 4), np.uint8)
            st = hip.render(sc, hip.RenderConfig(w, h, spp, depth, 4), img, ctx=ctx)
            frames.append((img, st["spp_chunk"], st["segments"]))
        small = np.zeros((90, 160, 4), np.uint8)
        hip.render(sc, hip.RenderConfig(160, 90, 8, depth, 4), small, ctx=ctx)  # another shape in between
        img = np.zeros((h, w, 4), np.uint8)
        st = hip.render(sc, hip.RenderConfig(w, h, spp, depth, 4), img, ctx=ctx)
        frames.append((img, st["spp_chunk"], st["segments"]))
    assert frames[0][1] < spp  # the first frame needed several passes
    for f in frames[1:]:
        assert np.array_equal(f[0], frames[0][0]) and f[2] == frames[0][2]  # pixels do not depend on the chunking
    if frames[1][1] == frames[0][1]:
        pytest.skip("the device does not have 160 GiB + a tenth free right now (other contexts of this session hold them): no growth to look at")
    assert frames[1][1] > frames[0][1] and frames[2][1] == frames[1][1]  # the second and third took the grown size (this box has the room)
    assert frames[3][1] == frames[0][1]  # first frame of the shape again (the small one came in between): the small size
    for f in frames[1:]:
        assert np.array_equal(f[0], frames[0][0]) and f[2] == frames[0][2]  # pixels do not depend on the chunking
    monkeypatch.setenv("PTCORE_AUTO_GROW", "0")
    with capi.Context(ndev=1) as ctx:
        chunks = []
        for _ in range(2):
            img = np.zeros((h, w, 4), np.uint8)
            chunks.append(hip.render(sc, hip.RenderConfig(w, h, spp, depth, 4), img, ctx=ctx)["spp_chunk"])
        assert chunks[0] == chunks[1] == frames[0][1] and np.array_equal(img, frames[0][0])


# ---------------------------------------------------------------- the per-pass memory plan, through spp_chunk
#
# 70 x 45 frames: 3 x 2 tiles with both edges ragged, 6144 pixel slots.  What a sample of a pass costs (dev_begin):
#   90 B per job, 98 B with pixel stats; 104 B per queue entry (80 + 8 + 4 x 4 planes), 112 B with pixel stats (6 planes);
#   a queue holds one entry per job + the window slack of queue_slack(): 24 blocks x 4 waves x 1024 slots per writer pass
#   and sample here, where num_cu x blocks per CU >= 240 (an MI355X has 256 CUs).
# The expected samples per pass follow frame_open's first guess, dev_begin's shrink loop and balance_chunk by hand:
#   no queues        4 MiB / (6144 x 90 B) = 7.6 -> 7; with stats 7 x 6144 x 98 B is over 4 MiB, 6 fit, 20 spp in 4 passes -> 5
#   split, 2 queues  6144 x 90 + 2 x 104448 x 104 = 22 278 144 B per sample: 3 fit in 80 MiB, 4 (89 112 576 B) do not;
#                    with stats 6144 x 98 + 2 x 104448 x 112 = 23 998 464 B: 3 again
#   primary pass, 1  552 960 + 104448 x 104 = 11 415 552 B per sample: 3 fit in 40 MiB
#   wavefront, 3     two writer passes, twice the slack: 552 960 + 3 x 202752 x 104 = 63 811 584 B per sample: 3 fit in 200 MiB
_W, _H = 70, 45
PLAN_CASES = {  # name: (scene, environment, budget MiB, spp, depth, pixel stats, spp_chunk, trace_launches or None, has queues)
    "no_queues": ("example_simple", {"PTCORE_SPLIT_ROUNDS": "0"}, 4, 20, 4, False, 7, 3, False),
    "no_queues_stats": ("example_simple", {"PTCORE_SPLIT_ROUNDS": "0"}, 4, 20, 4, True, 5, 4, False),
    "split": ("gpu_showcase", {}, 80, 10, 8, False, 3, None, True),
    "split_stats": ("gpu_showcase", {}, 80, 10, 8, True, 3, None, True),
    # the same two, the budget a MiB either side of three samples (66 834 432 B = 63.7 MiB; with stats 71 995 392 B = 68.7 MiB):
    # a queue entry priced one 4-byte plane higher or lower (626 688 entries in a pass of three samples) moves one of each pair
    "split_64": ("gpu_showcase", {}, 64, 10, 8, False, 3, None, True),
    "split_63": ("gpu_showcase", {}, 63, 10, 8, False, 2, None, True),
    "split_stats_69": ("gpu_showcase", {}, 69, 10, 8, True, 3, None, True),
    "split_stats_68": ("gpu_showcase", {}, 68, 10, 8, True, 2, None, True),
    "primary": ("synth_300_6", {}, 40, 10, 8, False, 3, None, True),
    "wavefront": ("gpu_showcase", {"PTCORE_PIPELINE": "wavefront"}, 200, 10, 8, False, 3, None, True),
}
_reference = {}  # (scene, environment, spp, depth) -> the frame under the default budget, rendered once


def _small_frame(monkeypatch, name, env, budget_mb, spp, depth, stats):
    from path_trace_golang_amd import capi, hip, scene, synth

    for k in ("PTCORE_SPLIT_ROUNDS", "PTCORE_PIPELINE", "PTCORE_L_BUDGET_MB"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if budget_mb is not None:
        monkeypatch.setenv("PTCORE_L_BUDGET_MB", str(budget_mb))
    sc = hip.FlatScene(synth.make_scene(300, 6) if name == "synth_300_6" else scene.load(scene_path(name)))
    img = np.zeros((_H, _W, 4), np.uint8)
    acc = np.zeros((_H, _W, 3))
    nseg, ndraw = (np.zeros((_H, _W), np.uint32), np.zeros((_H, _W), np.uint32)) if stats else (None, None)
    with capi.Context(ndev=1) as ctx:  # the budget is read by pt_create
        st = hip.render(sc, hip.RenderConfig(_W, _H, spp, depth, 7, 0, capi.PT_FLAG_PIXEL_STATS if stats else 0), img, None, acc, nseg,
                        ndraw, ctx=ctx)
    return st, img, acc


@pytest.mark.parametrize("case", list(PLAN_CASES))
def test_the_samples_per_pass_follow_the_memory_plan(monkeypatch, case):
    import torch

    name, env, budget_mb, spp, depth, stats, chunk, launches, queues = PLAN_CASES[case]
    if queues:  # the window slack is 24 blocks per sample only with that many writer blocks on the device
        assert torch.cuda.get_device_properties(0).multi_processor_count >= 240
    key = (name, tuple(sorted(env.items())), spp, depth)
    if key not in _reference:
        _reference[key] = _small_frame(monkeypatch, name, env, None, spp, depth, False)
    st_ref, img_ref, acc_ref = _reference[key]
    st, img, acc = _small_frame(monkeypatch, name, env, budget_mb, spp, depth, stats)
    print(case, "spp_chunk", st["spp_chunk"], "trace_launches", st["trace_launches"], "default budget:", st_ref["spp_chunk"])
    assert st_ref["spp_chunk"] == spp
    assert st["spp_chunk"] == chunk
    if launches is not None:
        assert st["trace_launches"] == launches
    for k in ("samples", "segments", "exit_scans", "draws"):
        assert st[k] == st_ref[k], k
    assert np.array_equal(img, img_ref)
    assert np.array_equal(acc, acc_ref, equal_nan=True)  # same additions in the same order, whatever the pass size
