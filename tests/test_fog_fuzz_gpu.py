"""Fog on the MI355X on random scenes, through the public entry points, on every form of the trace loop.

fog_kernel reads a job's primary ray back from the ray-generation buffers after the chunk's last trace pass and relies on no
trace form writing them (pt_kernels.h).  A form that reused or permuted those buffers would change fogged frames only, so
every scene here is rendered with its fog block on a matrix of contexts -- the three flat scans, the wavefront form with
and without ray binning, the unsplit loop, the trip tail, one block per CU -- and, for thin-lens cameras, under every ray
generation, in both kernel builds, and held to the independent restatement tests/fog_reference.c and to each other.  The
scenes are the generator's (fuzz_support.py): overlapping, nested, coincident geometry, missing material ids, up to 128
spheres and 128 boxes (the grouped scan; nothing lands on the BVH path), 0 / 1 / 8 / 9 / 12 lights, random fog blocks.
Every test uses contexts of its own, so the shared session context never carries a fog block."""
from __future__ import annotations

import os
import time

import numpy as np
import pytest

import fog_support as fs
from fuzz_support import LIGHT_COUNTS, count_kinds, random_doc, random_fog_block, set_lights, trim_to_limits

pytestmark = pytest.mark.gpu

SEEDS = 24
FRAMES = ((33, 20), (50, 33), (20, 33))
SPP_CHUNK = ((1, 2), (3, 2), (5, 3), (5, 2))  # a chunk that does not divide the sample count
DEPTHS = (1, 7, 12)
CONTEXT_ENV = {
    "default": {},
    "broad": {"PTCORE_SCAN": "broad"},
    "wide": {"PTCORE_SCAN": "wide"},
    "uniform": {"PTCORE_SCAN": "uniform"},
    "wavefront": {"PTCORE_PIPELINE": "wavefront", "PTCORE_WF_SORT": "0"},
    "wavefront/sort": {"PTCORE_PIPELINE": "wavefront", "PTCORE_WF_SORT": "1"},
    "split_rounds_0": {"PTCORE_SPLIT_ROUNDS": "0"},
    "tail_trip": {"PTCORE_TAIL": "trip"},
    "blocks_per_cu_1": {"PTCORE_BLOCKS_PER_CU": "1"},
}
ENV_KEYS = sorted({k for e in CONTEXT_ENV.values() for k in e})
DROPPED = {"scenes": 0, "dropped": 0}  # nothing is dropped today; a later reason to drop a scene has to count itself here


@pytest.fixture(autouse=True, scope="module")
def _torch_before_libptcore():
    import torch  # noqa: F401  (one HIP runtime in the process, as in test_fog_gpu.py)


@pytest.fixture(scope="module")
def contexts():
    from path_trace_golang_amd import capi

    out = {}
    old = {k: os.environ.get(k) for k in ENV_KEYS}
    try:
        for name, env in CONTEXT_ENV.items():
            for k in ENV_KEYS:  # read at pt_create
                if k in env:
                    os.environ[k] = env[k]
                else:
                    os.environ.pop(k, None)
            out[name] = capi.Context(ndev=1)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    yield out
    for c in out.values():
        c.close()


def fog_fuzz_case(seed: int) -> dict:
    """Scene, fog block and render configuration of a seed.  seed % 4 picks the size band: 1-32 objects, 33-64, 70-150 (more
    than 32 of a kind: the grouped scan), and 100-260 cut to the limits of 128 spheres and 128 boxes."""
    rng = np.random.default_rng([77, int(seed)])
    band = seed % 4
    nobj = int(rng.integers(1, 33)) if band == 0 else int(rng.integers(33, 65)) if band == 1 else \
        int(rng.integers(70, 151)) if band == 2 else (260 if seed % 8 == 3 else int(rng.integers(100, 261)))
    doc = random_doc(rng, nobj)
    doc["fog"] = random_fog_block(rng)
    if seed % 3 != 2:
        doc["fog"]["gpu_volumetric"] = True
        if doc["fog"]["density"] == 0.0 and "sigma_s" not in doc["fog"]:
            doc["fog"]["density"] = 0.05
    if seed % 5 == 1:
        doc["camera"]["aperture"] = 0.2  # thin lens: the column and simple ray generations are rendered too
    lights = LIGHT_COUNTS[(seed // 2) % len(LIGHT_COUNTS)]
    if lights is not None:
        set_lights(doc, lights, "sphere_light" if seed % 2 else "sphere", seed=seed)
    trim_to_limits(doc)
    w, h = FRAMES[seed % len(FRAMES)]
    spp, chunk = SPP_CHUNK[(seed // 3) % len(SPP_CHUNK)]
    return {"doc": doc, "w": w, "h": h, "spp": spp, "chunk": chunk, "depth": DEPTHS[(seed // 2) % len(DEPTHS)], "seed": seed + 1}


def _render(ctx, sc, case, fog, flags=0):
    from path_trace_golang_amd import hip

    w, h = case["w"], case["h"]
    img = np.zeros((h, w, 4), np.uint8)
    acc = np.zeros((h, w, 3))
    st = hip.render(sc, hip.RenderConfig(w, h, case["spp"], case["depth"], case["seed"], case["chunk"], flags), img, None, acc,
                    ctx=ctx, fog=fog)
    return img, acc, st, hip.fog_last_stats(ctx)


def _check_render(tag, got, ref, off_st, depth):
    """What test_fog_parity_with_reference asserts of one fogged render, the radiance sums in the form of
    conftest.render_vs_oracle (NaN where the reference has NaN)."""
    img, acc, st, fst = got
    ref_img, ref_acc, ref_st = ref
    assert np.array_equal(img, ref_img), (tag, int(np.count_nonzero(img != ref_img)))
    ok = (np.isnan(acc) & np.isnan(ref_acc)) | (np.abs(acc - ref_acc) <= 4 * max(depth, 1) * 2.0 ** -52 * np.maximum(np.abs(ref_acc), 1e-300))
    assert np.all(ok), (tag, int(np.count_nonzero(~ok)))
    assert (st["segments"], st["draws"]) == (off_st["segments"], off_st["draws"]) == (ref_st["segments"], ref_st["draws"]), tag
    assert (fst["shadow_rays"], fst["draws"], fst["steps"]) == (ref_st["shadow_rays"], ref_st["fog_draws"], ref_st["steps"]), tag


def _one_scene(contexts, case, monkeypatch):
    """Renders the case on every context (and ray generation), both builds; returns (reference stats, renders compared)."""
    from oracle import ora
    from path_trace_golang_amd import capi, scene

    doc = case["doc"]
    sc, oc = scene.Scene.decode(doc), ora.Scene(doc)
    fog = fs.fog_of_scene(doc["fog"])
    ref = fs.reference_render(oc, case["w"], case["h"], case["spp"], case["depth"], case["seed"], fog)
    DROPPED["scenes"] += 1
    _, _, off_st, off_fog = _render(contexts["default"], sc, case, False)
    assert off_fog["fog_launches"] == 0
    lens = doc["camera"].get("aperture", 0) > 0
    first = None
    renders = 0
    for name, ctx in contexts.items():
        for raygen in ((None, "column", "simple") if lens else (None,)):
            if raygen is None:
                monkeypatch.delenv("PTCORE_RAYGEN", raising=False)
            else:
                monkeypatch.setenv("PTCORE_RAYGEN", raygen)  # read at render time
            for flags in (capi.PT_FLAG_PIXEL_STATS, 0):
                tag = (case["seed"], name, raygen, flags)
                got = _render(ctx, sc, case, True, flags)
                _check_render(tag, got, ref, off_st, case["depth"])
                if ref[2]["steps"] > 0:
                    assert got[3]["fog_launches"] >= 1, tag
                if first is None:
                    first = got
                assert np.array_equal(got[0], first[0]) and np.array_equal(got[1].view(np.uint64), first[1].view(np.uint64)), \
                    (tag, "differs from the first context")
                renders += 1
    monkeypatch.delenv("PTCORE_RAYGEN", raising=False)
    return ref[2], renders


def test_the_chosen_scenes_reach_what_they_are_for():
    grouped = lens = at_limit = volumetric = 0
    sizes, lights, spps, depths, frames = set(), set(), set(), set(), set()
    for seed in range(SEEDS):
        case = fog_fuzz_case(seed)
        ns, nb, _ = count_kinds(case["doc"])
        assert ns <= 128 and nb <= 128  # nothing on the BVH path
        grouped += ns > 32 or nb > 32
        at_limit += ns >= 120 or nb >= 120
        lens += case["doc"]["camera"]["aperture"] > 0
        volumetric += bool(case["doc"]["fog"]["gpu_volumetric"])
        sizes.add(len(case["doc"]["objects"]))
        lights.add(LIGHT_COUNTS[(seed // 2) % len(LIGHT_COUNTS)])
        spps.add(case["spp"]); depths.add(case["depth"]); frames.add((case["w"], case["h"]))
        assert case["spp"] % case["chunk"] != 0
    assert SEEDS >= 24 and grouped * 4 >= SEEDS and at_limit >= 2 and lens >= 3 and volumetric * 3 >= SEEDS * 2
    assert min(sizes) <= 32 and any(33 <= s <= 128 for s in sizes) and max(sizes) > 200
    assert {0, 1, 8, 9, 12, None} <= lights and spps == {1, 3, 5} and depths == {1, 7, 12} and len(frames) == 3


@pytest.mark.parametrize("seed", range(SEEDS))
def test_random_scenes_with_fog_on_every_form_of_the_loop(contexts, monkeypatch, seed):
    st, renders = _one_scene(contexts, fog_fuzz_case(seed), monkeypatch)
    print("fog fuzz seed %d: %d renders on %d contexts equal the restatement (%d fog steps, %d shadow rays)"
          % (seed, renders, len(contexts), st["steps"], st["shadow_rays"]))


def test_the_fuzz_is_not_over_zeros_and_drops_nothing():
    # the reference side only (cheap): most scenes march, many cast shadow rays
    from oracle import ora

    marched = shadowed = 0
    for seed in range(SEEDS):
        case = fog_fuzz_case(seed)
        fog = fs.fog_of_scene(case["doc"]["fog"])
        _, _, st = fs.reference_render(ora.Scene(case["doc"]), case["w"], case["h"], 1, case["depth"], case["seed"], fog)
        marched += st["steps"] > 0
        shadowed += st["shadow_rays"] > 0
    assert marched * 3 >= SEEDS * 2 and shadowed * 3 >= SEEDS, (marched, shadowed)
    assert DROPPED["dropped"] * 20 <= max(DROPPED["scenes"], 1)  # the cap on dropped scenes (none is dropped today)


@pytest.mark.parametrize("name", ["default", "wavefront"])
def test_a_scene_above_the_limits_is_refused_and_the_context_goes_on(contexts, monkeypatch, name):
    from path_trace_golang_amd import capi, scene

    rng = np.random.default_rng(4242)
    doc = random_doc(rng, 330)
    doc["fog"] = random_fog_block(rng)
    doc["fog"].update(gpu_volumetric=True, density=0.05)
    assert count_kinds(doc)[0] > 128
    big = {"doc": doc, "w": 33, "h": 20, "spp": 1, "chunk": 0, "depth": 3, "seed": 9}
    ctx = contexts[name]
    with pytest.raises(capi.PtError) as e:
        _render(ctx, scene.Scene.decode(doc), big, True)
    assert e.value.code == capi.PT_ERR_INVALID and "BVH" in str(e.value)
    # the same context renders the next scene correctly
    case = fog_fuzz_case(6)
    single = {name: ctx, "default": contexts["default"]}
    st, renders = _one_scene(single, case, monkeypatch)
    assert renders >= 2 and st["steps"] > 0


@pytest.mark.skipif(not os.environ.get("PT_SOAK_SECONDS"), reason="long run: PT_SOAK_SECONDS=<seconds> [PT_SOAK_SEED=<n>]")
def test_random_fog_scenes_soak(contexts, monkeypatch):
    t0, budget = time.time(), float(os.environ["PT_SOAK_SECONDS"])
    seed = int(os.environ.get("PT_SOAK_SEED", "70001"))
    scenes = renders = steps = 0
    while time.time() - t0 < budget:
        st, n = _one_scene(contexts, fog_fuzz_case(seed + scenes), monkeypatch)
        scenes, renders, steps = scenes + 1, renders + n, steps + st["steps"]
        if scenes % 50 == 0:
            print("fog soak: %d scenes, %.0f s" % (scenes, time.time() - t0), flush=True)  # a silent GPU job is taken to be hung
    assert DROPPED["dropped"] * 20 <= max(DROPPED["scenes"], 1)
    print("fog soak: %d random scenes x %d contexts, %d renders, %d reference march steps, %d dropped, %.0f s, all equal"
          % (scenes, len(contexts), renders, steps, DROPPED["dropped"], time.time() - t0), flush=True)
