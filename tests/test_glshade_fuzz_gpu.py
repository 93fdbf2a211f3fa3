"""GL shading on the MI355X on random scenes, through the public entry points: whole frames against the independent
restatement tests/glshade_reference.c on what the generator (fuzz_support.py) exists to produce and test_glshade_gpu.py
never sees -- overlapping, nested, coincident and half-grid geometry, missing material ids, scenes above 32 objects (up to
128 spheres and 128 boxes), 0 / 1 / 8 / 9 / 12 lights around the 8-light subset rule, random GL material extras -- half of
them with a random fog block, on a default context and one with a single block per CU.  Every test uses contexts of its
own, so the shared session context never carries a shading model."""
from __future__ import annotations

import os
import time

import numpy as np
import pytest

import glshade_support as gs
from fuzz_support import LIGHT_COUNTS, count_kinds, random_doc, random_fog_block, random_gl_extras, set_lights, trim_to_limits

pytestmark = pytest.mark.gpu

SEEDS = 24
FRAMES = ((33, 20), (20, 33), (40, 17))
PASSES_CHUNK = ((1, 0), (2, 1), (3, 2), (3, 1))
DEPTHS = (1, 6, 12)
DEEP_SEED, NO_MATERIALS_SEED, NO_LIGHTS_SEED = 5, 9, 2
DROPPED = {"scenes": 0, "dropped": 0}  # nothing is dropped today; a later reason to drop a scene has to count itself here


@pytest.fixture(autouse=True, scope="module")
def _torch_before_libptcore():
    import torch  # noqa: F401  (one HIP runtime in the process, as in test_glshade_gpu.py)


@pytest.fixture(scope="module")
def contexts():
    from path_trace_golang_amd import capi

    out = {}
    old = os.environ.get("PTCORE_BLOCKS_PER_CU")
    try:
        os.environ.pop("PTCORE_BLOCKS_PER_CU", None)
        out["default"] = capi.Context(ndev=1)
        os.environ["PTCORE_BLOCKS_PER_CU"] = "1"  # read at pt_create
        out["blocks_per_cu_1"] = capi.Context(ndev=1)
    finally:
        if old is None:
            os.environ.pop("PTCORE_BLOCKS_PER_CU", None)
        else:
            os.environ["PTCORE_BLOCKS_PER_CU"] = old
    yield out
    for c in out.values():
        c.close()


def gl_fuzz_case(seed: int) -> dict:
    """Scene with GL extras and a fog block, and the render configuration of a seed.  seed % 3 picks the size band: 1-32
    objects, 33-128, and 129-260 cut to the limits of 128 spheres and 128 boxes."""
    rng = np.random.default_rng([88, int(seed)])
    band = seed % 3
    nobj = int(rng.integers(1, 33)) if band == 0 else int(rng.integers(33, 129)) if band == 1 else int(rng.integers(129, 261))
    doc = random_doc(rng, nobj)
    doc["fog"] = random_fog_block(rng)
    random_gl_extras(doc, rng)
    lights = 0 if seed == NO_LIGHTS_SEED else LIGHT_COUNTS[(seed // 3) % len(LIGHT_COUNTS)]
    if lights is not None:
        set_lights(doc, lights, "sphere_light" if seed % 2 else "sphere", seed=seed)
    if seed == NO_MATERIALS_SEED:
        doc["materials"] = []  # every object then falls to the zero material
    trim_to_limits(doc)
    fog = seed % 2 == 0
    if fog:  # the fog block is rendered: make it one that marches
        doc["fog"]["gpu_volumetric"] = True
        if doc["fog"]["density"] == 0.0:
            doc["fog"]["density"] = 0.05
        if doc["fog"].get("sigma_s", 0.0) < 0 < doc["fog"].get("sigma_a", 0.0):
            doc["fog"]["sigma_a"] = -doc["fog"]["sigma_a"]  # absorbing only would not march: both negative falls back to the density
    w, h = FRAMES[seed % len(FRAMES)]
    passes, chunk = PASSES_CHUNK[(seed // 2) % len(PASSES_CHUNK)]
    depth = 80 if seed == DEEP_SEED else DEPTHS[(seed // 2) % len(DEPTHS)]
    return {"doc": doc, "w": w, "h": h, "passes": passes, "chunk": chunk, "depth": depth, "seed": 100 + seed, "fog": fog}


def _one_scene(contexts, case):
    """What _check of test_glshade_gpu.py asserts, on every context; returns the reference counters."""
    from oracle import ora
    from path_trace_golang_amd import hip, scene

    doc = case["doc"]
    sc, o = scene.Scene.decode(doc), ora.Scene(doc)
    w, h, passes, depth, fog = case["w"], case["h"], case["passes"], case["depth"], case["fog"]
    ref_img, ref_acc, ref_st = gs.reference_render(o, gs.extras(sc), w, h, passes, depth, case["seed"], hip.pt_fog(sc.fog) if fog else None)
    DROPPED["scenes"] += 1
    first = None
    for name, ctx in contexts.items():
        tag = (case["seed"], name)
        img = np.zeros((h, w, 4), np.uint8)
        acc = np.zeros((h, w, 3))
        st = hip.render(sc, hip.RenderConfig(w, h, passes, depth, case["seed"], case["chunk"], 0), img, None, acc, ctx=ctx, fog=fog,
                        shading="gl")
        gst, fst = hip.shading_last_stats(ctx), hip.fog_last_stats(ctx)
        assert np.array_equal(img, ref_img), (tag, int(np.count_nonzero(img != ref_img)))
        ok = (np.isnan(acc) & np.isnan(ref_acc)) | (np.abs(acc - ref_acc) <= 4 * max(depth, 1) * 2.0 ** -52 * np.maximum(np.abs(ref_acc), 1e-300))
        assert np.all(ok), (tag, int(np.count_nonzero(~ok)))
        assert (gst["paths"], gst["segments"], gst["shadow_rays"], gst["probe_rays"], gst["draws"]) == \
            (ref_st["paths"], ref_st["segments"], ref_st["shadow_rays"], ref_st["probe_rays"], ref_st["draws"]), tag
        assert (st["samples"], st["segments"], st["draws"]) == (ref_st["paths"], ref_st["segments"], ref_st["draws"]), tag
        assert gst["gl_launches"] >= 1 and gst["gl_ms"] > 0 and st["trace_ms"] == pytest.approx(gst["gl_ms"]), tag
        if fog:
            assert (fst["shadow_rays"], fst["draws"], fst["steps"]) == \
                (ref_st["fog_shadow_rays"], ref_st["fog_draws"], ref_st["fog_steps"]), tag
        if first is None:
            first = (img, acc)
        assert np.array_equal(img, first[0]) and np.array_equal(acc.view(np.uint64), first[1].view(np.uint64)), (tag, "contexts differ")
    return ref_st


def test_the_chosen_scenes_reach_what_they_are_for():
    from path_trace_golang_amd import scene

    above32 = with_fog = missing = 0
    lights, depths, passes, sizes = set(), set(), set(), set()
    for seed in range(SEEDS):
        case = gl_fuzz_case(seed)
        doc = case["doc"]
        ns, nb, _ = count_kinds(doc)
        assert ns <= 128 and nb <= 128  # nothing on the BVH path
        above32 += len(doc["objects"]) > 32
        with_fog += case["fog"]
        ids = {m["id"] for m in doc["materials"]}
        missing += any(o["material_id"] not in ids for o in doc["objects"])
        lights.add(0 if seed == NO_LIGHTS_SEED else LIGHT_COUNTS[(seed // 3) % len(LIGHT_COUNTS)])
        depths.add(case["depth"]); passes.add((case["passes"], case["chunk"])); sizes.add(len(doc["objects"]))
    assert SEEDS >= 24 and with_fog * 2 == SEEDS and above32 * 2 >= SEEDS and missing * 2 >= SEEDS
    assert {0, 1, 8, 9, 12, None} <= lights and {1, 6, 12, 80} <= depths and {p for p, _ in passes} == {1, 2, 3}
    assert min(sizes) <= 32 and max(sizes) > 128
    assert gl_fuzz_case(NO_MATERIALS_SEED)["doc"]["materials"] == [] and gl_fuzz_case(DEEP_SEED)["depth"] == 80
    sc = scene.Scene.decode(gl_fuzz_case(NO_LIGHTS_SEED)["doc"])
    assert not any(m.type == "emissive" for m in sc.materials)


@pytest.mark.parametrize("seed", range(SEEDS))
def test_random_scenes_with_gl_shading(contexts, seed):
    case = gl_fuzz_case(seed)
    st = _one_scene(contexts, case)
    assert st["paths"] == 16 * case["w"] * case["h"] * case["passes"]
    if case["fog"]:
        assert st["fog_steps"] > 0
    print("gl fuzz seed %d: %d objects, depth %d, %d passes%s: %d paths, %d segments, %d shadow rays, %d probe rays on %d contexts"
          % (seed, len(case["doc"]["objects"]), case["depth"], case["passes"], " + fog" if case["fog"] else "", st["paths"],
             st["segments"], st["shadow_rays"], st["probe_rays"], len(contexts)))


def test_the_fuzz_drops_nothing():
    assert DROPPED["dropped"] * 20 <= max(DROPPED["scenes"], 1)  # the cap on dropped scenes (none is dropped today)


@pytest.mark.skipif(not os.environ.get("PT_SOAK_SECONDS"), reason="long run: PT_SOAK_SECONDS=<seconds> [PT_SOAK_SEED=<n>]")
def test_random_gl_scenes_soak(contexts):
    t0, budget = time.time(), float(os.environ["PT_SOAK_SECONDS"])
    seed = int(os.environ.get("PT_SOAK_SEED", "80001"))
    scenes = paths = segs = 0
    while time.time() - t0 < budget:
        st = _one_scene(contexts, gl_fuzz_case(seed + scenes))
        scenes, paths, segs = scenes + 1, paths + st["paths"], segs + st["segments"]
        if scenes % 50 == 0:
            print("gl soak: %d scenes, %.0f s" % (scenes, time.time() - t0), flush=True)  # a silent GPU job is taken to be hung
    assert DROPPED["dropped"] * 20 <= max(DROPPED["scenes"], 1)
    print("gl soak: %d random scenes x %d contexts, %d reference paths, %d segments, %d dropped, %.0f s, all equal"
          % (scenes, len(contexts), paths, segs, DROPPED["dropped"], time.time() - t0), flush=True)
