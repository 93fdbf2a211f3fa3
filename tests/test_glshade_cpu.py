"""GL shading (pt_set_shading, csrc/pt_glshade.h) without a GPU: the host build of pt_glshade.h against the independent
restatement tests/glshade_reference.c (linked to the oracle), bit for bit, per (pixel, pass) over the shipped and
synthetic scenes and several depths; the material resolution; the ABI structs; the Python and C++ host layers."""
from __future__ import annotations

import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import glshade_support as gs
from conftest import ROOT, scene_path
from oracle import ora

SHIPPED = ["example_simple", "gpu_showcase", "metal_glass_room", "test_comprehensive", "test_scene"]
SEED = 20261016


def _jobs(n, w, h, passes, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, w, n), rng.integers(0, h, n), rng.integers(0, passes, n)], 1).astype(np.int32)


def _compare(sc, flat, o, w, h, depth, jobs, fog=None):
    ex = gs.extras(sc)
    a, ca = gs.ref_passes(o, ex, w, h, depth, SEED, jobs, fog)
    b, cb = gs.host_passes(flat, ex, w, h, depth, SEED, jobs, fog)
    bad = np.flatnonzero((a.view(np.uint64) != b.view(np.uint64)).any(1) | (ca != cb).any(1))
    assert bad.size == 0, (jobs[bad[:3]], a[bad[:3]], b[bad[:3]], ca[bad[:3]], cb[bad[:3]])
    return ca.sum(0)


def _shipped(name):
    from path_trace_golang_amd import hip, scene

    p = scene_path(name)
    sc = scene.load(p)
    with open(p) as f:
        return sc, hip.FlatScene(sc), ora.Scene(json.load(f))


@pytest.mark.parametrize("name", SHIPPED)
def test_host_build_equals_restatement_on_the_shipped_scenes(name):
    from path_trace_golang_amd import hip

    sc, flat, o = _shipped(name)
    fog = hip.pt_fog(sc.fog) if sc.fog is not None else None  # the scene's own fog block with GL shading
    n = 0  # jobs: 5 scenes x 15000 (+3000) here and 4 synthetic scenes x 12000 below, 1.26 * 10^5 in all
    for depth, k in ((8, 9000), (3, 3000), (1, 3000)):
        c = _compare(sc, flat, o, 64, 36, depth, _jobs(k, 64, 36, 6, depth), fog)
        n += k
        assert c[0] == 16 * k  # 16 paths per pass
    if name == "gpu_showcase":  # the issue's deep case, plain and with fog
        _compare(sc, flat, o, 64, 36, 80, _jobs(1500, 64, 36, 4, 80), fog)
        _compare(sc, flat, o, 64, 36, 80, _jobs(1500, 64, 36, 4, 81))
        n += 3000
    assert n >= 15000


@pytest.mark.parametrize("name", ["twelve_lights", "edge", "glass", "metal"])
def test_host_build_equals_restatement_on_synthetic_scenes(name, tmp_path):
    sc, flat, o = gs.scene_pair(gs.synthetic_docs()[name], str(tmp_path), name)
    totals = np.zeros(8, np.uint64)
    for depth, k in ((1, 2000), (3, 3000), (8, 5000), (80, 2000)):
        totals += _compare(sc, flat, o, 48, 32, depth, _jobs(k, 48, 32, 5, depth + 7))
    assert totals[1] > totals[0]  # bounces happened
    if name == "twelve_lights":
        assert totals[2] > 0
    if name == "metal":
        assert totals[3] > 0  # rough-metal probes


FUZZ_SCENES, FUZZ_JOBS, FUZZ_W, FUZZ_H, FUZZ_PASSES = 64, 400, 33, 20, 3


def test_host_build_equals_restatement_on_random_scenes(tmp_path):
    """The generator's scenes (fuzz_support.host_fuzz_case: overlapping, nested, coincident geometry, missing material ids,
    1..150 objects, 0 / 1 / 8 / 9 / 12 lights, GL extras), depths 1 / 3 / 7 / 12, half of them with the random fog block:
    the inputs of the GPU fuzz are clean when the host build and the restatement agree on them."""
    from test_fog_cpu import fuzz_scene

    totals = np.zeros(8, np.uint64)
    n = with_fog = nans = 0
    sizes, depths, nlights = set(), set(), set()
    for i in range(FUZZ_SCENES):
        case, sc, flat, o, fog = fuzz_scene(i, tmp_path)
        jobs = _jobs(FUZZ_JOBS, FUZZ_W, FUZZ_H, FUZZ_PASSES, 500 + i)
        ex = gs.extras(sc)
        f = fog if case["fog"] else None
        a, ca = gs.ref_passes(o, ex, FUZZ_W, FUZZ_H, case["depth"], SEED, jobs, f)
        b, cb = gs.host_passes(flat, ex, FUZZ_W, FUZZ_H, case["depth"], SEED, jobs, f)
        bad = np.flatnonzero((a.view(np.uint64) != b.view(np.uint64)).any(1) | (ca != cb).any(1))
        assert bad.size == 0, (i, jobs[bad[:3]], a[bad[:3]], b[bad[:3]], ca[bad[:3]], cb[bad[:3]])
        totals += ca.sum(0)
        n += FUZZ_JOBS
        with_fog += FUZZ_JOBS if case["fog"] else 0
        nans += int(np.count_nonzero(np.isnan(b)))
        sizes.add(case["nobj"])
        depths.add(case["depth"])
        nlights.add(sum(1 for k in range(len(sc.objects)) if _is_gl_light(sc, flat, k)))
    assert FUZZ_SCENES >= 60 and n >= 20_000 and with_fog * 2 == n
    assert min(sizes) == 1 and max(sizes) == 150 and {1, 12} <= depths
    assert nans == 0
    assert totals[0] == 16 * n and totals[1] > totals[0]  # every path, and bounces
    assert totals[2] > n and totals[3] > 0 and totals[4] > 0  # shadow rays, rough-metal probes, draws
    assert totals[5] > 0 and totals[7] > 0  # the fog term's shadow rays and march steps
    assert {0, 1, 8, 9, 12} <= nlights, nlights


def _is_gl_light(sc, flat, k):
    """gl_is_light restated on the flattened scene: the material (index 0 for a missing id) is emissive with some emit > 0."""
    from path_trace_golang_amd import capi

    nmat = len(sc.materials)
    if nmat == 0:
        return False
    mi = flat.objects[k].material
    m = flat.materials[mi if 0 <= mi < nmat else 0]
    return m.type == capi.PT_MAT_EMISSIVE and max(m.emit) > 0


def test_synthetic_scenes_have_the_corners_they_are_for(tmp_path):
    docs = gs.synthetic_docs()
    sc, flat, _ = gs.scene_pair(docs["edge"], str(tmp_path), "edge")
    types = [o.type for o in flat.objects[:len(sc.objects)]]
    mats = [o.material for o in flat.objects[:len(sc.objects)]]
    assert -1 in types and -1 in mats  # an unknown object type and a missing material id
    assert any(m.type == "emissive" and o.type == "box" for o in sc.objects for m in sc.materials if m.id == o.material_id)
    sc12, _, _ = gs.scene_pair(docs["twelve_lights"], str(tmp_path), "twelve")
    assert sum(1 for m in sc12.materials if m.type == "emissive") == 12


def test_material_resolution_table(tmp_path):
    """The host packing (gpu.go:1840-1898) of pt_glshade.h against the restatement, over the corners of its rules."""
    from path_trace_golang_amd import capi

    cases = []
    for typ in range(5):
        for rough, smooth in ((0.0, 0.0), (0.3, 0.0), (0.3, 0.6), (1.4, 0.0), (0.2, -0.5), (0.2, 1.7)):
            for refl in (0.0, 0.4, -1.0, 2.0):
                for tint, asc in (((0, 0, 0), 0.0), ((0.5, 0.2, 0.9), 0.0), ((0, 0, 0), 0.7), ((-1, 0, 0), -0.2)):
                    cases.append((typ, rough, smooth, refl, tint, asc))
    m = capi.PtMaterial()
    x = capi.PtGlMaterial()
    shim, ref = gs.product_host(), gs.reference()
    for typ, rough, smooth, refl, tint, asc in cases:
        m.type, m.rough, m.smoothness, m.ior, m.power = typ, rough, smooth, 1.5, 2.5
        m.albedo[:] = [0.1, 0.2, 0.3]
        m.emit[:] = [1.0, 0.5, 0.0]
        m.absorption[:] = [0.4, 0.5, 0.6]
        x.reflectivity, x.absorption_scale = refl, asc
        x.tint[:] = list(tint)
        a = np.zeros(19)
        b = np.zeros(19)
        shim.shim_material(C.byref(m), C.byref(x), gs.ptr(a))
        ref.gr_material(C.byref(m), C.byref(x), gs.ptr(b))  # ora_material has pt_material's layout
        assert a.view(np.uint64).tolist() == b.view(np.uint64).tolist(), (typ, rough, smooth, refl, tint, asc)
    # spot checks of the rules themselves
    m.type, m.rough, m.smoothness = capi.PT_MAT_METAL, 0.3, 0.0
    x.reflectivity, x.absorption_scale = 0.0, 0.0
    x.tint[:] = [0, 0, 0]
    a = np.zeros(19)
    shim.shim_material(C.byref(m), C.byref(x), gs.ptr(a))
    assert a[3] == 1.0 - 0.3 and a[4] == 1.0 and a[8] == 2.5 and a[14] == 0.0
    m.type = capi.PT_MAT_DIELECTRIC
    shim.shim_material(C.byref(m), C.byref(x), gs.ptr(a))
    assert a[14] == 0.01 and list(a[15:18]) == [1.0, 1.0, 1.0] and a[4] == 0.0


def test_struct_sizes_and_abi_version():
    from path_trace_golang_amd import capi

    out = (C.c_int32 * 4)()
    gs.product_host().shim_sizes(out)
    assert list(out) == [C.sizeof(capi.PtGlMaterial), C.sizeof(capi.PtShading), C.sizeof(capi.PtShadingStats), 4]
    assert (C.sizeof(capi.PtGlMaterial), C.sizeof(capi.PtShading), C.sizeof(capi.PtShadingStats)) == (40, 16, 56)
    assert capi.PT_ABI_VERSION == 4
    with open(os.path.join(ROOT, "include", "ptcore.h")) as f:
        assert "#define PT_ABI_VERSION 4" in f.read()


def test_python_flattening_and_env_switch(tmp_path):
    from path_trace_golang_amd import capi, hip

    sc, _, _ = gs.scene_pair(gs.synthetic_docs()["glass"], str(tmp_path), "glass")
    arr = hip.gl_materials(sc)
    for i, m in enumerate(sc.materials):
        assert arr[i].reflectivity == m.reflectivity
        assert list(arr[i].tint) == m.tint.as_list()
        assert arr[i].absorption_scale == m.absorption_scale
    assert arr[2].absorption_scale == 0.3 and list(arr[2].tint) == [0.6, 1.0, 0.7]
    assert hip.ShadingConfig.from_env({}).model == "cpu"
    assert hip.ShadingConfig.from_env({"PATHTRACER_GPU_SHADING": "gl"}).model == "gl"
    assert hip.ShadingConfig.from_env({"PATHTRACER_GPU_SHADING": " GL "}).model == "gl"
    assert hip.ShadingConfig.from_env({"PATHTRACER_GPU_SHADING": "cpu"}).model == "cpu"
    assert hip.ShadingConfig.from_env({"PATHTRACER_GPU_SHADING": "opengl"}).model == "cpu"
    assert hip.SHADING_MODELS == {"cpu": capi.PT_SHADING_CPU, "gl": capi.PT_SHADING_GL}
    with pytest.raises(ValueError):
        hip.set_shading(None, "vulkan")


def _host_lib():
    lib = C.CDLL(os.path.join(ROOT, "path_trace_golang_amd", "libpthost.so"))
    lib.pth_scene_load.restype = C.c_void_p
    lib.pth_scene_load.argtypes = [C.c_char_p]
    lib.pth_scene_gl_materials.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    lib.pth_set_shading.argtypes = [C.c_int]
    lib.pth_get_shading.restype = C.c_int
    return lib


def test_cpp_host_flattens_the_gl_materials_and_takes_the_switch(tmp_path):
    from path_trace_golang_amd import capi, hip

    lib = _host_lib()
    doc = gs.synthetic_docs()["metal"]
    p = tmp_path / "metal.json"
    p.write_text(json.dumps(doc))
    h = lib.pth_scene_load(str(p).encode())
    assert h
    sc, _, _ = gs.scene_pair(doc, str(tmp_path), "metal_py")
    arr = (capi.PtGlMaterial * 16)()
    n = lib.pth_scene_gl_materials(h, C.cast(arr, C.c_void_p), 16)
    want = hip.gl_materials(sc)
    assert n == len(sc.materials)
    for i in range(n):
        assert bytes(arr[i]) == bytes(want[i])
    lib.pth_set_shading(capi.PT_SHADING_GL)
    assert lib.pth_get_shading() == capi.PT_SHADING_GL
    lib.pth_set_shading(capi.PT_SHADING_CPU)
    assert lib.pth_get_shading() == capi.PT_SHADING_CPU


def _render_cli(args, env_extra=None):
    env = dict(os.environ)
    env.pop("PATHTRACER_GPU_SHADING", None)
    env.update(env_extra or {})
    return subprocess.run([os.path.join(ROOT, "path_trace_golang_amd", "render"), *args], capture_output=True, text=True,
                          env=env, timeout=60)


def test_render_cli_shading_flag():
    r = _render_cli(["-h"])
    assert "-shading string" in r.stderr
    r = _render_cli(["-shading", "vulkan", "-headless"])
    assert r.returncode == 2 and "want cpu or gl" in r.stderr
    r = _render_cli(["-shading=gl", "-headless", "-scene", "/nonexistent.json"])  # parsed, then the load fails
    assert r.returncode == 1 and "flags:" in r.stderr and "load scene" in r.stderr
    r = _render_cli(["-headless", "-scene", "/nonexistent.json"], {"PATHTRACER_GPU_SHADING": "gl"})
    assert r.returncode == 1 and "flags:" in r.stderr


def test_cpp_env_switch_default():
    code = ("import ctypes as C; l=C.CDLL(%r); l.pth_get_shading.restype=C.c_int; print(l.pth_get_shading())"
            % os.path.join(ROOT, "path_trace_golang_amd", "libpthost.so"))
    for val, want in (("gl", "1"), ("GL", "1"), ("cpu", "0"), (None, "0")):
        env = dict(os.environ)
        env.pop("PATHTRACER_GPU_SHADING", None)
        if val is not None:
            env["PATHTRACER_GPU_SHADING"] = val
        out = subprocess.run(["python", "-c", code], capture_output=True, text=True, env=env, check=True).stdout.strip()
        assert out == want, (val, out)
