"""Fog (pt_set_fog, csrc/pt_fog.h) without a GPU: Go's Sin, the parameter resolution, the sky rewrite and the
in-scatter term of a host build of pt_fog.h against the independent restatement tests/fog_reference.c (linked to the
oracle), bit for bit; the ABI structs; the Python and C++ host layers that flatten scene.Fog."""
from __future__ import annotations

import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

import fog_support as fs
from conftest import ROOT, scene_path

# fog blocks over the corners of the parameter resolution (gpu.go:2024-2096) and of mediumCoeffs (gpu.go:1174-1203)
BASE = dict(color=(0.8, 0.85, 0.9), gpu_volumetric=1)
FOG_TABLE = {
    "density_only": dict(density=0.05, **BASE),
    "explicit_sigma": dict(density=0.02, scatter=0.3, sigma_s=0.04, sigma_a=0.01, g=0.2, **BASE),
    "scatter_0": dict(density=0.1, scatter=0.0, sigma_s=0.05, **BASE),
    "scatter_0_no_density": dict(sigma_s=0.05, sigma_a=0.02, **BASE),
    "negative_sigma": dict(density=0.1, scatter=0.5, sigma_s=-0.2, sigma_a=0.03, **BASE),
    "negative_both": dict(density=0.1, scatter=2.0, sigma_s=-0.2, sigma_a=-0.1, **BASE),
    "g_above": dict(density=0.05, g=1.7, **BASE),
    "g_below": dict(density=0.05, g=-3.0, **BASE),
    "octaves_0": dict(density=0.05, hetero_strength=0.3, noise_octaves=0, **BASE),
    "octaves_1": dict(density=0.05, hetero_strength=0.3, noise_octaves=1, noise_scale=2.5, **BASE),
    "octaves_7": dict(density=0.05, hetero_strength=0.3, noise_octaves=7, **BASE),
    "hetero_0": dict(density=0.05, hetero_strength=0.0, **BASE),
    "hetero_1.5": dict(density=0.05, hetero_strength=1.5, **BASE),
    "noise_scale_0": dict(density=0.05, hetero_strength=0.6, noise_scale=0.0, **BASE),
    "huge_noise_scale": dict(density=0.05, hetero_strength=0.6, noise_scale=3e7, **BASE),
}


def _doc(name):
    with open(scene_path(name)) as f:
        return json.load(f)


def _bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---------------------------------------------------------------- go_sin

def _sins(x: np.ndarray):
    x = np.ascontiguousarray(x, np.float64)
    a, b = np.empty_like(x), np.empty_like(x)
    fs.product_host().shim_sin_many(fs.ptr(x), fs.ptr(a), x.size)
    fs.reference().fr_sin_many(fs.ptr(x), fs.ptr(b), x.size)
    return a, b


def sin_range_arguments() -> np.ndarray:
    """The arguments of the range test (also what test_device_math_gpu.py gives the device): |x| < 2^29."""
    rng = np.random.default_rng(7)
    lim = 2.0 ** 29
    parts = [
        rng.uniform(-lim, lim, 400_000),                                           # the whole signed range
        np.sign(rng.uniform(-1, 1, 300_000)) * np.exp2(rng.uniform(-60, 29, 300_000)),  # every binade
        rng.uniform(-3000.0, 3000.0, 300_000),                                     # what hash31 produces on the shipped scenes
        rng.uniform(-2 * math.pi, 2 * math.pi, 50_000),
    ]
    x = np.concatenate(parts)
    return x[np.abs(x) < lim]


def sin_special_arguments() -> np.ndarray:
    """Signed zeros, subnormals, +-3 ulp around k pi/4 for k < 200, the top of the range."""
    tiny = np.array([0.0, -0.0, 5e-324, -5e-324, 2.2250738585072009e-308, -2.2250738585072014e-308, 1e-300, 2.0 ** -28])
    edges = []
    for k in range(1, 200):
        e = k * math.pi / 4
        for d in range(-3, 4):
            v = e
            for _ in range(abs(d)):
                v = np.nextafter(v, np.inf if d > 0 else -np.inf)
            edges += [v, -v]
    top = np.nextafter(2.0 ** 29, 0.0)
    return np.concatenate([tiny, np.array(edges), np.array([top, -top, 1.0, -1.0])])


def test_go_sin_equals_go_sin_bit_for_bit_over_the_range():
    x = sin_range_arguments()
    assert x.size >= 1_000_000
    a, b = _sins(x)
    bad = np.flatnonzero(_bits(a) != _bits(b))
    assert bad.size == 0, (x[bad[:5]], a[bad[:5]], b[bad[:5]])


def test_go_sin_special_arguments():
    x = sin_special_arguments()
    a, b = _sins(x)
    assert np.array_equal(_bits(a), _bits(b))
    assert math.copysign(1.0, a[1]) == -1.0  # -0 keeps its sign


# ---------------------------------------------------------------- resolution, sky

@pytest.mark.parametrize("name", sorted(FOG_TABLE))
def test_parameter_resolution_matches_reference(name):
    f = fs.fog_struct(**FOG_TABLE[name])
    a, b = np.zeros(13), np.zeros(13)
    fs.product_host().shim_resolve_flat(C.byref(f), fs.ptr(a))
    fs.reference().fr_resolve_flat(C.byref(f), fs.ptr(b))
    assert np.array_equal(_bits(a), _bits(b)), (a, b)


def test_parameter_resolution_values():
    a = np.zeros(13)
    fs.product_host().shim_resolve_flat(C.byref(fs.fog_struct(density=0.05, g=1.7, noise_octaves=7, hetero_strength=1.5)), fs.ptr(a))
    # density, scatter (1 for density > 0), sigma_s = density, sigma_a = 0, g clamped, hetero clamped, noise scale 4, octaves 5
    assert list(a[:7]) == [0.05, 1.0, 0.05, 0.0, 0.9, 1.0, 4.0] and a[10] == 5
    fs.product_host().shim_resolve_flat(C.byref(fs.fog_struct(density=-1, scatter=0, noise_octaves=0)), fs.ptr(a))
    assert list(a[:7]) == [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 4.0] and a[10] == 3


def test_sky_rewrite_matches_reference():
    from path_trace_golang_amd import capi

    for fog in (dict(density=0.02, color=(0.8, 0.85, 0.9), affect_sky=1), dict(density=0.5, color=(0.1, 0.2, 0.3), affect_sky=1),
                dict(density=0.0, color=(0.1, 0.2, 0.3), affect_sky=1), dict(density=0.3, affect_sky=0)):
        f = fs.fog_struct(**fog)
        s1, s2 = capi.PtSky(), capi.PtSky()
        for s in (s1, s2):
            s.kind = capi.PT_SKY_GRADIENT
            s.background[:] = [0.1, 0.2, 0.3]
            s.color[:] = [0.4, 0.5, 0.6]
            s.horizon[:] = [0.7, 0.8, 0.9]
            s.zenith[:] = [0.25, 0.5, 1.0]
        fs.product_host().shim_sky(C.byref(f), C.byref(s1))
        fs.reference().fr_sky(C.byref(f), C.byref(s2))  # ora_sky has pt_sky's layout
        assert bytes(s1) == bytes(s2)
        changed = bytes(s1) != bytes(capi.PtSky(capi.PT_SKY_GRADIENT, 0, (0.1, 0.2, 0.3), (0.4, 0.5, 0.6), (0.7, 0.8, 0.9), (0.25, 0.5, 1.0)))
        assert changed == (fog["density"] > 0 and fog.get("affect_sky", 0) == 1)


# ---------------------------------------------------------------- the in-scatter term

def _rays(oc, n, rng, depth_cam):
    """n rays for scene `oc` (an ora.Scene): a third are the scene camera's primary rays, the rest random positions in
    the scene's box with random (not unit) directions."""
    from oracle import ora

    cam = np.zeros(22)
    w, h = 96, 54
    ora.lib().ora_camera_setup(C.byref(oc.c.camera), w, h, cam.ctypes.data_as(C.POINTER(C.c_double)))
    k = n // 3
    u, v = rng.random(k), rng.random(k)
    d_cam = cam[3:6] + cam[6:9] * u[:, None] + cam[9:12] * v[:, None] - cam[0:3]
    o_cam = np.broadcast_to(cam[0:3], (k, 3))
    pos = np.array([list(oc.c.objects[i].position) for i in range(oc.c.nobjects)])
    lo, hi = pos.min(0) - 2.0, pos.max(0) + 2.0
    m = n - k
    o_rnd = lo + (hi - lo) * rng.random((m, 3))
    d_rnd = rng.normal(size=(m, 3)) * rng.uniform(0.2, 3.0, (m, 1))
    rays = np.concatenate([np.hstack([o_cam, d_cam]), np.hstack([o_rnd, d_rnd])])
    keys = np.stack([rng.integers(0, 2 ** 63, n, dtype=np.uint64), rng.integers(0, 2 ** 28, n, dtype=np.uint64),
                     rng.integers(0, 2 ** 12, n, dtype=np.uint64)], axis=1)
    return np.ascontiguousarray(rays), np.ascontiguousarray(keys)


def _terms(oc, fog, depth, rays, keys):
    n = rays.shape[0]
    La, Lb = np.zeros((n, 3)), np.zeros((n, 3))
    ca, cb = np.zeros((n, 3), np.uint32), np.zeros((n, 3), np.uint32)
    fs.product_host().shim_inscatter_many(C.byref(oc.c), C.byref(fog), depth, n, fs.ptr(rays), fs.ptr(keys), fs.ptr(La), fs.ptr(ca))
    fs.reference().fr_inscatter_many(C.byref(oc.c), C.byref(fog), depth, n, fs.ptr(rays), fs.ptr(keys), fs.ptr(Lb), fs.ptr(cb))
    return La, Lb, ca, cb


def test_scene_layouts_are_shared():
    from oracle import ora

    from path_trace_golang_amd import capi

    # the shim reads the oracle's scene structs as pt_scene
    for a, b in ((ora.OraScene, capi.PtScene), (ora.OraMaterial, capi.PtMaterial), (ora.OraObject, capi.PtObject),
                 (ora.OraSky, capi.PtSky), (ora.OraCamera, capi.PtCamera)):
        assert C.sizeof(a) == C.sizeof(b)


@pytest.mark.parametrize("scene_name", ["gpu_showcase", "test_scene"])
def test_inscatter_term_matches_reference_bit_for_bit(scene_name):
    from oracle import ora

    oc = ora.Scene.load(scene_path(scene_name))
    rng = np.random.default_rng(11 if scene_name == "gpu_showcase" else 12)
    blocks = [("scene", fs.fog_of_scene(_doc(scene_name)["fog"]))] + [(k, fs.fog_struct(**v)) for k, v in sorted(FOG_TABLE.items())]
    per = 50_000 // len(blocks) + 1
    total = nonzero = shadow = 0
    for name, fog in blocks:
        rays, keys = _rays(oc, per, rng, 8)
        La, Lb, ca, cb = _terms(oc, fog, 8, rays, keys)
        bad = np.flatnonzero(np.any(_bits(La) != _bits(Lb), axis=1))
        assert bad.size == 0, (name, bad[:3], La[bad[:3]], Lb[bad[:3]])
        assert np.array_equal(ca, cb), name
        total += per
        nonzero += int(np.count_nonzero(np.any(La != 0, axis=1)))
        shadow += int(ca[:, 0].sum())
    assert total >= 50_000
    assert nonzero > total // 4 and shadow > total  # the comparison is not over zeros
    # max_depth 0 and a block without gpu_volumetric add nothing
    rays, keys = _rays(oc, 300, rng, 8)
    La, Lb, ca, cb = _terms(oc, blocks[0][1], 0, rays, keys)
    assert not La.any() and not Lb.any() and not ca.any()


def test_scene_fog_blocks_use_every_light():
    from oracle import ora

    oc = ora.Scene.load(scene_path("gpu_showcase"))
    rays, keys = _rays(oc, 64, np.random.default_rng(3), 8)
    _, _, ca, _ = _terms(oc, fs.fog_of_scene(_doc("gpu_showcase")["fog"]), 8, rays, keys)
    # seven emissive spheres: two draws per light and march step taken
    assert np.array_equal(ca[:, 1], ca[:, 2] * 14)


# ---------------------------------------------------------------- the term on random scenes

def fuzz_scene(i, tmp_dir):
    """Case i of fuzz_support.host_fuzz_case as (case, scene.Scene, hip.FlatScene, ora.Scene, PtFog)."""
    import glshade_support as gs
    from fuzz_support import host_fuzz_case

    case = host_fuzz_case(i)
    sc, flat, oc = gs.scene_pair(case["doc"], str(tmp_dir), "fuzz%d" % i)
    return case, sc, flat, oc, fs.fog_of_scene(case["doc"]["fog"])


FUZZ_SCENES, FUZZ_RAYS = 64, 600


def test_inscatter_term_matches_reference_on_random_scenes(tmp_path):
    """The host build against the restatement on the generator's scenes (overlapping, nested, coincident, half-grid geometry,
    missing material ids, 1..150 objects, 0 / 1 / 8 / 9 / 12 lights) with random fog blocks: this is what says the inputs of
    the GPU fuzz are clean -- a disagreement there then belongs to the device."""
    total = nonzero = shadow = steps = nans = volumetric = 0
    sizes, lights = set(), set()
    for i in range(FUZZ_SCENES):
        case, sc, flat, oc, fog = fuzz_scene(i, tmp_path)
        rays, keys = _rays(oc, FUZZ_RAYS, np.random.default_rng([31, i]), 8)
        La, Lb, ca, cb = _terms(oc, fog, case["depth"], rays, keys)
        bad = np.flatnonzero(np.any(_bits(La) != _bits(Lb), axis=1) | np.any(ca != cb, axis=1))
        assert bad.size == 0, (i, bad[:3], La[bad[:3]], Lb[bad[:3]], ca[bad[:3]], cb[bad[:3]])
        total += FUZZ_RAYS
        nans += int(np.count_nonzero(np.isnan(La)))
        nonzero += int(np.count_nonzero(np.any(La != 0, axis=1)))
        shadow += int(ca[:, 0].sum())
        steps += int(ca[:, 2].sum())
        volumetric += int(fog.gpu_volumetric)
        sizes.add(case["nobj"])
        lights.add(int(ca[:, 1].max()) // 48 if ca[:, 2].max() == 24 else -1)  # draws = 2 per light and step
    assert FUZZ_SCENES >= 60 and total >= 30_000
    assert min(sizes) == 1 and max(sizes) == 150
    assert nans == 0
    assert nonzero > total // 10 and shadow > total and steps > total  # the comparison is not over zeros
    assert {0, 1, 8, 9, 12} <= lights, lights
    assert FUZZ_SCENES // 2 < volumetric < FUZZ_SCENES  # mostly, not always, volumetric


# ---------------------------------------------------------------- ABI and host layers

def test_fog_struct_sizes_agree_between_c_and_ctypes(tmp_path):
    from path_trace_golang_amd import capi

    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ptcore.h"\n'
                   'int main(void) { printf("%d %d %d %d\\n", (int)sizeof(pt_fog), (int)sizeof(pt_fog_stats), '
                   '(int)offsetof(pt_fog, noise_octaves), (int)offsetof(pt_fog_stats, shadow_rays)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(capi.PtFog), C.sizeof(capi.PtFogStats), capi.PtFog.noise_octaves.offset,
                   capi.PtFogStats.shadow_rays.offset]
    assert got[:2] == [96, 40]
    assert capi.PT_ABI_VERSION == 4
    names = [n for n, _, _ in capi.SYMBOLS]
    assert "pt_set_fog" in names and "pt_fog_last_stats" in names


class _FakeLib:
    """Stands in for libptcore.so: records what hip.render hands to pt_set_fog."""

    def __init__(self):
        self.fog = []

    def pt_set_fog(self, ctx, fog):
        self.fog.append(None if fog is None else bytes(fog._obj))
        return 0

    def pt_render(self, *a):
        return 0


class _FakeCtx:
    handle = None


def test_render_flattens_the_fog_block(monkeypatch):
    from path_trace_golang_amd import capi, hip, scene

    fake = _FakeLib()
    monkeypatch.setattr(capi, "load", lambda: fake)
    sc = scene.load(scene_path("gpu_showcase"))
    img = np.zeros((4, 4, 4), np.uint8)
    cfg = hip.RenderConfig(4, 4, 1, 2, 1)
    hip.render(sc, cfg, img, ctx=_FakeCtx(), fog=True)
    hip.render(sc, cfg, img, ctx=_FakeCtx())
    hip.render(scene.load(scene_path("example_simple")), cfg, img, ctx=_FakeCtx(), fog=True)
    assert fake.fog[1] is None and fake.fog[2] is None
    f = capi.PtFog.from_buffer_copy(fake.fog[0])
    d = _doc("gpu_showcase")["fog"]
    assert (f.density, list(f.color), f.scatter, f.sigma_s, f.sigma_a, f.g, f.hetero_strength, f.noise_scale) == (
        d["density"], [d["color"]["r"], d["color"]["g"], d["color"]["b"]], d["scatter"], d["sigma_s"], d["sigma_a"], d["g"],
        d["hetero_strength"], d["noise_scale"])
    assert (f.noise_octaves, f.affect_sky, f.gpu_volumetric, f.reserved) == (3, 0, 1, 0)


def test_fog_config_from_env():
    from path_trace_golang_amd import hip

    assert hip.FogConfig.from_env({}).enabled is False
    for v in ("1", "true", "ON", "yes"):
        assert hip.FogConfig.from_env({"PATHTRACER_GPU_FOG": v}).enabled is True
    for v in ("0", "false", "", "2"):
        assert hip.FogConfig.from_env({"PATHTRACER_GPU_FOG": v}).enabled is False


def _host():
    from path_trace_golang_amd import build

    build.build_host()
    return os.path.join(ROOT, "path_trace_golang_amd", "render"), os.path.join(ROOT, "path_trace_golang_amd", "libpthost.so")


def test_host_mirror_flattens_the_fog_block():
    from path_trace_golang_amd import capi

    _, lib = _host()
    L = C.CDLL(lib)
    L.pth_scene_load.restype = C.c_void_p
    L.pth_scene_load.argtypes = [C.c_char_p]
    L.pth_scene_fog.argtypes = [C.c_void_p, C.POINTER(capi.PtFog)]
    L.pth_scene_free.argtypes = [C.c_void_p]
    h = L.pth_scene_load(scene_path("test_scene").encode())
    f = capi.PtFog()
    assert L.pth_scene_fog(h, C.byref(f)) == 1
    assert bytes(f) == bytes(fs.fog_of_scene(_doc("test_scene")["fog"]))
    L.pth_scene_free(h)
    h = L.pth_scene_load(scene_path("example_simple").encode())
    assert L.pth_scene_fog(h, C.byref(f)) == 0
    L.pth_scene_free(h)


def _run_render(args, env_extra=None, tmp_path=None):
    exe, _ = _host()
    env = {k: v for k, v in os.environ.items() if k != "PATHTRACER_GPU_FOG"}
    env.update(env_extra or {})
    out = os.path.join(str(tmp_path), "o.png")
    r = subprocess.run([exe, "-headless", "-gpu", "-scene", scene_path("test_scene"), "-width", "8", "-height", "8", "-spp", "1",
                        "-depth", "2", "-out", out, *args], capture_output=True, text=True, timeout=120, env=env)
    return r


def test_render_cli_fog_flag_and_env(tmp_path):
    r = _run_render(["-fog"], tmp_path=tmp_path)
    assert "fog: drawing the scene's fog block (present)" in r.stderr
    r = _run_render([], {"PATHTRACER_GPU_FOG": "1"}, tmp_path=tmp_path)
    assert "fog: drawing the scene's fog block" in r.stderr
    r = _run_render(["-fog=false"], {"PATHTRACER_GPU_FOG": "1"}, tmp_path=tmp_path)
    assert "fog:" not in r.stderr
    r = _run_render([], tmp_path=tmp_path)
    assert "fog:" not in r.stderr
    r = _run_render(["-fog=maybe"], tmp_path=tmp_path)
    assert r.returncode == 2 and 'invalid boolean value "maybe" for -fog' in r.stderr
    exe, _ = _host()
    assert "-fog" in subprocess.run([exe, "-h"], capture_output=True, text=True).stderr
