"""Volumetric fog on the BVH path (pt_set_fog_walk), the parts that need no GPU: the C surface and its ctypes binding,
the new header against the gfx950 target with the library's flags and its kernels in the built code object, the environment switch,
the CLI flag, the host rule call by call -- engine.render_into (Python), engine::RenderInto (libpthost.so) and the `render` CLI in
child processes against tests/fake_ptcore_fogwalk.c, the recording stand-in of the host-trace tests with the two new entry points
beside it -- the split of pt_fog.h held to the reference by its host build, and, through the reference and numpy alone, that the
scenes of test_fog_walk_gpu.py reach what they are for."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import fog_support as fs
import fog_walk_support as fw
import host_trace_support as hts

ROOT = hts.ROOT
E = "PATHTRACER_GPU_"
CSRC = os.path.join(ROOT, "path_trace_golang_amd", "csrc")


# ---------------------------------------------------------------- the surface
def test_header_export_and_binding():
    from path_trace_golang_amd import capi

    text = open(os.path.join(ROOT, "include", "ptcore.h")).read()
    assert "int32_t pt_set_fog_walk(pt_ctx *ctx, int32_t on);" in text
    assert "int32_t pt_fog_walk_stats(pt_ctx *ctx, uint64_t out[6]);" in text
    assert "#define PT_ABI_VERSION 4" in text  # additive: the ABI number stays
    lib = capi.load()
    bound = {name: (res, args) for name, res, args in capi.SYMBOLS}
    for sym in ("pt_set_fog_walk", "pt_fog_walk_stats"):
        assert sym in bound and capi.has(sym) and sym in capi.ADDITIVE, sym
    assert bound["pt_set_fog_walk"] == (C.c_int32, [C.c_void_p, C.c_int32])
    assert bound["pt_fog_walk_stats"] == (C.c_int32, [C.c_void_p, C.POINTER(C.c_uint64)])
    # no context: refused, nothing written
    out = (C.c_uint64 * 6)(*([7] * 6))
    assert lib.pt_set_fog_walk(None, 1) == capi.PT_ERR_INVALID
    assert lib.pt_fog_walk_stats(None, out) == capi.PT_ERR_INVALID and list(out) == [7] * 6


def test_the_header_compiles_for_gfx950_and_its_kernels_are_in_the_code_object(tmp_path):
    """The header by itself against the gfx950 target with build.HIP_FLAGS (device side, front end only: a full -O3 pass over
    pt_kernels.h takes a minute, and build_core has done it for the library whose code object is read below)."""
    from path_trace_golang_amd import build

    assert "-ffp-contract=off" in build.HIP_FLAGS and "--offload-arch=gfx950" in build.HIP_FLAGS
    src = tmp_path / "fog_walk_tu.hip"
    src.write_text('#include "pt_fog_walk.h"\n')
    r = subprocess.run([build.HIPCC, *build.HIP_FLAGS, "--cuda-device-only", "-fsyntax-only", "-I" + CSRC, str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    walk = open(os.path.join(CSRC, "pt_fog_walk.h")).read()
    for name in ("void fog_bvh_kernel(", "void fog_bvh_adaptive_kernel(", "bool wave_any_hit(", "ptf::hit_object(o, r, tmin, tmax, t)",
                 "wave_first_hit<true>(", "scan_uniform(F, g_obj, r, 0, best, t_hit)", "wave_walk_coop(F, casts, r, fr.a)"):
        assert name in walk, name
    assert "asm" not in re.sub(r"//.*", "", walk)
    core = open(os.path.join(CSRC, "ptcore.hip")).read()
    assert '#include "pt_feature_walk.h"\n#include "pt_fog_walk.h"\n' in core
    assert '"fog: gpu_volumetric is not available for scenes on the BVH path (more than 128 spheres or "' in core  # the refusal text stands
    lib = open(build.build_core(), "rb").read()
    for kernel in (b"fog_bvh_kernel", b"fog_bvh_adaptive_kernel", b"fog_kernel", b"fog_adaptive_kernel"):
        assert kernel in lib, kernel


def test_env_switch():
    from path_trace_golang_amd import hip

    for v in ("1", "true", "TRUE", "on", "yes"):
        assert hip.fog_walk_from_env({"PATHTRACER_GPU_FOG_WALK": v}), v
    for v in ("", "0", "2", "no", "off", " 1", "walk"):
        assert not hip.fog_walk_from_env({"PATHTRACER_GPU_FOG_WALK": v}), v
    assert not hip.fog_walk_from_env({})


# ---------------------------------------------------------------- the split of pt_fog.h: the host build still is the reference's term
def test_the_split_model_still_matches_the_reference_ray_by_ray():
    """pt_fog.h's volume_light and fog_inscatter were split into the pieces fog_bvh_kernel walks (light_sample, light_add, light_total,
    march_range): its host build against tests/fog_reference.c on the rays of a scene with occluders, bit for bit."""
    from path_trace_golang_amd import hip

    case = fw.small_case()
    ref, shim = fs.reference(), fs.product_host()
    flat = hip.FlatScene(case["sc"])
    fog = fs.fog_of_scene(case["doc"]["fog"])
    rng = np.random.default_rng(3)
    n = 400
    rays = np.concatenate([rng.uniform([-3, 0.5, 2], [3, 4, 4], (n, 3)), rng.uniform([-0.6, -0.5, -1.2], [0.6, 0.3, -0.8], (n, 3))], 1).copy()
    keys = np.stack([np.full(n, 9, np.uint64), np.arange(n, dtype=np.uint64), np.arange(n, dtype=np.uint64) % 3], 1).copy()
    out = {}
    for name, f, scene_c in (("ref", ref.fr_inscatter_many, case["ora"].c), ("shim", shim.shim_inscatter_many, flat.c)):
        L, cnt = np.zeros((n, 3)), np.zeros((n, 3), np.uint32)
        f(C.byref(scene_c), C.byref(fog), 4, n, fs.ptr(rays), fs.ptr(keys), fs.ptr(L), fs.ptr(cnt))
        out[name] = (L, cnt)
    assert np.array_equal(out["ref"][1], out["shim"][1]) and int(out["ref"][1][:, 0].sum()) > 0
    assert np.array_equal(out["ref"][0].view(np.uint64), out["shim"][0].view(np.uint64))
    assert np.count_nonzero(out["ref"][0]) > 0


# ---------------------------------------------------------------- what the GPU scenes reach, by the reference and numpy alone
def _gpu_cases():
    return ([fw.threshold_case(), fw.room_case(), fw.far_case()] + [fw.lights_case(n) for n in (1, 9)] +
            [fw.fuzz_case(i) for i in range(len(fw.FUZZ_SEEDS))])


def test_every_gpu_scene_marches_and_casts_shadow_rays_on_the_bvh_path():
    for case in _gpu_cases():
        ns, nb, _ = fw.kinds(case)
        assert ns > 128 or nb > 128, case["name"]
        st = fw.reference(case)[2]
        assert st["steps"] > 0 and st["shadow_rays"] > 0, (case["name"], st)
    st0 = fw.reference(fw.lights_case(0))[2]
    assert st0["steps"] > 0 and st0["shadow_rays"] == 0 and st0["fog_draws"] == 0
    assert fw.kinds(fw.threshold_case()) == (131, 0, 1)  # 129 spheres + 2 sphere lights, one plane: one sphere past the grouped scan
    x = fw.far_crossing(fw.far_case())
    assert x["first_point"] > x["clip_bound"] > x["last_point"], x


@pytest.mark.parametrize("name", ["room", "far"])
def test_the_room_has_rays_hidden_by_the_plane_alone_by_an_object_alone_and_rays_that_arrive(name):
    census = fw.shadow_census(fw.room_case() if name == "room" else fw.far_case())
    assert census["plane_only"] > 0 and census["finite_only"] > 0 and census["reached"] > 0, census


def test_the_hand_made_lights_are_hidden_by_what_they_were_made_for():
    world = fw._world(fw.room_case()["doc"])
    p = np.array([0.5, 2.0, 2.0])  # a point of the open room
    for light, radius, want in ((fw.ROOM_HIDDEN_LIGHT, 0.3, "plane"), (fw.ROOM_BOXED_LIGHT, 0.2, "box")):
        to = np.array(light) - p
        dist = float(np.linalg.norm(to))
        npl, nfin = fw._blockers(world, p, to / dist, dist - radius - 0.002)
        assert (npl >= 1) if want == "plane" else (nfin >= 1), (light, npl, nfin)
    # the box does enclose its light: every axis direction from the light's centre ends on it within half its edge
    for d in np.concatenate([np.eye(3), -np.eye(3)]):
        assert fw._blockers(world, np.array(fw.ROOM_BOXED_LIGHT), d, 0.5)[1] >= 1


# ---------------------------------------------------------------- the host rule, call by call
@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    from path_trace_golang_amd import build

    build.build_host()
    tmp = str(tmp_path_factory.mktemp("host_fogwalk"))
    cc = os.environ.get("CC") or shutil.which("gcc") or "cc"
    out = {"tmp": tmp}
    for name, src in (("walk", "fake_ptcore_fogwalk.c"), ("plain", "fake_ptcore.c")):
        out[name] = os.path.join(tmp, "libptfake_%s.so" % name)
        subprocess.run([cc, "-std=c11", "-O1", "-g", "-fPIC", "-shared", "-Wall", "-Wextra", "-Wno-unused-function", "-Wno-unused-variable",
                        os.path.join(ROOT, "tests", src), "-o", out[name]], check=True)
    return out


def child(libs, driver, lib, env, mode=""):
    log = os.path.join(libs["tmp"], "%s_%s_%d.log" % (driver, lib, len(os.listdir(libs["tmp"]))))
    e = {k: v for k, v in os.environ.items() if not k.startswith(("PATHTRACER_", "PTCORE_", "PTFAKE_"))}
    e.update({E + k: v for k, v in env.items()}, PTCORE_LIB=libs[lib], PTFAKE_LOG=log, PTFAKE_SCRIPT="")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), driver, *([mode] if mode else [])], capture_output=True, text=True, cwd=ROOT,
                       env=e, timeout=120)
    trace = open(log).read().split("\n")[:-1] if os.path.exists(log) else []
    return r, trace


def run(libs, driver, lib, env, mode=""):
    r, trace = child(libs, driver, lib, env, mode)
    assert r.returncode == 0, (r.stdout, r.stderr)
    return trace


def names(trace):
    return [ln.split()[0] for ln in trace]


@pytest.mark.parametrize("driver", ["py", "host"])
def test_the_rule_call_by_call(libs, driver):
    # the switch alone: said once, in front of the frame, and nothing else changes
    trace = run(libs, driver, "walk", {"FOG_WALK": "1"})
    n = names(trace)
    assert [ln for ln in trace if ln.startswith("pt_set_fog_walk")] == ["pt_set_fog_walk on=1"]
    assert n.index("pt_set_fog") < n.index("pt_set_fog_walk") < n.index("pt_render")
    assert [ln for ln in trace if not ln.startswith("pt_set_fog_walk")] == run(libs, driver, "plain", {})
    # two frames on one context: said when it changes, not again
    twice = run(libs, driver, "walk", {"FOG_WALK": "1"}, "twice")
    assert names(twice).count("pt_set_fog_walk") == 1 and sum(ln.startswith("pt_render cfg{") for ln in twice) == 2


@pytest.mark.parametrize("driver", ["py", "host"])
def test_with_the_variable_unset_the_calls_are_what_they_were(libs, driver):
    for env in ({}, {"FOG": "1"}, {"ATROUS": "1"}, {"FEATURES": "3"}, {"FOG_WALK": "0"}, {"FOG_WALK": "walk"}):
        with_symbols = run(libs, driver, "walk", env)
        assert with_symbols == run(libs, driver, "plain", {k: v for k, v in env.items() if k != "FOG_WALK"}), env
        assert not any(x in ("pt_set_fog_walk", "pt_fog_walk_stats") for x in names(with_symbols)), env


def test_a_library_without_the_entry_point_is_refused_by_name(libs):
    r, trace = child(libs, "host", "plain", {"FOG_WALK": "1"}, "expect-error")
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "fog walk: libptcore.so lacks pt_set_fog_walk" in r.stdout
    assert not any(ln.startswith(("pt_render", "pt_begin")) for ln in trace)  # nothing was rendered
    r, trace = child(libs, "py", "plain", {"FOG_WALK": "1"})
    assert r.returncode != 0 and "has no pt_set_fog_walk" in r.stderr
    assert not any(ln.startswith(("pt_render", "pt_begin")) for ln in trace)


def test_the_python_stats_call_reaches_the_library(libs):
    r, trace = child(libs, "stats", "walk", {})
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert json.loads(r.stdout.strip().split("\n")[-1]) == {"primary_walked": 60, "primary_plain": 2, "shadow_walked": 1440, "shadow_plain": 48,
                                                            "node_visits": 30500, "deepest_stack": 11}
    assert "pt_fog_walk_stats out=set" in trace


def cli(libs, lib, *args, env=None):
    log = os.path.join(libs["tmp"], "cli_%d.log" % len(os.listdir(libs["tmp"])))
    e = {k: v for k, v in os.environ.items() if not k.startswith(("PATHTRACER_", "PTCORE_", "PTFAKE_"))}
    e.update({E + k: v for k, v in (env or {}).items()}, PTCORE_LIB=libs[lib], PTFAKE_LOG=log, PTFAKE_SCRIPT="")
    cmd = [os.path.join(ROOT, "path_trace_golang_amd", "render"), "-headless", "-gpu", "-scene", hts.FOGGY, "-width", "8", "-height", "8", "-depth", "3",
           "-spp", "16", "-out", log + ".png", *args]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, env=e, timeout=120)
    return r.returncode, r.stderr, open(log).read().split("\n")[:-1] if os.path.exists(log) else []


def test_the_cli_flag_is_one_row_and_reaches_the_engine(libs):
    for args, env, want in ((["-fog", "-fog-walk"], None, True), (["--fog-walk=true"], None, True), ([], {"FOG_WALK": "1"}, True),
                            (["-fog-walk=false"], {"FOG_WALK": "1"}, False), (["-fog"], None, False), ([], None, False)):
        code, err, trace = cli(libs, "walk", *args, env=env)
        assert code == 0, err
        assert [ln for ln in trace if ln.startswith("pt_set_fog_walk")] == (["pt_set_fog_walk on=1"] if want else []), (args, env)
    code, err, trace = cli(libs, "walk", "-fog-walk=maybe")  # a bad value is a flag error, like -fog's
    assert code == 2 and not trace and "invalid boolean value" in err
    code, err, trace = cli(libs, "plain", "-fog-walk")  # an older library: refused by name, nothing rendered
    assert code == 1 and "fog walk: libptcore.so lacks pt_set_fog_walk" in err and "pt_render" not in names(trace)
    assert cli(libs, "walk", "-fog")[2] == cli(libs, "plain", "-fog")[2]  # unset, the CLI says to the library what it said before
    main = open(os.path.join(CSRC, "host", "render_main.cpp")).read()
    assert '{"fog-walk", BOOL, &f.fog_walk}' in main and "PATHTRACER_GPU_FOG_WALK" in main


def test_the_host_layers_name_the_setting():
    host = os.path.join(CSRC, "host")
    hpp = open(os.path.join(host, "engine.hpp")).read()
    cpp = open(os.path.join(host, "engine.cpp")).read()
    assert "void SetFogWalk(bool on);" in hpp and "bool FogWalk();" in hpp and "bool FogWalkFromEnv();" in hpp
    for name in ("OPTIONAL(pt_set_fog_walk)", "PATHTRACER_GPU_FOG_WALK", "fog walk: libptcore.so lacks pt_set_fog_walk", "FOG_WALK }"):
        assert name in cpp, name
    go = open(os.path.join(ROOT, "go", "internal", "engine", "hip", "hip.go")).read()
    for name in ("C.pt_set_fog_walk(", "func SetFogWalk(", "PATHTRACER_GPU_FOG_WALK"):
        assert name in go, name
    gomain = open(os.path.join(ROOT, "go", "cmd", "render", "main.go")).read()
    assert 'flag.Bool("fog-walk"' in gomain and "hip.SetFogWalk(" in gomain
    # every C name the Go sources use is declared in the header
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptcore.h")).read(), flags=re.S)
    assert set(re.findall(r"C\.(pt_\w+)", go + gomain)) <= set(re.findall(r"\b(pt_\w+)\b", header))
    for f in ("hip.py", "engine.py"):
        assert "fog_walk" in open(os.path.join(ROOT, "path_trace_golang_amd", f)).read(), f


# ---------------------------------------------------------------- the child process
def _scene_doc():
    with open(os.path.join(ROOT, hts.SIMPLE)) as f:
        return json.load(f)


def _child_py(mode):
    sys.path.insert(0, ROOT)
    from path_trace_golang_amd import engine, scene

    img = np.zeros((8, 8, 4), np.uint8)
    for _ in range(2 if mode == "twice" else 1):
        engine.render_into(scene.Scene.decode(_scene_doc()), engine.RenderConfig(8, 8, 16, 3, 5), img, None)


def _child_stats():
    sys.path.insert(0, ROOT)
    from path_trace_golang_amd import capi, hip

    with capi.Context(ndev=1) as ctx:
        print(json.dumps(hip.fog_walk_stats(ctx)))


def _child_host(mode):
    L = C.CDLL(os.environ.get("PTHOST_LIB") or os.path.join(ROOT, "path_trace_golang_amd", "libpthost.so"))
    L.pth_last_error.restype = C.c_char_p
    L.pth_scene_decode.restype = C.c_void_p
    L.pth_scene_decode.argtypes = [C.c_char_p]
    L.pth_scene_free.argtypes = [C.c_void_p]
    L.pth_render_into.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_void_p, C.c_int32, C.c_int32,
                                  C.c_int32, C.c_void_p]
    L.pth_set_backend(1)
    h = L.pth_scene_decode(json.dumps(_scene_doc()).encode())
    assert h, L.pth_last_error()
    buf = np.zeros((8, 8, 4), np.uint8)
    for _ in range(2 if mode == "twice" else 1):
        rc = L.pth_render_into(h, 8, 8, 16, 3, 5, buf.ctypes.data_as(C.c_void_p), 8, 8, 32, None)
    L.pth_scene_free(h)
    if mode == "expect-error":
        assert rc != 0
        print(L.pth_last_error().decode())
    else:
        assert rc == 0, L.pth_last_error()
    L.pth_shutdown()


if __name__ == "__main__":
    mode = sys.argv[2] if len(sys.argv) > 2 else ""
    if sys.argv[1] == "py":
        _child_py(mode)
    elif sys.argv[1] == "stats":
        _child_stats()
    else:
        _child_host(mode)
