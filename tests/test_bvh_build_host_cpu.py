"""B5: the device BVH build (pt_set_bvh_build) in the layers above the library, without a GPU: the C surface and its
ctypes binding, the debug entry point, the environment setting, the CLI flag and the host rule call by call -- engine.render_into
(Python), engine::RenderInto (libpthost.so) and the `render` CLI in child processes against tests/fake_ptcore_build.c, the recording
stand-in of the host-trace tests with the two new entry points beside it."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

import host_trace_support as hts

ROOT = hts.ROOT
E = "PATHTRACER_GPU_"
CSRC = os.path.join(ROOT, "path_trace_golang_amd", "csrc")
KERNELS = (b"bvh_build_centroid_kernel", b"bvh_build_frame_kernel", b"bvh_build_keys_kernel", b"bvh_build_sort_hist_kernel",
           b"bvh_build_sort_scatter_kernel", b"bvh_build_scan_reduce_kernel", b"bvh_build_scan_sums_kernel", b"bvh_build_scan_apply_kernel",
           b"bvh_build_radix_kernel", b"bvh_build_boxes_kernel", b"bvh_build_level_count_kernel", b"bvh_build_level_write_kernel",
           b"bvh_build_objs_kernel")


def test_header_export_and_binding():
    from path_trace_golang_amd import capi

    text = open(os.path.join(ROOT, "include", "ptcore.h")).read()
    assert "int32_t pt_set_bvh_build(pt_ctx *ctx, int32_t mode);" in text
    assert "int32_t pt_bvh_build_stats(pt_ctx *ctx, struct pt_bvh_build_stats *out);" in text
    assert "int32_t pt_debug_bvh_build_check(const pt_scene *scene, int32_t out[8]);" in text
    assert "#define PT_ABI_VERSION 4" in text  # additive: the ABI number stays
    lib = capi.load()
    bound = {name: (res, args) for name, res, args in capi.SYMBOLS}
    for sym in ("pt_set_bvh_build", "pt_bvh_build_stats", "pt_debug_bvh_build_check"):
        assert sym in bound and capi.has(sym) and sym in capi.ADDITIVE, sym
    assert bound["pt_set_bvh_build"] == (C.c_int32, [C.c_void_p, C.c_int32])
    assert C.sizeof(capi.PtBvhBuildStats) == 2 * 8 + 6 * 4 + 5 * 8
    st = capi.PtBvhBuildStats()
    st.device_builds = 9
    assert lib.pt_set_bvh_build(None, 1) == capi.PT_ERR_INVALID
    assert lib.pt_bvh_build_stats(None, C.byref(st)) == capi.PT_ERR_INVALID and st.device_builds == 9
    assert lib.pt_debug_bvh_build_check(None, None) == capi.PT_ERR_INVALID
    for k, name in enumerate(("NONE", "HOST", "DEVICE")):
        assert getattr(capi, "PT_BVH_BUILDER_" + name) == k and re.search(r"PT_BVH_BUILDER_%s = %d\b" % (name, k), text), name
    for k, name in enumerate(("NONE", "STACK", "WALK32", "NOT_BVH")):
        assert getattr(capi, "PT_BVH_BUILD_FALLBACK_" + name) == k and re.search(r"PT_BVH_BUILD_FALLBACK_%s = %d\b" % (name, k), text), name


def test_the_kernels_are_in_the_code_object():
    lib = open(os.path.join(ROOT, "path_trace_golang_amd", "libptcore.so"), "rb").read()
    for name in KERNELS:
        assert name in lib, name


def test_the_debug_entry_point_checks_the_host_restatement():
    from path_trace_golang_amd import hip, synth

    for n in (1, 5, 300):
        r = hip.bvh_build_check(synth.make_scene(max(n, 17), 4) if n >= 17 else _few(n))
        assert r["nodes"] >= 1 and r["objects"] >= n and r["depth"] >= 1
        assert (r["not_reached_once"], r["objects_outside"], r["children_outside"], r["faults"]) == (0, 0, 0, 0), (n, r)
        assert r["stack_need"] < 96


def _few(n):
    from path_trace_golang_amd import synth

    sc = synth.make_scene(17, 4)
    keep = [o for o in sc.objects if o.type == "plane"] + [o for o in sc.objects if o.type != "plane"][:n]
    sc.objects[:] = keep
    return sc


def test_environment_parsing():
    from path_trace_golang_amd import hip

    for v, want in (("device", 1), (" Device ", 1), ("host", 0), ("", 0)):
        assert hip.bvh_build_from_env({E + "BVH_BUILD": v}) == want, v
    assert hip.bvh_build_from_env({}) == 0
    for v in ("1", "gpu", "on"):
        with pytest.raises(ValueError):
            hip.bvh_build_from_env({E + "BVH_BUILD": v})


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    from path_trace_golang_amd import build

    build.build_host()
    tmp = str(tmp_path_factory.mktemp("host_build"))
    cc = os.environ.get("CC") or shutil.which("gcc") or "cc"
    out = {"tmp": tmp}
    for name, src in (("build", "fake_ptcore_build.c"), ("plain", "fake_ptcore.c")):
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
    # the mode alone: said once, in front of the frame, and nothing else changes
    trace = run(libs, driver, "build", {"BVH_BUILD": "device"})
    n = names(trace)
    assert [ln for ln in trace if ln.startswith("pt_set_bvh_build")] == ["pt_set_bvh_build mode=1"]
    assert n.index("pt_set_bvh_build") < n.index("pt_render")
    assert [ln for ln in trace if not ln.startswith("pt_set_bvh_build")] == run(libs, driver, "plain", {})
    # two frames on one context: said when it changes, not again
    twice = run(libs, driver, "build", {"BVH_BUILD": "device"}, "twice")
    assert names(twice).count("pt_set_bvh_build") == 1 and sum(ln.startswith("pt_render cfg{") for ln in twice) == 2


@pytest.mark.parametrize("driver", ["py", "host"])
def test_with_the_variable_unset_the_calls_are_what_they_were(libs, driver):
    for env in ({}, {"ATROUS": "1"}, {"TEMPORAL": "1"}, {"BVH_BUILD": "host"}):
        with_symbols = run(libs, driver, "build", env)
        assert with_symbols == run(libs, driver, "plain", {k: v for k, v in env.items() if k != "BVH_BUILD"}), env
        assert "pt_set_bvh_build" not in names(with_symbols)


def test_a_library_without_the_entry_point_is_refused_by_name(libs):
    r, trace = child(libs, "host", "plain", {"BVH_BUILD": "device"}, "expect-error")
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "BVH device build: libptcore.so lacks pt_set_bvh_build" in r.stdout
    assert not any(ln.startswith(("pt_render", "pt_begin")) for ln in trace)  # nothing was rendered
    r, trace = child(libs, "py", "plain", {"BVH_BUILD": "device"})
    assert r.returncode != 0 and "has no pt_set_bvh_build" in r.stderr
    assert not any(ln.startswith(("pt_render", "pt_begin")) for ln in trace)


def test_the_python_stats_call_reaches_the_library(libs):
    r, trace = child(libs, "stats", "build", {})
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert json.loads(r.stdout.strip().split("\n")[-1]) == dict(host_builds=3, device_builds=5, builder=2, last_fallback=1, nodes=77, depth=6,
                                                                stack_need=9, cost=12.5, device_ms=0.25, prepare_ms=1.5, upload_ms=0.75, readback_ms=0.125)
    assert "pt_bvh_build_stats out=set" in trace


def cli(libs, lib, *args, env=None):
    log = os.path.join(libs["tmp"], "cli_%d.log" % len(os.listdir(libs["tmp"])))
    e = {k: v for k, v in os.environ.items() if not k.startswith(("PATHTRACER_", "PTCORE_", "PTFAKE_"))}
    e.update({E + k: v for k, v in (env or {}).items()}, PTCORE_LIB=libs[lib], PTFAKE_LOG=log, PTFAKE_SCRIPT="")
    cmd = [os.path.join(ROOT, "path_trace_golang_amd", "render"), "-headless", "-gpu", "-scene", hts.SIMPLE, "-width", "8", "-height", "8", "-depth", "3",
           "-spp", "16", "-out", log + ".png", *args]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, env=e, timeout=120)
    return r.returncode, r.stderr, open(log).read().split("\n")[:-1] if os.path.exists(log) else []


def test_the_cli_flag_is_one_row_and_reaches_the_engine(libs):
    for args, env, want in ((["-bvh-build", "device"], None, "1"), (["--bvh-build=device"], None, "1"), ([], {"BVH_BUILD": "device"}, "1"),
                            (["-bvh-build=host"], {"BVH_BUILD": "device"}, None), ([], None, None)):
        code, err, trace = cli(libs, "build", *args, env=env)
        assert code == 0, err
        assert [ln for ln in trace if ln.startswith("pt_set_bvh_build")] == (["pt_set_bvh_build mode=" + want] if want else []), (args, env)
    code, err, trace = cli(libs, "build", "-bvh-build", "gpu")
    assert code == 2 and "want host or device" in err and "pt_render" not in names(trace)
    code, err, trace = cli(libs, "plain", "-bvh-build", "device")  # an older library: refused by name, nothing rendered
    assert code == 1 and "BVH device build: libptcore.so lacks pt_set_bvh_build" in err and "pt_render" not in names(trace)
    assert cli(libs, "build")[2] == cli(libs, "plain")[2]  # unset, the CLI says to the library what it said before
    main = open(os.path.join(CSRC, "host", "render_main.cpp")).read()
    assert main.count('{"bvh-build", BUILDER, &f.bvh_build}') == 1


def test_the_host_layers_name_the_setting():
    host = os.path.join(CSRC, "host")
    hpp = open(os.path.join(host, "engine.hpp")).read()
    cpp = open(os.path.join(host, "engine.cpp")).read()
    assert "void SetBvhBuild(int mode);" in hpp and "int BvhBuildFromEnv();" in hpp
    for name in ("OPTIONAL(pt_set_bvh_build)", "PATHTRACER_GPU_BVH_BUILD", "BVH device build: libptcore.so lacks pt_set_bvh_build"):
        assert name in cpp, name
    go = open(os.path.join(ROOT, "go", "internal", "engine", "hip", "hip.go")).read()
    for name in ("C.pt_set_bvh_build(", "func SetBvhBuild(", "PATHTRACER_GPU_BVH_BUILD"):
        assert name in go, name
    gomain = open(os.path.join(ROOT, "go", "cmd", "render", "main.go")).read()
    assert 'flag.String("bvh-build"' in gomain and "hip.SetBvhBuild(" in gomain
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptcore.h")).read(), flags=re.S)
    assert set(re.findall(r"C\.(pt_\w+)", go + gomain)) <= set(re.findall(r"\b(pt_\w+)\b", header))


# ---------------------------------------------------------------- the child process
def _scene_doc():
    with open(os.path.join(ROOT, hts.SIMPLE)) as f:
        return json.load(f)


def _child_py(mode):
    import numpy as np

    sys.path.insert(0, ROOT)
    from path_trace_golang_amd import engine, scene

    img = np.zeros((8, 8, 4), np.uint8)
    for _ in range(2 if mode == "twice" else 1):
        engine.render_into(scene.Scene.decode(_scene_doc()), engine.RenderConfig(8, 8, 16, 3, 5), img, None)


def _child_stats():
    sys.path.insert(0, ROOT)
    from path_trace_golang_amd import capi, hip

    with capi.Context(ndev=1) as ctx:
        print(json.dumps(hip.bvh_build_stats(ctx)))


def _child_host(mode):
    import numpy as np

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
    which, mode = sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else ""
    if which == "py":
        _child_py(mode)
    elif which == "stats":
        _child_stats()
    else:
        _child_host(mode)
