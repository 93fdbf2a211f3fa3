"""First-hit features and the a-trous filter for GL-shaded frames (pt_set_shading_features), the parts that need no GPU:
the host build of csrc/pt_gl_features.h against tests/gl_features_reference.c bit for bit -- over the loop and over the tree --, the
classes of first hit the test scenes hold (asserted from the reference alone), the C surface and its ctypes binding, the environment
switch, and the host rule call by call against tests/fake_ptcore_glfeat.c."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import gl_features_support as gf
import host_trace_support as hts

ROOT = hts.ROOT
E = "PATHTRACER_GPU_"
CSRC = os.path.join(ROOT, "path_trace_golang_amd", "csrc")


# ---------------------------------------------------------------- the model against its reference
@pytest.mark.parametrize("k", gf.KS)
@pytest.mark.parametrize("name", gf.SHIPPED)
def test_host_build_equals_the_reference_on_the_shipped_scenes(name, k):
    case = gf.shipped_case(name)
    assert case["cfg"][:3] == (40, 24, 3)
    ref, got = gf.ref_features(case, k=k), gf.host_features(case, k=k)
    assert gf.same_planes(ref, got), [int(np.count_nonzero(a != b)) for a, b in zip(ref, got[:4])]
    assert np.all(ref[2][..., 2] == 16 * min(k, 3))  # every path counts, only the passes that exist


def test_host_build_equals_the_reference_on_random_scenes():
    hits = 0
    for i in range(gf.N_FUZZ):
        case = gf.fuzz_case(i)
        assert case["cfg"][:2] == (24, 16)
        k = (1, 2, 3)[i % 3]
        ref, got = gf.ref_features(case, k=k), gf.host_features(case, k=k)
        assert gf.same_planes(ref, got), (i, [int(np.count_nonzero(a != b)) for a, b in zip(ref, got[:4])])
        hits += int(ref[2][..., 1].sum())
    assert gf.N_FUZZ == 32 and hits > 50_000


@pytest.mark.parametrize("k", [1, 3])
def test_the_tree_walk_gives_the_bits_of_the_loop_past_128_spheres(k):
    room = gf.room_case()
    ns, nb, _ = gf.gw.kinds(room)
    assert ns > 128 and nb > 128 and room["cfg"][:2] == (33, 20)
    ref = gf.ref_features(room, k=k)
    loop, tree = gf.host_features(room, k=k), gf.host_features(room, k=k, tree=True)
    assert gf.same_planes(ref, loop) and gf.same_planes(ref, tree)
    wc = tree[4]
    assert wc["closest_walked"] == 16 * k * 33 * 20 and wc["closest_plain"] == 0 and wc["shadow_walked"] == 0 and wc["deepest_stack"] >= 1, wc


def test_a_frame_with_fewer_passes_than_k_holds_the_passes_it_has():
    case = gf.shipped_case("test_scene")
    for done in (1, 2):
        ref, got = gf.ref_features(case, passes=done, k=5), gf.host_features(case, passes=done, k=5)
        assert gf.same_planes(ref, got) and np.all(ref[2][..., 2] == 16 * done)
        assert gf.same_planes(ref, gf.ref_features(case, passes=3, k=done))  # ... which are those of k = passes done


def test_the_scenes_are_not_hollow():
    """From the reference alone, over the scenes of these tests and of test_gl_features_gpu.py together."""
    cases = [gf.shipped_case(n) for n in gf.SHIPPED] + [gf.fuzz_case(i) for i in range(gf.N_FUZZ)] + [gf.room_case(), gf.back_face_case()]
    full = partial = none = 0
    cls = dict.fromkeys(gf.CLASSES, 0)
    for case in cases:
        k = 2
        fd = gf.ref_features(case, passes=3, k=k)[2]
        full += int(np.count_nonzero(fd[..., 1] == 16 * k))
        partial += int(np.count_nonzero((fd[..., 1] > 0) & (fd[..., 1] < 16 * k)))
        none += int(np.count_nonzero(fd[..., 1] == 0))
        for key, v in gf.ref_classes(case, passes=3, k=k).items():
            cls[key] += v
    print(full, partial, none, cls)
    assert full > 1000 and partial > 100 and none > 100, (full, partial, none)
    assert cls["sphere"] > 1000 and cls["box"] > 1000 and cls["plane"] > 1000 and cls["back_face"] > 100 and cls["miss"] > 1000, cls
    assert cls["paths"] == cls["sphere"] + cls["box"] + cls["plane"] + cls["miss"]
    # the GPU tests' own scenes hold an edge pixel and a miss each way too
    gpu_cls = dict.fromkeys(gf.CLASSES, 0)
    for case in (gf.shipped_case("gpu_showcase"), gf.shipped_case("test_scene"), gf.fuzz_case(2, gf.W, gf.H, 3, gpu=True), gf.fuzz_case(3, gf.W, gf.H, 3, gpu=True)):
        for key, v in gf.ref_classes(case, k=1).items():
            gpu_cls[key] += v
    assert min(gpu_cls[key] for key in ("sphere", "box", "plane", "back_face", "miss")) > 0, gpu_cls
    # thin lens and pinhole
    lens = {n: float(gf.shipped_case(n)["doc"]["camera"].get("aperture", 0)) for n in gf.SHIPPED}
    assert lens["gpu_showcase"] > 0 and lens["metal_glass_room"] > 0 and lens["test_scene"] == 0, lens
    # the id plane is the first hit of path 0, an index into the scene's own list
    case = gf.shipped_case("gpu_showcase")
    ids = gf.ref_features(case, k=1)[3]
    assert ids.min() >= -1 and ids.max() < len(case["doc"]["objects"]) and len(np.unique(ids)) > 5


def test_an_unknown_type_is_a_sphere_and_keeps_its_index():
    """GL's object list is the scene's: the id plane indexes pt_scene.objects, and the unknown object can be hit."""
    import glshade_support as gs

    doc = gs.synthetic_docs()["edge"]
    case = gf.gw._case("glf-edge", doc, (gf.W, gf.H, 2, gf.DEPTH, gf.SEED))
    torus = [o["id"] for o in doc["objects"]].index("torus")
    ref, got = gf.ref_features(case, k=2), gf.host_features(case, k=2)
    assert gf.same_planes(ref, got) and int(np.count_nonzero(ref[3] == torus)) > 5


def test_the_quality_measurement_runs_and_is_finite():
    """tools/gl_features_quality.py's measurement at a size a test can afford (the figures of DESIGN 3.8b are the tool's, at 80 x 48
    against 512 passes).  Nothing but finiteness is asserted: the default sigmas were chosen on CPU-model frames."""
    q = gf.quality("example_simple", 20, 12, 4, 32, depth=3)
    print(q)
    for key in ("rel_mse_unfiltered", "rel_mse_filtered", "ratio", "noise_before", "noise_after"):
        assert np.isfinite(q[key]) and q[key] >= 0, (key, q[key])
    assert q["bad_pixels"] == 0


# ---------------------------------------------------------------- the surface
def test_header_export_and_binding():
    from path_trace_golang_amd import capi

    text = open(os.path.join(ROOT, "include", "ptcore.h")).read()
    assert "int32_t pt_set_shading_features(pt_ctx *ctx, int32_t on);" in text
    assert "#define PT_ABI_VERSION 4" in text  # additive: the ABI number stays
    assert "16 x the mean path radiance" in text and "csrc/pt_gl_features.h" in text
    lib = capi.load()
    bound = {name: (res, args) for name, res, args in capi.SYMBOLS}
    assert "pt_set_shading_features" in bound and capi.has("pt_set_shading_features") and "pt_set_shading_features" in capi.ADDITIVE
    assert bound["pt_set_shading_features"] == (C.c_int32, [C.c_void_p, C.c_int32])
    assert lib.pt_set_shading_features(None, 1) == capi.PT_ERR_INVALID  # no context


def test_the_header_is_one_statement_and_its_kernels_are_in_the_code_object(tmp_path):
    from path_trace_golang_amd import build

    src = tmp_path / "gl_features_tu.hip"
    src.write_text('#include "pt_gl_features.h"\n')
    r = subprocess.run([build.HIPCC, *build.HIP_FLAGS, "--cuda-device-only", "-fsyntax-only", "-I" + CSRC, str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    feat = re.sub(r"//.*", "", open(os.path.join(CSRC, "pt_gl_features.h")).read())
    shade = re.sub(r"//.*", "", open(os.path.join(CSRC, "pt_glshade.h")).read())
    assert "primary_ray(S, key, x, y, pass, k, rs, cnt, ro, rd);" in feat and "world.closest(ro, rd, 0.001, 1e20, -1, t)" in feat
    assert "stream_init" not in feat and "lens_radius" not in feat  # the ray is not restated
    assert shade.count("primary_ray(") == 2 and shade.count("lens_radius > 0.0") == 1  # the helper, and gl_pass calling it
    kernels = open(os.path.join(CSRC, "pt_kernels.h")).read()
    for text in ("void gl_feature_kernel(const GlFeatureArgs A)", "void gl_feature_bvh_kernel(const GlFeatureWalkArgs W)",
                 "void atrous_finish_gl_kernel(", "void atrous_finish_kernel(const double *__restrict__ col, uint8_t *__restrict__ rgba, uint32_t npix)"):
        assert text in kernels, text
    core = open(os.path.join(CSRC, "ptcore.hip")).read()
    for refusal in ('"features: not available with GL shading (pt_set_shading), where a sample is a pass of 16 paths"',
                    '"not available for a frame rendered with GL shading (pt_set_shading)"',
                    '"adaptive sampling: not available with GL shading (pt_set_shading)"'):
        assert refusal in core, refusal  # the refusals stand
    lib = open(build.build_core(), "rb").read()
    for kernel in (b"gl_feature_kernel", b"gl_feature_bvh_kernel", b"atrous_finish_gl_kernel"):
        assert kernel in lib, kernel


def test_env_switch():
    from path_trace_golang_amd import hip

    for v in ("1", "true", "TRUE", "on", "yes"):
        assert hip.shading_features_from_env({"PATHTRACER_GPU_SHADING_FEATURES": v}), v
    for v in ("", "0", "2", "no", "off", " 1", "features"):
        assert not hip.shading_features_from_env({"PATHTRACER_GPU_SHADING_FEATURES": v}), v
    assert not hip.shading_features_from_env({})


def test_scene_allows_features_keeps_its_answers_and_knows_the_switch():
    from path_trace_golang_amd import hip

    small, big = gf.shipped_case("test_scene")["sc"], gf.room_case()["sc"]
    # the positional calls of before
    assert hip.scene_allows_features(small) and hip.scene_allows_features(small, "cpu", False)
    assert not hip.scene_allows_features(small, "gl") and not hip.scene_allows_features(small, "gl", True)
    assert not hip.scene_allows_features(big) and hip.scene_allows_features(big, "cpu", True)
    # the switch
    assert hip.scene_allows_features(small, "gl", shading_features=True)
    assert not hip.scene_allows_features(big, "gl", shading_features=True)
    assert not hip.scene_allows_features(big, "gl", True, shading_features=True)  # pt_set_feature_walk is not consulted in GL mode
    assert hip.scene_allows_features(big, "gl", shading_features=True, shading_walk=True)
    assert hip.scene_allows_features(small, "cpu", shading_features=True) and not hip.scene_allows_features(big, "cpu", shading_features=True, shading_walk=True)


# ---------------------------------------------------------------- the host rule, call by call
@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    from path_trace_golang_amd import build

    build.build_host()
    tmp = str(tmp_path_factory.mktemp("host_glfeat"))
    cc = os.environ.get("CC") or shutil.which("gcc") or "cc"
    out = {"tmp": tmp}
    for name, src in (("feat", "fake_ptcore_glfeat.c"), ("plain", "fake_ptcore.c")):
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


SETTER = "pt_set_shading_features"
GL_ON = {"SHADING": "gl", "SHADING_FEATURES": "1"}


@pytest.mark.parametrize("driver", ["py", "host"])
def test_the_rule_call_by_call(libs, driver):
    # the switch alone: said once, in front of the frame, and nothing else changes
    trace = run(libs, driver, "feat", GL_ON)
    n = names(trace)
    assert [ln for ln in trace if ln.startswith(SETTER)] == [SETTER + " on=1"]
    assert n.index(SETTER) < n.index("pt_render")
    assert [ln for ln in trace if not ln.startswith(SETTER)] == run(libs, driver, "plain", {"SHADING": "gl"})
    # with the filter: the SHADING=gl trace plus the feature and filter calls -- k = 1 (a pass of 16 paths) where it was 0
    trace = run(libs, driver, "feat", dict(GL_ON, ATROUS="1"))
    n = names(trace)
    assert n.count(SETTER) == 1 and n.index(SETTER) < n.index("pt_render") < n.index("pt_atrous")
    assert "pt_set_features k=1" in trace and n.count("pt_set_features") == 1
    off = run(libs, driver, "plain", {"SHADING": "gl", "ATROUS": "1"})  # (the library refuses that frame's filter; the hosts' calls are these)
    assert "pt_set_features k=0" in off
    assert [ln for ln in trace if not ln.startswith(SETTER)] == [ln.replace("pt_set_features k=0", "pt_set_features k=1") for ln in off]
    plain_gl = run(libs, driver, "plain", {"SHADING": "gl"})
    assert set(n) - set(names(plain_gl)) <= {SETTER, "pt_atrous", "pt_set_features", "pt_set_moments", "pt_noise_estimate", "pt_set_halves"}, set(n) - set(names(plain_gl))
    # features said outright: passes, as given
    trace = run(libs, driver, "feat", dict(GL_ON, FEATURES="3"))
    assert "pt_set_features k=3" in trace and names(trace).count(SETTER) == 1
    # two frames on one context: said when it changes, not again
    twice = run(libs, driver, "feat", GL_ON, "twice")
    assert names(twice).count(SETTER) == 1 and sum(ln.startswith("pt_render cfg{") for ln in twice) == 2


@pytest.mark.parametrize("driver", ["py", "host"])
def test_the_filtered_noise_target_reaches_a_gl_frame_only_with_the_switch(libs, driver):
    env = {"SHADING": "gl", "ATROUS": "1", "FILTERED_NOISE": "0.05"}
    r, trace = child(libs, driver, "feat", env, "expect-error")
    assert "not available with GL shading" in (r.stdout + r.stderr) and "pt_begin" not in names(trace)
    trace = run(libs, driver, "feat", dict(env, SHADING_FEATURES="1"))
    n = names(trace)
    assert n.count(SETTER) == 1 and "pt_set_halves on=1" in trace and "pt_atrous_halves" in n and n.index(SETTER) < n.index("pt_begin")


@pytest.mark.parametrize("driver", ["py", "host"])
def test_with_the_variable_unset_the_calls_are_what_they_were(libs, driver):
    for env in ({}, {"SHADING": "gl"}, {"ATROUS": "1"}, {"SHADING": "gl", "ATROUS": "1"}, {"FEATURES": "3"}, {"SHADING_FEATURES": "0"},
                {"SHADING": "gl", "SHADING_FEATURES": "features"}):
        with_symbol = run(libs, driver, "feat", env)
        assert with_symbol == run(libs, driver, "plain", {k: v for k, v in env.items() if k != "SHADING_FEATURES"}), env
        assert SETTER not in names(with_symbol), env


def test_the_recorded_host_traces_stand():
    """The traces against tests/fake_ptcore.c recorded in tests/golden/host_traces.json name no entry point of this change."""
    golden = open(hts.GOLDEN).read()
    assert SETTER not in golden and "SHADING_FEATURES" not in golden


def test_a_library_without_the_entry_point_is_refused_by_name(libs):
    r, trace = child(libs, "host", "plain", {"SHADING_FEATURES": "1"}, "expect-error")
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "shading features: libptcore.so lacks pt_set_shading_features" in r.stdout
    assert not any(ln.startswith(("pt_render", "pt_begin")) for ln in trace)  # nothing was rendered
    r, trace = child(libs, "py", "plain", {"SHADING_FEATURES": "1"})
    assert r.returncode != 0 and "shading features: libptcore.so lacks pt_set_shading_features" in r.stderr
    assert not any(ln.startswith(("pt_render", "pt_begin")) for ln in trace)


def cli(libs, lib, *args, env=None):
    log = os.path.join(libs["tmp"], "cli_%d.log" % len(os.listdir(libs["tmp"])))
    e = {k: v for k, v in os.environ.items() if not k.startswith(("PATHTRACER_", "PTCORE_", "PTFAKE_"))}
    e.update({E + k: v for k, v in (env or {}).items()}, PTCORE_LIB=libs[lib], PTFAKE_LOG=log, PTFAKE_SCRIPT="")
    cmd = [os.path.join(ROOT, "path_trace_golang_amd", "render"), "-headless", "-gpu", "-scene", hts.SIMPLE, "-width", "8", "-height", "8", "-depth", "3",
           "-spp", "16", "-out", log + ".png", *args]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, env=e, timeout=120)
    return r.returncode, r.stderr, open(log).read().split("\n")[:-1] if os.path.exists(log) else []


def test_the_cli_flag_is_one_row_and_reaches_the_engine(libs):
    for args, env, want in ((["-shading", "gl", "-shading-features"], None, True), (["--shading-features=true"], None, True),
                            ([], {"SHADING_FEATURES": "1"}, True), (["-shading-features=false"], {"SHADING_FEATURES": "1"}, False),
                            (["-shading", "gl"], None, False), ([], None, False)):
        code, err, trace = cli(libs, "feat", *args, env=env)
        assert code == 0, err
        assert [ln for ln in trace if ln.startswith(SETTER)] == ([SETTER + " on=1"] if want else []), (args, env)
    code, err, trace = cli(libs, "feat", "-shading", "gl", "-shading-features", "-atrous")
    assert code == 0 and "pt_set_features k=1" in trace and "pt_atrous" in names(trace), err
    code, err, trace = cli(libs, "feat", "-shading-features=maybe")  # a bad value is a flag error
    assert code == 2 and not trace and "invalid boolean value" in err
    code, err, trace = cli(libs, "plain", "-shading-features")  # an older library: refused by name, nothing rendered
    assert code == 1 and "shading features: libptcore.so lacks pt_set_shading_features" in err and "pt_render" not in names(trace)
    assert cli(libs, "feat", "-shading", "gl")[2] == cli(libs, "plain", "-shading", "gl")[2]  # unset, the CLI says what it said before
    main = open(os.path.join(CSRC, "host", "render_main.cpp")).read()
    assert '{"shading-features", BOOL, &f.shading_features}' in main and "PATHTRACER_GPU_SHADING_FEATURES" in main


def test_the_host_layers_name_the_setting():
    host = os.path.join(CSRC, "host")
    hpp = open(os.path.join(host, "engine.hpp")).read()
    cpp = open(os.path.join(host, "engine.cpp")).read()
    assert "void SetShadingFeatures(bool on);" in hpp and "bool ShadingFeatures();" in hpp and "bool ShadingFeaturesFromEnv();" in hpp
    for name in ("OPTIONAL(pt_set_shading_features)", "PATHTRACER_GPU_SHADING_FEATURES", "shading features: libptcore.so lacks pt_set_shading_features"):
        assert name in cpp, name
    go = open(os.path.join(ROOT, "go", "internal", "engine", "hip", "hip.go")).read()
    for name in ("C.pt_set_shading_features(", "func SetShadingFeatures(", "PATHTRACER_GPU_SHADING_FEATURES"):
        assert name in go, name
    gomain = open(os.path.join(ROOT, "go", "cmd", "render", "main.go")).read()
    assert 'flag.Bool("shading-features"' in gomain and "hip.SetShadingFeatures(" in gomain
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptcore.h")).read(), flags=re.S)
    assert set(re.findall(r"C\.(pt_\w+)", go + gomain)) <= set(re.findall(r"\b(pt_\w+)\b", header))
    for f in ("hip.py", "engine.py"):
        assert "shading_features" in open(os.path.join(ROOT, "path_trace_golang_amd", f)).read(), f


# ---------------------------------------------------------------- the child process
def _scene_doc():
    with open(os.path.join(ROOT, hts.SIMPLE)) as f:
        return json.load(f)


def _child_py(mode):
    sys.path.insert(0, ROOT)
    from path_trace_golang_amd import engine, scene

    img = np.zeros((8, 8, 4), np.uint8)
    for _ in range(2 if mode == "twice" else 1):
        try:
            engine.render_into(scene.Scene.decode(_scene_doc()), engine.RenderConfig(8, 8, 16, 3, 5), img, None)
        except ValueError as e:
            if mode != "expect-error":
                raise
            print(e)


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
    else:
        _child_host(mode)
