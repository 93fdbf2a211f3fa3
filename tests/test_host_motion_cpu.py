"""The host rule of displaced reprojection, call by call: engine.render_into (Python) and engine::RenderInto
(libpthost.so) render a sequence of edits of one scene in a child process against tests/fake_ptcore_motion.c -- the recording
stand-in of the host-trace tests with the new entry points beside it -- and the log must show the rule: object ids on, a moved
scene's table passed on, an unmoved scene passing nothing, a resize resetting the history, and, with
PATHTRACER_GPU_TEMPORAL_MOTION unset, exactly the calls the plain stand-in records."""
import copy
import json
import os
import shutil
import subprocess
import sys

import pytest

import host_trace_support as hts

ROOT = hts.ROOT
E = "PATHTRACER_GPU_"


def edits():
    """Five scenes: the shipped one; objects 6 and 9 moved (and the camera); the same again; object 6 resized; object 9 moved."""
    with open(os.path.join(ROOT, hts.SIMPLE)) as f:
        base = json.load(f)
    out = [base]
    d = copy.deepcopy(base)
    d["objects"][6]["position"]["x"] += 0.125
    d["objects"][9]["position"]["z"] -= 0.25
    d["camera"]["position"]["x"] += 0.5
    out.append(d)
    out.append(copy.deepcopy(d))
    d = copy.deepcopy(d)
    d["objects"][6]["size"]["x"] = 1.5
    out.append(d)
    d = copy.deepcopy(d)
    d["objects"][9]["position"]["y"] += 0.5
    out.append(d)
    return out


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    from path_trace_golang_amd import build

    build.build_host()
    tmp = str(tmp_path_factory.mktemp("host_motion"))
    cc = os.environ.get("CC") or shutil.which("gcc") or "cc"
    out = {"tmp": tmp}
    for name, src in (("motion", "fake_ptcore_motion.c"), ("plain", "fake_ptcore.c")):
        out[name] = os.path.join(tmp, "libptfake_%s.so" % name)
        subprocess.run([cc, "-std=c11", "-O1", "-g", "-fPIC", "-shared", "-Wall", "-Wextra", "-Wno-unused-function", "-Wno-unused-variable",
                        os.path.join(ROOT, "tests", src), "-o", out[name]], check=True)
    return out


def run(libs, driver, lib, env, mode=""):
    """The five frames through `driver` ("py" or "host") in a child process: the stand-in's log, line by line."""
    log = os.path.join(libs["tmp"], "%s_%s_%d.log" % (driver, lib, len(os.listdir(libs["tmp"]))))
    e = {k: v for k, v in os.environ.items() if not k.startswith(("PATHTRACER_", "PTCORE_", "PTFAKE_"))}
    e.update({E + k: v for k, v in env.items()}, PTCORE_LIB=libs[lib], PTFAKE_LOG=log, PTFAKE_SCRIPT="")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), driver, *([mode] if mode else [])], capture_output=True, text=True, cwd=ROOT,
                       env=e, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    with open(log) as f:
        return f.read().split("\n")[:-1]


def frames_of(trace):
    """The log cut into frames: a frame ends with its pt_temporal (or pt_temporal_motion_stats, when that follows)."""
    out, cur = [], []
    for ln in trace:
        name = ln.split()[0]
        if name in ("pt_create", "pt_destroy"):
            continue
        if cur and cur[-1].split()[0] in ("pt_temporal", "pt_temporal_clip_stats", "pt_temporal_motion_stats") and name not in (
                "pt_temporal_clip_stats", "pt_temporal_motion_stats"):
            out.append(cur)
            cur = []
        cur.append(ln)
    out.append(cur)
    return out


def names(frame):
    return [ln.split()[0] for ln in frame]


MOTION_ENV = {"TEMPORAL": "1", "TEMPORAL_CLIP": "2.5", "TEMPORAL_MOTION": "1"}


@pytest.mark.parametrize("driver", ["py", "host"])
def test_the_rule_frame_by_frame(libs, driver):
    fr = frames_of(run(libs, driver, "motion", MOTION_ENV))
    assert len(fr) == 5, fr
    # object ids are turned on once, in front of the first frame, and stay on
    assert [n for f in fr for n in names(f)].count("pt_set_object_ids") == 1 and "pt_set_object_ids on=1" in fr[0]
    assert names(fr[0]).index("pt_set_object_ids") < names(fr[0]).index("pt_render")
    # frame 0: nothing to compare with; frame 1: the table, in front of pt_temporal; frame 2: nothing moved, nothing passed
    assert "pt_temporal_set_motion" not in names(fr[0]) and "pt_temporal_reset" not in names(fr[0])
    sets = [ln for ln in fr[1] if ln.startswith("pt_temporal_set_motion")]
    assert sets == ["pt_temporal_set_motion delta=set n=19 moved=[ 6:(0.125,0.000,0.000) 9:(0.000,0.000,-0.250) ]"], fr[1]
    assert names(fr[1]).index("pt_render") < names(fr[1]).index("pt_temporal_set_motion") < names(fr[1]).index("pt_temporal")
    assert "pt_temporal_reset" not in names(fr[1])
    assert "pt_temporal_set_motion" not in names(fr[2]) and "pt_temporal_reset" not in names(fr[2])
    # frame 3: a resize is not motion -- the history is reset, in front of pt_temporal, and no table goes with it
    assert names(fr[3]).count("pt_temporal_reset") == 1 and "pt_temporal_set_motion" not in names(fr[3])
    assert names(fr[3]).index("pt_temporal_reset") < names(fr[3]).index("pt_temporal")
    # frame 4: against the resized scene, only the move is left
    assert [ln for ln in fr[4] if ln.startswith("pt_temporal_set_motion")] == ["pt_temporal_set_motion delta=set n=19 moved=[ 9:(0.000,0.500,0.000) ]"]
    for k, f in enumerate(fr):  # the stats follow the frames that ran with a table
        assert (names(f)[-1] == "pt_temporal_motion_stats") == (k in (1, 4)) and names(f).count("pt_temporal_motion_stats") == (k in (1, 4))
        assert names(f).count("pt_temporal") == 1


@pytest.mark.parametrize("driver", ["py", "host"])
def test_with_the_variable_unset_the_calls_are_what_they_were(libs, driver):
    env = {"TEMPORAL": "1", "TEMPORAL_CLIP": "2.5"}
    with_symbols = run(libs, driver, "motion", env)
    plain = run(libs, driver, "plain", env)
    assert with_symbols == plain and len(frames_of(plain)) == 5
    assert not any(ln.split()[0] in ("pt_set_object_ids", "pt_temporal_set_motion", "pt_temporal_motion_stats", "pt_temporal_reset") for ln in plain)
    # ... and the variable is read only when the accumulation is on
    assert run(libs, driver, "motion", {"TEMPORAL_MOTION": "1"}) == run(libs, driver, "plain", {})


def test_a_new_context_is_told_about_object_ids_again(libs):
    """engine::hip::SetDevices between frames 1 and 2 destroys the process-wide context: the next frame runs on a new one, which must
    hear pt_set_object_ids(1) again and has no scene to compare with; the frames after it follow the rule as before."""
    trace = run(libs, "host", "motion", MOTION_ENV, mode="devices")
    called = [ln.split()[0] for ln in trace]
    assert called.count("pt_create") == 2 and called.count("pt_destroy") == 2
    second = len(called) - 1 - called[::-1].index("pt_create")
    assert [ln for ln in trace[:second] if ln.startswith("pt_set_object_ids")] == ["pt_set_object_ids on=1"]
    assert [ln for ln in trace[second:] if ln.startswith("pt_set_object_ids")] == ["pt_set_object_ids on=1"]
    after = called[second:]
    assert after.index("pt_set_object_ids") < after.index("pt_render")
    fr = frames_of(trace)
    assert len(fr) == 5
    assert "pt_temporal_set_motion" in names(fr[1])
    assert "pt_temporal_set_motion" not in names(fr[2]) and "pt_temporal_reset" not in names(fr[2])  # nothing is remembered of the old context
    assert names(fr[3]).count("pt_temporal_reset") == 1  # the resize, against the scene remembered on the new context
    assert [ln for ln in fr[4] if ln.startswith("pt_temporal_set_motion")] == ["pt_temporal_set_motion delta=set n=19 moved=[ 9:(0.000,0.500,0.000) ]"]


def test_a_library_without_the_entry_points_is_refused_by_name(libs):
    log = os.path.join(libs["tmp"], "lacks.log")
    e = {k: v for k, v in os.environ.items() if not k.startswith(("PATHTRACER_", "PTCORE_", "PTFAKE_"))}
    e.update({E + k: v for k, v in MOTION_ENV.items()}, PTCORE_LIB=libs["plain"], PTFAKE_LOG=log, PTFAKE_SCRIPT="")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "host", "expect-error"], capture_output=True, text=True, cwd=ROOT, env=e, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "temporal motion: libptcore.so lacks pt_set_object_ids / pt_temporal_set_motion" in r.stdout
    assert not any(ln.startswith(("pt_render", "pt_begin")) for ln in open(log).read().split("\n"))  # nothing was rendered


def test_the_three_host_layers_name_the_rule():
    hpp = open(os.path.join(ROOT, "path_trace_golang_amd", "csrc", "host", "engine.hpp")).read()
    cpp = open(os.path.join(ROOT, "path_trace_golang_amd", "csrc", "host", "engine.cpp")).read()
    assert "SetTemporalMotion(" in hpp and "TemporalMotionFromEnv(" in hpp
    for name in ("OPTIONAL(pt_set_object_ids)", "OPTIONAL(pt_temporal_set_motion)", "OPTIONAL(pt_temporal_motion_stats)",
                 "PATHTRACER_GPU_TEMPORAL_MOTION", "temporal motion: libptcore.so lacks"):
        assert name in cpp, name
    go = open(os.path.join(ROOT, "go", "internal", "engine", "hip", "hip.go")).read()
    for name in ("C.pt_set_object_ids(", "C.pt_temporal_set_motion(", "C.pt_temporal_motion_stats(", "C.struct_pt_temporal_motion_stats",
                 "func SetTemporalMotion(", "func sceneMotion(", "C.pt_temporal_reset(", "PATHTRACER_GPU_TEMPORAL_MOTION"):
        assert name in go, name
    py = open(os.path.join(ROOT, "path_trace_golang_amd", "hip.py")).read()
    assert "PATHTRACER_GPU_TEMPORAL_MOTION" in py


# ---------------------------------------------------------------- the child process
def _child_py():
    import numpy as np

    sys.path.insert(0, ROOT)
    from path_trace_golang_amd import engine, scene

    for f, doc in enumerate(edits()):
        img = np.zeros((8, 8, 4), np.uint8)
        engine.render_into(scene.Scene.decode(doc), engine.RenderConfig(8, 8, 4, 3, 5 + f), img)


def _child_host(mode):
    import ctypes as C

    import numpy as np

    L = C.CDLL(os.environ.get("PTHOST_LIB") or os.path.join(ROOT, "path_trace_golang_amd", "libpthost.so"))
    L.pth_last_error.restype = C.c_char_p
    L.pth_scene_decode.restype = C.c_void_p
    L.pth_scene_decode.argtypes = [C.c_char_p]
    L.pth_scene_free.argtypes = [C.c_void_p]
    L.pth_render_into.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_void_p, C.c_int32, C.c_int32,
                                  C.c_int32, C.c_void_p]
    L.pth_set_backend(1)
    for f, doc in enumerate(edits()):
        h = L.pth_scene_decode(json.dumps(doc).encode())
        assert h, L.pth_last_error()
        buf = np.zeros((8, 8, 4), np.uint8)
        rc = L.pth_render_into(h, 8, 8, 4, 3, 5 + f, buf.ctypes.data_as(C.c_void_p), 8, 8, 32, None)
        L.pth_scene_free(h)
        if mode == "devices" and f == 1:  # the context goes, and with it what was said to it
            L.pth_set_devices((C.c_int32 * 1)(0), 1)
        if mode == "expect-error":
            assert rc != 0
            print(L.pth_last_error().decode())
            break
        assert rc == 0, L.pth_last_error()
    L.pth_shutdown()


if __name__ == "__main__":
    if sys.argv[1] == "py":
        _child_py()
    else:
        _child_host(sys.argv[2] if len(sys.argv) > 2 else "")
