"""The host rule of adaptive sampling by the filtered frame's pooled noise, call by call: engine.render_into (Python)
and engine::RenderInto (libpthost.so) render a frame in a child process against tests/fake_ptcore_filtered.c -- the recording
stand-in of the host-trace tests with the two new entry points beside it -- and the log must show the rule: an adaptive frame
with the rule's target, the filter's configuration and the pool handed to pt_set_adaptive_filtered in front of the frame, the
figures read after it, pt_atrous as the finish; and, with PATHTRACER_GPU_FILTERED_ADAPTIVE unset, exactly the calls the plain
stand-in records."""
import json
import os
import shutil
import subprocess
import sys

import pytest

import host_trace_support as hts

ROOT = hts.ROOT
E = "PATHTRACER_GPU_"
RULE_ENV = {"ATROUS": "1", "ATROUS_ITERS": "4", "FILTERED_ADAPTIVE": "0.05", "POOL": "2", "NOISE_STEP": "8", "ADAPTIVE_MIN_SPP": "6"}


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    from path_trace_golang_amd import build

    build.build_host()
    tmp = str(tmp_path_factory.mktemp("host_filtered"))
    cc = os.environ.get("CC") or shutil.which("gcc") or "cc"
    out = {"tmp": tmp}
    for name, src in (("filtered", "fake_ptcore_filtered.c"), ("plain", "fake_ptcore.c")):
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


@pytest.mark.parametrize("mode", ["", "progress"])
@pytest.mark.parametrize("driver", ["py", "host"])
def test_the_rule_call_by_call(libs, driver, mode):
    trace = run(libs, driver, "filtered", RULE_ENV, mode)
    n = names(trace)
    # an adaptive frame with the rule's target, the noise step and the adaptive min_spp
    assert [ln for ln in trace if ln.startswith("pt_set_adaptive ")] == ["pt_set_adaptive adaptive{target=0.05 min_spp=6 step=8}"]
    # the filter's configuration and the pool
    assert [ln for ln in trace if ln.startswith("pt_set_adaptive_filtered")] == [
        "pt_set_adaptive_filtered filter={iters=4 reserved=0 sigma_l=4 sigma_n=0.1 sigma_z=0.1 sigma_a=0.2} pool=2 reserved=0"]
    frame = "pt_begin" if mode else "pt_render"
    assert sum(ln.startswith(frame + " cfg{") for ln in trace) == 1 and ("pt_render" if mode else "pt_begin") not in n
    assert "spp=16" in [ln for ln in trace if ln.startswith(frame + " cfg{")][0]  # the cap
    assert n.index("pt_set_adaptive") < n.index(frame) and n.index("pt_set_adaptive_filtered") < n.index(frame)
    if mode:  # steps of 8 up to the cap of 16, clipped; the blocks stop inside pt_step
        assert [ln for ln in trace if ln.startswith("pt_step")] == ["pt_step nspp=8 -> OK done=8", "pt_step nspp=8 -> OK done=16"]
    # no other stop rule runs beside it, and the half sums are the frame's own business
    assert "pt_atrous_halves" not in n and "pt_set_halves on=1" not in trace
    # after the frame: the block table, the figures, and pt_atrous as the finish
    end = len(n) - 1 - n[::-1].index("pt_step") if mode else n.index(frame)  # (the table is readable in the open frame too)
    for after in ("pt_adaptive_state", "pt_read_block_figures", "pt_atrous"):
        assert n.count(after) == 1 and n.index(after) > end, after
    assert [ln for ln in trace if ln.startswith("pt_atrous ")][0].startswith("pt_atrous cfg={iters=4 ")


@pytest.mark.parametrize("driver", ["py", "host"])
def test_with_the_variable_unset_the_calls_are_what_they_were(libs, driver):
    for env in ({}, {"ATROUS": "1"}, {"ATROUS": "1", "NOISE": "0.1", "ADAPTIVE": "1"}, {"ATROUS": "1", "FILTERED_NOISE": "0.1"},
                {"ATROUS": "1", "POOL": "3"}):
        with_symbols = run(libs, driver, "filtered", env)
        assert with_symbols == run(libs, driver, "plain", env), env
        assert not any(x in ("pt_set_adaptive_filtered", "pt_read_block_figures") for x in names(with_symbols))
    # ... and the variable is read only with the filter on
    assert run(libs, driver, "filtered", {"FILTERED_ADAPTIVE": "0.05", "POOL": "2"}) == run(libs, driver, "plain", {})


def test_the_pool_defaults_to_one_block_and_a_bad_value_counts_as_unset(libs):
    for driver in ("py", "host"):
        for pool in (None, "7", "x"):
            env = dict(RULE_ENV)
            env.pop("POOL")
            if pool is not None:
                env["POOL"] = pool
            trace = run(libs, driver, "filtered", env)
            assert [ln.split(" pool=")[1] for ln in trace if ln.startswith("pt_set_adaptive_filtered")] == ["1 reserved=0"], (driver, pool)


def test_one_stop_rule_per_frame_in_the_host_layer(libs):
    """engine::hip::Render refuses the rule beside a frame noise target and beside the filtered noise target, before any frame."""
    for extra in ({"NOISE": "0.1"}, {"FILTERED_NOISE": "0.1"}):
        r, trace = child(libs, "host", "filtered", dict(RULE_ENV, **extra), "expect-error")
        assert r.returncode == 0, (r.stdout, r.stderr)
        assert "filtered adaptive target: excludes a frame noise target" in r.stdout and "one stop rule per frame" in r.stdout
        assert not any(ln.startswith(("pt_render", "pt_begin")) for ln in trace)
    r, trace = child(libs, "host", "filtered", dict(RULE_ENV, SHADING="gl"), "expect-error")
    assert "filtered adaptive target: not available with GL shading" in r.stdout


def test_the_python_layer_refuses_the_same_combinations(libs):
    """engine.render_into beside PATHTRACER_GPU_NOISE or PATHTRACER_GPU_FILTERED_NOISE: the refusal of the other host layers, not silence."""
    for extra in ({"NOISE": "0.1"}, {"FILTERED_NOISE": "0.1"}):
        r, trace = child(libs, "py", "filtered", dict(RULE_ENV, **extra))
        assert r.returncode != 0 and "one stop rule per frame" in r.stderr, (extra, r.stderr)
        assert not any(ln.startswith(("pt_render", "pt_begin")) for ln in trace)


def cli(libs, lib, *args, env=None):
    """path_trace_golang_amd/render -headless -gpu on the 8 x 8 frame of the trace tests, cap 16: (exit code, stderr, the stand-in's log)."""
    log = os.path.join(libs["tmp"], "cli_%d.log" % len(os.listdir(libs["tmp"])))
    e = {k: v for k, v in os.environ.items() if not k.startswith(("PATHTRACER_", "PTCORE_", "PTFAKE_"))}
    e.update({E + k: v for k, v in (env or {}).items()}, PTCORE_LIB=libs[lib], PTFAKE_LOG=log, PTFAKE_SCRIPT="")
    cmd = [os.path.join(ROOT, "path_trace_golang_amd", "render"), "-headless", "-gpu", "-scene", hts.SIMPLE, "-width", "8", "-height", "8", "-depth", "3",
           "-spp", "16", "-out", log + ".png", *args]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, env=e, timeout=120)
    return r.returncode, r.stderr, open(log).read().split("\n")[:-1] if os.path.exists(log) else []


def test_the_cli_flags_are_one_row_each_and_reach_the_engine(libs):
    rule = ["-atrous", "-atrous-iters", "4", "-filtered-adaptive", "0.05", "-noise-step", "8", "-min-spp", "6"]
    code, err, trace = cli(libs, "filtered", *rule, "-pool", "2")
    assert code == 0, err
    assert "pt_set_adaptive adaptive{target=0.05 min_spp=6 step=8}" in trace
    assert [ln.split(" pool=")[1] for ln in trace if ln.startswith("pt_set_adaptive_filtered")] == ["2 reserved=0"]
    assert "filtered adaptive: pooled target 0.05 over 2 block(s) around" in err and "after 3 checks" in err
    # Go's flag syntax, the pool's range, and the flags over the environment
    for args, env, want in ((["--pool=0"], None, "0"), (["-pool", "9"], None, "1"), ([], None, "1"), ([], {"POOL": "3"}, "3"), (["-pool=4"], {"POOL": "3"}, "4")):
        code, err, trace = cli(libs, "filtered", *rule, *args, env=env)
        assert code == 0 and [ln.split(" pool=")[1] for ln in trace if ln.startswith("pt_set_adaptive_filtered")] == [want + " reserved=0"], (args, env)
    code, err, trace = cli(libs, "filtered", "-atrous", env={"FILTERED_ADAPTIVE": "0.07"})  # the environment alone
    assert code == 0 and any(ln.startswith("pt_set_adaptive adaptive{target=0.07 ") for ln in trace)
    code, err, trace = cli(libs, "filtered", "-atrous", "-filtered-adaptive=0", env={"FILTERED_ADAPTIVE": "0.07"})  # ... and the flag turning it off
    assert code == 0 and "pt_set_adaptive_filtered" not in names(trace)
    # bad values are flag errors, like -noise's
    for bad in (["-filtered-adaptive", "-1"], ["-filtered-adaptive=nan"], ["-pool", "x"], ["-filtered-adaptive"]):
        code, err, trace = cli(libs, "filtered", "-atrous", *bad)
        assert code == 2 and not trace, (bad, err)
    # without the filter there is nothing to measure: said, and a plain frame
    code, err, trace = cli(libs, "filtered", "-filtered-adaptive", "0.05")
    assert code == 0 and "filtered-adaptive: no -atrous given" in err and "pt_set_adaptive_filtered" not in names(trace)
    # one stop rule per frame
    for other in (["-noise", "0.1"], ["-filtered-noise", "0.1"]):
        code, err, trace = cli(libs, "filtered", *rule, *other)
        assert code == 1 and "one stop rule per frame" in err and not any(ln.startswith(("pt_render", "pt_begin")) for ln in trace), other
    # unset, the CLI says to the library what it said before
    assert cli(libs, "filtered", "-atrous")[2] == cli(libs, "plain", "-atrous")[2]
    main = open(os.path.join(ROOT, "path_trace_golang_amd", "csrc", "host", "render_main.cpp")).read()
    assert '{"filtered-adaptive", NOT_NEGATIVE, &f.filtered_adaptive}' in main and '{"pool", INT, &f.pool, 0, 4, 1}' in main


def test_a_library_without_the_entry_points_is_refused_by_name(libs):
    r, trace = child(libs, "host", "plain", RULE_ENV, "expect-error")
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "filtered adaptive target: libptcore.so lacks pt_set_adaptive_filtered / pt_read_block_figures" in r.stdout
    assert not any(ln.startswith(("pt_render", "pt_begin")) for ln in trace)  # nothing was rendered
    r, trace = child(libs, "py", "plain", RULE_ENV)
    assert r.returncode != 0 and "has no pt_set_adaptive_filtered" in r.stderr
    assert not any(ln.startswith(("pt_render", "pt_begin")) for ln in trace)


def test_the_host_layers_name_the_rule():
    host = os.path.join(ROOT, "path_trace_golang_amd", "csrc", "host")
    hpp = open(os.path.join(host, "engine.hpp")).read()
    cpp = open(os.path.join(host, "engine.cpp")).read()
    assert "SetFilteredAdaptive(" in hpp and "FilteredAdaptiveFromEnv(" in hpp
    for name in ("OPTIONAL(pt_set_adaptive_filtered)", "OPTIONAL(pt_read_block_figures)", "PATHTRACER_GPU_FILTERED_ADAPTIVE",
                 "PATHTRACER_GPU_POOL", "filtered adaptive target: libptcore.so lacks"):
        assert name in cpp, name
    go = open(os.path.join(ROOT, "go", "internal", "engine", "hip", "hip.go")).read()
    for name in ("C.pt_set_adaptive_filtered(", "C.pt_read_block_figures(", "func SetFilteredAdaptive(", "PATHTRACER_GPU_FILTERED_ADAPTIVE",
                 "PATHTRACER_GPU_POOL"):
        assert name in go, name
    for f in ("hip.py", "engine.py"):
        assert "filtered_adaptive" in open(os.path.join(ROOT, "path_trace_golang_amd", f)).read(), f
    main = open(os.path.join(host, "render_main.cpp")).read()
    assert "PATHTRACER_GPU_FILTERED_ADAPTIVE" in main and "to_filtered_adaptive" in main


# ---------------------------------------------------------------- the child process
def _scene_doc():
    with open(os.path.join(ROOT, hts.SIMPLE)) as f:
        return json.load(f)


def _child_py(mode):
    import numpy as np

    sys.path.insert(0, ROOT)
    from path_trace_golang_amd import engine, scene

    img = np.zeros((8, 8, 4), np.uint8)
    engine.render_into(scene.Scene.decode(_scene_doc()), engine.RenderConfig(8, 8, 16, 3, 5), img, (lambda: None) if mode == "progress" else None)


def _child_host(mode):
    import ctypes as C

    import numpy as np

    L = C.CDLL(os.environ.get("PTHOST_LIB") or os.path.join(ROOT, "path_trace_golang_amd", "libpthost.so"))
    L.pth_last_error.restype = C.c_char_p
    L.pth_scene_decode.restype = C.c_void_p
    L.pth_scene_decode.argtypes = [C.c_char_p]
    L.pth_scene_free.argtypes = [C.c_void_p]
    CB = C.CFUNCTYPE(None)
    L.pth_render_into.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_void_p, C.c_int32, C.c_int32,
                                  C.c_int32, C.c_void_p]
    L.pth_set_backend(1)
    h = L.pth_scene_decode(json.dumps(_scene_doc()).encode())
    assert h, L.pth_last_error()
    buf = np.zeros((8, 8, 4), np.uint8)
    cb = CB(lambda: None)
    rc = L.pth_render_into(h, 8, 8, 16, 3, 5, buf.ctypes.data_as(C.c_void_p), 8, 8, 32, C.cast(cb, C.c_void_p) if mode == "progress" else None)
    L.pth_scene_free(h)
    if mode == "expect-error":
        assert rc != 0
        print(L.pth_last_error().decode())
    else:
        assert rc == 0, L.pth_last_error()
    L.pth_shutdown()


if __name__ == "__main__":
    if sys.argv[1] == "py":
        _child_py(sys.argv[2] if len(sys.argv) > 2 else "")
    else:
        _child_host(sys.argv[2] if len(sys.argv) > 2 else "")
