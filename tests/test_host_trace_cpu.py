"""The host layer above the C ABI (engine.cpp, render_main.cpp, hip.py), call by call: every case of host_trace_support.CASES runs in a
child process against the recording stand-in for libptcore.so (tests/fake_ptcore.c) and must give exactly what
tests/golden/host_traces.json holds -- the sequence of C-ABI calls with their arguments, the error text or exception, the progress()
count and, for the CLI, the exit code and the masked stderr.  No GPU, nothing preloaded."""
import json
from concurrent.futures import ThreadPoolExecutor

import pytest

import host_trace_support as hts


@pytest.fixture(scope="module")
def golden():
    with open(hts.GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def outcomes(tmp_path_factory):
    from path_trace_golang_amd import build

    build.build_host()
    tmp = str(tmp_path_factory.mktemp("host_trace"))
    libs = hts.build_fakes(tmp)
    names = sorted(hts.CASES)
    with ThreadPoolExecutor(8) as pool:  # the children are independent processes with a log file each
        return dict(zip(names, pool.map(lambda n: hts.run_case(n, libs, tmp), names)))


def test_the_golden_file_holds_exactly_the_cases(golden):
    assert sorted(golden) == sorted(hts.CASES)


@pytest.mark.parametrize("name", sorted(hts.CASES))
def test_case_gives_the_recorded_calls_texts_and_codes(outcomes, golden, name):
    got, want = json.loads(json.dumps(outcomes[name])), golden[name]
    assert got["trace"] == want["trace"]
    assert got == want


def test_every_error_return_and_every_raise_is_reached(golden):
    """hts.REACHED names, for every `return` with a text in hip::Render and every `raise` in hip.render, the cases that reach it; the
    recorded outcome of each must carry that text (the generic `return err` entries: the name of the call that failed)."""
    for where, entries in hts.REACHED.items():
        for key, cases in entries.items():
            for c in cases.split():
                rec = golden[c]
                text = rec["error"] if where == "engine.cpp" else (rec["exception"] or ["", ""])[1]
                assert text, (key, c)
                if key == "return g_core.error":
                    assert "ABI version mismatch" in text
                elif key.startswith("return err: "):
                    assert ("GPU render error: " + key.split()[2].rstrip(":") + ": injected") == text, (key, c)
                elif key.startswith("pt_"):
                    assert text == "GPU render error: " + key.split()[0] + " injected", (key, c)
                else:
                    assert key in text, (key, c)


def test_failure_handling_keeps_pt_end_and_the_first_text(golden):
    def calls(c):
        return [ln.split()[0] for ln in golden[c]["trace"]]

    for c in ("host_fail_step2_progress", "host_fail_step2_noise", "host_fail_step2_filtered", "host_fail_read_progress", "host_fail_noise_estimate",
              "host_fail_atrous_halves", "py_fail_step2", "py_fail_read", "py_fail_noise_estimate", "py_fail_atrous_halves"):
        assert "pt_end" in calls(c), c
    for c in ("host_fail_begin_progress", "host_fail_begin_noise", "host_fail_begin_filtered", "py_fail_begin"):
        assert "pt_end" not in calls(c) and "pt_step" not in calls(c), c
    assert calls("host_progress_spp25").count("pt_step") == 13 and golden["host_progress_spp25"]["progress_calls"] == 14
    assert [ln for ln in golden["host_noise_to_cap"]["trace"] if ln.startswith("pt_step")] == [
        "pt_step nspp=16 -> OK done=16", "pt_step nspp=16 -> OK done=32", "pt_step nspp=8 -> OK done=40"]
    c = calls("host_adaptive_stall")
    assert c.index("pt_adaptive_state") < c.index("pt_read") < c.index("pt_end")
