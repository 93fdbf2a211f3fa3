"""The roulette table (csrc/pt_convert.h: roulette_record, roulette_table; csrc/pt_kernels.h: roulette_table_advance, roulette_step):
the attenuation triples the tests run, the stand-alone host program and the device probe (tests/roulette_probe.hip), built like
shade_probe_support.py builds its own -- with the library's compiler and flags, into a temporary directory, never into the tree."""
from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

import shade_probe_support as sp
from fog_support import CSRC, ROOT, ptr

HOST_SOURCE = os.path.join(ROOT, "tests", "roulette_table_probe.cpp")
SOURCE = os.path.join(ROOT, "tests", "roulette_probe.hip")
PRODUCT = ("ptd::roulette_record", "ptd::roulette_table", "ptk::roulette_table_advance<STATS>", "ptk::roulette_step<STATS>", "ptk::stage_lds")
ENDED = -1.0           # ptd::ROULETTE_ENDED
# MWC64X's first output is x ^ c of the state (c << 32) | x: with x == c the draw is below 2^-32, under every survival probability
# (those are >= 1e-6), so a path with this state survives whatever record is not `ended`
SURVIVOR_STATE = 0x0000000500000005

_dir = None
_lib = None


def _tmp():
    global _dir
    if _dir is None:
        _dir = tempfile.mkdtemp(prefix="rrprobe_")
    return _dir


def extra_triples():
    """What the issue lists next to the probe table's own triples."""
    nan, inf, den = float("nan"), float("inf"), 5e-324
    t = [(-0.0, -0.0, -0.0), (-0.0, 0.5, 0.25), (0.5, -0.0, 0.0)]
    for v in (1e-6, 0.95):
        for w in (v, sp.down(v), sp.up(v)):
            t += [(w, w, w), (w, w / 2, w / 4), (w / 4, w / 2, w), (w / 2, w, w / 4)]
    t += [(den, den, den), (den, 0.0, 0.0), (0.5, den, 0.25), (2.5e-308, 1e-308, 5e-324)]
    t += [(inf, 0.5, 0.25), (0.5, inf, 0.25), (0.5, 0.25, inf), (inf, inf, inf), (-inf, 0.5, 0.25), (-inf, -inf, -inf)]
    t += [(nan, 0.5, 0.25), (0.5, nan, 0.25), (0.5, 0.25, nan), (nan, nan, nan), (nan, inf, 0.5), (inf, nan, 0.5), (nan, 1e-7, 1e-8)]
    return t


def triples():
    """dict(att f64 [m, 3], state u64 [m], at_prob bool [m]): every distinct (attenuation, state) the CPU test runs at depth 3 --
    the triples of sp.roulette_table() (the draw-at-probability cases with their own state: at_prob) and extra_triples(), each also
    with SURVIVOR_STATE."""
    R = sp.roulette_table()
    n_grid = len(sp.ROULETTE_DEPTHS) * 4 * (len(sp.ALBEDOS) + 7) * len(sp.ROULETTE_T) * 6   # roulette_table's loops; 150 x 3 cases follow
    assert R["n"] - n_grid in (449, 450)
    att, state, at_prob, seen = [], [], [], set()
    for i in range(R["n"]):
        own = i >= n_grid   # the draw-at-probability cases
        key = (sp.bits(R["att"][i]).tobytes(), int(R["state"][i]) if own else 0)
        if key in seen:
            continue
        seen.add(key)
        att.append(tuple(R["att"][i])); state.append(int(R["state"][i])); at_prob.append(own)
    for t in extra_triples():
        att.append(t); state.append(int(R["state"][len(att) % R["n"]])); at_prob.append(False)
    m = len(att)
    att, state, at_prob = att + att, state + [SURVIVOR_STATE] * m, at_prob + [False] * m
    return dict(att=np.array(att, np.float64), state=np.array(state, np.uint64), at_prob=np.array(at_prob))


def build_host(flags=(), name="roulette_table_probe"):
    exe = os.path.join(_tmp(), name)
    cxx = os.environ.get("CXX") or shutil.which("g++") or "g++"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fno-fast-math", *flags, "-I" + CSRC,
                    HOST_SOURCE, "-o", exe], check=True)
    return exe


def run_host(exe, att):
    """(records f64 [m, 4] = prob, q; table f64 [4, 4]: roulette_table of three materials with the first three triples as albedo)."""
    text = "".join("%016x %016x %016x\n" % tuple(int(v) for v in sp.bits(a)) for a in att)
    r = subprocess.run([exe], input=text, check=True, capture_output=True, text=True)
    assert r.stderr == "", r.stderr  # a sanitizer report goes there
    lines = r.stdout.split("\n")[:-1]
    at = lines.index("table")
    parse = lambda ls: np.array([[int(w, 16) for w in ln.split()] for ln in ls], np.uint64).view(np.float64).reshape(len(ls), 4)
    assert at == len(att)
    return parse(lines[:at]), parse(lines[at + 1:])


# ---------------------------------------------------------------- the device probe
def compile_probe() -> str:
    from path_trace_golang_amd import build

    out = os.path.join(_tmp(), "librouletteprobe.so")
    if not os.path.exists(out):
        r = subprocess.run([build.HIPCC, *build.HIP_FLAGS, "-shared", "-I", CSRC, "-I", os.path.join(ROOT, "tests"), SOURCE, "-o", out],
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("roulette probe does not compile:\n%s\n%s" % (r.stdout, r.stderr))
    return out


def load():
    """The probe, loaded after torch so that the process keeps one HIP runtime (as conftest.gpu_ctx does for libptcore.so)."""
    global _lib
    if _lib is None:
        import torch  # noqa: F401

        L = C.CDLL(compile_probe())
        vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
        L.probe_roulette_guard.restype = i64
        L.probe_roulette_guard.argtypes = []
        L.probe_roulette_records.restype = None
        L.probe_roulette_records.argtypes = [i64, vp, vp]
        L.probe_roulette_table.restype = C.c_int
        L.probe_roulette_table.argtypes = [i32, i64, vp, vp, vp, vp, vp, vp, vp]
        _lib = L
    return _lib


def gpu_table_step(depth, att, T, states, stats: bool, lds: bool, mixed: bool) -> dict:
    """probe_roulette_table over n cases.  dict(I i32 [n, 5] = finished, depth, record used, c_draw, j_draw; F f64 [n, 3] = T; S u64 [n])."""
    L = load()
    n = len(depth)
    depth, states = np.ascontiguousarray(depth, np.int32), np.ascontiguousarray(states, np.uint64)
    att, T = np.ascontiguousarray(att, np.float64), np.ascontiguousarray(T, np.float64)
    g = int(L.probe_roulette_guard())
    I, F, S = np.zeros((n + g, 5), np.int32), np.zeros((n + g, 3)), np.zeros(n + g, np.uint64)
    rc = L.probe_roulette_table(int(stats) | (int(lds) << 1) | (int(mixed) << 2), n, ptr(depth), ptr(att), ptr(T), ptr(states), ptr(I), ptr(F), ptr(S))
    if rc != 0:
        raise RuntimeError("probe_roulette_table: status %d" % rc)
    for a in (I, F, S):
        assert np.all(a[n:].view(np.uint8) == 0xFF), "guard words were written"
    return dict(I=I[:n], F=F[:n], S=S[:n])
