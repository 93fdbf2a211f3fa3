"""Displaced reprojection and the object index plane without a GPU (step 4a of csrc/pt_temporal.h, pt_set_object_ids).
The reference of the model is temporal_motion_support.Restatement, plain Python floats written from the header comment; the host
build of the product's header is held against it bit for bit.  The ids' reference is tests/object_ids_reference.c on the oracle."""
from __future__ import annotations

import copy
import ctypes as C
import inspect
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import atrous_support as at
import denoise_probe_support as dp
import temporal_clip_support as tc
import temporal_motion_support as tm
import temporal_support as ts
from conftest import scene_path
from fog_support import CSRC, CXXFLAGS, ROOT, ptr

ENTRY_POINTS = ("pt_set_object_ids", "pt_read_object_ids", "pt_temporal_set_motion", "pt_temporal_motion_stats")


# ---------------------------------------------------------------- 1. the model
SEQUENCES = [("example_simple", (40, 24), 0.0), ("example_simple", (37, 21), 1.0), ("metal_glass_room", (40, 24), 1.0),
             ("metal_glass_room", (37, 21), 0.0)]


@pytest.mark.parametrize("gamma", [0.0, tm.GAMMA])
@pytest.mark.parametrize("name,size,cam", SEQUENCES, ids=["%s %dx%d cam %g" % (n, s[0], s[1], c) for n, s, c in SEQUENCES])
def test_host_build_equals_the_restatement_with_moved_objects(name, size, cam, gamma, oracle):
    """Four frames, one sphere and one box moved per frame, in two of the four sequences the camera as well: output, stored
    history, len, placement and every count of the host build against the Python restatement."""
    frames = tm.sequence(name, 4, *size, cam=cam)
    got = tm.run_sequence("host", frames, None, gamma)
    want = tm.restate_sequence(frames, gamma)
    plain = tm.restate_sequence(frames, gamma, motion="none")
    for f, (a, b) in enumerate(zip(got, want)):
        tm.assert_same_model(a, b, (name, size, cam, gamma, f))
    moved = np.isin(frames[-1]["ids"], list(tm.MOVES[name]))
    assert moved.sum() > 8 and want[-1]["moved"] > 8 and 0 < want[-1]["moved_reprojected"] <= want[-1]["moved"]
    assert want[0]["moved"] == 0  # the first frame has no table
    # the table does something, and only on the moved objects' pixels
    differs = ~(np.isclose(want[-1]["place"], plain[-1]["place"], rtol=0, atol=0, equal_nan=True).all(axis=2))
    assert differs.any() and not (differs & ~moved).any()
    print(name, size, cam, gamma, [(o["moved"], o["moved_reprojected"], o["reprojected"]) for o in want])


def test_the_displaced_placement_is_where_the_object_was():
    """An unmoved camera and a pixel well inside a moved object: the displaced placement lies the object's image-space move away
    from the pixel, the undisplaced one on the pixel itself."""
    name, (w, h) = "example_simple", (40, 24)
    frames = tm.sequence(name, 2, w, h)
    a = tm.restate_sequence(frames)[-1]["place"]
    b = tm.restate_sequence(frames, motion="none")[-1]["place"]
    ids0, ids1 = frames[0]["ids"], frames[1]["ids"]
    ys, xs = np.nonzero((ids1 == 6) & (ids0 == 6))
    assert len(ys) > 4
    for y, x in zip(ys, xs):
        assert abs(b[y, x, 0] - x) < 1e-6 and abs(b[y, x, 1] - y) < 1e-6
        assert -1.5 < a[y, x, 0] - x < -0.05 and abs(a[y, x, 1] - y) < 0.2  # +x in the scene is +x in this view: it came from the left


# ---------------------------------------------------------------- 2. table and reset
@pytest.mark.parametrize("flt", [None, dict()], ids=["no filter", "filter"])
def test_a_zero_table_is_no_table_bit_for_bit(flt, oracle):
    frames = tm.sequence("example_simple", 3, 37, 21)
    for gamma in (0.0, tm.GAMMA):
        zero = tm.run_sequence("host", frames, flt, gamma, motion="zero")
        none = tm.run_sequence("host", frames, flt, gamma, motion="none")
        for f, (a, b) in enumerate(zip(zero, none)):
            tm.assert_same_frame(a, b, (gamma, f))
            assert at.same_bits(a["place"], b["place"])
            assert a["moved"] == 0
    # ... and the shim of before the table existed gives those bits too
    old = tc.run_sequence("host", frames, flt, tm.GAMMA)
    for a, b in zip(zero, old):
        tc.assert_same_frame(a, b)


def test_a_table_on_an_empty_history_and_after_a_reset(oracle):
    """The model's side of "consumed" and of "nothing is left": with the history empty every good pixel is new whatever the table
    says (moved is counted, nothing is reprojected), and the frame after a reset is the first frame of a fresh history."""
    frames = tm.sequence("example_simple", 3, 40, 24)
    with_table = [dict(frames[1]), dict(frames[2])]  # frame 1 carries a table and meets an empty history
    got = tm.run_sequence("host", with_table, None, tm.GAMMA)
    want = tm.restate_sequence(with_table, tm.GAMMA)
    for a, b in zip(got, want):
        tm.assert_same_model(a, b)
    assert got[0]["reprojected"] == 0 and got[0]["moved"] > 0 and got[0]["moved_reprojected"] == 0
    assert at.same_bits(got[0]["mean"], tc.prep_frame(frames[1])[0])
    # reset before the third frame: it is a first frame again, with or without its table
    seq = [frames[0], frames[1], dict(frames[2], reset=True)]
    fresh = tm.run_sequence("host", [dict(frames[2], delta=None)], None, tm.GAMMA)[0]
    for motion in ("table", "none"):
        last = tm.run_sequence("host", seq, None, tm.GAMMA, motion=motion)[-1]
        for k in ("mean", "var", "hist_mean", "hist_var"):
            assert at.same_bits(last[k], fresh[k]), (motion, k)
        assert last["reprojected"] == 0 and last["moved_reprojected"] == 0


def test_ids_outside_the_table_and_misses_take_the_undisplaced_path(oracle):
    frames = tm.sequence("example_simple", 2, 37, 21)
    f1 = frames[1]
    plain = tm.run_sequence("host", frames, None, 0.0, motion="none")[-1]
    for ids in (np.full_like(f1["ids"], -1), np.full_like(f1["ids"], len(f1["delta"])), np.full_like(f1["ids"], 2 ** 31 - 1),
                np.full_like(f1["ids"], -2 ** 31)):
        got = tm.run_sequence("host", [frames[0], dict(f1, ids=ids)], None, 0.0)[-1]
        tm.assert_same_frame(got, plain)
        assert got["moved"] == 0
    # every pixel claims the moved sphere: the sky's pixels (misses) are still undisplaced
    got = tm.run_sequence("host", [frames[0], dict(f1, ids=np.full_like(f1["ids"], 6))], None, 0.0)[-1]
    want = tm.restate_sequence([frames[0], dict(f1, ids=np.full_like(f1["ids"], 6))], 0.0)[-1]
    tm.assert_same_model(got, want)
    miss = ~(f1["feats"][2][..., 1] > 0)
    assert at.same_bits(got["place"][miss], plain["place"][miss])


# ---------------------------------------------------------------- 3. object ids
IDS_SHIM = r"""
#include <cstring>
#include <vector>
#include "pt_atrous.h"
extern "C" void shim_ids(const pt_scene *sc, int64_t n, const double *rays, int32_t *ids) {
    std::vector<ptd::DevObj> objs;
    std::vector<int32_t> scene_index;  // per object of the world its index into sc->objects
    std::vector<ptd::DevMat> mats((size_t)sc->num_materials + 1);
    std::memset(mats.data(), 0, mats.size() * sizeof(ptd::DevMat));
    for (int32_t i = 0; i < sc->num_objects; i++) {
        const pt_object &o = sc->objects[i];
        ptd::DevObj d = {};
        if (o.type == PT_OBJ_SPHERE || o.type == PT_OBJ_SPHERE_LIGHT) {
            d.kind = ptd::KIND_SPHERE;
            for (int k = 0; k < 3; k++) d.a[k] = o.position[k];
            d.radius = o.size[0];
            d.radius_sq = d.radius * d.radius;
            d.inv_radius = 1.0 / d.radius;
        } else if (o.type == PT_OBJ_PLANE) {
            d.kind = ptd::KIND_PLANE;
            for (int k = 0; k < 3; k++) d.a[k] = o.position[k];
            d.b[1] = 1;
        } else if (o.type == PT_OBJ_BOX) {
            d.kind = ptd::KIND_BOX;
            for (int k = 0; k < 3; k++) { d.a[k] = o.position[k] - o.size[k] * 0.5; d.b[k] = o.position[k] + o.size[k] * 0.5; }
        } else {
            continue;
        }
        d.mat = (o.material >= 0 && o.material < sc->num_materials) ? o.material : sc->num_materials;
        objs.push_back(d);
        scene_index.push_back(i);
    }
    for (int64_t i = 0; i < n; i++) {
        double nn[3], a[3], dist;
        int32_t best = -7;
        const bool hit = pta::first_hit(objs.data(), mats.data(), (int32_t)objs.size(), rays + 6 * i, rays + 6 * i + 3, nn, a, dist, &best);
        ids[i] = hit ? scene_index[(size_t)best] : (best == -1 ? -1 : -7);
    }
}
"""


def _ids_shim():
    d = at._build_dir()
    src, out = os.path.join(d, "ids_shim.cpp"), os.path.join(d, "libidsshim.so")
    if not os.path.exists(out):
        with open(src, "w") as f:
            f.write(IDS_SHIM)
        subprocess.run(["g++", *CXXFLAGS, "-shared", "-I", CSRC, src, "-o", out], check=True, capture_output=True)
    L = C.CDLL(out)
    L.shim_ids.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    return L


@pytest.mark.parametrize("name", ["example_simple", "metal_glass_room", "unknown in the middle"])
def test_first_hit_index_of_the_host_build_equals_the_oracle(name, oracle):
    from path_trace_golang_amd import hip, scene

    w, h, seed = 40, 24, 3
    doc = tm.doc_with_an_unknown_object("example_simple") if name == "unknown in the middle" else json.load(open(scene_path(name)))
    osc = oracle.Scene(doc)
    flat = hip.FlatScene(scene.Scene.decode(doc))
    rays = np.array([sum(oracle.primary_ray(osc, w, h, 1, 1, seed, x, y, 0), []) for y in range(h) for x in range(w)])
    want, tie = tm.oracle_ids_of_rays(osc, rays)
    frame_ids, frame_tie = tm.oracle_ids(osc, w, h, seed)
    assert np.array_equal(frame_ids.reshape(-1), want) and np.array_equal(frame_tie.reshape(-1), tie)
    got = np.full(len(rays), -9, np.int32)
    _ids_shim().shim_ids(C.byref(flat.c), len(rays), ptr(rays), ptr(got))
    assert not tie.any()
    assert np.array_equal(got, want), int(np.count_nonzero(got != want))
    assert len(set(want.tolist())) > 5
    if name == "unknown in the middle":
        assert 5 not in set(want.tolist()) and max(want) > 5  # the ghost is never hit and the objects behind it keep their scene index
        plain, _ = tm.oracle_ids(oracle.Scene(json.load(open(scene_path("example_simple")))), w, h, seed)
        assert np.array_equal(np.where(plain >= 5, plain + 1, plain), frame_ids)


def test_first_hit_keeps_its_old_argument_list():
    """The shims of before the out-parameter call first_hit with eight arguments and must build unedited."""
    assert "first_hit(objs.data(), mats.data(), (int32_t)objs.size(), rays + 6 * i, rays + 6 * i + 3, nn, a, dist))" in at.SHIM
    at.product_host()
    assert "displacement" not in ts.SHIM and "ndelta" not in open(dp.SOURCE).read() and "ndelta" not in open(tc.PROBE_SOURCE).read()
    ts.product_host()
    tc.product_host()


# ---------------------------------------------------------------- 4. hip.scene_motion
def _scene(doc):
    from path_trace_golang_amd import scene

    return scene.Scene.decode(doc)


def test_scene_motion_gives_the_deltas_of_a_position_only_edit():
    from path_trace_golang_amd import hip

    a = tm.motion_doc("example_simple", 0)
    b = tm.motion_doc("example_simple", 1, cam=1.0)  # two objects and the camera moved
    d = hip.scene_motion(_scene(a), _scene(b))
    assert d.shape == (19, 3) and np.array_equal(d, tm.doc_delta(a, b))
    assert np.count_nonzero(d.any(axis=1)) == 2 and d[6, 0] != 0 and d[9, 0] != 0
    z = hip.scene_motion(_scene(a), _scene(a))
    assert z.shape == (19, 3) and not z.any()
    assert np.array_equal(hip.scene_motion(hip.FlatScene(_scene(a)), hip.FlatScene(_scene(b))), d)


def _edits():
    def count(d): d["objects"].pop()
    def order(d): d["objects"][6], d["objects"][7] = d["objects"][7], d["objects"][6]
    def typ(d): d["objects"][9]["type"] = "sphere"
    def size(d): d["objects"][6]["size"]["x"] = 1.25
    def material_id(d): d["objects"][6]["material_id"] = d["objects"][7]["material_id"]
    def material_table(d): d["materials"][0]["albedo"]["r"] = 0.123
    def material_count(d): d["materials"].append(dict(d["materials"][0], id="one-more"))
    def sky(d): d["sky"] = {"type": "solid", "color": {"r": 0.1, "g": 0.2, "b": 0.3}}
    def background(d): d["background"] = {"r": 0.5, "g": 0.25, "b": 0.125}
    return [count, order, typ, size, material_id, material_table, material_count, sky, background]


@pytest.mark.parametrize("edit", _edits(), ids=[e.__name__ for e in _edits()])
def test_scene_motion_is_none_for_every_other_edit(edit):
    from path_trace_golang_amd import hip

    a = tm.motion_doc("example_simple", 0)
    b = tm.motion_doc("example_simple", 1)
    edit(b)
    assert hip.scene_motion(_scene(a), _scene(b)) is None


def test_scene_motion_is_none_for_a_fog_edit():
    from path_trace_golang_amd import hip

    a = json.load(open(scene_path("test_scene")))
    b = copy.deepcopy(a)
    assert hip.scene_motion(_scene(a), _scene(b)) is not None
    b["fog"]["density"] = float(b["fog"].get("density", 0.0)) + 0.01
    assert hip.scene_motion(_scene(a), _scene(b)) is None
    c = copy.deepcopy(a)
    del c["fog"]
    assert hip.scene_motion(_scene(a), _scene(c)) is None
    # a FlatScene keeps the fog block of the scene it was made from: the answers are the same
    fa, fb, fc = (hip.FlatScene(_scene(d)) for d in (a, b, c))
    assert hip.scene_motion(fa, hip.FlatScene(_scene(a))) is not None
    assert hip.scene_motion(fa, fb) is None and hip.scene_motion(fa, fc) is None and hip.scene_motion(fa, _scene(b)) is None


def test_render_says_object_ids_only_when_they_change_whoever_said_them_last():
    """hip.set_object_ids and hip.render share one record of what the context was told: ids turned on by hand are turned off by a
    render that does not ask for them, and a render that asks again says so again.  Against the recording stand-in."""
    import test_host_motion_cpu as hm

    code = (
        "import sys, numpy as np\n"
        "sys.path.insert(0, %r)\n"
        "from path_trace_golang_amd import capi, hip, scene\n"
        "sc = scene.load(%r)\n"
        "img = np.zeros((8, 8, 4), np.uint8)\n"
        "with capi.Context(ndev=1) as ctx:\n"
        "    hip.render(sc, hip.RenderConfig(8, 8, 2, 2, 1), img, ctx=ctx)\n"
        "    hip.set_object_ids(ctx, True)\n"
        "    hip.render(sc, hip.RenderConfig(8, 8, 2, 2, 1), img, ctx=ctx)\n"
        "    hip.render(sc, hip.RenderConfig(8, 8, 2, 2, 1), img, ctx=ctx, features=2, object_ids=True)\n"
        "    hip.render(sc, hip.RenderConfig(8, 8, 2, 2, 1), img, ctx=ctx, features=2, object_ids=True)\n"
        "    hip.set_object_ids(ctx, False)\n"
        "    hip.render(sc, hip.RenderConfig(8, 8, 2, 2, 1), img, ctx=ctx)\n" % (ROOT, os.path.join(ROOT, hm.hts.SIMPLE)))
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        lib, log = os.path.join(tmp, "libptfake_motion.so"), os.path.join(tmp, "log")
        subprocess.run(["gcc", "-std=c11", "-O1", "-fPIC", "-shared", "-Wno-unused-function", "-Wno-unused-variable",
                        os.path.join(ROOT, "tests", "fake_ptcore_motion.c"), "-o", lib], check=True)
        env = {k: v for k, v in os.environ.items() if not k.startswith(("PATHTRACER_", "PTCORE_", "PTFAKE_"))}
        env.update(PTCORE_LIB=lib, PTFAKE_LOG=log, PTFAKE_SCRIPT="")
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0, (r.stdout, r.stderr)
        trace = [ln for ln in open(log).read().split("\n") if ln.startswith(("pt_set_object_ids", "pt_render cfg"))]
    kinds = [ln.split()[0] + (ln.split()[1][2:] if ln.startswith("pt_set") else "") for ln in trace]
    #        frame 1      by hand                 frame 2 turns them off               frame 3 on                          frame 4      by hand              frame 5
    assert kinds == ["pt_render", "pt_set_object_ids=1", "pt_set_object_ids=0", "pt_render", "pt_set_object_ids=1", "pt_render", "pt_render",
                     "pt_set_object_ids=0", "pt_render"], trace


# ---------------------------------------------------------------- 5. the surface
def test_entry_points_are_declared_exported_and_bound():
    from path_trace_golang_amd import build, capi

    build.build_core()
    lib = capi.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptcore.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pt_[a-z_0-9]+)\s*\(", text))
    bound = {name for name, _, _ in capi.SYMBOLS}
    for sym in ENTRY_POINTS:
        assert sym in declared, sym
        assert hasattr(lib, sym), sym
        assert sym in bound and capi.has(sym) and sym in capi.ADDITIVE, sym
    assert re.search(r"struct\s+pt_temporal_motion_stats\s*\{", text)
    assert lib.pt_abi_version() == 4  # additive: the version stays


def test_null_and_bad_arguments_are_refused_with_a_message():
    from path_trace_golang_amd import capi, hip

    lib = capi.load()
    st = capi.PtTemporalMotionStats()
    ids = np.zeros(4, np.int32)
    d = np.zeros(3)
    for call in (lambda: lib.pt_set_object_ids(None, 1), lambda: lib.pt_read_object_ids(None, ids.ctypes.data_as(C.POINTER(C.c_int32))),
                 lambda: lib.pt_temporal_set_motion(None, d.ctypes.data_as(C.POINTER(C.c_double)), 1),
                 lambda: lib.pt_temporal_motion_stats(None, C.byref(st))):
        assert call() == capi.PT_ERR_INVALID
        assert lib.pt_last_error()
    with pytest.raises(ValueError):
        hip.render(None, hip.RenderConfig(4, 4, 2, 2, 1), np.zeros((4, 4, 4), np.uint8), temporal_motion=np.zeros((1, 3)))  # without temporal=
    for fn in (hip.render,):
        p = inspect.signature(fn).parameters
        assert p["object_ids"].default is False and p["temporal_motion"].default is None


def test_struct_layout_in_c99_and_in_ctypes(tmp_path):
    from path_trace_golang_amd import build, capi

    lib = build.build_core()
    S = capi.PtTemporalMotionStats
    assert C.sizeof(S) == 24
    assert C.sizeof(capi.PtTemporalConfig) == 40 and C.sizeof(capi.PtTemporalStats) == 72 and C.sizeof(capi.PtTemporalClipStats) == 24
    src = tmp_path / "consumer.c"
    src.write_text(r'''
#include <stddef.h>
#include <stdio.h>
#include "ptcore.h"
int main(void) {
    struct pt_temporal_motion_stats s;
    double nan_row[3] = {0.0, 0.0, 0.0};
    int rc = pt_temporal_set_motion(0, nan_row, 1) + 10 * pt_temporal_motion_stats(0, &s) + 100 * pt_set_object_ids(0, 1) +
             1000 * pt_read_object_ids(0, 0);
    printf("%d %d %d %d\n", (int)sizeof s, (int)offsetof(struct pt_temporal_motion_stats, objects),
           (int)offsetof(struct pt_temporal_motion_stats, moved), (int)offsetof(struct pt_temporal_motion_stats, moved_reprojected));
    printf("%d\n", rc);
    return 0;
}
''')
    exe = tmp_path / "consumer"
    libdir = os.path.dirname(lib)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe), "-L", libdir, "-lptcore", "-Wl,-rpath," + libdir], check=True)
    lines = [[int(x) for x in l.split()] for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert lines[0] == [24] + [getattr(S, n).offset for n in ("objects", "moved", "moved_reprojected")]
    assert lines[0] == [24, 0, 8, 16]
    assert lines[1] == [1111 * capi.PT_ERR_INVALID]
    cpp = tmp_path / "consumer.cpp"
    cpp.write_text('#include "ptcore.h"\nint main() { struct pt_temporal_motion_stats s; return pt_temporal_motion_stats(nullptr, &s) == 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(cpp), "-o", str(tmp_path / "cpp"),
                    "-L", libdir, "-lptcore", "-Wl,-rpath," + libdir], check=True)


def test_the_probe_compiles_and_includes_the_product_headers_unchanged():
    src = open(tm.PROBE_SOURCE).read()
    assert '#include "pt_filter_launch.h"' in src and '#include "pt_kernels.h"' in src
    for name in ("ptk::temporal_kernel", "ptk::TemporalArgs", "ptl::filter_sequence", "ptl::temporal_figures", "TA.ids", "TA.delta", "TA.ndelta"):
        assert name in src, name
    assert "asm" not in re.sub(r"//.*", "", src)
    tm.compile_probe()


# ---------------------------------------------------------------- 6. quality, from oracle samples only
QUALITY_MOVES = {6: (0.08, 0.0, 0.0), 9: (0.08, 0.0, 0.0)}  # the rough-metal sphere and the red box, about half a pixel per frame at 80 x 45


@pytest.mark.parametrize("seed0", [100, 200, 300])
def test_displaced_history_beats_unknown_motion_and_a_reset(seed0, oracle):
    """DESIGN 3.13b's set-up: example_simple, depth 4, 80 x 45, six frames of 16 spp (seeds seed0 + f), objects 6 and 9 moved +0.08 in
    x per frame, default pt_temporal and filter configurations, the clip at 2.5; relative MSE of the last frame against a 1024-spp
    oracle frame of the last scene (seed 999).  On the pixels whose id is a moved object the displaced history must beat both the
    history that knows nothing of the motion and the reset frame; on the whole frame it must not lose to either.  (Measured, seeds
    100 / 200 / 300, moved pixels: displaced 0.121 / 0.143 / 0.106, unknown 0.298 / 0.355 / 0.306, reset 0.144 / 0.215 / 0.139.)"""
    w, h = 80, 45
    frames = tm.sequence("example_simple", 6, w, h, seed0=seed0, moves=QUALITY_MOVES)
    last = frames[-1]
    truth = oracle.render(oracle.Scene(last["doc"]), w, h, 1024, 4, seed=999, want=("accum",))["accum"] / 1024.0
    moved = np.isin(last["ids"], list(QUALITY_MOVES))
    den = np.maximum(truth.sum(axis=2) / 3.0, 0.01)

    def errors(res):
        e = ((res["mean"] - truth) ** 2).mean(axis=2) / (den * den)  # atrous_support.relative_mse's terms
        assert abs(float(e.mean()) - at.relative_mse(res["mean"], truth)) < 1e-15
        return float(e.mean()), float(e[moved].mean()), float(e[~moved].mean())

    reset = errors(tm.run_sequence("host", [dict(last, delta=None)], dict(), tm.GAMMA)[-1])
    unknown_run = tm.run_sequence("host", frames, dict(), tm.GAMMA, motion="none")[-1]
    displaced_run = tm.run_sequence("host", frames, dict(), tm.GAMMA)[-1]
    unknown, displaced = errors(unknown_run), errors(displaced_run)
    for label, e in (("reset", reset), ("unknown", unknown), ("displaced", displaced)):
        print("| %d | %s | %.4f | %.3f | %.4f |" % (seed0, label, *e))
    assert 60 < moved.sum() < 120 and displaced_run["moved"] == moved.sum() and displaced_run["moved_reprojected"] > moved.sum() // 2
    assert unknown_run["reprojected"] > w * h * 3 // 4  # the tap tests do not notice a half-pixel move: the wrong history is accepted
    assert displaced[1] < unknown[1] and displaced[1] < reset[1], (displaced, unknown, reset)
    assert displaced[0] <= unknown[0] and displaced[0] <= reset[0], (displaced, unknown, reset)
