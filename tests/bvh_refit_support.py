"""Helpers of the BVH refit tests (test_bvh_refit_cpu.py, test_bvh_refit_probe_gpu.py, test_bvh_refit_gpu.py,
test_bvh_refit_edits_gpu.py): the device worlds and scenes the cases are made from, the moves, the edits that are no
translations (resizes for worlds, edited_scenes for scenes), tests/bvh_refit_probe.cpp as a ctypes library (the host build of
csrc/pt_bvh_refit.h and of the builder) and tests/bvh_refit_probe.hip (the product's kernels on arrays a test hands in)."""
from __future__ import annotations

import copy
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from fog_support import CSRC, CXXFLAGS, ROOT, ptr

HOST_SOURCE = os.path.join(ROOT, "tests", "bvh_refit_probe.cpp")
GPU_SOURCE = os.path.join(ROOT, "tests", "bvh_refit_probe.hip")

# ptd::DevObj (csrc/pt_device.h), 80 bytes
DEVOBJ = np.dtype([("a", "<f8", 3), ("b", "<f8", 3), ("radius", "<f8"), ("radius_sq", "<f8"), ("inv_radius", "<f8"), ("kind", "<i4"),
                   ("mat", "<i4")])
assert DEVOBJ.itemsize == 80
NODE_BYTES, OBJ_BYTES = 128, 96
KIND_SPHERE, KIND_BOX = 0, 2

SIZES = (1, 2, 5, 17, 300, 3000)
DIELECTRICS = (0, 1, 7)

_vp = C.c_void_p
_libs = {}
_dir = None
_worlds = {}


def _build_dir() -> str:
    global _dir
    if _dir is None:
        _dir = tempfile.mkdtemp(prefix="bvhrefit_")
    return _dir


# ---------------------------------------------------------------- worlds and scenes
def world_of(n: int, ndiel: int = 0, seed: int = 3) -> np.ndarray:
    """The first n spheres and boxes of synth.make_scene(max(n, 17)) as device records (the plane and the rest left out); the
    first min(ndiel, n) of every third of them made dielectric.  Computed once per (n, ndiel, seed); read-only."""
    key = (n, ndiel, seed)
    if key not in _worlds:
        from path_trace_golang_amd import synth

        sc = synth.make_scene(max(n, 17), seed)
        rows = []
        for o in sc.objects:
            if o.type == "plane" or len(rows) == n:
                continue
            r = np.zeros((), DEVOBJ)
            p = np.array([o.position.x, o.position.y, o.position.z])
            if o.type == "box":
                half = 0.5 * np.array([o.size.x, o.size.y, o.size.z])
                r["a"], r["b"], r["kind"] = p - half, p + half, KIND_BOX
            else:
                rad = float(o.size.x)
                r["a"], r["radius"], r["radius_sq"], r["inv_radius"], r["kind"] = p, rad, rad * rad, 1.0 / rad, KIND_SPHERE
            r["mat"] = len(rows) % 5
            rows.append(r)
        w = np.array(rows, DEVOBJ)
        assert len(w) == n
        for i in list(range(0, n, 3))[:ndiel]:
            w["kind"][i] |= 0x100
        w.setflags(write=False)
        _worlds[key] = w
    return _worlds[key]


def shifted(w: np.ndarray, idx, delta) -> np.ndarray:
    """A copy of world w with the objects idx moved by delta ([len(idx), 3] or [3])."""
    out = w.copy()
    idx = np.asarray(idx, np.int64)
    d = np.broadcast_to(np.asarray(delta, np.float64), (len(idx), 3))
    out["a"][idx] += d
    box = (out["kind"][idx] & 0xff) == KIND_BOX
    out["b"][idx[box]] += d[box]
    return out


def size_of(w: np.ndarray) -> np.ndarray:
    """[n] every object's size: the radius, or a box's largest half extent."""
    return np.where((w["kind"] & 0xff) == KIND_BOX, 0.5 * np.abs(w["b"] - w["a"]).max(axis=1), np.abs(w["radius"]))


def moves(w: np.ndarray, seed: int = 5):
    """The four moves of a world, in order, each applied to the result of the one before: 1 % of the objects (one at least) by half
    their size; every object by a random offset; one object far enough to double the scene bound (the margin grows); that object
    back (the margin shrinks).  Yields (name, world)."""
    rng = np.random.default_rng(seed)
    n = len(w)
    idx = rng.choice(n, max(1, n // 100), replace=False)
    d = rng.standard_normal((len(idx), 3))
    d *= (0.5 * size_of(w)[idx] / np.linalg.norm(d, axis=1))[:, None]
    w1 = shifted(w, idx, d)
    yield "one percent by half their size", w1
    w2 = shifted(w1, np.arange(n), rng.uniform(-1.0, 1.0, (n, 3)))
    yield "all by a random offset", w2
    bound = max(1.0, float(np.abs(np.concatenate([w2["a"], w2["b"]])).max()))
    far = n - 1
    w3 = shifted(w2, [far], [2.5 * bound, 0.0, 0.0])
    yield "one far away: the margin grows", w3
    w4 = shifted(w3, [far], [-2.5 * bound, 0.0, 0.0])
    yield "the far one back: the margin shrinks", w4


def with_radius(w: np.ndarray, idx, radius) -> np.ndarray:
    """A copy of world w with the spheres idx given `radius` ([len(idx)]); radius_sq and inv_radius as the scene conversion forms
    them (r * r, 1 / r: infinite for a zero radius)."""
    out = w.copy()
    idx = np.asarray(idx, np.int64)
    assert np.all((w["kind"][idx] & 0xff) == KIND_SPHERE)
    r = np.broadcast_to(np.asarray(radius, np.float64), (len(idx),))
    out["radius"][idx] = r
    out["radius_sq"][idx] = r * r
    with np.errstate(divide="ignore"):
        out["inv_radius"][idx] = 1.0 / r
    return out


def with_box_scale(w: np.ndarray, idx, factor) -> np.ndarray:
    """A copy of world w with the boxes idx scaled about their centres by factor ([3], per axis)."""
    out = w.copy()
    idx = np.asarray(idx, np.int64)
    assert np.all((w["kind"][idx] & 0xff) == KIND_BOX)
    c, half = 0.5 * (w["a"][idx] + w["b"][idx]), 0.5 * (w["b"][idx] - w["a"][idx]) * np.asarray(factor, np.float64)
    out["a"][idx], out["b"][idx] = c - half, c + half
    return out


RESIZES = ("spheres grown x1.7", "spheres shrunk x0.01", "boxes x2.5 on x, x0.2 on y", "two radii negated", "two radii zero",
           "dielectrics moved and grown x1.3", "back to the built world")
DIELECTRIC_MOVE = (0.4, 0.25, -0.3)


def resizes(w: np.ndarray):
    """The edits of a world that are no translations, each made to w itself (RESIZES, in order): every sphere grown, every sphere
    shrunk, every box stretched on x and flattened on y, two spheres given the negative of their radius, two spheres a zero radius,
    every dielectric (bit 8 of `kind`: also in the second tree) moved and grown about its centre, then w again.  Yields (name, world).
    Kinds and materials never change, so ptbvh::refit_reason accepts every step."""
    sph = np.flatnonzero((w["kind"] & 0xff) == KIND_SPHERE)
    box = np.flatnonzero((w["kind"] & 0xff) == KIND_BOX)
    yield RESIZES[0], with_radius(w, sph, w["radius"][sph] * 1.7)
    yield RESIZES[1], with_radius(w, sph, w["radius"][sph] * 0.01)
    yield RESIZES[2], with_box_scale(w, box, [2.5, 0.2, 1.0])
    two, other = sph[:2], sph[-2:]
    yield RESIZES[3], with_radius(w, two, -w["radius"][two])
    yield RESIZES[4], with_radius(w, other, [0.0, 0.0])
    die = np.flatnonzero((w["kind"] & 0x100) != 0)
    wd = shifted(w, die, DIELECTRIC_MOVE)
    ds, db = die[(w["kind"][die] & 0xff) == KIND_SPHERE], die[(w["kind"][die] & 0xff) == KIND_BOX]
    wd = with_box_scale(with_radius(wd, ds, w["radius"][ds] * 1.3), db, [1.3, 1.3, 1.3])
    yield RESIZES[5], wd
    yield RESIZES[6], w.copy()


# ---------------------------------------------------------------- the host build
def host():
    """tests/bvh_refit_probe.cpp as a shared library, built with the flags of the library's host code."""
    if "host" not in _libs:
        out = os.path.join(_build_dir(), "libbvhrefitprobe.so")
        subprocess.run(["g++", *CXXFLAGS, "-Wall", "-Wextra", "-Werror", "-shared", "-I", CSRC, HOST_SOURCE, "-o", out], check=True,
                       capture_output=True)
        L = C.CDLL(out)
        L.rp_build.restype = _vp
        L.rp_build.argtypes = [_vp, C.c_int32]
        L.rp_free.argtypes = [_vp]
        L.rp_free.restype = None
        L.rp_counts.argtypes = [_vp, _vp]
        L.rp_counts.restype = None
        L.rp_margin.argtypes = [_vp]
        L.rp_margin.restype = C.c_double
        L.rp_get.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp]
        L.rp_get.restype = None
        L.rp_get_built.argtypes = [_vp, _vp]
        L.rp_get_built.restype = None
        L.rp_refit.argtypes = [_vp, _vp, C.c_int32]
        L.rp_refit.restype = C.c_double
        L.rp_cost_of.argtypes = [_vp, C.c_int64]
        L.rp_cost_of.restype = C.c_double
        L.rp_check.argtypes = [_vp, _vp, C.c_int32, _vp]
        L.rp_check.restype = None
        L.rp_rays.argtypes = [_vp, _vp, C.c_int32, C.c_int32, C.c_uint64, _vp]
        L.rp_rays.restype = C.c_int32
        L.rp_next_up.argtypes = [C.c_uint32]
        L.rp_next_up.restype = C.c_uint32
        L.rp_round_up.argtypes = [C.c_double]
        L.rp_round_up.restype = C.c_uint32
        L.rp_encode_axis.argtypes = [C.c_double, C.c_double, C.c_double, _vp]
        L.rp_encode_axis.restype = None
        L.rp_h_word.argtypes = [C.c_uint32, C.c_uint32]
        L.rp_h_word.restype = C.c_uint32
        _libs["host"] = L
    return _libs["host"]


def standalone(flags=(), name="bvh_refit_probe") -> str:
    """The same source as a program of its own."""
    exe = os.path.join(_build_dir(), name)
    subprocess.run(["g++", *CXXFLAGS, "-g", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC, HOST_SOURCE, "-o", exe], check=True,
                   capture_output=True)
    return exe


class Tree:
    """The two trees of a world on the host: built as a render builds them, refitted by the host restatement."""

    def __init__(self, world: np.ndarray):
        self.L = host()
        w = np.ascontiguousarray(world)
        self.h = self.L.rp_build(ptr(w), len(w))
        assert self.h, "tree deeper than the traversal stack"
        c = np.zeros(6, np.int32)
        self.L.rp_counts(self.h, ptr(c))
        self.n_nodes, self.n_objs, self.n_levels, self.main_nodes, self.depth, self.main_objs = (int(v) for v in c)
        self.built = np.zeros(self.n_nodes * NODE_BYTES, np.uint8)
        self.L.rp_get_built(self.h, ptr(self.built))
        self.built.setflags(write=False)

    def close(self):
        if self.h:
            self.L.rp_free(self.h)
            self.h = None

    __del__ = close

    @property
    def margin(self) -> float:
        return float(self.L.rp_margin(self.h))

    def state(self) -> dict:
        """nodes and records as bytes, levels [n_levels + 1], box [n_nodes, 6], area [n_nodes] as they are now."""
        nodes = np.zeros(self.n_nodes * NODE_BYTES, np.uint8)
        objs = np.zeros(self.n_objs * OBJ_BYTES, np.uint8)
        levels = np.zeros(self.n_levels + 1, np.int32)
        box, area = np.zeros((self.n_nodes, 6)), np.zeros(self.n_nodes)
        self.L.rp_get(self.h, ptr(nodes), ptr(objs), ptr(levels), ptr(box), ptr(area))
        return dict(nodes=nodes, objs=objs, levels=levels, box=box, area=area)

    def refit(self, world: np.ndarray) -> float:
        w = np.ascontiguousarray(world)
        return float(self.L.rp_refit(self.h, ptr(w), len(w)))

    def check(self, world: np.ndarray) -> dict:
        w = np.ascontiguousarray(world)
        out = np.zeros(5, np.int32)
        self.L.rp_check(self.h, ptr(w), len(w), ptr(out))
        return dict(zip(("objects_outside", "children_outside", "bytes_differ", "topology_changed", "records_differ"), (int(v) for v in out)))

    def rays(self, world: np.ndarray, nrays: int, seed: int):
        """(disagreements between the tree's winner and the linear scan's, rays that hit anything)."""
        w = np.ascontiguousarray(world)
        hits = C.c_int32(0)
        bad = self.L.rp_rays(self.h, ptr(w), len(w), nrays, seed, C.byref(hits))
        return int(bad), int(hits.value)


def python_cost(area) -> float:
    """The figure from a[q] in plain Python floats: node order inside blocks of 4096, the block sums in block order."""
    a = [float(x) for x in area]
    total = 0.0
    for b0 in range(0, len(a), 4096):
        s = 0.0
        for x in a[b0:b0 + 4096]:
            s = s + x
        total = total + s
    return total


# ---------------------------------------------------------------- the device probe
def gpu():
    """tests/bvh_refit_probe.hip, compiled with the library's compiler and flags; loaded after torch (one HIP runtime)."""
    if "gpu" not in _libs:
        import torch  # noqa: F401

        from path_trace_golang_amd import build

        out = os.path.join(_build_dir(), "libbvhrefitgpuprobe.so")
        r = subprocess.run([build.HIPCC, *build.HIP_FLAGS, "-shared", "-I", CSRC, "-I", os.path.join(ROOT, "tests"), GPU_SOURCE, "-o", out],
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("bvh refit probe does not compile:\n%s\n%s" % (r.stdout, r.stderr))
        L = C.CDLL(out)
        L.rpg_refit.argtypes = [_vp, C.c_int32, _vp, C.c_int32, _vp, C.c_int32, _vp, C.c_int32, C.c_double, C.c_int32, _vp, _vp, _vp]
        L.rpg_refit.restype = C.c_int
        L.rpg_bits.argtypes = [_vp, _vp, C.c_int32]
        L.rpg_bits.restype = C.c_int
        _libs["gpu"] = L
    return _libs["gpu"]


def gpu_refit(state: dict, world: np.ndarray, margin: float, main_nodes: int) -> dict:
    """The product's kernels on a host state (Tree.state()) and a world: the refitted state and the figure."""
    nodes, objs = state["nodes"].copy(), state["objs"].copy()
    levels = np.ascontiguousarray(state["levels"], np.int32)
    n_nodes, n_objs = len(nodes) // NODE_BYTES, len(objs) // OBJ_BYTES
    w = np.ascontiguousarray(world)
    box, area = np.zeros((n_nodes, 6)), np.zeros(n_nodes)
    cost = C.c_double(0.0)
    rc = gpu().rpg_refit(ptr(nodes), n_nodes, ptr(objs), n_objs, ptr(w), len(w), ptr(levels), len(levels) - 1, float(margin), main_nodes,
                         ptr(box), ptr(area), C.byref(cost))
    if rc != 0:
        raise RuntimeError("rpg_refit: status %d" % rc)
    return dict(nodes=nodes, objs=objs, levels=levels, box=box, area=area, cost=float(cost.value))


# ---------------------------------------------------------------- whole scenes
def moved_scene(sc, moves_by_index: dict):
    """A deep copy of scene.Scene sc with object i moved by moves_by_index[i] = (dx, dy, dz)."""
    out = copy.deepcopy(sc)
    for i, d in moves_by_index.items():
        p = out.objects[i].position
        p.x, p.y, p.z = p.x + d[0], p.y + d[1], p.z + d[2]
    return out


def finite_indices(sc, kinds=("sphere", "box", "sphere_light")):
    return [i for i, o in enumerate(sc.objects) if o.type in kinds and not o.id.startswith("wall-")]


EDITS = ("spheres grown", "spheres shrunk", "boxes resized", "radii negated", "radii zero", "plane lowered", "dielectrics moved and grown")
DIELECTRIC_EDIT = "dielectrics moved and grown"


def dielectric_indices(sc):
    kinds = {m.id: m.type for m in sc.materials}
    return [i for i in finite_indices(sc) if kinds.get(sc.objects[i].material_id) == "dielectric"]


def edited_scenes(sc):
    """The edits of resizes() on a scene.Scene, each made to sc itself (EDITS, in order), and the ground plane lowered by 0.5: the
    free spheres (lights among them) grown x1.7; shrunk x0.01; the free boxes x2.5 on x and x0.2 on y; two spheres' radii negated (one of them glass);
    two spheres' radii zero; the plane; every free dielectric moved by DIELECTRIC_MOVE and grown x1.3.  The room's walls stay.
    Yields (name, scene)."""
    sph = finite_indices(sc, ("sphere", "sphere_light"))
    box = finite_indices(sc, ("box",))

    def scaled(idx, fx, fy=None, fz=None):
        out = copy.deepcopy(sc)
        for i in idx:
            s = out.objects[i].size
            s.x, s.y, s.z = s.x * fx, s.y * (fx if fy is None else fy), s.z * (fx if fz is None else fz)
        return out

    yield EDITS[0], scaled(sph, 1.7)
    yield EDITS[1], scaled(sph, 0.01)
    yield EDITS[2], scaled(box, 2.5, 0.2, 1.0)
    die = dielectric_indices(sc)
    # a negative radius keeps the hits (radius_sq) and turns the outward normal (inv_radius) round: an opaque sphere looks the same,
    # a glass one swaps its inside and outside -- so the two are the glass sphere and the other sphere that look largest from the camera
    def apparent(i):
        p, c = sc.objects[i].position, sc.camera.position
        return sc.objects[i].size.x / float(np.linalg.norm([p.x - c.x, p.y - c.y, p.z - c.z]))

    yield EDITS[3], scaled([max((i for i in sph if i in die), key=apparent), max((i for i in sph if i not in die), key=apparent)], -1.0)
    yield EDITS[4], scaled(sph[-2:], 0.0)
    low = copy.deepcopy(sc)
    planes = [o for o in low.objects if o.type == "plane"]
    assert len(planes) == 1
    planes[0].position.y -= 0.5
    yield EDITS[5], low
    grown = moved_scene(scaled(die, 1.3), {i: DIELECTRIC_MOVE for i in die})
    yield EDITS[6], grown


def teleported(sc):
    """sc with object i given the position of object n - 1 - i (T4 / T7): every object keeps its type, size and material."""
    out = copy.deepcopy(sc)
    n = len(sc.objects)
    for i in range(n):
        src = sc.objects[n - 1 - i].position
        p = out.objects[i].position
        p.x, p.y, p.z = src.x, src.y, src.z
    return out
