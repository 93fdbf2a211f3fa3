"""Helpers of the device BVH build's tests (test_bvh_build_cpu.py, test_bvh_build_reference_cpu.py, test_bvh_build_probe_gpu.py,
test_bvh_build_gpu.py, test_bvh_build_edges_gpu.py): the worlds and scenes of the cases, tests/bvh_build_probe.cpp as a
ctypes library and as a program (the host restatement of csrc/pt_bvh_build.h) and tests/bvh_build_probe.hip (the product's launch
sequence on a world a test hands in).  The independent statement of the build is bvh_build_reference.py."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import bvh_build_reference as ref
import bvh_refit_support as rs
from fog_support import CSRC, CXXFLAGS, ROOT, ptr

HOST_SOURCE = os.path.join(ROOT, "tests", "bvh_build_probe.cpp")
GPU_SOURCE = os.path.join(ROOT, "tests", "bvh_build_probe.hip")
DEVOBJ, NODE_BYTES, OBJ_BYTES = rs.DEVOBJ, rs.NODE_BYTES, rs.OBJ_BYTES
PT_BVH_STACK = 96  # csrc/pt_device.h

SIZES = (1, 2, 3, 5, 17, 129, 300, 3000)
DIELECTRICS = (0, 1, 7)
SPECIAL = ("one centroid", "a line", "64 identical among 300", "geometric ratio 2")
LARGE = 20000  # more than one block of every kernel and scan, more than one tile of the sort (see test_bvh_build_probe_gpu.py)

_vp = C.c_void_p
_libs = {}
_worlds = {}


def _spheres(centres, radii) -> np.ndarray:
    w = np.zeros(len(centres), DEVOBJ)
    w["a"] = centres
    w["radius"] = radii
    w["radius_sq"] = w["radius"] * w["radius"]
    w["inv_radius"] = 1.0 / w["radius"]
    w["kind"] = rs.KIND_SPHERE
    w["mat"] = np.arange(len(w)) % 5
    return w


def special_world(name: str) -> np.ndarray:
    """The smallest worlds where the radix tree, the tie-break and the collapse can go wrong; every ninth object dielectric."""
    if name not in _worlds:
        kind, _, size = name.partition(", ")
        n = int(size) if size.isdigit() else 300
        if kind == "one centroid":  # all keys equal: the tree is the tie-break's alone
            w = _spheres(np.tile([1.0, 2.0, 3.0], (n, 1)), 0.5 + np.arange(n) / 256.0)  # (binary fractions: every centroid is exact)
        elif kind == "a line":  # extent 0 on two axes
            w = _spheres(np.stack([np.arange(n) * 1.0, np.full(n, 2.0), np.full(n, -1.0)], axis=1), np.full(n, 0.4))
        elif name == "64 identical among 300":
            base = rs.world_of(300, 0).copy()
            same = np.repeat(base[7:8], 64)
            w = np.concatenate([base[:150], same, base[150:]])
        elif name == "geometric ratio 2":  # x = 2^(i - 200): all but the last 21 share the lowest cell of the key
            x = np.ldexp(1.0, np.arange(n) - 200)
            w = _spheres(np.stack([x, np.zeros(n), np.zeros(n)], axis=1), 0.25 * x)
        elif kind == "three centroids interleaved":  # object i at centroid i mod 3: every sort tile holds all three keys
            x = np.array([1.0, 2.0, 0.0])[np.arange(n) % 3]  # (the key order 2, 0, 1 is not the order of the residues)
            w = _spheres(np.stack([x, np.full(n, 2.0), np.full(n, -1.0)], axis=1), 0.5 + np.arange(n) / 8192.0)
        elif name == "duplicates over the seams":
            w = seam_world()
        elif kind == "deep":
            w = deep_world(n)
        else:
            raise KeyError(name)
        w = np.ascontiguousarray(w)
        w["kind"][4::9] |= 0x100
        w.setflags(write=False)
        _worlds[name] = w
    return _worlds[name]


SEAM_COPIES = tuple(range(1000, 1101)) + tuple(range(4090, 4111))  # positions in `finite` over the first tile seam and the first sort-block seam


def seam_world() -> np.ndarray:
    """rs.world_of(5000, 0) with one object copied to the positions SEAM_COPIES: 123 equal keys that enter the sort from both sides of
    position 1024 and of position 4096.  The copied object is the one at position 7 if the run of its key then lies over positions
    1023 / 1024 of the sorted order as well; else the first object by sorted rank for which it does (bvh_build_reference says)."""
    base = rs.world_of(5000, 0)
    lo, hi = ref.object_boxes(base)
    rank = np.argsort(ref.keys_of(ref.centroids(lo, hi)), kind="stable")
    for src in [7] + [int(i) for i in rank[900:1024] if int(i) not in SEAM_COPIES]:
        w = base.copy()
        w[list(SEAM_COPIES)] = base[src]
        lo, hi = ref.object_boxes(w)
        keys = ref.keys_of(ref.centroids(lo, hi))
        run = np.flatnonzero(np.sort(keys, kind="stable") == keys[src])
        if run[0] <= 1023 and run[-1] >= 1024:
            return w
    raise AssertionError("no object of the world gives a run of equal keys over sorted positions 1023 / 1024")


def deep_keys(ties: int) -> list:
    """The keys of deep_world(ties), sorted: a chain that peels one small group off per binary level for 60 levels."""
    keys = [(1 << 63) - 1]
    for k in range(60):
        bit = 62 - k
        base = 1 << bit
        low = base - 1
        keys += [base, base | low, base | low >> 1, base | (low >> 1) + 1] if bit >= 2 else [base]
    return [0] * ties + sorted(set(keys))


def deep_world(ties: int, extra=()) -> np.ndarray:
    """Spheres of radius 0.25 whose keys are deep_keys(ties): the centroid of key K is its three de-interleaved 21-bit coordinates, with
    2097151 replaced by 2097152, so that every extent is exactly 2^21 and every scale exactly 1.  `extra` rows of (x, y, z, radius)
    are appended (their centroids must lie inside the extent: the keys of the others then stay)."""
    cen = []
    for key in deep_keys(ties):
        q = [sum(((key >> (3 * b + 2 - a)) & 1) << b for b in range(21)) for a in range(3)]
        cen.append([2097152.0 if v == 2097151 else float(v) for v in q])
    cen, rad = np.array(cen), np.full(len(cen), 0.25)
    if len(extra):
        e = np.asarray(extra, np.float64)
        cen, rad = np.concatenate([cen, e[:, :3]]), np.concatenate([rad, e[:, 3]])
    return _spheres(cen, rad)


DEEP_SCALE = 2.0 ** -18  # a power of two, so exact: the chain's extent of 2^21 becomes 8
# (x, y, z, radius, material) in the scaled frame: a radius does not move a centroid, and these centroids lie inside the chain's extent
DEEP_BIG = ((4.0, 4.0, 4.0, 2.5, "chrome"), (1.5, 6.0, 2.0, 2.0, "red"), (6.0, 2.0, 5.0, 2.0, "glass"), (2.0, 1.5, 6.0, 1.5, "green"))


def deep_scene(ties: int, big: bool = True):
    """deep_world(ties) scaled by DEEP_SCALE as a scene.Scene (every ninth sphere glass), with the spheres DEEP_BIG in front of a
    camera that sees them (`big`) or without them."""
    from path_trace_golang_amd import scene as scn
    from path_trace_golang_amd import synth

    sc = synth.make_scene(0, 1)  # its camera block, sky and materials
    sc.name = "deep-%d" % ties
    sc.camera = scn.Camera(position=scn.Vec3(4.0, 4.0, 22.0), target=scn.Vec3(4.0, 4.0, 4.0), up=scn.Vec3(0, 1, 0), fov=35.0, aperture=0.0,
                           focus_dist=18.0, aspect_ratio=0.0)
    w = deep_world(ties)
    surf = ("red", "green", "blue", "gold", "glass", "chrome", "mirror", "red", "green")
    sc.objects = [scn.Object(id="c%d" % i, type="sphere", position=scn.Vec3(*(float(v) * DEEP_SCALE for v in o["a"])),
                             size=scn.Vec3(float(o["radius"]) * DEEP_SCALE, 0, 0), material_id=surf[i % 9]) for i, o in enumerate(w)]
    if big:
        sc.objects += [scn.Object(id="big%d" % i, type="sphere", position=scn.Vec3(x, y, z), size=scn.Vec3(r, 0, 0), material_id=m)
                       for i, (x, y, z, r, m) in enumerate(DEEP_BIG)]
    return sc


def scene_world(sc) -> np.ndarray:
    """The finite objects of a scene.Scene as device records, in scene order (what the library's scene conversion gives, planes left
    out): the world whose trees a render of `sc` builds, up to the world indices."""
    glass = {m.id: m.type == "dielectric" for m in sc.materials}
    rows = [o for o in sc.objects if o.type in ("sphere", "sphere_light", "box")]
    w = np.zeros(len(rows), DEVOBJ)
    for i, o in enumerate(rows):
        p, s = np.array(o.position.as_list()), np.array(o.size.as_list())
        if o.type == "box":
            w[i]["a"], w[i]["b"], w[i]["kind"] = p - s * 0.5, p + s * 0.5, rs.KIND_BOX
        else:
            with np.errstate(divide="ignore"):
                w[i]["a"], w[i]["radius"], w[i]["radius_sq"], w[i]["inv_radius"], w[i]["kind"] = p, s[0], s[0] * s[0], np.float64(1.0) / s[0], rs.KIND_SPHERE
        w[i]["kind"] |= 0x100 if glass.get(o.material_id, False) else 0
    return w


def large_world() -> np.ndarray:
    if "large" not in _worlds:
        rng = np.random.default_rng(11)
        n = LARGE
        w = _spheres(rng.uniform(-50.0, 50.0, (n, 3)), rng.uniform(0.05, 0.6, n))
        box = np.arange(n) % 3 == 0
        half = rng.uniform(0.05, 0.5, (n, 3))
        w["b"][box] = w["a"][box] + half[box]
        w["a"][box] = w["a"][box] - half[box]
        w["kind"][box] = rs.KIND_BOX
        w["radius"][box] = w["radius_sq"][box] = w["inv_radius"][box] = 0.0
        w["kind"][4::9] |= 0x100
        w.setflags(write=False)
        _worlds["large"] = w
    return _worlds["large"]


def cases():
    """(name, world) of B2: the sizes with 0 / 1 / 7 dielectrics, then the special worlds."""
    for n in SIZES:
        for nd in DIELECTRICS:
            yield "n=%d diel=%d" % (n, nd), rs.world_of(n, nd)
    for name in SPECIAL:
        yield name, special_world(name)


CASE_NAMES = [name for name, _ in cases()]

# The worlds on the boundaries of the build's kernels (test_bvh_build_reference_cpu.py asserts what each is chosen for).
BOUNDARY_SIZES = (255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 5121)  # a block of 256, a tile of 1024, a sort block of 4096, a fifth tile
TIE_WORLDS = ("one centroid, 5000", "a line, 5000", "three centroids interleaved, 4500", "duplicates over the seams")
DEEP_TIES = 26  # the smallest number of equal keys in front of the chain for which the tree does not fit the stack (found on the host)
DEEP_FITS, DEEP_TOO_DEEP = "deep, 1", "deep, %d" % DEEP_TIES
NEW_CASE_NAMES = ["n=%d diel=7" % n for n in BOUNDARY_SIZES] + list(TIE_WORLDS) + [DEEP_FITS, DEEP_TOO_DEEP]


def case_world(name: str) -> np.ndarray:
    if name == "large":
        return large_world()
    if name.startswith("n="):
        n, nd = (int(part.split("=")[1]) for part in name.split())
        return rs.world_of(n, nd)
    return special_world(name)


# ---------------------------------------------------------------- the host build
def host():
    if "host" not in _libs:
        out = os.path.join(rs._build_dir(), "libbvhbuildprobe.so")
        subprocess.run(["g++", *CXXFLAGS, "-Wall", "-Wextra", "-Werror", "-shared", "-I", CSRC, "-I", os.path.join(ROOT, "tests"), HOST_SOURCE,
                        "-o", out], check=True, capture_output=True)
        L = C.CDLL(out)
        L.bp_build.restype = _vp
        L.bp_build.argtypes = [_vp, C.c_int32, C.c_int32]
        L.bp_free.argtypes = [_vp]
        L.bp_free.restype = None
        L.bp_counts.argtypes = [_vp, _vp]
        L.bp_counts.restype = None
        L.bp_margin.argtypes = [_vp]
        L.bp_margin.restype = C.c_double
        L.bp_get.argtypes = [_vp, _vp, _vp, _vp]
        L.bp_get.restype = None
        L.bp_tree_counts.argtypes = [_vp, C.c_int32, _vp]
        L.bp_tree_counts.restype = None
        L.bp_tree_get.argtypes = [_vp, C.c_int32] + [_vp] * 8
        L.bp_tree_get.restype = None
        L.bp_tree_slots.argtypes = [_vp, C.c_int32, _vp]
        L.bp_tree_slots.restype = None
        L.bp_check.argtypes = [_vp, _vp]
        L.bp_check.restype = None
        L.bp_rays.argtypes = [_vp, C.c_int32, C.c_uint64, _vp]
        L.bp_rays.restype = C.c_int32
        L.bp_refit_same.argtypes = [_vp]
        L.bp_refit_same.restype = C.c_int32
        L.bp_key_scale.argtypes = [C.c_double, C.c_double]
        L.bp_key_scale.restype = C.c_double
        L.bp_quantise.argtypes = [_vp, C.c_int32, C.c_double, C.c_double, _vp]
        L.bp_quantise.restype = None
        L.bp_morton.argtypes = [_vp, C.c_int32, _vp]
        L.bp_morton.restype = None
        L.bp_sah_bytes.argtypes = [_vp, C.c_int32, _vp]
        L.bp_sah_bytes.restype = C.c_int64
        _libs["host"] = L
    return _libs["host"]


def standalone(flags=(), name="bvh_build_probe") -> str:
    """The same source as a program of its own."""
    exe = os.path.join(rs._build_dir(), name)
    subprocess.run(["g++", *CXXFLAGS, "-g", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC, "-I", os.path.join(ROOT, "tests"), HOST_SOURCE,
                    "-o", exe], check=True, capture_output=True)
    return exe


CHECK_KEYS = ("nodes", "objects", "depth", "stack_need", "not_reached_once", "objects_outside", "children_outside", "faults")


class Trees:
    """The Morton-order trees of a world by the host restatement."""

    def __init__(self, world: np.ndarray, stack_limit: int = PT_BVH_STACK):
        self.L = host()
        self.world = np.ascontiguousarray(world)
        self.h = self.L.bp_build(ptr(self.world), len(self.world), stack_limit)
        c = np.zeros(8, np.int32)
        self.L.bp_counts(self.h, ptr(c))
        self.n_nodes, self.n_objs, self.n_levels, self.main_nodes, self.depth, self.main_objs, self.stack_need, fits = (int(v) for v in c)
        self.fits = bool(fits)
        self.margin = float(self.L.bp_margin(self.h))

    def close(self):
        if self.h:
            self.L.bp_free(self.h)
            self.h = None

    __del__ = close

    def arrays(self) -> dict:
        nodes = np.zeros(self.n_nodes * NODE_BYTES, np.uint8)
        objs = np.zeros(self.n_objs * OBJ_BYTES, np.uint8)
        levels = np.zeros(self.n_levels + 1, np.int32)
        self.L.bp_get(self.h, ptr(nodes), ptr(objs), ptr(levels))
        return dict(nodes=nodes, objs=objs, levels=levels)

    def tree(self, t: int) -> dict:
        """The stages of tree t (0 main, 1 dielectric)."""
        c = np.zeros(3, np.int32)
        self.L.bp_tree_counts(self.h, t, ptr(c))
        n, nn, nl = (int(v) for v in c)
        d = dict(n=n, keys=np.zeros(n, np.uint64), sorted=np.zeros(n, np.int32), child=np.zeros((max(n - 1, 0), 2), np.int32),
                 parent=np.zeros(max(2 * n - 1, 0), np.int32), box=np.zeros((max(2 * n - 1, 0), 6)), nodes=np.zeros(nn * NODE_BYTES, np.uint8),
                 order=np.zeros(n, np.int32), levels=np.zeros(nl + 1 if n else 0, np.int32))
        if n:
            self.L.bp_tree_get(self.h, t, ptr(d["keys"]), ptr(d["sorted"]), ptr(d["child"]) if n > 1 else None, ptr(d["parent"]), ptr(d["box"]),
                               ptr(d["nodes"]), ptr(d["order"]), ptr(d["levels"]))
        d["slots"] = np.full((nn, 4), -1, np.int32)  # the binary nodes gather4 put into every wide node
        if n:
            self.L.bp_tree_slots(self.h, t, ptr(d["slots"]))
        return d

    def check(self) -> dict:
        out = np.zeros(8, np.int32)
        self.L.bp_check(self.h, ptr(out))
        return dict(zip(CHECK_KEYS, (int(v) for v in out)))

    def rays(self, nrays: int, seed: int):
        hits = C.c_int32(0)
        bad = self.L.bp_rays(self.h, nrays, seed, C.byref(hits))
        return int(bad), int(hits.value)

    def refit_same(self) -> int:
        return int(self.L.bp_refit_same(self.h))


def object_lists(world: np.ndarray):
    """The world indices of the finite objects and of the dielectric ones among them (ptbvh::scene_object_lists; no planes here)."""
    finite = np.arange(len(world), dtype=np.int32)
    glass = finite[(world["kind"] & 0x100) != 0]
    return finite, np.ascontiguousarray(glass)


# ---------------------------------------------------------------- the device probe
def gpu():
    """tests/bvh_build_probe.hip, compiled with the library's compiler and flags; loaded after torch (one HIP runtime)."""
    if "gpu" not in _libs:
        import torch  # noqa: F401

        from path_trace_golang_amd import build

        out = os.path.join(rs._build_dir(), "libbvhbuildgpuprobe.so")
        r = subprocess.run([build.HIPCC, *build.HIP_FLAGS, "-shared", "-I", CSRC, "-I", os.path.join(ROOT, "tests"), GPU_SOURCE, "-o", out],
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("bvh build probe does not compile:\n%s\n%s" % (r.stdout, r.stderr))
        L = C.CDLL(out)
        L.bpg_tree.argtypes = [_vp, C.c_int32, _vp, C.c_int32, C.c_double, C.c_int32, C.c_int32] + [_vp] * 8 + [C.c_int32, _vp]
        L.bpg_tree.restype = C.c_int
        L.bpg_objs.argtypes = [_vp, C.c_int32, _vp, C.c_int32, _vp]
        L.bpg_objs.restype = C.c_int
        L.bpg_sizes.argtypes = [_vp]
        L.bpg_sizes.restype = None
        _libs["gpu"] = L
    return _libs["gpu"]


def gpu_tree(world: np.ndarray, finite: np.ndarray, margin: float, node_off: int, obj_off: int) -> dict:
    """The product's launch sequence for one tree: every stage as the device left it."""
    n = len(finite)
    w = np.ascontiguousarray(world)
    f = np.ascontiguousarray(finite, np.int32)
    d = dict(n=n, keys=np.zeros(n, np.uint64), sorted=np.zeros(n, np.int32), child=np.zeros((max(n - 1, 0), 2), np.int32),
             parent=np.zeros(max(2 * n - 1, 0), np.int32), box=np.zeros((max(2 * n - 1, 0), 6)), nodes=np.zeros(n * NODE_BYTES, np.uint8),
             order=np.zeros(n, np.int32))
    levels = np.zeros(n + 2, np.int32)
    nl = C.c_int32(0)
    if n:
        rc = gpu().bpg_tree(ptr(w), len(w), ptr(f), n, float(margin), node_off, obj_off, ptr(d["keys"]), ptr(d["sorted"]),
                            ptr(d["child"]) if n > 1 else None, ptr(d["parent"]), ptr(d["box"]), ptr(d["nodes"]), ptr(d["order"]), ptr(levels),
                            len(levels), C.byref(nl))
        if rc != 0:
            raise RuntimeError("bpg_tree: status %d" % rc)
    d["levels"] = levels[:nl.value].copy()
    nn = int(d["levels"][-1]) if nl.value else 0
    d["nodes"] = d["nodes"][:nn * NODE_BYTES]
    return d


def gpu_objs(order: np.ndarray, world: np.ndarray) -> np.ndarray:
    o = np.ascontiguousarray(order, np.int32)
    w = np.ascontiguousarray(world)
    out = np.zeros(len(o) * OBJ_BYTES, np.uint8)
    if len(o):
        rc = gpu().bpg_objs(ptr(o), len(o), ptr(w), len(w), ptr(out))
        if rc != 0:
            raise RuntimeError("bpg_objs: status %d" % rc)
    return out


def gpu_sizes() -> dict:
    out = np.zeros(4, np.int32)
    gpu().bpg_sizes(ptr(out))
    return dict(zip(("sort_tile", "scan_tile", "reduce_tile", "sort_passes"), (int(v) for v in out)))
