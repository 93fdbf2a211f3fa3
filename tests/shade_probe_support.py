"""Builds and loads tests/shade_probe.hip -- the surface step of the trace kernels (csrc/pt_kernels.h: outward_normal, reflect_vec,
shade_hit, dielectric_scatter, exit_post, roulette_advance) one lane per case -- and holds the tables it runs on
(test_shade_probe_cpu.py checks them with the oracle alone, test_shade_probe_gpu.py runs them on the device).

The probe is compiled with the library's compiler and exactly its flags (path_trace_golang_amd.build.HIPCC, HIP_FLAGS), into a
temporary directory, never into the tree.  The tables are functions of fixed seeds.  A case is one (object, ray, material, stream
state); its t is the one ora_hit returned with tMin = 0.001, and a generated ray the reference does not hit is no case.  The
reference of every comparison is the oracle's own step functions (ora_scatter_steps, ora_exit_steps, ora_roulette_steps,
ora_reflects), i.e. the code rayColorOpt runs."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from fog_support import CSRC, CXXFLAGS, ROOT, ptr

SOURCE = os.path.join(ROOT, "tests", "shade_probe.hip")
SYMBOLS = ("probe_shade_guard", "probe_shade", "probe_normal", "probe_reflect", "probe_exit", "probe_roulette")
PRODUCT = ("ptk::shade_hit<STATS, GLASS>", "ptk::outward_normal", "ptk::reflect_vec", "ptk::dielectric_scatter<STATS>", "ptk::exit_post",
           "ptk::roulette_advance<STATS>", "ptk::stage_lds", "convert_material")
MAXF = 1.7976931348623157e308
LAMBERT, METAL, DIELECTRIC, EMISSIVE, MIRROR = range(5)
SPHERE, PLANE, BOX = 0, 1, 2

DEVOBJ = np.dtype([("a", "f8", 3), ("b", "f8", 3), ("radius", "f8"), ("radius_sq", "f8"), ("inv_radius", "f8"), ("kind", "i4"),
                   ("mat", "i4")])   # ptd::DevObj (csrc/pt_device.h)
DEVMAT = np.dtype([("albedo", "f8", 3), ("rough", "f8"), ("ior", "f8"), ("emit", "f8", 3), ("absorption", "f8", 3), ("typ", "i4"),
                   ("absorbs", "i4"), ("rough_sq", "f8"), ("inv_ior", "f8"), ("r0_front", "f8"), ("r0_back", "f8")])   # ptd::DevMat
assert DEVOBJ.itemsize == 80 and DEVMAT.itemsize == 128

_dir = None
_lib = None
_shim = None


def _ora():
    from oracle import ora

    return ora


def up(x):
    return float(np.nextafter(x, np.inf))


def down(x):
    return float(np.nextafter(x, -np.inf))


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same(dev, ref):
    """Element-wise: the same bits, or a NaN where the reference has a NaN."""
    dev, ref = np.ascontiguousarray(dev, np.float64), np.ascontiguousarray(ref, np.float64)
    return (bits(dev) == bits(ref)) | (np.isnan(dev) & np.isnan(ref))


# ---------------------------------------------------------------- the probe
def compile_probe() -> str:
    """Path of the probe's shared library (built once per process)."""
    global _dir
    from path_trace_golang_amd import build

    if _dir is None:
        _dir = tempfile.mkdtemp(prefix="shprobe_")
    out = os.path.join(_dir, "libshadeprobe.so")
    if not os.path.exists(out):
        r = subprocess.run([build.HIPCC, *build.HIP_FLAGS, "-shared", "-I", CSRC, SOURCE, "-o", out], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("shade probe does not compile:\n%s\n%s" % (r.stdout, r.stderr))
    return out


def load():
    """The probe, loaded after torch so that the process keeps one HIP runtime (as conftest.gpu_ctx does for libptcore.so)."""
    global _lib
    if _lib is None:
        import torch  # noqa: F401

        L = C.CDLL(compile_probe())
        vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
        L.probe_shade_guard.restype = i64
        L.probe_shade_guard.argtypes = []
        L.probe_shade.argtypes = [i32, i32, vp, i32, i64, vp, vp, vp, vp, vp, vp, vp]
        L.probe_normal.argtypes = [i64, vp, vp, vp]
        L.probe_reflect.argtypes = [i64, vp, vp, vp]
        L.probe_exit.argtypes = [vp, i32, i64, vp, vp, vp, vp, vp, vp]
        L.probe_roulette.argtypes = [i32, i64, vp, vp, vp, vp, vp, vp, vp]
        for s in SYMBOLS[1:]:
            getattr(L, s).restype = C.c_int
        _lib = L
    return _lib


def convert_host():
    """csrc/pt_convert.h built for the host with g++ -ffp-contract=off: shim_convert(pt_material *, n, DevMat *)."""
    global _shim, _dir
    if _shim is None:
        if _dir is None:
            _dir = tempfile.mkdtemp(prefix="shprobe_")
        src = os.path.join(_dir, "convert_shim.cpp")
        with open(src, "w") as f:
            f.write('#include "pt_convert.h"\nextern "C" void shim_convert(const pt_material *m, int32_t n, ptd::DevMat *out) {\n'
                    "    for (int32_t i = 0; i < n; i++) out[i] = ptd::convert_material(m[i]);\n}\n")
        out = os.path.join(_dir, "libconvertshim.so")
        subprocess.run(["g++", *CXXFLAGS, "-shared", "-I", CSRC, src, "-o", out], check=True, capture_output=True)
        _shim = C.CDLL(out)
        _shim.shim_convert.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        _shim.shim_convert.restype = None
    return _shim


def _ok(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError("%s: status %d" % (what, rc))


def _guarded(n, cols, dtype):
    g = int(load().probe_shade_guard())
    return np.zeros((n + g, cols) if cols else (n + g,), dtype)


def _strip(n, *arrays):
    """The first n rows of every output array, after the check that the guard rows behind them still hold 0xFF bytes."""
    for a in arrays:
        assert len(a) > n and np.all(a[n:].view(np.uint8) == 0xFF), "guard words were written"
    return [a[:n] for a in arrays]


def gpu_shade(mats, objs, t, rays, states, stats: bool, glass: bool, lds: bool, sequence: bool = False) -> dict:
    """probe_shade over n cases: shade_hit<stats, glass> with the material table in LDS or in global memory, or (sequence) the
    glass_kernel sequence.  dict(I i32 [n, 5] = finished, exit_search, exit_mat, c_draw, j_draw; F f64 [n, 12] = term, att, origin,
    direction; S u64 [n])."""
    n = len(objs)
    objs, t, rays = np.ascontiguousarray(objs, DEVOBJ), np.ascontiguousarray(t, np.float64), np.ascontiguousarray(rays, np.float64)
    states = np.ascontiguousarray(states, np.uint64)
    assert t.shape == (n,) and rays.shape == (n, 6) and states.shape == (n,)
    I, F, S = _guarded(n, 5, np.int32), _guarded(n, 12, np.float64), _guarded(n, 0, np.uint64)
    variant = (4 | int(stats)) if sequence else (int(stats) | (int(glass) << 1))
    _ok(load().probe_shade(variant, int(lds), C.addressof(mats), len(mats), n, ptr(objs), ptr(t), ptr(rays), ptr(states), ptr(I), ptr(F),
                           ptr(S)), "probe_shade")
    I, F, S = _strip(n, I, F, S)
    return dict(I=I, F=F, S=S)


def gpu_normal(objs, p):
    n = len(objs)
    objs, p = np.ascontiguousarray(objs, DEVOBJ), np.ascontiguousarray(p, np.float64)
    F = _guarded(n, 3, np.float64)
    _ok(load().probe_normal(n, ptr(objs), ptr(p), ptr(F)), "probe_normal")
    return _strip(n, F)[0]


def gpu_reflect(v, nrm):
    v, nrm = np.ascontiguousarray(v, np.float64), np.ascontiguousarray(nrm, np.float64)
    n = len(v)
    F = _guarded(n, 3, np.float64)
    _ok(load().probe_reflect(n, ptr(v), ptr(nrm), ptr(F)), "probe_reflect")
    return _strip(n, F)[0]


def gpu_exit(mats, mat, best, tmax, rays, att):
    n = len(mat)
    mat, best = np.ascontiguousarray(mat, np.int32), np.ascontiguousarray(best, np.int32)
    tmax, rays, att = (np.ascontiguousarray(x, np.float64) for x in (tmax, rays, att))
    F = _guarded(n, 6, np.float64)
    _ok(load().probe_exit(C.addressof(mats), len(mats), n, ptr(mat), ptr(best), ptr(tmax), ptr(rays), ptr(att), ptr(F)), "probe_exit")
    F = _strip(n, F)[0]
    return F[:, 3:6], F[:, 0:3]   # att, origin


def gpu_roulette(depth, att, T, states, stats: bool) -> dict:
    n = len(depth)
    depth, states = np.ascontiguousarray(depth, np.int32), np.ascontiguousarray(states, np.uint64)
    att, T = np.ascontiguousarray(att, np.float64), np.ascontiguousarray(T, np.float64)
    I, F, S = _guarded(n, 5, np.int32), _guarded(n, 3, np.float64), _guarded(n, 0, np.uint64)
    _ok(load().probe_roulette(int(stats), n, ptr(depth), ptr(att), ptr(T), ptr(states), ptr(I), ptr(F), ptr(S)), "probe_roulette")
    I, F, S = _strip(n, I, F, S)
    return dict(I=I, F=F, S=S)


# ---------------------------------------------------------------- materials
ROUGHS = (0.0, -0.0, 1e-6, down(1e-6), up(1e-6), 1e-3, 0.5, 1.0, 1.5, -0.5)
SMOOTHS = (0.0, 0.3, 1.0, 2.0)
IORS = (0.0, 1.0, down(1.0), up(1.0), 0.5, 1.1, 1.5, 2.4, -1.0, -1.5, 1e-300, 1e300, 5e-324)
ALBEDOS = (0.0, -0.0, 5e-324, 1e-6, down(1e-6), up(1e-6), 0.95, down(0.95), up(0.95), 1.0, 5.0, 1e308, -0.25)
EMITS = (((1.0, 0.8, 0.6), 3.0), ((1.0, 0.8, 0.6), 0.0), ((1.0, -0.8, 0.6), 3.0), ((1e308, 1.0, 1e200), 1e10))   # ordinary, 0, negative, -> inf
ABSORBS = ((0.0, 0.0, 0.0), (-0.0, -0.0, -0.0), (0.4, -0.2, -0.1), (1e-300, 1e-300, 1e-300), (1e3, 2e3, 5e2), (1e308, 1e308, 1e308))
BASE = dict(albedo=(0.8, 0.6, 0.4), rough=0.3, smoothness=0.0, ior=1.5, emit=(1.0, 0.8, 0.6), power=3.0, absorption=(0.3, 0.1, 0.05))
NONFINITE = (float("inf"), float("-inf"), float("nan"))


def _material(typ, **kw):
    m = _ora().OraMaterial()
    m.type = typ
    for k, v in dict(BASE, **kw).items():
        if isinstance(v, (tuple, list)):
            getattr(m, k)[:] = v
        else:
            setattr(m, k, v)
    return m


def _component(base, k, v):
    out = list(base)
    out[k % 3] = v
    return tuple(out)


def material_specs():
    """[(set name, keyword arguments over BASE)]: every type gets every one, so that a field read by the wrong type shows."""
    specs = [("base", {})]
    specs += [("rough", dict(rough=v)) for v in ROUGHS]
    specs += [("smoothness", dict(smoothness=v)) for v in SMOOTHS]
    specs += [("ior", dict(ior=v)) for v in IORS]
    specs += [("albedo", dict(albedo=_component(BASE["albedo"], k, v))) for k, v in enumerate(ALBEDOS)]
    specs += [("emit", dict(emit=e, power=p)) for e, p in EMITS]
    specs += [("absorption", dict(absorption=a)) for a in ABSORBS]
    nf = []
    for v in NONFINITE:
        nf += [dict(rough=v), dict(smoothness=v), dict(ior=v), dict(power=v)]
        nf += [dict(albedo=_component(BASE["albedo"], k, v)) for k in range(3)]
        nf += [dict(emit=_component(BASE["emit"], 0, v))]
        nf += [dict(absorption=_component(BASE["absorption"], k, v)) for k in range(3)]
    return specs + [("nonfinite", kw) for kw in nf]


_materials = None


def materials():
    """dict(arr: the ctypes table (OraMaterial and pt_material share one layout), n, set: the set name of each, finite bool [n],
    conv f64 [n, 12]: ora_convert_material of each).  Material k has type k % 5."""
    global _materials
    if _materials is None:
        ora = _ora()
        specs = material_specs()
        ms, names = [], []
        for name, kw in specs:
            for typ in range(5):
                ms.append(_material(typ, **kw))
                names.append(name)
        arr = ora.material_array(ms)
        conv = np.zeros((len(ms), 12))
        for k in range(len(ms)):
            ora.lib().ora_convert_material(C.byref(arr[k]), conv[k].ctypes.data_as(C.POINTER(C.c_double)))
        names = np.array(names)
        _materials = dict(arr=arr, n=len(ms), set=names, finite=names != "nonfinite", conv=conv, typ=conv[:, 0].astype(np.int32))
    return _materials


# ---------------------------------------------------------------- hit geometry
# (kind, a, b, radius): a unit sphere, a sphere of radius -0.8, a sphere of radius 1e-9, the plane, the box
OBJECTS = ((SPHERE, (0.25, -0.125, 0.5), (0.0, 0.0, 0.0), 1.0),
           (SPHERE, (-0.375, 0.125, 0.25), (0.0, 0.0, 0.0), -0.8),
           (SPHERE, (0.125, 0.25, 0.375), (0.0, 0.0, 0.0), 1e-9),
           (PLANE, (0.0, -0.5, 0.0), (0.0, 1.0, 0.0), 0.0),
           (BOX, (-1.0, -0.5, -0.75), (1.0, 0.5, 0.75), 0.0))
OBJECT_NAMES = ("sphere", "sphere_neg", "sphere_tiny", "plane", "box")
SCALES = (1.0, 1e-150, 1e-160, 1e-170, 1e-200, 1e-300, 1e100, 1e150)
CRITICAL_IORS = (1.5, 2.4, 0.5)
# classes of generated rays; the share of each that the reference does not hit is bounded by the CPU test
CLASSES = ("normal", "grazing", "inside", "plane", "box_face", "box_inside", "box_edge", "box_corner", "basis_normal", "basis_mirror",
           "scale", "critical")


def _unit(r, n):
    v = r.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _ortho(r, n):
    e1 = _unit(r, n)
    e2 = np.cross(e1, _unit(r, n))
    e2 /= np.linalg.norm(e2, axis=1, keepdims=True)
    return e1, e2


def _ulps(x, k):
    """x moved by k units in the last place (k an integer array or scalar), through the integer view."""
    x = np.asarray(x, np.float64)
    i = x.view(np.int64) + np.where(x >= 0, 1, -1) * np.asarray(k, np.int64)
    return i.view(np.float64)


class _Rays:
    def __init__(self):
        self.obj, self.ray, self.cls, self.tag = [], [], [], []

    def add(self, obj, o, d, cls, tag=0):
        o, d = np.atleast_2d(np.asarray(o, np.float64)), np.atleast_2d(np.asarray(d, np.float64))
        n = max(len(o), len(d))
        self.ray.append(np.hstack([np.broadcast_to(o, (n, 3)), np.broadcast_to(d, (n, 3))]))
        self.obj.append(np.broadcast_to(np.asarray(obj, np.int32), (n,)).copy())
        self.cls.append(np.full(n, CLASSES.index(cls), np.int32))
        self.tag.append(np.broadcast_to(np.asarray(tag, np.int32), (n,)).copy())


def _sphere_templates(r):
    """Rays against the unit sphere at the origin: (q, w, class)."""
    out = []
    n = _unit(r, 40)
    out.append((3.0 * n, -n, "normal"))
    for b in (0.5, 0.9, 0.99, 1 - 1e-6, 1 - 1e-9, 1 - 1e-12):   # impact parameter
        e1, e2 = _ortho(r, 40)
        out.append((3.0 * e1 + b * e2, -e1, "grazing"))
    q = _unit(r, 300) * (0.6 * r.random((300, 1)))                # off centre, so that back faces see every angle
    out.append((q, _unit(r, 300), "inside"))
    return out


def _unit_xy(x):
    """(x, y) with y < 0 next to -sqrt(1 - x*x) and x*x + y*y == 1.0 exactly as the reference sums it: 1/sqrt is then 1.0 and the unit
    direction is (x, y, 0) itself.  None when no y within 64 ulps does it."""
    y0 = -np.sqrt(1.0 - x * x)
    for k in sorted(range(-64, 65), key=abs):
        y = float(_ulps(y0, k))
        if x * x + y * y + 0.0 * 0.0 == 1.0:
            return x, y
    return None


def generated_rays(seed=20260401):
    """dict(obj i32 [n]: index into OBJECTS or -1 (see `shape`); shape: (kind i32, a, b f64 [n, 3], radius f64) [n] of each ray's
    object; ray f64 [n, 6]; cls i32 [n]: index into CLASSES; tag i32 [n]: (scale index * 5 + object) * 2 + (origin moved), critical ior index, 0 otherwise)."""
    r = np.random.default_rng(seed)
    R = _Rays()
    planes = []   # basis_normal: planes of their own, one normal each
    for oi, (kind, a, b, radius) in enumerate(OBJECTS):
        a, b = np.array(a), np.array(b)
        if kind == SPHERE:
            for q, w, cls in _sphere_templates(r):
                R.add(oi, a + abs(radius) * q, abs(radius) * w, cls)
        elif kind == PLANE:
            for side in (1.0, -1.0):
                for dy in (1.0, 0.5, 1e-2, 1e-5, 2e-6):      # down to the |denom| >= 1e-6 limit of objects.go:100
                    n = 30
                    t2 = r.standard_normal((n, 2))
                    t2 *= np.sqrt(1.0 - dy * dy) / np.linalg.norm(t2, axis=1, keepdims=True)
                    d = np.stack([t2[:, 0], np.full(n, -side * dy), t2[:, 1]], axis=1)
                    land = np.stack([r.uniform(-2, 2, n), np.full(n, a[1]), r.uniform(-2, 2, n)], axis=1)
                    R.add(oi, land - d * (0.5 + r.random((n, 1))), d, "plane")
        else:
            c, half = (a + b) / 2, (b - a) / 2
            n = 400
            target = c + half * r.uniform(-0.98, 0.98, (n, 3))
            face = r.integers(0, 6, n)
            target[np.arange(n), face % 3] = np.where(face < 3, a[face % 3], b[face % 3])
            w = _unit(r, n)
            w[np.arange(n), face % 3] = np.where(face < 3, 1.0, -1.0) * (0.05 + np.abs(w[np.arange(n), face % 3]))
            R.add(oi, target - 2.5 * w, w, "box_face")
            R.add(oi, c + half * r.uniform(-0.999, 0.999, (200, 3)), _unit(r, 200), "box_inside")   # t = tMin: the point stays inside
            steps = np.arange(-2, 3)
            for axes in ((0, 1), (0, 2), (1, 2), (0, 1, 2)):   # edges along the remaining axis; the corners
                for sgn in np.ndindex(*(2,) * len(axes)):
                    pt = c.copy()
                    d = np.zeros(3)
                    for ax, s in zip(axes, sgn):
                        pt[ax] = b[ax] if s else a[ax]
                        d[ax] = -1.0 if s else 1.0
                    free = [ax for ax in range(3) if ax not in axes]
                    for rep in range(3 if free else 1):
                        p0 = pt.copy()
                        for ax in free:
                            p0[ax] = c[ax] + half[ax] * (0.0, 0.5, -0.25)[rep]
                        o0 = p0 - 2.0 * d      # exact: the ray reaches the edge or corner itself at t = 2
                        grid = np.stack(np.meshgrid(*([steps] * len(axes)), indexing="ij"), axis=-1).reshape(-1, len(axes))
                        o = np.tile(o0, (len(grid), 1))
                        for j, ax in enumerate(axes):
                            o[:, ax] = _ulps(o[:, ax], grid[:, j])   # ... or a few ulps beside it
                        R.add(oi, o, d, "box_corner" if len(axes) == 3 else "box_edge")
    # the basis switch of randomCosineDirection (math.go:104): lambert takes the face normal, rough metal the mirror direction
    for x0 in (0.9, down(0.9), up(0.9)):
        for sx in (1.0, -1.0):
            nb = np.array([sx * x0, np.sqrt(1.0 - 0.81), 0.0])
            for side in (1.0, -1.0):
                n = 12
                e = np.cross(nb, _unit(r, n))
                o = r.uniform(-1, 1, (n, 3)) + side * 2.0 * nb
                planes.append((len(R.ray), nb))
                R.add(-1, o, -side * nb + 0.3 * e, "basis_normal")
            xy = _unit_xy(x0)
            if xy is not None:
                n = 12
                d = np.array([sx * xy[0], xy[1], 0.0])
                land = np.stack([r.uniform(-1, 1, n), np.full(n, -0.5), r.uniform(-1, 1, n)], axis=1)
                R.add(3, land - 2.0 * d, d, "basis_mirror")
    # direction lengths: the rays of a few templates with the direction scaled, from the same origin and from one moved back so that
    # t stays near 0.01 (large scales).  What the reference still hits becomes a case.
    for si, s in enumerate(SCALES):
        for oi, (kind, a, b, radius) in enumerate(OBJECTS):
            a, b = np.array(a), np.array(b)
            n = 8
            if kind == SPHERE:
                w = _unit(r, n)
                o, d, t1 = a - 3.0 * abs(radius) * w, abs(radius) * w, np.full((n, 1), 2.0)
            elif kind == PLANE:
                d = _unit(r, n)
                d[:, 1] = -0.3 - np.abs(d[:, 1])
                o = np.stack([r.uniform(-1, 1, n), np.full(n, 1.0), r.uniform(-1, 1, n)], axis=1)
                t1 = (1.5 / -d[:, 1])[:, None]
            else:
                d = _unit(r, n)
                d[:2] = (1.0, 0.0, 0.0), (0.0, 0.0, -1.0)
                o, t1 = (a + b) / 2 + (b - a) / 2 * r.uniform(-0.5, 0.5, (n, 3)) - 4.0 * d, np.full((n, 1), 4.0)
            R.add(oi, o, d * s, "scale", (si * len(OBJECTS) + oi) * 2)
            R.add(oi, o + d * t1 - (d * s) * 0.01, d * s, "scale", (si * len(OBJECTS) + oi) * 2 + 1)   # t near 0.01 at any scale
    # the critical angle on the plane: ior > 1 from below (back face, ratio = ior), ior < 1 from above (front face, ratio = 1/ior);
    # one component stepped one ulp at a time across ratio * sinTheta = 1
    for ci, ior in enumerate(CRITICAL_IORS):
        s0 = 1.0 / ior if ior > 1 else ior
        c0 = np.sqrt(1.0 - s0 * s0)
        k = np.arange(-150, 151)
        sx = _ulps(np.full(len(k), s0), k)
        d = np.stack([sx, np.full(len(k), c0 if ior > 1 else -c0), np.zeros(len(k))], axis=1)
        land = np.array([0.25, -0.5, 0.125])
        R.add(3, land - 2.0 * d, d, "critical", ci)
    obj = np.concatenate(R.obj)
    n = len(obj)
    kind, a, b, radius = np.zeros(n, np.int32), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n)
    for oi, (k_, a_, b_, r_) in enumerate(OBJECTS):
        m = obj == oi
        kind[m], a[m], b[m], radius[m] = k_, a_, b_, r_
    pos = np.cumsum([0] + [len(x) for x in R.ray])
    for at, nb in planes:
        sl = slice(pos[at], pos[at + 1])
        kind[sl], a[sl], b[sl] = PLANE, 0.0, nb
    return dict(obj=obj, kind=kind, a=a, b=b, radius=radius, ray=np.vstack(R.ray), cls=np.concatenate(R.cls), tag=np.concatenate(R.tag))


# materials per ray of each class: (count, which materials: "all" finite ones, by type, or the dielectrics of the class's ior)
_PER_RAY = dict(normal=10, grazing=12, inside=10, plane=12, box_face=10, box_inside=8, box_edge=5, box_corner=3, basis_normal=30,
                basis_mirror=30, scale=25, critical=3)
NONFINITE_EVERY = 3   # every third hit ray of the general classes also meets two materials of the non-finite set

_cases = None


def cases(seed=20260402):
    """The table of the shade and glass-sequence wrappers, from the rays the reference hits.  dict(n; objs DEVOBJ [n]; t f64 [n]; hit
    f64 [n, 8]: ora_hit's record; ray f64 [n, 6]; mat i32 [n]; state u64 [n]; cls, tag, obj i32 [n]; typ i32 [n]: converted type;
    rays: the generated rays with `ok` i32, for the drop shares).  n is no multiple of 64."""
    global _cases
    if _cases is not None:
        return _cases
    ora = _ora()
    M = materials()
    G = generated_rays()
    ok, hit = ora.hits(G["kind"], G["a"], G["b"], G["radius"], G["ray"], 0.001, MAXF)
    # a (scale, object, origin) combination the reference does not hit with at least three rays in four is no source of cases
    is_scale = G["cls"] == CLASSES.index("scale")
    combos = {}
    for tag in np.unique(G["tag"][is_scale]):
        m = is_scale & (G["tag"] == tag)
        combos[int(tag)] = (int(ok[m].sum()), int(m.sum()))
    dead = np.array([t for t, (h, k) in combos.items() if 4 * h < 3 * k])
    G["kept"] = ~(is_scale & np.isin(G["tag"], dead))
    G["ok"], G["combos"] = ok, combos
    ok = ok * G["kept"]
    r = np.random.default_rng(seed)
    fin = np.flatnonzero(M["finite"])
    nonfin = np.flatnonzero(~M["finite"])
    by_type = [fin[M["typ"][fin] == t] for t in range(5)]
    ray_i, mat_i = [], []
    for gi in np.flatnonzero(ok):
        cls = CLASSES[G["cls"][gi]]
        k = _PER_RAY[cls]
        if cls == "critical":
            ior = CRITICAL_IORS[G["tag"][gi]]
            pool = by_type[DIELECTRIC][M["conv"][by_type[DIELECTRIC], 5] == ior]
            ms = pool[r.integers(0, len(pool), k)]
        elif cls in ("basis_normal", "basis_mirror"):   # two thirds lambert and metal
            ms = np.concatenate([by_type[LAMBERT][r.integers(0, len(by_type[LAMBERT]), k // 3)],
                                 by_type[METAL][r.integers(0, len(by_type[METAL]), k // 3)], fin[r.integers(0, len(fin), k - 2 * (k // 3))]])
        elif cls == "scale":                            # every type at every scale
            ms = np.concatenate([by_type[t][r.integers(0, len(by_type[t]), k // 5)] for t in range(5)])
        else:
            ms = fin[r.integers(0, len(fin), k)]
            if gi % NONFINITE_EVERY == 0:
                ms = np.concatenate([ms, nonfin[r.integers(0, len(nonfin), 2)]])
        ray_i.append(np.full(len(ms), gi))
        mat_i.append(ms)
    ray_i, mat_i = np.concatenate(ray_i), np.concatenate(mat_i).astype(np.int32)
    if len(ray_i) % 64 == 0:
        ray_i, mat_i = ray_i[:-1], mat_i[:-1]
    n = len(ray_i)
    objs = np.zeros(n, DEVOBJ)
    objs["a"], objs["b"], objs["radius"] = G["a"][ray_i], G["b"][ray_i], G["radius"][ray_i]
    objs["radius_sq"] = objs["radius"] * objs["radius"]               # scene_to_world (ptcore.hip)
    with np.errstate(divide="ignore"):
        objs["inv_radius"] = 1.0 / objs["radius"]
    typ = M["typ"][mat_i]
    objs["kind"] = G["kind"][ray_i] | np.where(typ == DIELECTRIC, 0x100, 0)
    objs["mat"] = mat_i
    k = np.arange(n, dtype=np.uint64)
    L = ora.lib()
    state = np.array([L.ora_stream_init(seed, int(i) // 4, int(i) % 4) for i in k], np.uint64)   # running (pixel, sample)
    _cases = dict(n=n, objs=objs, t=hit[ray_i, 0].copy(), hit=hit[ray_i].copy(), ray=G["ray"][ray_i].copy(), mat=mat_i, state=state,
                  cls=G["cls"][ray_i], tag=G["tag"][ray_i], obj=G["obj"][ray_i], kind=G["kind"][ray_i], typ=typ, rays=G)
    return _cases


_reference = None


def reference():
    """ora_scatter_steps over cases(), and what the conditions and the sorted layout need of it: dict(ok, out [n, 12] = emitted,
    att, origin, direction; state; draws; front bool; mirror f64 [n, 3]: the mirror direction of the same ray (the reference's own
    scatter with a mirror material; NaN rows where that fails); branch i32 [n]: see BRANCHES)."""
    global _reference
    if _reference is not None:
        return _reference
    ora = _ora()
    T, M = cases(), materials()
    ref = ora.scatter_steps(M["arr"], T["mat"], T["hit"], T["ray"], T["state"])
    mirror_mat = int(np.flatnonzero((M["typ"] == MIRROR) & (M["set"] == "base"))[0])
    mir = ora.scatter_steps(M["arr"], np.full(T["n"], mirror_mat, np.int32), T["hit"], T["ray"], T["state"])
    ref["mirror"] = np.where(mir["ok"][:, None] != 0, mir["out"][:, 9:12], np.nan)
    ref["front"] = T["hit"][:, 7] != 0
    ref["branch"] = branches(T, M, ref)
    _reference = ref
    return ref


BRANCHES = ("emissive", "zero_dir", "lambert_smooth", "lambert_rough", "metal_smooth", "metal_rough", "metal_fallback", "mirror",
            "glass_tir", "glass_reflect", "glass_refract")


def branches(T, M, ref):
    """The branch of material.scatter each case took, read off the reference's results alone."""
    typ, ok, draws = T["typ"], ref["ok"] != 0, ref["draws"]
    rough = M["conv"][T["mat"], 4]
    is_mirror = np.all(same(ref["out"][:, 9:12], ref["mirror"]), axis=1) & ~np.isnan(ref["mirror"][:, 0])
    br = np.full(T["n"], -1, np.int32)
    B = BRANCHES.index
    br[typ == EMISSIVE] = B("emissive")
    br[(typ != EMISSIVE) & ~ok] = B("zero_dir")
    br[(typ == LAMBERT) & ok] = B("lambert_smooth")
    br[(typ == LAMBERT) & ok & (draws > 2)] = B("lambert_rough")
    br[(typ == METAL) & ok] = B("metal_smooth")
    br[(typ == METAL) & ok & (draws == 2)] = B("metal_rough")
    # (with a tiny alpha the blend can round to the mirror direction by itself, so only rough >= 0.1 counts as the fallback;
    # lenSq < 1e-8 needs non-finite operands: see the CPU test)
    br[(typ == METAL) & ok & (draws == 2) & is_mirror & (rough >= 0.1)] = B("metal_fallback")
    br[(typ == MIRROR) & ok] = B("mirror")
    br[(typ == DIELECTRIC) & ok & (draws == 0)] = B("glass_tir")
    br[(typ == DIELECTRIC) & ok & (draws == 1)] = B("glass_refract")
    br[(typ == DIELECTRIC) & ok & (draws == 1) & is_mirror] = B("glass_reflect")
    assert np.all(br >= 0)
    return br


def layouts(n, key):
    """The two lane layouts: table order, and sorted by `key` (stable), as index arrays."""
    return dict(table=np.arange(n), sorted=np.argsort(key, kind="stable"))


# ---------------------------------------------------------------- reflect_vec
def reflect_table(seed=20260403):
    """(v, n) f64 [m, 3]: the unit directions and face normals of the cases, then the same rescaled and with specials planted."""
    T = cases()
    r = np.random.default_rng(seed)
    sel = r.permutation(T["n"])[:6000]
    d = T["ray"][sel, 3:6]
    with np.errstate(all="ignore"):
        v = d / np.sqrt(np.sum(d * d, axis=1, keepdims=True))
    nrm = T["hit"][sel, 4:7]
    vs, ns = [v, v * 1e150, v * 1e-160, v * 1e200, v], [nrm, nrm, nrm * 1e-160, nrm * 1e200, nrm * 3.0]
    sp = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, MAXF, 1.0])
    vv, nn = r.choice(sp, (999, 3)), r.choice(sp, (999, 3))
    vv[::2], nn[1::3] = v[:500], nrm[:333]
    v, nrm = np.vstack(vs + [vv]), np.vstack(ns + [nn])
    assert len(v) % 64 != 0
    return np.ascontiguousarray(v), np.ascontiguousarray(nrm)


# ---------------------------------------------------------------- the exit epilogue
def exit_table(seed=20260404):
    """dict(n, mat, best i32 [n], tmax f64 [n], ray f64 [n, 6], att f64 [n, 3] = 1, 1, 1 as the callers give it): every dielectric of
    the table, finite or not, with best = -1 and >= 0, tmax of 1e-4, 1, 1e3, 1e300 and directions of three lengths."""
    M = materials()
    r = np.random.default_rng(seed)
    diel = np.flatnonzero(M["typ"] == DIELECTRIC)
    mat, best, tmax, ray = [], [], [], []
    for m in diel:
        for b in (-1, 0, 5):
            for t in (1e-4, 1.0, 1e3, 1e300):
                for s in (1.0, 1e-150, 1e150):
                    mat.append(m); best.append(b); tmax.append(t)
                    ray.append(np.concatenate([r.uniform(-2, 2, 3), _unit(r, 1)[0] * s]))
    n = len(mat) - (len(mat) % 64 == 0)
    return dict(n=n, mat=np.array(mat[:n], np.int32), best=np.array(best[:n], np.int32), tmax=np.array(tmax[:n]), ray=np.array(ray[:n]),
                att=np.ones((n, 3)))


# ---------------------------------------------------------------- roulette
ROULETTE_DEPTHS = (1, 2, 3, 4, 50)
ROULETTE_T = ((0.7, 0.5, 0.9), (0.0, 0.0, 0.0), (1e308, 1e308, 1e308), (float("nan"), 0.5, 0.25))
ROULETTE_CLASSES = ("ended_small", "ended_draw", "survived_max", "survived_095", "no_draw_deep", "ended_depth0", "nan_att", "draw_equals_prob")


def roulette_table(seed=20260405):
    """dict(n, depth i32 [n], att, T f64 [n, 3], state u64 [n]): attenuations from the albedo list and a few more, alone in every
    component in turn (the maximum sits there) and in all three."""
    vals = ALBEDOS + (0.5, 0.3, 2e-6, 0.949, 0.96, float("nan"), float("inf"))
    trip = []
    for v in vals:
        trip.append((v, v, v))
        for k in range(3):
            t = [v / 2, v / 4, v / 8]
            t[k] = v
            trip.append(tuple(t))
    depth, att, T = [], [], []
    for d in ROULETTE_DEPTHS:
        for a in trip:
            for tt in ROULETTE_T:
                for _ in range(6):
                    depth.append(d); att.append(a); T.append(tt)
    L = _ora().lib()
    state = [L.ora_stream_init(seed, i // 3, i % 3) for i in range(len(depth))]
    # the draw exactly at the survival probability, and one ulp to either side of it: the attenuation's maximum is the number the
    # case's own stream gives next (xi > rrProb is false at equality: the path survives)
    for j in range(150):
        st = L.ora_stream_init(seed + 1, j, 0)
        c = C.c_uint64(st)
        xi = L.ora_stream_next(C.byref(c))
        for v in (xi, down(xi), up(xi)):
            a = [v / 2, v / 4, v / 8]
            a[j % 3] = v
            depth.append(1 + j % 3); att.append(tuple(a)); T.append(ROULETTE_T[0]); state.append(st)
    n = len(depth) - (len(depth) % 64 == 0)
    return dict(n=n, depth=np.array(depth[:n], np.int32), att=np.array(att[:n]), T=np.array(T[:n]), state=np.array(state[:n], np.uint64))


def roulette_classes(R, ref):
    """bool [n] per name of ROULETTE_CLASSES, from the inputs and the reference's results."""
    ora = _ora()
    L = ora.lib()
    mx = np.array([L.ora_max(a[0], L.ora_max(a[1], a[2])) for a in R["att"]])
    deep, e, nd = R["depth"] > 3, ref["ended"], ref["draws"]
    nan = np.isnan(R["att"]).any(axis=1)
    xi = np.array([L.ora_stream_next(C.byref(C.c_uint64(int(st)))) for st in R["state"]])   # what a draw from the case's state gives
    with np.errstate(invalid="ignore"):
        prob = np.minimum(mx, 0.95)
    return dict(ended_small=(e == 1) & (nd == 0), ended_draw=(e == 2) & (nd == 1),
                survived_max=~deep & np.isin(e, (0, 3)) & (nd == 1) & (mx < 0.95), survived_095=~deep & np.isin(e, (0, 3)) & (nd == 1) & (mx >= 0.95),
                no_draw_deep=deep & (nd == 0) & (e == 0), ended_depth0=e == 3, nan_att=nan, draw_equals_prob=(nd == 1) & (xi == prob))
