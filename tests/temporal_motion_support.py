"""Helpers of the displaced-reprojection and object-id tests (test_temporal_motion_cpu.py, test_temporal_motion_gpu.py,
test_object_ids_gpu.py): builds tests/object_ids_reference.c -- the oracle-side restatement of the object index plane
--, a host build of csrc/pt_temporal.h with the index plane and the motion table wired through (temporal_clip_support's shim with
those additions) and tests/temporal_motion_probe.hip; holds `Restatement`, the restatement of pt_temporal's per-pixel model WITH
step 4a in plain Python floats, written from the header comment of pt_temporal.h and sharing nothing with the product's headers;
and makes the sequences: shipped scenes with one sphere and one box moved per frame, with or without the camera moving as well."""
from __future__ import annotations

import copy
import ctypes as C
import json
import math
import os
import subprocess
import tempfile

import numpy as np

import atrous_support as at
import temporal_clip_support as tc
import temporal_support as ts
from conftest import scene_path
from fog_support import CFLAGS, CSRC, CXXFLAGS, ORACLE, ROOT, ptr

GAMMA = tc.GAMMA
PROBE_SOURCE = os.path.join(ROOT, "tests", "temporal_motion_probe.hip")

# one sphere and one box of each scene, and what each moves by per frame
MOVES = {"example_simple": {6: (0.16, 0.0, 0.0), 9: (0.16, 0.0, 0.0)},
         "metal_glass_room": {10: (0.16, 0.0, 0.05), 6: (-0.12, 0.0, 0.08)}}

_vp = C.c_void_p
_libs = {}
_cache = {}
_dir = None
_FRAME_ARGS = ts._FRAME_ARGS + [_vp, _vp, C.c_int32]


# ---------------------------------------------------------------- the object index plane on the oracle
def ids_reference():
    """object_ids_reference.c linked against oracle/libptoracle.so."""
    if "ids" not in _libs:
        from oracle import ora

        ora.lib()
        out = os.path.join(at._build_dir(), "libobjectidsref.so")
        subprocess.run(["gcc", *CFLAGS, "-shared", "-I", ORACLE, os.path.join(ROOT, "tests", "object_ids_reference.c"), "-o", out,
                        "-L", ORACLE, "-Wl,-rpath," + ORACLE, "-lptoracle", "-lm"], check=True, capture_output=True)
        L = C.CDLL(out)
        L.oid_frame.argtypes = [_vp, _vp, _vp, _vp]
        L.oid_rays.argtypes = [_vp, C.c_int64, _vp, _vp, _vp]
        _libs["ids"] = L
    return _libs["ids"]


def oracle_ids(sc, w: int, h: int, seed: int):
    """(ids int32 [H, W], tie bool [H, W]) of sample 0 of every pixel of the oracle scene `sc` (ora.Scene)."""
    from oracle import ora

    cfg = ora.OraConfig(w, h, 1, 1, seed, 1, 0)
    ids, tie = np.zeros((h, w), np.int32), np.zeros((h, w), np.uint8)
    ids_reference().oid_frame(C.byref(sc.c), C.byref(cfg), ptr(ids), ptr(tie))
    return ids, tie.astype(bool)


def oracle_ids_of_rays(sc, rays):
    """(ids int32 [n], tie bool [n]) of chosen rays float64 [n, 6]."""
    rays = np.ascontiguousarray(rays, np.float64)
    ids, tie = np.zeros(len(rays), np.int32), np.zeros(len(rays), np.uint8)
    ids_reference().oid_rays(C.byref(sc.c), len(rays), ptr(rays), ptr(ids), ptr(tie))
    return ids, tie.astype(bool)


# ---------------------------------------------------------------- sequences with moved objects
def doc_with_an_unknown_object(name: str, at_index: int = 5) -> dict:
    """The shipped scene with an object of a type nobody knows in the middle of the list: scene index != world index behind it."""
    with open(scene_path(name), "r", encoding="utf-8") as fh:
        doc = json.load(fh)
    ghost = copy.deepcopy(doc["objects"][at_index])
    ghost["type"] = "torus"
    doc["objects"].insert(at_index, ghost)
    return doc


def motion_doc(name: str, f: int, moves=None, cam: float = 0.0) -> dict:
    """The shipped scene's document at frame f: object i at its position + f * moves[i], the camera moved sideways by f * cam steps
    of temporal_support.moved_doc."""
    doc = ts.moved_doc(name, f * cam)
    for i, d in (MOVES[name] if moves is None else moves).items():
        p = doc["objects"][i]["position"]
        for k, ax in enumerate("xyz"):
            p[ax] = float(p[ax]) + f * d[k]
    return doc


def doc_delta(prev: dict, cur: dict) -> np.ndarray:
    """[n, 3]: the positions of cur's objects minus those of prev's."""
    return np.array([[float(b["position"][ax]) - float(a["position"][ax]) for ax in "xyz"] for a, b in zip(prev["objects"], cur["objects"])])


def ora_scene_of_doc(key, doc):
    from oracle import ora

    if ("ora", key) not in _cache:
        _cache[("ora", key)] = ora.Scene(doc)
    return _cache[("ora", key)]


def oracle_frame(name: str, f: int, w: int, h: int, spp: int, depth: int, seed: int, k: int = 4, moves=None, cam: float = 0.0) -> dict:
    """Frame f of a moving sequence from oracle samples only: dict(S, Q, n, feats, cam, ids, tie, delta, doc), computed once.  delta
    = the table against frame f - 1 (None for f = 0)."""
    from oracle import ora

    mv = MOVES[name] if moves is None else moves
    key = ("frame", name, f, w, h, spp, depth, seed, k, repr(sorted(mv.items())), cam)
    if key not in _cache:
        doc = motion_doc(name, f, mv, cam)
        sc = ora_scene_of_doc(key, doc)
        cfg = ora.OraConfig(w, h, spp, depth, seed, 1, 0)
        S, Q = np.zeros((h, w, 3)), np.zeros((h, w, 3))
        ts.reference().tr_sums(C.byref(sc.c), C.byref(cfg), ptr(S), ptr(Q))
        ids, tie = oracle_ids(sc, w, h, seed)
        for a in (S, Q, ids, tie):
            a.setflags(write=False)
        _cache[key] = dict(S=S, Q=Q, n=spp, feats=at.ref_features(sc, w, h, spp, depth, seed, k), cam=ts.camera_of(sc, w, h), ids=ids,
                           tie=tie, delta=doc_delta(motion_doc(name, f - 1, mv, cam), doc) if f > 0 else None, doc=doc)
    return _cache[key]


def sequence(name: str, frames: int, w: int, h: int, spp: int = 16, depth: int = 4, seed0: int = 100, cam: float = 0.0, moves=None):
    return [oracle_frame(name, f, w, h, spp, depth, seed0 + f, moves=moves, cam=cam) for f in range(frames)]


# ---------------------------------------------------------------- the host build and the probe
def shim_source() -> str:
    """temporal_clip_support's shim with the index plane and the motion table: ids, delta, ndelta behind `place`, counts[5] = moved,
    counts[6] = moved_reprojected, and `place` the displaced placement."""
    s = tc.shim_source()
    r = tc._replace_once
    s = r(s, "double *var, uint8_t *rgba, double *noise, uint64_t *counts, double *place) {",
          "double *var, uint8_t *rgba, double *noise, uint64_t *counts, double *place, const int32_t *ids, const double *delta, int32_t ndelta) {")
    s = r(s, "counts[3] = counts[4] = 0;", "counts[3] = counts[4] = counts[5] = counts[6] = 0;")
    s = r(s, "bool clipped = false;\n", "bool clipped = false;\n            const double *disp = ptt::displacement(ids, delta, ndelta, i, hit);\n")
    s = r(s, "v[0][i], len, &clipped);", "v[0][i], len, &clipped, disp);")
    s = r(s, "counts[4] += clipped;", "counts[4] += clipped;\n            counts[5] += disp && st != ptt::ST_BAD;\n"
                                      "            counts[6] += disp && st == ptt::ST_REPROJECTED;")
    s = r(s, "ptt::reproject(V, s.cam, x, y, hit, g[i].z, fx, fy, zexp)", "ptt::reproject(V, s.cam, x, y, hit, g[i].z, fx, fy, zexp, disp)")
    return s


def product_host():
    """csrc/pt_temporal.h built for the host with g++, clip and motion wired through."""
    if "shim" not in _libs:
        d = at._build_dir()
        src = os.path.join(d, "temporal_motion_shim.cpp")
        with open(src, "w") as f:
            f.write(shim_source())
        out = os.path.join(d, "libtemporalmotionshim.so")
        subprocess.run(["g++", *CXXFLAGS, "-shared", "-I", CSRC, src, "-o", out], check=True, capture_output=True)
        L = C.CDLL(out)
        L.shim_new.restype = _vp
        L.shim_free.argtypes = [_vp]
        L.shim_reset.argtypes = [_vp]
        L.shim_read.argtypes = [_vp, _vp, _vp, _vp]
        L.shim_frame.argtypes = _FRAME_ARGS
        _libs["shim"] = L
    return _libs["shim"]


def compile_probe(source: str = PROBE_SOURCE, include: str = CSRC) -> str:
    """Path of the probe's shared library, compiled with the library's compiler and flags into a temporary directory."""
    global _dir
    from path_trace_golang_amd import build

    if _dir is None:
        _dir = tempfile.mkdtemp(prefix="tmprobe_")
    out = os.path.join(_dir, "libtemporalmotionprobe.so")
    if not os.path.exists(out):
        r = subprocess.run([build.HIPCC, *build.HIP_FLAGS, "-shared", "-I", include, "-I", os.path.join(ROOT, "tests"), source, "-o", out],
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("temporal motion probe does not compile:\n%s\n%s" % (r.stdout, r.stderr))
    return out


def probe():
    """The probe, loaded after torch so that the process keeps one HIP runtime."""
    if "probe" not in _libs:
        import torch  # noqa: F401

        L = C.CDLL(compile_probe())
        L.motion_probe_new.restype = _vp
        L.motion_probe_new.argtypes = []
        L.motion_probe_free.argtypes = [_vp]
        L.motion_probe_free.restype = None
        L.motion_probe_reset.argtypes = [_vp]
        L.motion_probe_reset.restype = None
        L.motion_probe_read.argtypes = [_vp, _vp, _vp, _vp, _vp]
        L.motion_probe_read.restype = C.c_int
        L.motion_probe_frame.argtypes = _FRAME_ARGS
        L.motion_probe_frame.restype = C.c_int
        _libs["probe"] = L
    return _libs["probe"]


class MotionAccumulator:
    """One history with clip and motion: on the host build of the product's header ("host") or the probe's device history ("gpu").
    frame(..., ids=, delta=) returns temporal_clip_support.ClipAccumulator.frame's dict plus `moved` and `moved_reprojected`."""

    def __init__(self, kind: str):
        self.kind = kind
        if kind == "host":
            L = product_host()
            self._new, self._free, self._reset, self._readfn, self._frame = L.shim_new, L.shim_free, L.shim_reset, L.shim_read, L.shim_frame
        else:
            L = probe()
            self._new, self._free, self._reset, self._readfn, self._frame = (L.motion_probe_new, L.motion_probe_free, L.motion_probe_reset,
                                                                              L.motion_probe_read, L.motion_probe_frame)
        self.h = self._new()

    def close(self):
        if self.h:
            self._free(self.h)
            self.h = None

    __del__ = close

    def reset(self):
        self._reset(self.h)

    def read(self, w: int, h: int):
        mean, var, ln = np.zeros((h, w, 3)), np.zeros((h, w)), np.zeros((h, w), np.int32)
        if self.kind == "gpu":
            valid = C.c_int32(-1)
            rc = self._readfn(self.h, ptr(mean), ptr(var), ptr(ln), C.byref(valid))
            if rc != 0:
                raise RuntimeError("motion_probe_read: status %d" % rc)
            return (mean, var, ln) if valid.value else None
        return (mean, var, ln) if self._readfn(self.h, ptr(mean), ptr(var), ptr(ln)) else None

    def frame(self, S, Q, n, feats, cam, counts=None, filter=None, gamma=0.0, ids=None, delta=None, ndelta=None, **tcfg) -> dict:
        t = dict(ts.T_DEFAULTS, **tcfg)
        S = np.ascontiguousarray(S, np.float64)
        Q = np.ascontiguousarray(Q, np.float64)
        H, W = S.shape[:2]
        cnt = np.ascontiguousarray(counts, np.uint32) if counts is not None else None
        f = [np.ascontiguousarray(a, np.float64) for a in feats]
        cam = np.ascontiguousarray(cam, np.float64)
        tcv = np.array([t["alpha"], t["tol_z"], t["n_min"], t["tol_a"], float(t["max_len"]), float(gamma)], np.float64)
        fc = dict(at.DEFAULTS, **filter) if filter is not None else None
        sig = np.array([fc[k] for k in ("sigma_l", "sigma_n", "sigma_z", "sigma_a")] if fc else [1.0, 0, 0, 0], np.float64)
        mean, var = np.zeros((H, W, 3)), np.zeros((H, W))
        rgba = np.zeros((H, W, 4), np.uint8)
        noise = np.zeros(3)
        cnts = np.zeros(7, np.uint64)
        place = np.zeros((H, W, 2))
        idv = np.ascontiguousarray(ids, np.int32) if ids is not None else None
        dv = np.ascontiguousarray(delta, np.float64) if delta is not None else None
        nd = (len(dv) if dv is not None else 0) if ndelta is None else ndelta
        rc = self._frame(self.h, W, H, ptr(S), ptr(Q), ptr(cnt) if cnt is not None else None, int(n), ptr(f[0]), ptr(f[1]), ptr(f[2]), ptr(cam),
                         ptr(tcv), int(fc["iterations"]) if fc else -1, ptr(sig), ptr(mean), ptr(var), ptr(rgba), ptr(noise), ptr(cnts), ptr(place),
                         ptr(idv) if idv is not None else None, ptr(dv) if dv is not None and dv.size else None, int(nd))
        if self.kind == "gpu" and rc != 0:
            raise RuntimeError("motion_probe_frame: status %d" % rc)
        hist = self.read(W, H)
        return dict(mean=mean, var=var, rgba=rgba, noise_before=float(noise[0]), noise_blended=float(noise[1]), noise_after=float(noise[2]),
                    reprojected=int(cnts[0]), disoccluded=int(cnts[1]), bad_pixels=int(cnts[2]), mean_len=float(cnts[3]) / (W * H),
                    clipped=int(cnts[4]), moved=int(cnts[5]), moved_reprojected=int(cnts[6]), place=place, hist_mean=hist[0], hist_var=hist[1],
                    hist_len=hist[2])


def assert_same_frame(a: dict, b: dict, tag="") -> None:
    """temporal_clip_support.assert_same_frame, and the two motion counts exactly."""
    tc.assert_same_frame(a, b, tag)
    for k in ("moved", "moved_reprojected"):
        assert a[k] == b[k], (tag, k, a[k], b[k])


def run_sequence(kind: str, frames, filter=None, gamma=0.0, motion="table", **tcfg):
    """Every frame of `frames` through one MotionAccumulator.  motion: "table" passes each frame's ids and delta, "zero" an all-zero
    table of the same shape, "none" nothing; a frame with reset = True resets the history first."""
    acc = MotionAccumulator(kind)
    try:
        out = []
        for f in frames:
            if f.get("reset"):
                acc.reset()
            ids, delta = None, None
            if motion != "none" and f.get("delta") is not None:
                ids, delta = f["ids"], (f["delta"] if motion == "table" else np.zeros_like(f["delta"]))
            out.append(acc.frame(f["S"], f["Q"], f["n"], f["feats"], f["cam"], f.get("counts"), filter, gamma, ids, delta, **tcfg))
        return out
    finally:
        acc.close()


# ---------------------------------------------------------------- the restatement, in plain Python floats
def _finite(x: float) -> bool:
    return x == x and x not in (math.inf, -math.inf)


def _dot(a, b) -> float:
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


class Restatement:
    """pt_temporal's per-pixel model (steps 1 - 9 of the header comment of csrc/pt_temporal.h, with 4a and 7a; no filter stage) on
    Python floats, which are IEEE doubles with +, -, *, / and math.sqrt correctly rounded.  One history; frame() takes the frame's
    raw sums, feature sums, camera (the first 12 of ora_camera_setup's doubles), and optionally ids [H][W] and delta [n][3]."""

    def __init__(self):
        self.hist = None  # dict(W, H, cam, c, var, len, N, A, z, hit) -- lists per pixel

    def reset(self):
        self.hist = None

    @staticmethod
    def _prep(S, Q, n, fn, fa, fd):
        n = float(n)
        c, v = [0.0] * 3, [0.0] * 3
        for k in range(3):
            c[k] = S[k] / n
            e = Q[k] / n - c[k] * c[k]
            if e < 0:
                e = 0.0
            v[k] = e / (n - 1.0)
        var = ((v[0] + v[1]) + v[2]) / 3.0
        bad = not (_finite(c[0]) and _finite(c[1]) and _finite(c[2]) and _finite(var))
        h = fd[1]
        N, A, z = [0.0] * 3, [0.0] * 3, 0.0
        if h != 0:
            N = [fn[k] / h for k in range(3)]
            A = [fa[k] / h for k in range(3)]
            z = fd[0] / h
        return c, var, bad, N, A, z, h > 0

    def frame(self, S, Q, n, feats, cam, counts=None, gamma=0.0, ids=None, delta=None, alpha=0.2, tol_z=0.1, n_min=0.9, tol_a=0.05,
              max_len=32) -> dict:
        S, Q = np.asarray(S, np.float64), np.asarray(Q, np.float64)
        H, W = S.shape[:2]
        Sl, Ql = S.reshape(-1, 3).tolist(), Q.reshape(-1, 3).tolist()
        fn, fa, fd = (np.asarray(a, np.float64).reshape(-1, 3).tolist() for a in feats)
        cnt = np.asarray(counts).reshape(-1).tolist() if counts is not None else None
        cam = [float(x) for x in np.asarray(cam)[:12]]
        org, ll, hor, ver = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
        idl = np.asarray(ids).reshape(-1).tolist() if ids is not None else None
        table = [[float(x) for x in row] for row in np.asarray(delta, np.float64).reshape(-1, 3)] if delta is not None else None
        hist = self.hist if self.hist is not None and self.hist["W"] == W and self.hist["H"] == H else None
        inv_width, inv_height = 1.0 / float(W - 1), 1.0 / float(H - 1)
        np_ = W * H
        out = dict(c=[None] * np_, var=[0.0] * np_, len=[0] * np_, N=[None] * np_, A=[None] * np_, z=[0.0] * np_, hit=[False] * np_)
        place = [[math.nan, math.nan] for _ in range(np_)]
        nrep = ndis = nbad = nclip = nmov = nmrp = 0
        for y in range(H):
            for x in range(W):
                i = y * W + x
                c, var, bad, N, A, z, hit = self._prep(Sl[i], Ql[i], cnt[i] if cnt is not None else n, fn[i], fa[i], fd[i])
                out["N"][i], out["A"][i], out["z"][i], out["hit"][i] = N, A, z, hit
                out["c"][i], out["var"][i] = list(c), var
                if bad:  # step 1
                    out["len"][i] = 0
                    nbad += 1
                    continue
                out["len"][i] = 1
                # step 4a's choice, counted whether or not there is a history
                row = None
                if table is not None and idl is not None and hit:
                    o = idl[i]
                    if 0 <= o < len(table) and (table[o][0] != 0 or table[o][1] != 0 or table[o][2] != 0):
                        row = table[o]
                        nmov += 1
                if hist is None:  # step 2
                    continue
                # step 3
                u = (float(x) + 0.5) * inv_width
                v = ((float(H - 1) - float(y)) + 0.5) * inv_height
                d = [((ll[k] + hor[k] * u) + ver[k] * v) - org[k] for k in range(3)]
                # steps 4, 4a
                ho, hl, hh, hv = hist["cam"][0:3], hist["cam"][3:6], hist["cam"][6:9], hist["cam"][9:12]
                zexp = 0.0
                if hit:
                    s = z / math.sqrt(_dot(d, d))
                    P = [org[k] + d[k] * s for k in range(3)]
                    if row is not None:
                        P = [P[k] - row[k] for k in range(3)]
                    q = [P[k] - ho[k] for k in range(3)]
                    zexp = math.sqrt(_dot(q, q))
                else:
                    q = d
                # step 5
                e = [hl[k] - ho[k] for k in range(3)]
                nrm = [hh[1] * hv[2] - hh[2] * hv[1], hh[2] * hv[0] - hh[0] * hv[2], hh[0] * hv[1] - hh[1] * hv[0]]
                den, num = _dot(q, nrm), _dot(e, nrm)
                found = den * num > 0
                if found:
                    s = num / den
                    pt = [q[k] * s - e[k] for k in range(3)]
                    pu = _dot(pt, hh) / _dot(hh, hh)
                    pv = _dot(pt, hv) / _dot(hv, hv)
                    fx = pu * float(W - 1) - 0.5
                    fy = (float(H - 1) - pv * float(H - 1)) + 0.5
                    found = _finite(fx) and _finite(fy) and -1.0 <= fx <= float(W) and -1.0 <= fy <= float(H)
                if found:
                    place[i] = [fx, fy]
                    # steps 6, 7
                    x0, y0 = math.floor(fx), math.floor(fy)
                    ax, ay = fx - float(x0), fy - float(y0)
                    sw = sv = 0.0
                    sc = [0.0, 0.0, 0.0]
                    L = None
                    for dy in (0, 1):
                        for dx in (0, 1):
                            xj, yj = x0 + dx, y0 + dy
                            if not (0 <= xj < W and 0 <= yj < H):
                                continue
                            j = yj * W + xj
                            w = (ax if dx else 1.0 - ax) * (ay if dy else 1.0 - ay)
                            if not (hist["len"][j] > 0 and hist["hit"][j] == hit and w > 0):
                                continue
                            if hit:
                                if not (abs(hist["z"][j] - zexp) <= tol_z * zexp):
                                    continue
                                if not (_dot(N, hist["N"][j]) >= n_min):
                                    continue
                                dr, dg, db = (A[k] - hist["A"][j][k] for k in range(3))
                                if not (dr * dr + dg * dg + db * db <= tol_a * tol_a):
                                    continue
                            sw = sw + w
                            for k in range(3):
                                sc[k] = sc[k] + w * hist["c"][j][k]
                            sv = sv + (w * w) * hist["var"][j]
                            L = hist["len"][j] if L is None or hist["len"][j] < L else L
                    found = sw > 0.01
                if not found:
                    ndis += 1
                    continue
                nrep += 1
                nmrp += row is not None
                cr = [sc[k] / sw for k in range(3)]
                vr = sv / (sw * sw)
                if gamma > 0:  # step 7a
                    s = var + vr
                    half = gamma * math.sqrt(s if s > 0 else 0.0)
                    changed = False
                    for k in range(3):
                        lo, hi = c[k] - half, c[k] + half
                        if cr[k] < lo:
                            cr[k], changed = lo, True
                        elif cr[k] > hi:
                            cr[k], changed = hi, True
                    nclip += changed
                # step 8
                r = 1.0 / float(L + 1)
                a = alpha if alpha > r else r
                out["c"][i] = [cr[k] + a * (c[k] - cr[k]) for k in range(3)]
                out["var"][i] = ((1.0 - a) * (1.0 - a)) * vr + (a * a) * var
                out["len"][i] = L + 1 if L + 1 < max_len else max_len
        self.hist = dict(out, W=W, H=H, cam=cam)  # step 9
        mean = np.array(out["c"], np.float64).reshape(H, W, 3)
        var = np.array(out["var"], np.float64).reshape(H, W)
        ln = np.array(out["len"], np.int32).reshape(H, W)
        return dict(mean=mean, var=var, hist_mean=mean, hist_var=var, hist_len=ln, reprojected=nrep, disoccluded=ndis, bad_pixels=nbad,
                    mean_len=float(sum(out["len"])) / np_, clipped=nclip, moved=nmov, moved_reprojected=nmrp,
                    place=np.array(place, np.float64).reshape(H, W, 2))


def assert_same_model(got: dict, want: dict, tag="") -> None:
    """A host-build (or device) run without a filter against the restatement: the output, the stored history and the placement bit
    for bit, len and every count exactly."""
    for k in ("mean", "var", "hist_mean", "hist_var", "place"):
        assert at.same_bits(got[k], want[k]), (tag, k, int(np.count_nonzero(~np.isclose(got[k], want[k], rtol=0, atol=0, equal_nan=True))))
    assert np.array_equal(got["hist_len"], want["hist_len"]), (tag, "len")
    for k in ("reprojected", "disoccluded", "bad_pixels", "clipped", "moved", "moved_reprojected"):
        assert got[k] == want[k], (tag, k, got[k], want[k])
    assert abs(got["mean_len"] - want["mean_len"]) <= 1e-12, (tag, "mean_len")


def restate_sequence(frames, gamma=0.0, motion="table", **tcfg):
    """run_sequence's twin on the restatement."""
    acc = Restatement()
    out = []
    for f in frames:
        if f.get("reset"):
            acc.reset()
        ids, delta = None, None
        if motion != "none" and f.get("delta") is not None:
            ids, delta = f["ids"], (f["delta"] if motion == "table" else np.zeros_like(f["delta"]))
        out.append(acc.frame(f["S"], f["Q"], f["n"], f["feats"], f["cam"], f.get("counts"), gamma, ids, delta, **tcfg))
    return out
