"""The scenes and ray tables of ray_inject_support.py with every length multiplied by 2^k, shared by test_scaled_scenes_cpu.py (no
GPU: the inputs are what they claim, through the oracle) and test_scaled_scenes_gpu.py (every scaled ray through the kernels).

Every culled scan keeps FP32 bounds of the objects, built on B = max(1, largest |coordinate|) and m = B / 4096 (build_broad in
csrc/ptcore.hip, scene_margin in csrc/pt_bvh.h).  The constants around them were reasoned for B of about 10; the scales K put B on
either side of each:
  floor                  8 * 2^k < 1: B stays 1, the margin 2^-12 dwarfs the scene (k = -140: coordinates are FP32 denormals)
  ordinary               1 <= B and B^2 <= FLT_MAX
  fp32 squares overflow  B^2 > FLT_MAX (B >= 2^64): d2 of far spheres, then rm2 of large and of all spheres, are infinite in FP32
  keep all               1e30 <= B < 1e37: B is taken for infinite, every bound is unbounded, every object a candidate
  plain loop             B >= 1e37 (the wall reaches B exactly): scene_prepare sends the world to the reference's own loop
A power of two scales every FP64 coordinate exactly (nothing over- or underflows for |k| <= 140 but what SIMILAR_LIMITS names), so
every designed coincidence, tangency and ulp relation of the base scenes survives, and the oracle's first hits of the similar family
are those of k = 0, id for id."""
from __future__ import annotations

import copy

import numpy as np

import ray_inject_support as S

K = (-140, -40, -4, -3, 40, 60, 61, 64, 90, 96, 97, 119, 120, 130)
SCENES = ("bitmask", "grouped", "bvh")
TABLES = ("near geometry", "incoherent", "far origins", "mixed", "components")   # "length" is about |d|: covered at B = 8
FAMILIES = ("similar", "unit")
BANDS = ("floor", "ordinary", "fp32 squares overflow", "keep all", "plain loop")
UNIT_MIN_K = -4          # below it every t of the unit family is under the reference's tMin = 0.001 (t = 2^k t0, t0 of order 10)
KEEP_ALL = 1e30          # build_broad, scene_margin, pt_walk32.h
PLAIN_LOOP = 1e37        # the `fin` rule of scene_prepare
SQUARES = float(np.sqrt(np.float64(S.FLT_MAX)))   # 2^64 (1 - 2^-25): B = 2^64 is the first scale whose square is infinite in FP32
# scales of the other walkers and of the feature walk (the "bvh" scene)
WALKER_K = (-40, 61, 90, 96, 97, 119, 120)


def scaled_doc(doc: dict, k: int) -> dict:
    """doc with every length times 2^k, exactly: object positions and sizes (planes are objects), the camera's position, target,
    focus_dist and aperture.  Materials, sky, fov and up stay."""
    s = 2.0 ** k
    out = copy.deepcopy(doc)
    for o in out["objects"]:
        for key in ("position", "size"):
            o[key] = {c: float(v) * s for c, v in o[key].items()}
    cam = out["camera"]
    for key in ("position", "target"):
        cam[key] = {c: float(v) * s for c, v in cam[key].items()}
    for key in ("focus_dist", "aperture"):
        cam[key] = float(cam[key]) * s
    return out


def scaled_rays(table, k: int, family: str) -> np.ndarray:
    """[n][6]: origins times 2^k; directions times 2^k too ("similar": every t is the unscaled ray's, a = 4^k a0) or as they are
    ("unit": a = a0, t = 2^k t0)."""
    assert family in FAMILIES, family
    s = 2.0 ** k
    out = np.array(table, np.float64)
    with np.errstate(all="ignore"):
        out[:, 0:3] *= s
        if family == "similar":
            out[:, 3:6] *= s
    return np.ascontiguousarray(out)


def families(k: int):
    return FAMILIES if k >= UNIT_MIN_K else ("similar",)


def coordinate(k: int) -> float:
    """The scaled scene's largest |coordinate|: the wall's 8 * 2^k."""
    return S.BOUND * 2.0 ** k


def bound(k: int) -> float:
    """B of the scaled scenes as build_broad leaves it: max(1, 8 * 2^k), infinite from 1e30 on."""
    b = max(1.0, coordinate(k))
    return b if b < KEEP_ALL else float("inf")


def band(k: int) -> str:
    c = coordinate(k)
    if c < 1.0:
        return "floor"
    if c >= PLAIN_LOOP:
        return "plain loop"
    if c >= KEEP_ALL:
        return "keep all"
    return "fp32 squares overflow" if c > SQUARES else "ordinary"


def is_trusted(rays, k: int) -> np.ndarray:
    """`trust` of csrc/pt_kernels.h restated: fa (a from the FP32 direction) in (1e-30, 1e30) and every FP32 |origin component| within
    origin_bound = (float)min(4 B, 3e38)."""
    ob = np.float32(min(4.0 * bound(k), 3.0e38))
    with np.errstate(all="ignore"):
        return S.is_trusted_length(rays) & (np.abs(rays[:, 0:3].astype(np.float32)).max(axis=1) <= ob)


def similar_trusted(k: int) -> bool:
    """Unit directions times 2^k: fa = 4^k, inside (1e-30, 1e30) for |k| <= 49 (4^49 = 3.2e29, 4^50 = 1.3e30; 4^-49 = 3.2e-30,
    4^-50 = 7.9e-31; at k = -140 the FP32 square is zero)."""
    return abs(k) <= 49


def overflows_in_fp64(table, k: int, family: str) -> np.ndarray:
    """[n] bool: rows on which the reference's own FP64 arithmetic leaves the finite range although the row is finite -- the only
    rows the similarity anchor excuses, by this predicate on the inputs alone.  objects.go:41-48 forms b = oc.d, c = oc.oc - r^2
    and b b - a c: with |o| <= M and a = d.d, every term is at most 3 M^2 a (and c at most 3 M^2), so nothing overflows while
    3 M^2 max(a, 1) < DBL_MAX / 4; and the slab products of a box stay finite with it.  At k = 0 M is at most 2e100 (the tame
    limit's rows of "far origins") and a about 1: 1.2e201.  Scaled, the similar family multiplies that by 16^k: rows with a
    component of 1e100 overflow from k = 90 on.  The unit family multiplies by 4^k and never gets there for k <= 130."""
    r = scaled_rays(table, k, family)
    with np.errstate(all="ignore"):
        m = S.omax(r) + coordinate(k)
        a = S.dir_a(r)
        worst = 3.0 * m * m * np.maximum(a, 1.0)
        lim = float(np.finfo(np.float64).max) / 4.0
        return S.is_finite(np.asarray(table, float)) & ~(worst < lim)


def underflows_in_fp64(table, k: int, family: str) -> np.ndarray:
    """[n] bool: finite rows a component of whose scaled ray is no longer 2^k times the original (a subnormal direction component of
    the "components" table times 2^k < 1 rounds to zero or to another subnormal): scaling is not exact for them."""
    t = np.asarray(table, np.float64)
    r = scaled_rays(t, k, family)
    with np.errstate(all="ignore"):
        back = r.copy()
        back[:, 0:3] *= 2.0 ** -k
        if family == "similar":
            back[:, 3:6] *= 2.0 ** -k
        same = (back == t) | (np.isnan(back) & np.isnan(t))
        return S.is_finite(t) & ~np.all(same, axis=1)


PLANE_DENOM = 1e-6   # objects.go:103: a plane answers only while |n.d| >= 1e-6 -- the reference's one absolute test on a direction


def without_planes(doc: dict) -> dict:
    """doc with every plane replaced by a box of size zero, which no ray hits (objects.go:176: t1 <= t0): indices stay."""
    out = copy.deepcopy(doc)
    for o in out["objects"]:
        if o["type"] == "plane":
            o["type"], o["size"] = "box", S.V(0, 0, 0)
    return out


def anchor_ids(oracle, scene_name: str, table_name: str):
    """(first hits at k = 0, the same with the planes taken out) of a table.  Cached."""
    key = ("anchor", scene_name, table_name)
    if key not in _cache:
        doc, tab = S.scene_doc(scene_name), S.classes()[table_name]
        _cache[key] = (S.first_hits(oracle, doc, tab), S.first_hits(oracle, without_planes(doc), tab))
    return _cache[key]


def similar_expectation(oracle, scene_name: str, table_name: str, k: int):
    """What the oracle's first hits of the similar family at scale k must be, from k = 0: (want [n], exact [n] bool, gained [n] bool).
    Every t of a similar ray is the unscaled ray's and every FP64 operation scales exactly, so the ids are those of k = 0 -- but for
    the plane's |n.d| >= 1e-6, which is absolute: n.d is the y component of the direction, 2^k times the original.
      * still accepted, or still refused: the id of k = 0;
      * refused now, accepted at k = 0 (k < 0): the id of k = 0 in the scene without its planes;
      * accepted now, refused at k = 0 (k > 0: the flat rays of "components"): the plane is one more candidate, at
        t = (p_y - o_y) / d_y -- `gained`: the id is that of k = 0 or the plane's, and the plane's only if that t is at least tMin.
    `exact` is false on the rows the comparison excuses, by predicates on the inputs alone: not finite, a component that scaling
    rounds (underflows_in_fp64), or FP64 products of the reference beyond DBL_MAX (overflows_in_fp64)."""
    tab = S.classes()[table_name]
    r = rays_of(table_name, k, "similar")
    base, base_np = anchor_ids(oracle, scene_name, table_name)
    with np.errstate(all="ignore"):
        now, then = np.abs(r[:, 4]) >= PLANE_DENOM, np.abs(tab[:, 4]) >= PLANE_DENOM
    want = np.where(now, base, base_np)
    exact = S.is_finite(tab) & ~underflows_in_fp64(tab, k, "similar") & ~overflows_in_fp64(tab, k, "similar")
    return want, exact, now & ~then


def nonfinite_rows(oracle, doc, rays, depth=S.DEPTH) -> int:
    """Rows of a table whose radiance by ora_sample_ray holds a NaN or an infinity: the rows a comparison cannot hold to a number."""
    rgb, _, _ = oracle.sample_rays(oracle.Scene(doc), len(rays), 1, 1, depth, S.SEED, rays)
    return int(np.count_nonzero(~np.all(np.isfinite(rgb), axis=1)))


def far_sides(rays, k: int) -> dict:
    """Finite rows of a table on either side of 3.5 B, 4 B and the far threshold 2034.5 B, by the restated predicates with the bound
    as it is at that scale (infinite in the keep-all band: nothing is beyond it)."""
    b = bound(k)
    fin = S.is_finite(rays)
    with np.errstate(all="ignore"):
        clip, orig = S.beyond_clip(rays, b), S.beyond_origin_bound(rays, b)
        far = S.is_far(rays, b) if np.isfinite(b) else np.zeros(len(rays), bool)
    n = lambda m: int(np.count_nonzero(fin & m))  # noqa: E731
    return {"3.5B": (n(~clip), n(clip)), "4B": (n(~orig), n(orig)), "2034.5B": (n(clip & ~far), n(far))}


def walk_odd(rays, k: int) -> np.ndarray:
    """feature_inject_support.walk_odd with the bound as it is at scale k.  The kernel's test (csrc/pt_feature_walk.h) is
    1e-29 < a < 1e29, |o| <= clip_bound = 3.5 B and |o| <= 0.99 origin_bound (bvh_ray_trusted); for a finite B the first bound on the
    origin is the tighter one, which is fi.walk_odd; in the keep-all band 3.5 B is infinite and 0.99 * (float)3e38 is what is left."""
    import feature_inject_support as fi

    b = bound(k)
    if np.isfinite(b):
        return fi.walk_odd(rays, b)
    with np.errstate(all="ignore"):
        return fi.walk_odd(rays, b) | ~(S.omax(rays) <= 0.99 * float(np.float32(3.0e38)))


def walk_layouts(rays, k: int) -> dict:
    """{layout: (table, waves that hold an odd row)} of a scaled table: as it is, and fi.walk_layout's stable partition (the
    non-odd rows first, wave by wave) by walk_odd at that scale."""
    odd = walk_odd(rays, k)
    order = np.concatenate([np.flatnonzero(~odd), np.flatnonzero(odd)])
    walk = S.to_table(np.asarray(rays)[order])
    waves = lambda t: len(np.unique(S.waves_of_table(t)[walk_odd(t, k)]))  # noqa: E731
    return {"original": (rays, waves(rays)), "walk": (walk, waves(walk))}


_cache = {}


def doc_of(scene_name: str, k: int) -> dict:
    key = ("doc", scene_name, k)
    if key not in _cache:
        _cache[key] = scaled_doc(S.scene_doc(scene_name), k)
    return _cache[key]


def rays_of(table_name: str, k: int, family: str) -> np.ndarray:
    key = ("rays", table_name, k, family)
    if key not in _cache:
        r = scaled_rays(S.classes()[table_name], k, family)
        r.setflags(write=False)
        _cache[key] = r
    return _cache[key]


def report_line(what, scene_name, k, rays, ids, segments, delta) -> str:
    """One line per (test, scene, scale, table, family) in the style of test_ray_inject_gpu.py's."""
    fin = S.is_finite(rays)
    return ("scaled scenes: %-28s on %-8s k %4d [%s]: %d rays, %d hit / %d miss / %d non-finite, trusted %.3f, %d segments, scan-mismatch delta %s"
            % (what, scene_name, k, band(k), len(rays), np.count_nonzero(fin & (ids >= 0)), np.count_nonzero(fin & (ids < 0)),
               np.count_nonzero(~fin), float(np.mean(is_trusted(rays, k))), segments, delta))
