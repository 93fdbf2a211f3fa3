"""HIP backend: the plug-in that takes the place of the reference's
internal/engine/gpu package behind engine.RenderInto.

    gpu.Render(sc *scene.Scene, cfg gpu.RenderConfig, img *image.RGBA, progress func()) error
                                                   (/root/reference/internal/engine/gpu/gpu.go:2534)

`render` has that shape: it flattens the scene into the C ABI's plain structs,
renders through libptcore.so on the MI355X and fills `img` (H x W x 4 uint8, row 0 on
top) in place.  Errors raise (the Go binding returns them as `error`); there is no
CPU fallback here -- in the Go integration the fallback stays the reference's own CPU
engine (renderer.go:257-262).
"""
from __future__ import annotations

import copy
import ctypes as C
import math
import os
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np

from . import capi
from . import scene as scn

_MAT = {scn.MATERIAL_LAMBERT: capi.PT_MAT_LAMBERT, scn.MATERIAL_METAL: capi.PT_MAT_METAL,
        scn.MATERIAL_DIELECTRIC: capi.PT_MAT_DIELECTRIC, scn.MATERIAL_EMISSIVE: capi.PT_MAT_EMISSIVE,
        scn.MATERIAL_MIRROR: capi.PT_MAT_MIRROR}
_OBJ = {scn.OBJECT_SPHERE: capi.PT_OBJ_SPHERE, scn.OBJECT_PLANE: capi.PT_OBJ_PLANE, scn.OBJECT_BOX: capi.PT_OBJ_BOX,
        scn.OBJECT_SPHERE_LIGHT: capi.PT_OBJ_SPHERE_LIGHT}


# ---- the environment parsers of the *from_env rules (environ None = os.environ)
def _env_on(environ, key: str) -> bool:
    """1 / true / on / yes in any case, nothing else."""
    return (os.environ if environ is None else environ).get(key, "").lower() in ("1", "true", "on", "yes")


def _env_int(environ, key: str, lo: int, hi: Optional[int] = None) -> Optional[int]:
    """The integer the variable holds when it lies in [lo, hi] (hi None: no upper bound), else None."""
    try:
        i = int((os.environ if environ is None else environ)[key])
    except (KeyError, ValueError):
        return None
    return i if i >= lo and (hi is None or i <= hi) else None


def _env_positive(environ, key: str) -> Optional[float]:
    """The finite float > 0 the variable holds, else None."""
    try:
        f = float((os.environ if environ is None else environ)[key])
    except (KeyError, ValueError):
        return None
    return f if f > 0 and math.isfinite(f) else None


@dataclass
class RenderConfig:  # gpu.RenderConfig, gpu.go:227-232 (+ the stream seed)
    width: int = 0
    height: int = 0
    samples_per_px: int = 0
    max_depth: int = 0
    seed: int = 1
    spp_chunk: int = 0
    flags: int = 0


class FlatScene:
    """pt_scene plus the arrays it points to (kept alive together)."""

    def __init__(self, sc: scn.Scene):
        nm, no = len(sc.materials), len(sc.objects)
        self.materials = (capi.PtMaterial * max(1, nm))()
        ids = {}
        for i, m in enumerate(sc.materials):
            pm = self.materials[i]
            pm.type = _MAT.get(m.type, capi.PT_MAT_LAMBERT)  # default branch, materials.go:51-53
            pm.albedo[:] = m.albedo.as_list()
            pm.rough = m.rough
            pm.ior = m.ior
            pm.emit[:] = m.emit.as_list()
            pm.power = m.power
            pm.absorption[:] = m.absorption.as_list()
            pm.smoothness = m.smoothness
            ids[m.id] = i  # later duplicates replace earlier ones, objects.go:227-229
        self.objects = (capi.PtObject * max(1, no))()
        for i, o in enumerate(sc.objects):
            po = self.objects[i]
            po.type = _OBJ.get(o.type, capi.PT_OBJ_UNKNOWN)
            po.material = ids.get(o.material_id, -1)
            po.position[:] = o.position.as_list()
            po.size[:] = o.size.as_list()
        s = capi.PtScene()
        cam = sc.camera
        s.camera.position[:] = cam.position.as_list()
        s.camera.target[:] = cam.target.as_list()
        s.camera.up[:] = cam.up.as_list()
        s.camera.fov = cam.fov
        s.camera.aperture = cam.aperture
        s.camera.focus_dist = cam.focus_dist
        s.camera.aspect_ratio = cam.aspect_ratio
        s.sky.background[:] = sc.background.as_list()
        if sc.sky is not None:
            s.sky.kind = (capi.PT_SKY_GRADIENT if sc.sky.type == "gradient"
                          else capi.PT_SKY_SOLID if sc.sky.type == "solid" else capi.PT_SKY_BACKGROUND)
            s.sky.color[:] = sc.sky.color.as_list()
            s.sky.horizon[:] = sc.sky.horizon.as_list()
            s.sky.zenith[:] = sc.sky.zenith.as_list()
        else:
            s.sky.kind = capi.PT_SKY_BACKGROUND
        s.num_materials = nm
        s.num_objects = no
        s.materials = C.cast(self.materials, C.POINTER(capi.PtMaterial))
        s.objects = C.cast(self.objects, C.POINTER(capi.PtObject))
        self.c = s
        # a copy of the scene's fog block, for scene_motion alone (rendering fog still takes the Scene: see `render`)
        self.fog_block = copy.deepcopy(getattr(sc, "fog", None))


def pt_fog(fog: scn.Fog) -> capi.PtFog:
    """scene.Fog flattened into the C ABI's pt_fog: the raw fields, resolved inside libptcore (gpu.go:2024-2096)."""
    f = capi.PtFog()
    f.density = fog.density
    f.color[:] = fog.color.as_list()
    f.scatter = fog.scatter
    f.sigma_s = fog.sigma_s
    f.sigma_a = fog.sigma_a
    f.g = fog.g
    f.hetero_strength = fog.hetero_strength
    f.noise_scale = fog.noise_scale
    f.noise_octaves = int(fog.noise_octaves)
    f.affect_sky = 1 if fog.affect_sky else 0
    f.gpu_volumetric = 1 if fog.gpu_volumetric else 0
    return f


def set_fog(ctx: capi.Context, fog: Optional[scn.Fog]) -> None:
    """pt_set_fog: `fog` for the later renders on ctx, None = off."""
    L = capi.load()
    if fog is None:
        capi.check(L.pt_set_fog(ctx.handle, None))
    else:
        f = pt_fog(fog)
        capi.check(L.pt_set_fog(ctx.handle, C.byref(f)))


def fog_last_stats(ctx: Optional[capi.Context] = None) -> dict:
    """pt_fog_last_stats of ctx: fog_ms, fog_launches, shadow_rays, draws, steps of its last frame."""
    st = capi.PtFogStats()
    capi.check(capi.load().pt_fog_last_stats((ctx or context()).handle, C.byref(st)))
    return st.as_dict()


SHADING_MODELS = {"cpu": capi.PT_SHADING_CPU, "gl": capi.PT_SHADING_GL}


def gl_materials(sc) -> "C.Array":
    """The pt_gl_material table of a scene: per material its raw reflectivity, tint and absorption_scale (scene.go:41-63), in
    material order; resolved inside libptcore (gpu.go:1840-1898)."""
    mats = sc.materials
    arr = (capi.PtGlMaterial * max(1, len(mats)))()
    for i, m in enumerate(mats):
        arr[i].reflectivity = m.reflectivity
        arr[i].tint[:] = m.tint.as_list()
        arr[i].absorption_scale = m.absorption_scale
    return arr


def set_shading(ctx: capi.Context, shading: str = "cpu", sc=None) -> None:
    """pt_set_shading: "cpu" (the CPU engine, the default) or "gl" (the OpenGL backend's estimator, which needs the Scene `sc`
    for its per-material fields) for the later renders on ctx."""
    L = capi.load()
    if shading not in SHADING_MODELS:
        raise ValueError("shading must be one of %s" % sorted(SHADING_MODELS))
    if not capi.has("pt_set_shading"):
        raise RuntimeError("this libptcore.so has no pt_set_shading (rebuild it)")
    if shading == "cpu":
        capi.check(L.pt_set_shading(ctx.handle, None))
        return
    if sc is None or isinstance(sc, FlatScene):
        raise ValueError("GL shading needs the Scene (its materials' reflectivity, tint and absorption_scale)")
    arr = gl_materials(sc)
    s = capi.PtShading(capi.PT_SHADING_GL, len(sc.materials), C.cast(arr, C.POINTER(capi.PtGlMaterial)))
    capi.check(L.pt_set_shading(ctx.handle, C.byref(s)))


def shading_last_stats(ctx: Optional[capi.Context] = None) -> dict:
    """pt_shading_last_stats of ctx: gl_ms, gl_launches, paths, segments, shadow_rays, probe_rays, draws of its last frame."""
    st = capi.PtShadingStats()
    capi.check(capi.load().pt_shading_last_stats((ctx or context()).handle, C.byref(st)))
    return st.as_dict()


def set_moments(ctx: capi.Context, on: bool) -> None:
    """pt_set_moments: later frames on ctx collect the per-pixel second moments (off by default)."""
    if not capi.has("pt_set_moments"):
        if on:
            raise RuntimeError("this libptcore.so has no pt_set_moments (rebuild it)")
        return
    capi.check(capi.load().pt_set_moments(ctx.handle, 1 if on else 0))


def read_moments(ctx: capi.Context, m2: np.ndarray) -> None:
    """pt_read_moments into m2 (contiguous float64 [H, W, 3]): per pixel and channel the sum over the samples done of L*L."""
    if m2.dtype != np.float64 or m2.ndim != 3 or m2.shape[2] != 3 or not m2.flags.c_contiguous:
        raise ValueError("moments must be contiguous float64 [H, W, 3]")
    capi.check(capi.load().pt_read_moments(ctx.handle, m2.ctypes.data_as(C.POINTER(C.c_double))))


def noise_estimate(ctx: Optional[capi.Context] = None) -> dict:
    """pt_noise_estimate of ctx's open or last frame: noise, max_pixel, pixels, bad_pixels, spp."""
    n = capi.PtNoise()
    capi.check(capi.load().pt_noise_estimate((ctx or context()).handle, C.byref(n)))
    return n.as_dict()


def noise_estimate_host(accum: np.ndarray, m2: np.ndarray, n: int) -> dict:
    """The metric of pt_noise_estimate (include/ptcore.h) in NumPy, from the sums a frame returns: accum = per pixel the sum
    of the sample radiances, m2 = the sum of their squares, n = samples done.
        m_c = S_c / n;  v_c = max(0, Q_c / n - m_c^2) / (n - 1);  e2 = mean_c(v_c) / max(mean_c(m_c), 0.01)^2
        noise = sqrt(sum(e2) / pixels); a pixel with a NaN or infinite e2 contributes 0 and counts as bad; n < 2: +inf."""
    S = np.asarray(accum, np.float64).reshape(-1, 3)
    Q = np.asarray(m2, np.float64).reshape(-1, 3)
    pixels = S.shape[0]
    if n < 2:
        return {"noise": float("inf"), "max_pixel": float("inf"), "pixels": pixels, "bad_pixels": 0, "spp": int(n)}
    with np.errstate(all="ignore"):
        m = S / float(n)
        v = np.maximum(Q / float(n) - m * m, 0.0) / float(n - 1)
        den = np.maximum((m[:, 0] + m[:, 1] + m[:, 2]) / 3.0, 0.01)
        e2 = ((v[:, 0] + v[:, 1] + v[:, 2]) / 3.0) / (den * den)
    good = np.isfinite(e2)
    e2 = np.where(good, e2, 0.0)
    return {"noise": float(np.sqrt(e2.sum() / pixels)), "max_pixel": float(e2.max()) if pixels else 0.0, "pixels": pixels,
            "bad_pixels": int(pixels - np.count_nonzero(good)), "spp": int(n)}


def set_adaptive(ctx: capi.Context, target: Optional[float] = None, min_spp: int = 0, step: int = 16) -> None:
    """pt_set_adaptive: later frames on ctx stop every 8x8 block whose own noise is at or below `target` (checked at the end of
    every pt_step once max(min_spp, 2) samples are done); `step` is what pt_render adds per step.  target=None turns it off."""
    if not capi.has("pt_set_adaptive"):
        if target is not None:
            raise RuntimeError("this libptcore.so has no pt_set_adaptive (rebuild it)")
        return
    if target is None:
        capi.check(capi.load().pt_set_adaptive(ctx.handle, None))
        return
    a = capi.PtAdaptive(float(target), int(min_spp), int(step))
    capi.check(capi.load().pt_set_adaptive(ctx.handle, C.byref(a)))


def adaptive_state(ctx: Optional[capi.Context] = None) -> dict:
    """pt_adaptive_state of ctx's open or last frame: blocks, active_blocks, samples, spp_min, spp_max, worst_active."""
    st = capi.PtAdaptiveState()
    capi.check(capi.load().pt_adaptive_state((ctx or context()).handle, C.byref(st)))
    return st.as_dict()


def read_sample_counts(ctx: capi.Context, spp: np.ndarray) -> None:
    """pt_read_sample_counts into spp (contiguous uint32 [H, W]): the samples each pixel of the adaptive frame holds."""
    if spp.dtype != np.uint32 or spp.ndim != 2 or not spp.flags.c_contiguous:
        raise ValueError("sample counts must be contiguous uint32 [H, W]")
    capi.check(capi.load().pt_read_sample_counts(ctx.handle, spp.ctypes.data_as(C.POINTER(C.c_uint32))))


def adaptive_plan_host(samples: np.ndarray, target: float, step: int, min_spp: int, cap: int) -> np.ndarray:
    """The count map an adaptive frame ends with, in NumPy, from per-sample radiances: samples = float64 [H, W, >= cap, 3].
    Samples are added `step` at a time up to `cap`; after every step with done >= max(min_spp, 2) each still-active 8x8 block
    (aligned to the frame's origin, cut at its right and bottom edges) whose noise b = sqrt(sum of e2 / k) over its k pixels is at
    or below `target` stops (e2 = the per-pixel quantity of noise_estimate_host with n = done; a NaN or infinite e2 adds 0).
    Returns int32 [ceil(H / 8), ceil(W / 8)]: the samples each block holds at the end."""
    l = np.asarray(samples, np.float64)
    H, W = l.shape[0], l.shape[1]
    if l.ndim != 4 or l.shape[3] != 3 or l.shape[2] < cap:
        raise ValueError("samples must be [H, W, >= cap, 3]")
    step = max(1, int(step))
    nby, nbx = (H + 7) // 8, (W + 7) // 8
    counts = np.zeros((nby, nbx), np.int32)
    active = np.ones((nby, nbx), bool)
    S = np.zeros((H, W, 3))
    Q = np.zeros((H, W, 3))
    done = 0
    while done < cap and active.any():
        n = min(step, cap - done)
        for s in range(done, done + n):  # in sample order, like the device sums
            S = S + l[:, :, s]
            Q = Q + l[:, :, s] * l[:, :, s]
        done += n
        counts[active] = done
        if done < max(int(min_spp), 2):
            continue
        with np.errstate(all="ignore"):
            m = S / float(done)
            v = np.maximum(Q / float(done) - m * m, 0.0) / float(done - 1)
            den = np.maximum((m[..., 0] + m[..., 1] + m[..., 2]) / 3.0, 0.01)
            e2 = ((v[..., 0] + v[..., 1] + v[..., 2]) / 3.0) / (den * den)
        e2 = np.where(np.isfinite(e2), e2, 0.0)
        for by in range(nby):
            for bx in range(nbx):
                if active[by, bx]:
                    blk = e2[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8]
                    if np.sqrt(blk.sum() / blk.size) <= target:
                        active[by, bx] = False
    return counts


def set_features(ctx: capi.Context, k: int) -> None:
    """pt_set_features: later frames on ctx collect the first-hit normal, albedo and distance of every pixel's first k samples
    (DESIGN 3.11); 0 = off, the default."""
    if not capi.has("pt_set_features"):
        if k:
            raise RuntimeError("this libptcore.so has no pt_set_features (rebuild it)")
        return
    capi.check(capi.load().pt_set_features(ctx.handle, int(k)))


def read_features(ctx: capi.Context, normal: Optional[np.ndarray] = None, albedo: Optional[np.ndarray] = None,
                  depth: Optional[np.ndarray] = None) -> None:
    """pt_read_features into the arrays given (contiguous float64 [H, W, 3] each): the raw sums over the feature samples of the
    face-forward normal, of the albedo and of (distance, samples that hit, feature samples taken)."""
    for a in (normal, albedo, depth):
        if a is not None and (a.dtype != np.float64 or a.ndim != 3 or a.shape[2] != 3 or not a.flags.c_contiguous):
            raise ValueError("feature planes must be contiguous float64 [H, W, 3]")
    p = [a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None for a in (normal, albedo, depth)]
    capi.check(capi.load().pt_read_features(ctx.handle, *p))


def set_feature_walk(ctx: capi.Context, on: bool) -> None:
    """pt_set_feature_walk: later frames on ctx with features on are accepted on the bounding-volume-hierarchy path too, the first
    hit found by one walk of the tree per 8x8 block and feature sample.  A library without the entry point takes
    False only."""
    if not capi.has("pt_set_feature_walk"):
        if on:
            raise RuntimeError("this libptcore.so has no pt_set_feature_walk (rebuild it)")
        return
    capi.check(capi.load().pt_set_feature_walk(ctx.handle, 1 if on else 0))
    ctx._feature_walk_on = bool(on)  # what `render` compares with: it says the setting only when it changes


def feature_walk_stats(ctx: capi.Context) -> dict:
    """pt_feature_walk_stats of the last frame: (wave, feature sample) pairs walked by the wave and sent to the plain scan, the
    walks' node visits, the deepest wave stack."""
    if not capi.has("pt_feature_walk_stats"):
        raise RuntimeError("this libptcore.so has no pt_feature_walk_stats (rebuild it)")
    out = (C.c_uint64 * 4)()
    capi.check(capi.load().pt_feature_walk_stats(ctx.handle, out))
    return {"walked": int(out[0]), "plain": int(out[1]), "node_visits": int(out[2]), "deepest_stack": int(out[3])}


def feature_walk_from_env(environ=None) -> bool:
    """PATHTRACER_GPU_FEATURE_WALK=1 (or true / on / yes): features on the bounding-volume-hierarchy path (pt_set_feature_walk)."""
    return _env_on(environ, "PATHTRACER_GPU_FEATURE_WALK")


def set_fog_walk(ctx: capi.Context, on: bool) -> None:
    """pt_set_fog_walk: later frames on ctx with a gpu_volumetric fog block are accepted on the bounding-volume-hierarchy path too,
    the closest hit and every shadow ray of the term answered by one walk of the tree per 8x8 block.  A library without
    the entry point takes False only."""
    if not capi.has("pt_set_fog_walk"):
        if on:
            raise RuntimeError("this libptcore.so has no pt_set_fog_walk (rebuild it)")
        return
    capi.check(capi.load().pt_set_fog_walk(ctx.handle, 1 if on else 0))
    ctx._fog_walk_on = bool(on)  # what `render` compares with: it says the setting only when it changes


def fog_walk_stats(ctx: capi.Context) -> dict:
    """pt_fog_walk_stats of the last frame: (wave, sample) pairs whose primary rays the wave walked and those sent to the plain scan,
    shadow turns (one march step x one light of a wave) walked and sent to the plain loop, the shadow walks' node visits, the
    deepest wave stack."""
    if not capi.has("pt_fog_walk_stats"):
        raise RuntimeError("this libptcore.so has no pt_fog_walk_stats (rebuild it)")
    out = (C.c_uint64 * 6)()
    capi.check(capi.load().pt_fog_walk_stats(ctx.handle, out))
    return {"primary_walked": int(out[0]), "primary_plain": int(out[1]), "shadow_walked": int(out[2]), "shadow_plain": int(out[3]),
            "node_visits": int(out[4]), "deepest_stack": int(out[5])}


def fog_walk_from_env(environ=None) -> bool:
    """PATHTRACER_GPU_FOG_WALK=1 (or true / on / yes): volumetric fog on the bounding-volume-hierarchy path (pt_set_fog_walk)."""
    return _env_on(environ, "PATHTRACER_GPU_FOG_WALK")


def set_shading_walk(ctx: capi.Context, on: bool) -> None:
    """pt_set_shading_walk: later GL frames on ctx (shading="gl") are accepted on the bounding-volume-hierarchy path too, every
    closest hit, shadow ray and metal probe answered by the lane's own walk of the tree.  A library without the entry
    point takes False only."""
    if not capi.has("pt_set_shading_walk"):
        if on:
            raise RuntimeError("shading walk: libptcore.so lacks pt_set_shading_walk")
        return
    capi.check(capi.load().pt_set_shading_walk(ctx.handle, 1 if on else 0))
    ctx._shading_walk_on = bool(on)  # what `render` compares with: it says the setting only when it changes


SHADING_WALK_STATS = ("closest_walked", "closest_plain", "shadow_walked", "shadow_plain", "closest_visits", "shadow_visits",
                      "deepest_stack")


def shading_walk_stats(ctx: capi.Context) -> dict:
    """pt_shading_walk_stats of the last frame: closest-hit queries answered by a walk and those sent to the plain loop, shadow
    queries walked and sent to the plain loop, the node visits of either kind of walk, the deepest stack."""
    if not capi.has("pt_shading_walk_stats"):
        raise RuntimeError("shading walk: libptcore.so lacks pt_shading_walk_stats")
    out = (C.c_uint64 * 7)()
    capi.check(capi.load().pt_shading_walk_stats(ctx.handle, out))
    return dict(zip(SHADING_WALK_STATS, (int(v) for v in out)))


def shading_walk_from_env(environ=None) -> bool:
    """PATHTRACER_GPU_SHADING_WALK=1 (or true / on / yes): GL shading on the bounding-volume-hierarchy path (pt_set_shading_walk)."""
    return _env_on(environ, "PATHTRACER_GPU_SHADING_WALK")


def set_shading_features(ctx: capi.Context, on: bool) -> None:
    """pt_set_shading_features: later GL frames on ctx (shading="gl") accept features, object ids and the a-trous filter
    (pt_atrous, pt_atrous_halves), the features being those of the GL pass's own camera rays.  A library without
    the entry point takes False only."""
    if not capi.has("pt_set_shading_features"):
        if on:
            raise RuntimeError("shading features: libptcore.so lacks pt_set_shading_features")
        return
    capi.check(capi.load().pt_set_shading_features(ctx.handle, 1 if on else 0))
    ctx._shading_features_on = bool(on)  # what `render` compares with: it says the setting only when it changes


def shading_features_from_env(environ=None) -> bool:
    """PATHTRACER_GPU_SHADING_FEATURES=1 (or true / on / yes): features and the a-trous filter for GL-shaded frames
    (pt_set_shading_features)."""
    return _env_on(environ, "PATHTRACER_GPU_SHADING_FEATURES")


def set_bvh_refit(ctx: capi.Context, max_growth: float) -> None:
    """pt_set_bvh_refit: with max_growth >= 1 (or inf) a later frame on ctx whose scene differs from the previous
    frame's only in where its objects are and how large (planes included; types, materials and the count stay) keeps the
    bounding-volume hierarchy's topology and recomputes its boxes on the devices;
    a refitted tree whose quality figure exceeds max_growth x the built one's is rebuilt before the next frame.  0 turns it off.  A
    library without the entry point takes 0 only."""
    if not capi.has("pt_set_bvh_refit"):
        if max_growth:
            raise RuntimeError("this libptcore.so has no pt_set_bvh_refit (rebuild it)")
        return
    capi.check(capi.load().pt_set_bvh_refit(ctx.handle, float(max_growth)))
    ctx._bvh_refit = float(max_growth)  # what `render` compares with: it says the setting only when it changes


def bvh_refit_stats(ctx: capi.Context) -> dict:
    """pt_bvh_refit_stats: builds and refits since the context was made, what the last frame's scene preparation did
    (last_action: 0 nothing, 1 build, 2 refit), why the last full build happened (capi.PT_BVH_REASON_*), the quality figure at the
    last full build and now, and the device milliseconds of the last refit."""
    if not capi.has("pt_bvh_refit_stats"):
        raise RuntimeError("this libptcore.so has no pt_bvh_refit_stats (rebuild it)")
    st = capi.PtBvhRefitStats()
    capi.check(capi.load().pt_bvh_refit_stats(ctx.handle, C.byref(st)))
    return st.as_dict()


def bvh_refit_check(before, after) -> dict:
    """pt_debug_bvh_refit_check (no GPU needed): the hierarchy of scene `before` refitted to `after` on the host, checked."""
    a = before if isinstance(before, FlatScene) else FlatScene(before)
    b = after if isinstance(after, FlatScene) else FlatScene(after)
    out = (C.c_int32 * 8)()
    capi.check(capi.load().pt_debug_bvh_refit_check(C.byref(a.c), C.byref(b.c), out))
    keys = ("nodes", "objects", "reason", "objects_outside", "children_outside", "bytes_differ", "cost_ratio_x1000", "topology_changed")
    return dict(zip(keys, (int(v) for v in out)))


def bvh_refit_from_env(environ=None) -> float:
    """PATHTRACER_GPU_BVH_REFIT=<G>: the growth bound of pt_set_bvh_refit (a number >= 1 or "inf"); unset, empty or 0: off."""
    v = (os.environ if environ is None else environ).get("PATHTRACER_GPU_BVH_REFIT", "").strip()
    if not v:
        return 0.0
    g = float(v)
    if not (g == 0.0 or g >= 1.0):
        raise ValueError("PATHTRACER_GPU_BVH_REFIT must be 0, at least 1 or inf")
    return g


BVH_BUILD_MODES = {"host": 0, "device": 1}


def _bvh_build_mode(mode) -> int:
    """0 / 1, "host" / "device", False / True as the mode of pt_set_bvh_build."""
    if isinstance(mode, str):
        if mode.strip().lower() not in BVH_BUILD_MODES:
            raise ValueError("bvh_build must be 'host' or 'device', not %r" % (mode,))
        return BVH_BUILD_MODES[mode.strip().lower()]
    if int(mode) not in (0, 1):
        raise ValueError("bvh_build must be 0 (host) or 1 (device), not %r" % (mode,))
    return int(mode)


def set_bvh_build(ctx: capi.Context, mode) -> None:
    """pt_set_bvh_build: with "device" (1) a later full build of the bounding-volume hierarchy on ctx -- an object added
    or removed, a material or a type changed, the first frame, a refitted tree that outgrew its bound -- runs on devices[0] in Morton
    order instead of on the host; "host" (0) is the default.  The frame is the same, bit for bit.  A library without the entry point
    takes "host" only."""
    m = _bvh_build_mode(mode)
    if not capi.has("pt_set_bvh_build"):
        if m:
            raise RuntimeError("this libptcore.so has no pt_set_bvh_build (rebuild it)")
        return
    capi.check(capi.load().pt_set_bvh_build(ctx.handle, m))
    ctx._bvh_build = m  # what `render` compares with: it says the setting only when it changes


def bvh_build_stats(ctx: capi.Context) -> dict:
    """pt_bvh_build_stats: host and device builds since the context was made, the builder of the tree in use (capi.PT_BVH_BUILDER_*),
    why the last build fell back to the host (capi.PT_BVH_BUILD_FALLBACK_*), the tree's nodes, depth, stack need and quality figure,
    the device milliseconds of the last device build, the host's wall milliseconds of its upload and of its readback, and the wall
    milliseconds of the last full scene preparation."""
    if not capi.has("pt_bvh_build_stats"):
        raise RuntimeError("this libptcore.so has no pt_bvh_build_stats (rebuild it)")
    st = capi.PtBvhBuildStats()
    capi.check(capi.load().pt_bvh_build_stats(ctx.handle, C.byref(st)))
    return st.as_dict()


def bvh_build_check(sc) -> dict:
    """pt_debug_bvh_build_check (no GPU needed): the Morton-order hierarchy of scene `sc` by the host restatement, checked."""
    a = sc if isinstance(sc, FlatScene) else FlatScene(sc)
    out = (C.c_int32 * 8)()
    capi.check(capi.load().pt_debug_bvh_build_check(C.byref(a.c), out))
    keys = ("nodes", "objects", "depth", "stack_need", "not_reached_once", "objects_outside", "children_outside", "faults")
    return dict(zip(keys, (int(v) for v in out)))


def bvh_build_from_env(environ=None) -> int:
    """PATHTRACER_GPU_BVH_BUILD=host|device: the mode of pt_set_bvh_build; unset or empty: host."""
    v = (os.environ if environ is None else environ).get("PATHTRACER_GPU_BVH_BUILD", "").strip().lower()
    if not v:
        return 0
    if v not in BVH_BUILD_MODES:
        raise ValueError("PATHTRACER_GPU_BVH_BUILD must be host or device")
    return BVH_BUILD_MODES[v]


def set_object_ids(ctx: capi.Context, on: bool) -> None:
    """pt_set_object_ids: later frames on ctx with features on also record, per pixel, the index into the scene's object list of
    the first hit of the pixel's sample 0 (-1: a miss).  A library without the entry point takes False only."""
    if not capi.has("pt_set_object_ids"):
        if on:
            raise RuntimeError("this libptcore.so has no pt_set_object_ids (rebuild it)")
        return
    capi.check(capi.load().pt_set_object_ids(ctx.handle, 1 if on else 0))
    ctx._object_ids_on = bool(on)  # what `render` compares with: it says the setting only when it changes


def read_object_ids(ctx: capi.Context, ids: np.ndarray) -> None:
    """pt_read_object_ids into ids (contiguous int32 [H, W]): scene indices, -1 where sample 0 missed."""
    if not capi.has("pt_read_object_ids"):
        raise RuntimeError("this libptcore.so has no pt_read_object_ids (rebuild it)")
    if ids.dtype != np.int32 or ids.ndim != 2 or not ids.flags.c_contiguous:
        raise ValueError("ids must be contiguous int32 [H, W]")
    capi.check(capi.load().pt_read_object_ids(ctx.handle, ids.ctypes.data_as(C.POINTER(C.c_int32))))


@dataclass
class AtrousConfig:
    """The a-trous filter of pt_atrous: iterations 0..6 and the four sigmas (a feature sigma of 0 turns its term
    off); `features` = feature samples per pixel that `render` asks for (None: 4 where the scene allows them, else 0)."""
    iterations: int = 5
    sigma_l: float = 4.0
    sigma_n: float = 0.1
    sigma_z: float = 0.1
    sigma_a: float = 0.2
    features: Optional[int] = None

    @classmethod
    def from_env(cls, environ=None) -> Optional["AtrousConfig"]:
        """PATHTRACER_GPU_ATROUS=1 (or true / on / yes) turns the filter on (None otherwise); PATHTRACER_GPU_ATROUS_ITERS=<0..6>
        and PATHTRACER_GPU_FEATURES=<int >= 0> set the iterations and the feature samples, anything else keeps the default."""
        if not _env_on(environ, "PATHTRACER_GPU_ATROUS"):
            return None
        i = _env_int(environ, "PATHTRACER_GPU_ATROUS_ITERS", 0, 6)
        return cls(iterations=5 if i is None else i, features=features_from_env(environ))

    def c(self) -> capi.PtAtrousConfig:
        return capi.PtAtrousConfig(int(self.iterations), 0, float(self.sigma_l), float(self.sigma_n), float(self.sigma_z),
                                   float(self.sigma_a))


def features_from_env(environ=None) -> Optional[int]:
    """PATHTRACER_GPU_FEATURES=<int >= 0>: the feature samples per pixel, None when unset or not such a number."""
    return _env_int(environ, "PATHTRACER_GPU_FEATURES", 0)


def atrous(ctx: capi.Context, cfg: Optional[AtrousConfig], img: Optional[np.ndarray], mean: Optional[np.ndarray] = None,
           var: Optional[np.ndarray] = None) -> dict:
    """pt_atrous on ctx's open or last frame (cfg None = the defaults): img (uint8 [H, W, 4] or None) receives the finished
    filtered image, mean (float64 [H, W, 3]) and var (float64 [H, W]) the filtered mean and its variance.  Returns the
    pt_atrous_stats: atrous_ms, launches, iterations, noise_before, noise_after, bad_pixels."""
    if not capi.has("pt_atrous"):
        raise RuntimeError("this libptcore.so has no pt_atrous (rebuild it)")
    stride = 0
    if img is not None:
        if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 4 or img.strides[2] != 1 or img.strides[1] != 4:
            raise ValueError("img must be uint8 [H, W, 4] with contiguous RGBA rows")
        stride = int(img.strides[0])
    if mean is not None and (mean.dtype != np.float64 or mean.ndim != 3 or mean.shape[2] != 3 or not mean.flags.c_contiguous):
        raise ValueError("mean must be contiguous float64 [H, W, 3]")
    if var is not None and (var.dtype != np.float64 or var.ndim != 2 or not var.flags.c_contiguous):
        raise ValueError("var must be contiguous float64 [H, W]")
    for a in (mean, var):
        if a is not None and img is not None and a.shape[:2] != img.shape[:2]:
            raise ValueError("mean / var must have the image's height and width")
    c = cfg.c() if cfg is not None else None
    st = capi.PtAtrousStats()
    dp = C.POINTER(C.c_double)
    capi.check(capi.load().pt_atrous(ctx.handle, C.byref(c) if c is not None else None, _ptr(img), stride,
                                     mean.ctypes.data_as(dp) if mean is not None else None,
                                     var.ctypes.data_as(dp) if var is not None else None, C.byref(st)))
    return st.as_dict()


_atrous = atrous  # (`render` has an argument of that name)


@dataclass
class TemporalConfig:
    """The temporal accumulation of pt_temporal: alpha = the least weight of the current frame, max_len = where the
    history length saturates, and the three tests a history tap has to pass (relative first-hit distance, normal, albedo)."""
    alpha: float = 0.2
    max_len: int = 32
    tol_z: float = 0.1
    n_min: float = 0.9
    tol_a: float = 0.05

    @classmethod
    def from_env(cls, environ=None) -> Optional["TemporalConfig"]:
        """PATHTRACER_GPU_TEMPORAL=1 (or true / on / yes) turns the accumulation on (None otherwise)."""
        return cls() if _env_on(environ, "PATHTRACER_GPU_TEMPORAL") else None

    def c(self) -> capi.PtTemporalConfig:
        return capi.PtTemporalConfig(float(self.alpha), float(self.tol_z), float(self.n_min), float(self.tol_a), int(self.max_len), 0)


def temporal(ctx: capi.Context, cfg: Optional[TemporalConfig], filter: Optional[AtrousConfig], img: Optional[np.ndarray],
             mean: Optional[np.ndarray] = None, var: Optional[np.ndarray] = None) -> dict:
    """pt_temporal on ctx's open or last frame (cfg None = the defaults; filter None = no filter): blends the frame into the
    context's reprojected history, stores the result as the new history and filters it.  img (uint8 [H, W, 4] or None) receives the
    finished image, mean (float64 [H, W, 3]) and var (float64 [H, W]) the output and its variance.  Returns the pt_temporal_stats.
    The frame needs features on, and the caller changes the seed from frame to frame (the blended variance assumes independent
    frames)."""
    if not capi.has("pt_temporal"):
        raise RuntimeError("this libptcore.so has no pt_temporal (rebuild it)")
    stride = 0
    if img is not None:
        if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 4 or img.strides[2] != 1 or img.strides[1] != 4:
            raise ValueError("img must be uint8 [H, W, 4] with contiguous RGBA rows")
        stride = int(img.strides[0])
    if mean is not None and (mean.dtype != np.float64 or mean.ndim != 3 or mean.shape[2] != 3 or not mean.flags.c_contiguous):
        raise ValueError("mean must be contiguous float64 [H, W, 3]")
    if var is not None and (var.dtype != np.float64 or var.ndim != 2 or not var.flags.c_contiguous):
        raise ValueError("var must be contiguous float64 [H, W]")
    for a in (mean, var):
        if a is not None and img is not None and a.shape[:2] != img.shape[:2]:
            raise ValueError("mean / var must have the image's height and width")
    c = cfg.c() if cfg is not None else None
    f = filter.c() if filter is not None else None
    st = capi.PtTemporalStats()
    dp = C.POINTER(C.c_double)
    capi.check(capi.load().pt_temporal(ctx.handle, C.byref(c) if c is not None else None, C.byref(f) if f is not None else None,
                                       _ptr(img), stride, mean.ctypes.data_as(dp) if mean is not None else None,
                                       var.ctypes.data_as(dp) if var is not None else None, C.byref(st)))
    return st.as_dict()


_temporal = temporal  # (`render` has an argument of that name)


def temporal_read(ctx: capi.Context, mean: Optional[np.ndarray] = None, var: Optional[np.ndarray] = None,
                  length: Optional[np.ndarray] = None) -> None:
    """pt_temporal_read: the stored history into mean (float64 [H, W, 3]), var (float64 [H, W]) and length (int32 [H, W]: the
    frames behind each pixel, 0 = a bad pixel).  Raises PtError (PT_ERR_STATE) when the history is empty."""
    if mean is not None and (mean.dtype != np.float64 or mean.ndim != 3 or mean.shape[2] != 3 or not mean.flags.c_contiguous):
        raise ValueError("mean must be contiguous float64 [H, W, 3]")
    if var is not None and (var.dtype != np.float64 or var.ndim != 2 or not var.flags.c_contiguous):
        raise ValueError("var must be contiguous float64 [H, W]")
    if length is not None and (length.dtype != np.int32 or length.ndim != 2 or not length.flags.c_contiguous):
        raise ValueError("length must be contiguous int32 [H, W]")
    if len({a.shape[:2] for a in (mean, var, length) if a is not None}) > 1:
        raise ValueError("mean / var / length must have the same height and width")
    dp = C.POINTER(C.c_double)
    capi.check(capi.load().pt_temporal_read(ctx.handle, mean.ctypes.data_as(dp) if mean is not None else None,
                                            var.ctypes.data_as(dp) if var is not None else None,
                                            length.ctypes.data_as(C.POINTER(C.c_int32)) if length is not None else None))


def temporal_reset(ctx: capi.Context) -> None:
    """pt_temporal_reset: empties the context's history (after a scene edit or a cut)."""
    if capi.has("pt_temporal_reset"):
        capi.check(capi.load().pt_temporal_reset(ctx.handle))


def temporal_set_clip(ctx: capi.Context, gamma: float) -> None:
    """pt_temporal_set_clip: later pt_temporal calls on ctx clamp the reprojected history to the frame's mean
    +- gamma * sqrt(var_frame + var_history) before the blend.  0 = off, the default; 2.5 is the recommended value.
    Raises PtError (PT_ERR_INVALID) for a NaN, a negative or an infinite gamma."""
    if not capi.has("pt_temporal_set_clip"):
        raise RuntimeError("this libptcore.so has no pt_temporal_set_clip (rebuild it)")
    capi.check(capi.load().pt_temporal_set_clip(ctx.handle, float(gamma)))


def temporal_clip_stats(ctx: capi.Context) -> dict:
    """pt_temporal_clip_stats: dict(gamma, clipped, reprojected) of the last pt_temporal that succeeded on ctx.  Raises PtError
    (PT_ERR_STATE) while the history is empty."""
    if not capi.has("pt_temporal_clip_stats"):
        raise RuntimeError("this libptcore.so has no pt_temporal_clip_stats (rebuild it)")
    st = capi.PtTemporalClipStats()
    capi.check(capi.load().pt_temporal_clip_stats(ctx.handle, C.byref(st)))
    return st.as_dict()


def temporal_set_motion(ctx: capi.Context, delta) -> None:
    """pt_temporal_set_motion: delta = [n, 3], per scene object its position in the frame about to be accumulated minus its position
    in the frame the history was stored from (None or empty clears the table).  One-shot: the next pt_temporal that succeeds
    consumes it.  The frame must have recorded object ids (set_object_ids); DESIGN 3.13b."""
    if not capi.has("pt_temporal_set_motion"):
        raise RuntimeError("this libptcore.so has no pt_temporal_set_motion (rebuild it)")
    if delta is None:
        capi.check(capi.load().pt_temporal_set_motion(ctx.handle, None, 0))
        return
    d = np.ascontiguousarray(delta, np.float64)
    if d.size and (d.ndim != 2 or d.shape[1] != 3):
        raise ValueError("delta must be [num_objects, 3]")
    n = d.shape[0] if d.size else 0
    capi.check(capi.load().pt_temporal_set_motion(ctx.handle, d.ctypes.data_as(C.POINTER(C.c_double)) if n else None, n))


def temporal_motion_stats(ctx: capi.Context) -> dict:
    """pt_temporal_motion_stats: dict(objects, moved, moved_reprojected) of the last pt_temporal that succeeded on ctx.  Raises
    PtError (PT_ERR_STATE) while the history is empty."""
    if not capi.has("pt_temporal_motion_stats"):
        raise RuntimeError("this libptcore.so has no pt_temporal_motion_stats (rebuild it)")
    st = capi.PtTemporalMotionStats()
    capi.check(capi.load().pt_temporal_motion_stats(ctx.handle, C.byref(st)))
    return st.as_dict()


def scene_motion(prev, cur) -> Optional[np.ndarray]:
    """What moved between two scenes, for temporal_set_motion: the [n, 3] array of cur's object positions minus prev's when the two
    differ in object positions and the camera only; None when anything else differs -- the number, order, type, size or material
    id of the objects, the material table, the sky, the background or the fog -- and the history has to be reset.  A pure
    function of the two scenes (Scene or FlatScene each; a FlatScene keeps a copy of the fog block of the Scene it was made from)."""
    a = prev if isinstance(prev, FlatScene) else FlatScene(prev)
    b = cur if isinstance(cur, FlatScene) else FlatScene(cur)
    ca, cb = a.c, b.c
    if ca.num_objects != cb.num_objects or ca.num_materials != cb.num_materials:
        return None
    if C.string_at(C.addressof(ca.sky), C.sizeof(ca.sky)) != C.string_at(C.addressof(cb.sky), C.sizeof(cb.sky)):
        return None
    msz = C.sizeof(capi.PtMaterial) * ca.num_materials
    if msz and C.string_at(ca.materials, msz) != C.string_at(cb.materials, msz):
        return None
    if a.fog_block != b.fog_block:
        return None
    out = np.zeros((ca.num_objects, 3))
    for i in range(ca.num_objects):
        oa, ob = ca.objects[i], cb.objects[i]
        if oa.type != ob.type or oa.material != ob.material or tuple(oa.size) != tuple(ob.size):
            return None
        out[i] = np.array(tuple(ob.position)) - np.array(tuple(oa.position))
    return out


def temporal_clip_from_env(environ=None) -> float:
    """PATHTRACER_GPU_TEMPORAL_CLIP=<gamma>: the clip of the RenderInto path when PATHTRACER_GPU_TEMPORAL is on.  Unset, empty or
    not a finite number >= 0: 0.0 (off)."""
    env = os.environ if environ is None else environ
    try:
        g = float(env.get("PATHTRACER_GPU_TEMPORAL_CLIP", "") or 0.0)
    except ValueError:
        return 0.0
    return g if math.isfinite(g) and g >= 0.0 else 0.0


def temporal_motion_from_env(environ=None) -> bool:
    """PATHTRACER_GPU_TEMPORAL_MOTION=1 (or true / on / yes): the RenderInto path passes the objects' displacements to the
    accumulation.  Read only when PATHTRACER_GPU_TEMPORAL turned the accumulation on."""
    return _env_on(environ, "PATHTRACER_GPU_TEMPORAL_MOTION")


def set_halves(ctx: capi.Context, on: bool) -> None:
    """pt_set_halves: later frames on ctx also collect the half-buffer sums SA, QA (even-indexed samples) and SB, QB (odd-indexed
    ones) of every pixel; off by default.  Such frames collect second moments too."""
    if not capi.has("pt_set_halves"):
        if on:
            raise RuntimeError("this libptcore.so has no pt_set_halves (rebuild it)")
        return
    capi.check(capi.load().pt_set_halves(ctx.handle, 1 if on else 0))


def read_halves(ctx: capi.Context, sa: Optional[np.ndarray] = None, qa: Optional[np.ndarray] = None, sb: Optional[np.ndarray] = None,
                qb: Optional[np.ndarray] = None) -> None:
    """pt_read_halves into the arrays given (contiguous float64 [H, W, 3] each): the raw sums of the sample radiances and of
    their squares over the even-indexed samples (sa, qa) and over the odd-indexed ones (sb, qb)."""
    for a in (sa, qa, sb, qb):
        if a is not None and (a.dtype != np.float64 or a.ndim != 3 or a.shape[2] != 3 or not a.flags.c_contiguous):
            raise ValueError("half-buffer sums must be contiguous float64 [H, W, 3]")
    p = [a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None for a in (sa, qa, sb, qb)]
    capi.check(capi.load().pt_read_halves(ctx.handle, *p))


def atrous_halves(ctx: capi.Context, cfg: Optional[AtrousConfig], mean: Optional[np.ndarray] = None, err: Optional[np.ndarray] = None,
                  half_means: Optional[np.ndarray] = None) -> dict:
    """pt_atrous_halves on ctx's open or last frame (cfg None = the defaults): the a-trous filter on each half of the samples;
    mean (float64 [H, W, 3]) receives (fA + fB) / 2, err (float64 [H, W]) the per-pixel ((fA - fB) / 2)^2 averaged over the channels,
    half_means (float64 [2, H, W, 3]) fA and fB.  Returns the pt_halves_stats: atrous_ms, launches, iterations, noise (measured),
    noise_model (propagated), bad_pixels, spp_min.  Neither figure sees the bias the filter adds."""
    if not capi.has("pt_atrous_halves"):
        raise RuntimeError("this libptcore.so has no pt_atrous_halves (rebuild it)")
    if mean is not None and (mean.dtype != np.float64 or mean.ndim != 3 or mean.shape[2] != 3 or not mean.flags.c_contiguous):
        raise ValueError("mean must be contiguous float64 [H, W, 3]")
    if err is not None and (err.dtype != np.float64 or err.ndim != 2 or not err.flags.c_contiguous):
        raise ValueError("err must be contiguous float64 [H, W]")
    if half_means is not None and (half_means.dtype != np.float64 or half_means.ndim != 4 or half_means.shape[0] != 2
                                   or half_means.shape[3] != 3 or not half_means.flags.c_contiguous):
        raise ValueError("half_means must be contiguous float64 [2, H, W, 3]")
    shapes = {a.shape[:2] for a in (mean, err) if a is not None} | ({half_means.shape[1:3]} if half_means is not None else set())
    if len(shapes) > 1:
        raise ValueError("mean / err / half_means must have the same height and width")
    c = cfg.c() if cfg is not None else None
    st = capi.PtHalvesStats()
    dp = C.POINTER(C.c_double)
    capi.check(capi.load().pt_atrous_halves(ctx.handle, C.byref(c) if c is not None else None,
                                            *(a.ctypes.data_as(dp) if a is not None else None for a in (mean, err, half_means)),
                                            C.byref(st)))
    return st.as_dict()


def filtered_noise_from_env(environ=None) -> Optional[float]:
    """PATHTRACER_GPU_FILTERED_NOISE=<float > 0>: the noise target on the filtered frame (used with PATHTRACER_GPU_ATROUS; the step
    is PATHTRACER_GPU_NOISE_STEP); None when unset or not such a number."""
    return _env_positive(environ, "PATHTRACER_GPU_FILTERED_NOISE")


def set_adaptive_filtered(ctx: capi.Context, cfg: Optional[AtrousConfig] = None, pool: int = 1, on: bool = True) -> None:
    """pt_set_adaptive_filtered: later adaptive frames on ctx (set_adaptive gives the target, min_spp and step) stop their 8x8 blocks
    by the noise left in the filtered frame, pooled over the blocks within `pool` blocks (0..4) of each; cfg None = the
    filter's defaults.  on=False turns the rule off."""
    if not capi.has("pt_set_adaptive_filtered"):
        if on:
            raise RuntimeError("this libptcore.so has no pt_set_adaptive_filtered (rebuild it)")
        return
    if not on:
        capi.check(capi.load().pt_set_adaptive_filtered(ctx.handle, None))
        return
    f = capi.PtAdaptiveFiltered((cfg or AtrousConfig()).c(), int(pool), 0)
    capi.check(capi.load().pt_set_adaptive_filtered(ctx.handle, C.byref(f)))


def read_block_figures(ctx: capi.Context, pooled: Optional[np.ndarray] = None, own: Optional[np.ndarray] = None) -> int:
    """pt_read_block_figures of ctx's open or last frame into the arrays given (contiguous float64 [ceil(H / 8), ceil(W / 8)] each):
    the last deciding check's pooled figure P_B and the block's own sqrt(s_B / k_B).  Returns the number of checks that have decided."""
    if not capi.has("pt_read_block_figures"):
        raise RuntimeError("this libptcore.so has no pt_read_block_figures (rebuild it)")
    for a in (pooled, own):
        if a is not None and (a.dtype != np.float64 or a.ndim != 2 or not a.flags.c_contiguous):
            raise ValueError("block figures must be contiguous float64 [blocks down, blocks across]")
    n = C.c_int32(0)
    dp = C.POINTER(C.c_double)
    capi.check(capi.load().pt_read_block_figures(ctx.handle, *(a.ctypes.data_as(dp) if a is not None else None for a in (pooled, own)),
                                                 C.byref(n)))
    return n.value


def filtered_adaptive_from_env(environ=None):
    """PATHTRACER_GPU_FILTERED_ADAPTIVE=<float > 0>: the block target on the filtered frame's pooled noise (used with
    PATHTRACER_GPU_ATROUS; the step is PATHTRACER_GPU_NOISE_STEP) and PATHTRACER_GPU_POOL=<0..4>, the pool radius in blocks (1 when
    unset or not such a number).  Returns (target or None, pool)."""
    pool = _env_int(environ, "PATHTRACER_GPU_POOL", 0, 4)
    return _env_positive(environ, "PATHTRACER_GPU_FILTERED_ADAPTIVE"), 1 if pool is None else pool


def scene_allows_features(sc, shading: str = "cpu", feature_walk: bool = False, shading_features: bool = False,
                          shading_walk: bool = False) -> bool:
    """Does a frame of this scene accept pt_set_features(k > 0)?  Not with GL shading unless the context collects GL's own
    features (shading_features: pt_set_shading_features), and not on the bounding-volume-hierarchy path (more than 128 spheres or
    128 boxes, or PTCORE_SCAN=bvh) unless the context walks the tree for them (feature_walk: pt_set_feature_walk; with GL shading
    shading_walk: pt_set_shading_walk, which such a GL frame needs anyway)."""
    if shading != "cpu":
        if not shading_features:
            return False
        feature_walk = shading_walk  # (pt_set_feature_walk is not consulted in GL mode)
    if feature_walk:
        return True
    if os.environ.get("PTCORE_SCAN", "") in ("bvh", "verify_bvh"):
        return False
    if isinstance(sc, FlatScene):
        types = [sc.objects[i].type for i in range(sc.c.num_objects)]
        ns = sum(t in (capi.PT_OBJ_SPHERE, capi.PT_OBJ_SPHERE_LIGHT) for t in types)
        nb = sum(t == capi.PT_OBJ_BOX for t in types)
    else:
        ns = sum(o.type in (scn.OBJECT_SPHERE, scn.OBJECT_SPHERE_LIGHT) for o in sc.objects)
        nb = sum(o.type == scn.OBJECT_BOX for o in sc.objects)
    return ns <= 128 and nb <= 128


def pt_config(cfg: RenderConfig) -> capi.PtConfig:
    return capi.PtConfig(cfg.width, cfg.height, cfg.samples_per_px, cfg.max_depth, cfg.seed & 0xFFFFFFFFFFFFFFFF,
                         cfg.spp_chunk, cfg.flags)


_default_ctx: Optional[capi.Context] = None
_default_devices = None


def set_devices(devices) -> None:
    """Devices (HIP ordinals) used by `render`; like the reference's process-wide GL worker."""
    global _default_ctx, _default_devices
    if _default_ctx is not None:
        _default_ctx.close()
        _default_ctx = None
    _default_devices = list(devices) if devices is not None else None


def context() -> capi.Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = capi.Context(devices=_default_devices) if _default_devices else capi.Context(ndev=1)
    return _default_ctx


@dataclass
class _StopRule:
    """How the stepping loop of `render` advances and what ends a frame before the cap."""
    step: int                                    # samples per pt_step
    clip: bool = False                           # ... clipped to what is left of the cap
    stalls: bool = False                         # a step that adds nothing ends the frame (adaptive: every block has stopped)
    check: Optional[Callable[[], float]] = None  # measured after a step once measure_from samples are done; from stop_from
    measure_from: int = 0                        # samples on, a figure at or below target ends the frame
    stop_from: int = 0
    target: float = 0.0


def _ptr(a: Optional[np.ndarray]):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def render(sc, cfg: RenderConfig, img: np.ndarray, progress: Optional[Callable[[], None]] = None,
           accum: Optional[np.ndarray] = None, nseg: Optional[np.ndarray] = None,
           ndraw: Optional[np.ndarray] = None, ctx: Optional[capi.Context] = None, fog: bool = False,
           shading: str = "cpu", moments: Optional[np.ndarray] = None, noise: Optional[float] = None,
           noise_step: int = 16, adaptive: bool = False, min_spp: int = 0, counts: Optional[np.ndarray] = None,
           features: Optional[int] = None, atrous: Optional["AtrousConfig"] = None,
           filtered_noise: Optional[float] = None, halves: bool = False,
           temporal: Optional["TemporalConfig"] = None, temporal_clip: Optional[float] = None,
           object_ids: bool = False, temporal_motion=None, filtered_adaptive: Optional[float] = None, pool: int = 1,
           feature_walk: bool = False, bvh_refit: Optional[float] = None, bvh_build=None, fog_walk: bool = False,
           shading_walk: bool = False, shading_features: bool = False) -> dict:
    """Fills img (uint8 [H, W, 4], C-contiguous rows; row stride may exceed 4*W).

    With fog=True and a scene that has a fog block (`sc.fog`), that block is rendered as the reference's OpenGL backend
    draws it (sky blend, volumetric in-scatter; pt_set_fog in include/ptcore.h); otherwise fog is off for the call, which
    is the CPU engine's image.  (A FlatScene carries no fog block: pass the Scene.)

    shading="gl" renders with the OpenGL backend's estimator (pt_set_shading): samples_per_px counts passes of
    16 paths each, accum holds the sum of the pass sums, and img is GL's tone-mapped finish.  It needs the Scene.

    moments (float64 [H, W, 3]) receives the per-pixel second moments (pt_set_moments).  noise=T renders until
    the frame noise (pt_noise_estimate) is at or below T: samples are added noise_step at a time, the check follows every
    step, and the frame stops at the first check with at least 2 samples done and noise <= T, or at the cap
    cfg.samples_per_px; progress() is called after each step.  The image is that of a frame of the samples done.  With either
    argument the returned dict gains spp_done and noise; without them moments are off for the call.

    adaptive=True (with noise=T) makes T the target of every 8x8 block instead of the frame's (pt_set_adaptive):
    samples are added noise_step at a time, after each step (once max(min_spp, 2) samples are done) the blocks at or below T stop,
    and the frame ends when no block is active or at the cap.  Every pixel is normalised by its own count; counts (uint32
    [H, W]) receives them, and the returned dict gains "adaptive": the pt_adaptive_state of the frame (spp_done is its spp_max).

    features=k collects the first-hit feature planes over every pixel's first k samples (pt_set_features; read
    them with read_features(ctx, ...) afterwards -- that needs moments on).  atrous=AtrousConfig() turns moments on, renders, and
    then replaces img by the a-trous filtered image (pt_atrous); features then defaults to the config's value, or to 4 where the
    scene allows features (scene_allows_features) and 0 where it does not.  The returned dict gains "atrous": the pt_atrous_stats.
    Without the two arguments features are off for the call.

    filtered_noise=T (with atrous=) renders until the *filtered* frame is good enough: the frame collects the
    half-buffer sums (pt_set_halves), samples are added noise_step at a time, after every step with at least 4 samples done
    pt_atrous_halves runs with the filter's configuration, and the frame stops at the first check whose measured `noise` is at or
    below T, or at the cap cfg.samples_per_px.  The image is pt_atrous on the full sums: that of a plain frame of the samples done.
    It excludes noise= and adaptive=True.  The returned dict gains filtered_noise and noise_model (the last check's two figures;
    inf when no check ran) and spp_done.  Neither figure sees the bias the filter adds.  halves=True collects the half-buffer
    sums without the stop rule (read them with read_halves / atrous_halves afterwards); without the two arguments halves are off.

    filtered_adaptive=T (with atrous=) is adaptive sampling by the filtered frame's noise: an adaptive frame (counts=,
    "adaptive" in the returned dict, noise_step and min_spp as above, a min_spp below 4 counting as 4) whose blocks stop when the noise
    measured in the filtered frame, pooled over the blocks within `pool` blocks (0..4) of each, is at or below T
    (pt_set_adaptive_filtered).  The image is pt_atrous on the full sums with every pixel's own count.  It excludes noise=,
    adaptive=True and filtered_noise=.  The returned dict gains "block_checks", the checks that decided.

    temporal=TemporalConfig() is for a caller that renders frame after frame on one context while the camera
    moves: it turns moments and features on (k = 4 unless features= or the filter's config says otherwise), renders, and then
    calls pt_temporal with atrous= as its filter (None: no filter); img is its output and the returned dict gains "temporal": the
    pt_temporal_stats.  It excludes nothing that atrous= allows.  Change cfg.seed from frame to frame; call temporal_reset(ctx)
    after editing the scene.  temporal_clip=gamma (with temporal=) sets the context's history clip first (temporal_set_clip,
    DESIGN 3.13a; 2.5 is the recommended value, 0 turns it off) and the "temporal" dict gains "clipped"; None leaves the context's
    setting as it is, which is off unless temporal_set_clip was called.

    object_ids=True also records the per-pixel object index plane (pt_set_object_ids; read it with
    read_object_ids(ctx, ...) afterwards); it turns features on (k = 4) where nothing else did.  temporal_motion=delta (with
    temporal=; [n, 3], see scene_motion) turns object ids on and passes the objects' displacements since the last accumulated
    frame to pt_temporal (temporal_set_motion); the "temporal" dict gains "objects", "moved" and "moved_reprojected".

    feature_walk=True lets a scene on the bounding-volume-hierarchy path collect features (pt_set_feature_walk;
    feature_walk_stats(ctx) afterwards says what the walk did): atrous=, temporal= and object_ids= then work there as on the small
    scenes.  Without it such a scene has features refused, and atrous= alone filters it with k = 0.

    fog_walk=True lets a scene on the bounding-volume-hierarchy path render a gpu_volumetric fog block
    (pt_set_fog_walk; fog_walk_stats(ctx) afterwards says what the walks did).  The frame is the model's, bit for bit; the cost
    stays 24 x lights shadow rays per sample.  Without it such a frame is refused.

    shading_walk=True lets a scene on the bounding-volume-hierarchy path render with shading="gl"
    (pt_set_shading_walk; shading_walk_stats(ctx) afterwards says what the walks did).  The frame is the model's, bit for bit.
    Without it such a frame is refused; with it a gpu_volumetric fog block, features, adaptive sampling and pixel statistics
    stay refused there.

    shading_features=True lets a shading="gl" frame take features=k (k counts passes of 16 paths; the planes are
    those of the GL pass's own camera rays), object_ids=, atrous= (img is then GL's tone map of the filtered mean; features
    defaults to 1 where the scene allows them), filtered_noise= and halves= (pt_set_shading_features).  Without it they stay
    refused.  temporal=, adaptive=True and filtered_adaptive= stay refused with GL shading either way.

    bvh_refit=G (G >= 1 or inf, 0 = off) lets a frame whose scene differs from the context's previous frame only in
    where its objects are refit the bounding-volume hierarchy on the devices instead of rebuilding it on the host
    (pt_set_bvh_refit; bvh_refit_stats(ctx) afterwards says what happened).  The frame is the one a rebuild gives, bit for bit.
    None leaves the context's setting as it is, which is off unless set_bvh_refit was called.

    bvh_build="device" ("host" = 0 is the default) lets every full build of the hierarchy on the context run on
    devices[0] in Morton order instead of on the host (pt_set_bvh_build; bvh_build_stats(ctx) afterwards says who built the tree).
    The frame is the one the host-built tree gives, bit for bit.  None leaves the context's setting as it is.

    With `progress`, samples are added in ~10 steps and progress() is called after each
    (the cadence of gpu.go:2209-2212, :2229) and once at the end (gpu.go:2523-2525).
    Returns the pt_stats of the frame as a dict.
    """
    if temporal_clip is not None and temporal is None:
        raise ValueError("temporal_clip needs the accumulation it clips (temporal=)")
    if temporal_motion is not None and temporal is None:
        raise ValueError("temporal_motion needs the accumulation it displaces (temporal=)")
    if filtered_noise is not None:
        if atrous is None:
            raise ValueError("filtered_noise needs the filter whose output it measures (atrous=)")
        if noise is not None or adaptive:
            raise ValueError("filtered_noise excludes noise= and adaptive=True: one stop rule per frame")
        if shading != "cpu" and not shading_features:
            raise ValueError("filtered_noise is not available with GL shading (pt_atrous_halves refuses such frames)")
    if filtered_adaptive is not None:
        if atrous is None:
            raise ValueError("filtered_adaptive needs the filter whose output it measures (atrous=)")
        if noise is not None or adaptive or filtered_noise is not None:
            raise ValueError("filtered_adaptive excludes noise=, adaptive=True and filtered_noise=: one stop rule per frame")
        if shading != "cpu":
            raise ValueError("filtered_adaptive is not available with GL shading (adaptive frames refuse it)")
        if not 0 <= int(pool) <= 4:
            raise ValueError("pool must be 0..4 blocks")
        adaptive, noise = True, filtered_adaptive  # from here on an adaptive frame with T as its block target
    L = capi.load()
    ctx = ctx or context()
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 4:
        raise ValueError("img must be uint8 [H, W, 4]")
    if img.shape[0] != cfg.height or img.shape[1] != cfg.width:
        # renderIntoCPU returns silently on a size mismatch (renderer.go:46-49)
        return {}
    if img.strides[2] != 1 or img.strides[1] != 4:
        raise ValueError("img rows must be contiguous RGBA")
    flat = sc if isinstance(sc, FlatScene) else FlatScene(sc)  # callers that render one scene repeatedly flatten it once
    set_fog(ctx, getattr(sc, "fog", None) if fog else None)
    if bool(fog_walk) != getattr(ctx, "_fog_walk_on", False):  # (said only when it changes: with it never on, the calls are what they were)
        set_fog_walk(ctx, bool(fog_walk))
    if bool(shading_walk) != getattr(ctx, "_shading_walk_on", False):  # (the same)
        set_shading_walk(ctx, bool(shading_walk))
    if bool(shading_features) != getattr(ctx, "_shading_features_on", False):  # (the same)
        set_shading_features(ctx, bool(shading_features))
    if shading != "cpu" or capi.has("pt_set_shading"):
        set_shading(ctx, shading, sc)
    if adaptive and noise is None:
        raise ValueError("adaptive needs the block noise target (noise=)")
    if counts is not None and (not adaptive or counts.dtype != np.uint32 or counts.shape != (cfg.height, cfg.width)
                               or not counts.flags.c_contiguous):
        raise ValueError("counts needs adaptive=True and a contiguous uint32 [H, W] array")
    if temporal_clip is not None:
        temporal_set_clip(ctx, temporal_clip)
    set_adaptive(ctx, noise if adaptive else None, min_spp, noise_step)
    if (filtered_adaptive is not None) or getattr(ctx, "_filtered_adaptive_on", False):  # (said only where it was ever on)
        set_adaptive_filtered(ctx, atrous, pool, on=filtered_adaptive is not None)
        ctx._filtered_adaptive_on = filtered_adaptive is not None
    want_moments = moments is not None or noise is not None or atrous is not None or halves or temporal is not None
    set_moments(ctx, want_moments)
    set_halves(ctx, halves or filtered_noise is not None)
    fstats = {"filtered_noise": float("inf"), "noise_model": float("inf")}
    if features is None:
        features = 0
        if atrous is not None:
            if atrous.features is not None:
                features = atrous.features
            elif shading != "cpu":  # (k counts passes there: 1 is 16 paths)
                features = 1 if scene_allows_features(sc, shading, feature_walk, shading_features=shading_features, shading_walk=shading_walk) else 0
            else:
                features = 4 if scene_allows_features(sc, shading, feature_walk) else 0
        if temporal is not None and not features:  # (where the scene refuses features, pt_temporal says so)
            features = 4
        if (object_ids or temporal_motion is not None) and not features:
            features = 4
    if bool(feature_walk) != getattr(ctx, "_feature_walk_on", False):  # (said only when it changes: with it never on, the calls are what they were)
        set_feature_walk(ctx, bool(feature_walk))
    if bvh_refit is not None and float(bvh_refit) != getattr(ctx, "_bvh_refit", 0.0):  # (said only when it changes: with it never on, the calls are what they were)
        set_bvh_refit(ctx, float(bvh_refit))
    if bvh_build is not None and _bvh_build_mode(bvh_build) != getattr(ctx, "_bvh_build", 0):  # (the same rule)
        set_bvh_build(ctx, bvh_build)
    set_features(ctx, features)
    want_ids = object_ids or temporal_motion is not None
    if want_ids != getattr(ctx, "_object_ids_on", False):  # (said only when it changes: with it never on, the calls are what they were)
        set_object_ids(ctx, want_ids)
    if moments is not None and (moments.dtype != np.float64 or moments.shape != (cfg.height, cfg.width, 3)
                                or not moments.flags.c_contiguous):
        raise ValueError("moments must be contiguous float64 [H, W, 3]")
    pc = pt_config(cfg)
    st = capi.PtStats()
    if accum is not None and (accum.dtype != np.float64 or accum.shape != (cfg.height, cfg.width, 3)
                              or not accum.flags.c_contiguous):
        raise ValueError("accum must be contiguous float64 [H, W, 3]")
    for a in (nseg, ndraw):
        if a is not None and (a.dtype != np.uint32 or a.shape != (cfg.height, cfg.width) or not a.flags.c_contiguous):
            raise ValueError("nseg/ndraw must be contiguous uint32 [H, W]")
    stride = int(img.strides[0])

    def with_moments(d: dict) -> dict:  # after pt_end: the sums stay readable until the next frame opens
        if want_moments and cfg.samples_per_px > 0:
            if moments is not None:
                read_moments(ctx, moments)
            d.update(noise=noise_estimate(ctx)["noise"])
            if temporal is not None:  # the accumulated (and filtered) image takes the place of the plain finish
                if temporal_motion is not None:
                    temporal_set_motion(ctx, temporal_motion)
                d["temporal"] = _temporal(ctx, temporal, atrous, img)
                if temporal_clip is not None:
                    d["temporal"]["clipped"] = temporal_clip_stats(ctx)["clipped"]
                if temporal_motion is not None:
                    d["temporal"].update(temporal_motion_stats(ctx))
            elif atrous is not None:  # the filtered image takes the place of the plain finish
                d["atrous"] = _atrous(ctx, atrous, img)
            if filtered_noise is not None:
                d.update(fstats)
            if adaptive:
                d["adaptive"] = adaptive_state(ctx)
                d["spp_done"] = d["adaptive"]["spp_max"]
                if counts is not None:
                    read_sample_counts(ctx, counts)
                if filtered_adaptive is not None:
                    d["block_checks"] = read_block_figures(ctx) if d["spp_done"] >= max(min_spp, 4) else 0
        elif want_moments:
            d.update(noise=float("inf"))
            if filtered_noise is not None:
                d.update(fstats)
        return d

    if progress is None and (noise is None or adaptive) and filtered_noise is None:  # (an adaptive frame steps inside pt_render)
        capi.check(L.pt_render(ctx.handle, C.byref(flat.c), C.byref(pc), _ptr(img), stride, _ptr(accum), _ptr(nseg),
                               _ptr(ndraw), C.byref(st)))
        d = st.as_dict()
        if want_moments:
            d["spp_done"] = max(0, cfg.samples_per_px)
        return with_moments(d)
    if nseg is not None or ndraw is not None:
        raise ValueError("per-pixel stats are only available without a progress callback and without a noise target")
    nz = capi.PtNoise()

    def frame_noise() -> float:
        capi.check(L.pt_noise_estimate(ctx.handle, C.byref(nz)))
        return nz.noise

    def filtered_frame_noise() -> float:
        nonlocal fstats
        hs = atrous_halves(ctx, atrous)
        fstats = {"filtered_noise": hs["noise"], "noise_model": hs["noise_model"]}
        return hs["noise"]

    nstep = max(1, int(noise_step))
    if adaptive:  # the blocks stop inside pt_step
        rule = _StopRule(nstep, stalls=True)
    elif filtered_noise is not None:  # each half needs two samples for its variance
        rule = _StopRule(nstep, clip=True, check=filtered_frame_noise, measure_from=4, stop_from=4, target=filtered_noise)
    elif noise is not None:  # the check follows every step
        rule = _StopRule(nstep, clip=True, check=frame_noise, stop_from=2, target=noise)
    else:  # the preview cadence: ~10 steps
        rule = _StopRule(max(1, cfg.samples_per_px // 10))
    capi.check(L.pt_begin(ctx.handle, C.byref(flat.c), C.byref(pc)))
    done = C.c_int32(0)
    try:
        while done.value < cfg.samples_per_px:
            before = done.value
            capi.check(L.pt_step(ctx.handle, min(rule.step, cfg.samples_per_px - before) if rule.clip else rule.step, C.byref(done)))
            if rule.stalls and done.value == before:
                break
            if progress is not None:
                capi.check(L.pt_read(ctx.handle, _ptr(img), stride, _ptr(accum)))
                progress()
            if rule.check is not None and done.value >= rule.measure_from and rule.check() <= rule.target and done.value >= rule.stop_from:
                break
        if progress is None or cfg.samples_per_px <= 0:
            capi.check(L.pt_read(ctx.handle, _ptr(img), stride, _ptr(accum)))
    finally:
        rc = L.pt_end(ctx.handle, C.byref(st))
    capi.check(rc)
    if progress is not None:
        progress()
    d = st.as_dict()
    if want_moments:
        d["spp_done"] = done.value
    return with_moments(d)


@dataclass
class PostConfig:
    """Post-process passes of the reference's OpenGL backend (gpu.go:22-47, :2309-2520); all off by default
    because they are not part of the CPU engine's image."""
    tonemap: bool = False
    denoise: bool = False
    sigma_s: float = 1.0
    sigma_r: float = 0.15
    smooth: bool = False
    smooth_radius: int = 2
    smooth_strength: float = 0.5

    @classmethod
    def from_env(cls, environ=None) -> "PostConfig":
        """The reference's switches: PATHTRACER_GPU_DENOISE (default on there), _SIGMA_S, _SIGMA_R (gpu.go:77-95),
        PATHTRACER_GPU_SMOOTH (default off), _RADIUS, _STRENGTH (gpu.go:140-175); tone mapping always on."""
        env = os.environ if environ is None else environ
        cfg = cls(tonemap=True, denoise=True)
        v = env.get("PATHTRACER_GPU_DENOISE", "").lower()
        if v in ("0", "false", "off", "no"):
            cfg.denoise = False
        for key, attr in (("PATHTRACER_GPU_DENOISE_SIGMA_S", "sigma_s"), ("PATHTRACER_GPU_DENOISE_SIGMA_R", "sigma_r")):
            try:
                f = float(env[key])
                if f > 0:
                    setattr(cfg, attr, f)
            except (KeyError, ValueError):
                pass
        cfg.smooth = _env_on(env, "PATHTRACER_GPU_SMOOTH")
        try:
            cfg.smooth_radius = max(1, min(5, int(env["PATHTRACER_GPU_SMOOTH_RADIUS"])))
        except (KeyError, ValueError):
            pass
        try:
            cfg.smooth_strength = max(0.0, min(1.0, float(env["PATHTRACER_GPU_SMOOTH_STRENGTH"])))
        except (KeyError, ValueError):
            pass
        return cfg


@dataclass
class FogConfig:
    """Whether `render` draws the scene's fog block (off by default: the CPU engine ignores fog)."""
    enabled: bool = False

    @classmethod
    def from_env(cls, environ=None) -> "FogConfig":
        """PATHTRACER_GPU_FOG=1 (or true / on / yes) turns it on, like the PATHTRACER_GPU_* switches of PostConfig."""
        return cls(enabled=_env_on(environ, "PATHTRACER_GPU_FOG"))


@dataclass
class NoiseConfig:
    """The stop rule of `render`: target 0 = off (render cfg.samples_per_px samples), else render until the frame noise is at or
    below it, checking every `step` samples, with cfg.samples_per_px as the cap."""
    target: float = 0.0
    step: int = 16

    @classmethod
    def from_env(cls, environ=None) -> "NoiseConfig":
        """PATHTRACER_GPU_NOISE=<float > 0> and PATHTRACER_GPU_NOISE_STEP=<int >= 1>; anything else keeps the default."""
        return cls(target=_env_positive(environ, "PATHTRACER_GPU_NOISE") or 0.0, step=_env_int(environ, "PATHTRACER_GPU_NOISE_STEP", 1) or 16)

    @property
    def enabled(self) -> bool:
        return self.target > 0


@dataclass
class AdaptiveConfig:
    """Whether the noise target of NoiseConfig is that of every 8x8 block (adaptive sampling) instead of the
    frame's, and the samples every block gets before the first check."""
    enabled: bool = False
    min_spp: int = 0

    @classmethod
    def from_env(cls, environ=None) -> "AdaptiveConfig":
        """PATHTRACER_GPU_ADAPTIVE=1 (or true / on / yes) and PATHTRACER_GPU_ADAPTIVE_MIN_SPP=<int >= 0>; it takes effect
        together with PATHTRACER_GPU_NOISE, whose value is then the block target."""
        return cls(enabled=_env_on(environ, "PATHTRACER_GPU_ADAPTIVE"), min_spp=_env_int(environ, "PATHTRACER_GPU_ADAPTIVE_MIN_SPP", 0) or 0)


@dataclass
class ShadingConfig:
    """Which estimator `render` uses: "cpu" (the CPU engine, default) or "gl" (the OpenGL backend's shader)."""
    model: str = "cpu"

    @classmethod
    def from_env(cls, environ=None) -> "ShadingConfig":
        """PATHTRACER_GPU_SHADING=gl (or cpu; case-insensitive, anything else is cpu), like the other PATHTRACER_GPU_* switches."""
        v = (os.environ if environ is None else environ).get("PATHTRACER_GPU_SHADING", "").strip().lower()
        return cls(model=v if v in SHADING_MODELS else "cpu")


def post_process(img: np.ndarray, post: PostConfig, accum: Optional[np.ndarray] = None, samples_per_px: int = 1,
                 ctx: Optional[capi.Context] = None) -> None:
    """Applies the selected passes to img (uint8 [H, W, 4]) in place on the GPU."""
    L = capi.load()
    ctx = ctx or context()
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 4 or img.strides[2] != 1 or img.strides[1] != 4:
        raise ValueError("img must be uint8 [H, W, 4] with contiguous RGBA rows")
    h, w = img.shape[0], img.shape[1]
    if accum is not None and (accum.dtype != np.float64 or accum.shape != (h, w, 3) or not accum.flags.c_contiguous):
        raise ValueError("accum must be contiguous float64 [H, W, 3]")
    pc = capi.PtPostConfig(int(post.tonemap), int(post.denoise), post.sigma_s, post.sigma_r, int(post.smooth),
                           post.smooth_radius, post.smooth_strength)
    capi.check(L.pt_post_process(ctx.handle, C.byref(pc), _ptr(accum), samples_per_px, _ptr(img), int(img.strides[0]), w, h))
