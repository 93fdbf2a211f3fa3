"""Python mirror of the reference's internal/engine public surface for the hot path.

Names follow /root/reference/internal/engine: RenderConfig, Render, RenderInto
(renderer.go:17-41), Backend / SetBackend / GetBackend (backend.go:5-28),
RenderScene, RenderSettingsForMode, SavePNG (util.go:13-55).  Only the GPU branch
of RenderInto exists here, and it goes to the MI355X core (hip.render) instead of the
OpenGL package.  The CPU branch is the reference's own Go code and is not part of
this package: selecting it raises instead of silently rendering somewhere else.
"""
from __future__ import annotations

import copy
import enum
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np

from . import hip
from . import scene as scn


class Backend(enum.IntEnum):  # backend.go:5-10
    CPU = 0
    GPU = 1


BackendCPU = Backend.CPU
BackendGPU = Backend.GPU

# The reference starts on BackendCPU (backend.go:12); this package has only the GPU branch.
_current_backend = Backend.GPU


def set_backend(b) -> None:
    """SetBackend, backend.go:16-23: unknown values select the CPU backend."""
    global _current_backend
    try:
        _current_backend = Backend(int(b))
    except ValueError:
        _current_backend = Backend.CPU


def get_backend() -> Backend:
    return _current_backend


@dataclass
class RenderConfig:  # renderer.go:17-22
    width: int = 0
    height: int = 0
    samples_per_px: int = 0
    max_depth: int = 0
    seed: int = 1  # stream seed (the reference seeds from the clock, random.go:14-16)


def new_image(w: int, h: int) -> np.ndarray:
    """image.NewRGBA(image.Rect(0, 0, w, h)): zeroed [h, w, 4] uint8."""
    return np.zeros((h, w, 4), np.uint8)


def render_into(sc: scn.Scene, cfg: RenderConfig, img: np.ndarray,
                progress: Optional[Callable[[], None]] = None, shading: Optional[str] = None,
                moments: Optional[np.ndarray] = None, noise: Optional[float] = None, noise_step: Optional[int] = None,
                adaptive: Optional[bool] = None, min_spp: Optional[int] = None, counts: Optional[np.ndarray] = None,
                features: Optional[int] = None, atrous: Optional["hip.AtrousConfig"] = None,
                filtered_noise: Optional[float] = None, temporal: Optional["hip.TemporalConfig"] = None,
                temporal_clip: Optional[float] = None, temporal_motion: Optional[bool] = None,
                filtered_adaptive: Optional[float] = None, pool: Optional[int] = None,
                feature_walk: Optional[bool] = None, bvh_refit: Optional[float] = None, bvh_build=None,
                fog_walk: Optional[bool] = None, shading_walk: Optional[bool] = None,
                shading_features: Optional[bool] = None) -> dict:
    """RenderInto, renderer.go:34-41.  `shading` is "cpu" (the CPU engine's image) or "gl" (the OpenGL backend's estimator,
    DESIGN 3.8); None takes PATHTRACER_GPU_SHADING (hip.ShadingConfig.from_env), which defaults to "cpu".  `moments`, `noise` and
    `noise_step` are hip.render's: render until the frame noise is at or below `noise`, cfg.samples_per_px as the
    cap; noise None takes PATHTRACER_GPU_NOISE / PATHTRACER_GPU_NOISE_STEP (hip.NoiseConfig.from_env), off by default.
    `adaptive`, `min_spp` and `counts` are hip.render's too: with a noise target, every 8x8 block stops at it by
    itself; None takes PATHTRACER_GPU_ADAPTIVE / PATHTRACER_GPU_ADAPTIVE_MIN_SPP (hip.AdaptiveConfig.from_env).  Without a
    noise target adaptive has nothing to adapt to and the frame is a plain one.  `features` and `atrous` are hip.render's as well
    (DESIGN 3.11): the first-hit feature samples per pixel and the a-trous filter that replaces the image; None takes
    PATHTRACER_GPU_FEATURES and PATHTRACER_GPU_ATROUS / PATHTRACER_GPU_ATROUS_ITERS (hip.AtrousConfig.from_env), both off by default.
    `filtered_noise` is hip.render's: with the filter on, render until the measured noise of the filtered frame is at or
    below it; None takes PATHTRACER_GPU_FILTERED_NOISE (hip.filtered_noise_from_env), off by default and ignored without the filter
    or beside a noise target.  `temporal` is hip.render's: the frame is blended into the history the process-wide
    context keeps from call to call (change cfg.seed from frame to frame); None takes PATHTRACER_GPU_TEMPORAL (temporal_setup),
    which also turns on moments, 4 feature samples (unless PATHTRACER_GPU_FEATURES says otherwise) and the filter.  `temporal_clip`
    is hip.render's; None takes PATHTRACER_GPU_TEMPORAL_CLIP=<gamma> (hip.temporal_clip_from_env; unset = off),
    which is read only when PATHTRACER_GPU_TEMPORAL turned the accumulation on.  `temporal_motion` is for an
    editor that drags objects: True records the object index plane, remembers the scene of the last accumulated frame and, frame by
    frame, hands hip.scene_motion's answer on -- a table of displacements goes to pt_temporal, None (anything but positions and the
    camera changed) resets the history, an all-zero table passes nothing; None takes PATHTRACER_GPU_TEMPORAL_MOTION
    (hip.temporal_motion_from_env), which too is read only when PATHTRACER_GPU_TEMPORAL turned the accumulation on.
    `filtered_adaptive` and `pool` are hip.render's: with the filter on, an adaptive frame whose 8x8 blocks stop by the
    filtered frame's pooled noise; None takes PATHTRACER_GPU_FILTERED_ADAPTIVE / PATHTRACER_GPU_POOL (hip.filtered_adaptive_from_env),
    off by default and ignored without the filter; beside a noise target or a filtered noise target it is an error, as in the other host
    layers: one stop rule per frame.  `feature_walk` is hip.render's: features, and with them the filter's feature terms,
    the accumulation and the object ids, on scenes that take the bounding-volume hierarchy; None takes PATHTRACER_GPU_FEATURE_WALK=1
    (hip.feature_walk_from_env), off by default.  `bvh_refit` is hip.render's: the growth bound under which a frame whose
    scene differs from the previous frame's only in where its objects are refits the hierarchy on the devices; None takes
    PATHTRACER_GPU_BVH_REFIT=<G> (hip.bvh_refit_from_env), off by default.  `bvh_build` is hip.render's: "device" builds
    the hierarchy on devices[0] whenever a full build is due; None takes PATHTRACER_GPU_BVH_BUILD=host|device (hip.bvh_build_from_env),
    host by default.  `fog_walk` is hip.render's: a gpu_volumetric fog block on scenes that take the bounding-volume
    hierarchy, the shadow rays answered by the wave's walk of the tree; None takes PATHTRACER_GPU_FOG_WALK=1 (hip.fog_walk_from_env),
    off by default.  `shading_walk` is hip.render's: GL shading on scenes that take the bounding-volume hierarchy,
    the model's ray queries answered by the lane's walk of the tree; None takes PATHTRACER_GPU_SHADING_WALK=1
    (hip.shading_walk_from_env), off by default.  `shading_features` is hip.render's: features, object ids and the
    a-trous filter for GL-shaded frames, the features being those of the GL pass's own camera rays; None takes
    PATHTRACER_GPU_SHADING_FEATURES=1 (hip.shading_features_from_env), off by default."""
    if get_backend() != Backend.GPU:
        raise NotImplementedError(
            "BackendCPU is the reference's Go renderer (renderIntoCPU) and is not shipped here; "
            "this package implements only the GPU branch of RenderInto")
    gcfg = hip.RenderConfig(cfg.width, cfg.height, cfg.samples_per_px, cfg.max_depth, cfg.seed)
    model = shading if shading is not None else hip.ShadingConfig.from_env().model
    ncfg = hip.NoiseConfig.from_env()
    if noise is None and ncfg.enabled:
        noise = ncfg.target
    acfg = hip.AdaptiveConfig.from_env()
    if adaptive is None:
        adaptive = acfg.enabled
    if temporal is None:
        temporal, t_atrous, t_features = temporal_setup()
        if temporal is not None:
            atrous = atrous if atrous is not None else t_atrous
            features = features if features is not None else t_features
            if temporal_clip is None:
                temporal_clip = hip.temporal_clip_from_env()
            if temporal_motion is None:
                temporal_motion = hip.temporal_motion_from_env()
    if atrous is None:
        atrous = hip.AtrousConfig.from_env()
    if features is None:
        features = hip.features_from_env()
    if filtered_noise is None and atrous is not None and noise is None:
        filtered_noise = hip.filtered_noise_from_env()
    rule = {}
    if filtered_adaptive is None and atrous is not None:  # (beside a noise target or a filtered noise target hip.render refuses it)
        filtered_adaptive, env_pool = hip.filtered_adaptive_from_env()
        pool = pool if pool is not None else env_pool
    if filtered_adaptive is not None:
        rule = dict(filtered_adaptive=filtered_adaptive, pool=1 if pool is None else pool)
        adaptive = False  # (the rule brings its own adaptive frame; PATHTRACER_GPU_ADAPTIVE has no noise target to adapt to here)
    if feature_walk is None:
        feature_walk = hip.feature_walk_from_env()
    walk = dict(feature_walk=True) if feature_walk else {}  # (passed only when on: with it off the call is what it was)
    if bvh_refit is None:
        bvh_refit = hip.bvh_refit_from_env()
    if bvh_refit:  # (the same: hip.render leaves the context's setting alone unless told)
        walk["bvh_refit"] = float(bvh_refit)
    if bvh_build is None:
        bvh_build = hip.bvh_build_from_env()
    if bvh_build:  # (the same)
        walk["bvh_build"] = bvh_build
    if fog_walk is None:
        fog_walk = hip.fog_walk_from_env()
    if fog_walk:  # (the same)
        walk["fog_walk"] = True
    if shading_walk is None:
        shading_walk = hip.shading_walk_from_env()
    if shading_walk:  # (the same)
        walk["shading_walk"] = True
    if shading_features is None:
        shading_features = hip.shading_features_from_env()
    if shading_features:  # (the same)
        walk["shading_features"] = True
    motion = {}
    if temporal is not None and temporal_motion:
        motion = _motion_for(sc)
    out = hip.render(sc, gcfg, img, progress, shading=model, features=features, atrous=atrous, moments=moments, noise=noise,
                     noise_step=noise_step if noise_step is not None else ncfg.step, adaptive=bool(adaptive) and noise is not None,
                     min_spp=min_spp if min_spp is not None else acfg.min_spp, counts=counts, filtered_noise=filtered_noise,
                     temporal=temporal, temporal_clip=temporal_clip if temporal is not None else None, **motion, **rule, **walk)
    if "temporal" in out:
        global _accumulated_scene
        # (the caller edits its scene in place; a frame accumulated without the rule is not what the next table is against)
        _accumulated_scene = copy.deepcopy(sc) if motion else None
    return out


# The scene of the last frame that render_into accumulated with temporal_motion on, on the process-wide context (None: none yet).
_accumulated_scene: Optional[scn.Scene] = None


def _motion_for(sc: scn.Scene) -> dict:
    """The host rule of displaced reprojection: hip.render's arguments for a frame of `sc` after the remembered
    scene.  Object ids are on; a table of displacements is passed on, an all-zero one is not, and when anything but positions and
    the camera changed the history is reset here."""
    delta = hip.scene_motion(_accumulated_scene, sc) if _accumulated_scene is not None else None
    if _accumulated_scene is not None and delta is None:
        hip.temporal_reset(hip.context())
    if delta is not None and not delta.any():
        delta = None
    return dict(object_ids=True, temporal_motion=delta)


def temporal_setup(environ=None):
    """PATHTRACER_GPU_TEMPORAL=1: (the accumulation's config, the filter's, the feature samples) that the switch turns on -- the
    filter with PATHTRACER_GPU_ATROUS_ITERS, k = PATHTRACER_GPU_FEATURES or 4; (None, None, None) when it is off."""
    import os

    env = os.environ if environ is None else environ
    t = hip.TemporalConfig.from_env(env)
    if t is None:
        return None, None, None
    a = hip.AtrousConfig.from_env(dict(env, PATHTRACER_GPU_ATROUS="1"))
    k = a.features if a.features is not None else 4
    a.features = None
    return t, a, k


def render(sc: scn.Scene, cfg: RenderConfig) -> np.ndarray:
    """Render, renderer.go:25-29."""
    img = new_image(cfg.width, cfg.height)
    render_into(sc, cfg, img, None)
    return img


def render_scene(sc: scn.Scene, settings: scn.RenderSettings, seed: int = 1) -> np.ndarray:
    """RenderScene, util.go:13-22."""
    return render(sc, RenderConfig(settings.width, settings.height, settings.samples_per_px, settings.max_depth, seed))


def render_settings_for_mode(mode: str) -> scn.RenderSettings:
    """RenderSettingsForMode, util.go:25-42."""
    if mode == "final":
        return scn.RenderSettings(1920, 1080, 1000, 80)
    return scn.RenderSettings(400, 225, 20, 20)


def render_settings_for_scene(sc: scn.Scene, mode: str) -> scn.RenderSettings:
    """The editor's scene-settings override, internal/ui/app.go:60-75: the mode preset, replaced by the scene's
    width x height when both are > 0 (and only then by its samples_per_px / max_depth when > 0); a "final"
    render then takes 4x the samples and 2x the depth.  cmd/render itself ignores scene.settings (main.go:52)."""
    s = render_settings_for_mode(mode)
    st = sc.settings
    if st.width > 0 and st.height > 0:
        s.width, s.height = st.width, st.height
        if st.samples_per_px > 0:
            s.samples_per_px = st.samples_per_px
        if st.max_depth > 0:
            s.max_depth = st.max_depth
    if mode == "final":
        s.samples_per_px *= 4
        s.max_depth *= 2
    return s


def save_png(path: str, img: np.ndarray) -> None:
    """SavePNG, util.go:45-55: 8-bit RGBA PNG."""
    from PIL import Image

    try:
        Image.fromarray(np.ascontiguousarray(img), "RGBA").save(path, format="PNG")
    except OSError as e:
        raise OSError("create png: %s" % e) from e
