"""ctypes binding of include/ptcore.h (libptcore.so).

This is the only way Python reaches the renderer: there is no Python or CPU
rendering path in this package.  If the library has not been built, or no HIP
device is present, the calls raise -- they never fall back.

A process that also uses torch must `import torch` BEFORE the first capi.load(): torch bundles
its own libamdhip64.so.7, and loading it first lets libptcore.so bind to that same copy (one HIP
runtime, so torch streams and device pointers are valid inside libptcore).  The other order
loads two HIP runtimes and torch then reports no GPUs.
"""
from __future__ import annotations

import ctypes as C
import os

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PTCORE_LIB") or os.path.join(PKG, "libptcore.so")  # PTCORE_LIB: another build of the same ABI (A/B runs)

PT_ABI_VERSION = 4
PT_OK, PT_ERR_INVALID, PT_ERR_NO_DEVICE, PT_ERR_HIP, PT_ERR_NOMEM, PT_ERR_STATE = range(6)
PT_MAT_LAMBERT, PT_MAT_METAL, PT_MAT_DIELECTRIC, PT_MAT_EMISSIVE, PT_MAT_MIRROR = range(5)
PT_OBJ_UNKNOWN, PT_OBJ_SPHERE, PT_OBJ_PLANE, PT_OBJ_BOX, PT_OBJ_SPHERE_LIGHT = -1, 0, 1, 2, 3
PT_SKY_BACKGROUND, PT_SKY_GRADIENT, PT_SKY_SOLID = range(3)
PT_FLAG_NONE, PT_FLAG_PIXEL_STATS = 0, 1

_d3 = C.c_double * 3


class PtMaterial(C.Structure):
    _fields_ = [("type", C.c_int32), ("reserved", C.c_int32), ("albedo", _d3), ("rough", C.c_double),
                ("ior", C.c_double), ("emit", _d3), ("power", C.c_double), ("absorption", _d3),
                ("smoothness", C.c_double)]


class PtObject(C.Structure):
    _fields_ = [("type", C.c_int32), ("material", C.c_int32), ("position", _d3), ("size", _d3)]


class PtCamera(C.Structure):
    _fields_ = [("position", _d3), ("target", _d3), ("up", _d3), ("fov", C.c_double), ("aperture", C.c_double),
                ("focus_dist", C.c_double), ("aspect_ratio", C.c_double)]


class PtSky(C.Structure):
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("background", _d3), ("color", _d3),
                ("horizon", _d3), ("zenith", _d3)]


class PtScene(C.Structure):
    _fields_ = [("camera", PtCamera), ("sky", PtSky), ("num_materials", C.c_int32), ("num_objects", C.c_int32),
                ("materials", C.POINTER(PtMaterial)), ("objects", C.POINTER(PtObject))]


class PtConfig(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("samples_per_px", C.c_int32),
                ("max_depth", C.c_int32), ("seed", C.c_uint64), ("spp_chunk", C.c_int32), ("flags", C.c_int32)]


class PtPostConfig(C.Structure):
    _fields_ = [("tonemap", C.c_int32), ("denoise", C.c_int32), ("sigma_s", C.c_double), ("sigma_r", C.c_double),
                ("smooth", C.c_int32), ("smooth_radius", C.c_int32), ("smooth_strength", C.c_double)]


class PtFog(C.Structure):  # scene.Fog (internal/scene/scene.go:101-131), raw fields; resolved inside libptcore
    _fields_ = [("density", C.c_double), ("color", _d3), ("scatter", C.c_double), ("sigma_s", C.c_double),
                ("sigma_a", C.c_double), ("g", C.c_double), ("hetero_strength", C.c_double),
                ("noise_scale", C.c_double), ("noise_octaves", C.c_int32), ("affect_sky", C.c_int32),
                ("gpu_volumetric", C.c_int32), ("reserved", C.c_int32)]


class PtFogStats(C.Structure):
    _fields_ = [("fog_ms", C.c_double), ("fog_launches", C.c_int32), ("reserved", C.c_int32),
                ("shadow_rays", C.c_uint64), ("draws", C.c_uint64), ("steps", C.c_uint64)]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}


class PtGlMaterial(C.Structure):  # scene.Material fields only GL shading reads (scene.go:41-63), raw
    _fields_ = [("reflectivity", C.c_double), ("tint", _d3), ("absorption_scale", C.c_double)]


class PtShading(C.Structure):
    _fields_ = [("model", C.c_int32), ("num_materials", C.c_int32), ("materials", C.POINTER(PtGlMaterial))]


class PtShadingStats(C.Structure):
    _fields_ = [("gl_ms", C.c_double), ("gl_launches", C.c_int32), ("reserved", C.c_int32), ("paths", C.c_uint64),
                ("segments", C.c_uint64), ("shadow_rays", C.c_uint64), ("probe_rays", C.c_uint64), ("draws", C.c_uint64)]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}


PT_SHADING_CPU, PT_SHADING_GL = 0, 1


class PtNoise(C.Structure):  # pt_noise: the frame noise figure of pt_noise_estimate (the metric is stated in include/ptcore.h)
    _fields_ = [("noise", C.c_double), ("max_pixel", C.c_double), ("pixels", C.c_uint64), ("bad_pixels", C.c_uint64),
                ("spp", C.c_int32), ("reserved", C.c_int32)]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}


class PtAdaptive(C.Structure):  # pt_adaptive: block noise target, samples before the first check, pt_render's step
    _fields_ = [("target", C.c_double), ("min_spp", C.c_int32), ("step", C.c_int32)]


class PtAdaptiveState(C.Structure):  # struct pt_adaptive_state: the block table of an adaptive frame
    _fields_ = [("blocks", C.c_uint64), ("active_blocks", C.c_uint64), ("samples", C.c_uint64), ("spp_min", C.c_int32),
                ("spp_max", C.c_int32), ("worst_active", C.c_double)]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_}


class PtAtrousConfig(C.Structure):  # pt_atrous_config: iterations and the four sigmas of the a-trous filter
    _fields_ = [("iterations", C.c_int32), ("reserved", C.c_int32), ("sigma_l", C.c_double), ("sigma_n", C.c_double),
                ("sigma_z", C.c_double), ("sigma_a", C.c_double)]


class PtAtrousStats(C.Structure):  # pt_atrous_stats
    _fields_ = [("atrous_ms", C.c_double), ("launches", C.c_int32), ("iterations", C.c_int32), ("noise_before", C.c_double),
                ("noise_after", C.c_double), ("bad_pixels", C.c_uint64)]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_}


class PtHalvesStats(C.Structure):  # pt_halves_stats
    _fields_ = [("atrous_ms", C.c_double), ("launches", C.c_int32), ("iterations", C.c_int32), ("noise", C.c_double),
                ("noise_model", C.c_double), ("bad_pixels", C.c_uint64), ("spp_min", C.c_int32), ("reserved", C.c_int32)]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}


class PtAdaptiveFiltered(C.Structure):  # pt_adaptive_filtered: the filter whose output is measured and the pool radius in blocks
    _fields_ = [("filter", PtAtrousConfig), ("pool", C.c_int32), ("reserved", C.c_int32)]


class PtTemporalConfig(C.Structure):  # pt_temporal_config: the blend weight, the tap tests and the history length of pt_temporal
    _fields_ = [("alpha", C.c_double), ("tol_z", C.c_double), ("n_min", C.c_double), ("tol_a", C.c_double),
                ("max_len", C.c_int32), ("reserved", C.c_int32)]


class PtTemporalClipStats(C.Structure):  # struct pt_temporal_clip_stats: of the last pt_temporal that succeeded
    _fields_ = [("gamma", C.c_double), ("clipped", C.c_uint64), ("reprojected", C.c_uint64)]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_}


class PtTemporalMotionStats(C.Structure):  # struct pt_temporal_motion_stats: of the last pt_temporal that succeeded
    _fields_ = [("objects", C.c_int32), ("reserved", C.c_int32), ("moved", C.c_uint64), ("moved_reprojected", C.c_uint64)]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}


PT_BVH_REASON_NONE, PT_BVH_REASON_FIRST, PT_BVH_REASON_OFF, PT_BVH_REASON_CHANGED, PT_BVH_REASON_NOT_BVH, PT_BVH_REASON_GROWTH, \
    PT_BVH_REASON_NONFINITE = range(7)


class PtBvhRefitStats(C.Structure):  # struct pt_bvh_refit_stats: what the scene preparations of a context did (pt_set_bvh_refit)
    _fields_ = [("builds", C.c_uint64), ("refits", C.c_uint64), ("last_action", C.c_int32), ("last_build_reason", C.c_int32),
                ("cost_built", C.c_double), ("cost_now", C.c_double), ("refit_ms", C.c_double)]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_}


PT_BVH_BUILDER_NONE, PT_BVH_BUILDER_HOST, PT_BVH_BUILDER_DEVICE = range(3)
PT_BVH_BUILD_FALLBACK_NONE, PT_BVH_BUILD_FALLBACK_STACK, PT_BVH_BUILD_FALLBACK_WALK32, PT_BVH_BUILD_FALLBACK_NOT_BVH = range(4)


class PtBvhBuildStats(C.Structure):  # struct pt_bvh_build_stats: who built the hierarchy of a context's scenes (pt_set_bvh_build)
    _fields_ = [("host_builds", C.c_uint64), ("device_builds", C.c_uint64), ("builder", C.c_int32), ("last_fallback", C.c_int32),
                ("nodes", C.c_int32), ("depth", C.c_int32), ("stack_need", C.c_int32), ("reserved", C.c_int32), ("cost", C.c_double),
                ("device_ms", C.c_double), ("prepare_ms", C.c_double), ("upload_ms", C.c_double), ("readback_ms", C.c_double)]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}


class PtTemporalStats(C.Structure):  # pt_temporal_stats
    _fields_ = [("temporal_ms", C.c_double), ("launches", C.c_int32), ("iterations", C.c_int32), ("reprojected", C.c_uint64),
                ("disoccluded", C.c_uint64), ("bad_pixels", C.c_uint64), ("mean_len", C.c_double), ("noise_before", C.c_double),
                ("noise_blended", C.c_double), ("noise_after", C.c_double)]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_}


class PtShard(C.Structure):
    _fields_ = [("index", C.c_int32), ("count", C.c_int32)]


class PtStats(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("segments", C.c_uint64), ("exit_scans", C.c_uint64),
                ("draws", C.c_uint64), ("seconds", C.c_double), ("trace_ms", C.c_double),
                ("resolve_ms", C.c_double), ("device_ms", C.c_double), ("trace_launches", C.c_int32),
                ("resolve_launches", C.c_int32), ("spp_chunk", C.c_int32), ("num_devices", C.c_int32),
                ("per_device_ms", C.c_double * 8), ("raygen_ms", C.c_double), ("glass_ms", C.c_double),
                ("trace_split_ms", C.c_double), ("glass_launches", C.c_int32), ("trace_split_launches", C.c_int32),
                ("glass_events", C.c_uint64), ("continuations", C.c_uint64), ("split_cont_in", C.c_uint64),
                ("split_finished", C.c_uint64), ("shader_clock_mhz", C.c_double)]

    def as_dict(self) -> dict:
        d = {n: getattr(self, n) for n, _ in self._fields_ if n != "per_device_ms"}
        d["per_device_ms"] = list(self.per_device_ms)[: max(1, self.num_devices)]
        return d


# every symbol include/ptcore.h declares: (name, restype, argtypes)
_vp = C.c_void_p
SYMBOLS = [
    ("pt_abi_version", C.c_int32, []),
    ("pt_last_error", C.c_char_p, []),
    ("pt_device_count", C.c_int32, [C.POINTER(C.c_int32)]),
    ("pt_create", C.c_int32, [C.POINTER(C.c_int32), C.c_int32, C.POINTER(_vp)]),
    ("pt_destroy", None, [_vp]),
    ("pt_render", C.c_int32, [_vp, C.POINTER(PtScene), C.POINTER(PtConfig), _vp, C.c_int32, _vp, _vp, _vp,
                               C.POINTER(PtStats)]),
    ("pt_begin", C.c_int32, [_vp, C.POINTER(PtScene), C.POINTER(PtConfig)]),
    ("pt_step", C.c_int32, [_vp, C.c_int32, C.POINTER(C.c_int32)]),
    ("pt_read", C.c_int32, [_vp, _vp, C.c_int32, _vp]),
    ("pt_end", C.c_int32, [_vp, C.POINTER(PtStats)]),
    ("pt_shard_tiles", C.c_int32, [C.c_int32, C.c_int32, C.POINTER(PtShard), C.POINTER(C.c_int32),
                                    C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("pt_render_tiles_device", C.c_int32, [_vp, C.POINTER(PtScene), C.POINTER(PtConfig), C.POINTER(PtShard), _vp, _vp,
                                            _vp, C.POINTER(PtStats)]),
    ("pt_untile_device", C.c_int32, [_vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_int32, _vp,
                                      _vp]),
    ("pt_post_process", C.c_int32, [_vp, C.POINTER(PtPostConfig), _vp, C.c_int32, _vp, C.c_int32, C.c_int32, C.c_int32]),
    ("pt_set_fog", C.c_int32, [_vp, C.POINTER(PtFog)]),
    ("pt_fog_last_stats", C.c_int32, [_vp, C.POINTER(PtFogStats)]),
    ("pt_set_shading", C.c_int32, [_vp, C.POINTER(PtShading)]),          # additive to ABI 4 (see has())
    ("pt_shading_last_stats", C.c_int32, [_vp, C.POINTER(PtShadingStats)]),
    ("pt_set_moments", C.c_int32, [_vp, C.c_int32]),                     # additive to ABI 4 (see has())
    ("pt_read_moments", C.c_int32, [_vp, C.POINTER(C.c_double)]),
    ("pt_noise_estimate", C.c_int32, [_vp, C.POINTER(PtNoise)]),
    ("pt_set_adaptive", C.c_int32, [_vp, C.POINTER(PtAdaptive)]),         # additive to ABI 4 (see has())
    ("pt_adaptive_state", C.c_int32, [_vp, C.POINTER(PtAdaptiveState)]),
    ("pt_read_sample_counts", C.c_int32, [_vp, C.POINTER(C.c_uint32)]),
    ("pt_set_features", C.c_int32, [_vp, C.c_int32]),                     # additive to ABI 4 (see has())
    ("pt_read_features", C.c_int32, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("pt_set_feature_walk", C.c_int32, [_vp, C.c_int32]),                 # additive to ABI 4 (see has())
    ("pt_feature_walk_stats", C.c_int32, [_vp, C.POINTER(C.c_uint64)]),
    ("pt_set_fog_walk", C.c_int32, [_vp, C.c_int32]),                     # additive to ABI 4 (see has())
    ("pt_fog_walk_stats", C.c_int32, [_vp, C.POINTER(C.c_uint64)]),
    ("pt_set_shading_walk", C.c_int32, [_vp, C.c_int32]),                 # additive to ABI 4 (see has())
    ("pt_shading_walk_stats", C.c_int32, [_vp, C.POINTER(C.c_uint64)]),
    ("pt_set_shading_features", C.c_int32, [_vp, C.c_int32]),             # additive to ABI 4 (see has())
    ("pt_set_object_ids", C.c_int32, [_vp, C.c_int32]),                   # additive to ABI 4 (see has())
    ("pt_read_object_ids", C.c_int32, [_vp, C.POINTER(C.c_int32)]),
    ("pt_atrous", C.c_int32, [_vp, C.POINTER(PtAtrousConfig), _vp, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double),
                               C.POINTER(PtAtrousStats)]),
    ("pt_set_halves", C.c_int32, [_vp, C.c_int32]),                       # additive to ABI 4 (see has())
    ("pt_read_halves", C.c_int32, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("pt_atrous_halves", C.c_int32, [_vp, C.POINTER(PtAtrousConfig), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                      C.POINTER(C.c_double), C.POINTER(PtHalvesStats)]),
    ("pt_set_adaptive_filtered", C.c_int32, [_vp, C.POINTER(PtAdaptiveFiltered)]),  # additive to ABI 4 (see has())
    ("pt_read_block_figures", C.c_int32, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32)]),
    ("pt_temporal", C.c_int32, [_vp, C.POINTER(PtTemporalConfig), C.POINTER(PtAtrousConfig), _vp, C.c_int32, C.POINTER(C.c_double),
                                 C.POINTER(C.c_double), C.POINTER(PtTemporalStats)]),  # additive to ABI 4 (see has())
    ("pt_temporal_read", C.c_int32, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32)]),
    ("pt_temporal_reset", C.c_int32, [_vp]),
    ("pt_temporal_set_clip", C.c_int32, [_vp, C.c_double]),
    ("pt_temporal_clip_stats", C.c_int32, [_vp, C.POINTER(PtTemporalClipStats)]),
    ("pt_temporal_set_motion", C.c_int32, [_vp, C.POINTER(C.c_double), C.c_int32]),
    ("pt_temporal_motion_stats", C.c_int32, [_vp, C.POINTER(PtTemporalMotionStats)]),
    ("pt_set_bvh_refit", C.c_int32, [_vp, C.c_double]),                    # additive to ABI 4 (see has())
    ("pt_bvh_refit_stats", C.c_int32, [_vp, C.POINTER(PtBvhRefitStats)]),
    ("pt_debug_bvh_refit_check", C.c_int32, [C.POINTER(PtScene), C.POINTER(PtScene), C.POINTER(C.c_int32)]),
    ("pt_set_bvh_build", C.c_int32, [_vp, C.c_int32]),                     # additive to ABI 4 (see has())
    ("pt_bvh_build_stats", C.c_int32, [_vp, C.POINTER(PtBvhBuildStats)]),
    ("pt_debug_bvh_build_check", C.c_int32, [C.POINTER(PtScene), C.POINTER(C.c_int32)]),
    ("pt_debug_profile", C.c_int32, [_vp, C.POINTER(C.c_uint64), C.c_int32]),
    ("pt_debug_scan_mismatches", C.c_int64, [_vp]),
    ("pt_debug_div_selftest", C.c_int64, [_vp, C.c_int32, C.c_uint64]),
    ("pt_debug_bvh_check", C.c_int32, [C.POINTER(PtScene), C.POINTER(C.c_int32)]),
    ("pt_debug_gather_mode", C.c_int32, [_vp]),
    ("pt_debug_set_primary_rays", C.c_int32, [_vp, C.POINTER(C.c_double), C.c_int64]),  # additive to ABI 4 (see has())
]


class PtError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__("ptcore error %d: %s" % (code, msg))
        self.code = code


_lib = None


def load():
    """Loads libptcore.so; raises if it was not built (run path_trace_golang_amd.build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s is missing: build it with `python -m path_trace_golang_amd.build` "
                              "(there is no fallback renderer)" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            f = getattr(L, name, None)
            if f is None:
                if name in ADDITIVE:  # a library from before these entry points (PTCORE_LIB A/B runs): has() says no
                    continue
                getattr(L, name)  # AttributeError: the symbol is not exported
            f.restype = res
            f.argtypes = args
        if L.pt_abi_version() != PT_ABI_VERSION:
            raise ImportError("libptcore.so ABI %d != binding %d" % (L.pt_abi_version(), PT_ABI_VERSION))
        _lib = L
    return _lib


ADDITIVE = ("pt_set_shading", "pt_shading_last_stats", "pt_debug_set_primary_rays", "pt_set_moments", "pt_read_moments",
            "pt_noise_estimate", "pt_set_adaptive", "pt_adaptive_state", "pt_read_sample_counts", "pt_set_features",
            "pt_read_features", "pt_atrous", "pt_set_halves", "pt_read_halves", "pt_atrous_halves", "pt_temporal", "pt_temporal_read",
            "pt_temporal_reset", "pt_temporal_set_clip", "pt_temporal_clip_stats", "pt_set_object_ids", "pt_read_object_ids",
            "pt_temporal_set_motion", "pt_temporal_motion_stats", "pt_set_adaptive_filtered", "pt_read_block_figures",
            "pt_set_feature_walk", "pt_feature_walk_stats", "pt_set_fog_walk", "pt_fog_walk_stats", "pt_set_shading_walk", "pt_shading_walk_stats", "pt_set_shading_features", "pt_set_bvh_refit", "pt_bvh_refit_stats",
            "pt_debug_bvh_refit_check", "pt_set_bvh_build", "pt_bvh_build_stats",
            "pt_debug_bvh_build_check")  # added within ABI 4: detected by presence


def has(name: str) -> bool:
    """Does the loaded libptcore.so export `name` (the ADDITIVE entry points may be missing from an older build)?"""
    return getattr(load(), name, None) is not None


def check(rc: int) -> None:
    if rc != PT_OK:
        raise PtError(rc, (load().pt_last_error() or b"").decode("utf-8", "replace"))


def device_count() -> int:
    n = C.c_int32(0)
    rc = load().pt_device_count(C.byref(n))
    return n.value if rc == PT_OK else 0


class Context:
    """pt_ctx owner."""

    def __init__(self, devices=None, ndev: int = 1):
        L = load()
        self._h = _vp()
        if devices is not None:
            arr = (C.c_int32 * len(devices))(*devices)
            check(L.pt_create(arr, len(devices), C.byref(self._h)))
        else:
            check(L.pt_create(None, ndev, C.byref(self._h)))

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h:
            load().pt_destroy(self._h)
            self._h = _vp()

    def set_primary_rays(self, rays=None) -> None:
        """pt_debug_set_primary_rays: `rays` (float64 [n, 6]: origin, direction; the ray of pixel (x, y), sample s at
        (y*width + x)*spp + s) replaces the camera's primary rays in the later frames of this context; None clears."""
        L = load()
        if rays is None:
            check(L.pt_debug_set_primary_rays(self._h, None, 0))
            return
        import numpy as np

        a = np.ascontiguousarray(rays, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != 6:
            raise ValueError("rays must be [n, 6]")
        check(L.pt_debug_set_primary_rays(self._h, a.ctypes.data_as(C.POINTER(C.c_double)), a.shape[0]))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
