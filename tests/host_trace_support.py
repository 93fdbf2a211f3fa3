"""The host layer above the C ABI, call by call, against a recording stand-in for libptcore.so (tests/fake_ptcore.c).

Four drivers, each in a child process with PTCORE_LIB pointing at a fake:
    cli   the `render` CLI twin, driven by flags and environment
    stats hip::Render called from a stand-alone C++ program (tests/host_env_probe.cpp) that prints every engine::Stats field
    host  libpthost.so through pth_render_into (engine::RenderInto -> hip::Render), settings through the environment
    py    hip.render / engine.render_into
A case's outcome -- the fake's log, the error text or exception, the progress() count, for the CLI the exit code and the masked
stderr -- is compared with tests/golden/host_traces.json, recorded from this project's own code before the host layer was rewritten:
    python tests/host_trace_support.py record        # rewrites the golden file from the tree as it stands

REACHED lists every `return` with a text in hip::Render (engine.cpp) and every `raise` in hip.render (hip.py) as they stood when
the golden was recorded, next to the case that reaches it."""
import json
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "host_traces.json")
SIMPLE, FOGGY = "scenes/example_simple.json", "scenes/gpu_showcase.json"  # without / with a fog block

# fake builds: name -> extra compiler flags
FAKES = {"full": [], "base": ["-DPTFAKE_BASE_ABI"], "no_adaptive": ["-DPTFAKE_NO_ADAPTIVE"], "no_halves": ["-DPTFAKE_NO_HALVES"],
         "no_clip": ["-DPTFAKE_NO_CLIP"], "abi3": ["-DPTFAKE_ABI=3"]}

E = "PATHTRACER_GPU_"


def _host(env=None, script="", spp=16, progress=False, lib="full", scene=SIMPLE, **kw):
    return dict(driver="host", env={E + k: v for k, v in (env or {}).items()}, script=script, spp=spp, progress=progress, lib=lib, scene=scene, **kw)


def _cli(*args, env=None, script="", lib="full", scene=SIMPLE, spp=16, raw_env=None):
    e = {E + k: v for k, v in (env or {}).items()}
    e.update(raw_env or {})
    return dict(driver="cli", args=list(args), env=e, script=script, lib=lib, scene=scene, spp=spp)


def _py(api="hip.render", script="", spp=16, progress=False, lib="full", scene=SIMPLE, env=None, raw_env=None, img="ok", arrays=None, **kwargs):
    e = {E + k: v for k, v in (env or {}).items()}
    e.update(raw_env or {})
    return dict(driver="py", api=api, kwargs=kwargs, script=script, spp=spp, progress=progress, lib=lib, scene=scene, env=e, img=img,
                arrays=arrays or {})


def _stats(env=None, script="", spp=16, progress=False, lib="full", scene=SIMPLE):
    return dict(driver="stats", env={E + k: v for k, v in (env or {}).items()}, script=script, spp=spp, progress=progress, lib=lib, scene=scene)


NOISE = {"NOISE": "0.1", "NOISE_STEP": "16"}
CASES = {
    # ---- plain frames
    "host_plain": _host(),                                                     # pt_render
    "host_progress_spp25": _host(spp=25, progress=True),                       # step 25 / 10 = 2, unclipped: 13 steps, final progress()
    "host_spp0": _host(spp=0),
    "host_spp0_progress": _host(spp=0, progress=True),                         # the final-read branch
    "host_size_mismatch": _host(img_w=4),                                      # silently nothing
    "cli_plain": _cli(),
    "py_plain": _py(),
    "py_progress_spp25": _py(spp=25, progress=True),
    "py_spp0": _py(spp=0),
    "py_spp0_progress": _py(spp=0, progress=True),
    "py_size_mismatch": _py(img="small"),
    "py_plain_accum_stats": _py(arrays={"accum": ["float64", [8, 8, 3]], "nseg": ["uint32", [8, 8]], "ndraw": ["uint32", [8, 8]]}),
    "py_engine_plain": _py(api="engine.render_into"),
    # ---- engine::Stats, field by field, through a stand-alone program over engine.hpp (tests/host_env_probe.cpp)
    "stats_plain": _stats(),
    "stats_progress": _stats(spp=25, progress=True),
    "stats_noise": _stats(NOISE, "noise=0.5,0.05", spp=40),
    "stats_adaptive": _stats(dict(NOISE, NOISE_STEP="8", ADAPTIVE="1"), "stall_at=24;noise=0.3", spp=40),
    "stats_filtered": _stats({"ATROUS": "1", "ATROUS_ITERS": "3", "FILTERED_NOISE": "0.1", "NOISE_STEP": "4"}, "halves=0.5/0.6,0.05/0.06", spp=12),
    "stats_atrous": _stats({"ATROUS": "1", "FEATURES": "2"}),
    "stats_temporal_clip": _stats({"TEMPORAL": "1", "TEMPORAL_CLIP": "2.5"}),
    "stats_temporal_no_clip_library": _stats({"TEMPORAL": "1"}, lib="no_clip"),
    "stats_untouched_on_error": _stats({"ATROUS": "1"}, "fail=pt_atrous:1"),
    "stats_base_library": _stats(lib="base"),
    # ---- the CLI's flag syntax: messages, the usage text and exit codes (no frame is rendered)
    "cli_help": _cli("-h"),
    "cli_help_long": _cli("--help"),
    "cli_flag_unknown": _cli("-nope"),
    "cli_flag_unknown_with_value": _cli("--nope=3"),
    "cli_flag_needs_argument": _cli("-noise-step"),
    "cli_flag_bad_bool": _cli("-atrous=maybe"),
    "cli_flag_bool_spellings": _cli("-fog=T", "--adaptive=FALSE", "-atrous=0", "-scene-settings=True"),
    "cli_flag_bad_int": _cli("-min-spp", "4x"),
    "cli_flag_bad_int_overflow": _cli("-width=99999999999999999999"),
    "cli_flag_bad_double": _cli("-noise", "-0.5"),
    "cli_flag_bad_double_nan": _cli("-filtered-noise=nan"),
    "cli_flag_bad_shading": _cli("-shading", "GL"),
    "cli_flag_bad_seed": _cli("-seed", "x"),
    "cli_flag_clamps": _cli("-noise", "0.1", "-noise-step=0", "-min-spp", "-2", "-adaptive", "-features", "2147483648", script="noise=0.5", spp=20),
    "cli_flag_seed_negative_and_sizes": _cli("-seed", "-1", "-width", "0", "-height=-3", "-depth", "4", "-mode", "final", "-spp", "2"),
    "cli_flag_non_flag_ends_parsing": _cli("stop", "-nope"),
    "cli_flag_double_dash_ends_parsing": _cli("--", "-nope"),
    "cli_seed_env": _cli(raw_env={"PATHTRACER_SEED": "77"}),
    "cli_no_gpu_flag": dict(_cli(), no_gpu=True),
    # ---- noise target: cap 40, step 16 -> 16, 16, 8
    "host_noise_stops_second": _host(NOISE, "noise=0.5,0.05", spp=40),
    "host_noise_to_cap": _host(NOISE, "noise=0.5", spp=40),
    "host_noise_to_cap_progress": _host(NOISE, "noise=0.5", spp=40, progress=True),
    "host_noise_step1_not_before_2": _host({"NOISE": "0.1", "NOISE_STEP": "1"}, "noise=0.01", spp=8),
    "host_noise_spp0_progress": _host(NOISE, spp=0, progress=True),
    "cli_noise": _cli("-noise", "0.1", "-noise-step", "16", script="noise=0.5,0.05", spp=40),
    "cli_noise_env": _cli(env=NOISE, script="noise=0.5", spp=40),
    "py_noise_stops_second": _py(noise=0.1, noise_step=16, script="noise=0.5,0.05", spp=40),
    "py_noise_to_cap_progress": _py(noise=0.1, noise_step=16, script="noise=0.5", spp=40, progress=True),
    "py_noise_step1_not_before_2": _py(noise=0.1, noise_step=1, script="noise=0.01", spp=8),
    "py_noise_step0": _py(noise=0.1, noise_step=0, script="noise=0.5", spp=3),  # max(1, ...)
    "py_engine_noise_env": _py(api="engine.render_into", env=NOISE, script="noise=0.5,0.05", spp=40),
    "py_moments": _py(arrays={"moments": ["float64", [8, 8, 3]]}),
    # ---- adaptive: ends on the step that adds nothing
    "host_adaptive_stall": _host(dict(NOISE, NOISE_STEP="8", ADAPTIVE="1", ADAPTIVE_MIN_SPP="4"), "stall_at=24", spp=40),
    "host_adaptive_stall_progress": _host(dict(NOISE, NOISE_STEP="8", ADAPTIVE="on"), "stall_at=24", spp=40, progress=True),
    "host_adaptive_without_noise": _host({"ADAPTIVE": "1"}),                    # nothing to adapt to: a plain frame
    "cli_adaptive": _cli("-noise", "0.1", "-noise-step", "8", "-adaptive", "-min-spp", "4", script="stall_at=24", spp=40),
    "cli_adaptive_without_noise": _cli("-adaptive"),
    "py_adaptive_no_progress": _py(noise=0.1, adaptive=True, min_spp=4, arrays={"counts": ["uint32", [8, 8]]}, spp=40),  # pt_render steps
    "py_adaptive_stall_progress": _py(noise=0.1, noise_step=7, adaptive=True, script="stall_at=21", spp=40, progress=True),  # step unclipped
    "py_adaptive_step0_progress": _py(noise=0.1, noise_step=0, adaptive=True, spp=3, progress=True),
    "py_adaptive_spp0_progress": _py(noise=0.1, adaptive=True, spp=0, progress=True),
    "py_engine_adaptive_env": _py(api="engine.render_into", env=dict(NOISE, ADAPTIVE="1"), spp=40),
    # ---- filtered noise: first pt_atrous_halves at done == 4
    "host_filtered_step1": _host({"ATROUS": "1", "FILTERED_NOISE": "0.1", "NOISE_STEP": "1"}, "halves=0.5/0.6,0.3/0.4,0.05/0.06", spp=12),
    "host_filtered_to_cap_progress": _host({"ATROUS": "1", "FILTERED_NOISE": "0.1", "NOISE_STEP": "16"}, "halves=0.5/0.6", spp=40, progress=True),
    "host_filtered_without_filter": _host({"FILTERED_NOISE": "0.1"}),          # ignored without the filter
    "cli_filtered": _cli("-atrous", "-filtered-noise", "0.1", "-noise-step", "1", script="halves=0.5/0.6,0.05/0.06", spp=12),
    "cli_filtered_without_atrous": _cli("-filtered-noise", "0.1"),
    "py_filtered_step1": _py(atrous={}, filtered_noise=0.1, noise_step=1, script="halves=0.5/0.6,0.3/0.4,0.05/0.06", spp=12),
    "py_filtered_to_cap_progress": _py(atrous={}, filtered_noise=0.1, script="halves=0.5/0.6", spp=40, progress=True),
    "py_filtered_spp0": _py(atrous={}, filtered_noise=0.1, spp=0),
    "py_halves": _py(halves=True),
    "py_engine_filtered_env": _py(api="engine.render_into", env={"ATROUS": "1", "FILTERED_NOISE": "0.1", "NOISE_STEP": "4"}, script="halves=0.05/0.06", spp=12),
    # ---- the filter and temporal finishes
    "cli_atrous_iters_flag": _cli("-atrous", "-atrous-iters", "3"),
    "cli_atrous_iters_env": _cli(env={"ATROUS": "yes", "ATROUS_ITERS": "2"}),
    "cli_atrous_iters_default": _cli("-atrous", env={"ATROUS_ITERS": "9"}),
    "cli_atrous_iters_flag_out_of_range": _cli("-atrous", "-atrous-iters", "7"),
    "host_atrous_progress": _host({"ATROUS": "1"}, progress=True),
    "host_temporal": _host({"TEMPORAL": "1"}),
    "host_temporal_clip": _host({"TEMPORAL": "1", "TEMPORAL_CLIP": "2.5", "ATROUS_ITERS": "4"}),
    "host_clip_without_temporal": _host({"TEMPORAL_CLIP": "2.5"}),
    "cli_temporal_clip_env": _cli(env={"TEMPORAL": "true", "TEMPORAL_CLIP": "2.5"}),
    "py_atrous": _py(atrous={"iterations": 3, "sigma_l": 2.0}),
    "py_atrous_spp0": _py(atrous={}, spp=0),
    "py_temporal": _py(temporal={}),
    "py_temporal_filter_clip": _py(temporal={"alpha": 0.5, "max_len": 8}, atrous={"iterations": 2}, temporal_clip=2.5),
    "py_engine_temporal_env": _py(api="engine.render_into", env={"TEMPORAL": "1", "TEMPORAL_CLIP": "2.5", "ATROUS_ITERS": "4", "FEATURES": "6"}),
    "py_engine_atrous_env": _py(api="engine.render_into", env={"ATROUS": "1", "ATROUS_ITERS": "2"}),
    # ---- features
    "cli_features_flag": _cli("-features", "3"),
    "cli_features_env": _cli(env={"FEATURES": "2"}),
    "cli_features_flag_negative": _cli("-atrous", "-features", "-5", env={"FEATURES": "2"}),
    "cli_features_unsaid_filter": _cli("-atrous"),
    "cli_features_unsaid_gl": _cli("-atrous", "-shading", "gl"),
    "cli_features_unsaid_bvh": _cli("-atrous", raw_env={"PTCORE_SCAN": "bvh"}),
    "host_features_unsaid_temporal_gl": _host({"TEMPORAL": "1", "SHADING": "gl"}),
    "py_features": _py(features=3),
    "py_features_unsaid_filter": _py(atrous={}),
    "py_features_unsaid_gl": _py(atrous={}, shading="gl"),
    "py_features_unsaid_bvh": _py(atrous={}, raw_env={"PTCORE_SCAN": "verify_bvh"}),
    "py_features_from_config": _py(atrous={"features": 0}, temporal={}),
    # ---- scene settings
    "cli_fog_present": _cli("-fog", scene=FOGGY),
    "cli_fog_absent": _cli("-fog"),
    "cli_fog_false_over_env": _cli("-fog=false", env={"FOG": "1"}, scene=FOGGY),
    "cli_fog_env": _cli(env={"FOG": "TRUE"}, scene=FOGGY),
    "host_fog_env": _host({"FOG": "1"}, scene=FOGGY),
    "cli_gl": _cli("-shading", "gl"),
    "cli_gl_env_upper": _cli(env={"SHADING": "GL"}),
    "cli_gl_env_padded": _cli(env={"SHADING": " gl "}),
    "cli_cpu_over_env": _cli("-shading=cpu", env={"SHADING": "gl"}),
    "cli_devices": _cli("-devices", "2", "-seed", "9"),
    "py_fog_present": _py(fog=True, scene=FOGGY),
    "py_fog_absent": _py(fog=True),
    "py_gl": _py(shading="gl"),
    "py_engine_gl_env_padded": _py(api="engine.render_into", env={"SHADING": " GL "}),
    # ---- refusals
    "host_filtered_with_noise": _host(dict(NOISE, ATROUS="1", FILTERED_NOISE="0.1")),
    "host_filtered_with_gl": _host({"ATROUS": "1", "FILTERED_NOISE": "0.1", "SHADING": "gl"}),
    "host_filtered_with_noise_and_gl": _host(dict(NOISE, ATROUS="1", FILTERED_NOISE="0.1", SHADING="gl")),
    "cli_filtered_with_noise": _cli("-atrous", "-filtered-noise", "0.1", "-noise", "0.2"),
    "py_raise_clip_without_temporal": _py(temporal_clip=2.5, filtered_noise=0.1),                       # the first of the two
    "py_raise_filtered_without_atrous": _py(filtered_noise=0.1, noise=0.1, shading="gl"),
    "py_raise_filtered_with_noise": _py(filtered_noise=0.1, atrous={}, noise=0.1, shading="gl"),
    "py_raise_filtered_with_adaptive": _py(filtered_noise=0.1, atrous={}, adaptive=True),
    "py_raise_filtered_with_gl": _py(filtered_noise=0.1, atrous={}, shading="gl", img="float"),
    "py_raise_img_dtype": _py(img="float", adaptive=True),
    "py_raise_img_rows": _py(img="strided", adaptive=True),
    "py_raise_shading_name": _py(shading="vulkan", adaptive=True),
    "py_raise_adaptive_without_noise": _py(adaptive=True, arrays={"counts": ["uint8", [8, 8]]}),
    "py_raise_counts_without_adaptive": _py(arrays={"counts": ["uint32", [8, 8]], "moments": ["float32", [8, 8, 3]]}),
    "py_raise_counts_dtype": _py(noise=0.1, adaptive=True, arrays={"counts": ["uint8", [8, 8]]}),
    "py_raise_moments_shape": _py(arrays={"moments": ["float64", [8, 8]], "accum": ["float32", [8, 8, 3]]}),
    "py_raise_accum_dtype": _py(arrays={"accum": ["float32", [8, 8, 3]], "nseg": ["uint8", [8, 8]]}),
    "py_raise_nseg_dtype": _py(arrays={"nseg": ["uint8", [8, 8]]}, progress=True),
    "py_raise_pixel_stats_with_progress": _py(arrays={"nseg": ["uint32", [8, 8]]}, progress=True),
    "py_raise_pixel_stats_with_noise": _py(arrays={"ndraw": ["uint32", [8, 8]]}, noise=0.1),
    # ---- "libptcore.so lacks ..." and capi.has()
    "host_abi_mismatch": _host(lib="abi3"),
    "host_lacks_gl": _host({"SHADING": "gl"}, lib="base"),
    "host_lacks_noise": _host(dict(NOISE, ADAPTIVE="1"), lib="base"),
    "host_lacks_temporal": _host({"TEMPORAL": "1", "ATROUS": "1"}, lib="base"),
    "host_lacks_clip": _host({"TEMPORAL": "1", "TEMPORAL_CLIP": "2.5"}, lib="no_clip"),
    "host_no_clip_without_clip": _host({"TEMPORAL": "1"}, lib="no_clip"),
    "host_lacks_atrous": _host({"ATROUS": "1", "FEATURES": "2"}, lib="base"),
    "host_lacks_halves": _host({"ATROUS": "1", "FILTERED_NOISE": "0.1"}, lib="no_halves"),
    "host_lacks_features": _host({"FEATURES": "2"}, lib="base"),
    "host_lacks_adaptive": _host(dict(NOISE, ADAPTIVE="1"), lib="no_adaptive"),
    "host_base_plain": _host(lib="base"),                                      # no optional setter is called
    "host_base_progress": _host(lib="base", progress=True, spp=5),
    "cli_lacks_gl": _cli("-shading", "gl", lib="base"),
    "py_base_plain": _py(lib="base"),
    "py_lacks_gl": _py(shading="gl", lib="base"),
    "py_lacks_moments": _py(noise=0.1, lib="base"),
    "py_lacks_adaptive": _py(noise=0.1, adaptive=True, lib="no_adaptive"),
    "py_lacks_features": _py(features=2, lib="base"),
    "py_lacks_halves": _py(halves=True, lib="no_halves"),
    "py_lacks_atrous_halves": _py(atrous={}, filtered_noise=0.1, lib="no_halves"),
    "py_lacks_clip": _py(temporal={}, temporal_clip=1.0, lib="no_clip"),
    # ---- injected failures: the error text is the first failure's; pt_end still runs after a mid-loop failure, not after pt_begin's
    "host_fail_create": _host(script="fail=pt_create:1"),
    "host_fail_render": _host(script="fail=pt_render:1"),
    "host_fail_begin_progress": _host(script="fail=pt_begin:1", progress=True),
    "host_fail_begin_noise": _host(NOISE, "fail=pt_begin:1"),
    "host_fail_begin_filtered": _host({"ATROUS": "1", "FILTERED_NOISE": "0.1"}, "fail=pt_begin:1"),
    "host_fail_step2_progress": _host(script="fail=pt_step:2", spp=25, progress=True),
    "host_fail_step2_noise": _host(NOISE, "fail=pt_step:2;noise=0.5", spp=40),
    "host_fail_step2_filtered": _host({"ATROUS": "1", "FILTERED_NOISE": "0.1", "NOISE_STEP": "4"}, "fail=pt_step:2", spp=12),
    "host_fail_read_progress": _host(script="fail=pt_read:1", progress=True),
    "host_fail_read_noise_progress": _host(NOISE, "fail=pt_read:1", progress=True),
    "host_fail_read_filtered_progress": _host({"ATROUS": "1", "FILTERED_NOISE": "0.1"}, "fail=pt_read:1", progress=True),
    "host_fail_read_final_noise": _host(NOISE, "fail=pt_read:1;noise=0.01"),
    "host_fail_read_final_filtered": _host({"ATROUS": "1", "FILTERED_NOISE": "0.1"}, "fail=pt_read:1;halves=0.01/0.01"),
    "host_fail_read_final_spp0_progress": _host(script="fail=pt_read:1", spp=0, progress=True),
    "host_fail_noise_estimate": _host(NOISE, "fail=pt_noise_estimate:1", spp=40),
    "host_fail_atrous_halves": _host({"ATROUS": "1", "FILTERED_NOISE": "0.1"}, "fail=pt_atrous_halves:1"),
    "host_fail_adaptive_state": _host(dict(NOISE, ADAPTIVE="1"), "fail=pt_adaptive_state:1"),
    "host_fail_end_progress": _host(script="fail=pt_end:1", progress=True, spp=5),
    "host_fail_end_noise": _host(NOISE, "fail=pt_end:1;noise=0.01"),
    "host_fail_end_filtered": _host({"ATROUS": "1", "FILTERED_NOISE": "0.1"}, "fail=pt_end:1;halves=0.01/0.01"),
    "host_fail_step1_progress": _host(script="fail=pt_step:1", progress=True),
    "host_fail_atrous": _host({"ATROUS": "1"}, "fail=pt_atrous:1"),
    "host_fail_temporal": _host({"TEMPORAL": "1"}, "fail=pt_temporal:1"),
    "host_fail_temporal_set_clip": _host({"TEMPORAL": "1", "TEMPORAL_CLIP": "2.5"}, "fail=pt_temporal_set_clip:1"),
    "host_fail_temporal_clip_stats": _host({"TEMPORAL": "1", "TEMPORAL_CLIP": "2.5"}, "fail=pt_temporal_clip_stats:1"),
    "host_fail_set_fog": _host(script="fail=pt_set_fog:1"),
    "host_fail_set_shading": _host(script="fail=pt_set_shading:1"),
    "host_fail_set_halves": _host(script="fail=pt_set_halves:1"),
    "host_fail_set_features": _host(script="fail=pt_set_features:1"),
    "host_fail_set_moments": _host(script="fail=pt_set_moments:1"),
    "host_fail_set_adaptive": _host(script="fail=pt_set_adaptive:1"),
    "cli_fail_render": _cli(script="fail=pt_render:1"),
    "py_fail_render": _py(script="fail=pt_render:1"),
    "py_fail_begin": _py(script="fail=pt_begin:1", progress=True),
    "py_fail_step2": _py(script="fail=pt_step:2", spp=25, progress=True),
    "py_fail_step2_noise": _py(noise=0.1, script="fail=pt_step:2;noise=0.5", spp=40),
    "py_fail_read": _py(script="fail=pt_read:1", progress=True),
    "py_fail_noise_estimate": _py(noise=0.1, script="fail=pt_noise_estimate:1", spp=40),
    "py_fail_atrous_halves": _py(atrous={}, filtered_noise=0.1, script="fail=pt_atrous_halves:1"),
    "py_fail_end": _py(script="fail=pt_end:1", progress=True, spp=5),
    "py_fail_atrous": _py(atrous={}, script="fail=pt_atrous:1"),
    "py_fail_temporal": _py(temporal={}, script="fail=pt_temporal:1"),
    "py_fail_set_fog": _py(script="fail=pt_set_fog:1"),
    "py_fail_set_shading": _py(script="fail=pt_set_shading:1"),
    "py_fail_set_clip": _py(temporal={}, temporal_clip=2.5, script="fail=pt_temporal_set_clip:1"),
    "py_fail_set_adaptive": _py(script="fail=pt_set_adaptive:1"),
    "py_fail_set_moments": _py(script="fail=pt_set_moments:1"),
    "py_fail_set_halves": _py(script="fail=pt_set_halves:1"),
    "py_fail_set_features": _py(script="fail=pt_set_features:1"),
}

# every `return` with a text in hip::Render and every `raise` in hip.render, as recorded -> a case that reaches it
REACHED = {
    "engine.cpp": {
        "return g_core.error": "host_abi_mismatch",
        "pt_create: ": "host_fail_create",
        "pt_set_fog: ": "host_fail_set_fog",
        "GL shading: libptcore.so lacks pt_set_shading": "host_lacks_gl",
        "pt_set_shading: ": "host_fail_set_shading",
        "noise target: libptcore.so lacks pt_set_moments / pt_noise_estimate": "host_lacks_noise",
        "temporal accumulation: libptcore.so lacks pt_temporal": "host_lacks_temporal",
        "temporal clip: libptcore.so lacks pt_temporal_set_clip": "host_lacks_clip",
        "a-trous filter: libptcore.so lacks pt_atrous / pt_set_moments": "host_lacks_atrous",
        "filtered noise target: excludes a frame noise target": "host_filtered_with_noise",
        "filtered noise target: not available with GL shading": "host_filtered_with_gl",
        "filtered noise target: libptcore.so lacks pt_set_halves / pt_atrous_halves": "host_lacks_halves",
        "pt_set_halves: ": "host_fail_set_halves",
        "features: libptcore.so lacks pt_set_features": "host_lacks_features",
        "pt_set_features: ": "host_fail_set_features",
        "pt_set_moments: ": "host_fail_set_moments",
        "adaptive sampling: libptcore.so lacks pt_set_adaptive / pt_adaptive_state": "host_lacks_adaptive",
        "pt_set_adaptive: ": "host_fail_set_adaptive",
        "pt_begin: (filtered-noise loop)": "host_fail_begin_filtered",
        "pt_begin: (noise loop)": "host_fail_begin_noise",
        "pt_begin: (progress loop)": "host_fail_begin_progress",
        "return err: pt_step (each loop)": "host_fail_step2_filtered host_fail_step2_noise host_fail_step2_progress",
        "return err: pt_read in a loop": "host_fail_read_filtered_progress host_fail_read_noise_progress host_fail_read_progress",
        "return err: pt_read (the final one)": "host_fail_read_final_filtered host_fail_read_final_noise host_fail_read_final_spp0_progress",
        "return err: pt_atrous_halves": "host_fail_atrous_halves",
        "return err: pt_noise_estimate": "host_fail_noise_estimate",
        "return err: pt_adaptive_state": "host_fail_adaptive_state",
        "return err: pt_end (each loop)": "host_fail_end_filtered host_fail_end_noise host_fail_end_progress",
        "return err: pt_render": "host_fail_render",
        "return err: pt_temporal_set_clip": "host_fail_temporal_set_clip",
        "return err: pt_temporal": "host_fail_temporal",
        "return err: pt_temporal_clip_stats": "host_fail_temporal_clip_stats",
        "return err: pt_atrous": "host_fail_atrous",
    },
    "hip.py": {
        "temporal_clip needs the accumulation it clips": "py_raise_clip_without_temporal",
        "filtered_noise needs the filter whose output it measures": "py_raise_filtered_without_atrous",
        "filtered_noise excludes noise= and adaptive=True": "py_raise_filtered_with_noise py_raise_filtered_with_adaptive",
        "filtered_noise is not available with GL shading": "py_raise_filtered_with_gl",
        "img must be uint8 [H, W, 4]": "py_raise_img_dtype",
        "img rows must be contiguous RGBA": "py_raise_img_rows",
        "adaptive needs the block noise target": "py_raise_adaptive_without_noise",
        "counts needs adaptive=True and a contiguous uint32": "py_raise_counts_without_adaptive py_raise_counts_dtype",
        "moments must be contiguous float64": "py_raise_moments_shape",
        "accum must be contiguous float64": "py_raise_accum_dtype",
        "nseg/ndraw must be contiguous uint32": "py_raise_nseg_dtype",
        "per-pixel stats are only available without a progress callback": "py_raise_pixel_stats_with_progress py_raise_pixel_stats_with_noise",
    },
}


def build_probe(outdir, flags=(), name="host_env_probe"):
    """tests/host_env_probe.cpp with the host layer's sources, stand-alone."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or "g++"
    hdir = os.path.join(ROOT, "path_trace_golang_amd", "csrc", "host")
    exe = os.path.join(outdir, name)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", *flags, "-I" + os.path.join(ROOT, "path_trace_golang_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host_env_probe.cpp"), *[os.path.join(hdir, f) for f in ("engine.cpp", "scene.cpp", "json.cpp", "png.cpp")],
                    "-o", exe, "-ldl", "-lpthread"], check=True)
    return exe


def build_fakes(outdir, probe=True):
    """gcc -shared of tests/fake_ptcore.c in each variant, and the stats driver's program; returns name -> path."""
    cc = os.environ.get("CC") or shutil.which("gcc") or "cc"
    libs = {}
    for name, flags in FAKES.items():
        libs[name] = os.path.join(outdir, "libptfake_%s.so" % name)
        subprocess.run([cc, "-std=c11", "-O1", "-g", "-fPIC", "-shared", "-Wall", "-Wextra", "-Wno-unused-function", "-Wno-unused-variable", *flags,
                        os.path.join(ROOT, "tests", "fake_ptcore.c"), "-o", libs[name]], check=True)
    if probe:
        libs["probe"] = build_probe(outdir)
    return libs


_STAMP = re.compile(r"^\d{4}/\d\d/\d\d \d\d:\d\d:\d\d ", re.M)
_RATE = re.compile(r"in \S+ s: \S+ M segments/s, \S+ M samples/s")


def mask(stderr):
    return _RATE.sub("in # s: # M segments/s, # M samples/s", _STAMP.sub("<stamp> ", stderr))


def run_case(name, libs, workdir):
    """One case in a child process; returns the outcome that the golden file records."""
    case = CASES[name]
    log = os.path.join(workdir, name + ".log")
    if os.path.exists(log):
        os.remove(log)
    env = {k: v for k, v in os.environ.items() if not k.startswith(("PATHTRACER_", "PTCORE_", "PTFAKE_"))}
    env.update(case["env"], PTCORE_LIB=libs[case["lib"]], PTFAKE_LOG=log, PTFAKE_SCRIPT=case["script"])
    if case["driver"] == "cli":
        exe = os.path.join(ROOT, "path_trace_golang_amd", "render")
        cmd = [exe, "-headless", *([] if case.get("no_gpu") else ["-gpu"]), "-scene", case["scene"], "-width", "8", "-height", "8", "-depth", "3", "-spp", str(case["spp"]),
               "-out", os.path.join(workdir, name + ".png"), *case["args"]]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, env=env, timeout=120)
        out = {"exit": r.returncode, "stderr": mask(r.stderr.replace(workdir, "<tmp>"))}
    elif case["driver"] == "stats":
        r = subprocess.run([libs["probe"], "stats", case["scene"], str(case["spp"]), str(int(case["progress"]))], capture_output=True, text=True,
                           cwd=ROOT, env=env, timeout=120)
        out = {"exit": r.returncode, "stdout": r.stdout.split("\n")[:-1], "stderr": r.stderr}
    else:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", json.dumps(case)], capture_output=True, text=True, cwd=ROOT,
                           env=env, timeout=120)
        assert r.returncode == 0, (name, r.stdout, r.stderr)
        out = json.loads(r.stdout.strip().split("\n")[-1])
    out["trace"] = open(log).read().split("\n")[:-1] if os.path.exists(log) else []
    return out


# ---------------------------------------------------------------- the child process
def _child_host(case):
    import ctypes as C

    import numpy as np

    L = C.CDLL(os.environ.get("PTHOST_LIB") or os.path.join(ROOT, "path_trace_golang_amd", "libpthost.so"))  # PTHOST_LIB: a sanitizer build
    L.pth_last_error.restype = C.c_char_p
    L.pth_scene_load.restype = C.c_void_p
    L.pth_scene_load.argtypes = [C.c_char_p]
    L.pth_scene_free.argtypes = [C.c_void_p]
    L.pth_render_into.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_void_p, C.c_int32, C.c_int32,
                                  C.c_int32, C.c_void_p]
    L.pth_set_backend(1)
    h = L.pth_scene_load(os.path.join(ROOT, case["scene"]).encode())
    assert h, L.pth_last_error()
    iw = case.get("img_w", 8)
    buf = np.full((8, iw, 4), 7, np.uint8)
    calls = []
    cb = C.CFUNCTYPE(None)(lambda: calls.append(1))
    rc = L.pth_render_into(h, 8, 8, case["spp"], 3, 5, buf.ctypes.data_as(C.c_void_p), iw, 8, iw * 4,
                           C.cast(cb, C.c_void_p) if case["progress"] else None)
    out = {"rc": rc, "error": L.pth_last_error().decode() if rc else "", "progress_calls": len(calls), "pixel0": buf[0, 0].tolist()}
    L.pth_scene_free(h)
    L.pth_shutdown()
    return out


def _child_py(case):
    import numpy as np

    sys.path.insert(0, ROOT)
    from path_trace_golang_amd import engine, hip, scene

    sc = scene.load(os.path.join(ROOT, case["scene"]))
    kw = dict(case["kwargs"])
    if "atrous" in kw:
        kw["atrous"] = hip.AtrousConfig(**kw["atrous"])
    if "temporal" in kw:
        kw["temporal"] = hip.TemporalConfig(**kw["temporal"])
    for k, (dtype, shape) in case["arrays"].items():
        kw[k] = np.zeros(shape, dtype)
    img = {"ok": lambda: np.full((8, 8, 4), 7, np.uint8), "small": lambda: np.full((4, 4, 4), 7, np.uint8),
           "float": lambda: np.zeros((8, 8, 4), np.float32), "strided": lambda: np.zeros((8, 8, 8), np.uint8)[:, :, ::2]}[case["img"]]()
    calls = []
    if case["progress"]:
        kw["progress"] = lambda: calls.append(1)
    out = {"exception": None}
    try:
        if case["api"] == "engine.render_into":
            out["result"] = engine.render_into(sc, engine.RenderConfig(8, 8, case["spp"], 3, 5), img, **kw)
        else:
            out["result"] = hip.render(sc, hip.RenderConfig(8, 8, case["spp"], 3, 5), img, **kw)
    except Exception as e:  # the text and the type are what the golden records
        out["exception"] = [type(e).__name__, str(e)]
    out.update(progress_calls=len(calls), pixel0=np.asarray(img[0, 0], np.float64).tolist())
    return out


def record():
    import tempfile

    from path_trace_golang_amd import build

    build.build_host()
    with tempfile.TemporaryDirectory() as tmp:
        libs = build_fakes(tmp)
        got = {name: run_case(name, libs, tmp) for name in sorted(CASES)}
    with open(GOLDEN, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d cases into %s" % (len(got), GOLDEN))


if __name__ == "__main__":
    if sys.argv[1] == "child":
        c = json.loads(sys.argv[2])
        print(json.dumps(_child_host(c) if c["driver"] == "host" else _child_py(c), sort_keys=True))
    elif sys.argv[1] == "record":
        sys.path.insert(0, ROOT)
        record()
