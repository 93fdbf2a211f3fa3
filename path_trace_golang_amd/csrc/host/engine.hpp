// engine.hpp -- C++ mirror of the reference's internal/engine public surface for the render path
// (/root/reference/internal/engine/renderer.go:17-41, backend.go:5-28, util.go:13-55) and of the
// backend plug-in shape gpu.Render (/root/reference/internal/engine/gpu/gpu.go:2534).
#pragma once

#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "../../../include/ptcore.h"
#include "scene.hpp"

namespace pthost {
namespace engine {

// image.RGBA: Pix holds Height rows of Stride bytes, 4 bytes per pixel, row 0 on top.
struct RGBA {
    int Width = 0, Height = 0, Stride = 0;
    std::vector<uint8_t> Pix;
};
RGBA NewRGBA(int width, int height);  // image.NewRGBA(image.Rect(0, 0, w, h))

struct RenderConfig {  // renderer.go:17-22 (+ the stream seed; the reference seeds from the clock)
    int Width = 0, Height = 0, SamplesPerPx = 0, MaxDepth = 0;
    uint64_t Seed = 1;
};

enum Backend { BackendCPU = 0, BackendGPU = 1 };  // backend.go:7-10
void SetBackend(int b);                           // backend.go:16-23: unknown values select the CPU backend
Backend GetBackend();

struct Stats {
    uint64_t samples = 0, segments = 0, exit_scans = 0, draws = 0;
    double seconds = 0, trace_ms = 0, resolve_ms = 0, device_ms = 0;
    int num_devices = 0, spp_chunk = 0;
    int spp_done = 0;   // samples per pixel actually rendered (below SamplesPerPx when a noise target stopped the frame)
    double noise = 0;   // frame noise at the stop (pt_noise_estimate); 0 when no noise target was set
    bool adaptive = false;  // the frame was adaptive (SetAdaptive): spp_done is the largest count, samples the sum of the counts
    uint64_t blocks = 0, active_blocks = 0;  // pt_adaptive_state of the frame: 8x8 blocks inside it, those still above the target
    int spp_min = 0;
    bool atrous = false;   // the image is the a-trous filtered one (SetAtrous); noise_before / noise_after are pt_atrous_stats' figures
    int features = 0;      // feature samples per pixel the frame collected (pt_set_features)
    double atrous_ms = 0, noise_before = 0, noise_after = 0;
    bool to_filtered_noise = false;  // the stop rule was the measured noise of the filtered frame (SetFilteredNoise); spp_done is the count
    double filtered_noise = 0, noise_model = 0;  // pt_halves_stats' noise and noise_model at the last check (0: no check ran)
    bool to_filtered_adaptive = false;  // the blocks stopped by the filtered frame's pooled noise (SetFilteredAdaptive); the adaptive fields hold
    int pool = 0, block_checks = 0;     // ... the pool radius in blocks and the checks that decided (pt_read_block_figures)
    bool temporal = false;  // the image is pt_temporal's (SetTemporal): the frame blended into the reprojected history, then filtered
    uint64_t reprojected = 0, disoccluded = 0;  // pt_temporal_stats of the frame
    double temporal_ms = 0, mean_len = 0, noise_blended = 0;
    double temporal_clip = 0;  // gamma of the history clip the frame ran with (SetTemporalClip; 0 = off)
    uint64_t clipped = 0;      // pt_temporal_clip_stats of the frame: reprojected pixels whose history the clip changed
    // displaced reprojection (SetTemporalMotion): pt_temporal_motion_stats of the frame (motion_objects 0: it ran without a table),
    // and whether the history was reset before it because more than positions and the camera had changed
    int motion_objects = 0;
    uint64_t moved = 0, moved_reprojected = 0;
    bool motion_reset = false;
};

namespace hip {
// The MI355X backend: same shape as gpu.Render(sc, cfg, img, progress) error.
// Returns "" on success, the error text otherwise.  Never renders on the CPU.
std::string Render(const scene::Scene &sc, const RenderConfig &cfg, RGBA &img, const std::function<void()> &progress,
                   Stats *stats = nullptr);
void SetDevices(const std::vector<int> &ordinals);  // HIP ordinals used by Render (default: device 0)
// Whether Render draws the scene's fog block (pt_set_fog; off by default, like the CPU engine, which ignores fog).  The
// initial value is PATHTRACER_GPU_FOG (FogFromEnv).
void SetFog(bool on);
bool GetFog();
bool FogFromEnv();  // PATHTRACER_GPU_FOG = 1 / true / on / yes
// The shading model Render uses (pt_set_shading): PT_SHADING_CPU (the CPU engine, default) or PT_SHADING_GL (the OpenGL
// backend's estimator).  The initial value is PATHTRACER_GPU_SHADING (ShadingFromEnv).
void SetShading(int model);
int GetShading();
int ShadingFromEnv();  // PATHTRACER_GPU_SHADING = gl (any case) -> PT_SHADING_GL, else PT_SHADING_CPU
// The stop rule of Render: target > 0 renders until the frame noise (pt_noise_estimate) is at or below target,
// checking every `step` samples per pixel, with cfg.SamplesPerPx as the cap; target <= 0 (the default) renders SamplesPerPx
// samples.  The initial value is PATHTRACER_GPU_NOISE / PATHTRACER_GPU_NOISE_STEP (NoiseFromEnv).
void SetNoiseTarget(double target, int step = 16);
double GetNoiseTarget();
int GetNoiseStep();
void NoiseFromEnv(double &target, int &step);  // PATHTRACER_GPU_NOISE = float > 0 (else 0: off), _STEP = int >= 1 (else 16)
// Adaptive sampling: with a noise target set, that target is the one of every 8x8 block (pt_set_adaptive) instead of
// the frame's: blocks stop one by one, the frame ends when none is active or at the cap.  min_spp = samples every block gets before
// the first check.  The initial value is PATHTRACER_GPU_ADAPTIVE / PATHTRACER_GPU_ADAPTIVE_MIN_SPP (AdaptiveFromEnv).
void SetAdaptive(bool on, int min_spp = 0);
bool GetAdaptive();
int GetAdaptiveMinSpp();
void AdaptiveFromEnv(bool &on, int &min_spp);  // PATHTRACER_GPU_ADAPTIVE = 1 / true / on / yes, _MIN_SPP = int >= 0 (else 0)
// The a-trous filter: Render turns moments on and, after the frame, replaces the image by pt_atrous's (the default
// sigmas, `iterations` 0..6).  The initial value is PATHTRACER_GPU_ATROUS / PATHTRACER_GPU_ATROUS_ITERS (AtrousFromEnv).
void SetAtrous(bool on, int iterations = 5);
bool GetAtrous();
int GetAtrousIterations();
void AtrousFromEnv(bool &on, int &iterations);  // PATHTRACER_GPU_ATROUS = 1 / true / on / yes, _ITERS = int 0..6 (else 5)
// First-hit feature planes (pt_set_features): k feature samples per pixel; k < 0 = not said (PATHTRACER_GPU_FEATURES, and without
// it 4 under the filter where the scene allows features -- not with GL shading or on the BVH path -- else 0).
// A noise target on the filtered frame: with the filter on and target > 0, the frame collects the half-buffer sums
// (pt_set_halves), samples are added GetNoiseStep() at a time, after every step with at least 4 samples done pt_atrous_halves runs
// with the filter's configuration, and the frame stops at the first check whose measured noise is at or below target, SamplesPerPx
// being the cap.  The image is pt_atrous on the full sums.  Ignored without the filter; a frame noise target (SetNoiseTarget) or
// GL shading beside it is an error.  The initial value is PATHTRACER_GPU_FILTERED_NOISE (FilteredNoiseFromEnv).
void SetFilteredNoise(double target);
double GetFilteredNoise();
double FilteredNoiseFromEnv();  // PATHTRACER_GPU_FILTERED_NOISE = float > 0, else 0: off
// Adaptive sampling by the filtered frame's pooled noise: with the filter on and target > 0 the frame is an adaptive one
// (pt_set_adaptive with this target, GetNoiseStep() and GetAdaptiveMinSpp()) whose 8x8 blocks stop once the noise measured in the
// filtered frame over the blocks within `pool` blocks (0..4, anything else counts as 1) of them is at or below target
// (pt_set_adaptive_filtered with the filter's configuration).  The image is pt_atrous on the full sums with every pixel's own count.
// Ignored without the filter; a frame noise target, the filtered noise target or GL shading beside it is an error.  The initial value
// is PATHTRACER_GPU_FILTERED_ADAPTIVE / PATHTRACER_GPU_POOL (FilteredAdaptiveFromEnv).
void SetFilteredAdaptive(double target, int pool = 1);
double GetFilteredAdaptive();
int GetPool();
void FilteredAdaptiveFromEnv(double &target, int &pool);  // PATHTRACER_GPU_FILTERED_ADAPTIVE = float > 0 (else 0: off), _POOL = int 0..4 (else 1)
// Temporal accumulation, for a caller that renders frame after frame while the camera moves: the process-wide context
// keeps a history, and after the frame Render calls pt_temporal -- the frame blended into the reprojected history, then filtered
// -- in place of pt_atrous.  On turns on moments, the filter and 4 feature samples per pixel (unless SetFeatures /
// PATHTRACER_GPU_FEATURES name another number).  Change cfg.Seed from frame to frame (the blended variance assumes independent
// frames) and call ResetTemporal after a scene edit or a cut.  The initial value is PATHTRACER_GPU_TEMPORAL (TemporalFromEnv).
void SetTemporal(bool on);
bool Temporal();
bool TemporalFromEnv();  // PATHTRACER_GPU_TEMPORAL = 1 / true / on / yes
void ResetTemporal();    // pt_temporal_reset on the process-wide context
// The history clip of the accumulation (pt_temporal_set_clip): before the blend the reprojected history is clamped to
// the frame's mean +- gamma * sqrt(var_frame + var_history).  0 = off (the default); 2.5 is the recommended value; a NaN, a negative
// or an infinite gamma is taken as 0.  Read by Render when the accumulation is on.  The initial value is
// PATHTRACER_GPU_TEMPORAL_CLIP (TemporalClipFromEnv).
void SetTemporalClip(double gamma);
double TemporalClipFromEnv();  // PATHTRACER_GPU_TEMPORAL_CLIP = finite float >= 0, else 0: off
// pt_temporal_clip_stats of the process-wide context: the gamma, the clipped and the reprojected pixels of the last accumulated
// frame.  False while the history is empty (or the library lacks the entry point).
bool TemporalClipStats(double &gamma, uint64_t &clipped, uint64_t &reprojected);
// Displaced reprojection (pt_temporal_set_motion), for an editor whose user drags objects.  Read by Render when the
// accumulation is on: the frame records the object index plane (pt_set_object_ids), Render remembers the scene of the last frame it
// accumulated and compares the next one with it -- when only object positions and the camera differ, the displacements go to
// pt_temporal (nothing is passed when none is non-zero); when anything else differs (the number, order, type, size or material of
// the objects, the material table, sky, background or fog) the history is reset first.  The initial value is
// PATHTRACER_GPU_TEMPORAL_MOTION (TemporalMotionFromEnv).
void SetTemporalMotion(bool on);
bool TemporalMotion();
bool TemporalMotionFromEnv();  // PATHTRACER_GPU_TEMPORAL_MOTION = 1 / true / on / yes
// Features on the BVH path (pt_set_feature_walk): scenes beyond 128 spheres or 128 boxes collect the feature planes by a
// wave-shared walk of the tree, so the filter's feature terms, the accumulation and the object ids work there too.  Off unless said
// or PATHTRACER_GPU_FEATURE_WALK (FeatureWalkFromEnv); with it on, the unsaid feature count is 4 under the filter on those scenes too.
void SetFeatureWalk(bool on);
bool FeatureWalk();
bool FeatureWalkFromEnv();  // PATHTRACER_GPU_FEATURE_WALK = 1 / true / on / yes
// Volumetric fog on the BVH path (pt_set_fog_walk): scenes beyond 128 spheres or 128 boxes draw a gpu_volumetric fog
// block, the closest hit and the shadow rays of the term answered by wave-shared walks of the tree; the frame is the model's, bit for
// bit, at 24 x lights shadow rays per sample.  Off unless said or PATHTRACER_GPU_FOG_WALK (FogWalkFromEnv); without it such a frame
// is refused by the library.
void SetFogWalk(bool on);
bool FogWalk();
bool FogWalkFromEnv();  // PATHTRACER_GPU_FOG_WALK = 1 / true / on / yes
// GL shading on the BVH path (pt_set_shading_walk): scenes beyond 128 spheres or 128 boxes render with the GL model,
// its closest hits, shadow rays and metal probes answered by the lane's own walk of the tree; the frame is the model's, bit for
// bit.  Off unless said or PATHTRACER_GPU_SHADING_WALK (ShadingWalkFromEnv); without it such a frame is refused by the library.
void SetShadingWalk(bool on);
bool ShadingWalk();
bool ShadingWalkFromEnv();  // PATHTRACER_GPU_SHADING_WALK = 1 / true / on / yes
// Features and the a-trous filter for GL-shaded frames (pt_set_shading_features): a GL frame collects the first-hit
// features of its own camera rays (k counts passes of 16 paths; 1 under the filter unless said), and the filter and the filtered
// noise target accept it, the image being GL's tone map of the filtered mean.  Off unless said or PATHTRACER_GPU_SHADING_FEATURES
// (ShadingFeaturesFromEnv); without it such frames are refused as before.
void SetShadingFeatures(bool on);
bool ShadingFeatures();
bool ShadingFeaturesFromEnv();  // PATHTRACER_GPU_SHADING_FEATURES = 1 / true / on / yes
// Refit of the hierarchy on the devices (pt_set_bvh_refit): a frame whose scene differs from the previous frame's only in
// where its objects are keeps the tree's topology and recomputes its boxes on the GPU; max_growth >= 1 (or inf) bounds how far the
// refitted tree's quality figure may exceed the built one's before the next frame rebuilds.  0 (and anything below 1) is off, the
// default; not said: PATHTRACER_GPU_BVH_REFIT (BvhRefitFromEnv).  The library detects the refittable edits by itself.
void SetBvhRefit(double max_growth);
double BvhRefit();
double BvhRefitFromEnv();  // PATHTRACER_GPU_BVH_REFIT = a number >= 1 or inf, else 0
// Build of the hierarchy on the device (pt_set_bvh_build): with mode 1 every full build of a scene's tree -- an object
// added or removed, a material or a type changed, the first frame, a refitted tree that outgrew its bound -- runs on devices[0] in
// Morton order instead of on the host.  0 is the host builder, the default; not said: PATHTRACER_GPU_BVH_BUILD (BvhBuildFromEnv).
void SetBvhBuild(int mode);
int BvhBuild();
int BvhBuildFromEnv();  // PATHTRACER_GPU_BVH_BUILD = device: 1, else 0
void SetFeatures(int k);
int GetFeatures();     // -1: not said
int FeaturesFromEnv(); // PATHTRACER_GPU_FEATURES = int >= 0, else -1
void Shutdown();                                    // releases the process-wide context
}  // namespace hip

// scene.Fog flattened into the C ABI's pt_fog (raw fields; libptcore resolves them).
void FlattenFog(const scene::Fog &f, pt_fog &out);
// The scene's pt_gl_material table (reflectivity, tint, absorption_scale per material, raw) for pt_set_shading.
void FlattenGlMaterials(const scene::Scene &sc, std::vector<pt_gl_material> &out);

// RenderInto (renderer.go:34-41).  BackendGPU goes to hip::Render.  The CPU branch is the reference's
// own Go renderer and is not shipped: selecting it, or a GPU failure (where the reference falls back
// to it, renderer.go:257-262), throws std::runtime_error here.
void RenderInto(const scene::Scene &sc, const RenderConfig &cfg, RGBA &img, const std::function<void()> &progress,
                Stats *stats = nullptr);
RGBA Render(const scene::Scene &sc, const RenderConfig &cfg);                       // renderer.go:25-29
RGBA RenderScene(const scene::Scene &sc, const scene::RenderSettings &settings, uint64_t seed = 1);  // util.go:13-22
scene::RenderSettings RenderSettingsForMode(const std::string &mode);               // util.go:25-42
// The editor's "scene settings override" (internal/ui/app.go:60-75): the mode preset, replaced by the scene's own
// width x height when BOTH are > 0 (and, only then, by its samples_per_px / max_depth when > 0); a "final" render
// then takes four times the samples and twice the depth (app.go:72-75).  cmd/render ignores scene.settings
// (main.go:52); the CLI twin applies this rule only under -scene-settings.
scene::RenderSettings RenderSettingsForScene(const scene::Scene &sc, const std::string &mode);
void SavePNG(const std::string &path, const RGBA &img);                             // util.go:45-55; throws "create png: ..."

}  // namespace engine
}  // namespace pthost
