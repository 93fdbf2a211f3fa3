/*
 * ptcore.h -- C ABI of libptcore.so, the MI355X (gfx950) path-tracing core.
 *
 * Drop-in boundary for ONE path of MarkJulian19/path_trace_golang: the per-pixel
 * Monte-Carlo render loop of internal/engine.  The entry points are what a Go
 * backend package binds through cgo in place of the reference's OpenGL backend
 *
 *     gpu.Render(sc *scene.Scene, cfg gpu.RenderConfig, img *image.RGBA,
 *                progress func()) error          internal/engine/gpu/gpu.go:2534
 *
 * which engine.RenderInto dispatches to (internal/engine/renderer.go:34-41,
 * :250-263).  Plain pointers and sizes only; no C++ or torch types.  The cgo
 * binding is shown in INTEGRATION.md; a C++ mirror of the Go host layer lives in
 * path_trace_golang_amd/csrc/host/ for machines without a Go toolchain.
 *
 * Semantics are those of the reference CPU engine (renderIntoCPU,
 * renderer.go:44-246), not of its GLSL backend: FP64 arithmetic, linear object
 * scan, sqrt gamma, uint8(v*255.999).  The one deliberate difference is the RNG:
 * the reference seeds math/rand from the clock (random.go:14-16); here each
 * (seed, pixel, sample) owns a counter-based stream, so a render is reproducible
 * and independent of device count.
 *
 * Threading: a pt_ctx is not re-entrant (the reference serialises GPU renders
 * through one goroutine too, gpu.go:250-297, :2534-2546).  Different contexts
 * may be used from different threads.  No pointer passed in is retained after a
 * call returns (cgo pointer rule).
 */
#ifndef PTCORE_H
#define PTCORE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PT_ABI_VERSION 4

/* status codes; pt_last_error() holds the text (thread-local) */
enum {
    PT_OK = 0,
    PT_ERR_INVALID = 1,   /* bad argument / inconsistent scene */
    PT_ERR_NO_DEVICE = 2, /* no usable HIP device */
    PT_ERR_HIP = 3,       /* HIP runtime error */
    PT_ERR_NOMEM = 4,
    PT_ERR_STATE = 5      /* call out of sequence (pt_step without pt_begin, ...) */
};

/* scene.MaterialType strings (internal/scene/scene.go:33-40) in materialType
 * order (internal/engine/materials.go:11-17).  Any other string is PT_MAT_LAMBERT:
 * convertMaterial's default branch (materials.go:51-53). */
enum { PT_MAT_LAMBERT = 0, PT_MAT_METAL = 1, PT_MAT_DIELECTRIC = 2, PT_MAT_EMISSIVE = 3, PT_MAT_MIRROR = 4 };

/* scene.ObjectType strings (scene.go:66-73).  Any other string is PT_OBJ_UNKNOWN
 * and is skipped like sceneToWorld does (internal/engine/objects.go:237-266). */
enum { PT_OBJ_UNKNOWN = -1, PT_OBJ_SPHERE = 0, PT_OBJ_PLANE = 1, PT_OBJ_BOX = 2, PT_OBJ_SPHERE_LIGHT = 3 };

/* Sky selection of the closure at renderer.go:56-92. */
enum {
    PT_SKY_BACKGROUND = 0, /* scene.Sky == nil, or Sky.Type not "gradient"/"solid": scene.Background */
    PT_SKY_GRADIENT = 1,
    PT_SKY_SOLID = 2
};

/* scene.Material (scene.go:41-63): the fields convertMaterial reads
 * (materials.go:28-55).  Reflectivity, Tint, AbsorptionScale are ignored by the
 * CPU engine and do not cross the boundary. */
typedef struct pt_material {
    int32_t type; /* PT_MAT_* */
    int32_t reserved;
    double albedo[3];
    double rough;
    double ior;
    double emit[3];
    double power;
    double absorption[3];
    double smoothness;
} pt_material;

/* scene.Object (scene.go:76-84). `material` is the index into pt_scene.materials
 * of the material whose ID equals Object.MaterialID (the LAST one if IDs repeat:
 * the map assignment at objects.go:227-229), or -1 when no material has that ID
 * (zero material = black lambert, objects.go:233). */
typedef struct pt_object {
    int32_t type; /* PT_OBJ_* */
    int32_t material;
    double position[3];
    double size[3]; /* sphere radius = size[0]; box full extents; plane ignores it */
} pt_object;

/* scene.Camera (scene.go:24-32) */
typedef struct pt_camera {
    double position[3];
    double target[3];
    double up[3];
    double fov;
    double aperture;
    double focus_dist;
    double aspect_ratio;
} pt_camera;

/* scene.Sky (scene.go:135-140) + scene.Background (scene.go:150) */
typedef struct pt_sky {
    int32_t kind; /* PT_SKY_* */
    int32_t reserved;
    double background[3];
    double color[3];
    double horizon[3];
    double zenith[3];
} pt_sky;

typedef struct pt_scene {
    pt_camera camera;
    pt_sky sky;
    int32_t num_materials;
    int32_t num_objects;
    const pt_material *materials;
    const pt_object *objects;
} pt_scene;

/* engine.RenderConfig (renderer.go:17-22) + the stream seed. */
typedef struct pt_config {
    int32_t width;
    int32_t height;
    int32_t samples_per_px;
    int32_t max_depth;
    uint64_t seed;
    int32_t spp_chunk; /* samples per pixel per device pass; 0 = choose from the buffer budget */
    int32_t flags;     /* PT_FLAG_* */
} pt_config;

enum {
    PT_FLAG_NONE = 0,
    PT_FLAG_PIXEL_STATS = 1 /* also produce per-pixel segment / RNG-draw counts (slower; parity debugging) */
};

/* Which 32x32 tiles (renderer.go:132, row-major tile index t = ty*ntx + tx) this
 * call renders: t = index, index+count, index+2*count, ...  {0,1} = whole frame. */
typedef struct pt_shard {
    int32_t index;
    int32_t count;
} pt_shard;

typedef struct pt_stats {
    uint64_t samples;    /* primary samples traced */
    uint64_t segments;   /* closest-hit scans = rayColorOpt activations with depth > 0 (renderer.go:286-302) */
    uint64_t exit_scans; /* dielectric exit searches (renderer.go:316-371) */
    uint64_t draws;      /* RNG draws */
    double seconds;      /* host wall time of the call (upload + kernels + download) */
    double trace_ms;     /* device time inside the trace kernel(s) alone, HIP events around each launch */
    double resolve_ms;   /* device time inside the resolve kernel(s) */
    double device_ms;    /* device time first launch -> last launch complete */
    int32_t trace_launches;
    int32_t resolve_launches;
    int32_t spp_chunk;   /* chunk actually used */
    int32_t num_devices;
    double per_device_ms[8];
    double raygen_ms;    /* device time inside the ray-generation kernel(s) */
    /* split passes (ABI 2): dielectric hits leave the trace kernel through a path-state queue and are shaded by glass_kernel */
    double glass_ms;       /* device time inside glass_kernel */
    double trace_split_ms; /* the part of trace_ms spent in the split form of the trace kernel (the dominant launches) */
    int32_t glass_launches;
    int32_t trace_split_launches;
    uint64_t glass_events;    /* paths parked in the glass queue by the split trace passes (= dielectric closest hits there) */
    uint64_t continuations;   /* paths glass_kernel handed back through the continuation queue */
    uint64_t split_cont_in;   /* continuation entries taken up by split trace passes (the rest finish in the all-in-one pass) */
    uint64_t split_finished;  /* paths that ended inside a split trace pass */
    /* ABI 3: the shader clock the trace kernels actually ran at: one wave per launch reads the shader-cycle counter
     * (s_memtime) and the 100 MHz reference counter (s_memrealtime) when it starts and when it retires; the ratio of
     * the sums over the frame's trace launches (0 when no trace launch was observed) */
    double shader_clock_mhz;
} pt_stats;

typedef struct pt_ctx pt_ctx;

int32_t pt_abi_version(void);

/* Text of the last failure on the calling thread ("" if none). Never NULL. */
const char *pt_last_error(void);

/* Number of visible HIP devices (0 and PT_ERR_NO_DEVICE if none). */
int32_t pt_device_count(int32_t *count);

/* Creates a context on `ndev` devices (`devices` = HIP ordinals; NULL = 0..ndev-1).
 * Replaces the lazily created GL worker of gpu.go:266-297.  Like the reference,
 * an init failure is an error return, never an abort. */
int32_t pt_create(const int32_t *devices, int32_t ndev, pt_ctx **out);
void pt_destroy(pt_ctx *ctx);

/*
 * Blocking whole-frame render into caller memory: the body of gpu.Render.
 *   rgba   : `height` rows of `stride` bytes (image.RGBA.Pix / .Stride), row 0 = top,
 *            A = 255, written completely before return (renderer.go:106-112, :218-221)
 *   accum  : optional width*height*3 doubles, per pixel the raw sum over samples of
 *            the sample radiance (before the 1/spp scale of renderer.go:190-192)
 *   nseg / ndraw : optional width*height uint32 (need PT_FLAG_PIXEL_STATS)
 * With several devices in the context the frame is split over interleaved 32x32
 * tiles and gathered on devices[0]; pixels do not depend on the device count.
 */
int32_t pt_render(pt_ctx *ctx, const pt_scene *scene, const pt_config *cfg, uint8_t *rgba, int32_t stride,
                  double *accum, uint32_t *nseg, uint32_t *ndraw, pt_stats *stats);

/*
 * Progressive form (the interactive contract of gpu.go:2209-2290: preview
 * refreshes while samples accumulate).  pt_begin uploads the scene; each pt_step
 * adds up to `nspp` samples per pixel and returns the total done so far; pt_read
 * resolves the current estimate (normalised by the samples done) without ending
 * the render; pt_end releases the frame and reports totals.  The Go wrapper calls
 * progress() between steps, so no C -> Go callback is needed.
 */
int32_t pt_begin(pt_ctx *ctx, const pt_scene *scene, const pt_config *cfg);
int32_t pt_step(pt_ctx *ctx, int32_t nspp, int32_t *done_spp);
int32_t pt_read(pt_ctx *ctx, uint8_t *rgba, int32_t stride, double *accum);
int32_t pt_end(pt_ctx *ctx, pt_stats *stats);

/*
 * Device-resident form for one-process-per-GPU hosts (bench.py, torch.distributed):
 * renders the tiles of `shard` on the context's first device, asynchronously on
 * `stream` (a hipStream_t; NULL = the context's own stream) and leaves
 *   d_tiles_rgba  : [ntiles_local][32][32][4] uint8 (device), tile-major
 *   d_tiles_accum : optional [ntiles_local][32][32][3] double (device)
 * for the caller to gather.  Pixels outside the frame in edge tiles are zero.
 * pt_shard_tiles() gives ntiles_local.  Stats are filled after the stream drains
 * only if `stats` is non-NULL (that makes the call blocking).
 */
int32_t pt_shard_tiles(int32_t width, int32_t height, const pt_shard *shard, int32_t *ntiles_local,
                       int32_t *ntiles_x, int32_t *ntiles_y);
int32_t pt_render_tiles_device(pt_ctx *ctx, const pt_scene *scene, const pt_config *cfg, const pt_shard *shard,
                               void *d_tiles_rgba, void *d_tiles_accum, void *stream, pt_stats *stats);

/* Scatters gathered tile buffers into a row-major frame on the device: d_rgba =
 * height rows of `stride` bytes (stride % 4 == 0); d_accum optional width*height*3
 * doubles.  The gathered buffer holds shard 0's tiles, then shard 1's, ...; shard k
 * starts at tile k*shard_stride_tiles, or right after shard k-1 when
 * shard_stride_tiles == 0 (compact).  A fixed stride is what an equal-sized
 * collective gather (ncclGather / torch.distributed.gather) produces. */
int32_t pt_untile_device(pt_ctx *ctx, int32_t width, int32_t height, int32_t shard_count, int32_t shard_stride_tiles,
                         const void *d_tiles_rgba, const void *d_tiles_accum, void *d_rgba, int32_t stride,
                         void *d_accum, void *stream);

/*
 * Optional post-process passes of the reference's OpenGL backend, applied after a render:
 *   tonemap : rgba = uint8(sqrt(aces(float32(accum/spp)))*255 + 0.5)   acesTonemap internal/engine/gpu/gpu.go:22-47,
 *             the loop at gpu.go:2309-2350 -- replaces the CPU engine's finish; needs `accum`
 *   denoise : 3x3 bilateral filter on the 8-bit image, gpu.go:2355-2439 (defaults sigma_s 1.0, sigma_r 0.15,
 *             gpu.go:77-95; skipped unless width > 2 && height > 2)
 *   smooth  : box blur of radius 1..5 blended by strength 0..1, gpu.go:2444-2520 (defaults 2 and 0.5, gpu.go:140-175)
 * None of them is part of the CPU engine's image; they exist so that a user of the reference's -gpu look can have
 * it.  rgba is `height` rows of `stride` bytes in host memory, updated in place; accum (width*height*3 doubles, the
 * raw sums pt_render returns) may be NULL when tonemap is 0.
 */
typedef struct pt_post_config {
    int32_t tonemap;
    int32_t denoise;
    double sigma_s;
    double sigma_r;
    int32_t smooth;
    int32_t smooth_radius;
    double smooth_strength;
} pt_post_config;
int32_t pt_post_process(pt_ctx *ctx, const pt_post_config *post, const double *accum, int32_t samples_per_px, uint8_t *rgba,
                        int32_t stride, int32_t width, int32_t height);

/*
 * Fog (ABI 4): the scene's fog block (scene.Fog, internal/scene/scene.go:101-131) as the reference's OpenGL backend draws it
 * (internal/engine/gpu/gpu.go:1125-1341): a sky blended towards the fog colour (affect_sky) and single-scattered light from
 * the emissive spheres along each sample's primary ray (gpu_volumetric), added to the sample radiance.  Not part of the CPU
 * engine's image, so it is off unless asked for.  The model, restated in FP64, is documented in csrc/pt_fog.h and DESIGN.md.
 *   pt_set_fog(ctx, &fog) : later renders on ctx (every entry point) use this block; pt_set_fog(ctx, NULL) turns fog off
 *                           (the default).  The block is copied.
 *   pt_fog_last_stats     : what the fog kernel did in the last finished frame of ctx (zeros when it did not run).
 * Scenes on the bounding-volume-hierarchy path (more than 128 spheres or 128 boxes) refuse gpu_volumetric with
 * PT_ERR_INVALID unless pt_set_fog_walk is on; affect_sky alone works on every scene.  Segment and draw counts (pt_stats,
 * nseg / ndraw) stay those of the surface paths: the fog term draws from a stream of its own.
 *   pt_set_fog_walk(ctx, on) : additive to ABI 4; default 0; PT_ERR_STATE while a frame is open.  With it on, a frame with a
 *                           gpu_volumetric block on the bounding-volume-hierarchy path is accepted: the closest hit of a sample's
 *                           primary ray and every shadow ray of the term are answered by one walk of the tree per wave of 64
 *                           coherent rays (an 8 x 8 pixel block) instead of a loop over all objects, with the same
 *                           exact tests -- the image, the sums and pt_fog_last_stats are those of the model, bit for bit.  A wave
 *                           that holds a ray outside the range the walk was analysed for (non-finite components, an origin beyond
 *                           3.5 scene sizes -- march points of a camera far from the scene) takes the plain loop for that turn.  The
 *                           cost stays 24 x lights shadow rays per sample.  Frames on the other scans ignore the setting; GL shading
 *                           on that path stays refused unless pt_set_shading_walk (which refuses gpu_volumetric there); injected
 *                           primary rays with fog on stay refused.
 *   pt_fog_walk_stats     : out[0] = (wave, sample) pairs of the last frame whose primary rays were walked by the wave, out[1] = those
 *                           sent to the plain scan, out[2] = shadow turns (one march step x one light of a wave) walked, out[3] =
 *                           those sent to the plain loop, out[4] = node visits of the shadow walks, out[5] = the deepest wave stack
 *                           seen; summed over the devices (out[5]: their largest).  PT_ERR_STATE when the last frame did not run the
 *                           walk.  Waits for the devices' streams.
 */
typedef struct pt_fog {
    double density;
    double color[3];
    double scatter;
    double sigma_s;
    double sigma_a;
    double g;
    double hetero_strength;
    double noise_scale;
    int32_t noise_octaves;
    int32_t affect_sky;     /* 0 or 1 */
    int32_t gpu_volumetric; /* 0 or 1 */
    int32_t reserved;
} pt_fog;

typedef struct pt_fog_stats {
    double fog_ms;          /* device time inside fog_kernel / fog_bvh_kernel (longest device) */
    int32_t fog_launches;
    int32_t reserved;
    uint64_t shadow_rays;   /* light samples that reached the occlusion test */
    uint64_t draws;         /* fog-stream draws */
    uint64_t steps;         /* march steps taken (sigma_s > 0 and sigma_t > 0) */
} pt_fog_stats;

int32_t pt_set_fog(pt_ctx *ctx, const pt_fog *fog);
int32_t pt_fog_last_stats(pt_ctx *ctx, pt_fog_stats *out);
int32_t pt_set_fog_walk(pt_ctx *ctx, int32_t on);
int32_t pt_fog_walk_stats(pt_ctx *ctx, uint64_t out[6]);

/*
 * GL shading (additive to ABI 4): the estimator of the reference's OpenGL compute shader (rayColor and main,
 * internal/engine/gpu/gpu.go:1300-1732) as a second shading model, restated in FP64 in csrc/pt_glshade.h:
 * next-event estimation over the emissive objects, GGX rough metals, smoothness / reflectivity, glass tint and absorption,
 * 16 stratified paths per pass.  Not the CPU engine's image, so it is off unless asked for.
 *   pt_set_shading(ctx, &s) : later renders on ctx (every entry point) use model s.model; NULL = PT_SHADING_CPU (the default).
 *                             The block and its material table are copied.
 *   pt_shading_last_stats   : what the GL kernel did in the last finished frame of ctx (zeros when it did not run).
 * In GL mode a "sample" is a pass: spp, spp_chunk and pt_step count passes.  A pass adds its 16 paths WITHOUT dividing by
 * 16 (the shader as its host drives it), so accum / passes is GL's linear value, and the 8-bit image is the tone-mapped
 * finish of pt_post_process(tonemap = 1) on accum.  pt_stats.samples, segments and draws count GL paths, closest-hit scans
 * and draws; trace_ms is the GL kernel's time.  A GL render returns PT_ERR_INVALID without launching anything when the
 * scene's material count differs from num_materials, with PT_FLAG_PIXEL_STATS, and for scenes on the bounding-volume-
 * hierarchy path (more than 128 spheres or 128 boxes) unless pt_set_shading_walk is on.
 *   pt_set_shading_walk(ctx, on) : additive to ABI 4; default 0; PT_ERR_STATE while a frame is open.  With it on, a GL frame on
 *                             the bounding-volume-hierarchy path is accepted: every segment's closest hit, every shadow ray and
 *                             every metal probe is answered by the lane's own walk of the tree (csrc/pt_gl_walk.h, DESIGN.md
 *                             3.8a) instead of a loop over all objects, with the same exact tests and the loop's winner under
 *                             GL's tie rule -- the image, the sums and pt_shading_last_stats are those of the model, bit for
 *                             bit.  A query whose ray lies outside the range the walk was analysed for (non-finite components,
 *                             an origin beyond 3.5 scene sizes) takes the plain loop, per lane and per query.  Frames on the
 *                             other scans ignore the setting.  Refused on that path, each with PT_ERR_INVALID or PT_ERR_STATE
 *                             and a message of its own: a scene with an object of unknown type (or one whose GL objects are not
 *                             the tree's: the message names the object and the rule), a gpu_volumetric fog block (its march
 *                             still loops over all objects; affect_sky alone is accepted), PT_FLAG_PIXEL_STATS, features,
 *                             adaptive sampling and injected primary rays.
 *   pt_shading_walk_stats   : out[0] = closest-hit queries of the last frame answered by a walk, out[1] = those sent to the plain
 *                             loop, out[2] = shadow queries walked, out[3] = those sent to the plain loop, out[4] = node visits
 *                             of the closest walks, out[5] = of the shadow walks, out[6] = the deepest stack seen; summed over the
 *                             devices (out[6]: their largest).  PT_ERR_STATE when the last frame did not run the walk.  Waits for
 *                             the devices' streams.
 */
enum { PT_SHADING_CPU = 0, PT_SHADING_GL = 1 };

/* scene.Material fields only the GL model reads (scene.go:41-63), one entry per scene material, raw */
typedef struct pt_gl_material {
    double reflectivity;
    double tint[3];
    double absorption_scale;
} pt_gl_material;

typedef struct pt_shading {
    int32_t model;         /* PT_SHADING_* */
    int32_t num_materials; /* entries of `materials` (GL model) */
    const pt_gl_material *materials;
} pt_shading;

typedef struct pt_shading_stats {
    double gl_ms;          /* device time inside gl_trace_kernel / gl_bvh_kernel (longest device) */
    int32_t gl_launches;
    int32_t reserved;
    uint64_t paths;        /* GL paths traced (16 per pixel and pass) */
    uint64_t segments;     /* closest-hit scans of the main loop */
    uint64_t shadow_rays;  /* NEE shadow rays traced (after the distance and cosine tests) */
    uint64_t probe_rays;   /* rough-metal reflect-direction probes */
    uint64_t draws;        /* main-stream draws (the fog stream's are in pt_fog_stats) */
} pt_shading_stats;

int32_t pt_set_shading(pt_ctx *ctx, const pt_shading *s);
int32_t pt_shading_last_stats(pt_ctx *ctx, pt_shading_stats *out);
int32_t pt_set_shading_walk(pt_ctx *ctx, int32_t on);
int32_t pt_shading_walk_stats(pt_ctx *ctx, uint64_t out[7]);

/*
 * Second moments and the frame noise figure (additive to ABI 4).  Off unless asked for: with moments off
 * nothing is allocated or launched.
 *   pt_set_moments(ctx, on) : default 0; later frames on ctx (pt_begin ... pt_end, pt_render) also collect, per pixel and
 *                             channel, Q = the sum over the samples done of L*L, next to accum's S = the sum of L.  L is the
 *                             radiance the pixel receives (fog included; in GL mode a pass sum).  48 B per pixel on the
 *                             devices, outside PTCORE_L_BUDGET_MB.  pt_render_tiles_device neither collects moments nor fails.
 *   pt_read_moments         : m2 = width*height*3 doubles, row-major like accum: Q.
 *   pt_noise_estimate       : the noise of the frame, computed on the device.  With n = samples done, per pixel
 *                                 m_c = S_c / n                                   (c = r, g, b)
 *                                 v_c = max(0, Q_c / n - m_c * m_c) / (n - 1)     variance of the pixel's mean
 *                                 e2  = ((v_r + v_g + v_b) / 3) / max((m_r + m_g + m_b) / 3, 0.01)^2
 *                             and noise = sqrt(sum of e2 / pixels), max_pixel = the largest e2, pixels = width*height.  A
 *                             pixel whose e2 is NaN or infinite contributes 0 and is counted in bad_pixels.  With n < 2
 *                             noise and max_pixel are +inf.  The sum is taken over a fixed tree (per block on the device,
 *                             blocks and devices in order on the host): the same bits every time for one context shape.
 * Both reads are valid between pt_begin and pt_end once a step has run, and after pt_end / pt_render until the next frame
 * opens on ctx; otherwise, and for a frame rendered with moments off, they return PT_ERR_STATE (the context stays usable).
 * A host that wants "render until the noise is at or below T" steps a pt_begin frame whose samples_per_px is the cap and
 * stops at the first check with n >= 2 and noise <= T; the image at the stop is the image of a frame of n samples.
 */
typedef struct pt_noise {
    double noise;
    double max_pixel;
    uint64_t pixels;
    uint64_t bad_pixels;
    int32_t spp; /* samples done (n) */
    int32_t reserved;
} pt_noise;

int32_t pt_set_moments(pt_ctx *ctx, int32_t on);
int32_t pt_read_moments(pt_ctx *ctx, double *m2);
int32_t pt_noise_estimate(pt_ctx *ctx, pt_noise *out);

/*
 * Adaptive sampling (additive to ABI 4): 8x8 pixel blocks stop when their own noise reaches a target.  Off unless
 * asked for.
 *   pt_set_adaptive(ctx, &a) : later frames on ctx (pt_begin ... pt_end, pt_render) are adaptive; NULL = off (the default).  Such
 *                              frames collect second moments whether or not pt_set_moments asked for them.
 * The unit is one 8x8 sub-block of a 32x32 tile.  A block with no pixel inside the frame is never sampled and has count 0.  With
 * e2 the per-pixel quantity of pt_noise_estimate, taken with the pixel's own n, a block's noise is b = sqrt(sum of e2 / k) over its
 * k pixels inside the frame (a NaN or infinite e2 adds 0 and still counts in k).  At the end of every pt_step, once the samples
 * done reach max(min_spp, 2), every still-active block with b <= target becomes inactive and stays so for the rest of the frame;
 * later steps trace the active blocks only.  All active blocks hold `done` samples, an inactive block keeps the count it stopped
 * at.  pt_step returns `done`; once no block is active it adds nothing and keeps returning the last value.  Which blocks stop
 * depends on the sizes of the steps, and on nothing else: not on spp_chunk, the buffer budget, the device count or the scan form.
 * pt_read / pt_end / pt_render normalise each pixel by its own count; accum and the moments stay raw sums, so a block stopped at
 * n holds exactly the pixels of a plain n-sample frame.  pt_render steps internally, `step` samples at a time (values < 1 count
 * as 1), up to samples_per_px, and stops early when no block is active.  pt_stats.samples is the sum of the counts;
 * pt_noise_estimate uses each pixel's own n and reports spp = the largest count; PT_FLAG_PIXEL_STATS gives the nseg / ndraw of each
 * pixel's first n samples.
 * Known bias: a block can stop while it is still missing rare bright paths (its variance estimate has not seen them either);
 * min_spp is the guard against that.  Neighbouring blocks do not keep each other alive.
 *   pt_adaptive_state       : the block table of the open or last frame.
 *   pt_read_sample_counts   : spp = width*height uint32, row-major: the samples each pixel holds.
 * Both are valid when pt_read_moments is (and return PT_ERR_STATE otherwise, also for a frame that was not adaptive).
 * pt_render_tiles_device neither adapts nor fails.  An adaptive frame is refused with PT_ERR_STATE, before anything is launched and
 * with the context left usable, together with GL shading (pt_set_shading), with injected primary rays
 * (pt_debug_set_primary_rays) and on a context created with PTCORE_PIPELINE=wavefront or walk32 (the adaptive job map exists for
 * the default pipeline only).  Thin-lens cameras take the one-job-per-lane ray generation in adaptive frames.
 */
typedef struct pt_adaptive {
    double target;
    int32_t min_spp;
    int32_t step; /* used by pt_render only */
} pt_adaptive;

/* (the struct and the function that fills it share their name: C keeps struct tags apart from functions, a typedef name it would
 * not, so this one struct is spelled with its tag) */
struct pt_adaptive_state {
    uint64_t blocks;        /* blocks with a pixel inside the frame */
    uint64_t active_blocks;
    uint64_t samples;       /* sum of the in-frame pixels' counts */
    int32_t spp_min, spp_max;
    double worst_active;    /* largest block noise among active blocks at the last check, 0 if none */
};

int32_t pt_set_adaptive(pt_ctx *ctx, const pt_adaptive *a);
int32_t pt_adaptive_state(pt_ctx *ctx, struct pt_adaptive_state *out);
int32_t pt_read_sample_counts(pt_ctx *ctx, uint32_t *spp);

/*
 * First-hit feature planes (additive to ABI 4): what each pixel looks at, for filters, picking and previews.  Off
 * unless asked for: with k = 0 nothing is allocated or launched.
 *   pt_set_features(ctx, k) : k = feature samples per pixel (0 = off, the default; k < 0 is PT_ERR_INVALID).  Later frames on ctx
 *                             (pt_begin ... pt_end, pt_render) collect, per pixel and over its samples with index s < k, the first hit
 *                             of the sample's primary ray -- the CPU engine's closest hit of the first segment -- as three raw sums
 *                             of three doubles, added in sample order:
 *                                 normal : the hit record's face-forward unit normal (a miss adds nothing)
 *                                 albedo : the converted material's albedo (a missing material id is the zero material)
 *                                 depth  : (sum of t * |direction|, samples that hit, feature samples taken = min(k, the pixel's count))
 *                             72 B per pixel on the devices, outside PTCORE_L_BUDGET_MB.  pt_render_tiles_device neither collects
 *                             nor fails.  A frame with k > 0 is refused with PT_ERR_INVALID, before anything is launched and with the
 *                             context left usable, for scenes on the bounding-volume-hierarchy path (more than 128 spheres or 128
 *                             boxes) and with GL shading (pt_set_shading).  pt_set_feature_walk lifts the first refusal.
 *   pt_set_feature_walk(ctx, on) : default 0; PT_ERR_STATE while a frame is open.  With it on, a frame with k > 0 on the bounding-
 *                             volume-hierarchy path is accepted: the first hit of a feature sample is found by one walk of the tree
 *                             per wave of 64 coherent primary rays (an 8 x 8 pixel block) instead of a linear scan,
 *                             with the same tests and the same winner -- the planes and ids are those of the definition above, bit
 *                             for bit.  A wave that holds a ray outside the range the walk was analysed for (non-finite or absurd
 *                             components, an origin beyond 3.5 scene sizes) takes the plain scan for that sample.  Frames on the
 *                             other scans ignore the setting.  GL shading on that path stays refused unless pt_set_shading_walk;
 *                             volumetric fog has a switch of its own (pt_set_fog_walk).
 *   pt_set_shading_features(ctx, on) : additive to ABI 4; default 0; PT_ERR_STATE while a frame is open, PT_ERR_INVALID for a null
 *                             ctx.  With it off everything is as described above.  With it on, a frame rendered with GL shading
 *                             (pt_set_shading) accepts pt_set_features(k > 0) and pt_set_object_ids -- on the hierarchy path together
 *                             with pt_set_shading_walk, which GL shading needs there anyway; pt_set_feature_walk is not consulted --
 *                             and pt_atrous and pt_atrous_halves accept the frame (with k = 0: on luminance alone).  In GL mode k
 *                             counts passes, as samples_per_px, spp_chunk and pt_step do.  The definition (csrc/pt_gl_features.h):
 *                             for pixel (x, y), pass p < k and stratum j = 0 .. 15, in (p, j) order,
 *                                 ray    : the GL pass's own camera ray of path 16 p + j (its stream, its two jitter draws, its lens
 *                                          rejection of at most 16 tries when aperture > 0), direction of unit length
 *                                 hit    : GL's closest hit in [0.001, 1e20] -- GL's tests, a later object winning a tie, no object skipped
 *                                 normal : the hit's face-forward unit normal (a miss adds nothing)
 *                                 albedo : the hit material's albedo as GL packs it (emissive materials included; a missing id is material 0)
 *                                 depth  : (sum of t, paths that hit, paths taken = 16 * min(k, passes done))
 *                             and the object id is the first hit of (p = 0, j = 0) or -1.  GL's object list is the scene's -- an
 *                             object of unknown type is a sphere there and can be hit -- so the id indexes pt_scene.objects.  The
 *                             fog term does not enter.  pt_read_features and pt_read_object_ids are valid as documented below.
 *                             pt_atrous finishes rgba by GL's tone map (pt_post_process's, of the mean); with 0 iterations the bytes
 *                             are pt_read's.  Note that c is accum / passes there, 16 x the mean path radiance, so the 0.01 floor
 *                             on l in the noise figures is 16 times tighter relative to the path radiance than on a CPU-model frame.
 *                             Still refused, each with its message: pt_temporal on a GL frame (its projection is the CPU camera's),
 *                             adaptive sampling with GL shading, PT_FLAG_PIXEL_STATS, injected rays, and gpu_volumetric fog with
 *                             pt_set_shading_walk.
 *   pt_feature_walk_stats  : out[0] = (wave, feature sample) pairs of the last frame walked by the wave, out[1] = those sent to the
 *                             plain scan, out[2] = node visits of the walks, out[3] = the deepest wave stack seen; summed over the
 *                             devices (out[3]: their largest).  PT_ERR_STATE when the last frame did not run the walk.  Waits for
 *                             the devices' streams.
 *   pt_read_features        : normal / albedo / depth = width*height*3 doubles each, row-major, any of them NULL.  Valid exactly
 *                             when pt_read_moments is (so the frame collects moments); PT_ERR_STATE otherwise and for a frame with k = 0.
 *   pt_set_object_ids(ctx, on) : default 0; PT_ERR_STATE while a frame is open.  Later frames on ctx with features on (k > 0) also
 *                             record, per in-frame pixel, the index into pt_scene.objects (file order) of the first hit of the pixel's
 *                             sample 0, or -1 on a miss: the hit that sample's normal, albedo and depth come from, the same test
 *                             and the same winner.  An object of unknown type keeps its index and is never hit.  With injected
 *                             primary rays the id is that of the injected ray, as the features are.  4 B per pixel on the devices,
 *                             outside PTCORE_L_BUDGET_MB, allocated on the first frame that asks.  A frame with ids on and k = 0 is
 *                             PT_ERR_INVALID before anything is launched (the context stays usable); the BVH and GL-shading refusals
 *                             are the features' own.  pt_render_tiles_device neither collects nor fails.  For picking, and for
 *                             pt_temporal_set_motion below.
 *   pt_read_object_ids      : ids = width*height int32, row-major.  Valid exactly when pt_read_features is and the frame recorded
 *                             ids; PT_ERR_STATE otherwise.  Gathered on devices[0] like the sample counts.
 *
 * Variance-guided a-trous filter on linear radiance (additive to ABI 4; the model and its order of evaluation are
 * stated in csrc/pt_atrous.h).  With c = S / n the pixel's mean and var the variance of that mean (the (v_r + v_g + v_b) / 3 of
 * pt_noise_estimate, with the pixel's own n), `iterations` passes of a 5x5 B3-spline kernel at strides 1, 2, 4, ... weight tap j of
 * pixel i by exp(-pen),
 *     pen = |l_i - l_j| / (sigma_l * sqrt(var_i) + 1e-8) + max(0, 1 - N_i . N_j) / sigma_n
 *         + |z_i - z_j| / (sigma_z * max(z_i, 1e-8)) + |A_i - A_j|^2 / sigma_a^2
 * (l = the mean of the three channels of the current iteration; N, A, z = the feature sums over the samples that hit), and carry the
 * variance along (var' = sum of w^2 var_j / (sum of w)^2).  A frame without features runs with the three feature terms off, whatever
 * the sigmas.  A pixel whose mean or variance is NaN or infinite is passed through and never read as a tap (bad_pixels counts them).
 *   rgba  : the CPU engine's finish of the filtered mean (sqrt, * 255.999, clamp, truncate, NaN -> 0, A = 255); may be NULL
 *           (a GL-shaded frame, pt_set_shading_features: GL's tone map of the filtered mean)
 *   mean  : optional width*height*3 doubles, the filtered mean;  var : optional width*height doubles, its variance
 *   noise_before / noise_after : sqrt(sum of var / max(l, 0.01)^2 / pixels) of the input and of the output; noise_before is
 *                                pt_noise_estimate's figure.  Reduced over a fixed tree: the same bits every time.
 * cfg == NULL: 5 iterations, sigma_l 4, sigma_n 0.1, sigma_z 0.1, sigma_a 0.2.  NaN or negative sigmas, sigma_l <= 0 and iterations
 * outside 0..6 are PT_ERR_INVALID.  Valid when pt_read_moments is -- also between two pt_steps, for previews -- and every pixel holds
 * at least 2 samples; otherwise, and for a frame rendered with GL shading without pt_set_shading_features, PT_ERR_STATE.  A pure read: the sums, the counts and
 * whatever a later pt_step or read sees stay as they are.  Runs on devices[0].
 * Known limit: the weights are relative to each pixel's own noise, so the relative error falls while the plain, un-normalised squared
 * error of a frame dominated by a few very bright pixels (emitters seen directly) can rise.
 */
typedef struct pt_atrous_config {
    int32_t iterations;   /* 0..6; 0 = finish only */
    int32_t reserved;
    double sigma_l;       /* > 0: luminance, in standard deviations of the pixel's mean */
    double sigma_n;       /* >= 0, 0 = term off: normal */
    double sigma_z;       /* >= 0, 0 = term off: relative first-hit distance */
    double sigma_a;       /* >= 0, 0 = term off: albedo */
} pt_atrous_config;

typedef struct pt_atrous_stats {
    double atrous_ms;     /* device time first filter launch -> last filter launch complete (the gathers are not in it) */
    int32_t launches;     /* prep + noise + iterations + noise + finish */
    int32_t iterations;
    double noise_before;
    double noise_after;
    uint64_t bad_pixels;
} pt_atrous_stats;

int32_t pt_set_features(pt_ctx *ctx, int32_t k);
int32_t pt_read_features(pt_ctx *ctx, double *normal, double *albedo, double *depth);
int32_t pt_set_feature_walk(pt_ctx *ctx, int32_t on);
int32_t pt_feature_walk_stats(pt_ctx *ctx, uint64_t out[4]);
int32_t pt_set_shading_features(pt_ctx *ctx, int32_t on);
int32_t pt_set_object_ids(pt_ctx *ctx, int32_t on);
int32_t pt_read_object_ids(pt_ctx *ctx, int32_t *ids);
int32_t pt_atrous(pt_ctx *ctx, const pt_atrous_config *cfg, uint8_t *rgba, int32_t stride, double *mean, double *var,
                  pt_atrous_stats *stats);

/*
 * Half-buffer sums and the measured noise of the filtered frame (additive to ABI 4; the model and its order of
 * evaluation are stated in csrc/pt_atrous.h, HALVES).  pt_atrous's noise_after is the model's own propagated variance and reports half
 * to two thirds of the noise that is really left; the figure here is measured: the samples of every pixel are split into the even-
 * indexed half A and the odd-indexed half B, each half is filtered as a frame of its own, and ((fA - fB) / 2)^2 estimates the variance of
 * (fA + fB) / 2 with no assumption about the taps, since the halves share no sample.  Off unless asked for: with halves off nothing is
 * allocated or launched.
 *   pt_set_halves(ctx, on)  : default 0; later frames on ctx (pt_begin ... pt_end, pt_render) also collect, per pixel and channel, four
 *                             raw sums, each added in sample order: SA = sum of L and QA = sum of L*L over the pixel's samples with an
 *                             even 0-based index, SB and QB over the odd ones (L as in pt_set_moments: after the fog term).  96 B per
 *                             pixel on the devices, outside PTCORE_L_BUDGET_MB.  Such frames collect second moments whether or not
 *                             pt_set_moments asked.  pt_render_tiles_device neither collects nor fails.  PT_ERR_STATE while a frame
 *                             is open.
 *   pt_read_halves          : sa / qa / sb / qb = width*height*3 doubles each, row-major like accum, any of them NULL.  Valid exactly
 *                             when pt_read_moments is; PT_ERR_STATE otherwise and for a frame rendered with halves off.
 *   pt_atrous_halves        : with a pixel's count n, nA = (n + 1) / 2 and nB = n / 2: fA = pt_atrous's model on (SA, QA, nA) and the
 *                             frame's feature planes, fB the same on (SB, QB, nB); per pixel mean = (fA + fB) / 2 and
 *                             err = mean over the channels of ((fA - fB) / 2)^2.
 *       mean       : optional width*height*3 doubles, the combined mean.  As an image it is somewhat worse than pt_atrous's (weights from
 *                    half the samples are noisier): this call is the meter, pt_atrous makes the picture.
 *       err        : optional width*height doubles.  A one-degree-of-freedom estimate per pixel: only meaningful averaged over many
 *                    pixels, as `noise` does.
 *       half_means : optional 2*width*height*3 doubles, fA then fB
 *       noise      : sqrt(sum of err / max(l, 0.01)^2 / pixels), l = the mean of mean's three channels; a pixel that is bad in either
 *                    half, or whose term is NaN or infinite, adds 0 and is counted in bad_pixels.  Reduced over a fixed tree: the
 *                    same bits every time.
 *       noise_model: the same figure with (varA' + varB') / 4, the halves' propagated variances, in place of err: the optimistic
 *                    estimate, beside the measured one so that the gap is visible.
 *   Neither figure sees the bias the filter adds.  cfg as for pt_atrous, with the same PT_ERR_INVALID refusals.  Valid when
 *   pt_read_halves is and every in-frame pixel holds at least 4 samples, so that each half has a variance (an adaptive frame: set
 *   min_spp >= 4); otherwise PT_ERR_STATE, with the smallest count named in the message, and PT_ERR_STATE for a frame rendered with GL
 *   shading.  A pure read, also between two pt_steps; every refusal leaves the context usable.  Runs on devices[0].
 */
typedef struct pt_halves_stats {
    double atrous_ms;     /* device time first launch -> last launch complete (the gathers are not in it) */
    int32_t launches;     /* prep + iterations + combine */
    int32_t iterations;
    double noise;
    double noise_model;
    uint64_t bad_pixels;
    int32_t spp_min;      /* the smallest count a pixel of the frame holds */
    int32_t reserved;
} pt_halves_stats;

int32_t pt_set_halves(pt_ctx *ctx, int32_t on);
int32_t pt_read_halves(pt_ctx *ctx, double *sa, double *qa, double *sb, double *qb);
int32_t pt_atrous_halves(pt_ctx *ctx, const pt_atrous_config *cfg, double *mean, double *err, double *half_means,
                         pt_halves_stats *stats);

/*
 * Adaptive sampling by the pooled noise of the filtered frame (additive to ABI 4; the model and its order of
 * evaluation are stated in csrc/pt_atrous.h, BLOCKS).  pt_set_adaptive stops a block by the noise of its unfiltered pixels, and
 * pt_atrous_halves' measured figure can only stop a whole frame; this rule stops the 8x8 blocks of an adaptive frame by the noise that is
 * left in the filtered frame around them.  Off unless asked for: with the rule off nothing is allocated or launched.
 *   pt_set_adaptive_filtered(ctx, &f) : later adaptive frames on ctx take their block decisions from this rule; NULL = off (the
 *                             default).  The target, min_spp and step are pt_set_adaptive's; a min_spp below 4 counts as 4.  Such a
 *                             frame is adaptive in every respect (counts, pt_read / pt_end by each pixel's own count, pt_adaptive_state,
 *                             pt_read_sample_counts) and collects the half-buffer sums whether or not pt_set_halves asked.  At the end of
 *                             every pt_step, once the samples done reach max(min_spp, 4): pt_atrous_halves' model with `filter` on the
 *                             frame as it stands gives err per pixel; per block B of the frame's 8x8 grid, s_B = the sum of
 *                             err / max(l, 0.01)^2 over its k_B pixels inside the frame (pt_atrous_halves' `noise` term: a pixel that is
 *                             bad or whose term is not finite adds 0 and still counts);
 *                             P_B = sqrt(sum of s_B' / sum of k_B') over the blocks within `pool` blocks of B in x and in y that lie inside
 *                             the grid, stopped blocks included with the samples they hold; every still-active block with
 *                             P_B <= target becomes inactive and stays so.  Every sum has a stated order: the same bits for every
 *                             spp_chunk, buffer budget, scan form and device count.  Unlike pt_set_adaptive's rule, neighbouring blocks
 *                             do keep each other alive: that is what the pool is for, since err has one degree of freedom per pixel.
 *                             pool = 0 judges every block by itself.  The figure inherits the limit of `noise`: where rare bright paths
 *                             were missed it overstates or misses them, and it does not see the filter's bias.
 *                             PT_ERR_STATE while a frame is open; PT_ERR_INVALID for a pool outside 0..4 and for pt_atrous's own
 *                             refusals of `filter`.  A frame opened with the rule on and pt_set_adaptive off is PT_ERR_INVALID, before
 *                             anything is launched and with the context left usable; the refusals of adaptive frames stay as they are.
 *   pt_read_block_figures   : of the last check that decided, row-major over the frame's grid of ((width + 7) / 8) x ((height + 7) / 8)
 *                             blocks: pooled = P_B, own = sqrt(s_B / k_B), either of them NULL; *checks = the checks that have decided
 *                             so far in the frame.  PT_ERR_STATE when the open or last frame did not use the rule or no check has
 *                             decided yet.
 *   pt_adaptive_state.worst_active is, for such frames, the largest P_B among the active blocks (+inf before the first decision).
 * The check runs on devices[0]; the map of flags and figures travels to the other devices through the host.
 */
typedef struct pt_adaptive_filtered {
    pt_atrous_config filter;
    int32_t pool;      /* radius of the window in blocks, 0..4 */
    int32_t reserved;
} pt_adaptive_filtered;

int32_t pt_set_adaptive_filtered(pt_ctx *ctx, const pt_adaptive_filtered *f);
int32_t pt_read_block_figures(pt_ctx *ctx, double *pooled, double *own, int32_t *checks);

/*
 * Temporal accumulation (additive to ABI 4; the model and its order of evaluation are stated in csrc/pt_temporal.h):
 * for a caller that renders frame after frame while the camera moves.  The context keeps a history -- per pixel a blended mean, the
 * variance of that mean, the number of frames behind it, and the first-hit normal, albedo and distance it belongs to -- with the camera
 * it was seen from.  pt_temporal finds, for every pixel of the current frame, where its first hit (or, for a pixel that sees the sky,
 * its direction) lay in the previous frame, reads the history there (bilinear; a tap counts only where distance, normal and albedo
 * agree), blends the frame's own mean into it with weight a = max(alpha, 1 / (len + 1)), stores the result as the new history and
 * then, unless `filter` is NULL, runs pt_atrous's filter on the blended mean and variance with this frame's feature planes.  Off
 * unless called: until the first pt_temporal nothing is allocated or launched.
 *   cfg == NULL : alpha 0.2, max_len 32, tol_z 0.1, n_min 0.9, tol_a 0.05.  A NaN, alpha outside [0, 1], max_len < 1 or a negative
 *                 tolerance is PT_ERR_INVALID.
 *   filter      : NULL = no filter (the output is the blended frame); otherwise as pt_atrous's cfg, with the same PT_ERR_INVALID
 *                 refusals.  (pt_atrous's defaults: pass a config with 5, 0, 4.0, 0.1, 0.1, 0.2.)
 *   rgba, stride, mean, var : as pt_atrous's, of the blended (and filtered) frame; any may be NULL
 *   reprojected / disoccluded : good pixels that found history / that did not although the history was not empty
 *   mean_len    : the mean of the new history's len over the frame's pixels (a bad pixel counts 0)
 *   noise_before / noise_blended / noise_after : pt_atrous's figure of the frame's own (mean, variance) -- pt_noise_estimate's
 *                 figure --, of the blended state and of the output (= noise_blended when filter is NULL).  The blended variance
 *                 (1 - a)^2 var_history + a^2 var_frame assumes that the frames are independent: CHANGE THE SEED FROM FRAME TO FRAME.
 * Valid when pt_atrous is -- also between two pt_steps -- on a frame rendered with features on (pt_set_features, k > 0); otherwise
 * PT_ERR_STATE: features off, GL shading, a pixel with fewer than 2 samples.  A second call for the same frame at the same number
 * of samples done is PT_ERR_STATE too ("already accumulated": it would blend the frame into itself); after a further pt_step the
 * call is valid again.  Every refusal leaves the context and the history as they were, and the new history replaces the old one
 * only when the call succeeds.  A pure read of the frame: sums, counts and later pt_steps are unaffected.  Runs on devices[0]; the
 * history takes 192 B per pixel there (two sets of 12 planes), outside PTCORE_L_BUDGET_MB, allocated on the first call.
 *   pt_temporal_read  : the stored history, row-major: mean = width*height*3 doubles, var = width*height doubles,
 *                       len = width*height int32 (0: a bad pixel, never read as a tap); any may be NULL.  PT_ERR_STATE when empty.
 *   pt_temporal_reset : empties the history (after a scene edit, a cut).  The history is also empty after pt_create and is dropped
 *                       by a call whose width x height differs from the history's.
 * The history is keyed by geometry alone: moving or edited objects are caught only by the distance, normal and albedo tests, so
 * the caller resets after an edit -- or, where the edit moved objects and nothing else, passes their displacements
 * (pt_temporal_set_motion below).  Known limit: ghosting of view-dependent content.  Where what is seen at a pixel changes while
 * its first-hit normal, distance and albedo still agree (a reflection, a refraction, a moving shadow edge), every tap passes and the
 * history overrules the frame with another view's radiance; on test_scene that costs more than the history gains.
 * The answer is the clip below.  (Firefly rejection in the frame is not done; the test sequences contain no firefly.)
 *
 * The history clip (additive to ABI 4; step 7a of csrc/pt_temporal.h): before the blend the reprojected history
 * mean is clamped, per channel, to the frame's mean +- gamma * sqrt(var_frame + var_history).  It rectifies the history and rejects
 * nothing in the frame: a noisy frame pixel has a wide interval.  Where both variances are zero the history becomes the frame.
 *   pt_temporal_set_clip   : gamma for later pt_temporal calls of this context; it may change between frames of one history.
 *                            0 = off, the default after pt_create: pt_temporal then gives the bits it gave before the clip existed.
 *                            RECOMMENDED: 2.5 (the smallest of 2, 2.5, 3 that gains on test_scene and costs no other shipped scene
 *                            more than a twentieth).  NaN, negative or infinite: PT_ERR_INVALID.
 *   pt_temporal_clip_stats : of the last pt_temporal that succeeded: the gamma it ran with, the reprojected pixels and those of them
 *                            whose history the clip changed (0 when it ran with the clip off).  PT_ERR_STATE while the history is
 *                            empty.  The struct shares its name with the function: write `struct pt_temporal_clip_stats`.
 * Every refusal leaves the context and the history as they were.
 *
 * Displaced reprojection (additive to ABI 4; step 4a of csrc/pt_temporal.h): for an editor whose user drags objects.
 * A half-pixel move of an object passes the distance, normal and albedo tests, so without this the history of the place where the
 * object was is blended into the place where it is.  The scene schema has positions and sizes and no rotations: a translation per
 * object is every edit of geometry short of a resize.
 *   pt_temporal_set_motion   : delta = [num_objects][3] doubles: for object i of pt_scene.objects, its position in the frame about to
 *                              be accumulated minus its position in the frame the history was stored from.  The table is copied.
 *                              NULL or 0 clears it.  A NaN or infinite entry, or num_objects < 0, is PT_ERR_INVALID.  (A table
 *                              that cannot be held is PT_ERR_NOMEM and leaves the pending one as it was.)  ONE-SHOT: the
 *                              table is consumed by the next pt_temporal that succeeds, also when that call finds the history empty;
 *                              a refused pt_temporal leaves it set, pt_temporal_reset drops it.  With a table pending, pt_temporal is
 *                              refused with PT_ERR_STATE when the frame recorded no object ids (pt_set_object_ids) and with
 *                              PT_ERR_INVALID when num_objects differs from the frame's scene.  On a pixel whose sample 0 hit object o
 *                              with delta[o] != 0 the point that is projected into the previous frame is the hit point minus
 *                              delta[o]; everything else -- taps, tests, clip, blend, the stored history -- is unchanged, and an
 *                              all-zero table gives the bits of no table.  RECOMMENDED with it: the clip at 2.5, since the radiance on
 *                              and near a moved object changes (its reflections, its shadow).  Limits: the id is sample 0's while
 *                              normal, albedo and depth are means over k samples, so silhouette pixels are left to the tap tests;
 *                              the strip an object uncovers is disoccluded and starts at len 1; resizes, material edits and sky
 *                              edits are not motion -- reset.
 *   pt_temporal_motion_stats : of the last pt_temporal that succeeded: objects = the table's length (0: it ran without one), moved =
 *                              good hit pixels whose object had a non-zero delta, moved_reprojected = those of them that found
 *                              history.  PT_ERR_STATE while the history is empty.  The struct shares its name with the function.
 * Every refusal leaves the context, the history and the table as they were.
 */
typedef struct pt_temporal_config {
    double alpha;         /* 0..1: the least weight of the current frame */
    double tol_z;         /* >= 0: relative first-hit distance a tap may be off by */
    double n_min;         /* the least N_i . N_h of a tap */
    double tol_a;         /* >= 0: the albedo distance a tap may be off by */
    int32_t max_len;      /* >= 1: the history length saturates here */
    int32_t reserved;
} pt_temporal_config;

typedef struct pt_temporal_stats {
    double temporal_ms;   /* device time first launch -> last launch complete (the gathers are not in it) */
    int32_t launches;     /* temporal + noise [+ iterations + noise] + finish */
    int32_t iterations;   /* of the filter; 0 without one */
    uint64_t reprojected;
    uint64_t disoccluded;
    uint64_t bad_pixels;
    double mean_len;
    double noise_before;
    double noise_blended;
    double noise_after;
} pt_temporal_stats;

int32_t pt_temporal(pt_ctx *ctx, const pt_temporal_config *cfg, const pt_atrous_config *filter, uint8_t *rgba, int32_t stride,
                    double *mean, double *var, pt_temporal_stats *stats);
int32_t pt_temporal_read(pt_ctx *ctx, double *mean, double *var, int32_t *len);
int32_t pt_temporal_reset(pt_ctx *ctx);

struct pt_temporal_clip_stats {
    double gamma;         /* what the call ran with; 0 = the clip was off */
    uint64_t clipped;     /* reprojected pixels with at least one channel of the history changed */
    uint64_t reprojected;
};

int32_t pt_temporal_set_clip(pt_ctx *ctx, double gamma);
int32_t pt_temporal_clip_stats(pt_ctx *ctx, struct pt_temporal_clip_stats *out);

struct pt_temporal_motion_stats {
    int32_t objects;      /* the length of the table the call ran with; 0 = without one */
    int32_t reserved;
    uint64_t moved;       /* good hit pixels whose object had a non-zero delta */
    uint64_t moved_reprojected;
};

int32_t pt_temporal_set_motion(pt_ctx *ctx, const double *delta, int32_t num_objects);
int32_t pt_temporal_motion_stats(pt_ctx *ctx, struct pt_temporal_motion_stats *out);

/*
 * Refit of the bounding-volume hierarchy on the devices (additive to ABI 4).  Off by default: with it off every
 * call, launch and bit is what it is without these entry points.
 * A scene on the bounding-volume-hierarchy path (more than 128 spheres or 128 boxes) has its hierarchy built on the host whenever
 * the scene changed.  With the refit on, a frame whose scene differs from the previous frame's only in where its objects are and
 * how large -- positions and sizes of spheres and boxes (a zero or negative radius included), glass objects among them, and the
 * positions of planes; the same materials, the same object count, every object's type and material unchanged, every coordinate
 * below 1e37, the same scan -- keeps the hierarchy's topology: each device recomputes the boxes of the tree it holds from the edited
 * objects, level by level from the leaves (one small launch per level of the tree; csrc/pt_bvh_refit.h states the bits).  The boxes hold their objects, so
 * the frame is the one a full build gives, bit for bit; what degrades is how fast it is traced.  Any other edit, PTCORE_PIPELINE=
 * walk32 and scenes on the other scans build in full as before.
 *   pt_set_bvh_refit(ctx, max_growth) : 0 = off (the default); >= 1 or +inf = on; NaN, negative values and values in (0, 1) are
 *                             PT_ERR_INVALID; PT_ERR_STATE while a frame is open.  The quality figure of a tree is the sum over the
 *                             main tree's nodes of the half areas dx dy + dy dz + dz dx of their slots' exact boxes, added in a
 *                             fixed order.  When the tree a frame was rendered with is a refitted one whose figure exceeds
 *                             max_growth x the figure at the last full build, the next frame -- also one with an unchanged scene --
 *                             builds in full first: a degraded tree serves one frame at the most.  Recommended: 1.25, the ratio at which
 *                             one rebuild of a 10^5-object scene repays itself within about 12 frames.
 *   pt_bvh_refit_stats      : since pt_create; PT_ERR_STATE before the first frame.  cost_now is that of devices[0]'s tree.
 *   pt_debug_bvh_refit_check: diagnostics only, no GPU needed.  Builds the hierarchy of `before`, refits it to `after` on the
 *                             host and reports out = {nodes, objects, 0 or the PT_BVH_REASON_* that forbids the refit (the checks
 *                             then run on a full build of `after`), objects not inside their slot's box, child boxes not inside
 *                             their parent's, nodes (and object records) whose bytes differ from a fresh encode of the same
 *                             topology, the figure ratio x 1000, nodes whose topology words changed (must be 0)}.
 */
enum {
    PT_BVH_REASON_NONE = 0,       /* no full build yet / the edit is refittable */
    PT_BVH_REASON_FIRST = 1,      /* the context's first scene */
    PT_BVH_REASON_OFF = 2,        /* pt_set_bvh_refit is off */
    PT_BVH_REASON_CHANGED = 3,    /* materials, object count, an object's type or material changed */
    PT_BVH_REASON_NOT_BVH = 4,    /* not on the bounding-volume-hierarchy path, another scan asked for, or walk32 */
    PT_BVH_REASON_GROWTH = 5,     /* the refitted tree's figure exceeded max_growth x the built one's */
    PT_BVH_REASON_NONFINITE = 6   /* a coordinate of 1e37 or more (also when the last scene was off the hierarchy for it) */
};

struct pt_bvh_refit_stats {
    uint64_t builds;              /* full scene preparations */
    uint64_t refits;              /* preparations served by a refit */
    int32_t last_action;          /* of the last frame's preparation: 0 = nothing (scene unchanged), 1 = full build, 2 = refit */
    int32_t last_build_reason;    /* PT_BVH_REASON_* of the last full build */
    double cost_built;            /* the figure at the last full build (0 unless the refit was on, or a refit has run since) */
    double cost_now;              /* ... and of the tree the last frame was rendered with */
    double refit_ms;              /* device time of the last refit on devices[0] */
};

int32_t pt_set_bvh_refit(pt_ctx *ctx, double max_growth);
int32_t pt_bvh_refit_stats(pt_ctx *ctx, struct pt_bvh_refit_stats *out);
int32_t pt_debug_bvh_refit_check(const pt_scene *before, const pt_scene *after, int32_t out[8]);

/*
 * Build of the bounding-volume hierarchy on the device (additive to ABI 4).  Off by default: with it off every
 * call, launch and bit is what it is without these entry points.
 * Whenever a scene on the bounding-volume-hierarchy path changed in a way a refit cannot serve -- an object added or removed, a
 * material or a type changed, a context's first frame, a refitted tree that outgrew its bound -- the hierarchy is built on the host,
 * single-threaded, by a binned surface-area-heuristic builder.  With mode 1 devices[0] builds it instead, in Morton order (keys from
 * the objects' centroids, a stable radix sort, a binary radix tree, boxes bottom-up, a collapse to 4-wide nodes level by level;
 * csrc/pt_bvh_build.h states every step once for the host and the device), in the same node format, numbering and payload bytes.
 * The tree is read back and from there on handled as the host builder's: the other devices receive it, a refit keeps its topology
 * and is held against its figure.  Its boxes hold their objects, so the frame is the one the host-built tree gives, bit for bit;
 * what differs is how long the build takes and how fast the tree is traced (DESIGN.md 3.4d has the figures).
 *   pt_set_bvh_build(ctx, mode): 0 = host (the default), 1 = device; other values PT_ERR_INVALID; PT_ERR_STATE while a frame is open.
 *                             Takes effect at the next full build.  The host builder still serves, by reason and never as an error:
 *                             a device-built tree too deep for the traversal stack, PTCORE_PIPELINE=walk32 (its core twins are
 *                             not built on the device), and scenes on the other scans, which have no tree.
 *   pt_bvh_build_stats      : since pt_create; PT_ERR_STATE before the first frame.  builder, nodes, depth, stack_need and cost
 *                             describe the tree of the last full preparation (builder 0: that scene has none).  cost is the refit's
 *                             figure (pt_set_bvh_refit) of the tree as built; it is computed when the device build or the refit is
 *                             on and is 0 otherwise.
 *   pt_debug_bvh_build_check: diagnostics only, no GPU needed.  Runs the host restatement of the device build on `scene` and reports
 *                             out = {nodes, objects, depth, stack_need, objects not reached exactly once, objects not inside their
 *                             slot's box, child boxes not inside their parent's, structural faults (children or objects not
 *                             consecutive, a level table that does not increase, bytes a refit to the same world changes)}.
 */
enum { PT_BVH_BUILDER_NONE = 0, PT_BVH_BUILDER_HOST = 1, PT_BVH_BUILDER_DEVICE = 2 };
enum {
    PT_BVH_BUILD_FALLBACK_NONE = 0,     /* the selected builder built the tree */
    PT_BVH_BUILD_FALLBACK_STACK = 1,    /* the device-built tree is too deep for the traversal stack */
    PT_BVH_BUILD_FALLBACK_WALK32 = 2,   /* PTCORE_PIPELINE=walk32 */
    PT_BVH_BUILD_FALLBACK_NOT_BVH = 3   /* the scene is not on the bounding-volume-hierarchy path: no tree */
};

struct pt_bvh_build_stats {
    uint64_t host_builds;         /* hierarchies built by the host builder */
    uint64_t device_builds;       /* ... and on devices[0] */
    int32_t builder;              /* PT_BVH_BUILDER_* of the tree of the last full preparation */
    int32_t last_fallback;        /* PT_BVH_BUILD_FALLBACK_* of the last full preparation while mode 1 was set */
    int32_t nodes;                /* both trees */
    int32_t depth;                /* levels of wide nodes */
    int32_t stack_need;           /* entries a traversal can have pushed at once */
    int32_t reserved;
    double cost;                  /* the figure of the main tree as built */
    double device_ms;             /* device time of the last device build, first launch to last */
    double prepare_ms;            /* wall time of the last full scene preparation, from its first line: converting the scene,
                                     comparing it with the previous one, the build */
    double upload_ms;             /* of the last device build: host wall time of its allocations and the world's upload */
    double readback_ms;           /* ... and of reading nodes and records back, from the end of the last launch */
};

int32_t pt_set_bvh_build(pt_ctx *ctx, int32_t mode);
int32_t pt_bvh_build_stats(pt_ctx *ctx, struct pt_bvh_build_stats *out);
int32_t pt_debug_bvh_build_check(const pt_scene *scene, int32_t out[8]);

/*
 * Diagnostics only (not part of the rendering boundary): with PTCORE_PROFILE=1 in the
 * environment at pt_create, the trace kernel runs a build that counts, per code
 * section, wave executions, active lanes and shader-clock cycles.  Copies up to n
 * values of the last collected frame ([section][executions, lanes, cycles]) and
 * returns the number available (negative status is impossible: errors return PT_ERR_*
 * as positive codes <= 5, counts are >= 6).
 */
int32_t pt_debug_profile(pt_ctx *ctx, uint64_t *out, int32_t n);

/* Diagnostics only: with PTCORE_SCAN=verify at pt_create the trace kernel runs BOTH closest-hit
 * strategies (the FP32-culled one and the plain every-object FP64 scan) for every segment, renders
 * with the plain one and counts the segments on which the two disagree.  Returns that count,
 * accumulated over every frame finished in this process (0 = the culling never changed a result). */
int64_t pt_debug_scan_mismatches(pt_ctx *ctx);

/* Diagnostics only: the narrow phase and Russian roulette divide several numerators by one denominator and share the
 * reciprocal refinement of the IEEE division between them (div_shared in csrc/pt_kernels.h).  Compares that form with
 * the plain division, bit for bit, on `millions` x 10^6 random and patterned operand pairs on the GPU and returns the
 * number of pairs that differ (must be 0), or -PT_ERR_* on failure. */
int64_t pt_debug_div_selftest(pt_ctx *ctx, int32_t millions, uint64_t seed);

/* Diagnostics only, no GPU needed: builds the bounding-volume hierarchy used for scenes with more
 * than 128 spheres or 128 boxes and checks its invariants.  out = {nodes, objects in the tree, depth, most slots
 * used by a node (<= 4), objects or nodes not reached exactly once, objects not inside their slot's box,
 * child boxes not inside the parent's box, planes kept outside the tree}. */
int32_t pt_debug_bvh_check(const pt_scene *scene, int32_t out[8]);

/* Diagnostics only: replaces the primary rays of later frames on ctx.  `rays` is [n][6] doubles (origin x y z, direction x y z),
 * the ray of pixel (x, y), sample s at index (y*width + x)*samples_per_px + s; the table is copied.  rays == NULL or n == 0 clears
 * it (the default: the camera's rays).  While a table is set, every chunk's ray generation still runs -- stream state and draw
 * counts are the camera's -- and a small kernel then overwrites the rays, so the chosen rays go through the shipped trace
 * kernels of every form (split, nested, all-in-one, grouped, hierarchy with its primary pass, wavefront, walk32) untouched.  A
 * frame whose width*height*samples_per_px differs from n fails with PT_ERR_INVALID; with fog on (pt_set_fog), GL shading
 * (pt_set_shading) or several devices in the context it fails with PT_ERR_STATE.  Nothing is launched in either case and the
 * context stays usable.  Any double is a legal component (zeros, subnormals, infinities, NaN): such rays take the reference's
 * own scan. */
int32_t pt_debug_set_primary_rays(pt_ctx *ctx, const double *rays, int64_t n);

/* Diagnostics only: how a context that holds several devices collects the tiles of a frame on devices[0]: 0 = one
 * hipMemcpyPeerAsync per peer (the default), 1 = grouped ncclSend / ncclRecv through librccl.so (PTCORE_GATHER=rccl at
 * pt_create; the library is dlopen'ed then and only then). */
int32_t pt_debug_gather_mode(pt_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* PTCORE_H */
