/*
 * pt_oracle.h -- TEST INFRASTRUCTURE ONLY.
 *
 * CPU restatement (plain C, FP64, no FMA contraction) of the reference's Go CPU
 * engine, package internal/engine of MarkJulian19/path_trace_golang.  It is the
 * parity checker for the HIP path and the timed "port" CPU baseline of bench.py.
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load
 * it; the product (path_trace_golang_amd/, include/) never does.
 *
 * PARITY UNPINNED BY THE REFERENCE: the reference ships no tests, golden images
 * or known-answer vectors, its Go toolchain is absent here, and its RNG is
 * time-seeded (internal/engine/random.go:14-16), so no reference output exists
 * to pin this restatement against.  It is pinned instead by hand-derived KATs
 * and closed-form scenes (tests/test_oracle_*.py); see DESIGN.md.
 *
 * The structs below carry exactly the scene.Scene fields the CPU engine reads
 * (internal/scene/scene.go:9-158); convertMaterial and sceneToWorld are
 * restated inside the oracle, not in the harness.
 */
#ifndef PT_ORACLE_H
#define PT_ORACLE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* scene.Material (scene.go:41-63), fields read by convertMaterial (materials.go:28-55) */
typedef struct {
    int32_t type;        /* 0 lambert (also any unknown string), 1 metal, 2 dielectric, 3 emissive, 4 mirror */
    int32_t _pad;
    double albedo[3];
    double rough;
    double ior;
    double emit[3];
    double power;
    double absorption[3];
    double smoothness;
} ora_material;

/* scene.Object (scene.go:76-84) */
typedef struct {
    int32_t type;        /* 0 sphere, 1 plane, 2 box, 3 sphere_light, -1 unknown (skipped, objects.go:237-266) */
    int32_t material;    /* index of the LAST material with that id, -1 = id not present -> zero material (objects.go:233) */
    double position[3];
    double size[3];
} ora_object;

/* scene.Camera (scene.go:24-32) */
typedef struct {
    double position[3], target[3], up[3];
    double fov, aperture, focus_dist, aspect_ratio;
} ora_camera;

/* scene.Sky + scene.Background as the closure of renderer.go:56-92 sees them */
typedef struct {
    int32_t sky_type;    /* 0: sky == nil or type not in {gradient, solid} -> background; 1 gradient; 2 solid */
    int32_t _pad;
    double background[3], color[3], horizon[3], zenith[3];
} ora_sky;

typedef struct {
    ora_camera camera;
    ora_sky sky;
    int32_t nmaterials, nobjects;
    const ora_material *materials;
    const ora_object *objects;
} ora_scene;

typedef struct {
    int32_t width, height, spp, max_depth;
    uint64_t seed;
    int32_t workers;     /* 0 = PATHTRACER_WORKERS or online CPUs (renderer.go:117-129) */
    int32_t _pad;
} ora_config;

typedef struct {
    uint64_t samples;    /* W*H*spp */
    uint64_t segments;   /* rayColorOpt activations with depth > 0 (closest-hit scans) */
    uint64_t exit_scans; /* dielectric exit searches (renderer.go:316-371) */
    uint64_t draws;      /* RNG draws */
    double seconds;      /* wall time of the pixel loop */
    int32_t workers;
    int32_t _pad;
} ora_stats;

/*
 * Renders like renderIntoCPU (renderer.go:44-246).
 *   rgba    : H rows of `stride` bytes, row 0 = top (may be NULL)
 *   accum   : W*H*3 doubles, per pixel the raw sum over samples of the sample
 *             radiance, before the 1/spp scale (may be NULL)
 *   nseg    : W*H uint32, per pixel segment count (may be NULL)
 *   ndraw   : W*H uint32, per pixel RNG draw count (may be NULL)
 * Returns 0.  If x0/y0/x1/y1 window is non-empty only those pixels are done.
 */
int ora_render(const ora_scene *sc, const ora_config *cfg, uint8_t *rgba, int32_t stride,
               double *accum, uint32_t *nseg, uint32_t *ndraw, ora_stats *stats);

/* Same, restricted to pixel window [x0,x1) x [y0,y1) of the full W x H frame;
 * buffers are still full-frame sized and only the window is written. */
int ora_render_window(const ora_scene *sc, const ora_config *cfg, int32_t x0, int32_t y0, int32_t x1,
                      int32_t y1, uint8_t *rgba, int32_t stride, double *accum, uint32_t *nseg,
                      uint32_t *ndraw, ora_stats *stats);

/* One sample's radiance for pixel (x, y), sample s: the value renderer.go:186 adds. */
void ora_sample(const ora_scene *sc, const ora_config *cfg, int32_t x, int32_t y, int32_t s,
                double out_rgb[3], uint32_t *nseg, uint32_t *ndraw);

/* Test hooks for chosen primary rays.  ora_primary_ray: the ray sample_once traces for (x, y, s), i.e. what camera.getRay
 * returned (renderer.go:181-184).  ora_sample_ray: ora_sample with that ray replaced by (orig, dir) after getRay -- the camera
 * draws still happen, so the stream and the draw count line up with a renderer that generated a ray and dropped it.
 * ora_sample_rays: the same for n consecutive samples in table order from (x, y, s) on (s fastest, then x, then y: ray k of a
 * whole-frame table has index (y*width + x)*spp + s); rays is [n][6] (origin, direction), out_rgb [n][3], nseg / ndraw [n] or
 * NULL. */
void ora_primary_ray(const ora_scene *sc, const ora_config *cfg, int32_t x, int32_t y, int32_t s, double orig[3], double dir[3]);
void ora_sample_ray(const ora_scene *sc, const ora_config *cfg, int32_t x, int32_t y, int32_t s, const double orig[3],
                    const double dir[3], double out_rgb[3], uint32_t *nseg, uint32_t *ndraw);
void ora_sample_rays(const ora_scene *sc, const ora_config *cfg, int32_t x, int32_t y, int32_t s, int64_t n, const double *rays,
                     double *out_rgb, uint32_t *nseg, uint32_t *ndraw);

/* ---- unit-level entry points for KATs ---- */
double ora_sin(double x);   /* Go math.Sin (Cephes), pure-Go path */
double ora_cos(double x);
double ora_tan(double x);
double ora_exp(double x);   /* Go math.Exp, pure-Go (FreeBSD) path */
double ora_pow(double x, double y); /* Go math.Pow; only integral y >= 0 supported here */
double ora_min(double a, double b); /* Go math.Min special cases */
double ora_max(double a, double b);
uint64_t ora_stream_init(uint64_t seed, uint64_t pixel, uint64_t sample);
double ora_stream_next(uint64_t *state);

/* hit tests: obj = {kind 0 sphere / 1 plane / 2 box, a[3], b[3], radius};
 * out = {t, p[3], normal[3], frontFace}. Returns 1 on hit. */
int ora_hit(int32_t kind, const double a[3], const double b[3], double radius, const double orig[3],
            const double dir[3], double tmin, double tmax, double out[8]);
/* n cases of ora_hit, one object each: kind [n], a / b [n][3], radius [n], rays [n][6] (origin, direction), out [n][8], ok [n] */
void ora_hits(int64_t n, const int32_t *kind, const double *a, const double *b, const double *radius, const double *rays,
              double tmin, double tmax, double *out, int32_t *ok);
/* reflectVec (math.go:39-46) on n pairs (v, n): out [n][3] */
void ora_reflects(int64_t n, const double *v, const double *nrm, double *out);
/* converted material: out = {typ, albedo[3], rough, ior, emit[3], absorption[3]} (12 doubles) */
void ora_convert_material(const ora_material *m, double out[12]);
/* what the reference forms from a converted material on every hit: out = {1/ior, reflectance's r0 with ratio = 1/ior, r0 with
 * ratio = ior (materials.go:183, :227-228), rough*rough (materials.go:121), renderer.go:360's absorption test as 0 / 1} */
void ora_material_derived(const ora_material *m, double out[5]);

/* ---- the surface step of rayColorOpt, one call at a time: the same static functions rayColorOpt calls ----
 * ora_scatter_step: renderer.go:308-311 on the record ora_hit returned (hit = its out[8]) and the incoming ray, with the stream
 *   at *state.  out = {emitted[3], attenuation[3], scattered origin[3], scattered direction[3]}; *state and *ndraw (draws taken)
 *   are written; returns scatter's ok.  m == NULL is the zero material of a missing id.
 * ora_exit_step: renderer.go:352-370 with the entry point and the exit record's point, exit_p == NULL when no exit was found;
 *   att and orig (the scattered ray's origin) are updated in place.
 * ora_roulette_step: renderer.go:375-393 at `depth`; att is updated in place.  Returns 0 when the path goes on, 1 when
 *   maxAttenuation < 1e-6 ended it, 2 when the draw did.
 * The array forms run n independent cases.  ora_exit_steps takes the scattered ray [n][6], the exit hit's t and best (< 0: none),
 *   forms the exit point as ray.at does and writes orig [n][3]; ora_roulette_steps also multiplies T [n][3] by the attenuation
 *   of a surviving path (renderer.go:403) and reports 3 when depth - 1 reaches 0 (renderer.go:287-289 of the callee). */
int ora_scatter_step(const ora_material *m, const double hit[8], const double orig[3], const double dir[3], uint64_t *state,
                     double out[12], uint32_t *ndraw);
void ora_exit_step(const ora_material *m, const double entry[3], const double *exit_p, double att[3], double orig[3]);
int ora_roulette_step(int32_t depth, double att[3], uint64_t *state, uint32_t *ndraw);
void ora_scatter_steps(int64_t n, const ora_material *mats, const int32_t *mat, const double *hits, const double *rays,
                       uint64_t *states, double *out, int32_t *ok, uint32_t *ndraw);
void ora_exit_steps(int64_t n, const ora_material *mats, const int32_t *mat, const double *rays, const double *t,
                    const int32_t *best, double *att, double *orig);
void ora_roulette_steps(int64_t n, const int32_t *depth, double *att, double *T, uint64_t *states, int32_t *ended, uint32_t *ndraw);
/* camera: out = origin[3], lowerLeft[3], horizontal[3], vertical[3], u[3], v[3], w[3], lensRadius (22) */
void ora_camera_setup(const ora_camera *c, int32_t width, int32_t height, double out[22]);
/* ---- post-process passes of the reference's GPU backend, CPU restatement ----
 * internal/engine/gpu/gpu.go:22-47 (acesTonemap), :2309-2350 (tone-map + gamma + round), :2355-2439
 * (3x3 bilateral on the 8-bit image), :2444-2520 (box blur blended with the original). */
typedef struct {
    int32_t tonemap;        /* 1: rgba = round(sqrt(aces(float32(accum/spp))) * 255), needs accum */
    int32_t denoise;        /* 1: bilateral 3x3, skipped unless w > 2 && h > 2 (gpu.go:2358) */
    double sigma_s, sigma_r;
    int32_t smooth;         /* 1: box blur, radius clamped to 1..5, strength to 0..1 */
    int32_t smooth_radius;
    double smooth_strength;
} ora_post_config;
void ora_post_process(const ora_post_config *cfg, const double *accum, int32_t spp, uint8_t *rgba, int32_t stride,
                      int32_t width, int32_t height);
float ora_aces_tonemap(float x);

/* pixel finish (renderer.go:190-221): raw sum -> 3 bytes */
void ora_finish_pixel(const double sum[3], int32_t spp, uint8_t out[3]);

#ifdef __cplusplus
}
#endif
#endif
