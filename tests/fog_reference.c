/*
 * fog_reference.c -- TEST INFRASTRUCTURE ONLY: an independent CPU restatement of the fog model of
 * path_trace_golang_amd/csrc/pt_fog.h (the reference's OpenGL fog, internal/engine/gpu/gpu.go:1125-1341 and :2011-2105,
 * in FP64), written against the CPU oracle (oracle/libptoracle.so) and no product header.  tests/test_fog_cpu.py and
 * tests/test_fog_gpu.py compile it with the oracle's flags (no contraction, no fast-math) and load it with ctypes.
 *
 *   fr_resolve    the parameter resolution of gpu.go:2024-2096
 *   fr_sky        the affect_sky rewrite of the sky constants (applyFog(c, 50))
 *   fr_inscatter  the in-scatter term of one (pixel, sample) for a given primary ray
 *   fr_render     a whole frame: per sample ora_sample + the fog term of its regenerated primary ray, summed in sample
 *                 order, finished with ora_finish_pixel
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "pt_oracle.h"

#define FOG_SALT 0x464F475F53545245ULL /* ASCII "FOG_STRE" */
#define PI_GO 3.141592653589793

/* scene.Fog, raw (the layout of pt_fog in include/ptcore.h, restated) */
typedef struct {
    double density, color[3], scatter, sigma_s, sigma_a, g, hetero_strength, noise_scale;
    int32_t noise_octaves, affect_sky, gpu_volumetric, reserved;
} fr_fog;

/* resolved block */
typedef struct {
    double density, scatter, sigma_s, sigma_a, g, hetero, noise_scale, color[3];
    int32_t octaves, affect_sky, volumetric, pad;
} fr_params;

typedef struct {
    int32_t kind; /* 0 sphere, 1 plane, 2 box */
    double a[3], b[3], radius;
} fr_obj;

typedef struct {
    double c[3], radius, le[3];
} fr_light;

typedef struct {
    fr_obj *objs;
    int nobj;
    fr_light *lights;
    int nlight;
} fr_world;

static double clamp01(double x) { return x < 0 ? 0.0 : (x > 1 ? 1.0 : x); }

void fr_resolve(const fr_fog *f, fr_params *p) {
    memset(p, 0, sizeof *p);
    p->density = f->density > 0 ? f->density : 0.0;
    if (f->scatter > 0) p->scatter = f->scatter;
    else if (p->density > 0) p->scatter = 1.0;
    else p->scatter = 0.0;
    if (f->sigma_s > 0 || f->sigma_a > 0) {
        p->sigma_s = f->sigma_s;
        p->sigma_a = f->sigma_a;
    } else if (p->density > 0) {
        double smul = p->scatter;
        if (smul < 0) smul = 0;
        if (smul > 1) smul = 1;
        p->sigma_s = p->density * smul;
        p->sigma_a = p->density - p->sigma_s;
        if (p->sigma_a < 0) p->sigma_a = 0;
    }
    if (f->g < -0.9) p->g = -0.9;
    else if (f->g > 0.9) p->g = 0.9;
    else p->g = f->g;
    if (f->hetero_strength > 0) p->hetero = f->hetero_strength > 1 ? 1.0 : f->hetero_strength;
    p->noise_scale = f->noise_scale > 0 ? f->noise_scale : 4.0;
    if (f->noise_octaves > 0) p->octaves = f->noise_octaves > 5 ? 5 : f->noise_octaves;
    else p->octaves = 3;
    p->color[0] = f->color[0];
    p->color[1] = f->color[1];
    p->color[2] = f->color[2];
    p->affect_sky = f->affect_sky != 0;
    p->volumetric = f->gpu_volumetric != 0;
}

/* applyFog(c, 50) on background, color, horizon, zenith, in that order */
void fr_sky(const fr_fog *raw, ora_sky *sky) {
    fr_params p;
    fr_resolve(raw, &p);
    if (!(p.density > 0 && p.affect_sky)) return;
    double a = ora_exp(-p.density * 50);
    double *cs[4] = {sky->background, sky->color, sky->horizon, sky->zenith};
    for (int k = 0; k < 4; k++)
        for (int i = 0; i < 3; i++) cs[k][i] = cs[k][i] * a + p.color[i] * (1 - a);
}

static double fract(double x) { return x - floor(x); }

static double hash31(double px, double py, double pz) {
    double qx = px * 127.1 + py * 311.7 + pz * 74.7;
    double qy = px * 269.5 + py * 183.3 + pz * 246.1;
    double qz = px * 113.5 + py * 271.9 + pz * 124.6;
    double s = qx + qy + qz;
    if (!(fabs(s) < 536870912.0)) return 0.5; /* Go's Sin is only restated below 2^29 */
    return fract(ora_sin(s) * 43758.5453);
}

static double volume_noise(const fr_params *p, double px, double py, double pz) {
    double amp = 1.0, freq = p->noise_scale, sum = 0.0, norm = 0.0;
    for (int i = 0; i < p->octaves && i < 5; i++) {
        sum += hash31(px * freq, py * freq, pz * freq) * amp;
        norm += amp;
        amp *= 0.5;
        freq *= 2.0;
    }
    if (norm <= 0) return 1.0;
    return sum / norm;
}

/* returns sigma_s, writes sigma_t */
static double medium(const fr_params *p, double px, double py, double pz, double *st) {
    double ss = ora_max(p->sigma_s, 0.0), sa = ora_max(p->sigma_a, 0.0);
    if (ss <= 0 && sa <= 0 && p->density > 0) {
        ss = p->density * clamp01(p->scatter);
        sa = p->density - ss;
        if (sa < 0) sa = 0;
    }
    *st = ss + sa;
    if (*st <= 0) return 0;
    if (p->hetero > 0) {
        double n = volume_noise(p, px, py, pz);
        double k = clamp01(p->hetero);
        double scale = (1 - k) * (1 - n) + (1 + k) * n;
        ss *= scale;
        sa *= scale;
        *st = ss + sa;
    }
    return ss;
}

static double phase_hg(double ct, double g) {
    double gg = g * g;
    double denom = 1 + gg - 2 * g * ct;
    return (1 - gg) / (4 * PI_GO * denom * sqrt(ora_max(denom, 1e-6)));
}

static int any_hit(const fr_world *w, const double o[3], const double d[3], double tmax) {
    double out[8];
    for (int i = 0; i < w->nobj; i++)
        if (ora_hit(w->objs[i].kind, w->objs[i].a, w->objs[i].b, w->objs[i].radius, o, d, 0.001, tmax, out)) return 1;
    return 0;
}

static void volume_light(const fr_params *p, const fr_world *w, const double pos[3], const double u[3], uint64_t *rs,
                         uint32_t cnt[3], double out[3]) {
    out[0] = out[1] = out[2] = 0;
    if (p->scatter <= 0) return;
    double sum[3] = {0, 0, 0};
    for (int j = 0; j < w->nlight; j++) {
        const fr_light *l = &w->lights[j];
        double u1 = ora_stream_next(rs);
        double u2 = ora_stream_next(rs);
        cnt[1] += 2;
        double z = 1 - 2 * u1;
        double r = sqrt(ora_max(0.0, 1 - z * z));
        double phi = 2 * PI_GO * u2;
        double lx = r * ora_cos(phi), ly = r * ora_sin(phi), lz = z;
        double len = sqrt(lx * lx + ly * ly + lz * lz);
        double n[3] = {lx / len, ly / len, lz / len};
        double lp[3];
        for (int k = 0; k < 3; k++) lp[k] = l->c[k] + l->radius * n[k];
        double pdf = 1 / (4 * PI_GO * l->radius * l->radius);
        if (pdf <= 0) continue;
        double t[3] = {lp[0] - pos[0], lp[1] - pos[1], lp[2] - pos[2]};
        double dist_sq = t[0] * t[0] + t[1] * t[1] + t[2] * t[2];
        if (dist_sq <= 1e-6) continue;
        double dist = sqrt(dist_sq);
        double wi[3] = {t[0] / dist, t[1] / dist, t[2] / dist};
        double cl = n[0] * -wi[0] + n[1] * -wi[1] + n[2] * -wi[2];
        if (!(cl > 0)) continue; /* max(0, cosLight) <= 0 */
        cnt[0]++;
        if (any_hit(w, pos, wi, dist - 0.002)) continue;
        double ct = -wi[0] * u[0] + -wi[1] * u[1] + -wi[2] * u[2];
        double ph = phase_hg(ct, p->g);
        double geometry = cl / ora_max(1e-6, dist_sq);
        double ip = ora_max(1e-6, pdf);
        for (int c = 0; c < 3; c++) sum[c] += l->le[c] * geometry * ph / ip;
    }
    for (int c = 0; c < 3; c++) out[c] = sum[c] * 2.0;
    double lum = 0.2126 * out[0] + 0.7152 * out[1] + 0.0722 * out[2];
    if (lum > 500.0) {
        double scale = 500.0 / ora_max(lum, 1e-6);
        for (int c = 0; c < 3; c++) out[c] *= scale;
    }
}

static void world_build(const ora_scene *sc, fr_world *w) {
    int n = sc->nobjects > 0 ? sc->nobjects : 1;
    w->objs = (fr_obj *)calloc((size_t)n, sizeof(fr_obj));
    w->lights = (fr_light *)calloc((size_t)n, sizeof(fr_light));
    w->nobj = w->nlight = 0;
    for (int i = 0; i < sc->nobjects; i++) {
        const ora_object *o = &sc->objects[i];
        fr_obj *h = &w->objs[w->nobj];
        memset(h, 0, sizeof *h);
        if (o->type == 0 || o->type == 3) {
            h->kind = 0;
            for (int k = 0; k < 3; k++) h->a[k] = o->position[k];
            h->radius = o->size[0];
        } else if (o->type == 1) {
            h->kind = 1;
            for (int k = 0; k < 3; k++) h->a[k] = o->position[k];
            h->b[1] = 1;
        } else if (o->type == 2) {
            h->kind = 2;
            for (int k = 0; k < 3; k++) {
                h->a[k] = o->position[k] - o->size[k] * 0.5;
                h->b[k] = o->position[k] + o->size[k] * 0.5;
            }
        } else {
            continue;
        }
        w->nobj++;
        /* lights: emissive spheres with some raw emit > 0 and some converted emit > 0, object order */
        if (h->kind != 0 || o->material < 0 || o->material >= sc->nmaterials) continue;
        const ora_material *m = &sc->materials[o->material];
        if (m->type != 3 || !(m->emit[0] > 0 || m->emit[1] > 0 || m->emit[2] > 0)) continue;
        double cm[12];
        ora_convert_material(m, cm); /* {typ, albedo[3], rough, ior, emit[3], absorption[3]} */
        if (!(cm[6] > 0 || cm[7] > 0 || cm[8] > 0)) continue;
        fr_light *l = &w->lights[w->nlight++];
        for (int k = 0; k < 3; k++) { l->c[k] = o->position[k]; l->le[k] = cm[6 + k]; }
        l->radius = o->size[0];
    }
}

static void world_free(fr_world *w) {
    free(w->objs);
    free(w->lights);
}

static void inscatter(const fr_params *p, const fr_world *w, const double orig[3], const double dir[3], uint64_t rs,
                      uint32_t cnt[3], double L[3]) {
    L[0] = L[1] = L[2] = 0;
    double closest = 1.79769313486231570814527423731704356798070e+308, out[8];
    int hit = 0;
    for (int i = 0; i < w->nobj; i++)
        if (ora_hit(w->objs[i].kind, w->objs[i].a, w->objs[i].b, w->objs[i].radius, orig, dir, 0.001, closest, out)) {
            hit = 1;
            closest = out[0];
        }
    double len = sqrt(dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2]);
    double u[3] = {dir[0] / len, dir[1] / len, dir[2] / len};
    double tmax = 40.0;
    if (hit && closest * len < 40.0) tmax = closest * len;
    double step = tmax / 24;
    if (!(step > 0)) return;
    for (int i = 0; i < 24; i++) {
        double t = ((double)i + 0.5) * step;
        double pos[3] = {orig[0] + u[0] * t, orig[1] + u[1] * t, orig[2] + u[2] * t};
        double st;
        double ss = medium(p, pos[0], pos[1], pos[2], &st);
        if (st <= 0 || ss <= 0) continue;
        cnt[2]++;
        double tr = ora_exp(-st * t);
        double ls[3];
        volume_light(p, w, pos, u, &rs, cnt, ls);
        for (int c = 0; c < 3; c++) L[c] += p->color[c] * ls[c] * ss * tr * step;
    }
}

/* The term of one sample: its fog stream is ora_stream_init(seed ^ FOG_SALT, pixel, sample).  cnt = {shadow rays, draws,
 * steps} (added to).  Returns 0 (fog_volumetric off: L = 0) or 1. */
int fr_inscatter(const ora_scene *sc, const fr_fog *raw, int32_t max_depth, const double orig[3], const double dir[3],
                 uint64_t seed, uint64_t pixel, uint64_t sample, double L[3], uint32_t cnt[3]) {
    fr_params p;
    fr_resolve(raw, &p);
    L[0] = L[1] = L[2] = 0;
    if (!(p.volumetric && max_depth > 0)) return 0;
    fr_world w;
    world_build(sc, &w);
    inscatter(&p, &w, orig, dir, ora_stream_init(seed ^ FOG_SALT, pixel, sample), cnt, L);
    world_free(&w);
    return 1;
}

/* primary ray of (x, y, s), following the oracle's pixel loop (renderer.go:181-184, camera.go:60-74) */
static void primary_ray(const double cam[22], const ora_config *cfg, int x, int y, int s, double o[3], double d[3]) {
    uint64_t rs = ora_stream_init(cfg->seed, (uint64_t)y * (uint64_t)cfg->width + (uint64_t)x, (uint64_t)s);
    double inv_w = 1.0 / (double)(cfg->width - 1), inv_h = 1.0 / (double)(cfg->height - 1);
    double flip_y = (double)(cfg->height - 1) - (double)y;
    double u = ((double)x + ora_stream_next(&rs)) * inv_w;
    double v = (flip_y + ora_stream_next(&rs)) * inv_h;
    const double *origin = cam, *llc = cam + 3, *hor = cam + 6, *ver = cam + 9, *cu = cam + 12, *cv = cam + 15;
    double lr = cam[21];
    double off[3] = {0, 0, 0};
    if (lr > 0) {
        double rx, ry, rz;
        for (;;) {
            rx = ora_stream_next(&rs) * 2 - 1;
            ry = ora_stream_next(&rs) * 2 - 1;
            rz = ora_stream_next(&rs) * 2 - 1;
            if (rx * rx + ry * ry + rz * rz >= 1.0) continue;
            break;
        }
        rx = rx * lr;
        ry = ry * lr;
        for (int k = 0; k < 3; k++) off[k] = cu[k] * rx + cv[k] * ry;
        for (int k = 0; k < 3; k++) {
            o[k] = origin[k] + off[k];
            d[k] = ((llc[k] + hor[k] * u) + ver[k] * v - origin[k]) - off[k];
        }
        return;
    }
    for (int k = 0; k < 3; k++) {
        o[k] = origin[k];
        d[k] = (llc[k] + hor[k] * u) + ver[k] * v - origin[k];
    }
}

/* Whole frame with fog: rgba (W*H*4, A = 255), accum (W*H*3 raw sums), stats = {segments, draws, shadow rays, fog draws,
 * steps}.  The sky rewrite is applied to a copy of the scene first. */
int fr_render(const ora_scene *sc_in, const ora_config *cfg, const fr_fog *raw, uint8_t *rgba, double *accum, uint64_t stats[5]) {
    ora_scene sc = *sc_in;
    fr_sky(raw, &sc.sky);
    fr_params p;
    fr_resolve(raw, &p);
    const int vol = p.volumetric && cfg->max_depth > 0;
    fr_world w;
    world_build(&sc, &w);
    double cam[22];
    ora_camera_setup(&sc.camera, cfg->width, cfg->height, cam);
    memset(stats, 0, 5 * sizeof(uint64_t));
    for (int y = 0; y < cfg->height; y++)
        for (int x = 0; x < cfg->width; x++) {
            double sum[3] = {0, 0, 0};
            for (int s = 0; s < cfg->spp; s++) {
                double c[3], f[3] = {0, 0, 0};
                uint32_t nseg = 0, ndraw = 0, cnt[3] = {0, 0, 0};
                ora_sample(&sc, cfg, x, y, s, c, &nseg, &ndraw);
                stats[0] += nseg;
                stats[1] += ndraw;
                if (vol) {
                    double o[3], d[3];
                    primary_ray(cam, cfg, x, y, s, o, d);
                    const uint64_t pix = (uint64_t)y * (uint64_t)cfg->width + (uint64_t)x;
                    inscatter(&p, &w, o, d, ora_stream_init(cfg->seed ^ FOG_SALT, pix, (uint64_t)s), cnt, f);
                    stats[2] += cnt[0];
                    stats[3] += cnt[1];
                    stats[4] += cnt[2];
                }
                for (int k = 0; k < 3; k++) sum[k] += c[k] + f[k];
            }
            size_t i = (size_t)y * (size_t)cfg->width + (size_t)x;
            if (accum) for (int k = 0; k < 3; k++) accum[3 * i + k] = sum[k];
            if (rgba) {
                ora_finish_pixel(sum, cfg->spp, rgba + 4 * i);
                rgba[4 * i + 3] = 255;
            }
        }
    world_free(&w);
    return 0;
}

/* ---- batch entry points for the tests ---- */

/* out[i] = Go's math.Sin(x[i]) through the oracle */
void fr_sin_many(const double *x, double *out, int64_t n) {
    for (int64_t i = 0; i < n; i++) out[i] = ora_sin(x[i]);
}

/* resolved block as doubles: density, scatter, sigma_s, sigma_a, g, hetero, noise_scale, color[3], octaves, affect_sky,
 * volumetric (13) */
void fr_resolve_flat(const fr_fog *raw, double out[13]) {
    fr_params p;
    fr_resolve(raw, &p);
    double v[13] = {p.density, p.scatter, p.sigma_s, p.sigma_a, p.g, p.hetero, p.noise_scale, p.color[0], p.color[1],
                    p.color[2], (double)p.octaves, (double)p.affect_sky, (double)p.volumetric};
    memcpy(out, v, sizeof v);
}

/* n terms: rays[i] = {ox, oy, oz, dx, dy, dz}, keys[i] = {seed, pixel, sample}; L[3i..], cnt[3i..] */
void fr_inscatter_many(const ora_scene *sc, const fr_fog *raw, int32_t max_depth, int64_t n, const double *rays,
                       const uint64_t *keys, double *L, uint32_t *cnt) {
    fr_params p;
    fr_resolve(raw, &p);
    fr_world w;
    world_build(sc, &w);
    for (int64_t i = 0; i < n; i++) {
        L[3 * i] = L[3 * i + 1] = L[3 * i + 2] = 0;
        cnt[3 * i] = cnt[3 * i + 1] = cnt[3 * i + 2] = 0;
        if (!(p.volumetric && max_depth > 0)) continue;
        inscatter(&p, &w, rays + 6 * i, rays + 6 * i + 3, ora_stream_init(keys[3 * i] ^ FOG_SALT, keys[3 * i + 1], keys[3 * i + 2]),
                  cnt + 3 * i, L + 3 * i);
    }
    world_free(&w);
}

/* the pieces of the term one at a time (the device probe, test_device_math_gpu.py): p[i] = {x, y, z} */
void fr_hash31_many(const double *p, double *out, int64_t n) {
    for (int64_t i = 0; i < n; i++) out[i] = hash31(p[3 * i], p[3 * i + 1], p[3 * i + 2]);
}
void fr_noise_many(const fr_fog *raw, const double *p, double *out, int64_t n) {
    fr_params q;
    fr_resolve(raw, &q);
    for (int64_t i = 0; i < n; i++) out[i] = volume_noise(&q, p[3 * i], p[3 * i + 1], p[3 * i + 2]);
}
void fr_phase_many(const double *ct, const double *g, double *out, int64_t n) {
    for (int64_t i = 0; i < n; i++) out[i] = phase_hg(ct[i], g[i]);
}

/* the oracle's scalar routines over arrays (a million ctypes calls would take minutes): which = 0 ora_sin, 1 ora_cos,
 * 2 ora_tan, 3 ora_exp; 0 ora_pow, 1 ora_min, 2 ora_max */
void fr_ora_unary_many(int which, const double *x, double *out, int64_t n) {
    for (int64_t i = 0; i < n; i++)
        out[i] = which == 0 ? ora_sin(x[i]) : which == 1 ? ora_cos(x[i]) : which == 2 ? ora_tan(x[i]) : ora_exp(x[i]);
}
void fr_ora_binary_many(int which, const double *a, const double *b, double *out, int64_t n) {
    for (int64_t i = 0; i < n; i++)
        out[i] = which == 0 ? ora_pow(a[i], b[i]) : which == 1 ? ora_min(a[i], b[i]) : ora_max(a[i], b[i]);
}
/* keys[i] = {seed, pixel, sample}: state0[i] = ora_stream_init, out[i][0..ndraw) = that many ora_stream_next */
void fr_ora_streams(const uint64_t *keys, int32_t ndraw, uint64_t *state0, double *out, int64_t n) {
    for (int64_t i = 0; i < n; i++) {
        uint64_t s = ora_stream_init(keys[3 * i], keys[3 * i + 1], keys[3 * i + 2]);
        state0[i] = s;
        for (int32_t k = 0; k < ndraw; k++) out[i * ndraw + k] = ora_stream_next(&s);
    }
}

/* n shadow rays, rays[7i] = o, d, tmax: out[i] = any_hit, the shadow test of volume_light, over [0.001, tmax]. */
void fr_occluded_many(const ora_scene *sc, int64_t n, const double *rays, int32_t *out) {
    fr_world w;
    world_build(sc, &w);
    for (int64_t i = 0; i < n; i++) out[i] = any_hit(&w, rays + 7 * i, rays + 7 * i + 3, rays[7 * i + 6]);
    world_free(&w);
}
