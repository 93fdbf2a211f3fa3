/* fake_ptcore.c -- a recording stand-in for libptcore.so (include/ptcore.h), for the host-layer trace tests
 * (tests/test_host_trace_cpu.py).  CPU only; it renders nothing.  Every entry point appends one line to the file named by
 * PTFAKE_LOG: its name, its scalar arguments, the fields of the structs passed in and which pointers are NULL.
 *
 * PTFAKE_SCRIPT = items separated by ';' drives what a frame needs:
 *     noise=a,b,c       what successive pt_noise_estimate calls return (the last value repeats; default 1)
 *     halves=a/b,c/d    noise/noise_model of successive pt_atrous_halves calls (the last pair repeats; default 1/1)
 *     stall_at=N        pt_step adds nothing once done == N (an adaptive frame whose blocks have all stopped)
 *     fail=NAME:K       the K-th call of NAME returns PT_ERR_HIP with pt_last_error() = "injected"
 *
 * -DPTFAKE_BASE_ABI leaves out every entry point added within ABI 4 (capi.ADDITIVE); -DPTFAKE_NO_ADAPTIVE, -DPTFAKE_NO_HALVES and
 * -DPTFAKE_NO_CLIP leave out one group each, for the "libptcore.so lacks ..." texts that sit behind another group's check;
 * -DPTFAKE_ABI=N answers pt_abi_version with N. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/ptcore.h"

struct pt_ctx { int unused; };
static struct pt_ctx g_ctx;
static const char *g_err = "";
static int32_t g_w, g_h, g_cap, g_done;
static double g_clip;
static int g_calls_n;
static struct { char name[40]; int n; } g_calls[64];

static const char *script_item(const char *key, char *buf, size_t cap) {
    const char *s = getenv("PTFAKE_SCRIPT");
    size_t kl = strlen(key);
    while (s && *s) {
        const char *e = strchr(s, ';');
        size_t n = e ? (size_t)(e - s) : strlen(s);
        if (n > kl && !strncmp(s, key, kl) && s[kl] == '=') {
            size_t m = n - kl - 1 < cap - 1 ? n - kl - 1 : cap - 1;
            memcpy(buf, s + kl + 1, m);
            buf[m] = 0;
            return buf;
        }
        s = e ? e + 1 : NULL;
    }
    return NULL;
}

/* the idx-th (0-based) comma-separated entry of a script list, the last one when the list is shorter */
static const char *script_entry(const char *key, int idx, char *buf, size_t cap) {
    char *p = (char *)script_item(key, buf, cap), *q;
    if (!p) return NULL;
    while (idx-- > 0 && (q = strchr(p, ','))) p = q + 1;
    if ((q = strchr(p, ','))) *q = 0;
    return p;
}

static void logf_(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
#include <stdarg.h>
static void logf_(const char *fmt, ...) {
    const char *path = getenv("PTFAKE_LOG");
    FILE *f = path ? fopen(path, "a") : NULL;
    va_list ap;
    if (!f) return;
    va_start(ap, fmt);
    vfprintf(f, fmt, ap);
    va_end(ap);
    fputc('\n', f);
    fclose(f);
}

/* counts the call and returns what it returns: PT_ERR_HIP when the script fails this one */
static int32_t ret(const char *name) {
    char buf[64], *colon;
    int i, n;
    for (i = 0; i < g_calls_n && strcmp(g_calls[i].name, name); i++) {}
    if (i == g_calls_n && g_calls_n < 64) { snprintf(g_calls[i].name, sizeof g_calls[i].name, "%s", name); g_calls[i].n = 0; g_calls_n++; }
    n = i < 64 ? ++g_calls[i].n : 0;
    if (script_item("fail", buf, sizeof buf) && (colon = strchr(buf, ':'))) {
        *colon = 0;
        if (!strcmp(buf, name) && atoi(colon + 1) == n) { g_err = "injected"; return PT_ERR_HIP; }
    }
    return PT_OK;
}
static int calls_of(const char *name) {
    for (int i = 0; i < g_calls_n; i++) if (!strcmp(g_calls[i].name, name)) return g_calls[i].n;
    return 0;
}

#define P(p) ((p) ? "set" : "NULL")

static void log_frame(const char *name, const pt_scene *sc, const pt_config *c) {
    logf_("%s cfg{w=%d h=%d spp=%d depth=%d seed=%llu chunk=%d flags=%d} scene{objects=%d materials=%d}", name, c->width, c->height,
          c->samples_per_px, c->max_depth, (unsigned long long)c->seed, c->spp_chunk, c->flags, sc->num_objects, sc->num_materials);
}
static void paint(uint8_t *rgba, int32_t stride) { /* R = samples done, A = 255: enough to see that an image came back */
    if (!rgba || stride < 4 * g_w) return;
    for (int32_t y = 0; y < g_h; y++)
        for (int32_t x = 0; x < g_w; x++) {
            uint8_t *p = rgba + (size_t)y * (size_t)stride + 4 * (size_t)x;
            p[0] = (uint8_t)g_done; p[1] = 0; p[2] = 0; p[3] = 255;
        }
}
static void fill_stats(pt_stats *st) {
    if (!st) return;
    memset(st, 0, sizeof *st);
    st->samples = (uint64_t)g_w * (uint64_t)g_h * (uint64_t)g_done + 1; st->segments = 2000; st->exit_scans = 30; st->draws = 4000;
    st->seconds = 0.5; st->trace_ms = 1.5; st->resolve_ms = 0.25; st->device_ms = 2.0;
    st->trace_launches = 3; st->resolve_launches = 1; st->spp_chunk = 4; st->num_devices = 1; st->per_device_ms[0] = 2.0;
}
static void log_atrous_cfg(char *out, size_t cap, const pt_atrous_config *c) {
    if (!c) snprintf(out, cap, "NULL");
    else snprintf(out, cap, "{iters=%d reserved=%d sigma_l=%g sigma_n=%g sigma_z=%g sigma_a=%g}", c->iterations, c->reserved, c->sigma_l,
                  c->sigma_n, c->sigma_z, c->sigma_a);
}

#ifndef PTFAKE_ABI
#define PTFAKE_ABI PT_ABI_VERSION
#endif
int32_t pt_abi_version(void) { logf_("pt_abi_version"); return PTFAKE_ABI; }
const char *pt_last_error(void) { logf_("pt_last_error -> %s", g_err); return g_err; }
int32_t pt_device_count(int32_t *count) { logf_("pt_device_count"); if (count) *count = 1; return ret("pt_device_count"); }

int32_t pt_create(const int32_t *devices, int32_t ndev, pt_ctx **out) {
    char list[128] = "NULL";
    if (devices) {
        size_t k = 0;
        list[0] = 0;
        for (int32_t i = 0; i < ndev && k + 16 < sizeof list; i++) k += (size_t)snprintf(list + k, sizeof list - k, i ? ",%d" : "%d", devices[i]);
    }
    logf_("pt_create devices=%s ndev=%d", list, ndev);
    *out = &g_ctx;
    return ret("pt_create");
}
void pt_destroy(pt_ctx *ctx) { logf_("pt_destroy ctx=%s", P(ctx)); }

int32_t pt_render(pt_ctx *ctx, const pt_scene *scene, const pt_config *cfg, uint8_t *rgba, int32_t stride, double *accum, uint32_t *nseg,
                  uint32_t *ndraw, pt_stats *stats) {
    (void)ctx;
    log_frame("pt_render", scene, cfg);
    logf_("pt_render rgba=%s stride=%d accum=%s nseg=%s ndraw=%s stats=%s", P(rgba), stride, P(accum), P(nseg), P(ndraw), P(stats));
    int32_t rc = ret("pt_render");
    if (rc) return rc;
    g_w = cfg->width; g_h = cfg->height; g_cap = cfg->samples_per_px; g_done = g_cap > 0 ? g_cap : 0;
    paint(rgba, stride);
    fill_stats(stats);
    return PT_OK;
}
int32_t pt_begin(pt_ctx *ctx, const pt_scene *scene, const pt_config *cfg) {
    (void)ctx;
    log_frame("pt_begin", scene, cfg);
    int32_t rc = ret("pt_begin");
    if (rc) return rc;
    g_w = cfg->width; g_h = cfg->height; g_cap = cfg->samples_per_px; g_done = 0;
    return PT_OK;
}
int32_t pt_step(pt_ctx *ctx, int32_t nspp, int32_t *done_spp) {
    char buf[32];
    (void)ctx;
    int32_t rc = ret("pt_step");
    if (!rc && !(script_item("stall_at", buf, sizeof buf) && g_done == atoi(buf))) {
        g_done += nspp > 0 ? nspp : 0;
        if (g_done > g_cap) g_done = g_cap > 0 ? g_cap : 0;
    }
    logf_("pt_step nspp=%d -> %s done=%d", nspp, rc ? "ERR" : "OK", g_done);
    if (!rc && done_spp) *done_spp = g_done;
    return rc;
}
int32_t pt_read(pt_ctx *ctx, uint8_t *rgba, int32_t stride, double *accum) {
    (void)ctx;
    logf_("pt_read rgba=%s stride=%d accum=%s", P(rgba), stride, P(accum));
    int32_t rc = ret("pt_read");
    if (!rc) paint(rgba, stride);
    return rc;
}
int32_t pt_end(pt_ctx *ctx, pt_stats *stats) {
    (void)ctx;
    logf_("pt_end stats=%s", P(stats));
    fill_stats(stats);
    return ret("pt_end");
}
int32_t pt_shard_tiles(int32_t width, int32_t height, const pt_shard *shard, int32_t *ntiles_local, int32_t *ntiles_x, int32_t *ntiles_y) {
    (void)shard;
    logf_("pt_shard_tiles w=%d h=%d", width, height);
    if (ntiles_x) *ntiles_x = (width + 31) / 32;
    if (ntiles_y) *ntiles_y = (height + 31) / 32;
    if (ntiles_local) *ntiles_local = ((width + 31) / 32) * ((height + 31) / 32);
    return ret("pt_shard_tiles");
}
int32_t pt_render_tiles_device(pt_ctx *ctx, const pt_scene *scene, const pt_config *cfg, const pt_shard *shard, void *d_tiles_rgba,
                               void *d_tiles_accum, void *stream, pt_stats *stats) {
    (void)ctx; (void)shard; (void)d_tiles_rgba; (void)d_tiles_accum; (void)stream; (void)stats;
    log_frame("pt_render_tiles_device", scene, cfg);
    return ret("pt_render_tiles_device");
}
int32_t pt_untile_device(pt_ctx *ctx, int32_t width, int32_t height, int32_t shard_count, int32_t shard_stride_tiles, const void *d_tiles_rgba,
                         const void *d_tiles_accum, void *d_rgba, int32_t stride, void *d_accum, void *stream) {
    (void)ctx; (void)shard_count; (void)shard_stride_tiles; (void)d_tiles_rgba; (void)d_tiles_accum; (void)d_rgba; (void)stride; (void)d_accum;
    (void)stream;
    logf_("pt_untile_device w=%d h=%d", width, height);
    return ret("pt_untile_device");
}
int32_t pt_post_process(pt_ctx *ctx, const pt_post_config *post, const double *accum, int32_t samples_per_px, uint8_t *rgba, int32_t stride,
                        int32_t width, int32_t height) {
    (void)ctx; (void)post; (void)accum; (void)rgba; (void)stride;
    logf_("pt_post_process spp=%d w=%d h=%d", samples_per_px, width, height);
    return ret("pt_post_process");
}
int32_t pt_set_fog(pt_ctx *ctx, const pt_fog *fog) {
    (void)ctx;
    if (fog) logf_("pt_set_fog fog{density=%g sigma_s=%g octaves=%d affect_sky=%d gpu_volumetric=%d}", fog->density, fog->sigma_s, fog->noise_octaves,
                   fog->affect_sky, fog->gpu_volumetric);
    else logf_("pt_set_fog fog=NULL");
    return ret("pt_set_fog");
}
int32_t pt_fog_last_stats(pt_ctx *ctx, pt_fog_stats *out) {
    (void)ctx;
    logf_("pt_fog_last_stats");
    if (out) memset(out, 0, sizeof *out);
    return ret("pt_fog_last_stats");
}
int64_t pt_debug_scan_mismatches(pt_ctx *ctx) { (void)ctx; logf_("pt_debug_scan_mismatches"); return 0; }
int64_t pt_debug_div_selftest(pt_ctx *ctx, int32_t millions, uint64_t seed) { (void)ctx; (void)seed; logf_("pt_debug_div_selftest millions=%d", millions); return 0; }
int32_t pt_debug_profile(pt_ctx *ctx, uint64_t *out, int32_t n) { (void)ctx; (void)out; logf_("pt_debug_profile n=%d", n); return ret("pt_debug_profile"); }
int32_t pt_debug_bvh_check(const pt_scene *scene, int32_t out[8]) { (void)scene; logf_("pt_debug_bvh_check"); if (out) memset(out, 0, 8 * sizeof out[0]); return ret("pt_debug_bvh_check"); }
int32_t pt_debug_gather_mode(pt_ctx *ctx) { (void)ctx; logf_("pt_debug_gather_mode"); return 0; }

/* ---------------------------------------------------------------- the entry points added within ABI 4 */
#ifndef PTFAKE_BASE_ABI
int32_t pt_set_shading(pt_ctx *ctx, const pt_shading *s) {
    (void)ctx;
    if (s) logf_("pt_set_shading shading{model=%d num_materials=%d materials=%s}", s->model, s->num_materials, P(s->materials));
    else logf_("pt_set_shading shading=NULL");
    return ret("pt_set_shading");
}
int32_t pt_shading_last_stats(pt_ctx *ctx, pt_shading_stats *out) {
    (void)ctx;
    logf_("pt_shading_last_stats");
    if (out) memset(out, 0, sizeof *out);
    return ret("pt_shading_last_stats");
}
int32_t pt_debug_set_primary_rays(pt_ctx *ctx, const double *rays, int64_t n) {
    (void)ctx;
    logf_("pt_debug_set_primary_rays rays=%s n=%lld", P(rays), (long long)n);
    return ret("pt_debug_set_primary_rays");
}
int32_t pt_set_moments(pt_ctx *ctx, int32_t on) { (void)ctx; logf_("pt_set_moments on=%d", on); return ret("pt_set_moments"); }
int32_t pt_read_moments(pt_ctx *ctx, double *m2) { (void)ctx; logf_("pt_read_moments m2=%s", P(m2)); return ret("pt_read_moments"); }
int32_t pt_noise_estimate(pt_ctx *ctx, pt_noise *out) {
    char buf[256];
    (void)ctx;
    int32_t rc = ret("pt_noise_estimate");
    const char *v = script_entry("noise", calls_of("pt_noise_estimate") - 1, buf, sizeof buf);
    memset(out, 0, sizeof *out);
    out->noise = v ? atof(v) : 1.0;
    out->max_pixel = 2 * out->noise;
    out->pixels = (uint64_t)g_w * (uint64_t)g_h;
    out->spp = g_done;
    logf_("pt_noise_estimate -> %s noise=%g", rc ? "ERR" : "OK", out->noise);
    return rc;
}
#ifndef PTFAKE_NO_ADAPTIVE
int32_t pt_set_adaptive(pt_ctx *ctx, const pt_adaptive *a) {
    (void)ctx;
    if (a) logf_("pt_set_adaptive adaptive{target=%g min_spp=%d step=%d}", a->target, a->min_spp, a->step);
    else logf_("pt_set_adaptive adaptive=NULL");
    return ret("pt_set_adaptive");
}
int32_t pt_adaptive_state(pt_ctx *ctx, struct pt_adaptive_state *out) {
    (void)ctx;
    logf_("pt_adaptive_state");
    memset(out, 0, sizeof *out);
    out->blocks = 4; out->active_blocks = 1; out->samples = 77; out->spp_min = 3; out->spp_max = g_done; out->worst_active = 0.5;
    return ret("pt_adaptive_state");
}
int32_t pt_read_sample_counts(pt_ctx *ctx, uint32_t *spp) { (void)ctx; logf_("pt_read_sample_counts spp=%s", P(spp)); return ret("pt_read_sample_counts"); }
#endif
int32_t pt_set_features(pt_ctx *ctx, int32_t k) { (void)ctx; logf_("pt_set_features k=%d", k); return ret("pt_set_features"); }
int32_t pt_read_features(pt_ctx *ctx, double *normal, double *albedo, double *depth) {
    (void)ctx;
    logf_("pt_read_features normal=%s albedo=%s depth=%s", P(normal), P(albedo), P(depth));
    return ret("pt_read_features");
}
int32_t pt_atrous(pt_ctx *ctx, const pt_atrous_config *cfg, uint8_t *rgba, int32_t stride, double *mean, double *var, pt_atrous_stats *stats) {
    char c[160];
    (void)ctx;
    log_atrous_cfg(c, sizeof c, cfg);
    logf_("pt_atrous cfg=%s rgba=%s stride=%d mean=%s var=%s stats=%s", c, P(rgba), stride, P(mean), P(var), P(stats));
    int32_t rc = ret("pt_atrous");
    if (rc) return rc;
    paint(rgba, stride);
    if (stats) {
        memset(stats, 0, sizeof *stats);
        stats->atrous_ms = 0.75; stats->launches = 9; stats->iterations = cfg ? cfg->iterations : 5; stats->noise_before = 0.4; stats->noise_after = 0.2;
    }
    return PT_OK;
}
#ifndef PTFAKE_NO_HALVES
int32_t pt_set_halves(pt_ctx *ctx, int32_t on) { (void)ctx; logf_("pt_set_halves on=%d", on); return ret("pt_set_halves"); }
int32_t pt_read_halves(pt_ctx *ctx, double *sa, double *qa, double *sb, double *qb) {
    (void)ctx;
    logf_("pt_read_halves sa=%s qa=%s sb=%s qb=%s", P(sa), P(qa), P(sb), P(qb));
    return ret("pt_read_halves");
}
int32_t pt_atrous_halves(pt_ctx *ctx, const pt_atrous_config *cfg, double *mean, double *err, double *half_means, pt_halves_stats *stats) {
    char c[160], buf[256];
    (void)ctx;
    log_atrous_cfg(c, sizeof c, cfg);
    int32_t rc = ret("pt_atrous_halves");
    const char *v = script_entry("halves", calls_of("pt_atrous_halves") - 1, buf, sizeof buf);
    const char *slash = v ? strchr(v, '/') : NULL;
    const double noise = v ? atof(v) : 1.0, model = slash ? atof(slash + 1) : 1.0;
    logf_("pt_atrous_halves cfg=%s mean=%s err=%s half_means=%s stats=%s done=%d -> %s noise=%g noise_model=%g", c, P(mean), P(err), P(half_means),
          P(stats), g_done, rc ? "ERR" : "OK", noise, model);
    if (rc) return rc;
    if (stats) {
        memset(stats, 0, sizeof *stats);
        stats->atrous_ms = 0.5; stats->launches = 7; stats->iterations = cfg ? cfg->iterations : 5; stats->noise = noise; stats->noise_model = model;
        stats->spp_min = g_done;
    }
    return PT_OK;
}
#endif
int32_t pt_temporal(pt_ctx *ctx, const pt_temporal_config *cfg, const pt_atrous_config *filter, uint8_t *rgba, int32_t stride, double *mean, double *var,
                    pt_temporal_stats *stats) {
    char c[160], t[160] = "NULL";
    (void)ctx;
    log_atrous_cfg(c, sizeof c, filter);
    if (cfg) snprintf(t, sizeof t, "{alpha=%g tol_z=%g n_min=%g tol_a=%g max_len=%d reserved=%d}", cfg->alpha, cfg->tol_z, cfg->n_min, cfg->tol_a,
                      cfg->max_len, cfg->reserved);
    logf_("pt_temporal cfg=%s filter=%s rgba=%s stride=%d mean=%s var=%s stats=%s", t, c, P(rgba), stride, P(mean), P(var), P(stats));
    int32_t rc = ret("pt_temporal");
    if (rc) return rc;
    paint(rgba, stride);
    if (stats) {
        memset(stats, 0, sizeof *stats);
        stats->temporal_ms = 1.25; stats->launches = 10; stats->iterations = filter ? filter->iterations : 0; stats->reprojected = 50;
        stats->disoccluded = 3; stats->mean_len = 2.5; stats->noise_before = 0.4; stats->noise_blended = 0.3; stats->noise_after = 0.15;
    }
    return PT_OK;
}
int32_t pt_temporal_read(pt_ctx *ctx, double *mean, double *var, int32_t *len) {
    (void)ctx;
    logf_("pt_temporal_read mean=%s var=%s len=%s", P(mean), P(var), P(len));
    return ret("pt_temporal_read");
}
int32_t pt_temporal_reset(pt_ctx *ctx) { (void)ctx; logf_("pt_temporal_reset"); return ret("pt_temporal_reset"); }
#ifndef PTFAKE_NO_CLIP
int32_t pt_temporal_set_clip(pt_ctx *ctx, double gamma) {
    (void)ctx;
    logf_("pt_temporal_set_clip gamma=%g", gamma);
    int32_t rc = ret("pt_temporal_set_clip");
    if (!rc) g_clip = gamma;
    return rc;
}
int32_t pt_temporal_clip_stats(pt_ctx *ctx, struct pt_temporal_clip_stats *out) {
    (void)ctx;
    logf_("pt_temporal_clip_stats");
    out->gamma = g_clip; out->clipped = 7; out->reprojected = 50;
    return ret("pt_temporal_clip_stats");
}
#endif
#endif /* PTFAKE_BASE_ABI */
