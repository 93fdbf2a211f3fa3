/* atrous_reference.c -- independent CPU restatement of the first-hit feature planes and of the variance-guided a-trous filter,
 * written from the specification in path_trace_golang_amd/csrc/pt_atrous.h's header comment, on the oracle: ora_primary_ray,
 * ora_hit and ora_convert_material supply the features, ora_exp and C's sqrt the filter's arithmetic.  Built at test time
 * (tests/atrous_support.py) with the oracle's flags: no contraction, no fast-math.  Whole-image loops over plain arrays; nothing
 * here is shared with the product's header. */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "pt_oracle.h"

typedef struct {
    int32_t kind;
    double a[3], b[3], radius, albedo[3];
} ar_obj;

/* sceneToWorld (objects.go:225-269): unknown types are skipped, a missing material id is the zero material */
static int ar_world(const ora_scene *sc, ar_obj *w) {
    int n = 0;
    for (int i = 0; i < sc->nobjects; i++) {
        const ora_object *o = &sc->objects[i];
        ar_obj h;
        memset(&h, 0, sizeof h);
        if (o->type == 0 || o->type == 3) {
            h.kind = 0;
            for (int k = 0; k < 3; k++) h.a[k] = o->position[k];
            h.radius = o->size[0];
        } else if (o->type == 1) {
            h.kind = 1;
            for (int k = 0; k < 3; k++) h.a[k] = o->position[k];
            h.b[1] = 1;
        } else if (o->type == 2) {
            h.kind = 2;
            for (int k = 0; k < 3; k++) {
                h.a[k] = o->position[k] - o->size[k] * 0.5;
                h.b[k] = o->position[k] + o->size[k] * 0.5;
            }
        } else {
            continue;
        }
        if (o->material >= 0 && o->material < sc->nmaterials) {
            double m[12];
            ora_convert_material(&sc->materials[o->material], m);
            h.albedo[0] = m[1]; h.albedo[1] = m[2]; h.albedo[2] = m[3];
        }
        w[n++] = h;
    }
    return n;
}

/* the closest hit of the first segment (renderer.go:297-302): out = {hit, normal[3], albedo[3], t * |dir|} */
static void ar_first_hit(const ar_obj *w, int nw, const double o[3], const double d[3], double out[8]) {
    double closest = DBL_MAX;
    memset(out, 0, 8 * sizeof(double));
    for (int i = 0; i < nw; i++) {
        double rec[8];
        if (ora_hit(w[i].kind, w[i].a, w[i].b, w[i].radius, o, d, 0.001, closest, rec)) {
            closest = rec[0];
            out[0] = 1;
            for (int k = 0; k < 3; k++) { out[1 + k] = rec[4 + k]; out[4 + k] = w[i].albedo[k]; }
            out[7] = rec[0] * sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        }
    }
}

/* the first hit of n chosen rays ([n][6]: origin, direction): out [n][8] */
void ar_first_hit_many(const ora_scene *sc, int64_t n, const double *rays, double *out) {
    ar_obj *w = malloc(sizeof(ar_obj) * (size_t)(sc->nobjects > 0 ? sc->nobjects : 1));
    const int nw = ar_world(sc, w);
    for (int64_t i = 0; i < n; i++) ar_first_hit(w, nw, rays + 6 * i, rays + 6 * i + 3, out + 8 * i);
    free(w);
}

/* The feature sums of a frame: every pixel takes its samples s < min(k, its count) (counts == NULL: cfg->spp for every pixel).
 * fn, fa, fd: [H][W][3]. */
void ar_features(const ora_scene *sc, const ora_config *cfg, int32_t k, const uint32_t *counts, double *fn, double *fa, double *fd) {
    ar_obj *w = malloc(sizeof(ar_obj) * (size_t)(sc->nobjects > 0 ? sc->nobjects : 1));
    const int nw = ar_world(sc, w);
    for (int32_t y = 0; y < cfg->height; y++)
        for (int32_t x = 0; x < cfg->width; x++) {
            const size_t i = (size_t)y * (size_t)cfg->width + (size_t)x;
            const int64_t n = counts ? (int64_t)counts[i] : (int64_t)cfg->spp;
            const int64_t take = k < n ? k : n;
            double sn[3] = {0, 0, 0}, sa[3] = {0, 0, 0}, sd[3] = {0, 0, 0};
            for (int32_t s = 0; s < take; s++) {
                double o[3], d[3], h[8];
                ora_primary_ray(sc, cfg, x, y, s, o, d);
                ar_first_hit(w, nw, o, d, h);
                if (h[0] != 0) {
                    for (int c = 0; c < 3; c++) { sn[c] += h[1 + c]; sa[c] += h[4 + c]; }
                    sd[0] += h[7];
                    sd[1] += 1;
                }
                sd[2] += 1;
            }
            for (int c = 0; c < 3; c++) { fn[3 * i + c] = sn[c]; fa[3 * i + c] = sa[c]; fd[3 * i + c] = sd[c]; }
        }
    free(w);
}

static int ar_finite(double x) { return !isnan(x) && !isinf(x); }

/* The filter.  S, Q: [H][W][3] raw sums; cnt: [H][W] counts or NULL (n for every pixel); fn, fa, fd: feature sums or NULL (a frame
 * without features).  sig = {sigma_l, sigma_n, sigma_z, sigma_a}.  Outputs (any may be NULL): mean [H][W][3], var [H][W], rgba
 * [H][W][4], noise[2] = before, after, bad = bad pixels. */
void ar_filter(int32_t W, int32_t H, const double *S, const double *Q, const uint32_t *cnt, uint32_t n, const double *fn,
               const double *fa, const double *fd, int32_t T, const double sig[4], double *mean, double *var, uint8_t *rgba,
               double noise[2], uint64_t *bad_out) {
    const size_t np = (size_t)W * (size_t)H;
    double *c = malloc(np * 3 * sizeof(double)), *c2 = malloc(np * 3 * sizeof(double));
    double *v = malloc(np * sizeof(double)), *v2 = malloc(np * sizeof(double));
    double *N = calloc(np * 3, sizeof(double)), *A = calloc(np * 3, sizeof(double)), *z = calloc(np, sizeof(double));
    unsigned char *bad = calloc(np, 1);
    const int have = fn && fa && fd;
    const int n_on = have && sig[1] > 0, z_on = have && sig[2] > 0, a_on = have && sig[3] > 0;
    uint64_t nbad = 0;
    /* prep */
    for (size_t i = 0; i < np; i++) {
        const double ni = (double)(cnt ? cnt[i] : n);
        double vs[3];
        int ok = 1;
        for (int k = 0; k < 3; k++) {
            const double m = S[3 * i + k] / ni;
            double d = Q[3 * i + k] / ni - m * m;
            if (d < 0) d = 0;
            vs[k] = d / (ni - 1);
            c[3 * i + k] = m;
            if (!ar_finite(m)) ok = 0;
        }
        v[i] = (vs[0] + vs[1] + vs[2]) / 3;
        if (!ar_finite(v[i])) ok = 0;
        bad[i] = !ok;
        nbad += !ok;
        if (have && fd[3 * i + 1] != 0) {
            const double h = fd[3 * i + 1];
            for (int k = 0; k < 3; k++) { N[3 * i + k] = fn[3 * i + k] / h; A[3 * i + k] = fa[3 * i + k] / h; }
            z[i] = fd[3 * i] / h;
        }
    }
    for (int pass = 0; pass < 2; pass++) {
        if (pass == 1) {
            /* iterations */
            static const double B[5] = {1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16};
            for (int32_t t = 0; t < T; t++) {
                const int32_t step = 1 << t;
                for (int32_t y = 0; y < H; y++)
                    for (int32_t x = 0; x < W; x++) {
                        const size_t i = (size_t)y * (size_t)W + (size_t)x;
                        if (bad[i]) {
                            for (int k = 0; k < 3; k++) c2[3 * i + k] = c[3 * i + k];
                            v2[i] = v[i];
                            continue;
                        }
                        const double li = (c[3 * i] + c[3 * i + 1] + c[3 * i + 2]) / 3;
                        double sw = 0, sc[3] = {0, 0, 0}, sv = 0;
                        for (int dy = -2; dy <= 2; dy++)
                            for (int dx = -2; dx <= 2; dx++) {
                                const int32_t xj = x + dx * step, yj = y + dy * step;
                                if (xj < 0 || yj < 0 || xj >= W || yj >= H) continue;
                                const size_t j = (size_t)yj * (size_t)W + (size_t)xj;
                                if (bad[j]) continue;
                                const double lj = (c[3 * j] + c[3 * j + 1] + c[3 * j + 2]) / 3;
                                double pen = fabs(li - lj) / (sig[0] * sqrt(v[i]) + 1e-8);
                                if (n_on) {
                                    const double q = 1 - (N[3 * i] * N[3 * j] + N[3 * i + 1] * N[3 * j + 1] + N[3 * i + 2] * N[3 * j + 2]);
                                    pen = pen + (q > 0 ? q : 0) / sig[1];
                                }
                                if (z_on) pen = pen + fabs(z[i] - z[j]) / (sig[2] * (z[i] > 1e-8 ? z[i] : 1e-8));
                                if (a_on) {
                                    const double dr = A[3 * i] - A[3 * j], dg = A[3 * i + 1] - A[3 * j + 1], db = A[3 * i + 2] - A[3 * j + 2];
                                    pen = pen + (dr * dr + dg * dg + db * db) / (sig[3] * sig[3]);
                                }
                                const double w = (B[dy + 2] * B[dx + 2]) * ora_exp(-pen); /* (exactly 0 for a pen above 745.2) */
                                sw = sw + w;
                                for (int k = 0; k < 3; k++) sc[k] = sc[k] + w * (c[3 * j + k] - c[3 * i + k]);
                                sv = sv + (w * w) * v[j];
                            }
                        for (int k = 0; k < 3; k++) c2[3 * i + k] = c[3 * i + k] + sc[k] / sw;
                        v2[i] = sv / (sw * sw);
                    }
                double *tmp = c; c = c2; c2 = tmp;
                tmp = v; v = v2; v2 = tmp;
            }
        }
        /* the noise figure of the state */
        double sum = 0;
        for (size_t i = 0; i < np; i++) {
            double den = (c[3 * i] + c[3 * i + 1] + c[3 * i + 2]) / 3;
            if (den < 0.01) den = 0.01;
            const double e2 = v[i] / (den * den);
            if (ar_finite(e2)) sum += e2;
        }
        if (noise) noise[pass] = sqrt(sum / (double)np);
    }
    for (size_t i = 0; i < np; i++) {
        if (mean) for (int k = 0; k < 3; k++) mean[3 * i + k] = c[3 * i + k];
        if (var) var[i] = v[i];
        if (rgba) {
            ora_finish_pixel(c + 3 * i, 1, rgba + 4 * i);
            rgba[4 * i + 3] = 255;
        }
    }
    if (bad_out) *bad_out = nbad;
    free(c); free(c2); free(v); free(v2); free(N); free(A); free(z); free(bad);
}
