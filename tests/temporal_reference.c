/* temporal_reference.c -- independent CPU restatement of the temporal accumulation, written from the specification in
 * path_trace_golang_amd/csrc/pt_temporal.h's header comment (and, for the filter stage, pt_atrous.h's FILTER), on the oracle:
 * ora_sample supplies the radiance sums of a frame, ora_exp and C's sqrt and floor the arithmetic, ora_finish_pixel the bytes.  Built
 * at test time (tests/temporal_support.py) with the oracle's flags: no contraction, no fast-math.  Whole-image loops over plain
 * interleaved arrays; nothing here is shared with the product's headers. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "pt_oracle.h"

typedef struct {
    int valid, W, H;
    double cam[12]; /* origin, lower_left, horizontal, vertical */
    double *c, *var, *N, *A, *z;
    int32_t *len;
    unsigned char *hit;
} tr_history;

static void tr_drop(tr_history *h) {
    free(h->c); free(h->var); free(h->N); free(h->A); free(h->z); free(h->len); free(h->hit);
    memset(h, 0, sizeof *h);
}

tr_history *tr_new(void) { return calloc(1, sizeof(tr_history)); }
void tr_free(tr_history *h) {
    if (h) tr_drop(h);
    free(h);
}
void tr_reset(tr_history *h) { h->valid = 0; }

/* the stored history: 0 when it is empty */
int tr_read(const tr_history *h, double *mean, double *var, int32_t *len) {
    if (!h->valid) return 0;
    const size_t np = (size_t)h->W * (size_t)h->H;
    if (mean) memcpy(mean, h->c, np * 3 * sizeof(double));
    if (var) memcpy(var, h->var, np * sizeof(double));
    if (len) memcpy(len, h->len, np * sizeof(int32_t));
    return 1;
}

/* the raw sums of a frame from oracle samples, added in sample order: S, Q [H][W][3] */
void tr_sums(const ora_scene *sc, const ora_config *cfg, double *S, double *Q) {
    for (int32_t y = 0; y < cfg->height; y++)
        for (int32_t x = 0; x < cfg->width; x++) {
            double s[3] = {0, 0, 0}, q[3] = {0, 0, 0};
            for (int32_t k = 0; k < cfg->spp; k++) {
                double l[3];
                uint32_t a, b;
                ora_sample(sc, cfg, x, y, k, l, &a, &b);
                for (int c = 0; c < 3; c++) { s[c] = s[c] + l[c]; q[c] = q[c] + l[c] * l[c]; }
            }
            const size_t i = (size_t)y * (size_t)cfg->width + (size_t)x;
            for (int c = 0; c < 3; c++) { S[3 * i + c] = s[c]; Q[3 * i + c] = q[c]; }
        }
}

static int tr_finite(double x) { return !isnan(x) && !isinf(x); }
static double tr_dot(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

/* steps 3 - 5: 1 and (fx, fy, zexp) when pixel (x, y) has a place in the previous frame */
static int tr_reproject(const double cam[12], const double camh[12], int32_t W, int32_t H, int32_t x, int32_t y, int hit, double z,
                        double *fx, double *fy, double *zexp) {
    const double *org = cam, *ll = cam + 3, *hor = cam + 6, *ver = cam + 9;
    const double *orgh = camh, *llh = camh + 3, *horh = camh + 6, *verh = camh + 9;
    const double inv_w = 1.0 / (double)(W - 1), inv_h = 1.0 / (double)(H - 1);
    const double u = ((double)x + 0.5) * inv_w;
    const double v = (((double)(H - 1) - (double)y) + 0.5) * inv_h;
    double d[3], q[3], e[3], nrm[3], pt[3];
    for (int k = 0; k < 3; k++) d[k] = ((ll[k] + hor[k] * u) + ver[k] * v) - org[k];
    *zexp = 0;
    if (hit) {
        const double s = z / sqrt(tr_dot(d, d));
        for (int k = 0; k < 3; k++) q[k] = (org[k] + d[k] * s) - orgh[k];
        *zexp = sqrt(tr_dot(q, q));
    } else {
        for (int k = 0; k < 3; k++) q[k] = d[k];
    }
    for (int k = 0; k < 3; k++) e[k] = llh[k] - orgh[k];
    nrm[0] = horh[1] * verh[2] - horh[2] * verh[1];
    nrm[1] = horh[2] * verh[0] - horh[0] * verh[2];
    nrm[2] = horh[0] * verh[1] - horh[1] * verh[0];
    const double den = tr_dot(q, nrm), num = tr_dot(e, nrm);
    if (!(den * num > 0)) return 0;
    const double s = num / den;
    for (int k = 0; k < 3; k++) pt[k] = q[k] * s - e[k];
    const double pu = tr_dot(pt, horh) / tr_dot(horh, horh), pv = tr_dot(pt, verh) / tr_dot(verh, verh);
    *fx = pu * (double)(W - 1) - 0.5;
    *fy = ((double)(H - 1) - pv * (double)(H - 1)) + 0.5;
    if (!tr_finite(*fx) || !tr_finite(*fy)) return 0;
    return *fx >= -1 && *fx <= (double)W && *fy >= -1 && *fy <= (double)H;
}

static double tr_figure(const double *c, const double *v, size_t np) {
    double sum = 0;
    for (size_t i = 0; i < np; i++) {
        double den = (c[3 * i] + c[3 * i + 1] + c[3 * i + 2]) / 3;
        if (den < 0.01) den = 0.01;
        const double e2 = v[i] / (den * den);
        if (tr_finite(e2)) sum += e2;
    }
    return sqrt(sum / (double)np);
}

/* One frame through the accumulation.  S, Q, fn, fa, fd: [H][W][3]; cnt: [H][W] or NULL (n for every pixel); cam: this frame's
 * camera.  tcfg = {alpha, tol_z, n_min, tol_a, max_len}.  T < 0: no filter; else T iterations with sig = {sigma_l, sigma_n, sigma_z,
 * sigma_a}.  Outputs (any may be NULL): mean [H][W][3], var [H][W], rgba [H][W][4], noise[3] = before, blended, after,
 * counts[4] = reprojected, disoccluded, bad, sum of len', place [H][W][2] = (fx, fy) of every pixel that has one (NaN otherwise). */
void tr_frame(tr_history *h, int32_t W, int32_t H, const double *S, const double *Q, const uint32_t *cnt, uint32_t n, const double *fn,
              const double *fa, const double *fd, const double cam[12], const double tcfg[5], int32_t T, const double sig[4], double *mean,
              double *var, uint8_t *rgba, double noise[3], uint64_t counts[4], double *place) {
    const size_t np = (size_t)W * (size_t)H;
    double *c = malloc(np * 3 * sizeof(double)), *c2 = malloc(np * 3 * sizeof(double));
    double *v = malloc(np * sizeof(double)), *v2 = malloc(np * sizeof(double));
    double *ci = malloc(np * 3 * sizeof(double)), *vi = malloc(np * sizeof(double));
    double *N = calloc(np * 3, sizeof(double)), *A = calloc(np * 3, sizeof(double)), *z = calloc(np, sizeof(double));
    unsigned char *bad = calloc(np, 1), *hit = calloc(np, 1);
    int32_t *len = calloc(np, sizeof(int32_t));
    const double alpha = tcfg[0], tol_z = tcfg[1], n_min = tcfg[2], tol_a = tcfg[3];
    const int32_t max_len = (int32_t)tcfg[4];
    const int have = h->valid && h->W == W && h->H == H;
    uint64_t nrep = 0, ndis = 0, nbad = 0, lens = 0;
    /* prep (FILTER's) */
    for (size_t i = 0; i < np; i++) {
        const double ni = (double)(cnt ? cnt[i] : n);
        double vs[3];
        int ok = 1;
        for (int k = 0; k < 3; k++) {
            const double m = S[3 * i + k] / ni;
            double d = Q[3 * i + k] / ni - m * m;
            if (d < 0) d = 0;
            vs[k] = d / (ni - 1);
            ci[3 * i + k] = m;
            if (!tr_finite(m)) ok = 0;
        }
        vi[i] = (vs[0] + vs[1] + vs[2]) / 3;
        if (!tr_finite(vi[i])) ok = 0;
        bad[i] = !ok;
        nbad += !ok;
        const double hh = fd[3 * i + 1];
        hit[i] = hh > 0;
        if (hh != 0) {
            for (int k = 0; k < 3; k++) { N[3 * i + k] = fn[3 * i + k] / hh; A[3 * i + k] = fa[3 * i + k] / hh; }
            z[i] = fd[3 * i] / hh;
        }
    }
    /* reproject and blend */
    for (int32_t y = 0; y < H; y++)
        for (int32_t x = 0; x < W; x++) {
            const size_t i = (size_t)y * (size_t)W + (size_t)x;
            for (int k = 0; k < 3; k++) c[3 * i + k] = ci[3 * i + k];
            v[i] = vi[i];
            if (place) place[2 * i] = place[2 * i + 1] = NAN;
            if (bad[i]) { len[i] = 0; continue; }
            len[i] = 1;
            if (!have) continue;
            double fx, fy, zexp;
            int found = tr_reproject(cam, h->cam, W, H, x, y, hit[i], z[i], &fx, &fy, &zexp);
            if (found && place) { place[2 * i] = fx; place[2 * i + 1] = fy; }
            double sw = 0, sc[3] = {0, 0, 0}, sv = 0;
            int32_t L = INT32_MAX;
            if (found) {
                const double x0 = floor(fx), y0 = floor(fy), ax = fx - x0, ay = fy - y0;
                for (int dy = 0; dy < 2; dy++)
                    for (int dx = 0; dx < 2; dx++) {
                        const int32_t xj = (int32_t)x0 + dx, yj = (int32_t)y0 + dy;
                        if (xj < 0 || yj < 0 || xj >= W || yj >= H) continue;
                        const size_t j = (size_t)yj * (size_t)W + (size_t)xj;
                        const double w = (dx ? ax : 1 - ax) * (dy ? ay : 1 - ay);
                        if (h->len[j] <= 0 || h->hit[j] != hit[i] || !(w > 0)) continue;
                        if (hit[i]) {
                            if (!(fabs(h->z[j] - zexp) <= tol_z * zexp)) continue;
                            if (!(tr_dot(N + 3 * i, h->N + 3 * j) >= n_min)) continue;
                            const double dr = A[3 * i] - h->A[3 * j], dg = A[3 * i + 1] - h->A[3 * j + 1], db = A[3 * i + 2] - h->A[3 * j + 2];
                            if (!(dr * dr + dg * dg + db * db <= tol_a * tol_a)) continue;
                        }
                        sw = sw + w;
                        for (int k = 0; k < 3; k++) sc[k] = sc[k] + w * h->c[3 * j + k];
                        sv = sv + (w * w) * h->var[j];
                        if (h->len[j] < L) L = h->len[j];
                    }
            }
            if (!(sw > 0.01)) { ndis++; continue; }
            nrep++;
            const double r = 1.0 / (double)(L + 1), a = alpha > r ? alpha : r;
            const double vr = sv / (sw * sw);
            for (int k = 0; k < 3; k++) {
                const double cr = sc[k] / sw;
                c[3 * i + k] = cr + a * (ci[3 * i + k] - cr);
            }
            v[i] = ((1 - a) * (1 - a)) * vr + (a * a) * vi[i];
            len[i] = L + 1 < max_len ? L + 1 : max_len;
        }
    for (size_t i = 0; i < np; i++) lens += (uint64_t)len[i];
    /* the new history: the blended state, before any filtering */
    if (!have) {
        tr_drop(h);
        h->W = W; h->H = H;
        h->c = malloc(np * 3 * sizeof(double)); h->var = malloc(np * sizeof(double));
        h->N = malloc(np * 3 * sizeof(double)); h->A = malloc(np * 3 * sizeof(double)); h->z = malloc(np * sizeof(double));
        h->len = malloc(np * sizeof(int32_t)); h->hit = malloc(np);
    }
    memcpy(h->c, c, np * 3 * sizeof(double)); memcpy(h->var, v, np * sizeof(double));
    memcpy(h->N, N, np * 3 * sizeof(double)); memcpy(h->A, A, np * 3 * sizeof(double)); memcpy(h->z, z, np * sizeof(double));
    memcpy(h->len, len, np * sizeof(int32_t)); memcpy(h->hit, hit, np);
    memcpy(h->cam, cam, 12 * sizeof(double));
    h->valid = 1;
    if (noise) { noise[0] = tr_figure(ci, vi, np); noise[1] = tr_figure(c, v, np); }
    /* the filter stage: FILTER's iterations on (c', var') with this frame's guide */
    if (T >= 0) {
        static const double B[5] = {1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16};
        const int n_on = sig[1] > 0, z_on = sig[2] > 0, a_on = sig[3] > 0;
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
                                const double q = 1 - tr_dot(N + 3 * i, N + 3 * j);
                                pen = pen + (q > 0 ? q : 0) / sig[1];
                            }
                            if (z_on) pen = pen + fabs(z[i] - z[j]) / (sig[2] * (z[i] > 1e-8 ? z[i] : 1e-8));
                            if (a_on) {
                                const double dr = A[3 * i] - A[3 * j], dg = A[3 * i + 1] - A[3 * j + 1], db = A[3 * i + 2] - A[3 * j + 2];
                                pen = pen + (dr * dr + dg * dg + db * db) / (sig[3] * sig[3]);
                            }
                            const double w = (B[dy + 2] * B[dx + 2]) * ora_exp(-pen);
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
    if (noise) noise[2] = tr_figure(c, v, np);
    for (size_t i = 0; i < np; i++) {
        if (mean) for (int k = 0; k < 3; k++) mean[3 * i + k] = c[3 * i + k];
        if (var) var[i] = v[i];
        if (rgba) {
            ora_finish_pixel(c + 3 * i, 1, rgba + 4 * i);
            rgba[4 * i + 3] = 255;
        }
    }
    if (counts) { counts[0] = nrep; counts[1] = ndis; counts[2] = nbad; counts[3] = lens; }
    free(c); free(c2); free(v); free(v2); free(ci); free(vi); free(N); free(A); free(z); free(bad); free(hit); free(len);
}
