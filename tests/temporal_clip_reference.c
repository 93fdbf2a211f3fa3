/* temporal_clip_reference.c -- independent CPU restatement of the temporal accumulation WITH the history clip (step 7a), written
 * from the specification in path_trace_golang_amd/csrc/pt_temporal.h's header comment (and, for the filter stage, pt_atrous.h's
 * FILTER), on the oracle: ora_exp and C's sqrt and floor supply the arithmetic, ora_finish_pixel the bytes.  Built at test time
 * (tests/temporal_clip_support.py) with the oracle's flags: no contraction, no fast-math.  One function per step of the
 * specification, on plain interleaved arrays; nothing here is shared with the product's headers or with temporal_reference.c,
 * which stays as the statement of the model without the clip. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "pt_oracle.h"

typedef struct {
    int valid;
    int32_t W, H;
    double org[3], ll[3], hor[3], ver[3];
    double *mean;  /* [np][3] */
    double *var;   /* [np] */
    double *nrm;   /* [np][3] */
    double *alb;   /* [np][3] */
    double *dist;  /* [np] */
    int32_t *len;  /* [np] */
    uint8_t *hit;  /* [np] */
} trc_history;

typedef struct {
    double c[3], var, N[3], A[3], z;
    int bad, hit;
} trc_pixel;

static void trc_release(trc_history *h) {
    free(h->mean); free(h->var); free(h->nrm); free(h->alb); free(h->dist); free(h->len); free(h->hit);
    h->mean = h->var = h->nrm = h->alb = h->dist = NULL;
    h->len = NULL;
    h->hit = NULL;
}

trc_history *trc_new(void) { return calloc(1, sizeof(trc_history)); }

void trc_free(trc_history *h) {
    if (!h) return;
    trc_release(h);
    free(h);
}

void trc_reset(trc_history *h) { h->valid = 0; }

int trc_read(const trc_history *h, double *mean, double *var, int32_t *len) {
    if (!h->valid) return 0;
    const size_t np = (size_t)h->W * (size_t)h->H;
    for (size_t i = 0; i < np; i++) {
        if (mean) { mean[3 * i] = h->mean[3 * i]; mean[3 * i + 1] = h->mean[3 * i + 1]; mean[3 * i + 2] = h->mean[3 * i + 2]; }
        if (var) var[i] = h->var[i];
        if (len) len[i] = h->len[i];
    }
    return 1;
}

static int is_number(double x) { return x == x && x != INFINITY && x != -INFINITY; }
static double dot(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

/* CURRENT FRAME: FILTER's prep of one pixel */
static void prep(const double S[3], const double Q[3], uint32_t count, const double fn[3], const double fa[3], const double fd[3], trc_pixel *p) {
    const double n = (double)count;
    double v[3];
    memset(p, 0, sizeof *p);
    for (int k = 0; k < 3; k++) {
        p->c[k] = S[k] / n;
        double e = Q[k] / n - p->c[k] * p->c[k];
        if (e < 0) e = 0;
        v[k] = e / (n - 1);
    }
    p->var = (v[0] + v[1] + v[2]) / 3;
    p->bad = !(is_number(p->c[0]) && is_number(p->c[1]) && is_number(p->c[2]) && is_number(p->var));
    const double h = fd[1];
    p->hit = h > 0;
    if (h != 0) {
        for (int k = 0; k < 3; k++) { p->N[k] = fn[k] / h; p->A[k] = fa[k] / h; }
        p->z = fd[0] / h;
    }
}

/* step 3: the centre ray of pixel (x, y) */
static void centre_ray(const double org[3], const double ll[3], const double hor[3], const double ver[3], int32_t W, int32_t H, int32_t x,
                       int32_t y, double d[3]) {
    const double inv_width = 1.0 / (double)(W - 1), inv_height = 1.0 / (double)(H - 1);
    const double u = ((double)x + 0.5) * inv_width;
    const double v = (((double)(H - 1) - (double)y) + 0.5) * inv_height;
    for (int k = 0; k < 3; k++) {
        const double a = (ll[k] + hor[k] * u) + ver[k] * v;
        d[k] = a - org[k];
    }
}

/* steps 4 and 5: 1 when the pixel has a place (fx, fy) in the previous frame */
static int place_in_previous(const trc_history *h, const double org[3], const double d[3], const trc_pixel *p, double *fx, double *fy, double *zexp) {
    double q[3], e[3], nrm[3], pt[3];
    *zexp = 0;
    if (p->hit) {
        const double t = p->z / sqrt(dot(d, d));
        for (int k = 0; k < 3; k++) {
            const double P = org[k] + d[k] * t;
            q[k] = P - h->org[k];
        }
        *zexp = sqrt(dot(q, q));
    } else {
        q[0] = d[0]; q[1] = d[1]; q[2] = d[2];
    }
    for (int k = 0; k < 3; k++) e[k] = h->ll[k] - h->org[k];
    nrm[0] = h->hor[1] * h->ver[2] - h->hor[2] * h->ver[1];
    nrm[1] = h->hor[2] * h->ver[0] - h->hor[0] * h->ver[2];
    nrm[2] = h->hor[0] * h->ver[1] - h->hor[1] * h->ver[0];
    const double den = dot(q, nrm), num = dot(e, nrm);
    if (!(den * num > 0)) return 0;
    const double s = num / den;
    for (int k = 0; k < 3; k++) pt[k] = q[k] * s - e[k];
    const double pu = dot(pt, h->hor) / dot(h->hor, h->hor);
    const double pv = dot(pt, h->ver) / dot(h->ver, h->ver);
    const double wm1 = (double)(h->W - 1), hm1 = (double)(h->H - 1);
    *fx = pu * wm1 - 0.5;
    *fy = (hm1 - pv * hm1) + 0.5;
    if (!is_number(*fx) || !is_number(*fy)) return 0;
    if (*fx < -1 || *fx > (double)h->W || *fy < -1 || *fy > (double)h->H) return 0;
    return 1;
}

/* steps 6 and 7: the valid taps gathered; 1 when sw > 0.01, with c_r, var_r and L */
static int gather(const trc_history *h, const trc_pixel *p, double fx, double fy, double zexp, double tol_z, double n_min, double tol_a,
                  double cr[3], double *vr, int32_t *L) {
    const double x0 = floor(fx), y0 = floor(fy);
    const double ax = fx - x0, ay = fy - y0;
    double sw = 0, sc[3] = {0, 0, 0}, sv = 0;
    int32_t least = INT32_MAX;
    for (int dy = 0; dy <= 1; dy++)
        for (int dx = 0; dx <= 1; dx++) {
            const int64_t xj = (int64_t)x0 + dx, yj = (int64_t)y0 + dy;
            if (xj < 0 || xj >= h->W || yj < 0 || yj >= h->H) continue;
            const size_t j = (size_t)yj * (size_t)h->W + (size_t)xj;
            const double wx = dx ? ax : 1 - ax, wy = dy ? ay : 1 - ay;
            const double w = wx * wy;
            if (!(h->len[j] > 0)) continue;
            if ((h->hit[j] != 0) != (p->hit != 0)) continue;
            if (!(w > 0)) continue;
            if (p->hit) {
                if (!(fabs(h->dist[j] - zexp) <= tol_z * zexp)) continue;
                if (!(dot(p->N, h->nrm + 3 * j) >= n_min)) continue;
                const double dr = p->A[0] - h->alb[3 * j], dg = p->A[1] - h->alb[3 * j + 1], db = p->A[2] - h->alb[3 * j + 2];
                if (!(dr * dr + dg * dg + db * db <= tol_a * tol_a)) continue;
            }
            sw = sw + w;
            for (int k = 0; k < 3; k++) sc[k] = sc[k] + w * h->mean[3 * j + k];
            sv = sv + (w * w) * h->var[j];
            if (h->len[j] < least) least = h->len[j];
        }
    if (!(sw > 0.01)) return 0;
    for (int k = 0; k < 3; k++) cr[k] = sc[k] / sw;
    *vr = sv / (sw * sw);
    *L = least;
    return 1;
}

/* step 7a: the history clipped to what the frame allows; 1 when any channel changed */
static int clip(double gamma, const double ci[3], double var_i, double var_r, double cr[3]) {
    if (!(gamma > 0)) return 0;
    const double s = var_i + var_r;
    const double half = gamma * sqrt(s > 0 ? s : 0);
    int changed = 0;
    for (int k = 0; k < 3; k++) {
        const double lo = ci[k] - half, hi = ci[k] + half;
        if (cr[k] < lo) { cr[k] = lo; changed = 1; }
        else if (cr[k] > hi) { cr[k] = hi; changed = 1; }
    }
    return changed;
}

static double figure(const double *c, const double *v, size_t np) {
    double sum = 0;
    for (size_t i = 0; i < np; i++) {
        double den = (c[3 * i] + c[3 * i + 1] + c[3 * i + 2]) / 3;
        if (den < 0.01) den = 0.01;
        const double e2 = v[i] / (den * den);
        if (is_number(e2)) sum += e2;
    }
    return sqrt(sum / (double)np);
}

/* FILTER's iteration t on (c, v) -> (c2, v2) */
static void filter_pass(const trc_pixel *px, int32_t W, int32_t H, int32_t step, const double sig[4], const double *c, const double *v,
                        double *c2, double *v2) {
    static const double B[5] = {1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16};
    for (int32_t y = 0; y < H; y++)
        for (int32_t x = 0; x < W; x++) {
            const size_t i = (size_t)y * (size_t)W + (size_t)x;
            if (px[i].bad) {
                for (int k = 0; k < 3; k++) c2[3 * i + k] = c[3 * i + k];
                v2[i] = v[i];
                continue;
            }
            const double li = (c[3 * i] + c[3 * i + 1] + c[3 * i + 2]) / 3;
            double sw = 0, sc[3] = {0, 0, 0}, sv = 0;
            for (int dy = -2; dy <= 2; dy++)
                for (int dx = -2; dx <= 2; dx++) {
                    const int32_t xj = x + dx * step, yj = y + dy * step;
                    if (xj < 0 || xj >= W || yj < 0 || yj >= H) continue;
                    const size_t j = (size_t)yj * (size_t)W + (size_t)xj;
                    if (px[j].bad) continue;
                    const double lj = (c[3 * j] + c[3 * j + 1] + c[3 * j + 2]) / 3;
                    double pen = fabs(li - lj) / (sig[0] * sqrt(v[i]) + 1e-8);
                    if (sig[1] > 0) {
                        const double q = 1 - dot(px[i].N, px[j].N);
                        pen = pen + (q > 0 ? q : 0) / sig[1];
                    }
                    if (sig[2] > 0) pen = pen + fabs(px[i].z - px[j].z) / (sig[2] * (px[i].z > 1e-8 ? px[i].z : 1e-8));
                    if (sig[3] > 0) {
                        const double dr = px[i].A[0] - px[j].A[0], dg = px[i].A[1] - px[j].A[1], db = px[i].A[2] - px[j].A[2];
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
}

/* One frame.  S, Q, fn, fa, fd: [H][W][3]; cnt: [H][W] or NULL (n everywhere); cam: origin, lower_left, horizontal, vertical.
 * tcfg = {alpha, tol_z, n_min, tol_a, max_len, gamma}.  T < 0: no filter; else T iterations with sig = {sigma_l, sigma_n, sigma_z,
 * sigma_a}.  Outputs (any may be NULL): mean [H][W][3], var [H][W], rgba [H][W][4], noise[3] = before, blended, after;
 * counts[5] = reprojected, disoccluded, bad, the sum of len', clipped; place [H][W][2] = (fx, fy) or NaN;
 * repro [H][W][5] = of a reprojected pixel c_r (three channels, as step 7 leaves them: before the clip), var_r and the blend
 * weight a; NaN elsewhere. */
void trc_frame(trc_history *h, int32_t W, int32_t H, const double *S, const double *Q, const uint32_t *cnt, uint32_t n, const double *fn,
               const double *fa, const double *fd, const double cam[12], const double tcfg[6], int32_t T, const double sig[4], double *mean,
               double *var, uint8_t *rgba, double noise[3], uint64_t counts[5], double *place, double *repro) {
    const size_t np = (size_t)W * (size_t)H;
    const double alpha = tcfg[0], tol_z = tcfg[1], n_min = tcfg[2], tol_a = tcfg[3], gamma = tcfg[5];
    const int32_t max_len = (int32_t)tcfg[4];
    const int have = h->valid && h->W == W && h->H == H;
    trc_pixel *px = malloc(np * sizeof *px);
    double *ci = malloc(np * 3 * sizeof(double)), *vi = malloc(np * sizeof(double));
    double *c = malloc(np * 3 * sizeof(double)), *v = malloc(np * sizeof(double));
    double *c2 = malloc(np * 3 * sizeof(double)), *v2 = malloc(np * sizeof(double));
    int32_t *len = malloc(np * sizeof(int32_t));
    uint64_t nrep = 0, ndis = 0, nbad = 0, nclip = 0, lens = 0;
    for (size_t i = 0; i < np; i++) {
        prep(S + 3 * i, Q + 3 * i, cnt ? cnt[i] : n, fn + 3 * i, fa + 3 * i, fd + 3 * i, &px[i]);
        for (int k = 0; k < 3; k++) ci[3 * i + k] = px[i].c[k];
        vi[i] = px[i].var;
    }
    for (int32_t y = 0; y < H; y++)
        for (int32_t x = 0; x < W; x++) {
            const size_t i = (size_t)y * (size_t)W + (size_t)x;
            const trc_pixel *p = &px[i];
            for (int k = 0; k < 3; k++) c[3 * i + k] = p->c[k];
            v[i] = p->var;
            if (place) place[2 * i] = place[2 * i + 1] = NAN;
            if (repro) for (int k = 0; k < 5; k++) repro[5 * i + k] = NAN;
            if (p->bad) { len[i] = 0; nbad++; continue; }        /* step 1 */
            len[i] = 1;
            if (!have) continue;                                  /* step 2 */
            double d[3], fx, fy, zexp, cr[3], vr;
            int32_t L;
            centre_ray(cam, cam + 3, cam + 6, cam + 9, W, H, x, y, d);
            int found = place_in_previous(h, cam, d, p, &fx, &fy, &zexp);
            if (found && place) { place[2 * i] = fx; place[2 * i + 1] = fy; }
            if (found) found = gather(h, p, fx, fy, zexp, tol_z, n_min, tol_a, cr, &vr, &L);
            if (!found) { ndis++; continue; }
            nrep++;
            const double r = 1.0 / (double)(L + 1);
            const double a = alpha > r ? alpha : r;
            if (repro) { repro[5 * i] = cr[0]; repro[5 * i + 1] = cr[1]; repro[5 * i + 2] = cr[2]; repro[5 * i + 3] = vr; repro[5 * i + 4] = a; }
            nclip += (uint64_t)clip(gamma, p->c, p->var, vr, cr);  /* step 7a */
            for (int k = 0; k < 3; k++) c[3 * i + k] = cr[k] + a * (p->c[k] - cr[k]);
            v[i] = ((1 - a) * (1 - a)) * vr + (a * a) * p->var;
            len[i] = L + 1 < max_len ? L + 1 : max_len;
        }
    /* step 9 */
    if (!have) {
        trc_release(h);
        h->W = W; h->H = H;
        h->mean = malloc(np * 3 * sizeof(double)); h->var = malloc(np * sizeof(double));
        h->nrm = malloc(np * 3 * sizeof(double)); h->alb = malloc(np * 3 * sizeof(double)); h->dist = malloc(np * sizeof(double));
        h->len = malloc(np * sizeof(int32_t)); h->hit = malloc(np);
    }
    for (size_t i = 0; i < np; i++) {
        for (int k = 0; k < 3; k++) { h->mean[3 * i + k] = c[3 * i + k]; h->nrm[3 * i + k] = px[i].N[k]; h->alb[3 * i + k] = px[i].A[k]; }
        h->var[i] = v[i];
        h->dist[i] = px[i].z;
        h->len[i] = len[i];
        h->hit[i] = (uint8_t)px[i].hit;
        lens += (uint64_t)len[i];
    }
    for (int k = 0; k < 3; k++) { h->org[k] = cam[k]; h->ll[k] = cam[3 + k]; h->hor[k] = cam[6 + k]; h->ver[k] = cam[9 + k]; }
    h->valid = 1;
    if (noise) { noise[0] = figure(ci, vi, np); noise[1] = figure(c, v, np); }
    for (int32_t t = 0; t < T; t++) {
        filter_pass(px, W, H, 1 << t, sig, c, v, c2, v2);
        double *sw = c; c = c2; c2 = sw;
        sw = v; v = v2; v2 = sw;
    }
    if (noise) noise[2] = figure(c, v, np);
    for (size_t i = 0; i < np; i++) {
        if (mean) for (int k = 0; k < 3; k++) mean[3 * i + k] = c[3 * i + k];
        if (var) var[i] = v[i];
        if (rgba) {
            ora_finish_pixel(c + 3 * i, 1, rgba + 4 * i);
            rgba[4 * i + 3] = 255;
        }
    }
    if (counts) { counts[0] = nrep; counts[1] = ndis; counts[2] = nbad; counts[3] = lens; counts[4] = nclip; }
    free(px); free(ci); free(vi); free(c); free(v); free(c2); free(v2); free(len);
}
