// pt_atrous.h -- first-hit feature planes (pt_set_features) and the variance-guided a-trous filter (pt_atrous), host + device.
//
// Opt-in per context; with both off nothing here is allocated or launched.  Everything is PT_HD and built from IEEE +,-,*,/, sqrt
// and the Go routines of pt_math.h (compile with -ffp-contract=off), so the gfx950 kernels (feature_kernel, atrous_prep_kernel,
// atrous_kernel, atrous_finish_kernel in pt_kernels.h) and a host build of this header give the same bits.  This comment is the
// specification tests/atrous_reference.c restates.  Every sum below is written in its order of evaluation: a + b + c means (a + b) + c.
//
// FEATURES.  Per pixel, over its samples with index s < k, the first hit of the sample's primary ray (o, d): the CPU engine's closest
// hit of the first segment -- exact FP64 tests, tMin 0.001, tMax = the closest t so far, objects in file order (ptf::closest_hit).
// Three sums of three doubles, added in sample order from zero:
//   normal += the hit record's face-forward normal (objects.go:17-24, :37-222): n_out if d . n_out < 0, else -n_out, with
//             sphere  p = o + d*t per component, n_out = (p - centre) * (1 / radius)
//             plane   n_out = the plane's normal, front face when denom = normal . d < 0
//             box     p = o + d*t; of dxMin = p.x - min.x, dxMax = max.x - p.x, dyMin, dyMax, dzMin, dzMax the first strictly smallest
//                     names the axis normal (-1,0,0), (1,0,0), (0,-1,0), ...
//   albedo += the converted material's albedo (materials.go:28-55; emissive and missing materials: 0)
//   depth  += (t * sqrt(d.x*d.x + d.y*d.y + d.z*d.z), 1, 0) on a hit, and depth[2] += 1 for every feature sample taken
// A miss adds nothing to normal, albedo, depth[0] and depth[1].
//
// FILTER.  Inputs per in-frame pixel: its sample count n >= 2, the raw sums S (radiance) and Q (squared radiance) per channel, and --
// when the frame has features -- the sums above.  Configuration: T iterations (0..6), sigma_l > 0, sigma_n, sigma_z, sigma_a >= 0; a
// feature term is ON when its sigma is > 0 and the frame has features.
//   Prep:  c_k = S_k / n;  m_k = Q_k / n - c_k * c_k, a negative m_k counts as 0 (a NaN stays);  v_k = m_k / (n - 1);
//          var = (v_r + v_g + v_b) / 3.   The pixel is BAD when some c_k or var is NaN or infinite.
//          With h = depth[1] (samples that hit): N = normal / h, A = albedo / h, z = depth[0] / h, per component; all 0 when h = 0
//          or the frame has no features.  N is not renormalised.
//   Iteration t = 0 .. T-1, step = 2^t, from (c, var) to (c', var'), all pixels at once (ping-pong):
//          a bad pixel keeps its c and var.  A good pixel i = (x, y) visits its 25 taps j = (x + dx*step, y + dy*step), dy outer and
//          dx inner, both from -2 to 2; a tap outside the frame or on a bad pixel is skipped.  With l = (c_r + c_g + c_b) / 3,
//          B = [1/16, 1/4, 3/8, 1/4, 1/16]:
//              pen = |l_i - l_j| / (sigma_l * sqrt(var_i) + 1e-8)
//              if N on:  pen = pen + pos(1 - (N_i.x*N_j.x + N_i.y*N_j.y + N_i.z*N_j.z)) / sigma_n       pos(v) = v > 0 ? v : 0
//              if z on:  pen = pen + |z_i - z_j| / (sigma_z * (z_i > 1e-8 ? z_i : 1e-8))
//              if A on:  pen = pen + (dr*dr + dg*dg + db*db) / (sigma_a * sigma_a),  (dr, dg, db) = A_i - A_j
//              w = (B[dy+2] * B[dx+2]) * go_exp(-pen);  a tap whose pen is > 745.2 has w = 0 (go_exp returns exactly 0 below
//                  -745.133..., so skipping the call and the tap gives the same bits: every c_j and var_j of a tap is finite)
//              sw = sw + w;  sd_k = sd_k + w * (c_j,k - c_i,k);  sv = sv + (w * w) * var_j           (all from 0)
//          c'_k = c_i,k + sd_k / sw;  var' = sv / (sw * sw).   The centre tap has pen = 0 and w = 9/64, so sw > 0.  (The weighted
//          mean sum(w c_j) / sum(w), taken about c_i: a constant image with zero variance is unchanged bit for bit.)
//   Finish: byte_k = quantise(sqrt(c_k) * 255.999) -- the CPU engine's finish (renderer.go:190-221) of c as a 1-sample sum: below 0
//          -> 0, above 255.999 -> 255.999, NaN -> 0, truncate; A = 255.
//   Noise figure of a state (c, var): sqrt(sum over the pixels of e2 / pixels), e2 = var / den^2, den = l < 0.01 ? 0.01 : l; a NaN or
//          infinite e2 adds 0.  Before the first iteration this is pt_noise_estimate's figure.  (The order of that one sum is the
//          reduction tree's, not specified here: compare to 1e-9.)
//
// HALVES (pt_set_halves, pt_atrous_halves).  Sample s of a pixel (its 0-based index within the pixel) belongs to half A when s is even
// and to half B when it is odd.  Per pixel and channel four raw sums, each added in sample order from zero: SA = sum of L and
// QA = sum of L*L over A, SB and QB over B, L the radiance record the frame's sum adds (after the fog term).  With the pixel's own
// count n: nA = (n + 1) / 2 and nB = n / 2 in integer division; every pixel holds n >= 4.
//   Each half is a frame of its own:  fA, varA' = FILTER (prep, T iterations) on (SA, QA, nA) and the frame's feature sums,
//          fB, varB' = FILTER on (SB, QB, nB) and the same feature sums.  A pixel can be bad in one half only; a half passes its own
//          bad pixels through and skips them as taps, exactly as FILTER says.
//   Combine, per pixel:  mean_k = (fA_k + fB_k) * 0.5;  d_k = (fA_k - fB_k) * 0.5;  err = (d_r*d_r + d_g*d_g + d_b*d_b) / 3;
//          l = (mean_r + mean_g + mean_b) / 3;  den = l < 0.01 ? 0.01 : l;  e2 = err / (den * den);
//          e2_model = ((varA' + varB') * 0.25) / (den * den).
//          err is a one-degree-of-freedom estimate of the variance of mean: meaningful only averaged over many pixels.
//   Figures:  noise = sqrt(sum of e2 / pixels), noise_model = sqrt(sum of e2_model / pixels).  A pixel that is bad in either half, or
//          whose e2 is NaN or infinite, adds 0 to both sums and is counted as bad; a NaN or infinite e2_model adds 0.  (The order of
//          the two sums is the reduction tree's: compare to 1e-9.)  Neither figure sees the bias the filter adds.
//
// BLOCKS (pt_set_adaptive_filtered).  The stop rule of an adaptive frame (pt_set_adaptive) taken from the filtered frame's
// noise instead of the block's own.  The frame is adaptive in every respect (active lists, job map, per-pixel counts) and collects the
// half sums by itself.  At the end of a pt_step, once done >= max(min_spp, 4) samples (every pixel then holds at least 4), in this order:
//   1. Pair filter:  HALVES above on the frame as it stands, every pixel with its own count, the frame's feature sums if it has them:
//          per pixel mean, err and the bad mask (0..3).
//   2. Per-block sum, per 8x8 block B = (bx, by) = (x >> 3, y >> 3) of the frame's grid of nbx = (W + 7) / 8 by nby = (H + 7) / 8 blocks
//          (the sub-blocks of the 32x32 tiles):  k_B = its pixels inside the frame;  s_B = the sum over them of Combine's e2 (a pixel
//          that is bad in either half, or whose e2 is NaN or infinite, adds 0 and still counts in k_B).  The 64 terms, lane = row * 8 +
//          column inside the block and 0 for a lane outside the frame, are added by the xor butterfly: for off = 32, 16, 8, 4, 2, 1
//          every lane adds lane ^ off's value to its own; s_B is lane 0's.
//   3. Pooled figure:  P_B = sqrt(ss / kk), ss = the sum of s_B' and kk = the sum of k_B' over the blocks B' of the grid with
//          |bx' - bx| <= r and |by' - by| <= r, taken sequentially from zero, rows top to bottom and left to right within a row; kk is an
//          integer, converted once.  r = the pool radius in blocks (0..4, default 1).  Blocks that have stopped are in the window with
//          the samples they hold.  The block's own figure, for reading: own_B = sqrt(s_B / k_B).
//   4. Decision:  every still-active block with P_B <= target becomes inactive and stays so.
// Before that count no block stops.  Unlike pt_set_adaptive's rule, neighbouring blocks DO keep each other alive: a block whose own
// figure is below the target goes on while the window around it is not -- err has one degree of freedom per pixel, and 64 of them
// decide nothing at the counts where blocks stop.  Which blocks stop depends on the step sizes and on nothing else.
#pragma once

#include <stdint.h>

#include "pt_device.h"
#include "pt_fog.h"
#include "pt_math.h"

namespace pta {

#define PTA_MAX_ITERATIONS 6
#define PTA_PEN_CUT 745.2  // go_exp(-pen) == 0 for every pen above this

// ---------------------------------------------------------------- features

// The feature record of the hit of the ray (o, d) on objs[best] at parameter t: n = the face-forward normal, a = the albedo of the
// object's converted material, dist = t * |d|.  The one statement of the record: first_hit and the BVH walk's kernels
// (pt_feature_walk.h) both end here.
PT_HD void hit_record(const ptd::DevObj *objs, const ptd::DevMat *mats, int32_t best, double t, const double o[3], const double d[3], double n[3],
                      double a[3], double &dist) {
    const ptd::DevObj &ob = objs[best];
    const int kind = ob.kind & 0xff;
    double nx, ny, nz;
    bool front;
    if (kind == ptd::KIND_SPHERE) {
        const double px = o[0] + d[0] * t, py = o[1] + d[1] * t, pz = o[2] + d[2] * t;
        nx = (px - ob.a[0]) * ob.inv_radius;
        ny = (py - ob.a[1]) * ob.inv_radius;
        nz = (pz - ob.a[2]) * ob.inv_radius;
        front = d[0] * nx + d[1] * ny + d[2] * nz < 0;
    } else if (kind == ptd::KIND_PLANE) {
        nx = ob.b[0]; ny = ob.b[1]; nz = ob.b[2];
        front = ob.b[0] * d[0] + ob.b[1] * d[1] + ob.b[2] * d[2] < 0;
    } else {
        const double px = o[0] + d[0] * t, py = o[1] + d[1] * t, pz = o[2] + d[2] * t;
        double m = px - ob.a[0];
        nx = -1; ny = 0; nz = 0;
        double v = ob.b[0] - px;
        if (v < m) { m = v; nx = 1; ny = 0; nz = 0; }
        v = py - ob.a[1];
        if (v < m) { m = v; nx = 0; ny = -1; nz = 0; }
        v = ob.b[1] - py;
        if (v < m) { m = v; nx = 0; ny = 1; nz = 0; }
        v = pz - ob.a[2];
        if (v < m) { m = v; nx = 0; ny = 0; nz = -1; }
        v = ob.b[2] - pz;
        if (v < m) { nx = 0; ny = 0; nz = 1; }
        front = d[0] * nx + d[1] * ny + d[2] * nz < 0;
    }
    n[0] = front ? nx : -nx;
    n[1] = front ? ny : -ny;
    n[2] = front ? nz : -nz;
    const ptd::DevMat &mt = mats[ob.mat];
    a[0] = mt.albedo[0]; a[1] = mt.albedo[1]; a[2] = mt.albedo[2];
    dist = t * ptm::f_sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
}

// The first hit of the primary ray (o, d) against the world: false on a miss; n, a, dist = the hit's record (hit_record); *index
// (when asked for) = the winner's index into objs, -1 on a miss.
PT_HD bool first_hit(const ptd::DevObj *objs, const ptd::DevMat *mats, int32_t nobj, const double o[3], const double d[3], double n[3],
                     double a[3], double &dist, int32_t *index = nullptr) {
    const ptf::FRay r = ptf::make_fray(o[0], o[1], o[2], d[0], d[1], d[2]);
    double t;
    int32_t best;
    const bool any = ptf::closest_hit(objs, nobj, r, t, best);
    if (index) *index = best;
    if (!any) return false;
    hit_record(objs, mats, best, t, o, d, n, a, dist);
    return true;
}

// ---------------------------------------------------------------- filter

struct Params {
    double sigma_l, sigma_n, sigma_z, sigma_a;
    int32_t iterations;
    int32_t n_on, z_on, a_on;  // the feature terms that are on (sigma > 0 and the frame has features)
};

// Guide record of a pixel, read-only through the iterations: N, A, z and the bad flag (as a double: 0 good, 1 bad).
struct Guide {
    double n[3], a[3], z, bad;
};

PT_HD bool finite(double x) { return x - x == 0.0; }

// Prep of one pixel: S, Q raw sums, cnt samples (>= 2); fn / fa / fd the feature sums or null.
PT_HD void prep_pixel(const double S[3], const double Q[3], uint32_t cnt, const double *fn, const double *fa, const double *fd,
                      double c[3], double &var, Guide &g) {
    const double n = (double)cnt, n1 = (double)(cnt - 1u);
    double vsum = 0.0;
    bool ok = true;
    for (int k = 0; k < 3; k++) {
        c[k] = S[k] / n;
        double m = Q[k] / n - c[k] * c[k];
        if (m < 0.0) m = 0.0;  // (a NaN stays a NaN)
        vsum += m / n1;
        ok = ok && finite(c[k]);
    }
    var = vsum / 3.0;
    ok = ok && finite(var);
    g.bad = ok ? 0.0 : 1.0;
    const double h = fd ? fd[1] : 0.0;
    if (h != 0.0) {
        for (int k = 0; k < 3; k++) { g.n[k] = fn[k] / h; g.a[k] = fa[k] / h; }
        g.z = fd[0] / h;
    } else {
        for (int k = 0; k < 3; k++) g.n[k] = g.a[k] = 0.0;
        g.z = 0.0;
    }
}

// One iteration at pixel (x, y) of a W x H frame: col [W*H][3], var [W*H], guide [W*H] -> the pixel's c', var'.
PT_HD void filter_pixel(const Params &P, int32_t W, int32_t H, int32_t x, int32_t y, int32_t step, const double *__restrict__ col,
                        const double *__restrict__ var, const Guide *__restrict__ guide, double co[3], double &vo) {
    const size_t i = (size_t)y * (size_t)W + (size_t)x;
    const Guide gi = guide[i];
    const double ci0 = col[3 * i], ci1 = col[3 * i + 1], ci2 = col[3 * i + 2], vi = var[i];
    if (gi.bad != 0.0) {
        co[0] = ci0; co[1] = ci1; co[2] = ci2;
        vo = vi;
        return;
    }
    const double li = (ci0 + ci1 + ci2) / 3.0;
    const double den_l = P.sigma_l * ptm::f_sqrt(vi) + 1e-8;
    const double den_z = P.sigma_z * (gi.z > 1e-8 ? gi.z : 1e-8);
    const double den_a = P.sigma_a * P.sigma_a;
    const double B[5] = {0.0625, 0.25, 0.375, 0.25, 0.0625};
    double sw = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0, sv = 0.0;
    for (int dy = -2; dy <= 2; dy++) {
        const int32_t yj = y + dy * step;
        if (yj < 0 || yj >= H) continue;
        for (int dx = -2; dx <= 2; dx++) {
            const int32_t xj = x + dx * step;
            if (xj < 0 || xj >= W) continue;
            const size_t j = (size_t)yj * (size_t)W + (size_t)xj;
            const Guide &gj = guide[j];
            if (gj.bad != 0.0) continue;
            const double cj0 = col[3 * j], cj1 = col[3 * j + 1], cj2 = col[3 * j + 2];
            const double lj = (cj0 + cj1 + cj2) / 3.0;
            double pen = ptm::f_abs(li - lj) / den_l;
            if (P.n_on) {
                const double q = 1.0 - (gi.n[0] * gj.n[0] + gi.n[1] * gj.n[1] + gi.n[2] * gj.n[2]);
                pen = pen + (q > 0.0 ? q : 0.0) / P.sigma_n;
            }
            if (P.z_on) pen = pen + ptm::f_abs(gi.z - gj.z) / den_z;
            if (P.a_on) {
                const double dr = gi.a[0] - gj.a[0], dg = gi.a[1] - gj.a[1], db = gi.a[2] - gj.a[2];
                pen = pen + (dr * dr + dg * dg + db * db) / den_a;
            }
            if (pen > PTA_PEN_CUT) continue;  // w = 0 exactly: adds nothing
            const double w = (B[dy + 2] * B[dx + 2]) * ptm::go_exp(-pen);
            sw = sw + w;
            s0 = s0 + w * (cj0 - ci0);
            s1 = s1 + w * (cj1 - ci1);
            s2 = s2 + w * (cj2 - ci2);
            sv = sv + (w * w) * var[j];
        }
    }
    co[0] = ci0 + s0 / sw;
    co[1] = ci1 + s1 / sw;
    co[2] = ci2 + s2 / sw;
    vo = sv / (sw * sw);
}

// The finish of one channel: the byte of the CPU engine for a mean c.
PT_HD uint32_t finish_byte(double c) {
    double v = ptm::f_sqrt(c) * 255.999;
    if (v < 0) v = 0;
    else if (v > 255.999) v = 255.999;
    if (v != v) return 0;
    return (uint32_t)v;
}
PT_HD uint32_t finish_pack(const double c[3]) { return finish_byte(c[0]) | (finish_byte(c[1]) << 8) | (finish_byte(c[2]) << 16) | (255u << 24); }

// The noise term of one pixel; a NaN or infinite one is returned as 0.
PT_HD double noise_term(const double c[3], double var) {
    double den = (c[0] + c[1] + c[2]) / 3.0;
    if (den < 0.01) den = 0.01;
    const double e2 = var / (den * den);
    return finite(e2) ? e2 : 0.0;
}

// ---------------------------------------------------------------- pair filter (HALVES above)

// The plane-per-component layout of the pair filter, np = W * H doubles per plane: neighbouring pixels are neighbouring words.
//   guide [8][np]: N.x, N.y, N.z, A.r, A.g, A.b, z and the bad mask as a double (0 good, 1 bad in half A, 2 bad in half B, 3 in both)
//   col   [6][np]: half A's r, g, b, then half B's;   var [2][np]: half A's, half B's
#define PTA_GUIDE_PLANES 8
#define PTA_GUIDE_Z 6
#define PTA_GUIDE_BAD 7

// Prep of one pixel of both halves: the four raw sums, cnt = the pixel's own count (>= 2; nA = (cnt + 1) / 2, nB = cnt / 2), the feature
// sums or null -> plane element i of guide, col and var.
PT_HD void prep_pair_pixel(const double SA[3], const double QA[3], const double SB[3], const double QB[3], uint32_t cnt, const double *fn,
                           const double *fa, const double *fd, size_t np, size_t i, double *guide, double *col, double *var) {
    double c[3], v;
    Guide g, gb;
    prep_pixel(SA, QA, (cnt + 1u) / 2u, fn, fa, fd, c, v, g);
    for (int k = 0; k < 3; k++) col[(size_t)k * np + i] = c[k];
    var[i] = v;
    prep_pixel(SB, QB, cnt / 2u, fn, fa, fd, c, v, gb);  // (the same N, A and z: they do not depend on the radiance sums)
    for (int k = 0; k < 3; k++) col[(size_t)(3 + k) * np + i] = c[k];
    var[np + i] = v;
    for (int k = 0; k < 3; k++) { guide[(size_t)k * np + i] = g.n[k]; guide[(size_t)(3 + k) * np + i] = g.a[k]; }
    guide[(size_t)PTA_GUIDE_Z * np + i] = g.z;
    guide[(size_t)PTA_GUIDE_BAD * np + i] = g.bad + 2.0 * gb.bad;
}

// One iteration of both halves at pixel (x, y): filter_pixel on half A and on half B, bit for bit, with the guide record of a tap
// loaded once and the three feature terms computed once.  co = half A's c' then half B's, vo = the two var'.
PT_HD void filter_pair_pixel(const Params &P, int32_t W, int32_t H, int32_t x, int32_t y, int32_t step, const double *__restrict__ col,
                             const double *__restrict__ var, const double *__restrict__ guide, double co[6], double vo[2]) {
    const size_t np = (size_t)W * (size_t)H;
    const size_t i = (size_t)y * (size_t)W + (size_t)x;
    const int badi = (int)guide[(size_t)PTA_GUIDE_BAD * np + i];
    double ci[6], vi[2];
    for (int k = 0; k < 6; k++) co[k] = ci[k] = col[(size_t)k * np + i];
    vo[0] = vi[0] = var[i];
    vo[1] = vi[1] = var[np + i];
    if (badi == 3) return;
    const double gin0 = guide[i], gin1 = guide[np + i], gin2 = guide[2 * np + i];
    const double gia0 = guide[3 * np + i], gia1 = guide[4 * np + i], gia2 = guide[5 * np + i];
    const double giz = guide[(size_t)PTA_GUIDE_Z * np + i];
    const double li[2] = {(ci[0] + ci[1] + ci[2]) / 3.0, (ci[3] + ci[4] + ci[5]) / 3.0};
    const double den_l[2] = {P.sigma_l * ptm::f_sqrt(vi[0]) + 1e-8, P.sigma_l * ptm::f_sqrt(vi[1]) + 1e-8};
    const double den_z = P.sigma_z * (giz > 1e-8 ? giz : 1e-8);
    const double den_a = P.sigma_a * P.sigma_a;
    const double B[5] = {0.0625, 0.25, 0.375, 0.25, 0.0625};
    double sw[2] = {0.0, 0.0}, sv[2] = {0.0, 0.0}, sd[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int dy = -2; dy <= 2; dy++) {
        const int32_t yj = y + dy * step;
        if (yj < 0 || yj >= H) continue;
        for (int dx = -2; dx <= 2; dx++) {
            const int32_t xj = x + dx * step;
            if (xj < 0 || xj >= W) continue;
            const size_t j = (size_t)yj * (size_t)W + (size_t)xj;
            const int skip = (int)guide[(size_t)PTA_GUIDE_BAD * np + j] | badi;  // bit h: the tap does not count in half h
            if (skip == 3) continue;
            double tn = 0.0, tz = 0.0, ta = 0.0;  // the feature terms, the same in both halves
            if (P.n_on) {
                const double q = 1.0 - (gin0 * guide[j] + gin1 * guide[np + j] + gin2 * guide[2 * np + j]);
                tn = (q > 0.0 ? q : 0.0) / P.sigma_n;
            }
            if (P.z_on) tz = ptm::f_abs(giz - guide[(size_t)PTA_GUIDE_Z * np + j]) / den_z;
            if (P.a_on) {
                const double dr = gia0 - guide[3 * np + j], dg = gia1 - guide[4 * np + j], db = gia2 - guide[5 * np + j];
                ta = (dr * dr + dg * dg + db * db) / den_a;
            }
            const double b = B[dy + 2] * B[dx + 2];
            for (int h = 0; h < 2; h++) {
                if (skip & (1 << h)) continue;
                const double cj0 = col[(size_t)(3 * h) * np + j], cj1 = col[(size_t)(3 * h + 1) * np + j], cj2 = col[(size_t)(3 * h + 2) * np + j];
                const double lj = (cj0 + cj1 + cj2) / 3.0;
                double pen = ptm::f_abs(li[h] - lj) / den_l[h];
                if (P.n_on) pen = pen + tn;  // ((lum + n) + z) + a, the order of filter_pixel
                if (P.z_on) pen = pen + tz;
                if (P.a_on) pen = pen + ta;
                if (pen > PTA_PEN_CUT) continue;
                const double w = b * ptm::go_exp(-pen);
                sw[h] = sw[h] + w;
                sd[3 * h] = sd[3 * h] + w * (cj0 - ci[3 * h]);
                sd[3 * h + 1] = sd[3 * h + 1] + w * (cj1 - ci[3 * h + 1]);
                sd[3 * h + 2] = sd[3 * h + 2] + w * (cj2 - ci[3 * h + 2]);
                sv[h] = sv[h] + (w * w) * var[(size_t)h * np + j];
            }
        }
    }
    for (int h = 0; h < 2; h++) {
        if (badi & (1 << h)) continue;
        for (int k = 0; k < 3; k++) co[3 * h + k] = ci[3 * h + k] + sd[3 * h + k] / sw[h];
        vo[h] = sv[h] / (sw[h] * sw[h]);
    }
}

// The two noise terms of a pixel of the combined frame: mean and err of Combine, va, vb the halves' propagated variances, bad = the
// pixel's bad mask.  Returns whether the pixel counts as bad; a term that adds nothing is returned as 0.
PT_HD bool err_terms(const double mean[3], double err, double va, double vb, int bad, double &e2, double &e2_model) {
    const double l = (mean[0] + mean[1] + mean[2]) / 3.0;
    const double den = l < 0.01 ? 0.01 : l;
    e2 = err / (den * den);
    e2_model = ((va + vb) * 0.25) / (den * den);
    const bool isbad = bad != 0 || !finite(e2);
    if (isbad) e2 = 0.0;
    if (isbad || !finite(e2_model)) e2_model = 0.0;
    return isbad;
}

// The combine of one pixel: fA, fB the filtered halves, va, vb their propagated variances, bad = the pixel's bad mask -> mean, err and
// the two noise terms (measured, model).  Returns whether the pixel counts as bad; a term that adds nothing is returned as 0.
PT_HD bool combine_pixel(const double fA[3], const double fB[3], double va, double vb, int bad, double mean[3], double &err, double &e2,
                         double &e2_model) {
    double d[3];
    for (int k = 0; k < 3; k++) {
        mean[k] = (fA[k] + fB[k]) * 0.5;
        d[k] = (fA[k] - fB[k]) * 0.5;
    }
    err = (d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) / 3.0;
    return err_terms(mean, err, va, vb, bad, e2, e2_model);
}

// ---------------------------------------------------------------- block figures (BLOCKS above)

#define PTA_MAX_POOL 4

// Step 2's term of one pixel, from the planes the combine leaves: the e2 err_terms adds into `noise`.
PT_HD double block_term(const double mean[3], double err, int bad) {
    double e2, e2_model;
    err_terms(mean, err, 0.0, 0.0, bad, e2, e2_model);
    return e2;
}

// Step 3 at block (bx, by) of the nbx x nby grid: s, k row-major over the grid -> P_B; own = sqrt(s_B / k_B).
PT_HD double pool_block(const double *__restrict__ s, const uint32_t *__restrict__ k, int32_t nbx, int32_t nby, int32_t bx, int32_t by,
                        int32_t r, double &own) {
    double ss = 0.0;
    uint32_t kk = 0;
    for (int32_t y = by - r; y <= by + r; y++) {
        if (y < 0 || y >= nby) continue;
        for (int32_t x = bx - r; x <= bx + r; x++) {
            if (x < 0 || x >= nbx) continue;
            const size_t b = (size_t)y * (size_t)nbx + (size_t)x;
            ss = ss + s[b];
            kk += k[b];
        }
    }
    const size_t b = (size_t)by * (size_t)nbx + (size_t)bx;
    own = ptm::f_sqrt(s[b] / (double)k[b]);
    return ptm::f_sqrt(ss / (double)kk);
}

}  // namespace pta
