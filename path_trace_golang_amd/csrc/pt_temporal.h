// pt_temporal.h -- temporal accumulation (pt_temporal): the last frame's blended history reprojected into this frame, host + device.
//
// Opt-in per context; until pt_temporal is called nothing here is allocated or launched.  Everything is PT_HD and built from IEEE
// +,-,*,/, sqrt (compile with -ffp-contract=off), so the gfx950 kernel (temporal_kernel in pt_kernels.h) and a host build of this
// header give the same bits.  This comment is the specification tests/temporal_reference.c restates.  Every sum below is written in
// its order of evaluation: a + b + c means (a + b) + c, and a . b = a.x*b.x + a.y*b.y + a.z*b.z.
//
// CURRENT FRAME.  The inputs of FILTER (pt_atrous.h): per pixel the raw sums S and Q, its own count n >= 2 and the three feature sums
// (required here), and the frame's camera (origin, lower_left, horizontal, vertical), W, H, inv_width = 1 / (W - 1),
// inv_height = 1 / (H - 1).  Prep is FILTER's prep unchanged: c, var, bad, N, A, z and h = depth[1], the samples that hit;
// hit = h > 0.
//
// HISTORY.  Per pixel c_h[3], var_h, len_h (an integer; 0 = not usable as a tap), N_h[3], A_h[3], z_h, hit_h, and one camera cam_h
// (its fields carry the suffix _h below).  Empty after pt_create, after pt_temporal_reset and on a call whose W x H differs from
// the history's.
//
// PER PIXEL i = (x, y):
//   1. A bad pixel:  out = (c_i, var_i), len' = 0.
//   2. Empty history:  out = (c_i, var_i), len' = 1.
//   3. The centre ray, the camera sample of ray generation with both draws replaced by 0.5:
//          u = (x + 0.5) * inv_width;  v = ((H-1 - y) + 0.5) * inv_height;
//          a = (lower_left + horizontal * u) + vertical * v;  d = a - origin            (per component)
//      With a thin lens (lens_radius > 0) this is the ray through the centre of the lens: an approximation of the pixel's bundle of
//      rays, exact in the plane of focus.
//   4. The vector to project:  hit:  P = origin + d * (z / sqrt(d . d));  q = P - origin_h;  zexp = sqrt(q . q)
//                              miss: q = d                                (the sky is reprojected by direction; zexp unused)
//  4a. Displacement (a motion table only: pt_temporal_set_motion; without one this step does not exist and every bit is as it is
//      without it).  The frame carries, per pixel, the object index o of its sample 0's first hit (-1: a miss) and the table
//      delta[n][3]: per object its position in this frame minus its position in the frame the history was stored from.  On a hit
//      with 0 <= o < n and delta[o] != (0, 0, 0), step 4's P becomes, per component k,
//          P_k = (origin_k + d_k * s) - delta[o][k]          (s = z / sqrt(d . d); then q = P - origin_h and zexp as in step 4)
//      -- where the point now seen lay when the history was stored.  A miss, o < 0, o >= n and a zero delta change nothing (P - 0 = P:
//      an all-zero table gives the bits of no table).  Taps, validity tests, clip, blend and the stored history are unchanged.
//      Limits:
//        - o is sample 0's while N, A and z are means over the k feature samples: a pixel on a silhouette is ambiguous, and is left to
//          the tap tests.
//        - The radiance on and near a moved object changes (its reflections, its shadow).  That is the clip's work: gamma = 2.5
//          whenever motion is on.
//        - The strip a moved object uncovers is disoccluded and starts again at len 1.
//        - A resize, a material edit and a sky edit are not motion: the caller resets the history.
//      Counted: a good hit pixel with such an o is `moved`, and `moved_reprojected` when it reaches step 8 with history.
//   5. The inverse of the previous camera:
//          e = lower_left_h - origin_h;  nrm = horizontal_h x vertical_h   (nrm.x = hor.y*ver.z - hor.z*ver.y, and cyclically)
//          den = q . nrm;  num = e . nrm;  unless den * num > 0 there is no history (behind the camera, parallel, NaN)
//          s = num / den;  pt = q * s - e;
//          pu = (pt . horizontal_h) / (horizontal_h . horizontal_h);  pv = (pt . vertical_h) / (vertical_h . vertical_h)
//          fx = pu * (W-1) - 0.5;  fy = ((H-1) - pv * (H-1)) + 0.5
//      fx or fy NaN, infinite or outside [-1, W] x [-1, H]: no history.  (An unmoved camera gives fx = x, fy = y up to rounding.)
//   6. Taps:  x0 = floor(fx), y0 = floor(fy), ax = fx - x0, ay = fy - y0.  The four taps j = (x0 + dx, y0 + dy), dy outer and dx inner,
//      both 0 then 1, with w = wx * wy, wx = dx ? ax : 1 - ax, wy = dy ? ay : 1 - ay.  A tap is VALID when it lies in the frame,
//      len_h > 0, hit_h == hit_i, w > 0 and, on a hit,
//          |z_h - zexp| <= tol_z * zexp,   N_i . N_h >= n_min,   dr*dr + dg*dg + db*db <= tol_a * tol_a   ((dr, dg, db) = A_i - A_h).
//   7. Over the valid taps, in tap order from 0:  sw = sw + w;  sc_k = sc_k + w * c_h,k;  sv = sv + (w * w) * var_h;
//      L = the smallest len_h.  Unless sw > 0.01 there is no history.   c_r,k = sc_k / sw;  var_r = sv / (sw * sw).
//  7a. Clip (gamma > 0 only; gamma = 0, the default, skips this step and leaves every bit as it is without it):
//          s = var_i + var_r;   half = gamma * sqrt(s > 0 ? s : 0)
//          per channel k:  lo = c_i,k - half;  hi = c_i,k + half;
//                          c_r,k = c_r,k < lo ? lo : (c_r,k > hi ? hi : c_r,k)
//      var_r and L stay as they are.  A reprojected pixel is `clipped` when any channel changed (a c_r,k that lies exactly on a
//      bound did not).  Both comparisons are false on a NaN, so a NaN half changes nothing.  The variances are the
//      model's channel-mean variances, applied to every channel.  The clip rectifies the HISTORY: the reprojection is keyed by
//      first-hit geometry alone, and where what is seen at a pixel changed although normal, distance and albedo still agree (a
//      reflection, a refraction, a shadow that moved) the history holds another view's radiance -- ghosting.  The frame says, with
//      its own variance, how far the truth can lie from c_i; the history is pulled to within that.  Consequences:
//        - Where frame and history both have zero variance (emitters, sky) half = 0 and the history becomes the frame exactly.
//        - A firefly in the FRAME has a large var_i, so the clip is loose there: it rejects no frame outliers.
//        - A dark pixel whose samples are all zero (c_i = 0, var_i = 0) pulls its history to within gamma * sqrt(var_r) of zero.
//          That is a bias, and it is inside the measured tables.
//   8. Blend:  r = 1 / (L + 1);  a = alpha > r ? alpha : r;   c'_k = c_r,k + a * (c_i,k - c_r,k);
//          var' = ((1 - a) * (1 - a)) * var_r + (a * a) * var_i;   len' = min(L + 1, max_len).
//      No history:  out = (c_i, var_i), len' = 1.
//      var' is the variance of the blended mean when the frames are independent: the caller changes the seed from frame to frame.
//      Frames rendered with one seed repeat their noise, and var' then understates what is left.
//   9. The new history = (c', var', len', N_i, A_i, z_i, hit_i) and this frame's camera: what step 8 leaves, before any filtering.
//
// FILTER STAGE.  FILTER's iterations (pt_atrous.h) on (c', var') with this frame's guide (N, A, z, bad), then its finish; the noise
// figure of a state is FILTER's.
//
// Counted: a pixel of step 1 is `bad`; a good pixel that reaches step 8 with history is `reprojected`; a good pixel that does not,
// while the history is not empty, is `disoccluded`; a reprojected pixel that step 7a changed is also `clipped`.
#pragma once

#include <stdint.h>

#include "pt_atrous.h"

namespace ptt {

// The history planes, np = W * H elements each: neighbouring pixels are neighbouring words of every plane.
//   d [11][np]: c.r, c.g, c.b, var, N.x, N.y, N.z, A.r, A.g, A.b, z      lh [np][2]: len, hit
#define PTT_PLANES 12  // doubles per pixel, lh included
#define PTT_VAR 3
#define PTT_N 4
#define PTT_A 7
#define PTT_Z 10
#define PTT_LH 11      // lh lies behind the eleven double planes

struct Config {
    double alpha, tol_z, n_min, tol_a;
    int32_t max_len;
    int32_t have_history;  // 0: the history is empty
    double clip_gamma = 0.0;  // step 7a; 0 = off (also what a zero-filled or default-constructed Config has)
};

// The frame's camera and size.
struct View {
    ptd::DevCamera cam;
    double inv_width, inv_height;
    int32_t W, H;
};

enum Status { ST_BAD = 0, ST_NEW = 1, ST_DISOCCLUDED = 2, ST_REPROJECTED = 3 };

PT_HD double dot3(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// Steps 3 - 5: where pixel (x, y) of the view V, whose first hit lies z away along the centre ray (hit) or which sees the sky, was in
// the frame of cam_h.  False: no history.  disp (step 4a) = the displacement of the pixel's object since the history was stored, or
// null: the object did not move, or nothing is known about it.
PT_HD bool reproject(const View &V, const ptd::DevCamera &ch, int32_t x, int32_t y, bool hit, double z, double &fx, double &fy, double &zexp,
                     const double *disp = nullptr) {
    const ptd::DevCamera &cm = V.cam;
    const double hm1 = (double)(V.H - 1), wm1 = (double)(V.W - 1);
    const double u = ((double)x + 0.5) * V.inv_width;
    const double v = ((hm1 - (double)y) + 0.5) * V.inv_height;
    double d[3], q[3], e[3];
    for (int k = 0; k < 3; k++) {
        const double a = (cm.lower_left[k] + cm.horizontal[k] * u) + cm.vertical[k] * v;
        d[k] = a - cm.origin[k];
    }
    zexp = 0.0;
    if (hit) {
        const double s = z / ptm::f_sqrt(dot3(d, d));
        for (int k = 0; k < 3; k++) {
            double P = cm.origin[k] + d[k] * s;
            if (disp) P = P - disp[k];
            q[k] = P - ch.origin[k];
        }
        zexp = ptm::f_sqrt(dot3(q, q));
    } else {
        for (int k = 0; k < 3; k++) q[k] = d[k];
    }
    for (int k = 0; k < 3; k++) e[k] = ch.lower_left[k] - ch.origin[k];
    const double *hh = ch.horizontal, *vv = ch.vertical;
    const double nrm[3] = {hh[1] * vv[2] - hh[2] * vv[1], hh[2] * vv[0] - hh[0] * vv[2], hh[0] * vv[1] - hh[1] * vv[0]};
    const double den = dot3(q, nrm), num = dot3(e, nrm);
    if (!(den * num > 0.0)) return false;
    const double s = num / den;
    double pt[3];
    for (int k = 0; k < 3; k++) pt[k] = q[k] * s - e[k];
    const double pu = dot3(pt, hh) / dot3(hh, hh);
    const double pv = dot3(pt, vv) / dot3(vv, vv);
    fx = pu * wm1 - 0.5;
    fy = (hm1 - pv * hm1) + 0.5;
    if (!pta::finite(fx) || !pta::finite(fy)) return false;
    return fx >= -1.0 && fx <= (double)V.W && fy >= -1.0 && fy <= (double)V.H;
}

// Step 4a's lookup for pixel i: the row of delta [n][3] that displaces it, or null (no table, a miss, an index outside the table,
// a zero row).  ids = the frame's object index plane, row-major.
PT_HD const double *displacement(const int32_t *__restrict__ ids, const double *__restrict__ delta, int32_t n, size_t i, bool hit) {
    if (!delta || !ids || !hit) return nullptr;
    const int32_t o = ids[i];
    if (o < 0 || o >= n) return nullptr;
    const double *r = delta + 3 * (size_t)o;
    return (r[0] != 0.0 || r[1] != 0.0 || r[2] != 0.0) ? r : nullptr;
}

// floor of a value in [-1, 2^31)
PT_HD int32_t floor_i(double f) {
    int32_t i = (int32_t)f;
    if ((double)i > f) i--;
    return i;
}

// Steps 1 - 8 of pixel (x, y): c, var, g = the prep of the pixel, hit = h > 0; hd, hl = the history planes (read when
// C.have_history) and ch its camera -> c', var', len'; *clipped (when asked for) = whether step 7a changed the history; disp =
// reproject's.
PT_HD Status blend_pixel(const Config &C, const View &V, const ptd::DevCamera &ch, const double *__restrict__ hd, const int32_t *__restrict__ hl,
                         int32_t x, int32_t y, const double c[3], double var, const pta::Guide &g, bool hit, double co[3], double &vo,
                         int32_t &len, bool *clipped = nullptr, const double *disp = nullptr) {
    co[0] = c[0]; co[1] = c[1]; co[2] = c[2];
    vo = var;
    if (clipped) *clipped = false;
    if (g.bad != 0.0) {
        len = 0;
        return ST_BAD;
    }
    len = 1;
    if (!C.have_history) return ST_NEW;
    double fx, fy, zexp;
    if (!reproject(V, ch, x, y, hit, g.z, fx, fy, zexp, disp)) return ST_DISOCCLUDED;
    const size_t np = (size_t)V.W * (size_t)V.H;
    const int32_t x0 = floor_i(fx), y0 = floor_i(fy);
    const double ax = fx - (double)x0, ay = fy - (double)y0;
    const double tz = C.tol_z * zexp, ta = C.tol_a * C.tol_a;
    double sw = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0, sv = 0.0;
    int32_t L = 0x7fffffff;
    for (int dy = 0; dy < 2; dy++) {
        const int32_t yj = y0 + dy;
        if (yj < 0 || yj >= V.H) continue;
        const double wy = dy ? ay : 1.0 - ay;
        for (int dx = 0; dx < 2; dx++) {
            const int32_t xj = x0 + dx;
            if (xj < 0 || xj >= V.W) continue;
            const size_t j = (size_t)yj * (size_t)V.W + (size_t)xj;
            const int32_t lj = hl[2 * j];
            if (lj <= 0 || (hl[2 * j + 1] != 0) != hit) continue;
            const double w = (dx ? ax : 1.0 - ax) * wy;
            if (!(w > 0.0)) continue;
            if (hit) {
                if (!(ptm::f_abs(hd[(size_t)PTT_Z * np + j] - zexp) <= tz)) continue;
                const double nh[3] = {hd[(size_t)PTT_N * np + j], hd[(size_t)(PTT_N + 1) * np + j], hd[(size_t)(PTT_N + 2) * np + j]};
                if (!(dot3(g.n, nh) >= C.n_min)) continue;
                const double dr = g.a[0] - hd[(size_t)PTT_A * np + j], dg = g.a[1] - hd[(size_t)(PTT_A + 1) * np + j],
                             db = g.a[2] - hd[(size_t)(PTT_A + 2) * np + j];
                if (!(dr * dr + dg * dg + db * db <= ta)) continue;
            }
            sw = sw + w;
            s0 = s0 + w * hd[j];
            s1 = s1 + w * hd[np + j];
            s2 = s2 + w * hd[2 * np + j];
            sv = sv + (w * w) * hd[(size_t)PTT_VAR * np + j];
            if (lj < L) L = lj;
        }
    }
    if (!(sw > 0.01)) return ST_DISOCCLUDED;
    double cr[3] = {s0 / sw, s1 / sw, s2 / sw};
    const double vr = sv / (sw * sw);
    if (C.clip_gamma > 0.0) {
        const double s = var + vr;
        const double half = C.clip_gamma * ptm::f_sqrt(s > 0.0 ? s : 0.0);
        bool any = false;
        for (int k = 0; k < 3; k++) {
            const double lo = c[k] - half, hi = c[k] + half;
            const bool below = cr[k] < lo, above = cr[k] > hi;
            cr[k] = below ? lo : (above ? hi : cr[k]);
            any = any || below || above;
        }
        if (clipped) *clipped = any;
    }
    const double r = 1.0 / (double)(L + 1);
    const double a = C.alpha > r ? C.alpha : r;
    const double om = 1.0 - a;
    for (int k = 0; k < 3; k++) co[k] = cr[k] + a * (c[k] - cr[k]);
    vo = (om * om) * vr + (a * a) * var;
    len = L + 1 < C.max_len ? L + 1 : C.max_len;
    return ST_REPROJECTED;
}

// Step 9: the history element of pixel i.
PT_HD void store_history(double *__restrict__ hd, int32_t *__restrict__ hl, size_t np, size_t i, const double c[3], double var, int32_t len,
                         const pta::Guide &g, bool hit) {
    for (int k = 0; k < 3; k++) {
        hd[(size_t)k * np + i] = c[k];
        hd[(size_t)(PTT_N + k) * np + i] = g.n[k];
        hd[(size_t)(PTT_A + k) * np + i] = g.a[k];
    }
    hd[(size_t)PTT_VAR * np + i] = var;
    hd[(size_t)PTT_Z * np + i] = g.z;
    hl[2 * i] = len;
    hl[2 * i + 1] = hit ? 1 : 0;
}

}  // namespace ptt
