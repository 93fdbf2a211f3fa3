// temporal_motion_probe.hip -- test-only: temporal_kernel with displaced reprojection (the object index plane and the motion table
// of step 4a of csrc/pt_temporal.h; the history clip of step 7a beside it) and the a-trous kernels behind it on the gfx950 device,
// on frames the caller makes up.
//
// pt_kernels.h and pt_filter_launch.h are included unchanged and compiled with the library's own flags
// (tests/temporal_motion_support.py), so what runs here is the code libptcore.so ships.  motion_probe_frame uploads its host arrays,
// launches temporal_kernel as pt_temporal does (ptcore.hip) and then pt_temporal's own launch sequence (pt_filter_launch.h), copies
// the results back and returns the first HIP status that was not hipSuccess (0 = fine; a negative value: the arguments were refused
// before anything was launched).  Every output buffer has its full size and is filled with 0xFF bytes before the launch, so what a
// kernel did not write reads as a NaN.  The figures and the counts come from the kernels' partials through the product's own sums.
// No inline assembly.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "probe_common.h"
#include "pt_filter_launch.h"
#include "pt_kernels.h"

namespace {

const int64_t MAX_PIXELS = (int64_t)1 << 24;

// The history: what pt_ctx keeps (tp_hist, tp_cur, tp_valid, tp_w, tp_h, tp_cam).
struct History {
    double *set[2] = {nullptr, nullptr};
    size_t cap[2] = {0, 0};  // doubles
    int cur = 0;
    int32_t W = 0, H = 0;
    bool valid = false;
    ptd::DevCamera cam{};
};

ptd::DevCamera camera(const double *c) {  // ora_camera_setup's 22 doubles
    ptd::DevCamera d{};
    for (int k = 0; k < 3; k++) {
        d.origin[k] = c[k]; d.lower_left[k] = c[3 + k]; d.horizontal[k] = c[6 + k]; d.vertical[k] = c[9 + k];
        d.u[k] = c[12 + k]; d.v[k] = c[15 + k];
    }
    d.lens_radius = c[21];
    return d;
}

}  // namespace

extern "C" {

void *motion_probe_new() { return new History(); }

void motion_probe_free(void *hp) {
    History *h = static_cast<History *>(hp);
    if (!h) return;
    for (int k = 0; k < 2; k++)
        if (h->set[k]) (void)hipFree(h->set[k]);
    delete h;
}

void motion_probe_reset(void *hp) {
    if (hp) static_cast<History *>(hp)->valid = false;
}

// pt_temporal_read: *valid = 0 and nothing written when the history is empty; else mean [H][W][3], var [H][W], len [H][W] of it.
int motion_probe_read(void *hp, double *mean, double *var, int32_t *len, int32_t *valid) {
    if (!hp || !mean || !var || !len || !valid) return -2;
    History &h = *static_cast<History *>(hp);
    *valid = h.valid ? 1 : 0;
    if (!h.valid) return 0;
    const size_t np = (size_t)h.W * (size_t)h.H;
    std::vector<double> planes((size_t)PTT_PLANES * np);
    hipError_t st = hipSuccess;
    PROBE_TRY(hipMemcpy(planes.data(), h.set[h.cur], planes.size() * sizeof(double), hipMemcpyDeviceToHost));
    if (st != hipSuccess) return (int)st;
    for (size_t i = 0; i < np; i++) {
        for (size_t k = 0; k < 3; k++) mean[3 * i + k] = planes[k * np + i];
        var[i] = planes[(size_t)PTT_VAR * np + i];
        std::memcpy(&len[i], reinterpret_cast<const char *>(&planes[(size_t)PTT_LH * np]) + 8 * i, sizeof(int32_t));
    }
    return 0;
}

// pt_temporal's chain on one frame: S, Q, the feature sums [H][W][3]; cnt [H][W] or null (n everywhere); cam22 = this frame's
// camera; tcfg = {alpha, tol_z, n_min, tol_a, max_len, gamma}; T < 0: no filter, else T iterations with sig.  mean [H][W][3],
// var [H][W], rgba [H][W][4]; noise[3] = before, blended, after; counts[7] = reprojected, disoccluded, bad, the sum of len', clipped,
// moved, moved_reprojected.  `place` is not written.  ids [H][W] = the object index plane, delta [ndelta][3] = the motion table:
// delta null or ndelta 0 is a call without a table (ids is then not uploaded and the kernel gets three nulls), refused as
// pt_temporal_set_motion and pt_temporal refuse: ndelta < 0 or an entry that is not finite (-8), a table without ids (-9).  The
// ids themselves are not checked: an index outside the table is the kernel's to ignore.
int motion_probe_frame(void *hp, int32_t W, int32_t H, const double *S, const double *Q, const uint32_t *cnt, uint32_t n, const double *fn,
                     const double *fa, const double *fd, const double *cam22, const double *tcfg, int32_t T, const double *sig, double *mean,
                     double *var, uint8_t *rgba, double *noise, uint64_t *counts, double *place, const int32_t *ids, const double *delta, int32_t ndelta) {
    (void)place;
    if (!hp || W < 2 || H < 2 || (int64_t)W * (int64_t)H > MAX_PIXELS || T > PTA_MAX_ITERATIONS) return -1;
    if (!S || !Q || !fn || !fa || !fd || !cam22 || !tcfg || !sig || !mean || !var || !rgba || !noise || !counts) return -2;
    if (T >= 0 && (!(sig[0] > 0.0) || !(sig[1] >= 0.0) || !(sig[2] >= 0.0) || !(sig[3] >= 0.0))) return -4;
    if (!(tcfg[0] >= 0.0 && tcfg[0] <= 1.0) || !(tcfg[1] >= 0.0) || !(tcfg[3] >= 0.0) || tcfg[2] != tcfg[2] || !(tcfg[4] >= 1.0 && tcfg[4] <= 2147483647.0))
        return -6;
    if (!(tcfg[5] >= 0.0) || std::isinf(tcfg[5])) return -7;  // pt_temporal_set_clip's refusal
    if (ndelta < 0) return -8;  // pt_temporal_set_motion's refusals
    const bool table = delta && ndelta > 0;
    if (table)
        for (size_t i = 0; i < 3 * (size_t)ndelta; i++)
            if (!std::isfinite(delta[i])) return -8;
    if (table && !ids) return -9;  // pt_temporal's: a table pending and a frame without object ids
    History &h = *static_cast<History *>(hp);
    const size_t np = (size_t)W * (size_t)H;
    for (size_t i = 0; i < np; i++)
        if ((cnt ? cnt[i] : n) < 2) return -5;
    const uint32_t grid1 = ptl::grid_1d(np);
    const dim3 grid2 = ptl::grid_2d(W, H);
    const size_t nblk = (size_t)grid2.x * grid2.y;
    const bool have = h.valid && h.W == W && h.H == H;  // another size: the history is dropped (when the call succeeds)
    hipError_t st = hipSuccess;
    for (int k = 0; k < 2; k++) {  // both sets are kept at the size of this frame; a set that has to grow loses its contents
        if (h.cap[k] >= (size_t)PTT_PLANES * np) continue;
        h.valid = false;
        if (h.set[k]) (void)hipFree(h.set[k]);
        h.set[k] = nullptr;
        h.cap[k] = 0;
        PROBE_TRY(hipMalloc(reinterpret_cast<void **>(&h.set[k]), (size_t)PTT_PLANES * np * sizeof(double)));
        if (st != hipSuccess) { h.set[k] = nullptr; return (int)st; }
        h.cap[k] = (size_t)PTT_PLANES * np;
        PROBE_TRY(hipMemset(h.set[k], 0xFF, h.cap[k] * sizeof(double)));
    }
    const int next = h.cur ^ 1;
    PROBE_TRY(hipMemset(h.set[next], 0xFF, (size_t)PTT_PLANES * np * sizeof(double)));
    Buf<double> dS(S, 3 * np), dQ(Q, 3 * np), dfn(fn, 3 * np), dfa(fa, 3 * np), dfd(fd, 3 * np);
    Buf<uint32_t> dcnt(cnt, cnt ? np : 0);
    Buf<int32_t> dids(table ? ids : nullptr, table ? np : 0);
    Buf<double> ddelta(table ? delta : nullptr, table ? 3 * (size_t)ndelta : 0);
    Buf<ptk::TemporalPartial> tpart(nullptr, nblk);
    Buf<double> col0(nullptr, 3 * np), col1(nullptr, 3 * np), var0(nullptr, np), var1(nullptr, np);
    Buf<pta::Guide> guide(nullptr, np);
    Buf<ptk::NoisePartial> part(nullptr, 2 * (size_t)grid1);
    Buf<uint8_t> drgba(nullptr, 4 * np);
    for (hipError_t e : {dS.st, dQ.st, dfn.st, dfa.st, dfd.st, dcnt.st, dids.st, ddelta.st, tpart.st, col0.st, col1.st, var0.st, var1.st, guide.st, part.st, drgba.st})
        PROBE_TRY(e);
    if (st != hipSuccess) return (int)st;
    double *const col[2] = {col0.d, col1.d}, *const vr[2] = {var0.d, var1.d};
    ptk::TemporalArgs TA;
    std::memset(&TA, 0, sizeof TA);
    TA.C.alpha = tcfg[0]; TA.C.tol_z = tcfg[1]; TA.C.n_min = tcfg[2]; TA.C.tol_a = tcfg[3];
    TA.C.max_len = (int32_t)tcfg[4];
    TA.C.have_history = have ? 1 : 0;
    TA.C.clip_gamma = tcfg[5];
    TA.V.cam = camera(cam22);
    TA.V.inv_width = 1.0 / (double)(W - 1);
    TA.V.inv_height = 1.0 / (double)(H - 1);
    TA.V.W = W;
    TA.V.H = H;
    TA.cam_h = h.cam;
    TA.acc = dS.d;
    TA.m2 = dQ.d;
    TA.cnt = cnt ? dcnt.d : nullptr;
    TA.fn = dfn.d;
    TA.fa = dfa.d;
    TA.fd = dfd.d;
    TA.hist = h.set[h.cur];
    TA.hist_out = h.set[next];
    TA.col = col[0];
    TA.var = vr[0];
    TA.guide = guide.d;
    TA.partial = tpart.d;
    TA.n = n;
    if (table) {
        TA.ids = dids.d;
        TA.delta = ddelta.d;
        TA.ndelta = ndelta;
    }
    hipLaunchKernelGGL(ptk::temporal_kernel, grid2, dim3(PT_BLOCK), 0, 0, TA);
    const pta::Params P = ptl::filter_params({T, 0, sig[0], sig[1], sig[2], sig[3]}, true);
    const int cur = ptl::filter_sequence(T >= 0 ? &P : nullptr, col, vr, guide.d, part.d, drgba.d, W, H, 0);
    int rc = finish(st);
    if (rc) return rc;  // the stored history is untouched: the kernel wrote the other set
    std::vector<ptk::NoisePartial> hp_part(2 * (size_t)grid1);
    std::vector<ptk::TemporalPartial> tp(nblk);
    rc = (int)part.download(hp_part.data());
    if (!rc) rc = (int)(cur ? col1 : col0).download(mean);
    if (!rc) rc = (int)(cur ? var1 : var0).download(var);
    if (!rc) rc = (int)drgba.download(rgba);
    if (!rc) rc = (int)tpart.download(tp.data());
    if (rc) return rc;
    h.cur = next;
    h.valid = true;
    h.W = W;
    h.H = H;
    h.cam = TA.V.cam;
    const ptl::TemporalFigures tf = ptl::temporal_figures(tp.data(), nblk, np);
    const ptl::NoiseFigures nf = ptl::noise_figures(hp_part.data(), grid1, T >= 0, np);
    counts[0] = tf.reprojected;
    counts[1] = tf.disoccluded;
    counts[2] = nf.bad;
    counts[3] = tf.len_sum;
    counts[4] = tf.clipped;
    counts[5] = tf.moved;
    counts[6] = tf.moved_reprojected;
    noise[0] = tf.noise_before;
    noise[1] = nf.before;
    noise[2] = nf.after;
    return 0;
}

}  // extern "C"
