// denoise_probe.hip -- test-only: the kernels of the a-trous filter, of the pair filter and of the temporal accumulation
// (csrc/pt_kernels.h) on the gfx950 device, on frames the caller makes up: any size, any sums, any camera.
//
// pt_kernels.h and pt_filter_launch.h are included unchanged and compiled with the library's own flags
// (tests/denoise_probe_support.py), so what runs here is the code libptcore.so ships.  Each extern "C" entry point uploads its host
// arrays, launches the first kernel of the host function it names (ptcore.hip) and then that function's own launch sequence
// (pt_filter_launch.h), copies the results back and returns the first HIP status that was not hipSuccess (0 = fine; a negative
// value: the arguments were refused before anything was launched).  Every output buffer has its full size and is filled with 0xFF
// bytes before the launch, so what a kernel did not write reads as a NaN.  The figures and the counts come from the kernels'
// partials through the product's own sums.  No inline assembly.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "probe_common.h"
#include "pt_filter_launch.h"
#include "pt_kernels.h"

namespace {

const int64_t MAX_PIXELS = (int64_t)1 << 24;

bool size_ok(int32_t W, int32_t H, int32_t least) { return W >= least && H >= least && (int64_t)W * (int64_t)H <= MAX_PIXELS; }

// every pixel holds at least `least` samples
bool counts_ok(const uint32_t *cnt, uint32_t n, size_t np, uint32_t least) {
    if (!cnt) return n >= least;
    for (size_t i = 0; i < np; i++)
        if (cnt[i] < least) return false;
    return true;
}

pt_atrous_config config(const double *sig, int32_t T) { return {T, 0, sig[0], sig[1], sig[2], sig[3]}; }

// The buffers pt_atrous and pt_temporal run the filter on (ctx->at, f_rgba).
struct FilterBufs {
    size_t np;
    uint32_t grid1;
    Buf<double> col0, col1, var0, var1;
    Buf<pta::Guide> guide;
    Buf<ptk::NoisePartial> part;
    Buf<uint8_t> rgba;
    explicit FilterBufs(size_t npix)
        : np(npix), grid1(ptl::grid_1d(npix)), col0(nullptr, 3 * npix), col1(nullptr, 3 * npix), var0(nullptr, npix),
          var1(nullptr, npix), guide(nullptr, npix), part(nullptr, 2 * (size_t)grid1), rgba(nullptr, 4 * npix) {}
    hipError_t status() const {
        hipError_t st = hipSuccess;
        for (hipError_t e : {col0.st, col1.st, var0.st, var1.st, guide.st, part.st, rgba.st}) PROBE_TRY(e);
        return st;
    }
};

// What follows the kernel that leaves (col0, var0, guide): the product's sequence, without a filter when T < 0.  Returns the index of
// the buffers that hold the result.
int filter_tail(FilterBufs &B, int32_t W, int32_t H, int32_t T, const double *sig, bool feat) {
    double *const col[2] = {B.col0.d, B.col1.d}, *const var[2] = {B.var0.d, B.var1.d};
    const pta::Params P = ptl::filter_params(config(sig, T), feat);
    return ptl::filter_sequence(T >= 0 ? &P : nullptr, col, var, B.guide.d, B.part.d, B.rgba.d, W, H, 0);
}

// mean, var and rgba of the result, and the partials.
int filter_results(FilterBufs &B, int cur, double *mean, double *var, uint8_t *rgba, std::vector<ptk::NoisePartial> &part) {
    part.resize(2 * (size_t)B.grid1);
    int rc = (int)B.part.download(part.data());
    if (!rc) rc = (int)(cur ? B.col1 : B.col0).download(mean);
    if (!rc) rc = (int)(cur ? B.var1 : B.var0).download(var);
    return rc ? rc : (int)B.rgba.download(rgba);
}

// The history of probe_temporal_*: what pt_ctx keeps (tp_hist, tp_cur, tp_valid, tp_w, tp_h, tp_cam).
struct State {
    double *hist[2] = {nullptr, nullptr};
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

// pt_atrous's chain on a W x H frame: S, Q [H][W][3] raw sums; cnt [H][W] or null (n everywhere); fn, fa, fd the feature sums or all
// null; T iterations; sig = {sigma_l, sigma_n, sigma_z, sigma_a}.  mean [H][W][3], var [H][W], rgba [H][W][4], noise[2] = before,
// after; bad = the bad pixels.  (The arguments of atrous_support's shim_filter.)
int probe_filter(int32_t W, int32_t H, const double *S, const double *Q, const uint32_t *cnt, uint32_t n, const double *fn, const double *fa,
                 const double *fd, int32_t T, const double *sig, double *mean, double *var, uint8_t *rgba, double *noise, uint64_t *bad) {
    if (!size_ok(W, H, 1) || T < 0 || T > PTA_MAX_ITERATIONS) return -1;
    if (!S || !Q || !sig || !mean || !var || !rgba || !noise || !bad) return -2;
    const bool feat = fn && fa && fd;
    if (!feat && (fn || fa || fd)) return -3;
    if (!(sig[0] > 0.0) || !(sig[1] >= 0.0) || !(sig[2] >= 0.0) || !(sig[3] >= 0.0)) return -4;
    const size_t np = (size_t)W * (size_t)H;
    if (!counts_ok(cnt, n, np, 2)) return -5;
    Buf<double> dS(S, 3 * np), dQ(Q, 3 * np), dfn(fn, feat ? 3 * np : 0), dfa(fa, feat ? 3 * np : 0), dfd(fd, feat ? 3 * np : 0);
    Buf<uint32_t> dcnt(cnt, cnt ? np : 0);
    FilterBufs B(np);
    hipError_t st = B.status();
    for (hipError_t e : {dS.st, dQ.st, dfn.st, dfa.st, dfd.st, dcnt.st}) PROBE_TRY(e);
    if (st != hipSuccess) return (int)st;
    ptk::AtrousPrepArgs PA;
    std::memset(&PA, 0, sizeof PA);
    PA.acc = dS.d;
    PA.m2 = dQ.d;
    PA.cnt = cnt ? dcnt.d : nullptr;
    PA.fn = feat ? dfn.d : nullptr;
    PA.fa = feat ? dfa.d : nullptr;
    PA.fd = feat ? dfd.d : nullptr;
    PA.col = B.col0.d;
    PA.var = B.var0.d;
    PA.guide = B.guide.d;
    PA.npix = (uint32_t)np;
    PA.n = n;
    hipLaunchKernelGGL(ptk::atrous_prep_kernel, dim3(B.grid1), dim3(PT_BLOCK), 0, 0, PA);
    const int cur = filter_tail(B, W, H, T, sig, feat);
    int rc = finish(st);
    if (rc) return rc;
    std::vector<ptk::NoisePartial> part;
    rc = filter_results(B, cur, mean, var, rgba, part);
    if (rc) return rc;
    const ptl::NoiseFigures f = ptl::noise_figures(part.data(), B.grid1, true, np);
    *bad = f.bad;
    noise[0] = f.before;
    noise[1] = f.after;
    return 0;
}

// pt_atrous_halves's chain: the four half sums [H][W][3], the pixel's own count (cnt or n, at least 4), the feature sums or all null.
// mean [H][W][3], err [H][W], half_means [2][H][W][3], noise[2] = measured, model; bad.  (The arguments of halves_support's shim_pair.)
int probe_pair(int32_t W, int32_t H, const double *SA, const double *QA, const double *SB, const double *QB, const uint32_t *cnt, uint32_t n,
               const double *fn, const double *fa, const double *fd, int32_t T, const double *sig, double *mean, double *err,
               double *half_means, double *noise, uint64_t *bad) {
    if (!size_ok(W, H, 1) || T < 0 || T > PTA_MAX_ITERATIONS) return -1;
    if (!SA || !QA || !SB || !QB || !sig || !mean || !err || !half_means || !noise || !bad) return -2;
    const bool feat = fn && fa && fd;
    if (!feat && (fn || fa || fd)) return -3;
    if (!(sig[0] > 0.0) || !(sig[1] >= 0.0) || !(sig[2] >= 0.0) || !(sig[3] >= 0.0)) return -4;
    const size_t np = (size_t)W * (size_t)H;
    if (!counts_ok(cnt, n, np, 4)) return -5;
    const uint32_t grid1 = ptl::grid_1d(np);
    Buf<double> dSA(SA, 3 * np), dQA(QA, 3 * np), dSB(SB, 3 * np), dQB(QB, 3 * np);
    Buf<double> dfn(fn, feat ? 3 * np : 0), dfa(fa, feat ? 3 * np : 0), dfd(fd, feat ? 3 * np : 0);
    Buf<uint32_t> dcnt(cnt, cnt ? np : 0);
    Buf<double> guide(nullptr, PTA_GUIDE_PLANES * np), col0(nullptr, 6 * np), col1(nullptr, 6 * np), var0(nullptr, 2 * np), var1(nullptr, 2 * np);
    Buf<double> dmean(nullptr, 3 * np), derr(nullptr, np), dhalf(nullptr, 6 * np);
    Buf<ptk::HalvesPartial> dpart(nullptr, grid1);
    hipError_t st = hipSuccess;
    for (hipError_t e : {dSA.st, dQA.st, dSB.st, dQB.st, dfn.st, dfa.st, dfd.st, dcnt.st, guide.st, col0.st, col1.st, var0.st, var1.st, dmean.st,
                         derr.st, dhalf.st, dpart.st})
        PROBE_TRY(e);
    if (st != hipSuccess) return (int)st;
    double *const col[2] = {col0.d, col1.d}, *const var[2] = {var0.d, var1.d};
    ptk::AtrousPairPrepArgs PA;
    std::memset(&PA, 0, sizeof PA);
    PA.sa = dSA.d; PA.qa = dQA.d; PA.sb = dSB.d; PA.qb = dQB.d;
    PA.cnt = cnt ? dcnt.d : nullptr;
    PA.fn = feat ? dfn.d : nullptr;
    PA.fa = feat ? dfa.d : nullptr;
    PA.fd = feat ? dfd.d : nullptr;
    PA.guide = guide.d;
    PA.col = col[0];
    PA.var = var[0];
    PA.npix = (uint32_t)np;
    PA.n = n;
    hipLaunchKernelGGL(ptk::atrous_pair_prep_kernel, dim3(grid1), dim3(PT_BLOCK), 0, 0, PA);
    const int cur = ptl::pair_iterations(ptl::filter_params(config(sig, T), feat), col, var, guide.d, W, H, 0);
    ptk::HalvesCombineArgs CA;
    std::memset(&CA, 0, sizeof CA);
    CA.col = col[cur]; CA.var = var[cur]; CA.guide = guide.d;
    CA.mean = dmean.d;
    CA.err = derr.d;
    CA.half_means = dhalf.d;
    CA.partial = dpart.d;
    CA.npix = (uint32_t)np;
    hipLaunchKernelGGL(ptk::halves_combine_kernel, dim3(grid1), dim3(PT_BLOCK), 0, 0, CA);
    int rc = finish(st);
    if (rc) return rc;
    std::vector<ptk::HalvesPartial> part(grid1);
    rc = (int)dpart.download(part.data());
    if (!rc) rc = (int)dmean.download(mean);
    if (!rc) rc = (int)derr.download(err);
    if (!rc) rc = (int)dhalf.download(half_means);
    if (rc) return rc;
    const ptl::HalvesFigures f = ptl::halves_figures(part.data(), grid1, np);
    *bad = f.bad;
    noise[0] = f.noise;
    noise[1] = f.noise_model;
    return 0;
}

// A history: two sets of device planes, the stored camera and valid / W / H, as pt_ctx keeps them for pt_temporal.
void *probe_temporal_new() { return new State(); }

void probe_temporal_free(void *sp) {
    State *s = static_cast<State *>(sp);
    if (!s) return;
    for (int k = 0; k < 2; k++)
        if (s->hist[k]) (void)hipFree(s->hist[k]);
    delete s;
}

void probe_temporal_reset(void *sp) {
    if (sp) static_cast<State *>(sp)->valid = false;
}

// pt_temporal_read: *valid = 0 and nothing written when the history is empty; else mean [H][W][3], var [H][W], len [H][W] of it.
int probe_temporal_read(void *sp, double *mean, double *var, int32_t *len, int32_t *valid) {
    if (!sp || !mean || !var || !len || !valid) return -2;
    State &s = *static_cast<State *>(sp);
    *valid = s.valid ? 1 : 0;
    if (!s.valid) return 0;
    const size_t np = (size_t)s.W * (size_t)s.H;
    std::vector<double> h((size_t)PTT_PLANES * np);
    hipError_t st = hipSuccess;
    PROBE_TRY(hipMemcpy(h.data(), s.hist[s.cur], h.size() * sizeof(double), hipMemcpyDeviceToHost));
    if (st != hipSuccess) return (int)st;
    for (size_t i = 0; i < np; i++) {
        for (size_t k = 0; k < 3; k++) mean[3 * i + k] = h[k * np + i];
        var[i] = h[(size_t)PTT_VAR * np + i];
        std::memcpy(&len[i], reinterpret_cast<const char *>(&h[(size_t)PTT_LH * np]) + 8 * i, sizeof(int32_t));
    }
    return 0;
}

// pt_temporal's chain on one frame: S, Q, the feature sums [H][W][3]; cam22 = this frame's camera; tcfg = {alpha, tol_z, n_min, tol_a,
// max_len}; T < 0: no filter, else T iterations with sig.  mean, var, rgba as probe_filter; noise[3] = before, blended, after;
// counts[4] = reprojected, disoccluded, bad, the sum of len'.  `place` is not written.  (The arguments of temporal_support's shim_frame.)
int probe_temporal_frame(void *sp, int32_t W, int32_t H, const double *S, const double *Q, const uint32_t *cnt, uint32_t n, const double *fn,
                         const double *fa, const double *fd, const double *cam22, const double *tcfg, int32_t T, const double *sig,
                         double *mean, double *var, uint8_t *rgba, double *noise, uint64_t *counts, double *place) {
    (void)place;
    if (!sp || !size_ok(W, H, 2) || T > PTA_MAX_ITERATIONS) return -1;
    if (!S || !Q || !fn || !fa || !fd || !cam22 || !tcfg || !sig || !mean || !var || !rgba || !noise || !counts) return -2;
    if (T >= 0 && (!(sig[0] > 0.0) || !(sig[1] >= 0.0) || !(sig[2] >= 0.0) || !(sig[3] >= 0.0))) return -4;
    if (!(tcfg[0] >= 0.0 && tcfg[0] <= 1.0) || !(tcfg[1] >= 0.0) || !(tcfg[3] >= 0.0) || tcfg[2] != tcfg[2] || !(tcfg[4] >= 1.0 && tcfg[4] <= 2147483647.0))
        return -6;
    State &s = *static_cast<State *>(sp);
    const size_t np = (size_t)W * (size_t)H;
    if (!counts_ok(cnt, n, np, 2)) return -5;
    const dim3 grid2 = ptl::grid_2d(W, H);
    const size_t nblk = (size_t)grid2.x * grid2.y;
    const bool have = s.valid && s.W == W && s.H == H;  // another size: the history is dropped (when the call succeeds)
    hipError_t st = hipSuccess;
    // both sets are kept at the size of this frame; a set that has to grow loses its contents
    for (int k = 0; k < 2; k++) {
        if (s.cap[k] >= (size_t)PTT_PLANES * np) continue;
        s.valid = false;
        if (s.hist[k]) (void)hipFree(s.hist[k]);
        s.hist[k] = nullptr;
        s.cap[k] = 0;
        PROBE_TRY(hipMalloc(reinterpret_cast<void **>(&s.hist[k]), (size_t)PTT_PLANES * np * sizeof(double)));
        if (st != hipSuccess) { s.hist[k] = nullptr; return (int)st; }
        s.cap[k] = (size_t)PTT_PLANES * np;
        PROBE_TRY(hipMemset(s.hist[k], 0xFF, s.cap[k] * sizeof(double)));
    }
    const int next = s.cur ^ 1;
    PROBE_TRY(hipMemset(s.hist[next], 0xFF, (size_t)PTT_PLANES * np * sizeof(double)));
    Buf<double> dS(S, 3 * np), dQ(Q, 3 * np), dfn(fn, 3 * np), dfa(fa, 3 * np), dfd(fd, 3 * np);
    Buf<uint32_t> dcnt(cnt, cnt ? np : 0);
    Buf<ptk::TemporalPartial> tpart(nullptr, nblk);
    FilterBufs B(np);
    PROBE_TRY(B.status());
    for (hipError_t e : {dS.st, dQ.st, dfn.st, dfa.st, dfd.st, dcnt.st, tpart.st}) PROBE_TRY(e);
    if (st != hipSuccess) return (int)st;
    ptk::TemporalArgs TA;
    std::memset(&TA, 0, sizeof TA);
    TA.C.alpha = tcfg[0]; TA.C.tol_z = tcfg[1]; TA.C.n_min = tcfg[2]; TA.C.tol_a = tcfg[3];
    TA.C.max_len = (int32_t)tcfg[4];
    TA.C.have_history = have ? 1 : 0;
    TA.V.cam = camera(cam22);
    TA.V.inv_width = 1.0 / (double)(W - 1);
    TA.V.inv_height = 1.0 / (double)(H - 1);
    TA.V.W = W;
    TA.V.H = H;
    TA.cam_h = s.cam;
    TA.acc = dS.d;
    TA.m2 = dQ.d;
    TA.cnt = cnt ? dcnt.d : nullptr;
    TA.fn = dfn.d;
    TA.fa = dfa.d;
    TA.fd = dfd.d;
    TA.hist = s.hist[s.cur];
    TA.hist_out = s.hist[next];
    TA.col = B.col0.d;
    TA.var = B.var0.d;
    TA.guide = B.guide.d;
    TA.partial = tpart.d;
    TA.n = n;
    hipLaunchKernelGGL(ptk::temporal_kernel, grid2, dim3(PT_BLOCK), 0, 0, TA);
    const int cur = filter_tail(B, W, H, T, sig, true);
    int rc = finish(st);
    if (rc) return rc;  // the stored history is untouched: the kernel wrote the other set
    std::vector<ptk::NoisePartial> part;
    std::vector<ptk::TemporalPartial> tp(nblk);
    rc = filter_results(B, cur, mean, var, rgba, part);
    if (!rc) rc = (int)tpart.download(tp.data());
    if (rc) return rc;
    s.cur = next;
    s.valid = true;
    s.W = W;
    s.H = H;
    s.cam = TA.V.cam;
    const ptl::TemporalFigures tf = ptl::temporal_figures(tp.data(), nblk, np);
    const ptl::NoiseFigures nf = ptl::noise_figures(part.data(), B.grid1, T >= 0, np);
    counts[0] = tf.reprojected;
    counts[1] = tf.disoccluded;
    counts[2] = nf.bad;
    counts[3] = tf.len_sum;
    noise[0] = tf.noise_before;
    noise[1] = nf.before;
    noise[2] = nf.after;
    return 0;
}

}  // extern "C"
