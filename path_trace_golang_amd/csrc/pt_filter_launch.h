// pt_filter_launch.h -- host side of the post-frame filters: the launch sequences of pt_atrous, pt_temporal and
// pt_atrous_halves behind their first kernel, the grids of a W x H frame, the filter's Params and the sums of the kernels' partials;
// and the two sequences of pt_set_adaptive_filtered's check: the block map on devices[0], the map applied per device.
//
// Inline host functions over raw device pointers, sizes and a stream: no context, no buffer ownership, no error texts.  ptcore.hip
// runs them on its own buffers and tests/denoise_probe.hip, tests/temporal_clip_probe.hip and tests/filtered_adaptive_probe.hip on
// theirs, so the probes launch the product's sequence itself.  The launches report through hipGetLastError, which the caller reads after the last one.
#pragma once

#include <cmath>
#include <cstring>

#include "pt_kernels.h"

namespace ptl {

// One thread per pixel; one 32 x 8 block of atrous_kernel / atrous_pair_kernel / temporal_kernel per 32 x 8 pixels.
inline uint32_t grid_1d(size_t npix) { return (uint32_t)((npix + PT_BLOCK - 1) / PT_BLOCK); }
inline dim3 grid_2d(int32_t W, int32_t H) { return dim3((unsigned)((W + 31) / 32), (unsigned)((H + 7) / 8)); }

// A feature term is on when its sigma is and the frame has features.
inline pta::Params filter_params(const pt_atrous_config &c, bool features) {
    pta::Params P;
    std::memset(&P, 0, sizeof P);
    P.sigma_l = c.sigma_l; P.sigma_n = c.sigma_n; P.sigma_z = c.sigma_z; P.sigma_a = c.sigma_a;
    P.iterations = c.iterations;
    P.n_on = features && c.sigma_n > 0.0;
    P.z_on = features && c.sigma_z > 0.0;
    P.a_on = features && c.sigma_a > 0.0;
    return P;
}

// P.iterations iterations of Kernel at steps 1, 2, 4, ... from (col[0], var[0]), ping-pong.  Returns the index of the buffers that
// hold the result.
template <typename Args, void (*Kernel)(const Args), typename Guide>
int iterate(const pta::Params &P, double *const col[2], double *const var[2], const Guide *guide, int32_t W, int32_t H, hipStream_t stream) {
    Args A;
    std::memset(&A, 0, sizeof A);
    A.P = P;
    A.guide = guide;
    A.W = W;
    A.H = H;
    int cur = 0;
    for (int32_t t = 0; t < P.iterations; t++, cur ^= 1) {
        A.col = col[cur]; A.var = var[cur];
        A.col_out = col[cur ^ 1]; A.var_out = var[cur ^ 1];
        A.step = 1 << t;
        hipLaunchKernelGGL(Kernel, grid_2d(W, H), dim3(PT_BLOCK), 0, stream, A);
    }
    return cur;
}

// pt_atrous_halves's iterations on the planes of both halves.
inline int pair_iterations(const pta::Params &P, double *const col[2], double *const var[2], const double *guide, int32_t W, int32_t H,
                           hipStream_t stream) {
    return iterate<ptk::AtrousPairArgs, ptk::atrous_pair_kernel>(P, col, var, guide, W, H, stream);
}

// The check of pt_set_adaptive_filtered behind the pair filter's combine (pt_atrous.h BLOCKS, steps 2 to 4), on devices[0]: the
// per-block sums of the (mean, err, bad) planes, then the pooled figure, the block's own and the stop flag of every block of the
// frame's grid.
struct BlockMap {
    double *s;        // [nbx * nby]
    uint32_t *k;      // [nbx * nby]
    double *pooled;   // [nbx * nby]
    double *own;      // [nbx * nby]
    uint8_t *stop;    // [nbx * nby]
};
inline int32_t blocks_across(int32_t n) { return (n + 7) / 8; }
inline void block_map_sequence(const double *mean, const double *err, const double *bad, const BlockMap &M, int32_t W, int32_t H, int32_t pool,
                               double target, hipStream_t stream) {
    const int32_t nbx = blocks_across(W), nby = blocks_across(H);
    const size_t nb = (size_t)nbx * (size_t)nby;
    ptk::BlockErrArgs E;
    std::memset(&E, 0, sizeof E);
    E.mean = mean; E.err = err; E.bad = bad;
    E.s = M.s; E.k = M.k;
    E.W = W; E.H = H; E.nbx = nbx; E.nby = nby;
    hipLaunchKernelGGL(ptk::block_err_kernel, dim3(grid_1d(nb * 64u)), dim3(PT_BLOCK), 0, stream, E);
    ptk::BlockPoolArgs Q;
    std::memset(&Q, 0, sizeof Q);
    Q.s = M.s; Q.k = M.k;
    Q.pooled = M.pooled; Q.own = M.own; Q.stop = M.stop;
    Q.target = target;
    Q.nbx = nbx; Q.nby = nby; Q.pool = pool;
    hipLaunchKernelGGL(ptk::block_pool_kernel, dim3(grid_1d(nb)), dim3(PT_BLOCK), 0, stream, Q);
}

// ... and on every device: the map (null before the check decides) applied to the nact entries of the active list, then compact_kernel
// as dev_adaptive_check launches it.  K.keep and K.noise are A's.
inline void keep_sequence(const ptk::KeepFromMapArgs &A, const ptk::CompactArgs *K, hipStream_t stream) {
    hipLaunchKernelGGL(ptk::keep_from_map_kernel, dim3(grid_1d(A.nact)), dim3(PT_BLOCK), 0, stream, A);
    if (K) hipLaunchKernelGGL(ptk::compact_kernel, dim3(1), dim3(PT_COMPACT_BLOCK), 0, stream, *K);
}

// What pt_atrous and pt_temporal run behind the kernel that leaves (col[0], var[0], guide): the figure of that state into
// part[0 .. grid), then -- with a filter (P not null) -- its iterations and the figure of their result into part[grid .. 2 grid), then
// the finish of the result into rgba (gl_finish: by GL's tone map, for a frame rendered with GL shading).  Returns the index of the
// buffers that hold the result.
inline int filter_sequence(const pta::Params *P, double *const col[2], double *const var[2], const pta::Guide *guide, ptk::NoisePartial *part,
                           uint8_t *rgba, int32_t W, int32_t H, hipStream_t stream, bool gl_finish = false) {
    const uint32_t npix = (uint32_t)((size_t)W * (size_t)H), grid = grid_1d(npix);
    hipLaunchKernelGGL(ptk::atrous_noise_kernel, dim3(grid), dim3(PT_BLOCK), 0, stream, col[0], var[0], guide, part, npix);
    int cur = 0;
    if (P) {
        cur = iterate<ptk::AtrousArgs, ptk::atrous_kernel>(*P, col, var, guide, W, H, stream);
        hipLaunchKernelGGL(ptk::atrous_noise_kernel, dim3(grid), dim3(PT_BLOCK), 0, stream, col[cur], var[cur], guide, part + grid, npix);
    }
    if (gl_finish) hipLaunchKernelGGL(ptk::atrous_finish_gl_kernel, dim3(grid), dim3(PT_BLOCK), 0, stream, col[cur], rgba, npix);
    else hipLaunchKernelGGL(ptk::atrous_finish_kernel, dim3(grid), dim3(PT_BLOCK), 0, stream, col[cur], rgba, npix);
    return cur;
}

// The figures of the partials, copied to the host: every sum in block order, sqrt(sum / npix).

// filter_sequence's: `after` is `before` without a filter; the bad pixels are those of the first pass.
struct NoiseFigures {
    double before, after;
    uint64_t bad;
};
inline NoiseFigures noise_figures(const ptk::NoisePartial *part, uint32_t grid, bool filtered, size_t npix) {
    double sum[2] = {0.0, 0.0};
    NoiseFigures r = {0.0, 0.0, 0};
    for (uint32_t b = 0; b < grid; b++) {
        sum[0] += part[b].sum;
        r.bad += part[b].bad;
        if (filtered) sum[1] += part[(size_t)grid + b].sum;
    }
    r.before = std::sqrt(sum[0] / (double)npix);
    r.after = filtered ? std::sqrt(sum[1] / (double)npix) : r.before;
    return r;
}

// halves_combine_kernel's
struct HalvesFigures {
    double noise, noise_model;
    uint64_t bad;
};
inline HalvesFigures halves_figures(const ptk::HalvesPartial *part, uint32_t grid, size_t npix) {
    double sum = 0.0, sum_model = 0.0;
    HalvesFigures r = {0.0, 0.0, 0};
    for (uint32_t b = 0; b < grid; b++) {
        sum += part[b].sum;
        sum_model += part[b].sum_model;
        r.bad += part[b].bad;
    }
    r.noise = std::sqrt(sum / (double)npix);
    r.noise_model = std::sqrt(sum_model / (double)npix);
    return r;
}

// temporal_kernel's: the figure of the frame before the blend and the counts
struct TemporalFigures {
    double noise_before;
    uint64_t reprojected, disoccluded, clipped, len_sum;
    uint64_t moved, moved_reprojected;  // step 4a's counts (0 without a motion table)
};
inline TemporalFigures temporal_figures(const ptk::TemporalPartial *part, size_t nblk, size_t npix) {
    double sum = 0.0;
    TemporalFigures r = {0.0, 0, 0, 0, 0, 0, 0};
    for (size_t b = 0; b < nblk; b++) {
        sum += part[b].sum_before;
        r.reprojected += part[b].reprojected;
        r.disoccluded += part[b].disoccluded;
        r.clipped += part[b].clipped;
        r.len_sum += part[b].len_sum;
        r.moved += part[b].moved;
        r.moved_reprojected += part[b].moved_reprojected;
    }
    r.noise_before = std::sqrt(sum / (double)npix);
    return r;
}

}  // namespace ptl
