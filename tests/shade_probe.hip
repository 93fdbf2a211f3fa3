// shade_probe.hip -- test-only: the surface step of the trace kernels (csrc/pt_kernels.h: outward_normal, reflect_vec, shade_hit,
// dielectric_scatter, exit_post, roulette_advance) on the gfx950 device, one lane per case, on operands no rendered frame reaches.
//
// pt_kernels.h and pt_convert.h are included unchanged and compiled with the library's own flags (tests/shade_probe_support.py), so
// what runs here is the code libptcore.so ships, and the materials are converted by the product's convert_material.  The __global__
// wrappers give att, finished, exit_search, term and the counters the values the callers give them (trace_kernel's shade block,
// glass_kernel: att = 1, 1, 1, flags false).  Each extern "C" entry point uploads its host arrays, launches one wrapper over blocks of
// PT_BLOCK lanes, copies the results back and returns the first HIP status that was not hipSuccess (0 = fine; a negative value: the
// arguments were refused before anything was launched).  Every output array is GUARD elements longer than the case count and filled
// with 0xFF bytes before the launch: lanes beyond the count write nothing, so the caller finds the guard untouched.  No inline
// assembly.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "probe_common.h"
#include "pt_convert.h"
#include "pt_kernels.h"

namespace {

using namespace ptd;

const int64_t GUARD = 64;             // elements (rows) behind every output array
const int64_t MAX_CASES = (int64_t)1 << 22;
const int32_t MAX_MATS = 512;         // 64 KiB of LDS

struct ShadeIn {
    const DevObj *objs;   // [n] the object of each case; .mat indexes mats
    const DevMat *mats;   // [nmat]
    const double *t;      // [n] ora_hit's t
    const double *rays;   // [n][6]
    const uint64_t *rs;   // [n]
    int64_t n;
    int32_t nmat;
};
struct Out {
    int32_t *I;           // [n + GUARD][5]
    double *F;            // [n + GUARD][12]
    uint64_t *S;          // [n + GUARD]
};

// shade_hit as trace_kernel (LDS: the material table staged by stage_lds) and primary_bvh_kernel (global memory) call it.
// I = finished, exit_search, exit_mat, c_draw, j_draw;  F = term, att, origin, direction;  S = stream state.
template <bool STATS, bool GLASS, bool LDS>
__global__ void __launch_bounds__(PT_BLOCK) shade_wrap(ShadeIn in, Out out) {
    extern __shared__ __align__(16) unsigned char smem[];
    const DevMat *mats = in.mats;
    if (LDS) {
        ptk::stage_lds(smem, in.mats, in.nmat * (int)(sizeof(DevMat) / 8));
        mats = reinterpret_cast<const DevMat *>(smem);
    }
    const int64_t i = (int64_t)blockIdx.x * PT_BLOCK + threadIdx.x;
    if (i >= in.n) return;
    const double *r = in.rays + 6 * i;
    double ox = r[0], oy = r[1], oz = r[2], dx = r[3], dy = r[4], dz = r[5];
    uint64_t rs = in.rs[i];
    uint32_t c_draw = 0, j_draw = 0;
    bool finished = false, exit_search = false;
    int exit_mat = -1;
    double termx = 0, termy = 0, termz = 0, attx = 1, atty = 1, attz = 1;
    ptk::shade_hit<STATS, GLASS>(in.objs[i], mats, in.t[i], ox, oy, oz, dx, dy, dz, rs, c_draw, j_draw, finished, termx, termy, termz, attx,
                                 atty, attz, exit_search, exit_mat);
    int32_t *I = out.I + 5 * i;
    I[0] = finished; I[1] = exit_search; I[2] = exit_mat; I[3] = (int32_t)c_draw; I[4] = (int32_t)j_draw;
    double *F = out.F + 12 * i;
    F[0] = termx; F[1] = termy; F[2] = termz; F[3] = attx; F[4] = atty; F[5] = attz;
    F[6] = ox; F[7] = oy; F[8] = oz; F[9] = dx; F[10] = dy; F[11] = dz;
    out.S[i] = rs;
}

// glass_kernel's bounce up to its exit search, EXACTLY as it stands in the kernel body (pt_kernels.h, "hit record of the winner" to
// "double attx = 1, ..."): the kernel does not go through shade_hit.  THIS COPY AND THE KERNEL BODY MUST STAY THE SAME.
// I = finished, ff (the exit search would run), mi, c_draw, j_draw;  F = 0 x 3, att, origin, direction.
template <bool STATS>
__global__ void __launch_bounds__(PT_BLOCK) glass_wrap(ShadeIn in, Out out) {
    extern __shared__ __align__(16) unsigned char smem[];
    DevMat *lds_mat = reinterpret_cast<DevMat *>(smem);
    ptk::stage_copy(lds_mat, in.mats, in.nmat * (int)(sizeof(DevMat) / 8));
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * PT_BLOCK + threadIdx.x;
    if (i >= in.n) return;
    const double *ray = in.rays + 6 * i;
    double ox = ray[0], oy = ray[1], oz = ray[2], dx = ray[3], dy = ray[4], dz = ray[5];
    const double tmax = in.t[i];
    uint64_t rs = in.rs[i];
    uint32_t c_draw = 0, j_draw = 0;
    double attx = 1, atty = 1, attz = 1;
    bool exits = false;

    // hit record of the winner
    const DevObj &o = in.objs[i];
    const int kind = o.kind & 0xff;
    const double px = ox + dx * tmax, py = oy + dy * tmax, pz = oz + dz * tmax;
    double nx, ny, nz;
    ptk::outward_normal(o, kind, px, py, pz, nx, ny, nz);
    const bool ff = (dx * nx + dy * ny + dz * nz) < 0;
    if (!ff) { nx = -nx; ny = -ny; nz = -nz; }
    const int mi = o.mat;
    const DevMat &m = lds_mat[mi];
    bool finished = false;
    // materials.go:175-182
    const double dirLen = ptm::f_sqrt(dx * dx + dy * dy + dz * dz);
    if (dirLen == 0) {
        finished = true;  // scatter fails -> emitted (0)
    } else {
        const double invLen = 1.0 / dirLen;
        const double ux = dx * invLen, uy = dy * invLen, uz = dz * invLen;
        double rfx, rfy, rfz;
        ptk::reflect_vec(ux, uy, uz, nx, ny, nz, rfx, rfy, rfz);
        double ndx, ndy, ndz;
        ptk::dielectric_scatter<STATS>(m, ff, ux, uy, uz, nx, ny, nz, rfx, rfy, rfz, rs, c_draw, j_draw, ndx, ndy, ndz);
        // scattered ray starts at the hit point (no offset)
        ox = px; oy = py; oz = pz;
        dx = ndx; dy = ndy; dz = ndz;
        exits = ff;  // renderer.go:316-371: the way out, before roulette
    }

    int32_t *I = out.I + 5 * i;
    I[0] = finished; I[1] = exits; I[2] = mi; I[3] = (int32_t)c_draw; I[4] = (int32_t)j_draw;
    double *F = out.F + 12 * i;
    F[0] = 0; F[1] = 0; F[2] = 0; F[3] = attx; F[4] = atty; F[5] = attz;
    F[6] = ox; F[7] = oy; F[8] = oz; F[9] = dx; F[10] = dy; F[11] = dz;
    out.S[i] = rs;
}

// outward_normal at the reference's hit point: F[0..2] = the normal.
__global__ void __launch_bounds__(PT_BLOCK) normal_wrap(const DevObj *objs, const double *p, int64_t n, double *F) {
    const int64_t i = (int64_t)blockIdx.x * PT_BLOCK + threadIdx.x;
    if (i >= n) return;
    double nx, ny, nz;
    ptk::outward_normal(objs[i], objs[i].kind & 0xff, p[3 * i], p[3 * i + 1], p[3 * i + 2], nx, ny, nz);
    F[3 * i] = nx; F[3 * i + 1] = ny; F[3 * i + 2] = nz;
}

__global__ void __launch_bounds__(PT_BLOCK) reflect_wrap(const double *v, const double *nrm, int64_t n, double *F) {
    const int64_t i = (int64_t)blockIdx.x * PT_BLOCK + threadIdx.x;
    if (i >= n) return;
    double rx, ry, rz;
    ptk::reflect_vec(v[3 * i], v[3 * i + 1], v[3 * i + 2], nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2], rx, ry, rz);
    F[3 * i] = rx; F[3 * i + 1] = ry; F[3 * i + 2] = rz;
}

// exit_post on (material, best, tmax, the scattered ray, att): F = origin, att.
__global__ void __launch_bounds__(PT_BLOCK) exit_wrap(const DevMat *mats, const int32_t *mat, const int32_t *best, const double *tmax,
                                                      const double *rays, const double *att, int64_t n, double *F) {
    const int64_t i = (int64_t)blockIdx.x * PT_BLOCK + threadIdx.x;
    if (i >= n) return;
    const double *r = rays + 6 * i;
    double ox = r[0], oy = r[1], oz = r[2];
    double attx = att[3 * i], atty = att[3 * i + 1], attz = att[3 * i + 2];
    ptk::exit_post(mats[mat[i]], best[i], tmax[i], ox, oy, oz, r[3], r[4], r[5], attx, atty, attz);
    F[6 * i] = ox; F[6 * i + 1] = oy; F[6 * i + 2] = oz; F[6 * i + 3] = attx; F[6 * i + 4] = atty; F[6 * i + 5] = attz;
}

// roulette_advance on (depth, att, T, stream state): I = finished, depth afterwards, 0, c_draw, j_draw;  F = T;  S = stream state.
template <bool STATS>
__global__ void __launch_bounds__(PT_BLOCK) roulette_wrap(const int32_t *depth, const double *att, const double *T, const uint64_t *state,
                                                          int64_t n, Out out) {
    const int64_t i = (int64_t)blockIdx.x * PT_BLOCK + threadIdx.x;
    if (i >= n) return;
    int d = depth[i];
    double Tx = T[3 * i], Ty = T[3 * i + 1], Tz = T[3 * i + 2];
    uint64_t rs = state[i];
    uint32_t c_draw = 0, j_draw = 0;
    const bool finished = ptk::roulette_advance<STATS>(d, att[3 * i], att[3 * i + 1], att[3 * i + 2], Tx, Ty, Tz, rs, c_draw, j_draw);
    int32_t *I = out.I + 5 * i;
    I[0] = finished; I[1] = d; I[2] = 0; I[3] = (int32_t)c_draw; I[4] = (int32_t)j_draw;
    out.F[3 * i] = Tx; out.F[3 * i + 1] = Ty; out.F[3 * i + 2] = Tz;
    out.S[i] = rs;
}

bool count_ok(int64_t n) { return n > 0 && n <= MAX_CASES; }
unsigned grid_of(int64_t n) { return (unsigned)((n + PT_BLOCK - 1) / PT_BLOCK); }

// every object names a material of the table
bool mats_ok(const DevObj *objs, int64_t n, int32_t nmat) {
    if (nmat <= 0 || nmat > MAX_MATS) return false;
    for (int64_t i = 0; i < n; i++)
        if (objs[i].mat < 0 || objs[i].mat >= nmat) return false;
    return true;
}

std::vector<DevMat> convert_all(const pt_material *mats, int32_t nmat) {
    std::vector<DevMat> dm;
    for (int32_t k = 0; k < nmat; k++) dm.push_back(convert_material(mats[k]));
    return dm;
}

}  // namespace

extern "C" {

int64_t probe_shade_guard(void) { return GUARD; }

// variant: bit 0 STATS, bit 1 GLASS, bit 2 the glass_kernel sequence instead of shade_hit (LDS always).  lds: the material table
// through an LDS copy (trace_kernel) or from global memory (primary_bvh_kernel).
int probe_shade(int32_t variant, int32_t lds, const pt_material *mats, int32_t nmat, int64_t n, const DevObj *objs, const double *t,
                const double *rays, const uint64_t *state, int32_t *I, double *F, uint64_t *S) {
    if (!count_ok(n) || !mats_ok(objs, n, nmat) || variant < 0 || variant > 5) return -1;
    const std::vector<DevMat> dm = convert_all(mats, nmat);
    if (!(variant & 2) || (variant & 4))  // no dielectric reaches a GLASS = false instantiation; only dielectrics reach glass_kernel
        for (int64_t i = 0; i < n; i++)
            if ((dm[(size_t)objs[i].mat].typ == MAT_DIELECTRIC) != ((variant & 4) != 0)) return -2;
    hipError_t st = hipSuccess;
    Buf<DevObj> d_obj(objs, (size_t)n);
    Buf<DevMat> d_mat(dm.data(), dm.size());
    Buf<double> d_t(t, (size_t)n), d_ray(rays, 6 * (size_t)n), d_F(nullptr, 12 * (size_t)(n + GUARD));
    Buf<uint64_t> d_rs(state, (size_t)n), d_S(nullptr, (size_t)(n + GUARD));
    Buf<int32_t> d_I(nullptr, 5 * (size_t)(n + GUARD));
    for (hipError_t e : {d_obj.st, d_mat.st, d_t.st, d_ray.st, d_F.st, d_rs.st, d_S.st, d_I.st}) PROBE_TRY(e);
    if (st != hipSuccess) return (int)st;
    const ShadeIn in{d_obj.d, d_mat.d, d_t.d, d_ray.d, d_rs.d, n, nmat};
    const Out out{d_I.d, d_F.d, d_S.d};
    const size_t smem = (lds || (variant & 4)) ? (size_t)nmat * sizeof(DevMat) : 0;
    const dim3 g(grid_of(n)), b(PT_BLOCK);
#define SHADE_CASE(V, ST, GL)                                                                          \
    case V:                                                                                            \
        if (lds) hipLaunchKernelGGL((shade_wrap<ST, GL, true>), g, b, smem, 0, in, out);               \
        else hipLaunchKernelGGL((shade_wrap<ST, GL, false>), g, b, smem, 0, in, out);                  \
        break;
    switch (variant) {
        SHADE_CASE(0, false, false)
        SHADE_CASE(1, true, false)
        SHADE_CASE(2, false, true)
        SHADE_CASE(3, true, true)
        case 4: hipLaunchKernelGGL((glass_wrap<false>), g, b, smem, 0, in, out); break;
        default: hipLaunchKernelGGL((glass_wrap<true>), g, b, smem, 0, in, out); break;
    }
#undef SHADE_CASE
    st = (hipError_t)finish(st);
    PROBE_TRY(d_I.download(I));
    PROBE_TRY(d_F.download(F));
    PROBE_TRY(d_S.download(S));
    return (int)st;
}

// outward_normal: objs [n], p [n][3]; F [n + GUARD][3].
int probe_normal(int64_t n, const DevObj *objs, const double *p, double *F) {
    if (!count_ok(n)) return -1;
    hipError_t st = hipSuccess;
    Buf<DevObj> d_obj(objs, (size_t)n);
    Buf<double> d_p(p, 3 * (size_t)n), d_F(nullptr, 3 * (size_t)(n + GUARD));
    for (hipError_t e : {d_obj.st, d_p.st, d_F.st}) PROBE_TRY(e);
    if (st != hipSuccess) return (int)st;
    hipLaunchKernelGGL(normal_wrap, dim3(grid_of(n)), dim3(PT_BLOCK), 0, 0, d_obj.d, d_p.d, n, d_F.d);
    st = (hipError_t)finish(st);
    PROBE_TRY(d_F.download(F));
    return (int)st;
}

// reflect_vec: v, nrm [n][3]; F [n + GUARD][3].
int probe_reflect(int64_t n, const double *v, const double *nrm, double *F) {
    if (!count_ok(n)) return -1;
    hipError_t st = hipSuccess;
    Buf<double> d_v(v, 3 * (size_t)n), d_n(nrm, 3 * (size_t)n), d_F(nullptr, 3 * (size_t)(n + GUARD));
    for (hipError_t e : {d_v.st, d_n.st, d_F.st}) PROBE_TRY(e);
    if (st != hipSuccess) return (int)st;
    hipLaunchKernelGGL(reflect_wrap, dim3(grid_of(n)), dim3(PT_BLOCK), 0, 0, d_v.d, d_n.d, n, d_F.d);
    st = (hipError_t)finish(st);
    PROBE_TRY(d_F.download(F));
    return (int)st;
}

// exit_post: mat, best [n], tmax [n], rays [n][6], att [n][3]; F [n + GUARD][6] = origin, att.
int probe_exit(const pt_material *mats, int32_t nmat, int64_t n, const int32_t *mat, const int32_t *best, const double *tmax,
               const double *rays, const double *att, double *F) {
    if (!count_ok(n) || nmat <= 0 || nmat > MAX_MATS) return -1;
    for (int64_t i = 0; i < n; i++)
        if (mat[i] < 0 || mat[i] >= nmat) return -1;
    const std::vector<DevMat> dm = convert_all(mats, nmat);
    hipError_t st = hipSuccess;
    Buf<DevMat> d_mat(dm.data(), dm.size());
    Buf<int32_t> d_mi(mat, (size_t)n), d_best(best, (size_t)n);
    Buf<double> d_t(tmax, (size_t)n), d_ray(rays, 6 * (size_t)n), d_att(att, 3 * (size_t)n), d_F(nullptr, 6 * (size_t)(n + GUARD));
    for (hipError_t e : {d_mat.st, d_mi.st, d_best.st, d_t.st, d_ray.st, d_att.st, d_F.st}) PROBE_TRY(e);
    if (st != hipSuccess) return (int)st;
    hipLaunchKernelGGL(exit_wrap, dim3(grid_of(n)), dim3(PT_BLOCK), 0, 0, d_mat.d, d_mi.d, d_best.d, d_t.d, d_ray.d, d_att.d, n, d_F.d);
    st = (hipError_t)finish(st);
    PROBE_TRY(d_F.download(F));
    return (int)st;
}

// roulette_advance<stats>: depth [n], att, T [n][3], state [n]; I [n + GUARD][5], F [n + GUARD][3], S [n + GUARD].
int probe_roulette(int32_t stats, int64_t n, const int32_t *depth, const double *att, const double *T, const uint64_t *state, int32_t *I,
                   double *F, uint64_t *S) {
    if (!count_ok(n)) return -1;
    hipError_t st = hipSuccess;
    Buf<int32_t> d_depth(depth, (size_t)n), d_I(nullptr, 5 * (size_t)(n + GUARD));
    Buf<double> d_att(att, 3 * (size_t)n), d_T(T, 3 * (size_t)n), d_F(nullptr, 3 * (size_t)(n + GUARD));
    Buf<uint64_t> d_rs(state, (size_t)n), d_S(nullptr, (size_t)(n + GUARD));
    for (hipError_t e : {d_depth.st, d_I.st, d_att.st, d_T.st, d_F.st, d_rs.st, d_S.st}) PROBE_TRY(e);
    if (st != hipSuccess) return (int)st;
    const Out out{d_I.d, d_F.d, d_S.d};
    if (stats) hipLaunchKernelGGL((roulette_wrap<true>), dim3(grid_of(n)), dim3(PT_BLOCK), 0, 0, d_depth.d, d_att.d, d_T.d, d_rs.d, n, out);
    else hipLaunchKernelGGL((roulette_wrap<false>), dim3(grid_of(n)), dim3(PT_BLOCK), 0, 0, d_depth.d, d_att.d, d_T.d, d_rs.d, n, out);
    st = (hipError_t)finish(st);
    PROBE_TRY(d_I.download(I));
    PROBE_TRY(d_F.download(F));
    PROBE_TRY(d_S.download(S));
    return (int)st;
}

}  // extern "C"
