// roulette_probe.hip -- test-only: the roulette step of the trace kernels that reads a record of the roulette table
// (csrc/pt_kernels.h: roulette_table_advance, roulette_step; the table: csrc/pt_convert.h roulette_record) on the gfx950 device, one
// lane per case, in the style of shade_probe.hip.
//
// pt_kernels.h and pt_convert.h are included unchanged and compiled with the library's own flags (tests/roulette_probe_support.py).
// Every case has a record of its own, built here on the host by the product's roulette_record from the case's attenuation -- as
// scene_prepare builds a material's from its albedo.  The kernel reads it through an LDS copy (the block's PT_BLOCK records, staged
// by stage_lds: trace_kernel's flat scans, glass_kernel) or from global memory (the BVH form, primary_bvh_kernel, the wavefront
// passes).  With `mixed` every third lane has no record (rec < 0) and takes roulette_advance behind roulette_step's ballot, as a
// dielectric bounce through absorbing glass does; the results must be the same.  Each output array is GUARD rows longer than the
// case count and filled with 0xFF bytes before the launch: lanes beyond the count write nothing.  No inline assembly.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "probe_common.h"
#include "pt_convert.h"
#include "pt_kernels.h"

namespace {

using namespace ptd;

const int64_t GUARD = 64;
const int64_t MAX_CASES = (int64_t)1 << 22;

struct Out {
    int32_t *I;   // [n + GUARD][5] finished, depth afterwards, record used (1) or not (0), c_draw, j_draw
    double *F;    // [n + GUARD][3] T
    uint64_t *S;  // [n + GUARD] stream state
};

template <bool STATS, bool LDS, bool MIXED>
__global__ void __launch_bounds__(PT_BLOCK) table_wrap(const int32_t *depth, const double *att, const double *T, const uint64_t *state,
                                                       const DevRoulette *recs, int64_t n, Out out) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int64_t b0 = (int64_t)blockIdx.x * PT_BLOCK;
    const DevRoulette *tab = recs + b0;  // the block's records; lane t takes record t
    if (LDS) {
        const int64_t left = n - b0;
        const int cnt = (int)(left < PT_BLOCK ? left : PT_BLOCK);
        ptk::stage_lds(smem, recs + b0, cnt * (int)(sizeof(DevRoulette) / 8));
        tab = reinterpret_cast<const DevRoulette *>(smem);
    }
    const int64_t i = b0 + threadIdx.x;
    if (i >= n) return;
    int d = depth[i];
    double Tx = T[3 * i], Ty = T[3 * i + 1], Tz = T[3 * i + 2];
    uint64_t rs = state[i];
    uint32_t c_draw = 0, j_draw = 0;
    const int rec = (MIXED && i % 3 == 2) ? -1 : (int)threadIdx.x;
    bool finished;
    if (MIXED) finished = ptk::roulette_step<STATS>(tab, rec, d, att[3 * i], att[3 * i + 1], att[3 * i + 2], Tx, Ty, Tz, rs, c_draw, j_draw);
    else finished = ptk::roulette_table_advance<STATS>(d, tab[rec], att[3 * i], att[3 * i + 1], att[3 * i + 2], Tx, Ty, Tz, rs, c_draw, j_draw);
    int32_t *I = out.I + 5 * i;
    I[0] = finished; I[1] = d; I[2] = rec >= 0; I[3] = (int32_t)c_draw; I[4] = (int32_t)j_draw;
    out.F[3 * i] = Tx; out.F[3 * i + 1] = Ty; out.F[3 * i + 2] = Tz;
    out.S[i] = rs;
}

}  // namespace

extern "C" {

int64_t probe_roulette_guard(void) { return GUARD; }

// The product's record of every attenuation (host): att [n][3] -> rec [n][4] = prob, q.
void probe_roulette_records(int64_t n, const double *att, double *rec) {
    for (int64_t i = 0; i < n; i++) {
        const DevRoulette r = roulette_record(att[3 * i], att[3 * i + 1], att[3 * i + 2]);
        rec[4 * i] = r.prob; rec[4 * i + 1] = r.q[0]; rec[4 * i + 2] = r.q[1]; rec[4 * i + 3] = r.q[2];
    }
}

// variant: bit 0 STATS, bit 1 the records through LDS, bit 2 mixed (every third lane without a record).
// depth [n], att, T [n][3], state [n]; I [n + GUARD][5], F [n + GUARD][3], S [n + GUARD].
int probe_roulette_table(int32_t variant, int64_t n, const int32_t *depth, const double *att, const double *T, const uint64_t *state,
                         int32_t *I, double *F, uint64_t *S) {
    if (n <= 0 || n > MAX_CASES || variant < 0 || variant > 7) return -1;
    std::vector<DevRoulette> recs((size_t)n);
    for (int64_t i = 0; i < n; i++) recs[(size_t)i] = roulette_record(att[3 * i], att[3 * i + 1], att[3 * i + 2]);
    hipError_t st = hipSuccess;
    Buf<int32_t> d_depth(depth, (size_t)n), d_I(nullptr, 5 * (size_t)(n + GUARD));
    Buf<double> d_att(att, 3 * (size_t)n), d_T(T, 3 * (size_t)n), d_F(nullptr, 3 * (size_t)(n + GUARD));
    Buf<uint64_t> d_rs(state, (size_t)n), d_S(nullptr, (size_t)(n + GUARD));
    Buf<DevRoulette> d_rec(recs.data(), recs.size());
    for (hipError_t e : {d_depth.st, d_I.st, d_att.st, d_T.st, d_F.st, d_rs.st, d_S.st, d_rec.st}) PROBE_TRY(e);
    if (st != hipSuccess) return (int)st;
    const Out out{d_I.d, d_F.d, d_S.d};
    const dim3 g((unsigned)((n + PT_BLOCK - 1) / PT_BLOCK)), b(PT_BLOCK);
    const size_t smem = (variant & 2) ? (size_t)PT_BLOCK * sizeof(DevRoulette) : 0;
#define TABLE_CASE(V, ST, LD, MX) \
    case V: hipLaunchKernelGGL((table_wrap<ST, LD, MX>), g, b, smem, 0, d_depth.d, d_att.d, d_T.d, d_rs.d, d_rec.d, n, out); break;
    switch (variant) {
        TABLE_CASE(0, false, false, false)
        TABLE_CASE(1, true, false, false)
        TABLE_CASE(2, false, true, false)
        TABLE_CASE(3, true, true, false)
        TABLE_CASE(4, false, false, true)
        TABLE_CASE(5, true, false, true)
        TABLE_CASE(6, false, true, true)
        default: hipLaunchKernelGGL((table_wrap<true, true, true>), g, b, smem, 0, d_depth.d, d_att.d, d_T.d, d_rs.d, d_rec.d, n, out); break;
    }
#undef TABLE_CASE
    st = (hipError_t)finish(st);
    PROBE_TRY(d_I.download(I));
    PROBE_TRY(d_F.download(F));
    PROBE_TRY(d_S.download(S));
    return (int)st;
}

}  // extern "C"
