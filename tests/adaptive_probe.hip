// adaptive_probe.hip -- test-only: the two kernels of the adaptive check (csrc/pt_kernels.h), each by itself, on the
// gfx950 device, on active lists of any length.
//
// pt_kernels.h is included unchanged and compiled with the library's own flags (tests/adaptive_probe_support.py), so what runs
// here is the code libptcore.so ships.  Each extern "C" entry point uploads its host arrays, launches the product kernel with
// the grid expression of dev_adaptive_check (ptcore.hip), copies the results back and returns the first HIP status that was not
// hipSuccess (0 = fine; a negative value: the arguments were refused before anything was launched).  Every output buffer has
// its full size and is filled with 0xFF bytes before the launch, so what a kernel did not write reads 0xFFFFFFFF (or a NaN).
// No inline assembly.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "probe_common.h"
#include "pt_kernels.h"

extern "C" {

// compact_kernel on a list of nact >= 1 entries.  next_out [nact] (what follows the kept entries stays 0xFFFFFFFF);
// res_out: one ptk::AdaptResult (16 bytes).
int probe_compact(const uint32_t *active, const uint32_t *keep, const double *noise, int64_t nact, uint32_t *next_out, void *res_out) {
    if (nact <= 0 || nact > (int64_t)1 << 30) return -1;
    const size_t n = (size_t)nact;
    Buf<uint32_t> dact(active, n), dkeep(keep, n), dnext(nullptr, n);
    Buf<double> dnoise(noise, n);
    Buf<ptk::AdaptResult> dres(nullptr, 1);
    hipError_t st = hipSuccess;
    for (hipError_t e : {dact.st, dkeep.st, dnext.st, dnoise.st, dres.st}) PROBE_TRY(e);
    if (st != hipSuccess) return (int)st;
    ptk::CompactArgs K = {};
    K.active = dact.d;
    K.keep = dkeep.d;
    K.noise = dnoise.d;
    K.next = dnext.d;
    K.res = dres.d;
    K.nact = (uint32_t)nact;
    hipLaunchKernelGGL(ptk::compact_kernel, dim3(1), dim3(PT_COMPACT_BLOCK), 0, 0, K);
    int rc = finish(st);
    if (rc) return rc;
    rc = (int)dnext.download(next_out);
    return rc ? rc : (int)dres.download(static_cast<ptk::AdaptResult *>(res_out));
}

// block_noise_kernel on a shard of nslots slots (a multiple of 1024: whole tiles) with nact >= 1 active blocks, each below
// nslots / 64.  acc, m2 [3][nslots]; geom = {width, height, ntx, shard_index, shard_count} (TileGeom); blk_spp_out [nslots / 64]
// (the blocks that are not in the list stay 0xFFFFFFFF); keep_out, noise_out [nact].
int probe_block_noise(const double *acc, const double *m2, int64_t nslots, const uint32_t *active, int64_t nact, int32_t n, int32_t decide,
                      double target, const int32_t *geom, uint32_t *blk_spp_out, uint32_t *keep_out, double *noise_out) {
    if (nslots <= 0 || nslots % 1024 != 0 || nslots > (int64_t)1 << 30 || nact <= 0 || nact > nslots / 64) return -1;
    for (int64_t i = 0; i < nact; i++)
        if (active[i] >= (uint64_t)(nslots / 64)) return -2;  // the kernel would read acc and write blk_spp out of bounds
    for (int k = 0; k < 5; k++)
        if (geom[k] < (k == 3 ? 0 : 1)) return -3;
    const size_t ns = (size_t)nslots, na = (size_t)nact;
    Buf<double> dacc(acc, 3 * ns), dm2(m2, 3 * ns), dnoise(nullptr, na);
    Buf<uint32_t> dact(active, na), dspp(nullptr, ns / 64), dkeep(nullptr, na);
    hipError_t st = hipSuccess;
    for (hipError_t e : {dacc.st, dm2.st, dnoise.st, dact.st, dspp.st, dkeep.st}) PROBE_TRY(e);
    if (st != hipSuccess) return (int)st;
    ptk::BlockNoiseArgs A = {};
    A.acc = dacc.d;
    A.m2 = dm2.d;
    A.active = dact.d;
    A.blk_spp = dspp.d;
    A.keep = dkeep.d;
    A.noise = dnoise.d;
    A.target = target;
    A.nslots = (uint32_t)nslots;
    A.nact = (uint32_t)nact;
    A.n = n;
    A.decide = decide;
    A.G.width = geom[0];
    A.G.height = geom[1];
    A.G.ntx = geom[2];
    A.G.shard_index = geom[3];
    A.G.shard_count = geom[4];
    hipLaunchKernelGGL(ptk::block_noise_kernel, dim3((A.nact * 64u + PT_BLOCK - 1) / PT_BLOCK), dim3(PT_BLOCK), 0, 0, A);
    int rc = finish(st);
    if (rc) return rc;
    rc = (int)dspp.download(blk_spp_out);
    if (!rc) rc = (int)dkeep.download(keep_out);
    return rc ? rc : (int)dnoise.download(noise_out);
}

}  // extern "C"
