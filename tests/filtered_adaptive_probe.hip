// filtered_adaptive_probe.hip -- test-only: the three kernels of pt_set_adaptive_filtered's check (csrc/pt_kernels.h) on
// the gfx950 device, on planes no rendered frame gives and on active lists of any length.
//
// pt_filter_launch.h and pt_kernels.h are included unchanged and compiled with the library's own flags
// (tests/filtered_adaptive_probe_support.py), and the launches are the product's own sequences (ptl::block_map_sequence,
// ptl::keep_sequence), so what runs here is the code libptcore.so ships.  Each extern "C" entry point uploads its host arrays, runs
// the sequence, copies the results back and returns the first HIP status that was not hipSuccess (0 = fine; a negative value: the
// arguments were refused before anything was launched).  Every output buffer has its full size and is filled with 0xFF bytes before
// the launch, so what a kernel did not write reads 0xFFFFFFFF, 0xFF or a NaN.  No inline assembly.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "probe_common.h"
#include "pt_filter_launch.h"
#include "pt_kernels.h"

extern "C" {

// block_err_kernel and block_pool_kernel on a W x H frame: mean [npix][3], err and bad [npix]; s, pooled, own (doubles), k (uint32)
// and stop (bytes) over the grid of ((W + 7) / 8) x ((H + 7) / 8) blocks.
int probe_block_map(const double *mean, const double *err, const double *bad, int32_t W, int32_t H, int32_t pool, double target, double *s_out,
                    uint32_t *k_out, double *pooled_out, double *own_out, uint8_t *stop_out) {
    if (W <= 0 || H <= 0 || (int64_t)W * H > (int64_t)1 << 26 || pool < 0 || pool > PTA_MAX_POOL) return -1;
    const size_t npix = (size_t)W * (size_t)H, nb = (size_t)ptl::blocks_across(W) * (size_t)ptl::blocks_across(H);
    Buf<double> dmean(mean, 3 * npix), derr(err, npix), dbad(bad, npix), ds(nullptr, nb), dpooled(nullptr, nb), down(nullptr, nb);
    Buf<uint32_t> dk(nullptr, nb);
    Buf<uint8_t> dstop(nullptr, nb);
    hipError_t st = hipSuccess;
    for (hipError_t e : {dmean.st, derr.st, dbad.st, ds.st, dpooled.st, down.st, dk.st, dstop.st}) PROBE_TRY(e);
    if (st != hipSuccess) return (int)st;
    ptl::block_map_sequence(dmean.d, derr.d, dbad.d, ptl::BlockMap{ds.d, dk.d, dpooled.d, down.d, dstop.d}, W, H, pool, target, 0);
    int rc = finish(st);
    if (rc) return rc;
    rc = (int)ds.download(s_out);
    if (!rc) rc = (int)dk.download(k_out);
    if (!rc) rc = (int)dpooled.download(pooled_out);
    if (!rc) rc = (int)down.download(own_out);
    return rc ? rc : (int)dstop.download(stop_out);
}

// keep_from_map_kernel and, behind its keep[], compact_kernel, on a shard of nslots slots (a multiple of 1024: whole tiles) with
// nact >= 1 active blocks, each below nslots / 64 and with its first pixel inside the frame.  pooled, stop: the map over the frame's
// grid, or both null (the counts are stamped, nothing is decided).  geom = {width, height, ntx, shard_index, shard_count} (TileGeom).
// blk_spp_out [nslots / 64] (the blocks that are not in the list stay 0xFFFFFFFF); keep_out, noise_out, next_out [nact];
// res_out: one ptk::AdaptResult (16 bytes).
int probe_keep_from_map(const uint32_t *active, int64_t nact, int64_t nslots, const double *pooled, const uint8_t *stop, int32_t n,
                        const int32_t *geom, uint32_t *blk_spp_out, uint32_t *keep_out, double *noise_out, uint32_t *next_out, void *res_out) {
    if (nslots <= 0 || nslots % 1024 != 0 || nslots > (int64_t)1 << 30 || nact <= 0 || nact > nslots / 64) return -1;
    if ((pooled == nullptr) != (stop == nullptr)) return -1;
    for (int k = 0; k < 5; k++)
        if (geom[k] < (k == 3 ? 0 : 1)) return -3;
    if (geom[3] >= geom[4] || geom[2] != (geom[0] + 31) / 32) return -3;
    const int32_t nbx = ptl::blocks_across(geom[0]), nby = ptl::blocks_across(geom[1]);
    const int64_t ntiles = (int64_t)geom[2] * ((geom[1] + 31) / 32);
    for (int64_t i = 0; i < nact; i++) {  // the kernel would write blk_spp, or read the map, out of bounds
        if (active[i] >= (uint64_t)(nslots / 64)) return -2;
        if ((int64_t)geom[3] + (int64_t)(active[i] >> 4) * geom[4] >= ntiles) return -2;
    }
    const size_t ns = (size_t)nslots, na = (size_t)nact, nb = (size_t)nbx * (size_t)nby;
    Buf<uint32_t> dact(active, na), dspp(nullptr, ns / 64), dkeep(nullptr, na), dnext(nullptr, na);
    Buf<double> dpooled(pooled, pooled ? nb : 0), dnoise(nullptr, na);
    Buf<uint8_t> dstop(stop, stop ? nb : 0);
    Buf<ptk::AdaptResult> dres(nullptr, 1);
    hipError_t st = hipSuccess;
    for (hipError_t e : {dact.st, dspp.st, dkeep.st, dnext.st, dpooled.st, dnoise.st, dstop.st, dres.st}) PROBE_TRY(e);
    if (st != hipSuccess) return (int)st;
    ptk::KeepFromMapArgs A = {};
    A.active = dact.d;
    A.pooled = pooled ? dpooled.d : nullptr;
    A.stop = stop ? dstop.d : nullptr;
    A.blk_spp = dspp.d;
    A.keep = dkeep.d;
    A.noise = dnoise.d;
    A.nact = (uint32_t)nact;
    A.n = n;
    A.nbx = nbx;
    A.nby = nby;
    A.G.width = geom[0];
    A.G.height = geom[1];
    A.G.ntx = geom[2];
    A.G.shard_index = geom[3];
    A.G.shard_count = geom[4];
    ptk::CompactArgs K = {};
    K.active = dact.d;
    K.keep = dkeep.d;
    K.noise = dnoise.d;
    K.next = dnext.d;
    K.res = dres.d;
    K.nact = (uint32_t)nact;
    ptl::keep_sequence(A, &K, 0);
    int rc = finish(st);
    if (rc) return rc;
    rc = (int)dspp.download(blk_spp_out);
    if (!rc) rc = (int)dkeep.download(keep_out);
    if (!rc) rc = (int)dnoise.download(noise_out);
    if (!rc) rc = (int)dnext.download(next_out);
    return rc ? rc : (int)dres.download(static_cast<ptk::AdaptResult *>(res_out));
}

}  // extern "C"
