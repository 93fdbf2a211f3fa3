// pt_primary.h -- the first segment of every path of a BVH scene, traversed by the WAVE instead of by the lane (round 4).
//
// The primary rays of a pass are a population the wave can walk the tree for: 64 consecutive jobs are one sample of one 8 x 8 pixel
// block (pt_device.h), i.e. 64 rays from (nearly) one point through (nearly) one direction.  primary_bvh_kernel finds their first
// hits with ONE stack per wave, by wave_first_hit (pt_wave_walk.h, which says how and why the result is the sequential loop's
// winner, bit for bit; `verify_bvh` checks it).
//
// The kernel then shades the hit (renderer.go:304-403: sky, emitted, scatter, roulette) with the code the trace loop uses
// and appends the paths that go on to the continuation queue (the split passes' PathQueue, windows of PT_CONT_BLOCK slots per
// atomic), from which trace_kernel<.., SCAN_BVH, ..> takes them like fresh jobs; paths that end write their radiance record.
// Whatever this kernel is not meant for goes to the queue UNSHADED, as the primary ray itself at full depth, and trace_kernel
// does what it always did: a wave that holds a ray with non-finite or absurd components, one that starts outside 3.5 scene
// sizes (clip / far-origin logic of clip_ray) or outside the range the FP32 bounds were analysed for; and dielectric hits
// (their exit search walks the second tree; one object in ten of the synthetic scenes).
#pragma once

#include "pt_wave_walk.h"

namespace ptk {

#ifndef PT_PRIMARY_WAVES
#define PT_PRIMARY_WAVES 6  // blocks of 256 threads per CU the kernel is compiled for (84 VGPRs)
#endif

template <bool STATS, bool VERIFY>
__global__ __launch_bounds__(PT_BLOCK, PT_PRIMARY_WAVES) void primary_bvh_kernel(const TraceArgs A) {
    __shared__ int wstack[PT_BLOCK / PT_WAVE][PT_BVH_STACK];
    const DevFrame &F = A.F;
    const TraceBuffers &B = A.B;
    typedef const BvhNode __attribute__((address_space(4))) *ConstNodePtr;
    typedef const BvhObj __attribute__((address_space(4))) *ConstBObjPtr;
    typedef const DevObj __attribute__((address_space(4))) *ConstObjPtr;
    typedef const int32_t __attribute__((address_space(4))) *ConstIdxPtr;
    const ConstNodePtr nodes = (ConstNodePtr)B.bvh_nodes;
    const ConstBObjPtr bobjs = (ConstBObjPtr)B.bvh_objs;
    const ConstObjPtr g_obj = (ConstObjPtr)B.objs;
    const ConstIdxPtr g_pl = (ConstIdxPtr)B.plane_idx;
    const uint32_t lane = threadIdx.x & (PT_WAVE - 1);
    int *const wst = wstack[threadIdx.x >> 6];
    const uint32_t wave0 = (blockIdx.x * PT_BLOCK + threadIdx.x) >> 6, nwaves = (gridDim.x * PT_BLOCK) >> 6;
    const size_t nj = F.njobs, qc = B.cont.cap;
    uint32_t q_cur = 0, q_end = 0;  // this wave's window of continuation slots (one atomic per PT_CONT_BLOCK slots, see trace_kernel)
    uint32_t c_seg = 0, c_draw = 0, c_samples = 0, c_mismatch = 0, c_cont = 0;
    uint32_t c_visits = 0, c_coop = 0, c_odd = 0;  // wave-uniform (diagnostics)

    for (uint32_t wj = wave0; (size_t)wj * PT_WAVE < nj; wj += nwaves) {  // njobs is a multiple of 64: a wave's jobs all exist
        const uint32_t job = wj * PT_WAVE + lane;
        const uint32_t nd = B.ray_ndraw[job];
        const bool have = nd != 0xffffu;  // 0xffff: the job's pixel lies outside the frame (edge tile)
        double ox = B.ray[job], oy = B.ray[nj + job], oz = B.ray[2 * nj + job];
        double dx = B.ray[3 * nj + job], dy = B.ray[4 * nj + job], dz = B.ray[5 * nj + job];
        uint64_t rs = B.ray_rng[job];
        uint32_t j_seg = 0, j_draw = nd;
        if (have) { c_samples++; c_draw += nd; }
        if (F.max_depth <= 0) {  // rayColorOpt returns black before any scan (renderer.go:287-289); the camera draws happened
            if (have) store_path_end<STATS>(&B, job, 0.0, 0.0, 0.0, 0u, nd);
            continue;
        }
        // ------------------------------------------------------------ the wave's walk (pt_wave_walk.h), or none for an odd wave
        const double a = dx * dx + dy * dy + dz * dz;
        const RayD r{ox, oy, oz, dx, dy, dz};
        const bool coop = wave_walk_coop(F, have, r, a);
        if (coop) c_coop++;
        else c_odd++;
        int best = -1;
        double tmax = ptm::max_float64();
        if (coop && have) {
            uint32_t no_deep = 0;
            wave_first_hit<false>(F, nodes, bobjs, g_obj, g_pl, ox, oy, oz, dx, dy, dz, a, wst, best, tmax, c_visits, no_deep);
            if (VERIFY) {
                int best2;
                double tmax2;
                scan_uniform(F, g_obj, r, 0, best2, tmax2);
                if (best != best2 || (best >= 0 && !(tmax == tmax2))) c_mismatch++;
                best = best2;
                tmax = tmax2;
            }
        }
        // ------------------------------------------------------------ shade (renderer.go:304-403), or hand the ray over unshaded
        bool go_on = false;
        int depth = F.max_depth;
        double Tx = 1, Ty = 1, Tz = 1;
        if (have) {
            const bool hit_glass = coop && best >= 0 && (B.objs[best].kind & 0x100);
            if (!coop || hit_glass) {
                go_on = true;  // the primary ray itself, at full depth: trace_kernel scans and shades it
            } else {
                c_seg++;
                j_seg = 1;
                bool finished = false;
                double termx = 0, termy = 0, termz = 0;
                if (best < 0) {
                    finished = true;
                    sky_radiance(&A.sky, dx, dy, dz, termx, termy, termz);
                } else {
                    double attx = 1, atty = 1, attz = 1;
                    bool exit_search = false;
                    int exit_mat = 0;
                    uint32_t jd = j_draw;
                    shade_hit<true, false>(B.objs[best], B.mats, tmax, ox, oy, oz, dx, dy, dz, rs, c_draw, jd, finished, termx, termy, termz, attx,
                                           atty, attz, exit_search, exit_mat);
                    // (no dielectric is shaded here: the material's own record, from memory like the material)
                    if (!finished) finished = roulette_table_advance<true>(depth, B.roulette[B.objs[best].mat], attx, atty, attz, Tx, Ty, Tz, rs, c_draw, jd);
                    j_draw = jd;
                }
                if (finished) store_path_end<STATS>(&B, job, Tx * termx, Ty * termy, Tz * termz, j_seg, j_draw);
                else go_on = true;
            }
        }
        // ------------------------------------------------------------ survivors -> continuation queue (as glass_kernel does)
        // (hand-written, by slot: through window_reserve / queue_store of pt_kernels.h the STATS and VERIFY forms of this kernel, which sits at its 80
        // VGPRs with 55 - 71 spilled SGPRs, spill 2 - 6 VGPRs to scratch: profiles/core_dedupe_kernel_regs.txt)
        const uint64_t pm = __ballot(go_on);
        if (pm != 0) {
            const uint32_t np = (uint32_t)__popcll(pm), room = q_end - q_cur;
            uint32_t nbase = 0;
            if (np > room) {
                if (lane == 0) nbase = atomicAdd(B.cont.count, (uint32_t)PT_CONT_BLOCK);
                nbase = __builtin_amdgcn_readfirstlane(nbase);
            }
            const uint32_t rank = lane_rank(pm);
            const uint32_t slot = rank < room ? q_cur + rank : nbase + (rank - room);
            if (np > room) {
                q_cur = nbase + (np - room);
                q_end = nbase + PT_CONT_BLOCK;
            } else {
                q_cur += np;
            }
            if (go_on && slot >= B.cont.cap) {
                atomicAdd(B.counters + 19, 1ull);  // cannot happen (the queue holds every job plus every window); never write outside it
            } else if (go_on) {
                B.cont.d[slot] = ox;
                B.cont.d[qc + slot] = oy;
                B.cont.d[2 * qc + slot] = oz;
                B.cont.d[3 * qc + slot] = dx;
                B.cont.d[4 * qc + slot] = dy;
                B.cont.d[5 * qc + slot] = dz;
                B.cont.d[6 * qc + slot] = Tx;
                B.cont.d[7 * qc + slot] = Ty;
                B.cont.d[8 * qc + slot] = Tz;
                B.cont.rs[slot] = rs;
                B.cont.job[slot] = job;
                B.cont.depth[slot] = depth;
                if (STATS) { B.cont.jseg[slot] = j_seg; B.cont.jdraw[slot] = j_draw; }
                c_cont++;
            }
        }
    }
    for (uint32_t s = q_cur + lane; s < q_end && s < B.cont.cap; s += PT_WAVE) B.cont.job[s] = PT_HOLE;  // the rest of the window stays empty
    flush_count(&B.counters[0], c_seg, lane);
    flush_count(&B.counters[2], c_draw, lane);
    flush_count(&B.counters[3], c_samples, lane);
    flush_count(&B.counters[6], c_cont, lane);
    if (lane == 0) {
        if (c_visits) atomicAdd(&B.counters[40], (unsigned long long)c_visits);  // wave-level node visits (diagnostics)
        if (c_coop) atomicAdd(&B.counters[41], (unsigned long long)c_coop);      // blocks of 64 jobs walked by the wave
        if (c_odd) atomicAdd(&B.counters[42], (unsigned long long)c_odd);        // ... handed over unshaded
    }
    if (VERIFY) flush_count(&B.counters[4], c_mismatch, lane);
}

}  // namespace ptk
