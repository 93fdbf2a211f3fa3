// pt_feature_walk.h -- the first-hit feature sums of a BVH scene (pt_set_feature_walk), the tree walked by the WAVE.
//
// feature_kernel (pt_kernels.h) finds a feature sample's first hit by the linear scan of pta::first_hit, which is why features are
// refused on the BVH path.  Its waves are the population primary_bvh_kernel (pt_primary.h) was written for: one lane per slot makes a
// wave one 8 x 8 block, and sample s of the block is the 64 consecutive jobs at (cblk * S + s) * 64 -- 64 rays from (nearly) one point
// through (nearly) one direction.  feature_bvh_kernel keeps feature_body's bookkeeping (chunk_slot, first, take, the nine running sums,
// the id of global sample 0, no atomics on the sums) and finds each sample's (best, t) by that kernel's walk, wave_first_hit
// (pt_wave_walk.h): one LDS stack per wave, nodes by scalar loads, FP32 slab tests with the node as scalar operands, ballot descent
// nearest first, the exact FP64 tests and `wins` on pierced object slots, per-lane tmax culling -- the sequential loop's winner, bit
// for bit.  Glass objects are ordinary candidates: a feature sample has no exit search.  A wave that holds an odd ray (the same
// classification, wave_walk_coop) takes the plain loop, scan_uniform, for that sample.  pta::hit_record turns (best, t) into the record,
// as it does for first_hit.  (profiles/wave_walk_kernel_regs.txt.)
#pragma once

#include "pt_wave_walk.h"

namespace ptk {

struct FeatureWalkArgs {
    FeatureArgs A;
    DevFrame F;                       // bvh_root, n_plane, planes_y, clip_bound, origin_bound, nobj
    const BvhNode *bvh_nodes;
    const BvhObj *bvh_objs;
    const int32_t *plane_idx;
    unsigned long long *stats;        // [4]: (wave, sample) pairs walked, ... sent to the plain scan, node visits, the deepest stack
};

template <bool ADAPT>
__device__ __forceinline__ void feature_walk_body(const FeatureWalkArgs &W, const AdaptTable &T, int *const wst) {
    const FeatureArgs &A = W.A;
    const DevFrame &F = W.F;
    typedef const BvhNode __attribute__((address_space(4))) *ConstNodePtr;
    typedef const BvhObj __attribute__((address_space(4))) *ConstBObjPtr;
    typedef const DevObj __attribute__((address_space(4))) *ConstObjPtr;
    typedef const int32_t __attribute__((address_space(4))) *ConstIdxPtr;
    const ConstNodePtr nodes = (ConstNodePtr)W.bvh_nodes;
    const ConstBObjPtr bobjs = (ConstBObjPtr)W.bvh_objs;
    const ConstObjPtr g_obj = (ConstObjPtr)A.objs;
    const ConstIdxPtr g_pl = (ConstIdxPtr)W.plane_idx;
    uint32_t slot, cblk;
    if (!chunk_slot<ADAPT>(T, A.nslots, slot, cblk)) return;  // (whole waves: the slots come in blocks of 64)
    const uint32_t p = slot & 63u;
    const size_t base = (size_t)cblk * A.S * 64u + p;
    const bool have = A.ray_ndraw[base] != 0xffffu;  // outside the frame (the same for every sample of the slot): the lane stays, idle
    const uint64_t hm = __ballot(have);
    if (hm == 0) return;  // a block with no pixel inside the frame (wave-uniform)
    const int lead = __ffsll((long long)hm) - 1;  // a lane that takes part in every walk: the walk's counts are read from it
    double f[9];
    for (uint32_t q = 0; q < 9u; q++) f[q] = (A.first || !have) ? 0.0 : A.feat[q * (size_t)A.nslots + slot];
    const size_t nj = A.njobs;
    uint32_t c_walked = 0, c_plain = 0;  // wave-uniform
    uint32_t c_visits = 0, c_deep = 0;   // the same in every lane that has a pixel
    for (uint32_t s = 0; s < A.take; s++) {
        const size_t job = base + (size_t)s * 64u;
        const double ox = A.ray[job], oy = A.ray[nj + job], oz = A.ray[2 * nj + job];
        const double dx = A.ray[3 * nj + job], dy = A.ray[4 * nj + job], dz = A.ray[5 * nj + job];
        // ------------------------------------------------------------ the wave's walk (pt_wave_walk.h), or the plain loop for an odd wave
        const double a = dx * dx + dy * dy + dz * dz;
        const RayD r{ox, oy, oz, dx, dy, dz};
        const bool coop = wave_walk_coop(F, have, r, a);
        if (coop) c_walked++;
        else c_plain++;
        int best = -1;
        double tmax = ptm::max_float64();
        if (coop && have) {
            wave_first_hit<true>(F, nodes, bobjs, g_obj, g_pl, ox, oy, oz, dx, dy, dz, a, wst, best, tmax, c_visits, c_deep);
        } else if (have) {
            scan_uniform(F, g_obj, r, 0, best, tmax);  // the plain loop, every lane on the same object
        }
        // ------------------------------------------------------------ (best, tmax) -> the record, as feature_body
        if (have) {
            if (A.ids && A.first && s == 0u) A.ids[slot] = best;  // the chunk that starts the sums holds global sample 0
            if (best >= 0) {
                const double o[3] = {ox, oy, oz}, d[3] = {dx, dy, dz};
                double n[3], al[3], dist;
                pta::hit_record(A.objs, A.mats, best, tmax, o, d, n, al, dist);
                f[0] += n[0]; f[1] += n[1]; f[2] += n[2];
                f[3] += al[0]; f[4] += al[1]; f[5] += al[2];
                f[6] += dist;
                f[7] += 1.0;
            }
            f[8] += 1.0;
        }
    }
    if (have)
        for (uint32_t q = 0; q < 9u; q++) A.feat[q * (size_t)A.nslots + slot] = f[q];
    // once per wave: what it walked (the counts of the walk itself from a lane that took part in it)
    const uint32_t visits = (uint32_t)__builtin_amdgcn_readlane((int)c_visits, lead);
    const uint32_t deep = (uint32_t)__builtin_amdgcn_readlane((int)c_deep, lead);
    if ((threadIdx.x & (PT_WAVE - 1)) == 0u) {
        if (c_walked) atomicAdd(W.stats + 0, (unsigned long long)c_walked);
        if (c_plain) atomicAdd(W.stats + 1, (unsigned long long)c_plain);
        if (visits) atomicAdd(W.stats + 2, (unsigned long long)visits);
        if (deep) atomicMax(W.stats + 3, (unsigned long long)deep);
    }
}

__global__ __launch_bounds__(PT_BLOCK) void feature_bvh_kernel(const FeatureWalkArgs W) {
    __shared__ int wstack[PT_BLOCK / PT_WAVE][PT_BVH_STACK];
    feature_walk_body<false>(W, AdaptTable{nullptr, 0u}, wstack[threadIdx.x >> 6]);
}

__global__ __launch_bounds__(PT_BLOCK) void feature_bvh_adaptive_kernel(const FeatureWalkArgs W, const AdaptTable T) {
    __shared__ int wstack[PT_BLOCK / PT_WAVE][PT_BVH_STACK];
    feature_walk_body<true>(W, T, wstack[threadIdx.x >> 6]);
}

}  // namespace ptk
