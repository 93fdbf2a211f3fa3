// pt_feature_walk.h -- the first-hit feature sums of a BVH scene (pt_set_feature_walk), the tree walked by the WAVE.
//
// feature_kernel (pt_kernels.h) finds a feature sample's first hit by the linear scan of pta::first_hit, which is why features are
// refused on the BVH path.  Its waves are the population primary_bvh_kernel (pt_primary.h) was written for: one lane per slot makes a
// wave one 8 x 8 block, and sample s of the block is the 64 consecutive jobs at (cblk * S + s) * 64 -- 64 rays from (nearly) one point
// through (nearly) one direction.  feature_bvh_kernel keeps feature_body's bookkeeping (chunk_slot, first, take, the nine running sums,
// the id of global sample 0, no atomics on the sums) and finds each sample's (best, t) by that kernel's walk: one LDS stack per wave,
// nodes by scalar loads, FP32 slab tests with the node as scalar operands, ballot descent nearest first, the exact FP64 tests and
// `wins` on pierced object slots, per-lane tmax culling -- the sequential loop's winner, bit for bit.  Glass objects are ordinary
// candidates: a feature sample has no exit search.  A wave that holds an odd ray (primary_bvh_kernel's classification) takes the plain
// loop, scan_uniform, for that sample.  pta::hit_record turns (best, t) into the record, as it does for first_hit.
//
// The walk below is a second copy of primary_bvh_kernel's: that kernel sits at its register limit and its body stays as it is
// (profiles/feature_bvh_kernel_regs.txt).
#pragma once

#include "pt_kernels.h"

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
    const double tmin = 0.001;  // renderer.go:292
    uint32_t c_walked = 0, c_plain = 0;  // wave-uniform
    uint32_t c_visits = 0, c_deep = 0;   // the same in every lane that has a pixel
    for (uint32_t s = 0; s < A.take; s++) {
        const size_t job = base + (size_t)s * 64u;
        const double ox = A.ray[job], oy = A.ray[nj + job], oz = A.ray[2 * nj + job];
        const double dx = A.ray[3 * nj + job], dy = A.ray[4 * nj + job], dz = A.ray[5 * nj + job];
        // ------------------------------------------------------------ is this a wave for the shared walk?  (as primary_bvh_kernel)
        const RayD r{ox, oy, oz, dx, dy, dz};
        const double a = dx * dx + dy * dy + dz * dz;
        const double Cb = F.clip_bound;
        const bool tame = (a >= 1e-100) && (a <= 1e100) && (ptm::f_abs(ox) <= Cb) && (ptm::f_abs(oy) <= Cb) && (ptm::f_abs(oz) <= Cb);
        const Clip noclip{0.0, 0.0, 0.0, false, false};
        const bool odd = have && !(tame && bvh_ray_trusted(F, r, noclip, a));
        const bool coop = __ballot(odd) == 0;
        if (coop) c_walked++;
        else c_plain++;
        int best = -1;
        double tmax = ptm::max_float64();
        if (coop && have) {
            bool best_is_box = false;
            // ---- planes: infinite, always tested exactly
            for (int k = 0; k < F.n_plane; k++) {
                const int i = g_pl[k];
                const auto &o = g_obj[i];
                double t = 0;
                if (F.planes_y ? plane_exact_y(o.a[1], r, tmin, tmax, t)
                               : plane_exact(o.a[0], o.a[1], o.a[2], o.b[0], o.b[1], o.b[2], r, tmin, tmax, t)) {
                    if (wins(0, false, i, t, best, best_is_box, tmax)) {
                        best = i;
                        tmax = t;
                        best_is_box = false;
                    }
                }
            }
            if (F.bvh_root >= 0) {
                const double ya = div_recip(a);
                const double ivx = 1 / dx, ivy = 1 / dy, ivz = 1 / dz;  // objects.go:149,154,159
                // FP32 quantities of the node tests (ts = 0: the ray starts inside the clip bound)
                const float fox = (float)ox, foy = (float)oy, foz = (float)oz;
                const float fdx = (float)dx, fdy = (float)dy, fdz = (float)dz;
                float tminf = (float)tmin;
                tminf -= __builtin_fabsf(tminf) * 1e-2f + 1e-6f;
                tminf = __builtin_fmaxf(tminf, 0.0f);
                const float ivxf = __builtin_amdgcn_rcpf(slab_dir(fdx, F.dir_floor)), ivyf = __builtin_amdgcn_rcpf(slab_dir(fdy, F.dir_floor)),
                            ivzf = __builtin_amdgcn_rcpf(slab_dir(fdz, F.dir_floor));
                const float aivxf = __builtin_fabsf(ivxf), aivyf = __builtin_fabsf(ivyf), aivzf = __builtin_fabsf(ivzf);
                const float noxf = -fox * ivxf, noyf = -foy * ivyf, nozf = -foz * ivzf;
                float tmaxf = (float)tmax;
                tmaxf += __builtin_fabsf(tmaxf) * 4.8e-7f;  // >= tmax (MaxFloat64 becomes +inf)
                int sp = 0;
                int cur = F.bvh_root;
                while (cur >= 0) {
                    c_visits++;
                    const auto &nd_ = nodes[cur];  // wave-uniform: scalar loads
                    const uint32_t meta = nd_.meta;
                    const int nbase = nd_.node_base, obase = nd_.obj_base;
                    uint32_t key[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
#pragma unroll
                    for (int c = 0; c < 4; c++) {
                        const bool is_node = (meta >> (8 + c)) & 1u, is_obj = (meta >> (12 + c)) & 1u;
                        if (!(is_node || is_obj)) continue;  // empty slot (wave-uniform)
                        const float tcx = __builtin_fmaf(nd_.c[0][c], ivxf, noxf), tcy = __builtin_fmaf(nd_.c[1][c], ivyf, noyf),
                                    tcz = __builtin_fmaf(nd_.c[2][c], ivzf, nozf);
                        const float t0 = pt_vmax3(__builtin_fmaf(-nd_.h[0][c], aivxf, tcx), __builtin_fmaf(-nd_.h[1][c], aivyf, tcy),
                                                  pt_vmax(__builtin_fmaf(-nd_.h[2][c], aivzf, tcz), tminf));
                        const float t1 = pt_vmin3(__builtin_fmaf(nd_.h[0][c], aivxf, tcx), __builtin_fmaf(nd_.h[1][c], aivyf, tcy),
                                                  pt_vmin(__builtin_fmaf(nd_.h[2][c], aivzf, tcz), tmaxf));
                        const bool pierced = !(t1 < t0);  // NaN slabs constrain nothing, like the per-lane walk
                        const uint64_t pm = __ballot(pierced);
                        if (pm == 0) continue;
                        if (is_node) {
                            // entry parameter of the first lane that pierces the slot (>= 0: its bits order like the value), slot in the low bits
                            const int src = __ffsll((long long)pm) - 1;
                            const uint32_t bits = (uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(t0), src);
                            key[c] = (bits & ~3u) | (uint32_t)c;
                        } else if (pierced) {
                            // the slot's object, for every lane whose own slab test passed: the reference's exact test
                            const auto &bo = bobjs[obase + (int)((meta >> (2 * c)) & 3u)];
                            const int i = bo.index;
                            const bool is_box = (bo.o.kind & 0xff) == KIND_BOX;  // wave-uniform
                            double t = 0;
                            bool valid;
                            if (is_box)
                                valid = box_exact<true>(bo.o.a[0], bo.o.a[1], bo.o.a[2], bo.o.b[0], bo.o.b[1], bo.o.b[2], r, ivx, ivy, ivz, tmin,
                                                        ptm::max_float64(), t);
                            else
                                valid = sphere_exact_shared<false>(bo.o.a[0], bo.o.a[1], bo.o.a[2], bo.o.radius_sq, r, a, ya, tmin, tmax, t);
                            if (valid && wins(0, is_box, i, t, best, best_is_box, tmax)) {
                                best = i;
                                tmax = t;
                                best_is_box = is_box;
                                tmaxf = (float)tmax;
                                tmaxf += __builtin_fabsf(tmaxf) * 4.8e-7f;
                            }
                        }
                    }
                    // internal children nearest first (wave-uniform keys: scalar unit); 0xffffffff = not a candidate
                    uint32_t k0, k1, k2, k3;
                    {
                        const uint32_t a0 = key[0] < key[1] ? key[0] : key[1], a1 = key[0] < key[1] ? key[1] : key[0];
                        const uint32_t a2 = key[2] < key[3] ? key[2] : key[3], a3 = key[2] < key[3] ? key[3] : key[2];
                        k0 = a0 < a2 ? a0 : a2;
                        const uint32_t m0 = a0 < a2 ? a2 : a0;
                        k3 = a1 < a3 ? a3 : a1;
                        const uint32_t m1 = a1 < a3 ? a1 : a3;
                        k1 = m0 < m1 ? m0 : m1;
                        k2 = m0 < m1 ? m1 : m0;
                    }
#define PT_CHILD(k) (nbase + (int)((meta >> (2u * ((k) & 3u))) & 3u))
                    if (k1 != 0xffffffffu) {
                        if (k2 != 0xffffffffu) {
                            if (k3 != 0xffffffffu) { wst[sp] = PT_CHILD(k3); sp++; }
                            wst[sp] = PT_CHILD(k2);
                            sp++;
                        }
                        wst[sp] = PT_CHILD(k1);
                        sp++;
                        if ((uint32_t)sp > c_deep) c_deep = (uint32_t)sp;
                    }
                    if (k0 != 0xffffffffu) {
                        cur = PT_CHILD(k0);
                    } else if (sp > 0) {
                        sp--;
                        cur = __builtin_amdgcn_readfirstlane(wst[sp]);
                    } else {
                        cur = -1;
                    }
#undef PT_CHILD
                }
            }
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
