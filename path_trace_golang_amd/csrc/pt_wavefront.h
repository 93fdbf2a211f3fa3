// pt_wavefront.h -- the wavefront form of the render loop (included by ptcore.hip after pt_kernels.h).
//
// Every path of a chunk lives in a path-state queue in HBM (PathQueue, pt_device.h) and the loop of
// rayColorOpt (renderer.go:286-404) is cut into passes over those queues, one level of the recursion at a time:
//
//   wf_init_kernel       fresh jobs (primary rays of raygen_kernel) -> queue A
//   per level:
//     wf_traverse_kernel<0>  closest hit of every path in A        (renderer.go:297-302)
//     wf_shade_kernel        sky / emitted / scatter / roulette       (renderer.go:303-319, :375-403): paths that go on
//                            are appended to queue B, dielectric front-face hits to the exit queue E
//     wf_traverse_kernel<1>  exit search of every path in E        (renderer.go:321-349)
//     wf_exit_kernel         Beer-Lambert + origin move + roulette    (renderer.go:352-403): survivors -> B
//     (optional) wf_bin_*    B is reordered by direction octant and cell of the origin, so that a wave's 64 rays walk
//                            the hierarchy together
//     A <-> B
//
// Why: in the all-in-one loop a wave does one scan per trip for all its lanes and then shades; in a scene with 10^5
// objects the traversals of one wave differ by an order of magnitude in length, and the wave waits for its longest
// (20 % of lanes busy, profiles/r01_n3_summary.json).  Here a lane that has finished its traversal writes the hit
// and takes the next ray of the queue at once (ballot + mbcnt refill, as for jobs in trace_kernel), so the walk loop
// always runs on full waves, and shading runs as its own pass at one path per lane.
// The price is HBM traffic: 48 B in + 12 B out per traversal, 100 B in + up to 100 B out per shaded path.
#pragma once

#include "pt_kernels.h"

namespace ptk {

struct WfArgs {
    DevFrame F;
    DevSky sky;
    TraceBuffers B;
    PathQueue qin;    // paths of this level
    PathQueue qout;   // paths that go on to the next level
    PathQueue qexit;  // exit searches of this level
    unsigned int *cursor;  // item cursor of the running traversal pass
    // ray sorting (optional): the traversal pass takes its rays in the order of `perm`, which lists the entries of qin by
    // direction octant and cell of the origin (counting sort: wf_bin_count / wf_bin_scan / wf_bin_scatter)
    const uint32_t *perm;      // [n_sorted] entry indices, or null: queue order
    const uint32_t *n_sorted;  // number of entries in perm (holes are left out)
    uint32_t *bin_count;       // [PT_WF_BINS + 1] histogram, then exclusive offsets
    uint32_t *bin_key;         // [cap] key of every entry (PT_HOLE for a hole)
};

#define PT_WF_GRID 8u                                        // cells per axis over the scene cube
#define PT_WF_BINS (8u * PT_WF_GRID * PT_WF_GRID * PT_WF_GRID)  // direction octant x cell = 4096

// 3-bit Morton interleave of a cell coordinate
__device__ __forceinline__ uint32_t wf_spread3(uint32_t v) {
    v &= 7u;
    return (v & 1u) | ((v & 2u) << 2) | ((v & 4u) << 4);
}
// direction octant (3 bits, high) and Morton cell of the origin inside the scene cube (9 bits): rays of one bin start
// in the same eighth of each axis and head the same way, so they meet the same upper nodes of the hierarchy
__device__ __forceinline__ uint32_t wf_ray_key(const DevFrame &F, double ox, double oy, double oz, double dx, double dy, double dz) {
    const float inv = (float)(0.5 * PT_WF_GRID) / (float)F.scene_bound;
    const float half = 0.5f * PT_WF_GRID;
    const float fx = __builtin_fminf(__builtin_fmaxf(__builtin_fmaf((float)ox, inv, half), 0.0f), (float)(PT_WF_GRID - 1u));
    const float fy = __builtin_fminf(__builtin_fmaxf(__builtin_fmaf((float)oy, inv, half), 0.0f), (float)(PT_WF_GRID - 1u));
    const float fz = __builtin_fminf(__builtin_fmaxf(__builtin_fmaf((float)oz, inv, half), 0.0f), (float)(PT_WF_GRID - 1u));
    const uint32_t cell = wf_spread3((uint32_t)fx) | (wf_spread3((uint32_t)fy) << 1) | (wf_spread3((uint32_t)fz) << 2);
    const uint32_t oct = (dx < 0 ? 1u : 0u) | (dy < 0 ? 2u : 0u) | (dz < 0 ? 4u : 0u);
    return (oct << 9) | cell;
}

// The pieces every pass below shares.
// Number of entries a pass walks: what the writers counted, never more than the queue holds.
__device__ __forceinline__ uint32_t queue_len(const PathQueue &q) {
    typedef const uint32_t __attribute__((address_space(4))) *ConstU32Ptr;
    const uint32_t n_count = *(ConstU32Ptr)(q.count);
    return n_count < q.cap ? n_count : q.cap;
}
// (The staging copies, the queue window and entry store, flush_count, record_mismatch and store_path_end are pt_kernels.h's.)

// The mirror of queue_store for one entry by its index, in the two parts a pass reads it in: the ray, which finds (or is all that is needed to find) the entry's
// answer, and then the path state -- throughput, stream state, depth, the optional counts.  (The job id comes first: it tells a hole.)
__device__ __forceinline__ RayD queue_load_ray(const PathQueue &q, uint32_t i) {
    const size_t qc = q.cap;
    return RayD{q.d[i], q.d[qc + i], q.d[2 * qc + i], q.d[3 * qc + i], q.d[4 * qc + i], q.d[5 * qc + i]};
}
__device__ __forceinline__ void queue_load_state(const PathQueue &q, uint32_t i, double &Tx, double &Ty, double &Tz, uint64_t &rs, int &depth,
                                                 uint32_t &j_seg, uint32_t &j_draw, bool stats) {
    const size_t qc = q.cap;
    Tx = q.d[6 * qc + i]; Ty = q.d[7 * qc + i]; Tz = q.d[8 * qc + i];
    rs = q.rs[i];
    depth = q.depth[i];
    if (stats) { j_seg = q.jseg[i]; j_draw = q.jdraw[i]; }
}

// Counting sort of the entries of A.qin by key.  Every block owns one contiguous slice of the queue in passes 1 and 3
// and keeps its histogram in LDS, so the global counters see one atomic per block and bin instead of one per ray
// (a single address serves ~10^8 returning atomics a second on this chip: a popular bin would take longer than the
// traversal it is meant to speed up).
__device__ __forceinline__ void wf_slice(uint32_t n, uint32_t &lo, uint32_t &hi) {
    const uint32_t per = (n + gridDim.x - 1) / gridDim.x;
    lo = blockIdx.x * per < n ? blockIdx.x * per : n;
    hi = lo + per < n ? lo + per : n;
}
// pass 1: key of every entry (PT_HOLE for a hole) and the histogram of the keys
__global__ __launch_bounds__(PT_BLOCK) void wf_bin_count_kernel(const WfArgs A) {
    __shared__ uint32_t hist[PT_WF_BINS];
    const PathQueue &Q = A.qin;
    const uint32_t n = queue_len(Q);
    const size_t qc = Q.cap;
    for (uint32_t k = threadIdx.x; k < PT_WF_BINS; k += PT_BLOCK) hist[k] = 0;
    __syncthreads();
    uint32_t lo, hi;
    wf_slice(n, lo, hi);
    for (uint32_t i = lo + threadIdx.x; i < hi; i += PT_BLOCK) {
        uint32_t key = PT_HOLE;
        if (Q.job[i] != PT_HOLE) {
            key = wf_ray_key(A.F, Q.d[i], Q.d[qc + i], Q.d[2 * qc + i], Q.d[3 * qc + i], Q.d[4 * qc + i], Q.d[5 * qc + i]);
            atomicAdd(&hist[key], 1u);
        }
        A.bin_key[i] = key;
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < PT_WF_BINS; k += PT_BLOCK)
        if (hist[k]) atomicAdd(&A.bin_count[k], hist[k]);
}
// pass 2: exclusive prefix sum of the histogram (one block), total -> bin_count[PT_WF_BINS]
__global__ __launch_bounds__(1024) void wf_bin_scan_kernel(const WfArgs A) {
    __shared__ uint32_t part[1024];
    constexpr uint32_t PER = PT_WF_BINS / 1024u;
    uint32_t loc[PER];
    uint32_t s = 0;
    for (uint32_t k = 0; k < PER; k++) {
        loc[k] = s;
        s += A.bin_count[threadIdx.x * PER + k];
    }
    part[threadIdx.x] = s;
    __syncthreads();
    for (uint32_t off = 1; off < 1024u; off <<= 1) {  // Hillis-Steele over the 1024 partial sums
        const uint32_t v = threadIdx.x >= off ? part[threadIdx.x - off] : 0u;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    const uint32_t base = part[threadIdx.x] - s;
    for (uint32_t k = 0; k < PER; k++) A.bin_count[threadIdx.x * PER + k] = base + loc[k];
    if (threadIdx.x == 1023u) A.bin_count[PT_WF_BINS] = part[1023];
}
// pass 3: the block reserves room for its slice in every bin (one atomic per bin), its entries take the places
__global__ __launch_bounds__(PT_BLOCK) void wf_bin_scatter_kernel(const WfArgs A, uint32_t *perm) {
    __shared__ uint32_t hist[PT_WF_BINS];
    const uint32_t n = queue_len(A.qin);
    for (uint32_t k = threadIdx.x; k < PT_WF_BINS; k += PT_BLOCK) hist[k] = 0;
    __syncthreads();
    uint32_t lo, hi;
    wf_slice(n, lo, hi);
    for (uint32_t i = lo + threadIdx.x; i < hi; i += PT_BLOCK) {
        const uint32_t key = A.bin_key[i];
        if (key != PT_HOLE) atomicAdd(&hist[key], 1u);
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < PT_WF_BINS; k += PT_BLOCK)
        if (hist[k]) hist[k] = atomicAdd(&A.bin_count[k], hist[k]);  // from here on: next free place of the bin for this block
    __syncthreads();
    for (uint32_t i = lo + threadIdx.x; i < hi; i += PT_BLOCK) {
        const uint32_t key = A.bin_key[i];
        if (key != PT_HOLE) perm[atomicAdd(&hist[key], 1u)] = i;
    }
}

// Fresh jobs -> queue entries (entry i = job i; a job whose pixel lies outside the frame is a hole).
template <bool STATS>
__global__ __launch_bounds__(PT_BLOCK) void wf_init_kernel(const WfArgs A) {
    const DevFrame &F = A.F;
    const TraceBuffers &B = A.B;
    uint32_t c_samples = 0, c_draw = 0;
    // grid-stride: the two counters below get one atomic per wave of a few thousand, not one per 64 jobs
    for (uint32_t i = blockIdx.x * PT_BLOCK + threadIdx.x; i < F.njobs; i += gridDim.x * PT_BLOCK) {
        const uint32_t nd = B.ray_ndraw[i];
        uint32_t job = PT_HOLE;
        if (nd != 0xffffu) {
            c_samples++;
            c_draw += nd;
            if (F.max_depth <= 0) {  // rayColorOpt returns black before any scan (renderer.go:287-289)
                store_path_end<STATS>(&B, i, 0.0, 0.0, 0.0, 0u, nd);
            } else {
                job = i;
                const size_t nj = F.njobs;
                queue_store<ENTRY_PLAIN, STATS>(&A.qin, &B, WindowPush::at(i), B.ray[i], B.ray[nj + i], B.ray[2 * nj + i], B.ray[3 * nj + i], B.ray[4 * nj + i],
                                                B.ray[5 * nj + i], 1.0, 1.0, 1.0, 0.0, B.ray_rng[i], i, F.max_depth, -1, 0u, nd);
            }
        }
        if (job == PT_HOLE && i < A.qin.cap) A.qin.job[i] = PT_HOLE;
    }
    flush_count(&B.counters[2], c_draw, threadIdx.x & (PT_WAVE - 1));
    flush_count(&B.counters[3], c_samples, threadIdx.x & (PT_WAVE - 1));
    if (blockIdx.x == 0 && threadIdx.x == 0) *A.qin.count = F.njobs;
}

// Closest hit (MODE 0) or exit search (MODE 1) of every path in A.qin: best and tmax are written into the entry.
// Persistent waves; a lane that has its answer takes the next entry at once, so the walk loop of scan_bvh always
// starts on a full wave (it is left, as in trace_kernel, once fewer than F.bvh_min_lanes lanes are still walking).
template <int MODE, bool VERIFY>
__global__ __launch_bounds__(PT_BLOCK, PT_BVH_WAVES) void wf_traverse_kernel(const WfArgs A) {
    extern __shared__ __align__(16) unsigned char smem[];
    const DevFrame &F = A.F;
    const TraceBuffers &B = A.B;
    const PathQueue &Q = A.qin;
    int *lds_stack = reinterpret_cast<int *>(smem);
    BvhNode *lds_nodes = reinterpret_cast<BvhNode *>(smem + (size_t)F.bvh_stack * PT_BLOCK * sizeof(int));
    {
        const uint64_t *gsrc = reinterpret_cast<const uint64_t *>(B.bvh_nodes);
        uint64_t *ldst = reinterpret_cast<uint64_t *>(lds_nodes);
        const int nw = F.bvh_lds_nodes * (int)(sizeof(BvhNode) / 8);
        for (int i = threadIdx.x; i < nw; i += PT_BLOCK) ldst[i] = gsrc[i];
        __syncthreads();
    }
    typedef const DevObj __attribute__((address_space(4))) *ConstObjPtr;
    typedef const int32_t __attribute__((address_space(4))) *ConstIdxPtr;
    typedef const uint32_t __attribute__((address_space(4))) *ConstU32Ptr;
    const ConstObjPtr g_obj = (ConstObjPtr)(B.objs);
    const ConstIdxPtr g_pl = (ConstIdxPtr)(B.plane_idx);
    const uint32_t lane = threadIdx.x & (PT_WAVE - 1);
    const uint32_t n_items = A.perm ? *(ConstU32Ptr)(A.n_sorted) : queue_len(Q);
    const size_t qc = Q.cap;

    bool have = false;
    uint32_t idx = 0;
    double ox = 0, oy = 0, oz = 0, dx = 0, dy = 0, dz = 0;
    TravState trav;
    uint32_t cur = 0, end = 0;
    bool exhausted = false;
    uint32_t c_mismatch = 0;
    const ProfHooks ph{nullptr, nullptr, nullptr, lane, nullptr};

    for (;;) {
        const uint64_t need = __ballot(!have);
        if (need != 0) {
            if (cur >= end && !exhausted) {
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(A.cursor, F.claim);
                base = __builtin_amdgcn_readfirstlane(base);
                if (base >= n_items) {
                    exhausted = true;
                } else {
                    cur = base;
                    end = (n_items - base < F.claim) ? n_items : base + F.claim;
                }
            }
            const uint32_t avail = end - cur;
            const uint32_t rank = lane_rank(need);
            const bool take = !have && rank < avail;
            const uint32_t nneed = (uint32_t)__popcll(need);
            const uint32_t item = cur + rank;
            cur += nneed < avail ? nneed : avail;
            if (take) {
                const uint32_t e = A.perm ? A.perm[item] : item;  // sorted order lists no holes
                if (A.perm || Q.job[e] != PT_HOLE) {
                    idx = e;
                    ox = Q.d[e]; oy = Q.d[qc + e]; oz = Q.d[2 * qc + e];
                    dx = Q.d[3 * qc + e]; dy = Q.d[4 * qc + e]; dz = Q.d[5 * qc + e];
                    have = true;
                    trav = TravState();
                }
            }
            if (__ballot(have) == 0) {
                if (exhausted) break;
                continue;
            }
        }
        int best = -1;
        double tmax = 0;
        bool scanned = true;
        bool fat = false;  // a far-away ray with bounds as wide as the scene: the whole wave scans the world for it (see trace_kernel)
        if (have) {
            const RayD ray{ox, oy, oz, dx, dy, dz};
            const double a_ = dx * dx + dy * dy + dz * dz;
            const Clip clip = clip_ray(F, ray, MODE ? 0.0001 : 0.001);
            const bool tame = (a_ >= 1e-100) && (a_ <= 1e100) && (ptm::f_abs(ox) <= 1e100) && (ptm::f_abs(oy) <= 1e100) &&
                              (ptm::f_abs(oz) <= 1e100);
            if (__ballot(!tame) != 0) {  // rays with non-finite or absurd components: the reference's own loop
                scan_uniform(F, g_obj, ray, MODE, best, tmax);
                trav.live = false;
            } else {
                if ((fat = !trav.live && clip.far && !clip.miss && clip.infl * 16.0 > F.scene_bound))
                    scanned = false;
                else if (__ballot(clip.far || !bvh_ray_trusted(F, ray, clip, a_)) != 0)
                    scanned = scan_bvh<false, true>(F, g_obj, g_pl, B.bvh_nodes, lds_nodes, B.bvh_objs, lds_stack + threadIdx.x, ray, clip, MODE,
                                                    trav, best, tmax, ph);
                else
                    scanned = scan_bvh<false, false>(F, g_obj, g_pl, B.bvh_nodes, lds_nodes, B.bvh_objs, lds_stack + threadIdx.x, ray, clip, MODE,
                                                     trav, best, tmax, ph);
                if (VERIFY && scanned) {
                    int best2;
                    double tmax2;
                    scan_uniform(F, g_obj, ray, MODE, best2, tmax2);
                    if (best != best2 || (best >= 0 && !(tmax == tmax2))) {
                        c_mismatch++;
                        record_mismatch(B.counters, best, best2, tmax, tmax2, (unsigned long long)MODE, ray);
                    }
                    best = best2;
                    tmax = tmax2;
                }
            }
        }
        {
            uint64_t fm = __ballot(fat);
            while (fm != 0) {
                const int src = __ffsll((long long)fm) - 1;
                fm &= fm - 1;
                const LinearHit fh = scan_linear_wave(F.nobj, B.objs, __shfl(ox, src, 64), __shfl(oy, src, 64), __shfl(oz, src, 64), __shfl(dx, src, 64),
                                                      __shfl(dy, src, 64), __shfl(dz, src, 64), MODE, lane);
                if ((int)lane == src) {
                    best = fh.best;
                    tmax = fh.tmax;
                    scanned = true;
                    if (VERIFY) {  // the verify instantiation checks this path like the walks above
                        int best2;
                        double tmax2;
                        scan_uniform(F, g_obj, RayD{ox, oy, oz, dx, dy, dz}, MODE, best2, tmax2);
                        if (best != best2 || (best >= 0 && !(tmax == tmax2))) c_mismatch++;
                        best = best2;
                        tmax = tmax2;
                    }
                }
                if (lane == 0) atomicAdd(B.counters + 23, 1ull);
            }
        }
        if (have && scanned) {
            Q.hit[idx] = best;  // (`best` of an exit-queue entry keeps the glass material)
            Q.d[9 * qc + idx] = tmax;
            have = false;
        }
    }
    if (VERIFY) flush_count(&B.counters[4], c_mismatch, lane);
}

// The flat scans as a pass: one path per lane (bitmask scan over <= 32 + 32 records; the wavefront form of the
// reference-sized scenes, kept as the A/B of the all-in-one loop).
template <int MODE, bool VERIFY>
__global__ __launch_bounds__(PT_BLOCK) void wf_scan_flat_kernel(const WfArgs A) {
    extern __shared__ __align__(16) unsigned char smem[];
    const DevFrame &F = A.F;
    const TraceBuffers &B = A.B;
    const PathQueue &Q = A.qin;
    DevObj *lds_obj = reinterpret_cast<DevObj *>(smem);
    int *lds_kidx = reinterpret_cast<int *>(smem + (size_t)F.nobj * sizeof(DevObj));
    stage_record_index(lds_kidx, B.bsph, B.bbox, F.n_bsph, F.n_bbox);
    stage_lds(lds_obj, B.objs, F.nobj * (int)(sizeof(DevObj) / 8));
    typedef const DevObj __attribute__((address_space(4))) *ConstObjPtr;
    typedef const BroadSphere __attribute__((address_space(4))) *ConstSphPtr;
    typedef const BroadBox __attribute__((address_space(4))) *ConstBoxPtr;
    typedef const int32_t __attribute__((address_space(4))) *ConstIdxPtr;
    const ConstObjPtr g_obj = (ConstObjPtr)(B.objs);
    const ConstIdxPtr g_pl = (ConstIdxPtr)(B.plane_idx);
    const BroadLists<ConstSphPtr, ConstBoxPtr> BL{(ConstSphPtr)B.bsph, (ConstBoxPtr)B.bbox, F.n_bsph, F.n_bbox, F.sph_all, F.box_all,
                                                  F.sph_diel, F.box_diel, lds_kidx, lds_kidx + F.n_bsph};
    const uint32_t lane = threadIdx.x & (PT_WAVE - 1);
    const uint32_t n = queue_len(Q);
    const size_t qc = Q.cap;
    uint32_t c_mismatch = 0;
    const ProfHooks ph{nullptr, nullptr, nullptr, lane, nullptr};
    for (uint32_t i0 = blockIdx.x * PT_BLOCK + (threadIdx.x & ~(PT_WAVE - 1u)); i0 < n; i0 += gridDim.x * PT_BLOCK) {
        const uint32_t i = i0 + lane;
        if (i < n && Q.job[i] != PT_HOLE) {
            const RayD ray = queue_load_ray(Q, i);
            int best = -1;
            double tmax = 0;
            const double a_ = ray.dx * ray.dx + ray.dy * ray.dy + ray.dz * ray.dz;
            const Clip clip = clip_ray(F, ray, MODE ? 0.0001 : 0.001);
            const bool tame = (a_ >= 1e-100) && (a_ <= 1e100) && (ptm::f_abs(ray.ox) <= 1e100) && (ptm::f_abs(ray.oy) <= 1e100) &&
                              (ptm::f_abs(ray.oz) <= 1e100) && !clip.far;
            if (__ballot(!tame) != 0) {
                scan_uniform(F, g_obj, ray, MODE, best, tmax);
            } else {
                scan_broad_narrow<false, VERIFY, MODE>(F, g_obj, BL, g_pl, lds_obj, ray, clip, MODE, best, tmax, ph);
                if (VERIFY) {
                    int best2;
                    double tmax2;
                    scan_uniform(F, g_obj, ray, MODE, best2, tmax2);
                    if (best != best2 || (best >= 0 && !(tmax == tmax2))) c_mismatch++;
                    best = best2;
                    tmax = tmax2;
                }
            }
            Q.hit[i] = best;
            Q.d[9 * qc + i] = tmax;
        }
    }
    if (VERIFY) flush_count(&B.counters[4], c_mismatch, lane);
}

// How the wavefront form answers an entry: wf_traverse_kernel (or wf_scan_flat_kernel) left hit and tmax in it.  (pt_walk32.h has the
// other policy, the exact pass.)  A policy is called with the entry and its ray and flushes whatever it counted when the pass ends;
// `before_state` says on which side of the entry's path state it is called, so that each form keeps the order of loads it had: here
// the two planes are read with the rest of the entry, in walk32 the exact pass runs before throughput and stream state are alive.
struct QueueAnswer {
    static constexpr bool before_state = false;
    __device__ __forceinline__ void operator()(const PathQueue &Q, uint32_t i, const RayD &, int &best, double &tmax) const {
        best = Q.hit[i];  // (`best` of an exit-queue entry keeps the glass material)
        tmax = Q.d[9 * (size_t)Q.cap + i];
    }
    __device__ __forceinline__ void flush(unsigned long long *, uint32_t) const {}
};

// Shading of every path in A.qin once its closest hit is known (renderer.go:303-319, :375-403): sky / emitted / scatter / roulette.  Paths that
// go on are appended to A.qout, dielectric front-face hits to A.qexit.  `objs` is where a hit object is read from (the LDS copy of a flat
// scene's world, or HBM / L2), `lds_mat` the staged materials.
template <bool STATS, typename Answer>
__device__ __forceinline__ void shade_pass(const WfArgs &A, const DevObj *objs, const DevMat *lds_mat, Answer answer) {
    const TraceBuffers &B = A.B;
    const PathQueue &Q = A.qin;
    const uint32_t lane = threadIdx.x & (PT_WAVE - 1);
    const uint32_t n = queue_len(Q);
    uint32_t c_seg = 0, c_draw = 0, c_exit = 0;
    QueueWindow w_out, w_exit;

    for (uint32_t i0 = blockIdx.x * PT_BLOCK + (threadIdx.x & ~(PT_WAVE - 1u)); i0 < n; i0 += gridDim.x * PT_BLOCK) {
        const uint32_t i = i0 + lane;
        bool go_on = false, to_exit = false;
        RayD r{0, 0, 0, 0, 0, 0};
        double Tx = 0, Ty = 0, Tz = 0;
        uint64_t rs = 0;
        uint32_t job = PT_HOLE, j_seg = 0, j_draw = 0;
        int depth = 0, exit_mat = 0;
        if (i < n) job = Q.job[i];
        if (job != PT_HOLE) {
            r = queue_load_ray(Q, i);
            int best = -1;
            double tmax = 0;
            if (Answer::before_state) answer(Q, i, r, best, tmax);
            queue_load_state(Q, i, Tx, Ty, Tz, rs, depth, j_seg, j_draw, STATS);
            if (!Answer::before_state) answer(Q, i, r, best, tmax);
            c_seg++;
            if (STATS) j_seg++;
            bool finished = false;
            double termx = 0, termy = 0, termz = 0, attx = 1, atty = 1, attz = 1;
            if (best < 0) {
                finished = true;
                sky_radiance(&A.sky, r.dx, r.dy, r.dz, termx, termy, termz);
            } else {
                bool exit_search = false;
                shade_hit<STATS, true>(objs[best], lds_mat, tmax, r.ox, r.oy, r.oz, r.dx, r.dy, r.dz, rs, c_draw, j_draw, finished, termx, termy,
                                       termz, attx, atty, attz, exit_search, exit_mat);
                if (exit_search) {
                    to_exit = true;
                    c_exit++;
                } else if (!finished) {
                    // (the roulette table from memory: these passes stage the materials only)
                    finished = roulette_step<STATS>(B.roulette, roulette_record_of(objs[best], A.F.nmat), depth, attx, atty, attz, Tx, Ty, Tz, rs, c_draw, j_draw);
                    go_on = !finished;
                }
            }
            if (finished) store_path_end<STATS>(&B, job, Tx * termx, Ty * termy, Tz * termz, j_seg, j_draw);
        }
        if (const uint64_t pm = __ballot(go_on)) {
            const WindowPush wp = window_reserve(w_out, &A.qout, pm, lane, PT_CONT_BLOCK);
            if (go_on) queue_store<ENTRY_PLAIN, STATS>(&A.qout, &B, WindowPush::at(wp.slot), r.ox, r.oy, r.oz, r.dx, r.dy, r.dz, Tx, Ty, Tz, 0.0, rs, job, depth, -1, j_seg, j_draw);
        }
        if (const uint64_t pm = __ballot(to_exit)) {
            const WindowPush wp = window_reserve(w_exit, &A.qexit, pm, lane, PT_QUEUE_BLOCK);
            if (to_exit) queue_store<ENTRY_BEST, STATS>(&A.qexit, &B, WindowPush::at(wp.slot), r.ox, r.oy, r.oz, r.dx, r.dy, r.dz, Tx, Ty, Tz, 0.0, rs, job, depth, exit_mat, j_seg, j_draw);
        }
    }
    window_close(w_out, &A.qout, lane);
    window_close(w_exit, &A.qexit, lane);
    flush_count(&B.counters[0], c_seg, lane);
    flush_count(&B.counters[1], c_exit, lane);
    flush_count(&B.counters[2], c_draw, lane);
    answer.flush(B.counters, lane);
}

// After the exit searches of a level (renderer.go:352-403): every entry of A.qin (the exit queue; `best` = the glass
// material, the policy's answer = where the way out ends) gets its attenuation, its origin moved to the exit
// point and its roulette; survivors are appended to A.qout.
template <bool STATS, typename Answer>
__device__ __forceinline__ void exit_pass(const WfArgs &A, const DevMat *lds_mat, Answer answer) {
    const TraceBuffers &B = A.B;
    const PathQueue &Q = A.qin;
    const uint32_t lane = threadIdx.x & (PT_WAVE - 1);
    const uint32_t n = queue_len(Q);
    uint32_t c_draw = 0;
    QueueWindow w_out;
    for (uint32_t i0 = blockIdx.x * PT_BLOCK + (threadIdx.x & ~(PT_WAVE - 1u)); i0 < n; i0 += gridDim.x * PT_BLOCK) {
        const uint32_t i = i0 + lane;
        bool go_on = false;
        RayD r{0, 0, 0, 0, 0, 0};
        double Tx = 0, Ty = 0, Tz = 0;
        uint64_t rs = 0;
        uint32_t job = PT_HOLE, j_seg = 0, j_draw = 0;
        int depth = 0;
        if (i < n) job = Q.job[i];
        if (job != PT_HOLE) {
            r = queue_load_ray(Q, i);
            int ebest = -1;
            double tmax = 0;
            if (Answer::before_state) answer(Q, i, r, ebest, tmax);
            queue_load_state(Q, i, Tx, Ty, Tz, rs, depth, j_seg, j_draw, STATS);
            if (!Answer::before_state) answer(Q, i, r, ebest, tmax);
            const int exit_mat = Q.best[i];
            double attx = 1, atty = 1, attz = 1;
            exit_post(lds_mat[exit_mat], ebest, tmax, r.ox, r.oy, r.oz, r.dx, r.dy, r.dz, attx, atty, attz);
            go_on = !roulette_step<STATS>(B.roulette, roulette_record_after_exit(lds_mat[exit_mat], ebest, A.F.nmat), depth, attx, atty, attz, Tx, Ty, Tz, rs, c_draw, j_draw);
            if (!go_on) store_path_end<STATS>(&B, job, Tx * 0.0, Ty * 0.0, Tz * 0.0, j_seg, j_draw);
        }
        if (const uint64_t pm = __ballot(go_on)) {
            const WindowPush wp = window_reserve(w_out, &A.qout, pm, lane, PT_CONT_BLOCK);
            if (go_on) queue_store<ENTRY_PLAIN, STATS>(&A.qout, &B, WindowPush::at(wp.slot), r.ox, r.oy, r.oz, r.dx, r.dy, r.dz, Tx, Ty, Tz, 0.0, rs, job, depth, -1, j_seg, j_draw);
        }
    }
    window_close(w_out, &A.qout, lane);
    flush_count(&B.counters[2], c_draw, lane);
    answer.flush(B.counters, lane);
}

// The wavefront form of the two passes: small scenes keep world and materials in LDS; BVH scenes: materials only (objects come from
// HBM / L2).
template <bool STATS>
__global__ __launch_bounds__(PT_BLOCK) void wf_shade_kernel(const WfArgs A) {
    extern __shared__ __align__(16) unsigned char smem[];
    const DevFrame &F = A.F;
    const bool world_in_lds = F.world_in_lds != 0;
    DevObj *lds_obj = reinterpret_cast<DevObj *>(smem);
    DevMat *lds_mat = reinterpret_cast<DevMat *>(smem + (world_in_lds ? (size_t)F.nobj * sizeof(DevObj) : 0));
    if (world_in_lds) stage_lds(lds_obj, A.B.objs, F.nobj * (int)(sizeof(DevObj) / 8));
    stage_lds(lds_mat, A.B.mats, F.nmat * (int)(sizeof(DevMat) / 8));
    shade_pass<STATS>(A, world_in_lds ? lds_obj : A.B.objs, lds_mat, QueueAnswer{});
}
template <bool STATS>
__global__ __launch_bounds__(PT_BLOCK) void wf_exit_kernel(const WfArgs A) {
    extern __shared__ __align__(16) unsigned char smem[];
    DevMat *lds_mat = reinterpret_cast<DevMat *>(smem);
    stage_lds(lds_mat, A.B.mats, A.F.nmat * (int)(sizeof(DevMat) / 8));
    exit_pass<STATS>(A, lds_mat, QueueAnswer{});
}

}  // namespace ptk
