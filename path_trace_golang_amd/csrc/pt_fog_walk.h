// pt_fog_walk.h -- the fog's in-scatter term on a BVH scene (pt_set_fog_walk), the tree walked by the WAVE.
//
// fog_kernel (pt_kernels.h) answers every shadow ray of the term by ptf::occluded's loop over all objects: 24 march steps x lights x
// objects per sample, which is why the volumetric term is refused on the BVH path.  A fog wave is one sample of one 8 x 8 block
// (job = q * 64 + p, the same row q in every lane): its 64 primary rays are the population wave_first_hit (pt_wave_walk.h) was written
// for, and its 64 shadow rays of one (march step, light) start at 64 neighbouring march points and end on one light sphere.
// fog_bvh_kernel keeps fog_body's bookkeeping (job -> pixel, the fog stream, L = L_path + L_fog in place, the three counters by
// wave_sum) and the model's pieces as pt_fog.h states them (march_range, medium_coeffs, light_sample, light_add, light_total), and
//   * takes the primary ray's closest hit from wave_first_hit (an odd wave: scan_uniform, mode 0), the loop's t bit for bit;
//   * walks the march and light loops in wave-uniform control flow: the lanes' skips (pixel outside the frame, !(step > 0),
//     st <= 0 || ss <= 0, pdf <= 0, dist_sq <= 1e-6, !(cl > 0)) are a predicate, the draws u1, u2 are taken before the skips by the
//     lanes that reach the light loop, as in volume_light;
//   * answers the 64 shadow rays of a (step, light) turn by ONE walk, wave_any_hit below.
//
// wave_any_hit has wave_first_hit's shape -- one LDS stack per wave, nodes and object records by scalar loads at wave-uniform
// addresses, the four slot boxes as scalar operands of the lanes' FP32 slab tests, descent into a child that any still-unoccluded
// lane pierces (ballot) -- and none of its order: occlusion is an OR over objects, so there are no tie rules, no winner and no
// nearest-first sort (children are visited in slot order).  On a pierced object slot the lanes whose own slab test passed run
// ptf::hit_object itself on the BvhObj's DevObj, the very test of ptf::occluded, with the lane's own fixed [0.001, tmax].  The FP32
// bounds are conservative (slab_recips with F.dir_floor, tminf lowered, tmaxf raised to >= tmax, NaN slabs constrain nothing: the
// derivation of wave_first_hit), the planes are outside the tree and tested exactly before it, a blocked lane pierces nothing more,
// and the walk ends on an empty stack or when no active lane is unoccluded.  A lane therefore runs the exact test on every object
// whose inflated box its ray pierces within its range unless it is occluded already: the OR of the loop, bit for bit.
// A turn goes to the walk only when wave_walk_coop holds for its rays (march points can lie outside clip_bound when the camera is
// far from the scene); otherwise it takes the plain loop over all objects, where inactive lanes count as occluded so that the
// ballot exit still works.  (profiles/fog_bvh_kernel_regs.txt.)
#pragma once

#include "pt_wave_walk.h"

namespace ptk {

struct FogWalkArgs {
    FogArgs A;
    DevFrame F;                       // bvh_root, n_plane, clip_bound, origin_bound, dir_floor, nobj
    const BvhNode *bvh_nodes;
    const BvhObj *bvh_objs;
    const int32_t *plane_idx;
    unsigned long long *stats;        // [6]: primary (wave, sample) pairs walked, ... sent to the plain scan, shadow turns walked, ... sent to
                                      // the plain loop, node visits of the shadow walks, the deepest stack of either walk
};

// A record behind a scalar (constant address space) pointer as the DevObj ptf::hit_object takes: the fields its tests read.
template <typename O>
__device__ __forceinline__ DevObj fog_obj(const O &o) {
    DevObj d;
    d.a[0] = o.a[0]; d.a[1] = o.a[1]; d.a[2] = o.a[2];
    d.b[0] = o.b[0]; d.b[1] = o.b[1]; d.b[2] = o.b[2];
    d.radius = 0.0;
    d.radius_sq = o.radius_sq;
    d.inv_radius = 0.0;
    d.kind = o.kind;
    d.mat = 0;
    return d;
}

// ptf::occluded's loop for a wave: every lane on the same object; `active` lanes hold a shadow ray, the others count as occluded.
template <typename ObjPtr>
__device__ __forceinline__ bool wave_any_hit_plain(const DevFrame &F, ObjPtr g_obj, bool active, const ptf::FRay &r, double tmax) {
    bool blocked = !active;
    for (int i = 0; i < F.nobj; i++) {
        const DevObj o = fog_obj(g_obj[i]);
        double t;
        if (!blocked && ptf::hit_object(o, r, 0.001, tmax, t)) blocked = true;
        if (__ballot(!blocked) == 0) break;
    }
    return blocked;
}

// Does any object of the scene hit the lane's ray in [0.001, tmax]?  For every lane of a wave_walk_coop wave; `active` lanes hold a
// ray (r.a = d.d), the others take no part.  wst is the wave's stack (PT_BVH_STACK words of LDS).  c_visits counts the nodes visited,
// c_deep follows the deepest stack; both are wave-uniform.
template <typename NodePtr, typename BObjPtr, typename ObjPtr, typename IdxPtr>
__device__ __forceinline__ bool wave_any_hit(const DevFrame &F, NodePtr nodes, BObjPtr bobjs, ObjPtr g_obj, IdxPtr g_pl, bool active,
                                             const ptf::FRay &r, double tmax, int *const wst, uint32_t &c_visits, uint32_t &c_deep) {
    const double tmin = 0.001;
    bool blocked = !active;
    // ---- planes: infinite, outside the tree, always tested exactly
    for (int k = 0; k < F.n_plane; k++) {
        const DevObj o = fog_obj(g_obj[g_pl[k]]);
        double t;
        if (!blocked && ptf::hit_object(o, r, tmin, tmax, t)) blocked = true;
    }
    if (F.bvh_root < 0 || __ballot(!blocked) == 0) return blocked;
    // FP32 quantities of the node tests, as wave_first_hit derives them (the ray starts inside the clip bound).  tmaxf >= tmax for
    // every tmax >= tmin, where floats are normal; below tmin the exact tests accept nothing and the slabs may cull anything.
    const float fox = (float)r.o[0], foy = (float)r.o[1], foz = (float)r.o[2];
    float tminf = (float)tmin;
    tminf -= __builtin_fabsf(tminf) * 1e-2f + 1e-6f;
    tminf = __builtin_fmaxf(tminf, 0.0f);
    float ivxf, ivyf, ivzf;
    slab_recips(F.dir_floor, (float)r.d[0], (float)r.d[1], (float)r.d[2], ivxf, ivyf, ivzf);
    const float aivxf = __builtin_fabsf(ivxf), aivyf = __builtin_fabsf(ivyf), aivzf = __builtin_fabsf(ivzf);
    const float noxf = -fox * ivxf, noyf = -foy * ivyf, nozf = -foz * ivzf;
    float tmaxf = (float)tmax;
    tmaxf += __builtin_fabsf(tmaxf) * 4.8e-7f;
    int sp = 0;
    int cur = F.bvh_root;
    while (cur >= 0) {
        c_visits++;
        const auto &nd_ = nodes[cur];  // wave-uniform: scalar loads
        const uint32_t meta = nd_.meta;
        const int nbase = nd_.node_base, obase = nd_.obj_base;
        int next = -1;
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const bool is_node = (meta >> (8 + s)) & 1u, is_obj = (meta >> (12 + s)) & 1u;
            if (!(is_node || is_obj)) continue;  // empty slot (wave-uniform)
            const float tcx = __builtin_fmaf(nd_.c[0][s], ivxf, noxf), tcy = __builtin_fmaf(nd_.c[1][s], ivyf, noyf),
                        tcz = __builtin_fmaf(nd_.c[2][s], ivzf, nozf);
            const float t0 = pt_vmax3(__builtin_fmaf(-nd_.h[0][s], aivxf, tcx), __builtin_fmaf(-nd_.h[1][s], aivyf, tcy),
                                      pt_vmax(__builtin_fmaf(-nd_.h[2][s], aivzf, tcz), tminf));
            const float t1 = pt_vmin3(__builtin_fmaf(nd_.h[0][s], aivxf, tcx), __builtin_fmaf(nd_.h[1][s], aivyf, tcy),
                                      pt_vmin(__builtin_fmaf(nd_.h[2][s], aivzf, tcz), tmaxf));
            const bool pierced = !blocked && !(t1 < t0);  // NaN slabs constrain nothing; a blocked lane pierces nothing
            if (__ballot(pierced) == 0) continue;
            const int rank = (int)((meta >> (2 * s)) & 3u);
            if (is_node) {
                if (next < 0) {
                    next = nbase + rank;
                } else {
                    wst[sp] = nbase + rank;
                    sp++;
                }
            } else if (pierced) {
                // the slot's object, for every lane whose own slab test passed: the test of ptf::occluded itself
                const DevObj o = fog_obj(bobjs[obase + rank].o);
                double t;
                if (ptf::hit_object(o, r, tmin, tmax, t)) blocked = true;
            }
        }
        if ((uint32_t)sp > c_deep) c_deep = (uint32_t)sp;
        if (__ballot(!blocked) == 0) break;  // every active lane is occluded
        if (next >= 0) {
            cur = next;
        } else if (sp > 0) {
            sp--;
            cur = __builtin_amdgcn_readfirstlane(wst[sp]);
        } else {
            cur = -1;
        }
    }
    return blocked;
}

template <bool ADAPT>
__device__ __forceinline__ void fog_walk_body(const FogWalkArgs &W, const uint32_t *__restrict__ active_blocks, int *const wst) {
    const FogArgs &A = W.A;
    const DevFrame &F = W.F;
    typedef const BvhNode __attribute__((address_space(4))) *ConstNodePtr;
    typedef const BvhObj __attribute__((address_space(4))) *ConstBObjPtr;
    typedef const DevObj __attribute__((address_space(4))) *ConstObjPtr;
    typedef const int32_t __attribute__((address_space(4))) *ConstIdxPtr;
    typedef const ptf::FogLight __attribute__((address_space(4))) *ConstLightPtr;
    const ConstNodePtr nodes = (ConstNodePtr)W.bvh_nodes;
    const ConstBObjPtr bobjs = (ConstBObjPtr)W.bvh_objs;
    const ConstObjPtr g_obj = (ConstObjPtr)A.objs;
    const ConstIdxPtr g_pl = (ConstIdxPtr)W.plane_idx;
    const ConstLightPtr g_light = (ConstLightPtr)A.lights;
    const ptf::FogParams &P = A.P;
    const uint32_t job = blockIdx.x * PT_BLOCK + threadIdx.x;
    if (job >= A.njobs) return;  // (whole waves: the jobs come in rows of 64)
    const bool have = A.ray_ndraw[job] != 0xffffu;  // a pixel outside the frame: the lane stays, idle
    if (__ballot(have) == 0) return;                // a block with no pixel inside the frame (wave-uniform)
    // job -> (tile, sub-block, sample, pixel) as in fog_body
    const uint32_t p = job & 63u;
    const uint32_t q = job >> 6;
    const uint32_t cblk = q / A.S;
    const uint32_t sl = q - cblk * A.S;
    const uint32_t blk = ADAPT ? active_blocks[__builtin_amdgcn_readfirstlane(cblk)] : cblk;
    const Pixel px = block_pixel(A.G, blk, p);
    const size_t nj = A.njobs;
    // an idle lane marches a harmless ray of its own; nothing of it is counted or stored
    const double orig[3] = {have ? A.ray[job] : 0.0, have ? A.ray[nj + job] : 0.0, have ? A.ray[2 * nj + job] : 0.0};
    const double dir[3] = {have ? A.ray[3 * nj + job] : 0.0, have ? A.ray[4 * nj + job] : 0.0, have ? A.ray[5 * nj + job] : 1.0};
    uint64_t rs = ptm::stream_init(A.fog_key, (uint64_t)px.y * (uint64_t)(uint32_t)A.G.width + px.x, (uint64_t)(A.s0 + sl));
    ptf::FogCount cnt = {0u, 0u, 0u};
    uint32_t c_prim_walked = 0, c_prim_plain = 0, c_walked = 0, c_plain = 0, c_visits = 0, c_deep = 0;  // wave-uniform
    // ------------------------------------------------------------ the primary ray's closest hit: the wave's walk, or the plain loop for an odd wave
    double tmax, u[3];
    {
        const double a = dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2];
        const RayD r{orig[0], orig[1], orig[2], dir[0], dir[1], dir[2]};
        const bool coop = wave_walk_coop(F, have, r, a);
        int best = -1;
        double t_hit = ptm::max_float64();
        uint32_t pv = 0, pd = 0;
        if (coop) c_prim_walked++;
        else c_prim_plain++;
        if (coop && have) {
            wave_first_hit<true>(F, nodes, bobjs, g_obj, g_pl, orig[0], orig[1], orig[2], dir[0], dir[1], dir[2], a, wst, best, t_hit, pv, pd);
        } else if (have) {
            scan_uniform(F, g_obj, r, 0, best, t_hit);
        }
        const uint32_t deep = (uint32_t)__builtin_amdgcn_readlane((int)pd, __ffsll((long long)__ballot(have)) - 1);
        if (deep > c_deep) c_deep = deep;
        tmax = ptf::march_range(dir, best >= 0, t_hit, u);
    }
    // ------------------------------------------------------------ the march (ptf::fog_march) with the lanes' skips as predicates
    double L[3] = {0, 0, 0};
    const double step = tmax / PTF_STEPS;
    const bool live = have && step > 0;
    for (int i = 0; i < PTF_STEPS; i++) {
        const double t = ((double)i + 0.5) * step;
        const double mx = orig[0] + u[0] * t, my = orig[1] + u[1] * t, mz = orig[2] + u[2] * t;
        double ss, st;
        ptf::medium_coeffs(P, mx, my, mz, ss, st);
        const bool stepping = live && !(st <= 0 || ss <= 0);
        if (stepping) cnt.steps++;
        if (__ballot(stepping) == 0) continue;
        const double tr = ptm::go_exp(-st * t);
        double ls[3] = {0, 0, 0};
        if (!(P.scatter <= 0)) {  // ptf::volume_light
            double sum[3] = {0, 0, 0};
            for (int32_t j = 0; j < A.nlight; j++) {
                ptf::FogLight l;
                l.c[0] = g_light[j].c[0]; l.c[1] = g_light[j].c[1]; l.c[2] = g_light[j].c[2];
                l.radius = g_light[j].radius;
                l.le[0] = g_light[j].le[0]; l.le[1] = g_light[j].le[1]; l.le[2] = g_light[j].le[2];
                l.pad = 0;
                double u1 = 0.5, u2 = 0.5;
                if (stepping) {
                    u1 = ptm::stream_next(rs);
                    u2 = ptm::stream_next(rs);
                    cnt.draws += 2;
                }
                ptf::LightSample s;
                const bool lit = ptf::light_sample(l, u1, u2, mx, my, mz, s);
                const bool casts = stepping && lit;  // the lane holds a shadow ray this turn
                if (casts) cnt.shadow_rays++;
                if (__ballot(casts) == 0) continue;
                // -------------------------------------------------- one shadow turn of the wave
                const ptf::FRay fr = ptf::make_fray(mx, my, mz, casts ? s.w[0] : 0.0, casts ? s.w[1] : 0.0, casts ? s.w[2] : 1.0);
                const double stmax = casts ? ptf::shadow_tmax(s) : 0.0;
                const RayD r{mx, my, mz, fr.d[0], fr.d[1], fr.d[2]};
                const bool coop = wave_walk_coop(F, casts, r, fr.a);
                bool blocked;
                if (coop) {
                    c_walked++;
                    blocked = wave_any_hit(F, nodes, bobjs, g_obj, g_pl, casts, fr, stmax, wst, c_visits, c_deep);
                } else {
                    c_plain++;
                    blocked = wave_any_hit_plain(F, g_obj, casts, fr, stmax);
                }
                if (!blocked) ptf::light_add(P, l, s, u, sum);  // (blocked holds for every lane without a ray)
            }
            ptf::light_total(sum, ls);
        }
        if (stepping)
            for (int c = 0; c < 3; c++) L[c] += P.color[c] * ls[c] * ss * tr * step;
    }
    if (have) {
        double4 *rec = reinterpret_cast<double4 *>(A.L) + job;
        double4 l = *rec;
        l.x = l.x + L[0];
        l.y = l.y + L[1];
        l.z = l.z + L[2];
        *rec = l;
    }
    const uint32_t sr = wave_sum(cnt.shadow_rays), dr = wave_sum(cnt.draws), sn = wave_sum(cnt.steps);
    if ((threadIdx.x & 63u) == 0u) {
        if ((sr | dr | sn) != 0u) {
            atomicAdd(A.counters + 0, (unsigned long long)sr);
            atomicAdd(A.counters + 1, (unsigned long long)dr);
            atomicAdd(A.counters + 2, (unsigned long long)sn);
        }
        if (c_prim_walked) atomicAdd(W.stats + 0, (unsigned long long)c_prim_walked);
        if (c_prim_plain) atomicAdd(W.stats + 1, (unsigned long long)c_prim_plain);
        if (c_walked) atomicAdd(W.stats + 2, (unsigned long long)c_walked);
        if (c_plain) atomicAdd(W.stats + 3, (unsigned long long)c_plain);
        if (c_visits) atomicAdd(W.stats + 4, (unsigned long long)c_visits);
        if (c_deep) atomicMax(W.stats + 5, (unsigned long long)c_deep);
    }
}

__global__ __launch_bounds__(PT_BLOCK) void fog_bvh_kernel(const FogWalkArgs W) {
    __shared__ int wstack[PT_BLOCK / PT_WAVE][PT_BVH_STACK];
    fog_walk_body<false>(W, nullptr, wstack[threadIdx.x >> 6]);
}

__global__ __launch_bounds__(PT_BLOCK) void fog_bvh_adaptive_kernel(const FogWalkArgs W, const uint32_t *__restrict__ active_blocks) {
    __shared__ int wstack[PT_BLOCK / PT_WAVE][PT_BVH_STACK];
    fog_walk_body<true>(W, active_blocks, wstack[threadIdx.x >> 6]);
}

}  // namespace ptk
