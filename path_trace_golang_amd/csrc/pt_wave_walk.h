// pt_wave_walk.h -- the first hit of 64 coherent rays of a BVH scene, the tree walked by the WAVE instead of by the lane.
//
// A trace wave of the BVH path walks 64 unrelated rays, one stack per lane: divergent node fetches (six 16-byte requests per
// lane and visit), a fifth to a half of the lanes waiting for the slowest walks of the wave.  Where the 64 jobs of a
// wave are one sample of one 8 x 8 pixel block (pt_device.h), i.e. 64 rays from (nearly) one point through (nearly) one direction,
// none of that is necessary.  wave_first_hit gives such a wave ONE stack:
//   * a node is fetched once per wave by scalar loads (wave-uniform address, no vector memory request at all) and its four
//     slot boxes feed the lanes' FP32 slab tests as scalar operands;
//   * the wave descends into a child when ANY lane's ray pierces it before that lane's own tmax (ballot), nearest first
//     by the entry parameter of the first lane that pierces it, the others pushed on the wave's stack (LDS, 96 words);
//   * an object slot pierced by any lane is tested at once: the 96-byte record arrives by scalar loads, the kind is
//     wave-uniform (no divergence between sphere and box code), the lanes whose own slab test passed run the reference's
//     exact FP64 test (objects.go:37-61, :141-179) and take the winner by `wins` (order-free statement of the loop,
//     renderer.go:297-302), each culling against its own tmax from then on.
// Every lane therefore tests at least the objects its own per-lane walk would have tested (those whose inflated box its ray
// pierces before its current tmax) -- the result is the sequential loop's winner, bit for bit; `verify_bvh` checks it.
//
// primary_bvh_kernel (pt_primary.h) and feature_bvh_kernel (pt_feature_walk.h) both call it.  The ray comes in BY VALUE, component
// by component: primary_bvh_kernel sits at its 80 VGPRs with 62 - 74 spilled SGPRs, and with the ray as a `const RayD &` it spills
// 2 - 23 VGPRs to scratch and the feature kernels take 101 VGPRs instead of 87 (profiles/wave_walk_kernel_regs.txt).  The
// classification reads the ray once, before the walk, and costs the same either way.
#pragma once

#include "pt_kernels.h"

namespace ptk {

// Is this a wave for the shared walk?  Not one that holds a ray with non-finite or absurd components, one that starts outside
// 3.5 scene sizes (clip / far-origin logic of clip_ray) or outside the range the FP32 bounds were analysed for.  Wave-uniform.
__device__ __forceinline__ bool wave_walk_coop(const DevFrame &F, bool have, const RayD &r, double a) {
    const double ox = r.ox, oy = r.oy, oz = r.oz;
    const double Cb = F.clip_bound;
    const bool tame = (a >= 1e-100) && (a <= 1e100) && (ptm::f_abs(ox) <= Cb) && (ptm::f_abs(oy) <= Cb) && (ptm::f_abs(oz) <= Cb);
    const Clip noclip{0.0, 0.0, 0.0, false, false};  // origins within 3.5 scene sizes are scanned from where they are (clip_ray: `inside`)
    const bool odd = have && !(tame && bvh_ray_trusted(F, r, noclip, a));
    return __ballot(odd) == 0;
}

// The walk, for the lanes of a wave_walk_coop wave that hold a ray: `best` / `tmax` come in as "no hit" (-1, MaxFloat64) and leave
// as the winner of the scene's planes and BVH objects.  a = d.d; wst is the wave's stack (PT_BVH_STACK words of LDS).  c_visits
// counts the nodes visited; DEEP: c_deep follows the deepest stack.
template <bool DEEP, typename NodePtr, typename BObjPtr, typename ObjPtr, typename IdxPtr>
__device__ __forceinline__ void wave_first_hit(const DevFrame &F, NodePtr nodes, BObjPtr bobjs, ObjPtr g_obj, IdxPtr g_pl, double ox, double oy,
                                               double oz, double dx, double dy, double dz, double a, int *const wst, int &best, double &tmax,
                                               uint32_t &c_visits, uint32_t &c_deep) {
    const RayD r{ox, oy, oz, dx, dy, dz};
    const double tmin = 0.001;  // renderer.go:292
    bool best_is_box = false;
    // ---- planes: infinite, always tested exactly (scan_bvh does the same)
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
    if (F.bvh_root < 0) return;
    const double ya = div_recip(a);
    const double ivx = 1 / dx, ivy = 1 / dy, ivz = 1 / dz;  // objects.go:149,154,159
    // FP32 quantities of the node tests, as scan_bvh derives them (ts = 0: the ray starts inside the clip bound)
    const float fox = (float)ox, foy = (float)oy, foz = (float)oz;
    float tminf = (float)tmin;
    tminf -= __builtin_fabsf(tminf) * 1e-2f + 1e-6f;
    tminf = __builtin_fmaxf(tminf, 0.0f);
    float ivxf, ivyf, ivzf;
    slab_recips(F.dir_floor, (float)dx, (float)dy, (float)dz, ivxf, ivyf, ivzf);
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
        for (int s = 0; s < 4; s++) {
            const bool is_node = (meta >> (8 + s)) & 1u, is_obj = (meta >> (12 + s)) & 1u;
            if (!(is_node || is_obj)) continue;  // empty slot (wave-uniform)
            // slab parameters from centre and half extent (see PT_BOX_SLABS); the half extents carry the embedded index
            // bytes of the per-lane walk in their low mantissa bits: still upper bounds
            const float tcx = __builtin_fmaf(nd_.c[0][s], ivxf, noxf), tcy = __builtin_fmaf(nd_.c[1][s], ivyf, noyf),
                        tcz = __builtin_fmaf(nd_.c[2][s], ivzf, nozf);
            const float t0 = pt_vmax3(__builtin_fmaf(-nd_.h[0][s], aivxf, tcx), __builtin_fmaf(-nd_.h[1][s], aivyf, tcy),
                                      pt_vmax(__builtin_fmaf(-nd_.h[2][s], aivzf, tcz), tminf));
            const float t1 = pt_vmin3(__builtin_fmaf(nd_.h[0][s], aivxf, tcx), __builtin_fmaf(nd_.h[1][s], aivyf, tcy),
                                      pt_vmin(__builtin_fmaf(nd_.h[2][s], aivzf, tcz), tmaxf));
            const bool pierced = !(t1 < t0);  // NaN slabs constrain nothing, like the per-lane walk
            const uint64_t pm = __ballot(pierced);
            if (pm == 0) continue;
            if (is_node) {
                // entry parameter of the first lane that pierces the slot (>= 0: its bits order like the value), slot in the low bits
                const int src = __ffsll((long long)pm) - 1;
                const uint32_t bits = (uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(t0), src);
                key[s] = (bits & ~3u) | (uint32_t)s;
            } else if (pierced) {
                // the slot's object, for every lane whose own slab test passed: the reference's exact test
                const auto &bo = bobjs[obase + (int)((meta >> (2 * s)) & 3u)];
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
        sort4_keys(key[0], key[1], key[2], key[3], k0, k1, k2, k3);
#define PT_CHILD(k) (nbase + (int)((meta >> (2u * ((k) & 3u))) & 3u))
        if (k1 != 0xffffffffu) {  // sorted: k2 and k3 can only be candidates when k1 is
            if (k2 != 0xffffffffu) {
                if (k3 != 0xffffffffu) { wst[sp] = PT_CHILD(k3); sp++; }
                wst[sp] = PT_CHILD(k2);
                sp++;
            }
            wst[sp] = PT_CHILD(k1);
            sp++;
            if (DEEP && (uint32_t)sp > c_deep) c_deep = (uint32_t)sp;
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

}  // namespace ptk
