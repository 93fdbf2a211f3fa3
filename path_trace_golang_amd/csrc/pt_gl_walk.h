// pt_gl_walk.h -- GL shading's two ray queries on a BVH scene (pt_set_shading_walk), the tree walked by the LANE.
//
// gl_trace_kernel answers every segment, every NEE shadow ray and every metal probe of ptg::ray_color by a loop over all objects
// (ptg::closest, ptg::occluded), which is why GL shading is refused on the BVH path.  The lanes of a GL wave sit at different
// depths, materials and light indices, so the wave-shared walks (wave_first_hit, wave_any_hit) do not fit: here one lane walks
// one ray with one stack -- its column of an LDS array on the device (F.bvh_stack entries, stride PT_BLOCK, as scan_bvh's), a
// local array of PT_BVH_STACK on the host -- with no ballot and no wave-uniform assumption, so the routines may be called from
// divergent control flow.  Everything is PT_HD: the CPU suite holds the walk to the loop without a GPU.
//
//   walk_closest   = ptg::closest:  planes first (outside the tree, exact), then the tree nearest child first; a pierced object
//                    slot runs ptg::hit_t itself on S.objs[bobjs[k].index] with the query's own [tmin, tmax_start], and the
//                    candidate replaces the holder by walk_wins, the order-free statement of the loop's winner (below).
//   walk_occluded  = ptg::occluded: planes first, then the tree in slot order, ended by the first hit of hit_t in [0.001, tmax].
//
// The FP32 slot-box tests are wave_any_hit's (pt_fog_walk.h): slab_recips with F.dir_floor, tminf lowered below tmin and clamped
// at 0, tmaxf = the current best raised by 4.8e-7 relative and re-derived whenever best shrinks, NaN slabs constrain nothing,
// and pruning is non-strict (!(t1 < t0)): a child entered exactly at tmaxf is visited, so ties reach the exact test.
//
// The winner.  In ptg::closest an object's candidate parameter t_i does not depend on the running best: a sphere's is its near
// root if that is >= tmin, else its far root; a box's is max(tmin, entry) provided its slabs overlap; a plane's is its tt.  Only
// acceptance reads best: sphere and plane are accepted iff t_i <= best (`root > tmax` rejects), a box iff t_i < best (`t1 <= t0`
// rejects, with t1 = min(best, exits)).  So the loop returns the smallest t, and among equal t the non-box of LARGEST index if
// there is one, else the box of SMALLEST index; the same at tmax_start (a sphere at <=, a box at <), which hit_t applies when it
// is given tmax_start.  walk_wins compares by exactly that total order, so any visit order gives the loop's (index, t), bit for
// bit.  (the per-lane fallback: a ray outside the analysed range -- walk_ok -- takes the plain loop for that query.)
#pragma once

#include "pt_device.h"
#include "pt_glshade.h"
#include "pt_slab.h"

#include <string>
#include <vector>

namespace ptg {

// What the walks of one lane did: queries walked / sent to the plain loop, node visits, the deepest stack.
struct WalkCount {
    uint32_t closest_walked, closest_plain, shadow_walked, shadow_plain, closest_visits, shadow_visits, deepest;
};

// May this ray walk?  Finite, 1e-29 < d.d < 1e29, the origin within F.clip_bound and 0.99 F.origin_bound: the conditions of
// wave_walk_coop / bvh_ray_trusted, per lane and per query.  (A NaN or an infinity fails a comparison.)
PT_HD bool walk_ok(const ptd::DevFrame &F, const double ro[3], const double rd[3]) {
    const double a = dot3(rd, rd);
    const double lim = 0.99 * (double)F.origin_bound, Cb = F.clip_bound;
    bool ok = (a > 1e-29) && (a < 1e29);
    for (int k = 0; k < 3; k++) ok = ok && (ptm::f_abs(ro[k]) <= Cb) && (ptm::f_abs(ro[k]) <= lim);
    return ok;
}

// Does candidate (is_box, i, t) replace the holder (hit, hit_is_box, best)?  The loop's winner as a total order: smaller t; on
// equal t a non-box before a box, the larger index among non-boxes, the smaller among boxes.  No holder: the candidate passed
// hit_t's own range test against tmax_start, which is the loop's acceptance of a first hit.
PT_HD bool walk_wins(bool is_box, int32_t i, double t, int32_t hit, bool hit_is_box, double best) {
    if (hit < 0) return true;
    if (t != best) return t < best;
    return is_box ? (hit_is_box && i < hit) : (hit_is_box || i > hit);
}

// The per-ray FP32 constants of the slot-box tests (ts = 0: a walking ray starts inside the clip bound).
struct WalkRay {
    float ivx, ivy, ivz, aivx, aivy, aivz, nox, noy, noz, tminf;
};
PT_HD WalkRay walk_ray(const ptd::DevFrame &F, const double ro[3], const double rd[3], double tmin) {
    WalkRay w;
    ptk::slab_recips(F.dir_floor, (float)rd[0], (float)rd[1], (float)rd[2], w.ivx, w.ivy, w.ivz);
    w.aivx = __builtin_fabsf(w.ivx); w.aivy = __builtin_fabsf(w.ivy); w.aivz = __builtin_fabsf(w.ivz);
    w.nox = -(float)ro[0] * w.ivx; w.noy = -(float)ro[1] * w.ivy; w.noz = -(float)ro[2] * w.ivz;
    float tminf = (float)tmin;
    tminf -= __builtin_fabsf(tminf) * 1e-2f + 1e-6f;  // a little below tmin
    w.tminf = __builtin_fmaxf(tminf, 0.0f);            // ... and never below 0: an entry parameter's bits then order like it
    return w;
}
PT_HD float walk_tmaxf(double tmax) {  // >= tmax
    float f = (float)tmax;
    return f + __builtin_fabsf(f) * 4.8e-7f;
}
// Slot s of a node against the ray in [tminf, tmaxf]: slab parameters from centre and half extent (PT_BOX_SLABS); fmaxf / fminf
// return the other operand for a NaN, so a NaN slab (0 * inf) constrains nothing.  t0 = the entry parameter.
PT_HD bool walk_slab(const ptd::BvhNode &nd, int s, const WalkRay &w, float tmaxf, float &t0) {
    const float tcx = __builtin_fmaf(nd.c[0][s], w.ivx, w.nox), tcy = __builtin_fmaf(nd.c[1][s], w.ivy, w.noy),
                tcz = __builtin_fmaf(nd.c[2][s], w.ivz, w.noz);
    t0 = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaf(-nd.h[0][s], w.aivx, tcx), __builtin_fmaf(-nd.h[1][s], w.aivy, tcy)),
                         __builtin_fmaxf(__builtin_fmaf(-nd.h[2][s], w.aivz, tcz), w.tminf));
    const float t1 = __builtin_fminf(__builtin_fminf(__builtin_fmaf(nd.h[0][s], w.aivx, tcx), __builtin_fmaf(nd.h[1][s], w.aivy, tcy)),
                                     __builtin_fminf(__builtin_fmaf(nd.h[2][s], w.aivz, tcz), tmaxf));
    return !(t1 < t0);
}

PT_HD uint32_t walk_float_bits(float f) { return __builtin_bit_cast(uint32_t, f); }
PT_HD void walk_order2(uint32_t &a, uint32_t &b) {
    const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
    a = lo;
    b = hi;
}

// ptg::closest by a walk of the tree.  stack: this lane's entries, `stride` apart.  visits / deep: node visits and deepest stack.
PT_HD int32_t walk_closest(const GlObj *objs, const ptd::DevFrame &F, const ptd::BvhNode *nodes, const ptd::BvhObj *bobjs,
                           const int32_t *plane_idx, int *stack, int stride, const double ro[3], const double rd[3], double tmin,
                           double tmax_start, int32_t skip, double &t_hit, uint32_t &visits, uint32_t &deep) {
    double best = tmax_start;
    int32_t hit = -1;
    bool hit_is_box = false;
    // ---- planes: infinite, outside the tree, always tested exactly
    for (int k = 0; k < F.n_plane; k++) {
        const int32_t i = plane_idx[k];
        double t;
        if (i != skip && hit_t(objs[i], ro, rd, tmin, tmax_start, t) && walk_wins(false, i, t, hit, hit_is_box, best)) {
            best = t;
            hit = i;
            hit_is_box = false;
        }
    }
    if (F.bvh_root >= 0) {
        const WalkRay w = walk_ray(F, ro, rd, tmin);
        float tmaxf = walk_tmaxf(best);
        int sp = 0;
        int cur = F.bvh_root;
        while (cur >= 0) {
            visits++;
            const ptd::BvhNode &nd = nodes[cur];
            const uint32_t meta = nd.meta;
            const int nbase = nd.node_base, obase = nd.obj_base;
            uint32_t key[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
#pragma unroll
            for (int s = 0; s < 4; s++) {
                const bool is_node = (meta >> (8 + s)) & 1u, is_obj = (meta >> (12 + s)) & 1u;
                if (!(is_node || is_obj)) continue;  // empty slot
                float t0;
                if (!walk_slab(nd, s, w, tmaxf, t0)) continue;
                if (is_node) {  // nearest first: the entry parameter's bits (>= 0) with the slot in the low two
                    key[s] = (walk_float_bits(t0) & ~3u) | (uint32_t)s;
                    continue;
                }
                const int32_t i = bobjs[obase + (int)((meta >> (2 * s)) & 3u)].index;
                const GlObj &o = objs[i];
                const bool is_box = o.type == GT_BOX;
                double t;
                if (i != skip && hit_t(o, ro, rd, tmin, tmax_start, t) && walk_wins(is_box, i, t, hit, hit_is_box, best)) {
                    best = t;
                    hit = i;
                    hit_is_box = is_box;
                    tmaxf = walk_tmaxf(best);
                }
            }
            // the pierced internal children sorted by entry (5-exchange network); the farther ones wait on the stack
            walk_order2(key[0], key[1]);
            walk_order2(key[2], key[3]);
            walk_order2(key[0], key[2]);
            walk_order2(key[1], key[3]);
            walk_order2(key[1], key[2]);
#pragma unroll
            for (int q = 3; q >= 1; q--)
                if (key[q] != 0xffffffffu) {
                    stack[sp * stride] = nbase + (int)((meta >> (2 * (key[q] & 3u))) & 3u);
                    sp++;
                }
            if ((uint32_t)sp > deep) deep = (uint32_t)sp;
            if (key[0] != 0xffffffffu) {
                cur = nbase + (int)((meta >> (2 * (key[0] & 3u))) & 3u);
            } else if (sp > 0) {
                sp--;
                cur = stack[sp * stride];
            } else {
                cur = -1;
            }
        }
    }
    t_hit = best;
    return hit;
}

// ptg::occluded by a walk of the tree: an OR over a fixed interval, so there is no order and no winner.
PT_HD bool walk_occluded(const GlObj *objs, const ptd::DevFrame &F, const ptd::BvhNode *nodes, const ptd::BvhObj *bobjs,
                         const int32_t *plane_idx, int *stack, int stride, const double ro[3], const double rd[3], double tmax,
                         uint32_t &visits, uint32_t &deep) {
    const double tmin = 0.001;
    for (int k = 0; k < F.n_plane; k++) {
        double t;
        if (hit_t(objs[plane_idx[k]], ro, rd, tmin, tmax, t)) return true;
    }
    if (F.bvh_root < 0) return false;
    const WalkRay w = walk_ray(F, ro, rd, tmin);
    // tmaxf >= tmax for every tmax >= tmin, where floats are normal; below tmin the exact tests accept nothing
    const float tmaxf = walk_tmaxf(tmax);
    int sp = 0;
    int cur = F.bvh_root;
    while (cur >= 0) {
        visits++;
        const ptd::BvhNode &nd = nodes[cur];
        const uint32_t meta = nd.meta;
        const int nbase = nd.node_base, obase = nd.obj_base;
        int next = -1;
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const bool is_node = (meta >> (8 + s)) & 1u, is_obj = (meta >> (12 + s)) & 1u;
            if (!(is_node || is_obj)) continue;
            float t0;
            if (!walk_slab(nd, s, w, tmaxf, t0)) continue;
            const int rank = (int)((meta >> (2 * s)) & 3u);
            if (is_node) {
                if (next < 0) {
                    next = nbase + rank;
                } else {
                    stack[sp * stride] = nbase + rank;
                    sp++;
                }
            } else {
                double t;
                if (hit_t(objs[bobjs[obase + rank].index], ro, rd, tmin, tmax, t)) return true;
            }
        }
        if ((uint32_t)sp > deep) deep = (uint32_t)sp;
        if (next >= 0) {
            cur = next;
        } else if (sp > 0) {
            sp--;
            cur = stack[sp * stride];
        } else {
            cur = -1;
        }
    }
    return false;
}

// The tree policy of ray_color / gl_pass (LinearWorld's twin): a query whose ray may walk (walk_ok) walks, any other takes the
// plain loop; decided per lane and per query, counted in wc.
struct TreeWorld {
    const GlObj *objs;
    int32_t nobj;
    const ptd::DevFrame &F;  // bvh_root, n_plane, clip_bound, origin_bound, dir_floor
    const ptd::BvhNode *nodes;
    const ptd::BvhObj *bobjs;
    const int32_t *plane_idx;
    int *stack;              // this lane's stack: F.bvh_stack entries, `stride` apart
    int stride;
    WalkCount &wc;
    PT_HD int32_t closest(const double ro[3], const double rd[3], double tmin, double tmax_start, int32_t skip, double &t_hit) const {
        if (walk_ok(F, ro, rd)) {
            wc.closest_walked++;
            return walk_closest(objs, F, nodes, bobjs, plane_idx, stack, stride, ro, rd, tmin, tmax_start, skip, t_hit, wc.closest_visits,
                                wc.deepest);
        }
        wc.closest_plain++;
        return ptg::closest(objs, nobj, ro, rd, tmin, tmax_start, skip, t_hit);
    }
    PT_HD bool occluded(const double ro[3], const double rd[3], double tmax) const {
        if (walk_ok(F, ro, rd)) {
            wc.shadow_walked++;
            return walk_occluded(objs, F, nodes, bobjs, plane_idx, stack, stride, ro, rd, tmax, wc.shadow_visits, wc.deepest);
        }
        wc.shadow_plain++;
        return ptg::occluded(objs, nobj, ro, rd, tmax);
    }
};

// (host only) May this scene's GL objects be found through its main tree?  O(objects).  `scene_objs` are the caller's objects (GL index =
// scene index), `gl` their GL form; nodes[0 .. main_nodes) and bobjs[0 .. main_objs) the main tree as the devices hold it.
//   * no object of unknown type: GL makes those spheres, the device world drops them, and the tree's indices would shift;
//   * every GL sphere or box is an object slot of the main tree exactly once, its GL extent (sphere: pos +- |size[0]|; box:
//     [bmin, bmax]) inside that slot's box [c - h, c + h]; a box with bmin >= bmax on some axis can never be hit (hit_box_t's
//     t1 <= t0) and its extent is not asked for;
//   * every GL plane is in the plane list.
// On failure `why` names the object and the rule.
inline bool walk_scene_check(const pt_object *scene_objs, int32_t nobj, const GlObj *gl, const ptd::BvhNode *nodes, int32_t main_nodes,
                             const ptd::BvhObj *bobjs, int32_t main_objs, const int32_t *plane_idx, int32_t n_plane, std::string &why) {
    auto fail = [&](int32_t i, const char *rule) {
        why = "object " + std::to_string(i) + " " + rule;
        return false;
    };
    for (int32_t i = 0; i < nobj; i++) {
        const int32_t ty = scene_objs[i].type;
        if (!(ty == PT_OBJ_SPHERE || ty == PT_OBJ_SPHERE_LIGHT || ty == PT_OBJ_PLANE || ty == PT_OBJ_BOX))
            return fail(i, "is of unknown type (GL shading draws it as a sphere, the hierarchy does not hold it)");
    }
    std::vector<int32_t> seen((size_t)(nobj > 0 ? nobj : 0), 0);
    for (int32_t k = 0; k < n_plane; k++) {
        const int32_t i = plane_idx[k];
        if (i < 0 || i >= nobj || gl[i].type != GT_PLANE) return fail(i, "is in the plane list and is no GL plane");
        seen[(size_t)i]++;
    }
    for (int32_t q = 0; q < main_nodes; q++) {
        const ptd::BvhNode &nd = nodes[q];
        for (int s = 0; s < 4; s++) {
            if (!((nd.meta >> (12 + s)) & 1u)) continue;
            const int32_t k = nd.obj_base + (int32_t)((nd.meta >> (2 * s)) & 3u);
            if (k < 0 || k >= main_objs) return fail(-1, "(a slot of the hierarchy points outside its object array)");
            const int32_t i = bobjs[k].index;
            if (i < 0 || i >= nobj || gl[i].type == GT_PLANE) return fail(i, "is in the hierarchy and is no GL sphere or box");
            seen[(size_t)i]++;
            const GlObj &o = gl[i];
            double lo[3], hi[3];
            bool empty = false;
            for (int a = 0; a < 3; a++) {
                if (o.type == GT_SPHERE) {
                    lo[a] = o.pos[a] - ptm::f_abs(o.size[0]);
                    hi[a] = o.pos[a] + ptm::f_abs(o.size[0]);
                } else {
                    lo[a] = o.bmin[a];
                    hi[a] = o.bmax[a];
                    empty = empty || o.bmin[a] >= o.bmax[a];
                }
            }
            if (empty) continue;
            for (int a = 0; a < 3; a++)
                if (!(ptd::bvh_slot_lo(nd, a, s) <= lo[a] && hi[a] <= ptd::bvh_slot_hi(nd, a, s)))
                    return fail(i, "has a GL extent outside its slot's box in the hierarchy");
        }
    }
    for (int32_t i = 0; i < nobj; i++)
        if (seen[(size_t)i] != 1)
            return fail(i, gl[i].type == GT_PLANE ? "is a GL plane and not in the plane list exactly once"
                                                  : "is not an object slot of the hierarchy exactly once");
    return true;
}

}  // namespace ptg
