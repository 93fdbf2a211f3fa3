// pt_bvh.h -- host-side BVH builder for scenes beyond the candidate bitmasks (more than 128 spheres or boxes).
//
// The reference scans every object for every ray segment (renderer.go:297-302).  Its winner is
// an order-free function of the per-object hit distances (see `wins` in pt_kernels.h), so any
// structure that never skips an object the exact test would accept returns the same winner.  The
// hierarchy stores FP32 boxes inflated by the same margin as the flat broad phase and rounded
// outward; the exact FP64 tests run only on objects whose own FP32 box the ray pierces.
//
// Build: binned-SAH binary tree down to single objects, then collapsed into 4-wide nodes (the
// child with the largest box is replaced by its two children until the node has four).  A slot
// of a wide node is an internal node, one object, or empty.  Nodes are numbered breadth-first, so
// the internal children of a node are consecutive (node_base + rank), its object children are
// consecutive in the object array (obj_base + rank), and the top of the tree is one prefix that
// the kernel stages in LDS.
//
// The bits of a slot's box -- inflate, centre, half extent rounded up, payload byte -- are stated once, in pt_bvh_refit.h, and
// called from here: a slot's box is a pure function of the objects beneath it, so when only positions and sizes changed the devices
// recompute the boxes of this topology themselves (pt_set_bvh_refit).  build() keeps the level table for that
// (Built::level_start), build_scene_trees() makes the two trees a render uses, and refit() is the host restatement of what the
// device kernels do.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "pt_bvh_build.h"
#include "pt_bvh_refit.h"
#include "pt_device.h"

namespace ptbvh {

using namespace ptd;

constexpr int WIDTH = 4;

struct Aabb {
    double lo[3], hi[3];
    void reset() {
        for (int k = 0; k < 3; k++) { lo[k] = INFINITY; hi[k] = -INFINITY; }
    }
    void grow(const Aabb &o) {
        for (int k = 0; k < 3; k++) { lo[k] = std::min(lo[k], o.lo[k]); hi[k] = std::max(hi[k], o.hi[k]); }
    }
    double area() const {
        const double dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
        if (!(dx >= 0 && dy >= 0 && dz >= 0)) return 0;
        return 2 * (dx * dy + dy * dz + dz * dx);
    }
};

inline Aabb object_bounds(const DevObj &o) {  // (the one definition is ptrf::object_box: the device refit computes the same)
    const ptrf::Box x = ptrf::object_box(o);
    Aabb b;
    for (int k = 0; k < 3; k++) { b.lo[k] = x.lo[k]; b.hi[k] = x.hi[k]; }
    return b;
}

struct Built {
    std::vector<BvhNode> nodes;      // nodes[0] is the root (present whenever there is an object)
    std::vector<int32_t> order;      // object slot -> index into the world array
    int depth = 0;                   // levels of wide nodes
    int stack_need = 0;              // most internal-node entries a traversal can have pushed at once
    std::vector<int32_t> level_start;  // [depth + 1] first node of every level of wide nodes (breadth-first numbering), then nodes.size()
};

namespace detail {

inline float down(double v) {
    float f = (float)v;
    if ((double)f > v) f = std::nextafterf(f, -INFINITY);
    return f;
}
inline float up(double v) {
    float f = (float)v;
    if ((double)f < v) f = std::nextafterf(f, INFINITY);
    return f;
}

struct BinNode {
    Aabb box;
    int32_t left = -1, right = -1;  // both -1: leaf
    int32_t obj = -1;               // leaf: world index
};

struct Builder {
    const std::vector<Aabb> &bounds;
    std::vector<double> cx[3];
    std::vector<int32_t> idx;       // working permutation of the object list
    std::vector<BinNode> bin;
    double margin;

    // chooses the split position inside [a, b): binned SAH (32 bins: 5 % fewer node visits per ray than 16 on the synthetic scenes, tools/bvh_quality.cpp) over each centroid axis, the cheapest of the
    // three wins; median of the widest axis when no bin boundary separates the objects
    int split(int a, int b) {
        Aabb cb;
        cb.reset();
        for (int i = a; i < b; i++)
            for (int k = 0; k < 3; k++) {
                const double c = cx[k][(size_t)idx[(size_t)i]];
                cb.lo[k] = std::min(cb.lo[k], c);
                cb.hi[k] = std::max(cb.hi[k], c);
            }
        int wide = 0;
        double ext = -1;
        for (int k = 0; k < 3; k++) {
            const double e = cb.hi[k] - cb.lo[k];
            if (e == e && e > ext && std::isfinite(e)) { ext = e; wide = k; }
        }
        const int mid = (a + b) / 2;
        if (!(ext > 0)) return mid;  // all centroids coincide (or are not finite): any split is as good
        constexpr int NB = 32;
        double best = INFINITY;
        int best_bin = -1, best_axis = -1;
        double best_scale = 0;
        for (int axis = 0; axis < 3; axis++) {
            const double e = cb.hi[axis] - cb.lo[axis];
            if (!(e > 0) || !std::isfinite(e)) continue;
            Aabb bb[NB];
            int cnt[NB];
            for (int i = 0; i < NB; i++) { bb[i].reset(); cnt[i] = 0; }
            const double scale = NB / e;
            for (int i = a; i < b; i++) {
                const int32_t o = idx[(size_t)i];
                const int q = std::max(0, std::min(NB - 1, (int)((cx[axis][(size_t)o] - cb.lo[axis]) * scale)));
                bb[q].grow(bounds[(size_t)o]);
                cnt[q]++;
            }
            Aabb right[NB];
            int rc[NB];
            Aabb acc;
            acc.reset();
            int n = 0;
            for (int i = NB - 1; i >= 0; i--) { acc.grow(bb[i]); n += cnt[i]; right[i] = acc; rc[i] = n; }
            acc.reset();
            n = 0;
            for (int i = 0; i + 1 < NB; i++) {
                acc.grow(bb[i]);
                n += cnt[i];
                if (n == 0 || rc[i + 1] == 0) continue;
                const double cost = acc.area() * n + right[i + 1].area() * rc[i + 1];
                if (cost < best) { best = cost; best_bin = i; best_axis = axis; best_scale = scale; }
            }
        }
        int m = mid;
        if (best_bin >= 0 && std::isfinite(best)) {
            const double lo = cb.lo[best_axis];
            auto it = std::partition(idx.begin() + a, idx.begin() + b, [&](int32_t o) {
                return std::max(0, std::min(NB - 1, (int)((cx[best_axis][(size_t)o] - lo) * best_scale))) <= best_bin;
            });
            m = (int)(it - idx.begin());
        }
        if (m <= a || m >= b) {
            std::nth_element(idx.begin() + a, idx.begin() + mid, idx.begin() + b,
                             [&](int32_t u, int32_t v) { return cx[wide][(size_t)u] < cx[wide][(size_t)v]; });
            m = mid;
        }
        return m;
    }

    // binary tree over idx[a, b); returns its node.  Below `sah_levels` levels the split is the median of the
    // object list (whatever SAH would like): a scene that makes SAH peel off one object per level
    // (geometrically spaced objects) must not drive the recursion or the traversal stack to depth n.
    int sah_levels = 40;
    int32_t build(int a, int b, int level = 0) {
        const int32_t me = (int32_t)bin.size();
        bin.emplace_back();
        if (b - a == 1) {
            bin[(size_t)me].obj = idx[(size_t)a];
            bin[(size_t)me].box = bounds[(size_t)idx[(size_t)a]];
            return me;
        }
        const int m = level < sah_levels ? split(a, b) : (a + b) / 2;
        const int32_t l = build(a, m, level + 1);
        const int32_t r = build(m, b, level + 1);
        BinNode &nd = bin[(size_t)me];
        nd.left = l;
        nd.right = r;
        nd.box = bin[(size_t)l].box;
        nd.box.grow(bin[(size_t)r].box);
        return me;
    }

    // the (up to WIDTH) binary nodes that become the slots of the wide node made from binary node b: the rule is stated once, in
    // pt_bvh_build.h (ptbb::gather4), for this builder and for the device build
    bool leaf(int32_t b) const { return bin[(size_t)b].obj >= 0; }
    int32_t left(int32_t b) const { return bin[(size_t)b].left; }
    int32_t right(int32_t b) const { return bin[(size_t)b].right; }
    double area(int32_t b) const { return bin[(size_t)b].box.area(); }
    int32_t object(int32_t b) const { return bin[(size_t)b].obj; }
    void box6(int32_t b, double out[6]) const {
        for (int k = 0; k < 3; k++) { out[k] = bin[(size_t)b].box.lo[k]; out[3 + k] = bin[(size_t)b].box.hi[k]; }
    }
    int gather(int32_t b, int32_t out[WIDTH]) const { return ptbb::gather4(*this, b, out); }
};

}  // namespace detail

// deepest stack of the tree whose nodes are [first, last) of `nodes`, its root `first` (children carry larger numbers than their
// parents): a node with k internal children leaves at most k-1 entries below the subtree being walked
inline int stack_need_of(const std::vector<BvhNode> &nodes, size_t first, size_t last) {
    if (last <= first) return 0;
    std::vector<int32_t> need(last - first, 0);
    for (size_t q = last; q-- > first;) {
        const BvhNode &nd = nodes[q];
        const int k = __builtin_popcount((nd.meta >> 8) & 0xfu);
        int deepest = 0;
        for (int c = 0; c < k; c++) deepest = std::max(deepest, need[(size_t)(nd.node_base + c) - first]);
        need[q - first] = k > 0 ? (k - 1) + deepest : 0;
    }
    return need[0];
}

// `finite` lists the world indices of the spheres and boxes (planes stay outside the tree).
inline Built build(const std::vector<DevObj> &world, const std::vector<int32_t> &finite, double margin, int sah_levels = 40) {
    Built out;
    const int n = (int)finite.size();
    if (n == 0) return out;  // no finite objects: the kernel skips the traversal
    std::vector<Aabb> bounds(world.size());
    detail::Builder bl{bounds, {}, finite, {}, margin};
    for (int k = 0; k < 3; k++) bl.cx[k].assign(world.size(), 0.0);
    for (int32_t i : finite) {
        bounds[(size_t)i] = object_bounds(world[(size_t)i]);
        for (int k = 0; k < 3; k++) {
            double c = 0.5 * (bounds[(size_t)i].lo[k] + bounds[(size_t)i].hi[k]);
            if (!std::isfinite(c)) c = 0;
            bl.cx[k][(size_t)i] = c;
        }
    }
    bl.sah_levels = sah_levels;
    bl.bin.reserve((size_t)2 * n);
    const int32_t root = bl.build(0, n);

    // breadth-first collapse into wide nodes: stated once, in pt_bvh_build.h, for this builder and for the device build's restatement
    out.order.reserve((size_t)n);
    ptbb::collapse(bl, root, world.data(), margin, 0, 0, false, out.nodes, out.order, out.level_start);
    out.depth = (int)out.level_start.size() - 1;
    out.stack_need = stack_need_of(out.nodes, 0, out.nodes.size());
    return out;
}

// The certain core of an object (pt_walk32.h): a box every point of which lies inside the object by the margin m.  A ray
// that passes through it is hit by the reference's FP64 test of the object (objects.go:37-61, :141-179) no later than where
// it enters the core: the FP32 slab arithmetic of the walk is off by <= 1.2e-6 B in position, two orders of magnitude less
// than m = B / 4096.
//   box     [min + m, max - m]; only a proper box (min < max on every axis: anything else the slab test never hits)
//   sphere  the cube of half side (|r| - m) / sqrt(3) about the centre (the reference squares the radius: its sign is irrelevant)
// Returns false when the object has no core (thinner than 2 m, degenerate, not finite).
inline bool object_core(const DevObj &o, double m, double lo[3], double hi[3]) {
    if (!(m > 0) || !std::isfinite(m)) return false;
    const int kind = o.kind & 0xff;
    if (kind == KIND_SPHERE) {
        const double r = std::fabs(o.radius);
        const double q = (r - m) * 0.57735026 * (1.0 - 1e-9);
        if (!(q > 0.25 * m) || !std::isfinite(q)) return false;
        for (int k = 0; k < 3; k++) { lo[k] = o.a[k] - q; hi[k] = o.a[k] + q; }
    } else if (kind == KIND_BOX) {
        for (int k = 0; k < 3; k++) {
            if (!(o.a[k] < o.b[k])) return false;
            lo[k] = o.a[k] + m;
            hi[k] = o.b[k] - m;
            if (!(hi[k] - lo[k] > 0.5 * m)) return false;
        }
    } else {
        return false;
    }
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(lo[k]) || !std::isfinite(hi[k])) return false;
    return true;
}

// Core twins of the nodes of `b`: twin q holds, in slot s, a box INSIDE the core of the object in slot s of node q, as FP32
// centre / half extent rounded INWARD (meta bits 12-15: the slot has a core; no internal slots).  Also marks in the NODE's
// meta (bits 20-23) which object slots have a core.
inline std::vector<BvhNode> build_cores(Built &b, const std::vector<DevObj> &world, double margin) {
    std::vector<BvhNode> cores(b.nodes.size());
    for (size_t q = 0; q < b.nodes.size(); q++) {
        BvhNode &nd = b.nodes[q];
        BvhNode tw;
        std::memset(&tw, 0, sizeof tw);
        uint32_t has = 0;
        for (int s = 0; s < WIDTH; s++) {
            for (int k = 0; k < 3; k++) { tw.c[k][s] = 3.0e38f; tw.h[k][s] = 0.0f; }
            if (!((nd.meta >> (12 + s)) & 1u)) continue;
            const int32_t oi = b.order[(size_t)(nd.obj_base + (int)((nd.meta >> (2 * s)) & 3u))];
            double lo[3], hi[3];
            if (!object_core(world[(size_t)oi], margin, lo, hi)) continue;
            float c[3], h[3];
            bool ok = true;
            for (int k = 0; k < 3; k++) {
                const float cf = (float)(0.5 * lo[k] + 0.5 * hi[k]);
                const double g = std::min((double)cf - lo[k], hi[k] - (double)cf);  // [cf - g, cf + g] lies inside [lo, hi]
                // cf - hf and cf + hf are formed in FP32 by the walk (c*iv - h*|iv|): keep two more ulps of the larger magnitude clear
                const float hf = detail::down(g - 2.0 * 1.1920929e-7 * (std::fabs((double)cf) + std::fabs(g)));
                ok = ok && hf > 0 && std::isfinite(cf) && std::isfinite(hf);
                c[k] = cf;
                h[k] = hf;
            }
            if (!ok) continue;
            for (int k = 0; k < 3; k++) { tw.c[k][s] = c[k]; tw.h[k][s] = h[k]; }
            has |= 1u << s;
        }
        tw.meta = has << 12;
        nd.meta = (nd.meta & ~(0xfu << 20)) | (has << 20);
        cores[q] = tw;
    }
    return cores;
}

// ---------------------------------------------------------------- the two trees of a scene, and their refit

// The hierarchy a scene on the BVH path renders with: the tree of every finite object, then the tree of the dielectric ones,
// appended in both arrays, with scene_prepare's payload bytes in place.
struct SceneTrees {
    std::vector<BvhNode> nodes;
    std::vector<BvhObj> objs;
    std::vector<BvhNode> cores;         // walk32 only
    std::vector<int32_t> level_start;   // first node of every level of the main tree, then of the dielectric tree, then nodes.size()
    int depth = 0, stack_need = 0;
    int32_t main_nodes = 0, main_objs = 0;
    int32_t root = -1, root_exit = -1;
    double margin = 0.0;
};

// the inflation of the hierarchy's boxes: 2^-12 of the bound of every finite object's coordinates
inline double scene_margin(const std::vector<DevObj> &w) {
    double Bnd = 1.0;
    for (size_t i = 0; i < w.size(); i++) {
        if ((w[i].kind & 0xff) == KIND_PLANE) continue;
        const Aabb bb = object_bounds(w[i]);
        for (int k = 0; k < 3; k++) Bnd = std::max(Bnd, std::max(std::fabs(bb.lo[k]), std::fabs(bb.hi[k])));
    }
    if (!(Bnd < 1e30)) Bnd = INFINITY;
    return Bnd * (1.0 / 4096.0);
}

// B bounds every finite object's coordinates (scene_prepare's build_broad; a host build of a walk takes it from here too).
inline double world_bound(const std::vector<DevObj> &world) {
    double B = 1.0;
    for (const DevObj &o : world) {
        const int kind = o.kind & 0xff;
        if (kind == KIND_SPHERE) {
            for (int k = 0; k < 3; k++) B = std::max(B, std::fabs(o.a[k]) + std::fabs(o.radius));
        } else if (kind == KIND_BOX) {
            for (int k = 0; k < 3; k++) B = std::max(B, std::max(std::fabs(o.a[k]), std::fabs(o.b[k])));
        }
    }
    if (!(B < 1e30)) B = INFINITY;  // absurd or non-finite geometry: every object stays a candidate
    return B;
}
// ... and the fields of DevFrame the FP32 tests derive from it.
inline void frame_bounds(double B, DevFrame &F) {
    F.origin_bound = (float)std::min(4.0 * B, 3.0e38);
    // With |1/d| (4 origin_bound) < 3e38 no product of a slab test (a centre, a half extent or an origin within origin_bound times
    // 1/d) leaves the finite range, nor does their sum.  A smaller component is taken for zero, whose slab constrains nothing (the
    // walks of the hierarchy, the grouped scan), or the ray keeps every box (the scan of at most 32 records): a
    // product past FLT_MAX is an INFINITY, not a NaN, and tf = -inf culled boxes the ray goes through (B = 8: 4.3e-37; from
    // B = 2^61 on a component of 2^-60 is below it; in the keep-everything band every component is).
    F.dir_floor = detail::up(4.0 * (double)F.origin_bound / 3.0e38);
    F.scene_bound = B * (1.0 + 1.0 / 512.0);  // the inflation is B/4096
    F.clip_bound = B * 3.5;
    F.margin = B * (1.0 / 4096.0);
}

// The walk of scan_bvh reads the first 96 bytes of a node only (six 16-byte requests per lane and visit instead of seven: the
// CU's address unit, not the caches, is what its visits wait for -- DESIGN 10.3): node_base, obj_base and meta ride in the LOW BYTES
// of the twelve half extents, which are rounded up to a multiple of 256 ulp first (they only ever had to be upper bounds).
// The fields themselves stay where they were for everything else that reads a node (host tools, the walk32 form, the refit).
inline void embed_payload(BvhNode &nd) {
    const uint32_t payload[3] = {(uint32_t)nd.node_base, (uint32_t)nd.obj_base, nd.meta & 0xffffffu};
    for (int k = 0; k < 3; k++)
        for (int sl = 0; sl < 4; sl++) nd.h[k][sl] = ptrf::bits_float(ptrf::h_word(nd.h[k][sl], payload[k] >> (8 * sl)));
}

// Builds both trees of `w`.  A tree too deep for a per-lane stack of `stack_limit` entries (adversarial spacing) is rebuilt with
// fewer SAH levels; false when that does not help.
inline bool build_scene_trees(const std::vector<DevObj> &w, bool with_cores, int stack_limit, SceneTrees &T) {
    T = SceneTrees();
    std::vector<int32_t> finite, glass;
    for (size_t i = 0; i < w.size(); i++)
        if ((w[i].kind & 0xff) != KIND_PLANE) finite.push_back((int32_t)i);
    // two hierarchies: every finite object (closest-hit scans) and the dielectric ones only (exit
    // searches accept nothing else, renderer.go:333, and would otherwise walk the whole line of sight)
    for (int32_t i : finite)
        if (w[(size_t)i].kind & 0x100) glass.push_back(i);
    const double margin = scene_margin(w);
    T.margin = margin;
    Built built = build(w, finite, margin);
    Built builtd = build(w, glass, margin);
    for (int lv = 16; built.stack_need >= stack_limit && lv >= 0; lv -= 16) built = build(w, finite, margin, lv);
    for (int lv = 16; builtd.stack_need >= stack_limit && lv >= 0; lv -= 16) builtd = build(w, glass, margin, lv);
    T.depth = std::max(built.depth, builtd.depth);
    T.stack_need = std::max(built.stack_need, builtd.stack_need);
    if (T.stack_need >= stack_limit) return false;
    // core twins (the FP32 walk of pt_walk32.h): inside-the-object boxes of the main tree's object slots; the dielectric
    // tree's twins are empty (an exit search takes no FP32 bound)
    if (with_cores) {
        T.cores = build_cores(built, w, margin);
        T.cores.resize(built.nodes.size() + builtd.nodes.size());
        for (size_t q = built.nodes.size(); q < T.cores.size(); q++) std::memset(&T.cores[q], 0, sizeof(BvhNode));
    }
    const int32_t node_off = (int32_t)built.nodes.size(), obj_off = (int32_t)built.order.size();
    T.main_nodes = node_off;
    T.main_objs = obj_off;
    T.nodes = std::move(built.nodes);
    for (BvhNode nd : builtd.nodes) {  // the dielectric tree follows the main one in both arrays
        nd.node_base += node_off;
        nd.obj_base += obj_off;
        T.nodes.push_back(nd);
    }
    for (BvhNode &nd : T.nodes) embed_payload(nd);
    for (size_t l = 0; l + 1 < built.level_start.size(); l++) T.level_start.push_back(built.level_start[l]);
    for (size_t l = 0; l + 1 < builtd.level_start.size(); l++) T.level_start.push_back(builtd.level_start[l] + node_off);
    T.level_start.push_back((int32_t)T.nodes.size());
    T.objs.resize(built.order.size() + builtd.order.size());
    for (size_t k = 0; k < T.objs.size(); k++) {
        const int32_t oi = k < built.order.size() ? built.order[k] : builtd.order[k - built.order.size()];
        std::memset(&T.objs[k], 0, sizeof(BvhObj));
        T.objs[k].o = w[(size_t)oi];
        T.objs[k].index = oi;
    }
    T.root_exit = builtd.nodes.empty() ? -1 : node_off;
    T.root = T.nodes.empty() || built.order.empty() ? -1 : 0;
    return true;
}

// The same two trees by the Morton-order build of pt_bvh_build.h, restated on the host (the product runs ptbb::build_tree_launch):
// what pt_set_bvh_build(ctx, 1) renders with, byte for byte.  There are no core twins (walk32 builds on the host).  False when
// the tree is too deep for a per-lane stack of `stack_limit` entries: the caller falls back to build_scene_trees.
using ptbb::build_lbvh;
inline void scene_object_lists(const std::vector<DevObj> &w, std::vector<int32_t> &finite, std::vector<int32_t> &glass) {
    finite.clear();
    glass.clear();
    for (size_t i = 0; i < w.size(); i++)
        if ((w[i].kind & 0xff) != KIND_PLANE) finite.push_back((int32_t)i);
    for (int32_t i : finite)
        if (w[(size_t)i].kind & 0x100) glass.push_back(i);
}
// depth, stack_need, the roots and the counts of T from its nodes, order counts and level tables (both builders' last step)
inline bool finish_lbvh_trees(SceneTrees &T, int32_t main_nodes, int32_t main_objs, const std::vector<int32_t> &levels_main,
                              const std::vector<int32_t> &levels_glass, int stack_limit) {
    T.main_nodes = main_nodes;
    T.main_objs = main_objs;
    const int dm = levels_main.empty() ? 0 : (int)levels_main.size() - 1, dg = levels_glass.empty() ? 0 : (int)levels_glass.size() - 1;
    T.depth = std::max(dm, dg);
    T.stack_need = std::max(stack_need_of(T.nodes, 0, (size_t)main_nodes), stack_need_of(T.nodes, (size_t)main_nodes, T.nodes.size()));
    T.level_start.clear();
    for (size_t l = 0; l + 1 < levels_main.size(); l++) T.level_start.push_back(levels_main[l]);
    for (size_t l = 0; l + 1 < levels_glass.size(); l++) T.level_start.push_back(levels_glass[l] + main_nodes);
    T.level_start.push_back((int32_t)T.nodes.size());
    T.root_exit = (size_t)main_nodes == T.nodes.size() ? -1 : main_nodes;
    T.root = T.nodes.empty() || main_objs == 0 ? -1 : 0;
    return T.stack_need < stack_limit;
}
inline bool build_scene_trees_lbvh(const std::vector<DevObj> &w, int stack_limit, SceneTrees &T, ptbb::Lbvh *main_out = nullptr,
                                   ptbb::Lbvh *glass_out = nullptr) {
    T = SceneTrees();
    std::vector<int32_t> finite, glass;
    scene_object_lists(w, finite, glass);
    T.margin = scene_margin(w);
    ptbb::Lbvh A, B;
    build_lbvh(w.data(), finite.data(), (int32_t)finite.size(), T.margin, 0, 0, A);
    build_lbvh(w.data(), glass.data(), (int32_t)glass.size(), T.margin, (int32_t)A.nodes.size(), (int32_t)A.order.size(), B);
    T.nodes = A.nodes;
    T.nodes.insert(T.nodes.end(), B.nodes.begin(), B.nodes.end());
    T.objs.resize(A.order.size() + B.order.size());
    for (size_t k = 0; k < T.objs.size(); k++) {
        const int32_t oi = k < A.order.size() ? A.order[k] : B.order[k - A.order.size()];
        std::memset(&T.objs[k], 0, sizeof(BvhObj));
        T.objs[k].o = w[(size_t)oi];
        T.objs[k].index = oi;
    }
    const bool fits = finish_lbvh_trees(T, (int32_t)A.nodes.size(), (int32_t)A.order.size(), A.level_start, B.level_start, stack_limit);
    if (main_out) *main_out = std::move(A);
    if (glass_out) *glass_out = std::move(B);
    return fits;
}

// The refit, restated on the host (the product runs ptrf::refit_launch): nodes and records of unchanged topology brought to
// `world` and `margin`, level by level from the last to the first.  node_box [n][6] and node_area [n] receive every node's
// exact box and a[q].
inline void refit(std::vector<BvhNode> &nodes, std::vector<BvhObj> &objs, const std::vector<DevObj> &world, double margin,
                  const std::vector<int32_t> &level_start, std::vector<double> &node_box, std::vector<double> &node_area) {
    for (BvhObj &bo : objs) bo.o = world[(size_t)bo.index];
    node_box.assign(nodes.size() * 6, 0.0);
    node_area.assign(nodes.size(), 0.0);
    for (size_t l = level_start.size() - 1; l-- > 0;)
        for (int32_t q = level_start[l]; q < level_start[l + 1]; q++) {
            BvhNode &nd = nodes[(size_t)q];
            ptrf::Box bx[4];
            double area[4];
            for (int s = 0; s < WIDTH; s++) {
                bx[s] = ptrf::empty_box();
                area[s] = 0.0;
                const int rank = ptrf::slot_rank(nd.meta, s);
                if (ptrf::slot_object(nd.meta, s)) {
                    bx[s] = ptrf::object_box(objs[(size_t)(nd.obj_base + rank)].o);
                } else if (ptrf::slot_internal(nd.meta, s)) {
                    const double *p = &node_box[6 * (size_t)(nd.node_base + rank)];
                    for (int k = 0; k < 3; k++) { bx[s].lo[k] = p[k]; bx[s].hi[k] = p[3 + k]; }
                } else {
                    continue;
                }
                ptrf::encode_slot(nd, s, bx[s], margin);
                area[s] = ptrf::half_area(bx[s]);
            }
            ptrf::grow(bx[0], bx[1]);
            ptrf::grow(bx[2], bx[3]);
            ptrf::grow(bx[0], bx[2]);
            for (int k = 0; k < 3; k++) { node_box[6 * (size_t)q + k] = bx[0].lo[k]; node_box[6 * (size_t)q + 3 + k] = bx[0].hi[k]; }
            node_area[(size_t)q] = ((area[0] + area[1]) + area[2]) + area[3];
        }
}

// The invariants of a scene's two trees, whoever built them.  out = {nodes, objects, depth, stack_need, objects not reached exactly
// once, objects not inside their slot's box, child boxes not inside their parent's, structural faults: children or objects not
// consecutive in the breadth-first numbering, a level table that does not increase strictly, a slot count above 4 (by the masks),
// and nodes or records whose bytes a refit to the build's own world changes}.
inline void check_trees(const SceneTrees &T, const std::vector<DevObj> &w, int32_t out[8]) {
    int reached = 0, outside = 0, nested = 0, faults = 0;
    std::vector<int32_t> finite, glass;
    scene_object_lists(w, finite, glass);
    const double held = std::isfinite(T.margin) ? T.margin * 0.999 : 0.0;
    std::vector<ptrf::Box> sub(T.nodes.size());
    for (size_t q = T.nodes.size(); q-- > 0;) {
        const BvhNode &nd = T.nodes[q];
        ptrf::Box all = ptrf::empty_box();
        if (((nd.meta >> 8) & 0xfu) & ((nd.meta >> 12) & 0xfu)) faults++;
        for (int s = 0; s < WIDTH; s++) {
            const int rank = ptrf::slot_rank(nd.meta, s);
            ptrf::Box b;
            const bool is_obj = ptrf::slot_object(nd.meta, s);
            if (is_obj) {
                const size_t k = (size_t)(nd.obj_base + rank);
                if (k >= T.objs.size()) { faults++; continue; }
                b = ptrf::object_box(w[(size_t)T.objs[k].index]);
            } else if (ptrf::slot_internal(nd.meta, s)) {
                const size_t c = (size_t)(nd.node_base + rank);
                if (c <= q || c >= T.nodes.size()) { faults++; continue; }
                b = sub[c];
            } else {
                continue;
            }
            ptrf::grow(all, b);
            for (int k = 0; k < 3; k++)
                if (bvh_slot_lo(nd, k, s) > b.lo[k] - held || bvh_slot_hi(nd, k, s) < b.hi[k] + held) {
                    (is_obj ? outside : nested)++;
                    break;
                }
        }
        sub[q] = all;
    }
    // breadth-first numbering, tree by tree: the children of node q follow those of the nodes before it, and so do its objects
    const size_t first[3] = {0, (size_t)T.main_nodes, T.nodes.size()};
    const int32_t obj_first[3] = {0, T.main_objs, (int32_t)T.objs.size()};
    for (int t = 0; t < 2; t++) {
        int32_t kids = (int32_t)first[t] + 1, objs = obj_first[t];
        for (size_t q = first[t]; q < first[t + 1]; q++) {
            const BvhNode &nd = T.nodes[q];
            if (nd.node_base != kids || nd.obj_base != objs) faults++;
            kids += __builtin_popcount((nd.meta >> 8) & 0xfu);
            objs += __builtin_popcount((nd.meta >> 12) & 0xfu);
        }
        if (first[t] < first[t + 1] && (kids != (int32_t)first[t + 1] || objs != obj_first[t + 1])) faults++;
        std::vector<int32_t> seen(w.size(), 0);
        for (int32_t k = obj_first[t]; k < obj_first[t + 1]; k++) {
            const int32_t oi = T.objs[(size_t)k].index;
            if (oi < 0 || (size_t)oi >= w.size()) reached++;
            else seen[(size_t)oi]++;
        }
        for (int32_t oi : t == 0 ? finite : glass)
            if (seen[(size_t)oi]-- != 1) reached++;
        for (int32_t c : seen)
            if (c > 0) reached++;
    }
    for (size_t l = 0; l + 1 < T.level_start.size(); l++)
        if (T.level_start[l] >= T.level_start[l + 1]) faults++;
    if (!T.nodes.empty() && (T.level_start.empty() || T.level_start.front() != 0 || T.level_start.back() != (int32_t)T.nodes.size())) faults++;
    if (!T.nodes.empty() && !T.level_start.empty()) {
        std::vector<BvhNode> nodes = T.nodes;
        std::vector<BvhObj> objs = T.objs;
        std::vector<double> box, area;
        refit(nodes, objs, w, T.margin, T.level_start, box, area);
        for (size_t q = 0; q < nodes.size(); q++)
            if (std::memcmp(&nodes[q], &T.nodes[q], sizeof(BvhNode)) != 0) faults++;
        for (size_t k = 0; k < objs.size(); k++)
            if (std::memcmp(&objs[k], &T.objs[k], sizeof(BvhObj)) != 0) faults++;
    }
    out[0] = (int32_t)T.nodes.size();
    out[1] = (int32_t)T.objs.size();
    out[2] = T.depth;
    out[3] = T.stack_need;
    out[4] = reached;
    out[5] = outside;
    out[6] = nested;
    out[7] = faults;
}

// Why a scene edit cannot be served by a refit (pt_bvh_refit_stats.last_build_reason; 0: it can).
enum RefitReason { REFIT_OK = 0, REFIT_FIRST = 1, REFIT_OFF = 2, REFIT_CHANGED = 3, REFIT_NOT_BVH = 4, REFIT_GROWTH = 5, REFIT_NONFINITE = 6 };

// A coordinate or a size of 1e37 or more (or none at all: NaN): such a world is on the plain loop and has no tree to refit.
inline bool world_beyond_fp32(const std::vector<DevObj> &w) {
    for (const DevObj &o : w) {
        bool fin = std::fabs(o.radius) < 1e37;
        for (int k = 0; k < 3; k++) fin = fin && std::fabs(o.a[k]) < 1e37 && std::fabs(o.b[k]) < 1e37;
        if (!fin) return true;
    }
    return false;
}

// The scene-side conditions of a refit from `before` to `after` (converted worlds and materials): the same materials, the same
// objects by count, kind (bit 8 included) and material, and every coordinate below 1e37.
inline int refit_reason(const std::vector<DevObj> &before, const std::vector<DevMat> &mats_before, const std::vector<DevObj> &after,
                        const std::vector<DevMat> &mats_after) {
    if (mats_before.size() != mats_after.size() ||
        (!mats_after.empty() && std::memcmp(mats_before.data(), mats_after.data(), mats_after.size() * sizeof(DevMat)) != 0))
        return REFIT_CHANGED;
    if (before.size() != after.size()) return REFIT_CHANGED;
    for (size_t i = 0; i < after.size(); i++)
        if (before[i].kind != after[i].kind || before[i].mat != after[i].mat) return REFIT_CHANGED;
    return world_beyond_fp32(after) ? REFIT_NONFINITE : REFIT_OK;
}

}  // namespace ptbvh
