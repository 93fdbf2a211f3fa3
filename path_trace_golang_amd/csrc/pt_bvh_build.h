// pt_bvh_build.h -- a Morton-order (LBVH) build of the 4-wide hierarchy, stated once for the host and the device.
//
// pt_bvh.h's binned-SAH builder runs on the host, single-threaded.  Any hierarchy whose boxes hold their objects returns the linear
// scan's winner, so a tree of another topology gives the same frame; this file builds one on the device, in the node format, the
// breadth-first numbering and the payload bytes of ptbvh::build_scene_trees, so every walker, the refit and verify_bvh read it as it is.
//
//   1. keys     per object of `finite` (in that order): the exact box (ptrf::object_box), its centroid 0.5 (lo + hi) (0 where that is
//               not finite); min / max of the centroids per axis (exact, order-free); one scale per axis 2^21 / extent, computed once
//               (0 where the extent is not positive and finite, and where the quotient is not finite: a denormal extent); per object
//               q = clamp((c - cmin) * scale, 0, 2^21 - 1) truncated, the three q interleaved into 63 bits (x highest).
//   2. sort     a stable 8-bit LSD radix sort of (key, position in `finite`): equal keys stay in position order, so the order is a
//               function of the scene alone.  Per pass: digit histogram per tile, exclusive scan, stable scatter.
//   3. tree     Karras' binary radix tree over the sorted keys, one lane per internal node; equal keys compare by sorted position
//               (delta = 64 + clz(i ^ j)), so n equal keys give a balanced subtree.  Internal node i has id i, sorted leaf k has id
//               n - 1 + k; node 0 is the root (a tree of one object is its leaf).
//   4. boxes    bottom-up with one visit counter per internal node: the first arrival leaves, the second unions left then right
//               (min / max) and goes up.  No lane waits for another.
//   5. collapse to 4-wide nodes, top-down, one level per round: the gather rule of ptbvh::build (open the internal slot of the largest
//               area until four slots are filled; NaN counts as infinite; the first of equals wins), an exclusive scan of the internal
//               and object children gives node_base / obj_base, and a quad of lanes writes each node, the next level's list and
//               `order`.  The level's totals (8 bytes) are read back to size the next round.
//   6. the second tree (the dielectric objects) is built the same way behind the first, with node_base / obj_base offset; the
//               payload bytes are written with the node; the records are filled from `order`.
//
// Only + - x, three divisions done once, comparisons, conversions and integer work: the host restatement (build_lbvh below) and
// the kernels agree byte for byte.  Compiled with -ffp-contract=off like the other shared headers.  There is no spin loop in the build.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "pt_bvh_refit.h"
#include "pt_device.h"

namespace ptbb {

using namespace ptd;
using ptrf::Box;

constexpr int KEY_BITS = 21;                 // per axis
constexpr int SORT_PASSES = 8;               // 8-bit digits of the 63-bit key
constexpr int SORT_TILE = 1024;              // keys one wave ranks per pass, 64 at a time
constexpr int SCAN_TILE = 1024;              // elements one block of 256 scans
constexpr int RED_TILE = 1024;               // centroids one block of 256 reduces

PT_HOST_DEVICE inline bool finite_d(double v) {
    uint64_t b;
    __builtin_memcpy(&b, &v, 8);
    return (b & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// ---------------------------------------------------------------- 1. keys
PT_HOST_DEVICE inline void centroid(const Box &b, double c[3]) {
    for (int k = 0; k < 3; k++) {
        c[k] = 0.5 * (b.lo[k] + b.hi[k]);
        if (!finite_d(c[k])) c[k] = 0.0;
    }
}
PT_HOST_DEVICE inline double key_scale(double cmin, double cmax) {
    const double e = cmax - cmin;
    if (!(e > 0.0) || !finite_d(e)) return 0.0;
    const double s = 2097152.0 / e;
    return finite_d(s) ? s : 0.0;
}
PT_HOST_DEVICE inline uint32_t quantise(double c, double cmin, double scale) {
    const double t = (c - cmin) * scale;
    if (!(t > 0.0)) return 0u;  // (also NaN)
    if (t >= 2097151.0) return 2097151u;
    return (uint32_t)(int64_t)t;
}
PT_HOST_DEVICE inline uint64_t spread21(uint64_t v) {  // bit i of v to bit 3 i
    v &= 0x1fffffull;
    v = (v | v << 32) & 0x1f00000000ffffull;
    v = (v | v << 16) & 0x1f0000ff0000ffull;
    v = (v | v << 8) & 0x100f00f00f00f00full;
    v = (v | v << 4) & 0x10c30c30c30c30c3ull;
    v = (v | v << 2) & 0x1249249249249249ull;
    return v;
}
PT_HOST_DEVICE inline uint64_t morton(uint32_t qx, uint32_t qy, uint32_t qz) { return spread21(qx) << 2 | spread21(qy) << 1 | spread21(qz); }
PT_HOST_DEVICE inline uint64_t object_key(const DevObj &o, const double cmin[3], const double scale[3]) {
    double c[3];
    centroid(ptrf::object_box(o), c);
    return morton(quantise(c[0], cmin[0], scale[0]), quantise(c[1], cmin[1], scale[1]), quantise(c[2], cmin[2], scale[2]));
}

// ---------------------------------------------------------------- 3. the binary radix tree
// length of the common prefix of sorted entries i and j (-1 outside the array); equal keys go on with the positions
PT_HOST_DEVICE inline int prefix_len(const uint64_t *keys, int32_t n, int64_t i, int64_t j) {
    if (j < 0 || j >= (int64_t)n) return -1;
    const uint64_t a = keys[i], b = keys[j];
    if (a != b) return __builtin_clzll(a ^ b);
    return 64 + __builtin_clz((uint32_t)i ^ (uint32_t)j);  // (i != j)
}
PT_HOST_DEVICE inline int32_t leaf_id(int32_t n, int32_t k) { return n - 1 + k; }
PT_HOST_DEVICE inline bool is_leaf(int32_t n, int32_t id) { return id >= n - 1; }
// children of internal node i of n >= 2 sorted keys
PT_HOST_DEVICE inline void radix_node(const uint64_t *keys, int32_t n, int32_t i, int32_t &left, int32_t &right) {
    const int64_t d = prefix_len(keys, n, i, (int64_t)i + 1) > prefix_len(keys, n, i, (int64_t)i - 1) ? 1 : -1;
    const int dmin = prefix_len(keys, n, i, i - d);
    int64_t lmax = 2;
    while (prefix_len(keys, n, i, i + lmax * d) > dmin) lmax *= 2;
    int64_t l = 0;
    for (int64_t t = lmax / 2; t >= 1; t /= 2)
        if (prefix_len(keys, n, i, i + (l + t) * d) > dmin) l += t;
    const int64_t j = i + l * d;
    const int dnode = prefix_len(keys, n, i, j);
    int64_t s = 0, t = l;
    do {
        t = (t + 1) >> 1;
        if (prefix_len(keys, n, i, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    const int64_t g = i + s * d + (d < 0 ? -1 : 0);
    const int64_t lo = i < j ? i : j, hi = i < j ? j : i;
    left = lo == g ? leaf_id(n, (int32_t)g) : (int32_t)g;
    right = hi == g + 1 ? leaf_id(n, (int32_t)(g + 1)) : (int32_t)(g + 1);
}

// ---------------------------------------------------------------- 5. the collapse
// ptbvh::Aabb::area
PT_HOST_DEVICE inline double box_area(const double *lo, const double *hi) {
    const double dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
    if (!(dx >= 0 && dy >= 0 && dz >= 0)) return 0;
    return 2 * (dx * dy + dy * dz + dz * dx);
}

// The (up to 4) binary nodes that become the slots of the wide node made from binary node b.  T gives leaf(id), left(id), right(id)
// and area(id).  Start from the two children; the internal slot of the largest area is replaced by its left child and its right
// child is appended, until four slots are filled or none is internal.
template <typename T>
PT_HOST_DEVICE inline int gather4(const T &tr, int32_t b, int32_t out[4]) {
    out[0] = out[1] = out[2] = out[3] = -1;
    if (tr.leaf(b)) {  // a tree of one object: the root holds it in slot 0
        out[0] = b;
        return 1;
    }
    int n = 2;
    out[0] = tr.left(b);
    out[1] = tr.right(b);
    for (int round = 0; round < 2; round++) {
        int pick = -1;
        double area = -1;
        for (int k = 0; k < 4; k++) {
            if (k >= n || tr.leaf(out[k])) continue;
            double ar = tr.area(out[k]);
            if (!(ar == ar)) ar = (double)ptrf::bits_float(0x7f800000u);  // unbounded boxes first
            if (ar > area) { area = ar; pick = k; }
        }
        if (pick < 0) break;
        int32_t from = -1;
        for (int k = 0; k < 4; k++)
            if (k == pick) from = out[k];
        const int32_t l = tr.left(from), r = tr.right(from);
        for (int k = 0; k < 4; k++) {
            if (k == pick) out[k] = l;
            if (k == n) out[k] = r;
        }
        n++;
    }
    return n;
}

// the binary tree of stages 3 and 4 as the collapse reads it
struct BinView {
    const int32_t *child;     // [n - 1][2] left, right
    const double *box;        // [2 n - 1][6] lo, hi
    const int32_t *leaf_obj;  // [n] world index of sorted leaf k
    int32_t n;
    PT_HOST_DEVICE bool leaf(int32_t id) const { return is_leaf(n, id); }
    PT_HOST_DEVICE int32_t left(int32_t id) const { return child[2 * (size_t)id]; }
    PT_HOST_DEVICE int32_t right(int32_t id) const { return child[2 * (size_t)id + 1]; }
    PT_HOST_DEVICE double area(int32_t id) const { return box_area(box + 6 * (size_t)id, box + 6 * (size_t)id + 3); }
    PT_HOST_DEVICE int32_t object(int32_t id) const { return leaf_obj[id - (n - 1)]; }
    PT_HOST_DEVICE void box6(int32_t id, double out[6]) const {
        for (int k = 0; k < 6; k++) out[k] = box[6 * (size_t)id + k];
    }
};

// what a wide node's four gathered slots say: ranks, masks, and how many internal and object children
struct SlotPlan {
    uint32_t meta;
    int ni, no;
};
template <typename T>
PT_HOST_DEVICE inline SlotPlan plan_slots(const T &tr, const DevObj *world, const int32_t slot[4]) {
    uint32_t ranks = 0, intm = 0, objm = 0, boxm = 0;
    int ni = 0, no = 0;
    for (int s = 0; s < 4; s++) {
        if (slot[s] < 0) continue;
        if (tr.leaf(slot[s])) {
            ranks |= (uint32_t)no << (2 * s);
            objm |= 1u << s;
            if ((world[(size_t)tr.object(slot[s])].kind & 0xff) == KIND_BOX) boxm |= 1u << s;
            no++;
        } else {
            ranks |= (uint32_t)ni << (2 * s);
            intm |= 1u << s;
            ni++;
        }
    }
    return SlotPlan{ranks | (intm << 8) | (objm << 12) | (boxm << 16), ni, no};
}
// the two counts of a node as one scanned word
PT_HOST_DEVICE inline uint64_t pack_counts(int ni, int no) { return (uint64_t)(uint32_t)ni << 32 | (uint32_t)no; }

// Slot s of a node: its centre and half extent from the binary node's box (an empty slot: a far-away point), with the payload
// bytes of node_base / obj_base / meta in the half extents' low bytes (ptbvh::embed_payload).
PT_HOST_DEVICE inline void write_slot(BvhNode &nd, int s, const double *box6, double margin, int32_t node_base, int32_t obj_base, uint32_t meta,
                                      bool payload = true) {
    const uint32_t bytes[3] = {(uint32_t)node_base, (uint32_t)obj_base, meta & 0xffffffu};
    for (int k = 0; k < 3; k++) {
        float c = 3.0e38f, h = 0.0f;
        if (box6) ptrf::encode_axis(box6[k], box6[3 + k], margin, c, h);
        nd.c[k][s] = c;
        nd.h[k][s] = payload ? ptrf::bits_float(ptrf::h_word(h, bytes[k] >> (8 * s))) : h;  // (ptbvh::build leaves the payload to build_scene_trees)
    }
}
PT_HOST_DEVICE inline void write_words(BvhNode &nd, int32_t node_base, int32_t obj_base, uint32_t meta) {
    nd.node_base = node_base;
    nd.obj_base = obj_base;
    nd.meta = meta;
    for (int k = 0; k < 5; k++) nd.pad[k] = 0;
}

// The breadth-first collapse of a binary tree into wide nodes, on the host: ptbvh::build's and the restatement of the device's
// level rounds (one statement of the numbering).  T gives leaf, left, right, area (gather4), object(id) -- a leaf's world index --
// and box6(id, out) -- lo[3], hi[3].  Level by level from `root`: a node's internal children are consecutive from node_base = the
// next level's first node + the internal children of the level's earlier nodes, its objects from obj_base = the objects so far;
// both offset by node_off / obj_off.  level_start receives the first node of every level (not offset), then the node count.
template <typename T>
inline void collapse(const T &tr, int32_t root, const DevObj *world, double margin, int32_t node_off, int32_t obj_off, bool payload,
                     std::vector<BvhNode> &nodes, std::vector<int32_t> &order, std::vector<int32_t> &level_start) {
    std::vector<int32_t> cur{root}, next;
    int32_t objs_so_far = 0;
    while (!cur.empty()) {
        const int32_t start = (int32_t)nodes.size(), next_start = start + (int32_t)cur.size();
        level_start.push_back(start);
        next.clear();
        for (size_t i = 0; i < cur.size(); i++) {
            int32_t slot[4];
            gather4(tr, cur[i], slot);
            const SlotPlan P = plan_slots(tr, world, slot);
            const int32_t node_base = node_off + next_start + (int32_t)next.size(), obj_base = obj_off + objs_so_far;
            BvhNode nd;
            write_words(nd, node_base, obj_base, P.meta);
            for (int s = 0; s < 4; s++) {
                double b[6];
                if (slot[s] >= 0) tr.box6(slot[s], b);
                write_slot(nd, s, slot[s] >= 0 ? b : nullptr, margin, node_base, obj_base, P.meta, payload);
                if (slot[s] < 0) continue;
                if (tr.leaf(slot[s])) order.push_back(tr.object(slot[s]));
                else next.push_back(slot[s]);
            }
            objs_so_far += P.no;
            nodes.push_back(nd);
        }
        cur.swap(next);
    }
    level_start.push_back((int32_t)nodes.size());
}

// ---------------------------------------------------------------- the host restatement
struct Lbvh {
    std::vector<uint64_t> keys;        // sorted
    std::vector<int32_t> sorted;       // sorted leaf -> position in `finite`
    std::vector<int32_t> child;        // [n - 1][2]
    std::vector<int32_t> parent;       // [2 n - 1], -1 for the root
    std::vector<double> box;           // [2 n - 1][6]
    std::vector<BvhNode> nodes;        // payload bytes in place, node_base / obj_base offset
    std::vector<int32_t> order;        // object slot -> world index
    std::vector<int32_t> level_start;  // first node of every level (not offset), then nodes.size()
};

inline void build_lbvh(const DevObj *world, const int32_t *finite, int32_t n, double margin, int32_t node_off, int32_t obj_off, Lbvh &L) {
    L = Lbvh();
    if (n <= 0) return;
    double cmin[3], cmax[3], scale[3];
    for (int k = 0; k < 3; k++) { cmin[k] = (double)ptrf::bits_float(0x7f800000u); cmax[k] = -cmin[k]; }
    for (int32_t i = 0; i < n; i++) {
        double c[3];
        centroid(ptrf::object_box(world[(size_t)finite[i]]), c);
        for (int k = 0; k < 3; k++) { cmin[k] = ptrf::min_d(cmin[k], c[k]); cmax[k] = ptrf::max_d(cmax[k], c[k]); }
    }
    for (int k = 0; k < 3; k++) scale[k] = key_scale(cmin[k], cmax[k]);
    std::vector<uint64_t> key((size_t)n);
    for (int32_t i = 0; i < n; i++) key[(size_t)i] = object_key(world[(size_t)finite[i]], cmin, scale);
    L.sorted.resize((size_t)n);
    for (int32_t i = 0; i < n; i++) L.sorted[(size_t)i] = i;
    std::stable_sort(L.sorted.begin(), L.sorted.end(), [&](int32_t a, int32_t b) { return key[(size_t)a] < key[(size_t)b]; });
    L.keys.resize((size_t)n);
    std::vector<int32_t> leaf_obj((size_t)n);
    for (int32_t i = 0; i < n; i++) {
        L.keys[(size_t)i] = key[(size_t)L.sorted[(size_t)i]];
        leaf_obj[(size_t)i] = finite[L.sorted[(size_t)i]];
    }
    L.child.assign(2 * (size_t)(n - 1), -1);
    L.parent.assign(2 * (size_t)n - 1, -1);
    for (int32_t i = 0; i + 1 < n; i++) {
        int32_t l, r;
        radix_node(L.keys.data(), n, i, l, r);
        L.child[2 * (size_t)i] = l;
        L.child[2 * (size_t)i + 1] = r;
        L.parent[(size_t)l] = L.parent[(size_t)r] = i;
    }
    L.box.assign(6 * (2 * (size_t)n - 1), 0.0);
    std::vector<uint32_t> visits((size_t)n, 0u);
    for (int32_t k = 0; k < n; k++) {  // the device's walk, one leaf after the other
        const Box b = ptrf::object_box(world[(size_t)leaf_obj[(size_t)k]]);
        double *p = &L.box[6 * (size_t)leaf_id(n, k)];
        for (int a = 0; a < 3; a++) { p[a] = b.lo[a]; p[3 + a] = b.hi[a]; }
        for (int32_t cur = L.parent[(size_t)leaf_id(n, k)]; cur >= 0; cur = L.parent[(size_t)cur]) {
            if (visits[(size_t)cur]++ == 0u) break;
            const double *l = &L.box[6 * (size_t)L.child[2 * (size_t)cur]], *r = &L.box[6 * (size_t)L.child[2 * (size_t)cur + 1]];
            double *q = &L.box[6 * (size_t)cur];
            for (int a = 0; a < 3; a++) { q[a] = ptrf::min_d(l[a], r[a]); q[3 + a] = ptrf::max_d(l[3 + a], r[3 + a]); }
        }
    }
    const BinView tr{L.child.data(), L.box.data(), leaf_obj.data(), n};
    collapse(tr, 0, world, margin, node_off, obj_off, true, L.nodes, L.order, L.level_start);  // (n == 1: id 0 is the leaf)
}

#ifdef __HIPCC__

// ---------------------------------------------------------------- shared device pieces
// exclusive scan of one value per thread of a block of 256; *total receives the block's sum
__device__ inline uint64_t block_scan_256(uint64_t v, uint64_t *lds /* [256] */, uint64_t *total) {
    const uint32_t t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (uint32_t off = 1; off < 256u; off <<= 1) {
        const uint64_t add = t >= off ? lds[t - off] : 0ull;
        __syncthreads();
        lds[t] += add;
        __syncthreads();
    }
    const uint64_t incl = lds[t];
    *total = lds[255];
    __syncthreads();
    return incl - v;
}

// Exclusive scan of in[0, n) in three launches (no look-back, no waiting): the block sums, their scan, the apply.
__global__ void __launch_bounds__(256) bvh_build_scan_reduce_kernel(const uint64_t *in, uint32_t n, uint64_t *sums) {
    __shared__ uint64_t lds[256];
    const uint32_t base = blockIdx.x * (uint32_t)SCAN_TILE + threadIdx.x * 4u;
    uint64_t s = 0;
    for (uint32_t k = 0; k < 4u; k++)
        if (base + k < n) s += in[base + k];
    uint64_t total;
    (void)block_scan_256(s, lds, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
// one block: sums[0, nb) becomes its exclusive scan, sums[nb] the total
__global__ void __launch_bounds__(256) bvh_build_scan_sums_kernel(uint64_t *sums, uint32_t nb) {
    __shared__ uint64_t lds[256];
    uint64_t carry = 0;
    for (uint32_t b0 = 0; b0 < nb; b0 += 256u) {
        const uint32_t i = b0 + threadIdx.x;
        const uint64_t v = i < nb ? sums[i] : 0ull;
        uint64_t total;
        const uint64_t ex = block_scan_256(v, lds, &total);
        if (i < nb) sums[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) sums[nb] = carry;
}
__global__ void __launch_bounds__(256) bvh_build_scan_apply_kernel(const uint64_t *in, uint32_t n, const uint64_t *sums, uint64_t *out) {
    __shared__ uint64_t lds[256];
    const uint32_t base = blockIdx.x * (uint32_t)SCAN_TILE + threadIdx.x * 4u;
    uint64_t v[4], s = 0;
    for (uint32_t k = 0; k < 4u; k++) {
        v[k] = base + k < n ? in[base + k] : 0ull;
        s += v[k];
    }
    uint64_t total;
    uint64_t run = sums[blockIdx.x] + block_scan_256(s, lds, &total);
    for (uint32_t k = 0; k < 4u; k++) {
        if (base + k < n) out[base + k] = run;
        run += v[k];
    }
}
inline uint32_t scan_blocks(uint32_t n) { return (n + (uint32_t)SCAN_TILE - 1u) / (uint32_t)SCAN_TILE; }
// out[i] = in[0] + ... + in[i - 1]; sums [scan_blocks(n) + 1], sums[scan_blocks(n)] the total.  in == out is allowed.
inline void scan_launch(hipStream_t stream, const uint64_t *in, uint32_t n, uint64_t *sums, uint64_t *out) {
    const uint32_t nb = scan_blocks(n);
    if (nb == 0) return;
    hipLaunchKernelGGL(bvh_build_scan_reduce_kernel, dim3(nb), dim3(256), 0, stream, in, n, sums);
    hipLaunchKernelGGL(bvh_build_scan_sums_kernel, dim3(1), dim3(256), 0, stream, sums, nb);
    hipLaunchKernelGGL(bvh_build_scan_apply_kernel, dim3(nb), dim3(256), 0, stream, in, n, sums, out);
}

// ---------------------------------------------------------------- 1. keys
// min / max of the centroids of a block's RED_TILE objects: part[block][6] = min[3], max[3]
__global__ void __launch_bounds__(256) bvh_build_centroid_kernel(const DevObj *objs, const int32_t *finite, uint32_t n, double *part) {
    __shared__ double lds[4][6];
    const double inf = (double)ptrf::bits_float(0x7f800000u);
    double m[6] = {inf, inf, inf, -inf, -inf, -inf};
    for (uint32_t k = 0; k < (uint32_t)RED_TILE / 256u; k++) {
        const uint32_t i = blockIdx.x * (uint32_t)RED_TILE + k * 256u + threadIdx.x;
        if (i >= n) continue;
        double c[3];
        centroid(ptrf::object_box(objs[(size_t)finite[i]]), c);
        for (int a = 0; a < 3; a++) { m[a] = ptrf::min_d(m[a], c[a]); m[3 + a] = ptrf::max_d(m[3 + a], c[a]); }
    }
    for (int step = 1; step < 64; step <<= 1)
        for (int a = 0; a < 3; a++) {
            m[a] = ptrf::min_d(m[a], __shfl_xor(m[a], step));
            m[3 + a] = ptrf::max_d(m[3 + a], __shfl_xor(m[3 + a], step));
        }
    if ((threadIdx.x & 63u) == 0u)
        for (int a = 0; a < 6; a++) lds[threadIdx.x >> 6][a] = m[a];
    __syncthreads();
    if (threadIdx.x < 6u) {
        const int a = (int)threadIdx.x;
        double v = lds[0][a];
        for (int w = 1; w < 4; w++) v = a < 3 ? ptrf::min_d(v, lds[w][a]) : ptrf::max_d(v, lds[w][a]);
        part[6 * (size_t)blockIdx.x + a] = v;
    }
}
// one block: the min / max of the nb partial results, and the three scales: frame[6] = cmin[3], scale[3]
__global__ void __launch_bounds__(256) bvh_build_frame_kernel(const double *part, uint32_t nb, double *frame) {
    __shared__ double lds[4][6];
    const double inf = (double)ptrf::bits_float(0x7f800000u);
    double m[6] = {inf, inf, inf, -inf, -inf, -inf};
    for (uint32_t b = threadIdx.x; b < nb; b += 256u)
        for (int a = 0; a < 3; a++) { m[a] = ptrf::min_d(m[a], part[6 * (size_t)b + a]); m[3 + a] = ptrf::max_d(m[3 + a], part[6 * (size_t)b + 3 + a]); }
    for (int step = 1; step < 64; step <<= 1)
        for (int a = 0; a < 3; a++) {
            m[a] = ptrf::min_d(m[a], __shfl_xor(m[a], step));
            m[3 + a] = ptrf::max_d(m[3 + a], __shfl_xor(m[3 + a], step));
        }
    if ((threadIdx.x & 63u) == 0u)
        for (int a = 0; a < 6; a++) lds[threadIdx.x >> 6][a] = m[a];
    __syncthreads();
    if (threadIdx.x < 3u) {  // (three divisions per build, one lane each)
        const int a = (int)threadIdx.x;
        double lo = lds[0][a], hi = lds[0][3 + a];
        for (int w = 1; w < 4; w++) { lo = ptrf::min_d(lo, lds[w][a]); hi = ptrf::max_d(hi, lds[w][3 + a]); }
        frame[a] = lo;
        frame[3 + a] = key_scale(lo, hi);
    }
}
__global__ void __launch_bounds__(256) bvh_build_keys_kernel(const DevObj *objs, const int32_t *finite, uint32_t n, const double *frame, uint64_t *keys,
                                                             int32_t *vals) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const double cmin[3] = {frame[0], frame[1], frame[2]}, scale[3] = {frame[3], frame[4], frame[5]};
    keys[i] = object_key(objs[(size_t)finite[i]], cmin, scale);
    vals[i] = (int32_t)i;
}

// ---------------------------------------------------------------- 2. the sort
// One wave per tile of SORT_TILE keys, four tiles per block.  hist[digit][tile], so that its exclusive scan is, for every (digit,
// tile), where the tile's first key of that digit goes.
__global__ void __launch_bounds__(256) bvh_build_sort_hist_kernel(const uint64_t *keys, uint32_t n, int shift, uint64_t *hist, uint32_t ntiles) {
    __shared__ uint32_t cnt[4][256];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, tile = blockIdx.x * 4u + wave;
    for (uint32_t d = lane; d < 256u; d += 64u) cnt[wave][d] = 0u;
    __syncthreads();
    for (uint32_t c = 0; c < (uint32_t)SORT_TILE / 64u; c++) {
        const uint32_t e = tile * (uint32_t)SORT_TILE + c * 64u + lane;
        if (tile < ntiles && e < n) atomicAdd(&cnt[wave][(uint32_t)(keys[e] >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tile < ntiles)
        for (uint32_t d = lane; d < 256u; d += 64u) hist[(size_t)d * ntiles + tile] = cnt[wave][d];
}
// Stable: a wave takes its tile 64 keys at a time in order; within the 64, a key's rank among the equal digits is the number of
// lower lanes that hold the same digit (eight ballots), and the digit's running position moves on by their count.
__global__ void __launch_bounds__(256) bvh_build_sort_scatter_kernel(const uint64_t *keys_in, const int32_t *vals_in, uint64_t *keys_out,
                                                                    int32_t *vals_out, uint32_t n, int shift, const uint64_t *where, uint32_t ntiles) {
    __shared__ uint32_t pos[4][256];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, tile = blockIdx.x * 4u + wave;
    if (tile < ntiles)
        for (uint32_t d = lane; d < 256u; d += 64u) pos[wave][d] = (uint32_t)where[(size_t)d * ntiles + tile];
    __syncthreads();
    for (uint32_t c = 0; c < (uint32_t)SORT_TILE / 64u; c++) {  // (every wave of the block runs every round: the barriers are uniform)
        const uint32_t e = tile * (uint32_t)SORT_TILE + c * 64u + lane;
        const bool live = tile < ntiles && e < n;
        const uint64_t key = live ? keys_in[e] : 0ull;
        const int32_t val = live ? vals_in[e] : 0;
        const uint32_t d = (uint32_t)(key >> shift) & 255u;
        unsigned long long same = __ballot(live);
        for (int b = 0; b < 8; b++) {
            const unsigned long long set = __ballot((d >> b) & 1u);
            same &= ((d >> b) & 1u) ? set : ~set;
        }
        const uint32_t rank = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
        const uint32_t to = live ? pos[wave][d] + rank : 0u;
        __syncthreads();
        if (live && rank == 0u) pos[wave][d] += (uint32_t)__popcll(same);
        __syncthreads();
        if (live && to < n) {
            keys_out[to] = key;
            vals_out[to] = val;
        }
    }
}

// ---------------------------------------------------------------- 3. and 4.
__global__ void __launch_bounds__(256) bvh_build_radix_kernel(const uint64_t *keys, int32_t n, int32_t *child, int32_t *parent) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i == 0u) parent[n >= 2 ? 0 : leaf_id(n, 0)] = -1;
    if (i + 1u >= (uint32_t)n) return;
    int32_t l, r;
    radix_node(keys, n, (int32_t)i, l, r);
    child[2 * (size_t)i] = l;
    child[2 * (size_t)i + 1] = r;
    parent[(size_t)l] = (int32_t)i;
    parent[(size_t)r] = (int32_t)i;
}

// A box word as the other CUs see it.  Every box is stored and loaded with agent-scope atomics: the store goes through to the
// device's coherent level, the load is not served from this CU's vector L1 (nor, across XCDs, from a stale L2 line: agent scope
// is what the whole device agrees on), so no copy of a line made before the sibling stored it can answer.
__device__ inline void box_store(double *p, double v) {
    unsigned long long b;
    __builtin_memcpy(&b, &v, 8);
    __hip_atomic_store(reinterpret_cast<unsigned long long *>(p), b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline double box_load(const double *p) {
    const unsigned long long b = __hip_atomic_load(reinterpret_cast<const unsigned long long *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    double v;
    __builtin_memcpy(&v, &b, 8);
    return v;
}

// One lane per sorted leaf: its box and world index, then up the tree.  At every internal node the first arrival leaves and the
// second one unions the children, left then right.  `visits` [n - 1] is zero on entry.  Nobody waits: a lane either goes on or ends.
// Ordering.  What the hand-off rests on is the form of the accesses, not the fences alone: every box word is an agent-scope atomic
// store (box_store: written through), and the storing lane has waited for those stores before its atomic add on the parent's counter
// reaches memory; the lane whose add returns 1 then reads the children with agent-scope atomic loads (box_load), which no line
// cached before the sibling's store can serve.  The add that returned 0 happened before the one that returned 1 (one counter,
// device-wide atomics).  The release fence in front of the add and the acquire fence behind it state that order to the compiler
// and write back / invalidate the caches, but as compiled for gfx950 today the release is a cache write-back WITHOUT a wait of its
// own: the wait that drains the box stores in front of the add is the one the load of parent[] brings.  No inline assembly may add
// one here, so whoever changes this loop or the compiler re-reads the kernel's ISA: the box stores must carry sc1 and a
// vmcnt(0) wait must stand between the last of them and the atomic add.
__global__ void __launch_bounds__(256) bvh_build_boxes_kernel(const DevObj *objs, const int32_t *finite, const int32_t *sorted, int32_t n, const int32_t *child,
                                                              const int32_t *parent, double *box, int32_t *leaf_obj, uint32_t *visits) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= (uint32_t)n) return;
    const int32_t oi = finite[sorted[k]];
    leaf_obj[k] = oi;
    const Box b = ptrf::object_box(objs[(size_t)oi]);
    double *p = box + 6 * (size_t)leaf_id(n, (int32_t)k);
    for (int a = 0; a < 3; a++) { box_store(p + a, b.lo[a]); box_store(p + 3 + a, b.hi[a]); }
    int32_t cur = parent[leaf_id(n, (int32_t)k)];
    for (int up = 0; cur >= 0 && up < 128; up++) {  // (a radix tree over 63 + 32 bits is at most 95 levels deep: the bound only guards the loop)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        const uint32_t before = __hip_atomic_fetch_add(visits + cur, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (before == 0u) break;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        const double *l = box + 6 * (size_t)child[2 * (size_t)cur], *r = box + 6 * (size_t)child[2 * (size_t)cur + 1];
        double *q = box + 6 * (size_t)cur;
        for (int a = 0; a < 3; a++) {
            box_store(q + a, ptrf::min_d(box_load(l + a), box_load(r + a)));
            box_store(q + 3 + a, ptrf::max_d(box_load(l + 3 + a), box_load(r + 3 + a)));
        }
        cur = parent[cur];
    }
}

// ---------------------------------------------------------------- 5. the collapse, one level
struct LevelArgs {
    BinView tr;
    const DevObj *objs;
    const int32_t *cur;      // [count] the binary nodes of this level's wide nodes
    int32_t *next;           // the next level's list
    int32_t *slots;          // [count][4] what the count kernel gathered
    uint64_t *counts;        // [count] pack_counts, then (in place) their exclusive scan
    BvhNode *nodes;          // the whole array (both trees)
    int32_t *order;          // ... and its object slots
    int32_t count;
    int32_t node_first;      // number of this level's first node in `nodes`
    int32_t node_base0;      // node_base of the level's first node: the first node of the next level
    int32_t obj_base0;       // obj_base of the level's first node
    int32_t obj_end;         // one past the tree's last object slot in `order` (a write beyond it is dropped, never made)
    double margin;
};
__global__ void __launch_bounds__(256) bvh_build_level_count_kernel(const LevelArgs A) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint32_t)A.count) return;
    int32_t slot[4];
    gather4(A.tr, A.cur[i], slot);
    *reinterpret_cast<int4 *>(A.slots + 4 * (size_t)i) = make_int4(slot[0], slot[1], slot[2], slot[3]);
    const SlotPlan P = plan_slots(A.tr, A.objs, slot);
    A.counts[i] = pack_counts(P.ni, P.no);
}
// a quad of lanes per node, lane & 3 the slot
__global__ void __launch_bounds__(256) bvh_build_level_write_kernel(const LevelArgs A) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const uint32_t i = t >> 2;
    const int s = (int)(t & 3u);
    if (i >= (uint32_t)A.count) return;
    const int4 g = *reinterpret_cast<const int4 *>(A.slots + 4 * (size_t)i);
    const int32_t slot[4] = {g.x, g.y, g.z, g.w};
    const SlotPlan P = plan_slots(A.tr, A.objs, slot);
    const uint64_t before = A.counts[i];
    const int32_t ni_before = (int32_t)(before >> 32), no_before = (int32_t)(uint32_t)before;
    const int32_t node_base = A.node_base0 + ni_before, obj_base = A.obj_base0 + no_before;
    BvhNode &nd = A.nodes[(size_t)A.node_first + i];
    const int32_t mine = s == 0 ? slot[0] : s == 1 ? slot[1] : s == 2 ? slot[2] : slot[3];
    write_slot(nd, s, mine >= 0 ? A.tr.box + 6 * (size_t)mine : nullptr, A.margin, node_base, obj_base, P.meta);
    if (s == 0) write_words(nd, node_base, obj_base, P.meta);
    if (mine < 0) return;
    const int rank = ptrf::slot_rank(P.meta, s);
    if (A.tr.leaf(mine)) {
        if (obj_base + rank < A.obj_end) A.order[(size_t)obj_base + (size_t)rank] = A.tr.object(mine);
    } else if (ni_before + rank < A.tr.n) {
        A.next[(size_t)ni_before + (size_t)rank] = mine;
    }
}

// ---------------------------------------------------------------- 6. the records
__global__ void __launch_bounds__(256) bvh_build_objs_kernel(BvhObj *bobjs, const int32_t *order, const DevObj *objs, int32_t n) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= (uint32_t)n) return;
    const int32_t idx = order[k];
    const uint4 *src = reinterpret_cast<const uint4 *>(objs + idx);
    uint4 *dst = reinterpret_cast<uint4 *>(bobjs + k);
    const uint4 v0 = src[0], v1 = src[1], v2 = src[2], v3 = src[3], v4 = src[4];
    dst[0] = v0;
    dst[1] = v1;
    dst[2] = v2;
    dst[3] = v3;
    dst[4] = v4;
    dst[5] = make_uint4((uint32_t)idx, 0u, 0u, 0u);
}

// ---------------------------------------------------------------- the launch sequence
// Device memory of one tree's build, allocated for n objects and freed with the object.
struct Scratch {
    void *arena = nullptr;
    uint64_t *keys[2] = {nullptr, nullptr}, *hist = nullptr, *sums = nullptr, *counts = nullptr;
    int32_t *vals[2] = {nullptr, nullptr}, *finite = nullptr, *child = nullptr, *parent = nullptr, *leaf_obj = nullptr, *list[2] = {nullptr, nullptr},
            *slots = nullptr;
    uint32_t *visits = nullptr;
    double *box = nullptr, *part = nullptr, *frame = nullptr;
    uint32_t ntiles = 0, nred = 0;
    Scratch() = default;
    Scratch(const Scratch &) = delete;
    Scratch &operator=(const Scratch &) = delete;
    ~Scratch() {
        if (arena) (void)hipFree(arena);
    }
    hipError_t reserve(int32_t n) {
        if (arena) { (void)hipFree(arena); arena = nullptr; }
        const size_t N = (size_t)(n > 0 ? n : 1);
        ntiles = (uint32_t)((N + SORT_TILE - 1) / SORT_TILE);
        nred = (uint32_t)((N + RED_TILE - 1) / RED_TILE);
        const size_t nhist = 256 * (size_t)ntiles, nsums = scan_blocks((uint32_t)std::max(nhist, N)) + 1;
        size_t off = 0;
        auto take = [&](size_t bytes) { const size_t at = off; off += (bytes + 255) & ~(size_t)255; return at; };
        const size_t o_k0 = take(8 * N), o_k1 = take(8 * N), o_h = take(8 * nhist), o_s = take(8 * nsums), o_c = take(8 * N), o_v0 = take(4 * N), o_v1 = take(4 * N),
                     o_f = take(4 * N), o_ch = take(8 * N), o_p = take(8 * N), o_lo = take(4 * N), o_l0 = take(4 * N), o_l1 = take(4 * N), o_sl = take(16 * N),
                     o_vi = take(4 * N), o_b = take(96 * N), o_pa = take(48 * (size_t)nred), o_fr = take(48);
        const hipError_t e = hipMalloc(&arena, off);
        if (e != hipSuccess) { arena = nullptr; return e; }
        char *b = static_cast<char *>(arena);
        keys[0] = reinterpret_cast<uint64_t *>(b + o_k0);
        keys[1] = reinterpret_cast<uint64_t *>(b + o_k1);
        hist = reinterpret_cast<uint64_t *>(b + o_h);
        sums = reinterpret_cast<uint64_t *>(b + o_s);
        counts = reinterpret_cast<uint64_t *>(b + o_c);
        vals[0] = reinterpret_cast<int32_t *>(b + o_v0);
        vals[1] = reinterpret_cast<int32_t *>(b + o_v1);
        finite = reinterpret_cast<int32_t *>(b + o_f);
        child = reinterpret_cast<int32_t *>(b + o_ch);
        parent = reinterpret_cast<int32_t *>(b + o_p);
        leaf_obj = reinterpret_cast<int32_t *>(b + o_lo);
        list[0] = reinterpret_cast<int32_t *>(b + o_l0);
        list[1] = reinterpret_cast<int32_t *>(b + o_l1);
        slots = reinterpret_cast<int32_t *>(b + o_sl);
        visits = reinterpret_cast<uint32_t *>(b + o_vi);
        box = reinterpret_cast<double *>(b + o_b);
        part = reinterpret_cast<double *>(b + o_pa);
        frame = reinterpret_cast<double *>(b + o_fr);
        return hipSuccess;
    }
};

// One tree of the n objects `finite` (host array of world indices) of the device world `objs`, on `stream`; synchronises once per
// level of wide nodes.  Nodes are written from nodes[node_off] and `order` from order[obj_off] (room for n each); level_start
// receives the first node of every level, not offset, then the node count.  Stages 1 - 4 are left in S for whoever compares them.
inline hipError_t build_tree_launch(hipStream_t stream, Scratch &S, const DevObj *objs, const int32_t *finite, int32_t n, double margin, BvhNode *nodes,
                                    int32_t *order, int32_t node_off, int32_t obj_off, std::vector<int32_t> &level_start) {
    level_start.clear();
    if (n <= 0) return hipSuccess;
#define PTBB_TRY(expr)                      \
    do {                                    \
        const hipError_t e_ = (expr);       \
        if (e_ != hipSuccess) return e_;    \
    } while (0)
    PTBB_TRY(S.reserve(n));
    const uint32_t un = (uint32_t)n, nb256 = (un + 255u) / 256u;
    PTBB_TRY(hipMemcpyAsync(S.finite, finite, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(bvh_build_centroid_kernel, dim3(S.nred), dim3(256), 0, stream, objs, S.finite, un, S.part);
    hipLaunchKernelGGL(bvh_build_frame_kernel, dim3(1), dim3(256), 0, stream, S.part, S.nred, S.frame);
    hipLaunchKernelGGL(bvh_build_keys_kernel, dim3(nb256), dim3(256), 0, stream, objs, S.finite, un, S.frame, S.keys[0], S.vals[0]);
    const uint32_t nblk = (S.ntiles + 3u) / 4u, nhist = 256u * S.ntiles;
    for (int pass = 0; pass < SORT_PASSES; pass++) {  // (an even number of passes: the sorted pairs end in keys[0] / vals[0])
        const int in = pass & 1, out = in ^ 1;
        hipLaunchKernelGGL(bvh_build_sort_hist_kernel, dim3(nblk), dim3(256), 0, stream, S.keys[in], un, 8 * pass, S.hist, S.ntiles);
        scan_launch(stream, S.hist, nhist, S.sums, S.hist);
        hipLaunchKernelGGL(bvh_build_sort_scatter_kernel, dim3(nblk), dim3(256), 0, stream, S.keys[in], S.vals[in], S.keys[out], S.vals[out], un, 8 * pass,
                           S.hist, S.ntiles);
    }
    static_assert(SORT_PASSES % 2 == 0, "the sorted pairs end where they began");
    hipLaunchKernelGGL(bvh_build_radix_kernel, dim3(nb256), dim3(256), 0, stream, S.keys[0], n, S.child, S.parent);
    PTBB_TRY(hipMemsetAsync(S.visits, 0, (size_t)n * sizeof(uint32_t), stream));
    hipLaunchKernelGGL(bvh_build_boxes_kernel, dim3(nb256), dim3(256), 0, stream, objs, S.finite, S.vals[0], n, S.child, S.parent, S.box, S.leaf_obj, S.visits);
    PTBB_TRY(hipMemsetAsync(S.list[0], 0, sizeof(int32_t), stream));  // the root: binary node 0
    PTBB_TRY(hipGetLastError());
    int32_t count = 1, node_first = 0, objs_so_far = 0;
    for (int level = 0; count > 0; level++) {
        if (node_first + count > n || level > n) return hipErrorUnknown;  // (a tree of n objects has at most n wide nodes)
        level_start.push_back(node_first);
        LevelArgs A{BinView{S.child, S.box, S.leaf_obj, n}, objs, S.list[level & 1], S.list[(level & 1) ^ 1], S.slots, S.counts, nodes, order,
                    count, node_off + node_first, node_off + node_first + count, obj_off + objs_so_far, obj_off + n, margin};
        hipLaunchKernelGGL(bvh_build_level_count_kernel, dim3(((uint32_t)count + 255u) / 256u), dim3(256), 0, stream, A);
        scan_launch(stream, S.counts, (uint32_t)count, S.sums, S.counts);
        hipLaunchKernelGGL(bvh_build_level_write_kernel, dim3((4u * (uint32_t)count + 255u) / 256u), dim3(256), 0, stream, A);
        PTBB_TRY(hipGetLastError());
        uint64_t total = 0;
        PTBB_TRY(hipMemcpyAsync(&total, S.sums + scan_blocks((uint32_t)count), sizeof total, hipMemcpyDeviceToHost, stream));
        PTBB_TRY(hipStreamSynchronize(stream));
        const int32_t ni = (int32_t)(total >> 32), no = (int32_t)(uint32_t)total;
        if (ni < 0 || no < 0 || objs_so_far + no > n) return hipErrorUnknown;
        node_first += count;
        objs_so_far += no;
        count = ni;
    }
    level_start.push_back(node_first);
    return objs_so_far == n ? hipSuccess : hipErrorUnknown;
#undef PTBB_TRY
}

inline void objs_launch(hipStream_t stream, BvhObj *bobjs, const int32_t *order, const DevObj *objs, int32_t n) {
    if (n > 0) hipLaunchKernelGGL(bvh_build_objs_kernel, dim3(((uint32_t)n + 255u) / 256u), dim3(256), 0, stream, bobjs, order, objs, n);
}

#endif  // __HIPCC__

}  // namespace ptbb
