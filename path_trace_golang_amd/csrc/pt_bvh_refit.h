// pt_bvh_refit.h -- the bits of a BVH slot, written once for the host builder (pt_bvh.h), for scene_prepare's payload
// step (ptcore.hip) and for the device refit below.
//
// A slot of a wide node stores its box as an FP32 centre c and half extent h per axis.  The box is a pure function of the
// slot's EXACT FP64 box [lo, hi] -- the bounds of the objects beneath it -- and of the margin m:
//   1. inflate: lo - m, hi + m;
//   2. c = float(0.5 lo + 0.5 hi); h = the larger of c - lo and hi - c, rounded UP to a float, so [c - h, c + h] holds [lo, hi];
//      bounds that are NaN, or a centre that is not finite, give c = 0, h = +inf (the slab constrains nothing);
//   3. h is rounded up to a multiple of 256 ulp (the largest such finite float where that is not finite), and the low byte
//      carries one byte of node_base / obj_base / meta (scan_bvh reads the first 96 bytes of a node only).
// Only + - x, comparisons and conversions: the host (g++) and the device (gfx950) give the same bits.  Compiled with
// -ffp-contract=off like the other shared headers.
//
// A REFIT keeps the topology (node_base, obj_base, meta, the object order) and recomputes, from the bottom level up,
//   bvh_objs[k].o = objs[bvh_objs[k].index];
//   the exact box of an object slot   = object_box of that record;
//   the exact box of an internal slot = the union of the exact boxes of the child node's occupied slots (min / max: exact);
//   every occupied slot's c / h by the three steps above, keeping the payload byte that is in h already.
// Empty slots and the topology words are not touched.  With the world unchanged the nodes come out byte for byte as built;
// after a move they are the bytes the builder's encoder gives for this topology.  Nothing accumulates from refit to refit.
//
// The union of a node's four slots is taken as (s0 u s1) u (s2 u s3) on both sides, so the FP64 scratch boxes (node_box) agree
// down to the sign of a zero.  The quality figure of a node is a[q] = ((A0 + A1) + A2) + A3, A_s the half area dx dy + dy dz + dz dx
// of slot s's exact box (0 for an empty slot); the figure of a tree is a[q] added in node order within blocks of COST_BLOCK nodes,
// the block sums added in block order.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "pt_device.h"

namespace ptrf {

using namespace ptd;

constexpr int COST_BLOCK = 4096;

struct Box {
    double lo[3], hi[3];
};

PT_HOST_DEVICE inline uint32_t float_bits(float f) {
    uint32_t b;
    __builtin_memcpy(&b, &f, 4);
    return b;
}
PT_HOST_DEVICE inline float bits_float(uint32_t b) {
    float f;
    __builtin_memcpy(&f, &b, 4);
    return f;
}
PT_HOST_DEVICE inline double min_d(double a, double b) { return b < a ? b : a; }  // std::min / std::max, spelled out
PT_HOST_DEVICE inline double max_d(double a, double b) { return a < b ? b : a; }

// nextafterf(f, +inf) of a finite f, on the bits
PT_HOST_DEVICE inline float next_up(float f) {
    uint32_t b = float_bits(f);
    if ((b & 0x7fffffffu) == 0u) b = 1u;  // +-0 -> the smallest positive float
    else if (b >> 31) b -= 1u;
    else b += 1u;
    return bits_float(b);
}
// the smallest float >= v
PT_HOST_DEVICE inline float round_up(double v) {
    float f = (float)v;
    if ((double)f < v) f = next_up(f);
    return f;
}

// steps 1 and 2 for one axis
PT_HOST_DEVICE inline void encode_axis(double lo_exact, double hi_exact, double margin, float &c, float &h) {
    const double lo = lo_exact - margin, hi = hi_exact + margin;
    const float cf = (float)(0.5 * lo + 0.5 * hi);
    const bool cf_finite = (float_bits(cf) & 0x7f800000u) != 0x7f800000u;
    if (lo == lo && hi == hi && cf_finite) {
        c = cf;
        h = round_up(max_d((double)cf - lo, hi - (double)cf));  // [c - h, c + h] holds [lo, hi]
        if (!(h == h)) h = bits_float(0x7f800000u);
    } else {  // absurd or non-finite bounds: the slab constrains nothing
        c = 0.0f;
        h = bits_float(0x7f800000u);
    }
}

// step 3: the stored word of a half extent
PT_HOST_DEVICE inline uint32_t h_word(float h, uint32_t payload_byte) {
    uint32_t b = float_bits(h);
    if ((b & 0x7f800000u) == 0x7f800000u || (b >> 31)) b = 0x7f7fff00u;  // inf (unbounded slab) / NaN: the largest finite float
    else b = (b + 0xffu) & ~0xffu;                                          // up to the next multiple of 256 ulp
    if (b >= 0x7f800000u) b = 0x7f7fff00u;
    return b | (payload_byte & 0xffu);
}

PT_HOST_DEVICE inline Box empty_box() {
    Box b;
    for (int k = 0; k < 3; k++) { b.lo[k] = (double)bits_float(0x7f800000u); b.hi[k] = -(double)bits_float(0x7f800000u); }
    return b;
}
PT_HOST_DEVICE inline void grow(Box &a, const Box &o) {
    for (int k = 0; k < 3; k++) { a.lo[k] = min_d(a.lo[k], o.lo[k]); a.hi[k] = max_d(a.hi[k], o.hi[k]); }
}

// exact bounds of a sphere or a box (ptbvh::object_bounds)
PT_HOST_DEVICE inline Box object_box(const DevObj &o) {
    Box b;
    if ((o.kind & 0xff) == KIND_SPHERE) {
        const double r = __builtin_fabs(o.radius);
        for (int k = 0; k < 3; k++) { b.lo[k] = o.a[k] - r; b.hi[k] = o.a[k] + r; }
    } else {
        for (int k = 0; k < 3; k++) { b.lo[k] = min_d(o.a[k], o.b[k]); b.hi[k] = max_d(o.a[k], o.b[k]); }
    }
    for (int k = 0; k < 3; k++) {  // non-finite geometry: unbounded box, always descended into
        if (!(b.lo[k] == b.lo[k]) || !(b.hi[k] == b.hi[k])) { b.lo[k] = -(double)bits_float(0x7f800000u); b.hi[k] = (double)bits_float(0x7f800000u); }
    }
    return b;
}

PT_HOST_DEVICE inline double half_area(const Box &b) {
    const double dx = b.hi[0] - b.lo[0], dy = b.hi[1] - b.lo[1], dz = b.hi[2] - b.lo[2];
    if (!(dx >= 0 && dy >= 0 && dz >= 0)) return 0.0;
    return dx * dy + dy * dz + dz * dx;
}

// One slot of node `nd` re-encoded from its exact box: c and h of the three axes, the payload bytes kept.
PT_HOST_DEVICE inline void encode_slot(BvhNode &nd, int s, const Box &b, double margin) {
    for (int k = 0; k < 3; k++) {
        float c, h;
        encode_axis(b.lo[k], b.hi[k], margin, c, h);
        const uint32_t w = h_word(h, float_bits(nd.h[k][s]));
        nd.c[k][s] = c;
        nd.h[k][s] = bits_float(w);
    }
}

// slot kinds of a node's meta word
PT_HOST_DEVICE inline bool slot_internal(uint32_t meta, int s) { return (meta >> (8 + s)) & 1u; }
PT_HOST_DEVICE inline bool slot_object(uint32_t meta, int s) { return (meta >> (12 + s)) & 1u; }
PT_HOST_DEVICE inline int slot_rank(uint32_t meta, int s) { return (int)((meta >> (2 * s)) & 3u); }

// the figure of a tree from its nodes' a[q], in the fixed shape
inline double cost_of(const double *node_area, size_t n) {
    double total = 0.0;
    for (size_t b0 = 0; b0 < n; b0 += COST_BLOCK) {
        double s = 0.0;
        for (size_t q = b0; q < n && q < b0 + COST_BLOCK; q++) s += node_area[q];
        total += s;
    }
    return total;
}

#ifdef __HIPCC__

// bvh_objs[k].o = objs[bvh_objs[k].index]: one record per lane, five 16-byte loads and stores
__global__ void __launch_bounds__(256) bvh_refit_objs_kernel(BvhObj *bobjs, const DevObj *objs, int32_t n) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= (uint32_t)n) return;
    const int32_t idx = bobjs[k].index;
    const uint4 *src = reinterpret_cast<const uint4 *>(objs + idx);
    uint4 *dst = reinterpret_cast<uint4 *>(bobjs + k);
    const uint4 v0 = src[0], v1 = src[1], v2 = src[2], v3 = src[3], v4 = src[4];
    dst[0] = v0;
    dst[1] = v1;
    dst[2] = v2;
    dst[3] = v3;
    dst[4] = v4;
}

struct RefitLevelArgs {
    BvhNode *nodes;
    const BvhObj *objs;   // refitted already
    double *node_box;     // [n_nodes][6] exact boxes lo[3], hi[3]; the children's were written by the launch before
    double *node_area;    // [n_nodes] a[q]
    int32_t start, count; // the nodes of this level
    double margin;
};

// One level of the tree: a quad of lanes per node, lane & 3 the slot.  The levels are launched deepest first on one stream; the
// kernel boundary is the only ordering between a node and its children.
__global__ void __launch_bounds__(256) bvh_refit_level_kernel(const RefitLevelArgs A) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const uint32_t local = t >> 2;
    const int s = (int)(t & 3u);
    const bool live = local < (uint32_t)A.count;
    const size_t q = (size_t)A.start + (live ? local : 0u);
    Box bx = empty_box();
    double area = 0.0;
    if (live) {
        BvhNode &nd = A.nodes[q];
        const int4 w = *reinterpret_cast<const int4 *>(&nd.node_base);  // node_base, obj_base, meta, pad
        const uint32_t meta = (uint32_t)w.z;
        const bool is_obj = slot_object(meta, s), is_int = slot_internal(meta, s);
        const int rank = slot_rank(meta, s);
        if (is_obj) {
            bx = object_box(A.objs[(size_t)w.y + (size_t)rank].o);
        } else if (is_int) {
            const double *p = A.node_box + 6 * ((size_t)w.x + (size_t)rank);
            for (int k = 0; k < 3; k++) { bx.lo[k] = p[k]; bx.hi[k] = p[3 + k]; }
        }
        if (is_obj || is_int) {
            encode_slot(nd, s, bx, A.margin);
            area = half_area(bx);
        }
    }
    // the quad's union, (s0 u s1) u (s2 u s3), and its four areas in slot order (every lane of the wave takes part)
    for (int step = 1; step <= 2; step <<= 1) {
        Box o;
        for (int k = 0; k < 3; k++) { o.lo[k] = __shfl_xor(bx.lo[k], step); o.hi[k] = __shfl_xor(bx.hi[k], step); }
        grow(bx, o);
    }
    const int base = (int)(threadIdx.x & 63u) & ~3;
    const double a0 = __shfl(area, base), a1 = __shfl(area, base + 1), a2 = __shfl(area, base + 2), a3 = __shfl(area, base + 3);
    if (live && s == 0) {
        double *p = A.node_box + 6 * q;
        for (int k = 0; k < 3; k++) { p[k] = bx.lo[k]; p[3 + k] = bx.hi[k]; }
        A.node_area[q] = ((a0 + a1) + a2) + a3;
    }
}

// block sums of a[0, n): one lane per COST_BLOCK nodes, added in node order
__global__ void __launch_bounds__(64) bvh_refit_cost_kernel(const double *node_area, int32_t n, double *part) {
    const size_t b = (size_t)blockIdx.x * 64u + threadIdx.x;
    const size_t q0 = b * COST_BLOCK;
    if (q0 >= (size_t)n) return;
    const size_t q1 = q0 + COST_BLOCK < (size_t)n ? q0 + COST_BLOCK : (size_t)n;
    double s = 0.0;
    for (size_t q = q0; q < q1; q++) s += node_area[q];
    part[b] = s;
}

inline uint32_t cost_blocks(int32_t n) { return (uint32_t)(((size_t)(n > 0 ? n : 0) + COST_BLOCK - 1) / COST_BLOCK); }

// The whole refit on `stream`: the records, then the levels of level_start[0 .. nlevels] (ascending node numbers, both trees)
// from the last to the first, then the block sums of the first cost_nodes nodes into part[cost_blocks(cost_nodes)].
// node_box holds 6 doubles and node_area one per node.  Returns the first launch error.
inline hipError_t refit_launch(hipStream_t stream, BvhNode *nodes, BvhObj *bobjs, const DevObj *objs, int32_t n_objs, const int32_t *level_start,
                               int nlevels, double margin, double *node_box, double *node_area, int32_t cost_nodes, double *part) {
    if (n_objs > 0) hipLaunchKernelGGL(bvh_refit_objs_kernel, dim3(((uint32_t)n_objs + 255u) / 256u), dim3(256), 0, stream, bobjs, objs, n_objs);
    for (int l = nlevels - 1; l >= 0; l--) {
        RefitLevelArgs A{nodes, bobjs, node_box, node_area, level_start[l], level_start[l + 1] - level_start[l], margin};
        if (A.count <= 0) continue;
        hipLaunchKernelGGL(bvh_refit_level_kernel, dim3((4u * (uint32_t)A.count + 255u) / 256u), dim3(256), 0, stream, A);
    }
    if (cost_nodes > 0) hipLaunchKernelGGL(bvh_refit_cost_kernel, dim3((cost_blocks(cost_nodes) + 63u) / 64u), dim3(64), 0, stream, node_area, cost_nodes, part);
    return hipGetLastError();
}

#endif  // __HIPCC__

}  // namespace ptrf
