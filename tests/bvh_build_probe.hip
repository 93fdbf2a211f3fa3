// Test-only: the product's build kernels and launch sequence (csrc/pt_bvh_build.h: ptbb::build_tree_launch, ptbb::objs_launch) on a
// world the test hands in.  test_bvh_build_probe_gpu.py compares every stage that comes back with the host restatement of the same
// header (tests/bvh_build_probe.cpp).
#include "probe_common.h"
#include "pt_bvh_build.h"

#include <vector>

using namespace ptd;

extern "C" {

// One tree of the n objects finite[] of world[n_world], written as the product writes it with node_base / obj_base offset by
// node_off / obj_off.  Out: the sorted keys [n], sorted positions [n], children [n - 1][2], parents [2 n - 1], boxes [2 n - 1][6],
// nodes [room for n], order [n], the level table (at most levels_cap entries; *n_levels receives how many).  Returns the first HIP
// error, -1 for arguments out of range, 0 for none.
int bpg_tree(const DevObj *world, int32_t n_world, const int32_t *finite, int32_t n, double margin, int32_t node_off, int32_t obj_off, uint64_t *keys,
             int32_t *sorted, int32_t *child, int32_t *parent, double *box, BvhNode *nodes, int32_t *order, int32_t *levels, int32_t levels_cap,
             int32_t *n_levels) {
    if (n <= 0 || n_world <= 0 || node_off < 0 || obj_off < 0) return -1;
    for (int32_t i = 0; i < n; i++)
        if (finite[i] < 0 || finite[i] >= n_world) return -1;
    hipError_t st = hipSuccess;
    Buf<DevObj> dw(world, (size_t)n_world);
    // the probe's arrays begin where the product's whole arrays would: the kernels index them with the offsets in
    Buf<BvhNode> dn(nullptr, (size_t)node_off + (size_t)n);
    Buf<int32_t> dord(nullptr, (size_t)obj_off + (size_t)n);
    for (hipError_t e : {dw.st, dn.st, dord.st}) PROBE_TRY(e);
    if (st != hipSuccess) return (int)st;
    ptbb::Scratch S;
    std::vector<int32_t> ls;
    PROBE_TRY(ptbb::build_tree_launch(nullptr, S, dw.d, finite, n, margin, dn.d, dord.d, node_off, obj_off, ls));
    const int rc = finish(st);
    if (rc != 0) return rc;
    if ((int32_t)ls.size() > levels_cap || ls.empty() || ls.back() > n) return -2;
    for (size_t l = 0; l < ls.size(); l++) levels[l] = ls[l];
    *n_levels = (int32_t)ls.size();
    PROBE_TRY(hipMemcpy(keys, S.keys[0], (size_t)n * 8, hipMemcpyDeviceToHost));
    PROBE_TRY(hipMemcpy(sorted, S.vals[0], (size_t)n * 4, hipMemcpyDeviceToHost));
    if (n > 1) PROBE_TRY(hipMemcpy(child, S.child, 2 * (size_t)(n - 1) * 4, hipMemcpyDeviceToHost));
    PROBE_TRY(hipMemcpy(parent, S.parent, (2 * (size_t)n - 1) * 4, hipMemcpyDeviceToHost));
    PROBE_TRY(hipMemcpy(box, S.box, (2 * (size_t)n - 1) * 48, hipMemcpyDeviceToHost));
    PROBE_TRY(hipMemcpy(nodes, dn.d + node_off, (size_t)ls.back() * sizeof(BvhNode), hipMemcpyDeviceToHost));
    PROBE_TRY(hipMemcpy(order, dord.d + obj_off, (size_t)n * 4, hipMemcpyDeviceToHost));
    return (int)st;
}

// the records of order[n] over world[n_world]
int bpg_objs(const int32_t *order, int32_t n, const DevObj *world, int32_t n_world, BvhObj *out) {
    if (n <= 0 || n_world <= 0) return -1;
    for (int32_t k = 0; k < n; k++)
        if (order[k] < 0 || order[k] >= n_world) return -1;
    hipError_t st = hipSuccess;
    Buf<DevObj> dw(world, (size_t)n_world);
    Buf<int32_t> dord(order, (size_t)n);
    Buf<BvhObj> dout(nullptr, (size_t)n);
    for (hipError_t e : {dw.st, dord.st, dout.st}) PROBE_TRY(e);
    if (st != hipSuccess) return (int)st;
    ptbb::objs_launch(nullptr, dout.d, dord.d, dw.d, n);
    const int rc = finish(st);
    if (rc != 0) return rc;
    return (int)dout.download(out);
}

// the tile sizes the kernels were built with: {keys a wave sorts per pass, elements a block scans, centroids a block reduces, passes}
void bpg_sizes(int32_t out[4]) {
    out[0] = ptbb::SORT_TILE;
    out[1] = ptbb::SCAN_TILE;
    out[2] = ptbb::RED_TILE;
    out[3] = ptbb::SORT_PASSES;
}

}  // extern "C"
