// Test-only: the product's refit kernels and level sequence (csrc/pt_bvh_refit.h: ptrf::refit_launch) on arrays the test hands in,
// and the header's bit routines evaluated on the device.  test_bvh_refit_probe_gpu.py compares what comes back with the host build
// of the same header (tests/bvh_refit_probe.cpp).
#include "probe_common.h"
#include "pt_bvh_refit.h"

using namespace ptd;

namespace {

// in[i] = {lo, hi, margin}: out[i] = {bits of c, bits of h, the stored word with payload byte i & 255, bits of next_up(c)}
__global__ void bits_kernel(const double *in, uint32_t *out, int32_t n) {
    const int32_t i = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    float c, h;
    ptrf::encode_axis(in[3 * i], in[3 * i + 1], in[3 * i + 2], c, h);
    out[4 * i] = ptrf::float_bits(c);
    out[4 * i + 1] = ptrf::float_bits(h);
    out[4 * i + 2] = ptrf::h_word(h, (uint32_t)i);
    out[4 * i + 3] = ptrf::float_bits(ptrf::next_up(c));
}

}  // namespace

extern "C" {

// nodes [n_nodes] and records [n_objs] of some topology, the world [n_world] to bring them to, the level table [nlevels + 1] and the
// margin.  On return nodes and records are the refitted ones, box [n_nodes][6], area [n_nodes], *cost the figure of the first
// main_nodes nodes (block sums added in block order).  Returns the first HIP error, 0 for none.
int rpg_refit(BvhNode *nodes, int32_t n_nodes, BvhObj *objs, int32_t n_objs, const DevObj *world, int32_t n_world, const int32_t *levels,
              int32_t nlevels, double margin, int32_t main_nodes, double *box, double *area, double *cost) {
    if (n_nodes <= 0 || nlevels <= 0 || levels[nlevels] != n_nodes || main_nodes > n_nodes) return -1;
    for (int32_t l = 0; l < nlevels; l++)
        if (levels[l] < 0 || levels[l] > levels[l + 1]) return -1;
    for (int32_t k = 0; k < n_objs; k++)
        if (objs[k].index < 0 || objs[k].index >= n_world) return -1;
    for (int32_t q = 0; q < n_nodes; q++) {  // every slot points inside the arrays
        const BvhNode &nd = nodes[q];
        for (int s = 0; s < 4; s++) {
            const int rank = ptrf::slot_rank(nd.meta, s);
            if (ptrf::slot_object(nd.meta, s) && (nd.obj_base + rank < 0 || nd.obj_base + rank >= n_objs)) return -1;
            if (ptrf::slot_internal(nd.meta, s) && (nd.node_base + rank <= q || nd.node_base + rank >= n_nodes)) return -1;
        }
    }
    hipError_t st = hipSuccess;
    Buf<BvhNode> dn(nodes, (size_t)n_nodes);
    Buf<BvhObj> dobj(objs, (size_t)n_objs);
    Buf<DevObj> dw(world, (size_t)n_world);
    Buf<double> dbox(nullptr, 6 * (size_t)n_nodes), darea(nullptr, (size_t)n_nodes);
    const uint32_t nb = ptrf::cost_blocks(main_nodes);
    Buf<double> dpart(nullptr, nb);
    for (hipError_t e : {dn.st, dobj.st, dw.st, dbox.st, darea.st, dpart.st}) PROBE_TRY(e);
    if (st != hipSuccess) return (int)st;
    PROBE_TRY(ptrf::refit_launch(nullptr, dn.d, dobj.d, dw.d, n_objs, levels, nlevels, margin, dbox.d, darea.d, main_nodes, dpart.d));
    const int rc = finish(st);
    if (rc != 0) return rc;
    PROBE_TRY(dn.download(nodes));
    PROBE_TRY(dobj.download(objs));
    PROBE_TRY(dbox.download(box));
    PROBE_TRY(darea.download(area));
    double part[1 + (1 << 20) / ptrf::COST_BLOCK] = {};
    if (nb > sizeof part / sizeof part[0]) return -2;
    if (nb) PROBE_TRY(hipMemcpy(part, dpart.d, nb * sizeof(double), hipMemcpyDeviceToHost));
    double total = 0.0;
    for (uint32_t b = 0; b < nb; b++) total += part[b];
    *cost = total;
    return (int)st;
}

int rpg_bits(const double *in, uint32_t *out, int32_t n) {
    hipError_t st = hipSuccess;
    Buf<double> din(in, 3 * (size_t)n);
    Buf<uint32_t> dout(nullptr, 4 * (size_t)n);
    PROBE_TRY(din.st);
    PROBE_TRY(dout.st);
    if (st != hipSuccess) return (int)st;
    hipLaunchKernelGGL(bits_kernel, dim3(((uint32_t)n + 255u) / 256u), dim3(256), 0, nullptr, din.d, dout.d, n);
    const int rc = finish(st);
    if (rc != 0) return rc;
    return (int)dout.download(out);
}

}  // extern "C"
