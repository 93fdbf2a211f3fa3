/* fake_ptcore_build.c -- tests/fake_ptcore.c, unedited, with the entry points of the device BVH build beside it (include/ptcore.h:
 * pt_set_bvh_build, pt_bvh_build_stats), for the host-rule tests (tests/test_bvh_build_host_cpu.py).  Each appends one line to
 * PTFAKE_LOG like the others. */
#include "fake_ptcore.c"

int32_t pt_set_bvh_build(pt_ctx *ctx, int32_t mode) {
    (void)ctx;
    logf_("pt_set_bvh_build mode=%d", (int)mode);
    return ret("pt_set_bvh_build");
}

int32_t pt_bvh_build_stats(pt_ctx *ctx, struct pt_bvh_build_stats *out) {
    (void)ctx;
    logf_("pt_bvh_build_stats out=%s", P(out));
    if (out) {
        out->host_builds = 3;
        out->device_builds = 5;
        out->builder = PT_BVH_BUILDER_DEVICE;
        out->last_fallback = PT_BVH_BUILD_FALLBACK_STACK;
        out->nodes = 77;
        out->depth = 6;
        out->stack_need = 9;
        out->reserved = 0;
        out->cost = 12.5;
        out->device_ms = 0.25;
        out->prepare_ms = 1.5;
        out->upload_ms = 0.75;
        out->readback_ms = 0.125;
    }
    return ret("pt_bvh_build_stats");
}
