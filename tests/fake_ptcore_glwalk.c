/* fake_ptcore_glwalk.c -- tests/fake_ptcore.c, unedited, with the entry points of GL shading on the BVH path beside it
 * (include/ptcore.h: pt_set_shading_walk, pt_shading_walk_stats), for the host-rule tests (tests/test_glshade_walk_cpu.py).
 * Each appends one line to PTFAKE_LOG like the others. */
#include "fake_ptcore.c"

int32_t pt_set_shading_walk(pt_ctx *ctx, int32_t on) {
    (void)ctx;
    logf_("pt_set_shading_walk on=%d", on);
    return ret("pt_set_shading_walk");
}

int32_t pt_shading_walk_stats(pt_ctx *ctx, uint64_t out[7]) {
    (void)ctx;
    logf_("pt_shading_walk_stats out=%s", P(out));
    if (out) { out[0] = 9000; out[1] = 12; out[2] = 14400; out[3] = 3; out[4] = 250000; out[5] = 310000; out[6] = 17; }
    return ret("pt_shading_walk_stats");
}
