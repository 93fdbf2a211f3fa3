/* fake_ptcore_fogwalk.c -- tests/fake_ptcore.c, unedited, with the entry points of volumetric fog on the BVH path beside it
 * (include/ptcore.h: pt_set_fog_walk, pt_fog_walk_stats), for the host-rule tests (tests/test_fog_walk_cpu.py).
 * Each appends one line to PTFAKE_LOG like the others. */
#include "fake_ptcore.c"

int32_t pt_set_fog_walk(pt_ctx *ctx, int32_t on) {
    (void)ctx;
    logf_("pt_set_fog_walk on=%d", on);
    return ret("pt_set_fog_walk");
}

int32_t pt_fog_walk_stats(pt_ctx *ctx, uint64_t out[6]) {
    (void)ctx;
    logf_("pt_fog_walk_stats out=%s", P(out));
    if (out) { out[0] = 60; out[1] = 2; out[2] = 1440; out[3] = 48; out[4] = 30500; out[5] = 11; }
    return ret("pt_fog_walk_stats");
}
