/* fake_ptcore_walk.c -- tests/fake_ptcore.c, unedited, with the entry points of features on the BVH path beside it
 * (include/ptcore.h: pt_set_feature_walk, pt_feature_walk_stats), for the host-rule tests (tests/test_feature_walk_cpu.py).
 * Each appends one line to PTFAKE_LOG like the others. */
#include "fake_ptcore.c"

int32_t pt_set_feature_walk(pt_ctx *ctx, int32_t on) {
    (void)ctx;
    logf_("pt_set_feature_walk on=%d", on);
    return ret("pt_set_feature_walk");
}

int32_t pt_feature_walk_stats(pt_ctx *ctx, uint64_t out[4]) {
    (void)ctx;
    logf_("pt_feature_walk_stats out=%s", P(out));
    if (out) { out[0] = 60; out[1] = 2; out[2] = 1380; out[3] = 9; }
    return ret("pt_feature_walk_stats");
}
