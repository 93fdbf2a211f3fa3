/* fake_ptcore_refit.c -- tests/fake_ptcore.c, unedited, with the entry points of the BVH refit beside it (include/ptcore.h:
 * pt_set_bvh_refit, pt_bvh_refit_stats), for the host-rule tests (tests/test_bvh_refit_host_cpu.py).  Each appends one line to
 * PTFAKE_LOG like the others. */
#include "fake_ptcore.c"

int32_t pt_set_bvh_refit(pt_ctx *ctx, double max_growth) {
    (void)ctx;
    logf_("pt_set_bvh_refit max_growth=%g", max_growth);
    return ret("pt_set_bvh_refit");
}

int32_t pt_bvh_refit_stats(pt_ctx *ctx, struct pt_bvh_refit_stats *out) {
    (void)ctx;
    logf_("pt_bvh_refit_stats out=%s", P(out));
    if (out) {
        out->builds = 2;
        out->refits = 7;
        out->last_action = 2;
        out->last_build_reason = PT_BVH_REASON_GROWTH;
        out->cost_built = 100.0;
        out->cost_now = 125.0;
        out->refit_ms = 0.5;
    }
    return ret("pt_bvh_refit_stats");
}
