/* fake_ptcore_filtered.c -- tests/fake_ptcore.c, unedited, with the entry points of adaptive sampling by the filtered frame's pooled
 * noise beside it (include/ptcore.h: pt_set_adaptive_filtered, pt_read_block_figures), for the host-rule tests
 * (tests/test_host_filtered_adaptive_cpu.py).  Each appends one line to PTFAKE_LOG like the others. */
#include "fake_ptcore.c"

int32_t pt_set_adaptive_filtered(pt_ctx *ctx, const pt_adaptive_filtered *f) {
    char c[160];
    (void)ctx;
    log_atrous_cfg(c, sizeof c, f ? &f->filter : NULL);
    if (f) logf_("pt_set_adaptive_filtered filter=%s pool=%d reserved=%d", c, f->pool, f->reserved);
    else logf_("pt_set_adaptive_filtered f=NULL");
    return ret("pt_set_adaptive_filtered");
}

int32_t pt_read_block_figures(pt_ctx *ctx, double *pooled, double *own, int32_t *checks) {
    (void)ctx;
    logf_("pt_read_block_figures pooled=%s own=%s checks=%s", P(pooled), P(own), P(checks));
    if (checks) *checks = 3;
    return ret("pt_read_block_figures");
}
