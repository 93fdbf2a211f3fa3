/* fake_ptcore_motion.c -- tests/fake_ptcore.c, unedited, with the entry points of displaced reprojection beside it (include/ptcore.h:
 * pt_set_object_ids, pt_read_object_ids, pt_temporal_set_motion, pt_temporal_motion_stats), for the host-rule tests
 * (tests/test_host_motion_cpu.py).  Each appends one line to PTFAKE_LOG like the others; pt_temporal_set_motion logs the table's
 * length and its non-zero rows. */
#include "fake_ptcore.c"

static int32_t g_motion_n;

int32_t pt_set_object_ids(pt_ctx *ctx, int32_t on) { (void)ctx; logf_("pt_set_object_ids on=%d", on); return ret("pt_set_object_ids"); }

int32_t pt_read_object_ids(pt_ctx *ctx, int32_t *ids) { (void)ctx; logf_("pt_read_object_ids ids=%s", P(ids)); return ret("pt_read_object_ids"); }

int32_t pt_temporal_set_motion(pt_ctx *ctx, const double *delta, int32_t num_objects) {
    char rows[512] = "";
    size_t used = 0;
    (void)ctx;
    for (int32_t i = 0; delta && i < num_objects; i++) {
        const double *d = delta + 3 * i;
        if ((d[0] != 0 || d[1] != 0 || d[2] != 0) && used < sizeof rows - 64)
            used += (size_t)snprintf(rows + used, sizeof rows - used, " %d:(%.3f,%.3f,%.3f)", i, d[0], d[1], d[2]);
    }
    logf_("pt_temporal_set_motion delta=%s n=%d moved=[%s ]", P(delta), num_objects, rows);
    g_motion_n = delta ? num_objects : 0;
    return ret("pt_temporal_set_motion");
}

int32_t pt_temporal_motion_stats(pt_ctx *ctx, struct pt_temporal_motion_stats *out) {
    (void)ctx;
    logf_("pt_temporal_motion_stats out=%s", P(out));
    if (out) { memset(out, 0, sizeof *out); out->objects = g_motion_n; out->moved = g_motion_n ? 11 : 0; out->moved_reprojected = g_motion_n ? 7 : 0; }
    g_motion_n = 0; /* one-shot */
    return ret("pt_temporal_motion_stats");
}
