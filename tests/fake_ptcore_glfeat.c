/* fake_ptcore_glfeat.c -- tests/fake_ptcore.c, unedited, with the entry point of features for GL-shaded frames beside it
 * (include/ptcore.h: pt_set_shading_features), for the host-rule tests (tests/test_gl_features_cpu.py).  It appends one line to
 * PTFAKE_LOG like the others. */
#include "fake_ptcore.c"

int32_t pt_set_shading_features(pt_ctx *ctx, int32_t on) {
    (void)ctx;
    logf_("pt_set_shading_features on=%d", on);
    return ret("pt_set_shading_features");
}
