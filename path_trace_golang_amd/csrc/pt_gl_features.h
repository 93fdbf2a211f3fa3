// pt_gl_features.h -- the first-hit features of a GL-shaded frame (pt_set_shading_features).
//
// A CPU-model frame takes its features from the rays its ray-generation kernel wrote (pt_atrous.h FEATURES).  GL shading runs no
// such kernel: every lane of gl_trace_kernel makes its own camera rays, with GL's camera, GL's streams, GL's hit tests and GL's tie
// rule.  This header states what the features of such a frame are, once, for the kernels (gl_feature_kernel, gl_feature_bvh_kernel in
// pt_kernels.h) and for a host build.  Everything is PT_HD and built from the routines of pt_glshade.h (compile with
// -ffp-contract=off), so the device and the host give the same bits.
//
// For pixel (x, y), pass p < k and stratum j = 0 .. 15, in (p, j) order from zero:
//   * the ray is ptg::primary_ray's -- gl_pass's own: stream_init(key, pix, 16 p + j), the two jitter draws, the lens rejection of at
//     most 16 tries when lens_radius > 0, the unit direction;
//   * the first hit is world.closest(ro, rd, 0.001, 1e20, -1, t), the first segment of ray_color: GL's tests, a later object winning a
//     tie, nothing skipped;
//   * a hit adds GlHit.n of ptg::hit_record (the face-forward normal) to `normal`, S.mats[h.mat].albedo (as gl_material packed it,
//     emissive materials included) to `albedo`, t to depth[0] (the direction is unit length: no |d| factor) and 1 to depth[1];
//   * every path adds 1 to depth[2], so depth[2] = 16 * min(k, passes done); a miss adds nothing else;
//   * the object id (pt_set_object_ids) is the index of the first hit of (p = 0, j = 0), -1 on a miss.  GL's object list is the scene's
//     list (an unknown type is a sphere there), so the id is an index into pt_scene.objects as it stands.
// The fog term does not enter.  In GL mode k counts passes, as spp, spp_chunk and pt_step do.
//
// The nine sums are laid out as pt_atrous.h's: f[0..2] normal, f[3..5] albedo, f[6] distance, f[7] paths that hit, f[8] paths taken;
// pta::prep_pixel divides by f[7] and never asks how the sums were made.
#pragma once

#include "pt_glshade.h"

namespace ptg {

// Adds the 16 paths of pass `pass` of pixel (x, y) to the nine running sums f.  `id` (may be null) receives the object of path 0.
template <typename W>
PT_HD void feature_pass(const GlScene &S, const W &world, uint64_t key, int32_t x, int32_t y, uint32_t pass, double f[9], int32_t *id) {
    GlCount cnt = {0u, 0u, 0u, 0u, 0u};  // the rays are gl_pass's; its counters stay gl_pass's
    for (int32_t k = 0; k < PTG_STRATA * PTG_STRATA; k++) {
        uint64_t rs;
        double ro[3], rd[3];
        primary_ray(S, key, x, y, pass, k, rs, cnt, ro, rd);
        double t;
        const int32_t hi = world.closest(ro, rd, 0.001, 1e20, -1, t);
        if (id && k == 0) *id = hi;
        if (hi >= 0) {
            GlHit h;
            hit_record(S.objs[hi], hi, ro, rd, t, h);
            const GlMat &m = S.mats[h.mat];
            f[0] += h.n[0]; f[1] += h.n[1]; f[2] += h.n[2];
            f[3] += m.albedo[0]; f[4] += m.albedo[1]; f[5] += m.albedo[2];
            f[6] += t;
            f[7] += 1.0;
        }
        f[8] += 1.0;
    }
}

// ... over the loop over all objects
PT_HD void feature_pass(const GlScene &S, uint64_t key, int32_t x, int32_t y, uint32_t pass, double f[9], int32_t *id) {
    const LinearWorld world{S.objs, S.nobj};
    feature_pass(S, world, key, x, y, pass, f, id);
}

}  // namespace ptg
