// pt_slab.h -- the reciprocals of a ray's FP32 slab tests, stated once for every walk of the hierarchy and for the host build of
// the per-lane GL walk (pt_gl_walk.h).
#pragma once

#include "pt_math.h"

namespace ptk {

// 1 / x for a slab test: v_rcp_f32 (1 ulp) on the device, the IEEE quotient on the host.  The bounds were analysed for the looser.
PT_HD float slab_rcp(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rcpf(x);
#else
    return 1.0f / x;
#endif
}

// The direction component a slab test takes its reciprocal of: zero below F.dir_floor (build_broad).  The reciprocal of zero is
// infinite and gives NaN parameters, which are skipped; the reciprocal of a tiny component is finite, its products with the origin
// and the centres pass FLT_MAX, and an infinite tf is no NaN: it culled every box of a ray whose origin lay inside the slab.
PT_HD float slab_dir(float d, float floor) { return __builtin_fabsf(d) < floor ? 0.0f : d; }
// ... and the three reciprocals of a ray's slab tests (floor = F.dir_floor).
PT_HD void slab_recips(float floor, float fdx, float fdy, float fdz, float &ivx, float &ivy, float &ivz) {
    ivx = slab_rcp(slab_dir(fdx, floor));
    ivy = slab_rcp(slab_dir(fdy, floor));
    ivz = slab_rcp(slab_dir(fdz, floor));
}

}  // namespace ptk
