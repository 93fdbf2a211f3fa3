// pt_convert.h -- host-side conversion of a scene's materials and objects to the device records (included by ptcore.hip; tests build it for
// the host with g++ -ffp-contract=off and for the device probe, so that what they check is this text and not a copy).
#pragma once

#include <cstring>
#include <vector>

#include "../../include/ptcore.h"
#include "pt_device.h"
#include "pt_math.h"

namespace ptd {

inline double clampd(double x, double lo, double hi) {  // materials.go:57-65
    if (x < lo) return lo;
    if (x > hi) return hi;
    return x;
}

inline DevMat convert_material(const pt_material &m) {  // materials.go:28-55
    DevMat r;
    std::memset(&r, 0, sizeof r);
    switch (m.type) {
        case PT_MAT_METAL: {
            double rough = m.rough;
            if (m.smoothness > 0) rough = 1.0 - clampd(m.smoothness, 0, 1);
            r.typ = MAT_METAL;
            for (int i = 0; i < 3; i++) r.albedo[i] = m.albedo[i];
            r.rough = clampd(rough, 0, 1);
            break;
        }
        case PT_MAT_DIELECTRIC: {
            double ior = m.ior;
            if (ior == 0) ior = 1.5;
            r.typ = MAT_DIELECTRIC;
            for (int i = 0; i < 3; i++) { r.albedo[i] = m.albedo[i]; r.absorption[i] = m.absorption[i]; }
            r.ior = ior;
            // reflectance's r0 for both faces (materials.go:183, :226-229): the reference recomputes these on every hit
            // from the same operands; done once here with the same IEEE operations (this file is built with
            // -ffp-contract=off like the kernels)
            r.inv_ior = 1.0 / ior;
            {
                double a = (1 - r.inv_ior) / (1 + r.inv_ior);
                r.r0_front = a * a;
                double b = (1 - ior) / (1 + ior);
                r.r0_back = b * b;
            }
            break;
        }
        case PT_MAT_EMISSIVE:
            r.typ = MAT_EMISSIVE;
            for (int i = 0; i < 3; i++) r.emit[i] = m.emit[i] * m.power;
            break;
        case PT_MAT_MIRROR:
            r.typ = MAT_MIRROR;
            for (int i = 0; i < 3; i++) r.albedo[i] = m.albedo[i];
            break;
        default:
            r.typ = MAT_LAMBERT;
            for (int i = 0; i < 3; i++) r.albedo[i] = m.albedo[i];
            r.rough = clampd(m.rough, 0, 1);
            break;
    }
    r.absorbs = (r.absorption[0] > 0 || r.absorption[1] > 0 || r.absorption[2] > 0) ? 1 : 0;
    r.rough_sq = r.rough * r.rough;
    return r;
}

// Russian roulette on the attenuation (a0, a1, a2) (renderer.go:376-392), for the table beside mats[]: the operations of
// ptk::roulette_advance on the same operands in the same order, so the same bits (this file is built with -ffp-contract=off like the
// kernels; the device's division sequences are IEEE divisions, tests/test_div_shared_gpu.py).
inline DevRoulette roulette_record(double a0, double a1, double a2) {
    DevRoulette r;
    const double maxAtt = ptm::go_max(a0, ptm::go_max(a1, a2));
    if (maxAtt < 1e-6) {
        r.prob = ROULETTE_ENDED;
        r.q[0] = r.q[1] = r.q[2] = 0.0;  // never read
        return r;
    }
    const double rrProb = ptm::go_min(maxAtt, 0.95);
    r.prob = rrProb;
    r.q[0] = a0 / rrProb;
    r.q[1] = a1 / rrProb;
    r.q[2] = a2 / rrProb;
    return r;
}

// The table of a converted material list: mats[i]'s albedo at i, the attenuation (1, 1, 1) behind them.
inline void roulette_table(const std::vector<DevMat> &mats, std::vector<DevRoulette> &tab) {
    tab.clear();
    for (const DevMat &m : mats) tab.push_back(roulette_record(m.albedo[0], m.albedo[1], m.albedo[2]));
    tab.push_back(roulette_record(1.0, 1.0, 1.0));
}

// objects.go:225-269; materials are converted once and indexed (the zero material
// of a missing id is slot num_materials)
inline void scene_to_world(const pt_scene &sc, std::vector<DevObj> &world, std::vector<DevMat> &mats) {
    mats.clear();
    for (int i = 0; i < sc.num_materials; i++) mats.push_back(convert_material(sc.materials[i]));
    DevMat zero;
    std::memset(&zero, 0, sizeof zero);
    mats.push_back(zero);
    world.clear();
    for (int i = 0; i < sc.num_objects; i++) {
        const pt_object &o = sc.objects[i];
        DevObj d;
        std::memset(&d, 0, sizeof d);
        d.mat = (o.material >= 0 && o.material < sc.num_materials) ? o.material : sc.num_materials;
        int kind;
        switch (o.type) {
            case PT_OBJ_SPHERE:
            case PT_OBJ_SPHERE_LIGHT:
                kind = KIND_SPHERE;
                for (int k = 0; k < 3; k++) d.a[k] = o.position[k];
                d.radius = o.size[0];
                d.radius_sq = d.radius * d.radius;
                d.inv_radius = 1.0 / d.radius;
                break;
            case PT_OBJ_PLANE:
                kind = KIND_PLANE;
                for (int k = 0; k < 3; k++) d.a[k] = o.position[k];
                d.b[0] = 0; d.b[1] = 1; d.b[2] = 0;
                break;
            case PT_OBJ_BOX:
                kind = KIND_BOX;
                for (int k = 0; k < 3; k++) {
                    d.a[k] = o.position[k] - o.size[k] * 0.5;
                    d.b[k] = o.position[k] + o.size[k] * 0.5;
                }
                break;
            default:
                continue;  // unknown types are skipped
        }
        d.kind = kind | (mats[(size_t)d.mat].typ == MAT_DIELECTRIC ? 0x100 : 0);
        world.push_back(d);
    }
}

}  // namespace ptd
