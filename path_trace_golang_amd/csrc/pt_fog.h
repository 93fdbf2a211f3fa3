// pt_fog.h -- the scene's fog block (scene.Fog) as single-scattered light along the primary ray: the model of the reference's
// OpenGL backend (internal/engine/gpu/gpu.go:1125-1341, host packing :2011-2105), restated in FP64.
//
// Opt-in per context (pt_set_fog); the CPU engine, whose image is the default contract, ignores fog (scene.go:100).
// Everything here is PT_HD and built from IEEE +,-,*,/, sqrt, floor and the Go routines of pt_math.h (compile with
// -ffp-contract=off), so the gfx950 kernel (fog_kernel, pt_kernels.h) and a host build of this header give the same bits.
//
// Deviations from the GL shader, all deliberate:
//   * FP64 throughout and the parameters stay doubles (GL packs them as float32); Go's Sin / Cos / Exp instead of GLSL's.
//   * hash31's sine is only defined below 2^29 (Go's Sin switches to Payne-Hanek there, not restated): for
//     |q.x + q.y + q.z| >= 2^29, infinities and NaN the hash is 0.5.  GLSL float32 sin has no precision left there either.
//   * affect_sky is a host-side rewrite of the sky constants (fog_sky_rewrite); the trace kernels are not touched.
//   * The march starts from the CPU engine's primary ray and its closest hit (exact FP64 tests, tMin 0.001, no tMax), not
//     from GL's normalised ray: len = |dir|, u = dir / len, tMax = t_hit * len if that is < 40, else 40.
//   * Vector divisions (u, wi, the light normal) divide each component by the scalar.
//   * The draws come from a stream of their own (fog stream below), so the surface path and its draws do not change.
//   * Scenes on the BVH path are refused for the volumetric term (the shadow rays scan every object) unless pt_set_fog_walk is on:
//     then fog_bvh_kernel (pt_fog_walk.h) answers the closest hit and every shadow ray by the wave's walk of the tree.
//
// Fog stream: stream_init(seed_key(seed XOR PTF_STREAM_SALT), y*W + x, s) -- the salt is ASCII "FOG_STRE".  Per
// (pixel, sample) the draws are, march step by march step and light by light in object order, u1 then u2.
#pragma once

#include <stdint.h>

#include "../../include/ptcore.h"
#include "pt_device.h"
#include "pt_math.h"

namespace ptf {

#define PTF_STREAM_SALT 0x464F475F53545245ULL  // "FOG_STRE"
#define PTF_STEPS 24                           // gpu.go:1322
#define PTF_TMAX 40.0                          // gpu.go:1316
#define PTF_PI 3.141592653589793               // math.Pi
#define PTF_HASH_LIMIT 536870912.0             // 2^29

// Resolved fog block: gpu.go:2024-2096 restated on the raw scene.Fog fields, as doubles.
struct FogParams {
    double density;      // > 0 or 0
    double scatter;      // > 0, else 1 when density > 0, else 0
    double sigma_s, sigma_a;
    double g;            // [-0.9, 0.9]
    double hetero;       // (0, 1] or 0
    double noise_scale;  // > 0, default 4
    double color[3];
    int32_t octaves;     // [1, 5], default 3
    int32_t affect_sky;
    int32_t volumetric;
    int32_t pad;
};

// Emissive sphere of the light list: centre, radius, converted emit (Emit * Power, materials.go:47-49).
struct FogLight {
    double c[3];
    double radius;
    double le[3];
    double pad;
};

// Object i of the scene as a light of the fog term: a sphere or sphere_light whose material is emissive with some raw Emit
// component > 0 (the host test, gpu.go:1961-1966) and some Emit*Power component > 0 (the shader's test, :1232).  Objects
// without a material are never lights (GL would fall back to material 0).
PT_HD bool fog_light_of(const pt_scene &sc, int32_t i, FogLight &l) {
    const pt_object &o = sc.objects[i];
    if (o.type != PT_OBJ_SPHERE && o.type != PT_OBJ_SPHERE_LIGHT) return false;
    if (o.material < 0 || o.material >= sc.num_materials) return false;
    const pt_material &m = sc.materials[o.material];
    if (m.type != PT_MAT_EMISSIVE || !(m.emit[0] > 0 || m.emit[1] > 0 || m.emit[2] > 0)) return false;
    double le[3];
    for (int k = 0; k < 3; k++) le[k] = m.emit[k] * m.power;  // convertMaterial, materials.go:47-49
    if (!(le[0] > 0 || le[1] > 0 || le[2] > 0)) return false;
    for (int k = 0; k < 3; k++) { l.c[k] = o.position[k]; l.le[k] = le[k]; }
    l.radius = o.size[0];
    l.pad = 0;
    return true;
}

// Counters of one sample's in-scatter term.
struct FogCount {
    uint32_t shadow_rays;  // light samples that reached the occlusion test (after the distance and cosine tests)
    uint32_t draws;        // fog-stream draws
    uint32_t steps;        // march steps with sigma_s > 0 and sigma_t > 0
};

PT_HD double clamp01(double x) { return x < 0 ? 0.0 : (x > 1 ? 1.0 : x); }

PT_HD FogParams fog_resolve(const pt_fog &f) {
    FogParams p;
    p.density = f.density > 0 ? f.density : 0.0;
    p.scatter = f.scatter > 0 ? f.scatter : (p.density > 0 ? 1.0 : 0.0);
    if (f.sigma_s > 0 || f.sigma_a > 0) {
        p.sigma_s = f.sigma_s;
        p.sigma_a = f.sigma_a;
    } else if (p.density > 0) {
        p.sigma_s = p.density * clamp01(p.scatter);
        p.sigma_a = p.density - p.sigma_s;
        if (p.sigma_a < 0) p.sigma_a = 0;
    } else {
        p.sigma_s = p.sigma_a = 0;
    }
    p.g = f.g < -0.9 ? -0.9 : (f.g > 0.9 ? 0.9 : f.g);
    p.hetero = f.hetero_strength > 0 ? (f.hetero_strength > 1 ? 1.0 : f.hetero_strength) : 0.0;
    p.noise_scale = f.noise_scale > 0 ? f.noise_scale : 4.0;
    p.octaves = f.noise_octaves > 0 ? (f.noise_octaves > 5 ? 5 : f.noise_octaves) : 3;
    for (int i = 0; i < 3; i++) p.color[i] = f.color[i];
    p.affect_sky = f.affect_sky != 0;
    p.volumetric = f.gpu_volumetric != 0;
    p.pad = 0;
    return p;
}

// applyFog(c, 50) (gpu.go:1125-1133, :1392-1393) on one sky constant, per channel: c*a + fog*(1 - a), a = exp(-density*50).
// For a gradient sky this is GL's per-ray form in exact arithmetic (the blend is affine in c).
PT_HD bool fog_sky_applies(const FogParams &p) { return p.density > 0 && p.affect_sky; }
PT_HD void fog_sky_rewrite(const FogParams &p, double c[3]) {
    const double a = ptm::go_exp(-p.density * 50);
    for (int i = 0; i < 3; i++) c[i] = c[i] * a + p.color[i] * (1 - a);
}

PT_HD bool fog_volumetric(const FogParams &p, int32_t max_depth) { return p.volumetric && max_depth > 0; }

PT_HD double fract(double x) { return x - __builtin_floor(x); }

// hash31, gpu.go:1145-1152 (dot products and the sum left to right).
PT_HD double hash31(double px, double py, double pz) {
    const double qx = px * 127.1 + py * 311.7 + pz * 74.7;
    const double qy = px * 269.5 + py * 183.3 + pz * 246.1;
    const double qz = px * 113.5 + py * 271.9 + pz * 124.6;
    const double s = qx + qy + qz;
    if (!(ptm::f_abs(s) < PTF_HASH_LIMIT)) return 0.5;
    return fract(ptm::go_sin(s) * 43758.5453);
}

// volumeNoise, gpu.go:1155-1171.
PT_HD double volume_noise(const FogParams &p, double px, double py, double pz) {
    double amp = 1.0, freq = p.noise_scale, sum = 0.0, norm = 0.0;
    for (int i = 0; i < 5; i++) {
        if (i >= p.octaves) break;
        sum += hash31(px * freq, py * freq, pz * freq) * amp;
        norm += amp;
        amp *= 0.5;
        freq *= 2.0;
    }
    if (norm <= 0) return 1.0;
    return sum / norm;
}

// mediumCoeffs, gpu.go:1174-1203: sigma_s and sigma_t at pos.
PT_HD void medium_coeffs(const FogParams &p, double px, double py, double pz, double &ss, double &st) {
    ss = ptm::go_max(p.sigma_s, 0.0);
    double sa = ptm::go_max(p.sigma_a, 0.0);
    if (ss <= 0 && sa <= 0 && p.density > 0) {
        ss = p.density * clamp01(p.scatter);
        sa = p.density - ss;
        if (sa < 0) sa = 0;
    }
    st = ss + sa;
    if (st <= 0) {
        ss = 0;
        return;
    }
    if (p.hetero > 0) {
        const double n = volume_noise(p, px, py, pz);
        const double k = clamp01(p.hetero);
        const double scale = (1 - k) * (1 - n) + (1 + k) * n;  // mix(1-k, 1+k, n)
        ss *= scale;
        sa *= scale;
        st = ss + sa;
    }
}

// phaseHG, gpu.go:1138-1142.
PT_HD double phase_hg(double cos_theta, double g) {
    const double gg = g * g;
    const double denom = 1 + gg - 2 * g * cos_theta;
    return (1 - gg) / (4 * PTF_PI * denom * ptm::f_sqrt(ptm::go_max(denom, 1e-6)));
}

// sampleLightGeometry for a sphere, gpu.go:889-915: u1, u2 -> point, normal, area pdf.
PT_HD void sample_sphere_light(const FogLight &l, double u1, double u2, double pos[3], double nrm[3], double &pdf) {
    const double z = 1 - 2 * u1;
    const double r = ptm::f_sqrt(ptm::go_max(0.0, 1 - z * z));
    const double phi = 2 * PTF_PI * u2;
    double sn, cs;
    ptm::sincos_pos(phi, &sn, &cs);  // phi in [0, 2 pi): math.Sin / math.Cos
    const double lx = r * cs, ly = r * sn, lz = z;
    const double len = ptm::f_sqrt(lx * lx + ly * ly + lz * lz);
    nrm[0] = lx / len;
    nrm[1] = ly / len;
    nrm[2] = lz / len;
    for (int i = 0; i < 3; i++) pos[i] = l.c[i] + l.radius * nrm[i];
    pdf = 1 / (4 * PTF_PI * l.radius * l.radius);
}

// ---------------------------------------------------------------- exact ray tests (objects.go:37-222, as the CPU engine)

// One ray's per-ray constants: origin, direction, |dir|^2 (the sphere test's `a`), 1/dir (the box slabs).
struct FRay {
    double o[3], d[3], a, inv[3];
};
PT_HD FRay make_fray(double ox, double oy, double oz, double dx, double dy, double dz) {
    FRay r;
    r.o[0] = ox; r.o[1] = oy; r.o[2] = oz;
    r.d[0] = dx; r.d[1] = dy; r.d[2] = dz;
    r.a = dx * dx + dy * dy + dz * dz;
    r.inv[0] = 1 / dx; r.inv[1] = 1 / dy; r.inv[2] = 1 / dz;
    return r;
}

// Hit of object o in [tmin, tmax]; t of the hit.  Same operations as the engine's sphere / plane / box tests.
PT_HD bool hit_object(const ptd::DevObj &o, const FRay &r, double tmin, double tmax, double &t) {
    const int kind = o.kind & 0xff;
    if (kind == ptd::KIND_SPHERE) {
        const double ocx = r.o[0] - o.a[0], ocy = r.o[1] - o.a[1], ocz = r.o[2] - o.a[2];
        const double half_b = ocx * r.d[0] + ocy * r.d[1] + ocz * r.d[2];
        const double oc2 = ocx * ocx + ocy * ocy + ocz * ocz;
        const double c = oc2 - o.radius_sq;
        const double disc = half_b * half_b - r.a * c;
        if (disc < 0) return false;
        const double sq = ptm::f_sqrt(disc);
        double root = (-half_b - sq) / r.a;
        if (root < tmin || root > tmax) {
            root = (-half_b + sq) / r.a;
            if (root < tmin || root > tmax) return false;
        }
        t = root;
        return true;
    }
    if (kind == ptd::KIND_PLANE) {
        const double denom = o.b[0] * r.d[0] + o.b[1] * r.d[1] + o.b[2] * r.d[2];
        if (ptm::f_abs(denom) < 1e-6) return false;
        const double tt = ((o.a[0] - r.o[0]) * o.b[0] + (o.a[1] - r.o[1]) * o.b[1] + (o.a[2] - r.o[2]) * o.b[2]) / denom;
        if (tt < tmin || tt > tmax) return false;
        t = tt;
        return true;
    }
    double t0 = tmin, t1 = tmax;
    for (int i = 0; i < 3; i++) {
        double tn = (o.a[i] - r.o[i]) * r.inv[i];
        double tf = (o.b[i] - r.o[i]) * r.inv[i];
        if (r.inv[i] < 0) { const double s = tn; tn = tf; tf = s; }
        if (tn > t0) t0 = tn;
        if (tf < t1) t1 = tf;
        if (t1 <= t0) return false;
    }
    t = t0;
    return true;
}

// The CPU engine's closest hit of the first segment (renderer.go:297-302): t and the object hit, or false when nothing is hit.
PT_HD bool closest_hit(const ptd::DevObj *objs, int32_t nobj, const FRay &r, double &t_hit, int32_t &best) {
    double closest = ptm::max_float64();
    best = -1;
    for (int32_t i = 0; i < nobj; i++) {
        double t;
        if (hit_object(objs[i], r, 0.001, closest, t)) {
            best = i;
            closest = t;
        }
    }
    t_hit = closest;
    return best >= 0;
}
PT_HD bool closest_hit(const ptd::DevObj *objs, int32_t nobj, const FRay &r, double &t_hit) {
    int32_t best;
    return closest_hit(objs, nobj, r, t_hit, best);
}

// Does any object hit the shadow ray in [0.001, tmax]?  On the device the object loop is left when no active lane is still
// unoccluded (ballot); the lanes of a wave never diverge per object.
PT_HD bool occluded(const ptd::DevObj *objs, int32_t nobj, const FRay &r, double tmax) {
    bool blocked = false;
    for (int32_t i = 0; i < nobj; i++) {
        double t;
        if (!blocked && hit_object(objs[i], r, 0.001, tmax, t)) blocked = true;
#if defined(__HIP_DEVICE_COMPILE__)
        if (__ballot(!blocked) == 0) break;
#else
        if (blocked) break;
#endif
    }
    return blocked;
}

// One light's sample as seen from the march point pos (gpu.go:1222-1262): the unit direction to the sampled point, the distance, the
// cosine at the light and the area pdf.  false: the sample adds nothing and casts no shadow ray (the skips of the shader, in its order).
struct LightSample {
    double w[3], dist, dist_sq, cl, pdf;
};
PT_HD bool light_sample(const FogLight &l, double u1, double u2, double px, double py, double pz, LightSample &s) {
    double lp[3], ln[3];
    sample_sphere_light(l, u1, u2, lp, ln, s.pdf);
    if (s.pdf <= 0) return false;
    const double tx = lp[0] - px, ty = lp[1] - py, tz = lp[2] - pz;
    s.dist_sq = tx * tx + ty * ty + tz * tz;
    if (s.dist_sq <= 1e-6) return false;
    s.dist = ptm::f_sqrt(s.dist_sq);
    s.w[0] = tx / s.dist;
    s.w[1] = ty / s.dist;
    s.w[2] = tz / s.dist;
    // cosLight = max(0, n . -wi) (a NaN counts as 0); tested before the shadow ray, which gives the same result
    s.cl = ln[0] * -s.w[0] + ln[1] * -s.w[1] + ln[2] * -s.w[2];
    return s.cl > 0;
}
// The shadow ray of a sample: from pos along w, occluded by anything in [0.001, shadow_tmax].
PT_HD double shadow_tmax(const LightSample &s) { return s.dist - 0.002; }

// An unoccluded sample's term into the lights' sum (gpu.go:1275-1290), for the view direction u.
PT_HD void light_add(const FogParams &p, const FogLight &l, const LightSample &s, const double u[3], double sum[3]) {
    const double cos_theta = -s.w[0] * u[0] + -s.w[1] * u[1] + -s.w[2] * u[2];
    const double phase = phase_hg(cos_theta, p.g);
    const double geometry = s.cl / ptm::go_max(1e-6, s.dist_sq);
    const double ipdf = ptm::go_max(1e-6, s.pdf);
    for (int c = 0; c < 3; c++) sum[c] += l.le[c] * geometry * phase / ipdf;
}

// The lights' sum into the step's light (gpu.go:1295-1302): times two, clamped to a luminance of 500.
PT_HD void light_total(const double sum[3], double out[3]) {
    for (int c = 0; c < 3; c++) out[c] = sum[c] * 2.0;
    const double lum = 0.2126 * out[0] + 0.7152 * out[1] + 0.0722 * out[2];
    if (lum > 500.0) {
        const double scale = 500.0 / ptm::go_max(lum, 1e-6);
        for (int c = 0; c < 3; c++) out[c] *= scale;
    }
}

// estimateVolumeLight, gpu.go:1208-1303, at pos for the view direction u.  Draws u1, u2 per light from rs.  (fog_bvh_kernel,
// pt_fog_walk.h, walks the same pieces with the lanes' skips as a predicate and the shadow ray answered by the wave's tree walk.)
PT_HD void volume_light(const FogParams &p, const ptd::DevObj *objs, int32_t nobj, const FogLight *lights, int32_t nlight,
                        double px, double py, double pz, const double u[3], uint64_t &rs, FogCount &cnt, double out[3]) {
    out[0] = out[1] = out[2] = 0;
    if (p.scatter <= 0) return;
    double sum[3] = {0, 0, 0};
    for (int32_t j = 0; j < nlight; j++) {
        const FogLight &l = lights[j];
        const double u1 = ptm::stream_next(rs);
        const double u2 = ptm::stream_next(rs);
        cnt.draws += 2;
        LightSample s;
        if (!light_sample(l, u1, u2, px, py, pz, s)) continue;
        cnt.shadow_rays++;
        if (occluded(objs, nobj, make_fray(px, py, pz, s.w[0], s.w[1], s.w[2]), shadow_tmax(s))) continue;
        light_add(p, l, s, u, sum);
    }
    light_total(sum, out);
}

// The march of gpu.go:1319-1340: 24 steps over [0, tmax] along the unit direction u from orig.  `rs` is the sample's fog stream.
PT_HD void fog_march(const FogParams &p, const ptd::DevObj *objs, int32_t nobj, const FogLight *lights, int32_t nlight,
                     const double orig[3], const double u[3], double tmax, uint64_t rs, FogCount &cnt, double L[3]) {
    L[0] = L[1] = L[2] = 0;
    const double step = tmax / PTF_STEPS;
    if (!(step > 0)) return;  // gpu.go:1325 (a zero-length direction)
    for (int i = 0; i < PTF_STEPS; i++) {
        const double t = ((double)i + 0.5) * step;
        const double px = orig[0] + u[0] * t, py = orig[1] + u[1] * t, pz = orig[2] + u[2] * t;
        double ss, st;
        medium_coeffs(p, px, py, pz, ss, st);
        if (st <= 0 || ss <= 0) continue;
        cnt.steps++;
        const double tr = ptm::go_exp(-st * t);
        double ls[3];
        volume_light(p, objs, nobj, lights, nlight, px, py, pz, u, rs, cnt, ls);
        for (int c = 0; c < 3; c++) L[c] += p.color[c] * ls[c] * ss * tr * step;
    }
}

// The march's unit direction u and its length along it (gpu.go:1311-1318 on the CPU engine's ray): to the closest hit, 40 at the most.
PT_HD double march_range(const double dir[3], bool hit, double t_hit, double u[3]) {
    const double len = ptm::f_sqrt(dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2]);
    u[0] = dir[0] / len;
    u[1] = dir[1] / len;
    u[2] = dir[2] / len;
    double tmax = PTF_TMAX;
    if (hit && t_hit * len < PTF_TMAX) tmax = t_hit * len;
    return tmax;
}

// The in-scatter term of one (pixel, sample) along its primary ray (orig, dir), gpu.go:1311-1341, on the CPU engine's ray and
// its closest hit.  `rs` is the sample's fog stream.  Adds nothing unless fog_volumetric() holds (the caller checks).
PT_HD void fog_inscatter(const FogParams &p, const ptd::DevObj *objs, int32_t nobj, const FogLight *lights, int32_t nlight,
                         const double orig[3], const double dir[3], uint64_t rs, FogCount &cnt, double L[3]) {
    double t_hit;
    const bool hit = closest_hit(objs, nobj, make_fray(orig[0], orig[1], orig[2], dir[0], dir[1], dir[2]), t_hit);
    double u[3];
    const double tmax = march_range(dir, hit, t_hit, u);
    fog_march(p, objs, nobj, lights, nlight, orig, u, tmax, rs, cnt, L);
}

}  // namespace ptf
