// pt_glshade.h -- GL shading: the estimator of the reference's OpenGL compute shader (rayColor and main,
// internal/engine/gpu/gpu.go:1300-1732; helpers :443-1124; host packing :1829-2010; pass loop :2214-2216), restated in FP64.
//
// Opt-in per context (pt_set_shading); the CPU engine's image stays the default.  Everything here is PT_HD and built from
// IEEE +,-,*,/, sqrt and the Go routines of pt_math.h (compile with -ffp-contract=off), so the gfx950 kernel
// (gl_trace_kernel, pt_kernels.h) and a host build of this header give the same bits.  The model asks the scene two things -- the
// closest hit of a ray and whether a shadow ray is blocked -- through a "world" policy (a template parameter of ray_color and gl_pass):
// LinearWorld below is the loop over all objects, ptg::TreeWorld (pt_gl_walk.h, gl_bvh_kernel) a walk of the hierarchy.
//
// The shader, as the host drives it (uSamplesPerPx = 1 per dispatch, :2214-2216), traces 16 stratified paths per pixel and
// pass and adds them WITHOUT dividing by 16 (samplesPerStratum = max(1, 1/16) = 1, col /= uSamplesPerPx = 1, :1685-1732).  A
// pass here is that sum, so GL's linear value is accum / passes = 16 x the mean path radiance.  This quirk is kept.
//
// Deviations from the shader, all deliberate:
//   * FP64 throughout, no contraction; Go's Sqrt / Sin / Cos / Tan / Exp (pt_math.h) instead of GLSL's float32 routines.
//   * The RNG is the project's counter-based stream (pt_math.h), not the clock-seeded hash_u: one stream per path,
//     stream_init(seed_key(seed ^ PTG_STREAM_SALT), y*W + x, 16*pass + k), so the image does not depend on device, chunk
//     or shard.
//   * An emissive hit adds its emission and ends the path.  The shader goes on with an uninitialised newDir (:1400-1405,
//     :1652-1666), which is undefined.  A metal whose dotNorm <= 1e-6 goes on, as in the shader: its direction is defined.
//   * Sky: the shader's sky types (:1093-1108) come from pt_sky.kind.  A sky block of an unknown type is PT_SKY_BACKGROUND in
//     pt_sky and draws scene.Background here; the shader would draw Sky.Color.
//   * Fog (pt_fog.h): affect_sky is the host-side sky rewrite.  gpu_volumetric marches GL's primary ray, unit direction,
//     length = the first hit of hitWorld capped at 40 (:1312-1318), added before the path terms; its light list and shadow
//     tests stay pt_fog.h's (emissive spheres of the CPU world, exact tests), and its draws come from the fog stream at
//     (y*W + x, 16*pass + k).
//   * Vector divisions divide each component by the scalar; GLSL min / max are y if x < y (max) / y < x (min), else x.
//   * A shadow ray's cosine tests (cosSurf, cosLight) are made before the ray is traced, which gives the same result.
//
// Draw order per path (main stream): the stratum jitter jx, jy; the lens (3 per try of randomInUnitSphere, up to 16 tries)
// when aperture > 0; then per bounce the draws of the material in shader order (cosine direction r1 r2, NEE: startIdx when
// more than 8 lights, u1 u2 per sphere light; GGX r1 r2 before its NEE; dielectric: one choice draw unless TIR), and the
// roulette draw on the last three levels.
#pragma once

#include <stdint.h>

#include "../../include/ptcore.h"
#include "pt_fog.h"
#include "pt_math.h"

namespace ptg {

#define PTG_STREAM_SALT 0x474C5F5348414445ULL  // ASCII "GL_SHADE"
#define PTG_PI 3.14159265359                   // const float PI, gpu.go:441
#define PTG_TWO_PI_COS 6.28318530718           // randomCosineDirection, gpu.go:751
#define PTG_MAX_LIGHTS 8                       // MAX_LIGHTS_TO_SAMPLE, gpu.go:1039
#define PTG_STRATA 4                           // strataSize, gpu.go:1685

enum { GT_SPHERE = 0, GT_PLANE = 1, GT_BOX = 2 };  // OBJ_*, gpu.go:245-247

// A material as the shader reads it after the host packing (gpu.go:1829-1900).
struct GlMat {
    int32_t type;  // PT_MAT_* (unknown strings are lambert on both sides)
    int32_t pad;
    double rough, ior, smoothness, reflectivity, absorption_scale;
    double albedo[3], emit[3], absorption[3], tint[3];
};

// An object as the shader reads it (gpu.go:1900-1950): GL type, resolved material, position, size and the box slabs.
struct GlObj {
    int32_t type;  // GT_*
    int32_t mat;   // index into the GlMat table
    double pos[3], size[3];
    double bmin[3], bmax[3];      // pos -/+ 0.5 * size (gpu.go:1372-1374)
    double center[3], half[3];    // (bmin + bmax) * 0.5, (bmax - bmin) * 0.5 (gpu.go:626-627)
};

// The camera constants of buildCamera (gpu.go:1113-1124), computed once on the host.
struct GlCam {
    double origin[3], llc[3], horizontal[3], vertical[3], u[3], v[3];
    double lens_radius;
};

// The sky as backgroundColor sees it (gpu.go:1093-1108, host packing :1985-2002).
struct GlSky {
    int32_t gradient;
    int32_t pad;
    double color[3], horizon[3], zenith[3];
};

struct GlCount {
    uint32_t paths, segments, shadow_rays, probe_rays, draws;
};

// ---------------------------------------------------------------- small vector helpers (GLSL semantics)
PT_HD double gmax(double x, double y) { return x < y ? y : x; }
PT_HD double gmin(double x, double y) { return y < x ? y : x; }
PT_HD double gclamp(double x, double lo, double hi) { return gmin(gmax(x, lo), hi); }
PT_HD double gsign(double x) { return x > 0 ? 1.0 : (x < 0 ? -1.0 : 0.0); }
PT_HD double dot3(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
PT_HD void cross3(const double a[3], const double b[3], double o[3]) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
PT_HD void normalize3(double v[3]) {
    const double len = ptm::f_sqrt(dot3(v, v));
    v[0] = v[0] / len;
    v[1] = v[1] / len;
    v[2] = v[2] / len;
}
// reflectVec(v, n) = v - 2 * dot(v, n) * n (gpu.go:812-816)
PT_HD void reflect3(const double v[3], const double n[3], double o[3]) {
    const double vn = dot3(v, n);
    for (int i = 0; i < 3; i++) o[i] = v[i] - 2.0 * vn * n[i];
}

// ---------------------------------------------------------------- host set-up

// Material i after the host packing, gpu.go:1840-1898.  `x` holds the fields pt_material does not carry.
PT_HD GlMat gl_material(const pt_material &m, const pt_gl_material &x) {
    GlMat g;
    g.type = m.type;
    g.pad = 0;
    g.rough = m.rough;
    g.ior = m.ior;
    double s = m.smoothness;
    if (s == 0 && m.type == PT_MAT_METAL) s = 1.0 - m.rough;
    if (s < 0) s = 0;
    if (s > 1) s = 1;
    g.smoothness = s;
    double r = x.reflectivity;
    if (r == 0 && m.type == PT_MAT_METAL) r = 1.0;
    if (r < 0) r = 0;
    if (r > 1) r = 1;
    g.reflectivity = r;
    g.absorption_scale = x.absorption_scale;
    if (g.absorption_scale == 0 && m.type == PT_MAT_DIELECTRIC) g.absorption_scale = 0.01;
    double t[3] = {x.tint[0], x.tint[1], x.tint[2]};
    if (t[0] == 0 && t[1] == 0 && t[2] == 0 && m.type == PT_MAT_DIELECTRIC) t[0] = t[1] = t[2] = 1.0;
    for (int i = 0; i < 3; i++) {
        g.albedo[i] = m.albedo[i];
        g.emit[i] = m.emit[i] * m.power;
        g.absorption[i] = m.absorption[i];
        g.tint[i] = t[i];
    }
    return g;
}

// Object i, gpu.go:1912-1940: unknown types are spheres, a missing material id is material 0.  `nmat` = 0 leaves the
// index at 0 of a one-entry table holding the zero material (the caller's convention, see gl_world_size).
PT_HD GlObj gl_object(const pt_object &o, int32_t nmat) {
    GlObj g;
    g.type = o.type == PT_OBJ_PLANE ? GT_PLANE : (o.type == PT_OBJ_BOX ? GT_BOX : GT_SPHERE);
    g.mat = (o.material >= 0 && o.material < nmat) ? o.material : 0;
    for (int i = 0; i < 3; i++) {
        g.pos[i] = o.position[i];
        g.size[i] = o.size[i];
        const double h = 0.5 * o.size[i];
        g.bmin[i] = o.position[i] - h;
        g.bmax[i] = o.position[i] + h;
        g.center[i] = (g.bmin[i] + g.bmax[i]) * 0.5;
        g.half[i] = (g.bmax[i] - g.bmin[i]) * 0.5;
    }
    return g;
}

// Is object i in the shader's light list (gpu.go:1942-1948)?  Material emissive with some raw Emit component > 0.
PT_HD bool gl_is_light(const pt_scene &sc, int32_t i) {
    const int32_t nmat = sc.num_materials;
    if (nmat <= 0) return false;
    const pt_object &o = sc.objects[i];
    const int32_t mi = (o.material >= 0 && o.material < nmat) ? o.material : 0;
    const pt_material &m = sc.materials[mi];
    return m.type == PT_MAT_EMISSIVE && (m.emit[0] > 0 || m.emit[1] > 0 || m.emit[2] > 0);
}

PT_HD GlCam gl_camera(const pt_camera &c, int32_t width, int32_t height) {
    GlCam k;
    const double aspect = c.aspect_ratio != 0 ? c.aspect_ratio : (double)width / (double)height;
    const double theta = c.fov * 3.14159265359 / 180.0;
    const double h = ptm::go_tan(theta * 0.5);
    const double vh = 2.0 * h;
    const double vw = aspect * vh;
    double w[3], u[3], v[3], ow[3];
    for (int i = 0; i < 3; i++) ow[i] = c.position[i] - c.target[i];
    for (int i = 0; i < 3; i++) w[i] = ow[i];
    normalize3(w);
    cross3(c.up, w, u);
    normalize3(u);
    cross3(w, u, v);
    const double fd = c.focus_dist != 0 ? c.focus_dist : ptm::f_sqrt(dot3(ow, ow));
    for (int i = 0; i < 3; i++) {
        k.origin[i] = c.position[i];
        k.horizontal[i] = vw * fd * u[i];
        k.vertical[i] = vh * fd * v[i];
        k.u[i] = u[i];
        k.v[i] = v[i];
    }
    for (int i = 0; i < 3; i++) k.llc[i] = k.origin[i] - 0.5 * k.horizontal[i] - 0.5 * k.vertical[i] - w[i] * fd;
    k.lens_radius = c.aperture * 0.5;
    return k;
}

PT_HD GlSky gl_sky(const pt_sky &s) {
    GlSky g;
    g.gradient = s.kind == PT_SKY_GRADIENT;
    g.pad = 0;
    for (int i = 0; i < 3; i++) {
        g.color[i] = s.kind == PT_SKY_SOLID ? s.color[i] : s.background[i];
        g.horizon[i] = s.horizon[i];
        g.zenith[i] = s.zenith[i];
    }
    return g;
}

// ---------------------------------------------------------------- intersection (t only; the record is built for the winner)

// hitSphere's t, gpu.go:535-553 (disc < 1e-8 rejects).
PT_HD bool hit_sphere_t(const GlObj &o, const double ro[3], const double rd[3], double tmin, double tmax, double &t) {
    const double oc[3] = {ro[0] - o.pos[0], ro[1] - o.pos[1], ro[2] - o.pos[2]};
    const double a = dot3(rd, rd);
    const double hb = dot3(oc, rd);
    const double c = dot3(oc, oc) - o.size[0] * o.size[0];
    const double disc = hb * hb - a * c;
    if (disc < 1e-8) return false;
    const double sq = ptm::f_sqrt(disc);
    double root = (-hb - sq) / a;
    if (root < tmin || root > tmax) {
        root = (-hb + sq) / a;
        if (root < tmin || root > tmax) return false;
    }
    t = root;
    return true;
}

// hitPlane's t, normal (0, 1, 0), gpu.go:555-564.
PT_HD bool hit_plane_t(const GlObj &o, const double ro[3], const double rd[3], double tmin, double tmax, double &t) {
    const double denom = 0.0 * rd[0] + 1.0 * rd[1] + 0.0 * rd[2];
    if (ptm::f_abs(denom) < 1e-6) return false;
    const double tt = ((o.pos[0] - ro[0]) * 0.0 + (o.pos[1] - ro[1]) * 1.0 + (o.pos[2] - ro[2]) * 0.0) / denom;
    if (tt < tmin || tt > tmax) return false;
    t = tt;
    return true;
}

// hitBox's slabs, gpu.go:597-624: t0 (entry) or t1 (exit).
PT_HD bool hit_box_t(const GlObj &o, const double ro[3], const double rd[3], double tmin, double tmax, bool find_exit, double &t) {
    double t0 = tmin, t1 = tmax;
    for (int i = 0; i < 3; i++) {
        const double inv = 1.0 / rd[i];
        double tn = (o.bmin[i] - ro[i]) * inv;
        double tf = (o.bmax[i] - ro[i]) * inv;
        if (inv < 0.0) { const double s = tn; tn = tf; tf = s; }
        t0 = gmax(t0, tn);
        t1 = gmin(t1, tf);
        if (t1 <= t0) return false;
    }
    const double ht = find_exit ? t1 : t0;
    if (ht < tmin || ht > tmax) return false;
    t = ht;
    return true;
}

PT_HD bool hit_t(const GlObj &o, const double ro[3], const double rd[3], double tmin, double tmax, double &t) {
    if (o.type == GT_SPHERE) return hit_sphere_t(o, ro, rd, tmin, tmax, t);
    if (o.type == GT_PLANE) return hit_plane_t(o, ro, rd, tmin, tmax, t);
    return hit_box_t(o, ro, rd, tmin, tmax, false, t);
}

struct GlHit {
    double p[3], n[3], t;
    int32_t obj, mat;
    bool front;
};

// The record of object o hit at t (rayAt, the outward normal and setFaceNormal of gpu.go:549-552, :560-562, :625-654).
PT_HD void hit_record(const GlObj &o, int32_t idx, const double ro[3], const double rd[3], double t, GlHit &h) {
    h.t = t;
    h.obj = idx;
    h.mat = o.mat;
    for (int i = 0; i < 3; i++) h.p[i] = ro[i] + t * rd[i];
    double out[3];
    if (o.type == GT_SPHERE) {
        for (int i = 0; i < 3; i++) out[i] = (h.p[i] - o.pos[i]) / o.size[0];
    } else if (o.type == GT_PLANE) {
        out[0] = 0.0; out[1] = 1.0; out[2] = 0.0;
    } else {
        double lp[3], al[3];
        for (int i = 0; i < 3; i++) { lp[i] = h.p[i] - o.center[i]; al[i] = ptm::f_abs(lp[i]); }
        out[0] = out[1] = out[2] = 0.0;
        if (ptm::f_abs(al[0] - o.half[0]) < 1e-4) out[0] = gsign(lp[0]);
        else if (ptm::f_abs(al[1] - o.half[1]) < 1e-4) out[1] = gsign(lp[1]);
        else out[2] = gsign(lp[2]);
    }
    h.front = dot3(rd, out) < 0.0;
    for (int i = 0; i < 3; i++) h.n[i] = h.front ? out[i] : -out[i];
}

// Closest hit over the objects in [tmin, tmax_start], skipping object `skip` (-1: none).  A later object wins a tie (`root >
// tMax` rejects, equality accepts).  Returns the winner's index or -1.
PT_HD int32_t closest(const GlObj *objs, int32_t nobj, const double ro[3], const double rd[3], double tmin, double tmax_start,
                      int32_t skip, double &t_hit) {
    double best = tmax_start;
    int32_t hit = -1;
    for (int32_t i = 0; i < nobj; i++) {
        double t;
        if (i != skip && hit_t(objs[i], ro, rd, tmin, best, t)) {
            best = t;
            hit = i;
        }
    }
    t_hit = best;
    return hit;
}

// hitWorld as a shadow test (gpu.go:708-738 in [0.001, tmax]): some object hits.  On the device the object loop is left by
// ballot once every active lane is occluded; the lanes of a wave never diverge per object.
PT_HD bool occluded(const GlObj *objs, int32_t nobj, const double ro[3], const double rd[3], double tmax) {
    bool blocked = false;
    for (int32_t i = 0; i < nobj; i++) {
        double t;
        if (!blocked && hit_t(objs[i], ro, rd, 0.001, tmax, t)) blocked = true;
#if defined(__HIP_DEVICE_COMPILE__)
        if (__ballot(!blocked) == 0) break;
#else
        if (blocked) break;
#endif
    }
    return blocked;
}

// The two ray queries of the model as a "world" policy: ray_color and gl_pass below take them through a template parameter.  This
// one is the loop over all objects, what the non-template ray_color and gl_pass use; ptg::TreeWorld (pt_gl_walk.h) answers the same
// queries by a walk of the resident hierarchy, bit for bit.
struct LinearWorld {
    const GlObj *objs;
    int32_t nobj;
    PT_HD int32_t closest(const double ro[3], const double rd[3], double tmin, double tmax_start, int32_t skip, double &t_hit) const {
        return ptg::closest(objs, nobj, ro, rd, tmin, tmax_start, skip, t_hit);
    }
    PT_HD bool occluded(const double ro[3], const double rd[3], double tmax) const { return ptg::occluded(objs, nobj, ro, rd, tmax); }
};

// ---------------------------------------------------------------- the scene as the kernel sees it
struct GlScene {
    const GlObj *objs;
    const GlMat *mats;
    const int32_t *lights;  // object indices of the light list, object order
    int32_t nobj, nlight;
    GlSky sky;
    GlCam cam;
    int32_t max_depth;
    int32_t width, height;
    int32_t fog_on;  // gpu_volumetric march on the primary ray (pt_fog.h)
    ptf::FogParams fog;
    const ptd::DevObj *fog_objs;  // the CPU world, for the fog term's shadow tests
    const ptf::FogLight *fog_lights;
    int32_t fog_nobj, fog_nlight;
};

// sampleLightGeometry + estimateDirectLightSingle (gpu.go:866-990) for light object `li`.
template <typename W>
PT_HD void direct_single(const GlScene &S, const W &world, int32_t li, const GlHit &h, const double albedo[3], uint64_t &rs, GlCount &cnt,
                         double out[3]) {
    out[0] = out[1] = out[2] = 0.0;
    const GlObj &o = S.objs[li];
    if (o.type != GT_SPHERE) return;  // area sampling of spheres only
    const double u1 = ptm::stream_next(rs);
    const double u2 = ptm::stream_next(rs);
    cnt.draws += 2;
    const double z = 1.0 - 2.0 * u1;
    const double r = ptm::f_sqrt(gmax(0.0, 1.0 - z * z));
    const double phi = 2.0 * PTG_PI * u2;
    double sn, cs;
    ptm::sincos_pos(phi, &sn, &cs);
    double ln[3] = {r * cs, r * sn, z};
    normalize3(ln);
    double lp[3];
    for (int i = 0; i < 3; i++) lp[i] = o.pos[i] + o.size[0] * ln[i];
    const double area = 4.0 * PTG_PI * o.size[0] * o.size[0];
    const double pdf = 1.0 / area;
    if (pdf <= 0.0) return;
    const double tl[3] = {lp[0] - h.p[0], lp[1] - h.p[1], lp[2] - h.p[2]};
    const double dsq = dot3(tl, tl);
    if (dsq <= 1e-6) return;
    const double dist = ptm::f_sqrt(dsq);
    const double wi[3] = {tl[0] / dist, tl[1] / dist, tl[2] / dist};
    const GlMat &m = S.mats[o.mat];
    if (m.type != PT_MAT_EMISSIVE) return;
    const double nwi[3] = {-wi[0], -wi[1], -wi[2]};
    const double cos_s = gmax(0.0, dot3(h.n, wi));
    const double cos_l = gmax(0.0, dot3(ln, nwi));
    if (cos_s <= 0.0 || cos_l <= 0.0) return;
    const double so[3] = {h.p[0] + h.n[0] * 0.001, h.p[1] + h.n[1] * 0.001, h.p[2] + h.n[2] * 0.001};
    cnt.shadow_rays++;
    if (world.occluded(so, wi, dist - 0.002)) return;
    const double inv_dsq = 1.0 / gmax(1e-6, dsq);
    const double inv_pdf = 1.0 / gmax(1e-6, pdf);
    const double geom = (cos_s * cos_l) * inv_dsq;
    double c[3];
    for (int i = 0; i < 3; i++) c[i] = albedo[i] / PTG_PI * m.emit[i] * geom * inv_pdf;
    const double lum = c[0] * 0.2126 + c[1] * 0.7152 + c[2] * 0.0722;
    if (lum > 500.0) {
        const double scale = 500.0 / gmax(lum, 1e-6);
        for (int i = 0; i < 3; i++) c[i] = c[i] * scale;
    }
    for (int i = 0; i < 3; i++) out[i] = c[i];
}

// estimateDirectLight, gpu.go:995-1090: every light, or 8 from startIdx when there are more, scaled.
template <typename W>
PT_HD void direct_light(const GlScene &S, const W &world, const GlHit &h, const double albedo[3], uint64_t &rs, GlCount &cnt, double out[3]) {
    out[0] = out[1] = out[2] = 0.0;
    const int32_t L = S.nlight;
    if (L == 0) return;
    const bool subset = L > PTG_MAX_LIGHTS;
    const int32_t n = subset ? PTG_MAX_LIGHTS : L;
    const double scale = subset ? (double)L / (double)PTG_MAX_LIGHTS : 1.0;
    const double inv_l = 1.0 / (double)L;
    int32_t start = 0;
    if (subset) {
        const double r = ptm::stream_next(rs);
        cnt.draws++;
        start = (int32_t)(r * (double)L) % L;
    }
    double tot[3] = {0.0, 0.0, 0.0};
    for (int32_t j = 0; j < n; j++) {
        int32_t i = start + j;
        if (i >= L) i -= L;
        double c[3];
        direct_single(S, world, S.lights[i], h, albedo, rs, cnt, c);
        for (int k = 0; k < 3; k++) tot[k] = tot[k] + c[k];
    }
    if (subset)
        for (int k = 0; k < 3; k++) tot[k] = tot[k] * scale;
    for (int k = 0; k < 3; k++) out[k] = tot[k] * inv_l;
}

// randomCosineDirection, gpu.go:743-770.
PT_HD void cosine_dir(const double n[3], uint64_t &rs, GlCount &cnt, double o[3]) {
    const double r1 = ptm::stream_next(rs);
    const double r2 = ptm::stream_next(rs);
    cnt.draws += 2;
    const double phi = PTG_TWO_PI_COS * r1;
    const double ct = ptm::f_sqrt(r2);
    const double st = ptm::f_sqrt(1.0 - r2);
    double u[3] = {0.0, 0.0, 0.0};
    if (ptm::f_abs(n[0]) > 0.9) u[1] = 1.0;
    else u[0] = 1.0;
    normalize3(u);
    double v[3];
    cross3(n, u, v);
    normalize3(v);
    double sp, cp;
    ptm::sincos_pos(phi, &sp, &cp);
    const double lx = st * cp, ly = st * sp, lz = ct;
    for (int i = 0; i < 3; i++) o[i] = lx * u[i] + ly * v[i] + lz * n[i];
    normalize3(o);
}

// sampleGGX, gpu.go:774-810.
PT_HD void ggx_dir(const double view[3], const double n[3], double rough, uint64_t &rs, GlCount &cnt, double o[3]) {
    const double alpha = rough * rough;
    const double a2 = alpha * alpha;
    const double r1 = ptm::stream_next(rs);
    const double r2 = ptm::stream_next(rs);
    cnt.draws += 2;
    const double ct = ptm::f_sqrt((1.0 - r2) / (1.0 + (a2 - 1.0) * r2));
    const double st = ptm::f_sqrt(1.0 - ct * ct);
    const double phi = 2.0 * PTG_PI * r1;
    double up[3] = {0.0, 0.0, 0.0};
    if (ptm::f_abs(n[2]) < 0.999) up[2] = 1.0;
    else up[0] = 1.0;
    double tg[3], bt[3];
    cross3(up, n, tg);
    normalize3(tg);
    cross3(n, tg, bt);
    double sp, cp;
    ptm::sincos_pos(phi, &sp, &cp);
    const double hx = st * cp, hy = st * sp, hz = ct;
    double hv[3];
    for (int i = 0; i < 3; i++) hv[i] = hx * tg[i] + hy * bt[i] + hz * n[i];
    normalize3(hv);
    const double nv[3] = {-view[0], -view[1], -view[2]};
    reflect3(nv, hv, o);  // GLSL reflect(I, N) = I - 2 dot(N, I) N
    if (dot3(o, n) <= 0.0) reflect3(nv, n, o);
    normalize3(o);
}

// refractVec, gpu.go:820-840 (unit v).
PT_HD void refract3(const double v[3], const double n[3], double eta, double o[3]) {
    const double nv[3] = {-v[0], -v[1], -v[2]};
    const double ct = gmin(dot3(nv, n), 1.0);
    const double s2 = 1.0 - ct * ct;
    if (eta * eta * s2 > 1.0) {
        reflect3(v, n, o);
        return;
    }
    double perp[3];
    for (int i = 0; i < 3; i++) perp[i] = eta * (v[i] + ct * n[i]);
    const double par = ptm::f_sqrt(1.0 - gmin(dot3(perp, perp), 1.0));
    for (int i = 0; i < 3; i++) o[i] = perp[i] + -par * n[i];
}

// reflectance (Schlick with relIOR = n2/n1), gpu.go:843-856.
PT_HD double schlick(double cosine, double rel) {
    double r0 = (rel - 1.0) / (rel + 1.0);
    r0 = r0 * r0;
    const double x = 1.0 - cosine;
    const double x5 = x * x * x * x * x;
    return r0 + (1.0 - r0) * x5;
}

// absorption and tint of a glass leg, gpu.go:1588-1601 / :1615-1630: attenuation *= 0.1 + 0.9 exp(-(a s) d), then * tint.
PT_HD void glass_absorb(const GlMat &m, double d, double att[3]) {
    for (int i = 0; i < 3; i++) {
        const double ab = ptm::go_exp(-(m.absorption[i] * m.absorption_scale * d));
        att[i] = att[i] * (0.1 + ab * 0.9);
    }
    if (m.tint[0] > 0.0 || m.tint[1] > 0.0 || m.tint[2] > 0.0)
        for (int i = 0; i < 3; i++) att[i] = att[i] * m.tint[i];
}

// backgroundColor, gpu.go:1093-1108.
PT_HD void background(const GlSky &s, const double rd[3], double o[3]) {
    if (s.gradient) {
        double d[3] = {rd[0], rd[1], rd[2]};
        normalize3(d);
        const double t = gclamp((d[1] + 1.0) * 0.5, 0.0, 1.0);
        for (int i = 0; i < 3; i++) o[i] = s.horizon[i] * (1.0 - t) + s.zenith[i] * t;
    } else {
        for (int i = 0; i < 3; i++) o[i] = s.color[i];
    }
}

// rayColor, gpu.go:1300-1670, from the primary ray (ro, rd) with the path's stream; `L` starts at the fog term.  `world` answers
// the segment's closest hit, the shadow rays and the metal probe.
template <typename W>
PT_HD void ray_color(const GlScene &S, const W &world, double ro[3], double rd[3], uint64_t &rs, GlCount &cnt, double L[3]) {
    double thr[3] = {1.0, 1.0, 1.0};
    int32_t depth = S.max_depth;
    int32_t glass = -1;     // currentGlassObject
    double travel = 0.0;    // accumulatedTravelDistance
    while (depth > 0) {
        cnt.segments++;
        double th;
        const int32_t hi = world.closest(ro, rd, 0.001, 1e20, glass, th);
        if (hi < 0) {
            double bg[3];
            background(S.sky, rd, bg);
            for (int i = 0; i < 3; i++) L[i] = L[i] + thr[i] * bg[i];
            break;
        }
        GlHit h;
        hit_record(S.objs[hi], hi, ro, rd, th, h);
        const GlMat &m = S.mats[h.mat];
        if (m.type == PT_MAT_EMISSIVE) {  // emission, then the path ends (deviation, see the head of this file)
            for (int i = 0; i < 3; i++) L[i] = L[i] + thr[i] * m.emit[i];
            break;
        }
        double nd[3];
        double att[3] = {m.albedo[0], m.albedo[1], m.albedo[2]};
        if (m.type == PT_MAT_LAMBERT) {
            cosine_dir(h.n, rs, cnt, nd);
            double dl[3];
            direct_light(S, world, h, m.albedo, rs, cnt, dl);
            for (int i = 0; i < 3; i++) L[i] = L[i] + thr[i] * dl[i];
        } else if (m.type == PT_MAT_METAL || m.type == PT_MAT_MIRROR) {
            double view[3] = {rd[0], rd[1], rd[2]};
            normalize3(view);
            const double mr = m.smoothness > 0.0 ? 1.0 - m.smoothness : m.rough;
            const double er = m.reflectivity > 0.0 ? m.reflectivity : 1.0;
            const bool rough = m.type == PT_MAT_METAL && mr > 1e-4;
            if (rough) {
                ggx_dir(view, h.n, mr, rs, cnt, nd);
                const double mr2 = mr * mr;
                const double sw = gclamp(1.0 / (1.0 + mr2 * 2.0), 0.1, 0.9);
                const double dw = 1.0 - sw;
                double dd[3];
                direct_light(S, world, h, m.albedo, rs, cnt, dd);
                for (int i = 0; i < 3; i++) L[i] = L[i] + thr[i] * dd[i] * dw * er * 0.5;
                for (int i = 0; i < 3; i++) att[i] = m.albedo[i] * (sw * er + dw * 0.3);
            } else {
                reflect3(view, h.n, nd);
                if (ptm::f_abs(dot3(nd, nd) - 1.0) > 1e-4) normalize3(nd);
                for (int i = 0; i < 3; i++) att[i] = m.albedo[i] * er;
            }
            if (rough && dot3(nd, h.n) > 1e-6) {  // the reflect-direction probe of an emissive hit (gpu.go:1474-1497)
                double pd[3], po[3];
                reflect3(view, h.n, pd);
                for (int i = 0; i < 3; i++) po[i] = h.p[i] + h.n[i] * 0.001;
                cnt.probe_rays++;
                double pt;
                const int32_t pi = world.closest(po, pd, 0.001, 1e20, -1, pt);
                if (pi >= 0) {
                    const GlMat &pm = S.mats[S.objs[pi].mat];
                    if (pm.type == PT_MAT_EMISSIVE) {
                        GlHit ph;
                        hit_record(S.objs[pi], pi, po, pd, pt, ph);
                        const double dsq = ph.t * ph.t;
                        const double npd[3] = {-pd[0], -pd[1], -pd[2]};
                        const double cl = gmax(0.0, dot3(ph.n, npd));
                        for (int i = 0; i < 3; i++) L[i] = L[i] + thr[i] * (pm.emit[i] * cl / dsq) * m.albedo[i] * 0.5;
                    }
                }
            }
        } else {  // PT_MAT_DIELECTRIC
            att[0] = att[1] = att[2] = 1.0;
            double ud[3] = {rd[0], rd[1], rd[2]};
            normalize3(ud);
            const double nu[3] = {-ud[0], -ud[1], -ud[2]};
            const double ct = gmin(dot3(nu, h.n), 1.0);
            const double s2 = 1.0 - ct * ct;
            const double st = s2 > 0.0 ? ptm::f_sqrt(s2) : 0.0;
            const bool entering = h.front;
            const double inv_ior = 1.0 / m.ior;
            const double eta = entering ? inv_ior : m.ior;
            const double rel = entering ? m.ior : inv_ior;
            if (eta * st > 1.0) {
                reflect3(ud, h.n, nd);
            } else {
                double rp = schlick(ct, rel);
                if (!entering) rp = gmax(rp, 0.05);
                const double ch = ptm::stream_next(rs);
                cnt.draws++;
                if (ch < rp) {
                    reflect3(ud, h.n, nd);
                } else {
                    refract3(ud, h.n, eta, nd);
                    if (entering) {
                        glass = h.obj;
                        const GlObj &go = S.objs[h.obj];
                        double d = 0.0;
                        const double eo[3] = {h.p[0] + nd[0] * 0.001, h.p[1] + nd[1] * 0.001, h.p[2] + nd[2] * 0.001};
                        if (go.type == GT_BOX) {
                            double te;
                            if (hit_box_t(go, eo, nd, 0.001, 1e20, true, te)) d = te;
                        } else if (go.type == GT_SPHERE) {
                            const double r2 = go.size[0] * go.size[0];
                            const double oc[3] = {eo[0] - go.pos[0], eo[1] - go.pos[1], eo[2] - go.pos[2]};
                            const double hb = dot3(oc, nd);
                            const double c = dot3(oc, oc) - r2;
                            const double disc = hb * hb - c;
                            if (disc > 0.0) {
                                const double sq = ptm::f_sqrt(disc);
                                const double et = gmax(-hb - sq, -hb + sq);
                                if (et > 0.001) d = et;
                            }
                        }
                        if (d > 0.0) {
                            travel = d;
                            glass_absorb(m, d, att);
                        }
                    } else {
                        glass = -1;
                        if (travel > 0.0) glass_absorb(m, travel, att);
                        travel = 0.0;
                    }
                }
            }
            normalize3(nd);
        }
        if (depth <= 3) {  // Russian roulette, gpu.go:1641-1652
            const double mc = gmax(att[0], gmax(att[1], att[2]));
            if (mc < 1e-6) break;
            const double rr = gmin(mc, 0.95);
            const double x = ptm::stream_next(rs);
            cnt.draws++;
            if (x > rr) break;
            for (int i = 0; i < 3; i++) att[i] = att[i] / rr;
        }
        for (int i = 0; i < 3; i++) {
            thr[i] = thr[i] * att[i];
            ro[i] = h.p[i] + h.n[i] * 0.001;
            rd[i] = nd[i];
        }
        depth--;
    }
}

// The primary ray of path (pass, k) of pixel (x, y): the stream of the path, the stratum jitter, buildCamera (gpu.go:1110-1124) with
// the lens rejection of at most 16 tries, and the unit direction.  `rs` is left where ray_color goes on drawing.  gl_pass calls
// this for every path; the first-hit features of a GL frame (pt_gl_features.h) are the features of exactly these rays.
PT_HD void primary_ray(const GlScene &S, uint64_t key, int32_t x, int32_t y, uint32_t pass, int32_t k, uint64_t &rs, GlCount &cnt,
                       double ro[3], double rd[3]) {
    const uint64_t pix = (uint64_t)(uint32_t)y * (uint64_t)(uint32_t)S.width + (uint64_t)(uint32_t)x;
    const double wm1 = (double)(S.width - 1), hm1 = (double)(S.height - 1);
    const double fy = (double)(S.height - 1 - y);
    const int32_t sy = k >> 2, sx = k & 3;
    rs = ptm::stream_init(key, pix, (uint64_t)pass * 16u + (uint64_t)k);
    cnt.paths++;
    const double jx = ptm::stream_next(rs);
    const double jy = ptm::stream_next(rs);
    cnt.draws += 2;
    const double u = ((double)x + ((double)sx + jx) / 4.0) / wm1;
    const double v = (fy + ((double)sy + jy) / 4.0) / hm1;
    // buildCamera, gpu.go:1110-1124
    double off[3] = {0.0, 0.0, 0.0};
    const GlCam &c = S.cam;
    if (c.lens_radius > 0.0) {
        double p[3] = {0.0, 0.0, 1.0};
        for (int t = 0; t < 16; t++) {  // randomInUnitSphere, gpu.go:741-748
            const double a = ptm::stream_next(rs);
            const double b = ptm::stream_next(rs);
            const double e = ptm::stream_next(rs);
            cnt.draws += 3;
            const double q[3] = {2.0 * a - 1.0, 2.0 * b - 1.0, 2.0 * e - 1.0};
            if (dot3(q, q) >= 1.0) continue;
            p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
            break;
        }
        const double rdx = c.lens_radius * p[0], rdy = c.lens_radius * p[1];
        for (int i = 0; i < 3; i++) off[i] = c.u[i] * rdx + c.v[i] * rdy;
        for (int i = 0; i < 3; i++) {
            rd[i] = c.llc[i] + u * c.horizontal[i] + v * c.vertical[i] - c.origin[i] - off[i];
            ro[i] = c.origin[i] + off[i];
        }
    } else {
        for (int i = 0; i < 3; i++) {
            rd[i] = c.llc[i] + u * c.horizontal[i] + v * c.vertical[i] - c.origin[i];
            ro[i] = c.origin[i];
        }
    }
    normalize3(rd);
}

// One pass of pixel (x, y): the 16 strata of main (gpu.go:1685-1732) summed in k = 4 sy + sx order, without the /16.
// `key` = seed_key(seed ^ PTG_STREAM_SALT), `fog_key` = seed_key(seed ^ PTF_STREAM_SALT).
template <typename W>
PT_HD void gl_pass(const GlScene &S, const W &world, uint64_t key, uint64_t fog_key, int32_t x, int32_t y, uint32_t pass, GlCount &cnt,
                   ptf::FogCount &fcnt, double col[3]) {
    col[0] = col[1] = col[2] = 0.0;
    const uint64_t pix = (uint64_t)(uint32_t)y * (uint64_t)(uint32_t)S.width + (uint64_t)(uint32_t)x;
    for (int32_t k = 0; k < PTG_STRATA * PTG_STRATA; k++) {
        uint64_t rs;
        double ro[3], rd[3];
        primary_ray(S, key, x, y, pass, k, rs, cnt, ro, rd);
        double L[3] = {0.0, 0.0, 0.0};
        if (S.fog_on && S.max_depth > 0) {  // in-scatter along the primary ray, before the path terms (gpu.go:1310-1340)
            double th;
            const int32_t hi = world.closest(ro, rd, 0.001, PTF_TMAX, -1, th);
            const double tmax = hi >= 0 ? th : PTF_TMAX;
            const uint64_t frs = ptm::stream_init(fog_key, pix, (uint64_t)pass * 16u + (uint64_t)k);
            ptf::fog_march(S.fog, S.fog_objs, S.fog_nobj, S.fog_lights, S.fog_nlight, ro, rd, tmax, frs, fcnt, L);
        }
        ray_color(S, world, ro, rd, rs, cnt, L);
        for (int i = 0; i < 3; i++) col[i] = col[i] + L[i];
    }
}

// The model over the loop over all objects: the signatures gl_trace_kernel and the host builds call.
PT_HD void ray_color(const GlScene &S, double ro[3], double rd[3], uint64_t &rs, GlCount &cnt, double L[3]) {
    const LinearWorld world{S.objs, S.nobj};
    ray_color(S, world, ro, rd, rs, cnt, L);
}
PT_HD void gl_pass(const GlScene &S, uint64_t key, uint64_t fog_key, int32_t x, int32_t y, uint32_t pass, GlCount &cnt,
                   ptf::FogCount &fcnt, double col[3]) {
    const LinearWorld world{S.objs, S.nobj};
    gl_pass(S, world, key, fog_key, x, y, pass, cnt, fcnt, col);
}

}  // namespace ptg
