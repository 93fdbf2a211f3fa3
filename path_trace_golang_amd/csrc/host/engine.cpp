#include "engine.hpp"

#include <dlfcn.h>

#include <algorithm>
#include <cctype>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <mutex>
#include <optional>
#include <stdexcept>
#include <utility>

#include "../../../include/ptcore.h"
#include "png.hpp"

namespace pthost {
namespace engine {

RGBA NewRGBA(int width, int height) {
    RGBA img;
    img.Width = width;
    img.Height = height;
    img.Stride = 4 * width;
    img.Pix.assign((size_t)img.Stride * (size_t)(height > 0 ? height : 0), 0);
    return img;
}

namespace {
// The reference starts on BackendCPU (backend.go:12); this host layer only has the GPU branch.
Backend g_backend = BackendGPU;
}  // namespace

void SetBackend(int b) {
    switch (b) {
        case BackendCPU:
        case BackendGPU:
            g_backend = (Backend)b;
            break;
        default:
            g_backend = BackendCPU;
    }
}
Backend GetBackend() { return g_backend; }

// ---------------------------------------------------------------- libptcore binding (dlopen)
namespace {

// One row per entry point of include/ptcore.h that the host layer binds: the Core member carries the entry point's own name.
// REQUIRED: part of ABI 4 from the start, load_core fails without it.  OPTIONAL: added within ABI 4, null in an older build.
#define PT_ENTRY_POINTS(REQUIRED, OPTIONAL)                                                                                      \
    REQUIRED(pt_abi_version) REQUIRED(pt_last_error) REQUIRED(pt_create) REQUIRED(pt_destroy) REQUIRED(pt_render)               \
    REQUIRED(pt_begin) REQUIRED(pt_step) REQUIRED(pt_read) REQUIRED(pt_end) REQUIRED(pt_set_fog)                                 \
    OPTIONAL(pt_set_shading) OPTIONAL(pt_set_moments) OPTIONAL(pt_noise_estimate) OPTIONAL(pt_set_adaptive)                      \
    OPTIONAL(pt_adaptive_state) OPTIONAL(pt_set_features) OPTIONAL(pt_atrous) OPTIONAL(pt_set_halves) OPTIONAL(pt_atrous_halves) \
    OPTIONAL(pt_temporal) OPTIONAL(pt_temporal_reset) OPTIONAL(pt_temporal_set_clip) OPTIONAL(pt_temporal_clip_stats)           \
    OPTIONAL(pt_set_object_ids) OPTIONAL(pt_temporal_set_motion) OPTIONAL(pt_temporal_motion_stats)                              \
    OPTIONAL(pt_set_adaptive_filtered) OPTIONAL(pt_read_block_figures) OPTIONAL(pt_set_feature_walk) \
    OPTIONAL(pt_set_bvh_refit) OPTIONAL(pt_set_bvh_build) OPTIONAL(pt_set_fog_walk) \
    OPTIONAL(pt_set_shading_walk) OPTIONAL(pt_set_shading_features)

struct Core {
    void *handle = nullptr;
#define MEMBER(fn) decltype(&::fn) fn = nullptr;
    PT_ENTRY_POINTS(MEMBER, MEMBER)
#undef MEMBER
    std::string error;  // sticky load error, like the reference's cached GL init failure (gpu.go:279-286)
};

// What a frame setting needs from the library beyond the required entry points, and what Render answers when it is not there.
enum Feature { GL_SHADING, NOISE_TARGET, TEMPORAL, TEMPORAL_CLIP, ATROUS, FILTERED_NOISE, FEATURES, ADAPTIVE, TEMPORAL_MOTION, FILTERED_ADAPTIVE, FEATURE_WALK, BVH_REFIT, BVH_BUILD, SHADING_FEATURES, SHADING_WALK, FOG_WALK };
const struct { bool (*have)(const Core &); const char *lacks; } kNeeds[] = {
    {[](const Core &c) { return c.pt_set_shading != nullptr; }, "GL shading: libptcore.so lacks pt_set_shading"},
    {[](const Core &c) { return c.pt_set_moments && c.pt_noise_estimate; }, "noise target: libptcore.so lacks pt_set_moments / pt_noise_estimate"},
    {[](const Core &c) { return c.pt_temporal != nullptr; }, "temporal accumulation: libptcore.so lacks pt_temporal"},
    {[](const Core &c) { return c.pt_temporal_set_clip && c.pt_temporal_clip_stats; }, "temporal clip: libptcore.so lacks pt_temporal_set_clip"},
    {[](const Core &c) { return c.pt_atrous && c.pt_set_moments; }, "a-trous filter: libptcore.so lacks pt_atrous / pt_set_moments"},
    {[](const Core &c) { return c.pt_set_halves && c.pt_atrous_halves; }, "filtered noise target: libptcore.so lacks pt_set_halves / pt_atrous_halves"},
    {[](const Core &c) { return c.pt_set_features != nullptr; }, "features: libptcore.so lacks pt_set_features"},
    {[](const Core &c) { return c.pt_set_adaptive && c.pt_adaptive_state; }, "adaptive sampling: libptcore.so lacks pt_set_adaptive / pt_adaptive_state"},
    {[](const Core &c) { return c.pt_set_object_ids && c.pt_temporal_set_motion && c.pt_temporal_motion_stats && c.pt_temporal_reset; },
     "temporal motion: libptcore.so lacks pt_set_object_ids / pt_temporal_set_motion"},
    {[](const Core &c) { return c.pt_set_adaptive_filtered && c.pt_read_block_figures && c.pt_set_adaptive && c.pt_adaptive_state; },
     "filtered adaptive target: libptcore.so lacks pt_set_adaptive_filtered / pt_read_block_figures"},
    {[](const Core &c) { return c.pt_set_feature_walk != nullptr; }, "feature walk: libptcore.so lacks pt_set_feature_walk"},
    {[](const Core &c) { return c.pt_set_bvh_refit != nullptr; }, "BVH refit: libptcore.so lacks pt_set_bvh_refit"},
    {[](const Core &c) { return c.pt_set_bvh_build != nullptr; }, "BVH device build: libptcore.so lacks pt_set_bvh_build"},
    {[](const Core &c) { return c.pt_set_shading_features != nullptr; }, "shading features: libptcore.so lacks pt_set_shading_features"},
    {[](const Core &c) { return c.pt_set_shading_walk != nullptr; }, "shading walk: libptcore.so lacks pt_set_shading_walk"},
    {[](const Core &c) { return c.pt_set_fog_walk != nullptr; }, "fog walk: libptcore.so lacks pt_set_fog_walk"},
};

// What the Set* calls said; an empty field leaves the matter to the environment (the *FromEnv rules).
struct NoiseRule { double target; int step; };
struct Switch { bool on; int n; };  // adaptive + min_spp, a-trous + iterations
struct BlockRule { double target; int pool; };
struct Settings {
    std::optional<bool> fog, temporal, temporal_motion, feature_walk, fog_walk, shading_walk, shading_features;
    std::optional<int> shading, features, bvh_build;
    std::optional<NoiseRule> noise;
    std::optional<Switch> adaptive, atrous;
    std::optional<double> filtered_noise, temporal_clip, bvh_refit;
    std::optional<BlockRule> filtered_adaptive;
};

Core g_core;
pt_ctx *g_ctx = nullptr;
std::vector<int> g_devices;
Settings g_set;
std::mutex g_mu;  // requests are serialised, like the reference's single GL worker (gpu.go:2534-2546)

std::string self_dir() {
    Dl_info info;
    if (dladdr((void *)&self_dir, &info) && info.dli_fname) {
        std::string p(info.dli_fname);
        size_t k = p.find_last_of('/');
        if (k != std::string::npos) return p.substr(0, k);
    }
    return ".";
}

bool load_core() {
    if (g_core.handle) return true;
    if (!g_core.error.empty()) return false;
    std::vector<std::string> cands;
    if (const char *e = std::getenv("PTCORE_LIB")) cands.push_back(e);
    cands.push_back(self_dir() + "/libptcore.so");
    cands.push_back("libptcore.so");
    std::string errs;
    void *h = nullptr;
    for (const std::string &c : cands) {
        h = dlopen(c.c_str(), RTLD_NOW | RTLD_LOCAL);
        if (h) break;
        errs += std::string(dlerror() ? dlerror() : "dlopen failed") + "; ";
    }
    if (!h) { g_core.error = "cannot load libptcore.so (" + errs + ")"; return false; }
    Core c;
    c.handle = h;
    std::string err;
#define OPTIONAL(fn) c.fn = reinterpret_cast<decltype(c.fn)>(dlsym(h, #fn));
#define REQUIRED(fn) OPTIONAL(fn) if (!c.fn && err.empty()) err = "libptcore.so lacks symbol " #fn;
    PT_ENTRY_POINTS(REQUIRED, OPTIONAL)
#undef REQUIRED
#undef OPTIONAL
    if (err.empty() && c.pt_abi_version() != PT_ABI_VERSION) err = "libptcore.so ABI version mismatch";
    if (!err.empty()) {
        g_core.error = err;
        dlclose(h);
        return false;
    }
    g_core = c;
    return true;
}

// The text of a failed call: "pt_x: " + what the library says about it; "" when the call succeeded.
std::string call(const char *name, int32_t rc) { return rc == PT_OK ? std::string() : std::string(name) + ": " + g_core.pt_last_error(); }
#define PT_CALL(fn, ...) call(#fn, g_core.fn(__VA_ARGS__))

// ---- the three environment parsers every *FromEnv goes through
std::string env_lower(const char *name) {
    const char *e = std::getenv(name);
    std::string v(e ? e : "");
    for (char &ch : v) ch = (char)std::tolower((unsigned char)ch);
    return v;
}
bool env_switch(const char *name) {  // 1 / true / on / yes in any case, nothing else
    const std::string v = env_lower(name);
    return v == "1" || v == "true" || v == "on" || v == "yes";
}
int env_int(const char *name, long lo, long hi, int fallback) {  // the whole string a decimal integer in [lo, hi]
    const char *e = std::getenv(name);
    if (!e) return fallback;
    char *end = nullptr;
    const long v = std::strtol(e, &end, 10);
    return end != e && *end == 0 && v >= lo && v <= hi ? (int)v : fallback;
}
double env_double(const char *name, bool (*ok)(double), double fallback) {  // the whole string a number that `ok` accepts
    const char *e = std::getenv(name);
    if (!e) return fallback;
    char *end = nullptr;
    const double v = std::strtod(e, &end);
    return end != e && *end == 0 && ok(v) ? v : fallback;
}
bool positive_finite(double v) { return v > 0 && v <= 1.7976931348623157e308; }
bool finite_not_negative(double v) { return std::isfinite(v) && v >= 0; }

struct Flat {
    std::vector<pt_material> materials;
    std::vector<pt_object> objects;
    pt_scene sc;
};

int material_type(const std::string &t) {
    if (t == scene::MaterialMetal) return PT_MAT_METAL;
    if (t == scene::MaterialDielectric) return PT_MAT_DIELECTRIC;
    if (t == scene::MaterialEmissive) return PT_MAT_EMISSIVE;
    if (t == scene::MaterialMirror) return PT_MAT_MIRROR;
    return PT_MAT_LAMBERT;  // convertMaterial's default branch (materials.go:51-53)
}
int object_type(const std::string &t) {
    if (t == scene::ObjectSphere) return PT_OBJ_SPHERE;
    if (t == scene::ObjectPlane) return PT_OBJ_PLANE;
    if (t == scene::ObjectBox) return PT_OBJ_BOX;
    if (t == scene::ObjectSphereLight) return PT_OBJ_SPHERE_LIGHT;
    return PT_OBJ_UNKNOWN;
}
void set3(double *d, const scene::Vec3 &v) { d[0] = v.X; d[1] = v.Y; d[2] = v.Z; }
void set3(double *d, const scene::Color &c) { d[0] = c.R; d[1] = c.G; d[2] = c.B; }

}  // namespace

void FlattenGlMaterials(const scene::Scene &sc, std::vector<pt_gl_material> &out) {
    out.clear();
    for (const scene::Material &m : sc.Materials) {
        pt_gl_material g;
        g.reflectivity = m.Reflectivity;
        set3(g.tint, m.Tint);
        g.absorption_scale = m.AbsorptionScale;
        out.push_back(g);
    }
}

void FlattenFog(const scene::Fog &f, pt_fog &out) {
    std::memset(&out, 0, sizeof out);
    out.density = f.Density;
    set3(out.color, f.Col);
    out.scatter = f.Scatter;
    out.sigma_s = f.SigmaS;
    out.sigma_a = f.SigmaA;
    out.g = f.G;
    out.hetero_strength = f.HeteroStrength;
    out.noise_scale = f.NoiseScale;
    out.noise_octaves = f.NoiseOctaves;
    out.affect_sky = f.AffectSky ? 1 : 0;
    out.gpu_volumetric = f.GPUVolumetric ? 1 : 0;
}

// Flattens scene.Scene into the C ABI's plain structs.  Exposed for tests through capi.cpp.
void FlattenScene(const scene::Scene &sc, std::vector<pt_material> &materials, std::vector<pt_object> &objects,
                  pt_scene &out) {
    materials.clear();
    objects.clear();
    std::map<std::string, int> ids;
    for (size_t i = 0; i < sc.Materials.size(); i++) {
        const scene::Material &m = sc.Materials[i];
        pt_material pm;
        std::memset(&pm, 0, sizeof pm);
        pm.type = material_type(m.Type);
        set3(pm.albedo, m.Albedo);
        pm.rough = m.Rough;
        pm.ior = m.IOR;
        set3(pm.emit, m.Emit);
        pm.power = m.Power;
        set3(pm.absorption, m.Absorption);
        pm.smoothness = m.Smoothness;
        materials.push_back(pm);
        ids[m.ID] = (int)i;  // later duplicates replace earlier ones (objects.go:227-229)
    }
    for (const scene::Object &o : sc.Objects) {
        pt_object po;
        std::memset(&po, 0, sizeof po);
        po.type = object_type(o.Type);
        auto it = ids.find(o.MaterialID);
        po.material = it == ids.end() ? -1 : it->second;
        set3(po.position, o.Position);
        set3(po.size, o.Size);
        objects.push_back(po);
    }
    std::memset(&out, 0, sizeof out);
    set3(out.camera.position, sc.Cam.Position);
    set3(out.camera.target, sc.Cam.Target);
    set3(out.camera.up, sc.Cam.Up);
    out.camera.fov = sc.Cam.FOV;
    out.camera.aperture = sc.Cam.Aperture;
    out.camera.focus_dist = sc.Cam.FocusDist;
    out.camera.aspect_ratio = sc.Cam.AspectRatio;
    set3(out.sky.background, sc.Background);
    out.sky.kind = PT_SKY_BACKGROUND;
    if (sc.SkyPtr) {
        if (sc.SkyPtr->Type == "gradient") out.sky.kind = PT_SKY_GRADIENT;
        else if (sc.SkyPtr->Type == "solid") out.sky.kind = PT_SKY_SOLID;
        set3(out.sky.color, sc.SkyPtr->Col);
        set3(out.sky.horizon, sc.SkyPtr->Horizon);
        set3(out.sky.zenith, sc.SkyPtr->Zenith);
    }
    out.num_materials = (int32_t)materials.size();
    out.num_objects = (int32_t)objects.size();
    out.materials = materials.empty() ? nullptr : materials.data();
    out.objects = objects.empty() ? nullptr : objects.data();
}

namespace hip {

namespace {
void drop_context();  // destroys the process-wide context and forgets what was said to it (defined beside that state, below)
}

void SetDevices(const std::vector<int> &ordinals) {
    std::lock_guard<std::mutex> lk(g_mu);
    drop_context();
    g_devices = ordinals;
}

bool FogFromEnv() { return env_switch("PATHTRACER_GPU_FOG"); }
int ShadingFromEnv() { return env_lower("PATHTRACER_GPU_SHADING") == "gl" ? PT_SHADING_GL : PT_SHADING_CPU; }
void NoiseFromEnv(double &target, int &step) {
    target = env_double("PATHTRACER_GPU_NOISE", positive_finite, 0);
    step = env_int("PATHTRACER_GPU_NOISE_STEP", 1, 0x7fffffffL, 16);
}
void AdaptiveFromEnv(bool &on, int &min_spp) {
    on = env_switch("PATHTRACER_GPU_ADAPTIVE");
    min_spp = env_int("PATHTRACER_GPU_ADAPTIVE_MIN_SPP", 0, 0x7fffffffL, 0);
}
void AtrousFromEnv(bool &on, int &iterations) {
    on = env_switch("PATHTRACER_GPU_ATROUS");
    iterations = env_int("PATHTRACER_GPU_ATROUS_ITERS", 0, 6, 5);
}
int FeaturesFromEnv() { return env_int("PATHTRACER_GPU_FEATURES", 0, 0x7fffffffL, -1); }
double FilteredNoiseFromEnv() { return env_double("PATHTRACER_GPU_FILTERED_NOISE", positive_finite, 0); }
void FilteredAdaptiveFromEnv(double &target, int &pool) {
    target = env_double("PATHTRACER_GPU_FILTERED_ADAPTIVE", positive_finite, 0);
    pool = env_int("PATHTRACER_GPU_POOL", 0, 4, 1);
}
bool TemporalFromEnv() { return env_switch("PATHTRACER_GPU_TEMPORAL"); }
double TemporalClipFromEnv() { return env_double("PATHTRACER_GPU_TEMPORAL_CLIP", finite_not_negative, 0); }
bool TemporalMotionFromEnv() { return env_switch("PATHTRACER_GPU_TEMPORAL_MOTION"); }
bool FeatureWalkFromEnv() { return env_switch("PATHTRACER_GPU_FEATURE_WALK"); }
bool FogWalkFromEnv() { return env_switch("PATHTRACER_GPU_FOG_WALK"); }
bool ShadingWalkFromEnv() { return env_switch("PATHTRACER_GPU_SHADING_WALK"); }
bool ShadingFeaturesFromEnv() { return env_switch("PATHTRACER_GPU_SHADING_FEATURES"); }
int BvhBuildFromEnv() {  // PATHTRACER_GPU_BVH_BUILD=host|device: anything else is host
    const char *e = std::getenv("PATHTRACER_GPU_BVH_BUILD");
    return e && std::string(e) == "device" ? 1 : 0;
}
double BvhRefitFromEnv() {  // PATHTRACER_GPU_BVH_REFIT=<G>: a growth bound of at least 1, or inf; anything else is off
    return env_double("PATHTRACER_GPU_BVH_REFIT", [](double g) { return g >= 1.0; }, 0);
}

namespace {

// What one frame does, from what was set and, where nothing was, from the environment.  Computed once per Render, under the lock.
struct FramePlan {
    bool fog;             // the scene has a fog block and it was asked for
    int shading;          // PT_SHADING_*
    NoiseRule noise;      // target > 0: render until the frame noise is there
    Switch adaptive;      // on only with a noise target: without one there is nothing to adapt to
    Switch atrous;        // on also under temporal accumulation, which brings the filter with it
    bool temporal;
    double clip;          // > 0 only under temporal accumulation
    bool motion;          // displaced reprojection: on only under temporal accumulation
    double filtered;      // > 0 only under the filter
    BlockRule blocks;     // target > 0 only under the filter: an adaptive frame whose blocks stop by the filtered frame's pooled noise
    int features;
    bool walk;            // features on the BVH path too (pt_set_feature_walk)
    bool fog_walk;        // volumetric fog on the BVH path too (pt_set_fog_walk)
    bool shading_walk;    // GL shading on the BVH path too (pt_set_shading_walk)
    bool shading_features;  // features and the a-trous filter for GL-shaded frames (pt_set_shading_features)
    double refit;         // >= 1: the growth bound of pt_set_bvh_refit; 0: off
    int build;            // the mode of pt_set_bvh_build: 0 host, 1 device
    bool moments, halves;
};

NoiseRule noise_rule(const Settings &s) {
    NoiseRule r;
    NoiseFromEnv(r.target, r.step);
    return s.noise.value_or(r);
}
Switch adaptive_switch(const Settings &s) {
    Switch r;
    AdaptiveFromEnv(r.on, r.n);
    return s.adaptive.value_or(r);
}
BlockRule block_rule(const Settings &s) {
    BlockRule r;
    FilteredAdaptiveFromEnv(r.target, r.pool);
    return s.filtered_adaptive.value_or(r);
}
Switch atrous_switch(const Settings &s) {
    Switch r;
    AtrousFromEnv(r.on, r.n);
    return s.atrous.value_or(r);
}

FramePlan resolve(const scene::Scene &sc, const std::vector<pt_object> &objects, const Settings &s) {
    FramePlan p;
    p.fog = s.fog.value_or(FogFromEnv()) && sc.FogPtr;
    p.shading = s.shading.value_or(ShadingFromEnv());
    p.noise = noise_rule(s);
    p.adaptive = adaptive_switch(s);
    p.adaptive.on = p.adaptive.on && p.noise.target > 0;
    p.atrous = atrous_switch(s);
    p.temporal = s.temporal.value_or(TemporalFromEnv());
    p.clip = p.temporal ? s.temporal_clip.value_or(TemporalClipFromEnv()) : 0;
    p.motion = p.temporal && s.temporal_motion.value_or(TemporalMotionFromEnv());
    p.atrous.on = p.atrous.on || p.temporal;
    p.filtered = p.atrous.on ? s.filtered_noise.value_or(FilteredNoiseFromEnv()) : 0;
    p.blocks = block_rule(s);
    if (!p.atrous.on) p.blocks.target = 0;
    p.features = s.features.value_or(FeaturesFromEnv());
    p.walk = s.feature_walk.value_or(FeatureWalkFromEnv());
    p.fog_walk = s.fog_walk.value_or(FogWalkFromEnv());
    p.shading_walk = s.shading_walk.value_or(ShadingWalkFromEnv());
    p.shading_features = s.shading_features.value_or(ShadingFeaturesFromEnv());
    p.refit = s.bvh_refit.value_or(BvhRefitFromEnv());
    p.build = s.bvh_build.value_or(BvhBuildFromEnv());
    if (p.features < 0 && p.temporal) p.features = 4;  // (pt_temporal needs them: where the frame refuses features, pt_begin says so)
    if (p.features < 0) {  // not said: 4 under the filter unless the frame would refuse them (GL shading, the BVH path without the walk), else off
        p.features = 0;
        const bool gl = p.shading == PT_SHADING_GL;  // (there k counts passes of 16 paths, and the walk that matters is the shading's)
        if (p.atrous.on && (!gl || p.shading_features)) {
            size_t spheres = 0, boxes = 0;
            for (const pt_object &o : objects) {
                spheres += o.type == PT_OBJ_SPHERE || o.type == PT_OBJ_SPHERE_LIGHT;
                boxes += o.type == PT_OBJ_BOX;
            }
            const char *scan = std::getenv("PTCORE_SCAN");
            const bool forced_bvh = scan && (!std::strcmp(scan, "bvh") || !std::strcmp(scan, "verify_bvh"));
            if ((gl ? p.shading_walk : p.walk) || (spheres <= 128 && boxes <= 128 && !forced_bvh)) p.features = gl ? 1 : 4;
        }
    }
    p.moments = p.noise.target > 0 || p.atrous.on;
    p.halves = p.filtered > 0;  // (the block rule's frames collect the half sums by themselves)
    return p;
}

// The scene of the last frame Render accumulated with displaced reprojection on: what scene_motion compares.
struct AccumulatedScene {
    bool valid = false;
    std::vector<pt_material> materials;
    std::vector<pt_object> objects;
    pt_sky sky;
    bool has_fog = false;
    pt_fog fog;
};
AccumulatedScene g_accumulated;
bool g_object_ids_on = false;  // pt_set_object_ids(1) was the last thing said to the context
bool g_block_rule_on = false;  // pt_set_adaptive_filtered(&f) was the last thing said to the context
bool g_feature_walk_on = false;  // pt_set_feature_walk(1) was the last thing said to the context
bool g_fog_walk_on = false;      // pt_set_fog_walk(1) was the last thing said to the context
bool g_shading_walk_on = false;  // pt_set_shading_walk(1) was the last thing said to the context
bool g_shading_features_on = false;  // pt_set_shading_features(1) was the last thing said to the context
double g_bvh_refit = 0;          // the bound pt_set_bvh_refit was last given (0: never said, or off)
int g_bvh_build = 0;             // the mode pt_set_bvh_build was last given (0: never said, or host)

// Both belong to the context: a new one has object ids off and an empty history.  Called with g_mu held.
void drop_context() {
    if (g_ctx && g_core.handle) g_core.pt_destroy(g_ctx);
    g_ctx = nullptr;
    g_accumulated.valid = false;
    g_object_ids_on = false;
    g_block_rule_on = false;
    g_feature_walk_on = false;
    g_fog_walk_on = false;
    g_shading_walk_on = false;
    g_shading_features_on = false;
    g_bvh_refit = 0;
    g_bvh_build = 0;
}

void remember(const scene::Scene &sc, const Flat &flat, AccumulatedScene &a) {
    a.valid = true;
    a.materials = flat.materials;
    a.objects = flat.objects;
    a.sky = flat.sc.sky;
    a.has_fog = sc.FogPtr != nullptr;
    std::memset(&a.fog, 0, sizeof a.fog);
    if (sc.FogPtr) FlattenFog(*sc.FogPtr, a.fog);
}

// What moved between the remembered scene and this one: true and delta [n][3] (this frame's position minus the remembered one)
// when the two differ in object positions and the camera only; false when anything else differs -- the number, order, type, size
// or material of the objects, the material table, sky, background or fog.
bool scene_motion(const AccumulatedScene &a, const scene::Scene &sc, const Flat &flat, std::vector<double> &delta) {
    AccumulatedScene b;
    remember(sc, flat, b);
    if (a.objects.size() != b.objects.size() || a.materials.size() != b.materials.size() || a.has_fog != b.has_fog) return false;
    if (std::memcmp(&a.sky, &b.sky, sizeof a.sky) || std::memcmp(&a.fog, &b.fog, sizeof a.fog)) return false;
    if (!a.materials.empty() && std::memcmp(a.materials.data(), b.materials.data(), a.materials.size() * sizeof(pt_material))) return false;
    delta.assign(3 * a.objects.size(), 0.0);
    for (size_t i = 0; i < a.objects.size(); i++) {
        const pt_object &x = a.objects[i], &y = b.objects[i];
        if (x.type != y.type || x.material != y.material || std::memcmp(x.size, y.size, sizeof x.size)) return false;
        for (int k = 0; k < 3; k++) delta[3 * i + (size_t)k] = y.position[k] - x.position[k];
    }
    return true;
}

// How the stepping loop of a frame advances and what ends it before the cap.
struct StopRule {
    enum Check { NONE, FRAME_NOISE, FILTERED_NOISE } check;
    int32_t step;          // samples per pt_step
    bool clip_step;        // clipped to what is left of the cap (the noise rules), or not (the preview cadence)
    bool ends_when_stalled;  // adaptive: every block has stopped once a step adds nothing
    int32_t measure_from, stop_from;  // samples done from which the check runs / from which it may end the frame
    double target;
};

}  // namespace

void SetShading(int model) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_set.shading = model == PT_SHADING_GL ? PT_SHADING_GL : PT_SHADING_CPU;
}
int GetShading() {
    std::lock_guard<std::mutex> lk(g_mu);
    return g_set.shading.value_or(ShadingFromEnv());
}
void SetFog(bool on) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_set.fog = on;
}
bool GetFog() {
    std::lock_guard<std::mutex> lk(g_mu);
    return g_set.fog.value_or(FogFromEnv());
}
void SetNoiseTarget(double target, int step) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_set.noise = NoiseRule{target > 0 ? target : 0, step >= 1 ? step : 16};
}
double GetNoiseTarget() {
    std::lock_guard<std::mutex> lk(g_mu);
    return noise_rule(g_set).target;
}
int GetNoiseStep() {
    std::lock_guard<std::mutex> lk(g_mu);
    return noise_rule(g_set).step;
}
void SetAdaptive(bool on, int min_spp) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_set.adaptive = Switch{on, min_spp >= 0 ? min_spp : 0};
}
bool GetAdaptive() {
    std::lock_guard<std::mutex> lk(g_mu);
    return adaptive_switch(g_set).on;
}
int GetAdaptiveMinSpp() {
    std::lock_guard<std::mutex> lk(g_mu);
    return adaptive_switch(g_set).n;
}
void SetAtrous(bool on, int iterations) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_set.atrous = Switch{on, iterations >= 0 && iterations <= 6 ? iterations : 5};
}
bool GetAtrous() {
    std::lock_guard<std::mutex> lk(g_mu);
    return atrous_switch(g_set).on;
}
int GetAtrousIterations() {
    std::lock_guard<std::mutex> lk(g_mu);
    return atrous_switch(g_set).n;
}
void SetFilteredNoise(double target) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_set.filtered_noise = target > 0 ? target : 0;
}
double GetFilteredNoise() {
    std::lock_guard<std::mutex> lk(g_mu);
    return g_set.filtered_noise.value_or(FilteredNoiseFromEnv());
}
void SetFilteredAdaptive(double target, int pool) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_set.filtered_adaptive = BlockRule{target > 0 ? target : 0, pool >= 0 && pool <= 4 ? pool : 1};
}
double GetFilteredAdaptive() {
    std::lock_guard<std::mutex> lk(g_mu);
    return block_rule(g_set).target;
}
int GetPool() {
    std::lock_guard<std::mutex> lk(g_mu);
    return block_rule(g_set).pool;
}
void SetTemporal(bool on) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_set.temporal = on;
}
bool Temporal() {
    std::lock_guard<std::mutex> lk(g_mu);
    return g_set.temporal.value_or(TemporalFromEnv());
}
void ResetTemporal() {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_ctx && g_core.pt_temporal_reset) (void)g_core.pt_temporal_reset(g_ctx);
    g_accumulated.valid = false;
}
void SetTemporalClip(double gamma) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_set.temporal_clip = finite_not_negative(gamma) ? gamma : 0;
}
bool TemporalClipStats(double &gamma, uint64_t &clipped, uint64_t &reprojected) {
    std::lock_guard<std::mutex> lk(g_mu);
    struct pt_temporal_clip_stats cs;
    if (!g_ctx || !g_core.pt_temporal_clip_stats || g_core.pt_temporal_clip_stats(g_ctx, &cs) != PT_OK) return false;
    gamma = cs.gamma;
    clipped = cs.clipped;
    reprojected = cs.reprojected;
    return true;
}
void SetTemporalMotion(bool on) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_set.temporal_motion = on;
}
bool TemporalMotion() {
    std::lock_guard<std::mutex> lk(g_mu);
    return g_set.temporal_motion.value_or(TemporalMotionFromEnv());
}
void SetFeatureWalk(bool on) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_set.feature_walk = on;
}
bool FeatureWalk() {
    std::lock_guard<std::mutex> lk(g_mu);
    return g_set.feature_walk.value_or(FeatureWalkFromEnv());
}
void SetFogWalk(bool on) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_set.fog_walk = on;
}
bool FogWalk() {
    std::lock_guard<std::mutex> lk(g_mu);
    return g_set.fog_walk.value_or(FogWalkFromEnv());
}
void SetShadingWalk(bool on) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_set.shading_walk = on;
}
bool ShadingWalk() {
    std::lock_guard<std::mutex> lk(g_mu);
    return g_set.shading_walk.value_or(ShadingWalkFromEnv());
}
void SetShadingFeatures(bool on) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_set.shading_features = on;
}
bool ShadingFeatures() {
    std::lock_guard<std::mutex> lk(g_mu);
    return g_set.shading_features.value_or(ShadingFeaturesFromEnv());
}
void SetBvhRefit(double max_growth) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_set.bvh_refit = max_growth >= 1.0 ? max_growth : 0.0;
}
double BvhRefit() {
    std::lock_guard<std::mutex> lk(g_mu);
    return g_set.bvh_refit.value_or(BvhRefitFromEnv());
}
void SetBvhBuild(int mode) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_set.bvh_build = mode == 1 ? 1 : 0;
}
int BvhBuild() {
    std::lock_guard<std::mutex> lk(g_mu);
    return g_set.bvh_build.value_or(BvhBuildFromEnv());
}
void SetFeatures(int k) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (k >= 0) g_set.features = k;
    else g_set.features.reset();
}
int GetFeatures() {
    std::lock_guard<std::mutex> lk(g_mu);
    return g_set.features.value_or(FeaturesFromEnv());
}

void Shutdown() {
    std::lock_guard<std::mutex> lk(g_mu);
    drop_context();
}

std::string Render(const scene::Scene &sc, const RenderConfig &cfg, RGBA &img, const std::function<void()> &progress,
                   Stats *stats) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (img.Width != cfg.Width || img.Height != cfg.Height) return "";  // renderIntoCPU: silently do nothing (renderer.go:46-49)
    if (!load_core()) return g_core.error;
    std::string err;
    auto failed = [&err](std::string text) { return !(err = std::move(text)).empty(); };  // keeps the text of the call that failed
    if (!g_ctx) {
        int32_t n = g_devices.empty() ? 1 : (int32_t)g_devices.size();
        std::vector<int32_t> ords(g_devices.begin(), g_devices.end());
        if (failed(PT_CALL(pt_create, ords.empty() ? nullptr : ords.data(), n, &g_ctx))) return err;
    }
    Flat flat;
    FlattenScene(sc, flat.materials, flat.objects, flat.sc);
    const FramePlan p = resolve(sc, flat.objects, g_set);
    const bool gl = p.shading == PT_SHADING_GL, to_noise = p.noise.target > 0, to_filtered = p.filtered > 0, to_blocks = p.blocks.target > 0;
    const bool adaptive = p.adaptive.on || to_blocks;  // the block rule's frame is an adaptive one, with its own target
    const char *missing = nullptr;  // the text of the last need that was not met
    auto lacks = [&missing](bool wanted, Feature f) { return wanted && !kNeeds[f].have(g_core) && (missing = kNeeds[f].lacks); };

    // ---- the plan onto the context: each check stands in front of the first call that depends on it
    pt_fog fog;
    if (p.fog) FlattenFog(*sc.FogPtr, fog);
    if (failed(PT_CALL(pt_set_fog, g_ctx, p.fog ? &fog : nullptr))) return err;
    if (lacks(gl, GL_SHADING)) return missing;
    std::vector<pt_gl_material> gl_mats;
    if (g_core.pt_set_shading) {
        pt_shading sh;
        std::memset(&sh, 0, sizeof sh);
        sh.model = p.shading;
        if (gl) {
            FlattenGlMaterials(sc, gl_mats);
            sh.num_materials = (int32_t)gl_mats.size();
            sh.materials = gl_mats.data();
        }
        if (failed(PT_CALL(pt_set_shading, g_ctx, gl ? &sh : nullptr))) return err;
    }
    if (lacks(to_noise, NOISE_TARGET)) return missing;
    if (lacks(p.temporal, TEMPORAL)) return missing;
    if (lacks(p.clip > 0, TEMPORAL_CLIP)) return missing;
    if (lacks(p.motion, TEMPORAL_MOTION)) return missing;
    if (lacks(p.atrous.on, ATROUS)) return missing;
    if (to_filtered && to_noise) return "filtered noise target: excludes a frame noise target (-noise) and adaptive sampling: one stop rule per frame";
    if (to_filtered && gl && !p.shading_features) return "filtered noise target: not available with GL shading";
    if (lacks(to_filtered, FILTERED_NOISE)) return missing;
    if (to_blocks && (to_noise || to_filtered))
        return "filtered adaptive target: excludes a frame noise target (-noise), adaptive sampling and the filtered noise target: one stop rule per frame";
    if (to_blocks && gl) return "filtered adaptive target: not available with GL shading";
    if (lacks(to_blocks, FILTERED_ADAPTIVE)) return missing;
    if (g_core.pt_set_halves && failed(PT_CALL(pt_set_halves, g_ctx, p.halves ? 1 : 0))) return err;
    if (lacks(p.features > 0, FEATURES)) return missing;
    if (lacks(p.walk, FEATURE_WALK)) return missing;
    if (p.walk != g_feature_walk_on) {  // (said only when the switch changes: with it never on, the calls are what they were)
        if (failed(PT_CALL(pt_set_feature_walk, g_ctx, p.walk ? 1 : 0))) return err;
        g_feature_walk_on = p.walk;
    }
    if (lacks(p.refit > 0, BVH_REFIT)) return missing;
    if (p.refit != g_bvh_refit) {  // (the same: said only when the bound changes)
        if (failed(PT_CALL(pt_set_bvh_refit, g_ctx, p.refit))) return err;
        g_bvh_refit = p.refit;
    }
    if (lacks(p.build != 0, BVH_BUILD)) return missing;
    if (p.build != g_bvh_build) {  // (the same: said only when the mode changes)
        if (failed(PT_CALL(pt_set_bvh_build, g_ctx, p.build))) return err;
        g_bvh_build = p.build;
    }
    if (lacks(p.fog_walk, FOG_WALK)) return missing;
    if (p.fog_walk != g_fog_walk_on) {  // (the same: said only when the switch changes)
        if (failed(PT_CALL(pt_set_fog_walk, g_ctx, p.fog_walk ? 1 : 0))) return err;
        g_fog_walk_on = p.fog_walk;
    }
    if (lacks(p.shading_walk, SHADING_WALK)) return missing;
    if (p.shading_walk != g_shading_walk_on) {  // (the same)
        if (failed(PT_CALL(pt_set_shading_walk, g_ctx, p.shading_walk ? 1 : 0))) return err;
        g_shading_walk_on = p.shading_walk;
    }
    if (lacks(p.shading_features, SHADING_FEATURES)) return missing;
    if (p.shading_features != g_shading_features_on) {  // (the same)
        if (failed(PT_CALL(pt_set_shading_features, g_ctx, p.shading_features ? 1 : 0))) return err;
        g_shading_features_on = p.shading_features;
    }
    if (g_core.pt_set_features && failed(PT_CALL(pt_set_features, g_ctx, p.features))) return err;
    if (p.motion != g_object_ids_on) {  // (said only when the switch changes: with it never on, the calls are what they were)
        if (failed(PT_CALL(pt_set_object_ids, g_ctx, p.motion ? 1 : 0))) return err;
        g_object_ids_on = p.motion;
    }
    if (g_core.pt_set_moments && failed(PT_CALL(pt_set_moments, g_ctx, p.moments ? 1 : 0))) return err;
    if (lacks(p.adaptive.on, ADAPTIVE)) return missing;
    if (g_core.pt_set_adaptive) {
        pt_adaptive ad;
        std::memset(&ad, 0, sizeof ad);
        ad.target = to_blocks ? p.blocks.target : p.noise.target;
        ad.min_spp = p.adaptive.n;
        ad.step = p.noise.step;
        if (failed(PT_CALL(pt_set_adaptive, g_ctx, adaptive ? &ad : nullptr))) return err;
    }
    if (to_blocks || g_block_rule_on) {  // (said only where it was ever on: with it never on, the calls are what they were)
        pt_adaptive_filtered fa;
        std::memset(&fa, 0, sizeof fa);
        fa.filter = pt_atrous_config{p.atrous.n, 0, 4.0, 0.1, 0.1, 0.2};
        fa.pool = p.blocks.pool;
        if (failed(PT_CALL(pt_set_adaptive_filtered, g_ctx, to_blocks ? &fa : nullptr))) return err;
        g_block_rule_on = to_blocks;
    }

    // ---- the frame: pt_render, or one stepping loop under the frame's stop rule
    pt_config pc;
    std::memset(&pc, 0, sizeof pc);
    pc.width = cfg.Width;
    pc.height = cfg.Height;
    pc.samples_per_px = cfg.SamplesPerPx;
    pc.max_depth = cfg.MaxDepth;
    pc.seed = cfg.Seed;
    const pt_atrous_config filter = {p.atrous.n, 0, 4.0, 0.1, 0.1, 0.2};  // the filter's configuration, for the check and the finish alike
    pt_stats st;
    std::memset(&st, 0, sizeof st);
    pt_noise nz;
    std::memset(&nz, 0, sizeof nz);
    pt_halves_stats hs;
    std::memset(&hs, 0, sizeof hs);
    struct pt_adaptive_state as;
    std::memset(&as, 0, sizeof as);
    int32_t done = cfg.SamplesPerPx > 0 ? cfg.SamplesPerPx : 0;
    int32_t block_checks = 0;
    if (!to_filtered && !to_noise && !progress) {  // (the block rule's frame steps inside pt_render, like every adaptive one)
        err = PT_CALL(pt_render, g_ctx, &flat.sc, &pc, img.Pix.data(), img.Stride, nullptr, nullptr, nullptr, &st);
        if (to_blocks && err.empty()) err = PT_CALL(pt_adaptive_state, g_ctx, &as);
        if (to_blocks && err.empty()) done = as.spp_max;
    } else {
        // filtered noise: each half needs two samples for its variance, so the check runs from 4 on.  frame noise: the check follows
        // every step and may end the frame from 2 on -- never when adaptive, where the blocks stop inside pt_step.  Otherwise the
        // preview cadence: a refresh every spp/10 samples and once at the end (gpu.go:2209-2212, :2229, :2523-2525).
        const int32_t never = INT32_MAX, preview_step = cfg.SamplesPerPx / 10 > 0 ? cfg.SamplesPerPx / 10 : 1;
        //                                 check                     step          clip_step  ends_when_stalled  measure_from  stop_from  target
        const StopRule rule = to_blocks   ? StopRule{StopRule::NONE,           p.noise.step, true,  true,          0, 0,                         0}
                              : to_filtered ? StopRule{StopRule::FILTERED_NOISE, p.noise.step, true,  false,         4, 4,                         p.filtered}
                              : to_noise  ? StopRule{StopRule::FRAME_NOISE,    p.noise.step, true,  p.adaptive.on, 0, p.adaptive.on ? never : 2, p.noise.target}
                                          : StopRule{StopRule::NONE,           preview_step, false, false,         0, 0,                         0};
        if (failed(PT_CALL(pt_begin, g_ctx, &flat.sc, &pc))) return err;
        done = 0;
        while (err.empty() && done < cfg.SamplesPerPx) {
            const int32_t left = cfg.SamplesPerPx - done, before = done;
            if (failed(PT_CALL(pt_step, g_ctx, rule.clip_step && left < rule.step ? left : rule.step, &done))) break;
            if (rule.ends_when_stalled && done == before) break;
            if (progress) {
                if (failed(PT_CALL(pt_read, g_ctx, img.Pix.data(), img.Stride, nullptr))) break;
                progress();
            }
            if (rule.check == StopRule::NONE || done < rule.measure_from) continue;
            double measured;
            if (rule.check == StopRule::FRAME_NOISE) {
                err = PT_CALL(pt_noise_estimate, g_ctx, &nz);
                measured = nz.noise;
            } else {
                err = PT_CALL(pt_atrous_halves, g_ctx, &filter, nullptr, nullptr, nullptr, &hs);
                measured = hs.noise;
            }
            if (err.empty() && done >= rule.stop_from && measured <= rule.target) break;
        }
        if (adaptive && err.empty()) err = PT_CALL(pt_adaptive_state, g_ctx, &as);
        if (err.empty() && (!progress || cfg.SamplesPerPx <= 0)) err = PT_CALL(pt_read, g_ctx, img.Pix.data(), img.Stride, nullptr);
        const int32_t end_rc = g_core.pt_end(g_ctx, &st);  // (the frame is released whatever went wrong before)
        if (err.empty()) err = call("pt_end", end_rc);
        if (err.empty() && progress) progress();
    }

    if (to_blocks && err.empty() && done >= (p.adaptive.n > 4 ? p.adaptive.n : 4))
        err = PT_CALL(pt_read_block_figures, g_ctx, nullptr, nullptr, &block_checks);

    // ---- the finish: the accumulated or the filtered image takes the place of the plain one (the sums stay readable after pt_end)
    pt_atrous_stats ats;
    std::memset(&ats, 0, sizeof ats);
    pt_temporal_stats tst;
    std::memset(&tst, 0, sizeof tst);
    struct pt_temporal_clip_stats tcs;
    std::memset(&tcs, 0, sizeof tcs);
    struct pt_temporal_motion_stats tms;
    std::memset(&tms, 0, sizeof tms);
    bool motion_reset = false, motion_table = false;
    if (p.temporal && err.empty()) {  // the frame blended into the context's reprojected history, then filtered
        if (g_core.pt_temporal_set_clip) err = PT_CALL(pt_temporal_set_clip, g_ctx, p.clip);
        if (p.motion && err.empty() && g_accumulated.valid) {  // the host rule of displaced reprojection
            std::vector<double> delta;
            if (!scene_motion(g_accumulated, sc, flat, delta)) {
                err = PT_CALL(pt_temporal_reset, g_ctx);
                motion_reset = true;
            } else if (std::any_of(delta.begin(), delta.end(), [](double d) { return d != 0.0; })) {
                err = PT_CALL(pt_temporal_set_motion, g_ctx, delta.data(), (int32_t)(delta.size() / 3));
                motion_table = true;
            }
        }
        if (err.empty()) err = PT_CALL(pt_temporal, g_ctx, nullptr, &filter, img.Pix.data(), img.Stride, nullptr, nullptr, &tst);
        if (err.empty() && p.clip > 0) err = PT_CALL(pt_temporal_clip_stats, g_ctx, &tcs);
        if (err.empty() && motion_table) err = PT_CALL(pt_temporal_motion_stats, g_ctx, &tms);
        if (err.empty() && p.motion) remember(sc, flat, g_accumulated);
        if (!p.motion) g_accumulated.valid = false;  // (frames accumulated without the rule are not what the next table is against)
        ats.atrous_ms = tst.temporal_ms;
        ats.noise_before = tst.noise_before;
        ats.noise_after = tst.noise_after;
    } else if (p.atrous.on && err.empty()) {
        err = PT_CALL(pt_atrous, g_ctx, &filter, img.Pix.data(), img.Stride, nullptr, nullptr, &ats);
    }
    if (stats && err.empty()) {
        stats->atrous = p.atrous.on;
        stats->features = p.features;
        stats->atrous_ms = ats.atrous_ms;
        stats->noise_before = ats.noise_before;
        stats->noise_after = ats.noise_after;
        stats->temporal = p.temporal;
        stats->reprojected = tst.reprojected;
        stats->disoccluded = tst.disoccluded;
        stats->temporal_ms = tst.temporal_ms;
        stats->mean_len = tst.mean_len;
        stats->noise_blended = tst.noise_blended;
        stats->temporal_clip = tcs.gamma;
        stats->clipped = tcs.clipped;
        stats->motion_objects = tms.objects;
        stats->moved = tms.moved;
        stats->moved_reprojected = tms.moved_reprojected;
        stats->motion_reset = motion_reset;
        stats->to_filtered_noise = to_filtered;
        stats->filtered_noise = hs.noise;
        stats->noise_model = hs.noise_model;
        stats->samples = st.samples; stats->segments = st.segments; stats->exit_scans = st.exit_scans; stats->draws = st.draws;
        stats->seconds = st.seconds; stats->trace_ms = st.trace_ms; stats->resolve_ms = st.resolve_ms;
        stats->device_ms = st.device_ms; stats->num_devices = st.num_devices; stats->spp_chunk = st.spp_chunk;
        stats->spp_done = done;
        stats->noise = nz.noise;  // (stays 0 without a noise target: the check never ran)
        stats->adaptive = adaptive;
        stats->to_filtered_adaptive = to_blocks;
        stats->pool = to_blocks ? p.blocks.pool : 0;
        stats->block_checks = block_checks;
        stats->blocks = as.blocks;
        stats->active_blocks = as.active_blocks;
        stats->spp_min = as.spp_min;
    }
    return err;
}

}  // namespace hip

void RenderInto(const scene::Scene &sc, const RenderConfig &cfg, RGBA &img, const std::function<void()> &progress,
                Stats *stats) {
    if (GetBackend() != BackendGPU)
        throw std::runtime_error("BackendCPU is the reference's Go renderer (renderIntoCPU) and is not part of this host layer");
    std::string err = hip::Render(sc, cfg, img, progress, stats);
    if (!err.empty()) {
        // the reference prints this and falls back to its CPU renderer (renderer.go:257-262); that fallback
        // lives in the reference, so here the error is surfaced
        std::fprintf(stderr, "GPU render error: %s\n", err.c_str());
        throw std::runtime_error("GPU render error: " + err);
    }
}

RGBA Render(const scene::Scene &sc, const RenderConfig &cfg) {
    RGBA img = NewRGBA(cfg.Width, cfg.Height);
    RenderInto(sc, cfg, img, nullptr);
    return img;
}

RGBA RenderScene(const scene::Scene &sc, const scene::RenderSettings &s, uint64_t seed) {
    RenderConfig cfg;
    cfg.Width = s.Width;
    cfg.Height = s.Height;
    cfg.SamplesPerPx = s.SamplesPerPx;
    cfg.MaxDepth = s.MaxDepth;
    cfg.Seed = seed;
    return Render(sc, cfg);
}

scene::RenderSettings RenderSettingsForMode(const std::string &mode) {
    scene::RenderSettings s;
    if (mode == "final") { s.Width = 1920; s.Height = 1080; s.SamplesPerPx = 1000; s.MaxDepth = 80; }
    else { s.Width = 400; s.Height = 225; s.SamplesPerPx = 20; s.MaxDepth = 20; }
    return s;
}

scene::RenderSettings RenderSettingsForScene(const scene::Scene &sc, const std::string &mode) {
    scene::RenderSettings s = RenderSettingsForMode(mode);  // baseSettings, app.go:60
    if (sc.Settings.Width > 0 && sc.Settings.Height > 0) {  // app.go:61-70
        s.Width = sc.Settings.Width;
        s.Height = sc.Settings.Height;
        if (sc.Settings.SamplesPerPx > 0) s.SamplesPerPx = sc.Settings.SamplesPerPx;
        if (sc.Settings.MaxDepth > 0) s.MaxDepth = sc.Settings.MaxDepth;
    }
    if (mode == "final") {  // finalSettings, app.go:72-75
        s.SamplesPerPx *= 4;
        s.MaxDepth *= 2;
    }
    return s;
}

void SavePNG(const std::string &path, const RGBA &img) {
    std::ofstream f(path, std::ios::binary | std::ios::trunc);
    if (!f) throw std::runtime_error("create png: open " + path + ": " + std::strerror(errno));
    std::vector<uint8_t> data = EncodePNG(img.Pix.data(), img.Width, img.Height, img.Stride);
    f.write(reinterpret_cast<const char *>(data.data()), (std::streamsize)data.size());
    if (!f) throw std::runtime_error("encode png: write failed");
}

}  // namespace engine
}  // namespace pthost
