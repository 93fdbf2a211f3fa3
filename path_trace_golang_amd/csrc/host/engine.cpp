#include "engine.hpp"

#include <dlfcn.h>

#include <cctype>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <mutex>
#include <stdexcept>

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

struct Core {
    void *handle = nullptr;
    decltype(&pt_abi_version) abi_version = nullptr;
    decltype(&pt_last_error) last_error = nullptr;
    decltype(&pt_create) create = nullptr;
    decltype(&pt_destroy) destroy = nullptr;
    decltype(&pt_render) render = nullptr;
    decltype(&pt_begin) begin = nullptr;
    decltype(&pt_step) step = nullptr;
    decltype(&pt_read) read = nullptr;
    decltype(&pt_end) end = nullptr;
    decltype(&pt_set_fog) set_fog = nullptr;
    decltype(&pt_set_shading) set_shading = nullptr;  // optional (additive to ABI 4): null in an older build
    decltype(&pt_set_moments) set_moments = nullptr;  // optional, as set_shading (the noise target needs all three)
    decltype(&pt_noise_estimate) noise_estimate = nullptr;
    decltype(&pt_set_adaptive) set_adaptive = nullptr;  // optional, as set_shading (adaptive sampling needs both)
    int32_t (*adaptive_state)(pt_ctx *, struct pt_adaptive_state *) = nullptr;
    decltype(&pt_set_features) set_features = nullptr;  // optional, as set_shading (the a-trous filter needs pt_atrous and moments)
    decltype(&pt_atrous) atrous = nullptr;
    decltype(&pt_set_halves) set_halves = nullptr;  // optional, as set_shading (the filtered noise target needs both)
    decltype(&pt_atrous_halves) atrous_halves = nullptr;
    decltype(&pt_temporal) temporal = nullptr;  // optional, as set_shading
    decltype(&pt_temporal_reset) temporal_reset = nullptr;
    decltype(&pt_temporal_set_clip) temporal_set_clip = nullptr;  // optional, as set_shading
    int32_t (*temporal_clip_stats)(pt_ctx *, struct pt_temporal_clip_stats *) = nullptr;
    std::string error;  // sticky load error, like the reference's cached GL init failure (gpu.go:279-286)
};

Core g_core;
pt_ctx *g_ctx = nullptr;
std::vector<int> g_devices;
int g_fog = -1;  // -1: not set yet, PATHTRACER_GPU_FOG decides
int g_shading = -1;  // -1: not set yet, PATHTRACER_GPU_SHADING decides; else PT_SHADING_*
bool g_noise_set = false;  // false: PATHTRACER_GPU_NOISE / _STEP decide
double g_noise_target = 0;
int g_noise_step = 16;
int g_adaptive = -1;  // -1: not set yet, PATHTRACER_GPU_ADAPTIVE / _MIN_SPP decide
int g_adaptive_min_spp = 0;
int g_atrous = -1;  // -1: not set yet, PATHTRACER_GPU_ATROUS / _ITERS decide
int g_atrous_iters = 5;
double g_filtered_noise = -1;  // < 0: not set yet, PATHTRACER_GPU_FILTERED_NOISE decides
int g_temporal = -1;  // -1: not set yet, PATHTRACER_GPU_TEMPORAL decides
double g_temporal_clip = -1;  // < 0: not set yet, PATHTRACER_GPU_TEMPORAL_CLIP decides
int g_features = -1;  // -1: not set yet, PATHTRACER_GPU_FEATURES decides (and without it: 4 under the filter where the scene allows, else 0)
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

template <typename F>
bool sym(void *h, const char *name, F &out, std::string &err) {
    out = reinterpret_cast<F>(dlsym(h, name));
    if (!out) { err = std::string("libptcore.so lacks symbol ") + name; return false; }
    return true;
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
    std::string err;
    Core c;
    c.handle = h;
    if (!(sym(h, "pt_abi_version", c.abi_version, err) && sym(h, "pt_last_error", c.last_error, err) &&
          sym(h, "pt_create", c.create, err) && sym(h, "pt_destroy", c.destroy, err) && sym(h, "pt_render", c.render, err) &&
          sym(h, "pt_begin", c.begin, err) && sym(h, "pt_step", c.step, err) && sym(h, "pt_read", c.read, err) &&
          sym(h, "pt_end", c.end, err) && sym(h, "pt_set_fog", c.set_fog, err))) {
        g_core.error = err;
        dlclose(h);
        return false;
    }
    c.set_shading = reinterpret_cast<decltype(c.set_shading)>(dlsym(h, "pt_set_shading"));
    c.set_moments = reinterpret_cast<decltype(c.set_moments)>(dlsym(h, "pt_set_moments"));
    c.noise_estimate = reinterpret_cast<decltype(c.noise_estimate)>(dlsym(h, "pt_noise_estimate"));
    c.set_adaptive = reinterpret_cast<decltype(c.set_adaptive)>(dlsym(h, "pt_set_adaptive"));
    c.adaptive_state = reinterpret_cast<decltype(c.adaptive_state)>(dlsym(h, "pt_adaptive_state"));
    c.set_features = reinterpret_cast<decltype(c.set_features)>(dlsym(h, "pt_set_features"));
    c.atrous = reinterpret_cast<decltype(c.atrous)>(dlsym(h, "pt_atrous"));
    c.set_halves = reinterpret_cast<decltype(c.set_halves)>(dlsym(h, "pt_set_halves"));
    c.atrous_halves = reinterpret_cast<decltype(c.atrous_halves)>(dlsym(h, "pt_atrous_halves"));
    c.temporal = reinterpret_cast<decltype(c.temporal)>(dlsym(h, "pt_temporal"));
    c.temporal_reset = reinterpret_cast<decltype(c.temporal_reset)>(dlsym(h, "pt_temporal_reset"));
    c.temporal_set_clip = reinterpret_cast<decltype(c.temporal_set_clip)>(dlsym(h, "pt_temporal_set_clip"));
    c.temporal_clip_stats = reinterpret_cast<decltype(c.temporal_clip_stats)>(dlsym(h, "pt_temporal_clip_stats"));
    if (c.abi_version() != PT_ABI_VERSION) {
        g_core.error = "libptcore.so ABI version mismatch";
        dlclose(h);
        return false;
    }
    g_core = c;
    return true;
}

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

void SetDevices(const std::vector<int> &ordinals) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_ctx && g_core.handle) { g_core.destroy(g_ctx); g_ctx = nullptr; }
    g_devices = ordinals;
}

int ShadingFromEnv() {
    const char *e = std::getenv("PATHTRACER_GPU_SHADING");
    if (!e) return PT_SHADING_CPU;
    std::string v(e);
    for (char &ch : v) ch = (char)std::tolower((unsigned char)ch);
    return v == "gl" ? PT_SHADING_GL : PT_SHADING_CPU;
}

void SetShading(int model) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_shading = model == PT_SHADING_GL ? PT_SHADING_GL : PT_SHADING_CPU;
}

int GetShading() {
    std::lock_guard<std::mutex> lk(g_mu);
    return g_shading < 0 ? ShadingFromEnv() : g_shading;
}

bool FogFromEnv() {
    const char *e = std::getenv("PATHTRACER_GPU_FOG");
    if (!e) return false;
    std::string v(e);
    for (char &ch : v) ch = (char)std::tolower((unsigned char)ch);
    return v == "1" || v == "true" || v == "on" || v == "yes";
}

void SetFog(bool on) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_fog = on ? 1 : 0;
}

bool GetFog() {
    std::lock_guard<std::mutex> lk(g_mu);
    return g_fog < 0 ? FogFromEnv() : g_fog == 1;
}

void NoiseFromEnv(double &target, int &step) {
    target = 0;
    step = 16;
    if (const char *e = std::getenv("PATHTRACER_GPU_NOISE")) {
        char *end = nullptr;
        const double v = std::strtod(e, &end);
        if (end != e && *end == 0 && v > 0 && v <= 1.7976931348623157e308) target = v;
    }
    if (const char *e = std::getenv("PATHTRACER_GPU_NOISE_STEP")) {
        char *end = nullptr;
        const long v = std::strtol(e, &end, 10);
        if (end != e && *end == 0 && v >= 1 && v <= 0x7fffffffL) step = (int)v;
    }
}

void SetNoiseTarget(double target, int step) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_noise_set = true;
    g_noise_target = target > 0 ? target : 0;
    g_noise_step = step >= 1 ? step : 16;
}

double GetNoiseTarget() {
    std::lock_guard<std::mutex> lk(g_mu);
    double t;
    int s;
    NoiseFromEnv(t, s);
    return g_noise_set ? g_noise_target : t;
}

int GetNoiseStep() {
    std::lock_guard<std::mutex> lk(g_mu);
    double t;
    int s;
    NoiseFromEnv(t, s);
    return g_noise_set ? g_noise_step : s;
}

void AdaptiveFromEnv(bool &on, int &min_spp) {
    on = false;
    min_spp = 0;
    if (const char *e = std::getenv("PATHTRACER_GPU_ADAPTIVE")) {
        std::string v(e);
        for (char &ch : v) ch = (char)std::tolower((unsigned char)ch);
        on = v == "1" || v == "true" || v == "on" || v == "yes";
    }
    if (const char *e = std::getenv("PATHTRACER_GPU_ADAPTIVE_MIN_SPP")) {
        char *end = nullptr;
        const long v = std::strtol(e, &end, 10);
        if (end != e && *end == 0 && v >= 0 && v <= 0x7fffffffL) min_spp = (int)v;
    }
}

void SetAdaptive(bool on, int min_spp) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_adaptive = on ? 1 : 0;
    g_adaptive_min_spp = min_spp >= 0 ? min_spp : 0;
}

bool GetAdaptive() {
    std::lock_guard<std::mutex> lk(g_mu);
    bool on;
    int m;
    AdaptiveFromEnv(on, m);
    return g_adaptive < 0 ? on : g_adaptive == 1;
}

int GetAdaptiveMinSpp() {
    std::lock_guard<std::mutex> lk(g_mu);
    bool on;
    int m;
    AdaptiveFromEnv(on, m);
    return g_adaptive < 0 ? m : g_adaptive_min_spp;
}

void AtrousFromEnv(bool &on, int &iterations) {
    on = false;
    iterations = 5;
    if (const char *e = std::getenv("PATHTRACER_GPU_ATROUS")) {
        std::string v(e);
        for (char &ch : v) ch = (char)std::tolower((unsigned char)ch);
        on = v == "1" || v == "true" || v == "on" || v == "yes";
    }
    if (const char *e = std::getenv("PATHTRACER_GPU_ATROUS_ITERS")) {
        char *end = nullptr;
        const long v = std::strtol(e, &end, 10);
        if (end != e && *end == 0 && v >= 0 && v <= 6) iterations = (int)v;
    }
}

int FeaturesFromEnv() {
    if (const char *e = std::getenv("PATHTRACER_GPU_FEATURES")) {
        char *end = nullptr;
        const long v = std::strtol(e, &end, 10);
        if (end != e && *end == 0 && v >= 0 && v <= 0x7fffffffL) return (int)v;
    }
    return -1;
}

void SetAtrous(bool on, int iterations) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_atrous = on ? 1 : 0;
    g_atrous_iters = iterations >= 0 && iterations <= 6 ? iterations : 5;
}

bool GetAtrous() {
    std::lock_guard<std::mutex> lk(g_mu);
    bool on;
    int it;
    AtrousFromEnv(on, it);
    return g_atrous < 0 ? on : g_atrous == 1;
}

int GetAtrousIterations() {
    std::lock_guard<std::mutex> lk(g_mu);
    bool on;
    int it;
    AtrousFromEnv(on, it);
    return g_atrous < 0 ? it : g_atrous_iters;
}

double FilteredNoiseFromEnv() {
    if (const char *e = std::getenv("PATHTRACER_GPU_FILTERED_NOISE")) {
        char *end = nullptr;
        const double v = std::strtod(e, &end);
        if (end != e && *end == 0 && v > 0 && v <= 1.7976931348623157e308) return v;
    }
    return 0;
}

void SetFilteredNoise(double target) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_filtered_noise = target > 0 ? target : 0;
}

double GetFilteredNoise() {
    std::lock_guard<std::mutex> lk(g_mu);
    return g_filtered_noise < 0 ? FilteredNoiseFromEnv() : g_filtered_noise;
}

bool TemporalFromEnv() {
    const char *e = std::getenv("PATHTRACER_GPU_TEMPORAL");
    if (!e) return false;
    std::string v(e);
    for (char &c : v) c = (char)std::tolower((unsigned char)c);
    return v == "1" || v == "true" || v == "on" || v == "yes";
}

void SetTemporal(bool on) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_temporal = on ? 1 : 0;
}

bool Temporal() {
    std::lock_guard<std::mutex> lk(g_mu);
    return g_temporal < 0 ? TemporalFromEnv() : g_temporal == 1;
}

void ResetTemporal() {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_ctx && g_core.temporal_reset) (void)g_core.temporal_reset(g_ctx);
}

double TemporalClipFromEnv() {
    const char *e = std::getenv("PATHTRACER_GPU_TEMPORAL_CLIP");
    if (!e || !*e) return 0;
    char *end = nullptr;
    const double g = std::strtod(e, &end);
    return end != e && *end == 0 && std::isfinite(g) && g >= 0 ? g : 0;
}

void SetTemporalClip(double gamma) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_temporal_clip = std::isfinite(gamma) && gamma >= 0 ? gamma : 0;
}

bool TemporalClipStats(double &gamma, uint64_t &clipped, uint64_t &reprojected) {
    std::lock_guard<std::mutex> lk(g_mu);
    struct pt_temporal_clip_stats cs;
    if (!g_ctx || !g_core.temporal_clip_stats || g_core.temporal_clip_stats(g_ctx, &cs) != PT_OK) return false;
    gamma = cs.gamma;
    clipped = cs.clipped;
    reprojected = cs.reprojected;
    return true;
}

void SetFeatures(int k) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_features = k >= 0 ? k : -1;
}

int GetFeatures() {
    std::lock_guard<std::mutex> lk(g_mu);
    return g_features >= 0 ? g_features : FeaturesFromEnv();
}

void Shutdown() {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_ctx && g_core.handle) g_core.destroy(g_ctx);
    g_ctx = nullptr;
}

std::string Render(const scene::Scene &sc, const RenderConfig &cfg, RGBA &img, const std::function<void()> &progress,
                   Stats *stats) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (img.Width != cfg.Width || img.Height != cfg.Height) return "";  // renderIntoCPU: silently do nothing (renderer.go:46-49)
    if (!load_core()) return g_core.error;
    if (!g_ctx) {
        int32_t n = g_devices.empty() ? 1 : (int32_t)g_devices.size();
        std::vector<int32_t> ords(g_devices.begin(), g_devices.end());
        if (g_core.create(ords.empty() ? nullptr : ords.data(), n, &g_ctx) != PT_OK)
            return std::string("pt_create: ") + g_core.last_error();
    }
    Flat flat;
    FlattenScene(sc, flat.materials, flat.objects, flat.sc);
    {  // the scene's fog block when asked for (SetFog / PATHTRACER_GPU_FOG), else off
        const bool fog_on = (g_fog < 0 ? FogFromEnv() : g_fog == 1) && sc.FogPtr;
        pt_fog fog;
        if (fog_on) FlattenFog(*sc.FogPtr, fog);
        if (g_core.set_fog(g_ctx, fog_on ? &fog : nullptr) != PT_OK) return std::string("pt_set_fog: ") + g_core.last_error();
    }
    std::vector<pt_gl_material> gl_mats;
    bool gl_model = false;
    {  // the shading model (SetShading / PATHTRACER_GPU_SHADING): the CPU engine unless GL is asked for
        const int model = g_shading < 0 ? ShadingFromEnv() : g_shading;
        gl_model = model == PT_SHADING_GL;
        if (model == PT_SHADING_GL && !g_core.set_shading) return "GL shading: libptcore.so lacks pt_set_shading";
        if (g_core.set_shading) {
            pt_shading sh;
            std::memset(&sh, 0, sizeof sh);
            sh.model = model;
            if (model == PT_SHADING_GL) {
                FlattenGlMaterials(sc, gl_mats);
                sh.num_materials = (int32_t)gl_mats.size();
                sh.materials = gl_mats.data();
            }
            if (g_core.set_shading(g_ctx, model == PT_SHADING_GL ? &sh : nullptr) != PT_OK)
                return std::string("pt_set_shading: ") + g_core.last_error();
        }
    }
    double noise_target = g_noise_target;
    int noise_step = g_noise_step;
    if (!g_noise_set) NoiseFromEnv(noise_target, noise_step);
    const bool to_noise = noise_target > 0;
    if (to_noise && !(g_core.set_moments && g_core.noise_estimate)) return "noise target: libptcore.so lacks pt_set_moments / pt_noise_estimate";
    // the a-trous filter (SetAtrous / PATHTRACER_GPU_ATROUS) reads the moments, and the feature planes where the scene allows them
    bool atrous = g_atrous == 1;
    int atrous_iters = g_atrous_iters;
    if (g_atrous < 0) AtrousFromEnv(atrous, atrous_iters);
    // temporal accumulation (SetTemporal / PATHTRACER_GPU_TEMPORAL) brings the filter, the moments and the feature planes with it
    const bool temporal = g_temporal < 0 ? TemporalFromEnv() : g_temporal == 1;
    if (temporal && !g_core.temporal) return "temporal accumulation: libptcore.so lacks pt_temporal";
    const double clip = temporal ? (g_temporal_clip < 0 ? TemporalClipFromEnv() : g_temporal_clip) : 0;
    if (clip > 0 && !(g_core.temporal_set_clip && g_core.temporal_clip_stats)) return "temporal clip: libptcore.so lacks pt_temporal_set_clip";
    atrous = atrous || temporal;
    if (atrous && !(g_core.atrous && g_core.set_moments)) return "a-trous filter: libptcore.so lacks pt_atrous / pt_set_moments";
    // a noise target on the filtered frame (SetFilteredNoise / PATHTRACER_GPU_FILTERED_NOISE): the half-buffer sums and pt_atrous_halves
    const double filtered_target = atrous ? (g_filtered_noise < 0 ? FilteredNoiseFromEnv() : g_filtered_noise) : 0;
    const bool to_filtered = filtered_target > 0;
    if (to_filtered && to_noise) return "filtered noise target: excludes a frame noise target (-noise) and adaptive sampling: one stop rule per frame";
    if (to_filtered && gl_model) return "filtered noise target: not available with GL shading";
    if (to_filtered && !(g_core.set_halves && g_core.atrous_halves)) return "filtered noise target: libptcore.so lacks pt_set_halves / pt_atrous_halves";
    if (g_core.set_halves && g_core.set_halves(g_ctx, to_filtered ? 1 : 0) != PT_OK) return std::string("pt_set_halves: ") + g_core.last_error();
    int features = g_features >= 0 ? g_features : FeaturesFromEnv();
    if (features < 0 && temporal) features = 4;  // (pt_temporal needs them: where the frame refuses features, pt_begin says so)
    if (features < 0) {  // not said: 4 under the filter unless the frame would refuse them (GL shading, the BVH path), else off
        features = 0;
        if (atrous && !gl_model) {
            size_t spheres = 0, boxes = 0;
            for (const pt_object &o : flat.objects) {
                spheres += o.type == PT_OBJ_SPHERE || o.type == PT_OBJ_SPHERE_LIGHT;
                boxes += o.type == PT_OBJ_BOX;
            }
            const char *scan = std::getenv("PTCORE_SCAN");
            const bool forced_bvh = scan && (!std::strcmp(scan, "bvh") || !std::strcmp(scan, "verify_bvh"));
            if (spheres <= 128 && boxes <= 128 && !forced_bvh) features = 4;
        }
    }
    if (features > 0 && !g_core.set_features) return "features: libptcore.so lacks pt_set_features";
    if (g_core.set_features && g_core.set_features(g_ctx, features) != PT_OK) return std::string("pt_set_features: ") + g_core.last_error();
    if (g_core.set_moments && g_core.set_moments(g_ctx, to_noise || atrous ? 1 : 0) != PT_OK) return std::string("pt_set_moments: ") + g_core.last_error();
    bool adaptive = g_adaptive == 1;
    int min_spp = g_adaptive_min_spp;
    if (g_adaptive < 0) AdaptiveFromEnv(adaptive, min_spp);
    adaptive = adaptive && to_noise;  // the noise target is the blocks' target; without one there is nothing to adapt to
    if (adaptive && !(g_core.set_adaptive && g_core.adaptive_state)) return "adaptive sampling: libptcore.so lacks pt_set_adaptive / pt_adaptive_state";
    if (g_core.set_adaptive) {
        pt_adaptive ad;
        std::memset(&ad, 0, sizeof ad);
        ad.target = noise_target;
        ad.min_spp = min_spp;
        ad.step = noise_step;
        if (g_core.set_adaptive(g_ctx, adaptive ? &ad : nullptr) != PT_OK) return std::string("pt_set_adaptive: ") + g_core.last_error();
    }
    struct pt_adaptive_state as;
    std::memset(&as, 0, sizeof as);
    pt_config pc;
    std::memset(&pc, 0, sizeof pc);
    pc.width = cfg.Width;
    pc.height = cfg.Height;
    pc.samples_per_px = cfg.SamplesPerPx;
    pc.max_depth = cfg.MaxDepth;
    pc.seed = cfg.Seed;
    pt_stats st;
    std::memset(&st, 0, sizeof st);
    std::string err;
    int32_t spp_done = cfg.SamplesPerPx > 0 ? cfg.SamplesPerPx : 0;
    pt_noise nz;
    std::memset(&nz, 0, sizeof nz);
    pt_halves_stats hs;
    std::memset(&hs, 0, sizeof hs);
    if (to_filtered) {  // render until the measured noise of the filtered frame is at the target, SamplesPerPx as the cap
        if (g_core.begin(g_ctx, &flat.sc, &pc) != PT_OK) return std::string("pt_begin: ") + g_core.last_error();
        const pt_atrous_config ac = {atrous_iters, 0, 4.0, 0.1, 0.1, 0.2};
        int32_t done = 0;
        while (err.empty() && done < cfg.SamplesPerPx) {
            const int32_t left = cfg.SamplesPerPx - done;
            if (g_core.step(g_ctx, noise_step < left ? noise_step : left, &done) != PT_OK) { err = std::string("pt_step: ") + g_core.last_error(); break; }
            if (progress) {
                if (g_core.read(g_ctx, img.Pix.data(), img.Stride, nullptr) != PT_OK) { err = std::string("pt_read: ") + g_core.last_error(); break; }
                progress();
            }
            if (done < 4) continue;  // each half needs two samples for its variance
            if (g_core.atrous_halves(g_ctx, &ac, nullptr, nullptr, nullptr, &hs) != PT_OK) { err = std::string("pt_atrous_halves: ") + g_core.last_error(); break; }
            if (hs.noise <= filtered_target) break;
        }
        if (err.empty() && (!progress || cfg.SamplesPerPx <= 0) && g_core.read(g_ctx, img.Pix.data(), img.Stride, nullptr) != PT_OK)
            err = std::string("pt_read: ") + g_core.last_error();
        if (g_core.end(g_ctx, &st) != PT_OK && err.empty()) err = std::string("pt_end: ") + g_core.last_error();
        if (err.empty() && progress) progress();
        spp_done = done;
    } else if (to_noise) {  // render until the noise target, SamplesPerPx as the cap; the check follows every step
        if (g_core.begin(g_ctx, &flat.sc, &pc) != PT_OK) return std::string("pt_begin: ") + g_core.last_error();
        int32_t done = 0;
        while (err.empty() && done < cfg.SamplesPerPx) {
            const int32_t left = cfg.SamplesPerPx - done, before = done;
            if (g_core.step(g_ctx, noise_step < left ? noise_step : left, &done) != PT_OK) { err = std::string("pt_step: ") + g_core.last_error(); break; }
            if (adaptive && done == before) break;  // every block has stopped: the step added nothing
            if (progress) {
                if (g_core.read(g_ctx, img.Pix.data(), img.Stride, nullptr) != PT_OK) { err = std::string("pt_read: ") + g_core.last_error(); break; }
                progress();
            }
            if (g_core.noise_estimate(g_ctx, &nz) != PT_OK) { err = std::string("pt_noise_estimate: ") + g_core.last_error(); break; }
            if (!adaptive && done >= 2 && nz.noise <= noise_target) break;  // (adaptive: the blocks stop inside pt_step)
        }
        if (adaptive && err.empty() && g_core.adaptive_state(g_ctx, &as) != PT_OK) err = std::string("pt_adaptive_state: ") + g_core.last_error();
        if (err.empty() && (!progress || cfg.SamplesPerPx <= 0) && g_core.read(g_ctx, img.Pix.data(), img.Stride, nullptr) != PT_OK)
            err = std::string("pt_read: ") + g_core.last_error();
        if (g_core.end(g_ctx, &st) != PT_OK && err.empty()) err = std::string("pt_end: ") + g_core.last_error();
        if (err.empty() && progress) progress();
        spp_done = done;
    } else if (!progress) {
        if (g_core.render(g_ctx, &flat.sc, &pc, img.Pix.data(), img.Stride, nullptr, nullptr, nullptr, &st) != PT_OK)
            err = std::string("pt_render: ") + g_core.last_error();
    } else {
        if (g_core.begin(g_ctx, &flat.sc, &pc) != PT_OK) return std::string("pt_begin: ") + g_core.last_error();
        // refresh the preview every spp/10 samples and once at the end (gpu.go:2209-2212, :2229, :2523-2525)
        const int32_t step = cfg.SamplesPerPx / 10 > 0 ? cfg.SamplesPerPx / 10 : 1;
        int32_t done = 0;
        while (err.empty() && done < cfg.SamplesPerPx) {
            if (g_core.step(g_ctx, step, &done) != PT_OK) { err = std::string("pt_step: ") + g_core.last_error(); break; }
            if (g_core.read(g_ctx, img.Pix.data(), img.Stride, nullptr) != PT_OK) { err = std::string("pt_read: ") + g_core.last_error(); break; }
            progress();
        }
        if (err.empty() && cfg.SamplesPerPx <= 0 && g_core.read(g_ctx, img.Pix.data(), img.Stride, nullptr) != PT_OK)
            err = std::string("pt_read: ") + g_core.last_error();
        if (g_core.end(g_ctx, &st) != PT_OK && err.empty()) err = std::string("pt_end: ") + g_core.last_error();
        if (err.empty()) progress();
    }
    pt_atrous_stats ats;
    std::memset(&ats, 0, sizeof ats);
    pt_temporal_stats tst;
    std::memset(&tst, 0, sizeof tst);
    struct pt_temporal_clip_stats tcs;
    std::memset(&tcs, 0, sizeof tcs);
    if (temporal && err.empty()) {  // the frame blended into the context's reprojected history, then filtered
        pt_atrous_config ac = {atrous_iters, 0, 4.0, 0.1, 0.1, 0.2};
        if (g_core.temporal_set_clip && g_core.temporal_set_clip(g_ctx, clip) != PT_OK) err = std::string("pt_temporal_set_clip: ") + g_core.last_error();
        if (err.empty() && g_core.temporal(g_ctx, nullptr, &ac, img.Pix.data(), img.Stride, nullptr, nullptr, &tst) != PT_OK) err = std::string("pt_temporal: ") + g_core.last_error();
        if (err.empty() && clip > 0 && g_core.temporal_clip_stats(g_ctx, &tcs) != PT_OK) err = std::string("pt_temporal_clip_stats: ") + g_core.last_error();
        ats.atrous_ms = tst.temporal_ms;
        ats.noise_before = tst.noise_before;
        ats.noise_after = tst.noise_after;
    } else if (atrous && err.empty()) {  // the filtered image takes the place of the plain finish (the sums stay readable after pt_end)
        pt_atrous_config ac = {atrous_iters, 0, 4.0, 0.1, 0.1, 0.2};
        if (g_core.atrous(g_ctx, &ac, img.Pix.data(), img.Stride, nullptr, nullptr, &ats) != PT_OK) err = std::string("pt_atrous: ") + g_core.last_error();
    }
    if (stats && err.empty()) {
        stats->atrous = atrous;
        stats->features = features;
        stats->atrous_ms = ats.atrous_ms;
        stats->noise_before = ats.noise_before;
        stats->noise_after = ats.noise_after;
        stats->temporal = temporal;
        stats->reprojected = tst.reprojected;
        stats->disoccluded = tst.disoccluded;
        stats->temporal_ms = tst.temporal_ms;
        stats->mean_len = tst.mean_len;
        stats->noise_blended = tst.noise_blended;
        stats->temporal_clip = tcs.gamma;
        stats->clipped = tcs.clipped;
        stats->to_filtered_noise = to_filtered;
        stats->filtered_noise = hs.noise;
        stats->noise_model = hs.noise_model;
        stats->samples = st.samples; stats->segments = st.segments; stats->exit_scans = st.exit_scans; stats->draws = st.draws;
        stats->seconds = st.seconds; stats->trace_ms = st.trace_ms; stats->resolve_ms = st.resolve_ms;
        stats->device_ms = st.device_ms; stats->num_devices = st.num_devices; stats->spp_chunk = st.spp_chunk;
        stats->spp_done = spp_done;
        stats->noise = to_noise ? nz.noise : 0;
        stats->adaptive = adaptive;
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
