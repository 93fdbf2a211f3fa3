// render_main.cpp -- CLI twin of the reference's cmd/render (/root/reference/cmd/render/main.go:14-63)
// for machines without a Go toolchain.  Same five flags with the same defaults and Go's flag syntax
// (-flag value, -flag=value, --flag, boolean -flag / -flag=false); the interactive UI is not part of
// this build, so running without -headless is an error instead of opening a window.
//
// Additive flags (the reference CLI cannot express the benchmark configurations, main.go:52 and
// util.go:25-42 hard-wire two presets): -width -height -spp -depth override the mode preset,
// -seed selects the sample streams (also env PATHTRACER_SEED), -devices N uses N GPUs (0..N-1),
// -scene-settings applies the editor's scene-settings override (internal/ui/app.go:60-75) before them;
// without it scene.settings is ignored exactly as main.go:52 does.  -fog draws the scene's fog block the way the
// reference's OpenGL backend does (sky blend, volumetric in-scatter; also env PATHTRACER_GPU_FOG=1); without it fog is
// ignored like the CPU engine ignores it.  -noise T renders until the frame noise (pt_noise_estimate) is at or
// below T, checking every -noise-step samples, with -spp as the cap (also env PATHTRACER_GPU_NOISE, PATHTRACER_GPU_NOISE_STEP).
// -adaptive makes T the target of every 8x8 block (pt_set_adaptive): blocks stop one by one, each pixel keeps the
// samples its block got; -min-spp N samples every block at least N times first (also env PATHTRACER_GPU_ADAPTIVE, _MIN_SPP).
// -atrous writes the variance-guided a-trous filtered image (pt_atrous) instead of the plain finish, -atrous-iters N
// (0..6) sets its iterations and -features K the first-hit feature samples per pixel that guide it (default: 4 where the scene allows
// them; also env PATHTRACER_GPU_ATROUS, PATHTRACER_GPU_ATROUS_ITERS, PATHTRACER_GPU_FEATURES).  -filtered-noise T (with -atrous)
// renders until the measured noise of the filtered frame (pt_atrous_halves) is at or below T, checking every -noise-step
// samples, with -spp as the cap (also env PATHTRACER_GPU_FILTERED_NOISE); it excludes -noise.  -filtered-adaptive T (with -atrous) stops every
// 8x8 block of an adaptive frame by the filtered frame's noise pooled over the blocks within -pool N (0..4, default 1) blocks of it
// (pt_set_adaptive_filtered; also env PATHTRACER_GPU_FILTERED_ADAPTIVE, PATHTRACER_GPU_POOL); -noise-step and -min-spp
// apply, and it excludes -noise and -filtered-noise.  -feature-walk lets a scene on the bounding-volume-hierarchy path (more than 128
// spheres or 128 boxes) collect features, by a wave-shared walk of the tree (pt_set_feature_walk; also env
// PATHTRACER_GPU_FEATURE_WALK).  -bvh-refit G (G >= 1 or inf) lets a frame whose scene differs from the previous frame's only in where
// its objects are refit the hierarchy on the devices instead of rebuilding it; G bounds how far the tree may degrade before it is
// rebuilt (pt_set_bvh_refit; also env PATHTRACER_GPU_BVH_REFIT).  -bvh-build host|device
// chooses who builds the hierarchy when a full build is due: the host's builder (the default) or devices[0], in Morton order
// (pt_set_bvh_build; also env PATHTRACER_GPU_BVH_BUILD).  -fog-walk (with -fog) lets a scene on the
// bounding-volume-hierarchy path draw a gpu_volumetric fog block, its shadow rays answered by a wave-shared walk of the tree
// (pt_set_fog_walk; also env PATHTRACER_GPU_FOG_WALK).  -shading-walk (with -shading gl) lets such a scene render
// with the GL model, its ray queries answered by the lane's own walk of the tree (pt_set_shading_walk; also env
// PATHTRACER_GPU_SHADING_WALK).  -shading-features (with -shading gl) lets a GL-shaded frame take -features and -atrous, the
// features being those of the GL pass's own camera rays (pt_set_shading_features; also env
// PATHTRACER_GPU_SHADING_FEATURES).  These eight flags are parsed like the others but are
// not in the usage text below, which stands as recorded in tests/golden/host_traces.json.
#include <cerrno>
#include <chrono>
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <map>
#include <string>

#include "engine.hpp"
#include "scene.hpp"

using namespace pthost;

namespace {

void logf(const char *fmt, ...) {  // log.Printf: "2006/01/02 15:04:05 msg" on stderr
    std::time_t t = std::time(nullptr);
    std::tm tm;
    localtime_r(&t, &tm);
    char stamp[32];
    std::strftime(stamp, sizeof stamp, "%Y/%m/%d %H:%M:%S", &tm);
    std::fprintf(stderr, "%s ", stamp);
    va_list ap;
    va_start(ap, fmt);
    std::vfprintf(stderr, fmt, ap);
    va_end(ap);
    std::fputc('\n', stderr);
}

struct Flags {
    std::string scene = "scenes/example_simple.json";
    std::string mode = "preview";
    bool gpu = false;
    bool headless = false;
    bool scene_settings = false;
    bool fog = false;
    std::string shading = "cpu";
    std::string out = "output.png";
    int width = 0, height = 0, spp = -1, depth = -1, devices = 1;
    unsigned long long seed = 1;
    double noise = 0;
    int noise_step = 16;
    bool adaptive = false;
    int min_spp = 0;
    bool atrous = false;
    int atrous_iters = 5;
    int features = -1;  // -1: not said
    double filtered_noise = 0;
    double filtered_adaptive = 0;
    int pool = 1;
    bool feature_walk = false;
    bool fog_walk = false;
    bool shading_walk = false;
    bool shading_features = false;
    double bvh_refit = 0;
    std::string bvh_build = "host";
};

void usage() {
    std::fprintf(stderr,
                 "Usage of render:\n"
                 "  -adaptive\n    \twith -noise: stop every 8x8 block at the target by itself (default false, or PATHTRACER_GPU_ADAPTIVE)\n"
                 "  -atrous\n    \twrite the variance-guided a-trous filtered image (DESIGN 3.11) (default false, or PATHTRACER_GPU_ATROUS)\n"
                 "  -atrous-iters int\n    \twith -atrous: iterations 0..6 (default 5, or PATHTRACER_GPU_ATROUS_ITERS)\n"
                 "  -depth int\n    \tmax path depth (default: the mode preset)\n"
                 "  -devices int\n    \tnumber of GPUs to tile the image over (default 1)\n"
                 "  -features int\n    \tfirst-hit feature samples per pixel (default: 4 with -atrous where the scene allows them, else 0; or\n"
                 "    \tPATHTRACER_GPU_FEATURES)\n"
                 "  -filtered-noise float\n    \twith -atrous: render until the measured noise of the filtered frame (DESIGN 3.12) is at or below this\n"
                 "    \ttarget, checking every -noise-step samples, -spp being the cap (default 0 = off, or PATHTRACER_GPU_FILTERED_NOISE)\n"
                 "  -fog\n    \tdraw the scene's fog block like the reference's GPU backend (default false, or PATHTRACER_GPU_FOG)\n"
                 "  -gpu\n    \tuse GPU backend for rendering (if available)\n"
                 "  -headless\n    \trender without UI and save PNG\n"
                 "  -height int\n    \timage height (default: the mode preset)\n"
                 "  -min-spp int\n    \twith -adaptive: samples every block gets before the first check (default 0, or\n"
                 "    \tPATHTRACER_GPU_ADAPTIVE_MIN_SPP)\n"
                 "  -mode string\n    \trender mode: preview or final (default \"preview\")\n"
                 "  -noise float\n    \trender until the frame noise is at or below this target, -spp being the cap (default 0 = off, or\n"
                 "    \tPATHTRACER_GPU_NOISE)\n"
                 "  -noise-step int\n    \tsamples per pixel between two noise checks (default 16, or PATHTRACER_GPU_NOISE_STEP)\n"
                 "  -out string\n    \toutput PNG file for headless render (default \"output.png\")\n"
                 "  -scene string\n    \tpath to scene JSON file (default \"scenes/example_simple.json\")\n"
                 "  -scene-settings\n    \tlet the scene file's settings block override the mode preset (the editor's rule); with -mode final this also\n"
                 "    \tapplies the editor's Final button (x4 samples, x2 depth, internal/ui/app.go:73-75), which in the editor is\n"
                 "    \tindependent of the preset\n"
                 "  -shading string\n    \tshading model: cpu (the CPU engine) or gl (the reference's GPU shader, DESIGN 3.8) (default \"cpu\", or\n"
                 "    \tPATHTRACER_GPU_SHADING)\n"
                 "  -seed uint\n    \tsample-stream seed (default 1, or PATHTRACER_SEED)\n"
                 "  -spp int\n    \tsamples per pixel (default: the mode preset)\n"
                 "  -width int\n    \timage width (default: the mode preset)\n");
}

bool parse_bool(const std::string &v, bool &out) {
    if (v == "1" || v == "t" || v == "T" || v == "true" || v == "TRUE" || v == "True") { out = true; return true; }
    if (v == "0" || v == "f" || v == "F" || v == "false" || v == "FALSE" || v == "False") { out = false; return true; }
    return false;
}

// One row per flag: its name, how its value is read, and where it goes.  INT rows keep a value inside [lo, hi] and take `fallback`
// for one outside (the plain sizes take any value, as Go's flag.Int does).
enum Kind { BOOL, STRING, SHADING, BUILDER, INT, NOT_NEGATIVE, UINT };
struct FlagRow {
    const char *name;
    Kind kind;
    void *dst;
    long long lo = LLONG_MIN, hi = LLONG_MAX;
    int fallback = 0;
};

int bad_flag(const char *fmt, const std::string &a, const std::string &b = "") {
    std::fprintf(stderr, fmt, a.c_str(), b.c_str());
    usage();
    return 2;
}

// Go's flag package rules
int parse(int argc, char **argv, Flags &f) {
    const FlagRow table[] = {
        {"gpu", BOOL, &f.gpu}, {"headless", BOOL, &f.headless}, {"scene-settings", BOOL, &f.scene_settings}, {"fog", BOOL, &f.fog},
        {"adaptive", BOOL, &f.adaptive}, {"atrous", BOOL, &f.atrous}, {"feature-walk", BOOL, &f.feature_walk}, {"fog-walk", BOOL, &f.fog_walk},
        {"shading-walk", BOOL, &f.shading_walk}, {"shading-features", BOOL, &f.shading_features},
        {"scene", STRING, &f.scene}, {"mode", STRING, &f.mode}, {"out", STRING, &f.out}, {"shading", SHADING, &f.shading},
        {"width", INT, &f.width}, {"height", INT, &f.height}, {"spp", INT, &f.spp}, {"depth", INT, &f.depth}, {"devices", INT, &f.devices},
        {"noise-step", INT, &f.noise_step, 1, 0x7fffffffLL, 16}, {"min-spp", INT, &f.min_spp, 0, 0x7fffffffLL, 0},
        {"atrous-iters", INT, &f.atrous_iters, 0, 6, 5}, {"features", INT, &f.features, 0, 0x7fffffffLL, -1},
        {"noise", NOT_NEGATIVE, &f.noise}, {"filtered-noise", NOT_NEGATIVE, &f.filtered_noise}, {"seed", UINT, &f.seed},
        {"filtered-adaptive", NOT_NEGATIVE, &f.filtered_adaptive}, {"pool", INT, &f.pool, 0, 4, 1},
        {"bvh-refit", NOT_NEGATIVE, &f.bvh_refit}, {"bvh-build", BUILDER, &f.bvh_build},
    };
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        if (a.size() < 2 || a[0] != '-') break;  // first non-flag argument ends parsing
        if (a == "--") break;
        size_t dash = a[1] == '-' ? 2 : 1;
        std::string name = a.substr(dash), val;
        bool has_val = false;
        size_t eq = name.find('=');
        if (eq != std::string::npos) { val = name.substr(eq + 1); name = name.substr(0, eq); has_val = true; }
        if (name == "h" || name == "help") { usage(); return 0; }
        const FlagRow *row = nullptr;
        for (const FlagRow &r : table)
            if (name == r.name) row = &r;
        if (!row) return bad_flag("flag provided but not defined: -%s\n", name);
        if (row->kind == BOOL) {
            bool b = true;
            if (has_val && !parse_bool(val, b)) return bad_flag("invalid boolean value \"%s\" for -%s: parse error\n", val, name);
            *static_cast<bool *>(row->dst) = b;
            continue;
        }
        if (!has_val) {
            if (i + 1 >= argc) return bad_flag("flag needs an argument: -%s\n", name);
            val = argv[++i];
        }
        char *end = nullptr;
        errno = 0;
        switch (row->kind) {
            case STRING:
                *static_cast<std::string *>(row->dst) = val;
                break;
            case SHADING:
                if (val != "cpu" && val != "gl") return bad_flag("invalid value \"%s\" for flag -%s: want cpu or gl\n", val, name);
                *static_cast<std::string *>(row->dst) = val;
                break;
            case BUILDER:
                if (val != "host" && val != "device") return bad_flag("invalid value \"%s\" for flag -%s: want host or device\n", val, name);
                *static_cast<std::string *>(row->dst) = val;
                break;
            case NOT_NEGATIVE: {
                const double v = std::strtod(val.c_str(), &end);
                if (errno || end == val.c_str() || *end || !(v >= 0)) return bad_flag("invalid value \"%s\" for flag -%s: parse error\n", val, name);
                *static_cast<double *>(row->dst) = v;
                break;
            }
            default: {
                const long long n = std::strtoll(val.c_str(), &end, 10);
                if (errno || end == val.c_str() || *end) return bad_flag("invalid value \"%s\" for flag -%s: parse error\n", val, name);
                if (row->kind == UINT) *static_cast<unsigned long long *>(row->dst) = (unsigned long long)n;
                else *static_cast<int *>(row->dst) = n >= row->lo && n <= row->hi ? (int)n : row->fallback;
            }
        }
    }
    return -1;
}

// renderHeadless, main.go:46-63
int render_headless(const Flags &f) {
    std::unique_ptr<scene::Scene> sc;
    try {
        sc = scene::Load(f.scene);
    } catch (const std::exception &e) {
        logf("headless render error: load scene: %s", e.what());
        return 1;
    }
    // scene.settings is ignored, like main.go:52, unless -scene-settings asks for the editor's rule (ui/app.go:60-75)
    scene::RenderSettings s = f.scene_settings ? engine::RenderSettingsForScene(*sc, f.mode) : engine::RenderSettingsForMode(f.mode);
    if (f.width > 0) s.Width = f.width;
    if (f.height > 0) s.Height = f.height;
    if (f.spp >= 0) s.SamplesPerPx = f.spp;
    if (f.depth >= 0) s.MaxDepth = f.depth;
    engine::hip::SetFog(f.fog);
    engine::hip::SetShading(f.shading == "gl" ? PT_SHADING_GL : PT_SHADING_CPU);
    engine::hip::SetNoiseTarget(f.noise, f.noise_step);
    engine::hip::SetAdaptive(f.adaptive, f.min_spp);
    engine::hip::SetAtrous(f.atrous, f.atrous_iters);
    engine::hip::SetFeatures(f.features);
    engine::hip::SetFeatureWalk(f.feature_walk);
    engine::hip::SetFogWalk(f.fog_walk);
    engine::hip::SetShadingWalk(f.shading_walk);
    engine::hip::SetShadingFeatures(f.shading_features);
    engine::hip::SetBvhRefit(f.bvh_refit);
    engine::hip::SetBvhBuild(f.bvh_build == "device" ? 1 : 0);
    engine::hip::SetFilteredNoise(f.filtered_noise);
    engine::hip::SetFilteredAdaptive(f.filtered_adaptive, f.pool);
    if (f.filtered_adaptive > 0 && !f.atrous) logf("filtered-adaptive: no -atrous given, nothing to measure (a plain frame)");
    if (f.filtered_noise > 0 && !f.atrous) logf("filtered-noise: no -atrous given, nothing to measure (a plain frame)");
    if (f.adaptive && !(f.noise > 0)) logf("adaptive: no -noise target given, nothing to adapt to (a plain frame)");
    if (f.shading == "gl") logf("shading: gl (the reference's GPU shader; spp counts passes of 16 paths)");
    if (f.fog) logf("fog: drawing the scene's fog block (%s)", sc->FogPtr ? "present" : "absent: nothing to draw");
    try {
        if (f.devices > 1) {
            std::vector<int> ords;
            for (int i = 0; i < f.devices; i++) ords.push_back(i);
            engine::hip::SetDevices(ords);
        }
        engine::RenderConfig cfg;
        cfg.Width = s.Width; cfg.Height = s.Height; cfg.SamplesPerPx = s.SamplesPerPx; cfg.MaxDepth = s.MaxDepth;
        cfg.Seed = f.seed;
        engine::RGBA img = engine::NewRGBA(cfg.Width, cfg.Height);
        engine::Stats st;
        auto t0 = std::chrono::steady_clock::now();
        engine::RenderInto(*sc, cfg, img, nullptr, &st);
        double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (st.to_filtered_adaptive)  // (PATHTRACER_GPU_FILTERED_ADAPTIVE / PATHTRACER_GPU_POOL with -atrous)
            logf("rendered %dx%d, %d to %d of at most %d spp per 8x8 block (filtered adaptive: pooled target %.6g over %d block(s) around, %llu "
                 "of %llu blocks still above it after %d checks), depth %d on %d GPU(s) in %.3f s: %.1f M segments/s, %.1f M samples/s", cfg.Width,
                 cfg.Height, st.spp_min, st.spp_done, cfg.SamplesPerPx, f.filtered_adaptive, st.pool,
                 (unsigned long long)st.active_blocks, (unsigned long long)st.blocks, st.block_checks, cfg.MaxDepth, st.num_devices, dt,
                 st.segments / dt / 1e6, st.samples / dt / 1e6);
        else if (st.adaptive)
            logf("rendered %dx%d, %d to %d of at most %d spp per 8x8 block (adaptive: block target %.6g, %llu of %llu blocks still above it; "
                 "frame noise %.6g), depth %d on %d GPU(s) in %.3f s: %.1f M segments/s, %.1f M samples/s", cfg.Width, cfg.Height, st.spp_min,
                 st.spp_done, cfg.SamplesPerPx, f.noise, (unsigned long long)st.active_blocks, (unsigned long long)st.blocks, st.noise,
                 cfg.MaxDepth, st.num_devices, dt, st.segments / dt / 1e6, st.samples / dt / 1e6);
        else if (st.to_filtered_noise)
            logf("rendered %dx%d, %d of at most %d spp (filtered noise %.6g measured, %.6g propagated, target %.6g), depth %d on %d GPU(s) in "
                 "%.3f s: %.1f M segments/s, %.1f M samples/s", cfg.Width, cfg.Height, st.spp_done, cfg.SamplesPerPx, st.filtered_noise,
                 st.noise_model, f.filtered_noise, cfg.MaxDepth, st.num_devices, dt, st.segments / dt / 1e6, st.samples / dt / 1e6);
        else if (f.noise > 0)
            logf("rendered %dx%d, %d of at most %d spp (noise %.6g, target %.6g), depth %d on %d GPU(s) in %.3f s: %.1f M segments/s, "
                 "%.1f M samples/s", cfg.Width, cfg.Height, st.spp_done, cfg.SamplesPerPx, st.noise, f.noise, cfg.MaxDepth, st.num_devices, dt,
                 st.segments / dt / 1e6, st.samples / dt / 1e6);
        else
            logf("rendered %dx%d, %d spp, depth %d on %d GPU(s) in %.3f s: %.1f M segments/s, %.1f M samples/s", cfg.Width,
                 cfg.Height, cfg.SamplesPerPx, cfg.MaxDepth, st.num_devices, dt, st.segments / dt / 1e6, st.samples / dt / 1e6);
        if (st.atrous)
            logf("a-trous filter: %d iterations, %d feature samples per pixel, noise %.6g -> %.6g in %.3f ms", f.atrous_iters, st.features,
                 st.noise_before, st.noise_after, st.atrous_ms);
        engine::SavePNG(f.out, img);
    } catch (const std::exception &e) {
        logf("headless render error: %s", e.what());
        engine::hip::Shutdown();
        return 1;
    }
    engine::hip::Shutdown();
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    logf("pathtracer: starting main()");
    Flags f;
    if (const char *e = std::getenv("PATHTRACER_SEED")) f.seed = std::strtoull(e, nullptr, 10);
    f.fog = engine::hip::FogFromEnv();
    f.shading = engine::hip::ShadingFromEnv() == PT_SHADING_GL ? "gl" : "cpu";
    engine::hip::NoiseFromEnv(f.noise, f.noise_step);
    engine::hip::AdaptiveFromEnv(f.adaptive, f.min_spp);
    engine::hip::AtrousFromEnv(f.atrous, f.atrous_iters);
    f.features = engine::hip::FeaturesFromEnv();
    f.feature_walk = engine::hip::FeatureWalkFromEnv();
    f.fog_walk = engine::hip::FogWalkFromEnv();
    f.shading_walk = engine::hip::ShadingWalkFromEnv();
    f.shading_features = engine::hip::ShadingFeaturesFromEnv();
    f.bvh_refit = engine::hip::BvhRefitFromEnv();
    f.bvh_build = engine::hip::BvhBuildFromEnv() ? "device" : "host";
    f.filtered_noise = engine::hip::FilteredNoiseFromEnv();
    engine::hip::FilteredAdaptiveFromEnv(f.filtered_adaptive, f.pool);
    int rc = parse(argc, argv, f);
    if (rc >= 0) return rc;
    logf("flags: scene=%s mode=%s headless=%s out=%s", f.scene.c_str(), f.mode.c_str(), f.headless ? "true" : "false",
         f.out.c_str());
    // main.go:26-30: -gpu selects BackendGPU, otherwise BackendCPU.  Only the GPU branch exists in this
    // build, so without -gpu the render fails with a clear message instead of using a different engine.
    engine::SetBackend(f.gpu ? engine::BackendGPU : engine::BackendCPU);
    if (f.headless) return render_headless(f);
    logf("ui error: the interactive UI (internal/ui) is not part of this build; use -headless");
    return 1;
}
