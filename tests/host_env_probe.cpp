// host_env_probe.cpp -- a stand-alone program over csrc/host/engine.hpp for the CPU tests.
//   host_env_probe env VALUE...   every *FromEnv with all PATHTRACER_GPU_* variables set to VALUE ("<unset>": removed), one line each
//   host_env_probe set            the Set* / Get* pairs: what out-of-range arguments are clamped to, and the environment behind "not set"
//   host_env_probe stats SCENE SPP PROGRESS   hip::Render against the library PTCORE_LIB names; prints every engine::Stats field
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>

#include "host/engine.hpp"

using namespace pthost;
namespace hip = pthost::engine::hip;

static const char *VARS[] = {"FOG", "SHADING", "NOISE", "NOISE_STEP", "ADAPTIVE", "ADAPTIVE_MIN_SPP", "ATROUS", "ATROUS_ITERS", "FEATURES",
                             "FILTERED_NOISE", "TEMPORAL", "TEMPORAL_CLIP"};

static void set_all(const char *v) {
    for (const char *k : VARS) {
        std::string name = std::string("PATHTRACER_GPU_") + k;
        if (v) setenv(name.c_str(), v, 1);
        else unsetenv(name.c_str());
    }
}

static void print_env(const char *label) {
    double nt, fn = hip::FilteredNoiseFromEnv(), clip = hip::TemporalClipFromEnv();
    int ns, ms, it;
    bool ad, at;
    hip::NoiseFromEnv(nt, ns);
    hip::AdaptiveFromEnv(ad, ms);
    hip::AtrousFromEnv(at, it);
    std::printf("[%s] fog=%d shading=%d noise=%.17g step=%d adaptive=%d min_spp=%d atrous=%d iters=%d features=%d filtered=%.17g temporal=%d clip=%.17g\n",
                label, (int)hip::FogFromEnv(), hip::ShadingFromEnv(), nt, ns, (int)ad, ms, (int)at, it, hip::FeaturesFromEnv(), fn,
                (int)hip::TemporalFromEnv(), clip);
}

static void print_get(const char *label) {
    std::printf("[%s] fog=%d shading=%d noise=%.17g step=%d adaptive=%d min_spp=%d atrous=%d iters=%d features=%d filtered=%.17g temporal=%d\n", label,
                (int)hip::GetFog(), hip::GetShading(), hip::GetNoiseTarget(), hip::GetNoiseStep(), (int)hip::GetAdaptive(), hip::GetAdaptiveMinSpp(),
                (int)hip::GetAtrous(), hip::GetAtrousIterations(), hip::GetFeatures(), hip::GetFilteredNoise(), (int)hip::Temporal());
}

int main(int argc, char **argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "env")) {
        for (int i = 2; i < argc; i++) {
            set_all(std::strcmp(argv[i], "<unset>") ? argv[i] : nullptr);
            print_env(argv[i]);
        }
        return 0;
    }
    if (argc >= 2 && !std::strcmp(argv[1], "set")) {
        set_all("1");
        print_get("nothing set, environment 1");
        set_all(nullptr);
        print_get("nothing set, environment empty");
        set_all("1");
        hip::SetFog(false); hip::SetShading(7); hip::SetNoiseTarget(-2.0, 0); hip::SetAdaptive(false, -3); hip::SetAtrous(false, 7);
        hip::SetFeatures(-9); hip::SetFilteredNoise(-1.0); hip::SetTemporal(false);
        print_get("out of range over environment 1");  // (SetFeatures(-9) is "not said": the environment's 1)
        hip::SetFog(true); hip::SetShading(PT_SHADING_GL); hip::SetNoiseTarget(0.25, 3); hip::SetAdaptive(true, 2); hip::SetAtrous(true, 0);
        hip::SetFeatures(0); hip::SetFilteredNoise(0.5); hip::SetTemporal(true);
        set_all(nullptr);
        print_get("in range over environment empty");
        hip::SetNoiseTarget(std::numeric_limits<double>::quiet_NaN(), -1);
        hip::SetAtrous(true, 6);
        print_get("NaN target, 6 iterations");
        return 0;
    }
    if (argc == 5 && !std::strcmp(argv[1], "stats")) {
        std::unique_ptr<scene::Scene> sc = scene::Load(argv[2]);
        engine::RenderConfig cfg;
        cfg.Width = 8; cfg.Height = 8; cfg.SamplesPerPx = std::atoi(argv[3]); cfg.MaxDepth = 3; cfg.Seed = 5;
        engine::RGBA img = engine::NewRGBA(8, 8);
        engine::Stats st;
        int calls = 0;
        std::function<void()> cb;
        if (std::atoi(argv[4])) cb = [&calls]() { calls++; };
        const std::string err = hip::Render(*sc, cfg, img, cb, &st);
        std::printf("error=%s\nprogress_calls=%d pixel0=%d,%d\n", err.c_str(), calls, img.Pix[0], img.Pix[3]);
        std::printf("samples=%llu segments=%llu exit_scans=%llu draws=%llu seconds=%g trace_ms=%g resolve_ms=%g device_ms=%g num_devices=%d spp_chunk=%d\n",
                    (unsigned long long)st.samples, (unsigned long long)st.segments, (unsigned long long)st.exit_scans, (unsigned long long)st.draws,
                    st.seconds, st.trace_ms, st.resolve_ms, st.device_ms, st.num_devices, st.spp_chunk);
        std::printf("spp_done=%d noise=%g adaptive=%d blocks=%llu active_blocks=%llu spp_min=%d\n", st.spp_done, st.noise, (int)st.adaptive,
                    (unsigned long long)st.blocks, (unsigned long long)st.active_blocks, st.spp_min);
        std::printf("atrous=%d features=%d atrous_ms=%g noise_before=%g noise_after=%g to_filtered_noise=%d filtered_noise=%g noise_model=%g\n",
                    (int)st.atrous, st.features, st.atrous_ms, st.noise_before, st.noise_after, (int)st.to_filtered_noise, st.filtered_noise,
                    st.noise_model);
        std::printf("temporal=%d reprojected=%llu disoccluded=%llu temporal_ms=%g mean_len=%g noise_blended=%g temporal_clip=%g clipped=%llu\n",
                    (int)st.temporal, (unsigned long long)st.reprojected, (unsigned long long)st.disoccluded, st.temporal_ms, st.mean_len,
                    st.noise_blended, st.temporal_clip, (unsigned long long)st.clipped);
        double g = -1;
        uint64_t c = 0, r = 0;
        const bool ok = hip::TemporalClipStats(g, c, r);
        std::printf("TemporalClipStats=%d gamma=%g clipped=%llu reprojected=%llu\n", (int)ok, g, (unsigned long long)c, (unsigned long long)r);
        hip::ResetTemporal();
        hip::Shutdown();
        return err.empty() ? 0 : 1;
    }
    std::fprintf(stderr, "usage: host_env_probe env VALUE... | set | stats SCENE SPP PROGRESS\n");
    return 2;
}
