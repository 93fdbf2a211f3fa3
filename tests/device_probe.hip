// device_probe.hip -- test-only: the routines of csrc/pt_math.h, pt_fog.h and pt_glshade.h, one at a time, on the gfx950 device.
//
// The headers are included unchanged and compiled with the library's own flags (tests/device_probe_support.py), so what
// runs here is the code libptcore.so ships.  Every extern "C" entry point uploads its arrays, launches one __global__
// wrapper with one lane per element, copies the results back and returns the first HIP status that was not hipSuccess
// (0 = fine).  All lanes of a launch work on one scene: the headers assume wave-uniform object and light counts, and
// their shadow tests leave the object loop by ballot.  No inline assembly.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "pt_glshade.h"

namespace {

constexpr int BLOCK = 256;

#define PROBE_TRY(expr)                          \
    do {                                         \
        const hipError_t e_ = (expr);            \
        if (e_ != hipSuccess && st == hipSuccess) st = e_; \
    } while (0)

// Device copy of a host array; freed with the object.  Any failure is kept in `st` and makes the pointer null.
template <typename T>
struct Buf {
    T *d = nullptr;
    size_t n = 0;
    hipError_t st = hipSuccess;
    Buf(const T *host, size_t count, bool upload) : n(count) {
        PROBE_TRY(hipMalloc(reinterpret_cast<void **>(&d), (count ? count : 1) * sizeof(T)));
        if (st != hipSuccess) { d = nullptr; return; }
        if (upload && count) PROBE_TRY(hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice));
        else PROBE_TRY(hipMemset(d, 0, (count ? count : 1) * sizeof(T)));
    }
    ~Buf() { if (d) (void)hipFree(d); }
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    hipError_t download(T *host) {
        if (st == hipSuccess && n) PROBE_TRY(hipMemcpy(host, d, n * sizeof(T), hipMemcpyDeviceToHost));
        return st;
    }
};

inline unsigned grid_of(int64_t n) { return (unsigned)((n + BLOCK - 1) / BLOCK); }

inline int finish(hipError_t st) {
    PROBE_TRY(hipGetLastError());
    PROBE_TRY(hipDeviceSynchronize());
    return (int)st;
}

enum { U_SIN = 0, U_TAN = 1, U_EXP = 2, U_POW5 = 3, U_SQRT_OUTLINE = 4, U_SQRT_INLINE = 5 };
enum { B_MIN = 0, B_MAX = 1, B_PHASE_HG = 2 };

template <int WHICH>
__global__ __launch_bounds__(BLOCK) void unary_kernel(const double *__restrict__ x, double *__restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const double v = x[i];
    double r;
    if (WHICH == U_SIN) r = ptm::go_sin(v);
    else if (WHICH == U_TAN) r = ptm::go_tan(v);
    else if (WHICH == U_EXP) r = ptm::go_exp(v);
    else if (WHICH == U_POW5) r = ptm::go_pow5(v);
    else if (WHICH == U_SQRT_OUTLINE) r = ptm::f_sqrt<true>(v);
    else r = ptm::f_sqrt<false>(v);
    out[i] = r;
}

template <int WHICH>
__global__ __launch_bounds__(BLOCK) void binary_kernel(const double *__restrict__ a, const double *__restrict__ b,
                                                         double *__restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    out[i] = WHICH == B_MIN ? ptm::go_min(a[i], b[i]) : WHICH == B_MAX ? ptm::go_max(a[i], b[i]) : ptf::phase_hg(a[i], b[i]);
}

__global__ __launch_bounds__(BLOCK) void sincos_kernel(const double *__restrict__ x, double *__restrict__ s, double *__restrict__ c,
                                                         int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    double sv, cv;
    ptm::sincos_pos(x[i], &sv, &cv);
    s[i] = sv;
    c[i] = cv;
}

__global__ __launch_bounds__(BLOCK) void streams_kernel(const uint64_t *__restrict__ keys, int32_t ndraw, uint64_t *__restrict__ state0,
                                                          double *__restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    uint64_t s = ptm::stream_init(ptm::seed_key(keys[3 * i]), keys[3 * i + 1], keys[3 * i + 2]);
    state0[i] = s;
    for (int32_t k = 0; k < ndraw; k++) out[i * ndraw + k] = ptm::stream_next(s);
}

__global__ __launch_bounds__(BLOCK) void hash31_kernel(const double *__restrict__ p, double *__restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    out[i] = ptf::hash31(p[3 * i], p[3 * i + 1], p[3 * i + 2]);
}

__global__ __launch_bounds__(BLOCK) void noise_kernel(const ptf::FogParams P, const double *__restrict__ p, double *__restrict__ out,
                                                        int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    out[i] = ptf::volume_noise(P, p[3 * i], p[3 * i + 1], p[3 * i + 2]);
}

struct InscatterArgs {
    ptf::FogParams P;
    const ptd::DevObj *objs;
    const ptf::FogLight *lights;
    const double *rays;    // [n][6]
    const uint64_t *keys;  // [n][3] seed, pixel, sample
    double *L;             // [n][3]
    uint32_t *cnt;         // [n][3]
    int32_t nobj, nlight, volumetric;
    int64_t n;
};

__global__ __launch_bounds__(BLOCK) void inscatter_kernel(const InscatterArgs A) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= A.n) return;
    ptf::FogCount c = {0u, 0u, 0u};
    double f[3] = {0.0, 0.0, 0.0};
    if (A.volumetric) {
        const double o[3] = {A.rays[6 * i], A.rays[6 * i + 1], A.rays[6 * i + 2]};
        const double d[3] = {A.rays[6 * i + 3], A.rays[6 * i + 4], A.rays[6 * i + 5]};
        const uint64_t rs = ptm::stream_init(ptm::seed_key(A.keys[3 * i] ^ PTF_STREAM_SALT), A.keys[3 * i + 1], A.keys[3 * i + 2]);
        ptf::fog_inscatter(A.P, A.objs, A.nobj, A.lights, A.nlight, o, d, rs, c, f);
    }
    for (int k = 0; k < 3; k++) A.L[3 * i + k] = f[k];
    A.cnt[3 * i] = c.shadow_rays;
    A.cnt[3 * i + 1] = c.draws;
    A.cnt[3 * i + 2] = c.steps;
}

struct PassArgs {
    ptg::GlScene S;
    const int32_t *jobs;  // [n][3] x, y, pass
    double *out;          // [n][3]
    uint64_t *cnt;        // [n][8]
    uint64_t key, fog_key;
    int64_t n;
};

__global__ __launch_bounds__(BLOCK) void pass_kernel(const PassArgs A) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= A.n) return;
    ptg::GlCount c = {0u, 0u, 0u, 0u, 0u};
    ptf::FogCount f = {0u, 0u, 0u};
    double col[3];
    ptg::gl_pass(A.S, A.key, A.fog_key, A.jobs[3 * i], A.jobs[3 * i + 1], (uint32_t)A.jobs[3 * i + 2], c, f, col);
    for (int k = 0; k < 3; k++) A.out[3 * i + k] = col[k];
    const uint64_t v[8] = {c.paths, c.segments, c.shadow_rays, c.probe_rays, c.draws, f.shadow_rays, f.draws, f.steps};
    for (int k = 0; k < 8; k++) A.cnt[8 * i + k] = v[k];
}

// The CPU world of the fog term, converted the way scene_to_world (ptcore.hip) converts it, and its light list.
void fog_world(const pt_scene *sc, std::vector<ptd::DevObj> &objs, std::vector<ptf::FogLight> &lights) {
    for (int32_t i = 0; i < sc->num_objects; i++) {
        const pt_object &o = sc->objects[i];
        ptd::DevObj d = {};
        if (o.type == PT_OBJ_SPHERE || o.type == PT_OBJ_SPHERE_LIGHT) {
            d.kind = ptd::KIND_SPHERE;
            for (int k = 0; k < 3; k++) d.a[k] = o.position[k];
            d.radius = o.size[0];
            d.radius_sq = d.radius * d.radius;
        } else if (o.type == PT_OBJ_PLANE) {
            d.kind = ptd::KIND_PLANE;
            for (int k = 0; k < 3; k++) d.a[k] = o.position[k];
            d.b[1] = 1;
        } else if (o.type == PT_OBJ_BOX) {
            d.kind = ptd::KIND_BOX;
            for (int k = 0; k < 3; k++) { d.a[k] = o.position[k] - o.size[k] * 0.5; d.b[k] = o.position[k] + o.size[k] * 0.5; }
        } else {
            continue;
        }
        objs.push_back(d);
        ptf::FogLight l;
        if (ptf::fog_light_of(*sc, i, l)) lights.push_back(l);
    }
}

template <typename K>
int run_unary(K kernel, const double *x, double *out, int64_t n) {
    if (n <= 0) return 0;
    Buf<double> dx(x, (size_t)n, true), dout(nullptr, (size_t)n, false);
    hipError_t st = dx.st != hipSuccess ? dx.st : dout.st;
    if (st != hipSuccess) return (int)st;
    hipLaunchKernelGGL(kernel, dim3(grid_of(n)), dim3(BLOCK), 0, 0, (const double *)dx.d, dout.d, n);
    const int rc = finish(st);
    if (rc) return rc;
    return (int)dout.download(out);
}

template <typename K>
int run_binary(K kernel, const double *a, const double *b, double *out, int64_t n) {
    if (n <= 0) return 0;
    Buf<double> da(a, (size_t)n, true), db(b, (size_t)n, true), dout(nullptr, (size_t)n, false);
    hipError_t st = da.st != hipSuccess ? da.st : db.st != hipSuccess ? db.st : dout.st;
    if (st != hipSuccess) return (int)st;
    hipLaunchKernelGGL(kernel, dim3(grid_of(n)), dim3(BLOCK), 0, 0, (const double *)da.d, (const double *)db.d, dout.d, n);
    const int rc = finish(st);
    if (rc) return rc;
    return (int)dout.download(out);
}

}  // namespace

extern "C" {

int probe_device_count(int *count) { return (int)hipGetDeviceCount(count); }

// which: 0 go_sin, 1 go_tan, 2 go_exp, 3 go_pow5, 4 f_sqrt<true>, 5 f_sqrt<false>; -1 for anything else
int probe_unary(int which, const double *x, double *out, int64_t n) {
    switch (which) {
        case U_SIN: return run_unary(unary_kernel<U_SIN>, x, out, n);
        case U_TAN: return run_unary(unary_kernel<U_TAN>, x, out, n);
        case U_EXP: return run_unary(unary_kernel<U_EXP>, x, out, n);
        case U_POW5: return run_unary(unary_kernel<U_POW5>, x, out, n);
        case U_SQRT_OUTLINE: return run_unary(unary_kernel<U_SQRT_OUTLINE>, x, out, n);
        case U_SQRT_INLINE: return run_unary(unary_kernel<U_SQRT_INLINE>, x, out, n);
    }
    return -1;
}

// which: 0 go_min(a, b), 1 go_max(a, b), 2 phase_hg(cos_theta = a, g = b)
int probe_binary(int which, const double *a, const double *b, double *out, int64_t n) {
    switch (which) {
        case B_MIN: return run_binary(binary_kernel<B_MIN>, a, b, out, n);
        case B_MAX: return run_binary(binary_kernel<B_MAX>, a, b, out, n);
        case B_PHASE_HG: return run_binary(binary_kernel<B_PHASE_HG>, a, b, out, n);
    }
    return -1;
}

int probe_sincos(const double *x, double *s, double *c, int64_t n) {
    if (n <= 0) return 0;
    Buf<double> dx(x, (size_t)n, true), ds(nullptr, (size_t)n, false), dc(nullptr, (size_t)n, false);
    hipError_t st = dx.st != hipSuccess ? dx.st : ds.st != hipSuccess ? ds.st : dc.st;
    if (st != hipSuccess) return (int)st;
    hipLaunchKernelGGL(sincos_kernel, dim3(grid_of(n)), dim3(BLOCK), 0, 0, (const double *)dx.d, ds.d, dc.d, n);
    int rc = finish(st);
    if (rc) return rc;
    rc = (int)ds.download(s);
    return rc ? rc : (int)dc.download(c);
}

// keys[i] = {seed, pixel, sample}: state0[i] = stream_init(seed_key(seed), pixel, sample), out[i][0..ndraw) = stream_next
int probe_streams(const uint64_t *keys, int32_t ndraw, uint64_t *state0, double *out, int64_t n) {
    if (n <= 0 || ndraw < 0) return 0;
    Buf<uint64_t> dk(keys, (size_t)n * 3, true), ds(nullptr, (size_t)n, false);
    Buf<double> dout(nullptr, (size_t)n * (size_t)ndraw, false);
    hipError_t st = dk.st != hipSuccess ? dk.st : ds.st != hipSuccess ? ds.st : dout.st;
    if (st != hipSuccess) return (int)st;
    hipLaunchKernelGGL(streams_kernel, dim3(grid_of(n)), dim3(BLOCK), 0, 0, (const uint64_t *)dk.d, ndraw, ds.d, dout.d, n);
    int rc = finish(st);
    if (rc) return rc;
    rc = (int)ds.download(state0);
    return rc ? rc : (int)dout.download(out);
}

int probe_hash31(const double *p, double *out, int64_t n) {
    if (n <= 0) return 0;
    Buf<double> dp(p, (size_t)n * 3, true), dout(nullptr, (size_t)n, false);
    hipError_t st = dp.st != hipSuccess ? dp.st : dout.st;
    if (st != hipSuccess) return (int)st;
    hipLaunchKernelGGL(hash31_kernel, dim3(grid_of(n)), dim3(BLOCK), 0, 0, (const double *)dp.d, dout.d, n);
    const int rc = finish(st);
    return rc ? rc : (int)dout.download(out);
}

int probe_volume_noise(const pt_fog *raw, const double *p, double *out, int64_t n) {
    if (n <= 0) return 0;
    const ptf::FogParams P = ptf::fog_resolve(*raw);
    Buf<double> dp(p, (size_t)n * 3, true), dout(nullptr, (size_t)n, false);
    hipError_t st = dp.st != hipSuccess ? dp.st : dout.st;
    if (st != hipSuccess) return (int)st;
    hipLaunchKernelGGL(noise_kernel, dim3(grid_of(n)), dim3(BLOCK), 0, 0, P, (const double *)dp.d, dout.d, n);
    const int rc = finish(st);
    return rc ? rc : (int)dout.download(out);
}

// The arguments of shim_inscatter_many (tests/fog_support.py): n terms, rays[i] = {o, d}, keys[i] = {seed, pixel, sample}.
int probe_inscatter_many(const pt_scene *sc, const pt_fog *raw, int32_t max_depth, int64_t n, const double *rays,
                         const uint64_t *keys, double *L, uint32_t *cnt) {
    if (n <= 0) return 0;
    std::vector<ptd::DevObj> objs;
    std::vector<ptf::FogLight> lights;
    fog_world(sc, objs, lights);
    InscatterArgs A = {};
    A.P = ptf::fog_resolve(*raw);
    A.volumetric = ptf::fog_volumetric(A.P, max_depth) ? 1 : 0;
    Buf<ptd::DevObj> dobjs(objs.data(), objs.size(), true);
    Buf<ptf::FogLight> dlights(lights.data(), lights.size(), true);
    Buf<double> drays(rays, (size_t)n * 6, true), dL(nullptr, (size_t)n * 3, false);
    Buf<uint64_t> dkeys(keys, (size_t)n * 3, true);
    Buf<uint32_t> dcnt(nullptr, (size_t)n * 3, false);
    hipError_t st = hipSuccess;
    for (hipError_t e : {dobjs.st, dlights.st, drays.st, dL.st, dkeys.st, dcnt.st}) PROBE_TRY(e);
    if (st != hipSuccess) return (int)st;
    A.objs = dobjs.d; A.lights = dlights.d; A.rays = drays.d; A.keys = dkeys.d; A.L = dL.d; A.cnt = dcnt.d;
    A.nobj = (int32_t)objs.size(); A.nlight = (int32_t)lights.size(); A.n = n;
    hipLaunchKernelGGL(inscatter_kernel, dim3(grid_of(n)), dim3(BLOCK), 0, 0, A);
    int rc = finish(st);
    if (rc) return rc;
    rc = (int)dL.download(L);
    return rc ? rc : (int)dcnt.download(cnt);
}

// The arguments of shim_pass_many (tests/glshade_support.py): the scene tables are built on the host by the same gl_*
// calls frame_open (ptcore.hip) makes, and the pointers of GlScene are those of their device copies.
int probe_pass_many(const pt_scene *sc, const pt_gl_material *ex, int32_t w, int32_t h, int32_t depth, uint64_t seed,
                    const pt_fog *fog, int64_t n, const int32_t *jobs, double *out, uint64_t *cnt) {
    if (n <= 0) return 0;
    const int32_t nmat = sc->num_materials;
    std::vector<ptg::GlMat> mats((size_t)(nmat > 0 ? nmat : 1), ptg::GlMat{});
    for (int32_t i = 0; i < nmat; i++) mats[(size_t)i] = ptg::gl_material(sc->materials[i], ex[i]);
    std::vector<ptg::GlObj> objs;
    std::vector<int32_t> lights;
    for (int32_t i = 0; i < sc->num_objects; i++) {
        objs.push_back(ptg::gl_object(sc->objects[i], nmat));
        if (ptg::gl_is_light(*sc, i)) lights.push_back(i);
    }
    PassArgs A = {};
    ptg::GlScene &S = A.S;
    pt_sky sky = sc->sky;
    std::vector<ptd::DevObj> fobjs;
    std::vector<ptf::FogLight> flights;
    if (fog) {
        S.fog = ptf::fog_resolve(*fog);
        if (ptf::fog_sky_applies(S.fog))
            for (double *c : {sky.background, sky.color, sky.horizon, sky.zenith}) ptf::fog_sky_rewrite(S.fog, c);
        S.fog_on = ptf::fog_volumetric(S.fog, depth) ? 1 : 0;
        fog_world(sc, fobjs, flights);
    }
    Buf<ptg::GlObj> dobjs(objs.data(), objs.size(), true);
    Buf<ptg::GlMat> dmats(mats.data(), mats.size(), true);
    Buf<int32_t> dlights(lights.data(), lights.size(), true);
    Buf<ptd::DevObj> dfobjs(fobjs.data(), fobjs.size(), true);
    Buf<ptf::FogLight> dflights(flights.data(), flights.size(), true);
    Buf<int32_t> djobs(jobs, (size_t)n * 3, true);
    Buf<double> dout(nullptr, (size_t)n * 3, false);
    Buf<uint64_t> dcnt(nullptr, (size_t)n * 8, false);
    hipError_t st = hipSuccess;
    for (hipError_t e : {dobjs.st, dmats.st, dlights.st, dfobjs.st, dflights.st, djobs.st, dout.st, dcnt.st}) PROBE_TRY(e);
    if (st != hipSuccess) return (int)st;
    S.objs = dobjs.d; S.mats = dmats.d; S.lights = dlights.d;
    S.nobj = (int32_t)objs.size(); S.nlight = (int32_t)lights.size();
    S.fog_objs = dfobjs.d; S.fog_nobj = (int32_t)fobjs.size();
    S.fog_lights = dflights.d; S.fog_nlight = (int32_t)flights.size();
    S.sky = ptg::gl_sky(sky);
    S.cam = ptg::gl_camera(sc->camera, w, h);
    S.max_depth = depth; S.width = w; S.height = h;
    A.key = ptm::seed_key(seed ^ PTG_STREAM_SALT);
    A.fog_key = ptm::seed_key(seed ^ PTF_STREAM_SALT);
    A.jobs = djobs.d; A.out = dout.d; A.cnt = dcnt.d; A.n = n;
    hipLaunchKernelGGL(pass_kernel, dim3(grid_of(n)), dim3(BLOCK), 0, 0, A);
    int rc = finish(st);
    if (rc) return rc;
    rc = (int)dout.download(out);
    return rc ? rc : (int)dcnt.download(cnt);
}

}  // extern "C"
