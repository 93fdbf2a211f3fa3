// walk_probe.hip -- test-only: the two tree walks that answer shadow and segment queries outside the trace kernels, asked ray by ray
// on the gfx950 device.  csrc/pt_gl_walk.h (ptg::TreeWorld: walk_ok, walk_closest, walk_occluded) and csrc/pt_fog_walk.h
// (wave_walk_coop, wave_any_hit, wave_any_hit_plain) are included unchanged and compiled with the library's own flags
// (tests/walk_probe_support.py); this file holds no traversal code of its own.
//
// wp_open builds a scene's tables on the host the way glwalk_support's gw_open does -- gl_material / gl_object, scene_to_world, the
// plane list, ptbvh::build_scene_trees, world_bound + frame_bounds -- sets F.bvh_stack as ptcore.hip rounds it from stack_need, and
// uploads them.
//   probe_gl_queries  one lane per query q[11] = kind (0 closest, 1 occluded), ro, rd, tmin, tmax, skip, unused; the lane's TreeWorld
//                     is gl_bvh_kernel's: stack = its column of the block's dynamic LDS (F.bvh_stack entries, stride PT_BLOCK).
//   probe_fog_turns   one wave per 64 shadow rays r[7] = o, d, tmax with an `active` byte per lane: the shadow turn of fog_walk_body.
// Every output array is GUARD rows longer than the count and filled with 0xFF bytes before the launch.  No inline assembly.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "probe_common.h"
#include "pt_bvh.h"
#include "pt_convert.h"
#include "pt_fog_walk.h"
#include "pt_gl_walk.h"

namespace {

using namespace ptd;

const int64_t GUARD = 64;
const int64_t MAX_QUERIES = (int64_t)1 << 22;

struct Probe {
    std::vector<ptg::GlObj> objs;
    std::vector<int32_t> plane_idx;
    std::vector<DevObj> world;
    std::vector<DevMat> dmats;
    ptbvh::SceneTrees T;
    DevFrame F;
    bool built = false, gl_ok = false;
    std::string why;
    Buf<ptg::GlObj> *d_objs = nullptr;
    Buf<DevObj> *d_world = nullptr;
    Buf<BvhNode> *d_nodes = nullptr;
    Buf<BvhObj> *d_bobjs = nullptr;
    Buf<int32_t> *d_planes = nullptr;
    ~Probe() {
        delete d_objs;
        delete d_world;
        delete d_nodes;
        delete d_bobjs;
        delete d_planes;
    }
};

__global__ void __launch_bounds__(PT_BLOCK) probe_gl_queries(const ptg::GlObj *objs, int32_t nobj, const DevFrame F, const BvhNode *nodes,
                                                             const BvhObj *bobjs, const int32_t *plane_idx, const double *q, int64_t n,
                                                             int32_t *idx, uint64_t *tbits, uint32_t *wcs) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int64_t i = (int64_t)blockIdx.x * PT_BLOCK + threadIdx.x;
    if (i >= n) return;
    ptg::WalkCount wc = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
    const ptg::TreeWorld world{objs, nobj, F, nodes, bobjs, plane_idx, reinterpret_cast<int *>(smem) + threadIdx.x, PT_BLOCK, wc};
    const double *r = q + 11 * i;
    const double ro[3] = {r[1], r[2], r[3]}, rd[3] = {r[4], r[5], r[6]};
    if (r[0] == 0) {
        double t;
        idx[i] = world.closest(ro, rd, r[7], r[8], (int32_t)r[9], t);
        tbits[i] = __builtin_bit_cast(uint64_t, t);
    } else {
        idx[i] = world.occluded(ro, rd, r[8]) ? 1 : 0;
        tbits[i] = 0;
    }
    uint32_t *w = wcs + 7 * i;
    w[0] = wc.closest_walked; w[1] = wc.closest_plain; w[2] = wc.shadow_walked; w[3] = wc.shadow_plain;
    w[4] = wc.closest_visits; w[5] = wc.shadow_visits; w[6] = wc.deepest;
}

// The shadow turn of fog_walk_body: make_fray (an idle lane: direction (0, 0, 1), tmax 0), wave_walk_coop, wave_any_hit on the
// wave's PT_BVH_STACK words of LDS or wave_any_hit_plain.  blocked [n]; per wave {coop, visits, deepest}.
__global__ void __launch_bounds__(PT_BLOCK) probe_fog_turns(const DevFrame F, const BvhNode *g_nodes, const BvhObj *g_bobjs, const DevObj *g_world,
                                                            const int32_t *g_planes, const double *rays, const uint8_t *active, int64_t nwaves,
                                                            int32_t *blocked_out, uint32_t *wave_out) {
    __shared__ int wstack[PT_BLOCK / PT_WAVE][PT_BVH_STACK];
    typedef const BvhNode __attribute__((address_space(4))) *ConstNodePtr;
    typedef const BvhObj __attribute__((address_space(4))) *ConstBObjPtr;
    typedef const DevObj __attribute__((address_space(4))) *ConstObjPtr;
    typedef const int32_t __attribute__((address_space(4))) *ConstIdxPtr;
    const ConstNodePtr nodes = (ConstNodePtr)g_nodes;
    const ConstBObjPtr bobjs = (ConstBObjPtr)g_bobjs;
    const ConstObjPtr g_obj = (ConstObjPtr)g_world;
    const ConstIdxPtr g_pl = (ConstIdxPtr)g_planes;
    const int64_t i = (int64_t)blockIdx.x * PT_BLOCK + threadIdx.x;
    const int64_t wave = i >> 6;
    if (wave >= nwaves) return;  // (whole waves)
    int *const wst = wstack[threadIdx.x >> 6];
    const double *r = rays + 7 * i;
    const bool casts = active[i] != 0;
    if (__ballot(casts) == 0) {  // no lane holds a shadow ray: the turn is skipped, every lane counts as occluded
        blocked_out[i] = 1;
        return;
    }
    const double mx = r[0], my = r[1], mz = r[2];
    const ptf::FRay fr = ptf::make_fray(mx, my, mz, casts ? r[3] : 0.0, casts ? r[4] : 0.0, casts ? r[5] : 1.0);
    const double stmax = casts ? r[6] : 0.0;
    const ptk::RayD rd{mx, my, mz, fr.d[0], fr.d[1], fr.d[2]};
    const bool coop = ptk::wave_walk_coop(F, casts, rd, fr.a);
    uint32_t c_visits = 0, c_deep = 0;
    bool blocked;
    if (coop) blocked = ptk::wave_any_hit(F, nodes, bobjs, g_obj, g_pl, casts, fr, stmax, wst, c_visits, c_deep);
    else blocked = ptk::wave_any_hit_plain(F, g_obj, casts, fr, stmax);
    blocked_out[i] = blocked ? 1 : 0;
    if ((threadIdx.x & 63u) == 0u) {
        uint32_t *w = wave_out + 3 * wave;
        w[0] = coop ? 1u : 0u; w[1] = c_visits; w[2] = c_deep;
    }
}

}  // namespace

extern "C" {

int64_t wp_guard(void) { return GUARD; }

// The scene's tables, built as gw_open builds them, and their device copies.  Null when an allocation or a copy failed.
void *wp_open(const pt_scene *sc, const pt_gl_material *ex) {
    (void)ex;  // (the walks read no material)
    Probe *K = new Probe;
    const int32_t nmat = sc->num_materials;
    for (int32_t i = 0; i < sc->num_objects; i++) K->objs.push_back(ptg::gl_object(sc->objects[i], nmat));
    scene_to_world(*sc, K->world, K->dmats);
    for (size_t i = 0; i < K->world.size(); i++)
        if ((K->world[i].kind & 0xff) == KIND_PLANE) K->plane_idx.push_back((int32_t)i);
    K->built = ptbvh::build_scene_trees(K->world, false, PT_BVH_STACK, K->T);
    std::memset(&K->F, 0, sizeof K->F);
    ptbvh::frame_bounds(ptbvh::world_bound(K->world), K->F);
    K->F.n_plane = (int32_t)K->plane_idx.size();
    K->F.bvh_root = K->built ? K->T.root : -1;
    K->F.bvh_stack = K->T.stack_need + 1 + 3;
    K->F.bvh_stack = K->F.bvh_stack / 4 * 4 > 4 ? K->F.bvh_stack / 4 * 4 : 4;  // ptcore.hip: max(4, the need + 1 rounded up to 4)
    K->F.nobj = (int32_t)K->world.size();
    K->gl_ok = K->built && ptg::walk_scene_check(sc->objects, sc->num_objects, K->objs.data(), K->T.nodes.data(), K->T.main_nodes, K->T.objs.data(),
                                                 K->T.main_objs, K->plane_idx.data(), (int32_t)K->plane_idx.size(), K->why);
    K->d_objs = new Buf<ptg::GlObj>(K->objs.data(), K->objs.size());
    K->d_world = new Buf<DevObj>(K->world.data(), K->world.size());
    K->d_nodes = new Buf<BvhNode>(K->T.nodes.data(), K->T.nodes.size());
    K->d_bobjs = new Buf<BvhObj>(K->T.objs.data(), K->T.objs.size());
    K->d_planes = new Buf<int32_t>(K->plane_idx.data(), K->plane_idx.size());
    hipError_t st = hipSuccess;
    for (hipError_t e : {K->d_objs->st, K->d_world->st, K->d_nodes->st, K->d_bobjs->st, K->d_planes->st}) PROBE_TRY(e);
    if (st != hipSuccess) {
        delete K;
        return nullptr;
    }
    return K;
}
void wp_close(void *h) { delete static_cast<Probe *>(h); }

// {built, nodes of the main tree, records of the main tree, stack_need, planes, world objects, F.bvh_stack, walk_scene_check, all nodes};
// bounds = {origin_bound, dir_floor, clip_bound, margin}
void wp_info(void *h, int32_t out[9], double bounds[4]) {
    Probe *K = static_cast<Probe *>(h);
    const int32_t v[9] = {K->built ? 1 : 0, K->T.main_nodes, K->T.main_objs, K->T.stack_need, K->F.n_plane, K->F.nobj, K->F.bvh_stack, K->gl_ok ? 1 : 0,
                          (int32_t)K->T.nodes.size()};
    for (int k = 0; k < 9; k++) out[k] = v[k];
    bounds[0] = K->F.origin_bound; bounds[1] = K->F.dir_floor; bounds[2] = K->F.clip_bound; bounds[3] = K->F.margin;
}

// q [n][11]; idx [n + GUARD], tbits [n + GUARD], wc [n + GUARD][7] (the lane's WalkCount).
int wp_gl_queries(void *h, int64_t n, const double *q, int32_t *idx, uint64_t *tbits, uint32_t *wc) {
    Probe *K = static_cast<Probe *>(h);
    const size_t smem = (size_t)K->F.bvh_stack * PT_BLOCK * sizeof(int);
    if (n <= 0 || n > MAX_QUERIES || !K->built || !K->gl_ok || smem > 65536) return -1;
    hipError_t st = hipSuccess;
    Buf<double> d_q(q, 11 * (size_t)n);
    Buf<int32_t> d_idx(nullptr, (size_t)(n + GUARD));
    Buf<uint64_t> d_t(nullptr, (size_t)(n + GUARD));
    Buf<uint32_t> d_wc(nullptr, 7 * (size_t)(n + GUARD));
    for (hipError_t e : {d_q.st, d_idx.st, d_t.st, d_wc.st}) PROBE_TRY(e);
    if (st != hipSuccess) return (int)st;
    hipLaunchKernelGGL(probe_gl_queries, dim3((unsigned)((n + PT_BLOCK - 1) / PT_BLOCK)), dim3(PT_BLOCK), smem, 0, K->d_objs->d, (int32_t)K->objs.size(),
                       K->F, K->d_nodes->d, K->d_bobjs->d, K->d_planes->d, d_q.d, n, d_idx.d, d_t.d, d_wc.d);
    st = (hipError_t)finish(st);
    PROBE_TRY(d_idx.download(idx));
    PROBE_TRY(d_t.download(tbits));
    PROBE_TRY(d_wc.download(wc));
    return (int)st;
}

// rays [64 nwaves][7], active [64 nwaves]; blocked [64 nwaves + GUARD], waves [nwaves + GUARD][3] = coop, visits, deepest.
int wp_fog_turns(void *h, int64_t nwaves, const double *rays, const uint8_t *active, int32_t *blocked, uint32_t *waves) {
    Probe *K = static_cast<Probe *>(h);
    const int64_t n = 64 * nwaves;
    if (nwaves <= 0 || n > MAX_QUERIES || !K->built) return -1;
    hipError_t st = hipSuccess;
    Buf<double> d_r(rays, 7 * (size_t)n);
    Buf<uint8_t> d_a(active, (size_t)n);
    Buf<int32_t> d_b(nullptr, (size_t)(n + GUARD));
    Buf<uint32_t> d_w(nullptr, 3 * (size_t)(nwaves + GUARD));
    for (hipError_t e : {d_r.st, d_a.st, d_b.st, d_w.st}) PROBE_TRY(e);
    if (st != hipSuccess) return (int)st;
    hipLaunchKernelGGL(probe_fog_turns, dim3((unsigned)((n + PT_BLOCK - 1) / PT_BLOCK)), dim3(PT_BLOCK), 0, 0, K->F, K->d_nodes->d, K->d_bobjs->d,
                       K->d_world->d, K->d_planes->d, d_r.d, d_a.d, nwaves, d_b.d, d_w.d);
    st = (hipError_t)finish(st);
    PROBE_TRY(d_b.download(blocked));
    PROBE_TRY(d_w.download(waves));
    return (int)st;
}

}  // extern "C"
