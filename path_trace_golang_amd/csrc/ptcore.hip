// ptcore.hip -- libptcore.so: C ABI (include/ptcore.h) over the gfx950 kernels.
//
// Host responsibilities, all restating the set-up half of the reference CPU engine:
//   * convertMaterial      internal/engine/materials.go:28-55
//   * sceneToWorld         internal/engine/objects.go:225-269
//   * newCamera            internal/engine/camera.go:19-58
//   * sky closure select   internal/engine/renderer.go:56-92
//   * frame constants      internal/engine/renderer.go:95-98
//   * 32x32 tile grid      internal/engine/renderer.go:132-157 (here: the multi-GPU shard unit)
// then per chunk of samples: reset queue -> trace_kernel -> resolve_kernel.
// There is no CPU rendering path in this library: without a HIP device every entry
// point fails with PT_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h>  // types and prototypes only: librccl.so is loaded on request (PTCORE_GATHER=rccl), never linked

#include <algorithm>
#include <chrono>
#include <cmath>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/ptcore.h"
#include "pt_bvh.h"
#include "pt_convert.h"
#include "pt_device.h"
#include "pt_kernels.h"
#include "pt_filter_launch.h"
#include "pt_wavefront.h"
#include "pt_walk32.h"
#include "pt_primary.h"
#include "pt_feature_walk.h"
#include "pt_fog_walk.h"
#include "pt_math.h"

using namespace ptd;

namespace {

thread_local std::string g_last_error;
unsigned long long g_profile_scratch[3 * ptk::SEC_COUNT] = {};
unsigned long long g_mismatches = 0;
unsigned long long g_mismatch_sample[10] = {};  // SCAN_VERIFY disagreements of the last collected frame

int32_t fail(int32_t code, const std::string &msg) {
    g_last_error = msg;
    return code;
}

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return fail(PT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));                 \
    } while (0)

// Set by pt_destroy while it lets go of memory and events whose device could not be made current: they are left alone then, as they
// always were, not freed under another device.
thread_local bool g_leave_device_memory = false;

// (untyped, for DevBuf and for the rows of pass_plan)
void dev_release(void **p, size_t *cap) {
    if (*p && !g_leave_device_memory) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
}
hipError_t dev_reserve(void **p, size_t *cap, size_t n, size_t size) {
    if (n <= *cap) return hipSuccess;
    dev_release(p, cap);
    hipError_t e = hipMalloc(p, n * size);
    if (e == hipSuccess) *cap = n;
    return e;
}

// Device memory that grows on request and frees itself: move-only, and a move-assignment hands the old memory to the source, which
// frees it when it dies.  Its device must be current then (pt_destroy sees to that).
template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;  // elements
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept { swap(o); }
    DevBuf &operator=(DevBuf &&o) noexcept { swap(o); return *this; }
    ~DevBuf() { release(); }
    void swap(DevBuf &o) { std::swap(p, o.p); std::swap(cap, o.cap); }
    hipError_t reserve(size_t n) { return dev_reserve(reinterpret_cast<void **>(&p), &cap, n, sizeof(T)); }
    void release() { dev_release(reinterpret_cast<void **>(&p), &cap); }
};

// The per-pass buffers of a device, the one list of them (pass_plan): what need_bytes() prices, what dev_begin reserves (and releases
// when the device is short of memory) and what dev_held_bytes() adds up all follow from it.  A row is one buffer and does not depend on
// the frame: what its length goes by, its elements of `size` bytes per job or per queue entry (`elems_stats` more with pixel stats),
// and the forms of the loop that use it.  (wf_bins, of fixed size, is not here.)
enum PassPer {
    PER_JOB,    // the jobs of a pass: pixel slots x samples
    PER_ENTRY,  // the entries of a path-state queue: one per job + queue_slack()
    PER_EXTRA   // the same, for what rides along with the queues (dev_begin's first guess at a pass that fits leaves these out)
};
enum PassWhen : unsigned { WHEN_Q_GLASS = 1, WHEN_Q_CONT = 2, WHEN_Q_PATH_B = 4, WHEN_WF_SORT = 8, WHEN_WALK32 = 16 };  // 0: every frame
struct PassBuf {
    void **p;     // the DevBuf's pointer and capacity
    size_t *cap;
    size_t size;
    PassPer per;
    size_t elems, elems_stats;
    unsigned when;
    template <typename T>
    PassBuf(DevBuf<T> &b, PassPer per_, size_t elems_, size_t elems_stats_, unsigned when_)
        : p(reinterpret_cast<void **>(&b.p)), cap(&b.cap), size(sizeof(T)), per(per_), elems(elems_), elems_stats(elems_stats_), when(when_) {}
    // elements per job / entry in a frame of the forms `have` (frame_forms): 0 = the frame does not use the buffer
    size_t used(unsigned have, bool stats) const { return (when & ~have) ? 0 : elems + (stats ? elems_stats : 0); }
};

struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
};

// The event pairs of one kind of timed launch (timed, sum_ms): made when first needed, used again by every frame; the first n are
// those of the running frame.  Owns its events the way DevBuf owns its memory.
struct EventList {
    std::vector<EventPair> v;
    size_t n = 0;
    EventList() = default;
    EventList(EventList &&o) noexcept { swap(o); }
    EventList &operator=(EventList &&o) noexcept { swap(o); return *this; }
    ~EventList() {
        if (g_leave_device_memory) return;
        for (EventPair &e : v) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    }
    void swap(EventList &o) { v.swap(o.v); std::swap(n, o.n); }
};
enum EventKind { EV_TRACE, EV_RESOLVE, EV_RAYGEN, EV_GLASS, EV_FOG, EV_MOMENTS, EV_CHECK, EV_FEATURE, EV_HALVES, EV_BLOCKS, EV_REFIT, EV_KINDS };

// Storage of one path-state queue (PathQueue, pt_device.h): per entry 10 doubles, the stream state and 4 words -- job, depth, hit
// object, answer -- or 6 with pixel stats (+ the job's two counters); every plane of `u` is as long as the queue.
struct QueueBuf {
    DevBuf<double> d;
    DevBuf<unsigned long long> rs;
    DevBuf<uint32_t> u;
    // its rows of pass_plan: 80 + 8 + 4 x 4 = 104 B per entry, 112 B with pixel stats
    void plan(std::vector<PassBuf> &rows, unsigned when) {
        rows.insert(rows.end(), {{d, PER_ENTRY, 10, 0, when}, {rs, PER_ENTRY, 1, 0, when}, {u, PER_ENTRY, 4, 2, when}});
    }
    // the queue as the kernels take it: `cap` entries (what the buffers were reserved for), appended at *count
    PathQueue bind(size_t cap, bool stats, unsigned int *count) const {
        PathQueue q{};
        q.d = d.p;
        q.rs = rs.p;
        q.job = u.p;
        q.depth = reinterpret_cast<int32_t *>(u.p + cap);
        q.best = reinterpret_cast<int32_t *>(u.p + 2 * cap);
        q.hit = reinterpret_cast<int32_t *>(u.p + 3 * cap);
        q.jseg = stats ? u.p + 4 * cap : nullptr;
        q.jdraw = stats ? u.p + 5 * cap : nullptr;
        q.count = count;
        q.cap = (uint32_t)cap;
        return q;
    }
};

// One device's share of a frame.
struct Device {
    int ordinal = 0;
    int num_cu = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;  // own_stream or the caller's
    DevBuf<DevObj> objs;
    DevBuf<DevMat> mats;
    DevBuf<DevRoulette> roulette;     // the roulette table of mats (pt_convert.h: roulette_table), uploaded with them
    DevBuf<BroadSphere> bsph;
    DevBuf<BroadBox> bbox;
    DevBuf<int32_t> plane_idx;
    size_t bytes_cap = 0;             // bytes of per-pass buffers (jobs + path-state queues) that fitted after an allocation failed (0: never failed)
    DevBuf<BvhNode> bvh_nodes;
    DevBuf<BvhObj> bvh_objs;
    DevBuf<BvhNode> bvh_cores;
    DevBuf<double> L;
    DevBuf<double> ray;
    DevBuf<unsigned long long> ray_rng;
    DevBuf<uint16_t> ray_ndraw;
    DevBuf<double> inject;            // pt_debug_set_primary_rays: the table's device copy
    uint64_t inject_gen = 0;          // generation of the table it holds (0 = none)
    DevBuf<uint32_t> job_seg, job_draw;
    DevBuf<double> acc;
    DevBuf<uint32_t> acc_seg, acc_draw;
    DevBuf<double> m2;                // pt_set_moments: [3][nslots] running sums of squares (allocated only then)
    DevBuf<double> tiles_m2;          // ... and their tile-major copy for the gather
    DevBuf<ptk::NoisePartial> noise_part;  // pt_noise_estimate: one partial per block of noise_kernel
    DevBuf<double> feat;              // pt_set_features: [9][nslots] running first-hit feature sums (allocated only then)
    DevBuf<double> tiles_feat;        // ... and the tile-major copy of one plane of them for the gather
    DevBuf<int32_t> obj_ids;          // pt_set_object_ids: [nslots] sample 0's first hit as an index into the device world (allocated only then)
    DevBuf<int32_t> obj_map;          // ... and [nobj] the world's indices into pt_scene.objects (the world skips unknown types)
    DevBuf<double> hv;                // pt_set_halves: [12][nslots] running half-buffer sums SA, QA, SB, QB (allocated only then)
    DevBuf<double> tiles_hv;          // ... and the tile-major copy of one plane of them for the gather
    // pt_set_adaptive (allocated only then): the active list (two buffers, the check compacts from one into the other), the
    // samples per block, the check's per-block decision and noise, and the word the host reads back after every check
    DevBuf<uint32_t> act[2], blk_spp, blk_keep;
    DevBuf<double> blk_noise;
    DevBuf<ptk::AdaptResult> ad_res;
    int act_cur = 0;                  // which of act[] holds the current list
    DevBuf<double> map_pooled;        // pt_set_adaptive_filtered: this device's copy of the check's map, P_B and the stop flag per frame block
    DevBuf<uint8_t> map_stop;
    uint32_t nact = 0;                // its length
    DevBuf<uint8_t> tiles_rgba;
    DevBuf<double> tiles_accum;
    DevBuf<uint32_t> tiles_seg, tiles_draw;
    DevBuf<unsigned int> queue;       // [0] item cursor of the running trace pass, [1] glass count, [2],[3] continuation counts (ping-pong), [4] always 0
    DevBuf<BroadSphere> bsph_diel;    // broad-phase records of the dielectric objects only
    DevBuf<BroadBox> bbox_diel;
    // path-state queues (one entry per job of a chunk at most, + queue_slack): the split form's glass queue = the wavefront form's
    // exit queue; the continuation queue = the wavefront form's path queue A; its path queue B
    QueueBuf q_glass, q_cont, q_path_b;
    int blocks_per_cu_wf = 0;
    int blocks_per_cu_walk = 0;        // wf_walk32_kernel (PTCORE_PIPELINE=walk32)
    DevBuf<uint32_t> cand_ids, cand_n, slow_list;  // walk32: candidate lists of the running level, entries left to the FP64 traversal
    DevBuf<uint32_t> wf_perm, wf_key, wf_bins;  // ray sorting of the wavefront form
    size_t q_cap = 0;
    DevBuf<unsigned long long> counters;
    DevBuf<unsigned long long> prof;
    EventList ev[EV_KINDS];
    DevBuf<ptf::FogLight> fog_lights;        // the frame's light list (fog on)
    DevBuf<unsigned long long> fog_counters; // [3] shadow rays, draws, march steps of the frame
    DevBuf<unsigned long long> fog_walk_counters; // [6] pt_set_fog_walk: primary pairs walked / scanned plainly, shadow turns walked / looped plainly, node visits, deepest stack
    DevBuf<unsigned long long> walk_counters; // [4] pt_set_feature_walk: (wave, sample) pairs walked, ... scanned plainly, node visits, deepest stack
    DevBuf<ptg::GlObj> gl_objs;              // GL shading: the frame's objects, materials and light list
    DevBuf<ptg::GlMat> gl_mats;
    DevBuf<int32_t> gl_lights;
    DevBuf<unsigned long long> gl_counters;  // [5] paths, segments, shadow rays, probe rays, draws of the frame
    DevBuf<unsigned long long> gl_walk_counters;  // [7] pt_set_shading_walk: closest queries walked / looped plainly, shadow queries walked / looped plainly, node visits of either, deepest stack
    std::vector<char> trace_is_split;  // per trace launch of the frame: the split form?
    hipEvent_t ev_first = nullptr, ev_last = nullptr;
    bool first_recorded = false;
    unsigned long long pass_log_prev[24] = {};  // PTCORE_DEBUG_PASS_LOG: the counters after the previous pass of this frame
    // frame state
    pt_shard shard{0, 1};
    int32_t nlocal = 0;
    uint32_t nslots = 0;
    bool acc_started = false;
    int blocks_per_cu = 0, blocks_per_cu_split = 0, blocks_per_cu_glass = 0, blocks_per_cu_primary = 0;
    uint64_t scene_gen = 0;  // SceneData generation resident on this device (0 = none)
    uint64_t topo_gen = 0;   // ... and the generation of the hierarchy's topology (pt_set_bvh_refit: a moved world keeps it)
    DevBuf<double> rf_box, rf_area, rf_part;  // the refit's scratch: exact box and a[q] per node, the figure's block sums
};

struct Frame {
    bool open = false;
    pt_config cfg{};
    DevFrame F{};
    DevCamera cam{};
    DevSky sky{};
    int32_t nobj = 0, nmat = 0;
    int32_t ntx = 0, nty = 0;
    int32_t done_spp = 0;
    uint32_t chunk = 0;
    bool stats_on = false;
    size_t lds_bytes = 0;
    size_t glass_lds_bytes = 0;
    bool wavefront = false;  // the wavefront form (pt_wavefront.h) instead of the all-in-one loop
    bool walk32 = false;     // ... with its traversal pass split into the FP32 walk and the exact pass of pt_walk32.h
    size_t shade_lds_bytes = 0;
    int split_rounds = 0;  // trace + glass pass pairs before the all-in-one pass (0: all-in-one only)
    size_t budget_bytes = 0;  // job-buffer budget of this frame (pt_ctx::l_budget_bytes, or the grown one)
    int tail_form = 0;     // ptk::FORM_* of the pass behind the split rounds (FORM_NESTED for the bitmask scans, see pt_kernels.h)
    bool has_glass = false;  // some object is dielectric
    bool primary_pass = false;  // BVH scans: the first segment of every path by primary_bvh_kernel (pt_primary.h), the rest through the continuation queue
    int scan = 0;  // ptk::SCAN_* used for this frame
    bool fog_vol = false;  // fog_kernel runs after every chunk (pt_set_fog with gpu_volumetric, max_depth > 0)
    ptf::FogParams fog{};
    std::vector<ptf::FogLight> fog_lights;
    bool gl = false;  // GL shading (pt_set_shading): gl_trace_kernel replaces ray generation and the trace kernels
    bool gl_walk = false;  // pt_set_shading_walk on a BVH scan with GL shading: gl_bvh_kernel (pt_gl_walk.h) in gl_trace_kernel's place
    bool gl_filter = false;  // pt_set_shading_features on a GL frame: features by gl_feature_kernel (pt_gl_features.h), pt_atrous / pt_atrous_halves accept it
    bool moments = false;  // pt_set_moments: moments_kernel runs after every chunk's resolve add (pt_begin / pt_render frames only)
    bool adaptive = false; // pt_set_adaptive: the frame's jobs are those of the active blocks, a check ends every pt_step (implies moments)
    pt_adaptive ad{};
    bool halves = false;   // pt_set_halves: halves_kernel runs after every chunk's moments_kernel (pt_begin / pt_render frames only; implies moments)
    uint64_t serial = 0;   // pt_ctx::frames_opened when the frame opened: tells two frames of a context apart
    int32_t features = 0;  // pt_set_features: feature_kernel runs after the chunks that hold samples below this index (pt_begin / pt_render frames only)
    bool fog_walk = false;      // pt_set_fog_walk on a BVH scan with fog_vol: fog_bvh_kernel (pt_fog_walk.h) in fog_kernel's place
    bool feature_walk = false;  // pt_set_feature_walk on a BVH scan: feature_bvh_kernel (pt_feature_walk.h) in feature_kernel's place
    bool object_ids = false;  // pt_set_object_ids: feature_kernel also records the object of sample 0's first hit
    int32_t scene_objects = 0;  // ... pt_scene.num_objects of the frame, the length a motion table must have
    std::vector<int32_t> world_scene;  // ... per object of the device world its index into pt_scene.objects
    double worst_active = 0.0;  // largest block noise among the blocks the last check kept
    bool filtered = false;      // pt_set_adaptive_filtered: the adaptive check decides by the pooled noise of the filtered frame (implies halves)
    pt_adaptive_filtered fa{};
    int32_t fa_checks = 0;      // ... the checks that have decided so far
    std::vector<ptg::GlObj> gl_objs;
    std::vector<ptg::GlMat> gl_mats;
    std::vector<int32_t> gl_lights;
    ptg::GlCam gl_cam{};
    ptg::GlSky gl_sky{};
    std::chrono::steady_clock::time_point t0;
};

// Everything derived from the scene alone (world, broad-phase records, hierarchies).  Kept across
// frames: an unchanged scene (progressive previews, benchmark loops, camera-only edits do not count:
// the camera is not part of it) is neither rebuilt nor uploaded again.
struct SceneData {
    bool valid = false;
    int scan_req = -2;
    uint64_t gen = 0;
    std::vector<DevObj> world;
    std::vector<DevMat> mats;
    std::vector<DevRoulette> roulette;  // the roulette table of mats: rebuilt wherever mats is replaced
    std::vector<BroadSphere> bsph;
    std::vector<BroadBox> bbox;
    std::vector<BroadSphere> bsph_diel;
    std::vector<BroadBox> bbox_diel;
    std::vector<pt_material> raw_mats;  // the caller's arrays as last seen (change detection without converting)
    std::vector<pt_object> raw_objs;
    std::vector<int32_t> plane_idx;
    std::vector<BvhNode> bvh_nodes;
    std::vector<BvhObj> bvh_objs;
    std::vector<BvhNode> bvh_cores;   // core twins of bvh_nodes (the FP32 walk's certain bounds)
    std::vector<int32_t> bvh_levels;  // first node of every level of both trees, then the node count (the refit's launch table)
    uint64_t topo_gen = 0;            // advances with every full build; a refit (pt_set_bvh_refit) advances gen only
    bool tree_moved = false;          // the world is not the one bvh_nodes / bvh_objs were built from: the devices refit their copies
    double bvh_margin = 0.0;          // the inflation of the hierarchy's boxes for the current world
    int bvh_depth = 0;
    int bvh_stack_need = 0;
    bool has_glass = false;           // some object is dielectric
    uint64_t gl_walk_gen = 0;         // pt_set_shading_walk: the generation ptg::walk_scene_check last looked at (0 = none), its answer
    bool gl_walk_ok = false;          // ... and what it objected to
    std::string gl_walk_why;
    size_t lds_bytes = 0;
    size_t glass_lds_bytes = 0;
    int scan = 0;
    DevFrame Fs{};  // the scene-dependent fields of DevFrame
};

}  // namespace

struct pt_ctx {
    std::vector<Device> devs;
    Frame frame;
    SceneData sd;
    // device-0 gather / frame buffers for the host-memory entry points
    DevBuf<uint8_t> g_tiles_rgba;
    DevBuf<double> g_tiles_accum;
    DevBuf<uint32_t> g_tiles_seg, g_tiles_draw;
    DevBuf<uint8_t> f_rgba;
    DevBuf<double> f_accum;
    DevBuf<double> g_tiles_m2, f_m2;  // pt_read_moments: the gathered tiles and the row-major frame of the second moments
    bool moments_on = false;          // pt_set_moments
    bool adaptive_on = false;         // pt_set_adaptive
    int32_t features_k = 0;           // pt_set_features: feature samples per pixel (0 = off)
    DevBuf<double> g_tiles_feat, f_feat_n, f_feat_a, f_feat_d;  // pt_read_features / pt_atrous: one gathered plane, the three row-major frames
    bool fog_walk_on = false;         // pt_set_fog_walk: the volumetric fog term on the BVH path, by the wave-shared walks
    bool shading_walk_on = false;     // pt_set_shading_walk: GL shading on the BVH path, its ray queries by the lane's walk
    bool shading_features_on = false; // pt_set_shading_features: a GL frame takes features, object ids and the a-trous filter
    bool feature_walk_on = false;     // pt_set_feature_walk: features on the BVH path, by the wave-shared walk
    struct Refit {  // pt_set_bvh_refit
        double max_growth = 0.0;      // 0 = off
        struct pt_bvh_refit_stats st{};
        bool figure_pending = false;  // a refit was prepared and no device has run it yet: cost_now is not known
    } rf;
    struct Build {  // pt_set_bvh_build
        int32_t mode = 0;             // 0 = the host builder, 1 = the device build
        struct pt_bvh_build_stats st{};
    } bb;
    bool object_ids_on = false;      // pt_set_object_ids
    DevBuf<uint32_t> f_ids;           // pt_read_object_ids / pt_temporal with a motion table: the row-major plane (the bits of int32, scene indices)
    // The buffers of the post-frame filters, on devices[0]: allocated on the first call, never shrunk.
    struct Atrous {  // pt_atrous, pt_temporal: colour and variance ping-pong, the guide records, the noise partials
        DevBuf<double> col[2], var[2];
        DevBuf<pta::Guide> guide;
        DevBuf<ptk::NoisePartial> part;
    } at;
    bool halves_on = false;           // pt_set_halves
    DevBuf<double> g_tiles_hv, f_hv_sa, f_hv_qa, f_hv_sb, f_hv_qb;  // pt_read_halves / pt_atrous_halves: one gathered plane, the four row-major frames
    struct Halves {  // pt_atrous_halves: guide, colour and variance planes of both halves (ping-pong), the combined mean, err and the two
        DevBuf<double> guide, col[2], var[2], mean, err, half;  // filtered halves row-major, the partials of the two figures
        DevBuf<ptk::HalvesPartial> part;
    } ah;
    struct Temporal {  // pt_temporal: two sets of history planes, hist[cur] the stored one, and the block partials
        DevBuf<double> hist[2];
        DevBuf<ptk::TemporalPartial> part;
        int cur = 0;
        bool valid = false;           // the history is not empty
        int32_t w = 0, h = 0;         // its size and camera
        DevCamera cam{};
        uint64_t serial = 0;          // the frame and the samples done of the last call that succeeded ("already accumulated")
        int32_t spp = 0;
        double clip = 0.0;            // pt_temporal_set_clip: gamma of step 7a for later calls (0 = off)
        struct pt_temporal_clip_stats clip_stats{};  // of the last pt_temporal that succeeded
        // pt_temporal_set_motion: the pending table [motion_n][3] (step 4a), consumed by the next pt_temporal that succeeds
        std::vector<double> motion;
        int32_t motion_n = 0;         // 0 = no table pending
        DevBuf<double> delta;         // its copy on devices[0] for the call that consumes it
        struct pt_temporal_motion_stats motion_stats{};  // of the last pt_temporal that succeeded
    } tp;
    uint64_t frames_opened = 0;      // pt_begin / pt_render frames of this context so far
    pt_adaptive adaptive{};
    bool filtered_on = false;         // pt_set_adaptive_filtered
    pt_adaptive_filtered filtered{};
    struct Blocks {  // ... the check's per-block sums and map on devices[0], and the host copy that travels to the devices and to pt_read_block_figures.
                     // The host copies outlive the frame: they are that frame's only while frame.fa_checks > 0 (frame_open resets the Frame).
        DevBuf<double> s, pooled, own;
        DevBuf<uint32_t> k;
        DevBuf<uint8_t> stop;
        std::vector<double> h_pooled, h_own;
        std::vector<uint8_t> h_stop;
    } bf;
    DevBuf<uint32_t> f_seg, f_draw;
    size_t l_budget_bytes = (size_t)48 << 30;  // per-chunk job buffers (radiance, primary rays, path-state queues): a sixth of the 288 GB
    // A context that renders frame after frame of one shape (a UI, an animation: gpu.go:2534-2546 is called once per frame) grows its
    // job buffers by itself from the second such frame on, to the size bench.py asks for explicitly (4 instead of 13 passes per
    // 1080p x 1024-spp frame: -4.5 % time per frame), provided the device has that much free: a one-shot render keeps the small set-up.
    // Off when PTCORE_L_BUDGET_MB names a size, or with PTCORE_AUTO_GROW=0.
    size_t grown_budget_bytes = (size_t)160 << 30;
    bool auto_grow = true;
    int32_t last_w = 0, last_h = 0, last_spp = 0;  // the shape of the previous frame of this context
    bool grown = false;
    int pipeline = -1;     // PTCORE_PIPELINE=mega|wavefront|walk32 (default: by scene, see frame_open)
    int wf_min_lanes = 40; // PTCORE_WF_MIN_LANES: the walk loop of a traversal pass is left for a refill below this many walking lanes
    int wf_sort = 0;       // PTCORE_WF_SORT=1: reorder the paths of a level by direction octant and origin cell
    int split_rounds = 2;  // PTCORE_SPLIT_ROUNDS: trace + glass pass pairs per chunk before the all-in-one pass (bitmask scan only)
    bool primary_coop = true;  // PTCORE_PRIMARY=lane: BVH scenes without the wave-cooperative primary pass (the round-3 loop)
    bool tail_nested = true;  // PTCORE_TAIL=trip: the pass behind the split rounds in the round-1 form (exit search = the lane's next trip) instead of FORM_NESTED
    // PTCORE_GATHER=rccl: the tiles of a frame reach devices[0] through RCCL (grouped ncclSend / ncclRecv over one communicator per
    // device, ncclCommInitAll) instead of hipMemcpyPeerAsync.  librccl.so is dlopen'ed then and only then.
    struct Rccl {
        void *lib = nullptr;
        std::vector<ncclComm_t> comms;
        decltype(&ncclCommInitAll) CommInitAll = nullptr;
        decltype(&ncclCommDestroy) CommDestroy = nullptr;
        decltype(&ncclGroupStart) GroupStart = nullptr;
        decltype(&ncclGroupEnd) GroupEnd = nullptr;
        decltype(&ncclSend) Send = nullptr;
        decltype(&ncclRecv) Recv = nullptr;
        decltype(&ncclGetErrorString) GetErrorString = nullptr;
        uint64_t gathers = 0;  // frames gathered through it
    } rccl;
    uint32_t claim = 0;   // jobs per queue claim; 0 = by pass shape (dev_step), PTCORE_CLAIM forces one
    int max_blocks_per_cu = 8;
    int scan_mode = -1;  // -1 = choose by scene size; PTCORE_SCAN=uniform|broad|verify|bvh|verify_bvh forces one
    unsigned long long last_mismatches = 0;
    bool profile_sections = false;  // PTCORE_PROFILE=1: diagnostic kernel build with per-section counters
    unsigned long long last_profile[3 * ptk::SEC_COUNT] = {};
    // fog (pt_set_fog): off by default; the raw block as given
    bool fog_on = false;
    pt_fog fog_raw{};
    pt_fog_stats fog_last{};
    int fog_pending = 0;  // the last frame's fog counters are still on the device: 1 = every device, 2 = devs[0] only
    // shading model (pt_set_shading): the CPU engine by default; GL with one pt_gl_material per scene material
    int32_t shading_model = PT_SHADING_CPU;
    std::vector<pt_gl_material> gl_extras;
    pt_shading_stats shading_last{};
    int shading_pending = 0;  // as fog_pending, for the GL counters
    // pt_debug_set_primary_rays: [n][6] rays that replace ray generation's (empty = none, the default)
    std::vector<double> inject_rays;
    uint64_t inject_gen = 0;  // bumped by every call that sets a table
};

namespace {

// ---------------------------------------------------------------- scene conversion

// (scene_to_world, objects.go:225-269: pt_convert.h)

struct H3 {
    double x, y, z;
};
H3 h3(const double *p) { return H3{p[0], p[1], p[2]}; }
H3 sub(H3 a, H3 b) { return H3{a.x - b.x, a.y - b.y, a.z - b.z}; }
H3 mul(H3 a, double t) { return H3{a.x * t, a.y * t, a.z * t}; }
H3 divs(H3 a, double t) { double inv = 1.0 / t; return H3{a.x * inv, a.y * inv, a.z * inv}; }
double dot(H3 a, H3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
H3 cross(H3 a, H3 b) { return H3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
double length(H3 a) { return ptm::f_sqrt(dot(a, a)); }
H3 unit(H3 a) {
    double l = length(a);
    if (l == 0) return a;
    return divs(a, l);
}
void put(double *d, H3 v) { d[0] = v.x; d[1] = v.y; d[2] = v.z; }

DevCamera new_camera(const pt_camera &c, int width, int height) {  // camera.go:19-58
    DevCamera cam;
    double aspect = (double)width / (double)height;
    if (c.aspect_ratio != 0) aspect = c.aspect_ratio;
    const double theta = c.fov * 3.141592653589793 / 180;
    const double h = ptm::go_tan(theta / 2);
    const double viewportHeight = 2.0 * h;
    const double viewportWidth = aspect * viewportHeight;
    const H3 origin = h3(c.position), target = h3(c.target), up = h3(c.up);
    const H3 w = unit(sub(origin, target));
    const H3 u = unit(cross(up, w));
    const H3 v = cross(w, u);
    double focusDist = c.focus_dist;
    if (focusDist == 0) focusDist = length(sub(origin, target));
    const H3 horizontal = mul(u, viewportWidth * focusDist);
    const H3 vertical = mul(v, viewportHeight * focusDist);
    const H3 llc = sub(sub(sub(origin, divs(horizontal, 2)), divs(vertical, 2)), mul(w, focusDist));
    put(cam.origin, origin);
    put(cam.lower_left, llc);
    put(cam.horizontal, horizontal);
    put(cam.vertical, vertical);
    put(cam.u, u);
    put(cam.v, v);
    cam.lens_radius = c.aperture / 2;
    return cam;
}

DevSky make_sky(const pt_sky &s) {  // renderer.go:56-92
    DevSky d;
    std::memset(&d, 0, sizeof d);
    d.kind = s.kind == PT_SKY_GRADIENT ? 1 : (s.kind == PT_SKY_SOLID ? 2 : 0);
    const double *c0 = d.kind == 1 ? s.horizon : (d.kind == 2 ? s.color : s.background);
    for (int i = 0; i < 3; i++) { d.c0[i] = c0[i]; d.c1[i] = s.zenith[i]; }
    return d;
}

float round_up_f(double v) {
    float f = (float)v;
    if ((double)f < v) f = std::nextafterf(f, INFINITY);
    return f;
}
float round_down_f(double v) {
    float f = (float)v;
    if ((double)f > v) f = std::nextafterf(f, -INFINITY);
    return f;
}

// Conservative FP32 bounds for the broad phase.  B bounds every finite object's coordinates;
// everything is inflated by m = B * 2^-12 (two orders of magnitude above the worst FP32 rounding of
// the broad-phase arithmetic for ray origins inside [-4B, 4B]^3), and rounded outward.
void build_broad(const std::vector<DevObj> &world, SceneData &fr) {
    DevFrame &F = fr.Fs;
    fr.bsph.clear();
    fr.bbox.clear();
    fr.bsph_diel.clear();
    fr.bbox_diel.clear();
    fr.plane_idx.clear();
    F.sph_all = F.box_all = F.sph_diel = F.box_diel = 0;
    const double B = ptbvh::world_bound(world);
    const double m = B * (1.0 / 4096.0);
    for (size_t i = 0; i < world.size(); i++) {
        const DevObj &o = world[i];
        const int kind = o.kind & 0xff;
        if (kind == KIND_SPHERE) {
            BroadSphere s;
            std::memset(&s, 0, sizeof s);
            s.cx = (float)o.a[0]; s.cy = (float)o.a[1]; s.cz = (float)o.a[2];
            const double rm = std::fabs(o.radius) + m;
            s.rm2 = round_up_f(rm * rm);
            if (!(s.rm2 == s.rm2)) s.rm2 = INFINITY;
            s.index = (int32_t)i;
            s.diel = (o.kind & 0x100) ? 1 : 0;
            fr.bsph.push_back(s);
            if (o.kind & 0x100) fr.bsph_diel.push_back(s);
        } else if (kind == KIND_BOX) {
            BroadBox b;
            std::memset(&b, 0, sizeof b);
            for (int k = 0; k < 3; k++) {
                const double lo = std::min(o.a[k], o.b[k]) - m, hi = std::max(o.a[k], o.b[k]) + m;
                const float c = (float)(0.5 * lo + 0.5 * hi);
                if (lo == lo && hi == hi && std::isfinite(c)) {
                    b.c[k] = c;
                    b.h[k] = round_up_f(std::max((double)c - lo, hi - (double)c));  // [c - h, c + h] holds [lo, hi]
                    if (!(b.h[k] == b.h[k])) b.h[k] = INFINITY;
                } else {  // absurd or non-finite bounds: this slab constrains nothing
                    b.c[k] = 0.0f;
                    b.h[k] = INFINITY;
                }
            }
            b.index = (int32_t)i;
            b.diel = (o.kind & 0x100) ? 1 : 0;
            fr.bbox.push_back(b);
            if (o.kind & 0x100) fr.bbox_diel.push_back(b);
        } else {
            fr.plane_idx.push_back((int32_t)i);
        }
    }
    F.n_bsph = (int32_t)fr.bsph.size();
    F.n_bbox = (int32_t)fr.bbox.size();
    // the dielectric records among the first 32 of each kind, in the bit order of the kernels' candidate masks (push_keep_bit)
    for (int i = 0; i < F.n_bsph && i < 32 && F.n_bsph <= 32; i++)
        if (fr.bsph[(size_t)i].diel) F.sph_diel |= 1u << ptk::pt_record_slot(i, F.n_bsph);
    for (int i = 0; i < F.n_bbox && i < 32 && F.n_bbox <= 32; i++)
        if (fr.bbox[(size_t)i].diel) F.box_diel |= 1u << ptk::pt_record_slot(i, F.n_bbox);
    F.n_plane = (int32_t)fr.plane_idx.size();
    F.planes_y = 1;
    for (int32_t i : fr.plane_idx) {
        const DevObj &o = world[(size_t)i];
        if (!(o.b[0] == 0.0 && o.b[1] == 1.0 && o.b[2] == 0.0) || std::signbit(o.b[0]) || std::signbit(o.b[2])) F.planes_y = 0;
        // plane_exact_y drops the terms (px - ox) * 0 and (pz - oz) * 0 of objects.go:107: they are zeros only for a finite point
        // (inf * 0 = NaN makes the reference's t a NaN, which its range test accepts)
        if (!(std::isfinite(o.a[0]) && std::isfinite(o.a[1]) && std::isfinite(o.a[2]))) F.planes_y = 0;
    }
    F.plane0_index = -1;
    F.plane0_y = 0.0;
    F.plane0_kind = 0;
    if (F.planes_y && fr.plane_idx.size() == 1) {
        const DevObj &o = world[(size_t)fr.plane_idx[0]];
        F.plane0_index = fr.plane_idx[0];
        F.plane0_y = o.a[1];
        F.plane0_kind = o.kind;
    }
    F.n_dsph = (int32_t)fr.bsph_diel.size();
    F.n_dbox = (int32_t)fr.bbox_diel.size();
    F.broad_ok = (fr.bsph.size() <= 32 && fr.bbox.size() <= 32) ? 1 : (fr.bsph.size() <= 128 && fr.bbox.size() <= 128) ? 2 : 0;
    F.sph_all = fr.bsph.size() >= 32 ? 0xffffffffu : ((1u << fr.bsph.size()) - 1u);
    F.box_all = fr.bbox.size() >= 32 ? 0xffffffffu : ((1u << fr.bbox.size()) - 1u);
    ptbvh::frame_bounds(B, F);  // origin_bound, dir_floor, scene_bound, clip_bound, margin
}

int32_t tiles_of_shard(int32_t ntiles, const pt_shard &sh) {
    if (sh.index >= ntiles) return 0;
    return (ntiles - sh.index + sh.count - 1) / sh.count;
}

int32_t validate(const pt_scene *scene, const pt_config *cfg) {
    if (!scene || !cfg) return fail(PT_ERR_INVALID, "null scene or config");
    if (cfg->width <= 0 || cfg->height <= 0) return fail(PT_ERR_INVALID, "width and height must be positive");
    if (cfg->samples_per_px < 0) return fail(PT_ERR_INVALID, "samples_per_px must be >= 0");
    if ((int64_t)cfg->width * cfg->height > (int64_t)1 << 28) return fail(PT_ERR_INVALID, "frame too large");
    // pixel slots are 32-bit: 1024 per 32x32 tile, also for the nearly empty tiles of a 1-pixel-wide frame
    if ((int64_t)((cfg->width + 31) / 32) * ((cfg->height + 31) / 32) > (int64_t)1 << 21)
        return fail(PT_ERR_INVALID, "frame too large (more than 2^21 tiles)");
    if (scene->num_materials < 0 || scene->num_objects < 0) return fail(PT_ERR_INVALID, "negative scene counts");
    if (scene->num_materials > 0 && !scene->materials) return fail(PT_ERR_INVALID, "materials is null");
    if (scene->num_objects > 0 && !scene->objects) return fail(PT_ERR_INVALID, "objects is null");
    return PT_OK;
}

// ---------------------------------------------------------------- per-device frame

// Pixels of 8x8 block `blk` of a shard (16 per 32x32 tile, the shard's tiles in order: the map of ptk::block_pixel) that lie inside the frame.
uint32_t block_pixels(const Frame &fr, const pt_shard &sh, uint32_t blk) {
    const uint32_t lt = blk >> 4, sb = blk & 15u;
    const uint32_t t = (uint32_t)sh.index + lt * (uint32_t)sh.count;
    const uint32_t ty = t / (uint32_t)fr.ntx, tx = t - ty * (uint32_t)fr.ntx;
    const int64_t x0 = (int64_t)tx * 32 + (sb & 3u) * 8, y0 = (int64_t)ty * 32 + (sb >> 2) * 8;
    const int64_t w = std::min<int64_t>(8, (int64_t)fr.cfg.width - x0), h = std::min<int64_t>(8, (int64_t)fr.cfg.height - y0);
    return w > 0 && h > 0 ? (uint32_t)(w * h) : 0u;
}

using TraceFn = void (*)(const TraceArgs);

// The shipping instantiations are <false,false,*,*>; STATS adds per-pixel counters, PROF the section profile.
// form (pt_kernels.h): FORM_SPLIT = dielectric hits leave for the glass queue, FORM_NESTED = the pass behind the split rounds (both: the
// bitmask scans of the reference-sized scenes only), FORM_ALL_IN_ONE = everything else.
TraceFn pick_trace(bool stats, bool prof, int scan, int form = ptk::FORM_ALL_IN_ONE) {
    using namespace ptk;
    if (prof) {
        if (scan == SCAN_UNIFORM) return trace_kernel<false, true, SCAN_UNIFORM, FORM_ALL_IN_ONE>;
        if (scan == SCAN_BVH || scan == SCAN_VERIFY_BVH) return trace_kernel<false, true, SCAN_BVH, FORM_ALL_IN_ONE>;
        if (scan == SCAN_BROAD_WIDE || scan == SCAN_VERIFY_WIDE) return trace_kernel<false, true, SCAN_BROAD_WIDE, FORM_ALL_IN_ONE>;
        return form == FORM_SPLIT ? trace_kernel<false, true, SCAN_BROAD, FORM_SPLIT>
               : form == FORM_NESTED ? trace_kernel<false, true, SCAN_BROAD, FORM_NESTED> : trace_kernel<false, true, SCAN_BROAD, FORM_ALL_IN_ONE>;
    }
#define PT_PICK(SCAN_, FORM_) (stats ? trace_kernel<true, false, SCAN_, FORM_> : trace_kernel<false, false, SCAN_, FORM_>)
    if (form != FORM_ALL_IN_ONE) {  // bitmask scans only (trace_form() never asks otherwise)
        const bool nest = form == FORM_NESTED;
        if (scan == SCAN_VERIFY) return nest ? PT_PICK(SCAN_VERIFY, FORM_NESTED) : PT_PICK(SCAN_VERIFY, FORM_SPLIT);
        if (scan == SCAN_BROAD_WIDE) return nest ? PT_PICK(SCAN_BROAD_WIDE, FORM_NESTED) : PT_PICK(SCAN_BROAD_WIDE, FORM_SPLIT);
        if (scan == SCAN_VERIFY_WIDE) return nest ? PT_PICK(SCAN_VERIFY_WIDE, FORM_NESTED) : PT_PICK(SCAN_VERIFY_WIDE, FORM_SPLIT);
        return nest ? PT_PICK(SCAN_BROAD, FORM_NESTED) : PT_PICK(SCAN_BROAD, FORM_SPLIT);
    }
    switch (scan) {
        case SCAN_BROAD: return PT_PICK(SCAN_BROAD, FORM_ALL_IN_ONE);
        case SCAN_VERIFY: return PT_PICK(SCAN_VERIFY, FORM_ALL_IN_ONE);
        case SCAN_BROAD_WIDE: return PT_PICK(SCAN_BROAD_WIDE, FORM_ALL_IN_ONE);
        case SCAN_VERIFY_WIDE: return PT_PICK(SCAN_VERIFY_WIDE, FORM_ALL_IN_ONE);
        case SCAN_BVH: return PT_PICK(SCAN_BVH, FORM_ALL_IN_ONE);
        case SCAN_VERIFY_BVH: return PT_PICK(SCAN_VERIFY_BVH, FORM_ALL_IN_ONE);
        default: return PT_PICK(SCAN_UNIFORM, FORM_ALL_IN_ONE);
    }
#undef PT_PICK
}

TraceFn pick_primary(bool stats, int scan) {
    using namespace ptk;
    if (scan == SCAN_VERIFY_BVH) return stats ? primary_bvh_kernel<true, true> : primary_bvh_kernel<false, true>;
    return stats ? primary_bvh_kernel<true, false> : primary_bvh_kernel<false, false>;
}

using GlassFn = void (*)(const ptk::GlassArgs);
GlassFn pick_glass(bool stats, int scan) {
    using namespace ptk;
    if (scan == SCAN_VERIFY) return stats ? glass_kernel<true, true, false> : glass_kernel<false, true, false>;
    if (scan == SCAN_BROAD_WIDE) return stats ? glass_kernel<true, false, true> : glass_kernel<false, false, true>;
    if (scan == SCAN_VERIFY_WIDE) return stats ? glass_kernel<true, true, true> : glass_kernel<false, true, true>;
    return stats ? glass_kernel<true, false, false> : glass_kernel<false, false, false>;
}

// The wavefront form's kernels (pt_wavefront.h, pt_walk32.h).  mode: 0 = closest hit, 1 = exit search.  The compiler emits the
// instantiations in the order this file first names them: the tables stand, and list their kernels, in the order that keeps the code
// object what it was when dev_begin and dev_step_wavefront named them (profiles/host_plan_kernel_regs.txt).
using WfFn = void (*)(const ptk::WfArgs);
using Walk32Fn = void (*)(const ptk::Walk32Args);
WfFn pick_wf_scan0(bool bvh) { return bvh ? ptk::wf_traverse_kernel<0, false> : ptk::wf_scan_flat_kernel<0, false>; }  // dev_begin's occupancy probe
Walk32Fn pick_wf_walk32(int mode, bool diag) {
    if (mode == 0 && !diag) return ptk::wf_walk32_kernel<0>;
    if (diag) return mode == 0 ? ptk::wf_walk32_kernel<0, true> : ptk::wf_walk32_kernel<1, true>;
    return ptk::wf_walk32_kernel<1>;
}
WfFn pick_wf_traverse(int mode, bool verify) {
    if (!verify) return mode == 0 ? ptk::wf_traverse_kernel<0, false> : ptk::wf_traverse_kernel<1, false>;
    return mode == 0 ? ptk::wf_traverse_kernel<0, true> : ptk::wf_traverse_kernel<1, true>;
}
WfFn pick_wf_scan_flat(int mode, bool verify) {
    if (verify) return mode == 0 ? ptk::wf_scan_flat_kernel<0, true> : ptk::wf_scan_flat_kernel<1, true>;
    return mode == 0 ? ptk::wf_scan_flat_kernel<0, false> : ptk::wf_scan_flat_kernel<1, false>;
}
WfFn pick_wf_init(bool stats) { return stats ? ptk::wf_init_kernel<true> : ptk::wf_init_kernel<false>; }
Walk32Fn pick_wf_shade32(bool stats, bool verify) {
    return stats ? (verify ? ptk::wf_shade32_kernel<true, true> : ptk::wf_shade32_kernel<true, false>)
                 : (verify ? ptk::wf_shade32_kernel<false, true> : ptk::wf_shade32_kernel<false, false>);
}
WfFn pick_wf_shade(bool stats) { return stats ? ptk::wf_shade_kernel<true> : ptk::wf_shade_kernel<false>; }
Walk32Fn pick_wf_exit32(bool stats, bool verify) {
    return stats ? (verify ? ptk::wf_exit32_kernel<true, true> : ptk::wf_exit32_kernel<true, false>)
                 : (verify ? ptk::wf_exit32_kernel<false, true> : ptk::wf_exit32_kernel<false, false>);
}
WfFn pick_wf_exit(bool stats) { return stats ? ptk::wf_exit_kernel<true> : ptk::wf_exit_kernel<false>; }

// One timed launch on d's stream: takes the next event pair of d.ev[kind] (making it if the list is short), records a, runs `launch` --
// one kernel launch, or several that are timed as one --, checks hipGetLastError and records b.  The pair is v[n - 1] afterwards.
template <typename Launch>
int32_t timed(Device &d, EventKind kind, Launch &&launch) {
    EventList &l = d.ev[kind];
    if (l.v.size() <= l.n) {
        EventPair e;
        HIP_TRY(hipEventCreate(&e.a));
        HIP_TRY(hipEventCreate(&e.b));
        l.v.push_back(e);
    }
    const EventPair e = l.v[l.n++];
    HIP_TRY(hipEventRecord(e.a, d.stream));
    launch();
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(e.b, d.stream));
    return PT_OK;
}

// A pass that has an adaptive form (pt_set_adaptive), one lane for each of `lanes`: `plain(args...)`, or in an adaptive frame
// `adapt(args..., table)`, the same body working through the frame's block tables.  Timed under `kind`; EV_KINDS: not timed.
template <typename Plain, typename Adapt, typename Table, typename... Args>
int32_t launch_pass(Device &d, bool adaptive, EventKind kind, uint32_t lanes, Plain plain, Adapt adapt, const Table &table, const Args &...args) {
    const dim3 grid((lanes + PT_BLOCK - 1) / PT_BLOCK), block(PT_BLOCK);
    auto launch = [&] {
        if (adaptive) hipLaunchKernelGGL(adapt, grid, block, 0, d.stream, args..., table);
        else hipLaunchKernelGGL(plain, grid, block, 0, d.stream, args...);
    };
    if (kind != EV_KINDS) return timed(d, kind, launch);
    launch();
    HIP_TRY(hipGetLastError());
    return PT_OK;
}
// The lanes of a pass over the slots a chunk adds to: every slot of the shard, in an adaptive frame those of the active blocks
uint32_t live_slots(const Frame &fr, const Device &d) { return fr.adaptive ? d.nact * 64u : d.nslots; }

// A timed launch of a trace pass (EV_TRACE), marked as the split form or not for pt_stats.trace_split_ms / trace_split_launches.
template <typename Launch>
int32_t timed_trace(Device &d, bool split, Launch &&launch) {
    const size_t i = d.ev[EV_TRACE].n;
    if (d.trace_is_split.size() <= i) d.trace_is_split.resize(i + 1);
    d.trace_is_split[i] = split ? 1 : 0;
    return timed(d, EV_TRACE, launch);
}

// Milliseconds between a and b, added up over the pairs the frame took from `l` (their device is current and has finished them);
// `flagged`: the share of the pairs i with flag[i] set.
int32_t sum_ms(const EventList &l, double &sum, const std::vector<char> *flag = nullptr, double *flagged = nullptr) {
    sum = 0;
    for (size_t i = 0; i < l.n; i++) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, l.v[i].a, l.v[i].b));
        sum += ms;
        if (flag && i < flag->size() && (*flag)[i]) *flagged += ms;
    }
    return PT_OK;
}

// A host table on device d: room for it (for `room` elements at least, never none: the kernels get a valid pointer for an empty
// table too) and, unless it is empty, the copy on d's stream.  (Pageable source: the copy is complete when the call returns.)
template <typename T>
int32_t upload(Device &d, DevBuf<T> &buf, const std::vector<T> &src, size_t room = 1) {
    HIP_TRY(buf.reserve(std::max(room, src.size())));
    if (!src.empty()) HIP_TRY(hipMemcpyAsync(buf.p, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, d.stream));
    return PT_OK;
}

// Blocks of `kernel` that a CU holds with `lds` bytes of dynamic LDS per block: at least 1, at most `cap`.
template <typename Kernel>
int32_t occupancy(Kernel kernel, size_t lds, int cap, int &blocks_per_cu) {
    int nb = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, PT_BLOCK, lds));
    blocks_per_cu = std::max(1, std::min(nb, cap));
    return PT_OK;
}

// The shard of the open frame that device d renders, for the slot -> pixel map of the kernels (ptk::block_pixel).
TileGeom tile_geom(const Frame &fr, const Device &d) { return TileGeom{fr.cfg.width, fr.cfg.height, fr.ntx, d.shard.index, d.shard.count}; }

#define PT_GLASS_MAX_BLOCKS_PER_CU 8

size_t walk32_lds_bytes() { return 0; }  // the stacks are static LDS of the kernel

// Slots a path-state queue needs beyond one per job of the pass: every wave of a pass that appends to it reserves slots in
// windows (one atomic per window, see trace_kernel) and may leave its last window partly empty -- fewer than one window per
// wave and pass.  Derived from the very grids the launches use (dev_step, dev_step_wavefront), none of which is wider
// than one block per PT_BLOCK items of the pass:
//   split form      glass queue <- trace_kernel<split> (num_cu x blocks_per_cu_split blocks, windows of PT_QUEUE_BLOCK)
//                   continuation queue <- glass_kernel (num_cu x blocks_per_cu_glass blocks, windows of PT_CONT_BLOCK)
//   wavefront form  path queue <- wf_shade_kernel AND wf_exit_kernel of one level (num_cu x PT_WF_PASS_BLOCKS_PER_CU blocks each)
// every window priced at PT_CONT_BLOCK (static_assert in pt_kernels.h: PT_QUEUE_BLOCK <= PT_CONT_BLOCK).
#define PT_WF_PASS_BLOCKS_PER_CU 4
size_t queue_slack(const pt_ctx *ctx, const Device &d, size_t njobs_max) {
    const Frame &fr = ctx->frame;
    const size_t grid_cap = std::max<size_t>(1, (njobs_max + PT_BLOCK - 1) / PT_BLOCK);
    size_t writer_blocks;
    if (fr.wavefront)
        writer_blocks = 2 * std::min<size_t>((size_t)d.num_cu * PT_WF_PASS_BLOCKS_PER_CU, grid_cap);
    else if (fr.primary_pass)  // continuation queue <- primary_bvh_kernel (num_cu x blocks_per_cu_primary blocks, windows of PT_CONT_BLOCK)
        writer_blocks = std::min<size_t>((size_t)d.num_cu * (size_t)d.blocks_per_cu_primary, grid_cap);
    else
        writer_blocks = std::min<size_t>((size_t)d.num_cu * (size_t)std::max(d.blocks_per_cu_split, d.blocks_per_cu_glass), grid_cap);
    return writer_blocks * (PT_BLOCK / PT_WAVE) * PT_CONT_BLOCK;
}

// The forms of the loop a frame runs, as far as the per-pass buffers go (PassWhen).  Path-state queues: three in the wavefront
// form, the continuation queue alone behind the primary pass of the BVH path, glass and continuation queue for the split rounds of
// a scene with glass.
unsigned frame_forms(const pt_ctx *ctx) {
    const Frame &fr = ctx->frame;
    const unsigned queues = fr.wavefront ? WHEN_Q_GLASS | WHEN_Q_CONT | WHEN_Q_PATH_B : fr.primary_pass ? WHEN_Q_CONT
                            : (fr.split_rounds > 0 && fr.has_glass) ? WHEN_Q_GLASS | WHEN_Q_CONT : 0u;
    return queues | (fr.wavefront && ctx->wf_sort ? WHEN_WF_SORT : 0u) | (fr.walk32 ? WHEN_WALK32 : 0u);
}

std::vector<PassBuf> pass_plan(Device &d) {
    std::vector<PassBuf> plan = {
        // 90 B per job: radiance record, primary ray, stream state, draw count; + 8 B with pixel stats
        {d.L, PER_JOB, 4, 0, 0}, {d.ray, PER_JOB, 6, 0, 0}, {d.ray_rng, PER_JOB, 1, 0, 0}, {d.ray_ndraw, PER_JOB, 1, 0, 0},
        {d.job_seg, PER_JOB, 0, 1, 0}, {d.job_draw, PER_JOB, 0, 1, 0}};
    d.q_glass.plan(plan, WHEN_Q_GLASS);
    d.q_cont.plan(plan, WHEN_Q_CONT);
    d.q_path_b.plan(plan, WHEN_Q_PATH_B);
    // ray sorting of the wavefront form: 8 B per entry; walk32: (PT_CAND_MAX + 2) x 4 B per entry
    plan.insert(plan.end(), {{d.wf_perm, PER_EXTRA, 1, 0, WHEN_WF_SORT}, {d.wf_key, PER_EXTRA, 1, 0, WHEN_WF_SORT},
                             {d.cand_ids, PER_EXTRA, PT_CAND_MAX, 0, WHEN_WALK32}, {d.cand_n, PER_EXTRA, 1, 0, WHEN_WALK32},
                             {d.slow_list, PER_EXTRA, 1, 0, WHEN_WALK32}});
    return plan;
}

// bytes of per-pass buffers a device holds right now (capacities: buffers never shrink, a frame may need less than is held)
size_t dev_held_bytes(Device &d) {
    size_t held = 0;
    for (const PassBuf &b : pass_plan(d)) held += *b.cap * b.size;
    return held;
}

// the samples per pass were chosen from the buffer budget (not forced by pt_config.spp_chunk)
bool cfg_chunk_free(const Frame &fr) { return fr.cfg.spp_chunk <= 0; }

// equal passes: ceil(spp / chunk) passes of ceil(spp / passes) samples instead of full passes and a short last one
void balance_chunk(Frame &fr) {
    const uint32_t spp = (uint32_t)std::max(1, fr.cfg.samples_per_px);
    if (fr.chunk >= spp) { fr.chunk = spp; return; }
    const uint32_t passes = (spp + fr.chunk - 1) / fr.chunk;
    fr.chunk = (spp + passes - 1) / passes;
}

int32_t dev_begin(pt_ctx *ctx, Device &d, const pt_shard &shard, hipStream_t stream) {
    Frame &fr = ctx->frame;
    const SceneData &sd = ctx->sd;
    HIP_TRY(hipSetDevice(d.ordinal));
    d.stream = stream ? stream : d.own_stream;
    d.shard = shard;
    d.nlocal = tiles_of_shard(fr.ntx * fr.nty, shard);
    d.nslots = (uint32_t)d.nlocal * 1024u;
    d.acc_started = false;
    for (EventList &l : d.ev) l.n = 0;
    d.first_recorded = false;
    std::memset(d.pass_log_prev, 0, sizeof d.pass_log_prev);  // the device counters are cleared below, once per frame
    if (d.scene_gen != sd.gen) {
        if (int32_t rc = upload(d, d.objs, sd.world)) return rc;
        if (int32_t rc = upload(d, d.mats, sd.mats)) return rc;
        if (int32_t rc = upload(d, d.roulette, sd.roulette)) return rc;
        if (int32_t rc = upload(d, d.bsph, sd.bsph)) return rc;
        if (int32_t rc = upload(d, d.bbox, sd.bbox)) return rc;
        if (int32_t rc = upload(d, d.plane_idx, sd.plane_idx)) return rc;
        if (int32_t rc = upload(d, d.bsph_diel, sd.bsph_diel)) return rc;
        if (int32_t rc = upload(d, d.bbox_diel, sd.bbox_diel)) return rc;
        if (d.topo_gen != sd.topo_gen) {  // (a world that only moved, pt_set_bvh_refit, keeps the hierarchy this device holds)
            if (int32_t rc = upload(d, d.bvh_nodes, sd.bvh_nodes)) return rc;
            if (int32_t rc = upload(d, d.bvh_objs, sd.bvh_objs)) return rc;
            if (int32_t rc = upload(d, d.bvh_cores, sd.bvh_cores)) return rc;
        }
        // ... and is brought to the moved world here, from the world just uploaded: every device refits its own copy, and the
        // result depends on the topology and this world only (pt_bvh_refit.h)
        const bool refit = sd.tree_moved && !sd.bvh_nodes.empty();
        const int32_t n_nodes = (int32_t)sd.bvh_nodes.size(), cost_nodes = sd.Fs.bvh_main_nodes;
        if (refit) {
            HIP_TRY(d.rf_box.reserve(6 * (size_t)n_nodes));
            HIP_TRY(d.rf_area.reserve((size_t)n_nodes));
            HIP_TRY(d.rf_part.reserve(std::max<size_t>(1, ptrf::cost_blocks(cost_nodes))));
            hipError_t e = hipSuccess;
            if (int32_t rc = timed(d, EV_REFIT, [&] {
                    e = ptrf::refit_launch(d.stream, d.bvh_nodes.p, d.bvh_objs.p, d.objs.p, (int32_t)sd.bvh_objs.size(), sd.bvh_levels.data(),
                                           (int)sd.bvh_levels.size() - 1, sd.bvh_margin, d.rf_box.p, d.rf_area.p, cost_nodes, d.rf_part.p);
                }))
                return rc;
            HIP_TRY(e);
        }
        HIP_TRY(hipStreamSynchronize(d.stream));
        d.scene_gen = sd.gen;
        d.topo_gen = sd.topo_gen;
        if (refit && &d == &ctx->devs[0]) {  // the figure of the refitted tree and the time it took, from devices[0]
            std::vector<double> part(ptrf::cost_blocks(cost_nodes));
            if (!part.empty()) HIP_TRY(hipMemcpy(part.data(), d.rf_part.p, part.size() * sizeof(double), hipMemcpyDeviceToHost));
            double total = 0.0;
            for (double p : part) total += p;
            double ms = 0.0;
            if (int32_t rc = sum_ms(d.ev[EV_REFIT], ms)) return rc;
            ctx->rf.st.cost_now = total;
            ctx->rf.st.refit_ms = ms;
            ctx->rf.figure_pending = false;
        }
    }
    HIP_TRY(d.queue.reserve(8));
    HIP_TRY(d.counters.reserve(48));
    HIP_TRY(hipMemsetAsync(d.counters.p, 0, 48 * sizeof(unsigned long long), d.stream));
    if (fr.fog_vol) {
        HIP_TRY(d.fog_counters.reserve(3));
        HIP_TRY(hipMemsetAsync(d.fog_counters.p, 0, 3 * sizeof(unsigned long long), d.stream));
        if (int32_t rc = upload(d, d.fog_lights, fr.fog_lights)) return rc;
    }
    if (fr.fog_walk) {  // the walk's counters, zeroed when the frame opens
        HIP_TRY(d.fog_walk_counters.reserve(6));
        HIP_TRY(hipMemsetAsync(d.fog_walk_counters.p, 0, 6 * sizeof(unsigned long long), d.stream));
    }
    if (fr.gl_walk) {  // the walk's counters, zeroed when the frame opens
        HIP_TRY(d.gl_walk_counters.reserve(7));
        HIP_TRY(hipMemsetAsync(d.gl_walk_counters.p, 0, 7 * sizeof(unsigned long long), d.stream));
    }
    if (fr.gl) {
        HIP_TRY(d.gl_counters.reserve(5));
        HIP_TRY(hipMemsetAsync(d.gl_counters.p, 0, 5 * sizeof(unsigned long long), d.stream));
        if (int32_t rc = upload(d, d.gl_objs, fr.gl_objs)) return rc;
        if (int32_t rc = upload(d, d.gl_mats, fr.gl_mats)) return rc;
        if (int32_t rc = upload(d, d.gl_lights, fr.gl_lights)) return rc;
    }
    if (ctx->profile_sections) {
        HIP_TRY(d.prof.reserve(3 * ptk::SEC_COUNT));
        HIP_TRY(hipMemsetAsync(d.prof.p, 0, 3 * ptk::SEC_COUNT * sizeof(unsigned long long), d.stream));
    }
    const size_t ns = std::max<uint32_t>(1, d.nslots);
    HIP_TRY(d.acc.reserve(3 * ns));
    if (fr.moments) HIP_TRY(d.m2.reserve(3 * ns));
    if (fr.adaptive) {  // every block with a pixel inside the frame starts active, in block order
        std::vector<uint32_t> act;
        for (uint32_t blk = 0; blk < d.nslots / 64u; blk++)
            if (block_pixels(fr, d.shard, blk) > 0) act.push_back(blk);
        const size_t nb = std::max<size_t>(1, d.nslots / 64u);
        if (int32_t rc = upload(d, d.act[0], act, nb)) return rc;
        HIP_TRY(d.act[1].reserve(nb));
        HIP_TRY(d.blk_spp.reserve(nb));
        HIP_TRY(d.blk_keep.reserve(nb));
        HIP_TRY(d.blk_noise.reserve(nb));
        HIP_TRY(d.ad_res.reserve(1));
        HIP_TRY(hipMemsetAsync(d.blk_spp.p, 0, nb * sizeof(uint32_t), d.stream));
        d.act_cur = 0;
        d.nact = (uint32_t)act.size();
    }
    if (fr.stats_on) {
        HIP_TRY(d.acc_seg.reserve(ns));
        HIP_TRY(d.acc_draw.reserve(ns));
    }
    if (!d.ev_first) {
        HIP_TRY(hipEventCreate(&d.ev_first));
        HIP_TRY(hipEventCreate(&d.ev_last));
    }
    // occupancy of the kernels of this frame for the scene's LDS footprint (before the buffers: the queue slack depends on it)
    const size_t lds = fr.lds_bytes;
    const int max_bpc = ctx->max_blocks_per_cu;
    if (int32_t rc = occupancy(pick_trace(fr.stats_on, ctx->profile_sections, fr.scan, fr.tail_form), lds, max_bpc, d.blocks_per_cu)) return rc;
    d.blocks_per_cu_split = d.blocks_per_cu;
    d.blocks_per_cu_glass = 1;
    if (fr.wavefront) {
        const bool bvh = fr.scan == ptk::SCAN_BVH || fr.scan == ptk::SCAN_VERIFY_BVH;
        if (int32_t rc = occupancy(pick_wf_scan0(bvh), lds, max_bpc, d.blocks_per_cu_wf)) return rc;
        if (fr.walk32) {
            if (int32_t rc = occupancy(pick_wf_walk32(0, false), walk32_lds_bytes(), max_bpc, d.blocks_per_cu_walk)) return rc;
            if (std::getenv("PTCORE_VERBOSE")) std::fprintf(stderr, "ptcore: walk32: %d blocks per CU for the FP32 walk, %d for the FP64 traversal of the slow list\n", d.blocks_per_cu_walk, d.blocks_per_cu_wf);
        }
    }
    if (fr.primary_pass)
        if (int32_t rc = occupancy(pick_primary(fr.stats_on, fr.scan), 0, 8, d.blocks_per_cu_primary)) return rc;
    if (fr.split_rounds > 0) {
        if (int32_t rc = occupancy(pick_trace(fr.stats_on, ctx->profile_sections, fr.scan, ptk::FORM_SPLIT), lds, max_bpc, d.blocks_per_cu_split)) return rc;
        if (int32_t rc = occupancy(pick_glass(fr.stats_on, fr.scan), fr.glass_lds_bytes, PT_GLASS_MAX_BLOCKS_PER_CU, d.blocks_per_cu_glass)) return rc;
    }
    // per-pass buffers (pass_plan): 90 B per job and, for the forms that park paths in HBM, one to three path-state queues with one
    // entry per job at most, plus the slots the waves of the writing passes reserve in windows and may leave empty
    const std::vector<PassBuf> plan = pass_plan(d);
    const unsigned forms = frame_forms(ctx);
    const bool queues = (forms & WHEN_Q_CONT) != 0;  // (every form with queues has that one)
    auto queue_cap = [&](size_t njobs_max) { return njobs_max + queue_slack(ctx, d, njobs_max); };
    auto need_bytes = [&](uint32_t chunk) {
        const size_t nj = (size_t)ns * chunk, nq = queue_cap(nj);
        size_t need = 0;
        for (const PassBuf &b : plan) need += (b.per == PER_JOB ? nj : nq) * b.used(forms, fr.stats_on) * b.size;
        return need;
    };
    // The budget covers everything a pass holds, the window slack of the queues included: when the queues push the total over it,
    // the samples per pass shrink (a frame is cut into more passes; pixels do not depend on that).
    if (cfg_chunk_free(fr) && need_bytes(fr.chunk) > fr.budget_bytes) {
        size_t per = 0;  // per sample of the pass without the slack: the jobs and one queue entry per job
        for (const PassBuf &b : plan)
            if (b.per != PER_EXTRA) per += (size_t)ns * b.used(forms, fr.stats_on) * b.size;
        const size_t fixed = need_bytes(1) > per ? need_bytes(1) - per : 0;
        fr.chunk = (uint32_t)std::max<size_t>(1, fr.budget_bytes > fixed ? (fr.budget_bytes - fixed) / per : 1);
        while (fr.chunk > 1 && need_bytes(fr.chunk) > fr.budget_bytes) fr.chunk -= std::max(1u, fr.chunk / 64u);
        balance_chunk(fr);
    }
    // A device that once could not give the budget keeps the size that fitted (trying the full budget again on every frame costs
    // seconds of hipMalloc / hipFree per frame when two processes share one GPU) -- until the device shows room for it again.
    if (d.bytes_cap && need_bytes(fr.chunk) > d.bytes_cap) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b + dev_held_bytes(d) >= need_bytes(fr.chunk) + need_bytes(fr.chunk) / 16) {
            d.bytes_cap = 0;  // whatever took the memory is gone: back to the full size
        } else {
            while (fr.chunk > 1 && need_bytes(fr.chunk) > d.bytes_cap) fr.chunk = std::max<uint32_t>(1, fr.chunk / 2);
        }
    }
    // when the device cannot give that much right now the chunk is halved until it can
    // (the ordered accumulation makes the pixels independent of the chunk size)
    for (;;) {
        const size_t njobs_max = (size_t)ns * fr.chunk;
        size_t qcap = queues ? queue_cap(njobs_max) : 0;
        // PTCORE_DEBUG_QUEUE_CAP=<entries> (tests only): queues too small for the frame, to show that an overflow fails the
        // frame with PT_ERR_STATE instead of writing outside them
        if (const char *dbg = queues ? std::getenv("PTCORE_DEBUG_QUEUE_CAP") : nullptr) qcap = (size_t)std::max(64L, std::atol(dbg));
        hipError_t e = hipSuccess;
        for (const PassBuf &b : plan)
            if (const size_t n = (b.per == PER_JOB ? njobs_max : qcap) * b.used(forms, fr.stats_on))
                if (e == hipSuccess) e = dev_reserve(b.p, b.cap, n, b.size);
        if (e == hipSuccess && fr.wavefront && ctx->wf_sort) e = d.wf_bins.reserve(PT_WF_BINS + 8);
        if (queues) d.q_cap = qcap;
        if (e == hipSuccess) break;
        (void)hipGetLastError();
        if (e != hipErrorOutOfMemory || fr.chunk <= 1) return fail(PT_ERR_HIP, std::string("job buffers: ") + hipGetErrorString(e));
        for (const PassBuf &b : plan) dev_release(b.p, b.cap);
        fr.chunk = std::max<uint32_t>(1, fr.chunk / 2);
        d.bytes_cap = need_bytes(fr.chunk);
        if (std::getenv("PTCORE_VERBOSE")) std::fprintf(stderr, "ptcore: device %d is short of memory, samples per pass reduced to %u\n", d.ordinal, fr.chunk);
    }
    return PT_OK;
}

// One chunk in the wavefront form (pt_wavefront.h): primary rays are in the ray buffers (raygen_kernel ran); queue words:
// [0] item cursor of the running traversal pass, [1] [2] entries of the two path queues, [3] entries of the exit queue.
int32_t dev_step_wavefront(pt_ctx *ctx, Device &d, const DevFrame &F, const TraceBuffers &B) {
    Frame &fr = ctx->frame;
    const bool bvh = fr.scan == ptk::SCAN_BVH || fr.scan == ptk::SCAN_VERIFY_BVH;
    const bool verify = fr.scan == ptk::SCAN_VERIFY_BVH || fr.scan == ptk::SCAN_VERIFY;
    const bool stats = fr.stats_on;
    unsigned int *qw = d.queue.p;
    const PathQueue qa = d.q_cont.bind(d.q_cap, stats, qw + 1), qb = d.q_path_b.bind(d.q_cap, stats, qw + 2);
    const PathQueue qe = d.q_glass.bind(d.q_cap, stats, qw + 3);
    ptk::WfArgs A;
    std::memset(&A, 0, sizeof A);
    A.F = F;
    A.F.fresh = F.njobs;
    A.F.bvh_min_lanes = ctx->wf_min_lanes;
    A.sky = fr.sky;
    A.B = B;
    A.cursor = qw;
    const size_t lds_scan = fr.lds_bytes, lds_shade = fr.shade_lds_bytes, lds_mat = (size_t)F.nmat * sizeof(DevMat);
    const dim3 block(PT_BLOCK);
    const uint32_t blocks_all = (F.njobs + PT_BLOCK - 1) / PT_BLOCK;
    const uint32_t grid_scan = std::max(1u, std::min((uint32_t)(d.num_cu * d.blocks_per_cu_wf), blocks_all));
    // shading passes: PT_WF_PASS_BLOCKS_PER_CU blocks per CU.  Their waves append to the next level's queue in windows of
    // PT_CONT_BLOCK slots (one atomic per window: a pass this short cannot afford more on one address); shade + exit pass
    // together leave at most 2 x grid_pass x 4 waves x PT_CONT_BLOCK slots empty, which is what queue_slack() allocates.
    const uint32_t grid_pass = std::max(1u, std::min((uint32_t)(d.num_cu * PT_WF_PASS_BLOCKS_PER_CU), blocks_all));
    const int levels = std::max(0, fr.cfg.max_depth);
    // walk32 (pt_walk32.h): the FP32 walk lists candidates, the FP64 traversal answers the few entries the walk hands over
    const bool walk32 = fr.walk32 && bvh;
    const bool walk_diag = std::getenv("PTCORE_WALK_STATS") != nullptr;
    auto walk_args = [&]() {
        ptk::Walk32Args K;
        std::memset(&K, 0, sizeof K);
        K.W = A;
        K.cand_ids = d.cand_ids.p;
        K.cand_n = d.cand_n.p;
        K.slow_list = d.slow_list.p;
        K.slow_count = qw + 6;
        K.cores = d.bvh_cores.p;
        K.min_lanes = ctx->wf_min_lanes;
        K.diag = d.counters.p + 24;
        return K;
    };
    const uint32_t grid_walk = std::max(1u, std::min((uint32_t)(d.num_cu * std::max(1, d.blocks_per_cu_walk)), blocks_all));
    auto scan_pass = [&](int mode) -> int32_t {
        HIP_TRY(hipMemsetAsync(qw, 0, sizeof(unsigned int), d.stream));
        if (!walk32)
            return timed_trace(d, false, [&] {
                hipLaunchKernelGGL(bvh ? pick_wf_traverse(mode, verify) : pick_wf_scan_flat(mode, verify), dim3(grid_scan), block, lds_scan, d.stream, A);
            });
        HIP_TRY(hipMemsetAsync(qw + 6, 0, sizeof(unsigned int), d.stream));
        const ptk::Walk32Args K = walk_args();
        if (int32_t rc = timed_trace(d, false, [&] {
                hipLaunchKernelGGL(pick_wf_walk32(mode, walk_diag), dim3(grid_walk), block, walk32_lds_bytes(), d.stream, K);
            }))
            return rc;
        // the entries the walk handed over, through the FP64 traversal (their number lives on the device)
        HIP_TRY(hipMemsetAsync(qw, 0, sizeof(unsigned int), d.stream));
        ptk::WfArgs S = A;
        S.perm = d.slow_list.p;
        S.n_sorted = qw + 6;
        const uint32_t grid_slow = std::max(1u, std::min(grid_scan, (uint32_t)d.num_cu));
        return timed_trace(d, false, [&] { hipLaunchKernelGGL(pick_wf_traverse(mode, false), dim3(grid_slow), block, lds_scan, d.stream, S); });
    };
    // a level's shading pass and its exit pass: the exact tests of the walk's candidates in front with walk32
    auto shade_pass = [&](Walk32Fn with_walk, WfFn plain, size_t lds_plain) {
        return timed(d, EV_GLASS, [&] {
            if (walk32) hipLaunchKernelGGL(with_walk, dim3(grid_pass), block, lds_mat, d.stream, walk_args());
            else hipLaunchKernelGGL(plain, dim3(grid_pass), block, lds_plain, d.stream, A);
        });
    };
    // fresh jobs -> queue A
    A.qin = qa;
    A.qout = qb;
    A.qexit = qe;
    if (int32_t rc = timed(d, EV_GLASS, [&] {
            hipLaunchKernelGGL(pick_wf_init(stats), dim3(std::min(blocks_all, (uint32_t)d.num_cu * 8u)), block, 0, d.stream, A);
        }))
        return rc;
    PathQueue cur_in = qa, cur_out = qb;
    for (int level = 0; level < levels; level++) {
        A.qin = cur_in;
        A.qout = cur_out;
        A.qexit = qe;
        A.perm = nullptr;
        if (ctx->wf_sort && level >= 1 && bvh) {
            // primary rays leave raygen_kernel in pixel order, which is coherent; from the first bounce on the queue order
            // means nothing, and the traversal pass takes the rays by direction octant and cell of the origin instead
            A.bin_count = d.wf_bins.p;
            A.bin_key = d.wf_key.p;
            HIP_TRY(hipMemsetAsync(d.wf_bins.p, 0, (PT_WF_BINS + 1) * sizeof(uint32_t), d.stream));
            if (int32_t rc = timed(d, EV_GLASS, [&] {
                    hipLaunchKernelGGL(ptk::wf_bin_count_kernel, dim3(grid_pass), block, 0, d.stream, A);
                    hipLaunchKernelGGL(ptk::wf_bin_scan_kernel, dim3(1), dim3(1024), 0, d.stream, A);
                    hipLaunchKernelGGL(ptk::wf_bin_scatter_kernel, dim3(grid_pass), block, 0, d.stream, A, d.wf_perm.p);
                }))
                return rc;
            A.perm = d.wf_perm.p;
            A.n_sorted = d.wf_bins.p + PT_WF_BINS;
        }
        if (int32_t rc = scan_pass(0)) return rc;
        A.perm = nullptr;
        HIP_TRY(hipMemsetAsync(cur_out.count, 0, sizeof(unsigned int), d.stream));
        HIP_TRY(hipMemsetAsync(qe.count, 0, sizeof(unsigned int), d.stream));
        if (int32_t rc = shade_pass(pick_wf_shade32(stats, verify), pick_wf_shade(stats), lds_shade)) return rc;
        if (fr.has_glass) {
            A.qin = qe;
            if (int32_t rc = scan_pass(1)) return rc;
            if (int32_t rc = shade_pass(pick_wf_exit32(stats, verify), pick_wf_exit(stats), lds_mat)) return rc;
        }
        std::swap(cur_in, cur_out);
        // deep presets (the "final" mode asks for 80 levels): stop as soon as no path is left
        if (level >= 8 && level % 4 == 0 && level + 1 < levels) {
            unsigned int left = 0;
            HIP_TRY(hipMemcpyAsync(&left, cur_in.count, sizeof left, hipMemcpyDeviceToHost, d.stream));
            HIP_TRY(hipStreamSynchronize(d.stream));
            if (left == 0) break;
        }
    }
    return PT_OK;
}

// ---- dev_step's stages, in the order they run.  F is the chunk's DevFrame (F.s0, F.S, F.njobs), G the device's tile map.

// GL shading: one pass per job, camera rays made in the kernel (pt_glshade.h)
void gl_scene(const Frame &fr, const Device &d, const TileGeom &G, ptg::GlScene &GS) {
    GS.objs = d.gl_objs.p;
    GS.mats = d.gl_mats.p;
    GS.lights = d.gl_lights.p;
    GS.nobj = (int32_t)fr.gl_objs.size();
    GS.nlight = (int32_t)fr.gl_lights.size();
    GS.sky = fr.gl_sky;
    GS.cam = fr.gl_cam;
    GS.max_depth = fr.cfg.max_depth;
    GS.width = G.width;
    GS.height = G.height;
    GS.fog_on = fr.fog_vol ? 1 : 0;
    GS.fog = fr.fog;
    GS.fog_objs = d.objs.p;
    GS.fog_lights = d.fog_lights.p;
    GS.fog_nobj = fr.nobj;
    GS.fog_nlight = (int32_t)fr.fog_lights.size();
}

int32_t step_gl(pt_ctx *ctx, Device &d, const DevFrame &F, const TileGeom &G) {
    const Frame &fr = ctx->frame;
    ptk::GlArgs GA;
    std::memset(&GA, 0, sizeof GA);
    gl_scene(fr, d, G, GA.S);
    GA.L = d.L.p;
    GA.counters = d.counters.p;
    GA.gl_counters = d.gl_counters.p;
    GA.fog_counters = fr.fog_vol ? d.fog_counters.p : nullptr;
    GA.key = ptm::seed_key(fr.cfg.seed ^ PTG_STREAM_SALT);
    GA.fog_key = ptm::seed_key(fr.cfg.seed ^ PTF_STREAM_SALT);
    GA.njobs = F.njobs;
    GA.nS = F.S;
    GA.s0 = F.s0;
    GA.ntx = G.ntx;  // (the frame size is GS's)
    GA.shard_index = G.shard_index;
    GA.shard_count = G.shard_count;
    if (fr.gl_walk) {  // BVH scans with pt_set_shading_walk: the same jobs, the model's ray queries by the lane's walk of the resident tree
        const ptk::GlWalkArgs W{GA, F, d.bvh_nodes.p, d.bvh_objs.p, d.plane_idx.p, d.gl_walk_counters.p};
        const size_t stack_bytes = (size_t)F.bvh_stack * PT_BLOCK * sizeof(int);
        return timed_trace(d, false, [&] { hipLaunchKernelGGL(ptk::gl_bvh_kernel, dim3((F.njobs + PT_BLOCK - 1) / PT_BLOCK), dim3(PT_BLOCK), stack_bytes, d.stream, W); });
    }
    return timed_trace(d, false, [&] { hipLaunchKernelGGL(ptk::gl_trace_kernel, dim3((F.njobs + PT_BLOCK - 1) / PT_BLOCK), dim3(PT_BLOCK), 0, d.stream, GA); });
}

// Ray generation (`active`: the adaptive frame's list of blocks), then pt_debug_set_primary_rays' table over its rays
int32_t step_raygen(pt_ctx *ctx, Device &d, const DevFrame &F, const uint32_t *active) {
    const Frame &fr = ctx->frame;
    const dim3 block(PT_BLOCK), per_job((F.njobs + PT_BLOCK - 1) / PT_BLOCK);
    const char *rg_form = std::getenv("PTCORE_RAYGEN");  // A/B: "column" = round 2's walk down a lane's column, "simple" = one job per lane
    const bool rg_simple = std::getenv("PTCORE_RAYGEN_SIMPLE") || (rg_form && !std::strcmp(rg_form, "simple"));
    if (!fr.adaptive && fr.cam.lens_radius > 0 && !rg_simple) {  // thin lens: the rejection loop over a wave's pool of jobs, or down a lane's column
        const bool pool = !(rg_form && !std::strcmp(rg_form, "column"));
        const uint32_t per_block = PT_BLOCK * (pool ? PT_RG_POOL_ROWS : PT_RG_ROWS);
        if (int32_t rc = timed(d, EV_RAYGEN, [&] {
                hipLaunchKernelGGL(pool ? ptk::raygen_lens_pool_kernel : ptk::raygen_lens_kernel, dim3((F.njobs + per_block - 1) / per_block), block, 0,
                                   d.stream, F, fr.cam, d.ray.p, d.ray_rng.p, d.ray_ndraw.p);
            }))
            return rc;
    } else if (int32_t rc = launch_pass(d, fr.adaptive, EV_RAYGEN, F.njobs, ptk::raygen_kernel, ptk::raygen_adaptive_kernel, active, F, fr.cam, d.ray.p,
                                        d.ray_rng.p, d.ray_ndraw.p)) {
        return rc;
    }
    if (ctx->inject_rays.empty()) return PT_OK;
    if (d.inject_gen != ctx->inject_gen) {
        HIP_TRY(hipStreamSynchronize(d.stream));
        HIP_TRY(d.inject.reserve(ctx->inject_rays.size()));
        HIP_TRY(hipMemcpy(d.inject.p, ctx->inject_rays.data(), ctx->inject_rays.size() * sizeof(double), hipMemcpyHostToDevice));
        d.inject_gen = ctx->inject_gen;
    }
    hipLaunchKernelGGL(ptk::inject_rays_kernel, per_job, block, 0, d.stream, F, d.inject.p, (uint64_t)(ctx->inject_rays.size() / 6),
                       (uint32_t)fr.cfg.samples_per_px, d.ray.p, d.ray_ndraw.p);
    HIP_TRY(hipGetLastError());
    return PT_OK;
}

// PTCORE_DEBUG_TIMELINE (diagnostics): when each wave of the trace launch just timed retired; serialises the stream
int32_t print_timeline(Device &d, const char *pass, int form, uint32_t grid) {
    const EventPair &e = d.ev[EV_TRACE].v[d.ev[EV_TRACE].n - 1];
    HIP_TRY(hipStreamSynchronize(d.stream));
    const uint32_t nw = std::min(grid * 4u, 65536u);
    std::vector<unsigned long long> t(nw);
    HIP_TRY(hipMemcpy(t.data(), d.prof.p, nw * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    std::sort(t.begin(), t.end());
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, e.a, e.b));
    auto back = [&](double q) { return (double)(t[nw - 1] - t[(size_t)(q * (nw - 1))]) * 1e-5; };  // ms before the last wave
    double mean = 0;
    for (auto v : t) mean += (double)(t[nw - 1] - v);
    std::fprintf(stderr, "ptcore timeline: %s form %d  %.3f ms, %u waves; before the last wave retired: first %.3f ms, 1 %% %.3f, 10 %% %.3f, 25 %% %.3f, 50 %% %.3f, 75 %% %.3f, 90 %% %.3f, 99 %% %.3f; mean %.3f ms\n",
                 pass, form, ms, nw, back(0.0), back(0.01), back(0.10), back(0.25), back(0.50), back(0.75), back(0.90), back(0.99), mean / nw * 1e-5);
    return PT_OK;
}

// PTCORE_DEBUG_PASS_LOG=1 (diagnostics): what the trace pass just timed did (`pass` null: the primary pass); serialises the stream
int32_t print_pass_log(Device &d, const char *pass, uint32_t grid) {
    const EventPair &e = d.ev[EV_TRACE].v[d.ev[EV_TRACE].n - 1];
    HIP_TRY(hipStreamSynchronize(d.stream));
    unsigned long long c[48];
    HIP_TRY(hipMemcpy(c, d.counters.p, sizeof c, hipMemcpyDeviceToHost));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, e.a, e.b));
    const unsigned long long *prev = d.pass_log_prev;
    if (pass)
        std::fprintf(stderr, "ptcore pass: %s grid %u  %.3f ms  segments +%llu  exit scans +%llu  parked +%llu  ended here +%llu  continuations in +%llu  -> %.1f Mseg/s\n",
                     pass, grid, ms, c[0] - prev[0], c[1] - prev[1], c[5] - prev[5], c[18] - prev[18], c[7] - prev[7], (double)(c[0] - prev[0]) / (ms * 1e3));
    else
        std::fprintf(stderr, "ptcore pass: primary<wave> grid %u  %.3f ms  segments shaded %llu  handed on %llu  wave-level node visits %llu over %llu blocks of 64 jobs (%llu more handed over unwalked)\n",
                     grid, ms, c[0] - prev[0], c[6], c[40], c[41], c[42]);
    std::memcpy(d.pass_log_prev, c, sizeof d.pass_log_prev);
    return PT_OK;
}

// The trace schedule of the all-in-one loop and its split forms.  Queue words: [0] item cursor of the running trace pass, [1] glass
// entries, [2],[3] continuation entries (one is read by a trace pass while glass_kernel fills the other), [4] stays 0 (a first pass
// starts from no continuations)
int32_t step_trace(pt_ctx *ctx, Device &d, const DevFrame &F, TraceBuffers &B, bool timeline) {
    const Frame &fr = ctx->frame;
    unsigned int *qw = d.queue.p;
    const dim3 block(PT_BLOCK);
    const int rounds = fr.split_rounds;
    const uint32_t waves_needed = (F.njobs + 63u) / 64u, blocks_all = (F.njobs + PT_BLOCK - 1) / PT_BLOCK;
    const bool pass_log = std::getenv("PTCORE_DEBUG_PASS_LOG") != nullptr;
    auto launch_trace = [&](bool split, bool first) -> int32_t {
        TraceArgs A;
        A.F = F;
        A.F.fresh = first ? F.njobs : 0u;
        A.sky = fr.sky;
        A.B = B;
        uint32_t grid = (uint32_t)(d.num_cu * (split ? d.blocks_per_cu_split : d.blocks_per_cu));
        // (later passes: the item count lives on the device; no pass holds more items than the chunk has jobs, which is also
        // the bound queue_slack() assumes)
        grid = std::max(1u, std::min(grid, (waves_needed + 3u) / 4u));
        const int form = split ? (int)ptk::FORM_SPLIT : fr.tail_form;
        if (int32_t rc = timed_trace(d, split, [&] {
                hipLaunchKernelGGL(pick_trace(fr.stats_on, ctx->profile_sections, fr.scan, form), dim3(grid), block, fr.lds_bytes, d.stream, A);
            }))
            return rc;
        if (timeline)
            if (int32_t rc = print_timeline(d, split ? "trace<split>" : "trace<tail>", split ? 1 : fr.tail_form, grid)) return rc;
        if (pass_log) return print_pass_log(d, split ? "trace<split>" : "trace<all-in-one>", grid);
        return PT_OK;
    };
    if (fr.primary_pass) {
        // BVH scenes: the first segment of every path by the wave-cooperative kernel (pt_primary.h); what goes on -- and what that
        // kernel is not meant for, unshaded -- reaches the per-lane loop through the continuation queue
        B.cont_in = qw + 2;
        B.cont.count = qw + 2;
        TraceArgs A;
        A.F = F;
        A.F.fresh = 0u;
        A.sky = fr.sky;
        A.B = B;
        const uint32_t pgrid = std::max(1u, std::min((uint32_t)(d.num_cu * d.blocks_per_cu_primary), blocks_all));  // same bound as queue_slack()
        if (int32_t rc = timed_trace(d, false, [&] { hipLaunchKernelGGL(pick_primary(fr.stats_on, fr.scan), dim3(pgrid), block, 0, d.stream, A); }))
            return rc;
        if (pass_log)
            if (int32_t rc = print_pass_log(d, nullptr, pgrid)) return rc;
        return launch_trace(false, false);
    }
    if (rounds == 0) return launch_trace(false, true);
    // Split passes: trace (dielectric hits -> glass queue), glass (-> continuation queue), `rounds` times; what is
    // still under way then (paths with more than `rounds` dielectric bounces) finishes in the all-in-one form.
    const uint32_t glass_grid = std::max(1u, std::min((uint32_t)(d.num_cu * d.blocks_per_cu_glass), blocks_all));  // same bound as queue_slack()
    for (int r = 0; r < rounds; r++) {
        if (r > 0) HIP_TRY(hipMemsetAsync(qw, 0, 2 * sizeof(unsigned int), d.stream));  // cursor and glass count
        unsigned int *c_in = r == 0 ? qw + 4 : qw + 2 + (r & 1), *c_out = qw + 2 + ((r + 1) & 1);
        HIP_TRY(hipMemsetAsync(c_out, 0, sizeof(unsigned int), d.stream));
        B.cont_in = c_in;
        B.cont.count = c_out;
        if (int32_t rc = launch_trace(true, r == 0)) return rc;
        if (!fr.has_glass) return PT_OK;  // nothing can have entered the glass queue: the frame is done
        ptk::GlassArgs GA;
        GA.F = F;
        GA.B = B;
        if (int32_t rc = timed(d, EV_GLASS, [&] {
                hipLaunchKernelGGL(pick_glass(fr.stats_on, fr.scan), dim3(glass_grid), block, fr.glass_lds_bytes, d.stream, GA);
            }))
            return rc;
    }
    HIP_TRY(hipMemsetAsync(qw, 0, sizeof(unsigned int), d.stream));
    B.cont_in = qw + 2 + (rounds & 1);
    B.cont.count = qw + 5;  // unused by the all-in-one form
    return launch_trace(false, false);
}

// The fog's in-scatter term into the chunk's radiance records (pt_fog.h)
int32_t step_fog(pt_ctx *ctx, Device &d, const DevFrame &F, const TileGeom &G, const uint32_t *active) {
    const Frame &fr = ctx->frame;
    ptk::FogArgs FA;
    std::memset(&FA, 0, sizeof FA);
    FA.P = fr.fog;
    FA.objs = d.objs.p;
    FA.lights = d.fog_lights.p;
    FA.ray = d.ray.p;
    FA.ray_ndraw = d.ray_ndraw.p;
    FA.L = d.L.p;
    FA.counters = d.fog_counters.p;
    FA.fog_key = ptm::seed_key(fr.cfg.seed ^ PTF_STREAM_SALT);
    FA.nobj = fr.nobj;
    FA.nlight = (int32_t)fr.fog_lights.size();
    FA.njobs = F.njobs;
    FA.S = F.S;
    FA.s0 = F.s0;
    FA.G = G;
    if (fr.fog_walk) {  // BVH scans with pt_set_fog_walk: the same jobs, the closest hit and the shadow rays by the wave's walks of the tree
        const ptk::FogWalkArgs W{FA, F, d.bvh_nodes.p, d.bvh_objs.p, d.plane_idx.p, d.fog_walk_counters.p};
        return launch_pass(d, fr.adaptive, EV_FOG, F.njobs, ptk::fog_bvh_kernel, ptk::fog_bvh_adaptive_kernel, active, W);
    }
    return launch_pass(d, fr.adaptive, EV_FOG, F.njobs, ptk::fog_kernel, ptk::fog_adaptive_kernel, active, FA);
}

// The first-hit features of the chunk's samples with index below k into their running sums (pt_set_features)
int32_t step_features(pt_ctx *ctx, Device &d, const DevFrame &F, const ptk::AdaptTable &AT) {
    const Frame &fr = ctx->frame;
    ptk::FeatureArgs A;
    std::memset(&A, 0, sizeof A);
    A.objs = d.objs.p;
    A.mats = d.mats.p;
    A.ray = d.ray.p;
    A.ray_ndraw = d.ray_ndraw.p;
    A.feat = d.feat.p;
    A.ids = fr.object_ids ? d.obj_ids.p : nullptr;
    A.nobj = fr.nobj;
    A.first = F.s0 == 0 ? 1 : 0;
    A.nslots = d.nslots;
    A.njobs = F.njobs;
    A.S = F.S;
    A.take = std::min(F.S, (uint32_t)fr.features - F.s0);
    if (fr.feature_walk) {  // BVH scans with pt_set_feature_walk: the same slots, the first hit by the wave's walk of the tree
        const ptk::FeatureWalkArgs W{A, F, d.bvh_nodes.p, d.bvh_objs.p, d.plane_idx.p, d.walk_counters.p};
        return launch_pass(d, fr.adaptive, EV_FEATURE, live_slots(fr, d), ptk::feature_bvh_kernel, ptk::feature_bvh_adaptive_kernel, AT, W);
    }
    return launch_pass(d, fr.adaptive, EV_FEATURE, live_slots(fr, d), ptk::feature_kernel, ptk::feature_adaptive_kernel, AT, A);
}

// ... of a GL-shaded frame (pt_set_shading_features): the features of the camera rays the chunk's GL kernel made, made again from
// their streams (pt_gl_features.h); k counts passes
int32_t step_gl_features(pt_ctx *ctx, Device &d, const DevFrame &F, const TileGeom &G) {
    const Frame &fr = ctx->frame;
    ptk::GlFeatureArgs A;
    std::memset(&A, 0, sizeof A);
    gl_scene(fr, d, G, A.S);
    A.feat = d.feat.p;
    A.ids = fr.object_ids ? d.obj_ids.p : nullptr;
    A.key = ptm::seed_key(fr.cfg.seed ^ PTG_STREAM_SALT);
    A.nslots = d.nslots;
    A.s0 = F.s0;
    A.take = std::min(F.S, (uint32_t)fr.features - F.s0);
    A.first = F.s0 == 0 ? 1 : 0;
    A.ntx = G.ntx;
    A.shard_index = G.shard_index;
    A.shard_count = G.shard_count;
    const dim3 grid((d.nslots + PT_BLOCK - 1) / PT_BLOCK), block(PT_BLOCK);
    if (fr.gl_walk) {  // BVH scans: the closest hit by the lane's walk, its stack in LDS as gl_bvh_kernel's
        const ptk::GlFeatureWalkArgs W{A, F, d.bvh_nodes.p, d.bvh_objs.p, d.plane_idx.p};
        const size_t stack_bytes = (size_t)F.bvh_stack * PT_BLOCK * sizeof(int);
        return timed(d, EV_FEATURE, [&] { hipLaunchKernelGGL(ptk::gl_feature_bvh_kernel, grid, block, stack_bytes, d.stream, W); });
    }
    return timed(d, EV_FEATURE, [&] { hipLaunchKernelGGL(ptk::gl_feature_kernel, grid, block, 0, d.stream, A); });
}

// The chunk's radiance records into the running sums (resolve_kernel), then into the sums the frame opted into, each over the same
// records in the same order: their squares (pt_set_moments), the half-buffer sums (pt_set_halves)
int32_t step_accumulate(pt_ctx *ctx, Device &d, const DevFrame &F, const TileGeom &G, const ptk::AdaptTable &AT) {
    const Frame &fr = ctx->frame;
    const ptk::ChunkArgs C{d.L.p, d.nslots, F.S, d.acc_started ? 0 : 1, G};
    const uint32_t lanes = live_slots(fr, d);
    const bool st = fr.stats_on;
    const ptk::ResolveArgs R{C, st ? d.job_seg.p : nullptr, st ? d.job_draw.p : nullptr, d.acc.p, st ? d.acc_seg.p : nullptr, st ? d.acc_draw.p : nullptr};
    if (int32_t rc = launch_pass(d, fr.adaptive, EV_RESOLVE, lanes, ptk::resolve_kernel, ptk::resolve_adaptive_kernel, AT, R)) return rc;
    if (fr.moments)
        if (int32_t rc = launch_pass(d, fr.adaptive, EV_MOMENTS, lanes, ptk::moments_kernel, ptk::moments_adaptive_kernel, AT, ptk::MomentsArgs{C, d.m2.p}))
            return rc;
    if (fr.halves)
        if (int32_t rc = launch_pass(d, fr.adaptive, EV_HALVES, lanes, ptk::halves_kernel, ptk::halves_adaptive_kernel, AT, ptk::HalvesArgs{C, d.hv.p, F.s0}))
            return rc;
    d.acc_started = true;
    return PT_OK;
}

// Adds samples [s0, s0+S) to this device's running sums.
int32_t dev_step(pt_ctx *ctx, Device &d, uint32_t s0, uint32_t S) {
    Frame &fr = ctx->frame;
    if (d.nlocal == 0 || S == 0) return PT_OK;
    if (fr.adaptive && d.nact == 0) return PT_OK;  // every block of this device has stopped
    HIP_TRY(hipSetDevice(d.ordinal));
    DevFrame F = fr.F;
    F.shard_index = d.shard.index;
    F.shard_count = d.shard.count;
    F.nlocal = d.nlocal;
    F.s0 = s0;
    F.S = S;
    F.njobs = live_slots(fr, d) * S;  // adaptive: the active blocks' jobs only, compact
    const ptk::AdaptTable AT{d.act[d.act_cur].p, d.nact};
    const TileGeom G = tile_geom(fr, d);
    // jobs a wave claims per pop of the item cursor: 256, and 512 for the bitmask scans once a pass holds 128 samples per pixel
    // or more (same-box sweeps, profiles/r02_claim_sweep.txt: C4 at 265 spp per pass 664 / 653 / 654 / 659 / 673 ms for 256 / 512 /
    // 1024 / 2048 / 4096, at 79 spp per pass 677 / 675 / 678 ms; the BVH path loses 3 % at 512 and 7 % at 1024)
    const bool bvh_scan = fr.scan == ptk::SCAN_BVH || fr.scan == ptk::SCAN_VERIFY_BVH;
    F.claim = ctx->claim ? ctx->claim : (!bvh_scan && S >= 128u) ? 512u : 256u;
    unsigned int *qw = d.queue.p;
    TraceBuffers B;
    B.objs = d.objs.p;
    B.mats = d.mats.p;
    B.roulette = d.roulette.p;
    B.bsph = d.bsph.p;
    B.bbox = d.bbox.p;
    B.plane_idx = d.plane_idx.p;
    B.bvh_nodes = d.bvh_nodes.p;
    B.bvh_objs = d.bvh_objs.p;
    B.bvh_cores = d.bvh_cores.p;
    B.L = d.L.p;
    B.ray = d.ray.p;
    B.ray_rng = d.ray_rng.p;
    B.ray_ndraw = d.ray_ndraw.p;
    B.job_seg = fr.stats_on ? d.job_seg.p : nullptr;
    B.job_draw = fr.stats_on ? d.job_draw.p : nullptr;
    B.queue = qw;
    B.counters = d.counters.p;
    B.prof = ctx->profile_sections ? d.prof.p : nullptr;
    const bool timeline = !ctx->profile_sections && std::getenv("PTCORE_DEBUG_TIMELINE") != nullptr;  // diagnostics: when each wave of a trace launch retires
    if (timeline) {
        HIP_TRY(d.prof.reserve(65536));
        B.prof = d.prof.p;
    }
    B.cont_in = qw + 4;
    B.bsph_diel = d.bsph_diel.p;
    B.bbox_diel = d.bbox_diel.p;
    // the queues of the split passes and of the primary pass (step_trace sets where the continuation queue's entries are counted)
    std::memset(&B.glass, 0, sizeof B.glass);
    std::memset(&B.cont, 0, sizeof B.cont);
    if (fr.split_rounds > 0) B.glass = d.q_glass.bind(d.q_cap, fr.stats_on, nullptr);
    if (fr.split_rounds > 0 || fr.primary_pass) {
        B.cont = d.q_cont.bind(d.q_cap, fr.stats_on, nullptr);
        B.glass.count = qw + 1;
    }
    if (!d.first_recorded) {
        HIP_TRY(hipEventRecord(d.ev_first, d.stream));
        d.first_recorded = true;
    }
    if (fr.gl) {
        if (int32_t rc = step_gl(ctx, d, F, G)) return rc;
        if (fr.features > 0 && s0 < (uint32_t)fr.features)  // (only with pt_set_shading_features)
            if (int32_t rc = step_gl_features(ctx, d, F, G)) return rc;
    } else {  // ray generation, then the trace passes (which also handle max_depth <= 0: black samples, camera draws counted)
        HIP_TRY(hipMemsetAsync(qw, 0, 8 * sizeof(unsigned int), d.stream));
        if (int32_t rc = step_raygen(ctx, d, F, AT.active)) return rc;
        if (int32_t rc = fr.wavefront ? dev_step_wavefront(ctx, d, F, B) : step_trace(ctx, d, F, B, timeline)) return rc;
        if (fr.fog_vol)  // (GL shading adds the term itself)
            if (int32_t rc = step_fog(ctx, d, F, G, AT.active)) return rc;
        if (fr.features > 0 && s0 < (uint32_t)fr.features)  // (after the injected-ray overwrite: the rays that are traced)
            if (int32_t rc = step_features(ctx, d, F, AT)) return rc;
    }
    return step_accumulate(ctx, d, F, G, AT);
}

// The check that ends a pt_step of an adaptive frame, on one device: block_noise_kernel (counts, noise, decision per active block),
// then compact_kernel into the other list buffer.  The result word is read by the caller once the stream has drained.
int32_t dev_adaptive_check(pt_ctx *ctx, Device &d, ptk::AdaptResult *host_res) {
    const Frame &fr = ctx->frame;
    if (d.nlocal == 0 || d.nact == 0) return PT_OK;
    HIP_TRY(hipSetDevice(d.ordinal));
    ptk::BlockNoiseArgs A;
    std::memset(&A, 0, sizeof A);
    A.acc = d.acc.p;
    A.m2 = d.m2.p;
    A.active = d.act[d.act_cur].p;
    A.blk_spp = d.blk_spp.p;
    A.keep = d.blk_keep.p;
    A.noise = d.blk_noise.p;
    A.target = fr.ad.target;
    A.nslots = d.nslots;
    A.nact = d.nact;
    A.n = fr.done_spp;
    A.decide = fr.done_spp >= std::max(fr.ad.min_spp, 2) ? 1 : 0;
    A.G = tile_geom(fr, d);
    ptk::CompactArgs K;
    std::memset(&K, 0, sizeof K);
    K.active = d.act[d.act_cur].p;
    K.keep = d.blk_keep.p;
    K.noise = d.blk_noise.p;
    K.next = d.act[d.act_cur ^ 1].p;
    K.res = d.ad_res.p;
    K.nact = d.nact;
    if (int32_t rc = timed(d, EV_CHECK, [&] {  // the two as one
            hipLaunchKernelGGL(ptk::block_noise_kernel, dim3((d.nact * 64u + PT_BLOCK - 1) / PT_BLOCK), dim3(PT_BLOCK), 0, d.stream, A);
            hipLaunchKernelGGL(ptk::compact_kernel, dim3(1), dim3(PT_COMPACT_BLOCK), 0, d.stream, K);
        }))
        return rc;
    HIP_TRY(hipMemcpyAsync(host_res, d.ad_res.p, sizeof *host_res, hipMemcpyDeviceToHost, d.stream));
    return PT_OK;
}

// Writes the current estimate of this device's tiles (normalised by spp_done; in an adaptive frame every pixel by the count of its own block).
int32_t dev_finish(pt_ctx *ctx, Device &d, int32_t spp_done, uint8_t *tiles_rgba, double *tiles_accum,
                   uint32_t *tiles_seg, uint32_t *tiles_draw) {
    Frame &fr = ctx->frame;
    if (d.nlocal == 0) return PT_OK;
    HIP_TRY(hipSetDevice(d.ordinal));
    ptk::FinishArgs A;
    std::memset(&A, 0, sizeof A);
    A.acc = d.acc.p;
    A.acc_seg = d.acc_seg.p;
    A.acc_draw = d.acc_draw.p;
    A.blk_spp = fr.adaptive ? d.blk_spp.p : nullptr;
    A.tiles_rgba = tiles_rgba;
    A.tiles_accum = tiles_accum;
    A.tiles_seg = fr.stats_on ? tiles_seg : nullptr;
    A.tiles_draw = fr.stats_on ? tiles_draw : nullptr;
    A.nslots = d.nslots;
    A.zero = d.acc_started ? 0 : 1;
    A.inv_samples = 1.0 / (double)spp_done;  // renderer.go:97
    A.gl_spp = fr.gl ? std::max(1, spp_done) : 0;  // GL shading: tone-mapped finish of accum / passes
    A.G = tile_geom(fr, d);
    if (int32_t rc = timed(d, EV_RESOLVE, [&] {
            hipLaunchKernelGGL(ptk::finish_kernel, dim3((d.nslots + PT_BLOCK - 1) / PT_BLOCK), dim3(PT_BLOCK), 0, d.stream, A);
        }))
        return rc;
    HIP_TRY(hipEventRecord(d.ev_last, d.stream));
    return PT_OK;
}

int32_t dev_collect(Device &d, pt_stats *st, int slot) {
    HIP_TRY(hipSetDevice(d.ordinal));
    HIP_TRY(hipStreamSynchronize(d.stream));
    if (d.nlocal == 0) return PT_OK;
    unsigned long long c[48] = {};
    HIP_TRY(hipMemcpy(c, d.counters.p, sizeof c, hipMemcpyDeviceToHost));
    if (std::getenv("PTCORE_WALK_STATS") && c[24 + 2])
        std::fprintf(stderr, "ptcore walk32: rays walked %llu (+%llu missing the scene cube, %llu handed over before the walk, %llu of them far AND through the cube, widest inflation %llu margins), "
                             "node visits %llu, core visits %llu, wave iterations %llu (%.1f lanes per iteration), refills %llu, candidates %llu, handed over for > %d candidates %llu, for stack depth %llu\n",
                     c[24 + 8], c[24 + 9], c[24 + 5], c[24 + 10], c[24 + 11], c[24 + 0], c[24 + 1], c[24 + 2], (double)(c[24] + c[25]) / (double)c[24 + 2], c[24 + 3], c[24 + 4], PT_CAND_MAX,
                     c[24 + 6], c[24 + 7]);
    if (c[19]) return fail(PT_ERR_STATE, "internal: a path-state queue overflowed (" + std::to_string(c[19]) + " paths lost); the frame is invalid");
    g_mismatches += c[4];
    if ((c[20] || c[21] || c[23]) && std::getenv("PTCORE_VERBOSE"))
        std::fprintf(stderr, "ptcore: BVH path: %llu wave-trips through the plain every-object scan (rays with non-finite or absurd components), "
                             "%llu through the careful traversal (far-away rays), %llu lane-trips with bounds the FP32 tests were not analysed for, "
                             "%llu rays scanned by a whole wave (bounds as wide as the scene)\n", c[20], c[21], c[22], c[23]);
    if (c[4]) std::memcpy(g_mismatch_sample, c + 8, sizeof g_mismatch_sample);
    st->segments += c[0];
    st->exit_scans += c[1];
    st->draws += c[2];
    st->samples += c[3];
    if (c[47]) st->shader_clock_mhz = (double)c[46] / ((double)c[47] / 100.0);  // cycles / (ticks of the 100 MHz counter) = MHz (device 0 of the last collected)
    st->glass_events += c[5];
    st->continuations += c[6];
    st->split_cont_in += c[7];
    st->split_finished += c[18];
    if (d.prof.p && slot == 0)
        HIP_TRY(hipMemcpy(g_profile_scratch, d.prof.p, sizeof g_profile_scratch, hipMemcpyDeviceToHost));
    double tr = 0, rs = 0, trs = 0, gl = 0, rg = 0;
    const size_t n_trace = d.ev[EV_TRACE].n;
    if (int32_t rc = sum_ms(d.ev[EV_TRACE], tr, &d.trace_is_split, &trs)) return rc;
    if (int32_t rc = sum_ms(d.ev[EV_GLASS], gl)) return rc;
    if (int32_t rc = sum_ms(d.ev[EV_RESOLVE], rs)) return rc;
    if (int32_t rc = sum_ms(d.ev[EV_RAYGEN], rg)) return rc;
    st->glass_ms = std::max(st->glass_ms, gl);
    st->trace_split_ms = std::max(st->trace_split_ms, trs);
    st->glass_launches += (int32_t)d.ev[EV_GLASS].n;
    for (size_t i = 0; i < n_trace && i < d.trace_is_split.size(); i++) st->trace_split_launches += d.trace_is_split[i] ? 1 : 0;
    st->raygen_ms = std::max(st->raygen_ms, rg);
    float span = 0;
    if (d.first_recorded) HIP_TRY(hipEventElapsedTime(&span, d.ev_first, d.ev_last));
    st->trace_ms = std::max(st->trace_ms, tr);
    st->resolve_ms = std::max(st->resolve_ms, rs);
    st->device_ms = std::max(st->device_ms, (double)span);
    st->trace_launches += (int32_t)n_trace;
    st->resolve_launches += (int32_t)d.ev[EV_RESOLVE].n;
    if (slot < 8) st->per_device_ms[slot] = span;
    return PT_OK;
}

// pt_set_bvh_build(ctx, 1): both trees of world `w` built on devices[0] by the launch sequence of pt_bvh_build.h, on a stream of
// their own, and read back into T (nodes with their payload bytes, records, level table; depth and stack_need from the nodes, on
// the host).  ms = {the device time between the first and the last launch; the host's wall time of the allocations and the world's
// upload in front of it; of the readback behind it, from the last launch's end}.  The world is uploaded for the build alone:
// dev_begin uploads what it always did afterwards.
struct DeviceBuildHold {
    hipStream_t stream = nullptr;
    hipEvent_t a = nullptr, b = nullptr;
    void *world = nullptr, *nodes = nullptr, *order = nullptr, *objs = nullptr;
    ~DeviceBuildHold() {
        for (void *p : {world, nodes, order, objs})
            if (p) (void)hipFree(p);
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
        if (stream) (void)hipStreamDestroy(stream);
    }
};
int32_t device_build_trees(pt_ctx *ctx, const std::vector<DevObj> &w, ptbvh::SceneTrees &T, double ms[3]) {
    T = ptbvh::SceneTrees();
    ms[0] = ms[1] = ms[2] = 0.0;
    const auto wall = [](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    std::vector<int32_t> finite, glass;
    ptbvh::scene_object_lists(w, finite, glass);
    T.margin = ptbvh::scene_margin(w);
    const int32_t nf = (int32_t)finite.size(), ng = (int32_t)glass.size();
    if (nf == 0) return PT_OK;
    HIP_TRY(hipSetDevice(ctx->devs[0].ordinal));
    const auto t_up = std::chrono::steady_clock::now();
    DeviceBuildHold H;
    HIP_TRY(hipStreamCreate(&H.stream));
    HIP_TRY(hipEventCreate(&H.a));
    HIP_TRY(hipEventCreate(&H.b));
    const size_t room = (size_t)nf + (size_t)ng;  // (a tree of n objects has at most n nodes)
    HIP_TRY(hipMalloc(&H.world, w.size() * sizeof(DevObj)));
    HIP_TRY(hipMalloc(&H.nodes, room * sizeof(BvhNode)));
    HIP_TRY(hipMalloc(&H.order, room * sizeof(int32_t)));
    HIP_TRY(hipMalloc(&H.objs, room * sizeof(BvhObj)));
    HIP_TRY(hipMemcpyAsync(H.world, w.data(), w.size() * sizeof(DevObj), hipMemcpyHostToDevice, H.stream));
    HIP_TRY(hipStreamSynchronize(H.stream));
    ms[1] = wall(t_up);
    HIP_TRY(hipEventRecord(H.a, H.stream));
    std::vector<int32_t> levels_main, levels_glass;
    ptbb::Scratch S;
    BvhNode *nodes = static_cast<BvhNode *>(H.nodes);
    int32_t *order = static_cast<int32_t *>(H.order);
    const DevObj *objs = static_cast<const DevObj *>(H.world);
    HIP_TRY(ptbb::build_tree_launch(H.stream, S, objs, finite.data(), nf, T.margin, nodes, order, 0, 0, levels_main));
    const int32_t main_nodes = levels_main.empty() ? 0 : levels_main.back();
    HIP_TRY(ptbb::build_tree_launch(H.stream, S, objs, glass.data(), ng, T.margin, nodes, order, main_nodes, nf, levels_glass));
    const int32_t n_nodes = main_nodes + (levels_glass.empty() ? 0 : levels_glass.back());
    ptbb::objs_launch(H.stream, static_cast<BvhObj *>(H.objs), order, objs, nf + ng);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(H.b, H.stream));
    HIP_TRY(hipStreamSynchronize(H.stream));
    const auto t_back = std::chrono::steady_clock::now();
    T.nodes.resize((size_t)n_nodes);
    T.objs.resize(room);
    HIP_TRY(hipMemcpyAsync(T.nodes.data(), H.nodes, T.nodes.size() * sizeof(BvhNode), hipMemcpyDeviceToHost, H.stream));
    HIP_TRY(hipMemcpyAsync(T.objs.data(), H.objs, T.objs.size() * sizeof(BvhObj), hipMemcpyDeviceToHost, H.stream));
    HIP_TRY(hipStreamSynchronize(H.stream));
    ms[2] = wall(t_back);
    float fms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&fms, H.a, H.b));
    ms[0] = fms;
    (void)ptbvh::finish_lbvh_trees(T, main_nodes, nf, levels_main, levels_glass, PT_BVH_STACK);
    return PT_OK;
}

// (Re)builds ctx->sd when the scene or the requested scan strategy changed.
int32_t scene_prepare(pt_ctx *ctx, const pt_scene *scene) {
    SceneData &sd = ctx->sd;
    pt_ctx::Refit &rf = ctx->rf;
    const auto prepare_t0 = std::chrono::steady_clock::now();  // (pt_bvh_build_stats.prepare_ms: the conversion and the comparisons count)
    const bool refit_on = rf.max_growth >= 1.0;
    rf.st.last_action = 0;
    // pt_set_bvh_refit: the tree in use is a refitted one that has degraded past the bound (its figure is known since the last
    // dev_begin): this preparation rebuilds, also for an unchanged scene -- a degraded tree serves one frame at the most
    const bool outgrown = refit_on && sd.valid && sd.tree_moved && !rf.figure_pending && rf.st.cost_now > rf.max_growth * rf.st.cost_built;
    // fast path for a scene that has not changed since the last frame (progressive previews, benchmark loops): compare the
    // caller's arrays with the copy kept from then; converting a 10^6-object world just to find it unchanged cost 25 ms a frame
    {
        const size_t nm = (size_t)std::max(0, scene->num_materials), no = (size_t)std::max(0, scene->num_objects);
        const bool raw_same = sd.valid && sd.scan_req == ctx->scan_mode && sd.raw_mats.size() == nm && sd.raw_objs.size() == no &&
                              (nm == 0 || std::memcmp(sd.raw_mats.data(), scene->materials, nm * sizeof(pt_material)) == 0) &&
                              (no == 0 || std::memcmp(sd.raw_objs.data(), scene->objects, no * sizeof(pt_object)) == 0);
        if (raw_same && !outgrown) return PT_OK;
        sd.raw_mats.assign(scene->materials, scene->materials + nm);
        sd.raw_objs.assign(scene->objects, scene->objects + no);
    }
    std::vector<DevObj> world;
    std::vector<DevMat> mats;
    scene_to_world(*scene, world, mats);
    const bool same = sd.valid && sd.scan_req == ctx->scan_mode && world.size() == sd.world.size() &&
                      mats.size() == sd.mats.size() &&
                      (world.empty() || std::memcmp(world.data(), sd.world.data(), world.size() * sizeof(DevObj)) == 0) &&
                      std::memcmp(mats.data(), sd.mats.data(), mats.size() * sizeof(DevMat)) == 0;
    if (same && !outgrown) return PT_OK;
    // Why this preparation builds in full; REFIT_OK: only positions and sizes changed and the devices refit the tree they hold.
    int reason = ptbvh::REFIT_OK;
    if (!sd.valid) reason = ptbvh::REFIT_FIRST;
    else if (!refit_on) reason = ptbvh::REFIT_OFF;
    else if (outgrown) reason = ptbvh::REFIT_GROWTH;
    else if (!(sd.scan == ptk::SCAN_BVH || sd.scan == ptk::SCAN_VERIFY_BVH) || sd.scan_req != ctx->scan_mode || ctx->pipeline == 2)
        // (the walk32 core twins are not refitted; a world kept off the hierarchy by the 1e37 rule says so, whatever the last one was)
        reason = ptbvh::world_beyond_fp32(world) ? ptbvh::REFIT_NONFINITE : ptbvh::REFIT_NOT_BVH;
    else reason = ptbvh::refit_reason(sd.world, sd.mats, world, mats);
    if (reason == ptbvh::REFIT_OK) {
        // Same objects by kind and material, all finite: the scan, the counts, the depth, the stack and the LDS plan stay.  The
        // broad-phase fields and the margin follow the move; bvh_nodes / bvh_objs stay those of the last full build, the topology
        // the devices refit from.
        if (!sd.tree_moved && !(rf.st.cost_built > 0.0)) {  // built while the feature was off: the figure of the tree as built, late
            std::vector<double> box, area;
            ptbvh::refit(sd.bvh_nodes, sd.bvh_objs, sd.world, sd.bvh_margin, sd.bvh_levels, box, area);  // (to its own world: no byte changes)
            rf.st.cost_built = ptrf::cost_of(area.data(), (size_t)sd.Fs.bvh_main_nodes);
        }
        sd.world = std::move(world);
        build_broad(sd.world, sd);
        sd.bvh_margin = ptbvh::scene_margin(sd.world);
        sd.tree_moved = true;
        sd.gen++;
        rf.figure_pending = true;
        rf.st.refits++;
        rf.st.last_action = 2;
        return PT_OK;
    }
    rf.st.builds++;
    rf.st.last_action = 1;
    rf.st.last_build_reason = reason;
    rf.st.cost_built = rf.st.cost_now = 0.0;
    rf.figure_pending = false;
    pt_ctx::Build &bb = ctx->bb;
    bb.st.builder = PT_BVH_BUILDER_NONE;
    bb.st.last_fallback = PT_BVH_BUILD_FALLBACK_NONE;
    bb.st.nodes = bb.st.depth = bb.st.stack_need = 0;
    bb.st.cost = 0.0;
    sd.tree_moved = false;
    sd.valid = false;
    sd.world = std::move(world);
    sd.mats = std::move(mats);
    roulette_table(sd.mats, sd.roulette);  // (a refit keeps mats -- refit_reason asks for the same bytes -- and so the table)
    sd.scan_req = ctx->scan_mode;
    DevFrame &F = sd.Fs;
    std::memset(&F, 0, sizeof F);
    F.nobj = (int32_t)sd.world.size();
    F.nmat = (int32_t)sd.mats.size();
    build_broad(sd.world, sd);
    // closest-hit strategy: at most 32 spheres and 32 boxes -> candidate bitmasks; at most 128 of each -> the same in
    // groups of 32; more -> BVH.  PTCORE_SCAN overrides.
    int scan = ctx->scan_mode;
    // the LDS copy of the world (objects + materials + record indices) and the roulette table behind it must leave room for five blocks per CU
    const size_t world_lds = RouletteLds::behind(LdsLayout::trace(sd.world.size(), sd.mats.size(), sd.bsph.size(), sd.bbox.size(), sd.bsph_diel.size(), sd.bbox_diel.size(), false), sd.mats.size()).total;
    const bool wide_ok = F.broad_ok == 2 && world_lds <= 30 * 1024;
    if (scan < 0) scan = F.broad_ok == 1 ? ptk::SCAN_BROAD : wide_ok ? ptk::SCAN_BROAD_WIDE : ptk::SCAN_BVH;
    if ((scan == ptk::SCAN_BROAD || scan == ptk::SCAN_VERIFY) && F.broad_ok != 1) {
        const bool verify = scan == ptk::SCAN_VERIFY;
        scan = wide_ok ? (verify ? ptk::SCAN_VERIFY_WIDE : ptk::SCAN_BROAD_WIDE) : (verify ? ptk::SCAN_VERIFY_BVH : ptk::SCAN_BVH);
    }
    if ((scan == ptk::SCAN_BROAD_WIDE || scan == ptk::SCAN_VERIFY_WIDE) && !wide_ok && F.broad_ok != 1)
        scan = scan == ptk::SCAN_VERIFY_WIDE ? ptk::SCAN_VERIFY_BVH : ptk::SCAN_BVH;
    // A NaN or an infinity in the geometry (reachable through the C ABI, not through the JSON loader) makes the reference's own
    // tests return NaN parameters, which its range tests accept (NaN compares false, objects.go:56-60, :110) and which then
    // poison `closest` for every later object of the loop.  Only the loop itself reproduces that: such a world takes the
    // plain object-by-object scan, whatever was asked for.
    // The same for coordinates or sizes of 1e37 and more: every culled strategy keeps FP32 bounds of the objects, which must stay
    // finite UPPER bounds (the hierarchy rounds its half extents up to a multiple of 256 ulp and has no room to do so within a
    // factor 34 of FLT_MAX).
    for (const DevObj &o : sd.world) {
        bool fin = std::fabs(o.radius) < 1e37;
        for (int k = 0; k < 3; k++) fin = fin && std::fabs(o.a[k]) < 1e37 && std::fabs(o.b[k]) < 1e37;
        if (!fin) scan = ptk::SCAN_UNIFORM;
    }
    sd.scan = scan;
    const bool big = scan == ptk::SCAN_BVH || scan == ptk::SCAN_VERIFY_BVH;
    sd.bvh_nodes.clear();
    sd.bvh_objs.clear();
    sd.bvh_cores.clear();
    sd.bvh_levels.clear();
    F.bvh_root = F.bvh_root_exit = -1;
    const std::vector<DevObj> &w = sd.world;
    if (big) {
        // Only PTCORE_PIPELINE=walk32 reads the core twins (and the bits 20-23 build_cores sets in the nodes' meta): the default loop
        // neither builds nor uploads 128 B per node for nothing.
        ptbvh::SceneTrees T;
        // pt_set_bvh_build(ctx, 1): the Morton-order build on devices[0] (pt_bvh_build.h), read back; everything below and every
        // device take it as they take the host builder's.  A tree too deep for the stack and walk32 (no core twins) build on the host.
        bool on_device = false;
        if (bb.mode == 1) {
            if (ctx->pipeline == 2) {
                bb.st.last_fallback = PT_BVH_BUILD_FALLBACK_WALK32;
            } else {
                double ms[3];
                if (int32_t rc = device_build_trees(ctx, w, T, ms)) return rc;
                bb.st.device_ms = ms[0];
                bb.st.upload_ms = ms[1];
                bb.st.readback_ms = ms[2];
                on_device = T.stack_need < PT_BVH_STACK;
                if (!on_device) bb.st.last_fallback = PT_BVH_BUILD_FALLBACK_STACK;
            }
        }
        if (!on_device) {
            if (!ptbvh::build_scene_trees(w, ctx->pipeline == 2, PT_BVH_STACK, T)) {
                sd.bvh_depth = T.depth;
                sd.bvh_stack_need = T.stack_need;
                return fail(PT_ERR_INVALID, "BVH deeper than the traversal stack");
            }
        }
        sd.bvh_depth = T.depth;
        sd.bvh_stack_need = T.stack_need;
        if (on_device) bb.st.device_builds++;
        else bb.st.host_builds++;
        bb.st.builder = on_device ? PT_BVH_BUILDER_DEVICE : PT_BVH_BUILDER_HOST;
        bb.st.nodes = (int32_t)T.nodes.size();
        bb.st.depth = T.depth;
        bb.st.stack_need = T.stack_need;
        if (refit_on || bb.mode == 1) {  // the figure later refits are held against: a refit to the world it was built from changes no byte
            std::vector<double> box, area;
            ptbvh::refit(T.nodes, T.objs, w, T.margin, T.level_start, box, area);
            bb.st.cost = ptrf::cost_of(area.data(), (size_t)T.main_nodes);
            if (refit_on) rf.st.cost_built = rf.st.cost_now = bb.st.cost;
        }
        F.bvh_main_nodes = T.main_nodes;
        sd.bvh_nodes = std::move(T.nodes);
        sd.bvh_objs = std::move(T.objs);
        sd.bvh_cores = std::move(T.cores);
        sd.bvh_levels = std::move(T.level_start);
        sd.bvh_margin = T.margin;
        F.bvh_root_exit = T.root_exit;
        F.bvh_root = T.root;
    } else if (bb.mode == 1) {
        bb.st.last_fallback = PT_BVH_BUILD_FALLBACK_NOT_BVH;  // (no tree at all)
    }
    F.n_bvh_nodes = (int32_t)sd.bvh_nodes.size();
    F.n_bvh_objs = (int32_t)sd.bvh_objs.size();
    F.world_in_lds = big ? 0 : 1;
    // LDS plan of the BVH path: per-lane stacks sized by the tree depth, and the first (top-level)
    // nodes of the main tree in what is left of a 40 KiB budget (4 blocks of 256 threads per CU)
    F.bvh_stack = big ? std::max(4, ((sd.bvh_stack_need + 1 + 3) / 4) * 4) : 0;
    const size_t stack_bytes = (size_t)F.bvh_stack * PT_BLOCK * sizeof(int);
    F.bvh_lds_nodes = 0;
    F.bvh_min_lanes = 24;
    F.debug_drop = 0;  // PTCORE_DEBUG_DROP=<mask>: the verify instantiations of the bitmask scans lose these candidate bits
    if (const char *e = std::getenv("PTCORE_DEBUG_DROP")) F.debug_drop = (uint32_t)std::strtoul(e, nullptr, 0);
    if (const char *e = std::getenv("PTCORE_BVH_MIN_LANES")) F.bvh_min_lanes = std::max(0, std::min(64, std::atoi(e)));
    F.bvh_leaf_single = 1;
    if (const char *e = std::getenv("PTCORE_BVH_LEAF_SINGLE")) F.bvh_leaf_single = std::atoi(e) != 0;
    F.bvh_node_min = 16;
    if (const char *e = std::getenv("PTCORE_BVH_NODE_MIN")) F.bvh_node_min = std::max(0, std::min(65, std::atoi(e)));
    size_t lds_budget = (size_t)(160 * 1024 / PT_BVH_WAVES);
    if (const char *e = std::getenv("PTCORE_BVH_LDS_BUDGET")) lds_budget = (size_t)std::max(0, std::min(160 * 1024, std::atoi(e)));
    if (big && F.bvh_root == 0 && stack_bytes < lds_budget)
        F.bvh_lds_nodes = (int32_t)std::min<size_t>((lds_budget - stack_bytes) / sizeof(BvhNode), (size_t)F.bvh_main_nodes);
    // single-group scans keep the records' objects a second time, in record order (LdsLayout, pt_device.h); glass_kernel the dielectric ones
    const bool rec_order = scan == ptk::SCAN_BROAD || scan == ptk::SCAN_VERIFY;
    sd.lds_bytes = big ? stack_bytes + (size_t)F.bvh_lds_nodes * sizeof(BvhNode)
                       : RouletteLds::behind(LdsLayout::trace((size_t)F.nobj, (size_t)F.nmat, sd.bsph.size(), sd.bbox.size(), sd.bsph_diel.size(), sd.bbox_diel.size(), rec_order), (size_t)F.nmat).total;
    sd.glass_lds_bytes = RouletteLds::behind(LdsLayout::glass((size_t)F.nobj, (size_t)F.nmat, sd.bsph_diel.size(), sd.bbox_diel.size(), rec_order), (size_t)F.nmat).total;
    // PTCORE_BVH_LDS_PAD=<bytes>: unused LDS on top of the BVH plan (occupancy experiments: 4 blocks per CU fit 40 KiB each)
    if (const char *e = std::getenv("PTCORE_BVH_LDS_PAD"))
        if (big) sd.lds_bytes += (size_t)std::max(0, std::min(120 * 1024, std::atoi(e)));
    if (big && std::getenv("PTCORE_VERBOSE"))
        std::fprintf(stderr, "ptcore: BVH %d nodes (%d wide levels), %d objects, stack %d entries per lane, %d nodes in LDS, %zu B of LDS per block\n",
                     F.n_bvh_nodes, sd.bvh_depth, F.n_bvh_objs, F.bvh_stack, F.bvh_lds_nodes, sd.lds_bytes);
    if (sd.lds_bytes > 160 * 1024)
        return fail(PT_ERR_INVALID, "scene does not fit the 160 KiB LDS of a CU with this scan strategy (use the BVH: unset PTCORE_SCAN)");
    sd.has_glass = false;
    for (const DevObj &o : sd.world) sd.has_glass = sd.has_glass || (o.kind & 0x100);
    sd.gen++;
    sd.topo_gen = sd.gen;
    sd.valid = true;
    bb.st.prepare_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - prepare_t0).count();
    return PT_OK;
}

// pt_set_shading_walk: ptg::walk_scene_check on the tree the devices hold (a moved world's, pt_set_bvh_refit: the host's restatement
// of their refit), cached with the scene's generation.
int32_t gl_walk_check(pt_ctx *ctx, const pt_scene *scene, const std::vector<ptg::GlObj> &gl_objs) {
    SceneData &sd = ctx->sd;
    if (sd.gl_walk_gen != sd.gen) {
        const std::vector<BvhNode> *nodes = &sd.bvh_nodes;
        std::vector<BvhNode> moved_nodes;
        if (sd.tree_moved && !sd.bvh_nodes.empty()) {
            moved_nodes = sd.bvh_nodes;
            std::vector<BvhObj> moved_objs = sd.bvh_objs;
            std::vector<double> box, area;
            ptbvh::refit(moved_nodes, moved_objs, sd.world, sd.bvh_margin, sd.bvh_levels, box, area);
            nodes = &moved_nodes;
        }
        int32_t main_objs = 0;  // the main tree's records come first
        for (int32_t q = 0; q < sd.Fs.bvh_main_nodes; q++)
            for (int s = 0; s < 4; s++)
                if (((*nodes)[(size_t)q].meta >> (12 + s)) & 1u) main_objs++;
        sd.gl_walk_why.clear();
        sd.gl_walk_ok = ptg::walk_scene_check(scene->objects, scene->num_objects, gl_objs.data(), nodes->data(), sd.Fs.bvh_main_nodes, sd.bvh_objs.data(),
                                              main_objs, sd.plane_idx.data(), (int32_t)sd.plane_idx.size(), sd.gl_walk_why);
        sd.gl_walk_gen = sd.gen;
    }
    if (!sd.gl_walk_ok) return fail(PT_ERR_INVALID, "GL shading on the BVH path (pt_set_shading_walk): " + sd.gl_walk_why);
    return PT_OK;
}

int32_t frame_open(pt_ctx *ctx, const pt_scene *scene, const pt_config *cfg, uint32_t max_slots) {
    if (int32_t rc = scene_prepare(ctx, scene)) return rc;
    const SceneData &sd = ctx->sd;
    Frame &fr = ctx->frame;
    if (!ctx->inject_rays.empty()) {  // pt_debug_set_primary_rays: refuse what the table does not cover before anything is launched
        if (ctx->fog_on) return fail(PT_ERR_STATE, "injected primary rays: not available with fog on (pt_set_fog)");
        if (ctx->shading_model != PT_SHADING_CPU) return fail(PT_ERR_STATE, "injected primary rays: not available with GL shading (pt_set_shading)");
        if (ctx->devs.size() != 1) return fail(PT_ERR_STATE, "injected primary rays: not available on a context with several devices");
        const uint64_t want = (uint64_t)cfg->width * (uint64_t)cfg->height * (uint64_t)std::max(0, cfg->samples_per_px);
        if (want != ctx->inject_rays.size() / 6)
            return fail(PT_ERR_INVALID, "injected primary rays: the table holds " + std::to_string(ctx->inject_rays.size() / 6) + " rays, the frame needs width*height*samples_per_px = " +
                                            std::to_string(want));
    }
    fr = Frame();
    fr.cfg = *cfg;
    std::memset(&ctx->fog_last, 0, sizeof ctx->fog_last);
    ctx->fog_pending = 0;
    std::memset(&ctx->shading_last, 0, sizeof ctx->shading_last);
    ctx->shading_pending = 0;
    fr.nobj = sd.Fs.nobj;
    fr.nmat = sd.Fs.nmat;
    fr.scan = sd.scan;
    fr.lds_bytes = sd.lds_bytes;
    fr.glass_lds_bytes = sd.glass_lds_bytes;
    fr.has_glass = sd.has_glass;
    // split passes: the bitmask scan of reference-sized scenes; a path has at most max_depth dielectric bounces
    fr.split_rounds = 0;
    if ((sd.scan == ptk::SCAN_BROAD || sd.scan == ptk::SCAN_VERIFY || sd.scan == ptk::SCAN_BROAD_WIDE || sd.scan == ptk::SCAN_VERIFY_WIDE) &&
        cfg->max_depth > 0)
        fr.split_rounds = fr.has_glass ? std::max(0, std::min(ctx->split_rounds, cfg->max_depth)) : (ctx->split_rounds > 0 ? 1 : 0);
    {
        const bool bitmask = sd.scan == ptk::SCAN_BROAD || sd.scan == ptk::SCAN_VERIFY || sd.scan == ptk::SCAN_BROAD_WIDE || sd.scan == ptk::SCAN_VERIFY_WIDE;
        fr.tail_form = (bitmask && fr.has_glass && ctx->tail_nested && !ctx->profile_sections) ? ptk::FORM_NESTED : ptk::FORM_ALL_IN_ONE;
    }
    {  // the wavefront form: on request (PTCORE_PIPELINE=wavefront), for the scans that have a pass form (bitmask, BVH).
       // Measured slower than the all-in-one loop in every regime, so it is the A/B, not the default.
        const bool bvh = sd.scan == ptk::SCAN_BVH || sd.scan == ptk::SCAN_VERIFY_BVH;
        const bool flat = sd.scan == ptk::SCAN_BROAD || sd.scan == ptk::SCAN_VERIFY;
        fr.wavefront = !ctx->profile_sections && ((ctx->pipeline == 1 && (bvh || flat)) || (ctx->pipeline == 2 && bvh));
        fr.walk32 = fr.wavefront && ctx->pipeline == 2;
        if (fr.wavefront) { fr.split_rounds = 0; fr.tail_form = ptk::FORM_ALL_IN_ONE; }
        fr.primary_pass = bvh && !fr.wavefront && !ctx->profile_sections && ctx->primary_coop && sd.Fs.bvh_root >= 0;
        fr.shade_lds_bytes = (size_t)sd.Fs.nmat * sizeof(DevMat) + (sd.Fs.world_in_lds ? (size_t)sd.Fs.nobj * sizeof(DevObj) : 0);
    }
    fr.cam = new_camera(scene->camera, cfg->width, cfg->height);
    {
        pt_sky sky = scene->sky;
        if (ctx->fog_on) {
            fr.fog = ptf::fog_resolve(ctx->fog_raw);
            const bool bvh = sd.scan == ptk::SCAN_BVH || sd.scan == ptk::SCAN_VERIFY_BVH;
            const bool gl = ctx->shading_model == PT_SHADING_GL;
            if (bvh && ctx->fog_walk_on && gl && !ctx->shading_walk_on)  // stays refused, and refused first
                return fail(PT_ERR_INVALID, "GL shading is not available for scenes on the BVH path (more than 128 spheres or 128 boxes)");
            if (fr.fog.volumetric && bvh && gl && ctx->shading_walk_on)  // (fog_march's shadow tests are still the loop over all objects)
                return fail(PT_ERR_INVALID, "fog: gpu_volumetric is not available with GL shading on the BVH path (pt_set_shading_walk); "
                                            "affect_sky alone is");
            if (fr.fog.volumetric && bvh && !ctx->fog_walk_on)
                return fail(PT_ERR_INVALID, "fog: gpu_volumetric is not available for scenes on the BVH path (more than 128 spheres or "
                                            "128 boxes); affect_sky alone is");
            if (ptf::fog_sky_applies(fr.fog))  // applyFog(bg, 50), gpu.go:1392-1393, as a rewrite of the sky constants
                for (double *c : {sky.background, sky.color, sky.horizon, sky.zenith}) ptf::fog_sky_rewrite(fr.fog, c);
            fr.fog_vol = ptf::fog_volumetric(fr.fog, cfg->max_depth);
            fr.fog_walk = fr.fog_vol && bvh;  // (only with pt_set_fog_walk; the other scans ignore the setting)
            if (fr.fog_vol)  // the emissive spheres, in object order
                for (int32_t i = 0; i < scene->num_objects; i++) {
                    ptf::FogLight l;
                    if (ptf::fog_light_of(*scene, i, l)) fr.fog_lights.push_back(l);
                }
        }
        fr.sky = make_sky(sky);
        if (ctx->shading_model == PT_SHADING_GL) {
            if (cfg->flags & PT_FLAG_PIXEL_STATS) return fail(PT_ERR_INVALID, "GL shading: PT_FLAG_PIXEL_STATS is not available");
            const bool bvh = sd.scan == ptk::SCAN_BVH || sd.scan == ptk::SCAN_VERIFY_BVH;
            if (bvh && !ctx->shading_walk_on)
                return fail(PT_ERR_INVALID, "GL shading is not available for scenes on the BVH path (more than 128 spheres or 128 boxes)");
            if ((int32_t)ctx->gl_extras.size() != scene->num_materials)
                return fail(PT_ERR_INVALID, "GL shading: " + std::to_string(ctx->gl_extras.size()) + " material entries for a scene with " +
                                                std::to_string(scene->num_materials) + " materials");
            fr.gl = true;
            fr.gl_filter = ctx->shading_features_on;
            const int32_t nmat = scene->num_materials;
            fr.gl_mats.assign((size_t)std::max(1, nmat), ptg::GlMat{});  // no materials: one zero material for every object
            for (int32_t i = 0; i < nmat; i++) fr.gl_mats[(size_t)i] = ptg::gl_material(scene->materials[i], ctx->gl_extras[(size_t)i]);
            for (int32_t i = 0; i < scene->num_objects; i++) {
                fr.gl_objs.push_back(ptg::gl_object(scene->objects[i], nmat));
                if (ptg::gl_is_light(*scene, i)) fr.gl_lights.push_back(i);
            }
            if (bvh) {  // pt_set_shading_walk: may the GL objects be found through the tree?  Asked once per scene generation.
                if (int32_t rc = gl_walk_check(ctx, scene, fr.gl_objs)) return rc;
                fr.gl_walk = true;
            }
            fr.gl_cam = ptg::gl_camera(scene->camera, cfg->width, cfg->height);
            fr.gl_sky = ptg::gl_sky(sky);
        }
    }
    fr.ntx = (cfg->width + 31) / 32;
    fr.nty = (cfg->height + 31) / 32;
    fr.stats_on = (cfg->flags & PT_FLAG_PIXEL_STATS) != 0;
    DevFrame &F = fr.F;
    F = sd.Fs;
    F.width = cfg->width;
    F.height = cfg->height;
    F.max_depth = cfg->max_depth;
    F.ntx = fr.ntx;
    F.nty = fr.nty;
    F.seed_key = ptm::seed_key(cfg->seed);
    F.inv_width = 1.0 / (double)(cfg->width - 1);
    F.inv_height = 1.0 / (double)(cfg->height - 1);
    F.height_m1 = (double)(cfg->height - 1);
    // chunk of samples per pass: bounded by the L budget and by 2^31 jobs
    uint32_t chunk = cfg->spp_chunk > 0 ? (uint32_t)cfg->spp_chunk : 0;
    const uint32_t slots = std::max(1u, max_slots);
    // per job: 32 B radiance record + 58 B primary ray, and with split passes two path-state queues of 100 B per entry.  A first guess,
    // coarser than the plan on purpose (no window slack, no pixel stats): dev_begin prices the pass from pass_plan() and shrinks it
    // where the guess was too large.
    const size_t job_bytes = 90 + (fr.wavefront ? 330 + (fr.walk32 ? 4 * (PT_CAND_MAX + 2) : 0) : fr.split_rounds > 0 && fr.has_glass ? 220 : fr.primary_pass ? 110 : 0);
    fr.budget_bytes = ctx->l_budget_bytes;
    if (ctx->auto_grow && ctx->grown_budget_bytes > fr.budget_bytes && !ctx->devs.empty()) {
        const bool same_shape = cfg->width == ctx->last_w && cfg->height == ctx->last_h && cfg->samples_per_px == ctx->last_spp;
        if (same_shape && !ctx->grown && (size_t)slots * job_bytes * (size_t)std::max(1, cfg->samples_per_px) > fr.budget_bytes) {
            // the second frame of this shape, and it takes more than one pass: is the room there?  (free memory + what this context
            // already holds must cover the grown size with a tenth to spare, on the first device -- the others are its twins)
            size_t free_b = 0, total_b = 0;
            if (hipSetDevice(ctx->devs[0].ordinal) == hipSuccess && hipMemGetInfo(&free_b, &total_b) == hipSuccess &&
                free_b + dev_held_bytes(ctx->devs[0]) >= ctx->grown_budget_bytes + ctx->grown_budget_bytes / 10)
                ctx->grown = true;
            (void)hipGetLastError();
        }
        if (ctx->grown && same_shape) fr.budget_bytes = ctx->grown_budget_bytes;
    }
    ctx->last_w = cfg->width; ctx->last_h = cfg->height; ctx->last_spp = cfg->samples_per_px;
    if (chunk == 0) chunk = (uint32_t)std::max<size_t>(1, fr.budget_bytes / ((size_t)slots * job_bytes));
    chunk = std::min<uint32_t>(chunk, (uint32_t)std::max(1, cfg->samples_per_px));
    chunk = std::min<uint32_t>(chunk, std::max(1u, 0x7fffffffu / slots));
    fr.chunk = chunk;
    if (cfg->spp_chunk <= 0) balance_chunk(fr);
    fr.done_spp = 0;
    fr.t0 = std::chrono::steady_clock::now();
    fr.serial = ++ctx->frames_opened;
    fr.open = true;
    return PT_OK;
}

// Reads the fog counters and fog_kernel times of the last frame into ctx->fog_last (waits for the devices' streams).
int32_t collect_fog(pt_ctx *ctx) {
    if (!ctx->fog_pending) return PT_OK;
    const bool first_only = ctx->fog_pending == 2;
    ctx->fog_pending = 0;
    pt_fog_stats fs;
    std::memset(&fs, 0, sizeof fs);
    for (size_t i = 0; i < ctx->devs.size() && !(first_only && i > 0); i++) {
        Device &d = ctx->devs[i];
        if (d.ev[EV_FOG].n == 0 && !(ctx->frame.gl && d.ev[EV_TRACE].n > 0)) continue;  // GL shading: the term ran inside gl_trace_kernel
        HIP_TRY(hipSetDevice(d.ordinal));
        HIP_TRY(hipStreamSynchronize(d.stream));
        unsigned long long c[3] = {};
        HIP_TRY(hipMemcpy(c, d.fog_counters.p, sizeof c, hipMemcpyDeviceToHost));
        fs.shadow_rays += c[0];
        fs.draws += c[1];
        fs.steps += c[2];
        double ms = 0;
        if (int32_t rc = sum_ms(d.ev[EV_FOG], ms)) return rc;
        fs.fog_ms = std::max(fs.fog_ms, ms);
        fs.fog_launches += (int32_t)d.ev[EV_FOG].n;
    }
    ctx->fog_last = fs;
    return PT_OK;
}

// Reads the GL counters and gl_trace_kernel times of the last frame into ctx->shading_last (waits for the devices' streams).
int32_t collect_shading(pt_ctx *ctx) {
    if (!ctx->shading_pending) return PT_OK;
    const bool first_only = ctx->shading_pending == 2;
    ctx->shading_pending = 0;
    pt_shading_stats ss;
    std::memset(&ss, 0, sizeof ss);
    for (size_t i = 0; i < ctx->devs.size() && !(first_only && i > 0); i++) {
        Device &d = ctx->devs[i];
        if (d.ev[EV_TRACE].n == 0 || !d.gl_counters.p) continue;
        HIP_TRY(hipSetDevice(d.ordinal));
        HIP_TRY(hipStreamSynchronize(d.stream));
        unsigned long long c[5] = {};
        HIP_TRY(hipMemcpy(c, d.gl_counters.p, sizeof c, hipMemcpyDeviceToHost));
        ss.paths += c[0];
        ss.segments += c[1];
        ss.shadow_rays += c[2];
        ss.probe_rays += c[3];
        ss.draws += c[4];
        double ms = 0;
        if (int32_t rc = sum_ms(d.ev[EV_TRACE], ms)) return rc;
        ss.gl_ms = std::max(ss.gl_ms, ms);
        ss.gl_launches += (int32_t)d.ev[EV_TRACE].n;
    }
    ctx->shading_last = ss;
    return PT_OK;
}

void fill_stats_common(pt_ctx *ctx, pt_stats *st) {
    Frame &fr = ctx->frame;
    st->spp_chunk = (int32_t)fr.chunk;
    st->num_devices = (int32_t)ctx->devs.size();
    st->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - fr.t0).count();
}

}  // namespace

// ==================================================================== C ABI

namespace {

// Loads librccl.so and makes one communicator per device of the context (one process, ncclCommInitAll).  RCCL refuses a
// device list that names one GPU twice -- the "virtual devices" of the tests -- and so does this.
int32_t rccl_open(pt_ctx *ctx) {
    pt_ctx::Rccl &R = ctx->rccl;
    const char *path = std::getenv("PTCORE_RCCL_LIB");
    // A process that already has an RCCL (PyTorch brings its own, soname librccl.so.1) must not get a second copy of it: ask for
    // the loaded one first.
    void *lib = path ? dlopen(path, RTLD_NOW | RTLD_LOCAL) : dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
    if (!lib && !path) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!lib && !path) lib = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!lib && !path) lib = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!lib) return fail(PT_ERR_HIP, std::string("PTCORE_GATHER=rccl: cannot load librccl.so: ") + dlerror());
#define PT_RCCL_SYM(field, name)                                                              \
    R.field = reinterpret_cast<decltype(R.field)>(dlsym(lib, name));                          \
    if (!R.field) return fail(PT_ERR_HIP, std::string("PTCORE_GATHER=rccl: librccl.so has no ") + name);
    PT_RCCL_SYM(CommInitAll, "ncclCommInitAll")
    PT_RCCL_SYM(CommDestroy, "ncclCommDestroy")
    PT_RCCL_SYM(GroupStart, "ncclGroupStart")
    PT_RCCL_SYM(GroupEnd, "ncclGroupEnd")
    PT_RCCL_SYM(Send, "ncclSend")
    PT_RCCL_SYM(Recv, "ncclRecv")
    PT_RCCL_SYM(GetErrorString, "ncclGetErrorString")
#undef PT_RCCL_SYM
    std::vector<int> devs;
    for (const Device &d : ctx->devs) devs.push_back(d.ordinal);
    R.comms.assign(devs.size(), nullptr);
    const ncclResult_t r = R.CommInitAll(R.comms.data(), (int)devs.size(), devs.data());
    if (r != ncclSuccess) {
        R.comms.clear();
        return fail(PT_ERR_HIP, std::string("PTCORE_GATHER=rccl: ncclCommInitAll: ") + R.GetErrorString(r));
    }
    R.lib = lib;
    return PT_OK;
}

#define RCCL_TRY(expr)                                                                                   \
    do {                                                                                                 \
        const ncclResult_t r_ = (expr);                                                                  \
        if (r_ != ncclSuccess) return fail(PT_ERR_HIP, std::string(#expr ": ") + ctx->rccl.GetErrorString(r_)); \
    } while (0)

// The gather: every device writes its tiles of some per-pixel planes, the tiles reach devices[0], untile_kernel turns them into
// row-major frames there, the frames go to the host.  A plane is one such quantity: its kind (element type, elements per tile, the
// UntileArgs pair it goes through), its three buffers -- the device's tiles, every shard's tiles one behind the other on devices[0], the
// frame on devices[0]; each as a function that reserves n elements and returns the pointer -- and where on the host it goes.
enum PlaneKind { PLANE_RGBA, PLANE_F64X3, PLANE_U32A, PLANE_U32B };
const struct { size_t per_tile, elem; ncclDataType_t type; } plane_kinds[] = {
    {4096, 1, ncclUint8}, {3072, sizeof(double), ncclDouble}, {1024, sizeof(uint32_t), ncclUint32}, {1024, sizeof(uint32_t), ncclUint32}};

template <typename Owner, auto Member>
void *reserved(Owner &o, size_t n, hipError_t &e) {
    e = (o.*Member).reserve(n);
    return (o.*Member).p;
}

struct Plane {
    bool on;                                          // false: left out of this gather
    PlaneKind kind;
    void *(*tiles)(Device &, size_t, hipError_t &);
    void *(*gathered)(pt_ctx &, size_t, hipError_t &);
    void *(*frame)(pt_ctx &, size_t, hipError_t &);
    void *host;                                       // or null: gathered and untiled, not copied
    size_t host_stride;                               // bytes per row; 0: rows back to back
};

// fill(d, dst) has device d write its tiles of plane k to dst[k] (null for a plane that is off), on d's stream.  devices[0] fills the
// gather buffers themselves; the others fill their own buffers, which a peer copy on the same stream takes over.  With RCCL loaded every
// device, devices[0] too, fills its own buffers and one group of sends and receives moves all planes of all devices: the sends on the
// devices' streams, the matching receives on devices[0]'s -- one group, so that the sends and receives of this one process pair up without
// deadlock (ncclGather is this same pattern; the counts differ per rank here).
template <size_t N, typename Fill>
int32_t gather_planes(pt_ctx *ctx, const Plane (&planes)[N], Fill &&fill) {
    const Frame &fr = ctx->frame;
    const size_t W = (size_t)fr.cfg.width, H = (size_t)fr.cfg.height;
    const size_t ndev = ctx->devs.size(), ntiles = (size_t)fr.ntx * (size_t)fr.nty;
    const pt_ctx::Rccl &R = ctx->rccl;
    Device &d0 = ctx->devs[0];
    auto bytes = [&](size_t k, size_t tiles) { return tiles * plane_kinds[planes[k].kind].per_tile * plane_kinds[planes[k].kind].elem; };
    hipError_t e = hipSuccess;
    char *g[N] = {};
    HIP_TRY(hipSetDevice(d0.ordinal));
    for (size_t k = 0; k < N; k++) {
        if (!planes[k].on) continue;
        g[k] = static_cast<char *>(planes[k].gathered(*ctx, ntiles * plane_kinds[planes[k].kind].per_tile, e));
        HIP_TRY(e);
    }
    std::vector<void *> own(ndev * N, nullptr);  // RCCL: what device i sends for plane k
    size_t before = 0;
    for (size_t i = 0; i < ndev; i++) {
        Device &d = ctx->devs[i];
        if (d.nlocal == 0) continue;
        const size_t nt = (size_t)d.nlocal;
        const bool direct = i == 0 && !R.lib;
        void **dst = &own[i * N];
        HIP_TRY(hipSetDevice(d.ordinal));
        for (size_t k = 0; k < N; k++) {
            if (!planes[k].on) continue;
            dst[k] = direct ? g[k] + bytes(k, before) : planes[k].tiles(d, nt * plane_kinds[planes[k].kind].per_tile, e);
            HIP_TRY(e);
        }
        if (int32_t rc = fill(d, dst)) return rc;
        if (!direct && !R.lib)  // gather over xGMI: peer DMA into devices[0]'s buffer, ordered on the source stream
            for (size_t k = 0; k < N; k++)
                if (planes[k].on) HIP_TRY(hipMemcpyPeerAsync(g[k] + bytes(k, before), d0.ordinal, dst[k], d.ordinal, bytes(k, nt), d.stream));
        before += nt;
    }
    if (R.lib) {
        RCCL_TRY(R.GroupStart());
        size_t off = 0;
        for (size_t i = 0; i < ndev; i++) {
            Device &d = ctx->devs[i];
            if (d.nlocal == 0) continue;
            const size_t nt = (size_t)d.nlocal;
            for (size_t k = 0; k < N; k++) {
                if (!planes[k].on) continue;
                const size_t count = nt * plane_kinds[planes[k].kind].per_tile;
                RCCL_TRY(R.Send(own[i * N + k], count, plane_kinds[planes[k].kind].type, 0, R.comms[i], d.stream));
                RCCL_TRY(R.Recv(g[k] + bytes(k, off), count, plane_kinds[planes[k].kind].type, (int)i, R.comms[0], d0.stream));
            }
            off += nt;
        }
        RCCL_TRY(R.GroupEnd());
    }
    for (size_t i = 1; i < ndev; i++) {
        HIP_TRY(hipSetDevice(ctx->devs[i].ordinal));
        HIP_TRY(hipStreamSynchronize(ctx->devs[i].stream));
    }
    HIP_TRY(hipSetDevice(d0.ordinal));
    ptk::UntileArgs U;
    std::memset(&U, 0, sizeof U);
    U.width = (int32_t)W; U.height = (int32_t)H; U.ntx = fr.ntx; U.nty = fr.nty; U.stride = (int32_t)W * 4; U.shard_count = (int32_t)ndev;
    char *f[N] = {};
    for (size_t k = 0; k < N; k++) {
        if (!planes[k].on) continue;
        f[k] = static_cast<char *>(planes[k].frame(*ctx, W * H * (plane_kinds[planes[k].kind].per_tile / 1024), e));
        HIP_TRY(e);
        switch (planes[k].kind) {
            case PLANE_RGBA: U.tiles_rgba = reinterpret_cast<uint8_t *>(g[k]); U.rgba = reinterpret_cast<uint8_t *>(f[k]); break;
            case PLANE_F64X3: U.tiles_accum = reinterpret_cast<double *>(g[k]); U.accum = reinterpret_cast<double *>(f[k]); break;
            case PLANE_U32A: U.tiles_u32a = reinterpret_cast<uint32_t *>(g[k]); U.u32a = reinterpret_cast<uint32_t *>(f[k]); break;
            case PLANE_U32B: U.tiles_u32b = reinterpret_cast<uint32_t *>(g[k]); U.u32b = reinterpret_cast<uint32_t *>(f[k]); break;
        }
    }
    hipLaunchKernelGGL(ptk::untile_kernel, dim3((unsigned)fr.ntx, (unsigned)fr.nty, 4), dim3(PT_BLOCK), 0, d0.stream, U);
    HIP_TRY(hipGetLastError());
    for (size_t k = 0; k < N; k++) {
        if (!planes[k].on || !planes[k].host) continue;
        const size_t row = W * (plane_kinds[planes[k].kind].per_tile / 1024) * plane_kinds[planes[k].kind].elem;
        if (planes[k].host_stride)
            HIP_TRY(hipMemcpy2DAsync(planes[k].host, planes[k].host_stride, f[k], row, row, H, hipMemcpyDeviceToHost, d0.stream));
        else
            HIP_TRY(hipMemcpyAsync(planes[k].host, f[k], row * H, hipMemcpyDeviceToHost, d0.stream));
    }
    HIP_TRY(hipStreamSynchronize(d0.stream));
    return PT_OK;
}

// ---- The quantities that travel through gather_planes one plane at a time: the plane's row and what has device d write its tiles
// of it to dst, on d's stream.  gather_one runs one of them into its row-major frame on devices[0] and, when asked for, to the host.
struct Gathered {
    Plane row;
    int32_t (*fill)(pt_ctx *ctx, Device &d, uint32_t which, void *dst);
    uint32_t which;  // the feature or half-sum plane
};

int32_t gather_one(pt_ctx *ctx, const Gathered &g, void *host) {
    Plane planes[] = {g.row};
    planes[0].host = host;
    return gather_planes(ctx, planes, [&](Device &d, void *const *dst) { return g.fill(ctx, d, g.which, dst[0]); });
}

template <auto Tiles, auto Gather, auto Framed>
Plane plane_row(PlaneKind kind) {
    return {true, kind, reserved<Device, Tiles>, reserved<pt_ctx, Gather>, reserved<pt_ctx, Framed>, nullptr, 0};
}

// The fills.  Group `which` of one of the device's arrays of per-slot double sums (planes_tiles_kernel): the radiance sums S, their
// squares Q, a half-buffer sum (0 SA, 1 QA, 2 SB, 3 QB), a feature plane (0 normal, 1 albedo, 2 depth); zeros before the first chunk
template <auto Sums>
int32_t fill_sum(pt_ctx *ctx, Device &d, uint32_t which, void *dst) {
    hipLaunchKernelGGL(ptk::planes_tiles_kernel, dim3((d.nslots + PT_BLOCK - 1) / PT_BLOCK), dim3(PT_BLOCK), 0, d.stream, (d.*Sums).p,
                       static_cast<double *>(dst), d.nslots, which, d.acc_started ? 0 : 1, tile_geom(ctx->frame, d));
    HIP_TRY(hipGetLastError());
    return PT_OK;
}
// the counts of an adaptive frame, through untile_kernel's u32a plane (the buffers of read_frame's nseg)
int32_t fill_counts(pt_ctx *ctx, Device &d, uint32_t, void *dst) {
    hipLaunchKernelGGL(ptk::counts_tiles_kernel, dim3((d.nslots + PT_BLOCK - 1) / PT_BLOCK), dim3(PT_BLOCK), 0, d.stream, d.blk_spp.p,
                       static_cast<uint32_t *>(dst), d.nslots, tile_geom(ctx->frame, d));
    HIP_TRY(hipGetLastError());
    return PT_OK;
}
// the object index plane in scene indices, through untile_kernel's u32a plane like the counts
int32_t fill_ids(pt_ctx *ctx, Device &d, uint32_t, void *dst) {
    hipLaunchKernelGGL(ptk::ids_tiles_kernel, dim3((d.nslots + PT_BLOCK - 1) / PT_BLOCK), dim3(PT_BLOCK), 0, d.stream, d.obj_ids.p, d.obj_map.p,
                       (int32_t)ctx->frame.world_scene.size(), static_cast<uint32_t *>(dst), d.nslots, tile_geom(ctx->frame, d));
    HIP_TRY(hipGetLastError());
    return PT_OK;
}

const Gathered g_sums = {plane_row<&Device::tiles_accum, &pt_ctx::g_tiles_accum, &pt_ctx::f_accum>(PLANE_F64X3), fill_sum<&Device::acc>, 0};
const Gathered g_m2 = {plane_row<&Device::tiles_m2, &pt_ctx::g_tiles_m2, &pt_ctx::f_m2>(PLANE_F64X3), fill_sum<&Device::m2>, 0};
const Gathered g_counts = {plane_row<&Device::tiles_seg, &pt_ctx::g_tiles_seg, &pt_ctx::f_seg>(PLANE_U32A), fill_counts, 0};
const Gathered g_feature[3] = {{plane_row<&Device::tiles_feat, &pt_ctx::g_tiles_feat, &pt_ctx::f_feat_n>(PLANE_F64X3), fill_sum<&Device::feat>, 0},
                               {plane_row<&Device::tiles_feat, &pt_ctx::g_tiles_feat, &pt_ctx::f_feat_a>(PLANE_F64X3), fill_sum<&Device::feat>, 1},
                               {plane_row<&Device::tiles_feat, &pt_ctx::g_tiles_feat, &pt_ctx::f_feat_d>(PLANE_F64X3), fill_sum<&Device::feat>, 2}};
const Gathered g_ids = {plane_row<&Device::tiles_seg, &pt_ctx::g_tiles_seg, &pt_ctx::f_ids>(PLANE_U32A), fill_ids, 0};
const Gathered g_half[4] = {{plane_row<&Device::tiles_hv, &pt_ctx::g_tiles_hv, &pt_ctx::f_hv_sa>(PLANE_F64X3), fill_sum<&Device::hv>, 0},
                            {plane_row<&Device::tiles_hv, &pt_ctx::g_tiles_hv, &pt_ctx::f_hv_qa>(PLANE_F64X3), fill_sum<&Device::hv>, 1},
                            {plane_row<&Device::tiles_hv, &pt_ctx::g_tiles_hv, &pt_ctx::f_hv_sb>(PLANE_F64X3), fill_sum<&Device::hv>, 2},
                            {plane_row<&Device::tiles_hv, &pt_ctx::g_tiles_hv, &pt_ctx::f_hv_qb>(PLANE_F64X3), fill_sum<&Device::hv>, 3}};

// The inputs of the post-frame filters as row-major planes on devices[0]: the four half sums or S and Q, the counts of an adaptive
// frame, the features of a frame that has them.  All reads: the sums, the block table and the event lists of the frame stay as they are.
int32_t gather_filter_inputs(pt_ctx *ctx, bool halves) {
    const Frame &fr = ctx->frame;
    if (halves) {
        for (const Gathered &g : g_half)
            if (int32_t rc = gather_one(ctx, g, nullptr)) return rc;
    } else {
        if (int32_t rc = gather_one(ctx, g_sums, nullptr)) return rc;
        if (int32_t rc = gather_one(ctx, g_m2, nullptr)) return rc;
    }
    if (fr.adaptive)
        if (int32_t rc = gather_one(ctx, g_counts, nullptr)) return rc;
    if (fr.features > 0)
        for (const Gathered &g : g_feature)
            if (int32_t rc = gather_one(ctx, g, nullptr)) return rc;
    return PT_OK;
}

// ---- What the entry points that read a finished frame ask of it.  The frame is the open one, or the last one finished on ctx (its
// sums stay on the devices until the next frame opens), with at least one step done; then the needs, tested in the order given.
// (NEED_NOT_GL: the filters, which a GL frame opened with pt_set_shading_features meets; NEED_CPU_CAMERA: pt_temporal, whose projection
// is the CPU engine's camera, which no GL frame meets)
enum FrameNeed { NEED_MOMENTS, NEED_ADAPTIVE, NEED_HALVES, NEED_FEATURES, NEED_NOT_GL, NEED_2_SAMPLES, NEED_CPU_CAMERA };

int32_t frame_needs(pt_ctx *ctx, const char *who, std::initializer_list<FrameNeed> needs) {
    const Frame &fr = ctx->frame;
    const std::string w = std::string(who) + ": ";
    if (fr.done_spp <= 0 || fr.chunk == 0) return fail(PT_ERR_STATE, w + "no frame with samples on this context (pt_step or pt_render first)");
    // (an adaptive block stops at two samples or more, so every pixel holds at least min(done, 2))
    const struct { bool met; const char *text; } table[] = {
        {fr.moments, "the frame was rendered with moments off (pt_set_moments)"},
        {fr.adaptive, "the frame was rendered with adaptive sampling off (pt_set_adaptive)"},
        {fr.halves, "the frame was rendered with halves off (pt_set_halves)"},
        {fr.features > 0, "the frame was rendered with features off (pt_set_features)"},
        {!fr.gl || fr.gl_filter, "not available for a frame rendered with GL shading (pt_set_shading)"},
        {fr.done_spp >= 2, "every pixel needs at least 2 samples"},
        {!fr.gl, "not available for a frame rendered with GL shading (pt_set_shading)"}};
    for (FrameNeed n : needs)
        if (!table[n].met) return fail(PT_ERR_STATE, w + table[n].text);
    return PT_OK;
}

int32_t stride_fits(const Frame &fr, const uint8_t *rgba, int32_t stride) {
    if (rgba && stride < fr.cfg.width * 4) return fail(PT_ERR_INVALID, "stride smaller than 4*width");
    return PT_OK;
}

// The filter configuration of entry point `who`: the caller's, or the defaults with `iterations`; `what` is "" or, where the filter
// is one argument among others, "filter ".
int32_t filter_config(const char *who, const char *what, const pt_atrous_config *cfg, int32_t iterations, pt_atrous_config &c) {
    c = {iterations, 0, 4.0, 0.1, 0.1, 0.2};
    if (cfg) c = *cfg;
    const std::string w = std::string(who) + ": " + what;
    if (c.iterations < 0 || c.iterations > PTA_MAX_ITERATIONS) return fail(PT_ERR_INVALID, w + "iterations must be 0..6");
    if (!(c.sigma_l > 0.0) || !(c.sigma_n >= 0.0) || !(c.sigma_z >= 0.0) || !(c.sigma_a >= 0.0))
        return fail(PT_ERR_INVALID, w + "sigma_l must be > 0, sigma_n, sigma_z and sigma_a >= 0 (0 = term off)");
    return PT_OK;
}

// The wall clock and the N events of one filter call: created where the call is about to launch, destroyed with the scope, on every
// path.  (Not Device::ev: those lists are the open frame's statistics.)
template <int N>
struct FilterClock {
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    hipEvent_t ev[N] = {};
    FilterClock() = default;
    FilterClock(const FilterClock &) = delete;
    FilterClock &operator=(const FilterClock &) = delete;
    ~FilterClock() {
        if (g_leave_device_memory) return;
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    int32_t create() {
        for (hipEvent_t &e : ev)
            if (hipError_t err = hipEventCreate(&e); err != hipSuccess) return fail(PT_ERR_HIP, std::string("hipEventCreate: ") + hipGetErrorString(err));
        return PT_OK;
    }
    double wall_ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

// What pt_atrous and pt_temporal filter in and into, for a frame of npix pixels (devices[0] is current).
int32_t reserve_filter(pt_ctx *ctx, size_t npix) {
    pt_ctx::Atrous &B = ctx->at;
    for (int k = 0; k < 2; k++) {
        HIP_TRY(B.col[k].reserve(3 * npix));
        HIP_TRY(B.var[k].reserve(npix));
    }
    HIP_TRY(B.guide.reserve(npix));
    HIP_TRY(B.part.reserve(2 * (size_t)ptl::grid_1d(npix)));
    HIP_TRY(ctx->f_rgba.reserve(npix * 4));
    return PT_OK;
}

// rgba (rows `stride` bytes apart), mean and var of pt_atrous and pt_temporal to the host, each when asked for, on devices[0]'s stream
int32_t copy_filtered(pt_ctx *ctx, int cur, uint8_t *rgba, int32_t stride, double *mean, double *var) {
    const size_t W = (size_t)ctx->frame.cfg.width, H = (size_t)ctx->frame.cfg.height;
    const hipStream_t s = ctx->devs[0].stream;
    if (rgba) HIP_TRY(hipMemcpy2DAsync(rgba, (size_t)stride, ctx->f_rgba.p, W * 4, W * 4, H, hipMemcpyDeviceToHost, s));
    if (mean) HIP_TRY(hipMemcpyAsync(mean, ctx->at.col[cur].p, 3 * W * H * sizeof(double), hipMemcpyDeviceToHost, s));
    if (var) HIP_TRY(hipMemcpyAsync(var, ctx->at.var[cur].p, W * H * sizeof(double), hipMemcpyDeviceToHost, s));
    return PT_OK;
}

// pt_atrous_halves behind its refusals, and step 1 of pt_set_adaptive_filtered's check: the inputs gathered to devices[0], then prep, the
// pair iterations and the combine on its stream (between the clock's two events, when there is one).  ctx->ah holds the result: mean,
// err, the partials of the figures (grid_1d(npix) of them), fA and fB when `half` asks, and the bad mask in the guide's last plane.
int32_t halves_filter(pt_ctx *ctx, const pt_atrous_config &c, bool half, FilterClock<2> *clock) {
    Frame &fr = ctx->frame;
    const int32_t W = fr.cfg.width, H = fr.cfg.height;
    if (int32_t rc = gather_filter_inputs(ctx, true)) return rc;
    const bool feat = fr.features > 0;
    Device &d0 = ctx->devs[0];
    pt_ctx::Halves &B = ctx->ah;
    HIP_TRY(hipSetDevice(d0.ordinal));
    const size_t npix = (size_t)W * (size_t)H;
    const uint32_t grid1 = ptl::grid_1d(npix);
    for (int k = 0; k < 2; k++) {
        HIP_TRY(B.col[k].reserve(6 * npix));
        HIP_TRY(B.var[k].reserve(2 * npix));
    }
    HIP_TRY(B.guide.reserve(PTA_GUIDE_PLANES * npix));
    HIP_TRY(B.mean.reserve(3 * npix));
    HIP_TRY(B.err.reserve(npix));
    if (half) HIP_TRY(B.half.reserve(6 * npix));
    HIP_TRY(B.part.reserve(grid1));
    if (clock) {
        if (int32_t rc = clock->create()) return rc;
        HIP_TRY(hipEventRecord(clock->ev[0], d0.stream));
    }
    ptk::AtrousPairPrepArgs PA;
    std::memset(&PA, 0, sizeof PA);
    PA.sa = ctx->f_hv_sa.p; PA.qa = ctx->f_hv_qa.p; PA.sb = ctx->f_hv_sb.p; PA.qb = ctx->f_hv_qb.p;
    PA.cnt = fr.adaptive ? ctx->f_seg.p : nullptr;
    PA.fn = feat ? ctx->f_feat_n.p : nullptr;
    PA.fa = feat ? ctx->f_feat_a.p : nullptr;
    PA.fd = feat ? ctx->f_feat_d.p : nullptr;
    PA.guide = B.guide.p;
    PA.col = B.col[0].p;
    PA.var = B.var[0].p;
    PA.npix = (uint32_t)npix;
    PA.n = (uint32_t)fr.done_spp;
    hipLaunchKernelGGL(ptk::atrous_pair_prep_kernel, dim3(grid1), dim3(PT_BLOCK), 0, d0.stream, PA);
    double *const col[2] = {B.col[0].p, B.col[1].p}, *const vr[2] = {B.var[0].p, B.var[1].p};
    const int cur = ptl::pair_iterations(ptl::filter_params(c, feat), col, vr, B.guide.p, W, H, d0.stream);
    ptk::HalvesCombineArgs CA;
    std::memset(&CA, 0, sizeof CA);
    CA.col = col[cur]; CA.var = vr[cur]; CA.guide = B.guide.p;
    CA.mean = B.mean.p;
    CA.err = B.err.p;
    CA.half_means = half ? B.half.p : nullptr;
    CA.partial = B.part.p;
    CA.npix = (uint32_t)npix;
    hipLaunchKernelGGL(ptk::halves_combine_kernel, dim3(grid1), dim3(PT_BLOCK), 0, d0.stream, CA);
    HIP_TRY(hipGetLastError());
    if (clock) HIP_TRY(hipEventRecord(clock->ev[1], d0.stream));
    return PT_OK;
}

// The check that ends a pt_step of an adaptive frame with pt_set_adaptive_filtered's rule (pt_atrous.h BLOCKS), on every device.  Once
// it decides: the active blocks' counts are stamped first (the pair filter reads every pixel's own count through the gather), then on
// devices[0] the pair filter and ptl::block_map_sequence; the map goes to the host -- where pt_read_block_figures finds it -- and from
// there to every device, whatever their number; keep_from_map_kernel and compact_kernel follow on each.  Before it decides only those
// two run, without a map.  The result words are read by the caller once the streams have drained.
int32_t filtered_check(pt_ctx *ctx, ptk::AdaptResult *host_res) {
    Frame &fr = ctx->frame;
    const int32_t W = fr.cfg.width, H = fr.cfg.height, nbx = ptl::blocks_across(W), nby = ptl::blocks_across(H);
    const size_t nb = (size_t)nbx * (size_t)nby;
    const bool decide = fr.done_spp >= std::max(fr.ad.min_spp, 4);
    auto keep_args = [&](Device &d, bool mapped, bool stamp_only = false) {
        ptk::KeepFromMapArgs A;
        std::memset(&A, 0, sizeof A);
        A.active = d.act[d.act_cur].p;
        A.pooled = mapped ? d.map_pooled.p : nullptr;
        A.stop = mapped ? d.map_stop.p : nullptr;
        A.blk_spp = d.blk_spp.p;
        A.keep = stamp_only ? nullptr : d.blk_keep.p;
        A.noise = stamp_only ? nullptr : d.blk_noise.p;
        A.nact = d.nact;
        A.n = fr.done_spp;
        A.nbx = nbx; A.nby = nby;
        A.G = tile_geom(fr, d);
        return A;
    };
    if (decide) {
        for (Device &d : ctx->devs) {
            if (d.nlocal == 0 || d.nact == 0) continue;
            HIP_TRY(hipSetDevice(d.ordinal));
            ptl::keep_sequence(keep_args(d, false, true), nullptr, d.stream);
            HIP_TRY(hipGetLastError());
        }
        Device &d0 = ctx->devs[0];
        pt_ctx::Blocks &M = ctx->bf;
        HIP_TRY(hipSetDevice(d0.ordinal));
        HIP_TRY(M.s.reserve(nb));
        HIP_TRY(M.k.reserve(nb));
        HIP_TRY(M.pooled.reserve(nb));
        HIP_TRY(M.own.reserve(nb));
        HIP_TRY(M.stop.reserve(nb));
        int32_t frc = PT_OK;
        if (int32_t rc = timed(d0, EV_BLOCKS, [&] {  // gathers, pair filter and the map as one
                frc = halves_filter(ctx, fr.fa.filter, false, nullptr);
                if (frc != PT_OK) return;
                const pt_ctx::Halves &B = ctx->ah;
                const size_t npix = (size_t)W * (size_t)H;
                ptl::block_map_sequence(B.mean.p, B.err.p, B.guide.p + (size_t)PTA_GUIDE_BAD * npix, ptl::BlockMap{M.s.p, M.k.p, M.pooled.p, M.own.p, M.stop.p},
                                        W, H, fr.fa.pool, fr.ad.target, d0.stream);
            }))
            return frc != PT_OK ? frc : rc;
        if (frc != PT_OK) return frc;
        M.h_pooled.resize(nb);
        M.h_own.resize(nb);
        M.h_stop.resize(nb);
        HIP_TRY(hipMemcpyAsync(M.h_pooled.data(), M.pooled.p, nb * sizeof(double), hipMemcpyDeviceToHost, d0.stream));
        HIP_TRY(hipMemcpyAsync(M.h_own.data(), M.own.p, nb * sizeof(double), hipMemcpyDeviceToHost, d0.stream));
        HIP_TRY(hipMemcpyAsync(M.h_stop.data(), M.stop.p, nb, hipMemcpyDeviceToHost, d0.stream));
        HIP_TRY(hipStreamSynchronize(d0.stream));
        fr.fa_checks++;
    }
    for (size_t i = 0; i < ctx->devs.size(); i++) {
        Device &d = ctx->devs[i];
        if (d.nlocal == 0 || d.nact == 0) continue;
        HIP_TRY(hipSetDevice(d.ordinal));
        if (decide) {
            HIP_TRY(d.map_pooled.reserve(nb));
            HIP_TRY(d.map_stop.reserve(nb));
            HIP_TRY(hipMemcpyAsync(d.map_pooled.p, ctx->bf.h_pooled.data(), nb * sizeof(double), hipMemcpyHostToDevice, d.stream));
            HIP_TRY(hipMemcpyAsync(d.map_stop.p, ctx->bf.h_stop.data(), nb, hipMemcpyHostToDevice, d.stream));
        }
        ptk::CompactArgs K;
        std::memset(&K, 0, sizeof K);
        K.active = d.act[d.act_cur].p;
        K.keep = d.blk_keep.p;
        K.noise = d.blk_noise.p;
        K.next = d.act[d.act_cur ^ 1].p;
        K.res = d.ad_res.p;
        K.nact = d.nact;
        if (int32_t rc = timed(d, EV_CHECK, [&] { ptl::keep_sequence(keep_args(d, decide), &K, d.stream); })) return rc;
        HIP_TRY(hipMemcpyAsync(&host_res[i], d.ad_res.p, sizeof host_res[i], hipMemcpyDeviceToHost, d.stream));
    }
    return PT_OK;
}

}  // namespace

extern "C" {

int32_t pt_abi_version(void) { return PT_ABI_VERSION; }

int32_t pt_set_fog(pt_ctx *ctx, const pt_fog *fog) {
    if (!ctx) return fail(PT_ERR_INVALID, "ctx is null");
    if (ctx->frame.open) return fail(PT_ERR_STATE, "pt_set_fog while a frame is open");
    ctx->fog_on = fog != nullptr;
    if (fog) ctx->fog_raw = *fog;
    else std::memset(&ctx->fog_raw, 0, sizeof ctx->fog_raw);
    return PT_OK;
}

int32_t pt_fog_last_stats(pt_ctx *ctx, pt_fog_stats *out) {
    if (!ctx || !out) return fail(PT_ERR_INVALID, "null argument");
    if (int32_t rc = collect_fog(ctx)) return rc;
    *out = ctx->fog_last;
    return PT_OK;
}

int32_t pt_set_shading(pt_ctx *ctx, const pt_shading *s) {
    if (!ctx) return fail(PT_ERR_INVALID, "ctx is null");
    if (ctx->frame.open) return fail(PT_ERR_STATE, "pt_set_shading while a frame is open");
    if (s && s->model != PT_SHADING_CPU && s->model != PT_SHADING_GL) return fail(PT_ERR_INVALID, "unknown shading model");
    if (s && s->model == PT_SHADING_GL && (s->num_materials < 0 || (s->num_materials > 0 && !s->materials)))
        return fail(PT_ERR_INVALID, "GL shading needs num_materials >= 0 entries in materials");
    ctx->shading_model = s ? s->model : PT_SHADING_CPU;
    ctx->gl_extras.clear();
    if (s && s->model == PT_SHADING_GL) ctx->gl_extras.assign(s->materials, s->materials + s->num_materials);
    return PT_OK;
}

int32_t pt_shading_last_stats(pt_ctx *ctx, pt_shading_stats *out) {
    if (!ctx || !out) return fail(PT_ERR_INVALID, "null argument");
    if (int32_t rc = collect_shading(ctx)) return rc;
    *out = ctx->shading_last;
    return PT_OK;
}

const char *pt_last_error(void) { return g_last_error.c_str(); }

int32_t pt_device_count(int32_t *count) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (count) *count = (e == hipSuccess) ? n : 0;
    if (e != hipSuccess || n <= 0) return fail(PT_ERR_NO_DEVICE, std::string("no HIP device: ") + hipGetErrorString(e));
    return PT_OK;
}

int32_t pt_create(const int32_t *devices, int32_t ndev, pt_ctx **out) {
    if (!out) return fail(PT_ERR_INVALID, "out is null");
    *out = nullptr;
    if (ndev <= 0 || ndev > 64) return fail(PT_ERR_INVALID, "ndev must be in 1..64");
    int32_t n = 0;
    if (int32_t rc = pt_device_count(&n)) return rc;
    pt_ctx *ctx = new pt_ctx();
    if (const char *e = std::getenv("PTCORE_L_BUDGET_MB")) {
        long mb = std::atol(e);
        if (mb > 0) { ctx->l_budget_bytes = (size_t)mb << 20; ctx->auto_grow = false; }
    }
    if (const char *e = std::getenv("PTCORE_AUTO_GROW")) ctx->auto_grow = std::atoi(e) != 0;
    if (const char *e = std::getenv("PTCORE_CLAIM")) {
        long c = std::atol(e);
        if (c >= 64 && c % 64 == 0) ctx->claim = (uint32_t)c;
    }
    if (const char *e = std::getenv("PTCORE_SCAN")) {
        if (!std::strcmp(e, "uniform")) ctx->scan_mode = ptk::SCAN_UNIFORM;
        else if (!std::strcmp(e, "verify")) ctx->scan_mode = ptk::SCAN_VERIFY;
        else if (!std::strcmp(e, "wide")) ctx->scan_mode = ptk::SCAN_BROAD_WIDE;
        else if (!std::strcmp(e, "verify_wide")) ctx->scan_mode = ptk::SCAN_VERIFY_WIDE;
        else if (!std::strcmp(e, "bvh")) ctx->scan_mode = ptk::SCAN_BVH;
        else if (!std::strcmp(e, "verify_bvh")) ctx->scan_mode = ptk::SCAN_VERIFY_BVH;
        else ctx->scan_mode = -1;
    }
    if (const char *e = std::getenv("PTCORE_PROFILE")) ctx->profile_sections = std::atoi(e) != 0;
    if (const char *e = std::getenv("PTCORE_SPLIT_ROUNDS")) ctx->split_rounds = std::max(0, std::min(64, std::atoi(e)));
    if (const char *e = std::getenv("PTCORE_TAIL")) ctx->tail_nested = std::strcmp(e, "trip") != 0;
    if (const char *e = std::getenv("PTCORE_PRIMARY")) ctx->primary_coop = std::strcmp(e, "lane") != 0;
    if (const char *e = std::getenv("PTCORE_PIPELINE")) ctx->pipeline = !std::strcmp(e, "wavefront") ? 1 : !std::strcmp(e, "walk32") ? 2 : !std::strcmp(e, "mega") ? 0 : -1;
    if (const char *e = std::getenv("PTCORE_WF_MIN_LANES")) ctx->wf_min_lanes = std::max(1, std::min(64, std::atoi(e)));
    if (const char *e = std::getenv("PTCORE_WF_SORT")) ctx->wf_sort = std::atoi(e);
    if (const char *e = std::getenv("PTCORE_BLOCKS_PER_CU")) {
        long c = std::atol(e);
        if (c >= 1 && c <= 8) ctx->max_blocks_per_cu = (int)c;
    }
    ctx->devs.resize((size_t)ndev);
    for (int i = 0; i < ndev; i++) {
        Device &d = ctx->devs[(size_t)i];
        d.ordinal = devices ? devices[i] : i;
        if (d.ordinal < 0 || d.ordinal >= n) {
            pt_destroy(ctx);
            return fail(PT_ERR_INVALID, "device ordinal out of range");
        }
        hipError_t e = hipSetDevice(d.ordinal);
        hipDeviceProp_t prop;
        if (e == hipSuccess) e = hipGetDeviceProperties(&prop, d.ordinal);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&d.own_stream, hipStreamNonBlocking);
        if (e != hipSuccess) {
            pt_destroy(ctx);
            return fail(PT_ERR_HIP, std::string("device init: ") + hipGetErrorString(e));
        }
        d.num_cu = prop.multiProcessorCount;
        d.stream = d.own_stream;
    }
    // tile gather goes device -> devices[0] by peer DMA over xGMI: enable direct access where the
    // topology offers it (without it hipMemcpyPeerAsync still works, staged through the host)
    for (int i = 1; i < ndev; i++) {
        const int a = ctx->devs[(size_t)i].ordinal, b = ctx->devs[0].ordinal;
        if (a == b) continue;
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, a, b) == hipSuccess && can && hipSetDevice(a) == hipSuccess) {
            hipError_t e = hipDeviceEnablePeerAccess(b, 0);
            if (e != hipSuccess) (void)hipGetLastError();  // already enabled or refused: the copy path copes
        }
    }
    if (const char *e = std::getenv("PTCORE_GATHER")) {
        if (!std::strcmp(e, "rccl")) {
            if (int32_t rc = rccl_open(ctx)) {
                pt_destroy(ctx);
                return rc;
            }
        } else if (std::strcmp(e, "peer") != 0) {
            pt_destroy(ctx);
            return fail(PT_ERR_INVALID, "PTCORE_GATHER must be peer or rccl");
        }
    }
    *out = ctx;
    return PT_OK;
}

int32_t pt_debug_gather_mode(pt_ctx *ctx) { return ctx && ctx->rccl.lib ? 1 : 0; }

void pt_destroy(pt_ctx *ctx) {
    if (!ctx) return;
    if (ctx->rccl.lib) {
        for (size_t i = 0; i < ctx->rccl.comms.size(); i++)
            if (ctx->rccl.comms[i] && hipSetDevice(ctx->devs[i].ordinal) == hipSuccess) (void)ctx->rccl.CommDestroy(ctx->rccl.comms[i]);
        ctx->rccl.comms.clear();
        // (the library stays mapped: RCCL keeps threads and device state of its own that a dlclose would pull away under them)
        ctx->rccl.lib = nullptr;
    }
    // each device's memory and events are freed with that device current, after its stream has drained: Device() takes them over
    // in the assignment and dies with them there.  Then the context's own planes, which live on the first device, with the context.
    const int first = ctx->devs.empty() ? 0 : ctx->devs[0].ordinal;
    for (Device &d : ctx->devs) {
        g_leave_device_memory = hipSetDevice(d.ordinal) != hipSuccess;
        const hipStream_t own = g_leave_device_memory ? nullptr : d.own_stream;
        if (own) (void)hipStreamSynchronize(own);
        if (d.ev_first && !g_leave_device_memory) (void)hipEventDestroy(d.ev_first);
        if (d.ev_last && !g_leave_device_memory) (void)hipEventDestroy(d.ev_last);
        d = Device();
        if (own) (void)hipStreamDestroy(own);
    }
    g_leave_device_memory = hipSetDevice(first) != hipSuccess;
    delete ctx;
    g_leave_device_memory = false;
}

int32_t pt_post_process(pt_ctx *ctx, const pt_post_config *post, const double *accum, int32_t spp, uint8_t *rgba, int32_t stride,
                        int32_t width, int32_t height) {
    if (!ctx || !post || !rgba) return fail(PT_ERR_INVALID, "null argument");
    if (width <= 0 || height <= 0 || stride < width * 4) return fail(PT_ERR_INVALID, "bad frame size or stride");
    if (post->tonemap && !accum) return fail(PT_ERR_INVALID, "tonemap needs the accum buffer");
    if (ctx->frame.open) return fail(PT_ERR_STATE, "a frame is open");
    Device &d = ctx->devs[0];
    HIP_TRY(hipSetDevice(d.ordinal));
    const size_t npix = (size_t)width * (size_t)height;
    HIP_TRY(ctx->f_rgba.reserve(npix * 4));
    HIP_TRY(ctx->g_tiles_rgba.reserve(npix * 4));  // second frame-sized byte buffer (ping-pong)
    uint8_t *cur = ctx->f_rgba.p, *other = ctx->g_tiles_rgba.p;
    hipStream_t s = d.own_stream;
    const unsigned grid = ptl::grid_1d(npix);
    if (post->tonemap) {
        HIP_TRY(ctx->f_accum.reserve(npix * 3));
        HIP_TRY(hipMemcpyAsync(ctx->f_accum.p, accum, npix * 3 * sizeof(double), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(ptk::post_tonemap_kernel, dim3(grid), dim3(PT_BLOCK), 0, s, ctx->f_accum.p, spp, cur, (int32_t)npix);
        HIP_TRY(hipGetLastError());
    } else {
        HIP_TRY(hipMemcpy2DAsync(cur, (size_t)width * 4, rgba, (size_t)stride, (size_t)width * 4, (size_t)height,
                                 hipMemcpyHostToDevice, s));
    }
    if (post->denoise && width > 2 && height > 2) {
        const double ss = post->sigma_s > 0 ? post->sigma_s : 1.0, sr = post->sigma_r > 0 ? post->sigma_r : 0.15;
        hipLaunchKernelGGL(ptk::post_bilateral_kernel, dim3(grid), dim3(PT_BLOCK), 0, s, cur, other, width, height, 2 * ss * ss,
                           2 * sr * sr);
        HIP_TRY(hipGetLastError());
        std::swap(cur, other);
    }
    if (post->smooth && width > 2 && height > 2 && post->smooth_radius > 0 && post->smooth_strength > 0) {
        const int32_t rad = std::max(1, std::min(5, post->smooth_radius));
        const double str = std::max(0.0, std::min(1.0, post->smooth_strength));
        hipLaunchKernelGGL(ptk::post_smooth_kernel, dim3(grid), dim3(PT_BLOCK), 0, s, cur, other, width, height, rad, str);
        HIP_TRY(hipGetLastError());
        std::swap(cur, other);
    }
    HIP_TRY(hipMemcpy2DAsync(rgba, (size_t)stride, cur, (size_t)width * 4, (size_t)width * 4, (size_t)height, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return PT_OK;
}

int32_t pt_debug_profile(pt_ctx *ctx, uint64_t *out, int32_t n) {
    if (!ctx || !out) return fail(PT_ERR_INVALID, "null argument");
    if (!ctx->profile_sections) return fail(PT_ERR_STATE, "set PTCORE_PROFILE=1 before pt_create");
    for (int32_t i = 0; i < n && i < 3 * ptk::SEC_COUNT; i++) out[i] = g_profile_scratch[i];
    return 3 * ptk::SEC_COUNT;
}

// Host-only: builds the BVH of `scene` exactly as a render would and checks its invariants.
// out = {nodes, objects, depth, most slots used in a node, objects (or nodes) not reached exactly once,
// objects outside their slot's box, child boxes not inside the parent's box (or malformed slots), plane count}.
int32_t pt_debug_bvh_check(const pt_scene *scene, int32_t out[8]) {
    if (!scene || !out) return fail(PT_ERR_INVALID, "null argument");
    if (scene->num_materials < 0 || scene->num_objects < 0) return fail(PT_ERR_INVALID, "negative scene counts");
    std::vector<DevObj> world;
    std::vector<DevMat> mats;
    scene_to_world(*scene, world, mats);
    std::vector<int32_t> finite;
    double Bnd = 1.0;
    int planes = 0;
    for (size_t i = 0; i < world.size(); i++) {
        if ((world[i].kind & 0xff) == KIND_PLANE) { planes++; continue; }
        finite.push_back((int32_t)i);
        const ptbvh::Aabb bb = ptbvh::object_bounds(world[i]);
        for (int k = 0; k < 3; k++) Bnd = std::max(Bnd, std::max(std::fabs(bb.lo[k]), std::fabs(bb.hi[k])));
    }
    const double margin = Bnd * (1.0 / 4096.0);
    ptbvh::Built b = ptbvh::build(world, finite, margin);
    for (int lv = 16; b.stack_need >= PT_BVH_STACK && lv >= 0; lv -= 16) b = ptbvh::build(world, finite, margin, lv);
    std::vector<int> seen(world.size(), 0);
    int widest = 0, outside = 0, nested = 0;
    struct Item { int32_t node; double lo[3], hi[3]; };
    std::vector<Item> st;
    if (!b.nodes.empty()) {
        Item r;
        r.node = 0;
        for (int k = 0; k < 3; k++) { r.lo[k] = -INFINITY; r.hi[k] = INFINITY; }
        st.push_back(r);
    }
    std::vector<int> visits(b.nodes.size(), 0);
    while (!st.empty()) {
        const Item it = st.back();
        st.pop_back();
        const BvhNode &nd = b.nodes[(size_t)it.node];
        visits[(size_t)it.node]++;
        const uint32_t intm = (nd.meta >> 8) & 0xfu, objm = (nd.meta >> 12) & 0xfu;
        if (intm & objm) nested++;  // a slot is one or the other
        widest = std::max(widest, __builtin_popcount(intm | objm));
        for (int s = 0; s < 4; s++) {
            if (!((intm | objm) & (1u << s))) continue;
            const int rank = (int)((nd.meta >> (2 * s)) & 3u);
            // (centre / half-extent boxes are rounded one by one: a child's may stick out of its parent's by a few ulps, which
            // the walk does not care about -- every box holds its own content, that is all it relies on)
            for (int k = 0; k < 3; k++) {
                const double slo = bvh_slot_lo(nd, k, s), shi = bvh_slot_hi(nd, k, s);
                // (centre / half-extent boxes are rounded one by one: a child's may stick out of its parent's by a few ulps, which
                // the walk does not care about -- every box holds its own content, that is all it relies on)
                const double tol = 8.0 * 1.1920929e-7 * std::max(std::fabs(slo), std::fabs(shi));
                if (slo < it.lo[k] - tol || shi > it.hi[k] + tol) nested++;
            }
            if (intm & (1u << s)) {
                Item c;
                c.node = bvh_node_base(nd) + rank;
                for (int k = 0; k < 3; k++) { c.lo[k] = bvh_slot_lo(nd, k, s); c.hi[k] = bvh_slot_hi(nd, k, s); }
                if (c.node <= it.node || c.node >= (int32_t)b.nodes.size()) { nested++; continue; }
                st.push_back(c);
            } else {
                const int32_t slot = bvh_obj_base(nd) + rank;
                if (slot < 0 || slot >= (int32_t)b.order.size()) { outside++; continue; }
                const int32_t oi = b.order[(size_t)slot];
                seen[(size_t)oi]++;
                const ptbvh::Aabb bb = ptbvh::object_bounds(world[(size_t)oi]);
                for (int a = 0; a < 3; a++)
                    if (bvh_slot_lo(nd, a, s) > bb.lo[a] - margin * 0.999 || bvh_slot_hi(nd, a, s) < bb.hi[a] + margin * 0.999) { outside++; break; }
            }
        }
    }
    int bad = 0;
    for (int32_t i : finite)
        if (seen[(size_t)i] != 1) bad++;
    for (int v : visits)
        if (v != 1) bad++;
    const int largest = widest;
    if (b.stack_need >= PT_BVH_STACK) bad++;
    out[0] = (int32_t)b.nodes.size();
    out[1] = (int32_t)b.order.size();
    out[2] = b.depth;
    out[3] = largest;
    out[4] = bad;
    out[5] = outside;
    out[6] = nested;
    out[7] = planes;
    return PT_OK;
}

// Runs div_selftest_kernel on device 0 of the context: `millions` x 10^6 operand pairs; returns the number of pairs
// whose shared-reciprocal quotient differs from the IEEE division (must be 0), or a negative PT_ERR_* code.
int64_t pt_debug_div_selftest(pt_ctx *ctx, int32_t millions, uint64_t seed) {
    if (!ctx || millions <= 0) return -(int64_t)fail(PT_ERR_INVALID, "null context or no work");
    Device &d = ctx->devs[0];
    if (hipSetDevice(d.ordinal) != hipSuccess) return -(int64_t)fail(PT_ERR_HIP, "hipSetDevice");
    unsigned long long *out = nullptr;
    if (hipMalloc(reinterpret_cast<void **>(&out), 8) != hipSuccess) return -(int64_t)fail(PT_ERR_HIP, "hipMalloc");
    (void)hipMemsetAsync(out, 0, 8, d.own_stream);
    const uint32_t per_thread = 1000;
    const uint32_t blocks = (uint32_t)(((uint64_t)millions * 1000000ull + (uint64_t)per_thread * PT_BLOCK - 1) / ((uint64_t)per_thread * PT_BLOCK));
    hipLaunchKernelGGL(ptk::div_selftest_kernel, dim3(blocks), dim3(PT_BLOCK), 0, d.own_stream, (unsigned long long)seed, per_thread, out);
    unsigned long long bad = 0;
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, out, 8, hipMemcpyDeviceToHost, d.own_stream);
    if (e == hipSuccess) e = hipStreamSynchronize(d.own_stream);
    (void)hipFree(out);
    if (e != hipSuccess) return -(int64_t)fail(PT_ERR_HIP, std::string("div selftest: ") + hipGetErrorString(e));
    return (int64_t)bad;
}

int64_t pt_debug_scan_mismatches(pt_ctx *ctx) {
    (void)ctx;
    if (g_mismatches && std::getenv("PTCORE_VERBOSE")) {
        const unsigned long long *s = g_mismatch_sample;
        double v[8];
        for (int i = 0; i < 2; i++) std::memcpy(&v[i], &s[1 + i], 8);
        for (int i = 0; i < 6; i++) std::memcpy(&v[2 + i], &s[4 + i], 8);
        std::fprintf(stderr, "scan mismatch sample: culled best %d t %.17g | plain best %d t %.17g | mode %llu | o %.17g %.17g %.17g d %.17g %.17g %.17g\n",
                     (int)(s[0] >> 32), v[0], (int)(uint32_t)s[0], v[1], s[3], v[2], v[3], v[4], v[5], v[6], v[7]);
    }
    return (int64_t)g_mismatches;
}

int32_t pt_debug_set_primary_rays(pt_ctx *ctx, const double *rays, int64_t n) {
    if (!ctx) return fail(PT_ERR_INVALID, "ctx is null");
    if (n < 0) return fail(PT_ERR_INVALID, "pt_debug_set_primary_rays: n is negative");
    if (n > (int64_t)1 << 31) return fail(PT_ERR_INVALID, "pt_debug_set_primary_rays: more than 2^31 rays");
    if (ctx->frame.open) return fail(PT_ERR_STATE, "pt_debug_set_primary_rays while a frame is open");
    if (!rays || n == 0) {  // back to ray generation's own rays (the device copy is kept for a later table)
        ctx->inject_rays.clear();
        return PT_OK;
    }
    try {
        ctx->inject_rays.assign(rays, rays + 6 * (size_t)n);
    } catch (const std::bad_alloc &) {
        ctx->inject_rays.clear();
        return fail(PT_ERR_NOMEM, "pt_debug_set_primary_rays: out of host memory");
    }
    ctx->inject_gen++;
    return PT_OK;
}

int32_t pt_shard_tiles(int32_t width, int32_t height, const pt_shard *shard, int32_t *ntiles_local, int32_t *ntiles_x,
                       int32_t *ntiles_y) {
    if (width <= 0 || height <= 0) return fail(PT_ERR_INVALID, "width and height must be positive");
    pt_shard sh = shard ? *shard : pt_shard{0, 1};
    if (sh.count <= 0 || sh.index < 0 || sh.index >= sh.count) return fail(PT_ERR_INVALID, "bad shard");
    const int32_t ntx = (width + 31) / 32, nty = (height + 31) / 32;
    if (ntiles_x) *ntiles_x = ntx;
    if (ntiles_y) *ntiles_y = nty;
    if (ntiles_local) *ntiles_local = tiles_of_shard(ntx * nty, sh);
    return PT_OK;
}

int32_t pt_begin(pt_ctx *ctx, const pt_scene *scene, const pt_config *cfg) {
    if (!ctx) return fail(PT_ERR_INVALID, "ctx is null");
    if (int32_t rc = validate(scene, cfg)) return rc;
    if (ctx->frame.open) return fail(PT_ERR_STATE, "pt_begin: a frame is already open");
    if (ctx->adaptive_on) {  // refused before anything is launched; the context stays as it was
        if (ctx->shading_model != PT_SHADING_CPU) return fail(PT_ERR_STATE, "adaptive sampling: not available with GL shading (pt_set_shading)");
        if (!ctx->inject_rays.empty()) return fail(PT_ERR_STATE, "adaptive sampling: not available with injected primary rays (pt_debug_set_primary_rays)");
        if (ctx->pipeline == 1 || ctx->pipeline == 2)
            return fail(PT_ERR_STATE, "adaptive sampling: not available with PTCORE_PIPELINE=wavefront or walk32 (the default pipeline only)");
    }
    if (ctx->filtered_on && !ctx->adaptive_on)  // refused before anything is launched; the context stays as it was
        return fail(PT_ERR_INVALID, "pt_set_adaptive_filtered: the rule decides the blocks of an adaptive frame (pt_set_adaptive first)");
    const int32_t ndev = (int32_t)ctx->devs.size();
    const int32_t ntiles = ((cfg->width + 31) / 32) * ((cfg->height + 31) / 32);
    const uint32_t max_slots = (uint32_t)tiles_of_shard(ntiles, pt_shard{0, ndev}) * 1024u;
    if (int32_t rc = frame_open(ctx, scene, cfg, max_slots)) return rc;
    ctx->frame.adaptive = ctx->adaptive_on;
    ctx->frame.ad = ctx->adaptive;
    ctx->frame.filtered = ctx->filtered_on;
    ctx->frame.fa = ctx->filtered;
    ctx->frame.halves = ctx->halves_on || ctx->filtered_on;
    ctx->frame.moments = ctx->moments_on || ctx->adaptive_on || ctx->halves_on;
    if (ctx->features_k > 0) {  // refused before anything is launched; the context stays usable
        const bool bvh = ctx->frame.scan == ptk::SCAN_BVH || ctx->frame.scan == ptk::SCAN_VERIFY_BVH;
        const bool gl_feat = ctx->frame.gl && ctx->frame.gl_filter;  // pt_set_shading_features: GL's own features, on either GL kernel's path
        if (!gl_feat && ((bvh && !ctx->feature_walk_on) || ctx->frame.gl)) {
            ctx->frame.open = false;
            return fail(PT_ERR_INVALID, bvh ? "features: not available for scenes on the BVH path (more than 128 spheres or 128 boxes): a linear "
                                              "scan per feature sample"
                                            : "features: not available with GL shading (pt_set_shading), where a sample is a pass of 16 paths");
        }
        ctx->frame.features = ctx->features_k;
        ctx->frame.feature_walk = bvh && !gl_feat;  // (only with pt_set_feature_walk; the other scans ignore the setting)
    }
    if (ctx->object_ids_on) {
        if (ctx->frame.features <= 0) {  // refused before anything is launched; the context stays usable
            ctx->frame.open = false;
            return fail(PT_ERR_INVALID, "object ids: the frame needs features on (pt_set_features, k > 0): the id is the first hit of feature sample 0");
        }
        Frame &fr = ctx->frame;
        fr.object_ids = true;
        fr.scene_objects = scene->num_objects;
        fr.world_scene.clear();
        for (int32_t i = 0; i < scene->num_objects; i++) {  // scene_to_world's rule: unknown types have no object in the world
            const int32_t t = scene->objects[i].type;  // (GL's list is the scene's: an unknown type is a sphere there, the map the identity)
            if (fr.gl || t == PT_OBJ_SPHERE || t == PT_OBJ_SPHERE_LIGHT || t == PT_OBJ_PLANE || t == PT_OBJ_BOX) fr.world_scene.push_back(i);
        }
        if ((int32_t)fr.world_scene.size() != (fr.gl ? (int32_t)fr.gl_objs.size() : fr.nobj)) {
            fr.open = false;
            return fail(PT_ERR_INVALID, "object ids: the device world and the scene's object list disagree");
        }
    }
    for (int32_t i = 0; i < ndev; i++) {
        Device &d = ctx->devs[(size_t)i];
        int32_t rc = dev_begin(ctx, d, pt_shard{i, ndev}, nullptr);
        if (rc == PT_OK && ctx->frame.features > 0 && d.nlocal > 0) {  // outside PTCORE_L_BUDGET_MB, on the first frame that asks
            hipError_t e = hipSetDevice(d.ordinal);
            if (e == hipSuccess) e = d.feat.reserve(9 * (size_t)d.nslots);
            if (e != hipSuccess) rc = fail(e == hipErrorOutOfMemory ? PT_ERR_NOMEM : PT_ERR_HIP, std::string("features: ") + hipGetErrorString(e));
        }
        if (rc == PT_OK && ctx->frame.feature_walk && d.nlocal > 0) {  // the walk's counters, zeroed when the frame opens
            hipError_t e = hipSetDevice(d.ordinal);
            if (e == hipSuccess) e = d.walk_counters.reserve(4);
            if (e == hipSuccess) e = hipMemsetAsync(d.walk_counters.p, 0, 4 * sizeof(unsigned long long), d.stream);
            if (e != hipSuccess) rc = fail(e == hipErrorOutOfMemory ? PT_ERR_NOMEM : PT_ERR_HIP, std::string("feature walk: ") + hipGetErrorString(e));
        }
        if (rc == PT_OK && ctx->frame.object_ids && d.nlocal > 0) {  // outside PTCORE_L_BUDGET_MB, on the first frame that asks
            const std::vector<int32_t> &map = ctx->frame.world_scene;
            hipError_t e = hipSetDevice(d.ordinal);
            if (e == hipSuccess) e = d.obj_ids.reserve((size_t)d.nslots);
            if (e == hipSuccess) e = d.obj_map.reserve(std::max<size_t>(1, map.size()));
            if (e == hipSuccess && !map.empty()) e = hipMemcpyAsync(d.obj_map.p, map.data(), map.size() * sizeof(int32_t), hipMemcpyHostToDevice, d.stream);
            if (e != hipSuccess) rc = fail(e == hipErrorOutOfMemory ? PT_ERR_NOMEM : PT_ERR_HIP, std::string("object ids: ") + hipGetErrorString(e));
        }
        if (rc == PT_OK && ctx->frame.halves && d.nlocal > 0) {  // outside PTCORE_L_BUDGET_MB, on the first frame that asks
            hipError_t e = hipSetDevice(d.ordinal);
            if (e == hipSuccess) e = d.hv.reserve(12 * (size_t)d.nslots);
            if (e != hipSuccess) rc = fail(e == hipErrorOutOfMemory ? PT_ERR_NOMEM : PT_ERR_HIP, std::string("halves: ") + hipGetErrorString(e));
        }
        if (rc) {
            ctx->frame.open = false;
            return rc;
        }
    }
    return PT_OK;
}

int32_t pt_step(pt_ctx *ctx, int32_t nspp, int32_t *done_spp) {
    if (!ctx || !ctx->frame.open) return fail(PT_ERR_STATE, "pt_step without pt_begin");
    Frame &fr = ctx->frame;
    int32_t left = fr.cfg.samples_per_px - fr.done_spp;
    int32_t todo = std::max(0, std::min(nspp, left));
    if (fr.adaptive) {  // nothing is added once every block has stopped
        uint64_t nact = 0;
        for (const Device &d : ctx->devs) nact += d.nlocal ? d.nact : 0u;
        if (nact == 0) todo = 0;
    }
    const bool check = fr.adaptive && todo > 0;
    while (todo > 0) {
        const uint32_t S = std::min<uint32_t>((uint32_t)todo, fr.chunk);
        for (Device &d : ctx->devs)
            if (int32_t rc = dev_step(ctx, d, (uint32_t)fr.done_spp, S)) return rc;
        fr.done_spp += (int32_t)S;
        todo -= (int32_t)S;
    }
    std::vector<ptk::AdaptResult> res(check ? ctx->devs.size() : 0);
    if (check && fr.filtered) {  // ... by the pooled noise of the filtered frame
        if (int32_t rc = filtered_check(ctx, res.data())) return rc;
    } else if (check) {  // the blocks at or below the target leave the active lists
        for (size_t i = 0; i < ctx->devs.size(); i++)
            if (int32_t rc = dev_adaptive_check(ctx, ctx->devs[i], &res[i])) return rc;
    }
    for (Device &d : ctx->devs) {
        HIP_TRY(hipSetDevice(d.ordinal));
        HIP_TRY(hipStreamSynchronize(d.stream));
    }
    if (check) {
        fr.worst_active = 0.0;
        for (size_t i = 0; i < ctx->devs.size(); i++) {
            Device &d = ctx->devs[i];
            if (d.nlocal == 0 || d.nact == 0) continue;
            if (res[i].nact > d.nact) return fail(PT_ERR_STATE, "internal: the adaptive check returned a longer active list");
            d.nact = res[i].nact;
            d.act_cur ^= 1;
            if (d.nact) fr.worst_active = std::max(fr.worst_active, res[i].worst);
        }
    }
    if (done_spp) *done_spp = fr.done_spp;
    return PT_OK;
}

// the frame so far: rgba (always gathered; copied when asked for), the sums, the per-pixel counters
static int32_t read_frame(pt_ctx *ctx, uint8_t *rgba, int32_t stride, double *accum, uint32_t *nseg, uint32_t *ndraw) {
    Frame &fr = ctx->frame;
    if (int32_t rc = stride_fits(fr, rgba, stride)) return rc;
    const bool want_stats = fr.stats_on && (nseg || ndraw);
    const int32_t spp_done = fr.done_spp;
    const Plane planes[] = {
        {true, PLANE_RGBA, reserved<Device, &Device::tiles_rgba>, reserved<pt_ctx, &pt_ctx::g_tiles_rgba>, reserved<pt_ctx, &pt_ctx::f_rgba>, rgba, (size_t)stride},
        {accum != nullptr, PLANE_F64X3, reserved<Device, &Device::tiles_accum>, reserved<pt_ctx, &pt_ctx::g_tiles_accum>, reserved<pt_ctx, &pt_ctx::f_accum>, accum, 0},
        {want_stats, PLANE_U32A, reserved<Device, &Device::tiles_seg>, reserved<pt_ctx, &pt_ctx::g_tiles_seg>, reserved<pt_ctx, &pt_ctx::f_seg>, nseg, 0},
        {want_stats, PLANE_U32B, reserved<Device, &Device::tiles_draw>, reserved<pt_ctx, &pt_ctx::g_tiles_draw>, reserved<pt_ctx, &pt_ctx::f_draw>, ndraw, 0}};
    if (int32_t rc = gather_planes(ctx, planes, [&](Device &d, void *const *dst) {
            return dev_finish(ctx, d, spp_done, static_cast<uint8_t *>(dst[0]), static_cast<double *>(dst[1]), static_cast<uint32_t *>(dst[2]),
                              static_cast<uint32_t *>(dst[3]));
        }))
        return rc;
    if (ctx->rccl.lib) ctx->rccl.gathers++;
    return PT_OK;
}

int32_t pt_read(pt_ctx *ctx, uint8_t *rgba, int32_t stride, double *accum) {
    if (!ctx || !ctx->frame.open) return fail(PT_ERR_STATE, "pt_read without pt_begin");
    return read_frame(ctx, rgba, stride, accum, nullptr, nullptr);
}

int32_t pt_end(pt_ctx *ctx, pt_stats *stats) {
    if (!ctx || !ctx->frame.open) return fail(PT_ERR_STATE, "pt_end without pt_begin");
    pt_stats st;
    std::memset(&st, 0, sizeof st);
    int32_t rc = PT_OK;
    int slot = 0;
    for (Device &d : ctx->devs) {
        if (!d.first_recorded || d.nlocal == 0) { slot++; continue; }
        // make sure ev_last exists even if pt_read was never called
        if (hipSetDevice(d.ordinal) == hipSuccess) (void)hipEventRecord(d.ev_last, d.stream);
        if (int32_t r = dev_collect(d, &st, slot)) rc = r;
        slot++;
    }
    fill_stats_common(ctx, &st);
    ctx->frame.open = false;
    auto report = [&](EventKind kind, const char *what) {  // PTCORE_VERBOSE: the slowest device's time in the launches of one kind
        double worst = 0;
        size_t launches = 0;
        for (Device &d : ctx->devs) {
            double ms = 0;
            if (hipSetDevice(d.ordinal) == hipSuccess) (void)sum_ms(d.ev[kind], ms);
            worst = std::max(worst, ms);
            launches += d.ev[kind].n;
        }
        std::fprintf(stderr, "ptcore: %s %.3f ms in %zu launches%s (resolve_kernel %.3f ms in %d)\n", what, worst, launches,
                     kind != EV_CHECK ? "" : ctx->frame.filtered ? " of keep_from_map_kernel + compact_kernel" : " of block_noise_kernel + compact_kernel",
                     st.resolve_ms, st.resolve_launches);
    };
    if (ctx->frame.moments && rc == PT_OK && std::getenv("PTCORE_VERBOSE")) report(EV_MOMENTS, "moments_kernel");
    if (ctx->frame.adaptive && rc == PT_OK && std::getenv("PTCORE_VERBOSE")) report(EV_CHECK, "adaptive check");
    if (ctx->frame.features > 0 && rc == PT_OK && std::getenv("PTCORE_VERBOSE")) report(EV_FEATURE, ctx->frame.gl ? (ctx->frame.gl_walk ? "gl_feature_bvh_kernel" : "gl_feature_kernel") : ctx->frame.feature_walk ? "feature_bvh_kernel" : "feature_kernel");
    if (ctx->frame.halves && rc == PT_OK && std::getenv("PTCORE_VERBOSE")) report(EV_HALVES, "halves_kernel");
    if (ctx->frame.filtered && rc == PT_OK && std::getenv("PTCORE_VERBOSE")) report(EV_BLOCKS, "filtered block checks (gathers, pair filter, block map)");
    if (ctx->frame.fog_vol) {
        ctx->fog_pending = 1;
        if (int32_t r = collect_fog(ctx)) rc = rc != PT_OK ? rc : r;
    }
    if (ctx->frame.gl) {
        ctx->shading_pending = 1;
        if (int32_t r = collect_shading(ctx)) rc = rc != PT_OK ? rc : r;
    }
    if (stats) *stats = st;
    return rc;
}

int32_t pt_render(pt_ctx *ctx, const pt_scene *scene, const pt_config *cfg, uint8_t *rgba, int32_t stride, double *accum,
                  uint32_t *nseg, uint32_t *ndraw, pt_stats *stats) {
    if (!ctx) return fail(PT_ERR_INVALID, "ctx is null");
    if ((nseg || ndraw) && cfg && !(cfg->flags & PT_FLAG_PIXEL_STATS))
        return fail(PT_ERR_INVALID, "nseg/ndraw need PT_FLAG_PIXEL_STATS");
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    if (int32_t rc = pt_begin(ctx, scene, cfg)) return rc;
    const auto t1 = clk::now();
    int32_t rc = PT_OK;
    if (ctx->frame.adaptive) {  // `step` samples at a time, until the cap or until no block is active
        const int32_t step = std::max(1, ctx->frame.ad.step);
        for (int32_t done = 0, before = -1; rc == PT_OK && done < cfg->samples_per_px && done != before;) {
            before = done;
            rc = pt_step(ctx, step, &done);
        }
    } else {
        rc = pt_step(ctx, cfg->samples_per_px, nullptr);
    }
    const auto t2 = clk::now();
    if (rc == PT_OK) rc = read_frame(ctx, rgba, stride, accum, nseg, ndraw);
    const auto t3 = clk::now();
    pt_stats st;
    int32_t rc2 = pt_end(ctx, &st);
    if (std::getenv("PTCORE_VERBOSE")) {
        auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        std::fprintf(stderr, "ptcore: pt_render host phases: begin %.2f ms, step %.2f ms, read %.2f ms, end %.2f ms\n", ms(t0, t1), ms(t1, t2),
                     ms(t2, t3), ms(t3, clk::now()));
    }
    if (stats) *stats = st;
    return rc != PT_OK ? rc : rc2;
}

int32_t pt_set_moments(pt_ctx *ctx, int32_t on) {
    if (!ctx) return fail(PT_ERR_INVALID, "ctx is null");
    if (ctx->frame.open) return fail(PT_ERR_STATE, "pt_set_moments while a frame is open");
    ctx->moments_on = on != 0;
    return PT_OK;
}

int32_t pt_set_adaptive(pt_ctx *ctx, const pt_adaptive *a) {
    if (!ctx) return fail(PT_ERR_INVALID, "ctx is null");
    if (ctx->frame.open) return fail(PT_ERR_STATE, "pt_set_adaptive while a frame is open");
    if (a && !(a->target >= 0.0)) return fail(PT_ERR_INVALID, "pt_set_adaptive: target must be >= 0");
    if (a && a->min_spp < 0) return fail(PT_ERR_INVALID, "pt_set_adaptive: min_spp must be >= 0");
    ctx->adaptive_on = a != nullptr;
    if (a) ctx->adaptive = *a;
    else std::memset(&ctx->adaptive, 0, sizeof ctx->adaptive);
    return PT_OK;
}

int32_t pt_adaptive_state(pt_ctx *ctx, struct pt_adaptive_state *out) {
    if (!ctx || !out) return fail(PT_ERR_INVALID, "null argument");
    if (int32_t rc = frame_needs(ctx, "pt_adaptive_state", {NEED_MOMENTS, NEED_ADAPTIVE})) return rc;
    const Frame &fr = ctx->frame;
    struct pt_adaptive_state r;
    std::memset(&r, 0, sizeof r);
    r.spp_min = INT32_MAX;
    std::vector<uint32_t> spp;
    for (Device &d : ctx->devs) {
        if (d.nlocal == 0) continue;
        HIP_TRY(hipSetDevice(d.ordinal));
        spp.resize(d.nslots / 64u);
        HIP_TRY(hipMemcpyAsync(spp.data(), d.blk_spp.p, spp.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, d.stream));
        HIP_TRY(hipStreamSynchronize(d.stream));
        for (uint32_t blk = 0; blk < (uint32_t)spp.size(); blk++) {
            const uint32_t k = block_pixels(fr, d.shard, blk);
            if (k == 0) continue;
            r.blocks++;
            r.samples += (uint64_t)k * spp[blk];
            r.spp_min = std::min(r.spp_min, (int32_t)spp[blk]);
            r.spp_max = std::max(r.spp_max, (int32_t)spp[blk]);
        }
        r.active_blocks += d.nact;
    }
    if (r.blocks == 0) r.spp_min = 0;
    r.worst_active = r.active_blocks ? fr.worst_active : 0.0;
    *out = r;
    return PT_OK;
}

int32_t pt_read_sample_counts(pt_ctx *ctx, uint32_t *spp) {
    if (!ctx || !spp) return fail(PT_ERR_INVALID, "null argument");
    if (int32_t rc = frame_needs(ctx, "pt_read_sample_counts", {NEED_MOMENTS, NEED_ADAPTIVE})) return rc;
    return gather_one(ctx, g_counts, spp);
}

int32_t pt_read_moments(pt_ctx *ctx, double *m2) {
    if (!ctx || !m2) return fail(PT_ERR_INVALID, "null argument");
    if (int32_t rc = frame_needs(ctx, "pt_read_moments", {NEED_MOMENTS})) return rc;
    return gather_one(ctx, g_m2, m2);
}

int32_t pt_noise_estimate(pt_ctx *ctx, pt_noise *out) {
    if (!ctx || !out) return fail(PT_ERR_INVALID, "null argument");
    if (int32_t rc = frame_needs(ctx, "pt_noise_estimate", {NEED_MOMENTS})) return rc;
    const Frame &fr = ctx->frame;
    pt_noise r;
    std::memset(&r, 0, sizeof r);
    r.spp = fr.done_spp;
    r.pixels = (uint64_t)fr.cfg.width * (uint64_t)fr.cfg.height;
    if (fr.done_spp < 2) {  // no variance estimate from one sample
        r.noise = r.max_pixel = INFINITY;
        *out = r;
        return PT_OK;
    }
    double sum = 0.0;
    std::vector<ptk::NoisePartial> part;
    for (Device &d : ctx->devs) {  // partials in block order, devices in order
        if (d.nlocal == 0) continue;
        HIP_TRY(hipSetDevice(d.ordinal));
        const uint32_t grid = (d.nslots + PT_BLOCK - 1) / PT_BLOCK;
        HIP_TRY(d.noise_part.reserve(grid));
        ptk::NoiseArgs A;
        std::memset(&A, 0, sizeof A);
        A.acc = d.acc.p;
        A.m2 = d.m2.p;
        A.partial = d.noise_part.p;
        A.nslots = d.nslots;
        A.n = fr.done_spp;
        A.G = tile_geom(fr, d);
        // (adaptive: every slot of the shard too, each pixel with the n of its own block)
        if (int32_t rc = launch_pass(d, fr.adaptive, EV_KINDS, d.nslots, ptk::noise_kernel, ptk::noise_adaptive_kernel, d.blk_spp.p, A)) return rc;
        part.resize(grid);
        HIP_TRY(hipMemcpyAsync(part.data(), d.noise_part.p, grid * sizeof(ptk::NoisePartial), hipMemcpyDeviceToHost, d.stream));
        HIP_TRY(hipStreamSynchronize(d.stream));
        for (const ptk::NoisePartial &p : part) {
            sum += p.sum;
            r.max_pixel = std::max(r.max_pixel, p.max);
            r.bad_pixels += p.bad;
        }
    }
    r.noise = std::sqrt(sum / (double)r.pixels);
    *out = r;
    return PT_OK;
}

int32_t pt_set_features(pt_ctx *ctx, int32_t k) {
    if (!ctx) return fail(PT_ERR_INVALID, "ctx is null");
    if (ctx->frame.open) return fail(PT_ERR_STATE, "pt_set_features while a frame is open");
    if (k < 0) return fail(PT_ERR_INVALID, "pt_set_features: k must be >= 0");
    ctx->features_k = k;
    return PT_OK;
}

int32_t pt_set_feature_walk(pt_ctx *ctx, int32_t on) {
    if (!ctx) return fail(PT_ERR_INVALID, "ctx is null");
    if (ctx->frame.open) return fail(PT_ERR_STATE, "pt_set_feature_walk while a frame is open");
    ctx->feature_walk_on = on != 0;
    return PT_OK;
}

int32_t pt_feature_walk_stats(pt_ctx *ctx, uint64_t out[4]) {
    if (!ctx) return fail(PT_ERR_INVALID, "ctx is null");
    if (!out) return fail(PT_ERR_INVALID, "pt_feature_walk_stats: out is null");
    if (!ctx->frame.feature_walk)
        return fail(PT_ERR_STATE, "pt_feature_walk_stats: the last frame did not run the walk (pt_set_feature_walk and pt_set_features on a BVH scene)");
    uint64_t sum[4] = {0, 0, 0, 0};
    for (Device &d : ctx->devs) {
        if (d.nlocal == 0 || !d.walk_counters.p) continue;
        HIP_TRY(hipSetDevice(d.ordinal));
        HIP_TRY(hipStreamSynchronize(d.stream));
        unsigned long long c[4] = {};
        HIP_TRY(hipMemcpy(c, d.walk_counters.p, sizeof c, hipMemcpyDeviceToHost));
        for (int k = 0; k < 3; k++) sum[k] += c[k];
        sum[3] = std::max<uint64_t>(sum[3], c[3]);  // the deepest stack: the largest of the devices'
    }
    for (int k = 0; k < 4; k++) out[k] = sum[k];
    return PT_OK;
}

int32_t pt_set_fog_walk(pt_ctx *ctx, int32_t on) {
    if (!ctx) return fail(PT_ERR_INVALID, "ctx is null");
    if (ctx->frame.open) return fail(PT_ERR_STATE, "pt_set_fog_walk while a frame is open");
    ctx->fog_walk_on = on != 0;
    return PT_OK;
}

int32_t pt_fog_walk_stats(pt_ctx *ctx, uint64_t out[6]) {
    if (!ctx) return fail(PT_ERR_INVALID, "ctx is null");
    if (!out) return fail(PT_ERR_INVALID, "pt_fog_walk_stats: out is null");
    if (!ctx->frame.fog_walk)
        return fail(PT_ERR_STATE, "pt_fog_walk_stats: the last frame did not run the walk (pt_set_fog_walk and a gpu_volumetric fog block on a BVH scene)");
    uint64_t sum[6] = {0, 0, 0, 0, 0, 0};
    for (Device &d : ctx->devs) {
        if (d.nlocal == 0 || !d.fog_walk_counters.p) continue;
        HIP_TRY(hipSetDevice(d.ordinal));
        HIP_TRY(hipStreamSynchronize(d.stream));
        unsigned long long c[6] = {};
        HIP_TRY(hipMemcpy(c, d.fog_walk_counters.p, sizeof c, hipMemcpyDeviceToHost));
        for (int k = 0; k < 5; k++) sum[k] += c[k];
        sum[5] = std::max<uint64_t>(sum[5], c[5]);  // the deepest stack: the largest of the devices'
    }
    for (int k = 0; k < 6; k++) out[k] = sum[k];
    return PT_OK;
}

int32_t pt_set_shading_walk(pt_ctx *ctx, int32_t on) {
    if (!ctx) return fail(PT_ERR_INVALID, "ctx is null");
    if (ctx->frame.open) return fail(PT_ERR_STATE, "pt_set_shading_walk while a frame is open");
    ctx->shading_walk_on = on != 0;
    return PT_OK;
}

int32_t pt_set_shading_features(pt_ctx *ctx, int32_t on) {
    if (!ctx) return fail(PT_ERR_INVALID, "ctx is null");
    if (ctx->frame.open) return fail(PT_ERR_STATE, "pt_set_shading_features while a frame is open");
    ctx->shading_features_on = on != 0;
    return PT_OK;
}

int32_t pt_shading_walk_stats(pt_ctx *ctx, uint64_t out[7]) {
    if (!ctx) return fail(PT_ERR_INVALID, "ctx is null");
    if (!out) return fail(PT_ERR_INVALID, "pt_shading_walk_stats: out is null");
    if (!ctx->frame.gl_walk)
        return fail(PT_ERR_STATE, "pt_shading_walk_stats: the last frame did not run the walk (pt_set_shading_walk and GL shading on a BVH scene)");
    uint64_t sum[7] = {0, 0, 0, 0, 0, 0, 0};
    for (Device &d : ctx->devs) {
        if (d.nlocal == 0 || !d.gl_walk_counters.p) continue;
        HIP_TRY(hipSetDevice(d.ordinal));
        HIP_TRY(hipStreamSynchronize(d.stream));
        unsigned long long c[7] = {};
        HIP_TRY(hipMemcpy(c, d.gl_walk_counters.p, sizeof c, hipMemcpyDeviceToHost));
        for (int k = 0; k < 6; k++) sum[k] += c[k];
        sum[6] = std::max<uint64_t>(sum[6], c[6]);  // the deepest stack: the largest of the devices'
    }
    for (int k = 0; k < 7; k++) out[k] = sum[k];
    return PT_OK;
}

int32_t pt_set_bvh_refit(pt_ctx *ctx, double max_growth) {
    if (!ctx) return fail(PT_ERR_INVALID, "ctx is null");
    if (ctx->frame.open) return fail(PT_ERR_STATE, "pt_set_bvh_refit while a frame is open");
    if (!(max_growth == 0.0 || max_growth >= 1.0))  // (NaN compares false)
        return fail(PT_ERR_INVALID, "pt_set_bvh_refit: max_growth must be 0 (off), at least 1, or +inf");
    ctx->rf.max_growth = max_growth;
    return PT_OK;
}

int32_t pt_bvh_refit_stats(pt_ctx *ctx, struct pt_bvh_refit_stats *out) {
    if (!ctx) return fail(PT_ERR_INVALID, "ctx is null");
    if (!out) return fail(PT_ERR_INVALID, "pt_bvh_refit_stats: out is null");
    if (ctx->frames_opened == 0) return fail(PT_ERR_STATE, "pt_bvh_refit_stats before the first frame");
    *out = ctx->rf.st;
    return PT_OK;
}

int32_t pt_set_bvh_build(pt_ctx *ctx, int32_t mode) {
    if (!ctx) return fail(PT_ERR_INVALID, "ctx is null");
    if (ctx->frame.open) return fail(PT_ERR_STATE, "pt_set_bvh_build while a frame is open");
    if (mode != 0 && mode != 1) return fail(PT_ERR_INVALID, "pt_set_bvh_build: mode must be 0 (host) or 1 (device)");
    ctx->bb.mode = mode;
    return PT_OK;
}

int32_t pt_bvh_build_stats(pt_ctx *ctx, struct pt_bvh_build_stats *out) {
    if (!ctx) return fail(PT_ERR_INVALID, "ctx is null");
    if (!out) return fail(PT_ERR_INVALID, "pt_bvh_build_stats: out is null");
    if (ctx->frames_opened == 0) return fail(PT_ERR_STATE, "pt_bvh_build_stats before the first frame");
    *out = ctx->bb.st;
    return PT_OK;
}

// Host-only: the Morton-order build of `scene` by the host restatement (ptbvh::build_scene_trees_lbvh), checked the way
// pt_debug_bvh_check checks the host builder's tree.  out = {nodes, objects, depth, stack_need, objects not reached exactly once,
// objects not inside their slot's box, child boxes not inside their parent's, structural faults (children or objects not consecutive,
// a level table that does not increase, a node whose bytes a refit to the build's own world changes)}.
int32_t pt_debug_bvh_build_check(const pt_scene *scene, int32_t out[8]) {
    if (!scene || !out) return fail(PT_ERR_INVALID, "null argument");
    if (scene->num_materials < 0 || scene->num_objects < 0) return fail(PT_ERR_INVALID, "negative scene counts");
    std::vector<DevObj> w;
    std::vector<DevMat> m;
    scene_to_world(*scene, w, m);
    ptbvh::SceneTrees T;
    (void)ptbvh::build_scene_trees_lbvh(w, PT_BVH_STACK, T);
    ptbvh::check_trees(T, w, out);
    return PT_OK;
}

// Host-only: builds the hierarchy of `before` as a render would, refits it to `after` by the host restatement (ptbvh::refit) and
// checks the result.  Where `after` is not a refittable edit of `before` (out[2] says why) the checks run on a full build of `after`.
// out = {nodes, objects, 0 or the ptbvh::RefitReason, objects not inside their slot's box, child boxes not inside their parent's,
// nodes whose bytes differ from a fresh encode of the same topology, the figure ratio x 1000, nodes whose topology words changed}.
int32_t pt_debug_bvh_refit_check(const pt_scene *before, const pt_scene *after, int32_t out[8]) {
    if (!before || !after || !out) return fail(PT_ERR_INVALID, "null argument");
    for (const pt_scene *s : {before, after})
        if (s->num_materials < 0 || s->num_objects < 0) return fail(PT_ERR_INVALID, "negative scene counts");
    std::vector<DevObj> w0, w1;
    std::vector<DevMat> m0, m1;
    scene_to_world(*before, w0, m0);
    scene_to_world(*after, w1, m1);
    const int reason = ptbvh::refit_reason(w0, m0, w1, m1);
    ptbvh::SceneTrees T;
    if (!ptbvh::build_scene_trees(reason == ptbvh::REFIT_OK ? w0 : w1, false, PT_BVH_STACK, T))
        return fail(PT_ERR_INVALID, "BVH deeper than the traversal stack");
    std::vector<double> box, area;
    ptbvh::refit(T.nodes, T.objs, reason == ptbvh::REFIT_OK ? w0 : w1, T.margin, T.level_start, box, area);
    const double cost0 = ptrf::cost_of(area.data(), (size_t)T.main_nodes);
    const std::vector<BvhNode> built = T.nodes;
    const double margin = ptbvh::scene_margin(w1);
    ptbvh::refit(T.nodes, T.objs, w1, margin, T.level_start, box, area);
    const double cost1 = ptrf::cost_of(area.data(), (size_t)T.main_nodes);
    int outside = 0, nested = 0, differ = 0, topo = 0;
    const double held = std::isfinite(margin) ? margin * 0.999 : 0.0;  // (an infinite margin: the slabs constrain nothing)
    // a fresh encode of the same topology: every node's subtree box gathered top-down from the objects, not level by level
    std::vector<ptrf::Box> sub(T.nodes.size());
    for (size_t q = T.nodes.size(); q-- > 0;) {  // (children carry larger numbers than their parents)
        const BvhNode &nd = T.nodes[q];
        BvhNode fresh = built[q];
        ptrf::Box all = ptrf::empty_box();
        for (int s = 0; s < 4; s++) {
            const int rank = ptrf::slot_rank(nd.meta, s);
            ptrf::Box b;
            if (ptrf::slot_object(nd.meta, s)) b = ptrf::object_box(w1[(size_t)T.objs[(size_t)(nd.obj_base + rank)].index]);
            else if (ptrf::slot_internal(nd.meta, s)) b = sub[(size_t)(nd.node_base + rank)];
            else continue;
            ptrf::grow(all, b);
            ptrf::encode_slot(fresh, s, b, margin);
            for (int k = 0; k < 3; k++) {
                const double slo = bvh_slot_lo(nd, k, s), shi = bvh_slot_hi(nd, k, s);
                if (ptrf::slot_object(nd.meta, s)) {
                    if (slo > b.lo[k] - held || shi < b.hi[k] + held) { outside++; break; }
                } else if (slo > b.lo[k] - held || shi < b.hi[k] + held) {  // the child's content, by the margin
                    nested++;
                    break;
                }
            }
        }
        sub[q] = all;
        if (std::memcmp(&fresh, &nd, sizeof(BvhNode)) != 0) differ++;
        if (nd.node_base != built[q].node_base || nd.obj_base != built[q].obj_base || nd.meta != built[q].meta ||
            std::memcmp(nd.pad, built[q].pad, sizeof nd.pad) != 0)
            topo++;
        for (int k = 0; k < 3; k++)
            for (int s = 0; s < 4; s++)
                if ((ptrf::float_bits(nd.h[k][s]) ^ ptrf::float_bits(built[q].h[k][s])) & 0xffu) { topo++; k = 3; break; }
    }
    for (size_t k = 0; k < T.objs.size(); k++)
        if (std::memcmp(&T.objs[k].o, &w1[(size_t)T.objs[k].index], sizeof(DevObj)) != 0) differ++;
    out[0] = (int32_t)T.nodes.size();
    out[1] = (int32_t)T.objs.size();
    out[2] = reason;
    out[3] = outside;
    out[4] = nested;
    out[5] = differ;
    out[6] = cost0 > 0.0 ? (int32_t)std::min(2.0e9, cost1 / cost0 * 1000.0) : 0;
    out[7] = topo;
    return PT_OK;
}

int32_t pt_read_features(pt_ctx *ctx, double *normal, double *albedo, double *depth) {
    if (!ctx) return fail(PT_ERR_INVALID, "ctx is null");
    if (int32_t rc = frame_needs(ctx, "pt_read_features", {NEED_MOMENTS, NEED_FEATURES})) return rc;
    double *const host[3] = {normal, albedo, depth};
    for (uint32_t k = 0; k < 3u; k++)
        if (host[k])
            if (int32_t rc = gather_one(ctx, g_feature[k], host[k])) return rc;
    return PT_OK;
}

int32_t pt_set_object_ids(pt_ctx *ctx, int32_t on) {
    if (!ctx) return fail(PT_ERR_INVALID, "ctx is null");
    if (ctx->frame.open) return fail(PT_ERR_STATE, "pt_set_object_ids while a frame is open");
    ctx->object_ids_on = on != 0;
    return PT_OK;
}

int32_t pt_read_object_ids(pt_ctx *ctx, int32_t *ids) {
    if (!ctx) return fail(PT_ERR_INVALID, "ctx is null");
    if (!ids) return fail(PT_ERR_INVALID, "pt_read_object_ids: ids is null");
    if (int32_t rc = frame_needs(ctx, "pt_read_object_ids", {NEED_MOMENTS, NEED_FEATURES})) return rc;
    if (!ctx->frame.object_ids) return fail(PT_ERR_STATE, "pt_read_object_ids: the frame was rendered with object ids off (pt_set_object_ids)");
    return gather_one(ctx, g_ids, ids);
}

int32_t pt_atrous(pt_ctx *ctx, const pt_atrous_config *cfg, uint8_t *rgba, int32_t stride, double *mean, double *var, pt_atrous_stats *stats) {
    if (!ctx) return fail(PT_ERR_INVALID, "ctx is null");
    pt_atrous_config c;
    if (int32_t rc = filter_config("pt_atrous", "", cfg, 5, c)) return rc;
    if (int32_t rc = frame_needs(ctx, "pt_atrous", {NEED_MOMENTS, NEED_NOT_GL, NEED_2_SAMPLES})) return rc;
    Frame &fr = ctx->frame;
    if (int32_t rc = stride_fits(fr, rgba, stride)) return rc;
    const int32_t W = fr.cfg.width, H = fr.cfg.height;
    FilterClock<2> clock;
    if (int32_t rc = gather_filter_inputs(ctx, false)) return rc;
    const bool feat = fr.features > 0;
    Device &d0 = ctx->devs[0];
    pt_ctx::Atrous &B = ctx->at;
    HIP_TRY(hipSetDevice(d0.ordinal));
    const size_t npix = (size_t)W * (size_t)H;
    const uint32_t grid1 = ptl::grid_1d(npix);
    if (int32_t rc = reserve_filter(ctx, npix)) return rc;
    if (int32_t rc = clock.create()) return rc;
    HIP_TRY(hipEventRecord(clock.ev[0], d0.stream));
    ptk::AtrousPrepArgs PA;
    std::memset(&PA, 0, sizeof PA);
    PA.acc = ctx->f_accum.p;
    PA.m2 = ctx->f_m2.p;
    PA.cnt = fr.adaptive ? ctx->f_seg.p : nullptr;
    PA.fn = feat ? ctx->f_feat_n.p : nullptr;
    PA.fa = feat ? ctx->f_feat_a.p : nullptr;
    PA.fd = feat ? ctx->f_feat_d.p : nullptr;
    PA.col = B.col[0].p;
    PA.var = B.var[0].p;
    PA.guide = B.guide.p;
    PA.npix = (uint32_t)npix;
    PA.n = (uint32_t)fr.done_spp;
    hipLaunchKernelGGL(ptk::atrous_prep_kernel, dim3(grid1), dim3(PT_BLOCK), 0, d0.stream, PA);
    double *const col[2] = {B.col[0].p, B.col[1].p}, *const vr[2] = {B.var[0].p, B.var[1].p};
    const pta::Params P = ptl::filter_params(c, feat);
    const int cur = ptl::filter_sequence(&P, col, vr, B.guide.p, B.part.p, ctx->f_rgba.p, W, H, d0.stream, fr.gl);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(clock.ev[1], d0.stream));
    std::vector<ptk::NoisePartial> part(2 * (size_t)grid1);
    HIP_TRY(hipMemcpyAsync(part.data(), B.part.p, part.size() * sizeof(ptk::NoisePartial), hipMemcpyDeviceToHost, d0.stream));
    if (int32_t rc = copy_filtered(ctx, cur, rgba, stride, mean, var)) return rc;
    HIP_TRY(hipStreamSynchronize(d0.stream));
    if (stats) {
        pt_atrous_stats st;
        std::memset(&st, 0, sizeof st);
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, clock.ev[0], clock.ev[1]));
        st.atrous_ms = ms;
        st.launches = c.iterations + 4;
        st.iterations = c.iterations;
        const ptl::NoiseFigures f = ptl::noise_figures(part.data(), grid1, true, npix);
        st.bad_pixels = f.bad;
        st.noise_before = f.before;
        st.noise_after = f.after;
        *stats = st;
    }
    if (std::getenv("PTCORE_VERBOSE"))
        std::fprintf(stderr, "ptcore: pt_atrous %d iterations, %.3f ms host wall (gathers included)\n", c.iterations, clock.wall_ms());
    return PT_OK;
}

int32_t pt_temporal(pt_ctx *ctx, const pt_temporal_config *cfg, const pt_atrous_config *filter, uint8_t *rgba, int32_t stride, double *mean,
                    double *var, pt_temporal_stats *stats) {
    if (!ctx) return fail(PT_ERR_INVALID, "ctx is null");
    pt_temporal_config c = {0.2, 0.1, 0.9, 0.05, 32, 0};
    if (cfg) c = *cfg;
    if (!(c.alpha >= 0.0 && c.alpha <= 1.0) || !(c.tol_z >= 0.0) || !(c.tol_a >= 0.0) || c.n_min != c.n_min || c.max_len < 1)
        return fail(PT_ERR_INVALID, "pt_temporal: alpha must be 0..1, tol_z and tol_a >= 0, n_min a number, max_len >= 1");
    pt_atrous_config f;
    if (int32_t rc = filter_config("pt_temporal", "filter ", filter, 0, f)) return rc;
    if (int32_t rc = frame_needs(ctx, "pt_temporal", {NEED_MOMENTS})) return rc;
    Frame &fr = ctx->frame;
    pt_ctx::Temporal &T = ctx->tp;
    if (int32_t rc = stride_fits(fr, rgba, stride)) return rc;
    if (int32_t rc = frame_needs(ctx, "pt_temporal", {NEED_CPU_CAMERA, NEED_FEATURES, NEED_2_SAMPLES})) return rc;
    if (T.serial == fr.serial && T.spp == fr.done_spp)
        return fail(PT_ERR_STATE, "pt_temporal: already accumulated (this frame, at this number of samples, is in the history)");
    const int32_t motion_n = T.motion_n;  // step 4a's table, pending since pt_temporal_set_motion
    if (motion_n > 0) {
        if (!fr.object_ids) return fail(PT_ERR_STATE, "pt_temporal: a motion table is pending and the frame was rendered with object ids off (pt_set_object_ids)");
        if (motion_n != fr.scene_objects)
            return fail(PT_ERR_INVALID, "pt_temporal: the pending motion table has " + std::to_string(motion_n) + " objects, the frame's scene " +
                                            std::to_string(fr.scene_objects));
    }
    const int32_t W = fr.cfg.width, H = fr.cfg.height;
    FilterClock<3> clock;  // events: first launch, last launch complete, temporal_kernel complete
    if (int32_t rc = gather_filter_inputs(ctx, false)) return rc;
    if (motion_n > 0)
        if (int32_t rc = gather_one(ctx, g_ids, nullptr)) return rc;
    Device &d0 = ctx->devs[0];
    pt_ctx::Atrous &B = ctx->at;
    HIP_TRY(hipSetDevice(d0.ordinal));
    const size_t npix = (size_t)W * (size_t)H;
    const uint32_t grid1 = ptl::grid_1d(npix);
    const dim3 grid2 = ptl::grid_2d(W, H);
    const size_t nblk = (size_t)grid2.x * grid2.y;
    const bool have = T.valid && T.w == W && T.h == H;  // another size: the history is dropped (when the call succeeds)
    // Both sets are kept at the size of this frame.  A set that has to grow loses its contents, which is what a change of size means;
    // a smaller frame after a larger one keeps the memory and is caught by `have`.
    for (int k = 0; k < 2; k++) {
        if (T.hist[k].cap < (size_t)PTT_PLANES * npix) T.valid = false;
        if (hipError_t e = T.hist[k].reserve((size_t)PTT_PLANES * npix); e != hipSuccess)
            return fail(e == hipErrorOutOfMemory ? PT_ERR_NOMEM : PT_ERR_HIP, std::string("pt_temporal: history: ") + hipGetErrorString(e));
    }
    HIP_TRY(T.part.reserve(nblk));
    if (motion_n > 0) {
        HIP_TRY(T.delta.reserve(3 * (size_t)motion_n));
        HIP_TRY(hipMemcpyAsync(T.delta.p, T.motion.data(), 3 * (size_t)motion_n * sizeof(double), hipMemcpyHostToDevice, d0.stream));
    }
    if (int32_t rc = reserve_filter(ctx, npix)) return rc;
    if (int32_t rc = clock.create()) return rc;
    const int next = T.cur ^ 1;  // a failed call leaves the stored history untouched: the kernel writes the other set
    HIP_TRY(hipEventRecord(clock.ev[0], d0.stream));
    ptk::TemporalArgs TA;
    std::memset(&TA, 0, sizeof TA);
    TA.C.alpha = c.alpha; TA.C.tol_z = c.tol_z; TA.C.n_min = c.n_min; TA.C.tol_a = c.tol_a;
    TA.C.max_len = c.max_len;
    TA.C.have_history = have ? 1 : 0;
    TA.C.clip_gamma = T.clip;
    TA.V.cam = fr.cam;
    TA.V.inv_width = fr.F.inv_width;
    TA.V.inv_height = fr.F.inv_height;
    TA.V.W = W;
    TA.V.H = H;
    TA.cam_h = T.cam;
    TA.acc = ctx->f_accum.p;
    TA.m2 = ctx->f_m2.p;
    TA.cnt = fr.adaptive ? ctx->f_seg.p : nullptr;
    TA.fn = ctx->f_feat_n.p;
    TA.fa = ctx->f_feat_a.p;
    TA.fd = ctx->f_feat_d.p;
    TA.hist = T.hist[T.cur].p;
    TA.hist_out = T.hist[next].p;
    TA.col = B.col[0].p;
    TA.var = B.var[0].p;
    TA.guide = B.guide.p;
    TA.partial = T.part.p;
    TA.n = (uint32_t)fr.done_spp;
    if (motion_n > 0) {
        TA.ids = reinterpret_cast<const int32_t *>(ctx->f_ids.p);
        TA.delta = T.delta.p;
        TA.ndelta = motion_n;
    }
    hipLaunchKernelGGL(ptk::temporal_kernel, grid2, dim3(PT_BLOCK), 0, d0.stream, TA);
    HIP_TRY(hipEventRecord(clock.ev[2], d0.stream));
    double *const col[2] = {B.col[0].p, B.col[1].p}, *const vr[2] = {B.var[0].p, B.var[1].p};
    const pta::Params P = ptl::filter_params(f, true);
    const int cur = ptl::filter_sequence(filter ? &P : nullptr, col, vr, B.guide.p, B.part.p, ctx->f_rgba.p, W, H, d0.stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(clock.ev[1], d0.stream));
    std::vector<ptk::NoisePartial> part(2 * (size_t)grid1);
    std::vector<ptk::TemporalPartial> tpart(nblk);
    HIP_TRY(hipMemcpyAsync(part.data(), B.part.p, (filter ? 2 : 1) * (size_t)grid1 * sizeof(ptk::NoisePartial), hipMemcpyDeviceToHost, d0.stream));
    HIP_TRY(hipMemcpyAsync(tpart.data(), T.part.p, nblk * sizeof(ptk::TemporalPartial), hipMemcpyDeviceToHost, d0.stream));
    if (int32_t rc = copy_filtered(ctx, cur, rgba, stride, mean, var)) return rc;
    HIP_TRY(hipStreamSynchronize(d0.stream));
    float kernel_ms = 0;
    HIP_TRY(hipEventElapsedTime(&kernel_ms, clock.ev[0], clock.ev[2]));
    const ptl::TemporalFigures tf = ptl::temporal_figures(tpart.data(), nblk, npix);
    if (stats) {
        pt_temporal_stats st;
        std::memset(&st, 0, sizeof st);
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, clock.ev[0], clock.ev[1]));
        st.temporal_ms = ms;
        st.iterations = filter ? f.iterations : 0;
        st.launches = filter ? f.iterations + 4 : 3;
        const ptl::NoiseFigures nf = ptl::noise_figures(part.data(), grid1, filter != nullptr, npix);
        st.reprojected = tf.reprojected;
        st.disoccluded = tf.disoccluded;
        st.bad_pixels = nf.bad;
        st.mean_len = (double)tf.len_sum / (double)npix;
        st.noise_before = tf.noise_before;
        st.noise_blended = nf.before;
        st.noise_after = nf.after;
        *stats = st;
    }
    T.cur = next;
    T.valid = true;
    T.w = W;
    T.h = H;
    T.cam = fr.cam;
    T.serial = fr.serial;
    T.spp = fr.done_spp;
    T.clip_stats = {T.clip, tf.clipped, tf.reprojected};
    T.motion_stats = {motion_n, 0, tf.moved, tf.moved_reprojected};
    T.motion.clear();  // one-shot: consumed, also when the history was empty
    T.motion_n = 0;
    if (std::getenv("PTCORE_VERBOSE"))
        std::fprintf(stderr,
                     "ptcore: pt_temporal %d filter iterations, clip gamma %g: clipped %llu of %llu reprojected, temporal_kernel %.3f ms, "
                     "%.3f ms host wall (gathers included)\n",
                     filter ? f.iterations : 0, T.clip, (unsigned long long)tf.clipped, (unsigned long long)tf.reprojected, kernel_ms,
                     clock.wall_ms());
    return PT_OK;
}

int32_t pt_temporal_set_clip(pt_ctx *ctx, double gamma) {
    if (!ctx) return fail(PT_ERR_INVALID, "ctx is null");
    if (!(gamma >= 0.0) || std::isinf(gamma)) return fail(PT_ERR_INVALID, "pt_temporal_set_clip: gamma must be a finite number >= 0 (0 = off)");
    ctx->tp.clip = gamma;
    return PT_OK;
}

int32_t pt_temporal_clip_stats(pt_ctx *ctx, struct pt_temporal_clip_stats *out) {
    if (!ctx) return fail(PT_ERR_INVALID, "ctx is null");
    if (!out) return fail(PT_ERR_INVALID, "pt_temporal_clip_stats: out is null");
    if (!ctx->tp.valid) return fail(PT_ERR_STATE, "pt_temporal_clip_stats: the history is empty (pt_temporal first)");
    *out = ctx->tp.clip_stats;
    return PT_OK;
}

int32_t pt_temporal_set_motion(pt_ctx *ctx, const double *delta, int32_t num_objects) {
    if (!ctx) return fail(PT_ERR_INVALID, "ctx is null");
    if (num_objects < 0) return fail(PT_ERR_INVALID, "pt_temporal_set_motion: num_objects must be >= 0");
    if (!delta || num_objects == 0) {
        ctx->tp.motion.clear();
        ctx->tp.motion_n = 0;
        return PT_OK;
    }
    for (size_t i = 0; i < 3 * (size_t)num_objects; i++)
        if (!std::isfinite(delta[i])) return fail(PT_ERR_INVALID, "pt_temporal_set_motion: every delta must be a finite number");
    try {  // (a copy first: a table that cannot be held leaves the pending one as it was)
        std::vector<double> table(delta, delta + 3 * (size_t)num_objects);
        ctx->tp.motion.swap(table);
    } catch (const std::bad_alloc &) {
        return fail(PT_ERR_NOMEM, "pt_temporal_set_motion: out of host memory");
    }
    ctx->tp.motion_n = num_objects;
    return PT_OK;
}

int32_t pt_temporal_motion_stats(pt_ctx *ctx, struct pt_temporal_motion_stats *out) {
    if (!ctx) return fail(PT_ERR_INVALID, "ctx is null");
    if (!out) return fail(PT_ERR_INVALID, "pt_temporal_motion_stats: out is null");
    if (!ctx->tp.valid) return fail(PT_ERR_STATE, "pt_temporal_motion_stats: the history is empty (pt_temporal first)");
    *out = ctx->tp.motion_stats;
    return PT_OK;
}

int32_t pt_temporal_read(pt_ctx *ctx, double *mean, double *var, int32_t *len) {
    if (!ctx) return fail(PT_ERR_INVALID, "ctx is null");
    if (!ctx->tp.valid) return fail(PT_ERR_STATE, "pt_temporal_read: the history is empty (pt_temporal first)");
    const size_t np = (size_t)ctx->tp.w * (size_t)ctx->tp.h;
    Device &d0 = ctx->devs[0];
    HIP_TRY(hipSetDevice(d0.ordinal));
    std::vector<double> h((size_t)PTT_PLANES * np);
    HIP_TRY(hipMemcpyAsync(h.data(), ctx->tp.hist[ctx->tp.cur].p, h.size() * sizeof(double), hipMemcpyDeviceToHost, d0.stream));
    HIP_TRY(hipStreamSynchronize(d0.stream));
    for (size_t i = 0; i < np; i++) {
        if (mean)
            for (size_t k = 0; k < 3; k++) mean[3 * i + k] = h[k * np + i];
        if (var) var[i] = h[(size_t)PTT_VAR * np + i];
        if (len) std::memcpy(&len[i], reinterpret_cast<const char *>(&h[(size_t)PTT_LH * np]) + 8 * i, sizeof(int32_t));
    }
    return PT_OK;
}

int32_t pt_temporal_reset(pt_ctx *ctx) {
    if (!ctx) return fail(PT_ERR_INVALID, "ctx is null");
    ctx->tp.valid = false;
    ctx->tp.serial = 0;
    ctx->tp.motion.clear();  // a table describes a move since the history that is now gone
    ctx->tp.motion_n = 0;
    return PT_OK;
}

int32_t pt_set_halves(pt_ctx *ctx, int32_t on) {
    if (!ctx) return fail(PT_ERR_INVALID, "ctx is null");
    if (ctx->frame.open) return fail(PT_ERR_STATE, "pt_set_halves while a frame is open");
    ctx->halves_on = on != 0;
    return PT_OK;
}

int32_t pt_read_halves(pt_ctx *ctx, double *sa, double *qa, double *sb, double *qb) {
    if (!ctx) return fail(PT_ERR_INVALID, "ctx is null");
    if (int32_t rc = frame_needs(ctx, "pt_read_halves", {NEED_MOMENTS, NEED_HALVES})) return rc;
    double *const host[4] = {sa, qa, sb, qb};
    for (uint32_t k = 0; k < 4u; k++)
        if (host[k])
            if (int32_t rc = gather_one(ctx, g_half[k], host[k])) return rc;
    return PT_OK;
}

int32_t pt_atrous_halves(pt_ctx *ctx, const pt_atrous_config *cfg, double *mean, double *err, double *half_means, pt_halves_stats *stats) {
    if (!ctx) return fail(PT_ERR_INVALID, "ctx is null");
    pt_atrous_config c;
    if (int32_t rc = filter_config("pt_atrous_halves", "", cfg, 5, c)) return rc;
    if (int32_t rc = frame_needs(ctx, "pt_atrous_halves", {NEED_MOMENTS, NEED_HALVES, NEED_NOT_GL})) return rc;
    Frame &fr = ctx->frame;
    int32_t spp_min = fr.done_spp;  // the smallest count the frame holds: every half needs two samples for its variance
    if (fr.adaptive) {
        struct pt_adaptive_state as;
        if (int32_t rc = pt_adaptive_state(ctx, &as)) return rc;
        spp_min = as.spp_min;
    }
    if (spp_min < 4)
        return fail(PT_ERR_STATE, "pt_atrous_halves: every pixel needs at least 4 samples (the frame's smallest count is " + std::to_string(spp_min) + ")");
    const int32_t W = fr.cfg.width, H = fr.cfg.height;
    FilterClock<2> clock;
    if (int32_t rc = halves_filter(ctx, c, half_means != nullptr, &clock)) return rc;
    Device &d0 = ctx->devs[0];
    pt_ctx::Halves &B = ctx->ah;
    const size_t npix = (size_t)W * (size_t)H;
    const uint32_t grid1 = ptl::grid_1d(npix);
    std::vector<ptk::HalvesPartial> part(grid1);
    HIP_TRY(hipMemcpyAsync(part.data(), B.part.p, part.size() * sizeof(ptk::HalvesPartial), hipMemcpyDeviceToHost, d0.stream));
    if (mean) HIP_TRY(hipMemcpyAsync(mean, B.mean.p, 3 * npix * sizeof(double), hipMemcpyDeviceToHost, d0.stream));
    if (err) HIP_TRY(hipMemcpyAsync(err, B.err.p, npix * sizeof(double), hipMemcpyDeviceToHost, d0.stream));
    if (half_means) HIP_TRY(hipMemcpyAsync(half_means, B.half.p, 6 * npix * sizeof(double), hipMemcpyDeviceToHost, d0.stream));
    HIP_TRY(hipStreamSynchronize(d0.stream));
    if (stats) {
        pt_halves_stats st;
        std::memset(&st, 0, sizeof st);
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, clock.ev[0], clock.ev[1]));
        st.atrous_ms = ms;
        st.launches = c.iterations + 2;
        st.iterations = c.iterations;
        st.spp_min = spp_min;
        const ptl::HalvesFigures f = ptl::halves_figures(part.data(), grid1, npix);
        st.bad_pixels = f.bad;
        st.noise = f.noise;
        st.noise_model = f.noise_model;
        *stats = st;
    }
    if (std::getenv("PTCORE_VERBOSE"))
        std::fprintf(stderr, "ptcore: pt_atrous_halves %d iterations, %.3f ms host wall (gathers included)\n", c.iterations, clock.wall_ms());
    return PT_OK;
}

int32_t pt_set_adaptive_filtered(pt_ctx *ctx, const pt_adaptive_filtered *f) {
    if (!ctx) return fail(PT_ERR_INVALID, "ctx is null");
    if (ctx->frame.open) return fail(PT_ERR_STATE, "pt_set_adaptive_filtered while a frame is open");
    pt_adaptive_filtered r;
    std::memset(&r, 0, sizeof r);
    if (f) {
        if (int32_t rc = filter_config("pt_set_adaptive_filtered", "filter ", &f->filter, 5, r.filter)) return rc;
        if (f->pool < 0 || f->pool > PTA_MAX_POOL) return fail(PT_ERR_INVALID, "pt_set_adaptive_filtered: pool must be 0..4");
        r.pool = f->pool;
    }
    ctx->filtered_on = f != nullptr;
    ctx->filtered = r;
    return PT_OK;
}

int32_t pt_read_block_figures(pt_ctx *ctx, double *pooled, double *own, int32_t *checks) {
    if (!ctx) return fail(PT_ERR_INVALID, "ctx is null");
    if (int32_t rc = frame_needs(ctx, "pt_read_block_figures", {NEED_MOMENTS, NEED_ADAPTIVE})) return rc;
    const Frame &fr = ctx->frame;
    if (!fr.filtered) return fail(PT_ERR_STATE, "pt_read_block_figures: the frame was rendered with the rule off (pt_set_adaptive_filtered)");
    if (fr.fa_checks <= 0) return fail(PT_ERR_STATE, "pt_read_block_figures: no check of the frame has decided yet");
    const size_t nb = (size_t)ptl::blocks_across(fr.cfg.width) * (size_t)ptl::blocks_across(fr.cfg.height);
    if (pooled) std::memcpy(pooled, ctx->bf.h_pooled.data(), nb * sizeof(double));
    if (own) std::memcpy(own, ctx->bf.h_own.data(), nb * sizeof(double));
    if (checks) *checks = fr.fa_checks;
    return PT_OK;
}

int32_t pt_render_tiles_device(pt_ctx *ctx, const pt_scene *scene, const pt_config *cfg, const pt_shard *shard,
                               void *d_tiles_rgba, void *d_tiles_accum, void *stream, pt_stats *stats) {
    if (!ctx) return fail(PT_ERR_INVALID, "ctx is null");
    if (int32_t rc = validate(scene, cfg)) return rc;
    if (ctx->frame.open) return fail(PT_ERR_STATE, "a frame is already open");
    if (!d_tiles_rgba) return fail(PT_ERR_INVALID, "d_tiles_rgba is null");
    pt_shard sh = shard ? *shard : pt_shard{0, 1};
    if (sh.count <= 0 || sh.index < 0 || sh.index >= sh.count) return fail(PT_ERR_INVALID, "bad shard");
    if (cfg->flags & PT_FLAG_PIXEL_STATS) return fail(PT_ERR_INVALID, "pixel stats are not available on the device entry point");
    const int32_t ntiles = ((cfg->width + 31) / 32) * ((cfg->height + 31) / 32);
    const uint32_t slots = (uint32_t)tiles_of_shard(ntiles, sh) * 1024u;
    if (int32_t rc = frame_open(ctx, scene, cfg, slots)) return rc;
    Frame &fr = ctx->frame;
    Device &d = ctx->devs[0];
    int32_t rc = dev_begin(ctx, d, sh, static_cast<hipStream_t>(stream));
    for (int32_t s = 0; rc == PT_OK && s < cfg->samples_per_px;) {
        const uint32_t S = std::min<uint32_t>((uint32_t)(cfg->samples_per_px - s), fr.chunk);
        rc = dev_step(ctx, d, (uint32_t)s, S);
        s += (int32_t)S;
    }
    fr.done_spp = cfg->samples_per_px;
    if (rc == PT_OK)
        rc = dev_finish(ctx, d, cfg->samples_per_px, static_cast<uint8_t *>(d_tiles_rgba), static_cast<double *>(d_tiles_accum),
                        nullptr, nullptr);
    if (rc == PT_OK && fr.fog_vol) ctx->fog_pending = 2;  // collected now with stats, else when pt_fog_last_stats asks
    if (rc == PT_OK && fr.gl) ctx->shading_pending = 2;
    if (rc == PT_OK && stats) {
        pt_stats st;
        std::memset(&st, 0, sizeof st);
        rc = dev_collect(d, &st, 0);
        if (rc == PT_OK) rc = collect_fog(ctx);
        if (rc == PT_OK) rc = collect_shading(ctx);
        fill_stats_common(ctx, &st);
        st.num_devices = 1;
        *stats = st;
    }
    fr.open = false;
    return rc;
}

int32_t pt_untile_device(pt_ctx *ctx, int32_t width, int32_t height, int32_t shard_count, int32_t shard_stride_tiles,
                         const void *d_tiles_rgba, const void *d_tiles_accum, void *d_rgba, int32_t stride, void *d_accum,
                         void *stream) {
    if (!ctx) return fail(PT_ERR_INVALID, "ctx is null");
    if (width <= 0 || height <= 0 || shard_count <= 0) return fail(PT_ERR_INVALID, "bad frame or shard count");
    {
        const int32_t nt = ((width + 31) / 32) * ((height + 31) / 32);
        if (shard_stride_tiles != 0 && shard_stride_tiles < tiles_of_shard(nt, pt_shard{0, shard_count}))
            return fail(PT_ERR_INVALID, "shard_stride_tiles smaller than the largest shard");
    }
    if (d_rgba && (stride < width * 4 || stride % 4 != 0)) return fail(PT_ERR_INVALID, "stride must be a multiple of 4 and >= 4*width");
    if (d_rgba && !d_tiles_rgba) return fail(PT_ERR_INVALID, "d_tiles_rgba is null");
    if (d_accum && !d_tiles_accum) return fail(PT_ERR_INVALID, "d_tiles_accum is null");
    Device &d = ctx->devs[0];
    HIP_TRY(hipSetDevice(d.ordinal));
    ptk::UntileArgs U;
    std::memset(&U, 0, sizeof U);
    U.tiles_rgba = static_cast<const uint8_t *>(d_tiles_rgba);
    U.tiles_accum = d_accum ? static_cast<const double *>(d_tiles_accum) : nullptr;
    U.rgba = static_cast<uint8_t *>(d_rgba);
    U.accum = static_cast<double *>(d_accum);
    U.width = width; U.height = height;
    U.ntx = (width + 31) / 32; U.nty = (height + 31) / 32;
    U.stride = stride; U.shard_count = shard_count; U.shard_stride_tiles = shard_stride_tiles;
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : d.own_stream;
    hipLaunchKernelGGL(ptk::untile_kernel, dim3((unsigned)U.ntx, (unsigned)U.nty, 4), dim3(PT_BLOCK), 0, s, U);
    HIP_TRY(hipGetLastError());
    return PT_OK;
}

}  // extern "C"
