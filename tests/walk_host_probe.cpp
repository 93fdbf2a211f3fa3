// walk_host_probe.cpp -- test-only, host only: ptg::TreeWorld (csrc/pt_gl_walk.h) on a scene and a query table from standard input,
// with a local stack of PT_BVH_STACK entries, so that a walk that overruns its stack is a sanitizer report.
// In: "nobj nq"; nobj lines "type px py pz sx sy sz" (type: PT_OBJ_*, the doubles as 16-digit hexadecimal words); nq lines of ten
// words: kind (0 closest, 1 occluded), ro, rd, tmin, tmax, skip.  The tables are built as glwalk_support's gw_open builds them.
// Out: "built stack_need deepest walked plain", then per query "idx_loop idx_tree t_loop t_tree" (t as words; occluded: 0 / 1 and 0).
// Built by tests/test_walk_probe_cpu.py with g++ -ffp-contract=off, once more with the sanitizers.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pt_bvh.h"
#include "pt_convert.h"
#include "pt_gl_walk.h"

static double from_hex(uint64_t u) {
    double d;
    std::memcpy(&d, &u, sizeof d);
    return d;
}
static uint64_t to_hex(double d) {
    uint64_t u;
    std::memcpy(&u, &d, sizeof u);
    return u;
}

int main() {
    int nobj = 0, nq = 0;
    if (std::scanf("%d %d", &nobj, &nq) != 2 || nobj < 0 || nq < 0) return 2;
    std::vector<pt_object> raw((size_t)nobj);
    for (pt_object &o : raw) {
        uint64_t w[6];
        std::memset(&o, 0, sizeof o);
        if (std::scanf("%d %" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64, &o.type, &w[0], &w[1], &w[2], &w[3], &w[4], &w[5]) != 7)
            return 2;
        for (int k = 0; k < 3; k++) {
            o.position[k] = from_hex(w[k]);
            o.size[k] = from_hex(w[3 + k]);
        }
    }
    pt_material mat;
    std::memset(&mat, 0, sizeof mat);
    pt_scene sc;
    std::memset(&sc, 0, sizeof sc);
    sc.num_materials = 1;
    sc.materials = &mat;
    sc.num_objects = nobj;
    sc.objects = raw.data();
    std::vector<ptg::GlObj> objs;
    for (int i = 0; i < nobj; i++) objs.push_back(ptg::gl_object(raw[(size_t)i], 1));
    std::vector<ptd::DevObj> world;
    std::vector<ptd::DevMat> dmats;
    ptd::scene_to_world(sc, world, dmats);
    std::vector<int32_t> plane_idx;
    for (size_t i = 0; i < world.size(); i++)
        if ((world[i].kind & 0xff) == ptd::KIND_PLANE) plane_idx.push_back((int32_t)i);
    ptbvh::SceneTrees T;
    const bool built = ptbvh::build_scene_trees(world, false, PT_BVH_STACK, T);
    ptd::DevFrame F;
    std::memset(&F, 0, sizeof F);
    ptbvh::frame_bounds(ptbvh::world_bound(world), F);
    F.n_plane = (int32_t)plane_idx.size();
    F.bvh_root = built ? T.root : -1;
    F.bvh_stack = PT_BVH_STACK;
    F.nobj = (int32_t)world.size();
    std::vector<uint64_t> lines;
    uint32_t deepest = 0, walked = 0, plain = 0;
    const ptg::LinearWorld lin{objs.data(), nobj};
    for (int i = 0; i < nq; i++) {
        uint64_t w[10];
        for (uint64_t &v : w)
            if (std::scanf("%" SCNx64, &v) != 1) return 2;
        double r[10];
        for (int k = 0; k < 10; k++) r[k] = from_hex(w[k]);
        int stack[PT_BVH_STACK];
        ptg::WalkCount wc = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
        const ptg::TreeWorld tree{objs.data(), nobj, F, T.nodes.data(), T.objs.data(), plane_idx.data(), stack, 1, wc};
        int32_t a, b;
        double ta = 0.0, tb = 0.0;
        if (r[0] == 0) {
            a = lin.closest(r + 1, r + 4, r[7], r[8], (int32_t)r[9], ta);
            b = tree.closest(r + 1, r + 4, r[7], r[8], (int32_t)r[9], tb);
        } else {
            a = lin.occluded(r + 1, r + 4, r[8]) ? 1 : 0;
            b = tree.occluded(r + 1, r + 4, r[8]) ? 1 : 0;
        }
        if (wc.deepest > deepest) deepest = wc.deepest;
        walked += wc.closest_walked + wc.shadow_walked;
        plain += wc.closest_plain + wc.shadow_plain;
        lines.push_back((uint64_t)(uint32_t)a);
        lines.push_back((uint64_t)(uint32_t)b);
        lines.push_back(to_hex(ta));
        lines.push_back(to_hex(tb));
    }
    std::printf("%d %d %u %u %u\n", built ? 1 : 0, T.stack_need, deepest, walked, plain);
    for (size_t i = 0; i < lines.size(); i += 4)
        std::printf("%d %d %016" PRIx64 " %016" PRIx64 "\n", (int32_t)lines[i], (int32_t)lines[i + 1], lines[i + 2], lines[i + 3]);
    return 0;
}
