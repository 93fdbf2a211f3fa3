// Host build of the device build's shared header (csrc/pt_bvh_build.h) and of its restatement (ptbvh::build_scene_trees_lbvh), for
// test_bvh_build_cpu.py and, as the host side of the comparison, for test_bvh_build_probe_gpu.py.  The ray generator, the linear scan
// and the tree walk are the refit probe's: its source is included here (its main renamed).  Built as a shared library for ctypes; with
// its own main it reads worlds from files of DevObj records (argv) and returns the number of failed checks, so the same source runs
// stand-alone (under the sanitizers, for one).
#define main bvh_refit_probe_main
#include "bvh_refit_probe.cpp"
#undef main

namespace {

struct BuildProbe {
    Probe P;             // the two trees, as the refit probe holds them
    ptbb::Lbvh tree[2];  // the stages of the main and the dielectric tree
    std::vector<DevObj> w;
    bool fits = false;
};

}  // namespace

extern "C" {

// the Morton-order trees of world[n]; never NULL (bp_counts says whether they fit a stack of `stack_limit` entries)
void *bp_build(const DevObj *world, int32_t n, int32_t stack_limit) {
    BuildProbe *B = new BuildProbe;
    B->w.assign(world, world + n);
    B->fits = ptbvh::build_scene_trees_lbvh(B->w, stack_limit, B->P.T, &B->tree[0], &B->tree[1]);
    B->P.built = B->P.T.nodes;
    B->P.margin = B->P.T.margin;
    return B;
}
void bp_free(void *h) { delete static_cast<BuildProbe *>(h); }

// out = {nodes, records, levels, nodes of the main tree, depth, records of the main tree, stack_need, fits}
void bp_counts(void *h, int32_t out[8]) {
    BuildProbe *B = static_cast<BuildProbe *>(h);
    rp_counts(&B->P, out);
    out[6] = B->P.T.stack_need;
    out[7] = B->fits ? 1 : 0;
}
double bp_margin(void *h) { return static_cast<BuildProbe *>(h)->P.margin; }
void bp_get(void *h, void *nodes, void *objs, int32_t *levels) { rp_get(&static_cast<BuildProbe *>(h)->P, nodes, objs, levels, nullptr, nullptr); }

// tree t (0 main, 1 dielectric): out = {objects, nodes, levels}
void bp_tree_counts(void *h, int32_t t, int32_t out[3]) {
    const ptbb::Lbvh &L = static_cast<BuildProbe *>(h)->tree[t];
    out[0] = (int32_t)L.sorted.size();
    out[1] = (int32_t)L.nodes.size();
    out[2] = L.level_start.empty() ? 0 : (int32_t)L.level_start.size() - 1;
}
// ... its sorted keys [n], sorted positions [n], children [n - 1][2], parents [2 n - 1], boxes [2 n - 1][6], nodes, order [n], levels
void bp_tree_get(void *h, int32_t t, uint64_t *keys, int32_t *sorted, int32_t *child, int32_t *parent, double *box, void *nodes, int32_t *order,
                 int32_t *levels) {
    const ptbb::Lbvh &L = static_cast<BuildProbe *>(h)->tree[t];
    auto copy = [](void *dst, const void *src, size_t bytes) {
        if (dst && bytes) std::memcpy(dst, src, bytes);
    };
    copy(keys, L.keys.data(), L.keys.size() * 8);
    copy(sorted, L.sorted.data(), L.sorted.size() * 4);
    copy(child, L.child.data(), L.child.size() * 4);
    copy(parent, L.parent.data(), L.parent.size() * 4);
    copy(box, L.box.data(), L.box.size() * 8);
    copy(nodes, L.nodes.data(), L.nodes.size() * sizeof(BvhNode));
    copy(order, L.order.data(), L.order.size() * 4);
    copy(levels, L.level_start.data(), L.level_start.size() * 4);
}

// ... and the binary nodes ptbb::gather4 puts into the four slots of its wide nodes, breadth-first as ptbb::collapse takes them:
// out [nodes][4], -1 for an empty slot
void bp_tree_slots(void *h, int32_t t, int32_t *out) {
    const ptbb::Lbvh &L = static_cast<BuildProbe *>(h)->tree[t];
    const int32_t n = (int32_t)L.sorted.size();
    if (n == 0) return;
    const ptbb::BinView tr{L.child.data(), L.box.data(), nullptr, n};  // (gather4 asks for no leaf's object)
    std::vector<int32_t> cur{0}, next;
    size_t q = 0;
    while (!cur.empty() && q < L.nodes.size()) {
        next.clear();
        for (size_t i = 0; i < cur.size() && q < L.nodes.size(); i++, q++) {
            int32_t *slot = out + 4 * q;
            ptbb::gather4(tr, cur[i], slot);
            for (int s = 0; s < 4; s++)
                if (slot[s] >= 0 && !tr.leaf(slot[s])) next.push_back(slot[s]);
        }
        cur.swap(next);
    }
}

// ptbvh::check_trees on the trees
void bp_check(void *h, int32_t out[8]) {
    const BuildProbe *B = static_cast<BuildProbe *>(h);
    ptbvh::check_trees(B->P.T, B->w, out);
}
// the refit probe's rays against the trees and the linear scan of the same world
int32_t bp_rays(void *h, int32_t nrays, uint64_t seed, int32_t *hits) {
    BuildProbe *B = static_cast<BuildProbe *>(h);
    return rp_rays(&B->P, B->w.data(), (int32_t)B->w.size(), nrays, seed, hits);
}
// a refit of the trees to their own world: the number of nodes whose bytes changed
int32_t bp_refit_same(void *h) {
    BuildProbe *B = static_cast<BuildProbe *>(h);
    if (B->P.T.nodes.empty()) return 0;
    (void)rp_refit(&B->P, B->w.data(), (int32_t)B->w.size());
    int32_t differ = 0;
    for (size_t q = 0; q < B->P.built.size(); q++) differ += std::memcmp(&B->P.built[q], &B->P.T.nodes[q], sizeof(BvhNode)) != 0;
    return differ;
}

// the key routines: the scale of an axis, a quantised coordinate, the interleave
double bp_key_scale(double cmin, double cmax) { return ptbb::key_scale(cmin, cmax); }
void bp_quantise(const double *c, int32_t n, double cmin, double scale, uint32_t *out) {
    for (int32_t i = 0; i < n; i++) {
        double v = c[i];
        if (!ptbb::finite_d(v)) v = 0.0;  // (as ptbb::centroid does)
        out[i] = ptbb::quantise(v, cmin, scale);
    }
}
void bp_morton(const uint32_t *q, int32_t n, uint64_t *out) {
    for (int32_t i = 0; i < n; i++) out[i] = ptbb::morton(q[3 * i], q[3 * i + 1], q[3 * i + 2]);
}
// the bytes of ptbvh::build_scene_trees (the host builder): nodes, then records; returns the byte count (call with NULL first)
int64_t bp_sah_bytes(const DevObj *world, int32_t n, void *out) {
    ptbvh::SceneTrees T;
    const std::vector<DevObj> w(world, world + n);
    if (!ptbvh::build_scene_trees(w, false, 96, T)) return -1;
    const size_t a = T.nodes.size() * sizeof(BvhNode), b = T.objs.size() * sizeof(BvhObj);
    if (out) {
        if (a) std::memcpy(out, T.nodes.data(), a);
        if (b) std::memcpy(static_cast<char *>(out) + a, T.objs.data(), b);
    }
    return (int64_t)(a + b);
}

}  // extern "C"

// Stand-alone: every argument is a file of DevObj records (one world).  Each is built, checked, refitted to itself and walked by
// 2000 rays; prints one line per world and returns how many checks failed.
int main(int argc, char **argv) {
    int failed = 0;
    for (int a = 1; a < argc; a++) {
        std::FILE *f = std::fopen(argv[a], "rb");
        if (!f) { failed++; continue; }
        std::vector<DevObj> w;
        DevObj o;
        while (std::fread(&o, sizeof o, 1, f) == 1) w.push_back(o);
        std::fclose(f);
        void *h = bp_build(w.data(), (int32_t)w.size(), 96);
        int32_t c[8], chk[8], hits = 0;
        bp_counts(h, c);
        bp_check(h, chk);
        int bad = 0;
        for (int k = 4; k < 8; k++) bad += chk[k] != 0;
        bad += bp_rays(h, 2000, 11, &hits) != 0;
        bad += bp_refit_same(h) != 0;
        std::printf("%s: objects %zu nodes %d records %d levels %d stack %d ray hits %d failed %d\n", argv[a], w.size(), c[0], c[1], c[2], c[6], hits, bad);
        failed += bad;
        bp_free(h);
    }
    return failed;
}
