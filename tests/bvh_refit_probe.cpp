// Host build of the refit's shared header (csrc/pt_bvh_refit.h) and of the builder that calls it (csrc/pt_bvh.h), for
// test_bvh_refit_cpu.py and, as the host restatement, for test_bvh_refit_probe_gpu.py.  Built as a shared library for ctypes; it has
// a main of its own as well, which builds, moves and refits a generated world and returns the number of failed checks, so the same
// source runs stand-alone (under the sanitizers, for one).
#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pt_bvh.h"

using namespace ptd;

namespace {

struct Probe {
    ptbvh::SceneTrees T;
    std::vector<BvhNode> built;  // the nodes as built (payload bytes in place)
    std::vector<double> box, area;
    double margin = 0.0;
};

struct Ray {
    double o[3], d[3];
};

// objects.go:37-61 and :141-179 in the reference's order; tmax is the closest hit so far
bool hit_sphere(const DevObj &s, const Ray &r, double tmin, double tmax, double &t) {
    const double oc[3] = {r.o[0] - s.a[0], r.o[1] - s.a[1], r.o[2] - s.a[2]};
    const double a = r.d[0] * r.d[0] + r.d[1] * r.d[1] + r.d[2] * r.d[2];
    const double halfB = oc[0] * r.d[0] + oc[1] * r.d[1] + oc[2] * r.d[2];
    const double c = (oc[0] * oc[0] + oc[1] * oc[1] + oc[2] * oc[2]) - s.radius_sq;
    const double disc = halfB * halfB - a * c;
    if (disc < 0) return false;
    const double sq = std::sqrt(disc);
    double root = (-halfB - sq) / a;
    if (root < tmin || root > tmax) {
        root = (-halfB + sq) / a;
        if (root < tmin || root > tmax) return false;
    }
    t = root;
    return true;
}
bool hit_box(const DevObj &b, const Ray &r, double tmin, double tmax, double &t) {
    double t0 = tmin, t1 = tmax;
    for (int k = 0; k < 3; k++) {
        const double iv = 1.0 / r.d[k];
        double tn = (b.a[k] - r.o[k]) * iv, tf = (b.b[k] - r.o[k]) * iv;
        if (iv < 0) { const double s = tn; tn = tf; tf = s; }
        if (tn > t0) t0 = tn;
        if (tf < t1) t1 = tf;
    }
    t = t0;
    return !(t1 <= t0);
}
bool hit(const DevObj &o, const Ray &r, double tmin, double tmax, double &t) {
    return (o.kind & 0xff) == KIND_SPHERE ? hit_sphere(o, r, tmin, tmax, t) : hit_box(o, r, tmin, tmax, t);
}

// `wins` of pt_kernels.h, closest-hit mode
bool wins(bool is_box, int i, double t, int best, bool best_is_box, double tmax) {
    if (t < tmax) return true;
    if (!(t == tmax)) return false;
    if (best < 0) return !is_box;
    if (is_box) return best_is_box && i < best;
    return best_is_box || i > best;
}

// the reference's loop: every finite object in file order, each against the closest hit so far
int linear_winner(const std::vector<DevObj> &w, const Ray &r, double tmin) {
    int best = -1;
    double closest = DBL_MAX;
    for (size_t i = 0; i < w.size(); i++) {
        if ((w[i].kind & 0xff) == KIND_PLANE) continue;
        double t;
        if (hit(w[i], r, tmin, closest, t)) { closest = t; best = (int)i; }
    }
    return best;
}

// a walk of the main tree: slots in order, internal slots pushed, a slot entered when the ray's segment [tmin, closest] meets
// its stored box [c - h, c + h]; objects merged by `wins`
int tree_winner(const Probe &P, const Ray &r, double tmin) {
    int best = -1;
    bool best_is_box = false;
    double closest = DBL_MAX;
    if (P.T.root < 0) return -1;
    std::vector<int32_t> stack{P.T.root};
    while (!stack.empty()) {
        const BvhNode &nd = P.T.nodes[(size_t)stack.back()];
        stack.pop_back();
        for (int s = 0; s < 4; s++) {
            const bool is_obj = ptrf::slot_object(nd.meta, s), is_int = ptrf::slot_internal(nd.meta, s);
            if (!is_obj && !is_int) continue;
            double t0 = tmin, t1 = closest;
            for (int k = 0; k < 3; k++) {
                const double iv = 1.0 / r.d[k];
                double tn = (bvh_slot_lo(nd, k, s) - r.o[k]) * iv, tf = (bvh_slot_hi(nd, k, s) - r.o[k]) * iv;
                if (iv < 0) { const double x = tn; tn = tf; tf = x; }
                if (tn > t0) t0 = tn;
                if (tf < t1) t1 = tf;
            }
            if (t1 < t0) continue;
            const int rank = ptrf::slot_rank(nd.meta, s);
            if (is_int) { stack.push_back(nd.node_base + rank); continue; }
            const BvhObj &bo = P.T.objs[(size_t)(nd.obj_base + rank)];
            const bool is_box = (bo.o.kind & 0xff) == KIND_BOX;
            double t;
            if (!hit(bo.o, r, tmin, is_box ? DBL_MAX : closest, t)) continue;
            if (wins(is_box, bo.index, t, best, best_is_box, closest)) { closest = t; best = bo.index; best_is_box = is_box; }
        }
    }
    return best;
}

uint64_t next_u64(uint64_t &s) {  // splitmix64
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
double next_unit(uint64_t &s) { return (double)(next_u64(s) >> 11) * (1.0 / 9007199254740992.0); }

}  // namespace

extern "C" {

// the trees of world[n] as a render builds them; NULL when they are deeper than the traversal stack
void *rp_build(const DevObj *world, int32_t n) {
    Probe *P = new Probe;
    const std::vector<DevObj> w(world, world + n);
    if (!ptbvh::build_scene_trees(w, false, 96, P->T)) { delete P; return nullptr; }
    P->built = P->T.nodes;
    P->margin = P->T.margin;
    P->box.assign(P->T.nodes.size() * 6, 0.0);
    P->area.assign(P->T.nodes.size(), 0.0);
    return P;
}
void rp_free(void *h) { delete static_cast<Probe *>(h); }

// out = {nodes, object records, levels, nodes of the main tree, depth, records of the main tree}
void rp_counts(void *h, int32_t out[6]) {
    const Probe *P = static_cast<Probe *>(h);
    out[0] = (int32_t)P->T.nodes.size();
    out[1] = (int32_t)P->T.objs.size();
    out[2] = (int32_t)P->T.level_start.size() - 1;
    out[3] = P->T.main_nodes;
    out[4] = P->T.depth;
    out[5] = P->T.main_objs;
}
double rp_margin(void *h) { return static_cast<Probe *>(h)->margin; }

// the current nodes [128 B each], records [96 B each], level table [levels + 1], exact boxes [nodes][6] and a[q] [nodes]; any NULL
void rp_get(void *h, void *nodes, void *objs, int32_t *levels, double *box, double *area) {
    const Probe *P = static_cast<Probe *>(h);
    if (nodes && !P->T.nodes.empty()) std::memcpy(nodes, P->T.nodes.data(), P->T.nodes.size() * sizeof(BvhNode));
    if (objs && !P->T.objs.empty()) std::memcpy(objs, P->T.objs.data(), P->T.objs.size() * sizeof(BvhObj));
    if (levels) std::memcpy(levels, P->T.level_start.data(), P->T.level_start.size() * sizeof(int32_t));
    if (box && !P->box.empty()) std::memcpy(box, P->box.data(), P->box.size() * sizeof(double));
    if (area && !P->area.empty()) std::memcpy(area, P->area.data(), P->area.size() * sizeof(double));
}
void rp_get_built(void *h, void *nodes) {
    const Probe *P = static_cast<Probe *>(h);
    if (!P->built.empty()) std::memcpy(nodes, P->built.data(), P->built.size() * sizeof(BvhNode));
}

// the host refit to world[n] (same count, kinds and order as the built one) and its margin; returns the figure
double rp_refit(void *h, const DevObj *world, int32_t n) {
    Probe *P = static_cast<Probe *>(h);
    const std::vector<DevObj> w(world, world + n);
    P->margin = ptbvh::scene_margin(w);
    ptbvh::refit(P->T.nodes, P->T.objs, w, P->margin, P->T.level_start, P->box, P->area);
    return ptrf::cost_of(P->area.data(), (size_t)P->T.main_nodes);
}

// the figure in the fixed shape from a[0, n)
double rp_cost_of(const double *area, int64_t n) { return ptrf::cost_of(area, (size_t)n); }

// The current tree against world[n]: out = {objects not inside their slot's box by the margin, children's exact boxes not inside the
// parent slot's box by the margin, nodes whose bytes differ from a fresh encode (exact boxes gathered from the objects by recursion,
// encoded into a copy of the built node), nodes whose topology words or payload bytes differ from the built ones, records that are
// not the world's}
void rp_check(void *h, const DevObj *world, int32_t n, int32_t out[5]) {
    const Probe *P = static_cast<Probe *>(h);
    const std::vector<DevObj> w(world, world + n);
    const double m = ptbvh::scene_margin(w);
    int outside = 0, nested = 0, differ = 0, topo = 0, recs = 0;
    std::vector<ptrf::Box> sub(P->T.nodes.size());
    for (size_t q = P->T.nodes.size(); q-- > 0;) {
        const BvhNode &nd = P->T.nodes[q];
        BvhNode fresh = P->built[q];
        ptrf::Box all = ptrf::empty_box();
        for (int s = 0; s < 4; s++) {
            const int rank = ptrf::slot_rank(nd.meta, s);
            const bool is_obj = ptrf::slot_object(nd.meta, s);
            ptrf::Box b;
            if (is_obj) b = ptrf::object_box(w[(size_t)P->T.objs[(size_t)(nd.obj_base + rank)].index]);
            else if (ptrf::slot_internal(nd.meta, s)) b = sub[(size_t)(nd.node_base + rank)];
            else continue;
            ptrf::grow(all, b);
            ptrf::encode_slot(fresh, s, b, m);
            bool in = true;
            for (int k = 0; k < 3; k++) in = in && bvh_slot_lo(nd, k, s) <= b.lo[k] - m * 0.999 && bvh_slot_hi(nd, k, s) >= b.hi[k] + m * 0.999;
            if (!in) (is_obj ? outside : nested)++;
        }
        sub[q] = all;
        if (std::memcmp(&fresh, &nd, sizeof(BvhNode)) != 0) differ++;
        const BvhNode &b0 = P->built[q];
        bool same = nd.node_base == b0.node_base && nd.obj_base == b0.obj_base && nd.meta == b0.meta && std::memcmp(nd.pad, b0.pad, sizeof nd.pad) == 0;
        for (int k = 0; k < 3; k++)
            for (int s = 0; s < 4; s++) same = same && ((ptrf::float_bits(nd.h[k][s]) ^ ptrf::float_bits(b0.h[k][s])) & 0xffu) == 0u;
        if (!same) topo++;
    }
    for (const BvhObj &bo : P->T.objs)
        if (std::memcmp(&bo.o, &w[(size_t)bo.index], sizeof(DevObj)) != 0) recs++;
    out[0] = outside; out[1] = nested; out[2] = differ; out[3] = topo; out[4] = recs;
}

// rays from inside the world's bounds in random directions: how many find another winner through the tree than the reference's
// linear scan of world[n]; *hits receives how many hit anything
int32_t rp_rays(void *h, const DevObj *world, int32_t n, int32_t nrays, uint64_t seed, int32_t *hits) {
    const Probe *P = static_cast<Probe *>(h);
    const std::vector<DevObj> w(world, world + n);
    ptrf::Box all = ptrf::empty_box();
    for (const DevObj &o : w)
        if ((o.kind & 0xff) != KIND_PLANE) ptrf::grow(all, ptrf::object_box(o));
    int bad = 0, nh = 0;
    for (int i = 0; i < nrays; i++) {
        Ray r;
        for (int k = 0; k < 3; k++) {
            r.o[k] = all.lo[k] + (all.hi[k] - all.lo[k]) * (1.2 * next_unit(seed) - 0.1);
            r.d[k] = 2.0 * next_unit(seed) - 1.0;
        }
        const int a = linear_winner(w, r, 0.001), b = tree_winner(*P, r, 0.001);
        bad += a != b;
        nh += a >= 0;
    }
    if (hits) *hits = nh;
    return bad;
}

// bit probes of the shared header: nextafterf(f, +inf) on the bits, the smallest float >= v, one axis, the stored word
uint32_t rp_next_up(uint32_t bits) { return ptrf::float_bits(ptrf::next_up(ptrf::bits_float(bits))); }
uint32_t rp_round_up(double v) { return ptrf::float_bits(ptrf::round_up(v)); }
void rp_encode_axis(double lo, double hi, double margin, uint32_t out[2]) {
    float c, hf;
    ptrf::encode_axis(lo, hi, margin, c, hf);
    out[0] = ptrf::float_bits(c);
    out[1] = ptrf::float_bits(hf);
}
uint32_t rp_h_word(uint32_t h_bits, uint32_t payload) { return ptrf::h_word(ptrf::bits_float(h_bits), payload); }

}  // extern "C"

// Stand-alone: a generated world of `n` objects (argv[1], default 300), one in nine dielectric; built, refitted unchanged, moved
// and refitted, moved back; prints the counts and returns how many checks failed.
int main(int argc, char **argv) {
    const int n = argc > 1 ? std::atoi(argv[1]) : 300;
    uint64_t seed = 7;
    std::vector<DevObj> w((size_t)(n > 0 ? n : 1));
    for (size_t i = 0; i < w.size(); i++) {
        DevObj &o = w[i];
        std::memset(&o, 0, sizeof o);
        const double s = 0.2 + 0.6 * next_unit(seed);
        double p[3];
        for (int k = 0; k < 3; k++) p[k] = 40.0 * next_unit(seed) - 20.0;
        if (i % 3 == 0) {
            o.kind = KIND_BOX;
            for (int k = 0; k < 3; k++) { o.a[k] = p[k] - s; o.b[k] = p[k] + s; }
        } else {
            o.kind = KIND_SPHERE;
            for (int k = 0; k < 3; k++) o.a[k] = p[k];
            o.radius = s;
            o.radius_sq = s * s;
            o.inv_radius = 1.0 / s;
        }
        if (i % 9 == 4) o.kind |= 0x100;
    }
    int failed = 0;
    void *h = rp_build(w.data(), (int32_t)w.size());
    if (!h) return 100;
    int32_t c[6], chk[5], hits = 0;
    rp_counts(h, c);
    std::vector<BvhNode> built((size_t)c[0]), now((size_t)c[0]);
    rp_get_built(h, built.data());
    const double cost0 = rp_refit(h, w.data(), (int32_t)w.size());
    rp_get(h, now.data(), nullptr, nullptr, nullptr, nullptr);
    failed += std::memcmp(built.data(), now.data(), built.size() * sizeof(BvhNode)) != 0;
    std::vector<DevObj> moved = w;
    for (size_t i = 0; i < moved.size(); i += 7) {
        moved[i].a[0] += 1.5;
        moved[i].b[0] += 1.5;
    }
    moved[0].a[1] += 90.0;  // the bound, and with it the margin, grows
    moved[0].b[1] += 90.0;
    const double cost1 = rp_refit(h, moved.data(), (int32_t)moved.size());
    rp_check(h, moved.data(), (int32_t)moved.size(), chk);
    for (int k = 0; k < 5; k++) failed += chk[k] != 0;
    failed += rp_rays(h, moved.data(), (int32_t)moved.size(), 2000, 11, &hits) != 0;
    const double cost2 = rp_refit(h, w.data(), (int32_t)w.size());
    rp_get(h, now.data(), nullptr, nullptr, nullptr, nullptr);
    failed += std::memcmp(built.data(), now.data(), built.size() * sizeof(BvhNode)) != 0;
    failed += !(cost2 == cost0);
    std::printf("nodes %d records %d levels %d figure %.17g moved %.17g ray hits %d failed %d\n", c[0], c[1], c[2], cost0, cost1, hits, failed);
    rp_free(h);
    return failed;
}
