// feature_record_probe.cpp -- stand-alone host program over csrc/pt_atrous.h (tests/test_feature_walk_cpu.py builds it with
// -fsanitize=address,undefined and runs it).  pta::hit_record is the tail that was split out of pta::first_hit so that the BVH
// walk's kernels (csrc/pt_feature_walk.h) state the feature record with the same code.  For one object of each kind and random
// rays, three computations of the record must agree bit for bit:
//   * first_hit as it stands;
//   * closest_hit, then hit_record on its (best, t) -- what feature_bvh_kernel does with the walk's winner;
//   * closest_hit, then the record as first_hit computed it before the split, restated below.
// Prints "<rays> rays, <hits> hits, 0 differences" and exits 0, or the first difference and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "pt_atrous.h"

namespace {

// The record as first_hit computed it in line before hit_record existed.
void record_before_the_split(const ptd::DevObj *objs, const ptd::DevMat *mats, int32_t best, double t, const double o[3], const double d[3],
                             double n[3], double a[3], double &dist) {
    const ptd::DevObj &ob = objs[best];
    const int kind = ob.kind & 0xff;
    double nx, ny, nz;
    bool front;
    if (kind == ptd::KIND_SPHERE) {
        const double px = o[0] + d[0] * t, py = o[1] + d[1] * t, pz = o[2] + d[2] * t;
        nx = (px - ob.a[0]) * ob.inv_radius;
        ny = (py - ob.a[1]) * ob.inv_radius;
        nz = (pz - ob.a[2]) * ob.inv_radius;
        front = d[0] * nx + d[1] * ny + d[2] * nz < 0;
    } else if (kind == ptd::KIND_PLANE) {
        nx = ob.b[0]; ny = ob.b[1]; nz = ob.b[2];
        front = ob.b[0] * d[0] + ob.b[1] * d[1] + ob.b[2] * d[2] < 0;
    } else {
        const double px = o[0] + d[0] * t, py = o[1] + d[1] * t, pz = o[2] + d[2] * t;
        double m = px - ob.a[0];
        nx = -1; ny = 0; nz = 0;
        double v = ob.b[0] - px;
        if (v < m) { m = v; nx = 1; ny = 0; nz = 0; }
        v = py - ob.a[1];
        if (v < m) { m = v; nx = 0; ny = -1; nz = 0; }
        v = ob.b[1] - py;
        if (v < m) { m = v; nx = 0; ny = 1; nz = 0; }
        v = pz - ob.a[2];
        if (v < m) { m = v; nx = 0; ny = 0; nz = -1; }
        v = ob.b[2] - pz;
        if (v < m) { nx = 0; ny = 0; nz = 1; }
        front = d[0] * nx + d[1] * ny + d[2] * nz < 0;
    }
    n[0] = front ? nx : -nx;
    n[1] = front ? ny : -ny;
    n[2] = front ? nz : -nz;
    const ptd::DevMat &mt = mats[ob.mat];
    a[0] = mt.albedo[0]; a[1] = mt.albedo[1]; a[2] = mt.albedo[2];
    dist = t * ptm::f_sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
}

uint64_t g_state = 0x9e3779b97f4a7c15ull;
double uniform(double lo, double hi) {  // xorshift64*: the same rays on every run
    g_state ^= g_state >> 12;
    g_state ^= g_state << 25;
    g_state ^= g_state >> 27;
    const uint64_t r = g_state * 0x2545f4914f6cdd1dull;
    return lo + (hi - lo) * ((double)(r >> 11) * (1.0 / 9007199254740992.0));
}

struct Record {
    double n[3], a[3], dist;
};

bool same(const Record &x, const Record &y) { return std::memcmp(&x, &y, sizeof x) == 0; }

}  // namespace

int main() {
    ptd::DevMat mats[3];
    std::memset(mats, 0, sizeof mats);
    for (int m = 0; m < 3; m++)
        for (int k = 0; k < 3; k++) mats[m].albedo[k] = 0.125 * (double)(1 + m) + 0.0625 * (double)k;
    ptd::DevObj kinds[3];
    std::memset(kinds, 0, sizeof kinds);
    kinds[0].kind = ptd::KIND_SPHERE;
    kinds[0].a[0] = 0.25; kinds[0].a[1] = 1.5; kinds[0].a[2] = -0.75;
    kinds[0].radius = 1.25;
    kinds[0].radius_sq = kinds[0].radius * kinds[0].radius;
    kinds[0].inv_radius = 1.0 / kinds[0].radius;
    kinds[0].mat = 0;
    kinds[1].kind = ptd::KIND_PLANE;
    kinds[1].a[1] = 0.5;
    kinds[1].b[1] = 1.0;
    kinds[1].mat = 1;
    kinds[2].kind = ptd::KIND_BOX;
    kinds[2].a[0] = -1.0; kinds[2].a[1] = 0.25; kinds[2].a[2] = -1.5;
    kinds[2].b[0] = 0.5; kinds[2].b[1] = 2.0; kinds[2].b[2] = 0.75;
    kinds[2].mat = 2;
    const char *names[3] = {"sphere", "plane", "box"};
    long rays = 0, hits = 0;
    for (int kind = 0; kind < 3; kind++) {
        long kind_hits = 0;
        for (int i = 0; i < 20000; i++) {
            // origins around and inside the object, directions of any length towards its neighbourhood
            const double o[3] = {uniform(-4, 4), uniform(-3, 5), uniform(-4, 4)};
            const double scale = i % 3 == 0 ? 1.0 : i % 3 == 1 ? 1e-3 : 37.5;
            const double d[3] = {(uniform(-1.5, 1.5) - o[0]) * scale, (uniform(-0.5, 2.5) - o[1]) * scale, (uniform(-1.5, 1.5) - o[2]) * scale};
            rays++;
            Record whole, split, before;
            std::memset(&whole, 0, sizeof whole);
            std::memset(&split, 0, sizeof split);
            std::memset(&before, 0, sizeof before);
            int32_t index = -7;
            const bool any = pta::first_hit(&kinds[kind], mats, 1, o, d, whole.n, whole.a, whole.dist, &index);
            const ptf::FRay r = ptf::make_fray(o[0], o[1], o[2], d[0], d[1], d[2]);
            double t = 0;
            int32_t best = -7;
            const bool any2 = ptf::closest_hit(&kinds[kind], 1, r, t, best);
            if (any != any2 || index != best || (any && best != 0) || (!any && best != -1)) {
                std::printf("%s ray %d: first_hit says %d (index %d), closest_hit %d (index %d)\n", names[kind], i, (int)any, index, (int)any2, best);
                return 1;
            }
            if (!any) continue;
            hits++;
            kind_hits++;
            pta::hit_record(&kinds[kind], mats, best, t, o, d, split.n, split.a, split.dist);
            record_before_the_split(&kinds[kind], mats, best, t, o, d, before.n, before.a, before.dist);
            if (!same(whole, split) || !same(whole, before)) {
                std::printf("%s ray %d: the records differ: normal %.17g %.17g %.17g | %.17g %.17g %.17g | %.17g %.17g %.17g, dist %.17g | %.17g | %.17g\n",
                            names[kind], i, whole.n[0], whole.n[1], whole.n[2], split.n[0], split.n[1], split.n[2], before.n[0], before.n[1],
                            before.n[2], whole.dist, split.dist, before.dist);
                return 1;
            }
        }
        if (kind_hits < 2000) {
            std::printf("%s: only %ld hits\n", names[kind], kind_hits);
            return 1;
        }
    }
    std::printf("%ld rays, %ld hits, 0 differences\n", rays, hits);
    return 0;
}
