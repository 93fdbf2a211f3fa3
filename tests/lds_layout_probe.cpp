// Prints ptd::LdsLayout (csrc/pt_device.h) for rows of counts given on the command line, six numbers a row:
//   nobj nmat n_bsph n_bbox n_dsph n_dbox
// One line per row and shape: "trace|glass <rec_order> mat kidx kidx_diel world rec rec_diel total".  Host-only: built with g++.
#include <cstdio>
#include <cstdlib>

#include "pt_device.h"

static void print(const char *shape, int ro, const ptd::LdsLayout &l) {
    std::printf("%s %d %zu %zu %zu %zu %zu %zu %zu\n", shape, ro, l.mat, l.kidx, l.kidx_diel, l.world, l.rec, l.rec_diel, l.total);
}

int main(int argc, char **argv) {
    if ((argc - 1) % 6 != 0) return 2;
    for (int i = 1; i + 5 < argc; i += 6) {
        size_t n[6];
        for (int k = 0; k < 6; k++) n[k] = (size_t)std::strtoull(argv[i + k], nullptr, 10);
        for (int ro = 0; ro < 2; ro++) {
            print("trace", ro, ptd::LdsLayout::trace(n[0], n[1], n[2], n[3], n[4], n[5], ro != 0));
            print("glass", ro, ptd::LdsLayout::glass(n[0], n[1], n[4], n[5], ro != 0));
        }
    }
    // usable in a constant expression: the kernels' offsets fold where the counts are known
    static_assert(ptd::LdsLayout::trace(1, 1, 1, 0, 0, 0, true).rec == 224, "80 + 128 + 4, rounded up to 16");
    return 0;
}
