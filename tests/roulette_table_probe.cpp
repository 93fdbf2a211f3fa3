// roulette_table_probe.cpp -- test-only, host only: prints the roulette record (csrc/pt_convert.h: roulette_record) of every
// attenuation on standard input.  One triple per line as three 16-digit hexadecimal words (the doubles' bits); one line out per
// triple: prob q0 q1 q2, the same way.  After the triples' records it prints, behind a line "table", roulette_table() of three
// materials whose albedos are the first three triples: the records of mats[] and the unit record behind them.
// Built by tests/test_roulette_table_cpu.py with g++ -ffp-contract=off, once more with the sanitizers.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pt_convert.h"

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
static void print_record(const ptd::DevRoulette &r) {
    std::printf("%016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", to_hex(r.prob), to_hex(r.q[0]), to_hex(r.q[1]), to_hex(r.q[2]));
}

int main() {
    static_assert(sizeof(ptd::DevRoulette) == 32 && alignof(ptd::DevRoulette) == 16, "DevRoulette layout");
    std::vector<ptd::DevMat> mats;
    uint64_t a, b, c;
    while (std::scanf("%" SCNx64 " %" SCNx64 " %" SCNx64, &a, &b, &c) == 3) {
        print_record(ptd::roulette_record(from_hex(a), from_hex(b), from_hex(c)));
        if (mats.size() < 3) {
            ptd::DevMat m;
            std::memset(&m, 0, sizeof m);
            m.albedo[0] = from_hex(a); m.albedo[1] = from_hex(b); m.albedo[2] = from_hex(c);
            mats.push_back(m);
        }
    }
    std::vector<ptd::DevRoulette> tab;
    ptd::roulette_table(mats, tab);
    std::printf("table\n");
    for (const ptd::DevRoulette &r : tab) print_record(r);
    return 0;
}
