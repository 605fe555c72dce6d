// TEST-ONLY stand-alone program over the host instantiation of asyncflow_amd/csrc/af_wide.hpp and the per-cell routine of
// asyncflow_amd/csrc/af_series_warmup.hpp (tests/test_series_warmup_hostcheck.py builds it with the sanitizer flags of
// tests/hostcheck/build.py and checks what it prints against Python integers).
//   warmup_check ops     stdin: lines of eight hexadecimal words, a.w[0..3] b.w[0..3].  Per line the limbs, low first, of
//                        a + b, a - b, a * b.w[0], a * (b.w[1] 2^64 + b.w[0]) -- all modulo 2^256 -- and cmp(a, b).
//   warmup_check cells   stdin, binary: per sequence a u32 J and J u64 batch sums Y.  Per sequence d* and the limbs of S1(d*),
//                        S2(d*), S1(0), S2(0), from afwu::cell_of: the lanes of the device's wave one after the other.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../asyncflow_amd/csrc/af_series_warmup.hpp"

using afw256::U256;

static void print_limbs(const U256& v) {
    for (int i = 0; i < 4; ++i) std::printf("%016" PRIx64 " ", v.w[i]);
}

static int run_ops() {
    U256 a, b;
    for (;;) {
        uint64_t w[8];
        int got = 0;
        for (; got < 8; ++got)
            if (std::scanf("%" SCNx64, &w[got]) != 1) break;
        if (got == 0) return 0;
        if (got != 8) return 2;
        for (int i = 0; i < 4; ++i) a.w[i] = w[i], b.w[i] = w[4 + i];
        print_limbs(afw256::add(a, b));
        print_limbs(afw256::sub(a, b));
        print_limbs(afw256::mul_u64(a, b.w[0]));
        print_limbs(afw256::mul_u128(a, b.w[0], b.w[1]));
        std::printf("%d\n", afw256::cmp(a, b));
    }
}

static int run_cells() {
    std::vector<uint64_t> y;
    for (;;) {
        uint32_t J;
        const size_t head = std::fread(&J, sizeof J, 1, stdin);
        if (head != 1) return 0;
        if (J >= afwu::kMaxWindowBatches) return 3;
        y.assign(J, 0u);
        if (J && std::fread(y.data(), sizeof(uint64_t), J, stdin) != J) return 2;
        const afwu::Cell c = afwu::cell_of(y.data(), J);
        std::printf("%" PRIu32 " ", c.trunc);
        print_limbs(c.at.s1);
        print_limbs(c.at.s2);
        print_limbs(c.all.s1);
        print_limbs(c.all.s2);
        std::printf("\n");
    }
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "ops")) return run_ops();
    if (argc == 2 && !std::strcmp(argv[1], "cells")) return run_cells();
    std::fprintf(stderr, "usage: warmup_check ops | cells\n");
    return 1;
}
