// TEST-ONLY stand-alone program: the per-row rule of asyncflow_amd/csrc/af_latency_histogram.hpp (aflh::make_binning,
// aflh::bin_of_latency, aflh::row_cell with afex::window_of_time, and the sequential statement aflh::scenario_cells) as g++
// compiles them, built with -fsanitize=address,undefined by tests/test_latency_histogram_hostcheck.py.  Rows, edges and counters
// live in heap blocks of exactly their size, so an index one past any of them is a sanitizer report.
//
// stdin:  cases of  `m W by_arrival sub_bits min_exp octaves`  then W + 1 edges (W > 0) and 2 m doubles (start, finish), all as
//         hexadecimal bit patterns.
// stdout: per case six lines:  `n_bins`, then count, under, over and nan (W' words each), then the non-zero histogram words as
//         `window:bin:n` triples.  A binning that make_binning refuses prints the one line `refused`.
// With the argument `bins`: stdin lines of `sub_bits min_exp octaves bits`, stdout the entry of each (n_bins under, n_bins + 1
// over, n_bins + 2 nan) or `refused`.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../../asyncflow_amd/csrc/af_latency_histogram.hpp"

static bool read_double(double& v) {
    uint64_t u;
    if (std::scanf("%" SCNx64, &u) != 1) return false;
    std::memcpy(&v, &u, 8);
    return true;
}

template <class T>
static void print_row(const T* v, uint32_t n) {
    for (uint32_t k = 0; k < n; ++k) std::printf(k ? " %" PRIu64 : "%" PRIu64, (uint64_t)v[k]);
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "bins") == 0) {
        uint32_t sub_bits, octaves;
        int32_t min_exp;
        uint64_t bits;
        while (std::scanf("%" SCNu32 " %" SCNd32 " %" SCNu32 " %" SCNx64, &sub_bits, &min_exp, &octaves, &bits) == 4) {
            aflh::Binning b{};
            if (!aflh::make_binning(sub_bits, min_exp, octaves, b)) {
                std::printf("refused\n");
                continue;
            }
            double x;
            std::memcpy(&x, &bits, 8);
            std::printf("%" PRIu32 "\n", aflh::bin_of_latency(x, b));
        }
        return 0;
    }
    uint32_t m, W, by_arrival, sub_bits, octaves;
    int32_t min_exp;
    while (std::scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNd32 " %" SCNu32, &m, &W, &by_arrival, &sub_bits, &min_exp, &octaves) == 6) {
        const uint32_t ne = W ? W + 1u : 0u, wins = W ? W : 1u;
        double* edges = new double[ne];
        for (uint32_t k = 0; k < ne; ++k)
            if (!read_double(edges[k])) return 2;
        double* rows = new double[2u * (size_t)m];
        for (size_t i = 0; i < 2u * (size_t)m; ++i)
            if (!read_double(rows[i])) return 2;
        aflh::Binning b{};
        if (!aflh::make_binning(sub_bits, min_exp, octaves, b)) {
            std::printf("refused\n");
        } else {
            uint64_t* count = new uint64_t[wins]();
            uint32_t* hist = new uint32_t[(size_t)wins * b.n_bins]();
            uint32_t* under = new uint32_t[wins]();
            uint32_t* over = new uint32_t[wins]();
            uint32_t* nan = new uint32_t[wins]();
            aflh::scenario_cells(rows, m, edges, W, by_arrival != 0u, b, count, hist, under, over, nan);
            std::printf("%" PRIu32 "\n", b.n_bins);
            print_row(count, wins);
            print_row(under, wins);
            print_row(over, wins);
            print_row(nan, wins);
            bool any = false;
            for (uint32_t w = 0; w < wins; ++w)
                for (uint32_t k = 0; k < b.n_bins; ++k)
                    if (hist[(size_t)w * b.n_bins + k]) {
                        std::printf(any ? " %" PRIu32 ":%" PRIu32 ":%" PRIu32 : "%" PRIu32 ":%" PRIu32 ":%" PRIu32, w, k, hist[(size_t)w * b.n_bins + k]);
                        any = true;
                    }
            std::printf("\n");
            delete[] count;
            delete[] hist;
            delete[] under;
            delete[] over;
            delete[] nan;
        }
        delete[] edges;
        delete[] rows;
    }
    return 0;
}
