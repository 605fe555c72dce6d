// TEST-ONLY stand-alone program: the per-row rules of asyncflow_amd/csrc/af_paired.hpp (afpr::lower_bound_from, match_start,
// arrival_of, window_from, fold64, delta_kind, the order keys, and the sequential statement afpr::pair_statement) as g++ compiles
// them, built with -fsanitize=address,undefined by tests/test_paired_hostcheck.py.  Times, rows, edges, thresholds, slots and
// counters live in heap blocks of exactly their size, so an index one past any of them is a sanitizer report.
//
// stdin:  cases of  `n_draw m_a m_b W T sub_bits min_exp octaves`  then W + 1 edges (W > 0), T thresholds, n_draw times, 2 m_a and
//         2 m_b doubles (start, finish), all as hexadecimal bit patterns.
// stdout: per case ten lines: `unmatched_a unmatched_b`, slot_a, slot_b (n_draw words each), pair_counts (W' x 5), pair_sums
//         (W' x 2, bit patterns), cell_counts (W' x 8), above (W' x T), min_d and max_d (W' x 2, bit patterns), tails (W' x 4),
//         then the non-zero histogram words as `window:side:bin:n`.  A binning that make_binning refuses prints `refused`.
// With the argument `search`: stdin cases of `m guess x` then m times; stdout the count lower_bound_from gives and the plain one.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../asyncflow_amd/csrc/af_paired.hpp"

static bool read_double(double& v) {
    uint64_t u;
    if (std::scanf("%" SCNx64, &u) != 1) return false;
    std::memcpy(&v, &u, 8);
    return true;
}
static double* read_doubles(size_t n) {
    double* v = new double[n];
    for (size_t i = 0; i < n; ++i)
        if (!read_double(v[i])) std::exit(2);
    return v;
}

template <class T>
static void print_row(const T* v, size_t n) {
    for (size_t k = 0; k < n; ++k) std::printf(k ? " %" PRIu64 : "%" PRIu64, (uint64_t)v[k]);
    std::printf("\n");
}
static void print_bits(const double* v, size_t n) {
    for (size_t k = 0; k < n; ++k) std::printf(k ? " %" PRIx64 : "%" PRIx64, afpr::bits_of(v[k]));
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "search") == 0) {
        uint32_t m, guess;
        uint64_t xb;
        while (std::scanf("%" SCNu32 " %" SCNu32 " %" SCNx64, &m, &guess, &xb) == 3) {
            double* row = read_doubles(m);
            const double x = afpr::double_of(xb);
            std::printf("%" PRIu32 " %" PRIu32 "\n", afpr::lower_bound_from(row, m, x, guess), afpr::lower_bound(row, m, x));
            delete[] row;
        }
        return 0;
    }
    uint32_t n_draw, m_a, m_b, W, T, sub_bits, octaves;
    int32_t min_exp;
    while (std::scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNd32 " %" SCNu32, &n_draw, &m_a, &m_b, &W, &T,
                      &sub_bits, &min_exp, &octaves) == 8) {
        const uint32_t wins = W ? W : 1u;
        double* edges = read_doubles(W ? W + 1u : 0u);
        double* thr = read_doubles(T);
        double* times = read_doubles(n_draw);
        double* ca = read_doubles(2u * (size_t)m_a);
        double* cb = read_doubles(2u * (size_t)m_b);
        aflh::Binning b{};
        if (!aflh::make_binning(sub_bits, min_exp, octaves, b)) {
            std::printf("refused\n");
        } else {
            const uint32_t B = b.n_bins;
            uint32_t* slot_a = new uint32_t[n_draw];
            uint32_t* slot_b = new uint32_t[n_draw];
            uint32_t* pair_counts = new uint32_t[(size_t)wins * afpr::kPairCounts];
            double* pair_sums = new double[(size_t)wins * 2u];
            uint32_t unmatched[2];
            uint64_t* cell_counts = new uint64_t[(size_t)wins * afpr::kCellCounts]();
            uint64_t* above = new uint64_t[(size_t)wins * T]();
            uint64_t* kmin = new uint64_t[wins];
            uint64_t* kmax = new uint64_t[wins];
            for (uint32_t w = 0; w < wins; ++w) kmin[w] = afpr::kKeyPosInf, kmax[w] = afpr::kKeyNegInf;
            uint32_t* hist = new uint32_t[(size_t)wins * 2u * B]();
            uint32_t* tails = new uint32_t[(size_t)wins * afpr::kTails]();
            afpr::pair_statement(times, n_draw, ca, m_a, cb, m_b, edges, W, thr, T, b, true, slot_a, slot_b, pair_counts, pair_sums, unmatched,
                                 cell_counts, above, kmin, kmax, hist, tails);
            std::printf("%" PRIu32 " %" PRIu32 "\n", unmatched[0], unmatched[1]);
            print_row(slot_a, n_draw);
            print_row(slot_b, n_draw);
            print_row(pair_counts, (size_t)wins * afpr::kPairCounts);
            print_bits(pair_sums, (size_t)wins * 2u);
            print_row(cell_counts, (size_t)wins * afpr::kCellCounts);
            print_row(above, (size_t)wins * T);
            double* ext = new double[(size_t)wins * 2u];
            for (uint32_t w = 0; w < wins; ++w) ext[2u * w] = afpr::key_value(kmin[w]), ext[2u * w + 1u] = afpr::key_value(kmax[w]);
            print_bits(ext, (size_t)wins * 2u);
            print_row(tails, (size_t)wins * afpr::kTails);
            bool any = false;
            for (uint32_t w = 0; w < wins; ++w)
                for (uint32_t side = 0; side < 2u; ++side)
                    for (uint32_t k = 0; k < B; ++k) {
                        const uint32_t n = hist[((size_t)w * 2u + side) * B + k];
                        if (!n) continue;
                        std::printf(any ? " %" PRIu32 ":%" PRIu32 ":%" PRIu32 ":%" PRIu32 : "%" PRIu32 ":%" PRIu32 ":%" PRIu32 ":%" PRIu32, w, side, k, n);
                        any = true;
                    }
            std::printf("\n");
            delete[] slot_a;
            delete[] slot_b;
            delete[] pair_counts;
            delete[] pair_sums;
            delete[] cell_counts;
            delete[] above;
            delete[] kmin;
            delete[] kmax;
            delete[] hist;
            delete[] tails;
            delete[] ext;
        }
        delete[] edges;
        delete[] thr;
        delete[] times;
        delete[] ca;
        delete[] cb;
    }
    return 0;
}
