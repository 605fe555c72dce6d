// TEST-ONLY stand-alone program: the per-row rule, the arrival rule, the binary search on the tick, the clamp and the chunk walk of
// asyncflow_amd/csrc/af_alert_outcomes.hpp (afao::outcome_row, afao::arrival_tick, afao::arrival_lower, afao::timeouts_of,
// afao::deficit_of and afao::scenario_outcome_ticks with its carries from chunk to chunk) as g++ compiles them, built with
// -fsanitize=address,undefined by tests/test_alert_outcomes_hostcheck.py.  Rows, arrivals, chunk arrays, prefix arrays and outputs
// live in heap blocks of exactly their size, so an index one past any of them is a sanitizer report.
//
// stdin:  cases of  `m n_arr t_s chunk`  (chunk 0: the kernel's kChunkTicks), then 3 + 2 m + n_arr doubles as hexadecimal bit
//         patterns: the period, the slo, the timeout, the rows (start, finish), the arrival row.
// stdout: per case six lines:  `chunk deficit timed_out`, then total, bad, timeouts, PT and PB (t_s words each).
// With the argument `search`: stdin cases of `n n_bounds`, then 2 + n doubles (the period, the timeout, the row), then n_bounds
// tick bounds; stdout one line of the n_bounds results of afao::arrival_lower.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../../asyncflow_amd/csrc/af_alert_outcomes.hpp"

static bool read_double(double& v) {
    uint64_t u;
    if (std::scanf("%" SCNx64, &u) != 1) return false;
    std::memcpy(&v, &u, 8);
    return true;
}

static void print_row(const uint32_t* v, size_t n) {
    for (size_t k = 0; k < n; ++k) std::printf(k ? " %" PRIu32 : "%" PRIu32, v[k]);
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "search") == 0) {
        uint32_t n, nb;
        while (std::scanf("%" SCNu32 " %" SCNu32, &n, &nb) == 2) {
            double period, tau;
            if (!read_double(period) || !read_double(tau)) return 2;
            double* arr = new double[n];
            for (uint32_t j = 0; j < n; ++j)
                if (!read_double(arr[j])) return 2;
            for (uint32_t k = 0; k < nb; ++k) {
                uint32_t bound;
                if (std::scanf("%" SCNu32, &bound) != 1) return 2;
                std::printf(k ? " %" PRIu32 : "%" PRIu32, afao::arrival_lower(arr, n, period, tau, bound));
            }
            std::printf("\n");
            delete[] arr;
        }
        return 0;
    }
    uint32_t m, n_arr, t_s, chunk;
    while (std::scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &m, &n_arr, &t_s, &chunk) == 4) {
        if (chunk == 0u) chunk = afao::kChunkTicks;
        double period, slo, tau;
        if (!read_double(period) || !read_double(slo) || !read_double(tau)) return 2;
        double* rows = new double[2u * (size_t)m];
        for (size_t i = 0; i < 2u * (size_t)m; ++i)
            if (!read_double(rows[i])) return 2;
        double* arr = new double[n_arr];
        for (uint32_t j = 0; j < n_arr; ++j)
            if (!read_double(arr[j])) return 2;
        const uint32_t words = t_s < chunk ? t_s : chunk;   // what a chunk needs at the most
        uint32_t* c_c = new uint32_t[words];
        uint32_t* cbad_c = new uint32_t[words];
        int32_t* pend_c = new int32_t[words];
        uint32_t* tick[5];   // total, bad, timeouts, PT, PB
        for (auto& p : tick) {
            p = new uint32_t[t_s];
            for (uint32_t k = 0; k < t_s; ++k) p[k] = 0xDEADBEEFu;
        }
        uint32_t deficit = 0xDEADBEEFu, timed_out = 0xDEADBEEFu;
        afao::scenario_outcome_ticks(rows, m, arr, n_arr, period, slo, tau, t_s, chunk, c_c, cbad_c, pend_c, tick[3], tick[4], tick[0], tick[1],
                                     tick[2], deficit, timed_out);
        std::printf("%" PRIu32 " %" PRIu32 " %" PRIu32 "\n", chunk, deficit, timed_out);
        for (auto& p : tick) print_row(p, t_s);
        delete[] rows;
        delete[] arr;
        delete[] c_c;
        delete[] cbad_c;
        delete[] pend_c;
        for (auto& p : tick) delete[] p;
    }
    return 0;
}
