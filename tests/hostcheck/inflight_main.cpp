// TEST-ONLY stand-alone program: the per-row logic and the chunk walk of asyncflow_amd/csrc/af_inflight.hpp (afif::row_ticks,
// afif::chunk_hit, afif::scenario_series with its carry from chunk to chunk, afif::bin_of) as g++ compiles them, built with
// -fsanitize=address,undefined by tests/test_inflight_hostcheck.py.  Rows, chunk arrays and outputs live in heap blocks of
// exactly their size, so an index one past any of them is a sanitizer report.
//
// stdin:  cases of  `m t_s chunk`  (chunk 0: the kernel's kChunkTicks) then 1 + 2 m doubles as hexadecimal bit patterns: the
//         period, then the rows (start, finish).
// stdout: per case four lines:  `last chunk`  (in_flight at the last tick, the chunk used), then started, finished and in_flight,
//         t_s words each.
// With the argument `bins`: stdin lines of `v lo n_bins`, stdout the bin of each.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../../asyncflow_amd/csrc/af_inflight.hpp"

static bool read_double(double& v) {
    uint64_t u;
    if (std::scanf("%" SCNx64, &u) != 1) return false;
    std::memcpy(&v, &u, 8);
    return true;
}

static void print_row(const uint32_t* v, uint32_t n) {
    for (uint32_t k = 0; k < n; ++k) std::printf(k ? " %" PRIu32 : "%" PRIu32, v[k]);
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "bins") == 0) {
        uint32_t v, lo, n_bins;
        while (std::scanf("%" SCNu32 " %" SCNu32 " %" SCNu32, &v, &lo, &n_bins) == 3) std::printf("%" PRIu32 "\n", afif::bin_of(v, lo, n_bins));
        return 0;
    }
    uint32_t m, t_s, chunk;
    while (std::scanf("%" SCNu32 " %" SCNu32 " %" SCNu32, &m, &t_s, &chunk) == 3) {
        if (chunk == 0u) chunk = afif::kChunkTicks;
        double period;
        if (!read_double(period)) return 2;
        double* rows = new double[2u * (size_t)m];
        for (size_t i = 0; i < 2u * (size_t)m; ++i)
            if (!read_double(rows[i])) return 2;
        const uint32_t words = t_s < chunk ? t_s : chunk;   // what a chunk needs at the most
        uint32_t* diff = new uint32_t[words];
        uint32_t* fin = new uint32_t[words];
        uint32_t* started = new uint32_t[t_s];
        uint32_t* finished = new uint32_t[t_s];
        uint32_t* in_flight = new uint32_t[t_s];
        for (uint32_t k = 0; k < t_s; ++k) started[k] = finished[k] = in_flight[k] = 0xDEADBEEFu;
        const uint32_t last = afif::scenario_series(rows, m, period, t_s, chunk, diff, fin, started, finished, in_flight);
        std::printf("%" PRIu32 " %" PRIu32 "\n", last, chunk);
        print_row(started, t_s);
        print_row(finished, t_s);
        print_row(in_flight, t_s);
        delete[] rows;
        delete[] diff;
        delete[] fin;
        delete[] started;
        delete[] finished;
        delete[] in_flight;
    }
    return 0;
}
