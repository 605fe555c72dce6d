// TEST-ONLY stand-alone program: the per-row logic of asyncflow_amd/csrc/af_arrival_counts.hpp (afac::row_bounds: row length,
// the binary searches, the streaming pass, the rule between them) as g++ compiles it, built with -fsanitize=address,undefined
// by tests/test_arrival_counts_cpu.py.  Rows and bounds live in heap blocks of exactly their size, so an index one past either
// is a sanitizer report.
//
// stdin:  cases of  `n_draw n_windows force`  then n_draw + n_windows + 1 doubles as hexadecimal bit patterns (the row, the edges);
//         force: 0 the rule's choice, 1 binary searches, 2 the streaming pass.
// stdout: per case  `length streamed b[0] ... b[n_windows]`  (streamed: 1 when the rule picks the streaming pass for this row).
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../asyncflow_amd/csrc/af_arrival_counts.hpp"

static bool read_double(double& v) {
    uint64_t u;
    if (std::scanf("%" SCNx64, &u) != 1) return false;
    std::memcpy(&v, &u, 8);
    return true;
}

int main() {
    uint32_t n_draw, n_windows;
    int force;
    while (std::scanf("%" SCNu32 " %" SCNu32 " %d", &n_draw, &n_windows, &force) == 3) {
        double* row = new double[n_draw];
        double* edges = new double[n_windows + 1u];
        uint32_t* b = new uint32_t[n_windows + 1u];
        for (uint32_t i = 0; i < n_draw; ++i)
            if (!read_double(row[i])) return 2;
        for (uint32_t k = 0; k <= n_windows; ++k)
            if (!read_double(edges[k])) return 2;
        for (uint32_t k = 0; k <= n_windows; ++k) b[k] = 0xDEADBEEFu;
        const uint32_t m = afac::row_bounds(row, n_draw, (const double*)edges, n_windows, b, force);
        const uint32_t lo = afac::count_le(row, m, edges[0]), hi = afac::count_le(row, m, edges[n_windows]);
        std::printf("%" PRIu32 " %d", m, afac::use_stream(hi - lo, n_windows) ? 1 : 0);
        for (uint32_t k = 0; k <= n_windows; ++k) std::printf(" %" PRIu32, b[k]);
        std::printf("\n");
        delete[] row;
        delete[] edges;
        delete[] b;
    }
    return 0;
}
