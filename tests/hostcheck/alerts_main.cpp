// TEST-ONLY stand-alone program: the per-row rule, the chunk walk, the rolling condition and the mask steps of
// asyncflow_amd/csrc/af_alerts.hpp (afal::row_tick, afal::rolling, afal::alert_cond, afal::hold_step, afal::cell_step and
// afal::scenario_alerts with its carries from chunk to chunk and from step to step) as g++ compiles them, built with
// -fsanitize=address,undefined by tests/test_alerts_hostcheck.py.  Rows, chunk arrays, prefix arrays and outputs live in heap
// blocks of exactly their size, so an index one past any of them is a sanitizer report.
//
// stdin:  cases of  `m t_s chunk R W`  (chunk 0: the kernel's kChunkTicks), then 2 + 2 m doubles as hexadecimal bit patterns: the
//         period, the slo, then the rows (start, finish); then 6 R words: the rules; then W + 1 words: the tick edges.
// stdout: per case eleven lines:  `chunk`, then total, bad and firing (t_s words each), count (W words), and fired, episodes,
//         longest, longest_start, first, last (W R words each).
// With the argument `hold`: stdin lines of `hold n` and n hexadecimal condition masks, the steps of one run of ticks; stdout the
// n firing masks and the run carried out of the last step.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../../asyncflow_amd/csrc/af_alerts.hpp"

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
    if (argc > 1 && std::strcmp(argv[1], "hold") == 0) {
        uint32_t hold, n;
        while (std::scanf("%" SCNu32 " %" SCNu32, &hold, &n) == 2) {
            uint32_t run = 0u;
            for (uint32_t k = 0; k < n; ++k) {
                uint64_t cond;
                if (std::scanf("%" SCNx64, &cond) != 1) return 2;
                std::printf("%" PRIx64 " ", afal::hold_step(cond, hold, run));
            }
            std::printf("%" PRIu32 "\n", run);
        }
        return 0;
    }
    uint32_t m, t_s, chunk, R, W;
    while (std::scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &m, &t_s, &chunk, &R, &W) == 5) {
        if (chunk == 0u) chunk = afal::kChunkTicks;
        double period, slo;
        if (!read_double(period) || !read_double(slo)) return 2;
        double* rows = new double[2u * (size_t)m];
        for (size_t i = 0; i < 2u * (size_t)m; ++i)
            if (!read_double(rows[i])) return 2;
        afal::Rule* rules = new afal::Rule[R];
        for (uint32_t r = 0; r < R; ++r)
            if (std::scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &rules[r].long_ticks, &rules[r].short_ticks,
                           &rules[r].num, &rules[r].den, &rules[r].min_total, &rules[r].hold_ticks) != 6)
                return 2;
        uint32_t* edges = new uint32_t[(size_t)W + 1u];
        for (uint32_t w = 0; w <= W; ++w)
            if (std::scanf("%" SCNu32, &edges[w]) != 1) return 2;
        const uint32_t words = t_s < chunk ? t_s : chunk;   // what a chunk needs at the most
        uint32_t* tot_c = new uint32_t[words];
        uint32_t* bad_c = new uint32_t[words];
        uint32_t* pt = new uint32_t[t_s];
        uint32_t* pb = new uint32_t[t_s];
        uint32_t* tick[3];
        for (auto& p : tick) {
            p = new uint32_t[t_s];
            for (uint32_t k = 0; k < t_s; ++k) p[k] = 0xDEADBEEFu;
        }
        const size_t cells = (size_t)W * R;
        uint32_t* count = new uint32_t[W];
        for (uint32_t w = 0; w < W; ++w) count[w] = 0xDEADBEEFu;
        uint32_t* cell[6];
        for (auto& p : cell) {
            p = new uint32_t[cells];
            for (size_t k = 0; k < cells; ++k) p[k] = 0xDEADBEEFu;
        }
        afal::scenario_alerts(rows, m, period, slo, t_s, chunk, tot_c, bad_c, pt, pb, rules, R, edges, W, tick[0], tick[1], tick[2], count,
                              cell[0], cell[1], cell[2], cell[3], cell[4], cell[5]);
        std::printf("%" PRIu32 "\n", chunk);
        for (auto& p : tick) print_row(p, t_s);
        print_row(count, W);
        for (auto& p : cell) print_row(p, cells);
        delete[] rows;
        delete[] rules;
        delete[] edges;
        delete[] tot_c;
        delete[] bad_c;
        delete[] pt;
        delete[] pb;
        delete[] count;
        for (auto& p : tick) delete[] p;
        for (auto& p : cell) delete[] p;
    }
    return 0;
}
