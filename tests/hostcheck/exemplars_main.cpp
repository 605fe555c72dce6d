// TEST-ONLY stand-alone program: the plain-C++ routines of asyncflow_amd/csrc/af_exemplars.hpp as g++ compiles them -- the per-row
// rule (afex::row_cell: latency, canonical key, window, rejections; afex::state_row), the order (afex::before), the two
// networks (afex::sort_wave, afex::merge_sorted) and afex::insert_one over a wave of 64 records held in an array --, built with
// -fsanitize=address,undefined by tests/test_exemplars_hostcheck.py.  Edges and rows live in heap blocks of exactly their size, so
// an index one past any of them is a sanitizer report.
//
// stdin, one case after the other:
//   rows W by_arrival m      then W + 1 edges (W > 0) and 2 m values (start, finish), doubles as hexadecimal bit patterns
//                            -> m lines  `in w key`  (key in hexadecimal; `0 0 0` for a row in no cell)
//   state t_s m              then the period and m starts  -> m lines: the sample row, or 4294967295
//   sort n                   then n records  `lane key scen row`  (key hexadecimal; the other lanes are empty)
//                            -> 64 lines  `key scen row`: the wave after sort_wave
//   merge na nb              then na records `key scen row` IN THE ORDER (the list, lanes 0 .. na - 1) and nb records
//                            `lane key scen row` in any lanes (the candidates, sorted by sort_wave first, as the kernel does)
//                            -> 64 lines: the list after merge_sorted
//   insert na nb             then na records `key scen row` in the order (the list) and nb records `key scen row`, put in one by
//                            one with insert_one  -> 64 lines: the list after them
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../../asyncflow_amd/csrc/af_exemplars.hpp"

// the wave type of the networks on the host: 64 records, every lane's step taken from a copy of the wave before it
struct HostWave {
    afex::Rec r[64];
    HostWave() {
        for (auto& x : r) x = afex::empty_rec();
    }
    void cx(uint32_t j, uint32_t k) {
        afex::Rec n[64];
        for (uint32_t lane = 0; lane < 64u; ++lane) n[lane] = afex::cx_keep(r[lane], r[lane ^ j], afex::keeps_first(lane, j, k));
        std::memcpy(r, n, sizeof r);
    }
    void reverse() {
        afex::Rec n[64];
        for (uint32_t lane = 0; lane < 64u; ++lane) n[lane] = r[63u - lane];
        std::memcpy(r, n, sizeof r);
    }
    void pick_first(const HostWave& o) {
        for (uint32_t lane = 0; lane < 64u; ++lane)
            if (afex::before(o.r[lane], r[lane])) r[lane] = o.r[lane];
    }
    uint32_t count_before(const afex::Rec& c) const {
        uint32_t n = 0u;
        for (const auto& x : r) n += afex::before(x, c) ? 1u : 0u;
        return n;
    }
    void insert_at(uint32_t pos, const afex::Rec& c) {
        afex::Rec n[64];
        for (uint32_t lane = 0; lane < 64u; ++lane) n[lane] = lane < pos ? r[lane] : lane == pos ? c : r[lane - 1u];
        std::memcpy(r, n, sizeof r);
    }
    void print() const {
        for (const auto& x : r) std::printf("%" PRIx64 " %" PRIu32 " %" PRIu32 "\n", x.key, x.scen, x.row);
    }
};

static bool read_double(double& v) {
    uint64_t u;
    if (std::scanf("%" SCNx64, &u) != 1) return false;
    std::memcpy(&v, &u, 8);
    return true;
}

static bool read_placed(HostWave& w, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t lane;
        afex::Rec x;
        if (std::scanf("%" SCNu32 " %" SCNx64 " %" SCNu32 " %" SCNu32, &lane, &x.key, &x.scen, &x.row) != 4 || lane >= 64u) return false;
        w.r[lane] = x;
    }
    return true;
}

int main() {
    char what[16];
    while (std::scanf("%15s", what) == 1) {
        if (std::strcmp(what, "rows") == 0) {
            uint32_t W, by_arrival, m;
            if (std::scanf("%" SCNu32 " %" SCNu32 " %" SCNu32, &W, &by_arrival, &m) != 3) return 2;
            double* e = W ? new double[(size_t)W + 1u] : nullptr;
            for (uint32_t k = 0; W && k <= W; ++k)
                if (!read_double(e[k])) return 2;
            double* rows = new double[2u * (size_t)m];
            for (size_t i = 0; i < 2u * (size_t)m; ++i)
                if (!read_double(rows[i])) return 2;
            for (uint32_t i = 0; i < m; ++i) {
                uint32_t w = 0u;
                uint64_t key = 0u;
                const bool in = afex::row_cell(rows[2u * i], rows[2u * i + 1u], e, W, by_arrival != 0u, w, key);
                if (in) std::printf("1 %" PRIu32 " %" PRIx64 "\n", w, key);
                else std::printf("0 0 0\n");
            }
            delete[] e;
            delete[] rows;
        } else if (std::strcmp(what, "state") == 0) {
            uint32_t t_s, m;
            double period;
            if (std::scanf("%" SCNu32 " %" SCNu32, &t_s, &m) != 2 || !read_double(period)) return 2;
            for (uint32_t i = 0; i < m; ++i) {
                double start;
                if (!read_double(start)) return 2;
                std::printf("%" PRIu32 "\n", afex::state_row(start, period, t_s));
            }
        } else if (std::strcmp(what, "sort") == 0) {
            uint32_t n;
            HostWave w;
            if (std::scanf("%" SCNu32, &n) != 1 || !read_placed(w, n)) return 2;
            afex::sort_wave(w);
            w.print();
        } else if (std::strcmp(what, "merge") == 0) {
            uint32_t na, nb;
            HostWave list, cand;
            if (std::scanf("%" SCNu32 " %" SCNu32, &na, &nb) != 2 || na > 64u) return 2;
            for (uint32_t i = 0; i < na; ++i)
                if (std::scanf("%" SCNx64 " %" SCNu32 " %" SCNu32, &list.r[i].key, &list.r[i].scen, &list.r[i].row) != 3) return 2;
            if (!read_placed(cand, nb)) return 2;
            afex::sort_wave(cand);
            afex::merge_sorted(list, cand);
            list.print();
        } else if (std::strcmp(what, "insert") == 0) {
            uint32_t na, nb;
            HostWave list;
            if (std::scanf("%" SCNu32 " %" SCNu32, &na, &nb) != 2 || na > 64u) return 2;
            for (uint32_t i = 0; i < na; ++i)
                if (std::scanf("%" SCNx64 " %" SCNu32 " %" SCNu32, &list.r[i].key, &list.r[i].scen, &list.r[i].row) != 3) return 2;
            for (uint32_t i = 0; i < nb; ++i) {
                afex::Rec c;
                if (std::scanf("%" SCNx64 " %" SCNu32 " %" SCNu32, &c.key, &c.scen, &c.row) != 3) return 2;
                afex::insert_one(list, c);
            }
            list.print();
        } else {
            return 2;
        }
    }
    return 0;
}
