// af_exemplars.hpp -- the k SLOWEST REQUESTS per window and group, WITH THEIR IDENTITY (af_engine_summarize_exemplars, launched
// by engine.hip): which scenario, which row of its rqs_clock, the stored (start, finish) pair and, optionally, the sample row the
// request met on arrival.  Every other analyzer answers with numbers about a cell; this one says which requests are behind them
// (a dashboard's "exemplars", and the input of an extreme-value fit of the tail).
//
// DEFINITION.  Scenario s has m_s = min(counts[s][completed], clock_cap) stored rows (start_i, finish_i).
//   latency   lat = finish - start, one f64 subtraction; a NaN latency is in no cell.
//   window    with edges e[0] < ... < e[W]: window w where e[w] < t <= e[w + 1], t = finish (by finish) or start (by arrival); t <=
//             e[0], t > e[W] or t NaN: no cell.  A mask on every row: no order of the rows is needed or checked.  Without edges
//             (W == 0) one window with no condition on time.  W' = max(W, 1).
//   order     within cell c = g W' + w: larger latency first, compared as f64 VALUES (-0.0 == +0.0, +inf a value like any other),
//             ties by ascending scenario index, then ascending row index -- a total order: the result does not depend on the
//             algorithm, the launch or the batch.
//   outputs   total = the rows of the cell (u64), kept = min(k, total); the first `kept` places of the order as (scenario, row,
//             the stored pair bit for bit); the slots at or past kept: every byte 0xFF.
//   state     for a kept slot the n_series words of sample row q - 1, q = floor(start / period) (af_state.hpp's rule: one f64
//             division, then floor); no state (q < 1, q - 1 >= t_s, start NaN or negative): every word 0xFFFFFFFF.
//
// A RECORD is (key, scenario, row): key = key_of_latency(lat), a u64 that orders like the f64 value (the sign bit flipped of a
// non-negative value, all bits flipped of a negative one; -0.0 is made +0.0 first).  No latency has key 0 (only a NaN's bits
// could), so key 0 with all-ones indices is the EMPTY record, which sorts behind every real one.  `before` is the order.
//
// KERNELS.
//   lists   one wave per scenario (the turns of a scenario are in program order), 64 rows at a time, kUnroll 16-byte loads in
//           flight.  Each lane finds its row's window by binary search and compares its key with the window's THRESHOLD thr[w]: the
//           key of the list's k-th record, 0 while the list holds fewer than k.  Rows arrive in ascending row index, so a row
//           whose key EQUALS the k-th loses the tie: a hit is key > thr[w].  The lanes of a chunk are taken window by window
//           (the __ballot leader loop of afw::partition_place); where a window has hits the wave
//             loads the (scenario, window) list of <= k <= 64 records, one per lane, from the engine's scratch [n][W'][k],
//             with more than kInsertHits hits: sorts them with a 21-stage bitonic network over the wave (sort_wave) and keeps
//             the first 64 of both by the element-wise pick against the reversed hits and a 6-stage bitonic merge
//             (merge_sorted); with few hits -- the steady state of a window, once its list is warm --: puts each in its place
//             (insert_one: a ballot for the place, one shift of the lanes behind it),
//             stores the first min(len + hits, k) back and refreshes thr[w].
//           A chunk without a hit costs a search and a compare per row.  Never hit by hit: in an overloaded run latency grows
//           along the rows and every row is a hit.  The rows of each window are counted as well (cnt[s][w], u32).
//           thr, cnt and the edges lie in dynamic LDS up to kLdsExemplarWindows windows (20 W' + 8 B <= 64 KB, no attribute to
//           set); above, thr and cnt are the engine's scratch (zeroed) and the edges are read from global memory.
//   cells   one wave per cell: the lists of the group's members in ascending scenario index, kMembers loads in flight, each
//           merged into the running list by merge_sorted (both are sorted; the scenario is part of the order, so ties across a
//           member seam fall as the definition says).  total is the sum of the members' counts -- the wave owns the cell, a plain
//           store --, then scenario, row, the pair re-read from the clock rows, and 0xFF bytes behind kept.
//   state   one thread per (slot, series word): only the n_series words of a row are read, never the padding of the pitch.
// Integer compares only, no atomics: every word is identical from run to run.
//
// The per-row rule (row_cell, state_row), the order and the two networks are AF_HD text without a HIP include, the networks over
// a small wave type Wv that holds one record per lane (cx: compare-exchange with lane ^ j; reverse; pick_first; count_before;
// insert_at): gfx950 device
// code with WaveRecs below and, under g++ with an array of 64 records, what tests/hostcheck/exemplars_main.cpp runs under the
// sanitizers.
#pragma once

#include <stdint.h>

#if !defined(AF_HD)
#if defined(__HIPCC__)
#define AF_HD __host__ __device__ __forceinline__
#else
#define AF_HD inline
#endif
#endif

namespace afex {

constexpr uint32_t kMaxK = 64;                     // AF_MAX_EXEMPLARS: a list is one record per lane
constexpr uint32_t kSkip = 0xFFFFFFFFu;            // AF_POOL_SKIP
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kLdsExemplarWindows = 3276;     // windows whose edges, thresholds and counts af_exemplar_lists keeps in LDS (20 W' + 8 B <= 64 KB)
constexpr uint32_t kInsertHits = 8;                // up to this many hits of a window in a chunk are inserted one by one, more are sorted and merged
constexpr uint32_t kUnroll = 4;                    // 16-byte loads a lane of af_exemplar_lists has in flight
constexpr uint32_t kMembers = 4;                   // members' lists a wave of af_exemplar_cells has in flight
constexpr uint32_t kCellWaves = 4;                 // cells per workgroup of af_exemplar_cells

struct Rec {
    uint64_t key;
    uint32_t scen, row;
};
AF_HD Rec empty_rec() { return Rec{0ull, kNone, kNone}; }

// a u64 that orders like the f64 value of a latency that is not NaN; never 0
AF_HD uint64_t key_of_latency(double lat) {
    if (lat == 0.0) lat = 0.0;   // -0.0 and +0.0 are one value
    uint64_t u;
    __builtin_memcpy(&u, &lat, 8);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// THE ORDER: larger key first, then ascending scenario, then ascending row
AF_HD bool before(const Rec& a, const Rec& b) {
    if (a.key != b.key) return a.key > b.key;
    if (a.scen != b.scen) return a.scen < b.scen;
    return a.row < b.row;
}

// the window of a time among the edges e[0 .. W]: w with e[w] < t <= e[w + 1], or kNone (t <= e[0], t > e[W], t NaN)
template <class EdgePtr>
AF_HD uint32_t window_of_time(EdgePtr e, uint32_t W, double t) {
    uint32_t lo = 0u, hi = W + 1u;   // #{ k <= W : e[k] < t }; a NaN counts every edge
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (!(t <= e[mid])) lo = mid + 1u;
        else hi = mid;
    }
    return lo >= 1u && lo <= W ? lo - 1u : kNone;
}

// THE PER-ROW RULE: is the row in a cell, and then its window (0 without edges) and its key
template <class EdgePtr>
AF_HD bool row_cell(double start, double finish, EdgePtr e, uint32_t W, bool by_arrival, uint32_t& w, uint64_t& key) {
    const double lat = finish - start;
    if (lat != lat) return false;
    w = 0u;
    if (W) {
        w = window_of_time(e, W, by_arrival ? start : finish);
        if (w == kNone) return false;
    }
    key = key_of_latency(lat);
    return true;
}

// the sample row a request met on arrival (af_state.hpp's tick rule), or kNone
AF_HD uint32_t state_row(double start, double period, uint32_t t_s) {
    if (!(start >= 0.0)) return kNone;   // NaN, negative
    const double q = __builtin_floor(start / period);
    if (!(q >= 1.0) || q - 1.0 >= (double)t_s) return kNone;
    return (uint32_t)(q - 1.0);
}

// one compare-exchange of a bitonic network: what lane `lane` keeps of its record and lane ^ j's.  k is the length of the
// sorted runs the stage builds (k == 64: one run, the first record at lane 0).
AF_HD bool keeps_first(uint32_t lane, uint32_t j, uint32_t k) { return ((lane & j) == 0u) == ((lane & k) == 0u); }
AF_HD Rec pick(bool a_not_b, const Rec& a, const Rec& b) {   // (word by word: a choice between the two objects would put both in memory)
    return Rec{a_not_b ? a.key : b.key, a_not_b ? a.scen : b.scen, a_not_b ? a.row : b.row};
}
AF_HD Rec cx_keep(const Rec& mine, const Rec& other, bool first) { return pick(before(mine, other) == first, mine, other); }

// 64 records in any places -> in the order, the first at lane 0 (the empty ones last): 21 stages
template <class Wv>
AF_HD void sort_wave(Wv& v) {
#pragma unroll
    for (uint32_t k = 2u; k <= 64u; k <<= 1)
#pragma unroll
        for (uint32_t j = k >> 1; j > 0u; j >>= 1) v.cx(j, k);
}

// two waves of records, each in the order -> `list` holds the first 64 of both, in the order; `cand` is used up.  Lane i takes
// the earlier of list[i] and cand[63 - i]: those are the first 64 of the union, as a bitonic sequence; six stages sort it.
template <class Wv>
AF_HD void merge_sorted(Wv& list, Wv& cand) {
    cand.reverse();
    list.pick_first(cand);
#pragma unroll
    for (uint32_t j = 32u; j > 0u; j >>= 1) list.cx(j, 64u);
}

// one record more into a wave in the order: behind the records that are before it, the others move one lane up (lane 63's is lost)
template <class Wv>
AF_HD void insert_one(Wv& list, const Rec& c) {
    list.insert_at(list.count_before(c), c);
}

struct ExArgs {
    const double* clock;            // [n][clock_cap][2]
    const uint32_t* counts;         // [n][8]
    uint32_t clock_cap, cnt_completed_slot;
    const uint32_t* group;          // [n], or null: all in group 0
    uint32_t n_win, wins;           // W and W' = max(W, 1)
    const double* edges;            // DEVICE [W + 1] (W > 0)
    uint32_t by_arrival, k;
    unsigned long long* lkey;       // scratch [n][W'][k]: the lists' keys ...
    uint32_t* lrow;                 // ... and rows
    uint32_t* cnt;                  // scratch [n][W']: the rows of (scenario, window); zeroed before the launch
    unsigned long long* thr;        // scratch [n][W'], zeroed (more than kLdsExemplarWindows windows only)
    const uint32_t* members;        // [members of all groups] scenario indices, group by group, ascending within a group
    const uint32_t* g_off;          // [G + 1] a group's first member
    uint64_t cells;                 // G W'
    unsigned long long* total;      // [C]
    uint32_t* kept;                 // [C] or null
    uint32_t* scenario;             // [C][k]
    uint32_t* row;                  // [C][k]
    double* pair;                   // [C][k][2]
    // the state gather
    const uint32_t* samples;        // [n][tick_cap][pitch]
    uint32_t tick_cap, pitch, n_series, cnt_ticks_slot;
    double period;
    uint32_t* state;                // [C][k][n_series]
};

#if defined(__HIPCC__)
// the wave's records, one per lane.  kScen == false: every record of the wave has the same scenario, which is not exchanged.
template <bool kScen>
struct WaveRecs {
    Rec r;
    __device__ __forceinline__ static Rec from_lane(const Rec& v, int src) {
        Rec o;
        const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v.key, src, 64), hi = (uint32_t)__shfl((int)(uint32_t)(v.key >> 32), src, 64);
        o.key = ((uint64_t)hi << 32) | lo;
        o.scen = kScen ? (uint32_t)__shfl((int)v.scen, src, 64) : v.scen;
        o.row = (uint32_t)__shfl((int)v.row, src, 64);
        return o;
    }
    __device__ __forceinline__ void cx(uint32_t j, uint32_t k) {
        const uint32_t lane = threadIdx.x & 63u;
        const Rec o = from_lane(r, (int)(lane ^ j));
        r = cx_keep(r, o, keeps_first(lane, j, k));
    }
    __device__ __forceinline__ void reverse() { r = from_lane(r, 63 - (int)(threadIdx.x & 63u)); }
    __device__ __forceinline__ void pick_first(const WaveRecs& o) { r = pick(before(o.r, r), o.r, r); }
    // the records before c are the first lanes (the wave is in the order): their number is c's place
    __device__ __forceinline__ uint32_t count_before(const Rec& c) const { return (uint32_t)__popcll(__ballot(before(r, c))); }
    __device__ __forceinline__ void insert_at(uint32_t pos, const Rec& c) {   // (pos and c: the same in every lane)
        const uint32_t lane = threadIdx.x & 63u;
        const Rec below = from_lane(r, lane ? (int)lane - 1 : 0);
        r = pick(lane < pos, r, pick(lane == pos, c, below));
    }
};

// the lists of scenario blockIdx.x, window by window, and the windows' row counts; ONE wave
template <bool kLds>
__global__ void __launch_bounds__(64) af_exemplar_lists(const ExArgs a) {
    extern __shared__ __attribute__((aligned(8))) unsigned char afex_dyn[];   // kLds: [W + 1] f64 edges (W > 0), [W'] u64 thr, [W'] u32 cnt
    const uint32_t s = blockIdx.x, lane = threadIdx.x;
    const uint32_t g = a.group ? a.group[s] : 0u;
    if (g == kSkip) return;
    const uint32_t W = a.n_win, wins = a.wins, ne = W ? W + 1u : 0u, K = a.k;
    uint32_t m = a.counts[(size_t)s * 8u + a.cnt_completed_slot];
    if (m > a.clock_cap) m = a.clock_cap;
    const double2* ck = reinterpret_cast<const double2*>(a.clock) + (size_t)s * a.clock_cap;
    double* le = reinterpret_cast<double*>(afex_dyn);
    unsigned long long* thr = kLds ? reinterpret_cast<unsigned long long*>(afex_dyn + (size_t)ne * 8u) : a.thr + (size_t)s * wins;
    uint32_t* cnt = kLds ? reinterpret_cast<uint32_t*>(afex_dyn + (size_t)ne * 8u + (size_t)wins * 8u) : a.cnt + (size_t)s * wins;
    if (kLds) {
        for (uint32_t k = lane; k < ne; k += 64u) le[k] = a.edges[k];
        for (uint32_t w = lane; w < wins; w += 64u) {
            thr[w] = 0ull;
            cnt[w] = 0u;
        }
        __syncthreads();
    }
    const double* e = kLds ? le : a.edges;
    const size_t list0 = (size_t)s * wins * K;
    for (uint32_t base = 0u; base < m; base += kUnroll * 64u) {   // (uniform trip count: the ballots below are wave-wide)
        double2 c[kUnroll];
#pragma unroll
        for (uint32_t u = 0; u < kUnroll; ++u) {
            const uint32_t i = base + u * 64u + lane;
            c[u] = i < m && i >= base ? ck[i] : double2{0.0, 0.0};   // (i >= base: no wrap)
        }
#pragma unroll
        for (uint32_t u = 0; u < kUnroll; ++u) {   // 64 rows at a time, in row order
            const uint32_t i = base + u * 64u + lane;
            uint32_t w = 0u;
            uint64_t key = 0ull;
            const bool in = i < m && i >= base && row_cell(c[u].x, c[u].y, e, W, a.by_arrival != 0u, w, key);
            const bool hit = in && key > thr[w];
            unsigned long long todo = __ballot(in);
            while (todo) {   // one turn per distinct window of the 64 rows
                const int leader = __ffsll((long long)todo) - 1;
                const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)w, leader);
                const bool mine = in && w == v;
                const unsigned long long same = __ballot(mine), hits = __ballot(mine && hit);
                const uint32_t have = cnt[v];   // (the same word in every lane)
                if (hits) {
                    const uint32_t len = have < K ? have : K;
                    const size_t at = list0 + (size_t)v * K;
                    const Rec none{0ull, s, kNone};   // (one scenario: the empty records carry it too)
                    WaveRecs<false> L;
                    L.r = lane < len ? Rec{a.lkey[at + lane], s, a.lrow[at + lane]} : none;
                    const uint32_t n_hits = (uint32_t)__popcll(hits);
                    if (n_hits > kInsertHits) {
                        WaveRecs<false> C;
                        C.r = mine && hit ? Rec{key, s, i} : none;
                        sort_wave(C);
                        merge_sorted(L, C);
                    } else {
                        for (unsigned long long h = hits; h; h &= h - 1ull) {   // in row order: an equal key goes behind
                            const int src = __ffsll((long long)h) - 1;
                            const uint32_t klo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)key, src);
                            const uint32_t khi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(key >> 32), src);
                            insert_one(L, Rec{((uint64_t)khi << 32) | klo, s, (uint32_t)__builtin_amdgcn_readlane((int)i, src)});
                        }
                    }
                    const uint32_t grown = len + n_hits, now = grown < K ? grown : K;
                    if (lane < now) {
                        a.lkey[at + lane] = L.r.key;
                        a.lrow[at + lane] = L.r.row;
                    }
                    if (lane == K - 1u) thr[v] = now == K ? L.r.key : 0ull;
                }
                if ((int)lane == leader) cnt[v] = have + (uint32_t)__popcll(same);
                todo &= ~same;
            }
            __syncthreads();   // (one wave: the lists, thr and cnt written by one lane are read by another in a later turn)
        }
        if (m - base <= kUnroll * 64u) break;   // (base + kUnroll * 64 could wrap)
    }
    if (kLds)
        for (uint32_t w = lane; w < wins; w += 64u) a.cnt[(size_t)s * wins + w] = cnt[w];
}

// cell c0 + blockIdx.x * kCellWaves + wave: the members' lists merged, then the outputs
__global__ void __launch_bounds__(64u * kCellWaves) af_exemplar_cells(const ExArgs a, uint64_t c0) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t cell = c0 + (uint64_t)blockIdx.x * kCellWaves + (threadIdx.x >> 6);
    if (cell >= a.cells) return;   // (the whole wave)
    const uint32_t wins = a.wins, K = a.k;
    const uint32_t g = (uint32_t)(cell / wins), w = (uint32_t)(cell % wins);
    const uint32_t m0 = a.g_off[g], m1 = a.g_off[g + 1u];
    WaveRecs<true> L;
    L.r = empty_rec();
    unsigned long long tot = 0ull;
    for (uint32_t j = m0; j < m1; j += kMembers) {   // (uniform; m1 <= n)
        uint32_t sc[kMembers], cn[kMembers];
        Rec r[kMembers];
#pragma unroll
        for (uint32_t u = 0; u < kMembers; ++u) {
            sc[u] = m1 - j > u ? a.members[j + u] : kNone;
            cn[u] = sc[u] != kNone ? a.cnt[(size_t)sc[u] * wins + w] : 0u;
        }
#pragma unroll
        for (uint32_t u = 0; u < kMembers; ++u) {
            const uint32_t len = cn[u] < K ? cn[u] : K;
            const size_t at = ((size_t)sc[u] * wins + w) * K;
            r[u] = lane < len ? Rec{a.lkey[at + lane], sc[u], a.lrow[at + lane]} : empty_rec();
        }
#pragma unroll
        for (uint32_t u = 0; u < kMembers; ++u) {
            if (cn[u] == 0u) continue;   // (uniform)
            tot += cn[u];
            WaveRecs<true> C;
            C.r = r[u];
            merge_sorted(L, C);
        }
        if (m1 - j <= kMembers) break;
    }
    const uint32_t kept = tot < K ? (uint32_t)tot : K;
    if (lane == 0u) {
        a.total[cell] = tot;
        if (a.kept) a.kept[cell] = kept;
    }
    if (lane < K) {
        const size_t o = (size_t)cell * K + lane;
        double2* pair = reinterpret_cast<double2*>(a.pair) + o;
        if (lane < kept) {
            a.scenario[o] = L.r.scen;
            a.row[o] = L.r.row;
            *pair = (reinterpret_cast<const double2*>(a.clock) + (size_t)L.r.scen * a.clock_cap)[L.r.row];
        } else {
            a.scenario[o] = kNone;
            a.row[o] = kNone;
            const double ones = __longlong_as_double(-1ll);
            *pair = double2{ones, ones};
        }
    }
}

// state[slot][j] = word j of the sample row the slot's request met on arrival, or all ones; a thread per word
__global__ void __launch_bounds__(256) af_exemplar_state(const ExArgs a, uint64_t words) {
    const uint32_t S = a.n_series;
    for (uint64_t x = (uint64_t)blockIdx.x * 256u + threadIdx.x; x < words; x += (uint64_t)gridDim.x * 256u) {
        const uint64_t slot = x / S;
        const uint32_t j = (uint32_t)(x % S);
        const uint32_t sc = a.scenario[slot];
        uint32_t word = kNone;
        if (sc != kNone) {
            uint32_t t_s = a.counts[(size_t)sc * 8u + a.cnt_ticks_slot];
            if (t_s > a.tick_cap) t_s = a.tick_cap;
            const uint32_t k = state_row(a.pair[2u * slot], a.period, t_s);
            if (k != kNone) word = a.samples[((size_t)sc * a.tick_cap + k) * a.pitch + j];
        }
        a.state[x] = word;
    }
}
#endif  // __HIPCC__

}  // namespace afex
