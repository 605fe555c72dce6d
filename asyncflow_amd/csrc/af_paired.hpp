// af_paired.hpp -- PAIRED LATENCY DIFFERENCES between scenarios that share their seeds (af_engine_summarize_pairs, launched by
// engine.hip): the same request under configuration A and under configuration B, joined through the arrival row both were sent.
//
// DEFINITION.  Pair p compares scenarios a = pair_a[p] and b = pair_b[p]; A = its arrival row (times[time_row[p]], ascending, +inf
// behind the last arrival, m = its finite entries); side x has m_x = min(counts[x][completed], clock_cap) stored rows (start, finish).
//   match     row i of side x maps to j = #{ k < m : A[k] < start_i } (np.searchsorted "left") when j < m and A[j] has the BIT
//             PATTERN of start_i (a NaN, a -0.0 against +0.0, a start beside an arrival: no match).  row_x[j] = the smallest i that
//             maps to j, kNone without one; unmatched_x = m_x - #{ j : row_x[j] set }.
//   arrival j state bit 0: row_a[j] set, bit 1: row_b[j] set (3 both, 1 only a, 2 only b, 0 neither).  Of a `both` arrival
//             lat_x = finish - start of row row_x[j], d = lat_b - lat_a: three f64 subtractions.  d NaN: counted in nan, nothing else.
//   window    by the arrival time A[j]: w with e[w] < A[j] <= e[w + 1] -- the rank c = #{ k : e[k] < A[j] } among the edges, w =
//             c - 1 when 1 <= c <= W --, A ascending: a contiguous range of j.  Without edges one window over every j.  W' = max(W, 1).
//   per (pair, window)   counts[5] u32: both, only_a, only_b, neither, nan;  sums[2] f64: sum_d and sum_a over the `both` arrivals
//             with d not NaN, in the FIXED ORDER of fold64 below: lane l = j mod 64 adds its values in ascending j from +0.0, the
//             64 partial sums fold part[l] += part[l + h], l < h, h = 32 .. 1.
//   per cell c = g W' + w (the pairs of group g): cell_counts[8] u64 = the five counts and slower (d > 0), faster (d < 0), equal
//             (d == 0);  above[T] u64 = #{ d > thresholds[t] };  extremes[2] f64 = min and max of d in float order (-0.0 < +0.0;
//             +inf / -inf without a value);  hist[2][n_bins] u32: d > 0 binned on d, d < 0 on -d (aflh::bin_of_latency);
//             tails[4] u32: under_pos, under_neg (0 < |d| < 2^min_exp), over_pos, over_neg (at or above the last bin, infinities).
//             equal + tails + sum(hist) + nan == both.  Integer + and min / max only: no order of the pairs matters.
//
// KERNELS.  Two passes per chunk of pairs; the slots between them are 2 x 4 B per (pair, draw), 0xFF-filled (the row_a / row_b
// outputs themselves when the caller asks for them).
//   match     af_pairs_match: a WAVE per (pair, side, kMatchRows rows).  A lane loads its (start, finish) pair as one 16-byte
//             word and looks `start` up in the arrival row from a guess -- the position the wave's previous step found, one row
//             further per lane: completion order is close to arrival order, so lower_bound_from gallops a few probes where a
//             plain search takes 17 --, then atomicMin of the row index into the slot.  Every probe is below m.
//   reduce    af_pairs_reduce: a WAVE per pair walks j in steps of 64: A[j], the two slots, the two clock rows they name (each
//             checked against m_x), d, and the window from the previous step's rank (afac::edge_rank_from; edges in LDS up to
//             kLdsPairWindows windows).  Per-lane partial sums and the LDS histogram belong to the wave's CURRENT window
//             (index n_bins - 1 - bin for d < 0, n_bins + bin for d > 0: the two-sided histogram in the order of d, small |d| in the
//             middle); when the window changes the sums fold, the pair's words are stored and the cell's are added with integer
//             atomics (float-ordered min / max: the sign decides between a signed min and an unsigned max of the word).
//   LDS       2 n_bins words a wave (32 KiB at 4 096 bins, 8 KiB at the default), four waves a block, plus 8 B per edge.
// No index depends on the data being sorted or matched: a start that is not in the row is a counted `unmatched`, a slot at or
// past m_x is no row, every window index is below W'.  Rows that are not ascending give meaningless counts, nothing else.
//
// The per-row rules (lower_bound_from, match_start, arrival_of, fold64, order keys) and the sequential statement of one pair
// (pair_statement) are AF_HD text without a HIP include: gfx950 device code and, under g++, what tests/hostcheck/paired_main.cpp
// runs under the sanitizers.
#pragma once

#include <stdint.h>

#include "af_arrival_counts.hpp"
#include "af_latency_histogram.hpp"

namespace afpr {

constexpr uint32_t kSkip = 0xFFFFFFFFu;            // AF_POOL_SKIP
constexpr uint32_t kNone = 0xFFFFFFFFu;            // AF_PAIR_NONE: no row
constexpr uint32_t kMaxThresholds = 64;            // AF_MAX_PAIR_THRESHOLDS: one per lane
constexpr uint32_t kThreads = 256;                 // four waves a workgroup
constexpr uint32_t kWaves = kThreads / 64u;
constexpr uint32_t kMatchRows = 4096;              // clock rows of one work item of af_pairs_match
constexpr uint32_t kLdsPairWindows = 1023;         // windows whose edges af_pairs_reduce keeps in LDS (8 (W + 1) B <= 8 KiB)
constexpr uint32_t kMaxBlocks = 1u << 16;          // workgroups of a launch; the work items beyond are taken grid-stride
constexpr uint32_t kPairCounts = 5, kCellCounts = 8, kTails = 4;
enum { kBoth = 0, kOnlyA = 1, kOnlyB = 2, kNeither = 3, kNan = 4, kSlower = 5, kFaster = 6, kEqual = 7 };
enum { kUnderPos = 0, kUnderNeg = 1, kOverPos = 2, kOverNeg = 3 };

AF_HD uint64_t bits_of(double x) {
    uint64_t u;
    __builtin_memcpy(&u, &x, 8);
    return u;
}
AF_HD double double_of(uint64_t u) {
    double x;
    __builtin_memcpy(&x, &u, 8);
    return x;
}
// a u64 that orders like the f64 value, -0.0 below +0.0 (not for NaN), and back
AF_HD uint64_t order_key(double x) {
    const uint64_t u = bits_of(x);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
AF_HD double key_value(uint64_t k) { return double_of((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k); }
constexpr uint64_t kKeyPosInf = 0xFFF0000000000000ull, kKeyNegInf = 0x000FFFFFFFFFFFFFull;   // order_key(+inf), order_key(-inf)

// #{ k < n : row[k] < x } of an ascending row: np.searchsorted(row[:n], x, side="left"); a NaN x: 0 here, and matches nothing
AF_HD uint32_t lower_bound(const double* row, uint32_t n, double x) {
    uint32_t lo = 0u;
    while (n > 0u) {
        const uint32_t half = n >> 1;
        if (row[lo + half] < x) {
            lo += half + 1u;
            n -= half + 1u;
        } else {
            n = half;
        }
    }
    return lo;
}

// the same count from a guess: gallop 1, 2, 4 ... entries away from it in the direction the entry at the guess points, then
// search the bracket.  Any guess gives the same count on an ascending row; every probe is below m.
AF_HD uint32_t lower_bound_from(const double* row, uint32_t m, double x, uint32_t guess) {
    if (m == 0u) return 0u;
    const uint32_t h = guess < m ? guess : m - 1u;
    if (row[h] < x) {   // the count lies in (h, m]
        uint32_t base = h + 1u, step = 1u;
        while (m - base >= step && row[base + step - 1u] < x) {
            base += step;
            step <<= 1;
        }
        const uint32_t room = m - base;
        return base + lower_bound(row + base, room < step - 1u ? room : step - 1u, x);
    }
    uint32_t top = h, step = 1u;   // the count lies in [0, top]: row[top] is not below x
    while (top >= step && !(row[top - step] < x)) {
        top -= step;
        step <<= 1;
    }
    const uint32_t lo = top >= step ? top - step + 1u : 0u;   // (row[top - step] < x: the count is above top - step)
    return lo + lower_bound(row + lo, top - lo, x);
}

// THE MATCH of one start: `pos` = its count in the row; the arrival index when A[pos] is the start bit for bit, else kNone
AF_HD uint32_t match_start(const double* row, uint32_t m, double start, uint32_t guess, uint32_t& pos) {
    pos = lower_bound_from(row, m, start, guess);
    return pos < m && bits_of(row[pos]) == bits_of(start) ? pos : kNone;
}

// THE STATE AND DELTA of one arrival from its two slots; a slot at or past m_x names no row
struct Arrival {
    uint32_t state;   // bit 0: a, bit 1: b
    double d, lat_a;  // of state 3
};
AF_HD Arrival arrival_of(uint32_t ra, uint32_t rb, const double* clock_a, uint32_t m_a, const double* clock_b, uint32_t m_b) {
    Arrival r{(ra < m_a ? 1u : 0u) | (rb < m_b ? 2u : 0u), 0.0, 0.0};
    if (r.state == 3u) {
        r.lat_a = clock_a[2u * (uint64_t)ra + 1u] - clock_a[2u * (uint64_t)ra];
        const double lat_b = clock_b[2u * (uint64_t)rb + 1u] - clock_b[2u * (uint64_t)rb];
        r.d = lat_b - r.lat_a;
    }
    return r;
}

// the window of an arrival time from the rank of an earlier one (W > 0), or kNone; `rank` receives this one's
template <class EdgePtr>
AF_HD uint32_t window_from(EdgePtr e, uint32_t W, double t, uint32_t from, uint32_t& rank) {
    rank = afac::edge_rank_from(e, W + 1u, t, from);
    return rank >= 1u && rank <= W ? rank - 1u : kNone;
}

// THE FIXED-ORDER SUM: the 64 lanes' partial sums to one
AF_HD double fold64(double* part) {
    for (uint32_t h = 32u; h > 0u; h >>= 1)
        for (uint32_t l = 0u; l < h; ++l) part[l] += part[l + h];
    return part[0];
}

// what the delta of a `both` arrival adds to, beyond the sums: kNan / kSlower / kFaster / kEqual, and for a non-zero d its entry
// among the bins of |d| (n_bins: under, n_bins + 1: over)
AF_HD uint32_t delta_kind(double d, const aflh::Binning& b, uint32_t& entry) {
    entry = 0u;
    if (d != d) return kNan;
    if (d == 0.0) return kEqual;
    entry = aflh::bin_of_latency(d > 0.0 ? d : -d, b);
    return d > 0.0 ? kSlower : kFaster;
}

// The sequential statement of ONE pair.  slot_a / slot_b [n_draw] receive the join (kNone behind m and where no row maps);
// pair_counts [W'][5], pair_sums [W'][2], unmatched [2] are written; the cell words of the pair's group -- cell_counts [W'][8],
// above [W'][T], min_key / max_key [W'] (order keys: kKeyPosInf / kKeyNegInf when empty), hist [W'][2][n_bins], tails [W'][4] --
// are added to, or left alone when add_cells is false (a skipped pair).
AF_HD void pair_statement(const double* A, uint32_t n_draw, const double* clock_a, uint32_t m_a, const double* clock_b, uint32_t m_b,
                          const double* edges, uint32_t W, const double* thresholds, uint32_t T, const aflh::Binning& bin, bool add_cells,
                          uint32_t* slot_a, uint32_t* slot_b, uint32_t* pair_counts, double* pair_sums, uint32_t* unmatched,
                          uint64_t* cell_counts, uint64_t* above, uint64_t* min_key, uint64_t* max_key, uint32_t* hist, uint32_t* tails) {
    const uint32_t wins = W ? W : 1u, B = bin.n_bins;
    const uint32_t m = afac::row_length(A, n_draw);
    for (uint32_t j = 0; j < n_draw; ++j) slot_a[j] = slot_b[j] = kNone;
    for (uint32_t side = 0; side < 2u; ++side) {
        const double* ck = side ? clock_b : clock_a;
        uint32_t* slot = side ? slot_b : slot_a;
        const uint32_t rows = side ? m_b : m_a;
        uint32_t guess = 0u, set = 0u;
        for (uint32_t i = 0; i < rows; ++i) {
            uint32_t pos = 0u;
            const uint32_t j = match_start(A, m, ck[2u * (uint64_t)i], guess, pos);
            guess = pos + 1u;
            if (j != kNone && i < slot[j]) {
                set += slot[j] == kNone ? 1u : 0u;
                slot[j] = i;
            }
        }
        unmatched[side] = rows - set;
    }
    for (uint32_t w = 0; w < wins; ++w) {
        for (uint32_t k = 0; k < kPairCounts; ++k) pair_counts[w * kPairCounts + k] = 0u;
        pair_sums[2u * w] = pair_sums[2u * w + 1u] = 0.0;
    }
    double part_d[64], part_a[64];
    uint32_t cur = kNone, rank = 0u;
    auto flush = [&]() {
        if (cur == kNone) return;
        pair_sums[2u * cur] = fold64(part_d);
        pair_sums[2u * cur + 1u] = fold64(part_a);
    };
    for (uint32_t j = 0; j < m; ++j) {
        uint32_t w = 0u;
        if (W) w = window_from(edges, W, A[j], rank, rank);
        if (w == kNone) continue;
        if (w != cur) {
            flush();
            cur = w;
            for (uint32_t l = 0; l < 64u; ++l) part_d[l] = part_a[l] = 0.0;
        }
        const Arrival r = arrival_of(slot_a[j], slot_b[j], clock_a, m_a, clock_b, m_b);
        const uint32_t state_slot = r.state == 3u ? kBoth : r.state == 1u ? kOnlyA : r.state == 2u ? kOnlyB : kNeither;
        pair_counts[w * kPairCounts + state_slot] += 1u;
        if (add_cells) cell_counts[w * kCellCounts + state_slot] += 1u;
        if (r.state != 3u) continue;
        uint32_t entry = 0u;
        const uint32_t kind = delta_kind(r.d, bin, entry);
        if (kind == kNan) {
            pair_counts[w * kPairCounts + kNan] += 1u;
            if (add_cells) cell_counts[w * kCellCounts + kNan] += 1u;
            continue;
        }
        part_d[j & 63u] += r.d;
        part_a[j & 63u] += r.lat_a;
        if (!add_cells) continue;
        cell_counts[w * kCellCounts + kind] += 1u;
        for (uint32_t t = 0; t < T; ++t)
            if (r.d > thresholds[t]) above[(uint64_t)w * T + t] += 1u;
        const uint64_t key = order_key(r.d);
        if (key < min_key[w]) min_key[w] = key;
        if (key > max_key[w]) max_key[w] = key;
        if (kind == kEqual) continue;
        const uint32_t neg = kind == kFaster ? 1u : 0u;
        if (entry < B) hist[((uint64_t)w * 2u + neg) * B + entry] += 1u;
        else tails[w * kTails + (entry == B ? kUnderPos : kOverPos) + neg] += 1u;
    }
    flush();
}

struct PairArgs {
    const double* clock;            // [n_scen][clock_cap][2]
    const uint32_t* counts;         // [n_scen][8]
    uint32_t clock_cap, cnt_completed_slot;
    const uint32_t* pair_a;         // [P], already at the chunk's first pair (as group, time_row and the outputs per pair below)
    const uint32_t* pair_b;
    const uint32_t* group;          // or null: all in group 0
    const uint32_t* time_row;
    const double* times;            // [n_time_rows][n_draw]
    uint32_t n_pairs, n_draw;       // the pairs of this chunk
    uint32_t n_win, wins;           // W and W' = max(W, 1)
    const double* edges;            // DEVICE [W + 1] (W > 0)
    const double* thresholds;       // DEVICE [T]
    uint32_t n_thr;
    uint32_t chunks;                // work items per (pair, side) of the match pass: ceil(clock_cap / kMatchRows)
    aflh::Binning bin;
    uint32_t* slot_a;               // [P][n_draw], 0xFF-filled before the match pass
    uint32_t* slot_b;
    uint32_t* pair_counts;          // [P][W'][5]
    double* pair_sums;              // [P][W'][2]
    uint32_t* unmatched;            // [P][2]
    unsigned long long* cell_counts;   // [C][8]
    unsigned long long* above;      // [C][T]
    double* extremes;               // [C][2], +inf / -inf before the first chunk
    uint32_t* hist;                 // [C][2][n_bins]
    uint32_t* tails;                // [C][4]
};

#if defined(__HIPCC__)
__device__ __forceinline__ uint32_t ballot_count(bool p) { return (uint32_t)__popcll(__ballot(p)); }
__device__ __forceinline__ double readlane_double(double x, uint32_t l) {   // (l uniform)
    const uint64_t u = bits_of(x);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, (int)l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), (int)l);
    return double_of(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ uint32_t stored_rows(const PairArgs& a, uint32_t s) {
    const uint32_t m = a.counts[(size_t)s * 8u + a.cnt_completed_slot];
    return m < a.clock_cap ? m : a.clock_cap;
}

// cells' extremes before the first chunk: +inf / -inf
__global__ void __launch_bounds__(256) af_pairs_init_extremes(double* extremes, uint64_t cells) {
    const uint64_t c = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (c >= cells) return;
    extremes[2u * c] = double_of(0x7FF0000000000000ull);
    extremes[2u * c + 1u] = double_of(0xFFF0000000000000ull);
}

__global__ void __launch_bounds__(kThreads) af_pairs_match(const PairArgs a) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t items = (uint64_t)a.n_pairs * 2u * a.chunks;
    for (uint64_t item = (uint64_t)blockIdx.x * kWaves + wave; item < items; item += (uint64_t)gridDim.x * kWaves) {
        const uint32_t p = (uint32_t)(item / (2u * a.chunks)), rest = (uint32_t)(item % (2u * a.chunks));
        const uint32_t side = rest / a.chunks;
        const uint64_t first = (uint64_t)(rest % a.chunks) * kMatchRows;
        const uint32_t s = side ? a.pair_b[p] : a.pair_a[p];
        const uint32_t rows = stored_rows(a, s);
        if (first >= rows) continue;
        const uint32_t r0 = (uint32_t)first, r1 = rows - r0 > kMatchRows ? r0 + kMatchRows : rows;
        const double* A = a.times + (size_t)a.time_row[p] * a.n_draw;
        const uint32_t m = afac::row_length(A, a.n_draw);
        const double2* ck = reinterpret_cast<const double2*>(a.clock) + (size_t)s * a.clock_cap;
        uint32_t* slot = (side ? a.slot_b : a.slot_a) + (size_t)p * a.n_draw;
        uint32_t guess = r0;   // (requests complete roughly in the order they were sent, few are lost)
        for (uint32_t base = r0; base < r1; base += 64u) {   // (uniform trip count)
            const uint32_t i = base + lane;
            const bool in = i < r1 && i >= base;
            uint32_t pos = 0u;
            if (in) {
                const double2 c = ck[i];
                const uint32_t mine = guess + lane < guess ? kNone : guess + lane;
                const uint32_t j = match_start(A, m, c.x, mine, pos);
                if (j != kNone) atomicMin(&slot[j], i);   // (j < m <= n_draw)
            }
            guess = (uint32_t)__builtin_amdgcn_readfirstlane((int)pos) + 64u;   // (lane 0 is in; pos <= m < 2^31)
            if (r1 - base <= 64u) break;   // (base + 64 could wrap)
        }
    }
}

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// min / max of a cell's extremes in float order with -0.0 below +0.0, by integer atomics on the word: words with the sign clear
// order like signed integers, words with it set in reverse as unsigned ones, and a set sign is above every clear one unsigned
__device__ __forceinline__ void atomic_min_double(double* p, double v) {
    const uint64_t u = bits_of(v);
    if (u >> 63) atomicMax(reinterpret_cast<unsigned long long*>(p), (unsigned long long)u);
    else atomicMin(reinterpret_cast<long long*>(p), (long long)u);
}
__device__ __forceinline__ void atomic_max_double(double* p, double v) {
    const uint64_t u = bits_of(v);
    if (u >> 63) atomicMin(reinterpret_cast<unsigned long long*>(p), (unsigned long long)u);
    else atomicMax(reinterpret_cast<long long*>(p), (long long)u);
}

// what a wave holds of its current window besides the LDS histogram
struct Current {
    uint32_t win;                    // the window, or kNone (the counters below: the same in every lane)
    uint32_t counts[kCellCounts];
    uint32_t tails[kTails];
    double sum_d, sum_a;             // per lane: the partial sums of lane l = j mod 64
    uint64_t kmin, kmax;             // per lane: order keys
    uint32_t above;                  // lane t: the deltas above thresholds[t]
    uint32_t lo, hi;                 // per lane: the lowest and highest word of the LDS histogram it added to
};
__device__ __forceinline__ void clear(Current& c) {
#pragma unroll
    for (uint32_t k = 0; k < kCellCounts; ++k) c.counts[k] = 0u;
#pragma unroll
    for (uint32_t k = 0; k < kTails; ++k) c.tails[k] = 0u;
    c.sum_d = c.sum_a = 0.0;
    c.kmin = kKeyPosInf;
    c.kmax = kKeyNegInf;
    c.above = 0u;
    c.lo = kNone;
    c.hi = 0u;
}

// the current window's words: the pair's are stored, the cell's added (g != kSkip); the LDS histogram is all zero afterwards
__device__ __forceinline__ void flush(const PairArgs& a, uint32_t* lh, uint32_t p, uint32_t g, Current& c, uint32_t lane) {
    if (c.win == kNone) return;   // (uniform)
    const uint32_t B = a.bin.n_bins;
    double sd = c.sum_d, sa = c.sum_a;
    uint64_t kmin = c.kmin, kmax = c.kmax;
    uint32_t lo = c.lo, hi = c.hi;
#pragma unroll
    for (int h = 32; h > 0; h >>= 1) {   // (fold64: lane l < h takes lane l + h; what the lanes at or above h hold is not used)
        sd += __shfl_down(sd, h, 64);
        sa += __shfl_down(sa, h, 64);
        const uint64_t k0 = __shfl_xor((unsigned long long)kmin, h, 64), k1 = __shfl_xor((unsigned long long)kmax, h, 64);
        kmin = k0 < kmin ? k0 : kmin;
        kmax = k1 > kmax ? k1 : kmax;
        const uint32_t l2 = (uint32_t)__shfl_xor((int)lo, h, 64), h2 = (uint32_t)__shfl_xor((int)hi, h, 64);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    const size_t pw = (size_t)p * a.wins + c.win;
    if (lane == 0u) {
#pragma unroll
        for (uint32_t k = 0; k < kPairCounts; ++k) a.pair_counts[pw * kPairCounts + k] = c.counts[k];
        a.pair_sums[2u * pw] = sd;
        a.pair_sums[2u * pw + 1u] = sa;
    }
    wave_sync();
    if (g != kSkip) {
        const size_t cell = (size_t)g * a.wins + c.win;
        if (lane == 0u) {
#pragma unroll
            for (uint32_t k = 0; k < kCellCounts; ++k)
                if (c.counts[k]) atomicAdd(&a.cell_counts[cell * kCellCounts + k], (unsigned long long)c.counts[k]);
#pragma unroll
            for (uint32_t k = 0; k < kTails; ++k)
                if (c.tails[k]) atomicAdd(&a.tails[cell * kTails + k], c.tails[k]);
            if (kmin <= kmax) {   // (some delta was not NaN)
                atomic_min_double(&a.extremes[2u * cell], key_value(kmin));
                atomic_max_double(&a.extremes[2u * cell + 1u], key_value(kmax));
            }
        }
        if (lane < a.n_thr && c.above) atomicAdd(&a.above[cell * a.n_thr + lane], (unsigned long long)c.above);
        if (lo <= hi) {   // (some lane added to a bin: lo <= hi < 2 n_bins)
            uint32_t* out = a.hist + cell * 2u * B;
            for (uint32_t i = (lo & ~63u) + lane; i <= hi; i += 64u) {
                const uint32_t n = lh[i];
                if (n) {
                    atomicAdd(&out[i < B ? B + (B - 1u - i) : i - B], n);   // (words below B: d < 0, bin B - 1 - i of the second half)
                    lh[i] = 0u;
                }
            }
        }
    } else if (lo <= hi) {
        for (uint32_t i = (lo & ~63u) + lane; i <= hi; i += 64u) lh[i] = 0u;
    }
    const uint32_t win = c.win;
    clear(c);
    c.win = win;
    wave_sync();   // (the next window adds to these words)
}

// one pair; ONE wave
template <class EdgePtr>
__device__ __forceinline__ void wave_pair(const PairArgs& a, uint32_t p, EdgePtr e, uint32_t* lh, uint32_t lane) {
    const uint32_t W = a.n_win, B = a.bin.n_bins, T = a.n_thr;
    const uint32_t sa = a.pair_a[p], sb = a.pair_b[p], g = a.group ? a.group[p] : 0u;
    const uint32_t m_a = stored_rows(a, sa), m_b = stored_rows(a, sb);
    const double* A = a.times + (size_t)a.time_row[p] * a.n_draw;
    const uint32_t m = afac::row_length(A, a.n_draw);
    const double* ck_a = a.clock + (size_t)sa * a.clock_cap * 2u;
    const double* ck_b = a.clock + (size_t)sb * a.clock_cap * 2u;
    const uint32_t* slot_a = a.slot_a + (size_t)p * a.n_draw;
    const uint32_t* slot_b = a.slot_b + (size_t)p * a.n_draw;
    const double thr = lane < T ? a.thresholds[lane] : 0.0;
    Current cur;
    clear(cur);
    cur.win = kNone;
    uint32_t set_a = 0u, set_b = 0u, last = 0u;
    for (uint32_t base = 0u; base < m; base += 64u) {   // (uniform trip count: the ballots below are wave-wide)
        const uint32_t j = base + lane;
        const bool in = j < m;
        uint32_t w = in ? 0u : kNone, rank = W + 1u;
        Arrival r{0u, 0.0, 0.0};
        if (in) {
            if (W) w = window_from(e, W, A[j], last, rank);
            r = arrival_of(slot_a[j], slot_b[j], ck_a, m_a, ck_b, m_b);
        }
        last = (uint32_t)__builtin_amdgcn_readlane((int)rank, 63);   // (an ascending row: every later time has at least this rank)
        set_a += ballot_count(in && (r.state & 1u));
        set_b += ballot_count(in && (r.state & 2u));
        uint32_t entry = 0u;
        const uint32_t kind = r.state == 3u ? delta_kind(r.d, a.bin, entry) : kNone;
        unsigned long long todo = __ballot(in && w != kNone);
        while (todo) {   // one turn per distinct window of the step
            const int leader = __ffsll((long long)todo) - 1;
            const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)w, leader);
            const bool mine = in && w == v;
            const unsigned long long same = __ballot(mine);
            if (v != cur.win) {   // (uniform)
                flush(a, lh, p, g, cur, lane);
                cur.win = v;
            }
            cur.counts[kBoth] += ballot_count(mine && r.state == 3u);
            cur.counts[kOnlyA] += ballot_count(mine && r.state == 1u);
            cur.counts[kOnlyB] += ballot_count(mine && r.state == 2u);
            cur.counts[kNeither] += ballot_count(mine && r.state == 0u);
            const bool ok = mine && r.state == 3u && kind != kNan;
            if (__ballot(mine && r.state == 3u)) {   // (uniform)
                cur.counts[kNan] += ballot_count(mine && kind == kNan);
                cur.counts[kSlower] += ballot_count(mine && kind == kSlower);
                cur.counts[kFaster] += ballot_count(mine && kind == kFaster);
                cur.counts[kEqual] += ballot_count(mine && kind == kEqual);
                const bool sided = ok && kind != kEqual;
                if (__ballot(sided && entry >= B)) {   // (uniform; rare)
                    cur.tails[kUnderPos] += ballot_count(sided && entry == B && kind == kSlower);
                    cur.tails[kUnderNeg] += ballot_count(sided && entry == B && kind == kFaster);
                    cur.tails[kOverPos] += ballot_count(sided && entry == B + 1u && kind == kSlower);
                    cur.tails[kOverNeg] += ballot_count(sided && entry == B + 1u && kind == kFaster);
                }
                for (uint32_t t = 0; t < T; ++t) {   // (lane t keeps the count of threshold t)
                    const double th = readlane_double(thr, t);
                    const uint32_t n = ballot_count(ok && r.d > th);
                    if (lane == t) cur.above += n;
                }
                if (ok) {
                    cur.sum_d += r.d;
                    cur.sum_a += r.lat_a;
                    const uint64_t key = order_key(r.d);
                    cur.kmin = key < cur.kmin ? key : cur.kmin;
                    cur.kmax = key > cur.kmax ? key : cur.kmax;
                    if (sided && entry < B) {
                        const uint32_t idx = kind == kFaster ? B - 1u - entry : B + entry;
                        atomicAdd(&lh[idx], 1u);
                        cur.lo = idx < cur.lo ? idx : cur.lo;
                        cur.hi = idx > cur.hi ? idx : cur.hi;
                    }
                }
            }
            todo &= ~same;
        }
        if (m - base <= 64u) break;   // (base + 64 could wrap)
    }
    flush(a, lh, p, g, cur, lane);
    if (lane == 0u) {
        a.unmatched[2u * (size_t)p] = m_a - (set_a < m_a ? set_a : m_a);
        a.unmatched[2u * (size_t)p + 1u] = m_b - (set_b < m_b ? set_b : m_b);
    }
}

// kLds: the edges lie in dynamic LDS.  Dynamic LDS: kLds [W + 1] f64 edges (W > 0), then [kWaves][2 n_bins] u32.
template <bool kLds>
__global__ void __launch_bounds__(kThreads) af_pairs_reduce(const PairArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char afpr_dyn[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t W = a.n_win, B2 = 2u * a.bin.n_bins, ne = kLds && W ? W + 1u : 0u;
    double* le = reinterpret_cast<double*>(afpr_dyn);
    uint32_t* lh = reinterpret_cast<uint32_t*>(afpr_dyn + (size_t)ne * 8u) + (size_t)wave * B2;
    for (uint32_t k = threadIdx.x; k < ne; k += kThreads) le[k] = a.edges[k];
    for (uint32_t i = lane; i < B2; i += 64u) lh[i] = 0u;
    __syncthreads();   // (the only block-wide barrier: the waves go their own ways below)
    for (uint64_t p = (uint64_t)blockIdx.x * kWaves + wave; p < a.n_pairs; p += (uint64_t)gridDim.x * kWaves) {
        if (kLds) wave_pair(a, (uint32_t)p, (const double*)le, lh, lane);
        else wave_pair(a, (uint32_t)p, a.edges, lh, lane);
    }
}
#endif  // __HIPCC__

}  // namespace afpr
