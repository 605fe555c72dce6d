// af_latency_histogram.hpp -- mergeable LOG-LINEAR LATENCY HISTOGRAMS per window and group (af_engine_summarize_latency_histogram,
// launched by engine.hip): the distribution of a cell instead of finished numbers about it.  An HDR-style sketch whose binning is
// defined on the BIT PATTERN of the f64 latency -- no logarithm, no rounding question --, counted with integer + only: two results
// over the same cells add word by word (devices, member splits, saved sweeps), windows and groups coarsen by summing cells, and
// quantile brackets at any level are read off afterwards.
//
// DEFINITION.  Scenario s has m_s = min(counts[s][completed], clock_cap) stored rows (start_i, finish_i).
//   binning   sub_bits m in 0 .. 8, min_exp e >= -1022, octaves o >= 1, e + o <= 1023, n_bins = o << m <= kMaxBins.  Octave
//             [2^(e + k), 2^(e + k + 1)) is cut into 2^m bins of equal width: the relative width of a bin is 2^-m.
//   latency   x = finish - start, one f64 subtraction; bits = its 64-bit pattern.
//             x NaN -> nan;  x < 2^e (zeros, -0.0, negatives, denormals, -inf) -> under;  x >= 2^(e + o) (+inf) -> over;
//             else bin (bits >> (52 - m)) - ((e + 1023) << m): integer arithmetic on the word.  Bin b covers [E[b], E[b + 1]),
//             E[b] = ldexp(1 + (b & (2^m - 1)) / 2^m, e + (b >> m)), exact in f64.
//   window    af_exemplars.hpp's: with edges e[0] < ... < e[W], window w where e[w] < t <= e[w + 1], t = finish (by finish) or
//             start (by arrival); t <= e[0], t > e[W] or t NaN: no cell.  A mask on every row: no order of the rows is needed or
//             checked.  Without edges (W == 0) one window with no condition on time.  W' = max(W, 1).
//   outputs   of cell c = g W' + w: count[c] u64 = the rows of the cell; hist[c][n_bins], under[c], over[c], nan[c] u32 with
//             under + over + nan + sum(hist) == count.  The cells of an empty or skipped group are all zero.
//
// KERNEL.  One streaming pass over the clock rows; nothing else of size is read.
//   work      a WAVE per (scenario, chunk of kChunkRows rows), four waves a workgroup, grid-stride over the work items.  A lane
//             loads its (start, finish) pair as one 16-byte word, kUnroll loads in flight, 64 consecutive rows a step.
//   per row   one subtraction, the bit rule (bin_of_latency) and the window by binary search (afex::window_of_time) over the
//             edges, which lie in LDS up to kLdsHistogramWindows windows and are read from global memory above.
//   counting  every wave has an LDS histogram of n_bins words for ONE window, its CURRENT window; under / over / nan and the
//             rows of that window are counted by __ballot into registers.  The lanes of a step are taken window by window (the
//             leader loop of af_exemplars.hpp).  A window that holds at least kSwitchRows rows of the step becomes the current
//             one: the non-zero words of the LDS histogram between the lowest and the highest bin touched are added to the old
//             window's cell by integer atomics and cleared.  By finish the rows are sorted and the window only advances; by
//             arrival `start` is nearly sorted.  Rows of any other window -- stragglers, TINY windows of fewer than kSwitchRows
//             rows a step, unsorted clocks -- are added to their cell in HBM directly, so no order is relied on and a step
//             switches at most twice.
//   same bin  (latencies of a steady window crowd into a few bins) the lanes of a window compare their bin with the leader's
//             (one readlane, one __ballot): the leader adds the popcount of the agreeing lanes at once, a lane that disagrees
//             adds 1.
//   LDS       BUDGET: af_series_histogram.hpp's -- at most 4 096 words = 16 KiB a wave (under / over / nan live in registers),
//             64 KiB a block of four waves, plus 8 B per edge up to kLdsHistogramWindows (8 KiB): two blocks fit the 160 KiB of
//             a CU.  A call asks for what its binning needs: 16 KiB + the edges at the default 1 024 bins.
//   The entry zeroes the outputs first; every addition to a cell is an integer atomic, every store a plain vector store.
// Only integer + combines: the result cannot depend on the launch, on the batch a scenario sits in, or on the run.
// Scratch (engine-owned, shared with the other analyzers): 8 B per edge.  No per-row and no per-cell records.
//
// The per-row rule (bin_of_latency, row_cell) and the sequential statement of a scenario (scenario_cells) are AF_HD text without
// a HIP include: gfx950 device code and, under g++, what tests/hostcheck/latency_histogram_main.cpp runs under the sanitizers.
#pragma once

#include <stdint.h>

#include "af_exemplars.hpp"

namespace aflh {

constexpr uint32_t kMaxBins = 4096;                // AF_MAX_LATENCY_HISTOGRAM_BINS: the LDS histogram of one wave, in words
constexpr uint32_t kMaxSubBits = 8;
constexpr uint32_t kSkip = 0xFFFFFFFFu;            // AF_POOL_SKIP
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kThreads = 256;                 // four waves, four work items
constexpr uint32_t kWaves = kThreads / 64u;
constexpr uint32_t kUnroll = 4;                    // 16-byte loads a lane has in flight
constexpr uint32_t kChunkRows = 16384;             // rows of one work item: one flush of the LDS histogram per window it meets
constexpr uint32_t kSwitchRows = 32;               // rows of a step a window needs to become the wave's current window
constexpr uint32_t kLdsHistogramWindows = 1023;    // windows whose edges the kernel keeps in LDS (8 (W + 1) B <= 8 KiB)
constexpr uint32_t kMaxBlocks = 1u << 16;          // workgroups of a launch; the work items beyond are taken grid-stride
static_assert(kChunkRows % (kUnroll * 64u) == 0u, "a chunk is whole steps");

struct Binning {
    uint32_t sub_bits;   // m
    int32_t min_exp;     // e
    uint32_t octaves;    // o
    uint32_t n_bins;     // o << m
};

// is (m, e, o) a binning?  Then b holds it with its n_bins.
AF_HD bool make_binning(uint32_t sub_bits, int32_t min_exp, uint32_t octaves, Binning& b) {
    if (sub_bits > kMaxSubBits || min_exp < -1022 || octaves == 0u || octaves > kMaxBins) return false;
    if ((int64_t)min_exp + (int64_t)octaves > 1023) return false;
    const uint32_t n = octaves << sub_bits;   // (<= 4 096 << 8: no wrap)
    if (n > kMaxBins) return false;
    b = Binning{sub_bits, min_exp, octaves, n};
    return true;
}

// THE BIT RULE: the ENTRY of a latency among the n_bins + 3 counters of a cell: its bin, or n_bins (under), n_bins + 1 (over),
// n_bins + 2 (nan).  Non-negative f64 values order like their bit patterns; 2^e and 2^(e + o) are normal numbers.
AF_HD uint32_t bin_of_latency(double x, const Binning& b) {
    uint64_t bits;
    __builtin_memcpy(&bits, &x, 8);
    if ((bits & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull) return b.n_bins + 2u;   // NaN, either sign
    if (bits >> 63) return b.n_bins;                                                     // -0.0, negatives, -inf
    const uint64_t e0 = (uint64_t)(b.min_exp + 1023);                                    // 1 .. 2 045
    if (bits < (e0 << 52)) return b.n_bins;                                              // +0.0, denormals, below 2^e
    if (bits >= ((e0 + b.octaves) << 52)) return b.n_bins + 1u;                          // (e0 + o <= 2 046; +inf is above)
    return (uint32_t)((bits >> (52u - b.sub_bits)) - (e0 << b.sub_bits));
}

// THE PER-ROW RULE: is the row in a cell, and then its window (0 without edges) and its entry
template <class EdgePtr>
AF_HD bool row_cell(double start, double finish, EdgePtr e, uint32_t W, bool by_arrival, const Binning& b, uint32_t& w, uint32_t& entry) {
    w = 0u;
    if (W) {
        w = afex::window_of_time(e, W, by_arrival ? start : finish);
        if (w == afex::kNone) return false;
    }
    entry = bin_of_latency(finish - start, b);
    return true;
}

// The sequential statement of one scenario: its m rows into the W' cells of its group, whose counters the caller zeroed.
// count [W'] u64, hist [W'][n_bins], under / over / nan [W'].
AF_HD void scenario_cells(const double* rows, uint32_t m, const double* edges, uint32_t W, bool by_arrival, const Binning& b,
                          uint64_t* count, uint32_t* hist, uint32_t* under, uint32_t* over, uint32_t* nan) {
    for (uint32_t i = 0; i < m; ++i) {
        uint32_t w = 0u, entry = 0u;
        if (!row_cell(rows[2u * (uint64_t)i], rows[2u * (uint64_t)i + 1u], edges, W, by_arrival, b, w, entry)) continue;
        count[w] += 1u;
        if (entry < b.n_bins) hist[(uint64_t)w * b.n_bins + entry] += 1u;
        else if (entry == b.n_bins) under[w] += 1u;
        else if (entry == b.n_bins + 1u) over[w] += 1u;
        else nan[w] += 1u;
    }
}

struct LhArgs {
    const double* clock;            // [n][clock_cap][2]
    const uint32_t* counts;         // [n][8]
    uint32_t clock_cap, cnt_completed_slot;
    const uint32_t* group;          // [n], or null: all in group 0
    uint32_t n_scen, n_win, wins;   // W and W' = max(W, 1)
    const double* edges;            // DEVICE [W + 1] (W > 0)
    uint32_t by_arrival;
    uint32_t chunks;                // work items per scenario: ceil(clock_cap / kChunkRows)
    Binning bin;
    unsigned long long* count;      // [C]
    uint32_t* hist;                 // [C][n_bins]
    uint32_t* under;                // [C] or null
    uint32_t* over;                 // [C] or null
    uint32_t* nan;                  // [C] or null
};

#if defined(__HIPCC__)
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t ballot_count(bool p) { return (uint32_t)__popcll(__ballot(p)); }

// what a wave holds of its current window besides the LDS histogram (the counters: the same in every lane)
struct Current {
    uint32_t win;                    // the window, or kNone: none yet
    uint32_t rows, under, over, nan;
    uint32_t lo, hi;                 // per lane: the lowest and the highest bin it added to
};

// the current window's counts to its cell; the LDS histogram is all zero afterwards
__device__ __forceinline__ void flush(const LhArgs& a, uint32_t* lh, size_t cell0, Current& c, uint32_t lane) {
    if (c.win == kNone) return;   // (uniform)
    const size_t cell = cell0 + c.win;
    uint32_t lo = c.lo, hi = c.hi;
#pragma unroll
    for (int j = 32; j > 0; j >>= 1) {
        const uint32_t l2 = (uint32_t)__shfl_xor((int)lo, j, 64), h2 = (uint32_t)__shfl_xor((int)hi, j, 64);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    wave_sync();
    if (lo <= hi) {   // (some lane added to a bin: lo <= hi < n_bins)
        uint32_t* out = a.hist + cell * a.bin.n_bins;
        for (uint32_t i = (lo & ~63u) + lane; i <= hi; i += 64u) {
            const uint32_t n = lh[i];
            if (n) {
                atomicAdd(&out[i], n);
                lh[i] = 0u;
            }
        }
    }
    if (lane == 0u) {
        if (c.rows) atomicAdd(&a.count[cell], (unsigned long long)c.rows);
        if (a.under && c.under) atomicAdd(&a.under[cell], c.under);
        if (a.over && c.over) atomicAdd(&a.over[cell], c.over);
        if (a.nan && c.nan) atomicAdd(&a.nan[cell], c.nan);
    }
    c.rows = c.under = c.over = c.nan = 0u;
    c.lo = kNone;
    c.hi = 0u;
    wave_sync();   // (the next window adds to these words)
}

// one row of entry `entry` to `cell` in HBM
__device__ __forceinline__ void add_cell(const LhArgs& a, size_t cell, uint32_t entry) {
    const uint32_t B = a.bin.n_bins;
    if (entry < B) atomicAdd(&a.hist[cell * B + entry], 1u);
    else if (entry == B) {
        if (a.under) atomicAdd(&a.under[cell], 1u);
    } else if (entry == B + 1u) {
        if (a.over) atomicAdd(&a.over[cell], 1u);
    } else if (a.nan) atomicAdd(&a.nan[cell], 1u);
}

// rows [r0, r1) of one scenario, 0 < r1 - r0 <= kChunkRows, into the cells cell0 .. cell0 + W' - 1 of its group; ONE wave
template <class EdgePtr>
__device__ __forceinline__ void wave_rows(const LhArgs& a, const double2* ck, uint32_t r0, uint32_t r1, EdgePtr e, uint32_t* lh,
                                          size_t cell0, uint32_t lane) {
    const uint32_t W = a.n_win, B = a.bin.n_bins;
    const bool by_arrival = a.by_arrival != 0u;
    Current cur{W ? kNone : 0u, 0u, 0u, 0u, 0u, kNone, 0u};
    for (uint32_t base = r0; base < r1; base += kUnroll * 64u) {   // (uniform trip count: the ballots below are wave-wide)
        double2 c[kUnroll];
#pragma unroll
        for (uint32_t u = 0; u < kUnroll; ++u) {
            const uint32_t i = base + u * 64u + lane;
            c[u] = i < r1 && i >= base ? ck[i] : double2{0.0, 0.0};   // (i >= base: no wrap)
        }
#pragma unroll
        for (uint32_t u = 0; u < kUnroll; ++u) {   // 64 rows a step, in row order
            const uint32_t i = base + u * 64u + lane;
            uint32_t w = 0u, entry = 0u;
            const bool in = i < r1 && i >= base && row_cell(c[u].x, c[u].y, e, W, by_arrival, a.bin, w, entry);
            unsigned long long todo = __ballot(in);
            while (todo) {   // one turn per distinct window of the step
                const int leader = __ffsll((long long)todo) - 1;
                const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)w, leader);
                const bool mine = in && w == v;
                const unsigned long long same = __ballot(mine);
                const uint32_t rows = (uint32_t)__popcll(same);
                if (v != cur.win && rows >= kSwitchRows) {   // (uniform)
                    flush(a, lh, cell0, cur, lane);
                    cur.win = v;
                }
                if (v == cur.win) {
                    const bool binned = mine && entry < B;
                    cur.rows += rows;
                    if (__ballot(mine && entry >= B)) {   // (uniform; rare)
                        cur.under += ballot_count(mine && entry == B);
                        cur.over += ballot_count(mine && entry == B + 1u);
                        cur.nan += ballot_count(mine && entry == B + 2u);
                    }
                    const uint32_t e_first = (uint32_t)__builtin_amdgcn_readlane((int)entry, leader);
                    const bool agree = binned && entry == e_first;
                    const uint32_t n_agree = ballot_count(agree);
                    if (binned) {
                        if (!agree) atomicAdd(&lh[entry], 1u);
                        else if ((int)lane == leader) atomicAdd(&lh[entry], n_agree);   // (the leader agrees with itself)
                        cur.lo = entry < cur.lo ? entry : cur.lo;
                        cur.hi = entry > cur.hi ? entry : cur.hi;
                    }
                } else {
                    const size_t cell = cell0 + v;
                    if ((int)lane == leader) atomicAdd(&a.count[cell], (unsigned long long)rows);
                    if (mine) add_cell(a, cell, entry);
                }
                todo &= ~same;
            }
        }
        if (r1 - base <= kUnroll * 64u) break;   // (base + kUnroll * 64 could wrap)
    }
    flush(a, lh, cell0, cur, lane);
}

// kLds: the edges lie in dynamic LDS.  Dynamic LDS: kLds [W + 1] f64 edges (W > 0), then [kWaves][n_bins] u32.
template <bool kLds>
__global__ void __launch_bounds__(kThreads) af_latency_histogram_kernel(const LhArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char aflh_dyn[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t W = a.n_win, B = a.bin.n_bins, ne = kLds && W ? W + 1u : 0u;
    double* le = reinterpret_cast<double*>(aflh_dyn);
    uint32_t* lh = reinterpret_cast<uint32_t*>(aflh_dyn + (size_t)ne * 8u) + (size_t)wave * B;
    for (uint32_t k = threadIdx.x; k < ne; k += kThreads) le[k] = a.edges[k];
    for (uint32_t i = lane; i < B; i += 64u) lh[i] = 0u;
    __syncthreads();   // (the only block-wide barrier: the waves go their own ways below)
    const uint64_t items = (uint64_t)a.n_scen * a.chunks;
    for (uint64_t item = (uint64_t)blockIdx.x * kWaves + wave; item < items; item += (uint64_t)gridDim.x * kWaves) {
        const uint32_t s = (uint32_t)(item / a.chunks);
        const uint64_t first = (item % a.chunks) * (uint64_t)kChunkRows;
        const uint32_t g = a.group ? a.group[s] : 0u;
        if (g == kSkip) continue;
        uint32_t m = a.counts[(size_t)s * 8u + a.cnt_completed_slot];
        if (m > a.clock_cap) m = a.clock_cap;
        if (first >= m) continue;
        const uint32_t r0 = (uint32_t)first, r1 = m - r0 > kChunkRows ? r0 + kChunkRows : m;
        const double2* ck = reinterpret_cast<const double2*>(a.clock) + (size_t)s * a.clock_cap;
        const size_t cell0 = (size_t)g * a.wins;
        if (kLds) wave_rows(a, ck, r0, r1, (const double*)le, lh, cell0, lane);
        else wave_rows(a, ck, r0, r1, a.edges, lh, cell0, lane);
    }
}
#endif  // __HIPCC__

}  // namespace aflh
