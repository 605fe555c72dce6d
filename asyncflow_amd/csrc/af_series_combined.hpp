// Combinations ACROSS the sampled series per tick, then per (group, window of ticks): fleet totals and the imbalance between
// servers (af_engine_summarize_series_combined).
// A combination c is (op, columns): op is sum, min, max or spread (max - min) of the words of its columns in ONE sample row;
// the columns are all integer series or all ram_in_use columns.  Per-tick value of a row:
//   integer columns   the words as u32: the exact u64 sum, the smallest / largest word, their difference; x = (double)v
//   ram columns       each word as (double)(float)word: the f64 sum in ascending column order, left to right, one rounding an
//                     addition, starting from the first column's value (the sum of -0.0s is -0.0); min / max in the IEEE total
//                     order on the non-NaN values (-0.0 below +0.0); spread = max - min, one f64 subtraction
// The cells are af_series_windows.hpp's: window w of scenario s is its sample rows [min(b[w], m_s), min(b[w + 1], m_s)), m_s =
// min(counts[s][ticks], tick_cap); rows at or past m_s and the padding words of a row are never read.
//   partial   a WAVE per (scenario, run of consecutive windows), one window at a time, A LANE PER ROW: lane l takes rows r0 + l,
//             r0 + l + 64, ... top down and reads the words of the combination's columns from its own row itself -- rows are
//             16-byte aligned and lie one after the other, so the 64 rows of a step are one contiguous stretch of memory and every
//             cache line of it that holds a wanted word is fetched once a load instruction; the reduction across the columns is a
//             loop in one lane: no cross-lane step, no segments that are not powers of two, and the only ordered operation (the
//             ram sum across columns) is in program order.  The combinations go through in PASSES of at most kPer = 4 (three
//             with more than 1 022 bins): their running statistics live in registers.  Per combination in registers: ONE 64-bit
//             sum over the rows (the u64 sum of v, or the bits of the f64 sum of x with, next to it, the f64 sum of what its
//             additions rounded away -- TwoSum --, added back once before the division), min / max as 64-bit keys (v itself;
//             of a ram value the bits b mapped to (b >> 63) ? ~b : (b | 1 << 63)), the rows with x > threshold.  The 64 lanes meet by
//             shuffles down 32, 16, ... 1 -- a fixed tree -- and lane 0 writes one record per combination: into the outputs when
//             every group is a single scenario, else into scratch.
//   histogram every wave has an LDS histogram of its own, (n_bins + 2) words per combination of the pass -- the bins, under,
//             over; the bin of x by af_series_histogram.hpp's rule, bit for bit.  Same-bin contention: the lanes compare their
//             entry with that of lane 0 (one shuffle, one __ballot); lane 0 adds the popcount of the agreeing lanes at once, a
//             lane that disagrees adds 1.  A window of at most kTinyRows rows adds to the cell in HBM directly; a longer one
//             clears its words, counts in LDS and adds the non-zero words to the cell.  LDS adds are ds_add_u32, HBM adds
//             global_atomic_add on outputs the entry zeroed.  BUDGET: kWaveLdsWords = 4 096 words = 16 KiB a wave, 64 KiB a block.
//   reduce    a thread per (group, window, combination) folds its members' records in ascending scenario index, divides once,
//             and writes the cell; empty cells (after a direct pass only those of groups without members) get count 0, NaN.
// Every integer output is combined with integer +, min and max only; the f64 sum of a ram combination is added in a fixed
// order -- a lane's rows top down, the lanes' tree, the members ascending -- that depends on the window alone: nothing depends on
// the launch, the batch a scenario sits in, the other combinations of the call, or the run.  The rounding errors of those
// additions are carried along (a compensated sum): while every partial sum is exact they are zero and the mean is the plain
// sum's; otherwise the sum is good to about 2^-100 relative, so the mean is fsum(v) / count or its neighbour -- a plain sum's
// count - 1 roundings, with those of fsum and of the two divisions on top, miss (count - 1) * 2^-53 in cells of 3 to 8 rows.
// Scratch (engine-owned, shared with the other analyzers): 4 B per edge + 40 B per combination + 4 B per listed column + 4 B per
// group + 4 B per scenario (+ up to 256 B of alignment for each of the ten parts), and -- unless every group is a single
// scenario -- 36 B per (scenario, window, combination): 8 B sum, 8 B its compensation, 8 B each min, max (as keys), 4 B above.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "af_summary.hpp"

namespace afsc {

constexpr int kThreads = 256;               // the partial kernel: four waves, four work items
constexpr int kWaves = kThreads / 64;
constexpr int kReduceThreads = 256;
constexpr uint32_t kSkip = 0xFFFFFFFFu;     // AF_POOL_SKIP
constexpr uint32_t kMaxCombos = 64;         // AF_MAX_SERIES_COMBINATIONS
constexpr uint32_t kMaxBins = 1024;         // AF_MAX_SERIES_HISTOGRAM_BINS
constexpr uint32_t kPer = 4;                // combinations of a pass: their statistics are in registers
constexpr uint32_t kWaveLdsWords = 4096;    // the LDS histogram of one wave, in words
constexpr uint32_t kTinyRows = 64;          // windows of at most this many rows (one step) add to HBM directly
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kSum = 0, kMin = 1, kMax = 2, kSpread = 3;   // AF_COMBINE_*
static_assert(kMaxBins + 2u <= kWaveLdsWords, "one combination must fit the LDS of a wave");

// one combination, as the host lays it out
struct Combo {
    uint32_t op, c0, c1, is_f;   // its columns: cols[c0 .. c1 - 1]; is_f: ram_in_use columns
    double thr, lo, wd;
};
static_assert(sizeof(Combo) == 40, "the scratch bound counts 40 bytes a combination");

struct ScArgs {
    const uint32_t* samples;   // [n][tick_cap][pitch]
    const uint32_t* counts;    // [n][8]
    uint32_t tick_cap, pitch, cnt_ticks_slot;
    const uint32_t* group;     // [n] or null (all in group 0)
    uint32_t n_scen, n_groups, n_win;
    uint32_t run;              // windows per work item of the partial kernel
    uint32_t direct;           // every group is one scenario or none: the partial kernel writes the cells
    const uint32_t* edges;     // [W + 1]
    uint32_t n_combos, n_bins;
    uint32_t per;              // combinations of a pass: min(kPer, kWaveLdsWords / (n_bins + 2))
    const Combo* combos;       // [n_combos]
    const uint32_t* cols;      // the columns of combination 0, of combination 1, ... each ascending
    const uint32_t* mem_off;   // [G + 1] into members
    const uint32_t* members;   // the scenarios of group 0, of group 1, ... each ascending
    unsigned long long *rec_sum, *rec_min, *rec_max;   // [n][W][n_combos]
    double* rec_comp;
    uint32_t* rec_above;
    uint32_t* count;           // [G][W], or null
    double* mean;              // [G][W][n_combos]
    double *minv, *maxv;       // same shape, or null
    uint32_t* above;           // same shape, or null
    uint32_t* hist;            // [G][W][n_combos][n_bins], or null (n_bins == 0)
    uint32_t *under, *over;    // [G][W][n_combos], or null
};

__device__ __forceinline__ uint32_t stored_ticks(const ScArgs& a, uint32_t s) {
    const uint32_t m = a.counts[(size_t)s * 8u + a.cnt_ticks_slot];
    return m < a.tick_cap ? m : a.tick_cap;
}

// f64 bits (no NaN) -> unsigned keys that order like the values, -0.0 below +0.0, all of them > 0 and < 2^64 - 1; and back
__device__ __forceinline__ unsigned long long double_key(double x) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double double_unkey(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}

// the per-tick value of one combination in one row: v (integer columns) or x (ram columns); x = (double)v of an integer one
struct Tick {
    unsigned long long v;
    double x;
};
__device__ __forceinline__ Tick tick_value(const uint32_t* row, const uint32_t* cols, const Combo& cb, bool live) {
    unsigned long long isum = 0ull;
    uint32_t imn = 0xFFFFFFFFu, imx = 0u;
    double fsum = 0.0;
    unsigned long long kmn = ~0ull, kmx = 0ull;
    const bool is_f = cb.is_f != 0u;
    for (uint32_t k = cb.c0; k < cb.c1; k += 4u) {   // (uniform; four loads in flight)
        uint32_t w[4];
#pragma unroll
        for (uint32_t u = 0; u < 4u; ++u) w[u] = live && k + u < cb.c1 ? row[cols[k + u]] : 0u;
#pragma unroll
        for (uint32_t u = 0; u < 4u; ++u) {
            if (k + u >= cb.c1) break;               // (uniform)
            if (is_f) {
                const double d = (double)__uint_as_float(w[u]);
                fsum = k + u == cb.c0 ? d : fsum + d;
                const unsigned long long key = double_key(d);
                kmn = key < kmn ? key : kmn;
                kmx = key > kmx ? key : kmx;
            } else {
                isum += w[u];
                imn = w[u] < imn ? w[u] : imn;
                imx = w[u] > imx ? w[u] : imx;
            }
        }
    }
    Tick t;
    if (is_f) {
        t.v = 0ull;
        t.x = cb.op == kSum ? fsum : cb.op == kMin ? double_unkey(kmn) : cb.op == kMax ? double_unkey(kmx) : double_unkey(kmx) - double_unkey(kmn);
    } else {
        t.v = cb.op == kSum ? isum : cb.op == kMin ? imn : cb.op == kMax ? imx : (unsigned long long)(imx - imn);
        t.x = (double)t.v;
    }
    return t;
}

// what a lane keeps of one combination over its rows of a window: ONE 64-bit sum -- the u64 sum of v, or the bits of the f64
// sum of x (the form the record stores) --, min / max of the keys, the rows above the threshold
struct Acc {
    unsigned long long sum = 0ull;   // (+0.0 as a double)
    double comp = 0.0;               // a ram combination: what the additions into `sum` rounded away (the error terms of TwoSum)
    unsigned long long mn = ~0ull, mx = 0ull;
    uint32_t ab = 0u;
    // acc + v; of a ram combination as f64 with the rounding error of the addition added to `comp` (Knuth's TwoSum: exact
    // under round-to-nearest; the build has -ffp-contract=off -fno-fast-math)
    __device__ __forceinline__ static unsigned long long plus(unsigned long long acc, unsigned long long v, bool is_f, double& comp) {
        if (!is_f) return acc + v;
        const double a = __longlong_as_double((long long)acc), b = __longlong_as_double((long long)v);
        const double t = a + b, bb = t - a;
        comp = comp + ((a - (t - bb)) + (b - bb));
        return (unsigned long long)__double_as_longlong(t);
    }
    __device__ __forceinline__ void add(const Tick& t, bool is_f, double thr) {
        sum = plus(sum, is_f ? (unsigned long long)__double_as_longlong(t.x) : t.v, is_f, comp);
        const unsigned long long key = is_f ? double_key(t.x) : t.v;
        mn = key < mn ? key : mn;
        mx = key > mx ? key : mx;
        ab += t.x > thr ? 1u : 0u;
    }
    // the partner `dist` lanes up
    __device__ __forceinline__ void fold(int dist, bool take, bool is_f) {
        const unsigned long long osum = __shfl_down(sum, dist, 64), omn = __shfl_down(mn, dist, 64), omx = __shfl_down(mx, dist, 64);
        const uint32_t oab = __shfl_down(ab, dist, 64);
        const double ocomp = __shfl_down(comp, dist, 64);
        if (take) {
            sum = plus(sum, osum, is_f, comp);
            comp = comp + ocomp;
            mn = omn < mn ? omn : mn;
            mx = omx > mx ? omx : mx;
            ab += oab;
        }
    }
    __device__ __forceinline__ static double total(unsigned long long s, double comp, bool is_f) {
        return is_f ? __longlong_as_double((long long)s) + comp : (double)s;
    }
    // a key of a cell that holds a row -> the value that is written
    __device__ __forceinline__ static double value(unsigned long long key, bool is_f) { return is_f ? double_unkey(key) : (double)key; }
};

// the entry of a value among a combination's (n_bins + 2) words: its bin, n_bins for under, n_bins + 1 for over
// (af_series_histogram.hpp's rule)
__device__ __forceinline__ uint32_t entry_of(const Tick& t, bool plain, double lo, double width, uint32_t B) {
    if (plain) return t.v < (unsigned long long)B ? (uint32_t)t.v : B + 1u;
    if (t.x < lo) return B;
    const double q = (t.x - lo) / width;
    if (q >= (double)B) return B + 1u;
    const uint32_t b = (uint32_t)q;
    return b < B ? b : B + 1u;   // (q is in [0, B) here; a NaN, which no series holds, must not leave the combination's words)
}

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// n rows of combination c in entry e of cell `cell`, to HBM
__device__ __forceinline__ void add_cell(const ScArgs& a, size_t cell, uint32_t c, uint32_t e, uint32_t n) {
    const size_t o = cell * a.n_combos + c;
    if (e < a.n_bins) atomicAdd(&a.hist[o * a.n_bins + e], n);
    else if (e == a.n_bins) {
        if (a.under) atomicAdd(&a.under[o], n);
    } else if (a.over) atomicAdd(&a.over[o], n);
}

__global__ __launch_bounds__(kThreads) void af_scomb_partial(ScArgs a) {
    extern __shared__ uint32_t afsc_lds[];
    const int lane = threadIdx.x & 63;
    const uint32_t W = a.n_win, C = a.n_combos, B = a.n_bins, E = B + 2u;
    uint32_t* lh = afsc_lds + (threadIdx.x >> 6) * a.per * E;   // this wave's histogram (no word where B == 0)
    const uint32_t runs = (W + a.run - 1u) / a.run;             // work items per scenario
    const uint64_t item = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (item >= (uint64_t)a.n_scen * runs) return;              // (a whole wave; there is no block-wide barrier below)
    const uint32_t s = (uint32_t)(item / runs), w0 = (uint32_t)(item % runs) * a.run;
    const uint32_t w1 = W - w0 < a.run ? W : w0 + a.run;
    const uint32_t g = a.group ? a.group[s] : 0u;
    if (g == kSkip || g >= a.n_groups) return;
    const uint32_t m = stored_ticks(a, s);
    const uint32_t* rows = a.samples + (size_t)s * a.tick_cap * a.pitch;
    const bool want_hist = B != 0u;
    for (uint32_t q0 = 0; q0 < C; q0 += a.per) {                // a pass: the combinations q0 .. q0 + nq - 1
        const uint32_t nq = C - q0 < a.per ? C - q0 : a.per;
        Combo cb[kPer];
        bool plain[kPer];
#pragma unroll
        for (uint32_t i = 0; i < kPer; ++i) {
            cb[i] = a.combos[q0 + (i < nq ? i : 0u)];
            plain[i] = !cb[i].is_f && cb[i].lo == 0.0 && cb[i].wd == 1.0;
        }
        for (uint32_t w = w0; w < w1; ++w) {
            uint32_t r0 = a.edges[w], r1 = a.edges[w + 1u];
            r0 = r0 < m ? r0 : m;
            r1 = r1 < m ? r1 : m;
            const size_t cell = (size_t)g * W + w;
            const bool tiny = r1 - r0 <= kTinyRows;
            const bool in_lds = want_hist && !tiny && r1 > r0;
            if (in_lds) {
                for (uint32_t i = (uint32_t)lane; i < nq * E; i += 64u) lh[i] = 0u;
                wave_sync();
            }
            Acc acc[kPer];
            for (uint32_t r = r0; r < r1; r += 64u) {           // (uniform; r1 <= tick_cap < 2^31: no wrap)
                const uint32_t k = r + (uint32_t)lane;
                const bool live = k < r1;
                const uint32_t* row = rows + (size_t)k * a.pitch;   // (not read unless live)
#pragma unroll
                for (uint32_t i = 0; i < kPer; ++i) {
                    if (i >= nq) break;                          // (uniform)
                    const bool is_f = cb[i].is_f != 0u;
                    const Tick t = tick_value(row, a.cols, cb[i], live);
                    if (live) acc[i].add(t, is_f, cb[i].thr);
                    if (!want_hist) continue;                    // (uniform)
                    const uint32_t e = live ? entry_of(t, plain[i], cb[i].lo, cb[i].wd, B) : kNone;
                    const uint32_t e_first = (uint32_t)__shfl((int)e, 0, 64);   // (lane 0 holds the first row of the step: live)
                    const bool agree = live && e == e_first;
                    const unsigned long long same = __ballot(agree);
                    const uint32_t n = lane == 0 ? (uint32_t)__popcll(same) : (live && !agree ? 1u : 0u);
                    if (n) {
                        if (tiny) add_cell(a, cell, q0 + i, e, n);
                        else atomicAdd(&lh[i * E + e], n);
                    }
                }
            }
            if (in_lds) {
                wave_sync();
                for (uint32_t i = (uint32_t)lane; i < nq * E; i += 64u) {
                    const uint32_t n = lh[i];
                    if (n) add_cell(a, cell, q0 + i / E, i % E, n);
                }
                wave_sync();   // (the next window clears these words)
            }
            for (int h = 32; h >= 1; h >>= 1) {                 // (uniform: every lane of the wave shuffles)
#pragma unroll
                for (uint32_t i = 0; i < kPer; ++i) acc[i].fold(h, lane < h, cb[i].is_f != 0u);
            }
            if (lane != 0) continue;
            const uint32_t cnt = r1 - r0;
            if (a.direct && q0 == 0u && a.count) a.count[cell] = cnt;
#pragma unroll
            for (uint32_t i = 0; i < kPer; ++i) {
                if (i >= nq) break;
                const bool is_f = cb[i].is_f != 0u;
                if (a.direct) {
                    const size_t o = cell * C + q0 + i;
                    a.mean[o] = cnt ? Acc::total(acc[i].sum, acc[i].comp, is_f) / (double)cnt : __builtin_nan("");
                    if (a.minv) a.minv[o] = cnt ? Acc::value(acc[i].mn, is_f) : __builtin_nan("");
                    if (a.maxv) a.maxv[o] = cnt ? Acc::value(acc[i].mx, is_f) : __builtin_nan("");
                    if (a.above) a.above[o] = acc[i].ab;
                } else {
                    const size_t o = ((size_t)s * W + w) * C + q0 + i;
                    a.rec_sum[o] = acc[i].sum;
                    a.rec_comp[o] = acc[i].comp;
                    a.rec_min[o] = acc[i].mn;
                    a.rec_max[o] = acc[i].mx;
                    a.rec_above[o] = acc[i].ab;
                }
            }
        }
    }
}

// entries [first, first + n_entries) of the (group, window, combination) array
__global__ __launch_bounds__(kReduceThreads) void af_scomb_reduce(ScArgs a, uint64_t first, uint64_t n_entries) {
    const uint64_t idx = first + (uint64_t)blockIdx.x * kReduceThreads + threadIdx.x;
    if (idx >= n_entries) return;
    const uint32_t C = a.n_combos, W = a.n_win;
    const uint64_t cell = idx / C;
    const uint32_t c = (uint32_t)(idx % C);
    const uint32_t g = (uint32_t)(cell / W), w = (uint32_t)(cell % W);
    const uint32_t k0 = a.mem_off[g], k1 = a.mem_off[g + 1u];
    if (a.direct && k1 != k0) return;   // its one member's wave wrote the cell
    const bool is_f = a.combos[c].is_f != 0u;
    const uint32_t b0 = a.edges[w], b1 = a.edges[w + 1u];
    unsigned long long si = 0ull, mn = ~0ull, mx = 0ull;
    double comp = 0.0;
    uint32_t ab = 0u, cnt = 0u;
    for (uint32_t k = k0; k < k1; ++k) {
        const uint32_t s = a.members[k];
        const uint32_t m = stored_ticks(a, s);
        cnt += (b1 < m ? b1 : m) - (b0 < m ? b0 : m);
        const size_t o = ((size_t)s * W + w) * C + c;
        si = Acc::plus(si, a.rec_sum[o], is_f, comp);
        if (is_f) comp = comp + a.rec_comp[o];
        const unsigned long long rmn = a.rec_min[o], rmx = a.rec_max[o];
        mn = rmn < mn ? rmn : mn;
        mx = rmx > mx ? rmx : mx;
        ab += a.rec_above[o];
    }
    if (c == 0u && a.count) a.count[cell] = cnt;
    a.mean[idx] = cnt ? Acc::total(si, comp, is_f) / (double)cnt : __builtin_nan("");
    if (a.minv) a.minv[idx] = cnt ? Acc::value(mn, is_f) : __builtin_nan("");
    if (a.maxv) a.maxv[idx] = cnt ? Acc::value(mx, is_f) : __builtin_nan("");
    if (a.above) a.above[idx] = ab;
}

}  // namespace afsc
