// Latency by the STATE a request met on arrival (af_engine_summarize_state_windows, af_engine_summarize_state_quantiles): how
// slow were the requests that arrived while the ready queue, the IO sleep set, the RAM or an edge was at level b?  The cell of
// a stored row of scenario s with start = clock[s][i][0] is (arrival window w, bin b of ONE sampled series at the row's tick):
//   tick     q = floor(start / period) (one f64 division, rounded to nearest, then floor), k = q - 1: sample row k is taken at
//            (k + 1) * period (collector.py:53), so k is the last sample taken at or before the arrival AS THE F64 QUOTIENT
//            SEES IT.  No state, no cell: q < 1 (no sample yet), k >= t_s = min(counts[s][ticks], tick_cap), start NaN or
//            negative.
//   value    x = word samples[s][k][column] as f64, as af_series_histogram.hpp takes it: (double)word of an integer series,
//            (double)(float) of a ram_in_use column (a NaN, which no series holds: no cell).
//   bin      x < lo: no cell (-0.0 is not below 0.0);  t = (x - lo) / width, one f64 subtraction and one f64 division;
//            t >= n_bins: bin n_bins - 1 (the last bin takes the overflow: "queue >= k");  otherwise bin (uint32_t)t.
//   window   with n_time > 0 windows af_arrival.hpp's rule, e[w] < start <= e[w + 1], else no cell; with none, window 0.
// Key = w * n_bins + b < K = max(n_time, 1) * n_bins, the "windows" of WinArgs: cell (g, w, b) is cell g K + key of the
// windowed layout, and everything behind the compacted array is af_windowed.hpp's / af_quantiles.hpp's.  The two kernels are
// af_arrival.hpp's with this key:
//   counts    one workgroup per scenario: a counter per key, then the block's prefix into the [n][K + 1] bounds array:
//             c_s[0] = 0, c_s[k + 1] = #{ stored rows of s with key <= k }, the CUMULATIVE CELL COUNTS
//   compact   the stable partition by one wave per scenario (afw::partition_place): a cell's rows stay in row order
// The key is RECOMPUTED in the partition, as the arrival kernels recompute the window: a stored key would cost 4 B of scratch
// per stored row (3 GB beside a 12 GB rqs_clock) and a write and a read of it, the second gather one word per row from sample
// rows the first pass has just touched -- start is nearly sorted, so the 64 rows of a wave read the same or neighbouring
// sample rows.  Only word `column` of a row is read, never the padding, never a row at or past t_s.
// Up to kLdsStateCells keys the edges, counters and cursors lie in LDS (at most 64 KB, no attribute to set); above, the edges
// are read from global memory, the counters are the bounds array itself and the cursors are `pre`, advanced in place: no
// scratch beyond af_windowed.hpp's.
// The cohorts are RIGHT-CENSORED like the arrival windows: a request that had not completed when the run ended, or was
// dropped, is in no row.
// Integer atomics only, and a cursor is advanced by one wave in row order: results are run-to-run identical and do not depend
// on the batch a scenario sits in.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "af_arrival.hpp"

namespace afst {

using afw::kThreads, afw::kWaves, afw::kSkip;
constexpr uint32_t kLdsStateCells = 4095;   // keys whose edges and cursors the state kernels keep in LDS (n_time <= K: 16 K + 8 B <= 64 KB)
constexpr int kStateCompactThreads = 64;    // the stable partition: one wave per scenario
constexpr uint32_t kNoCell = 0xFFFFFFFFu;

struct StateArgs {
    afw::WinArgs w;            // n_win = K keys per group; edges [n_time + 1] (n_time > 0); bounds [n][K + 1]
    const uint32_t* samples;   // [n][tick_cap][pitch]
    uint32_t tick_cap, pitch, cnt_ticks_slot;
    uint32_t column;           // the series, < pitch
    uint32_t is_float;         // a ram_in_use column
    uint32_t n_time;           // windows by arrival time; 0: one, with no condition on time
    uint32_t n_bins;
    double lo, width, period;
};

// the key of a row that starts at `start` (rows: the scenario's sample rows, t_s of them stored), or kNoCell
__device__ __forceinline__ uint32_t key_of_row(const StateArgs& a, const double* e, const uint32_t* rows, uint32_t t_s, double start) {
    if (!(start >= 0.0)) return kNoCell;                 // NaN, negative
    const double q = __builtin_floor(start / a.period);
    if (!(q >= 1.0) || q - 1.0 >= (double)t_s) return kNoCell;   // (q is a whole number: q - 1 is exact below 2^53, and at or past t_s above)
    const uint32_t k = (uint32_t)(q - 1.0);
    const uint32_t word = rows[(size_t)k * a.pitch + a.column];
    const double x = a.is_float ? (double)__uint_as_float(word) : (double)word;
    if (!(x >= a.lo)) return kNoCell;                    // below lo (or a NaN)
    const double t = (x - a.lo) / a.width;
    const uint32_t b = t >= (double)a.n_bins ? a.n_bins - 1u : (uint32_t)t;
    uint32_t w = 0u;
    if (a.n_time) {
        const uint32_t eb = afw::edges_below(e, a.n_time + 1u, start);
        if (eb < 1u || eb > a.n_time) return kNoCell;    // outside (e[0], e[n_time]]
        w = eb - 1u;
    }
    return w * a.n_bins + b;
}

// c_s[0] = 0, c_s[k + 1] = #{ i < m_s : key[s, i] <= k } of scenario blockIdx.x (skipped ones too) into bounds[s][0 .. K]
template <bool kLds>
__global__ __launch_bounds__(kThreads) void af_state_counts(StateArgs a) {
    extern __shared__ __attribute__((aligned(8))) unsigned char dyn[];   // kLds: [n_time + 1] f64 edges (n_time > 0), then [K + 1] u32 counters
    __shared__ uint32_t wave_total[kWaves];
    const uint32_t s = blockIdx.x;
    const int tid = threadIdx.x;
    const uint32_t ne = a.w.n_win + 1u, n_edge = a.n_time ? a.n_time + 1u : 0u;
    uint32_t m = a.w.counts[(size_t)s * 8u + a.w.cnt_completed_slot];
    if (m > a.w.clock_cap) m = a.w.clock_cap;
    uint32_t t_s = a.w.counts[(size_t)s * 8u + a.cnt_ticks_slot];
    if (t_s > a.tick_cap) t_s = a.tick_cap;
    const double2* ck = reinterpret_cast<const double2*>(a.w.clock) + (size_t)s * a.w.clock_cap;
    const uint32_t* rows = a.samples + (size_t)s * a.tick_cap * a.pitch;
    uint32_t* out = a.w.bounds + (size_t)s * ne;
    double* le = reinterpret_cast<double*>(dyn);
    uint32_t* hist = kLds ? reinterpret_cast<uint32_t*>(dyn + (size_t)n_edge * 8u) : out;
    if (kLds)
        for (uint32_t k = tid; k < n_edge; k += kThreads) le[k] = a.w.edges[k];
    for (uint32_t k = tid; k < ne; k += kThreads) {
        if (kLds) hist[k] = 0u;
        else atomicExch(&hist[k], 0u);   // (in global memory the counters are touched by atomics only, until their thread writes c_s[k])
    }
    __syncthreads();
    const double* e = kLds ? le : a.w.edges;
    for (uint32_t base = 0; base < m; base += kThreads) {   // (uniform trip count: wave_agg_add is wave-wide)
        const uint32_t i = base + (uint32_t)tid;
        const uint32_t key = i < m ? key_of_row(a, e, rows, t_s, ck[i].x) : kNoCell;
        afs::wave_agg_add(hist, key + 1u, key != kNoCell);   // (counter 0 stays 0: c_s[0])
    }
    __syncthreads();
    afw::counters_prefix<kLds>(hist, out, ne, wave_total);
}

// the stable partition of scenario blockIdx.x's stored rows by their key: finish - start to the cells, by ONE wave
template <bool kLds>
__global__ __launch_bounds__(kStateCompactThreads) void af_state_compact(StateArgs a) {
    extern __shared__ __attribute__((aligned(8))) unsigned char dyn[];   // kLds: [n_time + 1] f64 edges (n_time > 0), then [K] u64 cursors
    const uint32_t s = blockIdx.x;
    const uint32_t g = a.w.group ? a.w.group[s] : 0u;
    if (g == kSkip) return;
    const int lane = threadIdx.x;
    const uint32_t K = a.w.n_win, n_edge = a.n_time ? a.n_time + 1u : 0u;
    uint32_t m = a.w.counts[(size_t)s * 8u + a.w.cnt_completed_slot];
    if (m > a.w.clock_cap) m = a.w.clock_cap;
    uint32_t t_s = a.w.counts[(size_t)s * 8u + a.cnt_ticks_slot];
    if (t_s > a.tick_cap) t_s = a.tick_cap;
    const double2* ck = reinterpret_cast<const double2*>(a.w.clock) + (size_t)s * a.w.clock_cap;
    const uint32_t* rows = a.samples + (size_t)s * a.tick_cap * a.pitch;
    uint32_t* gcur = a.w.pre + (size_t)s * K;   // !kLds: the cursors, relative to the cell's first latency
    const uint64_t* goff = a.w.cell_off + (size_t)g * K;
    double* le = reinterpret_cast<double*>(dyn);
    uint64_t* lcur = reinterpret_cast<uint64_t*>(dyn + (size_t)n_edge * 8u);
    if (kLds) {
        for (uint32_t k = lane; k < n_edge; k += 64u) le[k] = a.w.edges[k];
        for (uint32_t c = lane; c < K; c += 64u) lcur[c] = goff[c] + gcur[c];
        __syncthreads();
    }
    const double* e = kLds ? le : a.w.edges;
    constexpr uint32_t kU = 4;
    for (uint32_t base = 0; base < m; base += kU * 64u) {   // (uniform trip count: the ballots below are wave-wide)
        double2 c[kU];
        uint32_t key[kU];
#pragma unroll
        for (uint32_t u = 0; u < kU; ++u) c[u] = base + u * 64u + (uint32_t)lane < m ? ck[base + u * 64u + (uint32_t)lane] : double2{};
#pragma unroll
        for (uint32_t u = 0; u < kU; ++u)   // (the four gathers in flight before the first turn)
            key[u] = base + u * 64u + (uint32_t)lane < m ? key_of_row(a, e, rows, t_s, c[u].x) : kNoCell;
#pragma unroll
        for (uint32_t u = 0; u < kU; ++u) {   // 64 rows at a time, in row order
            const bool in = key[u] != kNoCell;
            const uint64_t d = afw::partition_place<kLds>(in, key[u], lcur, gcur, goff, lane);
            if (in) a.w.lat[d] = c[u].y - c[u].x;
        }
    }
}

}  // namespace afst
