// af_inflight.hpp -- requests IN FLIGHT end to end per tick, window of ticks and group, from the clock rows
// (af_engine_summarize_inflight, launched by engine.hip).  L of Little's law: af_engine_summarize_arrivals gives lambda, the
// by-arrival windows give W; no sampled series or combination of them holds a request that sits in a CPU step or between hops.
//
// DEFINITION.  Scenario s has m_s = min(counts[s][completed], clock_cap) stored rows (start_i, finish_i) and t_s =
// min(counts[s][ticks], tick_cap) sample rows; p = sample_period.
//   tick of a time   q(t) = floor(t / p): one f64 division rounded to nearest, then floor -- af_state.hpp's rule for `start`.
//                    a_i = q(start_i), f_i = q(finish_i).
//   rows counted     sample row k is taken at (k + 1) p (af_series_windows_t).  Request i is counted in the rows a_i <= k < f_i,
//                    clipped to [0, t_s): the samples taken strictly after its start and at or before its finish, as the
//                    quotient sees them (the row a request "met on arrival", q - 1 of af_state.hpp, does not contain it; the
//                    next one does).
//   counted nowhere  start or finish NaN; start < 0; f_i <= a_i (it lived between two samples, or finish < start); a_i >= t_s.
//                    The comparisons with t_s are made on the f64 quotients: a huge finish / p clips, it does not wrap.
//   per tick         started[s][k]   = #{ counted i : a_i == k }                          (a_i >= 0: start >= 0)
//                    finished[s][k]  = #{ counted i : f_i == k }    (f_i >= t_s: in none -- still in flight at the last sample)
//                    in_flight[s][k] = #{ counted i : a_i <= k < f_i } = sum over j <= k of started[s][j] - finished[s][j]
//   per cell (g, w)  the values in_flight[s][k] of the members s of g, min(b[w], t_s) <= k < min(b[w + 1], t_s) (the cells of
//                    af_series_windows.hpp): count, sum (u64), minv, maxv, above = #{ v > threshold }, hist[b] = #{ v == lo + b }
//                    with the last bin taking everything above it, under = #{ v < lo }.  An empty cell is all zeros.
// COMPLETED REQUESTS ONLY: a dropped request, and one still in flight when the run ended, is in no clock row.  The last seconds
// of a run under-count as the by-arrival cohorts do; `lost` of the arrivals call says by how much.
//
// KERNEL.  A workgroup owns a scenario and walks its ticks in CHUNKS of kChunkTicks.  Per chunk [c0, c1):
//   rows   every stored row once, 16-byte loads (one (start, finish) pair), kUnroll of them in flight per lane; two f64
//          divisions per row; +1 at a_i and -1 at f_i into the chunk's tick-indexed LDS array of DIFFERENCES (mod 2^32) where
//          they fall inside the chunk.  With the started / finished outputs a second array counts the finishes alone.
//   scan   tiles of kThreads ticks: the DPP wave scan of the engine, the waves' totals through LDS, and the CARRY: in_flight
//          at the chunk's last tick is what is open at the next chunk's first one -- a request that spans a seam adds its +1
//          in one chunk and its -1 in another, and is in the carry in between.  The per-tick outputs are written here.
//   fold   a wave per window that meets the chunk: sum, min, max, above by lane and then by shuffles, the histogram by
//          wave-aggregated adds, and ONE set of integer atomics per (scenario, window, chunk) on initialised outputs.
// LDS: kChunkTicks words = 48 KiB (96 KiB with started / finished): two workgroups (one) per compute unit of 160 KiB.
// Integer add / min / max atomics only: every word is identical from run to run and does not depend on the batch.
// af_inflight_finish turns the min of an empty cell (still the initial all-ones word) into 0.
//
// The per-row logic -- the quotient, the rejections, the clipping, where a row falls in a chunk -- and the sequential
// statement of a scenario (scenario_series) are AF_HD text without a HIP include: gfx950 device code and, under g++, what
// tests/hostcheck/inflight_main.cpp runs under the sanitizers.
#pragma once

#include <stdint.h>

#if !defined(AF_HD)
#if defined(__HIPCC__)
#define AF_HD __host__ __device__ __forceinline__
#else
#define AF_HD inline
#endif
#endif

namespace afif {

constexpr uint32_t kChunkTicks = 12288;       // ticks of one LDS chunk (config 2's 12 000 ticks: one pass over the rows)
constexpr uint32_t kThreads = 512;            // eight waves a workgroup
constexpr uint32_t kWaves = kThreads / 64u;
constexpr uint32_t kUnroll = 4;               // 16-byte loads a lane has in flight
constexpr uint32_t kSkip = 0xFFFFFFFFu;       // AF_POOL_SKIP
constexpr uint32_t kMaxBins = 1024;           // AF_MAX_SERIES_HISTOGRAM_BINS
constexpr uint32_t kNone = 0xFFFFFFFFu;
static_assert(kChunkTicks % kThreads == 0u, "a chunk is whole tiles");

// The ticks of a row: true when the request is counted, then it is in the rows a <= k < f, f <= t_s (f == t_s: it does not
// finish within the samples).  a < f and a < t_s then hold.
AF_HD bool row_ticks(double start, double finish, double period, uint32_t t_s, uint32_t& a, uint32_t& f) {
    if (!(start >= 0.0) || finish != finish) return false;   // NaN, negative (-0.0 is not negative)
    const double qa = __builtin_floor(start / period), qf = __builtin_floor(finish / period);
    if (!(qa < (double)t_s) || !(qf > qa)) return false;     // a_i >= t_s; f_i <= a_i (qa, qf: whole numbers or +-inf, no NaN here)
    a = (uint32_t)qa;                                         // 0 <= qa < t_s < 2^32
    f = qf >= (double)t_s ? t_s : (uint32_t)qf;               // (+inf clips)
    return true;
}

// Where a counted row (a, f) falls in the chunk [c0, c1): the chunk-relative ticks of its +1 and its -1, or kNone.
struct ChunkHit {
    uint32_t start, finish;
};
AF_HD ChunkHit chunk_hit(uint32_t a, uint32_t f, uint32_t c0, uint32_t c1) {
    ChunkHit h;
    h.start = a >= c0 && a < c1 ? a - c0 : kNone;
    h.finish = f >= c0 && f < c1 ? f - c0 : kNone;   // (f == t_s >= c1: never)
    return h;
}

// One scenario, sequentially, chunk by chunk as the kernel walks it: rows [m][2], outputs [t_s] each (any may be null).
// `diff` and `fin` are the chunk arrays, `chunk` words each.  Returns in_flight at the last tick (0 without ticks).
AF_HD uint32_t scenario_series(const double* rows, uint32_t m, double period, uint32_t t_s, uint32_t chunk, uint32_t* diff, uint32_t* fin,
                               uint32_t* started, uint32_t* finished, uint32_t* in_flight) {
    uint32_t carry = 0u;   // in flight at the previous chunk's last tick
    for (uint32_t c0 = 0u; c0 < t_s; c0 += chunk) {
        const uint32_t c1 = t_s - c0 < chunk ? t_s : c0 + chunk;
        for (uint32_t k = 0u; k < c1 - c0; ++k) diff[k] = fin[k] = 0u;
        for (uint32_t i = 0u; i < m; ++i) {
            uint32_t a, f;
            if (!row_ticks(rows[2u * i], rows[2u * i + 1u], period, t_s, a, f)) continue;
            const ChunkHit h = chunk_hit(a, f, c0, c1);
            if (h.start != kNone) diff[h.start] += 1u;
            if (h.finish != kNone) {
                diff[h.finish] -= 1u;
                fin[h.finish] += 1u;
            }
        }
        for (uint32_t k = 0u; k < c1 - c0; ++k) {
            if (started) started[c0 + k] = diff[k] + fin[k];
            if (finished) finished[c0 + k] = fin[k];
            carry += diff[k];
            if (in_flight) in_flight[c0 + k] = carry;
        }
        if (c1 == t_s) break;   // (c0 + chunk could wrap)
    }
    return carry;
}

// the bin of a value: 0 .. n_bins - 1 (the last one takes everything above it), or n_bins for a value below lo
AF_HD uint32_t bin_of(uint32_t v, uint32_t lo, uint32_t n_bins) {
    if (v < lo) return n_bins;
    const uint32_t b = v - lo;
    return b < n_bins ? b : n_bins - 1u;
}

struct IfArgs {
    const double* clock;       // [n][clock_cap][2]
    const uint32_t* counts;    // [n][8]
    uint32_t clock_cap, tick_cap, cnt_completed_slot, cnt_ticks_slot;
    double period;
    const uint32_t* group;     // [n], or null: all in group 0
    uint32_t n_win;
    const uint32_t* edges;     // DEVICE [n_win + 1]
    uint32_t threshold, n_bins, lo;
    uint32_t* count;           // [G][W]
    unsigned long long* sum;   // [G][W]
    uint32_t* minv;            // [G][W] or null, all-ones before the launch
    uint32_t* maxv;            // [G][W] or null
    uint32_t* above;           // [G][W] or null
    uint32_t* hist;            // [G][W][n_bins] or null
    uint32_t* under;           // [G][W] or null
    uint32_t* in_flight;       // [n][tick_cap] or null
    uint32_t* started;         // [n][tick_cap] or null
    uint32_t* finished;        // [n][tick_cap] or null
};

#if defined(__HIPCC__)
// #{ k <= n_win : edges[k] <= x } of the ascending edges
__device__ __forceinline__ uint32_t edges_at_or_below(const uint32_t* e, uint32_t n_edges, uint32_t x) {
    uint32_t lo = 0u, n = n_edges;
    while (n > 0u) {
        const uint32_t half = n >> 1;
        if (e[lo + half] <= x) {
            lo += half + 1u;
            n -= half + 1u;
        } else {
            n = half;
        }
    }
    return lo;
}

// The windows that meet the chunk [c0, c1), a wave each: ticks [r0, r1) of window w lie in d[r0 - c0 .. r1 - c0).
__device__ __forceinline__ void fold_chunk(const IfArgs& a, const uint32_t* d, uint32_t g, uint32_t c0, uint32_t c1) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t below = edges_at_or_below(a.edges, a.n_win + 1u, c0);   // (uniform)
    const uint32_t B = a.n_bins;
    for (uint32_t w = (below ? below - 1u : 0u) + wave; w < a.n_win; w += kWaves) {   // (uniform per wave)
        uint32_t r0 = a.edges[w], r1 = a.edges[w + 1u];
        if (r0 >= c1) break;
        r0 = r0 < c0 ? c0 : r0;
        r1 = r1 > c1 ? c1 : r1;
        if (r1 <= r0) continue;
        const size_t cell = (size_t)g * a.n_win + w;
        unsigned long long sum = 0ull;
        uint32_t mn = 0xFFFFFFFFu, mx = 0u, ab = 0u;
        for (uint32_t k0 = r0; k0 < r1; k0 += 64u) {        // (uniform; r1 <= tick_cap < 2^31: no wrap)
            const uint32_t k = k0 + lane;
            const bool on = k < r1;
            const uint32_t v = on ? d[k - c0] : 0u;
            if (on) {
                sum += v;
                mn = v < mn ? v : mn;
                mx = v > mx ? v : mx;
                ab += v > a.threshold ? 1u : 0u;
            }
            if (a.hist) {                                   // (uniform) one add per distinct bin of the wave, up to four, then one per lane
                const uint32_t e = on ? bin_of(v, a.lo, B) : kNone;
                const bool act = on && (e < B || a.under != nullptr);
                uint32_t* word = !act ? nullptr : e < B ? a.hist + cell * B + e : a.under + cell;
                unsigned long long todo = __ballot(act);
                for (int it = 0; it < 4 && todo; ++it) {
                    const int leader = __ffsll((long long)todo) - 1;
                    const uint32_t ev = (uint32_t)__builtin_amdgcn_readlane((int)e, leader);
                    const unsigned long long same = __ballot(act && e == ev) & todo;
                    if ((int)lane == leader) atomicAdd(word, (uint32_t)__popcll(same));
                    todo &= ~same;
                }
                if ((todo >> lane) & 1ull) atomicAdd(word, 1u);
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            sum += __shfl_down(sum, off, 64);
            const uint32_t omn = (uint32_t)__shfl_down((int)mn, off, 64), omx = (uint32_t)__shfl_down((int)mx, off, 64);
            mn = omn < mn ? omn : mn;
            mx = omx > mx ? omx : mx;
            ab += (uint32_t)__shfl_down((int)ab, off, 64);
        }
        if (lane == 0u) {
            atomicAdd(&a.count[cell], r1 - r0);
            if (sum) atomicAdd(&a.sum[cell], sum);
            if (a.minv) atomicMin(&a.minv[cell], mn);
            if (a.maxv && mx) atomicMax(&a.maxv[cell], mx);
            if (a.above && ab) atomicAdd(&a.above[cell], ab);
        }
    }
}

// W: the engine's wave primitives (scan_incl_u32, the DPP scan).  kBoth: the started / finished outputs are wanted.
template <class W, bool kBoth>
__global__ void __launch_bounds__(kThreads) af_inflight_kernel(const IfArgs a) {
    extern __shared__ uint32_t afif_lds[];   // [kChunkTicks] differences, then in_flight; kBoth: [kChunkTicks] finishes behind
    __shared__ uint32_t wave_total[kWaves];
    uint32_t* d = afif_lds;
    uint32_t* fn = afif_lds + kChunkTicks;
    const uint32_t s = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t g = a.group ? a.group[s] : 0u;
    if (g == kSkip && !a.in_flight && !a.started && !a.finished) return;   // (the whole workgroup)
    uint32_t m = a.counts[(size_t)s * 8u + a.cnt_completed_slot];
    m = m < a.clock_cap ? m : a.clock_cap;
    uint32_t t_s = a.counts[(size_t)s * 8u + a.cnt_ticks_slot];
    t_s = t_s < a.tick_cap ? t_s : a.tick_cap;
    const double2* ck = reinterpret_cast<const double2*>(a.clock) + (size_t)s * a.clock_cap;
    const size_t row = (size_t)s * a.tick_cap;
    uint32_t carry = 0u;   // in flight at the previous chunk's last tick
    for (uint32_t c0 = 0u; c0 < t_s; c0 += kChunkTicks) {   // (uniform; t_s <= tick_cap < 2^31: no wrap)
        const uint32_t c1 = t_s - c0 < kChunkTicks ? t_s : c0 + kChunkTicks, len = c1 - c0;
        for (uint32_t k = tid; k < len; k += kThreads) {
            d[k] = 0u;
            if (kBoth) fn[k] = 0u;
        }
        __syncthreads();
        for (uint32_t base = 0u; base < m; base += kThreads * kUnroll) {   // (m <= clock_cap; the engine keeps n * clock_cap rows addressable)
            double2 c[kUnroll];
#pragma unroll
            for (uint32_t u = 0; u < kUnroll; ++u) {
                const uint32_t i = base + u * kThreads + tid;
                c[u] = i < m && i >= base ? ck[i] : double2{-1.0, -1.0};   // (a row that counts nowhere; i >= base: no wrap)
            }
#pragma unroll
            for (uint32_t u = 0; u < kUnroll; ++u) {
                uint32_t ra, rf;
                if (!row_ticks(c[u].x, c[u].y, a.period, t_s, ra, rf)) continue;
                const ChunkHit h = chunk_hit(ra, rf, c0, c1);
                if (h.start != kNone) atomicAdd(&d[h.start], 1u);
                if (h.finish != kNone) {
                    atomicSub(&d[h.finish], 1u);
                    if (kBoth) atomicAdd(&fn[h.finish], 1u);
                }
            }
            if (m - base <= kThreads * kUnroll) break;   // (base + kThreads * kUnroll could wrap)
        }
        __syncthreads();
        for (uint32_t t0 = 0u; t0 < len; t0 += kThreads) {   // (uniform: the scan and the barriers are block-wide)
            const uint32_t k = t0 + tid;
            const uint32_t dv = k < len ? d[k] : 0u;
            uint32_t v = W::scan_incl_u32(dv);
            if (lane == 63u) wave_total[wave] = v;
            __syncthreads();
            uint32_t before = 0u, total = 0u;
#pragma unroll
            for (uint32_t w = 0; w < kWaves; ++w) {
                const uint32_t t = wave_total[w];
                before += w < wave ? t : 0u;
                total += t;
            }
            v += carry + before;
            carry += total;
            if (k < len) {
                d[k] = v;
                if (a.in_flight) a.in_flight[row + c0 + k] = v;
                if (kBoth) {
                    const uint32_t f = fn[k];
                    if (a.started) a.started[row + c0 + k] = dv + f;
                    if (a.finished) a.finished[row + c0 + k] = f;
                }
            }
            __syncthreads();   // (wave_total is written again; d is read by other waves below)
        }
        if (g != kSkip) fold_chunk(a, d, g, c0, c1);
        if (c1 == t_s) break;
        __syncthreads();       // (the next chunk clears d)
    }
}

// the min of a cell without values is 0, like its other outputs
__global__ void __launch_bounds__(256) af_inflight_finish(const uint32_t* count, uint32_t* minv, uint32_t cells) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c < cells && count[c] == 0u) minv[c] = 0u;
}
#endif  // __HIPCC__

}  // namespace afif
