// Windows by ARRIVAL time for the windowed and the quantile analyzer (af_engine_summarize_arrival_windows,
// af_engine_summarize_arrival_quantiles): with edges e[0] < ... < e[W], window w of scenario s holds its rows with
// e[w] < start <= e[w+1] -- the bucket rule of af_windowed.hpp applied to column 0: the cohort of the requests SENT in the
// window, which is what a user sees and what an objective is written against (by finish time an outage's slow requests are
// charged to the recovery).  start is NOT sorted in rqs_clock (rows are in completion order), so a window is a scattered
// subset of the scenario's rows, not a row range: instead of af_win_bounds / af_win_compact
//   counts    one workgroup per scenario: every stored row's window by binary search over the edges, a counter per edge,
//             then the block's prefix: c_s[k] = #{ i < m_s : start[s, i] <= e[k] } into the [n][W + 1] bounds array, whose
//             differences c_s[w+1] - c_s[w] are the windows' sizes -- the host lays the cells out from them as it does from
//             row bounds
//   compact   a STABLE partition: one wave per scenario takes its rows 64 at a time, in order; the lanes of one window are
//             found by the __ballot leader loop of afs::wave_agg_add, a lane's rank is the number of lanes below it in its
//             window, and the leader lane alone advances the window's cursor -- so row i of window w goes to
//             cell_off[g W + w] + pre[s][w] + #{ i' < i in w }: the rows of a cell's member stay in row (completion) order
// and the sample of cell (g, w) is again the concatenation, in ascending scenario index over the members of g, of
// finish - start over those rows.  Everything behind the compacted array is af_windowed.hpp's / af_quantiles.hpp's.
// Up to kLdsArrivalWindows windows the edges, counters and cursors lie in LDS (at most 64 KB, no attribute to set); above,
// the edges are read from global memory, the counters are the bounds array itself and the cursors are `pre`, advanced in
// place (nothing reads it afterwards): no scratch beyond af_windowed.hpp's.
// The cohorts are RIGHT-CENSORED: a request that arrived in a window but had not completed when the run ended, or was
// dropped, is in no row; a cell's total / count is the cohort's COMPLETIONS, not its arrivals, and the last windows of a run
// under-report slow requests.
// Integer atomics only, and a cursor is advanced by one wave in row order: results are run-to-run identical.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "af_windowed.hpp"

namespace afw {

constexpr uint32_t kLdsArrivalWindows = 4095;   // windows whose edges and cursors the arrival kernels keep in LDS (16 W + 8 B <= 64 KB)
constexpr int kArrivalCompactThreads = 64;      // the stable partition: one wave per scenario

// #{ k < ne : e[k] < x }: a start x lies in window b - 1 = (e[b-1], e[b]] where 1 <= b < ne (a NaN: ne, no window)
__device__ __forceinline__ uint32_t edges_below(const double* e, uint32_t ne, double x) {
    uint32_t lo = 0u, hi = ne;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (!(x <= e[mid])) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// The block's prefix over ne counters: out[k] = hist[0] + ... + hist[k].  A run of consecutive counters per thread, the runs' sums
// through the block; hist may BE out (the counters in global memory: every thread reads and writes its own run only).
template <bool kLds>
__device__ __forceinline__ void counters_prefix(uint32_t* hist, uint32_t* out, uint32_t ne, uint32_t* wave_total /* LDS [kWaves] */) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const auto counter = [&](uint32_t k) -> uint32_t {   // (global counters were written by atomics: read them where those went)
        return kLds ? hist[k] : __hip_atomic_load(&hist[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    const uint32_t per = (ne + (uint32_t)kThreads - 1u) / (uint32_t)kThreads;
    const uint32_t k0 = min((uint32_t)tid * per, ne), k1 = min(k0 + per, ne);
    uint32_t sum = 0u;
    for (uint32_t k = k0; k < k1; ++k) sum += counter(k);
    uint32_t incl = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(incl, d, 64);
        if (lane >= d) incl += t;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    uint32_t run = incl - sum;
    for (int v = 0; v < wave; ++v) run += wave_total[v];
    for (uint32_t k = k0; k < k1; ++k) {
        run += counter(k);
        out[k] = run;
    }
}

// The place of a row in the STABLE partition of a wave's 64 rows by key v (`in`: the lane has a row with a key): one turn per
// distinct key of the 64 rows (start is nearly sorted: one or two), lowest row first; a lane's rank is the number of lanes below
// it with its key, and the leader lane alone advances the key's cursor (the turns of a wave are in program order).  kLds: lcur[v]
// is the next place of key v; otherwise goff[v] + gcur[v].  Wave-wide: every lane of the wave calls it.
template <bool kLds>
__device__ __forceinline__ uint64_t partition_place(bool in, uint32_t w, uint64_t* lcur, uint32_t* gcur, const uint64_t* goff, int lane) {
    const unsigned long long below = (1ull << lane) - 1ull;
    uint64_t place = 0u;
    unsigned long long todo = __ballot(in);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)w, leader);
        const unsigned long long same = __ballot(in && w == v);
        uint64_t first = 0u;
        if (lane == leader) {   // one lane takes the key's rows off its cursor
            if (kLds) first = atomicAdd(reinterpret_cast<unsigned long long*>(&lcur[v]), (unsigned long long)__popcll(same));
            else first = goff[v] + atomicAdd(&gcur[v], (uint32_t)__popcll(same));
        }
        const uint32_t f_lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)first, leader);
        const uint32_t f_hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(first >> 32), leader);
        if (in && w == v) place = (((uint64_t)f_hi << 32) | f_lo) + (uint64_t)__popcll(same & below);
        todo &= ~same;
    }
    return place;
}

// c_s[k] = #{ i < m_s : start[s, i] <= e[k] } of scenario blockIdx.x (skipped ones too) into bounds[s][0 .. W]
template <bool kLds>
__global__ __launch_bounds__(kThreads) void af_arrival_counts(WinArgs a) {
    extern __shared__ __attribute__((aligned(8))) unsigned char dyn[];   // kLds: [W + 1] f64 edges, then [W + 1] u32 counters
    __shared__ uint32_t wave_total[kWaves];
    const uint32_t s = blockIdx.x;
    const int tid = threadIdx.x;
    const uint32_t ne = a.n_win + 1u;
    uint32_t m = a.counts[(size_t)s * 8u + a.cnt_completed_slot];
    if (m > a.clock_cap) m = a.clock_cap;
    const double2* ck = reinterpret_cast<const double2*>(a.clock) + (size_t)s * a.clock_cap;
    uint32_t* out = a.bounds + (size_t)s * ne;
    double* le = reinterpret_cast<double*>(dyn);
    uint32_t* hist = kLds ? reinterpret_cast<uint32_t*>(dyn + (size_t)ne * 8u) : out;
    for (uint32_t k = tid; k < ne; k += kThreads) {
        if (kLds) {
            le[k] = a.edges[k];
            hist[k] = 0u;
        } else {
            atomicExch(&hist[k], 0u);   // (in global memory the counters are touched by atomics only, until their thread writes c_s[k])
        }
    }
    __syncthreads();
    const double* e = kLds ? le : a.edges;
    for (uint32_t base = 0; base < m; base += kThreads) {   // (uniform trip count: wave_agg_add is wave-wide)
        const uint32_t i = base + (uint32_t)tid;
        const uint32_t b = i < m ? edges_below(e, ne, ck[i].x) : ne;
        afs::wave_agg_add(hist, b, b < ne);
    }
    __syncthreads();
    counters_prefix<kLds>(hist, out, ne, wave_total);
}

// the stable partition of scenario blockIdx.x's stored rows by the window of start: finish - start to the cells, by ONE wave
template <bool kLds>
__global__ __launch_bounds__(kArrivalCompactThreads) void af_arrival_compact(WinArgs a) {
    extern __shared__ __attribute__((aligned(8))) unsigned char dyn[];   // kLds: [W + 1] f64 edges, then [W] u64 cursors (next place of a window's row)
    const uint32_t s = blockIdx.x;
    const uint32_t g = a.group ? a.group[s] : 0u;
    if (g == kSkip) return;
    const int lane = threadIdx.x;
    const uint32_t W = a.n_win, ne = W + 1u;
    uint32_t m = a.counts[(size_t)s * 8u + a.cnt_completed_slot];
    if (m > a.clock_cap) m = a.clock_cap;
    const double2* ck = reinterpret_cast<const double2*>(a.clock) + (size_t)s * a.clock_cap;
    uint32_t* gcur = a.pre + (size_t)s * W;   // !kLds: the cursors, relative to the cell's first latency
    const uint64_t* goff = a.cell_off + (size_t)g * W;
    double* le = reinterpret_cast<double*>(dyn);
    uint64_t* lcur = reinterpret_cast<uint64_t*>(dyn + (size_t)ne * 8u);
    if (kLds) {
        for (uint32_t k = lane; k < ne; k += 64u) le[k] = a.edges[k];
        for (uint32_t w = lane; w < W; w += 64u) lcur[w] = goff[w] + gcur[w];
        __syncthreads();
    }
    const double* e = kLds ? le : a.edges;
    constexpr uint32_t kU = 4;
    for (uint32_t base = 0; base < m; base += kU * 64u) {   // (uniform trip count: the ballots below are wave-wide)
        double2 c[kU];
#pragma unroll
        for (uint32_t u = 0; u < kU; ++u) c[u] = base + u * 64u + (uint32_t)lane < m ? ck[base + u * 64u + (uint32_t)lane] : double2{};
#pragma unroll
        for (uint32_t u = 0; u < kU; ++u) {   // 64 rows at a time, in row order
            const uint32_t i = base + u * 64u + (uint32_t)lane;
            const uint32_t b = i < m ? edges_below(e, ne, c[u].x) : 0u;
            const bool in = b >= 1u && b <= W;   // lanes past m_s and rows outside (e[0], e[W]] take no part
            const uint32_t w = b - 1u;
            const uint64_t d = partition_place<kLds>(in, w, lcur, gcur, goff, lane);
            if (in) a.lat[d] = c[u].y - c[u].x;
        }
    }
}

}  // namespace afw
