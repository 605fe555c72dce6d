// af_arrival_counts.hpp -- arrivals per window and group from the pre-generated arrival times (af_engine_summarize_arrivals,
// launched by engine.hip).
//
// A row is one scenario's arrival times as af_pregen.hpp writes them: ascending, +inf behind the last one, n_draw doubles.
// With edges e[0] < ... < e[W] the analyzer wants b[k] = #{ i < m : row[i] <= e[k] } (np.searchsorted(row[:m], e, "right"),
// m = the number of finite times), and per group the sums of b[w + 1] - b[w] over its members.  Three steps:
//
//   1. the row's length m, and the part of the row the windows can tell apart: [lo, hi) = [b[0], b[W]) -- three binary searches;
//   2. the bounds, one of two ways, chosen per row by the bytes each moves (use_stream below);
//        search : lane k looks e[k] up in the row.  A probe is a cache line of 64 bytes, a search ceil(log2(span + 1)) probes:
//                 64 (W + 1) ceil(log2(span + 1)) bytes -- ~17 lines per edge on a row of 80 000 arrivals;
//        stream : the wave reads row[lo .. hi) once, 64 ascending values a step: 8 span bytes.  Each value's RANK among the
//                 edges, c = #{ k : e[k] < v }, is searched in LDS from the previous step's last rank on (edge_rank_from); ranks
//                 never decrease along the row, so where the rank
//                 steps from p to c at index i the bounds b[p .. c) are all i.  Every bound is stored exactly once, by the lane
//                 that sees its step (index hi counts as a value above every edge): no atomics, no second pass;
//      few windows over a long row search, many windows (600 over 80 000 arrivals: 0.64 MB streamed against 0.65 MB probed,
//      and the stream is contiguous) stream;
//   3. the group sums (af_arrival_group_sums): a thread per window walks kSumRows consecutive scenarios, adds up while the group
//      id stays the same and hands each run to the output with ONE 64-bit integer atomic add.  Integer + on zeroed outputs:
//      the result does not depend on the order, hence not on the launch or on the chunk a scenario sits in.
//
// The edges live in LDS while they fit (kMaxLdsEdges doubles per workgroup of four waves = four scenarios); above that the
// same code reads them where the engine keeps them in HBM.
//
// No index depends on the DATA being sorted: every row access is below n_draw, every bound written has k <= W.  Rows that
// are not ascending give meaningless bounds, nothing else.
//
// The per-row logic is AF_HD text without a HIP include: gfx950 device code and, under g++, what
// tests/hostcheck/arrival_counts_main.cpp runs under the sanitizers.
#pragma once

#include <stdint.h>

#if !defined(AF_HD)
#if defined(__HIPCC__)
#define AF_HD __host__ __device__ __forceinline__
#else
#define AF_HD inline
#endif
#endif

namespace afac {

constexpr uint32_t kSkip = 0xFFFFFFFFu;       // AF_POOL_SKIP
constexpr uint32_t kMaxLdsEdges = 4096u;      // window edges (W + 1) a workgroup keeps in LDS: 8 (W + 1) bytes, 32 KB at most
constexpr uint32_t kWavesPerBlock = 4u;       // scenarios per workgroup of af_arrival_bounds
constexpr uint32_t kSumRows = 64u;            // scenarios a thread of af_arrival_group_sums walks
constexpr double kMaxFinite = 1.7976931348623157e308;

// #{ i < m : row[i] <= x } of an ascending row: np.searchsorted(row[:m], x, side="right")
AF_HD uint32_t count_le(const double* row, uint32_t m, double x) {
    uint32_t lo = 0u, n = m;
    while (n > 0u) {
        const uint32_t half = n >> 1;
        if (row[lo + half] <= x) {
            lo += half + 1u;
            n -= half + 1u;
        } else {
            n = half;
        }
    }
    return lo;
}
// the finite times of a row (+inf behind the last arrival)
AF_HD uint32_t row_length(const double* row, uint32_t n_draw) { return count_le(row, n_draw, kMaxFinite); }

// the rank of a value among the edges: #{ k < n_edges : e[k] < v }
template <class EdgePtr>
AF_HD uint32_t edge_rank(EdgePtr e, uint32_t n_edges, double v) {
    uint32_t lo = 0u, n = n_edges;
    while (n > 0u) {
        const uint32_t half = n >> 1;
        if (e[lo + half] < v) {
            lo += half + 1u;
            n -= half + 1u;
        } else {
            n = half;
        }
    }
    return lo;
}

// the same rank for a value known to have at least `from` edges below it -- the rank of an earlier value of an ascending row:
// gallop from there (1, 2, 4 ... edges ahead), then search the bracket.  Ranks advance slowly along a row (600 windows over
// 80 000 arrivals: one window per 133 values), so this is one to three probes where the plain search takes ten.  A row that is
// not ascending gets a rank that means nothing; every probe stays below n_edges.
template <class EdgePtr>
AF_HD uint32_t edge_rank_from(EdgePtr e, uint32_t n_edges, double v, uint32_t from) {
    uint32_t base = from < n_edges ? from : n_edges, step = 1u;
    while (n_edges - base >= step && e[base + step - 1u] < v) {
        base += step;
        step <<= 1;
    }
    const uint32_t room = n_edges - base;
    return base + edge_rank(e + base, room < step - 1u ? room : step - 1u, v);
}

AF_HD uint32_t log2_ceil(uint32_t v) {   // ceil(log2(v)), 0 for v <= 1
    uint32_t b = 0u;
    while (b < 32u && (1ull << b) < (uint64_t)v) ++b;
    return b;
}
// THE RULE: stream the row's span when that moves fewer bytes than the searches' probes do
AF_HD bool use_stream(uint32_t span, uint32_t n_windows) {
    return 8ull * span < 64ull * ((uint64_t)n_windows + 1u) * log2_ceil(span + 1u);
}

// the rank steps from p to c at row index i: the bounds p .. c - 1 are i
AF_HD void emit_bounds(uint32_t* b, uint32_t p, uint32_t c, uint32_t i) {
    for (uint32_t k = p; k < c; ++k) b[k] = i;
}

// One row, sequentially: what a wave of af_arrival_bounds computes (host builds, and the statement of the kernel's steps).
// b[0 .. n_windows]; returns the row's length.  `force`: 0 the rule's choice, 1 search, 2 stream.
template <class EdgePtr>
AF_HD uint32_t row_bounds(const double* row, uint32_t n_draw, EdgePtr e, uint32_t n_windows, uint32_t* b, int force = 0) {
    const uint32_t n_edges = n_windows + 1u;
    const uint32_t m = row_length(row, n_draw);
    const uint32_t lo = count_le(row, m, e[0]), hi = count_le(row, m, e[n_windows]);
    const bool stream = force ? force == 2 : use_stream(hi - lo, n_windows);
    if (!stream) {
        for (uint32_t k = 0u; k < n_edges; ++k) b[k] = count_le(row, m, e[k]);
        return m;
    }
    uint32_t p = 0u;   // the rank of everything before lo: at or below e[0]
    for (uint32_t i = lo; i <= hi; ++i) {
        const uint32_t c = i < hi ? edge_rank_from(e, n_edges, row[i], p) : n_edges;
        emit_bounds(b, p, c, i);
        p = c;
    }
    return m;
}

struct CountArgs {
    const double* times;     // [n_scen][n_draw]
    uint32_t n_scen, n_draw, n_win, n_groups;
    const double* edges;     // DEVICE [n_win + 1]
    const uint32_t* group;   // DEVICE [n_scen] or null: scenario s is group first_group + s
    uint32_t first_group;
    uint32_t* bounds;        // [n_scen][n_win + 1]
    uint32_t* generated;     // [n_scen] or null
    unsigned long long* arrivals;   // [n_groups][n_win], zeroed before the first chunk
};

#if defined(__HIPCC__)
// A wave per scenario.  Everything that decides a branch or a trip count (m, lo, hi, the rule) is the same in all lanes of
// a wave: the searches for them run in every lane on the same addresses.
template <bool kLdsEdges>
__global__ void __launch_bounds__(64u * kWavesPerBlock) af_arrival_bounds(const CountArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char arrival_counts_smem[];
    const uint32_t n_edges = a.n_win + 1u;
    const double* E = a.edges;
    if (kLdsEdges) {
        double* le = reinterpret_cast<double*>(arrival_counts_smem);
        for (uint32_t k = threadIdx.x; k < n_edges; k += blockDim.x) le[k] = a.edges[k];
        __syncthreads();
        E = le;
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t s = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (s >= a.n_scen) return;
    const double* row = a.times + (size_t)s * a.n_draw;
    uint32_t* b = a.bounds + (size_t)s * n_edges;
    const uint32_t m = row_length(row, a.n_draw);
    if (lane == 0u && a.generated) a.generated[s] = m;
    const uint32_t lo = count_le(row, m, E[0]), hi = count_le(row, m, E[a.n_win]);
    if (!use_stream(hi - lo, a.n_win)) {
        for (uint32_t k = lane; k < n_edges; k += 64u) b[k] = count_le(row, m, E[k]);
        return;
    }
    uint32_t last = 0u;   // the rank of the value before this step's first
    for (uint32_t base = lo; base <= hi; base += 64u) {
        const uint32_t i = base + lane;
        const uint32_t c = i < hi ? edge_rank_from(E, n_edges, row[i], last) : n_edges;
        uint32_t p = (uint32_t)__shfl_up((int)c, 1, 64);
        if (lane == 0u) p = last;
        if (i <= hi) emit_bounds(b, p, c, i);
        last = (uint32_t)__shfl((int)c, 63, 64);
        if (hi - base < 64u) break;   // (index hi was in this step; base + 64 could wrap)
    }
}

// arrivals[g][w] += b[s][w + 1] - b[s][w] over the members s of g
__global__ void __launch_bounds__(256) af_arrival_group_sums(const CountArgs a) {
    const uint32_t w = blockIdx.y * 256u + threadIdx.x;   // (grid: x over the scenarios, y over the windows' tiles)
    if (w >= a.n_win) return;
    const uint32_t s0 = blockIdx.x * kSumRows;
    const uint32_t s1 = a.n_scen - s0 < kSumRows ? a.n_scen : s0 + kSumRows;
    const uint32_t n_edges = a.n_win + 1u;
    uint32_t cur = kSkip;
    unsigned long long acc = 0ull;
    for (uint32_t s = s0; s < s1; ++s) {
        const uint32_t g = a.group ? a.group[s] : a.first_group + s;
        if (g != cur) {
            if (cur != kSkip && acc) atomicAdd(&a.arrivals[(size_t)cur * a.n_win + w], acc);
            cur = g;
            acc = 0ull;
        }
        if (g != kSkip) {
            const uint32_t* b = a.bounds + (size_t)s * n_edges + w;
            acc += (unsigned long long)(b[1] - b[0]);
        }
    }
    if (cur != kSkip && acc) atomicAdd(&a.arrivals[(size_t)cur * a.n_win + w], acc);
}
#endif  // __HIPCC__

}  // namespace afac
