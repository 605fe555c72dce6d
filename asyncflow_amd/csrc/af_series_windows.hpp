// Sampled-series analyzer per (group, window of ticks): count, mean, min, max and the number of values above a threshold of
// every sampled series (af_engine_summarize_series_windows).
// Windows are on TICK INDICES: with edges b[0] < ... < b[W] and m_s = min(counts[s][ticks], tick_cap), window w of scenario s
// is its sample rows [min(b[w], m_s), min(b[w + 1], m_s)); rows at or past m_s and the padding words of a row are never used.
// The sample of (group g, window w, series j) is column j of those rows of every member of g.
//   partial   a WAVE per (scenario, run of consecutive windows), one window at a time.  samples[s] is [tick][pitch] words,
//             pq = pitch / 4 16-byte groups per row: lane l reads group l % L of row r0 + l / L, L = min(pq, 64), and then
//             every 64 / L-th row below it -- consecutive lanes read consecutive 16 bytes, a lane stays on its four columns
//             (plans of more than 256 padded series: 64 column groups at a time, the rows walked once per 64 groups).  EVERY
//             STORED ROW INSIDE THE WINDOWS IS READ ONCE.  Per column in registers: the u64 sum of the words or the f64 sum of the
//             float values (ram_in_use), min / max as keys -- the word itself, or afs::float_key of a ram_in_use word, which
//             orders like the float values with -0.0 below +0.0 --, the values above the threshold.  The lanes of a column group
//             meet by shuffles down L, 2 L, 4 L, ... lanes -- a fixed tree, the largest distance first -- and the first L lanes
//             write one record per series: into the outputs when every group is a single scenario, else into scratch.
//   reduce    a thread per (group, window, series) folds its members' records in ascending scenario index, divides once, and
//             writes the cell; empty cells (and, after a direct pass, only those of groups without members) get count 0, NaN.
// No atomics at all.  The integer sums are exact (a cell holds < 2^32 words below 2^32); the f64 sum of a float column is
// added in a fixed order -- a lane's rows top down, the lanes' tree, the members ascending -- that depends on the plan's pitch
// and the window alone, never on the launch: results are identical from run to run and for every batch a scenario sits in.
// No limit on the number of series (af_series_kernel stops at 1 024 padded ones).
// Scratch (engine-owned, shared with the pooled and windowed analyzers): 4 B per edge + 8 B per series + 4 B per group +
// 4 B per scenario (+ up to 256 B of alignment for each of the eight parts), and -- unless every group is a single scenario --
// 20 B per (scenario, window, series): 8 B sum, 4 B each min, max (as keys), above.
// Every key of a value lies strictly between 0 and 0xFFFFFFFF (no NaN is sampled), so a lane, a record or a member without a row
// keeps 0xFFFFFFFF / 0 and never wins; keys become words again only where a cell is written.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "af_summary.hpp"

namespace afsw {

constexpr int kThreads = 256;             // the partial kernel: four waves, four work items
constexpr int kWaves = kThreads / 64;
constexpr int kReduceThreads = 256;
constexpr uint32_t kSkip = 0xFFFFFFFFu;   // AF_POOL_SKIP
constexpr uint32_t kUnroll = 4;           // 16-byte loads a lane has in flight

struct SwinArgs {
    const uint32_t* samples;   // [n][tick_cap][pitch]
    const uint32_t* counts;    // [n][8]
    uint32_t tick_cap, pitch, n_series, n_edges, cnt_ticks_slot;
    const uint32_t* group;     // [n] or null (all in group 0)
    uint32_t n_scen, n_groups, n_win;
    uint32_t run;              // windows per work item of the partial kernel
    uint32_t direct;           // every group is one scenario or none: the partial kernel writes the cells
    const uint32_t* edges;     // [W + 1]
    const double* thr;         // [n_series]
    const uint32_t* mem_off;   // [G + 1] into members
    const uint32_t* members;   // the scenarios of group 0, of group 1, ... each ascending
    unsigned long long* rec_sum;   // [n][W][n_series] u64 sum, or the bits of the f64 sum of a float column
    uint32_t *rec_min, *rec_max, *rec_above;
    uint32_t* count;           // [G][W]
    double* mean;              // [G][W][n_series]
    uint32_t *minv, *maxv, *above;   // same shape, or null
};

__device__ __forceinline__ uint32_t stored_ticks(const SwinArgs& a, uint32_t s) {
    const uint32_t m = a.counts[(size_t)s * 8u + a.cnt_ticks_slot];
    return m < a.tick_cap ? m : a.tick_cap;
}

// what a lane keeps of one column: ONE 64-bit sum -- the u64 sum of the words, or the bits of the f64 sum of the float values of
// a ram_in_use column (the form the record stores) --, min / max of the keys (the words; float_key of a ram_in_use word), the
// values above the threshold
struct Col {
    unsigned long long sum = 0ull;   // (+0.0 as a double)
    uint32_t mn = 0xFFFFFFFFu, mx = 0u, ab = 0u;
    __device__ __forceinline__ static unsigned long long plus(unsigned long long acc, unsigned long long v, bool is_f) {
        return is_f ? (unsigned long long)__double_as_longlong(__longlong_as_double((long long)acc) + __longlong_as_double((long long)v))
                    : acc + v;
    }
    __device__ __forceinline__ void add(uint32_t w, bool is_f, double thr) {
        const double x = is_f ? (double)__uint_as_float(w) : (double)w;
        sum = plus(sum, is_f ? (unsigned long long)__double_as_longlong(x) : (unsigned long long)w, is_f);
        const uint32_t key = is_f ? afs::float_key(w) : w;
        mn = key < mn ? key : mn;
        mx = key > mx ? key : mx;
        ab += x > thr ? 1u : 0u;
    }
    // the partner hdist lanes up; `take` where this lane is the left operand of the tree
    __device__ __forceinline__ void fold(int hdist, bool take, bool is_f) {
        const unsigned long long osum = __shfl_down(sum, hdist, 64);
        const uint32_t omn = __shfl_down(mn, hdist, 64), omx = __shfl_down(mx, hdist, 64), oab = __shfl_down(ab, hdist, 64);
        if (take) {
            sum = plus(sum, osum, is_f);
            mn = omn < mn ? omn : mn;
            mx = omx > mx ? omx : mx;
            ab += oab;
        }
    }
    __device__ __forceinline__ double total(bool is_f) const { return is_f ? __longlong_as_double((long long)sum) : (double)sum; }
    // a key of a cell that holds a value -> the word that is written
    __device__ __forceinline__ static uint32_t word(uint32_t key, bool is_f) { return is_f ? afs::float_unkey(key) : key; }
};

__global__ __launch_bounds__(kThreads) void af_swin_partial(SwinArgs a) {
    const int lane = threadIdx.x & 63;
    const uint32_t W = a.n_win;
    const uint32_t runs = (W + a.run - 1u) / a.run;   // work items per scenario
    const uint64_t item = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (item >= (uint64_t)a.n_scen * runs) return;
    const uint32_t s = (uint32_t)(item / runs), w0 = (uint32_t)(item % runs) * a.run;
    const uint32_t w1 = W - w0 < a.run ? W : w0 + a.run;
    const uint32_t g = a.group ? a.group[s] : 0u;
    if (g == kSkip || g >= a.n_groups) return;
    const uint32_t m = stored_ticks(a, s);
    const uint32_t pq = a.pitch / 4u;
    const uint32_t L = pq < 64u ? pq : 64u;     // lanes per row
    const uint32_t rps = 64u / L;               // rows per step of the wave
    const uint32_t row_off = (uint32_t)lane / L;
    const bool lane_on = row_off < rps;
    uint32_t p2 = 1u;
    while (p2 < rps) p2 <<= 1;
    const uint4* rows = reinterpret_cast<const uint4*>(a.samples) + (size_t)s * a.tick_cap * pq;
    const uint32_t S = a.n_series;
    for (uint32_t cg0 = 0; cg0 < pq; cg0 += 64u) {
        const uint32_t cg = cg0 + (uint32_t)lane % L;
        const bool on = lane_on && cg < pq;
        bool is_f[4];
        double thr[4];
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            const uint32_t j = cg * 4u + k;
            is_f[k] = afs::series_is_float(j, a.n_edges, S);
            thr[k] = j < S ? a.thr[j] : 0.0;
        }
        for (uint32_t w = w0; w < w1; ++w) {
            uint32_t r0 = a.edges[w], r1 = a.edges[w + 1u];
            r0 = r0 < m ? r0 : m;
            r1 = r1 < m ? r1 : m;
            Col c[4];
            if (on) {
                for (uint32_t r = r0 + row_off; r < r1; r += kUnroll * rps) {
                    uint4 v[kUnroll];
#pragma unroll
                    for (uint32_t u = 0; u < kUnroll; ++u)   // (r1 <= tick_cap < 2^31: no wrap)
                        v[u] = r + u * rps < r1 ? rows[(size_t)(r + u * rps) * pq + cg] : uint4{};
#pragma unroll
                    for (uint32_t u = 0; u < kUnroll; ++u)
                        if (r + u * rps < r1) {
                            c[0].add(v[u].x, is_f[0], thr[0]);
                            c[1].add(v[u].y, is_f[1], thr[1]);
                            c[2].add(v[u].z, is_f[2], thr[2]);
                            c[3].add(v[u].w, is_f[3], thr[3]);
                        }
                }
            }
            for (uint32_t h = p2 >> 1; h >= 1u; h >>= 1) {   // (uniform: every lane of the wave shuffles)
                const bool take = row_off < h && row_off + h < rps;
#pragma unroll
                for (int k = 0; k < 4; ++k) c[k].fold((int)(h * L), take, is_f[k]);
            }
            if (!on || row_off != 0u) continue;
            const uint32_t cnt = r1 - r0;
            if (a.direct) {
                const size_t cell = (size_t)g * W + w;
                if (cg == 0u) a.count[cell] = cnt;
#pragma unroll
                for (uint32_t k = 0; k < 4u; ++k) {
                    const uint32_t j = cg * 4u + k;
                    if (j >= S) continue;
                    const size_t o = cell * S + j;
                    a.mean[o] = cnt ? c[k].total(is_f[k]) / (double)cnt : __builtin_nan("");
                    if (a.minv) a.minv[o] = cnt ? Col::word(c[k].mn, is_f[k]) : 0u;
                    if (a.maxv) a.maxv[o] = cnt ? Col::word(c[k].mx, is_f[k]) : 0u;
                    if (a.above) a.above[o] = c[k].ab;
                }
            } else {
#pragma unroll
                for (uint32_t k = 0; k < 4u; ++k) {
                    const uint32_t j = cg * 4u + k;
                    if (j >= S) continue;
                    const size_t o = ((size_t)s * W + w) * S + j;
                    a.rec_sum[o] = c[k].sum;
                    a.rec_min[o] = c[k].mn;
                    a.rec_max[o] = c[k].mx;
                    a.rec_above[o] = c[k].ab;
                }
            }
        }
    }
}

// entries [first, first + n_entries) of the (group, window, series) array
__global__ __launch_bounds__(kReduceThreads) void af_swin_reduce(SwinArgs a, uint64_t first, uint64_t n_entries) {
    const uint64_t idx = first + (uint64_t)blockIdx.x * kReduceThreads + threadIdx.x;
    if (idx >= n_entries) return;
    const uint32_t S = a.n_series, W = a.n_win;
    const uint64_t cell = idx / S;
    const uint32_t j = (uint32_t)(idx % S);
    const uint32_t g = (uint32_t)(cell / W), w = (uint32_t)(cell % W);
    const uint32_t k0 = a.mem_off[g], k1 = a.mem_off[g + 1u];
    if (a.direct && k1 != k0) return;   // its one member's wave wrote the cell
    const bool is_f = afs::series_is_float(j, a.n_edges, S);
    const uint32_t b0 = a.edges[w], b1 = a.edges[w + 1u];
    unsigned long long si = 0ull;
    double sf = 0.0;
    uint32_t mn = 0xFFFFFFFFu, mx = 0u, ab = 0u, cnt = 0u;
    for (uint32_t k = k0; k < k1; ++k) {
        const uint32_t s = a.members[k];
        const uint32_t m = stored_ticks(a, s);
        cnt += (b1 < m ? b1 : m) - (b0 < m ? b0 : m);
        const size_t o = ((size_t)s * W + w) * S + j;
        const unsigned long long v = a.rec_sum[o];
        if (is_f) sf = sf + __longlong_as_double((long long)v);
        else si += v;
        const uint32_t rmn = a.rec_min[o], rmx = a.rec_max[o];
        mn = rmn < mn ? rmn : mn;
        mx = rmx > mx ? rmx : mx;
        ab += a.rec_above[o];
    }
    if (j == 0u) a.count[cell] = cnt;
    a.mean[idx] = cnt ? (is_f ? sf : (double)si) / (double)cnt : __builtin_nan("");
    if (a.minv) a.minv[idx] = cnt ? Col::word(mn, is_f) : 0u;
    if (a.maxv) a.maxv[idx] = cnt ? Col::word(mx, is_f) : 0u;
    if (a.above) a.above[idx] = ab;
}

}  // namespace afsw
