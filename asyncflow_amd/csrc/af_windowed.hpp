// Windowed analyzer: the eight latency statistics of every (group, time window) of a batch (af_engine_summarize_windows).
// Windows are by FINISH time: with edges e[0] < ... < e[W], window w of scenario s holds its rows with e[w] < finish <= e[w+1]
// (the bucket rule of the throughput series).  rqs_clock rows are in completion order, so finish is non-decreasing within a
// scenario and a window is a CONTIGUOUS row range [r_s[w], r_s[w+1]), r_s[k] = #{stored rows with finish <= e[k]}.  The sample
// of CELL c = g * W + w is the concatenation, in ascending scenario index over the members of group g, of finish - start over
// those ranges; its statistics are numpy's on that array, bit for bit (af_summary.hpp, af_pooled.hpp).
//   bounds    one lane per (scenario, edge): r_s[k] by binary search on the finish column (log2(rows) 16-byte rows each)
//   (host)    reads the bounds back: the cells' sizes and offsets, and per (scenario, window) how many latencies of its cell
//             come from earlier members (u32: a cell holds < 2^32 latencies)
//   compact   one workgroup per scenario: every stored row is read once -- finish[i] < finish[i-1] sets the error word (the
//             assumption the windows rest on, checked where the rows are read anyway) -- and the rows inside [e[0], e[W]] go
//             to their cell's place in the compacted array; the row's window by binary search over the scenario's bounds in LDS
//   tiny      a cell of <= kTinyMax latencies is reduced by ONE WAVE (four cells per workgroup): the latencies staged in LDS,
//             numpy's pairwise sum with the wave's eight 8-lane groups as the recursion's (at most eight) leaves, the wanted
//             ranks by counting over the whole cell.  No histograms, no barrier but the one after staging.
//   small     a cell of <= kPiece latencies (one numpy piece) is reduced by ONE workgroup, everything in LDS, as
//             af_summary_kernel does for a scenario: numpy's pairwise sum, min / max, exponent histogram; then that kernel's
//             own afs::select_and_finish: MSB-first radix select (af_select.hpp), squared deviations and candidates.  No
//             global scratch per cell beyond its offset and list entry.
//   large     cells above one piece take the pooled analyzer's tiled passes (af_pooled.hpp) over their compacted range, with
//             that analyzer's per-group scratch -- for them only.
// Scratch (engine-owned, shared with the pooled analyzer): 8 B per windowed latency + 4 B per (scenario, edge) (the bounds,
// unless the caller takes them) + 4 B per (scenario, window) + 8 B per cell (+ 4 B per small cell) + 8 B per edge +
// af_pooled.hpp's per large cell.
// Integer atomics only; the candidates' order does not matter to selection by counting: results are run-to-run identical.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "af_pooled.hpp"

namespace afw {

using afs::kThreads, afs::kWaves, afs::kRanks, afs::kExpBins, afs::kDigBins;
using afp::kSkip;
constexpr uint32_t kSmallMax = afs::kPiece;   // latencies of the largest cell one workgroup reduces
constexpr uint32_t kTinyMax = 512;            // latencies of the largest cell one wave reduces
constexpr int kTinyWaves = 4;                 // cells per workgroup of the wave kernel
constexpr int kBoundsThreads = 256;
constexpr uint32_t kLdsWindows = 4096;        // windows whose bounds and destinations the compaction keeps in LDS (48 KB)
constexpr uint32_t kNoError = 0xFFFFFFFFu;

struct WinArgs {
    const double* clock;      // [n][clock_cap][2]
    const uint32_t* counts;   // [n][8]
    uint32_t clock_cap, cnt_completed_slot;
    const uint32_t* group;    // [n] or null (all in group 0)
    uint32_t n_scen, n_win;
    const double* edges;      // [W + 1]
    uint32_t* bounds;         // [n][W + 1]  r_s[k]
    uint32_t* pre;            // [n][W] latencies of cell (group[s], w) that come from members before s (af_arrival.hpp advances it)
    const uint64_t* cell_off; // [C + 1] first latency of every cell in the compacted array
    double* lat;              // compacted latencies
    uint32_t* err;            // [1] smallest scenario index with an inversion (kNoError: none)
    const uint32_t* small;    // the cells of kTinyMax < latencies <= kSmallMax
    double* stats;            // [C][8]
};

// r_s[k] = #{ i < m_s : finish[s, i] <= e[k] }
__global__ __launch_bounds__(kBoundsThreads) void af_win_bounds(WinArgs a) {
    const uint64_t idx = (uint64_t)blockIdx.x * kBoundsThreads + threadIdx.x;
    const uint32_t ne = a.n_win + 1u;
    if (idx >= (uint64_t)a.n_scen * ne) return;
    const uint32_t s = (uint32_t)(idx / ne), k = (uint32_t)(idx % ne);
    uint32_t m = a.counts[(size_t)s * 8u + a.cnt_completed_slot];
    if (m > a.clock_cap) m = a.clock_cap;
    const double2* ck = reinterpret_cast<const double2*>(a.clock) + (size_t)s * a.clock_cap;
    const double e = a.edges[k];
    uint32_t lo = 0u, hi = m;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (ck[mid].y <= e) lo = mid + 1u;
        else hi = mid;
    }
    a.bounds[idx] = lo;
}

// the window of row i: bs[w] <= i < bs[w + 1] (the caller has bs[0] <= i < bs[W])
__device__ __forceinline__ uint32_t window_of(const uint32_t* bs, uint32_t n_win, uint32_t i) {
    uint32_t lo = 0u, hi = n_win - 1u;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (bs[mid + 1u] <= i) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// every stored row of scenario blockIdx.x: order check; finish - start of the rows inside the windows to their cells
template <bool kLds>
__global__ __launch_bounds__(kThreads) void af_win_compact(WinArgs a) {
    extern __shared__ __attribute__((aligned(8))) unsigned char dyn[];   // kLds: [W] u64 destinations - first row, then [W + 1] bounds
    const uint32_t s = blockIdx.x;
    const uint32_t g = a.group ? a.group[s] : 0u;
    if (g == kSkip) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t W = a.n_win;
    uint32_t m = a.counts[(size_t)s * 8u + a.cnt_completed_slot];
    if (m > a.clock_cap) m = a.clock_cap;
    const double2* ck = reinterpret_cast<const double2*>(a.clock) + (size_t)s * a.clock_cap;
    const uint32_t* gb = a.bounds + (size_t)s * (W + 1u);
    const uint32_t* gpre = a.pre + (size_t)s * W;
    const uint64_t* goff = a.cell_off + (size_t)g * W;
    uint64_t* ldst = reinterpret_cast<uint64_t*>(dyn);
    uint32_t* lb = reinterpret_cast<uint32_t*>(dyn + (size_t)(kLds ? W : 0u) * 8u);
    if (kLds) {
        for (uint32_t k = tid; k <= W; k += kThreads) lb[k] = gb[k];
        for (uint32_t w = tid; w < W; w += kThreads) ldst[w] = goff[w] + gpre[w] - gb[w];   // (+ the row's index: its place)
        __syncthreads();
    }
    const uint32_t* bs = kLds ? lb : gb;
    const uint32_t r0 = bs[0], rW = bs[W];
    bool bad = false;
    constexpr uint32_t kU = 4;
    for (uint32_t base = 0; base < m; base += kU * kThreads) {   // (uniform trip count: the shuffles below are wave-wide)
        const uint32_t i0 = base + (uint32_t)tid;
        double2 c[kU];
#pragma unroll
        for (uint32_t u = 0; u < kU; ++u) c[u] = i0 + u * kThreads < m ? ck[i0 + u * kThreads] : double2{};
#pragma unroll
        for (uint32_t u = 0; u < kU; ++u) {
            const uint32_t i = i0 + u * kThreads;
            double prev = __shfl_up(c[u].y, 1, 64);   // the row before this one: the lane below holds it, but for a wave's first lane
            if (lane == 0 && i > 0u && i < m) prev = ck[i - 1u].y;
            if (i > 0u && i < m && c[u].y < prev) bad = true;
            if (i >= r0 && i < rW) {
                const uint32_t w = window_of(bs, W, i);
                const uint64_t d = kLds ? ldst[w] + i : goff[w] + gpre[w] + (i - gb[w]);
                a.lat[d] = c[u].y - c[u].x;
            }
        }
    }
    if (bad) atomicMin(a.err, s);
}

// numpy's pairwise sum of f(q[i]), i < m <= kTinyMax, by ONE wave: afs::numpy_sum's partial piece with the wave's eight 8-lane
// groups as the recursion's leaves (a leaf holds 64 .. 128 elements, or all of them: at most eight, at most three levels
// down) and the recursion's additions in registers, the same in every lane.
template <class F>
__device__ __forceinline__ double wave_numpy_sum(const double* q, uint32_t m, F&& f) {
    const int lane = threadIdx.x & 63;
    const uint32_t j = (uint32_t)lane & 7u, g = (uint32_t)lane >> 3;
    const uint32_t e = 64u * g;
    uint32_t o = 0u, len = m, path = 0u, depth = 0u;
    bool mine = g < (m + 63u) / 64u;
    if (mine) {   // the leaf of element 64 g, taken if that is its first such element
        while (len > 128u) {
            const uint32_t n2 = (len >> 1) & ~7u;
            if (e - o < n2) { len = n2; path <<= 1; }
            else { o += n2; len -= n2; path = (path << 1) | 1u; }
            depth += 1u;
        }
        if (g > 0u && e - 64u >= o) mine = false;
    }
    const uint32_t rows = mine ? len >> 3 : 0u, rem = mine ? len & 7u : 0u;
    double acc = -0.0;
    for (uint32_t r = 0; r < (uint32_t)afs::kLeafRows; ++r)
        if (r < rows) acc = acc + f(q[o + r * 8u + j]);
    double leaf = afs::xor_add(acc, 1);
    leaf = afs::xor_add(leaf, 2);
    leaf = afs::xor_add(leaf, 4);
    if (rows == 0u) leaf = -0.0;   // n < 8: one after the other, from -0.0
    {
        const double x = j < rem ? f(q[o + 8u * rows + j]) : 0.0;
#pragma unroll
        for (int t = 0; t < 7; ++t) {
            const double xt = __shfl(x, (lane & ~7) + t, 64);
            if ((uint32_t)t < rem) leaf = leaf + xt;
        }
    }
    const int slot = mine ? (int)(path << (3u - depth)) : 8;   // (a leaf of depth d with path p: the first of its 8 >> d slots)
    double v[8];
    uint32_t has = 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int sk = __shfl(slot, 8 * k, 64);
        const double lk = __shfl(leaf, 8 * k, 64);
#pragma unroll
        for (int p = 0; p < 8; ++p)
            if (sk == p) {
                v[p] = lk;
                has |= 1u << p;
            }
    }
#pragma unroll
    for (int st = 1; st < 8; st <<= 1)   // the recursion's additions, bottom up; an absent right half = a leaf higher up
#pragma unroll
        for (int p = 0; p < 8; p += 2 * st)
            if ((has >> (p + st)) & 1u) v[p] = v[p] + v[p + st];
    return 0.0 + v[0];
}

// one WAVE per cell of <= kTinyMax latencies (and the empty cells' rows)
__global__ __launch_bounds__(kTinyWaves * 64) void af_win_tiny(WinArgs a, uint64_t cell0, uint64_t n_cells) {
    __shared__ double buf[kTinyWaves][kTinyMax];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t cell = cell0 + (uint64_t)blockIdx.x * kTinyWaves + (uint64_t)wave;
    uint64_t off = 0u;
    uint32_t n = 0u;
    bool mine = false;
    if (cell < n_cells) {
        off = a.cell_off[cell];
        const uint64_t len = a.cell_off[cell + 1u] - off;
        mine = len <= (uint64_t)kTinyMax;
        n = mine ? (uint32_t)len : 0u;
    }
    double* b = buf[wave];
    double mn = __builtin_inf(), mx = -__builtin_inf();
    for (uint32_t i = lane; i < n; i += 64u) {
        const double x = a.lat[off + i];
        b[i] = x;
        mn = fmin(mn, x);
        mx = fmax(mx, x);
    }
    __syncthreads();
    if (!mine) return;
    double* st = a.stats + cell * 8u;
    if (n == 0u) {
        afs::write_empty_row(st, lane);
        return;
    }
    mn = afs::wave_min(mn);
    mx = afs::wave_max(mx);
    const double mean = wave_numpy_sum(b, n, [](const double x) { return x; }) / (double)n;
    const double sq = wave_numpy_sum(b, n, [mean](const double x) {
        const double d = x - mean;
        return d * d;
    });
    uint32_t want[kRanks];
    double tfrac[2];
    afs::stat_ranks(n, want, tfrac);
    double val[kRanks] = {};
    for (uint32_t i0 = 0; i0 < n; i0 += 64u) {   // the ranks by counting: every latency against the whole cell
        const bool valid = i0 + (uint32_t)lane < n;
        const double x = valid ? b[i0 + (uint32_t)lane] : 0.0;
        uint32_t less = 0u, leq = 0u;
        for (uint32_t k = 0; k < n; ++k) {
            const double y = b[k];
            less += y < x ? 1u : 0u;
            leq += y <= x ? 1u : 0u;
        }
#pragma unroll
        for (int r = 0; r < kRanks; ++r) {
            const unsigned long long hit = __ballot(valid && less <= want[r] && want[r] < leq);
            if (hit) val[r] = __shfl(x, __ffsll((long long)hit) - 1, 64);
        }
    }
    if (lane == 0) afs::write_stats_row(st, n, mean, sq, val, tfrac, mn, mx);
}

// one workgroup per listed cell (kTinyMax < latencies <= kSmallMax): af_summary_kernel over a compacted f64 range
__global__ __launch_bounds__(kThreads) void af_win_small(WinArgs a, uint32_t first) {
    __shared__ uint32_t exp_hist[kExpBins];
    __shared__ __attribute__((aligned(16))) uint32_t dig_hist[kRanks][kDigBins];
    __shared__ double red[2][kWaves];
    __shared__ afs::SelectLds sel;
    __shared__ double wsum[2 * kWaves];
    __shared__ double tail_slots[afs::kTailSlots];

    const int tid = threadIdx.x;
    const uint64_t cell = a.small[first + blockIdx.x];
    const uint64_t off = a.cell_off[cell];
    const uint32_t n = (uint32_t)(a.cell_off[cell + 1u] - off);
    const double* src = a.lat + off;
    for (int i = tid; i < kExpBins; i += kThreads) exp_hist[i] = 0u;
    __syncthreads();

    // ---- pass 1: the sum in numpy's order, min / max, the exponent histogram
    double mn = __builtin_inf(), mx = -__builtin_inf();
    const double total = afs::numpy_sum<8>(src, n, wsum, tail_slots, [&](const double x, const bool act) -> double {
        if (act) {
            mn = fmin(mn, x);
            mx = fmax(mx, x);
        }
        afs::wave_agg_add(exp_hist, (uint32_t)(afs::key_of(x) >> 52) & (kExpBins - 1), act);
        return x;
    });
    if (tid == 0) afs::stat_ranks(n, sel.want, sel.tfrac);
    double vmin, vmax;
    afs::block_min_max(mn, mx, red, vmin, vmax);
    // ---- level 0: exponent bin of every wanted rank; then as the scenarios' kernel goes on
    afs::select_first_level(exp_hist, sel.want, sel.pfx, sel.rank_in, sel.cnt);
    afs::select_and_finish<8>(src, n, [](const double x) { return x; }, 52, total / (double)n, vmin, vmax, sel, &dig_hist[0][0], wsum, tail_slots,
                              a.stats + cell * 8u);
}

}  // namespace afw
