// Quantile analyzer: any latency quantiles and SLO counts of every (group, time window) of a batch, or of every group over the
// whole run (af_engine_summarize_quantiles).  The cells and their samples are the windowed analyzer's (af_windowed.hpp:
// af_win_bounds / af_win_compact, used as they are) or, without windows, the pooled analyzer's (af_pooled.hpp:
// af_pool_compact): the latencies of cell c lie contiguous at lat[cell_off[c] .. cell_off[c + 1]).
// For a cell of n >= 1 latencies x[0] <= ... <= x[n-1] and a level q in [0, 1]   (numpy: np.quantile(a, q), method 'linear')
//     v = (double)(n - 1) * q;  lo = floor(v);  hi = min(lo + 1, n - 1);  t = v - lo;  d = x[hi] - x[lo]
//     quantile = t >= 0.5 ? x[hi] - d * (1 - t) : x[lo] + d * t                                          (numpy's _lerp)
// and for a threshold th:  within = #{ x <= th }, compared as f64.  An empty cell: count 0, quantiles NaN, within 0.
//   * level 0.5 is np.quantile(a, 0.5).  It is NOT always the `median` column of the other analyzers bit for bit: np.median is
//     the mean of the middle pair, (x[lo] + x[hi]) / 2, and x[lo] + d * 0.5 (or x[hi] - d * 0.5) rounds differently in about one
//     sample of 280.
//   * levels 0.95 and 0.99 DO equal the p95 / p99 columns (np.percentile(a, 95) is this formula at 95 / 100), 0 and 1 min / max.
// Three tiers by the cell's size, none of which adds floating-point numbers, so a result depends on the cell's VALUES alone:
//   tiny   <= kTinyMax (512): ONE WAVE per cell, four cells per workgroup.  The cell in LDS; the place of every latency in the
//          sorted cell by counting (#{y < x} + #{equal ones before it}); the sorted cell to a second LDS array.  Any number of
//          levels and thresholds is then a read / a binary search per lane.
//   small  <= kSmallMax (8 192): ONE WORKGROUP per cell: the cell, padded with +inf to a power of two P, is sorted in P * 8 B
//          of LDS (bitonic), read like the tiny tier's.  The cells are launched by P, so a cell of 1 300 latencies takes
//          16 KB and 66 exchange steps, not 64 KB and 91: at 64 KB two workgroups (32 waves) share a CU's 160 KB, at 16 KB the
//          wave slots limit (4 workgroups of 512).
//          (Steps whose pairs stay inside a wave's own elements, run without the workgroup barrier, measured no faster.)
//   large  above: MSB-first radix select (af_select.hpp) over the compacted range, as af_pooled.hpp's: the cell's exponent histogram, then
//          10 key bits per pass under the wanted ranks' prefixes (af_pool_digits, as it is) until every rank has <= kCand
//          candidates, the candidates to global memory, selection among them by counting.  The per-rank histograms of ONE
//          workgroup hold kRanks = 6 ranks = the lo / hi of kLv = 3 levels: more levels run as ceil(n_levels / 3) independent
//          JOBS per cell (the rounds), each with the pooled analyzer's per-group state.  `within` comes from the pass that
//          builds the exponent histogram: lane t of a wave keeps the count of threshold t.  Latencies here are >= +0.0 (the
//          key order is the value order), as in af_summary.hpp.
// Integer atomics only (histograms, candidate slots, within counts); the candidates' order does not matter to selection by
// counting: results are identical from run to run.
// Scratch (engine-owned, shared with the pooled / windowed analyzers): the compaction's (8 B per latency in a cell + 4 B per
// (scenario, edge) + 4 B per (scenario, window) + 8 B per edge, or 8 B per scenario without windows) + 8 B per cell + 4 B per
// small cell + 8 B per level and threshold; per large cell 16 B + 4 B per threshold + 16 B per 131 072 latencies, and per JOB
// of a large cell af_pooled.hpp's per-group state (~57 KB) + 16 B + 16 B per 131 072 latencies.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "af_pooled.hpp"

namespace afq {

using afs::kThreads, afs::kRanks, afs::kCand, afs::kPiece, afs::kExpBins, afs::kDigBins, afs::key_of, afs::level_ranks, afs::lerp;
constexpr int kLv = 3;                      // levels per job of the large tier: their lo / hi ranks are one workgroup's kRanks
static_assert(2 * kLv == kRanks, "a job's ranks are the lo / hi of its levels");
constexpr uint32_t kMaxLevels = 64;         // AF_MAX_QUANTILE_LEVELS
constexpr uint32_t kMaxThresholds = 64;     // AF_MAX_SLO_THRESHOLDS: one lane of a wave per threshold
constexpr uint32_t kTinyMax = 512;          // latencies of the largest cell one wave sorts
constexpr int kTinyWaves = 4;               // cells per workgroup of the wave kernel (32 KB of LDS)
constexpr uint32_t kSmallMax = 8192;        // latencies of the largest cell one workgroup sorts (64 KB of LDS)
constexpr uint32_t kSmallMinPad = 1024;     // smallest padded size of the workgroup sort

struct QCell {   // a large cell
    uint64_t off;      // first latency in the compacted array
    uint32_t n;        // latencies
    uint32_t row;      // its cell index: the row of the outputs
};

struct QJob {    // levels [lev0, lev0 + n_lev) of large cell lc; its select state is groups[job] of the PoolArgs
    uint32_t lc, lev0, n_lev, pad;
};

struct QArgs {
    const double* lat;          // compacted latencies
    const uint64_t* cell_off;   // [C + 1]
    uint32_t n_lev, n_thr;
    const double* levels;       // [n_lev]
    const double* thr;          // [n_thr]
    uint32_t* count;            // [C] or null
    double* quant;              // [C][n_lev] or null
    uint32_t* within;           // [C][n_thr] or null
    const uint32_t* small;      // the cells of kTinyMax < latencies <= kSmallMax, by padded size
    const QCell* lcells;        // the large cells
    const afp::PoolTile* ctiles;   // their tiles (group = index into lcells)
    const QJob* jobs;
    uint32_t* thist;            // [large cells][n_thr] within counts
};

// #{ i < n : s[i] <= th } of a sorted array
__device__ __forceinline__ uint32_t count_leq(const double* s, uint32_t n, double th) {
    uint32_t lo = 0u, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (s[mid] <= th) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// the rows of cell `cell` from its n >= 1 sorted latencies: thread t of the caller (at least 64 call) writes column t
__device__ __forceinline__ void write_sorted_cell(const QArgs& a, uint64_t cell, const double* s, uint32_t n, uint32_t t) {
    if (t == 0u && a.count) a.count[cell] = n;
    if (t < a.n_lev && a.quant) {
        uint32_t lo, hi;
        double w;
        level_ranks(n, a.levels[t], lo, hi, w);
        a.quant[cell * a.n_lev + t] = lerp(s[lo], s[hi], w);
    }
    if (t < a.n_thr && a.within) a.within[cell * a.n_thr + t] = count_leq(s, n, a.thr[t]);
}

__device__ __forceinline__ void write_empty_cell(const QArgs& a, uint64_t cell, uint32_t t) {
    if (t == 0u && a.count) a.count[cell] = 0u;
    if (t < a.n_lev && a.quant) a.quant[cell * a.n_lev + t] = __builtin_nan("");
    if (t < a.n_thr && a.within) a.within[cell * a.n_thr + t] = 0u;
}

// one WAVE per cell of <= kTinyMax latencies (and the empty cells' rows)
__global__ __launch_bounds__(kTinyWaves * 64) void af_q_tiny(QArgs a, uint64_t cell0, uint64_t n_cells) {
    __shared__ double buf[kTinyWaves][kTinyMax];
    __shared__ double srt[kTinyWaves][kTinyMax];
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
    double* s = srt[wave];
    for (uint32_t i = lane; i < n; i += 64u) b[i] = a.lat[off + i];
    __syncthreads();
    for (uint32_t i0 = 0; i0 < n; i0 += 64u) {   // every latency to its place: those below it, then the equal ones before it
        const uint32_t i = i0 + (uint32_t)lane;
        if (i < n) {
            const double x = b[i];
            uint32_t at = 0u;
            for (uint32_t k = 0; k < n; ++k) {
                const double y = b[k];
                at += (y < x || (y == x && k < i)) ? 1u : 0u;
            }
            s[at] = x;
        }
    }
    __syncthreads();
    if (!mine) return;
    if (n == 0u) write_empty_cell(a, cell, (uint32_t)lane);
    else write_sorted_cell(a, cell, s, n, (uint32_t)lane);
}

// one workgroup per listed cell (kTinyMax < latencies <= pad <= kSmallMax): bitonic sort of the padded cell in `pad` * 8 B of LDS
__global__ __launch_bounds__(kThreads) void af_q_small(QArgs a, uint32_t first, uint32_t pad) {
    extern __shared__ __attribute__((aligned(8))) unsigned char dyn[];
    double* s = reinterpret_cast<double*>(dyn);
    const uint32_t tid = threadIdx.x;
    const uint64_t cell = a.small[first + blockIdx.x];
    const uint64_t off = a.cell_off[cell];
    const uint32_t n = (uint32_t)(a.cell_off[cell + 1u] - off);
    for (uint32_t i = tid; i < pad; i += kThreads) s[i] = i < n ? a.lat[off + i] : __builtin_inf();
    __syncthreads();
    for (uint32_t k = 2u; k <= pad; k <<= 1)
        for (uint32_t j = k >> 1; j > 0u; j >>= 1) {
            for (uint32_t i = tid; i < (pad >> 1); i += kThreads) {
                const uint32_t lo = ((i & ~(j - 1u)) << 1) | (i & (j - 1u)), hi = lo | j;   // (lo < hi < pad)
                const bool up = (lo & k) == 0u;
                const double x = s[lo], y = s[hi];
                if ((x > y) == up && x != y) {
                    s[lo] = y;
                    s[hi] = x;
                }
            }
            __syncthreads();
        }
    write_sorted_cell(a, cell, s, n, tid);
}

// large cells, first pass: the exponent histogram of the cell (when levels are wanted) and the within counts
__global__ __launch_bounds__(kThreads) void af_q_pass0(QArgs a, uint32_t* hist0) {
    __shared__ uint32_t hist[kExpBins];
    const int tid = threadIdx.x, lane = tid & 63;
    const afp::PoolTile t = a.ctiles[blockIdx.x];
    const QCell c = a.lcells[t.group];
    const bool want_hist = a.n_lev > 0u && a.quant;
    const uint32_t T = a.within ? a.n_thr : 0u;
    for (int i = tid; i < kExpBins; i += kThreads) hist[i] = 0u;
    __syncthreads();
    const uint32_t len = afp::tile_len(t, c.n);
    const double* src = a.lat + c.off + (uint64_t)t.piece * kPiece;
    uint32_t acc = 0u;   // lane t: the latencies <= thr[t] this wave has met
    constexpr uint32_t kU = 4;
    for (uint32_t base = 0; base < len; base += kU * kThreads) {   // (uniform trip count: the ballots below are wave-wide)
        double x[kU];
#pragma unroll
        for (uint32_t u = 0; u < kU; ++u) x[u] = base + tid + u * kThreads < len ? src[base + tid + u * kThreads] : 0.0;
#pragma unroll
        for (uint32_t u = 0; u < kU; ++u) {
            const bool act = base + tid + u * kThreads < len;
            if (want_hist) afs::wave_agg_add(hist, (uint32_t)(key_of(x[u]) >> 52) & (kExpBins - 1), act);
            for (uint32_t k = 0; k < T; ++k) {
                const uint32_t c_k = (uint32_t)__popcll(__ballot(act && x[u] <= a.thr[k]));
                if ((uint32_t)lane == k) acc += c_k;
            }
        }
    }
    if ((uint32_t)lane < T && acc) atomicAdd(&a.thist[(size_t)t.group * a.n_thr + lane], acc);
    __syncthreads();
    if (want_hist)
        for (int i = tid; i < kExpBins; i += kThreads)
            if (hist[i]) atomicAdd(&hist0[(size_t)t.group * kExpBins + i], hist[i]);
}

// one workgroup per job: level 0 (after af_q_pass0) or a digit level (after af_pool_digits): afp::select_step for the job's ranks
__global__ __launch_bounds__(kThreads) void af_q_select(QArgs qa, afp::PoolArgs a, int level) {
    __shared__ uint32_t want[kRanks];
    const int tid = threadIdx.x;
    const uint32_t ji = blockIdx.x;
    const QJob job = qa.jobs[ji];
    afp::PoolGroup* g = a.groups + ji;
    if (level == 0 && tid < kLv) {   // (a job of fewer than kLv levels repeats its first: the same prefixes, no slot more)
        const uint32_t l = job.lev0 + ((uint32_t)tid < job.n_lev ? (uint32_t)tid : 0u);
        uint32_t lo, hi;
        double t;
        level_ranks(g->n, qa.levels[l], lo, hi, t);
        want[2 * tid] = lo;
        want[2 * tid + 1] = hi;
    }
    afp::select_step(g, want, a.hist0 + (size_t)job.lc * kExpBins, a.dhist + (size_t)ji * kRanks * kDigBins, level, a.any_more);
}

// the <= kCand candidates of every rank of the tile's job into global memory (af_pool_last without its sums)
__global__ __launch_bounds__(kThreads) void af_q_cand(afp::PoolArgs a) {
    const uint32_t tid = threadIdx.x;
    const afp::PoolTile t = a.tiles[blockIdx.x];
    const afp::PoolGroup* g = a.groups + t.group;
    const int shift = g->shift;
    if (shift == 0) return;   // the whole key is known
    uint64_t sp[kRanks];
    afs::load_slot_prefixes(sp, g->slot_pfx, g->n_slots);
    uint32_t* cn = a.cand_n + (size_t)t.group * kRanks;
    double* cd = a.cand + (size_t)t.group * kRanks * kCand;
    const uint32_t len = afp::tile_len(t, g->n);
    const double* src = a.lat + g->off + (uint64_t)t.piece * kPiece;
    constexpr uint32_t kU = 4;
    for (uint32_t i0 = tid; i0 < len; i0 += kU * kThreads) {
        double x[kU];
#pragma unroll
        for (uint32_t u = 0; u < kU; ++u) x[u] = i0 + u * kThreads < len ? src[i0 + u * kThreads] : 0.0;
#pragma unroll
        for (uint32_t u = 0; u < kU; ++u)
            if (i0 + u * kThreads < len) afs::collect_candidate(x[u], shift, sp, cn, cd);
    }
}

// one workgroup per job: the ranks' values among the candidates, the job's quantiles
__global__ __launch_bounds__(kThreads) void af_q_final(QArgs qa, afp::PoolArgs a) {
    __shared__ double cand[kRanks * kCand];
    __shared__ double val[kRanks];
    const int tid = threadIdx.x;
    const uint32_t ji = blockIdx.x;
    const QJob job = qa.jobs[ji];
    const afp::PoolGroup* g = a.groups + ji;
    afp::load_candidates(a, ji, g, cand);
    afs::rank_values(cand, a.cand_n + (size_t)ji * kRanks, g->slot_of, g->rank_in, g->pfx, g->shift, val);
    __syncthreads();
    if ((uint32_t)tid < job.n_lev) {
        const uint32_t l = job.lev0 + (uint32_t)tid;
        uint32_t lo, hi;
        double t;
        level_ranks(g->n, qa.levels[l], lo, hi, t);
        qa.quant[(size_t)qa.lcells[job.lc].row * qa.n_lev + l] = lerp(val[2 * tid], val[2 * tid + 1], t);
    }
}

// one wave per large cell: its count and within rows
__global__ __launch_bounds__(64) void af_q_large_rows(QArgs a) {
    const uint32_t lc = blockIdx.x, lane = threadIdx.x;
    const QCell c = a.lcells[lc];
    if (lane == 0u && a.count) a.count[c.row] = c.n;
    if (lane < a.n_thr && a.within) a.within[(size_t)c.row * a.n_thr + lane] = a.thist[(size_t)lc * a.n_thr + lane];
}

}  // namespace afq
