// Pooled analyzer: the eight latency statistics of GROUPS of scenarios, every group's latencies taken as ONE sample
// (af_engine_summarize_pooled).  For group g
//   lat_g = concatenation over its scenarios s, in ascending scenario index, of clock[s, :m_s, 1] - clock[s, :m_s, 0],
//           m_s = min(counts[s][AF_CNT_COMPLETED], clock_capacity)
// and the statistics are numpy's on lat_g, bit for bit, as af_summary.hpp computes them for one scenario: np.mean / np.std add
// in numpy's order -- pieces of 8 192 elements of the CONCATENATED array, each summed pairwise, the piece sums added one after
// the other --, the order statistics by MSB-first radix select, then selection among <= kCand candidates by counting
// (af_select.hpp: the select's steps, here over a group's state in global memory).
//
// A group may be one scenario or a whole batch (10 000 replicas of LB-2 at T = 600 s: 7.6e8 latencies), so a group is spread
// over the chip: the latencies are first COMPACTED into engine-owned scratch (8 B per completion, group after group, members in
// ascending scenario order), and every pass then streams contiguous ranges -- a tile of up to kTilePieces numpy pieces per
// workgroup, any number of tiles per group:
//   compact   one workgroup per scenario: finish - start of its rows to scratch          (reads 16 B, writes 8 B per completion)
//   pass 1    per piece its pairwise sum; per tile min / max and the exponent histogram, added into the group's global one
//   select    one workgroup per group: piece sums in order (mean), min / max, the wanted ranks' bins; more key bits needed?
//   digits    (while some group's rank has > kCand candidates) the next 10 key bits of the elements under the groups' prefixes
//   last      per piece the pairwise sum of (x - mean)^2; the <= kCand candidates of every rank into global memory
//   final     one workgroup per group: squared sums in order (std_dev), the ranks' values among the candidates, the stats row
// Counters are u32: the host rejects a group of 2^32 or more latencies (AF_ERR_CAPACITY).  Integer atomics only (histograms,
// candidate slots); the candidates' order does not matter to selection by counting: results are run-to-run deterministic.
// Scratch (engine-owned, grown on demand, kept until the engine is destroyed):
//   8 B per pooled completion + 8 B per scenario + per group sizeof(PoolGroup) + 8 KB (exponent histogram) + 24 KB (digit
//   histograms) + 24 KB (candidates) + per piece 8 B + per tile 32 B.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "af_summary.hpp"

namespace afp {

using afs::kThreads, afs::kWaves, afs::kRanks, afs::kCand, afs::kPiece, afs::kExpBins, afs::kDigBits, afs::kDigBins, afs::key_of;
constexpr uint32_t kTilePieces = 16;   // numpy pieces per workgroup of the streaming passes (131 072 latencies)
constexpr uint32_t kSkip = 0xFFFFFFFFu;   // group id of a scenario left out

struct PoolGroup {   // host: off .. n_tiles; the select kernels the rest
    uint64_t off;          // first latency in the compacted array
    uint32_t n;            // latencies
    uint32_t piece0;       // first piece (index into the per-piece sums)
    uint32_t n_pieces;
    uint32_t tile0, n_tiles;
    uint32_t more;         // a wanted rank still has > kCand candidates: another digit pass
    int32_t shift;         // key bits below the known prefixes
    uint32_t n_slots;      // distinct prefixes
    double mean, vmin, vmax;
    double tfrac[2];
    uint64_t pfx[kRanks];       // key >> shift of the bin holding rank r
    uint64_t slot_pfx[kRanks];
    uint32_t want[kRanks], rank_in[kRanks], cnt[kRanks], slot_of[kRanks];
};

struct PoolTile {
    uint32_t group, piece, n_pieces, pad;   // pieces [piece, piece + n_pieces) of the group
};

struct PoolArgs {
    const double* clock;     // [n][clock_cap][2]
    const uint32_t* counts;  // [n][8]
    uint32_t clock_cap, cnt_completed_slot;
    const uint32_t* group;   // [n] or null (all in group 0)
    const uint64_t* dst;     // [n] first compacted slot of the scenario's latencies
    double* lat;             // compacted latencies
    PoolGroup* groups;
    const PoolTile* tiles;
    double* piece_sum;       // [pieces]: pass 1 the latencies' sums, last pass the squared deviations'
    double* tile_min;        // [tiles]
    double* tile_max;
    uint32_t* hist0;         // [G][kExpBins]
    uint32_t* dhist;         // [G][kRanks][kDigBins]
    uint32_t* cand_n;        // [G][kRanks]
    double* cand;            // [G][kRanks][kCand]
    uint32_t* any_more;      // [1]
    double* stats;           // [G][8]
    const uint32_t* stat_row;   // null, or group g's statistics go to row stat_row[g] of stats (af_windowed.hpp: the large cells)
};

__device__ __forceinline__ double readlane_f64(double v, int l) {
    const long long b = __double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)b, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(b >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// 0.0 + v[0] + v[1] + ... one after the other (numpy adds its pieces' sums so), by one wave; every lane returns the sum
__device__ inline double sum_in_order(const double* v, uint32_t n) {
    const int lane = threadIdx.x & 63;
    double tot = 0.0;
    for (uint32_t b = 0; b < n; b += 64u) {
        const double x = b + (uint32_t)lane < n ? v[b + (uint32_t)lane] : 0.0;
        const uint32_t k = n - b < 64u ? n - b : 64u;
#pragma unroll
        for (int t = 0; t < 64; ++t) {
            const double y = readlane_f64(x, t);
            if ((uint32_t)t < k) tot = tot + y;
        }
    }
    return tot;
}

// finish - start of every stored row of scenario blockIdx.x to its place in the compacted array
__global__ __launch_bounds__(kThreads) void af_pool_compact(PoolArgs a) {
    const uint32_t s = blockIdx.x;
    if (a.group && a.group[s] == kSkip) return;
    uint32_t m = a.counts[(size_t)s * 8u + a.cnt_completed_slot];
    if (m > a.clock_cap) m = a.clock_cap;
    const double2* ck = reinterpret_cast<const double2*>(a.clock) + (size_t)s * a.clock_cap;
    double* d = a.lat + a.dst[s];
    constexpr uint32_t kU = 4;
    for (uint32_t i0 = threadIdx.x; i0 < m; i0 += kU * kThreads) {
        double2 c[kU];
#pragma unroll
        for (uint32_t u = 0; u < kU; ++u) c[u] = i0 + u * kThreads < m ? ck[i0 + u * kThreads] : double2{};
#pragma unroll
        for (uint32_t u = 0; u < kU; ++u)
            if (i0 + u * kThreads < m) d[i0 + u * kThreads] = c[u].y - c[u].x;
    }
}

__device__ inline void tile_range(const PoolArgs& a, PoolTile& t, const PoolGroup*& g) {
    t = a.tiles[blockIdx.x];
    g = a.groups + t.group;
}

// the latencies of a tile of a sample of n: [piece * kPiece, min((piece + n_pieces) * kPiece, n))
__device__ __forceinline__ uint32_t tile_len(const PoolTile& t, uint32_t n) {
    const uint64_t lo = (uint64_t)t.piece * kPiece;
    const uint64_t hi_end = (uint64_t)(t.piece + t.n_pieces) * kPiece;
    return (uint32_t)((hi_end < n ? hi_end : (uint64_t)n) - lo);
}

// pass 1: piece sums, min / max, exponent histogram
__global__ __launch_bounds__(kThreads) void af_pool_pass1(PoolArgs a) {
    __shared__ uint32_t hist[kExpBins];
    __shared__ double wsum[2 * kWaves];
    __shared__ double slots[afs::kTailSlots];
    __shared__ double red[2][kWaves];
    const int tid = threadIdx.x;
    PoolTile t;
    const PoolGroup* g;
    tile_range(a, t, g);
    for (int i = tid; i < kExpBins; i += kThreads) hist[i] = 0u;
    __syncthreads();
    const uint32_t n = g->n;
    const double* src = a.lat + g->off;
    double mn = __builtin_inf(), mx = -__builtin_inf();
    for (uint32_t p = 0; p < t.n_pieces; ++p) {
        const uint64_t k = (uint64_t)t.piece + p;
        const uint64_t rest = (uint64_t)n - k * kPiece;
        const uint32_t len = rest < kPiece ? (uint32_t)rest : kPiece;
        const double s = afs::numpy_sum<8>(src + k * kPiece, len, wsum, slots, [&](const double x, const bool act) -> double {
            if (act) {
                mn = fmin(mn, x);
                mx = fmax(mx, x);
            }
            afs::wave_agg_add(hist, (uint32_t)(key_of(x) >> 52) & (kExpBins - 1), act);
            return x;
        });
        if (tid == 0) a.piece_sum[g->piece0 + k] = s;
        __syncthreads();   // (numpy_sum's wave buffers are the next piece's)
    }
    for (int i = tid; i < kExpBins; i += kThreads)
        if (hist[i]) atomicAdd(&a.hist0[(size_t)t.group * kExpBins + i], hist[i]);
    double vmin, vmax;
    afs::block_min_max(mn, mx, red, vmin, vmax);
    if (tid == 0) {
        a.tile_min[blockIdx.x] = vmin;
        a.tile_max[blockIdx.x] = vmax;
    }
}

// the next key bits of every element under one of its group's prefixes
__global__ __launch_bounds__(kThreads) void af_pool_digits(PoolArgs a) {
    __shared__ uint32_t dig[kRanks * kDigBins];
    const int tid = threadIdx.x;
    PoolTile t;
    const PoolGroup* g;
    tile_range(a, t, g);
    if (!g->more) return;
    const uint32_t ns = g->n_slots;
    const int shift = g->shift;
    const int bits = shift >= kDigBits ? kDigBits : shift;
    const int new_shift = shift - bits;
    uint64_t sp[kRanks];
    afs::load_slot_prefixes(sp, g->slot_pfx, ns);
    for (uint32_t i = tid; i < ns * (uint32_t)kDigBins; i += kThreads) dig[i] = 0u;
    __syncthreads();
    const uint32_t len = tile_len(t, g->n);
    const double* src = a.lat + g->off + (uint64_t)t.piece * kPiece;
    constexpr uint32_t kU = 4;
    for (uint32_t i0 = tid; i0 < len; i0 += kU * kThreads) {
        double x[kU];
#pragma unroll
        for (uint32_t u = 0; u < kU; ++u) x[u] = i0 + u * kThreads < len ? src[i0 + u * kThreads] : 0.0;
#pragma unroll
        for (uint32_t u = 0; u < kU; ++u)
            if (i0 + u * kThreads < len) afs::count_digit(key_of(x[u]), shift, new_shift, bits, sp, dig);
    }
    __syncthreads();
    uint32_t* gd = a.dhist + (size_t)t.group * kRanks * kDigBins;
    for (uint32_t i = tid; i < ns * (uint32_t)kDigBins; i += kThreads)
        if (dig[i]) atomicAdd(&gd[i], dig[i]);
}

// One workgroup, one step of the select of the sample whose state is *g: level 0 (the wanted ranks in want[], LDS, filled by
// the caller; hist0 the sample's exponent histogram) or a digit level (dhist: the digit histograms of g's slots)
__device__ __forceinline__ void select_step(PoolGroup* g, const uint32_t* want, const uint32_t* hist0, const uint32_t* dhist, int level,
                                            uint32_t* any_more) {
    __shared__ uint64_t pfx[kRanks];
    __shared__ uint32_t rank_in[kRanks], cnt[kRanks], slot_of[kRanks];
    __shared__ int shift_s;
    const int tid = threadIdx.x;
    if (level == 0) {
        if (tid == 0) shift_s = 52;
        __syncthreads();
        afs::select_first_level(hist0, want, pfx, rank_in, cnt);
    } else {
        if (!g->more) return;
        if (tid < kRanks) {
            pfx[tid] = g->pfx[tid];
            rank_in[tid] = g->rank_in[tid];
            slot_of[tid] = g->slot_of[tid];
        }
        if (tid == 0) shift_s = g->shift;
        __syncthreads();
        const int shift = shift_s;
        const int bits = shift >= kDigBits ? kDigBits : shift;
        afs::select_digit_level(dhist, bits, slot_of, pfx, rank_in, cnt);
        __syncthreads();
        if (tid == 0) shift_s = shift - bits;
    }
    __syncthreads();
    if (tid == 0) {
        const int shift = shift_s;
        uint32_t ns, more;
        afs::assign_slots(pfx, cnt, shift, g->slot_pfx, g->slot_of, &ns, &more);
        for (int r = 0; r < kRanks; ++r) {
            g->pfx[r] = pfx[r];
            g->rank_in[r] = rank_in[r];
            g->cnt[r] = cnt[r];
        }
        g->n_slots = ns;
        g->shift = shift;
        g->more = more;
        if (more) atomicOr(any_more, 1u);
    }
}

// one workgroup per group: level 0 (after pass 1: also the mean, min and max) or a digit level (after af_pool_digits)
__global__ __launch_bounds__(kThreads) void af_pool_select(PoolArgs a, int level) {
    __shared__ uint32_t want[kRanks];
    __shared__ double red[2][kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t gi = blockIdx.x;
    PoolGroup* g = a.groups + gi;
    const uint32_t n = g->n;
    if (level == 0) {
        if (n == 0u) {
            afs::write_empty_row(a.stats + (size_t)(a.stat_row ? a.stat_row[gi] : gi) * 8u, tid);
            if (tid == 0) g->more = 0u;
            return;
        }
        if (tid == 0) afs::stat_ranks(n, want, g->tfrac);
        if (wave == 0) {
            const double tot = sum_in_order(a.piece_sum + g->piece0, g->n_pieces);
            if (lane == 0) g->mean = tot / (double)n;
        }
        double mn = __builtin_inf(), mx = -__builtin_inf();
        for (uint32_t i = tid; i < g->n_tiles; i += kThreads) {
            mn = fmin(mn, a.tile_min[g->tile0 + i]);
            mx = fmax(mx, a.tile_max[g->tile0 + i]);
        }
        double vmin, vmax;
        afs::block_min_max(mn, mx, red, vmin, vmax);
        if (tid == 0) {
            g->vmin = vmin;
            g->vmax = vmax;
        }
    }
    select_step(g, want, a.hist0 + (size_t)gi * kExpBins, a.dhist + (size_t)gi * kRanks * kDigBins, level, a.any_more);
}

// last pass: squared deviations about the group's mean in numpy's order, the candidates on the way
__global__ __launch_bounds__(kThreads) void af_pool_last(PoolArgs a) {
    __shared__ double wsum[2 * kWaves];
    __shared__ double slots[afs::kTailSlots];
    const int tid = threadIdx.x;
    PoolTile t;
    const PoolGroup* g;
    tile_range(a, t, g);
    const uint32_t n = g->n;
    const double mean = g->mean;
    const int shift = g->shift;
    const uint32_t ns = g->n_slots;
    uint64_t sp[kRanks];
    afs::load_slot_prefixes(sp, g->slot_pfx, ns);
    uint32_t* cn = a.cand_n + (size_t)t.group * kRanks;
    double* cd = a.cand + (size_t)t.group * kRanks * kCand;
    const double* src = a.lat + g->off;
    for (uint32_t p = 0; p < t.n_pieces; ++p) {
        const uint64_t k = (uint64_t)t.piece + p;
        const uint64_t rest = (uint64_t)n - k * kPiece;
        const uint32_t len = rest < kPiece ? (uint32_t)rest : kPiece;
        const double s = afs::numpy_sum<8>(src + k * kPiece, len, wsum, slots, [&](const double x, const bool act) -> double {
            const double d = x - mean;
            if (act && shift > 0) afs::collect_candidate(x, shift, sp, cn, cd);
            return d * d;
        });
        if (tid == 0) a.piece_sum[g->piece0 + k] = s;
        __syncthreads();
    }
}

// called by the whole workgroup: the candidates of group gi's slots (af_pool_last's, af_q_cand's) into LDS, cand: [kRanks][kCand]
__device__ __forceinline__ void load_candidates(const PoolArgs& a, uint32_t gi, const PoolGroup* g, double* cand) {
    const uint32_t tid = threadIdx.x;
    if (g->shift > 0)
        for (uint32_t q = 0; q < g->n_slots; ++q) {
            const uint32_t c = a.cand_n[(size_t)gi * kRanks + q];
            const uint32_t m = c < (uint32_t)kCand ? c : (uint32_t)kCand;
            if (tid < m) cand[q * kCand + tid] = a.cand[((size_t)gi * kRanks + q) * kCand + tid];
        }
    __syncthreads();
}

// one workgroup per group: std_dev, the ranks' values, the stats row
__global__ __launch_bounds__(kThreads) void af_pool_final(PoolArgs a) {
    __shared__ double cand[kRanks * kCand];
    __shared__ double val[kRanks];
    __shared__ double sq;
    const int tid = threadIdx.x, wave = tid >> 6;
    const uint32_t gi = blockIdx.x;
    const PoolGroup* g = a.groups + gi;
    const uint32_t n = g->n;
    if (n == 0u) return;   // (written by the level-0 select)
    if (wave == 0) {
        const double tot = sum_in_order(a.piece_sum + g->piece0, g->n_pieces);
        if (tid == 0) sq = tot;
    }
    load_candidates(a, gi, g, cand);
    afs::rank_values(cand, a.cand_n + (size_t)gi * kRanks, g->slot_of, g->rank_in, g->pfx, g->shift, val);
    __syncthreads();
    if (tid == 0)
        afs::write_stats_row(a.stats + (size_t)(a.stat_row ? a.stat_row[gi] : gi) * 8u, n, g->mean, sq, val, g->tfrac, g->vmin, g->vmax);
}

}  // namespace afp
