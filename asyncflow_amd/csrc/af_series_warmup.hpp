// Warm-up truncation of the sampled series per (group, window of ticks, column): the MSER rule (White 1997) on the batch means of
// the ensemble over a group's members (Welch), stated in integers (af_engine_summarize_series_warmup).
// The cells are af_series_windows.hpp's: window w of scenario s is its sample rows [r0, r1) = [min(b[w], m_s), min(b[w + 1], m_s)),
// m_s = min(counts[s][ticks], tick_cap).  With B = batch ticks, batch j of a window is its rows [b[w] + j B, b[w] + (j + 1) B); it
// is complete for s when it lies inside [r0, r1).  J is the minimum over the members of the group of their complete batches (0
// for a group without a member); a trailing partial batch is in no cell.  For an INTEGER series (no ram_in_use column)
//   Y_j    = sum over the members and the B rows of batch j of the word as an unsigned 32-bit integer, j < J
//   S1(d)  = sum_{j >= d} Y_j,  S2(d) = sum_{j >= d} Y_j^2,  m = J - d
//   A(d)   = m S2(d) - S1(d)^2 >= 0,  MSER(d) = A(d) / m^3          (B and the member count are constant in d and cancel)
//   d*     = the smallest d in 0 .. D = J / 2 that minimises MSER(d), compared exactly: A(d1) m2^3 < A(d2) m1^3
// WIDTHS.  The entry refuses unless n_scenarios * B <= 2^32 and every window holds fewer than 2^25 batches.  Then
//   Y_j <= n B (2^32 - 1) < 2^64;  J < 2^25;  S1 < 2^25 2^64 = 2^89 (two u64);  S2 < 2^25 2^128 = 2^153 (three u64);
//   m S2 < 2^178, S1^2 < 2^178, so A < 2^178;  m^3 < 2^75;  every compared product A m'^3 < 2^253:
// 256-bit unsigned arithmetic (af_wide.hpp) is exact and no overflow flag is needed.
//   batches   a WAVE per (scenario, run of consecutive windows), 64 rows a step, only the rows of the scenario's complete batches.
//             af_series_joint.hpp's two load forms: STAGED (rows of at most kMaxStagedPitch words, 16-byte aligned samples), the
//             rows of a step in the wave's own LDS through 16-byte loads of consecutive lanes, stored at row stride pitch + 1;
//             GLOBAL (wider rows), 4-byte loads of the words themselves.  Either way a needed row is loaded ONCE a call whatever
//             the number of columns.  The work of a step is its (batch, column) ITEMS -- the batches that overlap the step times
//             the columns --, a lane group of `ns` lanes per item (ns = 64 / items rounded down to a power of two, 1 beyond 32
//             items, the items then taken 64 at a time): lane `sub` of the group adds the rows lo + sub, lo + sub + ns, ... of
//             the item, the group meets by integer shuffles, and its first lane adds the u64 sum into Y[g][c][batch] with ONE
//             64-bit integer atomic add (a zero sum adds nothing).  Y is zeroed first; a batch that straddles steps, and the
//             members of a larger group, meet in those adds.  Integer addition: exact and order-independent.
//             Lane 0 also lowers jmin[g][w] (preset to 2^32 - 1) to the scenario's complete batches with an integer atomic min.
//   cell      a WAVE per (group, window, column) over Y[0 .. J): (1) a lane owns a contiguous stretch of ceil(J / 64) batches and
//             adds its totals of Y and Y^2; (2) the wave forms the suffix sums of the 64 totals by shuffles; (3) a lane walks
//             its stretch again from the back, S1 and S2 running from its suffix, evaluates its candidates d <= D and keeps its
//             best (A, m, d) with the sums at d; (4) the wave reduces by the exact compare, the smaller d winning a tie.  Lane 0
//             writes the cell: d*, the sums at d* (from the lane that owns d*) and at d = 0.
// The lane routines (lane_totals, lane_best, better) are AF_HD and free of HIP: cell_of() runs the same 64 lanes one after the
// other on the host (tests/hostcheck/warmup_check.cpp).
// No floating point anywhere.  Every output word is a function of the data alone.
// LDS: 64 * (pitch + 1) words a wave, at most kWaveLdsWords = 4 096 words = 16 KiB a wave, 64 KiB a block.
// Scratch (engine-owned, shared with the other analyzers), integer ATOMICS into a zeroed buffer, no records: 8 B per (group,
// column, batch) with batch over sum_w floor((min(b[w + 1], cap) - min(b[w], cap)) / B) -- at B = 5 that is 0.4 x the bytes of the
// selected columns of one scenario per GROUP --, 4 B per (group, window), 8 B per edge, 4 B per column (+ up to 256 B of
// alignment for each of the five parts).
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#include <stdint.h>

#include "af_wide.hpp"

namespace afwu {

using afw256::U256;

constexpr uint32_t kNone = 0xFFFFFFFFu;          // no candidate
constexpr uint32_t kMaxWindowBatches = 1u << 25; // a window holds fewer batches than this

// S1 and S2 of a stretch of batches
struct Sums {
    U256 s1, s2;
};

AF_HD Sums no_sums() { return Sums{afw256::zero(), afw256::zero()}; }

AF_HD void add_sums(Sums& a, const Sums& b) {
    a.s1 = afw256::add(a.s1, b.s1);
    a.s2 = afw256::add(a.s2, b.s2);
}

AF_HD void add_batch(Sums& a, uint64_t y) {
    uint64_t hi;
    const uint64_t lo = afw256::mul64(y, y, hi);
    a.s1 = afw256::add_u64(a.s1, y);
    a.s2 = afw256::add(a.s2, afw256::from_u128(lo, hi));
}

// a candidate: A(d), m = J - d, d and the sums at d
struct Best {
    U256 a;
    Sums at;
    uint32_t m, d;
};

AF_HD Best no_best() { return Best{afw256::zero(), no_sums(), 0u, kNone}; }

// m^3 for m < 2^25 as (low, high) words
AF_HD uint64_t cube(uint32_t m, uint64_t& hi) { return afw256::mul64((uint64_t)m * m, (uint64_t)m, hi); }

// does candidate 1 beat candidate 2: MSER(d1) < MSER(d2) by A1 m2^3 < A2 m1^3, or equal and d1 < d2
AF_HD bool better(const U256& a1, uint32_t m1, uint32_t d1, const U256& a2, uint32_t m2, uint32_t d2) {
    if (d1 == kNone) return false;
    if (d2 == kNone) return true;
    uint64_t h1, h2;
    const uint64_t l1 = cube(m1, h1), l2 = cube(m2, h2);
    const int c = afw256::cmp(afw256::mul_u128(a1, l2, h2), afw256::mul_u128(a2, l1, h1));
    return c < 0 || (c == 0 && d1 < d2);
}

// A = m S2 - S1^2 (S1 < 2^128: its two low limbs are all of it)
AF_HD U256 spread(const Sums& s, uint32_t m) {
    return afw256::sub(afw256::mul_u64(s.s2, (uint64_t)m), afw256::mul_u128(s.s1, s.s1.w[0], s.s1.w[1]));
}

// the stretch [j0, j1) of lane `lane` of 64 over J batches
AF_HD void lane_stretch(uint32_t lane, uint32_t J, uint32_t& j0, uint32_t& j1) {
    const uint32_t len = (J + 63u) / 64u;      // (J < 2^25: lane * len < 2^32)
    j0 = lane * len < J ? lane * len : J;
    j1 = J - j0 < len ? J : j0 + len;
}

// step 1: the totals of a stretch
AF_HD Sums lane_totals(const uint64_t* y, uint32_t j0, uint32_t j1) {
    Sums t = no_sums();
    for (uint32_t j = j0; j < j1; ++j) add_batch(t, y[j]);
    return t;
}

// step 3: the best candidate d <= J / 2 of a stretch, `after` the sums of the batches at and past j1
AF_HD Best lane_best(const uint64_t* y, uint32_t j0, uint32_t j1, const Sums& after, uint32_t J) {
    Best best = no_best();
    const uint32_t D = J / 2u;
    if (j0 > D || j0 >= j1) return best;       // no candidate here
    Sums run = after;
    for (uint32_t j = j1; j-- > j0;) {
        add_batch(run, y[j]);
        if (j > D) continue;
        const uint32_t m = J - j;
        const U256 a = spread(run, m);
        if (better(a, m, j, best.a, best.m, best.d)) best = Best{a, run, m, j};
    }
    return best;
}

// what a cell's wave writes
struct Cell {
    uint32_t trunc;
    Sums at, all;   // the sums at d* and at d = 0
};

// the cell as its wave computes it, the 64 lanes one after the other
AF_HD Cell cell_of(const uint64_t* y, uint32_t J) {
    Cell out{0u, no_sums(), no_sums()};
    if (J == 0u) return out;
    Sums after[65];
    after[64] = no_sums();
    for (uint32_t lane = 64u; lane-- > 0u;) {  // step 2: after[lane] = the totals of the lanes above
        uint32_t j0, j1;
        lane_stretch(lane, J, j0, j1);
        after[lane] = after[lane + 1u];
        add_sums(after[lane], lane_totals(y, j0, j1));
    }
    out.all = after[0];
    Best best = no_best();
    for (uint32_t lane = 0; lane < 64u; ++lane) {
        uint32_t j0, j1;
        lane_stretch(lane, J, j0, j1);
        const Best b = lane_best(y, j0, j1, after[lane + 1u], J);
        if (better(b.a, b.m, b.d, best.a, best.m, best.d)) best = b;
    }
    out.trunc = best.d;
    out.at = best.at;
    return out;
}

#if defined(__HIPCC__)

constexpr int kThreads = 256;               // both kernels: four waves, four work items
constexpr int kWaves = kThreads / 64;
constexpr uint32_t kSkip = 0xFFFFFFFFu;     // AF_POOL_SKIP
constexpr uint32_t kMaxColumns = 64;        // AF_MAX_SERIES_WARMUP_COLUMNS
constexpr uint32_t kWaveLdsWords = 4096;    // the rows of one wave's step, in words
constexpr uint32_t kMaxStagedPitch = kWaveLdsWords / 64u - 1u - (kWaveLdsWords / 64u - 1u) % 4u;   // 60: 64 rows of pitch + 1 words fit

struct SwArgs {
    const uint32_t* samples;   // [n][tick_cap][pitch]
    const uint32_t* counts;    // [n][8]
    uint32_t tick_cap, pitch, cnt_ticks_slot;
    const uint32_t* group;     // [n] or null (all in group 0)
    uint32_t n_scen, n_groups, n_win;
    uint32_t run;              // windows per work item of the batches kernel
    const uint32_t* edges;     // [W + 1]
    const uint32_t* boff;      // [W + 1] the first batch of window w in a (group, column)'s sequence; boff[W] = n_batches
    uint32_t n_batches;        // batches of all windows
    uint32_t batch;            // B
    uint32_t n_cols;
    const uint32_t* cols;      // [n_cols]
    uint32_t staged;           // the staged form; else the global form
    uint32_t p4, q64, r64;     // pitch / 4, 64 / p4, 64 % p4
    uint64_t* y;               // [G][n_cols][n_batches], zeroed
    uint32_t* jmin;            // [G][W], preset to kNone
    uint32_t* batches;         // [G][W]
    uint32_t* trunc;           // [G][W][C]
    uint64_t *s1, *s1_all;     // [G][W][C][2], or null
    uint64_t *s2, *s2_all;     // [G][W][C][3], or null
};

__device__ __forceinline__ uint32_t stored_ticks(const SwArgs& a, uint32_t s) {
    const uint32_t m = a.counts[(size_t)s * 8u + a.cnt_ticks_slot];
    return m < a.tick_cap ? m : a.tick_cap;
}

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(kThreads) void af_swarm_batches(SwArgs a) {
    extern __shared__ uint32_t afwu_lds[];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t W = a.n_win, C = a.n_cols, B = a.batch, pitch = a.pitch, stride = pitch + 1u;
    const bool staged = a.staged != 0u;
    uint32_t* ring = afwu_lds + (threadIdx.x >> 6) * 64u * stride;      // this wave's rows (no word in the global form)
    const uint32_t runs = (W + a.run - 1u) / a.run;                      // work items per scenario
    const uint64_t item = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (item >= (uint64_t)a.n_scen * runs) return;                       // (a whole wave; there is no block-wide barrier below)
    const uint32_t s = (uint32_t)(item / runs), w0 = (uint32_t)(item % runs) * a.run;
    const uint32_t w1 = W - w0 < a.run ? W : w0 + a.run;
    const uint32_t g = a.group ? a.group[s] : 0u;
    if (g == kSkip || g >= a.n_groups) return;
    const uint32_t m = stored_ticks(a, s);
    const uint32_t* rows = a.samples + (size_t)s * a.tick_cap * pitch;
    // chunk `lane` of a stretch of rows: its row and its 16-byte group; chunk lane + 64 j follows by additions
    const uint32_t row_first = staged ? lane / a.p4 : 0u, grp_first = staged ? lane % a.p4 : 0u;
    for (uint32_t w = w0; w < w1; ++w) {
        uint32_t r0 = a.edges[w], r1 = a.edges[w + 1u];
        r0 = r0 < m ? r0 : m;
        r1 = r1 < m ? r1 : m;
        const uint32_t nb = (r1 - r0) / B;                               // this member's complete batches (r0 = b[w] unless none)
        if (lane == 0u) atomicMin(a.jmin + (size_t)g * W + w, nb);
        const uint32_t rend = r0 + nb * B;                               // (<= r1) the rows past it are in no batch
        uint64_t* yw = a.y + (size_t)g * C * a.n_batches + a.boff[w];
        for (uint32_t r = r0; r < rend; r += 64u) {                      // (uniform; rend <= tick_cap < 2^31: no wrap)
            const uint32_t here = rend - r < 64u ? rend - r : 64u;       // the rows of this step
            if (staged) {
                wave_sync();                                             // (the rows the last step read are overwritten)
                uint32_t row = row_first, grp = grp_first;
                for (uint32_t j = 0; j < a.p4; ++j) {                    // 64 * p4 chunks are 64 rows
                    if (row < here) {
                        const uint4 v = *reinterpret_cast<const uint4*>(rows + (size_t)(r + row) * pitch + 4u * grp);
                        uint32_t* d = ring + row * stride + 4u * grp;
                        d[0] = v.x;
                        d[1] = v.y;
                        d[2] = v.z;
                        d[3] = v.w;
                    }
                    row += a.q64;
                    grp += a.r64;
                    if (grp >= a.p4) {
                        grp -= a.p4;
                        row += 1u;
                    }
                }
                wave_sync();
            }
            const uint32_t jb0 = (r - r0) / B, jb1 = (r + here - 1u - r0) / B;   // the batches that overlap the step
            const uint32_t items = (jb1 - jb0 + 1u) * C;                 // (<= 64 * 64)
            uint32_t ns_log = 0u;                                        // lanes per item: 2^ns_log
            while (ns_log < 6u && (items << (ns_log + 1u)) <= 64u) ns_log += 1u;
            const uint32_t ns = 1u << ns_log, sub = lane & (ns - 1u), per_turn = 64u >> ns_log;
            for (uint32_t it0 = 0; it0 < items; it0 += per_turn) {       // (uniform)
                const uint32_t it = it0 + (lane >> ns_log);
                const bool has = it < items;
                const uint32_t c = has ? it % C : 0u, jb = jb0 + (has ? it / C : 0u);
                const uint32_t col = a.cols[c];
                uint32_t lo = r0 + jb * B, hi = lo + B;                  // (<= rend: no wrap)
                lo = lo > r ? lo : r;
                hi = hi < r + here ? hi : r + here;
                unsigned long long sum = 0ull;
                if (has)
                    for (uint32_t k = lo + sub; k < hi; k += ns) sum += staged ? ring[(k - r) * stride + col] : rows[(size_t)k * pitch + col];
                for (uint32_t h = ns >> 1; h >= 1u; h >>= 1) sum += __shfl_xor(sum, (int)h, 64);   // (uniform)
                if (has && sub == 0u && sum != 0ull)
                    __hip_atomic_fetch_add(yw + (size_t)c * a.n_batches + jb, (uint64_t)sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

__device__ __forceinline__ uint64_t shfl_down64(uint64_t v, int dist) { return (uint64_t)__shfl_down((unsigned long long)v, dist, 64); }
__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int dist) { return (uint64_t)__shfl_xor((unsigned long long)v, dist, 64); }
__device__ __forceinline__ uint64_t shfl_from64(uint64_t v, int lane) { return (uint64_t)__shfl((unsigned long long)v, lane, 64); }

// the sums of the lane `dist` up: S1 in two limbs, S2 in three (the width contract)
__device__ __forceinline__ Sums sums_down(const Sums& s, int dist) {
    Sums o = no_sums();
    o.s1.w[0] = shfl_down64(s.s1.w[0], dist);
    o.s1.w[1] = shfl_down64(s.s1.w[1], dist);
    o.s2.w[0] = shfl_down64(s.s2.w[0], dist);
    o.s2.w[1] = shfl_down64(s.s2.w[1], dist);
    o.s2.w[2] = shfl_down64(s.s2.w[2], dist);
    return o;
}

// cells [first, n_cells) of the (group, window, column) array, a wave each
__global__ __launch_bounds__(kThreads) void af_swarm_cell(SwArgs a, uint64_t first, uint64_t n_cells) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t idx = first + (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (idx >= n_cells) return;                                          // (a whole wave)
    const uint32_t C = a.n_cols, W = a.n_win;
    const uint64_t gw = idx / C;
    const uint32_t c = (uint32_t)(idx % C), g = (uint32_t)(gw / W), w = (uint32_t)(gw % W);
    uint32_t J = a.jmin[gw];
    J = J == kNone ? 0u : J;                                             // a group without a member
    if (lane == 0u && c == 0u) a.batches[gw] = J;
    Cell cell{0u, no_sums(), no_sums()};
    if (J != 0u) {                                                       // (uniform)
        const uint64_t* y = a.y + ((size_t)g * C + c) * a.n_batches + a.boff[w];
        uint32_t j0, j1;
        lane_stretch(lane, J, j0, j1);
        Sums inc = lane_totals(y, j0, j1);                               // step 1
        for (uint32_t h = 1u; h < 64u; h <<= 1) {                        // step 2: this lane's and the higher lanes' totals
            const Sums o = sums_down(inc, (int)h);
            if (lane + h < 64u) add_sums(inc, o);
        }
        Sums after = sums_down(inc, 1);
        if (lane == 63u) after = no_sums();
        Best best = lane_best(y, j0, j1, after, J);                      // step 3
        U256 ba = best.a;
        uint32_t bm = best.m, bd = best.d;
        for (uint32_t h = 32u; h >= 1u; h >>= 1) {                       // step 4: A < 2^178 is three limbs
            U256 oa = afw256::zero();
            oa.w[0] = shfl_xor64(ba.w[0], (int)h);
            oa.w[1] = shfl_xor64(ba.w[1], (int)h);
            oa.w[2] = shfl_xor64(ba.w[2], (int)h);
            const uint32_t om = __shfl_xor(bm, (int)h, 64), od = __shfl_xor(bd, (int)h, 64);
            if (better(oa, om, od, ba, bm, bd)) ba = oa, bm = om, bd = od;
        }
        const int owner = (int)(bd / ((J + 63u) / 64u));                 // (uniform) the lane whose stretch holds d*
        cell.trunc = bd;
        cell.at.s1.w[0] = shfl_from64(best.at.s1.w[0], owner);
        cell.at.s1.w[1] = shfl_from64(best.at.s1.w[1], owner);
        cell.at.s2.w[0] = shfl_from64(best.at.s2.w[0], owner);
        cell.at.s2.w[1] = shfl_from64(best.at.s2.w[1], owner);
        cell.at.s2.w[2] = shfl_from64(best.at.s2.w[2], owner);
        cell.all = inc;                                                  // (lane 0's: every batch)
    }
    if (lane != 0u) return;
    a.trunc[idx] = cell.trunc;
    if (a.s1) a.s1[2u * idx] = cell.at.s1.w[0], a.s1[2u * idx + 1u] = cell.at.s1.w[1];
    if (a.s2) a.s2[3u * idx] = cell.at.s2.w[0], a.s2[3u * idx + 1u] = cell.at.s2.w[1], a.s2[3u * idx + 2u] = cell.at.s2.w[2];
    if (a.s1_all) a.s1_all[2u * idx] = cell.all.s1.w[0], a.s1_all[2u * idx + 1u] = cell.all.s1.w[1];
    if (a.s2_all) a.s2_all[3u * idx] = cell.all.s2.w[0], a.s2_all[3u * idx + 1u] = cell.all.s2.w[1], a.s2_all[3u * idx + 2u] = cell.all.s2.w[2];
}

#endif  // __HIPCC__

}  // namespace afwu
