// Joint second moments of PAIRS of the sampled series per (group, window of ticks, pair): covariance, correlation, lagged
// cross-correlation and the autocorrelation function of a series are closed forms of six exact integer sums
// (af_engine_summarize_series_joint).
// A pair p is (a, b, lag): two integer series (no ram_in_use column) and a lag in ticks.  The cells are af_series_windows.hpp's:
// window w of scenario s is its sample rows [r0, r1) = [min(b[w], m_s), min(b[w + 1], m_s)), m_s = min(counts[s][ticks],
// tick_cap).  The sample of the pair in that window is (x, y) = (word a of row k, word b of row k + lag), k in [r0, r1 - lag):
// both rows inside the same window of the same scenario.  Per cell and pair, over the members of the group:
//   n = sum 1, sx = sum x, sy = sum y (u64), sxx = sum x * x, syy = sum y * y, sxy = sum x * y (128 bits: a u64 low word, the
//   sum mod 2^64, and the carries out of it; a cell holds < 2^32 samples of products < 2^64, so the carries stay below 2^32).
// Rows at or past m_s and the padding words of a row are never used; rows at or past m_s are never loaded.
//   partial   a WAVE per (scenario, run of consecutive windows), one window at a time, 64 rows a step.  A LANE PER (PAIR, SLICE OF
//             THE ROWS): with the pairs rounded up to a power of two p2, lane = slice * p2 + pair, and the 64 / p2 slices take
//             the rows of a step in turn (slice i the rows r + i, r + i + 64 / p2, ...).  One pair is a lane per row; 64 pairs
//             are a lane per pair that walks the 64 rows of the step.  Either way every row is loaded ONCE a call whatever the
//             number of pairs, and a lane keeps ONE pair's sums in registers: sx, sy (64 bits each) and for each of the three
//             products a 64-bit low word and a 32-bit carry count -- 13 VGPRs; n is the closed form max(rows - lag, 0) and needs
//             no register.
//             STAGED FORM (rows of at most kMaxStagedPitch words, 16-byte aligned samples): the rows of a step and the `lag_lds`
//             rows after them are kept in a ring of `ring` rows (a power of two >= 64 + lag_lds) in the wave's own LDS.  A step
//             loads only the rows the ring does not hold yet -- 64 new rows but for the first step -- with 16-byte loads of
//             CONSECUTIVE lanes over the contiguous stretch of memory the rows are (chunk c = lane, lane + 64, ... of the
//             stretch; its row and 16-byte group follow from one division a wave and additions), and stores the four words at
//             row stride pitch + 1 (odd: the lanes' reads of one column fall into 64 different banks).  x is read from the
//             ring; y too when lag <= lag_lds, else from global memory with a 4-byte load at row k + lag.
//             GLOBAL FORM (wider rows): both words with 4-byte loads from the lane's own rows, as af_series_combined.hpp does.
//             The slices of a pair meet by integer shuffles down 32, 16, ... p2; lane p < P writes pair p: the outputs when
//             every group is a single scenario, else one record per (scenario, window, pair) into scratch.
//   fold      a thread per (group, window, pair) adds its members' records in ascending scenario index (integer + only; any
//             order gives the same words) and writes the cell; after a direct pass only the cells of groups without a member.
// No floating point anywhere; no atomics.  Every output word is a function of the data alone.
// LDS: ring * (pitch + 1) words a wave, at most kWaveLdsWords = 4 096 words = 16 KiB a wave, 64 KiB a block.
// Scratch (engine-owned, shared with the other analyzers): 4 B per edge + 16 B per pair + 4 B per group + 4 B per scenario (+ up
// to 256 B of alignment for each of the six parts), and -- unless every group is a single scenario -- 52 B per (scenario,
// window, pair): five 64-bit words (sx, sy, the low words of sxx, syy, sxy) and three 32-bit carry counts.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace afsj {

constexpr int kThreads = 256;               // the partial kernel: four waves, four work items
constexpr int kWaves = kThreads / 64;
constexpr int kFoldThreads = 256;
constexpr uint32_t kSkip = 0xFFFFFFFFu;     // AF_POOL_SKIP
constexpr uint32_t kMaxPairs = 64;          // AF_MAX_SERIES_PAIRS
constexpr uint32_t kWaveLdsWords = 4096;    // the ring of one wave, in words
constexpr uint32_t kMaxStagedPitch = kWaveLdsWords / 64u - 1u - (kWaveLdsWords / 64u - 1u) % 4u;   // 60: 64 rows of pitch + 1 words fit

struct Pair {
    uint32_t a, b, lag, pad;
};
static_assert(sizeof(Pair) == 16, "the scratch bound counts 16 bytes a pair");

struct SjArgs {
    const uint32_t* samples;   // [n][tick_cap][pitch]
    const uint32_t* counts;    // [n][8]
    uint32_t tick_cap, pitch, cnt_ticks_slot;
    const uint32_t* group;     // [n] or null (all in group 0)
    uint32_t n_scen, n_groups, n_win;
    uint32_t run;              // windows per work item of the partial kernel
    uint32_t direct;           // every group is one scenario or none: the partial kernel writes the cells
    const uint32_t* edges;     // [W + 1]
    uint32_t n_pairs;
    uint32_t p2_log;           // the pairs rounded up to a power of two, 2^p2_log <= 64: lane = slice * 2^p2_log + pair
    const Pair* pairs;         // [n_pairs]
    uint32_t staged;           // the staged form; else the global form
    uint32_t ring;             // rows of a wave's ring, a power of two >= 64 + lag_lds
    uint32_t lag_lds;          // pairs with lag <= lag_lds read their second word from the ring
    uint32_t p4, q64, r64;     // pitch / 4, 64 / p4, 64 % p4
    const uint32_t* mem_off;   // [G + 1] into members
    const uint32_t* members;   // the scenarios of group 0, of group 1, ... each ascending
    unsigned long long* rec64; // [n][W][n_pairs][5]: sx, sy, low words of sxx, syy, sxy
    uint32_t* rec32;           // [n][W][n_pairs][3]: carries of sxx, syy, sxy
    uint32_t* n;               // [G][W][P]
    unsigned long long *sx, *sy;          // [G][W][P], or null
    unsigned long long *sxx, *syy, *sxy;  // [G][W][P][2], sxx and syy or null
};

__device__ __forceinline__ uint32_t stored_ticks(const SjArgs& a, uint32_t s) {
    const uint32_t m = a.counts[(size_t)s * 8u + a.cnt_ticks_slot];
    return m < a.tick_cap ? m : a.tick_cap;
}

// a 128-bit sum of 64-bit terms: the sum mod 2^64 and the carries out of it
struct Wide {
    unsigned long long lo = 0ull;
    uint32_t hi = 0u;
    __device__ __forceinline__ void add(unsigned long long v, uint32_t carries = 0u) {
        lo += v;
        hi += carries + (lo < v ? 1u : 0u);
    }
};

// what a lane keeps of one pair over its rows of a window
struct Acc {
    unsigned long long sx = 0ull, sy = 0ull;
    Wide xx, yy, xy;
    __device__ __forceinline__ void add(uint32_t x, uint32_t y) {   // (a row that is not live adds x = y = 0)
        sx += x;
        sy += y;
        xx.add((unsigned long long)x * x);
        yy.add((unsigned long long)y * y);
        xy.add((unsigned long long)x * y);
    }
    // the partner `dist` lanes up
    __device__ __forceinline__ void fold(int dist, bool take) {
        const unsigned long long osx = __shfl_down(sx, dist, 64), osy = __shfl_down(sy, dist, 64);
        const unsigned long long oxx = __shfl_down(xx.lo, dist, 64), oyy = __shfl_down(yy.lo, dist, 64), oxy = __shfl_down(xy.lo, dist, 64);
        const uint32_t hxx = __shfl_down(xx.hi, dist, 64), hyy = __shfl_down(yy.hi, dist, 64), hxy = __shfl_down(xy.hi, dist, 64);
        if (take) {
            sx += osx;
            sy += osy;
            xx.add(oxx, hxx);
            yy.add(oyy, hyy);
            xy.add(oxy, hxy);
        }
    }
};

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the samples of a pair in a window of `rows` rows
__device__ __forceinline__ uint32_t pair_count(uint32_t rows, uint32_t lag) { return rows > lag ? rows - lag : 0u; }

__global__ __launch_bounds__(kThreads) void af_sjoint_partial(SjArgs a) {
    extern __shared__ uint32_t afsj_lds[];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t W = a.n_win, P = a.n_pairs, pitch = a.pitch, stride = pitch + 1u, mask = a.ring - 1u;
    const bool staged = a.staged != 0u;
    uint32_t* ring = afsj_lds + (threadIdx.x >> 6) * a.ring * stride;   // this wave's rows (no word in the global form)
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
    // this lane's pair and its slice of the rows of a step: lane = slice * p2 + pair
    const uint32_t p2 = 1u << a.p2_log, n_slices = 64u >> a.p2_log;
    const uint32_t p = lane & (p2 - 1u), slice = lane >> a.p2_log;
    const bool has = p < P;                                              // (p2 - P lanes of a slice have no pair)
    const Pair pr = a.pairs[has ? p : 0u];
    const bool y_staged = staged && pr.lag <= a.lag_lds;
    for (uint32_t w = w0; w < w1; ++w) {
        uint32_t r0 = a.edges[w], r1 = a.edges[w + 1u];
        r0 = r0 < m ? r0 : m;
        r1 = r1 < m ? r1 : m;
        Acc acc;
        uint32_t have = r0;                                              // rows [.., have) of the window have been staged
        for (uint32_t r = r0; r < r1; r += 64u) {                        // (uniform; r1 <= tick_cap < 2^31: no wrap)
            if (staged) {
                uint32_t want = r + 64u + a.lag_lds;                     // (< 2^32: lag_lds < 4 096)
                want = want < r1 ? want : r1;
                wave_sync();                                             // (the rows the last step read are overwritten)
                while (have < want) {                                    // (uniform) a stretch of at most 64 rows
                    const uint32_t cnt = want - have < 64u ? want - have : 64u;
                    uint32_t row = row_first, grp = grp_first;
                    for (uint32_t j = 0; j < a.p4; ++j) {                // 64 * p4 chunks are 64 rows
                        if (row < cnt) {
                            const uint32_t k = have + row;
                            const uint4 v = *reinterpret_cast<const uint4*>(rows + (size_t)k * pitch + 4u * grp);
                            uint32_t* d = ring + ((k - r0) & mask) * stride + 4u * grp;
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
                    have += cnt;
                }
                wave_sync();
            }
            const uint32_t here = r1 - r < 64u ? r1 - r : 64u;           // the rows of this step
            const uint32_t turns = (here + n_slices - 1u) >> (6u - a.p2_log);   // every slice takes a row a turn
            for (uint32_t j = 0; j < turns; j += 4u) {                   // (uniform) four turns' loads in flight
                uint32_t x[4], y[4];
#pragma unroll
                for (uint32_t u = 0; u < 4u; ++u) {
                    x[u] = y[u] = 0u;
                    if (j + u >= turns) break;                           // (uniform)
                    const uint32_t k = r + slice + (j + u) * n_slices;   // (< r + 64: turns <= p2)
                    const uint32_t k2 = k + pr.lag;                      // (both below 2^31: no wrap)
                    if (has && k2 < r1) {                                // (then k < r1 too)
                        x[u] = staged ? ring[((k - r0) & mask) * stride + pr.a] : rows[(size_t)k * pitch + pr.a];
                        y[u] = y_staged ? ring[((k2 - r0) & mask) * stride + pr.b] : rows[(size_t)k2 * pitch + pr.b];
                    }
                }
#pragma unroll
                for (uint32_t u = 0; u < 4u; ++u) {
                    if (j + u >= turns) break;                           // (uniform)
                    acc.add(x[u], y[u]);
                }
            }
        }
        for (uint32_t h = 32u; h >= p2; h >>= 1) acc.fold((int)h, lane < h);   // (uniform) the slices of a pair are p2 lanes apart
        if (lane >= P) continue;                                         // lane p < P holds pair p
        if (a.direct) {
            const size_t o = ((size_t)g * W + w) * P + p;
            a.n[o] = pair_count(r1 - r0, pr.lag);
            if (a.sx) a.sx[o] = acc.sx;
            if (a.sy) a.sy[o] = acc.sy;
            if (a.sxx) a.sxx[2u * o] = acc.xx.lo, a.sxx[2u * o + 1u] = acc.xx.hi;
            if (a.syy) a.syy[2u * o] = acc.yy.lo, a.syy[2u * o + 1u] = acc.yy.hi;
            a.sxy[2u * o] = acc.xy.lo, a.sxy[2u * o + 1u] = acc.xy.hi;
        } else {
            const size_t o = ((size_t)s * W + w) * P + p;
            unsigned long long* r64 = a.rec64 + 5u * o;
            uint32_t* r32 = a.rec32 + 3u * o;
            r64[0] = acc.sx;
            r64[1] = acc.sy;
            r64[2] = acc.xx.lo;
            r64[3] = acc.yy.lo;
            r64[4] = acc.xy.lo;
            r32[0] = acc.xx.hi;
            r32[1] = acc.yy.hi;
            r32[2] = acc.xy.hi;
        }
    }
}

// entries [first, n_entries) of the (group, window, pair) array, a thread each
__global__ __launch_bounds__(kFoldThreads) void af_sjoint_fold(SjArgs a, uint64_t first, uint64_t n_entries) {
    const uint64_t idx = first + (uint64_t)blockIdx.x * kFoldThreads + threadIdx.x;
    if (idx >= n_entries) return;
    const uint32_t P = a.n_pairs, W = a.n_win;
    const uint64_t cell = idx / P;
    const uint32_t p = (uint32_t)(idx % P);
    const uint32_t g = (uint32_t)(cell / W), w = (uint32_t)(cell % W);
    const uint32_t k0 = a.mem_off[g], k1 = a.mem_off[g + 1u];
    if (a.direct && k1 != k0) return;   // its one member's wave wrote the cell
    const uint32_t b0 = a.edges[w], b1 = a.edges[w + 1u], lag = a.pairs[p].lag;
    uint32_t cnt = 0u;
    unsigned long long sx = 0ull, sy = 0ull;
    Wide xx, yy, xy;
    for (uint32_t k = k0; k < k1; ++k) {
        const uint32_t s = a.members[k];
        const uint32_t m = stored_ticks(a, s);
        cnt += pair_count((b1 < m ? b1 : m) - (b0 < m ? b0 : m), lag);
        const size_t o = ((size_t)s * W + w) * P + p;
        const unsigned long long* r64 = a.rec64 + 5u * o;
        const uint32_t* r32 = a.rec32 + 3u * o;
        sx += r64[0];
        sy += r64[1];
        xx.add(r64[2], r32[0]);
        yy.add(r64[3], r32[1]);
        xy.add(r64[4], r32[2]);
    }
    a.n[idx] = cnt;
    if (a.sx) a.sx[idx] = sx;
    if (a.sy) a.sy[idx] = sy;
    if (a.sxx) a.sxx[2u * idx] = xx.lo, a.sxx[2u * idx + 1u] = xx.hi;
    if (a.syy) a.syy[2u * idx] = yy.lo, a.syy[2u * idx + 1u] = yy.hi;
    a.sxy[2u * idx] = xy.lo, a.sxy[2u * idx + 1u] = xy.hi;
}

}  // namespace afsj
