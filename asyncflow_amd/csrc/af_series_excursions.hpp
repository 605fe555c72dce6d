// Excursions of the sampled series above a threshold per (scenario, window of ticks, series): how long a queue stayed high,
// when it first went up, when it had come back, how many separate backlogs formed and when the peak was
// (af_engine_summarize_series_excursions).
// The cells are af_series_windows.hpp's, always per scenario: window w of scenario s is its sample rows [lo, hi) =
// [min(b[w], m_s), min(b[w + 1], m_s)), m_s = min(counts[s][ticks], tick_cap); rows at or past m_s and the padding words of a
// row are never read.  A tick k is ABOVE when (double)value > threshold (the value as af_series_windows.hpp's `above` takes
// it); a RUN is a maximal stretch of consecutive above ticks inside [lo, hi) -- clipped at the window's edges.
//   a WAVE per (scenario, run of consecutive windows), one window at a time, with af_swin_partial's mapping of rows to lanes:
//   pq = pitch / 4 16-byte groups per row, L = min(pq, 64) lanes a row, R = 64 / L rows a STEP; lane l holds group l % L of row
//   base + l / L and then every R-th row below (plans of more than 64 groups: 64 groups per pass over the rows).  EVERY STORED
//   ROW INSIDE THE WINDOWS IS READ ONCE, 16 bytes a lane, consecutive across the lanes, four steps in flight.  Per step:
//     neighbour   whether tick k - 1 was above comes from the lane L below -- for the first row of a step from the last row of
//                 the step before, which that row's lanes kept: ONE shuffle of the four columns' bits serves both.  A RISE is
//                 an above tick whose predecessor in the window is not above.
//     open run    the start of the run a tick belongs to is the latest rise at or before it: an inclusive prefix maximum of
//                 (rise ? k + 1 : 0) over the rows of the step (shuffles up L, 2 L, 4 L, ... lanes), then the maximum with
//                 the CARRY, that value of the step before's last row.  (tick_cap < 2^31: k + 1 fits a word.)  A column
//                 that no lane of the wave holds above in this step is skipped after the neighbour shuffle: no rise, its
//                 carry cannot change.
//     per lane    above = sum of the above ticks, runs = sum of the rises, first / last = min / max of the above k, longest
//                 and its start = max of (length << 32 | ~start), the length at an above tick being k - start + 1 (the
//                 earliest start wins a tie), peak = max of (key << 32 | ~k) over every row (the smallest k wins a tie); the
//                 key is the word, or afs::float_key of a ram_in_use word.
//   The lanes of a column group meet by shuffles down L, 2 L, 4 L, ... lanes and the first L lanes write the cell.
// Every combining operation is an integer +, min or max -- commutative and associative: no atomics, no floating-point
// addition, and the result cannot depend on the launch, the batch a scenario sits in, or the run.
// Scratch (engine-owned, shared with the other analyzers): 4 B per edge + 8 B per series (+ up to 256 B of alignment for each
// of the two parts).  No per-cell records.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "af_summary.hpp"

namespace afsx {

constexpr int kThreads = 256;             // four waves, four work items
constexpr int kWaves = kThreads / 64;
constexpr uint32_t kUnroll = 4;           // 16-byte loads a lane has in flight
constexpr uint32_t kNone = 0xFFFFFFFFu;   // AF_TICK_NONE

struct SexArgs {
    const uint32_t* samples;   // [n][tick_cap][pitch]
    const uint32_t* counts;    // [n][8]
    uint32_t tick_cap, pitch, n_series, n_edges, cnt_ticks_slot;
    uint32_t n_scen, n_win;
    uint32_t run;              // windows per work item
    const uint32_t* edges;     // [W + 1]
    const double* thr;         // [n_series]
    uint32_t* count;           // [n][W], or null
    uint32_t *above, *runs, *longest, *longest_start, *first, *last, *peak_tick;   // [n][W][n_series], or null
};

// what a lane keeps of one column
struct Col {
    uint32_t ab = 0u, ru = 0u;
    uint32_t fi = kNone;                 // the smallest above tick
    uint32_t la = 0u;                    // the largest above tick + 1; 0: none
    unsigned long long lg = 0ull;        // max of (run length so far << 32 | ~start) over the above ticks; 0: none
    unsigned long long pk = 0ull;        // max of (key << 32 | ~k) over the rows; 0: no row (~k >= 2^31 for every row)
    uint32_t carry = 0u;                 // the latest rise of the steps before, + 1; 0: none yet in this window
    // the partner hdist lanes up; `take` where this lane is the left operand of the tree
    __device__ __forceinline__ void fold(int hdist, bool take) {
        const uint32_t oab = __shfl_down(ab, hdist, 64), oru = __shfl_down(ru, hdist, 64);
        const uint32_t ofi = __shfl_down(fi, hdist, 64), ola = __shfl_down(la, hdist, 64);
        const unsigned long long olg = __shfl_down(lg, hdist, 64), opk = __shfl_down(pk, hdist, 64);
        if (take) {
            ab += oab;
            ru += oru;
            fi = ofi < fi ? ofi : fi;
            la = ola > la ? ola : la;
            lg = olg > lg ? olg : lg;
            pk = opk > pk ? opk : pk;
        }
    }
};

__global__ __launch_bounds__(kThreads) void af_sexc_kernel(SexArgs a) {
    const int lane = threadIdx.x & 63;
    const uint32_t W = a.n_win;
    const uint32_t items = (W + a.run - 1u) / a.run;   // work items per scenario
    const uint64_t item = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (item >= (uint64_t)a.n_scen * items) return;    // (a whole wave)
    const uint32_t s = (uint32_t)(item / items), w0 = (uint32_t)(item % items) * a.run;
    const uint32_t w1 = W - w0 < a.run ? W : w0 + a.run;
    uint32_t m = a.counts[(size_t)s * 8u + a.cnt_ticks_slot];
    m = m < a.tick_cap ? m : a.tick_cap;
    const uint32_t pq = a.pitch / 4u;
    const uint32_t L = pq < 64u ? pq : 64u;     // lanes per row
    const uint32_t rps = 64u / L;               // rows per step of the wave
    const uint32_t row_off = (uint32_t)lane / L, cgl = (uint32_t)lane % L;
    const bool lane_on = row_off < rps;
    const bool last_row = row_off == rps - 1u;
    const int top_lane = (int)((rps - 1u) * L + cgl);               // this column group in the last row of a step
    const int below_lane = row_off > 0u ? lane - (int)L : top_lane;   // the lane that holds tick k - 1
    uint32_t p2 = 1u;
    while (p2 < rps) p2 <<= 1;
    const uint4* rows = reinterpret_cast<const uint4*>(a.samples) + (size_t)s * a.tick_cap * pq;
    const uint32_t S = a.n_series;
    for (uint32_t cg0 = 0; cg0 < pq; cg0 += 64u) {
        const uint32_t cg = cg0 + cgl;
        const bool on = lane_on && cg < pq;
        bool is_f[4];
        double thr[4];
#pragma unroll
        for (uint32_t c = 0; c < 4u; ++c) {
            const uint32_t j = cg * 4u + c;
            is_f[c] = afs::series_is_float(j, a.n_edges, S);
            thr[c] = j < S ? a.thr[j] : 0.0;
        }
        for (uint32_t w = w0; w < w1; ++w) {
            uint32_t r0 = a.edges[w], r1 = a.edges[w + 1u];
            r0 = r0 < m ? r0 : m;
            r1 = r1 < m ? r1 : m;
            Col col[4];
            uint32_t kept_bits = 0u;   // the above bits of this lane's row in the step before
            for (uint32_t r = r0; r < r1; r += kUnroll * rps) {   // (uniform; r1 <= tick_cap < 2^31: no wrap)
                uint4 v[kUnroll];
#pragma unroll
                for (uint32_t u = 0; u < kUnroll; ++u) {
                    const uint32_t k = r + u * rps + row_off;
                    v[u] = on && k < r1 ? rows[(size_t)k * pq + cg] : uint4{};
                }
#pragma unroll
                for (uint32_t u = 0; u < kUnroll; ++u) {
                    if (r + u * rps >= r1) break;                 // (uniform)
                    const uint32_t k = r + u * rps + row_off;
                    const bool live = on && k < r1;
                    const uint32_t word[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
                    uint32_t bits = 0u;
#pragma unroll
                    for (uint32_t c = 0; c < 4u; ++c) {
                        const double x = is_f[c] ? (double)__uint_as_float(word[c]) : (double)word[c];
                        const uint32_t key = is_f[c] ? afs::float_key(word[c]) : word[c];
                        bits |= live && x > thr[c] ? 1u << c : 0u;
                        const unsigned long long pk = live ? ((unsigned long long)key << 32) | (uint32_t)~k : 0ull;
                        col[c].pk = pk > col[c].pk ? pk : col[c].pk;
                    }
                    // tick k - 1: the lane L below; the first row of a step asks the last row, which offers the step before's
                    const uint32_t below = (uint32_t)__shfl((int)(last_row ? kept_bits : bits), below_lane, 64);
                    kept_bits = bits;
                    const uint32_t rise = bits & ~below;
#pragma unroll
                    for (uint32_t c = 0; c < 4u; ++c) {
                        const bool ab = (bits >> c) & 1u, up = (rise >> c) & 1u;
                        if (__ballot(ab) == 0ull) continue;       // (uniform: no rise, no above tick, the carry stays)
                        uint32_t st = up ? k + 1u : 0u;           // the latest rise at or before this row, + 1
                        for (uint32_t d = 1u; d < rps; d <<= 1) {
                            const uint32_t o = __shfl_up(st, d * L, 64);
                            st = row_off >= d && o > st ? o : st;
                        }
                        st = col[c].carry > st ? col[c].carry : st;
                        col[c].carry = __shfl(st, top_lane, 64);
                        if (ab) {                                 // (st >= 1: an above tick lies in a run that rose in the window)
                            col[c].ab += 1u;
                            col[c].ru += up ? 1u : 0u;
                            col[c].fi = k < col[c].fi ? k : col[c].fi;
                            col[c].la = k + 1u;                   // (a lane's rows ascend)
                            const unsigned long long lg = ((unsigned long long)(k + 2u - st) << 32) | (uint32_t)~(st - 1u);
                            col[c].lg = lg > col[c].lg ? lg : col[c].lg;
                        }
                    }
                }
            }
            for (uint32_t h = p2 >> 1; h >= 1u; h >>= 1) {   // (uniform: every lane of the wave shuffles)
                const bool take = row_off < h && row_off + h < rps;
#pragma unroll
                for (int c = 0; c < 4; ++c) col[c].fold((int)(h * L), take);
            }
            if (!on || row_off != 0u) continue;
            const size_t cell = (size_t)s * W + w;
            if (cg == 0u && a.count) a.count[cell] = r1 - r0;
#pragma unroll
            for (uint32_t c = 0; c < 4u; ++c) {
                const uint32_t j = cg * 4u + c;
                if (j >= S) continue;
                const size_t o = cell * S + j;
                const Col& x = col[c];
                if (a.above) a.above[o] = x.ab;
                if (a.runs) a.runs[o] = x.ru;
                if (a.longest) a.longest[o] = (uint32_t)(x.lg >> 32);
                if (a.longest_start) a.longest_start[o] = x.lg ? ~(uint32_t)x.lg : kNone;
                if (a.first) a.first[o] = x.fi;
                if (a.last) a.last[o] = x.la ? x.la - 1u : kNone;
                if (a.peak_tick) a.peak_tick[o] = x.pk ? ~(uint32_t)x.pk : kNone;
            }
        }
    }
}

}  // namespace afsx
