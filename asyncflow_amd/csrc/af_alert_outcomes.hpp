// af_alert_outcomes.hpp -- BURN-RATE ALERT RULES ON REQUEST OUTCOMES: a client timeout makes a request that never came back
// visible to the monitor (af_engine_outcome_alerts, launched by engine.hip).  af_alerts.hpp sees completions only; here
// every ARRIVAL produces exactly one event, a completion or a timeout, so the bad share has the arrivals as its denominator and
// slo = +inf is a pure availability alert.
//
// DEFINITION.  Scenario s has m_s stored rows (start_i, finish_i), t_s sample rows and p = sample_period, all as in af_alerts_t;
// an arrival row a[0 .. draw_capacity), row time_row[s] of `times`, ascending with +inf behind the last arrival; tau = timeout,
// finite and > 0; slo as in af_alerts_t (not NaN; +inf allowed).
//   tick of a time   q(x) = floor(x / p): one f64 division, then floor.  It is in range iff 0 <= q < t_s, compared on the f64
//                    quotient (afal::row_tick's rule).
//   in-time row      start_i and finish_i are not NaN and lat_i = finish_i - start_i <= tau: one f64 subtraction, a NaN latency
//                    is not in time.  A row that is not in time is never seen as a completion: the client gave up at start + tau.
//   C[k]             = #{ in-time rows with q(finish_i) == k }
//   Cbad[k]          = those of C[k] with lat_i > slo
//   G[k]             = #{ in-time rows with q(start_i + tau) == k }: one f64 addition, then the tick rule
//   A[k]             = #{ j < draw_capacity : a[j] finite and q(a[j] + tau) == k }: the same operations
//   timeouts[k]      = max(A[k] - G[k], 0)
//   deficit[s]       = sum over k of max(G[k] - A[k], 0)
//   timed_out[s]     = sum over k of timeouts[k]
//   total[k]         = C[k] + timeouts[k]
//   bad[k]           = Cbad[k] + timeouts[k]
// deficit is 0 whenever the arrival row is the run's own: every stored start is, bit for bit, one of its arrivals, so an in-time
// row and its own arrival land on the same timeout tick -- the same f64 operations on the same bits; the counts need no join.  A
// deficit above 0 says the arrival rows do not belong to these clock rows; the result is still defined.
// Prefix sums, rolling look-backs, rules, windows, cells, group cells and delay_hist are exactly af_engine_summarize_alerts's on
// these total / bad.  All per-tick values are u32.
// The host definition refuses a non-ascending arrival row; the device does not check: such a row gives meaningless counts and
// nothing worse (every tick is compared with the chunk before it indexes).
// flags[s]: kRowsTruncated when counts[s][completed] > clock_capacity (rows are missing and would be miscounted as timeouts),
// kDeficit when deficit[s] > 0.
//
// KERNEL.  af_alert_outcomes_prefix_kernel is shaped like af_alerts_prefix_kernel: a workgroup of eight waves owns a scenario and
// walks its ticks in CHUNKS of kChunkTicks.  Per chunk every stored row once, 16-byte loads (one (start, finish) pair), kUnroll of
// them in flight per lane; per row one subtraction, one addition and two divisions; LDS +1 into C[] and, where bad, into Cbad[],
// and -1 into the signed pend[] at the row's timeout tick.  Then the part of the arrival row that falls into the chunk: q(a + tau)
// is monotone in a, so the part is ONE contiguous range, found by two binary searches on the TICK (not on the time: a + tau
// rounds); it is streamed with 16-byte loads (an odd element in front and behind by one lane) and adds +1 into pend[].  Then the
// tile scan of af_alerts_prefix_kernel (the engine's DPP wave scan, the carry across tiles and chunks) over C + max(pend, 0) and
// Cbad + max(pend, 0); (PT, PB) go out as one 8-byte vector store per tick into the scratch layout af_alerts_eval_kernel reads; the
// per-tick total / bad / timeouts outputs when asked for; deficit and timed_out are summed beside the scan.  No global atomics, no
// zeroing.
// LDS: three arrays of kChunkTicks = 12 288 words = 147 456 B = 144 KiB, and the scan's 4 x 8 words (128 B) behind them: 147 584 B
// of the 163 840 B a compute unit has, which one workgroup may take whole.  So the chunk stays af_alerts.hpp's: a run of 11 999
// ticks is one chunk, one pass over the rows and the arrivals; one workgroup per compute unit, two waves per SIMD.
// af_alerts_eval_kernel is reused as it is.
//
// The per-row rule, the arrival rule, the binary search, the clamp and the sequential statement of a scenario that walks chunk by
// chunk as the kernel does (scenario_outcome_ticks) are AF_HD text without a HIP include: gfx950 device code and, under g++, what
// tests/hostcheck/alert_outcomes_main.cpp runs under the sanitizers.
#pragma once

#include <stdint.h>

#include "af_alerts.hpp"

namespace afao {

constexpr uint32_t kChunkTicks = afal::kChunkTicks;   // 12 288: three LDS arrays of it are 144 KiB (see above)
constexpr uint32_t kThreads = afal::kThreads;         // eight waves a workgroup
constexpr uint32_t kWaves = kThreads / 64u;
constexpr uint32_t kUnroll = afal::kUnroll;           // 16-byte loads a lane has in flight
constexpr uint32_t kRowsTruncated = 1u;               // AF_OUTCOME_ROWS_TRUNCATED
constexpr uint32_t kDeficit = 2u;                     // AF_OUTCOME_DEFICIT
static_assert(kChunkTicks % kThreads == 0u, "a chunk is whole tiles");
static_assert(3u * kChunkTicks * 4u + 4u * kWaves * 4u <= 160u * 1024u, "the chunk arrays and the scan's words fit a compute unit's LDS");

// q(x) as an f64: a whole number or +-inf (NaN for a NaN x)
AF_HD double tick_q(double x, double period) { return __builtin_floor(x / period); }
// the tick rule: true when 0 <= q < t_s, then k = q
AF_HD bool tick_in_range(double q, uint32_t t_s, uint32_t& k) {
    if (!(q >= 0.0) || !(q < (double)t_s)) return false;   // (-0.0 is tick 0; +inf clips; NaN is out)
    k = (uint32_t)q;
    return true;
}

// A stored row: true when it is in time.  Then f_ok / f: its completion tick is in range / that tick; bad: lat > slo;
// g_ok / g: its timeout tick is in range / that tick.
AF_HD bool outcome_row(double start, double finish, double period, double slo, double tau, uint32_t t_s, bool& f_ok, uint32_t& f,
                       bool& bad, bool& g_ok, uint32_t& g) {
    if (start != start || finish != finish) return false;   // NaN
    const double lat = finish - start;
    if (!(lat <= tau)) return false;                         // (a NaN latency, inf - inf, is not in time)
    f_ok = tick_in_range(tick_q(finish, period), t_s, f);
    bad = lat > slo;
    g_ok = tick_in_range(tick_q(start + tau, period), t_s, g);
    return true;
}

// An arrival: true when it is finite and its timeout tick is in range, then g = that tick.
AF_HD bool arrival_tick(double a, double period, double tau, uint32_t t_s, uint32_t& g) {
    if (!(a - a == 0.0)) return false;                       // NaN or +-inf
    return tick_in_range(tick_q(a + tau, period), t_s, g);
}

// The first j in [0, n) with q(a[j] + tau) >= bound on an ascending row (n: none).  On the tick, not on the time; +inf behind the
// last arrival has q = +inf and is never below a bound.
AF_HD uint32_t arrival_lower(const double* a, uint32_t n, double period, double tau, uint32_t bound) {
    uint32_t lo = 0u, hi = n;                                // (n < 2^31: lo + hi does not wrap)
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tick_q(a[mid] + tau, period) < (double)bound) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// what a tick makes of its chunk words: the timeouts and the deficit of the tick
AF_HD uint32_t timeouts_of(int32_t pend) { return pend > 0 ? (uint32_t)pend : 0u; }
AF_HD uint32_t deficit_of(int32_t pend) { return pend < 0 ? 0u - (uint32_t)pend : 0u; }

// One scenario, sequentially, chunk by chunk as the kernel walks it.  rows [m][2]; arr [n_arr] ascending; c_c / cbad_c / pend_c:
// the chunk arrays, `chunk` words each; pt / pb: the prefix arrays [t_s]; total / bad / timeouts: per-tick outputs [t_s] (any
// may be null); deficit / timed_out: one word each.
AF_HD void scenario_outcome_ticks(const double* rows, uint32_t m, const double* arr, uint32_t n_arr, double period, double slo, double tau,
                                  uint32_t t_s, uint32_t chunk, uint32_t* c_c, uint32_t* cbad_c, int32_t* pend_c, uint32_t* pt, uint32_t* pb,
                                  uint32_t* total, uint32_t* bad, uint32_t* timeouts, uint32_t& deficit, uint32_t& timed_out) {
    uint32_t ct = 0u, cb = 0u;   // the prefix at the previous chunk's last tick
    deficit = timed_out = 0u;
    for (uint32_t c0 = 0u; c0 < t_s; c0 += chunk) {
        const uint32_t c1 = t_s - c0 < chunk ? t_s : c0 + chunk;
        for (uint32_t k = 0u; k < c1 - c0; ++k) {
            c_c[k] = cbad_c[k] = 0u;
            pend_c[k] = 0;
        }
        for (uint32_t i = 0u; i < m; ++i) {
            bool f_ok, g_ok, is_bad;
            uint32_t f = 0u, g = 0u;
            if (!outcome_row(rows[2u * i], rows[2u * i + 1u], period, slo, tau, t_s, f_ok, f, is_bad, g_ok, g)) continue;
            if (f_ok && f >= c0 && f < c1) {
                c_c[f - c0] += 1u;
                if (is_bad) cbad_c[f - c0] += 1u;
            }
            if (g_ok && g >= c0 && g < c1) pend_c[g - c0] -= 1;
        }
        const uint32_t j_lo = arrival_lower(arr, n_arr, period, tau, c0), j_hi = arrival_lower(arr, n_arr, period, tau, c1);
        for (uint32_t j = j_lo; j < j_hi; ++j) {
            uint32_t g;
            if (arrival_tick(arr[j], period, tau, t_s, g) && g >= c0 && g < c1) pend_c[g - c0] += 1;
        }
        for (uint32_t k = 0u; k < c1 - c0; ++k) {
            const uint32_t to = timeouts_of(pend_c[k]), tv = c_c[k] + to, bv = cbad_c[k] + to;
            if (total) total[c0 + k] = tv;
            if (bad) bad[c0 + k] = bv;
            if (timeouts) timeouts[c0 + k] = to;
            timed_out += to;
            deficit += deficit_of(pend_c[k]);
            ct += tv;
            cb += bv;
            pt[c0 + k] = ct;
            pb[c0 + k] = cb;
        }
        if (c1 == t_s) break;   // (c0 + chunk could wrap)
    }
}

#if defined(__HIPCC__)
struct OcArgs {
    afal::AlArgs al;            // the clock rows, the counts, the prefix scratch and total / bad as af_alerts_prefix_kernel takes them
    const double* times;        // [n_time_rows][draw_cap]
    const uint32_t* time_row;   // [n], or null: scenario s reads row s
    uint32_t draw_cap;
    double tau;
    uint32_t* timeouts;         // [n][tick_cap] or null
    uint32_t *timed_out, *deficit, *flags;   // [n] or null
};

// W: the engine's wave primitives (scan_incl_u32, the DPP scan).
template <class W>
__global__ void __launch_bounds__(kThreads) af_alert_outcomes_prefix_kernel(const OcArgs o) {
    extern __shared__ uint32_t afao_lds[];   // [kChunkTicks] C, [kChunkTicks] Cbad, [kChunkTicks] pend (signed)
    __shared__ uint32_t wave_tot[kWaves], wave_bad[kWaves], wave_to[kWaves], wave_df[kWaves];
    const afal::AlArgs& a = o.al;
    uint32_t* cc = afao_lds;
    uint32_t* cbd = afao_lds + kChunkTicks;
    int32_t* pend = reinterpret_cast<int32_t*>(afao_lds + 2u * kChunkTicks);
    const uint32_t s = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t completed = a.counts[(size_t)s * 8u + a.cnt_completed_slot];
    const uint32_t m = completed < a.clock_cap ? completed : a.clock_cap;
    uint32_t t_s = a.counts[(size_t)s * 8u + a.cnt_ticks_slot];
    t_s = t_s < a.tick_cap ? t_s : a.tick_cap;
    const double2* ck = reinterpret_cast<const double2*>(a.clock) + (size_t)s * a.clock_cap;
    const double* ar = o.times + (size_t)(o.time_row ? o.time_row[s] : s) * o.draw_cap;   // (the host checked the row ids)
    const size_t row = (size_t)s * a.tick_cap;
    uint32_t ct = 0u, cb = 0u;           // the prefix at the previous tile's last tick
    uint32_t my_to = 0u, my_df = 0u;     // this lane's part of timed_out and deficit
    for (uint32_t c0 = 0u; c0 < t_s; c0 += kChunkTicks) {   // (uniform; t_s <= tick_cap < 2^31: no wrap)
        const uint32_t c1 = t_s - c0 < kChunkTicks ? t_s : c0 + kChunkTicks, len = c1 - c0;
        for (uint32_t k = tid; k < len; k += kThreads) {
            cc[k] = cbd[k] = 0u;
            pend[k] = 0;
        }
        __syncthreads();
        for (uint32_t base = 0u; base < m; base += kThreads * kUnroll) {   // (m <= clock_cap; the engine keeps n * clock_cap rows addressable)
            double2 c[kUnroll];
#pragma unroll
            for (uint32_t u = 0; u < kUnroll; ++u) {
                const uint32_t i = base + u * kThreads + tid;
                c[u] = i < m && i >= base ? ck[i] : double2{0.0, __builtin_nan("")};   // (a row that is not in time; i >= base: no wrap)
            }
#pragma unroll
            for (uint32_t u = 0; u < kUnroll; ++u) {
                bool f_ok, g_ok, is_bad;
                uint32_t f = 0u, g = 0u;
                if (!outcome_row(c[u].x, c[u].y, a.period, a.slo, o.tau, t_s, f_ok, f, is_bad, g_ok, g)) continue;
                if (f_ok && f >= c0 && f < c1) {
                    atomicAdd(&cc[f - c0], 1u);
                    if (is_bad) atomicAdd(&cbd[f - c0], 1u);
                }
                if (g_ok && g >= c0 && g < c1) atomicAdd(&pend[g - c0], -1);
            }
            if (m - base <= kThreads * kUnroll) break;   // (base + kThreads * kUnroll could wrap)
        }
        {   // the arrivals whose timeout falls into the chunk: a[j_lo .. j_hi), every lane searches the same words
            const uint32_t j_lo = arrival_lower(ar, o.draw_cap, a.period, o.tau, c0), j_hi = arrival_lower(ar, o.draw_cap, a.period, o.tau, c1);
            auto add = [&](double x) {
                uint32_t g;
                if (arrival_tick(x, a.period, o.tau, t_s, g) && g >= c0 && g < c1) atomicAdd(&pend[g - c0], 1);   // (compared again: a row out of order)
            };
            if (j_lo < j_hi) {   // (uniform)
                const uint32_t head = (uint32_t)((reinterpret_cast<uintptr_t>(ar + j_lo) >> 3) & 1u);   // an element before the first 16-byte pair
                const uint32_t j0 = j_lo + head, pairs = (j_hi - j0) >> 1;
                if (head && tid == 0u) add(ar[j_lo]);
                if (((j_hi - j0) & 1u) && tid == 64u) add(ar[j_hi - 1u]);                               // an element behind the last pair
                const double2* ap = reinterpret_cast<const double2*>(ar + j0);
                for (uint32_t base = 0u; base < pairs; base += kThreads * kUnroll) {                     // (pairs < 2^30: no wrap)
                    double2 v[kUnroll];
#pragma unroll
                    for (uint32_t u = 0; u < kUnroll; ++u) {
                        const uint32_t i = base + u * kThreads + tid;
                        v[u] = i < pairs ? ap[i] : double2{__builtin_nan(""), __builtin_nan("")};
                    }
#pragma unroll
                    for (uint32_t u = 0; u < kUnroll; ++u) {
                        add(v[u].x);
                        add(v[u].y);
                    }
                }
            }
        }
        __syncthreads();
        for (uint32_t t0 = 0u; t0 < len; t0 += kThreads) {   // (uniform: the scan and the barriers are block-wide)
            const uint32_t k = t0 + tid;
            const int32_t pv = k < len ? pend[k] : 0;
            const uint32_t to = timeouts_of(pv);
            const uint32_t tv = (k < len ? cc[k] : 0u) + to, bv = (k < len ? cbd[k] : 0u) + to;
            my_to += to;
            my_df += deficit_of(pv);
            uint32_t pt = W::scan_incl_u32(tv), pb = W::scan_incl_u32(bv);
            if (lane == 63u) {
                wave_tot[wave] = pt;
                wave_bad[wave] = pb;
            }
            __syncthreads();
            uint32_t before_t = 0u, all_t = 0u, before_b = 0u, all_b = 0u;
#pragma unroll
            for (uint32_t w = 0; w < kWaves; ++w) {
                const uint32_t t = wave_tot[w], b = wave_bad[w];
                before_t += w < wave ? t : 0u;
                before_b += w < wave ? b : 0u;
                all_t += t;
                all_b += b;
            }
            pt += ct + before_t;
            pb += cb + before_b;
            ct += all_t;
            cb += all_b;
            if (k < len) {
                a.prefix[row + c0 + k] = uint2{pt, pb};
                if (a.total) a.total[row + c0 + k] = tv;
                if (a.bad) a.bad[row + c0 + k] = bv;
                if (o.timeouts) o.timeouts[row + c0 + k] = to;
            }
            __syncthreads();   // (wave_tot and wave_bad are written again)
        }
        if (c1 == t_s) break;  // (the barrier above also stands before the next chunk's clearing)
    }
    // timed_out and deficit: the same wave scan over the lanes' parts, the waves' totals through LDS
    const uint32_t s_to = W::scan_incl_u32(my_to), s_df = W::scan_incl_u32(my_df);
    if (lane == 63u) {
        wave_to[wave] = s_to;
        wave_df[wave] = s_df;
    }
    __syncthreads();
    if (tid == 0u) {
        uint32_t all_to = 0u, all_df = 0u;
#pragma unroll
        for (uint32_t w = 0; w < kWaves; ++w) {
            all_to += wave_to[w];
            all_df += wave_df[w];
        }
        if (o.timed_out) o.timed_out[s] = all_to;
        if (o.deficit) o.deficit[s] = all_df;
        if (o.flags) o.flags[s] = (completed > a.clock_cap ? kRowsTruncated : 0u) | (all_df ? kDeficit : 0u);
    }
}
#endif  // __HIPCC__

}  // namespace afao
