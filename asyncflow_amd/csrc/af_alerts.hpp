// af_alerts.hpp -- BURN-RATE ALERT RULES evaluated at every tick over ROLLING look-backs of the completions, from the clock rows
// (af_engine_summarize_alerts, launched by engine.hip): would the alert have fired, how many ticks after an event, for how long,
// how often.  Every other analyzer puts requests into tumbling windows; a monitor evaluates a rule at every scrape.
//
// DEFINITION.  Scenario s has m_s = min(counts[s][completed], clock_cap) stored rows (start_i, finish_i) and t_s =
// min(counts[s][ticks], tick_cap) sample rows; p = sample_period; sample row k is taken at (k + 1) p (af_series_windows_t).
//   tick of a row    f_i = floor(finish_i / p): one f64 division rounded to nearest, then floor (af_inflight.hpp's rule).  Row i is
//                    COUNTED iff start_i and finish_i are not NaN and 0 <= f_i < t_s, compared on the f64 quotient: a huge or
//                    infinite quotient clips, it does not wrap.  Nothing else is rejected: start < 0, finish < start and a
//                    latency below a tick are counted -- a monitor sees every completion.
//   bad              lat_i = finish_i - start_i, one f64 subtraction; bad_i iff lat_i > slo (slo = +inf: nothing is bad).
//   per tick         total[s][k] = #{ counted i : f_i == k }, bad[s][k] = #{ counted bad i : f_i == k }, both u32, whatever the
//                    order of the rows.
//   prefix, rolling  PT[k] = sum over j <= k of total[j], PB likewise (u32: at most m_s).  For a look-back of L >= 1 ticks
//                    T_L[k] = PT[k] - (k >= L ? PT[k - L] : 0), B_L likewise: the first L - 1 ticks see the rows that exist; a
//                    look-back reaches across window edges -- it is a property of the tick.
//   rule r           (long_ticks >= short_ticks >= 1, num <= den, den >= 1, min_total, hold_ticks >= 1), products in u64:
//                    cond_r[k]   = B_long[k] den > num T_long[k]  &&  B_short[k] den > num T_short[k]  &&  T_long[k] >= min_total
//                    firing_r[k] = k + 1 >= hold_ticks and cond_r[j] for every j in (k - hold_ticks, k].  No hysteresis.
//   cell (s, w, r)   windows are tick edges b[0] < ... < b[W], lo = min(b[w], t_s), hi = min(b[w + 1], t_s); they choose where
//                    firing is REPORTED, never what a rule sees.  count = hi - lo; fired = the firing ticks; episodes = the
//                    maximal runs of firing ticks inside [lo, hi) (a run across an edge counts in both windows); longest and
//                    longest_start (the earliest run of that length); first, last (kNone: no such tick).
//   cell (g, w, r)   over the members s of g (AF_POOL_SKIP: in none): members (hi > lo), fired_members (first != NONE),
//                    open_members (last == hi - 1), fire_ticks and fire_episodes (u64 sums), delay_hist: a member that fired
//                    adds 1 to bin min((first - lo) / delay_width, n_bins - 1).
// COMPLETED REQUESTS ONLY: a dropped request, and one still in flight when the run ended, is in no clock row -- an alert on
// availability needs af_alert_outcomes.hpp, and the last ticks of a run see fewer completions.
//
// KERNELS.
//   af_alerts_prefix_kernel   a workgroup owns a scenario and walks its ticks in CHUNKS of kChunkTicks.  Per chunk every stored
//          row once, 16-byte loads (one (start, finish) pair), kUnroll of them in flight per lane; one f64 division and one
//          subtraction per row; LDS +1 into total[] and, where the row is bad, into bad[].  Then tiles of kThreads ticks: the
//          DPP wave scan of the engine, the waves' totals through LDS and the CARRY across tiles and chunks.  PT and PB go out
//          as one 8-byte vector store per tick to engine scratch [n][tick_cap]; the per-tick total / bad outputs when asked for.
//          No global atomics, no zeroing.  LDS: 2 kChunkTicks words = 96 KiB: one workgroup per compute unit of 160 KiB.
//   af_alerts_eval_kernel     a wave owns a scenario and walks its ticks in STEPS of 64, lane l at tick k0 + l.  Per rule every
//          lane loads (PT, PB) at k, k - long and k - short (L2 hits: the same rows a few steps back), forms the u64 products,
//          and the condition becomes a 64-bit ballot mask, which LANE r KEEPS for rule r.  From there the 32 rules run side by
//          side, one per lane, on their own masks: hold_step turns the condition mask into the firing mask (the run of ones
//          carried in from the step before stands for every earlier tick, so hold_ticks may be far above 64), cell_step adds the
//          part of the firing mask inside the current window to the cell (episodes, longest run and its start with the open
//          run carried across steps, first, last).  When a window ends, lanes 0 .. R - 1 store the scenario's cells of that
//          window side by side and add them to the group's cells: integer atomics on outputs the call initialised.
// Every word is identical from run to run and does not depend on the batch a scenario sits in.
//
// The per-row rule, the rolling difference, the condition and the mask steps (hold_step, cell_step, with their carries), and the
// sequential statement of a scenario that walks chunk by chunk and step by step as the kernels do (scenario_alerts) are AF_HD text
// without a HIP include: gfx950 device code and, under g++, what tests/hostcheck/alerts_main.cpp runs under the sanitizers.
#pragma once

#include <stdint.h>

#if !defined(AF_HD)
#if defined(__HIPCC__)
#define AF_HD __host__ __device__ __forceinline__
#else
#define AF_HD inline
#endif
#endif

namespace afal {

constexpr uint32_t kChunkTicks = 12288;       // ticks of one LDS chunk (config 2's 12 000 ticks: one pass over the rows)
constexpr uint32_t kThreads = 512;            // eight waves a workgroup of the prefix kernel
constexpr uint32_t kWaves = kThreads / 64u;
constexpr uint32_t kUnroll = 4;               // 16-byte loads a lane has in flight
constexpr uint32_t kEvalThreads = 256;        // four waves, four scenarios, a workgroup of the evaluation kernel
constexpr uint32_t kEvalWaves = kEvalThreads / 64u;
constexpr uint32_t kSkip = 0xFFFFFFFFu;       // AF_POOL_SKIP
constexpr uint32_t kNone = 0xFFFFFFFFu;       // AF_TICK_NONE
constexpr uint32_t kMaxRules = 32;            // AF_MAX_ALERT_RULES: a bit of the firing word each, a lane of the wave each
constexpr uint32_t kMaxBins = 1024;           // AF_MAX_SERIES_HISTOGRAM_BINS
static_assert(kChunkTicks % kThreads == 0u, "a chunk is whole tiles");

struct Rule {   // af_alert_rule_t
    uint32_t long_ticks, short_ticks, num, den, min_total, hold_ticks;
};

// The tick of a row's completion: true when the row is counted, then 0 <= f < t_s; `bad` is its latency above slo.
AF_HD bool row_tick(double start, double finish, double period, double slo, uint32_t t_s, uint32_t& f, bool& bad) {
    if (start != start || finish != finish) return false;   // NaN
    const double qf = __builtin_floor(finish / period);     // (a whole number or +-inf, no NaN here)
    if (!(qf >= 0.0) || !(qf < (double)t_s)) return false;  // (-0.0 is tick 0; +inf clips)
    f = (uint32_t)qf;
    bad = finish - start > slo;                             // (inf - inf: NaN, not bad)
    return true;
}

// T_L[k] or B_L[k] from the prefix at k and at k - L (`has_back`: k >= L)
AF_HD uint32_t rolling(uint32_t p_k, uint32_t p_back, bool has_back) { return p_k - (has_back ? p_back : 0u); }

AF_HD bool alert_cond(const Rule& r, uint32_t t_long, uint32_t b_long, uint32_t t_short, uint32_t b_short) {
    return (uint64_t)b_long * r.den > (uint64_t)r.num * t_long && (uint64_t)b_short * r.den > (uint64_t)r.num * t_short && t_long >= r.min_total;
}

// the first run of ones of a mask that is not 0: its lowest bit s and its length
AF_HD void first_run(uint64_t m, uint32_t& s, uint32_t& len) {
    s = (uint32_t)__builtin_ctzll(m);
    const uint64_t x = ~(m >> s);
    len = x ? (uint32_t)__builtin_ctzll(x) : 64u;   // (x == 0: s == 0 and all 64 ones)
}
// the mask without its bits below `top` (1 .. 64)
AF_HD uint64_t clear_below(uint64_t m, uint32_t top) { return top >= 64u ? 0ull : m & ~((1ull << top) - 1ull); }
// bits [lo, hi) of a step, 0 <= lo < hi <= 64
AF_HD uint64_t range_mask(uint32_t lo, uint32_t hi) { return (hi >= 64u ? ~0ull : (1ull << hi) - 1ull) & ~((1ull << lo) - 1ull); }

// The `for:` clause on one step of 64 ticks.  cond: the condition at the step's ticks; run: in, the ones of cond that end at the
// tick before the step (all the way back: hold may be far above 64); out, those that end at the step's last tick.  Returns the
// firing mask: bit j iff the run of ones that ends at j, the carried ones included, is at least `hold` long.
AF_HD uint64_t hold_step(uint64_t cond, uint32_t hold, uint32_t& run) {
    uint64_t out = 0ull, rest = cond;
    uint32_t run_out = 0u;
    while (rest) {
        uint32_t s, len;
        first_run(rest, s, len);
        const uint32_t prior = s == 0u ? run : 0u;
        const uint32_t need = hold - 1u > prior ? hold - 1u - prior : 0u;   // ones of this run before the first firing one
        if (need < len) out |= range_mask(s + need, s + len);
        if (s + len == 64u) run_out = prior + len;                            // (at most t_s < 2^31)
        rest = clear_below(rest, s + len);
    }
    run = run_out;
    return out;
}

// what a (scenario, window, rule) cell keeps while its window is walked
struct Cell {
    uint32_t fired, episodes, longest, longest_start, first, last;
    uint32_t open, open_start;   // the run that ends at the last tick seen: its length inside the window (0: none) and its start
};
AF_HD void cell_reset(Cell& c) {
    c.fired = c.episodes = c.longest = c.open = c.open_start = 0u;
    c.longest_start = c.first = c.last = kNone;
}
// One step's part of a window: f holds the firing bits of the ticks [a, b) of the window, a subrange of the step [k0, k0 + 64),
// and no other bit; the ticks of a window arrive in ascending order without gaps.
AF_HD void cell_step(Cell& c, uint64_t f, uint32_t k0, uint32_t a, uint32_t b) {
    const uint32_t sa = a - k0, sb = b - k0;
    const bool joined = c.open > 0u;   // tick a - 1 lies in the window and fires
    bool reaches = false;
    uint64_t rest = f;
    while (rest) {
        uint32_t s, len;
        first_run(rest, s, len);
        uint32_t start = k0 + s, length = len;
        if (s == sa && joined) {       // the open run goes on
            start = c.open_start;
            length += c.open;
        } else {
            c.episodes += 1u;
        }
        if (length > c.longest) {      // (ascending: the earliest run of a length wins)
            c.longest = length;
            c.longest_start = start;
        }
        if (s + len == sb) {
            c.open = length;
            c.open_start = start;
            reaches = true;
        }
        rest = clear_below(rest, s + len);
    }
    if (!reaches) c.open = 0u;
    if (f) {
        c.fired += (uint32_t)__builtin_popcountll(f);
        if (c.first == kNone) c.first = k0 + (uint32_t)__builtin_ctzll(f);
        c.last = k0 + 63u - (uint32_t)__builtin_clzll(f);
    }
}

AF_HD uint32_t delay_bin(uint32_t first, uint32_t lo, uint32_t width, uint32_t n_bins) {
    const uint32_t b = (first - lo) / width;
    return b < n_bins ? b : n_bins - 1u;
}

// One scenario, sequentially, chunk by chunk and step by step as the kernels walk it.  rows [m][2]; tot_c / bad_c: the chunk
// arrays, `chunk` words each; pt / pb: the prefix arrays [t_s]; total / bad / firing: per-tick outputs [t_s] (any may be null);
// count [W] and the cells [W][R] (any may be null).  edges [W + 1] ascending.
AF_HD void scenario_alerts(const double* rows, uint32_t m, double period, double slo, uint32_t t_s, uint32_t chunk, uint32_t* tot_c,
                           uint32_t* bad_c, uint32_t* pt, uint32_t* pb, const Rule* rules, uint32_t R, const uint32_t* edges, uint32_t W,
                           uint32_t* total, uint32_t* bad, uint32_t* firing, uint32_t* count, uint32_t* fired, uint32_t* episodes,
                           uint32_t* longest, uint32_t* longest_start, uint32_t* first, uint32_t* last) {
    uint32_t ct = 0u, cb = 0u;   // the prefix at the previous chunk's last tick
    for (uint32_t c0 = 0u; c0 < t_s; c0 += chunk) {
        const uint32_t c1 = t_s - c0 < chunk ? t_s : c0 + chunk;
        for (uint32_t k = 0u; k < c1 - c0; ++k) tot_c[k] = bad_c[k] = 0u;
        for (uint32_t i = 0u; i < m; ++i) {
            uint32_t f;
            bool is_bad;
            if (!row_tick(rows[2u * i], rows[2u * i + 1u], period, slo, t_s, f, is_bad) || f < c0 || f >= c1) continue;
            tot_c[f - c0] += 1u;
            if (is_bad) bad_c[f - c0] += 1u;
        }
        for (uint32_t k = 0u; k < c1 - c0; ++k) {
            if (total) total[c0 + k] = tot_c[k];
            if (bad) bad[c0 + k] = bad_c[k];
            ct += tot_c[k];
            cb += bad_c[k];
            pt[c0 + k] = ct;
            pb[c0 + k] = cb;
        }
        if (c1 == t_s) break;   // (c0 + chunk could wrap)
    }
    for (uint32_t r = 0u; r < R; ++r) {   // (the kernel: the rules side by side, a lane each)
        const Rule& ru = rules[r];
        uint32_t run = 0u, w = 0u;
        Cell c;
        cell_reset(c);
        auto flush = [&](uint32_t lo, uint32_t hi) {
            const uint64_t o = (uint64_t)w * R + r;
            if (count && r == 0u) count[w] = hi - lo;
            if (fired) fired[o] = c.fired;
            if (episodes) episodes[o] = c.episodes;
            if (longest) longest[o] = c.longest;
            if (longest_start) longest_start[o] = c.longest_start;
            if (first) first[o] = c.first;
            if (last) last[o] = c.last;
            cell_reset(c);
            ++w;
        };
        for (uint32_t k0 = 0u; k0 < t_s; k0 += 64u) {
            const uint32_t k_end = t_s - k0 < 64u ? t_s : k0 + 64u;
            uint64_t cond = 0ull;
            for (uint32_t k = k0; k < k_end; ++k) {
                const bool hl = k >= ru.long_ticks, hs = k >= ru.short_ticks;
                const uint32_t tl = rolling(pt[k], hl ? pt[k - ru.long_ticks] : 0u, hl), bl = rolling(pb[k], hl ? pb[k - ru.long_ticks] : 0u, hl);
                const uint32_t ts = rolling(pt[k], hs ? pt[k - ru.short_ticks] : 0u, hs), bs = rolling(pb[k], hs ? pb[k - ru.short_ticks] : 0u, hs);
                if (alert_cond(ru, tl, bl, ts, bs)) cond |= 1ull << (k - k0);
            }
            const uint64_t f = hold_step(cond, ru.hold_ticks, run);
            if (firing)
                for (uint32_t k = k0; k < k_end; ++k) firing[k] = (r ? firing[k] : 0u) | (uint32_t)((f >> (k - k0)) & 1ull) << r;
            while (w < W) {
                const uint32_t lo = edges[w] < t_s ? edges[w] : t_s, hi = edges[w + 1u] < t_s ? edges[w + 1u] : t_s;
                const uint32_t a = lo > k0 ? lo : k0, b = hi < k_end ? hi : k_end;
                if (a < b) cell_step(c, f & range_mask(a - k0, b - k0), k0, a, b);
                if (hi > k_end) break;   // the window goes on in the next step
                flush(lo, hi);
            }
        }
        while (w < W) {                  // (without ticks: every window is empty)
            const uint32_t lo = edges[w] < t_s ? edges[w] : t_s, hi = edges[w + 1u] < t_s ? edges[w + 1u] : t_s;
            flush(lo, hi);
        }
    }
}

#if defined(__HIPCC__)
struct AlArgs {
    const double* clock;        // [n][clock_cap][2]
    const uint32_t* counts;     // [n][8]
    uint32_t clock_cap, tick_cap, cnt_completed_slot, cnt_ticks_slot;
    double period, slo;
    uint32_t n_scen, n_win, n_rules, n_bins, delay_width;
    const uint32_t* group;      // [n], or null: all in group 0
    const uint32_t* edges;      // DEVICE [n_win + 1]
    const Rule* rules;          // DEVICE [n_rules]
    uint2* prefix;              // scratch [n][tick_cap]: (PT, PB)
    uint32_t *total, *bad, *firing;   // [n][tick_cap] or null
    uint32_t* count;            // [n][W] or null
    uint32_t *fired, *episodes, *longest, *longest_start, *first, *last;   // [n][W][R] or null
    uint32_t *members, *fired_members, *open_members;                      // [G][W][R] or null
    unsigned long long *fire_ticks, *fire_episodes;                        // [G][W][R] or null
    uint32_t* delay_hist;       // [G][W][R][n_bins] or null
};

// W: the engine's wave primitives (scan_incl_u32, the DPP scan).
template <class W>
__global__ void __launch_bounds__(kThreads) af_alerts_prefix_kernel(const AlArgs a) {
    extern __shared__ uint32_t afal_lds[];   // [kChunkTicks] completions per tick, [kChunkTicks] bad ones behind
    __shared__ uint32_t wave_tot[kWaves], wave_bad[kWaves];
    uint32_t* tt = afal_lds;
    uint32_t* bd = afal_lds + kChunkTicks;
    const uint32_t s = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t m = a.counts[(size_t)s * 8u + a.cnt_completed_slot];
    m = m < a.clock_cap ? m : a.clock_cap;
    uint32_t t_s = a.counts[(size_t)s * 8u + a.cnt_ticks_slot];
    t_s = t_s < a.tick_cap ? t_s : a.tick_cap;
    const double2* ck = reinterpret_cast<const double2*>(a.clock) + (size_t)s * a.clock_cap;
    const size_t row = (size_t)s * a.tick_cap;
    uint32_t ct = 0u, cb = 0u;   // the prefix at the previous tile's last tick
    for (uint32_t c0 = 0u; c0 < t_s; c0 += kChunkTicks) {   // (uniform; t_s <= tick_cap < 2^31: no wrap)
        const uint32_t c1 = t_s - c0 < kChunkTicks ? t_s : c0 + kChunkTicks, len = c1 - c0;
        for (uint32_t k = tid; k < len; k += kThreads) tt[k] = bd[k] = 0u;
        __syncthreads();
        for (uint32_t base = 0u; base < m; base += kThreads * kUnroll) {   // (m <= clock_cap; the engine keeps n * clock_cap rows addressable)
            double2 c[kUnroll];
#pragma unroll
            for (uint32_t u = 0; u < kUnroll; ++u) {
                const uint32_t i = base + u * kThreads + tid;
                c[u] = i < m && i >= base ? ck[i] : double2{0.0, -1.0};   // (a row that is not counted; i >= base: no wrap)
            }
#pragma unroll
            for (uint32_t u = 0; u < kUnroll; ++u) {
                uint32_t f;
                bool is_bad;
                if (!row_tick(c[u].x, c[u].y, a.period, a.slo, t_s, f, is_bad) || f < c0 || f >= c1) continue;
                atomicAdd(&tt[f - c0], 1u);
                if (is_bad) atomicAdd(&bd[f - c0], 1u);
            }
            if (m - base <= kThreads * kUnroll) break;   // (base + kThreads * kUnroll could wrap)
        }
        __syncthreads();
        for (uint32_t t0 = 0u; t0 < len; t0 += kThreads) {   // (uniform: the scan and the barriers are block-wide)
            const uint32_t k = t0 + tid;
            const uint32_t tv = k < len ? tt[k] : 0u, bv = k < len ? bd[k] : 0u;
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
            }
            __syncthreads();   // (wave_tot and wave_bad are written again)
        }
        if (c1 == t_s) break;  // (the barrier above also stands before the next chunk's clearing)
    }
}

// the cells of window w (ticks [lo, hi)) of scenario s: lane r stores rule r's and adds it to the group's
__device__ __forceinline__ void store_cells(const AlArgs& a, const Cell& c, uint32_t s, uint32_t g, uint32_t w, uint32_t lo, uint32_t hi,
                                            uint32_t lane) {
    const uint32_t R = a.n_rules;
    if (lane == 0u && a.count) a.count[(size_t)s * a.n_win + w] = hi - lo;
    if (lane >= R) return;
    const size_t o = ((size_t)s * a.n_win + w) * R + lane;
    if (a.fired) a.fired[o] = c.fired;
    if (a.episodes) a.episodes[o] = c.episodes;
    if (a.longest) a.longest[o] = c.longest;
    if (a.longest_start) a.longest_start[o] = c.longest_start;
    if (a.first) a.first[o] = c.first;
    if (a.last) a.last[o] = c.last;
    if (g == kSkip || hi <= lo) return;
    const size_t cell = ((size_t)g * a.n_win + w) * R + lane;
    if (a.members) atomicAdd(&a.members[cell], 1u);
    if (c.first == kNone) return;   // (nothing fired: every other sum gets 0)
    if (a.fired_members) atomicAdd(&a.fired_members[cell], 1u);
    if (a.open_members && c.last == hi - 1u) atomicAdd(&a.open_members[cell], 1u);
    if (a.fire_ticks) atomicAdd(&a.fire_ticks[cell], (unsigned long long)c.fired);
    if (a.fire_episodes) atomicAdd(&a.fire_episodes[cell], (unsigned long long)c.episodes);
    if (a.delay_hist) atomicAdd(&a.delay_hist[cell * a.n_bins + delay_bin(c.first, lo, a.delay_width, a.n_bins)], 1u);
}

__global__ void __launch_bounds__(kEvalThreads) af_alerts_eval_kernel(const AlArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t s = blockIdx.x * kEvalWaves + (threadIdx.x >> 6);
    if (s >= a.n_scen) return;                                   // (a whole wave)
    const uint32_t g = a.group ? a.group[s] : 0u;
    uint32_t t_s = a.counts[(size_t)s * 8u + a.cnt_ticks_slot];
    t_s = t_s < a.tick_cap ? t_s : a.tick_cap;
    const size_t row = (size_t)s * a.tick_cap;
    const uint2* P = a.prefix + row;
    const uint32_t R = a.n_rules, W = a.n_win;
    const uint32_t my_hold = lane < R ? a.rules[lane].hold_ticks : 1u;
    uint32_t run = 0u, w = 0u;                                   // (w: uniform)
    Cell c;
    cell_reset(c);
    for (uint32_t k0 = 0u; k0 < t_s; k0 += 64u) {                // (uniform; t_s < 2^31: no wrap)
        const uint32_t k_end = t_s - k0 < 64u ? t_s : k0 + 64u, k = k0 + lane;
        const bool on = k < k_end;
        const uint2 pk = on ? P[k] : uint2{0u, 0u};
        uint64_t cond = 0ull;                                    // lane r: the condition mask of rule r
        for (uint32_t r = 0u; r < R; ++r) {                      // (uniform)
            const Rule ru = a.rules[r];
            const bool hl = on && k >= ru.long_ticks, hs = on && k >= ru.short_ticks;
            const uint2 pl = hl ? P[k - ru.long_ticks] : uint2{0u, 0u};
            const uint2 ps = ru.short_ticks == ru.long_ticks ? pl : hs ? P[k - ru.short_ticks] : uint2{0u, 0u};
            const bool is = on && alert_cond(ru, rolling(pk.x, pl.x, hl), rolling(pk.y, pl.y, hl), rolling(pk.x, ps.x, hs), rolling(pk.y, ps.y, hs));
            const uint64_t mask = __ballot(is);
            if (lane == r) cond = mask;
        }
        const uint64_t f = hold_step(cond, my_hold, run);        // lane r: the firing mask of rule r
        if (a.firing) {                                          // (uniform) lane l: bit r = rule r fires at tick k0 + l
            uint32_t word = 0u;
            for (uint32_t r = 0u; r < R; ++r) {
                const uint32_t f_lo = (uint32_t)__shfl((int)(uint32_t)f, (int)r, 64), f_hi = (uint32_t)__shfl((int)(uint32_t)(f >> 32), (int)r, 64);
                word |= ((lane < 32u ? f_lo >> lane : f_hi >> (lane - 32u)) & 1u) << r;
            }
            if (on) a.firing[row + k] = word;
        }
        while (w < W) {                                          // (uniform) the windows that meet the step
            const uint32_t e0 = a.edges[w], e1 = a.edges[w + 1u];
            const uint32_t lo = e0 < t_s ? e0 : t_s, hi = e1 < t_s ? e1 : t_s;
            const uint32_t wa = lo > k0 ? lo : k0, wb = hi < k_end ? hi : k_end;
            if (wa < wb) cell_step(c, f & range_mask(wa - k0, wb - k0), k0, wa, wb);
            if (hi > k_end) break;                               // the window goes on in the next step
            store_cells(a, c, s, g, w, lo, hi, lane);
            cell_reset(c);
            ++w;
        }
    }
    for (; w < W; ++w) {                                         // (without ticks: every window is empty)
        const uint32_t e0 = a.edges[w], e1 = a.edges[w + 1u];
        store_cells(a, c, s, g, w, e0 < t_s ? e0 : t_s, e1 < t_s ? e1 : t_s, lane);
    }
}
#endif  // __HIPCC__

}  // namespace afal
