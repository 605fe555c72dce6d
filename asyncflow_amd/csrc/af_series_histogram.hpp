// Occupancy histograms of the sampled series per (group, window of ticks, output column): P(queue length = k) per window and
// grid point (af_engine_summarize_series_histogram).
// The cells are af_series_windows.hpp's: window w of scenario s is its sample rows [min(b[w], m_s), min(b[w + 1], m_s)), m_s =
// min(counts[s][ticks], tick_cap); rows at or past m_s and the padding words of a row are never read.  Output column c reads
// series columns[c] with its own binning (lo[c], width[c]):  x = the value as f64 ((double)word, or (double)(float) of a
// ram_in_use word);  x < lo -> under;  t = (x - lo) / width (one f64 subtraction, one f64 division);  t >= n_bins -> over;
// else bin (uint32_t)t.  An integer series with lo = 0 and width = 1 takes the word itself as its bin: no division.
//   The host sorts the output columns by series into SLOTS (slot q reads series j for first[j] <= q < first[j + 1]) and cuts
//   the slots into CHUNKS of at most kWaveLdsWords / (n_bins + 2) in which no series appears twice (a series requested once
//   more, with another binning, starts a chunk) -- one pass over the needed 16-byte groups per chunk.
//   a WAVE per (scenario, run of consecutive windows), one window at a time, with af_series_excursions.hpp's mapping of rows
//   to lanes: pq = pitch / 4 16-byte groups per row, L = min(pq, 64) lanes a row, R = 64 / L rows a STEP; lane l holds group
//   l % L of row base + l / L (plans of more than 64 groups: 64 groups per pass).  A lane loads its group only if a slot of
//   the chunk reads one of its four series: 16 bytes a lane, four steps in flight.
//   LDS: every wave has a histogram of its own, (n_bins + 2) words per slot of the chunk -- the bins, under, over.  BUDGET:
//   kWaveLdsWords = 4 096 words = 16 KiB a wave, 64 KiB a block of four waves at the most, so two such blocks fit the 160 KiB
//   of a CU; a call asks only for what its chunk needs (12 slots x 66 words x 4 waves = 12.4 KiB: LDS does not bound the
//   occupancy of the default binning).  1 024 bins: three slots a chunk.
//   Same-bin contention (a queue length is 0 in most ticks, and with 12 series 21 lanes of a wave hold the same column):
//     agreement   the lanes of a column compare their bin with that of the column's first row of the step (one shuffle, one
//                 __ballot); the first row's lane adds the popcount of the agreeing lanes at once, a lane that disagrees adds 1.
//     run         every lane keeps (bin, length) of what it has to add per column in registers and adds to memory only when
//                 the bin changes or the window ends: a column constant over a window costs one add per window.
//   Tiny windows: a window of at most kTinyRows rows neither clears nor flushes an LDS histogram -- its (few) runs are added
//   to the cell in HBM directly; a longer window clears its slots, counts in LDS and adds the non-zero words to the cell.
//   (The two forms of a window are two instances of one function: LDS adds are ds_add_u32, HBM adds global_atomic_add.)
//   The entry zeroes the outputs first; every addition to a cell is an integer atomic.
// Every combining operation is an integer +: the result cannot depend on the launch, on the batch a scenario sits in, on which
// other columns the call holds, or on the run.
// Scratch (engine-owned, shared with the other analyzers): 4 B per edge + 4 B per series + 24 B per output column + 8 B (+ up to
// 256 B of alignment for each of the six parts).  No per-element and no per-cell records.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "af_summary.hpp"

namespace afsh {

constexpr int kThreads = 256;               // four waves, four work items
constexpr int kWaves = kThreads / 64;
constexpr uint32_t kUnroll = 4;             // 16-byte loads a lane has in flight
constexpr uint32_t kSkip = 0xFFFFFFFFu;     // AF_POOL_SKIP
constexpr uint32_t kMaxBins = 1024;         // AF_MAX_SERIES_HISTOGRAM_BINS
constexpr uint32_t kWaveLdsWords = 4096;    // the LDS histogram of one wave, in words
constexpr uint32_t kTinyRows = 32;          // windows of at most this many rows add to HBM directly
constexpr uint32_t kNone = 0xFFFFFFFFu;
static_assert(kMaxBins + 2u <= kWaveLdsWords, "one slot must fit the LDS of a wave");

struct ShArgs {
    const uint32_t* samples;   // [n][tick_cap][pitch]
    const uint32_t* counts;    // [n][8]
    uint32_t tick_cap, pitch, n_series, n_edges, cnt_ticks_slot;
    const uint32_t* group;     // [n], or null: all in group 0
    uint32_t n_scen, n_win;
    uint32_t run;              // windows per work item
    const uint32_t* edges;     // [W + 1]
    uint32_t n_out;            // output columns = slots
    uint32_t n_bins;
    uint32_t n_chunks;
    uint32_t lds_slots;        // the slots of the largest chunk: a wave's LDS is lds_slots * (n_bins + 2) words
    const uint32_t* cstart;    // [n_chunks + 1] the slots of chunk k: cstart[k] .. cstart[k + 1] - 1, no series twice
    const uint32_t* first;     // [n_series + 1] the slots of series j: first[j] .. first[j + 1] - 1
    const uint32_t* scol;      // [n_out] the output column of a slot
    const double* slo;         // [n_out] lo of a slot
    const double* swidth;      // [n_out] width of a slot
    uint32_t* count;           // [G][W], or null
    uint32_t* hist;            // [G][W][n_out][n_bins]
    uint32_t* under;           // [G][W][n_out], or null
    uint32_t* over;            // [G][W][n_out], or null
};

// the entry of a value in a slot's (n_bins + 2) words: its bin, n_bins for under, n_bins + 1 for over
__device__ __forceinline__ uint32_t entry_of(uint32_t word, bool is_f, bool plain, double lo, double width, uint32_t B) {
    if (plain) return word < B ? word : B + 1u;
    const double x = is_f ? (double)__uint_as_float(word) : (double)word;
    if (x < lo) return B;
    const double t = (x - lo) / width;
    if (t >= (double)B) return B + 1u;
    const uint32_t b = (uint32_t)t;
    return b < B ? b : B + 1u;   // (t is in [0, B) here; a NaN, which no series holds, must not leave the slot)
}

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// n values of slot q in entry e of cell `cell`, to HBM
__device__ __forceinline__ void add_cell(const ShArgs& a, size_t cell, uint32_t q, uint32_t e, uint32_t n) {
    const size_t o = cell * a.n_out + a.scol[q];
    if (e < a.n_bins) atomicAdd(&a.hist[o * a.n_bins + e], n);
    else if (e == a.n_bins) {
        if (a.under) atomicAdd(&a.under[o], n);
    } else if (a.over) atomicAdd(&a.over[o], n);
}

// where a lane stands in its wave
struct Geo {
    const uint4* rows;          // the scenario's sample rows
    uint32_t pq, rps, row_off, cgl;
    bool leader;                // the first row of a step
    unsigned long long colmask; // the lanes that hold this lane's column group
    int lane;
};

// what a lane keeps for one chunk of slots and one pass over the groups
struct Pass {
    uint32_t cg;                // its 16-byte group
    bool load;                  // the chunk reads one of the group's series
    uint32_t q[4];              // the chunk's slot of each of them; kNone: none
    bool is_f[4], plain[4];
    double lo[4], wd[4];
};

// One window of one scenario, rows [r0, r1), r1 > r0: the chunk's slots [q0, q0 + words / E) into `cell`.
template <bool kTiny>
__device__ __forceinline__ void window(const ShArgs& a, const Geo& g, const Pass& p, uint32_t lbase, uint32_t q0, uint32_t words,
                                       size_t cell, uint32_t r0, uint32_t r1) {
    extern __shared__ uint32_t afsh_lds[];
    uint32_t* lh = afsh_lds + lbase;      // this wave's histogram
    const uint32_t B = a.n_bins, E = B + 2u;
    if (!kTiny) {
        for (uint32_t i = (uint32_t)g.lane; i < words; i += 64u) lh[i] = 0u;
        wave_sync();
    }
    // n values of slot q in entry e
    const auto add = [&](uint32_t q, uint32_t e, uint32_t n) {
        if (kTiny) add_cell(a, cell, q, e, n);
        else atomicAdd(&lh[(q - q0) * E + e], n);
    };
    uint32_t run_e[4] = {kNone, kNone, kNone, kNone}, run_n[4] = {0u, 0u, 0u, 0u};
    for (uint32_t r = r0; r < r1; r += kUnroll * g.rps) {   // (uniform; r1 <= tick_cap < 2^31: no wrap)
        uint4 v[kUnroll];
#pragma unroll
        for (uint32_t u = 0; u < kUnroll; ++u) {
            const uint32_t k = r + u * g.rps + g.row_off;
            v[u] = p.load && k < r1 ? g.rows[(size_t)k * g.pq + p.cg] : uint4{};
        }
#pragma unroll 1
        for (uint32_t u = 0; u < kUnroll; ++u) {             // (one copy of the body: it holds four f64 divisions)
            if (r + u * g.rps >= r1) break;                  // (uniform)
            const uint32_t k = r + u * g.rps + g.row_off;
            const bool live = p.load && k < r1;
            const uint32_t word[4] = {v[0].x, v[0].y, v[0].z, v[0].w};
            v[0] = v[1];                                     // (the next step moves up: no indexed register)
            v[1] = v[2];
            v[2] = v[3];
#pragma unroll
            for (uint32_t c = 0; c < 4u; ++c) {
                const bool has = live && p.q[c] != kNone;
                if (__ballot(has) == 0ull) continue;         // (uniform)
                const uint32_t e = has ? entry_of(word[c], p.is_f[c], p.plain[c], p.lo[c], p.wd[c], B) : kNone;
                // the column's first row of the step is live wherever one of its rows is
                const uint32_t e_first = (uint32_t)__shfl((int)e, (int)g.cgl, 64);
                const bool agree = has && e == e_first;
                const unsigned long long same = __ballot(agree) & g.colmask;
                const uint32_t n = g.leader ? (uint32_t)__popcll(same) : (has && !agree ? 1u : 0u);
                if (n) {
                    if (e == run_e[c]) run_n[c] += n;
                    else {
                        if (run_n[c]) add(p.q[c], run_e[c], run_n[c]);
                        run_e[c] = e;
                        run_n[c] = n;
                    }
                }
            }
        }
    }
#pragma unroll
    for (uint32_t c = 0; c < 4u; ++c)
        if (run_n[c]) add(p.q[c], run_e[c], run_n[c]);
    if (!kTiny) {
        wave_sync();
        for (uint32_t i = (uint32_t)g.lane; i < words; i += 64u) {
            const uint32_t n = lh[i];
            if (n) add_cell(a, cell, q0 + i / E, i % E, n);
        }
        wave_sync();   // (the next window clears these words)
    }
}

__global__ __launch_bounds__(kThreads) void af_shist_kernel(ShArgs a) {
    const int lane = threadIdx.x & 63;
    const uint32_t W = a.n_win, E = a.n_bins + 2u;
    const uint32_t lbase = (threadIdx.x >> 6) * a.lds_slots * E;
    const uint32_t items = (W + a.run - 1u) / a.run;   // work items per scenario
    const uint64_t item = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (item >= (uint64_t)a.n_scen * items) return;    // (a whole wave; there is no block-wide barrier below)
    const uint32_t s = (uint32_t)(item / items), w0 = (uint32_t)(item % items) * a.run;
    const uint32_t w1 = W - w0 < a.run ? W : w0 + a.run;
    const uint32_t grp = a.group ? a.group[s] : 0u;
    if (grp == kSkip) return;
    uint32_t m = a.counts[(size_t)s * 8u + a.cnt_ticks_slot];
    m = m < a.tick_cap ? m : a.tick_cap;
    Geo g;
    g.lane = lane;
    g.pq = a.pitch / 4u;
    const uint32_t L = g.pq < 64u ? g.pq : 64u;     // lanes per row
    g.rps = 64u / L;                                // rows per step of the wave
    g.row_off = (uint32_t)lane / L;
    g.cgl = (uint32_t)lane % L;
    const bool lane_on = g.row_off < g.rps;
    g.leader = g.row_off == 0u;
    g.colmask = 0ull;
    for (uint32_t r = 0; r < g.rps; ++r) g.colmask |= 1ull << (r * L + g.cgl);
    g.rows = reinterpret_cast<const uint4*>(a.samples) + (size_t)s * a.tick_cap * g.pq;
    const uint32_t S = a.n_series;
    const size_t cell0 = (size_t)grp * W;
    if (a.count)
        for (uint32_t w = w0 + (uint32_t)lane; w < w1; w += 64u) {
            const uint32_t e0 = a.edges[w], e1 = a.edges[w + 1u];
            const uint32_t c = (e1 < m ? e1 : m) - (e0 < m ? e0 : m);
            if (c) atomicAdd(&a.count[cell0 + w], c);
        }
    for (uint32_t ck = 0; ck < a.n_chunks; ++ck) {   // a chunk of slots: one pass over the groups it reads
        const uint32_t q0 = a.cstart[ck], q1 = a.cstart[ck + 1u];
        const uint32_t words = (q1 - q0) * E;
        for (uint32_t cg0 = 0; cg0 < g.pq; cg0 += 64u) {
            Pass p;
            p.cg = cg0 + g.cgl;
            const bool on = lane_on && p.cg < g.pq;
            p.load = false;
#pragma unroll
            for (uint32_t c = 0; c < 4u; ++c) {
                const uint32_t j = p.cg * 4u + c;
                p.q[c] = kNone;
                p.lo[c] = 0.0;
                p.wd[c] = 1.0;
                p.is_f[c] = afs::series_is_float(j, a.n_edges, S);
                if (on && j < S) {
                    const uint32_t f0 = a.first[j], f1 = a.first[j + 1u];
                    const uint32_t qa = f0 > q0 ? f0 : q0, qb = f1 < q1 ? f1 : q1;
                    if (qb > qa) {                  // (then qb == qa + 1: a chunk holds no series twice)
                        p.q[c] = qa;
                        p.lo[c] = a.slo[qa];
                        p.wd[c] = a.swidth[qa];
                        p.load = true;
                    }
                }
                p.plain[c] = !p.is_f[c] && p.lo[c] == 0.0 && p.wd[c] == 1.0;
            }
            if (__ballot(p.load) == 0ull) continue;   // (uniform: the chunk reads none of these groups)
            for (uint32_t w = w0; w < w1; ++w) {
                uint32_t r0 = a.edges[w], r1 = a.edges[w + 1u];
                r0 = r0 < m ? r0 : m;
                r1 = r1 < m ? r1 : m;
                if (r1 == r0) continue;             // (uniform)
                if (r1 - r0 <= kTinyRows) window<true>(a, g, p, lbase, q0, words, cell0 + w, r0, r1);
                else window<false>(a, g, p, lbase, q0, words, cell0 + w, r0, r1);
            }
        }
    }
}

}  // namespace afsh
