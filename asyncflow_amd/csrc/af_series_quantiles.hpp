// Exact quantiles of the sampled series per (group, window of ticks, series) (af_engine_summarize_series_quantiles).
// The cells are af_series_windows.hpp's: window w of scenario s is its sample rows [min(b[w], m_s), min(b[w + 1], m_s)), the
// sample of (g, w, j) is column j of those rows of every member of g; rows at or past m_s and padding words are never read.
// Every word has a 32-bit KEY that orders like its value -- the word itself, or afs::float_key of a ram_in_use word (-0.0 below
// +0.0) --; a quantile is afs::lerp between two order statistics (afs::level_ranks) of the keys, converted back to f64 only
// where a cell is written.  Nothing is ever added across elements but integer counts.
//   small     a cell of at most kSmallMax values per column: a workgroup per (cell, 16-byte column group that holds a selected
//             column) gathers the group's selected columns from its members' rows into LDS (one array per SELECTED column),
//             sorts them there (bitonic, all arrays in step) and reads each level's two order statistics
//   large     every other cell, a CHUNK of cells at a time (the host sizes a chunk to the histogram budget).  The row walk of
//             af_swin_partial -- a wave per (scenario, run of windows), a lane stays on its four columns, consecutive lanes read
//             consecutive 16 bytes -- streams the chunk's rows once per pass:
//               bounds    min / max key per (cell, selected column): atomicMin / atomicMax on u32
//               level 0   the top <= 11 bits of key - minkey into ONE histogram per (cell, column).  Where maxkey - minkey
//                         < 2^11 -- nearly every integer series -- that is the whole key and the column is done
//               level 1+  the next <= 11 bits of the elements under a wanted rank's prefix, one histogram per distinct prefix
//                         (slot) of the column; columns whose key is complete, and lanes without such a column, read nothing
//             after each level a workgroup per (cell, column) finds every rank's bin (afs::wave_select) and names the slots of
//             the next, whose histograms it clears (the host clears level 0's one per pair); 32 key bits are at most three
//             levels.  A lane adds a RUN of equal bins with one atomic.
//             final     a thread per (cell, column, level) interpolates and writes
// No kernel waits for another workgroup; integer vector atomics only, so a cell's result does not depend on scheduling, the
// launch, the batch a scenario sits in, or which other cells, levels and columns the call holds.  Unselected columns cost no
// LDS, scratch or atomics; their bytes come with the 16-byte load of a row.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "af_select.hpp"
#include "af_series_windows.hpp"

namespace afsq {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr uint32_t kSmallMax = 2048;   // values per column that the small tier sorts in LDS
constexpr int kBits = 11;              // key bits per level of the large tier
constexpr uint32_t kBins = 1u << kBits;
constexpr uint32_t kMaxRanks = 32;     // two per level: 2 * AF_MAX_SERIES_QUANTILE_LEVELS
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kUnroll = 4;        // 16-byte loads a lane has in flight

struct SqArgs {
    const uint32_t* samples;   // [n][tick_cap][pitch]
    const uint32_t* counts;    // [n][8]
    uint32_t tick_cap, pitch, n_series, n_edges, cnt_ticks_slot;
    const uint32_t* group;     // [n] or null (all in group 0)
    uint32_t n_scen, n_groups, n_win;
    uint32_t run;              // windows per work item of the row walk
    const uint32_t* edges;     // [W + 1]
    const uint32_t* mem_off;   // [G + 1] into members
    const uint32_t* members;   // the scenarios of group 0, of group 1, ... each ascending
    uint32_t n_lev, n_out, n_uniq, n_ranks;   // Q, output columns C, distinct selected series U, R = 2 Q
    const double* levels;      // [Q]
    const uint32_t* u_of;      // [pitch] series -> its index among the distinct selected ones, or kNone
    const uint32_t* u_series;  // [U] ascending
    const uint32_t* head;      // [U] the first output column of a distinct series
    const uint32_t* next;      // [C] the next output column of the same series, or kNone
    // small tier
    const uint32_t* small_cells;   // [n_small][2] cell index, values per column (the host sized every cell to route it)
    const uint32_t* sel_groups;    // [n_sg] the 16-byte column groups that hold a selected column, ascending
    uint32_t n_sg, lds_stride;     // lds_stride: words per LDS array (a power of two >= every small cell)
    // large tier
    const uint32_t* cell_lidx;     // [G * W] index among the large cells, or kNone
    const uint32_t* lcell;         // [n_large] cell index
    const uint32_t* lcell_n;       // [n_large] values per column
    uint32_t l0, l1;               // the chunk: large cells [l0, l1); pair p = (lidx - l0) * U + u
    uint32_t *bmin, *bmax;         // [pairs] key bounds
    uint32_t *pfx, *rank_in, *slot_of, *slot_pfx;   // [pairs][R]
    uint32_t* n_slots;             // [pairs]
    uint32_t* hist;                // [pairs][R][kBins]
    uint32_t* count;               // [G][W] or null
    double* quant;                 // [G][W][C][Q]
};

__device__ __forceinline__ uint32_t stored_ticks(const SqArgs& a, uint32_t s) {
    const uint32_t m = a.counts[(size_t)s * 8u + a.cnt_ticks_slot];
    return m < a.tick_cap ? m : a.tick_cap;
}
__device__ __forceinline__ uint32_t key_of(uint32_t w, bool is_f) { return is_f ? afs::float_key(w) : w; }
__device__ __forceinline__ double value_of(uint32_t key, bool is_f) {
    return is_f ? (double)__uint_as_float(afs::float_unkey(key)) : (double)key;
}
__device__ __forceinline__ uint32_t key_width(uint32_t mn, uint32_t mx) { return mx > mn ? 32u - (uint32_t)__clz((int)(mx - mn)) : 0u; }
// key bits still unknown BEFORE level `level` of a column whose keys span `width` bits
__device__ __forceinline__ uint32_t shift_before(uint32_t width, int level) {
    const uint32_t used = (uint32_t)(kBits * level);
    return width > used ? width - used : 0u;
}

// the quantile of level q from the keys of its two order statistics, into every output column of series j
__device__ __forceinline__ void write_level(const SqArgs& a, uint64_t cell, uint32_t u, uint32_t l, uint32_t n, uint32_t klo, uint32_t khi,
                                            bool is_f) {
    uint32_t lo, hi;
    double t;
    afs::level_ranks(n, a.levels[l], lo, hi, t);
    const double v = afs::lerp(value_of(klo, is_f), value_of(khi, is_f), t);
    for (uint32_t c = a.head[u]; c != kNone; c = a.next[c]) a.quant[(cell * a.n_out + c) * a.n_lev + l] = v;
}

// ---- small cells ----
__global__ __launch_bounds__(kThreads) void af_sq_small(SqArgs a, uint64_t item0) {
    extern __shared__ uint32_t keys[];   // [selected columns of the group][lds_stride]
    const uint32_t tid = threadIdx.x;
    const uint64_t item = item0 + blockIdx.x;
    const uint64_t cell = a.small_cells[2u * (item / a.n_sg)];
    const uint32_t n = a.small_cells[2u * (item / a.n_sg) + 1u];   // (at most lds_stride)
    const uint32_t sg = (uint32_t)(item % a.n_sg), cg = a.sel_groups[sg];
    const uint32_t W = a.n_win, S = a.n_series, pq = a.pitch / 4u, Q = a.n_lev;
    const uint32_t g = (uint32_t)(cell / W), w = (uint32_t)(cell % W);
    const uint32_t b0 = a.edges[w], b1 = a.edges[w + 1u];
    const uint32_t k0 = a.mem_off[g], k1 = a.mem_off[g + 1u];
    uint32_t u[4], slot[4], n_slots = 0;
    bool is_f[4];
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint32_t j = cg * 4u + k;
        u[k] = j < S ? a.u_of[j] : kNone;
        is_f[k] = afs::series_is_float(j, a.n_edges, S);
        slot[k] = n_slots;
        n_slots += u[k] != kNone ? 1u : 0u;
    }
    uint32_t pad = 1u;
    while (pad < n) pad <<= 1;
    const uint32_t stride = a.lds_stride;
    const uint4* rows = reinterpret_cast<const uint4*>(a.samples);
    uint32_t base = 0;
    for (uint32_t k = k0; k < k1; ++k) {
        const uint32_t s = a.members[k], m = stored_ticks(a, s);
        const uint32_t r0 = b0 < m ? b0 : m, r1 = b1 < m ? b1 : m;
        for (uint32_t r = r0 + tid; r < r1; r += kThreads) {
            const uint4 v = rows[((size_t)s * a.tick_cap + r) * pq + cg];
            const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (uint32_t c = 0; c < 4u; ++c)
                if (u[c] != kNone) keys[slot[c] * stride + base + (r - r0)] = key_of(wd[c], is_f[c]);
        }
        base += r1 - r0;
    }
    for (uint32_t i = n + tid; i < pad; i += kThreads)
        for (uint32_t q = 0; q < n_slots; ++q) keys[q * stride + i] = 0xFFFFFFFFu;
    __syncthreads();
    for (uint32_t kk = 2u; kk <= pad; kk <<= 1)
        for (uint32_t jj = kk >> 1; jj > 0u; jj >>= 1) {
            for (uint32_t i = tid; i < pad; i += kThreads) {
                const uint32_t x = i ^ jj;
                if (x <= i) continue;
                const bool up = (i & kk) == 0u;
                for (uint32_t q = 0; q < n_slots; ++q) {
                    const uint32_t lo = keys[q * stride + i], hi = keys[q * stride + x];
                    if ((lo > hi) == up) {
                        keys[q * stride + i] = hi;
                        keys[q * stride + x] = lo;
                    }
                }
            }
            __syncthreads();
        }
    if (sg == 0u && tid == 0u && a.count) a.count[cell] = n;
    if (tid >= Q) return;
    const uint32_t l = tid;   // a thread per level
#pragma unroll
    for (uint32_t c = 0; c < 4u; ++c) {
        if (u[c] == kNone) continue;
        if (n == 0u) {
            for (uint32_t oc = a.head[u[c]]; oc != kNone; oc = a.next[oc]) a.quant[(cell * a.n_out + oc) * Q + l] = __builtin_nan("");
            continue;
        }
        uint32_t lo, hi;
        double tt;
        afs::level_ranks(n, a.levels[l], lo, hi, tt);
        write_level(a, cell, u[c], l, n, keys[slot[c] * stride + lo], keys[slot[c] * stride + hi], is_f[c]);
    }
}

// ---- large cells ----
// what a lane keeps of one column of the window it walks
struct LaneCol {
    uint32_t p = kNone;                     // the pair, kNone: nothing to do for this column
    uint32_t mn = 0xFFFFFFFFu, mx = 0u;     // bounds: the lane's own; levels: the pair's minimum key in mn
    uint32_t sprev = 0, snew = 0, ns = 0;   // levels: the shifts before and after this level, the slots
    uint32_t last_hi = 0, last_q = kNone;   // the slot of the last prefix looked up
    size_t cur = 0;                         // a run of equal histogram entries
    uint32_t cnt = 0;
};

// MODE 0: bounds; 1: level 0; 2: a deeper level
template <int MODE>
__global__ __launch_bounds__(kThreads) void af_sq_rows(SqArgs a, int level) {
    const int lane = threadIdx.x & 63;
    const uint32_t W = a.n_win;
    const uint32_t runs = (W + a.run - 1u) / a.run;
    const uint64_t item = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (item >= (uint64_t)a.n_scen * runs) return;
    const uint32_t s = (uint32_t)(item / runs), w0 = (uint32_t)(item % runs) * a.run;
    const uint32_t w1 = W - w0 < a.run ? W : w0 + a.run;
    const uint32_t g = a.group ? a.group[s] : 0u;
    if (g == kNone || g >= a.n_groups) return;
    const uint32_t m = stored_ticks(a, s);
    const uint32_t pq = a.pitch / 4u;
    const uint32_t L = pq < 64u ? pq : 64u;
    const uint32_t rps = 64u / L;
    const uint32_t row_off = (uint32_t)lane / L;
    const bool lane_on = row_off < rps;
    const uint4* rows = reinterpret_cast<const uint4*>(a.samples) + (size_t)s * a.tick_cap * pq;
    const uint32_t S = a.n_series, U = a.n_uniq, R = a.n_ranks;
    for (uint32_t cg0 = 0; cg0 < pq; cg0 += 64u) {
        const uint32_t cg = cg0 + (uint32_t)lane % L;
        const bool on = lane_on && cg < pq;
        uint32_t u[4];
        bool is_f[4], any = false;
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            const uint32_t j = cg * 4u + k;
            u[k] = on && j < S ? a.u_of[j] : kNone;
            is_f[k] = afs::series_is_float(j, a.n_edges, S);
            any = any || u[k] != kNone;
        }
        if (!any) continue;
        for (uint32_t w = w0; w < w1; ++w) {
            const uint32_t lidx = a.cell_lidx[(size_t)g * W + w];
            if (lidx < a.l0 || lidx >= a.l1) continue;   // (kNone: a small cell)
            uint32_t r0 = a.edges[w], r1 = a.edges[w + 1u];
            r0 = r0 < m ? r0 : m;
            r1 = r1 < m ? r1 : m;
            LaneCol c[4];
            bool work = false;
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) {
                if (u[k] == kNone) continue;
                const uint32_t p = (lidx - a.l0) * U + u[k];
                if (MODE == 0) {
                    c[k].p = p;
                } else {
                    const uint32_t mn = a.bmin[p], width = key_width(mn, a.bmax[p]);
                    const uint32_t sprev = shift_before(width, level);
                    if (sprev == 0u) continue;   // every key bit of the column is known
                    c[k].p = p;
                    c[k].mn = mn;
                    c[k].sprev = sprev;
                    c[k].snew = shift_before(width, level + 1);
                    c[k].ns = MODE == 2 ? a.n_slots[p] : 1u;
                }
                work = true;
            }
            if (!work) continue;
            for (uint32_t r = r0 + row_off; r < r1; r += kUnroll * rps) {
                uint4 v[kUnroll];
#pragma unroll
                for (uint32_t q = 0; q < kUnroll; ++q)   // (r1 <= tick_cap < 2^31: no wrap)
                    v[q] = r + q * rps < r1 ? rows[(size_t)(r + q * rps) * pq + cg] : uint4{};
#pragma unroll
                for (uint32_t q = 0; q < kUnroll; ++q) {
                    if (r + q * rps >= r1) continue;
                    const uint32_t wd[4] = {v[q].x, v[q].y, v[q].z, v[q].w};
#pragma unroll
                    for (uint32_t k = 0; k < 4u; ++k) {
                        LaneCol& x = c[k];
                        if (x.p == kNone) continue;
                        const uint32_t key = key_of(wd[k], is_f[k]);
                        if (MODE == 0) {
                            x.mn = key < x.mn ? key : x.mn;
                            x.mx = key > x.mx ? key : x.mx;
                            continue;
                        }
                        const uint32_t d = key - x.mn;
                        uint32_t slot = 0u;
                        if (MODE == 2) {
                            const uint32_t hi = d >> x.sprev;   // (sprev <= 21)
                            if (x.last_q == kNone || hi != x.last_hi) {
                                x.last_hi = hi;
                                x.last_q = kNone - 1u;   // looked up, under no wanted prefix
                                for (uint32_t q2 = 0; q2 < x.ns; ++q2)
                                    if (a.slot_pfx[(size_t)x.p * R + q2] == hi) x.last_q = q2;
                            }
                            if (x.last_q == kNone - 1u) continue;
                            slot = x.last_q;
                        }
                        const uint32_t bin = (d >> x.snew) & ((1u << (x.sprev - x.snew)) - 1u);   // (at most kBits bits)
                        const size_t idx = ((size_t)x.p * R + slot) * kBins + bin;
                        if (x.cnt != 0u && idx == x.cur) {
                            x.cnt += 1u;
                        } else {
                            if (x.cnt != 0u) atomicAdd(&a.hist[x.cur], x.cnt);
                            x.cur = idx;
                            x.cnt = 1u;
                        }
                    }
                }
            }
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) {
                if (c[k].p == kNone) continue;
                if (MODE == 0) {
                    if (c[k].mn <= c[k].mx) {
                        atomicMin(&a.bmin[c[k].p], c[k].mn);
                        atomicMax(&a.bmax[c[k].p], c[k].mx);
                    }
                } else if (c[k].cnt != 0u) {
                    atomicAdd(&a.hist[c[k].cur], c[k].cnt);
                }
            }
        }
    }
}

// a workgroup per (cell, column) of the chunk, after the histograms of `level`: every rank's bin; the slots of the next level
__global__ __launch_bounds__(kThreads) void af_sq_select(SqArgs a, int level) {
    __shared__ uint32_t s_pfx[kMaxRanks], s_rank[kMaxRanks], s_slot[kMaxRanks], s_ns;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t p = blockIdx.x, R = a.n_ranks;
    const uint32_t n = a.lcell_n[a.l0 + p / a.n_uniq];
    const uint32_t width = key_width(a.bmin[p], a.bmax[p]);
    if (tid < R) {
        if (level == 0) {
            uint32_t lo, hi;
            double t;
            afs::level_ranks(n, a.levels[tid >> 1], lo, hi, t);
            s_pfx[tid] = 0u;
            s_rank[tid] = (tid & 1u) ? hi : lo;
            s_slot[tid] = 0u;
        } else {
            s_pfx[tid] = a.pfx[(size_t)p * R + tid];
            s_rank[tid] = a.rank_in[(size_t)p * R + tid];
            s_slot[tid] = a.slot_of[(size_t)p * R + tid];
        }
    }
    __syncthreads();
    const uint32_t sprev = shift_before(width, level), snew = shift_before(width, level + 1);
    if (sprev != 0u) {
        for (uint32_t r = wave; r < R; r += (uint32_t)kWaves) {
            uint32_t bin, below, count;
            afs::wave_select(a.hist + ((size_t)p * R + s_slot[r]) * kBins, (int)kBins, s_rank[r], bin, below, count);
            if (lane == 0u) {
                s_pfx[r] = (s_pfx[r] << (sprev - snew)) | bin;   // (at most kBits bits a level, `width` <= 32 in all)
                s_rank[r] -= below;
            }
        }
        __syncthreads();
        if (tid == 0u && snew != 0u) {   // the distinct prefixes become the slots of the next level
            uint32_t ns = 0;
            for (uint32_t r = 0; r < R; ++r) {
                uint32_t q = 0;
                while (q < ns && a.slot_pfx[(size_t)p * R + q] != s_pfx[r]) ++q;
                if (q == ns) a.slot_pfx[(size_t)p * R + ns++] = s_pfx[r];
                s_slot[r] = q;
            }
            a.n_slots[p] = ns;
            s_ns = ns;
        }
        __syncthreads();
        // the histograms of the next level's slots, empty: every wave has read this level's (the barrier above), and the
        // slots of a pair lie side by side.  A column that is done leaves its histograms as they are: nobody reads them
        if (snew != 0u) {
            uint32_t* h = a.hist + (size_t)p * R * kBins;
            for (uint32_t i = tid; i < s_ns * kBins; i += (uint32_t)kThreads) h[i] = 0u;
        }
    }
    if (tid < R && (level == 0 || sprev != 0u)) {
        a.pfx[(size_t)p * R + tid] = s_pfx[tid];
        a.rank_in[(size_t)p * R + tid] = s_rank[tid];
        a.slot_of[(size_t)p * R + tid] = s_slot[tid];
    }
}

// a thread per (cell, column, level) of the chunk: a rank's key is the column's minimum key + its prefix
__global__ __launch_bounds__(kThreads) void af_sq_final(SqArgs a, uint64_t n_entries) {
    const uint64_t idx = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= n_entries) return;
    const uint32_t Q = a.n_lev, R = a.n_ranks, U = a.n_uniq;
    const uint32_t p = (uint32_t)(idx / Q), l = (uint32_t)(idx % Q);
    const uint32_t lidx = a.l0 + p / U, u = p % U;
    const uint64_t cell = a.lcell[lidx];
    const uint32_t n = a.lcell_n[lidx], mn = a.bmin[p];
    if (u == 0u && l == 0u && a.count) a.count[cell] = n;
    const bool is_f = afs::series_is_float(a.u_series[u], a.n_edges, a.n_series);
    write_level(a, cell, u, l, n, mn + a.pfx[(size_t)p * R + 2u * l], mn + a.pfx[(size_t)p * R + 2u * l + 1u], is_f);
}

}  // namespace afsq
