// The order statistics of the latency analyzers (af_summary.hpp, af_pooled.hpp, af_windowed.hpp, af_quantiles.hpp), once.
//
// All of them want a few RANKS of a sample of f64 latencies >= +0.0 -- the bit pattern of such a double, read as an integer
// (key_of), orders like its value -- and interpolate between two of them as numpy does (lerp).  The sample is never sorted:
//   level 0   a histogram of the keys' exponent field (bits 62..52, kExpBins bins); wave r finds the bin of wanted rank r
//             (select_first_level): the rank's PREFIX pfx[r] = key >> shift, its rank inside that bin, the bin's count
//   slots     ranks that share a prefix share a SLOT (assign_slots): one digit histogram and one candidate list per slot;
//             another level is needed while some rank's bin holds more than kCand elements and key bits are left
//   digits    the next kDigBits key bits of every element under a slot's prefix (count_digit) into that slot's histogram;
//             wave r finds its rank's digit, the prefix grows by it (select_digit_level): shift 52 -> 42 -> ... -> 2 -> 0
//   last      the elements under the slots' prefixes are the ranks' CANDIDATES (collect_candidate, at most kCand each); the
//             value of a rank is the candidate with as many smaller ones as the rank asks for (rank_values: by counting, so
//             the candidates' order does not matter); at shift 0 the prefix IS the value
// Every function takes plain pointers: the state lies in LDS where one workgroup owns the sample (af_summary_kernel,
// af_win_small) and in global memory (afp::PoolGroup) where a sample is spread over the chip (af_pool_*, af_q_*).
// Integer atomics only: the results do not depend on scheduling.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace afs {

constexpr int kThreads = 512;   // (1 024 threads, two scenarios per CU, in the hope of Infinity Cache hits in the second pass: 6.4 -> 6.7 ms)
constexpr int kWaves = kThreads / 64;
constexpr int kRanks = 6;       // median lo/hi, p95 lo/hi, p99 lo/hi
constexpr int kCand = 512;      // candidates per rank resolved in LDS
constexpr int kExpBins = 2048;  // level 0: bits 62..52 (latencies are >= +0.0, the sign bit is clear)
constexpr int kDigBits = 10;    // deeper levels: 10 key bits each
constexpr int kDigBins = 1 << kDigBits;

__device__ __forceinline__ unsigned long long key_of(double x) { return (unsigned long long)__double_as_longlong(x); }

__device__ __forceinline__ double lerp(double lo, double hi, double t) {   // numpy _lerp
    const double d = hi - lo;
    return t >= 0.5 ? hi - d * (1.0 - t) : lo + d * t;
}

// the ranks of np.median (the mean of the middle pair: want[0], want[1]) and np.percentile 95 / 99, 'linear' (want[2 + 2 p],
// want[3 + 2 p] and the weight tfrac[p] of the upper one) of n >= 1 elements
__device__ __forceinline__ void stat_ranks(uint32_t n, uint32_t* want, double* tfrac) {
    want[0] = (n & 1u) ? n / 2u : n / 2u - 1u;
    want[1] = n / 2u;
    const double q[2] = {95.0 / 100.0, 99.0 / 100.0};
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const double v = (double)(n - 1u) * q[p];
        if (v >= (double)(n - 1u)) {
            want[2 + 2 * p] = want[3 + 2 * p] = n - 1u;
            tfrac[p] = 0.0;
        } else {
            const double f = floor(v);
            want[2 + 2 * p] = (uint32_t)f;
            want[3 + 2 * p] = (uint32_t)f + 1u;
            tfrac[p] = v - f;
        }
    }
}

// np.quantile(a, q), 'linear', q in [0, 1]: the two order statistics it interpolates between, and the weight of the upper one
__device__ __forceinline__ void level_ranks(uint32_t n, double q, uint32_t& lo, uint32_t& hi, double& t) {
    const double v = (double)(n - 1u) * q;
    const double f = floor(v);
    lo = (uint32_t)f;
    hi = lo + 1u < n ? lo + 1u : n - 1u;
    t = v - f;
}

__device__ inline double wave_min(double v) {
    for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_down(v, off, 64));
    return v;
}
__device__ inline double wave_max(double v) {
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
    return v;
}

// minimum and maximum over the workgroup's threads, in every thread (red: LDS; holds one barrier)
__device__ __forceinline__ void block_min_max(double mn, double mx, double (*red)[kWaves], double& vmin, double& vmax) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    mn = wave_min(mn);
    mx = wave_max(mx);
    if (lane == 0) {
        red[0][wave] = mn;
        red[1][wave] = mx;
    }
    __syncthreads();
    vmin = red[0][0];
    vmax = red[1][0];
    for (int w = 1; w < kWaves; ++w) {
        vmin = fmin(vmin, red[0][w]);
        vmax = fmax(vmax, red[1][w]);
    }
}

// One wave finds the bin holding rank k of a histogram: bin, #elements below it, its count.
__device__ inline void wave_select(const uint32_t* hist, int nbins, uint32_t k, uint32_t& bin, uint32_t& below,
                                   uint32_t& count) {
    const int lane = threadIdx.x & 63;
    const int per = nbins / 64;
    uint32_t mine = 0;
    for (int j = 0; j < per; ++j) mine += hist[lane * per + j];
    uint32_t incl = mine;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t up = __shfl_up(incl, off, 64);
        if (lane >= off) incl += up;
    }
    const uint32_t excl = incl - mine;
    const bool owner = excl <= k && k < incl;
    uint32_t b = 0, bl = 0, c = 0;
    if (owner) {
        uint32_t run = excl;
        for (int j = 0; j < per; ++j) {
            const uint32_t h = hist[lane * per + j];
            if (k < run + h) {
                b = (uint32_t)(lane * per + j);
                bl = run;
                c = h;
                break;
            }
            run += h;
        }
    }
    const unsigned long long m = __ballot(owner);
    const int src = m ? __ffsll((long long)m) - 1 : 0;
    bin = __shfl(b, src, 64);
    below = __shfl(bl, src, 64);
    count = __shfl(c, src, 64);
}

// level 0, called by the whole workgroup: wave r < kRanks finds the exponent bin of wanted rank r
__device__ __forceinline__ void select_first_level(const uint32_t* hist, const uint32_t* want, uint64_t* pfx, uint32_t* rank_in, uint32_t* cnt) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (wave < kRanks) {
        uint32_t bin, below, count;
        wave_select(hist, kExpBins, want[wave], bin, below, count);
        if (lane == 0) {
            pfx[wave] = bin;
            rank_in[wave] = want[wave] - below;
            cnt[wave] = count;
        }
    }
}

// a digit level, called by the whole workgroup: wave r < kRanks finds rank r's next `bits` key bits in its slot's histogram
// (hist: [slots][kDigBins])
__device__ __forceinline__ void select_digit_level(const uint32_t* hist, int bits, const uint32_t* slot_of, uint64_t* pfx, uint32_t* rank_in,
                                                   uint32_t* cnt) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (wave < kRanks) {
        uint32_t bin, below, count;
        wave_select(hist + (size_t)slot_of[wave] * kDigBins, kDigBins, rank_in[wave], bin, below, count);
        if (lane == 0) {
            pfx[wave] = (pfx[wave] << bits) | bin;
            rank_in[wave] -= below;
            cnt[wave] = count;
        }
    }
}

// by ONE thread: the distinct prefixes become slots; another level while a rank has too many candidates and key bits are left
__device__ __forceinline__ void assign_slots(const uint64_t* pfx, const uint32_t* cnt, int shift, uint64_t* slot_pfx, uint32_t* slot_of,
                                             uint32_t* n_slots, uint32_t* more) {
    uint32_t ns = 0, m = 0;
    for (int r = 0; r < kRanks; ++r) {
        uint32_t sidx = ns;
        for (uint32_t q = 0; q < ns; ++q)
            if (slot_pfx[q] == pfx[r]) sidx = q;
        if (sidx == ns) slot_pfx[ns++] = pfx[r];
        slot_of[r] = sidx;
        if (cnt[r] > (uint32_t)kCand && shift > 0) m = 1u;
    }
    *n_slots = ns;
    *more = m;
}

// the slots' prefixes into registers; the rest a prefix no key >> shift (shift > 0) can equal: latencies are >= +0.0
__device__ __forceinline__ void load_slot_prefixes(uint64_t (&sp)[kRanks], const uint64_t* slot_pfx, uint32_t ns) {
#pragma unroll
    for (int q = 0; q < kRanks; ++q) sp[q] = (uint32_t)q < ns ? slot_pfx[q] : ~0ull;
}

// an element's next `bits` key bits (shift - bits = new_shift) into the histogram of the slot whose prefix it lies under
__device__ __forceinline__ void count_digit(unsigned long long key, int shift, int new_shift, int bits, const uint64_t (&sp)[kRanks], uint32_t* hist) {
    const unsigned long long hi = key >> shift;
#pragma unroll
    for (int q = 0; q < kRanks; ++q)
        if (hi == sp[q]) atomicAdd(&hist[q * kDigBins + (uint32_t)((key >> new_shift) & ((1u << bits) - 1u))], 1u);
}

// an element under a slot's prefix (shift > 0) is a candidate of that slot's ranks (cand: [slots][kCand])
__device__ __forceinline__ void collect_candidate(double x, int shift, const uint64_t (&sp)[kRanks], uint32_t* cand_n, double* cand) {
    const unsigned long long hi = key_of(x) >> shift;
#pragma unroll
    for (int q = 0; q < kRanks; ++q)
        if (hi == sp[q]) {
            const uint32_t pos = atomicAdd(&cand_n[q], 1u);
            if (pos < (uint32_t)kCand) cand[q * kCand + pos] = x;
        }
}

// called by the whole workgroup: val[r] (LDS) = the value of every rank among its slot's candidates (LDS), by counting
__device__ __forceinline__ void rank_values(const double* cand, const uint32_t* cand_n, const uint32_t* slot_of, const uint32_t* rank_in,
                                            const uint64_t* pfx, int shift, double* val) {
    const uint32_t tid = threadIdx.x;
    for (int r = 0; r < kRanks; ++r) {
        if (shift == 0) {   // the whole key is known: every candidate has this value
            if (tid == 0u) val[r] = __longlong_as_double((long long)pfx[r]);
            continue;
        }
        const uint32_t q = slot_of[r];
        const uint32_t m = cand_n[q] < (uint32_t)kCand ? cand_n[q] : (uint32_t)kCand;
        const uint32_t k = rank_in[r];
        if (tid < m) {
            const double x = cand[q * kCand + tid];
            uint32_t less = 0, leq = 0;
            for (uint32_t j = 0; j < m; ++j) {
                const double y = cand[q * kCand + j];
                less += y < x ? 1u : 0u;
                leq += y <= x ? 1u : 0u;
            }
            if (less <= k && k < leq) val[r] = x;
        }
    }
}

// by ONE thread: total, mean, median, std_dev, p95, p99, min, max from the values of stat_ranks' ranks and the sum sq of the
// squared deviations
__device__ __forceinline__ void write_stats_row(double* st, uint32_t n, double mean, double sq, const double* val, const double* tfrac, double vmin,
                                                double vmax) {
    st[0] = (double)n;
    st[1] = mean;
    st[2] = (n & 1u) ? val[1] : (val[0] + val[1]) / 2.0;
    st[3] = sqrt(sq / (double)n);
    st[4] = lerp(val[2], val[3], tfrac[0]);
    st[5] = lerp(val[4], val[5], tfrac[1]);
    st[6] = vmin;
    st[7] = vmax;
}

// thread t < 8 writes column t of an empty sample's row: the reference leaves latency_stats empty (analyzer.py:105-106)
__device__ __forceinline__ void write_empty_row(double* st, int t) {
    if (t < 8) st[t] = t == 0 ? 0.0 : __builtin_nan("");
}

}  // namespace afs
