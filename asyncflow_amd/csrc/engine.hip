// engine.hip -- MI355X (gfx950) batched discrete-event engine: kernels + C ABI.
//
// Kernels of one af_engine_run:
//   af_pregen_arrivals<G>                  arrival times of every scenario (the windowed sampler), 64 / G scenarios per
//                                          wave, into HBM: arrivals[scenario][index]
//   af_flow_kernel<IPL, FEAT>              stage-parallel kernel (af_flow.hpp): ONE WAVE PER SCENARIO moves up to 64
//                                          requests per step through the stations of a feed-forward request path;
//                                          every other random draw is produced where it is consumed.  Runs every plan
//                                          in its range (af_engine_flow_reason); scenarios it hands back get a second
//                                          chance on its most tolerant instantiation, then go to:
//   af_pregen_edges + af_des_kernel<LDS?, SimPy-order path?, log2 lanes, waves/SIMD>
//                                          the sequential next-event loop (af_core.hpp): one scenario per lane, one
//                                          wave per workgroup, only the first 2^KLOG lanes of a wave carry scenarios;
//                                          every edge draw pre-generated into HBM: draws[slot][stream][index]
//   af_summary_kernel / af_series_kernel   af_engine_summarize: the analyzer (af_summary.hpp)
//   af_swin_partial / af_swin_reduce       af_engine_summarize_series_windows: the sampled series per (group, window of
//                                          ticks) (af_series_windows.hpp)
//   af_sq_small / af_sq_rows / af_sq_select / af_sq_final
//                                          af_engine_summarize_series_quantiles: exact quantiles of the sampled series per
//                                          (group, window of ticks, series) (af_series_quantiles.hpp)
//   af_sexc_kernel                         af_engine_summarize_series_excursions: runs of the sampled series above a threshold
//                                          per (scenario, window of ticks, series) (af_series_excursions.hpp)
//   af_shist_kernel                        af_engine_summarize_series_histogram: occupancy histograms of the sampled series
//                                          per (group, window of ticks, output column) (af_series_histogram.hpp)
//   af_scomb_partial / af_scomb_reduce     af_engine_summarize_series_combined: sum, min, max and spread across the series
//                                          of a sample row per (group, window of ticks, combination) (af_series_combined.hpp)
//   af_sjoint_partial / af_sjoint_fold     af_engine_summarize_series_joint: the six exact integer sums of pairs of series,
//                                          lagged or not, per (group, window of ticks, pair) (af_series_joint.hpp)
//   af_swarm_batches / af_swarm_cell       af_engine_summarize_series_warmup: the MSER truncation point of integer series per
//                                          (group, window of ticks, column) in exact integers (af_series_warmup.hpp, af_wide.hpp)
//
// Memory plan
//   LDS  : flow kernel: [plan blob, patched per scenario][station lists, select scratch / server segments, rings,
//          counters, tick-difference ring] (aff::make_flow_layout); next-event kernels: [plan blob][per-lane state:
//          64-bit words, SoA [index][lane]] -> any per-lane index pattern is bank-conflict free
//   HBM  : arrival times / pre-generated draws (read once), outputs (rqs_clock, sampled series, counts), the scratch
//          of the shared-instant path; the next-event per-lane state too when it does not fit the 160 KiB LDS of a CU
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see build.py).
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../include/asyncflow_hip.h"
#include "af_core.hpp"
#include "af_flow_host.hpp"
#include "af_plan_pack.hpp"
#include "af_pregen.hpp"
#include "af_summary.hpp"
#include "af_pooled.hpp"
#include "af_series_windows.hpp"
#include "af_series_quantiles.hpp"
#include "af_series_excursions.hpp"
#include "af_series_histogram.hpp"
#include "af_series_combined.hpp"
#include "af_series_joint.hpp"
#include "af_series_warmup.hpp"
#include "af_windowed.hpp"
#include "af_arrival.hpp"
#include "af_state.hpp"
#include "af_quantiles.hpp"
#include "af_cells.hpp"
#include "af_arrival_counts.hpp"
#include "af_inflight.hpp"
#include "af_alerts.hpp"
#include "af_alert_outcomes.hpp"
#include "af_exemplars.hpp"
#include "af_latency_histogram.hpp"
#include "af_paired.hpp"

#define LDS_AS __attribute__((address_space(3)))

namespace {

constexpr uint32_t kLdsLimit = 160u * 1024u;  // bytes per workgroup on gfx950
constexpr uint32_t kWave = 64u;

struct KArgs {
    double total_time, sample_period, gen_users_mean, gen_users_sigma, gen_rpm_mean, gen_window_s;
    uint32_t metrics_mask, gen_users_dist, gen_out_edge, client_out_edge;
    uint32_t n_edges, n_servers, lb_algo, n_lb_edges, n_rows, n_edge_marks, n_srv_marks, every_event_in_order;
    uint32_t off_edge, off_srv, off_ep, off_row, off_emark, off_smark, off_lb;  // word offsets in the blob
    uint32_t blob_bytes;  // multiple of 16
    const unsigned char* blob;
    af::Layout L;
    uint32_t n_scen;
    const uint64_t* seeds;
    uint32_t n_ovr;
    const uint32_t* ovr_param;
    const uint32_t* ovr_index;
    const double* ovr_values;  // [n_ovr][ovr_stride], already offset to this chunk's first scenario
    uint32_t ovr_stride;       // scenarios in the whole sweep
    double* clock;
    uint32_t clock_cap;
    uint32_t* samples;
    uint32_t tick_cap, n_series, series_pitch;
    uint32_t* counts;
    uint32_t* online_hist;  // [n_scen][online_hist_bins] or null
    uint32_t* online_rps;   // [n_scen][online_rps_buckets] or null
    uint32_t online_hist_bins, online_rps_buckets;
    double online_hist_scale;
    unsigned char* state;  // HBM-resident lane state (global-state mode only)
    uint64_t state_bytes_per_wave;
    double* draws;          // pre-generated draws [n_scen][1 + n_edges][n_draw]
    uint32_t n_draw;
    uint32_t* pre_flags;    // [n_scen] AF_FLAG_DRAW_OVERFLOW from the arrival pre-generation
    uint64_t* tie;          // [n_scen][L.tie_words] scratch of the shared-timestamp path (HBM)
    const uint32_t* scen_map;  // subset launches: lane j simulates scenario scen_map[j] (null = identity)
    const uint32_t* draw_slot; // where lane j's pre-generated draws / pre_flags / scratch live (null = draws_by_lane ? j : scenario)
    uint32_t draws_by_lane;
    uint32_t* n_shared;     // first pass: number of scenarios that met a shared instant
};

// Per-lane state memory, [index][lane] with 2^klog scenario lanes per wave.
// KLOG is a compile-time constant: the shift folds into the LDS instruction's immediate offset and
// into the address arithmetic of every state access (measured: -4.6 % kernel time against a
// run-time shift).
template <int KLOG>
struct MemLds {
    LDS_AS uint64_t* w;  // already offset by the lane
    __device__ __forceinline__ uint64_t ld(uint32_t i) const { return w[i << KLOG]; }
    __device__ __forceinline__ void st(uint32_t i, uint64_t v) const { w[i << KLOG] = v; }
};

template <int KLOG>
struct MemGlobal {
    uint64_t* w;
    __device__ __forceinline__ uint64_t ld(uint32_t i) const { return w[i << KLOG]; }
    __device__ __forceinline__ void st(uint32_t i, uint64_t v) const { w[i << KLOG] = v; }
};

__device__ __forceinline__ const LDS_AS uint64_t* lds_words(unsigned char* smem, uint32_t word_off) {
    return (const LDS_AS uint64_t*)smem + word_off;
}

// The wave's main loop.  Lanes free-run round().  In the variant that has the SimPy-order path, a
// lane that reports an instant shared by several timed events makes the wave leave the inner loop;
// that lane replays the instant in SimPy's event order and the wave re-enters.  The cold path sits
// OUTSIDE the inner loop and every lane's scalars go through memory around it, so that as little as
// possible stays live across it (measured on the 10k LB-2 sweep with the path never taken: 3 472 ms
// with the path inside the loop, 2 755 ms outside, 2 690 ms with the scalars parked; the lean
// variant, which has no such path at all, takes 2 085 ms -- the rest is register pressure the
// compiler still lets leak into the loop).
template <class LaneT, bool kFaithful>
__device__ __forceinline__ void run_lanes(LaneT& S, bool active) {
    if constexpr (!kFaithful) {  // lean variant: round() never reports ROUND_SHARED
        bool run = active;
        while (__any(run)) {
            if (run) run = S.round();
        }
    } else {
        uint32_t st = active ? LaneT::ROUND_MORE : LaneT::ROUND_STOP;
        for (;;) {
            do {
                if (st == LaneT::ROUND_MORE) st = S.round();
            } while (!__any(st == LaneT::ROUND_SHARED) && __any(st == LaneT::ROUND_MORE));
            if (!__any(st == LaneT::ROUND_SHARED)) break;
            volatile uint64_t* slot = S.D.tie + (S.L.tie_words - LaneT::PARK_WORDS);
            if (active) S.park_regs(slot);
            if (st == LaneT::ROUND_SHARED) {
                S.unpark_regs(slot);
                S.shared_instant();
                S.park_regs(slot);
                st = LaneT::ROUND_MORE;
            }
            if (active) S.unpark_regs(slot);
        }
    }
}

// (Measured on MI355X, profiles/r01: forcing more than the natural 3 waves/SIMD with a
// launch bound spills registers and is 1.5-3x slower; the lean variant keeps its natural 134 VGPRs.)
//
// kFaithful = false is the lean first pass: a scenario in which two timed events share an instant
// stops there (af_core.hpp) and is simulated again by the kFaithful = true variant, whose extra
// SimPy-order path costs ~30 % of kernel time through register pressure alone (measured).
//
// WPE = register budget as waves per SIMD: 3 (<= 168 VGPRs; the lean variant needs 134) or, for the
// SimPy-order variant only, 2 (it wants ~210 VGPRs: no spills, but a third fewer resident waves).
template <bool kLdsState, bool kFaithful, int KLOG>
__device__ __forceinline__ void des_body(const KArgs& a_in) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t lane = threadIdx.x;
#if defined(AF_JIT) && !defined(AF_FLOW_JIT)
    // Plan-specialised build (asyncflow_amd/jit.py): the plan's shape as compile-time constants --
    // state offsets fold into instruction immediates, loops over edges / servers / series unroll,
    // branches on the plan's shape disappear (measured on the 10k LB-2 sweep: 2 084 -> 1 912 ms).
    KArgs a = a_in;
    a.metrics_mask = AF_JIT_METRICS;
    a.gen_out_edge = AF_JIT_GEN_EDGE;
    a.client_out_edge = AF_JIT_CLIENT_EDGE;
    a.n_edges = AF_JIT_N_EDGES;
    a.n_servers = AF_JIT_N_SERVERS;
    a.lb_algo = AF_JIT_LB_ALGO;
    a.n_lb_edges = AF_JIT_N_LB;
    a.n_rows = AF_JIT_N_ROWS;
    a.n_edge_marks = AF_JIT_N_EMARKS;
    a.n_srv_marks = AF_JIT_N_SMARKS;
    a.every_event_in_order = AF_JIT_ORDER_ALL;
    a.off_edge = AF_JIT_OFF_EDGE;
    a.off_srv = AF_JIT_OFF_SRV;
    a.off_ep = AF_JIT_OFF_EP;
    a.off_row = AF_JIT_OFF_ROW;
    a.off_emark = AF_JIT_OFF_EMARK;
    a.off_smark = AF_JIT_OFF_SMARK;
    a.off_lb = AF_JIT_OFF_LB;
    a.blob_bytes = AF_JIT_BLOB_BYTES;
    a.L = af::make_layout(AF_JIT_CAP, AF_JIT_FCAP, AF_JIT_N_EDGES, AF_JIT_N_SERVERS, AF_JIT_N_LB, AF_JIT_N_ROWS, AF_JIT_OVR_MASK, AF_JIT_N_EMARKS, AF_JIT_N_SMARKS);
    // (clock / tick / draw capacities stay run-time values: they change with replicas, horizon and the runner's
    // auto-grow, and a key that contains them recompiles -- or silently misses -- for every such change)
    a.n_series = AF_JIT_N_EDGES + 3 * AF_JIT_N_SERVERS;
    a.series_pitch = (AF_JIT_N_EDGES + 3 * AF_JIT_N_SERVERS + 3) & ~3;
    if (AF_JIT_HAS_CLOCK) __builtin_assume(a.clock != nullptr); else a.clock = nullptr;
    if (AF_JIT_HAS_SAMPLES) __builtin_assume(a.samples != nullptr); else a.samples = nullptr;
    if (!AF_JIT_HAS_ONLINE) a.online_hist = a.online_rps = nullptr;
#else
    const KArgs& a = a_in;
#endif

    // stage the read-only plan into LDS (shared by the 64 scenarios of the wave)
    for (uint32_t i = lane * 16u; i < a.blob_bytes; i += kWave * 16u)
        *reinterpret_cast<uint4*>(smem + i) = *reinterpret_cast<const uint4*>(a.blob + i);
    __syncthreads();

    af::PlanView P;
    P.total_time = a.total_time;
    P.sample_period = a.sample_period;
    P.gen_users_mean = a.gen_users_mean;
    P.gen_users_sigma = a.gen_users_sigma;
    P.gen_rpm_mean = a.gen_rpm_mean;
    P.gen_window_s = a.gen_window_s;
    P.metrics_mask = a.metrics_mask;
    P.gen_users_dist = a.gen_users_dist;
    P.gen_out_edge = a.gen_out_edge;
    P.client_out_edge = a.client_out_edge;
    P.n_edges = a.n_edges;
    P.n_servers = a.n_servers;
    P.lb_algo = a.lb_algo;
    P.n_lb_edges = a.n_lb_edges;
    P.n_rows = a.n_rows;
    P.n_edge_marks = a.n_edge_marks;
    P.n_srv_marks = a.n_srv_marks;
    P.every_event_in_order = a.every_event_in_order;
    P.edge = lds_words(smem, a.off_edge);
    P.srv = lds_words(smem, a.off_srv);
    P.ep = lds_words(smem, a.off_ep);
    P.row = lds_words(smem, a.off_row);
    P.emark = lds_words(smem, a.off_emark);
    P.smark = lds_words(smem, a.off_smark);
    P.lb = lds_words(smem, a.off_lb);

    // Only the first 2^klog lanes of a wave carry scenarios.  With few scenarios per GPU the
    // sweep is spread over MANY narrow waves: fewer event kinds per round in each wave (less
    // divergence), every SIMD of the chip busy, several waves per SIMD hiding LDS latency.
    constexpr uint32_t kl = 1u << KLOG;
    const uint32_t scen = (blockIdx.x << KLOG) + lane;
    const bool active = lane < kl && scen < a.n_scen;
    const uint32_t sc = active ? (a.scen_map ? a.scen_map[scen] : scen) : 0u;

    af::LaneOut O;
    O.clock = a.clock ? a.clock + (size_t)sc * a.clock_cap * 2u : nullptr;
    O.samples = a.samples ? a.samples + (size_t)sc * a.series_pitch * a.tick_cap : nullptr;
    O.counts = a.counts + (size_t)sc * af::CNT_SLOTS;
    O.clock_cap = a.clock_cap;
    O.tick_cap = a.tick_cap;
    O.series_pitch = a.series_pitch;
    O.hist = a.online_hist ? a.online_hist + (size_t)sc * a.online_hist_bins : nullptr;
    O.rps = a.online_rps ? a.online_rps + (size_t)sc * a.online_rps_buckets : nullptr;
    O.hist_bins = a.online_hist_bins;
    O.rps_buckets = a.online_rps_buckets;
    O.hist_scale = a.online_hist_scale;

    const uint64_t seed = a.seeds[sc];
    auto ovr = [&](uint32_t k) { return a.ovr_values[(size_t)k * a.ovr_stride + sc]; };
    const uint32_t slot = !active ? 0u : a.draw_slot ? a.draw_slot[scen] : a.draws_by_lane ? scen : sc;
    af::PreDraws D;
    D.base = a.draws + (size_t)slot * (1u + a.n_edges) * a.n_draw;
    D.n_per_stream = a.n_draw;
    D.flags_in = a.pre_flags[slot];
    D.tie = a.tie + (size_t)slot * a.L.tie_words;

    if constexpr (kLdsState) {
        MemLds<KLOG> M;
        M.w = (LDS_AS uint64_t*)(smem + a.blob_bytes) + (lane & (kl - 1u));
        af::Lane<MemLds<KLOG>, kFaithful> S(P, a.L, M, O, D, seed);
        if (active) S.init(a.ovr_param, a.ovr_index, a.n_ovr, ovr);
        run_lanes<decltype(S), kFaithful>(S, active);
        if (active) S.write_counts();
        if (!kFaithful && active && (S.flags & af::FLAG_SHARED_INSTANT)) atomicAdd(a.n_shared, 1u);
    } else {
        unsigned char* base = a.state + (size_t)blockIdx.x * a.state_bytes_per_wave;
        MemGlobal<KLOG> M;
        M.w = reinterpret_cast<uint64_t*>(base) + (lane & (kl - 1u));
        af::Lane<MemGlobal<KLOG>, kFaithful> S(P, a.L, M, O, D, seed);
        if (active) S.init(a.ovr_param, a.ovr_index, a.n_ovr, ovr);
        run_lanes<decltype(S), kFaithful>(S, active);
        if (active) S.write_counts();
        if (!kFaithful && active && (S.flags & af::FLAG_SHARED_INSTANT)) atomicAdd(a.n_shared, 1u);
    }
}

#if !defined(AF_JIT) || defined(AF_FLOW_JIT)
// ---- stage-parallel kernel (af_flow.hpp): one wave per scenario -------------------------------------
struct WaveHip {
    static __device__ __forceinline__ uint32_t lane() { return threadIdx.x; }
    static __device__ __forceinline__ uint64_t ballot(bool p) { return __ballot(p); }
    static __device__ __forceinline__ bool any(bool p) { return __any(p) != 0; }
    static __device__ __forceinline__ uint32_t shfl32(uint32_t v, uint32_t src) {
        return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(src << 2), (int)v);
    }
    static __device__ __forceinline__ uint64_t shfl64(uint64_t v, uint32_t src) {
        const uint32_t lo = shfl32((uint32_t)v, src), hi = shfl32((uint32_t)(v >> 32), src);
        return ((uint64_t)hi << 32) | lo;
    }
    // One wave per workgroup: its LDS instructions execute in order, so "every lane's LDS writes are visible to every
    // lane" needs no hardware wait beyond the data dependences the compiler tracks (lgkmcnt) -- only the COMPILER must
    // not move LDS accesses to other lanes' data across this point: wavefront-scope fences + a scheduling barrier.
    // (Workgroup-scope fences here cost an s_waitcnt vmcnt(0) each: ~30 times per round the wave waited for its own
    // rqs_clock / sample stores to reach memory.)
    static __device__ __forceinline__ void sync() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    static __device__ __forceinline__ uint32_t lds_add(LDS_AS uint32_t* p, uint32_t v) {
        return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    static __device__ __forceinline__ void global_add(uint32_t* p, uint32_t v) {
        (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    static __device__ __forceinline__ uint32_t global_load(const uint32_t* p) {
        return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    static __device__ __forceinline__ void global_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent"); }
    // the scenario's outputs are in memory (every lane's stores: a device-scope release fence per lane, then the wave barrier that
    // orders the lanes), then the flag (release, device scope) and the count (release, SYSTEM scope: host-coherent memory the
    // analyzer's stream waits on with hipStreamWaitValue32)
    static __device__ __forceinline__ void signal_done(uint32_t* flag, uint32_t* count) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __builtin_amdgcn_wave_barrier();
        if (threadIdx.x == 0u) {
            __hip_atomic_store(flag, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            (void)__hip_atomic_fetch_add(count, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    static __device__ __forceinline__ double rcp(double x) { return __builtin_amdgcn_rcp(x); }
    static __device__ __forceinline__ double fract(double x) { return __builtin_amdgcn_fract(x); }   // v_fract_f64: x - floor(x), exact for x >= 0
    static __device__ __forceinline__ uint32_t bcast32(uint32_t v, uint32_t src) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)src); }
    static __device__ __forceinline__ uint64_t bcast64(uint64_t v, uint32_t src) {
        const uint32_t lo = bcast32((uint32_t)v, src), hi = bcast32((uint32_t)(v >> 32), src);
        return ((uint64_t)hi << 32) | lo;
    }
    // wave64 inclusive prefix sum without LDS: Kogge-Stone inside each row of 16 lanes with DPP row shifts (lanes
    // shifted in from outside the row read 0), then the row totals with row_bcast:15 into rows 1, 3 and row_bcast:31
    // into rows 2, 3 (a lane whose row is masked off keeps `old` = 0)
    template <int CTRL, int ROW_MASK>
    static __device__ __forceinline__ uint32_t dpp(uint32_t v) {
        return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xF, true);
    }
    static __device__ __forceinline__ uint32_t scan_incl_u32(uint32_t v) {
        v += dpp<0x111, 0xF>(v);   // row_shr:1
        v += dpp<0x112, 0xF>(v);   // row_shr:2
        v += dpp<0x114, 0xF>(v);   // row_shr:4
        v += dpp<0x118, 0xF>(v);   // row_shr:8
        v += dpp<0x142, 0xA>(v);   // row_bcast:15 -> rows 1 and 3
        v += dpp<0x143, 0xC>(v);   // row_bcast:31 -> rows 2 and 3
        return v;
    }
    // select()'s lane window (af_flow.hpp, AF_SELECT_WINDOW): the inclusive prefix MAXIMUM by the same six DPP steps (the lanes a
    // row shift leaves without a source read 0, the identity of an unsigned maximum, and so does a lane whose row is masked off),
    // the value of the lane below mine by one DPP wave shift (lane 0 reads 0), and my own bit of a wave-uniform mask as a lane
    // condition (an SGPR pair used as a carry-in or a select mask: no 64-bit vector shift)
    static __device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }
    static __device__ __forceinline__ uint32_t scan_incl_max_u32(uint32_t v) {
        v = umax(v, dpp<0x111, 0xF>(v));   // row_shr:1
        v = umax(v, dpp<0x112, 0xF>(v));   // row_shr:2
        v = umax(v, dpp<0x114, 0xF>(v));   // row_shr:4
        v = umax(v, dpp<0x118, 0xF>(v));   // row_shr:8
        v = umax(v, dpp<0x142, 0xA>(v));   // row_bcast:15 -> rows 1 and 3
        v = umax(v, dpp<0x143, 0xC>(v));   // row_bcast:31 -> rows 2 and 3
        return v;
    }
    static __device__ __forceinline__ uint32_t lane_below_u32(uint32_t v) { return dpp<0x138, 0xF>(v); }   // wave_shr:1
    static __device__ __forceinline__ bool my_bit(uint64_t m) { return __builtin_amdgcn_inverse_ballot_w64(m); }
    static __device__ __forceinline__ uint32_t mbcnt(uint64_t m) {
        return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    }
    static __device__ __forceinline__ unsigned long long clock() { return __builtin_amdgcn_s_memtime(); }   // shader cycles
};

// af_engine_run_summarized: the engine's counter block (FlowArgs::n_fallback) holds, at word kDoneWords, the addresses of the done
// flags and of the done counter, or zeros.  Read HERE, after run(), through a pointer the kernel keeps anyway: as two more
// kernel arguments they were two more scalar register pairs live across the whole kernel (general servers: 280 -> 295 ms).
constexpr uint32_t kDoneWords = 16u;
static __device__ __forceinline__ void signal_scenario_done(const uint32_t* counter_block, uint32_t sc) {
    if (counter_block == nullptr) return;
    const uint64_t* sig = reinterpret_cast<const uint64_t*>(counter_block + kDoneWords);
    uint32_t* flags = reinterpret_cast<uint32_t*>(sig[0]);
    if (flags != nullptr) WaveHip::signal_done(flags + sc, reinterpret_cast<uint32_t*>(sig[1]));
}

// Register budget as waves per SIMD (measured on MI355X, profiles/r02: see DESIGN.md section 4e).
#ifndef AF_FLOW_WPE
#define AF_FLOW_WPE 4
#endif
#endif
#ifndef AF_JIT
// (general servers: the LDS of that form admits ~2 waves per SIMD anyway, so its serial station gets the registers of a
// 3-waves-per-SIMD budget instead of spilling: 128 VGPRs + 112 B of scratch at 4)
template <uint32_t IPL, uint32_t FEAT>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu((FEAT & aff::FEAT_GENSRV) ? 3 : AF_FLOW_WPE))) af_flow_kernel(const aff::FlowArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (blockIdx.x >= a.n_scen) return;
    const uint32_t sc = a.scen_map ? a.scen_map[blockIdx.x] : blockIdx.x;
    aff::Flow<WaveHip, IPL, FEAT> f(a);
    f.run((LDS_AS uint64_t*)smem, sc);
    signal_scenario_done(a.n_fallback, sc);
    if (threadIdx.x == 0u && a.n_fallback) {
        const uint32_t flags = a.counts[(size_t)sc * af::CNT_SLOTS + af::CNT_FLAGS];
        if (flags & aff::FLAG_FLOW_FALLBACK) {
            atomicAdd(a.n_fallback, 1u);
            if (flags & aff::FLOW_WHY_TIE) atomicAdd(a.n_fallback + 1, 1u);
            if (flags & aff::FLOW_WHY_LIST) atomicAdd(a.n_fallback + 2, 1u);
            if (flags & aff::FLOW_WHY_RING) atomicAdd(a.n_fallback + 3, 1u);
            if (flags & aff::FLOW_WHY_RAM) atomicAdd(a.n_fallback + 4, 1u);
        }
    }
}

template <bool kLdsState, bool kFaithful, int KLOG, int WPE>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WPE))) af_des_kernel(const KArgs a) {
    des_body<kLdsState, kFaithful, KLOG>(a);
}
#endif

#ifdef AF_FLOW_JIT
}  // namespace

// Plan-specialised build of the stage-parallel kernel (asyncflow_amd/jit.py; the flags come from af_engine_jit_spec when
// the sweep would run on af_flow_kernel): the instantiation (IPL, FEAT), the plan's shape, the horizon / tick constants
// and the whole LDS layout are compile-time constants.  The generic kernel reads ~100 wave-uniform launch arguments
// that do not fit the 102 SGPRs (a quarter of its static VALU instructions are v_mov, 12 % SGPR<->VGPR-lane spills:
// DESIGN.md section 4e); here they are immediates, LDS offsets fold into the instructions, loops over servers / LB
// edges / step programs have constant trip counts.  Same source, same arithmetic: results are bit-identical.
// What stays a run-time argument: every pointer, the scenario count and the clock / tick / draw capacities (they
// change with replicas and the runner's auto-grow; a key that contained them would recompile for every such change).
#define AF_FJ_F64(bits) __builtin_bit_cast(double, (uint64_t)(bits))
// (the register budget follows the waves per SIMD the launch's LDS leaves room for -- AF_FJ_WPE, worked out by flow_jit_spec_string:
// BASELINE config 5's 20 KB per wave admit two waves per SIMD, and with the 256-register budget of two instead of the 128 of four
// its kernel takes 189 instead of 207 ms, round 5)
#ifndef AF_FJ_WPE
#define AF_FJ_WPE (((AF_FJ_FEAT) & aff::FEAT_GENSRV) ? 3 : AF_FLOW_WPE)
#endif
extern "C" __global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(AF_FJ_WPE))) af_flow_jit(const aff::FlowArgs a_in) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (blockIdx.x >= a_in.n_scen) return;
    aff::FlowArgs a = a_in;
    a.total_time = AF_FJ_F64(AF_FJ_TOTAL_TIME);
    a.sample_period = AF_FJ_F64(AF_FJ_PERIOD);
    a.inv_period = AF_FJ_F64(AF_FJ_INV_PERIOD);
    a.tick_eps = AF_FJ_F64(AF_FJ_TICK_EPS);
    a.metrics_mask = AF_FJ_METRICS;
    a.gen_out_edge = AF_FJ_GEN_EDGE;
    a.client_out_edge = AF_FJ_CLIENT_EDGE;
    a.n_edges = AF_FJ_N_EDGES;
    a.n_servers = AF_FJ_N_SERVERS;
    a.has_lb = AF_FJ_HAS_LB;
    a.n_lb_edges = AF_FJ_N_LB;
    a.n_edge_marks = AF_FJ_N_EMARKS;
    a.n_srv_marks = AF_FJ_N_SMARKS;
    a.lb_least_connections = AF_FJ_LC;
    a.max_pre = AF_FJ_MAX_PRE;
    a.max_cpu = AF_FJ_MAX_CPU;
    a.max_post = AF_FJ_MAX_POST;
    a.ram_scale = AF_FJ_RAM_SCALE;
    a.ram_unit = 1.0 / AF_FJ_RAM_SCALE;
    a.off_edge = AF_FJ_OFF_EDGE;
    a.off_srv = AF_FJ_OFF_SRV;
    a.off_ep = AF_FJ_OFF_EP;
    a.off_row = AF_FJ_OFF_ROW;
    a.off_emark = AF_FJ_OFF_EMARK;
    a.off_smark = AF_FJ_OFF_SMARK;
    a.off_lb = AF_FJ_OFF_LB;
    a.blob_bytes = AF_FJ_BLOB_BYTES;
    a.n_ticks = AF_FJ_N_TICKS;
    a.L = aff::FlowLayout{AF_FJ_LAYOUT};
    if (AF_FJ_HAS_CLOCK) __builtin_assume(a.clock != nullptr); else a.clock = nullptr;
    if (AF_FJ_HAS_SAMPLES) __builtin_assume(a.samples != nullptr); else a.samples = nullptr;
    if (!AF_FJ_HAS_ONLINE) a.online_hist = a.online_rps = nullptr;
    if (!AF_FJ_HAS_OVR) a.n_ovr = 0u;
    const uint32_t sc = a.scen_map ? a.scen_map[blockIdx.x] : blockIdx.x;
    aff::Flow<WaveHip, AF_FJ_IPL, AF_FJ_FEAT> f(a);
    f.run((LDS_AS uint64_t*)smem, sc);
    signal_scenario_done(a.n_fallback, sc);
    if (threadIdx.x == 0u && a.n_fallback) {
        const uint32_t flags = a.counts[(size_t)sc * af::CNT_SLOTS + af::CNT_FLAGS];
        if (flags & aff::FLAG_FLOW_FALLBACK) {
            atomicAdd(a.n_fallback, 1u);
            if (flags & aff::FLOW_WHY_TIE) atomicAdd(a.n_fallback + 1, 1u);
            if (flags & aff::FLOW_WHY_LIST) atomicAdd(a.n_fallback + 2, 1u);
            if (flags & aff::FLOW_WHY_RING) atomicAdd(a.n_fallback + 3, 1u);
            if (flags & aff::FLOW_WHY_RAM) atomicAdd(a.n_fallback + 4, 1u);
        }
    }
}
#elif defined(AF_JIT)
}  // namespace

// Entry points of a plan-specialised code object (built by asyncflow_amd/jit.py with hipcc --genco,
// loaded by af_engine_set_kernels): the lean variant and the SimPy-order variant with its two
// register budgets, for ONE (state placement, lanes per wave) pair.
extern "C" __global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3))) af_jit_lean(const KArgs a) {
    des_body<AF_JIT_LDS != 0, false, AF_JIT_KLOG>(a);
}
extern "C" __global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3))) af_jit_order3(const KArgs a) {
    des_body<AF_JIT_LDS != 0, true, AF_JIT_KLOG>(a);
}
extern "C" __global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) af_jit_order2(const KArgs a) {
    des_body<AF_JIT_LDS != 0, true, AF_JIT_KLOG>(a);
}
#else  // ------------------------------------------------------------------------------- AOT build

// ---- draw pre-generation (fully parallel, full occupancy) ---------------------------
__device__ __forceinline__ double ovr_or(const KArgs& a, uint32_t param, uint32_t index, uint32_t scen, double dflt) {
    for (uint32_t k = 0; k < a.n_ovr; ++k)
        if (a.ovr_param[k] == param && a.ovr_index[k] == index) dflt = a.ovr_values[(size_t)k * a.ovr_stride + scen];
    return dflt;
}

// Stream 0: the windowed arrival sampler (af::gen_next_gap is its sequential statement: samplers/
// poisson_poisson.py:51-82, gaussian_poisson.py:63-94) and the absolute arrival times
// t_k = t_{k-1} + gap_k (env.now + gap, rqs_generator.py:104).
//
// FOUR scenarios per wave, 16 lanes each.  The expensive part of a gap (Philox block, log, division) is
// evaluated for 16 consecutive draw indices of each scenario at once -- a draw is a pure function of its
// index.  The order-dependent part is two running f64 sums (the sampler's virtual clock and the
// simulation clock): lane l of a group adds the gaps 0..l of the batch to the group's sums ONE BY ONE, in
// draw order -- the sequential sampler's own additions, so every prefix is bit-identical to it -- while the
// 16 steps serve the four scenarios of the wave together.  The window / horizon tests are then evaluated
// on all prefixes at once; the first draw that crosses the window end (discarded, on to the next window:
// the next index is the new window's user draw) or the horizon ends the batch.
// Block b pre-generates for scenarios scen_map[4 b + g] (null = 4 b + g) into slots 4 b + g.  `stride` =
// doubles per slot (n_draw when only the arrivals are wanted: the flow kernel; (1 + n_edges) * n_draw otherwise).
// G = lanes per scenario (16, 12 or 8: 4, 5 or 8 scenarios per wave).  The kernel is bound by instruction issue per
// SIMD, so its time is (waves on the fullest SIMD) x (work of a wave): 2 500 waves of 4 scenarios on 1 024 SIMDs take
// the time of 3 waves, 2 000 waves of 5 scenarios the time of 2 slightly longer ones (af_engine_run picks G).
template <uint32_t G>
__global__ void __launch_bounds__(64) af_pregen_arrivals(const KArgs a, uint32_t stride) {
    constexpr uint32_t S = 64u / G;                     // scenarios per wave (lanes >= S * G idle)
    const uint32_t lane = threadIdx.x, grp = lane / G, l = lane - grp * G, gbase = grp * G;
    const uint32_t slot = blockIdx.x * S + grp;
    const bool valid = grp < S && slot < a.n_scen;
    const uint32_t scen = valid ? (a.scen_map ? a.scen_map[slot] : slot) : 0u;
    const uint64_t seed = a.seeds[scen];
    const double users_mean = ovr_or(a, af::PARAM_GEN_USERS_MEAN, 0u, scen, a.gen_users_mean);
    const double users_sigma = ovr_or(a, af::PARAM_GEN_USERS_SIGMA, 0u, scen, a.gen_users_sigma);
    const double rpm = ovr_or(a, af::PARAM_GEN_RPM_MEAN, 0u, scen, a.gen_rpm_mean);
    const double window_s = ovr_or(a, af::PARAM_GEN_WINDOW, 0u, scen, a.gen_window_s);
    const double rps_per_user = rpm / 60.0;
    const double T = a.total_time;
    double* out = a.draws + (size_t)slot * stride;  // stream 0 of this slot
    double g_now = 0.0, g_wend = 0.0, lam = 0.0, t = 0.0;  // identical in the G lanes of a group
    uint32_t draws = 0u, k = 0u, flags = 0u;
    bool run = valid;
    while (__any(run)) {
        run = run && g_now < T;
        if (run && g_now >= g_wend) {  // new window: the number of active users
            g_wend = g_now + window_s;
            const uint32_t idx = draws++;
            double users;
            if (a.gen_users_dist == af::DIST_NORMAL) {
                const double v = users_mean + users_sigma * af::af_norminv(af::uniform_j(seed, af::STREAM_GENERATOR, idx, 0u));
                users = v > 0.0 ? v : 0.0;
            } else {
                users = (double)af::af_poisson(users_mean, seed, af::STREAM_GENERATOR, idx, 0u);
            }
            lam = users * rps_per_user;
        }
        const bool idle = run && lam <= 0.0;   // nobody active in this window
        if (idle) g_now = g_wend;
        const bool draw = run && !idle;
        // G gaps of this scenario (lanes of scenarios that do not draw compute a harmless dummy)
        const af::U4 r = af::draw_block(seed, af::STREAM_GENERATOR, draws + l, 0u);
        double u = af::u53(r.x, r.y);
        if (u < 1e-15) u = 1e-15;
        const double dt = -af::af_log_unit(1.0 - u) / (draw ? lam : 1.0);
        // prefixes in draw order: Gs = sampler clock after gap l, Ss = simulation clock after gap l
        double Gs = g_now, Ss = t;
#pragma unroll
        for (uint32_t j = 0u; j < G; ++j) {
            const double dj = __shfl(dt, (int)((gbase + j) & 63u), 64);
            if (l >= j) {
                Gs += dj;
                Ss = Ss + dj;
            }
        }
        const bool over = Gs > T;                  // the sampler is exhausted at this draw
        const bool cross = !over && Gs >= g_wend;  // this draw crosses the window end: discarded
        const uint64_t stops = __ballot(draw && (over || cross));
        const uint32_t mine = (uint32_t)(stops >> (gbase & 63u)) & ((1u << G) - 1u);
        const uint32_t first = mine ? (uint32_t)__builtin_ctz(mine) : G;   // draws before it are arrivals
        uint32_t n_acc = first;
        bool full = false;
        if (draw && k + n_acc > a.n_draw) {  // more arrivals than the array holds
            n_acc = a.n_draw - k;
            full = true;
        }
        if (draw && l < n_acc) out[k + l] = Ss;
        // the group's state after the batch
        const double Glast = __shfl(Gs, (int)((gbase + G - 1u) & 63u), 64), Slast = __shfl(Ss, (int)((gbase + G - 1u) & 63u), 64);
        const double Sprev = __shfl(Ss, (int)((gbase + (first > 0u ? first - 1u : 0u)) & 63u), 64);
        const bool over_first = ((__ballot(over) >> (gbase & 63u)) >> (first % G)) & 1ull;
        if (draw) {
            k += n_acc;
            if (full) {
                flags = AF_FLAG_DRAW_OVERFLOW;
                run = false;
            } else if (first == G) {
                g_now = Glast;
                t = Slast;
                draws += G;
            } else {
                if (first > 0u) t = Sprev;
                draws += first + 1u;
                if (over_first) run = false;
                else g_now = g_wend;
            }
        }
    }
    if (valid) {
        for (uint32_t i = k + l; i < a.n_draw; i += G) out[i] = af::AF_INF;
        if (l == 0u) a.pre_flags[slot] = flags;
    }
}

// Round 3: the same kernel with ONE DPP ROW (16 lanes) per scenario.  The order-dependent part -- lane l adds gaps 0..l to
// the row's two running sums one by one -- used to fetch gap j of its group through the LDS crossbar (ds_bpermute, two
// per step and ~100+ cycles each, 12-16 dependent steps per batch: ~1 500 of a batch's ~2 000 cycles were this chain;
// the kernel was bound by that latency at 2 waves per SIMD, not by issue).  A group that IS a DPP row gets gap j as
// `v_mov_b32_dpp ... row_newbcast:j` (gfx90a+): register-file latency, no LDS.  Same draws, same f64 additions in the
// same order: bit-identical arrival times (tests/test_gpu_flow.py::test_arrival_pregeneration_group_widths_are_equivalent).
// The once-a-window user draw (Poisson by chunked inversion / normal quantile) sits behind a call so that the hot loop
// keeps <= 128 VGPRs: 2 500 waves of 4 scenarios are then all resident (4 per SIMD).
template <int J>
__device__ __forceinline__ double row_bcast(double v) {
    const uint64_t u = af::d2u(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)u, 0x150 + J, 0xF, 0xF, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(u >> 32), 0x150 + J, 0xF, 0xF, false);
    return af::u2d(((uint64_t)hi << 32) | lo);
}
__device__ __noinline__ double pregen_users_draw(uint32_t dist, double mean, double sigma, uint64_t seed, uint32_t idx) {
    if (dist == af::DIST_NORMAL) {
        const double v = mean + sigma * af::af_norminv(af::uniform_j(seed, af::STREAM_GENERATOR, idx, 0u));
        return v > 0.0 ? v : 0.0;
    }
    return (double)af::af_poisson(mean, seed, af::STREAM_GENERATOR, idx, 0u);
}
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4))) af_pregen_arrivals_rows(const KArgs a, uint32_t stride) {
    constexpr uint32_t G = 16u, S = 4u;
    const uint32_t lane = threadIdx.x, grp = lane >> 4, l = lane & 15u, gbase = grp * G;
    const uint32_t slot = blockIdx.x * S + grp;
    const bool valid = slot < a.n_scen;
    const uint32_t scen = valid ? (a.scen_map ? a.scen_map[slot] : slot) : 0u;
    const uint64_t seed = a.seeds[scen];
    const double users_mean = ovr_or(a, af::PARAM_GEN_USERS_MEAN, 0u, scen, a.gen_users_mean);
    const double users_sigma = ovr_or(a, af::PARAM_GEN_USERS_SIGMA, 0u, scen, a.gen_users_sigma);
    const double rpm = ovr_or(a, af::PARAM_GEN_RPM_MEAN, 0u, scen, a.gen_rpm_mean);
    const double window_s = ovr_or(a, af::PARAM_GEN_WINDOW, 0u, scen, a.gen_window_s);
    const double rps_per_user = rpm / 60.0;
    const double T = a.total_time;
    double* out = a.draws + (size_t)slot * stride;
    double g_now = 0.0, g_wend = 0.0, lam = 0.0, t = 0.0;   // identical in the 16 lanes of a row
    uint32_t draws = 0u, k = 0u, flags = 0u;
    bool run = valid;
    while (__any(run)) {
        run = run && g_now < T;
        if (run && g_now >= g_wend) {  // new window: the number of active users
            g_wend = g_now + window_s;
            lam = pregen_users_draw(a.gen_users_dist, users_mean, users_sigma, seed, draws++) * rps_per_user;
        }
        const bool idle = run && lam <= 0.0;   // nobody active in this window
        if (idle) g_now = g_wend;
        const bool draw = run && !idle;
        const af::U4 r = af::draw_block(seed, af::STREAM_GENERATOR, draws + l, 0u);
        double u = af::u53(r.x, r.y);
        if (u < 1e-15) u = 1e-15;
        const double dt = -af::af_log_unit(1.0 - u) / (draw ? lam : 1.0);
        // prefixes in draw order: Gs = sampler clock after gap l, Ss = simulation clock after gap l (x + 0.0 == x exactly)
        double Gs = g_now, Ss = t;
#define AF_ROW_STEP(J) { const double dj = row_bcast<J>(dt); const double m = l >= (J) ? dj : 0.0; Gs += m; Ss = Ss + m; }
        AF_ROW_STEP(0) AF_ROW_STEP(1) AF_ROW_STEP(2) AF_ROW_STEP(3) AF_ROW_STEP(4) AF_ROW_STEP(5) AF_ROW_STEP(6) AF_ROW_STEP(7)
        AF_ROW_STEP(8) AF_ROW_STEP(9) AF_ROW_STEP(10) AF_ROW_STEP(11) AF_ROW_STEP(12) AF_ROW_STEP(13) AF_ROW_STEP(14) AF_ROW_STEP(15)
#undef AF_ROW_STEP
        const bool over = Gs > T;                  // the sampler is exhausted at this draw
        const bool cross = !over && Gs >= g_wend;  // this draw crosses the window end: discarded
        const uint64_t stops = __ballot(draw && (over || cross));
        const double Glast = row_bcast<15>(Gs), Slast = row_bcast<15>(Ss);
        if (stops == 0ull && !__any(draw && k + G > a.n_draw)) {   // the usual batch: 16 arrivals per drawing row, nothing else
            if (draw) {
                out[k + l] = Ss;
                k += G;
                g_now = Glast;
                t = Slast;
                draws += G;
            }
            continue;
        }
        const uint32_t mine = (uint32_t)(stops >> gbase) & 0xFFFFu;
        const uint32_t first = mine ? (uint32_t)__builtin_ctz(mine) : G;   // draws before it are arrivals
        uint32_t n_acc = first;
        bool full = false;
        if (draw && k + n_acc > a.n_draw) {  // more arrivals than the array holds
            n_acc = a.n_draw - k;
            full = true;
        }
        if (draw && l < n_acc) out[k + l] = Ss;
        const double Sprev = __shfl(Ss, (int)((gbase + (first > 0u ? first - 1u : 0u)) & 63u), 64);
        const bool over_first = ((__ballot(over) >> gbase) >> (first & 15u)) & 1ull;
        if (draw) {
            k += n_acc;
            if (full) {
                flags = AF_FLAG_DRAW_OVERFLOW;
                run = false;
            } else if (first == G) {
                g_now = Glast;
                t = Slast;
                draws += G;
            } else {
                if (first > 0u) t = Sprev;
                draws += first + 1u;
                if (over_first) run = false;
                else g_now = g_wend;
            }
        }
    }
    if (valid) {
        for (uint32_t i = k + l; i < a.n_draw; i += G) out[i] = af::AF_INF;
        if (l == 0u) a.pre_flags[slot] = flags;
    }
}

// ---- the grouped form (round 3, af_pregen.hpp: af_arrival_groups) -- one LANE per scenario for the order-dependent part,
// the variates worked out beside it by the other waves of the workgroup ------------------------------------------------
// (A first split -- the variates by a parallel kernel into HBM, the sums by 8 lanes and 8 draws per scenario and step, the
// same masked-sum formulation as above -- was built and removed: its chain kernel alone executed 2.9e9 VALU wave-
// instructions, 233 per 64 draws, 11.9 ms against 11.0 ms for the fused row kernel.  The serial bookkeeping is what the
// pre-generation costs, and it only goes away when a lane does nothing but its own scenario's additions: 16 adds + 24
// instructions of division per 64 draws.  af_pregen.hpp tells what that lane must NOT do: touch HBM.)

// launch helper: the group width with the shortest issue-bound time for `n` scenarios (see the kernel's comment).
// Measured (10 000 / 8 192 LB-2 replicas): 4 per wave 15.2 / 9.5 ms, 5 per wave 11.7 / -, 8 per wave - / 15.1 ms (one wave
// per SIMD: nothing hides its latencies).  More than 4 per wave only when the SIMDs still get ~2 waves each and the
// scenarios are alike (`uniform_load`: no per-scenario users / rpm column -- a wave is as slow as its heaviest scenario).
// `grouped`: af_arrival_groups instead (af_engine_run decides: sweeps of alike scenarios from a few thousand on, long
// sampling windows; AF_PREGEN_MODE=rows / groups overrides, AF_PREGEN_GROUP = scenarios per workgroup).
// scenarios per workgroup of af_arrival_groups: one workgroup per CU while that leaves it <= 64 scenarios -- the chain wave of a
// workgroup is as long as ONE scenario's chain however many lanes it has, the producers' work grows with them
static uint32_t pregen_group_width(uint32_t n) {
    uint32_t group = (n + 255u) / 256u < 64u ? (n + 255u) / 256u : 64u;
    if (const char* env = std::getenv("AF_PREGEN_GROUP")) {
        const int v = std::atoi(env);
        if (v >= 1 && v <= 64) group = (uint32_t)v;
    }
    return group;
}

static int launch_pregen_arrivals(const KArgs& a, uint32_t n, uint32_t stride, bool uniform_load, hipStream_t stream,
                                  bool grouped = false, uint32_t* group_out = nullptr) {
    if (grouped) {
        afp::ArrivalArgs g{};
        g.total_time = a.total_time;
        g.users_mean = a.gen_users_mean;
        g.users_sigma = a.gen_users_sigma;
        g.rpm = a.gen_rpm_mean;
        g.window_s = a.gen_window_s;
        g.users_dist = a.gen_users_dist;
        g.n_scen = n;
        g.n_draw = a.n_draw;
        g.stride = stride;
        g.group = pregen_group_width(n);
        if (group_out) *group_out = g.group;
        g.seeds = a.seeds;
        g.scen_map = a.scen_map;
        g.n_ovr = a.n_ovr;
        g.ovr_param = a.ovr_param;
        g.ovr_index = a.ovr_index;
        g.ovr_values = a.ovr_values;
        g.ovr_stride = a.ovr_stride;
        g.out = a.draws;
        g.pre_flags = a.pre_flags;
        // (set before every launch: the attribute is per device, engines of several devices run in threads of one process,
        // and the call costs microseconds next to a kernel of milliseconds -- ADVICE r3)
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(afp::af_arrival_groups), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)sizeof(afp::GroupLds)) != hipSuccess)
            return 1;
        hipLaunchKernelGGL(afp::af_arrival_groups, dim3((n + g.group - 1u) / g.group), dim3(afp::kGroupThreads),
                           sizeof(afp::GroupLds), stream, g);
        return 0;
    }
    double best = 1e300;
    uint32_t best_s = 4u;
    for (uint32_t s : {4u, 5u, 8u}) {
        const double waves = std::ceil((double)n / (double)s);
        if (s != 4u && (!uniform_load || waves / 1024.0 < 1.9)) continue;
        const double cost = std::ceil(waves / 1024.0) * (4.06 * (double)s + 8.0);
        if (cost < best - 1e-9) {
            best = cost;
            best_s = s;
        }
    }
    bool rows = true;   // round 3: one DPP row per scenario (af_pregen_arrivals_rows) unless an older variant is asked for
    if (const char* env = std::getenv("AF_PREGEN_SCEN_PER_WAVE")) {
        const uint32_t v = (uint32_t)std::atoi(env);
        if (v == 4u || v == 5u || v == 8u) {
            best_s = v;
            rows = false;
        }
    }
    if (rows) {
        hipLaunchKernelGGL(af_pregen_arrivals_rows, dim3((n + 3u) / 4u), dim3(64), 0, stream, a, stride);
        return 0;
    }
    const dim3 grid((n + best_s - 1u) / best_s);
    if (best_s == 4u) hipLaunchKernelGGL(af_pregen_arrivals<16>, grid, dim3(64), 0, stream, a, stride);
    else if (best_s == 5u) hipLaunchKernelGGL(af_pregen_arrivals<12>, grid, dim3(64), 0, stream, a, stride);
    else hipLaunchKernelGGL(af_pregen_arrivals<8>, grid, dim3(64), 0, stream, a, stride);
    return 0;
}

// second pass: the online counters of the scenarios that start over are cleared first
__global__ void af_zero_online(const KArgs a, uint32_t count) {
    const uint32_t j = blockIdx.x;
    if (j >= count) return;
    const uint32_t sc = a.scen_map[j];
    if (a.online_hist)
        for (uint32_t i = threadIdx.x; i < a.online_hist_bins; i += blockDim.x) a.online_hist[(size_t)sc * a.online_hist_bins + i] = 0u;
    if (a.online_rps)
        for (uint32_t i = threadIdx.x; i < a.online_rps_buckets; i += blockDim.x) a.online_rps[(size_t)sc * a.online_rps_buckets + i] = 0u;
}

// Streams 1 + e: block (x, scenario, edge) draws 256 consecutive messages (coalesced stores).
__global__ void __launch_bounds__(256) af_pregen_edges(const KArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_draw) return;
    const uint32_t slot = blockIdx.y;
    const uint32_t scen = a.scen_map ? a.scen_map[slot] : slot;
    const uint32_t e = blockIdx.z;
    const uint64_t* rec = reinterpret_cast<const uint64_t*>(a.blob) + a.off_edge + af::EREC * e;
    const double mean = ovr_or(a, af::PARAM_EDGE_MEAN, e, scen, af::u2d(rec[0]));
    const double sigma = ovr_or(a, af::PARAM_EDGE_SIGMA, e, scen, af::u2d(rec[1]));
    const double dropout = ovr_or(a, af::PARAM_EDGE_DROPOUT, e, scen, af::u2d(rec[2]));
    const uint32_t dist = (uint32_t)(rec[3] >> 16) & 0xFFu;
    a.draws[((size_t)slot * (1u + a.n_edges) + 1u + e) * a.n_draw + i] =
        af::pre_edge_draw(a.seeds[scen], e, i, dist, mean, sigma, dropout);
}

__global__ void af_probe_kernel(int kind, uint64_t seed, const double* in, const double* in2, double* out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double x = in[i];
    const double y = in2 ? in2[i] : 0.0;
    double r;
    switch (kind) {
        case 0: {
            const uint32_t packed = (uint32_t)y;
            r = af::uniform_j(seed, packed >> 16, (uint32_t)x, packed & 0xFFFFu);
            break;
        }
        case 1: r = af::af_log(x); break;
        case 2: r = af::af_exp(x); break;
        case 3: r = af::af_norminv(x); break;
        case 4: r = af::af_sqrt(x); break;
        case 5: r = x / y; break;
        case 6: r = (double)af::af_poisson(x, seed, (uint32_t)y >> 16, (uint32_t)y & 0xFFFFu, 0u); break;
        case 7: r = af::af_log_unit(x); break;
        // the draw's integer side, operands and results as BIT PATTERNS of the doubles (tests/test_gpu_draw_bits.py):
        // 8 / 9: words (x, y) / (z, w) of block (index, 0) of stream `stream`, x = the 64-bit seed, y = stream << 32 | index
        case 8:
        case 9: {
            const uint64_t sd = af::d2u(x), si = af::d2u(y);
            const af::U4 b = af::draw_block(sd, (uint32_t)(si >> 32), (uint32_t)si, 0u);
            r = af::u2d(kind == 8 ? ((uint64_t)b.x << 32) | b.y : ((uint64_t)b.z << 32) | b.w);
            break;
        }
        // 10: 1 - u of the uniform made of the words x = hi << 32 | lo, as the exponential draws take it
        case 10: r = af::one_minus_unit_of(af::k53((uint32_t)(af::d2u(x) >> 32), (uint32_t)af::d2u(x))); break;
        default: r = 0.0;
    }
    out[i] = r;
}

// ---- store-pattern probes (af_probe_store): calibration of rocprofv3's WRITE_SIZE on the store shapes of the
// stage-parallel kernel (MI355X_MICROARCH.md: the counter is calibrated for wide coalesced stores only).  Each wave owns
// a contiguous region and fills it exactly once with
//   wide     : 16 B per lane, 64 lanes = 1 KB per store instruction (the reference pattern);
//   pairs16  : the rqs_clock store of Flow::complete -- 16 B per lane, `lanes` consecutive lanes (a batch of n_sel <= 64
//              completions), the next batch right behind it: chunks of lanes x 16 B that are not 64-B aligned;
//   rows48   : the sample store of Flow::flush_ticks for a 12-word pitch -- 4 B per lane, 60 lanes = five 48-byte rows
//              = 240 B per store instruction, the next five rows right behind them.
__global__ void __launch_bounds__(64) af_probe_store_wide(uint32_t* out, size_t words_per_wave) {
    uint32_t* base = out + (size_t)blockIdx.x * words_per_wave;
    for (size_t w = (size_t)threadIdx.x * 4u; w + 4u <= words_per_wave; w += 256u) af::store4(base + w, 1u, 2u, 3u, 4u);
}
__global__ void __launch_bounds__(64) af_probe_store_pairs16(uint32_t* out, size_t words_per_wave, uint32_t lanes) {
    uint32_t* base = out + (size_t)blockIdx.x * words_per_wave;
    for (size_t w0 = 0; w0 + 4u * lanes <= words_per_wave; w0 += 4u * lanes)
        if (threadIdx.x < lanes) af::store4(base + w0 + 4u * threadIdx.x, 1u, 2u, 3u, 4u);
}
__global__ void __launch_bounds__(64) af_probe_store_rows48(uint32_t* out, size_t words_per_wave) {
    uint32_t* base = out + (size_t)blockIdx.x * words_per_wave;
    for (size_t w0 = 0; w0 + 60u <= words_per_wave; w0 += 60u)
        if (threadIdx.x < 60u) base[w0 + threadIdx.x] = (uint32_t)w0;
}

// ---- host side ---------------------------------------------------------------
thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(AF_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));            \
    } while (0)

uint32_t pow2_at_least(uint32_t v) {
    uint32_t p = 1;
    while (p < v) p <<= 1;
    return p;
}

}  // namespace

// kernel variant table: [LDS state][SimPy-order path][log2 lanes per wave][waves per SIMD]
template <bool kLds, bool kFaithful, int WPE>
const void* des_kernel_klog(uint32_t klog) {
    switch (klog) {
        case 0: return reinterpret_cast<const void*>(af_des_kernel<kLds, kFaithful, 0, WPE>);
        case 1: return reinterpret_cast<const void*>(af_des_kernel<kLds, kFaithful, 1, WPE>);
        case 2: return reinterpret_cast<const void*>(af_des_kernel<kLds, kFaithful, 2, WPE>);
        case 3: return reinterpret_cast<const void*>(af_des_kernel<kLds, kFaithful, 3, WPE>);
        case 4: return reinterpret_cast<const void*>(af_des_kernel<kLds, kFaithful, 4, WPE>);
        case 5: return reinterpret_cast<const void*>(af_des_kernel<kLds, kFaithful, 5, WPE>);
        default: return reinterpret_cast<const void*>(af_des_kernel<kLds, kFaithful, 6, WPE>);
    }
}
const void* des_kernel_for(bool lds, bool faithful, uint32_t klog, bool roomy) {
    if (!faithful) return lds ? des_kernel_klog<true, false, 3>(klog) : des_kernel_klog<false, false, 3>(klog);
    if (roomy) return lds ? des_kernel_klog<true, true, 2>(klog) : des_kernel_klog<false, true, 2>(klog);
    return lds ? des_kernel_klog<true, true, 3>(klog) : des_kernel_klog<false, true, 3>(klog);
}

struct af_engine {
    int device = 0;
    bool plan_only = false;   // created with AF_DEVICE_PLAN_ONLY: af_engine_jit_spec and the pure queries only
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;
    KArgs args{};
    unsigned char* d_blob = nullptr;
    unsigned char* d_state = nullptr;
    size_t state_cap = 0;
    void* d_sweep = nullptr;  // seeds + override tables
    size_t sweep_cap = 0;
    double* d_draws = nullptr;  // pre-generated draws
    size_t draws_cap = 0;
    uint32_t* d_pre_flags = nullptr;
    size_t pre_flags_cap = 0;
    uint64_t* d_tie = nullptr;
    size_t tie_cap = 0;
    uint32_t* d_n_shared = nullptr;
    uint32_t* d_map = nullptr;
    size_t map_cap = 0;
    uint32_t* d_order = nullptr;   // launch order of the stage-parallel kernel for sweeps over the load (heaviest scenario first)
    size_t order_cap = 0;
    // af_engine_run_summarized: the analyzer of the scenarios of the stage-parallel kernel's FULL residency rounds runs on a
    // second stream beside the kernel's last, partial round (round 6)
    const af_summary_t* fused_sum = nullptr;   // non-null while af_engine_run works for af_engine_run_summarized
    const af_outputs_t* fused_out = nullptr;
    hipStream_t stream2 = nullptr;
    hipEvent_t ev_s0 = nullptr, ev_s1 = nullptr;
    bool fused_done = false;                   // the sweep's summary was written during af_engine_run (but for the retry lists)
    uint32_t* d_done_flags = nullptr;          // [n] set by a wave of the stage-parallel kernel when its scenario's outputs are in memory
    size_t done_flags_cap = 0;
    uint32_t* h_done_count = nullptr;          // pinned, host-coherent: finished scenarios (the second stream waits on it: hipStreamWaitValue32)
    uint32_t* d_done_count = nullptr;          // ... its device address
    uint32_t* d_retry = nullptr;               // [2][n + 1]: count, then the scenarios the latency / the series kernel met unfinished
    size_t retry_cap = 0;
    unsigned char* d_pool = nullptr;           // af_engine_summarize_pooled's scratch (af_pooled.hpp: compacted latencies, histograms, ...)
    size_t pool_cap = 0;
    bool pool_poisoned = false;                // af_probe_scratch was called: every later growth of the pool is filled with pool_word
    uint32_t pool_word = 0;
    int wait_value_ok = -1;                    // hipDeviceAttributeCanUseStreamWaitValue (-1: not asked yet)
    struct ResidentWaves {                     // gate_for_launch: waves of a flow kernel the device holds at once, per function and LDS size
        const void* fn;
        uint32_t lds, waves;
    };
    std::vector<ResidentWaves> resident_waves;
    uint64_t done_ptrs[2] = {0, 0};            // host copy of d_fb[kDoneWords ..] (a member: an asynchronous copy reads it)
    bool shared_instants_likely = false;
    hipModule_t jit_module = nullptr;  // plan-specialised kernels (af_engine_set_kernels), valid for jit_spec only
    hipFunction_t jit_lean = nullptr, jit_order3 = nullptr, jit_order2 = nullptr;
    std::string jit_spec;
    hipModule_t flow_jit_module = nullptr;   // plan-specialised stage-parallel kernel, valid for flow_jit_spec only
    hipFunction_t flow_jit_fn = nullptr;
    std::string flow_jit_spec;
    hipEvent_t ev3 = nullptr, ev4 = nullptr;
    size_t draw_memory_bytes = 0;
    uint32_t request_capacity = 0, fifo_capacity = 0, force_global = 0, lanes_per_wave = 0;
    uint32_t n_lb_edges = 0;
    std::vector<uint32_t> row_of_step;
    af_stats_t stats{};
    // stage-parallel kernel (af_flow.hpp)
    bool flow_ok = false, flow_general_servers = false, flow_chain = false;   // flow_chain: servers feed servers (FEAT_CHAIN)
    uint32_t flow_levels = 1u;   // levels the servers form (1: no server feeds a server)
    uint32_t flow_lb_pos = 0u;   // the LB station runs in front of the servers of this level (0: right behind the client)
    std::string flow_reason;
    uint32_t flow_mode = 0, flow_list_entries = 0, flow_ring_rows = 0;
    aff::FlowArgs fargs{};
    aff::TickTable tick;
    double* d_tick = nullptr;
    double* d_arr = nullptr;       // arrival times of the chunk [n][n_draw]
    size_t arr_cap = 0;
    uint32_t* d_arr_flags = nullptr;
    size_t arr_flags_cap = 0;
    uint32_t* d_fb = nullptr;      // [32]: [0..9] hand-over counters of the first and of the second-chance launch; [16..19] two 64-bit
                                   // words: af_engine_run_summarized's done flags / done counter (kDoneWords), 0 = nobody waits;
                                   // [21..24], what the second chance (d_fb + 5) finds at that offset: always 0
    uint32_t* d_slot = nullptr;    // draw slots of a second pass over a subset
    size_t slot_cap = 0;
    unsigned long long* d_prof = nullptr;   // AF_FLOW_PROF: shader-clock time per scenario and section of Flow::run
    size_t prof_cap = 0;
    // host copy of what the layout heuristics need
    uint32_t has_lb = 0, cores_max = 1, ram_slots_max = 1;
    std::vector<double> edge_mean, edge_sigma, edge_spike;   // per edge: latency law, largest cumulative spike
    std::vector<double> srv_ram_mb;
    std::vector<uint8_t> edge_dist;
    std::vector<int32_t> lb_edges, srv_out_edge;
    double service_max = 0.0, cpu_max = 0.0;
    int32_t gen_edge = 0, client_edge = 0;
    double rpm_mean = 0.0, users_mean = 0.0, users_sigma = 0.0;
    uint32_t users_dist = 0;
};

namespace {

int validate_plan(const af_plan_t* p) {
    if (!p) return fail(AF_ERR_INVALID, "plan is NULL");
    if (p->abi_version != AF_ABI_VERSION || p->struct_size != sizeof(af_plan_t))
        return fail(AF_ERR_ABI, "af_plan_t ABI mismatch (version or size)");
    if (!(p->total_time > 0.0) || !(p->sample_period > 0.0)) return fail(AF_ERR_INVALID, "bad horizon or sample period");
    if (p->n_edges == 0 || p->n_edges > 255 || p->n_servers > 255) return fail(AF_ERR_INVALID, "edge/server count out of range (1..255 edges, <=255 servers)");
    if (p->gen_out_edge < 0 || (uint32_t)p->gen_out_edge >= p->n_edges) return fail(AF_ERR_INVALID, "generator out edge invalid");
    if (p->client_out_edge < 0 || (uint32_t)p->client_out_edge >= p->n_edges) return fail(AF_ERR_INVALID, "client out edge invalid");
    if (p->has_lb && p->n_lb_edges == 0) return fail(AF_ERR_INVALID, "load balancer without out edges");
    for (uint32_t e = 0; e < p->n_edges; ++e) {
        if (p->edge_target_kind[e] > AF_NODE_SERVER) return fail(AF_ERR_INVALID, "edge target kind invalid");
        if (p->edge_target_kind[e] == AF_NODE_SERVER &&
            (p->edge_target_idx[e] < 0 || (uint32_t)p->edge_target_idx[e] >= p->n_servers))
            return fail(AF_ERR_INVALID, "edge targets unknown server");
        if (p->edge_target_kind[e] == AF_NODE_LB && !p->has_lb) return fail(AF_ERR_INVALID, "edge targets missing LB");
        if (p->edge_dist[e] > AF_DIST_UNIFORM) return fail(AF_ERR_INVALID, "edge distribution invalid");
    }
    for (uint32_t s = 0; s < p->n_servers; ++s) {
        if (p->srv_out_edge[s] < 0 || (uint32_t)p->srv_out_edge[s] >= p->n_edges) return fail(AF_ERR_INVALID, "server out edge invalid");
        if (p->srv_ep_begin[s + 1] <= p->srv_ep_begin[s]) return fail(AF_ERR_INVALID, "server without endpoints");
    }
    for (uint32_t i = 0; i < p->n_lb_edges; ++i)
        if (p->lb_edges[i] < 0 || (uint32_t)p->lb_edges[i] >= p->n_edges) return fail(AF_ERR_INVALID, "LB edge invalid");
    for (uint32_t i = 0; i < p->n_edge_marks; ++i)
        if (p->emark_edge[i] < 0 || (uint32_t)p->emark_edge[i] >= p->n_edges) return fail(AF_ERR_INVALID, "edge mark invalid");
    for (uint32_t i = 0; i < p->n_srv_marks; ++i)
        if (p->smark_lb_edge[i] >= (int32_t)p->n_edges) return fail(AF_ERR_INVALID, "server mark invalid");
    return AF_OK;
}

}  // namespace

namespace {

// Scenario lanes per wave and state placement.  The kernel is latency bound, so few scenarios are
// best spread over MANY narrow waves: fewer event kinds per round in a wave, every SIMD busy,
// several waves per SIMD hiding LDS latency.  Limits: <= 168 VGPRs -> 3 waves/SIMD = 12 per CU;
// LDS-resident state -> 160 KiB per CU.  Cost model fitted to MI355X measurements
// (profiles/r01/lanes_sweep.md): relative time of one wave-round f(lanes), x 2.3 when the state
// lives in HBM, x the number of residency batches.
void choose_lanes(const af_engine* e, uint32_t count, uint32_t blob_bytes, uint64_t bytes_per_lane, uint32_t& kl,
                  bool& lds_state) {
    static const double f_lanes[7] = {1.0, 1.4, 1.65, 2.2, 2.5, 2.4, 2.25};  // 1,2,4,...,64 lanes
    const double n_cu = 256.0, vgpr_waves_per_cu = 12.0;
    double best = 1e300;
    uint32_t best_kl = 4;
    bool best_lds = false;
    for (uint32_t k = 0; k < 7; ++k) {
        const uint32_t cand = 1u << k;
        if (e->lanes_per_wave != 0u && cand != e->lanes_per_wave) continue;
        const double waves_needed = (double)((count + cand - 1u) / cand);
        for (int lds = 1; lds >= 0; --lds) {
            if (lds && e->force_global) continue;
            double per_cu = vgpr_waves_per_cu;
            if (lds) {
                const uint64_t wg_bytes = (uint64_t)blob_bytes + bytes_per_lane * cand;
                if (wg_bytes > kLdsLimit) continue;
                const double fit = (double)(kLdsLimit / wg_bytes);
                per_cu = fit < per_cu ? fit : per_cu;
            }
            const double batches = waves_needed / (n_cu * per_cu);
            const double cost = (batches < 1.0 ? 1.0 : batches) * f_lanes[k] * (lds ? 1.0 : 2.3);
            if (cost < best) {
                best = cost;
                best_kl = cand;
                best_lds = lds != 0;
            }
        }
    }
    kl = best_kl;
    lds_state = best_lds;
}

// Everything a plan-specialised kernel bakes in, as hipcc -D flags (the JIT key).
std::string jit_spec_string(const KArgs& a, bool lds_state, uint32_t klog) {
    char buf[1024];
    std::snprintf(buf, sizeof buf,
                  "-DAF_JIT=1 -DAF_JIT_LDS=%d -DAF_JIT_KLOG=%u -DAF_JIT_METRICS=%u -DAF_JIT_GEN_EDGE=%u -DAF_JIT_CLIENT_EDGE=%u "
                  "-DAF_JIT_N_EDGES=%u -DAF_JIT_N_SERVERS=%u -DAF_JIT_LB_ALGO=%u -DAF_JIT_N_LB=%u -DAF_JIT_N_ROWS=%u "
                  "-DAF_JIT_N_EMARKS=%u -DAF_JIT_N_SMARKS=%u -DAF_JIT_ORDER_ALL=%u -DAF_JIT_OFF_EDGE=%u -DAF_JIT_OFF_SRV=%u "
                  "-DAF_JIT_OFF_EP=%u -DAF_JIT_OFF_ROW=%u -DAF_JIT_OFF_EMARK=%u -DAF_JIT_OFF_SMARK=%u -DAF_JIT_OFF_LB=%u "
                  "-DAF_JIT_BLOB_BYTES=%u -DAF_JIT_CAP=%u -DAF_JIT_FCAP=%u -DAF_JIT_OVR_MASK=%u "
                  "-DAF_JIT_HAS_CLOCK=%d -DAF_JIT_HAS_SAMPLES=%d -DAF_JIT_HAS_ONLINE=%d",
                  lds_state ? 1 : 0, klog, a.metrics_mask, a.gen_out_edge, a.client_out_edge, a.n_edges, a.n_servers, a.lb_algo,
                  a.n_lb_edges, a.n_rows, a.n_edge_marks, a.n_srv_marks, a.every_event_in_order, a.off_edge, a.off_srv, a.off_ep,
                  a.off_row, a.off_emark, a.off_smark, a.off_lb, a.blob_bytes, a.L.cap, a.L.fcap, a.L.ovr_mask,
                  a.clock ? 1 : 0, a.samples ? 1 : 0, (a.online_hist || a.online_rps) ? 1 : 0);
    return buf;
}

// Experiment hook (AF_WAVES_PER_CU=k): ask for more LDS per workgroup than it needs so that at most k waves fit a
// CU.  Measured on MI355X (10 000 LB-2 replicas): capping the stage-parallel kernel at 14 waves per CU -- three
// equal residency rounds instead of 16 + 16 + a partial one -- is SLOWER (81.6 vs 73.7 ms): the partial round already
// runs faster per wave (4 096 scenarios 30.1 ms, 8 192: 58.0 ms, 10 000: 73.7 ms), so the default pads nothing.
uint32_t spread_lds_bytes(uint32_t need_bytes) {
    if (const char* env = std::getenv("AF_WAVES_PER_CU")) {
        const uint32_t k = (uint32_t)std::atoi(env);
        if (k != 0u) {
            const uint32_t b = (kLdsLimit / k) & ~511u;
            return b > need_bytes ? b : need_bytes;
        }
    }
    return need_bytes;
}

uint32_t chunk_size(const af_engine* e, uint32_t n, size_t draw_bytes_per_scen, size_t mem_free) {
    // (one launch per chunk, and every launch ends with a latency-bound tail: chunks are a last resort)
    size_t budget = e->draw_memory_bytes ? e->draw_memory_bytes : (size_t)160 << 30;
    const size_t avail = mem_free + e->draws_cap;
    if (budget > avail / 10u * 6u) budget = avail / 10u * 6u;
    uint32_t chunk = (uint32_t)(budget / draw_bytes_per_scen < 65535u ? budget / draw_bytes_per_scen : 65535u);
    if (chunk == 0) return 0u;
    if (chunk > n) chunk = n;
    const uint32_t n_chunks = (n + chunk - 1u) / chunk;
    return (n + n_chunks - 1u) / n_chunks;  // equal chunks: no short, latency-bound tail launch
}

// An engine-owned device buffer, grown on demand (the contents are lost then) and kept until the engine is destroyed.
int reserve_device(void** ptr, size_t& cap, size_t need) {
    if (need <= cap) return AF_OK;
    if (*ptr) HIP_TRY(hipFree(*ptr));
    *ptr = nullptr;
    cap = 0;
    HIP_TRY(hipMalloc(ptr, need));
    cap = need;
    return AF_OK;
}

uint32_t klog_of(uint32_t lanes) {
    uint32_t klog = 0;
    while ((1u << klog) < lanes) ++klog;
    return klog;
}

// The columns a sweep overrides, as bits.  (Only a run reads the values: af_engine_jit_spec looks at them on the
// stage-parallel path alone.)
int sweep_override_mask(const af_sweep_t* sweep, bool values_required, uint32_t& mask) {
    mask = 0;
    for (uint32_t k = 0; k < sweep->n_overrides; ++k) {
        const af_override_t& o = sweep->overrides[k];
        if (o.param >= AF_PARAM_COUNT_ || (values_required && !o.values)) return fail(AF_ERR_INVALID, "bad override");
        mask |= 1u << o.param;
    }
    return AF_OK;
}

// pre-generated draws per stream and scenario
int draws_per_stream(const af_sweep_t* sweep, const af_outputs_t* out, uint32_t& n_draw) {
    n_draw = sweep->draw_capacity ? sweep->draw_capacity : out->clock_capacity;
    if (n_draw == 0) return fail(AF_ERR_INVALID, "draw_capacity (or clock_capacity) must be > 0");
    return AF_OK;
}


// ---- stage-parallel kernel: what one af_engine_run launches -------------------------------------------------
// Does this sweep run on the stage-parallel kernel?  flow_mode 0: whenever the plan is in its range; 2 = the same, but a sweep
// it cannot be sized for is an error instead of a fall-back; 1 = never.
// (Round 3 sent plans with general servers -- several endpoints per server, core re-entry -- there only as sweeps of <= 8
// scenarios: the event-by-event station handed 42 % of the two-endpoint LB-2 scenarios back at T = 600 s and ran at 3 waves
// per CU.  Round 4: shared instants are resolved in the station (Flow::gs_instant: no hand-backs on that plan) and the first
// launch needs 17.6 instead of 41 KB of LDS per wave: 512 / 10 000 / 40 000 scenarios x 600 s take 0.30 / 1.52 / 5.46 s against
// 1.48 / 2.45 / 13.35 s on the next-event kernels -- profiles/r04/gensrv_*.json -- so they take it at every sweep size.)
static bool flow_wanted(const af_engine_t* e, uint32_t n_scenarios) {
    (void)n_scenarios;
    return e->flow_ok && e->flow_mode != 1u;
}

// load (users x requests per minute) of the scenarios [lo, lo + nc) of a sweep: its users / rpm columns, else the plan's means
static std::vector<double> chunk_loads(const af_engine_t* e, const af_sweep_t* sweep, uint32_t lo, uint32_t nc) {
    const double* users = nullptr;
    const double* rpm = nullptr;
    for (uint32_t k = 0; k < sweep->n_overrides; ++k) {
        const af_override_t& o = sweep->overrides[k];
        if (o.param == AF_PARAM_GEN_USERS_MEAN) users = o.values + lo;
        else if (o.param == AF_PARAM_GEN_RPM_MEAN) rpm = o.values + lo;
    }
    std::vector<double> load(nc);
    for (uint32_t i = 0; i < nc; ++i) load[i] = (users ? users[i] : e->users_mean) * (rpm ? rpm[i] : e->rpm_mean);
    return load;
}
// launch order of a chunk's scenarios for sweeps with a users / rpm column: heaviest first (stable)
static std::vector<uint32_t> heaviest_first(const af_engine_t* e, const af_sweep_t* sweep, uint32_t lo, uint32_t nc) {
    const std::vector<double> load = chunk_loads(e, sweep, lo, nc);
    std::vector<uint32_t> order(nc);
    for (uint32_t i = 0; i < nc; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return load[x] > load[y]; });
    return order;
}
// Sweeps with a users / rpm column: does af_arrival_groups still pay?  Its workgroup is as slow as its heaviest scenario (the
// chain wave walks that scenario's draws; the lighter lanes idle, the producers skip them) and the kernel as slow as its slowest
// workgroup -- one per CU, all resident --, so its time follows the HEAVIEST scenario of the chunk whatever the others are,
// while the row kernel's follows the TOTAL number of draws at about twice the cost per draw.
// Measured (MI355X): config 3 (users 10 .. 1000, heaviest / mean = 1.98): rows 14.8 ms, groups 11.3 ms; config 4: 103 -> 90 ms.
static bool load_spread_suits_groups(const af_engine_t* e, const af_sweep_t* sweep, uint32_t lo, uint32_t nc) {
    double sum = 0.0, heaviest = 0.0;
    for (const double load : chunk_loads(e, sweep, lo, nc)) {
        heaviest = load > heaviest ? load : heaviest;
        sum += load;
    }
    return heaviest * (double)nc <= 2.5 * sum;
}

struct FlowPlan {
    aff::FlowLayout FL{}, FL2{};   // first launch; second chance (long lists with send times)
    bool big = false;              // the first launch already runs the long-list instantiation
    bool far = false;              // the tick ring does not reach the slowest message: a FEAT_FAR instantiation
    uint32_t big_caps[4] = {256u, 256u, 256u, 256u};
    uint32_t lds = 0;              // bytes of LDS per wave of the first launch
    uint32_t ipl = 1u, feat = 0u;  // instantiation of the first launch
    bool lean = false;
    bool gen_compact = false;      // general servers, first launch: long-list instantiation WITHOUT send times, lists sized by the load
};

// List capacity and tick ring from what will be in flight at the heaviest point of the sweep, the instantiation
// (IPL, FEAT) that covers the launch.  Shared by af_engine_run and af_engine_jit_spec (the plan-specialised build
// bakes exactly this in).
int plan_flow(const af_engine* e, const KArgs& a, const af_sweep_t* sweep, const af_outputs_t* out, FlowPlan& P) {
    const uint32_t n = sweep->n_scenarios;
    aff::FlowLayout& FL = P.FL;
    aff::FlowLayout& FL2 = P.FL2;
    bool& flow_big = P.big;
    bool& flow_far = P.far;
    uint32_t (&big_caps)[4] = P.big_caps;
    uint32_t& flow_lds = P.lds;
    double users = e->users_mean, rpm = e->rpm_mean, ram_mb_scale = 1.0, spike_extra = 0.0;
    uint32_t cores_max = e->cores_max, cores_min = e->cores_max;
    std::vector<double> emean = e->edge_mean;
    for (uint32_t k = 0; k < sweep->n_overrides; ++k) {
        const af_override_t& o = sweep->overrides[k];
        double mx = o.values[0];
        for (uint32_t i = 1; i < n; ++i) mx = o.values[i] > mx ? o.values[i] : mx;
        if (o.param == AF_PARAM_GEN_USERS_MEAN) users = mx;
        else if (o.param == AF_PARAM_GEN_RPM_MEAN) rpm = mx;
        else if (o.param == AF_PARAM_EDGE_MEAN) emean[o.index] = mx;
        else if (o.param == AF_PARAM_SRV_CORES) {
            double mn = o.values[0];
            for (uint32_t i = 1; i < n; ++i) mn = o.values[i] < mn ? o.values[i] : mn;
            cores_max = std::max(cores_max, (uint32_t)mx);
            cores_min = std::min(cores_min, (uint32_t)mn);
        } else if (o.param == AF_PARAM_SRV_RAM_MB) ram_mb_scale = std::max(ram_mb_scale, mx / std::max(e->srv_ram_mb[o.index], 1e-9));
        else if (o.param == AF_PARAM_EMARK_DELTA && mx > 0.0) spike_extra += mx;   // (an upper bound: every swept spike on every hop)
    }
    std::vector<double> edge_spike = e->edge_spike;
    for (double& sp : edge_spike) sp += spike_extra;
    // per-server rings: core releases of the widest server of the sweep, departures of as many requests as its RAM admits
    uint32_t g_ring = e->fargs.L.g_ring, c_ring = std::max(e->fargs.L.c_ring, cores_max);
    if (ram_mb_scale > 1.0) {
        const double lim = a.n_servers <= 4u ? 256.0 : 128.0;
        const double want = std::min(lim, std::ceil((double)g_ring * ram_mb_scale));
        g_ring = aff::pow2_ge((uint32_t)want);
    }
    if (c_ring > 64u) return fail(AF_ERR_CAPACITY, "cpu_cores column: the stage-parallel kernel handles at most 64 cores per server");
    const double sd = e->users_dist == AF_DIST_POISSON ? std::sqrt(users > 0.0 ? users : 0.0) : e->users_sigma;
    const double rate = (users + 4.0 * sd) * rpm / 60.0 + 1e-9;
    auto lat_mean = [&](int32_t ed) {
        const double m = emean[ed], sg = e->edge_sigma[ed];
        switch (e->edge_dist[ed]) {
            case AF_DIST_LOG_NORMAL: return std::exp(m + 0.5 * sg * sg < 50.0 ? m + 0.5 * sg * sg : 50.0);
            case AF_DIST_NORMAL: return (m > 0.0 ? m : 0.0) + 0.4 * sg;
            case AF_DIST_UNIFORM: return 0.5;
            case AF_DIST_POISSON: return m + 0.5;   // whole seconds: what is in flight is at least the next second's worth
            default: return m;
        }
    };
    // the hops of the request path: generator edge, client edge, the slowest LB edge, the slowest server out-edge
    std::vector<int32_t> hops = {e->gen_edge, e->client_edge};
    auto slowest = [&](const std::vector<int32_t>& es) {
        int32_t best = -1;
        for (int32_t ed : es)
            if (best < 0 || lat_mean(ed) + edge_spike[ed] > lat_mean(best) + edge_spike[best]) best = ed;
        return best;
    };
    if (!e->lb_edges.empty()) hops.push_back(slowest(e->lb_edges));
    hops.push_back(slowest(e->srv_out_edge));
    // time in a server: service + the M/D/1 wait for a core at the heaviest load of the sweep
    const double n_active = e->has_lb ? (double)(e->lb_edges.size() > 1 && a.n_srv_marks ? e->lb_edges.size() - 1 : e->lb_edges.size()) : 1.0;
    const double rho = rate / n_active * e->cpu_max / (double)cores_min;
    const double wait = rho < 0.9 ? rho * e->cpu_max / (2.0 * (1.0 - rho)) : 20.0 * e->cpu_max + 1.0;
    const double in_server = e->service_max + 4.0 * wait;
    // messages pending at a station ~ rate x time in flight towards it (the completion list also holds the server time)
    // (a spiked edge: the station behind it runs ahead by the spike while it lasts -- Flow::send_floor -- but when it
    // ends, the messages still in flight and the ones sent after it interleave: rate x spike of them wait there, and
    // the servers then work off that burst, so as many wait for their departure in the completion list)
    double pend = 0.0, burst = 0.0;
    std::vector<double> pend_of(hops.size(), 0.0);
    for (size_t h = 0; h < hops.size(); ++h) {
        const double fly = lat_mean(hops[h]) + edge_spike[hops[h]] + (h + 1 == hops.size() ? in_server : 0.0);
        burst = std::fmax(burst, rate * edge_spike[hops[h]]);
        pend_of[h] = rate * fly;
        pend = std::fmax(pend, rate * fly);
    }
    if (burst > 16.0)   // (millisecond spikes -- BASELINE config 4 -- change nothing a 64-entry list would notice)
        pend_of.back() = std::fmax(pend_of.back(), burst + rate * (lat_mean(hops.back()) + in_server));
    pend = std::fmax(pend, pend_of.back());
    // capacities of the four station lists for the FEAT_BIGLIST instantiation (hops -> lists: generator edge -> 0,
    // client edge -> 1 with a load balancer else 2, LB edges -> 2, server out-edges -> 3)
    {
        for (uint32_t s = 0; s < 4u; ++s) big_caps[s] = (s == 1u && !e->has_lb) ? 64u : 256u;   // (no LB: its list stays empty)
        for (size_t h = 0; h < hops.size(); ++h) {
            const uint32_t s = h == 0 ? 0u : h + 1 == hops.size() ? 3u : (h == 1 && e->has_lb && e->flow_lb_pos == 0u) ? 1u : 2u;
            const double want = 1.5 * pend_of[h] + 128.0;
            const uint32_t c = want < 16384.0 ? ((uint32_t)want + 63u) & ~63u : 16384u;   // any multiple of 64
            if (c > big_caps[s]) big_caps[s] = c;
        }
        if (e->flow_lb_pos != 0u && big_caps[2] > big_caps[1]) big_caps[1] = big_caps[2];   // (servers in front of the LB: the same load passes its list)
    }
    // A list only has to leave ROOM: 64 - pending new messages fit per round.  Larger lists cost LDS (occupancy) and
    // ranking work on every round of every scenario (measured on the config-3 grid: 64 entries 122 ms, 128 entries
    // 144 ms, no hand-backs either way); an overflow costs one scenario a second run.  `pend` is the MEAN at the
    // heaviest point of the sweep: half a list of pending messages still leaves half a batch of room.
    uint32_t entries = e->flow_list_entries;
    if (entries == 0u) {
        entries = pend <= 32.0 ? 64u : pend <= 96.0 ? 128u : 256u;
        flow_big = pend > 200.0;   // more than register-resident lists hold: the whole launch on the long-list instantiation
    }
    // What the tick ring has to reach past its window.  With FEAT_FAR: the time a request spends INSIDE a server (its
    // queue / step / RAM intervals are entered when it arrives); a delivery the ring does not reach is entered by the
    // receiving station (af_flow.hpp, "Sampled series").  Without: the in-flight time of the slowest message of the
    // sweep (~1e-11 per request) -- the largest single hop at that quantile, the other hops at mean + 3 sd, spikes.
    auto lat_sd = [&](int32_t ed) {
        const double m = emean[ed], sg = e->edge_sigma[ed];
        switch (e->edge_dist[ed]) {
            case AF_DIST_LOG_NORMAL: {
                const double v = sg * sg < 50.0 ? sg * sg : 50.0;
                return lat_mean(ed) * std::sqrt(std::exp(v) - 1.0);
            }
            case AF_DIST_NORMAL: return sg;
            case AF_DIST_UNIFORM: return 0.29;
            case AF_DIST_POISSON: return std::sqrt(m > 0.0 ? m : 0.0);
            default: return m;
        }
    };
    auto lat_q = [&](int32_t ed) {   // a transit time one message in ~1e11 exceeds
        const double m = emean[ed], sg = e->edge_sigma[ed];
        switch (e->edge_dist[ed]) {
            case AF_DIST_LOG_NORMAL: return std::exp(m + 6.7 * sg < 50.0 ? m + 6.7 * sg : 50.0);
            case AF_DIST_NORMAL: return (m > 0.0 ? m : 0.0) + 6.7 * sg;
            case AF_DIST_UNIFORM: return 1.0;
            case AF_DIST_POISSON: return m + 7.0 * std::sqrt(m > 0.0 ? m : 0.0) + 12.0;   // (Poisson tail beyond 1e-11)
            default: return 25.3 * m;
        }
    };
    double tail_full = in_server;
    {
        size_t worst = 0;
        for (size_t h = 1; h < hops.size(); ++h)
            if (lat_q(hops[h]) > lat_q(hops[worst])) worst = h;
        for (size_t h = 0; h < hops.size(); ++h)
            tail_full += edge_spike[hops[h]] + (h == worst ? lat_q(hops[h]) : lat_mean(hops[h]) + 3.0 * lat_sd(hops[h]));
    }
    const double tail = in_server;
    uint32_t rows = e->flow_ring_rows, win_rows = 0u;
    const uint32_t pitch = a.series_pitch;
    const double tail_rows = std::ceil(tail / a.sample_period) + 2.0;
    if (out->samples == nullptr) {
        rows = 0u;    // no series: neither ring nor rows are touched
    } else if (rows == AF_FLOW_RING_IN_HBM) {
        rows = 0u;
    } else if (rows == 0u) {
        // the ring covers the generator's window (enough ticks for a full batch of arrivals at the heaviest load,
        // at least 8) + the server time; 8 KB of LDS keep 16 waves per CU, 24 KB are the limit before HBM takes over
        const double want_win = std::fmin(std::fmax(std::ceil(96.0 / rate / a.sample_period), 8.0), 4096.0);
        const uint32_t cap_pref = aff::pow2_ge(8u * 1024u / (pitch * 4u) + 1u) / 2u, cap_max = aff::pow2_ge(24u * 1024u / (pitch * 4u) + 1u) / 2u;
        if (tail_rows + 8.0 > (double)cap_max) {
            rows = 0u;   // a request stays in its server longer than any ring that fits reaches: differences in HBM
        } else {
            rows = aff::pow2_ge((uint32_t)(tail_rows + want_win));
            if (rows > cap_pref) rows = cap_pref >= aff::pow2_ge((uint32_t)(tail_rows + 8.0)) ? cap_pref : aff::pow2_ge((uint32_t)(tail_rows + 8.0));
            if (rows < 16u) rows = 16u;
            // a window of two or three batches binds less often: take it where it costs no occupancy (16 waves per CU
            // leave 10 KB each)
            if (!flow_big) {
                const uint32_t no_ring = a.blob_bytes + aff::make_flow_layout(entries, 0u, g_ring, c_ring, a.n_edges,
                                                                              a.n_servers, a.n_edge_marks).n_words * 8u;
                while (rows < aff::pow2_ge((uint32_t)(tail_rows + 2.0 * want_win)) && no_ring + 2u * rows * pitch * 4u <= 10u * 1024u) rows *= 2u;
            }
        }
    } else {
        rows = aff::pow2_ge(rows);
    }
    if (rows != 0u) {
        const double full_rows = std::ceil(tail_full / a.sample_period) + 2.0;
        flow_far = (double)rows - full_rows < std::fmin(8.0, (double)(rows / 2u)) || std::getenv("AF_FLOW_FORCE_FAR") != nullptr;   // (env: experiment hook)
        const double w = (double)rows - (flow_far ? tail_rows : full_rows);
        win_rows = w >= (double)(rows / 2u) ? (uint32_t)w : rows / 2u;   // an explicit small ring: half of it, overflow -> hand-back
    }
    // long lists have to fit the LDS of a compute unit next to everything else: halve the longest until they do
    const bool gen_srv = e->flow_general_servers;   // several endpoints per server / programs that come back to the core queue
    auto big_layout = [&](uint32_t ring) {
        aff::FlowLayout L = aff::make_flow_layout(0u, ring, g_ring, c_ring, a.n_edges, a.n_servers, a.n_edge_marks, true, big_caps, gen_srv);
        while (a.blob_bytes + L.n_words * 8u > kLdsLimit) {
            uint32_t m = 0;
            for (uint32_t s = 1; s < 4u; ++s)
                if (big_caps[s] > big_caps[m]) m = s;
            if (big_caps[m] <= 256u) break;
            big_caps[m] = (big_caps[m] / 2u + 63u) & ~63u;
            L = aff::make_flow_layout(0u, ring, g_ring, c_ring, a.n_edges, a.n_servers, a.n_edge_marks, true, big_caps, gen_srv);
        }
        return L;
    };
    // General servers, first launch (round 4): the station is one busy lane per server -- a chain of dependent LDS round trips --
    // so what the launch needs is WAVES per compute unit, i.e. little LDS per wave: lists of what the load needs (>= 128
    // entries: a batch of 64 must find room) without the send times of the second-chance form, instead of 4 x 256 x 3 words:
    // 41 -> ~20 KB per wave, 3 -> 7 waves per CU.  What overflows or ties is caught by the second chance (FL2), as ever.
    P.gen_compact = gen_srv && !flow_big && std::getenv("AF_FLOW_GEN_ROBUST_FIRST") == nullptr;   // (env: measurement hook)
    if (gen_srv) flow_big = true;   // (the general server station exists in the long-list instantiations only)
    if (P.gen_compact) {
        uint32_t caps1[4];
        // (64 entries where little is pending -- what the tandem kernel's lists hold for the same load --, 128 for the completion
        // list: it takes a whole round's departures of every server at once)
        for (uint32_t s = 0; s < 4u; ++s) caps1[s] = s == 3u ? 128u : 64u;
        for (size_t h = 0; h < hops.size(); ++h) {
            const uint32_t s = h == 0 ? 0u : h + 1 == hops.size() ? 3u : (h == 1 && e->has_lb && e->flow_lb_pos == 0u) ? 1u : 2u;
            const double want = pend_of[h] <= 24.0 ? 64.0 : 1.5 * pend_of[h] + 64.0;
            const uint32_t c = want < 1024.0 ? ((uint32_t)want + 63u) & ~63u : 1024u;
            if (c > caps1[s]) caps1[s] = c;
        }
        if (rows * pitch * 4u > 4u * 1024u) {
            rows = 0u;
            win_rows = 0u;
        }
        // (servers in front of the LB: its list takes a whole round's departures of the server that feeds it, like the completion list)
        // (servers that feed servers: the ONE server list holds the messages bound for every level)
        if (e->flow_chain) caps1[2] = std::max(caps1[2], 128u);
        if (e->flow_lb_pos != 0u) caps1[1] = std::max({caps1[1], caps1[2], 128u});
        FL = aff::make_flow_layout(0u, rows, g_ring, c_ring, a.n_edges, a.n_servers, a.n_edge_marks, false, caps1, true);
    } else if (flow_big) {
        if (rows * pitch * 4u > 8u * 1024u) {   // the lists need the LDS more than the tick ring does
            rows = 0u;
            win_rows = 0u;
        }
        FL = big_layout(rows);
    } else {
        FL = aff::make_flow_layout(entries, rows, g_ring, c_ring, a.n_edges, a.n_servers, a.n_edge_marks);
    }
    FL.win_rows = win_rows;
    FL2 = big_layout(0u);   // second chance: tick differences in HBM (no reach limit)
    FL2.win_rows = 0u;
    flow_lds = a.blob_bytes + FL.n_words * 8u;
    if (flow_lds > kLdsLimit) return fail(AF_ERR_CAPACITY, "flow kernel layout exceeds the LDS of a compute unit");

    // the leanest instantiation that covers this launch (a compiled-in feature costs wave-uniform registers)
    const bool lc = e->fargs.lb_least_connections != 0u;
    const bool has_online = out->online_hist != nullptr || out->online_rps != nullptr;
    const bool ring_ok = FL.ring_rows != 0u || out->samples == nullptr;
    const bool lean = a.n_edge_marks == 0u && a.n_srv_marks == 0u && !has_online && ring_ok;
    // injected spikes / outages, but neither the kernel-side summary nor tick differences in HBM (BASELINE config 4)
    const bool marks_only = !lean && !has_online && ring_ok;
    constexpr uint32_t kRobust = aff::FEAT_ALL | aff::FEAT_TIEBREAK | aff::FEAT_BIGLIST;
    const bool chain = e->flow_chain;
    P.lean = lean && !flow_big && !lc && !chain;
    if (P.gen_compact) {
        P.ipl = 1u;
        P.feat = aff::FEAT_ALL | aff::FEAT_BIGLIST | aff::FEAT_GENSRV | (lc ? (uint32_t)aff::FEAT_LC : 0u) | (chain ? (uint32_t)aff::FEAT_CHAIN : 0u);
    } else if (flow_big) {
        P.ipl = 1u;
        P.feat = kRobust | (lc ? (uint32_t)aff::FEAT_LC : 0u) | (gen_srv ? (uint32_t)aff::FEAT_GENSRV : 0u) | (chain ? (uint32_t)aff::FEAT_CHAIN : 0u);
    } else if (chain) {   // one generic instantiation per list length (every optional feature in); the plan-specialised build is the same FEAT
        P.ipl = FL.cap == 64u ? 1u : FL.cap == 128u ? 2u : 4u;
        P.feat = aff::FEAT_ALL | aff::FEAT_CHAIN | (lc ? (uint32_t)aff::FEAT_LC : 0u);
    } else if (lc) {
        P.ipl = FL.cap == 64u ? 1u : FL.cap == 128u ? 2u : 4u;
        P.feat = aff::FEAT_ALL | aff::FEAT_LC;
    } else if (FL.cap == 64u || FL.cap == 128u) {
        P.ipl = FL.cap / 64u;
        P.feat = lean ? (flow_far ? (uint32_t)aff::FEAT_FAR : 0u) : marks_only ? (uint32_t)(aff::FEAT_MARKS | aff::FEAT_FAR) : (uint32_t)aff::FEAT_ALL;
    } else {
        P.ipl = 4u;
        P.feat = aff::FEAT_ALL;
    }
    return AF_OK;
}

// the library's own (generic) instantiation for (ipl, feat); nullptr = not built
const void* flow_kernel_for(uint32_t ipl, uint32_t feat) {
    constexpr uint32_t kRobust = aff::FEAT_ALL | aff::FEAT_TIEBREAK | aff::FEAT_BIGLIST, kLC = aff::FEAT_LC, kAll = aff::FEAT_ALL;
    constexpr uint32_t kFar = aff::FEAT_FAR, kMarksFar = aff::FEAT_MARKS | aff::FEAT_FAR;
#define AF_FLOW_CASE(I, F) if (ipl == (I) && feat == (F)) return reinterpret_cast<const void*>(af_flow_kernel<(I), (F)>)
    AF_FLOW_CASE(1u, kRobust | kLC);
    AF_FLOW_CASE(1u, kRobust);
    AF_FLOW_CASE(1u, kRobust | kLC | (uint32_t)aff::FEAT_GENSRV);
    AF_FLOW_CASE(1u, kRobust | (uint32_t)aff::FEAT_GENSRV);
    AF_FLOW_CASE(1u, kAll | (uint32_t)aff::FEAT_BIGLIST | (uint32_t)aff::FEAT_GENSRV);          // general servers, first launch (compact lists)
    AF_FLOW_CASE(1u, kAll | (uint32_t)aff::FEAT_BIGLIST | (uint32_t)aff::FEAT_GENSRV | kLC);
    AF_FLOW_CASE(1u, kAll | (uint32_t)aff::FEAT_BIGLIST | (uint32_t)aff::FEAT_GENSRV | (uint32_t)aff::FEAT_CHAIN);   // general servers in tiers
    AF_FLOW_CASE(1u, kRobust | (uint32_t)aff::FEAT_GENSRV | (uint32_t)aff::FEAT_CHAIN);
    AF_FLOW_CASE(1u, kAll | (uint32_t)aff::FEAT_BIGLIST | (uint32_t)aff::FEAT_GENSRV | kLC | (uint32_t)aff::FEAT_CHAIN);
    AF_FLOW_CASE(1u, kRobust | (uint32_t)aff::FEAT_GENSRV | kLC | (uint32_t)aff::FEAT_CHAIN);
    AF_FLOW_CASE(1u, kRobust | (uint32_t)aff::FEAT_CHAIN);   // servers that feed servers: the second-chance form and one per list length
    AF_FLOW_CASE(1u, kAll | (uint32_t)aff::FEAT_CHAIN);
    AF_FLOW_CASE(2u, kAll | (uint32_t)aff::FEAT_CHAIN);
    AF_FLOW_CASE(4u, kAll | (uint32_t)aff::FEAT_CHAIN);
    AF_FLOW_CASE(1u, kRobust | kLC | (uint32_t)aff::FEAT_CHAIN);   // ... behind a least-connections LB
    AF_FLOW_CASE(1u, kAll | kLC | (uint32_t)aff::FEAT_CHAIN);
    AF_FLOW_CASE(2u, kAll | kLC | (uint32_t)aff::FEAT_CHAIN);
    AF_FLOW_CASE(4u, kAll | kLC | (uint32_t)aff::FEAT_CHAIN);
    AF_FLOW_CASE(1u, kAll | kLC);
    AF_FLOW_CASE(2u, kAll | kLC);
    AF_FLOW_CASE(4u, kAll | kLC);
    AF_FLOW_CASE(1u, kFar);
    AF_FLOW_CASE(1u, 0u);
    AF_FLOW_CASE(1u, kMarksFar);
    AF_FLOW_CASE(1u, kAll);
    AF_FLOW_CASE(2u, kFar);
    AF_FLOW_CASE(2u, 0u);
    AF_FLOW_CASE(2u, kMarksFar);
    AF_FLOW_CASE(2u, kAll);
    AF_FLOW_CASE(4u, kAll);
#undef AF_FLOW_CASE
    return nullptr;
}

// Everything the plan-specialised stage-parallel kernel bakes in, as hipcc -D flags (the JIT key).
std::string flow_jit_spec_string(const af_engine* e, const FlowPlan& P, const af_outputs_t* out, bool has_ovr) {
    const aff::FlowArgs& f = e->fargs;
    const aff::FlowLayout& L = P.FL;
    auto bits = [](double v) {
        uint64_t u;
        std::memcpy(&u, &v, 8);
        return (unsigned long long)u;
    };
    uint32_t dist_all = e->edge_dist.empty() ? 255u : e->edge_dist[0];     // the ONE latency law of every edge, else 255
    for (uint8_t d : e->edge_dist)
        if (d != dist_all) dist_all = 255u;
    // (measured, round 3: the constant pays for the laws behind the call -- BASELINE config 5, log-normal: 245.4 -> 235.5 ms per
    // 50 000 replicas -- but NOT for the exponential law, whose variate is inline anyway: without the call site the compiler
    // allocates 72 instead of 110 VGPRs and the kernel is 6 % SLOWER (48.5 -> 51.6 ms on config 2), five waves per SIMD included)
    if ((dist_all == AF_DIST_EXPONENTIAL && !std::getenv("AF_FLOW_DIST_CONST_EXP")) || std::getenv("AF_FLOW_NO_DIST_CONST")) dist_all = 255u;
    // waves per SIMD the LDS of this launch admits (160 KB per compute unit, four SIMDs): the register budget to compile for
    uint32_t wpe = 4u;
    if (const char* env = std::getenv("AF_FLOW_JIT_WPE")) {   // (measurement hook; anything outside 1..8 is ignored)
        const int v = std::atoi(env);
        if (v >= 1 && v <= 8) wpe = (uint32_t)v;
    } else {
        const uint32_t lds_alloc = (P.lds + 511u) & ~511u, per_cu = lds_alloc ? (160u * 1024u) / lds_alloc : 16u;
        wpe = (per_cu + 3u) / 4u;
        wpe = wpe < 2u ? 2u : wpe > 4u ? 4u : wpe;
        // general servers: the kernel also holds gen_servers_par's walk and top-c arrays -- 128 registers (four waves) would
        // spill them; the generic instantiation and round 4's measurements are at three
        if ((P.feat & (uint32_t)aff::FEAT_GENSRV) != 0u && wpe > 3u) wpe = 3u;
    }
    char buf[2048];
    std::snprintf(buf, sizeof buf,
                  "-DAF_JIT=1 -DAF_FLOW_JIT=1 -DAF_FJ_IPL=%u -DAF_FJ_FEAT=%u -DAF_FJ_TOTAL_TIME=0x%llxull -DAF_FJ_PERIOD=0x%llxull "
                  "-DAF_FJ_INV_PERIOD=0x%llxull -DAF_FJ_TICK_EPS=0x%llxull -DAF_FJ_METRICS=%u -DAF_FJ_GEN_EDGE=%u -DAF_FJ_CLIENT_EDGE=%u "
                  "-DAF_FJ_N_EDGES=%u -DAF_FJ_N_SERVERS=%u -DAF_FJ_HAS_LB=%u -DAF_FJ_N_LB=%u -DAF_FJ_N_EMARKS=%u -DAF_FJ_N_SMARKS=%u "
                  "-DAF_FJ_LC=%u -DAF_FJ_MAX_PRE=%u -DAF_FJ_MAX_CPU=%u -DAF_FJ_MAX_POST=%u -DAF_FJ_OFF_EDGE=%u -DAF_FJ_OFF_SRV=%u "
                  "-DAF_FJ_OFF_EP=%u -DAF_FJ_OFF_ROW=%u -DAF_FJ_OFF_EMARK=%u -DAF_FJ_OFF_SMARK=%u -DAF_FJ_OFF_LB=%u -DAF_FJ_BLOB_BYTES=%u "
                  "-DAF_FJ_N_TICKS=%u -DAF_FJ_HAS_CLOCK=%d -DAF_FJ_HAS_SAMPLES=%d -DAF_FJ_HAS_ONLINE=%d -DAF_FJ_HAS_OVR=%d -DAF_FJ_DIST_ALL=%u -DAF_FJ_RAM_SCALE=%.1f "
                  "-DAF_FJ_N_LEVELS=%u -DAF_FJ_LB_POS=%u -DAF_FJ_WPE=%u -DAF_FJ_LAYOUT=%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u",
                  P.ipl, P.feat | (std::getenv("AF_FLOW_PROF") ? (uint32_t)aff::FEAT_PROF : 0u), bits(f.total_time), bits(f.sample_period), bits(f.inv_period), bits(f.tick_eps), f.metrics_mask,
                  f.gen_out_edge, f.client_out_edge, f.n_edges, f.n_servers, f.has_lb, f.n_lb_edges, f.n_edge_marks, f.n_srv_marks,
                  f.lb_least_connections, f.max_pre, f.max_cpu, f.max_post, f.off_edge, f.off_srv, f.off_ep, f.off_row, f.off_emark,
                  f.off_smark, f.off_lb, f.blob_bytes, f.n_ticks, out->clock ? 1 : 0, out->samples ? 1 : 0,
                  (out->online_hist || out->online_rps) ? 1 : 0, has_ovr ? 1 : 0, dist_all, f.ram_scale, e->flow_levels, e->flow_lb_pos, wpe,
                  L.cap, L.ring_rows, L.win_rows, L.g_ring, L.c_ring, L.pitch, L.list_arrays, L.off_spike, L.off_list, L.off_aux, L.off_aux3,
                  L.off_out, L.off_sorted, L.off_hist, L.off_seg, L.off_fr, L.off_gr, L.off_cnt, L.off_ring, L.n_words, L.cap_of[0],
                  L.cap_of[1], L.cap_of[2], L.cap_of[3], L.off_list_of[0], L.off_list_of[1], L.off_list_of[2], L.off_list_of[3], L.off_eb, L.off_gsrv);
    std::string spec(buf);
    // Philox's key schedule per call site instead of hoisted (af_flow.hpp: Flow::edge_draw) where it was measured to pay -- the
    // lean form and the forms with timeline marks (configs 2 / 4: 38.2 -> 37.9, 670 -> 653 ms); it costs on the others (FAR alone,
    // config 3: 55.7 -> 56.4; general servers, config 6: 281 -> 293; config 5: nothing): profiles/r05/philox_keys_ab.txt
    const bool keys = (P.feat == 0u || (P.feat & aff::FEAT_MARKS) != 0u) && (P.feat & aff::FEAT_GENSRV) == 0u;
    if (keys && !std::getenv("AF_FLOW_KEYS_HOISTED")) spec += " -DAF_FJ_KEYS_PER_CALL=1";
    // select()'s lane window (af_flow.hpp: AF_SELECT_WINDOW) where it was measured to pay: the lean form (config 2: 43.1 -> 41.8 ms).
    // The forms with FEAT_FAR / timeline marks run plans whose lists are far from sorted (config 3's grid reaches 50 ms edges:
    // the proof fails in most calls) and were slower with it in its first form (config 3 67.1 -> 69.3, config 4 747 -> 772 ms):
    // they keep the bucket rank alone (profiles/r08/ab_select_window.txt)
    if (P.feat != 0u && !std::getenv("AF_FLOW_SELECT_WINDOW_ALL")) spec += " -DAF_SELECT_WINDOW=0";
    // Round 9: the lean form's width per station list (af_flow.hpp: AF_FJ_SELECT_WINDOW_S<list>; a -DAF_SELECT_WINDOW_S<list> on the
    // compiler's command line still comes first).  CONSTANTS, measured on config 2 and not worked out from the plan: four lanes for
    // what the generator and the servers sent, three for what the client and the load balancer sent.  On the host emulator the
    // proof then holds in 92 / 96 / 94 / 95 % of the four lists' calls (99.2 / 100 / 100 / 99.7 % at six lanes), and each lane of
    // width costs every call more than the rare bucket rank costs the few: 42.27 ms per step at 6-6-6-6, 41.70 at 4-4-4-4, 41.57 at
    // 4-3-3-4, 41.61 at 3-3-3-3 (the two are within run-to-run noise of each other), 41.75 at 3-2-2-3, 42.18 at 2-2-2-2
    // (profiles/r09/ab_select_widths.txt).  No rule from the plan's numbers (in-edge latency x offered rate) was tested against
    // other plans, so none is claimed: EVERY plan of the lean form (single server, other topologies) gets these widths, measured
    // on LB-2 alone -- results are the same at any width, only the share of calls that fall back to the bucket rank differs.
    // The library's generic kernels were not measured at other widths and keep AF_SELECT_WINDOW in every list.
    else if (P.feat == 0u)
        spec += " -DAF_FJ_SELECT_WINDOW_S0=4 -DAF_FJ_SELECT_WINDOW_S1=3 -DAF_FJ_SELECT_WINDOW_S2=3 -DAF_FJ_SELECT_WINDOW_S3=4";
    return spec;
}
}  // namespace

extern "C" {

int af_abi_version(void) { return AF_ABI_VERSION; }

const char* af_last_error(void) { return g_err.c_str(); }

uint32_t af_tick_count(double sample_period, double total_time) {
    if (!(sample_period > 0.0)) return 0;
    uint32_t n = 0;
    double t = 0.0 + sample_period;
    while (t < total_time) {
        n += 1;
        t = t + sample_period;
    }
    return n;
}

uint32_t af_series_count(const af_plan_t* plan) { return plan ? plan->n_edges + 3u * plan->n_servers : 0u; }

uint32_t af_series_pitch(const af_plan_t* plan) { return (af_series_count(plan) + 3u) & ~3u; }

int af_engine_create(const af_plan_t* plan, int device, const af_engine_options_t* opts, af_engine_t** out) {
    if (!out) return fail(AF_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (int rc = validate_plan(plan)) return rc;
    // AF_DEVICE_PLAN_ONLY: a planning-only engine -- everything af_engine_jit_spec needs (plan facts, layout heuristics)
    // and no device state: it cannot run, and no HIP call is made on its behalf (build machines without a GPU)
    const bool plan_only = device == AF_DEVICE_PLAN_ONLY;
    if (!plan_only) {
        int n_dev = 0;
        if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0)
            return fail(AF_ERR_NO_DEVICE, "no HIP device visible: the asyncflow_amd engine has no CPU fallback");
        if (device < 0 || device >= n_dev) return fail(AF_ERR_NO_DEVICE, "device index out of range");
        HIP_TRY(hipSetDevice(device));
    }

    af_engine* e = new af_engine();
    e->device = device;
    e->plan_only = plan_only;
    KArgs& a = e->args;
    a.total_time = plan->total_time;
    a.sample_period = plan->sample_period;
    a.gen_users_mean = plan->gen_users_mean;
    a.gen_users_sigma = plan->gen_users_sigma;
    a.gen_rpm_mean = plan->gen_rpm_mean;
    a.gen_window_s = plan->gen_window_s;
    a.metrics_mask = plan->metrics_mask;
    a.gen_users_dist = plan->gen_users_dist;
    a.gen_out_edge = plan->gen_out_edge;
    a.client_out_edge = plan->client_out_edge;
    a.n_edges = plan->n_edges;
    a.n_servers = plan->n_servers;
    a.lb_algo = plan->lb_algo;
    a.n_lb_edges = plan->n_lb_edges;
    a.n_edge_marks = plan->n_edge_marks;
    a.n_srv_marks = plan->n_srv_marks;
    a.every_event_in_order = af::every_event_in_order(*plan) ? 1u : 0u;
    a.n_series = plan->n_edges + 3u * plan->n_servers;
    a.series_pitch = (a.n_series + 3u) & ~3u;

    af::PackedPlan pk;
    const std::string why = af::pack_plan(*plan, pk);
    if (!why.empty()) {
        delete e;
        return fail(AF_ERR_INVALID, why);
    }
    a.n_rows = pk.n_rows;
    a.off_edge = pk.off_edge;
    a.off_srv = pk.off_srv;
    a.off_ep = pk.off_ep;
    a.off_row = pk.off_row;
    a.off_emark = pk.off_emark;
    a.off_smark = pk.off_smark;
    a.off_lb = pk.off_lb;
    a.blob_bytes = (uint32_t)(pk.words.size() * 8u);
    e->row_of_step = pk.row_of_step;
    const std::vector<uint64_t>& blob = pk.words;

    e->request_capacity = opts && opts->request_capacity ? opts->request_capacity : 64u;
    e->fifo_capacity = pow2_at_least(opts && opts->fifo_capacity ? opts->fifo_capacity : 32u);
    e->force_global = opts ? opts->force_global_state : 0u;
    e->lanes_per_wave = opts ? opts->lanes_per_wave : 0u;
    e->draw_memory_bytes = opts ? (size_t)opts->draw_memory_mb << 20 : 0;
    e->shared_instants_likely = (opts && opts->expect_shared_instants != 0u) || a.every_event_in_order != 0u;
    if (e->lanes_per_wave & (e->lanes_per_wave - 1u)) {
        delete e;
        return fail(AF_ERR_INVALID, "lanes_per_wave must be 0 (auto) or a power of two <= 64");
    }
    if (e->lanes_per_wave > 64u) e->lanes_per_wave = 64u;
    // (a server's wait queues have a 32-bit word each since round 6: the cap is what a scenario's state may cost in HBM --
    // 32 bytes per waiter slot and server and queue pair; af_engine_run sizes its pieces by it)
    if (e->request_capacity > 65535u || e->fifo_capacity > AF_MAX_FIFO_CAPACITY) {
        delete e;
        return fail(AF_ERR_CAPACITY, "request_capacity must be <= 65535 and fifo_capacity <= 1048576");
    }
    if (a.blob_bytes > kLdsLimit / 2) {
        delete e;
        return fail(AF_ERR_CAPACITY, "plan too large for the LDS-resident plan blob");
    }

    // ---- stage-parallel kernel: is the plan in its range?  tick table, plan facts for the layout heuristics
    e->flow_mode = opts ? opts->flow_mode : 0u;
    e->flow_list_entries = opts ? opts->flow_list_entries : 0u;
    e->flow_ring_rows = opts ? opts->flow_ring_rows : 0u;
    if (e->flow_list_entries != 0u && e->flow_list_entries != 64u && e->flow_list_entries != 128u && e->flow_list_entries != 256u) {
        delete e;
        return fail(AF_ERR_INVALID, "flow_list_entries must be 0 (auto), 64, 128 or 256");
    }
    e->flow_reason = aff::flow_ineligible_reason(*plan);
    e->flow_ok = e->flow_reason.empty();
    e->flow_general_servers = e->flow_ok && aff::flow_needs_general_servers(*plan);
    e->flow_chain = e->flow_ok && aff::flow_needs_chain(*plan);
    e->flow_levels = e->flow_chain ? aff::flow_server_levels(*plan, nullptr) : 1u;
    e->flow_lb_pos = e->flow_chain ? aff::flow_lb_position(*plan) : 0u;
    e->has_lb = plan->has_lb;
    e->gen_edge = plan->gen_out_edge;
    e->client_edge = plan->client_out_edge;
    e->rpm_mean = plan->gen_rpm_mean;
    e->users_mean = plan->gen_users_mean;
    e->users_sigma = plan->gen_users_sigma;
    e->users_dist = plan->gen_users_dist;
    e->edge_mean.assign(plan->edge_mean, plan->edge_mean + plan->n_edges);
    e->edge_sigma.assign(plan->edge_sigma, plan->edge_sigma + plan->n_edges);
    e->edge_dist.assign(plan->edge_dist, plan->edge_dist + plan->n_edges);
    e->lb_edges.assign(plan->lb_edges, plan->lb_edges + plan->n_lb_edges);
    e->srv_out_edge.assign(plan->srv_out_edge, plan->srv_out_edge + plan->n_servers);
    e->srv_ram_mb.assign(plan->srv_ram_mb, plan->srv_ram_mb + plan->n_servers);
    e->edge_spike.assign(plan->n_edges, 0.0);
    {
        std::vector<double> acc(plan->n_edges, 0.0);
        for (uint32_t i = 0; i < plan->n_edge_marks; ++i) {
            const int32_t ed = plan->emark_edge[i];
            acc[ed] += plan->emark_delta[i];
            if (acc[ed] > e->edge_spike[ed]) e->edge_spike[ed] = acc[ed];
        }
    }
    for (uint32_t sv = 0; sv < plan->n_servers; ++sv) {
        if (plan->srv_cores[sv] > e->cores_max) e->cores_max = plan->srv_cores[sv];
        for (uint32_t ep = plan->srv_ep_begin[sv]; ep < plan->srv_ep_begin[sv + 1]; ++ep) {
            double svc = 0.0, cpu = 0.0;
            for (uint32_t i = plan->ep_step_begin[ep]; i < plan->ep_step_begin[ep + 1]; ++i) {
                svc += plan->step_time[i];
                if (plan->step_kind[i] == AF_STEP_CPU) cpu += plan->step_time[i];
            }
            if (svc > e->service_max) e->service_max = svc;
            if (cpu > e->cpu_max) e->cpu_max = cpu;
        }
    }
    if (e->flow_ok) {
        e->tick = aff::make_tick_table(plan->sample_period, plan->total_time);
        aff::FlowArgs& f = e->fargs;
        f.total_time = plan->total_time;
        f.sample_period = plan->sample_period;
        f.inv_period = e->tick.inv_period;
        f.tick_eps = e->tick.eps;
        f.metrics_mask = plan->metrics_mask;
        f.gen_out_edge = (uint32_t)plan->gen_out_edge;
        f.client_out_edge = (uint32_t)plan->client_out_edge;
        f.n_edges = plan->n_edges;
        f.n_servers = plan->n_servers;
        f.has_lb = plan->has_lb;
        f.n_lb_edges = plan->n_lb_edges;
        f.lb_least_connections = aff::lc_edges(*plan) != 0u ? 1u : 0u;
        f.n_edge_marks = plan->n_edge_marks;
        f.n_srv_marks = plan->n_srv_marks;
        aff::flow_step_maxima(*plan, f.max_pre, f.max_cpu, f.max_post);
        f.ram_scale = aff::flow_ram_scale(*plan);
        f.ram_unit = 1.0 / f.ram_scale;
        f.off_edge = pk.off_edge; f.off_srv = pk.off_srv; f.off_ep = pk.off_ep; f.off_row = pk.off_row;
        f.off_emark = pk.off_emark; f.off_smark = pk.off_smark; f.off_lb = pk.off_lb;
        f.blob_bytes = a.blob_bytes;
        f.n_ticks = (uint32_t)e->tick.t.size();
        f.L = aff::choose_flow_layout(*plan, 1u, 64u);   // g_ring / c_ring; entries and rows are chosen per run
    }

    if (plan_only) {
        *out = e;
        return AF_OK;
    }
    hipError_t err = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
    if (err == hipSuccess && e->flow_ok) err = hipMalloc((void**)&e->d_tick, (e->tick.t.size() + 1u) * 8u);
    if (err == hipSuccess && e->flow_ok && !e->tick.t.empty())
        err = hipMemcpy(e->d_tick, e->tick.t.data(), e->tick.t.size() * 8u, hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMalloc((void**)&e->d_fb, 32u * 4u);
    if (err == hipSuccess) err = hipEventCreate(&e->ev0);
    if (err == hipSuccess) err = hipEventCreate(&e->ev1);
    if (err == hipSuccess) err = hipEventCreate(&e->ev2);
    if (err == hipSuccess) err = hipEventCreate(&e->ev3);
    if (err == hipSuccess) err = hipEventCreate(&e->ev4);
    if (err == hipSuccess) err = hipMalloc((void**)&e->d_n_shared, 4);
    if (err == hipSuccess) err = hipMalloc((void**)&e->d_blob, blob.size() * 8u);
    if (err == hipSuccess) err = hipMemcpy(e->d_blob, blob.data(), blob.size() * 8u, hipMemcpyHostToDevice);
    if (err != hipSuccess) {
        af_engine_destroy(e);
        return fail(AF_ERR_HIP, std::string("engine setup: ") + hipGetErrorString(err));
    }
    a.blob = e->d_blob;
    e->fargs.blob = e->d_blob;
    e->fargs.tick_t = e->d_tick;
    *out = e;
    return AF_OK;
}

constexpr int kSummaryWpe = 8;   // (af_summary.hpp: kWpe; BASELINE config 2, 10 000 scenarios: 4.67 -> 4.28 ms for the analyzer's pair of kernels)

// argument checks shared by af_engine_summarize and af_engine_run_summarized
static int check_summary_request(const af_engine_t* e, const af_outputs_t* out, const af_summary_t* sum) {
    if (!e || !out || !sum) return fail(AF_ERR_INVALID, "NULL argument");
    if (e->plan_only) return fail(AF_ERR_NO_DEVICE, "planning-only engine (AF_DEVICE_PLAN_ONLY)");
    if (sum->n_scenarios == 0) return fail(AF_ERR_INVALID, "empty summary request");
    if (!out->counts) return fail(AF_ERR_INVALID, "outputs.counts is required");
    const bool want_lat = sum->stats || sum->rps || sum->hist;
    const bool want_series = sum->series_mean || sum->series_max;
    if (want_lat && !sum->stats) return fail(AF_ERR_INVALID, "summary.stats is required with rps/hist");
    if (want_lat && (!out->clock || out->clock_capacity == 0)) return fail(AF_ERR_INVALID, "summary needs outputs.clock");
    if (want_series && (!out->samples || out->tick_capacity == 0)) return fail(AF_ERR_INVALID, "series summary needs outputs.samples");
    if (sum->hist && (sum->hist_bins == 0 || sum->hist_bins > 8192u || !(sum->hist_max > 0.0)))
        return fail(AF_ERR_INVALID, "hist_bins must be 1..8192 and hist_max > 0");
    if (sum->rps && sum->rps_buckets == 0) return fail(AF_ERR_INVALID, "rps buffer with zero buckets");
    const size_t dyn_bytes = ((size_t)(sum->rps ? sum->rps_buckets : 0u) + (sum->hist ? sum->hist_bins : 0u)) * 4u;
    if (dyn_bytes > 96u * 1024u) return fail(AF_ERR_CAPACITY, "rps_buckets + hist_bins exceed the LDS budget (24576 words)");
    if (want_series && e->args.series_pitch / 4u > (uint32_t)afs::kSeriesThreads) return fail(AF_ERR_CAPACITY, "too many sampled series for af_series_kernel");
    return AF_OK;
}

// The analyzer's two kernels over scenarios [sc0, sc0 + count) of `out` / `sum`, enqueued on `stream` (no synchronisation).
// `done_flags` / `retry` ([2][n + 1]: count + scenarios, latency kernel then series kernel): workgroups check their scenario's flag
// and put an unfinished one on their kernel's retry list; `map_lat` / `map_ser` + their counts: the retry launch over such a list.
static int launch_summary_kernels(af_engine_t* e, const af_outputs_t* out, const af_summary_t* sum, uint32_t sc0, uint32_t count, hipStream_t stream,
                                  const uint32_t* done_flags = nullptr, uint32_t* retry = nullptr, const uint32_t* map_lat = nullptr, uint32_t n_map_lat = 0u,
                                  const uint32_t* map_ser = nullptr, uint32_t n_map_ser = 0u) {
    if (count == 0u) return AF_OK;
    const bool by_map = map_lat != nullptr || map_ser != nullptr;
    const bool want_lat = sum->stats || sum->rps || sum->hist;
    const bool want_series = sum->series_mean || sum->series_max;
    const uint32_t rps_buckets = sum->rps ? sum->rps_buckets : 0u;
    const size_t dyn_bytes = ((size_t)rps_buckets + (sum->hist ? sum->hist_bins : 0u)) * 4u;
    const uint32_t n_series = e->args.n_edges + 3u * e->args.n_servers;
    if (want_lat) {
        afs::SumArgs s{};
        s.clock = out->clock + (size_t)sc0 * out->clock_capacity * 2u;
        s.counts = out->counts + (size_t)sc0 * AF_CNT_SLOTS;
        s.clock_cap = out->clock_capacity;
        s.cnt_completed_slot = AF_CNT_COMPLETED;
        s.stats = sum->stats + (size_t)sc0 * 8u;
        s.rps = sum->rps ? sum->rps + (size_t)sc0 * rps_buckets : nullptr;
        s.rps_buckets = rps_buckets;
        s.hist = sum->hist ? sum->hist + (size_t)sc0 * sum->hist_bins : nullptr;
        s.hist_bins = sum->hist ? sum->hist_bins : 0u;
        s.hist_scale = sum->hist ? (double)sum->hist_bins / sum->hist_max : 0.0;
        s.done_flags = done_flags;
        s.retry = retry;
        s.scen_map = map_lat;
        // register budget of the latency kernel (af_summary.hpp: kWpe); AF_SUMMARY_WPE=4|8: measurements
        int wpe = kSummaryWpe;
        if (const char* env = std::getenv("AF_SUMMARY_WPE")) wpe = std::atoi(env);
        const void* fn = wpe == 8 ? reinterpret_cast<const void*>(afs::af_summary_kernel<8>)
                                  : reinterpret_cast<const void*>(afs::af_summary_kernel<4>);
        HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn_bytes));
        void* kargs[] = {&s};
        const uint32_t grid = by_map ? n_map_lat : count;
        if (grid != 0u) HIP_TRY(hipLaunchKernel(fn, dim3(grid), dim3(afs::kThreads), kargs, dyn_bytes, stream));
        HIP_TRY(hipGetLastError());
    }
    if (want_series) {
        afs::SeriesArgs s{};
        s.samples = out->samples + (size_t)sc0 * out->tick_capacity * e->args.series_pitch;
        s.counts = out->counts + (size_t)sc0 * AF_CNT_SLOTS;
        s.tick_cap = out->tick_capacity;
        s.pitch = e->args.series_pitch;
        s.n_series = n_series;
        s.cnt_ticks_slot = AF_CNT_TICKS;
        s.n_edges = e->args.n_edges;
        s.mean = sum->series_mean ? sum->series_mean + (size_t)sc0 * n_series : nullptr;
        s.maxv = sum->series_max ? sum->series_max + (size_t)sc0 * n_series : nullptr;
        s.done_flags = done_flags;
        s.retry = retry ? retry + (size_t)count + 1u : nullptr;
        s.scen_map = map_ser;
        const uint32_t grid = by_map ? n_map_ser : count;
        if (grid != 0u) hipLaunchKernelGGL(afs::af_series_kernel, dim3(grid), dim3(afs::kSeriesThreads), 0, stream, s);
        HIP_TRY(hipGetLastError());
    }
    return AF_OK;
}

// ---- af_engine_run: one sweep as a sequence of steps -------------------------------------------------------------------
// The totals of a run: what becomes e->stats at its end.
struct RunTotals {
    double ms_pregen = 0.0, ms_kernel = 0.0, ms_flow = 0.0;
    float ms_h2d = 0.f;
    uint32_t kl = 0, waves = 0, lds_bytes = 0;   // of the last next-event launch ...
    bool lds_state = false;                      // ... and where its state lived
    uint32_t n_chunks = 0, n_rerun = 0, n_jit = 0, n_jit_miss = 0;
    uint32_t fb_total[5] = {0, 0, 0, 0, 0}, flow_scen = 0;
    uint32_t flow_retried = 0, flow_to_next = 0;
    size_t draw_bytes = 0;
    uint32_t pregen_group = 0;
    uint32_t fused_first = 0u;   // af_engine_run_summarized: scenarios whose analyzer ran beside the stage-parallel kernel's last round
};

// What is fixed once the sweep is validated, staged and sized.  The steps of a run take it and what else they need; all they
// change in it are the totals.
struct Run {
    af_engine_t* e = nullptr;
    const af_sweep_t* sweep = nullptr;
    const af_outputs_t* out = nullptr;
    uint32_t mask = 0;   // the columns the sweep overrides
    uint32_t n = 0, n_draw = 0;
    size_t draw_bytes_per_scen = 0;
    af::Layout L{};
    uint64_t bytes_per_lane = 0;
    size_t tie_words = 0;
    bool hetero_load = false;   // a users / rpm column: scenario lengths differ by orders of magnitude
    // the staged sweep on the device
    const uint64_t* d_seeds = nullptr;
    const double* d_values = nullptr;   // [n_overrides][n]
    const uint32_t* d_params = nullptr;
    const uint32_t* d_idxs = nullptr;
    bool use_flow = false;   // the sweep starts on the stage-parallel kernel, sized by FP
    FlowPlan FP;
    RunTotals t;
};

// The override columns of a sweep: indices within the plan, integral columns integral, ranges the kernels rely on.
static int check_override_columns(const af_engine_t* e, const af_sweep_t* sweep) {
    const KArgs& a = e->args;
    const uint32_t n = sweep->n_scenarios;
    for (uint32_t k = 0; k < sweep->n_overrides; ++k) {
        const af_override_t& o = sweep->overrides[k];
        const uint32_t lim = (o.param >= AF_PARAM_EDGE_MEAN && o.param <= AF_PARAM_EDGE_DROPOUT) ? a.n_edges
                             : (o.param == AF_PARAM_STEP_TIME)                                   ? (uint32_t)e->row_of_step.size()
                             : (o.param == AF_PARAM_SRV_CORES || o.param == AF_PARAM_SRV_RAM_MB)  ? a.n_servers
                             : (o.param >= AF_PARAM_EMARK_TIME && o.param <= AF_PARAM_EMARK_EDGE) ? a.n_edge_marks
                             : (o.param >= AF_PARAM_SMARK_TIME && o.param <= AF_PARAM_SMARK_DOWN) ? a.n_srv_marks
                                                                                                 : 1u;
        if (o.index >= lim) return fail(AF_ERR_INVALID, "override index out of range");
        // integral columns are checked here: the kernels only ever see values inside the plan's ranges
        for (uint32_t i = 0; i < n; ++i) {
            const double v = o.values[i];
            if (o.param == AF_PARAM_SRV_CORES && !(v >= 1.0 && v <= 65535.0 && v == std::floor(v)))
                return fail(AF_ERR_INVALID, "cpu_cores column: integral values within 1..65535");
            if (o.param == AF_PARAM_EMARK_EDGE && !(v >= 0.0 && v < (double)a.n_edges && v == std::floor(v)))
                return fail(AF_ERR_INVALID, "edge-mark column names an unknown edge");
            if (o.param == AF_PARAM_SMARK_LB_EDGE && !(v >= -1.0 && v < (double)a.n_edges && v == std::floor(v)))
                return fail(AF_ERR_INVALID, "server-mark column names an unknown LB edge");
            if (o.param == AF_PARAM_GEN_WINDOW && !(v > 0.0)) return fail(AF_ERR_INVALID, "user_sampling_window column must be positive");
            if (o.param == AF_PARAM_SRV_RAM_MB && !(v > 0.0)) return fail(AF_ERR_INVALID, "ram_mb column must be positive");
        }
    }
    return AF_OK;
}

// The arguments and the override columns of a run; the columns' bits, the state layout they need.
static int validate_sweep(af_engine_t* e, const af_sweep_t* sweep, const af_outputs_t* out, Run& r) {
    if (!e || !sweep || !out) return fail(AF_ERR_INVALID, "NULL argument");
    if (sweep->n_scenarios == 0 || !sweep->seeds) return fail(AF_ERR_INVALID, "empty sweep");
    if (!out->counts) return fail(AF_ERR_INVALID, "outputs.counts is required");
    if (out->clock && out->clock_capacity == 0) return fail(AF_ERR_INVALID, "clock buffer with zero capacity");
    if (out->samples && out->tick_capacity == 0) return fail(AF_ERR_INVALID, "samples buffer with zero capacity");
    if (out->online_hist && (out->online_hist_bins == 0 || !(out->online_hist_max > 0.0)))
        return fail(AF_ERR_INVALID, "online_hist needs online_hist_bins > 0 and online_hist_max > 0");
    if (out->online_rps && out->online_rps_buckets == 0) return fail(AF_ERR_INVALID, "online_rps with zero buckets");
    if (e->plan_only) return fail(AF_ERR_NO_DEVICE, "planning-only engine (AF_DEVICE_PLAN_ONLY): it cannot run");
    HIP_TRY(hipSetDevice(e->device));
    const KArgs& a = e->args;
    const uint32_t n = sweep->n_scenarios;
    r.e = e;
    r.sweep = sweep;
    r.out = out;
    r.n = n;
    if (int rc = sweep_override_mask(sweep, true, r.mask)) return rc;
    if (int rc = check_override_columns(e, sweep)) return rc;
    r.L = af::make_layout(e->request_capacity, e->fifo_capacity, a.n_edges, a.n_servers, a.n_lb_edges, a.n_rows, r.mask, a.n_edge_marks, a.n_srv_marks);
    r.bytes_per_lane = af::layout_bytes_per_lane(r.L);
    r.tie_words = r.L.tie_words;
    r.hetero_load = (r.mask & ((1u << AF_PARAM_GEN_USERS_MEAN) | (1u << AF_PARAM_GEN_RPM_MEAN))) != 0u;
    return AF_OK;
}

// Upload seeds + override tables (one staging buffer).
static int stage_sweep(Run& r) {
    af_engine_t* e = r.e;
    const af_sweep_t* sweep = r.sweep;
    const uint32_t n = r.n;
    const size_t seeds_b = (size_t)n * 8;
    const size_t vals_b = (size_t)sweep->n_overrides * n * 8;
    const size_t tab_b = (size_t)(sweep->n_overrides ? sweep->n_overrides : 1) * 4;
    const size_t total = seeds_b + vals_b + 2 * ((tab_b + 7) & ~size_t(7));
    if (int rc = reserve_device(&e->d_sweep, e->sweep_cap, total)) return rc;
    unsigned char* ds = static_cast<unsigned char*>(e->d_sweep);
    HIP_TRY(hipEventRecord(e->ev0, e->stream));
    HIP_TRY(hipMemcpyAsync(ds, sweep->seeds, seeds_b, hipMemcpyHostToDevice, e->stream));
    std::vector<uint32_t> params(sweep->n_overrides ? sweep->n_overrides : 1, 0u), idxs(params.size(), 0u);
    for (uint32_t k = 0; k < sweep->n_overrides; ++k) {
        params[k] = sweep->overrides[k].param;
        idxs[k] = params[k] == AF_PARAM_STEP_TIME ? e->row_of_step[sweep->overrides[k].index] : sweep->overrides[k].index;
        HIP_TRY(hipMemcpyAsync(ds + seeds_b + (size_t)k * n * 8, sweep->overrides[k].values, (size_t)n * 8,
                               hipMemcpyHostToDevice, e->stream));
    }
    unsigned char* d_params = ds + seeds_b + vals_b;
    unsigned char* d_idxs = d_params + ((tab_b + 7) & ~size_t(7));
    HIP_TRY(hipMemcpyAsync(d_params, params.data(), tab_b, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(d_idxs, idxs.data(), tab_b, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));  // host staging vectors go out of scope below
    HIP_TRY(hipEventRecord(e->ev1, e->stream));
    r.d_seeds = reinterpret_cast<const uint64_t*>(ds);
    r.d_values = reinterpret_cast<const double*>(ds + seeds_b);
    r.d_params = reinterpret_cast<const uint32_t*>(d_params);
    r.d_idxs = reinterpret_cast<const uint32_t*>(d_idxs);
    return AF_OK;
}

// The kernel arguments of the chunk [lo, lo + nc) of the sweep.  Built once per chunk; a launch works on a copy of its own,
// in which it sets where ITS scenarios, draws and state are (scen_map, draw_slot, draws_by_lane, n_scen, draws, pre_flags, tie,
// state, state_bytes_per_wave).
static KArgs chunk_kargs(const Run& r, uint32_t lo, uint32_t nc) {
    const af_outputs_t* out = r.out;
    KArgs a = r.e->args;
    a.L = r.L;
    a.n_ovr = r.sweep->n_overrides;
    a.ovr_param = r.d_params;
    a.ovr_index = r.d_idxs;
    a.ovr_stride = r.n;
    a.clock_cap = out->clock_capacity;
    a.tick_cap = out->tick_capacity;
    a.n_draw = r.n_draw;
    a.n_shared = r.e->d_n_shared;
    a.n_scen = nc;
    a.scen_map = nullptr;
    a.draw_slot = nullptr;
    a.draws_by_lane = 0u;
    a.seeds = r.d_seeds + lo;
    a.ovr_values = r.d_values + lo;
    a.clock = out->clock ? out->clock + (size_t)lo * out->clock_capacity * 2u : nullptr;
    a.samples = out->samples ? out->samples + (size_t)lo * a.series_pitch * out->tick_capacity : nullptr;
    a.counts = out->counts + (size_t)lo * AF_CNT_SLOTS;
    a.online_hist = out->online_hist ? out->online_hist + (size_t)lo * out->online_hist_bins : nullptr;
    a.online_rps = out->online_rps ? out->online_rps + (size_t)lo * out->online_rps_buckets : nullptr;
    a.online_hist_bins = out->online_hist_bins;
    a.online_rps_buckets = out->online_rps_buckets;
    a.online_hist_scale = out->online_hist ? (double)out->online_hist_bins / out->online_hist_max : 0.0;
    return a;
}

// Draws per stream, the kernel family the sweep starts on and its sizing, scenarios per chunk.
static int size_run(Run& r, uint32_t& chunk) {
    af_engine_t* e = r.e;
    if (int rc = draws_per_stream(r.sweep, r.out, r.n_draw)) return rc;
    r.draw_bytes_per_scen = (size_t)(1u + e->args.n_edges) * r.n_draw * sizeof(double);
    // (a sweep the stage-parallel kernel cannot be sized for -- a cpu_cores column above 64, lists that do not fit the LDS --
    // runs on the next-event kernels like a plan outside its range does, unless flow_mode 2 asked for that kernel: ADVICE r3)
    r.use_flow = flow_wanted(e, r.n);
    if (r.use_flow) {
        const int rc = plan_flow(e, chunk_kargs(r, 0u, r.n), r.sweep, r.out, r.FP);
        if (rc == AF_ERR_CAPACITY && e->flow_mode != 2u) r.use_flow = false;
        else if (rc) return rc;
    }
    size_t mem_free = 0, mem_total = 0;
    HIP_TRY(hipMemGetInfo(&mem_free, &mem_total));
    // the stage-parallel kernel only needs the arrival times of a chunk; the next-event kernels every draw
    chunk = chunk_size(e, r.n, r.use_flow ? (size_t)r.n_draw * sizeof(double) : r.draw_bytes_per_scen,
                       mem_free + (r.use_flow ? e->arr_cap : 0));
    if (chunk == 0) return fail(AF_ERR_CAPACITY, "draw_capacity too large for the device memory budget");
    return AF_OK;
}

// One launch of the next-event kernel over `count` scenarios (all of the chunk, or the ones listed in a.scen_map).
static int launch_next_event(Run& r, KArgs a, uint32_t count, bool faithful) {
    af_engine_t* e = r.e;
    RunTotals& t = r.t;
    choose_lanes(e, count, a.blob_bytes, r.bytes_per_lane, t.kl, t.lds_state);
    const uint32_t klog = klog_of(t.kl);
    a.n_scen = count;
    const uint64_t state_per_wave = r.bytes_per_lane * t.kl;
    t.waves = (count + t.kl - 1) / t.kl;
    t.lds_bytes = t.lds_state ? (uint32_t)(a.blob_bytes + state_per_wave) : a.blob_bytes;
    a.state = nullptr;
    a.state_bytes_per_wave = state_per_wave;
    if (!t.lds_state) {
        if (int rc = reserve_device((void**)&e->d_state, e->state_cap, (size_t)state_per_wave * t.waves)) return rc;
        a.state = e->d_state;
    }
    // SimPy-order variant: when the waves do not all fit at 3 per SIMD anyway, the build with
    // the larger register budget (2 per SIMD, no spills) is the faster one (measured: 6 400
    // grid points 6.2 s -> 5.5 s; 2 500 waves that do fit: 2.7 s vs 4.3 s).  Sweeps over the load
    // (scenario lengths differ by orders of magnitude) do not run as lock-step batches: there the
    // per-wave speed decides and the roomy build wins even when everything would fit.
    const bool roomy = faithful && (t.waves > 3072u || r.hetero_load);
    const void* fn = des_kernel_for(t.lds_state, faithful, klog, roomy);
    hipFunction_t jit_fn = nullptr;
    if (e->jit_module && t.lds_bytes <= 64u * 1024u) {
        if (jit_spec_string(a, t.lds_state, klog) == e->jit_spec) jit_fn = !faithful ? e->jit_lean : roomy ? e->jit_order2 : e->jit_order3;
        else t.n_jit_miss += 1u;
    }
    if (std::getenv("AF_DEBUG"))
        std::fprintf(stderr, "[af] launch: %u scenarios, %u waves x %u lanes, %s state, %s%s%s\n", count, t.waves, t.kl,
                     t.lds_state ? "LDS" : "HBM", faithful ? "SimPy-order" : "lean", roomy ? " (2 waves/SIMD build)" : "",
                     jit_fn ? ", plan-specialised" : "");
    void* kargs[] = {&a};
    if (jit_fn) {
        HIP_TRY(hipModuleLaunchKernel(jit_fn, t.waves, 1, 1, kWave, 1, 1, t.lds_bytes, e->stream, kargs, nullptr));
        t.n_jit += 1u;
    } else {
        if (t.lds_state) HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)t.lds_bytes));
        HIP_TRY(hipLaunchKernel(fn, dim3(t.waves), dim3(kWave), kargs, t.lds_bytes, e->stream));
    }
    return AF_OK;
}

// Second pass over a piece: the scenarios of `first` (the piece's first launch over `cnt` scenarios, those of `list` or, without a
// list, [0, cnt)) that stopped at a shared instant run again, from their start, on the SimPy-order kernel, with the draws of
// their slot in the piece.
static int rerun_shared_instants(Run& r, const KArgs& first, uint32_t nc_all, const uint32_t* list, uint32_t cnt) {
    af_engine_t* e = r.e;
    std::vector<uint32_t> cnt_host((size_t)nc_all * AF_CNT_SLOTS);
    HIP_TRY(hipMemcpy(cnt_host.data(), first.counts, cnt_host.size() * 4u, hipMemcpyDeviceToHost));
    std::vector<uint32_t> map2, slot2;
    for (uint32_t j = 0; j < cnt; ++j) {
        const uint32_t scn = list ? list[j] : j;
        if (cnt_host[(size_t)scn * AF_CNT_SLOTS + AF_CNT_FLAGS] & af::FLAG_SHARED_INSTANT) {
            map2.push_back(scn);
            slot2.push_back(j);
        }
    }
    if (map2.empty()) return AF_OK;
    if (int rc = reserve_device((void**)&e->d_map, e->map_cap, (size_t)nc_all * 4u)) return rc;
    if (int rc = reserve_device((void**)&e->d_slot, e->slot_cap, map2.size() * 4u)) return rc;
    HIP_TRY(hipMemcpy(e->d_map, map2.data(), map2.size() * 4u, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->d_slot, slot2.data(), slot2.size() * 4u, hipMemcpyHostToDevice));
    KArgs a = first;
    a.scen_map = e->d_map;
    a.draw_slot = e->d_slot;
    if (a.online_hist || a.online_rps) {   // scenarios that start over: their online counters are cleared
        hipLaunchKernelGGL(af_zero_online, dim3((uint32_t)map2.size()), dim3(256), 0, e->stream, a, (uint32_t)map2.size());
        HIP_TRY(hipGetLastError());
    }
    if (int rc = launch_next_event(r, a, (uint32_t)map2.size(), true)) return rc;
    r.t.n_rerun += (uint32_t)map2.size();
    // such plans keep producing them: later runs start with the SimPy-order kernel, which
    // is cheaper than a second pass over a few long scenarios in narrow, latency-bound waves
    e->shared_instants_likely = true;
    return AF_OK;
}

// The next-event kernels over `count` scenarios of a chunk: all of them (h_map == nullptr) or the
// listed ones.  Draws are pre-generated per slot j = position in the list; pieces that fit the draw budget.
static int run_next_event(Run& r, const KArgs& chunk, uint32_t count, const uint32_t* h_map) {
    af_engine_t* e = r.e;
    RunTotals& t = r.t;
    size_t mf = 0, mt = 0;
    HIP_TRY(hipMemGetInfo(&mf, &mt));
    // (per scenario: its draws, its scratch of the SimPy-order path and -- when the state does not fit the LDS: long wait
    // queues -- its state words in HBM)
    const size_t state_hbm = r.bytes_per_lane > 48u * 1024u ? (size_t)r.bytes_per_lane : 0u;
    uint32_t piece = chunk_size(e, count, r.draw_bytes_per_scen + r.tie_words * 8u + state_hbm, mf);
    if (piece == 0) return fail(AF_ERR_CAPACITY, "draw_capacity / fifo_capacity too large for the device memory budget");
    if (const char* env = std::getenv("AF_SEQ_PIECE")) {   // test hook: force a whole chunk to run in pieces
        const uint32_t v = (uint32_t)std::atoi(env);
        if (v != 0u && v < piece) piece = v;
    }
    // A whole chunk (no list) that does not fit the draw budget in one piece -- the free memory is measured again
    // here, after the scratch buffers of the chunk were allocated -- runs as pieces over an identity list: piece
    // p0 simulates scenarios [p0, p0 + cnt) with its draws in slots [0, cnt).  (Round 2 ran [0, cnt) again: ADVICE r2.)
    std::vector<uint32_t> ident;
    if (h_map == nullptr && piece < count) {
        ident.resize(count);
        for (uint32_t i = 0; i < count; ++i) ident[i] = i;
        h_map = ident.data();
    }
    const bool listed_subset = h_map != nullptr && ident.empty();
    // First pass: the lean kernel.  A scenario in which two timed events share an instant stops
    // there and is simulated again, from its start, by the kernel that has SimPy's event-by-event
    // path; engines whose plan keeps producing such scenarios go straight to that kernel.
    // (a handful of scenarios handed back by the stage-parallel kernel -- usually for a tie -- go straight to the
    // SimPy-order kernel: a second pass over them would cost a whole latency-bound launch more)
    // (decided once for all pieces: what the first piece learns -- rerun_shared_instants -- must not make the others run
    // differently, or the launches of a chunk and its shared_instant_scenarios would depend on the draw budget)
    const bool faithful_first = e->shared_instants_likely || (listed_subset && (uint64_t)count * 50u < chunk.n_scen);
    for (uint32_t p0 = 0; p0 < count; p0 += piece) {
        const uint32_t cnt = count - p0 < piece ? count - p0 : piece;
        if (int rc = reserve_device((void**)&e->d_draws, e->draws_cap, r.draw_bytes_per_scen * cnt)) return rc;
        if (int rc = reserve_device((void**)&e->d_pre_flags, e->pre_flags_cap, (size_t)cnt * 4u)) return rc;
        if (int rc = reserve_device((void**)&e->d_tie, e->tie_cap, (size_t)cnt * r.tie_words * 8u)) return rc;
        if (r.draw_bytes_per_scen * cnt > t.draw_bytes) t.draw_bytes = r.draw_bytes_per_scen * cnt;
        KArgs a = chunk;
        a.draws = e->d_draws;
        a.pre_flags = e->d_pre_flags;
        a.tie = e->d_tie;
        if (h_map) {
            if (int rc = reserve_device((void**)&e->d_map, e->map_cap, (size_t)cnt * 4u)) return rc;
            HIP_TRY(hipMemcpyAsync(e->d_map, h_map + p0, (size_t)cnt * 4u, hipMemcpyHostToDevice, e->stream));
            a.scen_map = e->d_map;
            a.draws_by_lane = 1u;
        }
        a.n_scen = cnt;
        HIP_TRY(hipEventRecord(e->ev2, e->stream));
        if (launch_pregen_arrivals(a, cnt, (uint32_t)((1u + a.n_edges) * r.n_draw), !r.hetero_load, e->stream))
            return fail(AF_ERR_HIP, "af_pregen_arrivals: LDS attribute");
        hipLaunchKernelGGL(af_pregen_edges, dim3((r.n_draw + 255u) / 256u, cnt, a.n_edges), dim3(256), 0, e->stream, a);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(e->ev3, e->stream));
        if (listed_subset && (a.online_hist || a.online_rps)) {   // scenarios that start over: their online counters are cleared
            hipLaunchKernelGGL(af_zero_online, dim3(cnt), dim3(256), 0, e->stream, a, cnt);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemsetAsync(e->d_n_shared, 0, 4, e->stream));
        if (int rc = launch_next_event(r, a, cnt, faithful_first)) return rc;
        if (!faithful_first) {
            uint32_t n_shared = 0;
            HIP_TRY(hipMemcpyAsync(&n_shared, e->d_n_shared, 4, hipMemcpyDeviceToHost, e->stream));
            HIP_TRY(hipStreamSynchronize(e->stream));
            if (n_shared > 0u)
                if (int rc = rerun_shared_instants(r, a, chunk.n_scen, h_map ? h_map + p0 : nullptr, cnt)) return rc;
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(e->ev4, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        float ms_p = 0.f, ms_k = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms_p, e->ev2, e->ev3));
        HIP_TRY(hipEventElapsedTime(&ms_k, e->ev3, e->ev4));
        t.ms_pregen += ms_p;
        t.ms_kernel += ms_k;
    }
    return AF_OK;
}

// ---- one chunk on the stage-parallel kernel; what it hands back goes to the next-event kernels ----------------------------
// The first launch of a chunk, as its steps hand it on.
struct FlowLaunch {
    aff::FlowArgs f{};
    uint32_t lds = 0;            // bytes of LDS per wave asked for
    bool jit = false;            // the plan-specialised build of exactly this launch, else `fn`
    const void* fn = nullptr;    // the library's generic instantiation
    const char* prof_path = nullptr;   // AF_FLOW_PROF's file (f.prof: its counters), else null
    uint32_t gate = 0u;          // af_engine_run_summarized: the analyzer starts once this many scenarios are done (0: after the run)
};

// Rows or groups (af_pregen.hpp) for the arrival times of the chunk [lo, lo + nc)?  Grouped pre-generation: sweeps of alike
// scenarios -- a workgroup is as slow as its heaviest one -- with sampling windows long enough that a window start (a user draw
// by one wave, the pipeline refilled) does not count.
static bool pregen_grouped(const Run& r, const KArgs& a, uint32_t lo, uint32_t nc) {
    const char* pregen_mode = std::getenv("AF_PREGEN_MODE");   // rows | groups: tests and measurements
    const bool force_groups = pregen_mode && std::strcmp(pregen_mode, "groups") == 0;
    const bool force_rows = pregen_mode && std::strcmp(pregen_mode, "rows") == 0;
    // (sweeps over users / rpm -- BASELINE configs 3 / 4 -- as long as the heaviest scenario is within 2.5 x of the mean:
    // load_spread_suits_groups)
    return !force_rows && a.gen_window_s > 0.0 &&
           (force_groups || (!(r.mask & (1u << AF_PARAM_GEN_WINDOW)) && nc >= 3072u &&
                             (double)r.n_draw * a.gen_window_s >= 512.0 * a.total_time &&
                             (!r.hetero_load || load_spread_suits_groups(r.e, r.sweep, lo, nc))));
}

// Arrival times of the chunk's scenarios; for sweeps over the load, their launch order (`ordered`: e->d_order holds it).
static int pregen_flow_chunk(Run& r, const KArgs& chunk, uint32_t lo, bool& ordered) {
    af_engine_t* e = r.e;
    const uint32_t nc = chunk.n_scen, n_draw = r.n_draw;
    if (int rc = reserve_device((void**)&e->d_arr, e->arr_cap, (size_t)nc * n_draw * sizeof(double))) return rc;
    if (int rc = reserve_device((void**)&e->d_arr_flags, e->arr_flags_cap, (size_t)nc * 4u)) return rc;
    if ((size_t)nc * n_draw * sizeof(double) > r.t.draw_bytes) r.t.draw_bytes = (size_t)nc * n_draw * sizeof(double);
    KArgs a = chunk;
    a.draws = e->d_arr;
    a.pre_flags = e->d_arr_flags;
    const bool grouped = pregen_grouped(r, a, lo, nc);
    // Sweeps over the load: waves are dispatched in blockIdx order as slots free up, and a wave lasts as long as its scenario
    // has events.  A users-major grid (BASELINE configs 3 / 4: users ascending with the index) is then the WORST order --
    // the heaviest scenarios start last and the launch ends with a few long waves on an empty chip (list scheduling of
    // 10 000 waves with times ~ users on 4 096 slots: 3.54 mean wave times ascending, 2.73 heaviest first, 2.44 ideal).  Wave j
    // simulates scenario order[j]; everything the kernel reads or writes is indexed by the scenario.
    ordered = r.hetero_load && std::getenv("AF_FLOW_ORDER_OFF") == nullptr;
    if (ordered) {
        std::vector<uint32_t> order = heaviest_first(e, r.sweep, lo, nc);
        if (int rc = reserve_device((void**)&e->d_order, e->order_cap, (size_t)nc * 4u)) return rc;
        HIP_TRY(hipMemcpyAsync(e->d_order, order.data(), (size_t)nc * 4u, hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));   // (`order` leaves scope; 40 KB, before anything of this chunk is enqueued)
    }
    HIP_TRY(hipEventRecord(e->ev2, e->stream));
    if (launch_pregen_arrivals(a, nc, n_draw, !r.hetero_load, e->stream, grouped, &r.t.pregen_group)) return fail(AF_ERR_HIP, "af_arrival_groups: LDS attribute");
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(e->ev3, e->stream));
    return AF_OK;
}

// The stage-parallel kernel's arguments for the first launch over a chunk.
static aff::FlowArgs flow_chunk_args(const Run& r, const KArgs& a, bool ordered) {
    const af_engine_t* e = r.e;
    aff::FlowArgs f = e->fargs;
    f.L = r.FP.FL;
    f.n_scen = a.n_scen;
    f.seeds = a.seeds;
    f.n_ovr = a.n_ovr;
    f.ovr_param = a.ovr_param;
    f.ovr_index = a.ovr_index;
    f.ovr_values = a.ovr_values;
    f.ovr_stride = a.ovr_stride;
    f.arrivals = e->d_arr;
    f.n_draw = r.n_draw;
    f.pre_flags = e->d_arr_flags;
    if (ordered) f.scen_map = e->d_order;
    f.clock = a.clock;
    f.clock_cap = a.clock_cap;
    f.samples = a.samples;
    f.tick_cap = a.tick_cap;
    f.counts = a.counts;
    f.online_hist = a.online_hist;
    f.online_rps = a.online_rps;
    f.online_hist_bins = a.online_hist_bins;
    f.online_rps_buckets = a.online_rps_buckets;
    f.online_hist_scale = a.online_hist_scale;
    f.n_fallback = e->d_fb;
    return f;
}

// Which build runs the launch: the plan-specialised one of exactly this launch (af_engine_set_kernels), else the library's
// generic instantiation.
static int pick_flow_kernel(Run& r, uint32_t nc, FlowLaunch& fl) {
    af_engine_t* e = r.e;
    const FlowPlan& FP = r.FP;
    fl.lds = spread_lds_bytes(FP.lds);
    fl.jit = e->flow_jit_fn != nullptr && fl.lds <= 64u * 1024u &&
             flow_jit_spec_string(e, FP, r.out, r.sweep->n_overrides != 0u) == e->flow_jit_spec;
    if (e->flow_jit_fn != nullptr && !fl.jit) r.t.n_jit_miss += 1u;
    if (std::getenv("AF_DEBUG")) std::fprintf(stderr, "[af] flow jit spec: %s\n", flow_jit_spec_string(e, FP, r.out, r.sweep->n_overrides != 0u).c_str());
    if (std::getenv("AF_DEBUG"))
        std::fprintf(stderr, "[af] flow launch: %u scenarios, %u list entries%s, %u ring rows, %u B LDS per wave, af_flow_kernel<%u, %#x>%s%s\n", nc,
                     FP.FL.cap, FP.big ? " (long-list instantiation)" : "", FP.FL.ring_rows, FP.lds, FP.ipl, FP.feat,
                     FP.lean ? (FP.far ? ", lean instantiation with far edges" : ", lean instantiation") : "", fl.jit ? ", plan-specialised" : "");
    fl.fn = fl.jit ? nullptr : flow_kernel_for(FP.ipl, FP.feat);
    if (!fl.jit && fl.fn == nullptr) return fail(AF_ERR_INVALID, "no stage-parallel instantiation for this launch");
    if (!fl.jit && fl.lds > 48u * 1024u) HIP_TRY(hipFuncSetAttribute(fl.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fl.lds));
    return AF_OK;
}

// The analyzer beside the last round: after how many finished scenarios of `nc` it starts, given the waves that are resident at
// once (0: not beside the kernel).
static uint32_t analyzer_gate(uint32_t nc, uint32_t resident) {
    const uint32_t rem = resident ? nc % resident : 0u;
    // (a tail of more than three quarters of a round leaves no room for the analyzer's workgroups; no tail, nothing to fill)
    // (and only where the partial round is a good part of the launch -- at most six rounds --: the analyzer of a sweep of
    // many rounds needs longer than the tail lasts, and beside a FULL round it only takes the kernel's slots: BASELINE
    // config 5, 12.2 rounds, 227 instead of 223 ms per step, measured)
    if (resident != 0u && nc > resident && nc <= 6u * resident && rem != 0u && rem * 4u <= resident * 3u) return nc - rem;
    return 0u;
}

// af_engine_run_summarized: the analyzer starts on a second stream once the scenarios of the kernel's full residency rounds
// have finished (hipStreamWaitValue32 on a counter its waves bump) and runs beside the last, partial round, which leaves
// most of the chip idle; the analyzer is HBM-bound where this kernel is VALU-bound.  A workgroup of the analyzer that
// meets a scenario still being simulated (its done flag is clear) puts it on a retry list and leaves.
// (Measured first, round 6: the kernel launched in two parts with the analyzer of the first beside the second --
// 51.9 instead of 48.4 ms per step on BASELINE config 2: the second part cannot start before the LAST wave of the first
// has ended and then lasts a whole scenario at low occupancy, 11 ms against the 7 ms of the natural tail.)
static int gate_for_launch(const Run& r, uint32_t nc, const FlowLaunch& fl, uint32_t& gate) {
    af_engine_t* e = r.e;
    gate = 0u;
    if (e->wait_value_ok < 0) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeCanUseStreamWaitValue, e->device) != hipSuccess) { (void)hipGetLastError(); v = 0; }
        e->wait_value_ok = v;
    }
    // the resident waves of (function, LDS size) are asked once per engine: the device properties and the occupancy query cost
    // host time inside every af_engine_run_summarized otherwise; a newly loaded specialised kernel clears the list
    const void* fn = fl.jit ? (const void*)e->flow_jit_fn : fl.fn;
    uint32_t resident = 0u;
    bool known = false;
    for (const af_engine_t::ResidentWaves& rw : e->resident_waves)
        if (rw.fn == fn && rw.lds == fl.lds) {
            resident = rw.waves;
            known = true;
        }
    if (!known) {
        int per_cu = 0, n_cu = 0;
        HIP_TRY(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, e->device));
        if (fl.jit) HIP_TRY(hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, e->flow_jit_fn, (int)kWave, fl.lds));
        else HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fl.fn, (int)kWave, fl.lds));
        resident = (uint32_t)(per_cu > 0 ? per_cu : 0) * (uint32_t)(n_cu > 0 ? n_cu : 0);
        e->resident_waves.push_back({fn, fl.lds, resident});
    }
    if (e->wait_value_ok > 0) gate = analyzer_gate(nc, resident);
    if (std::getenv("AF_DEBUG")) std::fprintf(stderr, "[af] analyzer beside the last round: %u resident waves, gate at %u of %u scenarios\n", resident, gate, nc);
    return AF_OK;
}

// The second stream, the done flags and the retry lists of the analyzer beside the kernel, cleared; the kernel told where they are.
static int arm_side_stream(af_engine_t* e, uint32_t nc) {
    if (e->stream2 == nullptr) {
        HIP_TRY(hipStreamCreateWithFlags(&e->stream2, hipStreamNonBlocking));
        HIP_TRY(hipEventCreate(&e->ev_s0));
        HIP_TRY(hipEventCreate(&e->ev_s1));
        HIP_TRY(hipHostMalloc((void**)&e->h_done_count, 64, hipHostMallocCoherent | hipHostMallocMapped));
        HIP_TRY(hipHostGetDevicePointer((void**)&e->d_done_count, e->h_done_count, 0));
    }
    if (int rc = reserve_device((void**)&e->d_done_flags, e->done_flags_cap, (size_t)nc * 4u)) return rc;
    if (int rc = reserve_device((void**)&e->d_retry, e->retry_cap, 2u * ((size_t)nc + 1u) * 4u)) return rc;
    *e->h_done_count = 0u;   // (nothing of this engine is in flight: af_engine_run is synchronous)
    HIP_TRY(hipMemsetAsync(e->d_done_flags, 0, (size_t)nc * 4u, e->stream));
    HIP_TRY(hipMemsetAsync(e->d_retry, 0, 2u * ((size_t)nc + 1u) * 4u, e->stream));
    // (where the kernel's entry point finds them: behind the hand-over counters it already has a pointer to -- two more
    // kernel arguments cost the general-server form 5 %, measured: its register allocation answers small changes chaotically)
    e->done_ptrs[0] = reinterpret_cast<uint64_t>(e->d_done_flags);
    e->done_ptrs[1] = reinterpret_cast<uint64_t>(e->d_done_count);
    HIP_TRY(hipMemcpyAsync(e->d_fb + kDoneWords, e->done_ptrs, 16u, hipMemcpyHostToDevice, e->stream));
    return AF_OK;
}

static int launch_flow(Run& r, uint32_t nc, FlowLaunch& fl) {
    af_engine_t* e = r.e;
    fl.f.n_scen = nc;
    void* kargs[] = {&fl.f};
    if (fl.jit) {
        HIP_TRY(hipModuleLaunchKernel(e->flow_jit_fn, nc, 1, 1, kWave, 1, 1, fl.lds, e->stream, kargs, nullptr));
        r.t.n_jit += 1u;
    } else {
        HIP_TRY(hipLaunchKernel(fl.fn, dim3(nc), dim3(kWave), kargs, fl.lds, e->stream));
    }
    return AF_OK;
}

// The analyzer on the second stream, behind a wait for the kernel's done counter.
// (from here on the second stream waits for the counter: whatever goes wrong below must still let it through)
static int enqueue_side_stream(af_engine_t* e, uint32_t nc, uint32_t gate) {
    auto release_side = [&]() { *e->h_done_count = 0xFFFFFFFFu; };
    hipError_t err = hipStreamWaitValue32(e->stream2, e->d_done_count, gate, hipStreamWaitValueGte, 0xFFFFFFFFu);
    if (err == hipSuccess) err = hipEventRecord(e->ev_s0, e->stream2);
    int rc = AF_OK;
    if (err == hipSuccess) rc = launch_summary_kernels(e, e->fused_out, e->fused_sum, 0u, nc, e->stream2, e->d_done_flags, e->d_retry, nullptr, 0u);
    if (err == hipSuccess && rc == AF_OK) err = hipEventRecord(e->ev_s1, e->stream2);
    if (err != hipSuccess || rc != AF_OK) {
        release_side();
        (void)hipStreamSynchronize(e->stream);
        (void)hipStreamSynchronize(e->stream2);
        if (rc != AF_OK) return rc;
        HIP_TRY(err);
    }
    return AF_OK;
}

// AF_FLOW_PROF: the launch's section times, appended to the file.
static int dump_flow_profile(const FlowPlan& FP, uint32_t nc, const FlowLaunch& fl) {
    std::vector<unsigned long long> hp((size_t)nc * aff::kProfSections);
    HIP_TRY(hipMemcpy(hp.data(), fl.f.prof, hp.size() * 8u, hipMemcpyDeviceToHost));
    static const char* names[aff::kProfSections] = {"setup+end", "generator batch", "select", "series: delivery end (FAR)", "station logic",
                                                    "servers_solve + claim", "server series", "draws (Philox, log)", "send: spike + series",
                                                    "append + send_floor", "complete", "flush_ticks + round end",
                                                    "general servers: lanes", "general servers: walk", "general servers: rank + relax", "general servers: state at the horizon",
                                                    "COUNT rounds solved at once", "COUNT relaxation sweeps", "COUNT lanes in solved rounds", "COUNT rounds walked by event",
                                                    "general servers: standing (ranks, RAM)", "general servers: commit walk (series)",
                                                    "COUNT selects ranked by the lane window", "COUNT selects that fell back to the bucket rank"};
    double acc[aff::kProfSections] = {}, total = 0.0;
    for (uint32_t i = 0; i < nc; ++i)
        for (uint32_t k = 0; k < aff::kProfSections; ++k) acc[k] += (double)hp[(size_t)i * aff::kProfSections + k];
    for (uint32_t k = 0; k < aff::kProfSections; ++k)
        if (!names[k] || std::strncmp(names[k], "COUNT", 5) != 0) total += acc[k];
    if (FILE* fp = std::fopen(fl.prof_path, "a")) {
        std::fprintf(fp, "af_flow_kernel<%u, %#x> sections, %u waves, mean cycles per wave %.0f:\n", FP.ipl, FP.feat, nc, total / nc);
        for (uint32_t k = 0; k < aff::kProfSections; ++k)
            if (names[k]) std::fprintf(fp, "  %-28s %6.2f %%  %12.0f cycles per wave\n", names[k], 100.0 * acc[k] / total, acc[k] / nc);
        std::fclose(fp);
    }
    return AF_OK;
}

// Second chance on the stage-parallel kernel itself, in its most tolerant form: 256-entry lists, tick
// differences in HBM (no reach limit), messages carry their send time so that two deliveries of one station
// at the same instant are ordered the way SimPy orders them.  A wave costs tens of milliseconds; the same
// scenario on a next-event kernel is a latency-bound chain of ~1 s (LB-2).  Only what this launch hands
// back again -- or what can never fit its RAM model -- goes to the next-event kernels: those join `rest`.
static int flow_second_chance(Run& r, const KArgs& chunk, const aff::FlowArgs& f, uint32_t lo, const std::vector<uint32_t>& retry,
                              std::vector<uint32_t>& rest, std::vector<uint32_t>& cnt_host) {
    af_engine_t* e = r.e;
    const aff::FlowLayout& FL2 = r.FP.FL2;
    if (int rc = reserve_device((void**)&e->d_map, e->map_cap, retry.size() * 4u)) return rc;
    HIP_TRY(hipMemcpyAsync(e->d_map, retry.data(), retry.size() * 4u, hipMemcpyHostToDevice, e->stream));
    aff::FlowArgs f2 = f;
    f2.L = FL2;
    f2.n_scen = (uint32_t)retry.size();
    f2.scen_map = e->d_map;
    f2.n_fallback = e->d_fb + 5;
    const uint32_t lds2 = chunk.blob_bytes + f2.L.n_words * 8u;
    if (lds2 > kLdsLimit) return fail(AF_ERR_CAPACITY, "flow kernel layout exceeds the LDS of a compute unit");
    if (chunk.online_hist || chunk.online_rps) {   // scenarios that start over: their online counters are cleared
        KArgs a = chunk;
        a.scen_map = e->d_map;
        hipLaunchKernelGGL(af_zero_online, dim3((uint32_t)retry.size()), dim3(256), 0, e->stream, a, (uint32_t)retry.size());
        HIP_TRY(hipGetLastError());
    }
    constexpr uint32_t kRobust = aff::FEAT_ALL | aff::FEAT_TIEBREAK | aff::FEAT_BIGLIST;
    const void* fn2 = flow_kernel_for(1u, kRobust | (r.FP.gen_compact ? (uint32_t)aff::FEAT_GENSRV : 0u) | (e->flow_chain ? (uint32_t)aff::FEAT_CHAIN : 0u) |
                                              (f2.lb_least_connections ? (uint32_t)aff::FEAT_LC : 0u));
    if (fn2 == nullptr) return fail(AF_ERR_INVALID, "no stage-parallel instantiation for this launch");
    if (lds2 > 48u * 1024u) HIP_TRY(hipFuncSetAttribute(fn2, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2));
    HIP_TRY(hipEventRecord(e->ev3, e->stream));
    void* kargs2[] = {&f2};
    if (std::getenv("AF_DEBUG")) {
        std::fprintf(stderr, "[af] flow second chance: %zu scenarios (lists of %u/%u/%u/%u entries with send times, differences in HBM), %u B LDS:",
                     retry.size(), FL2.cap_of[0], FL2.cap_of[1], FL2.cap_of[2], FL2.cap_of[3], lds2);
        for (size_t q = 0; q < retry.size() && q < 16; ++q)
            std::fprintf(stderr, " %u(flags %#x)", lo + retry[q], cnt_host[(size_t)retry[q] * AF_CNT_SLOTS + AF_CNT_FLAGS]);
        std::fprintf(stderr, "\n");
    }
    HIP_TRY(hipLaunchKernel(fn2, dim3((uint32_t)retry.size()), dim3(kWave), kargs2, lds2, e->stream));
    HIP_TRY(hipEventRecord(e->ev4, e->stream));
    uint32_t fb2[5] = {0, 0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(fb2, e->d_fb + 5, sizeof fb2, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    float ms2 = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms2, e->ev3, e->ev4));
    r.t.ms_flow += ms2;
    r.t.flow_retried += (uint32_t)retry.size();
    if (fb2[0] > 0u) {
        HIP_TRY(hipMemcpy(cnt_host.data(), chunk.counts, cnt_host.size() * 4u, hipMemcpyDeviceToHost));
        for (uint32_t i : retry)
            if (cnt_host[(size_t)i * AF_CNT_SLOTS + AF_CNT_FLAGS] & aff::FLAG_FLOW_FALLBACK) rest.push_back(i);
        std::sort(rest.begin(), rest.end());
    }
    return AF_OK;
}

// What the first launch over a chunk handed back: a second chance for what can have one, the next-event kernels for the rest.
static int rerun_handed_back(Run& r, const KArgs& chunk, const aff::FlowArgs& f, uint32_t lo, bool& on_flow) {
    af_engine_t* e = r.e;
    const uint32_t nc = chunk.n_scen;
    std::vector<uint32_t> cnt_host((size_t)nc * AF_CNT_SLOTS);
    HIP_TRY(hipMemcpy(cnt_host.data(), chunk.counts, cnt_host.size() * 4u, hipMemcpyDeviceToHost));
    std::vector<uint32_t> retry, rest;
    for (uint32_t i = 0; i < nc; ++i) {
        const uint32_t fl = cnt_host[(size_t)i * AF_CNT_SLOTS + AF_CNT_FLAGS];
        if (!(fl & aff::FLAG_FLOW_FALLBACK)) continue;
        // (flow_big: that WAS the most tolerant form; a tie the general server station gives up on stops the second chance at
        // the same instant: straight to the next-event kernels)
        if ((fl & (aff::FLOW_WHY_RAM | aff::FLOW_WHY_GEN_TIE)) || (r.FP.big && !r.FP.gen_compact)) rest.push_back(i);
        else retry.push_back(i);
    }
    if (!retry.empty())
        if (int rc = flow_second_chance(r, chunk, f, lo, retry, rest, cnt_host)) return rc;
    r.t.flow_to_next += (uint32_t)rest.size();
    if (!rest.empty())
        if (int rc = run_next_event(r, chunk, (uint32_t)rest.size(), rest.data())) return rc;
    // A plan whose scenarios mostly end on the next-event kernels anyway (general servers fed by edges with discrete
    // latencies: arrivals that coincide with step ends) pays a flow pass, a second chance AND a next-event pass
    // per scenario: once a chunk handed more than a quarter of its scenarios over, the chunks still to come go to the
    // next-event kernels directly (results are the same either way; flow_mode 2 = "always" keeps the stage-parallel kernel).
    if ((uint64_t)rest.size() * 4u > (uint64_t)nc && e->flow_mode != 2u) on_flow = false;
    return AF_OK;
}

// The stage-parallel kernel over the whole chunk [lo, lo + chunk.n_scen).  `on_flow` turns false when the chunks still to come
// are better off on the next-event kernels.
static int run_flow_chunk(Run& r, const KArgs& chunk, uint32_t lo, bool& on_flow) {
    af_engine_t* e = r.e;
    RunTotals& t = r.t;
    const uint32_t nc = chunk.n_scen;
    bool ordered = false;
    if (int rc = pregen_flow_chunk(r, chunk, lo, ordered)) return rc;
    FlowLaunch fl;
    fl.f = flow_chunk_args(r, chunk, ordered);
    HIP_TRY(hipMemsetAsync(e->d_fb, 0, 32u * 4u, e->stream));
    // measurement hook (AF_FLOW_PROF=<file>, plan-specialised builds only): shader-clock time per section of Flow::run
    fl.prof_path = std::getenv("AF_FLOW_PROF");
    if (fl.prof_path != nullptr) {
        if (int rc = reserve_device((void**)&e->d_prof, e->prof_cap, (size_t)nc * aff::kProfSections * 8u)) return rc;
        HIP_TRY(hipMemsetAsync(e->d_prof, 0, (size_t)nc * aff::kProfSections * 8u, e->stream));
        fl.f.prof = e->d_prof;
    }
    if (int rc = pick_flow_kernel(r, nc, fl)) return rc;
    if (e->fused_sum != nullptr && lo == 0u && nc == r.n && fl.f.prof == nullptr)
        if (int rc = gate_for_launch(r, nc, fl, fl.gate)) return rc;
    if (fl.gate != 0u)
        if (int rc = arm_side_stream(e, nc)) return rc;
    if (int rc = launch_flow(r, nc, fl)) return rc;
    if (fl.gate != 0u)
        if (int rc = enqueue_side_stream(e, nc, fl.gate)) return rc;
    t.fused_first = fl.gate;
    HIP_TRY(hipEventRecord(e->ev4, e->stream));
    uint32_t fb[5] = {0, 0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(fb, e->d_fb, sizeof fb, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (t.fused_first != 0u) {
        HIP_TRY(hipStreamSynchronize(e->stream2));
        float ms_s = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms_s, e->ev_s0, e->ev_s1));
        e->stats.summary_beside_ms = ms_s;
        // (a scenario handed back is simulated again below and its outputs change: the sweep is then summarised again, in full)
        e->fused_done = fb[0] == 0u;
    }
    if (fl.f.prof != nullptr)
        if (int rc = dump_flow_profile(r.FP, nc, fl)) return rc;
    float ms_p = 0.f, ms_f = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms_p, e->ev2, e->ev3));
    HIP_TRY(hipEventElapsedTime(&ms_f, e->ev3, e->ev4));
    t.ms_pregen += ms_p;
    t.ms_flow += ms_f;
    t.flow_scen += nc;
    for (int k = 0; k < 5; ++k) t.fb_total[k] += fb[k];
    if (fb[0] > 0u)
        if (int rc = rerun_handed_back(r, chunk, fl.f, lo, on_flow)) return rc;
    return AF_OK;
}

// The totals of the run become e->stats.
static int write_stats(Run& r) {
    af_engine_t* e = r.e;
    RunTotals& t = r.t;
    HIP_TRY(hipEventElapsedTime(&t.ms_h2d, e->ev0, e->ev1));
    e->stats.kernel_ms = t.ms_kernel + t.ms_flow;
    e->stats.flow_kernel_ms = t.ms_flow;
    e->stats.flow_scenarios = t.flow_scen;
    e->stats.flow_fallback = t.fb_total[0];
    e->stats.flow_fallback_tie = t.fb_total[1];
    e->stats.flow_fallback_list = t.fb_total[2];
    e->stats.flow_fallback_ring = t.fb_total[3];
    e->stats.flow_fallback_ram = t.fb_total[4];
    e->stats.flow_retried = t.flow_retried;
    e->stats.flow_to_next_event = t.flow_to_next;
    e->stats.flow_list_entries = t.flow_scen ? r.FP.FL.cap : 0u;
    e->stats.flow_ring_rows = t.flow_scen ? r.FP.FL.ring_rows : 0u;
    e->stats.flow_lds_bytes = r.FP.lds;
    e->stats.jit_fallbacks = t.n_jit_miss;
    e->stats.pregen_group = t.pregen_group;
    e->stats.pregen_ms = t.ms_pregen;
    e->stats.h2d_ms = t.ms_h2d;
    e->stats.draw_bytes = t.draw_bytes;
    e->stats.state_bytes_per_scenario = r.bytes_per_lane;
    e->stats.state_in_lds = t.lds_state ? 1u : 0u;
    e->stats.lds_bytes_per_wave = t.lds_bytes;
    e->stats.waves = t.waves;
    e->stats.lanes_per_wave = t.kl;
    e->stats.chunks = t.n_chunks;
    e->stats.shared_instant_scenarios = t.n_rerun;
    e->stats.specialised_launches = t.n_jit;
    e->stats.request_capacity = e->request_capacity;
    e->stats.fifo_capacity = e->fifo_capacity;
    return AF_OK;
}

int af_engine_run(af_engine_t* e, const af_sweep_t* sweep, const af_outputs_t* out) {
    Run r;
    if (int rc = validate_sweep(e, sweep, out, r)) return rc;
    if (int rc = stage_sweep(r)) return rc;
    uint32_t chunk = 0;
    if (int rc = size_run(r, chunk)) return rc;
    bool on_flow = r.use_flow;
    for (uint32_t lo = 0; lo < r.n; lo += chunk) {
        const uint32_t nc = r.n - lo < chunk ? r.n - lo : chunk;
        r.t.n_chunks += 1u;
        const KArgs a = chunk_kargs(r, lo, nc);
        if (int rc = on_flow ? run_flow_chunk(r, a, lo, on_flow) : run_next_event(r, a, nc, nullptr)) return rc;
    }
    return write_stats(r);
}

int af_engine_jit_spec(af_engine_t* e, const af_sweep_t* sweep, const af_outputs_t* out, char* buf, size_t cap) {
    if (!e || !sweep || !out || !buf || cap == 0) return fail(AF_ERR_INVALID, "NULL argument");
    if (sweep->n_scenarios == 0) return fail(AF_ERR_INVALID, "empty sweep");
    if (!e->plan_only) HIP_TRY(hipSetDevice(e->device));
    KArgs a = e->args;
    uint32_t mask = 0;
    if (int rc = sweep_override_mask(sweep, false, mask)) return rc;
    a.L = af::make_layout(e->request_capacity, e->fifo_capacity, a.n_edges, a.n_servers, a.n_lb_edges, a.n_rows, mask, a.n_edge_marks, a.n_srv_marks);
    a.clock_cap = out->clock_capacity;
    a.tick_cap = out->tick_capacity;
    a.clock = out->clock;      // only their presence enters the spec
    a.samples = out->samples;
    a.online_hist = out->online_hist;
    a.online_rps = out->online_rps;
    if (int rc = draws_per_stream(sweep, out, a.n_draw)) return rc;
    bool on_flow = flow_wanted(e, sweep->n_scenarios);
    FlowPlan FP;
    if (on_flow) {
        for (uint32_t k = 0; k < sweep->n_overrides; ++k)
            if (!sweep->overrides[k].values) return fail(AF_ERR_INVALID, "bad override");
        const int rc = plan_flow(e, a, sweep, out, FP);
        if (rc == AF_ERR_CAPACITY && e->flow_mode != 2u) on_flow = false;   // (af_engine_run: the next-event kernels then)
        else if (rc) return rc;
    }
    if (on_flow) {   // the sweep runs on the stage-parallel kernel: its spec
        const std::string spec = flow_jit_spec_string(e, FP, out, sweep->n_overrides != 0u);
        if (spec.size() + 1 > cap) return fail(AF_ERR_CAPACITY, "spec buffer too small");
        std::memcpy(buf, spec.c_str(), spec.size() + 1);
        return AF_OK;
    }
    // (the next-event kernels' spec depends on the chunking, i.e. on the free device memory: not known without a device)
    if (e->plan_only) return fail(AF_ERR_NO_DEVICE, "planning-only engine: only sweeps of the stage-parallel kernel have a device-independent spec");
    size_t mem_free = 0, mem_total = 0;
    HIP_TRY(hipMemGetInfo(&mem_free, &mem_total));
    const uint32_t chunk = chunk_size(e, sweep->n_scenarios, (size_t)(1u + a.n_edges) * a.n_draw * sizeof(double), mem_free);
    if (chunk == 0) return fail(AF_ERR_CAPACITY, "draw_capacity too large for the device memory budget");
    uint32_t kl = 0;
    bool lds_state = false;
    choose_lanes(e, chunk, a.blob_bytes, af::layout_bytes_per_lane(a.L), kl, lds_state);
    const std::string spec = jit_spec_string(a, lds_state, klog_of(kl));
    if (spec.size() + 1 > cap) return fail(AF_ERR_CAPACITY, "spec buffer too small");
    std::memcpy(buf, spec.c_str(), spec.size() + 1);
    return AF_OK;
}

int af_engine_set_kernels(af_engine_t* e, const char* spec, const void* image, size_t size) {
    if (!e) return fail(AF_ERR_INVALID, "NULL argument");
    if (e->plan_only) return fail(AF_ERR_NO_DEVICE, "planning-only engine (AF_DEVICE_PLAN_ONLY)");
    HIP_TRY(hipSetDevice(e->device));
    const bool unload_all = !spec || !image || size == 0;
    const bool is_flow = spec && std::strstr(spec, "-DAF_FLOW_JIT=1") != nullptr;
    if (e->flow_jit_module && (unload_all || is_flow)) {
        HIP_TRY(hipStreamSynchronize(e->stream));
        (void)hipModuleUnload(e->flow_jit_module);
        e->flow_jit_module = nullptr;
        e->flow_jit_fn = nullptr;
        e->flow_jit_spec.clear();
        e->resident_waves.clear();   // (the next module's function may get the handle this one had)
    }
    if (is_flow && !unload_all) {   // a plan-specialised stage-parallel kernel (one entry point)
        hipModule_t mod = nullptr;
        HIP_TRY(hipModuleLoadData(&mod, image));
        hipFunction_t fn = nullptr;
        if (hipModuleGetFunction(&fn, mod, "af_flow_jit") != hipSuccess) {
            (void)hipModuleUnload(mod);
            return fail(AF_ERR_INVALID, "code object lacks af_flow_jit");
        }
        e->flow_jit_module = mod;
        e->flow_jit_fn = fn;
        e->flow_jit_spec = spec;
        return AF_OK;
    }
    if (e->jit_module) {
        HIP_TRY(hipStreamSynchronize(e->stream));
        (void)hipModuleUnload(e->jit_module);
        e->jit_module = nullptr;
        e->jit_lean = e->jit_order3 = e->jit_order2 = nullptr;
        e->jit_spec.clear();
    }
    if (!spec || !image || size == 0) return AF_OK;  // back to the generic kernels
    hipModule_t mod = nullptr;
    HIP_TRY(hipModuleLoadData(&mod, image));
    hipFunction_t f0 = nullptr, f1 = nullptr, f2 = nullptr;
    if (hipModuleGetFunction(&f0, mod, "af_jit_lean") != hipSuccess || hipModuleGetFunction(&f1, mod, "af_jit_order3") != hipSuccess ||
        hipModuleGetFunction(&f2, mod, "af_jit_order2") != hipSuccess) {
        (void)hipModuleUnload(mod);
        return fail(AF_ERR_INVALID, "code object lacks af_jit_lean / af_jit_order3 / af_jit_order2");
    }
    e->jit_module = mod;
    e->jit_lean = f0;
    e->jit_order3 = f1;
    e->jit_order2 = f2;
    e->jit_spec = spec;
    return AF_OK;
}

int af_engine_summarize(af_engine_t* e, const af_outputs_t* out, const af_summary_t* sum) {
    if (int rc = check_summary_request(e, out, sum)) return rc;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipEventRecord(e->ev0, e->stream));
    // (Measured, round 5: the series kernel on a second stream beside the latency kernel gains nothing -- 4.68 vs 4.65 ms for the
    // pair, both are HBM-bound -- and neither does the analyzer of a finished part of a sweep under the stage-parallel kernel of the
    // next part when every part pays the arrival chain's 5 ms again.  profiles/r05/summary_wpe_ab.txt, overlap_probe.log.  Round 6:
    // af_engine_run_summarized overlaps it with the LAST, partial residency round of ONE launch sequence instead.)
    if (int rc = launch_summary_kernels(e, out, sum, 0u, sum->n_scenarios, e->stream)) return rc;
    HIP_TRY(hipEventRecord(e->ev1, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e->ev0, e->ev1));
    e->stats.summary_ms = ms;
    e->stats.summary_overlapped = 0u;
    e->stats.summary_beside_ms = 0.0;
    return AF_OK;
}

// The pooled analyzer's engine-owned scratch: grown on demand (the contents are lost then), kept until the engine is destroyed.
// (After af_probe_scratch a grown pool starts as that call's word instead of as whatever hipMalloc returns.)
static int pool_fill(af_engine_t* e) {
    const size_t words = e->pool_cap / 4u, tail = e->pool_cap % 4u;
    if (words) HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)e->d_pool, (int)e->pool_word, words, e->stream));
    if (tail) HIP_TRY(hipMemsetAsync(e->d_pool + words * 4u, (int)(e->pool_word & 0xFFu), tail, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return AF_OK;
}
static int pool_reserve(af_engine_t* e, size_t bytes) {
    const size_t had = e->pool_cap;
    if (int rc = reserve_device((void**)&e->d_pool, e->pool_cap, bytes)) return rc;
    if (e->pool_poisoned && e->pool_cap != had) return pool_fill(e);
    return AF_OK;
}

// the layout of a request's scratch: 256-byte aligned parts, one after the other
struct ScratchLayout {
    size_t at = 0;
    size_t part(size_t bytes) {
        const size_t o = at;
        at += (bytes + 255u) & ~(size_t)255u;
        return o;
    }
};

constexpr uint64_t kBlocksPerLaunch = 1u << 21;   // workgroups of one launch of a kernel over any number of cells (at most 2^30 threads)

// the parts of that scratch that the tiled passes need for G groups
struct PoolParts {
    size_t grp, tile, piece, tmin, tmax, h0, dh, cn, cd, flag;
};
static PoolParts pool_parts(ScratchLayout& lay, size_t G, size_t n_tiles, uint64_t pieces) {
    PoolParts p{};
    p.grp = lay.part(std::max<size_t>(G, 1u) * sizeof(afp::PoolGroup));
    p.tile = lay.part(std::max<size_t>(n_tiles, 1u) * sizeof(afp::PoolTile));
    p.piece = lay.part(std::max<uint64_t>(pieces, 1u) * 8u);
    p.tmin = lay.part(std::max<size_t>(n_tiles, 1u) * 8u);
    p.tmax = lay.part(std::max<size_t>(n_tiles, 1u) * 8u);
    p.h0 = lay.part(G * afp::kExpBins * 4u);
    p.dh = lay.part(G * afp::kRanks * afp::kDigBins * 4u);
    p.cn = lay.part(G * afp::kRanks * 4u);
    p.cd = lay.part(G * afp::kRanks * afp::kCand * 8u);
    p.flag = lay.part(4u);
    return p;
}
static void pool_bind(afp::PoolArgs& a, unsigned char* b, const PoolParts& p) {
    a.groups = reinterpret_cast<afp::PoolGroup*>(b + p.grp);
    a.tiles = reinterpret_cast<const afp::PoolTile*>(b + p.tile);
    a.piece_sum = reinterpret_cast<double*>(b + p.piece);
    a.tile_min = reinterpret_cast<double*>(b + p.tmin);
    a.tile_max = reinterpret_cast<double*>(b + p.tmax);
    a.hist0 = reinterpret_cast<uint32_t*>(b + p.h0);
    a.dhist = reinterpret_cast<uint32_t*>(b + p.dh);
    a.cand_n = reinterpret_cast<uint32_t*>(b + p.cn);
    a.cand = reinterpret_cast<double*>(b + p.cd);
    a.any_more = reinterpret_cast<uint32_t*>(b + p.flag);
}

// one group more of `n` latencies at `off` of the compacted array: its pieces and the tiles of the streaming passes
static void pool_add_group(std::vector<afp::PoolGroup>& groups, std::vector<afp::PoolTile>& tiles, uint64_t& pieces, uint64_t off, uint32_t n) {
    const uint32_t g = (uint32_t)groups.size();
    afp::PoolGroup pg{};
    pg.off = off;
    pg.n = n;
    pg.n_pieces = (uint32_t)(((uint64_t)n + afp::kPiece - 1u) / afp::kPiece);
    pg.piece0 = (uint32_t)pieces;
    pg.tile0 = (uint32_t)tiles.size();
    for (uint32_t p = 0; p < pg.n_pieces; p += afp::kTilePieces)
        tiles.push_back(afp::PoolTile{g, p, std::min(afp::kTilePieces, pg.n_pieces - p), 0u});
    pg.n_tiles = (uint32_t)tiles.size() - pg.tile0;
    pieces += pg.n_pieces;
    groups.push_back(pg);
}

// The radix levels of G samples whose state is a.groups (af_select.hpp): launch_select(level) launches the analyzer's select
// kernel, af_pool_digits counts the next key bits, one level per launch pair while some sample still needs one (a 4-byte
// read-back decides).
static int radix_levels(hipStream_t st, const afp::PoolArgs& a, uint32_t G, uint32_t n_tiles, const char* analyzer, const std::function<void(int)>& launch_select) {
    for (int level = 0;; ++level) {   // (shift 52 -> 42 -> ... -> 2 -> 0: at most six digit levels)
        HIP_TRY(hipMemsetAsync(a.any_more, 0, 4u, st));
        launch_select(level);
        HIP_TRY(hipGetLastError());
        uint32_t more = 0;
        HIP_TRY(hipMemcpyAsync(&more, a.any_more, 4u, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (!more) return AF_OK;
        if (level >= 6) return fail(AF_ERR_HIP, std::string(analyzer) + " analyzer: radix select did not converge");
        HIP_TRY(hipMemsetAsync(a.dhist, 0, (size_t)G * afp::kRanks * afp::kDigBins * 4u, st));
        hipLaunchKernelGGL(afp::af_pool_digits, dim3(n_tiles), dim3(afp::kThreads), 0, st, a);
        HIP_TRY(hipGetLastError());
    }
}

// the passes over the compacted latencies (af_pooled.hpp) on the engine's stream; the last kernel is launched, not waited for
static int pool_run(af_engine_t* e, const afp::PoolArgs& a, const std::vector<afp::PoolGroup>& groups, const std::vector<afp::PoolTile>& tiles) {
    hipStream_t st = e->stream;
    const uint32_t G = (uint32_t)groups.size(), n_tiles = (uint32_t)tiles.size();
    HIP_TRY(hipMemcpyAsync(a.groups, groups.data(), (size_t)G * sizeof(afp::PoolGroup), hipMemcpyHostToDevice, st));
    if (n_tiles) HIP_TRY(hipMemcpyAsync(const_cast<afp::PoolTile*>(a.tiles), tiles.data(), (size_t)n_tiles * sizeof(afp::PoolTile), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(a.hist0, 0, (size_t)G * afp::kExpBins * 4u, st));
    if (n_tiles) hipLaunchKernelGGL(afp::af_pool_pass1, dim3(n_tiles), dim3(afp::kThreads), 0, st, a);
    HIP_TRY(hipGetLastError());
    if (int rc = radix_levels(st, a, G, n_tiles, "pooled", [&](int level) { hipLaunchKernelGGL(afp::af_pool_select, dim3(G), dim3(afp::kThreads), 0, st, a, level); }))
        return rc;
    HIP_TRY(hipMemsetAsync(a.cand_n, 0, (size_t)G * afp::kRanks * 4u, st));
    if (n_tiles) hipLaunchKernelGGL(afp::af_pool_last, dim3(n_tiles), dim3(afp::kThreads), 0, st, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(afp::af_pool_final, dim3(G), dim3(afp::kThreads), 0, st, a);
    HIP_TRY(hipGetLastError());
    return AF_OK;
}

static int check_window_edges(const double* edges, uint32_t W) {
    for (uint32_t k = 0; k <= W; ++k) {
        if (!std::isfinite(edges[k])) return fail(AF_ERR_INVALID, "window edge " + std::to_string(k) + " is not finite");
        if (k > 0 && !(edges[k - 1] < edges[k]))
            return fail(AF_ERR_INVALID, "window edges must be strictly increasing (edge " + std::to_string(k) + ")");
    }
    return AF_OK;
}

// the group ids of n scenarios to the host (none: all in group 0, grp stays empty), every one below G or AF_POOL_SKIP
static int check_group_ids(const std::vector<uint32_t>& grp, uint32_t G) {
    for (uint32_t s = 0; s < grp.size(); ++s)
        if (grp[s] != afp::kSkip && grp[s] >= G)
            return fail(AF_ERR_INVALID, "group id out of range (scenario " + std::to_string(s) + ": " + std::to_string(grp[s]) + ", n_groups " + std::to_string(G) + ")");
    return AF_OK;
}
static int read_groups(const uint32_t* group, uint32_t n, uint32_t G, std::vector<uint32_t>& grp) {
    grp.resize(group ? n : 0u);
    if (group) HIP_TRY(hipMemcpy(grp.data(), group, grp.size() * 4u, hipMemcpyDeviceToHost));
    return check_group_ids(grp, G);
}

// The cells of a request over whole runs: one per group, its sample the latencies of the group's members in ascending scenario
// index.  cell_off[g] is the cell's first latency in the compacted array, dst[s] the first of scenario s.
struct PooledCells {
    std::vector<uint64_t> cell_off, dst;   // [G + 1], [n]
};
static int layout_pooled_cells(const af_outputs_t* out, const std::vector<uint32_t>& grp, uint32_t n, uint32_t G, const char* holds, PooledCells& pc) {
    std::vector<uint32_t> counts((size_t)n * AF_CNT_SLOTS);
    HIP_TRY(hipMemcpy(counts.data(), out->counts, counts.size() * 4u, hipMemcpyDeviceToHost));
    pc.cell_off.assign((size_t)G + 1u, 0u);   // (first the sizes, at [g + 1])
    pc.dst.assign(n, 0u);
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t g = grp.empty() ? 0u : grp[s];
        if (g == afp::kSkip) continue;
        pc.dst[s] = pc.cell_off[1u + g];   // (for now: the latencies earlier members bring)
        pc.cell_off[1u + g] += std::min(counts[(size_t)s * AF_CNT_SLOTS + AF_CNT_COMPLETED], out->clock_capacity);
    }
    for (uint32_t g = 0; g < G; ++g) {
        if (pc.cell_off[1u + g] > 0xFFFFFFFFull) return fail(AF_ERR_CAPACITY, "group " + std::to_string(g) + " " + holds + " 2^32 or more latencies");
        pc.cell_off[1u + g] += pc.cell_off[g];
    }
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t g = grp.empty() ? 0u : grp[s];
        if (g != afp::kSkip) pc.dst[s] += pc.cell_off[g];
    }
    return AF_OK;
}
// ... and their latencies to lat (o_dst: a part of the scratch of n * 8 bytes; lat: cell_off[G] * 8 bytes, in the scratch or the caller's)
static int compact_pooled_cells(af_engine_t* e, const af_outputs_t* out, const uint32_t* group, uint32_t n, const PooledCells& pc, size_t o_dst, double* lat) {
    afp::PoolArgs a{};
    a.clock = out->clock;
    a.counts = out->counts;
    a.clock_cap = out->clock_capacity;
    a.cnt_completed_slot = AF_CNT_COMPLETED;
    a.group = group;
    a.dst = reinterpret_cast<const uint64_t*>(e->d_pool + o_dst);
    a.lat = lat;
    HIP_TRY(hipMemcpyAsync(e->d_pool + o_dst, pc.dst.data(), (size_t)n * 8u, hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(afp::af_pool_compact, dim3(n), dim3(afp::kThreads), 0, e->stream, a);
    HIP_TRY(hipGetLastError());
    return AF_OK;
}

// Pooled analyzer (af_pooled.hpp): the host reads counts and group ids back, checks them, and lays out the compacted array,
// the groups' pieces and the tiles of the streaming passes; the kernels run on the engine's stream.
int af_engine_summarize_pooled(af_engine_t* e, const af_outputs_t* out, af_pooled_t* pl) {
    if (!e || !out || !pl) return fail(AF_ERR_INVALID, "NULL argument");
    if (e->plan_only) return fail(AF_ERR_NO_DEVICE, "planning-only engine (AF_DEVICE_PLAN_ONLY)");
    if (pl->n_scenarios == 0 || pl->n_groups == 0) return fail(AF_ERR_INVALID, "empty pooled request (n_scenarios and n_groups must be > 0)");
    if (!pl->stats) return fail(AF_ERR_INVALID, "pooled.stats is required");
    if (!out->counts) return fail(AF_ERR_INVALID, "outputs.counts is required");
    if (!out->clock || out->clock_capacity == 0) return fail(AF_ERR_INVALID, "pooled summary needs outputs.clock");
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(e->device));
    const uint32_t n = pl->n_scenarios, G = pl->n_groups;
    std::vector<uint32_t> grp;
    if (int rc = read_groups(pl->group, n, G, grp)) return rc;
    PooledCells pc;
    if (int rc = layout_pooled_cells(out, grp, n, G, "pools", pc)) return rc;
    std::vector<afp::PoolGroup> groups;
    std::vector<afp::PoolTile> tiles;
    groups.reserve(G);
    uint64_t pieces = 0;
    for (uint32_t g = 0; g < G; ++g) pool_add_group(groups, tiles, pieces, pc.cell_off[g], (uint32_t)(pc.cell_off[g + 1u] - pc.cell_off[g]));
    ScratchLayout lay;
    const size_t o_lat = lay.part(pc.cell_off[G] * 8u), o_dst = lay.part((size_t)n * 8u);
    const PoolParts pp = pool_parts(lay, G, tiles.size(), pieces);
    if (int rc = pool_reserve(e, lay.at)) return rc;
    if (int rc = compact_pooled_cells(e, out, pl->group, n, pc, o_dst, reinterpret_cast<double*>(e->d_pool + o_lat))) return rc;
    afp::PoolArgs a{};
    a.lat = reinterpret_cast<double*>(e->d_pool + o_lat);
    pool_bind(a, e->d_pool, pp);
    a.stats = pl->stats;
    if (int rc = pool_run(e, a, groups, tiles)) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    pl->elapsed_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return AF_OK;
}

// The cells (group g, window w) of a request with windows by finish time (af_windowed.hpp), by arrival time (af_arrival.hpp) or
// by arrival time and the state met on arrival (af_state.hpp: W is then the number of keys, max(n_time, 1) * n_bins, and the edges
// are the n_time + 1 of the arrival windows, or none): layout_window_cells finds the row bounds (by arrival: the cumulative counts;
// by state: the cumulative cell counts) on the device and from them the cells' places; the caller sorts the cells into its tiers
// and adds its own parts to the scratch layout; compact_window_cells brings the latencies to their cells.  By arrival and by state
// nothing rests on the rows' order: it is not checked.
enum class CellsBy { kFinish, kArrival, kState };
struct WindowCells {
    afw::WinArgs a;                   // what the bounds / compaction kernels take (the analyzer's kernels too, where they take a WinArgs)
    CellsBy by;
    afst::StateArgs state;            // kState: the key (its WinArgs is bound at each launch)
    size_t n_edge;                    // the edges the request has: W + 1, by state n_time + 1 or none
    const double* edges;              // the caller's, [W + 1]
    uint32_t* row_bounds;             // the caller's, or null: the bounds lie in the scratch
    size_t o_edges, o_err, o_bounds, o_lat, o_pre, o_off;
    std::vector<uint32_t> hb, pre;    // the bounds [n][W + 1]; per (scenario, window) the latencies of its cell that earlier members bring
    std::vector<uint64_t> cell_off;   // [G * W + 1]
    // the export (af_engine_export_cells): the latencies go to the caller's buffer, and every scenario is its own group
    double* lat_dst = nullptr;                           // the caller's, or null: the compacted array lies in the scratch (o_lat)
    const std::vector<uint32_t>* own_group = nullptr;    // [n] group ids for the compaction, kept in the scratch at o_group
    size_t o_group = 0;
};
static void bind_window_bounds(const af_engine_t* e, WindowCells& wc) {
    wc.a.edges = reinterpret_cast<const double*>(e->d_pool + wc.o_edges);
    wc.a.err = reinterpret_cast<uint32_t*>(e->d_pool + wc.o_err);
    wc.a.bounds = wc.row_bounds ? wc.row_bounds : reinterpret_cast<uint32_t*>(e->d_pool + wc.o_bounds);
}
static int layout_window_cells(af_engine_t* e, const af_outputs_t* out, const uint32_t* group, const std::vector<uint32_t>& grp, uint32_t n, uint32_t G,
                               uint32_t W, const double* edges, uint32_t* row_bounds, CellsBy by, const afst::StateArgs* state, ScratchLayout& lay,
                               WindowCells& wc) {
    const size_t C = (size_t)G * W, NE = (size_t)n * (W + 1u);
    hipStream_t st = e->stream;
    const bool by_arrival = by == CellsBy::kArrival, by_state = by == CellsBy::kState;
    wc.by = by;
    wc.state = by_state ? *state : afst::StateArgs{};
    wc.n_edge = !by_state ? (size_t)W + 1u : state->n_time ? (size_t)state->n_time + 1u : 0u;
    wc.edges = edges;
    wc.row_bounds = row_bounds;
    // scratch, first part: edges, the error word, the bounds (unless the caller takes them)
    wc.o_edges = lay.part(std::max<size_t>(wc.n_edge, 1u) * 8u);
    wc.o_err = lay.part(4u);
    wc.o_bounds = row_bounds ? 0u : lay.part(NE * 4u);
    if (int rc = pool_reserve(e, lay.at)) return rc;
    wc.a = afw::WinArgs{};
    wc.a.clock = out->clock;
    wc.a.counts = out->counts;
    wc.a.clock_cap = out->clock_capacity;
    wc.a.cnt_completed_slot = AF_CNT_COMPLETED;
    wc.a.group = group;
    wc.a.n_scen = n;
    wc.a.n_win = W;
    bind_window_bounds(e, wc);
    if (wc.n_edge) HIP_TRY(hipMemcpyAsync(e->d_pool + wc.o_edges, edges, wc.n_edge * 8u, hipMemcpyHostToDevice, st));
    if (by_state) {
        wc.state.w = wc.a;
        if (W <= afst::kLdsStateCells)
            hipLaunchKernelGGL(afst::af_state_counts<true>, dim3(n), dim3(afst::kThreads), wc.n_edge * 8u + ((size_t)W + 1u) * 4u, st, wc.state);
        else
            hipLaunchKernelGGL(afst::af_state_counts<false>, dim3(n), dim3(afst::kThreads), 0, st, wc.state);
    } else if (!by_arrival)
        hipLaunchKernelGGL(afw::af_win_bounds, dim3((uint32_t)((NE + afw::kBoundsThreads - 1u) / afw::kBoundsThreads)), dim3(afw::kBoundsThreads), 0, st, wc.a);
    else if (W <= afw::kLdsArrivalWindows)
        hipLaunchKernelGGL(afw::af_arrival_counts<true>, dim3(n), dim3(afw::kThreads), ((size_t)W + 1u) * 12u, st, wc.a);
    else
        hipLaunchKernelGGL(afw::af_arrival_counts<false>, dim3(n), dim3(afw::kThreads), 0, st, wc.a);
    HIP_TRY(hipGetLastError());
    wc.hb.resize(NE);
    HIP_TRY(hipMemcpyAsync(wc.hb.data(), wc.a.bounds, NE * 4u, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // the cells: sizes, and per (scenario, window) the latencies of its cell that earlier members bring
    // (by finish: decreasing bounds -- a binary search on a sorted column cannot give them: the compaction would find the inversion too)
    const afc::LayoutResult lr = afc::layout_cells(wc.hb.data(), grp, n, G, W, by == CellsBy::kFinish, wc.cell_off, wc.pre);
    if (lr.error == afc::LayoutError::kOrder)
        return fail(AF_ERR_INVALID, "rqs_clock of scenario " + std::to_string(lr.scenario) + " is not in completion order (finish decreases): windows by finish time need it");
    if (lr.error == afc::LayoutError::kCellTooLarge)
        return fail(AF_ERR_CAPACITY, std::string(by_state ? "cell " : "window ") + std::to_string(lr.window) + " of group " + std::to_string(lr.group) + " holds 2^32 or more latencies");
    // scratch, second part: the compacted latencies (unless they go to the caller), pre, the cells' offsets; the caller's parts follow
    wc.o_lat = wc.lat_dst ? 0u : lay.part(wc.cell_off[C] * 8u);
    wc.o_pre = lay.part((size_t)n * W * 4u);
    wc.o_off = lay.part((C + 1u) * 8u);
    return AF_OK;
}
static int compact_window_cells(af_engine_t* e, const ScratchLayout& lay, WindowCells& wc) {
    hipStream_t st = e->stream;
    const uint32_t n = wc.a.n_scen, W = wc.a.n_win;
    const size_t NE = (size_t)n * (W + 1u);
    if (lay.at > e->pool_cap) {   // the scratch moves: its first part again
        if (int rc = pool_reserve(e, lay.at)) return rc;
        bind_window_bounds(e, wc);
        if (wc.n_edge) HIP_TRY(hipMemcpyAsync(e->d_pool + wc.o_edges, wc.edges, wc.n_edge * 8u, hipMemcpyHostToDevice, st));
        if (!wc.row_bounds) HIP_TRY(hipMemcpyAsync(wc.a.bounds, wc.hb.data(), NE * 4u, hipMemcpyHostToDevice, st));
    }
    unsigned char* b = e->d_pool;
    wc.a.lat = wc.lat_dst ? wc.lat_dst : reinterpret_cast<double*>(b + wc.o_lat);
    if (wc.own_group) {
        HIP_TRY(hipMemcpyAsync(b + wc.o_group, wc.own_group->data(), (size_t)n * 4u, hipMemcpyHostToDevice, st));
        wc.a.group = reinterpret_cast<const uint32_t*>(b + wc.o_group);
    }
    wc.a.pre = reinterpret_cast<uint32_t*>(b + wc.o_pre);
    wc.a.cell_off = reinterpret_cast<const uint64_t*>(b + wc.o_off);
    const uint32_t no_error = afw::kNoError;
    HIP_TRY(hipMemcpyAsync(b + wc.o_pre, wc.pre.data(), wc.pre.size() * 4u, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b + wc.o_off, wc.cell_off.data(), wc.cell_off.size() * 8u, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(wc.a.err, &no_error, 4u, hipMemcpyHostToDevice, st));
    const bool by_arrival = wc.by == CellsBy::kArrival;
    if (wc.by == CellsBy::kState) {
        wc.state.w = wc.a;
        if (W <= afst::kLdsStateCells)
            hipLaunchKernelGGL(afst::af_state_compact<true>, dim3(n), dim3(afst::kStateCompactThreads), wc.n_edge * 8u + (size_t)W * 8u, st, wc.state);
        else
            hipLaunchKernelGGL(afst::af_state_compact<false>, dim3(n), dim3(afst::kStateCompactThreads), 0, st, wc.state);
    } else if (by_arrival && W <= afw::kLdsArrivalWindows)
        hipLaunchKernelGGL(afw::af_arrival_compact<true>, dim3(n), dim3(afw::kArrivalCompactThreads), ((size_t)W + 1u) * 8u + (size_t)W * 8u, st, wc.a);
    else if (by_arrival)
        hipLaunchKernelGGL(afw::af_arrival_compact<false>, dim3(n), dim3(afw::kArrivalCompactThreads), 0, st, wc.a);
    else if (W <= afw::kLdsWindows)
        hipLaunchKernelGGL(afw::af_win_compact<true>, dim3(n), dim3(afw::kThreads), (size_t)W * 8u + ((size_t)W + 1u) * 4u, st, wc.a);
    else
        hipLaunchKernelGGL(afw::af_win_compact<false>, dim3(n), dim3(afw::kThreads), 0, st, wc.a);
    HIP_TRY(hipGetLastError());
    uint32_t bad = afw::kNoError;
    HIP_TRY(hipMemcpyAsync(&bad, wc.a.err, 4u, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (bad != afw::kNoError)
        return fail(AF_ERR_INVALID, "rqs_clock of scenario " + std::to_string(bad) + " is not in completion order (finish decreases): windows by finish time need it");
    return AF_OK;
}

// The key of a request by the state met on arrival (af_state.hpp), checked: the binning, the series, the sample rows.  K: the keys
// per group, max(n_time, 1) * n_bins.
static int check_state_bins(const af_engine_t* e, const af_outputs_t* out, const af_state_bins_t* sb, uint32_t n_time, uint32_t G, afst::StateArgs& sa, uint32_t& K) {
    if (sb->n_bins == 0) return fail(AF_ERR_INVALID, "state bins: n_bins must be > 0");
    if (!(std::isfinite(sb->width) && sb->width > 0.0)) return fail(AF_ERR_INVALID, "state bins: width must be finite and above 0");
    if (!std::isfinite(sb->lo)) return fail(AF_ERR_INVALID, "state bins: lo must be finite");
    if (!(std::isfinite(sb->sample_period) && sb->sample_period > 0.0)) return fail(AF_ERR_INVALID, "state bins: sample_period must be finite and above 0");
    const uint32_t S = e->args.n_edges + 3u * e->args.n_servers, pitch = e->args.series_pitch;
    if (S == 0 || pitch < S) return fail(AF_ERR_INVALID, "the plan has no sampled series");
    if (sb->column >= S) return fail(AF_ERR_INVALID, "state bins: column " + std::to_string(sb->column) + " is not a series (af_series_count " + std::to_string(S) + ")");
    if (!out->samples || out->tick_capacity == 0) return fail(AF_ERR_INVALID, "latency by state needs outputs.samples");
    const uint64_t wc = n_time ? n_time : 1u;
    if ((uint64_t)G * wc >= 0xFFFFFFFFull || (uint64_t)G * wc * sb->n_bins >= 0xFFFFFFFFull)
        return fail(AF_ERR_CAPACITY, "n_groups * max(n_windows, 1) * n_bins must be below 2^32 - 1");
    K = (uint32_t)(wc * sb->n_bins);
    sa = afst::StateArgs{};
    sa.samples = out->samples;
    sa.tick_cap = out->tick_capacity;
    sa.pitch = pitch;
    sa.cnt_ticks_slot = AF_CNT_TICKS;
    sa.column = sb->column;
    sa.is_float = sb->column >= e->args.n_edges && (sb->column - e->args.n_edges) % 3u == 2u ? 1u : 0u;
    sa.n_time = n_time;
    sa.n_bins = sb->n_bins;
    sa.lo = sb->lo;
    sa.width = sb->width;
    sa.period = sb->sample_period;
    return AF_OK;
}

// every cell of C to the wave kernel of a tiny tier, kTinyWaves cells per workgroup: launch(blocks, first cell)
static int launch_tiny_tier(uint64_t C, uint32_t tiny_waves, const std::function<void(uint32_t, uint64_t)>& launch) {
    for (uint64_t c0 = 0; c0 < C; c0 += kBlocksPerLaunch * tiny_waves) {   // every cell: a wave takes it if it is tiny (or empty)
        launch((uint32_t)std::min<uint64_t>(kBlocksPerLaunch, (C - c0 + tiny_waves - 1u) / tiny_waves), c0);
        HIP_TRY(hipGetLastError());
    }
    return AF_OK;
}

// The windowed analyzer behind the compacted array: what it needs are the cells' offsets alone.  plan_window_tiers sorts the C
// cells into the tiers of their sizes and adds the tiers' parts to the scratch layout (before the scratch is reserved);
// reduce_window_cells runs the tiers on lat / d_cell_off (DEVICE, the offsets [C + 1]) into stats; the last kernel is launched,
// not waited for.
struct WindowTiers {
    std::vector<afp::PoolGroup> groups;   // the large cells
    std::vector<afp::PoolTile> tiles;
    std::vector<uint32_t> stat_row, small;
    size_t o_row = 0, o_small = 0;
    PoolParts pp{};
};
static void plan_window_tiers(const std::vector<uint64_t>& cell_off, size_t C, ScratchLayout& lay, WindowTiers& t) {
    uint64_t pieces = 0;
    for (size_t c = 0; c < C; ++c) {
        const uint64_t len = cell_off[c + 1u] - cell_off[c];
        if (len > afw::kSmallMax) {
            pool_add_group(t.groups, t.tiles, pieces, cell_off[c], (uint32_t)len);
            t.stat_row.push_back((uint32_t)c);
        } else if (len > afw::kTinyMax) {
            t.small.push_back((uint32_t)c);
        }
    }
    t.o_row = lay.part(t.groups.size() * 4u);
    t.o_small = lay.part(t.small.size() * 4u);
    t.pp = !t.groups.empty() ? pool_parts(lay, t.groups.size(), t.tiles.size(), pieces) : PoolParts{};
}
static int reduce_window_cells(af_engine_t* e, const WindowTiers& t, afw::WinArgs a, size_t C, double* stats) {
    hipStream_t st = e->stream;
    unsigned char* b = e->d_pool;
    const uint32_t n_large = (uint32_t)t.groups.size(), n_small = (uint32_t)t.small.size();
    a.small = reinterpret_cast<const uint32_t*>(b + t.o_small);
    a.stats = stats;
    if (n_small) HIP_TRY(hipMemcpyAsync(b + t.o_small, t.small.data(), (size_t)n_small * 4u, hipMemcpyHostToDevice, st));
    if (int rc = launch_tiny_tier(C, afw::kTinyWaves, [&](uint32_t blocks, uint64_t c0) {
            hipLaunchKernelGGL(afw::af_win_tiny, dim3(blocks), dim3(afw::kTinyWaves * 64), 0, st, a, c0, (uint64_t)C);
        }))
        return rc;
    for (uint64_t c0 = 0; c0 < n_small; c0 += kBlocksPerLaunch) {
        hipLaunchKernelGGL(afw::af_win_small, dim3((uint32_t)std::min<uint64_t>(kBlocksPerLaunch, n_small - c0)), dim3(afw::kThreads), 0, st, a, (uint32_t)c0);
        HIP_TRY(hipGetLastError());
    }
    if (n_large) {
        afp::PoolArgs pa{};
        pa.lat = a.lat;
        pool_bind(pa, b, t.pp);
        pa.stats = stats;
        pa.stat_row = reinterpret_cast<const uint32_t*>(b + t.o_row);
        HIP_TRY(hipMemcpyAsync(b + t.o_row, t.stat_row.data(), (size_t)n_large * 4u, hipMemcpyHostToDevice, st));
        if (int rc = pool_run(e, pa, t.groups, t.tiles)) return rc;
    }
    return AF_OK;
}

// Windowed analyzer (af_windowed.hpp; windows by arrival: af_arrival.hpp; by the state met on arrival, `sb`: af_state.hpp, the
// "windows" W of everything below are then the keys of a group and n_windows == 0 is one window over all time).  The host reads
// the row bounds back and lays out the cells (group g, window w) of the compacted array; cells of at most one numpy piece are
// reduced by one workgroup each, larger ones by the pooled analyzer's tiled passes.
static int summarize_windows(af_engine_t* e, const af_outputs_t* out, af_windows_t* win, CellsBy by, const af_state_bins_t* sb = nullptr) {
    if (!e || !out || !win || (by == CellsBy::kState && !sb)) return fail(AF_ERR_INVALID, "NULL argument");
    if (e->plan_only) return fail(AF_ERR_NO_DEVICE, "planning-only engine (AF_DEVICE_PLAN_ONLY)");
    if (win->n_scenarios == 0 || win->n_groups == 0 || (win->n_windows == 0 && !sb))
        return fail(AF_ERR_INVALID, "empty windows request (n_scenarios, n_groups and n_windows must be > 0)");
    if (!win->stats) return fail(AF_ERR_INVALID, "windows.stats is required");
    if (win->n_windows > 0 && !win->edges) return fail(AF_ERR_INVALID, "windows.edges is required");
    if (win->n_windows == 0 && win->edges) return fail(AF_ERR_INVALID, "windows.edges given with n_windows == 0 (one window over all time takes none)");
    if (!out->counts) return fail(AF_ERR_INVALID, "outputs.counts is required");
    if (!out->clock || out->clock_capacity == 0) return fail(AF_ERR_INVALID, "windowed summary needs outputs.clock");
    const uint32_t n = win->n_scenarios, G = win->n_groups;
    if (win->n_windows > 0)
        if (int rc = check_window_edges(win->edges, win->n_windows)) return rc;
    uint32_t W = win->n_windows;   // the cells of a group
    afst::StateArgs sa{};
    if (sb) {
        if (int rc = check_state_bins(e, out, sb, win->n_windows, G, sa, W)) return rc;
    }
    if ((uint64_t)G * W >= 0xFFFFFFFFull) return fail(AF_ERR_CAPACITY, "n_groups * n_windows must be below 2^32 - 1");
    if ((uint64_t)n * ((uint64_t)W + 1u) > 0xFFFFFFFFull) return fail(AF_ERR_CAPACITY, "n_scenarios * (n_windows + 1) must be below 2^32");
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(e->device));
    const size_t C = (size_t)G * W;
    std::vector<uint32_t> grp;
    if (int rc = read_groups(win->group, n, G, grp)) return rc;
    ScratchLayout lay;
    WindowCells wc;
    if (int rc = layout_window_cells(e, out, win->group, grp, n, G, W, win->edges, win->row_bounds, by, sb ? &sa : nullptr, lay, wc)) return rc;
    WindowTiers tiers;
    plan_window_tiers(wc.cell_off, C, lay, tiers);
    const int rc_compact = compact_window_cells(e, lay, wc);
    win->scratch_bytes = e->pool_cap;
    if (rc_compact) return rc_compact;
    if (int rc = reduce_window_cells(e, tiers, wc.a, C, win->stats)) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    win->elapsed_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return AF_OK;
}
int af_engine_summarize_windows(af_engine_t* e, const af_outputs_t* out, af_windows_t* win) { return summarize_windows(e, out, win, CellsBy::kFinish); }
int af_engine_summarize_arrival_windows(af_engine_t* e, const af_outputs_t* out, af_windows_t* win) { return summarize_windows(e, out, win, CellsBy::kArrival); }
int af_engine_summarize_state_windows(af_engine_t* e, const af_outputs_t* out, const af_state_bins_t* sb, af_windows_t* win) {
    return summarize_windows(e, out, win, CellsBy::kState, sb);
}

// the levels and thresholds of a quantile request (af_quantiles_t's rules)
static int check_quantile_levels(uint32_t Q, const double* levels, uint32_t T, const double* thresholds) {
    if (Q > AF_MAX_QUANTILE_LEVELS) return fail(AF_ERR_INVALID, "more than AF_MAX_QUANTILE_LEVELS (" + std::to_string(AF_MAX_QUANTILE_LEVELS) + ") levels");
    if (T > AF_MAX_SLO_THRESHOLDS) return fail(AF_ERR_INVALID, "more than AF_MAX_SLO_THRESHOLDS (" + std::to_string(AF_MAX_SLO_THRESHOLDS) + ") thresholds");
    if (Q == 0 && T == 0) return fail(AF_ERR_INVALID, "quantiles request without levels and without thresholds");
    if (Q && !levels) return fail(AF_ERR_INVALID, "quantiles.levels is required with n_levels > 0");
    if (T && !thresholds) return fail(AF_ERR_INVALID, "quantiles.thresholds is required with n_thresholds > 0");
    for (uint32_t i = 0; i < Q; ++i)
        if (!(levels[i] >= 0.0 && levels[i] <= 1.0)) return fail(AF_ERR_INVALID, "quantile level " + std::to_string(i) + " is not in [0, 1]");
    for (uint32_t i = 0; i < T; ++i)
        if (std::isnan(thresholds[i])) return fail(AF_ERR_INVALID, "threshold " + std::to_string(i) + " is NaN");
    return AF_OK;
}

// The quantile analyzer behind the compacted array, as the windowed analyzer's pair above: plan_quantile_tiers sorts the C cells
// into their tiers and adds the tiers' parts to the scratch layout; reduce_quantile_cells runs them on lat / d_cell_off (DEVICE).
struct QuantileOutputs {
    uint32_t Q, T;
    const double *levels, *thresholds;   // HOST
    uint32_t* count;                     // DEVICE, each may be null
    double* quantiles;
    uint32_t* within;
};
struct QuantileTiers {
    struct SmallCell { uint32_t pad, cell; };
    std::vector<SmallCell> small_by;
    std::vector<uint32_t> small;
    std::vector<afq::QCell> lcells;
    std::vector<afp::PoolTile> ctiles, jtiles;
    std::vector<afp::PoolGroup> jgroups;
    std::vector<afq::QJob> jobs;
    size_t o_small = 0, o_lev = 0, o_thr = 0, o_lcell = 0, o_ctile = 0, o_job = 0, o_thist = 0;
    PoolParts pp{};
};
static void plan_quantile_tiers(const std::vector<uint64_t>& cell_off, size_t C, const QuantileOutputs& qo, ScratchLayout& lay, QuantileTiers& t) {
    const uint32_t Q = qo.Q, T = qo.T;
    for (size_t c = 0; c < C; ++c) {
        const uint64_t len = cell_off[c + 1u] - cell_off[c];
        if (len > afq::kSmallMax) {
            t.lcells.push_back(afq::QCell{cell_off[c], (uint32_t)len, (uint32_t)c});
        } else if (len > afq::kTinyMax) {
            uint32_t pad = afq::kSmallMinPad;
            while (pad < len) pad <<= 1;
            t.small_by.push_back(QuantileTiers::SmallCell{pad, (uint32_t)c});
        }
    }
    std::stable_sort(t.small_by.begin(), t.small_by.end(), [](const QuantileTiers::SmallCell& x, const QuantileTiers::SmallCell& y) { return x.pad < y.pad; });
    t.small.resize(t.small_by.size());
    for (size_t i = 0; i < t.small_by.size(); ++i) t.small[i] = t.small_by[i].cell;
    const uint32_t n_small = (uint32_t)t.small.size(), n_large = (uint32_t)t.lcells.size();
    const bool want_q = Q > 0 && qo.quantiles;
    // large cells: their tiles, and a job per cell and kLv levels
    uint64_t pieces_unused = 0;
    for (uint32_t lc = 0; lc < n_large; ++lc) {
        const uint32_t np = (uint32_t)(((uint64_t)t.lcells[lc].n + afp::kPiece - 1u) / afp::kPiece);
        for (uint32_t p = 0; p < np; p += afp::kTilePieces) t.ctiles.push_back(afp::PoolTile{lc, p, std::min(afp::kTilePieces, np - p), 0u});
        for (uint32_t l0 = 0; want_q && l0 < Q; l0 += afq::kLv) {
            pool_add_group(t.jgroups, t.jtiles, pieces_unused, t.lcells[lc].off, t.lcells[lc].n);
            t.jobs.push_back(afq::QJob{lc, l0, std::min<uint32_t>(afq::kLv, Q - l0), 0u});
        }
    }
    const uint32_t n_jobs = (uint32_t)t.jobs.size(), n_ctiles = (uint32_t)t.ctiles.size();
    t.o_small = lay.part((size_t)n_small * 4u);
    t.o_lev = lay.part((size_t)Q * 8u);
    t.o_thr = lay.part((size_t)T * 8u);
    t.o_lcell = lay.part((size_t)n_large * sizeof(afq::QCell));
    t.o_ctile = lay.part((size_t)n_ctiles * sizeof(afp::PoolTile));
    t.o_job = lay.part((size_t)n_jobs * sizeof(afq::QJob));
    t.o_thist = lay.part((size_t)n_large * T * 4u);
    t.pp = n_jobs ? pool_parts(lay, n_jobs, t.jtiles.size(), 1u) : PoolParts{};
}
static int reduce_quantile_cells(af_engine_t* e, const QuantileTiers& t, const QuantileOutputs& qo, const double* lat, const uint64_t* d_cell_off, size_t C) {
    hipStream_t st = e->stream;
    unsigned char* b = e->d_pool;
    const uint32_t Q = qo.Q, T = qo.T;
    const uint32_t n_small = (uint32_t)t.small.size(), n_large = (uint32_t)t.lcells.size();
    const uint32_t n_jobs = (uint32_t)t.jobs.size(), n_ctiles = (uint32_t)t.ctiles.size();
    const bool want_q = Q > 0 && qo.quantiles, want_w = T > 0 && qo.within;
    afq::QArgs qa{};
    qa.lat = lat;
    qa.cell_off = d_cell_off;
    qa.n_lev = Q;
    qa.n_thr = T;
    qa.levels = reinterpret_cast<const double*>(b + t.o_lev);
    qa.thr = reinterpret_cast<const double*>(b + t.o_thr);
    qa.count = qo.count;
    qa.quant = qo.quantiles;
    qa.within = qo.within;
    qa.small = reinterpret_cast<const uint32_t*>(b + t.o_small);
    qa.lcells = reinterpret_cast<const afq::QCell*>(b + t.o_lcell);
    qa.ctiles = reinterpret_cast<const afp::PoolTile*>(b + t.o_ctile);
    qa.jobs = reinterpret_cast<const afq::QJob*>(b + t.o_job);
    qa.thist = reinterpret_cast<uint32_t*>(b + t.o_thist);
    if (Q) HIP_TRY(hipMemcpyAsync(b + t.o_lev, qo.levels, (size_t)Q * 8u, hipMemcpyHostToDevice, st));
    if (T) HIP_TRY(hipMemcpyAsync(b + t.o_thr, qo.thresholds, (size_t)T * 8u, hipMemcpyHostToDevice, st));
    if (n_small) HIP_TRY(hipMemcpyAsync(b + t.o_small, t.small.data(), (size_t)n_small * 4u, hipMemcpyHostToDevice, st));
    if (qo.count || want_q || want_w) {
        if (int rc = launch_tiny_tier(C, afq::kTinyWaves, [&](uint32_t blocks, uint64_t c0) {
                hipLaunchKernelGGL(afq::af_q_tiny, dim3(blocks), dim3(afq::kTinyWaves * 64), 0, st, qa, c0, (uint64_t)C);
            }))
            return rc;
        for (size_t i0 = 0; i0 < t.small_by.size();) {   // the small cells, one padded size after the other
            size_t i1 = i0;
            while (i1 < t.small_by.size() && t.small_by[i1].pad == t.small_by[i0].pad && i1 - i0 < kBlocksPerLaunch) ++i1;
            hipLaunchKernelGGL(afq::af_q_small, dim3((uint32_t)(i1 - i0)), dim3(afq::kThreads), (size_t)t.small_by[i0].pad * 8u, st, qa, (uint32_t)i0, t.small_by[i0].pad);
            HIP_TRY(hipGetLastError());
            i0 = i1;
        }
    }
    if (n_large) {
        HIP_TRY(hipMemcpyAsync(b + t.o_lcell, t.lcells.data(), (size_t)n_large * sizeof(afq::QCell), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(b + t.o_ctile, t.ctiles.data(), (size_t)n_ctiles * sizeof(afp::PoolTile), hipMemcpyHostToDevice, st));
        afp::PoolArgs pa{};
        pa.lat = const_cast<double*>(qa.lat);
        if (n_jobs) {
            pool_bind(pa, b, t.pp);
            HIP_TRY(hipMemcpyAsync(b + t.o_job, t.jobs.data(), (size_t)n_jobs * sizeof(afq::QJob), hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(pa.groups, t.jgroups.data(), (size_t)n_jobs * sizeof(afp::PoolGroup), hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(const_cast<afp::PoolTile*>(pa.tiles), t.jtiles.data(), t.jtiles.size() * sizeof(afp::PoolTile), hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemsetAsync(pa.hist0, 0, (size_t)n_large * afp::kExpBins * 4u, st));   // (one per cell: the first n_large of the jobs')
        }
        if (want_w) HIP_TRY(hipMemsetAsync(qa.thist, 0, (size_t)n_large * T * 4u, st));
        if (n_jobs || want_w) {
            hipLaunchKernelGGL(afq::af_q_pass0, dim3(n_ctiles), dim3(afq::kThreads), 0, st, qa, pa.hist0);
            HIP_TRY(hipGetLastError());
        }
        if (n_jobs) {
            const uint32_t n_jtiles = (uint32_t)t.jtiles.size();
            if (int rc = radix_levels(st, pa, n_jobs, n_jtiles, "quantile", [&](int level) { hipLaunchKernelGGL(afq::af_q_select, dim3(n_jobs), dim3(afq::kThreads), 0, st, qa, pa, level); }))
                return rc;
            HIP_TRY(hipMemsetAsync(pa.cand_n, 0, (size_t)n_jobs * afp::kRanks * 4u, st));
            hipLaunchKernelGGL(afq::af_q_cand, dim3(n_jtiles), dim3(afq::kThreads), 0, st, pa);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(afq::af_q_final, dim3(n_jobs), dim3(afq::kThreads), 0, st, qa, pa);
            HIP_TRY(hipGetLastError());
        }
        if (qo.count || want_w) {
            hipLaunchKernelGGL(afq::af_q_large_rows, dim3(n_large), dim3(64), 0, st, qa);
            HIP_TRY(hipGetLastError());
        }
    }
    return AF_OK;
}

// Quantile analyzer (af_quantiles.hpp).  The cells are laid out and compacted as the windowed analyzer's (n_windows > 0; by the
// state met on arrival, `sb`, always: W is then the keys of a group) or the pooled one's (n_windows == 0: a cell per group; not by
// arrival: a whole run has no window); a cell then goes to the tier of its size.
static int summarize_quantiles(af_engine_t* e, const af_outputs_t* out, af_quantiles_t* qr, CellsBy by, const af_state_bins_t* sb = nullptr) {
    if (!e || !out || !qr || (by == CellsBy::kState && !sb)) return fail(AF_ERR_INVALID, "NULL argument");
    if (e->plan_only) return fail(AF_ERR_NO_DEVICE, "planning-only engine (AF_DEVICE_PLAN_ONLY)");
    if (by == CellsBy::kArrival && qr->n_windows == 0) return fail(AF_ERR_INVALID, "quantiles by arrival time need windows (n_windows must be > 0)");
    if (qr->n_scenarios == 0 || qr->n_groups == 0) return fail(AF_ERR_INVALID, "empty quantiles request (n_scenarios and n_groups must be > 0)");
    const uint32_t n = qr->n_scenarios, G = qr->n_groups, cap = out->clock_capacity, Q = qr->n_levels, T = qr->n_thresholds;
    uint32_t W = qr->n_windows;   // the cells of a group laid out as windows (0: a cell per group over the whole run); by state: the keys
    if (int rc = check_quantile_levels(Q, qr->levels, T, qr->thresholds)) return rc;
    if (W > 0 && !qr->edges) return fail(AF_ERR_INVALID, "quantiles.edges is required with n_windows > 0");
    if (W == 0 && qr->edges) return fail(AF_ERR_INVALID, "quantiles.edges given with n_windows == 0 (whole-run mode takes none)");
    if (W > 0)
        if (int rc = check_window_edges(qr->edges, W)) return rc;
    if (!out->counts) return fail(AF_ERR_INVALID, "outputs.counts is required");
    if (!out->clock || cap == 0) return fail(AF_ERR_INVALID, "quantile summary needs outputs.clock");
    afst::StateArgs sa{};
    if (sb) {
        if (int rc = check_state_bins(e, out, sb, qr->n_windows, G, sa, W)) return rc;
    }
    const uint32_t Wc = W ? W : 1u;
    if ((uint64_t)G * Wc >= 0xFFFFFFFFull) return fail(AF_ERR_CAPACITY, "n_groups * max(n_windows, 1) must be below 2^32 - 1");
    if (W && (uint64_t)n * ((uint64_t)W + 1u) > 0xFFFFFFFFull) return fail(AF_ERR_CAPACITY, "n_scenarios * (n_windows + 1) must be below 2^32");
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(e->device));
    const size_t C = (size_t)G * Wc;
    std::vector<uint32_t> grp;
    if (int rc = read_groups(qr->group, n, G, grp)) return rc;
    hipStream_t st = e->stream;
    ScratchLayout lay;
    WindowCells wc;     // the cells with windows
    PooledCells pc;     // ... and without
    if (W) {
        if (int rc = layout_window_cells(e, out, qr->group, grp, n, G, W, qr->edges, nullptr, by, sb ? &sa : nullptr, lay, wc)) return rc;
    } else {
        if (int rc = layout_pooled_cells(out, grp, n, G, "holds", pc)) return rc;
        lay.part(8u), lay.part(4u);   // (an edge and the error word, as with windows: the scratch of a request is as large as it was)
    }
    const std::vector<uint64_t>& cell_off = W ? wc.cell_off : pc.cell_off;
    const size_t o_lat = W ? wc.o_lat : lay.part(cell_off[C] * 8u), o_dst = W ? 0u : lay.part((size_t)n * 8u), o_off = W ? wc.o_off : lay.part((C + 1u) * 8u);
    const QuantileOutputs qo{Q, T, qr->levels, qr->thresholds, qr->count, qr->quantiles, qr->within};
    QuantileTiers tiers;
    plan_quantile_tiers(cell_off, C, qo, lay, tiers);
    if (W) {
        const int rc = compact_window_cells(e, lay, wc);
        qr->scratch_bytes = e->pool_cap;
        if (rc) return rc;
    } else {
        if (int rc = pool_reserve(e, lay.at)) return rc;
        qr->scratch_bytes = e->pool_cap;
        HIP_TRY(hipMemcpyAsync(e->d_pool + o_off, cell_off.data(), (C + 1u) * 8u, hipMemcpyHostToDevice, st));
        if (int rc = compact_pooled_cells(e, out, qr->group, n, pc, o_dst, reinterpret_cast<double*>(e->d_pool + o_lat))) return rc;
    }
    if (int rc = reduce_quantile_cells(e, tiers, qo, reinterpret_cast<const double*>(e->d_pool + o_lat), reinterpret_cast<const uint64_t*>(e->d_pool + o_off), C)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    qr->elapsed_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return AF_OK;
}
int af_engine_summarize_quantiles(af_engine_t* e, const af_outputs_t* out, af_quantiles_t* qr) { return summarize_quantiles(e, out, qr, CellsBy::kFinish); }
int af_engine_summarize_arrival_quantiles(af_engine_t* e, const af_outputs_t* out, af_quantiles_t* qr) { return summarize_quantiles(e, out, qr, CellsBy::kArrival); }
int af_engine_summarize_state_quantiles(af_engine_t* e, const af_outputs_t* out, const af_state_bins_t* sb, af_quantiles_t* qr) {
    return summarize_quantiles(e, out, qr, CellsBy::kState, sb);
}

// Cells across devices (af_cells.hpp), the exporting side: the windowed layout and compaction above with every scenario as its own
// group -- so pre == 0 and a scenario's windows follow one another -- into the caller's buffer.  The bounds stay in the scratch
// until the call cannot fail any more: a refused call writes nothing.
int af_engine_export_cells(af_engine_t* e, const af_outputs_t* out, af_cells_export_t* ex) {
    if (!e || !out || !ex) return fail(AF_ERR_INVALID, "NULL argument");
    if (e->plan_only) return fail(AF_ERR_NO_DEVICE, "planning-only engine (AF_DEVICE_PLAN_ONLY)");
    if (ex->n_scenarios == 0) return fail(AF_ERR_INVALID, "empty export request (n_scenarios must be > 0)");
    if (!ex->seg_bounds) return fail(AF_ERR_INVALID, "cells_export.seg_bounds is required");
    if (ex->lat_capacity > 0 && !ex->lat) return fail(AF_ERR_INVALID, "cells_export.lat is required with lat_capacity > 0");
    if (ex->n_windows > 0 && !ex->edges) return fail(AF_ERR_INVALID, "cells_export.edges is required with n_windows > 0");
    if (ex->n_windows == 0 && ex->edges) return fail(AF_ERR_INVALID, "cells_export.edges given with n_windows == 0 (the whole run takes none)");
    if (ex->n_windows == 0 && ex->by_arrival) return fail(AF_ERR_INVALID, "an export by arrival time needs windows (n_windows must be > 0)");
    if (!out->counts) return fail(AF_ERR_INVALID, "outputs.counts is required");
    if (!out->clock || out->clock_capacity == 0) return fail(AF_ERR_INVALID, "the export of cells needs outputs.clock");
    const uint32_t n = ex->n_scenarios, W = ex->n_windows;
    if (W > 0)
        if (int rc = check_window_edges(ex->edges, W)) return rc;
    if ((uint64_t)n * std::max(W, 1u) >= 0xFFFFFFFFull) return fail(AF_ERR_CAPACITY, "n_scenarios * max(n_windows, 1) must be below 2^32 - 1");
    if ((uint64_t)n * ((uint64_t)W + 1u) > 0xFFFFFFFFull) return fail(AF_ERR_CAPACITY, "n_scenarios * (n_windows + 1) must be below 2^32");
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(e->device));
    std::vector<uint32_t> grp;   // (only AF_POOL_SKIP matters here: the ids are the importing call's to check)
    if (int rc = read_groups(ex->group, n, 0xFFFFFFFFu, grp)) return rc;
    hipStream_t st = e->stream;
    ScratchLayout lay;
    std::vector<uint32_t> own(n);   // every scenario its own group
    for (uint32_t s = 0; s < n; ++s) own[s] = s;
    if (W == 0) {   // the whole run: the pooled compaction, a scenario's rows behind those of the scenarios before it
        PooledCells pc;   // (laid out for every scenario, the skipped ones too: cell_off[s + 1] - cell_off[s] is m_s)
        if (int rc = layout_pooled_cells(out, own, n, n, "holds", pc)) return rc;
        std::vector<uint32_t> hb((size_t)n * 2u);
        uint64_t total = 0;
        for (uint32_t s = 0; s < n; ++s) {
            hb[2u * s] = 0u;
            hb[2u * s + 1u] = (uint32_t)(pc.cell_off[s + 1u] - pc.cell_off[s]);
            pc.dst[s] = total;
            if (grp.empty() || grp[s] != afp::kSkip) total += hb[2u * s + 1u];
        }
        if (total > ex->lat_capacity)
            return fail(AF_ERR_CAPACITY, "cells_export.lat_capacity " + std::to_string(ex->lat_capacity) + " is below the " + std::to_string(total) + " latencies to export");
        const size_t o_dst = lay.part((size_t)n * 8u);
        if (int rc = pool_reserve(e, lay.at)) return rc;
        ex->scratch_bytes = e->pool_cap;
        if (int rc = compact_pooled_cells(e, out, ex->group, n, pc, o_dst, ex->lat)) return rc;
        HIP_TRY(hipMemcpyAsync(ex->seg_bounds, hb.data(), hb.size() * 4u, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
        ex->lat_count = total;
    } else {
        for (uint32_t s = 0; s < n; ++s)
            if (!grp.empty() && grp[s] == afp::kSkip) own[s] = afp::kSkip;
        WindowCells wc;
        wc.lat_dst = ex->lat;
        wc.own_group = &own;
        wc.o_group = lay.part((size_t)n * 4u);
        if (int rc = layout_window_cells(e, out, nullptr, own, n, n, W, ex->edges, nullptr, ex->by_arrival ? CellsBy::kArrival : CellsBy::kFinish, nullptr, lay, wc))
            return rc;
        const uint64_t total = wc.cell_off[(size_t)n * W];
        if (total > ex->lat_capacity)
            return fail(AF_ERR_CAPACITY, "cells_export.lat_capacity " + std::to_string(ex->lat_capacity) + " is below the " + std::to_string(total) + " latencies to export");
        const int rc = compact_window_cells(e, lay, wc);
        ex->scratch_bytes = e->pool_cap;
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(ex->seg_bounds, wc.hb.data(), wc.hb.size() * 4u, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
        ex->lat_count = total;
    }
    ex->elapsed_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return AF_OK;
}

// ... and the importing side: the segments are checked and the cells laid out on the host from the bounds alone, af_cells_merge
// brings every member's segment to its cells, and the windowed / quantile tiers above reduce the merged array.
int af_engine_import_cells(af_engine_t* e, af_cells_t* cr) {
    if (!e || !cr) return fail(AF_ERR_INVALID, "NULL argument");
    if (e->plan_only) return fail(AF_ERR_NO_DEVICE, "planning-only engine (AF_DEVICE_PLAN_ONLY)");
    if (cr->n_scenarios == 0 || cr->n_groups == 0) return fail(AF_ERR_INVALID, "empty cells request (n_scenarios and n_groups must be > 0)");
    if (!cr->seg_bounds || !cr->seg_begin) return fail(AF_ERR_INVALID, "cells.seg_bounds and cells.seg_begin are required");
    if (cr->n_lat > 0 && !cr->lat) return fail(AF_ERR_INVALID, "cells.lat is required with n_lat > 0");
    const uint32_t n = cr->n_scenarios, G = cr->n_groups, Wc = std::max(cr->n_windows, 1u), Q = cr->n_levels, T = cr->n_thresholds;
    const bool want_quantiles = cr->count || cr->quantiles || cr->within;
    if (!cr->stats && !want_quantiles) return fail(AF_ERR_INVALID, "cells request without an output (stats, count, quantiles or within)");
    if (want_quantiles)
        if (int rc = check_quantile_levels(Q, cr->levels, T, cr->thresholds)) return rc;
    if ((uint64_t)G * Wc >= 0xFFFFFFFFull) return fail(AF_ERR_CAPACITY, "n_groups * max(n_windows, 1) must be below 2^32 - 1");
    if ((uint64_t)n * ((uint64_t)Wc + 1u) > 0xFFFFFFFFull) return fail(AF_ERR_CAPACITY, "n_scenarios * (max(n_windows, 1) + 1) must be below 2^32");
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint32_t> grp;
    if (cr->group) grp.assign(cr->group, cr->group + n);
    if (int rc = check_group_ids(grp, G)) return rc;
    // the segments: inside the imported array, no two of them overlapping
    const size_t C = (size_t)G * Wc;
    std::vector<std::pair<uint64_t, uint64_t>> segs;   // (begin, length) of the members that bring something
    for (uint32_t s = 0; s < n; ++s) {
        if (!grp.empty() && grp[s] == afc::kSkip) continue;
        const uint32_t* r = cr->seg_bounds + (size_t)s * (Wc + 1u);
        if (r[Wc] < r[0]) return fail(AF_ERR_INVALID, "cells.seg_bounds of scenario " + std::to_string(s) + " decrease");
        const uint64_t len = r[Wc] - r[0], begin = cr->seg_begin[s];
        if (begin > cr->n_lat || len > cr->n_lat - begin)
            return fail(AF_ERR_INVALID, "the segment of scenario " + std::to_string(s) + " (" + std::to_string(begin) + " + " + std::to_string(len) + ") ends past n_lat " + std::to_string(cr->n_lat));
        if (len) segs.emplace_back(begin, len);
    }
    std::sort(segs.begin(), segs.end());
    for (size_t i = 1; i < segs.size(); ++i)
        if (segs[i].first < segs[i - 1u].first + segs[i - 1u].second)
            return fail(AF_ERR_INVALID, "two segments overlap (at element " + std::to_string(segs[i].first) + " of cells.lat)");
    std::vector<uint64_t> cell_off;
    std::vector<uint32_t> pre;
    const afc::LayoutResult lr = afc::layout_cells(cr->seg_bounds, grp, n, G, Wc, true, cell_off, pre);
    if (lr.error == afc::LayoutError::kOrder) return fail(AF_ERR_INVALID, "cells.seg_bounds of scenario " + std::to_string(lr.scenario) + " decrease");
    if (lr.error == afc::LayoutError::kCellTooLarge)
        return fail(AF_ERR_CAPACITY, "window " + std::to_string(lr.window) + " of group " + std::to_string(lr.group) + " holds 2^32 or more latencies");
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t st = e->stream;
    ScratchLayout lay;
    const size_t NE = (size_t)n * (Wc + 1u);
    const size_t o_lat = lay.part(cell_off[C] * 8u), o_bounds = lay.part(NE * 4u), o_pre = lay.part((size_t)n * Wc * 4u), o_off = lay.part((C + 1u) * 8u),
                 o_begin = lay.part((size_t)n * 8u), o_group = lay.part((size_t)n * 4u);
    WindowTiers wt;
    QuantileTiers qt;
    const QuantileOutputs qo{Q, T, cr->levels, cr->thresholds, cr->count, cr->quantiles, cr->within};
    if (cr->stats) plan_window_tiers(cell_off, C, lay, wt);
    if (want_quantiles) plan_quantile_tiers(cell_off, C, qo, lay, qt);
    if (int rc = pool_reserve(e, lay.at)) return rc;
    cr->scratch_bytes = e->pool_cap;
    unsigned char* b = e->d_pool;
    HIP_TRY(hipMemcpyAsync(b + o_bounds, cr->seg_bounds, NE * 4u, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b + o_pre, pre.data(), pre.size() * 4u, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b + o_off, cell_off.data(), cell_off.size() * 8u, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b + o_begin, cr->seg_begin, (size_t)n * 8u, hipMemcpyHostToDevice, st));
    if (!grp.empty()) HIP_TRY(hipMemcpyAsync(b + o_group, grp.data(), (size_t)n * 4u, hipMemcpyHostToDevice, st));
    afc::MergeArgs m{};
    m.src = cr->lat;
    m.begin = reinterpret_cast<const uint64_t*>(b + o_begin);
    m.bounds = reinterpret_cast<const uint32_t*>(b + o_bounds);
    m.pre = reinterpret_cast<const uint32_t*>(b + o_pre);
    m.cell_off = reinterpret_cast<const uint64_t*>(b + o_off);
    m.group = grp.empty() ? nullptr : reinterpret_cast<const uint32_t*>(b + o_group);
    m.n_win = Wc;
    m.lat = reinterpret_cast<double*>(b + o_lat);
    if (Wc <= afc::kLdsWindows)
        hipLaunchKernelGGL(afc::af_cells_merge<true>, dim3(n), dim3(afc::kThreads), (size_t)Wc * 8u + ((size_t)Wc + 1u) * 4u, st, m);
    else
        hipLaunchKernelGGL(afc::af_cells_merge<false>, dim3(n), dim3(afc::kThreads), 0, st, m);
    HIP_TRY(hipGetLastError());
    if (cr->stats) {
        afw::WinArgs a{};
        a.lat = m.lat;
        a.cell_off = m.cell_off;
        if (int rc = reduce_window_cells(e, wt, a, C, cr->stats)) return rc;
    }
    if (want_quantiles)
        if (int rc = reduce_quantile_cells(e, qt, qo, m.lat, m.cell_off, C)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    cr->elapsed_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return AF_OK;
}

// Sampled-series analyzer per (group, window of ticks) (af_series_windows.hpp).  The host reads the group ids and the counts
// back, checks them and builds the groups' member lists; one streaming pass over the sample rows, then -- unless every group
// is a single scenario -- the fold of the members' records.
// Arrivals per window and group (af_arrival_counts.hpp).  The arrival times are generated as a run generates them -- the same
// staged sweep, launch_pregen_arrivals with the same rows / groups choice, chunks by the same memory budget into the same
// e->d_arr -- or taken from the caller; per chunk one launch for the bounds of every row and one for the group sums.
static int summarize_arrivals(af_engine_t* e, const af_sweep_t* sweep, af_arrivals_t* req) {
    const uint32_t n = req->n_scenarios, W = req->n_windows, G = req->n_groups, n_draw = sweep->draw_capacity;
    const bool given = req->times && req->times_given != 0u;
    Run r;
    r.e = e;
    r.sweep = sweep;
    r.n = n;
    r.n_draw = n_draw;
    if (!given) {
        if (int rc = sweep_override_mask(sweep, true, r.mask)) return rc;
        if (int rc = check_override_columns(e, sweep)) return rc;
        r.hetero_load = (r.mask & ((1u << AF_PARAM_GEN_USERS_MEAN) | (1u << AF_PARAM_GEN_RPM_MEAN))) != 0u;
    }
    std::vector<uint32_t> grp;
    if (req->group)
        if (int rc = read_groups(req->group, n, G, grp)) return rc;
    uint32_t chunk = n;
    if (!req->times) {
        size_t mem_free = 0, mem_total = 0;
        HIP_TRY(hipMemGetInfo(&mem_free, &mem_total));
        chunk = chunk_size(e, n, (size_t)n_draw * sizeof(double), mem_free + e->arr_cap);
        if (chunk == 0) return fail(AF_ERR_CAPACITY, "draw_capacity too large for the device memory budget");
    }
    ScratchLayout lay;
    const size_t o_edges = lay.part(((size_t)W + 1u) * 8u);
    const size_t o_bounds = req->row_bounds ? 0u : lay.part((size_t)chunk * (W + 1u) * 4u);
    if (int rc = pool_reserve(e, lay.at)) return rc;
    hipStream_t st = e->stream;
    HIP_TRY(hipMemcpyAsync(e->d_pool + o_edges, req->edges, ((size_t)W + 1u) * 8u, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(req->arrivals, 0, (size_t)G * W * 8u, st));
    if (given && req->flags) HIP_TRY(hipMemsetAsync(req->flags, 0, (size_t)n * 4u, st));
    if (!given)
        if (int rc = stage_sweep(r)) return rc;
    for (uint32_t lo = 0; lo < n; lo += chunk) {
        const uint32_t nc = std::min(chunk, n - lo);
        double* rows = req->times;
        if (!rows) {
            if (int rc = reserve_device((void**)&e->d_arr, e->arr_cap, (size_t)nc * n_draw * sizeof(double))) return rc;
            rows = e->d_arr;
        }
        if (!given) {
            KArgs a = e->args;
            a.n_ovr = sweep->n_overrides;
            a.ovr_param = r.d_params;
            a.ovr_index = r.d_idxs;
            a.ovr_stride = n;
            a.ovr_values = r.d_values + lo;
            a.seeds = r.d_seeds + lo;
            a.n_draw = n_draw;
            a.n_scen = nc;
            a.scen_map = nullptr;
            a.draws = rows;
            a.pre_flags = req->flags ? req->flags + lo : nullptr;
            if (!a.pre_flags) {
                if (int rc = reserve_device((void**)&e->d_arr_flags, e->arr_flags_cap, (size_t)nc * 4u)) return rc;
                a.pre_flags = e->d_arr_flags;
            }
            if (launch_pregen_arrivals(a, nc, n_draw, !r.hetero_load, st, pregen_grouped(r, a, lo, nc)))
                return fail(AF_ERR_HIP, "af_arrival_groups: LDS attribute");
            HIP_TRY(hipGetLastError());
        }
        afac::CountArgs c{};
        c.times = rows;
        c.n_scen = nc;
        c.n_draw = n_draw;
        c.n_win = W;
        c.n_groups = G;
        c.edges = reinterpret_cast<const double*>(e->d_pool + o_edges);
        c.group = req->group ? req->group + lo : nullptr;
        c.first_group = lo;
        c.bounds = req->row_bounds ? req->row_bounds + (size_t)lo * (W + 1u) : reinterpret_cast<uint32_t*>(e->d_pool + o_bounds);
        c.generated = req->generated ? req->generated + lo : nullptr;
        c.arrivals = reinterpret_cast<unsigned long long*>(req->arrivals);
        const dim3 grid((nc + afac::kWavesPerBlock - 1u) / afac::kWavesPerBlock), block(64u * afac::kWavesPerBlock);
        if (W + 1u <= afac::kMaxLdsEdges) hipLaunchKernelGGL(afac::af_arrival_bounds<true>, grid, block, ((size_t)W + 1u) * 8u, st, c);
        else hipLaunchKernelGGL(afac::af_arrival_bounds<false>, grid, block, 0, st, c);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(afac::af_arrival_group_sums, dim3((nc + afac::kSumRows - 1u) / afac::kSumRows, (W + 255u) / 256u), dim3(256), 0, st, c);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(st));   // (the host edges are read by the copy until here)
    return AF_OK;
}

static_assert(afac::kSkip == AF_POOL_SKIP, "the kernel's skip id is the header's");

int af_engine_summarize_arrivals(af_engine_t* e, const af_sweep_t* sweep, af_arrivals_t* req) {
    if (!e || !sweep || !req) return fail(AF_ERR_INVALID, "NULL argument");
    if (e->plan_only) return fail(AF_ERR_NO_DEVICE, "planning-only engine (AF_DEVICE_PLAN_ONLY)");
    if (req->n_scenarios == 0 || req->n_windows == 0 || req->n_groups == 0)
        return fail(AF_ERR_INVALID, "empty arrivals request (n_scenarios, n_groups and n_windows must be > 0)");
    if (req->n_scenarios != sweep->n_scenarios) return fail(AF_ERR_INVALID, "arrivals.n_scenarios is not the sweep's");
    if (sweep->draw_capacity == 0) return fail(AF_ERR_INVALID, "draw_capacity must be > 0 (pass the run's value)");
    if (!req->arrivals) return fail(AF_ERR_INVALID, "arrivals.arrivals is required");
    if (!req->edges) return fail(AF_ERR_INVALID, "arrivals.edges is required");
    if (!(req->times && req->times_given) && !sweep->seeds) return fail(AF_ERR_INVALID, "empty sweep");
    if (!req->group && req->n_groups != req->n_scenarios)
        return fail(AF_ERR_INVALID, "group NULL means singletons: n_groups must be n_scenarios");
    if (int rc = check_window_edges(req->edges, req->n_windows)) return rc;
    if ((uint64_t)req->n_groups * req->n_windows >= 0xFFFFFFFFull) return fail(AF_ERR_CAPACITY, "n_groups * n_windows must be below 2^32 - 1");
    if (req->n_windows >= (1u << 24)) return fail(AF_ERR_CAPACITY, "n_windows must be below 2^24");
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(e->device));
    if (int rc = summarize_arrivals(e, sweep, req)) return rc;
    req->scratch_bytes = e->pool_cap;
    req->elapsed_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return AF_OK;
}

// Requests in flight per tick, window of ticks and group (af_inflight.hpp).  The host checks the request, reads the group ids
// and the counts back (may a cell reach 2^32 values?), uploads the edges and initialises the cells; one launch with a
// workgroup per scenario, then the min of the empty cells.
static_assert(afif::kSkip == AF_POOL_SKIP && afif::kMaxBins == AF_MAX_SERIES_HISTOGRAM_BINS, "the kernel's constants are the header's");

int af_engine_summarize_inflight(af_engine_t* e, const af_outputs_t* out, af_inflight_t* req) {
    if (!e || !out || !req) return fail(AF_ERR_INVALID, "NULL argument");
    if (e->plan_only) return fail(AF_ERR_NO_DEVICE, "planning-only engine (AF_DEVICE_PLAN_ONLY)");
    if (req->n_scenarios == 0 || req->n_groups == 0 || req->n_windows == 0)
        return fail(AF_ERR_INVALID, "empty in-flight request (n_scenarios, n_groups and n_windows must be > 0)");
    if (!req->tick_edges) return fail(AF_ERR_INVALID, "inflight.tick_edges is required");
    if (!req->count || !req->sum) return fail(AF_ERR_INVALID, "inflight.count and inflight.sum are required");
    const uint32_t n = req->n_scenarios, G = req->n_groups, W = req->n_windows, cap = out->tick_capacity, B = req->hist ? req->n_bins : 0u;
    if (req->hist && (B == 0 || B > AF_MAX_SERIES_HISTOGRAM_BINS))
        return fail(AF_ERR_INVALID, "inflight.n_bins must be 1 .. AF_MAX_SERIES_HISTOGRAM_BINS (" + std::to_string(AF_MAX_SERIES_HISTOGRAM_BINS) + ")");
    if (req->under && !req->hist) return fail(AF_ERR_INVALID, "inflight.under needs inflight.hist");
    for (uint32_t k = 1; k <= W; ++k)
        if (!(req->tick_edges[k - 1] < req->tick_edges[k]))
            return fail(AF_ERR_INVALID, "tick_edges must be strictly increasing (edge " + std::to_string(k) + ")");
    if (!(std::isfinite(req->sample_period) && req->sample_period > 0.0)) return fail(AF_ERR_INVALID, "inflight.sample_period must be a finite number above 0");
    if (!out->counts) return fail(AF_ERR_INVALID, "outputs.counts is required");
    if (!out->clock || out->clock_capacity == 0) return fail(AF_ERR_INVALID, "requests in flight need outputs.clock");
    if (cap == 0) return fail(AF_ERR_INVALID, "requests in flight need outputs.tick_capacity > 0");
    if ((uint64_t)G * W >= 0xFFFFFFFFull) return fail(AF_ERR_CAPACITY, "n_groups * n_windows must be below 2^32 - 1");
    if (cap >= 0x80000000u) return fail(AF_ERR_CAPACITY, "tick_capacity must be below 2^31");
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(e->device));
    std::vector<uint32_t> counts((size_t)n * AF_CNT_SLOTS), grp;
    HIP_TRY(hipMemcpy(counts.data(), out->counts, counts.size() * 4u, hipMemcpyDeviceToHost));
    if (int rc = read_groups(req->group, n, G, grp)) return rc;
    {   // may a cell reach 2^32 values?
        std::vector<uint64_t> g_ticks(G, 0u);
        bool big = false;
        for (uint32_t s = 0; s < n; ++s) {
            const uint32_t g = grp.empty() ? 0u : grp[s];
            if (g == afif::kSkip) continue;
            g_ticks[g] += std::min(counts[(size_t)s * AF_CNT_SLOTS + AF_CNT_TICKS], cap);
            big = big || g_ticks[g] > 0xFFFFFFFFull;
        }
        if (big) {   // (else no window of a group can hold 2^32 rows)
            std::vector<uint64_t> cells((size_t)G * W, 0u);
            for (uint32_t s = 0; s < n; ++s) {
                const uint32_t g = grp.empty() ? 0u : grp[s];
                if (g == afif::kSkip || g_ticks[g] <= 0xFFFFFFFFull) continue;
                const uint32_t m = std::min(counts[(size_t)s * AF_CNT_SLOTS + AF_CNT_TICKS], cap);
                for (uint32_t w = 0; w < W && req->tick_edges[w] < m; ++w) {
                    uint64_t& c = cells[(size_t)g * W + w];
                    c += std::min(req->tick_edges[w + 1u], m) - req->tick_edges[w];
                    if (c > 0xFFFFFFFFull) return fail(AF_ERR_CAPACITY, "window " + std::to_string(w) + " of group " + std::to_string(g) + " holds 2^32 or more values");
                }
            }
        }
    }
    ScratchLayout lay;
    const size_t o_edges = lay.part(((size_t)W + 1u) * 4u);
    if (int rc = pool_reserve(e, lay.at)) return rc;
    hipStream_t st = e->stream;
    HIP_TRY(hipMemcpyAsync(e->d_pool + o_edges, req->tick_edges, ((size_t)W + 1u) * 4u, hipMemcpyHostToDevice, st));
    const size_t cells = (size_t)G * W;
    HIP_TRY(hipMemsetAsync(req->count, 0, cells * 4u, st));
    HIP_TRY(hipMemsetAsync(req->sum, 0, cells * 8u, st));
    if (req->minv) HIP_TRY(hipMemsetAsync(req->minv, 0xFF, cells * 4u, st));
    if (req->maxv) HIP_TRY(hipMemsetAsync(req->maxv, 0, cells * 4u, st));
    if (req->above) HIP_TRY(hipMemsetAsync(req->above, 0, cells * 4u, st));
    if (req->hist) HIP_TRY(hipMemsetAsync(req->hist, 0, cells * B * 4u, st));
    if (req->under) HIP_TRY(hipMemsetAsync(req->under, 0, cells * 4u, st));
    afif::IfArgs a{};
    a.clock = out->clock;
    a.counts = out->counts;
    a.clock_cap = out->clock_capacity;
    a.tick_cap = cap;
    a.cnt_completed_slot = AF_CNT_COMPLETED;
    a.cnt_ticks_slot = AF_CNT_TICKS;
    a.period = req->sample_period;
    a.group = req->group;
    a.n_win = W;
    a.edges = reinterpret_cast<const uint32_t*>(e->d_pool + o_edges);
    a.threshold = req->threshold;
    a.n_bins = B;
    a.lo = req->lo;
    a.count = req->count;
    a.sum = reinterpret_cast<unsigned long long*>(req->sum);
    a.minv = req->minv;
    a.maxv = req->maxv;
    a.above = req->above;
    a.hist = req->hist;
    a.under = req->under;
    a.in_flight = req->in_flight;
    a.started = req->started;
    a.finished = req->finished;
    const bool both = req->started || req->finished;
    const size_t lds = (size_t)afif::kChunkTicks * (both ? 8u : 4u);
    const void* fn = both ? reinterpret_cast<const void*>(afif::af_inflight_kernel<WaveHip, true>)
                          : reinterpret_cast<const void*>(afif::af_inflight_kernel<WaveHip, false>);
    // (set before every launch: the attribute is per device and engines of several devices run in threads of one process)
    if (lds > 48u * 1024u) HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    void* kargs[] = {&a};
    HIP_TRY(hipLaunchKernel(fn, dim3(n), dim3(afif::kThreads), kargs, lds, st));
    if (req->minv) {
        hipLaunchKernelGGL(afif::af_inflight_finish, dim3((uint32_t)((cells + 255u) / 256u)), dim3(256), 0, st, req->count, req->minv, (uint32_t)cells);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(st));   // (the host edges are read by the copy until here)
    req->scratch_bytes = e->pool_cap;
    req->elapsed_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return AF_OK;
}

// Burn-rate alert rules per tick over rolling look-backs of the completions (af_alerts.hpp).  The host checks the request, reads
// the group ids back, uploads the edges and the rules and initialises the group cells; two launches: the prefix arrays by a
// workgroup per scenario, the evaluation by a wave per scenario.
static_assert(afal::kSkip == AF_POOL_SKIP && afal::kNone == AF_TICK_NONE && afal::kMaxRules == AF_MAX_ALERT_RULES &&
                  afal::kMaxBins == AF_MAX_SERIES_HISTOGRAM_BINS && sizeof(afal::Rule) == sizeof(af_alert_rule_t),
              "the kernel's constants are the header's");

// What both alert calls refuse before anything is touched.
static int alerts_check(const af_outputs_t* out, const af_alerts_t* req) {
    if (req->n_scenarios == 0 || req->n_groups == 0 || req->n_windows == 0 || req->n_rules == 0)
        return fail(AF_ERR_INVALID, "empty alerts request (n_scenarios, n_groups, n_windows and n_rules must be > 0)");
    if (req->n_rules > AF_MAX_ALERT_RULES) return fail(AF_ERR_INVALID, "alerts.n_rules must be 1 .. AF_MAX_ALERT_RULES (" + std::to_string(AF_MAX_ALERT_RULES) + ")");
    if (!req->tick_edges) return fail(AF_ERR_INVALID, "alerts.tick_edges is required");
    if (!req->rules) return fail(AF_ERR_INVALID, "alerts.rules is required");
    const uint32_t n = req->n_scenarios, G = req->n_groups, W = req->n_windows, R = req->n_rules, cap = out->tick_capacity;
    const uint32_t B = req->delay_hist ? req->n_bins : 0u;
    if (req->delay_hist && (B == 0 || B > AF_MAX_SERIES_HISTOGRAM_BINS))
        return fail(AF_ERR_INVALID, "alerts.n_bins must be 1 .. AF_MAX_SERIES_HISTOGRAM_BINS (" + std::to_string(AF_MAX_SERIES_HISTOGRAM_BINS) + ")");
    if (req->delay_hist && req->delay_width == 0) return fail(AF_ERR_INVALID, "alerts.delay_width must be above 0");
    for (uint32_t k = 1; k <= W; ++k)
        if (!(req->tick_edges[k - 1] < req->tick_edges[k]))
            return fail(AF_ERR_INVALID, "tick_edges must be strictly increasing (edge " + std::to_string(k) + ")");
    if (!(std::isfinite(req->sample_period) && req->sample_period > 0.0)) return fail(AF_ERR_INVALID, "alerts.sample_period must be a finite number above 0");
    if (std::isnan(req->slo)) return fail(AF_ERR_INVALID, "alerts.slo must not be NaN");
    for (uint32_t r = 0; r < R; ++r) {
        const af_alert_rule_t& ru = req->rules[r];
        if (ru.short_ticks == 0 || ru.long_ticks < ru.short_ticks || ru.den == 0 || ru.num > ru.den || ru.hold_ticks == 0)
            return fail(AF_ERR_INVALID, "alerts.rules[" + std::to_string(r) + "]: long_ticks >= short_ticks >= 1, den >= 1, num <= den and hold_ticks >= 1 must hold");
    }
    if (!out->counts) return fail(AF_ERR_INVALID, "outputs.counts is required");
    if (!out->clock || out->clock_capacity == 0) return fail(AF_ERR_INVALID, "alerts need outputs.clock");
    if (cap == 0) return fail(AF_ERR_INVALID, "alerts need outputs.tick_capacity > 0");
    if ((uint64_t)G * W >= 0xFFFFFFFFull || (uint64_t)G * W * R >= 0xFFFFFFFFull) return fail(AF_ERR_CAPACITY, "n_groups * n_windows * n_rules must be below 2^32 - 1");
    if ((uint64_t)n * W >= 0xFFFFFFFFull || (uint64_t)n * W * R >= 0xFFFFFFFFull) return fail(AF_ERR_CAPACITY, "n_scenarios * n_windows * n_rules must be below 2^32 - 1");
    if (cap >= 0x80000000u) return fail(AF_ERR_CAPACITY, "tick_capacity must be below 2^31");
    return AF_OK;
}

// The checked request on the device: the group ids read back, the edges and the rules uploaded, the group cells initialised, the
// prefix arrays by a workgroup per scenario -- from the completions (oc NULL) or from the outcomes --, then the evaluation.
static int alerts_run(af_engine_t* e, const af_outputs_t* out, af_alerts_t* req, const af_alert_outcomes_t* oc) {
    const uint32_t n = req->n_scenarios, G = req->n_groups, W = req->n_windows, R = req->n_rules, cap = out->tick_capacity;
    const uint32_t B = req->delay_hist ? req->n_bins : 0u;
    std::vector<uint32_t> grp;
    if (int rc = read_groups(req->group, n, G, grp)) return rc;
    ScratchLayout lay;
    const size_t o_edges = lay.part(((size_t)W + 1u) * 4u);
    const size_t o_rules = lay.part((size_t)R * sizeof(afal::Rule));
    const size_t o_prefix = lay.part((size_t)n * cap * 8u);
    if (int rc = pool_reserve(e, lay.at)) return rc;
    hipStream_t st = e->stream;
    HIP_TRY(hipMemcpyAsync(e->d_pool + o_edges, req->tick_edges, ((size_t)W + 1u) * 4u, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(e->d_pool + o_rules, req->rules, (size_t)R * sizeof(afal::Rule), hipMemcpyHostToDevice, st));
    const size_t cells = (size_t)G * W * R;
    if (req->members) HIP_TRY(hipMemsetAsync(req->members, 0, cells * 4u, st));
    if (req->fired_members) HIP_TRY(hipMemsetAsync(req->fired_members, 0, cells * 4u, st));
    if (req->open_members) HIP_TRY(hipMemsetAsync(req->open_members, 0, cells * 4u, st));
    if (req->fire_ticks) HIP_TRY(hipMemsetAsync(req->fire_ticks, 0, cells * 8u, st));
    if (req->fire_episodes) HIP_TRY(hipMemsetAsync(req->fire_episodes, 0, cells * 8u, st));
    if (req->delay_hist) HIP_TRY(hipMemsetAsync(req->delay_hist, 0, cells * B * 4u, st));
    afal::AlArgs a{};
    a.clock = out->clock;
    a.counts = out->counts;
    a.clock_cap = out->clock_capacity;
    a.tick_cap = cap;
    a.cnt_completed_slot = AF_CNT_COMPLETED;
    a.cnt_ticks_slot = AF_CNT_TICKS;
    a.period = req->sample_period;
    a.slo = req->slo;
    a.n_scen = n;
    a.n_win = W;
    a.n_rules = R;
    a.n_bins = B;
    a.delay_width = req->delay_width;
    a.group = req->group;
    a.edges = reinterpret_cast<const uint32_t*>(e->d_pool + o_edges);
    a.rules = reinterpret_cast<const afal::Rule*>(e->d_pool + o_rules);
    a.prefix = reinterpret_cast<uint2*>(e->d_pool + o_prefix);
    a.total = req->total;
    a.bad = req->bad;
    a.firing = req->firing;
    a.count = req->count;
    a.fired = req->fired;
    a.episodes = req->episodes;
    a.longest = req->longest;
    a.longest_start = req->longest_start;
    a.first = req->first;
    a.last = req->last;
    a.members = req->members;
    a.fired_members = req->fired_members;
    a.open_members = req->open_members;
    a.fire_ticks = reinterpret_cast<unsigned long long*>(req->fire_ticks);
    a.fire_episodes = reinterpret_cast<unsigned long long*>(req->fire_episodes);
    a.delay_hist = req->delay_hist;
    // (the attribute is set before every launch: it is per device and engines of several devices run in threads of one process)
    if (oc) {
        afao::OcArgs o{};
        o.al = a;
        o.times = oc->times;
        o.time_row = oc->time_row;
        o.draw_cap = oc->draw_capacity;
        o.tau = oc->timeout;
        o.timeouts = oc->timeouts;
        o.timed_out = oc->timed_out;
        o.deficit = oc->deficit;
        o.flags = oc->flags;
        const size_t lds = (size_t)afao::kChunkTicks * 12u;
        const void* fn = reinterpret_cast<const void*>(afao::af_alert_outcomes_prefix_kernel<WaveHip>);
        HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        void* kargs[] = {&o};
        HIP_TRY(hipLaunchKernel(fn, dim3(n), dim3(afao::kThreads), kargs, lds, st));
    } else {
        const size_t lds = (size_t)afal::kChunkTicks * 8u;
        const void* fn = reinterpret_cast<const void*>(afal::af_alerts_prefix_kernel<WaveHip>);
        HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        void* kargs[] = {&a};
        HIP_TRY(hipLaunchKernel(fn, dim3(n), dim3(afal::kThreads), kargs, lds, st));
    }
    hipLaunchKernelGGL(afal::af_alerts_eval_kernel, dim3((n + afal::kEvalWaves - 1u) / afal::kEvalWaves), dim3(afal::kEvalThreads), 0, st, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));   // (the host edges and rules are read by the copies until here)
    req->scratch_bytes = e->pool_cap;
    return AF_OK;
}

int af_engine_summarize_alerts(af_engine_t* e, const af_outputs_t* out, af_alerts_t* req) {
    if (!e || !out || !req) return fail(AF_ERR_INVALID, "NULL argument");
    if (e->plan_only) return fail(AF_ERR_NO_DEVICE, "planning-only engine (AF_DEVICE_PLAN_ONLY)");
    if (int rc = alerts_check(out, req)) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(e->device));
    if (int rc = alerts_run(e, out, req, nullptr)) return rc;
    req->elapsed_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return AF_OK;
}

// Alert rules on request outcomes (af_alert_outcomes.hpp): af_engine_summarize_alerts's request and evaluation; the prefix arrays
// come from the completions in time and the timeouts of the arrival rows.  The row ids are read back and checked on the host.
static_assert(afao::kRowsTruncated == AF_OUTCOME_ROWS_TRUNCATED && afao::kDeficit == AF_OUTCOME_DEFICIT, "the kernel's flags are the header's");

int af_engine_outcome_alerts(af_engine_t* e, const af_outputs_t* out, af_alert_outcomes_t* oc, af_alerts_t* req) {
    if (!e || !out || !oc || !req) return fail(AF_ERR_INVALID, "NULL argument");
    if (e->plan_only) return fail(AF_ERR_NO_DEVICE, "planning-only engine (AF_DEVICE_PLAN_ONLY)");
    if (int rc = alerts_check(out, req)) return rc;
    if (!oc->times) return fail(AF_ERR_INVALID, "alert_outcomes.times is required");
    if (oc->draw_capacity == 0) return fail(AF_ERR_INVALID, "alert_outcomes.draw_capacity must be > 0 (pass the run's value)");
    if (oc->n_time_rows == 0) return fail(AF_ERR_INVALID, "alert_outcomes.n_time_rows must be > 0");
    if (!oc->time_row && oc->n_time_rows != req->n_scenarios)
        return fail(AF_ERR_INVALID, "time_row NULL means scenario s reads row s: n_time_rows must be n_scenarios");
    if (!(std::isfinite(oc->timeout) && oc->timeout > 0.0)) return fail(AF_ERR_INVALID, "alert_outcomes.timeout must be a finite number above 0");
    if (oc->draw_capacity >= 0x80000000u) return fail(AF_ERR_CAPACITY, "draw_capacity must be below 2^31");
    if (out->clock_capacity >= 0x80000000u) return fail(AF_ERR_CAPACITY, "clock_capacity must be below 2^31 (a tick's arrivals minus its rows is an i32)");
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(e->device));
    if (oc->time_row) {
        std::vector<uint32_t> ids(req->n_scenarios);
        HIP_TRY(hipMemcpy(ids.data(), oc->time_row, ids.size() * 4u, hipMemcpyDeviceToHost));
        for (uint32_t s = 0; s < req->n_scenarios; ++s)
            if (ids[s] >= oc->n_time_rows)
                return fail(AF_ERR_INVALID, "alert_outcomes.time_row out of range (scenario " + std::to_string(s) + ": " + std::to_string(ids[s]) + ", limit " + std::to_string(oc->n_time_rows) + ")");
    }
    if (int rc = alerts_run(e, out, req, oc)) return rc;
    req->elapsed_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return AF_OK;
}

// The k slowest requests per window and group with their identity (af_exemplars.hpp).  The host checks the request, reads the
// group ids back and lists each group's members in ascending scenario index; three launches: the per-(scenario, window) lists by a
// wave per scenario, the cells by a wave per cell, the optional state gather.
static_assert(afex::kSkip == AF_POOL_SKIP && afex::kMaxK == AF_MAX_EXEMPLARS, "the kernel's constants are the header's");

int af_engine_summarize_exemplars(af_engine_t* e, const af_outputs_t* out, af_exemplars_t* req) {
    if (!e || !out || !req) return fail(AF_ERR_INVALID, "NULL argument");
    if (e->plan_only) return fail(AF_ERR_NO_DEVICE, "planning-only engine (AF_DEVICE_PLAN_ONLY)");
    if (req->n_scenarios == 0 || req->n_groups == 0) return fail(AF_ERR_INVALID, "empty exemplars request (n_scenarios and n_groups must be > 0)");
    if (req->k == 0 || req->k > AF_MAX_EXEMPLARS) return fail(AF_ERR_INVALID, "exemplars.k must be 1 .. AF_MAX_EXEMPLARS (" + std::to_string(AF_MAX_EXEMPLARS) + ")");
    const uint32_t n = req->n_scenarios, G = req->n_groups, W = req->n_windows, K = req->k;
    if (W > 0 && !req->edges) return fail(AF_ERR_INVALID, "exemplars.edges is required with n_windows > 0");
    if (W == 0 && req->edges) return fail(AF_ERR_INVALID, "exemplars.edges must be NULL with n_windows == 0");
    if (W == 0 && req->by_arrival) return fail(AF_ERR_INVALID, "windows by arrival time need n_windows > 0");
    if (W > 0)
        if (int rc = check_window_edges(req->edges, W)) return rc;
    if (!req->total || !req->scenario || !req->row || !req->clock) return fail(AF_ERR_INVALID, "exemplars.total, scenario, row and clock are required");
    if (reinterpret_cast<uintptr_t>(req->clock) % 16u) return fail(AF_ERR_INVALID, "exemplars.clock must be 16-byte aligned");
    if (!out->counts) return fail(AF_ERR_INVALID, "outputs.counts is required");
    if (!out->clock || out->clock_capacity == 0) return fail(AF_ERR_INVALID, "the slowest requests need outputs.clock");
    const uint32_t S = e->args.n_edges + 3u * e->args.n_servers, pitch = e->args.series_pitch;
    if (req->state) {
        if (S == 0 || pitch < S) return fail(AF_ERR_INVALID, "the plan has no sampled series");
        if (!out->samples || out->tick_capacity == 0) return fail(AF_ERR_INVALID, "exemplars.state needs outputs.samples");
        if (!(std::isfinite(req->sample_period) && req->sample_period > 0.0)) return fail(AF_ERR_INVALID, "exemplars.sample_period must be a finite number above 0");
    }
    const uint64_t wins = W ? W : 1u;
    if ((uint64_t)G * wins >= 0x100000000ull || (uint64_t)G * wins * K >= 0x100000000ull) return fail(AF_ERR_CAPACITY, "n_groups * max(n_windows, 1) * k must be below 2^32");
    if ((uint64_t)n * wins >= 0x100000000ull || (uint64_t)n * wins * K >= 0x100000000ull) return fail(AF_ERR_CAPACITY, "n_scenarios * max(n_windows, 1) * k must be below 2^32");
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(e->device));
    std::vector<uint32_t> grp;
    if (int rc = read_groups(req->group, n, G, grp)) return rc;
    std::vector<uint32_t> g_off((size_t)G + 1u, 0u), members;   // a counting sort: ascending scenario index within a group
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t g = grp.empty() ? 0u : grp[s];
        if (g != afex::kSkip) g_off[(size_t)g + 1u] += 1u;
    }
    for (uint32_t g = 0; g < G; ++g) g_off[(size_t)g + 1u] += g_off[g];
    members.resize(std::max<size_t>(g_off[G], 1u));
    {
        std::vector<uint32_t> next(g_off.begin(), g_off.end() - 1);
        for (uint32_t s = 0; s < n; ++s) {
            const uint32_t g = grp.empty() ? 0u : grp[s];
            if (g != afex::kSkip) members[next[g]++] = s;
        }
    }
    const bool lds = wins <= afex::kLdsExemplarWindows;
    const size_t NW = (size_t)n * wins, cells = (size_t)G * wins;
    ScratchLayout lay;
    const size_t o_edges = lay.part(((size_t)W + 1u) * 8u);
    const size_t o_members = lay.part(members.size() * 4u);
    const size_t o_goff = lay.part(g_off.size() * 4u);
    const size_t o_cnt = lay.part(NW * 4u);
    const size_t o_thr = lay.part(lds ? 0u : NW * 8u);
    const size_t o_lrow = lay.part(NW * K * 4u);
    const size_t o_lkey = lay.part(NW * K * 8u);
    if (int rc = pool_reserve(e, lay.at)) return rc;
    hipStream_t st = e->stream;
    unsigned char* b = e->d_pool;
    if (W) HIP_TRY(hipMemcpyAsync(b + o_edges, req->edges, ((size_t)W + 1u) * 8u, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b + o_members, members.data(), members.size() * 4u, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b + o_goff, g_off.data(), g_off.size() * 4u, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(b + o_cnt, 0, NW * 4u, st));   // (a skipped scenario writes none of its counts)
    if (!lds) HIP_TRY(hipMemsetAsync(b + o_thr, 0, NW * 8u, st));
    afex::ExArgs a{};
    a.clock = out->clock;
    a.counts = out->counts;
    a.clock_cap = out->clock_capacity;
    a.cnt_completed_slot = AF_CNT_COMPLETED;
    a.group = req->group;
    a.n_win = W;
    a.wins = (uint32_t)wins;
    a.edges = reinterpret_cast<const double*>(b + o_edges);
    a.by_arrival = req->by_arrival ? 1u : 0u;
    a.k = K;
    a.lkey = reinterpret_cast<unsigned long long*>(b + o_lkey);
    a.lrow = reinterpret_cast<uint32_t*>(b + o_lrow);
    a.cnt = reinterpret_cast<uint32_t*>(b + o_cnt);
    a.thr = lds ? nullptr : reinterpret_cast<unsigned long long*>(b + o_thr);
    a.members = reinterpret_cast<const uint32_t*>(b + o_members);
    a.g_off = reinterpret_cast<const uint32_t*>(b + o_goff);
    a.cells = cells;
    a.total = reinterpret_cast<unsigned long long*>(req->total);
    a.kept = req->kept;
    a.scenario = req->scenario;
    a.row = req->row;
    a.pair = req->clock;
    a.samples = out->samples;
    a.tick_cap = out->tick_capacity;
    a.pitch = pitch;
    a.n_series = S;
    a.cnt_ticks_slot = AF_CNT_TICKS;
    a.period = req->sample_period;
    a.state = req->state;
    if (lds)
        hipLaunchKernelGGL(afex::af_exemplar_lists<true>, dim3(n), dim3(64), (W ? ((size_t)W + 1u) * 8u : 0u) + (size_t)wins * 12u, st, a);
    else
        hipLaunchKernelGGL(afex::af_exemplar_lists<false>, dim3(n), dim3(64), 0, st, a);
    HIP_TRY(hipGetLastError());
    if (int rc = launch_tiny_tier(cells, afex::kCellWaves, [&](uint32_t blocks, uint64_t c0) {
            hipLaunchKernelGGL(afex::af_exemplar_cells, dim3(blocks), dim3(64u * afex::kCellWaves), 0, st, a, c0);
        }))
        return rc;
    if (req->state) {
        const uint64_t words = (uint64_t)cells * K * S;
        hipLaunchKernelGGL(afex::af_exemplar_state, dim3((uint32_t)std::min<uint64_t>((words + 255u) / 256u, kBlocksPerLaunch)), dim3(256), 0, st, a, words);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(st));   // (the host edges and lists are read by the copies until here)
    req->scratch_bytes = e->pool_cap;
    req->elapsed_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return AF_OK;
}

// Log-linear latency histograms per window and group (af_latency_histogram.hpp).  The host checks the request, reads the group
// ids and the counts back (may a group hold 2^32 rows?), uploads the edges and zeroes the outputs; one launch.
static_assert(aflh::kSkip == AF_POOL_SKIP && aflh::kMaxBins == AF_MAX_LATENCY_HISTOGRAM_BINS, "the kernel's constants are the header's");

int af_engine_summarize_latency_histogram(af_engine_t* e, const af_outputs_t* out, af_latency_histogram_t* req) {
    if (!e || !out || !req) return fail(AF_ERR_INVALID, "NULL argument");
    if (e->plan_only) return fail(AF_ERR_NO_DEVICE, "planning-only engine (AF_DEVICE_PLAN_ONLY)");
    if (req->n_scenarios == 0 || req->n_groups == 0) return fail(AF_ERR_INVALID, "empty latency histogram request (n_scenarios and n_groups must be > 0)");
    aflh::Binning bin{};
    if (!aflh::make_binning(req->sub_bits, req->min_exp, req->octaves, bin))
        return fail(AF_ERR_INVALID, "latency_histogram binning: sub_bits 0 .. 8, min_exp >= -1022, octaves >= 1, min_exp + octaves <= 1023 and octaves << sub_bits <= AF_MAX_LATENCY_HISTOGRAM_BINS (" + std::to_string(AF_MAX_LATENCY_HISTOGRAM_BINS) + ")");
    const uint32_t n = req->n_scenarios, G = req->n_groups, W = req->n_windows, B = bin.n_bins;
    if (W > 0 && !req->edges) return fail(AF_ERR_INVALID, "latency_histogram.edges is required with n_windows > 0");
    if (W == 0 && req->edges) return fail(AF_ERR_INVALID, "latency_histogram.edges must be NULL with n_windows == 0");
    if (W == 0 && req->by_arrival) return fail(AF_ERR_INVALID, "windows by arrival time need n_windows > 0");
    if (W > 0)
        if (int rc = check_window_edges(req->edges, W)) return rc;
    if (!req->count || !req->hist) return fail(AF_ERR_INVALID, "latency_histogram.count and latency_histogram.hist are required");
    if (!out->counts) return fail(AF_ERR_INVALID, "outputs.counts is required");
    if (!out->clock || out->clock_capacity == 0) return fail(AF_ERR_INVALID, "latency histograms need outputs.clock");
    if (reinterpret_cast<uintptr_t>(out->clock) % 16u) return fail(AF_ERR_INVALID, "outputs.clock must be 16-byte aligned");
    const uint64_t wins = W ? W : 1u;
    if ((uint64_t)G * wins >= 0x100000000ull || (uint64_t)G * wins * B >= 0x100000000ull)
        return fail(AF_ERR_CAPACITY, "n_groups * max(n_windows, 1) * n_bins must be below 2^32");
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(e->device));
    std::vector<uint32_t> grp;
    if (int rc = read_groups(req->group, n, G, grp)) return rc;
    {   // may a counter reach 2^32?  Not while no group holds that many stored rows (af_engine_summarize_pooled's rule)
        std::vector<uint32_t> counts((size_t)n * AF_CNT_SLOTS);
        HIP_TRY(hipMemcpy(counts.data(), out->counts, counts.size() * 4u, hipMemcpyDeviceToHost));
        std::vector<uint64_t> g_rows(G, 0u);
        for (uint32_t s = 0; s < n; ++s) {
            const uint32_t g = grp.empty() ? 0u : grp[s];
            if (g == aflh::kSkip) continue;
            g_rows[g] += std::min(counts[(size_t)s * AF_CNT_SLOTS + AF_CNT_COMPLETED], out->clock_capacity);
            if (g_rows[g] > 0xFFFFFFFFull) return fail(AF_ERR_CAPACITY, "group " + std::to_string(g) + " holds 2^32 or more latencies");
        }
    }
    ScratchLayout lay;
    const size_t o_edges = lay.part(((size_t)W + 1u) * 8u);
    if (int rc = pool_reserve(e, lay.at)) return rc;
    hipStream_t st = e->stream;
    if (W) HIP_TRY(hipMemcpyAsync(e->d_pool + o_edges, req->edges, ((size_t)W + 1u) * 8u, hipMemcpyHostToDevice, st));
    const size_t cells = (size_t)G * wins;
    HIP_TRY(hipMemsetAsync(req->count, 0, cells * 8u, st));
    HIP_TRY(hipMemsetAsync(req->hist, 0, cells * B * 4u, st));
    if (req->under) HIP_TRY(hipMemsetAsync(req->under, 0, cells * 4u, st));
    if (req->over) HIP_TRY(hipMemsetAsync(req->over, 0, cells * 4u, st));
    if (req->nan) HIP_TRY(hipMemsetAsync(req->nan, 0, cells * 4u, st));
    aflh::LhArgs a{};
    a.clock = out->clock;
    a.counts = out->counts;
    a.clock_cap = out->clock_capacity;
    a.cnt_completed_slot = AF_CNT_COMPLETED;
    a.group = req->group;
    a.n_scen = n;
    a.n_win = W;
    a.wins = (uint32_t)wins;
    a.edges = reinterpret_cast<const double*>(e->d_pool + o_edges);
    a.by_arrival = req->by_arrival ? 1u : 0u;
    a.chunks = (uint32_t)(((uint64_t)out->clock_capacity + aflh::kChunkRows - 1u) / aflh::kChunkRows);
    a.bin = bin;
    a.count = reinterpret_cast<unsigned long long*>(req->count);
    a.hist = req->hist;
    a.under = req->under;
    a.over = req->over;
    a.nan = req->nan;
    const bool in_lds = W <= aflh::kLdsHistogramWindows;
    const size_t lds = (in_lds && W ? ((size_t)W + 1u) * 8u : 0u) + (size_t)aflh::kWaves * B * 4u;
    const void* fn = in_lds ? reinterpret_cast<const void*>(aflh::af_latency_histogram_kernel<true>)
                            : reinterpret_cast<const void*>(aflh::af_latency_histogram_kernel<false>);
    // (set before every launch: the attribute is per device and engines of several devices run in threads of one process)
    if (lds > 48u * 1024u) HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const uint64_t items = (uint64_t)n * a.chunks;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((items + aflh::kWaves - 1u) / aflh::kWaves, aflh::kMaxBlocks);
    void* kargs[] = {&a};
    HIP_TRY(hipLaunchKernel(fn, dim3(blocks), dim3(aflh::kThreads), kargs, lds, st));
    HIP_TRY(hipStreamSynchronize(st));   // (the host edges are read by the copy until here)
    req->scratch_bytes = e->pool_cap;
    req->elapsed_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return AF_OK;
}

// Paired latency differences under common seeds (af_paired.hpp).  The host checks the request, reads the pair, row and group ids
// and the counts back (is every id in range?  may a counter reach 2^32?), uploads edges and thresholds and initialises the
// outputs; then per chunk of pairs the slots are filled with 0xFF, the match pass writes them and the reduce pass reads them.
static_assert(afpr::kSkip == AF_POOL_SKIP && afpr::kNone == AF_PAIR_NONE && afpr::kMaxThresholds == AF_MAX_PAIR_THRESHOLDS, "the kernel's constants are the header's");

int af_engine_summarize_pairs(af_engine_t* e, const af_outputs_t* out, af_pairs_t* req) {
    if (!e || !out || !req) return fail(AF_ERR_INVALID, "NULL argument");
    if (e->plan_only) return fail(AF_ERR_NO_DEVICE, "planning-only engine (AF_DEVICE_PLAN_ONLY)");
    if (req->n_pairs == 0 || req->n_groups == 0 || req->n_scenarios == 0 || req->n_time_rows == 0)
        return fail(AF_ERR_INVALID, "empty pairs request (n_pairs, n_groups, n_scenarios and n_time_rows must be > 0)");
    if (req->draw_capacity == 0) return fail(AF_ERR_INVALID, "pairs.draw_capacity must be > 0 (pass the run's value)");
    aflh::Binning bin{};
    if (!aflh::make_binning(req->sub_bits, req->min_exp, req->octaves, bin))
        return fail(AF_ERR_INVALID, "pairs binning: sub_bits 0 .. 8, min_exp >= -1022, octaves >= 1, min_exp + octaves <= 1023 and octaves << sub_bits <= AF_MAX_LATENCY_HISTOGRAM_BINS (" + std::to_string(AF_MAX_LATENCY_HISTOGRAM_BINS) + ")");
    const uint32_t P = req->n_pairs, G = req->n_groups, W = req->n_windows, B = bin.n_bins, T = req->n_thresholds, n_draw = req->draw_capacity;
    if (W > 0 && !req->edges) return fail(AF_ERR_INVALID, "pairs.edges is required with n_windows > 0");
    if (W == 0 && req->edges) return fail(AF_ERR_INVALID, "pairs.edges must be NULL with n_windows == 0");
    if (W > 0)
        if (int rc = check_window_edges(req->edges, W)) return rc;
    if (T > AF_MAX_PAIR_THRESHOLDS) return fail(AF_ERR_INVALID, "pairs.n_thresholds must be at most AF_MAX_PAIR_THRESHOLDS (" + std::to_string(AF_MAX_PAIR_THRESHOLDS) + ")");
    if (T > 0 && (!req->thresholds || !req->above)) return fail(AF_ERR_INVALID, "pairs.thresholds and pairs.above are required with n_thresholds > 0");
    for (uint32_t t = 0; t < T; ++t)
        if (!std::isfinite(req->thresholds[t])) return fail(AF_ERR_INVALID, "pairs threshold " + std::to_string(t) + " is not finite");
    if (!req->pair_a || !req->pair_b || !req->time_row || !req->times) return fail(AF_ERR_INVALID, "pairs.pair_a, pair_b, time_row and times are required");
    if (!req->pair_counts || !req->pair_sums || !req->unmatched || !req->cell_counts || !req->extremes || !req->hist || !req->tails)
        return fail(AF_ERR_INVALID, "pairs.pair_counts, pair_sums, unmatched, cell_counts, extremes, hist and tails are required");
    if (!out->counts) return fail(AF_ERR_INVALID, "outputs.counts is required");
    if (!out->clock || out->clock_capacity == 0) return fail(AF_ERR_INVALID, "paired differences need outputs.clock");
    if (reinterpret_cast<uintptr_t>(out->clock) % 16u) return fail(AF_ERR_INVALID, "outputs.clock must be 16-byte aligned");
    const uint64_t wins = W ? W : 1u;
    if ((uint64_t)P * wins >= 0x100000000ull) return fail(AF_ERR_CAPACITY, "n_pairs * max(n_windows, 1) must be below 2^32");
    if ((uint64_t)G * wins >= 0x100000000ull || (uint64_t)G * wins * B >= 0x100000000ull)
        return fail(AF_ERR_CAPACITY, "n_groups * max(n_windows, 1) * n_bins must be below 2^32");
    if (n_draw >= 0x80000000u) return fail(AF_ERR_CAPACITY, "draw_capacity must be below 2^31");
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(e->device));
    const uint32_t n = req->n_scenarios;
    std::vector<uint32_t> ids[3];   // pair_a, pair_b, time_row
    const uint32_t* src[3] = {req->pair_a, req->pair_b, req->time_row};
    const char* names[3] = {"pair_a", "pair_b", "time_row"};
    for (int k = 0; k < 3; ++k) {
        ids[k].resize(P);
        HIP_TRY(hipMemcpy(ids[k].data(), src[k], (size_t)P * 4u, hipMemcpyDeviceToHost));
        const uint32_t limit = k < 2 ? n : req->n_time_rows;
        for (uint32_t p = 0; p < P; ++p)
            if (ids[k][p] >= limit)
                return fail(AF_ERR_INVALID, std::string("pairs.") + names[k] + " out of range (pair " + std::to_string(p) + ": " + std::to_string(ids[k][p]) + ", limit " + std::to_string(limit) + ")");
    }
    std::vector<uint32_t> grp;
    if (int rc = read_groups(req->group, P, G, grp)) return rc;
    {   // may a u32 counter of a cell reach 2^32?  Not while the pairs of no group can match that many requests
        std::vector<uint32_t> counts((size_t)n * AF_CNT_SLOTS);
        HIP_TRY(hipMemcpy(counts.data(), out->counts, counts.size() * 4u, hipMemcpyDeviceToHost));
        std::vector<uint64_t> g_rows(G, 0u);
        for (uint32_t p = 0; p < P; ++p) {
            const uint32_t g = grp.empty() ? 0u : grp[p];
            if (g == afpr::kSkip) continue;
            const uint32_t m_a = std::min(counts[(size_t)ids[0][p] * AF_CNT_SLOTS + AF_CNT_COMPLETED], out->clock_capacity);
            const uint32_t m_b = std::min(counts[(size_t)ids[1][p] * AF_CNT_SLOTS + AF_CNT_COMPLETED], out->clock_capacity);
            g_rows[g] += std::min(std::min(m_a, m_b), n_draw);
            if (g_rows[g] > 0xFFFFFFFFull) return fail(AF_ERR_CAPACITY, "group " + std::to_string(g) + " could match 2^32 or more requests");
        }
    }
    // the pairs of one chunk: what the slots of the sides without a row_a / row_b output need must fit the memory
    const size_t slot_sides = (req->row_a ? 0u : 1u) + (req->row_b ? 0u : 1u);
    const size_t per_pair = slot_sides * (size_t)n_draw * 4u;
    uint32_t chunk = P;
    if (per_pair) {
        size_t mem_free = 0, mem_total = 0;
        HIP_TRY(hipMemGetInfo(&mem_free, &mem_total));
        size_t budget = e->draw_memory_bytes ? e->draw_memory_bytes : (size_t)160 << 30;
        const size_t avail = mem_free + e->pool_cap;
        if (budget > avail / 10u * 6u) budget = avail / 10u * 6u;
        if (budget / per_pair < chunk) chunk = (uint32_t)(budget / per_pair);
        if (chunk == 0) return fail(AF_ERR_CAPACITY, "draw_capacity too large for the device memory budget");
    }
    if (const char* env = std::getenv("AF_PAIRS_CHUNK")) {   // test hook: small chunks
        const long k = std::atol(env);
        if (k > 0 && (uint64_t)k < chunk) chunk = (uint32_t)k;
    }
    ScratchLayout lay;
    const size_t o_edges = lay.part(((size_t)W + 1u) * 8u);
    const size_t o_thr = lay.part(std::max<size_t>(T, 1u) * 8u);
    const size_t o_slots = lay.part((size_t)chunk * per_pair);
    if (int rc = pool_reserve(e, lay.at)) return rc;
    hipStream_t st = e->stream;
    if (W) HIP_TRY(hipMemcpyAsync(e->d_pool + o_edges, req->edges, ((size_t)W + 1u) * 8u, hipMemcpyHostToDevice, st));
    if (T) HIP_TRY(hipMemcpyAsync(e->d_pool + o_thr, req->thresholds, (size_t)T * 8u, hipMemcpyHostToDevice, st));
    const size_t cells = (size_t)G * wins;
    HIP_TRY(hipMemsetAsync(req->pair_counts, 0, (size_t)P * wins * afpr::kPairCounts * 4u, st));
    HIP_TRY(hipMemsetAsync(req->pair_sums, 0, (size_t)P * wins * 16u, st));
    HIP_TRY(hipMemsetAsync(req->cell_counts, 0, cells * afpr::kCellCounts * 8u, st));
    if (T) HIP_TRY(hipMemsetAsync(req->above, 0, cells * T * 8u, st));
    HIP_TRY(hipMemsetAsync(req->hist, 0, cells * 2u * B * 4u, st));
    HIP_TRY(hipMemsetAsync(req->tails, 0, cells * afpr::kTails * 4u, st));
    hipLaunchKernelGGL(afpr::af_pairs_init_extremes, dim3((uint32_t)((cells + 255u) / 256u)), dim3(256), 0, st, req->extremes, (uint64_t)cells);
    HIP_TRY(hipGetLastError());
    afpr::PairArgs a{};
    a.clock = out->clock;
    a.counts = out->counts;
    a.clock_cap = out->clock_capacity;
    a.cnt_completed_slot = AF_CNT_COMPLETED;
    a.times = req->times;
    a.n_draw = n_draw;
    a.n_win = W;
    a.wins = (uint32_t)wins;
    a.edges = reinterpret_cast<const double*>(e->d_pool + o_edges);
    a.thresholds = reinterpret_cast<const double*>(e->d_pool + o_thr);
    a.n_thr = T;
    a.chunks = (uint32_t)(((uint64_t)out->clock_capacity + afpr::kMatchRows - 1u) / afpr::kMatchRows);
    a.bin = bin;
    a.cell_counts = reinterpret_cast<unsigned long long*>(req->cell_counts);
    a.above = reinterpret_cast<unsigned long long*>(req->above);
    a.extremes = req->extremes;
    a.hist = req->hist;
    a.tails = req->tails;
    const bool in_lds = W <= afpr::kLdsPairWindows;
    const size_t lds = (in_lds && W ? ((size_t)W + 1u) * 8u : 0u) + (size_t)afpr::kWaves * 2u * B * 4u;
    const void* fn = in_lds ? reinterpret_cast<const void*>(afpr::af_pairs_reduce<true>) : reinterpret_cast<const void*>(afpr::af_pairs_reduce<false>);
    // (set before every launch: the attribute is per device and engines of several devices run in threads of one process)
    if (lds > 48u * 1024u) HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    for (uint32_t lo = 0; lo < P; lo += chunk) {
        const uint32_t nc = std::min(chunk, P - lo);
        uint32_t* scratch = reinterpret_cast<uint32_t*>(e->d_pool + o_slots);
        a.slot_a = req->row_a ? req->row_a + (size_t)lo * n_draw : scratch;
        a.slot_b = req->row_b ? req->row_b + (size_t)lo * n_draw : scratch + (req->row_a ? 0u : (size_t)nc * n_draw);
        HIP_TRY(hipMemsetAsync(a.slot_a, 0xFF, (size_t)nc * n_draw * 4u, st));
        HIP_TRY(hipMemsetAsync(a.slot_b, 0xFF, (size_t)nc * n_draw * 4u, st));
        a.pair_a = req->pair_a + lo;
        a.pair_b = req->pair_b + lo;
        a.group = req->group ? req->group + lo : nullptr;
        a.time_row = req->time_row + lo;
        a.n_pairs = nc;
        a.pair_counts = req->pair_counts + (size_t)lo * wins * afpr::kPairCounts;
        a.pair_sums = req->pair_sums + (size_t)lo * wins * 2u;
        a.unmatched = req->unmatched + (size_t)lo * 2u;
        const uint64_t items = (uint64_t)nc * 2u * a.chunks;
        const uint32_t match_blocks = (uint32_t)std::min<uint64_t>((items + afpr::kWaves - 1u) / afpr::kWaves, afpr::kMaxBlocks);
        hipLaunchKernelGGL(afpr::af_pairs_match, dim3(match_blocks), dim3(afpr::kThreads), 0, st, a);
        HIP_TRY(hipGetLastError());
        const uint32_t blocks = std::min<uint32_t>((nc + afpr::kWaves - 1u) / afpr::kWaves, afpr::kMaxBlocks);
        void* kargs[] = {&a};
        HIP_TRY(hipLaunchKernel(fn, dim3(blocks), dim3(afpr::kThreads), kargs, lds, st));
    }
    HIP_TRY(hipStreamSynchronize(st));   // (the host edges and thresholds are read by the copies until here)
    req->scratch_bytes = e->pool_cap;
    req->elapsed_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return AF_OK;
}

int af_engine_summarize_series_windows(af_engine_t* e, const af_outputs_t* out, af_series_windows_t* req) {
    if (!e || !out || !req) return fail(AF_ERR_INVALID, "NULL argument");
    if (e->plan_only) return fail(AF_ERR_NO_DEVICE, "planning-only engine (AF_DEVICE_PLAN_ONLY)");
    if (req->n_scenarios == 0 || req->n_groups == 0 || req->n_windows == 0)
        return fail(AF_ERR_INVALID, "empty series windows request (n_scenarios, n_groups and n_windows must be > 0)");
    if (!req->tick_edges) return fail(AF_ERR_INVALID, "series_windows.tick_edges is required");
    if (!req->count || !req->mean) return fail(AF_ERR_INVALID, "series_windows.count and series_windows.mean are required");
    if (!out->counts) return fail(AF_ERR_INVALID, "outputs.counts is required");
    if (!out->samples || out->tick_capacity == 0) return fail(AF_ERR_INVALID, "series windows need outputs.samples");
    const uint32_t n = req->n_scenarios, G = req->n_groups, W = req->n_windows, cap = out->tick_capacity;
    const uint32_t S = e->args.n_edges + 3u * e->args.n_servers, pitch = e->args.series_pitch;
    for (uint32_t k = 1; k <= W; ++k)
        if (!(req->tick_edges[k - 1] < req->tick_edges[k]))
            return fail(AF_ERR_INVALID, "tick_edges must be strictly increasing (edge " + std::to_string(k) + ")");
    for (uint32_t j = 0; req->thresholds && j < S; ++j)
        if (std::isnan(req->thresholds[j])) return fail(AF_ERR_INVALID, "threshold " + std::to_string(j) + " is NaN");
    if ((uint64_t)G * W >= 0xFFFFFFFFull) return fail(AF_ERR_CAPACITY, "n_groups * n_windows must be below 2^32 - 1");
    if (cap >= 0x80000000u) return fail(AF_ERR_CAPACITY, "tick_capacity must be below 2^31");
    if (S == 0 || pitch < S || pitch % 4u) return fail(AF_ERR_INVALID, "the plan has no sampled series");
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(e->device));
    std::vector<uint32_t> counts((size_t)n * AF_CNT_SLOTS), grp(req->group ? n : 0u);
    HIP_TRY(hipMemcpy(counts.data(), out->counts, counts.size() * 4u, hipMemcpyDeviceToHost));
    if (req->group) HIP_TRY(hipMemcpy(grp.data(), req->group, grp.size() * 4u, hipMemcpyDeviceToHost));
    // the groups' members, ascending; may a cell reach 2^32 values?
    std::vector<uint32_t> mem_off((size_t)G + 1u, 0u), members;
    std::vector<uint64_t> g_ticks(G, 0u);
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t g = req->group ? grp[s] : 0u;
        if (g == afsw::kSkip) continue;
        if (g >= G) return fail(AF_ERR_INVALID, "group id out of range (scenario " + std::to_string(s) + ": " + std::to_string(g) + ", n_groups " + std::to_string(G) + ")");
        mem_off[(size_t)g + 1u] += 1u;
        g_ticks[g] += std::min(counts[(size_t)s * AF_CNT_SLOTS + AF_CNT_TICKS], cap);
    }
    bool direct = true;
    for (uint32_t g = 0; g < G; ++g) {
        if (mem_off[(size_t)g + 1u] > 1u) direct = false;
        mem_off[(size_t)g + 1u] += mem_off[g];
    }
    members.resize(std::max<size_t>(mem_off[G], 1u));
    {
        std::vector<uint32_t> cursor(mem_off.begin(), mem_off.end() - 1);
        for (uint32_t s = 0; s < n; ++s) {
            const uint32_t g = req->group ? grp[s] : 0u;
            if (g != afsw::kSkip) members[cursor[g]++] = s;
        }
    }
    for (uint32_t g = 0; g < G; ++g) {
        if (g_ticks[g] <= 0xFFFFFFFFull) continue;   // (no window of the group can hold 2^32 rows)
        for (uint32_t w = 0; w < W; ++w) {
            uint64_t c = 0;
            for (uint32_t k = mem_off[g]; k < mem_off[(size_t)g + 1u]; ++k) {
                const uint32_t m = std::min(counts[(size_t)members[k] * AF_CNT_SLOTS + AF_CNT_TICKS], cap);
                c += std::min(req->tick_edges[w + 1u], m) - std::min(req->tick_edges[w], m);
            }
            if (c > 0xFFFFFFFFull) return fail(AF_ERR_CAPACITY, "window " + std::to_string(w) + " of group " + std::to_string(g) + " holds 2^32 or more samples");
        }
    }
    // scratch layout (256-byte aligned parts)
    ScratchLayout lay;
    const size_t R = direct ? 0u : (size_t)n * W * S;
    const size_t o_edges = lay.part(((size_t)W + 1u) * 4u), o_thr = lay.part((size_t)S * 8u), o_off = lay.part(((size_t)G + 1u) * 4u),
                 o_mem = lay.part(members.size() * 4u), o_sum = lay.part(R * 8u), o_min = lay.part(R * 4u), o_max = lay.part(R * 4u), o_above = lay.part(R * 4u);
    if (int rc = pool_reserve(e, lay.at)) return rc;
    unsigned char* b = e->d_pool;
    hipStream_t st = e->stream;
    std::vector<double> thr(S, 0.0);
    if (req->thresholds) thr.assign(req->thresholds, req->thresholds + S);
    HIP_TRY(hipMemcpyAsync(b + o_edges, req->tick_edges, ((size_t)W + 1u) * 4u, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b + o_thr, thr.data(), (size_t)S * 8u, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b + o_off, mem_off.data(), mem_off.size() * 4u, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b + o_mem, members.data(), members.size() * 4u, hipMemcpyHostToDevice, st));
    afsw::SwinArgs a{};
    a.samples = out->samples;
    a.counts = out->counts;
    a.tick_cap = cap;
    a.pitch = pitch;
    a.n_series = S;
    a.n_edges = e->args.n_edges;
    a.cnt_ticks_slot = AF_CNT_TICKS;
    a.group = req->group;
    a.n_scen = n;
    a.n_groups = G;
    a.n_win = W;
    a.direct = direct ? 1u : 0u;
    a.edges = reinterpret_cast<const uint32_t*>(b + o_edges);
    a.thr = reinterpret_cast<const double*>(b + o_thr);
    a.mem_off = reinterpret_cast<const uint32_t*>(b + o_off);
    a.members = reinterpret_cast<const uint32_t*>(b + o_mem);
    a.rec_sum = reinterpret_cast<unsigned long long*>(b + o_sum);
    a.rec_min = reinterpret_cast<uint32_t*>(b + o_min);
    a.rec_max = reinterpret_cast<uint32_t*>(b + o_max);
    a.rec_above = reinterpret_cast<uint32_t*>(b + o_above);
    a.count = req->count;
    a.mean = req->mean;
    a.minv = req->minv;
    a.maxv = req->maxv;
    a.above = req->above;
    // a wave per (scenario, run of windows): runs as long as leave the chip some 32 768 waves
    const uint32_t want_runs = (32768u + n - 1u) / n;
    a.run = std::max(1u, W / want_runs);
    const uint64_t items = (uint64_t)n * ((W + a.run - 1u) / a.run);
    hipLaunchKernelGGL(afsw::af_swin_partial, dim3((uint32_t)((items + afsw::kWaves - 1u) / afsw::kWaves)), dim3(afsw::kThreads), 0, st, a);
    HIP_TRY(hipGetLastError());
    if (!direct || mem_off[G] < G) {   // the members' fold; after a direct pass only the cells of groups without a member
        const uint64_t entries = (uint64_t)G * W * S;
        for (uint64_t f = 0; f < entries; f += kBlocksPerLaunch * afsw::kReduceThreads) {
            const uint64_t blocks = std::min<uint64_t>(kBlocksPerLaunch, (entries - f + afsw::kReduceThreads - 1u) / afsw::kReduceThreads);
            hipLaunchKernelGGL(afsw::af_swin_reduce, dim3((uint32_t)blocks), dim3(afsw::kReduceThreads), 0, st, a, f, entries);
            HIP_TRY(hipGetLastError());
        }
    }
    HIP_TRY(hipStreamSynchronize(st));
    req->scratch_bytes = e->pool_cap;
    req->elapsed_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return AF_OK;
}

// Excursions of the sampled series above a threshold per (scenario, window of ticks, series) (af_series_excursions.hpp): the
// host checks the request and uploads the edges and the thresholds; one streaming pass over the sample rows writes the cells.
int af_engine_summarize_series_excursions(af_engine_t* e, const af_outputs_t* out, af_series_excursions_t* req) {
    if (!e || !out || !req) return fail(AF_ERR_INVALID, "NULL argument");
    if (e->plan_only) return fail(AF_ERR_NO_DEVICE, "planning-only engine (AF_DEVICE_PLAN_ONLY)");
    if (req->n_scenarios == 0 || req->n_windows == 0)
        return fail(AF_ERR_INVALID, "empty series excursions request (n_scenarios and n_windows must be > 0)");
    if (!req->tick_edges) return fail(AF_ERR_INVALID, "series_excursions.tick_edges is required");
    if (!out->counts) return fail(AF_ERR_INVALID, "outputs.counts is required");
    if (!out->samples) return fail(AF_ERR_INVALID, "series excursions need outputs.samples");
    if (out->tick_capacity == 0) return fail(AF_ERR_INVALID, "series excursions need a tick_capacity above 0");
    const uint32_t n = req->n_scenarios, W = req->n_windows, cap = out->tick_capacity;
    const uint32_t S = e->args.n_edges + 3u * e->args.n_servers, pitch = e->args.series_pitch;
    for (uint32_t k = 1; k <= W; ++k)
        if (!(req->tick_edges[k - 1] < req->tick_edges[k]))
            return fail(AF_ERR_INVALID, "tick_edges must be strictly increasing (edge " + std::to_string(k) + ")");
    for (uint32_t j = 0; req->thresholds && j < S; ++j)
        if (std::isnan(req->thresholds[j])) return fail(AF_ERR_INVALID, "threshold " + std::to_string(j) + " is NaN");
    if ((uint64_t)n * W >= 0xFFFFFFFFull) return fail(AF_ERR_CAPACITY, "n_scenarios * n_windows must be below 2^32 - 1");
    if (cap >= 0x80000000u) return fail(AF_ERR_CAPACITY, "tick_capacity must be below 2^31");
    if (S == 0 || pitch < S || pitch % 4u) return fail(AF_ERR_INVALID, "the plan has no sampled series");
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(e->device));
    ScratchLayout lay;
    const size_t o_edges = lay.part(((size_t)W + 1u) * 4u), o_thr = lay.part((size_t)S * 8u);
    if (int rc = pool_reserve(e, lay.at)) return rc;
    unsigned char* b = e->d_pool;
    hipStream_t st = e->stream;
    std::vector<double> thr(S, 0.0);
    if (req->thresholds) thr.assign(req->thresholds, req->thresholds + S);
    HIP_TRY(hipMemcpyAsync(b + o_edges, req->tick_edges, ((size_t)W + 1u) * 4u, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b + o_thr, thr.data(), (size_t)S * 8u, hipMemcpyHostToDevice, st));
    afsx::SexArgs a{};
    a.samples = out->samples;
    a.counts = out->counts;
    a.tick_cap = cap;
    a.pitch = pitch;
    a.n_series = S;
    a.n_edges = e->args.n_edges;
    a.cnt_ticks_slot = AF_CNT_TICKS;
    a.n_scen = n;
    a.n_win = W;
    a.edges = reinterpret_cast<const uint32_t*>(b + o_edges);
    a.thr = reinterpret_cast<const double*>(b + o_thr);
    a.count = req->count;
    a.above = req->above;
    a.runs = req->runs;
    a.longest = req->longest;
    a.longest_start = req->longest_start;
    a.first = req->first;
    a.last = req->last;
    a.peak_tick = req->peak_tick;
    // a wave per (scenario, run of windows): runs as long as leave the chip some 32 768 waves (af_engine_summarize_series_windows' rule)
    const uint32_t want_runs = (32768u + n - 1u) / n;
    a.run = std::max(1u, W / want_runs);
    const uint64_t items = (uint64_t)n * ((W + a.run - 1u) / a.run);
    hipLaunchKernelGGL(afsx::af_sexc_kernel, dim3((uint32_t)((items + afsx::kWaves - 1u) / afsx::kWaves)), dim3(afsx::kThreads), 0, st, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));   // (the host thresholds are read by the copy until here)
    req->scratch_bytes = e->pool_cap;
    req->elapsed_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return AF_OK;
}

// Histograms of the sampled series per (group, window of ticks, output column) (af_series_histogram.hpp).  The host reads the
// group ids and the counts back and checks them, sorts the output columns by series, zeroes the outputs; one streaming pass.
static_assert(afsh::kMaxBins == AF_MAX_SERIES_HISTOGRAM_BINS, "the kernel's bins are the header's");

int af_engine_summarize_series_histogram(af_engine_t* e, const af_outputs_t* out, af_series_histogram_t* req) {
    if (!e || !out || !req) return fail(AF_ERR_INVALID, "NULL argument");
    if (e->plan_only) return fail(AF_ERR_NO_DEVICE, "planning-only engine (AF_DEVICE_PLAN_ONLY)");
    if (req->n_scenarios == 0 || req->n_groups == 0 || req->n_windows == 0)
        return fail(AF_ERR_INVALID, "empty series histogram request (n_scenarios, n_groups and n_windows must be > 0)");
    if (!req->tick_edges) return fail(AF_ERR_INVALID, "series_histogram.tick_edges is required");
    if (!req->hist) return fail(AF_ERR_INVALID, "series_histogram.hist is required");
    const uint32_t n = req->n_scenarios, G = req->n_groups, W = req->n_windows, cap = out->tick_capacity, B = req->n_bins;
    const uint32_t S = e->args.n_edges + 3u * e->args.n_servers, pitch = e->args.series_pitch;
    if (B == 0 || B > AF_MAX_SERIES_HISTOGRAM_BINS)
        return fail(AF_ERR_INVALID, "series_histogram.n_bins must be 1 .. AF_MAX_SERIES_HISTOGRAM_BINS (" + std::to_string(AF_MAX_SERIES_HISTOGRAM_BINS) + ")");
    for (uint32_t k = 1; k <= W; ++k)
        if (!(req->tick_edges[k - 1] < req->tick_edges[k]))
            return fail(AF_ERR_INVALID, "tick_edges must be strictly increasing (edge " + std::to_string(k) + ")");
    if ((req->n_columns == 0) != (req->columns == nullptr)) return fail(AF_ERR_INVALID, "series_histogram.columns and n_columns must be given together");
    for (uint32_t c = 0; c < req->n_columns; ++c)
        if (req->columns[c] >= S) return fail(AF_ERR_INVALID, "column " + std::to_string(c) + " names series " + std::to_string(req->columns[c]) + " of " + std::to_string(S));
    if ((req->lo == nullptr) != (req->width == nullptr)) return fail(AF_ERR_INVALID, "series_histogram.lo and width must be given together");
    const uint32_t Co = req->n_columns ? req->n_columns : S;
    for (uint32_t c = 0; req->lo && c < Co; ++c) {
        if (!std::isfinite(req->lo[c])) return fail(AF_ERR_INVALID, "lo of column " + std::to_string(c) + " is not finite");
        if (!(std::isfinite(req->width[c]) && req->width[c] > 0.0)) return fail(AF_ERR_INVALID, "width of column " + std::to_string(c) + " is not a finite number above 0");
    }
    if (!out->counts) return fail(AF_ERR_INVALID, "outputs.counts is required");
    if (!out->samples || cap == 0) return fail(AF_ERR_INVALID, "series histograms need outputs.samples");
    if ((uint64_t)G * W >= 0xFFFFFFFFull) return fail(AF_ERR_CAPACITY, "n_groups * n_windows must be below 2^32 - 1");
    if (cap >= 0x80000000u) return fail(AF_ERR_CAPACITY, "tick_capacity must be below 2^31");
    if (S == 0 || pitch < S || pitch % 4u) return fail(AF_ERR_INVALID, "the plan has no sampled series");
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(e->device));
    std::vector<uint32_t> counts((size_t)n * AF_CNT_SLOTS), grp;
    HIP_TRY(hipMemcpy(counts.data(), out->counts, counts.size() * 4u, hipMemcpyDeviceToHost));
    if (int rc = read_groups(req->group, n, G, grp)) return rc;
    // may a cell reach 2^32 values?
    {
        std::vector<uint64_t> g_ticks(G, 0u);
        bool big = false;
        for (uint32_t s = 0; s < n; ++s) {
            const uint32_t g = grp.empty() ? 0u : grp[s];
            if (g == afsh::kSkip) continue;
            g_ticks[g] += std::min(counts[(size_t)s * AF_CNT_SLOTS + AF_CNT_TICKS], cap);
            big = big || g_ticks[g] > 0xFFFFFFFFull;
        }
        if (big) {   // (else no window of a group can hold 2^32 rows)
            std::vector<uint64_t> cells((size_t)G * W, 0u);
            for (uint32_t s = 0; s < n; ++s) {
                const uint32_t g = grp.empty() ? 0u : grp[s];
                if (g == afsh::kSkip || g_ticks[g] <= 0xFFFFFFFFull) continue;
                const uint32_t m = std::min(counts[(size_t)s * AF_CNT_SLOTS + AF_CNT_TICKS], cap);
                for (uint32_t w = 0; w < W && req->tick_edges[w] < m; ++w) {
                    uint64_t& c = cells[(size_t)g * W + w];
                    c += std::min(req->tick_edges[w + 1u], m) - req->tick_edges[w];
                    if (c > 0xFFFFFFFFull) return fail(AF_ERR_CAPACITY, "window " + std::to_string(w) + " of group " + std::to_string(g) + " holds 2^32 or more samples");
                }
            }
        }
    }
    // the slots: the output columns sorted by series (a counting sort, stable)
    std::vector<uint32_t> first((size_t)S + 1u, 0u), scol(Co);
    std::vector<double> slo(Co), swidth(Co);
    for (uint32_t c = 0; c < Co; ++c) first[(size_t)(req->columns ? req->columns[c] : c) + 1u] += 1u;
    for (uint32_t j = 0; j < S; ++j) first[(size_t)j + 1u] += first[j];
    {
        std::vector<uint32_t> cursor(first.begin(), first.end() - 1);
        for (uint32_t c = 0; c < Co; ++c) {
            const uint32_t q = cursor[req->columns ? req->columns[c] : c]++;
            scol[q] = c;
            slo[q] = req->lo ? req->lo[c] : 0.0;
            swidth[q] = req->width ? req->width[c] : 1.0;
        }
    }
    // the chunks: as many slots as the LDS of a wave holds, no series twice
    const uint32_t chunk_cap = std::max(1u, afsh::kWaveLdsWords / (B + 2u));
    std::vector<uint32_t> cstart{0u}, series_of(Co);
    for (uint32_t j = 0; j < S; ++j)
        for (uint32_t q = first[j]; q < first[(size_t)j + 1u]; ++q) series_of[q] = j;
    uint32_t lds_slots = 1u;
    for (uint32_t q = 1; q <= Co; ++q)
        if (q == Co || q - cstart.back() == chunk_cap || series_of[q] == series_of[q - 1u]) {
            lds_slots = std::max(lds_slots, q - cstart.back());
            cstart.push_back(q);
        }
    const uint32_t n_chunks = (uint32_t)cstart.size() - 1u;
    ScratchLayout lay;
    const size_t o_edges = lay.part(((size_t)W + 1u) * 4u), o_first = lay.part(((size_t)S + 1u) * 4u), o_scol = lay.part((size_t)Co * 4u),
                 o_lo = lay.part((size_t)Co * 8u), o_width = lay.part((size_t)Co * 8u), o_chunk = lay.part(cstart.size() * 4u);
    if (int rc = pool_reserve(e, lay.at)) return rc;
    unsigned char* b = e->d_pool;
    hipStream_t st = e->stream;
    HIP_TRY(hipMemcpyAsync(b + o_edges, req->tick_edges, ((size_t)W + 1u) * 4u, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b + o_first, first.data(), first.size() * 4u, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b + o_scol, scol.data(), (size_t)Co * 4u, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b + o_lo, slo.data(), (size_t)Co * 8u, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b + o_width, swidth.data(), (size_t)Co * 8u, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b + o_chunk, cstart.data(), cstart.size() * 4u, hipMemcpyHostToDevice, st));
    const size_t cells = (size_t)G * W;
    HIP_TRY(hipMemsetAsync(req->hist, 0, cells * Co * B * 4u, st));
    if (req->count) HIP_TRY(hipMemsetAsync(req->count, 0, cells * 4u, st));
    if (req->under) HIP_TRY(hipMemsetAsync(req->under, 0, cells * Co * 4u, st));
    if (req->over) HIP_TRY(hipMemsetAsync(req->over, 0, cells * Co * 4u, st));
    afsh::ShArgs a{};
    a.samples = out->samples;
    a.counts = out->counts;
    a.tick_cap = cap;
    a.pitch = pitch;
    a.n_series = S;
    a.n_edges = e->args.n_edges;
    a.cnt_ticks_slot = AF_CNT_TICKS;
    a.group = req->group;
    a.n_scen = n;
    a.n_win = W;
    a.edges = reinterpret_cast<const uint32_t*>(b + o_edges);
    a.n_out = Co;
    a.n_bins = B;
    a.n_chunks = n_chunks;
    a.lds_slots = lds_slots;
    a.cstart = reinterpret_cast<const uint32_t*>(b + o_chunk);
    a.first = reinterpret_cast<const uint32_t*>(b + o_first);
    a.scol = reinterpret_cast<const uint32_t*>(b + o_scol);
    a.slo = reinterpret_cast<const double*>(b + o_lo);
    a.swidth = reinterpret_cast<const double*>(b + o_width);
    a.count = req->count;
    a.hist = req->hist;
    a.under = req->under;
    a.over = req->over;
    // a wave per (scenario, run of windows): runs as long as leave the chip some 32 768 waves (af_engine_summarize_series_windows' rule)
    const uint32_t want_runs = (32768u + n - 1u) / n;
    a.run = std::max(1u, W / want_runs);
    const uint64_t items = (uint64_t)n * ((W + a.run - 1u) / a.run);
    const size_t lds = (size_t)afsh::kWaves * lds_slots * (B + 2u) * 4u;
    hipLaunchKernelGGL(afsh::af_shist_kernel, dim3((uint32_t)((items + afsh::kWaves - 1u) / afsh::kWaves)), dim3(afsh::kThreads), lds, st, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));   // (the host vectors are read by the copies until here)
    req->scratch_bytes = e->pool_cap;
    req->elapsed_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return AF_OK;
}

// Combinations across the sampled series per (group, window of ticks, combination) (af_series_combined.hpp).  The host checks
// the combinations, reads the group ids and the counts back, builds the groups' member lists and zeroes the histogram outputs;
// one streaming pass over the sample rows, then -- unless every group is a single scenario -- the fold of the members' records.
static_assert(afsc::kMaxCombos == AF_MAX_SERIES_COMBINATIONS && afsc::kMaxBins == AF_MAX_SERIES_HISTOGRAM_BINS, "the kernel's limits are the header's");
static_assert(afsc::kSum == AF_COMBINE_SUM && afsc::kMin == AF_COMBINE_MIN && afsc::kMax == AF_COMBINE_MAX && afsc::kSpread == AF_COMBINE_SPREAD,
              "the kernel's ops are the header's");

int af_engine_summarize_series_combined(af_engine_t* e, const af_outputs_t* out, af_series_combined_t* req) {
    if (!e || !out || !req) return fail(AF_ERR_INVALID, "NULL argument");
    if (e->plan_only) return fail(AF_ERR_NO_DEVICE, "planning-only engine (AF_DEVICE_PLAN_ONLY)");
    if (req->n_scenarios == 0 || req->n_groups == 0 || req->n_windows == 0)
        return fail(AF_ERR_INVALID, "empty series combined request (n_scenarios, n_groups and n_windows must be > 0)");
    if (!req->tick_edges) return fail(AF_ERR_INVALID, "series_combined.tick_edges is required");
    if (!req->mean) return fail(AF_ERR_INVALID, "series_combined.mean is required");
    const uint32_t n = req->n_scenarios, G = req->n_groups, W = req->n_windows, cap = out->tick_capacity, B = req->n_bins, Cn = req->n_combos;
    const uint32_t S = e->args.n_edges + 3u * e->args.n_servers, pitch = e->args.series_pitch, n_edges = e->args.n_edges;
    if (Cn == 0 || Cn > AF_MAX_SERIES_COMBINATIONS)
        return fail(AF_ERR_INVALID, "series_combined.n_combos must be 1 .. AF_MAX_SERIES_COMBINATIONS (" + std::to_string(AF_MAX_SERIES_COMBINATIONS) + ")");
    if (!req->op || !req->col_start || !req->cols) return fail(AF_ERR_INVALID, "series_combined.op, col_start and cols are required");
    if (B > AF_MAX_SERIES_HISTOGRAM_BINS)
        return fail(AF_ERR_INVALID, "series_combined.n_bins must be at most AF_MAX_SERIES_HISTOGRAM_BINS (" + std::to_string(AF_MAX_SERIES_HISTOGRAM_BINS) + ")");
    if (B == 0 ? (req->hist || req->under || req->over) : !req->hist)
        return fail(AF_ERR_INVALID, "series_combined.hist (with under and over) and n_bins must be given together");
    if ((req->lo == nullptr) != (req->width == nullptr)) return fail(AF_ERR_INVALID, "series_combined.lo and width must be given together");
    for (uint32_t k = 1; k <= W; ++k)
        if (!(req->tick_edges[k - 1] < req->tick_edges[k]))
            return fail(AF_ERR_INVALID, "tick_edges must be strictly increasing (edge " + std::to_string(k) + ")");
    if (S == 0 || pitch < S || pitch % 4u) return fail(AF_ERR_INVALID, "the plan has no sampled series");
    const auto is_ram = [&](uint32_t j) { return j >= n_edges && (j - n_edges) % 3u == 2u; };
    std::vector<afsc::Combo> combos(Cn);
    uint32_t max_cols = 0;
    if (req->col_start[0] != 0u) return fail(AF_ERR_INVALID, "series_combined.col_start must begin at 0");
    for (uint32_t c = 0; c < Cn; ++c) {
        const std::string who = "combination " + std::to_string(c);
        const uint32_t c0 = req->col_start[c], c1 = req->col_start[c + 1u];
        if (req->op[c] > AF_COMBINE_SPREAD) return fail(AF_ERR_INVALID, who + " has an unknown op (" + std::to_string(req->op[c]) + ")");
        if (c1 <= c0) return fail(AF_ERR_INVALID, who + " has no columns");
        for (uint32_t k = c0; k < c1; ++k) {
            if (req->cols[k] >= S) return fail(AF_ERR_INVALID, who + " names series " + std::to_string(req->cols[k]) + " of " + std::to_string(S));
            if (k > c0 && !(req->cols[k - 1u] < req->cols[k])) return fail(AF_ERR_INVALID, who + ": the columns must be strictly increasing");
            if (is_ram(req->cols[k]) != is_ram(req->cols[c0])) return fail(AF_ERR_INVALID, who + " mixes ram_in_use columns with integer series");
        }
        if (req->thresholds && std::isnan(req->thresholds[c])) return fail(AF_ERR_INVALID, "threshold of " + who + " is NaN");
        if (req->lo) {
            if (!std::isfinite(req->lo[c])) return fail(AF_ERR_INVALID, "lo of " + who + " is not finite");
            if (!(std::isfinite(req->width[c]) && req->width[c] > 0.0)) return fail(AF_ERR_INVALID, "width of " + who + " is not a finite number above 0");
        }
        combos[c] = afsc::Combo{req->op[c], c0, c1, is_ram(req->cols[c0]) ? 1u : 0u, req->thresholds ? req->thresholds[c] : 0.0,
                                req->lo ? req->lo[c] : 0.0, req->width ? req->width[c] : 1.0};
        max_cols = std::max(max_cols, c1 - c0);
    }
    const uint32_t n_cols = req->col_start[Cn];
    if (!out->counts) return fail(AF_ERR_INVALID, "outputs.counts is required");
    if (!out->samples || cap == 0) return fail(AF_ERR_INVALID, "series combinations need outputs.samples");
    if ((uint64_t)G * W >= 0xFFFFFFFFull) return fail(AF_ERR_CAPACITY, "n_groups * n_windows must be below 2^32 - 1");
    if (cap >= 0x80000000u) return fail(AF_ERR_CAPACITY, "tick_capacity must be below 2^31");
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(e->device));
    std::vector<uint32_t> counts((size_t)n * AF_CNT_SLOTS), grp;
    HIP_TRY(hipMemcpy(counts.data(), out->counts, counts.size() * 4u, hipMemcpyDeviceToHost));
    if (int rc = read_groups(req->group, n, G, grp)) return rc;
    // the groups' members, ascending; may a cell reach 2^32 rows, or its rows times the longest column list?
    std::vector<uint32_t> mem_off((size_t)G + 1u, 0u), members;
    std::vector<uint64_t> g_ticks(G, 0u);
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t g = grp.empty() ? 0u : grp[s];
        if (g == afsc::kSkip) continue;
        mem_off[(size_t)g + 1u] += 1u;
        g_ticks[g] += std::min(counts[(size_t)s * AF_CNT_SLOTS + AF_CNT_TICKS], cap);
    }
    bool direct = true;
    for (uint32_t g = 0; g < G; ++g) {
        if (mem_off[(size_t)g + 1u] > 1u) direct = false;
        mem_off[(size_t)g + 1u] += mem_off[g];
    }
    members.resize(std::max<size_t>(mem_off[G], 1u));
    {
        std::vector<uint32_t> cursor(mem_off.begin(), mem_off.end() - 1);
        for (uint32_t s = 0; s < n; ++s) {
            const uint32_t g = grp.empty() ? 0u : grp[s];
            if (g != afsc::kSkip) members[cursor[g]++] = s;
        }
    }
    for (uint32_t g = 0; g < G; ++g) {
        if (g_ticks[g] * max_cols <= 0xFFFFFFFFull) continue;   // (no window of the group can reach either limit)
        for (uint32_t w = 0; w < W; ++w) {
            uint64_t c = 0;
            for (uint32_t k = mem_off[g]; k < mem_off[(size_t)g + 1u]; ++k) {
                const uint32_t m = std::min(counts[(size_t)members[k] * AF_CNT_SLOTS + AF_CNT_TICKS], cap);
                c += std::min(req->tick_edges[w + 1u], m) - std::min(req->tick_edges[w], m);
            }
            if (c > 0xFFFFFFFFull) return fail(AF_ERR_CAPACITY, "window " + std::to_string(w) + " of group " + std::to_string(g) + " holds 2^32 or more samples");
            if (c * max_cols > 0xFFFFFFFFull)
                return fail(AF_ERR_CAPACITY, "window " + std::to_string(w) + " of group " + std::to_string(g) + ": its rows times the longest column list reach 2^32");
        }
    }
    // scratch layout (256-byte aligned parts)
    ScratchLayout lay;
    const size_t R = direct ? 0u : (size_t)n * W * Cn;
    const size_t o_edges = lay.part(((size_t)W + 1u) * 4u), o_combo = lay.part((size_t)Cn * sizeof(afsc::Combo)), o_cols = lay.part((size_t)n_cols * 4u),
                 o_off = lay.part(((size_t)G + 1u) * 4u), o_mem = lay.part(members.size() * 4u), o_sum = lay.part(R * 8u), o_comp = lay.part(R * 8u),
                 o_min = lay.part(R * 8u), o_max = lay.part(R * 8u), o_above = lay.part(R * 4u);
    if (int rc = pool_reserve(e, lay.at)) return rc;
    unsigned char* b = e->d_pool;
    hipStream_t st = e->stream;
    HIP_TRY(hipMemcpyAsync(b + o_edges, req->tick_edges, ((size_t)W + 1u) * 4u, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b + o_combo, combos.data(), (size_t)Cn * sizeof(afsc::Combo), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b + o_cols, req->cols, (size_t)n_cols * 4u, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b + o_off, mem_off.data(), mem_off.size() * 4u, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b + o_mem, members.data(), members.size() * 4u, hipMemcpyHostToDevice, st));
    const size_t cells = (size_t)G * W;
    if (B) {
        HIP_TRY(hipMemsetAsync(req->hist, 0, cells * Cn * B * 4u, st));
        if (req->under) HIP_TRY(hipMemsetAsync(req->under, 0, cells * Cn * 4u, st));
        if (req->over) HIP_TRY(hipMemsetAsync(req->over, 0, cells * Cn * 4u, st));
    }
    afsc::ScArgs a{};
    a.samples = out->samples;
    a.counts = out->counts;
    a.tick_cap = cap;
    a.pitch = pitch;
    a.cnt_ticks_slot = AF_CNT_TICKS;
    a.group = req->group;
    a.n_scen = n;
    a.n_groups = G;
    a.n_win = W;
    a.direct = direct ? 1u : 0u;
    a.edges = reinterpret_cast<const uint32_t*>(b + o_edges);
    a.n_combos = Cn;
    a.n_bins = B;
    a.per = std::max(1u, std::min(afsc::kPer, afsc::kWaveLdsWords / (B + 2u)));
    a.combos = reinterpret_cast<const afsc::Combo*>(b + o_combo);
    a.cols = reinterpret_cast<const uint32_t*>(b + o_cols);
    a.mem_off = reinterpret_cast<const uint32_t*>(b + o_off);
    a.members = reinterpret_cast<const uint32_t*>(b + o_mem);
    a.rec_sum = reinterpret_cast<unsigned long long*>(b + o_sum);
    a.rec_comp = reinterpret_cast<double*>(b + o_comp);
    a.rec_min = reinterpret_cast<unsigned long long*>(b + o_min);
    a.rec_max = reinterpret_cast<unsigned long long*>(b + o_max);
    a.rec_above = reinterpret_cast<uint32_t*>(b + o_above);
    a.count = req->count;
    a.mean = req->mean;
    a.minv = req->minv;
    a.maxv = req->maxv;
    a.above = req->above;
    a.hist = req->hist;
    a.under = req->under;
    a.over = req->over;
    // a wave per (scenario, run of windows): runs as long as leave the chip some 32 768 waves (af_engine_summarize_series_windows' rule)
    const uint32_t want_runs = (32768u + n - 1u) / n;
    a.run = std::max(1u, W / want_runs);
    const uint64_t items = (uint64_t)n * ((W + a.run - 1u) / a.run);
    const size_t lds = B ? (size_t)afsc::kWaves * a.per * (B + 2u) * 4u : 0u;
    hipLaunchKernelGGL(afsc::af_scomb_partial, dim3((uint32_t)((items + afsc::kWaves - 1u) / afsc::kWaves)), dim3(afsc::kThreads), lds, st, a);
    HIP_TRY(hipGetLastError());
    if (!direct || mem_off[G] < G) {   // the members' fold; after a direct pass only the cells of groups without a member
        const uint64_t entries = (uint64_t)G * W * Cn;
        for (uint64_t f = 0; f < entries; f += kBlocksPerLaunch * afsc::kReduceThreads) {
            const uint64_t blocks = std::min<uint64_t>(kBlocksPerLaunch, (entries - f + afsc::kReduceThreads - 1u) / afsc::kReduceThreads);
            hipLaunchKernelGGL(afsc::af_scomb_reduce, dim3((uint32_t)blocks), dim3(afsc::kReduceThreads), 0, st, a, f, entries);
            HIP_TRY(hipGetLastError());
        }
    }
    HIP_TRY(hipStreamSynchronize(st));   // (the host vectors are read by the copies until here)
    req->scratch_bytes = e->pool_cap;
    req->elapsed_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return AF_OK;
}

// Joint moments of pairs of the sampled series per (group, window of ticks, pair) (af_series_joint.hpp).  The host checks the
// pairs, reads the group ids and the counts back, builds the groups' member lists and picks the load form; one streaming pass
// over the sample rows, then -- unless every group is a single scenario -- the fold of the members' records.
static_assert(afsj::kMaxPairs == AF_MAX_SERIES_PAIRS, "the kernel's limit is the header's");

int af_engine_summarize_series_joint(af_engine_t* e, const af_outputs_t* out, af_series_joint_t* req) {
    if (!e || !out || !req) return fail(AF_ERR_INVALID, "NULL argument");
    if (e->plan_only) return fail(AF_ERR_NO_DEVICE, "planning-only engine (AF_DEVICE_PLAN_ONLY)");
    if (req->n_scenarios == 0 || req->n_groups == 0 || req->n_windows == 0)
        return fail(AF_ERR_INVALID, "empty series joint request (n_scenarios, n_groups and n_windows must be > 0)");
    if (!req->tick_edges) return fail(AF_ERR_INVALID, "series_joint.tick_edges is required");
    if (!req->n || !req->sxy) return fail(AF_ERR_INVALID, "series_joint.n and sxy are required");
    const uint32_t n = req->n_scenarios, G = req->n_groups, W = req->n_windows, cap = out->tick_capacity, Pn = req->n_pairs;
    const uint32_t S = e->args.n_edges + 3u * e->args.n_servers, pitch = e->args.series_pitch, n_edges = e->args.n_edges;
    if (Pn == 0 || Pn > AF_MAX_SERIES_PAIRS)
        return fail(AF_ERR_INVALID, "series_joint.n_pairs must be 1 .. AF_MAX_SERIES_PAIRS (" + std::to_string(AF_MAX_SERIES_PAIRS) + ")");
    if (!req->a || !req->b || !req->lag) return fail(AF_ERR_INVALID, "series_joint.a, b and lag are required");
    for (uint32_t k = 1; k <= W; ++k)
        if (!(req->tick_edges[k - 1] < req->tick_edges[k]))
            return fail(AF_ERR_INVALID, "tick_edges must be strictly increasing (edge " + std::to_string(k) + ")");
    if (S == 0 || pitch < S || pitch % 4u) return fail(AF_ERR_INVALID, "the plan has no sampled series");
    const auto is_ram = [&](uint32_t j) { return j >= n_edges && (j - n_edges) % 3u == 2u; };
    std::vector<afsj::Pair> pairs(Pn);
    for (uint32_t p = 0; p < Pn; ++p) {
        const std::string who = "pair " + std::to_string(p);
        for (const uint32_t j : {req->a[p], req->b[p]}) {
            if (j >= S) return fail(AF_ERR_INVALID, who + " names series " + std::to_string(j) + " of " + std::to_string(S));
            if (is_ram(j)) return fail(AF_ERR_INVALID, who + " names a ram_in_use column (series " + std::to_string(j) + "): pairs take integer series only");
        }
        if (req->lag[p] >= 0x80000000u) return fail(AF_ERR_INVALID, "the lag of " + who + " must be below 2^31");
        pairs[p] = afsj::Pair{req->a[p], req->b[p], req->lag[p], 0u};
    }
    if (!out->counts) return fail(AF_ERR_INVALID, "outputs.counts is required");
    if (!out->samples || cap == 0) return fail(AF_ERR_INVALID, "series joint moments need outputs.samples");
    if ((uint64_t)G * W >= 0xFFFFFFFFull) return fail(AF_ERR_CAPACITY, "n_groups * n_windows must be below 2^32 - 1");
    if (cap >= 0x80000000u) return fail(AF_ERR_CAPACITY, "tick_capacity must be below 2^31");
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(e->device));
    std::vector<uint32_t> counts((size_t)n * AF_CNT_SLOTS), grp;
    HIP_TRY(hipMemcpy(counts.data(), out->counts, counts.size() * 4u, hipMemcpyDeviceToHost));
    if (int rc = read_groups(req->group, n, G, grp)) return rc;
    // the groups' members, ascending; may a cell reach 2^32 rows?
    std::vector<uint32_t> mem_off((size_t)G + 1u, 0u), members;
    std::vector<uint64_t> g_ticks(G, 0u);
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t g = grp.empty() ? 0u : grp[s];
        if (g == afsj::kSkip) continue;
        mem_off[(size_t)g + 1u] += 1u;
        g_ticks[g] += std::min(counts[(size_t)s * AF_CNT_SLOTS + AF_CNT_TICKS], cap);
    }
    bool direct = true;
    for (uint32_t g = 0; g < G; ++g) {
        if (mem_off[(size_t)g + 1u] > 1u) direct = false;
        mem_off[(size_t)g + 1u] += mem_off[g];
    }
    members.resize(std::max<size_t>(mem_off[G], 1u));
    {
        std::vector<uint32_t> cursor(mem_off.begin(), mem_off.end() - 1);
        for (uint32_t s = 0; s < n; ++s) {
            const uint32_t g = grp.empty() ? 0u : grp[s];
            if (g != afsj::kSkip) members[cursor[g]++] = s;
        }
    }
    for (uint32_t g = 0; g < G; ++g) {
        if (g_ticks[g] <= 0xFFFFFFFFull) continue;   // (no window of the group can reach the limit)
        for (uint32_t w = 0; w < W; ++w) {
            uint64_t c = 0;
            for (uint32_t k = mem_off[g]; k < mem_off[(size_t)g + 1u]; ++k) {
                const uint32_t m = std::min(counts[(size_t)members[k] * AF_CNT_SLOTS + AF_CNT_TICKS], cap);
                c += std::min(req->tick_edges[w + 1u], m) - std::min(req->tick_edges[w], m);
            }
            if (c > 0xFFFFFFFFull) return fail(AF_ERR_CAPACITY, "window " + std::to_string(w) + " of group " + std::to_string(g) + " holds 2^32 or more samples");
        }
    }
    // the load form: rows that fit a wave's LDS 64 at a time are staged, with as many rows after them as the largest lag that
    // still fits asks for; the pairs with longer lags read their second word from global memory
    const bool staged = pitch <= afsj::kMaxStagedPitch && reinterpret_cast<uintptr_t>(out->samples) % 16u == 0u;
    uint32_t ring = 64u, lag_lds = 0u;
    if (staged) {
        for (uint32_t p = 0; p < Pn; ++p) {
            uint32_t need = 64u;
            while (need < 64u + (uint64_t)pairs[p].lag && need < afsj::kWaveLdsWords) need *= 2u;
            if (need >= 64u + (uint64_t)pairs[p].lag && (uint64_t)need * (pitch + 1u) <= afsj::kWaveLdsWords && pairs[p].lag > lag_lds) {
                lag_lds = pairs[p].lag;
                ring = std::max(ring, need);
            }
        }
    }
    // scratch layout (256-byte aligned parts)
    ScratchLayout lay;
    const size_t R = direct ? 0u : (size_t)n * W * Pn;
    const size_t o_edges = lay.part(((size_t)W + 1u) * 4u), o_pairs = lay.part((size_t)Pn * sizeof(afsj::Pair)), o_off = lay.part(((size_t)G + 1u) * 4u),
                 o_mem = lay.part(members.size() * 4u), o_r64 = lay.part(R * 40u), o_r32 = lay.part(R * 12u);
    if (int rc = pool_reserve(e, lay.at)) return rc;
    unsigned char* b = e->d_pool;
    hipStream_t st = e->stream;
    HIP_TRY(hipMemcpyAsync(b + o_edges, req->tick_edges, ((size_t)W + 1u) * 4u, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b + o_pairs, pairs.data(), (size_t)Pn * sizeof(afsj::Pair), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b + o_off, mem_off.data(), mem_off.size() * 4u, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b + o_mem, members.data(), members.size() * 4u, hipMemcpyHostToDevice, st));
    afsj::SjArgs a{};
    a.samples = out->samples;
    a.counts = out->counts;
    a.tick_cap = cap;
    a.pitch = pitch;
    a.cnt_ticks_slot = AF_CNT_TICKS;
    a.group = req->group;
    a.n_scen = n;
    a.n_groups = G;
    a.n_win = W;
    a.direct = direct ? 1u : 0u;
    a.edges = reinterpret_cast<const uint32_t*>(b + o_edges);
    a.n_pairs = Pn;
    while ((1u << a.p2_log) < Pn) a.p2_log += 1u;
    a.pairs = reinterpret_cast<const afsj::Pair*>(b + o_pairs);
    a.staged = staged ? 1u : 0u;
    a.ring = ring;
    a.lag_lds = lag_lds;
    a.p4 = pitch / 4u;
    a.q64 = 64u / a.p4;
    a.r64 = 64u % a.p4;
    a.mem_off = reinterpret_cast<const uint32_t*>(b + o_off);
    a.members = reinterpret_cast<const uint32_t*>(b + o_mem);
    a.rec64 = reinterpret_cast<unsigned long long*>(b + o_r64);
    a.rec32 = reinterpret_cast<uint32_t*>(b + o_r32);
    a.n = req->n;
    a.sx = reinterpret_cast<unsigned long long*>(req->sx);
    a.sy = reinterpret_cast<unsigned long long*>(req->sy);
    a.sxx = reinterpret_cast<unsigned long long*>(req->sxx);
    a.syy = reinterpret_cast<unsigned long long*>(req->syy);
    a.sxy = reinterpret_cast<unsigned long long*>(req->sxy);
    // a wave per (scenario, run of windows): runs as long as leave the chip some 32 768 waves (af_engine_summarize_series_windows' rule)
    const uint32_t want_runs = (32768u + n - 1u) / n;
    a.run = std::max(1u, W / want_runs);
    const uint64_t items = (uint64_t)n * ((W + a.run - 1u) / a.run);
    const size_t lds = staged ? (size_t)afsj::kWaves * ring * (pitch + 1u) * 4u : 0u;
    hipLaunchKernelGGL(afsj::af_sjoint_partial, dim3((uint32_t)((items + afsj::kWaves - 1u) / afsj::kWaves)), dim3(afsj::kThreads), lds, st, a);
    HIP_TRY(hipGetLastError());
    if (!direct || mem_off[G] < G) {   // the members' fold; after a direct pass only the cells of groups without a member
        const uint64_t entries = (uint64_t)G * W * Pn;
        for (uint64_t f = 0; f < entries; f += kBlocksPerLaunch * afsj::kFoldThreads) {
            const uint64_t blocks = std::min<uint64_t>(kBlocksPerLaunch, (entries - f + afsj::kFoldThreads - 1u) / afsj::kFoldThreads);
            hipLaunchKernelGGL(afsj::af_sjoint_fold, dim3((uint32_t)blocks), dim3(afsj::kFoldThreads), 0, st, a, f, entries);
            HIP_TRY(hipGetLastError());
        }
    }
    HIP_TRY(hipStreamSynchronize(st));   // (the host vectors are read by the copies until here)
    req->scratch_bytes = e->pool_cap;
    req->elapsed_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return AF_OK;
}

// Warm-up truncation (MSER) of integer series per (group, window of ticks, column) (af_series_warmup.hpp).  The host checks the
// columns and the width contract, reads the group ids back to check them and picks the load form; one streaming pass adds the
// batch sums into a zeroed buffer and lowers the groups' batch counts, then a wave per cell finds the truncation point.
static_assert(afwu::kMaxColumns == AF_MAX_SERIES_WARMUP_COLUMNS, "the kernel's limit is the header's");

int af_engine_summarize_series_warmup(af_engine_t* e, const af_outputs_t* out, af_series_warmup_t* req) {
    if (!e || !out || !req) return fail(AF_ERR_INVALID, "NULL argument");
    if (e->plan_only) return fail(AF_ERR_NO_DEVICE, "planning-only engine (AF_DEVICE_PLAN_ONLY)");
    if (req->n_scenarios == 0 || req->n_groups == 0 || req->n_windows == 0)
        return fail(AF_ERR_INVALID, "empty series warmup request (n_scenarios, n_groups and n_windows must be > 0)");
    if (!req->tick_edges) return fail(AF_ERR_INVALID, "series_warmup.tick_edges is required");
    if (!req->batches || !req->trunc) return fail(AF_ERR_INVALID, "series_warmup.batches and trunc are required");
    const uint32_t n = req->n_scenarios, G = req->n_groups, W = req->n_windows, cap = out->tick_capacity, Cn = req->n_columns, B = req->batch;
    const uint32_t S = e->args.n_edges + 3u * e->args.n_servers, pitch = e->args.series_pitch, n_edges = e->args.n_edges;
    if (Cn == 0 || Cn > AF_MAX_SERIES_WARMUP_COLUMNS)
        return fail(AF_ERR_INVALID, "series_warmup.n_columns must be 1 .. AF_MAX_SERIES_WARMUP_COLUMNS (" + std::to_string(AF_MAX_SERIES_WARMUP_COLUMNS) + ")");
    if (!req->columns) return fail(AF_ERR_INVALID, "series_warmup.columns is required");
    if (B == 0) return fail(AF_ERR_INVALID, "series_warmup.batch must be at least 1 tick");
    for (uint32_t k = 1; k <= W; ++k)
        if (!(req->tick_edges[k - 1] < req->tick_edges[k]))
            return fail(AF_ERR_INVALID, "tick_edges must be strictly increasing (edge " + std::to_string(k) + ")");
    if (S == 0 || pitch < S || pitch % 4u) return fail(AF_ERR_INVALID, "the plan has no sampled series");
    for (uint32_t c = 0; c < Cn; ++c) {
        const uint32_t j = req->columns[c];
        if (j >= S) return fail(AF_ERR_INVALID, "column " + std::to_string(c) + " names series " + std::to_string(j) + " of " + std::to_string(S));
        if (j >= n_edges && (j - n_edges) % 3u == 2u)
            return fail(AF_ERR_INVALID, "column " + std::to_string(c) + " names a ram_in_use column (series " + std::to_string(j) + "): the warm-up rule takes integer series only");
    }
    if (!out->counts) return fail(AF_ERR_INVALID, "outputs.counts is required");
    if (!out->samples || cap == 0) return fail(AF_ERR_INVALID, "series warmup needs outputs.samples");
    if ((uint64_t)G * W >= 0xFFFFFFFFull) return fail(AF_ERR_CAPACITY, "n_groups * n_windows must be below 2^32 - 1");
    if (cap >= 0x80000000u) return fail(AF_ERR_CAPACITY, "tick_capacity must be below 2^31");
    if ((uint64_t)n * B > (1ull << 32)) return fail(AF_ERR_CAPACITY, "n_scenarios * batch must be at most 2^32 (a batch sum is 64 bits)");
    // the batches a window can hold, and where its batches start in a (group, column)'s sequence
    std::vector<uint32_t> boff((size_t)W + 1u, 0u);
    for (uint32_t w = 0; w < W; ++w) {
        const uint32_t nb = (std::min(req->tick_edges[w + 1u], cap) - std::min(req->tick_edges[w], cap)) / B;
        if (nb >= afwu::kMaxWindowBatches) return fail(AF_ERR_CAPACITY, "window " + std::to_string(w) + " holds 2^25 or more batches");
        boff[(size_t)w + 1u] = boff[w] + nb;   // (at most tick_capacity / B in all: below 2^31)
    }
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(e->device));
    {
        std::vector<uint32_t> grp;
        if (int rc = read_groups(req->group, n, G, grp)) return rc;
    }
    const uint32_t NB = boff[W];
    const bool staged = pitch <= afwu::kMaxStagedPitch && reinterpret_cast<uintptr_t>(out->samples) % 16u == 0u;
    // scratch layout (256-byte aligned parts)
    ScratchLayout lay;
    const size_t y_bytes = (size_t)G * Cn * NB * 8u, j_bytes = (size_t)G * W * 4u;
    const size_t o_edges = lay.part(((size_t)W + 1u) * 4u), o_boff = lay.part(((size_t)W + 1u) * 4u), o_cols = lay.part((size_t)Cn * 4u),
                 o_jmin = lay.part(j_bytes), o_y = lay.part(y_bytes);
    if (int rc = pool_reserve(e, lay.at)) return rc;
    unsigned char* b = e->d_pool;
    hipStream_t st = e->stream;
    HIP_TRY(hipMemcpyAsync(b + o_edges, req->tick_edges, ((size_t)W + 1u) * 4u, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b + o_boff, boff.data(), boff.size() * 4u, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b + o_cols, req->columns, (size_t)Cn * 4u, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(b + o_jmin, 0xFF, j_bytes, st));   // afwu::kNone: no member yet
    if (y_bytes) HIP_TRY(hipMemsetAsync(b + o_y, 0, y_bytes, st));
    afwu::SwArgs a{};
    a.samples = out->samples;
    a.counts = out->counts;
    a.tick_cap = cap;
    a.pitch = pitch;
    a.cnt_ticks_slot = AF_CNT_TICKS;
    a.group = req->group;
    a.n_scen = n;
    a.n_groups = G;
    a.n_win = W;
    a.edges = reinterpret_cast<const uint32_t*>(b + o_edges);
    a.boff = reinterpret_cast<const uint32_t*>(b + o_boff);
    a.n_batches = NB;
    a.batch = B;
    a.n_cols = Cn;
    a.cols = reinterpret_cast<const uint32_t*>(b + o_cols);
    a.staged = staged ? 1u : 0u;
    a.p4 = pitch / 4u;
    a.q64 = 64u / a.p4;
    a.r64 = 64u % a.p4;
    a.y = reinterpret_cast<uint64_t*>(b + o_y);
    a.jmin = reinterpret_cast<uint32_t*>(b + o_jmin);
    a.batches = req->batches;
    a.trunc = req->trunc;
    a.s1 = req->s1;
    a.s2 = req->s2;
    a.s1_all = req->s1_all;
    a.s2_all = req->s2_all;
    // a wave per (scenario, run of windows): runs as long as leave the chip some 32 768 waves (af_engine_summarize_series_windows' rule)
    const uint32_t want_runs = (32768u + n - 1u) / n;
    a.run = std::max(1u, W / want_runs);
    const uint64_t items = (uint64_t)n * ((W + a.run - 1u) / a.run);
    const size_t lds = staged ? (size_t)afwu::kWaves * 64u * (pitch + 1u) * 4u : 0u;
    hipLaunchKernelGGL(afwu::af_swarm_batches, dim3((uint32_t)((items + afwu::kWaves - 1u) / afwu::kWaves)), dim3(afwu::kThreads), lds, st, a);
    HIP_TRY(hipGetLastError());
    const uint64_t cells = (uint64_t)G * W * Cn;   // a wave each
    for (uint64_t f = 0; f < cells; f += kBlocksPerLaunch * afwu::kWaves) {
        const uint64_t blocks = std::min<uint64_t>(kBlocksPerLaunch, (cells - f + afwu::kWaves - 1u) / afwu::kWaves);
        hipLaunchKernelGGL(afwu::af_swarm_cell, dim3((uint32_t)blocks), dim3(afwu::kThreads), 0, st, a, f, cells);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(st));   // (the host vectors are read by the copies until here)
    req->scratch_bytes = e->pool_cap;
    req->elapsed_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return AF_OK;
}

// Quantiles of the sampled series per (group, window of ticks, series) (af_series_quantiles.hpp).  The host reads the group ids
// and the counts back, checks them, sizes every cell and sends it to its tier: the small cells in one launch sequence, the
// large ones a chunk at a time -- as many cells as the histogram budget holds, at least one.
constexpr size_t kSeriesQuantileHistBudget = (size_t)128u << 20;
static_assert(afsq::kMaxRanks == 2u * AF_MAX_SERIES_QUANTILE_LEVELS, "two ranks per level");

int af_engine_summarize_series_quantiles(af_engine_t* e, const af_outputs_t* out, af_series_quantiles_t* req) {
    if (!e || !out || !req) return fail(AF_ERR_INVALID, "NULL argument");
    if (e->plan_only) return fail(AF_ERR_NO_DEVICE, "planning-only engine (AF_DEVICE_PLAN_ONLY)");
    if (req->n_scenarios == 0 || req->n_groups == 0 || req->n_windows == 0)
        return fail(AF_ERR_INVALID, "empty series quantiles request (n_scenarios, n_groups and n_windows must be > 0)");
    if (!req->tick_edges) return fail(AF_ERR_INVALID, "series_quantiles.tick_edges is required");
    if (!req->quantiles) return fail(AF_ERR_INVALID, "series_quantiles.quantiles is required");
    const uint32_t n = req->n_scenarios, G = req->n_groups, W = req->n_windows, cap = out->tick_capacity, Q = req->n_levels;
    const uint32_t S = e->args.n_edges + 3u * e->args.n_servers, pitch = e->args.series_pitch;
    if (Q == 0 || Q > AF_MAX_SERIES_QUANTILE_LEVELS)
        return fail(AF_ERR_INVALID, "series_quantiles.n_levels must be 1 .. AF_MAX_SERIES_QUANTILE_LEVELS (" + std::to_string(AF_MAX_SERIES_QUANTILE_LEVELS) + ")");
    if (!req->levels) return fail(AF_ERR_INVALID, "series_quantiles.levels is required");
    for (uint32_t i = 0; i < Q; ++i)
        if (!(req->levels[i] >= 0.0 && req->levels[i] <= 1.0)) return fail(AF_ERR_INVALID, "quantile level " + std::to_string(i) + " is not in [0, 1]");
    for (uint32_t k = 1; k <= W; ++k)
        if (!(req->tick_edges[k - 1] < req->tick_edges[k]))
            return fail(AF_ERR_INVALID, "tick_edges must be strictly increasing (edge " + std::to_string(k) + ")");
    if ((req->n_columns == 0) != (req->columns == nullptr)) return fail(AF_ERR_INVALID, "series_quantiles.columns and n_columns must be given together");
    for (uint32_t c = 0; c < req->n_columns; ++c)
        if (req->columns[c] >= S) return fail(AF_ERR_INVALID, "column " + std::to_string(c) + " names series " + std::to_string(req->columns[c]) + " of " + std::to_string(S));
    if (!out->counts) return fail(AF_ERR_INVALID, "outputs.counts is required");
    if (!out->samples || cap == 0) return fail(AF_ERR_INVALID, "series quantiles need outputs.samples");
    if ((uint64_t)G * W >= 0xFFFFFFFFull) return fail(AF_ERR_CAPACITY, "n_groups * n_windows must be below 2^32 - 1");
    if (cap >= 0x80000000u) return fail(AF_ERR_CAPACITY, "tick_capacity must be below 2^31");
    if (S == 0 || pitch < S || pitch % 4u) return fail(AF_ERR_INVALID, "the plan has no sampled series");
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(e->device));
    std::vector<uint32_t> counts((size_t)n * AF_CNT_SLOTS), grp(req->group ? n : 0u);
    HIP_TRY(hipMemcpy(counts.data(), out->counts, counts.size() * 4u, hipMemcpyDeviceToHost));
    if (req->group) HIP_TRY(hipMemcpy(grp.data(), req->group, grp.size() * 4u, hipMemcpyDeviceToHost));
    // the groups' members, ascending
    std::vector<uint32_t> mem_off((size_t)G + 1u, 0u), members;
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t g = req->group ? grp[s] : 0u;
        if (g == afsq::kNone) continue;
        if (g >= G) return fail(AF_ERR_INVALID, "group id out of range (scenario " + std::to_string(s) + ": " + std::to_string(g) + ", n_groups " + std::to_string(G) + ")");
        mem_off[(size_t)g + 1u] += 1u;
    }
    for (uint32_t g = 0; g < G; ++g) mem_off[(size_t)g + 1u] += mem_off[g];
    members.resize(std::max<size_t>(mem_off[G], 1u));
    {
        std::vector<uint32_t> cursor(mem_off.begin(), mem_off.end() - 1);
        for (uint32_t s = 0; s < n; ++s) {
            const uint32_t g = req->group ? grp[s] : 0u;
            if (g != afsq::kNone) members[cursor[g]++] = s;
        }
    }
    // every cell's size, its tier
    const size_t C = (size_t)G * W;
    std::vector<uint32_t> small_cells, lcell, lcell_n, cell_lidx;   // (small_cells: cell, size)
    uint32_t small_max = 0;
    {
        std::vector<uint64_t> row(W);
        for (uint32_t g = 0; g < G; ++g) {
            std::fill(row.begin(), row.end(), 0u);
            for (uint32_t k = mem_off[g]; k < mem_off[(size_t)g + 1u]; ++k) {
                const uint32_t m = std::min(counts[(size_t)members[k] * AF_CNT_SLOTS + AF_CNT_TICKS], cap);
                for (uint32_t w = 0; w < W && req->tick_edges[w] < m; ++w) row[w] += std::min(req->tick_edges[w + 1u], m) - req->tick_edges[w];
            }
            for (uint32_t w = 0; w < W; ++w) {
                if (row[w] > 0xFFFFFFFFull) return fail(AF_ERR_CAPACITY, "window " + std::to_string(w) + " of group " + std::to_string(g) + " holds 2^32 or more samples");
                const uint32_t cell = (uint32_t)((size_t)g * W + w);
                if (row[w] <= afsq::kSmallMax) {
                    small_cells.push_back(cell);
                    small_cells.push_back((uint32_t)row[w]);
                    small_max = std::max(small_max, (uint32_t)row[w]);
                } else {
                    if (cell_lidx.empty()) cell_lidx.assign(C, afsq::kNone);
                    cell_lidx[cell] = (uint32_t)lcell.size();
                    lcell.push_back(cell);
                    lcell_n.push_back((uint32_t)row[w]);
                }
            }
        }
    }
    // the selected series: distinct ones ascending, and per series the chain of its output columns
    const uint32_t Co = req->n_columns ? req->n_columns : S;
    std::vector<uint32_t> u_of(pitch, afsq::kNone), u_series, head, next(Co, afsq::kNone), sel_groups;
    for (uint32_t c = 0; c < Co; ++c) u_of[req->columns ? req->columns[c] : c] = 0u;
    for (uint32_t j = 0; j < S; ++j)
        if (u_of[j] != afsq::kNone) {
            u_of[j] = (uint32_t)u_series.size();
            u_series.push_back(j);
            if (sel_groups.empty() || sel_groups.back() != j / 4u) sel_groups.push_back(j / 4u);
        }
    const uint32_t U = (uint32_t)u_series.size(), R = 2u * Q;
    head.assign(U, afsq::kNone);
    for (uint32_t c = Co; c-- > 0u;) {   // (back to front: a chain runs in ascending column order)
        const uint32_t u = u_of[req->columns ? req->columns[c] : c];
        next[c] = head[u];
        head[u] = c;
    }
    uint32_t lds_slots = 0;
    for (uint32_t cg : sel_groups) {
        uint32_t k = 0;
        for (uint32_t j = cg * 4u; j < cg * 4u + 4u && j < S; ++j) k += u_of[j] != afsq::kNone ? 1u : 0u;
        lds_slots = std::max(lds_slots, k);
    }
    const uint32_t n_small = (uint32_t)(small_cells.size() / 2u), n_large = (uint32_t)lcell.size(), n_sg = (uint32_t)sel_groups.size();
    const size_t pair_bytes = (size_t)R * (afsq::kBins * 4u + 16u) + 12u;
    const uint32_t chunk = n_large ? (uint32_t)std::min<size_t>(n_large, std::max<size_t>(1u, kSeriesQuantileHistBudget / (pair_bytes * U))) : 0u;
    const size_t P = (size_t)chunk * U;   // the (cell, column) pairs of a chunk
    if (P > 0xFFFFFFFFull / R) return fail(AF_ERR_CAPACITY, "too many selected series for one large cell");
    // scratch layout (256-byte aligned parts)
    ScratchLayout lay;
    const size_t o_edges = lay.part(((size_t)W + 1u) * 4u), o_lev = lay.part((size_t)Q * 8u), o_off = lay.part(((size_t)G + 1u) * 4u),
                 o_mem = lay.part(members.size() * 4u), o_uof = lay.part((size_t)pitch * 4u), o_user = lay.part((size_t)U * 4u),
                 o_head = lay.part((size_t)U * 4u), o_next = lay.part((size_t)Co * 4u), o_sg = lay.part((size_t)n_sg * 4u),
                 o_small = lay.part((size_t)n_small * 8u), o_lidx = lay.part(n_large ? C * 4u : 0u), o_lcell = lay.part((size_t)n_large * 4u),
                 o_ln = lay.part((size_t)n_large * 4u), o_bmin = lay.part(P * 4u), o_bmax = lay.part(P * 4u), o_ns = lay.part(P * 4u),
                 o_pfx = lay.part(P * R * 4u), o_rank = lay.part(P * R * 4u), o_slot = lay.part(P * R * 4u), o_spfx = lay.part(P * R * 4u),
                 o_hist = lay.part(P * R * afsq::kBins * 4u);
    if (int rc = pool_reserve(e, lay.at)) return rc;
    req->scratch_bytes = e->pool_cap;
    unsigned char* b = e->d_pool;
    hipStream_t st = e->stream;
    const auto up = [&](size_t o, const void* src, size_t bytes) { return bytes ? hipMemcpyAsync(b + o, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess; };
    HIP_TRY(up(o_edges, req->tick_edges, ((size_t)W + 1u) * 4u));
    HIP_TRY(up(o_lev, req->levels, (size_t)Q * 8u));
    HIP_TRY(up(o_off, mem_off.data(), mem_off.size() * 4u));
    HIP_TRY(up(o_mem, members.data(), members.size() * 4u));
    HIP_TRY(up(o_uof, u_of.data(), (size_t)pitch * 4u));
    HIP_TRY(up(o_user, u_series.data(), (size_t)U * 4u));
    HIP_TRY(up(o_head, head.data(), (size_t)U * 4u));
    HIP_TRY(up(o_next, next.data(), (size_t)Co * 4u));
    HIP_TRY(up(o_sg, sel_groups.data(), (size_t)n_sg * 4u));
    HIP_TRY(up(o_small, small_cells.data(), (size_t)n_small * 8u));
    HIP_TRY(up(o_lidx, cell_lidx.data(), cell_lidx.size() * 4u));
    HIP_TRY(up(o_lcell, lcell.data(), (size_t)n_large * 4u));
    HIP_TRY(up(o_ln, lcell_n.data(), (size_t)n_large * 4u));
    const auto u32p = [&](size_t o) { return reinterpret_cast<uint32_t*>(b + o); };
    afsq::SqArgs a{};
    a.samples = out->samples;
    a.counts = out->counts;
    a.tick_cap = cap;
    a.pitch = pitch;
    a.n_series = S;
    a.n_edges = e->args.n_edges;
    a.cnt_ticks_slot = AF_CNT_TICKS;
    a.group = req->group;
    a.n_scen = n;
    a.n_groups = G;
    a.n_win = W;
    a.edges = u32p(o_edges);
    a.mem_off = u32p(o_off);
    a.members = u32p(o_mem);
    a.n_lev = Q;
    a.n_out = Co;
    a.n_uniq = U;
    a.n_ranks = R;
    a.levels = reinterpret_cast<const double*>(b + o_lev);
    a.u_of = u32p(o_uof);
    a.u_series = u32p(o_user);
    a.head = u32p(o_head);
    a.next = u32p(o_next);
    a.small_cells = u32p(o_small);
    a.sel_groups = u32p(o_sg);
    a.n_sg = n_sg;
    a.lds_stride = pow2_at_least(std::max(small_max, 1u));
    a.cell_lidx = u32p(o_lidx);
    a.lcell = u32p(o_lcell);
    a.lcell_n = u32p(o_ln);
    a.bmin = u32p(o_bmin);
    a.bmax = u32p(o_bmax);
    a.n_slots = u32p(o_ns);
    a.pfx = u32p(o_pfx);
    a.rank_in = u32p(o_rank);
    a.slot_of = u32p(o_slot);
    a.slot_pfx = u32p(o_spfx);
    a.hist = u32p(o_hist);
    a.count = req->count;
    a.quant = req->quantiles;
    // a wave per (scenario, run of windows): runs as long as leave the chip some 32 768 waves
    const uint32_t want_runs = (32768u + n - 1u) / n;
    a.run = std::max(1u, W / want_runs);
    const uint64_t items = (uint64_t)n * ((W + a.run - 1u) / a.run);
    const dim3 row_grid((uint32_t)((items + afsq::kWaves - 1u) / afsq::kWaves));
    const uint64_t small_items = (uint64_t)n_small * n_sg;
    const size_t small_lds = (size_t)lds_slots * a.lds_stride * 4u;
    for (uint64_t i0 = 0; i0 < small_items; i0 += kBlocksPerLaunch) {
        hipLaunchKernelGGL(afsq::af_sq_small, dim3((uint32_t)std::min<uint64_t>(kBlocksPerLaunch, small_items - i0)), dim3(afsq::kThreads), small_lds, st, a, i0);
        HIP_TRY(hipGetLastError());
    }
    for (uint32_t l0 = 0; l0 < n_large; l0 += chunk) {
        a.l0 = l0;
        a.l1 = std::min(n_large, l0 + chunk);
        const size_t pairs = (size_t)(a.l1 - a.l0) * U;
        HIP_TRY(hipMemsetAsync(a.bmin, 0xFF, pairs * 4u, st));
        HIP_TRY(hipMemsetAsync(a.bmax, 0, pairs * 4u, st));
        hipLaunchKernelGGL(afsq::af_sq_rows<0>, row_grid, dim3(afsq::kThreads), 0, st, a, 0);
        HIP_TRY(hipGetLastError());
        // level 0 counts into slot 0 of every pair: only those are cleared here; af_sq_select clears the slots of the next level
        HIP_TRY(hipMemset2DAsync(a.hist, (size_t)R * afsq::kBins * 4u, 0, afsq::kBins * 4u, pairs, st));
        for (int level = 0; level * afsq::kBits < 32; ++level) {   // (a column whose key is complete takes no part)
            if (level == 0) hipLaunchKernelGGL(afsq::af_sq_rows<1>, row_grid, dim3(afsq::kThreads), 0, st, a, level);
            else hipLaunchKernelGGL(afsq::af_sq_rows<2>, row_grid, dim3(afsq::kThreads), 0, st, a, level);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(afsq::af_sq_select, dim3((uint32_t)pairs), dim3(afsq::kThreads), 0, st, a, level);
            HIP_TRY(hipGetLastError());
        }
        const uint64_t entries = (uint64_t)pairs * Q;
        hipLaunchKernelGGL(afsq::af_sq_final, dim3((uint32_t)((entries + afsq::kThreads - 1u) / afsq::kThreads)), dim3(afsq::kThreads), 0, st, a, entries);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(st));
    req->elapsed_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return AF_OK;
}

// af_engine_run + af_engine_summarize in one call, with the same results.  Where the sweep runs as ONE launch sequence of the
// stage-parallel kernel (one chunk), the kernel is launched ONCE and its waves bump a counter as their scenarios finish; the analyzer
// waits on a second stream until that counter reaches the scenarios of the kernel's full residency rounds (gate_for_launch) and
// then runs beside the last, partial round, which leaves most of the chip idle (BASELINE config 2: 10 000 scenarios = 2.44 rounds
// of 4 096 waves; the 0.44 round takes 8.5 ms); the analyzer is HBM-bound and the simulation kernel VALU-bound.  Scenarios it
// meets unfinished go on retry lists and are summarised after the run.  Scenarios the kernel hands back are simulated
// again afterwards: their sweep is then summarised once more, in full.
int af_engine_run_summarized(af_engine_t* e, const af_sweep_t* sweep, const af_outputs_t* out, const af_summary_t* sum) {
    if (int rc = check_summary_request(e, out, sum)) return rc;
    if (!sweep || sum->n_scenarios != sweep->n_scenarios) return fail(AF_ERR_INVALID, "summary.n_scenarios must equal sweep.n_scenarios");
    // (a profiler that collects counters runs the kernels of a process ONE AT A TIME -- rocprofv3 --pmc sets
    // ROCPROF_COUNTER_COLLECTION --: nothing can run beside anything, and a dispatch held back behind a stream wait can stall
    // the tool's serialiser.  There, and with AF_NO_SUMMARY_OVERLAP set, the analyzer runs after the simulation.)
    const bool serialised = std::getenv("AF_NO_SUMMARY_OVERLAP") != nullptr || std::getenv("ROCPROF_COUNTER_COLLECTION") != nullptr;
    e->fused_sum = serialised ? nullptr : sum;
    e->fused_out = out;
    e->fused_done = false;
    e->stats.summary_beside_ms = 0.0;
    const int rc = af_engine_run(e, sweep, out);
    e->fused_sum = nullptr;
    e->fused_out = nullptr;
    if (rc != AF_OK) {
        // (whatever went wrong after the second stream began to wait for the kernel's counter: let it through and drain it)
        if (e->h_done_count != nullptr) *e->h_done_count = 0xFFFFFFFFu;
        if (e->stream2 != nullptr) (void)hipStreamSynchronize(e->stream2);
        (void)hipGetLastError();
        return rc;
    }
    const uint32_t n = sum->n_scenarios;
    uint32_t n_lat = 0u, n_ser = 0u;
    if (e->fused_done) {   // what the analyzer beside the kernel met unfinished
        HIP_TRY(hipMemcpy(&n_lat, e->d_retry, 4u, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(&n_ser, e->d_retry + (size_t)n + 1u, 4u, hipMemcpyDeviceToHost));
    }
    HIP_TRY(hipEventRecord(e->ev0, e->stream));
    if (e->fused_done) {
        if (int rc2 = launch_summary_kernels(e, out, sum, 0u, n, e->stream, nullptr, nullptr, e->d_retry + 1u, n_lat, e->d_retry + (size_t)n + 2u, n_ser)) return rc2;
    } else {
        if (int rc2 = launch_summary_kernels(e, out, sum, 0u, n, e->stream)) return rc2;
    }
    HIP_TRY(hipEventRecord(e->ev1, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e->ev0, e->ev1));
    e->stats.summary_ms = ms;                 // the part of the analyzer that was NOT hidden
    const bool want_lat = sum->stats || sum->rps || sum->hist;
    e->stats.summary_overlapped = e->fused_done ? n - (want_lat ? n_lat : n_ser) : 0u;
    return AF_OK;
}

const char* af_engine_flow_reason(const af_engine_t* e) { return e ? e->flow_reason.c_str() : ""; }

int af_engine_stats(const af_engine_t* e, af_stats_t* stats) {
    if (!e || !stats) return fail(AF_ERR_INVALID, "NULL argument");
    *stats = e->stats;
    return AF_OK;
}

void af_engine_destroy(af_engine_t* e) {
    if (!e) return;
    if (e->plan_only) {   // (owns no device state)
        delete e;
        return;
    }
    (void)hipSetDevice(e->device);
    if (e->d_blob) (void)hipFree(e->d_blob);
    if (e->d_state) (void)hipFree(e->d_state);
    if (e->d_sweep) (void)hipFree(e->d_sweep);
    if (e->ev0) (void)hipEventDestroy(e->ev0);
    if (e->ev1) (void)hipEventDestroy(e->ev1);
    if (e->ev2) (void)hipEventDestroy(e->ev2);
    if (e->ev3) (void)hipEventDestroy(e->ev3);
    if (e->ev4) (void)hipEventDestroy(e->ev4);
    if (e->ev_s0) (void)hipEventDestroy(e->ev_s0);
    if (e->ev_s1) (void)hipEventDestroy(e->ev_s1);
    if (e->stream2) (void)hipStreamDestroy(e->stream2);
    if (e->d_done_flags) (void)hipFree(e->d_done_flags);
    if (e->d_retry) (void)hipFree(e->d_retry);
    if (e->d_pool) (void)hipFree(e->d_pool);
    if (e->h_done_count) (void)hipHostFree(e->h_done_count);
    if (e->d_draws) (void)hipFree(e->d_draws);
    if (e->d_pre_flags) (void)hipFree(e->d_pre_flags);
    if (e->d_tie) (void)hipFree(e->d_tie);
    if (e->d_n_shared) (void)hipFree(e->d_n_shared);
    if (e->d_map) (void)hipFree(e->d_map);
    if (e->d_order) (void)hipFree(e->d_order);
    if (e->d_tick) (void)hipFree(e->d_tick);
    if (e->d_arr) (void)hipFree(e->d_arr);
    if (e->d_arr_flags) (void)hipFree(e->d_arr_flags);
    if (e->d_fb) (void)hipFree(e->d_fb);
    if (e->d_slot) (void)hipFree(e->d_slot);
    if (e->d_prof) (void)hipFree(e->d_prof);
    if (e->jit_module) (void)hipModuleUnload(e->jit_module);
    if (e->flow_jit_module) (void)hipModuleUnload(e->flow_jit_module);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
}

// ---- RCCL, resolved at run time (include/asyncflow_hip.h: "the one collective") ------------------------
namespace {
struct nccl_id_t { char internal[AF_COMM_ID_BYTES]; };
struct RcclApi {
    void* handle = nullptr;
    int (*GetUniqueId)(nccl_id_t*) = nullptr;
    int (*CommInitRank)(void**, int, nccl_id_t, int) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    int (*CommCount)(void*, int*) = nullptr;      // (optional: af_comm_count)
    int (*CommUserRank)(void*, int*) = nullptr;
    std::string origin;
    bool ok() const { return AllGather != nullptr; }
};
RcclApi g_rccl;

bool rccl_bind(void* h, const std::string& origin) {
    RcclApi r;
    r.handle = h;
    r.origin = origin;
    void* scope = h ? h : RTLD_DEFAULT;
    r.GetUniqueId = reinterpret_cast<decltype(r.GetUniqueId)>(dlsym(scope, "ncclGetUniqueId"));
    r.CommInitRank = reinterpret_cast<decltype(r.CommInitRank)>(dlsym(scope, "ncclCommInitRank"));
    r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(dlsym(scope, "ncclCommDestroy"));
    r.AllGather = reinterpret_cast<decltype(r.AllGather)>(dlsym(scope, "ncclAllGather"));
    r.GroupStart = reinterpret_cast<decltype(r.GroupStart)>(dlsym(scope, "ncclGroupStart"));
    r.GroupEnd = reinterpret_cast<decltype(r.GroupEnd)>(dlsym(scope, "ncclGroupEnd"));
    r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(dlsym(scope, "ncclGetErrorString"));
    r.CommCount = reinterpret_cast<decltype(r.CommCount)>(dlsym(scope, "ncclCommCount"));
    r.CommUserRank = reinterpret_cast<decltype(r.CommUserRank)>(dlsym(scope, "ncclCommUserRank"));
    if (!r.GetUniqueId || !r.CommInitRank || !r.CommDestroy || !r.AllGather || !r.GroupStart || !r.GroupEnd) return false;
    g_rccl = r;
    return true;
}
int rccl_need() {
    if (g_rccl.ok()) return AF_OK;
    if (rccl_bind(nullptr, "already in the process")) return AF_OK;
    std::vector<std::string> cands;
    if (const char* env = std::getenv("ASYNCFLOW_RCCL_LIB")) cands.push_back(env);
    cands.push_back("librccl.so.1");
    cands.push_back("librccl.so");
    for (const std::string& c : cands)
        if (void* h = dlopen(c.c_str(), RTLD_NOW | RTLD_LOCAL))
            if (rccl_bind(h, c)) return AF_OK;
    return fail(AF_ERR_INVALID, "RCCL not found: call af_comm_load(path) or set ASYNCFLOW_RCCL_LIB");
}
#define RCCL_TRY(expr)                                                                                   \
    do {                                                                                                 \
        const int r_ = (expr);                                                                           \
        if (r_ != 0)                                                                                     \
            return fail(AF_ERR_HIP, std::string(#expr) + ": " + (g_rccl.GetErrorString ? g_rccl.GetErrorString(r_) : "rccl error")); \
    } while (0)
}  // namespace

int af_comm_load(const char* path) {
    if (!path) return rccl_need();
    void* h = dlopen(path, RTLD_NOW | RTLD_LOCAL);
    if (!h) return fail(AF_ERR_INVALID, std::string("dlopen(") + path + "): " + dlerror());
    if (!rccl_bind(h, path)) return fail(AF_ERR_INVALID, std::string(path) + " does not export the RCCL entry points");
    return AF_OK;
}

int af_comm_unique_id(void* id_out) {
    if (!id_out) return fail(AF_ERR_INVALID, "NULL argument");
    if (int rc = rccl_need()) return rc;
    nccl_id_t id;
    RCCL_TRY(g_rccl.GetUniqueId(&id));
    std::memcpy(id_out, &id, sizeof id);
    return AF_OK;
}

int af_comm_init_rank(const void* id, int world_size, int rank, int device, void** comm_out) {
    if (!id || !comm_out || world_size <= 0 || rank < 0 || rank >= world_size) return fail(AF_ERR_INVALID, "bad communicator arguments");
    if (int rc = rccl_need()) return rc;
    HIP_TRY(hipSetDevice(device));
    nccl_id_t nid;
    std::memcpy(&nid, id, sizeof nid);
    void* comm = nullptr;
    RCCL_TRY(g_rccl.CommInitRank(&comm, world_size, nid, rank));
    *comm_out = comm;
    return AF_OK;
}

void af_comm_destroy(void* comm) {
    if (comm && g_rccl.ok()) (void)g_rccl.CommDestroy(comm);
}

int af_comm_count(void* comm, int* world_size_out, int* rank_out) {
    if (!comm) return fail(AF_ERR_INVALID, "NULL communicator");
    if (int rc = rccl_need()) return rc;
    if (!g_rccl.CommCount || !g_rccl.CommUserRank) return fail(AF_ERR_INVALID, "this RCCL exports neither ncclCommCount nor ncclCommUserRank");
    int n = 0, r = 0;
    RCCL_TRY(g_rccl.CommCount(comm, &n));
    RCCL_TRY(g_rccl.CommUserRank(comm, &r));
    if (world_size_out) *world_size_out = n;
    if (rank_out) *rank_out = r;
    return AF_OK;
}

int af_engine_gather(af_engine_t* e, void* comm, int world_size, const af_summary_t* local, const af_summary_t* out) {
    if (!e || !comm || !local || !out || world_size <= 0) return fail(AF_ERR_INVALID, "NULL argument");
    if (local->n_scenarios == 0) return fail(AF_ERR_INVALID, "empty shard");
    if (out->n_scenarios != local->n_scenarios * (uint32_t)world_size)
        return fail(AF_ERR_INVALID, "gathered.n_scenarios must be world_size * local.n_scenarios");
    if (e->plan_only) return fail(AF_ERR_NO_DEVICE, "planning-only engine (AF_DEVICE_PLAN_ONLY)");
    if (int rc = rccl_need()) return rc;
    HIP_TRY(hipSetDevice(e->device));
    const size_t n = local->n_scenarios;
    const uint32_t n_series = e->args.n_series;
    struct Part { const void* src; void* dst; size_t row_bytes; const char* what; };
    const Part parts[] = {
        {local->stats, out->stats, 8u * sizeof(double), "stats"},
        {local->rps, out->rps, (size_t)local->rps_buckets * sizeof(float), "rps"},
        {local->hist, out->hist, (size_t)local->hist_bins * sizeof(uint32_t), "hist"},
        {local->series_mean, out->series_mean, (size_t)n_series * sizeof(double), "series_mean"},
        {local->series_max, out->series_max, (size_t)n_series * sizeof(uint32_t), "series_max"},
    };
    for (const Part& p : parts)
        if ((p.src == nullptr) != (p.dst == nullptr)) return fail(AF_ERR_INVALID, std::string("local / gathered disagree on ") + p.what);
    if (out->rps_buckets != local->rps_buckets || out->hist_bins != local->hist_bins)
        return fail(AF_ERR_INVALID, "local / gathered row lengths differ");
    HIP_TRY(hipEventRecord(e->ev0, e->stream));
    RCCL_TRY(g_rccl.GroupStart());
    // (an error inside the group must not leave it open: every later collective of this thread would be queued
    // behind a GroupEnd that never comes -- record the first failure, always close the group, then report)
    int first_err = 0;
    const char* first_what = "";
    for (const Part& p : parts)
        if (p.src && p.row_bytes && first_err == 0) {
            first_err = g_rccl.AllGather(p.src, p.dst, n * p.row_bytes, /* ncclInt8 */ 0, comm, e->stream);
            first_what = p.what;
        }
    const int end_err = g_rccl.GroupEnd();
    if (first_err != 0)
        return fail(AF_ERR_HIP, std::string("ncclAllGather(") + first_what + "): " + (g_rccl.GetErrorString ? g_rccl.GetErrorString(first_err) : "rccl error"));
    RCCL_TRY(end_err);
    HIP_TRY(hipEventRecord(e->ev1, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e->ev0, e->ev1));
    e->stats.gather_ms = ms;
    return AF_OK;
}

int af_probe_store(int device, int pattern, uint32_t n_waves, uint64_t bytes_per_wave, uint32_t lanes, double* ms_out) {
    if (n_waves == 0 || bytes_per_wave < 1024u || pattern < 0 || pattern > 2) return fail(AF_ERR_INVALID, "bad probe arguments");
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return fail(AF_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= n_dev) return fail(AF_ERR_NO_DEVICE, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    const size_t words = (size_t)(bytes_per_wave / 4u) & ~size_t(3);
    uint32_t* buf = nullptr;
    HIP_TRY(hipMalloc((void**)&buf, (size_t)n_waves * words * 4u));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    HIP_TRY(hipEventRecord(e0, 0));
    if (pattern == 0) hipLaunchKernelGGL(af_probe_store_wide, dim3(n_waves), dim3(64), 0, 0, buf, words);
    else if (pattern == 1) hipLaunchKernelGGL(af_probe_store_pairs16, dim3(n_waves), dim3(64), 0, 0, buf, words, lanes ? (lanes > 64u ? 64u : lanes) : 57u);
    else hipLaunchKernelGGL(af_probe_store_rows48, dim3(n_waves), dim3(64), 0, 0, buf, words);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(e1, 0));
    HIP_TRY(hipDeviceSynchronize());
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    if (ms_out) *ms_out = ms;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipFree(buf);
    return AF_OK;
}

// Test hook: the scratch pool of `engine` becomes exactly `bytes` of `word` (0 bytes: no pool), and from now on every growth of
// the pool starts as `word` too, so that an analyzer which relies on what its scratch held before gives itself away.
int af_probe_scratch(af_engine_t* e, uint64_t bytes, uint32_t word) {
    if (!e) return fail(AF_ERR_INVALID, "NULL argument");
    if (e->plan_only) return fail(AF_ERR_NO_DEVICE, "a plan-only engine has no scratch");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->pool_poisoned = true;
    e->pool_word = word;
    if ((size_t)bytes != e->pool_cap) {
        if (e->d_pool) HIP_TRY(hipFree(e->d_pool));
        e->d_pool = nullptr;
        e->pool_cap = 0;
        if (bytes) {
            HIP_TRY(hipMalloc((void**)&e->d_pool, (size_t)bytes));
            e->pool_cap = (size_t)bytes;
        }
    }
    return pool_fill(e);
}

int af_probe_math(int device, int kind, uint64_t seed, const double* in, const double* in2, double* out, size_t n) {
    if (!in || !out || n == 0) return fail(AF_ERR_INVALID, "NULL argument");
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return fail(AF_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= n_dev) return fail(AF_ERR_NO_DEVICE, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    double *d_in = nullptr, *d_in2 = nullptr, *d_out = nullptr;
    HIP_TRY(hipMalloc((void**)&d_in, n * 8));
    HIP_TRY(hipMalloc((void**)&d_out, n * 8));
    HIP_TRY(hipMemcpy(d_in, in, n * 8, hipMemcpyHostToDevice));
    if (in2) {
        HIP_TRY(hipMalloc((void**)&d_in2, n * 8));
        HIP_TRY(hipMemcpy(d_in2, in2, n * 8, hipMemcpyHostToDevice));
    }
    hipLaunchKernelGGL(af_probe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, kind, seed, d_in, d_in2,
                       d_out, n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, d_out, n * 8, hipMemcpyDeviceToHost));
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    if (d_in2) (void)hipFree(d_in2);
    return AF_OK;
}

}  // extern "C"

#endif  // AF_JIT
