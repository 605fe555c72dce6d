// af_flow.hpp -- stage-parallel ("flow") kernel: ONE WAVE PER SCENARIO, 64 requests per step.
//
// Replaces, for plans whose request path is feed-forward, the same thing af_core.hpp replaces --
// `SimulationRunner.run()` -> `env.run(until=T)` of the reference
// (/root/reference/src/asyncflow/runtime/simulation_runner.py:349-376) -- but instead of popping one
// event per lane per round it moves a whole batch of requests through the stations of the path:
//
//   generator -> edge -> client (1st visit) -> edge -> [load balancer -> edge] -> server -> edge -> client (2nd visit)
//   rqs_generator.py:97-119  edge.py:73-116  client.py:43-71  load_balancer.py:60-72  server.py:79-276
//
// Why this is exact.  A station's state (edge send counter = index of the edge's next random draw, the
// LB rotation, a server's core / RAM / queues, the client's completion list) is only touched by the
// events AT that station, and every message carries its own times.  If no two events of one station
// share a timestamp, each station sees a uniquely ordered event sequence and the run is a
// deterministic dataflow: processing the stations one after the other over a time window gives the
// same f64 values as popping events one by one -- the same additions in the same order
// (deliver = send + (transit + spike), edge.py:94-107; core grant = max(ready time, previous release),
// server.py:210-231).  Per station the events of a window are put in time order by a bucket rank
// (exact comparisons on the f64 keys), which also finds equal keys.  Whatever the scheme cannot
// express -- two events of one station at the same instant, a RAM queue that would block, a list or
// tick-ring overflow -- sets FLAG_FLOW_FALLBACK and the scenario is simulated again, from t = 0, by the
// sequential next-event kernels (af_core.hpp), which follow SimPy's event-by-event order.
//
// Windowing.  Station s owns a list of messages whose delivery time is known but not yet final in
// rank; `H_s` is its horizon: every message the station will ever receive with time < H_s is already in
// the list.  H_generator = time of the next arrival not yet generated; H_s <= H_{s-1} because a
// message leaves a station no earlier than it arrived.  Each round every station ranks the messages
// with time < min(H_{s-1}, T), handles at most 64 of them (one per lane) and hands the results to the
// next list; what does not fit stays (back-pressure through the list capacities).
//
// Sampled series (collector.py:50-66): every counter the collector reads is a sum of intervals
// [event that increments, event that decrements) -- a message in transit on an edge, a request in the
// ready queue / in an I/O step / holding RAM.  Each end is entered as +w / -w at the first tick after
// it in a ring of per-tick differences (LDS).  The sending station knows both ends of a message's stay
// on an edge: it enters nothing when no tick lies between them, both when the ring reaches the
// delivery's row (fast hops: always), and otherwise only the send -- it marks the message (sign of
// t0) and the RECEIVING station enters the delivery when it handles it, i.e. at a time no station is
// allowed to pass in that round (t_lim).  The server's queue / step / RAM intervals are entered by the
// server station.  An entry therefore never lies ahead of the ring's window by more than a server
// sojourn, however slow the edges are.  Rows older than the slowest station's horizon are final:
// prefix-summed and streamed out.
//
// Device code under hipcc (wave backend: af_wave_hip in engine.hip); plain C++ under g++ for the
// TEST-ONLY 64-fibre wave emulator of tests/hostcheck/ (never shipped).
#pragma once

#include <stdint.h>

#include "af_core.hpp"

namespace aff {

using af::AF_INF;
using af::d2u;
using af::u2d;

enum : uint32_t {
    FLAG_FLOW_FALLBACK = 1u << 8,   // internal: never visible in the outputs of af_engine_run
    // reasons (af_stats_t.flow_fallback_*), bits 9..12 of the same word, cleared with the flag
    FLOW_WHY_TIE = 1u << 9,         // two events of one station (or an event and a tick / timeline mark) share an instant
    FLOW_WHY_LIST = 1u << 10,       // more messages pending at a station than the list holds
    FLOW_WHY_RING = 1u << 11,       // an interval reaches further ahead than the tick ring
    FLOW_WHY_RAM = 1u << 12,        // a request would have to wait for RAM
    // (bit 13: AF_FLAG_NEGATIVE_DELAY)
    FLOW_WHY_GEN_TIE = 1u << 15,    // the tie is one the general server station gives up on (an arrival exactly at a step end, two
                                    // responses at one instant): the second-chance instantiation would stop at the same instant, so
                                    // such a scenario goes straight to the next-event kernels; set together with FLOW_WHY_TIE
    FLOW_WHY_MASK = FLOW_WHY_TIE | FLOW_WHY_LIST | FLOW_WHY_RING | FLOW_WHY_RAM | FLOW_WHY_GEN_TIE,
};
constexpr uint32_t kMaxServers = 16;   // least connections: 16-bit in-flight counts of <= 16 servers in 64-bit words and their draws in registers (round 6: 8;
                                       // Flow::lb_pick_lc_n<8> still serves fan-outs of up to 8 with two words and eight draws)
// servers behind a round-robin LB: 16 slots per per-server array of lbw() (what binds first is the 64 sampled series a wave's
// lanes carry: 2 + 5 S series -> S <= 12)
constexpr uint32_t kSrvSlots = 16;
enum : uint32_t { LBW_ARRIVALS = 24u, LBW_SEG_OFF = LBW_ARRIVALS + kSrvSlots, LBW_SEG_LEN = LBW_SEG_OFF + kSrvSlots,
                  LBW_PROG = LBW_SEG_LEN + kSrvSlots, LBW_SLOTS = LBW_PROG + kSrvSlots, LBW_U32 = LBW_SLOTS + kSrvSlots };
static_assert(LBW_U32 % 2u == 0u, "lbw() is carved out of 64-bit words");

// LDS layout behind the plan blob, in 8-byte words; computed on the host (make_flow_layout).
struct FlowLayout {
    uint32_t cap;        // capacity of every station list (multiple of 64)
    uint32_t ring_rows;  // rows of the tick-difference ring (power of two)
    uint32_t win_rows;   // how many ticks past the completed ones the generator may run (the rest of the ring is for
                         // intervals that end later: the in-flight time of the slowest message)
    uint32_t g_ring;     // per-server ring of departure times (power of two >= RAM slots looked back)
    uint32_t c_ring;     // per-server ring of core-release times (power of two >= max cpu_cores)
    uint32_t pitch;      // 4-byte words per tick row (n_series rounded up to 4)
    uint32_t list_arrays;  // f64 arrays per station list: key, t0 [, send time (FEAT_TIEBREAK)]
    uint32_t off_spike, off_list, off_aux, off_aux3, off_out, off_sorted, off_hist, off_seg, off_fr, off_gr, off_cnt, off_ring;
    uint32_t n_words;
    // FEAT_BIGLIST: every list has its own capacity (a list behind a spiked edge holds rate x spike messages when the
    // spike ends); cap is then the largest of them
    uint32_t cap_of[4], off_list_of[4], off_eb;
    uint32_t off_gsrv;   // FEAT_GENSRV: per-server state of the general server station (kGsWords words each), else 0
};
// FEAT_GENSRV: per-server state, in 8-byte words (Flow::gen_servers)
constexpr uint32_t kGsSlots = 32u;   // requests inside one server at once (more: handed back)
constexpr uint32_t kGsDeps = 64u;   // departures of one server in one round: at most what was inside plus the round's arrivals, which run() keeps within 64 (the room of the server station's select)
enum : uint32_t { GS_CPU = 0u /* cpu_free | ready << 32 */, GS_IO = 1u /* io | free-slot mask << 32 */, GS_RAM = 2u /* f64 free RAM */,
                  GS_ARR = 3u /* arrivals | RAM queue blocked << 32 */, GS_CQ = 4u /* head | n << 32 */, GS_RQ = 5u, GS_EV = 6u, GS_DEP = 7u /* departures of this round | tie instants so far << 32 */,
                  GS_LAST = 8u /* f64 time of the server's previous event */, GS_LASTDEP = 9u /* f64 time of its previous departure */,
                  GS_T0 = 10u, GS_NEED = GS_T0 + kGsSlots, GS_STATE = GS_NEED + kGsSlots /* row | holds core << 16 | in I/O << 17 */,
                  GS_EVT = GS_STATE + kGsSlots /* sorted ring of pending step ends: time */, GS_BYTES = GS_EVT + kGsSlots /* 4 x kGsSlots bytes: event slots, CPU waiters, RAM waiters, where each pending step end was created */,
                  GS_DEPT = GS_BYTES + (4u * kGsSlots + 7u) / 8u, GS_DEPT0 = GS_DEPT + kGsDeps,
                  GS_MQ = GS_DEPT0 + kGsDeps /* kGsMq bytes: the zero-time steps queued at a shared instant (Flow::gs_instant) */, kGsWords = GS_MQ + 8u };
constexpr uint32_t kGsMq = 64u;   // zero-time steps queued at one instant of one server (more: handed back)

inline FlowLayout make_flow_layout(uint32_t cap, uint32_t ring_rows, uint32_t g_ring, uint32_t c_ring, uint32_t n_edges,
                                   uint32_t n_servers, uint32_t n_edge_marks, bool tiebreak = false,
                                   const uint32_t* caps4 = nullptr, bool general_servers = false) {
    FlowLayout L{};
    for (uint32_t s = 0; s < 4u; ++s) {
        L.cap_of[s] = caps4 ? caps4[s] : cap;
        if (caps4 && caps4[s] > cap) cap = caps4[s];
    }
    L.cap = cap;
    L.ring_rows = ring_rows;
    L.win_rows = ring_rows / 2u;
    L.g_ring = g_ring;
    L.c_ring = 1u;   // a power of two >= the widest server: the ring is indexed by a mask (a modulo by `cores` was 60 instructions per round)
    while (L.c_ring < c_ring) L.c_ring *= 2u;
    c_ring = L.c_ring;
    L.pitch = (n_edges + 3u * n_servers + 3u) & ~3u;
    uint32_t w = 0;
    L.off_spike = w; w += n_edge_marks;                 // cumulative spike after each edge mark
    L.list_arrays = tiebreak ? 3u : 2u;
    L.off_list = w;                                     // 4 lists x (key, t0 [, send time])
    for (uint32_t s = 0; s < 4u; ++s) {
        L.off_list_of[s] = w;
        w += L.list_arrays * L.cap_of[s];
    }
    L.off_aux = w; w += (L.cap_of[2] + 3u) / 4u;        // u16 per entry of the server list: server | in-edge << 8
    L.off_aux3 = w; w += (L.cap_of[3] + 3u) / 4u;       // ... and of the completion list: the server's out-edge
    // scratch of select() (selected (key, t0) + u32 aux; bucket-sorted keys; 64 u32 counts, 64 u32 bases, scalars)
    // and the per-server segments of the server station (admission, B, S, F, G) are never live together
    const uint32_t scratch0 = w;
    L.off_out = w; w += 64u * 2u + 32u;
    L.off_sorted = w; w += tiebreak ? 2u * cap : cap;   // bucket-sorted keys [, their send times]
    L.off_hist = w; w += 32u + 32u + 8u;
    L.off_eb = w; w += caps4 ? ((cap + 1u) / 2u > 64u || !general_servers ? (cap + 1u) / 2u : 64u) : 0u;    // FEAT_BIGLIST: u32 per entry (bucket | slot, then rank); FEAT_GENSRV: also the solver's 128 place ids (gen_servers_par)
    L.off_seg = scratch0;
    if (w < scratch0 + 5u * 64u) w = scratch0 + 5u * 64u;
    L.off_fr = w; w += n_servers * c_ring;
    L.off_gr = w; w += n_servers * g_ring;
    L.off_cnt = w; w += (n_edges + 1u) / 2u + LBW_U32 / 2u + 12u + 8u;   // u32 sends per edge; LBW_U32 u32: lb order, head, n_live, mark cursor, per-server counters; send_floor's 4 x 3 f64; 8 horizon slots (Flow::hz)
    L.off_ring = w; w += (ring_rows * L.pitch + 1u) / 2u;
    L.off_gsrv = general_servers ? w : 0u;
    if (general_servers) w += n_servers * kGsWords + 128u;   // (+ 128 words of the round-at-once solver: Flow::par_words)
    L.n_words = w;
    return L;
}

struct FlowArgs {
    // plan (shape + blob; the blob is af_plan_pack.hpp's, patched per scenario with the overrides)
    double total_time, sample_period, inv_period, tick_eps;
    uint32_t metrics_mask, gen_out_edge, client_out_edge;
    uint32_t n_edges, n_servers, has_lb, n_lb_edges, n_edge_marks, n_srv_marks;
    uint32_t lb_least_connections;   // 0 round robin, 1 least connections (needs a FEAT_LC instantiation)
    uint32_t max_pre, max_cpu, max_post;   // longest leading-I/O / CPU / trailing-I/O run over the servers' endpoints
    // ram_in_use is a sum of the requests' RAM needs; the tick ring holds integer differences.  Needs that are whole MB: scale 1;
    // dyadic fractions (multiples of 1/256 MB: 100.25, 400.5 -- their sums are exact in f64 in any order, like the
    // reference's += / -=): scale 256, and the value leaves the ring as (sum of differences) x ram_unit = 1 / ram_scale
    double ram_scale, ram_unit;
    uint32_t off_edge, off_srv, off_ep, off_row, off_emark, off_smark, off_lb;  // word offsets in the blob
    uint32_t blob_bytes;
    const unsigned char* blob;
    FlowLayout L;
    // ticks: tick_t[k] = time of tick k+1 (repeated f64 addition of the period, collector.py:50-53)
    const double* tick_t;
    uint32_t n_ticks;
    // sweep
    uint32_t n_scen;
    const uint64_t* seeds;
    uint32_t n_ovr;
    const uint32_t* ovr_param;
    const uint32_t* ovr_index;
    const double* ovr_values;
    uint32_t ovr_stride;
    // inputs: arrival times of every scenario (af_pregen_arrivals), [n_scen][n_draw], AF_INF behind the last
    const double* arrivals;
    uint32_t n_draw;
    const uint32_t* pre_flags;
    // outputs (same arrays as the sequential kernels)
    double* clock;
    uint32_t clock_cap;
    uint32_t* samples;
    uint32_t tick_cap;
    uint32_t* counts;
    uint32_t* online_hist;
    uint32_t* online_rps;
    uint32_t online_hist_bins, online_rps_buckets;
    double online_hist_scale;
    uint32_t* n_fallback;   // [5]: scenarios handed over, then by reason (tie, list, ring, ram)
    const uint32_t* scen_map;  // second-chance launch: wave j simulates scenario scen_map[j] (null = j)
    unsigned long long* prof;  // FEAT_PROF builds: [n_scen][kProfSections] shader-clock cycles per section of run()
};
// FEAT_PROF: where a wave's time goes (measurement builds only: AF_FLOW_PROF)
enum : uint32_t { PROF_SETUP, PROF_GEN, PROF_SELECT, PROF_SERIES_RECV, PROF_STATION, PROF_SERVERS, PROF_SERVER_SERIES, PROF_DRAW, PROF_SEND_SERIES,
                  PROF_APPEND, PROF_COMPLETE, PROF_FLUSH, PROF_PAR_SETUP, PROF_PAR_WALK, PROF_PAR_RANK, PROF_PAR_FINAL,
                  PROF_N_PAR_ROUNDS /* counts, not cycles */, PROF_N_PAR_ITERS, PROF_N_PAR_LANES, PROF_N_WALKED_ROUNDS, PROF_PAR_STANDING, PROF_PAR_COMMIT_WALK,
                  PROF_N_SELECT_WINDOW /* counts: select() calls ranked by the lane window / that fell back to the bucket rank */, PROF_N_SELECT_BUCKET, kProfSections = 24u };

// select()'s lane window (Flow::select_regs): an entry is compared with the AF_SELECT_WINDOW entries in front of it in list order
// where a prefix maximum proves that nothing further away is out of order.  0: always the bucket rank.
// (The width is measured, not reasoned -- host emulator, LB-2 at its own parameters: the proof holds in 96.4 / 99.7 / 100 / 100 %
// of calls at 4 / 6 / 8 / 12 lanes; on the device, config 2: 41.80 ms per step at 6, 42.75 at 8, 43.12 without the window --
// profiles/r08/ab_select_window.txt.  The plan-specialised builds switch it off per spec: engine.hip, flow_jit_spec_string.)
#ifndef AF_SELECT_WINDOW
#define AF_SELECT_WINDOW 6
#endif
// Round 9: the width per station list (list 0: what the generator sent, one edge's jitter on a sorted batch; lists 1 .. 3: the
// jitter of later edges on an order already disturbed).  -DAF_SELECT_WINDOW_S<list>=w on the command line comes first, then what
// the plan-specialised build was given for its plan (AF_FJ_SELECT_WINDOW_S<list>: engine.hip, flow_jit_spec_string), then
// AF_SELECT_WINDOW; AF_SELECT_WINDOW=0 switches the window off in every list whatever the others say (select_window_of).
#ifndef AF_SELECT_WINDOW_S0
#ifdef AF_FJ_SELECT_WINDOW_S0
#define AF_SELECT_WINDOW_S0 AF_FJ_SELECT_WINDOW_S0
#else
#define AF_SELECT_WINDOW_S0 AF_SELECT_WINDOW
#endif
#endif
#ifndef AF_SELECT_WINDOW_S1
#ifdef AF_FJ_SELECT_WINDOW_S1
#define AF_SELECT_WINDOW_S1 AF_FJ_SELECT_WINDOW_S1
#else
#define AF_SELECT_WINDOW_S1 AF_SELECT_WINDOW
#endif
#endif
#ifndef AF_SELECT_WINDOW_S2
#ifdef AF_FJ_SELECT_WINDOW_S2
#define AF_SELECT_WINDOW_S2 AF_FJ_SELECT_WINDOW_S2
#else
#define AF_SELECT_WINDOW_S2 AF_SELECT_WINDOW
#endif
#endif
#ifndef AF_SELECT_WINDOW_S3
#ifdef AF_FJ_SELECT_WINDOW_S3
#define AF_SELECT_WINDOW_S3 AF_FJ_SELECT_WINDOW_S3
#else
#define AF_SELECT_WINDOW_S3 AF_SELECT_WINDOW
#endif
#endif
constexpr uint32_t select_window_of(uint32_t s) {
    return (uint32_t)(AF_SELECT_WINDOW) == 0u ? 0u
           : s == 0u ? (uint32_t)(AF_SELECT_WINDOW_S0) : s == 1u ? (uint32_t)(AF_SELECT_WINDOW_S1) : s == 2u ? (uint32_t)(AF_SELECT_WINDOW_S2) : (uint32_t)(AF_SELECT_WINDOW_S3);
}
// (one width for all four: select() stays ONE copy of select_regs, as the library's loop over the stations needs it)
constexpr bool kSelectWindowUniform = select_window_of(0u) == select_window_of(1u) && select_window_of(1u) == select_window_of(2u) && select_window_of(2u) == select_window_of(3u);
#if !defined(__HIPCC__)
// host builds only: select_regs calls ranked by the window / handed on to the bucket rank (of the instantiations that have the
// window at all), for the stand-alone programs that drive the selection on crafted lists; [2], [3]: of the ranked ones, those that
// kept entries in the list / selected fewer than were eligible; and the first two per station list (how a width suits a list:
// profiles/r09/emulator_widths_per_list.txt)
inline unsigned long long g_select_window_calls[4] = {0ull, 0ull, 0ull, 0ull};
inline unsigned long long g_select_window_by_list[4][2] = {};
#endif

// ---- the algorithm, written against a wave backend W ---------------------------------------------
//   W::lane()                       0..63
//   W::ballot(bool) -> u64, W::any(bool)
//   W::shfl32(v, src) / W::shfl64(v, src)   value of lane `src` (per-lane src allowed)
//   W::sync()                       wave barrier + LDS visibility
//   W::lds_add(p, v) -> old         atomic add on an LDS word
//   W::global_add(p, v) / W::global_load(p) / W::global_fence()   device-scope atomic add / load past the L1 / fence
//                                   (tick differences kept in HBM when the LDS ring would be too small)
//   W::mbcnt(mask)                  popcount(mask & lanes below me)
//   W::rcp(x)                       ~1/x (only ever used where the exact value does not matter)
//   W::scan_incl_u32(v)             inclusive prefix sum over the lanes (DPP row shifts / broadcasts on the device)
//   W::bcast32 / bcast64(v, lane)   value of a WAVE-UNIFORM lane (v_readlane on the device)
//   device only (select()'s lane window; host builds make them from shfl32): W::scan_incl_max_u32(v) inclusive prefix maximum,
//                                   W::lane_below_u32(v) value of lane - 1 (0 in lane 0), W::my_bit(mask) bit `lane` of a wave-uniform mask
// Every W:: call is made by all 64 lanes from wave-uniform control flow.
// IPL = list entries per lane (list capacity = 64 * IPL).
// FEAT = features compiled in (the host picks the leanest instantiation that covers the launch: every
// feature costs wave-uniform registers, and the kernel is short of them -- DESIGN.md section 4e):
//   FEAT_MARKS     injected spikes / outages (the plan has timeline marks)
//   FEAT_ONLINE    kernel-side latency histogram / completion counts (af_outputs_t.online_*)
//   FEAT_HBM_RING  tick differences kept in the sample rows in HBM (layout.ring_rows == 0 with series stored)
//   FEAT_TIEBREAK  every message also carries its SEND time; two deliveries of one station at the same instant are
//                  then handled in the order SimPy pops them -- the order their Timeouts were created, i.e. by send
//                  time (heap key (time, priority, event id)) -- instead of being handed back.  Used by
//                  the second-chance launch over the scenarios the lean instantiation hands back (engine.hip).
//   FEAT_BIGLIST   lists of any length with their own capacities (FlowLayout::cap_of): select() walks a list in
//                  chunks of 64 at a cost proportional to what it holds, instead of keeping IPL entries per lane in
//                  registers.  For plans whose spikes pile up rate x spike messages at one station when they end.
//   FEAT_LC        least-connections load balancer (Flow::lb_pick_lc): the batch of the LB station is walked one
//                  message at a time by the whole wave
//   FEAT_FAR       edges slower than the LDS tick ring reaches: the sender enters only the send of such a message and
//                  marks it, the receiving station enters the delivery (file header, "Sampled series").  Without it the
//                  sender enters both ends and a delivery beyond the ring hands the scenario back.
//   FEAT_GENSRV    general servers (round 3): several endpoints per server (server.py:101), step programs that come back to the
//                  core queue after an I/O step, RAM needs that differ per request.  The order in which requests reach a
//                  server's queues is then no longer their arrival order, so the station cannot finalise an arrival when it
//                  sees it: lane k runs server k as a little sequential next-event loop of its own (sorted ring of pending
//                  step ends, FIFO of core waiters, FIFO of RAM waiters: Flow::gen_servers) up to the horizon of the station --
//                  every arrival before it is known --, servers side by side in the lanes, and the departures it produced are
//                  then sent by the whole wave like any other batch.  Two events of one server at one instant are handed back.
//   FEAT_CHAIN     servers that feed servers (round 4; graph.py:135-157 forbids fan-out except at the LB, not server -> server
//                  edges).  The servers are put in LEVELS (0: fed by the client / the LB only; k: its deepest feeding server is of
//                  level k - 1) and the server station runs once per level and round, in level order, over the ONE server list:
//                  a level's select() takes the entries whose target server is of that level, with the level's own horizon.
//                  Everything a server of level k receives before min(horizon of the station in front of the servers, send floor
//                  of every level below k) is in the list, because a request leaves a server no earlier than it arrived.  What a
//                  level sends goes to the completion list or back into the server list, lane by lane.  Tandem or general
//                  servers (FEAT_GENSRV: the event-by-event station runs the servers of the pass's level); behind a
//                  least-connections LB the walk counts the list entries that came by the LB's OWN edges.
//   FEAT_PROF      measurement builds only: the wave's shader-clock time per section of run() (FlowArgs::prof)
enum : uint32_t { FEAT_MARKS = 1u, FEAT_ONLINE = 2u, FEAT_HBM_RING = 4u, FEAT_FAR = 64u, FEAT_ALL = 7u | FEAT_FAR, FEAT_TIEBREAK = 8u,
                  FEAT_BIGLIST = 16u, FEAT_LC = 32u, FEAT_PROF = 128u, FEAT_GENSRV = 256u, FEAT_CHAIN = 512u };
constexpr uint32_t kMaxLevels = 5u;      // FEAT_CHAIN: server levels (af_flow_host.hpp refuses deeper plans); round 4: 3
constexpr uint32_t kAnyLevel = 0xFFu;    // select(): no level filter
template <class W, uint32_t IPL = 1u, uint32_t FEAT = FEAT_ALL>
struct Flow {
    static constexpr bool kMarks = (FEAT & FEAT_MARKS) != 0u, kOnline = (FEAT & FEAT_ONLINE) != 0u,
                          kHbmRing = (FEAT & FEAT_HBM_RING) != 0u, kTieBreak = (FEAT & FEAT_TIEBREAK) != 0u,
                          kBig = (FEAT & FEAT_BIGLIST) != 0u, kLC = (FEAT & FEAT_LC) != 0u, kFar = (FEAT & FEAT_FAR) != 0u,
                          kProf = (FEAT & FEAT_PROF) != 0u, kGen = (FEAT & FEAT_GENSRV) != 0u, kChain = (FEAT & FEAT_CHAIN) != 0u;
    static_assert(!(kChain && kLC) || kFar, "server levels behind a least-connections LB: list entries carry their in-edge (FEAT_FAR)");
    // FEAT_PROF: the time since the previous mark belongs to `section` (marks sit at the END of a section, in
    // wave-uniform control flow, with a compile-time section: the accumulators stay in scalar registers)
    unsigned long long prof_t, prof_acc[kProfSections];
    AF_CORE void prof(uint32_t section) {
        if (kProf) {
            const unsigned long long t = W::clock();
#pragma unroll
            for (uint32_t k = 0u; k < kProfSections; ++k)
                if (k == section) prof_acc[k] += t - prof_t;
            prof_t = t;
        }
    }
    const FlowArgs& A;
    AF_PLAN_AS uint64_t* blob;   // plan blob (LDS copy, patched)
    AF_PLAN_AS uint64_t* M;      // layout words behind it
    uint32_t lane;
    uint64_t seed;

    // uniform state (identical in every lane)
    uint32_t cursor;             // arrivals generated so far
    // messages pending at client-1st / LB / server / client-2nd and their horizons: named scalars behind
    // accessors (an array indexed by the station would live in scratch memory)
    uint32_t nl0, nl1, nl2, nl3;
    double h0, h1, h2, h3;
    AF_CORE uint32_t n_list_get(uint32_t s) const { return s == 0u ? nl0 : s == 1u ? nl1 : s == 2u ? nl2 : nl3; }
    AF_CORE void n_list_set(uint32_t s, uint32_t v) {
        if (s == 0u) nl0 = v; else if (s == 1u) nl1 = v; else if (s == 2u) nl2 = v; else nl3 = v;
    }
    // horizon slots: 0..3 = the four lists' stations; FEAT_CHAIN: 4 .. 7 = the server station of levels 1 .. 4 (level 0 is slot 2)
    double h2b, h2c, h2d, h2e;
    uint32_t n_levels;           // FEAT_CHAIN: levels the plan's servers form (wave-uniform), else 1
    uint32_t lb_pos, lb_in_edge; // FEAT_CHAIN: the LB station runs in front of the servers of this level (0: right behind the client); the edge it receives by
    AF_CORE static constexpr uint32_t level_slot(uint32_t level) { return level == 0u ? 2u : 3u + level; }
    // The generic FEAT_CHAIN instantiations walk the stations in a LOOP, so the slot is a run-time value there -- and a select
    // over eight members of this object makes the compiler address the object indirectly, which puts ALL of it (912 B per lane)
    // in scratch memory: round 4's generic tiers ran at 437 ms against 66 ms for the plan-specialised build, which unrolls the
    // stations.  Those forms keep the horizons in eight LDS words behind send_floor's cache instead (round 5).
#if defined(AF_FLOW_JIT) && !defined(AF_FLOW_LOOP_STATIONS)
    static constexpr bool kStationsUnrolled = true;
#else
    static constexpr bool kStationsUnrolled = false;
#endif
    static constexpr bool kHzLds = kChain && !kStationsUnrolled;
    AF_CORE AF_PLAN_AS double* hz() const { return fcache() + 12; }
    AF_CORE double H_get(uint32_t s) const {
        if (kHzLds) return hz()[s];
        if (kChain && s >= 4u) return s == 4u ? h2b : s == 5u ? h2c : s == 6u ? h2d : h2e;
        return s == 0u ? h0 : s == 1u ? h1 : s == 2u ? h2 : h3;
    }
    AF_CORE void H_set(uint32_t s, double v) {
        if (kMarks) moved = moved || v > H_get(s);   // (without lookahead the last horizon is the slowest: run() watches h3)
        if (kHzLds) {
            hz()[s] = v;   // (every lane stores the same value)
            return;
        }
        if (kChain && s >= 4u) {
            if (s == 4u) h2b = v; else if (s == 5u) h2c = v; else if (s == 6u) h2d = v; else h2e = v;
            return;
        }
        if (s == 0u) h0 = v; else if (s == 1u) h1 = v; else if (s == 2u) h2 = v; else h3 = v;
    }
    // FEAT_CHAIN: a server's level, one byte per server in lbw()[20..23] (written once by run())
    AF_CORE AF_PLAN_AS uint8_t* srv_levels() const { return (AF_PLAN_AS uint8_t*)(lbw() + 20); }
    AF_CORE uint32_t level_of(uint32_t sv) const { return srv_levels()[sv]; }
    uint32_t n_comp, tick_base;
    double gen_pre;              // arrival time cursor + lane, fetched ahead (AF_INF behind the last draw)
    // send counter of edge e = index of its next random draw: in the REGISTER of lane e (round 4; n_edges <= 64 sampled series).
    // A wave-uniform edge is read with v_readlane, a per-lane one through the crossbar; the LDS words of sends() are unused.
    uint32_t my_sends;
    AF_CORE uint32_t sends_of(uint32_t e_uniform) const { return W::bcast32(my_sends, e_uniform); }
    double t_lim;                // FEAT_FAR: no station handles an event at or after this time in the current round (the tick ring's window)
    bool gen_done, moved;        // moved: a horizon advanced in this round
    // per-lane accumulators (reduced at the end)
    uint32_t ev, drops, why, info;   // info: informational result flags
    int32_t run_val, run_val2;   // lane s: current value of sampled series s and of series s + 64

    const double* arr;
    double* clock;
    uint32_t* samples;
    uint32_t* o_hist;
    uint32_t* o_rps;

    AF_CORE Flow(const FlowArgs& a) : A(a) {}

    // ---- LDS views ----------------------------------------------------------------------------
    // Register-resident lists have 64 * IPL entries: everything up to the per-server rings then sits at a compile-time
    // distance from the lists (make_flow_layout's own arithmetic; run() checks it in the host builds), and every offset that
    // is not loaded from the arguments is one wave-uniform register less in a kernel that spills them.
    // (Measured, not reasoned: the register allocation of this kernel is chaotic.  FEAT_FAR / MARKS | FAR instantiations
    // -2 % -- configs 3, 4, 5 --, the plain lean one +0.6 % with 224 instead of 153 static v_readlanes: it keeps loading.)
    static constexpr bool kCt = !kBig && !kTieBreak && FEAT != 0u;
    static constexpr uint32_t kCap = 64u * IPL, kAuxW = (kCap + 3u) / 4u;
    static constexpr uint32_t kBigRegIpl = 2u;   // FEAT_BIGLIST: lists of up to 128 entries are ranked out of registers (select_big)
    AF_CORE uint32_t o_list() const { return (kCt && !kMarks) ? 0u : A.L.off_list; }   // (no marks: no spike table in front)
    AF_CORE uint32_t o_aux() const { return kCt ? o_list() + 8u * kCap : A.L.off_aux; }
    AF_CORE uint32_t o_aux3() const { return kCt ? o_aux() + kAuxW : A.L.off_aux3; }
    AF_CORE uint32_t o_out() const { return kCt ? o_aux3() + kAuxW : A.L.off_out; }
    AF_CORE uint32_t o_sorted() const { return kCt ? o_out() + 160u : A.L.off_sorted; }
    AF_CORE uint32_t o_hst() const { return kCt ? o_sorted() + kCap : A.L.off_hist; }
    AF_CORE uint32_t o_fr() const { return kCt ? o_out() + (kCap + 232u > 320u ? kCap + 232u : 320u) : A.L.off_fr; }
    AF_CORE uint32_t cap_of(uint32_t s) const { return kBig ? A.L.cap_of[s] : kCt ? kCap : A.L.cap; }
    AF_CORE AF_PLAN_AS double* list_key(uint32_t s) const {
        return (AF_PLAN_AS double*)(M + (kBig ? A.L.off_list_of[s] : o_list() + (kTieBreak ? 3u : 2u) * cap_of(0u) * s));
    }
    AF_CORE AF_PLAN_AS double* list_t0(uint32_t s) const { return list_key(s) + cap_of(s); }
    AF_CORE AF_PLAN_AS double* list_ts(uint32_t s) const { return list_key(s) + 2u * cap_of(s); }   // FEAT_TIEBREAK only
    AF_CORE AF_PLAN_AS uint32_t* eb() const { return (AF_PLAN_AS uint32_t*)(M + A.L.off_eb); }       // FEAT_BIGLIST only
    AF_CORE AF_PLAN_AS double* sorted_ts() const { return sorted() + A.L.cap; }   // (cap: the largest list)
    AF_CORE AF_PLAN_AS uint16_t* list_aux(uint32_t s = 2u) const { return (AF_PLAN_AS uint16_t*)(M + ((kFar && s == 3u) ? o_aux3() : o_aux())); }   // lists 2 and (FEAT_FAR) 3
    AF_CORE AF_PLAN_AS double* out_key() const { return (AF_PLAN_AS double*)(M + o_out()); }
    AF_CORE AF_PLAN_AS double* out_t0() const { return out_key() + 64; }
    AF_CORE AF_PLAN_AS uint32_t* out_aux() const { return (AF_PLAN_AS uint32_t*)(M + o_out() + 128u); }
    AF_CORE AF_PLAN_AS double* sorted() const { return (AF_PLAN_AS double*)(M + o_sorted()); }
    AF_CORE AF_PLAN_AS uint32_t* hist() const { return (AF_PLAN_AS uint32_t*)(M + o_hst()); }
    AF_CORE AF_PLAN_AS uint32_t* bbase() const { return hist() + 64; }
    AF_CORE AF_PLAN_AS double* scal() const { return (AF_PLAN_AS double*)(M + o_hst() + 64u); }   // [8] scalars
    AF_CORE AF_PLAN_AS double* seg(uint32_t which) const { return (AF_PLAN_AS double*)(M + o_out()) + 64u * which; }   // (aliases select()'s scratch)
    AF_CORE AF_PLAN_AS double* fr(uint32_t sv) const { return (AF_PLAN_AS double*)(M + o_fr()) + sv * A.L.c_ring; }
    AF_CORE AF_PLAN_AS double* gr(uint32_t sv) const { return (AF_PLAN_AS double*)(M + A.L.off_gr) + sv * A.L.g_ring; }
    AF_CORE AF_PLAN_AS uint32_t* sends() const { return (AF_PLAN_AS uint32_t*)(M + A.L.off_cnt); }
    AF_CORE AF_PLAN_AS uint32_t* lbw() const { return sends() + ((A.n_edges + 1u) & ~1u); }  // [0..15] order, 16 head, 17 n_live, 18 mark cursor, 19 ceil(2^32 / n_live), 20..23 FEAT_CHAIN: a level byte per server, then kSrvSlots each: LBW_ARRIVALS per server, LBW_SEG_OFF / LBW_SEG_LEN segment start / length, LBW_PROG step counts (leading I/O | CPU << 8 | trailing I/O << 16), LBW_SLOTS RAM slots (requests that fit at once)
    AF_CORE AF_PLAN_AS double* fcache() const { return (AF_PLAN_AS double*)(M + A.L.off_cnt + (A.n_edges + 1u) / 2u + LBW_U32 / 2u); }   // [4][3], send_floor
    AF_CORE AF_PLAN_AS int32_t* ring() const { return (AF_PLAN_AS int32_t*)(M + A.L.off_ring); }
    AF_CORE AF_PLAN_AS double* spike_cum() const { return (AF_PLAN_AS double*)(M + A.L.off_spike); }

    AF_CORE const AF_PLAN_AS uint64_t* erec(uint32_t e) const { return blob + A.off_edge + af::EREC * e; }
    AF_CORE const AF_PLAN_AS uint64_t* emark(uint32_t i) const { return blob + A.off_emark + af::MREC * i; }
    AF_CORE const AF_PLAN_AS uint64_t* smark(uint32_t i) const { return blob + A.off_smark + af::NREC * i; }

    // ---- small wave helpers ---------------------------------------------------------------------
    AF_CORE static uint32_t popc64(uint64_t m) { return (uint32_t)__builtin_popcountll(m); }
    AF_CORE double bcast_f64(double v, uint32_t src) const { return u2d(W::bcast64(d2u(v), src)); }   // src wave-uniform
    AF_CORE uint32_t excl_scan(uint32_t v, uint32_t& total) const {
        const uint32_t inc = W::scan_incl_u32(v);
        total = W::bcast32(inc, 63u);
        return inc - v;
    }
    AF_CORE uint32_t wave_sum(uint32_t v) const {
#pragma unroll
        for (uint32_t d = 1u; d < 64u; d <<= 1) v += W::shfl32(v, lane ^ d);
        return v;
    }
    AF_CORE uint32_t wave_or(uint32_t v) const {
#pragma unroll
        for (uint32_t d = 1u; d < 64u; d <<= 1) v |= W::shfl32(v, lane ^ d);
        return v;
    }

    // ---- ticks ------------------------------------------------------------------------------------
    // number of ticks strictly before x, clipped to n_ticks (tick k = 1.. at tick_t[k-1]): floor(x / period) when x is
    // safely between two ticks, else a look-up in the table of the collector's own tick times.
    // ONE divergent region (round 4: 43.45 -> 41.94 ms on BASELINE config 2): the fractional part straight from v_fract_f64
    // (= q - floor(q), exact for q >= 0: no u32 -> f64 conversion and subtraction) and no early return -- x = +0 has fraction
    // 0 and goes through the table (which answers 0), an event beyond the last tick is clamped to N + 1.5 (fraction 0.5:
    // row N at once), a NaN too.  (Round 3 had measured the opposite -- two early returns beat clamps, 48.5 vs 50.1 ms -- with
    // the fraction worked out as q - (double)(uint32_t)q and three more compares.)
    AF_CORE uint32_t tick_index(double x, bool flag_ties) {
        const uint32_t N = A.n_ticks;
        const double q0 = x * A.inv_period, top = (double)N + 1.5;
        const double q = q0 < top ? q0 : top;
        const uint32_t g0 = q > 0.0 ? (uint32_t)q : 0u, g = g0 < N ? g0 : N;
        const double frac = W::fract(q);
        if (frac > A.tick_eps && frac < 1.0 - A.tick_eps) return g;   // safely between two ticks
        return tick_lookup(x, g, flag_ties);                          // next to a tick
    }
    // (behind a call: one event in ~1e8 lies this close to a tick, and the two table walks were 550 of the unrolled kernel's
    // 4 700 instructions -- 42 at each of tick_index's 13 inlined sites; bit 31 of the result: the event is AT a tick)
    AF_CORE uint32_t tick_lookup(double x, uint32_t g, bool flag_ties) {
        const uint32_t r = cold_tick_lookup(A.tick_t, A.n_ticks, x, g);
        if (flag_ties && (r >> 31)) why |= FLOW_WHY_TIE;
        return r & 0x7FFFFFFFu;
    }
    AF_CORE_NOINLINE static uint32_t cold_tick_lookup(const double* tick_t, uint32_t N, double x, uint32_t g) {
        while (g < N && tick_t[g] < x) ++g;
        while (g > 0u && tick_t[g - 1u] >= x) --g;
        return g | ((g < N && tick_t[g] == x) ? 0x80000000u : 0u);
    }
    // the counter of `series` changes by w at the first tick after an event: tick row `row` (tick_index of the event's
    // time).  Differences go to the LDS ring, or -- ring_rows == 0 -- straight into the scenario's (zeroed) rows of the
    // sample array in HBM, which flush_ticks() then prefix-sums in place.
    // (`on`: the caller's own condition, folded into the one divergent region around the atomic -- every region costs the
    // wave a handful of scalar instructions, and this is called ten times per request)
    AF_CORE void add_point(uint32_t series, uint32_t row, int32_t w, bool on = true) {
        const uint32_t R = A.L.ring_rows, N = A.n_ticks < A.tick_cap ? A.n_ticks : A.tick_cap;
        const bool in = on && row < N;
        if (kHbmRing && R == 0u) {
            if (in) W::global_add(samples + (size_t)row * A.L.pitch + series, (uint32_t)w);
            return;
        }
        const bool reach = row - tick_base < R;
        why |= (in && !reach) ? FLOW_WHY_RING : 0u;
        if (in && reach) W::lds_add((AF_PLAN_AS uint32_t*)(ring() + (row & (R - 1u)) * A.L.pitch + series), (uint32_t)w);
    }
    // the counter of `series` is larger by w during [a, b)
    AF_CORE void add_interval(uint32_t series, double a, double b, int32_t w) {
        const uint32_t ia = tick_index(a, true), ib = tick_index(b, true);
        add_span(series, ia, ib, w);
    }
    // ... is larger by w between the events whose tick rows are ia and ib (nothing to enter when no tick lies between)
    AF_CORE void add_span(uint32_t series, uint32_t ia, uint32_t ib, int32_t w, bool on = true) {
        const bool span = on && ia != ib;
        add_point(series, ia, w, span);
        add_point(series, ib, -w, span);
    }
    // rows [tick_base, upto) are final: prefix-sum the differences and stream the rows out
    // (a lane carries the running value of series `lane` and -- plans with more than 64 series: 13 .. 16 servers behind a
    // round-robin load balancer, round 5 -- of series `lane + 64` in run_val2)
    AF_CORE void series_kind(uint32_t ser, bool& on, bool& is_ram) const {
        const uint32_t n_series = A.n_edges + 3u * A.n_servers;
        constexpr uint32_t all = af::METRIC_READY | af::METRIC_IO | af::METRIC_RAM;
        const bool is_srv = ser >= A.n_edges && ser < n_series;
        is_ram = is_srv && (ser - A.n_edges) % 3u == 2u;
        on = ser < A.n_edges ? (A.metrics_mask & af::METRIC_EDGE) != 0u : (is_srv && (A.metrics_mask & all) == all);
    }
    AF_CORE uint32_t series_word(int32_t value, bool on, bool is_ram) const {
        if (!on) return 0u;
        return is_ram ? __builtin_bit_cast(uint32_t, (float)((double)value * A.ram_unit)) : (uint32_t)value;
    }
    AF_CORE void flush_ticks(uint32_t upto) {
        if (samples != nullptr) {
            const uint32_t R = A.L.ring_rows, pitch = A.L.pitch;
            const uint32_t stop = upto < A.tick_cap ? upto : A.tick_cap;
            if (pitch <= 32u && !(kHbmRing && R == 0u)) {
                // several rows per step: lane = (row q of the step, series): the rows of a step are one contiguous store
                // (5 rows = 240 B for LB-2 instead of five 48-byte stores), the running values of the series come from the
                // lanes of row 0 and go back there from the step's last row
                const uint32_t rpi = 64u / pitch;                                             // rows per step (2 .. 16)
                const uint32_t q = (lane * (65536u / pitch + 1u)) >> 16, ser = lane - q * pitch;   // lane / pitch, lane % pitch
                bool s_on, s_ram;
                series_kind(ser, s_on, s_ram);
                // (measured, round 4: letting only FULL steps leave before the end of the run -- ~8.6 rows become final per round of
                // LB-2, i.e. two steps of five, the second mostly empty -- gains nothing: 37.74 vs 37.93 ms)
                for (uint32_t r0 = tick_base; r0 < stop; r0 += rpi) {
                    const uint32_t rr = r0 + q, n_rows = stop - r0 < rpi ? stop - r0 : rpi;
                    const bool valid = q < n_rows;
                    int32_t acc = 0;
                    if (valid) {
                        AF_PLAN_AS int32_t* cell = ring() + (rr & (R - 1u)) * pitch + ser;
                        acc = *cell;
                        *cell = 0;
                    }
                    const int32_t d = acc;
                    for (uint32_t k = 1u; k < rpi; ++k) {   // inclusive sum over the rows above, same series
                        const int32_t up = (int32_t)W::shfl32((uint32_t)d, (lane - k * pitch) & 63u);
                        if (q >= k) acc += up;
                    }
                    const int32_t value = (int32_t)W::shfl32((uint32_t)run_val, ser) + acc;
                    if (valid) samples[(size_t)rr * pitch + ser] = series_word(value, s_on, s_ram);
                    const int32_t last = (int32_t)W::shfl32((uint32_t)value, ((n_rows - 1u) * pitch + lane) & 63u);
                    if (lane < pitch) run_val = last;
                }
            } else {
                // one row per lane set, the differences of kRows rows fetched before the first of them is summed: one latency (HBM
                // for differences kept in the sample rows -- config 5's round-2 form, -2.5 % --, LDS for the ring) per kRows rows
                // instead of one per row.  (Round 5: the row-by-row loop over the LDS ring was 17 % of config 5's kernel, ~290
                // cycles per row at two waves per SIMD.)
#if defined(AF_FLUSH_ROWS)
                constexpr uint32_t kRows = AF_FLUSH_ROWS;
#else
                constexpr uint32_t kRows = 8u;
#endif
                const bool in_hbm = kHbmRing && R == 0u;
#pragma unroll
                for (uint32_t half = 0u; half < 2u; ++half) {
                    const uint32_t ser = lane + 64u * half;
                    if (half == 1u && pitch <= 64u) break;   // (wave-uniform)
                    int32_t& value = half == 0u ? run_val : run_val2;
                    bool on, is_ram;
                    series_kind(ser, on, is_ram);
                    // (round 6: whole chunks first, with the row numbers in SCALAR registers and one divergent region per chunk -- the
                    // rows' own `r < stop` tests were vector compares and a branch each: ~23 instructions per row of config 5's 44
                    // series, 14 % of that kernel)
                    uint32_t r0 = W::bcast32(tick_base, 0u);
                    const uint32_t stop_u = W::bcast32(stop, 0u);
                    for (; r0 + kRows <= stop_u; r0 += kRows) {
                        if (ser < pitch) {
                            int32_t d[kRows];
#pragma unroll
                            for (uint32_t u = 0u; u < kRows; ++u)
                                d[u] = in_hbm ? (int32_t)W::global_load(samples + (size_t)(r0 + u) * pitch + ser) : ring()[((r0 + u) & (R - 1u)) * pitch + ser];
#pragma unroll
                            for (uint32_t u = 0u; u < kRows; ++u) {
                                if (!in_hbm) ring()[((r0 + u) & (R - 1u)) * pitch + ser] = 0;
                                value += d[u];
                                samples[(size_t)(r0 + u) * pitch + ser] = series_word(value, on, is_ram);
                            }
                        }
                    }
                    if (r0 < stop_u && ser < pitch) {   // (the rows left over: fewer than kRows, a scalar test each)
                        const uint32_t n_left = stop_u - r0;
                        int32_t d[kRows];
#pragma unroll
                        for (uint32_t u = 0u; u < kRows; ++u) {
                            d[u] = 0;
                            if (u < n_left) d[u] = in_hbm ? (int32_t)W::global_load(samples + (size_t)(r0 + u) * pitch + ser) : ring()[((r0 + u) & (R - 1u)) * pitch + ser];
                        }
#pragma unroll
                        for (uint32_t u = 0u; u < kRows; ++u)
                            if (u < n_left) {
                                if (!in_hbm) ring()[((r0 + u) & (R - 1u)) * pitch + ser] = 0;
                                value += d[u];
                                samples[(size_t)(r0 + u) * pitch + ser] = series_word(value, on, is_ram);
                            }
                    }
                }
            }
        }
        tick_base = upto;
    }

    // ---- edges --------------------------------------------------------------------------------------
    // cumulative spike of edge e seen by a message sent at `now` (injection.py:191-198: marks applied
    // strictly before `now`; a mark AT `now` is a tie)
    // (round 4: only the marks of THIS edge are walked -- a bit per mark in the edge's word of sends(), which the send
    // counters no longer use, written by run() -- instead of all marks of the plan: config 4 has six marks on three of
    // its six edges, so the walk is two steps for a spiked edge and none for the others)
    AF_CORE double spike_at(uint32_t e, double now) {
        double sp = 0.0;
        if (A.n_edge_marks <= 32u) {
            for (uint32_t m = sends()[e]; m != 0u; m &= m - 1u) {   // marks are in time order: the last one before `now` wins
                const uint32_t i = (uint32_t)__builtin_ctz(m);
                const double tm = u2d(emark(i)[0]);
                if (tm < now) sp = spike_cum()[i];
                else if (tm == now) why |= FLOW_WHY_TIE;
            }
            return sp;
        }
        for (uint32_t i = 0u; i < A.n_edge_marks; ++i) {
            const double tm = u2d(emark(i)[0]);
            if ((uint32_t)emark(i)[2] != e) continue;
            if (tm < now) sp = spike_cum()[i];
            else if (tm == now) why |= FLOW_WHY_TIE;
        }
        return sp;
    }
    // Earliest delivery time of anything station `st` sends from `h` on (it has sent everything before h): h plus
    // the spike its out-edges carry then, or a later mark's time plus the spike left after it.  A spike of s seconds
    // lets the next station run s seconds AHEAD of this one instead of piling up s seconds' worth of messages it may
    // not touch yet (conservative lookahead; f64 addition is monotone, so now >= h gives key >= the floor bit for bit).
    // `cached` = false: work it out afresh and leave the station's cache alone (FEAT_CHAIN: the server levels call this with
    // three different horizons per round, and the cache belongs to ONE non-decreasing sequence of them)
    AF_CORE double send_floor(uint32_t st, double h, bool cached = true) {
        if (!(kMarks && A.n_edge_marks != 0u) || !(h < AF_INF)) return h;
        if (kLC && st == 2u) return h;   // lb_pick_lc counts the server list as "everything not delivered before t"
        // per station: [0] the next mark of its out-edges at or after the h this was worked out for, [1] the smallest
        // spike its out-edges carry until then, [2] the smallest (mark time + spike left after it) over the later marks
        AF_PLAN_AS double* c = fcache() + 3u * st;
        double until = c[0], sp_min = c[1], cand = c[2];
        if (!cached || !(h < until)) {   // h passed a mark (or first call: the words start at 0): walk the marks again
            until = cand = sp_min = AF_INF;
            const uint32_t n_out = st == 2u ? A.n_lb_edges : st == 3u ? A.n_servers : 1u;
            for (uint32_t k = 0u; k < n_out; ++k) {
                const uint32_t e = st == 0u   ? A.gen_out_edge
                                   : st == 1u ? A.client_out_edge
                                   : st == 2u ? (uint32_t)blob[A.off_lb + k]
                                              : (uint32_t)(blob[A.off_srv + af::SREC * k + 1u] >> 16) & 0xFFFFu;
                double sp = 0.0;
                for (uint32_t i = 0u; i < A.n_edge_marks; ++i) {   // marks are in time order
                    if ((uint32_t)emark(i)[2] != e) continue;
                    const double tm = u2d(emark(i)[0]), after = spike_cum()[i];
                    if (tm < h) {
                        sp = after;
                    } else {
                        until = tm < until ? tm : until;
                        cand = tm + after < cand ? tm + after : cand;
                    }
                }
                sp_min = sp < sp_min ? sp : sp_min;
            }
            if (cached && lane == 0u) {   // (read again a round later at the earliest: many W::sync() in between)
                c[0] = until;
                c[1] = sp_min;
                c[2] = cand;
            }
        }
        const double fl = h + sp_min;
        return fl < cand ? fl : cand;
    }
    AF_CORE_NOINLINE static double cold_variate(uint32_t dist, double mean, double sigma, double u1, uint64_t seed, uint32_t stream,
                                                uint32_t idx) {
        return af::variate_from_u1(dist, mean, sigma, u1, seed, stream, idx);
    }
    // the draws of the idx-th message of edge e (af::pre_edge_draw, edge.py:78-90): false = dropped, else its transit
    // time; the exponential law -- the reference's default -- inline and the other laws behind one call
    AF_CORE bool edge_draw(uint32_t e, uint32_t idx, double& transit) const {
        const AF_PLAN_AS uint64_t* r = erec(e);
        const double mean = u2d(r[0]), sigma = u2d(r[1]);
        const uint32_t stream = af::stream_edge(e);
#if defined(__HIP_DEVICE_COMPILE__) && defined(AF_FJ_KEYS_PER_CALL)
        // The seed is the wave's (one scenario per wave), so Philox's key schedule -- seed + r x the Weyl constants -- is scalar
        // work.  Left alone the compiler makes twenty loop-invariant scalar registers of it, more than it has: part of them live
        // in the lanes of a vector register and come back through v_readlane, a VALU slot each, in a kernel bound by VALU issue.
        // The empty asm makes the seed opaque at every call site: ten pairs of s_add per draw instead (config 2: 63 -> 45
        // v_readlane, 1 903 -> 1 869 VALU instructions).  A plan-specialised build asks for it where it was measured to pay
        // (engine.hip: flow_jit_spec_string); the register allocation of this kernel is chaotic, and it does not everywhere.
        uint32_t sd_lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)seed), sd_hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(seed >> 32));
        asm volatile("" : "+s"(sd_lo), "+s"(sd_hi));
        const af::U4 rr = af::draw_block(((uint64_t)sd_hi << 32) | sd_lo, stream, idx, 0u);
#else
        const af::U4 rr = af::draw_block(seed, stream, idx, 0u);
#endif
        // dropped (edge.py:78-86)?  u < dropout_rate with u = k x 2^-53, k the draw's 53 bits: the same test on integers,
        // k < ceil(dropout x 2^53) -- run() turned the blob's dropout word into that threshold -- without the two u32 -> f64
        // conversions, the multiply-add and the scaling of af::u53 (round 4)
        const uint64_t k53 = ((uint64_t)(rr.x >> 5) << 26) | (uint64_t)(rr.y >> 6);
        const bool sent = !(k53 < r[2]);   // (the latency draw is worked out all the same: one region less)
        // (the exponential law takes 1 - u1 straight from the 53 bits: one fma on the device, af::one_minus_unit_of)
        const double K1 = af::k53(rr.z, rr.w);
#if defined(AF_FJ_DIST_ALL) && (AF_FJ_DIST_ALL != 255)
        // plan-specialised build of a plan whose edges all follow ONE law: the law is a constant, its variate code is
        // inlined and the call (with the registers it pins around the call site) is gone
        transit = af::test_quant(AF_FJ_DIST_ALL == af::DIST_EXPONENTIAL ? -(mean * af::af_log_unit(af::one_minus_unit_of(K1)))
                                                                        : af::variate_from_u1(AF_FJ_DIST_ALL, mean, sigma, af::unit_of(K1), seed, stream, idx));
#else
        const uint32_t dist = (uint32_t)(r[3] >> 16) & 0xFFu;
        transit = af::test_quant(dist == af::DIST_EXPONENTIAL ? -(mean * af::af_log_unit(af::one_minus_unit_of(K1)))
                                                              : cold_variate(dist, mean, sigma, af::unit_of(K1), seed, stream, idx));
#endif
        return sent;
    }
    // EdgeRuntime._deliver (edge.py:73-116) for the idx-th message of edge e, sent at `now`.
    // Returns false if the message is dropped; else `key` = delivery time.
    // `pre`: the draws were made earlier (lb_pick_lc): `pre_transit` < 0 = dropped.
    // Sampled series, FEAT_FAR: `row_now` = tick row of `now` (worked out by the caller); `counted` = only the send was
    // entered in the edge's series, the receiving station enters the delivery.  Otherwise both ends are entered here.
    // (two steps: send_draw -- dropped? transit time -- and, for the messages that were sent, send_finish)
    AF_CORE bool send_draw(uint32_t e, uint32_t idx, double& transit, bool pre = false, double pre_transit = 0.0) {
        transit = pre_transit;
        const bool sent = (kLC && pre) ? !(pre_transit < 0.0) : edge_draw(e, idx, transit);
        if (!sent) drops += 1u;
        return sent;
    }
    AF_CORE bool send_finish(uint32_t e, double now, uint32_t row_now, bool have_row, double transit, double& key, bool& counted) {
        counted = false;
        const double spike = (kMarks && A.n_edge_marks != 0u) ? spike_at(e, now) : 0.0;
        key = now + (transit + spike);
        // A transit time that does not advance the f64 clock (an exponential draw below half an ulp of `now`, a normal
        // truncated at 0) delivers at the send instant: an event of the NEXT station, which commutes with this one;
        // if the next station has another event at that instant the equal keys are seen there.  A NEGATIVE delay
        // (spike residue after += / -=) raises in the reference (simpy: "Negative delay"): handed back.
        if (transit + spike < 0.0) why |= FLOW_WHY_TIE;   // (the next-event kernels report it: AF_FLAG_NEGATIVE_DELAY)
        if (!kFar) {   // (have_row: the server station worked the row of the send time out for its own intervals)
            if (samples != nullptr) add_span(e, have_row ? row_now : tick_index(now, true), tick_index(key, true), 1);
        } else if (samples != nullptr) {   // (row_now: the caller needed it for the delivery it handled)
            const uint32_t ib = tick_index(key, true);
            if (ib != row_now) {
                add_point(e, row_now, 1);
                // the other end: here and now if the ring reaches it (fast hops: always), else by the receiving station
                const uint32_t R = A.L.ring_rows, N = A.n_ticks < A.tick_cap ? A.n_ticks : A.tick_cap;
                if ((kHbmRing && R == 0u) || ib >= N || ib - tick_base < R) add_point(e, ib, -1);
                else counted = true;
            }
        }
        return true;
    }

    // ---- station lists -------------------------------------------------------------------------------
    AF_CORE void append(uint32_t s, bool have, double key, double t0, uint32_t aux, double sent) {
        const uint64_t m = W::ballot(have);
        const uint32_t n = n_list_get(s);
        const uint32_t pos = n + W::mbcnt(m);
        if (have) {
            list_key(s)[pos] = key;
            list_t0(s)[pos] = t0;
            if (kTieBreak) list_ts(s)[pos] = sent;
            if (s == 2u || (kFar && s == 3u)) list_aux(s)[pos] = (uint16_t)aux;
        }
        n_list_set(s, n + popc64(m));
    }

    // select()'s lane window: DPP on the device (engine.hip: WaveHip), the same values from W::shfl32 in host builds
    AF_CORE uint32_t win_lane_below(uint32_t v) const {   // v of lane - 1; 0 in lane 0
#if defined(__HIP_DEVICE_COMPILE__)
        return W::lane_below_u32(v);
#else
        const uint32_t x = W::shfl32(v, (lane + 63u) & 63u);
        return lane != 0u ? x : 0u;
#endif
    }
    AF_CORE uint32_t win_prefix_max(uint32_t v) const {   // max of v over lanes 0 .. mine
#if defined(__HIP_DEVICE_COMPILE__)
        return W::scan_incl_max_u32(v);
#else
        for (uint32_t step = 1u; step < 64u; step <<= 1) {
            const uint32_t x = W::shfl32(v, (lane + 64u - step) & 63u);
            if (lane >= step && x > v) v = x;
        }
        return v;
#endif
    }
    AF_CORE bool win_my_bit(uint64_t m) const {   // bit `lane` of a wave-uniform mask
#if defined(__HIP_DEVICE_COMPILE__)
        return W::my_bit(m);
#else
        return ((m >> lane) & 1ull) != 0ull;
#endif
    }

    // Rank the messages of list s with time < min(H_in, T); hand the `n_sel` earliest (<= room, <= 64) to
    // lanes 0..n_sel-1 in time order; keep the rest.  Returns n_sel.
    // `hs`: the horizon slot of the station that selects (= s, except for the server levels of FEAT_CHAIN: level_slot());
    // `level` != kAnyLevel: only the entries of the server list whose target server is of that level.
    AF_CORE uint32_t select(uint32_t s, double H_in, uint32_t room, double& okey, double& ot0, uint32_t& oaux, uint32_t hs, uint32_t level = kAnyLevel) {
        if (kBig) return select_big(s, H_in, room, okey, ot0, oaux, hs, level);
        // (round 9: a window width per list.  Where they differ, each list has its own copy of select_regs: the plan-specialised
        // builds, whose unrolled stations call with a constant `s`, keep exactly one of the four at each call site.)
        if constexpr (kSelectWindowUniform) {
            return select_regs<IPL, select_window_of(0u)>(s, H_in, room, okey, ot0, oaux, hs, level);
        } else {
            switch (s) {
                case 0u: return select_regs<IPL, select_window_of(0u)>(s, H_in, room, okey, ot0, oaux, hs, level);
                case 1u: return select_regs<IPL, select_window_of(1u)>(s, H_in, room, okey, ot0, oaux, hs, level);
                case 2u: return select_regs<IPL, select_window_of(2u)>(s, H_in, room, okey, ot0, oaux, hs, level);
                default: return select_regs<IPL, select_window_of(3u)>(s, H_in, room, okey, ot0, oaux, hs, level);
            }
        }
    }
    // (IPLx entries per lane in registers: the class's own IPL for the register-resident lists; round 6: also what select_big()
    // hands a list of at most 64 x kBigRegIpl entries to)
    // (WIN: the lane window's width for this list, select_window_of(); 0 = the bucket rank alone)
    template <uint32_t IPLx, uint32_t WIN = 0u>
    AF_CORE uint32_t select_regs(uint32_t s, double H_in, uint32_t room, double& okey, double& ot0, uint32_t& oaux, uint32_t hs, uint32_t level) {
        W::sync();   // appends of the previous station are visible
        const double lo = H_get(hs);
        const double hi_t = H_in < A.total_time ? H_in : A.total_time, hi = (kFar && t_lim < hi_t) ? t_lim : hi_t;   // (t_lim: run())
        const uint32_t n = n_list_get(s);
        okey = AF_INF;
        ot0 = 0.0;
        oaux = 0u;
        if (!(hi > lo)) return 0u;
        if (n == 0u) {
            H_set(hs, hi);
            return 0u;
        }
        AF_PLAN_AS double* K = list_key(s);
        AF_PLAN_AS double* T0 = list_t0(s);
        AF_PLAN_AS double* TS = list_ts(s);
        AF_PLAN_AS uint16_t* AX = list_aux(s);
        // (any positive scale gives a monotone key -> bucket map; ranks come from exact comparisons, so the hardware's
        // approximate reciprocal is as good as a division here)
        double sc = 64.0 * W::rcp(hi - lo);
        if (!(sc < 1e300)) sc = 1e300;
        // Round 8: the lane window.  A list is the previous station's batch in time order plus a jitter far below the batch's span,
        // so it arrives almost sorted: the form with one entry per lane first tries to rank an entry against the kWindow lanes in
        // front of it alone (below), and zeroes and fills the bucket counts only where that is not proved exact.
        constexpr uint32_t kWindow = (IPLx == 1u && !kTieBreak && !kChain) ? WIN : 0u;
        static_assert(kWindow < 32u, "AF_SELECT_WINDOW: lanes an entry looks back");
        if (kWindow == 0u) {
            hist()[lane] = 0u;   // (zeroing them in front of the entry sync instead -- one sync less -- measured: no gain)
            W::sync();
        }
        uint32_t code = 0u;   // kWindow: the bucket map at 2^26 times the scale -- the bucket is its top six bits
        // my (up to 4) entries; bucket counts
        double k[IPLx], t[IPLx], sent[IPLx];
        uint32_t a[IPLx], b[IPLx], slot[IPLx];
        bool valid[IPLx], elig[IPLx];
#pragma unroll
        for (uint32_t q = 0u; q < IPLx; ++q) {
            valid[q] = elig[q] = false;
            k[q] = t[q] = sent[q] = 0.0;
            a[q] = b[q] = slot[q] = 0u;
            {
                // (entries past the list's end are read too -- the arrays hold 64 x IPLx -- and masked by `valid`: the loads and
                // the bucket arithmetic run for every lane, only the atomic sits in a divergent region)
                const uint32_t i = q * 64u + lane;
                valid[q] = i < n;
                k[q] = K[i];
                t[q] = T0[i];
                if (kTieBreak) sent[q] = TS[i];
                a[q] = (s == 2u || (kFar && s == 3u)) ? AX[i] : 0u;
                elig[q] = valid[q] && k[q] < hi && (!kChain || level == kAnyLevel || level_of(a[q] & (kSrvSlots - 1u)) == level);
                if (kWindow == 0u) {
                    double x = (k[q] - lo) * sc;
                    x = x < 63.0 ? x : 63.0;        // (also what a NaN from a stale entry becomes)
                    b[q] = x > 0.0 ? (uint32_t)x : 0u;
                    if (elig[q]) slot[q] = W::lds_add(hist() + b[q], 1u);
                } else {
                    // (a power of two more in the scale commutes with the rounding; an eligible entry's code is in 1 .. 0xFFFFFF00:
                    // 0 and ~0 stand for "no entry" below.  Non-decreasing in the key, so a smaller code IS an earlier key.)
                    double y = (k[q] - lo) * (sc * 67108864.0);
                    y = y < 4294967040.0 ? y : 4294967040.0;
                    code = y > 1.0 ? (uint32_t)y : 1u;
                    b[q] = code >> 26;
                }
            }
        }
        uint32_t E = 0u;
        uint32_t rank[IPLx];
        bool ranked = false;   // wave-uniform
        if constexpr (kWindow != 0u) {
            // c[d - 1]: the code of the entry d lanes in front of me, 0 where that is no eligible entry; `own`: mine, ~0 if I am not
            // eligible -- so neither "in front > own" nor "in front == own" ever holds for a pair with a non-eligible half
            const uint32_t own = elig[0] ? code : 0xFFFFFFFFu;
            uint32_t c[kWindow + 1u];
            c[0] = win_lane_below(elig[0] ? code : 0u);
#pragma unroll
            for (uint32_t d = 1u; d <= kWindow; ++d) c[d] = win_lane_below(c[d - 1u]);
            // An entry's rank is its place among the eligible ones in list order, less the entries of its window in front of it that
            // are later, plus the ones behind it that are earlier: each comparison is made once, by the lane behind, and its wave
            // mask shifted down by d (a scalar shift) tells the lane in front.
            const uint64_t em = W::ballot(elig[0]);
            uint32_t r = W::mbcnt(em);
            uint64_t same = 0ull;
#pragma unroll
            for (uint32_t d = 1u; d <= kWindow; ++d) {
                const bool later_in_front = c[d - 1u] > own;
                const uint64_t m = W::ballot(later_in_front);
                same |= W::ballot(c[d - 1u] == own);
                r -= later_in_front ? 1u : 0u;
                r += win_my_bit(m >> d) ? 1u : 0u;   // the lane d behind me found me later than itself
            }
            // The proof that this is exact: every eligible entry's code is strictly above every eligible code more than kWindow
            // lanes in front of it (their maximum: the prefix maximum of the codes shifted by kWindow + 1 lanes) -- two entries
            // further apart than the window are then in order and differ -- and no two codes inside a window are equal (equal
            // codes say nothing about their keys -- equal, or closer than the code resolves: the bucket rank compares the keys
            // themselves and raises FLOW_WHY_TIE where they are equal).
            // (Measured, config 2, profiles/r08/ab_select_window.txt: with the proof in FRONT of the comparisons -- a branch
            // between the shifts and their use -- the window was 0.4 ms SLOWER than the bucket rank, behind them 1.3 ms faster:
            // the comparisons fill the wait states of the shift chain, and on the benched lists the proof holds in 99.7 % of calls.)
            const uint32_t far_max = win_prefix_max(c[kWindow]);
            ranked = W::ballot(!(own > far_max)) == 0ull && same == 0ull;
            rank[0] = r;
            E = popc64(em);
            if (kProf) {   // (constant indices: the accumulators stay in scalar registers)
                if (ranked) prof_acc[PROF_N_SELECT_WINDOW] += 1ull;
                else prof_acc[PROF_N_SELECT_BUCKET] += 1ull;
            }
#if !defined(__HIPCC__)
            if (lane == 0u) {
                g_select_window_calls[ranked ? 0 : 1] += 1ull;
                g_select_window_by_list[s & 3u][ranked ? 0 : 1] += 1ull;
            }
#endif
            if (!ranked) {
                hist()[lane] = 0u;
                W::sync();
                if (elig[0]) slot[0] = W::lds_add(hist() + b[0], 1u);
            }
        }
        if (!ranked) {
            W::sync();
            const uint32_t cnt = hist()[lane];
            const uint32_t base = excl_scan(cnt, E);
            // a lane's bucket start and count straight from the bucket's lane (two ds_bpermute) instead of an LDS array written,
            // synchronised and read back (round 4: -0.4 %)
            uint32_t bb[IPLx], bc[IPLx];
#pragma unroll
            for (uint32_t q = 0u; q < IPLx; ++q) {
                bb[q] = W::shfl32(base, b[q]);
                bc[q] = W::shfl32(cnt, b[q]);
            }
#pragma unroll
            for (uint32_t q = 0u; q < IPLx; ++q)
                if (elig[q]) {
                    sorted()[bb[q] + slot[q]] = k[q];
                    if (kTieBreak) sorted_ts()[bb[q] + slot[q]] = sent[q];
                }
            W::sync();
#pragma unroll
            for (uint32_t q = 0u; q < IPLx; ++q) {
                rank[q] = 0u;
                if (elig[q]) {
                    const uint32_t p0 = bb[q], p1 = p0 + bc[q], me = p0 + slot[q];
                    uint32_t r = p0;
                    // no region inside the loop (round 4): count the bucket's keys below mine and the ones not above it; they differ
                    // by exactly one (me) unless another message of the station shares my instant
                    if (!kTieBreak) {
                        uint32_t c = p0;
                        // (round 6: the first kAhead keys of my bucket fetched at once -- 64 buckets for ~60 messages: the fullest holds
                        // three or four, and the wave walked it one LDS round trip per key; what lies behind the bucket is masked.
                        // Interleaved A/B, 0 / 2 / 4 ahead: config 2 37.75 / 37.50 / 37.06 ms, config 3 55.3 / 55.0 / 54.25, config 5
                        // 189.2 / 187.7 / 187.5: profiles/r06/ab_select_bucket_ahead.txt)
#if defined(AF_SELECT_BUCKET_AHEAD)
                        constexpr uint32_t kAhead = AF_SELECT_BUCKET_AHEAD;
#else
                        constexpr uint32_t kAhead = 4u;
#endif
                        double kq[kAhead > 0u ? kAhead : 1u];
#pragma unroll
                        for (uint32_t u = 0u; u < kAhead; ++u) kq[u] = sorted()[p0 + u];
#pragma unroll
                        for (uint32_t u = 0u; u < kAhead; ++u) {
                            const bool in = u < bc[q];
                            r += in && kq[u] < k[q] ? 1u : 0u;
                            c += in && kq[u] <= k[q] ? 1u : 0u;
                        }
#pragma nounroll
                        for (uint32_t p = p0 + kAhead; p < p1; ++p) {
                            const double kk = sorted()[p];
                            r += kk < k[q] ? 1u : 0u;
                            c += kk <= k[q] ? 1u : 0u;
                        }
                        why |= c != r + 1u ? FLOW_WHY_TIE : 0u;
                        (void)me;
                    } else
#pragma nounroll   // (a bucket holds one or two messages: the unrolled-by-eight form was 115 instructions per site for ~1.5 trips)
                    for (uint32_t p = p0; p < p1; ++p) {
                        const double kk = sorted()[p];
                        r += kk < k[q] ? 1u : 0u;
                        if (kk == k[q] && p != me) {   // two deliveries of this station at one instant
                            if (kTieBreak) {           // SimPy pops the one whose Timeout was created -- that was sent -- first
                                const double other = sorted_ts()[p];
                                r += other < sent[q] ? 1u : 0u;
                                if (other == sent[q]) why |= FLOW_WHY_TIE;
                            } else {
                                why |= FLOW_WHY_TIE;
                            }
                        }
                    }
                    rank[q] = r;
                }
            }
        }
        uint32_t n_sel = E < room ? E : room;
        n_sel = n_sel < 64u ? n_sel : 64u;
        double h_left = 0.0;   // the first message left behind bounds the horizon: its key straight from the lane that
        if (n_sel < E) {       // holds it (ballot + v_readlane), not through LDS (round 4)
#pragma unroll
            for (uint32_t q = 0u; q < IPLx; ++q) {
                const uint64_t mb = W::ballot(elig[q] && rank[q] == n_sel);
                if (mb != 0ull) h_left = bcast_f64(k[q], (uint32_t)__builtin_ctzll(mb));
            }
        }
        // (round 9: handing the window's batch over by a forward lane permute instead of the buffer below was measured and was
        // 1.4 ms per step slower -- DESIGN.md section 5, profiles/r09/ab_select_widths.txt)
        uint32_t kept = 0u;
#pragma unroll
        for (uint32_t q = 0u; q < IPLx; ++q) {
            {
                const bool sel = elig[q] && rank[q] < n_sel;
                const bool keep = valid[q] && !sel;
                const uint64_t m = W::ballot(keep);
                const uint32_t pos = kept + W::mbcnt(m);
                // the selected and the kept entries leave through ONE divergent region and one computed address each (batch buffer
                // at its rank, or the list at its new place); the aux word only where a list has one (round 4: 41.87 -> 41.46 ms)
                const bool has_aux = s == 2u || (kFar && s == 3u);
                if (valid[q]) {
                    AF_PLAN_AS double* dk = sel ? out_key() + rank[q] : K + pos;
                    AF_PLAN_AS double* dt = sel ? out_t0() + rank[q] : T0 + pos;
                    *dk = k[q];
                    *dt = t[q];
                    if (kTieBreak && keep) TS[pos] = sent[q];
                    if (has_aux) {
                        if (sel) out_aux()[rank[q]] = a[q];
                        else AX[pos] = (uint16_t)a[q];
                    }
                }
                kept += popc64(m);
            }
        }
        n_list_set(s, kept);
#if !defined(__HIPCC__)
        if (lane == 0u && ranked) {
            g_select_window_calls[2] += kept != 0u ? 1ull : 0ull;
            g_select_window_calls[3] += n_sel < E ? 1ull : 0ull;
        }
#endif
        W::sync();
        H_set(hs, n_sel < E ? h_left : hi);
        if (lane < n_sel) {
            okey = out_key()[lane];
            ot0 = out_t0()[lane];
            if (s == 2u || (kFar && s == 3u)) oaux = out_aux()[lane];
        }
        return n_sel;
    }

    // The same selection for lists of any length (FEAT_BIGLIST): the list is walked in chunks of 64, what select()
    // keeps in registers lives in a u32 per entry (bucket | slot, then the rank), and exact ranks are only worked out
    // for the buckets that can reach the first n_sel places (or hold the first message left behind).
    AF_CORE uint32_t select_big(uint32_t s, double H_in, uint32_t room, double& okey, double& ot0, uint32_t& oaux, uint32_t hs, uint32_t level) {
        W::sync();
        const double lo = H_get(hs);
        const double hi_t = H_in < A.total_time ? H_in : A.total_time, hi = (kFar && t_lim < hi_t) ? t_lim : hi_t;   // (t_lim: run())
        const uint32_t n = n_list_get(s);
        okey = AF_INF;
        ot0 = 0.0;
        oaux = 0u;
        if (!(hi > lo)) return 0u;
        if (n == 0u) {
            H_set(hs, hi);
            return 0u;
        }
#if !defined(AF_BIG_NO_REGS)
        // (round 6: a list that fits kBigRegIpl entries per lane is ranked out of registers like the short lists -- one pass and
        // five LDS round trips instead of four passes over u32 words per entry; the general servers' first launch, whose lists
        // hold 64 .. 128 entries, spent a fifth of its time here)
        if (n <= 64u * kBigRegIpl) return select_regs<kBigRegIpl>(s, H_in, room, okey, ot0, oaux, hs, level);
#endif
        AF_PLAN_AS double* K = list_key(s);
        AF_PLAN_AS double* T0 = list_t0(s);
        AF_PLAN_AS double* TS = list_ts(s);
        AF_PLAN_AS uint16_t* AX = list_aux(s);
        AF_PLAN_AS uint32_t* EB = eb();
        constexpr uint32_t kNone = 0xFFFFFFFFu, kFar = 0xFFFFFFFEu;
        double sc = 64.0 * W::rcp(hi - lo);
        if (!(sc < 1e300)) sc = 1e300;
        hist()[lane] = 0u;
        W::sync();
        const uint32_t nq = (n + 63u) / 64u;
        for (uint32_t q = 0u; q < nq; ++q) {
            const uint32_t i = q * 64u + lane;
            if (i < n) {
                const double k = K[i];
                uint32_t w = kNone;
                if (k < hi && (!kChain || level == kAnyLevel || level_of(AX[i] & (kSrvSlots - 1u)) == level)) {
                    double x = (k - lo) * sc;
                    x = x < 63.0 ? x : 63.0;
                    const uint32_t b = x > 0.0 ? (uint32_t)x : 0u;
                    w = (b << 16) | W::lds_add(hist() + b, 1u);
                }
                EB[i] = w;
            }
        }
        W::sync();
        uint32_t E;
        const uint32_t cnt = hist()[lane];
        const uint32_t base = excl_scan(cnt, E);
        bbase()[lane] = base;
        W::sync();
        for (uint32_t q = 0u; q < nq; ++q) {
            const uint32_t i = q * 64u + lane;
            if (i < n && EB[i] != kNone) {
                const uint32_t at = bbase()[EB[i] >> 16] + (EB[i] & 0xFFFFu);
                sorted()[at] = K[i];
                if (kTieBreak) sorted_ts()[at] = TS[i];
            }
        }
        W::sync();
        uint32_t n_sel = E < room ? E : room;
        n_sel = n_sel < 64u ? n_sel : 64u;
        for (uint32_t q = 0u; q < nq; ++q) {
            const uint32_t i = q * 64u + lane;
            if (i < n && EB[i] != kNone) {
                const uint32_t b = EB[i] >> 16, p0 = bbase()[b];
                uint32_t r = kFar;
                if (p0 <= n_sel) {
                    const uint32_t p1 = p0 + hist()[b], me = p0 + (EB[i] & 0xFFFFu);
                    const double k = K[i];
                    r = p0;
                    for (uint32_t p = p0; p < p1; ++p) {
                        const double kk = sorted()[p];
                        r += kk < k ? 1u : 0u;
                        if (kk == k && p != me) {   // two deliveries of this station at one instant (see select())
                            if (kTieBreak) {
                                const double other = sorted_ts()[p], mine = TS[i];
                                r += other < mine ? 1u : 0u;
                                if (other == mine) why |= FLOW_WHY_TIE;
                            } else {
                                why |= FLOW_WHY_TIE;
                            }
                        }
                    }
                    if (r == n_sel && n_sel < E) scal()[0] = k;   // the first message left behind bounds the horizon
                }
                EB[i] = r;
            }
        }
        W::sync();
        uint32_t kept = 0u;
        for (uint32_t q = 0u; q < nq; ++q) {
            const uint32_t i = q * 64u + lane;
            const bool valid = i < n;
            double k = 0.0, t = 0.0, ts = 0.0;
            uint32_t a = 0u, r = kNone;
            if (valid) {
                k = K[i];
                t = T0[i];
                if (kTieBreak) ts = TS[i];
                if (s == 2u || (kFar && s == 3u)) a = AX[i];
                r = EB[i];
            }
            const bool sel = valid && r < n_sel;
            if (sel) {
                out_key()[r] = k;
                out_t0()[r] = t;
                out_aux()[r] = a;
            }
            const bool keep = valid && !sel;
            const uint64_t m = W::ballot(keep);       // (every lane has read its entry of this chunk: writes below
            const uint32_t pos = kept + W::mbcnt(m);  //  land at or before the writer's own index)
            if (keep) {
                K[pos] = k;
                T0[pos] = t;
                if (kTieBreak) TS[pos] = ts;
                if (s == 2u || (kFar && s == 3u)) AX[pos] = (uint16_t)a;
            }
            kept += popc64(m);
        }
        n_list_set(s, kept);
        W::sync();
        H_set(hs, n_sel < E ? scal()[0] : hi);
        if (lane < n_sel) {
            okey = out_key()[lane];
            ot0 = out_t0()[lane];
            oaux = out_aux()[lane];
        }
        return n_sel;
    }

    // index of each lane's message on its edge: sends[e] + (messages of lower lanes on the same edge).
    // Candidate edges: the LB's out-edges (payload order) or the servers' out-edges; the lane that holds a candidate's
    // counter advances it.
    // (round 6, measured and dropped: the edges PRESENT in the batch taken from the lanes one after the other -- first lane left, its
    // edge through v_readlane, everybody on it by ballot -- instead of the walk over the candidates, whose edge numbers are LDS reads
    // at wave-uniform addresses: config 5 177.0 -> 181.1 ms, config 2 36.1 -> 36.6.  The candidates' reads do not wait for each other.)
    AF_CORE uint32_t claim_send_index(bool have, uint32_t e, bool server_edges) {
        const uint32_t n_cand = server_edges ? A.n_servers : A.n_lb_edges;
        uint32_t idx = 0u;
        for (uint32_t c = 0u; c < n_cand; ++c) {
            const uint32_t ce = server_edges ? (uint32_t)(blob[A.off_srv + af::SREC * c + 1u] >> 16) & 0xFFFFu
                                             : (uint32_t)blob[A.off_lb + c];
            const uint64_t m = W::ballot(have && e == ce);
            const uint32_t at = sends_of(ce);
            if (have && e == ce) idx = at + W::mbcnt(m);
            if (lane == ce) my_sends += popc64(m);
        }
        return idx;
    }

    // ---- load balancer (round robin, lb_algorithms.py:22-36; outages injection.py:201-226) -----------
    // picks for the n_sel messages now in out_key() (time order); lane r gets the out-edge of message r
    // (round robin: head of the rotation, live out-edges, mark cursor and ceil(2^32 / n_live) are wave-uniform REGISTERS since
    // round 4 -- lb_head .. lb_magic, written through to lbw()[16..19] only around the rare walk over an outage mark; the
    // least-connections walk, which never runs in the same scenario, keeps using the LDS words)
    uint32_t lb_head, lb_nl, lb_mark, lb_magic;
    AF_CORE uint32_t lb_pick(uint32_t n_sel, double my_key) {
        AF_PLAN_AS uint32_t* lw = lbw();
        uint32_t pick = 0u;
        const uint32_t mi = lb_mark;
        const double t_last = bcast_f64(my_key, n_sel - 1u);
        const bool marks_inside = kMarks && mi < A.n_srv_marks && u2d(smark(mi)[0]) <= t_last;
        if (!marks_inside) {
            const uint32_t head = lb_head, nl = lb_nl;
            // (head + lane) mod nl by multiplication: head + lane < 2^16, magic = ceil(2^32 / nl)
            const uint32_t x = head + lane;
            const uint32_t q = nl > 1u ? (uint32_t)(((uint64_t)x * lb_magic) >> 32) : x;
            if (lane < n_sel) pick = lw[x - q * nl];
            // (head + n_sel) mod nl by the same multiplication: a u32 division was 25 instructions per round
            const uint32_t y = head + n_sel, qy = nl > 1u ? (uint32_t)(((uint64_t)y * lb_magic) >> 32) : y;
            lb_head = y - qy * nl;
            return pick;
        } else {
            if (lane == 0u) {
                lw[16] = lb_head;
                lw[17] = lb_nl;
            }
            W::sync();
            if (lane == 0u) {   // rare (one round per outage mark): one lane walks the messages in time order
                uint32_t head = lw[16], nl = lw[17], cur = mi;
                for (uint32_t r = 0u; r < n_sel; ++r) {
                    const double tr = out_key()[r];
                    while (cur < A.n_srv_marks && u2d(smark(cur)[0]) <= tr) {
                        if (u2d(smark(cur)[0]) == tr) why |= FLOW_WHY_TIE;
                        const uint64_t meta = smark(cur)[1];
                        const uint32_t e1 = (uint32_t)meta;
                        if (e1 != 0u) {
                            uint32_t tmp[16];
                            for (uint32_t i = 0u; i < nl; ++i) tmp[i] = lw[(head + i) % nl];   // materialise the rotation
                            uint32_t m2 = 0u;
                            for (uint32_t i = 0u; i < nl; ++i)
                                if (tmp[i] != e1 - 1u) tmp[m2++] = tmp[i];
                            if (!(meta >> 32)) tmp[m2++] = e1 - 1u;   // SERVER_UP: back in at the tail
                            nl = m2;
                            head = 0u;
                            for (uint32_t i = 0u; i < nl; ++i) lw[i] = tmp[i];
                        }
                        cur += 1u;
                    }
                    out_aux()[r] = lw[head % (nl ? nl : 1u)];
                    head = nl ? (head + 1u) % nl : 0u;
                }
                lw[16] = head;
                lw[17] = nl;
                lw[18] = cur;
                lw[19] = nl ? 0xFFFFFFFFu / nl + 1u : 0u;
            }
            W::sync();
            if (lane < n_sel) pick = out_aux()[lane];
            lb_head = lw[16];
            lb_nl = lw[17];
            lb_mark = lw[18];
            lb_magic = lw[19];
        }
        W::sync();
        return pick;
    }

    // least_connections (lb_algorithms.py:10-20): the out-edge with the fewest messages in flight, the first such in
    // the current order.  "In flight on an LB edge at time t" is knowledge of the LB station alone: sent before t (by
    // this station, in time order) and delivered after t -- the entries of the server list with that target and a
    // later delivery time (the server station only ever took deliveries before its horizon <= t: no lookahead
    // behind a least-connections LB, send_floor) plus the earlier messages of this batch.  Dropped messages never
    // count (edge.py:78-88).  The picks depend on each other, so the whole wave walks the batch one message at a
    // time; what does not depend on them is done first and in parallel: the next 64 draws of every out-edge.
    // Returns lane r's out-edge; `tr` = its transit time (< 0: dropped).
    AF_CORE uint32_t lb_pick_lc(uint32_t n_sel, double my_key, double& tr) {
        // (the narrow form where the fan-out allows it: half the draws and half the count words in registers; wave-uniform,
        // a constant of a plan-specialised build)
        if (A.n_lb_edges <= 8u && A.n_servers <= 8u) return lb_pick_lc_n<8u>(n_sel, my_key, tr);
        return lb_pick_lc_n<kMaxServers>(n_sel, my_key, tr);
    }
    template <uint32_t NS>
    AF_CORE uint32_t lb_pick_lc_n(uint32_t n_sel, double my_key, double& tr) {
        static_assert(NS % 4u == 0u && NS <= kMaxServers, "four 16-bit counts per word");
        constexpr uint32_t NW = NS / 4u;
        AF_PLAN_AS uint32_t* lw = lbw();
        // xs[c]: my lane's draw on the c-th out-edge (payload order) = the transit time of the (lane+1)-th message this
        // batch sends there (< 0: dropped).  Registers, not LDS: the walk below reads one of them per message, and an
        // LDS round trip per message would be most of its time.
        double xs[NS];
#pragma unroll
        for (uint32_t c = 0u; c < NS; ++c) {
            xs[c] = -1.0;
            if (c < A.n_lb_edges) {
                const uint32_t e = (uint32_t)blob[A.off_lb + c];
                double x = -1.0;
                if (edge_draw(e, sends_of(e) + lane, x)) xs[c] = x;
            }
        }
        // What does not depend on the picks either: how many entries of the server list are still in flight towards
        // each server at MY message's time -- every lane walks the list (the same entry in all lanes: LDS broadcasts)
        // and keeps NS 16-bit counts in NS / 4 words (<= 16 384 entries).
        const AF_PLAN_AS double* K2 = list_key(2u);
        const AF_PLAN_AS uint16_t* AX = list_aux();
        const uint32_t n2 = n_list_get(2u);
        uint64_t bw[NW];
#pragma unroll
        for (uint32_t w = 0u; w < NW; ++w) bw[w] = 0ull;
        uint64_t lb_edges = 0ull;   // FEAT_CHAIN: the server list also holds what servers send to servers -- not in flight on an LB edge
        if (kChain)
            for (uint32_t c = 0u; c < A.n_lb_edges; ++c) lb_edges |= 1ull << ((uint32_t)blob[A.off_lb + c] & 63u);
        for (uint32_t i2 = 0u; i2 < n2; ++i2) {
            const double k = K2[i2];
            const uint32_t axw = W::bcast32(AX[i2], 0u), ax = axw & 0xFFu;
            const bool by_lb = !kChain || ((lb_edges >> ((axw >> 8) & 63u)) & 1ull) != 0ull;
            const uint64_t inc = (by_lb && k > my_key) ? 1ull << (16u * (ax & 3u)) : 0ull;
#pragma unroll
            for (uint32_t w = 0u; w < NW; ++w) bw[w] += (ax >> 2) == w ? inc : 0ull;   // (ax is wave-uniform: one scalar test per word)
            if (k == my_key) why |= FLOW_WHY_TIE;   // a delivery by the LB's edges at the very instant of a decision
        }
        // the candidates in the LB's current order: lane i < n_live holds (out-edge, its server, its place in the payload order)
        uint32_t live_e = 0u, live_srv = 0u, live_c = 0u, nl = 0u, cur = 0u;
        double next_mark = AF_INF;   // time of the next outage mark
        auto load_live = [&]() {
            nl = lw[17];
            cur = lw[18];
            next_mark = (kMarks && cur < A.n_srv_marks) ? u2d(smark(cur)[0]) : AF_INF;
            live_e = lane < nl ? lw[lane] : 0u;
            live_srv = (uint32_t)(erec(live_e)[3] >> 8) & 0xFFu;
            live_c = 0u;
            for (uint32_t c = 0u; c < A.n_lb_edges; ++c) live_c = (uint32_t)blob[A.off_lb + c] == live_e ? c : live_c;
        };
        load_live();
        uint32_t my_e = 0u;
        double my_k2 = -AF_INF;   // delivery time of my message once it is picked (-inf: not picked yet / dropped)
        tr = -1.0;
        for (uint32_t r = 0u; r < n_sel; ++r) {
            const double t = bcast_f64(my_key, r);
            if (kMarks && next_mark <= t) {   // outages up to t (injection.py:201-226)
                W::sync();
                if (lane == 0u) {
                    uint32_t m = lw[17];
                    while (cur < A.n_srv_marks && u2d(smark(cur)[0]) <= t) {
                        if (u2d(smark(cur)[0]) == t) why |= FLOW_WHY_TIE;
                        const uint64_t meta = smark(cur)[1];
                        const uint32_t e1 = (uint32_t)meta;
                        if (e1 != 0u) {
                            uint32_t m2 = 0u;
                            for (uint32_t i = 0u; i < m; ++i)
                                if (lw[i] != e1 - 1u) lw[m2++] = lw[i];
                            if (!(meta >> 32)) lw[m2++] = e1 - 1u;   // SERVER_UP: back in at the tail
                            m = m2;
                        }
                        cur += 1u;
                    }
                    lw[17] = m;
                    lw[18] = cur;
                }
                W::sync();
                load_live();
            }
            uint64_t br[NW];   // message r's counts
#pragma unroll
            for (uint32_t w = 0u; w < NW; ++w) br[w] = W::bcast64(bw[w], r);
            uint32_t best = 0xFFFFFFFFu, best_e = 0u, best_i = 0u;
            for (uint32_t i = 0u; i < nl; ++i) {
                const uint32_t e = W::bcast32(live_e, i), srv = W::bcast32(live_srv, i);
                uint64_t word = br[0];
#pragma unroll
                for (uint32_t w = 1u; w < NW; ++w) word = (srv >> 2) == w ? br[w] : word;
                uint32_t cnt = (uint32_t)(word >> (16u * (srv & 3u))) & 0xFFFFu;
                const bool earlier = lane < r && my_e == e;
                cnt += popc64(W::ballot(earlier && my_k2 > t));
                if (earlier && my_k2 == t) why |= FLOW_WHY_TIE;
                if (cnt < best) {
                    best = cnt;
                    best_e = e;
                    best_i = i;
                }
            }
            // the message's place among this batch's messages on that edge = which of the prepared draws is its own
            const uint32_t k_on_edge = popc64(W::ballot(lane < r && my_e == best_e));
            const uint32_t c_of = W::bcast32(live_c, best_i);
            double x = -1.0;
#pragma unroll
            for (uint32_t c = 0u; c < NS; ++c)
                if (c == c_of) x = bcast_f64(xs[c], k_on_edge);
            const double sp = (kMarks && A.n_edge_marks != 0u) ? spike_at(best_e, t) : 0.0;
            if (lane == r) {
                my_e = best_e;
                tr = x;
                my_k2 = x < 0.0 ? -AF_INF : t + (x + sp);
            }
        }
        W::sync();
        return my_e;
    }

    // ---- servers (server.py:79-276 for endpoints of the form IO* CPU* IO*) ----------------------------
    // Every request of a server runs the same step program, so the server is a tandem of FIFO stations and
    //   adm_j = max(arrival_j, G_{j-slots})      RAM admission: strict FIFO, `slots` requests fit at once (server.py:146-149)
    //   B_j   = adm_j + leading I/O steps
    //   S_j   = max(B_j, F_{j-cores})            the core released `cores` requests earlier (server.py:210-231)
    //   F_j   = S_j + CPU steps,  G_j = F_j + trailing I/O steps         (every + is one timed event)
    // The lanes hold the window's arrivals (one each, time order, grouped per server in `seg`).  The recurrence
    // is solved by relaxation: every lane recomputes its own times from its predecessors' until nothing changes.
    // Values only grow and each is the same max / + the sequential walk does, so the fixed point IS the
    // sequential result; the number of passes is the longest chain of requests that wait on each other.
    struct SrvTimes {
        double adm, b, s, f, g;
        uint32_t events;   // step ends before the horizon
        uint32_t out_edge; // servers_solve(): the server's out-edge and its endpoint's RAM need (read there anyway)
        double ram;
    };
    // (the loops run to the plan-wide maxima with the lane's own counts as predicates: wave-uniform loop control
    // instead of three per-lane while loops)
    // (round 6: the step times of my request's program in REGISTERS while the relaxation runs -- every pass read them again
    // from the plan blob, one LDS round trip per step and pass in a chain of dependent additions; programs of up to kStepRegs
    // leading-I/O, CPU and trailing-I/O steps, which is every example of the reference; longer ones keep reading the blob)
    static constexpr uint32_t kStepRegs = 2u;
    struct StepDur {
        double pre[kStepRegs], cpu[kStepRegs], post[kStepRegs];
    };
#if defined(AF_NO_STEP_REGS)
    AF_CORE bool step_regs_ok() const { return false; }   // (measurement hook)
#else
    AF_CORE bool step_regs_ok() const { return A.max_pre <= kStepRegs && A.max_cpu <= kStepRegs && A.max_post <= kStepRegs; }
#endif
    AF_CORE StepDur step_durations(uint32_t row0, uint32_t counts) const {
        StepDur d;
        const uint32_t n_pre = counts & 0xFFu, n_cpu = (counts >> 8) & 0xFFu;
#pragma unroll
        for (uint32_t i = 0u; i < kStepRegs; ++i) {   // (a row past my own program's is read and never used)
            d.pre[i] = i < A.max_pre ? u2d(blob[A.off_row + af::TREC * (row0 + i)]) : 0.0;
            d.cpu[i] = i < A.max_cpu ? u2d(blob[A.off_row + af::TREC * (row0 + n_pre + i)]) : 0.0;
            d.post[i] = i < A.max_post ? u2d(blob[A.off_row + af::TREC * (row0 + n_pre + n_cpu + i)]) : 0.0;
        }
        return d;
    }
    AF_CORE static double reg_step(const double (&v)[kStepRegs], uint32_t i) {
        double x = v[0];
#pragma unroll
        for (uint32_t u = 1u; u < kStepRegs; ++u) x = i == u ? v[u] : x;
        return x;
    }
    AF_CORE SrvTimes srv_program(uint32_t row0, uint32_t counts, double arrival, double g_prev, double f_prev, bool regs, const StepDur& d) const {
        SrvTimes r;
        const double T = A.total_time;
        const uint32_t n_pre = counts & 0xFFu, n_cpu = (counts >> 8) & 0xFFu, n_post = (counts >> 16) & 0xFFu;
        r.adm = g_prev > arrival ? g_prev : arrival;
        double t = r.adm;
        uint32_t e_cnt = 0u;
        for (uint32_t i = 0u; i < A.max_pre; ++i)   // leading I/O steps
            if (i < n_pre) {
                t = t + (regs ? reg_step(d.pre, i) : u2d(blob[A.off_row + af::TREC * (row0 + i)]));
                e_cnt += t < T ? 1u : 0u;
            }
        r.b = t;
        if (n_cpu > 0u && f_prev > t) t = f_prev;
        r.s = t;
        for (uint32_t i = 0u; i < A.max_cpu; ++i)
            if (i < n_cpu) {
                t = t + (regs ? reg_step(d.cpu, i) : u2d(blob[A.off_row + af::TREC * (row0 + n_pre + i)]));
                e_cnt += t < T ? 1u : 0u;
            }
        r.f = t;
        for (uint32_t i = 0u; i < A.max_post; ++i)  // trailing I/O steps
            if (i < n_post) {
                t = t + (regs ? reg_step(d.post, i) : u2d(blob[A.off_row + af::TREC * (row0 + n_pre + n_cpu + i)]));
                e_cnt += t < T ? 1u : 0u;
            }
        r.g = t;
        r.events = e_cnt;
        return r;
    }
    // `have` lanes: arrival `a` at server `sv`, position `pos` in seg (its server's segment starts at lbw()[LBW_SEG_OFF + sv] and
    // holds lbw()[LBW_SEG_LEN + sv] arrivals).  Returns the lane's times; advances the server's counters and rings.
    // (`seg_off` / `seg_len`: where my server's segment starts and how many arrivals it holds; `srv_cnt`: lane k < n_servers --
    // how many arrivals server k got in this window: registers, worked out where the segments are, not words of lbw())
    AF_CORE SrvTimes servers_solve(bool arrived, uint32_t sv, uint32_t pos, double a, uint32_t seg_off, uint32_t seg_len, uint32_t srv_cnt) {
        AF_PLAN_AS uint32_t* lw = lbw();
        // A server whose endpoint needs more RAM than the server has never admits anybody: the first request blocks in
        // RAM.get() for good and everything behind it queues up (server.py:146-149; Container gets are FIFO).  Such
        // arrivals are timed events and nothing else.
        // (round 6: three LDS round trips instead of seven -- what is indexed by the server first, every lane, no conditions (a
        // lane without an arrival reads server 0's words and uses none of them); then the endpoint's two words; then the ring
        // entries and the step times.  The station was a chain of dependent, conditional reads.)
        const uint32_t slots = lw[LBW_SLOTS + sv];   // requests that fit the RAM at once
        const uint32_t arrivals0 = lw[LBW_ARRIVALS + sv], prog = lw[LBW_PROG + sv];
        const uint64_t meta = blob[A.off_srv + af::SREC * sv + 1u];
        const bool have = arrived && slots != 0u;
        const uint32_t off = have ? seg_off : 0u, n_k = have ? seg_len : 0u;
        const uint32_t li = pos - off;                         // my index among this window's arrivals of my server
        const uint32_t j = have ? arrivals0 + li : 0u;         // ... and among all of them
        const uint32_t cores = (uint32_t)meta & 0xFFFFu;
        const uint32_t ep = (uint32_t)(meta >> 32) & 0xFFFFu;
        const double ram = u2d(blob[A.off_ep + af::PREC * ep]);
        const uint32_t row0 = (uint32_t)blob[A.off_ep + af::PREC * ep + 1u];
        const uint32_t G = A.L.g_ring;
        // where my predecessors' times come from: this window's segment, or the rings of earlier windows
        const bool ram_gate = have && ram > 0.0 && slots != 0u && slots <= G && j >= slots;
        const bool core_gate = have && j >= cores;
        const bool g_in_seg = ram_gate && li >= slots, f_in_seg = core_gate && li >= cores;
        // (the ring entries are read by every lane -- masked indices stay inside the rings -- and used where the gates say so)
        const double g_ring_v = gr(sv)[(j - slots) & (G - 1u)], f_ring_v = fr(sv)[(j - cores) & (A.L.c_ring - 1u)];   // (the release `cores` requests earlier: c_ring >= cores slots)
        const bool regs = step_regs_ok();   // (wave-uniform; a constant of a plan-specialised build)
        StepDur sd{};
        if (regs) sd = step_durations(row0, prog);
        double g_prev = (ram_gate && !g_in_seg) ? g_ring_v : -AF_INF;
        double f_prev = (core_gate && !f_in_seg) ? f_ring_v : -AF_INF;
        if (have && ram > 0.0) {
            if (slots > G && j >= G) {         // more slots than the ring remembers: fine while fewer than G requests are inside
                const double gq = li >= G ? AF_INF : gr(sv)[(j - G) & (G - 1u)];   // (li >= G: G arrivals of one server in one window)
                if (!(gq < a)) why |= FLOW_WHY_RAM;
            }
        }
        SrvTimes r = srv_program(row0, prog, a, g_prev, f_prev, regs, sd);
        for (;;) {
            if (have) {
                seg(3)[pos] = r.f;
                seg(4)[pos] = r.g;
            }
            W::sync();
            bool changed = false;
            if (g_in_seg || f_in_seg) {
                const double gp = g_in_seg ? seg(4)[pos - slots] : g_prev;
                const double fp = f_in_seg ? seg(3)[pos - cores] : f_prev;
                if (gp != g_prev || fp != f_prev) {
                    g_prev = gp;
                    f_prev = fp;
                    const SrvTimes n = srv_program(row0, prog, a, g_prev, f_prev, regs, sd);
                    changed = n.f != r.f || n.g != r.g;
                    r = n;
                }
            }
            const bool again = W::any(changed);
            W::sync();
            if (!again) break;
        }
        if (have) {
            // g_prev == a (an arrival at the instant a predecessor frees its RAM) and f_prev == r.b (a request for a
            // core at the instant one is released) need no hand-back: whichever of the two SimPy pops first, the
            // request is admitted / granted AT that instant, behind the same earlier waiters (both queues are FIFO
            // in arrival order), and the zero-length wait it may be counted for ends before any tick can see it
            // (a tick at that very instant is flagged by tick_index).  A RAM-bound server with deterministic step
            // times produces such instants all the time: F[j-1] = G[j-1-slots] + cpu and G[j-slots] = F[j-slots] + io
            // are the same sum.
            if (li + cores >= n_k) fr(sv)[j & (A.L.c_ring - 1u)] = r.f;   // the last `cores` releases / G departures feed later windows
            if (li + G >= n_k) gr(sv)[j & (G - 1u)] = r.g;
            ev += r.events;
        }
        W::sync();
        if (lane < A.n_servers) (void)W::lds_add(lw + LBW_ARRIVALS + lane, srv_cnt);   // (no value comes back: nothing to wait for)
        r.out_edge = (uint32_t)(meta >> 16) & 0xFFFFu;
        r.ram = ram;
        if (arrived && !have) {   // never admitted (the sequential kernels and the oracle report the same, informational, flag)
            r.adm = r.b = r.s = r.f = r.g = AF_INF;
            info |= af::FLAG_RAM_STARVED;
        }
        return r;
    }


    // ---- general servers (FEAT_GENSRV; server.py:79-313 without the tandem restriction) -------------------------------
    // Lane sv < n_servers runs server sv: its arrivals of this round (seg(0) / seg(1): time, start time, time order, segment
    // [LBW_SEG_OFF, + LBW_SEG_LEN)) merged with its pending step ends, in time order, up to `limit` (every arrival before it is
    // known).  Plain per-lane code: no cross-lane operation in here.  Departures go to the server's GS_DEPT / GS_DEPT0 arrays.
    AF_CORE AF_PLAN_AS uint64_t* gs(uint32_t sv) const { return M + A.L.off_gsrv + sv * kGsWords; }
    // The ten scalar words of the lane's server live in REGISTERS while gen_servers() runs (round 4): the station is a chain of
    // dependent LDS round trips of one lane, and these words were half of them.  Loaded on entry, stored on exit; everything
    // outside gen_servers() (run(): the departure counts, the setup) sees the LDS copy.
    struct GsRegs {
        uint64_t cpu, io, ram, arr, cq, rq, ev, dep, last, lastdep;
    } GR;
    AF_CORE void gs_load(const AF_PLAN_AS uint64_t* g) {
        GR.cpu = g[GS_CPU]; GR.io = g[GS_IO]; GR.ram = g[GS_RAM]; GR.arr = g[GS_ARR]; GR.cq = g[GS_CQ];
        GR.rq = g[GS_RQ]; GR.ev = g[GS_EV]; GR.dep = g[GS_DEP]; GR.last = g[GS_LAST]; GR.lastdep = g[GS_LASTDEP];
    }
    AF_CORE void gs_store(AF_PLAN_AS uint64_t* g) const {
        g[GS_CPU] = GR.cpu; g[GS_IO] = GR.io; g[GS_RAM] = GR.ram; g[GS_ARR] = GR.arr; g[GS_CQ] = GR.cq;
        g[GS_RQ] = GR.rq; g[GS_EV] = GR.ev; g[GS_DEP] = GR.dep; g[GS_LAST] = GR.last; g[GS_LASTDEP] = GR.lastdep;
    }
    AF_CORE static uint32_t lo32(uint64_t w) { return (uint32_t)w; }
    AF_CORE static uint32_t hi32(uint64_t w) { return (uint32_t)(w >> 32); }
    AF_CORE static uint64_t pack32(uint32_t lo, uint32_t hi) { return (uint64_t)lo | ((uint64_t)hi << 32); }
    AF_CORE AF_PLAN_AS uint8_t* gs_bytes(AF_PLAN_AS uint64_t* g, uint32_t which) const { return (AF_PLAN_AS uint8_t*)(g + GS_BYTES) + which * kGsSlots; }
    AF_CORE void gs_point(uint32_t series, uint32_t row, int32_t w) {
        if (samples != nullptr) add_point(series, row, w);
    }
    // pending step end of `slot` at `t`: sorted ring (ascending; equal times are found when they reach the front)
    // Step ends that share an instant are handled in the order their Timeouts were created (SimPy's heap key: time, priority,
    // event id): equal times go BEHIND what is there, and the calls below come in the order the reference creates the
    // Timeouts of one event's cascade (the request's own, then the core waiter's, then the RAM waiters': af_core.hpp, "stages").
    // In an instant the server shares between several of its step ends SimPy interleaves the zero-time steps of the tied
    // cascades: gs_instant() runs those in SimPy's order, so the order of the calls below is the creation order there too.
    AF_CORE void gs_schedule(AF_PLAN_AS uint64_t* g, double t, uint32_t slot) {
        const uint32_t head = lo32(GR.ev), n = hi32(GR.ev);
        AF_PLAN_AS uint8_t* es = gs_bytes(g, 0u);
        uint32_t i = n;
        while (i > 0u && u2d(g[GS_EVT + ((head + i - 1u) & (kGsSlots - 1u))]) > t) {
            g[GS_EVT + ((head + i) & (kGsSlots - 1u))] = g[GS_EVT + ((head + i - 1u) & (kGsSlots - 1u))];
            es[(head + i) & (kGsSlots - 1u)] = es[(head + i - 1u) & (kGsSlots - 1u)];
            i -= 1u;
        }
        g[GS_EVT + ((head + i) & (kGsSlots - 1u))] = d2u(t);
        es[(head + i) & (kGsSlots - 1u)] = (uint8_t)slot;
        GR.ev = pack32(head, n + 1u);
    }
    // a core became free: the first waiter gets it (Container FIFO, server.py:210-231) and starts its CPU step now
    AF_CORE void gs_core_release(AF_PLAN_AS uint64_t* g, uint32_t s0, double now, uint32_t rown) {
        const uint32_t head = lo32(GR.cq), n = hi32(GR.cq);
        if (n == 0u) {
            GR.cpu = GR.cpu + 1ull;   // cpu_free += 1
            return;
        }
        const uint32_t slot = gs_bytes(g, 1u)[head];
        GR.cq = pack32((head + 1u) & (kGsSlots - 1u), n - 1u);
        GR.cpu = GR.cpu - (1ull << 32);   // ready -= 1
        gs_point(s0, rown, -1);
        const uint64_t st = g[GS_STATE + slot];
        g[GS_STATE + slot] = st | (1ull << 16);   // holds the core
        gs_schedule(g, now + u2d(blob[A.off_row + af::TREC * (uint32_t)(st & 0xFFFFu)]), slot);
    }
    // the request in `slot` stands before step row `row` (the for-loop of _handle_request, server.py:197-276)
    AF_CORE void gs_advance(AF_PLAN_AS uint64_t* g, uint32_t sv, uint32_t slot, double now, uint32_t rown, bool& ram_released) {
        const uint32_t s0 = A.n_edges + 3u * sv;
        const uint64_t st = g[GS_STATE + slot];
        const uint32_t row = (uint32_t)(st & 0xFFFFu);
        const bool holds = (st >> 16) & 1ull, in_io = (st >> 17) & 1ull;
        const uint32_t kind = (uint32_t)blob[A.off_row + af::TREC * row + 2u];
        const double dur = u2d(blob[A.off_row + af::TREC * row]);
        if (kind == af::STEP_CPU) {   // server.py:199-231
            if (in_io) {
                GR.io = GR.io - 1ull;
                gs_point(s0 + 1u, rown, -1);
            }
            if (!holds) {
                const uint32_t cq_n = hi32(GR.cq);
                if (cq_n == 0u && lo32(GR.cpu) > 0u) {
                    GR.cpu = GR.cpu - 1ull;   // granted at once: never in the ready queue
                } else {
                    gs_bytes(g, 1u)[(lo32(GR.cq) + cq_n) & (kGsSlots - 1u)] = (uint8_t)slot;
                    GR.cq = pack32(lo32(GR.cq), cq_n + 1u);
                    GR.cpu = GR.cpu + (1ull << 32);   // ready += 1
                    gs_point(s0, rown, 1);
                    g[GS_STATE + slot] = (uint64_t)row;   // waiting: neither core nor I/O
                    return;
                }
            }
            g[GS_STATE + slot] = (uint64_t)row | (1ull << 16);
            gs_schedule(g, now + dur, slot);
            return;
        }
        if (kind == af::STEP_IO) {   // server.py:235-255 (its own Timeout is created before the core waiter's)
            if (!in_io) {
                GR.io = GR.io + 1ull;
                gs_point(s0 + 1u, rown, 1);
            }
            g[GS_STATE + slot] = (uint64_t)row | (1ull << 17);
            gs_schedule(g, now + dur, slot);
            if (holds) gs_core_release(g, s0, now, rown);
            return;
        }
        // the endpoint is through (server.py:257-276): core, RAM, the response
        if (holds) gs_core_release(g, s0, now, rown);
        if (in_io) {
            GR.io = GR.io - 1ull;
            gs_point(s0 + 1u, rown, -1);
        }
        const double need = u2d(g[GS_NEED + slot]);
        if (need > 0.0) {
            GR.ram = d2u(u2d(GR.ram) + need);
            gs_point(s0 + 2u, rown, -(int32_t)(need * A.ram_scale));
            ram_released = true;
        }
        const uint32_t nd = lo32(GR.dep);
        if (u2d(GR.lastdep) == now) why |= FLOW_WHY_TIE | FLOW_WHY_GEN_TIE;   // two responses at one instant: their order on the out-edge is SimPy's
        GR.lastdep = d2u(now);
        g[GS_DEPT + nd] = d2u(now);
        g[GS_DEPT0 + nd] = g[GS_T0 + slot];
        GR.dep = pack32(nd + 1u, hi32(GR.dep));
        GR.io = GR.io | (1ull << (32u + slot));   // the slot is free again
    }
    // RAM waiters, strictly FIFO with head-of-line blocking (Container._trigger_get, server.py:146-149)
    AF_CORE void gs_ram_queue(AF_PLAN_AS uint64_t* g, uint32_t sv, double now, uint32_t rown) {
        const uint32_t s0 = A.n_edges + 3u * sv;
        for (;;) {
            const uint32_t head = lo32(GR.rq), n = hi32(GR.rq);
            if (n == 0u) return;
            const uint32_t slot = gs_bytes(g, 2u)[head];
            const double need = u2d(g[GS_NEED + slot]), free_ram = u2d(GR.ram);
            if (free_ram < need) return;
            GR.rq = pack32((head + 1u) & (kGsSlots - 1u), n - 1u);
            GR.ram = d2u(free_ram - need);
            gs_point(s0 + 2u, rown, (int32_t)(need * A.ram_scale));
            bool again = false;
            gs_advance(g, sv, slot, now, rown, again);   // (an endpoint of RAM steps only gives its RAM straight back: the loop looks again)
        }
    }
    // ---- a SHARED instant of one server: several of its step ends at `now` (round 4) ----------------------------------------
    // Step times are constants of the plan, so once requests queue for a core the step ends of different requests coincide bit
    // for bit, and what happens next depends on the order SimPy runs the zero-time steps of the tied cascades in -- which request
    // stands first in the core queue, whose Timeout is created first (and so wins the NEXT tie), whose response goes out first.
    // SimPy's rule (heap key: time, priority, event id): every Timeout of the instant runs before anything the
    // instant itself schedules (they were created earlier: smaller ids), in creation order; whatever a step schedules "now" --
    // the Put that gives a core or the RAM back, the Get a waiter was granted -- goes to the back of ONE FIFO and its
    // continuation runs when it reaches the front.  That is af_core.hpp's micro_mode, restricted to what one server sees: events
    // of other nodes at the same instant touch other state, and a server's events only ever schedule events of that server, so
    // the server's subsequence of the global FIFO evolves exactly like a FIFO of its own.  The steps, in the reference's words:
    //   GM_STEP      a step's Timeout fires: the for-loop of _handle_request moves on (server.py:197-259)
    //   GM_CPU_GOT   `yield cpu_req` returns (server.py:220-231; _W: the request had been counted in the ready queue)
    //   GM_PUT_IO    `yield CPU.put(1)` before an I/O step returns: the Put's first callback grants waiters, then the step starts (:239-255)
    //   GM_PUT_END   `yield CPU.put(1)` at the end of the endpoint returns (:257-259)
    //   GM_RAM_PUT   `yield RAM.put(total_ram)` returns: waiters are admitted, the response leaves (:270-276)
    //   GM_RAM_GOT   `yield RAM.get(total_ram)` returns (:146-150)
    // The order in which this schedules new Timeouts IS their creation order, so later ties among them are exact too.
    enum : uint32_t { GM_STEP = 0u, GM_CPU_GOT = 1u, GM_CPU_GOT_W = 2u, GM_PUT_IO = 3u, GM_PUT_END = 4u, GM_RAM_PUT = 5u, GM_RAM_GOT = 6u };
    uint32_t gm_head, gm_n;
#if defined(AF_FUSED_ARRIVAL_PROBE)
    double probe_g = 0.0, probe_s = 0.0, probe_acc = 0.0;   // (measurement build only)
#endif
    uint32_t gs_rounds;   // server-station rounds of this scenario: solved at once << 16 | walked event by event (CNT_MAX_LIVE of a FEAT_GENSRV run)
    AF_CORE void gm_push(AF_PLAN_AS uint64_t* g, uint32_t kind, uint32_t slot) {
        if (gm_n >= kGsMq) {
            why |= FLOW_WHY_LIST;
            return;
        }
        ((AF_PLAN_AS uint8_t*)(g + GS_MQ))[(gm_head + gm_n) & (kGsMq - 1u)] = (uint8_t)((kind << 5) | slot);
        gm_n += 1u;
    }
    AF_CORE void gm_emit(AF_PLAN_AS uint64_t* g, uint32_t slot, double now, double dur) {
        if (!(now + dur > now)) why |= FLOW_WHY_TIE | FLOW_WHY_GEN_TIE;   // (a step too short to advance the f64 clock: SimPy queues it behind the instant's steps)
        gs_schedule(g, now + dur, slot);
    }
    // Container._trigger_get of the CPU container: waiters are served FIFO while cores are free; the first n_old entries had
    // been counted in the ready queue.  Returns the number of grants.
    AF_CORE uint32_t gm_cpu_trigger(AF_PLAN_AS uint64_t* g, uint32_t n_old) {
        uint32_t grants = 0u;
        for (;;) {
            const uint32_t head = lo32(GR.cq), n = hi32(GR.cq);
            if (n == 0u || lo32(GR.cpu) == 0u) return grants;
            const uint32_t slot = gs_bytes(g, 1u)[head];
            GR.cq = pack32((head + 1u) & (kGsSlots - 1u), n - 1u);
            GR.cpu = GR.cpu - 1ull;   // level -= 1
            gm_push(g, grants < n_old ? GM_CPU_GOT_W : GM_CPU_GOT, slot);
            grants += 1u;
        }
    }
    AF_CORE void gm_ram_trigger(AF_PLAN_AS uint64_t* g) {   // head-of-line blocking FIFO
        for (;;) {
            const uint32_t head = lo32(GR.rq), n = hi32(GR.rq);
            if (n == 0u) return;
            const uint32_t slot = gs_bytes(g, 2u)[head];
            const double need = u2d(g[GS_NEED + slot]), free_ram = u2d(GR.ram);
            if (free_ram < need) return;
            GR.rq = pack32((head + 1u) & (kGsSlots - 1u), n - 1u);
            GR.ram = d2u(free_ram - need);
            gm_push(g, GM_RAM_GOT, slot);
        }
    }
    AF_CORE void gm_depart(AF_PLAN_AS uint64_t* g, uint32_t slot, double now) {
        const uint32_t nd = lo32(GR.dep);
        if (nd >= kGsDeps) {
            why |= FLOW_WHY_LIST;
            return;
        }
        GR.lastdep = d2u(now);
        g[GS_DEPT + nd] = d2u(now);
        g[GS_DEPT0 + nd] = g[GS_T0 + slot];
        GR.dep = pack32(nd + 1u, hi32(GR.dep));
        GR.io = GR.io | (1ull << (32u + slot));   // the slot is free again
    }
    AF_CORE void gm_finish(AF_PLAN_AS uint64_t* g, uint32_t s0, uint32_t slot, bool in_io, double now, uint32_t rown) {   // server.py:261-276
        if (in_io) {
            GR.io = GR.io - 1ull;
            gs_point(s0 + 1u, rown, -1);
        }
        const double need = u2d(g[GS_NEED + slot]);
        if (need > 0.0) {
            GR.ram = d2u(u2d(GR.ram) + need);   // (ContainerPut succeeds at once; its continuation is queued)
            gs_point(s0 + 2u, rown, -(int32_t)(need * A.ram_scale));
            gm_push(g, GM_RAM_PUT, slot);
            return;
        }
        gm_depart(g, slot, now);
    }
    // the for-loop of _handle_request from step row `row` up to its next yield (server.py:197-259)
    AF_CORE void gm_continue(AF_PLAN_AS uint64_t* g, uint32_t s0, uint32_t slot, uint32_t row, bool holds, bool in_io, double now, uint32_t rown) {
        const uint32_t kind = (uint32_t)blob[A.off_row + af::TREC * row + 2u];
        const double dur = u2d(blob[A.off_row + af::TREC * row]);
        if (kind == af::STEP_CPU) {
            if (in_io) {
                GR.io = GR.io - 1ull;
                gs_point(s0 + 1u, rown, -1);
            }
            if (!holds) {   // cpu_req = CPU.get(1): append, trigger, `if not cpu_req.triggered` (server.py:210-217)
                const uint32_t cq_n = hi32(GR.cq);
                gs_bytes(g, 1u)[(lo32(GR.cq) + cq_n) & (kGsSlots - 1u)] = (uint8_t)slot;
                GR.cq = pack32(lo32(GR.cq), cq_n + 1u);
                g[GS_STATE + slot] = (uint64_t)row;
                if (gm_cpu_trigger(g, cq_n) <= cq_n) {   // still queued: ready += 1
                    GR.cpu = GR.cpu + (1ull << 32);
                    gs_point(s0, rown, 1);
                }
                return;
            }
            g[GS_STATE + slot] = (uint64_t)row | (1ull << 16);
            gm_emit(g, slot, now, dur);
            return;
        }
        if (kind == af::STEP_IO) {
            if (holds) {   // yield CPU.put(1)
                GR.cpu = GR.cpu + 1ull;
                g[GS_STATE + slot] = (uint64_t)row | (in_io ? 1ull << 17 : 0ull);
                gm_push(g, GM_PUT_IO, slot);
                return;
            }
            if (!in_io) {
                GR.io = GR.io + 1ull;
                gs_point(s0 + 1u, rown, 1);
            }
            g[GS_STATE + slot] = (uint64_t)row | (1ull << 17);
            gm_emit(g, slot, now, dur);
            return;
        }
        if (holds) {   // the endpoint is through while holding the core: yield CPU.put(1)
            GR.cpu = GR.cpu + 1ull;
            g[GS_STATE + slot] = (uint64_t)row | (in_io ? 1ull << 17 : 0ull);
            gm_push(g, GM_PUT_END, slot);
            return;
        }
        gm_finish(g, s0, slot, in_io, now, rown);
    }
    // every step end of server sv at `now` (the first n_now entries of its ring), then the FIFO until it is empty
    AF_CORE void gs_instant(AF_PLAN_AS uint64_t* g, uint32_t sv, double now, uint32_t rown) {
        const uint32_t s0 = A.n_edges + 3u * sv;
        gm_head = gm_n = 0u;
        for (;;) {   // the instant's Timeouts, in creation order (nothing scheduled in here lands at `now`: gm_emit)
            const uint32_t ev_head = lo32(GR.ev), ev_n = hi32(GR.ev);
            if (ev_n == 0u || u2d(g[GS_EVT + ev_head]) != now) break;
            const uint32_t slot = gs_bytes(g, 0u)[ev_head];
            GR.ev = pack32((ev_head + 1u) & (kGsSlots - 1u), ev_n - 1u);
            ev += 1u;
            const uint64_t st = g[GS_STATE + slot];
            gm_continue(g, s0, slot, ((uint32_t)st & 0xFFFFu) + 1u, (st >> 16) & 1ull, (st >> 17) & 1ull, now, rown);
        }
        while (gm_n != 0u && why == 0u) {
            const uint32_t w = ((AF_PLAN_AS uint8_t*)(g + GS_MQ))[gm_head];
            gm_head = (gm_head + 1u) & (kGsMq - 1u);
            gm_n -= 1u;
            const uint32_t kind = w >> 5, slot = w & 31u;
            const uint64_t st = g[GS_STATE + slot];
            const uint32_t row = (uint32_t)st & 0xFFFFu;
            const bool in_io = (st >> 17) & 1ull;
            if (kind == GM_CPU_GOT || kind == GM_CPU_GOT_W) {
                if (kind == GM_CPU_GOT_W) {
                    GR.cpu = GR.cpu - (1ull << 32);   // ready -= 1
                    gs_point(s0, rown, -1);
                }
                g[GS_STATE + slot] = (uint64_t)row | (1ull << 16);
                gm_emit(g, slot, now, u2d(blob[A.off_row + af::TREC * row]));
            } else if (kind == GM_PUT_IO) {
                gm_cpu_trigger(g, 0xFFFFFFFFu);
                if (!in_io) {
                    GR.io = GR.io + 1ull;
                    gs_point(s0 + 1u, rown, 1);
                }
                g[GS_STATE + slot] = (uint64_t)row | (1ull << 17);
                gm_emit(g, slot, now, u2d(blob[A.off_row + af::TREC * row]));
            } else if (kind == GM_PUT_END) {
                gm_cpu_trigger(g, 0xFFFFFFFFu);
                gm_finish(g, s0, slot, in_io, now, rown);
            } else if (kind == GM_RAM_PUT) {
                gm_ram_trigger(g);
                gm_depart(g, slot, now);
            } else {   // GM_RAM_GOT (server.py:149-150)
                gs_point(s0 + 2u, rown, (int32_t)(u2d(g[GS_NEED + slot]) * A.ram_scale));
                gm_continue(g, s0, slot, row, false, false, now, rown);
            }
        }
    }

    AF_CORE uint32_t gen_servers(uint32_t sv, double limit) {
        AF_PLAN_AS uint64_t* g = gs(sv);
        AF_PLAN_AS uint32_t* lw = lbw();
        const uint32_t off = lw[LBW_SEG_OFF + sv], n_k = lw[LBW_SEG_LEN + sv], s0 = A.n_edges + 3u * sv;
        const uint64_t meta = blob[A.off_srv + af::SREC * sv + 1u];
        const uint32_t epb = (uint32_t)(meta >> 32) & 0xFFFFu;
        const double ram_mb = u2d(blob[A.off_srv + af::SREC * sv]);
        uint32_t ai = 0u, done = 0u;
        bool ram_pending = false;
        gs_load(g);
        GR.dep = pack32(0u, hi32(GR.dep));
        for (;;) {
            const double ta = ai < n_k ? seg(0)[off + ai] : AF_INF;
            const uint32_t ev_head = lo32(GR.ev), ev_n = hi32(GR.ev);
            const double te = ev_n ? u2d(g[GS_EVT + ev_head]) : AF_INF;
            const double now = ta < te ? ta : te;
            if (!(now < limit)) break;
            const bool tie_next = te < ta && ev_n > 1u && u2d(g[GS_EVT + ((ev_head + 1u) & (kGsSlots - 1u))]) == te;
            const bool tie_prev = now == u2d(GR.last);
            // an arrival exactly at a step end (or at the instant a step end was handled in): the arrival's place among the
            // instant's zero-time steps is decided by events of OTHER nodes (the edge's Timeout, the inbox Store): handed back.
            // (With continuous edge latencies that is a null event; step ends sharing an instant are not: gs_instant.)
            const bool give_up = ta == te || tie_prev;
            if (give_up) {
#if defined(AF_FLOW_TRACE) && !defined(__HIP_DEVICE_COMPILE__)
                std::fprintf(stderr, "gen tie: sv %u ta %.17g te %.17g ev_n %u\n", sv, ta, te, ev_n);
#endif
                why |= FLOW_WHY_TIE | FLOW_WHY_GEN_TIE;   // the next-event kernels replay SimPy's event-by-event order
                break;
            }
            GR.last = d2u(now);
            if (lo32(GR.dep) >= kGsDeps) {   // (cannot happen: a round's departures <= requests inside + its arrivals)
                why |= FLOW_WHY_LIST;
                break;
            }
            // (an arrival's tick row and endpoint draw were worked out by its own lane: run())
            const uint64_t pre = te < ta ? 0ull : d2u(seg(2)[off + ai]);
            const uint32_t rown = samples == nullptr ? 0u : te < ta ? tick_index(now, true) : hi32(pre);
            bool ram_released = false;
            done += 1u;
            if (tie_next) {   // several step ends of this server at one instant: SimPy's order of their zero-time steps
                gs_instant(g, sv, now, rown);
                if (why != 0u) break;
                continue;
            }
            if (te < ta) {   // a CPU or I/O step ends
                const uint32_t slot = gs_bytes(g, 0u)[ev_head];
                GR.ev = pack32((ev_head + 1u) & (kGsSlots - 1u), ev_n - 1u);
                ev += 1u;
                const uint64_t st = g[GS_STATE + slot];
                g[GS_STATE + slot] = (st & ~0xFFFFull) | (uint64_t)(((uint32_t)st & 0xFFFFu) + 1u);   // next row; core / I/O as they were
                gs_advance(g, sv, slot, now, rown, ram_released);
            } else {         // a request arrives (server.py:303-313, 79-149)
                GR.arr = GR.arr + 1ull;   // (the arrival count: index of the next arrival's endpoint draw, run())
                const uint32_t pick = lo32(pre);
                const double need = u2d(blob[A.off_ep + af::PREC * (epb + pick)]);
                const uint32_t row0 = (uint32_t)blob[A.off_ep + af::PREC * (epb + pick) + 1u];
                const double t0a = seg(1)[off + ai];
                ai += 1u;
                const bool blocked = hi32(GR.arr) != 0u;
                if (need > 0.0 && (need > ram_mb || blocked)) {   // waits for good, and so does every RAM request behind it
                    info |= af::FLAG_RAM_STARVED;
                    GR.arr = pack32(lo32(GR.arr), 1u);
                } else {
                    const uint32_t free_mask = hi32(GR.io);
                    if (free_mask == 0u) {
                        why |= FLOW_WHY_LIST;   // more requests inside this server than the station holds
                        break;
                    }
                    const uint32_t slot = (uint32_t)__builtin_ctz(free_mask);
                    GR.io = GR.io & ~(1ull << (32u + slot));
                    g[GS_T0 + slot] = d2u(t0a);
                    g[GS_NEED + slot] = d2u(need);
                    g[GS_STATE + slot] = (uint64_t)row0;
                    bool go = true;
                    if (need > 0.0) {
                        const uint32_t rq_n = hi32(GR.rq);
                        const double free_ram = u2d(GR.ram);
                        if (rq_n == 0u && free_ram >= need) {
                            GR.ram = d2u(free_ram - need);
                            gs_point(s0 + 2u, rown, (int32_t)(need * A.ram_scale));
                        } else {
                            gs_bytes(g, 2u)[(lo32(GR.rq) + rq_n) & (kGsSlots - 1u)] = (uint8_t)slot;
                            GR.rq = pack32(lo32(GR.rq), rq_n + 1u);
                            go = false;
                        }
                    }
                    if (go) gs_advance(g, sv, slot, now, rown, ram_released);
                }
            }
            // RAM waiters come in when every step end of this instant has had its turn: in SimPy the Put that frees the RAM
            // is processed one or two zero-time events after the Timeout, behind the other Timeouts of the instant -- a request
            // of THOSE for a core stands in the queue before the admitted waiter's (tests/test_flow_hostcheck.py, tie storm 30)
            ram_pending = ram_pending || ram_released;
            if (ram_pending && !tie_next) {
                gs_ram_queue(g, sv, now, rown);
                ram_pending = false;
            }
        }
        gs_store(g);
        return done;
    }

    // ---- general servers, a whole ROUND at once (round 5: VERDICT r4 item 4) ---------------------------------------------------
    // gen_servers() above is exact but one lane per server walks its events one by one: a chain of dependent LDS round trips,
    // ~2 600 wave-cycles per server event with 2 of 64 lanes busy (LB-2).  Here a LANE IS A REQUEST -- the ones inside the servers
    // of this pass (in the order of the pending-step ring, then of the core queue) and the round's arrivals -- and the whole window
    // [previous horizon, `limit`) is solved at once:
    //   * a request's timeline is a function of its own start and of the times its core acquisitions are granted (server.py:197-259:
    //     RAM first, a core at the first CPU step of a burst, released at the next I/O step or at the end);
    //   * a ONE-core server grants in the order of the requests' CPU.get() calls (Container FIFO), so the grant of an acquisition
    //     that asks at r is  s = max(r, release of the acquisition that asked last before r)  -- the recurrence of servers_solve()
    //     without the assumption that the order is the arrival order;
    //   * relaxation: every lane walks its step program with the grants it knows (none at first), then looks up its predecessors
    //     in the current order of the r -- all lanes against all lanes, through the crossbar -- and walks again until nothing
    //     changes.  A fixed point satisfies the FIFO recurrence in its own order, and that recurrence has one solution (induction over
    //     the order), so the fixed point IS the event-by-event result: the same f64 additions, request by request.
    // Everything at or after `limit` is tentative (later arrivals can get in front of it) and only has to stay at or after
    // `limit`: a walk stops at its first such time, which is the request's state for the next round -- exactly the state gen_servers()
    // keeps (pending step end / place in the core queue), so either form can run any round.
    // With c cores the grant is max(r, the c-th LATEST release among the acquisitions that asked before r) -- the k-th request of a
    // Container FIFO is granted when fewer than c of the k - 1 before it still hold a core; c <= kParCores.
    // What the solver does not decide it leaves to gen_servers(), BEFORE touching any state (return false): more than four cores, a RAM
    // queue that is or could become non-empty, more than 64 requests in the window, step programs with more than kParBursts core
    // acquisitions or kParSteps steps ahead, and every instant at which the ORDER of two events of a server matters -- two CPU.get()
    // at one instant, two responses at one instant, two pending step ends at one instant (their creation order decides later
    // ties: gs_instant).  An event that merely coincides with another of the same server without competing for the core (a step end
    // at an arrival's instant, a release at a request's instant: the grant is at that instant either way, and the zero-length wait
    // it may be counted for ends before any tick sees it -- a tick AT the instant is flagged by tick_index) needs no order.
    static constexpr uint32_t kParBursts = 2u, kParSteps = 24u, kParIters = 24u, kParCores = 4u;
    static constexpr uint32_t kPairU = 8u;   // keys of the all-pairs loops in flight at once
    // 128 LDS words of the solver behind the servers' state (FlowLayout::off_gsrv; make_flow_layout)
    AF_CORE AF_PLAN_AS double* par_words() const { return (AF_PLAN_AS double*)(M + A.L.off_gsrv + A.n_servers * kGsWords); }
#if defined(AF_PAR_TRACE) && !defined(__HIP_DEVICE_COMPILE__)
#define AF_PAR_LEAVE(why_text) do { if (lane == 0u) std::fprintf(stderr, "par: left to gen_servers (%s), R %u limit %.9g\n", why_text, R, limit); return false; } while (0)
#else
#define AF_PAR_LEAVE(why_text) return false
#endif
    AF_CORE bool gen_servers_par(uint32_t level, double limit, uint32_t& done_any) {
        AF_PLAN_AS uint32_t* lw = lbw();
        const uint32_t S = A.n_servers;
#if defined(AF_PAR_OFF)
        return false;   // (test / measurement hook: every round by the event-by-event walk)
#endif
        // ---- lanes: per server of this pass its running requests, its core waiters, this round's arrivals
        uint32_t base = 0u, sv = 0u, role = 3u, idx = 0u, my_base = 0u, n_mine = 0u, blk_max = 0u;   // (blk_max: the largest server block, wave-uniform)
        uint32_t cores_max = 1u;   // the widest server of this pass (wave-uniform)
        bool ok = true;
        for (uint32_t k = 0u; k < S; ++k) {
            if (kChain && level_of(k) != level) continue;
            const AF_PLAN_AS uint64_t* gk = gs(k);
            const uint32_t n_run = hi32(gk[GS_EV]), n_wait = hi32(gk[GS_CQ]), n_new = lw[LBW_SEG_LEN + k];
            const uint32_t cores = (uint32_t)blob[A.off_srv + af::SREC * k + 1u] & 0xFFFFu;
            ok = ok && cores <= kParCores && hi32(gk[GS_RQ]) == 0u && hi32(gk[GS_ARR]) == 0u;
            cores_max = cores > cores_max ? cores : cores_max;
            const uint32_t n_k = n_run + n_wait + n_new;
            blk_max = n_k > blk_max ? n_k : blk_max;
            if (lane >= base && lane < base + n_k) {
                sv = k;
                my_base = base;
                n_mine = n_k;
                idx = lane - base;
                role = idx < n_run ? 0u : idx < n_run + n_wait ? 1u : 2u;
                idx -= role == 0u ? 0u : role == 1u ? n_run : n_run + n_wait;
            }
            base += n_k;
        }
        const uint32_t R = base;
        if (!ok || R > 64u) AF_PAR_LEAVE(!ok ? "cores / RAM queue" : "more than 64 requests");
        const bool mine = role != 3u;
        AF_PLAN_AS uint64_t* g = gs(sv);
        const uint32_t s0 = A.n_edges + 3u * sv;
        // ---- my request as gen_servers() left it, or as it arrives
        double t_start = AF_INF, t0v = 0.0, need = 0.0;
        uint32_t row_start = 0u, a_row = 0u;
        bool holds0 = false, io0 = false;
        if (role == 0u) {
            const uint32_t p = (lo32(g[GS_EV]) + idx) & (kGsSlots - 1u), slot = gs_bytes(g, 0u)[p];
            const uint64_t st = g[GS_STATE + slot];
            t_start = u2d(g[GS_EVT + p]);
            row_start = (uint32_t)st & 0xFFFFu;
            holds0 = ((st >> 16) & 1ull) != 0ull;
            io0 = ((st >> 17) & 1ull) != 0ull;
            t0v = u2d(g[GS_T0 + slot]);
            need = u2d(g[GS_NEED + slot]);
        } else if (role == 1u) {
            const uint32_t p = (lo32(g[GS_CQ]) + idx) & (kGsSlots - 1u), slot = gs_bytes(g, 1u)[p];
            t_start = -(double)(64u - idx);   // asked before everything of this window, in queue order
            row_start = (uint32_t)g[GS_STATE + slot] & 0xFFFFu;
            t0v = u2d(g[GS_T0 + slot]);
            need = u2d(g[GS_NEED + slot]);
        } else if (role == 2u) {
            const uint32_t at = lw[LBW_SEG_OFF + sv] + idx;
            const uint64_t pre = d2u(seg(2)[at]);
            const uint32_t epb = (uint32_t)(blob[A.off_srv + af::SREC * sv + 1u] >> 32) & 0xFFFFu;
            t_start = seg(0)[at];
            t0v = seg(1)[at];
            a_row = hi32(pre);
            need = u2d(blob[A.off_ep + af::PREC * (epb + lo32(pre))]);
            row_start = (uint32_t)blob[A.off_ep + af::PREC * (epb + lo32(pre)) + 1u];
        }
        const double ram_mb = u2d(blob[A.off_srv + af::SREC * sv]);
        bool hazard = role == 2u && need > ram_mb;   // (waits for good: FLAG_RAM_STARVED is gen_servers()'s to report)
        prof(PROF_PAR_SETUP);

        // ---- the walk: my request from where it stands up to its first time >= limit, with the grants G[] it knows
        double G[kParBursts], r[kParBursts], rel[kParBursts];
#pragma unroll
        for (uint32_t b = 0u; b < kParBursts; ++b) G[b] = -AF_INF;
        uint32_t cls = 3u, fin_row = 0u, n_ev = 0u;   // cls: 0 left the server, 1 a step is pending at limit, 2 waits for the core at limit
        double fin_key = AF_INF;
        bool fin_holds = false, fin_io = false;
        // (round 6: ONE straight line per step.  A lane is a request, so in every step some lanes stand before a CPU step, some
        // before an I/O step and some at the end of their endpoint: as nested branches the wave ran all of them one after the
        // other with the lane-varying booleans kept as scalar masks that every join merges -- ~200 instructions per step, most of
        // them scalar, the two words of the step row fetched one after the other.  Here every lane evaluates the three cases'
        // predicates and the state moves on through selects; only the series' entries sit in divergent regions.)
        const int32_t need_w = (int32_t)(need * A.ram_scale);
        auto walk = [&](bool commit) {
#pragma unroll
            for (uint32_t b = 0u; b < kParBursts; ++b) {
                r[b] = AF_INF;
                rel[b] = AF_INF;
            }
            double tt = t_start;
            uint32_t rw = row_start, nb = 0u, open = 0u;
            bool h = holds0, io = io0, alive = mine, pending = role == 0u, queued = role == 1u;
            n_ev = 0u;
            cls = 3u;
            if (holds0) {   // (the acquisition I hold was granted in an earlier round: first in the order, the holders among themselves in ring order)
                r[0] = -1000.0 - (double)idx;
                nb = 1u;
            }
            const bool ser = commit && samples != nullptr;   // (wave-uniform)
            if (ser && role == 2u && need > 0.0) add_point(s0 + 2u, a_row, need_w);
            for (uint32_t step = 0u; step < kParSteps; ++step) {
                if (!W::any(alive)) break;
                // the Timeout of step rw fires at tt: beyond the window it is the request's state for the next round
                const bool fire = alive && pending, in_win = tt < limit;
                const bool stop1 = fire && !in_win, adv = fire && in_win;
                cls = stop1 ? 1u : cls;
                fin_key = stop1 ? tt : fin_key;
                fin_row = stop1 ? rw : fin_row;
                fin_holds = stop1 ? h : fin_holds;
                fin_io = stop1 ? io : fin_io;
                alive = alive && !stop1;
                n_ev += adv ? 1u : 0u;
                rw += adv ? 1u : 0u;
                pending = pending && !adv;
                // (both words of the row at once, by every lane: a lane that is through reads the row it stopped at)
                const uint32_t kind = (uint32_t)blob[A.off_row + af::TREC * rw + 2u];
                const double dur = u2d(blob[A.off_row + af::TREC * rw]);
                // (one tick row per step: the time the step is reached at; a grant's own row below)
                const bool want_row = ser && alive && !queued;
                uint32_t rown = 0u;
                if (want_row) rown = (role == 2u && step == 0u) ? a_row : tick_index(tt, true);
                const bool is_cpu = alive && kind == af::STEP_CPU, is_io = alive && kind == af::STEP_IO, is_end = alive && !is_cpu && !is_io;
                // a CPU step of a request that does not hold the core: CPU.get() at rb, granted at max(rb, what it knows of its predecessor)
                const bool need_core = is_cpu && !h;
                const bool hz = need_core && nb >= kParBursts, acq = need_core && nb < kParBursts;
                double Gn = G[0];
#pragma unroll
                for (uint32_t b = 1u; b < kParBursts; ++b) Gn = nb == b ? G[b] : Gn;
                const double rb = tt, sg = Gn > rb ? Gn : rb;
#pragma unroll
                for (uint32_t b = 0u; b < kParBursts; ++b) r[b] = (acq && nb == b) ? rb : r[b];
                const bool waits = queued || sg > rb, sg_in = sg < limit;
                const bool stay = acq && !sg_in, got = acq && sg_in;   // stay: still in the core queue when the window ends
                if (ser) {
                    const bool io_down = (is_cpu || is_end) && io, io_up = is_io && !io;
                    add_point(s0 + 1u, rown, io_up ? 1 : -1, want_row && (io_down || io_up));
                    add_point(s0, rown, 1, want_row && acq && waits);   // (want_row: not a waiter of an earlier round, whose +1 was entered then)
                    if (got && waits) add_point(s0, tick_index(sg, true), -1);
                    add_point(s0 + 2u, rown, -need_w, want_row && is_end && need > 0.0);
                }
                cls = stay ? 2u : cls;
                fin_key = stay ? rb : fin_key;
                fin_row = stay ? rw : fin_row;
                hazard = hazard || hz;
                alive = alive && !stay && !hz;
                tt = got ? sg : tt;
                open = got ? nb : open;
                nb += got ? 1u : 0u;
                queued = queued && !got;
                // an I/O step or the end of the endpoint gives the core back (server.py:239-259)
                const bool give = (is_io || is_end) && h;
#pragma unroll
                for (uint32_t b = 0u; b < kParBursts; ++b) rel[b] = (give && open == b) ? tt : rel[b];
                h = (h || got) && !is_io;
                io = is_cpu ? false : is_io ? true : io;
                // the step's own Timeout
                const bool timed = (is_cpu && alive) || is_io;
                const double tn = tt + dur;
                hazard = hazard || (timed && !(tn > tt));
                tt = timed ? tn : tt;
                pending = pending || timed;
                // the endpoint is through (server.py:257-276)
                cls = is_end ? 0u : cls;
                fin_key = is_end ? tt : fin_key;
                alive = alive && !is_end;
            }
            hazard = hazard || alive;   // more steps ahead than the walk takes
        };

        // ---- relaxation to the fixed point of the FIFO recurrence
        // A lane finds the predecessors of its acquisitions by RANK: every lane publishes its request times, counts the ones of
        // its own server below each of its own (a loop over the server's block of lanes, one LDS read and four VALU operations per
        // pair -- round 5's first form compared all lanes with all lanes through v_readlane, 14 operations per pair, 75 % of the
        // station's time), publishes its release times at those places and reads the place in front of it.
        AF_PLAN_AS double* keys = seg(3);                                  // [64][kParBursts]: seg(3), seg(4) are free in this station
        AF_PLAN_AS double* sorted_rel = par_words();                       // [64][kParBursts]
        AF_PLAN_AS uint32_t* place_id = eb();                              // [64][kParBursts]: select_big()'s per-entry words are free in this station
        const uint32_t e0 = kParBursts * my_base, n_e = mine ? kParBursts * n_mine : 0u;
        bool settled = false;
        for (uint32_t it = 0u; it < kParIters && !settled; ++it) {
            walk(false);
            prof(PROF_PAR_WALK);
            if (kProf) prof_acc[PROF_N_PAR_ITERS] += 1ull;
            if (W::any(hazard)) AF_PAR_LEAVE("a step program outside the walk's range");
            W::sync();   // (the previous iteration's reads of keys / sorted_rel are done)
            if (mine)
#pragma unroll
                for (uint32_t b = 0u; b < kParBursts; ++b) keys[kParBursts * lane + b] = r[b];
            W::sync();
            uint32_t lt[kParBursts];
#pragma unroll
            for (uint32_t b = 0u; b < kParBursts; ++b) lt[b] = 0u;
            // (round 6: kPairU keys fetched before the first of them is compared -- the loads are unconditional, what lies behind
            // the block is masked by the comparison of the index -- instead of one masked LDS read, a wait and eight VALU
            // operations per trip; and only the keys BELOW mine are counted: two acquisitions with one request time get the same
            // place, which the place's id shows -- each writes its own, one of them reads the other's back)
            for (uint32_t i0 = 0u; i0 < kParBursts * blk_max; i0 += kPairU) {
                double kq[kPairU];
#pragma unroll
                for (uint32_t u = 0u; u < kPairU; ++u) kq[u] = keys[(e0 + i0 + u) & (64u * kParBursts - 1u)];   // (inside the array whatever the lane's block)
#pragma unroll
                for (uint32_t u = 0u; u < kPairU; ++u) {
                    const double ko = i0 + u < n_e ? kq[u] : AF_INF;
#pragma unroll
                    for (uint32_t b = 0u; b < kParBursts; ++b) lt[b] += ko < r[b] ? 1u : 0u;
                }
            }
#pragma unroll
            for (uint32_t b = 0u; b < kParBursts; ++b)
                if (mine && r[b] < AF_INF) {
                    sorted_rel[e0 + lt[b]] = rel[b];
                    place_id[e0 + lt[b]] = kParBursts * lane + b;
                }
            W::sync();
            bool changed = false, tie = false;
#pragma unroll
            for (uint32_t b = 0u; b < kParBursts; ++b)   // another CPU.get() of this server at my instant took my place (or I took its)
                tie = tie || (mine && r[b] < AF_INF && place_id[e0 + lt[b]] != kParBursts * lane + b);
#pragma unroll
            for (uint32_t b = 0u; b < kParBursts; ++b) {
                // one core: the acquisition in front of mine releases last of all before me.  c cores (Container FIFO: the k-th
                // request is granted when fewer than c of the k - 1 before it still run): the c-th LATEST release among them
                double found = (mine && r[b] < AF_INF && lt[b] > 0u) ? sorted_rel[e0 + lt[b] - 1u] : -AF_INF;
                if (cores_max > 1u) {   // (wave-uniform)
                    double top[kParCores];
#pragma unroll
                    for (uint32_t c = 0u; c < kParCores; ++c) top[c] = -AF_INF;
                    const uint32_t n_before = (mine && r[b] < AF_INF) ? lt[b] : 0u;
                    for (uint32_t i0 = 0u; i0 < kParBursts * blk_max; i0 += kPairU) {   // (loads first: see the rank loop)
                        double xq[kPairU];
#pragma unroll
                        for (uint32_t u = 0u; u < kPairU; ++u) xq[u] = sorted_rel[(e0 + i0 + u) & (64u * kParBursts - 1u)];
#pragma unroll
                        for (uint32_t u = 0u; u < kPairU; ++u) {
                            double x = i0 + u < n_before ? xq[u] : -AF_INF;
#pragma unroll
                            for (uint32_t c = 0u; c < kParCores; ++c) {   // insertion into the descending top-c list
                                const bool up = x > top[c];
                                const double t2 = up ? top[c] : x;
                                top[c] = up ? x : top[c];
                                x = t2;
                            }
                        }
                    }
                    const uint32_t my_cores = (uint32_t)blob[A.off_srv + af::SREC * sv + 1u] & 0xFFFFu;
                    double kth = -AF_INF;
#pragma unroll
                    for (uint32_t c = 0u; c < kParCores; ++c) kth = c + 1u == my_cores ? top[c] : kth;
                    found = my_cores > 1u ? kth : found;
                }
                // (what binds is max(r, G): a predecessor that released before I asked changes nothing)
                const double was = G[b] > r[b] ? G[b] : r[b], now = found > r[b] ? found : r[b];
                changed = changed || (r[b] < AF_INF && was != now);
                G[b] = found;
            }
            settled = !W::any(changed);
            prof(PROF_PAR_RANK);
            if (settled && W::any(tie)) AF_PAR_LEAVE("two CPU.get() at one instant");
        }
        if (!settled) AF_PAR_LEAVE("no fixed point within kParIters");

        // ---- where everybody stands at `limit`: places among the responses / pending step ends / core waiters of my server
        // (RAM: every arrival must find its need at once -- the level at its instant is what the round began with, less what the
        // arrivals before it took, plus what left before it; needs are multiples of 1/256 MB, so these sums are exact in any order)
        // (round 6: two words per peer -- its time, and class | role | RAM need in units of 1 / ram_scale MB in one u32 -- fetched
        // kPairU peers ahead; what the arrivals before mine took and the servers' totals are prefix sums over the lanes: a server's
        // block is contiguous and its arrivals stand in it in time order.  Round 5's loop read four words per peer one peer at a
        // time and kept four f64 sums.)
        uint32_t rank = 0u, back_u = 0u;
        bool tie = false;
        AF_PLAN_AS double* p_key = seg(3);
        AF_PLAN_AS uint32_t* p_meta = place_id;   // (the relaxation is over)
        const double need_s = need * A.ram_scale;
        const uint32_t need_u = (mine && need_s < 16777216.0) ? (uint32_t)need_s : 0u;
        if (W::any(mine && (double)need_u != need_s)) AF_PAR_LEAVE("a RAM need that is not a small multiple of the unit");
        W::sync();
        if (mine) {
            p_key[lane] = fin_key;
            p_meta[lane] = cls | (role << 2) | (need_u << 4);
        }
        W::sync();
        for (uint32_t i0 = 0u; i0 < blk_max; i0 += kPairU) {   // (loads first: see the rank loop)
            uint32_t mq[kPairU];
            double kq[kPairU];
#pragma unroll
            for (uint32_t u = 0u; u < kPairU; ++u) {
                const uint32_t o = (my_base + i0 + u) & 63u;   // (lanes past my block read somebody's words: masked below)
                mq[u] = p_meta[o];
                kq[u] = p_key[o];
            }
#pragma unroll
            for (uint32_t u = 0u; u < kPairU; ++u) {
                const bool in = mine && i0 + u < n_mine;
                const bool peer = in && (mq[u] & 3u) == cls;
                rank += peer && kq[u] < fin_key ? 1u : 0u;
                tie = tie || (peer && kq[u] == fin_key && my_base + i0 + u != lane && cls != 2u);
                back_u += (in && (mq[u] & 3u) == 0u && kq[u] < t_start) ? mq[u] >> 4 : 0u;   // RAM that came back before my arrival
            }
        }
        const uint32_t last = (my_base + (n_mine ? n_mine - 1u : 0u)) & 63u;
        const uint32_t new_u = role == 2u ? need_u : 0u, gone_u = (mine && cls == 0u) ? need_u : 0u;
        const uint32_t new_incl = W::scan_incl_u32(new_u), gone_incl = W::scan_incl_u32(gone_u);
        const uint32_t new_base = W::shfl32(new_incl - new_u, my_base), gone_base = W::shfl32(gone_incl - gone_u, my_base);
        const double took_before = (double)(new_incl - new_u - new_base) * A.ram_unit, back_before = (double)back_u * A.ram_unit;
        const double need_new = (double)(W::shfl32(new_incl, last) - new_base) * A.ram_unit;
        const double need_gone = (double)(W::shfl32(gone_incl, last) - gone_base) * A.ram_unit;
        if (W::any(tie && mine)) AF_PAR_LEAVE("two responses / two pending step ends at one instant");
        // per server: how many leave, stay with a pending step, stay in the core queue; RAM must never have run short
        uint32_t n_dep = 0u, n_run1 = 0u, n_wait1 = 0u;
        bool fits = true;
        for (uint32_t k = 0u; k < S; ++k) {
            if (kChain && level_of(k) != level) continue;
            const uint32_t d = popc64(W::ballot(mine && sv == k && cls == 0u)), a1 = popc64(W::ballot(mine && sv == k && cls == 1u)),
                           w1 = popc64(W::ballot(mine && sv == k && cls == 2u));
            fits = fits && a1 + w1 <= kGsSlots && d <= kGsDeps;
            if (sv == k) {
                n_dep = d;
                n_run1 = a1;
                n_wait1 = w1;
            }
        }
        const bool ram_short = role == 2u && need > 0.0 && u2d(g[GS_RAM]) - took_before + back_before < need;
        if (!fits || W::any(ram_short)) AF_PAR_LEAVE(!fits ? "more requests inside than slots" : "RAM could run short");
        prof(PROF_PAR_STANDING);

        // ---- commit: series and counts of the window's events, the servers' state at `limit`, the responses in time order
        walk(true);
        prof(PROF_PAR_COMMIT_WALK);
        ev += n_ev;
        done_any = W::any(n_ev != 0u || role == 2u) ? 1u : 0u;
        W::sync();
        const uint32_t arrivals_k = lw[LBW_SEG_LEN + sv];
        const double ram_now = u2d(g[GS_RAM]) - need_new + need_gone;
        const uint32_t n_hold = popc64(W::ballot(mine && cls == 1u && fin_holds)), n_io_all = 0u;
        (void)n_hold;
        (void)n_io_all;
        if (mine && cls == 0u) {
            g[GS_DEPT + rank] = d2u(fin_key);
            g[GS_DEPT0 + rank] = d2u(t0v);
        } else if (mine && cls == 1u) {
            g[GS_EVT + rank] = d2u(fin_key);
            gs_bytes(g, 0u)[rank] = (uint8_t)rank;
            g[GS_STATE + rank] = (uint64_t)fin_row | (fin_holds ? 1ull << 16 : 0ull) | (fin_io ? 1ull << 17 : 0ull);
            g[GS_T0 + rank] = d2u(t0v);
            g[GS_NEED + rank] = d2u(need);
        } else if (mine && cls == 2u) {
            const uint32_t slot = n_run1 + rank;
            gs_bytes(g, 1u)[rank] = (uint8_t)slot;
            g[GS_STATE + slot] = (uint64_t)fin_row;
            g[GS_T0 + slot] = d2u(t0v);
            g[GS_NEED + slot] = d2u(need);
        }
        for (uint32_t k = 0u; k < S; ++k) {   // the servers' scalar words, by the first lane of each server's block (or lane k for an idle server)
            if (kChain && level_of(k) != level) continue;
            const uint64_t in_k = W::ballot(mine && sv == k);
            const uint32_t holders = popc64(W::ballot(mine && sv == k && cls == 1u && fin_holds)),
                           in_io_k = popc64(W::ballot(mine && sv == k && cls == 1u && fin_io));
            const bool writer = in_k != 0ull ? lane == (uint32_t)__builtin_ctzll(in_k) : lane == k;
            if (writer) {
                AF_PLAN_AS uint64_t* gk = gs(k);
                if (in_k != 0ull) {
                    const uint32_t inside = n_run1 + n_wait1;
                    gk[GS_EV] = pack32(0u, n_run1);
                    gk[GS_CQ] = pack32(0u, n_wait1);
                    gk[GS_CPU] = pack32(((uint32_t)blob[A.off_srv + af::SREC * k + 1u] & 0xFFFFu) - holders, n_wait1);
                    gk[GS_IO] = pack32(in_io_k, inside >= 32u ? 0u : ~((1u << inside) - 1u));
                    gk[GS_RAM] = d2u(ram_now);
                    gk[GS_ARR] = pack32(lo32(gk[GS_ARR]) + arrivals_k, 0u);
                    gk[GS_DEP] = pack32(n_dep, hi32(gk[GS_DEP]));
                } else {
                    gk[GS_DEP] = pack32(0u, hi32(gk[GS_DEP]));
                }
            }
        }
        W::sync();
        prof(PROF_PAR_FINAL);
        if (kProf) {
            prof_acc[PROF_N_PAR_ROUNDS] += 1ull;
            prof_acc[PROF_N_PAR_LANES] += R;
        }
        return true;
    }

    // ---- completion (client.py:62-69) -------------------------------------------------------------------
    AF_CORE void complete(bool have, uint32_t r, double t0, double now) {
        const uint32_t at = n_comp + r;
        if (clock != nullptr) {
            if (have && at < A.clock_cap) {
                clock[2u * (size_t)at] = t0;
                clock[2u * (size_t)at + 1u] = now;
            }
        }
        if (!kOnline || !have) return;
        if (kOnline && o_hist != nullptr) {
            const double bf = (now - t0) * A.online_hist_scale;
            AF_BUMP(o_hist + (bf >= (double)(A.online_hist_bins - 1u) ? A.online_hist_bins - 1u : (uint32_t)bf));
        }
        if (kOnline && o_rps != nullptr) {
            const double kf = __builtin_ceil(now);
            const uint32_t k = kf < 1.0 ? 1u : (uint32_t)kf;
            if (k <= A.online_rps_buckets) AF_BUMP(o_rps + (k - 1u));
        }
    }

    // ---- one scenario ------------------------------------------------------------------------------------
    // `smem` : LDS of this wave (plan blob + layout words); `sc` : scenario index in the launch
    AF_CORE void run(AF_PLAN_AS uint64_t* smem, uint32_t sc) {
        lane = W::lane();
        blob = smem;
#if !defined(__HIP_DEVICE_COMPILE__)
        if (kCt && (A.L.cap != kCap || A.L.off_list != (kMarks ? A.L.off_list : 0u) || A.L.off_aux != o_aux() || A.L.off_aux3 != o_aux3() ||
                    A.L.off_out != o_out() || A.L.off_seg != o_out() || A.L.off_sorted != o_sorted() || A.L.off_hist != o_hst() || A.L.off_fr != o_fr()))
            __builtin_trap();   // make_flow_layout and the compile-time offsets above disagree
#endif
        M = smem + A.blob_bytes / 8u;
        seed = A.seeds[sc];
        arr = A.arrivals + (size_t)sc * A.n_draw;
        clock = A.clock ? A.clock + (size_t)sc * A.clock_cap * 2u : nullptr;
        samples = A.samples ? A.samples + (size_t)sc * A.L.pitch * A.tick_cap : nullptr;
        o_hist = (kOnline && A.online_hist) ? A.online_hist + (size_t)sc * A.online_hist_bins : nullptr;
        o_rps = (kOnline && A.online_rps) ? A.online_rps + (size_t)sc * A.online_rps_buckets : nullptr;
        const double T = A.total_time;

        // plan blob -> LDS, layout words zeroed
        {
            const uint64_t* g = reinterpret_cast<const uint64_t*>(A.blob);
            for (uint32_t i = lane; i < A.blob_bytes / 8u; i += 64u) blob[i] = g[i];
            for (uint32_t i = lane; i < A.L.n_words; i += 64u) M[i] = 0ull;
        }
        if (kHbmRing && samples != nullptr && A.L.ring_rows == 0u) {   // tick differences accumulate in the sample rows themselves
            const uint32_t rows = A.n_ticks < A.tick_cap ? A.n_ticks : A.tick_cap;
            const size_t words = (size_t)rows * A.L.pitch;
            for (size_t i = (size_t)lane * 4u; i < words; i += 256u) af::store4(samples + i, 0u, 0u, 0u, 0u);
            W::global_fence();
        }
        W::sync();
        if (lane == 0u) {
            // per-scenario parameters (af_override_t columns): edge law, step times
            for (uint32_t k = 0u; k < A.n_ovr; ++k) {
                const uint64_t v = d2u(A.ovr_values[(size_t)k * A.ovr_stride + sc]);
                const uint32_t p = A.ovr_param[k], idx = A.ovr_index[k];
                if (p == af::PARAM_EDGE_MEAN) blob[A.off_edge + af::EREC * idx] = v;
                else if (p == af::PARAM_EDGE_SIGMA) blob[A.off_edge + af::EREC * idx + 1u] = v;
                else if (p == af::PARAM_EDGE_DROPOUT) blob[A.off_edge + af::EREC * idx + 2u] = v;
                else if (p == af::PARAM_STEP_TIME) blob[A.off_row + af::TREC * idx] = v;   // idx is a step ROW
                // server resources, timeline marks (sweeps over server_resources and over the injected events)
                else if (p == af::PARAM_SRV_CORES) {
                    const uint32_t at = A.off_srv + af::SREC * idx + 1u;
                    blob[at] = (blob[at] & ~0xFFFFull) | (uint64_t)((uint32_t)u2d(v) & 0xFFFFu);
                } else if (p == af::PARAM_SRV_RAM_MB) blob[A.off_srv + af::SREC * idx] = v;
                else if (p == af::PARAM_EMARK_TIME) blob[A.off_emark + af::MREC * idx] = v;
                else if (p == af::PARAM_EMARK_DELTA) blob[A.off_emark + af::MREC * idx + 1u] = v;
                else if (p == af::PARAM_EMARK_EDGE) blob[A.off_emark + af::MREC * idx + 2u] = (uint64_t)(uint32_t)u2d(v);
                else if (p == af::PARAM_SMARK_TIME) blob[A.off_smark + af::NREC * idx] = v;
                else if (p == af::PARAM_SMARK_LB_EDGE) {
                    const uint32_t at = A.off_smark + af::NREC * idx + 1u;
                    blob[at] = (blob[at] & ~0xFFFFFFFFull) | (uint64_t)(uint32_t)((int32_t)u2d(v) + 1);
                } else if (p == af::PARAM_SMARK_DOWN) {
                    const uint32_t at = A.off_smark + af::NREC * idx + 1u;
                    blob[at] = (blob[at] & 0xFFFFFFFFull) | ((uint64_t)(u2d(v) != 0.0 ? 1u : 0u) << 32);
                }
            }
            // an edge's dropout rate as a threshold on the 53 bits of its uniform draw (edge_draw): ceil(rate x 2^53); the
            // scaling by a power of two is exact, and for an integer k: k x 2^-53 < rate  <=>  k < ceil(rate x 2^53)
            for (uint32_t e = 0u; e < A.n_edges; ++e) {
                const double x = u2d(blob[A.off_edge + af::EREC * e + 2u]) * 9007199254740992.0;
                blob[A.off_edge + af::EREC * e + 2u] = !(x > 0.0) ? 0ull : x >= 9007199254740992.0 ? (1ull << 53) : (uint64_t)__builtin_ceil(x);
            }
            // cumulative spike per edge after every mark, the reference's own += / -= in f64 (injection.py:191-198)
            for (uint32_t i = 0u; i < A.n_edge_marks; ++i) {
                double acc = 0.0;
                const uint32_t e = (uint32_t)emark(i)[2];
                for (uint32_t p = 0u; p < i; ++p)
                    if ((uint32_t)emark(p)[2] == e) acc = spike_cum()[p];
                spike_cum()[i] = acc + u2d(emark(i)[1]);
                if (i < 32u && e < A.n_edges) sends()[e] |= 1u << i;   // spike_at(): which marks belong to the edge
            }
            AF_PLAN_AS uint32_t* lw = lbw();
            for (uint32_t v = 0u; v < A.n_servers; ++v) {   // step counts of each server's (only) endpoint: IO* CPU* IO*
                const uint32_t ep = (uint32_t)(blob[A.off_srv + af::SREC * v + 1u] >> 32) & 0xFFFFu;
                uint32_t row = (uint32_t)blob[A.off_ep + af::PREC * ep + 1u], cnt[3] = {0u, 0u, 0u}, phase = 0u;
                for (;; ++row) {
                    const uint32_t kind = (uint32_t)blob[A.off_row + af::TREC * row + 2u];
                    if (kind == af::STEP_END) break;
                    if (phase == 0u && kind == af::STEP_CPU) phase = 1u;
                    else if (phase == 1u && kind == af::STEP_IO) phase = 2u;
                    cnt[phase] += 1u;
                }
                lw[LBW_PROG + v] = cnt[0] | (cnt[1] << 8) | (cnt[2] << 16);
                const double ram = u2d(blob[A.off_ep + af::PREC * ep]), ram_mb = u2d(blob[A.off_srv + af::SREC * v]);
                uint32_t slots = 0xFFFFFFFFu;   // requests that fit the RAM at once
                if (ram > 0.0) {
                    const double q = ram_mb / ram;
                    slots = q < 4.0e9 ? (uint32_t)q : 0xFFFFFFFFu;
                    while ((double)slots * ram > ram_mb && slots > 0u) --slots;
                }
                lw[LBW_SLOTS + v] = slots;
            }
            if (kGen)
                for (uint32_t v = 0u; v < A.n_servers; ++v) {   // build_containers (server_containers.py:61-68): full
                    AF_PLAN_AS uint64_t* g = gs(v);
                    g[GS_CPU] = blob[A.off_srv + af::SREC * v + 1u] & 0xFFFFull;   // cpu_free = cores, nobody ready
                    g[GS_IO] = 0xFFFFFFFF00000000ull;                                  // every slot free
                    g[GS_RAM] = blob[A.off_srv + af::SREC * v];
                }
            if (kChain) {   // levels: a server fed by a server of level k is of level k + 1 at least (the host checked: no cycle, <= kMaxLevels)
                AF_PLAN_AS uint8_t* lv = srv_levels();   // (zeroed with the layout words)
                for (uint32_t pass = 0u; pass + 1u < kMaxLevels; ++pass)
                    for (uint32_t v = 0u; v < A.n_servers; ++v) {
                        const uint64_t tw = erec((uint32_t)(blob[A.off_srv + af::SREC * v + 1u] >> 16) & 0xFFFFu)[3];
                        if (((uint32_t)tw & 0xFFu) == af::NODE_LB) {   // (round 5) a server that feeds the LB: everything behind the LB is deeper
                            for (uint32_t i = 0u; i < A.n_lb_edges; ++i) {
                                const uint32_t w = (uint32_t)(erec((uint32_t)blob[A.off_lb + i])[3] >> 8) & 0xFFu;
                                if (lv[w] < lv[v] + 1u) lv[w] = (uint8_t)(lv[v] + 1u);
                            }
                            continue;
                        }
                        if (((uint32_t)tw & 0xFFu) != af::NODE_SERVER) continue;
                        const uint32_t w = (uint32_t)(tw >> 8) & 0xFFu;
                        if (lv[w] < lv[v] + 1u) lv[w] = (uint8_t)(lv[v] + 1u);
                    }
            }
            for (uint32_t i = 0u; i < A.n_lb_edges; ++i) lw[i] = (uint32_t)blob[A.off_lb + i];
            lw[16] = 0u;
            lw[17] = A.n_lb_edges;
            lw[18] = 0u;
            lw[19] = A.n_lb_edges ? 0xFFFFFFFFu / A.n_lb_edges + 1u : 0u;
        }
        W::sync();

        if (kProf) {
#pragma unroll
            for (uint32_t k = 0u; k < kProfSections; ++k) prof_acc[k] = 0ull;
            prof_t = W::clock();
        }
        cursor = n_comp = tick_base = 0u;
        gen_pre = lane < A.n_draw ? arr[lane] : AF_INF;
        my_sends = 0u;
        lb_head = lb_mark = 0u;
        lb_nl = A.n_lb_edges;
        lb_magic = A.n_lb_edges ? 0xFFFFFFFFu / A.n_lb_edges + 1u : 0u;
        ev = drops = 0u;
        gs_rounds = 0u;
        why = info = 0u;
        run_val = run_val2 = 0;
        gen_done = false;
        nl0 = nl1 = nl2 = nl3 = 0u;
        h0 = h1 = h2 = h3 = 0.0;
        h2b = h2c = h2d = h2e = 0.0;   // (kHzLds: the LDS words were zeroed with the layout)
        n_levels = 1u;
        if (kChain)
            for (uint32_t v = 0u; v < A.n_servers; ++v) n_levels = level_of(v) + 1u > n_levels ? level_of(v) + 1u : n_levels;
        const uint32_t cap = kCt ? kCap : A.L.cap;
        // FEAT_CHAIN, round 5: client -> server chain -> LB -> servers -> client.  The LB station then runs BEHIND the server levels in
        // front of it: lb_pos = the level of the servers behind the LB (0: the client feeds the LB, the classic order); lb_in_edge = the
        // one edge the LB receives by (graph.py:135-157 allows fan-out at the LB only, so the path in front of it is one chain)
        lb_pos = 0u;
        lb_in_edge = A.client_out_edge;
        if (kChain && A.has_lb)
            for (uint32_t v = 0u; v < A.n_servers; ++v) {
                const uint32_t oe = (uint32_t)(blob[A.off_srv + af::SREC * v + 1u] >> 16) & 0xFFFFu;
                if (((uint32_t)erec(oe)[3] & 0xFFu) == af::NODE_LB) {
                    lb_pos = level_of(v) + 1u;
                    lb_in_edge = oe;
                }
            }
        // where the client's out-edge leads: the LB's list, or the servers' (round 5: also with an LB further down the path -- only the
        // FEAT_CHAIN forms run such plans, so everywhere else this stays the constant it was: a RUN-TIME list index makes the
        // long-list forms index FlowLayout::cap_of[] dynamically, which put the launch arguments in scratch memory and cost the
        // general-server workload 60 %, measured)
#if defined(AF_FJ_LB_POS)
        const uint32_t first_srv_stage = !A.has_lb ? 2u : (kChain && AF_FJ_LB_POS != 0u) ? 2u : 1u;
#else
        const uint32_t first_srv_stage = !A.has_lb ? 2u : (kChain && lb_pos != 0u) ? 2u : 1u;
#endif

        // Every round walks the five stations in order.  The code of select() and of edge_send() exists ONCE
        // (the loop is not unrolled): the kernel stays small enough for the instruction cache.
        prof(PROF_SETUP);
        for (;;) {
            uint32_t work = 0u;
            moved = false;
            // With an LDS tick ring the generator does not run further ahead of the completed ticks than the ring's window;
            // with FEAT_FAR no station handles an event beyond it (select()): the receiving station enters the delivery of
            // a marked message at the time of that event.
            if (kFar) t_lim = (samples != nullptr && (!kHbmRing || A.L.ring_rows != 0u)) ? (double)(tick_base + A.L.win_rows) * A.sample_period : AF_INF;
            const double h_done_before = H_get(3u);
            double H_in = AF_INF, h_gen = AF_INF;
            // (plan-specialised builds unroll the five stations: `st` becomes a constant in each copy -- list addresses fold,
            // the select chains over nl0..nl3 / h0..h3 and their scratch copy disappear: 58.8 -> 49.2 ms on BASELINE config 2,
            // 5 500 instructions = 36 KB of code.  The generic instantiations stay a loop: with run-time plan shapes the
            // unrolled body was 13 000 instructions and fell out of the instruction cache)
            // (FEAT_CHAIN: the server station once per level, in level order -- stx counts the passes, st is the station; a
            // plan-specialised build unrolls as many level passes as the plan has levels)
            // (FEAT_CHAIN: behind generator and client come kLevelPasses + 1 slots -- the server levels in order with the LB station
            // in front of level lb_pos --, then the client's second visit)
#if defined(AF_FJ_LB_POS)
            const uint32_t lbp = AF_FJ_LB_POS;
#else
            const uint32_t lbp = lb_pos;
#endif
#if defined(AF_FJ_N_LEVELS)
            constexpr uint32_t kLevelPasses = AF_FJ_N_LEVELS;
#else
            constexpr uint32_t kLevelPasses = kMaxLevels;
#endif
#if defined(AF_FLOW_JIT) && !defined(AF_FLOW_LOOP_STATIONS)
#pragma unroll
#else
#pragma nounroll
#endif
            for (uint32_t stx = 0u; stx < (kChain ? 4u + kLevelPasses : 5u); ++stx) {
                const uint32_t slot = stx - 2u;   // (FEAT_CHAIN, stx >= 2)
                const uint32_t st = !kChain ? stx : stx < 2u ? stx : stx == 3u + kLevelPasses ? 4u : slot == lbp ? 2u : 3u;
                const uint32_t level = (kChain && st == 3u) ? (slot < lbp ? slot : slot - 1u) : 0u;
                if (kChain && st == 3u && level >= n_levels) continue;
                if (st == 2u && !A.has_lb) continue;
                // ---- the station's batch: lane r < n_sel holds (key = event time, t0 = start time, aux)
                double key = 0.0, t0 = 0.0;
                uint32_t aux = 0u, n_sel;
                const uint32_t nxt = st == 0u ? 0u : st == 1u ? first_srv_stage : st;   // list the results go to (st < 4; FEAT_CHAIN, servers: see the appends)
                if (st == 0u) {   // generator (rqs_generator.py:97-119): up to 64 arrivals
                    uint32_t room = (kBig ? cap_of(0u) : cap) - nl0;
                    room = room < 64u ? room : 64u;
                    // (arrival cursor + lane was fetched a round ago -- gen_pre -- so the station never waits for HBM: round 4)
                    t0 = lane < room ? gen_pre : AF_INF;
                    const double t_cap = kFar ? t_lim
                                         : (samples != nullptr && (!kHbmRing || A.L.ring_rows != 0u)) ? (double)(tick_base + A.L.win_rows) * A.sample_period
                                                                                                       : AF_INF;
                    const uint64_t vm = W::ballot(t0 < T && t0 < t_cap);   // arrival times increase: a prefix of the lanes
                    n_sel = popc64(vm);
                    key = t0;
#if defined(AF_FUSED_ARRIVAL_PROBE)
                    // MEASUREMENT ONLY: the work a generator station would do if it drew its own gaps
                    // instead of reading af_arrival_groups' rows -- per lane the Philox block and the logarithm of draw cursor + lane
                    // and the IEEE division by lambda; then the sampler's two running sums, which are 64 DEPENDENT f64 additions
                    // (f64 addition does not associate: lane l needs gaps 0 .. l added one by one) -- WITHOUT the window bookkeeping a
                    // real one needs on top (draws discarded at window ends, the users draw).  The results are thrown away (the
                    // arrivals still come from HBM, so parity holds); only the kernel time is read.
                    {
                        const af::U4 pr = af::draw_block(seed, af::STREAM_GENERATOR, cursor + lane + 0x40000000u, 0u);
                        double pu = af::u53(pr.x, pr.y);
                        pu = pu < 1e-15 ? 1e-15 : pu;
                        const double pe = -af::af_log_unit(1.0 - pu), pdt = pe / (133.25 + probe_g * 1e-300);
                        double pg = probe_g, ps = probe_s, mine_s = 0.0;
#pragma unroll 8
                        for (uint32_t j = 0u; j < 64u; ++j) {
                            const double d = bcast_f64(pdt, j);
                            pg = pg + d;
                            ps = ps + d;
                            mine_s = lane == j ? ps : mine_s;
                        }
                        probe_g = pg;
                        probe_s = ps;
                        probe_acc += mine_s;
                    }
#endif
                } else {
                    // (FEAT_CHAIN: what a level sends back into the server list takes the places its own selection left there,
                    // so the room that binds is the completion list's)
                    uint32_t room = st == 4u ? 64u : (kBig ? cap_of(nxt) : cap) - n_list_get(nxt);
                    if (kChain && st == 3u && A.has_lb && level + 1u == lbp) {   // the level in front of the LB sends into the LB's list
                        const uint32_t room1 = (kBig ? cap_of(1u) : cap) - nl1;
                        room = room1 < room ? room1 : room;
                    }
                    if (kGen && st == 3u) {
                        // the round-at-once solver (gen_servers_par) gives every request of the window a lane: the ones inside the
                        // servers of this pass and the arrivals taken now -- no more arrivals than lanes are left
                        uint32_t inside = 0u;
                        for (uint32_t k = 0u; k < A.n_servers; ++k)
                            if (!kChain || level_of(k) == level) inside += hi32(gs(k)[GS_EV]) + hi32(gs(k)[GS_CQ]);
                        // (the same bound keeps a server's departures of one round within kGsDeps: <= 32 inside + 8, or <= 64 in all)
                        const uint32_t lanes_left = inside <= 56u ? 64u - inside : 8u;
                        if (lanes_left < room) room = lanes_left;
                    }
                    n_sel = select(st - 1u, H_in, room, key, t0, aux,
                                   (kChain && st == 3u) ? level_slot(level) : st - 1u, (kChain && st == 3u) ? level : kAnyLevel);
                }
                if (st == 0u) prof(PROF_GEN);
                else prof(PROF_SELECT);
                const bool have = lane < n_sel;
                if (have) ev += 1u;                       // one timed event per message: arrival / delivery
                work += n_sel;
                // ---- sampled series: the delivery ends the message's stay on the edge it came by (edge.py:115), if the
                // sender entered it (sign of t0); `row` = tick row of the station's event, which the send below starts at
                const bool series_on = samples != nullptr;
                const bool cnt_in = kFar && series_on && have && st > 0u && __builtin_signbit(t0);
                if (kFar && st > 0u) t0 = __builtin_fabs(t0);
                uint32_t row = 0u;
                if (kFar && series_on && have && (st <= 2u || cnt_in)) row = tick_index(key, true);
                if (kFar && cnt_in) add_point(st == 1u ? A.gen_out_edge : st == 2u ? (kChain ? lb_in_edge : A.client_out_edge) : st == 3u ? aux >> 8 : aux, row, -1);
                // ---- what the station does with it: the out-edge, the message's index on it, the send time
                prof(PROF_SERIES_RECV);
                bool sending = have, pre = false, to_srv = false, to_lb = false;   // to_srv / to_lb (FEAT_CHAIN): my server's out-edge leads to a server / to the LB
                uint32_t e = 0u, idx = 0u, tgt = 0u;
                double ts = key, pre_tr = 0.0;
                if (st == 0u) {
                    e = A.gen_out_edge;
                    idx = cursor + lane;
                    cursor += n_sel;
                    // next arrival not yet generated: one of the fetched ones unless all 64 went out
                    H_in = n_sel < 64u ? bcast_f64(gen_pre, n_sel) : cursor < A.n_draw ? arr[cursor] : AF_INF;
                    gen_pre = cursor + lane < A.n_draw ? arr[cursor + lane] : AF_INF;   // (used a round later)
                    gen_done = !(H_in < T);
                    h_gen = H_in;
                } else if (st == 1u) {   // client, first visit (client.py:46-60): forward on the client's out-edge
                    e = A.client_out_edge;
                    idx = sends_of(e) + lane;
                    if (lane == e) my_sends += n_sel;
                    tgt = (uint32_t)(erec(e)[3] >> 8) & 0xFFu;
                } else if (st == 2u) {   // load balancer
                    if (n_sel > 0u) {
                        if (kLC && A.lb_least_connections) {
                            e = lb_pick_lc(n_sel, key, pre_tr);
                            pre = true;
                        } else {
                            e = lb_pick(n_sel, key);
                        }
                        idx = claim_send_index(have, e, false);
                        tgt = (uint32_t)(erec(e)[3] >> 8) & 0xFFu;
                    }
                } else if (kGen && st == 3u) {   // servers, general form: lane k runs server k up to the station's horizon
                    const uint32_t sv = aux & 0xFFu;
                    uint32_t pos = 0u, off = 0u;
                    for (uint32_t k = 0u; k < A.n_servers; ++k) {
                        const uint64_t m = W::ballot(have && sv == k);
                        if (have && sv == k) pos = off + W::mbcnt(m);
                        if (lane == k) {
                            lbw()[LBW_SEG_OFF + k] = off;
                            lbw()[LBW_SEG_LEN + k] = popc64(m);
                        }
                        off += popc64(m);
                    }
                    W::sync();   // select()'s scratch is dead: the arrivals of the round, per server, in time order
                    if (have) {
                        seg(0)[pos] = key;
                        seg(1)[pos] = t0;
                        // what does not depend on the server's state is worked out here, one arrival per lane, instead of by the
                        // server's one lane: the endpoint draw (server.py:101; its index = the server's arrival count) and the
                        // arrival's tick row
                        const uint32_t n_ep = (uint32_t)(blob[A.off_srv + af::SREC * sv + 1u] >> 48);
                        const uint32_t a_idx = lo32(gs(sv)[GS_ARR]) + (pos - lbw()[LBW_SEG_OFF + sv]);
                        const uint32_t pick = n_ep > 1u ? af::cold_endpoint_pick(seed, sv, a_idx, n_ep) : 0u;
                        const uint32_t a_row = samples != nullptr ? tick_index(key, true) : 0u;
                        seg(2)[pos] = u2d(pack32(pick, a_row));
                    }
                    W::sync();
                    uint32_t done = 0u;
                    // (FEAT_CHAIN: the servers of this pass's level, up to the level's horizon; the others keep their state)
                    const bool my_pass = lane < A.n_servers && (!kChain || level_of(lane) == level);
                    // the whole round at once where the solver decides it (gen_servers_par), else event by event
                    uint32_t par_done = 0u;
                    const bool solved = gen_servers_par(level, H_get(kChain ? level_slot(level) : 2u), par_done);
                    W::sync();   // (every lane has read the servers' state before a lane's gen_servers() changes it)
                    // (diagnostic: rounds solved at once << 16 | rounds walked event by event; each half saturates on its own)
                    if (solved) gs_rounds += (gs_rounds >> 16) < 0xFFFFu ? 0x10000u : 0u;
                    else gs_rounds += (gs_rounds & 0xFFFFu) < 0xFFFFu ? 1u : 0u;
                    if (kProf && !solved) prof_acc[PROF_N_WALKED_ROUNDS] += 1ull;
                    if (!solved && my_pass) done = gen_servers(lane, H_get(kChain ? level_slot(level) : 2u));
                    W::sync();
                    work += solved ? par_done : popc64(W::ballot(done != 0u));
                    prof(PROF_SERVERS);
                    // the departures the servers produced (each server's in time order), sent by the whole wave, 64 at a time
                    auto dep_cnt = [&](uint32_t k) { return (!kChain || level_of(k) == level) ? lo32(gs(k)[GS_DEP]) : 0u; };
                    // (wave-uniform; FEAT_CHAIN: a server's departures go to the completion list, back into the server list or -- round 5 --
                    // into the LB's list, by the kind of node its out-edge leads to: each list must hold what is bound for it.  Round 4
                    // checked the whole total against the completion AND the server list, which handed a third of the first launches
                    // of tiers of general servers to the second chance for nothing.)
                    uint32_t total = 0u, to_list[4] = {0u, 0u, 0u, 0u};
                    for (uint32_t k = 0u; k < A.n_servers; ++k) {
                        const uint32_t kind = !kChain ? (uint32_t)af::NODE_CLIENT
                                                      : (uint32_t)erec((uint32_t)(blob[A.off_srv + af::SREC * k + 1u] >> 16) & 0xFFFFu)[3] & 0xFFu;
                        total += dep_cnt(k);
                        if (kind == af::NODE_SERVER) to_list[2] += dep_cnt(k);
                        else if (kind == af::NODE_LB) to_list[1] += dep_cnt(k);
                        else to_list[3] += dep_cnt(k);
                    }
                    const bool too_many = to_list[3] > cap_of(3u) - nl3 || to_list[2] > cap_of(2u) - nl2 || (A.has_lb && to_list[1] > cap_of(1u) - nl1);
                    if (too_many) why |= FLOW_WHY_LIST;
                    for (uint32_t base = 0u; base < total && !too_many; base += 64u) {
                        const uint32_t want = base + lane;   // my departure, counted over the servers in order
                        bool mine = false;
                        uint32_t me = 0u, mj = 0u, first = 0u;
                        for (uint32_t k = 0u; k < A.n_servers; ++k) {
                            const uint32_t cnt = dep_cnt(k);
                            if (want >= first && want < first + cnt) {
                                mine = true;
                                me = k;
                                mj = want - first;
                            }
                            first += cnt;
                        }
                        const uint32_t oe = (uint32_t)(blob[A.off_srv + af::SREC * me + 1u] >> 16) & 0xFFFFu;
                        const double dts = mine ? u2d(gs(me)[GS_DEPT + mj]) : 0.0, dt0 = mine ? u2d(gs(me)[GS_DEPT0 + mj]) : 0.0;
                        const uint32_t didx = W::shfl32(my_sends, oe) + mj;
                        double k2 = 0.0, transit = 0.0;
                        bool counted = false;
                        const bool sent = mine && send_draw(oe, didx, transit);
                        prof(PROF_DRAW);
                        const uint32_t drow = (kFar && sent && samples != nullptr) ? tick_index(dts, true) : 0u;
                        const bool ok = sent && send_finish(oe, dts, drow, kFar, transit, k2, counted);
                        prof(PROF_SEND_SERIES);
                        if (kChain) {   // to the client, or to a server of a deeper level (aux: the server | the edge the message comes by)
                            const uint64_t tw = erec(oe)[3];
                            const bool dep_to_srv = ((uint32_t)tw & 0xFFu) == af::NODE_SERVER, dep_to_lb = ((uint32_t)tw & 0xFFu) == af::NODE_LB;
                            const uint32_t dep_tgt = (uint32_t)(tw >> 8) & 0xFFu;
                            append(3u, ok && !dep_to_srv && !dep_to_lb, k2, (kFar && counted) ? -dt0 : dt0, oe, dts);
                            append(2u, ok && dep_to_srv, k2, (kFar && counted) ? -dt0 : dt0, !kFar ? dep_tgt : dep_tgt | (oe << 8), dts);
                            if (A.has_lb) append(1u, ok && dep_to_lb, k2, (kFar && counted) ? -dt0 : dt0, 0u, dts);
                        } else {
                            append(3u, ok, k2, (kFar && counted) ? -dt0 : dt0, oe, dts);
                        }
                    }
                    W::sync();
                    for (uint32_t k = 0u; k < A.n_servers; ++k) {   // the servers' out-edges: as many sends as departures
                        const uint32_t oe_k = (uint32_t)(blob[A.off_srv + af::SREC * k + 1u] >> 16) & 0xFFFFu;
                        if (lane == oe_k) my_sends += dep_cnt(k);
                    }
                    W::sync();
                    sending = false;   // (everything this station sends went out above)
                } else if (st == 3u) {   // servers
                    if (n_sel > 0u) {
                        const uint32_t sv = aux & 0xFFu;
                        uint32_t pos = 0u, off = 0u, seg_off = 0u, seg_len = 0u, srv_cnt = 0u;   // per-server segments of the time-ordered arrivals
                        for (uint32_t k = 0u; k < A.n_servers; ++k) {
                            const uint64_t m = W::ballot(have && sv == k);
                            if (have && sv == k) {
                                pos = off + W::mbcnt(m);
                                seg_off = off;
                                seg_len = popc64(m);
                            }
                            if (lane == k) srv_cnt = popc64(m);
                            off += popc64(m);
                        }
                        W::sync();   // select()'s scratch is dead from here on: the segments reuse it
                        const SrvTimes r = servers_solve(have, sv, pos, key, seg_off, seg_len, srv_cnt);
                        prof(PROF_SERVERS);
                        if (have) {
                            e = r.out_edge;   // (round 6: server words that servers_solve() read are not read again)
                            if (kChain) {
                                const uint64_t tw = erec(e)[3];
                                to_srv = ((uint32_t)tw & 0xFFu) == af::NODE_SERVER;
                                to_lb = ((uint32_t)tw & 0xFFu) == af::NODE_LB;
                                tgt = (uint32_t)(tw >> 8) & 0xFFu;
                            }
                            const double ram = r.ram;
                            const uint32_t s0 = A.n_edges + 3u * sv;
                            ts = r.g;
                            // ready queue: waited for a core (server.py:215-225); leading / trailing I/O steps; RAM held from
                            // admission to the end (server.py:146-149, 270-273)
                            // (round 3: also in the instantiations without FEAT_FAR, which used to call add_interval per
                            // interval -- 12 tick rows per request instead of 10: 49.7 -> 48.5 ms on BASELINE config 2)
                            if (series_on) {   // (one tick row per distinct time: the send below starts at G's)
                                const bool q_ready = r.s > r.b, q_pre = r.b > r.adm, q_post = r.g > r.f, q_ram = ram > 0.0;
                                uint32_t t_adm = 0u, t_b = 0u, t_s = 0u, t_f = 0u, t_g = 0u;
                                if (q_pre || q_ram) t_adm = tick_index(r.adm, true);
                                if (q_ready || q_pre) t_b = tick_index(r.b, true);
                                if (q_ready) t_s = tick_index(r.s, true);
                                if (q_post) t_f = tick_index(r.f, true);
                                if (q_post || q_ram || ts < T) t_g = tick_index(r.g, true);
                                add_span(s0, t_b, t_s, 1, q_ready);
                                add_span(s0 + 1u, t_adm, t_b, 1, q_pre);
                                add_span(s0 + 1u, t_f, t_g, 1, q_post);
                                add_span(s0 + 2u, t_adm, t_g, (int32_t)(ram * A.ram_scale), q_ram);
                                row = t_g;
                            }
                        }
                        sending = have && ts < T;      // transport() on the server's out-edge at G (server.py:276), if the horizon allows
                        prof(PROF_SERVER_SERIES);
                        idx = claim_send_index(sending, e, true);
                    }
                } else {   // client, second visit (client.py:62-69): the request is complete
                    complete(have, lane, t0, key);
                    n_comp += n_sel;
                    sending = false;
                }
                if (st == 3u) prof(PROF_SERVERS);
                else if (st == 4u) prof(PROF_COMPLETE);
                else prof(PROF_STATION);
                if (kGen && st == 3u) {
                    if (kChain) {   // (as for the tandem levels below: the running minimum of the send floors)
                        const double fl = send_floor(3u, H_get(level_slot(level)), level == 0u);
                        H_in = fl < H_in ? fl : H_in;
                    } else {
                        H_in = send_floor(3u, H_get(2u));
                    }
                    prof(PROF_APPEND);
                } else if (st < 4u) {
                    double k2 = 0.0;
                    bool counted = false;
                    double transit = 0.0;
                    const bool sent = sending && send_draw(e, idx, transit, kLC && pre, pre_tr);
                    prof(PROF_DRAW);
                    const bool ok = sent && send_finish(e, ts, row, st == 3u, transit, k2, counted);
                    prof(PROF_SEND_SERIES);
                    // (server list: the server and the edge the message comes by; completion list: the server's out-edge)
                    if (kChain && st == 3u) {   // lane by lane: to the client, or to a server of a deeper level
                        append(3u, ok && !to_srv && !to_lb, k2, (kFar && counted) ? -t0 : t0, e, ts);
                        append(2u, ok && to_srv, k2, (kFar && counted) ? -t0 : t0, !kFar ? tgt : tgt | (e << 8), ts);
                        if (A.has_lb) append(1u, ok && to_lb, k2, (kFar && counted) ? -t0 : t0, 0u, ts);
                        // what the deeper levels (and the client) may touch: everything the station in front of the servers AND
                        // every level so far delivered before it (the cache of send_floor belongs to level 0's horizon)
                        const double fl = send_floor(3u, H_get(level_slot(level)), level == 0u);
                        H_in = fl < H_in ? fl : H_in;
                    } else {
                        append(nxt, ok, k2, (kFar && counted) ? -t0 : t0, !kFar ? tgt : st == 3u ? e : tgt | (e << 8), ts);
                        if (st > 0u) H_in = H_get(st - 1u);
                        H_in = send_floor(st, H_in);   // what the next station may touch: everything delivered before this
                    }
                    prof(PROF_APPEND);
                }
            }
            // ---- ticks that can no longer change
            // (a station behind a spiked edge runs AHEAD of the one that feeds it: the slowest horizon bounds what is final)
            double h_min = H_get(3u);
            if (kMarks && A.n_edge_marks != 0u) {
                h_min = h_min < h_gen ? h_min : h_gen;
                h_min = h_min < H_get(0u) ? h_min : H_get(0u);
                h_min = (A.has_lb && H_get(1u) < h_min) ? H_get(1u) : h_min;
                h_min = h_min < H_get(2u) ? h_min : H_get(2u);
                if (kChain)
#pragma unroll
                    for (uint32_t lv = 1u; lv < kMaxLevels; ++lv)
                        if (n_levels > lv) h_min = h_min < H_get(level_slot(lv)) ? h_min : H_get(level_slot(lv));
            }
            const bool finished = gen_done && work == 0u && !(h_min < T);
            W::sync();
            flush_ticks(finished ? A.n_ticks : tick_index(h_min, false));
            W::sync();
            prof(PROF_FLUSH);
#if defined(AF_FLOW_TRACE) && !defined(__HIP_DEVICE_COMPILE__)
            if (lane == 0u) std::fprintf(stderr, "round: work %u cursor %u nl %u %u %u %u h %.6f %.6f %.6f %.6f hgen %.6f hmin %.6f moved %d tick_base %u n_comp %u why %x\n", work, cursor, nl0, nl1, nl2, nl3, H_get(0u), H_get(1u), H_get(2u), H_get(3u), h_gen, h_min, (int)moved, tick_base, n_comp, why);
#endif
            const bool stuck = work == 0u && !finished && !(kMarks ? moved : H_get(3u) > h_done_before);
            if (stuck) why |= FLOW_WHY_LIST;   // nothing moved, no horizon advanced: a list is full of later messages
            if (finished || W::any(why != 0u)) break;
        }

        // ---- counts
        const uint32_t ev_all = wave_sum(ev), drop_all = wave_sum(drops), why_all = wave_or(why), info_all = wave_or(info);
        if (lane == 0u) {
            uint32_t flags = A.pre_flags[sc] | info_all;
            if (n_comp > A.clock_cap && clock != nullptr) flags |= af::FLAG_CLOCK_OVERFLOW;
            if (A.n_ticks > A.tick_cap && samples != nullptr) flags |= af::FLAG_TICK_OVERFLOW;
            if (why_all != 0u) flags |= FLAG_FLOW_FALLBACK | why_all;
#if defined(AF_FUSED_ARRIVAL_PROBE)
            if (probe_acc == 1.2345e300) flags |= 1u << 30;   // (keeps the probe's arithmetic alive)
#endif
            uint32_t marks = 0u;
            for (uint32_t i = 0u; i < A.n_edge_marks; ++i) marks += u2d(emark(i)[0]) < T ? 1u : 0u;
            for (uint32_t i = 0u; i < A.n_srv_marks; ++i) marks += u2d(smark(i)[0]) < T ? 1u : 0u;
            uint32_t* c = A.counts + (size_t)sc * af::CNT_SLOTS;
            c[af::CNT_GENERATED] = cursor;
            c[af::CNT_COMPLETED] = n_comp;
            c[af::CNT_DROPPED] = drop_all;
            c[af::CNT_EVENTS] = ev_all;
            c[af::CNT_TICKS] = A.n_ticks;
            c[af::CNT_FLAGS] = flags;
            // a diagnostic: the sequential kernels' peak of live requests; FEAT_GENSRV: how the server station's rounds were run
            c[af::CNT_MAX_LIVE] = kGen ? gs_rounds : 0u;
            c[af::CNT_MARKS] = marks;
        }
        if (kProf) {
            prof(PROF_SETUP);
            if (lane == 0u && A.prof != nullptr)
#pragma unroll
                for (uint32_t k = 0u; k < kProfSections; ++k) A.prof[(size_t)sc * kProfSections + k] = prof_acc[k];
        }
    }
};

}  // namespace aff
