/* asyncflow_hip.h -- C ABI of the MI355X batched discrete-event engine.
 *
 * Drop-in boundary for ONE hot path of AsyncFlow (reference @ /root/reference):
 *
 *     SimulationRunner.run()  ->  simpy.Environment.run(until=T)
 *     (src/asyncflow/runtime/simulation_runner.py:349-376)
 *
 * executed over n independent scenarios (seed replicas / parameter-grid points)
 * on one MI355X.  The reference has NO FFI/plugin boundary for this path
 * (pure Python): the only seam is the Python call
 * `SimulationRunner(env=..., simulation_input=SimulationPayload).run()`.
 * The host-side mirror of that call is asyncflow_amd.SimulationRunner
 * (asyncflow_amd/runner.py); it lowers the validated payload to `af_plan_t`
 * and calls the entry points below through ctypes (INTEGRATION.md shows the
 * stub a reference maintainer would add).
 *
 * Conventions
 *  - plain C, no torch / HIP types in signatures; pointers + sizes only;
 *  - every `const T*` inside af_plan_t / af_sweep_t is HOST memory, borrowed for
 *    the duration of the call (the engine copies what it needs to the device);
 *  - every pointer inside af_outputs_t is DEVICE memory owned by the caller
 *    (e.g. torch tensors); the engine never allocates or frees output buffers;
 *  - all entry points return 0 on success, a negative af_status otherwise, and
 *    leave a thread-local message retrievable through af_last_error();
 *  - one host thread per engine AT A TIME; calls are synchronous with respect to the
 *    returned buffers (the engine's own HIP streams, synchronised before return);
 *    different engines may be called from different host threads at once: an
 *    engine owns its streams, counter block and scratch buffers, the library keeps
 *    no mutable global state besides the RCCL symbol table af_comm_load fills, and
 *    the error message is per thread (tests/test_gpu_flow.py::
 *    test_sweeps_in_flight_on_host_threads_equal_their_lone_runs);
 *  - capacity overflow is reported per scenario in counts[AF_CNT_FLAGS] and is
 *    never a silent drop.
 */
#ifndef ASYNCFLOW_HIP_H
#define ASYNCFLOW_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AF_ABI_VERSION 7

/* ---- status codes ------------------------------------------------------ */
enum af_status {
    AF_OK = 0,
    AF_ERR_INVALID = -1,     /* malformed plan / sweep / outputs            */
    AF_ERR_NO_DEVICE = -2,   /* no HIP device, or device index out of range */
    AF_ERR_HIP = -3,         /* a HIP runtime call failed                   */
    AF_ERR_CAPACITY = -4,    /* requested capacities exceed what a wave can hold */
    AF_ERR_ABI = -5          /* caller built against another AF_ABI_VERSION */
};

/* ---- enumerations mirrored from src/asyncflow/config/constants.py ------- */
/* Distribution (constants.py:39-52) */
enum af_dist {
    AF_DIST_POISSON = 0,
    AF_DIST_NORMAL = 1,
    AF_DIST_LOG_NORMAL = 2,
    AF_DIST_EXPONENTIAL = 3,
    AF_DIST_UNIFORM = 4
};
/* SystemNodes that can be an edge target (constants.py:155-166) */
enum af_node_kind { AF_NODE_CLIENT = 0, AF_NODE_LB = 1, AF_NODE_SERVER = 2 };
/* LbAlgorithmsName (constants.py:144-148) */
enum af_lb_algo { AF_LB_ROUND_ROBIN = 0, AF_LB_LEAST_CONNECTIONS = 1 };
/* EndpointStepCPU / EndpointStepIO (constants.py:58-89); RAM steps are folded
 * into ep_ram at lowering time (server.py:106-110 sums them up front). */
enum af_step_kind { AF_STEP_CPU = 0, AF_STEP_IO = 1 };
/* SampledMetricName (constants.py:195-205) as a bit mask */
enum af_metric_bit {
    AF_METRIC_READY_QUEUE_LEN = 1u << 0,
    AF_METRIC_EVENT_LOOP_IO_SLEEP = 1u << 1,
    AF_METRIC_RAM_IN_USE = 1u << 2,
    AF_METRIC_EDGE_CONCURRENT_CONNECTION = 1u << 3
};

/* ---- the lowered scenario (shared by every scenario of a sweep) -------- */
typedef struct af_plan {
    uint32_t abi_version;  /* = AF_ABI_VERSION                                   */
    uint32_t struct_size;  /* = sizeof(af_plan_t)                                */

    /* SimulationSettings (schemas/settings/simulation.py:13-44) */
    double total_time;     /* total_simulation_time (s)                          */
    double sample_period;  /* sample_period_s (s)                                */
    uint32_t metrics_mask; /* af_metric_bit                                      */

    /* RqsGenerator (schemas/workload/rqs_generator.py:10-59) */
    uint32_t gen_users_dist;   /* AF_DIST_POISSON | AF_DIST_NORMAL               */
    double gen_users_mean;     /* avg_active_users.mean                          */
    double gen_users_sigma;    /* avg_active_users.variance (used AS sigma)      */
    double gen_rpm_mean;       /* avg_request_per_minute_per_user.mean           */
    double gen_window_s;       /* user_sampling_window                           */
    int32_t gen_out_edge;      /* edge index leaving the generator               */

    /* topology (schemas/topology/{nodes,edges,graph}.py) */
    uint32_t n_edges;
    uint32_t n_servers;
    int32_t client_out_edge;   /* edge index leaving the client                  */
    uint32_t has_lb;
    uint32_t lb_algo;          /* af_lb_algo                                     */
    uint32_t n_lb_edges;
    const int32_t* lb_edges;   /* [n_lb_edges] LB out-edges in payload order     */

    const uint8_t* edge_target_kind;  /* [n_edges] af_node_kind                  */
    const int32_t* edge_target_idx;   /* [n_edges] server index (or 0)           */
    const uint8_t* edge_dist;         /* [n_edges] af_dist of latency            */
    const double* edge_mean;          /* [n_edges] latency.mean                  */
    const double* edge_sigma;         /* [n_edges] latency.variance (AS sigma)   */
    const double* edge_dropout;       /* [n_edges] dropout_rate                  */

    const uint32_t* srv_cores;        /* [n_servers] cpu_cores                   */
    const double* srv_ram_mb;         /* [n_servers] ram_mb                      */
    const int32_t* srv_out_edge;      /* [n_servers] edge leaving the server     */
    const uint32_t* srv_ep_begin;     /* [n_servers+1] CSR into endpoints        */

    uint32_t n_endpoints;
    const uint32_t* ep_step_begin;    /* [n_endpoints+1] CSR into steps          */
    const double* ep_ram;             /* [n_endpoints] sum of necessary_ram      */

    uint32_t n_steps;
    const uint8_t* step_kind;         /* [n_steps] af_step_kind                  */
    const double* step_time;          /* [n_steps] cpu_time | io_waiting_time    */

    /* EventInjection timelines, pre-sorted exactly like
     * runtime/events/injection.py:142-151; *_time is the simulation clock at
     * which the mark is applied (relative waits re-accumulated, :181-188). */
    uint32_t n_edge_marks;
    const double* emark_time;         /* [n_edge_marks]                          */
    const int32_t* emark_edge;        /* [n_edge_marks] edge index               */
    const double* emark_delta;        /* [n_edge_marks] +spike_s start / -spike_s end */
    uint32_t n_srv_marks;
    const double* smark_time;         /* [n_srv_marks]                           */
    const int32_t* smark_lb_edge;     /* [n_srv_marks] LB out-edge index, -1 = not behind LB */
    const uint8_t* smark_down;        /* [n_srv_marks] 1 = SERVER_DOWN, 0 = SERVER_UP */
} af_plan_t;

/* ---- per-scenario inputs ------------------------------------------------ */
enum af_param {
    AF_PARAM_GEN_USERS_MEAN = 0,
    AF_PARAM_GEN_USERS_SIGMA = 1,
    AF_PARAM_GEN_RPM_MEAN = 2,
    AF_PARAM_EDGE_MEAN = 3,     /* index = edge  */
    AF_PARAM_EDGE_SIGMA = 4,    /* index = edge  */
    AF_PARAM_EDGE_DROPOUT = 5,  /* index = edge  */
    AF_PARAM_STEP_TIME = 6,     /* index = step  */
    /* ABI 4 -- sweeps over the sampling window, server resources and the injected events
     * (schemas/workload/rqs_generator.py:33-45, schemas/topology/nodes.py:58-69, schemas/events/injection.py:25-119).
     * Timeline columns address mark SLOTS of the plan's pre-sorted timelines: a scenario whose event
     * times sort differently passes its own (time, delta, edge) per slot, so any order is exact. */
    AF_PARAM_GEN_WINDOW = 7,    /* user_sampling_window (s)                                  */
    AF_PARAM_SRV_CORES = 8,     /* index = server; integral value within 1..65535            */
    AF_PARAM_SRV_RAM_MB = 9,    /* index = server                                            */
    AF_PARAM_EMARK_TIME = 10,   /* index = edge-mark slot: emark_time                        */
    AF_PARAM_EMARK_DELTA = 11,  /*                         emark_delta (+spike_s / -spike_s) */
    AF_PARAM_EMARK_EDGE = 12,   /*                         emark_edge (integral value)       */
    AF_PARAM_SMARK_TIME = 13,   /* index = server-mark slot: smark_time                      */
    AF_PARAM_SMARK_LB_EDGE = 14,/*                           smark_lb_edge (-1 = not behind the LB) */
    AF_PARAM_SMARK_DOWN = 15,   /*                           smark_down (0 / 1)              */
    AF_PARAM_COUNT_ = 16
};

typedef struct af_override {
    uint32_t param;        /* af_param                                         */
    uint32_t index;        /* entity index for the indexed params, else 0      */
    const double* values;  /* HOST [n_scenarios]                               */
} af_override_t;

typedef struct af_sweep {
    uint32_t n_scenarios;
    const uint64_t* seeds;            /* HOST [n_scenarios] Philox keys          */
    uint32_t n_overrides;
    const af_override_t* overrides;   /* HOST [n_overrides]                      */
    uint32_t draw_capacity;           /* upper bound on generated requests per scenario: the
                                         engine pre-generates that many random draws per
                                         stream (0 = outputs.clock_capacity)          */
} af_sweep_t;

/* ---- outputs ------------------------------------------------------------- */
/* counts[scenario][AF_CNT_*] */
enum af_count_slot {
    AF_CNT_GENERATED = 0,  /* RqsGeneratorRuntime.id_counter                     */
    AF_CNT_COMPLETED = 1,  /* len(ClientRuntime.rqs_clock)                       */
    AF_CNT_DROPPED = 2,    /* messages lost on edges (edge.py:78-86)             */
    AF_CNT_EVENTS = 3,     /* request-events: arrivals + deliveries + cpu/io step ends */
    AF_CNT_TICKS = 4,      /* sampler ticks taken (collector.py:50-66)           */
    AF_CNT_FLAGS = 5,      /* af_flag bits                                       */
    AF_CNT_MAX_LIVE = 6,   /* high-water mark of live requests                   */
    AF_CNT_MARKS = 7,      /* injection marks applied                            */
    AF_CNT_SLOTS = 8
};
enum af_flag {
    AF_FLAG_POOL_OVERFLOW = 1u << 0,   /* more live requests than request_capacity */
    AF_FLAG_FIFO_OVERFLOW = 1u << 1,   /* a CPU/RAM wait queue exceeded fifo_capacity */
    AF_FLAG_CLOCK_OVERFLOW = 1u << 2,  /* more completions than clock_capacity     */
    AF_FLAG_TICK_OVERFLOW = 1u << 3,   /* more ticks than tick_capacity            */
    AF_FLAG_RAM_STARVED = 1u << 4,     /* a server's RAM queue is blocked for good: a request needs more RAM than
                                          ram_mb (server.py:146-149), or -- fractional needs only -- a RAM put that
                                          simpy refuses by one rounding faces a waiter that does not fit, so that
                                          neither can ever move.  The engine does what the reference does (every
                                          later RAM request of that server waits for ever; tests/golden/ram_starved_t30,
                                          ram_put_deadlock_t20 are the reference's own output); informational */
    AF_FLAG_TIME_TIE = 1u << 5,        /* a zero-delay Timeout that is not a delivery to the
                                          client was created while other zero-time steps were
                                          pending: SimPy may order those steps differently.
                                          Needs a step time or an exponential / log-normal /
                                          uniform latency that does not advance the f64 clock
                                          (probability ~2^-53 per draw): instants shared by
                                          several timed events and zero-latency hops between
                                          servers (poisson / truncated normal) are NOT flagged,
                                          they follow SimPy's event order exactly
                                          (DESIGN.md "Ties"; informational) */
    AF_FLAG_DRAW_OVERFLOW = 1u << 6,   /* more arrivals than draw_capacity            */
    /* (bits 7..12 are internal to the engine and never visible in the outputs) */
    AF_FLAG_NEGATIVE_DELAY = 1u << 13  /* a message was sent with transit + spike < 0: the residue of overlapping
                                          spikes' += / -= (injection.py:191-198) under a zero transit time.  The
                                          reference raises there (simpy: ValueError "Negative delay", edge.py:107);
                                          the engine delivers at now + (transit + spike) and reports the scenario:
                                          asyncflow_amd.SimulationRunner raises the same ValueError for it */
    /* (bit 14 was AF_FLAG_RAM_PUT_BLOCKED in ABI 6: simpy's waiting Container.put is modelled since ABI 7, never reported) */
};

typedef struct af_outputs {
    /* RqsClock list (metrics/client.py:9-18): (start, finish) per completion,
     * in completion order.  DEVICE [n_scenarios][clock_capacity][2] f64. */
    uint32_t clock_capacity;
    double* clock;
    /* Sampled series (metrics/collector.py:50-66).
     * DEVICE [n_scenarios][tick_capacity][af_series_pitch(plan)] 4-byte words (one
     * 16-byte aligned row per tick; pitch = n_series rounded up to 4), series order:
     *   e in [0,n_edges):            edge_concurrent_connection (int32)
     *   n_edges + 3*s + 0:           ready_queue_len   of server s (int32)
     *   n_edges + 3*s + 1:           event_loop_io_sleep of server s (int32)
     *   n_edges + 3*s + 2:           ram_in_use        of server s (float32)
     * May be NULL (series not stored; ticks still counted). */
    uint32_t tick_capacity;
    uint32_t* samples;
    /* DEVICE [n_scenarios][AF_CNT_SLOTS] u32 */
    uint32_t* counts;
    /* Optional summary accumulated by the next-event kernel itself, for sweeps whose rqs_clock
     * (16 B per completion) is not wanted: per scenario a linear latency histogram over
     * [0, online_hist_max) whose last bin also takes the overflow (same binning as
     * af_summary_t.hist) and the completions per 1-s window (k-1, k] (analyzer.py:112-121).
     * DEVICE u32 arrays ZEROED BY THE CALLER; NULL = off.  Exact integer counts; percentiles read
     * from the histogram are accurate to one bin. */
    uint32_t online_hist_bins;
    double online_hist_max;
    uint32_t* online_hist;      /* [n_scenarios][online_hist_bins] */
    uint32_t online_rps_buckets;
    uint32_t* online_rps;       /* [n_scenarios][online_rps_buckets] */
} af_outputs_t;

#define AF_MAX_REQUEST_CAPACITY 65535u
#define AF_MAX_FIFO_CAPACITY 1048576u /* rounded up to a power of two by the engine.  (ABI <= 6: 16 384.  The reference's simpy
                                         Container queues have no bound -- server.py:146-149, 210-227 --; a saturated server's
                                         backlog grows with the horizon, and 2^20 waiters per server queue is what a scenario
                                         may cost in HBM: 32 B per slot and server and queue pair) */

typedef struct af_engine_options {
    uint32_t request_capacity;  /* live requests per scenario (0 = engine default, <= AF_MAX_REQUEST_CAPACITY) */
    uint32_t fifo_capacity;     /* waiters per server queue   (0 = engine default, <= AF_MAX_FIFO_CAPACITY)   */
    uint32_t force_global_state;/* 1 = keep per-scenario state in HBM even if it fits LDS */
    uint32_t lanes_per_wave;    /* scenarios per wavefront: power of two <= 64, 0 = auto
                                   (few scenarios are spread over many narrow waves)    */
    uint32_t draw_memory_mb;    /* HBM budget for the pre-generated draws of one chunk of the
                                   sweep, MiB (0 = min(160 GiB, 60 % of the free memory));
                                   larger sweeps run as several chunks                   */
    uint32_t expect_shared_instants; /* 1 = start with the kernel variant that replays SimPy's
                                   event order at instants shared by several timed events
                                   (~20 % slower).  0 = lean variant first; scenarios that
                                   meet such an instant are handed over to the other variant
                                   and the engine remembers it for its later runs          */
    /* Stage-parallel ("flow") kernel: one wavefront per scenario moves 64 requests per step through
     * the stations of a feed-forward request path (generator -> client -> [LB, round robin or least connections ->] servers
     * with IO* CPU* IO* endpoints -> client).  Bit-identical to the next-event kernels; a scenario
     * it cannot express (two events of one station at one instant, a list / tick-ring overflow) is
     * simulated again by them.  af_engine_flow_reason() tells why a plan is outside its range. */
    uint32_t flow_mode;         /* 0 = use it whenever the plan is in range -- plans whose servers need the
                                   event-by-event station (several endpoints per server, step programs that come
                                   back to the core queue) only for sweeps of <= 8 scenarios, above that the
                                   next-event kernels are faster for them; 1 = never; 2 = whenever in range  */
    uint32_t flow_list_entries; /* capacity of each station's message list: 64, 128 or 256
                                   (0 = from the expected number of messages in flight)         */
    uint32_t flow_ring_rows;    /* rows of the LDS ring of per-tick differences (power of two);
                                   0 = auto (a window of a few batches of arrivals + the time a
                                   request spends inside a server; edges slower than the ring
                                   reaches are handled by the receiving station);
                                   AF_FLOW_RING_IN_HBM = keep the differences in the sample rows
                                   in HBM (no limit on how far an interval reaches)            */
} af_engine_options_t;
#define AF_FLOW_RING_IN_HBM 0xFFFFFFFFu

typedef struct af_stats {
    double kernel_ms;           /* HIP-event time of the next-event kernel (af_des_kernel) */
    double pregen_ms;           /* HIP-event time of the draw pre-generation kernels       */
    double h2d_ms;              /* seeds/overrides upload                          */
    double summary_ms;          /* last af_engine_summarize (both kernels)         */
    uint64_t draw_bytes;        /* size of the pre-generated draw arrays (HBM)     */
    uint64_t state_bytes_per_scenario;
    uint32_t state_in_lds;      /* 1 = LDS-resident state, 0 = HBM-resident        */
    uint32_t lds_bytes_per_wave;
    uint32_t waves;             /* workgroups launched (one wavefront each)        */
    uint32_t lanes_per_wave;    /* scenarios carried by each wavefront             */
    uint32_t chunks;            /* sub-launches the sweep was split into           */
    uint32_t specialised_launches; /* next-event launches that used kernels from af_engine_set_kernels */
    uint32_t shared_instant_scenarios; /* scenarios in which two timed events shared an instant:
                                   simulated a second time by the kernel variant that replays
                                   SimPy's event-by-event order (0 when the engine started
                                   with that variant)                              */
    uint32_t request_capacity;
    uint32_t fifo_capacity;
    /* stage-parallel kernel (last af_engine_run) */
    double flow_kernel_ms;         /* HIP-event time of the stage-parallel kernel, 0 = not used      */
    uint32_t flow_scenarios;       /* scenarios it was launched on                                  */
    uint32_t flow_fallback;        /* ... of which handed back by the first launch, by reason:        */
    uint32_t flow_fallback_tie;    /*   two events of one station (or an event and a tick / mark) at one instant */
    uint32_t flow_fallback_list;   /*   more messages pending at a station than flow_list_entries   */
    uint32_t flow_fallback_ring;   /*   a request stayed in its server (or, fast-hop launches, a message on its edge)
                                        longer than the tick ring reaches                          */
    uint32_t flow_fallback_ram;    /*   RAM admission the recurrence cannot express                 */
    uint32_t flow_retried;         /* handed-back scenarios run again by the kernel's most tolerant instantiation
                                      (256-entry lists carrying send times, tick differences in HBM)             */
    uint32_t flow_to_next_event;   /* scenarios finally simulated by the next-event kernels                       */
    uint32_t flow_list_entries;    /* layout used                                                   */
    uint32_t flow_ring_rows;       /* (0 = differences kept in HBM)                                 */
    uint32_t flow_lds_bytes;       /* LDS per wavefront                                             */
    uint32_t jit_fallbacks;        /* launches that wanted plan-specialised kernels but ran the generic ones */
    double gather_ms;              /* last af_engine_gather (HIP events around the grouped all-gather)        */
    uint32_t pregen_group;         /* arrival pre-generation of the stage-parallel path: scenarios per workgroup of
                                      af_arrival_groups, 0 = the row kernel                                   */
    uint32_t summary_overlapped;   /* af_engine_run_summarized: scenarios whose analyzer ran on a second stream beside the
                                      last residency round of the stage-parallel kernel (0: everything after the run) */
    double summary_beside_ms;      /* ... HIP-event time of those analyzer kernels; summary_ms is then what was NOT hidden */
} af_stats_t;

typedef struct af_engine af_engine_t;

/* Replaces: SimulationRunner.__init__ + _build_* (simulation_runner.py:52-294).
 * device = AF_DEVICE_PLAN_ONLY makes a planning-only engine: it owns no device state and no HIP call is made for it, so it
 * can be created on a machine without a GPU.  It answers af_engine_jit_spec for sweeps of the stage-parallel kernel (the
 * spec is a pure function of plan, sweep and output shape), af_engine_flow_reason and af_engine_stats; every call that
 * would touch the device returns AF_ERR_NO_DEVICE.  Used to pre-build plan-specialised kernels where hipcc is (the build
 * machine) for a box where it may not be. */
#define AF_DEVICE_PLAN_ONLY (-1)
int af_engine_create(const af_plan_t* plan, int device, const af_engine_options_t* opts,
                     af_engine_t** out);
/* Plan-specialised kernels (optional).  The library contains generic next-event kernels; for long
 * sweeps a host may compile asyncflow_amd/csrc/engine.hip once more with the plan's shape as
 * compile-time constants (state offsets become instruction immediates, loops over edges / servers /
 * series unroll: ~8 % less kernel time on the 10k LB-2 sweep) and hand the code object over:
 *   af_engine_jit_spec   writes the hipcc -D flags that describe what af_engine_run(sweep, out) would
 *                        launch (NUL-terminated, deterministic: usable as a cache key); build with
 *                        hipcc --genco --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off <flags>
 *   af_engine_set_kernels  loads the code object; launches whose spec differs from `spec` (another
 *                        sweep shape, the second pass over a subset) keep using the generic kernels.
 *                        NULL image: unload.  Results are bit-identical either way. */
int af_engine_jit_spec(af_engine_t* engine, const af_sweep_t* sweep, const af_outputs_t* out, char* buf, size_t cap);
int af_engine_set_kernels(af_engine_t* engine, const char* spec, const void* image, size_t size);

/* Batched analyzer on the device (replaces ResultsAnalyzer._process_event_metrics,
 * src/asyncflow/metrics/analyzer.py:83-126, for every scenario of a finished af_engine_run):
 * per-scenario latency statistics in LatencyKey order
 *   {total_requests, mean, median, std_dev, p95, p99, min, max}
 * (order statistics exact, numpy 'linear' interpolation; scenarios without completions: total 0,
 * the rest NaN), the 1-s throughput windows (k-1, k], k = 1..rps_buckets, an optional linear latency
 * histogram over [0, hist_max) whose last bin also takes the overflow, and the mean / maximum of
 * every sampled series.  All buffers are DEVICE memory owned by the caller; NULL skips an output. */
typedef struct af_summary_t {
    uint32_t n_scenarios;
    uint32_t rps_buckets;   /* floor(total_time)                                        */
    uint32_t hist_bins;     /* <= 8192                                                  */
    double hist_max;        /* seconds                                                  */
    double* stats;          /* [n][8] f64                                               */
    float* rps;             /* [n][rps_buckets] f32                                     */
    uint32_t* hist;         /* [n][hist_bins] u32                                       */
    double* series_mean;    /* [n][af_series_count] f64 (needs outputs.samples)         */
    uint32_t* series_max;   /* [n][af_series_count] u32                                 */
} af_summary_t;
/* series_mean / series_max over the m = min(counts[AF_CNT_TICKS], tick_capacity) stored rows of a scenario (m = 0: NaN / 0).
 * Integer series: (double)(exact integer sum) / (double)m and the largest word.  ram_in_use (float32 words, column
 * n_edges + 3 * server + 2): series_max is the FLOAT maximum, returned as its float32 bits -- also where the reference's
 * own arithmetic left negative residues such as -2.8e-14 in the column, whose words are larger than every positive
 * value's; series_mean is the f64 sum of the float values, per-thread partial sums added in a fixed order, divided once:
 * bit-equal to numpy's mean while the values add exactly (multiples of 1/256 below 2^16), otherwise within
 * m * 2^-52 * sum|x| / m of the exactly rounded sum / m; identical from run to run and in every batch.
 * rps_buckets + hist_bins <= 24 576 (words of LDS beside the kernel's own; AF_ERR_CAPACITY beyond). */

/* `out` is the af_outputs_t the run filled (clock + counts are required, samples only for the
 * series outputs).  Synchronous like af_engine_run. */
int af_engine_summarize(af_engine_t* engine, const af_outputs_t* out, const af_summary_t* summary);

/* Pooled analyzer: the same eight statistics per GROUP of scenarios, all latencies of a group taken as one sample
 * (a grid point's replicas: what a long reference run estimates).  Group g's sample is the concatenation, in ascending
 * scenario index, of finish - start over the stored rows of its scenarios (min(counts[AF_CNT_COMPLETED], clock_capacity)
 * each); every statistic is bit-equal to numpy's on that array, mean and std_dev included.  A group without completions:
 * total 0, the rest NaN.  group[s] = AF_POOL_SKIP leaves scenario s out; any other id must be < n_groups.  A group of 2^32
 * or more latencies is refused (AF_ERR_CAPACITY).  The engine keeps a scratch buffer of 8 B per pooled completion plus
 * ~56 KB per group (asyncflow_amd/csrc/af_pooled.hpp).  Synchronous like af_engine_summarize; the struct is written back
 * (elapsed_ms), hence the non-const pointer. */
#define AF_POOL_SKIP 0xFFFFFFFFu
typedef struct af_pooled {
    uint32_t n_scenarios;
    uint32_t n_groups;
    const uint32_t* group;  /* DEVICE [n_scenarios] group id per scenario; NULL: all in group 0 */
    double* stats;          /* DEVICE [n_groups][8] f64, LatencyKey order as af_summary_t.stats */
    double elapsed_ms;      /* out: wall time of the call */
} af_pooled_t;
int af_engine_summarize_pooled(af_engine_t* engine, const af_outputs_t* out, af_pooled_t* pooled);

/* Latency statistics per TIME WINDOW and group on the device (asyncflow_amd/csrc/af_windowed.hpp): what one would compute on
 * the host by masking every scenario's rqs_clock by finish time -- p95 DURING an outage, how fast it recovers.  With
 * edges[0] < edges[1] < ... < edges[n_windows] (finite seconds), m_s = min(counts[s][AF_CNT_COMPLETED], clock_capacity) and
 * r_s[k] = #{ i < m_s : finish[s, i] <= edges[k] } (np.searchsorted(finish, edges, side="right")), window w of scenario s
 * is its rows [r_s[w], r_s[w + 1]), i.e. edges[w] < finish <= edges[w + 1], the bucket rule of the throughput series
 * (analyzer.py:107-125); rows with finish <= edges[0] or > edges[n_windows] belong to no window.  The sample of (group g,
 * window w) is the concatenation, in ascending scenario index over the members of g, of finish - start over those rows;
 * stats[g][w][0..7] are numpy's on that array, bit for bit, in LatencyKey order (an empty sample: total 0, the rest NaN).
 * This rests on rqs_clock rows being in completion order (the client appends at env.now): finish is non-decreasing within
 * a scenario.  The call CHECKS that on every stored row of every scenario it uses and returns AF_ERR_INVALID naming a
 * scenario that breaks it, writing no statistics.  group as in af_pooled_t.  n_groups * n_windows must be < 2^32 - 1 and
 * a (group, window) must hold < 2^32 latencies (AF_ERR_CAPACITY).  Scratch kept by the engine (shared with
 * af_engine_summarize_pooled): 8 B per windowed latency + 8 B per (scenario, edge) + at most 12 B per (group, window) + the
 * pooled analyzer's ~56 KB for every (group, window) of more than 8 192 latencies only.  Synchronous; the struct is written
 * back. */
typedef struct af_windows {
    uint32_t n_scenarios;
    uint32_t n_groups;
    uint32_t n_windows;
    const uint32_t* group;   /* DEVICE [n_scenarios] group id per scenario (AF_POOL_SKIP: left out); NULL: all in group 0 */
    const double* edges;     /* HOST [n_windows + 1] strictly increasing, finite */
    double* stats;           /* DEVICE [n_groups][n_windows][8] f64 */
    uint32_t* row_bounds;    /* DEVICE [n_scenarios][n_windows + 1] out, optional: r_s[k] (also of skipped scenarios) */
    double elapsed_ms;       /* out: wall time of the call */
    uint64_t scratch_bytes;  /* out: size of the engine's scratch after the call */
} af_windows_t;
int af_engine_summarize_windows(af_engine_t* engine, const af_outputs_t* out, af_windows_t* windows);

/* The same statistics with windows by ARRIVAL time (asyncflow_amd/csrc/af_arrival.hpp): window w of scenario s holds its rows
 * with edges[w] < start <= edges[w + 1] (a start equal to an edge belongs to the window that ends there; rows with start <=
 * edges[0] or > edges[n_windows] belong to no window) -- the cohort of the requests SENT in the window, which is what an
 * objective is written against: by finish time the slow requests of an outage are charged to the recovery.  start is not
 * sorted in rqs_clock, so a window is a scattered subset of a scenario's rows; they stay in row (completion) order, and the
 * sample of (group g, window w) is their concatenation in ascending scenario index over the members of g, on which stats
 * are numpy's bit for bit.  The request, its refusals and the scratch are af_engine_summarize_windows's, except: nothing rests
 * on completion order, so it is not checked and there is no such error; row_bounds, if given, receives
 * c_s[k] = #{ i < m_s : start[s, i] <= edges[k] }, CUMULATIVE ARRIVAL COUNTS (not row ranges), also of skipped scenarios.
 * The cohorts are RIGHT-CENSORED: a request that arrived in a window but had not completed when the run ended, or was
 * dropped, is in no row; total is the cohort's completions, not its arrivals, and the last windows of a run under-report
 * slow requests. */
int af_engine_summarize_arrival_windows(af_engine_t* engine, const af_outputs_t* out, af_windows_t* windows);

/* Statistics of every SAMPLED SERIES per window of ticks and group on the device (asyncflow_amd/csrc/af_series_windows.hpp):
 * how long the ready queue of a server is DURING an outage, at each grid point.  Windows are on TICK INDICES: sample k of
 * scenario s is row k of its outputs.samples block, k = 0 .. m_s - 1, m_s = min(counts[s][AF_CNT_TICKS], tick_capacity); the
 * reference labels it k * sample_period (analyzer.py:239-244) although the collector takes it at (k + 1) * period
 * (collector.py:53), and the windows follow the label.  With tick_edges b[0] < b[1] < ... < b[n_windows], window w of
 * scenario s is its rows [min(b[w], m_s), min(b[w + 1], m_s)); rows at or past m_s and the padding words of a row are never
 * read.  The sample of (group g, window w, series j) is column j over those rows of every member of g (group as in
 * af_pooled_t).  Per (g, w): count, the values in the cell.  Per (g, w, j): mean -- integer series: the exact integer sum,
 * divided once, (double)sum / (double)count, bit-equal to np.mean of the int64 values while the sum is below 2^53;
 * ram_in_use (float32 words, column n_edges + 3 * server + 2): the f64 sum of the float values, divided once --; minv /
 * maxv as 4-byte words: of an integer series the smallest / largest word; of ram_in_use the float MINIMUM / MAXIMUM of the
 * values, returned as float32 bits, with -0.0 below +0.0 (the IEEE total order on the non-NaN values; the -2.8e-14 residues
 * that the reference's own arithmetic can leave in ram_in_use are the smallest values of their cells, not the largest).  One
 * window over a scenario's whole run therefore has maxv equal to af_summary_t.series_max word for word, and on non-negative
 * values the float order is the order of the words; above: the values > thresholds[j], compared as f64 (+0.0 is not above
 * -0.0; NULL: 0.0 each, the non-zero samples).  An empty cell: count
 * 0, mean NaN, minv = maxv = above = 0.
 * Exactness: no atomics; the f64 partial sums of a float column are combined in a fixed order (within a scenario's window:
 * a lane's rows top down, then a fixed tree over the lanes; across the members of a group: ascending scenario index), so the
 * result is identical from run to run and does not depend on the batch a scenario sits in.  When every value of a cell is a
 * multiple of 1/256 below 2^16 and count < 2^29, every partial sum is exact and the mean is bit-equal to numpy's; otherwise it
 * is within (count - 1) * 2^-53 relative of the exactly rounded sum / count.
 * Refused: tick_edges not strictly increasing or n_windows = 0, a NaN threshold, a group id >= n_groups, outputs.samples
 * NULL (AF_ERR_INVALID); a cell of 2^32 or more values, n_groups * n_windows >= 2^32 - 1, tick_capacity >= 2^31
 * (AF_ERR_CAPACITY); a planning-only engine (AF_ERR_NO_DEVICE).  Any number of series (af_engine_summarize stops at 1 024
 * padded ones).  `out` needs samples, tick_capacity and counts; clock is not read.
 * Scratch kept by the engine (shared with the pooled and windowed analyzers): 4 B per edge + 8 B per series + 4 B per group
 * + 4 B per scenario + 2 KB of alignment, and -- unless every group holds at most one scenario -- 20 B per (scenario,
 * window, series).  Synchronous; the struct is written back. */
typedef struct af_series_windows {
    uint32_t n_scenarios;
    uint32_t n_groups;
    uint32_t n_windows;
    const uint32_t* group;       /* DEVICE [n_scenarios] group id per scenario (AF_POOL_SKIP: left out); NULL: all in group 0 */
    const uint32_t* tick_edges;  /* HOST [n_windows + 1] strictly increasing */
    const double* thresholds;    /* HOST [af_series_count] or NULL (0.0 each) */
    uint32_t* count;             /* DEVICE [n_groups][n_windows] */
    double* mean;                /* DEVICE [n_groups][n_windows][af_series_count] f64 */
    uint32_t* minv;              /* DEVICE, same shape, 4-byte words; NULL skips */
    uint32_t* maxv;              /* DEVICE, same shape; NULL skips */
    uint32_t* above;             /* DEVICE, same shape; NULL skips */
    double elapsed_ms;           /* out: wall time of the call */
    uint64_t scratch_bytes;      /* out: size of the engine's scratch after the call */
} af_series_windows_t;
int af_engine_summarize_series_windows(af_engine_t* engine, const af_outputs_t* out, af_series_windows_t* series_windows);

/* Exact QUANTILES OF THE SAMPLED SERIES per window of ticks, group and series on the device
 * (asyncflow_amd/csrc/af_series_quantiles.hpp): how much RAM covers 99 % of the ticks during an outage at a grid point, the
 * median ready-queue length of every 10 s window, the p95 of edge concurrency a connection pool must be sized for.
 * Cells: those of af_series_windows_t.  Window w of scenario s is its sample rows [min(b[w], m_s), min(b[w + 1], m_s)), with
 * m_s = min(counts[s][AF_CNT_TICKS], tick_capacity); rows at or past m_s and the padding words of a row are never read.  The
 * sample of (g, w, j) is column j over those rows of every member of g (group as in af_pooled_t).
 * Key: every word has a 32-bit key -- of an integer series the word itself, unsigned; of a ram_in_use column (index n_edges +
 * 3 * server + 2) the float32 word w mapped to (w & 0x80000000) ? ~w : (w | 0x80000000), the IEEE total order on non-NaN
 * floats with -0.0 below +0.0 (no NaN is sampled).  Sort the sample by key; x[0 .. n-1] are the values in that order as f64:
 * (double)word of an integer series, (double)(float) of ram_in_use.  For a level q in [0, 1]:
 *     v = (double)(n - 1) * q;  lo = floor(v);  hi = min(lo + 1, n - 1);  t = v - lo;  d = x[hi] - x[lo];
 *     quantile = t >= 0.5 ? x[hi] - d * (1 - t) : x[lo] + d * t
 * which is np.quantile(values, q) (method 'linear'): bit for bit where the cell holds no zero, equal under == everywhere (numpy's
 * sort leaves -0.0 and +0.0 in input order).  Levels 0 and 1 are af_series_windows_t's minv / maxv as values.  An empty cell:
 * count 0, every quantile NaN.  Output column c belongs to columns[c]: any order, duplicates allowed.
 * Independence: a cell's result does not depend on which other cells, levels or columns the call holds, on the batch a scenario
 * sits in, or on the run: selection by sorting and counting, integer atomics only; no floating-point number is ever added
 * across elements.
 * Refused, no output buffer touched: n_levels == 0 or more than AF_MAX_SERIES_QUANTILE_LEVELS, a level that is NaN or outside
 * [0, 1], tick_edges not strictly increasing or n_windows == 0, a column index >= af_series_count, n_columns == 0 with columns
 * != NULL or the reverse, a group id >= n_groups, outputs.samples NULL (AF_ERR_INVALID); a cell of 2^32 or more values,
 * n_groups * n_windows >= 2^32 - 1, tick_capacity >= 2^31 (AF_ERR_CAPACITY); a planning-only engine (AF_ERR_NO_DEVICE).
 * `out` needs samples, tick_capacity and counts; clock is not read.
 * Scratch kept by the engine (shared with the other group analyzers), with C the output columns, U the distinct series among
 * them, P the plan's padded series (af_series_pitch) and L the cells of more than 2 048 values per column:
 *     4 B per edge + 8 B per level + 4 B per group + 4 B per scenario + 5 B per padded series + 8 U + 4 C + 8 B per cell of at
 *     most 2 048 values + 5 376 B of alignment, and only where L > 0:
 *     4 B per cell + 8 L + min(L, max(1, floor(128 MiB / (U * K)))) * U * K,   K = 2 * n_levels * 8 208 + 12 bytes
 * (one 2 048-bin histogram per wanted rank, column and cell of a chunk of large cells; the chunks run one after the other).
 * Synchronous; the struct is written back. */
#define AF_MAX_SERIES_QUANTILE_LEVELS 16
typedef struct af_series_quantiles {
    uint32_t n_scenarios;
    uint32_t n_groups;
    uint32_t n_windows;
    const uint32_t* group;       /* DEVICE [n_scenarios] group id per scenario (AF_POOL_SKIP: left out); NULL: all in group 0 */
    const uint32_t* tick_edges;  /* HOST [n_windows + 1] strictly increasing */
    uint32_t n_levels;
    const double* levels;        /* HOST [n_levels], each in [0, 1] */
    uint32_t n_columns;
    const uint32_t* columns;     /* HOST [n_columns] series indices < af_series_count, any order, duplicates allowed;
                                    NULL with n_columns == 0: every series, in device order */
    uint32_t* count;             /* DEVICE [n_groups][n_windows]; NULL skips */
    double* quantiles;           /* DEVICE [n_groups][n_windows][C][n_levels] f64, C = n_columns or af_series_count */
    double elapsed_ms;           /* out: wall time of the call */
    uint64_t scratch_bytes;      /* out: size of the engine's scratch after the call */
} af_series_quantiles_t;
int af_engine_summarize_series_quantiles(af_engine_t* engine, const af_outputs_t* out, af_series_quantiles_t* series_quantiles);

/* EXCURSIONS OF THE SAMPLED SERIES ABOVE A THRESHOLD per scenario, window of ticks and series on the device
 * (asyncflow_amd/csrc/af_series_excursions.hpp): how long the ready queue of a server stayed above 50 after another went down,
 * when it had come back below (and whether it had by the horizon), how many separate backlogs formed, when the peak was.
 * Cells: those of af_series_windows_t, always PER SCENARIO -- a duration is a property of one replica's path, so there is no
 * group.  With tick_edges b[0] < ... < b[W] and m_s = min(counts[s][AF_CNT_TICKS], tick_capacity), cell (s, w, j) is column j
 * over the rows k in [lo, hi), lo = min(b[w], m_s), hi = min(b[w + 1], m_s); rows at or past m_s and the padding words of a row
 * are never read.  x[k] is the value as f64 exactly as af_series_windows_t.above takes it -- (double)word of an integer
 * series, (double)(float) of a ram_in_use column -- and tick k is ABOVE when x[k] > thresholds[j], compared as f64 (+0.0 is
 * not above -0.0, a -2^-45 residue is not above 0.0; NULL: 0.0 each).  A RUN is a maximal stretch of consecutive above ticks
 * inside [lo, hi): runs are clipped at the window's edges, and a run that crosses an edge counts in both windows with its
 * clipped lengths.  Outputs, u32, AF_TICK_NONE for "no such tick":
 *     count          [n][W]      hi - lo
 *     above          [n][W][S]   the above ticks; word for word af_series_windows_t.above of singleton groups
 *     runs           same        the runs
 *     longest        same        the length in ticks of the longest run; 0: none
 *     longest_start  same        the first tick (absolute row index) of the earliest run of that length; NONE: none
 *     first          same        the smallest above k; NONE: none
 *     last           same        the largest above k; NONE: none.  last == hi - 1: still above at the end of the window (not
 *                                recovered, censored by the window); otherwise last + 1 is the tick at which it had come back
 *                                for good
 *     peak_tick      same        the smallest k whose key is the cell's largest; NONE in an empty cell.  The key is the series
 *                                analyzers': the word of an integer series, of a ram_in_use word w the value
 *                                (w & 0x80000000) ? ~w : (w | 0x80000000), so -0.0 < +0.0; the peak value itself is
 *                                af_series_windows_t.maxv
 * A NULL output pointer skips that output.  An empty cell: count 0, the counts 0, the ticks NONE.
 * Exactness: one streaming pass that reads every stored row inside the windows once; every combining operation is an integer
 * +, min or max: no atomics, no floating-point addition; the result does not depend on the launch, on the batch a scenario
 * sits in, or on the run.
 * Refused, no output touched: n_scenarios == 0 or n_windows == 0, tick_edges NULL or not strictly increasing, a NaN threshold,
 * outputs.samples or outputs.counts NULL, tick_capacity == 0 (AF_ERR_INVALID); n_scenarios * n_windows >= 2^32 - 1, tick_capacity >= 2^31
 * (AF_ERR_CAPACITY); a planning-only engine (AF_ERR_NO_DEVICE).  `out` needs samples, tick_capacity and counts; clock is not
 * read.  Any number of series.
 * Scratch kept by the engine (shared with the other analyzers): 4 B per edge + 8 B per series + 512 B of alignment -- the
 * edges and the thresholds only, no per-cell records.  Synchronous; the struct is written back. */
#define AF_TICK_NONE 0xFFFFFFFFu
typedef struct af_series_excursions {
    uint32_t n_scenarios;
    uint32_t n_windows;
    const uint32_t* tick_edges;  /* HOST [n_windows + 1] strictly increasing */
    const double* thresholds;    /* HOST [af_series_count] or NULL (0.0 each) */
    uint32_t* count;             /* DEVICE [n_scenarios][n_windows]; NULL skips */
    uint32_t* above;             /* DEVICE [n_scenarios][n_windows][af_series_count]; NULL skips (as every output below) */
    uint32_t* runs;
    uint32_t* longest;
    uint32_t* longest_start;
    uint32_t* first;
    uint32_t* last;
    uint32_t* peak_tick;
    double elapsed_ms;           /* out: wall time of the call */
    uint64_t scratch_bytes;      /* out: size of the engine's scratch after the call */
} af_series_excursions_t;
int af_engine_summarize_series_excursions(af_engine_t* engine, const af_outputs_t* out, af_series_excursions_t* series_excursions);

/* OCCUPANCY HISTOGRAMS OF THE SAMPLED SERIES per window of ticks, group and output column on the device
 * (asyncflow_amd/csrc/af_series_histogram.hpp): P(queue length = k) per window and grid point, the distribution an M/M/c or
 * Erlang check compares against; while no value falls outside the bins it also holds every quantile of an integer series.
 * Cells: those of af_series_windows_t.  Window w of scenario s is its sample rows [min(b[w], m_s), min(b[w + 1], m_s)), with
 * m_s = min(counts[s][AF_CNT_TICKS], tick_capacity); rows at or past m_s and the padding words of a row are never read.  The
 * sample of (g, w, c) is series columns[c] over those rows of every member of g (group as in af_pooled_t).  Output column c
 * has a binning of its own, lo[c] and width[c] (NULL, both: 0.0 and 1.0 each), so one series may appear twice with two
 * binnings.  Bin of a value, bit for bit: x is the value as f64 exactly as af_series_windows_t.above takes it -- (double)word
 * of an integer series, (double)(float) of a ram_in_use column --;
 *     x < lo[c]                      -> under   (-0.0 is not below 0.0; a -2^-45 residue is)
 *     t = (x - lo[c]) / width[c]     one f64 subtraction and one f64 division, each rounded to nearest
 *     t >= (double)n_bins            -> over
 *     otherwise                      -> bin (uint32_t)t
 * Outputs, u32: count [G][W] the values in the cell per column; hist [G][W][C][n_bins]; under, over [G][W][C], with
 * under + sum(hist) + over == count for every cell and column.  A NULL count / under / over skips that output.  An empty
 * cell, or a group without members: zeros everywhere.
 * Exactness: one streaming pass; every combining operation is an integer + (integer atomics on zeroed outputs): the result
 * does not depend on the launch, on the batch a scenario sits in, on which other columns the call holds, or on the run.
 * Refused, no output buffer touched: n_bins == 0 or more than AF_MAX_SERIES_HISTOGRAM_BINS, a width that is <= 0, NaN or
 * infinite, a lo that is NaN or infinite, exactly one of lo / width NULL, tick_edges NULL or not strictly increasing or
 * n_windows == 0, a column index >= af_series_count, n_columns == 0 with columns != NULL or the reverse, a group id >=
 * n_groups, outputs.samples or outputs.counts NULL, hist NULL (AF_ERR_INVALID); a cell of 2^32 or more values, n_groups *
 * n_windows >= 2^32 - 1, tick_capacity >= 2^31 (AF_ERR_CAPACITY); a planning-only engine (AF_ERR_NO_DEVICE).  `out` needs
 * samples, tick_capacity and counts; clock is not read.
 * Scratch kept by the engine (shared with the other analyzers): 4 B per edge + 4 B per series + 24 B per output column +
 * 1 544 B -- the edges, the columns sorted by series with their lo / width and the passes they are read in; the group ids are
 * read where the caller keeps them.  No per-element and no per-cell records.  Synchronous; the struct is written back. */
#define AF_MAX_SERIES_HISTOGRAM_BINS 1024
typedef struct af_series_histogram {
    uint32_t n_scenarios;
    uint32_t n_groups;
    uint32_t n_windows;
    const uint32_t* group;       /* DEVICE [n_scenarios] group id per scenario (AF_POOL_SKIP: left out); NULL: all in group 0 */
    const uint32_t* tick_edges;  /* HOST [n_windows + 1] strictly increasing */
    uint32_t n_columns;
    const uint32_t* columns;     /* HOST [n_columns] series indices < af_series_count, any order, duplicates allowed;
                                    NULL with n_columns == 0: every series, in device order */
    uint32_t n_bins;             /* 1 .. AF_MAX_SERIES_HISTOGRAM_BINS */
    const double* lo;            /* HOST [C] finite, C = n_columns or af_series_count; NULL (with width): 0.0 each */
    const double* width;         /* HOST [C] finite and > 0; NULL (with lo): 1.0 each */
    uint32_t* count;             /* DEVICE [n_groups][n_windows]; NULL skips */
    uint32_t* hist;              /* DEVICE [n_groups][n_windows][C][n_bins] */
    uint32_t* under;             /* DEVICE [n_groups][n_windows][C]; NULL skips */
    uint32_t* over;              /* DEVICE [n_groups][n_windows][C]; NULL skips */
    double elapsed_ms;           /* out: wall time of the call */
    uint64_t scratch_bytes;      /* out: size of the engine's scratch after the call */
} af_series_histogram_t;
int af_engine_summarize_series_histogram(af_engine_t* engine, const af_outputs_t* out, af_series_histogram_t* series_histogram);

/* COMBINATIONS ACROSS THE SAMPLED SERIES per tick, then per window of ticks and group, on the device
 * (asyncflow_amd/csrc/af_series_combined.hpp): the RAM the whole fleet holds at its peak (the peak of a sum is not the sum of
 * the peaks), the requests queued across all servers during an outage, the imbalance (max - min) of the servers' queues under
 * a load-balancing algorithm, the connections open on the edges that end at one node.
 * A COMBINATION c is (op[c], columns cols[col_start[c] .. col_start[c + 1] - 1]): op is AF_COMBINE_SUM, _MIN, _MAX or _SPREAD;
 * the columns are a non-empty, strictly increasing list of series indices < af_series_count, either all integer series or all
 * ram_in_use columns (index n_edges + 3 * server + 2).  At most AF_MAX_SERIES_COMBINATIONS a call.
 * Per-tick value v of combination c at sample row k of scenario s:
 *     integer columns   the words as unsigned 32-bit integers: sum their exact sum (64 bits), min / max the smallest / largest
 *                       word, spread max - min; all exact integers; as f64, x = (double)v
 *     ram_in_use        each word is (double)(float)word: sum the f64 sum in ascending series index, left to right from the
 *                       first column's value, one rounding per addition (the sum of -0.0s is -0.0); min / max in the IEEE total
 *                       order on the non-NaN values with -0.0 below +0.0, the order af_series_windows_t uses; spread max - min
 *                       as one f64 subtraction; x = v
 * Cells: those of af_series_windows_t.  Window w of scenario s is its sample rows [min(b[w], m_s), min(b[w + 1], m_s)), with
 * m_s = min(counts[s][AF_CNT_TICKS], tick_capacity); rows at or past m_s and the padding words of a row are never read.  Groups
 * as in af_pooled_t, AF_POOL_SKIP for a scenario left out.
 * Outputs per (g, w) and per (g, w, c):
 *     count  u32 [G][W]      the rows in the cell
 *     mean   f64 [G][W][C]   integer combination: the exact integer sum S of v over the cell (64 bits), then (double)S /
 *                            (double)count, the conversion rounded to nearest even.  ram combination: the f64 sum of the v in
 *                            the fixed order af_series_windows_t documents for a ram_in_use mean (within a scenario's window a
 *                            lane's rows top down -- lane l of 64 takes rows l, l + 64, ... of the window --, then a fixed tree
 *                            over the lanes; across the members ascending scenario index) with the rounding errors of the
 *                            additions carried along and added back once (a compensated sum), divided once: bit-equal to
 *                            fsum(v) / count whenever every partial sum is exact, otherwise within (count - 1) * 2^-53
 *                            relative of it
 *     minv, maxv  f64 [G][W][C]   the smallest / largest x of the cell in the same total order
 *     above  u32 [G][W][C]   the rows with x > thresholds[c], compared as f64 (NULL thresholds: 0.0 each)
 *     hist   u32 [G][W][C][n_bins], under, over u32 [G][W][C]   optional: n_bins == 0 with all three NULL skips them.  The bin
 *                            of x follows af_series_histogram_t's rule bit for bit with lo[c], width[c] per combination (NULL,
 *                            both: 0.0 and 1.0), and under + sum(hist) + over == count; n_bins <= AF_MAX_SERIES_HISTOGRAM_BINS
 * An empty cell has count 0, mean, minv and maxv NaN and every integer output 0.  A NULL count, minv, maxv, above, under or
 * over skips that output.
 * Determinism: every integer output is combined with integer +, min and max only (integer atomics on zeroed outputs for the
 * histogram); nothing depends on the launch, the batch a scenario sits in, the other combinations of the call, or the run.
 * Refused, no output buffer touched: n_combos == 0 or above the cap, an unknown op, an empty, unsorted, duplicate or
 * out-of-range column list, a list that mixes ram_in_use with integer series, a NaN threshold, the binning refusals of
 * af_series_histogram_t -- n_bins above the cap, a width that is <= 0, NaN or infinite, a lo that is NaN or infinite, exactly
 * one of lo / width NULL --, hist, under or over given with n_bins == 0 or n_bins > 0 without hist, tick_edges NULL or not strictly
 * increasing or n_windows == 0, a group id >= n_groups, outputs.samples, outputs.counts or mean NULL (AF_ERR_INVALID); a cell
 * of 2^32 or more rows, the longest column list times the rows of a cell at or above 2^32 (below that the 64-bit sums cannot
 * overflow), n_groups * n_windows >= 2^32 - 1, tick_capacity >= 2^31 (AF_ERR_CAPACITY); a planning-only engine
 * (AF_ERR_NO_DEVICE).  `out` needs samples, tick_capacity and counts; clock is not read.
 * Scratch kept by the engine (shared with the other analyzers): 4 B per edge + 40 B per combination + 4 B per listed column +
 * 4 B per group + 4 B per scenario + 2 560 B of alignment, and -- unless every group holds at most one scenario -- 36 B per
 * (scenario, window, combination).  Synchronous; the struct is written back. */
#define AF_MAX_SERIES_COMBINATIONS 64
enum { AF_COMBINE_SUM = 0, AF_COMBINE_MIN = 1, AF_COMBINE_MAX = 2, AF_COMBINE_SPREAD = 3 };
typedef struct af_series_combined {
    uint32_t n_scenarios;
    uint32_t n_groups;
    uint32_t n_windows;
    const uint32_t* group;       /* DEVICE [n_scenarios] group id per scenario (AF_POOL_SKIP: left out); NULL: all in group 0 */
    const uint32_t* tick_edges;  /* HOST [n_windows + 1] strictly increasing */
    uint32_t n_combos;           /* 1 .. AF_MAX_SERIES_COMBINATIONS */
    const uint32_t* op;          /* HOST [n_combos] AF_COMBINE_* */
    const uint32_t* col_start;   /* HOST [n_combos + 1] offsets into cols, col_start[0] == 0 */
    const uint32_t* cols;        /* HOST [col_start[n_combos]] series indices, strictly increasing within a combination */
    const double* thresholds;    /* HOST [n_combos] or NULL (0.0 each) */
    uint32_t n_bins;             /* 0 (no histogram) .. AF_MAX_SERIES_HISTOGRAM_BINS */
    const double* lo;            /* HOST [n_combos] finite; NULL (with width): 0.0 each */
    const double* width;         /* HOST [n_combos] finite and > 0; NULL (with lo): 1.0 each */
    uint32_t* count;             /* DEVICE [n_groups][n_windows]; NULL skips */
    double* mean;                /* DEVICE [n_groups][n_windows][n_combos] f64 */
    double* minv;                /* DEVICE, same shape, f64; NULL skips */
    double* maxv;                /* DEVICE, same shape, f64; NULL skips */
    uint32_t* above;             /* DEVICE, same shape, u32; NULL skips */
    uint32_t* hist;              /* DEVICE [n_groups][n_windows][n_combos][n_bins]; NULL with n_bins == 0 */
    uint32_t* under;             /* DEVICE [n_groups][n_windows][n_combos]; NULL skips */
    uint32_t* over;              /* DEVICE [n_groups][n_windows][n_combos]; NULL skips */
    double elapsed_ms;           /* out: wall time of the call */
    uint64_t scratch_bytes;      /* out: size of the engine's scratch after the call */
} af_series_combined_t;
int af_engine_summarize_series_combined(af_engine_t* engine, const af_outputs_t* out, af_series_combined_t* series_combined);

/* JOINT MOMENTS OF PAIRS OF THE SAMPLED SERIES per window of ticks and group on the device
 * (asyncflow_amd/csrc/af_series_joint.hpp): do the servers' queues rise together or in turn (covariance, correlation), does an
 * edge's concurrency lead a server's queue and by how many ticks (cross-correlation at a lag), how many independent samples
 * does a time average hold (the autocorrelation function and the integrated autocorrelation time).  Every one of these is a
 * closed form of SIX EXACT INTEGER SUMS per (pair, cell); the call returns the sums.
 * A PAIR p is (a[p], b[p], lag[p]): a and b are series indices < af_series_count, both INTEGER series -- a ram_in_use column
 * (index n_edges + 3 * server + 2) is refused in this version: second moments of floats need a rounding contract of their own
 * --; a == b is allowed (the autocorrelation); pairs are ordered, (a, b, l) and (b, a, l) differ for l > 0; 0 <= lag < 2^31.
 * At most AF_MAX_SERIES_PAIRS a call.
 * Cells: those of af_series_windows_t, with its group / AF_POOL_SKIP rules, its tick_edges and m_s = min(counts[s]
 * [AF_CNT_TICKS], tick_capacity).  Window w of scenario s is its rows [r0, r1) = [min(b[w], m_s), min(b[w + 1], m_s)).  The
 * sample of pair p in that window is (x, y) = (word a of row k, word b of row k + lag) for k in [r0, r1 - lag), the words as
 * unsigned 32-bit integers: both rows lie inside the same window of the same scenario.  A pair of rows that straddles a window
 * edge or reaches past m_s is in no cell.  Rows at or past m_s and the padding words of a row are never read.
 * Outputs per (g, w, p), over the windows of the members of g, all exact integers:
 *     n             u32 [G][W][P]      the (x, y) samples
 *     sx, sy        u64 [G][W][P]      sum x, sum y
 *     sxx, syy, sxy u64 [G][W][P][2]   sum x * x, sum y * y, sum x * y as 128-bit sums, low word first: the low word is the
 *                                      sum mod 2^64, the high word the carries out of it.  A cell holds < 2^32 samples of
 *                                      products < 2^64, so the high word stays below 2^32
 * A NULL sx, sy, sxx or syy skips that output; n and sxy are required.  An empty cell is all zeros.
 * Determinism: the outputs are combined with integer + only (no atomics, no floating point): they depend on the data alone, not
 * on the launch, the batch a scenario sits in, the other pairs of the call, or the run.
 * Refused, no output word touched: n_pairs == 0 or above the cap, a, b or lag NULL, a column >= af_series_count or a ram_in_use
 * column, a lag >= 2^31, tick_edges NULL or not strictly increasing or n_windows == 0, a group id >= n_groups,
 * outputs.samples or outputs.counts NULL, n or sxy NULL (AF_ERR_INVALID); a cell of 2^32 or more rows, n_groups * n_windows >=
 * 2^32 - 1, tick_capacity >= 2^31 (AF_ERR_CAPACITY); a planning-only engine (AF_ERR_NO_DEVICE).  `out` needs samples,
 * tick_capacity and counts; clock is not read.
 * Scratch kept by the engine (shared with the other analyzers): 4 B per edge + 16 B per pair + 4 B per group + 4 B per scenario
 * + 1 536 B of alignment, and -- unless every group holds at most one scenario -- 52 B per (scenario, window, pair).
 * Synchronous; the struct is written back. */
#define AF_MAX_SERIES_PAIRS 64
typedef struct af_series_joint {
    uint32_t n_scenarios;
    uint32_t n_groups;
    uint32_t n_windows;
    const uint32_t* group;       /* DEVICE [n_scenarios] group id per scenario (AF_POOL_SKIP: left out); NULL: all in group 0 */
    const uint32_t* tick_edges;  /* HOST [n_windows + 1] strictly increasing */
    uint32_t n_pairs;            /* 1 .. AF_MAX_SERIES_PAIRS */
    const uint32_t* a;           /* HOST [n_pairs] the series of x: an integer series < af_series_count */
    const uint32_t* b;           /* HOST [n_pairs] the series of y, likewise */
    const uint32_t* lag;         /* HOST [n_pairs] ticks between the row of x and the row of y, < 2^31 */
    uint32_t* n;                 /* DEVICE [n_groups][n_windows][n_pairs] u32 */
    uint64_t* sx;                /* DEVICE, same shape, u64; NULL skips */
    uint64_t* sy;                /* DEVICE, same shape, u64; NULL skips */
    uint64_t* sxx;               /* DEVICE [n_groups][n_windows][n_pairs][2] u64, low word first; NULL skips */
    uint64_t* syy;               /* DEVICE, same shape; NULL skips */
    uint64_t* sxy;               /* DEVICE, same shape */
    double elapsed_ms;           /* out: wall time of the call */
    uint64_t scratch_bytes;      /* out: size of the engine's scratch after the call */
} af_series_joint_t;
int af_engine_summarize_series_joint(af_engine_t* engine, const af_outputs_t* out, af_series_joint_t* series_joint);

/* WARM-UP TRUNCATION OF THE SAMPLED SERIES per window of ticks and group on the device
 * (asyncflow_amd/csrc/af_series_warmup.hpp): every sweep starts from an empty system, and every statistic of a window averages
 * that transient in.  The initial-transient rule MSER (White 1997; MSER-5 with batch = 5) says where the steady regime begins,
 * applied in pooled form to the batch sums of the ensemble over a group's members (Welch), and stated entirely in integers.
 * Cells: (g, w, c) = those of af_series_windows_t, with its group / AF_POOL_SKIP rules, its tick_edges and m_s = min(counts[s]
 * [AF_CNT_TICKS], tick_capacity); series columns[c] must be an INTEGER series -- a ram_in_use column (index n_edges + 3 * server
 * + 2) is refused as in af_series_joint_t: second moments of floats need a rounding contract of their own.  Any order of the
 * columns, duplicates allowed, at most AF_MAX_SERIES_WARMUP_COLUMNS a call.
 * With B = batch >= 1 ticks: member s has the rows [r0, r1) = [min(b[w], m_s), min(b[w + 1], m_s)) of window w; its batch j is
 * the rows [b[w] + j B, b[w] + (j + 1) B), complete when inside [r0, r1).  J = the minimum over the members of g of their
 * complete batches -- the same for every column; 0 for a group without a member or with a member that stored no row of the
 * window: one short member shortens the cell for all (`batches` shows it; leave a broken replica out with AF_POOL_SKIP).  A
 * trailing partial batch is in no cell.  For j < J
 *     Y_j = the sum over the members and the B rows of batch j of the word as an unsigned 32-bit integer
 *     S1(d) = sum_{j >= d} Y_j,  S2(d) = sum_{j >= d} Y_j^2,  m = J - d,  A(d) = m S2(d) - S1(d)^2 >= 0,  MSER(d) = A(d) / m^3
 *     d* = the smallest d in 0 .. J / 2 that minimises MSER(d), compared exactly by A(d1) m2^3 < A(d2) m1^3; J = 0: d* = 0.
 * Width contract, checked statically: n_scenarios * B <= 2^32 (Y_j < 2^64) and every window holds fewer than 2^25 batches.
 * Then S1 < 2^89, S2 < 2^153, A < 2^178, m^3 < 2^75 and every compared product is below 2^253: 256-bit arithmetic is exact.
 * Outputs, all exact integers:
 *     batches         u32 [G][W]         J
 *     trunc           u32 [G][W][C]      d*: the steady regime of the window starts at tick b[w] + d* B
 *     s1, s1_all      u64 [G][W][C][2]   S1(d*) and S1(0), low word first
 *     s2, s2_all      u64 [G][W][C][3]   S2(d*) and S2(0), low word first
 * A NULL s1, s2, s1_all or s2_all skips that output; batches and trunc are required.  A cell with J = 0 is all zeros.
 * Determinism: integer additions and an integer minimum only (64-bit integer atomics into a zeroed buffer, no floating point):
 * the outputs depend on the data alone, not on the launch, the batch a scenario sits in, the other columns of the call, or the
 * run.
 * Refused, no output word touched: batch == 0, n_columns == 0 or above the cap, columns NULL, a column >= af_series_count or a
 * ram_in_use column, tick_edges NULL or not strictly increasing or n_windows == 0, a group id >= n_groups, outputs.samples or
 * outputs.counts NULL, batches or trunc NULL (AF_ERR_INVALID); n_scenarios * batch > 2^32, a window of 2^25 or more batches,
 * n_groups * n_windows >= 2^32 - 1, tick_capacity >= 2^31 (AF_ERR_CAPACITY); a planning-only engine (AF_ERR_NO_DEVICE).  `out`
 * needs samples, tick_capacity and counts; clock is not read.
 * Scratch kept by the engine (shared with the other analyzers): 8 B per (group, column, batch) -- batch over sum_w floor((min(
 * b[w + 1], tick_capacity) - min(b[w], tick_capacity)) / B) --, 4 B per (group, window), 8 B per edge, 4 B per column + 1 280 B
 * of alignment.
 * Synchronous; the struct is written back. */
#define AF_MAX_SERIES_WARMUP_COLUMNS 64
typedef struct af_series_warmup {
    uint32_t n_scenarios;
    uint32_t n_groups;
    uint32_t n_windows;
    const uint32_t* group;       /* DEVICE [n_scenarios] group id per scenario (AF_POOL_SKIP: left out); NULL: all in group 0 */
    const uint32_t* tick_edges;  /* HOST [n_windows + 1] strictly increasing */
    uint32_t n_columns;          /* 1 .. AF_MAX_SERIES_WARMUP_COLUMNS */
    const uint32_t* columns;     /* HOST [n_columns] integer series < af_series_count; any order, duplicates allowed */
    uint32_t batch;              /* B >= 1 ticks a batch (MSER-5: 5) */
    uint32_t* batches;           /* DEVICE [n_groups][n_windows] u32 */
    uint32_t* trunc;             /* DEVICE [n_groups][n_windows][n_columns] u32 */
    uint64_t* s1;                /* DEVICE [n_groups][n_windows][n_columns][2] u64, low word first; NULL skips */
    uint64_t* s2;                /* DEVICE [n_groups][n_windows][n_columns][3] u64, low word first; NULL skips */
    uint64_t* s1_all;            /* DEVICE, the shape of s1; NULL skips */
    uint64_t* s2_all;            /* DEVICE, the shape of s2; NULL skips */
    double elapsed_ms;           /* out: wall time of the call */
    uint64_t scratch_bytes;      /* out: size of the engine's scratch after the call */
} af_series_warmup_t;
int af_engine_summarize_series_warmup(af_engine_t* engine, const af_outputs_t* out, af_series_warmup_t* series_warmup);

/* Arbitrary latency QUANTILES and SLO counts per group and time window on the device (asyncflow_amd/csrc/af_quantiles.hpp):
 * p99.9 at a grid point, p90 during an outage, how many requests met a 200 ms objective in every 10 s window.  The cells and
 * their samples are af_windows_t's: cell c = g * n_windows + w holds, in ascending scenario index over the members of g,
 * finish - start over the rows with edges[w] < finish <= edges[w + 1]; the same completion-order check, AF_ERR_INVALID naming
 * the scenario, nothing written.  With n_windows == 0 and edges == NULL there is ONE cell per group over all stored rows of
 * its members (af_pooled_t's sample); completion order is then neither needed nor checked.  C = n_groups * max(n_windows, 1).
 * For a cell of n >= 1 latencies x[0] <= ... <= x[n-1] and a level q in [0, 1]:
 *     v = (double)(n - 1) * q;  lo = floor(v);  hi = min(lo + 1, n - 1);  t = v - lo;  d = x[hi] - x[lo];
 *     quantile = t >= 0.5 ? x[hi] - d * (1 - t) : x[lo] + d * t
 * which is np.quantile(a, q) (method 'linear') bit for bit.  Level 0.5 is therefore np.quantile(a, 0.5), which is NOT always
 * the `median` column of the other analyzers bit for bit (np.median is the mean of the middle pair: about one sample in 280
 * differs in the last digit); levels 0.95 and 0.99 DO equal their p95 / p99 columns, levels 0 and 1 their min / max.
 * within[c][i] = #{ x <= thresholds[i] }, compared as f64: an exact integer.  An empty cell: count 0, every quantile NaN,
 * every within 0.  Column i of an output belongs to levels[i] / thresholds[i]; any order, duplicates allowed.  A cell's
 * result does not depend on which other cells, levels or thresholds the call holds, and is identical from run to run
 * (selection by sorting / counting, integer atomics only).
 * Refused: a level that is NaN or outside [0, 1], a NaN threshold (+-inf is fine), n_levels == 0 together with
 * n_thresholds == 0, more than AF_MAX_QUANTILE_LEVELS levels or AF_MAX_SLO_THRESHOLDS thresholds, edges not strictly
 * increasing or not finite, a group id >= n_groups, an inversion of completion order in windowed mode (AF_ERR_INVALID); a
 * cell of 2^32 or more latencies, C >= 2^32 - 1 (AF_ERR_CAPACITY); a planning-only engine (AF_ERR_NO_DEVICE).
 * Scratch kept by the engine (shared with the other group analyzers): 8 B per latency in a cell + 4 B per (scenario, edge)
 * + 4 B per (scenario, window) + 12 B per cell + 8 B per scenario + 8 B per edge + 1 KB (levels, thresholds) + 4 KB of
 * alignment, and for every cell of more than 8 192 latencies only: 4 B per threshold + ceil(n_levels / 3) * 58 KB +
 * (1 + ceil(n_levels / 3)) * 16 B per 131 072 latencies.  Synchronous; the struct is written back. */
#define AF_MAX_QUANTILE_LEVELS 64
#define AF_MAX_SLO_THRESHOLDS 64
typedef struct af_quantiles {
    uint32_t n_scenarios;
    uint32_t n_groups;
    uint32_t n_windows;        /* 0 (with edges NULL): one cell per group over the whole run */
    const uint32_t* group;     /* DEVICE [n_scenarios] group id per scenario (AF_POOL_SKIP: left out); NULL: all in group 0 */
    const double* edges;       /* HOST [n_windows + 1] strictly increasing, finite; NULL with n_windows == 0 */
    uint32_t n_levels;
    const double* levels;      /* HOST [n_levels] in [0, 1] */
    uint32_t n_thresholds;
    const double* thresholds;  /* HOST [n_thresholds] seconds, not NaN; may be NULL with n_thresholds == 0 */
    uint32_t* count;           /* DEVICE [C] u32; NULL skips */
    double* quantiles;         /* DEVICE [C][n_levels] f64; NULL skips */
    uint32_t* within;          /* DEVICE [C][n_thresholds] u32; NULL skips */
    double elapsed_ms;         /* out: wall time of the call */
    uint64_t scratch_bytes;    /* out: size of the engine's scratch after the call */
} af_quantiles_t;
int af_engine_summarize_quantiles(af_engine_t* engine, const af_outputs_t* out, af_quantiles_t* quantiles);

/* The same quantiles and SLO counts with windows by ARRIVAL time: the cells and their samples are
 * af_engine_summarize_arrival_windows's (edges[w] < start <= edges[w + 1], rows in stored order, right-censored cohorts: count
 * is the cohort's completions).  n_windows > 0 is required (a whole run has no window: AF_ERR_INVALID); completion order is
 * neither needed nor checked.  Everything else as af_engine_summarize_quantiles. */
int af_engine_summarize_arrival_quantiles(af_engine_t* engine, const af_outputs_t* out, af_quantiles_t* quantiles);

/* CELLS ACROSS DEVICES (asyncflow_amd/csrc/af_cells.hpp): the cells of af_windows_t / af_quantiles_t when the members of a
 * group ran on several devices.  Every device EXPORTS the latencies of its scenarios that fall into the windows -- 8 B each,
 * instead of its [n][clock_capacity][2] clock buffer -- and the reducing device merges the exports into the very array the
 * one-device call compacts, element for element, and runs the same reduction on it: every output word equals that call's.
 *
 * af_engine_export_cells: scenario s is one SEGMENT of lat.  With n_windows > 0 and edges as in af_windows_t, seg_bounds[s][k]
 * is r_s[k] (by_arrival == 0; the same completion-order check and AF_ERR_INVALID) or c_s[k] (by_arrival != 0), also for a
 * skipped scenario; with n_windows == 0 (edges NULL, by_arrival 0) there is one window over every stored row:
 * seg_bounds[s] = {0, m_s}.  Wc = max(n_windows, 1).  The segments follow one another in scenario order: segment s begins at
 * seg_begin[s] = the sum of seg_bounds[t][Wc] - seg_bounds[t][0] over the scenarios t < s that are not skipped
 * (group[t] != AF_POOL_SKIP; the other ids are not looked at), and holds finish - start of window 0's rows in row order, then
 * window 1's, ...: (s, w) starts at seg_begin[s] + seg_bounds[s][w] - seg_bounds[s][0].  lat_count = the elements written.
 * lat_capacity below that: AF_ERR_CAPACITY, nothing written (the sum of min(counts[AF_CNT_COMPLETED], clock_capacity) always
 * suffices).  seg_bounds is written only by a call that succeeds.  Scratch: 4 B per scenario + af_windows_t's without the
 * latencies, with a cell per (scenario, window). */
typedef struct af_cells_export {
    uint32_t n_scenarios;
    uint32_t n_windows;      /* 0 (with edges NULL): the whole run */
    uint32_t by_arrival;     /* 0: windows by finish time; otherwise by arrival time (needs n_windows > 0) */
    const uint32_t* group;   /* DEVICE [n_scenarios] or NULL: AF_POOL_SKIP exports nothing for the scenario */
    const double* edges;     /* HOST [n_windows + 1] strictly increasing, finite; NULL with n_windows == 0 */
    double* lat;             /* DEVICE [lat_capacity] f64 out, the caller's */
    uint64_t lat_capacity;   /* elements */
    uint32_t* seg_bounds;    /* DEVICE [n_scenarios][Wc + 1] u32 out */
    uint64_t lat_count;      /* out: elements of lat written */
    double elapsed_ms;       /* out: wall time of the call */
    uint64_t scratch_bytes;  /* out: size of the engine's scratch after the call */
} af_cells_export_t;
int af_engine_export_cells(af_engine_t* engine, const af_outputs_t* out, af_cells_export_t* cells_export);

/* af_engine_import_cells: n_scenarios members in the order the cells concatenate them (the order of the whole sweep), each
 * with its group id, its bounds (as exported) and the place seg_begin[s] of its segment in lat -- the exports of several
 * devices simply one after the other, in any order.  Cell c = g * Wc + w is the concatenation over the members of g, in
 * member order, of the members' window w.  stats is af_windows_t's ([n_groups][Wc][8]); count / quantiles / within with levels
 * and thresholds are af_quantiles_t's; every output is optional, at least one is needed, one merge serves all.
 * Refused with no output word written: a group id >= n_groups, bounds that decrease, a segment that ends past n_lat, two
 * segments (of members that are not skipped) that overlap, af_quantiles_t's rules for levels and thresholds (AF_ERR_INVALID);
 * a cell of 2^32 or more latencies, n_groups * Wc >= 2^32 - 1, n_scenarios * (Wc + 1) > 2^32 (AF_ERR_CAPACITY).
 * Scratch kept by the engine: 8 B per latency in a cell (the merged cells, beside the caller's 8 B per imported latency) +
 * 8 B per (scenario, edge) + 12 B per scenario + the per-cell parts of af_windows_t and af_quantiles_t.  Synchronous. */
typedef struct af_cells {
    uint32_t n_scenarios;
    uint32_t n_groups;
    uint32_t n_windows;          /* 0: one cell per group (Wc = 1) */
    const uint32_t* group;       /* HOST [n_scenarios] group id per member (AF_POOL_SKIP: left out); NULL: all in group 0 */
    const uint32_t* seg_bounds;  /* HOST [n_scenarios][Wc + 1] */
    const uint64_t* seg_begin;   /* HOST [n_scenarios] first element of the member's segment in lat */
    const double* lat;           /* DEVICE [n_lat] f64, on the engine's device */
    uint64_t n_lat;
    double* stats;               /* DEVICE [n_groups][Wc][8] f64; NULL skips */
    uint32_t n_levels;
    const double* levels;        /* HOST [n_levels] in [0, 1] */
    uint32_t n_thresholds;
    const double* thresholds;    /* HOST [n_thresholds] seconds, not NaN */
    uint32_t* count;             /* DEVICE [C] u32; NULL skips */
    double* quantiles;           /* DEVICE [C][n_levels] f64; NULL skips */
    uint32_t* within;            /* DEVICE [C][n_thresholds] u32; NULL skips */
    double elapsed_ms;           /* out: wall time of the call */
    uint64_t scratch_bytes;      /* out: size of the engine's scratch after the call */
} af_cells_t;
int af_engine_import_cells(af_engine_t* engine, af_cells_t* cells);

/* ARRIVALS per window and group (asyncflow_amd/csrc/af_arrival_counts.hpp): the offered load, and the denominator the
 * by-arrival cohorts above lack -- their count is the cohort's completions; a request that was dropped or was still in flight
 * when the run ended is in no rqs_clock row.  Arrival times are a pure function of the seed and the generator's parameters;
 * the engine works them out on the device before every run and this call does the same, WITHOUT a run: no simulation
 * kernel is launched and no af_outputs_t is read.
 * `sweep` is what af_engine_run takes; draw_capacity must be > 0 here (pass the run's value -- its clock_capacity where the
 * run passed 0 -- so that the arrivals counted are exactly the ones simulated).  Let a_s[0 .. m_s) be the arrival times of
 * scenario s: those of the sequential sampler (samplers/poisson_poisson.py:51-82, gaussian_poisson.py:63-94, summed on the
 * simulation clock as rqs_generator.py:97-119 does) under seeds[s], the plan's generator parameters and the scenario's
 * AF_PARAM_GEN_USERS_MEAN / _SIGMA / AF_PARAM_GEN_RPM_MEAN / AF_PARAM_GEN_WINDOW columns, cut at draw_capacity (m_s <=
 * draw_capacity; other columns are checked like a run checks them and otherwise ignored).  With edges[0] < ... <
 * edges[n_windows] (finite seconds):
 *     row_bounds[s][k] = #{ i < m_s : a_s[i] <= edges[k] }      np.searchsorted(a_s, edges, side="right")
 *     window w of s    = row_bounds[s][w + 1] - row_bounds[s][w] arrivals: edges[w] < t <= edges[w + 1], the bucket rule of
 *                        the by-arrival latency windows (an arrival on an edge belongs to the window that ends there)
 *     arrivals[g][w]   = the sum over the members of g;  generated[s] = m_s, which a run reports as counts[s][AF_CNT_GENERATED]
 *     flags[s]         = AF_FLAG_DRAW_OVERFLOW where the sampler had a further arrival when the row was full, else 0
 * Every output word is an exact integer (binary searches, integer atomics on zeroed outputs): the result does not depend on
 * the launch, on the pre-generation kernel (AF_PREGEN_MODE, chosen as a run chooses it) or on the chunks.
 * group: af_pooled_t's rule -- AF_POOL_SKIP leaves a scenario out of arrivals; its row_bounds / generated / flags are still
 * written --, except that NULL means SINGLETONS here -- scenario s is group s, and n_groups must be n_scenarios.
 * times / times_given:
 *     times NULL                  the engine generates into its own scratch, in chunks sized by the memory budget of a run
 *                                 (af_engine_options_t.draw_memory_mb), 8 B per scenario and draw;
 *     times set, times_given 0    the engine generates into the caller's buffer (all scenarios at once), which the caller keeps:
 *                                 a_s with +inf behind the last arrival, bit-equal to what the run consumed;
 *     times set, times_given 1    the rows are READ and nothing is generated: they must be ascending with +inf behind the last
 *                                 arrival (not checked: rows that are not give meaningless counts, nothing worse); seeds and
 *                                 overrides of the sweep are ignored (seeds may be NULL), flags are 0.  For traces and tests.
 * Refused, no output touched: n_scenarios == 0 or != sweep->n_scenarios, n_windows == 0, draw_capacity == 0, arrivals NULL,
 * edges NULL / not finite / not strictly increasing, a group id >= n_groups, group NULL with n_groups != n_scenarios, a bad
 * override, seeds NULL unless times_given (AF_ERR_INVALID); n_groups * n_windows >= 2^32 - 1, n_windows >= 2^24, a single
 * scenario's row that does not fit the memory budget (AF_ERR_CAPACITY); a planning-only engine (AF_ERR_NO_DEVICE).
 * Scratch kept by the engine: 8 B per edge and, without row_bounds, 4 B per (scenario of a chunk, edge), shared with the
 * other analyzers; without times, the run's own arrival buffer.  Synchronous; the struct is written back. */
typedef struct af_arrivals {
    uint32_t n_scenarios;    /* = sweep->n_scenarios */
    uint32_t n_groups;
    uint32_t n_windows;
    const uint32_t* group;   /* DEVICE [n_scenarios] group id per scenario (AF_POOL_SKIP: left out); NULL: scenario s is group s */
    const double* edges;     /* HOST [n_windows + 1] strictly increasing, finite */
    double* times;           /* DEVICE [n_scenarios][draw_capacity] f64, optional (see above) */
    uint32_t times_given;    /* 1: times holds the rows to count; 0: times, if set, receives the generated rows */
    uint64_t* arrivals;      /* DEVICE [n_groups][n_windows] u64 out */
    uint32_t* row_bounds;    /* DEVICE [n_scenarios][n_windows + 1] u32 out, optional */
    uint32_t* generated;     /* DEVICE [n_scenarios] u32 out, optional */
    uint32_t* flags;         /* DEVICE [n_scenarios] u32 out, optional */
    double elapsed_ms;       /* out: wall time of the call */
    uint64_t scratch_bytes;  /* out: size of the engine's scratch after the call */
} af_arrivals_t;
int af_engine_summarize_arrivals(af_engine_t* engine, const af_sweep_t* sweep, af_arrivals_t* arrivals);

/* Requests IN FLIGHT end to end per tick, window of ticks and group, from the clock rows (asyncflow_amd/csrc/af_inflight.hpp):
 * L of Little's law beside the arrivals per window (lambda, above) and the by-arrival latency windows (W).  No sampled series
 * or combination of them holds it: a request in a server's CPU step or between two hops is in none of them.  Reads
 * outputs.clock and outputs.counts only; no simulation kernel runs.
 * Per scenario s: m_s = min(counts[s][AF_CNT_COMPLETED], clock_capacity) stored rows (start_i, finish_i), t_s =
 * min(counts[s][AF_CNT_TICKS], tick_capacity) sample rows, p = sample_period.
 *     tick of a time   q(t) = floor(t / p): one f64 division rounded to nearest, then floor -- the rule af_state_bins_t uses
 *                      for `start`;  a_i = q(start_i), f_i = q(finish_i)
 *     rows counted     sample row k is taken at (k + 1) p (af_series_windows_t): request i is counted in the rows
 *                      a_i <= k < f_i, clipped to [0, t_s) -- the samples taken strictly after its start and at or before its
 *                      finish, as the quotient sees them; the row a request "met on arrival" (q - 1 of af_state_bins_t) does not
 *                      contain it, the next one does
 *     counted nowhere  start or finish NaN; start < 0; f_i <= a_i (a request that lived between two samples, or a negative-delay
 *                      residue with finish < start); a_i >= t_s.  The comparisons with t_s are made on the f64 quotients before
 *                      any conversion to an integer: a huge finish / p clips, it does not wrap
 *     started[s][k]    = #{ counted i : max(a_i, 0) == k }
 *     finished[s][k]   = #{ counted i : f_i == k }; a counted row with f_i >= t_s is in none: still in flight at the last sample
 *     in_flight[s][k]  = #{ counted i : a_i <= k < f_i } = the running sum of started - finished, finished[s][k] taken before
 *                      row k is read;  all three u32
 * Windows and groups: af_series_windows_t's -- tick_edges on tick indices, group / AF_POOL_SKIP, a cell of 2^32 or more values
 * refused.  Cell (g, w) holds the values in_flight[s][k] of the members s of g, min(b[w], t_s) <= k < min(b[w + 1], t_s):
 *     count u32, sum u64, minv / maxv u32, above u32 = the values > threshold;  with hist: hist[b] = the values == lo + b, the
 *     LAST bin taking everything above it, under = the values < lo;  an empty cell: count 0 and every other output 0.
 * in_flight / started / finished: optional DEVICE [n_scenarios][tick_capacity]; rows k < t_s are written, rows at or past t_s are
 * left untouched; written for skipped scenarios too (as row_bounds elsewhere).
 * COMPLETED REQUESTS ONLY: a dropped request, and a request still in flight when the run ended, is in no row, so the last
 * seconds of a run under-count as the by-arrival cohorts do -- `lost` of the arrivals call sizes the under-count.
 * Integer add / min / max atomics on initialised outputs only: every word is identical from run to run and does not depend on
 * the batch a scenario sits in.
 * Refused, no output touched: n_scenarios, n_groups or n_windows == 0, tick_edges NULL or not strictly increasing, a
 * sample_period that is <= 0, NaN or infinite, a group id >= n_groups, outputs.clock or outputs.counts NULL, clock_capacity or
 * tick_capacity == 0, count or sum NULL, with hist n_bins == 0 or above AF_MAX_SERIES_HISTOGRAM_BINS, under without hist
 * (AF_ERR_INVALID); n_groups * n_windows >= 2^32 - 1, tick_capacity >= 2^31, a cell of 2^32 or more values (AF_ERR_CAPACITY);
 * a planning-only engine (AF_ERR_NO_DEVICE).
 * outputs.clock must be 16-byte aligned: a row is read as one (start, finish) pair by a 16-byte load (any device allocation is).
 * Scratch kept by the engine: 4 B per edge, shared with the other analyzers.  Synchronous; the struct is written back. */
typedef struct af_inflight {
    uint32_t n_scenarios;
    uint32_t n_groups;
    uint32_t n_windows;
    const uint32_t* group;       /* DEVICE [n_scenarios] group id per scenario (AF_POOL_SKIP: left out); NULL: all in group 0 */
    const uint32_t* tick_edges;  /* HOST [n_windows + 1] strictly increasing tick indices */
    double sample_period;        /* p: seconds per tick, > 0 and finite */
    uint32_t threshold;          /* above counts the values > threshold */
    uint32_t n_bins;             /* with hist: 1 .. AF_MAX_SERIES_HISTOGRAM_BINS; ignored without */
    uint32_t lo;                 /* the value of bin 0 */
    uint32_t* count;             /* DEVICE [n_groups][n_windows] u32 out */
    uint64_t* sum;               /* DEVICE [n_groups][n_windows] u64 out */
    uint32_t* minv;              /* DEVICE [n_groups][n_windows] u32 out, optional */
    uint32_t* maxv;              /* DEVICE [n_groups][n_windows] u32 out, optional */
    uint32_t* above;             /* DEVICE [n_groups][n_windows] u32 out, optional */
    uint32_t* hist;              /* DEVICE [n_groups][n_windows][n_bins] u32 out, optional */
    uint32_t* under;             /* DEVICE [n_groups][n_windows] u32 out, optional, with hist only */
    uint32_t* in_flight;         /* DEVICE [n_scenarios][tick_capacity] u32 out, optional */
    uint32_t* started;           /* DEVICE [n_scenarios][tick_capacity] u32 out, optional */
    uint32_t* finished;          /* DEVICE [n_scenarios][tick_capacity] u32 out, optional */
    double elapsed_ms;           /* out: wall time of the call */
    uint64_t scratch_bytes;      /* out: size of the engine's scratch after the call */
} af_inflight_t;
int af_engine_summarize_inflight(af_engine_t* engine, const af_outputs_t* out, af_inflight_t* inflight);

/* The k SLOWEST REQUESTS per window and group WITH THEIR IDENTITY (asyncflow_amd/csrc/af_exemplars.hpp): the "exemplars" behind a
 * window's max or p99 -- which scenario, which row of its rqs_clock, when it was sent and what the servers looked like then --
 * and the input of an extreme-value fit of the tail.  The other analyzers return values only.  Reads outputs.clock and
 * outputs.counts (with `state` also outputs.samples); no simulation kernel runs.
 * Per scenario s: m_s = min(counts[s][AF_CNT_COMPLETED], clock_capacity) stored rows (start_i, finish_i).
 *     latency          lat = finish - start, one f64 subtraction; a row whose latency is NaN is in no cell
 *     window           with edges: the bucket rule of af_windows_t on t = finish (by_arrival == 0) or t = start (by_arrival != 0):
 *                      window w where edges[w] < t <= edges[w + 1]; t <= edges[0], t > edges[W] or t NaN: in no cell.  A mask on
 *                      every row: completion order is neither needed nor checked, in both modes.  Without edges (n_windows == 0,
 *                      edges NULL) one window with no condition on time; by_arrival is then refused.  W' = max(n_windows, 1)
 *     order            within cell c = g * W' + w: larger latency first, compared as f64 values (-0.0 and +0.0 are equal, +inf is
 *                      a value like any other); ties by ascending scenario index, then ascending row index.  A total order: the
 *                      result does not depend on the algorithm, the launch or the batch a scenario sits in
 *     total[c]         u64: the rows of the cell;  kept[c] u32 = min(k, total[c])
 *     scenario, row    [c][j], j < kept[c]: the j-th place of the order;  clock[c][j] = the stored (start, finish) pair bit for bit
 *     behind kept      every byte of scenario, row, clock (and state) of the slots j >= kept[c] is 0xFF
 *     state[c][j]      optional: the n_series (af_series_count) raw words of sample row q - 1, q = floor(start / sample_period) --
 *                      af_state_bins_t's rule: one f64 division, then floor; ram_in_use words stay f32 bits.  No state, every word
 *                      0xFFFFFFFF: q < 1, q - 1 >= t_s = min(counts[s][AF_CNT_TICKS], tick_capacity), start NaN or negative.  Only
 *                      the n_series words of a row are read, never the padding of the pitch
 * An empty or skipped (AF_POOL_SKIP) group's cells: total = kept = 0.
 * Integer compares only, no atomics: every word is identical from run to run.
 * Refused, no output touched: n_scenarios or n_groups == 0, k outside 1 .. AF_MAX_EXEMPLARS, edges not finite or not strictly
 * increasing, edges NULL with n_windows > 0, by_arrival with n_windows == 0, a group id >= n_groups, outputs.clock or
 * outputs.counts NULL, clock_capacity == 0, total / scenario / row / clock NULL, state without outputs.samples or with a
 * sample_period that is <= 0, NaN or infinite (AF_ERR_INVALID); n_groups * W' * k or n_scenarios * W' * k >= 2^32
 * (AF_ERR_CAPACITY); a planning-only engine (AF_ERR_NO_DEVICE).
 * outputs.clock and exemplars.clock must be 16-byte aligned (any device allocation is): a pair moves as one 16-byte word.
 * Scratch kept by the engine, shared with the other analyzers: n_scenarios * W' * (12 k + 4) bytes (the per-(scenario, window)
 * lists and row counts), 8 more per (scenario, window) above 3 276 windows, 8 per edge, 4 per scenario and per group.
 * Synchronous; the struct is written back. */
#define AF_MAX_EXEMPLARS 64
typedef struct af_exemplars {
    uint32_t n_scenarios;
    uint32_t n_groups;
    uint32_t n_windows;          /* 0: one window over all time (edges NULL) */
    const uint32_t* group;       /* DEVICE [n_scenarios] group id per scenario (AF_POOL_SKIP: left out); NULL: all in group 0 */
    const double* edges;         /* HOST [n_windows + 1] strictly increasing, finite; NULL with n_windows == 0 */
    uint32_t by_arrival;         /* 0: windows by finish time; otherwise by start time (needs n_windows > 0) */
    uint32_t k;                  /* 1 .. AF_MAX_EXEMPLARS */
    double sample_period;        /* seconds per tick, > 0 and finite; used with state only */
    uint64_t* total;             /* DEVICE [C] u64 out, C = n_groups * W' */
    uint32_t* kept;              /* DEVICE [C] u32 out, optional */
    uint32_t* scenario;          /* DEVICE [C][k] u32 out */
    uint32_t* row;               /* DEVICE [C][k] u32 out */
    double* clock;               /* DEVICE [C][k][2] f64 out, 16-byte aligned */
    uint32_t* state;             /* DEVICE [C][k][af_series_count] u32 out, optional; needs outputs.samples */
    double elapsed_ms;           /* out: wall time of the call */
    uint64_t scratch_bytes;      /* out: size of the engine's scratch after the call */
} af_exemplars_t;
int af_engine_summarize_exemplars(af_engine_t* engine, const af_outputs_t* out, af_exemplars_t* exemplars);

/* Mergeable LOG-LINEAR LATENCY HISTOGRAMS per window and group (asyncflow_amd/csrc/af_latency_histogram.hpp): the distribution of
 * every cell instead of finished numbers about it -- a latency heatmap over time, two cells compared, quantile brackets at levels
 * chosen afterwards.  An HDR-style sketch whose binning is defined on the bit pattern of the f64 latency, counted with integer +
 * only: the results of two calls over the same cells add word by word (devices, member splits, saved sweeps), and windows or
 * groups coarsen by summing cells.  Reads outputs.clock and outputs.counts; no simulation kernel runs.
 * Per scenario s: m_s = min(counts[s][AF_CNT_COMPLETED], clock_capacity) stored rows (start_i, finish_i).
 *     binning          sub_bits m in 0 .. 8, min_exp e >= -1022, octaves o >= 1, e + o <= 1023, n_bins = o << m in
 *                      1 .. AF_MAX_LATENCY_HISTOGRAM_BINS: every octave [2^(e + k), 2^(e + k + 1)) holds 2^m bins of equal width,
 *                      the relative width of a bin is 2^-m.  m = 5, e = -20, o = 32: 1 024 bins from 2^-20 s to 2^12 s, 3.1 % wide
 *     latency          x = finish - start, one f64 subtraction; bits = its 64-bit pattern.  x NaN: counted in nan;  x < 2^e
 *                      (zeros, -0.0, negatives, denormals, -inf): in under;  x >= 2^(e + o) (+inf): in over;  otherwise in bin
 *                      (bits >> (52 - m)) - ((e + 1023) << m) -- integer arithmetic on the word.  Bin b covers [E[b], E[b + 1]),
 *                      E[b] = ldexp(1 + (b & (2^m - 1)) / 2^m, e + (b >> m)), exact in f64
 *     window           af_exemplars_t's rule, a mask on every row: with edges, window w where edges[w] < t <= edges[w + 1], t =
 *                      finish (by_arrival == 0) or start (by_arrival != 0); t <= edges[0], t > edges[W] or t NaN: in no cell.
 *                      Completion order is neither needed nor checked.  Without edges (n_windows == 0, edges NULL) one window with
 *                      no condition on time; by_arrival is then refused.  W' = max(n_windows, 1)
 *     cell c = g * W' + w   count[c] u64 = the rows of the cell; hist[c][n_bins], under[c], over[c], nan[c] u32;
 *                      under + over + nan + sum(hist[c]) == count[c]
 * An empty or skipped (AF_POOL_SKIP) group's cells are all zero.
 * The outputs are zeroed, then integer add atomics only: every word is identical from run to run and does not depend on the
 * launch or on the batch a scenario sits in.
 * Refused, no output touched: n_scenarios or n_groups == 0, a binning outside the ranges above, edges not finite or not strictly
 * increasing, edges NULL with n_windows > 0 (or given with n_windows == 0), by_arrival with n_windows == 0, a group id >=
 * n_groups, outputs.clock or outputs.counts NULL, clock_capacity == 0, count or hist NULL (AF_ERR_INVALID); n_groups * W' * n_bins
 * >= 2^32, a group whose members hold 2^32 or more stored rows together (AF_ERR_CAPACITY); a planning-only engine
 * (AF_ERR_NO_DEVICE).
 * outputs.clock must be 16-byte aligned: a row is read as one (start, finish) pair by a 16-byte load (any device allocation is).
 * Scratch kept by the engine, shared with the other analyzers: 8 B per edge; no per-row and no per-cell records.
 * Synchronous; the struct is written back. */
#define AF_MAX_LATENCY_HISTOGRAM_BINS 4096
typedef struct af_latency_histogram {
    uint32_t n_scenarios;
    uint32_t n_groups;
    uint32_t n_windows;          /* 0: one window over all time (edges NULL) */
    const uint32_t* group;       /* DEVICE [n_scenarios] group id per scenario (AF_POOL_SKIP: left out); NULL: all in group 0 */
    const double* edges;         /* HOST [n_windows + 1] strictly increasing, finite; NULL with n_windows == 0 */
    uint32_t by_arrival;         /* 0: windows by finish time; otherwise by start time (needs n_windows > 0) */
    uint32_t sub_bits;           /* m: 0 .. 8 */
    int32_t min_exp;             /* e: the first bin starts at 2^e seconds */
    uint32_t octaves;            /* o: n_bins = o << m */
    uint64_t* count;             /* DEVICE [C] u64 out, C = n_groups * W' */
    uint32_t* hist;              /* DEVICE [C][n_bins] u32 out */
    uint32_t* under;             /* DEVICE [C] u32 out, optional */
    uint32_t* over;              /* DEVICE [C] u32 out, optional */
    uint32_t* nan;               /* DEVICE [C] u32 out, optional */
    double elapsed_ms;           /* out: wall time of the call */
    uint64_t scratch_bytes;      /* out: size of the engine's scratch after the call */
} af_latency_histogram_t;
int af_engine_summarize_latency_histogram(af_engine_t* engine, const af_outputs_t* out, af_latency_histogram_t* histogram);

/* PAIRED LATENCY DIFFERENCES between scenarios that share their seeds (asyncflow_amd/csrc/af_paired.hpp): two scenarios of one batch
 * with the same seed and the same generator columns were sent the same requests at the same instants, and every stored `start` is,
 * bit for bit, one of the arrival times af_arrivals_t.times hands out.  The call joins the clock rows of both sides through that
 * arrival row and reports the latency difference of the SAME request under A and under B -- the paired estimator common random
 * numbers are shared for.  Reads outputs.clock and outputs.counts; no simulation kernel runs.
 * Pair p: a = pair_a[p], b = pair_b[p]; A = times[time_row[p]], ascending, +inf behind the last arrival, m = its finite entries;
 * side x has m_x = min(counts[x][AF_CNT_COMPLETED], clock_capacity) stored rows (start_i, finish_i).
 *     match            row i of side x maps to j = #{ k < m : A[k] < start_i } (np.searchsorted "left") when j < m and the u64 word
 *                      of A[j] is the word of start_i (a NaN never matches).  row_x[j] = the smallest i that maps to j, AF_PAIR_NONE
 *                      without one.  unmatched_x = m_x - #{ j : row_x[j] set }: the rows that map nowhere or lose their j to a
 *                      smaller row index (two arrivals of one bit pattern: the result stays a function of the data alone)
 *     arrival j        both (row_a[j] and row_b[j] set), only_a, only_b, neither -- the latter three were dropped or still in flight
 *                      at the end of the run on one or both sides; the two are not told apart.  Of a `both` arrival lat_x = finish -
 *                      start of row row_x[j] and d = lat_b - lat_a, three f64 subtractions; d NaN: counted in nan, nothing else
 *     window           by the arrival time, the same on both sides: edges[w] < A[j] <= edges[w + 1] (af_windows_t's rule), a
 *                      contiguous range of j; A[j] <= edges[0] or > edges[W]: in no window.  Without edges (n_windows == 0, edges
 *                      NULL) one window over every arrival.  W' = max(n_windows, 1)
 *     per (pair, window)   pair_counts[5] u32 = both, only_a, only_b, neither, nan (nan is part of both);  pair_sums[2] f64 = sum_d,
 *                      sum_a over the `both` arrivals with d not NaN in a FIXED order: lane l = j mod 64 adds its values in
 *                      ascending j from +0.0, then part[l] += part[l + h] for l < h, h = 32, 16, 8, 4, 2, 1; sum = part[0]
 *     per cell c = g * W' + w, over the pairs of group g   cell_counts[8] u64 = the five counts, slower (d > 0), faster (d < 0),
 *                      equal (d == 0);  above[n_thresholds] u64 = #{ d > thresholds[t] };  extremes[2] f64 = min_d, max_d in float
 *                      order (-0.0 below +0.0), +inf / -inf for a cell without a value;  hist[2][n_bins] u32 on af_latency_histogram_t's
 *                      bit rule: [0] bins d > 0 on d, [1] bins d < 0 on -d;  tails[4] u32 = under_pos, under_neg (0 < |d| < 2^min_exp),
 *                      over_pos, over_neg (at or above the last bin's end, the infinities).  equal + sum(tails) + sum(hist) + nan == both
 * Cells take integer + and min / max only: no word depends on the launch, on the chunks or on the order of the pairs.
 * A skipped pair (AF_POOL_SKIP) is in no cell; its per-pair outputs are written like any other's.
 * Refused, no output touched: n_pairs, n_groups, n_scenarios or draw_capacity == 0, a NULL pair_a / pair_b / time_row / times /
 * outputs.clock / outputs.counts or output other than row_a / row_b (above may be NULL with n_thresholds == 0), a binning outside
 * af_latency_histogram_t's ranges, edges not finite or not strictly increasing, edges NULL with n_windows > 0 (or given with 0), more
 * than AF_MAX_PAIR_THRESHOLDS thresholds or one that is not finite, a pair_a / pair_b >= n_scenarios, a time_row >= n_time_rows, a
 * group id >= n_groups -- the ids are read back and checked on the host -- (AF_ERR_INVALID); n_pairs * W' >= 2^32, n_groups * W' *
 * n_bins >= 2^32, draw_capacity >= 2^31, a group whose pairs could match 2^32 or more requests, no room for one pair's slots
 * (AF_ERR_CAPACITY); a planning-only engine (AF_ERR_NO_DEVICE).
 * outputs.clock must be 16-byte aligned.  Scratch kept by the engine: 8 B per edge and threshold and 2 * 4 B per (pair, draw) for
 * the pairs of one chunk (a side whose row_a / row_b is given needs none); the pairs are taken in chunks that fit the memory.
 * Synchronous; the struct is written back. */
#define AF_MAX_PAIR_THRESHOLDS 64
#define AF_PAIR_NONE 0xFFFFFFFFu
typedef struct af_pairs {
    uint32_t n_scenarios;        /* the scenarios of `out`: pair_a / pair_b index them */
    uint32_t n_pairs;
    uint32_t n_groups;
    uint32_t n_windows;          /* 0: one window over every arrival (edges NULL) */
    const uint32_t* pair_a;      /* DEVICE [n_pairs] */
    const uint32_t* pair_b;      /* DEVICE [n_pairs] */
    const uint32_t* group;       /* DEVICE [n_pairs] group id per pair (AF_POOL_SKIP: in no cell); NULL: all in group 0 */
    const double* edges;         /* HOST [n_windows + 1] strictly increasing, finite; NULL with n_windows == 0 */
    const double* times;         /* DEVICE [n_time_rows][draw_capacity]: arrival rows as af_arrivals_t.times hands them out */
    const uint32_t* time_row;    /* DEVICE [n_pairs]: the row of `times` that holds the pair's arrivals */
    uint32_t n_time_rows;
    uint32_t draw_capacity;
    const double* thresholds;    /* HOST [n_thresholds] finite, signed; NULL with n_thresholds == 0 */
    uint32_t n_thresholds;       /* 0 .. AF_MAX_PAIR_THRESHOLDS */
    uint32_t sub_bits;           /* the binning of |d|: af_latency_histogram_t's m, e, o */
    int32_t min_exp;
    uint32_t octaves;
    uint32_t* pair_counts;       /* DEVICE [n_pairs][W'][5] u32 out */
    double* pair_sums;           /* DEVICE [n_pairs][W'][2] f64 out */
    uint32_t* unmatched;         /* DEVICE [n_pairs][2] u32 out: unmatched_a, unmatched_b */
    uint64_t* cell_counts;       /* DEVICE [C][8] u64 out, C = n_groups * W' */
    uint64_t* above;             /* DEVICE [C][n_thresholds] u64 out */
    double* extremes;            /* DEVICE [C][2] f64 out */
    uint32_t* hist;              /* DEVICE [C][2][n_bins] u32 out */
    uint32_t* tails;             /* DEVICE [C][4] u32 out */
    uint32_t* row_a;             /* DEVICE [n_pairs][draw_capacity] u32 out, optional: the join itself (AF_PAIR_NONE: no row) */
    uint32_t* row_b;             /* DEVICE [n_pairs][draw_capacity] u32 out, optional */
    double elapsed_ms;           /* out: wall time of the call */
    uint64_t scratch_bytes;      /* out: size of the engine's scratch after the call */
} af_pairs_t;
int af_engine_summarize_pairs(af_engine_t* engine, const af_outputs_t* out, af_pairs_t* pairs);

/* BURN-RATE ALERT RULES evaluated at every tick over ROLLING look-backs of the completions (asyncflow_amd/csrc/af_alerts.hpp):
 * would my alert have fired during this outage, how many ticks after it began (the detection delay, as a distribution over the
 * replicas of a grid point), does it fire under plain load, how long does it stay on and how often does it flap.  Every other
 * analyzer puts requests into TUMBLING windows; a monitor evaluates a rule at every scrape over the last L ticks.  Reads
 * outputs.clock and outputs.counts only; no simulation kernel runs.
 * Per scenario s: m_s = min(counts[s][AF_CNT_COMPLETED], clock_capacity) stored rows (start_i, finish_i), t_s =
 * min(counts[s][AF_CNT_TICKS], tick_capacity) sample rows, p = sample_period; sample row k is taken at (k + 1) p.
 *     tick of a row    f_i = floor(finish_i / p): one f64 division rounded to nearest, then floor -- the rule of af_inflight_t.
 *                      Row i is COUNTED iff start_i and finish_i are not NaN and 0 <= f_i < t_s; the comparison is made on the
 *                      f64 quotient before any conversion to an integer: a huge or infinite quotient clips, it does not wrap.
 *                      Nothing else is rejected: start < 0, finish < start and a latency below a tick are counted, because a
 *                      monitor sees every completion
 *     bad              lat_i = finish_i - start_i, one f64 subtraction;  bad_i iff lat_i > slo as f64 (slo = +inf: nothing is bad)
 *     total[s][k]      = #{ counted i : f_i == k },  bad[s][k] = #{ counted bad i : f_i == k };  u32, whatever the order of the rows
 *     prefix           PT[k] = sum over j <= k of total[j], PB likewise; u32 (at most m_s)
 *     rolling          for a look-back of L >= 1 ticks  T_L[k] = PT[k] - (k >= L ? PT[k - L] : 0), B_L likewise: the first L - 1
 *                      ticks are evaluated on the rows that exist.  A look-back reaches across window edges: it is a property of
 *                      the tick
 *     rule r           cond_r[k] = B_long[k] den > num T_long[k]  &&  B_short[k] den > num T_short[k]  &&  T_long[k] >= min_total,
 *                      every product in u64;  firing_r[k] iff k + 1 >= hold_ticks and cond_r[j] for every j in (k - hold_ticks, k].
 *                      No hysteresis: the alert resolves at the first tick whose condition fails
 * Windows: tick_edges b[0] < ... < b[W] as in af_series_excursions_t, lo = min(b[w], t_s), hi = min(b[w + 1], t_s).  They choose
 * where firing is REPORTED, never what a rule sees.  Cell (s, w) / (s, w, r), u32, AF_TICK_NONE for "no such tick", written for
 * every scenario (a skipped one too):
 *     count            hi - lo                                     fired          the firing ticks of [lo, hi)
 *     episodes         the maximal runs of firing ticks, clipped at the window's edges: a run across an edge counts in both
 *     longest          the length of the longest run               longest_start  the start of the earliest run of that length
 *     first / last     the first / last firing tick;  last == hi - 1: still firing at the window's end
 * An empty cell: count 0, the counts 0 and the ticks AF_TICK_NONE.
 * Groups: group / AF_POOL_SKIP as in af_inflight_t.  Cell (g, w, r), integer atomics on arrays the call initialises itself:
 *     members u32 = the members with hi > lo;  fired_members u32 = those with first != AF_TICK_NONE;  open_members u32 = those
 *     with last == hi - 1;  fire_ticks u64 = the sum of fired;  fire_episodes u64 = the sum of episodes;  delay_hist u32
 *     [n_bins]: a member with first != AF_TICK_NONE adds 1 to bin min((first - lo) / delay_width, n_bins - 1) -- integer
 *     division, the last bin takes the rest.  With a window edge at an event's tick delay_hist is the detection-delay distribution
 *     of the grid point's replicas.
 * total / bad / firing: optional DEVICE [n_scenarios][tick_capacity]; firing has bit r set where rule r fires; rows k < t_s are
 * written, rows at or past t_s are left untouched; written for skipped scenarios too.  Every output pointer may be NULL: that
 * output is skipped.
 * COMPLETED REQUESTS ONLY: a dropped request, and a request still in flight when the run ended, is in no row -- an alert on
 * availability needs af_engine_outcome_alerts (below), and the last ticks of a run see fewer completions.
 * Every word is identical from run to run and does not depend on the batch a scenario sits in.
 * Refused, no output touched: n_scenarios, n_groups, n_windows or n_rules == 0, n_rules > AF_MAX_ALERT_RULES, rules NULL,
 * tick_edges NULL or not strictly increasing, a sample_period that is <= 0, NaN or infinite, slo NaN, a rule with short_ticks
 * == 0, long_ticks < short_ticks, den == 0, num > den or hold_ticks == 0, a group id >= n_groups, outputs.clock or outputs.counts
 * NULL, clock_capacity or tick_capacity == 0, with delay_hist n_bins == 0 or above AF_MAX_SERIES_HISTOGRAM_BINS or delay_width
 * == 0 (AF_ERR_INVALID); n_groups * n_windows * n_rules >= 2^32 - 1, n_scenarios * n_windows * n_rules >= 2^32 - 1,
 * tick_capacity >= 2^31 (AF_ERR_CAPACITY); a planning-only engine (AF_ERR_NO_DEVICE).
 * outputs.clock must be 16-byte aligned: a row is read as one (start, finish) pair by a 16-byte load (any device allocation is).
 * Scratch kept by the engine, shared with the other analyzers: 8 B per scenario and tick of tick_capacity for the prefix arrays,
 * 4 B per edge, 24 B per rule.  Synchronous; the struct is written back. */
#define AF_MAX_ALERT_RULES 32
typedef struct af_alert_rule {
    uint32_t long_ticks;         /* the long look-back, >= short_ticks */
    uint32_t short_ticks;        /* the short look-back, >= 1; == long_ticks: a single-window rule */
    uint32_t num;                /* the rule burns where the bad share is above num / den; num <= den */
    uint32_t den;                /* >= 1 */
    uint32_t min_total;          /* the fewest completions in the long look-back */
    uint32_t hold_ticks;         /* the `for:` clause: consecutive evaluations, >= 1 */
} af_alert_rule_t;
typedef struct af_alerts {
    uint32_t n_scenarios;
    uint32_t n_groups;
    uint32_t n_windows;
    uint32_t n_rules;            /* 1 .. AF_MAX_ALERT_RULES */
    const uint32_t* group;       /* DEVICE [n_scenarios] group id per scenario (AF_POOL_SKIP: left out); NULL: all in group 0 */
    const uint32_t* tick_edges;  /* HOST [n_windows + 1] strictly increasing tick indices */
    const af_alert_rule_t* rules; /* HOST [n_rules] */
    double sample_period;        /* p: seconds per tick, > 0 and finite */
    double slo;                  /* a request is bad when its latency is above slo; not NaN */
    uint32_t n_bins;             /* with delay_hist: 1 .. AF_MAX_SERIES_HISTOGRAM_BINS; ignored without */
    uint32_t delay_width;        /* with delay_hist: ticks per bin, >= 1; ignored without */
    uint32_t* count;             /* DEVICE [n_scenarios][n_windows] u32 out, optional */
    uint32_t* fired;             /* DEVICE [n_scenarios][n_windows][n_rules] u32 out, optional */
    uint32_t* episodes;          /* DEVICE [n_scenarios][n_windows][n_rules] u32 out, optional */
    uint32_t* longest;           /* DEVICE [n_scenarios][n_windows][n_rules] u32 out, optional */
    uint32_t* longest_start;     /* DEVICE [n_scenarios][n_windows][n_rules] u32 out, optional */
    uint32_t* first;             /* DEVICE [n_scenarios][n_windows][n_rules] u32 out, optional */
    uint32_t* last;              /* DEVICE [n_scenarios][n_windows][n_rules] u32 out, optional */
    uint32_t* members;           /* DEVICE [n_groups][n_windows][n_rules] u32 out, optional */
    uint32_t* fired_members;     /* DEVICE [n_groups][n_windows][n_rules] u32 out, optional */
    uint32_t* open_members;      /* DEVICE [n_groups][n_windows][n_rules] u32 out, optional */
    uint64_t* fire_ticks;        /* DEVICE [n_groups][n_windows][n_rules] u64 out, optional */
    uint64_t* fire_episodes;     /* DEVICE [n_groups][n_windows][n_rules] u64 out, optional */
    uint32_t* delay_hist;        /* DEVICE [n_groups][n_windows][n_rules][n_bins] u32 out, optional */
    uint32_t* total;             /* DEVICE [n_scenarios][tick_capacity] u32 out, optional */
    uint32_t* bad;               /* DEVICE [n_scenarios][tick_capacity] u32 out, optional */
    uint32_t* firing;            /* DEVICE [n_scenarios][tick_capacity] u32 out, optional: bit r = rule r fires */
    double elapsed_ms;           /* out: wall time of the call */
    uint64_t scratch_bytes;      /* out: size of the engine's scratch after the call */
} af_alerts_t;
int af_engine_summarize_alerts(af_engine_t* engine, const af_outputs_t* out, af_alerts_t* alerts);

/* ALERT RULES ON REQUEST OUTCOMES (asyncflow_amd/csrc/af_alert_outcomes.hpp): a CLIENT TIMEOUT makes a request that never came back
 * visible to the monitor.  A request sent at a that has no answer by a + timeout is an error at a + timeout, so every arrival
 * produces exactly one event, a completion or a timeout: the bad share has the arrivals as its denominator, and slo = +inf is a
 * pure availability alert.  At tick k a live monitor also knows only the completions so far and the timeouts of the requests sent
 * before k p - timeout.  Reads outputs.clock, outputs.counts and the arrival rows; no simulation kernel runs.
 * Scenario s has m_s stored rows (start_i, finish_i), t_s sample rows and p = sample_period, all as in af_alerts_t; an arrival row
 * a[0 .. draw_capacity), row time_row[s] of `times`, ascending with +inf behind the last arrival; tau = timeout, finite and > 0;
 * slo as in af_alerts_t: not NaN, +inf allowed.
 *     tick of a time   q(x) = floor(x / p): one f64 division, then floor.  It is in range iff 0 <= q < t_s, compared on the f64
 *                      quotient (af_alerts_t's rule)
 *     in-time row      start_i and finish_i are not NaN and lat_i = finish_i - start_i <= tau: one f64 subtraction, a NaN latency
 *                      is not in time.  A row that is not in time is never seen as a completion: the client gave up at start + tau
 *     C[k]             = #{ in-time rows with q(finish_i) == k }
 *     Cbad[k]          = those of C[k] with lat_i > slo
 *     G[k]             = #{ in-time rows with q(start_i + tau) == k }: one f64 addition, then the tick rule
 *     A[k]             = #{ j < draw_capacity : a[j] finite and q(a[j] + tau) == k }: the same operations
 *     timeouts[k]      = max(A[k] - G[k], 0)
 *     deficit[s]       = sum over k of max(G[k] - A[k], 0)
 *     timed_out[s]     = sum over k of timeouts[k]
 *     total[k]         = C[k] + timeouts[k]
 *     bad[k]           = Cbad[k] + timeouts[k]
 * deficit is 0 whenever the arrival row is the run's own (every stored start is, bit for bit, one of its arrivals, so a row and its
 * arrival land on the same timeout tick); a deficit above 0 says the arrival rows do not belong to these clock rows.  The result
 * is still defined.  Prefix sums, rolling look-backs, rules, windows, cells, group cells and delay_hist are exactly
 * af_engine_summarize_alerts's on these total / bad (alerts->total / bad receive them).  All per-tick values are u32.
 * The arrival rows are not checked for order on the device: a row that is not ascending gives meaningless counts and nothing worse.
 * flags[s]: AF_OUTCOME_ROWS_TRUNCATED when counts[s][AF_CNT_COMPLETED] > clock_capacity (rows are missing and would be miscounted
 * as timeouts), AF_OUTCOME_DEFICIT when deficit[s] > 0.  timeouts: rows k < t_s are written.
 * Refused, no output touched: everything af_engine_summarize_alerts refuses, and times NULL, draw_capacity or n_time_rows == 0,
 * time_row NULL with n_time_rows != n_scenarios, a time_row >= n_time_rows -- the ids are read back and checked on the host --, a
 * timeout that is NaN, infinite or <= 0 (AF_ERR_INVALID); draw_capacity or clock_capacity >= 2^31 (AF_ERR_CAPACITY).
 * Scratch as af_engine_summarize_alerts.  Synchronous; elapsed_ms and scratch_bytes of `alerts` are written back. */
#define AF_OUTCOME_ROWS_TRUNCATED 1u
#define AF_OUTCOME_DEFICIT 2u
typedef struct af_alert_outcomes {
    const double* times;         /* DEVICE [n_time_rows][draw_capacity], as af_arrivals_t.times hands them out */
    const uint32_t* time_row;    /* DEVICE [n_scenarios]; NULL: scenario s reads row s (n_time_rows == n_scenarios) */
    uint32_t n_time_rows;
    uint32_t draw_capacity;
    double timeout;              /* finite, > 0 */
    uint32_t* timeouts;          /* DEVICE [n_scenarios][tick_capacity] u32 out, optional */
    uint32_t* timed_out;         /* DEVICE [n_scenarios] u32 out, optional */
    uint32_t* deficit;           /* DEVICE [n_scenarios] u32 out, optional */
    uint32_t* flags;             /* DEVICE [n_scenarios] u32 out, optional */
} af_alert_outcomes_t;
/* (Not an af_engine_summarize_* name on purpose: the rules, cells and scratch are af_engine_summarize_alerts's; what is new is
 * where total / bad come from.) */
int af_engine_outcome_alerts(af_engine_t* engine, const af_outputs_t* out, af_alert_outcomes_t* outcomes, af_alerts_t* alerts);

/* Latency by the STATE A REQUEST MET ON ARRIVAL (asyncflow_amd/csrc/af_state.hpp): how slow were the requests that arrived while
 * the ready queue, the IO sleep set, the RAM or an edge was at level b -- does p95 rise with the queue at a server, with RAM in
 * use, with the connections on an edge?  A cell is (group g, arrival window w, bin b of ONE sampled series at the row's tick).
 * For scenario s, m_s = min(counts[s][AF_CNT_COMPLETED], clock_capacity) rows and t_s = min(counts[s][AF_CNT_TICKS],
 * tick_capacity) sample rows; a stored row i has start = clock[s][i][0].
 *   tick    q = floor(start / sample_period) -- one f64 division rounded to nearest, then floor --, k = q - 1.  Sample row k is
 *           taken at (k + 1) * sample_period (collector.py:53; see af_series_windows_t), so k is the last sample taken at or
 *           before the arrival AS THE F64 QUOTIENT SEES IT (a start a rounding error below a multiple of the period may be
 *           given that multiple's sample).  The row has no state and belongs to no cell when q < 1 (no sample yet), k >= t_s,
 *           or start is NaN or negative.
 *   value   x = the word samples[s][k][column] as f64 exactly as af_series_histogram_t takes it: (double)word of an integer
 *           series, (double)(float) of a ram_in_use column.  Only that word of a row is read: never the padding, never a row
 *           at or past t_s.
 *   bin     x < lo -> no cell (-0.0 is not below 0.0; a -2^-45 residue is);  t = (x - lo) / width, one f64 subtraction and one
 *           f64 division;  t >= (double)n_bins -> bin n_bins - 1 (the last bin takes the overflow, as af_summary_t.hist does:
 *           "queue >= k" is a condition);  otherwise bin (uint32_t)t.
 *   window  with n_windows > 0 af_engine_summarize_arrival_windows's rule, edges[w] < start <= edges[w + 1], else no cell; with
 *           n_windows == 0 and edges == NULL ONE window with no condition on time.  W' = max(n_windows, 1).
 * Cell (g, w, b) has index (g * W' + w) * n_bins + b; its sample is the concatenation, in ascending scenario index over the
 * members of g, of finish - start over the member's rows of that cell IN ROW ORDER.
 *   af_engine_summarize_state_windows    stats [n_groups][W'][n_bins][8]: numpy's eight statistics of the cell, bit for bit
 *                                        (an empty cell: total 0, the rest NaN); row_bounds, if given, receives the CUMULATIVE
 *                                        CELL COUNTS [n_scenarios][W' * n_bins + 1]: c_s[0] = 0, c_s[k + 1] - c_s[k] = the rows of
 *                                        scenario s in cell (w, b) with w * n_bins + b = k (also of skipped scenarios)
 *   af_engine_summarize_state_quantiles  count / quantiles / within of af_quantiles_t over the same cells ([C], [C][n_levels],
 *                                        [C][n_thresholds] with C = n_groups * W' * n_bins): np.quantile and exact counts
 * The cohorts are RIGHT-CENSORED like the arrival windows': a request that had not completed when the run ended, or was
 * dropped, is in no row, so a cell's total / count is its cohort's completions.  A cell's result is identical from run to run
 * and does not depend on the batch a scenario sits in (integer atomics only; a cell's rows are placed in row order by one wave).
 * Refused, no output touched: n_bins == 0; a width that is <= 0, NaN or infinite; a lo that is NaN or infinite; a
 * sample_period that is <= 0, NaN or infinite; column >= af_series_count; outputs.samples or outputs.counts NULL or
 * tick_capacity == 0; edges given with n_windows == 0 or missing with n_windows > 0; the refusals of the arrival entry points
 * (AF_ERR_INVALID); n_groups * W' * n_bins >= 2^32 - 1, n_scenarios * (W' * n_bins + 1) >= 2^32, a cell of 2^32 or more latencies
 * (AF_ERR_CAPACITY); a planning-only engine (AF_ERR_NO_DEVICE).  `out` needs clock, samples, both capacities and counts.
 * Scratch kept by the engine: af_engine_summarize_windows's / af_engine_summarize_quantiles's with W' * n_bins for n_windows (8 B per
 * latency in a cell + 8 B per (scenario, cell) + at most 12 B per (group, cell) + 8 B per edge + the large cells' parts); the
 * key of a row is recomputed by the second pass, not stored.  Synchronous; the request struct is written back. */
typedef struct af_state_bins {
    uint32_t column;        /* the sampled series, < af_series_count */
    uint32_t n_bins;        /* > 0 */
    double lo;              /* finite: the lower edge of bin 0 */
    double width;           /* finite, > 0 */
    double sample_period;   /* seconds, finite, > 0: the plan's */
} af_state_bins_t;
int af_engine_summarize_state_windows(af_engine_t* engine, const af_outputs_t* out, const af_state_bins_t* bins, af_windows_t* windows);
int af_engine_summarize_state_quantiles(af_engine_t* engine, const af_outputs_t* out, const af_state_bins_t* bins, af_quantiles_t* quantiles);

/* af_engine_run followed by af_engine_summarize, in one call and with the same results (replaces SimulationRunner.run +
 * ResultsAnalyzer.process_all_metrics, simulation_runner.py:349-376 + analyzer.py:75-81, for the whole sweep).
 * summary->n_scenarios must equal sweep->n_scenarios.  Where the sweep is ONE launch of the stage-parallel kernel, the analyzer
 * starts on a second stream as soon as the scenarios of the kernel's full residency rounds have finished (a counter the kernel's
 * waves bump; hipStreamWaitValue32) and runs beside its last, partial round (af_stats_t.summary_overlapped / summary_beside_ms);
 * scenarios it meets unfinished, and everything else, are analysed after the simulation, as the two separate calls would.
 * AF_NO_SUMMARY_OVERLAP=1 in the environment: always the latter (measurements). */
int af_engine_run_summarized(af_engine_t* engine, const af_sweep_t* sweep, const af_outputs_t* out, const af_summary_t* summary);

/* ---- the one collective of a multi-GPU sweep ---------------------------------------------
 * Scenarios shard over the GPUs of a node with no exchange during simulation; at the end every rank
 * contributes the summaries of ITS scenarios and receives everybody's: one grouped RCCL all-gather
 * over xGMI on the engine's stream.  The reference has nothing to replace here (single process, one
 * env per run: docs/api/high-level/runner.md:203-207); this is the Monte-Carlo roadmap item
 * (ROADMAP.md:23-29) across devices.
 *
 * RCCL is resolved at run time, NOT linked: af_comm_load(path) opens a specific librccl (a host that
 * already uses RCCL -- e.g. PyTorch, whose copy is torch/lib/librccl.so -- must name that one so that a
 * single RCCL lives in the process); with NULL the engine takes the RCCL already visible in the process,
 * then $ASYNCFLOW_RCCL_LIB, then librccl.so.1.  `comm` is a ncclComm_t: the host's own, or one made by
 * af_comm_init_rank from the 128-byte id rank 0 obtained with af_comm_unique_id and shared out of band. */
#define AF_COMM_ID_BYTES 128
int af_comm_load(const char* librccl_path);
int af_comm_unique_id(void* id_out /* AF_COMM_ID_BYTES */);
int af_comm_init_rank(const void* id, int world_size, int rank, int device, void** comm_out);
void af_comm_destroy(void* comm);
/* What RCCL itself says about a communicator: ncclCommCount / ncclCommUserRank (either output may be NULL).  A
 * multi-GPU bench line carries these next to WORLD_SIZE so that the first run on N GPUs certifies that RCCL saw N ranks. */
int af_comm_count(void* comm, int* world_size_out, int* rank_out);
/* All-gather of per-scenario summaries: every non-NULL array of `local` (n_scenarios rows: the rank's
 * shard, padded by the caller to the same n on every rank) into the array of the same name in `gathered`
 * (world_size * n_scenarios rows, rank order).  rps_buckets / hist_bins give the row lengths; series
 * arrays have af_series_count(plan) columns.  DEVICE memory owned by the caller; synchronous. */
int af_engine_gather(af_engine_t* engine, void* rccl_comm, int world_size, const af_summary_t* local,
                     const af_summary_t* gathered);

/* Replaces: _start_* + env.run(until=T) (simulation_runner.py:301-369) for
 * sweep->n_scenarios independent scenarios. */
int af_engine_run(af_engine_t* eng, const af_sweep_t* sweep, const af_outputs_t* out);
int af_engine_stats(const af_engine_t* eng, af_stats_t* stats);
/* Empty string: the stage-parallel kernel can run this engine's plan; otherwise why not (the plan then
 * always runs on the next-event kernels).  The pointer stays valid until the engine is destroyed. */
const char* af_engine_flow_reason(const af_engine_t* eng);
void af_engine_destroy(af_engine_t* eng);

/* Number of sampler ticks env.run(until=T) takes for (period, T): repeated f64
 * addition from 0, tick at t < T only (collector.py:50-53). */
uint32_t af_tick_count(double sample_period, double total_time);
uint32_t af_series_count(const af_plan_t* plan);  /* n_edges + 3*n_servers */
uint32_t af_series_pitch(const af_plan_t* plan);  /* row length of outputs.samples (multiple of 4) */

const char* af_last_error(void);
int af_abi_version(void);

/* Spec probes (device): evaluate the engine's own RNG/math on the GPU so the
 * parity tests can pin them against the oracle bit for bit.
 *   kind 0: uniform(seed,stream,index,j)
 *   kind 1: log(x)   kind 2: exp(x)   kind 3: norminv(x)   kind 4: sqrt(x)
 *   kind 5: x / y (x = in[i], y = in2[i])
 *   kind 6: poisson(x)   kind 7: log of a normal number in (0, 1] (the exponential draws' logarithm)
 *   kinds 8-10 take and give BIT PATTERNS: 8 / 9: Philox words x << 32 | y  /  z << 32 | w of block (index, 0),
 *   in[i] = the 64-bit seed, in2[i] = stream << 32 | index; 10: 1 - u of the uniform made of the words in[i] = hi << 32 | lo
 * `in`, `in2`, `out` are HOST arrays of n doubles (kind 0: in[i] = index,
 * in2[i] = stream * 65536 + j, both exact small integers). */
int af_probe_math(int device, int kind, uint64_t seed, const double* in, const double* in2,
                  double* out, size_t n);

/* Measurement probe (device): one launch of n_waves wavefronts, each filling its own contiguous region of
 * bytes_per_wave bytes exactly once with the store shape of
 *   pattern 0: wide coalesced stores (16 B per lane, 1 KB per instruction) -- the shape rocprofv3's WRITE_SIZE is
 *              calibrated for (MI355X_MICROARCH.md);
 *   pattern 1: the stage-parallel kernel's rqs_clock store: 16 B per lane over `lanes` consecutive lanes (0 = 57,
 *              the average batch of BASELINE config 2), batch after batch;
 *   pattern 2: its sampled-series store for a 12-word pitch: 4 B per lane over 60 lanes = five 48-byte rows.
 * Run under `rocprofv3 --pmc WRITE_SIZE` (scripts/calibrate_write_size.py) it tells how many counter units a byte
 * of each shape costs, i.e. whether WRITE_SIZE above the output size is traffic or counting granularity.
 * ms_out (may be NULL): HIP-event time of the launch. */
int af_probe_store(int device, int pattern, uint32_t n_waves, uint64_t bytes_per_wave, uint32_t lanes, double* ms_out);

/* Test probe (device): the scratch pool of `engine`, from which every analyzer call takes its device scratch, becomes
 * exactly `bytes` large (freed and allocated anew when its size differs, so it can shrink; 0 frees it) and every 32-bit
 * word of it `word`.  From then on every growth of that engine's pool is filled with `word` before anything else uses it.
 * No analyzer may rely on what its scratch held before the call: with this probe a test chooses what it held
 * (tests/test_gpu_scratch_history.py).  An engine that never received the call works exactly as without the probe.
 * AF_ERR_NO_DEVICE on a planning-only engine. */
int af_probe_scratch(af_engine_t* engine, uint64_t bytes, uint32_t word);

#ifdef __cplusplus
}
#endif
#endif /* ASYNCFLOW_HIP_H */
