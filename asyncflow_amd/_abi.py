"""ctypes mirror of include/asyncflow_hip.h (the C ABI of the HIP engine).

Field order and types must match the header exactly; tests/test_abi.py checks
``sizeof`` against the values the shared library reports and that every symbol
declared in the header is exported.
"""

from __future__ import annotations

import ctypes as C

AF_ABI_VERSION = 7

# af_status
MAX_REQUEST_CAPACITY = 65535   # include/asyncflow_hip.h AF_MAX_REQUEST_CAPACITY
MAX_FIFO_CAPACITY = 1 << 20    # AF_MAX_FIFO_CAPACITY (rounds 1-5: 16 384)
COMM_ID_BYTES = 128            # AF_COMM_ID_BYTES
AF_OK = 0
AF_ERR_INVALID = -1
AF_ERR_NO_DEVICE = -2
DEVICE_PLAN_ONLY = -1          # AF_DEVICE_PLAN_ONLY
AF_ERR_HIP = -3
AF_ERR_CAPACITY = -4
AF_ERR_ABI = -5

# af_dist (src/asyncflow/config/constants.py:39-52)
DIST_CODES = {"poisson": 0, "normal": 1, "log_normal": 2, "exponential": 3, "uniform": 4}
# af_node_kind
NODE_CLIENT, NODE_LB, NODE_SERVER = 0, 1, 2
# af_lb_algo (constants.py:144-148)
LB_CODES = {"round_robin": 0, "least_connection": 1}
# af_step_kind
STEP_CPU, STEP_IO = 0, 1
# af_metric_bit (constants.py:195-205)
METRIC_BITS = {
    "ready_queue_len": 1,
    "event_loop_io_sleep": 2,
    "ram_in_use": 4,
    "edge_concurrent_connection": 8,
}
# af_param
PARAM_CODES = {
    "gen_users_mean": 0,
    "gen_users_sigma": 1,
    "gen_rpm_mean": 2,
    "edge_mean": 3,
    "edge_sigma": 4,
    "edge_dropout": 5,
    "step_time": 6,
    "gen_window": 7,
    "srv_cores": 8,
    "srv_ram_mb": 9,
    "emark_time": 10,
    "emark_delta": 11,
    "emark_edge": 12,
    "smark_time": 13,
    "smark_lb_edge": 14,
    "smark_down": 15,
}
# af_count_slot
CNT_GENERATED, CNT_COMPLETED, CNT_DROPPED, CNT_EVENTS, CNT_TICKS, CNT_FLAGS, CNT_MAX_LIVE, CNT_MARKS = range(8)
CNT_SLOTS = 8
# af_flag
FLAG_POOL_OVERFLOW = 1
FLAG_FIFO_OVERFLOW = 2
FLAG_CLOCK_OVERFLOW = 4
FLAG_TICK_OVERFLOW = 8
FLAG_RAM_STARVED = 16
FLAG_TIME_TIE = 32
FLAG_DRAW_OVERFLOW = 64
FLAG_NEGATIVE_DELAY = 1 << 13
FLAG_NAMES = {
    FLAG_POOL_OVERFLOW: "request pool overflow (raise request_capacity)",
    FLAG_FIFO_OVERFLOW: "server wait-queue overflow (raise fifo_capacity)",
    FLAG_CLOCK_OVERFLOW: "rqs_clock capacity overflow (raise clock_capacity)",
    FLAG_TICK_OVERFLOW: "sample capacity overflow",
    FLAG_RAM_STARVED: "a server's RAM queue is blocked for good, as in the reference: a request needs more RAM than the server owns, "
                      "or a refused fractional RAM put faces a waiter that does not fit",
    FLAG_TIME_TIE: "a zero-delay timeout was created in the middle of a zero-time cascade (SimPy may order the pending steps differently)",
    FLAG_DRAW_OVERFLOW: "more arrivals than draw_capacity (raise clock_capacity)",
    FLAG_NEGATIVE_DELAY: "a message was sent with transit + spike < 0 (the reference raises ValueError 'Negative delay')",
}
FATAL_FLAGS = (
    FLAG_POOL_OVERFLOW | FLAG_FIFO_OVERFLOW | FLAG_CLOCK_OVERFLOW | FLAG_TICK_OVERFLOW | FLAG_DRAW_OVERFLOW
)

_pd = C.POINTER(C.c_double)
_pi32 = C.POINTER(C.c_int32)
_pu32 = C.POINTER(C.c_uint32)
_pu8 = C.POINTER(C.c_uint8)
_pu64 = C.POINTER(C.c_uint64)


class AfPlan(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("struct_size", C.c_uint32),
        ("total_time", C.c_double),
        ("sample_period", C.c_double),
        ("metrics_mask", C.c_uint32),
        ("gen_users_dist", C.c_uint32),
        ("gen_users_mean", C.c_double),
        ("gen_users_sigma", C.c_double),
        ("gen_rpm_mean", C.c_double),
        ("gen_window_s", C.c_double),
        ("gen_out_edge", C.c_int32),
        ("n_edges", C.c_uint32),
        ("n_servers", C.c_uint32),
        ("client_out_edge", C.c_int32),
        ("has_lb", C.c_uint32),
        ("lb_algo", C.c_uint32),
        ("n_lb_edges", C.c_uint32),
        ("lb_edges", _pi32),
        ("edge_target_kind", _pu8),
        ("edge_target_idx", _pi32),
        ("edge_dist", _pu8),
        ("edge_mean", _pd),
        ("edge_sigma", _pd),
        ("edge_dropout", _pd),
        ("srv_cores", _pu32),
        ("srv_ram_mb", _pd),
        ("srv_out_edge", _pi32),
        ("srv_ep_begin", _pu32),
        ("n_endpoints", C.c_uint32),
        ("ep_step_begin", _pu32),
        ("ep_ram", _pd),
        ("n_steps", C.c_uint32),
        ("step_kind", _pu8),
        ("step_time", _pd),
        ("n_edge_marks", C.c_uint32),
        ("emark_time", _pd),
        ("emark_edge", _pi32),
        ("emark_delta", _pd),
        ("n_srv_marks", C.c_uint32),
        ("smark_time", _pd),
        ("smark_lb_edge", _pi32),
        ("smark_down", _pu8),
    ]


class AfOverride(C.Structure):
    _fields_ = [("param", C.c_uint32), ("index", C.c_uint32), ("values", _pd)]


class AfSweep(C.Structure):
    _fields_ = [
        ("n_scenarios", C.c_uint32),
        ("seeds", _pu64),
        ("n_overrides", C.c_uint32),
        ("overrides", C.POINTER(AfOverride)),
        ("draw_capacity", C.c_uint32),
    ]


class AfOutputs(C.Structure):
    _fields_ = [
        ("clock_capacity", C.c_uint32),
        ("clock", C.c_void_p),
        ("tick_capacity", C.c_uint32),
        ("samples", C.c_void_p),
        ("counts", C.c_void_p),
        ("online_hist_bins", C.c_uint32),
        ("online_hist_max", C.c_double),
        ("online_hist", C.c_void_p),
        ("online_rps_buckets", C.c_uint32),
        ("online_rps", C.c_void_p),
    ]


class AfEngineOptions(C.Structure):
    _fields_ = [
        ("request_capacity", C.c_uint32),
        ("fifo_capacity", C.c_uint32),
        ("force_global_state", C.c_uint32),
        ("lanes_per_wave", C.c_uint32),
        ("draw_memory_mb", C.c_uint32),
        ("expect_shared_instants", C.c_uint32),
        ("flow_mode", C.c_uint32),
        ("flow_list_entries", C.c_uint32),
        ("flow_ring_rows", C.c_uint32),
    ]


class AfStats(C.Structure):
    _fields_ = [
        ("kernel_ms", C.c_double),
        ("pregen_ms", C.c_double),
        ("h2d_ms", C.c_double),
        ("summary_ms", C.c_double),
        ("draw_bytes", C.c_uint64),
        ("state_bytes_per_scenario", C.c_uint64),
        ("state_in_lds", C.c_uint32),
        ("lds_bytes_per_wave", C.c_uint32),
        ("waves", C.c_uint32),
        ("lanes_per_wave", C.c_uint32),
        ("chunks", C.c_uint32),
        ("specialised_launches", C.c_uint32),
        ("shared_instant_scenarios", C.c_uint32),
        ("request_capacity", C.c_uint32),
        ("fifo_capacity", C.c_uint32),
        ("flow_kernel_ms", C.c_double),
        ("flow_scenarios", C.c_uint32),
        ("flow_fallback", C.c_uint32),
        ("flow_fallback_tie", C.c_uint32),
        ("flow_fallback_list", C.c_uint32),
        ("flow_fallback_ring", C.c_uint32),
        ("flow_fallback_ram", C.c_uint32),
        ("flow_retried", C.c_uint32),
        ("flow_to_next_event", C.c_uint32),
        ("flow_list_entries", C.c_uint32),
        ("flow_ring_rows", C.c_uint32),
        ("flow_lds_bytes", C.c_uint32),
        ("jit_fallbacks", C.c_uint32),
        ("gather_ms", C.c_double),
        ("pregen_group", C.c_uint32),
        ("summary_overlapped", C.c_uint32),
        ("summary_beside_ms", C.c_double),
    ]


FLOW_RING_IN_HBM = 0xFFFFFFFF   # AF_FLOW_RING_IN_HBM


class AfSummary(C.Structure):
    _fields_ = [
        ("n_scenarios", C.c_uint32),
        ("rps_buckets", C.c_uint32),
        ("hist_bins", C.c_uint32),
        ("hist_max", C.c_double),
        ("stats", C.c_void_p),
        ("rps", C.c_void_p),
        ("hist", C.c_void_p),
        ("series_mean", C.c_void_p),
        ("series_max", C.c_void_p),
    ]


POOL_SKIP = 0xFFFFFFFF   # AF_POOL_SKIP: af_pooled_t.group of a scenario left out


class AfPooled(C.Structure):
    """``af_pooled_t``: request of ``af_engine_summarize_pooled`` (``elapsed_ms`` is written back)."""

    _fields_ = [
        ("n_scenarios", C.c_uint32),
        ("n_groups", C.c_uint32),
        ("group", C.c_void_p),
        ("stats", C.c_void_p),
        ("elapsed_ms", C.c_double),
    ]


class AfWindows(C.Structure):
    """``af_windows_t``: request of ``af_engine_summarize_windows`` (``elapsed_ms`` and ``scratch_bytes`` are written back)."""

    _fields_ = [
        ("n_scenarios", C.c_uint32),
        ("n_groups", C.c_uint32),
        ("n_windows", C.c_uint32),
        ("group", C.c_void_p),
        ("edges", C.POINTER(C.c_double)),
        ("stats", C.c_void_p),
        ("row_bounds", C.c_void_p),
        ("elapsed_ms", C.c_double),
        ("scratch_bytes", C.c_uint64),
    ]


class AfSeriesWindows(C.Structure):
    """``af_series_windows_t``: request of ``af_engine_summarize_series_windows`` (``elapsed_ms`` and ``scratch_bytes`` are
    written back)."""

    _fields_ = [
        ("n_scenarios", C.c_uint32),
        ("n_groups", C.c_uint32),
        ("n_windows", C.c_uint32),
        ("group", C.c_void_p),
        ("tick_edges", C.POINTER(C.c_uint32)),
        ("thresholds", C.POINTER(C.c_double)),
        ("count", C.c_void_p),
        ("mean", C.c_void_p),
        ("minv", C.c_void_p),
        ("maxv", C.c_void_p),
        ("above", C.c_void_p),
        ("elapsed_ms", C.c_double),
        ("scratch_bytes", C.c_uint64),
    ]


MAX_QUANTILE_LEVELS = 64   # AF_MAX_QUANTILE_LEVELS
MAX_SLO_THRESHOLDS = 64    # AF_MAX_SLO_THRESHOLDS


class AfQuantiles(C.Structure):
    """``af_quantiles_t``: request of ``af_engine_summarize_quantiles`` (``elapsed_ms`` and ``scratch_bytes`` are written
    back)."""

    _fields_ = [
        ("n_scenarios", C.c_uint32),
        ("n_groups", C.c_uint32),
        ("n_windows", C.c_uint32),
        ("group", C.c_void_p),
        ("edges", C.POINTER(C.c_double)),
        ("n_levels", C.c_uint32),
        ("levels", C.POINTER(C.c_double)),
        ("n_thresholds", C.c_uint32),
        ("thresholds", C.POINTER(C.c_double)),
        ("count", C.c_void_p),
        ("quantiles", C.c_void_p),
        ("within", C.c_void_p),
        ("elapsed_ms", C.c_double),
        ("scratch_bytes", C.c_uint64),
    ]


class AfCellsExport(C.Structure):
    """``af_cells_export_t``: request of ``af_engine_export_cells`` (``lat_count``, ``elapsed_ms`` and ``scratch_bytes`` are
    written back)."""

    _fields_ = [
        ("n_scenarios", C.c_uint32),
        ("n_windows", C.c_uint32),
        ("by_arrival", C.c_uint32),
        ("group", C.c_void_p),
        ("edges", C.POINTER(C.c_double)),
        ("lat", C.c_void_p),
        ("lat_capacity", C.c_uint64),
        ("seg_bounds", C.c_void_p),
        ("lat_count", C.c_uint64),
        ("elapsed_ms", C.c_double),
        ("scratch_bytes", C.c_uint64),
    ]


class AfCells(C.Structure):
    """``af_cells_t``: request of ``af_engine_import_cells`` (``elapsed_ms`` and ``scratch_bytes`` are written back)."""

    _fields_ = [
        ("n_scenarios", C.c_uint32),
        ("n_groups", C.c_uint32),
        ("n_windows", C.c_uint32),
        ("group", C.POINTER(C.c_uint32)),
        ("seg_bounds", C.POINTER(C.c_uint32)),
        ("seg_begin", C.POINTER(C.c_uint64)),
        ("lat", C.c_void_p),
        ("n_lat", C.c_uint64),
        ("stats", C.c_void_p),
        ("n_levels", C.c_uint32),
        ("levels", C.POINTER(C.c_double)),
        ("n_thresholds", C.c_uint32),
        ("thresholds", C.POINTER(C.c_double)),
        ("count", C.c_void_p),
        ("quantiles", C.c_void_p),
        ("within", C.c_void_p),
        ("elapsed_ms", C.c_double),
        ("scratch_bytes", C.c_uint64),
    ]


MAX_SERIES_QUANTILE_LEVELS = 16   # AF_MAX_SERIES_QUANTILE_LEVELS


class AfSeriesQuantiles(C.Structure):
    """``af_series_quantiles_t``: request of ``af_engine_summarize_series_quantiles`` (``elapsed_ms`` and ``scratch_bytes``
    are written back)."""

    _fields_ = [
        ("n_scenarios", C.c_uint32),
        ("n_groups", C.c_uint32),
        ("n_windows", C.c_uint32),
        ("group", C.c_void_p),
        ("tick_edges", C.POINTER(C.c_uint32)),
        ("n_levels", C.c_uint32),
        ("levels", C.POINTER(C.c_double)),
        ("n_columns", C.c_uint32),
        ("columns", C.POINTER(C.c_uint32)),
        ("count", C.c_void_p),
        ("quantiles", C.c_void_p),
        ("elapsed_ms", C.c_double),
        ("scratch_bytes", C.c_uint64),
    ]


TICK_NONE = 0xFFFFFFFF   # AF_TICK_NONE


class AfSeriesExcursions(C.Structure):
    """``af_series_excursions_t``: request of ``af_engine_summarize_series_excursions`` (``elapsed_ms`` and
    ``scratch_bytes`` are written back)."""

    _fields_ = [
        ("n_scenarios", C.c_uint32),
        ("n_windows", C.c_uint32),
        ("tick_edges", C.POINTER(C.c_uint32)),
        ("thresholds", C.POINTER(C.c_double)),
        ("count", C.c_void_p),
        ("above", C.c_void_p),
        ("runs", C.c_void_p),
        ("longest", C.c_void_p),
        ("longest_start", C.c_void_p),
        ("first", C.c_void_p),
        ("last", C.c_void_p),
        ("peak_tick", C.c_void_p),
        ("elapsed_ms", C.c_double),
        ("scratch_bytes", C.c_uint64),
    ]


MAX_SERIES_HISTOGRAM_BINS = 1024   # AF_MAX_SERIES_HISTOGRAM_BINS


class AfSeriesHistogram(C.Structure):
    """``af_series_histogram_t``: request of ``af_engine_summarize_series_histogram`` (``elapsed_ms`` and
    ``scratch_bytes`` are written back)."""

    _fields_ = [
        ("n_scenarios", C.c_uint32),
        ("n_groups", C.c_uint32),
        ("n_windows", C.c_uint32),
        ("group", C.c_void_p),
        ("tick_edges", C.POINTER(C.c_uint32)),
        ("n_columns", C.c_uint32),
        ("columns", C.POINTER(C.c_uint32)),
        ("n_bins", C.c_uint32),
        ("lo", C.POINTER(C.c_double)),
        ("width", C.POINTER(C.c_double)),
        ("count", C.c_void_p),
        ("hist", C.c_void_p),
        ("under", C.c_void_p),
        ("over", C.c_void_p),
        ("elapsed_ms", C.c_double),
        ("scratch_bytes", C.c_uint64),
    ]


MAX_SERIES_COMBINATIONS = 64   # AF_MAX_SERIES_COMBINATIONS
#: AF_COMBINE_*: the op of a combination across the series of one sample row
COMBINE_OPS = {"sum": 0, "min": 1, "max": 2, "spread": 3}


class AfSeriesCombined(C.Structure):
    """``af_series_combined_t``: request of ``af_engine_summarize_series_combined`` (``elapsed_ms`` and
    ``scratch_bytes`` are written back)."""

    _fields_ = [
        ("n_scenarios", C.c_uint32),
        ("n_groups", C.c_uint32),
        ("n_windows", C.c_uint32),
        ("group", C.c_void_p),
        ("tick_edges", C.POINTER(C.c_uint32)),
        ("n_combos", C.c_uint32),
        ("op", C.POINTER(C.c_uint32)),
        ("col_start", C.POINTER(C.c_uint32)),
        ("cols", C.POINTER(C.c_uint32)),
        ("thresholds", C.POINTER(C.c_double)),
        ("n_bins", C.c_uint32),
        ("lo", C.POINTER(C.c_double)),
        ("width", C.POINTER(C.c_double)),
        ("count", C.c_void_p),
        ("mean", C.c_void_p),
        ("minv", C.c_void_p),
        ("maxv", C.c_void_p),
        ("above", C.c_void_p),
        ("hist", C.c_void_p),
        ("under", C.c_void_p),
        ("over", C.c_void_p),
        ("elapsed_ms", C.c_double),
        ("scratch_bytes", C.c_uint64),
    ]


MAX_SERIES_PAIRS = 64   # AF_MAX_SERIES_PAIRS


class AfSeriesJoint(C.Structure):
    """``af_series_joint_t``: request of ``af_engine_summarize_series_joint`` (``elapsed_ms`` and ``scratch_bytes`` are
    written back)."""

    _fields_ = [
        ("n_scenarios", C.c_uint32),
        ("n_groups", C.c_uint32),
        ("n_windows", C.c_uint32),
        ("group", C.c_void_p),
        ("tick_edges", C.POINTER(C.c_uint32)),
        ("n_pairs", C.c_uint32),
        ("a", C.POINTER(C.c_uint32)),
        ("b", C.POINTER(C.c_uint32)),
        ("lag", C.POINTER(C.c_uint32)),
        ("n", C.c_void_p),
        ("sx", C.c_void_p),
        ("sy", C.c_void_p),
        ("sxx", C.c_void_p),
        ("syy", C.c_void_p),
        ("sxy", C.c_void_p),
        ("elapsed_ms", C.c_double),
        ("scratch_bytes", C.c_uint64),
    ]


MAX_SERIES_WARMUP_COLUMNS = 64   # AF_MAX_SERIES_WARMUP_COLUMNS


class AfSeriesWarmup(C.Structure):
    """``af_series_warmup_t``: request of ``af_engine_summarize_series_warmup`` (``elapsed_ms`` and ``scratch_bytes`` are
    written back)."""

    _fields_ = [
        ("n_scenarios", C.c_uint32),
        ("n_groups", C.c_uint32),
        ("n_windows", C.c_uint32),
        ("group", C.c_void_p),
        ("tick_edges", C.POINTER(C.c_uint32)),
        ("n_columns", C.c_uint32),
        ("columns", C.POINTER(C.c_uint32)),
        ("batch", C.c_uint32),
        ("batches", C.c_void_p),
        ("trunc", C.c_void_p),
        ("s1", C.c_void_p),
        ("s2", C.c_void_p),
        ("s1_all", C.c_void_p),
        ("s2_all", C.c_void_p),
        ("elapsed_ms", C.c_double),
        ("scratch_bytes", C.c_uint64),
    ]


class AfArrivals(C.Structure):
    """``af_arrivals_t``: request of ``af_engine_summarize_arrivals`` (``elapsed_ms`` and ``scratch_bytes`` are written
    back)."""

    _fields_ = [
        ("n_scenarios", C.c_uint32),
        ("n_groups", C.c_uint32),
        ("n_windows", C.c_uint32),
        ("group", C.c_void_p),
        ("edges", C.POINTER(C.c_double)),
        ("times", C.c_void_p),
        ("times_given", C.c_uint32),
        ("arrivals", C.c_void_p),
        ("row_bounds", C.c_void_p),
        ("generated", C.c_void_p),
        ("flags", C.c_void_p),
        ("elapsed_ms", C.c_double),
        ("scratch_bytes", C.c_uint64),
    ]


class AfInflight(C.Structure):
    """``af_inflight_t``: request of ``af_engine_summarize_inflight`` (``elapsed_ms`` and ``scratch_bytes`` are written
    back)."""

    _fields_ = [
        ("n_scenarios", C.c_uint32),
        ("n_groups", C.c_uint32),
        ("n_windows", C.c_uint32),
        ("group", C.c_void_p),
        ("tick_edges", C.POINTER(C.c_uint32)),
        ("sample_period", C.c_double),
        ("threshold", C.c_uint32),
        ("n_bins", C.c_uint32),
        ("lo", C.c_uint32),
        ("count", C.c_void_p),
        ("sum", C.c_void_p),
        ("minv", C.c_void_p),
        ("maxv", C.c_void_p),
        ("above", C.c_void_p),
        ("hist", C.c_void_p),
        ("under", C.c_void_p),
        ("in_flight", C.c_void_p),
        ("started", C.c_void_p),
        ("finished", C.c_void_p),
        ("elapsed_ms", C.c_double),
        ("scratch_bytes", C.c_uint64),
    ]


class AfExemplars(C.Structure):
    """``af_exemplars_t``: request of ``af_engine_summarize_exemplars`` (``elapsed_ms`` and ``scratch_bytes`` are written
    back)."""

    _fields_ = [
        ("n_scenarios", C.c_uint32),
        ("n_groups", C.c_uint32),
        ("n_windows", C.c_uint32),
        ("group", C.c_void_p),
        ("edges", C.POINTER(C.c_double)),
        ("by_arrival", C.c_uint32),
        ("k", C.c_uint32),
        ("sample_period", C.c_double),
        ("total", C.c_void_p),
        ("kept", C.c_void_p),
        ("scenario", C.c_void_p),
        ("row", C.c_void_p),
        ("clock", C.c_void_p),
        ("state", C.c_void_p),
        ("elapsed_ms", C.c_double),
        ("scratch_bytes", C.c_uint64),
    ]


class AfLatencyHistogram(C.Structure):
    """``af_latency_histogram_t``: request of ``af_engine_summarize_latency_histogram`` (``elapsed_ms`` and ``scratch_bytes``
    are written back)."""

    _fields_ = [
        ("n_scenarios", C.c_uint32),
        ("n_groups", C.c_uint32),
        ("n_windows", C.c_uint32),
        ("group", C.c_void_p),
        ("edges", C.POINTER(C.c_double)),
        ("by_arrival", C.c_uint32),
        ("sub_bits", C.c_uint32),
        ("min_exp", C.c_int32),
        ("octaves", C.c_uint32),
        ("count", C.c_void_p),
        ("hist", C.c_void_p),
        ("under", C.c_void_p),
        ("over", C.c_void_p),
        ("nan", C.c_void_p),
        ("elapsed_ms", C.c_double),
        ("scratch_bytes", C.c_uint64),
    ]


MAX_PAIR_THRESHOLDS = 64   # AF_MAX_PAIR_THRESHOLDS
PAIR_NONE = 0xFFFFFFFF     # AF_PAIR_NONE: af_pairs_t.row_a / row_b of an arrival without a row


class AfPairs(C.Structure):
    """``af_pairs_t``: request of ``af_engine_summarize_pairs`` (``elapsed_ms`` and ``scratch_bytes`` are written back)."""

    _fields_ = [
        ("n_scenarios", C.c_uint32),
        ("n_pairs", C.c_uint32),
        ("n_groups", C.c_uint32),
        ("n_windows", C.c_uint32),
        ("pair_a", C.c_void_p),
        ("pair_b", C.c_void_p),
        ("group", C.c_void_p),
        ("edges", C.POINTER(C.c_double)),
        ("times", C.c_void_p),
        ("time_row", C.c_void_p),
        ("n_time_rows", C.c_uint32),
        ("draw_capacity", C.c_uint32),
        ("thresholds", C.POINTER(C.c_double)),
        ("n_thresholds", C.c_uint32),
        ("sub_bits", C.c_uint32),
        ("min_exp", C.c_int32),
        ("octaves", C.c_uint32),
        ("pair_counts", C.c_void_p),
        ("pair_sums", C.c_void_p),
        ("unmatched", C.c_void_p),
        ("cell_counts", C.c_void_p),
        ("above", C.c_void_p),
        ("extremes", C.c_void_p),
        ("hist", C.c_void_p),
        ("tails", C.c_void_p),
        ("row_a", C.c_void_p),
        ("row_b", C.c_void_p),
        ("elapsed_ms", C.c_double),
        ("scratch_bytes", C.c_uint64),
    ]


MAX_ALERT_RULES = 32   # AF_MAX_ALERT_RULES


class AfAlertRule(C.Structure):
    """``af_alert_rule_t``: one burn-rate rule of ``af_engine_summarize_alerts``, in ticks and as the fraction ``num / den``."""

    _fields_ = [
        ("long_ticks", C.c_uint32),
        ("short_ticks", C.c_uint32),
        ("num", C.c_uint32),
        ("den", C.c_uint32),
        ("min_total", C.c_uint32),
        ("hold_ticks", C.c_uint32),
    ]


class AfAlerts(C.Structure):
    """``af_alerts_t``: request of ``af_engine_summarize_alerts`` (``elapsed_ms`` and ``scratch_bytes`` are written back)."""

    _fields_ = [
        ("n_scenarios", C.c_uint32),
        ("n_groups", C.c_uint32),
        ("n_windows", C.c_uint32),
        ("n_rules", C.c_uint32),
        ("group", C.c_void_p),
        ("tick_edges", C.POINTER(C.c_uint32)),
        ("rules", C.POINTER(AfAlertRule)),
        ("sample_period", C.c_double),
        ("slo", C.c_double),
        ("n_bins", C.c_uint32),
        ("delay_width", C.c_uint32),
        ("count", C.c_void_p),
        ("fired", C.c_void_p),
        ("episodes", C.c_void_p),
        ("longest", C.c_void_p),
        ("longest_start", C.c_void_p),
        ("first", C.c_void_p),
        ("last", C.c_void_p),
        ("members", C.c_void_p),
        ("fired_members", C.c_void_p),
        ("open_members", C.c_void_p),
        ("fire_ticks", C.c_void_p),
        ("fire_episodes", C.c_void_p),
        ("delay_hist", C.c_void_p),
        ("total", C.c_void_p),
        ("bad", C.c_void_p),
        ("firing", C.c_void_p),
        ("elapsed_ms", C.c_double),
        ("scratch_bytes", C.c_uint64),
    ]


OUTCOME_ROWS_TRUNCATED = 1   # AF_OUTCOME_ROWS_TRUNCATED
OUTCOME_DEFICIT = 2          # AF_OUTCOME_DEFICIT


class AfAlertOutcomes(C.Structure):
    """``af_alert_outcomes_t``: the arrival rows, the client timeout and the outcome outputs of
    ``af_engine_outcome_alerts``."""

    _fields_ = [
        ("times", C.c_void_p),
        ("time_row", C.c_void_p),
        ("n_time_rows", C.c_uint32),
        ("draw_capacity", C.c_uint32),
        ("timeout", C.c_double),
        ("timeouts", C.c_void_p),
        ("timed_out", C.c_void_p),
        ("deficit", C.c_void_p),
        ("flags", C.c_void_p),
    ]


class AfStateBins(C.Structure):
    """``af_state_bins_t``: the series, its binning and the sample period of ``af_engine_summarize_state_windows`` /
    ``af_engine_summarize_state_quantiles``."""

    _fields_ = [
        ("column", C.c_uint32),
        ("n_bins", C.c_uint32),
        ("lo", C.c_double),
        ("width", C.c_double),
        ("sample_period", C.c_double),
    ]


#: every symbol include/asyncflow_hip.h declares
EXPORTED_SYMBOLS = (
    "af_engine_create",
    "af_engine_run",
    "af_engine_summarize",
    "af_engine_summarize_pooled",
    "af_engine_summarize_windows",
    "af_engine_summarize_arrival_windows",
    "af_engine_summarize_series_windows",
    "af_engine_summarize_series_quantiles",
    "af_engine_summarize_series_excursions",
    "af_engine_summarize_series_histogram",
    "af_engine_summarize_series_combined",
    "af_engine_summarize_series_joint",
    "af_engine_summarize_series_warmup",
    "af_engine_summarize_quantiles",
    "af_engine_summarize_arrival_quantiles",
    "af_engine_export_cells",
    "af_engine_import_cells",
    "af_engine_summarize_arrivals",
    "af_engine_summarize_inflight",
    "af_engine_summarize_exemplars",
    "af_engine_summarize_latency_histogram",
    "af_engine_summarize_pairs",
    "af_engine_summarize_alerts",
    "af_engine_outcome_alerts",
    "af_engine_summarize_state_windows",
    "af_engine_summarize_state_quantiles",
    "af_engine_run_summarized",
    "af_engine_jit_spec",
    "af_engine_set_kernels",
    "af_engine_stats",
    "af_engine_flow_reason",
    "af_engine_gather",
    "af_comm_load",
    "af_comm_unique_id",
    "af_comm_init_rank",
    "af_comm_destroy",
    "af_comm_count",
    "af_engine_destroy",
    "af_tick_count",
    "af_series_count",
    "af_series_pitch",
    "af_last_error",
    "af_abi_version",
    "af_probe_math",
    "af_probe_store",
    "af_probe_scratch",
)


def declare(lib: C.CDLL) -> C.CDLL:
    """Attach argtypes/restypes of the C ABI to a loaded library."""
    lib.af_engine_create.argtypes = [
        C.POINTER(AfPlan), C.c_int, C.POINTER(AfEngineOptions), C.POINTER(C.c_void_p),
    ]
    lib.af_engine_create.restype = C.c_int
    lib.af_engine_run.argtypes = [C.c_void_p, C.POINTER(AfSweep), C.POINTER(AfOutputs)]
    lib.af_engine_run.restype = C.c_int
    lib.af_engine_summarize.argtypes = [C.c_void_p, C.POINTER(AfOutputs), C.POINTER(AfSummary)]
    lib.af_engine_summarize.restype = C.c_int
    lib.af_engine_summarize_pooled.argtypes = [C.c_void_p, C.POINTER(AfOutputs), C.POINTER(AfPooled)]
    lib.af_engine_summarize_pooled.restype = C.c_int
    lib.af_engine_summarize_windows.argtypes = [C.c_void_p, C.POINTER(AfOutputs), C.POINTER(AfWindows)]
    lib.af_engine_summarize_windows.restype = C.c_int
    lib.af_engine_summarize_arrival_windows.argtypes = [C.c_void_p, C.POINTER(AfOutputs), C.POINTER(AfWindows)]
    lib.af_engine_summarize_arrival_windows.restype = C.c_int
    lib.af_engine_summarize_series_windows.argtypes = [C.c_void_p, C.POINTER(AfOutputs), C.POINTER(AfSeriesWindows)]
    lib.af_engine_summarize_series_windows.restype = C.c_int
    lib.af_engine_summarize_series_quantiles.argtypes = [C.c_void_p, C.POINTER(AfOutputs), C.POINTER(AfSeriesQuantiles)]
    lib.af_engine_summarize_series_quantiles.restype = C.c_int
    lib.af_engine_summarize_series_excursions.argtypes = [C.c_void_p, C.POINTER(AfOutputs), C.POINTER(AfSeriesExcursions)]
    lib.af_engine_summarize_series_excursions.restype = C.c_int
    lib.af_engine_summarize_series_histogram.argtypes = [C.c_void_p, C.POINTER(AfOutputs), C.POINTER(AfSeriesHistogram)]
    lib.af_engine_summarize_series_histogram.restype = C.c_int
    lib.af_engine_summarize_series_combined.argtypes = [C.c_void_p, C.POINTER(AfOutputs), C.POINTER(AfSeriesCombined)]
    lib.af_engine_summarize_series_combined.restype = C.c_int
    lib.af_engine_summarize_series_joint.argtypes = [C.c_void_p, C.POINTER(AfOutputs), C.POINTER(AfSeriesJoint)]
    lib.af_engine_summarize_series_joint.restype = C.c_int
    lib.af_engine_summarize_series_warmup.argtypes = [C.c_void_p, C.POINTER(AfOutputs), C.POINTER(AfSeriesWarmup)]
    lib.af_engine_summarize_series_warmup.restype = C.c_int
    lib.af_engine_summarize_quantiles.argtypes = [C.c_void_p, C.POINTER(AfOutputs), C.POINTER(AfQuantiles)]
    lib.af_engine_summarize_quantiles.restype = C.c_int
    lib.af_engine_summarize_arrival_quantiles.argtypes = [C.c_void_p, C.POINTER(AfOutputs), C.POINTER(AfQuantiles)]
    lib.af_engine_summarize_arrival_quantiles.restype = C.c_int
    lib.af_engine_export_cells.argtypes = [C.c_void_p, C.POINTER(AfOutputs), C.POINTER(AfCellsExport)]
    lib.af_engine_export_cells.restype = C.c_int
    lib.af_engine_import_cells.argtypes = [C.c_void_p, C.POINTER(AfCells)]
    lib.af_engine_import_cells.restype = C.c_int
    lib.af_engine_summarize_arrivals.argtypes = [C.c_void_p, C.POINTER(AfSweep), C.POINTER(AfArrivals)]
    lib.af_engine_summarize_arrivals.restype = C.c_int
    lib.af_engine_summarize_inflight.argtypes = [C.c_void_p, C.POINTER(AfOutputs), C.POINTER(AfInflight)]
    lib.af_engine_summarize_inflight.restype = C.c_int
    lib.af_engine_summarize_exemplars.argtypes = [C.c_void_p, C.POINTER(AfOutputs), C.POINTER(AfExemplars)]
    lib.af_engine_summarize_exemplars.restype = C.c_int
    lib.af_engine_summarize_latency_histogram.argtypes = [C.c_void_p, C.POINTER(AfOutputs), C.POINTER(AfLatencyHistogram)]
    lib.af_engine_summarize_latency_histogram.restype = C.c_int
    lib.af_engine_summarize_pairs.argtypes = [C.c_void_p, C.POINTER(AfOutputs), C.POINTER(AfPairs)]
    lib.af_engine_summarize_pairs.restype = C.c_int
    lib.af_engine_summarize_alerts.argtypes = [C.c_void_p, C.POINTER(AfOutputs), C.POINTER(AfAlerts)]
    lib.af_engine_summarize_alerts.restype = C.c_int
    lib.af_engine_outcome_alerts.argtypes = [C.c_void_p, C.POINTER(AfOutputs), C.POINTER(AfAlertOutcomes), C.POINTER(AfAlerts)]
    lib.af_engine_outcome_alerts.restype = C.c_int
    lib.af_engine_summarize_state_windows.argtypes = [C.c_void_p, C.POINTER(AfOutputs), C.POINTER(AfStateBins), C.POINTER(AfWindows)]
    lib.af_engine_summarize_state_windows.restype = C.c_int
    lib.af_engine_summarize_state_quantiles.argtypes = [C.c_void_p, C.POINTER(AfOutputs), C.POINTER(AfStateBins), C.POINTER(AfQuantiles)]
    lib.af_engine_summarize_state_quantiles.restype = C.c_int
    lib.af_engine_run_summarized.argtypes = [C.c_void_p, C.POINTER(AfSweep), C.POINTER(AfOutputs), C.POINTER(AfSummary)]
    lib.af_engine_run_summarized.restype = C.c_int
    lib.af_engine_jit_spec.argtypes = [C.c_void_p, C.POINTER(AfSweep), C.POINTER(AfOutputs), C.c_char_p, C.c_size_t]
    lib.af_engine_jit_spec.restype = C.c_int
    lib.af_engine_set_kernels.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t]
    lib.af_engine_set_kernels.restype = C.c_int
    lib.af_engine_stats.argtypes = [C.c_void_p, C.POINTER(AfStats)]
    lib.af_engine_stats.restype = C.c_int
    lib.af_engine_flow_reason.argtypes = [C.c_void_p]
    lib.af_engine_flow_reason.restype = C.c_char_p
    lib.af_engine_gather.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(AfSummary), C.POINTER(AfSummary)]
    lib.af_engine_gather.restype = C.c_int
    lib.af_comm_load.argtypes = [C.c_char_p]
    lib.af_comm_load.restype = C.c_int
    lib.af_comm_unique_id.argtypes = [C.c_void_p]
    lib.af_comm_unique_id.restype = C.c_int
    lib.af_comm_init_rank.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    lib.af_comm_init_rank.restype = C.c_int
    lib.af_comm_destroy.argtypes = [C.c_void_p]
    lib.af_comm_destroy.restype = None
    lib.af_comm_count.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.af_comm_count.restype = C.c_int
    lib.af_engine_destroy.argtypes = [C.c_void_p]
    lib.af_engine_destroy.restype = None
    lib.af_tick_count.argtypes = [C.c_double, C.c_double]
    lib.af_tick_count.restype = C.c_uint32
    lib.af_series_count.argtypes = [C.POINTER(AfPlan)]
    lib.af_series_count.restype = C.c_uint32
    lib.af_series_pitch.argtypes = [C.POINTER(AfPlan)]
    lib.af_series_pitch.restype = C.c_uint32
    lib.af_last_error.argtypes = []
    lib.af_last_error.restype = C.c_char_p
    lib.af_abi_version.argtypes = []
    lib.af_abi_version.restype = C.c_int
    lib.af_probe_math.argtypes = [C.c_int, C.c_int, C.c_uint64, _pd, _pd, _pd, C.c_size_t]
    lib.af_probe_math.restype = C.c_int
    lib.af_probe_store.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(C.c_double)]
    lib.af_probe_store.restype = C.c_int
    lib.af_probe_scratch.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32]
    lib.af_probe_scratch.restype = C.c_int
    return lib
