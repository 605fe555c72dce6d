"""asyncflow_amd -- MI355X-native batched discrete-event engine for AsyncFlow scenarios.

Drop-in for ONE hot path of AsyncFlow: ``SimulationRunner.run()`` ->
``env.run(until=T)`` (/root/reference/src/asyncflow/runtime/simulation_runner.py:349-376),
executed over thousands of independent scenarios by a hand-written HIP kernel
(gfx950).  See DESIGN.md and INTEGRATION.md.
"""

from .payload import load_yaml, normalize_payload
from .plan import DevicePlan, lower
from .results import BatchedResults, ScenarioResults, alert_cells, alert_delay_quantiles, alert_firing, alert_rule, alert_window_stats, autocorrelation_time, check_latency_bins, check_series_combinations, check_series_pairs, check_warmup_batch, completion_ticks, in_flight_series, outcome_ticks, scenario_outcome_alerts, in_flight_window_stats, latency_bin_edges, latency_bin_index, latency_exemplars, latency_histogram, latency_histogram_distance, latency_histogram_merge, latency_histogram_quantiles, latency_histogram_regroup, latency_pair_cells, latency_pairs, latency_quantiles, latency_state_cells, latency_state_quantiles, latency_state_stats, latency_window_quantiles, latency_window_stats, paired_delta_quantiles, paired_fixed_sum, paired_merge, series_combined_values, series_combined_window_stats, series_histogram_quantiles, series_joint_statistics, series_joint_sums, series_warmup_cut, series_warmup_statistics, series_warmup_sums, series_window_excursions, series_window_histogram, series_window_quantiles, window_edges
from .runner import SimulationRunner
from .sweep import Sweep, expand_grid

__all__ = [
    "BatchedResults",
    "DevicePlan",
    "ScenarioResults",
    "SimulationRunner",
    "Sweep",
    "alert_cells",
    "alert_delay_quantiles",
    "alert_firing",
    "alert_rule",
    "alert_window_stats",
    "autocorrelation_time",
    "check_latency_bins",
    "check_series_combinations",
    "check_series_pairs",
    "check_warmup_batch",
    "completion_ticks",
    "outcome_ticks",
    "scenario_outcome_alerts",
    "expand_grid",
    "in_flight_series",
    "in_flight_window_stats",
    "latency_bin_edges",
    "latency_bin_index",
    "latency_exemplars",
    "latency_histogram",
    "latency_histogram_distance",
    "latency_histogram_merge",
    "latency_histogram_quantiles",
    "latency_histogram_regroup",
    "latency_pair_cells",
    "latency_pairs",
    "latency_quantiles",
    "latency_state_cells",
    "latency_state_quantiles",
    "latency_state_stats",
    "latency_window_quantiles",
    "latency_window_stats",
    "load_yaml",
    "lower",
    "normalize_payload",
    "paired_delta_quantiles",
    "paired_fixed_sum",
    "paired_merge",
    "series_combined_values",
    "series_combined_window_stats",
    "series_histogram_quantiles",
    "series_joint_statistics",
    "series_joint_sums",
    "series_warmup_cut",
    "series_warmup_statistics",
    "series_warmup_sums",
    "series_window_excursions",
    "series_window_histogram",
    "series_window_quantiles",
    "window_edges",
]

__version__ = "0.1.0"
