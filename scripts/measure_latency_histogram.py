"""Log-linear latency histograms per window and group on BASELINE config 2's batch (10 000 LB-2 replicas, T = 600 s): one JSON line.

    python scripts/measure_latency_histogram.py [--replicas 10000] [--reps 3] [--no-yardstick]

Every case ALTERNATES, in the same process, `af_engine_summarize_latency_histogram` with two yardsticks over the same windows and
groups, neither of them the code under test:
  (a) `af_engine_summarize_inflight` (count, sum, min, max, above): one pass over the same clock rows -- the model is that the new
      call lies near it;
  (b) `af_engine_summarize_quantiles` with 64 thresholds (`af_engine_summarize_arrival_quantiles` by arrival): what gives a
      distribution per cell today.  The expectation, not a gate: the new call is not above (b) in any row (`met`).
Cases: one window / 60 windows of 10 s / 600 windows of 1 s, each with one group / 100 groups / singleton groups, by finish and by
arrival, at the default binning (1 024 bins) and at 4 096 bins.  Singletons x 600 windows would need 6.1e9 (2.5e10) histogram words,
past the 2^32 of the capacity rule: those cases run with 64 bins (sub_bits 1, 32 octaves) and say so (`bins`).  Every figure is
the wall time of the synchronous engine call (read-backs, host checks, the zeroing of the outputs, the kernel), started after a
device synchronisation, as min / median / max over --reps calls after one warm-up call of each.  `pass_tb_s` is the clock rows'
bytes per median call time, `zeroed_gb` the outputs the call clears first.  --no-yardstick repeats the call back to back.
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-yardstick", action="store_true", help="do not alternate with the in-flight and the quantile analyzer")
    args = ap.parse_args()

    import torch

    from asyncflow_amd import _abi
    from asyncflow_amd.results import tick_window_edges
    from asyncflow_amd.runner import SimulationRunner
    from asyncflow_amd.workloads import lb_two_servers

    res = SimulationRunner(simulation_input=lb_two_servers(), replicas=args.replicas).run()
    n, plan = len(res), res.plan
    p, ticks = float(plan.sample_period), int(plan.tick_count)
    clock, counts = res._clock_t, res._counts_t   # noqa: SLF001
    dev = clock.device
    clock_bytes = 16.0 * float(np.minimum(res.counts[:, _abi.CNT_COMPLETED].astype(np.int64), clock.shape[1]).sum())
    tick_cap = res._in_flight_ticks()   # noqa: SLF001
    eng, _ = res._arrival_engine()   # noqa: SLF001
    thresholds = np.geomspace(1e-3, 10.0, 64)

    def spread(ms: list[float]) -> dict:
        return {"min_ms": float(np.min(ms)), "median_ms": float(np.median(ms)), "max_ms": float(np.max(ms))}

    out: dict = {"replicas": n, "latencies": clock_bytes / 16.0, "clock_gb": clock_bytes / 1e9, "reps": args.reps}
    per = max(n // 100, 1)
    groupings = (("one_group", np.zeros(n, dtype=np.int64), 1), ("groups_100", np.arange(n) // per, int((n - 1) // per) + 1),
                 ("singletons", np.arange(n), n))
    windows = (("x1", np.array([0, tick_cap], dtype=np.uint32)), ("x60", tick_window_edges(round(10.0 / p), ticks)),
               ("x600", tick_window_edges(round(1.0 / p), ticks)))
    for wname, b in windows:
        n_win = int(b.shape[0] - 1)
        edges_s = b.astype(np.float64) * p
        for gname, ids, n_groups in groupings:
            grp = torch.from_numpy(ids.astype(np.uint32).view(np.int32)).to(dev)
            cells = n_groups * n_win
            small = [torch.empty((n_groups, n_win), dtype=torch.int32, device=dev) for _ in range(4)]
            total = torch.empty((n_groups, n_win), dtype=torch.int64, device=dev)
            count = torch.empty((n_groups, n_win), dtype=torch.int64, device=dev)

            def inflight() -> float:
                if args.no_yardstick:
                    return float("nan")
                torch.cuda.synchronize(dev)
                ms, _ = eng.summarize_inflight(n, n_groups, b, p, clock_ptr=clock.data_ptr(), clock_capacity=int(clock.shape[1]),   # noqa: B023
                                               tick_capacity=tick_cap, counts_ptr=counts.data_ptr(), count_ptr=small[0].data_ptr(),   # noqa: B023
                                               sum_ptr=total.data_ptr(), min_ptr=small[1].data_ptr(), max_ptr=small[2].data_ptr(),   # noqa: B023
                                               above_ptr=small[3].data_ptr(), group_ptr=grp.data_ptr())   # noqa: B023
                return float(ms)

            for window_of in ("finish", "arrival"):

                def quantiles() -> float:
                    if args.no_yardstick:
                        return float("nan")
                    torch.cuda.synchronize(dev)
                    return float(res.quantile_summary([], thresholds=thresholds, edges=edges_s, by=ids, window_of=window_of)["quantile_ms"])   # noqa: B023

                for label, binning in (("default", (5, -20, 32)), ("bins_4096", (7, -20, 32))):
                    if cells * (binning[2] << binning[0]) >= 2 ** 32:
                        binning = (1, -20, 32)                # the capacity rule: fewer bins
                    n_bins = binning[2] << binning[0]
                    hist = torch.empty((n_groups, n_win, n_bins), dtype=torch.int32, device=dev)
                    rest = torch.empty((3, n_groups, n_win), dtype=torch.int32, device=dev)

                    def histogram() -> float:
                        torch.cuda.synchronize(dev)           # nothing of the call before is still running
                        ms, _ = eng.summarize_latency_histogram(
                            n, n_groups, edges=edges_s, window_of=window_of, sub_bits=binning[0], min_exp=binning[1], octaves=binning[2],   # noqa: B023
                            clock_ptr=clock.data_ptr(), clock_capacity=int(clock.shape[1]), counts_ptr=counts.data_ptr(),
                            count_ptr=count.data_ptr(), hist_ptr=hist.data_ptr(), under_ptr=rest[0].data_ptr(),   # noqa: B023
                            over_ptr=rest[1].data_ptr(), nan_ptr=rest[2].data_ptr(), group_ptr=grp.data_ptr())   # noqa: B023
                        return float(ms)

                    histogram()
                    inflight()
                    quantiles()
                    mine, ya, yb = [], [], []
                    for _ in range(args.reps):
                        mine.append(histogram())
                        ya.append(inflight())
                        yb.append(quantiles())
                    med = float(np.median(mine))
                    rows = int(count.sum().item())
                    inside = int((hist.to(torch.int64) & 0xFFFFFFFF).sum().item())
                    out[f"{gname}_{wname}_{window_of}_{label}"] = {
                        "histogram": spread(mine), "inflight": spread(ya), "quantiles_64": spread(yb), "bins": n_bins, "cells": cells,
                        "ratio_inflight": med / float(np.median(ya)), "ratio_quantiles": med / float(np.median(yb)),
                        "met": bool(med <= float(np.median(yb))) if not args.no_yardstick else None,
                        "pass_tb_s": clock_bytes / (med * 1e-3) / 1e12, "zeroed_gb": 4.0 * cells * (n_bins + 5) / 1e9,
                        "rows": rows, "binned_share": inside / max(rows, 1)}
                    del hist, rest
            del small, total, count, grp
    print(json.dumps(out))


if __name__ == "__main__":
    main()
