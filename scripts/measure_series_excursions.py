"""Excursions of the sampled series above a threshold on BASELINE config 2's batch (10 000 LB-2 replicas, T = 600 s): one
JSON line.

    python scripts/measure_series_excursions.py [--replicas 10000] [--reps 5]

Cases: one window over the whole run, 60 windows of 10 s, 600 windows of 1 s; every scenario its own cells, all eight outputs,
a threshold of 0.5 on the integer series and of 64 MB on ram_in_use.  Each case ALTERNATES in the same process with the
yardstick: `af_engine_summarize_series_windows` over the same cells with singleton groups and the same thresholds (its
kernel reads the same sample rows once and is unchanged by the excursions).  Every figure is the host's wall time around the
synchronous engine call (uploads, the kernel, the synchronisation) as min / median / max over --reps calls after one warm-up
call of each; `scratch_bytes` is the engine's scratch after the case's first call on a fresh engine; `tb_s` the stored sample
rows' bytes (pitch * 4 B per tick) per median time; `out_bytes` what the call writes into its outputs; `above_share` the
share of the (tick, series) values above their threshold (a step of a wave in which no value is above skips the run
bookkeeping).
"""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()

    import torch

    from asyncflow_amd import _abi
    from asyncflow_amd.engine import Engine
    from asyncflow_amd.results import ram_columns, tick_window_edges, ticks_per_window_of
    from asyncflow_amd.runner import SimulationRunner
    from asyncflow_amd.workloads import lb_two_servers

    res = SimulationRunner(simulation_input=lb_two_servers(), replicas=args.replicas, collect_clock=False).run()
    n, plan = len(res), res.plan
    samples, counts = res._samples_t, res._counts_t   # noqa: SLF001
    dev = samples.device
    cap, S = int(samples.shape[1]), plan.n_series
    ticks = np.minimum(res.counts[:, _abi.CNT_TICKS].astype(np.int64), cap)
    sample_bytes = 4.0 * plan.series_pitch * float(ticks.sum())
    thr = np.where(ram_columns(S, plan.n_edges), 64.0, 0.5)

    def spread(ms: list[float]) -> dict:
        return {"min_ms": float(np.min(ms)), "median_ms": float(np.median(ms)), "max_ms": float(np.max(ms)),
                "tb_s": sample_bytes / (float(np.median(ms)) * 1e-3) / 1e12}

    out: dict = {"replicas": n, "ticks": float(ticks.sum()), "sample_gb": sample_bytes / 1e9, "series": S, "reps": args.reps}
    grp = torch.arange(n, dtype=torch.int32, device=dev)
    cases = [("x1", np.array([0, cap])),
             ("x60", tick_window_edges(ticks_per_window_of(10.0, plan.sample_period), cap)),
             ("x600", tick_window_edges(ticks_per_window_of(1.0, plan.sample_period), cap))]
    for name, edges in cases:
        W = len(edges) - 1
        y_count = torch.empty((n, W), dtype=torch.int32, device=dev)
        y_mean = torch.empty((n, W, S), dtype=torch.float64, device=dev)
        y_min, y_max, y_above = (torch.empty((n, W, S), dtype=torch.int32, device=dev) for _ in range(3))
        raw = {k: torch.empty((n, W) if k == "count" else (n, W, S), dtype=torch.int32, device=dev) for k in Engine.EXCURSION_OUTPUTS}
        eng = Engine(plan, dev.index or 0)                    # a fresh engine: this case's own scratch

        def yardstick() -> float:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            eng.summarize_series_windows(
                n, n, edges, samples_ptr=samples.data_ptr(), tick_capacity=cap, counts_ptr=counts.data_ptr(),
                count_ptr=y_count.data_ptr(), mean_ptr=y_mean.data_ptr(), min_ptr=y_min.data_ptr(), max_ptr=y_max.data_ptr(),
                above_ptr=y_above.data_ptr(), group_ptr=grp.data_ptr(), thresholds=thr)
            return (time.perf_counter() - t0) * 1e3

        def excursions() -> tuple[float, float, int]:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            ms, scratch = eng.summarize_series_excursions(
                n, edges, samples_ptr=samples.data_ptr(), tick_capacity=cap, counts_ptr=counts.data_ptr(), thresholds=thr,
                **{f"{k}_ptr": v.data_ptr() for k, v in raw.items()})
            return (time.perf_counter() - t0) * 1e3, ms, scratch

        first_ms, _, scratch = excursions()
        yardstick()
        yard, exc, inner = [], [], []
        for _ in range(args.reps):
            yard.append(yardstick())
            x_ms, e_ms, _ = excursions()
            exc.append(x_ms)
            inner.append(e_ms)
        assert int((raw["count"].to(torch.int64) & 0xFFFFFFFF).sum()) == int(ticks.sum())
        assert torch.equal(raw["above"], y_above) and torch.equal(raw["count"], y_count)
        above = int((raw["above"].to(torch.int64) & 0xFFFFFFFF).sum())
        out[name] = {"yardstick": spread(yard), "series_excursions": spread(exc), "elapsed_ms_median": float(np.median(inner)),
                     "vs_yardstick": float(np.median(exc) / np.median(yard)), "first_call_ms": first_ms, "scratch_bytes": scratch,
                     "cells": n * W, "out_bytes": n * W * (4 + 28 * S), "yardstick_out_bytes": n * W * (4 + 20 * S),
                     "above_share": above / (float(ticks.sum()) * S), "runs": int((raw["runs"].to(torch.int64) & 0xFFFFFFFF).sum())}
        eng.close()
        del y_count, y_mean, y_min, y_max, y_above, raw
    print(json.dumps(out))


if __name__ == "__main__":
    main()
