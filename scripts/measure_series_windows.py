"""Sampled-series analyzer per (group, window of ticks) on BASELINE config 2's batch (10 000 LB-2 replicas, T = 600 s): one
JSON line.

    python scripts/measure_series_windows.py [--replicas 10000] [--reps 5]

Cases: one window over the whole run with one group / 100 groups / singletons; 60 windows of 10 s with 100 groups /
singletons; 600 windows of 1 s with singletons.  Each case ALTERNATES in the same process with the yardstick:
`af_engine_summarize` asked for `series_mean` and `series_max` only (af_series_kernel, which reads the same sample rows
once).  Every figure is the host's wall time around the synchronous engine call (read-backs, host layout, all kernels) as
min / median / max over --reps calls after one warm-up call of each; `scratch_bytes` is the engine's scratch after the case's
first call on a fresh engine; `tb_s` the stored sample rows' bytes (pitch * 4 B per tick) per median time; `out_bytes` what
the call writes into its outputs.
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
    from asyncflow_amd.results import tick_window_edges, ticks_per_window_of
    from asyncflow_amd.runner import SimulationRunner
    from asyncflow_amd.workloads import lb_two_servers

    res = SimulationRunner(simulation_input=lb_two_servers(), replicas=args.replicas, collect_clock=False).run()
    n, plan = len(res), res.plan
    samples, counts = res._samples_t, res._counts_t   # noqa: SLF001
    dev = samples.device
    cap, S = int(samples.shape[1]), plan.n_series
    ticks = np.minimum(res.counts[:, _abi.CNT_TICKS].astype(np.int64), cap)
    sample_bytes = 4.0 * plan.series_pitch * float(ticks.sum())

    def spread(ms: list[float]) -> dict:
        return {"min_ms": float(np.min(ms)), "median_ms": float(np.median(ms)), "max_ms": float(np.max(ms)),
                "tb_s": sample_bytes / (float(np.median(ms)) * 1e-3) / 1e12}

    smean = torch.empty((n, S), dtype=torch.float64, device=dev)
    smax = torch.empty((n, S), dtype=torch.int32, device=dev)

    def yardstick(eng: Engine) -> float:
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        eng.summarize(n, clock_ptr=0, clock_capacity=0, samples_ptr=samples.data_ptr(), tick_capacity=cap,
                      counts_ptr=counts.data_ptr(), series_mean_ptr=smean.data_ptr(), series_max_ptr=smax.data_ptr())
        return (time.perf_counter() - t0) * 1e3

    out: dict = {"replicas": n, "ticks": float(ticks.sum()), "sample_gb": sample_bytes / 1e9, "series": S, "reps": args.reps}
    ids100 = np.arange(n) // max(n // 100, 1)
    groupings = {"one_group": np.zeros(n, dtype=np.int64), "groups_100": ids100, "singletons": np.arange(n)}
    whole = np.array([0, cap])
    cases = [(f"{g}_x1", g, whole) for g in groupings]
    cases += [("groups_100_x60", "groups_100", tick_window_edges(ticks_per_window_of(10.0, plan.sample_period), cap)),
              ("singletons_x60", "singletons", tick_window_edges(ticks_per_window_of(10.0, plan.sample_period), cap)),
              ("singletons_x600", "singletons", tick_window_edges(ticks_per_window_of(1.0, plan.sample_period), cap))]
    for name, gname, edges in cases:
        ids = groupings[gname]
        G, W = int(ids.max()) + 1, len(edges) - 1
        grp = torch.as_tensor(ids.astype(np.uint32).view(np.int32), device=dev)
        count = torch.empty((G, W), dtype=torch.int32, device=dev)
        mean = torch.empty((G, W, S), dtype=torch.float64, device=dev)
        mn, mx, ab = (torch.empty((G, W, S), dtype=torch.int32, device=dev) for _ in range(3))
        eng = Engine(plan, dev.index or 0)                    # a fresh engine: this case's own scratch

        def windows() -> tuple[float, float, int]:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            ms, scratch = eng.summarize_series_windows(
                n, G, edges, samples_ptr=samples.data_ptr(), tick_capacity=cap, counts_ptr=counts.data_ptr(),
                count_ptr=count.data_ptr(), mean_ptr=mean.data_ptr(), min_ptr=mn.data_ptr(), max_ptr=mx.data_ptr(),
                above_ptr=ab.data_ptr(), group_ptr=grp.data_ptr())
            return (time.perf_counter() - t0) * 1e3, ms, scratch

        first_ms, _, scratch = windows()
        yardstick(eng)
        yard, win, inner = [], [], []
        for _ in range(args.reps):
            yard.append(yardstick(eng))
            w_ms, e_ms, _ = windows()
            win.append(w_ms)
            inner.append(e_ms)
        assert int((count.to(torch.int64) & 0xFFFFFFFF).sum()) == int(ticks.sum())
        out[name] = {"yardstick": spread(yard), "series_windows": spread(win), "elapsed_ms_median": float(np.median(inner)),
                     "vs_yardstick": float(np.median(win) / np.median(yard)), "first_call_ms": first_ms, "scratch_bytes": scratch,
                     "cells": G * W, "out_bytes": G * W * (4 + 20 * S)}
        eng.close()
        del count, mean, mn, mx, ab
    print(json.dumps(out))


if __name__ == "__main__":
    main()
