"""Requests in flight per window and group on BASELINE config 2's batch (10 000 LB-2 replicas, T = 600 s): one JSON line.

    python scripts/measure_inflight.py [--replicas 10000] [--reps 5] [--no-yardstick]

Every case ALTERNATES, in the same process, `af_engine_summarize_inflight` with `af_engine_summarize_arrival_windows` over the
same windows and groups -- the yardstick: it also reads the clock rows (twice: a counts pass and a stable partition) and is not
the code under test.  Cases: one window / 60 windows of 10 s / 600 windows of 1 s, each with singleton groups / 100 groups / one
group, each without and with the per-tick `in_flight` output (4 B per scenario and tick).  Every figure is the wall time of the
synchronous engine call (read-backs, host checks, all kernels), started after a device synchronisation, as min / median / max over --reps calls after one warm-up call of
each.  Model, not a gate: one pass over the clock rows (two where the run has more ticks than the kernel's chunk), plus the
per-tick write when asked for; `pass_tb_s` is the clock rows' bytes per median call time.  --no-yardstick repeats the call back
to back without the other one in between (what a call costs when nothing else ran since the last one).
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-yardstick", action="store_true", help="do not alternate with af_engine_summarize_arrival_windows")
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

    def spread(ms: list[float]) -> dict:
        return {"min_ms": float(np.min(ms)), "median_ms": float(np.median(ms)), "max_ms": float(np.max(ms))}

    out: dict = {"replicas": n, "latencies": clock_bytes / 16.0, "clock_gb": clock_bytes / 1e9, "ticks": ticks, "tick_capacity": tick_cap,
                 "per_tick_gb": 4.0 * n * tick_cap / 1e9, "reps": args.reps}
    per_tick = torch.empty((n, tick_cap), dtype=torch.int32, device=dev)
    groupings = (("singletons", np.arange(n), n), ("groups_100", np.arange(n) // max(n // 100, 1), int((n - 1) // max(n // 100, 1)) + 1),
                 ("one_group", np.zeros(n, dtype=np.int64), 1))
    windows = (("x1", np.array([0, tick_cap], dtype=np.uint32)), ("x60", tick_window_edges(round(10.0 / p), ticks)),
               ("x600", tick_window_edges(round(1.0 / p), ticks)))
    for wname, b in windows:
        n_win = int(b.shape[0] - 1)
        edges_s = b.astype(np.float64) * p
        for gname, ids, n_groups in groupings:
            grp = torch.from_numpy(ids.astype(np.uint32).view(np.int32)).to(dev)
            cells = [torch.empty((n_groups, n_win), dtype=torch.int32, device=dev) for _ in range(4)]
            total = torch.empty((n_groups, n_win), dtype=torch.int64, device=dev)

            def inflight(with_rows: bool) -> float:
                torch.cuda.synchronize(dev)                   # nothing of the call before is still running
                ms, _ = eng.summarize_inflight(n, n_groups, b, p, clock_ptr=clock.data_ptr(), clock_capacity=int(clock.shape[1]),   # noqa: B023
                                               tick_capacity=tick_cap, counts_ptr=counts.data_ptr(), count_ptr=cells[0].data_ptr(),   # noqa: B023
                                               sum_ptr=total.data_ptr(), min_ptr=cells[1].data_ptr(), max_ptr=cells[2].data_ptr(),   # noqa: B023
                                               above_ptr=cells[3].data_ptr(), group_ptr=grp.data_ptr(),   # noqa: B023
                                               in_flight_ptr=per_tick.data_ptr() if with_rows else 0)
                return float(ms)

            def yardstick() -> float:
                if args.no_yardstick:
                    return float("nan")
                torch.cuda.synchronize(dev)
                return float(res.window_summary(edges=edges_s, by=ids, window_of="arrival")["window_ms"])   # noqa: B023

            for with_rows in (False, True):
                inflight(with_rows)
                yardstick()
                mine, theirs = [], []
                for _ in range(args.reps):
                    mine.append(inflight(with_rows))
                    theirs.append(yardstick())
                med = float(np.median(mine))
                out[f"{gname}_{wname}{'_rows' if with_rows else ''}"] = {
                    "inflight": spread(mine), "arrival_windows": spread(theirs), "ratio": med / float(np.median(theirs)),
                    "pass_tb_s": clock_bytes / (med * 1e-3) / 1e12, "cells": n_groups * n_win,
                    "mean_in_flight": float(total.sum().item()) / max(float((cells[0].to(torch.int64) & 0xFFFFFFFF).sum().item()), 1.0)}
            del cells, total, grp
    print(json.dumps(out))


if __name__ == "__main__":
    main()
