"""Latency by the state met on arrival on BASELINE config 2's batch (10 000 LB-2 replicas, T = 600 s): one JSON line.

    python scripts/measure_state_cells.py [--replicas 10000] [--reps 5]

Every case ALTERNATES, in the same process, `state_summary(...)` with `window_summary(window_of="arrival")` over THE SAME NUMBER
OF CELLS PER GROUP and the same groups -- the by-arrival call is the yardstick: both read every clock row twice (counts, then
the stable partition) and reduce the same number of cells; the state call also gathers one sample word per row in each pass.
Cases: 8 bins against 8 windows, and 60 windows x 8 bins against 480 windows; one group / 100 groups / singletons; once on the
first server's `ready_queue_len` (an integer column, width 1) and once on its `ram_in_use` (a float column, eight bins up to
the batch's maximum).  Every figure is the wall time of the synchronous engine call (read-backs, host layout, all kernels) as
min / median / max over --reps calls after one warm-up call of each.  MODEL: the by-arrival cost plus the gathered sample
lines of the two passes -- at most two passes over the sample rows at the 5.8 TB/s the series kernels reach: `model_extra_ms`;
`met` says whether the measured `extra_ms` (state - arrival, medians) stays within it.
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

SERIES_TB_S = 5.8


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()

    from asyncflow_amd import _abi
    from asyncflow_amd.runner import SimulationRunner
    from asyncflow_amd.workloads import lb_two_servers

    res = SimulationRunner(simulation_input=lb_two_servers(), replicas=args.replicas).run()
    n = len(res)
    T = float(res.plan.total_time)
    clock_bytes = 16.0 * float(np.minimum(res.counts[:, _abi.CNT_COMPLETED].astype(np.int64), res._clock_t.shape[1]).sum())   # noqa: SLF001
    ticks = np.minimum(res.counts[:, _abi.CNT_TICKS].astype(np.int64), res._samples_t.shape[1])   # noqa: SLF001
    sample_bytes = 4.0 * float(res._samples_t.shape[2]) * float(ticks.sum())   # noqa: SLF001
    model_extra_ms = 2.0 * sample_bytes / (SERIES_TB_S * 1e12) * 1e3

    def spread(ms: list[float]) -> dict:
        return {"min_ms": float(np.min(ms)), "median_ms": float(np.median(ms)), "max_ms": float(np.max(ms))}

    names = res.series_names()
    sid = res.plan.server_ids[0]
    ready, ram = names.index(f"{sid}:ready_queue_len"), names.index(f"{sid}:ram_in_use")
    ram_max = float(res.decode_series_max(res.summary(rps=False, series=True)["series_max"].cpu().numpy())[:, ram].max())
    series = {"ready_queue_len": (ready, 1.0), "ram_in_use": (ram, max(ram_max, 8.0) / 8.0)}
    out: dict = {"replicas": n, "latencies": clock_bytes / 16.0, "clock_gb": clock_bytes / 1e9, "sample_gb": sample_bytes / 1e9,
                 "reps": args.reps, "model_extra_ms": model_extra_ms, "ram_width": series["ram_in_use"][1]}
    groups_100 = np.arange(n) // max(n // 100, 1)
    for gname, by in (("one_group", None), ("groups_100", groups_100), ("singletons", "scenario")):
        for cname, state_kw, arrival_edges in (("8_bins_vs_8_windows", {}, np.linspace(0.0, T, 9)),
                                               ("60x8_vs_480_windows", {"window_s": 10.0}, np.linspace(0.0, T, 481))):
            for sname, (col, width) in series.items():
                res.close()                                   # a fresh analyzer engine: this case's own scratch
                first = res.state_summary(col, 8, width=width, by=by, **state_kw)
                res.window_summary(edges=arrival_edges, by=by, window_of="arrival")
                state, arrival = [], []
                for _ in range(args.reps):
                    state.append(float(res.state_summary(col, 8, width=width, by=by, **state_kw)["state_ms"]))
                    arrival.append(float(res.window_summary(edges=arrival_edges, by=by, window_of="arrival")["window_ms"]))
                st = first["stats"]
                extra_ms = float(np.median(state) - np.median(arrival))
                out[f"{gname}:{cname}:{sname}"] = {
                    "state": spread(state), "arrival": spread(arrival), "state_vs_arrival": float(np.median(state) / np.median(arrival)),
                    "extra_ms": extra_ms, "met": bool(extra_ms <= model_extra_ms), "scratch_bytes": first["scratch_bytes"],
                    "first_call_ms": first["state_ms"], "cells": int(st.shape[0] * st.shape[1] * st.shape[2]),
                    "cells_filled": int((st[..., 0] > 0).sum()), "latencies_in_cells": float(st[..., 0].sum())}
                del first, st
    print(json.dumps(out))


if __name__ == "__main__":
    main()
