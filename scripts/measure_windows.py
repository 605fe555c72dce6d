"""Windowed analyzer on BASELINE config 2's batch (10 000 LB-2 replicas, T = 600 s): one JSON line.

    python scripts/measure_windows.py [--replicas 10000] [--reps 5]

One window over the whole horizon with one group / 100 groups / singletons, each ALTERNATING in the same process with
`pooled_summary` over the same groups (the yardstick: the windowed call adds a binary search per scenario, the order check
and the bounds read-back); then 100 groups x 60 windows of 10 s, singletons x 60 windows and singletons x 600 windows
(6 000 000 small cells at the default size).  Every figure is the wall time of the synchronous engine call (read-backs, host
layout, all kernels) as min / median / max over --reps calls after one warm-up call; `scratch_bytes` is the engine's scratch
after the case's first call on a fresh analyzer engine; `tb_s` the clock rows' bytes (16 B per completion) per median time.
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
    args = ap.parse_args()

    from asyncflow_amd import _abi
    from asyncflow_amd.runner import SimulationRunner
    from asyncflow_amd.workloads import lb_two_servers

    res = SimulationRunner(simulation_input=lb_two_servers(), replicas=args.replicas).run()
    n = len(res)
    T = float(res.plan.total_time)
    clock_bytes = 16.0 * float(np.minimum(res.counts[:, _abi.CNT_COMPLETED].astype(np.int64), res._clock_t.shape[1]).sum())   # noqa: SLF001

    def spread(ms: list[float]) -> dict:
        return {"min_ms": float(np.min(ms)), "median_ms": float(np.median(ms)), "max_ms": float(np.max(ms)),
                "tb_s": clock_bytes / (float(np.median(ms)) * 1e-3) / 1e12}

    out: dict = {"replicas": n, "latencies": clock_bytes / 16.0, "clock_gb": clock_bytes / 1e9, "reps": args.reps}
    groups = {"one_group": None, "groups_100": np.arange(n) // max(n // 100, 1), "singletons": "scenario"}
    whole = [-1.0, T + 1.0]
    for name, by in groups.items():
        pby = np.arange(n) if isinstance(by, str) else by
        res.close()                                           # a fresh analyzer engine: this case's own scratch
        first = res.window_summary(edges=whole, by=by)
        res.pooled_summary(pby)
        pooled, windows = [], []
        for _ in range(args.reps):
            pooled.append(float(res.pooled_summary(pby)["pooled_ms"]))
            windows.append(float(res.window_summary(edges=whole, by=by)["window_ms"]))
        out[f"{name}_x1"] = {"pooled": spread(pooled), "windows": spread(windows), "scratch_bytes": first["scratch_bytes"],
                             "windows_vs_pooled": float(np.median(windows) / np.median(pooled))}
    for name, by, w in (("groups_100_x60", groups["groups_100"], 10.0), ("singletons_x60", "scenario", 10.0),
                        ("singletons_x600", "scenario", 1.0)):
        res.close()
        first = res.window_summary(w, by=by)
        ms = [float(res.window_summary(w, by=by)["window_ms"]) for _ in range(args.reps)]
        st = first["stats"]
        out[name] = {"windows": spread(ms), "scratch_bytes": first["scratch_bytes"], "first_call_ms": first["window_ms"],
                     "cells": int(st.shape[0] * st.shape[1]), "windowed_latencies": float(st[:, :, 0].sum())}
        del first, st
    print(json.dumps(out))


if __name__ == "__main__":
    main()
