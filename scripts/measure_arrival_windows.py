"""Windows by ARRIVAL time on BASELINE config 2's batch (10 000 LB-2 replicas, T = 600 s): one JSON line.

    python scripts/measure_arrival_windows.py [--replicas 10000] [--reps 5]

Every case ALTERNATES, in the same process, `window_summary(window_of="arrival")` with `window_summary()` over the same edges
and groups -- the by-finish call is the yardstick: its kernels find a window's rows by ~17 loads per edge and copy row ranges,
the by-arrival call reads every clock row twice (counts, then the stable partition).  Cases: one window over the whole horizon
with one group / 100 groups / singletons; 100 groups x 60 windows of 10 s; singletons x 60 windows; singletons x 600 windows.
Every figure is the wall time of the synchronous engine call (read-backs, host layout, all kernels) as min / median / max
over --reps calls after one warm-up call of each; `scratch_bytes` is the engine's scratch after the case's first by-arrival call
on a fresh analyzer engine; `extra_tb_s` the clock rows' bytes (16 B per completion) per (arrival - finish) median time: what
the one further streaming pass over the clock runs at, if that were all the difference.
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
        return {"min_ms": float(np.min(ms)), "median_ms": float(np.median(ms)), "max_ms": float(np.max(ms))}

    out: dict = {"replicas": n, "latencies": clock_bytes / 16.0, "clock_gb": clock_bytes / 1e9, "reps": args.reps}
    groups_100 = np.arange(n) // max(n // 100, 1)
    whole = np.array([-1.0, T + 1.0])
    cases = (("one_group_x1", None, whole), ("groups_100_x1", groups_100, whole), ("singletons_x1", "scenario", whole),
             ("groups_100_x60", groups_100, None), ("singletons_x60", "scenario", None), ("singletons_x600", "scenario", None))
    for name, by, edges in cases:
        kw = {"edges": edges} if edges is not None else {"window_s": 1.0 if name.endswith("x600") else 10.0}
        res.close()                                           # a fresh analyzer engine: this case's own scratch
        first = res.window_summary(by=by, window_of="arrival", **kw)
        res.window_summary(by=by, **kw)
        arrival, finish = [], []
        for _ in range(args.reps):
            arrival.append(float(res.window_summary(by=by, window_of="arrival", **kw)["window_ms"]))
            finish.append(float(res.window_summary(by=by, **kw)["window_ms"]))
        st = first["stats"]
        extra_ms = float(np.median(arrival) - np.median(finish))
        out[name] = {"arrival": spread(arrival), "finish": spread(finish), "arrival_vs_finish": float(np.median(arrival) / np.median(finish)),
                     "extra_ms": extra_ms, "extra_tb_s": clock_bytes / (extra_ms * 1e-3) / 1e12 if extra_ms > 0 else None,
                     "scratch_bytes": first["scratch_bytes"], "first_call_ms": first["window_ms"],
                     "cells": int(st.shape[0] * st.shape[1]), "windowed_latencies": float(st[:, :, 0].sum())}
        del first, st
    print(json.dumps(out))


if __name__ == "__main__":
    main()
