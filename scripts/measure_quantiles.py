"""Quantile analyzer on BASELINE config 2's batch (10 000 LB-2 replicas, T = 600 s): one JSON line.

    python scripts/measure_quantiles.py [--replicas 10000] [--reps 5]

The shapes of scripts/measure_windows.py: the whole run with one group / 100 groups / singletons (yardstick: `pooled_summary`
over the same groups), then 100 groups x 60 windows of 10 s and singletons x 60 windows (yardstick: `window_summary`).  In every
case three calls ALTERNATE in the same process: the yardstick, `quantile_summary` with levels (0.5, 0.95, 0.99) and no
thresholds -- the ranks the yardstick selects, without its mean / std passes -- and `quantile_summary` with 9 levels and 4
thresholds.  Every figure is the wall time of the synchronous engine call (read-backs, host layout, all kernels) as min /
median / max over --reps calls after one warm-up call each; `scratch_bytes` is the engine's scratch after the case's first
quantile call on a fresh analyzer engine; the ratios are of medians.
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

LEVELS3 = (0.5, 0.95, 0.99)
LEVELS9 = (0.0, 0.1, 0.5, 0.9, 0.95, 0.99, 0.999, 0.9999, 1.0)
THRESHOLDS4 = (0.01, 0.02, 0.05, 0.2)


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
    clock_bytes = 16.0 * float(np.minimum(res.counts[:, _abi.CNT_COMPLETED].astype(np.int64), res._clock_t.shape[1]).sum())   # noqa: SLF001

    def spread(ms: list[float]) -> dict:
        return {"min_ms": float(np.min(ms)), "median_ms": float(np.median(ms)), "max_ms": float(np.max(ms))}

    out: dict = {"replicas": n, "latencies": clock_bytes / 16.0, "clock_gb": clock_bytes / 1e9, "reps": args.reps,
                 "levels3": LEVELS3, "levels9": LEVELS9, "thresholds4": THRESHOLDS4}
    groups = {"one_group": None, "groups_100": np.arange(n) // max(n // 100, 1), "singletons": "scenario"}
    cases = [(f"{name}_whole", by, None) for name, by in groups.items()]
    cases += [("groups_100_x60", groups["groups_100"], 10.0), ("singletons_x60", "scenario", 10.0)]
    for name, by, w in cases:
        pby = np.arange(n) if isinstance(by, str) else by

        def yardstick() -> float:
            if w is None:
                return float(res.pooled_summary(pby)["pooled_ms"])
            return float(res.window_summary(w, by=by)["window_ms"])

        def q3() -> dict:
            return res.quantile_summary(LEVELS3, window_s=w, by=by)

        def q9() -> dict:
            return res.quantile_summary(LEVELS9, thresholds=THRESHOLDS4, window_s=w, by=by)

        res.close()                                           # a fresh analyzer engine: this case's own scratch
        first = q3()
        scratch3, cells = first["scratch_bytes"], int(first["count"].numel())
        in_cells = float(first["count"].sum())
        del first
        scratch9 = q9()["scratch_bytes"]
        yardstick()
        base, a3, a9 = [], [], []
        for _ in range(args.reps):
            base.append(yardstick())
            a3.append(float(q3()["quantile_ms"]))
            a9.append(float(q9()["quantile_ms"]))
        out[name] = {"cells": cells, "latencies_in_cells": in_cells, "yardstick": spread(base), "quantiles_3": spread(a3),
                     "quantiles_9_4": spread(a9), "scratch_bytes_3": scratch3, "scratch_bytes_9_4": scratch9,
                     "q3_vs_yardstick": float(np.median(a3) / np.median(base)), "q9_4_vs_yardstick": float(np.median(a9) / np.median(base))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
