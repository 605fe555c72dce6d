"""Pooled analyzer on BASELINE config 2's batch (10 000 LB-2 replicas, T = 600 s): one JSON line.

    python scripts/measure_pooled.py [--replicas 10000] [--reps 3]

Cases: one group of every replica, 100 groups of 100 replicas, 10 000 singleton groups; each the median wall time of
`af_engine_summarize_pooled` (the synchronous call: counts read back, layout, all kernels) over --reps calls after one
warm-up call, and the effective bandwidth by the clock rows' bytes (16 B per completion, read once by the compaction).
For comparison the per-scenario analyzer's latency kernel on the same batch (`summary(rps=False)`: summary_ms).
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
    args = ap.parse_args()

    from asyncflow_amd import _abi
    from asyncflow_amd.runner import SimulationRunner
    from asyncflow_amd.workloads import lb_two_servers

    res = SimulationRunner(simulation_input=lb_two_servers(), replicas=args.replicas).run()
    n = len(res)
    clock_bytes = 16.0 * float(np.minimum(res.counts[:, _abi.CNT_COMPLETED].astype(np.int64), res._clock_t.shape[1]).sum())   # noqa: SLF001

    def timed(fn) -> float:
        fn()
        return float(np.median([fn() for _ in range(args.reps)]))

    out: dict = {"replicas": n, "latencies": clock_bytes / 16.0, "clock_gb": clock_bytes / 1e9}
    per_ms = timed(lambda: float(res.summary(rps=False)["summary_ms"]))
    out["per_scenario_latency_kernel_ms"] = per_ms
    cases = {"one_group": None, "groups_100x100": np.arange(n) // max(n // 100, 1), "singletons": np.arange(n)}
    for name, by in cases.items():
        ms = timed(lambda by=by: res.pooled_summary(by)["pooled_ms"])
        out[f"{name}_ms"] = ms
        out[f"{name}_tb_s"] = clock_bytes / (ms * 1e-3) / 1e12
    out["singletons_vs_latency_kernel"] = out["singletons_ms"] / per_ms
    print(json.dumps(out))


if __name__ == "__main__":
    main()
