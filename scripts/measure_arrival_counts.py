"""Arrivals per window and group on BASELINE config 2's batch (10 000 LB-2 replicas, T = 600 s): one JSON line.

    python scripts/measure_arrival_counts.py [--replicas 10000] [--reps 5]

Every case ALTERNATES, in the same process, `af_engine_summarize_arrivals` with an `af_engine_run` of the same sweep (counts
only: no clock, no samples) whose `af_stats.pregen_ms` is the yardstick -- the call generates the same arrival times with the
same kernel and then reads them once at most.  Cases: 1 / 60 / 600 windows over the horizon x singletons / 100 groups / one
group.  Per case: the wall time of the synchronous call (host staging, pre-generation, both counting kernels) as min / median /
max over --reps calls after one warm-up call, the run's pregen_ms likewise, and the MODEL the median is held against:

    model_ms = pregen_ms (median) + n * draw_capacity * 8 bytes / 6 TB/s      (one streaming pass over the rows at most)

"met": median <= model_ms + 0.25 ms (the call's host side: a staged sweep, two launches, one synchronisation).
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

HBM_BYTES_PER_MS = 6.0e9      # ~6 TB/s: what a streaming read of a buffer far larger than the caches reaches
HOST_MS = 0.25


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()

    import torch

    from asyncflow_amd import _abi
    from asyncflow_amd.engine import Engine
    from asyncflow_amd.plan import lower
    from asyncflow_amd.workloads import lb_two_servers

    plan = lower(lb_two_servers())
    n, T, cap = args.replicas, float(plan.total_time), int(plan.clock_capacity())
    seeds = (np.uint64(0xC0F30000) + np.arange(n, dtype=np.uint64)).astype(np.uint64)
    dev = torch.device("cuda", 0)
    counts = torch.zeros((n, _abi.CNT_SLOTS), dtype=torch.int32, device=dev)
    eng = Engine(plan, 0)

    def spread(ms: list[float]) -> dict:
        return {"min_ms": float(np.min(ms)), "median_ms": float(np.median(ms)), "max_ms": float(np.max(ms))}

    def run_pregen_ms() -> float:
        counts.zero_()
        torch.cuda.synchronize(dev)
        return float(eng.run(seeds, [], clock_ptr=0, clock_capacity=cap, samples_ptr=0, tick_capacity=0, counts_ptr=counts.data_ptr(),
                             draw_capacity=cap).pregen_ms)

    row_bytes = float(n) * cap * 8.0
    out: dict = {"replicas": n, "draw_capacity": cap, "row_gb": row_bytes / 1e9, "reps": args.reps, "pass_ms_at_6_tb_s": row_bytes / HBM_BYTES_PER_MS}
    groupings = (("singletons", None, n), ("groups_100", np.arange(n) // max(n // 100, 1), int((n - 1) // max(n // 100, 1)) + 1),
                 ("one_group", np.zeros(n, dtype=np.int64), 1))
    for n_win in (1, 60, 600):
        edges = np.linspace(0.0, T, n_win + 1)
        for name, group, n_groups in groupings:
            arr = torch.zeros((n_groups, n_win), dtype=torch.int64, device=dev)
            grp = None if group is None else torch.as_tensor(group.astype(np.uint32).view(np.int32), device=dev)

            def call() -> float:
                torch.cuda.synchronize(dev)
                return eng.summarize_arrivals(seeds, [], n_groups, edges, draw_capacity=cap, arrivals_ptr=arr.data_ptr(),
                                              group_ptr=grp.data_ptr() if grp is not None else 0)[0]

            call()
            run_pregen_ms()
            mine, pregen = [], []
            for _ in range(args.reps):
                mine.append(call())
                pregen.append(run_pregen_ms())
            model = float(np.median(pregen)) + row_bytes / HBM_BYTES_PER_MS
            out[f"{name}_x{n_win}"] = {"call": spread(mine), "pregen": spread(pregen), "model_ms": model,
                                       "beyond_pregen_ms": float(np.median(mine) - np.median(pregen)),
                                       "verdict": "met" if float(np.median(mine)) <= model + HOST_MS else "missed",
                                       "arrivals": int(arr.sum().item())}
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
