"""The k slowest requests per window and group on BASELINE config 2's batch (10 000 LB-2 replicas, T = 600 s): one JSON line.

    python scripts/measure_exemplars.py [--replicas 10000] [--reps 5] [--ks 16 64]

Every case ALTERNATES, in the same process, `af_engine_summarize_exemplars` with the windowed analyzer of the same mode over the
same cells (`af_engine_summarize_windows` / `af_engine_summarize_arrival_windows`) -- the yardstick: it reads the clock rows
twice and partitions them, and is not the code under test.  Cases: k = 16 and 64; one window / 60 windows of 10 s / 600 windows
of 1 s; singleton groups / 100 groups / one group; both `window_of`.  Every figure is the wall time of the synchronous engine
call (read-backs, host checks, all kernels), started after a device synchronisation, as min / median / max over --reps calls
after one warm-up call of each.  Model, not a gate: one pass over the clock rows plus the candidate records written once and read
once (`n * W' * k * 12 .. 16 B`), so not above the yardstick; `pass_tb_s` is the clock rows' bytes per median call time.
The ascending-latency worst case (every chunk of rows displaces the kept list) is NOT in this batch: its latencies are stationary.
A line per case goes to stderr as it finishes.
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
    ap.add_argument("--ks", type=int, nargs="+", default=[16, 64])
    args = ap.parse_args()

    import torch

    from asyncflow_amd import _abi
    from asyncflow_amd.results import window_edges
    from asyncflow_amd.runner import SimulationRunner
    from asyncflow_amd.workloads import lb_two_servers

    res = SimulationRunner(simulation_input=lb_two_servers(), replicas=args.replicas).run()
    n, plan = len(res), res.plan
    T = float(plan.total_time)
    clock, counts = res._clock_t, res._counts_t   # noqa: SLF001
    dev = clock.device
    clock_bytes = 16.0 * float(np.minimum(res.counts[:, _abi.CNT_COMPLETED].astype(np.int64), clock.shape[1]).sum())
    eng, _ = res._arrival_engine()   # noqa: SLF001

    def spread(ms: list[float]) -> dict:
        return {"min_ms": float(np.min(ms)), "median_ms": float(np.median(ms)), "max_ms": float(np.max(ms))}

    out: dict = {"replicas": n, "latencies": clock_bytes / 16.0, "clock_gb": clock_bytes / 1e9, "reps": args.reps}
    groupings = (("singletons", np.arange(n), n), ("groups_100", np.arange(n) // max(n // 100, 1), int((n - 1) // max(n // 100, 1)) + 1),
                 ("one_group", np.zeros(n, dtype=np.int64), 1))
    windows = (("x1", np.array([0.0, 2.0 * T])), ("x60", window_edges(10.0, T)), ("x600", window_edges(1.0, T)))
    for wname, e in windows:
        n_win = int(e.shape[0] - 1)
        for gname, ids, n_groups in groupings:
            grp = torch.from_numpy(ids.astype(np.uint32).view(np.int32)).to(dev)
            for window_of in ("finish", "arrival"):
                def yardstick() -> float:
                    torch.cuda.synchronize(dev)
                    return float(res.window_summary(edges=e, by=ids, window_of=window_of)["window_ms"])   # noqa: B023

                for k in args.ks:
                    cells = n_groups * n_win
                    total = torch.empty(cells, dtype=torch.int64, device=dev)
                    kept = torch.empty(cells, dtype=torch.int32, device=dev)
                    scen, row = (torch.empty(cells * k, dtype=torch.int32, device=dev) for _ in range(2))
                    pair = torch.empty(cells * k * 2, dtype=torch.float64, device=dev)
                    scratch = 0

                    def exemplars() -> float:
                        nonlocal scratch
                        torch.cuda.synchronize(dev)               # nothing of the call before is still running
                        ms, scratch = eng.summarize_exemplars(
                            n, n_groups, k, edges=e, window_of=window_of, clock_ptr=clock.data_ptr(), clock_capacity=int(clock.shape[1]),   # noqa: B023
                            counts_ptr=counts.data_ptr(), total_ptr=total.data_ptr(), kept_ptr=kept.data_ptr(), scenario_ptr=scen.data_ptr(),   # noqa: B023
                            row_ptr=row.data_ptr(), pair_ptr=pair.data_ptr(), group_ptr=grp.data_ptr())   # noqa: B023
                        return float(ms)

                    exemplars()
                    yardstick()
                    mine, theirs = [], []
                    for _ in range(args.reps):
                        mine.append(exemplars())
                        theirs.append(yardstick())
                    med = float(np.median(mine))
                    name = f"{gname}_{wname}_{window_of}_k{k}"
                    out[name] = {"exemplars": spread(mine), "windows": spread(theirs), "ratio": med / float(np.median(theirs)),
                                 "pass_tb_s": clock_bytes / (med * 1e-3) / 1e12, "cells": cells, "scratch_bytes": int(scratch),
                                 "rows_in_cells": int(total.sum().item())}
                    print(name, json.dumps(out[name]), file=sys.stderr, flush=True)
                    del total, kept, scen, row, pair
            del grp
    print(json.dumps(out))


if __name__ == "__main__":
    main()
