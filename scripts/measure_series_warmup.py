"""Warm-up truncation (MSER-5) of the sampled series per (group, window of ticks, column) on BASELINE config 2's batch (10 000
LB-2 replicas, T = 600 s): one JSON line.

    python scripts/measure_series_warmup.py [--replicas 10000] [--reps 5]

Column sets: (i) `one`: srv-1:ready_queue_len; (ii) `all`: every integer series.  Shapes: one window over the whole run with
singletons / 100 groups / one group; 100 groups x 60 windows of 10 s.  B = 5 throughout.  Each leg ALTERNATES in the same
process with `af_engine_summarize_series_windows` (one streaming pass over the same sample rows) over the same cells.  Every
figure is the host's wall time around the synchronous engine call (read-backs, host layout, the zeroing of the batch sums, all
kernels) as min / median / max over --reps calls after one warm-up call of each; `scratch_bytes` is the engine's scratch after
the leg's first warm-up call on a fresh engine.  Model to judge, not a gate: the row pass reads the same bytes once and writes
at most 0.4 x the selected columns' bytes as batch sums, the second pass touches only those; one column should sit within a
small multiple of the yardstick.
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
    names = res.series_names()
    q1 = names.index("srv-1:ready_queue_len")
    ints = [int(j) for j in np.nonzero(~ram_columns(S, plan.n_edges))[0]]
    sets = {"one": [q1], "all": ints}
    batch = 5

    def spread(ms: list[float]) -> dict:
        return {"min_ms": float(np.min(ms)), "median_ms": float(np.median(ms)), "max_ms": float(np.max(ms)),
                "tb_s": sample_bytes / (float(np.median(ms)) * 1e-3) / 1e12}

    out: dict = {"replicas": n, "ticks": float(ticks.sum()), "sample_gb": sample_bytes / 1e9, "series": S, "reps": args.reps,
                 "batch": batch, "columns": sets}
    groupings = {"singletons": np.arange(n), "groups_100": np.arange(n) // max(n // 100, 1), "one_group": np.zeros(n, dtype=np.int64)}
    whole = np.array([0, cap])
    ten_s = tick_window_edges(ticks_per_window_of(10.0, plan.sample_period), cap)
    cases = [(f"{g}_x1", g, whole) for g in groupings] + [("groups_100_x60", "groups_100", ten_s)]
    for name, gname, edges in cases:
        ids = groupings[gname]
        G, W = int(ids.max()) + 1, len(edges) - 1
        grp = torch.as_tensor(ids.astype(np.uint32).view(np.int32), device=dev)
        count = torch.empty((G, W), dtype=torch.int32, device=dev)
        mean = torch.empty((G, W, S), dtype=torch.float64, device=dev)
        mn, mx, ab = (torch.empty((G, W, S), dtype=torch.int32, device=dev) for _ in range(3))
        for leg, cols in sets.items():
            Cn = len(cols)
            nb = torch.empty((G, W), dtype=torch.int32, device=dev)
            trunc = torch.empty((G, W, Cn), dtype=torch.int32, device=dev)
            s1, s1_all = (torch.empty((G, W, Cn, 2), dtype=torch.int64, device=dev) for _ in range(2))
            s2, s2_all = (torch.empty((G, W, Cn, 3), dtype=torch.int64, device=dev) for _ in range(2))
            eng = Engine(plan, dev.index or 0)                    # a fresh engine: this leg's own scratch

            def yardstick() -> float:
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                eng.summarize_series_windows(
                    n, G, edges, samples_ptr=samples.data_ptr(), tick_capacity=cap, counts_ptr=counts.data_ptr(),
                    count_ptr=count.data_ptr(), mean_ptr=mean.data_ptr(), min_ptr=mn.data_ptr(), max_ptr=mx.data_ptr(),
                    above_ptr=ab.data_ptr(), group_ptr=grp.data_ptr())
                return (time.perf_counter() - t0) * 1e3

            def warmup() -> tuple[float, int]:
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                _, scratch = eng.summarize_series_warmup(
                    n, G, edges, cols, batch, samples_ptr=samples.data_ptr(), tick_capacity=cap, counts_ptr=counts.data_ptr(),
                    batches_ptr=nb.data_ptr(), trunc_ptr=trunc.data_ptr(), s1_ptr=s1.data_ptr(), s2_ptr=s2.data_ptr(),
                    s1_all_ptr=s1_all.data_ptr(), s2_all_ptr=s2_all.data_ptr(), group_ptr=grp.data_ptr())
                return (time.perf_counter() - t0) * 1e3, scratch

            first_ms, scratch = warmup()
            yardstick()
            yard, ws = [], []
            for _ in range(args.reps):
                yard.append(yardstick())
                ws.append(warmup()[0])
            # S1(0) of a queue against the yardstick's mean where every member holds whole batches only: s1_all / count on the bits
            c64, j64 = count.to(torch.int64) & 0xFFFFFFFF, nb.to(torch.int64) & 0xFFFFFFFF
            members = torch.as_tensor(np.bincount(ids, minlength=G), device=dev)[:, None]
            whole_cells = (c64 > 0) & (c64 == j64 * batch * members)
            col = cols.index(q1)
            mine = s1_all[:, :, col, 0].to(torch.float64) / c64.to(torch.float64)
            assert bool((s1_all[:, :, col, 1] == 0).all()) and torch.equal(mine[whole_cells], mean[:, :, q1][whole_cells])
            live = j64 > 0
            row = {"yardstick": spread(yard), "series_warmup": spread(ws), "vs_series_windows": float(np.median(ws) / np.median(yard)),
                   "first_call_ms": first_ms, "scratch_bytes": scratch, "cells": G * W, "columns": Cn, "whole_cells": int(whole_cells.sum()),
                   "converged_share": float(((trunc.to(torch.int64) < (j64 // 2)[:, :, None]) & live[:, :, None]).sum() / max(int(live.sum()) * Cn, 1)),
                   "median_trunc": float(trunc.to(torch.float64).median())}
            out[f"{name}:{leg}"] = row
            print(f"{name}:{leg}", json.dumps(row), file=sys.stderr, flush=True)   # (progress; the result is stdout's line)
            eng.close()
            del nb, trunc, s1, s2, s1_all, s2_all
        del count, mean, mn, mx, ab
    print(json.dumps(out))


if __name__ == "__main__":
    main()
