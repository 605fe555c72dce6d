"""Joint moments of pairs of the sampled series per (group, window of ticks, pair) on BASELINE config 2's batch (10 000 LB-2
replicas, T = 600 s): one JSON line.

    python scripts/measure_series_joint.py [--replicas 10000] [--reps 5]

Pair sets: (i) `one`: the one pair (srv-1:ready_queue_len, srv-2:ready_queue_len, lag 0); (ii) `lags`: that pair at lags 0, 1,
2, 4, ..., 512 (11 pairs); (iii) `acf`: srv-1:ready_queue_len with itself at lags 0 ... 63 (64 pairs).  Shapes: one window over
the whole run with singletons / 100 groups / one group; 60 windows of 10 s with singletons / 100 groups.  Each leg ALTERNATES
in the same process with `af_engine_summarize_series_windows` (one streaming pass over the same sample rows) over the same
cells.  Every figure is the host's wall time around the synchronous engine call (read-backs, host layout, all kernels) as min
/ median / max over --reps calls after one warm-up call of each; `scratch_bytes` is the engine's scratch after the leg's first
joint call on a fresh engine.  Model to judge, not a gate: (i) reads the same sample rows once and should sit near the
yardstick; (ii) and (iii) add register passes over rows that stay in cache or LDS, not bytes.
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
    names = res.series_names()
    q1, q2 = names.index("srv-1:ready_queue_len"), names.index("srv-2:ready_queue_len")
    lags = [0, *(1 << k for k in range(10))]
    sets = {"one": ([q1], [q2], [0]), "lags": ([q1] * len(lags), [q2] * len(lags), lags), "acf": ([q1] * 64, [q1] * 64, list(range(64)))}

    def spread(ms: list[float]) -> dict:
        return {"min_ms": float(np.min(ms)), "median_ms": float(np.median(ms)), "max_ms": float(np.max(ms)),
                "tb_s": sample_bytes / (float(np.median(ms)) * 1e-3) / 1e12}

    out: dict = {"replicas": n, "ticks": float(ticks.sum()), "sample_gb": sample_bytes / 1e9, "series": S, "reps": args.reps,
                 "pairs": {k: [list(v[0]), list(v[1]), list(v[2])] for k, v in sets.items()}}
    groupings = {"singletons": np.arange(n), "groups_100": np.arange(n) // max(n // 100, 1), "one_group": np.zeros(n, dtype=np.int64)}
    whole = np.array([0, cap])
    ten_s = tick_window_edges(ticks_per_window_of(10.0, plan.sample_period), cap)
    cases = [(f"{g}_x1", g, whole) for g in groupings] + [("singletons_x60", "singletons", ten_s), ("groups_100_x60", "groups_100", ten_s)]
    for name, gname, edges in cases:
        ids = groupings[gname]
        G, W = int(ids.max()) + 1, len(edges) - 1
        grp = torch.as_tensor(ids.astype(np.uint32).view(np.int32), device=dev)
        count = torch.empty((G, W), dtype=torch.int32, device=dev)
        mean = torch.empty((G, W, S), dtype=torch.float64, device=dev)
        mn, mx, ab = (torch.empty((G, W, S), dtype=torch.int32, device=dev) for _ in range(3))
        for leg, (pa, pb, pl) in sets.items():
            P = len(pa)
            cnt = torch.empty((G, W, P), dtype=torch.int32, device=dev)
            sx, sy = (torch.empty((G, W, P), dtype=torch.int64, device=dev) for _ in range(2))
            sxx, syy, sxy = (torch.empty((G, W, P, 2), dtype=torch.int64, device=dev) for _ in range(3))
            eng = Engine(plan, dev.index or 0)                    # a fresh engine: this leg's own scratch

            def yardstick() -> float:
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                eng.summarize_series_windows(
                    n, G, edges, samples_ptr=samples.data_ptr(), tick_capacity=cap, counts_ptr=counts.data_ptr(),
                    count_ptr=count.data_ptr(), mean_ptr=mean.data_ptr(), min_ptr=mn.data_ptr(), max_ptr=mx.data_ptr(),
                    above_ptr=ab.data_ptr(), group_ptr=grp.data_ptr())
                return (time.perf_counter() - t0) * 1e3

            def joint() -> tuple[float, int]:
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                _, scratch = eng.summarize_series_joint(
                    n, G, edges, pa, pb, pl, samples_ptr=samples.data_ptr(), tick_capacity=cap, counts_ptr=counts.data_ptr(),
                    n_ptr=cnt.data_ptr(), sx_ptr=sx.data_ptr(), sy_ptr=sy.data_ptr(), sxx_ptr=sxx.data_ptr(), syy_ptr=syy.data_ptr(),
                    sxy_ptr=sxy.data_ptr(), group_ptr=grp.data_ptr())
                return (time.perf_counter() - t0) * 1e3, scratch

            first_ms, scratch = joint()
            yardstick()
            yard, js = [], []
            for _ in range(args.reps):
                yard.append(yardstick())
                js.append(joint()[0])
            assert torch.equal(cnt[:, :, 0], count)               # (every set's first pair has lag 0)
            # lag 0 of a queue against the yardstick's mean: sx / n on the bits
            live = (count.to(torch.int64) & 0xFFFFFFFF) > 0
            mine = sx[:, :, 0].to(torch.float64) / (count.to(torch.int64) & 0xFFFFFFFF).to(torch.float64)
            assert torch.equal(mine[live], mean[:, :, q1][live])
            row = {"yardstick": spread(yard), "series_joint": spread(js), "vs_series_windows": float(np.median(js) / np.median(yard)),
                   "first_call_ms": first_ms, "scratch_bytes": scratch, "cells": G * W, "pairs": P}
            out[f"{name}:{leg}"] = row
            print(f"{name}:{leg}", json.dumps(row), file=sys.stderr, flush=True)   # (progress; the result is stdout's line)
            eng.close()
            del cnt, sx, sy, sxx, syy, sxy
        del count, mean, mn, mx, ab
    print(json.dumps(out))


if __name__ == "__main__":
    main()
