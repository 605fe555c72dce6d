"""Combinations across the sampled series per (group, window of ticks, combination) on BASELINE config 2's batch (10 000 LB-2
replicas, T = 600 s): one JSON line.

    python scripts/measure_series_combined.py [--replicas 10000] [--reps 5]

Combinations: `sum` and `spread` of the two `ready_queue_len` columns, `sum` of the two `ram_in_use` columns, `sum` of the six
edge columns.  Shapes: one window over the whole run with singletons / 100 groups / one group; 60 windows of 10 s with
singletons / 100 groups; each without bins and with 64 bins.  Each leg ALTERNATES in the same process with its comparison
partners over the same cells: (a) `af_engine_summarize_series_windows` (one streaming pass over the same sample rows) and,
for the legs with bins, (b) `af_engine_summarize_series_histogram` of all 12 series with 64 bins.  Every figure is the host's
wall time around the synchronous engine call (read-backs, host layout, the zeroing of the outputs, all kernels) as min /
median / max over --reps calls after one warm-up call of each; `scratch_bytes` is the engine's scratch after the leg's first
combined call on a fresh engine.  Model to judge, not a gate: the call reads the same sample rows once, so without bins it
should sit near (a) and with bins near (b).
"""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

BINS = 64
COMBOS = {"queued": ("sum", "*:ready_queue_len"), "imbalance": ("spread", "*:ready_queue_len"), "fleet_ram": ("sum", "*:ram_in_use"),
          "open": ("sum", "*:edge_concurrent_connection")}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()

    import torch

    from asyncflow_amd import _abi
    from asyncflow_amd.engine import Engine
    from asyncflow_amd.results import check_series_combinations, tick_window_edges, ticks_per_window_of
    from asyncflow_amd.runner import SimulationRunner
    from asyncflow_amd.workloads import lb_two_servers

    res = SimulationRunner(simulation_input=lb_two_servers(), replicas=args.replicas, collect_clock=False).run()
    n, plan = len(res), res.plan
    samples, counts = res._samples_t, res._counts_t   # noqa: SLF001
    dev = samples.device
    cap, S = int(samples.shape[1]), plan.n_series
    ticks = np.minimum(res.counts[:, _abi.CNT_TICKS].astype(np.int64), cap)
    sample_bytes = 4.0 * plan.series_pitch * float(ticks.sum())
    labels, ops, columns = check_series_combinations(COMBOS, res.series_names(), plan.n_edges)
    codes = [_abi.COMBINE_OPS[o] for o in ops]
    Cn = len(labels)
    assert [len(c) for c in columns] == [2, 2, 2, 6]

    def spread(ms: list[float]) -> dict:
        return {"min_ms": float(np.min(ms)), "median_ms": float(np.median(ms)), "max_ms": float(np.max(ms)),
                "tb_s": sample_bytes / (float(np.median(ms)) * 1e-3) / 1e12}

    out: dict = {"replicas": n, "ticks": float(ticks.sum()), "sample_gb": sample_bytes / 1e9, "series": S, "reps": args.reps,
                 "bins": BINS, "combinations": {k: [ops[i], columns[i].tolist()] for i, k in enumerate(labels)}}
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
        ccount, hcount = (torch.empty((G, W), dtype=torch.int32, device=dev) for _ in range(2))
        cmean, cmn, cmx = (torch.empty((G, W, Cn), dtype=torch.float64, device=dev) for _ in range(3))
        cab, cunder, cover = (torch.empty((G, W, Cn), dtype=torch.int32, device=dev) for _ in range(3))
        chist = torch.empty((G, W, Cn, BINS), dtype=torch.int32, device=dev)
        hist = torch.empty((G, W, S, BINS), dtype=torch.int32, device=dev)
        under, over = (torch.empty((G, W, S), dtype=torch.int32, device=dev) for _ in range(2))
        for leg, bins in (("no_bins", 0), ("bins_64", BINS)):
            eng = Engine(plan, dev.index or 0)                    # a fresh engine: this leg's own scratch

            def yardstick() -> float:
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                eng.summarize_series_windows(
                    n, G, edges, samples_ptr=samples.data_ptr(), tick_capacity=cap, counts_ptr=counts.data_ptr(),
                    count_ptr=count.data_ptr(), mean_ptr=mean.data_ptr(), min_ptr=mn.data_ptr(), max_ptr=mx.data_ptr(),
                    above_ptr=ab.data_ptr(), group_ptr=grp.data_ptr())
                return (time.perf_counter() - t0) * 1e3

            def histogram() -> float:
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                eng.summarize_series_histogram(
                    n, G, edges, BINS, samples_ptr=samples.data_ptr(), tick_capacity=cap, counts_ptr=counts.data_ptr(),
                    hist_ptr=hist.data_ptr(), count_ptr=hcount.data_ptr(), under_ptr=under.data_ptr(), over_ptr=over.data_ptr(),
                    group_ptr=grp.data_ptr())
                return (time.perf_counter() - t0) * 1e3

            def combined() -> tuple[float, int]:
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                _, scratch = eng.summarize_series_combined(
                    n, G, edges, codes, columns, samples_ptr=samples.data_ptr(), tick_capacity=cap, counts_ptr=counts.data_ptr(),
                    mean_ptr=cmean.data_ptr(), count_ptr=ccount.data_ptr(), min_ptr=cmn.data_ptr(), max_ptr=cmx.data_ptr(),
                    above_ptr=cab.data_ptr(), hist_ptr=chist.data_ptr() if bins else 0, under_ptr=cunder.data_ptr() if bins else 0,
                    over_ptr=cover.data_ptr() if bins else 0, group_ptr=grp.data_ptr(), bins=bins)
                return (time.perf_counter() - t0) * 1e3, scratch

            first_ms, scratch = combined()
            yardstick()
            if bins:
                histogram()
            yard, hs, cs = [], [], []
            for _ in range(args.reps):
                yard.append(yardstick())
                if bins:
                    hs.append(histogram())
                cs.append(combined()[0])
            assert torch.equal(ccount, count)
            row = {"yardstick": spread(yard), "series_combined": spread(cs), "vs_series_windows": float(np.median(cs) / np.median(yard)),
                   "first_call_ms": first_ms, "scratch_bytes": scratch, "cells": G * W}
            if bins:
                total = (chist.to(torch.int64) & 0xFFFFFFFF).sum(dim=-1) + (cunder.to(torch.int64) & 0xFFFFFFFF) + (cover.to(torch.int64) & 0xFFFFFFFF)
                assert torch.equal(total, (count.to(torch.int64) & 0xFFFFFFFF)[:, :, None].expand_as(total))
                row.update(series_histogram=spread(hs), vs_series_histogram=float(np.median(cs) / np.median(hs)),
                           share_over=float((cover.to(torch.int64) & 0xFFFFFFFF).sum()) / max(float(total.sum()), 1.0))
            out[f"{name}:{leg}"] = row
            print(f"{name}:{leg}", json.dumps(row), file=sys.stderr, flush=True)   # (progress; the result is stdout's line)
            eng.close()
        del count, mean, mn, mx, ab, ccount, hcount, cmean, cmn, cmx, cab, cunder, cover, chist, hist, under, over
    print(json.dumps(out))


if __name__ == "__main__":
    main()
