"""Occupancy histograms of the sampled series per (group, window of ticks, series) on BASELINE config 2's batch (10 000 LB-2
replicas, T = 600 s): one JSON line.

    python scripts/measure_series_histogram.py [--replicas 10000] [--reps 5]

Shapes: one window over the whole run with singletons / 100 groups / one group; 60 windows of 10 s with singletons / 100
groups.  For each, the default binning with 64 bins once over all series and once over one `ready_queue_len` column.  Each leg
ALTERNATES in the same process with its two comparison partners over the same cells: (a) `af_engine_summarize_series_windows`
(one streaming pass over the same sample rows) and (b) `af_engine_summarize_series_quantiles` at levels (0.5, 0.95, 0.99) over
the same columns.  Every figure is the host's wall time around the synchronous engine call (read-backs, host layout, the
zeroing of the outputs, all kernels) as min / median / max over --reps calls after one warm-up call of each; `scratch_bytes`
is the engine's scratch after the leg's first histogram call on a fresh engine.  Expectation to judge: (a) a small multiple of
one pass; (b) below 1 in every all-series row.
"""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

LEVELS = (0.5, 0.95, 0.99)
BINS = 64


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
    ready = res.series_names().index(next(k for k in res.series_names() if k.endswith("ready_queue_len")))

    def spread(ms: list[float]) -> dict:
        return {"min_ms": float(np.min(ms)), "median_ms": float(np.median(ms)), "max_ms": float(np.max(ms)),
                "tb_s": sample_bytes / (float(np.median(ms)) * 1e-3) / 1e12}

    out: dict = {"replicas": n, "ticks": float(ticks.sum()), "sample_gb": sample_bytes / 1e9, "series": S, "reps": args.reps,
                 "bins": BINS, "levels": list(LEVELS), "one_column": ready}
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
        for leg, columns in (("all_series", None), ("one_column", [ready])):
            Cn = S if columns is None else len(columns)
            qcount, hcount = (torch.empty((G, W), dtype=torch.int32, device=dev) for _ in range(2))
            quant = torch.empty((G, W, Cn, len(LEVELS)), dtype=torch.float64, device=dev)
            hist = torch.empty((G, W, Cn, BINS), dtype=torch.int32, device=dev)
            under, over = (torch.empty((G, W, Cn), dtype=torch.int32, device=dev) for _ in range(2))
            eng = Engine(plan, dev.index or 0)                    # a fresh engine: this leg's own scratch

            def yardstick() -> float:
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                eng.summarize_series_windows(
                    n, G, edges, samples_ptr=samples.data_ptr(), tick_capacity=cap, counts_ptr=counts.data_ptr(),
                    count_ptr=count.data_ptr(), mean_ptr=mean.data_ptr(), min_ptr=mn.data_ptr(), max_ptr=mx.data_ptr(),
                    above_ptr=ab.data_ptr(), group_ptr=grp.data_ptr())
                return (time.perf_counter() - t0) * 1e3

            def quantiles() -> float:
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                eng.summarize_series_quantiles(
                    n, G, edges, LEVELS, samples_ptr=samples.data_ptr(), tick_capacity=cap, counts_ptr=counts.data_ptr(),
                    quantiles_ptr=quant.data_ptr(), count_ptr=qcount.data_ptr(), group_ptr=grp.data_ptr(), columns=columns)
                return (time.perf_counter() - t0) * 1e3

            def histogram() -> tuple[float, int]:
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                _, scratch = eng.summarize_series_histogram(
                    n, G, edges, BINS, samples_ptr=samples.data_ptr(), tick_capacity=cap, counts_ptr=counts.data_ptr(),
                    hist_ptr=hist.data_ptr(), count_ptr=hcount.data_ptr(), under_ptr=under.data_ptr(), over_ptr=over.data_ptr(),
                    group_ptr=grp.data_ptr(), columns=columns)
                return (time.perf_counter() - t0) * 1e3, scratch

            first_ms, scratch = histogram()
            yardstick()
            quantiles()
            yard, qs, hs = [], [], []
            for _ in range(args.reps):
                yard.append(yardstick())
                qs.append(quantiles())
                hs.append(histogram()[0])
            assert torch.equal(hcount, count) and torch.equal(qcount, count)
            total = (hist.to(torch.int64) & 0xFFFFFFFF).sum(dim=-1) + (under.to(torch.int64) & 0xFFFFFFFF) + (over.to(torch.int64) & 0xFFFFFFFF)
            assert torch.equal(total, (count.to(torch.int64) & 0xFFFFFFFF)[:, :, None].expand_as(total))
            share_over = float((over.to(torch.int64) & 0xFFFFFFFF).sum()) / max(float(total.sum()), 1.0)
            out[f"{name}:{leg}"] = {"yardstick": spread(yard), "series_quantiles": spread(qs), "series_histogram": spread(hs),
                                    "vs_series_windows": float(np.median(hs) / np.median(yard)),
                                    "vs_series_quantiles": float(np.median(hs) / np.median(qs)), "first_call_ms": first_ms,
                                    "scratch_bytes": scratch, "cells": G * W, "share_over": share_over}
            print(f"{name}:{leg}", json.dumps(out[f"{name}:{leg}"]), file=sys.stderr, flush=True)   # (progress; the result is stdout's line)
            eng.close()
            del qcount, hcount, quant, hist, under, over
        del count, mean, mn, mx, ab
    print(json.dumps(out))


if __name__ == "__main__":
    main()
