"""Cells across devices on BASELINE config 2's batch (10 000 LB-2 replicas, T = 600 s): one JSON line.

    python scripts/measure_sharded_cells.py [--replicas 10000] [--reps 5]

The same sweep is run twice in one process: unsharded, and with `devices=[0, 0]` (two shards on one card: the export, the
concatenation and the merge are all there, the link between two cards is not).  Per case the sharded call ALTERNATES with the
unsharded call over the same groups and windows: `pooled_summary` with one group and with 100 groups, `window_summary` with 100
groups x 60 windows of 10 s, `quantile_summary` (p50 / p99 / p99.9, one threshold) with 100 groups x 60 windows.  Every figure
is the wall time of the whole Python call up to a device synchronisation (for the sharded call: both exports, `torch.cat`, the
metadata on the host, merge and reduction) as min / median / max over --reps calls after one warm-up call.  `model_ms` is what
the sharded call moves beyond the unsharded one -- the export writes 8 B, the concatenation moves 16 B and the merge moves 16 B
per windowed latency -- at 4 TB/s; `reducing_device_bytes` the 16 B per windowed latency its device holds for the import and the
merged cells.  The outputs of both calls are compared word for word before anything is timed.
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

    from asyncflow_amd.runner import SimulationRunner
    from asyncflow_amd.workloads import lb_two_servers

    payload = lb_two_servers()
    seeds = 0xC0F30000 + np.arange(args.replicas, dtype=np.uint64)
    one = SimulationRunner(simulation_input=payload, seeds=seeds).run()
    two = SimulationRunner(simulation_input=payload, seeds=seeds, devices=[0, 0]).run()
    n = len(one)
    ids = np.arange(n) % 100                                  # (the shards are contiguous halves: every group has members in both)

    def timed(call) -> tuple[float, dict]:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def spread(ms: list[float]) -> dict:
        return {"min_ms": float(np.min(ms)), "median_ms": float(np.median(ms)), "max_ms": float(np.max(ms))}

    cases = {
        "pooled_one_group": (lambda r: r.pooled_summary(None), "stats"),
        "pooled_groups_100": (lambda r: r.pooled_summary(ids), "stats"),
        "windows_groups_100_x60": (lambda r: r.window_summary(10.0, by=ids), "stats"),
        "quantiles_groups_100_x60": (lambda r: r.quantile_summary([0.5, 0.99, 0.999], thresholds=[0.05], window_s=10.0, by=ids), "quantiles"),
    }
    out: dict = {"replicas": n, "reps": args.reps, "shards": [len(s) for s in two.shards]}
    for name, (call, key) in cases.items():
        one.close()
        for s in two.shards:
            s.close()                                         # fresh analyzer engines: this case's own scratch
        _, want = timed(lambda: call(one))
        _, got = timed(lambda: call(two))
        a, b = want[key].cpu().numpy().view(np.uint64), got[key].cpu().numpy().view(np.uint64)
        assert np.array_equal(a, b), name
        windowed = float(want["stats"][..., 0].sum()) if "stats" in want else float(want["count"].sum())
        plain, sharded = [], []
        for _ in range(args.reps):
            plain.append(timed(lambda: call(one))[0])
            sharded.append(timed(lambda: call(two))[0])
        out[name] = {"unsharded": spread(plain), "sharded": spread(sharded), "sharded_minus_unsharded_ms": float(np.median(sharded) - np.median(plain)),
                     "windowed_latencies": windowed, "model_ms": 40.0 * windowed / 4e12 * 1e3, "reducing_device_bytes": 16.0 * windowed,
                     "scratch_bytes": int(got.get("scratch_bytes", 0))}
        del want, got
    print(json.dumps(out))


if __name__ == "__main__":
    main()
