"""Alert rules on request outcomes on BASELINE config 2's batch (10 000 LB-2 replicas, T = 600 s): one JSON line.

    python scripts/measure_alert_outcomes.py [--replicas 10000] [--reps 5] [--timeout 2.0] [--no-yardstick]

Every case ALTERNATES, in the same process, `af_engine_outcome_alerts` with `af_engine_summarize_alerts` over the same
windows, groups and rules -- the yardstick: the completions-only call, whose evaluation kernel is the same code.  The arrival rows
are regenerated once beforehand (`af_engine_summarize_arrivals` with a `times` buffer; its time is reported as `arrival_ms`, it is
not part of a case).  Cases: the shapes of scripts/measure_alerts.py -- 1 / 4 / 32 rules, one window / 60 windows of 10 s / 600
windows of 1 s, each with singleton groups / 100 groups / one group.  Every cell output and the per-scenario `timed_out`, `deficit`
and `flags` are asked for, the per-tick outputs are not.  Every figure is the wall time of the synchronous engine call, started
after a device synchronisation, as min / median / max over --reps calls after one warm-up call of each.  Model, not a gate: the
prefix kernel streams the arrival rows beside the clock rows, so a call with one rule lands near the yardstick times `model_ratio`
= (clock rows + arrival rows) / clock rows in bytes, the arrival rows counted up to the last finite entry's 16-byte pair.
--no-yardstick repeats the call back to back without the other one in between.
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
    ap.add_argument("--timeout", type=float, default=2.0, help="the client timeout in seconds")
    ap.add_argument("--no-yardstick", action="store_true", help="do not alternate with af_engine_summarize_alerts")
    args = ap.parse_args()

    import torch

    from asyncflow_amd import _abi, alert_rule
    from asyncflow_amd.results import check_alert_rules, tick_window_edges
    from asyncflow_amd.runner import SimulationRunner
    from asyncflow_amd.workloads import lb_two_servers

    res = SimulationRunner(simulation_input=lb_two_servers(), replicas=args.replicas).run()
    n, plan = len(res), res.plan
    p, ticks = float(plan.sample_period), int(plan.tick_count)
    clock, counts = res._clock_t, res._counts_t   # noqa: SLF001
    dev = clock.device
    clock_bytes = 16.0 * float(np.minimum(res.counts[:, _abi.CNT_COMPLETED].astype(np.int64), clock.shape[1]).sum())
    tick_cap = res._in_flight_ticks()   # noqa: SLF001
    eng, _ = res._arrival_engine()   # noqa: SLF001
    lat = res[0].rqs_clock
    slo = float(np.quantile(lat[:, 1] - lat[:, 0], 0.9))          # a tenth of the requests of a plain run is bad

    torch.cuda.synchronize(dev)
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    times, time_row, n_rows, draw_cap = res._outcome_rows(eng, dev)   # noqa: SLF001
    t1.record()
    torch.cuda.synchronize(dev)
    arrivals = torch.isfinite(times).sum(dim=1)
    arrival_bytes = 8.0 * float(arrivals.sum().item())
    words = {k: torch.empty((n,), dtype=torch.int32, device=dev) for k in ("timed_out", "deficit", "flags")}
    oc = {"times_ptr": times.data_ptr(), "time_row_ptr": time_row.data_ptr(), "n_time_rows": n_rows, "draw_capacity": draw_cap,
          "timeout": float(args.timeout), **{k: v.data_ptr() for k, v in words.items()}}

    def spread(ms: list[float]) -> dict:
        return {"min_ms": float(np.min(ms)), "median_ms": float(np.median(ms)), "max_ms": float(np.max(ms))}

    first = alert_rule(60.0, 5.0, objective=0.9, burn_rate=1.5, hold_s=3 * p)
    more = [alert_rule(10.0 * (1 + j % 6), 1.0 + j % 5, bad_share=(5 + j) / 100.0, hold_s=(1 + j % 4) * p, min_total=10) for j in range(31)]
    rule_sets = (("r1", check_alert_rules([first], p)), ("r4", check_alert_rules([first] + more[:3], p)), ("r32", check_alert_rules([first] + more, p)))
    out: dict = {"replicas": n, "latencies": clock_bytes / 16.0, "clock_gb": clock_bytes / 1e9, "arrival_gb": arrival_bytes / 1e9,
                 "arrival_rows": n_rows, "draw_capacity": draw_cap, "times_gb": 8.0 * n_rows * draw_cap / 1e9,
                 "model_ratio": (clock_bytes + arrival_bytes) / clock_bytes, "ticks": ticks, "tick_capacity": tick_cap,
                 "prefix_gb": 8.0 * n * tick_cap / 1e9, "slo_s": slo, "timeout_s": float(args.timeout), "reps": args.reps,
                 "arrival_ms": float(t0.elapsed_time(t1))}
    groupings = (("singletons", np.arange(n), n), ("groups_100", np.arange(n) // max(n // 100, 1), int((n - 1) // max(n // 100, 1)) + 1),
                 ("one_group", np.zeros(n, dtype=np.int64), 1))
    windows = (("x1", np.array([0, tick_cap], dtype=np.uint32)), ("x60", tick_window_edges(round(10.0 / p), ticks)),
               ("x600", tick_window_edges(round(1.0 / p), ticks)))
    for wname, b in windows:
        n_win = int(b.shape[0] - 1)
        for gname, ids, n_groups in groupings:
            grp = torch.from_numpy(ids.astype(np.uint32).view(np.int32)).to(dev)
            for rname, r6 in rule_sets:
                n_rules = int(r6.shape[0])
                t = {"count": torch.empty((n, n_win), dtype=torch.int32, device=dev)}
                for k in ("fired", "episodes", "longest", "longest_start", "first", "last"):
                    t[k] = torch.empty((n, n_win, n_rules), dtype=torch.int32, device=dev)
                for k in ("members", "fired_members", "open_members"):
                    t[k] = torch.empty((n_groups, n_win, n_rules), dtype=torch.int32, device=dev)
                for k in ("fire_ticks", "fire_episodes"):
                    t[k] = torch.empty((n_groups, n_win, n_rules), dtype=torch.int64, device=dev)
                t["delay_hist"] = torch.empty((n_groups, n_win, n_rules, 4), dtype=torch.int32, device=dev)
                ptrs = {k: v.data_ptr() for k, v in t.items()}

                def call(outcomes: dict | None) -> float:
                    torch.cuda.synchronize(dev)                   # nothing of the call before is still running
                    ms, _ = eng.summarize_alerts(n, n_groups, b, p, slo, r6, clock_ptr=clock.data_ptr(), clock_capacity=int(clock.shape[1]),   # noqa: B023
                                                 tick_capacity=tick_cap, counts_ptr=counts.data_ptr(), group_ptr=grp.data_ptr(),   # noqa: B023
                                                 delay_bins=4, delay_width=100, ptrs=ptrs, outcomes=outcomes)   # noqa: B023
                    return float(ms)

                call(oc)
                if not args.no_yardstick:
                    call(None)
                mine, theirs = [], []
                for _ in range(args.reps):
                    mine.append(call(oc))
                    fired = int(t["fired_members"].sum().item())
                    theirs.append(float("nan") if args.no_yardstick else call(None))
                med = float(np.median(mine))
                out[f"{gname}_{wname}_{rname}"] = {
                    "outcome_alerts": spread(mine), "alerts": spread(theirs), "ratio": med / float(np.median(theirs)),
                    "pass_tb_s": (clock_bytes + arrival_bytes) / (med * 1e-3) / 1e12, "cells": n_groups * n_win * n_rules,
                    "fired_members": fired, "timed_out": int(words["timed_out"].to(torch.int64).sum().item()),
                    "deficit": int(words["deficit"].to(torch.int64).sum().item()), "flags": int(words["flags"].max().item())}
                del t, ptrs
            del grp
    print(json.dumps(out))


if __name__ == "__main__":
    main()
