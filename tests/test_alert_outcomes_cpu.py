"""Alert rules on request outcomes on the host: `asyncflow_amd.results.outcome_ticks` -- the counting definition
af_engine_outcome_alerts is held to -- against an independent JOIN of the arrivals to the in-time rows on the bit
pattern of `start` (tests/alert_outcomes_util.py), on synthetic rows and on CPU-oracle runs of a scenario with edge dropout and of
one with an injected outage; the edge cases of the definition; the chain into the rules; the refusals; the plumbing of the header
through the source lists and the ABI.  Every expectation is an exact integer."""

from __future__ import annotations

import copy
import ctypes as C
import inspect
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import asyncflow_amd
from asyncflow_amd import _abi
from asyncflow_amd.plan import lower
from asyncflow_amd.results import (BatchedResults, ScenarioResults, ShardedResults, alert_firing, alert_window_stats, arrival_times,
                                   completion_ticks, outcome_ticks, scenario_alerts, scenario_outcome_alerts)
from oracle import oracle_lib as ol
from oracle.rng_adapter import GeneratorRNG
from oracle.scenarios import lb_two_servers, lb_with_events
from tests.alert_outcomes_util import SLO, TAU, P, arrival_row, join_outcomes, rows_from

ROOT = Path(__file__).resolve().parent.parent
KEYS = ("total", "bad", "timeouts", "completions")
INF = float("inf")


def _same(got: dict, want: dict) -> None:
    for k in KEYS:
        assert got[k].dtype == np.uint32 and np.array_equal(got[k], want[k]), k
    assert got["timed_out"] == want["timed_out"] and want["excess"] == 0 and got["deficit"] == 0


def test_counting_definition_is_the_join_on_synthetic_rows():
    rng = np.random.default_rng(41)
    seen = 0
    for n_arr, m, t_s in ((0, 0, 5), (1, 0, 3), (1, 1, 3), (64, 40, 20), (65, 65, 20), (800, 500, 70), (6000, 5000, 300)):
        arr = arrival_row(rng, n_arr, t_s, n_arr + 3)
        rows = rows_from(rng, arr, m)
        fin = arr[np.isfinite(arr)]
        if n_arr > 3:
            assert fin[1] == fin[2] and (fin < 0).any()                  # two arrivals of one bit pattern, arrivals below 0
        for slo, tau in ((SLO, TAU), (INF, TAU), (SLO, P / 4), (2 * TAU, TAU), (SLO, (t_s + 5) * P), (0.0, 3 * P)):
            own = rows_from(rng, arr, m, tau)
            for r in (rows, own):
                got = outcome_ticks(r, arr, t_s, P, slo, tau)
                _same(got, join_outcomes(r, arr, t_s, P, slo, tau))
                seen += got["timed_out"]
                if slo == INF:
                    assert np.array_equal(got["bad"], got["timeouts"])   # a pure availability alert
                if tau >= (t_s + 5) * P:
                    assert got["timed_out"] <= int((fin < -4 * P).sum())  # beyond the run: only arrivals far below 0 time out inside it
    assert seen > 10000


def _oracle_replicas(payload: dict, seeds) -> tuple:
    """CPU-oracle runs of one payload and each seed's arrival row, as tests/test_paired_cpu.py obtains them."""
    plan = lower(payload)
    out = []
    for seed in seeds:
        run = ol.simulate(plan, seed)
        times, flags = arrival_times(GeneratorRNG(seed), plan.gen_users_dist, plan.gen_users_mean, plan.gen_users_sigma, plan.gen_rpm_mean,
                                     plan.gen_window_s, plan.total_time, plan.clock_capacity())
        assert flags == 0
        ticks = min(int(run.counts[_abi.CNT_TICKS]), plan.tick_count)
        out.append((run.clock, times, ticks, run))
    return plan, out


def _split_share(peaks: list) -> Fraction:
    """A share strictly inside the replicas' peaks: the replicas above it fire, the others do not."""
    levels = sorted(set(peaks))
    assert len(levels) > 1, "every replica has the same largest rolling bad share"
    return levels[(len(levels) - 1) // 2]


def _peak_share(total, bad, look: int) -> Fraction:
    pt, pb = np.cumsum(total.astype(np.int64)), np.cumsum(bad.astype(np.int64))
    best = Fraction(0)
    for k in range(len(pt)):
        t = int(pt[k] - (pt[k - look] if k >= look else 0))
        if t >= 5:
            best = max(best, Fraction(int(pb[k] - (pb[k - look] if k >= look else 0)), t))
    return best


def lossy(horizon: int = 20) -> dict:
    p = lb_two_servers(users=120, horizon=horizon)
    for e in p["topology_graph"]["edges"]:
        if e["id"] in ("client-lb", "srv2-client"):
            e["dropout_rate"] = 0.04
    return p


def test_counting_definition_is_the_join_on_oracle_runs_with_dropout_and_with_an_outage():
    tau = 0.75
    for payload, must_drop in ((lossy(), True), (lb_with_events(users=150, horizon=60, scale=0.1), False)):
        plan, reps = _oracle_replicas(payload, range(40, 46))
        p = plan.sample_period
        look = int(round(2.0 / p))
        peaks, outs = [], []
        for clock, times, ticks, run in reps:
            assert clock.shape[0] > 300
            for slo in (0.03, INF):
                got = outcome_ticks(clock, times, ticks, p, slo, tau)
                _same(got, join_outcomes(clock, times, ticks, p, slo, tau))       # deficit == 0: the run's own arrival row
            if must_drop:
                assert run.dropped > 0 and got["timed_out"] > 0
            assert int(got["total"].sum()) <= int(np.isfinite(times).sum())
            peaks.append(_peak_share(got["total"], got["bad"], look))
            outs.append(got)
        # an availability rule (slo = +inf) whose share lies inside the replicas' peaks: it fires in some replicas, not in all
        share = _split_share(peaks)
        rule = [(look, look, share.numerator, share.denominator, 5, 1)]
        fired = []
        for (clock, times, ticks, _), got in zip(reps, outs):
            full = scenario_outcome_alerts(clock, times, ticks, p, INF, tau, rule, [0, plan.tick_count])
            assert np.array_equal(full["total"], got["total"]) and full["deficit"] == 0
            assert np.array_equal(full["firing"], alert_firing(got["total"], got["bad"], rule)["firing"])
            assert np.array_equal(full["fired"], alert_window_stats(full["firing"], [0, plan.tick_count])["fired"])
            fired.append(int(full["fired"][0, 0]) > 0)
            assert not scenario_alerts(clock, ticks, p, INF, rule, [0, plan.tick_count])["firing"].any()   # completions only: never
        assert any(fired) and not all(fired), fired


def test_edge_cases_of_the_definition():
    none = np.zeros((0, 2))
    # the timeout lands on tick t_s - 1 and on t_s
    t_s = 10
    arr = np.array([(t_s - 1) * P - TAU, t_s * P - TAU - P / 8, t_s * P - TAU, np.inf])
    got = outcome_ticks(none, arr, t_s, P, SLO, TAU)
    assert got["timeouts"].tolist() == [0] * 9 + [2] and got["timed_out"] == 2 and got["deficit"] == 0
    # m = 0 and an arrival row that is all +inf; no ticks
    assert outcome_ticks(none, np.full(7, np.inf), 5, P, SLO, TAU)["total"].tolist() == [0] * 5
    empty = outcome_ticks(np.array([[0.0, 0.1]]), [0.0], 0, P, SLO, TAU)
    assert empty["total"].shape == (0,) and empty["deficit"] == 0 and empty["timed_out"] == 0
    # rows foreign to the arrival row: deficit > 0, and the result is still defined
    rows = np.array([[1 * P, 2 * P], [3 * P, 3 * P + TAU], [5 * P, 5 * P + TAU + P / 8]])
    got = outcome_ticks(rows, np.full(4, np.inf), 40, P, SLO, TAU)
    assert got["deficit"] == 2 and got["timed_out"] == 0 and got["total"].sum() == 2 and got["total"][2] == 1 and got["total"][19] == 1
    got = outcome_ticks(rows, [1 * P, 5 * P, 9 * P], 40, P, SLO, TAU)
    assert got["deficit"] == 1 and got["timeouts"][[21, 25]].tolist() == [1, 1] and got["timed_out"] == 2      # the late row: a timeout, never a completion
    assert got["bad"].sum() == 3 and got["completions"].sum() == 2                                                # lat == tau > slo: in time and bad
    # NaN rows are no completions: their arrivals time out
    arr = np.array([0.0, P, 2 * P])
    got = outcome_ticks(np.array([[0.0, np.nan], [np.nan, 1.0], [2 * P, 3 * P], [np.inf, 1.0], [-np.inf, -np.inf]]), arr, 40, P, SLO, TAU)
    assert got["timeouts"][[16, 17, 18]].tolist() == [1, 1, 0] and got["completions"].tolist()[3] == 1 and got["completions"][32] == 1
    assert got["deficit"] == 0                                           # (start = +inf is in time -- lat = -inf -- with no timeout tick)
    # tau below one tick: the timeout lands on the arrival's own tick; slo above tau: no completion is bad
    arr = np.array([0.0, P + P / 2, 7 * P])
    got = outcome_ticks(np.array([[0.0, P / 8]]), arr, 8, P, SLO, P / 4)
    assert got["total"].tolist() == [1, 1, 0, 0, 0, 0, 0, 1] and got["bad"].tolist() == [0, 1, 0, 0, 0, 0, 0, 1]
    got = outcome_ticks(np.array([[0.0, TAU], [P, P + TAU + P]]), [0.0, P], 40, P, 2 * TAU, TAU)
    assert got["bad"].tolist() == got["timeouts"].tolist() and got["timed_out"] == 1 and got["completions"][16] == 1
    # the counts do not depend on the order of the rows
    rng = np.random.default_rng(43)
    arr = arrival_row(rng, 300, 50)
    rows = rows_from(rng, arr, 200)
    a, b = outcome_ticks(rows, arr, 50, P, SLO, TAU), outcome_ticks(rows[::-1], arr, 50, P, SLO, TAU)
    assert all(np.array_equal(a[k], b[k]) for k in KEYS)
    # without a timeout that bites the completions are completion_ticks's
    done = rows[~np.isnan(rows).any(axis=1)]
    done = done[done[:, 1] - done[:, 0] <= TAU]
    assert np.array_equal(a["completions"], completion_ticks(done, 50, P, SLO)["total"])


def test_refusals():
    rows, arr = np.array([[0.0, 0.1]]), [0.0, 1.0]
    for bad in (0.0, -1.0, float("nan"), INF, None, True, "x"):
        with pytest.raises(ValueError, match="timeout"):
            outcome_ticks(rows, arr, 5, P, SLO, bad)
    with pytest.raises(ValueError, match="ascending"):
        outcome_ticks(rows, [1.0, 0.0], 5, P, SLO, TAU)
    with pytest.raises(ValueError, match="ascending"):
        outcome_ticks(rows, [0.0, np.nan, 1.0], 5, P, SLO, TAU)
    with pytest.raises(ValueError, match="NaN"):
        outcome_ticks(rows, arr, 5, P, float("nan"), TAU)
    with pytest.raises(ValueError, match="period"):
        outcome_ticks(rows, arr, 5, 0.0, SLO, TAU)
    with pytest.raises(ValueError, match="ticks"):
        outcome_ticks(rows, arr, -1, P, SLO, TAU)
    one = ScenarioResults(lower(lb_two_servers(horizon=5)), np.zeros(_abi.CNT_SLOTS, dtype=np.uint64), np.zeros((0, 2)), None)
    with pytest.raises(ValueError, match="arrival times"):
        one.get_alerts(SLO, [(5, 5, 1, 2, 0, 1)], timeout_s=1.0)
    assert one.get_alerts(SLO, [(5, 5, 1, 2, 0, 1)])["total"].sum() == 0


def test_header_is_registered_and_the_abi_mirrors_the_struct():
    from asyncflow_amd import build as af_build
    from asyncflow_amd import jit

    assert "af_alert_outcomes.hpp" in af_build.SOURCES and "af_alert_outcomes.hpp" in jit._SOURCES  # noqa: SLF001
    assert '"af_alert_outcomes.hpp"' in (ROOT / "asyncflow_amd/csrc/engine.hip").read_text()
    header = (ROOT / "include/asyncflow_hip.h").read_text()
    body = re.search(r"typedef struct af_alert_outcomes \{(.*?)\} af_alert_outcomes_t;", header, re.S).group(1)
    decl = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.search(r"(\w+)\s*$", part).group(1) for stmt in decl.split(";") if stmt.strip() for part in stmt.split(",")]
    assert names == [f[0] for f in _abi.AfAlertOutcomes._fields_], names  # noqa: SLF001
    assert C.sizeof(_abi.AfAlertOutcomes) == 64
    assert int(re.search(r"#define AF_OUTCOME_ROWS_TRUNCATED (\d+)u", header).group(1)) == _abi.OUTCOME_ROWS_TRUNCATED
    assert int(re.search(r"#define AF_OUTCOME_DEFICIT (\d+)u", header).group(1)) == _abi.OUTCOME_DEFICIT
    assert "af_engine_outcome_alerts" in _abi.EXPORTED_SYMBOLS
    for fn in (BatchedResults.alert_summary, ScenarioResults.get_alerts, ShardedResults.alert_summary):
        assert inspect.signature(fn).parameters["timeout_s"].default is None
    assert asyncflow_amd.outcome_ticks is outcome_ticks and asyncflow_amd.scenario_outcome_alerts is scenario_outcome_alerts
    # the definition stands in the same words in the C header, the kernel header and the host definition
    for text in (header, (ROOT / "asyncflow_amd/csrc/af_alert_outcomes.hpp").read_text(), inspect.getdoc(outcome_ticks)):
        flat = re.sub(r"[\s/*`]+", " ", text)
        for phrase in ("max(A[k] - G[k], 0)", "max(G[k] - A[k], 0)", "C[k] + timeouts[k]", "Cbad[k] + timeouts[k]", "<= tau"):
            assert phrase in flat, phrase
    assert copy.deepcopy(lossy())["topology_graph"]["edges"][1]["dropout_rate"] == 0.04
