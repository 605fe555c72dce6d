"""Arrivals per window and group on the device (`af_engine_summarize_arrivals`, asyncflow_amd/csrc/af_arrival_counts.hpp).

Every output word is an exact integer, so every comparison below is for equality: synthetic rows against
`np.searchsorted(side="right")`, generated rows against the sequential sampler on the host (`af::gen_next_gap` through
tests/hostcheck, and `asyncflow_amd.results.arrival_times`), and the whole against real runs of the same sweeps."""

from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from asyncflow_amd import _abi
from asyncflow_amd.plan import lower
from asyncflow_amd.results import arrival_times, arrival_window_counts
from oracle.scenarios import lb_two_servers, overload, single_server

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "asyncflow_amd" / "csrc" / "af_arrival_counts.hpp").read_text()
LDS_EDGES = int(re.search(r"constexpr\s+uint32_t\s+kMaxLdsEdges\s*=\s*(\d+)u?\s*;", HEADER).group(1))
SUM_ROWS = int(re.search(r"constexpr\s+uint32_t\s+kSumRows\s*=\s*(\d+)u?\s*;", HEADER).group(1))
INF = float("inf")
LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257]


def use_stream(span: int, n_win: int) -> bool:
    """afac::use_stream, restated: the tests must know which side of the rule a row is on"""
    return 8 * span < 64 * (n_win + 1) * max(int(span).bit_length(), 0)


def _groupings(n, rng):
    """(name, group ids or None, n_groups): singletons, one group, uneven groups, skipped members"""
    uneven = np.minimum((np.arange(n) ** 2) // max(n, 1), max(n // 3, 1) - 1 if n >= 3 else 0).astype(np.int64)
    skipped = rng.integers(0, 3, n).astype(np.int64)
    skipped[rng.random(n) < 0.3] = -1
    if n > 1:
        skipped[0] = -1
    return [("singletons", None, n), ("one", np.zeros(n, dtype=np.int64), 1), ("uneven", uneven, int(uneven.max()) + 2),   # (one group without members)
            ("skipped", skipped, 3)]


def _device(rows, group, n_groups, edges, *, engine=None, outputs=True):
    """Hand-made rows [n, cap] counted by the device (times_given = 1) -> arrivals [G, W], row_bounds [n, W + 1], generated [n],
    flags [n] as numpy."""
    import torch

    from asyncflow_amd.engine import Engine

    dev = torch.device("cuda", 0)
    n, cap = rows.shape
    n_win = len(edges) - 1
    times = torch.as_tensor(rows, device=dev)
    arr = torch.full((n_groups, n_win), -3, dtype=torch.int64, device=dev)
    rb = torch.full((n, n_win + 1), -1, dtype=torch.int32, device=dev)
    gen = torch.full((n,), -1, dtype=torch.int32, device=dev)
    flg = torch.full((n,), -1, dtype=torch.int32, device=dev)
    grp = None if group is None else torch.as_tensor(np.where(group < 0, _abi.POOL_SKIP, group).astype(np.uint32).view(np.int32), device=dev)
    eng = engine or Engine(lower(single_server(horizon=50)), 0)
    try:
        eng.summarize_arrivals(None, [], n_groups, edges, n=n, draw_capacity=cap, arrivals_ptr=arr.data_ptr(),
                               group_ptr=grp.data_ptr() if grp is not None else 0, row_bounds_ptr=rb.data_ptr() if outputs else 0,
                               generated_ptr=gen.data_ptr() if outputs else 0, flags_ptr=flg.data_ptr() if outputs else 0,
                               times_ptr=times.data_ptr(), times_given=True)
    finally:
        if engine is None:
            eng.close()
    assert np.array_equal(times.cpu().numpy().view(np.uint64), rows.view(np.uint64))      # given rows are read, never written
    return (arr.cpu().numpy().view(np.uint64), rb.cpu().numpy().view(np.uint32), gen.cpu().numpy().view(np.uint32),
            flg.cpu().numpy().view(np.uint32))


def _numpy(rows, group, n_groups, edges):
    n = rows.shape[0]
    n_win = len(edges) - 1
    arrivals = np.zeros((n_groups, n_win), dtype=np.uint64)
    bounds = np.zeros((n, n_win + 1), dtype=np.uint32)
    generated = np.zeros(n, dtype=np.uint32)
    for s in range(n):
        m = int(np.isfinite(rows[s]).sum())
        generated[s] = m
        bounds[s] = np.searchsorted(rows[s, :m], edges, side="right")
        g = s if group is None else int(group[s])
        if g >= 0:
            arrivals[g] += np.diff(bounds[s].astype(np.int64)).astype(np.uint64)
    return arrivals, bounds, generated


def _rows(rng, n, cap, lengths, hi):
    """n ascending rows of quarter-integer values in [0, hi) -- duplicates, values on integer edges -- +inf behind the last"""
    rows = np.full((n, cap), INF)
    for s in range(n):
        m = lengths[s % len(lengths)]
        rows[s, :m] = np.sort(rng.integers(0, max(int(4 * hi), 1), m).astype(np.float64) / 4.0)
    return rows


@pytest.mark.parametrize("n_win", [1, 2, 63, 64, 65, 600, LDS_EDGES - 1, LDS_EDGES])
def test_synthetic_rows_equal_searchsorted(n_win):
    """Row lengths around the wave's 64 and a full row, 1 / 3 / 130 scenarios (more than one workgroup of the bounds kernel, more
    than one run of the group sums), every grouping; W + 1 == kMaxLdsEdges is the last request with the edges in LDS, W + 1 ==
    kMaxLdsEdges + 1 the first that reads them from HBM.  Edges: on arrival values, e[0] above and e[W] below some arrivals, and
    wholly outside the rows."""
    from asyncflow_amd.engine import Engine

    rng = np.random.default_rng(4000 + n_win)
    cap = 300
    sides = set()
    eng = Engine(lower(single_server(horizon=50)), 0)
    try:
        for n in (1, 3, 130):
            lengths = [cap] if n == 1 else [*LENGTHS, cap]
            hi = float(n_win + 6)
            rows = _rows(rng, n, cap, lengths, hi)
            for shift in (2.0, 0.25, -hi - 1.0, hi + 1.0) if n == 3 else (2.0,):      # inside (on values / between), before and behind every row
                edges = np.arange(n_win + 1, dtype=np.float64) + shift
                for name, group, n_groups in _groupings(n, rng):
                    if n == 130 and name in ("one", "skipped") and n_win > 600:
                        continue                                                   # (the wide requests: two groupings are enough)
                    want = _numpy(rows, group, n_groups, edges)
                    got = _device(rows, group, n_groups, edges, engine=eng)
                    for what, g, w in zip(("arrivals", "row_bounds", "generated"), got, want):
                        assert np.array_equal(g, w), (what, n, name, shift)
                    assert not got[3].any()                                        # given rows carry no flag
                for s in range(n):
                    sides.add(use_stream(int(want[1][s, -1]) - int(want[1][s, 0]), n_win))
        arr_only = _device(rows, None, n, edges, engine=eng, outputs=False)[0]      # without the optional outputs: bounds in the scratch
        assert np.array_equal(arr_only, _numpy(rows, None, n, edges)[0])
    finally:
        eng.close()
    if n_win <= 2:
        assert sides == {False, True}                                              # short rows stream, the longer ones search


@pytest.mark.parametrize("n_win", [2, 64, 600])
def test_long_rows_on_both_sides_of_the_rule(n_win):
    """20 000 arrivals: 2 and 64 windows search (1 920 / 62 400 bytes of probes against 160 000 streamed), 600 stream."""
    rng = np.random.default_rng(77 + n_win)
    cap = 20000
    rows = _rows(rng, 5, cap, [cap, cap - 1, 5000, 0, 64 * 200 + 1], 610.0)
    edges = np.arange(n_win + 1, dtype=np.float64) * (600.0 / n_win) + 1.0
    group = np.array([1, 0, 1, -1, 0])
    want = _numpy(rows, group, 2, edges)
    got = _device(rows, group, 2, edges)
    for what, g, w in zip(("arrivals", "row_bounds", "generated"), got, want):
        assert np.array_equal(g, w), what
    assert use_stream(int(want[1][0, -1]) - int(want[1][0, 0]), n_win) == (n_win == 600)


def test_values_at_the_ends_of_the_number_line():
    rows = np.array([[0.0, 5e-324, 1.0, 1.7976931348623157e308, INF, INF],
                     [-0.0, 0.0, 0.0, 2.0 ** -1074, 2.0 ** 1023, 1.7976931348623157e308]])
    edges = np.array([-1.0, 0.0, 5e-324, 1.0, 1e308, 1.7976931348623157e308])
    want = _numpy(rows, None, 2, edges)
    got = _device(rows, None, 2, edges)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert got[2].tolist() == [4, 6]


# ---- generated rows ----------------------------------------------------------------------------------------------------------
def _normal_users(horizon=120):
    p = single_server(users=30, rpm=30, horizon=horizon)
    p["rqs_input"]["avg_active_users"] = {"mean": 30, "distribution": "normal", "variance": 12}
    p["rqs_input"]["user_sampling_window"] = 7
    return p


PLANS = {"single_server": single_server(50), "lb_two_servers": lb_two_servers(40), "normal_users": _normal_users()}
N_GEN = 70
_HOST: dict = {}


def _generated_case(name):
    """The sweep of a plan and its host definition (computed once, shared by the modes): 70 scenarios with their own users mean
    (one of them 0.0: nobody ever active), rpm and sampling window."""
    if name not in _HOST:
        from tests.hostcheck import build as hc

        plan = lower(PLANS[name])
        rng = np.random.default_rng(len(name))
        seeds = (np.uint64(0xA221) + np.arange(N_GEN, dtype=np.uint64) * np.uint64(7919)).astype(np.uint64)
        users = plan.gen_users_mean * rng.uniform(0.05, 1.0, N_GEN)
        users[5] = 0.0
        rpm = plan.gen_rpm_mean * rng.uniform(0.5, 1.2, N_GEN)
        window = rng.choice([1.0, 3.5, 60.0, 2.0 * plan.total_time], N_GEN)
        cap = int(plan.clock_capacity())
        rows = np.empty((N_GEN, cap))
        flags = np.zeros(N_GEN, dtype=np.uint32)
        for s in range(N_GEN):
            _n, rows[s], flags[s] = hc.arrivals(0, int(seeds[s]), dist=plan.gen_users_dist, mean=float(users[s]), sigma=plan.gen_users_sigma,
                                                rpm=float(rpm[s]), window_s=float(window[s]), horizon=plan.total_time, n_draw=cap)
        cols = [(_abi.PARAM_CODES["gen_users_mean"], 0, users), (_abi.PARAM_CODES["gen_rpm_mean"], 0, rpm),
                (_abi.PARAM_CODES["gen_window"], 0, window)]
        _HOST[name] = (plan, seeds, cols, cap, rows, flags)
    return _HOST[name]


def _generate(plan, seeds, cols, cap, group, n_groups, edges, *, engine_kw=None, keep_times=True):
    import torch

    from asyncflow_amd.engine import Engine

    dev = torch.device("cuda", 0)
    n, n_win = len(seeds), len(edges) - 1
    times = torch.full((n, cap), -1.0, dtype=torch.float64, device=dev) if keep_times else None
    arr = torch.full((n_groups, n_win), -3, dtype=torch.int64, device=dev)
    rb = torch.full((n, n_win + 1), -1, dtype=torch.int32, device=dev)
    gen = torch.full((n,), -1, dtype=torch.int32, device=dev)
    flg = torch.full((n,), -1, dtype=torch.int32, device=dev)
    grp = None if group is None else torch.as_tensor(np.where(group < 0, _abi.POOL_SKIP, group).astype(np.uint32).view(np.int32), device=dev)
    eng = Engine(plan, 0, **(engine_kw or {}))
    try:
        eng.summarize_arrivals(seeds, cols, n_groups, edges, draw_capacity=cap, arrivals_ptr=arr.data_ptr(),
                               group_ptr=grp.data_ptr() if grp is not None else 0, row_bounds_ptr=rb.data_ptr(),
                               generated_ptr=gen.data_ptr(), flags_ptr=flg.data_ptr(), times_ptr=times.data_ptr() if keep_times else 0)
    finally:
        eng.close()
    return (arr.cpu().numpy().view(np.uint64), rb.cpu().numpy().view(np.uint32), gen.cpu().numpy().view(np.uint32),
            flg.cpu().numpy().view(np.uint32), times.cpu().numpy() if keep_times else None)


@pytest.mark.parametrize("mode", ["rows", "groups"])
@pytest.mark.parametrize("name", list(PLANS))
def test_generated_rows_equal_the_host_definition(name, mode, monkeypatch):
    plan, seeds, cols, cap, rows, flags = _generated_case(name)
    monkeypatch.setenv("AF_PREGEN_MODE", mode)
    if mode == "groups":
        monkeypatch.setenv("AF_PREGEN_GROUP", "64")                 # 70 scenarios: a full workgroup and a short one
    edges = np.linspace(0.0, plan.total_time, 13)
    group = (np.arange(N_GEN) % 4).astype(np.int64)
    group[::9] = -1
    arr, rb, gen, flg, times = _generate(plan, seeds, cols, cap, group, 4, edges)
    assert np.array_equal(times.view(np.uint64), rows.view(np.uint64))          # the +inf tail included
    want = _numpy(rows, group, 4, edges)
    assert np.array_equal(arr, want[0]) and np.array_equal(rb, want[1]) and np.array_equal(gen, want[2])
    assert np.array_equal(flg, flags) and not flags.any()
    assert gen.max() > 1000 and (gen[5] == 0 or name == "normal_users")       # (a normal law around 0.0 users is positive half the time)
    # the engine's own scratch instead of the caller's buffer: the same words
    arr2, rb2, gen2, flg2, _ = _generate(plan, seeds, cols, cap, group, 4, edges, keep_times=False)
    assert np.array_equal(arr2, arr) and np.array_equal(rb2, rb) and np.array_equal(gen2, gen) and np.array_equal(flg2, flg)


def test_generated_rows_equal_the_python_definition():
    from oracle.rng_adapter import GeneratorRNG

    for name in PLANS:
        plan, seeds, cols, cap, rows, flags = _generated_case(name)
        for s in (5, 11):
            got, f = arrival_times(GeneratorRNG(int(seeds[s])), plan.gen_users_dist, float(cols[0][2][s]), plan.gen_users_sigma,
                                   float(cols[1][2][s]), float(cols[2][2][s]), plan.total_time, cap)
            assert np.array_equal(got.view(np.uint64), rows[s].view(np.uint64)) and f == flags[s]


# ---- against real runs ---------------------------------------------------------------------------------------------------------
def test_a_run_of_the_same_sweep_consumed_these_arrivals(tmp_path):
    from asyncflow_amd.results import load_summary
    from asyncflow_amd.runner import SimulationRunner

    n = 12
    seeds = 0xBEE0 + np.arange(n, dtype=np.uint64)
    sweep = {"rqs_input.avg_active_users.mean": np.linspace(20.0, 90.0, n), "rqs_input.user_sampling_window": np.tile([5.0, 60.0], n // 2)}
    res = SimulationRunner(simulation_input=lb_two_servers(horizon=40), seeds=seeds, sweep=sweep, device=0).run()
    by = np.arange(n) // 4
    summ = res.arrival_summary(window_s=5.0, by="scenario")
    assert np.array_equal(summ["generated"], res.counts[:, _abi.CNT_GENERATED]) and not summ["flags"].any()
    assert summ["arrivals"].dtype == np.uint64 and np.array_equal(summ["arrivals"].sum(axis=1), summ["generated"])   # (edges 0 .. T hold every arrival)
    assert np.all(summ["completed"] <= summ["arrivals"]) and np.array_equal(summ["lost"], summ["arrivals"].astype(np.int64) - summ["completed"])
    assert not summ["truncated"].any()
    for i in (0, 5, 11):
        times = res.arrival_times(i)
        one = res[i]
        assert times.shape[0] == one.total_generated and np.all(np.diff(times) > 0)
        assert np.isin(one.rqs_clock[:, 0].view(np.uint64), times.view(np.uint64)).all()          # every stored start, bit for bit
        counts = np.diff(arrival_window_counts(times, summ["edges"]))
        assert np.array_equal(counts, summ["arrivals"][i].astype(np.int64)) and np.array_equal(one.get_arrival_counts(5.0), counts)
    pooled = res.arrival_summary(window_s=5.0, by=by)
    for g in range(3):
        assert np.array_equal(pooled["arrivals"][g], summ["arrivals"][by == g].sum(axis=0))
        assert np.array_equal(pooled["completed"][g], summ["completed"][by == g].sum(axis=0))
    assert np.array_equal(pooled["offered_rps"], pooled["arrivals"].astype(np.int64) / (5.0 * 4))
    bands = res.arrival_bands(window_s=5.0, by=by)
    assert bands["mean"].shape == (3, 8, 2) and np.allclose(bands["mean"][:, :, 0], summ["offered_rps"].reshape(3, 4, 8).mean(axis=1))
    cols = res.save_arrival_summary(str(tmp_path / "arrivals.npz"), by, window_s=5.0, thresholds=[0.05])
    back = load_summary(str(tmp_path / "arrivals.npz"))
    assert np.array_equal(back["arrivals"], pooled["arrivals"].astype(np.int64)) and np.array_equal(back["within:0"], cols["within:0"])


def test_overload_slo_share_against_arrivals():
    """overload(30): most requests never come back; the share within 200 ms of the requests SENT is far below the share of the
    completions that quantile_summary reports."""
    from asyncflow_amd.runner import SimulationRunner
    from tests.hostcheck import build as hc

    n = 6
    seeds = np.array([1, 42, 777, 5, 6, 7], dtype=np.uint64)
    res = SimulationRunner(simulation_input=overload(30), seeds=seeds, device=0).run()
    plan = res.plan
    by = np.array([0, 0, 0, 1, 1, 1])
    summ = res.arrival_summary(window_s=5.0, by=by, thresholds=[0.2])
    edges = summ["edges"]
    arrivals = np.zeros((2, 6), dtype=np.int64)
    within = np.zeros((2, 6), dtype=np.int64)
    completed = np.zeros((2, 6), dtype=np.int64)
    for i in range(n):
        _m, times, _f = hc.arrivals(0, int(seeds[i]), dist=plan.gen_users_dist, mean=plan.gen_users_mean, sigma=plan.gen_users_sigma,
                                    rpm=plan.gen_rpm_mean, window_s=plan.gen_window_s, horizon=plan.total_time, n_draw=res.draw_capacity)
        arrivals[by[i]] += np.diff(arrival_window_counts(times, edges))
        ck = res[i].rqs_clock
        w = np.searchsorted(edges, ck[:, 0], side="left") - 1                      # edges[w] < start <= edges[w + 1]
        ok = (w >= 0) & (w < 6)
        completed[by[i]] += np.bincount(w[ok], minlength=6)
        within[by[i]] += np.bincount(w[ok & (ck[:, 1] - ck[:, 0] <= 0.2)], minlength=6)
    assert res.counts[0, _abi.CNT_GENERATED] == 3718 and res.counts[0, _abi.CNT_COMPLETED] == 719
    assert np.array_equal(summ["arrivals"].astype(np.int64), arrivals) and np.array_equal(summ["completed"], completed)
    assert np.array_equal(summ["within"][:, :, 0], within)
    host_share = np.where(arrivals > 0, within / np.maximum(arrivals, 1), np.nan)
    assert np.array_equal(summ["within_share"][:, :, 0], host_share, equal_nan=True)
    of_completions = res.quantile_summary([], thresholds=[0.2], window_s=5.0, by=by, window_of="arrival")["share"].cpu().numpy()[:, :, 0]
    lossy = (summ["lost"] > 0) & (within > 0)
    # (the server saturates within seconds: only the first windows' cohorts hold a request that came back within 200 ms)
    assert lossy.any(axis=1).all() and np.all(summ["within_share"][:, :, 0][lossy] < of_completions[lossy])
    assert np.nansum(within) / arrivals.sum() < 0.5 * np.nansum(within) / completed.sum()


# ---- overflow, chunks ----------------------------------------------------------------------------------------------------------
def test_a_full_row_is_flagged_and_holds_the_prefix():
    plan, seeds, _cols, cap, _rows_, _flags = _generated_case("single_server")
    edges = np.array([0.0, 10.0, 100.0, plan.total_time])
    seeds = seeds[:9]
    full = _generate(plan, seeds, [], cap, None, 9, edges)
    cut = _generate(plan, seeds, [], 200, None, 9, edges)
    assert np.all(cut[2] == 200) and np.all(cut[3] == _abi.FLAG_DRAW_OVERFLOW) and not full[3].any() and np.all(full[2] > 200)
    assert np.array_equal(cut[4].view(np.uint64), full[4][:, :200].view(np.uint64))
    want = _numpy(cut[4], None, 9, edges)
    assert np.array_equal(cut[0], want[0]) and np.array_equal(cut[1], want[1])


def test_chunks_of_a_small_memory_budget_return_the_same_words():
    plan, seeds, cols, _cap, _rows_, _flags = _generated_case("normal_users")
    cap = 2048                                                       # 16 KB a row: 64 rows fit 1 MiB, 70 do not
    assert N_GEN * cap * 8 > 1 << 20
    edges = np.linspace(3.0, 100.0, 66)
    group = (np.arange(N_GEN) * 5 // N_GEN).astype(np.int64)          # groups that straddle the chunks
    for grp, n_groups in ((group, 5), (None, N_GEN)):
        one = _generate(plan, seeds, cols, cap, grp, n_groups, edges, keep_times=False)
        two = _generate(plan, seeds, cols, cap, grp, n_groups, edges, engine_kw={"draw_memory_mb": 1}, keep_times=False)
        for a, b in zip(one[:4], two[:4]):
            assert np.array_equal(a, b)
        assert one[0].sum() > 1000


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_error_codes():
    import torch

    from asyncflow_amd.engine import Engine

    dev = torch.device("cuda", 0)
    n, cap = 4, 64
    plan = lower(single_server(horizon=20))
    arr = torch.full((n, 3), -3, dtype=torch.int64, device=dev)
    grp = torch.as_tensor(np.array([0, 1, 7, 1], dtype=np.int32), device=dev)
    seeds = (C.c_uint64 * n)(1, 2, 3, 4)
    pd = C.POINTER(C.c_double)

    def call(eng, *, edges=(0.0, 5.0, 10.0, 20.0), n_win=3, draw=cap, arrivals=arr.data_ptr(), group=0, n_groups=n, n_req=n, seeds_p=seeds):
        e = np.asarray(edges, dtype=np.float64)
        sweep = _abi.AfSweep(n, seeds_p, 0, None, draw)
        req = _abi.AfArrivals(n_req, n_groups, n_win, C.c_void_p(group or None), e.ctypes.data_as(pd), None, 0, C.c_void_p(arrivals or None),
                              None, None, None, 0.0, 0)
        return eng._lib.af_engine_summarize_arrivals(eng._h, C.byref(sweep), C.byref(req))   # noqa: SLF001

    eng = Engine(plan, 0)
    small = Engine(plan, 0, draw_memory_mb=1)
    only_plan = Engine(plan, _abi.DEVICE_PLAN_ONLY)
    try:
        assert call(eng) == _abi.AF_OK
        assert call(eng, edges=(0.0, 5.0, 5.0, 20.0)) == _abi.AF_ERR_INVALID
        assert call(eng, edges=(0.0, 5.0, float("nan"), 20.0)) == _abi.AF_ERR_INVALID
        assert call(eng, edges=(0.0, 5.0, 10.0, INF)) == _abi.AF_ERR_INVALID
        assert call(eng, group=grp.data_ptr(), n_groups=2) == _abi.AF_ERR_INVALID          # group id 7 of 2
        assert call(eng, n_win=0) == _abi.AF_ERR_INVALID
        assert call(eng, draw=0) == _abi.AF_ERR_INVALID
        assert call(eng, arrivals=0) == _abi.AF_ERR_INVALID
        assert call(eng, n_groups=2) == _abi.AF_ERR_INVALID                                # singletons need n_groups == n
        assert call(eng, n_req=3) == _abi.AF_ERR_INVALID
        assert call(eng, seeds_p=None) == _abi.AF_ERR_INVALID
        assert call(small, draw=200000) == _abi.AF_ERR_CAPACITY                            # one row of 1.6 MB against a budget of 1 MiB
        assert call(only_plan) == _abi.AF_ERR_NO_DEVICE
        assert (arr.cpu().numpy() >= 0).all()                                              # (the one good call wrote; none of the refused did)
    finally:
        eng.close()
        small.close()
        only_plan.close()
