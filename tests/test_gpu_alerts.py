"""Burn-rate alert rules on the MI355X (af_engine_summarize_alerts, asyncflow_amd/csrc/af_alerts.hpp): every output word against
the host definition (results.scenario_alerts per scenario, results.alert_cells per group).  Synthetic clocks through the C ABI,
with the dyadic period 2^-5 and a bad share that comes and goes in phases: row counts on the wave seams, tick counts on the
64-tick seams and on both sides of the kernel's chunk and of twice it, look-backs across a chunk seam and longer than the run,
1 and 32 rules with every hold, all rows bad and none, window and group arrangements, the delay histogram, every optional output
absent in turn, every refusal, and the independence of the launch.  Every output of a call lies in ONE buffer with sentinel
words on both sides of each.  An event workload goes through the Python API, unsharded and in two shards."""

from __future__ import annotations

import ctypes as C
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from asyncflow_amd import _abi, alert_delay_quantiles, alert_rule
from asyncflow_amd.plan import lower
from asyncflow_amd.results import alert_cells, check_alert_rules, completion_ticks, load_summary, scenario_alerts
from oracle.scenarios import lb_with_events, single_server
from tests.alerts_util import HOLDS, SLO, P, firing_words, rows_in_phases, rules_32, rules_few

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
CHUNK = int(re.search(r"constexpr\s+uint32_t\s+kChunkTicks\s*=\s*(\d+)\s*;", (ROOT / "asyncflow_amd" / "csrc" / "af_alerts.hpp").read_text()).group(1))
SENTINEL = 0x5A5A5A5A
GUARD = 16                                          # sentinel words on both sides of every output
CELLS = ("fired", "episodes", "longest", "longest_start", "first", "last")
GROUP32 = ("members", "fired_members", "open_members")
GROUP64 = ("fire_ticks", "fire_episodes")
TICKS = ("total", "bad", "firing")
ALL = ("count",) + CELLS + GROUP32 + GROUP64 + ("delay_hist",) + TICKS


@pytest.fixture(scope="module")
def plan():
    p = lower(single_server(horizon=50, period=P))
    assert p.sample_period == P
    return p


@pytest.fixture(scope="module")
def eng(plan):
    from asyncflow_amd.engine import Engine

    e = Engine(plan, 0)
    yield e
    e.close()


class _Batch:
    """Clocks and counts on the device; rows behind a scenario's stored ones hold bad requests that would count if they were read."""

    def __init__(self, clocks, ticks, tick_cap, cap=None):
        import torch

        n = len(clocks)
        self.n, self.tick_cap = n, int(tick_cap)
        self.cap = cap or max(max((len(x) for x in clocks), default=1), 1) + 3
        clock = np.empty((n, self.cap, 2))
        clock[:, :, 0], clock[:, :, 1] = 0.0, 1.0
        counts = np.zeros((n, _abi.CNT_SLOTS), dtype=np.uint32)
        self.stored, self.ticks = [], [min(int(t), self.tick_cap) for t in ticks]
        for i, rows in enumerate(clocks):
            rows = np.asarray(rows, dtype=np.float64).reshape(-1, 2)
            counts[i, _abi.CNT_COMPLETED], counts[i, _abi.CNT_TICKS] = rows.shape[0], ticks[i]
            clock[i, : rows.shape[0]] = rows
            self.stored.append(rows.copy())
        self.dev = torch.device("cuda", 0)
        self.clock_t = torch.as_tensor(clock, device=self.dev)
        self.counts_t = torch.as_tensor(counts.view(np.int32), device=self.dev)
        self._host = {}

    def host(self, rules, edges, slo):
        """The host definition of every scenario, computed once per (rules, edges, slo)."""
        key = (tuple(map(tuple, rules)), tuple(edges), slo)
        if key not in self._host:
            self._host[key] = [scenario_alerts(self.stored[i], self.ticks[i], P, slo, rules, edges) for i in range(self.n)]
        return self._host[key]

    def layout(self, n_groups, n_win, n_rules, bins, want):
        """Word offsets of the wanted outputs in one buffer, GUARD sentinel words before, between and behind them."""
        sc, gc = self.n * n_win * n_rules, n_groups * n_win * n_rules
        sizes = {"count": self.n * n_win, "delay_hist": gc * bins}
        sizes.update({k: sc for k in CELLS}, **{k: gc for k in GROUP32}, **{k: 2 * gc for k in GROUP64}, **{k: self.n * self.tick_cap for k in TICKS})
        off, at = {}, GUARD
        for k in ALL:
            if k in want:
                off[k] = (at, sizes[k])
                at += sizes[k] + (sizes[k] & 1) + GUARD          # (even: the u64 sums stay 8-byte aligned)
        return off, at

    def run(self, eng, group, n_groups, edges, rules, *, slo=SLO, bins=0, width=1, want=ALL, buf=None):
        """One call; returns the outputs (numpy) after checking that no word outside them changed."""
        import torch

        want = tuple(k for k in want if bins or k != "delay_hist")
        n_win, n_rules = len(edges) - 1, len(rules)
        off, total = self.layout(n_groups, n_win, n_rules, bins, want)
        if buf is None:
            buf = torch.full((total,), SENTINEL, dtype=torch.int32, device=self.dev)
        grp_t = None
        if group is not None:
            grp = np.asarray(group, dtype=np.int64)
            grp_t = torch.as_tensor(np.where(grp < 0, _abi.POOL_SKIP, grp).astype(np.uint32).view(np.int32), device=self.dev)
        torch.cuda.synchronize(self.dev)
        eng.summarize_alerts(self.n, n_groups, edges, P, slo, rules, clock_ptr=self.clock_t.data_ptr(), clock_capacity=self.cap,
                             tick_capacity=self.tick_cap, counts_ptr=self.counts_t.data_ptr(),
                             group_ptr=grp_t.data_ptr() if grp_t is not None else 0, delay_bins=bins, delay_width=width,
                             ptrs={k: buf.data_ptr() + 4 * o for k, (o, _) in off.items()})
        words = buf.cpu().numpy().view(np.uint32)
        inside = np.zeros(total, dtype=bool)
        out = {}
        for k, (o, size) in off.items():
            inside[o: o + size] = True
            out[k] = words[o: o + size].copy()
        assert (words[~inside] == SENTINEL).all(), "a word outside the outputs changed"
        for k in out:
            if k in GROUP64:
                out[k] = out[k].view(np.uint64)
            shape = ((self.n, n_win) if k == "count" else (self.n, n_win, n_rules) if k in CELLS else (self.n, self.tick_cap) if k in TICKS
                     else (n_groups, n_win, n_rules, bins) if k == "delay_hist" else (n_groups, n_win, n_rules))
            out[k] = out[k].reshape(shape)
        out["buf"] = buf
        return out

    def check(self, got, group, n_groups, edges, rules, *, slo=SLO, bins=0, width=1):
        """Every word of `got` against the host definition."""
        host = self.host(rules, edges, slo)
        grp = np.zeros(self.n, dtype=np.int64) if group is None else np.asarray(group, dtype=np.int64)
        for s in range(self.n):                             # (skipped scenarios too)
            t_s, h = self.ticks[s], host[s]
            if "count" in got:
                assert np.array_equal(got["count"][s], h["count"].astype(np.uint32)), ("count", s)
            for k in CELLS:
                if k in got:
                    assert np.array_equal(got[k][s], (h[k] & 0xFFFFFFFF).astype(np.uint32)), (k, s, got[k][s], h[k])
            for k in TICKS:
                if k in got:
                    want = firing_words(h["firing"]) if k == "firing" else h[k]
                    assert np.array_equal(got[k][s, :t_s], want), (k, s)
                    assert (got[k][s, t_s:] == SENTINEL).all(), (k, s, "rows at or past t_s were written")
        cells = alert_cells(host, grp, n_groups, bins, width)
        for k in GROUP32 + GROUP64 + ("delay_hist",):
            if k in got:
                assert np.array_equal(got[k].astype(np.uint64), cells[k].astype(np.uint64)), (k, got[k], cells[k])
        return host, cells


def test_row_counts_and_small_tick_counts(eng):
    rng = np.random.default_rng(31)
    m_rows = [0, 1, 63, 64, 65, 3000, 500, 2000, 700]
    ticks = [150, 0, 1, 63, 64, 65, 231, 128, 333]                # (333: more ticks counted than the capacity holds)
    b = _Batch([rows_in_phases(rng, m, min(t, 240), 40) for m, t in zip(m_rows, ticks)], ticks, 240)
    rules = rules_few(100)
    for group, n_groups, edges, kw in ((np.arange(b.n), b.n, [0, 240], {"bins": 5, "width": 1}),
                                       (None, 1, [0, 50, 51, 128, 300, 400], {"bins": 64, "width": 3}),
                                       ([0, 2, 2, -1, 0, 2, -1, 4, 0], 5, [3, 64, 65, 200, 239], {})):
        host, _ = b.check(b.run(eng, group, n_groups, edges, rules, **kw), group, n_groups, edges, rules, **kw)
    assert sum(int(h["fired"].sum()) for h in host) > 100
    one = [(40, 4, 2, 5, 2, 3)]
    b.check(b.run(eng, None, 1, [0, 100, 240], one), None, 1, [0, 100, 240], one)


def test_tick_counts_around_the_chunk_32_rules_and_every_hold(eng):
    rng = np.random.default_rng(32)
    ticks = [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3]
    b = _Batch([rows_in_phases(rng, 5 * t, t, 3000, "sorted") for t in ticks], ticks, 2 * CHUNK + 4)   # (dense: a hold of 200 is met)
    rules = rules_32(CHUNK)                                       # (CHUNK + 5, 3) looks back across a chunk seam, 2^32 - 1 past every t_s
    edges = [0, 100, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 5, 2 * CHUNK + 2, 2 * CHUNK + 3, 2 * CHUNK + 100]
    got = b.run(eng, [0, 1, -1, 1], 2, edges, rules, bins=8, width=500)
    host, cells = b.check(got, [0, 1, -1, 1], 2, edges, rules, bins=8, width=500)
    assert (got["firing"][3, : ticks[3]] >> 31).any()                                      # bit 31
    held = {int(r[5]): sum(int(h["fired"][:, j].sum()) for h in host) for j, r in enumerate(rules)}
    assert all(held[h] > 0 for h in HOLDS) and max(int(h["longest"].max()) for h in host) > 1000
    assert host[3]["fired"][3:6, 5].sum() > 0                                              # the look-back across the seam fires past it
    assert cells["delay_hist"][..., -1].sum() > 0 and cells["delay_hist"][..., :-1].sum() > 0
    b.check(b.run(eng, None, 1, [0, 2 * CHUNK + 4], rules[:1], want=("count", "fired", "members", "total")), None, 1, [0, 2 * CHUNK + 4], rules[:1])


def test_all_rows_bad_none_bad_and_an_infinite_slo(eng):
    rng = np.random.default_rng(33)
    ticks = [200, 130, 64]
    b = _Batch([rows_in_phases(rng, m, 200, 50) for m in (2500, 900, 300)], ticks, 200)
    rules, edges = rules_few(64), [0, 64, 130, 200]
    for slo in (-1.0e9, 1.0e9, float("inf"), 0.0):
        host, _ = b.check(b.run(eng, [0, 0, 1], 2, edges, rules, slo=slo, bins=4, width=2), [0, 0, 1], 2, edges, rules, slo=slo, bins=4, width=2)
        if slo == -1.0e9:
            assert all(int(h["total"].sum()) - int(h["bad"].sum()) <= 1 for h in host) and host[0]["fired"][:, 0].sum() > 0   # (inf - x is not above)
        if slo == 1.0e9:
            assert all(int(h["bad"].sum()) <= 1 for h in host)                             # (a start of -inf is the one latency above it)
        if slo == float("inf"):
            assert all(not h["bad"].any() and not h["firing"].any() for h in host)


def test_windows_one_per_tick_the_whole_run_and_edges_past_the_samples(eng):
    rng = np.random.default_rng(34)
    ticks = [70, 33, 70, 1]
    b = _Batch([rows_in_phases(rng, m, 70, 9) for m in (900, 300, 0, 5)], ticks, 80)
    rules = rules_few(16)[:8] + [(6, 2, 1, 3, 1, 2), (6, 2, 1, 3, 1, 5)]
    per_tick = list(range(0, 75))                                   # one window per tick; the last four past every t_s
    for group, n_groups, edges in ((np.arange(4), 4, per_tick), ([0, 0, 1, 1], 2, per_tick), (None, 1, [0, 70]), (None, 1, [70, 75, 4000]),
                                   ([1, 1, 1, 1], 2, [10, 20, 2 ** 31, 2 ** 32 - 1])):
        got = b.run(eng, group, n_groups, edges, rules, bins=3, width=4)
        b.check(got, group, n_groups, edges, rules, bins=3, width=4)
    assert (got["members"][0] == 0).all() and (got["count"][:, 2] == 0).all() and (got["first"][:, 2] == _abi.TICK_NONE).all()


def test_every_optional_output_absent_in_turn(eng):
    rng = np.random.default_rng(35)
    b = _Batch([rows_in_phases(rng, m, 120, 25) for m in (1500, 800, 50)], [120, 90, 120], 128)
    rules, edges, group = rules_few(64)[:9], [0, 40, 41, 100, 128], [0, 1, 0]
    for drop in [()] + [(k,) for k in ALL] + [CELLS, GROUP32 + GROUP64 + ("delay_hist",), TICKS, tuple(k for k in ALL if k != "first")]:
        want = tuple(k for k in ALL if k not in drop)
        got = b.run(eng, group, 2, edges, rules, bins=6, width=5, want=want)
        assert set(got) - {"buf"} == set(want)
        b.check(got, group, 2, edges, rules, bins=6, width=5)


def test_refusals_leave_every_output_word_alone(eng, plan):
    import torch

    from asyncflow_amd.engine import PLAN_ONLY, Engine

    rng = np.random.default_rng(36)
    b = _Batch([rows_in_phases(rng, 200, 50, 10) for _ in range(3)], [50, 50, 50], 64)
    lib, dev = eng._lib, b.dev  # noqa: SLF001
    n_rules, bins = 2, 4
    cells = 3 * 2 * n_rules                                         # n == G == 3, two windows
    slot = cells * bins                                             # the largest cell output
    buf = torch.full((GUARD + 16 * slot + 3 * b.n * b.tick_cap,), SENTINEL, dtype=torch.int32, device=dev)
    base = buf.data_ptr() + 4 * GUARD
    grp_ok = torch.zeros(3, dtype=torch.int32, device=dev)
    grp_bad = torch.as_tensor(np.array([0, 3, 1], dtype=np.int32), device=dev)
    big = np.arange(65538, dtype=np.uint32)
    good = ((10, 2, 1, 4, 1, 2), (5, 5, 0, 1, 0, 1))

    def call(handle=None, *, n_groups=3, edges=(0, 10, 64), period=P, slo=SLO, rules=good, n_rules=None, group=grp_ok, clock=True,
             counts=True, tick_cap=b.tick_cap, clock_cap=b.cap, bins=bins, width=1, n=3):
        e = np.ascontiguousarray(edges, dtype=np.uint32)
        r = np.ascontiguousarray(rules, dtype=np.uint32).reshape(-1, 6)
        out = _abi.AfOutputs(clock_cap, C.c_void_p(b.clock_t.data_ptr() if clock else None), tick_cap, None,
                             C.c_void_p(b.counts_t.data_ptr() if counts else None))
        p = [C.c_void_p(base + 4 * slot * k) for k in range(13)] + [C.c_void_p(base + 4 * (16 * slot + k * b.n * b.tick_cap)) for k in range(3)]
        req = _abi.AfAlerts(n, n_groups, e.shape[0] - 1, r.shape[0] if n_rules is None else n_rules,
                            C.c_void_p(group.data_ptr() if group is not None else None),
                            e.ctypes.data_as(C.POINTER(C.c_uint32)) if e.shape[0] > 1 else None,
                            r.ctypes.data_as(C.POINTER(_abi.AfAlertRule)) if r.shape[0] else None, period, slo, bins, width, *p, 0.0, 0)
        torch.cuda.synchronize(dev)
        rc = lib.af_engine_summarize_alerts(handle or eng._h, C.byref(out), C.byref(req))  # noqa: SLF001
        assert (buf.cpu().numpy().view(np.uint32) == SENTINEL).all(), "a refused call wrote an output word"
        return rc

    inv, cap_err = _abi.AF_ERR_INVALID, _abi.AF_ERR_CAPACITY
    assert call(n=0) == inv and call(n_groups=0) == inv and call(n_rules=0) == inv and call(rules=()) == inv
    assert call(edges=(0,)) == inv                                   # n_windows == 0, tick_edges NULL
    assert call(rules=[good[0]] * 33) == inv                         # n_rules > 32
    assert call(edges=(0, 10, 10)) == inv and call(edges=(5, 4, 9)) == inv
    for bad in (0.0, -P, float("nan"), float("inf"), -float("inf")):
        assert call(period=bad) == inv, bad
    assert call(slo=float("nan")) == inv
    for bad in ((10, 0, 1, 4, 1, 2), (2, 3, 1, 4, 1, 2), (10, 2, 1, 0, 1, 2), (10, 2, 5, 4, 1, 2), (10, 2, 1, 4, 1, 0)):
        assert call(rules=(good[0], bad)) == inv, bad
    assert call(group=grp_bad) == inv
    assert call(clock=False) == inv and call(counts=False) == inv and call(tick_cap=0) == inv and call(clock_cap=0) == inv
    assert call(bins=0) == inv and call(bins=1025) == inv and call(width=0) == inv
    assert call(n_groups=65537, edges=big) == cap_err                # n_groups * n_windows * n_rules >= 2^32 - 1
    assert call(n=32769, edges=big) == cap_err                       # n_scenarios * n_windows * n_rules >= 2^32 - 1
    assert call(tick_cap=2 ** 31) == cap_err
    plan_only = Engine(plan, PLAN_ONLY)
    try:
        assert call(plan_only._h) == _abi.AF_ERR_NO_DEVICE  # noqa: SLF001
    finally:
        plan_only.close()
    ok = b.run(eng, [0, 1, 2], 3, [0, 10, 64], good, bins=4)
    b.check(ok, [0, 1, 2], 3, [0, 10, 64], good, bins=4)


def test_cells_do_not_depend_on_the_launch_or_the_batch(eng):
    rng = np.random.default_rng(37)
    ticks = [CHUNK + 40, 300, CHUNK + 40, 180, 257]
    mine = [rows_in_phases(rng, m, t, 120) for m, t in zip((5000, 1500, 64, 1025, 10), ticks)]
    others = [rows_in_phases(rng, m, 400, 70, "sorted") for m in (2500, 0, 129, 700)]
    edges, rules = [0, 100, 101, 256, CHUNK - 1, CHUNK + 1, CHUNK + 64], rules_few(CHUNK)
    a = _Batch(mine, ticks, CHUNK + 64, cap=5100)
    group = [0, 1, 0, 2, 1]
    kw = {"bins": 7, "width": 20}
    first = a.run(eng, group, 3, edges, rules, **kw)
    a.check(first, group, 3, edges, rules, **kw)
    again = a.run(eng, group, 3, edges, rules, buf=first["buf"], **kw)       # the same buffers, written a second time
    order = [3, 0, 4, 2, 1]
    mixed = _Batch([others[0], mine[3], others[1], mine[0], mine[4], others[2], mine[2], mine[1], others[3]],
                   [400, ticks[3], 400, ticks[0], ticks[4], 400, ticks[2], ticks[1], 400], CHUNK + 64, cap=5100)
    where = [1, 3, 4, 6, 7]
    group2 = np.array([3, -7, -1, -7, -7, 4, -7, -7, 3])
    group2[where] = [group[o] for o in order]
    other = mixed.run(eng, group2, 5, edges, rules, **kw)
    mixed.check(other, group2, 5, edges, rules, **kw)
    for k in GROUP32 + GROUP64 + ("delay_hist",):
        assert np.array_equal(first[k], again[k]) and np.array_equal(first[k], other[k][:3]), k
    for k in ("count",) + CELLS + TICKS:
        assert np.array_equal(first[k], again[k]) and np.array_equal(first[k][order], other[k][where]), k


def test_event_workload_through_the_python_api_and_in_two_shards(tmp_path):
    from asyncflow_amd import expand_grid
    from asyncflow_amd.runner import SimulationRunner

    payload = lb_with_events(horizon=60, scale=0.1)                  # a spike on the client -> LB edge from t = 10 s, srv-1 down from 18 s
    users = "rqs_input.avg_active_users.mean"
    grid = expand_grid({users: [60.0, 200.0]}, replicas=12, order_by_load=users)
    res = SimulationRunner(simulation_input=payload, **grid.runner_kwargs()).run()
    plan, n = res.plan, len(res)
    p = plan.sample_period
    per = [res[s] for s in range(n)]
    ticks = [min(int(r.counts[_abi.CNT_TICKS]), plan.tick_count) for r in per]
    event = int(round(10.0 / p))                                     # a window edge at the event's tick
    edges = [0, event, int(round(18.0 / p)), plan.tick_count]
    look = int(round(1.0 / p))
    # The slo and the share come from the rows: the slo is the 0.9 quantile of all latencies, and the share of the first rule lies
    # between the replicas' largest rolling bad shares of the event window, so that the host definition fires in some replicas of
    # the window and not in others (asserted below).  The second rule is written in seconds, as a user writes it.
    lat = np.concatenate([r.rqs_clock[:, 1] - r.rqs_clock[:, 0] for r in per])
    slo = float(np.quantile(lat, 0.9))
    peak = []
    for r, t in zip(per, ticks):
        c = completion_ticks(r.rqs_clock, t, p, slo)
        pt, pb = np.cumsum(c["total"].astype(np.int64)), np.cumsum(c["bad"].astype(np.int64))
        shares = [Fraction(int(pb[k] - (pb[k - look] if k >= look else 0)), max(int(pt[k] - (pt[k - look] if k >= look else 0)), 1))
                  for k in range(edges[1], min(edges[2], t))]
        peak.append(max(shares, default=Fraction(0)))
    levels = sorted(set(peak))
    assert len(levels) > 1, "every replica has the same largest rolling bad share in the event window"
    share = levels[(len(levels) - 1) // 2]                           # replicas above it fire, the others do not
    rules = [(look, look, share.numerator, share.denominator, 1, 1), alert_rule(5.0, 1.0, objective=0.9, burn_rate=2, hold_s=2 * p, min_total=5)]
    r6 = check_alert_rules(rules, p)
    host = [scenario_alerts(r.rqs_clock, t, p, slo, r6, edges) for r, t in zip(per, ticks)]

    def check(summ, ids, n_groups, bins=0, width=1):
        for s in range(n):
            for k in ("count",) + CELLS:
                assert np.array_equal(summ[k][s], host[s][k]), (k, s)
        cells = alert_cells(host, ids, n_groups, bins, width)
        for k, v in cells.items():
            assert np.array_equal(summ[k], v), k
        share_of = np.where(cells["members"] > 0, cells["fired_members"] / np.maximum(cells["members"], 1), np.nan)
        assert np.array_equal(summ["fired_share"], share_of, equal_nan=True)
        return cells

    a = res.alert_summary(slo, rules, tick_edges=edges, by=grid, delay_bins=16, delay_width_s=4 * p, per_tick=True)
    cells = check(a, grid.point, 2, 16, 4)
    fired, members = int(cells["fired_members"][:, 1, 0].sum()), int(cells["members"][:, 1, 0].sum())
    assert members == n and 0 < fired < members, (fired, members)    # the event window: the alert fires in some replicas only
    assert a["replicas"].tolist() == [12, 12] and np.array_equal(a["tick_edges"], edges) and np.array_equal(a["times"], np.asarray(edges[:-1]) * p)
    assert a["rules"][1] == {"long_ticks": r6[1, 0], "short_ticks": r6[1, 1], "share": Fraction(1, 5), "min_total": 5, "hold_ticks": 2}
    assert np.array_equal(a["first_s"], np.where(a["first"] >= 0, a["first"] * p, np.nan), equal_nan=True)
    assert np.array_equal(a["longest_s"], a["longest"] * p) and np.array_equal(a["fired_s"], a["fired"] * p)
    for s in range(n):
        t = ticks[s]
        assert np.array_equal(a["total"][s, :t], host[s]["total"]) and np.array_equal(a["bad"][s, :t], host[s]["bad"])
        assert np.array_equal(a["firing"][s, :t], firing_words(host[s]["firing"])) and not a["firing"][s, t:].any()
        one = per[s].get_alerts(slo, rules, tick_edges=edges)
        assert all(np.array_equal(one[k], host[s][k]) for k in ("total", "firing") + CELLS)
    q = alert_delay_quantiles(a, [0.5, 1.0])
    delays = np.sort([host[s]["first"][1, 0] - event for s in range(n) if grid.point[s] == 1 and host[s]["first"][1, 0] >= 0])
    if delays.size:
        mid = delays[max(-(-delays.size // 2), 1) - 1]
        assert q["lo_s"][1, 1, 0, 0] == a["delay_edges_s"][min(mid // 4, 15)] and q["hi_s"][1, 1, 0, 0] == a["delay_edges_s"][min(mid // 4, 15) + 1]
    assert np.isnan(q["lo_s"][cells["fired_members"] == 0]).all()
    skip = np.where(np.arange(n) % 4 == 0, -1, grid.point)
    check(res.alert_summary(slo, rules, tick_edges=edges, by=skip), skip, 2)
    check(res.alert_summary(slo, rules, tick_edges=edges, by="scenario", delay_bins=3), np.arange(n), n, 3, 1)
    with pytest.raises(ValueError, match="multiple"):
        res.alert_summary(slo, [alert_rule(1.0 + p / 3, bad_share=0.5)])
    with pytest.raises(ValueError, match="NaN"):
        res.alert_summary(float("nan"), rules)
    for name in ("alerts.npz", "alerts.parquet"):
        written = res.save_alert_summary(str(tmp_path / name), slo, rules, grid, tick_edges=edges, delay_bins=16, delay_width_s=4 * p)
        back = load_summary(str(tmp_path / name))
        assert set(back) == set(written)
        for k, v in written.items():
            assert np.array_equal(np.asarray(back[k], dtype=v.dtype).reshape(v.shape), v, equal_nan=v.dtype.kind == "f"), (name, k)
        assert np.array_equal(written["alert_fired_members"], cells["fired_members"]) and np.array_equal(written["alert_delay_hist"], cells["delay_hist"])
    # the same sweep in two shards on one device: the group cells add up, the replicas' arrays go behind the sweep's indices
    two = SimulationRunner(simulation_input=payload, **grid.runner_kwargs(), devices=[0, 0]).run()
    assert len(two.shards) == 2
    s2 = two.alert_summary(slo, rules, tick_edges=edges, by=grid, delay_bins=16, delay_width_s=4 * p)
    for k in ("count",) + CELLS + GROUP32 + GROUP64 + ("delay_hist", "fired_share", "first_s"):
        assert np.array_equal(s2[k], a[k], equal_nan=True), k
