"""Alert rules on request outcomes on the MI355X (af_engine_outcome_alerts, asyncflow_amd/csrc/af_alert_outcomes.hpp):
every output word against the host definition (results.scenario_outcome_alerts per scenario, results.alert_cells per group).
Synthetic clocks and arrival rows through the C ABI with `times` given, the dyadic period 2^-5: row and arrival counts on the wave
and pair seams, tick counts on both sides of the kernel's chunk and of twice it, timeouts on chunk seams and on ticks t_s - 1 / t_s,
duplicated arrivals, NaN rows, an all-+inf row, foreign rows (deficit), cut rows (the truncation flag), shared time rows, groups and
AF_POOL_SKIP, 32 rules, every optional output absent in turn, every refusal, the independence of the batch and a scratch pool filled
with 0xFFFFFFFF beforehand.  Every output of a call lies in ONE buffer with sentinel words on both sides of each.  A dropout-and-
outage workload goes through the Python API, unsharded and in two shards."""

from __future__ import annotations

import ctypes as C
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from asyncflow_amd import _abi
from asyncflow_amd.plan import lower
from asyncflow_amd.results import alert_cells, outcome_ticks, scenario_outcome_alerts
from oracle.scenarios import lb_with_events, single_server
from tests.alert_outcomes_util import SLO, TAU, P, arrival_row, rows_from
from tests.alerts_util import firing_words, rules_32, rules_few

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
CHUNK = int(re.search(r"constexpr\s+uint32_t\s+kChunkTicks\s*=\s*(\d+)\s*;", (ROOT / "asyncflow_amd" / "csrc" / "af_alerts.hpp").read_text()).group(1))
assert "kChunkTicks = afal::kChunkTicks" in (ROOT / "asyncflow_amd" / "csrc" / "af_alert_outcomes.hpp").read_text()
SENTINEL = 0x5A5A5A5A
GUARD = 16                                          # sentinel words on both sides of every output
INF = float("inf")
CELLS = ("fired", "episodes", "longest", "longest_start", "first", "last")
GROUP32 = ("members", "fired_members", "open_members")
GROUP64 = ("fire_ticks", "fire_episodes")
TICKS = ("total", "bad", "firing", "timeouts")
WORDS = ("timed_out", "deficit", "flags")
OUTCOME = ("timeouts",) + WORDS
ALL = ("count",) + CELLS + GROUP32 + GROUP64 + ("delay_hist",) + TICKS + WORDS


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
    """Clocks, counts and arrival rows on the device; rows behind a scenario's stored ones hold in-time requests that would count if
    they were read.  `completed`: what counts[s][completed] says (above the stored rows: the clock was cut)."""

    def __init__(self, clocks, ticks, tick_cap, arrivals, time_row=None, cap=None, draw_cap=None, completed=None):
        import torch

        n = len(clocks)
        self.n, self.tick_cap = n, int(tick_cap)
        self.cap = cap or max(max((len(x) for x in clocks), default=1), 1) + 3
        clock = np.empty((n, self.cap, 2))
        clock[:, :, 0], clock[:, :, 1] = 0.0, P
        counts = np.zeros((n, _abi.CNT_SLOTS), dtype=np.uint32)
        self.stored, self.ticks = [], [min(int(t), self.tick_cap) for t in ticks]
        for i, rows in enumerate(clocks):
            rows = np.asarray(rows, dtype=np.float64).reshape(-1, 2)
            counts[i, _abi.CNT_COMPLETED], counts[i, _abi.CNT_TICKS] = rows.shape[0] if completed is None else completed[i], ticks[i]
            clock[i, : min(rows.shape[0], self.cap)] = rows[: self.cap]
            self.stored.append(clock[i, : min(int(counts[i, _abi.CNT_COMPLETED]), self.cap)].copy())
        self.draw_cap = draw_cap or max(max(len(a) for a in arrivals), 1)
        times = np.full((len(arrivals), self.draw_cap), np.inf)
        for j, a in enumerate(arrivals):
            times[j, : len(a)] = a
        self.arrivals = times
        self.time_row = None if time_row is None else np.asarray(time_row, dtype=np.int64)
        self.cut = counts[:, _abi.CNT_COMPLETED] > self.cap
        self.dev = torch.device("cuda", 0)
        self.clock_t = torch.as_tensor(clock, device=self.dev)
        self.counts_t = torch.as_tensor(counts.view(np.int32), device=self.dev)
        self.times_t = torch.as_tensor(times, device=self.dev)
        self.row_t = None if time_row is None else torch.as_tensor(self.time_row.astype(np.int32), device=self.dev)
        self._host = {}

    def row_of(self, s):
        return self.arrivals[s if self.time_row is None else self.time_row[s]]

    def host(self, rules, edges, slo, tau):
        """The host definition of every scenario, computed once per (rules, edges, slo, tau)."""
        key = (tuple(map(tuple, rules)), tuple(edges), slo, tau)
        if key not in self._host:
            self._host[key] = [scenario_outcome_alerts(self.stored[i], self.row_of(i), self.ticks[i], P, slo, tau, rules, edges) for i in range(self.n)]
        return self._host[key]

    def layout(self, n_groups, n_win, n_rules, bins, want):
        """Word offsets of the wanted outputs in one buffer, GUARD sentinel words before, between and behind them."""
        sc, gc = self.n * n_win * n_rules, n_groups * n_win * n_rules
        sizes = {"count": self.n * n_win, "delay_hist": gc * bins}
        sizes.update({k: sc for k in CELLS}, **{k: gc for k in GROUP32}, **{k: 2 * gc for k in GROUP64}, **{k: self.n * self.tick_cap for k in TICKS},
                     **{k: self.n for k in WORDS})
        off, at = {}, GUARD
        for k in ALL:
            if k in want:
                off[k] = (at, sizes[k])
                at += sizes[k] + (sizes[k] & 1) + GUARD          # (even: the u64 sums stay 8-byte aligned)
        return off, at

    def run(self, eng, group, n_groups, edges, rules, *, slo=SLO, tau=TAU, bins=0, width=1, want=ALL, buf=None):
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
        ptrs = {k: buf.data_ptr() + 4 * o for k, (o, _) in off.items()}
        oc = {"times_ptr": self.times_t.data_ptr(), "time_row_ptr": self.row_t.data_ptr() if self.row_t is not None else 0,
              "n_time_rows": self.arrivals.shape[0], "draw_capacity": self.draw_cap, "timeout": tau, **{k: ptrs.pop(k) for k in OUTCOME if k in ptrs}}
        torch.cuda.synchronize(self.dev)
        eng.summarize_alerts(self.n, n_groups, edges, P, slo, rules, clock_ptr=self.clock_t.data_ptr(), clock_capacity=self.cap,
                             tick_capacity=self.tick_cap, counts_ptr=self.counts_t.data_ptr(),
                             group_ptr=grp_t.data_ptr() if grp_t is not None else 0, delay_bins=bins, delay_width=width, ptrs=ptrs, outcomes=oc)
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
                     else (self.n,) if k in WORDS else (n_groups, n_win, n_rules, bins) if k == "delay_hist" else (n_groups, n_win, n_rules))
            out[k] = out[k].reshape(shape)
        out["buf"] = buf
        return out

    def check(self, got, group, n_groups, edges, rules, *, slo=SLO, tau=TAU, bins=0, width=1):
        """Every word of `got` against the host definition."""
        host = self.host(rules, edges, slo, tau)
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
            for k in ("timed_out", "deficit"):
                if k in got:
                    assert int(got[k][s]) == h[k], (k, s, int(got[k][s]), h[k])
            if "flags" in got:
                flags = (_abi.OUTCOME_ROWS_TRUNCATED if self.cut[s] else 0) | (_abi.OUTCOME_DEFICIT if h["deficit"] else 0)
                assert int(got["flags"][s]) == flags, ("flags", s)
        cells = alert_cells(host, grp, n_groups, bins, width)
        for k in GROUP32 + GROUP64 + ("delay_hist",):
            if k in got:
                assert np.array_equal(got[k].astype(np.uint64), cells[k].astype(np.uint64)), (k, got[k], cells[k])
        return host, cells


def _pairs(rng, shapes, t_of, cap=None):
    """(rows, arrival row) per (m, n_arr) of `shapes`; the rows' starts are drawn from the arrival row."""
    arrs = [arrival_row(rng, n_arr, t_of(i)) for i, (_, n_arr) in enumerate(shapes)]
    return [rows_from(rng, a, m) for a, (m, _) in zip(arrs, shapes)], arrs


def test_row_counts_arrival_counts_and_small_tick_counts(eng):
    rng = np.random.default_rng(61)
    shapes = [(0, 0), (1, 1), (40, 64), (40, 65), (5000, 6000), (0, 6000), (1, 64), (0, 1), (64, 65)]
    ticks = [150, 1, 63, 65, 240, 231, 0, 128, 333]               # (333: more ticks counted than the capacity holds)
    clocks, arrs = _pairs(rng, shapes, lambda i: min(ticks[i], 240))
    b = _Batch(clocks, ticks, 240, arrs, draw_cap=6001)            # (an odd capacity: every other row starts off a 16-byte boundary)
    rules = rules_few(100)
    for group, n_groups, edges, kw in ((np.arange(b.n), b.n, [0, 240], {"bins": 5, "width": 1}),
                                       (None, 1, [0, 50, 51, 128, 300, 400], {"bins": 64, "width": 3, "slo": INF}),
                                       ([0, 2, 2, -1, 0, 2, -1, 4, 0], 5, [3, 64, 65, 200, 239], {"tau": P / 4}),
                                       (None, 1, [0, 240], {"tau": 300 * P, "slo": 2.0})):
        host, _ = b.check(b.run(eng, group, n_groups, edges, rules, **kw), group, n_groups, edges, rules, **kw)
        assert all(h["deficit"] == 0 for h in host)
        if kw.get("slo") == INF:
            assert all(np.array_equal(h["bad"], h["timeouts"]) for h in host) and sum(int(h["fired"].sum()) for h in host) > 100
    assert all(h["timed_out"] == 0 for h in host)                  # a timeout beyond the run: nothing times out inside it
    assert sum(h["timed_out"] for h in b.host(rules, [0, 240], SLO, TAU)) > 1000


def test_tick_counts_around_the_chunk_timeouts_on_its_seams_and_32_rules(eng):
    rng = np.random.default_rng(62)
    ticks = [CHUNK - 1, CHUNK + 1, 2 * CHUNK + 3, 63, CHUNK + 1]
    clocks, arrs = _pairs(rng, [(3000, 4000)] * 4, lambda i: ticks[i])
    # timeouts on the last tick of a chunk, the first of the next, t_s - 1 and t_s; rows answer some of them in time, one too late
    seam = np.sort(np.asarray([k * P - TAU + d for k in (0, CHUNK - 1, CHUNK, CHUNK, CHUNK + 1) for d in (0.0, P / 2)]))
    arrs.append(seam)
    clocks.append(np.array([[seam[2], seam[2] + P / 4], [seam[5], seam[5] + TAU], [seam[6], seam[6] + TAU + P / 8], [seam[9], seam[9] + SLO + P]]))
    b = _Batch(clocks, ticks, 2 * CHUNK + 4, arrs)
    rules = rules_32(CHUNK)
    edges = [0, 100, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 5, 2 * CHUNK + 2, 2 * CHUNK + 3, 2 * CHUNK + 100]
    got = b.run(eng, [0, 1, -1, 1, 0], 2, edges, rules, bins=8, width=500)
    host, _ = b.check(got, [0, 1, -1, 1, 0], 2, edges, rules, bins=8, width=500)
    assert host[4]["timeouts"][[0, CHUNK - 1, CHUNK]].tolist() == [2, 1, 3] and host[4]["timed_out"] == 6     # tick CHUNK + 1 == t_s: past the run
    assert all(h["deficit"] == 0 and h["timed_out"] > 0 for h in host) and sum(int(h["fired"].sum()) for h in host) > 0
    b.check(b.run(eng, None, 1, [0, 2 * CHUNK + 4], rules[:1], want=("count", "fired", "members", "total", "timed_out")), None, 1, [0, 2 * CHUNK + 4], rules[:1])


def test_nan_rows_an_all_inf_row_foreign_rows_and_cut_rows(eng):
    rng = np.random.default_rng(63)
    arr = arrival_row(rng, 500, 100)
    own = rows_from(rng, arr, 400)
    nan_rows = np.array([[np.nan, 1.0], [1.0, np.nan], [arr[5], np.nan], [np.inf, 1.0], [-np.inf, -np.inf], [arr[7], arr[7] + P]])
    foreign = np.stack([np.arange(200) * (P / 8) + P / 16, np.arange(200) * (P / 8) + P / 16 + SLO / 2], axis=1)   # eight a tick
    clocks = [own, nan_rows, own, foreign, own[:0], own]
    b = _Batch(clocks, [100] * 6, 100, [arr, np.zeros(0), arr], time_row=[0, 0, 1, 2, 1, 2], cap=300, completed=[400, 6, 400, 200, 0, 301])
    assert b.cut.tolist() == [True, False, True, False, False, True]
    rules, edges, group = rules_few(64), [0, 50, 100], [0, 0, 1, 1, -1, 1]
    got = b.run(eng, group, 2, edges, rules, bins=4, width=2)
    host, _ = b.check(got, group, 2, edges, rules, bins=4, width=2)
    assert host[2]["deficit"] > 0 and host[2]["timed_out"] == 0 and host[3]["deficit"] > 0 and host[4]["total"].sum() == 0
    assert host[1]["deficit"] == 0 and host[1]["timed_out"] > host[0]["timed_out"] > 0
    assert got["flags"].tolist() == [1, 0, 3, 2, 0, 1]


def test_batches_of_1_3_and_70_scenarios_with_shared_time_rows_groups_and_skips(eng):
    rng = np.random.default_rng(64)
    arrs = [arrival_row(rng, n, 90) for n in (700, 65, 1200)]
    rules = rules_few(64)[:9]
    for n in (1, 3, 70):
        row = [(3 * s + s // 7) % 3 for s in range(n)]
        clocks = [rows_from(rng, arrs[r], int(rng.integers(0, np.isfinite(arrs[r]).sum()))) for r in row]
        ticks = [int(t) for t in rng.integers(60, 100, n)]
        b = _Batch(clocks, ticks, 96, arrs, time_row=row)
        group = [(-1 if s % 11 == 3 else s % 4) for s in range(n)]
        got = b.run(eng, group, 4, [0, 30, 31, 96], rules, bins=6, width=5, slo=INF)
        host, cells = b.check(got, group, 4, [0, 30, 31, 96], rules, bins=6, width=5, slo=INF)
        assert all(h["deficit"] == 0 for h in host)
    assert cells["fired_members"].sum() > 0 and cells["members"][:, 0, 0].sum() == 70 - 7


def test_every_optional_output_absent_in_turn(eng):
    rng = np.random.default_rng(65)
    clocks, arrs = _pairs(rng, [(1500, 2000), (800, 900), (50, 400)], lambda i: 120)
    b = _Batch(clocks, [120, 90, 120], 128, arrs)
    rules, edges, group = rules_few(64)[:9], [0, 40, 41, 100, 128], [0, 1, 0]
    for drop in [()] + [(k,) for k in ALL] + [CELLS, GROUP32 + GROUP64 + ("delay_hist",), TICKS, OUTCOME, tuple(k for k in ALL if k != "deficit")]:
        want = tuple(k for k in ALL if k not in drop)
        got = b.run(eng, group, 2, edges, rules, bins=6, width=5, want=want)
        assert set(got) - {"buf"} == set(want)
        b.check(got, group, 2, edges, rules, bins=6, width=5)


def test_refusals_leave_every_output_word_alone(eng, plan):
    import torch

    from asyncflow_amd.engine import PLAN_ONLY, Engine

    rng = np.random.default_rng(66)
    clocks, arrs = _pairs(rng, [(200, 300)] * 3, lambda i: 50)
    b = _Batch(clocks, [50, 50, 50], 64, arrs, time_row=[0, 1, 2])
    lib, dev = eng._lib, b.dev  # noqa: SLF001
    n_rules, bins = 2, 4
    cells = 3 * 2 * n_rules                                         # n == G == 3, two windows
    slot = cells * bins                                             # the largest cell output
    per_tick = b.n * b.tick_cap
    buf = torch.full((GUARD + 16 * slot + 4 * per_tick + 3 * 4,), SENTINEL, dtype=torch.int32, device=dev)
    base = buf.data_ptr() + 4 * GUARD
    grp_ok = torch.zeros(3, dtype=torch.int32, device=dev)
    row_bad = torch.as_tensor(np.array([0, 3, 1], dtype=np.int32), device=dev)
    grp_bad = torch.as_tensor(np.array([0, 3, 1], dtype=np.int32), device=dev)
    good = ((10, 2, 1, 4, 1, 2), (5, 5, 0, 1, 0, 1))

    def call(handle=None, *, n_groups=3, edges=(0, 10, 64), period=P, slo=SLO, rules=good, group=grp_ok, tick_cap=b.tick_cap, clock_cap=b.cap,
             n=3, times=True, time_row=b.row_t, n_time_rows=3, draw_cap=b.draw_cap, tau=TAU, oc=True, al=True):
        e = np.ascontiguousarray(edges, dtype=np.uint32)
        r = np.ascontiguousarray(rules, dtype=np.uint32).reshape(-1, 6)
        out = _abi.AfOutputs(clock_cap, C.c_void_p(b.clock_t.data_ptr()), tick_cap, None, C.c_void_p(b.counts_t.data_ptr()))
        p = [C.c_void_p(base + 4 * slot * k) for k in range(13)] + [C.c_void_p(base + 4 * (16 * slot + k * per_tick)) for k in range(3)]
        req = _abi.AfAlerts(n, n_groups, e.shape[0] - 1, r.shape[0], C.c_void_p(group.data_ptr() if group is not None else None),
                            e.ctypes.data_as(C.POINTER(C.c_uint32)), r.ctypes.data_as(C.POINTER(_abi.AfAlertRule)), period, slo, bins, 1, *p, 0.0, 0)
        tail = base + 4 * (16 * slot + 3 * per_tick)
        ocs = _abi.AfAlertOutcomes(C.c_void_p(b.times_t.data_ptr() if times else None), C.c_void_p(time_row.data_ptr() if time_row is not None else None),
                                   n_time_rows, draw_cap, tau, C.c_void_p(tail), *(C.c_void_p(tail + 4 * (per_tick + 4 * k)) for k in range(3)))
        torch.cuda.synchronize(dev)
        rc = lib.af_engine_outcome_alerts(handle or eng._h, C.byref(out), C.byref(ocs) if oc else None, C.byref(req) if al else None)  # noqa: SLF001
        assert (buf.cpu().numpy().view(np.uint32) == SENTINEL).all(), "a refused call wrote an output word"
        return rc

    inv, cap_err = _abi.AF_ERR_INVALID, _abi.AF_ERR_CAPACITY
    assert call(oc=False) == inv and call(al=False) == inv
    assert call(times=False) == inv and call(draw_cap=0) == inv and call(n_time_rows=0) == inv
    assert call(time_row=row_bad) == inv                             # a row id >= n_time_rows, read back on the host
    assert call(time_row=None, n_time_rows=2) == inv and call(n_time_rows=2) == inv
    for bad in (0.0, -TAU, float("nan"), INF, -INF):
        assert call(tau=bad) == inv, bad
    assert call(draw_cap=2 ** 31) == cap_err and call(clock_cap=2 ** 31) == cap_err
    # what af_engine_summarize_alerts refuses
    assert call(n=0) == inv and call(n_groups=0) == inv and call(rules=()) == inv and call(edges=(0, 10, 10)) == inv
    assert call(period=0.0) == inv and call(slo=float("nan")) == inv and call(rules=(good[0], (2, 3, 1, 4, 1, 2))) == inv
    assert call(group=grp_bad) == inv and call(tick_cap=0) == inv and call(clock_cap=0) == inv and call(tick_cap=2 ** 31) == cap_err
    plan_only = Engine(plan, PLAN_ONLY)
    try:
        assert call(plan_only._h) == _abi.AF_ERR_NO_DEVICE  # noqa: SLF001
    finally:
        plan_only.close()
    ok = b.run(eng, [0, 1, 2], 3, [0, 10, 64], good, bins=4)
    b.check(ok, [0, 1, 2], 3, [0, 10, 64], good, bins=4)
    plain = _Batch(clocks, [50, 50, 50], 64, arrs)                   # time_row NULL: scenario s reads row s
    b.check(plain.run(eng, [0, 1, 2], 3, [0, 10, 64], good, bins=4), [0, 1, 2], 3, [0, 10, 64], good, bins=4)


def test_cells_do_not_depend_on_the_batch_and_a_scratch_pool_full_of_ones(eng, plan):
    from asyncflow_amd.engine import Engine

    rng = np.random.default_rng(67)
    ticks = [CHUNK + 40, 300, 180, 257]
    mine, arrs = _pairs(rng, [(4000, 5000), (1500, 1600), (64, 1025), (10, 30)], lambda i: ticks[i])
    others, other_arrs = _pairs(rng, [(2500, 2600), (0, 100), (129, 700)], lambda i: 400)
    edges, rules = [0, 100, 101, 256, CHUNK - 1, CHUNK + 1, CHUNK + 64], rules_few(CHUNK)
    a = _Batch(mine, ticks, CHUNK + 64, arrs, cap=4100, draw_cap=5001)
    group = [0, 1, 0, 2]
    kw = {"bins": 7, "width": 20}
    first = a.run(eng, group, 3, edges, rules, **kw)
    a.check(first, group, 3, edges, rules, **kw)
    again = a.run(eng, group, 3, edges, rules, buf=first["buf"], **kw)       # the same buffers, written a second time
    order = [3, 0, 2, 1]
    where = [1, 3, 4, 6]
    clocks = [others[0], mine[3], others[1], mine[0], mine[2], others[2], mine[1]]
    rows_of = [other_arrs[0], arrs[3], other_arrs[1], arrs[0], arrs[2], other_arrs[2], arrs[1]]
    mixed = _Batch(clocks, [400, ticks[3], 400, ticks[0], ticks[2], 400, ticks[1]], CHUNK + 64, rows_of[::-1], time_row=[6, 5, 4, 3, 2, 1, 0],
                   cap=4100, draw_cap=5002)
    group2 = np.array([3, -7, -1, -7, -7, 4, -7])
    group2[where] = [group[o] for o in order]
    other = mixed.run(eng, group2, 5, edges, rules, **kw)
    mixed.check(other, group2, 5, edges, rules, **kw)
    # a fresh engine whose pool, twice what the call needs, holds 0xFFFFFFFF in every word
    dirty = Engine(plan, 0)
    try:
        need = a.n * a.tick_cap * 8 + 4096
        assert dirty._lib.af_probe_scratch(dirty._h, 2 * need, 0xFFFFFFFF) == 0  # noqa: SLF001
        third = a.run(dirty, group, 3, edges, rules, **kw)
    finally:
        dirty.close()
    for k in GROUP32 + GROUP64 + ("delay_hist",):
        assert np.array_equal(first[k], again[k]) and np.array_equal(first[k], third[k]) and np.array_equal(first[k], other[k][:3]), k
    for k in ("count",) + CELLS + TICKS + WORDS:
        assert np.array_equal(first[k], again[k]) and np.array_equal(first[k], third[k]) and np.array_equal(first[k][order], other[k][where]), k


def test_dropout_and_outage_workload_through_the_python_api_and_in_two_shards():
    from asyncflow_amd import expand_grid
    from asyncflow_amd.runner import SimulationRunner

    payload = lb_with_events(horizon=60, scale=0.1)                  # a spike on the client -> LB edge from t = 10 s, srv-1 down from 18 s
    for e in payload["topology_graph"]["edges"]:
        if e["id"] in ("client-lb", "srv2-client"):
            e["dropout_rate"] = 0.04                                 # a lossy edge on the way in and one on the way back
    users = "rqs_input.avg_active_users.mean"
    grid = expand_grid({users: [60.0, 200.0]}, replicas=6, order_by_load=users)
    res = SimulationRunner(simulation_input=payload, **grid.runner_kwargs()).run()
    plan, n = res.plan, len(res)
    p, tau = plan.sample_period, 0.75
    per = [res[s] for s in range(n)]
    ticks = [min(int(r.counts[_abi.CNT_TICKS]), plan.tick_count) for r in per]
    times = [res.arrival_times(s) for s in range(n)]
    edges = [0, int(round(10.0 / p)), int(round(18.0 / p)), plan.tick_count]
    look = int(round(2.0 / p))
    # The share of the availability rule comes from the rows: it lies between the replicas' largest rolling bad shares over the run, so
    # that the host definition fires in some replicas and not in others (asserted below).
    peak = []
    for r, t, a in zip(per, ticks, times):
        o = outcome_ticks(r.rqs_clock, a, t, p, INF, tau)
        assert o["deficit"] == 0 and o["timed_out"] > 0 and int(r.counts[_abi.CNT_DROPPED]) > 0
        pt, pb = np.cumsum(o["total"].astype(np.int64)), np.cumsum(o["bad"].astype(np.int64))
        shares = [Fraction(int(pb[k] - (pb[k - look] if k >= look else 0)), int(pt[k] - (pt[k - look] if k >= look else 0)))
                  for k in range(t) if pt[k] - (pt[k - look] if k >= look else 0) >= 5]
        peak.append(max(shares, default=Fraction(0)))
    levels = sorted(set(peak))
    assert len(levels) > 1, "every replica has the same largest rolling bad share"
    share = levels[(len(levels) - 1) // 2]
    rules = [(look, look, share.numerator, share.denominator, 5, 1), (2 * look, look // 2, 1, 50, 5, 2)]
    host = [scenario_outcome_alerts(r.rqs_clock, a, t, p, INF, tau, rules, edges) for r, t, a in zip(per, ticks, times)]

    def check(summ, ids, n_groups, bins=0, width=1):
        for s in range(n):
            for k in ("count",) + CELLS:
                assert np.array_equal(summ[k][s], host[s][k]), (k, s)
            assert int(summ["timed_out"][s]) == host[s]["timed_out"] and int(summ["deficit"][s]) == 0 and int(summ["flags"][s]) == 0
        cells = alert_cells(host, ids, n_groups, bins, width)
        for k, v in cells.items():
            assert np.array_equal(summ[k], v), k
        return cells

    a = res.alert_summary(INF, rules, tick_edges=edges, by=grid, delay_bins=16, delay_width_s=4 * p, per_tick=True, timeout_s=tau)
    cells = check(a, grid.point, 2, 16, 4)
    fired = [bool((h["first"][:, 0] >= 0).any()) for h in host]
    assert any(fired) and not all(fired), fired                      # the availability rule fires in some replicas, not in all
    assert a["timeout_s"] == tau and a["slo_s"] == INF and int(cells["fired_members"][..., 0].sum()) > 0
    for s in range(n):
        t = ticks[s]
        for k in ("total", "bad", "timeouts"):
            assert np.array_equal(a[k][s, :t], host[s][k]) and not a[k][s, t:].any(), (k, s)
        assert np.array_equal(a["firing"][s, :t], firing_words(host[s]["firing"])) and np.array_equal(a["bad"][s], a["timeouts"][s])
        one = per[s].get_alerts(INF, rules, tick_edges=edges, timeout_s=tau)
        assert all(np.array_equal(one[k], host[s][k]) for k in ("total", "timeouts", "firing") + CELLS)
    # the completions-only call cannot express it: with slo = +inf nothing is bad and no rule ever fires
    plain = res.alert_summary(INF, rules, tick_edges=edges, by=grid)
    assert not plain["fired"].any() and a["fired"][:, :, 0].any() and "timed_out" not in plain
    with pytest.raises(ValueError, match="timeout"):
        res.alert_summary(INF, rules, timeout_s=0.0)
    # the same sweep in two shards on one device: every shard regenerates its own arrival rows
    two = SimulationRunner(simulation_input=payload, **grid.runner_kwargs(), devices=[0, 0]).run()
    assert len(two.shards) == 2
    s2 = two.alert_summary(INF, rules, tick_edges=edges, by=grid, delay_bins=16, delay_width_s=4 * p, timeout_s=tau)
    for k in ("count",) + CELLS + GROUP32 + GROUP64 + ("delay_hist", "fired_share", "first_s", "timed_out", "deficit"):
        assert np.array_equal(s2[k], a[k], equal_nan=True), k
