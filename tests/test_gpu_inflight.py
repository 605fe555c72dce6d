"""Requests in flight on the MI355X (af_engine_summarize_inflight, asyncflow_amd/csrc/af_inflight.hpp): every output word
against the host definition (results.in_flight_series per scenario, results.in_flight_window_stats per group).  Synthetic clocks
through the C ABI, on a single-server plan with the dyadic period 2^-5: the wave and unroll seams of the row walk, start orders,
starts from before the first sample to past the last, latencies from 0 to past the end with NaN / negative / reversed rows, tick
counts on both sides of the kernel's chunk and of twice it with requests across the seams, window and group arrangements,
thresholds and histograms, every optional output present and absent, every refusal, and the independence of the launch.  Every
output of a call lies in ONE buffer with sentinel words on both sides of each.  An event workload goes through the Python API."""

from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from asyncflow_amd import _abi
from asyncflow_amd.plan import lower
from asyncflow_amd.results import in_flight_series, in_flight_window_stats, load_summary, series_histogram_quantiles
from oracle.scenarios import lb_with_events, single_server

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
CHUNK = int(re.search(r"constexpr\s+uint32_t\s+kChunkTicks\s*=\s*(\d+)\s*;",
                      (ROOT / "asyncflow_amd" / "csrc" / "af_inflight.hpp").read_text()).group(1))
P = 2.0 ** -5
ROWS = [0, 1, 63, 64, 65, 255, 256, 257, 1025]      # the wave and unroll seams of the row walk
ORDERS = ("sorted", "reversed", "random", "one")
SENTINEL = 0x5A5A5A5A
GUARD = 16                                          # sentinel words on both sides of every output
CELL_KEYS = ("count", "sum", "min", "max", "above", "hist", "under")
TICK_KEYS = ("in_flight", "started", "finished")


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


def _clock(rng, m, t_s, order):
    """m rows: starts multiples of P / 4 from before the first sample to past the last one; latencies 0, below one tick, exactly
    one tick, many ticks, past t_s; NaN and negative starts and one finish < start row mixed in."""
    tick4 = rng.integers(-6, 4 * (t_s + 4), m)
    if order == "one":
        tick4 = np.full(m, 4 * max(t_s // 2, 1) + 1)
    start = tick4 * (P / 4.0)
    if order in ("sorted", "reversed"):
        start = np.sort(start) if order == "sorted" else np.sort(start)[::-1]
    pool = np.array([0.0, P / 4, P / 2, P, P, 2 * P, 5 * P, 37 * P, 300 * P, (t_s + 9) * P, 2.0 ** 40])
    rows = np.stack([start, start + pool[rng.integers(0, pool.size, m)]], axis=1)
    if m > 8:
        at = rng.choice(m, 4, replace=False)
        rows[at[0]] = [np.nan, 1.0]
        rows[at[1]] = [2 * P, np.nan]
        rows[at[2]] = [-3 * P, 9 * P]
        rows[at[3]] = [7 * P, 3 * P]             # finish < start
    return rows


class _Batch:
    """Clocks and counts on the device; rows behind a scenario's stored ones hold requests that would count if they were read."""

    def __init__(self, clocks, ticks, tick_cap, cap=None, counts_extra=0):
        import torch

        n = len(clocks)
        self.n, self.tick_cap = n, int(tick_cap)
        self.cap = cap or max(max((len(x) for x in clocks), default=1), 1) + 3
        clock = np.empty((n, self.cap, 2))
        clock[:, :, 0], clock[:, :, 1] = 0.0, 1.0e9
        counts = np.zeros((n, _abi.CNT_SLOTS), dtype=np.uint32)
        self.stored, self.ticks = [], [min(int(t), self.tick_cap) for t in ticks]
        for i, rows in enumerate(clocks):
            rows = np.asarray(rows, dtype=np.float64).reshape(-1, 2)
            counts[i, _abi.CNT_COMPLETED] = rows.shape[0] + counts_extra
            counts[i, _abi.CNT_TICKS] = ticks[i]
            keep = rows[: self.cap]
            clock[i, : keep.shape[0]] = keep
            self.stored.append(clock[i, : min(rows.shape[0] + counts_extra, self.cap)].copy())
        self.dev = torch.device("cuda", 0)
        self.clock_t = torch.as_tensor(clock, device=self.dev)
        self.counts_t = torch.as_tensor(counts.view(np.int32), device=self.dev)
        self.series = [in_flight_series(self.stored[i], self.ticks[i], P) for i in range(n)]

    def layout(self, n_groups, n_win, bins, want):
        """Word offsets of the wanted outputs in one buffer, GUARD sentinel words before, between and behind them."""
        cells = n_groups * n_win
        sizes = {"count": cells, "sum": 2 * cells, "min": cells, "max": cells, "above": cells, "hist": cells * bins, "under": cells,
                 "in_flight": self.n * self.tick_cap, "started": self.n * self.tick_cap, "finished": self.n * self.tick_cap}
        off, at = {}, GUARD
        for k in CELL_KEYS + TICK_KEYS:
            if k in want:
                off[k] = (at, sizes[k])
                at += sizes[k] + (sizes[k] & 1) + GUARD          # (even: the u64 sums stay 8-byte aligned)
        return off, at

    def run(self, eng, group, n_groups, edges, *, threshold=0, bins=0, lo=0, want=CELL_KEYS + TICK_KEYS, buf=None):
        """One call; returns the outputs (numpy) after checking that no word outside them changed."""
        import torch

        want = tuple(k for k in want if bins or k not in ("hist", "under"))
        n_win = len(edges) - 1
        off, total = self.layout(n_groups, n_win, bins, want)
        if buf is None:
            buf = torch.full((total,), SENTINEL, dtype=torch.int32, device=self.dev)
        grp_t = None
        if group is not None:
            grp = np.asarray(group, dtype=np.int64)
            grp_t = torch.as_tensor(np.where(grp < 0, _abi.POOL_SKIP, grp).astype(np.uint32).view(np.int32), device=self.dev)
        ptr = {k: buf.data_ptr() + 4 * o for k, (o, _) in off.items()}
        torch.cuda.synchronize(self.dev)
        eng.summarize_inflight(self.n, n_groups, edges, P, clock_ptr=self.clock_t.data_ptr(), clock_capacity=self.cap,
                               tick_capacity=self.tick_cap, counts_ptr=self.counts_t.data_ptr(), count_ptr=ptr["count"], sum_ptr=ptr["sum"],
                               min_ptr=ptr.get("min", 0), max_ptr=ptr.get("max", 0), above_ptr=ptr.get("above", 0),
                               hist_ptr=ptr.get("hist", 0), under_ptr=ptr.get("under", 0), in_flight_ptr=ptr.get("in_flight", 0),
                               started_ptr=ptr.get("started", 0), finished_ptr=ptr.get("finished", 0),
                               group_ptr=grp_t.data_ptr() if grp_t is not None else 0, threshold=threshold, bins=bins, lo=lo)
        words = buf.cpu().numpy().view(np.uint32)
        inside = np.zeros(total, dtype=bool)
        out = {}
        for k, (o, size) in off.items():
            inside[o: o + size] = True
            out[k] = words[o: o + size].copy()
        assert (words[~inside] == SENTINEL).all(), "a word outside the outputs changed"
        out["sum"] = out["sum"].view(np.uint64)
        shape = (n_groups, n_win)
        for k in CELL_KEYS:
            if k in out:
                out[k] = out[k].reshape(shape + ((bins,) if k == "hist" else ()))
        for k in TICK_KEYS:
            if k in out:
                out[k] = out[k].reshape(self.n, self.tick_cap)
        out["buf"] = buf
        return out

    def check(self, got, group, n_groups, edges, *, threshold=0, bins=0, lo=0):
        """Every word of `got` against the host definition."""
        grp = np.zeros(self.n, dtype=np.int64) if group is None else np.asarray(group, dtype=np.int64)
        for g in range(n_groups):
            members = [self.series[s]["in_flight"] for s in range(self.n) if grp[s] == g]
            want = in_flight_window_stats(members, edges, threshold, bins, lo)
            for k in CELL_KEYS:
                if k in got:
                    assert np.array_equal(got[k][g].astype(np.uint64), np.asarray(want[k]).astype(np.uint64)), (k, g, got[k][g], want[k])
        for k in TICK_KEYS:
            if k in got:
                for s in range(self.n):                     # (skipped scenarios too)
                    t_s = self.ticks[s]
                    assert np.array_equal(got[k][s, :t_s], self.series[s][k]), (k, s)
                    assert (got[k][s, t_s:] == SENTINEL).all(), (k, s, "rows at or past t_s were written")


@pytest.mark.parametrize("order", ORDERS)
def test_row_counts_and_start_orders(eng, order):
    rng = np.random.default_rng(ORDERS.index(order))
    ticks = [150, 0, 97, 200, 64, 231, 128, 200, 333]             # (333: more ticks counted than the capacity holds)
    b = _Batch([_clock(rng, m, min(t, 240), order) for m, t in zip(ROWS, ticks)], ticks, 240)
    assert max(int(s["in_flight"].max()) for s in b.series if s["in_flight"].size) > 3
    for group, G, edges, kw in ((np.arange(b.n), b.n, [0, 240], {"threshold": 1, "bins": 5, "lo": 1}),
                                (None, 1, [0, 50, 51, 128, 300, 400], {"threshold": 0, "bins": 64}),
                                ([0, 2, 2, -1, 0, 2, -1, 4, 0], 5, [3, 64, 65, 200, 239], {"threshold": 7})):
        b.check(b.run(eng, group, G, edges, **kw), group, G, edges, **kw)


def test_tick_counts_around_the_chunk_and_twice_it(eng):
    rng = np.random.default_rng(12)
    ticks = [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1, 2 * CHUNK + 7]
    clocks = []
    for t in ticks:
        seam = [[(CHUNK - 1) * P, (CHUNK + 1) * P], [(CHUNK - 0.5) * P, (CHUNK + 0.25) * P], [CHUNK * P, (CHUNK + 1) * P],
                [(CHUNK - 3) * P, CHUNK * P], [5 * P, (2 * CHUNK + 1) * P], [(2 * CHUNK - 1) * P, (2 * CHUNK) * P],
                [(2 * CHUNK - 2) * P, (2 * CHUNK + 2) * P], [(CHUNK - 1) * P, (2 * CHUNK + 1) * P], [0.0, 1.0e9]]
        clocks.append(np.concatenate([_clock(rng, 600, t, "random"), np.array(seam)]))
    b = _Batch(clocks, ticks, 2 * CHUNK + 4)
    last = b.series[-1]["in_flight"]
    assert last[CHUNK - 1] >= 3 and last[CHUNK] >= 3 and last[2 * CHUNK] >= 3          # requests are open across both seams
    edges = [0, 100, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 5, 2 * CHUNK + 2, 2 * CHUNK + 3, 2 * CHUNK + 100]
    for group, G in (([0, 1, -1, 1, 3, 0, 3], 4), (None, 1), (np.arange(b.n), b.n)):
        kw = {"threshold": 4, "bins": 8, "lo": 2}
        b.check(b.run(eng, group, G, edges, **kw), group, G, edges, **kw)
    b.check(b.run(eng, None, 1, [0, 2 * CHUNK + 4], want=("count", "sum", "max", "in_flight")), None, 1, [0, 2 * CHUNK + 4])


def test_windows_one_per_tick_and_edges_past_the_samples(eng):
    rng = np.random.default_rng(13)
    ticks = [70, 33, 70, 1]
    b = _Batch([_clock(rng, m, 70, "random") for m in (300, 90, 0, 5)], ticks, 80)
    per_tick = list(range(0, 75))                                   # one window per tick; the last four past every t_s
    for group, G, edges in ((np.arange(4), 4, per_tick), ([0, 0, 1, 1], 2, per_tick), (None, 1, [0, 70]), (None, 1, [70, 75, 4000]),
                            ([1, 1, 1, 1], 2, [10, 20, 2 ** 31, 2 ** 32 - 1])):
        got = b.run(eng, group, G, edges, threshold=2, bins=3, lo=0)
        b.check(got, group, G, edges, threshold=2, bins=3, lo=0)
    assert (got["count"][0] == 0).all() and (got["min"][0] == 0).all() and got["count"][1, 2] == 0   # a group without members; empty cells


def test_thresholds_histograms_and_every_optional_output(eng):
    rng = np.random.default_rng(14)
    ticks = [120, 90, 120]
    b = _Batch([_clock(rng, m, 120, "sorted") for m in (700, 400, 50)], ticks, 128)
    top = max(int(s["in_flight"].max()) for s in b.series)
    assert top >= 6
    edges, group = [0, 40, 41, 100, 128], [0, 1, 0]
    for thr in (0, 1, top - 1, top, top + 1, 2 ** 32 - 1):
        b.check(b.run(eng, group, 2, edges, threshold=thr), group, 2, edges, threshold=thr)
    for bins, lo in ((1, 0), (1, 3), (4, 2), (top + 1, 0), (top, 1), (1024, 0), (3, top + 5)):   # lo > 0; the last bin overflowing
        got = b.run(eng, group, 2, edges, bins=bins, lo=lo)
        b.check(got, group, 2, edges, bins=bins, lo=lo)
        assert np.array_equal(got["under"].astype(np.int64) + got["hist"].sum(axis=2), got["count"])
    full = CELL_KEYS + TICK_KEYS
    for drop in [()] + [(k,) for k in full if k not in ("count", "sum", "hist")] + [("min", "max", "above", "hist", "under") + TICK_KEYS,
                                                                           ("started", "finished"), ("in_flight",), ("hist", "under")]:
        want = tuple(k for k in full if k not in drop)
        got = b.run(eng, group, 2, edges, threshold=2, bins=6, lo=1, want=want)
        assert set(got) - {"buf"} == set(want)
        b.check(got, group, 2, edges, threshold=2, bins=6, lo=1)


def test_refusals_leave_every_output_word_alone(eng, plan):
    import torch

    from asyncflow_amd.engine import PLAN_ONLY, Engine

    rng = np.random.default_rng(15)
    b = _Batch([_clock(rng, 40, 50, "random") for _ in range(3)], [50, 50, 50], 64)
    lib, dev = eng._lib, b.dev  # noqa: SLF001
    cells = 3 * 2
    buf = torch.full((GUARD + 13 * cells + 3 * b.n * b.tick_cap,), SENTINEL, dtype=torch.int32, device=dev)
    base = buf.data_ptr() + 4 * GUARD
    grp_ok = torch.zeros(3, dtype=torch.int32, device=dev)
    grp_bad = torch.as_tensor(np.array([0, 3, 1], dtype=np.int32), device=dev)
    big = np.arange(65538, dtype=np.uint32)

    def call(handle=None, *, n_groups=3, edges=(0, 10, 64), period=P, group=grp_ok, clock=True, counts=True, tick_cap=b.tick_cap,
             count=True, hist=True, bins=4, n=3, counts_t=None):
        e = np.ascontiguousarray(edges, dtype=np.uint32)
        out = _abi.AfOutputs(b.cap, C.c_void_p(b.clock_t.data_ptr() if clock else None), tick_cap, None,
                             C.c_void_p((counts_t if counts_t is not None else b.counts_t).data_ptr() if counts else None))
        p = [C.c_void_p(base + 4 * cells * k) for k in (0, 2, 4, 5, 6, 7, 11)] + [C.c_void_p(base + 4 * (12 * cells + k * b.n * b.tick_cap)) for k in range(3)]
        if not count:
            p[0] = C.c_void_p(None)
        if not hist:
            p[5] = C.c_void_p(None)                                   # (under without hist)
        req = _abi.AfInflight(n, n_groups, e.shape[0] - 1, C.c_void_p(group.data_ptr() if group is not None else None),
                              e.ctypes.data_as(C.POINTER(C.c_uint32)) if e.shape[0] else None, period, 1, bins, 0, *p, 0.0, 0)
        torch.cuda.synchronize(dev)
        rc = lib.af_engine_summarize_inflight(handle or eng._h, C.byref(out), C.byref(req))  # noqa: SLF001
        assert (buf.cpu().numpy().view(np.uint32) == SENTINEL).all(), "a refused call wrote an output word"
        return rc

    inv, cap_err = _abi.AF_ERR_INVALID, _abi.AF_ERR_CAPACITY
    assert call(edges=(0,)) == inv                                   # n_windows == 0
    assert call(edges=(0, 10, 10)) == inv and call(edges=(5, 4, 9)) == inv
    for bad in (0.0, -P, float("nan"), float("inf"), -float("inf")):
        assert call(period=bad) == inv, bad
    assert call(group=grp_bad) == inv
    assert call(clock=False) == inv and call(counts=False) == inv and call(tick_cap=0) == inv
    assert call(count=False) == inv and call(bins=0) == inv and call(bins=1025) == inv and call(hist=False) == inv
    assert call(n_groups=0) == inv and call(n=0) == inv
    assert call(n_groups=65537, edges=big) == cap_err                # n_groups * n_windows >= 2^32 - 1
    assert call(tick_cap=2 ** 31) == cap_err
    long_runs = np.zeros((3, _abi.CNT_SLOTS), dtype=np.uint32)
    long_runs[:, _abi.CNT_TICKS] = 2 ** 31 - 1
    full = torch.as_tensor(long_runs.view(np.int32), device=dev)
    assert call(n_groups=1, edges=(0, 2 ** 31 - 1), tick_cap=2 ** 31 - 1, counts_t=full) == cap_err   # a cell of 2^32 or more values
    plan_only = Engine(plan, PLAN_ONLY)
    try:
        assert call(plan_only._h) == _abi.AF_ERR_NO_DEVICE  # noqa: SLF001
    finally:
        plan_only.close()
    ok = b.run(eng, [0, 1, 2], 3, [0, 10, 64], threshold=1, bins=4)
    b.check(ok, [0, 1, 2], 3, [0, 10, 64], threshold=1, bins=4)


def test_cells_do_not_depend_on_the_launch_or_the_batch(eng):
    rng = np.random.default_rng(16)
    ticks = [CHUNK + 40, 300, CHUNK + 40, 180, 257]
    mine = [_clock(rng, m, t, "random") for m, t in zip((900, 300, 64, 1025, 10), ticks)]
    others = [_clock(rng, m, 400, "sorted") for m in (500, 0, 129, 700)]
    edges = [0, 100, 101, 256, CHUNK - 1, CHUNK + 1, CHUNK + 64]
    a = _Batch(mine, ticks, CHUNK + 64, cap=1100)
    group = [0, 1, 0, 2, 1]
    kw = {"threshold": 3, "bins": 7, "lo": 1}
    first = a.run(eng, group, 3, edges, **kw)
    a.check(first, group, 3, edges, **kw)
    again = a.run(eng, group, 3, edges, buf=first["buf"], **kw)       # the same buffers, written a second time
    order = [3, 0, 4, 2, 1]
    mixed = _Batch([others[0], mine[3], others[1], mine[0], mine[4], others[2], mine[2], mine[1], others[3]],
                   [400, ticks[3], 400, ticks[0], ticks[4], 400, ticks[2], ticks[1], 400], CHUNK + 64, cap=1100)
    where = [1, 3, 4, 6, 7]
    assert [mixed.stored[w].shape for w in where] == [a.stored[o].shape for o in order]
    group2 = np.array([3, -7, -1, -7, -7, 4, -7, -7, 3])
    group2[where] = [group[o] for o in order]
    other = mixed.run(eng, group2, 5, edges, **kw)
    mixed.check(other, group2, 5, edges, **kw)
    for k in CELL_KEYS:
        assert np.array_equal(first[k], again[k]), k
        assert np.array_equal(first[k], other[k][:3]), k
    for k in TICK_KEYS:
        assert np.array_equal(first[k], again[k]) and np.array_equal(first[k][order], other[k][where]), k


def test_event_workload_through_the_python_api(tmp_path):
    from asyncflow_amd import expand_grid
    from asyncflow_amd.runner import SimulationRunner

    payload = lb_with_events(horizon=60, scale=0.1)
    users = "rqs_input.avg_active_users.mean"
    grid = expand_grid({users: [60.0, 200.0]}, replicas=3, order_by_load=users)
    res = SimulationRunner(simulation_input=payload, **grid.runner_kwargs()).run()
    plan, n = res.plan, len(res)
    p = plan.sample_period
    per = [res[s] for s in range(n)]
    ticks = [min(int(r.counts[_abi.CNT_TICKS]), plan.tick_count) for r in per]
    series = [in_flight_series(r.rqs_clock, t, p) for r, t in zip(per, ticks)]
    assert max(int(s["in_flight"].max()) for s in series) >= 3

    def check(summ, ids, n_groups, b, thr=0, bins=0, lo=0):
        for g in range(n_groups):
            want = in_flight_window_stats([series[s]["in_flight"] for s in range(n) if ids[s] == g], b, thr, bins, lo)
            for k in ("count", "sum", "min", "max", "above"):
                assert np.array_equal(np.asarray(summ[k][g]).astype(np.uint64), np.asarray(want[k]).astype(np.uint64)), (k, g)
            some = want["count"] > 0
            mean = np.where(some, want["sum"].astype(np.float64) / np.maximum(want["count"], 1), np.nan)
            share = np.where(some, want["above"] / np.maximum(want["count"], 1), np.nan)
            assert np.array_equal(summ["mean"][g], mean, equal_nan=True) and np.array_equal(summ["above_share"][g], share, equal_nan=True)
            if bins:
                assert np.array_equal(summ["hist"][g, :, 0], want["hist"]) and np.array_equal(summ["under"][g, :, 0], want["under"])

    bins = max(int(res.in_flight_summary(10.0, by=grid)["max"].max()) + 2, 17)   # nothing reaches the last bin: exact quantiles
    assert bins <= 1024
    a = res.in_flight_summary(10.0, by=grid, threshold=2, bins=bins)
    b10 = a["tick_edges"]
    assert a["series"] == ["in_flight"] and a["mean"].shape == (2, len(b10) - 1) and a["replicas"].tolist() == [3, 3]
    assert np.array_equal(a["times"], b10[:-1] * p)
    check(a, grid.point, 2, b10, 2, bins, 0)
    assert (a["hist"][:, :, 0, -1] == 0).all()
    q = series_histogram_quantiles(a, [0.5, 0.99])
    for g in range(2):
        pooled = np.concatenate([series[s]["in_flight"][b10[0]: b10[1]] for s in range(n) if grid.point[s] == g]).astype(np.float64)
        assert np.array_equal(q[g, 0, 0], np.quantile(pooled, [0.5, 0.99]))
    one = res.in_flight_summary(ticks_per_window=333, by="scenario", threshold=1)
    check(one, np.arange(n), n, one["tick_edges"], 1)
    skip = np.where(np.arange(n) % 4 == 0, -1, grid.point)
    check(res.in_flight_summary(tick_edges=[5, 6, 700, 10 ** 6], by=skip, bins=3, lo=2), skip, 2, [5, 6, 700, 10 ** 6], 0, 3, 2)
    with pytest.raises(ValueError, match="bins"):
        res.in_flight_summary(bins=1025)
    with pytest.raises(ValueError, match="one of"):
        res.in_flight_summary(10.0, ticks_per_window=5)
    # bands over the replicas of a point
    bands = res.in_flight_bands(10.0, by=grid, threshold=2)
    own = res.in_flight_summary(10.0, by="scenario", threshold=2)
    for g in range(2):
        rows = own["mean"][grid.point == g]
        assert np.allclose(bands["mean"][g], rows.mean(axis=0), rtol=1e-12) and np.allclose(bands["std"][g], rows.std(axis=0, ddof=1), rtol=1e-9)
        assert np.allclose(bands["q_hi"][g], np.quantile(rows, 0.95, axis=0), rtol=1e-12)
    assert np.array_equal(bands["pooled"], res.in_flight_summary(10.0, by=grid, threshold=2)["mean"]) and (bands["n"] == 3).all()
    with pytest.raises(ValueError, match="of must be"):
        res.in_flight_bands(10.0, of="min")
    # one scenario's per-tick arrays, and the Series of a ScenarioResults
    for i in (0, n - 1):
        got = res.in_flight(i)
        for k in TICK_KEYS:
            assert got[k].dtype == np.uint32 and np.array_equal(got[k], series[i][k]), (i, k)
        times, vals = per[i].get_in_flight()
        assert np.array_equal(np.asarray(vals), series[i]["in_flight"].astype(np.float64)) and times[:2] == [0.0, p]
    with pytest.raises(IndexError):
        res.in_flight(n)
    # Little's law, side by side (informational: nothing asserts the ratio)
    ll = res.littles_law(10.0, by=grid)
    lat = res.window_summary(edges=ll["edges"], by=grid, window_of="arrival")["stats"].cpu().numpy()
    assert np.array_equal(ll["tick_edges"], b10) and np.array_equal(ll["edges"], b10 * p)
    assert np.array_equal(ll["L"], res.in_flight_summary(10.0, by=grid)["mean"], equal_nan=True)
    assert np.array_equal(ll["completed"], lat[:, :, 0].astype(np.int64)) and np.array_equal(ll["W"], lat[:, :, 1], equal_nan=True)
    assert np.array_equal(ll["lambda_eff"], lat[:, :, 0] / (np.diff(ll["edges"])[None, :] * 3))
    ok = ll["lambda_eff"] * ll["W"] > 0
    assert ok.any() and np.array_equal(ll["ratio"][ok], (ll["L"] / (ll["lambda_eff"] * ll["W"]))[ok]) and np.isnan(ll["ratio"][~ok]).all()
    # the dump, in both formats
    for name in ("in_flight.npz", "in_flight.parquet"):
        written = res.save_in_flight_summary(str(tmp_path / name), grid, window_s=10.0, threshold=2, bins=16)
        back = load_summary(str(tmp_path / name))
        assert set(back) == set(written)
        for k, v in written.items():
            assert np.array_equal(np.asarray(back[k], dtype=v.dtype).reshape(v.shape), v, equal_nan=v.dtype.kind == "f"), (name, k)
        assert np.array_equal(written["in_flight_mean"], a["mean"], equal_nan=True) and np.array_equal(written["in_flight_max"], a["max"])
        assert np.array_equal(written["in_flight_hist"][:, :, :15], a["hist"][:, :, 0, :15]) and written["in_flight_hist"].shape[2] == 16
