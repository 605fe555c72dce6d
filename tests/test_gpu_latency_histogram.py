"""Log-linear latency histograms on the MI355X (af_engine_summarize_latency_histogram, asyncflow_amd/csrc/af_latency_histogram.hpp):
every output word against the host definition (results.latency_histogram per group).  Synthetic clocks through the C ABI: the wave,
unroll and chunk seams of the row walk, sorted, reversed and unsorted rows, latencies on the bin edges and on their float neighbours
with zero, negative, NaN and infinite ones, times exactly on the window edges, windows that fill the wave's LDS histogram and tiny
ones that go to memory directly, window counts on both sides of the kernel's LDS-resident limit, group arrangements, three binnings,
every optional output present and absent, every refusal, and the independence of the launch.  Every output of a call lies in ONE
buffer with sentinel words on both sides of each.  An event workload goes through the Python API, a hand-built sharded run included."""

from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from asyncflow_amd import _abi
from asyncflow_amd.plan import lower
from asyncflow_amd.results import (ShardedResults, latency_bin_edges, latency_histogram, latency_histogram_merge,
                                   latency_histogram_quantiles, load_summary)
from oracle.scenarios import lb_with_events, single_server

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "asyncflow_amd" / "csrc" / "af_latency_histogram.hpp").read_text()
LDS_WINDOWS = int(re.search(r"constexpr\s+uint32_t\s+kLdsHistogramWindows\s*=\s*(\d+)\s*;", HEADER).group(1))
CHUNK = int(re.search(r"constexpr\s+uint32_t\s+kChunkRows\s*=\s*(\d+)\s*;", HEADER).group(1))
ROWS = [0, 1, 63, 64, 65, 255, 256, 257, 1025]      # the wave and unroll seams of the row walk
ORDERS = ("sorted", "reversed", "random")
BINNINGS = [(0, -3, 1), (5, -20, 32), (8, -10, 16)]  # one bin, the default, 4 096 bins
SENTINEL = 0x5A5A5A5A
GUARD = 16                                          # sentinel words on both sides of every output
KEYS = ("count", "hist", "under", "over", "nan")
T = 16.0                                            # the synthetic clocks' times are multiples of 1/4 in [-1, T + 2]


def _edges(n_win: int):
    """Window edges the clocks' times fall exactly on; None: no windows."""
    if n_win == 0:
        return None
    if n_win == 1:
        return np.array([0.0, T])
    if n_win == 3:
        return np.array([0.25, 4.0, 4.25, 12.0])
    step = 0.25 if n_win <= 64 else 1.0 / 64.0
    return 0.5 + step * np.arange(n_win + 1)


@pytest.fixture(scope="module")
def eng():
    from asyncflow_amd.engine import Engine

    e = Engine(lower(single_server(horizon=50)), 0)
    yield e
    e.close()


def _clock(rng, m, order, binning=(5, -20, 32)):
    """m rows: starts multiples of 1/4 from before the first edge to past the last (a fifth at 0, where start + latency is exact);
    latencies on the bin edges and their float neighbours, multiples of 1/4 (finishes on window edges), zero and tiny ones; NaN,
    negative, reversed and infinite rows mixed in."""
    E = latency_bin_edges(*binning)
    start = rng.integers(-4, int(4 * T) + 9, m) / 4.0
    start[rng.random(m) < 0.2] = 0.0
    pick = E[rng.integers(0, E.shape[0], m)]
    lat = np.where(rng.random(m) < 0.4, np.nextafter(pick, rng.choice([-np.inf, np.inf], m)), pick)
    lat = np.where(rng.random(m) < 0.4, rng.integers(0, 17, m) / 4.0, lat)
    lat = np.where(rng.random(m) < 0.3, rng.lognormal(-3.0, 1.0, m), lat)
    rows = np.stack([start, start + lat], axis=1)
    key = rows[:, 1]
    if order == "sorted":
        rows = rows[np.argsort(key, kind="stable")]
    elif order == "reversed":
        rows = rows[np.argsort(key, kind="stable")[::-1]]
    if m > 12:
        at = rng.choice(m, 9, replace=False)
        for k, bad in zip(at, ([np.nan, 1.0], [2.0, np.nan], [3.0, 2.0], [1.0, np.inf], [-np.inf, 1.0], [np.inf, np.inf], [1.0, -np.inf],
                               [2.0, 2.0], [-0.0, 0.0])):
            rows[k] = bad
    return np.ascontiguousarray(rows)


class _Batch:
    """Clocks and counts on the device; rows behind a scenario's stored ones hold requests that would count if they were read."""

    def __init__(self, clocks, cap=None, counts_extra=0):
        import torch

        n = len(clocks)
        self.n = n
        self.cap = cap or max(max((len(x) for x in clocks), default=1), 1) + 3
        clock = np.empty((n, self.cap, 2))
        clock[:, :, 0], clock[:, :, 1] = 1.0, 1.5                    # (in every window arrangement's range, latency 0.5)
        counts = np.zeros((n, _abi.CNT_SLOTS), dtype=np.uint32)
        self.stored = []
        for i, rows in enumerate(clocks):
            rows = np.asarray(rows, dtype=np.float64).reshape(-1, 2)
            counts[i, _abi.CNT_COMPLETED] = rows.shape[0] + counts_extra
            keep = rows[: self.cap]
            clock[i, : keep.shape[0]] = keep
            self.stored.append(clock[i, : min(rows.shape[0] + counts_extra, self.cap)].copy())
        self.dev = torch.device("cuda", 0)
        self.clock_t = torch.as_tensor(clock, device=self.dev)
        self.counts_t = torch.as_tensor(counts.view(np.int32), device=self.dev)

    @staticmethod
    def layout(n_groups, n_win, n_bins, want):
        """Word offsets of the wanted outputs in one buffer, GUARD sentinel words before, between and behind them."""
        cells = n_groups * max(n_win, 1)
        sizes = {"count": 2 * cells, "hist": cells * n_bins, "under": cells, "over": cells, "nan": cells}
        off, at = {}, GUARD
        for k in KEYS:
            if k in want:
                off[k] = (at, sizes[k])
                at += sizes[k] + (sizes[k] & 1) + GUARD              # (even: the u64 counts stay 8-byte aligned)
        return off, at

    def run(self, eng, group, n_groups, edges, window_of="finish", binning=(5, -20, 32), want=KEYS, buf=None):
        """One call; returns the outputs (numpy) after checking that no word outside them changed."""
        import torch

        m, e0, o = binning
        n_win = 0 if edges is None else len(edges) - 1
        off, total = self.layout(n_groups, n_win, o << m, want)
        if buf is None:
            buf = torch.full((total,), SENTINEL, dtype=torch.int32, device=self.dev)
        grp_t = None
        if group is not None:
            grp = np.asarray(group, dtype=np.int64)
            grp_t = torch.as_tensor(np.where(grp < 0, _abi.POOL_SKIP, grp).astype(np.uint32).view(np.int32), device=self.dev)
        ptr = {k: buf.data_ptr() + 4 * o_ for k, (o_, _) in off.items()}
        torch.cuda.synchronize(self.dev)
        ms, scratch = eng.summarize_latency_histogram(
            self.n, n_groups, edges=edges, window_of=window_of, sub_bits=m, min_exp=e0, octaves=o, clock_ptr=self.clock_t.data_ptr(),
            clock_capacity=self.cap, counts_ptr=self.counts_t.data_ptr(), count_ptr=ptr["count"], hist_ptr=ptr["hist"],
            under_ptr=ptr.get("under", 0), over_ptr=ptr.get("over", 0), nan_ptr=ptr.get("nan", 0),
            group_ptr=grp_t.data_ptr() if grp_t is not None else 0)
        assert ms > 0.0 and scratch >= 0
        words = buf.cpu().numpy().view(np.uint32)
        inside = np.zeros(total, dtype=bool)
        out = {}
        for k, (o_, size) in off.items():
            inside[o_: o_ + size] = True
            out[k] = words[o_: o_ + size].copy()
        assert (words[~inside] == SENTINEL).all(), "a word outside the outputs changed"
        shape = (n_groups, max(n_win, 1))
        out["count"] = out["count"].view(np.uint64)
        for k in KEYS:
            if k in out:
                out[k] = out[k].reshape(shape + ((o << m,) if k == "hist" else ()))
        out["buf"] = buf
        return out

    def check(self, got, group, n_groups, edges, window_of="finish", binning=(5, -20, 32)):
        """Every word of `got` against the host definition."""
        m, e0, o = binning
        grp = np.zeros(self.n, dtype=np.int64) if group is None else np.asarray(group, dtype=np.int64)
        for g in range(n_groups):
            members = [self.stored[s] for s in range(self.n) if grp[s] == g]
            want = latency_histogram(members, edges, window_of, sub_bits=m, min_exp=e0, octaves=o)
            for k in KEYS:
                if k in got:
                    assert got[k][g].dtype == want[k].dtype and np.array_equal(got[k][g], want[k]), (k, g, window_of, binning)

    def both(self, eng, group, n_groups, edges, window_of="finish", binning=(5, -20, 32), **kw):
        got = self.run(eng, group, n_groups, edges, window_of, binning, **kw)
        self.check(got, group, n_groups, edges, window_of, binning)
        return got


GROUPS9 = ((None, 1), (np.arange(9), 9), ([0, 2, 2, -1, 0, 2, 2, 2, 0], 4))       # NULL, singletons, two uneven groups + a skip + empty ones


@pytest.mark.parametrize("order", ORDERS)
def test_row_counts_orders_windows_groups_and_binnings(eng, order):
    rng = np.random.default_rng(ORDERS.index(order))
    for binning in BINNINGS:
        b = _Batch([_clock(rng, m, order, binning) for m in ROWS])
        for n_win in (0, 1, 3, 61):
            edges = _edges(n_win)
            for group, G in GROUPS9:
                for window_of in ("finish", "arrival") if n_win else ("finish",):
                    got = b.both(eng, group, G, edges, window_of, binning)
        assert int(got["count"].sum()) > 0 and (got["count"][1] == 0).all() and (got["hist"][3] == 0).all()   # the empty groups 1 and 3
    full = b.run(eng, None, 1, None, "finish", binning)
    assert int(full["count"][0, 0]) == sum(ROWS) and int(full["nan"][0, 0]) >= 4 and int(full["under"][0, 0]) > 0 and int(full["over"][0, 0]) > 0


@pytest.mark.parametrize("n", [1, 5, 67])
def test_scenario_counts_chunk_seams_and_clipped_counts(eng, n):
    rng = np.random.default_rng(20 + n)
    sizes = [int(x) for x in rng.integers(0, 700, n)]
    sizes[0] = 2 * CHUNK + 65                                       # three work items of one scenario
    if n > 2:
        sizes[1], sizes[2] = CHUNK, CHUNK + 1
    order = ORDERS[n % 3]
    b = _Batch([_clock(rng, m, order) for m in sizes], cap=2 * CHUNK + 70)
    group = np.arange(n) % 3 if n > 1 else None
    G = 3 if n > 1 else 1
    for n_win, window_of in ((0, "finish"), (3, "finish"), (3, "arrival"), (61, "finish"), (61, "arrival")):
        b.both(eng, group, G, _edges(n_win), window_of)
    b.both(eng, np.arange(n), n, _edges(3), "finish", (2, -8, 6))
    # counts above the capacity are clipped; the rows behind the stored ones are not read
    c = _Batch([_clock(rng, m, "random") for m in sizes[: min(n, 5)]], cap=600, counts_extra=2)
    assert all(len(x) <= 600 for x in c.stored) and any(len(x) == 600 for x in c.stored)
    c.both(eng, None, 1, _edges(3))
    c.both(eng, np.arange(c.n), c.n, None)


def test_window_counts_around_the_lds_resident_limit(eng):
    rng = np.random.default_rng(31)
    b = _Batch([_clock(rng, m, o) for m, o in ((1500, "sorted"), (900, "random"), (64, "reversed"), (0, "sorted"))])
    for n_win in (LDS_WINDOWS, LDS_WINDOWS + 1):
        edges = _edges(n_win)
        for window_of in ("finish", "arrival"):
            b.both(eng, [0, 1, 0, 1], 2, edges, window_of, (2, -8, 6))
        got = b.both(eng, None, 1, edges, "finish")
        assert int(got["count"].sum()) > 100
        # the same rows in a few wide windows: the sums over the windows agree
        wide = b.both(eng, None, 1, edges[[0, n_win // 2, n_win]], "finish")
        assert int(wide["count"].sum()) == int(got["count"].sum()) and np.array_equal(wide["hist"].sum(axis=1), got["hist"].sum(axis=1))


def test_every_optional_output_present_and_absent(eng):
    rng = np.random.default_rng(32)
    b = _Batch([_clock(rng, m, "sorted") for m in (700, 400, 50)])
    group, edges = [0, 1, 0], _edges(3)
    for drop in ((), ("under",), ("over",), ("nan",), ("under", "over"), ("under", "nan"), ("over", "nan"), ("under", "over", "nan")):
        want = tuple(k for k in KEYS if k not in drop)
        for e in (edges, None):
            got = b.both(eng, group, 2, e, want=want)
            assert set(got) - {"buf"} == set(want)
    got = b.both(eng, group, 2, edges)
    assert np.array_equal(got["under"].astype(np.uint64) + got["over"] + got["nan"] + got["hist"].sum(axis=2, dtype=np.uint64), got["count"])


def test_refusals_leave_every_output_word_alone(eng):
    import torch

    from asyncflow_amd.engine import PLAN_ONLY, Engine

    rng = np.random.default_rng(33)
    b = _Batch([_clock(rng, 40, "random") for _ in range(3)])
    lib, dev = eng._lib, b.dev  # noqa: SLF001
    cells, n_bins = 3 * 2, 1024
    buf = torch.full((GUARD + cells * (n_bins + 5) + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    base = buf.data_ptr() + 4 * GUARD
    grp_ok = torch.zeros(3, dtype=torch.int32, device=dev)
    grp_bad = torch.as_tensor(np.array([0, 3, 1], dtype=np.int32), device=dev)

    def call(handle=None, *, n_groups=3, edges=(0.0, 1.0, 8.0), n_win=None, group=grp_ok, clock=True, counts=True, cap=b.cap, count=True,
             hist=True, n=3, binning=(5, -20, 32), by_arrival=0, counts_t=None):
        e = np.ascontiguousarray(edges, dtype=np.float64) if edges is not None else None
        out = _abi.AfOutputs(cap, C.c_void_p(b.clock_t.data_ptr() if clock else None), 0, None,
                             C.c_void_p((counts_t if counts_t is not None else b.counts_t).data_ptr() if counts else None))
        p = [C.c_void_p(base + 4 * cells * k) for k in (0, 2, 3, 4, 5)]                 # count, under, over, nan, hist
        req = _abi.AfLatencyHistogram(n, n_groups, (0 if e is None else e.shape[0] - 1) if n_win is None else n_win,
                                      C.c_void_p(group.data_ptr() if group is not None else None),
                                      e.ctypes.data_as(C.POINTER(C.c_double)) if e is not None else None, by_arrival, *binning,
                                      p[0] if count else C.c_void_p(None), p[4] if hist else C.c_void_p(None), p[1], p[2], p[3], 0.0, 0)
        torch.cuda.synchronize(dev)
        rc = lib.af_engine_summarize_latency_histogram(handle or eng._h, C.byref(out), C.byref(req))  # noqa: SLF001
        assert (buf.cpu().numpy().view(np.uint32) == SENTINEL).all(), "a refused call wrote an output word"
        return rc

    inv, cap_err = _abi.AF_ERR_INVALID, _abi.AF_ERR_CAPACITY
    assert call(n=0) == inv and call(n_groups=0) == inv
    for bad in ((9, -20, 1), (5, -1023, 4), (5, -20, 0), (5, 1000, 24), (5, -20, 129), (0, -1022, 4097), (8, 0, 17), (0, 2 ** 31 - 1, 1)):
        assert call(binning=bad) == inv, bad
    for bad in ((0.0, 1.0, 1.0), (2.0, 1.0, 3.0), (0.0, float("inf"), 9.0), (float("nan"), 1.0, 2.0), (-float("inf"), 0.0, 1.0)):
        assert call(edges=bad) == inv, bad
    assert call(edges=None, n_win=2) == inv                          # edges NULL with n_windows > 0
    assert call(edges=None, by_arrival=1) == inv                     # by arrival without windows
    assert call(group=grp_bad) == inv
    assert call(clock=False) == inv and call(counts=False) == inv and call(count=False) == inv and call(hist=False) == inv
    assert call(cap=0) == inv
    assert call(n_groups=2 ** 22, edges=None, group=None) == cap_err                    # 2^22 groups * 1 window * 1 024 bins = 2^32 words
    assert call(n_groups=2 ** 21, group=None) == cap_err and call(n_groups=2 ** 20, group=None, binning=(8, -10, 16)) == cap_err
    many = np.zeros((3, _abi.CNT_SLOTS), dtype=np.uint32)
    many[:, _abi.CNT_COMPLETED] = 2 ** 31
    full = torch.as_tensor(many.view(np.int32), device=dev)
    assert call(n_groups=1, cap=2 ** 31, counts_t=full) == cap_err   # a group of 3 * 2^31 stored rows
    plan_only = Engine(lower(single_server(horizon=50)), PLAN_ONLY)
    try:
        assert call(plan_only._h) == _abi.AF_ERR_NO_DEVICE  # noqa: SLF001
    finally:
        plan_only.close()
    b.both(eng, [0, 1, 2], 3, np.array([0.0, 1.0, 8.0]))


def test_cells_do_not_depend_on_the_launch_or_the_batch(eng):
    rng = np.random.default_rng(34)
    mine = [_clock(rng, m, o) for m, o in ((900, "sorted"), (300, "random"), (64, "reversed"), (CHUNK + 30, "sorted"), (10, "random"))]
    others = [_clock(rng, m, "sorted") for m in (500, 0, 129, 700)]
    a = _Batch(mine, cap=CHUNK + 40)
    group = [0, 1, 0, 2, 1]
    for edges, window_of in ((_edges(61), "finish"), (_edges(3), "arrival"), (None, "finish")):
        first = a.both(eng, group, 3, edges, window_of)
        again = a.run(eng, group, 3, edges, window_of, buf=first["buf"])            # the same buffers, written a second time
        order = [3, 0, 4, 2, 1]
        mixed = _Batch([others[0], mine[3], others[1], mine[0], mine[4], others[2], mine[2], mine[1], others[3]], cap=CHUNK + 40)
        where = [1, 3, 4, 6, 7]
        group2 = np.array([3, -7, -1, -7, -7, 4, -7, -7, 3])
        group2[where] = [group[o] for o in order]
        other = mixed.both(eng, group2, 5, edges, window_of)
        for k in KEYS:
            assert np.array_equal(first[k], again[k]), k
            assert np.array_equal(first[k], other[k][:3]), k
        alone = _Batch([mine[3]], cap=CHUNK + 40).both(eng, None, 1, edges, window_of)  # a scenario alone: the cell it has inside a batch
        single = a.both(eng, np.arange(5), 5, edges, window_of)
        for k in KEYS:
            assert np.array_equal(alone[k][0], single[k][3]), k


def test_event_workload_through_the_python_api(tmp_path):
    from asyncflow_amd import expand_grid
    from asyncflow_amd.runner import SimulationRunner

    payload = lb_with_events(horizon=60, scale=0.1)
    users = "rqs_input.avg_active_users.mean"
    grid = expand_grid({users: [60.0, 200.0]}, replicas=4, order_by_load=users)
    res = SimulationRunner(simulation_input=payload, **grid.runner_kwargs()).run()
    n = len(res)
    clocks = [res[s].rqs_clock for s in range(n)]
    e10 = np.arange(0.0, 61.0, 10.0)

    def check(summ, ids, n_groups, edges, window_of, **binning):
        for g in range(n_groups):
            want = latency_histogram([clocks[s] for s in range(n) if ids[s] == g], edges, window_of, **binning)
            for k in KEYS:
                got = summ[k].cpu().numpy()
                assert got.dtype == np.int64 and np.array_equal(got[g], want[k].astype(np.int64)), (k, g, window_of)

    summ = {}
    for window_of in ("finish", "arrival"):
        s = summ[window_of] = res.latency_histogram_summary(10.0, by=grid, window_of=window_of)
        assert s["hist"].shape == (2, 6, 1024) and s["count"].shape == (2, 6) and s["hist"].is_cuda
        assert np.array_equal(s["edges"], e10) and s["replicas"].tolist() == [4, 4] and s["bin_edges"].shape == (1025,)
        assert (s["sub_bits"], s["min_exp"], s["octaves"], s["window_of"]) == (5, -20, 32, window_of) and s["latency_histogram_ms"] > 0
        check(s, grid.point, 2, e10, window_of)
        stats = res.window_summary(10.0, by=grid, window_of=window_of)["stats"].cpu().numpy()
        assert np.array_equal(s["count"].cpu().numpy(), stats[:, :, 0].astype(np.int64)) and int(s["count"].sum()) > 1000
        levels = [0.5, 0.95, 0.99]
        exact = res.quantile_summary(levels, window_s=10.0, by=grid, window_of=window_of)["quantiles"].cpu().numpy()
        br = latency_histogram_quantiles(s, levels)
        some = s["count"].cpu().numpy() > 0
        assert some.any() and ((br["lo"][some] <= exact[some]) & (exact[some] < br["hi"][some])).all()
        assert (br["hi"][some] / br["lo"][some] <= (1.0 + 2.0 ** -5) ** 2 * (1.0 + 1e-12)).mean() > 0.5
    whole = res.latency_histogram_summary(by="scenario", sub_bits=3, min_exp=-12, octaves=12)
    assert whole["hist"].shape == (n, 1, 96) and whole["edges"] is None
    check(whole, np.arange(n), n, None, "finish", sub_bits=3, min_exp=-12, octaves=12)
    skip = np.where(np.arange(n) % 4 == 0, -1, grid.point)
    check(res.latency_histogram_summary(edges=[5.0, 6.0, 40.0, 1e6], by=skip, window_of="arrival"), skip, 2, [5.0, 6.0, 40.0, 1e6], "arrival")
    by_name = res.latency_histogram_summary(10.0, by=users)
    for k in KEYS:
        assert (by_name[k] == summ["finish"][k]).all(), k
    with pytest.raises(ValueError, match="arrival"):
        res.latency_histogram_summary(window_of="arrival")
    with pytest.raises(ValueError, match="octaves"):
        res.latency_histogram_summary(octaves=200)
    with pytest.raises(ValueError, match="parameter columns"):
        res.latency_histogram_summary(by=["no.such.column"])
    # the dump, in both formats, and the merge of what is read back
    for name in ("lhist.npz", "lhist.parquet"):
        written = res.save_latency_histogram_summary(str(tmp_path / name), grid, window_s=10.0)
        back = load_summary(str(tmp_path / name))
        assert set(back) == set(written)
        assert np.array_equal(np.asarray(back["lhist_hist"]).reshape(written["lhist_hist"].shape), summ["finish"]["hist"].cpu().numpy())
        twice = latency_histogram_merge(back, summ["finish"])
        for k in KEYS:
            assert np.array_equal(twice[k], 2 * summ["finish"][k].cpu().numpy()), (name, k)
        assert twice["replicas"].tolist() == [8, 8] and np.array_equal(twice["edges"], e10)
        q = latency_histogram_quantiles(back, [0.5])
        assert np.array_equal(q["lo"], latency_histogram_quantiles(summ["finish"], [0.5])["lo"], equal_nan=True)
    # a sweep on several devices, built by hand from the even and the odd scenarios on device 0
    index = [np.arange(0, n, 2), np.arange(1, n, 2)]
    shards = [SimulationRunner(simulation_input=payload, seeds=grid.seeds[ix], sweep={k: v[ix] for k, v in grid.columns.items()}).run() for ix in index]
    for shard, ix in zip(shards, index):
        for j, s in enumerate(ix):
            assert np.array_equal(shard[j].rqs_clock, clocks[s])
    sharded = ShardedResults(shards, index, 0.0)
    for by in (np.asarray(grid.point), grid, [users], users):
        for window_of in ("finish", "arrival"):
            got = sharded.latency_histogram_summary(10.0, by=by, window_of=window_of)
            for k in KEYS:
                assert got[k].dtype == summ[window_of][k].dtype and got[k].shape == summ[window_of][k].shape
                assert (got[k] == summ[window_of][k]).all(), (k, window_of)
            assert got["replicas"].tolist() == [4, 4] and np.array_equal(got["edges"], e10)
    per = sharded.latency_histogram_summary(by="scenario", sub_bits=3, min_exp=-12, octaves=12)
    assert (per["hist"] == whole["hist"]).all() and (per["count"] == whole["count"]).all()
    one_sided = sharded.latency_histogram_summary(10.0, by=np.where(np.arange(n) % 2 == 0, 1, -1))   # only the first shard has members
    check(one_sided, np.where(np.arange(n) % 2 == 0, 1, -1), 2, e10, "finish")
    with pytest.raises(NotImplementedError, match="several devices"):
        sharded.window_summary(10.0)
    with pytest.raises(NotImplementedError, match="several devices"):
        sharded.quantile_summary([0.5])
