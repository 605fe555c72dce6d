"""Latency by the state a request met on arrival on the MI355X (af_engine_summarize_state_windows /
af_engine_summarize_state_quantiles, asyncflow_amd/csrc/af_state.hpp): every output word against the host definition
(results.latency_state_cells per scenario, concatenated per group in ascending scenario index) -- bit for bit.  Synthetic clocks
and sample blocks through the C ABI, in the series layout of a single-server plan with a dyadic period, cover the wave / unroll
seams of the stable partition, start orders, starts before the first and past the last sample, cell counts on both sides of the
LDS bound, with and without windows, integer and float columns, groups, skipped ids and all three tiers of both analyzers; an
event workload goes through the Python API."""

from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from asyncflow_amd import _abi
from asyncflow_amd.plan import lower
from asyncflow_amd.results import latency_state_cells, load_summary, window_edges
from oracle.scenarios import lb_with_events, single_server

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
LDS_BOUND = int(re.search(r"constexpr\s+uint32_t\s+kLdsStateCells\s*=\s*(\d+)\s*;",
                          (ROOT / "asyncflow_amd" / "csrc" / "af_state.hpp").read_text()).group(1))
P = 2.0 ** -5
ROWS = [0, 1, 63, 64, 65, 255, 256, 257, 1025]      # the wave and unroll seams of the partition (64, 4 x 64 rows)
ORDERS = ("sorted", "reversed", "random", "one")
LEVELS = [0.0, 0.5, 0.95, 0.999, 1.0]
THRESHOLDS = [2.0 ** -4, 0.0, 1.5]
LAT_POOL = np.array([0.0, 0.0, 2.0 ** -4, 2.0 ** -4, 2.0 ** -4, 2.0 ** -20, 1.0, 1.0, 3.0, 2.0 ** 40, 0.75, 2.0 ** -9])
FILL = 0x4F000000                                   # padding words and rows at or past t_s: 2^31 as a float, 1 325 400 064 as a count
READY, IO, RAM = 3, 4, 5                            # the series of the plan below: three edges, then ready / io / ram of srv-1
TICK_CAP = 1600


@pytest.fixture(scope="module")
def plan():
    p = lower(single_server(horizon=50, period=P))
    assert p.n_edges == 3 and p.n_series == 6 and p.series_pitch == 8 and p.sample_period == P
    return p


@pytest.fixture(scope="module")
def eng(plan):
    from asyncflow_amd.engine import Engine

    e = Engine(plan, 0)
    yield e
    e.close()


def _np_stats(lat: np.ndarray) -> np.ndarray:
    lat = np.ascontiguousarray(lat, dtype=np.float64)
    if lat.size == 0:
        return np.array([0.0] + [np.nan] * 7)
    if lat.size == 1:   # (numpy's results on one element, without eight calls: most cells of the wide requests)
        x = float(lat[0])
        return np.array([1.0, x, x, 0.0, x, x, x, x])
    return np.array([float(lat.size), float(np.mean(lat)), float(np.median(lat)), float(np.std(lat)),
                     float(np.percentile(lat, 95)), float(np.percentile(lat, 99)), float(np.min(lat)), float(np.max(lat))])


def _samples(rng, n, ticks, top):
    """Sample blocks [n, TICK_CAP, 8]: counts 0 .. top + 2 with half of the mass at 0 (ready, io, the edges), ram multiples of
    1/256 in [-1, top + 2) with -0.0, the -2^-45 residue and whole values; padding and rows at or past t_s hold FILL."""
    blk = np.full((n, TICK_CAP, 8), FILL, dtype=np.uint32)
    u = rng.random((n, TICK_CAP, 6))
    body = np.where(u < 0.5, 0, rng.integers(0, top + 3, (n, TICK_CAP, 6))).astype(np.uint32)
    f = (rng.integers(-256, (top + 2) * 256, (n, TICK_CAP)) / 256.0).astype(np.float32)
    f[u[:, :, RAM] < 0.1] = np.float32(-0.0)
    f[(u[:, :, RAM] >= 0.1) & (u[:, :, RAM] < 0.2)] = np.float32(-(2.0 ** -45))
    whole = (u[:, :, RAM] >= 0.2) & (u[:, :, RAM] < 0.4)
    f[whole] = rng.integers(0, top + 2, int(whole.sum())).astype(np.float32)
    body[:, :, RAM] = f.view(np.uint32)
    blk[:, :, :6] = body
    for s in range(n):
        blk[s, min(int(ticks[s]), TICK_CAP):] = FILL
    return blk


def _clock(rng, m, t_s, order, t_max):
    """m rows with dyadic starts (multiples of P / 4) from before the first sample to past the last one (and past t_max)."""
    last = min(t_s, TICK_CAP) + 3
    tick4 = rng.integers(0, 4 * last + 1, m)                        # start / (P / 4)
    if order == "one":
        tick4 = np.full(m, 4 * max(last // 2, 1) + 1)
    start = tick4 * (P / 4.0)
    start[rng.random(m) < 0.02] = t_max + 1.0                       # past every window
    if order in ("sorted", "reversed"):
        start = np.sort(start) if order == "sorted" else np.sort(start)[::-1]
    lat = LAT_POOL[rng.integers(0, LAT_POOL.size, m)]
    return np.stack([start, start + lat], axis=1)


class _Batch:
    """Clocks, sample blocks and counts on the device."""

    def __init__(self, clocks, blk, ticks, cap_limit=None, counts_extra=None):
        import torch

        n = len(clocks)
        self.n, self.cap = n, cap_limit or max(max((len(x) for x in clocks), default=1), 1)
        clock = np.full((n, self.cap, 2), np.nan)
        counts = np.zeros((n, _abi.CNT_SLOTS), dtype=np.uint32)
        self.stored, self.words = [], []
        for i, rows in enumerate(clocks):
            rows = np.asarray(rows, dtype=np.float64).reshape(-1, 2)
            counts[i, _abi.CNT_COMPLETED] = rows.shape[0] + (counts_extra[i] if counts_extra is not None else 0)
            counts[i, _abi.CNT_TICKS] = ticks[i]
            keep = rows[: self.cap]
            clock[i, : keep.shape[0]] = keep
            self.stored.append(keep)
            self.words.append(np.ascontiguousarray(blk[i, : min(int(ticks[i]), blk.shape[1]), :6].T))
        self.dev = torch.device("cuda", 0)
        self.tick_cap = blk.shape[1]
        self.clock_t = torch.as_tensor(clock, device=self.dev)
        self.blk_t = torch.as_tensor(blk.view(np.int32), device=self.dev)
        self.counts_t = torch.as_tensor(counts.view(np.int32), device=self.dev)

    def run(self, eng, group, n_groups, column, bins, lo=0.0, width=1.0, edges=None):
        """The two entry points: stats [G, W', bins, 8], row_bounds [n, K + 1], count [G, W', bins], quantiles, within (numpy)."""
        import torch

        n_win = 1 if edges is None else len(edges) - 1
        grp = np.asarray(group, dtype=np.int64)
        grp_t = torch.as_tensor(np.where(grp < 0, _abi.POOL_SKIP, grp).astype(np.uint32).view(np.int32), device=self.dev)
        shape = (n_groups, n_win, bins)
        stats = torch.full((*shape, 8), -7.0, dtype=torch.float64, device=self.dev)
        rb = torch.full((self.n, n_win * bins + 1), -1, dtype=torch.int32, device=self.dev)
        cnt = torch.full(shape, -3, dtype=torch.int32, device=self.dev)
        qt = torch.full((*shape, len(LEVELS)), -7.0, dtype=torch.float64, device=self.dev)
        wt = torch.full((*shape, len(THRESHOLDS)), -3, dtype=torch.int32, device=self.dev)
        torch.cuda.synchronize(self.dev)
        kw = {"column": column, "bins": bins, "lo": lo, "width": width, "sample_period": P, "edges": edges,
              "clock_ptr": self.clock_t.data_ptr(), "clock_capacity": self.cap, "samples_ptr": self.blk_t.data_ptr(),
              "tick_capacity": self.tick_cap, "counts_ptr": self.counts_t.data_ptr(), "group_ptr": grp_t.data_ptr()}
        eng.summarize_state_windows(self.n, n_groups, stats_ptr=stats.data_ptr(), row_bounds_ptr=rb.data_ptr(), **kw)
        eng.summarize_state_quantiles(self.n, n_groups, LEVELS, thresholds=THRESHOLDS, count_ptr=cnt.data_ptr(),
                                      quantiles_ptr=qt.data_ptr(), within_ptr=wt.data_ptr(), **kw)
        return {"stats": stats.cpu().numpy(), "row_bounds": rb.cpu().numpy().view(np.uint32), "count": cnt.cpu().numpy().view(np.uint32),
                "quantiles": qt.cpu().numpy(), "within": wt.cpu().numpy().view(np.uint32)}

    def cells(self, group, column, bins, lo=0.0, width=1.0, edges=None):
        """The host definition: {(g, key): latencies} of the non-empty cells and the cumulative cell counts [n, K + 1]."""
        n_keys = (1 if edges is None else len(edges) - 1) * bins
        cum = np.zeros((self.n, n_keys + 1), dtype=np.uint32)
        parts: dict[tuple[int, int], list[np.ndarray]] = {}
        for s in range(self.n):
            per = latency_state_cells(self.stored[s], self.words[s], 3, P, column, bins, lo, width, edges)
            cum[s, 1:] = np.cumsum([x.size for x in per])
            if group[s] < 0:
                continue
            for key, lat in enumerate(per):
                if lat.size:
                    parts.setdefault((int(group[s]), key), []).append(lat)
        return {k: np.concatenate(v) for k, v in parts.items()}, cum


def _compare(got, cells, cum, n_groups, n_keys, what):
    assert np.array_equal(got["row_bounds"], cum), what
    sizes = np.zeros((n_groups, n_keys), dtype=np.int64)
    for (g, key), lat in cells.items():
        sizes[g, key] = lat.size
    st = got["stats"].reshape(n_groups, n_keys, 8)
    qt, wt = got["quantiles"].reshape(n_groups, n_keys, -1), got["within"].reshape(n_groups, n_keys, -1)
    assert np.array_equal(st[:, :, 0], sizes.astype(np.float64)), what
    empty = sizes == 0
    assert np.isnan(st[empty][:, 1:]).all(), what
    assert np.array_equal(got["count"].reshape(n_groups, n_keys), sizes.astype(np.uint32)), what
    assert np.isnan(qt[empty]).all() and (wt[empty] == 0).all(), what
    for (g, key), lat in cells.items():
        want = _np_stats(lat)
        assert np.array_equal(st[g, key].view(np.uint64), want.view(np.uint64)), (what, g, key, st[g, key], want)
        assert np.array_equal(qt[g, key].view(np.uint64), np.quantile(lat, LEVELS).view(np.uint64)), (what, g, key)
        assert wt[g, key].tolist() == [int(np.count_nonzero(lat <= t)) for t in THRESHOLDS], (what, g, key)


# (arrival windows, bins): one cell, bins only, both, and the cells of a group at the LDS bound and one past it, each way
SHAPES = [(0, 1), (0, 8), (3, 5), (60, 8), (0, LDS_BOUND), (LDS_BOUND // 7, 7), ((LDS_BOUND + 1) // 8, 8), (0, LDS_BOUND + 1)]


@pytest.mark.parametrize("n_time, bins", SHAPES)
def test_start_orders_row_seams_and_cell_counts(eng, n_time, bins):
    assert LDS_BOUND == 4095 and (LDS_BOUND // 7) * 7 == LDS_BOUND and ((LDS_BOUND + 1) // 8) * 8 == LDS_BOUND + 1
    rng = np.random.default_rng(2000 + 31 * n_time + bins)
    rows = ROWS + [700, 300, 130]
    n = len(rows)
    ticks = rng.integers(40, TICK_CAP, n)
    ticks[2], ticks[5], ticks[7] = 0, TICK_CAP + 500, 1                  # no sample row; counts above the tick capacity; one row
    t_max = (TICK_CAP + 3) * P
    clocks = [_clock(rng, m, int(ticks[k]), ORDERS[(k + bins) % len(ORDERS)], t_max) for k, m in enumerate(rows)]
    top = min(bins, 40) if bins < 1000 else bins
    blk = _samples(rng, n, ticks, top)
    extra = np.zeros(n, dtype=np.int64)
    extra[8] = 50                                                        # counts above the clock capacity: clamped
    batch = _Batch(clocks, blk, ticks, cap_limit=1025, counts_extra=extra)
    assert [s.shape[0] for s in batch.stored[:9]] == ROWS
    edges = None if n_time == 0 else np.linspace(P, t_max - 7 * P, n_time + 1)
    n_keys = max(n_time, 1) * bins
    groupings = {"one group": np.zeros(n, dtype=np.int64), "members": np.arange(n) % 4, "singletons": np.arange(n)}
    for g in groupings.values():
        g[10] = -1                                                       # one scenario left out
    filled = 0
    for column, lo, width in ((IO, 0.0, 1.0), (READY, 1.0, 1.0 if bins > 100 else 2.0), (RAM, -0.5, 1.0 if bins > 100 else 0.75)):
        for name, grp in groupings.items():
            n_groups = int(grp.max()) + 1
            got = batch.run(eng, grp, n_groups, column, bins, lo, width, edges)
            cells, cum = batch.cells(grp, column, bins, lo, width, edges)
            assert column != IO or cum[10].max() > 0                     # (the cumulative counts of the skipped scenario too)
            assert cum[2].max() == 0 and cum[0].max() == 0               # no sample row / no request: no cell
            _compare(got, cells, cum, n_groups, n_keys, f"W={n_time} bins={bins} column={column} {name}")
            filled = max(filled, len(cells))
    assert filled >= min(n_keys, 4)


def test_cells_of_every_tier_in_one_call(eng):
    """Cells of 8, 512, 513, 8 192 and 8 193 latencies (and an empty one): the wave, workgroup and tiled tiers of both analyzers
    read the layout the state kernels made; two identical calls give identical bytes."""
    rng = np.random.default_rng(11)
    sizes = [8, 512, 513, 8192, 0, 8193]
    split = [[3, 5, 0], [500, 0, 12], [1, 256, 256], [4000, 4000, 192], [0, 0, 0], [8193 - 4097 - 1, 4097, 1]]
    ticks = np.array([1200, 1500, 900])
    blk = np.full((3, TICK_CAP, 8), FILL, dtype=np.uint32)
    clocks = []
    for s in range(3):
        blk[s, : ticks[s], :6] = 99
        blk[s, : ticks[s], READY] = np.arange(ticks[s]) % 6              # the ready queue at tick k: k % 6, the bin
        b = np.concatenate([np.full(split[c][s], c) for c in range(len(sizes))])
        rng.shuffle(b)
        k = rng.integers(0, ticks[s] // 6, b.size) * 6 + b               # a tick whose sample lies in the wanted bin
        start = (k + 1) * P + rng.integers(0, 4, b.size) * (P / 4.0)     # at the sample or before the next one
        clocks.append(np.stack([start, start + rng.lognormal(-3.0, 0.8, b.size)], axis=1))
    batch = _Batch(clocks, blk, ticks)
    cells, cum = batch.cells([0, 0, 0], READY, 6)
    assert [cells[0, c].size if (0, c) in cells else 0 for c in range(len(sizes))] == sizes
    got = batch.run(eng, [0, 0, 0], 1, READY, 6)
    _compare(got, cells, cum, 1, 6, "tiers")
    again = batch.run(eng, [0, 0, 0], 1, READY, 6)
    for k, v in got.items():
        assert v.tobytes() == again[k].tobytes(), k
    # the same rows behind two windows: the tiers' cells move to the keys of their windows
    edges = [0.0, 20.0, 60.0]
    cells, cum = batch.cells([0, 0, 0], READY, 6, edges=edges)
    _compare(batch.run(eng, [0, 0, 0], 1, READY, 6, edges=edges), cells, cum, 1, 12, "tiers in windows")


def _with_state(batch, s):
    rows = batch.stored[s]
    q = np.floor(rows[:, 0] / P)
    return rows[(rows[:, 0] >= 0) & (q >= 1) & (q - 1 < batch.words[s].shape[1])]


def test_one_bin_is_the_arrival_call_and_one_cell_the_pooled_call_on_the_rows_with_a_state(eng):
    import torch

    rng = np.random.default_rng(21)
    rows = [0, 5, 700, 3000, 257]
    ticks = np.array([100, 900, 1300, 1600, 64])
    t_max = (TICK_CAP + 3) * P
    clocks = [_clock(rng, m, int(ticks[k]), "random", 1e9) for k, m in enumerate(rows)]
    blk = _samples(rng, 5, ticks, 40)
    batch = _Batch(clocks, blk, ticks)
    grp = np.array([0, 1, 0, 1, 1])
    edges = np.linspace(0.0, t_max, 9)
    # ONE bin from below every value: the condition is "has a state", the cells are the arrival windows'
    got = batch.run(eng, grp, 2, RAM, 1, lo=-4.0, width=1.0, edges=edges)
    kept = [_with_state(batch, s) for s in range(5)]
    assert sum(k.shape[0] for k in kept) < sum(rows) and got["stats"][:, :, 0, 0].sum() == sum(k.shape[0] for k in kept)
    ref = _Batch(kept, blk, ticks)
    dev = ref.dev
    grp_t = torch.as_tensor(grp.astype(np.int32), device=dev)
    stats = torch.full((2, 8, 8), -7.0, dtype=torch.float64, device=dev)
    cnt = torch.full((2, 8), -3, dtype=torch.int32, device=dev)
    qt = torch.full((2, 8, len(LEVELS)), -7.0, dtype=torch.float64, device=dev)
    wt = torch.full((2, 8, len(THRESHOLDS)), -3, dtype=torch.int32, device=dev)
    kw = {"clock_ptr": ref.clock_t.data_ptr(), "clock_capacity": ref.cap, "counts_ptr": ref.counts_t.data_ptr(), "group_ptr": grp_t.data_ptr()}
    torch.cuda.synchronize(dev)
    eng.summarize_windows(5, 2, edges, stats_ptr=stats.data_ptr(), window_of="arrival", **kw)
    eng.summarize_quantiles(5, 2, LEVELS, edges=edges, thresholds=THRESHOLDS, count_ptr=cnt.data_ptr(), quantiles_ptr=qt.data_ptr(),
                            within_ptr=wt.data_ptr(), window_of="arrival", **kw)
    assert got["stats"].tobytes() == stats.cpu().numpy().tobytes()
    assert got["count"].tobytes() == cnt.cpu().numpy().tobytes() and got["quantiles"].tobytes() == qt.cpu().numpy().tobytes()
    assert got["within"].tobytes() == wt.cpu().numpy().tobytes()
    # ONE window and one bin: the pooled analyzer on those rows
    got = batch.run(eng, grp, 2, IO, 1, lo=0.0, width=1.0)
    pooled = torch.full((2, 8), -7.0, dtype=torch.float64, device=dev)
    eng.summarize_pooled(5, 2, stats_ptr=pooled.data_ptr(), **kw)
    assert got["stats"].tobytes() == pooled.cpu().numpy().tobytes() and got["stats"][:, 0, 0, 0].sum() == sum(k.shape[0] for k in kept)


def test_refusals_touch_no_output(eng, plan):
    import torch

    dev = torch.device("cuda", 0)
    clock = torch.zeros((2, 4, 2), dtype=torch.float64, device=dev)
    blk = torch.zeros((2, 4, 8), dtype=torch.int32, device=dev)
    counts = torch.zeros((2, _abi.CNT_SLOTS), dtype=torch.int32, device=dev)
    stats = torch.full((1, 1, 4, 8), -7.0, dtype=torch.float64, device=dev)
    cnt = torch.full((1, 1, 4), -3, dtype=torch.int32, device=dev)
    lib, h = eng._lib, eng._h  # noqa: SLF001
    good_out = (4, C.c_void_p(clock.data_ptr()), 4, C.c_void_p(blk.data_ptr()), C.c_void_p(counts.data_ptr()))
    good_sb = (0, 4, 0.0, 1.0, P)
    lv = (C.c_double * 1)(0.5)
    edges = (C.c_double * 2)(0.0, 1.0)

    def call(out=good_out, sb=good_sb, n_windows=0, e=None, n_groups=1):
        o, b = _abi.AfOutputs(*out), _abi.AfStateBins(*sb)
        wreq = _abi.AfWindows(2, n_groups, n_windows, None, e, C.c_void_p(stats.data_ptr()), None, 0.0, 0)
        qreq = _abi.AfQuantiles(2, n_groups, n_windows, None, e, 1, lv, 0, None, C.c_void_p(cnt.data_ptr()), None, None, 0.0, 0)
        rc = (lib.af_engine_summarize_state_windows(h, C.byref(o), C.byref(b), C.byref(wreq)),
              lib.af_engine_summarize_state_quantiles(h, C.byref(o), C.byref(b), C.byref(qreq)))
        assert rc[0] == rc[1], rc
        return rc[0]

    S = plan.n_series
    invalid = [{"sb": (0, 0, 0.0, 1.0, P)}, {"sb": (0, 4, 0.0, 0.0, P)}, {"sb": (0, 4, 0.0, -1.0, P)}, {"sb": (0, 4, 0.0, np.nan, P)},
               {"sb": (0, 4, 0.0, np.inf, P)}, {"sb": (0, 4, np.nan, 1.0, P)}, {"sb": (0, 4, -np.inf, 1.0, P)}, {"sb": (0, 4, 0.0, 1.0, 0.0)},
               {"sb": (0, 4, 0.0, 1.0, -P)}, {"sb": (0, 4, 0.0, 1.0, np.nan)}, {"sb": (0, 4, 0.0, 1.0, np.inf)}, {"sb": (S, 4, 0.0, 1.0, P)},
               {"out": good_out[:3] + (None,) + good_out[4:]}, {"out": good_out[:4] + (None,)}, {"out": good_out[:2] + (0,) + good_out[3:]},
               {"out": (4, None) + good_out[2:]}, {"n_windows": 0, "e": edges}, {"n_windows": 1, "e": None},
               {"n_windows": 1, "e": (C.c_double * 2)(1.0, 1.0)}]
    for kw in invalid:
        assert call(**kw) == _abi.AF_ERR_INVALID, kw
    assert call(sb=(0, 2 ** 31, 0.0, 1.0, P), n_groups=2) == _abi.AF_ERR_CAPACITY
    assert call(sb=(0, 2 ** 32 - 1, 0.0, 1.0, P)) == _abi.AF_ERR_CAPACITY
    assert (stats.cpu().numpy() == -7.0).all() and (cnt.cpu().numpy() == -3).all()
    assert call() == _abi.AF_OK and call(n_windows=1, e=edges) == _abi.AF_OK
    assert (stats.cpu().numpy()[..., 0] == 0.0).all() and (cnt.cpu().numpy() == 0).all()


def test_event_workload_through_the_python_api(tmp_path):
    from asyncflow_amd import expand_grid
    from asyncflow_amd.runner import SimulationRunner

    payload = lb_with_events(horizon=60, scale=0.1)
    users = "rqs_input.avg_active_users.mean"
    grid = expand_grid({users: [40.0, 120.0, 300.0]}, replicas=4, order_by_load=users)
    res = SimulationRunner(simulation_input=payload, **grid.runner_kwargs()).run()
    names = res.series_names()
    plan = res.plan
    per = [res[s] for s in range(len(res))]

    def host(col, bins, lo, width, edges, ids, n_groups):
        n_keys = (1 if edges is None else len(edges) - 1) * bins
        parts = [[[] for _ in range(n_keys)] for _ in range(n_groups)]
        for s, r in enumerate(per):
            if ids[s] >= 0:
                for key, lat in enumerate(latency_state_cells(r.rqs_clock, r._samples, plan.n_edges, plan.sample_period, col, bins, lo, width, edges)):  # noqa: SLF001
                    parts[ids[s]][key].append(lat)
        return [[np.concatenate(c) if c else np.zeros(0) for c in g] for g in parts]

    def check(series, col, bins, lo, width, window_s, by, ids, n_groups):
        edges = None if window_s is None else window_edges(window_s, plan.total_time)
        a = res.state_summary(series, bins, lo=lo, width=width, window_s=window_s, by=by)
        q = res.state_quantile_summary(series, [0.5, 0.99], thresholds=[0.2], bins=bins, lo=lo, width=width, window_s=window_s, by=by)
        n_win = 1 if edges is None else len(edges) - 1
        assert a["series"] == q["series"] == col and tuple(a["stats"].shape) == (n_groups, n_win, bins, 8)
        assert a["bin_lo"].tolist() == [lo + k * width for k in range(bins)]
        assert (a["edges"] is None) if edges is None else np.array_equal(a["edges"], edges)
        st = a["stats"].cpu().numpy().reshape(n_groups, n_win * bins, 8)
        qt = q["quantiles"].cpu().numpy().reshape(n_groups, n_win * bins, 2)
        cnt, wt = q["count"].cpu().numpy().reshape(n_groups, -1), q["within"].cpu().numpy().reshape(n_groups, -1)
        sh = q["share"].cpu().numpy().reshape(n_groups, -1)
        filled = 0
        for g, cells in enumerate(host(col, bins, lo, width, edges, ids, n_groups)):
            for key, lat in enumerate(cells):
                assert np.array_equal(st[g, key].view(np.uint64), _np_stats(lat).view(np.uint64)), (series, g, key)
                assert cnt[g, key] == lat.size and wt[g, key] == np.count_nonzero(lat <= 0.2)
                if lat.size:
                    assert np.array_equal(qt[g, key].view(np.uint64), np.quantile(lat, [0.5, 0.99]).view(np.uint64)), (series, g, key)
                    assert sh[g, key] == np.count_nonzero(lat <= 0.2) / lat.size
                    filled += 1
                else:
                    assert np.isnan(qt[g, key]).all() and np.isnan(sh[g, key])
        return a, filled

    io = f"{plan.server_ids[0]}:event_loop_io_sleep"
    ram = f"{plan.server_ids[1]}:ram_in_use"
    one = np.zeros(len(res), dtype=np.int64)
    a, filled = check(io, names.index(io), 8, 0.0, 1.0, None, None, one, 1)
    assert filled >= 3 and a["stats"][0, 0, :, 0].sum().item() >= 0.99 * sum(r.rqs_clock.shape[0] for r in per)
    check(names.index(io), names.index(io), 8, 0.0, 1.0, 10.0, grid, grid.point, 3)
    check(ram, names.index(ram), 5, 0.0, 64.0, 20.0, grid, grid.point, 3)
    assert names[0].endswith(":edge_concurrent_connection")
    check(names[0], 0, 4, 0.0, 1.0, None, "scenario", np.arange(len(res)), len(res))
    skip = np.where(np.arange(len(res)) % 5 == 0, -1, grid.point)
    check(io, names.index(io), 3, 1.0, 2.0, 30.0, skip, skip, 3)
    with pytest.raises(ValueError, match="unknown series"):
        res.state_summary("nobody:ram_in_use")
    with pytest.raises(ValueError, match="bins"):
        res.state_summary(io, 0)
    with pytest.raises(ValueError, match="at least one"):
        res.state_quantile_summary(io, [])
    # the dump, in both formats
    want = res.state_summary(io, 8, window_s=20.0, by=grid)["stats"].cpu().numpy()
    for name in ("state.npz", "state.parquet"):
        written = res.save_state_summary(str(tmp_path / name), grid, series=io, bins=8, window_s=20.0, levels=[0.5, 0.99], thresholds=[0.2])
        back = load_summary(str(tmp_path / name))
        assert set(back) == set(written)
        for k, v in written.items():
            assert np.array_equal(np.asarray(back[k], dtype=v.dtype).reshape(v.shape), v, equal_nan=v.dtype.kind == "f"), (name, k)
        assert np.array_equal(written["state_pooled:p95"], want[..., 4], equal_nan=True) and written["state_series"].tolist() == [names.index(io)]
        assert written["state_bin_lo"].tolist() == list(range(8)) and written["window_edges"].tolist() == [0.0, 20.0, 40.0, 60.0]
