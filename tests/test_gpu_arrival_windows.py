"""Latency windows by ARRIVAL time on the MI355X (af_engine_summarize_arrival_windows / af_engine_summarize_arrival_quantiles,
asyncflow_amd/csrc/af_arrival.hpp): every output word against the host definition -- boolean masks on start per scenario, the
latencies in row order, concatenated per group in ascending scenario index -- bit for bit.  Synthetic clocks through the C ABI
cover the wave / unroll seams of the stable partition, start orders from sorted to 64 windows in one wave, starts on edges and
outside the windows, window counts on both sides of the LDS bound and all three tiers of both analyzers; event workloads go
through the Python API."""

from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from asyncflow_amd import _abi
from asyncflow_amd.plan import lower
from asyncflow_amd.results import latency_window_quantiles, latency_window_stats, window_edges
from oracle.scenarios import lb_two_servers, lb_with_events, single_server

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
LDS_BOUND = int(re.search(r"constexpr\s+uint32_t\s+kLdsArrivalWindows\s*=\s*(\d+)\s*;",
                          (ROOT / "asyncflow_amd" / "csrc" / "af_arrival.hpp").read_text()).group(1))
ROWS = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049]      # the wave and unroll seams of the partition (64, 4 x 64 rows)
LEVELS = [0.0, 0.5, 0.95, 0.999, 1.0]
THRESHOLDS = [2.0 ** -4, 0.0, 1.5]
ORDERS = ("sorted", "reversed", "random", "spread", "one", "on_edge", "outside")
# dyadic latencies, so that finish = start + latency is exact for the dyadic starts below: ties, zeros, and magnitudes far enough
# apart that the order of a sum's terms shows in its last bits
LAT_POOL = np.array([0.0, 0.0, 2.0 ** -4, 2.0 ** -4, 2.0 ** -4, 2.0 ** -20, 1.0, 1.0, 3.0, 2.0 ** 40, 0.75, 2.0 ** -9])


def _np_stats(lat: np.ndarray) -> np.ndarray:
    lat = np.ascontiguousarray(lat, dtype=np.float64)
    if lat.size == 0:
        return np.array([0.0] + [np.nan] * 7)
    if lat.size == 1:   # (numpy's results on one element, without eight calls: most cells of the wide requests)
        x = float(lat[0])
        return np.array([1.0, x, x, 0.0, x, x, x, x])
    return np.array([float(lat.size), float(np.mean(lat)), float(np.median(lat)), float(np.std(lat)),
                     float(np.percentile(lat, 95)), float(np.percentile(lat, 99)), float(np.min(lat)), float(np.max(lat))])


def _upload(clocks, group, cap_limit=None, counts_extra=None):
    import torch

    n = len(clocks)
    cap = cap_limit or max(max((len(x) for x in clocks), default=1), 1)
    clock = np.full((n, cap, 2), np.nan)
    counts = np.zeros((n, _abi.CNT_SLOTS), dtype=np.uint32)
    stored = []
    for i, rows in enumerate(clocks):
        rows = np.asarray(rows, dtype=np.float64).reshape(-1, 2)
        counts[i, _abi.CNT_COMPLETED] = rows.shape[0] + (counts_extra[i] if counts_extra is not None else 0)
        keep = rows[:cap]
        clock[i, : keep.shape[0]] = keep
        stored.append(keep)
    dev = torch.device("cuda", 0)
    grp = np.asarray(group, dtype=np.int64)
    return (stored, cap, torch.as_tensor(clock, device=dev), torch.as_tensor(counts.view(np.int32), device=dev),
            torch.as_tensor(np.where(grp < 0, _abi.POOL_SKIP, grp).astype(np.uint32).view(np.int32), device=dev))


def _device(clocks, group, n_groups, edges, *, window_of="arrival", cap_limit=None, counts_extra=None, calls=("windows", "quantiles")):
    """Hand-made rqs_clock rows fed straight to the two entry points.  Returns the stored rows per scenario and a dict: stats
    [G, W, 8], row_bounds [n, W + 1], count [G, W], quantiles [G, W, Q], within [G, W, T] (numpy)."""
    import torch

    from asyncflow_amd.engine import Engine

    stored, cap, clock_t, counts_t, grp_t = _upload(clocks, group, cap_limit, counts_extra)
    dev = clock_t.device
    n, n_win = len(clocks), len(edges) - 1
    stats = torch.full((n_groups, n_win, 8), -7.0, dtype=torch.float64, device=dev)
    rb = torch.full((n, n_win + 1), -1, dtype=torch.int32, device=dev)
    cnt = torch.full((n_groups, n_win), -3, dtype=torch.int32, device=dev)
    qt = torch.full((n_groups, n_win, len(LEVELS)), -7.0, dtype=torch.float64, device=dev)
    wt = torch.full((n_groups, n_win, len(THRESHOLDS)), -3, dtype=torch.int32, device=dev)
    eng = Engine(lower(single_server(horizon=50)), 0)
    try:
        if "windows" in calls:
            eng.summarize_windows(n, n_groups, edges, clock_ptr=clock_t.data_ptr(), clock_capacity=cap, counts_ptr=counts_t.data_ptr(),
                                  stats_ptr=stats.data_ptr(), group_ptr=grp_t.data_ptr(), row_bounds_ptr=rb.data_ptr(), window_of=window_of)
        if "quantiles" in calls:
            eng.summarize_quantiles(n, n_groups, LEVELS, edges=edges, thresholds=THRESHOLDS, clock_ptr=clock_t.data_ptr(),
                                    clock_capacity=cap, counts_ptr=counts_t.data_ptr(), count_ptr=cnt.data_ptr(),
                                    quantiles_ptr=qt.data_ptr(), within_ptr=wt.data_ptr(), group_ptr=grp_t.data_ptr(), window_of=window_of)
    finally:
        eng.close()
    return stored, {"stats": stats.cpu().numpy(), "row_bounds": rb.cpu().numpy(), "count": cnt.cpu().numpy().view(np.uint32),
                    "quantiles": qt.cpu().numpy(), "within": wt.cpu().numpy().view(np.uint32)}


def _cells(stored, group, n_groups, edges):
    """The host definition: {(g, w): latencies} for the non-empty cells, and the cumulative counts [n, W + 1].  Per scenario the
    window of a row is found once (#{edges < start} - 1); the rows of a window are then taken by a boolean mask, in row order."""
    group = np.asarray(group)
    edges = np.asarray(edges, dtype=np.float64)
    n_win = len(edges) - 1
    cum = np.stack([(rows[:, 0][None, :] <= edges[:, None]).sum(axis=1) if n_win < 700
                    else np.searchsorted(np.sort(rows[:, 0]), edges, side="right") for rows in stored])
    parts: dict[tuple[int, int], list[np.ndarray]] = {}
    for s, rows in enumerate(stored):
        if group[s] < 0:
            continue
        start, lat = rows[:, 0], rows[:, 1] - rows[:, 0]
        win = (start[:, None] > edges[None, :]).sum(axis=1) - 1 if n_win < 700 else np.searchsorted(edges, start, side="left") - 1
        for w in np.unique(win[(win >= 0) & (win < n_win)]):
            assert ((start > edges[w]) & (start <= edges[w + 1]) == (win == w)).all()
            parts.setdefault((int(group[s]), int(w)), []).append(lat[win == w])
    return {k: np.concatenate(v) for k, v in parts.items()}, cum


def _compare(got, cells, cum, n_groups, n_win, what):
    assert np.array_equal(got["row_bounds"], cum), what
    sizes = np.zeros((n_groups, n_win), dtype=np.int64)
    for (g, w), lat in cells.items():
        sizes[g, w] = lat.size
    st = got["stats"]
    assert np.array_equal(st[:, :, 0], sizes.astype(np.float64)), what
    empty = sizes == 0
    assert np.isnan(st[empty][:, 1:]).all(), what
    assert np.array_equal(got["count"], sizes.astype(np.uint32)), what
    assert np.isnan(got["quantiles"][empty]).all() and (got["within"][empty] == 0).all(), what
    for (g, w), lat in cells.items():
        want = _np_stats(lat)
        assert np.array_equal(st[g, w].view(np.uint64), want.view(np.uint64)), (what, g, w, st[g, w], want)
        assert np.array_equal(got["quantiles"][g, w].view(np.uint64), np.quantile(lat, LEVELS).view(np.uint64)), (what, g, w)
        assert got["within"][g, w].tolist() == [int(np.count_nonzero(lat <= t)) for t in THRESHOLDS], (what, g, w)


def _clock(rng, m, edges, order):
    """m rows whose starts follow `order` over the windows of `edges` (dyadic, spacing 1): start = edge + k / 64."""
    n_win = len(edges) - 1
    i = np.arange(m)
    frac = rng.integers(1, 65, m) / 64.0                                   # (e[w], e[w + 1]]: 64 / 64 is ON the edge that ends the window
    if order in ("sorted", "reversed", "random"):                          # (the first two: the starts are sorted below)
        win = rng.integers(0, n_win, m)
    elif order == "spread":                                                # the 64 rows of a wave in 64 different windows (where there are 64)
        win = (i * max(n_win // 64, 1)) % n_win
    elif order == "one":
        win = np.full(m, n_win // 2)
    elif order == "on_edge":                                               # runs of equal starts exactly on an edge
        win = np.repeat(rng.integers(0, n_win, m // 5 + 1), rng.integers(1, 100, m // 5 + 1))[:m]
        win = np.resize(win, m)
        frac = np.full(m, 1.0)
    else:                                                                  # "outside": also at or before e[0] and past e[W]
        win = rng.integers(-2, n_win + 2, m)
        frac = np.where(win == -1, np.where(i % 2 == 0, 1.0, frac), frac)  # (window -1 at 64 / 64: start == e[0], no window)
    start = edges[0] + win + frac
    if order in ("sorted", "reversed"):
        start = np.sort(start) if order == "sorted" else np.sort(start)[::-1]
    lat = LAT_POOL[rng.integers(0, LAT_POOL.size, m)]
    return np.stack([start, start + lat], axis=1)


def test_the_dyadic_clocks_are_exact():
    rng = np.random.default_rng(1)
    edges = np.arange(-3.0, 5001.0 - 3.0)
    for order in ORDERS:
        ck = _clock(rng, 500, edges, order)
        assert np.isin(ck[:, 1] - ck[:, 0], LAT_POOL).all(), order
    sp = _clock(rng, 256, edges[:601], "spread")
    win = np.searchsorted(edges[:601], sp[:, 0], side="left") - 1
    assert all(np.unique(win[k:k + 64]).size == 64 for k in range(0, 256, 64))


@pytest.mark.parametrize("n_win", [1, 2, 63, 600, LDS_BOUND, LDS_BOUND + 1, 5000])
def test_start_orders_row_seams_and_window_counts(n_win):
    assert LDS_BOUND == 4095
    rng = np.random.default_rng(1000 + n_win)
    edges = -3.0 + np.arange(n_win + 1, dtype=np.float64)
    clocks = [_clock(rng, m, edges, ORDERS[(k + n_win) % len(ORDERS)]) for k, m in enumerate(ROWS)]
    clocks += [_clock(rng, 700, edges, "random"), _clock(rng, 300, edges, "spread"), _clock(rng, 130, edges, "on_edge")]
    n = len(clocks)
    extra = np.zeros(n, dtype=np.int64)
    extra[11] = 50                                                          # counts above the clock capacity: clamped
    groupings = {"one group": np.zeros(n, dtype=np.int64), "members": np.arange(n) % 4, "singletons": np.arange(n)}
    for g in groupings.values():
        g[13] = -1                                                          # one scenario left out
    for name, grp in groupings.items():
        n_groups = int(grp.max()) + 1
        stored, got = _device(clocks, grp, n_groups, edges, cap_limit=2049, counts_extra=extra)
        assert stored[12].shape[0] == 700 and [s.shape[0] for s in stored[:12]] == ROWS
        cells, cum = _cells(stored, grp, n_groups, edges)
        assert cum[13].max() > 0                                            # (the cumulative counts of the skipped scenario too)
        _compare(got, cells, cum, n_groups, n_win, f"W={n_win} {name}")


def test_counts_above_the_capacity_are_clamped_to_the_stored_rows():
    rng = np.random.default_rng(5)
    edges = np.array([0.0, 1.0, 2.0, 3.0])
    clocks = [_clock(rng, m, edges, "random") for m in (900, 500, 40)]
    stored, got = _device(clocks, [0, 0, 0], 1, edges, cap_limit=500)
    assert [s.shape[0] for s in stored] == [500, 500, 40]
    cells, cum = _cells(stored, [0, 0, 0], 1, edges)
    assert cum[:, -1].tolist() == [500, 500, 40]
    _compare(got, cells, cum, 1, 3, "clamped")


def test_a_subnormal_latency_and_the_order_inside_a_cell():
    """Reversing two members of a cell changes the bits of its mean: the device has to keep the rows in row order, scenario after
    scenario, although the starts are out of order."""
    edges = np.array([-1.0, 1.0, 2.0])
    big = 2.0 ** 53
    a = np.array([[0.75, 0.75 + 1.0], [0.25, 0.25 + big], [0.5, 0.5 + 1.0], [1.5, 1.5 + 0.25]])       # window 0: 1, 2^53, 1 in row order
    b = np.array([[0.0, 5e-324], [1.25, 1.25], [-0.5, -0.5]])                                       # window 0: a subnormal and a zero
    cell = np.array([1.0, big, 1.0, 5e-324, 0.0])
    assert np.array_equal(a[:3, 1] - a[:3, 0], cell[:3])
    assert np.mean(cell) != np.mean(cell[[0, 2, 1, 3, 4]])
    stored, got = _device([a, b], [0, 0], 1, edges)
    cells, cum = _cells(stored, [0, 0], 1, edges)
    assert np.array_equal(cells[0, 0], cell) and np.array_equal(cells[0, 1], [0.25, 0.0])
    _compare(got, cells, cum, 1, 2, "order")
    # 600 rows in one window, their starts reversed: rows 0, 1, 2, ... of the cell are still rows 0, 1, 2, ... of the clock
    rng = np.random.default_rng(3)
    start = 1.0 - np.arange(600) / 1024.0
    ck = np.stack([start, start + rng.lognormal(0.0, 8.0, 600)], axis=1)                           # (magnitudes e^-25 .. e^25)
    lat = ck[:, 1] - ck[:, 0]
    assert np.mean(lat) != np.mean(lat[::-1]) and np.std(lat) != np.std(lat[::-1])
    stored, got = _device([ck], [0], 1, edges)
    cells, cum = _cells(stored, [0], 1, edges)
    assert np.array_equal(cells[0, 0], lat)
    _compare(got, cells, cum, 1, 2, "reversed starts")


def test_cells_of_every_tier_in_one_call():
    """Cells of 8, 512, 513, 8 192 and 8 193 latencies (and an empty one): the wave, workgroup and tiled tiers of both analyzers
    read the layout the arrival kernels made."""
    rng = np.random.default_rng(11)
    sizes = [8, 512, 513, 8192, 0, 8193]
    edges = np.arange(len(sizes) + 1, dtype=np.float64)
    split = [[3, 5, 0], [500, 0, 12], [1, 256, 256], [4000, 4000, 192], [0, 0, 0], [8193 - 4097 - 1, 4097, 1]]
    clocks = []
    for s in range(3):
        win = np.concatenate([np.full(split[w][s], w) for w in range(len(sizes))])
        rng.shuffle(win)
        start = win + rng.integers(1, 65, win.size) / 64.0
        lat = rng.lognormal(-3.0, 0.8, win.size)
        clocks.append(np.stack([start, start + lat], axis=1))
    stored, got = _device(clocks, [0, 0, 0], 1, edges)
    cells, cum = _cells(stored, [0, 0, 0], 1, edges)
    assert [cells[0, w].size if (0, w) in cells else 0 for w in range(len(sizes))] == sizes
    _compare(got, cells, cum, 1, len(sizes), "tiers")
    again = _device(clocks, [0, 0, 0], 1, edges)[1]                        # two identical calls: identical bytes
    for k, v in got.items():
        assert v.tobytes() == again[k].tobytes(), k


def test_sorted_dyadic_starts_with_a_constant_latency_are_finish_windows_shifted():
    rng = np.random.default_rng(21)
    edges = np.arange(0.0, 41.0)
    L = 2.0 ** -3
    clocks = []
    for m in (0, 1, 700, 3000):
        start = np.sort(rng.integers(1, 40 * 64, m) / 64.0)
        clocks.append(np.stack([start, start + L], axis=1))
    grp = [0, 1, 0, 1]
    _, by_arrival = _device(clocks, grp, 2, edges)
    _, by_finish = _device(clocks, grp, 2, edges + L, window_of="finish")
    for k in ("stats", "row_bounds", "count", "quantiles", "within"):
        assert by_arrival[k].tobytes() == by_finish[k].tobytes(), k
    assert by_arrival["stats"][:, :, 0].sum() == 3701


def test_a_decreasing_finish_column_is_fine_by_arrival_and_refused_by_finish():
    from asyncflow_amd.engine import EngineError

    rng = np.random.default_rng(4)
    edges = np.array([0.0, 1.0, 2.0])
    clocks = [_clock(rng, 300, edges, "random") for _ in range(3)]
    assert all((np.diff(ck[:, 1]) < 0).any() for ck in clocks)
    stored, got = _device(clocks, [0, 0, 0], 1, edges)
    cells, cum = _cells(stored, [0, 0, 0], 1, edges)
    _compare(got, cells, cum, 1, 2, "unordered finish")
    with pytest.raises(EngineError, match="not in completion order"):
        _device(clocks, [0, 0, 0], 1, edges, window_of="finish")
    with pytest.raises(EngineError, match="not in completion order"):
        _device(clocks, [0, 0, 0], 1, edges, window_of="finish", calls=("quantiles",))


def test_the_quantiles_entry_needs_windows():
    import torch

    from asyncflow_amd.engine import Engine

    dev = torch.device("cuda", 0)
    clock = torch.zeros((2, 4, 2), dtype=torch.float64, device=dev)
    counts = torch.zeros((2, _abi.CNT_SLOTS), dtype=torch.int32, device=dev)
    cnt = torch.zeros((1, 1), dtype=torch.int32, device=dev)
    eng = Engine(lower(single_server(horizon=50)), 0)
    lib, h = eng._lib, eng._h  # noqa: SLF001
    try:
        out = _abi.AfOutputs(4, C.c_void_p(clock.data_ptr()), 0, None, C.c_void_p(counts.data_ptr()))
        lv = (C.c_double * 1)(0.5)
        edges = (C.c_double * 2)(0.0, 1.0)
        req = _abi.AfQuantiles(2, 1, 0, None, None, 1, lv, 0, None, C.c_void_p(cnt.data_ptr()), None, None, 0.0, 0)
        assert lib.af_engine_summarize_quantiles(h, C.byref(out), C.byref(req)) == _abi.AF_OK
        assert lib.af_engine_summarize_arrival_quantiles(h, C.byref(out), C.byref(req)) == _abi.AF_ERR_INVALID
        assert "need windows" in lib.af_last_error().decode()
        req = _abi.AfQuantiles(2, 1, 1, None, edges, 1, lv, 0, None, C.c_void_p(cnt.data_ptr()), None, None, 0.0, 0)
        assert lib.af_engine_summarize_arrival_quantiles(h, C.byref(out), C.byref(req)) == _abi.AF_OK
    finally:
        eng.close()


def test_one_window_around_everything_is_the_pooled_and_the_finish_analyzer():
    from asyncflow_amd.runner import SimulationRunner

    seeds = 0x5EED0000 + np.arange(64, dtype=np.uint64)
    res = SimulationRunner(simulation_input=lb_two_servers(horizon=60), seeds=seeds).run()
    whole = [-1.0, 61.0]
    for by in (None, np.arange(64) % 5, np.where(np.arange(64) % 7 == 0, -1, np.arange(64) % 3), "scenario"):
        a = res.window_summary(edges=whole, by=by, window_of="arrival")
        f = res.window_summary(edges=whole, by=by)
        assert a["window_of"] == "arrival" and f["window_of"] == "finish"
        assert a["stats"].cpu().numpy().tobytes() == f["stats"].cpu().numpy().tobytes()
        if not isinstance(by, str):
            p = res.pooled_summary(by)
            assert a["stats"].cpu().numpy()[:, 0].tobytes() == p["stats"].cpu().numpy().tobytes()
    with pytest.raises(ValueError, match="no window"):
        res.quantile_summary([0.5], window_of="arrival")
    with pytest.raises(ValueError, match="window_of"):
        res.window_summary(window_of="sent")
    with pytest.raises(ValueError, match="window_of"):
        res.quantile_summary([0.5], window_s=1.0, window_of="sent")


def _numpy_cells(res, ids, n_groups, edges, window_of):
    """Per (group, window) the latencies, by masks on start (arrival) or finish over res[s].rqs_clock, scenario after scenario."""
    col = 0 if window_of == "arrival" else 1
    clocks = [res[s].rqs_clock for s in range(len(res))]
    out = {}
    for g in range(n_groups):
        members = np.nonzero(ids == g)[0]
        for w in range(len(edges) - 1):
            seg = [(ck[:, 1] - ck[:, 0])[(ck[:, col] > edges[w]) & (ck[:, col] <= edges[w + 1])] for ck in (clocks[s] for s in members)]
            out[g, w] = np.concatenate(seg or [np.zeros(0)])
    return out


def _check_summaries(res, by, ids, n_groups, edges, window_of):
    kw = {} if window_of is None else {"window_of": window_of}
    cells = _numpy_cells(res, ids, n_groups, edges, window_of or "finish")
    a = res.window_summary(10.0, by=by, **kw)
    q = res.quantile_summary([0.5, 0.99], thresholds=[0.2], window_s=10.0, by=by, **kw)
    assert a["window_of"] == q["window_of"] == (window_of or "finish") and np.array_equal(a["edges"], edges)
    st, qt, cnt, wt = a["stats"].cpu().numpy(), q["quantiles"].cpu().numpy(), q["count"].cpu().numpy(), q["within"].cpu().numpy()
    for (g, w), lat in cells.items():
        want = _np_stats(lat)
        if lat.size:
            assert np.array_equal(st[g, w].view(np.uint64), want.view(np.uint64)), (window_of, g, w)
            assert np.array_equal(qt[g, w].view(np.uint64), np.quantile(lat, [0.5, 0.99]).view(np.uint64)), (window_of, g, w)
        else:
            assert st[g, w, 0] == 0 and np.isnan(st[g, w, 1:]).all() and np.isnan(qt[g, w]).all()
        assert cnt[g, w] == lat.size and wt[g, w, 0] == np.count_nonzero(lat <= 0.2)
    return st


def test_event_workload_through_the_python_api(tmp_path):
    from asyncflow_amd import expand_grid
    from asyncflow_amd.results import load_summary
    from asyncflow_amd.runner import SimulationRunner

    payload = lb_with_events(horizon=60, scale=0.1)
    seeds = 0xE7E70000 + np.arange(64, dtype=np.uint64)
    res = SimulationRunner(simulation_input=payload, seeds=seeds).run()
    edges = window_edges(10.0, res.plan.total_time)
    by_arrival = _check_summaries(res, None, np.zeros(64, dtype=np.int64), 1, edges, "arrival")
    by_finish = _check_summaries(res, None, np.zeros(64, dtype=np.int64), 1, edges, None)       # without the keyword: as before
    assert (by_arrival[:, :, 0] != by_finish[:, :, 0]).any()
    _check_summaries(res, "scenario", np.arange(64), 64, edges, "arrival")

    users = "rqs_input.avg_active_users.mean"
    grid = expand_grid({users: [40.0, 120.0, 300.0], "topology_graph.edges[*].latency.mean": [0.002, 0.006]},
                       replicas=4, order_by_load=users)
    res = SimulationRunner(simulation_input=payload, **grid.runner_kwargs()).run()
    st = _check_summaries(res, grid, grid.point, 6, edges, "arrival")
    _check_summaries(res, grid, grid.point, 6, edges, None)

    # bands: a numpy group-by of the per-scenario rows of the host definition
    bands = res.window_bands(10.0, by=grid, window_of="arrival")
    assert bands["window_of"] == "arrival"
    per = np.stack([latency_window_stats(res[s].rqs_clock, edges, window_of="arrival") for s in range(len(res))])
    for g in range(6):
        members = np.nonzero(grid.point == g)[0]
        for w in range(len(edges) - 1):
            body = per[members, w][per[members, w, 0] > 0]
            assert bands["n"][g, w] == body.shape[0]
            if body.shape[0]:
                np.testing.assert_allclose(bands["mean"][g, w], body.mean(axis=0), rtol=1e-12)
                np.testing.assert_allclose(bands["q_hi"][g, w], np.quantile(body, 0.95, axis=0), rtol=1e-12)
            if body.shape[0] > 1:
                np.testing.assert_allclose(bands["std"][g, w], body.std(axis=0, ddof=1), rtol=1e-12)
    assert bands["pooled"].tobytes() == st.tobytes()
    qb = res.quantile_bands([0.5, 0.99], thresholds=[0.2], window_s=10.0, by=grid, window_of="arrival")
    perq = [latency_window_quantiles(res[s].rqs_clock, edges, [0.5, 0.99], [0.2], window_of="arrival") for s in range(len(res))]
    for g in range(6):
        members = np.nonzero(grid.point == g)[0]
        for w in range(len(edges) - 1):
            body = np.array([perq[s][1][w] for s in members if perq[s][0][w] > 0])
            assert qb["n"][g, w] == body.shape[0]
            if body.shape[0]:
                np.testing.assert_allclose(qb["mean"][g, w, :2], body.mean(axis=0), rtol=1e-12)
    assert qb["window_of"] == "arrival"

    # the dumps say which windows they hold, in both formats
    for name in ("windows.npz", "windows.parquet"):
        for window_of in ("arrival", "finish"):
            written = res.save_window_summary(str(tmp_path / name), grid, window_s=10.0, window_of=window_of)
            back = load_summary(str(tmp_path / name))
            assert set(back) == set(written) and str(back["window_of"]) == window_of
            for k, v in written.items():
                assert np.array_equal(np.asarray(back[k], dtype=v.dtype), v, equal_nan=v.dtype.kind == "f"), (name, k)
        assert np.array_equal(load_summary(str(tmp_path / name))["window_pooled:p95"], res.window_summary(10.0, by=grid)["stats"].cpu().numpy()[:, :, 4], equal_nan=True)
        written = res.save_window_summary(str(tmp_path / name), grid, window_s=10.0, window_of="arrival")
        assert np.array_equal(written["window_pooled:p95"], st[:, :, 4], equal_nan=True)
    for name in ("quantiles.npz", "quantiles.parquet"):
        written = res.save_quantile_summary(str(tmp_path / name), grid, levels=[0.5, 0.99], thresholds=[0.2], window_s=10.0, window_of="arrival")
        back = load_summary(str(tmp_path / name))
        assert set(back) == set(written) and str(back["window_of"]) == "arrival"
        for k, v in written.items():
            assert np.array_equal(np.asarray(back[k], dtype=v.dtype), v, equal_nan=v.dtype.kind == "f"), (name, k)
        assert str(res.save_quantile_summary(str(tmp_path / name), grid, levels=[0.5], window_s=10.0)["window_of"]) == "finish"
