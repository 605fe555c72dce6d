"""Windowed analyzer on the MI355X (af_engine_summarize_windows): per (group, window by finish time) the eight latency
statistics of the concatenated row segments, bit-equal to numpy's / results.latency_window_stats -- synthetic sorted clocks
cover the seams of numpy's 8 / 128 / 8 192-element blocks, the small-cell and the tiled path in one call, edges on finish
values, the order check; event workloads through the Python API; 1 200 000 small cells within the scratch bound; bands."""

from __future__ import annotations

import numpy as np
import pytest

from asyncflow_amd import _abi
from asyncflow_amd.plan import lower
from asyncflow_amd.results import latency_window_stats, window_edges
from oracle.scenarios import lb_two_servers, lb_with_events, single_server

pytestmark = pytest.mark.gpu

SIZES = [0, 3, 5, 8, 1, 120, 7, 128, 0, 8000, 191, 1, 8192, 64, 63, 1, 12000, 4, 16384, 9, 255, 8191, 2]


def _np_stats(lat: np.ndarray) -> np.ndarray:
    lat = np.ascontiguousarray(lat, dtype=np.float64)
    if lat.size == 0:
        return np.array([0.0] + [np.nan] * 7)
    return np.array([float(lat.size), float(np.mean(lat)), float(np.median(lat)), float(np.std(lat)),
                     float(np.percentile(lat, 95)), float(np.percentile(lat, 99)), float(np.min(lat)), float(np.max(lat))])


def _check(got: np.ndarray, want: np.ndarray, what="") -> None:
    if want[0] > 0:
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (what, got, want, got - want)
    else:
        assert got[0] == 0 and np.isnan(got[1:]).all(), (what, got)


def _windows_synthetic(clocks, group, n_groups, edges, cap_limit=None, bounds=True):
    """Hand-made rqs_clock rows fed straight to af_engine_summarize_windows.  Returns the stored rows per scenario, the
    stats [G, W, 8], the row bounds [n, W + 1] (or None) and the engine's scratch size."""
    import torch

    from asyncflow_amd.engine import Engine

    plan = lower(single_server(horizon=50))
    n = len(clocks)
    cap = cap_limit or max(max((len(x) for x in clocks), default=1), 1)
    clock = np.full((n, cap, 2), np.nan)
    counts = np.zeros((n, _abi.CNT_SLOTS), dtype=np.uint32)
    stored = []
    for i, rows in enumerate(clocks):
        rows = np.asarray(rows, dtype=np.float64).reshape(-1, 2)
        counts[i, _abi.CNT_COMPLETED] = rows.shape[0]
        keep = rows[:cap]
        clock[i, : keep.shape[0]] = keep
        stored.append(keep)
    dev = torch.device("cuda", 0)
    clock_t = torch.as_tensor(clock, device=dev)
    counts_t = torch.as_tensor(counts.view(np.int32), device=dev)
    grp = np.asarray(group, dtype=np.int64)
    grp_t = torch.as_tensor(np.where(grp < 0, _abi.POOL_SKIP, grp).astype(np.uint32).view(np.int32), device=dev)
    n_win = len(edges) - 1
    stats = torch.full((n_groups, n_win, 8), -7.0, dtype=torch.float64, device=dev)
    rb = torch.full((n, n_win + 1), -1, dtype=torch.int32, device=dev) if bounds else None
    eng = Engine(plan, 0)
    try:
        _, scratch = eng.summarize_windows(n, n_groups, edges, clock_ptr=clock_t.data_ptr(), clock_capacity=cap,
                                           counts_ptr=counts_t.data_ptr(), stats_ptr=stats.data_ptr(), group_ptr=grp_t.data_ptr(),
                                           row_bounds_ptr=rb.data_ptr() if rb is not None else 0)
    finally:
        eng.close()
    return stored, stats.cpu().numpy(), (rb.cpu().numpy() if rb is not None else None), scratch


def _want(stored, group, n_groups, edges):
    """numpy on the concatenated segments: [G, W, 8] and the bounds [n, W + 1]."""
    group = np.asarray(group)
    edges = np.asarray(edges, dtype=np.float64)
    r = np.stack([np.searchsorted(rows[:, 1], edges, side="right") for rows in stored])
    out = np.zeros((n_groups, len(edges) - 1, 8))
    for g in range(n_groups):
        members = np.nonzero(group == g)[0]
        for w in range(len(edges) - 1):
            seg = [stored[s][r[s, w]:r[s, w + 1], 1] - stored[s][r[s, w]:r[s, w + 1], 0] for s in members]
            out[g, w] = _np_stats(np.concatenate(seg or [np.zeros(0)]))
    return out, r


def _sorted_clock(rng, per_window, edges, before=0, after=0, on_edge=0):
    """Rows in completion order with per_window[w] finishes inside (edges[w], edges[w + 1]] -- on_edge of them (where the
    window holds that many) exactly ON edges[w + 1] --, `before` rows at or before edges[0] and `after` rows past the last."""
    fin = [np.sort(rng.uniform(edges[0] - 1.0, edges[0], before))]
    if before:
        fin[0][-1] = edges[0]                      # a finish equal to e[0] belongs to no window
    for w, k in enumerate(per_window):
        f = np.sort(rng.uniform(edges[w], edges[w + 1], int(k)))
        f = f[f > edges[w]]
        f = np.concatenate([f, np.full(int(k) - f.size, edges[w + 1])])
        if on_edge and k >= on_edge:
            f[-on_edge:] = edges[w + 1]            # ties on the edge: all of them go left
        fin.append(f)
    fin.append(np.sort(rng.uniform(np.nextafter(edges[-1], np.inf), edges[-1] + 1.0, after)))
    finish = np.concatenate(fin)
    lat = rng.lognormal(-3.0, 0.8, finish.size)
    return np.stack([finish - lat, finish], axis=1)


def test_segment_seams_small_and_tiled_cells_in_one_call():
    rng = np.random.default_rng(17)
    edges = np.array([1.0, 2.0, 2.5, 4.0, 4.0 + 2.0 ** -20, 7.0, 9.0, 30.0])    # 7 windows, one of them 1 us wide
    n, n_win = len(SIZES), len(edges) - 1
    per = np.array([[SIZES[(3 * s + 5 * w) % len(SIZES)] for w in range(n_win)] for s in range(n)])
    per[:, 4] = 0                      # an empty window in every scenario
    per[:, 6] = 0                      # and one past the last finish
    per[:, 4][5] = 3                   # (but for three rows of one scenario inside the 1-us window)
    clocks = [_sorted_clock(rng, per[s], edges, before=s % 4, after=(s * 5) % 7, on_edge=(s % 3)) for s in range(n)]
    # one group: segments of a cell reach and cross 8, 128 and 8 192 elements at the scenarios' seams
    one = np.zeros(n, dtype=np.int64)
    stored, stats, rb, _ = _windows_synthetic(clocks, one, 1, edges)
    want, r = _want(stored, one, 1, edges)
    assert np.array_equal(rb, r)
    sizes = want[0, :, 0]
    assert (sizes > 8192).any() and ((sizes > 0) & (sizes <= 512)).any() and (sizes == 0).any(), sizes
    for w in range(n_win):
        _check(stats[0, w], want[0, w], f"one group, window {w}")
    # interleaved ids, skipped scenarios, an empty group (3): cells of every size, small and tiled in the same call
    grp = np.array([(i * 7) % 12 for i in range(n)])
    grp[grp == 3] = 4
    grp[[2, 9]] = -1
    stored, stats, rb, _ = _windows_synthetic(clocks, grp, 12, edges)
    want, r = _want(stored, grp, 12, edges)
    assert np.array_equal(rb, r)                                       # (also of the skipped scenarios)
    sizes = want[:, :, 0]
    assert (sizes > 8192).sum() >= 3 and ((sizes > 512) & (sizes <= 8192)).sum() >= 3 and ((sizes > 0) & (sizes <= 512)).sum() >= 3, sizes
    for g in range(12):
        for w in range(n_win):
            _check(stats[g, w], want[g, w], f"group {g}, window {w}")
    assert (stats[3, :, 0] == 0).all()
    # every scenario its own group: the host accessor's definition, window by window
    ids = np.arange(n)
    stored, stats, _, _ = _windows_synthetic(clocks, ids, n, edges, bounds=False)
    for s in range(n):
        want_s = latency_window_stats(stored[s], edges)
        for w in range(n_win):
            _check(stats[s, w], want_s[w], f"scenario {s}, window {w}")


def test_cell_sizes_around_the_block_boundaries_and_odd_values():
    rng = np.random.default_rng(23)
    # one scenario per size, one window around all of it and one empty on each side: the small path's every shape
    sizes = [1, 2, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 511, 512, 513, 1000, 4095, 4096, 8191, 8192, 8193, 20000]
    edges = np.array([-5.0, 0.0, 10.0, 20.0])
    clocks = [_sorted_clock(rng, [0, k, 0], edges) for k in sizes]
    stored, stats, rb, _ = _windows_synthetic(clocks, np.arange(len(sizes)), len(sizes), edges)
    want, r = _want(stored, np.arange(len(sizes)), len(sizes), edges)
    assert np.array_equal(rb, r) and want[:, 1, 0].tolist() == [float(k) for k in sizes]
    for s in range(len(sizes)):
        for w in range(3):
            _check(stats[s, w], want[s, w], f"size {sizes[s]}, window {w}")
    # ties, exact zeros and the whole exponent range as latencies, in cells of 600 .. 8 000 (radix select in LDS, all levels)
    vals = np.concatenate([np.zeros(5000), np.full(3000, 0.125), 2.0 ** rng.integers(-1074, 500, 4000).astype(np.float64),
                           rng.exponential(1.0, 3000), [5e-324, 2.0 ** -1022, 1e150]])
    rng.shuffle(vals)
    parts = np.array_split(np.arange(vals.size), 13)
    clocks = []
    for p in parts:
        lat = np.sort(vals[p])                       # finish = latency, start = 0: exact, and in completion order
        clocks.append(np.stack([np.zeros(lat.size), lat], axis=1))
    edges2 = np.array([-1.0, 0.0, 2.0 ** -1000, 0.125, 1.0, 1e200])
    grp = np.arange(13) % 3
    stored, stats, rb, _ = _windows_synthetic(clocks, grp, 3, edges2)
    want, r = _want(stored, grp, 3, edges2)
    assert np.array_equal(rb, r)
    for g in range(3):
        for w in range(5):
            _check(stats[g, w], want[g, w], f"odd values, group {g}, window {w}")


def test_candidates_that_part_in_the_last_key_bits_and_a_constant_cell():
    """0.05 + k ulp, k < 4096: every key shares its upper 52 bits, so the select takes five digit levels and stops at
    shift 2 with a handful of distinct candidates per rank -- no tie runs it down to shift 0, as the constant cell beside it
    does.  600 latencies: one workgroup's cell (af_win_small); 9 000: the tiled passes."""
    rng = np.random.default_rng(31)
    edges = np.array([0.0, 1.0])
    sizes = (600, 9000)
    for name, make in (("last bits", lambda n: 0.05 + rng.integers(0, 4096, n) * np.spacing(0.05)), ("constant", lambda n: np.full(n, 0.0625))):
        clocks = []
        for n in sizes:
            lat = np.sort(make(n))                     # finish = latency, start = 0: exact, and in completion order
            clocks.append(np.stack([np.zeros(n), lat], axis=1))
        stored, stats, _, _ = _windows_synthetic(clocks, np.arange(len(sizes)), len(sizes), edges, bounds=False)
        for s, n in enumerate(sizes):
            lat = stored[s][:, 1] - stored[s][:, 0]
            assert lat.size == n and (name == "constant" or np.unique(lat).size > 400)
            _check(stats[s, 0], _np_stats(lat), f"{name}, {n} latencies")


def test_counts_above_the_clock_capacity_and_more_windows_than_fit_the_lds():
    rng = np.random.default_rng(9)
    edges = np.array([0.0, 10.0, 20.0, 30.0])
    clocks = [_sorted_clock(rng, [400, 300, 300], edges), _sorted_clock(rng, [100, 350, 250], edges), _sorted_clock(rng, [20, 20, 10], edges)]
    stored, stats, rb, _ = _windows_synthetic(clocks, [0, 0, 0], 1, edges, cap_limit=500)
    assert [s.shape[0] for s in stored] == [500, 500, 50]
    want, r = _want(stored, [0, 0, 0], 1, edges)
    assert np.array_equal(rb, r) and r[:, -1].tolist() == [500, 500, 50]
    for w in range(3):
        _check(stats[0, w], want[0, w], f"window {w}")
    # 5 000 windows (the compaction reads bounds and destinations from global memory), two groups
    edges = np.linspace(0.0, 50.0, 5001)
    clocks = [_sorted_clock(rng, rng.integers(0, 4, 5000), edges, before=2, after=3) for _ in range(6)]
    grp = [0, 1, 0, -1, 1, 0]
    stored, stats, rb, _ = _windows_synthetic(clocks, grp, 2, edges)
    want, r = _want(stored, grp, 2, edges)
    assert np.array_equal(rb, r)
    bad = [(g, w) for g in range(2) for w in range(5000)
           if not (np.array_equal(stats[g, w].view(np.uint64), want[g, w].view(np.uint64)) if want[g, w, 0] > 0
                   else (stats[g, w, 0] == 0 and np.isnan(stats[g, w, 1:]).all()))]
    assert not bad, bad[:10]


def test_an_inversion_is_an_error_naming_the_scenario():
    """An error code from a finished call, checked once: the kernels read only rows inside the buffers whatever their order."""
    from asyncflow_amd.engine import EngineError

    rng = np.random.default_rng(4)
    edges = np.array([0.0, 10.0, 20.0])
    clocks = [_sorted_clock(rng, [700, 900], edges) for _ in range(8)]
    clocks[5][1203, 1], clocks[5][1204, 1] = clocks[5][1204, 1], clocks[5][1203, 1] - 1e-9    # one row finishes before its predecessor
    assert (np.diff(clocks[5][:, 1]) < 0).sum() == 1
    with pytest.raises(EngineError, match=r"scenario 5 is not in completion order"):
        _windows_synthetic(clocks, np.zeros(8, dtype=np.int64), 1, edges)
    # the same inversion in a scenario that is left out: fine
    grp = np.zeros(8, dtype=np.int64)
    grp[5] = -1
    stored, stats, _, _ = _windows_synthetic(clocks, grp, 1, edges)
    want, _ = _want([s if i != 5 else s[:0] for i, s in enumerate(stored)], grp, 1, edges)
    for w in range(2):
        _check(stats[0, w], want[0, w], f"window {w}")


def test_device_argument_checks():
    from asyncflow_amd.engine import EngineError

    rng = np.random.default_rng(1)
    clocks = [_sorted_clock(rng, [5], [0.0, 1.0]) for _ in range(3)]
    for edges, what in (([0.0, 2.0, 1.0], "strictly increasing"), ([0.0, 1.0, 1.0], "strictly increasing"), ([0.0, float("inf")], "not finite")):
        with pytest.raises(EngineError, match=what):
            _windows_synthetic(clocks, [0, 0, 0], 1, edges)
    with pytest.raises(EngineError, match="group id out of range"):
        _windows_synthetic(clocks, [0, 2, 0], 2, [0.0, 1.0])


def test_one_window_equals_the_pooled_and_the_per_scenario_analyzers():
    from asyncflow_amd.runner import SimulationRunner

    seeds = 0x5EED0000 + np.arange(64, dtype=np.uint64)
    res = SimulationRunner(simulation_input=lb_two_servers(horizon=60), seeds=seeds).run()
    whole = [-1.0, 61.0]
    for by in (None, np.arange(64) % 5, np.where(np.arange(64) % 7 == 0, -1, np.arange(64) % 3)):
        a = res.window_summary(edges=whole, by=by)
        p = res.pooled_summary(by)
        assert a["stats"].shape == (p["stats"].shape[0], 1, 8)
        assert np.array_equal(a["stats"].cpu().numpy()[:, 0].view(np.uint64), p["stats"].cpu().numpy().view(np.uint64))
        assert a["replicas"].tolist() == p["replicas"].tolist()
    per = res.summary(rps=False)["stats"].cpu().numpy()
    a = res.window_summary(edges=whole, by="scenario", row_bounds=True)
    assert np.array_equal(a["stats"].cpu().numpy()[:, 0].view(np.uint64), per.view(np.uint64))
    assert np.array_equal(a["row_bounds"].cpu().numpy()[:, 1], np.minimum(res.counts[:, _abi.CNT_COMPLETED], res._clock_t.shape[1]))  # noqa: SLF001
    with pytest.raises(ValueError, match="strictly increasing"):
        res.window_summary(edges=[0.0, 0.0])
    with pytest.raises(ValueError, match="by must be"):
        res.window_summary(by="point")
    res2 = SimulationRunner(simulation_input=lb_two_servers(horizon=10), seeds=seeds[:4], collect_clock=False).run()
    with pytest.raises(RuntimeError, match="kept no rqs_clock"):
        res2.window_summary()
    with pytest.raises(RuntimeError, match="kept no rqs_clock"):
        res2.window_bands()


def _numpy_cells(res, ids, n_groups, edges):
    out = np.zeros((n_groups, len(edges) - 1, 8))
    clocks = [res[s].rqs_clock for s in range(len(res))]
    for ck in clocks:
        assert (np.diff(ck[:, 1]) >= 0).all()
    r = [np.searchsorted(ck[:, 1], edges, side="right") for ck in clocks]
    for g in range(n_groups):
        members = np.nonzero(ids == g)[0]
        for w in range(len(edges) - 1):
            seg = [clocks[s][r[s][w]:r[s][w + 1], 1] - clocks[s][r[s][w]:r[s][w + 1], 0] for s in members]
            out[g, w] = _np_stats(np.concatenate(seg or [np.zeros(0)]))
    return out


def test_event_workload_through_the_python_api(tmp_path):
    from statistics import NormalDist

    from asyncflow_amd import expand_grid
    from asyncflow_amd.results import load_summary
    from asyncflow_amd.runner import SimulationRunner

    payload = lb_with_events(horizon=60, scale=0.1)       # all five events inside the horizon
    # ---- 64 seeds, one group and singletons
    seeds = 0xE7E70000 + np.arange(64, dtype=np.uint64)
    res = SimulationRunner(simulation_input=payload, seeds=seeds, summary=True).run()
    cached = {k: (v.clone() if hasattr(v, "clone") else v) for k, v in res.summary().items()}
    rps = cached["rps"].cpu().numpy().astype(np.float64)
    edges = window_edges(5.0, res.plan.total_time)
    assert edges.tolist() == [5.0 * k for k in range(13)]
    for by, ids, g in ((None, np.zeros(64, dtype=np.int64), 1), ("scenario", np.arange(64), 64), (np.arange(64) % 6, np.arange(64) % 6, 6)):
        a = res.window_summary(5.0, by=by)
        b = res.window_summary(5.0, by=by)
        st = a["stats"].cpu().numpy()
        assert st.shape == (g, 12, 8) and np.array_equal(a["edges"], edges)
        assert np.array_equal(st.view(np.uint64), b["stats"].cpu().numpy().view(np.uint64))          # two calls identical
        want = _numpy_cells(res, ids, g, edges)
        for gi in range(g):
            for w in range(12):
                _check(st[gi, w], want[gi, w], f"by={by!r} group {gi} window {w}")
            # a window's total / 5 = the 1-s RPS of the group's scenarios summed in fives
            assert np.array_equal(st[gi, :, 0], rps[ids == gi].sum(axis=0).reshape(12, 5).sum(axis=1))
    after = res.summary()
    for k in ("stats", "rps"):
        assert np.array_equal(after[k].cpu().numpy().view(np.uint8), cached[k].cpu().numpy().view(np.uint8)), k

    # ---- a 3 x 2 grid with 4 replicas: by=Sweep, bands over the replicas, the on-disk summary
    users = "rqs_input.avg_active_users.mean"
    grid = expand_grid({users: [40.0, 120.0, 300.0], "topology_graph.edges[*].latency.mean": [0.002, 0.006]},
                       replicas=4, order_by_load=users)
    res = SimulationRunner(simulation_input=payload, summary=True, **grid.runner_kwargs()).run()
    cached = {k: (v.clone() if hasattr(v, "clone") else v) for k, v in res.summary().items()}
    rps = cached["rps"].cpu().numpy().astype(np.float64)
    a = res.window_summary(5.0, by=grid)
    st = a["stats"].cpu().numpy()
    assert st.shape == (6, 12, 8) and a["replicas"].tolist() == [4] * 6
    assert np.array_equal(st.view(np.uint64), res.window_summary(5.0, by=grid)["stats"].cpu().numpy().view(np.uint64))
    want = _numpy_cells(res, grid.point, 6, edges)
    for g in range(6):
        for w in range(12):
            _check(st[g, w], want[g, w], f"point {g} window {w}")
        assert np.array_equal(st[g, :, 0], rps[grid.point == g].sum(axis=0).reshape(12, 5).sum(axis=1))
    after = res.summary()
    for k in ("stats", "rps"):
        assert np.array_equal(after[k].cpu().numpy().view(np.uint8), cached[k].cpu().numpy().view(np.uint8)), k

    # bands: the last window lies past the horizon (no replica has a completion there: NaN)
    edges_b = np.concatenate([edges, [70.0]])
    bands = res.window_bands(edges=edges_b, by=grid, level=0.9, q=(0.1, 0.75))
    per = np.stack([latency_window_stats(res[s].rqs_clock, edges_b) for s in range(len(res))])        # [n, 13, 8]
    z = NormalDist().inv_cdf(0.95)
    for g in range(6):
        members = np.nonzero(grid.point == g)[0]
        for w in range(13):
            body = per[members, w][per[members, w, 0] > 0]
            assert bands["n"][g, w] == body.shape[0]
            if body.shape[0] == 0:
                for k in ("mean", "std", "ci_halfwidth", "q_lo", "q_hi"):
                    assert np.isnan(bands[k][g, w]).all(), (k, g, w)
                continue
            sd = body.std(axis=0, ddof=1)
            np.testing.assert_allclose(bands["mean"][g, w], body.mean(axis=0), rtol=1e-12)
            np.testing.assert_allclose(bands["std"][g, w], sd, rtol=1e-12)
            np.testing.assert_allclose(bands["ci_halfwidth"][g, w], z * sd / np.sqrt(body.shape[0]), rtol=1e-12)
            np.testing.assert_allclose(bands["q_lo"][g, w], np.quantile(body, 0.1, axis=0), rtol=1e-12)
            np.testing.assert_allclose(bands["q_hi"][g, w], np.quantile(body, 0.75, axis=0), rtol=1e-12)
    assert (bands["n"][:, 12] == 0).all() and (bands["n"][:, :12] == 4).all()
    assert np.array_equal(bands["pooled"][:, :12].view(np.uint64), st.view(np.uint64))
    assert (bands["pooled"][:, 12, 0] == 0).all() and np.isnan(bands["pooled"][:, 12, 1:]).all()

    # one row per point, both formats
    for name in ("windows.npz", "windows.parquet"):
        written = res.save_window_summary(str(tmp_path / name), grid, window_s=5.0)
        back = load_summary(str(tmp_path / name))
        assert set(back) == set(written)
        for k, v in written.items():
            assert np.array_equal(np.asarray(back[k], dtype=v.dtype), v, equal_nan=v.dtype.kind == "f"), (name, k)
        for k, v in grid.point_columns().items():
            assert np.array_equal(back[f"param:{k}"], v)
        assert np.array_equal(back["window_pooled:p95"], st[:, :, 4], equal_nan=True)
        assert back["window_q95:median"].shape == (6, 12) and np.array_equal(back["window_edges"], edges)
        assert back["replicas"].tolist() == [4] * 6


def test_many_small_cells_stay_within_the_scratch_bound():
    """2 000 replicas x 600 windows of 1 s, every replica its own group: 1 200 000 cells of ~130 latencies.  Scratch bound:
    8 B per windowed latency + 8 B per (scenario, edge) + 256 B per cell of at most 8 192 latencies + the pooled analyzer's
    per-group scratch (af_pooled.hpp: < 60 000 B + 8 B per 8 192 latencies + 48 B per 131 072) for larger cells only -- the
    pooled analyzer's ~56 KB for EVERY cell would be 67 GB here."""
    from asyncflow_amd.runner import SimulationRunner

    n = 2000
    seeds = 0xC0FFEE00 + np.arange(n, dtype=np.uint64)
    res = SimulationRunner(simulation_input=lb_two_servers(horizon=600), seeds=seeds).run()
    a = res.window_summary(1.0, by="scenario")
    st = a["stats"]
    assert tuple(st.shape) == (n, 600, 8)
    sizes = st[:, :, 0].cpu().numpy()
    stored = np.minimum(res.counts[:, _abi.CNT_COMPLETED], res._clock_t.shape[1])  # noqa: SLF001
    assert sizes.sum() <= stored.sum() and sizes.sum() >= 0.99 * stored.sum()
    large = sizes > 8192
    bound = (8 * sizes.sum() + 8 * n * 601 + 256 * np.count_nonzero(~large)
             + (60_000 * np.count_nonzero(large) + (8 / 8192 + 48 / 131072) * sizes[large].sum()))
    print(f"scratch_bytes {a['scratch_bytes']} bound {int(bound)} windowed latencies {int(sizes.sum())} window_ms {a['window_ms']:.2f}")
    assert not large.any()
    assert 0 < a["scratch_bytes"] <= bound
    edges = a["edges"]
    rng = np.random.default_rng(77)
    host = st.cpu().numpy()
    for s, w in zip(rng.integers(0, n, 64), rng.integers(0, 600, 64)):
        ck = res[int(s)].rqs_clock
        lat = (ck[:, 1] - ck[:, 0])[(ck[:, 1] > edges[w]) & (ck[:, 1] <= edges[w + 1])]
        _check(host[s, w], _np_stats(lat), f"scenario {s} window {w}")
