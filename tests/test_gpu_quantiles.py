"""Quantile analyzer (af_engine_summarize_quantiles) on the device: EVERY cell of every call against np.quantile (uint64 view)
and np.count_nonzero(lat <= threshold) on the concatenated latencies -- all three size tiers and their seams, inputs that are
hard for a radix select, the cross-checks against the windowed / pooled / per-scenario analyzers on the same buffers,
independence from what else a call holds, every refusal, the scratch bound, and the Python API on simulated batches."""

from __future__ import annotations

import numpy as np
import pytest

from asyncflow_amd import _abi
from asyncflow_amd.plan import lower
from asyncflow_amd.results import LATENCY_KEYS, latency_quantiles, latency_window_quantiles, window_edges
from oracle.scenarios import lb_two_servers, lb_with_events, single_server

pytestmark = pytest.mark.gpu

LEVELS9 = [0.0, 1.0, 0.5, 0.95, 0.99, 0.999, 1.0 / 3.0, 0.5, 0.9999]          # 0, 1 and a duplicate among them
SENTINEL_Q, SENTINEL_U = -7.0, 0x7E7E7E7E


def _quantiles_synthetic(clocks, group, n_groups, edges, levels, thresholds=None, *, outputs=("count", "quantiles", "within"),
                         keep=None, counts_override=None, cap_override=None):
    """Hand-made rqs_clock rows fed straight to af_engine_summarize_quantiles (edges None: whole-run mode).  Returns the stored
    rows per scenario, count [G, W], quantiles [G, W, Q], within [G, W, T] (None where not asked for) and the engine's scratch
    size.  `keep` (a dict) receives the output buffers as they are after the call, also when the call raises."""
    import torch

    from asyncflow_amd.engine import Engine

    plan = lower(single_server(horizon=50))
    n = len(clocks)
    cap = max(max((len(x) for x in clocks), default=1), 1)
    clock = np.full((n, cap, 2), np.nan)
    counts = np.zeros((n, _abi.CNT_SLOTS), dtype=np.uint32)
    stored = []
    for i, rows in enumerate(clocks):
        rows = np.asarray(rows, dtype=np.float64).reshape(-1, 2)
        counts[i, _abi.CNT_COMPLETED] = rows.shape[0]
        clock[i, : rows.shape[0]] = rows
        stored.append(rows)
    if counts_override is not None:
        counts[:, _abi.CNT_COMPLETED] = counts_override
    dev = torch.device("cuda", 0)
    clock_t = torch.as_tensor(clock, device=dev)
    counts_t = torch.as_tensor(counts.view(np.int32), device=dev)
    grp = np.asarray(group, dtype=np.int64)
    grp_t = torch.as_tensor(np.where(grp < 0, _abi.POOL_SKIP, grp).astype(np.uint32).view(np.int32), device=dev)
    n_win = 1 if edges is None else max(len(edges) - 1, 1)
    n_lev, n_thr = len(levels), 0 if thresholds is None else len(thresholds)
    shape = (n_groups, n_win) if n_groups * n_win < 1 << 26 else (1, 1)      # (a request that must be refused for its size: nothing is written)
    cnt = torch.full(shape, SENTINEL_U, dtype=torch.int32, device=dev)
    qt = torch.full((*shape, n_lev), SENTINEL_Q, dtype=torch.float64, device=dev)
    wt = torch.full((*shape, n_thr), SENTINEL_U, dtype=torch.int32, device=dev)

    def grab():
        return {"count": cnt.cpu().numpy().view(np.uint32), "quantiles": qt.cpu().numpy(), "within": wt.cpu().numpy().view(np.uint32)}

    eng = Engine(plan, 0)
    try:
        _, scratch = eng.summarize_quantiles(
            n, n_groups, levels, edges=edges, thresholds=thresholds, clock_ptr=clock_t.data_ptr(),
            clock_capacity=cap_override or cap, counts_ptr=counts_t.data_ptr(),
            count_ptr=cnt.data_ptr() if "count" in outputs else 0, quantiles_ptr=qt.data_ptr() if "quantiles" in outputs and n_lev else 0,
            within_ptr=wt.data_ptr() if "within" in outputs and n_thr else 0, group_ptr=grp_t.data_ptr())
    finally:
        if keep is not None:
            torch.cuda.synchronize(dev)
            keep.update(grab())
        eng.close()
    got = grab()
    return stored, got["count"], got["quantiles"], got["within"], scratch


def _cells(stored, group, n_groups, edges):
    """The latencies of every cell: {(g, w): f64 array}, by masks on finish (edges None: all rows)."""
    group = np.asarray(group)
    n_win = 1 if edges is None else len(edges) - 1
    out = {}
    for g in range(n_groups):
        members = np.nonzero(group == g)[0]
        for w in range(n_win):
            seg = []
            for s in members:
                st, fin = stored[s][:, 0], stored[s][:, 1]
                m = np.ones(fin.shape, dtype=bool) if edges is None else (fin > edges[w]) & (fin <= edges[w + 1])
                seg.append((fin - st)[m])
            out[g, w] = np.concatenate(seg or [np.zeros(0)])
    return out


def _compare(cells, count, quant, within, levels, thresholds, what=""):
    """EVERY cell: count and within exactly, the quantiles bit for bit against np.quantile."""
    levels = np.asarray(levels, dtype=np.float64)
    thresholds = np.zeros(0) if thresholds is None else np.asarray(thresholds, dtype=np.float64)
    seen = 0
    for (g, w), lat in cells.items():
        seen += 1
        assert count[g, w] == lat.size, (what, g, w, count[g, w], lat.size)
        if lat.size == 0:
            assert np.isnan(quant[g, w]).all() and (within[g, w] == 0).all(), (what, g, w, quant[g, w], within[g, w])
            continue
        if levels.size:
            want = np.quantile(lat, levels)
            assert np.array_equal(quant[g, w].view(np.uint64), want.view(np.uint64)), (what, g, w, lat.size, quant[g, w], want, quant[g, w] - want)
        for j, th in enumerate(thresholds):
            assert within[g, w, j] == np.count_nonzero(lat <= th), (what, g, w, j, th, within[g, w, j], np.count_nonzero(lat <= th))
    assert seen == count.size


def _sorted_clock(rng, per_window, edges, on_edge=0):
    """Rows in completion order with per_window[w] finishes inside (edges[w], edges[w + 1]], on_edge of them ON edges[w + 1]."""
    fin = []
    for w, k in enumerate(per_window):
        f = np.sort(rng.uniform(edges[w], edges[w + 1], int(k)))
        f = f[f > edges[w]]
        f = np.concatenate([f, np.full(int(k) - f.size, edges[w + 1])])
        if on_edge and k >= on_edge:
            f[-on_edge:] = edges[w + 1]
        fin.append(f)
    finish = np.concatenate(fin) if fin else np.zeros(0)
    lat = rng.lognormal(-3.0, 0.8, finish.size)
    return np.stack([finish - lat, finish], axis=1)


def _rows_of(lat):
    """Rows whose latency is EXACTLY lat[i] (start 0), in the order given."""
    lat = np.asarray(lat, dtype=np.float64)
    return np.stack([np.zeros_like(lat), lat], axis=1)


SIZES = [0, 1, 2, 511, 512, 513, 8191, 8192, 8193, 16384]
BIG_MEMBERS, BIG_EACH = 8, 400_000          # one cell of 3.2 million latencies: eight scenarios of one group


def _sizes_batch(rng, edges):
    n_single = len(SIZES)
    clocks = [_sorted_clock(rng, [SIZES[s], SIZES[::-1][s]], edges) for s in range(n_single)]
    clocks += [_sorted_clock(rng, [BIG_EACH, 300], edges) for _ in range(BIG_MEMBERS)]
    grp = np.concatenate([np.arange(n_single), np.full(BIG_MEMBERS, n_single)])
    return clocks, grp, n_single + 1


def test_every_tier_and_every_seam_in_one_call():
    rng = np.random.default_rng(23)
    edges = np.array([0.0, 50.0, 90.0])
    clocks, grp, G = _sizes_batch(rng, edges)
    big = np.concatenate([c[:BIG_EACH, 1] - c[:BIG_EACH, 0] for c in clocks[len(SIZES):]])
    thresholds = [0.05, float(np.sort(big)[big.size // 3]), float("inf"), 0.0]      # one exactly ON a latency of the big cell
    assert np.count_nonzero(big == thresholds[1]) >= 1
    stored, count, quant, within, _ = _quantiles_synthetic(clocks, grp, G, edges, LEVELS9, thresholds)
    cells = _cells(stored, grp, G, edges)
    assert sorted(c.size for c in cells.values())[-1] == BIG_MEMBERS * BIG_EACH
    assert {c.size for c in cells.values()} >= set(SIZES) | {BIG_MEMBERS * 300}
    _compare(cells, count, quant, within, LEVELS9, thresholds, "windowed")
    assert (within[:, :, 2] == count).all()
    # the same batch over the whole run: one cell per group
    stored, count, quant, within, _ = _quantiles_synthetic(clocks, grp, G, None, LEVELS9, thresholds)
    _compare(_cells(stored, grp, G, None), count, quant, within, LEVELS9, thresholds, "whole run")
    # 64 levels and 64 thresholds, the caps; only levels; only thresholds; outputs left out
    lv64 = np.concatenate([[0.0, 1.0], rng.uniform(0.0, 1.0, 62)])
    th64 = np.concatenate([[np.inf, -np.inf], rng.lognormal(-3.0, 1.0, 62)])
    stored, count, quant, within, _ = _quantiles_synthetic(clocks, grp, G, edges, lv64, th64)
    _compare(cells, count, quant, within, lv64, th64, "64 + 64")
    _, c1, q1, w1, _ = _quantiles_synthetic(clocks, grp, G, edges, LEVELS9, None)
    _compare(cells, c1, q1, np.zeros(c1.shape + (0,), dtype=np.uint32), LEVELS9, None, "levels only")
    _, c2, q2, w2, _ = _quantiles_synthetic(clocks, grp, G, edges, [], thresholds)
    _compare(cells, c2, q2, w2, [], thresholds, "thresholds only")
    _, c3, q3, w3, _ = _quantiles_synthetic(clocks, grp, G, edges, LEVELS9, thresholds, outputs=("quantiles",))
    assert (c3 == SENTINEL_U).all() and (w3 == SENTINEL_U).all()
    assert np.array_equal(q3.view(np.uint64), q1.view(np.uint64))


HARD_SIZES = (300, 5000, 200_000)       # a cell of every tier


def _hard_inputs(rng, n):
    base = 0.123456789
    ulp = np.spacing(base)
    return {
        "all equal": np.full(n, 0.25),
        "half equal": np.where(rng.random(n) < 0.5, 0.0625, rng.lognormal(-3.0, 1.0, n)),
        "base + k ulp": base + rng.integers(0, 4096, n) * ulp,          # the candidates separate in the key's last digits only
        "two values one ulp apart": np.where(rng.random(n) < 0.5, base, base + ulp),
        "40 binades": np.ldexp(rng.uniform(1.0, 2.0, n), rng.integers(-30, 10, n)),
        "zeros and a tail": np.where(rng.random(n) < 0.9, 0.0, rng.exponential(1.0, n)),
    }


def test_inputs_that_are_hard_for_the_select():
    rng = np.random.default_rng(5)
    names = list(_hard_inputs(rng, 4))
    lats = [(_hard_inputs(rng, n)[name]) for n in HARD_SIZES for name in names]
    thresholds = [0.25, 0.0625, 0.123456789, float("inf"), 0.0]
    G = len(lats)
    # whole-run mode: the rows in the order drawn
    clocks = [_rows_of(x) for x in lats]
    for x, ck in zip(lats, clocks):
        assert np.array_equal(ck[:, 1] - ck[:, 0], x)
    stored, count, quant, within, _ = _quantiles_synthetic(clocks, np.arange(G), G, None, LEVELS9, thresholds)
    _compare(_cells(stored, np.arange(G), G, None), count, quant, within, LEVELS9, thresholds, "hard, whole run")
    # windowed mode wants completion order: the same values ascending, one window around them all; pooled in threes too
    clocks = [_rows_of(np.sort(x)) for x in lats]
    edges = [-1.0, 1.0e6]
    stored, c2, q2, w2, _ = _quantiles_synthetic(clocks, np.arange(G), G, edges, LEVELS9, thresholds)
    assert np.array_equal(q2.view(np.uint64), quant.view(np.uint64)) and np.array_equal(c2, count) and np.array_equal(w2, within)
    grp = np.arange(G) % len(names)             # a group = one kind of input at all three sizes
    stored, count, quant, within, _ = _quantiles_synthetic(clocks, grp, len(names), edges, LEVELS9, thresholds)
    _compare(_cells(stored, grp, len(names), edges), count, quant, within, LEVELS9, thresholds, "hard, pooled")


def test_levels_equal_the_columns_of_the_existing_analyzers_on_the_same_buffers():
    from asyncflow_amd.runner import SimulationRunner

    seeds = 0x5EED0000 + np.arange(64, dtype=np.uint64)
    res = SimulationRunner(simulation_input=lb_two_servers(horizon=60), seeds=seeds).run()
    lv = [0.95, 0.99, 0.0, 1.0]
    cols = [LATENCY_KEYS.index(k) for k in ("p95", "p99", "min", "max")]
    for by in (None, np.arange(64) % 5, np.where(np.arange(64) % 7 == 0, -1, np.arange(64) % 3), "scenario"):
        # windows: af_engine_summarize_windows
        for window_s in (5.0, 60.0):
            a = res.window_summary(window_s, by=by)["stats"].cpu().numpy()
            q = res.quantile_summary(lv, window_s=window_s, by=by)
            assert np.array_equal(q["count"].cpu().numpy(), a[:, :, 0].astype(np.int64))
            assert np.array_equal(q["quantiles"].cpu().numpy().view(np.uint64), a[:, :, cols].view(np.uint64)), (by, window_s)
        # the whole run: af_engine_summarize_pooled (by="scenario": af_engine_summarize)
        p = res.summary(rps=False)["stats"].cpu().numpy() if isinstance(by, str) else res.pooled_summary(by)["stats"].cpu().numpy()
        q = res.quantile_summary(lv, by=by)
        assert q["edges"] is None and tuple(q["quantiles"].shape) == (p.shape[0], 1, 4)
        assert np.array_equal(q["count"].cpu().numpy()[:, 0], p[:, 0].astype(np.int64))
        assert np.array_equal(q["quantiles"].cpu().numpy()[:, 0].view(np.uint64), p[:, cols].view(np.uint64)), by
    per = res.summary(rps=False)["stats"].cpu().numpy()
    q = res.quantile_summary([0.95, 0.99], by="scenario")["quantiles"].cpu().numpy()[:, 0]
    assert np.array_equal(q.view(np.uint64), per[:, [4, 5]].view(np.uint64))


def test_a_cell_does_not_depend_on_what_else_the_call_holds():
    rng = np.random.default_rng(31)
    edges = np.array([0.0, 10.0, 20.0, 30.0])
    sizes = [[3, 700, 9000], [520, 8192, 0], [20_000, 1, 513], [100, 100, 100], [8193, 300, 12_000], [60_000, 5, 2]]
    clocks = [_sorted_clock(rng, s, edges, on_edge=1) for s in sizes]
    thr = [0.04, 0.2]
    grp = np.array([0, 0, 1, 1, 2, 2])
    _, c0, q0, w0, _ = _quantiles_synthetic(clocks, grp, 3, edges, LEVELS9, thr)
    _, c1, q1, w1, _ = _quantiles_synthetic(clocks, grp, 3, edges, LEVELS9, thr)
    assert np.array_equal(q0.view(np.uint64), q1.view(np.uint64)) and np.array_equal(c0, c1) and np.array_equal(w0, w1)       # two calls
    sub = [5, 0, 3]                                                                                                         # a subset, reordered
    _, c2, q2, w2, _ = _quantiles_synthetic(clocks, grp, 3, edges, [LEVELS9[i] for i in sub], thr[::-1])
    assert np.array_equal(q2.view(np.uint64), q0[:, :, sub].view(np.uint64)) and np.array_equal(w2, w0[:, :, ::-1]) and np.array_equal(c2, c0)
    perm = rng.permutation(len(LEVELS9))
    _, _, q3, _, _ = _quantiles_synthetic(clocks, grp, 3, edges, [LEVELS9[i] for i in perm], thr)
    assert np.array_equal(q3.view(np.uint64), q0[:, :, perm].view(np.uint64))
    # group 0 as it was; the other scenarios grouped differently, one of them left out; group 0 under another id
    grp2 = np.array([2, 2, 0, 1, 1, -1])
    _, c4, q4, w4, _ = _quantiles_synthetic(clocks, grp2, 3, edges, LEVELS9, thr)
    assert np.array_equal(q4[2].view(np.uint64), q0[0].view(np.uint64)) and np.array_equal(c4[2], c0[0]) and np.array_equal(w4[2], w0[0])
    # one scenario of group 0 alone in a call of one window less: the windows it shares
    _, c5, q5, w5, _ = _quantiles_synthetic(clocks[:2], [0, 0], 1, edges[:3], LEVELS9, thr)
    assert np.array_equal(q5[0].view(np.uint64), q0[0, :2].view(np.uint64)) and np.array_equal(c5[0], c0[0, :2]) and np.array_equal(w5[0], w0[0, :2])
    for got_c, got_q, got_w, g in ((c0, q0, w0, grp), (c4, q4, w4, grp2)):
        _compare(_cells([np.asarray(c) for c in clocks], g, 3, edges), got_c, got_q, got_w, LEVELS9, thr)


def test_the_whole_run_takes_any_row_order_and_windows_refuse_an_inversion_untouched():
    """An error code from a finished call, checked once: the kernels read only rows inside the buffers whatever their order."""
    from asyncflow_amd.engine import EngineError

    rng = np.random.default_rng(4)
    edges = np.array([0.0, 10.0, 20.0])
    clocks = [_sorted_clock(rng, [700, 900], edges) for _ in range(8)]
    clocks[5] = clocks[5][rng.permutation(1600)]                        # scenario 5: not in completion order
    assert (np.diff(clocks[5][:, 1]) < 0).any()
    grp = np.arange(8) % 2
    thr = [0.05]
    stored, count, quant, within, _ = _quantiles_synthetic(clocks, grp, 2, None, LEVELS9, thr)
    _compare(_cells(stored, grp, 2, None), count, quant, within, LEVELS9, thr, "whole run, unordered rows")
    keep: dict = {}
    with pytest.raises(EngineError, match=r"scenario 5 is not in completion order"):
        _quantiles_synthetic(clocks, grp, 2, edges, LEVELS9, thr, keep=keep)
    assert (keep["count"] == SENTINEL_U).all() and (keep["within"] == SENTINEL_U).all() and (keep["quantiles"] == SENTINEL_Q).all()
    # the same scenario left out: fine
    grp2 = grp.copy()
    grp2[5] = -1
    stored, count, quant, within, _ = _quantiles_synthetic(clocks, grp2, 2, edges, LEVELS9, thr)
    _compare(_cells(stored, grp2, 2, edges), count, quant, within, LEVELS9, thr, "the inversion left out")


def test_skipped_scenarios_empty_groups_and_finishes_on_an_edge():
    rng = np.random.default_rng(8)
    edges = np.array([1.0, 2.0, 2.5, 4.0, 9.0])
    per = [[5, 0, 600, 9], [0, 0, 0, 0], [513, 512, 511, 1], [9000, 2, 0, 700], [1, 1, 1, 1], [64, 0, 8193, 3]]
    clocks = [_sorted_clock(rng, p, edges, on_edge=2) for p in per]
    clocks[4] = np.concatenate([[[0.5, 1.0]], clocks[4], [[9.0, 9.5]]])     # a finish ON edges[0] and one past the last edge: no window
    grp = np.array([0, 3, -1, 0, 5, 3])                                     # groups 1, 2 and 4 have no member, scenario 2 is left out
    thr = [0.03, float("-inf")]
    stored, count, quant, within, _ = _quantiles_synthetic(clocks, grp, 6, edges, LEVELS9, thr)
    cells = _cells(stored, grp, 6, edges)
    assert sum(c.size == 0 for c in cells.values()) >= 12 and count[5].tolist() == [1, 1, 1, 1]
    _compare(cells, count, quant, within, LEVELS9, thr, "windowed")
    assert (within[:, :, 1] == 0).all()
    for g, w in ((0, 0), (0, 3)):      # the finishes ON the right edge went left
        assert count[g, w] == sum(per[s][w] for s in np.nonzero(grp == g)[0])
    stored, count, quant, within, _ = _quantiles_synthetic(clocks, grp, 6, None, LEVELS9, thr)
    _compare(_cells(stored, grp, 6, None), count, quant, within, LEVELS9, thr, "whole run")
    assert count[:, 0].tolist() == [sum(len(clocks[s]) for s in np.nonzero(grp == g)[0]) for g in range(6)]


def test_every_refusal():
    from asyncflow_amd.engine import EngineError

    rng = np.random.default_rng(1)
    edges = [0.0, 1.0]
    clocks = [_sorted_clock(rng, [5], edges) for _ in range(3)]
    same = [0, 0, 0]
    for lv, what in (([0.5, float("nan")], "levels must lie"), ([-1e-9], "levels must lie"), ([1.0 + 1e-9], "levels must lie"),
                     (np.linspace(0, 1, 65), "at most 64 quantile levels")):
        with pytest.raises(ValueError, match=what):
            _quantiles_synthetic(clocks, same, 1, edges, lv, [0.1])
    with pytest.raises(ValueError, match="must not be NaN"):
        _quantiles_synthetic(clocks, same, 1, edges, [0.5], [0.1, float("nan")])
    with pytest.raises(ValueError, match="at most 64 thresholds"):
        _quantiles_synthetic(clocks, same, 1, edges, [0.5], np.linspace(0, 1, 65))
    with pytest.raises(ValueError, match="at least one"):
        _quantiles_synthetic(clocks, same, 1, edges, [], [])
    _quantiles_synthetic(clocks, same, 1, edges, [0.5], [float("inf"), float("-inf")])          # +-inf thresholds are fine
    for bad, what in (([0.0, 2.0, 1.0], "strictly increasing"), ([0.0, 1.0, 1.0], "strictly increasing"), ([0.0, float("inf")], "not finite"),
                      ([float("nan"), 1.0], "not finite")):
        with pytest.raises(EngineError, match=what):
            _quantiles_synthetic(clocks, same, 1, bad, [0.5])
    for e in (edges, None):
        with pytest.raises(EngineError, match="group id out of range"):
            _quantiles_synthetic(clocks, [0, 2, 0], 2, e, [0.5])
    # capacity: the host refuses from the counts alone, before any kernel reads a row
    keep: dict = {}
    with pytest.raises(EngineError, match=r"group 0 holds 2\^32 or more latencies"):
        _quantiles_synthetic(clocks, same, 1, None, [0.5], [0.1], keep=keep, counts_override=1 << 31, cap_override=1 << 31)
    assert (keep["count"] == SENTINEL_U).all() and (keep["quantiles"] == SENTINEL_Q).all()
    with pytest.raises(EngineError, match=r"below 2\^32 - 1"):
        _quantiles_synthetic(clocks, same, 0xFFFFFFFF, None, [0.5])
    with pytest.raises(EngineError, match=r"below 2\^32 - 1"):
        _quantiles_synthetic(clocks, same, 65537, np.arange(65536.0), [0.5])


def test_the_c_entry_refuses_what_the_python_wrapper_would_not_pass():
    import ctypes as C

    import torch

    from asyncflow_amd.engine import Engine

    dev = torch.device("cuda", 0)
    clock = torch.zeros((2, 4, 2), dtype=torch.float64, device=dev)
    counts = torch.zeros((2, _abi.CNT_SLOTS), dtype=torch.int32, device=dev)
    cnt = torch.zeros((1, 1), dtype=torch.int32, device=dev)
    eng = Engine(lower(single_server(horizon=50)), 0)
    lib, h = eng._lib, eng._h  # noqa: SLF001
    pd = C.POINTER(C.c_double)
    out = _abi.AfOutputs(4, C.c_void_p(clock.data_ptr()), 0, None, C.c_void_p(counts.data_ptr()))
    edges = (C.c_double * 2)(0.0, 1.0)

    def call(n_win, e, lv, th, n_lev=None, n_thr=None):
        lv_a = (C.c_double * max(len(lv), 1))(*lv)
        th_a = (C.c_double * max(len(th), 1))(*th)
        req = _abi.AfQuantiles(2, 1, n_win, None, e, len(lv) if n_lev is None else n_lev, C.cast(lv_a, pd),
                               len(th) if n_thr is None else n_thr, C.cast(th_a, pd), C.c_void_p(cnt.data_ptr()), None, None, 0.0, 0)
        return lib.af_engine_summarize_quantiles(h, C.byref(out), C.byref(req)), lib.af_last_error().decode()

    try:
        assert call(1, edges, [0.5], [])[0] == _abi.AF_OK
        assert call(0, None, [], [0.5])[0] == _abi.AF_OK
        for args, what in (((1, edges, [float("nan")], []), "not in [0, 1]"), ((1, edges, [1.5], []), "not in [0, 1]"),
                           ((1, edges, [-0.5], []), "not in [0, 1]"), ((1, edges, [0.5], [float("nan")]), "is NaN"),
                           ((1, edges, [], []), "without levels and without thresholds"),
                           ((1, None, [0.5], []), "edges is required"), ((0, edges, [0.5], []), "n_windows == 0")):
            rc, msg = call(*args)
            assert rc == _abi.AF_ERR_INVALID and what in msg, (args, rc, msg)
        rc, msg = call(1, edges, [0.5], [], n_lev=65)
        assert rc == _abi.AF_ERR_INVALID and "AF_MAX_QUANTILE_LEVELS" in msg
        rc, msg = call(1, edges, [0.5], [0.5], n_thr=65)
        assert rc == _abi.AF_ERR_INVALID and "AF_MAX_SLO_THRESHOLDS" in msg
    finally:
        eng.close()


def test_a_million_small_cells_stay_within_the_scratch_bound():
    """1 024 scenarios x 1 024 windows, every scenario its own group: 1 048 576 cells of 0 .. 5 latencies, every one compared.
    The documented bound (asyncflow_hip.h) without large cells: 8 B per latency in a cell + 4 B per (scenario, edge) + 4 B per
    (scenario, window) + 12 B per cell + 8 B per scenario + 8 B per edge + 1 KB (levels, thresholds) + 4 KB of alignment."""
    rng = np.random.default_rng(99)
    n, n_win = 1024, 1024
    edges = np.arange(n_win + 1, dtype=np.float64)
    sizes = rng.choice([0, 1, 2, 3, 5], size=(n, n_win))
    clocks = []
    for s in range(n):
        w_of = np.repeat(np.arange(n_win), sizes[s])
        fin = np.sort(w_of + rng.uniform(0.01, 0.99, w_of.size))        # (sorted as a whole: every finish stays in its window)
        lat = rng.lognormal(-3.0, 0.8, fin.size)
        clocks.append(np.stack([fin - lat, fin], axis=1))
    levels, thr = [0.0, 0.5, 0.9, 0.999, 1.0], [0.05, 0.2]
    stored, count, quant, within, scratch = _quantiles_synthetic(clocks, np.arange(n), n, edges, levels, thr)
    assert np.array_equal(count, sizes)
    total = int(sizes.sum())
    bound = 8 * total + 4 * n * (n_win + 1) + 4 * n * n_win + 12 * n * n_win + 8 * n + 8 * (n_win + 1) + 1024 + 4096
    print(f"scratch_bytes {scratch} bound {bound} cells {n * n_win} latencies {total}")
    assert 0 < scratch <= bound
    # every cell, vectorised by cell size (np.quantile along an axis is np.quantile on every row)
    lat_all = [c[:, 1] - c[:, 0] for c in stored]
    starts = np.concatenate([np.zeros((n, 1), dtype=np.int64), np.cumsum(sizes, axis=1)[:, :-1]], axis=1)
    checked = 0
    for k in (0, 1, 2, 3, 5):
        ss, ww = np.nonzero(sizes == k)
        checked += ss.size
        if k == 0:
            assert np.isnan(quant[ss, ww]).all() and (within[ss, ww] == 0).all()
            continue
        rows = np.stack([lat_all[s][starts[s, w]:starts[s, w] + k] for s, w in zip(ss, ww)])
        want = np.quantile(rows, levels, axis=1).T
        assert np.array_equal(quant[ss, ww].view(np.uint64), np.ascontiguousarray(want).view(np.uint64)), k
        for j, th in enumerate(thr):
            assert np.array_equal(within[ss, ww, j], np.count_nonzero(rows <= th, axis=1)), (k, j)
    assert checked == n * n_win
    one = np.quantile(lat_all[7][starts[7, 3]:starts[7, 3] + sizes[7, 3]], levels) if sizes[7, 3] else None
    if one is not None:
        assert np.array_equal(quant[7, 3].view(np.uint64), one.view(np.uint64))


def _host_cells(res, ids, n_groups, edges, levels, thr):
    """The host definitions on every (group, window): the members' rows concatenated in ascending scenario order."""
    n_win = 1 if edges is None else len(edges) - 1
    cnt = np.zeros((n_groups, n_win), dtype=np.int64)
    qt = np.full((n_groups, n_win, len(levels)), np.nan)
    wt = np.zeros((n_groups, n_win, len(thr)), dtype=np.int64)
    clocks = [res[s].rqs_clock for s in range(len(res))]
    for g in range(n_groups):
        members = np.nonzero(ids == g)[0]
        for w in range(n_win):
            seg = []
            for s in members:
                fin = clocks[s][:, 1]
                m = np.ones(fin.shape, dtype=bool) if edges is None else (fin > edges[w]) & (fin <= edges[w + 1])
                seg.append(clocks[s][m])
            rows = np.concatenate(seg) if seg else np.zeros((0, 2))
            c, q, wi = latency_window_quantiles(rows, None, levels, thr)
            cnt[g, w], qt[g, w], wt[g, w] = c[0], q[0], wi[0]
            if rows.shape[0]:
                assert np.array_equal(q[0].view(np.uint64), np.quantile(rows[:, 1] - rows[:, 0], levels).view(np.uint64))
                assert np.array_equal(latency_quantiles(rows[:, 1] - rows[:, 0], levels).view(np.uint64), q[0].view(np.uint64))
    return cnt, qt, wt


def _check_summary(a, cnt, qt, wt, what):
    assert np.array_equal(a["count"].cpu().numpy(), cnt), what
    assert np.array_equal(a["within"].cpu().numpy(), wt), what
    got = a["quantiles"].cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(qt)) and np.array_equal(got[~np.isnan(qt)].view(np.uint64), qt[~np.isnan(qt)].view(np.uint64)), what
    share = a["share"].cpu().numpy()
    with np.errstate(invalid="ignore", divide="ignore"):
        want = np.where(cnt[:, :, None] > 0, wt / cnt[:, :, None].astype(np.float64), np.nan)
    assert np.array_equal(share, want, equal_nan=True), what


@pytest.mark.parametrize("scenario", ["lb_with_events", "lb_two_servers"])
def test_simulated_batches_through_the_python_api(tmp_path, scenario):
    from statistics import NormalDist

    from asyncflow_amd import expand_grid
    from asyncflow_amd.results import load_summary
    from asyncflow_amd.runner import SimulationRunner

    payload = lb_with_events(horizon=60, scale=0.1) if scenario == "lb_with_events" else lb_two_servers(horizon=60)
    users = "rqs_input.avg_active_users.mean"
    grid = expand_grid({users: [40.0, 120.0, 300.0], "topology_graph.edges[*].latency.mean": [0.002, 0.006]}, replicas=4, order_by_load=users)
    res = SimulationRunner(simulation_input=payload, **grid.runner_kwargs()).run()
    n = len(res)
    levels, thr = [0.5, 0.9, 0.999, 0.0, 1.0, 0.9], [0.02, 0.05, float("inf")]
    edges = window_edges(5.0, res.plan.total_time)
    assert edges.tolist() == [5.0 * k for k in range(13)]
    for by, ids, g in ((None, np.zeros(n, dtype=np.int64), 1), ("scenario", np.arange(n), n), (grid, grid.point, 6)):
        for e in (edges, None):
            a = res.quantile_summary(levels, thresholds=thr, window_s=5.0 if e is not None else None, by=by)
            assert tuple(a["quantiles"].shape) == (g, 12 if e is not None else 1, 6)
            assert (a["edges"] is None) if e is None else np.array_equal(a["edges"], edges)
            cnt, qt, wt = _host_cells(res, ids, g, e, levels, thr)
            assert np.count_nonzero(cnt) * 2 >= cnt.size, "at least half of the cells hold latencies"
            _check_summary(a, cnt, qt, wt, (scenario, by if isinstance(by, str) else g, e is None))
            assert (a["within"].cpu().numpy()[:, :, 2] == cnt).all()
            assert a["replicas"].tolist() == np.bincount(ids, minlength=g).tolist() and a["scratch_bytes"] > 0
    # per scenario: ScenarioResults.get_latency_quantiles is the same definition
    a = res.quantile_summary(levels, thresholds=thr, window_s=5.0, by="scenario")
    for s in (0, n // 2, n - 1):
        one = res[s].get_latency_quantiles(levels, window_s=5.0, thresholds=thr)
        got = a["quantiles"].cpu().numpy()[s]
        assert np.array_equal(np.isnan(got), np.isnan(one["quantiles"]))
        assert np.array_equal(got[~np.isnan(got)].view(np.uint64), one["quantiles"][~np.isnan(got)].view(np.uint64))
        assert np.array_equal(a["count"].cpu().numpy()[s], one["count"]) and np.array_equal(a["within"].cpu().numpy()[s], one["within"])
        whole = res[s].get_latency_quantiles(levels)
        assert np.array_equal(whole["quantiles"].view(np.uint64), np.quantile(res[s].rqs_clock[:, 1] - res[s].rqs_clock[:, 0], levels).view(np.uint64))

    # bands over the replicas: the last window lies past the horizon (no replica has a completion there: NaN)
    edges_b = np.concatenate([edges, [70.0]])
    bands = res.quantile_bands(levels, thresholds=thr, edges=edges_b, by=grid, level=0.9, q=(0.1, 0.75))
    per = [latency_window_quantiles(res[s].rqs_clock, edges_b, levels, thr) for s in range(n)]
    with np.errstate(invalid="ignore", divide="ignore"):
        body_all = np.stack([np.concatenate([q, np.where(c[:, None] > 0, w / c[:, None].astype(np.float64), np.nan)], axis=1) for c, q, w in per])   # [n, 13, 9]
    cnt_all = np.stack([c for c, _, _ in per])
    z = NormalDist().inv_cdf(0.95)
    for g in range(6):
        members = np.nonzero(grid.point == g)[0]
        for w in range(13):
            body = body_all[members, w][cnt_all[members, w] > 0]
            assert bands["n"][g, w] == body.shape[0]
            if body.shape[0] == 0:
                for k in ("mean", "std", "ci_halfwidth", "q_lo", "q_hi"):
                    assert np.isnan(bands[k][g, w]).all(), (k, g, w)
                continue
            sd = body.std(axis=0, ddof=1) if body.shape[0] > 1 else np.full(body.shape[1], np.nan)
            np.testing.assert_allclose(bands["mean"][g, w], body.mean(axis=0), rtol=1e-12)
            # (values of magnitude <= 1: where the replicas agree to the last digit the two-pass deviations are rounding residue
            # of the mean, at most a few 1e-16 -- hence the absolute term)
            np.testing.assert_allclose(bands["std"][g, w], sd, rtol=1e-9, atol=1e-15)
            np.testing.assert_allclose(bands["ci_halfwidth"][g, w], z * sd / np.sqrt(body.shape[0]), rtol=1e-9, atol=1e-15)
            np.testing.assert_allclose(bands["q_lo"][g, w], np.quantile(body, 0.1, axis=0), rtol=1e-12)
            np.testing.assert_allclose(bands["q_hi"][g, w], np.quantile(body, 0.75, axis=0), rtol=1e-12)
    assert (bands["n"][:, 12] == 0).all()
    cnt, qt, wt = _host_cells(res, grid.point, 6, edges_b, levels, thr)
    assert np.array_equal(bands["pooled_count"], cnt)
    assert np.array_equal(bands["pooled_quantiles"].view(np.uint64)[~np.isnan(qt)], qt.view(np.uint64)[~np.isnan(qt)]) and np.isnan(bands["pooled_quantiles"][:, 12]).all()

    # one row per point, both formats, windows and the whole run
    pooled = res.quantile_summary(levels, thresholds=thr, window_s=5.0, by=grid)
    for name, kw, n_win in (("q.npz", {"window_s": 5.0}, 12), ("q.parquet", {"window_s": 5.0}, 12), ("whole.npz", {}, 1), ("whole.parquet", {}, 1)):
        written = res.save_quantile_summary(str(tmp_path / name), grid, levels=levels, thresholds=thr, **kw)
        back = load_summary(str(tmp_path / name))
        assert set(back) == set(written)
        for k, v in written.items():
            assert np.array_equal(np.asarray(back[k], dtype=v.dtype).reshape(v.shape), v, equal_nan=v.dtype.kind == "f"), (name, k)
        for k, v in grid.point_columns().items():
            assert np.array_equal(back[f"param:{k}"], v)
        assert np.asarray(back["quantile_pooled:2"]).shape == (6, n_win) and back["replicas"].tolist() == [4] * 6
        assert np.array_equal(back["quantile_levels"], levels) and np.array_equal(back["slo_thresholds"], thr)
        if n_win == 12:
            assert np.array_equal(back["window_edges"], edges)
            assert np.array_equal(np.asarray(back["quantile_pooled:2"]), pooled["quantiles"].cpu().numpy()[:, :, 2], equal_nan=True)
            assert np.array_equal(np.asarray(back["share_pooled:0"]), pooled["share"].cpu().numpy()[:, :, 0], equal_nan=True)
            assert np.array_equal(np.asarray(back["quantile_count"]), pooled["count"].cpu().numpy())
        else:
            assert np.asarray(back["window_edges"]).size == 0
    res2 = SimulationRunner(simulation_input=lb_two_servers(horizon=10), seeds=0x5EED0000 + np.arange(4, dtype=np.uint64), collect_clock=False).run()
    with pytest.raises(RuntimeError, match="kept no rqs_clock"):
        res2.quantile_summary([0.5])
    with pytest.raises(ValueError, match="not both"):
        res.quantile_summary([0.5], window_s=1.0, edges=[0.0, 1.0])
    with pytest.raises(ValueError, match="by must be"):
        res.quantile_summary([0.5], by="point")
