"""Sampled-series analyzer per (group, window of ticks) on the MI355X (af_engine_summarize_series_windows): synthetic sample
blocks handed straight to the entry -- padding words and the rows past a scenario's ticks filled with garbage -- against the
host definition bit for bit, on plans of 6, 12 and 42 series; arbitrary float32 RAM values against math.fsum; run-to-run and
batch independence; NULL outputs; the scratch bound; then event workloads through the Python API, bands, the on-disk summary
in both formats (tests of their own) and 14.4 M (cell, series) entries of singleton groups."""

from __future__ import annotations

import ctypes as C
import json
import math
from pathlib import Path

import numpy as np
import pytest

from asyncflow_amd import _abi
from asyncflow_amd.plan import lower
from asyncflow_amd.results import series_window_stats, tick_window_edges
from oracle.scenarios import lb_two_servers, lb_with_events, single_server

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GARBAGE = 0xDEADBEEF


def ram_columns(n_series: int, n_edges: int) -> np.ndarray:
    """The ram_in_use columns (float32 words), stated here and not taken from the package: the edges come first, then
    ready_queue_len, event_loop_io_sleep, ram_in_use per server (include/asyncflow_hip.h)."""
    return np.array([j >= n_edges and (j - n_edges) % 3 == 2 for j in range(n_series)], dtype=bool)


def _plan(name: str):
    if name == "single_server":
        return lower(single_server(horizon=50))
    if name == "lb_two_servers":
        return lower(lb_two_servers(horizon=20))
    z = np.load(ROOT / "tests" / "golden" / "fanout8_t20.npz")          # the 8-server fan-out: 42 series
    return lower(json.loads(str(z["payload_json"])))


def _block(plan, rng, n: int, cap: int, ticks, dyadic: bool = True):
    """Sample blocks [n, cap, pitch] of words: integer columns uniform in [0, 2^20], ram columns random multiples of 1/256
    below 2^16 (or, dyadic=False, arbitrary non-negative float32 over many binades); padding words and the rows at and past
    a scenario's min(ticks, cap) hold garbage.  Returns the block and the counts."""
    S, pitch = plan.n_series, plan.series_pitch
    ram = ram_columns(S, plan.n_edges)
    blk = np.full((n, cap, pitch), GARBAGE, dtype=np.uint32)
    body = rng.integers(0, 2 ** 20 + 1, (n, cap, S)).astype(np.uint32)
    if dyadic:
        f = (rng.integers(0, 2 ** 24, (n, cap, int(ram.sum()))) / 256.0).astype(np.float32)
    else:
        f = (rng.lognormal(0.0, 6.0, (n, cap, int(ram.sum()))) * (rng.random((n, cap, int(ram.sum()))) > 0.1)).astype(np.float32)
    body[:, :, ram] = f.view(np.uint32)
    blk[:, :, :S] = body
    counts = np.zeros((n, _abi.CNT_SLOTS), dtype=np.uint32)
    counts[:, _abi.CNT_TICKS] = ticks
    for s in range(n):
        blk[s, min(int(counts[s, _abi.CNT_TICKS]), cap):] = rng.integers(0, 2 ** 32, dtype=np.uint32) | np.uint32(0x7F800000)
    return blk, counts


def _run(plan, blk, counts, group, n_groups, tick_edges, thresholds=None, outputs=("min", "max", "above")):
    """The block through af_engine_summarize_series_windows on a fresh engine.  Every output lies inside one buffer with a
    sentinel on each side; returns the outputs as numpy, the scratch size and whether all sentinels stayed."""
    import torch

    from asyncflow_amd.engine import Engine

    n, cap, _ = blk.shape
    S, W = plan.n_series, len(tick_edges) - 1
    dev = torch.device("cuda", 0)
    blk_t = torch.as_tensor(blk.view(np.int32), device=dev)
    counts_t = torch.as_tensor(counts.view(np.int32), device=dev)
    grp_t = None
    if group is not None:
        g = np.asarray(group, dtype=np.int64)
        grp_t = torch.as_tensor(np.where(g < 0, _abi.POOL_SKIP, g).astype(np.uint32).view(np.int32), device=dev)
    cells = n_groups * W
    guard = 64                                                       # int32 words of sentinel between the outputs
    sizes = {"count": cells, "mean": 2 * cells * S, "min": cells * S, "max": cells * S, "above": cells * S}
    off, at = {}, guard
    for k, sz in sizes.items():
        off[k] = at
        at += sz + guard + (sz + guard) % 2                           # (keeps every output 8-byte aligned)
    buf = torch.full((at,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    ptr = {k: buf.data_ptr() + 4 * o for k, o in off.items()}
    eng = Engine(plan, 0)
    try:
        _, scratch = eng.summarize_series_windows(
            n, n_groups, tick_edges, samples_ptr=blk_t.data_ptr(), tick_capacity=cap, counts_ptr=counts_t.data_ptr(),
            count_ptr=ptr["count"], mean_ptr=ptr["mean"], min_ptr=ptr["min"] if "min" in outputs else 0,
            max_ptr=ptr["max"] if "max" in outputs else 0, above_ptr=ptr["above"] if "above" in outputs else 0,
            group_ptr=grp_t.data_ptr() if grp_t is not None else 0, thresholds=thresholds)
    finally:
        eng.close()
    host = buf.cpu().numpy()
    written = np.zeros(at, dtype=bool)
    out = {}
    for k, sz in sizes.items():
        if k in ("count", "mean") or k in outputs:
            written[off[k]:off[k] + sz] = True
            out[k] = host[off[k]:off[k] + sz].view(np.uint32)
    out["count"] = out["count"].reshape(n_groups, W)
    out["mean"] = out["mean"].view(np.float64).reshape(n_groups, W, S)
    for k in outputs:
        out[k] = out[k].reshape(n_groups, W, S)
    return out, scratch, bool((host[~written] == 0x5A5A5A5A).all())


def _reduceat(fn, arr, r):
    """fn over the columns [r[w], r[w + 1]) of arr [S, len] for every w (an empty range: anything)."""
    padded = np.concatenate([arr, np.zeros((arr.shape[0], 1), dtype=arr.dtype)], axis=1)
    return fn.reduceat(padded, r, axis=1)[:, :-1]


def _want(plan, blk, counts, group, n_groups, tick_edges, thresholds=None, fsum: bool = False):
    """The definition on the host, independent of results.series_window_stats: per scenario exact window sums (integers; the
    dyadic float values add exactly in float64 in any order), word minima / maxima and counts above the threshold by
    ufunc.reduceat, then the members of a group combined.  fsum=True: the float means by math.fsum over the cell."""
    n, cap, _ = blk.shape
    S = plan.n_series
    ram = ram_columns(S, plan.n_edges)
    b = np.asarray(tick_edges, dtype=np.int64)
    W = len(b) - 1
    thr = np.zeros(S) if thresholds is None else np.asarray(thresholds, dtype=np.float64)
    group = np.zeros(n, dtype=np.int64) if group is None else np.asarray(group)
    count = np.zeros((n_groups, W), dtype=np.int64)
    isum = np.zeros((n_groups, W, S), dtype=np.int64)
    fsm = np.zeros((n_groups, W, S))
    terms = [[[] for _ in range(W)] for _ in range(n_groups)]
    mn = np.full((n_groups, W, S), 0xFFFFFFFF, dtype=np.uint32)
    mx = np.zeros((n_groups, W, S), dtype=np.uint32)
    above = np.zeros((n_groups, W, S), dtype=np.int64)
    for s in range(n):
        g = int(group[s])
        if g < 0:
            continue
        m = min(int(counts[s, _abi.CNT_TICKS]), cap)
        words = np.ascontiguousarray(blk[s, :m, :S].T)                # [S, m]
        r = np.minimum(b, m)
        c = np.diff(r)
        live = c > 0
        values = words.astype(np.float64)
        values[ram] = words[ram].view(np.float32).astype(np.float64)
        count[g] += c
        isum[g] += np.where(live, _reduceat(np.add, words.astype(np.int64), r), 0).T
        fsm[g] += np.where(live, _reduceat(np.add, values, r), 0.0).T
        above[g] += np.where(live, _reduceat(np.add, (values > thr[:, None]).astype(np.int64), r), 0).T
        mn[g] = np.minimum(mn[g], np.where(live, _reduceat(np.minimum, words, r), 0xFFFFFFFF).astype(np.uint32).T)
        mx[g] = np.maximum(mx[g], np.where(live, _reduceat(np.maximum, words, r), 0).astype(np.uint32).T)
        if fsum:
            for w in np.nonzero(live)[0]:
                terms[g][w].append(values[:, r[w]:r[w + 1]])
    empty = count == 0
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(ram, fsm, isum.astype(np.float64)) / count[:, :, None].astype(np.float64)
    mean[empty] = np.nan
    mn[empty] = 0
    if fsum:
        for g in range(n_groups):
            for w in range(W):
                if count[g, w]:
                    cell = np.concatenate(terms[g][w], axis=1)
                    mean[g, w, ram] = [math.fsum(row.tolist()) / cell.shape[1] for row in cell[ram]]
    return {"count": count, "mean": mean, "min": mn, "max": mx, "above": above.astype(np.uint32)}


def _same(got, want, what, ram=None, float_tol: bool = False):
    assert np.array_equal(got["count"], want["count"].astype(np.uint32)), what
    for k in ("min", "max", "above"):
        if k in got:
            assert np.array_equal(got[k], want[k]), (what, k, np.argwhere(got[k] != want[k])[:5])
    if not float_tol:
        bad = np.argwhere(got["mean"].view(np.uint64) != want["mean"].view(np.uint64))
        bad = [t for t in bad if not (np.isnan(got["mean"][tuple(t)]) and np.isnan(want["mean"][tuple(t)]))]
        assert not bad, (what, bad[:5])
        return
    exact = ~ram
    assert np.array_equal(got["mean"][:, :, exact], want["mean"][:, :, exact], equal_nan=True), what
    n = want["count"][:, :, None].astype(np.float64)
    err = np.abs(got["mean"][:, :, ram] - want["mean"][:, :, ram])
    print(f"{what}: largest float-mean error / (n * 2^-52 * mean) = "
          f"{np.nanmax(err / np.maximum(n * 2.0 ** -52 * np.abs(want['mean'][:, :, ram]), 1e-300)):.3g}, largest cell {int(n.max())}")
    assert n.max() <= 4096
    assert ((err <= n * 2.0 ** -52 * np.abs(want["mean"][:, :, ram])) | (want["count"] == 0)[:, :, None]).all(), what
    assert np.isnan(got["mean"][want["count"] == 0]).all()


def _ticks(rng, n: int, cap: int) -> np.ndarray:
    t = rng.integers(1, cap + 1, n)
    t[0], t[1], t[2], t[3] = 0, cap, cap + 50, 1                       # no tick at all, all of them, more than were stored
    return t


def _thresholds(plan, blk) -> np.ndarray:
    """Per series: 0.0, a value that occurs in the data (strictly greater decides), 0.5 on an integer column, a value on a
    ram column."""
    S = plan.n_series
    ram = ram_columns(S, plan.n_edges)
    thr = np.zeros(S)
    for j in range(1, S):
        w = blk[1, 0, j]                                               # (scenario 1 stored every tick)
        thr[j] = float(np.uint32(w).view(np.float32)) if ram[j] else float(w)
    thr[1] = 0.5
    assert not ram[0] and not ram[1] and ram.any() and (thr[ram] > 0).all()
    return thr


@pytest.mark.parametrize("name", ["single_server", "lb_two_servers", "fanout8"])
def test_synthetic_blocks_equal_the_host_definition(name):
    plan = _plan(name)
    assert (plan.n_series, plan.series_pitch) == {"single_server": (6, 8), "lb_two_servers": (12, 12), "fanout8": (42, 44)}[name]
    rng = np.random.default_rng(len(name))
    n, cap = 23, 700
    blk, counts = _block(plan, rng, n, cap, _ticks(rng, n, cap))
    assert (blk[1, :, plan.n_series:] == GARBAGE).all()                 # (scenario 1 stored every tick: its padding words)
    interleaved = np.array([(i * 7) % 6 for i in range(n)])
    interleaved[interleaved == 3] = 4                                  # group 3 is empty
    interleaved[[2, 9, 20]] = -1                                       # and three scenarios are left out
    sparse = np.arange(n) * 2                                          # singletons, every other group without a member
    sparse[5] = -1
    groupings = [(None, 1, "one group (NULL)"), (np.zeros(n, dtype=np.int64), 1, "one group"), (interleaved, 6, "interleaved"),
                 (np.arange(n), n, "singletons"), (sparse, 2 * n, "singletons and empty groups")]
    shapes = [("one window", np.array([0, cap])), ("one tick each", np.arange(cap + 1)), ("20 ticks", tick_window_edges(20, cap)),
              ("64 ticks", tick_window_edges(64, cap)), ("65 ticks", tick_window_edges(65, cap)),
              ("200 ticks", tick_window_edges(200, cap)),
              ("uneven", np.array([3, 4, 10, 75, 76, 300, 650, cap - 1, cap, cap + 9, cap + 10, 5 * cap]))]
    thr = _thresholds(plan, blk)
    for what, edges in shapes:
        for group, n_groups, gname in groupings:
            if what == "one tick each" and gname not in ("interleaved", "singletons"):
                continue
            for t in (None, thr):
                got, _, intact = _run(plan, blk, counts, group, n_groups, edges, t)
                want = _want(plan, blk, counts, group, n_groups, edges, t)
                _same(got, want, f"{name}, {what}, {gname}, thresholds {'set' if t is not None else 'none'}")
                assert intact
    # singletons are the host definition of the package itself, scenario by scenario
    edges = shapes[-1][1]
    got, _, _ = _run(plan, blk, counts, np.arange(n), n, edges, thr)
    assert (got["count"][:, -2:] == 0).all() and np.isnan(got["mean"][:, -2:]).all() and (got["count"][0] == 0).all()
    for s in range(n):
        m = min(int(counts[s, _abi.CNT_TICKS]), cap)
        host = series_window_stats(np.ascontiguousarray(blk[s, :m, :plan.n_series].T), edges, plan.n_edges, thr)
        _same({k: v[s:s + 1] for k, v in got.items()}, {k: v[None] for k, v in host.items()}, f"{name}, scenario {s}")


def test_long_windows_and_long_runs():
    plan = _plan("lb_two_servers")
    rng = np.random.default_rng(41)
    n, cap = 6, 9000
    ticks = np.array([9000, 8191, 4097, 12000, 0, 4096])
    blk, counts = _block(plan, rng, n, cap, ticks)
    for edges in (tick_window_edges(4096, cap), np.array([0, cap]), np.array([5, 4101, 8197, 8198])):
        for group, n_groups in ((None, 1), (np.arange(n), n), (np.array([1, 0, 1, -1, 0, 1]), 3)):
            got, _, intact = _run(plan, blk, counts, group, n_groups, edges)
            _same(got, _want(plan, blk, counts, group, n_groups, edges), f"edges {edges.tolist()}, groups {n_groups}")
            assert intact


def test_arbitrary_float_values_run_to_run_and_batch_independence():
    plan = _plan("lb_two_servers")
    ram = ram_columns(plan.n_series, plan.n_edges)
    rng = np.random.default_rng(5)
    n, cap = 8, 512
    blk, counts = _block(plan, rng, n, cap, _ticks(rng, n, cap), dyadic=False)
    edges = tick_window_edges(200, cap)
    for group, n_groups in ((None, 1), (np.arange(n) % 3, 3), (np.arange(n), n)):
        got, _, _ = _run(plan, blk, counts, group, n_groups, edges)
        again, _, _ = _run(plan, blk, counts, group, n_groups, edges)
        for k in got:
            assert got[k].tobytes() == again[k].tobytes(), k              # the same call twice: identical bytes
        _same(got, _want(plan, blk, counts, group, n_groups, edges, fsum=True), f"arbitrary floats, {n_groups} groups", ram, float_tol=True)
    # the same scenarios inside a batch ten times as large: identical bytes for their cells
    for edges in (tick_window_edges(200, cap), tick_window_edges(7, cap), np.array([0, cap])):
        alone, _, _ = _run(plan, blk, counts, np.arange(n), n, edges)
        big, big_counts = _block(plan, rng, 10 * n, cap, rng.integers(0, cap + 1, 10 * n), dyadic=False)
        where = np.arange(n) * 10 + 3
        big[where], big_counts[where] = blk, counts
        inside, _, _ = _run(plan, big, big_counts, np.arange(10 * n), 10 * n, edges)
        for k in alone:
            assert alone[k].tobytes() == np.ascontiguousarray(inside[k][where]).tobytes(), k


def test_null_outputs_are_skipped():
    plan = _plan("single_server")
    rng = np.random.default_rng(2)
    n, cap = 9, 300
    blk, counts = _block(plan, rng, n, cap, _ticks(rng, n, cap))
    edges = tick_window_edges(64, cap)
    for group, n_groups in ((np.arange(n) % 2, 2), (np.arange(n), n)):
        full, _, intact = _run(plan, blk, counts, group, n_groups, edges)
        assert intact
        for outputs in ((), ("max",), ("min", "above")):
            got, _, intact = _run(plan, blk, counts, group, n_groups, edges, outputs=outputs)
            assert intact, f"a NULL output was written to (outputs {outputs})"
            assert set(got) == {"count", "mean", *outputs}
            for k in got:
                assert got[k].tobytes() == full[k].tobytes(), k


def _scratch_bound(n, n_groups, n_win, n_series, records: bool) -> int:
    """include/asyncflow_hip.h: 4 B per edge + 8 B per series + 4 B per group + 4 B per scenario + 2 KB of alignment, and
    -- unless every group holds at most one scenario -- 20 B per (scenario, window, series)."""
    return 4 * (n_win + 1) + 8 * n_series + 4 * (n_groups + 1) + 4 * n + 2048 + (20 * n * n_win * n_series if records else 0)


def test_scratch_stays_within_the_bound_of_the_header():
    plan = _plan("fanout8")
    rng = np.random.default_rng(3)
    n, cap = 40, 400
    blk, counts = _block(plan, rng, n, cap, rng.integers(0, cap + 1, n))
    edges = tick_window_edges(20, cap)
    W, S = len(edges) - 1, plan.n_series
    _, scratch, _ = _run(plan, blk, counts, np.arange(n) % 7, 7, edges)
    print(f"groups of several: scratch_bytes {scratch}, bound {_scratch_bound(n, 7, W, S, True)}")
    assert 20 * n * W * S <= scratch <= _scratch_bound(n, 7, W, S, True)
    _, scratch, _ = _run(plan, blk, counts, np.arange(n) * 3, 3 * n, edges)
    print(f"singletons: scratch_bytes {scratch}, bound {_scratch_bound(n, 3 * n, W, S, False)}")
    assert 0 < scratch <= _scratch_bound(n, 3 * n, W, S, False) < 20 * n * W * S


def test_device_argument_checks():
    """Error codes from calls that return before any kernel is launched."""
    import torch

    from asyncflow_amd.engine import Engine, EngineError, load_library

    plan = _plan("lb_two_servers")
    rng = np.random.default_rng(1)
    blk, counts = _block(plan, rng, 3, 50, [50, 20, 0])
    with pytest.raises(EngineError, match="group id out of range"):
        _run(plan, blk, counts, [0, 2, 0], 2, [0, 50])
    lib = load_library()
    dev = torch.device("cuda", 0)
    blk_t = torch.as_tensor(blk.view(np.int32), device=dev)
    counts_t = torch.as_tensor(counts.view(np.int32), device=dev)
    outs = torch.zeros(4096, dtype=torch.int32, device=dev)
    eng = Engine(plan, 0)
    try:
        def call(edges, thr=None, samples=True, n_groups=1, n_windows=None):
            e = (C.c_uint32 * len(edges))(*edges)
            t = (C.c_double * len(thr))(*thr) if thr is not None else None
            out = _abi.AfOutputs(0, None, 50, C.c_void_p(blk_t.data_ptr() if samples else None), C.c_void_p(counts_t.data_ptr()))
            req = _abi.AfSeriesWindows(3, n_groups, len(edges) - 1 if n_windows is None else n_windows, None, e, t,
                                       C.c_void_p(outs.data_ptr()), C.c_void_p(outs.data_ptr() + 1024), None, None, None, 0.0, 0)
            rc = lib.af_engine_summarize_series_windows(eng._h, C.byref(out), C.byref(req))  # noqa: SLF001
            return rc, lib.af_last_error().decode()

        assert call([0, 10, 10])[0] == _abi.AF_ERR_INVALID and "strictly increasing" in call([0, 10, 10])[1]
        assert call([10, 5])[0] == _abi.AF_ERR_INVALID
        assert call([0], n_windows=0)[0] == _abi.AF_ERR_INVALID
        rc, msg = call([0, 10], thr=[0.0] * 5 + [float("nan")] + [0.0] * 6)
        assert rc == _abi.AF_ERR_INVALID and "NaN" in msg
        rc, msg = call([0, 10], samples=False)
        assert rc == _abi.AF_ERR_INVALID and "samples" in msg
        rc, msg = call([0, 10], n_groups=0xFFFFFFFF)
        assert rc == _abi.AF_ERR_CAPACITY and "2^32" in msg
        assert call([0, 10])[0] == _abi.AF_OK and (outs[:1].cpu().numpy() == 10 + 10 + 0).all()
    finally:
        eng.close()


def _cells_on_the_host(res, ids, n_groups, edges, thr=None):
    """results.series_window_stats on every cell's samples: the members' window rows concatenated in scenario order."""
    W, S = len(edges) - 1, res.plan.n_series
    out = {"count": np.zeros((n_groups, W), dtype=np.int64), "mean": np.full((n_groups, W, S), np.nan),
           "min": np.zeros((n_groups, W, S), dtype=np.uint32), "max": np.zeros((n_groups, W, S), dtype=np.uint32),
           "above": np.zeros((n_groups, W, S), dtype=np.uint32)}
    words = [res[s]._samples for s in range(len(res))]  # noqa: SLF001
    for g in range(n_groups):
        members = np.nonzero(ids == g)[0]
        for w in range(W):
            seg = [words[s][:, min(edges[w], words[s].shape[1]):min(edges[w + 1], words[s].shape[1])] for s in members]
            cell = np.concatenate(seg, axis=1) if seg else np.zeros((S, 0), dtype=np.uint32)
            st = series_window_stats(cell, [0, max(cell.shape[1], 1)], res.plan.n_edges, thr)
            for k in out:
                out[k][g, w] = st[k][0]
    return out


def _api_as_numpy(a):
    return {"count": a["count"].cpu().numpy().astype(np.uint32), "mean": a["mean"].cpu().numpy(),
            "min": a["min_words"].cpu().numpy().view(np.uint32), "max": a["max_words"].cpu().numpy().view(np.uint32),
            "above": a["above"].cpu().numpy().view(np.uint32)}


def test_event_workload_through_the_python_api():
    from statistics import NormalDist

    from asyncflow_amd import expand_grid
    from asyncflow_amd.runner import SimulationRunner

    payload = lb_with_events(horizon=60, scale=0.1)
    # ---- 64 seeds: one group, six groups, singletons
    seeds = 0xE7E70000 + np.arange(64, dtype=np.uint64)
    res = SimulationRunner(simulation_input=payload, seeds=seeds).run()
    names = res.series_names()
    per_window = int(round(2.0 / res.plan.sample_period))
    edges = tick_window_edges(per_window, res.plan.tick_count)
    thr = {names[0]: 0.5, next(k for k in names if k.endswith("ram_in_use")): 64.0}
    thr_vec = res._series_thresholds(thr)  # noqa: SLF001
    for by, ids, g in ((None, np.zeros(64, dtype=np.int64), 1), (np.arange(64) % 6, np.arange(64) % 6, 6)):
        a = res.series_window_summary(2.0, by=by, thresholds=thr)
        assert np.array_equal(a["tick_edges"], edges) and a["series"] == names and a["replicas"].tolist() == np.bincount(ids).tolist()
        assert np.array_equal(a["times"], edges[:-1] * res.plan.sample_period) and a["count"].dtype.is_floating_point is False
        _same(_api_as_numpy(a), _cells_on_the_host(res, ids, g, edges, thr_vec), f"by={by!r}")
        b = res.series_window_summary(ticks_per_window=per_window, by=by, thresholds=thr_vec)
        for k in ("count", "mean", "min_words", "max_words", "above"):
            assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
    a = res.series_window_summary(2.0, by="scenario")
    got = _api_as_numpy(a)
    for s in range(64):
        host = res[s].get_series_window_stats(2.0)
        _same({k: v[s:s + 1] for k, v in got.items()}, {k: v[None] for k, v in host.items()}, f"scenario {s}")
    # the decoded values: counts as they are, the ram columns from their float32 bits, NaN where the window is empty
    ram = ram_columns(len(names), res.plan.n_edges)
    cnt = a["count"].cpu().numpy()
    assert (cnt > 0).all()
    mx = a["max"].cpu().numpy()
    assert np.array_equal(mx[:, :, ~ram], got["max"][:, :, ~ram].astype(np.float64))
    assert np.array_equal(mx[:, :, ram], got["max"][:, :, ram].view(np.float32).astype(np.float64))
    assert np.array_equal(a["above_share"].cpu().numpy(), got["above"] / cnt[:, :, None])
    past = res.series_window_summary(tick_edges=[0, 5, res.plan.tick_count + 5, res.plan.tick_count + 9], by="scenario")
    for k in ("mean", "min", "max", "above_share"):
        assert np.isnan(past[k][:, 2].cpu().numpy()).all() and not np.isnan(past[k][:, :2].cpu().numpy()).any()
    assert (past["count"][:, 2] == 0).all() and (past["min_words"][:, 2] == 0).all()

    # ---- one window over the whole run is the per-scenario series summary
    whole = res.series_window_summary(tick_edges=[0, res.plan.tick_count], by="scenario")
    summ = res.summary(rps=False, series=True)
    assert whole["mean"][:, 0].cpu().numpy().tobytes() == summ["series_mean"].cpu().numpy().tobytes()
    assert np.array_equal(whole["max_words"][:, 0].cpu().numpy(), summ["series_max"].cpu().numpy())

    # ---- a 3 x 2 grid with 4 replicas: by=Sweep, bands over the replicas, the on-disk summary
    users = "rqs_input.avg_active_users.mean"
    grid = expand_grid({users: [40.0, 120.0, 300.0], "topology_graph.edges[*].latency.mean": [0.002, 0.006]},
                       replicas=4, order_by_load=users)
    res = SimulationRunner(simulation_input=payload, **grid.runner_kwargs()).run()
    a = res.series_window_summary(2.0, by=grid)
    assert tuple(a["mean"].shape) == (6, len(edges) - 1, len(names)) and a["replicas"].tolist() == [4] * 6
    _same(_api_as_numpy(a), _cells_on_the_host(res, grid.point, 6, edges), "by=grid")
    z = NormalDist().inv_cdf(0.95)
    edges_b = np.concatenate([edges, [edges[-1] + 40]])              # the last window lies past the run: no replica has a sample
    for of in ("mean", "max", "above_share"):
        bands = res.series_window_bands(tick_edges=edges_b, by=grid, of=of, level=0.9, q=(0.1, 0.75))
        per = res.series_window_summary(tick_edges=edges_b, by="scenario")
        values, counts = per[of].cpu().numpy(), per["count"].cpu().numpy()
        for g in range(6):
            members = np.nonzero(grid.point == g)[0]
            for w in range(len(edges_b) - 1):
                body = values[members, w][counts[members, w] > 0]
                assert bands["n"][g, w] == body.shape[0]
                if body.shape[0] == 0:
                    for k in ("mean", "std", "ci_halfwidth", "q_lo", "q_hi"):
                        assert np.isnan(bands[k][g, w]).all(), (k, g, w)
                    continue
                sd = body.std(axis=0, ddof=1)
                np.testing.assert_allclose(bands["mean"][g, w], body.mean(axis=0), rtol=1e-12, atol=0.0)
                np.testing.assert_allclose(bands["std"][g, w], sd, rtol=1e-12, atol=0.0)
                np.testing.assert_allclose(bands["ci_halfwidth"][g, w], z * sd / np.sqrt(body.shape[0]), rtol=1e-12, atol=0.0)
                np.testing.assert_allclose(bands["q_lo"][g, w], np.quantile(body, 0.1, axis=0), rtol=1e-12, atol=0.0)
                np.testing.assert_allclose(bands["q_hi"][g, w], np.quantile(body, 0.75, axis=0), rtol=1e-12, atol=0.0)
        assert (bands["n"][:, -1] == 0).all() and (bands["n"][:, :-1] == 4).all()
        pooled = res.series_window_summary(tick_edges=edges_b, by=grid)[of].cpu().numpy()
        assert np.array_equal(bands["pooled"], pooled, equal_nan=True) and np.isnan(bands["pooled"][:, -1]).all()
    with pytest.raises(ValueError, match="of must be"):
        res.series_window_bands(2.0, of="min")
    with pytest.raises(ValueError, match="by must be"):
        res.series_window_summary(2.0, by="point")

    res2 = SimulationRunner(simulation_input=lb_two_servers(horizon=10), seeds=seeds[:4], collect_samples=False).run()
    for call in (res2.series_window_summary, res2.series_window_bands):
        with pytest.raises(RuntimeError, match="kept no sampled series"):
            call()


def _round_trip(path: str) -> None:
    """save_series_window_summary of a 3 x 2 grid with 4 replicas, one row per point, read back by load_summary."""
    from asyncflow_amd import expand_grid
    from asyncflow_amd.results import load_summary
    from asyncflow_amd.runner import SimulationRunner

    users = "rqs_input.avg_active_users.mean"
    grid = expand_grid({users: [40.0, 120.0, 300.0], "topology_graph.edges[*].latency.mean": [0.002, 0.006]},
                       replicas=4, order_by_load=users)
    res = SimulationRunner(simulation_input=lb_with_events(horizon=60, scale=0.1), **grid.runner_kwargs()).run()
    names = res.series_names()
    edges = tick_window_edges(int(round(2.0 / res.plan.sample_period)), res.plan.tick_count)
    thr = {names[0]: 0.5, next(k for k in names if k.endswith("ram_in_use")): 64.0}
    pooled = res.series_window_summary(2.0, by=grid, thresholds=thr)
    bands = res.series_window_bands(2.0, by=grid, thresholds=thr, of="mean", q=(0.05, 0.95))
    written = res.save_series_window_summary(path, grid, window_s=2.0, thresholds=thr)
    back = load_summary(path)
    assert set(back) == set(written)
    for k, v in written.items():
        assert np.array_equal(np.asarray(back[k], dtype=v.dtype), v, equal_nan=v.dtype.kind == "f"), k
    for k, v in grid.point_columns().items():
        assert np.array_equal(back[f"param:{k}"], v)
    for j, sname in enumerate(names):
        for col, want in (("mean", pooled["mean"]), ("max", pooled["max"]), ("above", pooled["above_share"])):
            assert np.array_equal(back[f"series_window_{col}:{sname}"], want.cpu().numpy()[:, :, j], equal_nan=True), (col, sname)
        assert np.array_equal(back[f"series_window_q05:{sname}"], bands["q_lo"][:, :, j], equal_nan=True)
        assert np.array_equal(back[f"series_window_q95:{sname}"], bands["q_hi"][:, :, j], equal_nan=True)
        assert back[f"series_window_q95:{sname}"].shape == (6, len(edges) - 1)
    assert np.array_equal(back["series_window_tick_edges"], edges) and back["replicas"].tolist() == [4] * 6
    assert np.array_equal(back["series_window_times"], edges[:-1] * res.plan.sample_period)


def test_save_series_window_summary_npz(tmp_path):
    _round_trip(str(tmp_path / "series_windows.npz"))


def test_save_series_window_summary_parquet(tmp_path):
    pytest.importorskip("pyarrow")
    _round_trip(str(tmp_path / "series_windows.parquet"))


def test_many_singleton_cells():
    """2 000 LB-2 replicas at T = 600 s, 600 windows of 1 s, every replica its own group: 14.4 M (cell, series) entries, written
    by the streaming pass itself; no per-record scratch."""
    from asyncflow_amd.runner import SimulationRunner

    n = 2000
    seeds = 0xC0FFEE00 + np.arange(n, dtype=np.uint64)
    res = SimulationRunner(simulation_input=lb_two_servers(horizon=600), seeds=seeds, collect_clock=False).run()
    a = res.series_window_summary(1.0, by="scenario")
    S = res.plan.n_series
    assert tuple(a["mean"].shape) == (n, 600, S) and n * 600 * S == 14_400_000
    bound = _scratch_bound(n, n, 600, S, False)
    print(f"scratch_bytes {a['scratch_bytes']} bound {bound} series_window_ms {a['series_window_ms']:.2f}")
    assert 0 < a["scratch_bytes"] <= bound
    assert int(a["count"].sum()) == int(np.minimum(res.counts[:, _abi.CNT_TICKS], res.plan.tick_count).sum())
    got = _api_as_numpy(a)
    rng = np.random.default_rng(77)
    for s in rng.choice(n, 32, replace=False):
        host = res[int(s)].get_series_window_stats(1.0)
        _same({k: v[s:s + 1] for k, v in got.items()}, {k: v[None] for k, v in host.items()}, f"scenario {s}")
