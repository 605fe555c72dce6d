"""Latency by the state a request met on arrival, CPU side: the host definition (results.latency_state_cells /
latency_state_stats / latency_state_quantiles) against a plain per-row Python loop on hand-made clocks and samples with a dyadic
period, so that every quotient is exact; the per-scenario accessor; on the oracle's runs of four scenarios the cells are
populated; the two C entry points, their struct and their refusals."""

from __future__ import annotations

import ctypes as C
import math
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import asyncflow_amd
from asyncflow_amd import _abi
from asyncflow_amd import build as af_build
from asyncflow_amd.plan import lower
from asyncflow_amd.results import (
    ScenarioResults,
    ShardedResults,
    check_state_bins,
    latency_quantiles,
    latency_state_cells,
    latency_state_quantiles,
    latency_state_stats,
    latency_stats_row,
    latency_within,
    series_names_of,
)
from oracle.scenarios import lb_two_servers, lb_with_events, overload, single_server

ROOT = Path(__file__).resolve().parent.parent
P = 2.0 ** -5                      # the sample period: start / P is exact for every start below
N_EDGES = 1                        # the synthetic layout: one edge, one server -> columns edge, ready, io, ram
RAM_COL = 3
RESIDUE = np.float32(-(2.0 ** -45))
LEVELS = [0.0, 0.5, 0.95, 1.0]
THRESHOLDS = [0.25, 1.0]
FIELDS = ["column", "n_bins", "lo", "width", "sample_period"]


@pytest.fixture(scope="module")
def lib():
    af_build.build()
    from asyncflow_amd.engine import load_library

    return load_library()


def _same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _loop(clock, words, column, bins, lo, width, edges, period=P, n_edges=N_EDGES):
    """The definition, one row after the other in plain Python: {cell index: [latencies in row order]}."""
    n_series, ticks = words.shape
    is_ram = column >= n_edges and (column - n_edges) % 3 == 2
    cells: dict[int, list[float]] = {}
    for start, finish in np.asarray(clock, dtype=np.float64).reshape(-1, 2).tolist():
        if math.isnan(start) or start < 0.0:
            continue
        q = math.floor(start / period) if math.isfinite(start) else math.inf
        if q < 1 or q - 1 >= ticks:
            continue
        word = words[column, int(q) - 1]
        x = float(np.float32(word.view(np.float32))) if is_ram else float(int(word))
        if x < lo:
            continue
        t = (x - lo) / width
        b = bins - 1 if t >= bins else int(t)
        w = 0
        if edges is not None:
            hit = [k for k in range(len(edges) - 1) if edges[k] < start <= edges[k + 1]]
            if not hit:
                continue
            w = hit[0]
        cells.setdefault(w * bins + b, []).append(finish - start)
    return cells


def _check(clock, words, column, bins, lo=0.0, width=1.0, edges=None):
    got = latency_state_cells(clock, words, N_EDGES, P, column, bins, lo, width, edges)
    want = _loop(clock, words, column, bins, lo, width, edges)
    n_win = 1 if edges is None else len(edges) - 1
    assert len(got) == n_win * bins
    for c, lat in enumerate(got):
        assert lat.tolist() == want.get(c, []), (c, lat, want.get(c))
    stats = latency_state_stats(clock, words, N_EDGES, P, column, bins, lo, width, edges)
    assert _same_bits(stats, np.stack([latency_stats_row(x) for x in got]).reshape(n_win, bins, 8))
    cnt, quant, within = latency_state_quantiles(clock, words, N_EDGES, P, column, bins, LEVELS, THRESHOLDS, lo, width, edges)
    assert cnt.dtype == np.uint32 and cnt.shape == (n_win, bins) and cnt.ravel().tolist() == [x.size for x in got]
    assert _same_bits(quant, np.stack([latency_quantiles(x, LEVELS) for x in got]).reshape(n_win, bins, len(LEVELS)))
    assert _same_bits(within, np.stack([latency_within(x, THRESHOLDS) for x in got]).reshape(n_win, bins, len(THRESHOLDS)))
    return got


def _words(ticks: int) -> np.ndarray:
    """Four series over `ticks` ticks: an edge (0..2), a ready queue that climbs (k), an IO set (k % 5) and RAM (floats)."""
    k = np.arange(ticks, dtype=np.uint32)
    ram = (np.arange(ticks) % 7 * 0.5).astype(np.float32)
    return np.stack([k % 3, k, k % 5, ram.view(np.uint32)])


# ------------------------------------------------------------------------------------ the definition, row by row
def test_the_tick_of_a_row():
    words = _words(8)                                   # ticks 0 .. 7: samples taken at P, 2 P, ... 8 P
    # starts: below the period, exactly on k P, between two samples, on the last sample (k = t_s - 1), one past it (k = t_s)
    starts = [0.0, P / 2, 0.999 * P, P, 1.5 * P, 2 * P, 7.5 * P, 8 * P, 8.5 * P, 9 * P, 100.0]
    clock = np.array([[s, s + 2.0 ** -3 * (i + 1)] for i, s in enumerate(starts)])
    got = _check(clock, words, 1, 8)                    # the ready queue holds k: the bin IS the tick
    assert [x.tolist() for x in got] == [[2.0 ** -3 * 4, 2.0 ** -3 * 5], [2.0 ** -3 * 6], [], [], [], [], [2.0 ** -3 * 7],
                                         [2.0 ** -3 * 8, 2.0 ** -3 * 9]]
    # (P and 1.5 P -> sample 0; 2 P -> sample 1; 7.5 P -> sample 6; 8 P and 8.5 P -> sample 7 = t_s - 1; 9 P -> sample 8 = t_s: none)
    assert sum(x.size for x in got) == 6
    assert sum(x.size for x in _check(clock, words[:, :0], 1, 8)) == 0          # no sample row at all


def test_negative_nan_and_infinite_starts_have_no_state():
    words = _words(64)
    clock = np.array([[-1.0, 1.0], [np.nan, 1.0], [-0.0, 1.0], [np.inf, np.inf], [2 * P, 1.0], [-P, 2.0], [3 * P, 3 * P + 0.5]])
    got = _check(clock, words, 2, 5)
    assert [x.size for x in got] == [0, 1, 1, 0, 0]
    assert got[1].tolist() == [1.0 - 2 * P] and got[2].tolist() == [0.5]


def test_values_below_lo_and_the_overflow_bin():
    words = _words(40)
    starts = (np.arange(1, 41) * P)
    clock = np.stack([starts, starts + 0.5], axis=1)
    got = _check(clock, words, 1, 4, lo=3.0, width=2.0)      # values 0 .. 39: 0 .. 2 below lo; 3, 4 -> bin 0; ... >= 11 -> bin 3
    assert [x.size for x in got] == [2, 2, 2, 40 - 9]
    got = _check(clock, words, 1, 1, lo=0.0, width=0.25)     # one bin: everything at or above lo
    assert got[0].size == 40
    _check(clock, words, 1, 7, lo=-2.5, width=1.0 / 3.0)
    _check(clock, words, 0, 3, lo=1.0, width=0.1)


def test_a_ram_column_with_a_residue_and_a_negative_zero():
    ram = np.array([0.0, -0.0, RESIDUE, 1.5, 2.0 ** -45, 256.0, -1.0, 3.999], dtype=np.float32)
    words = np.stack([np.zeros(8, np.uint32), np.zeros(8, np.uint32), np.zeros(8, np.uint32), ram.view(np.uint32)])
    starts = np.arange(1, 9) * P
    clock = np.stack([starts, starts + np.arange(1, 9)], axis=1)
    got = _check(clock, words, RAM_COL, 4)
    # -0.0 is not below 0.0 (bin 0); the residue and -1.0 are; 256 overflows into the last bin
    assert [x.tolist() for x in got] == [[1.0, 2.0, 5.0], [4.0], [], [6.0, 8.0]]
    got = _check(clock, words, RAM_COL, 4, lo=float(RESIDUE))
    assert got[0].tolist() == [1.0, 2.0, 3.0, 5.0]
    # the same words read as an INTEGER series are huge counts: all in the overflow bin but the zero word
    ints = np.stack([ram.view(np.uint32)] * 4)
    got = _check(clock, ints, 1, 4)
    assert [x.size for x in got] == [1, 0, 0, 7]


def test_windows_by_arrival_time_and_the_order_inside_a_cell():
    words = _words(64)
    rng = np.random.default_rng(7)
    starts = rng.integers(0, 70 * 4, 400) / 4.0 * P          # also before the first sample and past the last
    clock = np.stack([starts, starts + rng.integers(0, 64, 400) / 64.0], axis=1)
    edges = [8 * P, 16 * P, 17 * P, 40 * P]                  # starts ON edges belong to the window that ends there
    got = _check(clock, words, 2, 5, edges=edges)
    assert sum(x.size for x in got) == np.count_nonzero((starts > edges[0]) & (starts <= edges[-1]) & (starts < 65 * P))
    _check(clock, words, 1, 6, lo=4.0, width=10.0, edges=[0.0, 1.0])
    _check(clock, words, RAM_COL, 3, edges=[0.25, 0.5, 1.0, 1.5])
    # row order inside a cell, although the starts are out of order
    clock = np.array([[3.5 * P, 3.5 * P + 1.0], [3.25 * P, 3.25 * P + 2.0 ** 53], [3 * P, 3 * P + 1.0], [9 * P, 9 * P + 0.25]])
    got = _check(clock, words, 1, 4)
    assert got[2].tolist() == [1.0, 2.0 ** 53, 1.0] and np.mean(got[2]) != np.mean(got[2][[0, 2, 1]])


# ------------------------------------------------------------------------------------ the per-scenario accessor
def _scenario(counts_completed, counts_ticks, clock, words):
    plan = lower(single_server(horizon=50, period=P))
    assert plan.n_edges == 3 and plan.n_series == 6 and plan.sample_period == P
    counts = np.zeros(_abi.CNT_SLOTS, dtype=np.uint32)
    counts[_abi.CNT_COMPLETED], counts[_abi.CNT_TICKS] = counts_completed, counts_ticks
    return plan, ScenarioResults(plan, counts, clock, words)


def test_the_accessor_takes_names_windows_levels_and_counts_above_the_capacities():
    rng = np.random.default_rng(3)
    ticks = 200
    words = rng.integers(0, 6, (6, ticks)).astype(np.uint32)
    words[5] = (rng.integers(0, 40, ticks) / 8.0).astype(np.float32).view(np.uint32)
    starts = rng.integers(0, 220 * 8, 500) / 8.0 * P
    clock = np.stack([starts, starts + rng.integers(1, 100, 500) / 128.0], axis=1)
    # counts above the capacities: the stored rows are what the accessor holds (BatchedResults.__getitem__ clamps them)
    plan, res = _scenario(900, 5000, clock, words)
    names = series_names_of(plan)
    assert names[4] == "srv-1:event_loop_io_sleep" and names[5] == "srv-1:ram_in_use" and len(names) == 6
    out = res.get_latency_by_state("srv-1:event_loop_io_sleep", bins=6)
    assert out["series"] == 4 and out["edges"] is None and out["bin_lo"].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0]
    assert _same_bits(out["stats"], latency_state_stats(clock, words, 3, P, 4, 6)) and out["stats"].shape == (1, 6, 8)
    assert out["count"].sum() == np.count_nonzero((starts >= P) & (starts < (ticks + 1) * P)) and "quantiles" not in out
    out = res.get_latency_by_state(5, bins=4, lo=0.5, width=1.25, window_s=2.0, levels=LEVELS, thresholds=THRESHOLDS)
    e = out["edges"]
    assert e[0] == 0.0 and e[1] == 2.0 and out["stats"].shape == (len(e) - 1, 4, 8)
    cnt, quant, within = latency_state_quantiles(clock, words, 3, P, 5, 4, LEVELS, THRESHOLDS, 0.5, 1.25, e)
    assert _same_bits(out["quantiles"], quant) and _same_bits(out["within"], within) and np.array_equal(out["count"], cnt)
    assert np.array_equal(out["share"][cnt > 0], within[cnt > 0] / cnt[cnt > 0][:, None].astype(np.float64))
    assert _same_bits(res.get_latency_by_state(5, bins=4, edges=[0.0, 1.0, 3.0])["stats"], latency_state_stats(clock, words, 3, P, 5, 4, edges=[0.0, 1.0, 3.0]))
    for bad, what in (("srv-9:ram_in_use", "unknown series"), (6, "series columns"), (-1, "series columns"), (1.5, "one name"), ([4], "one name")):
        with pytest.raises(ValueError, match=what):
            res.get_latency_by_state(bad)
    with pytest.raises(ValueError, match="not both"):
        res.get_latency_by_state(4, window_s=1.0, edges=[0.0, 1.0])
    with pytest.raises(RuntimeError, match="no sampled series"):
        ScenarioResults(plan, res.counts, clock, None).get_latency_by_state(4)


def test_validators_and_refusals():
    assert check_state_bins(8) == (8, 0.0, 1.0, None) and check_state_bins(np.int64(3), -1, 0.5, P) == (3, -1.0, 0.5, P)
    for bins in (0, -1, 2.5, True, None, "8"):
        with pytest.raises(ValueError, match="bins"):
            check_state_bins(bins)
    for width in (0.0, -1.0, np.nan, np.inf, None):
        with pytest.raises(ValueError, match="width"):
            check_state_bins(8, 0.0, width)
    for lo in (np.nan, np.inf, -np.inf, "x"):
        with pytest.raises(ValueError, match="lo"):
            check_state_bins(8, lo)
    for period in (0.0, -P, np.nan, np.inf):
        with pytest.raises(ValueError, match="sample_period"):
            check_state_bins(8, 0.0, 1.0, period)
    words = _words(8)
    clock = np.array([[P, 1.0]])
    with pytest.raises(ValueError, match="sample_period"):
        latency_state_cells(clock, words, N_EDGES, 0.0, 1, 4)
    with pytest.raises(ValueError, match="series columns"):
        latency_state_cells(clock, words, N_EDGES, P, 4, 4)
    with pytest.raises(ValueError, match="strictly increasing"):
        latency_state_cells(clock, words, N_EDGES, P, 1, 4, edges=[0.0, 0.0])
    with pytest.raises(ValueError, match=r"words \[n_series, ticks\]"):
        latency_state_cells(clock, words[0], N_EDGES, P, 0, 4)
    with pytest.raises(ValueError, match="levels"):
        latency_state_quantiles(clock, words, N_EDGES, P, 1, 4, [1.5])
    for name in ("state_summary", "state_quantile_summary", "save_state_summary"):
        with pytest.raises(NotImplementedError, match="several devices"):
            getattr(ShardedResults, name)(None)
    assert asyncflow_amd.latency_state_cells is latency_state_cells and asyncflow_amd.latency_state_stats is latency_state_stats
    assert asyncflow_amd.latency_state_quantiles is latency_state_quantiles


# ------------------------------------------------------------------------------------ the oracle's runs: the cells are populated
@pytest.mark.parametrize("name, payload", [("single_server", single_server()), ("lb_two_servers", lb_two_servers(horizon=20)),
                                           ("overload", overload(horizon=30)), ("lb_with_events", lb_with_events(horizon=60, scale=0.1))])
def test_oracle_runs_fill_the_cells(name, payload):
    from oracle import oracle_lib as ol

    plan = lower(payload)
    r = ol.simulate(plan, 12345)
    assert r.clock.shape[0] > 100 and r.samples.shape == (plan.n_series, r.ticks)
    names = series_names_of(plan)
    col = names.index(f"{plan.server_ids[0]}:event_loop_io_sleep")
    cells = latency_state_cells(r.clock, r.samples, plan.n_edges, plan.sample_period, col, 8)
    want = _loop(r.clock, r.samples, col, 8, 0.0, 1.0, None, period=plan.sample_period, n_edges=plan.n_edges)
    assert [x.tolist() for x in cells] == [want.get(c, []) for c in range(8)]
    in_cells, filled = sum(x.size for x in cells), sum(1 for x in cells if x.size)
    print(f"{name}: {in_cells} of {r.clock.shape[0]} stored rows in a cell, {filled} of 8 bins filled, mean latency per bin",
          [round(float(x.mean()), 3) if x.size else None for x in cells])
    assert in_cells >= 0.99 * r.clock.shape[0]              # conditions, not tolerances: the comparison is not vacuous
    assert filled >= 3
    # with windows the cells partition the rows that start inside them
    edges = np.linspace(0.0, float(plan.total_time), 5)
    parts = latency_state_cells(r.clock, r.samples, plan.n_edges, plan.sample_period, col, 8, edges=edges)
    assert sum(x.size for x in parts) == np.count_nonzero((r.clock[:, 0] > 0.0) & (r.clock[:, 0] >= plan.sample_period)
                                                          & (np.floor(r.clock[:, 0] / plan.sample_period) - 1 < r.ticks))
    for w in range(4):
        for b in range(8):
            assert set(parts[w * 8 + b].tolist()) <= set(cells[b].tolist())


# ------------------------------------------------------------------------------------ the entries and their struct
def test_header_declares_and_library_exports_the_entries(lib):
    header = (ROOT / "include" / "asyncflow_hip.h").read_text()
    for name, req in (("af_engine_summarize_state_windows", _abi.AfWindows), ("af_engine_summarize_state_quantiles", _abi.AfQuantiles)):
        assert re.search(rf"int\s+{name}\s*\(\s*af_engine_t\s*\*\s*\w+,\s*const\s+af_outputs_t\s*\*\s*\w+,\s*const\s+af_state_bins_t\s*\*", header)
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).argtypes[2] is C.POINTER(_abi.AfStateBins) and getattr(lib, name).argtypes[3] is C.POINTER(req)
    assert re.search(r"#define\s+AF_ABI_VERSION\s+7\b", header) and lib.af_abi_version() == 7
    for listing in ((ROOT / "asyncflow_amd" / "build.py").read_text(), (ROOT / "asyncflow_amd" / "jit.py").read_text()):
        assert '"af_state.hpp"' in listing
    assert (ROOT / "asyncflow_amd" / "csrc" / "af_state.hpp").exists()


def test_af_state_bins_layout_matches_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "a host C compiler is needed for the layout probe"
    assert [name for name, _ in _abi.AfStateBins._fields_] == FIELDS  # noqa: SLF001
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "asyncflow_hip.h"\n'
                   'int main(void) { printf("%zu", sizeof(af_state_bins_t));\n'
                   + "".join(f'printf(" %zu", offsetof(af_state_bins_t, {f}));\n' for f in FIELDS) + 'printf("\\n"); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run([cc, "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(_abi.AfStateBins), *(getattr(_abi.AfStateBins, f).offset for f in FIELDS)]
    body = re.search(r"typedef struct af_state_bins \{(.*?)\} af_state_bins_t;", (ROOT / "include" / "asyncflow_hip.h").read_text(), re.S)
    assert body and re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S)) == FIELDS


def test_state_entries_refuse_without_a_device(lib):
    from asyncflow_amd.engine import PLAN_ONLY, Engine, EngineUnavailableError

    eng = Engine(lower(lb_two_servers(horizon=20)), PLAN_ONLY)
    try:
        out = _abi.AfOutputs(4, None, 4, None, None)
        sb = _abi.AfStateBins(0, 8, 0.0, 1.0, 0.05)
        edges = (C.c_double * 3)(0.0, 1.0, 2.0)
        lv = (C.c_double * 1)(0.5)
        wreq = _abi.AfWindows(4, 1, 2, None, edges, None, None, 0.0, 0)
        qreq = _abi.AfQuantiles(4, 1, 2, None, edges, 1, lv, 0, None, None, None, None, 0.0, 0)
        for call, req in ((lib.af_engine_summarize_state_windows, wreq), (lib.af_engine_summarize_state_quantiles, qreq)):
            assert call(None, C.byref(out), C.byref(sb), C.byref(req)) == _abi.AF_ERR_INVALID
            assert call(eng._h, None, C.byref(sb), C.byref(req)) == _abi.AF_ERR_INVALID  # noqa: SLF001
            assert call(eng._h, C.byref(out), None, C.byref(req)) == _abi.AF_ERR_INVALID  # noqa: SLF001
            assert call(eng._h, C.byref(out), C.byref(sb), None) == _abi.AF_ERR_INVALID  # noqa: SLF001
            assert call(eng._h, C.byref(out), C.byref(sb), C.byref(req)) == _abi.AF_ERR_NO_DEVICE  # noqa: SLF001
            assert b"planning-only" in lib.af_last_error()
        kw = {"column": 0, "sample_period": 0.05, "clock_ptr": 0, "clock_capacity": 4, "samples_ptr": 0, "tick_capacity": 4, "counts_ptr": 0}
        with pytest.raises(EngineUnavailableError, match="planning-only"):
            eng.summarize_state_windows(4, 1, bins=8, stats_ptr=0, **kw)
        with pytest.raises(EngineUnavailableError, match="planning-only"):
            eng.summarize_state_quantiles(4, 1, [0.5], bins=8, edges=[0.0, 1.0], **kw)
        # a bad request never reaches the library
        for bad, what in (({"bins": 0}, "bins"), ({"bins": 8, "width": 0.0}, "width"), ({"bins": 8, "lo": np.nan}, "lo"),
                          ({"bins": 8, "edges": [0.0]}, "at least two")):
            with pytest.raises(ValueError, match=what):
                eng.summarize_state_windows(4, 1, stats_ptr=0, **{**kw, **bad})
        with pytest.raises(ValueError, match="sample_period"):
            eng.summarize_state_windows(4, 1, bins=8, stats_ptr=0, **{**kw, "sample_period": 0.0})
        with pytest.raises(ValueError, match="series columns"):
            eng.summarize_state_windows(4, 1, bins=8, stats_ptr=0, **{**kw, "column": 99})
        with pytest.raises(ValueError, match="at least one"):
            eng.summarize_state_quantiles(4, 1, [], bins=8, **kw)
    finally:
        eng.close()
