"""Sampled-series analyzer per window of ticks, CPU side: the C entry point and its struct, argument checks, and the host
definition (results.tick_window_edges / series_window_stats) that the device analyzer matches."""

from __future__ import annotations

import ctypes as C
import json
import math
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from asyncflow_amd import _abi
from asyncflow_amd import build as af_build
from asyncflow_amd.plan import lower
from asyncflow_amd.results import (BatchedResults, ScenarioResults, check_tick_edges, ram_columns, series_window_stats,
                                   tick_window_edges, ticks_per_window_of)
from oracle.analyzer_oracle import series_mean_max
from oracle.scenarios import lb_two_servers

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = sorted(p for p in (ROOT / "tests" / "golden").glob("*.npz") if "samples" in np.load(p).files)
#: the fixtures whose ram_in_use samples are not all multiples of 1/256: float means compared with math.fsum, not bit for bit
NOT_DYADIC = {"frac_ram_waiting_put_t20", "ram_put_deadlock_t20"}
assert len(GOLDEN) == 12 and NOT_DYADIC <= {p.stem for p in GOLDEN}, "the twelve fixtures with sampled series"


@pytest.fixture(scope="module")
def lib():
    af_build.build()
    from asyncflow_amd.engine import load_library

    return load_library()


def test_header_declares_and_library_exports_the_series_windows_entry(lib):
    header = (ROOT / "include" / "asyncflow_hip.h").read_text()
    assert re.search(r"int\s+af_engine_summarize_series_windows\s*\(\s*af_engine_t\s*\*", header)
    assert "af_engine_summarize_series_windows" in _abi.EXPORTED_SYMBOLS
    assert hasattr(lib, "af_engine_summarize_series_windows")
    assert lib.af_engine_summarize_series_windows.argtypes[2] is C.POINTER(_abi.AfSeriesWindows)
    assert lib.af_abi_version() == 7


def test_af_series_windows_layout_matches_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "a host C compiler is needed for the layout probe"
    fields = [name for name, _ in _abi.AfSeriesWindows._fields_]  # noqa: SLF001
    assert fields == ["n_scenarios", "n_groups", "n_windows", "group", "tick_edges", "thresholds", "count", "mean", "minv", "maxv",
                      "above", "elapsed_ms", "scratch_bytes"]
    src = tmp_path / "probe.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "asyncflow_hip.h"\n'
        'int main(void) { printf("%zu", sizeof(af_series_windows_t));\n'
        + "".join(f'printf(" %zu", offsetof(af_series_windows_t, {f}));\n' for f in fields)
        + 'printf(" %zu\\n", sizeof(af_windows_t)); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run([cc, "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    P = _abi.AfSeriesWindows
    assert got == [C.sizeof(P), *(getattr(P, f).offset for f in fields), C.sizeof(_abi.AfWindows)]


def test_series_windows_entry_refuses_bad_requests_without_a_device(lib):
    from asyncflow_amd.engine import PLAN_ONLY, Engine, EngineUnavailableError

    eng = Engine(lower(lb_two_servers(horizon=20)), PLAN_ONLY)
    try:
        out = _abi.AfOutputs(0, None, 4, None, None)
        edges = (C.c_uint32 * 3)(0, 1, 2)
        req = _abi.AfSeriesWindows(4, 1, 2, None, edges, None, None, None, None, None, None, 0.0, 0)
        call = lib.af_engine_summarize_series_windows
        assert call(None, C.byref(out), C.byref(req)) == _abi.AF_ERR_INVALID
        assert call(eng._h, None, C.byref(req)) == _abi.AF_ERR_INVALID  # noqa: SLF001
        assert call(eng._h, C.byref(out), None) == _abi.AF_ERR_INVALID  # noqa: SLF001
        assert call(eng._h, C.byref(out), C.byref(req)) == _abi.AF_ERR_NO_DEVICE  # noqa: SLF001
        assert b"planning-only" in lib.af_last_error()
        kw = {"samples_ptr": 0, "tick_capacity": 4, "counts_ptr": 0, "count_ptr": 0, "mean_ptr": 0}
        with pytest.raises(EngineUnavailableError, match="planning-only"):
            eng.summarize_series_windows(4, 1, [0, 2, 4], **kw)
        # bad tick_edges and thresholds never reach the library
        for bad, what in (([0], "at least two"), ([0, 2, 2], "strictly increasing"), ([3, 1], "strictly increasing"),
                          ([0.5, 2], "whole"), ([-1, 2], r"\[0, 2\^32\)"), ([[0, 1]], "at least two")):
            with pytest.raises(ValueError, match=what):
                eng.summarize_series_windows(4, 1, bad, **kw)
        with pytest.raises(ValueError, match="NaN"):
            eng.summarize_series_windows(4, 1, [0, 4], thresholds=[float("nan")] * 12, **kw)
        with pytest.raises(ValueError, match="one value per series"):
            eng.summarize_series_windows(4, 1, [0, 4], thresholds=[0.0] * 5, **kw)
    finally:
        eng.close()


def _fixture(path: Path):
    z = np.load(path)
    plan = lower(json.loads(str(z["payload_json"])))
    words = np.ascontiguousarray(z["samples"]).view(np.uint32)
    counts = np.zeros(_abi.CNT_SLOTS, dtype=np.uint32)
    counts[_abi.CNT_TICKS] = words.shape[1]
    return plan, words, ScenarioResults(plan, counts, np.zeros((0, 2)), words)


def _float_order(word: int) -> tuple[float, int]:
    """Sorts the words of float32 values (no NaN) by value, -0.0 before +0.0."""
    x = float(np.uint32(word).view(np.float32))
    return (x, 0 if word >> 31 else 1)


def _by_loops(words: np.ndarray, edges, n_edges: int, thr: np.ndarray):
    """The definition stated independently: a loop over windows and series with slices, numpy's mean on the int64 values /
    on the float32 values as float64, min and max of the 4-byte words of an integer series, of a ram_in_use series the
    words of its smallest and largest float value (-0.0 below +0.0), a boolean count.  Also math.fsum / n for the float
    columns."""
    n_series, ticks = words.shape
    n_win = len(edges) - 1
    count = np.zeros(n_win, dtype=np.int64)
    mean = np.full((n_win, n_series), np.nan)
    fsum_mean = np.full((n_win, n_series), np.nan)
    mn, mx, above = (np.zeros((n_win, n_series), dtype=np.uint32) for _ in range(3))
    for w in range(n_win):
        lo, hi = min(int(edges[w]), ticks), min(int(edges[w + 1]), ticks)
        count[w] = hi - lo
        if hi == lo:
            continue
        for j in range(n_series):
            col = words[j, lo:hi]
            if j >= n_edges and (j - n_edges) % 3 == 2:
                vals = col.view(np.float32).astype(np.float64)
                mean[w, j] = np.mean(vals)
                fsum_mean[w, j] = math.fsum(vals.tolist()) / (hi - lo)
                mn[w, j], mx[w, j] = min(col.tolist(), key=_float_order), max(col.tolist(), key=_float_order)
            else:
                vals = col.astype(np.int64)
                mean[w, j] = np.mean(vals)
                mn[w, j], mx[w, j] = min(col.tolist()), max(col.tolist())
            above[w, j] = np.count_nonzero(vals > thr[j])
    return count, mean, fsum_mean, mn, mx, above


def _thresholds(words: np.ndarray, n_edges: int) -> np.ndarray:
    """One threshold per series that occurs in the data (the strictly-greater rule decides), 0.5 on the first column."""
    ram = ram_columns(words.shape[0], n_edges)
    thr = np.zeros(words.shape[0])
    for j in range(words.shape[0]):
        vals = words[j].view(np.float32).astype(np.float64) if ram[j] else words[j].astype(np.float64)
        thr[j] = np.median(vals) if vals.size else 0.0
    thr[0] = 0.5
    return thr


@pytest.mark.parametrize("path", GOLDEN, ids=[p.stem for p in GOLDEN])
def test_series_window_stats_on_every_fixture(path):
    plan, words, res = _fixture(path)
    n_series, ticks = words.shape
    assert n_series == plan.n_series
    ram = ram_columns(n_series, plan.n_edges)
    uneven = [3, 4, 10, 11, ticks // 2, ticks - 1, ticks + 7, ticks + 20, ticks + 21]
    cases = [tick_window_edges(m, ticks) for m in (1, 20, 200, ticks)] + [np.asarray(uneven)]
    for edges in cases:
        for thr in (None, _thresholds(words, plan.n_edges)):
            got = series_window_stats(words, edges, plan.n_edges, thr)
            count, mean, fsum_mean, mn, mx, above = _by_loops(words, edges, plan.n_edges, np.zeros(n_series) if thr is None else thr)
            assert np.array_equal(got["count"], count) and got["mean"].shape == (len(edges) - 1, n_series)
            assert np.array_equal(got["min"], mn) and np.array_equal(got["max"], mx) and np.array_equal(got["above"], above)
            assert got["min"].dtype == got["max"].dtype == got["above"].dtype == np.uint32
            assert np.array_equal(got["mean"][:, ~ram].view(np.uint64), mean[:, ~ram].view(np.uint64))
            if path.stem not in NOT_DYADIC:
                assert np.array_equal(got["mean"][:, ram].view(np.uint64), mean[:, ram].view(np.uint64))
            else:
                tol = count[:, None] * 2.0 ** -52 * np.abs(fsum_mean[:, ram])
                assert count.max() <= 4096
                ok = np.abs(got["mean"][:, ram] - fsum_mean[:, ram]) <= tol
                assert (ok | (count == 0)[:, None]).all()
            assert np.isnan(got["mean"][count == 0]).all() and not np.isnan(got["mean"][count > 0]).any()
    assert cases[-1][0] > 0 and cases[-1][-1] > ticks
    got = series_window_stats(words, cases[-1], plan.n_edges)
    assert got["count"].tolist() == [1, 6, 1, ticks // 2 - 11, ticks - 1 - ticks // 2, 1, 0, 0]
    # the accessor: seconds, ticks and explicit edges agree; the default is 1-s windows
    per_s = ticks_per_window_of(1.0, plan.sample_period)
    a = res.get_series_window_stats()
    b = res.get_series_window_stats(ticks_per_window=per_s)
    c = res.get_series_window_stats(tick_edges=tick_window_edges(per_s, plan.tick_count))
    for k in ("count", "mean", "min", "max", "above"):
        assert np.array_equal(a[k], b[k], equal_nan=True) and np.array_equal(a[k], c[k], equal_nan=True)
    assert a["count"].sum() == ticks and a["count"].shape[0] == -(-plan.tick_count // per_s)


@pytest.mark.parametrize("path", GOLDEN, ids=[p.stem for p in GOLDEN])
def test_one_window_is_the_whole_run_summary(path):
    plan, words, _ = _fixture(path)
    n_series, ticks = words.shape
    ram = ram_columns(n_series, plan.n_edges)
    whole = series_window_stats(words, [0, ticks], plan.n_edges)
    mean, mx = series_mean_max(words, plan.n_edges)
    # (frac_ram_waiting_put_t20 holds 179 ram samples of -2.8e-14, float residue of the reference's own arithmetic: as WORDS
    # they are the largest of their column, as VALUES the smallest; the oracle, af_engine_summarize's series_max and the
    # windows all take the float maximum)
    signed = (words >> 31).any(axis=1)
    assert signed.sum() == (1 if path.stem == "frac_ram_waiting_put_t20" else 0) and not signed[~ram].any()
    assert np.array_equal(whole["max"][0], mx)
    values = words.astype(np.float64)
    values[ram] = words[ram].view(np.float32).astype(np.float64)
    decode = lambda w: np.where(ram, w.view(np.float32).astype(np.float64), w.astype(np.float64))  # noqa: E731
    assert np.array_equal(decode(whole["max"][0]), values.max(axis=1)) and np.array_equal(decode(whole["min"][0]), values.min(axis=1))
    assert np.array_equal(whole["max"][0, ~signed], words.max(axis=1)[~signed])
    assert np.array_equal(whole["min"][0, ~signed], words.min(axis=1)[~signed])
    assert (whole["max"][0, signed] < words.max(axis=1)[signed]).all() and (whole["min"][0, signed] == words.max(axis=1)[signed]).all()
    exact = ~ram if path.stem in NOT_DYADIC else np.ones(n_series, dtype=bool)
    assert np.array_equal(whole["mean"][0, exact].view(np.uint64), mean[exact].view(np.uint64))
    np.testing.assert_allclose(whole["mean"][0], mean, rtol=ticks * 2.0 ** -52)
    # the windows partition the run: count-weighted means add up to the series' total, exactly for the integer series
    for m in (1, 20, 200):
        st = series_window_stats(words, tick_window_edges(m, ticks), plan.n_edges)
        total = words[~ram].astype(np.int64).sum(axis=1)
        parts = np.rint(st["count"][:, None].astype(np.float64) * st["mean"][:, ~ram]).astype(np.int64)
        assert np.array_equal(parts, np.add.reduceat(words[~ram].astype(np.int64), np.arange(0, ticks, m), axis=1).T)
        assert np.array_equal(parts.sum(axis=0), total)
        assert np.array_equal(decode(st["max"]).max(axis=0), decode(whole["max"][0]))       # (as values: the windows' float maxima)
        assert np.array_equal(st["max"].max(axis=0)[~signed], whole["max"][0, ~signed])
        assert np.array_equal(st["above"].sum(axis=0), whole["above"][0])


def test_series_window_stats_of_signed_ram_values():
    """Hand-made columns: min / max of a ram_in_use column are the float minimum / maximum as float32 bits, -0.0 below +0.0;
    an integer column keeps the order of its words, the sign bit included."""
    n_edges = 1                                                          # series: one edge, then one server's queue, sleep, ram
    f = lambda *v: np.array(v, dtype=np.float32).view(np.uint32)  # noqa: E731
    ram = f(1.5, -2.0, 0.25,   -3.0, -0.5, -7.25,   0.0, -0.0, 0.0,   -0.0, -1.0, -0.0,   -0.0, 0.0, 2.0,   -2.0 ** -45, 300.5, 0.0)
    edge = np.array([3, 0x80000001, 7] + [5] * 15, dtype=np.uint32)
    words = np.stack([edge, np.arange(18, dtype=np.uint32), np.zeros(18, dtype=np.uint32), ram])
    thr = np.array([4.0, 0.0, 0.0, -0.0])
    st = series_window_stats(words, [0, 3, 6, 9, 12, 15, 18, 40, 41], n_edges, thr)
    assert st["count"].tolist() == [3, 3, 3, 3, 3, 3, 0, 0]
    bits = lambda x: int(np.float32(x).view(np.uint32))  # noqa: E731
    #                              mixed      all negative  zeros      max is -0.0  -0.0 lowest  a residue      empty
    assert st["max"][:, 3].tolist() == [bits(1.5), bits(-0.5), bits(0.0), bits(-0.0), bits(2.0), bits(300.5), 0, 0]
    assert st["min"][:, 3].tolist() == [bits(-2.0), bits(-7.25), bits(-0.0), bits(-1.0), bits(-0.0), bits(-2.0 ** -45), 0, 0]
    assert bits(-0.0) == 0x80000000 and bits(0.0) == 0
    assert st["above"][:, 3].tolist() == [2, 0, 0, 0, 1, 1, 0, 0]         # (> -0.0 as f64: +0.0 is not above it)
    assert st["mean"][:6, 3].tolist() == [-0.25 / 3, -10.75 / 3, 0.0, -1.0 / 3, 2.0 / 3, (300.5 - 2.0 ** -45) / 3] and np.isnan(st["mean"][6:]).all()
    assert st["max"][:, 0].tolist() == [0x80000001, 5, 5, 5, 5, 5, 0, 0] and st["min"][:, 0].tolist() == [3, 5, 5, 5, 5, 5, 0, 0]
    assert st["above"][:, 0].tolist() == [2, 3, 3, 3, 3, 3, 0, 0]
    # the plain float reference over every window of every width
    values = ram.view(np.float32).astype(np.float64)
    for m in (1, 2, 5, 18):
        st = series_window_stats(words, tick_window_edges(m, 18), n_edges)
        for w in range(-(-18 // m)):
            seg, raw = values[m * w:m * (w + 1)], ram[m * w:m * (w + 1)]
            got_max, got_min = (st[k][w, 3:4].view(np.float32)[0] for k in ("max", "min"))
            assert got_max == seg.max() and got_min == seg.min()
            if seg.max() == 0:
                assert np.signbit(got_max) == bool((raw[seg == 0] == 0x80000000).all())      # +0.0 if there is one
            if seg.min() == 0:
                assert np.signbit(got_min) == bool((raw[seg == 0] == 0x80000000).any())      # -0.0 if there is one


def test_series_windows_show_the_spike_of_the_event_fixture():
    # lb2_events_t60: a network spike on client-lb from 10 s to 16 s: messages stay longer on the edge
    plan, _, res = _fixture(ROOT / "tests" / "golden" / "lb2_events_t60.npz")
    st = res.get_series_window_stats(2.0)
    j = list(plan.edge_ids).index("client-lb")
    conc = st["mean"][:, j]
    before, during = conc[0:5], conc[5:8]          # windows labelled 0-2 .. 8-10 s and 10-12 .. 14-16 s
    print("edge_concurrent_connection of client-lb per 2-s window before the spike:", before, "during:", during)
    assert during.min() > before.max()


def test_window_arguments_are_checked():
    plan, words, res = _fixture(ROOT / "tests" / "golden" / "lb2_rr_t30.npz")
    assert ticks_per_window_of(1.0, 0.05) == 20 and ticks_per_window_of(0.01, 0.01) == 1 and ticks_per_window_of(2.5, 0.05) == 50
    for bad in (0.33, 0.004, 1.02):
        with pytest.raises(ValueError, match="multiple of the sample period"):
            ticks_per_window_of(bad, 0.05)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="window_s"):
            ticks_per_window_of(bad, 0.05)
    with pytest.raises(ValueError, match="multiple of the sample period"):
        res.get_series_window_stats(0.33)
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError, match="ticks_per_window"):
            res.get_series_window_stats(ticks_per_window=bad)
    assert tick_window_edges(20, 599).tolist() == [20 * k for k in range(31)] and tick_window_edges(20, 600)[-1] == 600
    assert tick_window_edges(7, 0).tolist() == [0, 7] and tick_window_edges(20, 599).dtype == np.uint32
    for kw in ({"window_s": 1.0, "ticks_per_window": 20}, {"window_s": 1.0, "tick_edges": [0, 5]}, {"ticks_per_window": 20, "tick_edges": [0, 5]}):
        with pytest.raises(ValueError, match="one of"):
            res.get_series_window_stats(**kw)
    for bad, what in (([0, 2, 2], "strictly increasing"), ([5], "at least two"), ([0, 1.5], "whole"), ([0, 2 ** 32], r"\[0, 2\^32\)")):
        with pytest.raises(ValueError, match=what):
            check_tick_edges(bad)
    nan_thr = np.zeros(words.shape[0])
    nan_thr[3] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        series_window_stats(words, [0, 5], plan.n_edges, nan_thr)
    with pytest.raises(ValueError, match="NaN"):
        res.get_series_window_stats(thresholds=nan_thr)
    # the thresholds of a batch: a vector or names out of series_names()
    batch = BatchedResults.__new__(BatchedResults)
    batch.plan = plan
    names = batch.series_names()
    thr = batch._series_thresholds({names[2]: 1.5, names[-1]: 64.0})  # noqa: SLF001
    assert thr.tolist() == [0.0, 0.0, 1.5] + [0.0] * (len(names) - 4) + [64.0]
    assert batch._series_thresholds(None) is None  # noqa: SLF001
    with pytest.raises(ValueError, match="unknown series"):
        batch._series_thresholds({"nobody:ram_in_use": 1.0})  # noqa: SLF001
    with pytest.raises(ValueError, match="NaN"):
        batch._series_thresholds({names[0]: float("nan")})  # noqa: SLF001
    with pytest.raises(ValueError, match="one value per series"):
        batch._series_thresholds([0.0, 1.0])  # noqa: SLF001
    none = ScenarioResults(plan, res.counts, np.zeros((0, 2)), None)
    with pytest.raises(RuntimeError, match="kept no sampled series"):
        none.get_series_window_stats()


def test_sharded_results_refuse_series_windows():
    from asyncflow_amd.results import ShardedResults

    sh = ShardedResults.__new__(ShardedResults)
    for call in (sh.series_window_summary, sh.series_window_bands, sh.save_series_window_summary):
        with pytest.raises(NotImplementedError, match="several devices"):
            call(1.0)
