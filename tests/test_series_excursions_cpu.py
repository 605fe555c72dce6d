"""Excursions of the sampled series above a threshold, CPU side: the C entry point and its struct, the host definition
(results.series_window_excursions) against a naive loop over runs, identities with series_window_stats, and the refusals of
the Python layer."""

from __future__ import annotations

import ctypes as C
import itertools
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import asyncflow_amd
from asyncflow_amd import _abi
from asyncflow_amd import build as af_build
from asyncflow_amd import results as af_results
from asyncflow_amd.plan import lower
from asyncflow_amd.results import BatchedResults, ScenarioResults, series_window_excursions, series_window_stats, tick_window_edges
from oracle.scenarios import lb_two_servers

ROOT = Path(__file__).resolve().parent.parent
KEYS = ("above", "runs", "longest", "longest_start", "first", "last", "peak_tick")
N_EDGES = 1                                   # the synthetic scenario: one edge, then one server's queue, sleep, ram
RESIDUE = np.float32(-(2.0 ** -45))


@pytest.fixture(scope="module")
def lib():
    af_build.build()
    from asyncflow_amd.engine import load_library

    return load_library()


def test_header_declares_and_library_exports_the_series_excursions_entry(lib):
    header = (ROOT / "include" / "asyncflow_hip.h").read_text()
    assert re.search(r"int\s+af_engine_summarize_series_excursions\s*\(\s*af_engine_t\s*\*", header)
    assert re.search(r"#define\s+AF_TICK_NONE\s+0xFFFFFFFFu", header)
    assert "af_engine_summarize_series_excursions" in _abi.EXPORTED_SYMBOLS
    assert hasattr(lib, "af_engine_summarize_series_excursions")
    assert lib.af_engine_summarize_series_excursions.argtypes[2] is C.POINTER(_abi.AfSeriesExcursions)
    assert lib.af_engine_summarize_series_excursions.argtypes[1] is C.POINTER(_abi.AfOutputs)
    assert lib.af_engine_summarize_series_excursions.restype is C.c_int
    assert lib.af_abi_version() == 7 and _abi.TICK_NONE == 0xFFFFFFFF
    assert asyncflow_amd.series_window_excursions is af_results.series_window_excursions
    assert "series_window_excursions" in asyncflow_amd.__all__


def test_af_series_excursions_layout_matches_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "a host C compiler is needed for the layout probe"
    fields = [name for name, _ in _abi.AfSeriesExcursions._fields_]  # noqa: SLF001
    assert fields == ["n_scenarios", "n_windows", "tick_edges", "thresholds", "count", "above", "runs", "longest", "longest_start",
                      "first", "last", "peak_tick", "elapsed_ms", "scratch_bytes"]
    src = tmp_path / "probe.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "asyncflow_hip.h"\n'
        'int main(void) { printf("%zu", sizeof(af_series_excursions_t));\n'
        + "".join(f'printf(" %zu", offsetof(af_series_excursions_t, {f}));\n' for f in fields)
        + 'printf(" %zu %u\\n", sizeof(af_series_windows_t), AF_TICK_NONE); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run([cc, "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    P = _abi.AfSeriesExcursions
    assert got == [C.sizeof(P), *(getattr(P, f).offset for f in fields), C.sizeof(_abi.AfSeriesWindows), _abi.TICK_NONE]


def test_series_excursions_entry_refuses_without_a_device(lib):
    from asyncflow_amd.engine import PLAN_ONLY, Engine, EngineUnavailableError

    eng = Engine(lower(lb_two_servers(horizon=20)), PLAN_ONLY)
    try:
        out = _abi.AfOutputs(0, None, 4, None, None)
        edges = (C.c_uint32 * 3)(0, 1, 2)
        req = _abi.AfSeriesExcursions(4, 2, edges, None, None, None, None, None, None, None, None, None, 0.0, 0)
        call = lib.af_engine_summarize_series_excursions
        assert call(None, C.byref(out), C.byref(req)) == _abi.AF_ERR_INVALID
        assert call(eng._h, None, C.byref(req)) == _abi.AF_ERR_INVALID  # noqa: SLF001
        assert call(eng._h, C.byref(out), None) == _abi.AF_ERR_INVALID  # noqa: SLF001
        assert call(eng._h, C.byref(out), C.byref(req)) == _abi.AF_ERR_NO_DEVICE  # noqa: SLF001
        assert b"planning-only" in lib.af_last_error()
        kw = {"samples_ptr": 0, "tick_capacity": 4, "counts_ptr": 0}
        with pytest.raises(EngineUnavailableError, match="planning-only"):
            eng.summarize_series_excursions(4, [0, 2, 4], **kw)
        # bad tick_edges and thresholds never reach the library
        for bad, what in (([0], "at least two"), ([0, 2, 2], "strictly increasing"), ([3, 1], "strictly increasing"), ([0.5, 2], "whole")):
            with pytest.raises(ValueError, match=what):
                eng.summarize_series_excursions(4, bad, **kw)
        with pytest.raises(ValueError, match="NaN"):
            eng.summarize_series_excursions(4, [0, 4], thresholds=[float("nan")] * 12, **kw)
        with pytest.raises(ValueError, match="one value per series"):
            eng.summarize_series_excursions(4, [0, 4], thresholds=[0.0] * 5, **kw)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------ the host definition against a naive loop
def _float_order(word: int) -> tuple[float, int]:
    """Orders the words of float32 values (no NaN) by value, -0.0 before +0.0."""
    return (float(np.uint32(word).view(np.float32)), 0 if word >> 31 else 1)


def _naive(words: np.ndarray, edges, n_edges: int, thr) -> dict[str, np.ndarray]:
    """The definition in plain Python: per window and series the list of above flags, itertools.groupby for the runs, max()
    -- which returns the FIRST of equal maxima -- for the longest run and for the peak."""
    n_series, ticks = words.shape
    n_win = len(edges) - 1
    out = {k: np.zeros((n_win, n_series), dtype=np.int64) for k in KEYS}
    out["count"] = np.zeros(n_win, dtype=np.int64)
    for w in range(n_win):
        lo, hi = min(int(edges[w]), ticks), min(int(edges[w + 1]), ticks)
        out["count"][w] = hi - lo
        for j in range(n_series):
            col = [int(x) for x in words[j, lo:hi]]
            is_ram = j >= n_edges and (j - n_edges) % 3 == 2
            values = [float(np.uint32(x).view(np.float32)) if is_ram else float(x) for x in col]
            flags = [v > float(thr[j]) for v in values]
            runs, k = [], lo
            for flag, grp in itertools.groupby(flags):
                length = len(list(grp))
                if flag:
                    runs.append((k, length))
                k += length
            best = max(runs, key=lambda r: r[1]) if runs else (-1, 0)
            out["above"][w, j] = sum(flags)
            out["runs"][w, j] = len(runs)
            out["longest"][w, j], out["longest_start"][w, j] = best[1], best[0]
            out["first"][w, j] = runs[0][0] if runs else -1
            out["last"][w, j] = runs[-1][0] + runs[-1][1] - 1 if runs else -1
            order = (lambda i: _float_order(col[i])) if is_ram else (lambda i: col[i])
            out["peak_tick"][w, j] = lo + max(range(hi - lo), key=order) if hi > lo else -1
    return out


def _agree(words, edges, n_edges, thr, what):
    got = series_window_excursions(words, edges, n_edges, thr)
    want = _naive(words, edges, n_edges, np.zeros(words.shape[0]) if thr is None else thr)
    assert set(got) == {"count", *KEYS}
    for k in ("count", *KEYS):
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    return got


def _synthetic(rng, ticks: int) -> np.ndarray:
    """Words [4, ticks] of (edge, ready queue, io sleep, ram): small integers that cross their thresholds in runs of every
    length, ram values in MB with zeros of either sign and the -2^-45 residue among them."""
    edge = rng.integers(0, 4, ticks).astype(np.uint32)
    ready = np.resize(np.repeat(rng.integers(0, 9, ticks // 5 + 1), rng.integers(1, 9, ticks // 5 + 1)), ticks).astype(np.uint32)
    io = rng.integers(0, 2, ticks).astype(np.uint32)
    ram = rng.choice(np.array([0.0, -0.0, RESIDUE, 64.0, 128.0, 128.0, 256.5], dtype=np.float32), ticks)
    return np.stack([edge, ready, io, ram.view(np.uint32)])


def _windows(ticks: int):
    return [("one", np.array([0, max(ticks, 1)])), ("one tick each", np.arange(max(ticks, 1) + 1)), ("7 ticks", tick_window_edges(7, ticks)),
            ("uneven", np.array([k for k in (1, 2, 5, 6, 40, 63, 64, 66) if k < ticks + 3] + [ticks + 3, ticks + 4, 3 * ticks + 70]))]


@pytest.mark.parametrize("ticks", [0, 1, 2, 63, 64, 65, 300])
def test_host_definition_equals_the_naive_loop(ticks):
    rng = np.random.default_rng(100 + ticks)
    words = _synthetic(rng, ticks)
    assert words.shape == (4, ticks)
    for what, edges in _windows(ticks):
        for thr in (None, np.array([1.0, 4.0, 0.5, 100.0]), np.array([2.5, 0.0, 0.0, -0.0])):
            got = _agree(words, edges, N_EDGES, thr, f"{ticks} ticks, {what}")
            assert got["count"].sum() <= ticks and (got["count"][np.asarray(edges[:-1]) >= ticks] == 0).all()
            empty = got["count"] == 0
            assert (got["above"][empty] == 0).all() and (got["runs"][empty] == 0).all() and (got["longest"][empty] == 0).all()
            for k in ("longest_start", "first", "last", "peak_tick"):
                assert (got[k][empty] == -1).all()
            assert (got["peak_tick"][~empty] >= 0).all()
    if ticks == 300:
        assert _windows(ticks)[-1][1][-1] > ticks and series_window_excursions(words, _windows(ticks)[-1][1], N_EDGES)["count"][-1] == 0


def test_signed_zeros_and_residues_against_both_zero_thresholds():
    f = lambda *v: np.array(v, dtype=np.float32).view(np.uint32)  # noqa: E731
    ram = f(0.0, -0.0, RESIDUE, 0.0, 1.0, -0.0, 2.0, 2.0, RESIDUE, -0.0, -0.0, 0.0)
    words = np.stack([np.zeros(12, dtype=np.uint32)] * 3 + [ram])
    for thr in (0.0, -0.0):                                              # as f64 the two thresholds compare alike
        t = np.array([0.0, 0.0, 0.0, thr])
        got = _agree(words, [0, 12], N_EDGES, t, f"threshold {thr!r}")
        # +0.0 is not above -0.0 (nor -0.0 above +0.0), the residue is not above 0.0: ticks 4, 6, 7 only
        assert [got[k][0, 3] for k in KEYS[:6]] == [3, 2, 2, 6, 4, 7]
        assert got["peak_tick"][0, 3] == 6                               # (2.0 at ticks 6 and 7: the first)
    # the peak of zeros and residues only: +0.0 above -0.0 above the residue, the first +0.0 wins
    quiet = np.stack([np.zeros(5, dtype=np.uint32)] * 3 + [f(RESIDUE, -0.0, 0.0, -0.0, 0.0)])
    got = _agree(quiet, [0, 5, 9], N_EDGES, None, "zeros")
    assert got["peak_tick"][:, 3].tolist() == [2, -1] and got["above"][0, 3] == 0 and got["first"][0, 3] == -1
    got = _agree(quiet[:, [0, 1, 3]], [0, 3], N_EDGES, None, "no +0.0")
    assert got["peak_tick"][0, 3] == 1                                   # (-0.0 at ticks 1 and 2: the first; the residue is below)
    # a threshold below the residue: every tick above, one run, open at the window's end
    got = _agree(quiet, [0, 2, 5], N_EDGES, np.array([0.0, 0.0, 0.0, -1.0]), "below the residue")
    assert got["runs"][:, 3].tolist() == [1, 1] and got["longest"][:, 3].tolist() == [2, 3] and got["last"][:, 3].tolist() == [1, 4]
    assert got["longest_start"][:, 3].tolist() == [0, 2]                 # (one run of five ticks, clipped: counted in both windows)


def test_ties_for_the_longest_run_and_for_the_peak():
    ready = np.array([0, 5, 5, 0, 9, 9, 0, 0, 9, 9, 0, 5, 5, 5, 0, 7, 7, 7], dtype=np.uint32)
    words = np.stack([np.zeros(18, dtype=np.uint32), ready, np.zeros(18, dtype=np.uint32), (ready.astype(np.float32) * 0.5).view(np.uint32)])
    thr = np.array([0.0, 4.0, 0.0, 2.0])
    got = _agree(words, [0, 11, 18, 30], N_EDGES, thr, "ties")
    for j in (1, 3):                                                      # the integer column and the ram column alike
        assert got["runs"][:, j].tolist() == [3, 2, 0] and got["longest"][:, j].tolist() == [2, 3, 0]
        assert got["longest_start"][:, j].tolist() == [1, 11, -1]         # three runs of 2 / two runs of 3: the earliest
        assert got["peak_tick"][:, j].tolist() == [4, 15, -1]             # 9 at ticks 4, 5, 8, 9 / 7 at 15, 16, 17: the first
        assert got["first"][:, j].tolist() == [1, 11, -1] and got["last"][:, j].tolist() == [9, 17, -1]
    assert got["last"][1, 1] == 18 - 1                                    # still above at the end of the window: open


# ------------------------------------------------------------------------------------ identities on random input
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_cross_identities_on_random_input(seed):
    rng = np.random.default_rng(seed)
    n_edges, n_series, ticks = 3, 12, 500
    ram = af_results.ram_columns(n_series, n_edges)
    words = rng.integers(0, 6, (n_series, ticks)).astype(np.uint32)
    words[ram] = rng.choice(np.array([-1.5, -0.0, 0.0, RESIDUE, 3.0, 8.25], dtype=np.float32), (int(ram.sum()), ticks)).view(np.uint32)
    thr = np.where(ram, rng.choice([-0.0, 0.0, 2.0], n_series), rng.integers(0, 5, n_series).astype(np.float64))
    for edges in (np.array([0, ticks]), tick_window_edges(7, ticks), tick_window_edges(64, ticks), np.array([4, 9, 100, 499, 500, 620])):
        got = series_window_excursions(words, edges, n_edges, thr)
        stats = series_window_stats(words, edges, n_edges, thr)
        assert np.array_equal(got["above"], stats["above"].astype(np.int64)) and np.array_equal(got["count"], stats["count"])
        assert (got["runs"] <= got["above"]).all() and (got["longest"] <= got["above"]).all()
        assert ((got["runs"] == 0) == (got["first"] == -1)).all() and ((got["runs"] == 0) == (got["above"] == 0)).all()
        some = got["runs"] > 0
        assert some.any() and ((~some).any() or len(edges) - 1 < 10)
        assert (got["first"][some] <= got["longest_start"][some]).all() and (got["longest_start"][some] <= got["last"][some]).all()
        assert (got["longest_start"][some] + got["longest"][some] - 1 <= got["last"][some]).all()
        assert (got["last"][some] - got["first"][some] + 1 >= got["above"][some]).all()
        one = got["runs"] == 1
        assert (got["longest"][one] == got["above"][one]).all() and (got["longest_start"][one] == got["first"][one]).all()
        # the peak tick holds the maximum word of series_window_stats
        for w, j in zip(*np.nonzero(got["peak_tick"] >= 0)):
            k = got["peak_tick"][w, j]
            assert words[j, k] == stats["max"][w, j] and not (words[j, int(min(edges[w], ticks)):k] == stats["max"][w, j]).any()


# ------------------------------------------------------------------------------------ the Python layer
def _scenario(ticks: int = 40):
    plan = lower(lb_two_servers(horizon=20))
    rng = np.random.default_rng(7)
    words = rng.integers(0, 5, (plan.n_series, ticks)).astype(np.uint32)
    counts = np.zeros(_abi.CNT_SLOTS, dtype=np.uint32)
    counts[_abi.CNT_TICKS] = ticks
    return plan, words, ScenarioResults(plan, counts, np.zeros((0, 2)), words)


def test_scenario_accessor_and_its_default_window():
    plan, words, res = _scenario()
    thr = np.full(plan.n_series, 2.0)
    whole = res.get_series_excursions(thr)
    assert whole["tick_edges"].tolist() == [0, plan.tick_count] and whole["count"].tolist() == [40]      # ONE window by default
    want = series_window_excursions(words, [0, plan.tick_count], plan.n_edges, thr)
    for k in ("count", *KEYS):
        assert np.array_equal(whole[k], want[k])
    per = res.get_series_excursions(thr, ticks_per_window=8)
    assert np.array_equal(per["above"], series_window_excursions(words, tick_window_edges(8, plan.tick_count), plan.n_edges, thr)["above"])
    assert per["above"].sum() == whole["above"].sum() and res.get_series_excursions(None)["above"].sum() == np.count_nonzero(words)
    with pytest.raises(ValueError, match="one of"):
        res.get_series_excursions(thr, 1.0, ticks_per_window=8)


def test_refusals_of_the_python_layer():
    plan, words, res = _scenario()
    nan_thr = np.zeros(plan.n_series)
    nan_thr[3] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        series_window_excursions(words, [0, 5], plan.n_edges, nan_thr)
    with pytest.raises(ValueError, match="NaN"):
        res.get_series_excursions(nan_thr)
    with pytest.raises(ValueError, match="values"):
        series_window_excursions(words, [0, 5], plan.n_edges, [0.0, 1.0])
    with pytest.raises(ValueError, match="strictly increasing"):
        series_window_excursions(words, [0, 5, 5], plan.n_edges)
    none = ScenarioResults(plan, res.counts, np.zeros((0, 2)), None)
    with pytest.raises(RuntimeError, match="kept no sampled series"):
        none.get_series_excursions(None)
    batch = BatchedResults.__new__(BatchedResults)          # a batch of a run with collect_samples=False
    batch.plan = plan
    batch._samples_t = None  # noqa: SLF001
    names = batch.series_names()
    for call in (batch.series_excursion_summary, batch.series_excursion_bands,
                 lambda thr: batch.save_series_excursion_summary("unused.npz", thresholds=thr)):
        with pytest.raises(ValueError, match="unknown series"):
            call({"nobody:ram_in_use": 1.0})
        with pytest.raises(ValueError, match="NaN"):
            call({names[0]: float("nan")})
        with pytest.raises(ValueError, match="NaN"):
            call(nan_thr)
        with pytest.raises(RuntimeError, match="kept no sampled series"):
            call({names[0]: 1.0})
    for of in ("longest", "mean", "open", "last"):
        with pytest.raises(ValueError, match="of must be one of"):
            batch.series_excursion_bands({names[0]: 1.0}, of=of)
    assert BatchedResults.EXCURSION_BANDS == ("longest_s", "above_s", "runs", "first_s", "recovered_s", "peak_s")


def test_sharded_results_refuse_series_excursions():
    from asyncflow_amd.results import ShardedResults

    sh = ShardedResults.__new__(ShardedResults)
    for call in (sh.series_excursion_summary, sh.series_excursion_bands, sh.save_series_excursion_summary):
        with pytest.raises(NotImplementedError, match="several devices"):
            call(None)
