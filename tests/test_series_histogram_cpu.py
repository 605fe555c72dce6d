"""Occupancy histograms of the sampled series per window of ticks, CPU side: the C entry point and its struct, the host
definition (results.series_window_histogram) against a per-value Python loop that takes math.floor of the same float64
expression, the identities with series_window_stats and series_window_quantiles, the refusals of the Python layer, and the
on-disk summary and the bands of a batch whose device call is replaced by the host definition.  Every comparison of counts is
== on integers and every comparison of quantiles is on the bits of the float64; only the bands' means over the replicas, sums
of float shares, are held to 1e-12."""

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
from asyncflow_amd.results import (BatchedResults, ScenarioResults, ShardedResults, check_series_bins, load_summary,
                                   series_histogram_quantiles, series_window_histogram, series_window_quantiles, series_window_stats)
from oracle.scenarios import lb_two_servers

ROOT = Path(__file__).resolve().parent.parent
N_EDGES = 1                       # the synthetic scenario: one edge, one server -> columns edge, ready, io, ram
RAM = np.array([False, False, False, True])
RESIDUE = np.float32(-(2.0 ** -45))
WIDTHS = (1.0, 3.0, 0.25, 0.1, 1.0 / 3.0)
FIELDS = ["n_scenarios", "n_groups", "n_windows", "group", "tick_edges", "n_columns", "columns", "n_bins", "lo", "width",
          "count", "hist", "under", "over", "elapsed_ms", "scratch_bytes"]


@pytest.fixture(scope="module")
def lib():
    af_build.build()
    from asyncflow_amd.engine import load_library

    return load_library()


# ------------------------------------------------------------------------------------ the entry and its struct
def test_header_declares_and_library_exports_the_entry(lib):
    header = (ROOT / "include" / "asyncflow_hip.h").read_text()
    assert re.search(r"int\s+af_engine_summarize_series_histogram\s*\(\s*af_engine_t\s*\*", header)
    assert re.search(r"#define\s+AF_MAX_SERIES_HISTOGRAM_BINS\s+1024\b", header) and _abi.MAX_SERIES_HISTOGRAM_BINS == 1024
    assert "af_engine_summarize_series_histogram" in _abi.EXPORTED_SYMBOLS
    assert lib.af_engine_summarize_series_histogram.argtypes[2] is C.POINTER(_abi.AfSeriesHistogram)
    assert lib.af_abi_version() == 7
    assert asyncflow_amd.series_window_histogram is series_window_histogram
    assert asyncflow_amd.series_histogram_quantiles is series_histogram_quantiles
    for listing in ((ROOT / "asyncflow_amd" / "build.py").read_text(), (ROOT / "asyncflow_amd" / "jit.py").read_text()):
        assert '"af_series_histogram.hpp"' in listing


def test_af_series_histogram_layout_matches_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "a host C compiler is needed for the layout probe"
    assert [name for name, _ in _abi.AfSeriesHistogram._fields_] == FIELDS  # noqa: SLF001
    src = tmp_path / "probe.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "asyncflow_hip.h"\n'
        'int main(void) { printf("%zu", sizeof(af_series_histogram_t));\n'
        + "".join(f'printf(" %zu", offsetof(af_series_histogram_t, {f}));\n' for f in FIELDS)
        + 'printf(" %d\\n", AF_MAX_SERIES_HISTOGRAM_BINS); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run([cc, "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    P = _abi.AfSeriesHistogram
    assert got == [C.sizeof(P), *(getattr(P, f).offset for f in FIELDS), _abi.MAX_SERIES_HISTOGRAM_BINS]
    # the header states the fields in this order
    body = re.search(r"typedef struct af_series_histogram \{(.*?)\} af_series_histogram_t;", (ROOT / "include" / "asyncflow_hip.h").read_text(), re.S)
    assert body and re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S)) == FIELDS


def test_series_histogram_entry_refuses_without_a_device(lib):
    from asyncflow_amd.engine import PLAN_ONLY, Engine, EngineUnavailableError

    eng = Engine(lower(lb_two_servers(horizon=20)), PLAN_ONLY)
    try:
        out = _abi.AfOutputs(0, None, 4, None, None)
        edges = (C.c_uint32 * 3)(0, 1, 2)
        req = _abi.AfSeriesHistogram(4, 1, 2, None, edges, 0, None, 8, None, None, None, None, None, None, 0.0, 0)
        call = lib.af_engine_summarize_series_histogram
        assert call(None, C.byref(out), C.byref(req)) == _abi.AF_ERR_INVALID
        assert call(eng._h, None, C.byref(req)) == _abi.AF_ERR_INVALID  # noqa: SLF001
        assert call(eng._h, C.byref(out), None) == _abi.AF_ERR_INVALID  # noqa: SLF001
        assert call(eng._h, C.byref(out), C.byref(req)) == _abi.AF_ERR_NO_DEVICE  # noqa: SLF001
        assert b"planning-only" in lib.af_last_error()
        kw = {"samples_ptr": 0, "tick_capacity": 4, "counts_ptr": 0, "hist_ptr": 0}
        with pytest.raises(EngineUnavailableError, match="planning-only"):
            eng.summarize_series_histogram(4, 1, [0, 2, 4], 8, **kw)
        # a bad request never reaches the library
        for bad, what in (([0], "at least two"), ([0, 2, 2], "strictly increasing"), ([0.5, 2], "whole")):
            with pytest.raises(ValueError, match=what):
                eng.summarize_series_histogram(4, 1, bad, 8, **kw)
        for bins in (0, 1025, 2.5, True):
            with pytest.raises(ValueError, match="bins"):
                eng.summarize_series_histogram(4, 1, [0, 4], bins, **kw)
        with pytest.raises(ValueError, match="width"):
            eng.summarize_series_histogram(4, 1, [0, 4], 8, width=0.0, **kw)
        with pytest.raises(ValueError, match="series columns"):
            eng.summarize_series_histogram(4, 1, [0, 4], 8, columns=[12], **kw)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------ the host definition and a plain loop
def _values(words: np.ndarray) -> np.ndarray:
    return np.where(RAM[:, None], words.view(np.float32).astype(np.float64), words.astype(np.float64))


def _loop(words, edges, bins, columns, lo, width):
    """The rule of include/asyncflow_hip.h value by value in plain Python: x < lo -> under; t = (x - lo) / width as Python
    floats (IEEE doubles); t >= bins -> over; else bin math.floor(t)."""
    ticks = words.shape[1]
    values = _values(words)
    W, Cn = len(edges) - 1, len(columns)
    count = [min(edges[w + 1], ticks) - min(edges[w], ticks) for w in range(W)]
    hist = np.zeros((W, Cn, bins), dtype=np.int64)
    under, over = np.zeros((W, Cn), dtype=np.int64), np.zeros((W, Cn), dtype=np.int64)
    for w in range(W):
        for c, j in enumerate(columns):
            for k in range(min(edges[w], ticks), min(edges[w + 1], ticks)):
                x = float(values[j, k])
                if x < lo[c]:
                    under[w, c] += 1
                    continue
                t = (x - lo[c]) / width[c]
                if t >= float(bins):
                    over[w, c] += 1
                else:
                    hist[w, c, math.floor(t)] += 1
    return {"count": np.array(count, dtype=np.int64), "hist": hist, "under": under, "over": over}


def _words(rng, ticks: int, bins: int, lo: float) -> np.ndarray:
    """Words [4, ticks]: three integer columns with most of their mass at 0 and the values bins - 1, bins, lo - 1 and lo among
    the rest; a ram column of multiples of 1/256 with -0.0, +0.0 and the -2^-45 residue."""
    special = np.array([bins - 1, bins, max(int(lo) - 1, 0), max(int(lo), 0), bins + 1, 3 * bins], dtype=np.int64)
    words = np.zeros((4, ticks), dtype=np.uint32)
    for j in range(3):
        u = rng.random(ticks)
        v = np.where(u < 0.5, 0, np.where(u < 0.8, rng.integers(0, bins + 3, ticks), special[rng.integers(0, len(special), ticks)]))
        words[j] = v.astype(np.uint32)
    f = (rng.integers(-2 * 256, (bins + 2) * 256, ticks) / 256.0).astype(np.float32)
    u = rng.random(ticks)
    f[u < 0.1] = np.float32(-0.0)
    f[(u >= 0.1) & (u < 0.2)] = np.float32(0.0)
    f[(u >= 0.2) & (u < 0.3)] = RESIDUE
    f[(u >= 0.3) & (u < 0.4)] = rng.integers(0, bins + 2, int(((u >= 0.3) & (u < 0.4)).sum())).astype(np.float32)   # (whole values: bin edges)
    words[3] = f.view(np.uint32)
    return words


def _same(got, want, what):
    for k in ("count", "hist", "under", "over"):
        assert got[k].dtype == np.int64 and got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(got[k], want[k]), (what, k, np.argwhere(got[k] != want[k])[:5])
    assert np.array_equal(got["under"] + got["hist"].sum(axis=-1) + got["over"], np.broadcast_to(got["count"][:, None], got["under"].shape)), what


@pytest.mark.parametrize("bins", [1, 2, 16, 64])
def test_host_definition_equals_a_loop_over_the_values(bins):
    rng = np.random.default_rng(bins)
    ticks = 230
    edges = [0, 1, 2, 50, 51, 200, 229, 230, 231, 400]      # windows of one tick, a short one at the end, two past the samples
    words = _words(rng, ticks, bins, 2.0)
    # the default binning, all series
    got = series_window_histogram(words, edges, N_EDGES, bins)
    _same(got, _loop(words, edges, bins, [0, 1, 2, 3], [0.0] * 4, [1.0] * 4), f"{bins} bins, default")
    assert got["hist"][:, :3, 0].sum() > ticks                                         # the mass at 0
    assert got["count"].tolist() == [1, 1, 48, 1, 149, 29, 1, 0, 0] and not got["hist"][-2:].any()
    assert got["ram"].tolist() == RAM.tolist() and np.array_equal(got["bin_edges"], np.tile(np.arange(bins + 1.0), (4, 1)))
    # -0.0 is not below 0.0, the residue is
    ram_values = words[3].view(np.float32)
    assert got["under"][:, 3].sum() == int((ram_values.astype(np.float64) < 0.0).sum()) >= int((ram_values == RESIDUE).sum()) > 0
    assert np.signbit(ram_values[ram_values == 0]).any() and not np.signbit(ram_values[ram_values == 0]).all()
    # every width on every kind of column, lo on and off a value, columns in any order with duplicates
    columns = [3, 0, 1, 2, 3, 0, 3, 1, 2, 3]
    lo = [0.0, 2.0, 0.0, 1.0, -1.0, 0.0, 0.5, 3.0, 0.0, 0.0]
    width = [WIDTHS[i % 5] for i in range(10)]
    got = series_window_histogram(words, edges, N_EDGES, bins, columns, lo, width)
    want = _loop(words, edges, bins, columns, lo, width)
    _same(got, want, f"{bins} bins, per column")
    assert np.array_equal(got["bin_edges"], np.array(lo)[:, None] + np.arange(bins + 1.0)[None, :] * np.array(width)[:, None])
    # values on exact bin edges: t is a whole number below bins
    values = _values(words)
    on_edge = 0
    for c, j in enumerate(columns):
        t = (values[j] - lo[c]) / width[c]
        on_edge += int(((t == np.floor(t)) & (t > 0) & (t < bins)).sum())
    assert on_edge > 0 or bins == 1
    # a scalar lo / width is one value for every column
    a = series_window_histogram(words, edges, N_EDGES, bins, [1, 3], 2.0, 0.25)
    b = series_window_histogram(words, edges, N_EDGES, bins, [1, 3], [2.0, 2.0], [0.25, 0.25])
    _same(a, b, "scalars")


def test_the_values_bins_minus_one_bins_lo_minus_one_and_lo():
    bins, lo = 8, 5.0
    words = np.zeros((4, 6), dtype=np.uint32)
    words[0] = [7, 8, 4, 5, 12, 13]
    words[3] = np.array([7.0, 8.0, 4.0, 5.0, 12.99, 13.0], dtype=np.float32).view(np.uint32)
    plain = series_window_histogram(words, [0, 6], N_EDGES, bins, [0, 3])
    assert plain["hist"][0, :, 7].tolist() == [1, 1] and plain["over"][0].tolist() == [3, 3] and plain["under"][0].tolist() == [0, 0]
    moved = series_window_histogram(words, [0, 6], N_EDGES, bins, [0, 3], lo, 1.0)
    assert moved["under"][0].tolist() == [1, 1] and moved["over"][0].tolist() == [1, 1]
    assert moved["hist"][0, 0].tolist() == [1, 0, 1, 1, 0, 0, 0, 1] and moved["hist"][0, 1].tolist() == [1, 0, 1, 1, 0, 0, 0, 1]


# ------------------------------------------------------------------------------------ identities
def test_above_of_the_series_window_statistics():
    rng = np.random.default_rng(11)
    bins, ticks = 16, 300
    words = _words(rng, ticks, bins, 0.0)
    words[3] = rng.integers(0, bins + 3, ticks).astype(np.float32).view(np.uint32)      # (whole ram values: > t is bins k > t)
    edges = [0, 7, 150, 299, 300, 310]
    h = series_window_histogram(words, edges, N_EDGES, bins)
    for t in (0, 1, 5, bins - 1):
        above = series_window_stats(words, edges, N_EDGES, np.full(4, float(t)))["above"]
        assert np.array_equal(h["hist"][:, :, t + 1:].sum(axis=-1) + h["over"], above.astype(np.int64)), t
    assert (h["under"] == 0).all() and h["over"].sum() > 0


def test_quantiles_from_the_histogram_are_the_exact_quantiles():
    rng = np.random.default_rng(12)
    bins, ticks = 32, 400
    levels = np.concatenate([np.linspace(0.0, 1.0, 36), [0.001, 0.5, 0.999, 0.95]])
    assert levels.shape == (40,)
    words = _words(rng, ticks, bins, 3.0)
    edges = [0, 1, 3, 100, 101, 399, 400, 450]
    cols = [0, 1, 2, 1]
    for lo in (0.0, 3.0):
        h = series_window_histogram(words, edges, N_EDGES, bins, cols, lo, 1.0)
        got = series_histogram_quantiles(h, levels)
        _, exact = series_window_quantiles(words, edges, N_EDGES, levels[:16], cols)
        exact = np.concatenate([exact] + [series_window_quantiles(words, edges, N_EDGES, levels[i:i + 16], cols)[1] for i in (16, 32)], axis=2)
        assert got.shape == exact.shape == (7, 4, 40)
        whole = ((h["under"] == 0) & (h["over"] == 0) & (h["count"][:, None] > 0))
        assert whole.any() and (~whole).any()
        assert got[whole].tobytes() == exact[whole].tobytes()                        # bit for bit
        assert np.isnan(got[-1]).all()                                               # the empty cell
        # a rank outside the bins: NaN exactly where floor(v), or the next rank where t > 0, lies in under / over
        n = h["count"][:, None, None].astype(np.float64)
        v = (n - 1.0) * levels[None, None, :]
        lo_r = np.floor(v)
        hi_r = np.where(v > lo_r, np.minimum(lo_r + 1, n - 1), lo_r)
        first, last = h["under"][:, :, None], (h["under"] + h["hist"].sum(axis=-1))[:, :, None]
        outside = (n == 0) | (lo_r < first) | (hi_r >= last)
        assert np.array_equal(np.isnan(got), outside) and outside[~whole].any() and not outside[~whole].all()
        assert got[~outside].tobytes() == exact[~outside].tobytes()
    with pytest.raises(ValueError, match="ram_in_use"):
        series_histogram_quantiles(series_window_histogram(words, edges, N_EDGES, bins), [0.5])
    for lo, width in ((0.5, 1.0), (0.0, 2.0), (0.0, 0.25)):
        with pytest.raises(ValueError, match="whole lo and width == 1"):
            series_histogram_quantiles(series_window_histogram(words, edges, N_EDGES, bins, [0], lo, width), [0.5])
    for bad in ([], [1.5], [float("nan")], 0.5):
        with pytest.raises(ValueError, match="levels"):
            series_histogram_quantiles(h, bad)


# ------------------------------------------------------------------------------------ the Python layer
def test_check_series_bins():
    n_bins, lo, width = check_series_bins(64, 3)
    assert n_bins == 64 and lo.tolist() == [0.0] * 3 and width.tolist() == [1.0] * 3
    assert check_series_bins(np.int64(1024), 2, 1.5, [0.1, 3.0])[1:][0].tolist() == [1.5, 1.5]
    for bins in (0, -1, 1025, 2.0, "8", None, True):
        with pytest.raises(ValueError, match="bins"):
            check_series_bins(bins, 3)
    for width in (0.0, -1.0, [1.0, 0.0, 1.0]):
        with pytest.raises(ValueError, match="width must be above 0"):
            check_series_bins(8, 3, None, width)
    for width in (float("nan"), float("inf"), [1.0, float("nan"), 1.0]):
        with pytest.raises(ValueError, match="width must be finite"):
            check_series_bins(8, 3, None, width)
    for lo in (float("nan"), float("-inf"), [0.0, 0.0, float("inf")]):
        with pytest.raises(ValueError, match="lo must be finite"):
            check_series_bins(8, 3, lo)
    for lo in ([0.0, 1.0], [[0.0, 0.0, 0.0]]):
        with pytest.raises(ValueError, match="one value per output column"):
            check_series_bins(8, 3, lo)


def test_host_definition_refusals():
    words = np.zeros((4, 10), dtype=np.uint32)
    with pytest.raises(ValueError, match="strictly increasing"):
        series_window_histogram(words, [0, 5, 5], N_EDGES, 8)
    with pytest.raises(ValueError, match="bins"):
        series_window_histogram(words, [0, 5], N_EDGES, 0)
    with pytest.raises(ValueError, match="width"):
        series_window_histogram(words, [0, 5], N_EDGES, 8, None, 0.0, -1.0)
    for bad in ([], [4], [-1], [0.5]):
        with pytest.raises(ValueError, match="series"):
            series_window_histogram(words, [0, 5], N_EDGES, 8, bad)
    with pytest.raises(ValueError, match="samples must be words"):
        series_window_histogram(np.zeros(10, dtype=np.uint32), [0, 5], N_EDGES, 8)


def test_tick_edge_forms_of_a_scenario():
    plan = lower(lb_two_servers(horizon=10))
    rng = np.random.default_rng(3)
    ticks = plan.tick_count
    words = rng.integers(0, 50, (plan.n_series, ticks)).astype(np.uint32)
    res = ScenarioResults(plan, np.zeros(_abi.CNT_SLOTS, dtype=np.uint32), np.zeros((0, 2)), words)
    per = int(round(2.0 / plan.sample_period))
    a = res.get_series_histogram(64, 2.0)
    b = res.get_series_histogram(64, ticks_per_window=per)
    c = res.get_series_histogram(tick_edges=a["tick_edges"])
    assert a["hist"].shape == (-(-ticks // per), plan.n_series, 64) and int(a["count"].sum()) == ticks
    for other in (b, c):
        assert all(np.array_equal(other[k], a[k]) for k in ("count", "hist", "under", "over"))
    sel = res.get_series_histogram(64, 2.0, series=[5, 1], lo=[0.0, 10.0], width=2.0)
    assert sel["series"].tolist() == [5, 1] and np.array_equal(sel["bin_edges"][1], 10.0 + 2.0 * np.arange(65))
    with pytest.raises(ValueError, match="one of"):
        res.get_series_histogram(64, 2.0, ticks_per_window=per)
    none = ScenarioResults(plan, res.counts, np.zeros((0, 2)), None)
    with pytest.raises(RuntimeError, match="kept no sampled series"):
        none.get_series_histogram()


def test_refusals_of_the_batch_layer():
    plan = lower(lb_two_servers(horizon=10))
    batch = BatchedResults.__new__(BatchedResults)
    batch.plan = plan
    batch._samples_t = None  # noqa: SLF001
    for call in (batch.series_histogram_summary, batch.series_histogram_bands):
        with pytest.raises(RuntimeError, match="kept no sampled series"):
            call()
    with pytest.raises(RuntimeError, match="kept no sampled series"):
        batch.save_series_histogram_summary("nowhere.npz", ticks_per_window=10)
    batch._samples_t = object()  # noqa: SLF001  (the checks below come before the device is touched)
    names = batch.series_names()
    with pytest.raises(ValueError, match="bins"):
        batch.series_histogram_summary(0)
    with pytest.raises(ValueError, match="bins"):
        batch.series_histogram_summary(1025)
    with pytest.raises(ValueError, match="unknown series"):
        batch.series_histogram_summary(series=["nobody:ram_in_use"])
    with pytest.raises(ValueError, match="unknown series 'nobody' in width"):
        batch.series_histogram_summary(width={"nobody": 2.0})
    with pytest.raises(ValueError, match="unknown series 'nobody' in lo"):
        batch.series_histogram_summary(lo={"nobody": 2.0})
    with pytest.raises(ValueError, match="width must be above 0"):
        batch.series_histogram_summary(width={names[0]: 0.0})
    with pytest.raises(ValueError, match="one value per output column"):
        batch.series_histogram_summary(series=[0, 1], lo=[0.0, 0.0, 0.0])
    with pytest.raises(ValueError, match="lo must be finite"):
        batch.series_histogram_summary(lo=float("nan"))
    with pytest.raises(ValueError, match="one of"):
        batch.series_histogram_summary(64, 1.0, ticks_per_window=10)
    # a dict names series; missing ones keep the default
    col = np.array([3, 0, 3])
    assert batch._series_binning("width", {names[3]: 0.5}, col, 1.0).tolist() == [0.5, 1.0, 0.5]  # noqa: SLF001
    assert batch._series_binning("lo", 2.0, col, 0.0) == 2.0 and batch._series_binning("lo", None, col, 0.0) is None  # noqa: SLF001


def test_sharded_results_refuse_series_histograms():
    sh = ShardedResults.__new__(ShardedResults)
    for call in (sh.series_histogram_summary, sh.series_histogram_bands, sh.save_series_histogram_summary):
        with pytest.raises(NotImplementedError, match="several devices"):
            call(64)


# ------------------------------------------------------------------------------------ the on-disk summary
class _HostBatch(BatchedResults):
    """A batch of host arrays whose histogram call is the host definition, group by group."""

    def series_histogram_summary(self, bins=64, window_s=None, *, ticks_per_window=None, tick_edges=None, by=None, series=None,
                                 lo=None, width=None):
        import torch

        col = self._series_columns(series)
        b = self._series_tick_edges(window_s, ticks_per_window, tick_edges)
        ids, n_groups = self._window_groups(by)
        n_bins, lo_v, width_v = check_series_bins(bins, len(col), self._series_binning("lo", lo, col, 0.0),
                                                  self._series_binning("width", width, col, 1.0))
        W = len(b) - 1
        out = {"count": np.zeros((n_groups, W), dtype=np.int64), "hist": np.zeros((n_groups, W, len(col), n_bins), dtype=np.int64),
               "under": np.zeros((n_groups, W, len(col)), dtype=np.int64), "over": np.zeros((n_groups, W, len(col)), dtype=np.int64)}
        one = None
        for s, g in enumerate(ids):
            if g < 0:
                continue
            one = series_window_histogram(self.host_words[s], b, self.plan.n_edges, n_bins, col, lo_v, width_v)
            for k in out:
                out[k][g] += one[k]
        names = self.series_names()
        res = {k: torch.as_tensor(v) for k, v in out.items()}
        res.update(bin_edges=one["bin_edges"], ram=one["ram"], series=[names[j] for j in col], tick_edges=b,
                   times=b[:-1].astype(np.float64) * self.plan.sample_period, replicas=np.bincount(ids[ids >= 0], minlength=n_groups),
                   series_histogram_ms=0.0, scratch_bytes=0)
        return res


def _host_batch():
    plan = lower(lb_two_servers(horizon=10))
    rng = np.random.default_rng(21)
    n, ticks = 6, plan.tick_count
    batch = _HostBatch.__new__(_HostBatch)
    batch.plan = plan
    batch.counts = np.zeros((n, _abi.CNT_SLOTS), dtype=np.uint32)
    batch._samples_t = object()  # noqa: SLF001
    batch._summ_engine = None  # noqa: SLF001
    batch.host_words = np.where(rng.random((n, plan.n_series, ticks)) < 0.6, 0, rng.integers(0, 40, (n, plan.n_series, ticks))).astype(np.uint32)
    return batch, np.array([0, 1, 0, 1, -1, 1])


@pytest.mark.parametrize("ext", ["npz", "parquet"])
def test_on_disk_round_trip(tmp_path, ext):
    if ext == "parquet":
        pytest.importorskip("pyarrow")
    batch, ids = _host_batch()
    names = batch.series_names()
    queue = [k for k in names if k.endswith("ready_queue_len")]
    path = str(tmp_path / f"series_hist.{ext}")
    written = batch.save_series_histogram_summary(path, ids, bins=32, series=queue, lo={queue[0]: 1.0}, ticks_per_window=50)
    back = load_summary(path)
    assert set(back) == set(written)
    for k, v in written.items():
        assert np.array_equal(np.asarray(back[k], dtype=v.dtype), v), k
    W = -(-batch.plan.tick_count // 50)
    want = batch.series_histogram_summary(32, ticks_per_window=50, by=ids, series=queue, lo={queue[0]: 1.0})
    assert back["replicas"].tolist() == [2, 3] and np.array_equal(back["series_hist_count"], want["count"].numpy())
    for c, name in enumerate(queue):
        assert back[f"series_hist:{name}"].shape == (2, W, 32)
        assert np.array_equal(back[f"series_hist:{name}"], want["hist"].numpy()[:, :, c])
        assert np.array_equal(back[f"series_hist_under:{name}"], want["under"].numpy()[:, :, c])
        assert np.array_equal(back[f"series_hist_over:{name}"], want["over"].numpy()[:, :, c])
        assert np.array_equal(back[f"series_hist_bin_edges:{name}"], (1.0 if c == 0 else 0.0) + np.arange(33.0))
    assert back[f"series_hist_under:{queue[0]}"].sum() > 0                       # (lo = 1: the zeros are below)
    assert np.array_equal(back["series_hist_tick_edges"], want["tick_edges"]) and np.array_equal(back["series_hist_times"], want["times"])
    with pytest.raises(ValueError, match="selected once"):
        batch.save_series_histogram_summary(path, ids, series=[queue[0], queue[0]], ticks_per_window=50)


def test_bands_of_a_host_batch():
    """series_histogram_bands on the host stand-in: the shares' mean over the replicas and the pooled histogram."""
    batch, ids = _host_batch()
    bands = batch.series_histogram_bands(16, ticks_per_window=100, by=ids, series=[1, 4])
    per = batch.series_histogram_summary(16, ticks_per_window=100, by="scenario", series=[1, 4])
    pooled = batch.series_histogram_summary(16, ticks_per_window=100, by=ids, series=[1, 4])
    W = int(per["count"].shape[1])
    assert bands["mean"].shape == bands["q_lo"].shape == bands["pooled"].shape == (2, W, 2, 16) and bands["n"].shape == (2, W)
    assert np.array_equal(bands["pooled"], pooled["hist"].numpy()) and np.array_equal(bands["pooled_count"], pooled["count"].numpy())
    assert np.array_equal(bands["pooled_under"], pooled["under"].numpy()) and np.array_equal(bands["pooled_over"], pooled["over"].numpy())
    share = per["hist"].numpy() / per["count"].numpy()[:, :, None, None]
    for g in range(2):
        np.testing.assert_allclose(bands["mean"][g], share[ids == g].mean(axis=0), rtol=1e-12, atol=1e-15)
    assert bands["replicas"].tolist() == [2, 3] and bands["series"] == [batch.series_names()[j] for j in (1, 4)]
