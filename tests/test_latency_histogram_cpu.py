"""Log-linear latency histograms per window and group, CPU side: the C entry point and its struct, the bit rule
(`results.latency_bin_index`) against `np.searchsorted` on the exact edges, the host definition (`results.latency_histogram`) that
`af_engine_summarize_latency_histogram` is held to word for word against a brute-force mask per window on every committed golden
clock, and what is read off a summary afterwards: quantile brackets against `np.quantile`, the merge and regroup identities, the
Kolmogorov-Smirnov distance against a brute-force one, and every refusal of the host surface."""

from __future__ import annotations

import ctypes as C
import json
import math
import re
import shutil
import subprocess
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import asyncflow_amd
from asyncflow_amd import _abi, expand_grid
from asyncflow_amd import build as af_build
from asyncflow_amd.plan import lower
from asyncflow_amd.results import (ScenarioResults, ShardedResults, check_latency_bins, groups_of_columns, latency_bin_edges,
                                   latency_bin_index, latency_histogram, latency_histogram_distance, latency_histogram_merge,
                                   latency_histogram_quantiles, latency_histogram_regroup, latency_window_stats)
from oracle.scenarios import lb_two_servers

ROOT = Path(__file__).resolve().parent.parent
FIXTURES = sorted(p.stem for p in (ROOT / "tests" / "golden").glob("*.npz") if "clock" in np.load(p).files)
BINNINGS = [(0, -3, 1), (5, -20, 32), (7, -20, 32), (8, -1022, 16), (3, 1000, 23)]


@pytest.fixture(scope="module")
def lib():
    af_build.build()
    from asyncflow_amd.engine import load_library

    return load_library()


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry(lib):
    header = (ROOT / "include" / "asyncflow_hip.h").read_text()
    assert re.search(r"int\s+af_engine_summarize_latency_histogram\s*\(\s*af_engine_t\s*\*", header)
    assert re.search(r"#define\s+AF_MAX_LATENCY_HISTOGRAM_BINS\s+4096\b", header)
    assert re.search(r"#define\s+AF_ABI_VERSION\s+7\b", header)
    assert "af_engine_summarize_latency_histogram" in _abi.EXPORTED_SYMBOLS
    assert lib.af_engine_summarize_latency_histogram.argtypes[2] is C.POINTER(_abi.AfLatencyHistogram)
    assert lib.af_abi_version() == 7
    for src in ("build.py", "jit.py"):
        assert '"af_latency_histogram.hpp"' in (ROOT / "asyncflow_amd" / src).read_text()
    for name in ("check_latency_bins", "latency_bin_edges", "latency_bin_index", "latency_histogram", "latency_histogram_quantiles",
                 "latency_histogram_merge", "latency_histogram_regroup", "latency_histogram_distance"):
        assert name in asyncflow_amd.__all__ and getattr(asyncflow_amd, name) is getattr(asyncflow_amd.results, name)


def test_af_latency_histogram_layout_matches_the_header_and_the_other_structs_keep_their_sizes(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "a host C compiler is needed for the layout probe"
    fields = [name for name, _ in _abi.AfLatencyHistogram._fields_]  # noqa: SLF001
    assert fields == ["n_scenarios", "n_groups", "n_windows", "group", "edges", "by_arrival", "sub_bits", "min_exp", "octaves", "count",
                      "hist", "under", "over", "nan", "elapsed_ms", "scratch_bytes"]
    others = {"af_arrivals_t": (_abi.AfArrivals, 96), "af_inflight_t": (_abi.AfInflight, 152), "af_outputs_t": (_abi.AfOutputs, 80),
              "af_pooled_t": (_abi.AfPooled, 32), "af_quantiles_t": (_abi.AfQuantiles, 104), "af_windows_t": (_abi.AfWindows, 64),
              "af_state_bins_t": (_abi.AfStateBins, 32), "af_series_windows_t": (_abi.AfSeriesWindows, 96),
              "af_series_quantiles_t": (_abi.AfSeriesQuantiles, 96), "af_series_excursions_t": (_abi.AfSeriesExcursions, 104),
              "af_series_histogram_t": (_abi.AfSeriesHistogram, 120), "af_series_combined_t": (_abi.AfSeriesCombined, 176),
              "af_series_joint_t": (_abi.AfSeriesJoint, 128), "af_series_warmup_t": (_abi.AfSeriesWarmup, 120),
              "af_exemplars_t": (_abi.AfExemplars, 112), "af_summary_t": (_abi.AfSummary, 64), "af_sweep_t": (_abi.AfSweep, 40),
              "af_stats_t": (_abi.AfStats, 168)}
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "asyncflow_hip.h"\n'
                   'int main(void) { printf("%zu", sizeof(af_latency_histogram_t));\n'
                   + "".join(f'printf(" %zu", offsetof(af_latency_histogram_t, {f}));\n' for f in fields)
                   + "".join(f'printf(" %zu", sizeof({t}));\n' for t in others) + 'printf("\\n"); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run([cc, "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    P = _abi.AfLatencyHistogram
    assert C.sizeof(P) == 104 and P.min_exp.size == 4
    assert got == [C.sizeof(P), *(getattr(P, f).offset for f in fields), *(size for _, size in others.values())]
    assert [C.sizeof(cls) for cls, _ in others.values()] == [size for _, size in others.values()]


def test_entry_refuses_without_a_device(lib):
    from asyncflow_amd.engine import PLAN_ONLY, Engine, EngineUnavailableError

    eng = Engine(lower(lb_two_servers(horizon=20)), PLAN_ONLY)
    try:
        out = _abi.AfOutputs(4, None, 8, None, None)
        req = _abi.AfLatencyHistogram(4, 1, 0, None, None, 0, 5, -20, 32)
        entry = lib.af_engine_summarize_latency_histogram
        assert entry(None, C.byref(out), C.byref(req)) == _abi.AF_ERR_INVALID
        assert entry(eng._h, None, C.byref(req)) == _abi.AF_ERR_INVALID  # noqa: SLF001
        assert entry(eng._h, C.byref(out), None) == _abi.AF_ERR_INVALID  # noqa: SLF001
        assert entry(eng._h, C.byref(out), C.byref(req)) == _abi.AF_ERR_NO_DEVICE  # noqa: SLF001
        assert b"planning-only" in lib.af_last_error()
        kw = dict(clock_ptr=0, clock_capacity=4, counts_ptr=0, count_ptr=0, hist_ptr=0)
        with pytest.raises(EngineUnavailableError, match="planning-only"):
            eng.summarize_latency_histogram(4, 1, **kw)
        for bad in (dict(sub_bits=9), dict(sub_bits=-1), dict(min_exp=-1023), dict(octaves=0), dict(min_exp=1000, octaves=24),
                    dict(sub_bits=8, octaves=17), dict(sub_bits=2.0), dict(octaves=True)):
            with pytest.raises(ValueError, match="sub_bits|min_exp|octaves"):
                eng.summarize_latency_histogram(4, 1, **bad, **kw)
        with pytest.raises(ValueError, match="arrival"):
            eng.summarize_latency_histogram(4, 1, window_of="arrival", **kw)
        with pytest.raises(ValueError, match="window_of"):
            eng.summarize_latency_histogram(4, 1, edges=[0.0, 1.0], window_of="start", **kw)
        with pytest.raises(ValueError, match="strictly increasing"):
            eng.summarize_latency_histogram(4, 1, edges=[0.0, 1.0, 1.0], **kw)
    finally:
        eng.close()


# ---- the bit rule ---------------------------------------------------------------------------------------------------------
def _probe_values(binning, rng) -> np.ndarray:
    m, e, o = binning
    E = latency_bin_edges(m, e, o)
    mid = float(np.clip(e + o / 2.0, -1000, 1000))
    rnd = np.exp2(rng.normal(mid, o / 3.0 + 1.0, 2000).clip(-1070, 1023))          # log-normal around the bins
    return np.concatenate([E, np.nextafter(E, np.inf), np.nextafter(E, -np.inf), rnd,
                           [0.0, -0.0, -1.0, -1e-300, -5e-324, np.inf, -np.inf, np.nan, 5e-324, 2.0 ** -1022, np.finfo(np.float64).max]])


@pytest.mark.parametrize("binning", BINNINGS)
def test_the_bit_rule_equals_searchsorted_on_the_exact_edges(binning):
    m, e, o = binning
    assert check_latency_bins(m, e, o) == (m, e, o, o << m)
    E = latency_bin_edges(m, e, o)
    n_bins = o << m
    assert E.shape == (n_bins + 1,) and E.dtype == np.float64 and (np.diff(E) > 0).all()
    assert E[0] == math.ldexp(1.0, e) and E[-1] == math.ldexp(1.0, e + o)
    for b in (0, n_bins // 2, n_bins - 1):                                          # exact: the stated formula in Fractions
        want = (1 + Fraction(b & ((1 << m) - 1), 1 << m)) * Fraction(2) ** (e + (b >> m))
        assert Fraction(float(E[b])) == want
    assert np.allclose(np.diff(E) / E[:-1], 2.0 ** -m * (1.0 / (1.0 + (np.arange(n_bins) & ((1 << m) - 1)) / (1 << m))), rtol=1e-12)
    x = _probe_values(binning, np.random.default_rng(n_bins))
    got = latency_bin_index(x, m, e, o)
    pos = np.searchsorted(E, x, side="right") - 1
    want = np.where(np.isnan(x), -3, np.where(pos < 0, -1, np.where(pos >= n_bins, -2, pos)))
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert set(np.unique(got[got < 0]).tolist()) == {-3, -2, -1} and (got >= 0).sum() > n_bins
    assert latency_bin_index(2.0 ** e, m, e, o).shape == () and int(latency_bin_index(2.0 ** e, m, e, o)) == 0
    assert latency_bin_index(x.reshape(-1, 1), m, e, o).shape == (x.shape[0], 1)


def test_the_default_binning():
    assert check_latency_bins() == (5, -20, 32, 1024)
    E = latency_bin_edges()
    assert E[0] == 2.0 ** -20 and E[-1] == 4096.0 and E[1] / E[0] == 1.0 + 2.0 ** -5


# ---- the histogram against a brute-force mask -------------------------------------------------------------------------------
def _brute(members, edges, window_of, binning):
    m, e, o = binning
    E = latency_bin_edges(m, e, o)
    n_bins = o << m
    n_win = 1 if edges is None else len(edges) - 1
    out = {"count": np.zeros(n_win, np.int64), "hist": np.zeros((n_win, n_bins), np.int64), "under": np.zeros(n_win, np.int64),
           "over": np.zeros(n_win, np.int64), "nan": np.zeros(n_win, np.int64)}
    for rows in members:
        rows = np.asarray(rows, dtype=np.float64).reshape(-1, 2)
        with np.errstate(invalid="ignore", over="ignore"):
            lat = rows[:, 1] - rows[:, 0]
        t = rows[:, 1] if window_of == "finish" else rows[:, 0]
        for w in range(n_win):
            mask = np.ones(lat.shape, bool) if edges is None else (t > edges[w]) & (t <= edges[w + 1])
            x = lat[mask]
            out["count"][w] += x.shape[0]
            out["nan"][w] += int(np.isnan(x).sum())
            out["under"][w] += int((x < E[0]).sum())
            out["over"][w] += int((x >= E[-1]).sum())
            for b in range(n_bins) if n_bins <= 64 else np.unique(np.searchsorted(E, x[(x >= E[0]) & (x < E[-1])], side="right") - 1):
                out["hist"][w, b] += int(((x >= E[b]) & (x < E[b + 1])).sum())
    return out


def _check(members, edges, window_of, binning):
    m, e, o = binning
    got = latency_histogram(members, edges, window_of, sub_bits=m, min_exp=e, octaves=o)
    want = _brute(members, edges, window_of, binning)
    assert got["count"].dtype == np.uint64 and all(got[k].dtype == np.uint32 for k in ("hist", "under", "over", "nan"))
    for k, v in want.items():
        assert got[k].shape == v.shape and np.array_equal(got[k].astype(np.int64), v), (k, window_of, binning)
    assert np.array_equal(got["under"].astype(np.int64) + got["over"] + got["nan"] + got["hist"].sum(axis=1), got["count"].astype(np.int64))
    return got


def _fixture(name: str):
    z = np.load(ROOT / "tests" / "golden" / f"{name}.npz")
    plan = lower(json.loads(str(z["payload_json"])))
    return plan, np.asarray(z["clock"], dtype=np.float64).reshape(-1, 2)


@pytest.mark.parametrize("name", FIXTURES)
def test_golden_clocks_against_the_brute_force_mask_and_the_window_statistics(name):
    plan, clock = _fixture(name)
    T = float(plan.total_time)
    one_s = np.arange(0.0, math.floor(T) + 1.0)
    uneven = np.array([0.25, 1.0, 1.5, 0.4 * T, 0.41 * T, 0.9 * T])
    for window_of in ("finish", "arrival"):
        for edges in (one_s, uneven):
            got = _check([clock], edges, window_of, (5, -20, 32))
            _check([clock], edges, window_of, (2, -8, 6))                            # few bins: latencies in under and over
            stats = latency_window_stats(clock, edges, window_of)
            assert np.array_equal(got["count"].astype(np.float64), stats[:, 0])
        assert int(got["hist"].sum()) > 0
    whole = _check([clock], None, "finish", (5, -20, 32))
    assert int(whole["count"][0]) == clock.shape[0] and int(whole["nan"][0]) == 0
    assert np.array_equal(latency_histogram(clock)["hist"], whole["hist"])          # (one array is one member)
    lat = clock[:, 1] - clock[:, 0]
    top = np.flatnonzero(whole["hist"][0])[-1]
    E = latency_bin_edges()
    assert E[top] <= lat.max() < E[top + 1]


def test_synthetic_rows_nan_negative_infinite_reversed_and_times_on_the_edges():
    nan, inf = float("nan"), float("inf")
    a = np.array([[1.0, 3.0], [2.0, 4.0], [1.0, 1.0], [5.0, 5.0], [0.5, inf], [nan, 2.0], [2.0, nan], [3.0, 2.0], [-inf, 1.0], [4.0, 4.0],
                  [inf, inf], [1.0, 2.0], [2.0, 2.0 + 2.0 ** -20], [2.0, 2.0 + 2.0 ** -21], [0.0, 4096.0], [0.0, np.nextafter(4096.0, 0.0)]])
    b = np.array([[0.0, 2.0], [0.0, -0.0], [-0.0, 0.0], [2.0, 4.0], [1.5, 3.5], [1e-310, 3e-310], [0.0, 5e-324]])
    members = [a, b, np.zeros((0, 2)), np.array([[7.0, 9.0]] * 5)]
    for binning in BINNINGS[:3] + [(8, -4, 16)]:
        got = _check(members, None, "finish", binning)
        assert int(got["nan"][0]) == 3 and int(got["count"][0]) == len(a) + len(b) + 5   # NaN latencies count, in nan
        for window_of in ("finish", "arrival"):
            got = _check(members, [0.0, 1.0, 2.0, 4.0, 5.0], window_of, binning)
            assert int(got["count"].sum()) < len(a) + len(b) + 5                     # rows outside (e[0], e[W]] are in no cell
    got = latency_histogram(members)
    assert int(got["over"][0]) == 3 and int(got["hist"][0, 0]) == 1 and int(got["hist"][0, -1]) == 1   # two +inf and 4096 over; 2^-20 in bin 0
    assert latency_histogram([], [0.0, 1.0, 2.0])["count"].tolist() == [0, 0] and latency_histogram([])["hist"].shape == (1, 1024)


# ---- quantile brackets --------------------------------------------------------------------------------------------------
def _summary(cells, edges=None, window_of="finish", binning=(5, -20, 32), replicas=None):
    """A summary as `latency_histogram_summary` returns it (numpy in place of tensors) from per-group member lists."""
    m, e, o = binning
    per = [latency_histogram(members, edges, window_of, sub_bits=m, min_exp=e, octaves=o) for members in cells]
    out = {k: np.stack([p[k] for p in per]).astype(np.int64) for k in ("hist", "count", "under", "over", "nan")}
    out.update(edges=None if edges is None else np.asarray(edges, dtype=np.float64), window_of=window_of, sub_bits=m, min_exp=e, octaves=o,
               bin_edges=latency_bin_edges(m, e, o), replicas=np.asarray(replicas if replicas is not None else [len(c) for c in cells]))
    return out


def _rows_of(lat) -> np.ndarray:
    lat = np.asarray(lat, dtype=np.float64)
    return np.stack([np.zeros_like(lat), lat], axis=1)


def test_quantile_brackets_contain_np_quantile_with_no_exclusions():
    rng = np.random.default_rng(7)
    E = latency_bin_edges()
    levels = np.concatenate([[0.0, 1.0, 0.5, 0.95, 0.99, 0.999, 1.0 / 3.0], rng.random(9)])
    samples = [np.array([0.125]), np.array([0.1]), np.full(7, E[300]), E[200:260].copy(), np.nextafter(E[200:260], 0.0),
               np.array([E[10], E[11]]), np.array([1e-9, 0.5]), np.array([0.0, -1.0, 0.25, 0.5, 1e4]), np.array([1e-12, 1e-9, 1e-8]),
               np.array([5000.0, 1e6, 1e9]), np.array([0.5, np.nan, 0.25, np.nan])]
    for n in (2, 3, 10, 11, 101, 1000):
        samples += [rng.lognormal(-3.0, 1.5, n), rng.lognormal(-3.0, 0.01, n), np.exp2(rng.integers(-22, 14, n).astype(np.float64))]
    cells = [[_rows_of(x)] for x in samples]
    summ = _summary(cells)
    for binning in ((5, -20, 32), (0, -3, 1), (8, -8, 16)):
        summ = _summary(cells, binning=binning)
        br = latency_histogram_quantiles(summ, levels)
        assert br["lo"].shape == (len(samples), 1, levels.shape[0]) == br["hi"].shape
        width = (1.0 + 2.0 ** -binning[0]) ** 2
        for g, x in enumerate(samples):
            valid = x[~np.isnan(x)]
            q = np.quantile(valid, levels)
            lo, hi = br["lo"][g, 0], br["hi"][g, 0]
            assert ((lo <= q) & (q < hi)).all(), (g, binning, lo, q, hi)
            inside = np.isfinite(lo) & np.isfinite(hi)
            pos = (valid.shape[0] - 1) * levels
            idx = latency_bin_index(np.sort(valid), *binning)
            near = idx[np.ceil(pos).astype(int)] - idx[np.floor(pos).astype(int)] <= 1
            assert (hi[inside & near] / lo[inside & near] <= width).all()
    empty = latency_histogram_quantiles(_summary([[np.zeros((0, 2))], [_rows_of([np.nan])]]), [0.0, 0.5])
    assert np.isnan(empty["lo"]).all() and np.isnan(empty["hi"]).all()
    under = latency_histogram_quantiles(_summary([[_rows_of([0.0, 1e-9, 1e5])]]), [0.0, 0.5, 1.0])
    assert under["lo"][0, 0].tolist() == [-np.inf, -np.inf, 4096.0] and under["hi"][0, 0].tolist() == [2.0 ** -20, 2.0 ** -20, np.inf]


def test_quantile_brackets_on_random_cells():
    rng = np.random.default_rng(8)
    samples = [rng.lognormal(rng.normal(-4.0, 2.0), rng.random() * 3.0, int(rng.integers(1, 40))) for _ in range(400)]
    levels = rng.random(16)
    br = latency_histogram_quantiles(_summary([[_rows_of(x)] for x in samples]), levels)
    for g, x in enumerate(samples):
        q = np.quantile(x, levels)
        assert ((br["lo"][g, 0] <= q) & (q < br["hi"][g, 0])).all(), g


# ---- merge and regroup ------------------------------------------------------------------------------------------------------
def _equal(a, b):
    for k in ("hist", "count", "under", "over", "nan"):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_merge_and_regroup_identities():
    _, clock = _fixture("lb2_events_t60")
    _, other = _fixture("overload_t30")
    rng = np.random.default_rng(9)
    members = [clock, other, clock[::3] + 0.125, other[5:400], _rows_of([np.nan, 0.0, 1e9]), clock[100:900]]
    edges = np.arange(0.0, 61.0, 5.0)
    for window_of in ("finish", "arrival"):
        single = _summary([[x] for x in members], edges, window_of)
        # the pooled group is the sum of its singletons
        pooled = _summary([members[:4], members[4:]], edges, window_of)
        re = latency_histogram_regroup(single, groups=[0, 0, 0, 0, 1, 1])
        _equal(re, pooled)
        assert re["replicas"].tolist() == [4, 2] and np.array_equal(re["edges"], edges)
        # merged windows are the regroup of the window histograms
        ranges = [(2, 3), (3, 7), (7, 12)]
        coarse = _summary([[x] for x in members], edges[[2, 3, 7, 12]], window_of)
        rw = latency_histogram_regroup(single, windows=ranges)
        _equal(rw, coarse)
        assert np.array_equal(rw["edges"], edges[[2, 3, 7, 12]])
        both = latency_histogram_regroup(single, groups=[1, -1, 1, 0, 0, -1], windows=[(0, 12)])
        _equal(both, _summary([[members[3], members[4]], [members[0], members[2]]], edges[[0, 12]], window_of))
        assert both["replicas"].tolist() == [2, 2]
        # the merge of a member split is the whole
        pick = rng.random(clock.shape[0]) < 0.4
        whole = _summary([[clock], [other]], edges, window_of)
        parts = latency_histogram_merge(_summary([[clock[pick]], [other[:100]]], edges, window_of), _summary([[clock[~pick]], [other[100:]]], edges, window_of))
        _equal(parts, whole)
        three = latency_histogram_merge(whole, whole, whole)
        assert np.array_equal(three["hist"], 3 * whole["hist"]) and three["replicas"].tolist() == [3, 3]
        # the results are summaries: the other functions take them
        q = latency_histogram_quantiles(rw, [0.5])
        assert q["lo"].shape == (6, 3, 1)
        assert latency_histogram_distance(re, (0, 1), (0, 1))["d"] == 0.0
    no_windows = _summary([[clock], [other]])
    _equal(latency_histogram_regroup(no_windows, groups=[0, 0], windows=[(0, 1)]), _summary([[clock, other]]))


# ---- the distance -----------------------------------------------------------------------------------------------------------
def test_distance_against_a_brute_force_kolmogorov_smirnov_on_the_binned_data():
    rng = np.random.default_rng(10)
    samples = [rng.lognormal(-3.0, 1.0, 500), rng.lognormal(-2.5, 1.0, 300), rng.lognormal(-3.0, 1.0, 500), np.array([0.0, 1e-9, 0.1, 0.2, 1e5, np.nan]),
               np.array([0.1]), np.zeros(0), np.array([np.nan])]
    binning = (3, -12, 16)
    summ = _summary([[_rows_of(x)] for x in samples], binning=binning)
    entries = []
    for x in samples:                                                               # -1 under first, the bins, over last
        idx = latency_bin_index(x, *binning)
        entries.append(np.sort(np.where(idx == -2, 16 << 3, idx)[idx != -3]))
    for i in range(len(samples)):
        for j in range(len(samples)):
            got = latency_histogram_distance(summ, (i, 0), (j, 0))
            a, b = entries[i], entries[j]
            if not len(a) or not len(b):
                assert math.isnan(got["d"]) and got["den"] == 0
                continue
            ks = max(abs(Fraction(int((a <= k).sum()), len(a)) - Fraction(int((b <= k).sum()), len(b))) for k in range(-1, (16 << 3) + 1))
            assert isinstance(got["num"], int) and isinstance(got["den"], int) and got["den"] == len(a) * len(b)
            assert Fraction(got["num"], got["den"]) == ks and got["d"] == got["num"] / got["den"]
    assert latency_histogram_distance(summ, (0, 0), (0, 0))["d"] == 0.0
    assert 0.0 < latency_histogram_distance(summ, (0, 0), (2, 0))["d"] < latency_histogram_distance(summ, (0, 0), (1, 0))["d"] < 1.0
    pairs = latency_histogram_distance(summ, [[0, 0], [1, 0], [5, 0]], [[1, 0], [0, 0], [0, 0]])
    assert pairs["d"].shape == (3,) and pairs["d"][0] == pairs["d"][1] and math.isnan(pairs["d"][2]) and pairs["num"].dtype == object
    big = _summary([[_rows_of([0.1])], [_rows_of([0.2])]])
    big["hist"] = big["hist"] * (2 ** 40)                                           # counts whose products pass 2^64: exact integers
    got = latency_histogram_distance(big, (0, 0), (1, 0))
    assert got["num"] == got["den"] == 2 ** 80 and got["d"] == 1.0


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_host_surface():
    ck = np.array([[0.0, 1.0]])
    for bad in ((9, -20, 1), (-1, -20, 1), (5, -1023, 4), (5, -20, 0), (5, 1000, 24), (5, -20, 129), (0, -1022, 4097), (8, 0, 17),
                (5.0, -20, 32), (5, -20.0, 32), (5, -20, True), (None, -20, 32)):
        for call in (lambda: check_latency_bins(*bad), lambda: latency_bin_edges(*bad), lambda: latency_bin_index([1.0], *bad),
                     lambda: latency_histogram([ck], sub_bits=bad[0], min_exp=bad[1], octaves=bad[2])):
            with pytest.raises(ValueError, match="sub_bits|min_exp|octaves"):
                call()
    assert check_latency_bins(0, -1022, 2045) == (0, -1022, 2045, 2045) and check_latency_bins(8, 1007, 16)[3] == 4096
    with pytest.raises(ValueError, match="arrival"):
        latency_histogram([ck], None, "arrival")
    with pytest.raises(ValueError, match="window_of"):
        latency_histogram([ck], [0.0, 1.0], "start")
    for edges in ([0.0], [0.0, 0.0], [1.0, 0.0], [0.0, np.inf], [0.0, np.nan]):
        with pytest.raises(ValueError, match="edges"):
            latency_histogram([ck], edges)
    a = _summary([[ck], [ck]], [0.0, 1.0, 2.0])
    for other, what in ((_summary([[ck], [ck]], [0.0, 1.0, 2.0], binning=(4, -20, 32)), "sub_bits"),
                        (_summary([[ck], [ck]], [0.0, 1.0, 2.0], binning=(5, -19, 32)), "min_exp"),
                        (_summary([[ck], [ck]], [0.0, 1.0, 2.0], binning=(5, -20, 31)), "octaves"),
                        (_summary([[ck], [ck]], [0.0, 1.0, 2.5]), "edges"), (_summary([[ck], [ck]]), "edges"),
                        (_summary([[ck], [ck]], [0.0, 1.0, 2.0], "arrival"), "window_of"), (_summary([[ck]], [0.0, 1.0, 2.0]), "groups")):
        with pytest.raises(ValueError, match=what):
            latency_histogram_merge(a, other)
        with pytest.raises(ValueError, match=what):
            latency_histogram_merge(a, a, other)
    broken = dict(a, hist=a["hist"][:, :1])
    with pytest.raises(ValueError, match="not a latency histogram summary"):
        latency_histogram_quantiles(broken, [0.5])
    for levels in ([-0.1], [1.5], [np.nan]):
        with pytest.raises(ValueError, match="levels"):
            latency_histogram_quantiles(a, levels)
    for groups in ([0], [0, 1, 2], [-1, -1], [0.0, 1.0]):
        with pytest.raises(ValueError, match="groups"):
            latency_histogram_regroup(a, groups=groups)
    for windows in ([], [(0, 0)], [(0, 3)], [(1, 2), (0, 1)], [(0, 1), (0, 2)], [(-1, 1)]):
        with pytest.raises(ValueError, match="windows"):
            latency_histogram_regroup(a, windows=windows)
    for pa, pb in (((0, 0), (2, 0)), ((0, 2), (0, 0)), ((0, -1), (0, 0)), ((0, 0, 0), (0, 0, 0)), ([[0, 0]], (0, 0))):
        with pytest.raises(ValueError, match="pair"):
            latency_histogram_distance(a, pa, pb)
    with pytest.raises(ValueError, match="parameter columns"):
        groups_of_columns([])
    with pytest.raises(ValueError, match="parameter columns"):
        groups_of_columns([[1.0, 2.0], [1.0]])
    sharded = ShardedResults.__new__(ShardedResults)                                # the existing refusals stay
    for call in (sharded.window_summary, sharded.quantile_summary, sharded.exemplar_summary, sharded.pooled_summary):
        with pytest.raises(NotImplementedError, match="several devices"):
            call()


def test_parameter_columns_resolve_to_the_grids_points():
    users, rpm = "rqs_input.avg_active_users.mean", "rqs_input.avg_request_per_minute_per_user.mean"
    grid = expand_grid({users: [40.0, 90.0, 200.0], rpm: [10.0, 30.0]}, replicas=3, order_by_load=users)
    cols = grid.columns
    ids, n_groups = groups_of_columns([cols[users], cols[rpm]])
    assert n_groups == 6 and np.array_equal(ids, np.asarray(grid.point))
    ids, n_groups = groups_of_columns([cols[users]])
    assert n_groups == 3 and np.array_equal(ids, np.asarray(grid.point) // 2)


def test_a_scenario_gives_its_own_histogram():
    plan, clock = _fixture("lb2_events_t60")
    counts = np.zeros(_abi.CNT_SLOTS, dtype=np.uint32)
    counts[_abi.CNT_COMPLETED] = clock.shape[0]
    res = ScenarioResults(plan, counts, clock, None)
    got = res.get_latency_histogram()
    assert got["hist"].shape == (1, 1024) and got["hist"].dtype == np.int64 and got["edges"] is None and int(got["count"][0]) == clock.shape[0]
    assert np.array_equal(got["hist"], latency_histogram([clock])["hist"]) and got["bin_edges"].shape == (1025,)
    per = res.get_latency_histogram(window_s=10.0, window_of="arrival", sub_bits=3, min_exp=-12, octaves=12)
    assert per["hist"].shape == (6, 96) and per["window_of"] == "arrival" and (per["sub_bits"], per["min_exp"], per["octaves"]) == (3, -12, 12)
    want = latency_histogram([clock], np.arange(0.0, 61.0, 10.0), "arrival", sub_bits=3, min_exp=-12, octaves=12)
    assert np.array_equal(per["hist"], want["hist"]) and np.array_equal(per["count"], want["count"].astype(np.int64))
    q = latency_histogram_quantiles({**{k: v[None] for k, v in got.items() if k in ("hist", "count", "under", "over", "nan")},
                                     **{k: got[k] for k in ("edges", "window_of", "sub_bits", "min_exp", "octaves")}, "replicas": np.array([1])}, [0.5, 0.99])
    lat = clock[:, 1] - clock[:, 0]
    assert ((q["lo"][0, 0] <= np.quantile(lat, [0.5, 0.99])) & (np.quantile(lat, [0.5, 0.99]) < q["hi"][0, 0])).all()
    with pytest.raises(ValueError, match="arrival"):
        res.get_latency_histogram(window_of="arrival")
