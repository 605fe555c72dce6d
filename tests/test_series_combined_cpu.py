"""Combinations across the sampled series per tick (fleet totals, imbalance), CPU side: the C entry point and its struct, the
host definition (results.series_combined_values / series_combined_window_stats) against a per-row loop in plain Python, the
identities with series_window_stats, series_window_histogram and np.quantile, the refusals of the Python layer, and the bands
and the on-disk summary of a batch whose device call is replaced by the host definition.  Integers are compared with ==, floats
on their bits; only the bands' means over the replicas, sums of floats, are held to 1e-12."""

from __future__ import annotations

import ctypes as C
import math
import re
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import asyncflow_amd
from asyncflow_amd import _abi
from asyncflow_amd import build as af_build
from asyncflow_amd.plan import lower
from asyncflow_amd.results import (BatchedResults, ScenarioResults, ShardedResults, check_series_combinations, load_summary,
                                   series_combined_values, series_combined_window_stats, series_histogram_quantiles,
                                   series_names_of, series_window_histogram, series_window_stats)
from oracle.scenarios import lb_two_servers

ROOT = Path(__file__).resolve().parent.parent
N_EDGES = 2                        # the synthetic scenario: two edges, three servers -> 2 + 9 columns
S = 11
RAM = np.array([j >= N_EDGES and (j - N_EDGES) % 3 == 2 for j in range(S)])
INT_COLS = [int(j) for j in np.nonzero(~RAM)[0]]
RAM_COLS = [int(j) for j in np.nonzero(RAM)[0]]
RESIDUE = np.float32(-(2.0 ** -45))
OPS = ("sum", "min", "max", "spread")
FIELDS = ["n_scenarios", "n_groups", "n_windows", "group", "tick_edges", "n_combos", "op", "col_start", "cols", "thresholds",
          "n_bins", "lo", "width", "count", "mean", "minv", "maxv", "above", "hist", "under", "over", "elapsed_ms", "scratch_bytes"]


@pytest.fixture(scope="module")
def lib():
    af_build.build()
    from asyncflow_amd.engine import load_library

    return load_library()


# ------------------------------------------------------------------------------------ the entry and its struct
def test_header_declares_and_library_exports_the_entry(lib):
    header = (ROOT / "include" / "asyncflow_hip.h").read_text()
    assert re.search(r"int\s+af_engine_summarize_series_combined\s*\(\s*af_engine_t\s*\*", header)
    assert re.search(r"#define\s+AF_MAX_SERIES_COMBINATIONS\s+64\b", header) and _abi.MAX_SERIES_COMBINATIONS == 64
    assert re.search(r"AF_COMBINE_SUM = 0, AF_COMBINE_MIN = 1, AF_COMBINE_MAX = 2, AF_COMBINE_SPREAD = 3", header)
    assert _abi.COMBINE_OPS == {"sum": 0, "min": 1, "max": 2, "spread": 3}
    assert "af_engine_summarize_series_combined" in _abi.EXPORTED_SYMBOLS
    assert lib.af_engine_summarize_series_combined.argtypes[2] is C.POINTER(_abi.AfSeriesCombined)
    assert lib.af_abi_version() == 7
    assert asyncflow_amd.check_series_combinations is check_series_combinations
    assert asyncflow_amd.series_combined_values is series_combined_values
    assert asyncflow_amd.series_combined_window_stats is series_combined_window_stats
    for listing in ((ROOT / "asyncflow_amd" / "build.py").read_text(), (ROOT / "asyncflow_amd" / "jit.py").read_text()):
        assert '"af_series_combined.hpp"' in listing
    assert '#include "af_series_combined.hpp"' in (ROOT / "asyncflow_amd" / "csrc" / "engine.hip").read_text()


def test_af_series_combined_layout_matches_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "a host C compiler is needed for the layout probe"
    assert [name for name, _ in _abi.AfSeriesCombined._fields_] == FIELDS  # noqa: SLF001
    src = tmp_path / "probe.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "asyncflow_hip.h"\n'
        'int main(void) { printf("%zu", sizeof(af_series_combined_t));\n'
        + "".join(f'printf(" %zu", offsetof(af_series_combined_t, {f}));\n' for f in FIELDS)
        + 'printf(" %d %d %d %d %d\\n", AF_MAX_SERIES_COMBINATIONS, AF_COMBINE_SUM, AF_COMBINE_MIN, AF_COMBINE_MAX, AF_COMBINE_SPREAD); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run([cc, "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    P = _abi.AfSeriesCombined
    assert got == [C.sizeof(P), *(getattr(P, f).offset for f in FIELDS), _abi.MAX_SERIES_COMBINATIONS, 0, 1, 2, 3]
    body = re.search(r"typedef struct af_series_combined \{(.*?)\} af_series_combined_t;", (ROOT / "include" / "asyncflow_hip.h").read_text(), re.S)
    assert body and re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S)) == FIELDS


def test_series_combined_entry_refuses_without_a_device(lib):
    from asyncflow_amd.engine import PLAN_ONLY, Engine, EngineUnavailableError

    eng = Engine(lower(lb_two_servers(horizon=20)), PLAN_ONLY)
    try:
        out = _abi.AfOutputs(0, None, 4, None, None)
        edges = (C.c_uint32 * 3)(0, 1, 2)
        op, start, cols = (C.c_uint32 * 1)(0), (C.c_uint32 * 2)(0, 2), (C.c_uint32 * 2)(0, 1)
        req = _abi.AfSeriesCombined(4, 1, 2, None, edges, 1, op, start, cols, None, 0, None, None, None, None, None, None, None,
                                    None, None, None, 0.0, 0)
        call = lib.af_engine_summarize_series_combined
        assert call(None, C.byref(out), C.byref(req)) == _abi.AF_ERR_INVALID
        assert call(eng._h, None, C.byref(req)) == _abi.AF_ERR_INVALID  # noqa: SLF001
        assert call(eng._h, C.byref(out), None) == _abi.AF_ERR_INVALID  # noqa: SLF001
        assert call(eng._h, C.byref(out), C.byref(req)) == _abi.AF_ERR_NO_DEVICE  # noqa: SLF001
        assert b"planning-only" in lib.af_last_error()
        kw = {"samples_ptr": 0, "tick_capacity": 4, "counts_ptr": 0, "mean_ptr": 0}
        with pytest.raises(EngineUnavailableError, match="planning-only"):
            eng.summarize_series_combined(4, 1, [0, 2, 4], [0], [[0, 1]], **kw)
        # a bad request never reaches the library
        for bad, what in (([0], "at least two"), ([0, 2, 2], "strictly increasing"), ([0.5, 2], "whole")):
            with pytest.raises(ValueError, match=what):
                eng.summarize_series_combined(4, 1, bad, [0], [[0, 1]], **kw)
        with pytest.raises(ValueError, match="ops for"):
            eng.summarize_series_combined(4, 1, [0, 4], [0, 1], [[0, 1]], **kw)
        with pytest.raises(ValueError, match="thresholds"):
            eng.summarize_series_combined(4, 1, [0, 4], [0], [[0, 1]], thresholds=[0.0, 1.0], **kw)
        for bins in (1025, 2.5, True):
            with pytest.raises(ValueError, match="bins"):
                eng.summarize_series_combined(4, 1, [0, 4], [0], [[0, 1]], bins=bins, **kw)
        with pytest.raises(ValueError, match="width"):
            eng.summarize_series_combined(4, 1, [0, 4], [0], [[0, 1]], bins=8, width=0.0, **kw)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------ the host definition and a plain loop
def _f32(word: int) -> float:
    return struct.unpack("<f", struct.pack("<I", int(word)))[0]       # (a Python float: the float64 of the float32 value)


def _order(x: float) -> tuple:
    """A sort key of the IEEE total order on the non-NaN doubles: -0.0 below +0.0."""
    return (x, 0 if math.copysign(1.0, x) < 0 else 1)


def _loop_value(words, k: int, op: str, cols) -> float | int:
    """The header's per-tick value of one row in plain Python: ints exactly, floats one addition at a time."""
    if not RAM[cols[0]]:
        ws = [int(words[j, k]) for j in cols]
        return {"sum": sum(ws), "min": min(ws), "max": max(ws), "spread": max(ws) - min(ws)}[op]
    xs = [_f32(words[j, k]) for j in cols]
    if op == "sum":
        acc = xs[0]
        for x in xs[1:]:
            acc = acc + x
        return acc
    mn, mx = min(xs, key=_order), max(xs, key=_order)
    return mn if op == "min" else mx if op == "max" else mx - mn


def _loop(words, edges, combos, thr, bins, lo, width):
    ticks = words.shape[1]
    W, Cn = len(edges) - 1, len(combos)
    out = {"count": np.zeros(W, dtype=np.int64), "mean": np.full((W, Cn), np.nan), "min": np.full((W, Cn), np.nan),
           "max": np.full((W, Cn), np.nan), "above": np.zeros((W, Cn), dtype=np.int64), "hist": np.zeros((W, Cn, bins), dtype=np.int64),
           "under": np.zeros((W, Cn), dtype=np.int64), "over": np.zeros((W, Cn), dtype=np.int64)}
    for w in range(W):
        r0, r1 = min(edges[w], ticks), min(edges[w + 1], ticks)
        out["count"][w] = r1 - r0
        for c, (op, cols) in enumerate(combos):
            vs = [_loop_value(words, k, op, cols) for k in range(r0, r1)]
            if not vs:
                continue
            xs = [float(v) for v in vs]
            out["mean"][w, c] = (0.0 + math.fsum(vs) if RAM[cols[0]] else float(sum(vs))) / float(len(vs))
            out["min"][w, c], out["max"][w, c] = min(xs, key=_order), max(xs, key=_order)
            out["above"][w, c] = sum(x > thr[c] for x in xs)
            for x in xs:
                if x < lo[c]:
                    out["under"][w, c] += 1
                    continue
                t = (x - lo[c]) / width[c]
                if t >= float(bins):
                    out["over"][w, c] += 1
                else:
                    out["hist"][w, c, math.floor(t)] += 1
    return out


def _words(rng, ticks: int, top: int = 40, big: bool = False) -> np.ndarray:
    """Words [S, ticks]: integer columns with half of their mass at 0 (or, big, words that reach 2^32 - 1, so that sums of
    three columns pass 2^32); ram columns of multiples of 1/256 with -0.0, +0.0 and the -2^-45 residue among them."""
    words = np.zeros((S, ticks), dtype=np.uint32)
    for j in INT_COLS:
        u = rng.random(ticks)
        v = np.where(u < 0.5, 0, rng.integers(0, top, ticks))
        if big:
            v = np.where(u < 0.3, 0xFFFFFFFF, rng.integers(2 ** 31, 2 ** 32, ticks))
        words[j] = v.astype(np.uint32)
    for j in RAM_COLS:
        f = (rng.integers(-2 * 256, top * 256, ticks) / 256.0).astype(np.float32)
        u = rng.random(ticks)
        f[u < 0.25] = np.float32(-0.0)
        f[(u >= 0.25) & (u < 0.45)] = np.float32(0.0)
        f[(u >= 0.45) & (u < 0.55)] = RESIDUE
        words[j] = f.view(np.uint32)
    return words


def _combos():
    sets = [[INT_COLS[0]], INT_COLS[:2], [INT_COLS[0], INT_COLS[-1]], INT_COLS, INT_COLS[::3], [RAM_COLS[1]], RAM_COLS, RAM_COLS[::2]]
    return [(op, cols) for cols in sets for op in OPS]


def _bits(a) -> bytes:
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def _same(got, want, what):
    for k in ("count", "above", "hist", "under", "over"):
        assert np.array_equal(np.asarray(got[k], dtype=np.int64), want[k]), (what, k)
    for k in ("mean", "min", "max"):
        assert got[k].dtype == np.float64 and _bits(got[k]) == _bits(want[k]), (what, k, got[k], want[k])
    assert np.array_equal(got["under"] + got["hist"].sum(axis=-1) + got["over"], np.broadcast_to(got["count"][:, None], got["under"].shape)), what


@pytest.mark.parametrize("big", [False, True])
def test_host_definition_equals_a_loop_over_the_rows(big):
    rng = np.random.default_rng(5 + big)
    ticks = 130
    edges = [0, 1, 2, 50, 51, 120, 129, 130, 131, 400]
    words = _words(rng, ticks, big=big)
    combos = _combos()
    Cn = len(combos)
    thr = [(0.0, 1.0, 0.5, -1.0, 2.0 ** 32)[c % 5] for c in range(Cn)]
    lo = [(0.0, 2.0, -1.0, 0.5)[c % 4] for c in range(Cn)]
    width = [(1.0, 3.0, 0.25, 0.1, 1.0 / 3.0)[c % 5] for c in range(Cn)]
    got = series_combined_window_stats(words, edges, N_EDGES, combos, thr, 16, lo, width)
    _same(got, _loop(words, edges, combos, thr, 16, lo, width), f"big={big}")
    assert got["count"].tolist() == [1, 1, 48, 1, 69, 9, 1, 0, 0] and np.isnan(got["mean"][-2:]).all() and not got["above"][-2:].any()
    assert got["ram"].tolist() == [bool(RAM[c[1][0]]) for c in combos]
    # the per-tick values: exact integers past 2^32, floats in the stated order
    for c, (op, cols) in enumerate(combos):
        v = series_combined_values(words, N_EDGES, op, cols)
        assert v.dtype == (np.float64 if RAM[cols[0]] else np.uint64) and v.shape == (ticks,)
        want = [_loop_value(words, k, op, cols) for k in range(ticks)]
        if RAM[cols[0]]:
            assert _bits(v) == _bits(want), (op, cols)
        else:
            assert [int(x) for x in v] == want, (op, cols)
    if big:
        assert int(series_combined_values(words, N_EDGES, "sum", INT_COLS).max()) > 2 ** 34
    # the sign of a zero: the sum of -0.0s is -0.0, the smallest of {-0.0, +0.0} is -0.0, a zero mean is +0.0
    z = np.zeros((S, 4), dtype=np.uint32)
    z[RAM_COLS[0]] = 0x80000000
    z[RAM_COLS[1], :2] = 0x80000000
    assert np.signbit(series_combined_values(z, N_EDGES, "sum", RAM_COLS[:2])).tolist() == [True, True, False, False]
    assert np.signbit(series_combined_values(z, N_EDGES, "min", RAM_COLS)).all()
    assert not np.signbit(series_combined_values(z, N_EDGES, "max", RAM_COLS)).any()
    one = series_combined_window_stats(z, [0, 4], N_EDGES, [("sum", RAM_COLS[:1]), ("min", RAM_COLS)])
    assert not np.signbit(one["mean"]).any() and np.signbit(one["min"]).all() and np.signbit(one["max"][0, 0]) and one["above"].sum() == 0


# ------------------------------------------------------------------------------------ identities
def test_one_column_is_the_series_window_statistic():
    rng = np.random.default_rng(11)
    ticks = 300
    words = _words(rng, ticks, top=20)
    words[words == RESIDUE.view(np.uint32)] = np.float32(0.25).view(np.uint32)   # (every partial sum exact: np.mean is the exact mean)
    edges = [0, 7, 150, 299, 300, 310]
    thr = np.array([(0.0, 3.0, 0.5)[j % 3] for j in range(S)])
    base = series_window_stats(words, edges, N_EDGES, thr)
    full = base["count"] > 0
    for j in range(S):
        got = series_combined_window_stats(words, edges, N_EDGES, [(op, [j]) for op in OPS], np.full(4, thr[j]), 24, -1.0, 1.0)
        assert np.array_equal(got["count"], base["count"])
        decode = (lambda w: w.view(np.float32).astype(np.float64)) if RAM[j] else (lambda w: w.astype(np.float64))
        for c in range(3):                                               # sum, min, max of one column are the column
            assert _bits(got["mean"][full, c]) == _bits(base["mean"][full, j]), j
            assert _bits(got["min"][full, c]) == _bits(decode(base["min"][full, j])) and _bits(got["max"][full, c]) == _bits(decode(base["max"][full, j]))
            assert np.array_equal(got["above"][:, c], base["above"][:, j].astype(np.int64))
        assert (got["mean"][full, 3] == 0).all() and (got["max"][full, 3] == 0).all() and not got["above"][:, 3].any()   # spread: 0
        assert not np.signbit(got["max"][full, 3]).any()
        h = series_window_histogram(words, edges, N_EDGES, 24, [j], -1.0, 1.0)
        for c in range(3):
            for k in ("hist", "under", "over"):
                assert np.array_equal(got[k][:, c], h[k][:, 0]), (j, k)
        assert np.array_equal(got["bin_edges"][0], h["bin_edges"][0])


def test_quantiles_from_the_histogram_are_np_quantile_of_the_values():
    rng = np.random.default_rng(12)
    ticks = 400
    words = _words(rng, ticks, top=12)
    edges = [0, 1, 3, 100, 101, 399, 400, 450]
    levels = np.concatenate([np.linspace(0.0, 1.0, 21), [0.001, 0.5, 0.999, 0.95]])
    combos = [(op, cols) for cols in (INT_COLS, INT_COLS[:2], INT_COLS[::3]) for op in OPS]
    got = series_combined_window_stats(words, edges, N_EDGES, combos, None, 128)
    assert not got["under"].any() and not got["over"].any() and not got["ram"].any()
    q = series_histogram_quantiles(got, levels)
    assert q.shape == (7, len(combos), len(levels)) and np.isnan(q[-1]).all()
    for c, (op, cols) in enumerate(combos):
        v = series_combined_values(words, N_EDGES, op, cols).astype(np.float64)
        for w in range(6):
            want = np.quantile(v[edges[w]:min(edges[w + 1], ticks)], levels)
            assert _bits(q[w, c]) == _bits(want), (op, cols, w)
    with pytest.raises(ValueError, match="ram_in_use"):
        series_histogram_quantiles(series_combined_window_stats(words, edges, N_EDGES, [("sum", RAM_COLS)], None, 8), [0.5])


# ------------------------------------------------------------------------------------ the Python layer
def test_check_series_combinations():
    plan = lower(lb_two_servers(horizon=10))
    names = series_names_of(plan)
    ne = plan.n_edges
    queue = [j for j, k in enumerate(names) if k.endswith(":ready_queue_len")]
    ram = [j for j, k in enumerate(names) if k.endswith(":ram_in_use")]
    labels, ops, cols = check_series_combinations(
        {"imbalance": ("spread", "*:ready_queue_len"), "fleet_ram": ("sum", "*:ram_in_use"), "two": ("max", [names[queue[1]], names[queue[0]]]),
         "idx": ("min", np.array([3, 0])), "pats": ("sum", ["*:ready_queue_len", "*queue*", "*:event_loop_io_sleep"])}, names, ne)
    assert labels == ["imbalance", "fleet_ram", "two", "idx", "pats"] and ops == ["spread", "sum", "max", "min", "sum"]
    assert cols[0].tolist() == queue and cols[1].tolist() == ram and cols[2].tolist() == queue and cols[3].tolist() == [0, 3]
    assert cols[4].tolist() == sorted(queue + [j for j, k in enumerate(names) if k.endswith(":event_loop_io_sleep")])
    assert all(c.dtype == np.int64 for c in cols) and len(queue) == 2
    pairs = check_series_combinations([("a", ("sum", [0])), ("b", ("sum", [0]))], names, ne)
    assert pairs[0] == ["a", "b"]
    for bad, what in (({}, "1 .. 64"), ({str(i): ("sum", [0]) for i in range(65)}, "1 .. 64"),
                      ({"x": ("mean", [0])}, "unknown op"), ({"x": ("sum", "*:nothing")}, "matches no series"),
                      ({"x": ("sum", ["nobody:ram_in_use"])}, "unknown series"), ({"x": ("sum", [])}, "selects no series"),
                      ({"x": ("sum", [0, 0])}, "twice"), ({"x": ("sum", [len(names)])}, "no series name"), ({"x": ("sum", [-1])}, "no series name"),
                      ({"x": ("sum", [0.5])}, "no series name"), ({"x": ("sum", [True])}, "no series name"),
                      ({"x": ("sum", [queue[0], ram[0]])}, "mixes"), ({"x": ("sum", "*")}, "mixes"), ({"x": "sum"}, r"\(op, selection\)"),
                      ([("a", ("sum", [0])), ("a", ("max", [1]))], "given twice")):
        with pytest.raises(ValueError, match=what):
            check_series_combinations(bad, names, ne)


def test_host_definition_refusals():
    words = np.zeros((S, 10), dtype=np.uint32)
    ok = [("sum", INT_COLS[:2])]
    with pytest.raises(ValueError, match="strictly increasing"):
        series_combined_window_stats(words, [0, 5, 5], N_EDGES, ok)
    for bad, what in (([("avg", [0])], "unknown op"), ([("sum", [])], "non-empty"), ([("sum", [1, 0])], "strictly increasing"),
                      ([("sum", [0, 0])], "strictly increasing"), ([("sum", [0, S])], "strictly increasing"), ([("sum", [-1, 0])], "strictly increasing"),
                      ([("sum", [0.5])], "non-empty vector of series indices"), ([("sum", [INT_COLS[0], RAM_COLS[0]])], "mixes"),
                      ([], "1 .. 64"), (ok * 65, "1 .. 64")):
        with pytest.raises(ValueError, match=what):
            series_combined_window_stats(words, [0, 5], N_EDGES, bad)
    for thr in ([0.0, 1.0], [float("nan")]):
        with pytest.raises(ValueError, match="thresholds"):
            series_combined_window_stats(words, [0, 5], N_EDGES, ok, thr)
    with pytest.raises(ValueError, match="bins"):
        series_combined_window_stats(words, [0, 5], N_EDGES, ok, None, 1025)
    with pytest.raises(ValueError, match="bins"):
        series_combined_window_stats(words, [0, 5], N_EDGES, ok, None, 0, 0.0, 1.0)       # a binning without bins
    with pytest.raises(ValueError, match="width"):
        series_combined_window_stats(words, [0, 5], N_EDGES, ok, None, 8, 0.0, -1.0)
    with pytest.raises(ValueError, match="samples must be words"):
        series_combined_window_stats(np.zeros(10, dtype=np.uint32), [0, 5], N_EDGES, ok)
    with pytest.raises(ValueError, match="samples must be words"):
        series_combined_values(np.zeros(10, dtype=np.uint32), N_EDGES, "sum", [0])
    assert "hist" not in series_combined_window_stats(words, [0, 5], N_EDGES, ok)


def test_tick_edge_forms_of_a_scenario():
    plan = lower(lb_two_servers(horizon=10))
    rng = np.random.default_rng(3)
    ticks = plan.tick_count
    words = rng.integers(0, 50, (plan.n_series, ticks)).astype(np.uint32)
    res = ScenarioResults(plan, np.zeros(_abi.CNT_SLOTS, dtype=np.uint32), np.zeros((0, 2)), words)
    combos = {"imbalance": ("spread", "*:ready_queue_len"), "edges": ("sum", "*:edge_concurrent_connection")}
    per = int(round(2.0 / plan.sample_period))
    a = res.get_series_combined(combos, 2.0, bins=64)
    b = res.get_series_combined(combos, ticks_per_window=per, bins=64)
    c = res.get_series_combined(combos, tick_edges=a["tick_edges"], bins=64)
    assert a["mean"].shape == (-(-ticks // per), 2) and int(a["count"].sum()) == ticks and a["names"] == ["imbalance", "edges"]
    assert a["ops"] == ["spread", "sum"] and a["columns"][1].tolist() == list(range(plan.n_edges))
    for other in (b, c):
        assert all(np.array_equal(other[k], a[k]) for k in ("count", "mean", "min", "max", "above", "hist", "under", "over"))
    names = series_names_of(plan)
    q0, q1 = (words[j].astype(np.int64) for j, k in enumerate(names) if k.endswith(":ready_queue_len"))
    assert a["max"][0, 0] == float(np.abs(q0 - q1)[:per].max())
    with pytest.raises(ValueError, match="one of"):
        res.get_series_combined(combos, 2.0, ticks_per_window=per)
    none = ScenarioResults(plan, res.counts, np.zeros((0, 2)), None)
    with pytest.raises(RuntimeError, match="kept no sampled series"):
        none.get_series_combined(combos)


def test_refusals_of_the_batch_layer():
    plan = lower(lb_two_servers(horizon=10))
    batch = BatchedResults.__new__(BatchedResults)
    batch.plan = plan
    batch._samples_t = None  # noqa: SLF001
    ok = {"q": ("sum", "*:ready_queue_len")}
    for call in (batch.series_combined_summary, batch.series_combined_bands):
        with pytest.raises(RuntimeError, match="kept no sampled series"):
            call(ok)
    with pytest.raises(RuntimeError, match="kept no sampled series"):
        batch.save_series_combined_summary("nowhere.npz", combos=ok, ticks_per_window=10)
    batch._samples_t = object()  # noqa: SLF001  (the checks below come before the device is touched)
    with pytest.raises(ValueError, match="unknown op"):
        batch.series_combined_summary({"q": ("avg", "*:ready_queue_len")})
    with pytest.raises(ValueError, match="matches no series"):
        batch.series_combined_summary({"q": ("sum", "*:nothing")})
    with pytest.raises(ValueError, match="mixes"):
        batch.series_combined_summary({"q": ("sum", ["*:ready_queue_len", "*:ram_in_use"])})
    with pytest.raises(ValueError, match="unknown combination 'nobody' in thresholds"):
        batch.series_combined_summary(ok, thresholds={"nobody": 1.0})
    with pytest.raises(ValueError, match="thresholds"):
        batch.series_combined_summary(ok, thresholds=[1.0, 2.0])
    with pytest.raises(ValueError, match="thresholds"):
        batch.series_combined_summary(ok, thresholds={"q": float("nan")})
    with pytest.raises(ValueError, match="bins"):
        batch.series_combined_summary(ok, bins=1025)
    with pytest.raises(ValueError, match="width must be above 0"):
        batch.series_combined_summary(ok, bins=8, width=0.0)
    with pytest.raises(ValueError, match="one of"):
        batch.series_combined_summary(ok, 1.0, ticks_per_window=10)
    with pytest.raises(ValueError, match="of must be"):
        batch.series_combined_bands(ok, of="median")
    assert batch._combined_thresholds({"b": 2.0}, ["a", "b"]).tolist() == [0.0, 2.0]  # noqa: SLF001


def test_sharded_results_refuse_series_combinations():
    sh = ShardedResults.__new__(ShardedResults)
    for call in (sh.series_combined_summary, sh.series_combined_bands, sh.save_series_combined_summary):
        with pytest.raises(NotImplementedError, match="several devices"):
            call({})


# ------------------------------------------------------------------------------------ bands and the on-disk summary
def _pooled_host(words_of, ids, n_groups, b, n_edges, pairs, thr, bins, lo, width):
    """The host definition of a group: series_combined_window_stats of its members' rows, window by window side by side --
    integer outputs added up, min / max taken, the mean from the members' exact sums."""
    W, Cn = len(b) - 1, len(pairs)
    out = {"count": np.zeros((n_groups, W), dtype=np.int64), "above": np.zeros((n_groups, W, Cn), dtype=np.int64),
           "mean": np.full((n_groups, W, Cn), np.nan), "min": np.full((n_groups, W, Cn), np.nan), "max": np.full((n_groups, W, Cn), np.nan)}
    if bins:
        out.update(hist=np.zeros((n_groups, W, Cn, bins), dtype=np.int64), under=np.zeros((n_groups, W, Cn), dtype=np.int64),
                   over=np.zeros((n_groups, W, Cn), dtype=np.int64))
    sums = [[[[] for _ in range(Cn)] for _ in range(W)] for _ in range(n_groups)]
    one = None
    for s, g in enumerate(ids):
        if g < 0:
            continue
        one = series_combined_window_stats(words_of[s], b, n_edges, pairs, thr, bins, lo, width)
        for k in ("count", "above", "hist", "under", "over"):
            if k in out:
                out[k][g] += one[k]
        out["min"][g] = np.fmin(out["min"][g], one["min"])
        out["max"][g] = np.fmax(out["max"][g], one["max"])
        r = np.minimum(b.astype(np.int64), words_of[s].shape[1])
        for c, (op, col) in enumerate(pairs):
            v = series_combined_values(words_of[s], n_edges, op, col)
            for w in range(W):
                sums[g][w][c] += v[r[w]:r[w + 1]].tolist()
    for g in range(n_groups):
        for w in range(W):
            for c in range(Cn):
                vs = sums[g][w][c]
                if vs:
                    out["mean"][g, w, c] = (math.fsum(vs) if isinstance(vs[0], float) else float(sum(vs))) / float(len(vs))
    return out, one


class _HostBatch(BatchedResults):
    """A batch of host arrays whose combined call is the host definition, group by group."""

    def series_combined_summary(self, combos, window_s=None, *, ticks_per_window=None, tick_edges=None, by=None, thresholds=None,
                                bins=0, lo=None, width=None):
        import torch

        labels, ops, columns = check_series_combinations(combos, self.series_names(), self.plan.n_edges)
        thr = self._combined_thresholds(thresholds, labels)
        b = self._series_tick_edges(window_s, ticks_per_window, tick_edges)
        ids, n_groups = self._window_groups(by)
        out, one = _pooled_host(self.host_words, ids, n_groups, b, self.plan.n_edges, list(zip(ops, columns)), thr, bins, lo, width)
        res = {k: torch.as_tensor(v) for k, v in out.items()}
        res["above_share"] = res["above"].to(torch.float64) / res["count"].to(torch.float64)[:, :, None]
        if bins:
            res.update(bin_edges=one["bin_edges"], ram=one["ram"])
        res.update(names=labels, ops=ops, columns=columns, tick_edges=b, times=b[:-1].astype(np.float64) * self.plan.sample_period,
                   replicas=np.bincount(ids[ids >= 0], minlength=n_groups), series_combined_ms=0.0, scratch_bytes=0)
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
    words = np.where(rng.random((n, plan.n_series, ticks)) < 0.6, 0, rng.integers(0, 40, (n, plan.n_series, ticks))).astype(np.uint32)
    ram = np.array([k.endswith(":ram_in_use") for k in series_names_of(plan)])
    words[:, ram] = (rng.integers(0, 2 ** 16, (n, int(ram.sum()), ticks)) / 256.0).astype(np.float32).view(np.uint32)
    batch.host_words = words
    return batch, np.array([0, 1, 0, 1, -1, 1])


COMBOS = {"imbalance": ("spread", "*:ready_queue_len"), "fleet_ram": ("sum", "*:ram_in_use"), "queued": ("sum", "*:ready_queue_len")}


@pytest.mark.parametrize("ext", ["npz", "parquet"])
def test_on_disk_round_trip(tmp_path, ext):
    if ext == "parquet":
        pytest.importorskip("pyarrow")
    batch, ids = _host_batch()
    path = str(tmp_path / f"series_combined.{ext}")
    written = batch.save_series_combined_summary(path, ids, combos=COMBOS, thresholds={"queued": 20.0}, bins=32, lo=0.0, width=4.0,
                                                 ticks_per_window=50)
    back = load_summary(path)
    assert set(back) == set(written)
    for k, v in written.items():
        assert np.array_equal(np.asarray(back[k], dtype=v.dtype), v, equal_nan=True), k
    W = -(-batch.plan.tick_count // 50)
    want = batch.series_combined_summary(COMBOS, ticks_per_window=50, by=ids, thresholds={"queued": 20.0}, bins=32, lo=0.0, width=4.0)
    bands = batch.series_combined_bands(COMBOS, ticks_per_window=50, by=ids, thresholds={"queued": 20.0})
    assert back["replicas"].tolist() == [2, 3] and np.array_equal(back["series_combined_count"], want["count"].numpy())
    for c, name in enumerate(COMBOS):
        assert back[f"series_combined_mean:{name}"].shape == (2, W)
        for key, k in (("mean", "mean"), ("min", "min"), ("max", "max"), ("above", "above_share")):
            assert _bits(back[f"series_combined_{key}:{name}"]) == _bits(want[k].numpy()[:, :, c]), (name, key)
        assert _bits(back[f"series_combined_q05:{name}"]) == _bits(bands["q_lo"][:, :, c]) and _bits(back[f"series_combined_q95:{name}"]) == _bits(bands["q_hi"][:, :, c])
        assert back[f"series_combined_hist:{name}"].shape == (2, W, 32) and np.array_equal(back[f"series_combined_hist:{name}"], want["hist"].numpy()[:, :, c])
        assert np.array_equal(back[f"series_combined_under:{name}"], want["under"].numpy()[:, :, c])
        assert np.array_equal(back[f"series_combined_over:{name}"], want["over"].numpy()[:, :, c])
        assert np.array_equal(back[f"series_combined_bin_edges:{name}"], 4.0 * np.arange(33.0))
    assert back["series_combined_above:queued"].max() > 0 and back["series_combined_over:fleet_ram"].sum() > 0
    assert np.array_equal(back["series_combined_tick_edges"], want["tick_edges"]) and np.array_equal(back["series_combined_times"], want["times"])
    plain = batch.save_series_combined_summary(str(tmp_path / f"plain.{ext}"), ids, combos=COMBOS, ticks_per_window=50)
    assert not any(k.startswith("series_combined_hist") for k in plain) and "series_combined_mean:queued" in plain


def test_bands_of_a_host_batch():
    batch, ids = _host_batch()
    per = batch.series_combined_summary(COMBOS, ticks_per_window=100, by="scenario")
    pooled = batch.series_combined_summary(COMBOS, ticks_per_window=100, by=ids)
    W = int(per["count"].shape[1])
    for of in ("mean", "max", "min", "above_share"):
        bands = batch.series_combined_bands(COMBOS, ticks_per_window=100, by=ids, of=of)
        assert bands["mean"].shape == bands["q_lo"].shape == bands["pooled"].shape == (2, W, 3) and bands["n"].shape == (2, W)
        assert _bits(bands["pooled"]) == _bits(pooled[of].numpy()) and bands["of"] == of
        for g in range(2):
            np.testing.assert_allclose(bands["mean"][g], per[of].numpy()[ids == g].mean(axis=0), rtol=1e-12, atol=1e-15)
            np.testing.assert_allclose(bands["q_hi"][g], np.quantile(per[of].numpy()[ids == g], 0.95, axis=0), rtol=1e-12, atol=1e-15)
        assert bands["replicas"].tolist() == [2, 3] and bands["names"] == list(COMBOS)
