"""Quantiles of the sampled series per window of ticks, CPU side: the C entry point and its struct, the host definition
(results.series_window_quantiles) against np.quantile -- bit for bit wherever a cell holds no zero, equal under ==
everywhere --, windowing, column selection, and the refusals of the Python layer."""

from __future__ import annotations

import ctypes as C
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
from asyncflow_amd.results import (BatchedResults, ScenarioResults, ShardedResults, check_series_levels, series_window_quantiles,
                                   series_window_stats)
from oracle.scenarios import lb_two_servers

ROOT = Path(__file__).resolve().parent.parent
N_EDGES = 1                       # the synthetic scenario: one edge, one server -> columns edge, ready, io, ram
LEVELS = (0.0, 0.001, 0.25, 0.5, 0.95, 0.99, 0.999, 1.0)
SIZES = (1, 2, 3, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 8193)
INT_RANGES = (1, 3, 40, 2048, 70000, 2 ** 32)
RAM_KINDS = ("dyadic", "residues", "zeros", "decades")


@pytest.fixture(scope="module")
def lib():
    af_build.build()
    from asyncflow_amd.engine import load_library

    return load_library()


def test_header_declares_and_library_exports_the_entry(lib):
    header = (ROOT / "include" / "asyncflow_hip.h").read_text()
    assert re.search(r"int\s+af_engine_summarize_series_quantiles\s*\(\s*af_engine_t\s*\*", header)
    assert re.search(r"#define\s+AF_MAX_SERIES_QUANTILE_LEVELS\s+16\b", header) and _abi.MAX_SERIES_QUANTILE_LEVELS == 16
    assert "af_engine_summarize_series_quantiles" in _abi.EXPORTED_SYMBOLS
    assert lib.af_engine_summarize_series_quantiles.argtypes[2] is C.POINTER(_abi.AfSeriesQuantiles)
    assert lib.af_abi_version() == 7
    assert asyncflow_amd.series_window_quantiles is series_window_quantiles


def test_af_series_quantiles_layout_matches_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "a host C compiler is needed for the layout probe"
    fields = [name for name, _ in _abi.AfSeriesQuantiles._fields_]  # noqa: SLF001
    assert fields == ["n_scenarios", "n_groups", "n_windows", "group", "tick_edges", "n_levels", "levels", "n_columns", "columns",
                      "count", "quantiles", "elapsed_ms", "scratch_bytes"]
    src = tmp_path / "probe.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "asyncflow_hip.h"\n'
        'int main(void) { printf("%zu", sizeof(af_series_quantiles_t));\n'
        + "".join(f'printf(" %zu", offsetof(af_series_quantiles_t, {f}));\n' for f in fields)
        + 'printf("\\n"); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run([cc, "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == C.sizeof(_abi.AfSeriesQuantiles) == 96
    assert got[1:] == [getattr(_abi.AfSeriesQuantiles, f).offset for f in fields]


# ------------------------------------------------------------------------------------ the host definition and np.quantile
def _integers(rng, n: int, span: int) -> np.ndarray:
    """n words over `span` consecutive values; the full 32 bits start at 0, the others at a base above 2^31 or below."""
    if span == 2 ** 32:
        v = rng.integers(0, 2 ** 32, n, dtype=np.uint64)
        v[: min(n, 2)] = [0, 2 ** 32 - 1][: min(n, 2)]
        return v.astype(np.uint32)
    base = 2 ** 31 - 5 if span in (40, 70000) else 7
    return (base + rng.integers(0, span, n)).astype(np.uint32)


def _ram(rng, n: int, kind: str) -> np.ndarray:
    if kind == "dyadic":
        return (rng.integers(0, 2 ** 24, n) / 256.0).astype(np.float32)
    if kind == "residues":
        v = (rng.integers(0, 2 ** 16, n) / 256.0 + 0.5).astype(np.float32)
        v[rng.random(n) < 0.3] = np.float32(-2.842171e-14)
        return v
    if kind == "zeros":
        v = (rng.integers(-2 ** 10, 2 ** 10, n) / 256.0).astype(np.float32)
        u = rng.random(n)
        v[u < 0.3] = np.float32(0.0)
        v[u > 0.7] = np.float32(-0.0)
        return v
    v = (10.0 ** rng.uniform(-20.0, 20.0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    assert np.isfinite(v).all() and (v != 0).all()
    return v


def _case(rng, n: int, span: int, kind: str) -> np.ndarray:
    """Words [4, n]: three integer columns over `span` values, a ram column of `kind`."""
    words = np.stack([_integers(rng, n, span) for _ in range(3)] + [_ram(rng, n, kind).view(np.uint32)])
    return np.ascontiguousarray(words)


@pytest.mark.parametrize("n", SIZES)
def test_host_definition_equals_np_quantile(n):
    rng = np.random.default_rng(n)
    q = np.array(LEVELS)
    cases = bit_equal = 0
    for i in range(max(len(INT_RANGES), len(RAM_KINDS))):
        span, kind = INT_RANGES[i % len(INT_RANGES)], RAM_KINDS[i % len(RAM_KINDS)]
        words = _case(rng, n, span, kind)
        count, quant = series_window_quantiles(words, [0, n], N_EDGES, q)
        assert count.tolist() == [n] and quant.shape == (1, 4, q.shape[0])
        values = words.astype(np.float64)
        values[3] = words[3].view(np.float32).astype(np.float64)
        for j in range(4):
            want = np.quantile(values[j], q)
            assert np.array_equal(quant[0, j], want), (n, span, kind, j)
            cases += 1
            if not (values[j] == 0).any():
                assert quant[0, j].tobytes() == want.tobytes(), (n, span, kind, j)
                bit_equal += 1
        # levels 0 and 1 are the window's float minimum and maximum as values (the formula adds d * t = +0.0 to a -0.0)
        st = series_window_stats(words, [0, n], N_EDGES)
        lo = np.where([False, False, False, True], st["min"][0].view(np.float32).astype(np.float64), st["min"][0].astype(np.float64))
        hi = np.where([False, False, False, True], st["max"][0].view(np.float32).astype(np.float64), st["max"][0].astype(np.float64))
        assert np.array_equal(quant[0, :, 0], lo) and np.array_equal(quant[0, :, -1], hi)
    assert cases == 24 and bit_equal >= 20


def test_signed_zeros_sort_by_key():
    """-0.0 lies below +0.0: (+0, -0, -0, +0) sorts to (-0, -0, +0, +0).  The formula shows the sign where the upper neighbour is
    taken (t >= 0.5: x[hi] - d * (1 - t) keeps a -0.0; x[lo] + d * t turns it into +0.0); np.quantile agrees as a value."""
    words = np.zeros((4, 4), dtype=np.uint32)
    words[3] = np.array([0.0, -0.0, -0.0, 0.0], dtype=np.float32).view(np.uint32)
    q = [0.0, 0.2, 0.5, 0.9]
    _, quant = series_window_quantiles(words, [0, 4], N_EDGES, q)
    assert np.signbit(quant[0, 3]).tolist() == [False, True, False, False] and (quant[0, 3] == 0).all()
    assert np.array_equal(quant[0, 3], np.quantile(words[3].view(np.float32).astype(np.float64), q))


def test_windows_and_column_selection():
    rng = np.random.default_rng(8)
    ticks = 103
    words = _case(rng, ticks, 70000, "dyadic")
    q = [0.5, 0.0, 1.0, 0.95]
    edges = [0, 40, 80, 120, 160, 500]     # a short third window, two windows wholly past the samples
    count, quant = series_window_quantiles(words, edges, N_EDGES, q)
    assert count.tolist() == [40, 40, 23, 0, 0] and quant.shape == (5, 4, 4)
    assert np.isnan(quant[3:]).all() and not np.isnan(quant[:3]).any()
    values = words.astype(np.float64)
    values[3] = words[3].view(np.float32).astype(np.float64)
    for w, (a, b) in enumerate(((0, 40), (40, 80), (80, 103))):
        assert quant[w].tobytes() == np.stack([np.quantile(values[j, a:b], q) for j in range(4)]).tobytes()
    # columns: any order, duplicates; output column c belongs to columns[c]
    cols = [3, 0, 3, 2]
    count_c, quant_c = series_window_quantiles(words, edges, N_EDGES, q, cols)
    assert np.array_equal(count_c, count) and quant_c.tobytes() == np.ascontiguousarray(quant[:, cols]).tobytes()
    # a cell does not depend on the other windows or levels of the call
    _, one = series_window_quantiles(words, [40, 80], N_EDGES, [0.95], [2])
    assert one[0, 0, 0].tobytes() == quant[1, 2, 3].tobytes()
    for bad in ([], [4], [-1], [0.5]):
        with pytest.raises(ValueError, match="series"):
            series_window_quantiles(words, edges, N_EDGES, q, bad)
    with pytest.raises(ValueError, match="strictly increasing"):
        series_window_quantiles(words, [0, 5, 5], N_EDGES, q)


def test_tick_edge_forms_of_a_scenario():
    plan = lower(lb_two_servers(horizon=10))
    rng = np.random.default_rng(3)
    ticks = plan.tick_count
    words = rng.integers(0, 50, (plan.n_series, ticks)).astype(np.uint32)
    res = ScenarioResults(plan, np.zeros(_abi.CNT_SLOTS, dtype=np.uint32), np.zeros((0, 2)), words)
    per = int(round(2.0 / plan.sample_period))
    a = res.get_series_window_quantiles([0.5, 0.99], 2.0)
    b = res.get_series_window_quantiles([0.5, 0.99], ticks_per_window=per)
    c = res.get_series_window_quantiles([0.5, 0.99], tick_edges=a["tick_edges"])
    assert a["quantiles"].shape == (-(-ticks // per), plan.n_series, 2) and int(a["count"].sum()) == ticks
    for other in (b, c):
        assert other["quantiles"].tobytes() == a["quantiles"].tobytes() and np.array_equal(other["count"], a["count"])
    sel = res.get_series_window_quantiles([0.5, 0.99], 2.0, series=[5, 1])
    assert sel["series"].tolist() == [5, 1] and sel["quantiles"].tobytes() == np.ascontiguousarray(a["quantiles"][:, [5, 1]]).tobytes()
    with pytest.raises(ValueError, match="one of"):
        res.get_series_window_quantiles([0.5], 2.0, ticks_per_window=per)
    none = ScenarioResults(plan, res.counts, np.zeros((0, 2)), None)
    with pytest.raises(RuntimeError, match="kept no sampled series"):
        none.get_series_window_quantiles([0.5])


def test_refusals_of_the_python_layer():
    assert check_series_levels(np.linspace(0, 1, 16)).shape == (16,)
    with pytest.raises(ValueError, match="at most 16"):
        check_series_levels(np.linspace(0, 1, 17))
    for bad in ([1.5], [-0.1], [float("nan")], [0.5, 2.0]):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            check_series_levels(bad)
    for bad in ([], 0.5, [[0.5]]):
        with pytest.raises(ValueError, match="vector"):
            check_series_levels(bad)
    plan = lower(lb_two_servers(horizon=10))
    batch = BatchedResults.__new__(BatchedResults)
    batch.plan = plan
    batch._samples_t = None  # noqa: SLF001
    for call in (batch.series_quantile_summary, batch.series_quantile_bands):
        with pytest.raises(RuntimeError, match="kept no sampled series"):
            call([0.5])
    with pytest.raises(RuntimeError, match="kept no sampled series"):
        batch.save_series_quantile_summary("nowhere.npz", levels=[0.5], ticks_per_window=10)
    batch._samples_t = object()  # noqa: SLF001  (the checks below come before the device is touched)
    names = batch.series_names()
    assert batch._series_columns(None).tolist() == list(range(len(names)))  # noqa: SLF001
    assert batch._series_columns([names[3], names[0], names[3]]).tolist() == [3, 0, 3]  # noqa: SLF001
    assert batch._series_columns(names[2]).tolist() == [2] and batch._series_columns([4, 1]).tolist() == [4, 1]  # noqa: SLF001
    with pytest.raises(ValueError, match="at most 16"):
        batch.series_quantile_summary(np.linspace(0, 1, 17))
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        batch.series_quantile_summary([0.5, 1.01])
    with pytest.raises(ValueError, match="unknown series"):
        batch.series_quantile_summary([0.5], series=["nobody:ram_in_use"])
    with pytest.raises(ValueError, match="series columns"):
        batch.series_quantile_summary([0.5], series=[len(names)])
    with pytest.raises(ValueError, match="one of"):
        batch.series_quantile_summary([0.5], 1.0, ticks_per_window=10)


def test_sharded_results_refuse_series_quantiles():
    sh = ShardedResults.__new__(ShardedResults)
    for call in (sh.series_quantile_summary, sh.series_quantile_bands, sh.save_series_quantile_summary):
        with pytest.raises(NotImplementedError, match="several devices"):
            call([0.5])
