"""Quantile analyzer, CPU side: the C entry point and its struct, the argument checks that need no device, and the host
definitions (results.latency_quantiles / latency_window_quantiles) that the device analyzer is held to -- bit-equal to
np.quantile and np.count_nonzero(lat <= threshold)."""

from __future__ import annotations

import ctypes as C
import json
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
    check_levels,
    check_slo_thresholds,
    latency_quantiles,
    latency_window_quantiles,
    latency_window_stats,
    resolve_groups,
    window_edges,
)
from oracle.scenarios import lb_two_servers

ROOT = Path(__file__).resolve().parent.parent
LEVELS = [0.0, 1.0, 0.5, 0.95, 0.99, 0.999, 1.0 / 3.0]
SIZES = [1, 2, 3, 8, 9, 512, 513, 8192, 8193]


@pytest.fixture(scope="module")
def lib():
    af_build.build()
    from asyncflow_amd.engine import load_library

    return load_library()


def test_header_declares_and_library_exports_the_quantiles_entry(lib):
    header = (ROOT / "include" / "asyncflow_hip.h").read_text()
    assert re.search(r"int\s+af_engine_summarize_quantiles\s*\(\s*af_engine_t\s*\*", header)
    assert "af_engine_summarize_quantiles" in _abi.EXPORTED_SYMBOLS
    assert hasattr(lib, "af_engine_summarize_quantiles")
    assert lib.af_engine_summarize_quantiles.argtypes[2] is C.POINTER(_abi.AfQuantiles)
    declared = set(re.findall(r"^\s*(?:const\s+)?[A-Za-z_][\w\s\*]*?\b(af_[a-z_0-9]+)\s*\(", header, flags=re.MULTILINE))
    assert declared == set(_abi.EXPORTED_SYMBOLS)
    for name in _abi.EXPORTED_SYMBOLS:
        assert hasattr(lib, name), name
    assert re.search(r"#define\s+AF_ABI_VERSION\s+7\b", header) and lib.af_abi_version() == 7
    assert re.search(rf"#define\s+AF_MAX_QUANTILE_LEVELS\s+{_abi.MAX_QUANTILE_LEVELS}\b", header) and _abi.MAX_QUANTILE_LEVELS == 64
    assert re.search(rf"#define\s+AF_MAX_SLO_THRESHOLDS\s+{_abi.MAX_SLO_THRESHOLDS}\b", header) and _abi.MAX_SLO_THRESHOLDS == 64
    for name in ("latency_quantiles", "latency_window_quantiles"):
        assert name in asyncflow_amd.__all__ and hasattr(asyncflow_amd, name)


def test_af_quantiles_layout_matches_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "a host C compiler is needed for the layout probe"
    fields = [name for name, _ in _abi.AfQuantiles._fields_]  # noqa: SLF001
    assert fields == ["n_scenarios", "n_groups", "n_windows", "group", "edges", "n_levels", "levels", "n_thresholds", "thresholds",
                      "count", "quantiles", "within", "elapsed_ms", "scratch_bytes"]
    src = tmp_path / "probe.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "asyncflow_hip.h"\n'
        'int main(void) { printf("%zu", sizeof(af_quantiles_t));\n'
        + "".join(f'printf(" %zu", offsetof(af_quantiles_t, {f}));\n' for f in fields)
        + 'printf(" %zu\\n", sizeof(af_windows_t)); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run([cc, "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    P = _abi.AfQuantiles
    assert got == [C.sizeof(P), *(getattr(P, f).offset for f in fields), C.sizeof(_abi.AfWindows)]


def test_the_new_header_is_a_source_of_both_builds():
    from asyncflow_amd import jit

    for header in ("af_quantiles.hpp", "af_select.hpp"):
        assert header in af_build.SOURCES and header in jit._SOURCES  # noqa: SLF001
        assert (ROOT / "asyncflow_amd" / "csrc" / header).exists()


def test_quantiles_entry_refuses_bad_requests_without_a_device(lib):
    from asyncflow_amd.engine import PLAN_ONLY, Engine, EngineUnavailableError

    eng = Engine(lower(lb_two_servers(horizon=20)), PLAN_ONLY)
    try:
        out = _abi.AfOutputs(4, None, 0, None, None)
        edges = (C.c_double * 3)(0.0, 1.0, 2.0)
        lv = (C.c_double * 2)(0.5, 0.99)
        req = _abi.AfQuantiles(4, 1, 2, None, edges, 2, lv, 0, None, None, None, None, 0.0, 0)
        assert lib.af_engine_summarize_quantiles(None, C.byref(out), C.byref(req)) == _abi.AF_ERR_INVALID
        assert lib.af_engine_summarize_quantiles(eng._h, None, C.byref(req)) == _abi.AF_ERR_INVALID  # noqa: SLF001
        assert lib.af_engine_summarize_quantiles(eng._h, C.byref(out), None) == _abi.AF_ERR_INVALID  # noqa: SLF001
        assert lib.af_engine_summarize_quantiles(eng._h, C.byref(out), C.byref(req)) == _abi.AF_ERR_NO_DEVICE  # noqa: SLF001
        assert b"planning-only" in lib.af_last_error()
        kw = {"clock_ptr": 0, "clock_capacity": 4, "counts_ptr": 0}
        with pytest.raises(EngineUnavailableError, match="planning-only"):
            eng.summarize_quantiles(4, 1, [0.5], edges=[0.0, 1.0], **kw)
        with pytest.raises(EngineUnavailableError, match="planning-only"):
            eng.summarize_quantiles(4, 1, [0.5], thresholds=[0.2], **kw)
        with pytest.raises(ValueError, match="at least two"):
            eng.summarize_quantiles(4, 1, [0.5], edges=[0.0], **kw)
        with pytest.raises(ValueError, match="at least one"):
            eng.summarize_quantiles(4, 1, [], **kw)
        for bad in ([float("nan")], [-0.1], [1.0000001], [[0.5]]):
            with pytest.raises(ValueError, match="quantile levels"):
                eng.summarize_quantiles(4, 1, bad, **kw)
        with pytest.raises(ValueError, match="at most 64 quantile levels"):
            eng.summarize_quantiles(4, 1, np.linspace(0.0, 1.0, 65), **kw)
        with pytest.raises(ValueError, match="must not be NaN"):
            eng.summarize_quantiles(4, 1, [0.5], thresholds=[float("nan")], **kw)
        with pytest.raises(ValueError, match="at most 64 thresholds"):
            eng.summarize_quantiles(4, 1, [0.5], thresholds=np.arange(65.0), **kw)
    finally:
        eng.close()


def _samples(rng, n):
    return {
        "lognormal": rng.lognormal(-3.0, 0.8, n),
        "heavy ties": rng.integers(0, 5, n) / 7.0,
        "all equal": np.full(n, 0.1),
        "half equal": np.where(rng.random(n) < 0.5, 0.0625, rng.exponential(0.1, n)),
        "40 binades": np.ldexp(rng.uniform(1.0, 2.0, n), rng.integers(-30, 10, n)),
    }


@pytest.mark.parametrize("n", SIZES)
def test_host_definitions_are_numpy_bit_for_bit(n):
    rng = np.random.default_rng(1000 + n)
    for name, lat in _samples(rng, n).items():
        got = latency_quantiles(lat, LEVELS)
        want = np.quantile(lat, LEVELS)
        assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64)), (name, n, got, want)
        for q in LEVELS:      # scalar q takes numpy's other path
            assert latency_quantiles(lat, [q]).view(np.uint64)[0] == np.asarray(np.quantile(lat, q)).view(np.uint64), (name, n, q)
        # levels 0.95 / 0.99 / 0 / 1 are the p95 / p99 / min / max the other analyzers report
        assert np.array_equal(latency_quantiles(lat, [0.95, 0.99, 0.0, 1.0]).view(np.uint64),
                              np.array([np.percentile(lat, 95), np.percentile(lat, 99), np.min(lat), np.max(lat)]).view(np.uint64))
        thr = [float(lat[n // 2]), 0.05, float("inf"), float("-inf"), 0.0]       # the first exactly ON a latency
        ck = np.stack([np.zeros(n), lat], axis=1)
        assert np.array_equal(ck[:, 1] - ck[:, 0], lat)
        count, quant, within = latency_window_quantiles(ck, None, LEVELS, thr)
        assert count.tolist() == [n] and count.dtype == np.uint32 and within.dtype == np.uint32
        assert np.array_equal(quant[0].view(np.uint64), want.view(np.uint64))
        assert within[0].tolist() == [int(np.count_nonzero(lat <= t)) for t in thr]
        assert within[0, 0] >= 1 and within[0, 2] == n and within[0, 3] == 0


def test_the_half_level_is_not_always_the_median_column():
    # np.median is the mean of the middle pair; level 0.5 interpolates: the same number, not always the same bits
    rng = np.random.default_rng(2)
    differ = 0
    for _ in range(600):
        lat = rng.lognormal(-3.0, 0.8, 2 * int(rng.integers(1, 400)))
        q = latency_quantiles(lat, [0.5])[0]
        assert q.view(np.uint64) == np.asarray(np.quantile(lat, 0.5)).view(np.uint64)
        assert abs(q - np.median(lat)) <= np.spacing(q)
        differ += int(q != np.median(lat))
    print("level 0.5 differs from np.median in", differ, "of 600 even-sized samples")


def test_window_quantiles_follow_the_windows_of_the_stats():
    z = np.load(ROOT / "tests" / "golden" / "lb2_events_t60.npz")
    plan = lower(json.loads(str(z["payload_json"])))
    clock = np.asarray(z["clock"], dtype=np.float64).reshape(-1, 2)
    counts = np.zeros(_abi.CNT_SLOTS, dtype=np.uint32)
    counts[_abi.CNT_COMPLETED] = clock.shape[0]
    res = ScenarioResults(plan, counts, clock, None)
    finish, lat = clock[:, 1], clock[:, 1] - clock[:, 0]
    f = np.unique(finish)
    hand = np.unique(np.concatenate([[-1.0, f[0], f[len(f) // 3], f[len(f) // 2], np.nextafter(f[len(f) // 2], np.inf), f[-1], 65.0, 69.0]]))
    thr = [0.01, float(np.median(lat)), float("inf")]
    for edges in (window_edges(2.0, plan.total_time), window_edges(7.5, plan.total_time), hand):
        count, quant, within = latency_window_quantiles(clock, edges, LEVELS, thr)
        stats = latency_window_stats(clock, edges)
        assert count.shape == (len(edges) - 1,) and quant.shape == (len(edges) - 1, len(LEVELS)) and within.shape == (len(edges) - 1, 3)
        assert np.array_equal(count, stats[:, 0].astype(np.uint32))
        for w in range(len(edges) - 1):
            cell = lat[(finish > edges[w]) & (finish <= edges[w + 1])]
            assert count[w] == cell.size
            if cell.size == 0:
                assert np.isnan(quant[w]).all() and (within[w] == 0).all()
                continue
            assert np.array_equal(quant[w].view(np.uint64), np.quantile(cell, LEVELS).view(np.uint64))
            assert within[w].tolist() == [int(np.count_nonzero(cell <= t)) for t in thr]
            assert np.array_equal(quant[w, [3, 4, 0, 1]].view(np.uint64), stats[w, [4, 5, 6, 7]].view(np.uint64))
    got = res.get_latency_quantiles(LEVELS, window_s=2.0, thresholds=thr)
    count, quant, within = latency_window_quantiles(clock, window_edges(2.0, plan.total_time), LEVELS, thr)
    assert np.array_equal(got["count"], count) and np.array_equal(got["within"], within)
    assert np.array_equal(got["quantiles"].view(np.uint64), quant.view(np.uint64))
    assert np.array_equal(got["share"], within / count[:, None].astype(np.float64)) and np.array_equal(got["edges"], window_edges(2.0, plan.total_time))
    whole = res.get_latency_quantiles(LEVELS, thresholds=thr)
    assert whole["count"] == lat.size and whole["edges"] is None and whole["within"].tolist() == [int(np.count_nonzero(lat <= t)) for t in thr]
    assert np.array_equal(whole["quantiles"].view(np.uint64), np.quantile(lat, LEVELS).view(np.uint64))
    with pytest.raises(ValueError, match="not both"):
        res.get_latency_quantiles([0.5], window_s=1.0, edges=[0.0, 1.0])
    # the whole run takes the rows in any order, windows do not
    shuffled = clock[np.random.default_rng(3).permutation(clock.shape[0])]
    _, q2, w2 = latency_window_quantiles(shuffled, None, LEVELS, thr)
    assert np.array_equal(q2[0].view(np.uint64), whole["quantiles"].view(np.uint64)) and np.array_equal(w2[0], whole["within"])
    with pytest.raises(ValueError, match="completion order"):
        latency_window_quantiles(shuffled, [0.0, 60.0], LEVELS)


def test_bad_levels_thresholds_and_edges_are_refused():
    clock = np.array([[0.0, 0.5], [0.2, 0.9]])
    for bad in ([float("nan")], [-1e-9], [1.0 + 1e-9], [[0.5]], 0.5):
        with pytest.raises(ValueError, match="quantile levels"):
            check_levels(bad)
        with pytest.raises(ValueError, match="quantile levels"):
            latency_quantiles([0.1, 0.2], bad)
    with pytest.raises(ValueError, match="at most 64"):
        check_levels(np.linspace(0.0, 1.0, 65))
    assert check_levels(np.linspace(0.0, 1.0, 64)).shape == (64,) and check_levels([]).shape == (0,)
    assert check_slo_thresholds(None).shape == (0,) and check_slo_thresholds([float("inf"), float("-inf"), 0.2]).shape == (3,)
    for bad, what in (([float("nan")], "NaN"), ([[0.1]], "vector"), (np.arange(65.0), "at most 64")):
        with pytest.raises(ValueError, match=what):
            check_slo_thresholds(bad)
    for bad, what in (([0.0, 2.0, 1.0], "strictly increasing"), ([0.0, float("inf")], "finite"), ([1.0], "at least two")):
        with pytest.raises(ValueError, match=what):
            latency_window_quantiles(clock, bad, [0.5])
    count, quant, within = latency_window_quantiles(np.zeros((0, 2)), [0.0, 1.0, 2.0], [0.5, 0.9], [0.1])
    assert count.tolist() == [0, 0] and np.isnan(quant).all() and quant.shape == (2, 2) and within.tolist() == [[0], [0]]
    assert np.isnan(latency_quantiles([], [0.5, 1.0])).all()


def test_group_resolution_and_the_sharded_refusals():
    from asyncflow_amd.results import BatchedResults, ShardedResults

    ids, g = resolve_groups(np.array([2, 0, -1, 2]), 4)
    assert g == 3 and ids.tolist() == [2, 0, -1, 2]
    ids, g = resolve_groups(None, 5)
    assert g == 1 and ids.tolist() == [0] * 5
    br = BatchedResults.__new__(BatchedResults)
    br.counts = np.zeros((3, _abi.CNT_SLOTS), dtype=np.uint32)
    ids, g = BatchedResults._window_groups(br, "scenario")  # noqa: SLF001
    assert g == len(br) == 3 and ids.tolist() == [0, 1, 2]
    with pytest.raises(ValueError, match="by must be"):
        BatchedResults._window_groups(br, "point")  # noqa: SLF001
    sh = ShardedResults.__new__(ShardedResults)
    for call in (sh.quantile_summary, sh.quantile_bands, sh.save_quantile_summary):
        with pytest.raises(NotImplementedError, match="several devices"):
            call([0.5])
