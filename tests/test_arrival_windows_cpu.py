"""Latency windows by ARRIVAL time, CPU side: the host definition (results.latency_window_stats /
latency_window_quantiles with window_of="arrival") against boolean masks written out here, on every golden fixture; the edge
rule, the dropped rows, the refusals; the two C entry points and the unchanged ABI."""

from __future__ import annotations

import ctypes as C
import json
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from asyncflow_amd import _abi
from asyncflow_amd import build as af_build
from asyncflow_amd.plan import lower
from asyncflow_amd.results import (
    ScenarioResults,
    latency_quantiles,
    latency_stats_row,
    latency_window_quantiles,
    latency_window_stats,
    latency_within,
    window_edges,
)

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = sorted(p for p in (ROOT / "tests" / "golden").glob("*.npz") if "clock" in np.load(p).files)
LEVELS = [0.0, 0.5, 0.95, 0.999, 1.0]
THRESHOLDS = [0.01, 0.2, 5.0]


@pytest.fixture(scope="module")
def lib():
    af_build.build()
    from asyncflow_amd.engine import load_library

    return load_library()


def _fixture(path: Path):
    z = np.load(path)
    plan = lower(json.loads(str(z["payload_json"])))
    clock = np.asarray(z["clock"], dtype=np.float64).reshape(-1, 2)
    counts = np.zeros(_abi.CNT_SLOTS, dtype=np.uint32)
    counts[_abi.CNT_COMPLETED] = clock.shape[0]
    return plan, clock, ScenarioResults(plan, counts, clock, None)


def _masked(clock: np.ndarray, edges: np.ndarray) -> list[np.ndarray]:
    """The definition stated independently: per window a boolean mask on START, the latencies it keeps in row order."""
    start, finish = clock[:, 0], clock[:, 1]
    return [(finish - start)[(start > lo) & (start <= hi)] for lo, hi in zip(edges[:-1], edges[1:])]


def _same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("path", GOLDEN, ids=[p.stem for p in GOLDEN])
def test_arrival_windows_on_every_fixture(path):
    plan, clock, res = _fixture(path)
    start = clock[:, 0]
    T = plan.total_time
    cases = [window_edges(1.0, T)]
    if start.size >= 8:   # uneven edges that start after the first arrival and end before the last, two of them ON a start
        s = np.sort(start)
        cases.append(np.unique([s[2], s[len(s) // 5], 0.5 * (s[len(s) // 3] + s[len(s) // 2]), s[len(s) // 2], s[(3 * len(s)) // 4], s[-3]]))
        assert cases[1][0] > s[0] and cases[1][-1] < s[-1]
    for edges in cases:
        cells = _masked(clock, edges)
        got = latency_window_stats(clock, edges, window_of="arrival")
        want = np.stack([latency_stats_row(x) for x in cells])
        assert _same_bits(got, want), path.stem
        cnt, quant, within = latency_window_quantiles(clock, edges, LEVELS, THRESHOLDS, window_of="arrival")
        assert cnt.dtype == np.uint32 and cnt.tolist() == [x.size for x in cells]
        assert _same_bits(quant, np.stack([latency_quantiles(x, LEVELS) for x in cells]))
        assert _same_bits(within, np.stack([latency_within(x, THRESHOLDS) for x in cells]))
        # the totals over a partition of (e[0], e[W]] sum to the rows that start in it
        assert got[:, 0].sum() == np.count_nonzero((start > edges[0]) & (start <= edges[-1]))
    # the accessors of one scenario's results pass the keyword on
    assert _same_bits(res.get_latency_window_stats(1.0, window_of="arrival"), latency_window_stats(clock, cases[0], window_of="arrival"))
    acc = res.get_latency_quantiles(LEVELS, window_s=1.0, thresholds=THRESHOLDS, window_of="arrival")
    assert acc["window_of"] == "arrival" and _same_bits(acc["quantiles"], latency_window_quantiles(clock, cases[0], LEVELS, THRESHOLDS, "arrival")[1])
    # a partition of the starts' whole range holds every row
    if start.size:
        part = np.linspace(start.min() - 1.0, start.max(), 7)
        assert latency_window_stats(clock, part, window_of="arrival")[:, 0].sum() == start.size


def test_arrival_and_finish_windows_differ_on_the_overload_fixture():
    plan, clock, _ = _fixture(ROOT / "tests" / "golden" / "overload_t30.npz")
    edges = window_edges(1.0, plan.total_time)
    by_arrival = latency_window_stats(clock, edges, window_of="arrival")
    by_finish = latency_window_stats(clock, edges)
    assert (by_arrival[:, 0] != by_finish[:, 0]).any()
    moved = np.searchsorted(edges, clock[:, 0], side="left") != np.searchsorted(edges, clock[:, 1], side="left")
    print("overload_t30: rows whose start and finish lie in different 1-s windows:", int(moved.sum()), "of", clock.shape[0])
    assert moved.sum() > clock.shape[0] // 2


def test_one_window_around_every_start_is_the_whole_sample():
    _, clock, _ = _fixture(ROOT / "tests" / "golden" / "stress_mixed_t40.npz")
    start = clock[:, 0]
    lat = clock[:, 1] - start
    assert (np.diff(start) < 0).any(), "start is not sorted in rqs_clock: the case the arrival windows are for"
    for hi in (start.max(), start.max() + 1.0):
        got = latency_window_stats(clock, [start.min() - 1.0, hi], window_of="arrival")
        assert _same_bits(got[0], latency_stats_row(lat))
    cnt, quant, within = latency_window_quantiles(clock, [start.min() - 1.0, start.max()], LEVELS, THRESHOLDS, window_of="arrival")
    assert cnt.tolist() == [lat.size] and _same_bits(quant[0], latency_quantiles(lat, LEVELS)) and _same_bits(within[0], latency_within(lat, THRESHOLDS))


def test_a_start_on_an_edge_goes_left_and_rows_outside_are_dropped():
    # rows in completion order; starts out of order, three of them exactly on edges
    clock = np.array([[1.0, 1.5], [0.5, 1.75], [2.0, 2.25], [1.0, 2.5], [3.0, 3.125], [0.25, 3.5], [2.5, 3.75], [3.5, 4.0], [2.0, 9.0]])
    edges = [0.5, 1.0, 2.0, 3.0]
    got = latency_window_stats(clock, edges, window_of="arrival")
    assert got[:, 0].tolist() == [2.0, 2.0, 2.0]            # 0.5 (on e[0]) and 0.25 are before, 3.5 is past the windows
    assert _same_bits(got[0], latency_stats_row(np.array([0.5, 1.5])))        # starts 1.0, 1.0: ON e[1], in row order
    assert _same_bits(got[1], latency_stats_row(np.array([0.25, 7.0])))       # starts 2.0, 2.0: ON e[2]
    assert _same_bits(got[2], latency_stats_row(np.array([0.125, 1.25])))     # starts 3.0 (ON e[3]) and 2.5
    cnt, _, within = latency_window_quantiles(clock, edges, [0.5], [0.5], window_of="arrival")
    assert cnt.tolist() == [2, 2, 2] and within[:, 0].tolist() == [1, 1, 1]
    # no completion-order check by arrival; by finish it stays
    swapped = clock[[1, 0] + list(range(2, 9))]
    latency_window_stats(swapped, edges, window_of="arrival")
    with pytest.raises(ValueError, match="completion order"):
        latency_window_stats(swapped, edges)


def test_window_of_finish_is_the_call_without_the_keyword():
    for path in GOLDEN:
        plan, clock, res = _fixture(path)
        edges = window_edges(2.5, plan.total_time)
        assert _same_bits(latency_window_stats(clock, edges, window_of="finish"), latency_window_stats(clock, edges))
        for e in (edges, None):
            a = latency_window_quantiles(clock, e, LEVELS, THRESHOLDS, window_of="finish")
            b = latency_window_quantiles(clock, e, LEVELS, THRESHOLDS)
            assert all(_same_bits(x, y) for x, y in zip(a, b))
        assert _same_bits(res.get_latency_window_stats(2.5, window_of="finish"), res.get_latency_window_stats(2.5))


def test_refusals():
    clock = np.array([[0.0, 0.5], [0.2, 0.9]])
    for bad in ("start", "Arrival", "", None):
        with pytest.raises(ValueError, match="window_of"):
            latency_window_stats(clock, [0.0, 1.0], window_of=bad)
        with pytest.raises(ValueError, match="window_of"):
            latency_window_quantiles(clock, [0.0, 1.0], [0.5], window_of=bad)
        with pytest.raises(ValueError, match="window_of"):
            latency_window_quantiles(clock, None, [0.5], window_of=bad)
    with pytest.raises(ValueError, match="no window"):
        latency_window_quantiles(clock, None, [0.5], window_of="arrival")
    _, _, res = _fixture(ROOT / "tests" / "golden" / "lb2_rr_t30.npz")
    with pytest.raises(ValueError, match="no window"):
        res.get_latency_quantiles([0.5], window_of="arrival")
    with pytest.raises(ValueError, match="window_of"):
        res.get_latency_window_stats(1.0, window_of="sent")


def test_header_declares_and_library_exports_the_arrival_entries(lib):
    header = (ROOT / "include" / "asyncflow_hip.h").read_text()
    for name, req in (("af_engine_summarize_arrival_windows", _abi.AfWindows), ("af_engine_summarize_arrival_quantiles", _abi.AfQuantiles)):
        assert re.search(rf"int\s+{name}\s*\(\s*af_engine_t\s*\*", header)
        assert name in _abi.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
        assert getattr(lib, name).argtypes[2] is C.POINTER(req)
    assert re.search(r"#define\s+AF_ABI_VERSION\s+7\b", header) and lib.af_abi_version() == 7
    assert "af_arrival.hpp" in af_build.SOURCES and (ROOT / "asyncflow_amd" / "csrc" / "af_arrival.hpp").exists()


def test_request_structs_are_the_headers(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "a host C compiler is needed for the layout probe"
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "asyncflow_hip.h"\n'
                   'int main(void) { printf("%zu %zu\\n", sizeof(af_windows_t), sizeof(af_quantiles_t)); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run([cc, "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(_abi.AfWindows), C.sizeof(_abi.AfQuantiles)]


def test_arrival_entries_refuse_bad_requests_without_a_device(lib):
    from asyncflow_amd.engine import PLAN_ONLY, Engine, EngineUnavailableError
    from oracle.scenarios import lb_two_servers

    eng = Engine(lower(lb_two_servers(horizon=20)), PLAN_ONLY)
    try:
        out = _abi.AfOutputs(4, None, 0, None, None)
        edges = (C.c_double * 3)(0.0, 1.0, 2.0)
        req = _abi.AfWindows(4, 1, 2, None, edges, None, None, 0.0, 0)
        assert lib.af_engine_summarize_arrival_windows(None, C.byref(out), C.byref(req)) == _abi.AF_ERR_INVALID
        assert lib.af_engine_summarize_arrival_windows(eng._h, C.byref(out), C.byref(req)) == _abi.AF_ERR_NO_DEVICE  # noqa: SLF001
        lv = (C.c_double * 1)(0.5)
        qreq = _abi.AfQuantiles(4, 1, 2, None, edges, 1, lv, 0, None, None, None, None, 0.0, 0)
        assert lib.af_engine_summarize_arrival_quantiles(None, C.byref(out), C.byref(qreq)) == _abi.AF_ERR_INVALID
        assert lib.af_engine_summarize_arrival_quantiles(eng._h, C.byref(out), C.byref(qreq)) == _abi.AF_ERR_NO_DEVICE  # noqa: SLF001
        with pytest.raises(EngineUnavailableError, match="planning-only"):
            eng.summarize_windows(4, 1, [0.0, 1.0], clock_ptr=0, clock_capacity=4, counts_ptr=0, stats_ptr=0, window_of="arrival")
        with pytest.raises(ValueError, match="window_of"):
            eng.summarize_windows(4, 1, [0.0, 1.0], clock_ptr=0, clock_capacity=4, counts_ptr=0, stats_ptr=0, window_of="sent")
        with pytest.raises(ValueError, match="needs windows"):
            eng.summarize_quantiles(4, 1, [0.5], clock_ptr=0, clock_capacity=4, counts_ptr=0, window_of="arrival")
        with pytest.raises(ValueError, match="window_of"):
            eng.summarize_quantiles(4, 1, [0.5], clock_ptr=0, clock_capacity=4, counts_ptr=0, window_of="sent")
    finally:
        eng.close()
