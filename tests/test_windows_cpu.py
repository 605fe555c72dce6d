"""Windowed analyzer, CPU side: the C entry point and its struct, argument checks, and the host definition
(results.window_edges / latency_window_stats) that the device analyzer is bit-equal to."""

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
from asyncflow_amd.results import LATENCY_KEYS, ScenarioResults, check_edges, latency_window_stats, window_edges
from oracle.scenarios import lb_two_servers

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = sorted(p for p in (ROOT / "tests" / "golden").glob("*.npz") if "clock" in np.load(p).files)


@pytest.fixture(scope="module")
def lib():
    af_build.build()
    from asyncflow_amd.engine import load_library

    return load_library()


def test_header_declares_and_library_exports_the_windows_entry(lib):
    header = (ROOT / "include" / "asyncflow_hip.h").read_text()
    assert re.search(r"int\s+af_engine_summarize_windows\s*\(\s*af_engine_t\s*\*", header)
    assert "af_engine_summarize_windows" in _abi.EXPORTED_SYMBOLS
    assert hasattr(lib, "af_engine_summarize_windows")
    assert lib.af_engine_summarize_windows.argtypes[2] is C.POINTER(_abi.AfWindows)


def test_af_windows_layout_matches_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "a host C compiler is needed for the layout probe"
    fields = [name for name, _ in _abi.AfWindows._fields_]  # noqa: SLF001
    assert fields == ["n_scenarios", "n_groups", "n_windows", "group", "edges", "stats", "row_bounds", "elapsed_ms", "scratch_bytes"]
    src = tmp_path / "probe.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "asyncflow_hip.h"\n'
        'int main(void) { printf("%zu", sizeof(af_windows_t));\n'
        + "".join(f'printf(" %zu", offsetof(af_windows_t, {f}));\n' for f in fields)
        + 'printf(" %zu\\n", sizeof(af_pooled_t)); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run([cc, "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    P = _abi.AfWindows
    assert got == [C.sizeof(P), *(getattr(P, f).offset for f in fields), C.sizeof(_abi.AfPooled)]


def test_windows_entry_refuses_bad_requests_without_a_device(lib):
    from asyncflow_amd.engine import PLAN_ONLY, Engine, EngineUnavailableError

    eng = Engine(lower(lb_two_servers(horizon=20)), PLAN_ONLY)
    try:
        out = _abi.AfOutputs(4, None, 0, None, None)
        edges = (C.c_double * 3)(0.0, 1.0, 2.0)
        req = _abi.AfWindows(4, 1, 2, None, edges, None, None, 0.0, 0)
        assert lib.af_engine_summarize_windows(None, C.byref(out), C.byref(req)) == _abi.AF_ERR_INVALID
        assert lib.af_engine_summarize_windows(eng._h, None, C.byref(req)) == _abi.AF_ERR_INVALID  # noqa: SLF001
        assert lib.af_engine_summarize_windows(eng._h, C.byref(out), None) == _abi.AF_ERR_INVALID  # noqa: SLF001
        assert lib.af_engine_summarize_windows(eng._h, C.byref(out), C.byref(req)) == _abi.AF_ERR_NO_DEVICE  # noqa: SLF001
        assert b"planning-only" in lib.af_last_error()
        with pytest.raises(EngineUnavailableError, match="planning-only"):
            eng.summarize_windows(4, 1, [0.0, 1.0], clock_ptr=0, clock_capacity=4, counts_ptr=0, stats_ptr=0)
        with pytest.raises(ValueError, match="at least two"):
            eng.summarize_windows(4, 1, [0.0], clock_ptr=0, clock_capacity=4, counts_ptr=0, stats_ptr=0)
    finally:
        eng.close()


def _fixture(path: Path):
    z = np.load(path)
    plan = lower(json.loads(str(z["payload_json"])))
    clock = np.asarray(z["clock"], dtype=np.float64).reshape(-1, 2)
    counts = np.zeros(_abi.CNT_SLOTS, dtype=np.uint32)
    counts[_abi.CNT_COMPLETED] = clock.shape[0]
    return plan, clock, ScenarioResults(plan, counts, clock, None)


def test_window_edges_are_the_throughput_series_timestamps():
    plan, _, res = _fixture(ROOT / "tests" / "golden" / "lb2_events_t60.npz")
    for w in (1.0, 0.1, 7.5):
        e = window_edges(w, plan.total_time)
        ts, _ = res.get_throughput_series(w)
        assert e[0] == 0.0 and e[1:].tolist() == ts
    e = window_edges(0.1, 60)
    # the reference's accumulation, not k * w: 599 windows, the 600th edge would pass T
    assert e.shape == (600,) and e[-1] == 59.90000000000058 and e[-1] != 599 * 0.1
    assert window_edges(1.0, 60).tolist() == [float(k) for k in range(61)]
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="window_s"):
            window_edges(bad, 60)


def _by_masks(clock: np.ndarray, edges: np.ndarray) -> np.ndarray:
    """The definition stated independently: boolean masks on finish, the reference's numpy calls on what they keep."""
    start, finish = clock[:, 0], clock[:, 1]
    rows = []
    for lo, hi in zip(edges[:-1], edges[1:]):
        lat = (finish - start)[(finish > lo) & (finish <= hi)]
        if lat.size == 0:
            rows.append([0.0] + [np.nan] * 7)
        else:
            rows.append([float(lat.size), np.mean(lat), np.median(lat), np.std(lat), np.percentile(lat, 95),
                         np.percentile(lat, 99), np.min(lat), np.max(lat)])
    return np.asarray(rows, dtype=np.float64)


@pytest.mark.parametrize("path", GOLDEN, ids=[p.stem for p in GOLDEN])
def test_latency_window_stats_on_every_fixture(path):
    plan, clock, res = _fixture(path)
    finish = clock[:, 1]
    assert (np.diff(finish) >= 0.0).all(), "rqs_clock rows are in completion order: the assumption the windows rest on"
    T = plan.total_time
    hand = None
    if finish.size >= 8:   # edges that hit finish values exactly (such a row belongs to the window on the left), before and past the data
        f = np.unique(finish)
        hand = np.unique(np.concatenate([[-1.0, f[0], f[len(f) // 3], f[len(f) // 2], np.nextafter(f[len(f) // 2], np.inf), f[-1], T + 5.0, T + 9.0]]))
    for w, edges in ((1.0, window_edges(1.0, T)), (7.5, window_edges(7.5, T)), (None, hand)):
        if edges is None:
            continue
        got = latency_window_stats(clock, edges)
        want = _by_masks(clock, edges)
        assert got.shape == (len(edges) - 1, 8)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (path.stem, w)
        if w is not None:
            assert np.array_equal(res.get_latency_window_stats(w).view(np.uint64), got.view(np.uint64))
            assert (got[:, 0] / w).tolist() == res.get_throughput_series(w)[1]
    if hand is not None:   # the row whose finish IS an edge went left
        got = latency_window_stats(clock, hand)
        assert got[0, 0] == np.count_nonzero(finish <= hand[1]) and got[-1, 0] == 0 and got[:, 0].sum() == finish.size
    assert np.array_equal(res.get_latency_window_stats().view(np.uint64), latency_window_stats(clock, window_edges(1.0, T)).view(np.uint64))


def test_windows_show_the_spike_of_the_event_fixture():
    # lb2_events_t60: a network spike on client-lb from 10 s to 16 s; the whole-run median hardly moves, the windows' do
    _, clock, res = _fixture(ROOT / "tests" / "golden" / "lb2_events_t60.npz")
    st = res.get_latency_window_stats(2.0)
    med = st[:, LATENCY_KEYS.index("median")]
    before, during = med[0:5], med[5:8]          # windows (0, 2] .. (8, 10] and (10, 12] .. (14, 16]
    print("median per 2-s window before the spike:", before, "during:", during)
    assert during.min() > before.max()


def test_bad_edges_are_refused():
    clock = np.array([[0.0, 0.5], [0.2, 0.9]])
    for bad, what in (([0.0, 2.0, 1.0], "strictly increasing"), ([0.0, 1.0, 1.0], "strictly increasing"),
                      ([0.0, float("nan")], "finite"), ([0.0, float("inf")], "finite"), ([1.0], "at least two"), ([], "at least two"),
                      ([[0.0, 1.0]], "at least two")):
        with pytest.raises(ValueError, match=what):
            latency_window_stats(clock, bad)
        with pytest.raises(ValueError, match=what):
            check_edges(bad)
    with pytest.raises(ValueError, match="completion order"):
        latency_window_stats(np.array([[0.0, 0.9], [0.2, 0.5]]), [0.0, 1.0])
    _, _, res = _fixture(ROOT / "tests" / "golden" / "lb2_rr_t30.npz")
    with pytest.raises(ValueError, match="not both"):
        res.get_latency_window_stats(1.0, edges=[0.0, 1.0])


def test_sharded_results_refuse_windows():
    from asyncflow_amd.results import ShardedResults

    sh = ShardedResults.__new__(ShardedResults)
    for call in (sh.window_summary, sh.window_bands, sh.save_window_summary):
        with pytest.raises(NotImplementedError, match="several devices"):
            call(1.0)
