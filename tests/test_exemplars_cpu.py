"""The k slowest requests per window and group, CPU side: the C entry point and its struct, and the host definition
(`results.latency_exemplars`) that `af_engine_summarize_exemplars` is held to word for word -- against a brute-force Python
`sorted` with the stated comparator on every committed golden clock, the identities with the window statistics, and synthetic
ties, signed zeros, infinities, NaN rows and times on and outside the edges."""

from __future__ import annotations

import bisect
import ctypes as C
import functools
import json
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
from asyncflow_amd.results import ScenarioResults, ShardedResults, latency_exemplars, latency_window_stats
from oracle.scenarios import lb_two_servers

ROOT = Path(__file__).resolve().parent.parent
FIXTURES = sorted(p.stem for p in (ROOT / "tests" / "golden").glob("*.npz") if "clock" in np.load(p).files)
ONES64 = np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(scope="module")
def lib():
    af_build.build()
    from asyncflow_amd.engine import load_library

    return load_library()


def test_header_declares_and_library_exports_the_entry(lib):
    header = (ROOT / "include" / "asyncflow_hip.h").read_text()
    assert re.search(r"int\s+af_engine_summarize_exemplars\s*\(\s*af_engine_t\s*\*", header)
    assert re.search(r"#define\s+AF_MAX_EXEMPLARS\s+64\b", header)
    assert "af_engine_summarize_exemplars" in _abi.EXPORTED_SYMBOLS
    assert lib.af_engine_summarize_exemplars.argtypes[2] is C.POINTER(_abi.AfExemplars)
    assert lib.af_abi_version() == 7
    for src in ("build.py", "jit.py"):
        assert '"af_exemplars.hpp"' in (ROOT / "asyncflow_amd" / src).read_text()
    assert "latency_exemplars" in asyncflow_amd.__all__ and asyncflow_amd.latency_exemplars is latency_exemplars


def test_af_exemplars_layout_matches_the_header_and_the_other_structs_keep_their_sizes(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "a host C compiler is needed for the layout probe"
    fields = [name for name, _ in _abi.AfExemplars._fields_]  # noqa: SLF001
    assert fields == ["n_scenarios", "n_groups", "n_windows", "group", "edges", "by_arrival", "k", "sample_period", "total", "kept",
                      "scenario", "row", "clock", "state", "elapsed_ms", "scratch_bytes"]
    others = {"af_arrivals_t": (_abi.AfArrivals, 96), "af_inflight_t": (_abi.AfInflight, 152), "af_outputs_t": (_abi.AfOutputs, 80),
              "af_pooled_t": (_abi.AfPooled, 32), "af_quantiles_t": (_abi.AfQuantiles, 104), "af_windows_t": (_abi.AfWindows, 64),
              "af_state_bins_t": (_abi.AfStateBins, 32), "af_series_windows_t": (_abi.AfSeriesWindows, 96),
              "af_series_quantiles_t": (_abi.AfSeriesQuantiles, 96), "af_series_excursions_t": (_abi.AfSeriesExcursions, 104),
              "af_series_histogram_t": (_abi.AfSeriesHistogram, 120), "af_series_combined_t": (_abi.AfSeriesCombined, 176),
              "af_series_joint_t": (_abi.AfSeriesJoint, 128), "af_series_warmup_t": (_abi.AfSeriesWarmup, 120),
              "af_summary_t": (_abi.AfSummary, 64), "af_sweep_t": (_abi.AfSweep, 40), "af_stats_t": (_abi.AfStats, 168)}
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "asyncflow_hip.h"\n'
                   'int main(void) { printf("%zu", sizeof(af_exemplars_t));\n'
                   + "".join(f'printf(" %zu", offsetof(af_exemplars_t, {f}));\n' for f in fields)
                   + "".join(f'printf(" %zu", sizeof({t}));\n' for t in others) + 'printf("\\n"); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run([cc, "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    P = _abi.AfExemplars
    assert C.sizeof(P) == 112
    assert got == [C.sizeof(P), *(getattr(P, f).offset for f in fields), *(size for _, size in others.values())]
    assert [C.sizeof(cls) for cls, _ in others.values()] == [size for _, size in others.values()]


def test_entry_refuses_without_a_device(lib):
    from asyncflow_amd.engine import PLAN_ONLY, Engine, EngineUnavailableError

    eng = Engine(lower(lb_two_servers(horizon=20)), PLAN_ONLY)
    try:
        out = _abi.AfOutputs(4, None, 8, None, None)
        req = _abi.AfExemplars(4, 1, 0, None, None, 0, 4)
        assert lib.af_engine_summarize_exemplars(None, C.byref(out), C.byref(req)) == _abi.AF_ERR_INVALID
        assert lib.af_engine_summarize_exemplars(eng._h, None, C.byref(req)) == _abi.AF_ERR_INVALID  # noqa: SLF001
        assert lib.af_engine_summarize_exemplars(eng._h, C.byref(out), None) == _abi.AF_ERR_INVALID  # noqa: SLF001
        assert lib.af_engine_summarize_exemplars(eng._h, C.byref(out), C.byref(req)) == _abi.AF_ERR_NO_DEVICE  # noqa: SLF001
        assert b"planning-only" in lib.af_last_error()
        kw = dict(clock_ptr=0, clock_capacity=4, counts_ptr=0, total_ptr=0, scenario_ptr=0, row_ptr=0, pair_ptr=0)
        with pytest.raises(EngineUnavailableError, match="planning-only"):
            eng.summarize_exemplars(4, 1, 4, **kw)
        for bad in (0, 65, 1.5, True):
            with pytest.raises(ValueError, match="k must be"):
                eng.summarize_exemplars(4, 1, bad, **kw)
        with pytest.raises(ValueError, match="arrival"):
            eng.summarize_exemplars(4, 1, 4, window_of="arrival", **kw)
        with pytest.raises(ValueError, match="window_of"):
            eng.summarize_exemplars(4, 1, 4, edges=[0.0, 1.0], window_of="start", **kw)
        with pytest.raises(ValueError, match="strictly increasing"):
            eng.summarize_exemplars(4, 1, 4, edges=[0.0, 1.0, 1.0], **kw)
    finally:
        eng.close()


# ---- the definition against a brute-force sort ------------------------------------------------------------------------
def _brute(members: list[np.ndarray], ids: list[int], k: int, edges, window_of: str):
    """Python floats, `sorted` with the comparator as stated: larger latency first as VALUES, then scenario, then row."""
    n_win = 1 if edges is None else len(edges) - 1
    cells: list[list[tuple[float, int, int, float, float]]] = [[] for _ in range(n_win)]
    for rows, s in zip(members, ids):
        for i, (start, finish) in enumerate(np.asarray(rows, dtype=np.float64).reshape(-1, 2).tolist()):
            lat = finish - start
            if math.isnan(lat):
                continue
            w = 0
            if edges is not None:
                t = finish if window_of == "finish" else start
                w = bisect.bisect_left(edges, t) - 1                      # edges[w] < t <= edges[w + 1]
                if math.isnan(t) or not (0 <= w < n_win and edges[w] < t <= edges[w + 1]):
                    continue
            cells[w].append((lat, s, i, start, finish))

    def cmp(a, b):
        if a[0] != b[0]:
            return -1 if a[0] > b[0] else 1      # (-0.0 == +0.0 here)
        return -1 if a[1:3] < b[1:3] else 1 if a[1:3] > b[1:3] else 0

    return [(len(c), sorted(c, key=functools.cmp_to_key(cmp))[:k]) for c in cells]


def _check(members, k, edges, window_of, ids=None):
    ids = list(range(len(members))) if ids is None else ids
    got = latency_exemplars(members, k, edges, window_of, scenario_ids=ids)
    want = _brute(members, ids, k, None if edges is None else list(edges), window_of)
    assert got["total"].dtype == np.uint64 and got["kept"].dtype == np.uint32 and got["scenario"].dtype == np.uint32
    assert got["row"].shape == (len(want), k) and got["clock"].shape == (len(want), k, 2)
    for w, (total, top) in enumerate(want):
        assert int(got["total"][w]) == total and int(got["kept"][w]) == len(top) == min(k, total)
        assert got["scenario"][w, :len(top)].tolist() == [t[1] for t in top], (w, window_of)
        assert got["row"][w, :len(top)].tolist() == [t[2] for t in top], (w, window_of)
        pairs = np.array([[t[3], t[4]] for t in top], dtype=np.float64).reshape(-1, 2)
        assert np.array_equal(got["clock"][w, :len(top)].view(np.uint64), pairs.view(np.uint64))
        assert (got["scenario"][w, len(top):] == 0xFFFFFFFF).all() and (got["row"][w, len(top):] == 0xFFFFFFFF).all()
        assert (got["clock"][w, len(top):].view(np.uint64) == ONES64).all()
    return got


def _fixture(name: str):
    z = np.load(ROOT / "tests" / "golden" / f"{name}.npz")
    plan = lower(json.loads(str(z["payload_json"])))
    clock = np.asarray(z["clock"], dtype=np.float64).reshape(-1, 2)
    return plan, clock, z


def test_there_are_twelve_single_run_fixtures():
    assert len(FIXTURES) == 12 and "overload_t30" in FIXTURES and "stress_mixed_t40" in FIXTURES


@pytest.mark.parametrize("name", FIXTURES)
def test_golden_clocks_against_the_brute_force_sort_and_the_window_statistics(name):
    plan, clock, z = _fixture(name)
    T = float(plan.total_time)
    one_s = np.arange(0.0, math.floor(T) + 1.0)
    uneven = np.array([0.25, 1.0, 1.5, 0.4 * T, 0.41 * T, 0.9 * T])
    for window_of in ("finish", "arrival"):
        for edges in (one_s, uneven):
            for k in (1, 5, 64):
                got = _check([clock], k, edges, window_of)
            stats = latency_window_stats(clock, edges, window_of)          # the window statistics of the same cells
            assert np.array_equal(got["total"].astype(np.float64), stats[:, 0])
            top = latency_exemplars([clock], 1, edges, window_of)
            some = top["kept"] == 1
            lat = top["clock"][:, 0, 1] - top["clock"][:, 0, 0]
            assert np.array_equal(lat[some].view(np.uint64), stats[some, 7].view(np.uint64))   # k = 1 is the window's max
            assert np.array_equal(some, stats[:, 0] > 0)
    for k in (1, 16):
        whole = _check([clock], k, None, "finish")
    assert int(whole["total"][0]) == clock.shape[0]
    top = latency_exemplars(clock, 1)                                       # (one array is one member)
    assert float(top["clock"][0, 0, 1] - top["clock"][0, 0, 0]) == float(z["latency_stats"][7])
    if name in ("overload_t30", "stress_mixed_t40"):                        # latency grows along the run: the slowest rows are the last
        assert int(top["row"][0, 0]) > 0.9 * clock.shape[0]


def test_synthetic_ties_zeros_infinities_nan_rows_and_times_on_the_edges():
    nan, inf = float("nan"), float("inf")
    a = np.array([[1.0, 3.0], [2.0, 4.0], [1.0, 1.0], [5.0, 5.0 - 0.0], [0.5, inf], [nan, 2.0], [2.0, nan], [3.0, 2.0], [-inf, 1.0],
                  [4.0, 4.0], [inf, inf], [1.0, 2.0]])
    a[3] = [5.0, 5.0]
    b = np.array([[0.0, 2.0], [0.0, -0.0], [-0.0, 0.0], [2.0, 4.0], [1.5, 3.5], [1e-310, 3e-310], [0.0, 5e-324]])
    c = np.zeros((0, 2))
    d = np.array([[7.0, 9.0]] * 5)
    members, ids = [a, b, c, d], [2, 3, 7, 11]
    assert np.signbit((b[1, 1] - b[1, 0])) != np.signbit(b[2, 1] - b[2, 0])          # a -0.0 and a +0.0 latency
    for k in (1, 2, 3, 7, 8, 64):
        got = _check(members, k, None, "finish", ids)
    assert int(got["total"][0]) == len(a) + len(b) + len(d) - 3                      # NaN - x, x - NaN and inf - inf are in no cell
    assert got["scenario"][0, :2].tolist() == [2, 2] and got["row"][0, :2].tolist() == [4, 8]   # both +inf: the lower row first
    edges = [0.0, 1.0, 2.0, 4.0, 5.0]                                                # starts and finishes ON edges, before e[0], past e[W]
    for window_of in ("finish", "arrival"):
        for k in (1, 2, 6, 64):
            got = _check(members, k, edges, window_of, ids)
        assert int(got["total"].sum()) < len(a) + len(b) + len(d) - 3                # rows outside (e[0], e[W]] are in no cell
    ties = [np.array([[float(i % 3), float(i % 3) + 1.0] for i in range(40)]), np.array([[0.0, 1.0]] * 30), np.array([[1.0, 2.0]] * 3)]
    for k in (1, 39, 40, 41, 64):                                                    # a run of equal latencies across the member seam
        _check(ties, k, None, "finish")
        _check(ties, k, [0.5, 1.0, 2.5, 3.0], "finish")
        _check(ties, k, [-1.0, 0.0, 1.0, 2.0], "arrival")
    empty = latency_exemplars([np.zeros((0, 2))], 3, [0.0, 1.0, 2.0])
    assert empty["total"].tolist() == [0, 0] and empty["kept"].tolist() == [0, 0]
    assert latency_exemplars([], 2)["total"].tolist() == [0]


def test_state_met_on_arrival_follows_the_tick_rule():
    p, ticks = 0.25, 8
    words = np.arange(3 * ticks, dtype=np.uint32).reshape(3, ticks) + 100
    words[2] = np.linspace(0.5, 4.0, ticks).astype(np.float32).view(np.uint32)        # a ram_in_use column stays f32 bits
    starts = np.array([0.0, 0.2, 0.25, 0.26, 1.0, ticks * p, (ticks + 1) * p - 1e-9, (ticks + 1) * p, -0.5, np.nan, -0.0, 1e300])
    clock = np.stack([starts, starts + np.arange(len(starts), 0, -1)], axis=1)        # descending latency: slot j is row j
    got = latency_exemplars([clock], 64, samples=[words], sample_period=p)
    assert got["state"].shape == (1, 64, 3) and int(got["kept"][0]) == len(starts) - 1   # (the NaN start is in no cell)
    rows = got["row"][0, :11].tolist()
    for j, i in enumerate(rows):
        s = starts[i]
        q = math.floor(s / p) if s >= 0 else 0
        want = words[:, q - 1] if 1 <= q <= ticks else np.full(3, 0xFFFFFFFF, dtype=np.uint32)
        assert np.array_equal(got["state"][0, j], want), (i, s)
    assert (got["state"][0, 11:] == 0xFFFFFFFF).all()
    with pytest.raises(ValueError, match="sample_period"):
        latency_exemplars([clock], 4, samples=[words])
    with pytest.raises(ValueError, match="samples"):
        latency_exemplars([clock, clock], 4, samples=[words], sample_period=p)


def test_refusals_of_the_host_definition_and_the_python_surface():
    ck = np.array([[0.0, 1.0]])
    for bad in (0, 65, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="k must be"):
            latency_exemplars([ck], bad)
    with pytest.raises(ValueError, match="arrival"):
        latency_exemplars([ck], 1, None, "arrival")
    with pytest.raises(ValueError, match="window_of"):
        latency_exemplars([ck], 1, [0.0, 1.0], "start")
    for edges in ([0.0], [0.0, 0.0], [1.0, 0.0], [0.0, np.inf], [0.0, np.nan]):
        with pytest.raises(ValueError, match="edges"):
            latency_exemplars([ck], 1, edges)
    with pytest.raises(ValueError, match="scenario_ids"):
        latency_exemplars([ck, ck], 1, scenario_ids=[3, 3])
    sharded = ShardedResults.__new__(ShardedResults)
    for call in (sharded.exemplar_summary, sharded.save_exemplar_summary):
        with pytest.raises(NotImplementedError, match="several devices"):
            call()


def test_a_scenario_lists_its_own_slowest_requests():
    plan, clock, _ = _fixture("lb2_events_t60")
    counts = np.zeros(_abi.CNT_SLOTS, dtype=np.uint32)
    counts[_abi.CNT_COMPLETED] = clock.shape[0]
    res = ScenarioResults(plan, counts, clock, None)
    got = res.get_slowest_requests(3)
    lat = clock[:, 1] - clock[:, 0]
    assert got["row"].shape == (1, 3) and got["edges"] is None and "scenario" not in got
    assert got["row"][0].tolist() == np.lexsort((np.arange(len(lat)), -lat))[:3].tolist()
    assert np.array_equal(got["latency"][0], lat[got["row"][0]]) and np.array_equal(got["start"][0], clock[got["row"][0], 0])
    per = res.get_slowest_requests(2, window_s=10.0, window_of="arrival")
    assert per["row"].shape == (6, 2) and per["window_of"] == "arrival" and int(per["total"].sum()) <= clock.shape[0]
    w = 1                                                                             # the network spike from 10 s to 16 s
    in_w = (clock[:, 0] > 10.0) & (clock[:, 0] <= 20.0)
    assert per["latency"][w, 0] == lat[in_w].max() and int(per["total"][w]) == int(in_w.sum())
    late = res.get_slowest_requests(4, edges=[59.9, 59.95, 1000.0, 2000.0])
    assert late["row"][2].tolist() == [-1] * 4 and np.isnan(late["latency"][2]).all() and int(late["kept"][2]) == 0
    with pytest.raises(ValueError, match="arrival"):
        res.get_slowest_requests(2, window_of="arrival")
