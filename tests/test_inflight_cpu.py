"""Requests in flight, CPU side: the C entry point and its struct, and the host definitions
(`results.in_flight_series`, `results.in_flight_window_stats`) that `af_engine_summarize_inflight` is held to word for word --
against a brute-force double loop over rows and ticks, the identities that must hold exactly, the per-row bound that ties the
count to the latency, and the committed golden clocks."""

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
from asyncflow_amd.results import ScenarioResults, in_flight_series, in_flight_window_stats, series_histogram_quantiles
from oracle.scenarios import lb_two_servers

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def lib():
    af_build.build()
    from asyncflow_amd.engine import load_library

    return load_library()


def test_header_declares_and_library_exports_the_entry(lib):
    header = (ROOT / "include" / "asyncflow_hip.h").read_text()
    assert re.search(r"int\s+af_engine_summarize_inflight\s*\(\s*af_engine_t\s*\*", header)
    assert "af_engine_summarize_inflight" in _abi.EXPORTED_SYMBOLS
    assert lib.af_engine_summarize_inflight.argtypes[2] is C.POINTER(_abi.AfInflight)
    assert lib.af_abi_version() == 7
    sources = (ROOT / "asyncflow_amd" / "build.py").read_text()
    assert '"af_inflight.hpp"' in sources and '"af_inflight.hpp"' in (ROOT / "asyncflow_amd" / "jit.py").read_text()


def test_af_inflight_layout_matches_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "a host C compiler is needed for the layout probe"
    fields = [name for name, _ in _abi.AfInflight._fields_]  # noqa: SLF001
    assert fields == ["n_scenarios", "n_groups", "n_windows", "group", "tick_edges", "sample_period", "threshold", "n_bins", "lo", "count",
                      "sum", "minv", "maxv", "above", "hist", "under", "in_flight", "started", "finished", "elapsed_ms", "scratch_bytes"]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "asyncflow_hip.h"\n'
                   'int main(void) { printf("%zu", sizeof(af_inflight_t));\n'
                   + "".join(f'printf(" %zu", offsetof(af_inflight_t, {f}));\n' for f in fields) + 'printf("\\n"); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run([cc, "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    P = _abi.AfInflight
    assert got == [C.sizeof(P), *(getattr(P, f).offset for f in fields)]


def test_entry_refuses_without_a_device(lib):
    from asyncflow_amd.engine import PLAN_ONLY, Engine, EngineUnavailableError

    eng = Engine(lower(lb_two_servers(horizon=20)), PLAN_ONLY)
    try:
        out = _abi.AfOutputs(4, None, 8, None, None)
        edges = (C.c_uint32 * 3)(0, 1, 2)
        req = _abi.AfInflight(4, 1, 2, None, edges, 0.5)
        assert lib.af_engine_summarize_inflight(None, C.byref(out), C.byref(req)) == _abi.AF_ERR_INVALID
        assert lib.af_engine_summarize_inflight(eng._h, None, C.byref(req)) == _abi.AF_ERR_INVALID  # noqa: SLF001
        assert lib.af_engine_summarize_inflight(eng._h, C.byref(out), None) == _abi.AF_ERR_INVALID  # noqa: SLF001
        assert lib.af_engine_summarize_inflight(eng._h, C.byref(out), C.byref(req)) == _abi.AF_ERR_NO_DEVICE  # noqa: SLF001
        assert b"planning-only" in lib.af_last_error()
        with pytest.raises(EngineUnavailableError, match="planning-only"):
            eng.summarize_inflight(4, 1, [0, 4], 0.5, clock_ptr=0, clock_capacity=4, tick_capacity=8, counts_ptr=0, count_ptr=0, sum_ptr=0)
        with pytest.raises(ValueError, match="at least two"):
            eng.summarize_inflight(4, 1, [0], 0.5, clock_ptr=0, clock_capacity=4, tick_capacity=8, counts_ptr=0, count_ptr=0, sum_ptr=0)
        with pytest.raises(ValueError, match="threshold"):
            eng.summarize_inflight(4, 1, [0, 4], 0.5, clock_ptr=0, clock_capacity=4, tick_capacity=8, counts_ptr=0, count_ptr=0, sum_ptr=0,
                                   threshold=-1)
    finally:
        eng.close()


def _brute(rows: np.ndarray, t_s: int, p: float) -> dict[str, np.ndarray]:
    """The definition as a double loop over rows and ticks, with Python floats and integers."""
    import math

    started, finished, in_flight = ([0] * t_s for _ in range(3))
    for s, f in rows.tolist():
        if math.isnan(s) or math.isnan(f) or s < 0.0:
            continue
        qa, qf = s / p, f / p
        qa = qa if math.isinf(qa) else float(math.floor(qa))
        qf = qf if math.isinf(qf) else float(math.floor(qf))
        if qf <= qa or qa >= t_s:
            continue
        first = True
        for k in range(t_s):
            if qa <= k < qf:
                in_flight[k] += 1
                if first:
                    started[k] += 1            # (the first row that counts it is max(a_i, 0) = a_i)
                    first = False
            if qf == k:
                finished[k] += 1
    return {"started": np.array(started, dtype=np.uint32), "finished": np.array(finished, dtype=np.uint32),
            "in_flight": np.array(in_flight, dtype=np.uint32)}


def _random_rows(rng: np.random.Generator, m: int, t_s: int, p: float) -> np.ndarray:
    start = rng.integers(-8, 4 * (t_s + 6), m) * (p / 4.0) + rng.choice([0.0, 0.0, p * 2.0 ** -30, -p * 2.0 ** -30], m)
    lat = rng.choice([0.0, p / 4, p / 2, p, 3 * p, 17 * p, (t_s + 50) * p, 1e300, np.inf], m, p=[0.1, 0.1, 0.1, 0.15, 0.2, 0.2, 0.1, 0.025, 0.025])
    rows = np.stack([start, start + lat], axis=1)
    for k, bad in enumerate(([np.nan, 1.0], [1.0, np.nan], [-p, 5 * p], [3 * p, p], [-0.0, 2 * p], [np.inf, np.inf], [p, -np.inf])):
        if m > k:
            rows[rng.integers(0, m)] = bad
    return rows


@pytest.mark.parametrize("period", [2.0 ** -5, 0.25, 0.01, 0.3, 1.0 / 3.0])
def test_series_equal_the_brute_force_loop_and_the_identities_hold(period):
    rng = np.random.default_rng(int(period * 1e6))
    for m, t_s in ((0, 0), (0, 5), (1, 1), (40, 13), (300, 64), (500, 97)):
        rows = _random_rows(rng, m, t_s, period)           # unsorted starts, times on and beside the tick instants
        got, want = in_flight_series(rows, t_s, period), _brute(rows, t_s, period)
        for key in ("started", "finished", "in_flight"):
            assert got[key].dtype == np.uint32 and np.array_equal(got[key], want[key]), (key, m, t_s)
        s, f, v = (got[k].astype(np.int64) for k in ("started", "finished", "in_flight"))
        assert np.array_equal(v, np.cumsum(s) - np.cumsum(f))   # finished[k] is taken before row k is read
        with np.errstate(invalid="ignore", over="ignore"):
            qa, qf = np.floor(rows[:, 0] / period), np.floor(rows[:, 1] / period)
            ok = (rows[:, 0] >= 0) & ~np.isnan(rows[:, 1]) & (qa < t_s) & (qf > qa)
        assert int(v.sum()) == int((np.minimum(qf[ok], t_s) - np.maximum(qa[ok], 0)).sum())
        assert int(s.sum()) == int(ok.sum()) and int(f.sum()) == int((ok & (qf < t_s)).sum())
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="period"):
            in_flight_series(np.zeros((1, 2)), 4, bad)
    with pytest.raises(ValueError, match="ticks"):
        in_flight_series(np.zeros((1, 2)), -1, 0.5)


def test_dyadic_times_tie_the_count_to_the_latency_row_by_row():
    """With a dyadic period and dyadic times the quotient is exact: floor(x) <= x < floor(x) + 1 for start / p and finish / p,
    so |(f_i - a_i) p - (finish_i - start_i)| < p for every row with a_i >= 0, hence |p sum(in_flight) - sum(latency)| < m p over
    unclipped rows."""
    rng = np.random.default_rng(11)
    p, t_s, m = 2.0 ** -5, 4000, 3000
    start = rng.integers(0, 3000 * 64, m) * 2.0 ** -11
    lat = rng.integers(0, 40 * 64, m) * 2.0 ** -11           # ends before tick 3000 + 40 < t_s: nothing is clipped
    rows = np.stack([start, start + lat], axis=1)
    a, f = np.floor(rows[:, 0] / p), np.floor(rows[:, 1] / p)
    assert (np.abs((f - a) * p - lat) < p).all()
    got = in_flight_series(rows, t_s, p)["in_flight"].astype(np.int64)
    assert int(got.sum()) == int((f - a).sum())              # rows with f_i == a_i count nowhere and add 0 on both sides
    assert abs(p * float(got.sum()) - float(lat.sum())) < m * p


def _fixture(name: str):
    z = np.load(ROOT / "tests" / "golden" / f"{name}.npz")
    plan = lower(json.loads(str(z["payload_json"])))
    clock = np.asarray(z["clock"], dtype=np.float64).reshape(-1, 2)
    counts = np.zeros(_abi.CNT_SLOTS, dtype=np.uint32)
    counts[_abi.CNT_COMPLETED] = clock.shape[0]
    counts[_abi.CNT_TICKS] = plan.tick_count
    return plan, clock, ScenarioResults(plan, counts, clock, None)


@pytest.mark.parametrize("name", ["lb2_events_t60", "overload_t30"])
def test_golden_clocks(name):
    plan, clock, res = _fixture(name)
    t_s, p = plan.tick_count, plan.sample_period
    got = in_flight_series(clock, t_s, p)
    s, f, v = (got[k].astype(np.int64) for k in ("started", "finished", "in_flight"))
    assert v.shape == (t_s,) and np.array_equal(v, np.cumsum(s) - np.cumsum(f))
    qa, qf = np.floor(clock[:, 0] / p), np.floor(clock[:, 1] / p)
    ok = (qa < t_s) & (qf > qa)
    assert int(v.sum()) == int((np.minimum(qf[ok], t_s) - qa[ok]).sum())
    assert 0 < int(v.max()) <= clock.shape[0]
    # p * sum(in_flight) over the rows that end within the samples is the time they spent in the system up to the rounding of
    # every row to ticks: less than one period a row
    clipped = int((t_s - qa[ok & (qf >= t_s)]).sum())
    assert abs(p * float(v.sum() - clipped) - float((clock[:, 1] - clock[:, 0])[qf < t_s].sum())) <= clock.shape[0] * p
    times, vals = res.get_in_flight()
    assert len(times) == t_s and times[1] == p and np.array_equal(np.asarray(vals), v.astype(np.float64))
    if name == "lb2_events_t60":   # a network spike on client-lb from 10 s to 16 s: the backlog builds during it
        at = lambda t0, t1: float(v[int(t0 / p): int(t1 / p)].mean())   # noqa: E731
        assert at(11.0, 16.0) > 1.5 * at(2.0, 9.0)


def _numpy_stats(members: list[np.ndarray], b: list[int], thr: int, bins: int, lo: int) -> dict[str, list]:
    out: dict[str, list] = {k: [] for k in ("count", "sum", "min", "max", "above", "under", "hist")}
    for w in range(len(b) - 1):
        v = np.concatenate([np.asarray(r[b[w]: b[w + 1]], dtype=np.int64) for r in members])
        out["count"].append(v.size)
        out["sum"].append(int(v.sum()))
        out["min"].append(int(v.min()) if v.size else 0)
        out["max"].append(int(v.max()) if v.size else 0)
        out["above"].append(int(np.count_nonzero(v > thr)))
        out["under"].append(int(np.count_nonzero(v < lo)))
        out["hist"].append([int(np.count_nonzero(v == lo + k)) if k < bins - 1 else int(np.count_nonzero(v >= lo + k)) for k in range(bins)])
    return out


def test_window_statistics_equal_numpy_with_empty_cells_overflow_and_underflow():
    rng = np.random.default_rng(3)
    members = [rng.integers(0, 12, 50).astype(np.uint32), rng.integers(3, 9, 31).astype(np.uint32), np.zeros(0, dtype=np.uint32)]
    edges = [0, 1, 10, 31, 40, 50, 60, 75]                      # the second member ends inside a window; two windows are empty
    for thr, bins, lo in ((0, 0, 0), (5, 4, 0), (11, 6, 3), (3, 1, 5), (2, 20, 0)):
        got = in_flight_window_stats(members, edges, thr, bins, lo)
        want = _numpy_stats(members, edges, thr, max(bins, 1), lo)
        for key in ("count", "sum", "min", "max", "above") + (("under", "hist") if bins else ()):
            assert np.array_equal(np.asarray(got[key]).astype(np.int64), np.asarray(want[key], dtype=np.int64)), (key, thr, bins, lo)
        assert ("hist" in got) == bool(bins)
        assert got["count"][-1] == 0 and got["count"][-2] == 0 and got["sum"].dtype == np.uint64
        if bins:
            assert np.array_equal(got["under"] + got["hist"].sum(axis=1), got["count"])
    one = in_flight_window_stats(members[0], [0, 50], 0, 16, 0)
    assert one["count"][0] == 50
    # exact quantiles off the histogram, through the reader of the series histograms, unchanged
    summ = {"hist": one["hist"][:, None, :], "under": one["under"][:, None], "count": one["count"],
            "bin_edges": np.arange(17, dtype=np.float64)[None, :], "ram": np.zeros(1, dtype=bool)}
    q = series_histogram_quantiles(summ, [0.0, 0.5, 0.9, 1.0])
    assert np.array_equal(q[0, 0], np.quantile(members[0].astype(np.float64), [0.0, 0.5, 0.9, 1.0]))
    for bad in ({"threshold": -1}, {"bins": 1025}, {"lo": 2 ** 32}, {"bins": 1.5}):
        with pytest.raises(ValueError):
            in_flight_window_stats(members, edges, **bad)
