"""Joint moments of pairs of the sampled series (af_engine_summarize_series_joint) without a GPU: the entry and its struct,
the host definition (results.series_joint_sums) against a plain loop over the rows, the derived statistics
(results.series_joint_statistics) against fractions.Fraction and decimal, the autocorrelation time, and the API surface on a
host stand-in."""

from __future__ import annotations

import ctypes as C
import decimal
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
from asyncflow_amd import _abi
from asyncflow_amd import build as af_build
from asyncflow_amd.plan import lower
from asyncflow_amd.results import (JOINT_STATISTICS, JOINT_SUMS, BatchedResults, ScenarioResults, ShardedResults, autocorrelation_time,
                                   check_series_pairs, load_summary, series_joint_statistics, series_joint_sums, series_names_of,
                                   series_window_stats, tick_window_edges)
from oracle.scenarios import lb_two_servers

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = sorted(p for p in (ROOT / "tests" / "golden").glob("*.npz") if "samples" in np.load(p).files)
FIELDS = ["n_scenarios", "n_groups", "n_windows", "group", "tick_edges", "n_pairs", "a", "b", "lag", "n", "sx", "sy", "sxx", "syy",
          "sxy", "elapsed_ms", "scratch_bytes"]


@pytest.fixture(scope="module")
def lib():
    af_build.build()
    from asyncflow_amd.engine import load_library

    return load_library()


# ------------------------------------------------------------------------------------ the entry and its struct
def test_header_declares_and_library_exports_the_entry(lib):
    header = (ROOT / "include" / "asyncflow_hip.h").read_text()
    assert re.search(r"int\s+af_engine_summarize_series_joint\s*\(\s*af_engine_t\s*\*", header)
    assert re.search(r"#define\s+AF_MAX_SERIES_PAIRS\s+64\b", header) and _abi.MAX_SERIES_PAIRS == 64
    assert "af_engine_summarize_series_joint" in _abi.EXPORTED_SYMBOLS
    assert lib.af_engine_summarize_series_joint.argtypes[2] is C.POINTER(_abi.AfSeriesJoint)
    assert lib.af_abi_version() == 7
    assert asyncflow_amd.check_series_pairs is check_series_pairs and asyncflow_amd.series_joint_sums is series_joint_sums
    assert asyncflow_amd.series_joint_statistics is series_joint_statistics and asyncflow_amd.autocorrelation_time is autocorrelation_time
    for listing in ((ROOT / "asyncflow_amd" / "build.py").read_text(), (ROOT / "asyncflow_amd" / "jit.py").read_text()):
        assert '"af_series_joint.hpp"' in listing
    assert '#include "af_series_joint.hpp"' in (ROOT / "asyncflow_amd" / "csrc" / "engine.hip").read_text()


def test_af_series_joint_layout_matches_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "a host C compiler is needed for the layout probe"
    assert [name for name, _ in _abi.AfSeriesJoint._fields_] == FIELDS  # noqa: SLF001
    src = tmp_path / "probe.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "asyncflow_hip.h"\n'
        'int main(void) { printf("%zu", sizeof(af_series_joint_t));\n'
        + "".join(f'printf(" %zu", offsetof(af_series_joint_t, {f}));\n' for f in FIELDS)
        + 'printf(" %d\\n", AF_MAX_SERIES_PAIRS); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run([cc, "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    P = _abi.AfSeriesJoint
    assert got == [C.sizeof(P), *(getattr(P, f).offset for f in FIELDS), _abi.MAX_SERIES_PAIRS]
    body = re.search(r"typedef struct af_series_joint \{(.*?)\} af_series_joint_t;", (ROOT / "include" / "asyncflow_hip.h").read_text(), re.S)
    assert body and re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S)) == FIELDS


def test_series_joint_entry_refuses_without_a_device(lib):
    from asyncflow_amd.engine import PLAN_ONLY, Engine, EngineUnavailableError

    eng = Engine(lower(lb_two_servers(horizon=20)), PLAN_ONLY)
    try:
        out = _abi.AfOutputs(0, None, 4, None, None)
        edges = (C.c_uint32 * 3)(0, 1, 2)
        a, b, lag = (C.c_uint32 * 1)(0), (C.c_uint32 * 1)(1), (C.c_uint32 * 1)(0)
        req = _abi.AfSeriesJoint(4, 1, 2, None, edges, 1, a, b, lag, None, None, None, None, None, None, 0.0, 0)
        call = lib.af_engine_summarize_series_joint
        assert call(None, C.byref(out), C.byref(req)) == _abi.AF_ERR_INVALID
        assert call(eng._h, None, C.byref(req)) == _abi.AF_ERR_INVALID  # noqa: SLF001
        assert call(eng._h, C.byref(out), None) == _abi.AF_ERR_INVALID  # noqa: SLF001
        assert call(eng._h, C.byref(out), C.byref(req)) == _abi.AF_ERR_NO_DEVICE  # noqa: SLF001
        assert b"planning-only" in lib.af_last_error()
        kw = {"samples_ptr": 0, "tick_capacity": 4, "counts_ptr": 0, "n_ptr": 0, "sxy_ptr": 0}
        with pytest.raises(EngineUnavailableError, match="planning-only"):
            eng.summarize_series_joint(4, 1, [0, 2, 4], [0], [1], [0], **kw)
        # a bad request never reaches the library
        for bad, what in (([0], "at least two"), ([0, 2, 2], "strictly increasing"), ([0.5, 2], "whole")):
            with pytest.raises(ValueError, match=what):
                eng.summarize_series_joint(4, 1, bad, [0], [1], [0], **kw)
        with pytest.raises(ValueError, match="one entry per pair"):
            eng.summarize_series_joint(4, 1, [0, 4], [0, 1], [1], [0], **kw)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------ the host definition and a plain loop
def _fixture(path: Path):
    z = np.load(path)
    plan = lower(json.loads(str(z["payload_json"])))
    words = np.ascontiguousarray(z["samples"]).view(np.uint32)
    counts = np.zeros(_abi.CNT_SLOTS, dtype=np.uint32)
    counts[_abi.CNT_TICKS] = words.shape[1]
    return plan, words, ScenarioResults(plan, counts, np.zeros((0, 2)), words)


def _loop(words, edges, pairs):
    """The definition stated independently: a loop over the windows, the pairs and the rows with Python integers."""
    cols = [[int(v) for v in row] for row in words]
    ticks = words.shape[1]
    W, P = len(edges) - 1, len(pairs[0])
    out = {k: [[0] * P for _ in range(W)] for k in ("n", *JOINT_SUMS)}
    for w in range(W):
        r0, r1 = min(int(edges[w]), ticks), min(int(edges[w + 1]), ticks)
        for p, (a, b, lag) in enumerate(zip(*pairs)):
            xs, ys = cols[int(a)], cols[int(b)]
            for k in range(r0, r1 - int(lag)):
                x, y = xs[k], ys[k + int(lag)]
                out["n"][w][p] += 1
                out["sx"][w][p] += x
                out["sy"][w][p] += y
                out["sxx"][w][p] += x * x
                out["syy"][w][p] += y * y
                out["sxy"][w][p] += x * y
    return out


def _equal_sums(got, want, what):
    for k in ("n", *JOINT_SUMS):
        assert got[k].tolist() == (want[k] if isinstance(want[k], list) else want[k].tolist()), (what, k)


def _int_columns(plan):
    names = series_names_of(plan)
    return [j for j, nm in enumerate(names) if not nm.endswith(":ram_in_use")]


def _shapes(ticks):
    return [("1 tick", 1, tick_window_edges(1, ticks)), ("20 ticks", 20, tick_window_edges(20, ticks)),
            ("200 ticks", 200, tick_window_edges(200, ticks)), ("the whole run", ticks, np.array([0, ticks])),
            ("uneven, past the data", 30, np.array([3, 4, 10, 40, 41, ticks - 1, ticks, ticks + 9, 5 * ticks]))]


@pytest.mark.parametrize("path", GOLDEN, ids=[p.stem for p in GOLDEN])
def test_host_definition_equals_a_loop_over_the_rows(path):
    plan, words, _ = _fixture(path)
    words = words[:, :900]                                   # (a loop over the rows in Python: the first 900 ticks)
    ints = _int_columns(plan)
    first, last, mid = ints[0], ints[-1], ints[len(ints) // 2]
    for what, length, edges in _shapes(words.shape[1]):
        lags = [0, 1, 7, length, length + 1]
        a = np.array([first, first, last, mid, first] + [mid] * len(lags))
        b = np.array([first, last, first, mid, mid] + [last] * len(lags))
        lag = np.array([0, 0, 0, 1, 7] + lags)
        got = series_joint_sums(words, edges, plan.n_edges, (a, b, lag))
        _equal_sums(got, _loop(words, edges, (a, b, lag)), f"{path.stem}, {what}")
        count = np.diff(np.minimum(edges, words.shape[1]))
        assert got["n"].tolist() == np.maximum(count[:, None] - lag[None, :], 0).tolist()
        assert (got["n"][:, 5 + 3] == 0).all() or what.startswith("uneven")      # a lag of the window's length: no pair
        # lag 0: what series_window_stats implies, and (a, b) mirrors (b, a)
        stats = series_window_stats(words, edges, plan.n_edges)
        assert np.array_equal(got["n"][:, 0], stats["count"])
        for w in np.nonzero(count)[0]:
            assert float(got["sx"][w, 0]) / float(count[w]) == stats["mean"][w, first]
            assert got["sxx"][w, 0] == sum(int(v) ** 2 for v in words[first, min(edges[w], 900):min(edges[w + 1], 900)])
        for k, m in (("sx", "sy"), ("sy", "sx"), ("sxx", "syy"), ("syy", "sxx"), ("sxy", "sxy"), ("n", "n")):
            assert got[k][:, 1].tolist() == got[m][:, 2].tolist(), (what, k)


def test_words_to_2_pow_32_fill_the_high_words():
    rng = np.random.default_rng(32)
    words = rng.integers(2 ** 31, 2 ** 32, (5, 300), dtype=np.uint64).astype(np.uint32)
    words[:, ::7] = 0xFFFFFFFF
    pairs = (np.array([0, 0, 1, 3]), np.array([0, 1, 0, 4]), np.array([0, 3, 3, 234]))
    edges = np.array([0, 64, 65, 300, 400])
    got = series_joint_sums(words, edges, 5, pairs)
    _equal_sums(got, _loop(words, edges, pairs), "big words")
    for k in ("sxx", "syy", "sxy"):
        assert all(v >> 64 for v in got[k][0, :3]) and got[k][2, 0] >> 64 >= 50, k
    assert got["sxy"][2, 3] == int(words[3, 65]) * int(words[4, 299]) and got["n"][2, 3] == 1
    assert not np.asarray(got["n"][3]).any() and all(v == 0 for k in JOINT_SUMS for v in got[k][3])
    with pytest.raises(ValueError, match="ram_in_use"):
        series_joint_sums(words, edges, 0, (np.array([2]), np.array([0]), np.array([0])))
    with pytest.raises(ValueError, match="below 5"):
        series_joint_sums(words, edges, 5, (np.array([5]), np.array([0]), np.array([0])))
    with pytest.raises(ValueError, match="lag"):
        series_joint_sums(words, edges, 5, (np.array([1]), np.array([0]), np.array([-1])))
    with pytest.raises(ValueError, match="three vectors"):
        series_joint_sums(words, edges, 5, (np.zeros(65, dtype=int), np.zeros(65, dtype=int), np.zeros(65, dtype=int)))


# ------------------------------------------------------------------------------------ the derived statistics
def _cells_of(xs, ys):
    """The six sums of samples given as two lists of Python integers."""
    return {"n": len(xs), "sx": sum(xs), "sy": sum(ys), "sxx": sum(x * x for x in xs), "syy": sum(y * y for y in ys),
            "sxy": sum(x * y for x, y in zip(xs, ys))}


def _stack(cells):
    out = {"n": np.array([c["n"] for c in cells], dtype=np.int64)}
    for k in JOINT_SUMS:
        out[k] = np.empty(len(cells), dtype=object)
        out[k][:] = [c[k] for c in cells]
    return out


def _ulps(x: float, exact: decimal.Decimal) -> decimal.Decimal:
    return abs(decimal.Decimal(x) - exact) / decimal.Decimal(math.ulp(x))


def _reference(cell):
    """cov, the variances and the means as the correctly rounded float of the exact rational (Fraction); corr in decimal."""
    n, sx, sy, sxx, syy, sxy = (cell[k] for k in ("n", *JOINT_SUMS))
    if n == 0:
        return None
    num, dx, dy = n * sxy - sx * sy, n * sxx - sx * sx, n * syy - sy * sy
    want = {"mean_x": float(Fraction(sx, n)), "mean_y": float(Fraction(sy, n)), "cov": float(Fraction(num, n * n)),
            "var_x": float(Fraction(dx, n * n)), "var_y": float(Fraction(dy, n * n))}
    corr = None
    if dx and dy:
        with decimal.localcontext() as ctx:
            ctx.prec = 80
            corr = decimal.Decimal(num) / (decimal.Decimal(dx) * decimal.Decimal(dy)).sqrt()
    return want, corr


def _check_statistics(cells, what, exact=False):
    st = series_joint_statistics(_stack(cells), exact=exact)
    worst = decimal.Decimal(0)
    for j, cell in enumerate(cells):
        ref = _reference(cell)
        if ref is None:
            assert all(math.isnan(st[k][j]) for k in JOINT_STATISTICS), (what, j)
            continue
        want, corr = ref
        for k, v in want.items():
            assert st[k][j].tobytes() == np.float64(v).tobytes(), (what, j, k, st[k][j], v)
        if corr is None:
            assert math.isnan(st["corr"][j]), (what, j)
        else:
            assert -1.0 <= st["corr"][j] <= 1.0
            worst = max(worst, _ulps(float(st["corr"][j]), corr))
    print(f"{what}: corr within {float(worst):.3g} ulp of the 80-digit value")
    assert worst <= 3, (what, worst)        # three roundings of conversions at 1/2 ulp each carried through, a product, a root, a quotient: 2.25 ulp
    return st


def test_statistics_against_fractions_and_decimal():
    rng = np.random.default_rng(7)
    cells = [{"n": 0, "sx": 0, "sy": 0, "sxx": 0, "syy": 0, "sxy": 0}]
    for top, n in ((8, 3), (40, 100), (2 ** 20, 1000), (2 ** 32, 5), (2 ** 32, 700), (2 ** 32, 4000), (3, 50)):
        for _ in range(12):
            xs = [int(v) for v in rng.integers(0, top, n)]
            ys = [int(v) for v in (rng.integers(0, top, n) if rng.random() < 0.5 else (np.array(xs) // 2 + rng.integers(0, max(top // 8, 1), n)))]
            cells.append(_cells_of(xs, ys))
    cells.append(_cells_of([5] * 9, [1, 2, 3, 4, 5, 6, 7, 8, 9]))        # a constant column: corr NaN, cov 0
    cells.append(_cells_of([1, 2, 3], [7, 7, 7]))
    cells.append(_cells_of([4], [9]))                                    # one sample: both constant
    for exact in (False, True):
        st = _check_statistics(cells, f"random cells, exact={exact}", exact)
        assert math.isnan(st["corr"][-1]) and math.isnan(st["corr"][-2]) and math.isnan(st["corr"][-3]) and st["cov"][-3] == 0.0
        assert st["var_x"][-1] == 0.0 and st["mean_y"][-1] == 9.0
    fast, slow = series_joint_statistics(_stack(cells)), series_joint_statistics(_stack(cells), exact=True)
    for k in JOINT_STATISTICS:
        assert fast[k].tobytes() == slow[k].tobytes(), k


def test_a_series_with_itself_correlates_to_exactly_one():
    rng = np.random.default_rng(11)
    cells = []
    for top, n in ((2, 10), (40, 64), (2 ** 20, 500), (2 ** 32, 2), (2 ** 32, 3000)):
        for _ in range(20):
            xs = [int(v) for v in rng.integers(0, top, n)]
            if len(set(xs)) > 1:
                cells.append(_cells_of(xs, xs))
    for exact in (False, True):
        st = series_joint_statistics(_stack(cells), exact=exact)
        assert (st["corr"] == 1.0).all() and st["cov"].tobytes() == st["var_x"].tobytes() == st["var_y"].tobytes()
    flipped = [_cells_of(xs, [10 - x for x in xs]) for xs in ([1, 2, 3, 9], [0, 10], [3, 4, 3, 4, 7])]
    assert (series_joint_statistics(_stack(flipped))["corr"] == -1.0).all()


def test_both_sides_of_every_switch_agree_with_the_definition():
    """The switches of series_joint_statistics: the six products below 2^63 (int64), |N|, Dx, Dy and n^2 below 2^53 (float64
    division of the moments), the sums below 2^53 (float64 division of the means)."""
    cells = []
    v = math.isqrt(2 ** 61)                                  # n * sxx = 2 (v^2 + (v + 1)^2) ~ 4 v^2 crosses 2^63 near v = 2^30.5
    for d in (-3, -2, -1, 0, 1, 2, 3):
        cells.append(_cells_of([v + d, v + d + 1], [v + d + 1, v + d - 5]))
    assert 2 * cells[0]["sxx"] < 2 ** 63 < 2 * cells[-1]["sxx"]
    for n, x in ((2 ** 31, 2 ** 32 - 1), (2 ** 31 - 1, 2 ** 32 - 1), (3, 2 ** 32 - 1)):      # sx * sx at and around 2^63 .. 2^126
        cells.append({"n": n, "sx": (n - 1) * x, "sy": n - 1, "sxx": (n - 1) * x * x, "syy": n - 1, "sxy": (n - 1) * x})
    r = math.isqrt(2 ** 53)                                  # 94 906 265: (x1 - x2)^2 = Dx of two samples crosses 2^53
    assert r == 94906265 and r * r < 2 ** 53 < (r + 1) ** 2
    for d in (r - 1, r, r + 1, r + 2):
        cells.append(_cells_of([7, 7 + d], [3 + d, 3]))
        assert (cells[-1]["n"] * cells[-1]["sxx"] - cells[-1]["sx"] ** 2 < 2 ** 53) == (d <= r)
    for n in (r - 1, r, r + 1, r + 2):                       # n^2 crosses 2^53: a column of 1 000 ones among zeros
        cells.append({"n": n, "sx": 1000, "sy": 999, "sxx": 1000, "syy": 999, "sxy": 999})
    for n in (2 ** 21 - 1, 2 ** 21, 2 ** 21 + 1, 2 ** 21 + 2):                                # sx = n (2^32 - 1) crosses 2^53
        x = 2 ** 32 - 1
        cells.append({"n": n + 1, "sx": n * x, "sy": n * 3, "sxx": n * x * x, "syy": n * 9, "sxy": n * x * 3})
    assert cells[-4]["sx"] < 2 ** 53 < cells[-2]["sx"]
    _check_statistics(cells, "cells at the switches")
    fast, slow = series_joint_statistics(_stack(cells)), series_joint_statistics(_stack(cells), exact=True)
    for k in JOINT_STATISTICS:
        assert fast[k].tobytes() == slow[k].tobytes(), k
    # the device's form of the 128-bit sums: uint64 words, low word first
    words = _stack(cells)
    for k in ("sxx", "syy", "sxy"):
        words[k] = np.array([[c[k] & (2 ** 64 - 1), c[k] >> 64] for c in cells], dtype=np.uint64)
    for k in ("sx", "sy"):
        words[k] = np.array([c[k] for c in cells], dtype=np.uint64)
    again = series_joint_statistics(words)
    for k in JOINT_STATISTICS:
        assert again[k].tobytes() == slow[k].tobytes(), k
    shaped = series_joint_statistics({k: np.asarray(v).reshape(2, -1, *np.asarray(v).shape[1:]) for k, v in words.items()})
    assert shaped["corr"].shape == (2, len(cells) // 2) and shaped["cov"].tobytes() == slow["cov"].tobytes()


# ------------------------------------------------------------------------------------ the autocorrelation time
def test_autocorrelation_time_of_hand_made_functions():
    nan = float("nan")
    acf = np.array([[1.0, 0.5, 0.25, -0.1, 0.3],        # stops at lag 3: 1 + 2 (0.5 + 0.25)
                    [1.0, 0.5, 0.4, 0.3, 0.2],          # never stops: truncated
                    [1.0, -0.2, 0.9, 0.9, 0.9],         # stops at lag 1: white noise or faster
                    [1.0, 0.0, 0.5, 0.5, 0.5],          # 0 stops too
                    [1.0, 0.5, nan, 0.5, 0.5],          # a NaN stops
                    [nan, nan, nan, nan, nan],          # a constant series or an empty cell
                    [1.0, 0.1, 0.2, 0.3, 0.0]])
    got = autocorrelation_time(acf, [100, 200, 50, 10, 10, 70, 7])
    assert got["tau"].tolist()[:5] == [2.5, 1.0 + 2.0 * (((0.5 + 0.4) + 0.3) + 0.2), 1.0, 1.0, 2.0] and math.isnan(got["tau"][5])
    assert got["tau"][6] == 1.0 + 2.0 * ((0.1 + 0.2) + 0.3)
    assert got["tau_truncated"].tolist() == [False, True, False, False, False, False, False]
    assert got["ess"].tolist()[:5] == [40.0, 200.0 / got["tau"][1], 50.0, 10.0, 5.0] and math.isnan(got["ess"][5])
    only = autocorrelation_time(np.array([[1.0], [nan]]), [9, 9])                  # max_lag = 0: no lag to stop at
    assert only["tau"][0] == 1.0 and only["tau_truncated"].tolist() == [True, False] and only["ess"][0] == 9.0
    cube = autocorrelation_time(np.broadcast_to(acf, (2, 3, 7, 5)), np.full((2, 3, 7), 10))
    assert cube["tau"].shape == (2, 3, 7) and cube["tau"][1, 2, 0] == 2.5
    with pytest.raises(ValueError, match="lag 0"):
        autocorrelation_time(np.zeros((3, 0)), [1, 1, 1])


def _acf_of(x, max_lag, edges):
    words = np.asarray(x, dtype=np.uint32)[None, :]
    lags = np.arange(max_lag + 1)
    sums = series_joint_sums(words, edges, 1, (np.zeros_like(lags), np.zeros_like(lags), lags))
    return series_joint_statistics(sums)["corr"], sums["n"]


def test_autocorrelation_of_an_ar1_like_and_of_a_constant_sequence():
    rng = np.random.default_rng(3)
    n, phi = 20000, 0.8
    x, level = np.zeros(n, dtype=np.int64), 0.0
    for k in range(n):                                       # an AR(1) about 1 000, rounded to integers
        level = phi * level + rng.normal(0.0, 60.0)
        x[k] = int(round(1000.0 + level))
    assert x.min() > 0
    acf, cnt = _acf_of(x, 60, [0, n])
    assert acf[0, 0] == 1.0 and cnt[0].tolist() == (n - np.arange(61)).tolist()
    np.testing.assert_allclose(acf[0, 1:6], phi ** np.arange(1, 6), atol=0.03)
    got = autocorrelation_time(acf, cnt[:, 0])
    want = (1.0 + phi) / (1.0 - phi)                          # 9
    assert not got["tau_truncated"][0] and abs(got["tau"][0] - want) < 1.5 and math.isfinite(got["tau"][0])
    assert got["ess"][0] == n / got["tau"][0]
    short = autocorrelation_time(acf[:, :4], cnt[:, 0])        # three lags are too few
    assert short["tau_truncated"][0] and short["tau"][0] < got["tau"][0]
    flat, cnt = _acf_of(np.full(500, 7), 10, [0, 250, 500])
    assert np.isnan(flat).all() and cnt[:, 0].tolist() == [250, 250]
    got = autocorrelation_time(flat, cnt[:, 0])
    assert np.isnan(got["tau"]).all() and np.isnan(got["ess"]).all() and not got["tau_truncated"].any()


# ------------------------------------------------------------------------------------ the API surface
NAMES = ["e-1:edge_concurrent_connection", "e-2:edge_concurrent_connection", "srv-1:ready_queue_len", "srv-1:event_loop_io_sleep",
         "srv-1:ram_in_use", "srv-2:ready_queue_len", "srv-2:event_loop_io_sleep", "srv-2:ram_in_use"]


def test_check_series_pairs():
    labels, a, b, lag = check_series_pairs({"queues": ("srv-1:ready_queue_len", "srv-2:ready_queue_len"), "lead": (0, "srv-1:ready_queue_len", 4),
                                            "self": (np.int64(3), 3, np.int32(7))}, NAMES, 2)
    assert labels == ["queues", "lead", "self"] and a.tolist() == [2, 0, 3] and b.tolist() == [5, 2, 3] and lag.tolist() == [0, 4, 7]
    assert a.dtype == b.dtype == lag.dtype == np.int64
    assert check_series_pairs([("x", (1, 0, 2 ** 31 - 1))], NAMES, 2)[3].tolist() == [2 ** 31 - 1]
    many = {f"p{i}": (0, 1, i) for i in range(65)}
    for bad, what in (({}, "1 .. 64 pairs"), (many, "1 .. 64 pairs"), ([("a", (0, 1)), ("a", (1, 0))], "given twice"),
                      ({"a": (0,)}, r"must be \(a, b\)"), ({"a": (0, 1, 2, 3)}, r"must be \(a, b\)"), ({"a": "srv-1:ready_queue_len"}, r"must be \(a, b\)"),
                      ({"a": ("nobody:ready_queue_len", 0)}, "unknown series"), ({"a": (0, 8)}, "no series name or index below 8"),
                      ({"a": (-1, 0)}, "no series name or index"), ({"a": (0, 1.0)}, "no series name or index"), ({"a": (True, 0)}, "no series name or index"),
                      ({"a": (0, "srv-1:ram_in_use")}, "ram_in_use"), ({"a": (7, 0)}, "ram_in_use"),
                      ({"a": (0, 1, -1)}, "lag"), ({"a": (0, 1, 2 ** 31)}, "lag"), ({"a": (0, 1, 1.5)}, "lag"), ({"a": (0, 1, True)}, "lag")):
        with pytest.raises(ValueError, match=what):
            check_series_pairs(bad, NAMES, 2)


def test_a_scenario_from_the_host_definition():
    plan, words, res = _fixture(ROOT / "tests" / "golden" / "lb2_rr_t30.npz")
    names = series_names_of(plan)
    q = [nm for nm in names if nm.endswith(":ready_queue_len")]
    pairs = {"queues": (q[0], q[1]), "lead": (q[0], q[1], 3), "acf5": (q[0], q[0], 5)}
    got = res.get_series_joint(pairs, ticks_per_window=500)
    labels, a, b, lag = check_series_pairs(pairs, names, plan.n_edges)
    edges = tick_window_edges(500, plan.tick_count)
    want = series_joint_sums(words, edges, plan.n_edges, (a, b, lag))
    _equal_sums(got, want, "a scenario")
    st = series_joint_statistics(want)
    for k in JOINT_STATISTICS:
        assert got[k].tobytes() == st[k].tobytes() and got[k].shape == (len(edges) - 1, 3), k
    assert got["labels"] == labels and got["lag"].tolist() == [0, 3, 5] and np.array_equal(got["tick_edges"], edges)
    assert np.isfinite(got["corr"]).any()
    with pytest.raises(ValueError, match="ram_in_use"):
        res.get_series_joint({"x": (q[0], [nm for nm in names if nm.endswith(":ram_in_use")][0])})
    none = ScenarioResults(plan, res.counts, np.zeros((0, 2)), None)
    with pytest.raises(RuntimeError, match="kept no sampled series"):
        none.get_series_joint(pairs)


def _pooled_sums(words_of, ids, n_groups, b, n_edges, pairs):
    """The host definition of a group: series_joint_sums of its members, added."""
    W, P = len(b) - 1, len(pairs[0])
    out = {"n": np.zeros((n_groups, W, P), dtype=np.int64)}
    for k in JOINT_SUMS:
        out[k] = np.zeros((n_groups, W, P), dtype=object)
        out[k][...] = 0
    for s, g in enumerate(ids):
        if g < 0:
            continue
        one = series_joint_sums(words_of[s], b, n_edges, pairs)
        for k in out:
            out[k][g] = out[k][g] + one[k]
    return out


class _HostBatch(BatchedResults):
    """A batch of host arrays whose joint call is the host definition, group by group."""

    def _series_joint_call(self, ca, cb, lag, b, ids, n_groups):
        self.calls.append(len(ca))
        return _pooled_sums(self.host_words, ids, n_groups, b, self.plan.n_edges, (ca, cb, lag)), 0.0, 0


def _host_batch():
    plan = lower(lb_two_servers(horizon=10))
    rng = np.random.default_rng(21)
    n, ticks = 6, plan.tick_count
    batch = _HostBatch.__new__(_HostBatch)
    batch.plan = plan
    batch.counts = np.zeros((n, _abi.CNT_SLOTS), dtype=np.uint32)
    batch._samples_t = object()  # noqa: SLF001
    batch._summ_engine = None  # noqa: SLF001
    batch.calls = []
    walk = np.cumsum(rng.integers(-1, 2, (n, plan.n_series, ticks)), axis=2)
    batch.host_words = (walk - walk.min() + rng.integers(0, 3, walk.shape)).astype(np.uint32)
    return batch, np.array([0, 1, 0, 1, -1, 1])


PAIRS = {"queues": ("srv-1:ready_queue_len", "srv-2:ready_queue_len"), "lead": ("srv-1:ready_queue_len", "srv-2:ready_queue_len", 4),
         "sleepers": ("srv-2:event_loop_io_sleep", "srv-1:event_loop_io_sleep", 1)}


def _bits(a) -> bytes:
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def test_summary_and_bands_of_a_host_batch():
    batch, ids = _host_batch()
    names = batch.series_names()
    labels, a, b, lag = check_series_pairs(PAIRS, names, batch.plan.n_edges)
    edges = tick_window_edges(100, batch.plan.tick_count)
    W = len(edges) - 1
    pooled = batch.series_joint_summary(PAIRS, ticks_per_window=100, by=ids)
    want = _pooled_sums(batch.host_words, ids, 2, edges, batch.plan.n_edges, (a, b, lag))
    _equal_sums(pooled, want, "pooled")
    st = series_joint_statistics(want)
    for k in JOINT_STATISTICS:
        assert _bits(pooled[k]) == _bits(st[k]) and pooled[k].shape == (2, W, 3)
    assert pooled["labels"] == labels and pooled["replicas"].tolist() == [2, 3] and np.array_equal(pooled["times"], edges[:-1] * batch.plan.sample_period)
    per = batch.series_joint_summary(PAIRS, ticks_per_window=100, by="scenario")
    for of in ("corr", "cov"):
        bands = batch.series_joint_bands(PAIRS, ticks_per_window=100, by=ids, of=of)
        assert bands["mean"].shape == bands["q_lo"].shape == bands["pooled"].shape == bands["n"].shape == (2, W, 3)
        assert _bits(bands["pooled"]) == _bits(pooled[of]) and bands["of"] == of and bands["labels"] == labels
        for g in range(2):
            np.testing.assert_allclose(bands["mean"][g], per[of][ids == g].mean(axis=0), rtol=1e-12, atol=1e-15)
            np.testing.assert_allclose(bands["q_hi"][g], np.quantile(per[of][ids == g], 0.95, axis=0), rtol=1e-12, atol=1e-15)
        assert bands["replicas"].tolist() == [2, 3] and (bands["n"] == np.array([2, 3])[:, None, None]).all()
    # a replica whose column is constant in a window does not count there
    batch.host_words[0, names.index("srv-1:ready_queue_len"), :100] = 5
    bands = batch.series_joint_bands(PAIRS, ticks_per_window=100, by=ids)
    assert bands["n"][0, 0].tolist() == [1, 1, 2] and bands["n"][0, 1].tolist() == [2, 2, 2] and np.isfinite(bands["mean"][0, 0]).all()


def test_autocorrelation_summary_of_a_host_batch():
    batch, ids = _host_batch()
    names = batch.series_names()
    out = batch.series_autocorrelation_summary("*:ready_queue_len", 40, ticks_per_window=500, by=ids)
    cols = [names.index("srv-1:ready_queue_len"), names.index("srv-2:ready_queue_len")]
    assert out["series"] == [names[c] for c in cols] and out["columns"].tolist() == cols and out["lags"].tolist() == list(range(41))
    assert batch.calls == [64, 18] and out["calls"] == 2                                       # 82 pairs: two calls
    edges = tick_window_edges(500, batch.plan.tick_count)
    W = len(edges) - 1
    assert out["acf"].shape == out["n"].shape == (2, W, 2, 41) and out["tau"].shape == out["ess"].shape == out["tau_truncated"].shape == (2, W, 2)
    for i, c in enumerate(cols):
        lags = np.arange(41)
        sums = _pooled_sums(batch.host_words, ids, 2, edges, batch.plan.n_edges, (np.full(41, c), np.full(41, c), lags))
        assert _bits(out["acf"][:, :, i]) == _bits(series_joint_statistics(sums)["corr"]) and np.array_equal(out["n"][:, :, i], sums["n"])
    assert (out["acf"][..., 0] == 1.0).all() and (out["tau"] > 1.0).all()                       # random walks: strongly autocorrelated
    want = autocorrelation_time(out["acf"], out["n"][..., 0])
    for k in ("tau", "ess", "tau_truncated"):
        assert np.array_equal(out[k], want[k], equal_nan=True), k
    one = batch.series_autocorrelation_summary([cols[1]], 0, ticks_per_window=500)
    assert one["acf"].shape == (1, W, 1, 1) and one["tau_truncated"].all()
    for bad, what in ((("*:ram_in_use", 3), "ram_in_use"), (("*:nothing", 3), "matches no series"), (("srv-1:ready_queue_len", -1), "max_lag"),
                      (("srv-1:ready_queue_len", 1.5), "max_lag"), ((["srv-1:ready_queue_len", cols[0]], 2), "twice"), (("nobody", 2), "unknown series")):
        with pytest.raises(ValueError, match=what):
            batch.series_autocorrelation_summary(*bad)


@pytest.mark.parametrize("ext", ["npz", "parquet"])
def test_on_disk_round_trip(tmp_path, ext):
    if ext == "parquet":
        pytest.importorskip("pyarrow")
    batch, ids = _host_batch()
    path = str(tmp_path / f"series_joint.{ext}")
    written = batch.save_series_joint_summary(path, ids, pairs=PAIRS, ticks_per_window=50)
    back = load_summary(path)
    assert set(back) == set(written)
    for k, v in written.items():
        assert np.array_equal(np.asarray(back[k], dtype=v.dtype), v, equal_nan=True), k
    W = -(-batch.plan.tick_count // 50)
    want = batch.series_joint_summary(PAIRS, ticks_per_window=50, by=ids)
    bands = batch.series_joint_bands(PAIRS, ticks_per_window=50, by=ids)
    assert back["replicas"].tolist() == [2, 3]
    assert set(back) == {"replicas", "series_joint_tick_edges", "series_joint_times",
                         *(f"series_joint_{k}:{name}" for k in ("corr", "cov", "n", "q05", "q95") for name in PAIRS)}
    for p, name in enumerate(PAIRS):
        assert back[f"series_joint_corr:{name}"].shape == (2, W)
        assert _bits(back[f"series_joint_corr:{name}"]) == _bits(want["corr"][:, :, p]) and _bits(back[f"series_joint_cov:{name}"]) == _bits(want["cov"][:, :, p])
        assert np.array_equal(back[f"series_joint_n:{name}"], want["n"][:, :, p])
        assert _bits(back[f"series_joint_q05:{name}"]) == _bits(bands["q_lo"][:, :, p]) and _bits(back[f"series_joint_q95:{name}"]) == _bits(bands["q_hi"][:, :, p])
    assert np.array_equal(back["series_joint_tick_edges"], want["tick_edges"]) and np.array_equal(back["series_joint_times"], want["times"])


def test_refusals_of_the_batch_layer():
    plan = lower(lb_two_servers(horizon=10))
    batch = BatchedResults.__new__(BatchedResults)
    batch.plan = plan
    batch._samples_t = None  # noqa: SLF001
    ok = {"q": ("srv-1:ready_queue_len", "srv-2:ready_queue_len")}
    for call in (batch.series_joint_summary, batch.series_joint_bands):
        with pytest.raises(RuntimeError, match="kept no sampled series"):
            call(ok)
    with pytest.raises(RuntimeError, match="kept no sampled series"):
        batch.series_autocorrelation_summary("srv-1:ready_queue_len", 3)
    with pytest.raises(RuntimeError, match="kept no sampled series"):
        batch.save_series_joint_summary("nowhere.npz", pairs=ok, ticks_per_window=10)
    batch._samples_t = object()  # noqa: SLF001  (the checks below come before the device is touched)
    with pytest.raises(ValueError, match="ram_in_use"):
        batch.series_joint_summary({"q": ("srv-1:ready_queue_len", "srv-1:ram_in_use")})
    with pytest.raises(ValueError, match="unknown series"):
        batch.series_joint_summary({"q": ("srv-1:ready_queue_len", "srv-9:ready_queue_len")})
    with pytest.raises(ValueError, match="lag"):
        batch.series_joint_summary({"q": ("srv-1:ready_queue_len", "srv-2:ready_queue_len", -2)})
    with pytest.raises(ValueError, match="one of"):
        batch.series_joint_summary(ok, 1.0, ticks_per_window=10)
    with pytest.raises(ValueError, match="of must be"):
        batch.series_joint_bands(ok, of="mean")


def test_sharded_results_refuse_series_pairs():
    sh = ShardedResults.__new__(ShardedResults)
    for call in (sh.series_joint_summary, sh.series_joint_bands, sh.save_series_joint_summary, sh.series_autocorrelation_summary):
        with pytest.raises(NotImplementedError, match="several devices"):
            call({})
