"""Warm-up truncation of the sampled series (af_engine_summarize_series_warmup) without a GPU: the entry and its struct, the
host definition (results.series_warmup_sums) on cases worked by hand and against a plain walk, the statistics against
fractions.Fraction, and the API surface on a host stand-in."""

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
from asyncflow_amd import _abi
from asyncflow_amd import build as af_build
from asyncflow_amd.plan import lower
from asyncflow_amd.results import (WARMUP_STATISTICS, WARMUP_SUMS, BatchedResults, ScenarioResults, ShardedResults, check_warmup_batch,
                                   load_summary, ram_columns, series_names_of, series_warmup_cut, series_warmup_statistics,
                                   series_warmup_sums, tick_window_edges, warmup_truncation)
from oracle.scenarios import lb_two_servers

ROOT = Path(__file__).resolve().parent.parent
FIELDS = ["n_scenarios", "n_groups", "n_windows", "group", "tick_edges", "n_columns", "columns", "batch", "batches", "trunc", "s1", "s2",
          "s1_all", "s2_all", "elapsed_ms", "scratch_bytes"]


@pytest.fixture(scope="module")
def lib():
    af_build.build()
    from asyncflow_amd.engine import load_library

    return load_library()


# ------------------------------------------------------------------------------------ the entry and its struct
def test_header_declares_and_library_exports_the_entry(lib):
    header = (ROOT / "include" / "asyncflow_hip.h").read_text()
    assert re.search(r"int\s+af_engine_summarize_series_warmup\s*\(\s*af_engine_t\s*\*", header)
    assert re.search(r"#define\s+AF_MAX_SERIES_WARMUP_COLUMNS\s+64\b", header) and _abi.MAX_SERIES_WARMUP_COLUMNS == 64
    assert "af_engine_summarize_series_warmup" in _abi.EXPORTED_SYMBOLS
    assert lib.af_engine_summarize_series_warmup.argtypes[2] is C.POINTER(_abi.AfSeriesWarmup)
    assert lib.af_abi_version() == 7
    for name in ("check_warmup_batch", "series_warmup_sums", "series_warmup_statistics", "series_warmup_cut"):
        assert getattr(asyncflow_amd, name) is getattr(asyncflow_amd.results, name) and name in asyncflow_amd.__all__
    for listing in ((ROOT / "asyncflow_amd" / "build.py").read_text(), (ROOT / "asyncflow_amd" / "jit.py").read_text()):
        assert '"af_series_warmup.hpp"' in listing and '"af_wide.hpp"' in listing
    assert '#include "af_series_warmup.hpp"' in (ROOT / "asyncflow_amd" / "csrc" / "engine.hip").read_text()
    assert '#include "af_wide.hpp"' in (ROOT / "asyncflow_amd" / "csrc" / "af_series_warmup.hpp").read_text()
    assert "hip_runtime" not in (ROOT / "asyncflow_amd" / "csrc" / "af_wide.hpp").read_text()


def test_af_series_warmup_layout_matches_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "a host C compiler is needed for the layout probe"
    assert [name for name, _ in _abi.AfSeriesWarmup._fields_] == FIELDS  # noqa: SLF001
    src = tmp_path / "probe.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "asyncflow_hip.h"\n'
        'int main(void) { printf("%zu", sizeof(af_series_warmup_t));\n'
        + "".join(f'printf(" %zu", offsetof(af_series_warmup_t, {f}));\n' for f in FIELDS)
        + 'printf(" %d\\n", AF_MAX_SERIES_WARMUP_COLUMNS); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run([cc, "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    P = _abi.AfSeriesWarmup
    assert got == [C.sizeof(P), *(getattr(P, f).offset for f in FIELDS), _abi.MAX_SERIES_WARMUP_COLUMNS]
    body = re.search(r"typedef struct af_series_warmup \{(.*?)\} af_series_warmup_t;", (ROOT / "include" / "asyncflow_hip.h").read_text(), re.S)
    assert body and re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S)) == FIELDS


def test_series_warmup_entry_refuses_without_a_device(lib):
    from asyncflow_amd.engine import PLAN_ONLY, Engine, EngineUnavailableError

    eng = Engine(lower(lb_two_servers(horizon=20)), PLAN_ONLY)
    try:
        out = _abi.AfOutputs(0, None, 4, None, None)
        edges = (C.c_uint32 * 3)(0, 1, 2)
        cols = (C.c_uint32 * 1)(0)
        req = _abi.AfSeriesWarmup(4, 1, 2, None, edges, 1, cols, 5, None, None, None, None, None, None, 0.0, 0)
        call = lib.af_engine_summarize_series_warmup
        assert call(None, C.byref(out), C.byref(req)) == _abi.AF_ERR_INVALID
        assert call(eng._h, None, C.byref(req)) == _abi.AF_ERR_INVALID  # noqa: SLF001
        assert call(eng._h, C.byref(out), None) == _abi.AF_ERR_INVALID  # noqa: SLF001
        assert call(eng._h, C.byref(out), C.byref(req)) == _abi.AF_ERR_NO_DEVICE  # noqa: SLF001
        assert b"planning-only" in lib.af_last_error()
        kw = {"samples_ptr": 0, "tick_capacity": 4, "counts_ptr": 0, "batches_ptr": 0, "trunc_ptr": 0}
        with pytest.raises(EngineUnavailableError, match="planning-only"):
            eng.summarize_series_warmup(4, 1, [0, 2, 4], [0], 5, **kw)
        # a bad request never reaches the library
        for bad, what in (([0], "at least two"), ([0, 2, 2], "strictly increasing"), ([0.5, 2], "whole")):
            with pytest.raises(ValueError, match=what):
                eng.summarize_series_warmup(4, 1, bad, [0], 5, **kw)
        for bad in (0, -1, 2.5, True, 2 ** 32):
            with pytest.raises(ValueError, match="batch must be"):
                eng.summarize_series_warmup(4, 1, [0, 4], [0], bad, **kw)
        for bad in ([[0]], [0.5], [-1]):
            with pytest.raises(ValueError, match="series indices"):
                eng.summarize_series_warmup(4, 1, [0, 4], bad, 5, **kw)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------ the definition, worked by hand
def _plain(y):
    """MSER stated independently: every candidate's fraction, the smallest d of the smallest."""
    J = len(y)
    if J == 0:
        return 0, 0, 0, 0, 0
    cand = []
    for d in range(J // 2 + 1):
        tail = y[d:]
        m = len(tail)
        cand.append((Fraction(m * sum(v * v for v in tail) - sum(tail) ** 2, m ** 3), d))
    d = min(cand)[1]
    return d, sum(y[d:]), sum(v * v for v in y[d:]), sum(y), sum(v * v for v in y)


def _one(rows, batch, edges=None, n_edges=1):
    """series_warmup_sums of members given as lists of the values of ONE series."""
    mem = [np.array([r], dtype=np.uint32).reshape(1, -1) for r in rows]
    edges = [0, max(max((len(r) for r in rows), default=1), 1)] if edges is None else edges
    return series_warmup_sums(mem, edges, n_edges, batch)


def test_the_truncation_point_of_hand_made_sequences():
    assert warmup_truncation([]) == (0, 0, 0, 0, 0)
    assert warmup_truncation([7]) == (0, 7, 49, 7, 49)                              # J = 1: D = 0
    assert warmup_truncation([1, 5]) == (1, 5, 25, 6, 26)                           # J = 2: A(0) = 16 over 8, A(1) = 0
    assert warmup_truncation([5, 5]) == (0, 10, 50, 10, 50)                         # ... a tie at 0: the smaller d
    assert warmup_truncation([9, 1, 2]) == (1, 3, 5, 12, 86)                        # J = 3: D = 1; A(1) / 8 = 1 / 8 < A(0) / 27 = 114 / 27
    assert warmup_truncation([1, 2, 9]) == (0, 12, 86, 12, 86)                      # ... d = 2 is past D
    assert warmup_truncation([4] * 37)[0] == 0                                      # constant: A = 0 everywhere
    y = [5, 9, 1, 7] + [3] * 60
    assert warmup_truncation(y) == (4, 180, 540, sum(y), sum(v * v for v in y))     # the smallest d with A = 0
    rng = np.random.default_rng(4)
    for J in (1, 2, 3, 4, 5, 10, 63, 64, 65, 200):
        for hi in (2, 50, 2 ** 32, 2 ** 63):
            y = [int(v) for v in rng.integers(0, hi, J, dtype=np.uint64)]
            assert warmup_truncation(y) == _plain(y), (J, hi)
        y = [int(v) for v in rng.integers(0, 3, J)] + [1] * J                       # ties
        assert warmup_truncation(y) == _plain(y)


def test_cells_without_a_batch():
    short = _one([[1, 2, 3, 4]], 5)                                                 # a window shorter than B
    assert short["batches"].tolist() == [0] and short["trunc"].tolist() == [[0]] and all(short[k][0, 0] == 0 for k in WARMUP_SUMS)
    gone = _one([[1] * 20, []], 5, edges=[0, 20])                                   # a member with no row
    assert gone["batches"].tolist() == [0] and gone["s1_all"][0, 0] == 0
    nobody = series_warmup_sums([], [0, 10, 20], 1, 5, columns=[0, 0])              # a group without a member
    assert nobody["batches"].tolist() == [0, 0] and nobody["trunc"].shape == (2, 2) and not nobody["trunc"].any()
    past = _one([[2] * 12], 5, edges=[0, 10, 14, 30, 40])                           # edges past m_s = 12
    assert past["batches"].tolist() == [2, 0, 0, 0] and past["s1_all"][:, 0].tolist() == [20, 0, 0, 0]


def test_batches_windows_and_partial_batches():
    x = [5, 9, 1, 7] + [3] * 60
    assert _one([x], 1)["trunc"].tolist() == [[4]]
    got = _one([x + [1000, 1000]], 5, edges=[0, 66])                                # 13 batches; the 66th tick is in none
    y = [sum((x + [1000])[5 * j:5 * j + 5]) for j in range(13)]
    assert got["batches"].tolist() == [13] and (got["trunc"][0, 0], got["s1"][0, 0], got["s2"][0, 0], got["s1_all"][0, 0], got["s2_all"][0, 0]) == _plain(y)
    assert got["s1_all"][0, 0] == sum(x) + 1000                                     # the trailing partial batch is ignored
    # the batches of a window start at its edge, not at a multiple of B
    got = _one([list(range(40))], 4, edges=[3, 21, 40])
    assert got["batches"].tolist() == [4, 4] and got["s1_all"][:, 0].tolist() == [sum(range(3, 19)), sum(range(21, 37))]
    # one short member shortens the cell for all members
    got = _one([[1] * 40, [1] * 23, [1] * 31], 5, edges=[0, 40])
    assert got["batches"].tolist() == [4] and got["s1_all"][0, 0] == 3 * 20


def test_duplicate_columns_and_refused_columns():
    rng = np.random.default_rng(1)
    words = rng.integers(0, 9, (6, 50)).astype(np.uint32)                           # one edge; ready, io, ram of a server; ready, io of the next
    assert ram_columns(6, 1).tolist() == [False, False, False, True, False, False]
    got = series_warmup_sums(words, [0, 50], 1, 5, columns=[2, 0, 2])
    alone = series_warmup_sums(words, [0, 50], 1, 5, columns=[2])
    for k in ("trunc", *WARMUP_SUMS):
        assert got[k][0, 0] == got[k][0, 2] == alone[k][0, 0], k
    assert got["columns"].tolist() == [2, 0, 2]
    assert series_warmup_sums(words, [0, 50], 1, 5)["columns"].tolist() == [0, 1, 2, 4, 5]          # None: every integer series
    with pytest.raises(ValueError, match="ram_in_use"):
        series_warmup_sums(words, [0, 50], 1, 5, columns=[0, 3])
    with pytest.raises(ValueError, match="index below"):
        series_warmup_sums(words, [0, 50], 1, 5, columns=[6])
    for bad in (0, -3, 1.5, True, None, 2 ** 32):
        with pytest.raises(ValueError, match="batch must be"):
            check_warmup_batch(bad)
    assert check_warmup_batch(np.int64(5)) == 5 and check_warmup_batch(2 ** 32 - 1) == 2 ** 32 - 1


def test_a_group_is_its_summed_batch_series_not_a_combination_of_its_members():
    a = [9, 9, 9, 9, 1, 1, 1, 1, 1, 1, 1, 1]                                        # alone: d* = 4
    b = [1, 1, 1, 1, 1, 1, 1, 1, 9, 9, 9, 9]                                        # alone: d* = 0, the step is past D = 6
    c = [1, 1, 1, 1, 9, 9, 9, 9, 1, 1, 1, 1]                                        # alone: d* = 0
    alone = [int(_one([x], 1)["trunc"][0, 0]) for x in (a, b, c)]
    assert alone == [4, 0, 0]
    for members, d in (((a, b), 0), ((a, c), 0), ((b, c), 4)):                      # b + c is [2] * 4 + [10] * 8
        both = _one(list(members), 1)
        summed = _one([[x + y for x, y in zip(*members)]], 1)
        for k in ("batches", "trunc", *WARMUP_SUMS):
            assert both[k].tolist() == summed[k].tolist(), k
        assert both["trunc"].tolist() == [[d]]
    # b and c each start steady, their ensemble does not: no function of (0, 0) gives 4


# ------------------------------------------------------------------------------------ a golden file and a ramp
def _fixture(path: Path):
    z = np.load(path)
    plan = lower(json.loads(str(z["payload_json"])))
    words = np.ascontiguousarray(z["samples"]).view(np.uint32)
    counts = np.zeros(_abi.CNT_SLOTS, dtype=np.uint32)
    counts[_abi.CNT_TICKS] = words.shape[1]
    return plan, words, ScenarioResults(plan, counts, np.zeros((0, 2)), words)


def test_a_golden_run_against_a_plain_walk():
    plan, words, res = _fixture(ROOT / "tests" / "golden" / "lb2_rr_t600.npz")
    ticks = words.shape[1]
    got = res.get_series_warmup(5, tick_edges=[0, ticks])
    ints = np.nonzero(~ram_columns(plan.n_series, plan.n_edges))[0]
    assert got["columns"].tolist() == ints.tolist() and got["series"] == [series_names_of(plan)[j] for j in ints]
    J = ticks // 5
    assert got["batches"].tolist() == [J] and got["batch"] == 5
    for c, col in enumerate(ints):
        y = [int(v) for v in words[col, :J * 5].astype(np.int64).reshape(J, 5).sum(axis=1)]
        assert (got["trunc"][0, c], *(got[k][0, c] for k in WARMUP_SUMS)) == _plain(y), col
    assert got["converged"].all() and (got["trunc"] > 0).any() and (got["trunc"] == 0).any()      # no cell sits at the bound
    assert got["cut"].tolist() == [got["warmup_s"].max()]
    # windows: every window is its own sequence
    edges = tick_window_edges(4000, ticks)
    per = res.get_series_warmup(5, ticks_per_window=4000, series=[int(ints[2])])
    for w in range(len(edges) - 1):
        r0, r1 = int(edges[w]), min(int(edges[w + 1]), ticks)
        nb = (r1 - r0) // 5
        y = [int(v) for v in words[ints[2], r0:r0 + nb * 5].astype(np.int64).reshape(nb, 5).sum(axis=1)]
        assert per["batches"][w] == nb and (per["trunc"][w, 0], per["s1"][w, 0], per["s2"][w, 0]) == _plain(y)[:3]
    with pytest.raises(ValueError, match="ram_in_use"):
        res.get_series_warmup(series=["srv-1:ram_in_use"])
    with pytest.raises(ValueError, match="unknown series"):
        res.get_series_warmup(series=["srv-9:ready_queue_len"])
    with pytest.raises(RuntimeError, match="kept no sampled series"):
        ScenarioResults(plan, res.counts, np.zeros((0, 2)), None).get_series_warmup()


def test_a_ramp_followed_by_noise_is_cut_at_the_end_of_the_ramp():
    rng = np.random.default_rng(0)
    mem = [np.concatenate([np.arange(300) * 20 // 300, rng.poisson(20, 2000)]).astype(np.uint32)[None, :] for _ in range(8)]
    got = series_warmup_sums(mem, [0, 2300], 1, 5)
    st = series_warmup_statistics(got, 5, 8, 0.01, [0, 2300])
    y = [int(v) for v in sum(m[0, :2300].astype(np.int64).reshape(460, 5).sum(axis=1) for m in mem)]      # the summed batch series
    assert (got["trunc"][0, 0], *(got[k][0, 0] for k in WARMUP_SUMS)) == _plain(y)
    assert got["batches"].tolist() == [460] and st["warmup_tick"][0, 0] == 5 * _plain(y)[0] and 290 <= st["warmup_tick"][0, 0] <= 320 and st["converged"].all()
    assert abs(st["mean_steady"][0, 0] - 20.0) < 0.2 and st["mean_all"][0, 0] < 19.0 and st["mser_steady"][0, 0] < st["mser_all"][0, 0]


# ------------------------------------------------------------------------------------ the statistics
def test_statistics_are_the_rounded_fractions():
    rng = np.random.default_rng(9)
    G, W, Cn, B = 3, 4, 2, 7
    reps = np.array([5, 1, 0])
    edges = np.array([0, 100, 250, 400, 1000])
    period = 0.01
    sums = {"batches": rng.integers(1, 40, (G, W)), "trunc": np.zeros((G, W, Cn), dtype=np.int64)}
    sums["batches"][0, 1] = 0
    sums["batches"][2] = 0
    for k in WARMUP_SUMS:
        sums[k] = np.zeros((G, W, Cn), dtype=object)
    for idx in np.ndindex(G, W, Cn):
        J = int(sums["batches"][idx[:2]])
        y = [int(v) << 30 for v in rng.integers(0, 2 ** 33, J)]
        d, s1, s2, s1_all, s2_all = warmup_truncation(y)
        sums["trunc"][idx], sums["s1"][idx], sums["s2"][idx], sums["s1_all"][idx], sums["s2_all"][idx] = d, s1, s2, s1_all, s2_all
    st = series_warmup_statistics(sums, B, reps, period, edges)
    assert set(st) == {*WARMUP_STATISTICS, "warmup_tick", "converged"}
    for idx in np.ndindex(G, W, Cn):
        J, d, R = int(sums["batches"][idx[:2]]), int(sums["trunc"][idx]), int(reps[idx[0]])
        assert st["warmup_tick"][idx] == edges[idx[1]] + d * B and st["converged"][idx] == (d < J // 2)
        if J == 0 or R == 0:
            assert all(math.isnan(st[k][idx]) for k in WARMUP_STATISTICS) and not st["converged"][idx]
            continue
        m = J - d
        want = {"warmup_s": Fraction(int(st["warmup_tick"][idx])) * Fraction(period),
                "mean_all": Fraction(sums["s1_all"][idx], J * B * R), "mean_steady": Fraction(sums["s1"][idx], m * B * R),
                "mser_all": Fraction(J * sums["s2_all"][idx] - sums["s1_all"][idx] ** 2, J ** 3 * (B * R) ** 2),
                "mser_steady": Fraction(m * sums["s2"][idx] - sums["s1"][idx] ** 2, m ** 3 * (B * R) ** 2)}
        for k, v in want.items():
            assert st[k][idx] == float(v), (k, idx)
    # one scenario: [W, C] with a scalar number of replicas
    one = {k: v[0] for k, v in sums.items()}
    st1 = series_warmup_statistics(one, B, 5, period, edges)
    assert all(np.array_equal(st1[k], st[k][0], equal_nan=True) for k in st)
    with pytest.raises(ValueError, match="windows"):
        series_warmup_statistics(one, B, 5, period, edges[:-1])


def test_the_cut_is_the_latest_converged_series():
    summ = {"warmup_s": np.array([[[1.0, 3.5, 2.0], [0.0, 0.0, 0.0]], [[4.0, 1.0, 9.0], [np.nan, np.nan, np.nan]]]),
            "converged": np.array([[[True, True, True], [True, True, True]], [[True, True, False], [False, False, False]]])}
    cut = series_warmup_cut(summ)
    assert cut.shape == (2, 2) and cut[0].tolist() == [3.5, 0.0] and np.isnan(cut[1]).all()


# ------------------------------------------------------------------------------------ the batch layer on a host stand-in
def _pooled(words_of, ids, n_groups, b, n_edges, batch, cols):
    """The host definition of every group: series_warmup_sums of its members."""
    per = [series_warmup_sums([words_of[s] for s in np.nonzero(ids == g)[0]], b, n_edges, batch, cols) for g in range(n_groups)]
    return {k: np.stack([p[k] for p in per]) for k in ("batches", "trunc", *WARMUP_SUMS)}


class _HostBatch(BatchedResults):
    """A batch of host arrays whose warm-up call is the host definition, group by group."""

    def _series_warmup_call(self, cols, batch, b, ids, n_groups):
        self.calls.append(len(cols))
        return _pooled(self.host_words, ids, n_groups, b, self.plan.n_edges, batch, cols), 0.0, 0


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
    ramp = np.minimum(np.arange(ticks) // 3, 8)[None, None, :]                   # the first 24 ticks of 199
    batch.host_words = (ramp + rng.integers(0, 4, (n, plan.n_series, ticks))).astype(np.uint32)
    return batch, np.array([0, 1, 0, 1, -1, 1])


def _bits(a) -> bytes:
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def test_summary_and_bands_of_a_host_batch():
    batch, ids = _host_batch()
    names = batch.series_names()
    ints = np.nonzero(~ram_columns(len(names), batch.plan.n_edges))[0]
    edges = tick_window_edges(100, batch.plan.tick_count)
    W = len(edges) - 1
    pooled = batch.series_warmup_summary(5, ticks_per_window=100, by=ids)
    want = _pooled(batch.host_words, ids, 2, edges, batch.plan.n_edges, 5, ints)
    for k in ("batches", "trunc", *WARMUP_SUMS):
        assert pooled[k].tolist() == want[k].tolist(), k
    st = series_warmup_statistics(want, 5, np.array([2, 3]), batch.plan.sample_period, edges)
    for k in WARMUP_STATISTICS:
        assert _bits(pooled[k]) == _bits(st[k]) and pooled[k].shape == (2, W, len(ints)), k
    assert np.array_equal(pooled["converged"], st["converged"]) and np.array_equal(pooled["warmup_tick"], st["warmup_tick"])
    assert _bits(pooled["cut"]) == _bits(series_warmup_cut(st)) and pooled["cut"].shape == (2, W)
    assert pooled["series"] == [names[j] for j in ints] and pooled["replicas"].tolist() == [2, 3] and pooled["batch"] == 5
    assert np.array_equal(pooled["times"], edges[:-1] * batch.plan.sample_period) and pooled["calls"] == 1 and batch.calls == [len(ints)]
    assert (pooled["trunc"][:, 0] >= 4).all() and pooled["converged"][:, 0].any()                # the ramp of the first 24 ticks
    # by=None, the default: every replica in one group
    everyone = batch.series_warmup_summary(5, ticks_per_window=100)
    one = _pooled(batch.host_words, np.zeros(6, dtype=np.int64), 1, edges, batch.plan.n_edges, 5, ints)
    for k in ("batches", "trunc", *WARMUP_SUMS):
        assert everyone[k].tolist() == one[k].tolist(), k
    st6 = series_warmup_statistics(one, 5, 6, batch.plan.sample_period, edges)
    assert everyone["replicas"].tolist() == [6] and all(_bits(everyone[k]) == _bits(st6[k]) for k in WARMUP_STATISTICS)
    assert everyone["trunc"].shape == (1, W, len(ints)) and _bits(everyone["cut"]) == _bits(series_warmup_cut(st6))
    batch.calls.clear()
    # no window given: one window over the whole run; a selection by name and index, a duplicate
    whole = batch.series_warmup_summary(by=ids, series=["srv-1:ready_queue_len", int(ints[0]), "srv-1:ready_queue_len"])
    assert whole["tick_edges"].tolist() == [0, batch.plan.tick_count] and whole["trunc"].shape == (2, 1, 3)
    assert whole["trunc"][:, :, 0].tolist() == whole["trunc"][:, :, 2].tolist() and whole["columns"][1] == ints[0]
    # bands over the replicas
    per = batch.series_warmup_summary(5, ticks_per_window=100, by="scenario")
    bands = batch.series_warmup_bands(5, ticks_per_window=100, by=ids)
    assert bands["mean"].shape == bands["q_lo"].shape == bands["pooled"].shape == bands["converged_share"].shape == (2, W, len(ints))
    assert _bits(bands["pooled"]) == _bits(pooled["warmup_s"]) and np.array_equal(bands["pooled_converged"], pooled["converged"])
    for g in range(2):
        np.testing.assert_allclose(bands["mean"][g], per["warmup_s"][ids == g].mean(axis=0), rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(bands["q_hi"][g], np.quantile(per["warmup_s"][ids == g], 0.95, axis=0), rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(bands["converged_share"][g], per["converged"][ids == g].mean(axis=0), rtol=1e-15)
    assert bands["replicas"].tolist() == [2, 3] and (bands["n"] == np.array([2, 3])[:, None]).all()


def test_more_than_64_columns_are_split_into_calls():
    batch, ids = _host_batch()
    ints = np.nonzero(~ram_columns(batch.plan.n_series, batch.plan.n_edges))[0]
    sel = [int(ints[i % len(ints)]) for i in range(150)]
    out = batch.series_warmup_summary(4, ticks_per_window=70, by=ids, series=sel)
    assert batch.calls == [64, 64, 22] and out["calls"] == 3 and out["trunc"].shape[2] == 150
    want = _pooled(batch.host_words, ids, 2, tick_window_edges(70, batch.plan.tick_count), batch.plan.n_edges, 4, np.array(sel))
    for k in ("batches", "trunc", *WARMUP_SUMS):
        assert out[k].tolist() == want[k].tolist(), k


@pytest.mark.parametrize("ext", ["npz", "parquet"])
def test_on_disk_round_trip(tmp_path, ext):
    if ext == "parquet":
        pytest.importorskip("pyarrow")
    batch, ids = _host_batch()
    sel = ["srv-1:ready_queue_len", "srv-2:event_loop_io_sleep"]
    path = str(tmp_path / f"series_warmup.{ext}")
    written = batch.save_series_warmup_summary(path, ids, batch=5, ticks_per_window=60, series=sel)
    back = load_summary(path)
    assert set(back) == set(written)
    for k, v in written.items():
        assert np.array_equal(np.asarray(back[k], dtype=v.dtype), v, equal_nan=True), k
    W = -(-batch.plan.tick_count // 60)
    want = batch.series_warmup_summary(5, ticks_per_window=60, by=ids, series=sel)
    bands = batch.series_warmup_bands(5, ticks_per_window=60, by=ids, series=sel)
    per_series = ("tick", "s", "converged", "mean_all", "mean_steady", "q05", "q95", "converged_share")
    assert set(back) == {"replicas", "series_warmup_batches", "series_warmup_cut", "series_warmup_tick_edges", "series_warmup_times",
                         "series_warmup_batch", *(f"series_warmup_{k}:{name}" for k in per_series for name in sel)}
    assert back["replicas"].tolist() == [2, 3] and back["series_warmup_batch"].tolist() == [5.0]
    assert np.array_equal(back["series_warmup_batches"], want["batches"]) and _bits(back["series_warmup_cut"]) == _bits(want["cut"])
    for c, name in enumerate(sel):
        assert back[f"series_warmup_s:{name}"].shape == (2, W)
        assert np.array_equal(back[f"series_warmup_tick:{name}"], want["warmup_tick"][:, :, c])
        assert _bits(back[f"series_warmup_s:{name}"]) == _bits(want["warmup_s"][:, :, c])
        assert np.array_equal(back[f"series_warmup_converged:{name}"], want["converged"][:, :, c].astype(np.int64))
        assert _bits(back[f"series_warmup_mean_steady:{name}"]) == _bits(want["mean_steady"][:, :, c])
        assert _bits(back[f"series_warmup_q05:{name}"]) == _bits(bands["q_lo"][:, :, c]) and _bits(back[f"series_warmup_q95:{name}"]) == _bits(bands["q_hi"][:, :, c])
        assert _bits(back[f"series_warmup_converged_share:{name}"]) == _bits(bands["converged_share"][:, :, c])
    assert np.array_equal(back["series_warmup_tick_edges"], want["tick_edges"]) and np.array_equal(back["series_warmup_times"], want["times"])


def test_refusals_of_the_batch_layer():
    plan = lower(lb_two_servers(horizon=10))
    batch = BatchedResults.__new__(BatchedResults)
    batch.plan = plan
    batch._samples_t = None  # noqa: SLF001
    for call in (batch.series_warmup_summary, batch.series_warmup_bands):
        with pytest.raises(RuntimeError, match="kept no sampled series"):
            call(5)
    with pytest.raises(RuntimeError, match="kept no sampled series"):
        batch.save_series_warmup_summary("nowhere.npz", ticks_per_window=10)
    batch._samples_t = object()  # noqa: SLF001  (the checks below come before the device is touched)
    with pytest.raises(ValueError, match="ram_in_use"):
        batch.series_warmup_summary(series=["srv-1:ready_queue_len", "srv-1:ram_in_use"])
    with pytest.raises(ValueError, match="unknown series"):
        batch.series_warmup_summary(series="srv-9:ready_queue_len")
    with pytest.raises(ValueError, match="no series name or index"):
        batch.series_warmup_summary(series=[plan.n_series])
    with pytest.raises(ValueError, match="selects no series"):
        batch.series_warmup_summary(series=[])
    for bad in (0, 2.5, -5, None):
        with pytest.raises(ValueError, match="batch must be"):
            batch.series_warmup_summary(bad)
    with pytest.raises(ValueError, match="one of"):
        batch.series_warmup_summary(5, 1.0, ticks_per_window=10)
    with pytest.raises(ValueError, match="by must be"):
        batch.series_warmup_summary(5, ticks_per_window=10, by="point")


def test_sharded_results_refuse_the_warmup_analyzer():
    sh = ShardedResults.__new__(ShardedResults)
    for call in (sh.series_warmup_summary, sh.series_warmup_bands, sh.save_series_warmup_summary):
        with pytest.raises(NotImplementedError, match="several devices"):
            call({})
