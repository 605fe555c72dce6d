"""Paired latency differences under common seeds, CPU side: the host definition (`results.latency_pairs`,
`latency_pair_cells`) that `af_engine_summarize_pairs` is held to word for word against a brute-force dictionary join on synthetic
rows and on two CPU-oracle runs that share their seed; the self-pair and swapped-pair identities; the fixed-order sum against
`math.fsum`; the histogram identity; quantile brackets and the merge; `expand_grid(common_seeds=True)` and `Sweep.pairs`; the
refusals of the Python surface; and the C entry point with its struct."""

from __future__ import annotations

import copy
import ctypes as C
import math
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import asyncflow_amd
from asyncflow_amd import _abi, expand_grid
from asyncflow_amd import build as af_build
from asyncflow_amd.plan import lower
from asyncflow_amd.results import (PAIR_NONE, BatchedResults, ShardedResults, arrival_times, latency_bin_index, latency_pair_cells, latency_pairs,
                                   paired_delta_quantiles, paired_fixed_sum, paired_merge)
from oracle import oracle_lib as ol
from oracle.rng_adapter import GeneratorRNG
from oracle.scenarios import lb_two_servers
from tests import paired_cases as pc

ROOT = Path(__file__).resolve().parent.parent
COUNTS = ("both", "only_a", "only_b", "neither", "nan")


def _brute(clock_a, clock_b, times, edges):
    """The join through a dictionary {start bits: smallest row}, and the deltas per window by a mask on every arrival."""
    A = times[np.isfinite(times)]
    rows = []
    for ck in (clock_a, clock_b):
        first: dict[int, int] = {}
        for i, s in enumerate(np.ascontiguousarray(ck[:, 0]).view(np.uint64).tolist()):
            first.setdefault(s, i)
        seen: set[int] = set()
        row = []
        for word in A.view(np.uint64).tolist():                       # of equal arrivals only the first can be claimed
            row.append(first[word] if word in first and word not in seen else PAIR_NONE)
            seen.add(word)
        rows.append(np.array(row, dtype=np.uint32).reshape(-1))
    ra, rb = rows
    both = (ra != PAIR_NONE) & (rb != PAIR_NONE)
    d = np.full(A.shape[0], np.nan)
    with np.errstate(invalid="ignore"):
        d[both] = (clock_b[rb[both], 1] - clock_b[rb[both], 0]) - (clock_a[ra[both], 1] - clock_a[ra[both], 0])
    if edges is None:
        win = np.zeros(A.shape[0], dtype=np.int64)
    else:
        win = np.array([next((w for w in range(len(edges) - 1) if edges[w] < t <= edges[w + 1]), -1) for t in A], dtype=np.int64).reshape(-1)
    return ra, rb, both, d, win


def _check_against_brute(clock_a, clock_b, times, edges, **kw):
    got = latency_pairs(clock_a, clock_b, times, edges, **kw)
    ra, rb, both, d, win = _brute(clock_a, clock_b, times, edges)
    assert np.array_equal(got["row_a"], ra) and np.array_equal(got["row_b"], rb)
    assert got["unmatched_a"] == clock_a.shape[0] - np.count_nonzero(ra != PAIR_NONE) and got["unmatched_b"] == clock_b.shape[0] - np.count_nonzero(rb != PAIR_NONE)
    assert pc.same_words(got["d"], d)
    th = np.zeros(0) if kw.get("thresholds") is None else np.asarray(kw["thresholds"])
    binning = (kw.get("sub_bits", 5), kw.get("min_exp", -20), kw.get("octaves", 32))
    for w in range(got["both"].shape[0]):
        here = win == w
        x = d[here & both]
        x = x[~np.isnan(x)]
        assert got["both"][w] == np.count_nonzero(here & both) and got["nan"][w] == np.count_nonzero(here & both) - x.shape[0]
        assert got["only_a"][w] == np.count_nonzero(here & (ra != PAIR_NONE) & (rb == PAIR_NONE))
        assert got["only_b"][w] == np.count_nonzero(here & (ra == PAIR_NONE) & (rb != PAIR_NONE))
        assert got["neither"][w] == np.count_nonzero(here & (ra == PAIR_NONE) & (rb == PAIR_NONE))
        assert (got["slower"][w], got["faster"][w], got["equal"][w]) == (np.count_nonzero(x > 0), np.count_nonzero(x < 0), np.count_nonzero(x == 0))
        assert got["above"][w].tolist() == [np.count_nonzero(x > t) for t in th]
        if x.shape[0]:
            assert got["min_d"][w] == x.min() and got["max_d"][w] == x.max()
            # THE BOUND of any summation order of n terms: |s - exact| <= (n - 1) 2^-53 sum|x|
            if np.isfinite(x).all():                                  # (an infinite delta has no exact sum to compare with)
                assert abs(got["sum_d"][w] - math.fsum(x)) <= (x.shape[0] - 1) * 2.0 ** -53 * math.fsum(np.abs(x))
        else:
            assert np.isposinf(got["min_d"][w]) and np.isneginf(got["max_d"][w]) and got["sum_d"][w] == 0.0
        for side, v in (("pos", x[x > 0]), ("neg", -x[x < 0])):
            b = latency_bin_index(v, *binning)
            assert np.array_equal(got[f"hist_{side}"][w], np.bincount(b[b >= 0], minlength=got["hist_pos"].shape[1]))
            assert (got[f"under_{side}"][w], got[f"over_{side}"][w]) == (np.count_nonzero(b == -1), np.count_nonzero(b == -2))
        ident = int(got["equal"][w]) + int(got["nan"][w]) + sum(int(got[k][w]) for k in ("under_pos", "under_neg", "over_pos", "over_neg")) \
            + int(got["hist_pos"][w].sum()) + int(got["hist_neg"][w].sum())
        assert ident == int(got["both"][w])
    return got


def test_the_definition_equals_a_dictionary_join_on_synthetic_rows():
    rng = np.random.default_rng(1)
    k = 0
    for m in pc.ROWS:
        times = pc.arrival_row(rng, m, m + 7, duplicates=3)
        for rows_a, rows_b in ((m, m), (max(m - 5, 0), m), (m, 0), (m + 9, m // 2)):
            a, b = pc.side_rows(rng, times, rows_a, pc.ORDERS[k % 3]), pc.side_rows(rng, times, rows_b, pc.ORDERS[(k + 1) % 3])
            for n_win in (0, 1, 7, max(m, 2) + 3):
                _check_against_brute(a, b, times, pc.uneven_edges(n_win, times), thresholds=pc.signed_thresholds((0, 5, 64)[k % 3]),
                                     **dict(zip(("sub_bits", "min_exp", "octaves"), ((0, -3, 1), (5, -20, 32), (8, -10, 16))[k % 3])))
                k += 1


def test_the_fixed_order_sum_is_the_stated_order_and_close_to_fsum():
    rng = np.random.default_rng(2)
    for n, j0 in ((1, 0), (64, 0), (65, 3), (300, 17), (1000, 64), (129, 127)):
        v = np.zeros(j0 + n)
        v[j0:] = rng.normal(0.0, 1.0, n) * 10.0 ** rng.integers(-6, 6, n)
        mask = rng.random(j0 + n) < 0.8
        part = [0.0] * 64
        for j in range(j0, j0 + n):                                   # lane j mod 64 adds in ascending j from +0.0
            if mask[j]:
                part[j % 64] += float(v[j])
        h = 32
        while h:
            for lane in range(h):
                part[lane] += part[lane + h]
            h //= 2
        got = paired_fixed_sum(v, mask, j0, j0 + n)
        assert got == part[0]
        x = v[j0:][mask[j0:]]
        # the standard bound for any summation order of n terms: (n - 1) 2^-53 sum|x|
        assert abs(got - math.fsum(x)) <= max(x.shape[0] - 1, 0) * 2.0 ** -53 * math.fsum(np.abs(x))
    assert paired_fixed_sum(np.ones(10), np.ones(10, dtype=bool), 4, 4) == 0.0
    assert math.copysign(1.0, paired_fixed_sum(np.full(70, -0.0), np.ones(70, dtype=bool), 0, 70)) == 1.0     # from +0.0: never -0.0


def _oracle_runs():
    """Two CPU-oracle runs of one payload with the same seed and one changed edge latency, and their arrival row."""
    base = lb_two_servers(horizon=20)
    slow = copy.deepcopy(base)
    for e in slow["topology_graph"]["edges"]:
        if e["id"] == "lb-srv1":
            e["latency"]["mean"] = 0.02
    runs = []
    for payload in (base, slow):
        plan = lower(payload)
        runs.append(ol.simulate(plan, 42).clock)
    times, flags = arrival_times(GeneratorRNG(42), plan.gen_users_dist, plan.gen_users_mean, plan.gen_users_sigma, plan.gen_rpm_mean,
                                 plan.gen_window_s, plan.total_time, plan.clock_capacity())
    assert flags == 0
    return runs[0], runs[1], times


def test_two_oracle_runs_that_share_their_seed_pair_request_by_request():
    a, b, times = _oracle_runs()
    A = times[np.isfinite(times)]
    for ck in (a, b):
        assert ck.shape[0] > 500 and np.isin(np.ascontiguousarray(ck[:, 0]).view(np.uint64), A.view(np.uint64)).all()   # every start is in the row
    edges, th = np.arange(0.0, 21.0, 5.0), [-0.01, 0.0, 0.01, 0.2]
    got = _check_against_brute(a, b, times, edges, thresholds=th)
    assert got["unmatched_a"] == 0 and got["unmatched_b"] == 0
    assert int(got["both"].sum()) > 500 and int(got["slower"].sum()) > int(got["faster"].sum()) and got["neither"][-1] > 0
    _check_against_brute(a, b, times, None)
    # a run with itself: +0.0 everywhere
    own = latency_pairs(a, a, times, edges, thresholds=th)
    assert np.array_equal(own["equal"], own["both"]) and (own["sum_d"].view(np.uint64) == 0).all() and (own["only_a"] == 0).all() and (own["only_b"] == 0).all()
    assert (own["d"][own["state"] == 3].view(np.uint64) == 0).all() and (own["hist_pos"] == 0).all() and (own["hist_neg"] == 0).all()
    # the swapped pair mirrors every word
    back = latency_pairs(b, a, times, edges, thresholds=th)
    assert np.array_equal((-got["sum_d"]).view(np.uint64), back["sum_d"].view(np.uint64)) and (got["sum_d"] != 0).all()
    assert np.array_equal(got["hist_pos"], back["hist_neg"]) and np.array_equal(got["hist_neg"], back["hist_pos"])
    assert np.array_equal(got["slower"], back["faster"]) and np.array_equal(got["faster"], back["slower"]) and np.array_equal(got["only_a"], back["only_b"])
    assert np.array_equal((-got["max_d"]).view(np.uint64), back["min_d"].view(np.uint64)) and np.array_equal(got["under_pos"], back["under_neg"])


def test_cells_quantile_brackets_and_the_merge():
    rng = np.random.default_rng(3)
    times = pc.arrival_row(rng, 300, 300)
    edges, th = pc.uneven_edges(7, times), pc.signed_thresholds(5)
    pairs = [latency_pairs(pc.side_rows(rng, times, 280, "shuffle"), pc.side_rows(rng, times, 290, "arrival"), times, edges, thresholds=th) for _ in range(6)]
    groups = [0, 2, 2, -1, 0, 2]
    cells = latency_pair_cells(pairs, groups, 4)
    assert cells["replicas"].tolist() == [2, 0, 3, 0] and (cells["both"][1] == 0).all() and np.isposinf(cells["min_d"][3]).all() and np.isneginf(cells["max_d"][1]).all()
    for g, members in ((0, (0, 4)), (2, (1, 2, 5))):
        for key in (*COUNTS, "slower", "faster", "equal", "above", "hist_pos", "hist_neg", "under_pos", "over_neg"):
            assert np.array_equal(cells[key][g], sum(pairs[p][key].astype(np.uint64) for p in members)), key
        assert np.array_equal(cells["min_d"][g], np.min([pairs[p]["min_d"] for p in members], axis=0))
        assert np.array_equal(cells["max_d"][g], np.max([pairs[p]["max_d"] for p in members], axis=0))
    # the order of the pairs does not matter
    order = [5, 3, 0, 2, 4, 1]
    again = latency_pair_cells([pairs[p] for p in order], [groups[p] for p in order], 4)
    for key in (*COUNTS, "above", "hist_pos", "hist_neg", "min_d", "max_d"):
        assert np.array_equal(cells[key], again[key]), key
    # -0.0 is below +0.0 in min / max
    z = latency_pairs(np.array([[1.0, 2.0], [3.0, 4.0]]), np.array([[1.0, 2.0], [3.0, 4.0]]), np.array([1.0, 3.0]))
    n = dict(z, min_d=np.array([-0.0]), max_d=np.array([-0.0]))
    both_ways = latency_pair_cells([z, n], None, 1), latency_pair_cells([n, z], None, 1)
    for c in both_ways:
        assert math.copysign(1.0, c["min_d"][0, 0]) == -1.0 and math.copysign(1.0, c["max_d"][0, 0]) == 1.0
    # the merge of two halves is one call
    merged = paired_merge(latency_pair_cells(pairs[:3], groups[:3], 4), latency_pair_cells(pairs[3:], groups[3:], 4))
    for key in (*COUNTS, "slower", "faster", "equal", "above", "hist_pos", "hist_neg", "under_pos", "under_neg", "over_pos", "over_neg", "replicas"):
        assert np.array_equal(merged[key], cells[key].astype(np.int64)), key
    assert np.array_equal(merged["min_d"], cells["min_d"]) and np.array_equal(merged["max_d"], cells["max_d"])
    with pytest.raises(ValueError, match="edges"):
        paired_merge(cells, latency_pair_cells([latency_pairs(np.zeros((0, 2)), np.zeros((0, 2)), times, [0.0, 1.0], thresholds=th)], None, 4))
    # brackets of the quantiles of d
    levels = [0.0, 0.01, 0.25, 0.5, 0.75, 0.99, 1.0]
    br = paired_delta_quantiles(cells, levels)
    for g, members in ((0, (0, 4)), (2, (1, 2, 5))):
        for w in range(7):
            d = np.concatenate([pairs[p]["d"][pairs[p]["bounds"][w]: pairs[p]["bounds"][w + 1]] for p in members])
            d = d[~np.isnan(d)]
            if d.shape[0] == 0:
                assert np.isnan(br["lo"][g, w]).all()
                continue
            exact = np.quantile(d, levels, method="lower")
            fin = np.isfinite(exact)
            assert (br["lo"][g, w] <= exact).all() and (exact[fin] < br["hi"][g, w][fin]).all(), (g, w)
            inside = (np.abs(exact) > 2.0 ** -20) & fin
            assert (np.abs(br["hi"][g, w][inside] - br["lo"][g, w][inside]) <= np.abs(exact[inside]) * 2.0 ** -5 * 1.001).all()
    assert np.isnan(br["lo"][1]).all() and br["lo"].shape == (4, 7, 7)
    with pytest.raises(ValueError, match="levels"):
        paired_delta_quantiles(cells, [1.5])


def test_common_seeds_and_pairs_of_a_grid_with_and_without_order_by_load():
    users, edge = "rqs_input.avg_active_users.mean", "topology_graph.edges[lb-srv1].latency.mean"
    plain = expand_grid({users: [20.0, 60.0], edge: [0.002, 0.02]}, replicas=3, seed_base=100)
    assert plain.seeds.tolist() == list(range(100, 112))                                  # the default stays as it is
    for order in (None, users):
        grid = expand_grid({users: [20.0, 60.0, 40.0], edge: [0.002, 0.02]}, replicas=3, seed_base=100, common_seeds=True, order_by_load=order)
        assert np.array_equal(grid.seeds, 100 + grid.replica.astype(np.uint64))
        p = grid.pairs(edge, 0.002, 0.02)
        assert p["shape"] == (3,) and p["a"].shape == (9,) and p["by"].tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2]
        assert (grid.columns[edge][p["a"]] == 0.002).all() and (grid.columns[edge][p["b"]] == 0.02).all()
        assert np.array_equal(grid.columns[users][p["a"]], grid.columns[users][p["b"]]) and np.array_equal(grid.seeds[p["a"]], grid.seeds[p["b"]])
        assert np.array_equal(grid.replica[p["a"]], grid.replica[p["b"]]) and np.array_equal(grid.columns[users][p["a"]], np.repeat([20.0, 60.0, 40.0], 3))
        q = grid.pairs(users, 60.0, 20.0)
        assert q["shape"] == (2,) and (grid.columns[users][q["a"]] == 60.0).all() and (grid.columns[users][q["b"]] == 20.0).all()
        assert np.array_equal(grid.columns[edge][q["a"]], grid.columns[edge][q["b"]]) and q["by"].tolist() == [0, 0, 0, 1, 1, 1]
        with pytest.raises(ValueError, match="not an axis"):
            grid.pairs("no.such.axis", 1.0, 2.0)
        with pytest.raises(ValueError, match="not exactly one value"):
            grid.pairs(edge, 0.002, 0.5)


def test_paired_summary_refuses_pairs_that_were_not_sent_the_same_requests():
    users, edge = "rqs_input.avg_active_users.mean", "topology_graph.edges[lb-srv1].latency.mean"
    plan = lower(lb_two_servers(horizon=20))
    n = 8

    def batch(seeds, overrides):
        import torch

        return BatchedResults(plan, np.asarray(seeds, dtype=np.uint64), torch.zeros((n, _abi.CNT_SLOTS), dtype=torch.int32),
                              torch.zeros((n, 4, 2), dtype=torch.float64), None, _abi.AfStats(), 0.0, overrides)

    own_seeds = batch(np.arange(n), {edge: np.tile([0.002, 0.02], 4)})
    with pytest.raises(ValueError, match=r"pair 0 \(scenarios 0 and 1\).*seeds differ"):
        own_seeds.paired_summary([0, 2], [1, 3])
    shared = batch(np.arange(n) // 2, {edge: np.tile([0.002, 0.02], 4), users: np.array([20.0, 20.0, 20.0, 30.0, 20.0, 20.0, 20.0, 20.0])})
    with pytest.raises(ValueError, match=r"pair 1 \(scenarios 2 and 3\).*avg_active_users.mean differ"):
        shared.paired_summary([0, 2, 4], [1, 3, 5])
    for bad_a, bad_b in (([0, 1], [1]), ([], []), ([0], [8]), ([-1], [0])):
        with pytest.raises(ValueError, match="index vectors"):
            shared.paired_summary(bad_a, bad_b)
    for method in ("paired_summary", "paired_bands", "save_paired_summary"):
        with pytest.raises(NotImplementedError, match="several devices"):
            getattr(ShardedResults([shared], [np.arange(n)], 0.0), method)([0], [1])
    for bad in (dict(thresholds=[0.0] * 65), dict(thresholds=[float("inf")]), dict(octaves=200), dict(edges=[1.0, 1.0])):
        with pytest.raises(ValueError):
            latency_pairs(np.zeros((0, 2)), np.zeros((0, 2)), np.zeros(0), **bad)


# ---- the ABI ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    af_build.build()
    from asyncflow_amd.engine import load_library

    return load_library()


def test_header_declares_and_library_exports_the_entry(lib):
    header = (ROOT / "include" / "asyncflow_hip.h").read_text()
    assert re.search(r"int\s+af_engine_summarize_pairs\s*\(\s*af_engine_t\s*\*", header)
    assert re.search(r"#define\s+AF_MAX_PAIR_THRESHOLDS\s+64\b", header) and re.search(r"#define\s+AF_PAIR_NONE\s+0xFFFFFFFFu", header)
    assert re.search(r"#define\s+AF_ABI_VERSION\s+7\b", header)
    assert "af_engine_summarize_pairs" in _abi.EXPORTED_SYMBOLS
    assert lib.af_engine_summarize_pairs.argtypes[2] is C.POINTER(_abi.AfPairs)
    assert lib.af_abi_version() == 7 and _abi.MAX_PAIR_THRESHOLDS == 64 and _abi.PAIR_NONE == PAIR_NONE
    for src in ("build.py", "jit.py"):
        assert '"af_paired.hpp"' in (ROOT / "asyncflow_amd" / src).read_text()
    for name in ("latency_pairs", "latency_pair_cells", "paired_delta_quantiles", "paired_merge", "paired_fixed_sum"):
        assert name in asyncflow_amd.__all__ and getattr(asyncflow_amd, name) is getattr(asyncflow_amd.results, name)


def test_af_pairs_layout_matches_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "a host C compiler is needed for the layout probe"
    fields = [name for name, _ in _abi.AfPairs._fields_]  # noqa: SLF001
    assert fields == ["n_scenarios", "n_pairs", "n_groups", "n_windows", "pair_a", "pair_b", "group", "edges", "times", "time_row", "n_time_rows",
                      "draw_capacity", "thresholds", "n_thresholds", "sub_bits", "min_exp", "octaves", "pair_counts", "pair_sums", "unmatched",
                      "cell_counts", "above", "extremes", "hist", "tails", "row_a", "row_b", "elapsed_ms", "scratch_bytes"]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "asyncflow_hip.h"\n'
                   'int main(void) { printf("%zu", sizeof(af_pairs_t));\n'
                   + "".join(f'printf(" %zu", offsetof(af_pairs_t, {f}));\n' for f in fields)
                   + 'printf(" %zu %zu\\n", sizeof(af_latency_histogram_t), sizeof(af_outputs_t)); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run([cc, "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    P = _abi.AfPairs
    assert P.min_exp.size == 4 and got == [C.sizeof(P), *(getattr(P, f).offset for f in fields), C.sizeof(_abi.AfLatencyHistogram), C.sizeof(_abi.AfOutputs)]


def test_entry_refuses_without_a_device(lib):
    from asyncflow_amd.engine import PLAN_ONLY, Engine, EngineUnavailableError

    eng = Engine(lower(lb_two_servers(horizon=20)), PLAN_ONLY)
    try:
        out = _abi.AfOutputs(4, None, 8, None, None)
        req = _abi.AfPairs(4, 2, 1, 0)
        entry = lib.af_engine_summarize_pairs
        assert entry(None, C.byref(out), C.byref(req)) == _abi.AF_ERR_INVALID
        assert entry(eng._h, None, C.byref(req)) == _abi.AF_ERR_INVALID  # noqa: SLF001
        assert entry(eng._h, C.byref(out), None) == _abi.AF_ERR_INVALID  # noqa: SLF001
        assert entry(eng._h, C.byref(out), C.byref(req)) == _abi.AF_ERR_NO_DEVICE  # noqa: SLF001
        assert b"planning-only" in lib.af_last_error()
        kw = dict(pair_a_ptr=0, pair_b_ptr=0, times_ptr=0, time_row_ptr=0, n_time_rows=1, draw_capacity=8, clock_ptr=0, clock_capacity=4, counts_ptr=0,
                  pair_counts_ptr=0, pair_sums_ptr=0, unmatched_ptr=0, cell_counts_ptr=0, extremes_ptr=0, hist_ptr=0, tails_ptr=0)
        with pytest.raises(EngineUnavailableError, match="planning-only"):
            eng.summarize_pairs(4, 2, 1, **kw)
        for bad in (dict(sub_bits=9), dict(octaves=0), dict(min_exp=1000, octaves=24), dict(thresholds=[0.0] * 65), dict(thresholds=[float("nan")]),
                    dict(edges=[1.0, 0.0])):
            with pytest.raises(ValueError):
                eng.summarize_pairs(4, 2, 1, **bad, **kw)
    finally:
        eng.close()
