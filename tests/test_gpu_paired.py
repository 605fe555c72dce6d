"""Paired latency differences on the MI355X (af_engine_summarize_pairs, asyncflow_amd/csrc/af_paired.hpp): every output word
against the host definition (results.latency_pairs per pair, results.latency_pair_cells per group).  Synthetic arrival rows and
clocks through the C ABI: row lengths around the wave on both sides independently, a side without rows and one whose counts exceed
the clock capacity, completion in arrival order, reversed and shuffled, starts beside arrivals and hostile rows, duplicated
arrivals, window counts from none to one above what the kernel keeps in LDS, one and 130 pairs in one and in many chunks, a
baseline shared by every pair, group arrangements, no and 64 thresholds, three binnings, the join present and absent, every
refusal, and the independence of the launch.  Every output of a call lies in ONE buffer with sentinel words on both sides of each.
A run with common seeds goes through the Python API."""

from __future__ import annotations

import ctypes as C
import os
import re
from pathlib import Path

import numpy as np
import pytest

from asyncflow_amd import _abi
from asyncflow_amd.plan import lower
from asyncflow_amd.results import PAIR_NONE, latency_pair_cells, latency_pairs, load_summary, paired_delta_quantiles, paired_merge
from oracle.scenarios import lb_two_servers, single_server
from tests import paired_cases as pc

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "asyncflow_amd" / "csrc" / "af_paired.hpp").read_text()
LDS_WINDOWS = int(re.search(r"constexpr\s+uint32_t\s+kLdsPairWindows\s*=\s*(\d+)\s*;", HEADER).group(1))
MATCH_ROWS = int(re.search(r"constexpr\s+uint32_t\s+kMatchRows\s*=\s*(\d+)\s*;", HEADER).group(1))
BINNINGS = [(0, -3, 1), (5, -20, 32), (8, -10, 16)]
SENTINEL = 0x5A5A5A5A
GUARD = 16
PAIR_KEYS = ("both", "only_a", "only_b", "neither", "nan")
CELL_KEYS = (*PAIR_KEYS, "slower", "faster", "equal")
TAIL_KEYS = ("under_pos", "under_neg", "over_pos", "over_neg")
OUTPUTS = ("pair_counts", "pair_sums", "unmatched", "cell_counts", "above", "extremes", "hist", "tails", "row_a", "row_b")


@pytest.fixture(scope="module")
def eng():
    from asyncflow_amd.engine import Engine

    e = Engine(lower(single_server(horizon=50)), 0)
    yield e
    e.close()


class _Batch:
    """Arrival rows, clocks and counts on the device, and the pairs over them.  Rows behind a scenario's stored ones hold
    requests that would match if they were read."""

    def __init__(self, times, clocks, pair_a, pair_b, time_row, cap=None, counts_extra=0):
        import torch

        self.times = [np.asarray(t, dtype=np.float64) for t in times]
        self.n_draw = int(self.times[0].shape[0])
        self.n = len(clocks)
        self.cap = cap or max(max((len(x) for x in clocks), default=1), 1) + 3
        clock = np.empty((self.n, self.cap, 2))
        some = self.times[0][np.isfinite(self.times[0])]
        clock[:, :, 0], clock[:, :, 1] = (some[0] if some.shape[0] else 1.0), 99.0
        counts = np.zeros((self.n, _abi.CNT_SLOTS), dtype=np.uint32)
        self.stored = []
        for i, rows in enumerate(clocks):
            rows = np.asarray(rows, dtype=np.float64).reshape(-1, 2)
            counts[i, _abi.CNT_COMPLETED] = rows.shape[0] + counts_extra
            keep = rows[: self.cap]
            clock[i, : keep.shape[0]] = keep
            self.stored.append(clock[i, : min(rows.shape[0] + counts_extra, self.cap)].copy())
        self.pair_a, self.pair_b, self.time_row = (np.asarray(v, dtype=np.int64) for v in (pair_a, pair_b, time_row))
        self.P = int(self.pair_a.shape[0])
        self.dev = torch.device("cuda", 0)
        self.clock_t = torch.as_tensor(clock, device=self.dev)
        self.counts_t = torch.as_tensor(counts.view(np.int32), device=self.dev)
        self.times_t = torch.as_tensor(np.stack(self.times), device=self.dev)
        self.ids_t = [torch.as_tensor(v.astype(np.uint32).view(np.int32), device=self.dev) for v in (self.pair_a, self.pair_b, self.time_row)]
        self._want = {}

    def sizes(self, n_groups, n_win, n_thr, n_bins, rows):
        wins, cells = max(n_win, 1), n_groups * max(n_win, 1)
        s = {"pair_counts": self.P * wins * 5, "pair_sums": self.P * wins * 4, "unmatched": self.P * 2, "cell_counts": cells * 16,
             "above": cells * n_thr * 2, "extremes": cells * 4, "hist": cells * 2 * n_bins, "tails": cells * 4}
        if rows:
            s["row_a"] = s["row_b"] = self.P * self.n_draw
        return s

    def run(self, eng, group, n_groups, edges, thresholds=None, binning=(5, -20, 32), rows=True, buf=None):
        """One call; returns the outputs (numpy) after checking that no word outside them changed."""
        import torch

        m, e0, o = binning
        th = np.zeros(0) if thresholds is None else np.asarray(thresholds, dtype=np.float64)
        n_win, n_thr, n_bins = 0 if edges is None else len(edges) - 1, int(th.shape[0]), o << m
        off, at = {}, GUARD
        for k, size in self.sizes(n_groups, n_win, n_thr, n_bins, rows).items():
            off[k] = (at, size)
            at += size + (size & 1) + GUARD                             # (even: the 64-bit outputs stay 8-byte aligned)
        if buf is None:
            buf = torch.full((at,), SENTINEL, dtype=torch.int32, device=self.dev)
        grp_t = None
        if group is not None:
            grp = np.asarray(group, dtype=np.int64)
            grp_t = torch.as_tensor(np.where(grp < 0, _abi.POOL_SKIP, grp).astype(np.uint32).view(np.int32), device=self.dev)
        ptr = {k: buf.data_ptr() + 4 * o_ if size else 0 for k, (o_, size) in off.items()}
        torch.cuda.synchronize(self.dev)
        ms, scratch = eng.summarize_pairs(
            self.n, self.P, n_groups, pair_a_ptr=self.ids_t[0].data_ptr(), pair_b_ptr=self.ids_t[1].data_ptr(), times_ptr=self.times_t.data_ptr(),
            time_row_ptr=self.ids_t[2].data_ptr(), n_time_rows=len(self.times), draw_capacity=self.n_draw, clock_ptr=self.clock_t.data_ptr(),
            clock_capacity=self.cap, counts_ptr=self.counts_t.data_ptr(), pair_counts_ptr=ptr["pair_counts"], pair_sums_ptr=ptr["pair_sums"],
            unmatched_ptr=ptr["unmatched"], cell_counts_ptr=ptr["cell_counts"], extremes_ptr=ptr["extremes"], hist_ptr=ptr["hist"],
            tails_ptr=ptr["tails"], above_ptr=ptr["above"], row_a_ptr=ptr.get("row_a", 0), row_b_ptr=ptr.get("row_b", 0),
            group_ptr=grp_t.data_ptr() if grp_t is not None else 0, edges=edges, thresholds=th, sub_bits=m, min_exp=e0, octaves=o)
        assert ms > 0.0 and scratch >= 0
        words = buf.cpu().numpy().view(np.uint32)
        inside = np.zeros(at, dtype=bool)
        raw = {}
        for k, (o_, size) in off.items():
            inside[o_: o_ + size] = True
            raw[k] = words[o_: o_ + size].copy()
        assert (words[~inside] == SENTINEL).all(), "a word outside the outputs changed"
        wins = max(n_win, 1)
        out = {"buf": buf, "words": raw}
        pcn = raw["pair_counts"].reshape(self.P, wins, 5)
        for k, key in enumerate(PAIR_KEYS):
            out[key] = pcn[:, :, k]
        ps = raw["pair_sums"].view(np.float64).reshape(self.P, wins, 2)
        out["sum_d"], out["sum_a"] = ps[:, :, 0], ps[:, :, 1]
        out["unmatched"] = raw["unmatched"].reshape(self.P, 2)
        cc = raw["cell_counts"].view(np.uint64).reshape(n_groups, wins, 8)
        for k, key in enumerate(CELL_KEYS):
            out["cell_" + key] = cc[:, :, k]
        out["above"] = raw["above"].view(np.uint64).reshape(n_groups, wins, n_thr)
        ex = raw["extremes"].view(np.float64).reshape(n_groups, wins, 2)
        out["min_d"], out["max_d"] = ex[:, :, 0], ex[:, :, 1]
        hh = raw["hist"].reshape(n_groups, wins, 2, n_bins)
        out["hist_pos"], out["hist_neg"] = hh[:, :, 0], hh[:, :, 1]
        tt = raw["tails"].reshape(n_groups, wins, 4)
        for k, key in enumerate(TAIL_KEYS):
            out[key] = tt[:, :, k]
        if rows:
            out["row_a"], out["row_b"] = raw["row_a"].reshape(self.P, self.n_draw), raw["row_b"].reshape(self.P, self.n_draw)
        return out

    def want(self, p, edges, thresholds, binning):
        key = (p, None if edges is None else edges.tobytes(), None if thresholds is None else np.asarray(thresholds).tobytes(), binning)
        if key not in self._want:
            m, e0, o = binning
            self._want[key] = latency_pairs(self.stored[self.pair_a[p]], self.stored[self.pair_b[p]], self.times[self.time_row[p]], edges,
                                            thresholds=thresholds, sub_bits=m, min_exp=e0, octaves=o)
        return self._want[key]

    def check(self, got, group, n_groups, edges, thresholds=None, binning=(5, -20, 32)):
        """Every word of `got` against the host definition."""
        per = [self.want(p, edges, thresholds, binning) for p in range(self.P)]
        for p, w in enumerate(per):
            for key in PAIR_KEYS:
                assert got[key][p].dtype == np.uint32 and np.array_equal(got[key][p], w[key]), (key, p)
            for key in ("sum_d", "sum_a"):
                assert pc.same_words(got[key][p], w[key]), (key, p, got[key][p], w[key])
            assert got["unmatched"][p].tolist() == [w["unmatched_a"], w["unmatched_b"]], p
            if "row_a" in got:
                for key in ("row_a", "row_b"):
                    n_arr = w[key].shape[0]
                    assert np.array_equal(got[key][p, :n_arr], w[key]) and (got[key][p, n_arr:] == PAIR_NONE).all(), (key, p)
        cells = latency_pair_cells(per, group, n_groups)
        for key in CELL_KEYS:
            assert np.array_equal(got["cell_" + key], cells[key]), key
        for key in ("above", "hist_pos", "hist_neg", *TAIL_KEYS):
            assert got[key].dtype == cells[key].dtype and np.array_equal(got[key], cells[key]), key
        for key in ("min_d", "max_d"):
            assert np.array_equal(got[key].view(np.uint64), cells[key].view(np.uint64)), (key, got[key], cells[key])
        ident = got["cell_equal"] + got["cell_nan"] + sum(got[k].astype(np.uint64) for k in TAIL_KEYS) \
            + got["hist_pos"].sum(axis=2, dtype=np.uint64) + got["hist_neg"].sum(axis=2, dtype=np.uint64)
        assert np.array_equal(ident, got["cell_both"])
        return cells

    def both(self, eng, group, n_groups, edges, thresholds=None, binning=(5, -20, 32), **kw):
        got = self.run(eng, group, n_groups, edges, thresholds, binning, **kw)
        self.check(got, group, n_groups, edges, thresholds, binning)
        return got


def _own_sides(rng, arrivals, rows_a, rows_b, order, n_draw=331, **kw):
    """Pair p has its own arrival row (arrivals[p] of them) and its own two scenarios 2 p and 2 p + 1."""
    times = [pc.arrival_row(rng, m, n_draw, duplicates=3) for m in arrivals]
    clocks = []
    for t, ra, rb in zip(times, rows_a, rows_b):
        clocks += [pc.side_rows(rng, t, ra, order), pc.side_rows(rng, t, rb, pc.ORDERS[(pc.ORDERS.index(order) + 1) % 3] if ra % 2 else order)]
    P = len(times)
    return _Batch(times, clocks, 2 * np.arange(P), 2 * np.arange(P) + 1, np.arange(P), **kw)


@pytest.mark.parametrize("order", pc.ORDERS)
def test_row_lengths_on_both_sides_orders_windows_thresholds_and_binnings(eng, order):
    rng = np.random.default_rng(pc.ORDERS.index(order))
    L = pc.ROWS
    rows_a = [L[k % 6] for k in range(12)]
    rows_b = [L[(k // 2 + 3) % 6] if k < 6 else L[(k * 5 + 1) % 6] for k in range(12)]       # both sides independently, a side with no rows
    arrivals = [max(a, b, 1) + (k % 3) * 5 for k, (a, b) in enumerate(zip(rows_a, rows_b))]
    b = _own_sides(rng, arrivals, rows_a, rows_b, order)
    group = [0, 2, 2, -1, 0, 2, 2, 2, 0, 4, -1, 4]                                           # uneven groups, skips, the empty groups 1 and 3
    seen = 0
    for k, n_win in enumerate((0, 1, 7)):
        edges = pc.uneven_edges(n_win, b.times[5])
        for j, binning in enumerate(BINNINGS):
            th = pc.signed_thresholds((0, 64, 5)[(k + j) % 3])
            got = b.both(eng, group, 5, edges, th, binning, rows=(k + j) % 2 == 0)
            b.both(eng, None, 1, edges, th, binning, rows=(k + j) % 2 == 1)
            assert (got["cell_both"][1] == 0).all() and (got["hist_pos"][3] == 0).all() and np.isposinf(got["min_d"][1]).all() and np.isneginf(got["max_d"][3]).all()
            seen += int(got["cell_both"].sum() > 100 and got["cell_only_a"].sum() > 0 and got["cell_only_b"].sum() > 0 and got["cell_neither"].sum() > 0)
    assert seen >= 6
    got = b.both(eng, np.arange(12), 12, None, pc.signed_thresholds(64))
    assert got["unmatched"].sum() > 20 and got["cell_nan"].sum() > 0 and got["cell_equal"].sum() > 0 and got["above"].sum() > 0


def test_as_many_windows_as_arrivals_and_one_above_the_lds_resident_limit(eng):
    rng = np.random.default_rng(11)
    b = _own_sides(rng, [300, 65, 1], [300, 60, 1], [290, 65, 0], "shuffle")
    e300 = pc.uneven_edges(300, b.times[0])
    got = b.both(eng, [0, 1, 0], 2, e300, pc.signed_thresholds(5))
    assert int(got["cell_both"].sum()) > 250
    on_arrivals = np.unique(b.times[0][np.isfinite(b.times[0])])                             # every arrival an edge: windows of one request
    b.both(eng, None, 1, on_arrivals, None, (2, -8, 6))
    for n_win in (LDS_WINDOWS, LDS_WINDOWS + 1):
        edges = pc.uneven_edges(n_win, b.times[0])
        got = b.both(eng, [0, 1, 0], 2, edges, pc.signed_thresholds(3), (2, -8, 6))
        wide = b.both(eng, [0, 1, 0], 2, edges[[0, n_win // 2, n_win]], pc.signed_thresholds(3), (2, -8, 6))
        for key in ("cell_both", "cell_slower", "above", "hist_pos", "hist_neg"):
            assert np.array_equal(got[key].sum(axis=1), wide[key].sum(axis=1)), key


@pytest.mark.parametrize("P", [1, 130])
def test_one_and_many_pairs_in_one_and_in_small_chunks_twice_over(eng, P):
    rng = np.random.default_rng(20 + P)
    arrivals = [int(v) for v in rng.integers(0, 200, P)]
    arrivals[0] = 300
    rows_a = [int(rng.integers(0, m + 1)) for m in arrivals]
    rows_b = [int(rng.integers(0, m + 1)) for m in arrivals]
    b = _own_sides(rng, arrivals, rows_a, rows_b, "shuffle")
    group = None if P == 1 else np.arange(P) % 7 - 1
    G = 1 if P == 1 else 6
    edges, th = pc.uneven_edges(7, b.times[0]), pc.signed_thresholds(5)
    first = b.both(eng, group, G, edges, th)
    again = b.run(eng, group, G, edges, th, buf=first["buf"])                                 # the same buffers, written a second time
    os.environ["AF_PAIRS_CHUNK"] = "7"
    try:
        small = b.both(eng, group, G, edges, th)
        no_rows = b.both(eng, group, G, edges, th, rows=False)
    finally:
        del os.environ["AF_PAIRS_CHUNK"]
    for key, words in first["words"].items():
        assert np.array_equal(words, again["words"][key]) and np.array_equal(words, small["words"][key]), key
        if key not in ("row_a", "row_b"):
            assert np.array_equal(words, no_rows["words"][key]), key
    # the pairs in another order, among strangers: the same cells
    order = rng.permutation(P)
    mixed = _Batch(b.times, [b.stored[i] for i in range(b.n)], b.pair_a[order], b.pair_b[order], b.time_row[order], cap=b.cap)
    other = mixed.both(eng, None if group is None else group[order], G, edges, th)
    for key in ("cell_" + k for k in CELL_KEYS):
        assert np.array_equal(first[key], other[key]), key
    for key in ("above", "hist_pos", "hist_neg", "min_d", "max_d", *TAIL_KEYS):
        assert np.array_equal(first[key], other[key]), key


def test_one_baseline_shared_by_every_pair_and_counts_above_the_capacity(eng):
    rng = np.random.default_rng(31)
    n_draw = MATCH_ROWS + 200                                                                 # two work items a side in the match pass
    times = [pc.arrival_row(rng, MATCH_ROWS + 130, n_draw, duplicates=5)]
    clocks = [pc.side_rows(rng, times[0], MATCH_ROWS + 100, "arrival")] + [pc.side_rows(rng, times[0], r, o) for r, o in
                                                                         ((MATCH_ROWS + 65, "arrival"), (900, "shuffle"), (64, "reversed"), (0, "arrival"))]
    b = _Batch(times, clocks, [0, 0, 0, 0, 0], [1, 2, 3, 4, 0], [0] * 5)
    for edges in (None, pc.uneven_edges(7, times[0]), pc.uneven_edges(61, times[0])):
        got = b.both(eng, [0, 0, 1, 1, 2], 3, edges, pc.signed_thresholds(5))
        # the pair of the baseline with itself: every matched request differs by +0.0 (the hostile NaN and inf - inf rows: nan)
        assert np.array_equal(got["cell_equal"][2], got["cell_both"][2] - got["cell_nan"][2]) and got["cell_both"][2].sum() > 3000 and got["cell_nan"][2].sum() < 9
        assert (got["sum_d"][4].view(np.uint64) == 0).all() and (got["only_a"][4] == 0).all() and (got["only_b"][4] == 0).all()
        some = got["cell_equal"][2] > 0
        assert (got["min_d"][2][some].view(np.uint64) == 0).all() and (got["max_d"][2][some].view(np.uint64) == 0).all()
    # counts above the capacity are clipped; the rows behind the stored ones are not read
    c = _Batch(times, clocks, [0, 0, 0, 0], [1, 2, 3, 4], [0] * 4, cap=600, counts_extra=2)
    assert all(len(x) <= 600 for x in c.stored) and sum(len(x) == 600 for x in c.stored) == 3
    c.both(eng, None, 1, pc.uneven_edges(7, times[0]), pc.signed_thresholds(5))


def test_the_swapped_pair_mirrors_every_word(eng):
    rng = np.random.default_rng(32)
    times = [pc.arrival_row(rng, 300, 300)]
    clocks = [pc.side_rows(rng, times[0], 280, "shuffle"), pc.side_rows(rng, times[0], 290, "arrival")]
    b = _Batch(times, clocks, [0, 1], [1, 0], [0, 0])
    got = b.both(eng, [0, 1], 2, pc.uneven_edges(7, times[0]), pc.signed_thresholds(5))
    nz = got["sum_d"][0] != 0
    assert nz.any() and np.array_equal((-got["sum_d"][0][nz]).view(np.uint64), got["sum_d"][1][nz].view(np.uint64))
    assert np.array_equal(got["hist_pos"][0], got["hist_neg"][1]) and np.array_equal(got["hist_neg"][0], got["hist_pos"][1])
    assert np.array_equal(got["cell_slower"][0], got["cell_faster"][1]) and np.array_equal(got["cell_only_a"][0], got["cell_only_b"][1])
    some = got["cell_both"][0] > got["cell_nan"][0]
    assert np.array_equal((-got["max_d"][1][some]).view(np.uint64), got["min_d"][0][some].view(np.uint64))


def test_refusals_leave_every_output_word_alone(eng):
    import torch

    from asyncflow_amd.engine import PLAN_ONLY, Engine

    rng = np.random.default_rng(33)
    b = _own_sides(rng, [40, 40, 40], [30, 40, 20], [40, 10, 30], "shuffle", n_draw=50)
    lib, dev = eng._lib, b.dev  # noqa: SLF001
    P, G, n_bins, T = 3, 3, 1024, 2
    sizes = b.sizes(G, 2, T, n_bins, True)
    off, at = {}, GUARD
    for k, size in sizes.items():
        off[k] = at
        at += size + (size & 1) + GUARD
    buf = torch.full((at,), SENTINEL, dtype=torch.int32, device=dev)
    grp_ok = torch.zeros(3, dtype=torch.int32, device=dev)
    ids_bad = torch.as_tensor(np.array([0, 6, 1], dtype=np.int32), device=dev)
    grp_bad = torch.as_tensor(np.array([0, 3, 1], dtype=np.int32), device=dev)

    def call(handle=None, *, n=6, n_pairs=P, n_groups=G, edges=(0.0, 1.0, 8.0), n_win=None, group=grp_ok, clock=True, counts=True, cap=None,
             binning=(5, -20, 32), thresholds=(0.0, 0.1), n_thr=None, pair_a=None, pair_b=None, time_row=None, times=True, n_time_rows=3,
             n_draw=50, drop=(), counts_t=None):
        e = np.ascontiguousarray(edges, dtype=np.float64) if edges is not None else None
        th = np.ascontiguousarray(thresholds, dtype=np.float64) if thresholds is not None else None
        out = _abi.AfOutputs(b.cap if cap is None else cap, C.c_void_p(b.clock_t.data_ptr() if clock else None), 0, None,
                             C.c_void_p((counts_t if counts_t is not None else b.counts_t).data_ptr() if counts else None))
        p = {k: C.c_void_p(None if k in drop else buf.data_ptr() + 4 * o_) for k, o_ in off.items()}
        ids = [(given if given is not None else own) for given, own in zip((pair_a, pair_b, time_row), b.ids_t)]
        req = _abi.AfPairs(n, n_pairs, n_groups, (0 if e is None else e.shape[0] - 1) if n_win is None else n_win,
                           *(C.c_void_p(None if v is False else v.data_ptr()) for v in ids[:2]),
                           C.c_void_p(group.data_ptr() if group is not None else None),
                           e.ctypes.data_as(C.POINTER(C.c_double)) if e is not None else None,
                           C.c_void_p(b.times_t.data_ptr() if times else None), C.c_void_p(None if ids[2] is False else ids[2].data_ptr()),
                           n_time_rows, n_draw, th.ctypes.data_as(C.POINTER(C.c_double)) if th is not None else None,
                           (0 if th is None else th.shape[0]) if n_thr is None else n_thr, *binning,
                           p["pair_counts"], p["pair_sums"], p["unmatched"], p["cell_counts"], p["above"], p["extremes"], p["hist"], p["tails"],
                           p["row_a"], p["row_b"], 0.0, 0)
        torch.cuda.synchronize(dev)
        rc = lib.af_engine_summarize_pairs(handle or eng._h, C.byref(out), C.byref(req))  # noqa: SLF001
        assert (buf.cpu().numpy().view(np.uint32) == SENTINEL).all(), "a refused call wrote an output word"
        return rc

    inv, cap_err = _abi.AF_ERR_INVALID, _abi.AF_ERR_CAPACITY
    assert call(n=0) == inv and call(n_pairs=0) == inv and call(n_groups=0) == inv and call(n_time_rows=0) == inv and call(n_draw=0) == inv
    for bad in ((9, -20, 1), (5, -1023, 4), (5, -20, 0), (5, 1000, 24), (5, -20, 129), (8, 0, 17)):
        assert call(binning=bad) == inv, bad
    for bad in ((0.0, 1.0, 1.0), (2.0, 1.0, 3.0), (0.0, float("inf"), 9.0), (float("nan"), 1.0, 2.0), (-float("inf"), 0.0, 1.0)):
        assert call(edges=bad) == inv, bad
    assert call(edges=None, n_win=2) == inv                                               # edges NULL with n_windows > 0
    assert call(n_win=0) == inv                                                           # edges given with n_windows == 0
    assert call(thresholds=[0.0] * 65) == inv and call(thresholds=(0.0, float("inf"))) == inv and call(thresholds=(float("nan"),)) == inv
    assert call(thresholds=None, n_thr=2) == inv and call(drop=("above",)) == inv
    assert call(pair_a=ids_bad) == inv and call(pair_b=ids_bad) == inv and call(time_row=ids_bad) == inv and call(group=grp_bad) == inv
    assert call(n=5) == inv                                                               # scenario 5 is a side of the third pair
    assert call(pair_a=False) == inv and call(pair_b=False) == inv and call(time_row=False) == inv and call(times=False) == inv
    assert call(clock=False) == inv and call(counts=False) == inv and call(cap=0) == inv
    for k in ("pair_counts", "pair_sums", "unmatched", "cell_counts", "extremes", "hist", "tails"):
        assert call(drop=(k,)) == inv, k
    assert call(n_pairs=2 ** 31, edges=(0.0, 1.0, 2.0)) == cap_err                        # n_pairs * W' = 2^32
    assert call(n_groups=2 ** 22, edges=None, group=None) == cap_err                     # 2^22 groups * 1 window * 1 024 bins = 2^32 words
    assert call(n_groups=2 ** 21, group=None) == cap_err
    assert call(n_draw=2 ** 31) == cap_err
    many = np.zeros((6, _abi.CNT_SLOTS), dtype=np.uint32)
    many[:, _abi.CNT_COMPLETED] = 2 ** 31
    full = torch.as_tensor(many.view(np.int32), device=dev)
    assert call(n_groups=1, cap=2 ** 31, n_draw=2 ** 31 - 1, counts_t=full) == cap_err   # a group that could match 3 * (2^31 - 1) requests
    plan_only = Engine(lower(single_server(horizon=50)), PLAN_ONLY)
    try:
        assert call(plan_only._h) == _abi.AF_ERR_NO_DEVICE  # noqa: SLF001
    finally:
        plan_only.close()
    b.both(eng, [0, 1, 2], 3, np.array([0.0, 1.0, 8.0]), np.array([0.0, 0.1]))


def test_a_run_with_common_seeds_through_the_python_api(tmp_path):
    from asyncflow_amd import expand_grid
    from asyncflow_amd.results import ShardedResults
    from asyncflow_amd.runner import SimulationRunner

    payload = lb_two_servers(horizon=20)
    edge = "topology_graph.edges[lb-srv1].latency.mean"
    grid = expand_grid({edge: [0.002, 0.02]}, replicas=4, common_seeds=True)
    res = SimulationRunner(simulation_input=payload, **grid.runner_kwargs()).run()
    p = grid.pairs(edge, 0.002, 0.02)
    assert p["a"].tolist() == [0, 1, 2, 3] and p["b"].tolist() == [4, 5, 6, 7] and p["by"].tolist() == [0] * 4
    e5 = np.arange(0.0, 21.0, 5.0)
    th = [-0.01, 0.0, 0.01, 0.2]

    def host(a, b, edges, groups, n_groups, **kw):
        per = [latency_pairs(res[int(i)].rqs_clock, res[int(j)].rqs_clock, res.arrival_times(int(i)), edges, **kw) for i, j in zip(a, b)]
        return per, latency_pair_cells(per, groups, n_groups)

    def check(summ, per, cells):
        for k, w in enumerate(per):
            for key in PAIR_KEYS:
                assert np.array_equal(summ[key][k], w[key]), (key, k)
            for key in ("sum_d", "sum_a"):
                assert pc.same_words(summ[key][k], w[key]), (key, k)
            assert (int(summ["unmatched_a"][k]), int(summ["unmatched_b"][k])) == (w["unmatched_a"], w["unmatched_b"]) == (0, 0)
            if "row_a" in summ:
                n_arr = w["row_a"].shape[0]
                assert np.array_equal(summ["row_a"][k, :n_arr], w["row_a"]) and np.array_equal(summ["row_b"][k, :n_arr], w["row_b"])
        for key in PAIR_KEYS:
            assert np.array_equal(summ["cell_" + key], cells[key]), key
        for key in ("slower", "faster", "equal", "above", "hist_pos", "hist_neg", *TAIL_KEYS):
            assert np.array_equal(summ[key], cells[key]), key
        for key in ("min_d", "max_d"):
            assert np.array_equal(summ[key].view(np.uint64), cells[key].view(np.uint64)), key

    summ = res.paired_summary(p["a"], p["b"], 5.0, by=p["by"], thresholds=th, with_rows=True)
    per, cells = host(p["a"], p["b"], e5, p["by"], 1, thresholds=th)
    check(summ, per, cells)
    assert summ["both"].shape == (4, 4) and summ["hist_pos"].shape == (1, 4, 1024) and int(summ["cell_both"].sum()) > 1000
    assert int(summ["slower"].sum()) > int(summ["faster"].sum())                          # the slower edge slows requests
    valid = summ["both"].astype(np.float64) - summ["nan"]
    assert np.allclose(summ["mean_d"][valid > 0], (summ["sum_d"] / valid)[valid > 0]) and np.nanmean(summ["relative"]) > 0
    # one window, singletons, another binning, no thresholds
    whole = res.paired_summary(p["a"], p["b"], by="pair", sub_bits=3, min_exp=-12, octaves=12)
    check(whole, *host(p["a"], p["b"], None, np.arange(4), 4, sub_bits=3, min_exp=-12, octaves=12))
    # a run against itself, and the swapped pair
    own = res.paired_summary(p["a"], p["a"], 5.0)
    assert np.array_equal(own["equal"], own["cell_both"]) and (own["sum_d"].view(np.uint64) == 0).all() and (own["only_a"] == 0).all() and (own["only_b"] == 0).all()
    swapped = res.paired_summary(p["b"], p["a"], 5.0, by=p["by"], thresholds=th)
    check(swapped, *host(p["b"], p["a"], e5, p["by"], 1, thresholds=th))
    assert np.array_equal((-summ["sum_d"]).view(np.uint64)[summ["sum_d"] != 0], swapped["sum_d"].view(np.uint64)[summ["sum_d"] != 0])
    assert np.array_equal(summ["hist_pos"], swapped["hist_neg"]) and np.array_equal(summ["slower"], swapped["faster"])
    assert np.array_equal((-summ["max_d"]).view(np.uint64), swapped["min_d"].view(np.uint64))
    # what is read off a summary
    halves = paired_merge(res.paired_summary(p["a"][:2], p["b"][:2], 5.0, thresholds=th), res.paired_summary(p["a"][2:], p["b"][2:], 5.0, thresholds=th))
    for key in ("both", "slower", "above", "hist_pos", "hist_neg"):
        assert np.array_equal(halves[key], np.asarray(summ["cell_" + key if key == "both" else key]).astype(np.int64)), key
    assert np.array_equal(halves["min_d"], summ["min_d"]) and halves["replicas"].tolist() == [4]
    br = paired_delta_quantiles(summ, [0.05, 0.5, 0.95])
    for w in range(4):
        d = np.concatenate([x["d"][x["bounds"][w]: x["bounds"][w + 1]] for x in per])
        d = d[~np.isnan(d)]
        exact = np.quantile(d, [0.05, 0.5, 0.95], method="lower")
        assert ((br["lo"][0, w] <= exact) & (exact < br["hi"][0, w])).all(), w
    bands = res.paired_bands(p["a"], p["b"], 5.0, by=p["by"])
    assert bands["mean"].shape == (1, 4, 3) and bands["n"].tolist() == [[4, 4, 4, 4]] and (bands["ci_halfwidth"][0, :, 0] > 0).all()
    assert np.allclose(bands["mean"][0, :, 0], summ["mean_d"].mean(axis=0))
    for name in ("paired.npz", "paired.parquet"):
        written = res.save_paired_summary(str(tmp_path / name), p["a"], p["b"], p["by"], window_s=5.0, thresholds=th)
        back = load_summary(str(tmp_path / name))
        assert set(back) == set(written)
        twice = paired_merge(back, summ)
        assert np.array_equal(twice["hist_pos"], 2 * summ["hist_pos"].astype(np.int64)) and twice["replicas"].tolist() == [8]
    # refusals of the surface
    with pytest.raises(ValueError, match="seeds differ"):
        res.paired_summary([0, 1], [4, 6])
    other = expand_grid({edge: [0.002, 0.02]}, replicas=2)
    plain = SimulationRunner(simulation_input=payload, **other.runner_kwargs()).run()
    with pytest.raises(ValueError, match="pair 0 .*seeds differ"):
        plain.paired_summary(**{k: other.pairs(edge, 0.002, 0.02)[k] for k in ("a", "b")})
    with pytest.raises(NotImplementedError, match="several devices"):
        ShardedResults([res], [np.arange(8)], 0.0).paired_summary(p["a"], p["b"])
