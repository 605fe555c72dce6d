"""Occupancy histograms of the sampled series per (group, window of ticks, output column) on the MI355X
(af_engine_summarize_series_histogram): synthetic sample blocks handed straight to the entry -- the padding words and the rows
at or past a scenario's ticks hold 0xFFFFFFFF, a word that lands in `over` and breaks under + sum(hist) + over == count if it
is read -- with every output in one buffer between sentinels.  Every comparison is == on integers against the host definition
(results.series_window_histogram of every scenario, the members of a group added up); no count has a tolerance (the bands'
float means and quantiles over the replicas are held to 1e-12).

n = 23 scenarios of 700 ticks (0, all, more than stored, 1 among them): the plans of 32, 21 and 5 rows a step on every window
shape, grouping and binning; the wide plans (3, 2, 1 and 1 rows a step, and one whose rows need a second pass); columns that
every lane agrees on; many waves into one cell; 253 output columns of 1 024 bins in chunks; independence of column selection,
batch and call; NULL outputs; the scratch bound; the refusals; and an event workload through the Python API."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from asyncflow_amd import _abi
from asyncflow_amd.results import load_summary, series_histogram_quantiles, series_window_histogram, tick_window_edges
from oracle.scenarios import lb_with_events
from tests.test_gpu_series_windows import WIDE, _block, _groupings, _plan, _shapes, _ticks, _wide_plan, _wide_shapes, ram_columns

pytestmark = pytest.mark.gpu

FILL = 0xFFFFFFFF
PATTERN = 0x5A5A5A5A
OUTS = ("count", "hist", "under", "over")
RESIDUE = np.float32(-(2.0 ** -45))
WIDTHS = (1.0, 3.0, 0.25, 0.1, 1.0 / 3.0)
N, CAP = 23, 700


def _plans(name):
    return _wide_plan(name) if name in WIDE else _plan(name)


def _rows_per_step(plan) -> int:
    return 64 // min(plan.series_pitch // 4, 64)


def _hist_block(plan, rng, n: int, cap: int, ticks, top: int = 64):
    """Sample blocks [n, cap, pitch]: integer columns with more than half of their mass at 0, values up to top + 2 and the
    values top - 1, top, top + 1, 3 top and 2^20 among the rest; ram columns of multiples of 1/256 in [-2, top + 2) with -0.0,
    +0.0, the -2^-45 residue and whole values (bin edges).  Padding words and the rows at or past a scenario's min(ticks, cap)
    hold 0xFFFFFFFF.  Returns the block and the counts."""
    blk, counts = _block(plan, rng, n, cap, ticks)
    S = plan.n_series
    ram = ram_columns(S, plan.n_edges)
    u = rng.random((n, cap, S))
    special = np.array([top - 1, top, top + 1, 3 * top, 2 ** 20])
    body = np.where(u < 0.55, 0, np.where(u < 0.85, rng.integers(0, top + 3, (n, cap, S)), special[rng.integers(0, 5, (n, cap, S))])).astype(np.uint32)
    f = (rng.integers(-2 * 256, (top + 2) * 256, (n, cap, S)) / 256.0).astype(np.float32)
    f[u < 0.1] = np.float32(-0.0)
    f[(u >= 0.1) & (u < 0.2)] = np.float32(0.0)
    f[(u >= 0.2) & (u < 0.3)] = RESIDUE
    whole = (u >= 0.3) & (u < 0.4)
    f[whole] = rng.integers(0, top + 2, int(whole.sum())).astype(np.float32)
    body[:, :, ram] = f.view(np.uint32)[:, :, ram]
    blk[:, :, :S] = body
    blk[:, :, S:] = FILL
    for s in range(n):
        blk[s, min(int(counts[s, _abi.CNT_TICKS]), cap):] = FILL
    return blk, counts


class _Device:
    """A block on the device and an engine for any number of calls on it."""

    def __init__(self, plan, blk, counts):
        import torch

        from asyncflow_amd.engine import Engine

        self.torch, self.plan, self.n, self.cap = torch, plan, blk.shape[0], blk.shape[1]
        self.dev = torch.device("cuda", 0)
        self.blk_t = torch.as_tensor(blk.view(np.int32), device=self.dev)
        self.counts_t = torch.as_tensor(counts.view(np.int32), device=self.dev)
        self.eng = Engine(plan, 0)

    def close(self):
        self.eng.close()

    def run(self, edges, bins, group=None, n_groups=1, columns=None, lo=None, width=None, outputs=OUTS):
        """The requested outputs as uint32 arrays and scratch_bytes; all four outputs have their place in one buffer between
        sentinels, and no word outside the requested ones may change."""
        torch = self.torch
        W, Cn = len(edges) - 1, self.plan.n_series if columns is None else len(columns)
        shape = {"count": (n_groups, W), "hist": (n_groups, W, Cn, bins), "under": (n_groups, W, Cn), "over": (n_groups, W, Cn)}
        guard, at, off = 64, 64, {}
        for k in OUTS:
            off[k] = at
            at += int(np.prod(shape[k])) + guard
        assert at * 4 < 72 << 20, "an output buffer of a test stays below about 64 MB"
        buf = torch.full((at,), PATTERN, dtype=torch.int32, device=self.dev)
        grp_t = None
        if group is not None:
            ids = np.asarray(group, dtype=np.int64)
            grp_t = torch.as_tensor(np.where(ids < 0, _abi.POOL_SKIP, ids).astype(np.uint32).view(np.int32), device=self.dev)
        torch.cuda.synchronize(self.dev)              # (the engine has a stream of its own)
        _, scratch = self.eng.summarize_series_histogram(
            self.n, n_groups, edges, bins, samples_ptr=self.blk_t.data_ptr(), tick_capacity=self.cap,
            counts_ptr=self.counts_t.data_ptr(), group_ptr=0 if grp_t is None else grp_t.data_ptr(), columns=columns, lo=lo, width=width,
            **{f"{k}_ptr": buf.data_ptr() + 4 * off[k] for k in outputs})
        host = buf.cpu().numpy().view(np.uint32)
        written = np.zeros(at, dtype=bool)
        out = {}
        for k in outputs:
            size = int(np.prod(shape[k]))
            written[off[k]:off[k] + size] = True
            out[k] = host[off[k]:off[k] + size].reshape(shape[k])
        assert (host[~written] == PATTERN).all(), f"a word outside the requested outputs {outputs} was written"
        return out, scratch


def _want(plan, blk, counts, edges, bins, groupings, columns=None, lo=None, width=None):
    """results.series_window_histogram of every scenario's stored rows, the members of every group added up (a scenario with a
    negative id is left out; None: all in group 0): one dict of int64 arrays per (group, n_groups, ...) of `groupings`."""
    n, cap, _ = blk.shape
    out = None
    for s in range(n):
        m = min(int(counts[s, _abi.CNT_TICKS]), cap)
        one = series_window_histogram(np.ascontiguousarray(blk[s, :m, :plan.n_series].T), edges, plan.n_edges, bins, columns, lo, width)
        if out is None:
            out = [{k: np.zeros((g[1],) + one[k].shape, dtype=np.int64) for k in OUTS} for g in groupings]
        for g, acc in zip(groupings, out):
            gid = 0 if g[0] is None else int(g[0][s])
            if gid >= 0:
                for k in OUTS:
                    acc[k][gid] += one[k]
    return out


def _want_one(plan, blk, counts, edges, bins, group, n_groups, columns=None, lo=None, width=None):
    return _want(plan, blk, counts, edges, bins, [(group, n_groups)], columns, lo, width)[0]


def _equal(got, want, what):
    for k in got:
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        g = got[k].astype(np.int64)
        assert np.array_equal(g, want[k]), (what, k, np.argwhere(g != want[k])[:5], g[g != want[k]][:5], want[k][g != want[k]][:5])
    if set(got) == set(OUTS):
        total = got["under"].astype(np.int64) + got["hist"].astype(np.int64).sum(axis=-1) + got["over"]
        assert np.array_equal(total, np.broadcast_to(got["count"].astype(np.int64)[:, :, None], total.shape)), (what, "under + hist + over != count")


def _binnings(plan, rng):
    """(name, bins, columns, lo, width): the NULL default with 64 bins, 1 bin, 2 bins, and a binning per output column with
    every width on integer and on ram columns, the columns permuted and two of them twice."""
    S = plan.n_series
    ram = np.nonzero(ram_columns(S, plan.n_edges))[0]
    columns = np.concatenate([rng.permutation(S), [0, ram[0]]])
    lo = np.array([(0.0, 2.0, -1.0, 0.5, 3.0)[(i // 5) % 5] for i in range(len(columns))])
    width = np.array([WIDTHS[i % 5] for i in range(len(columns))])
    for j in (0, int(ram[0])):                      # every width on an integer and on a ram column
        assert j in columns
    return [("default, 64 bins", 64, None, None, None), ("1 bin", 1, None, None, None), ("2 bins", 2, None, None, None),
            ("per column, 16 bins", 16, columns, lo, width)]


# ------------------------------------------------------------------------------------ 1. against the host definition
@pytest.mark.parametrize("name", ["single_server", "lb_two_servers", "fanout8"])
def test_synthetic_blocks_equal_the_host_definition(name):
    plan = _plan(name)
    assert _rows_per_step(plan) == {"single_server": 32, "lb_two_servers": 21, "fanout8": 5}[name]
    rng = np.random.default_rng(len(name))
    ticks = _ticks(rng, N, CAP)
    assert ticks[0] == 0 and ticks[1] == CAP and ticks[2] > CAP and ticks[3] == 1
    blk, counts = _hist_block(plan, rng, N, CAP, ticks)
    binnings = _binnings(plan, rng)
    seen = np.zeros(4, dtype=np.int64)
    d = _Device(plan, blk, counts)
    try:
        for what, edges in _shapes(CAP):
            for bname, bins, columns, lo, width in binnings:
                groupings = _groupings(N)
                if what == "one tick each":         # (the other combinations: outputs of more than 64 MB)
                    groupings = [g for g in groupings if (g[2] == "interleaved" and bins <= 16) or (g[2] == "singletons" and bins <= 2)]
                if not groupings:
                    continue
                wants = _want(plan, blk, counts, edges, bins, groupings, columns, lo, width)  # (the host definition once for every grouping)
                for (group, n_groups, gname), want in zip(groupings, wants):
                    got, _ = d.run(edges, bins, group, n_groups, columns, lo, width)
                    _equal(got, want, f"{name}, {what}, {gname}, {bname}")
                    seen += [int((want["under"] > 0).sum()), int((want["over"] > 0).sum()), int((want["hist"] > 1).sum()),
                             int((want["count"] == 0).sum())]
        assert (seen > 0).all(), seen
    finally:
        d.close()


# ------------------------------------------------------------------------------------ 2. wide plans
@pytest.mark.parametrize("name", ["wide_fanout16", "wide_fanout20", "wide_fanout50", "deep_chain62", "wide_fanout51"])
def test_wide_rows_equal_the_host_definition(name):
    plan = _wide_plan(name)
    assert (plan.n_series, plan.series_pitch) == WIDE[name]
    assert _rows_per_step(plan) == {"wide_fanout16": 3, "wide_fanout20": 2}.get(name, 1)
    assert (plan.series_pitch // 4 > 64) == (name == "wide_fanout51")                       # a second pass over the rows
    S = plan.n_series
    rng = np.random.default_rng(S)
    blk, counts = _hist_block(plan, rng, N, CAP, _ticks(rng, N, CAP), top=16)
    interleaved = next(g for g in _groupings(N) if g[2] == "interleaved")
    lo = np.array([(0.0, 2.0, -1.0)[j % 3] for j in range(S)])
    width = np.array([WIDTHS[j % 5] for j in range(S)])
    d = _Device(plan, blk, counts)
    try:
        for what, edges in _wide_shapes(CAP):
            for bname, lo_w in (("default", (None, None)), ("per column", (lo, width))):
                if bname == "per column" and what not in ("64 ticks", "uneven"):
                    continue
                groupings = [(None, 1, "one group (NULL)")]
                if what != "one tick each":         # (there: outputs of more than 64 MB)
                    groupings += [interleaved, (np.arange(N), N, "singletons")]
                wants = _want(plan, blk, counts, edges, 16, groupings, None, *lo_w)
                for (group, n_groups, gname), want in zip(groupings, wants):
                    got, _ = d.run(edges, 16, group, n_groups, None, *lo_w)
                    _equal(got, want, f"{name}, {what}, {gname}, {bname}")
        if name == "wide_fanout51":                                                          # the one series of the second pass alone
            got, _ = d.run(_wide_shapes(CAP)[2][1], 16, None, 1, [S - 1])
            _equal(got, _want_one(plan, blk, counts, _wide_shapes(CAP)[2][1], 16, None, 1, [S - 1]), f"{name}, the last series alone")
    finally:
        d.close()


# ------------------------------------------------------------------------------------ 3. contention
def test_columns_that_every_lane_agrees_on():
    """Column 0 is 0 in every row, column 1 alternates 0 / 1 row by row, all 23 scenarios in one group: bin 0 of column 0
    is the count, bins 0 and 1 of column 1 are the even and the odd rows."""
    plan = _plan("lb_two_servers")
    rng = np.random.default_rng(7)
    blk, counts = _hist_block(plan, rng, N, CAP, _ticks(rng, N, CAP))
    m = np.minimum(counts[:, _abi.CNT_TICKS].astype(np.int64), CAP)
    blk[:, :, 0] = np.where(np.arange(CAP)[None, :] < m[:, None], 0, FILL)
    blk[:, :, 1] = np.where(np.arange(CAP)[None, :] < m[:, None], np.arange(CAP)[None, :] % 2, FILL)
    d = _Device(plan, blk, counts)
    try:
        for what, edges in _shapes(CAP):
            for group in (None, np.zeros(N, dtype=np.int64)):
                got, _ = d.run(edges, 64, group, 1)
                _equal(got, _want_one(plan, blk, counts, edges, 64, group, 1), f"{what}")
                assert np.array_equal(got["hist"][0, :, 0, 0], got["count"][0]) and not got["hist"][0, :, 0, 1:].any(), what
                b = np.minimum(np.asarray(edges, dtype=np.int64)[None, :], m[:, None])
                odd = ((b[:, 1:] + 0) // 2 - (b[:, :-1] + 0) // 2).sum(axis=0)              # the odd rows of [lo, hi): hi // 2 - lo // 2
                assert np.array_equal(got["hist"][0, :, 1, 1], odd) and np.array_equal(got["hist"][0, :, 1, 0], got["count"][0] - odd), what
    finally:
        d.close()


@pytest.mark.parametrize("name", ["lb_two_servers", "single_server"])
def test_many_waves_add_into_one_cell(name):
    """300 scenarios of 64 ticks in one group: 300 waves add into every cell -- through their LDS histograms (one window of
    64 ticks), directly (windows of 20 ticks and of one tick), and as work items of several windows."""
    plan = _plan(name)
    rng = np.random.default_rng(300)
    n, cap = 300, 64
    blk, counts = _hist_block(plan, rng, n, cap, _ticks(rng, n, cap), top=8)
    d = _Device(plan, blk, counts)
    try:
        for what, edges in (("one window", np.array([0, cap])), ("20 ticks", tick_window_edges(20, cap)), ("one tick each", np.arange(cap + 1)),
                            ("uneven", np.array([1, 40, 41, 64, 90]))):
            groupings = [(None, 1), (np.arange(n) % 3, 3)]
            for (group, n_groups), want in zip(groupings, _want(plan, blk, counts, edges, 8, groupings)):
                got, _ = d.run(edges, 8, group, n_groups)
                _equal(got, want, f"{name}, {what}, {n_groups} groups")
    finally:
        d.close()


def test_work_items_of_several_windows():
    """The engine gives a wave max(1, W / ceil(32768 / n)) consecutive windows: 300 scenarios and 700 windows of one tick are
    runs of 6 windows with a last run of 4."""
    plan = _plan("single_server")
    n, cap = 300, 700
    assert max(1, cap // -(-32768 // n)) == 6 and cap % 6 == 4
    rng = np.random.default_rng(6)
    blk, counts = _hist_block(plan, rng, n, cap, _ticks(rng, n, cap), top=4)
    edges = np.arange(cap + 1)
    group = np.arange(n) % 5
    d = _Device(plan, blk, counts)
    try:
        got, _ = d.run(edges, 4, group, 5)
    finally:
        d.close()
    _equal(got, _want_one(plan, blk, counts, edges, 4, group, 5), "700 windows of one tick")


# ------------------------------------------------------------------------------------ 4. column chunking
def test_all_columns_of_a_wide_plan_with_1024_bins():
    """252 series and one of them once more with a second binning, 1 024 bins: 1 026 words a column, three columns a chunk."""
    plan = _wide_plan("wide_fanout50")
    S = plan.n_series
    assert S == 252
    rng = np.random.default_rng(1024)
    blk, counts = _hist_block(plan, rng, N, CAP, _ticks(rng, N, CAP), top=1024)
    columns = np.concatenate([np.arange(S), [5]])
    lo, width = np.zeros(S + 1), np.ones(S + 1)
    lo[-1], width[-1] = 100.0, 0.5
    edges = np.array([0, CAP])
    d = _Device(plan, blk, counts)
    try:
        got, _ = d.run(edges, 1024, None, 1, columns, lo, width)
        want = _want_one(plan, blk, counts, edges, 1024, None, 1, columns, lo, width)
        _equal(got, want, "253 columns of 1 024 bins")
        used = (want["hist"][0, 0] > 0).sum(axis=1)                                         # the bins are in use
        assert (want["hist"][0, 0].sum(axis=0) > 0).all() and used[:S].min() > 900 and used[S] > 400
        assert not np.array_equal(got["hist"][0, 0, 5], got["hist"][0, 0, -1]) and got["under"][0, 0, -1] > 0
        plain, _ = d.run(edges, 1024, None, 1)                                              # the NULL default: the same first 252 columns
        for k in ("hist", "under", "over"):
            assert plain[k].tobytes() == np.ascontiguousarray(got[k][:, :, :S]).tobytes(), k
    finally:
        d.close()


# ------------------------------------------------------------------------------------ 5. independence
def test_cells_do_not_depend_on_columns_batch_or_call():
    plan = _plan("lb_two_servers")
    S = plan.n_series
    rng = np.random.default_rng(5)
    n, cap = 8, 256
    blk, counts = _hist_block(plan, rng, n, cap, _ticks(rng, n, cap))
    big, big_counts = _hist_block(plan, rng, 8 * n, cap, rng.integers(0, cap + 1, 8 * n))
    where = np.arange(n) * 8 + 3
    big[where], big_counts[where] = blk, counts
    d, d_big = _Device(plan, blk, counts), _Device(plan, big, big_counts)
    singles = [_Device(plan, blk[s:s + 1], counts[s:s + 1]) for s in range(n)]
    lo, width = np.arange(S) % 3 - 1.0, np.array([WIDTHS[j % 5] for j in range(S)])
    perm = rng.permutation(S)
    try:
        for edges in (tick_window_edges(100, cap), tick_window_edges(7, cap), np.array([0, cap])):
            for group, G in ((np.arange(n), n), (np.arange(n) % 2, 2)):
                full, _ = d.run(edges, 16, group, G, None, lo, width)
                again, _ = d.run(edges, 16, group, G, None, lo, width)
                for k in OUTS:
                    assert full[k].tobytes() == again[k].tobytes(), k                                     # the same call twice
                for j in (0, 2, S - 1):                                                                   # a column alone
                    alone, _ = d.run(edges, 16, group, G, [j], lo[[j]], width[[j]])
                    for k in ("hist", "under", "over"):
                        assert alone[k].tobytes() == np.ascontiguousarray(full[k][:, :, j:j + 1]).tobytes(), (k, j)
                mixed, _ = d.run(edges, 16, group, G, perm, lo[perm], width[perm])                        # permuted among the others
                twice, _ = d.run(edges, 16, group, G, [3, 3, 1, 3], lo[[3, 3, 1, 3]], width[[3, 3, 1, 3]])   # and more than once
                for k in ("hist", "under", "over"):
                    assert mixed[k].tobytes() == np.ascontiguousarray(full[k][:, :, perm]).tobytes(), k
                    assert twice[k].tobytes() == np.ascontiguousarray(full[k][:, :, [3, 3, 1, 3]]).tobytes(), k
            single_groups = np.full(8 * n, -1)
            single_groups[where] = np.arange(n)
            full, _ = d.run(edges, 16, np.arange(n), n, None, lo, width)
            inside, _ = d_big.run(edges, 16, single_groups, n, None, lo, width)                           # elsewhere in a larger batch
            for k in OUTS:
                assert full[k].tobytes() == inside[k].tobytes(), k
            for s, one in enumerate(singles):                                                             # alone in a batch
                mine, _ = one.run(edges, 16, None, 1, None, lo, width)
                for k in OUTS:
                    assert mine[k][0].tobytes() == full[k][s].tobytes(), (k, s)
    finally:
        for x in (d, d_big, *singles):
            x.close()


# ------------------------------------------------------------------------------------ 6. NULL outputs, scratch
def test_null_outputs_are_skipped():
    plan = _plan("single_server")
    rng = np.random.default_rng(2)
    n, cap = 9, 300
    blk, counts = _hist_block(plan, rng, n, cap, _ticks(rng, n, cap))
    d = _Device(plan, blk, counts)
    try:
        for edges in (tick_window_edges(64, cap), tick_window_edges(9, cap)):
            full, _ = d.run(edges, 64, np.arange(n) % 2, 2, None, 1.0, 2.0)
            for outputs in (("hist",), ("hist", "count"), ("hist", "under"), ("hist", "over"), ("hist", "under", "over")):
                got, _ = d.run(edges, 64, np.arange(n) % 2, 2, None, 1.0, 2.0, outputs=outputs)   # (asserts that the guard words and the skipped outputs stay)
                assert set(got) == set(outputs)
                for k in got:
                    assert got[k].tobytes() == full[k].tobytes(), (outputs, k)
    finally:
        d.close()


def test_scratch_stays_within_the_bound_of_the_header():
    """include/asyncflow_hip.h: 4 B per edge + 4 B per series + 24 B per output column + 1 544 B -- no per-element and no
    per-cell records."""
    plan = _plan("fanout8")
    S = plan.n_series
    rng = np.random.default_rng(3)
    n, cap = 40, 400
    blk, counts = _hist_block(plan, rng, n, cap, rng.integers(0, cap + 1, n))
    for edges, columns in ((tick_window_edges(20, cap), None), (np.arange(cap + 1), np.arange(3 * S) % S)):
        d = _Device(plan, blk, counts)                                  # (a fresh engine: the scratch of this call alone)
        try:
            _, scratch = d.run(edges, 8, np.arange(n) % 7, 7, columns)
        finally:
            d.close()
        Cn = S if columns is None else len(columns)
        bound = 4 * len(edges) + 4 * S + 24 * Cn + 1544
        print(f"{len(edges) - 1} windows, {Cn} columns: scratch_bytes {scratch}, bound {bound}")
        assert 0 < scratch <= bound < 4 * n * (len(edges) - 1)


# ------------------------------------------------------------------------------------ 7. refusals
def test_device_argument_checks():
    """Error codes from calls that return before anything is written: no output word is touched."""
    import torch

    from asyncflow_amd.engine import PLAN_ONLY, Engine, load_library

    plan = _plan("lb_two_servers")
    S = plan.n_series
    rng = np.random.default_rng(1)
    blk, counts = _hist_block(plan, rng, 3, 50, [50, 20, 0])
    lib = load_library()
    dev = torch.device("cuda", 0)
    blk_t = torch.as_tensor(blk.view(np.int32), device=dev)
    counts_t = torch.as_tensor(counts.view(np.int32), device=dev)
    huge = counts.copy()
    huge[:, _abi.CNT_TICKS] = 0xFFFFFFFF
    huge_t = torch.as_tensor(huge.view(np.int32), device=dev)
    bad_group = torch.as_tensor(np.array([0, 2, 0], dtype=np.int32), device=dev)
    outs = torch.full((64 * 1024,), PATTERN, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    eng, planner = Engine(plan, 0), Engine(plan, PLAN_ONLY)
    pd, pu = C.POINTER(C.c_double), C.POINTER(C.c_uint32)
    try:
        def call(edges, bins=8, columns=None, n_columns=None, lo=None, width=None, samples=True, counts_p=counts_t, n_windows=None,
                 cap=50, engine=eng, n_groups=2, group=None, hist=True):
            e = (C.c_uint32 * len(edges))(*edges) if edges is not None else None
            col = (C.c_uint32 * len(columns))(*columns) if columns is not None else None
            lo_a = (C.c_double * len(lo))(*lo) if lo is not None else None
            wd_a = (C.c_double * len(width))(*width) if width is not None else None
            out = _abi.AfOutputs(0, None, cap, C.c_void_p(blk_t.data_ptr() if samples else None),
                                 C.c_void_p(counts_p.data_ptr() if counts_p is not None else None))
            req = _abi.AfSeriesHistogram(3, n_groups, (len(edges) - 1 if n_windows is None else n_windows), C.c_void_p(group.data_ptr() if group is not None else None),
                                         C.cast(e, pu) if e is not None else None, (len(columns) if columns is not None else 0) if n_columns is None else n_columns,
                                         C.cast(col, pu) if col is not None else None, bins, C.cast(lo_a, pd) if lo_a is not None else None,
                                         C.cast(wd_a, pd) if wd_a is not None else None, C.c_void_p(outs.data_ptr()),
                                         C.c_void_p(outs.data_ptr() + 4096) if hist else None, C.c_void_p(outs.data_ptr() + 128 * 1024),
                                         C.c_void_p(outs.data_ptr() + 192 * 1024), 0.0, 0)
            rc = lib.af_engine_summarize_series_histogram(engine._h, C.byref(out), C.byref(req))  # noqa: SLF001
            return rc, lib.af_last_error().decode()

        nan, inf = float("nan"), float("inf")
        ones, zeros = [1.0] * S, [0.0] * S
        INV, CAPACITY = _abi.AF_ERR_INVALID, _abi.AF_ERR_CAPACITY
        refused = [
            (call([0, 10], bins=0), INV, "n_bins"),
            (call([0, 10], bins=1025), INV, "n_bins"),
            (call([0, 10], lo=zeros, width=[1.0] * 5 + [0.0] + [1.0] * 6), INV, "width"),
            (call([0, 10], lo=zeros, width=[1.0] * 5 + [-1.0] + [1.0] * 6), INV, "width"),
            (call([0, 10], lo=zeros, width=[1.0] * 5 + [nan] + [1.0] * 6), INV, "width"),
            (call([0, 10], lo=zeros, width=[1.0] * 5 + [inf] + [1.0] * 6), INV, "width"),
            (call([0, 10], lo=[0.0] * 5 + [nan] + [0.0] * 6, width=ones), INV, "lo"),
            (call([0, 10], lo=[0.0] * 5 + [-inf] + [0.0] * 6, width=ones), INV, "lo"),
            (call([0, 10], lo=zeros), INV, "together"),
            (call([0, 10], width=ones), INV, "together"),
            (call(None, n_windows=1), INV, "tick_edges"),
            (call([0, 10, 10]), INV, "strictly increasing"),
            (call([10, 5]), INV, "strictly increasing"),
            (call([0], n_windows=0), INV, "n_windows"),
            (call([0, 10], columns=[0, S]), INV, "column"),
            (call([0, 10], columns=[0, 1], n_columns=0), INV, "columns and n_columns"),
            (call([0, 10], n_columns=2), INV, "columns and n_columns"),
            (call([0, 10], group=bad_group), INV, "group id out of range"),
            (call([0, 10], samples=False), INV, "samples"),
            (call([0, 10], counts_p=None), INV, "counts"),
            (call([0, 10], hist=False), INV, "hist"),
            (call([0, 0x7FFFFFFF], counts_p=huge_t, cap=0x7FFFFFFF, n_groups=1), CAPACITY, "2^32 or more"),
            (call([0, 10], n_groups=0xFFFFFFFF), CAPACITY, "2^32 - 1"),
            (call([0, 10], cap=0x80000000), CAPACITY, "2^31"),
            (call([0, 10], engine=planner), _abi.AF_ERR_NO_DEVICE, "planning-only"),
        ]
        for i, ((rc, msg), code, reason) in enumerate(refused):
            assert rc == code and reason in msg, (i, rc, msg, code, reason)
        torch.cuda.synchronize(dev)
        assert (outs.cpu().numpy().view(np.uint32) == PATTERN).all(), "a refused call touched an output"
        assert call([0, 10], n_groups=1)[0] == _abi.AF_OK
        host = outs.cpu().numpy().view(np.uint32)
        assert host[0] == 10 + 10 + 0 and host[1] == PATTERN and host[1024:1024 + S * 8].sum() + host[32 * 1024:32 * 1024 + S].sum() + host[48 * 1024:48 * 1024 + S].sum() == 20 * S
    finally:
        eng.close()
        planner.close()


# ------------------------------------------------------------------------------------ 8. through the Python API
@pytest.fixture(scope="module")
def event_run():
    from asyncflow_amd.runner import SimulationRunner

    payload = lb_with_events(horizon=60, scale=0.1)
    seeds = 0xE7C50000 + np.arange(12, dtype=np.uint64)
    res = SimulationRunner(simulation_input=payload, seeds=seeds).run()
    return res, np.arange(12) % 3


def _host_groups(res, ids, n_groups, edges, bins, series=None, lo=None, width=None):
    """get_series_histogram of every scenario, the members of every group added up; and the first scenario's own result."""
    per = [res[s].get_series_histogram(bins, tick_edges=edges, series=series, lo=lo, width=width) for s in range(len(res))]
    out = {k: np.zeros((n_groups,) + per[0][k].shape, dtype=np.int64) for k in OUTS}
    for s, one in enumerate(per):
        for k in OUTS:
            out[k][ids[s]] += one[k]
    return out, per[0]


def test_event_workload_through_the_python_api(event_run):
    res, ids = event_run
    names = res.series_names()
    period = res.plan.sample_period
    edges = np.array([0, int(round(18.0 / period)), int(round(24.0 / period)), res.plan.tick_count, res.plan.tick_count + 40])
    a = res.series_histogram_summary(64, tick_edges=edges, by=ids)
    want, one = _host_groups(res, ids, 3, edges, 64)
    assert a["series"] == names and np.array_equal(a["tick_edges"], edges) and a["replicas"].tolist() == [4, 4, 4]
    assert np.array_equal(a["times"], edges[:-1] * period) and np.array_equal(a["bin_edges"], one["bin_edges"]) and np.array_equal(a["ram"], one["ram"])
    assert tuple(a["hist"].shape) == (3, 4, len(names), 64) and a["series_histogram_ms"] > 0 and a["scratch_bytes"] > 0
    for k in OUTS:
        got = a[k].cpu().numpy()
        assert got.dtype == np.int64 and np.array_equal(got, want[k]), k
    assert (want["count"][:, 3] == 0).all() and want["hist"].sum() > 0
    # names, a binning by name, a scalar, the same series twice; windows in seconds
    queue = [k for k in names if k.endswith("ready_queue_len")]
    sel = [queue[0], names[0], queue[0]]
    b = res.series_histogram_summary(16, 6.0, by=ids, series=sel, lo={queue[0]: 1.0}, width=2.0)
    tick6 = tick_window_edges(int(round(6.0 / period)), res.plan.tick_count)
    col = [names.index(k) for k in sel]
    want_b, _ = _host_groups(res, ids, 3, tick6, 16, col, [1.0, 0.0, 1.0], 2.0)
    assert b["series"] == sel and np.array_equal(b["tick_edges"], tick6) and np.array_equal(b["bin_edges"][1], 2.0 * np.arange(17))
    for k in OUTS:
        assert np.array_equal(b[k].cpu().numpy(), want_b[k]), k
    per_scenario = res.series_histogram_summary(64, tick_edges=edges, by="scenario", series=queue)
    assert tuple(per_scenario["hist"].shape) == (12, 4, len(queue), 64)
    # quantiles off the histogram are the exact quantiles of the series
    levels = (0.5, 0.95, 0.99)
    h = res.series_histogram_summary(1024, tick_edges=edges, by=ids, series=queue)
    assert int(h["over"].sum()) == 0 and int(h["under"].sum()) == 0
    exact = res.series_quantile_summary(levels, tick_edges=edges, by=ids, series=queue)
    got_q = series_histogram_quantiles(h, levels)
    assert got_q.shape == tuple(exact["quantiles"].shape) == (3, 4, len(queue), 3)
    exact_q = exact["quantiles"].cpu().numpy()
    full = ~np.isnan(exact_q)
    assert np.array_equal(np.isnan(got_q), ~full) and got_q[full].tobytes() == exact_q[full].tobytes()      # bit for bit
    assert np.isnan(got_q[:, 3]).all() and full[:, :3].all()
    with pytest.raises(ValueError, match="ram_in_use"):
        series_histogram_quantiles(a, levels)


def test_bands_over_the_replicas(event_run):
    res, ids = event_run
    names = res.series_names()
    queue = [k for k in names if k.endswith("ready_queue_len")]
    edges = tick_window_edges(int(round(20.0 / res.plan.sample_period)), res.plan.tick_count)
    W = len(edges) - 1
    bands = res.series_histogram_bands(16, tick_edges=edges, by=ids, series=queue, level=0.9, q=(0.1, 0.75))
    for k in ("mean", "std", "ci_halfwidth", "q_lo", "q_hi", "pooled"):
        assert bands[k].shape == (3, W, len(queue), 16), k
    assert bands["n"].shape == (3, W) and (bands["n"] == 4).all() and bands["replicas"].tolist() == [4, 4, 4]
    assert bands["series"] == queue and np.array_equal(bands["tick_edges"], edges) and bands["bin_edges"].shape == (len(queue), 17)
    col = [names.index(k) for k in queue]
    want, _ = _host_groups(res, ids, 3, edges, 16, col)
    assert np.array_equal(bands["pooled"], want["hist"]) and np.array_equal(bands["pooled_count"], want["count"])
    assert np.array_equal(bands["pooled_under"], want["under"]) and np.array_equal(bands["pooled_over"], want["over"])
    per, _ = _host_groups(res, np.arange(12), 12, edges, 16, col)
    share = per["hist"] / per["count"][:, :, None, None]
    for g in range(3):
        members = share[ids == g]
        np.testing.assert_allclose(bands["mean"][g], members.mean(axis=0), rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(bands["q_lo"][g], np.quantile(members, 0.1, axis=0), rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(bands["q_hi"][g], np.quantile(members, 0.75, axis=0), rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("ext", ["npz", "parquet"])
def test_save_series_histogram_summary(event_run, tmp_path, ext):
    if ext == "parquet":
        pytest.importorskip("pyarrow")
    res, ids = event_run
    names = res.series_names()
    queue = [k for k in names if k.endswith("ready_queue_len")]
    path = str(tmp_path / f"series_hist.{ext}")
    written = res.save_series_histogram_summary(path, ids, bins=32, series=queue, width={queue[0]: 2.0}, window_s=20.0)
    back = load_summary(path)
    assert set(back) == set(written)
    for k, v in written.items():
        assert np.array_equal(np.asarray(back[k], dtype=v.dtype), v), k
    edges = tick_window_edges(int(round(20.0 / res.plan.sample_period)), res.plan.tick_count)
    want, _ = _host_groups(res, ids, 3, edges, 32, [names.index(k) for k in queue], None, [2.0] + [1.0] * (len(queue) - 1))
    assert back["replicas"].tolist() == [4, 4, 4] and np.array_equal(back["series_hist_count"], want["count"])
    for c, name in enumerate(queue):
        assert np.array_equal(back[f"series_hist:{name}"], want["hist"][:, :, c]) and back[f"series_hist:{name}"].shape == (3, len(edges) - 1, 32)
        assert np.array_equal(back[f"series_hist_under:{name}"], want["under"][:, :, c])
        assert np.array_equal(back[f"series_hist_over:{name}"], want["over"][:, :, c])
        assert np.array_equal(back[f"series_hist_bin_edges:{name}"], (2.0 if c == 0 else 1.0) * np.arange(33))
    assert np.array_equal(back["series_hist_tick_edges"], edges)
    assert np.array_equal(back["series_hist_times"], edges[:-1] * res.plan.sample_period)
