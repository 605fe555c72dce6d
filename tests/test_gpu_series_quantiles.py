"""Exact quantiles of the sampled series per (group, window of ticks, series) on the MI355X
(af_engine_summarize_series_quantiles): synthetic sample blocks handed straight to the entry -- the padding words and the
rows at and past a scenario's ticks filled with 0xFFFFFFFF -- against the host definition (results.series_window_quantiles on
the members' rows side by side) BIT for bit, NaN positions included.

The tiers of the implementation (asyncflow_amd/csrc/af_series_quantiles.hpp):
    small   a cell of at most SMALL_MAX = 2 048 values per column is sorted in LDS;
    large   every other cell: radix select of key - minkey, 11 bits a level; a column whose keys span fewer than 2^11 values is
            done after ONE histogram pass, 2^22 after two, wider ones after three.  The large cells run in CHUNKS of
            max(1, 128 MiB / (U * (2 Q * 8 208 + 12) B)) cells (U distinct selected series, Q levels).
So the sizes at which the code takes another path are 2 047 / 2 048 / 2 049 values a cell, key ranges 2 047 / 2 048 / 2 049 and
2^22 + 1, and one / several chunks."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from asyncflow_amd import _abi
from asyncflow_amd.results import series_window_quantiles, tick_window_edges
from oracle.scenarios import lb_two_servers, lb_with_events
from tests.test_gpu_series_windows import _block, _plan, _signed_block, _ticks, _wide_plan, ram_columns

pytestmark = pytest.mark.gpu

SMALL_MAX = 2048
HIST_BUDGET = 128 << 20
FILL = 0xFFFFFFFF
LEVELS = (0.0, 0.001, 0.5, 0.95, 0.999, 1.0)
PATTERN = 0x5A5A5A5A


def _filled(plan, blk, counts):
    """The block with 0xFFFFFFFF in every padding word and in every row at or past a scenario's min(ticks, capacity): a word
    the analyzer must never read -- as a key it would be the largest of its cell."""
    blk = blk.copy()
    blk[:, :, plan.n_series:] = FILL
    for s in range(blk.shape[0]):
        blk[s, min(int(counts[s, _abi.CNT_TICKS]), blk.shape[1]):] = FILL
    return blk


def _make(plan, rng, n, cap, ticks, kind="block", **kw):
    blk, counts = (_block if kind == "block" else _signed_block)(plan, rng, n, cap, ticks, **kw)
    return _filled(plan, blk, counts), counts


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

    def group_tensor(self, group):
        if group is None:
            return None
        g = np.asarray(group, dtype=np.int64)
        return self.torch.as_tensor(np.where(g < 0, _abi.POOL_SKIP, g).astype(np.uint32).view(np.int32), device=self.dev)

    def run(self, group, n_groups, edges, levels=LEVELS, columns=None, with_count=True):
        """count [G, W], quantiles [G, W, C, Q], scratch_bytes; both outputs lie in one buffer between sentinels."""
        torch = self.torch
        W, Q = len(edges) - 1, len(levels)
        Cn = self.plan.n_series if columns is None else len(columns)
        cells, guard = n_groups * W, 64
        n_q = 2 * cells * Cn * Q
        o_count, o_q = guard, guard + cells + guard + cells % 2
        total = o_q + n_q + guard
        buf = torch.full((total,), PATTERN, dtype=torch.int32, device=self.dev)
        grp_t = self.group_tensor(group)
        _, scratch = self.eng.summarize_series_quantiles(
            self.n, n_groups, edges, levels, samples_ptr=self.blk_t.data_ptr(), tick_capacity=self.cap,
            counts_ptr=self.counts_t.data_ptr(), quantiles_ptr=buf.data_ptr() + 4 * o_q,
            count_ptr=buf.data_ptr() + 4 * o_count if with_count else 0, group_ptr=grp_t.data_ptr() if grp_t is not None else 0,
            columns=columns)
        host = buf.cpu().numpy()
        written = np.zeros(total, dtype=bool)
        written[o_q:o_q + n_q] = True
        if with_count:
            written[o_count:o_count + cells] = True
        assert (host[~written] == PATTERN).all(), "a word outside the requested outputs was written"
        count = host[o_count:o_count + cells].view(np.uint32).reshape(n_groups, W) if with_count else None
        return count, host[o_q:o_q + n_q].view(np.float64).reshape(n_groups, W, Cn, Q), scratch


def _host(plan, blk, counts, group, n_groups, edges, levels=LEVELS, columns=None):
    """The host definition on every cell: the members' window rows side by side, in scenario order."""
    n, cap, _ = blk.shape
    S = plan.n_series
    b = np.asarray(edges, dtype=np.int64)
    W, Q = len(b) - 1, len(levels)
    Cn = S if columns is None else len(columns)
    group = np.zeros(n, dtype=np.int64) if group is None else np.asarray(group)
    words = [np.ascontiguousarray(blk[s, :min(int(counts[s, _abi.CNT_TICKS]), cap), :S].T) for s in range(n)]
    count = np.zeros((n_groups, W), dtype=np.int64)
    quant = np.full((n_groups, W, Cn, Q), np.nan)
    for g in range(n_groups):
        members = np.nonzero(group == g)[0]
        if len(members) == 1:
            count[g], quant[g] = series_window_quantiles(words[members[0]], b, plan.n_edges, levels, columns)
            continue
        for w in range(W):
            seg = [words[s][:, min(b[w], words[s].shape[1]):min(b[w + 1], words[s].shape[1])] for s in members]
            cell = np.concatenate(seg, axis=1) if seg else np.zeros((S, 0), dtype=np.uint32)
            c, q = series_window_quantiles(cell, [0, max(cell.shape[1], 1)], plan.n_edges, levels, columns)
            count[g, w], quant[g, w] = c[0], q[0]
    return count, quant


def _same_bits(got, want, what):
    """Bit for bit; a NaN only where the other has one."""
    assert got.shape == want.shape, what
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    assert np.array_equal(nan_g, nan_w), (what, "NaN positions", np.argwhere(nan_g != nan_w)[:5])
    differ = (got.view(np.uint64) != want.view(np.uint64)) & ~nan_w
    assert not differ.any(), (what, np.argwhere(differ)[:5], got[differ][:5], want[differ][:5])


def _check(d, blk, counts, group, n_groups, edges, what, levels=LEVELS, columns=None):
    count, quant, scratch = d.run(group, n_groups, edges, levels, columns)
    want_count, want = _host(d.plan, blk, counts, group, n_groups, edges, levels, columns)
    assert np.array_equal(count, want_count.astype(np.uint32)), what
    _same_bits(quant, want, what)
    return count, quant, scratch


# ------------------------------------------------------------------------------------ 1. plans, groupings, windows
def _plans(name):
    return _wide_plan(name) if name.startswith("wide") else _plan(name)


def _three_groupings(n):
    uneven = np.array([0 if i % 5 < 3 else 1 if i % 5 == 3 else 3 for i in range(n)])     # group 2 is empty
    uneven[4] = -1                                                                          # one scenario is left out
    return [(np.arange(n), n, "singletons"), (uneven, 4, "three uneven groups"), (None, 1, "one group")]


@pytest.mark.parametrize("name", ["single_server", "lb_two_servers", "fanout8", "wide_fanout51"])
def test_plans_groupings_and_windows_equal_the_host_definition(name):
    plan = _plans(name)
    wide = name.startswith("wide")
    assert wide == (plan.series_pitch > 256)
    rng = np.random.default_rng(len(name))
    n, cap = (7, 500) if wide else (23, 700)
    ticks = _ticks(rng, n, cap)                                           # 0, cap, cap + 50, 1 and random ones
    ticks[-3:] = cap - np.arange(3)                                       # enough rows for a large cell whatever the draw
    assert np.minimum(ticks, cap).sum() > SMALL_MAX
    blk, counts = _make(plan, rng, n, cap, ticks, "signed")
    d = _Device(plan, blk, counts)
    try:
        uneven = np.array([0, 1, 2, 40, 41, 300, cap - 1, 5 * cap])
        sizes = set()
        for wname, edges in (("one window", np.array([0, cap])), ("7 uneven windows", uneven), ("one tick each", np.arange(151))):
            for group, n_groups, gname in _three_groupings(n):
                count, _, _ = _check(d, blk, counts, group, n_groups, edges, f"{name}, {wname}, {gname}")
                sizes |= {"small" if c <= SMALL_MAX else "large" for c in count.ravel()}
        assert sizes == {"small", "large"}
    finally:
        d.close()


def test_wide_plan_in_several_chunks():
    """257 series and 16 levels: 257 * (32 * 8 208 + 12) B = 67.5 MB of histograms a cell, one large cell a chunk."""
    plan = _wide_plan("wide_fanout51")
    assert plan.n_series == 257 and HIST_BUDGET // (257 * (32 * 8208 + 12)) == 1
    rng = np.random.default_rng(51)
    n, cap = 6, 1200
    blk, counts = _make(plan, rng, n, cap, [1200, 1100, 1200, 1150, 1200, 1000], "signed")
    levels = np.linspace(0.0, 1.0, 16)
    d = _Device(plan, blk, counts)
    try:
        count, _, _ = _check(d, blk, counts, np.array([0, 0, 1, 1, 2, 2]), 3, np.array([0, 1100, 1200]), "six cells", levels)
        assert (count[:, 0] > SMALL_MAX).all() and (count[:, 1] <= SMALL_MAX).all()
    finally:
        d.close()


# ------------------------------------------------------------------------------------ 2. cell sizes
def test_cell_sizes_at_the_tier_boundary_by_window_length():
    """One scenario; windows of 2 047, 2 048, 2 049, 1, 2 and 0 values."""
    plan = _plan("lb_two_servers")
    rng = np.random.default_rng(2)
    lengths = [SMALL_MAX - 1, SMALL_MAX, SMALL_MAX + 1, 1, 2]
    edges = np.concatenate([[0], np.cumsum(lengths), [sum(lengths) + 7]])
    cap = int(edges[-2])
    blk, counts = _make(plan, rng, 2, cap, [cap, 0], "signed")
    d = _Device(plan, blk, counts)
    try:
        count, quant, _ = _check(d, blk, counts, np.arange(2), 2, edges, "by window length")
        assert count[0].tolist() == lengths + [0] and (count[1] == 0).all()
        assert np.isnan(quant[0, -1]).all() and np.isnan(quant[1]).all()
    finally:
        d.close()


def test_cell_sizes_at_the_tier_boundary_by_member_count():
    """192 scenarios of 31 to 33 ticks: groups of 64 members with 2 047, 2 048 and 2 049 values in one window; and groups of
    one, two and no values."""
    plan = _plan("single_server")
    rng = np.random.default_rng(3)
    n, cap = 196, 33
    ticks = np.full(n, 32)
    ticks[0], ticks[128] = 31, 33
    ticks[192:] = [1, 1, 1, 0]
    group = np.concatenate([np.repeat([0, 1, 2], 64), [3, 4, 4, 5]])
    blk, counts = _make(plan, rng, n, cap, ticks, "signed", dyadic=False)   # (ram values of either sign over many binades)
    d = _Device(plan, blk, counts)
    try:
        count, quant, _ = _check(d, blk, counts, group, 6, np.array([0, cap]), "by member count")
        assert count[:, 0].tolist() == [SMALL_MAX - 1, SMALL_MAX, SMALL_MAX + 1, 1, 2, 0] and np.isnan(quant[5]).all()
        _check(d, blk, counts, group, 6, np.array([0, 16, cap]), "by member count, two windows")
    finally:
        d.close()


# ------------------------------------------------------------------------------------ 3. key ranges
def _key_range_block(rng, n, cap):
    """fanout8 (26 integer columns after the edges' ..., 8 ram columns): every column of a kind that drives the select."""
    plan = _plan("fanout8")
    S = plan.n_series
    ram = np.nonzero(ram_columns(S, plan.n_edges))[0]
    ints = np.nonzero(~ram_columns(S, plan.n_edges))[0]
    blk, counts = _block(plan, rng, n, cap, np.full(n, cap))
    shape = (n, cap)
    kinds = {}

    def spread(base, span):   # both ends occur: the range is exactly span
        v = base + rng.integers(0, span + 1, shape)
        v[0, 0], v[-1, -1] = base, base + span
        return v.astype(np.uint32)

    int_kinds = [("all equal", lambda: np.full(shape, 123456, dtype=np.uint32)),
                 ("range 2047", lambda: spread(1000, 2047)), ("range 2048", lambda: spread(1000, 2048)),
                 ("range 2049", lambda: spread(2 ** 31 - 1024, 2049)), ("range 2^22 + 1", lambda: spread(17, 2 ** 22 + 1)),
                 ("words >= 2^31", lambda: spread(2 ** 31, 2 ** 31 - 1)),
                 ("many equal at the wanted rank", lambda: np.where(rng.random(shape) < 0.6, np.uint32(3_000_000), spread(17, 2 ** 23)))]
    for i, (kname, make) in enumerate(int_kinds):
        blk[:, :, ints[i]] = make()
        kinds[kname] = int(ints[i])

    def f32(v):
        return np.asarray(v, dtype=np.float32).view(np.uint32)

    zeros = np.where(rng.random(shape) < 0.5, np.float32(0.0), np.float32(-0.0))
    mixed = (rng.integers(-2 ** 10, 2 ** 10, shape) / 256.0).astype(np.float32)
    u = rng.random(shape)
    mixed[u < 0.2], mixed[u > 0.8] = np.float32(0.0), np.float32(-0.0)
    residues = (rng.integers(0, 2 ** 16, shape) / 256.0 + 0.5).astype(np.float32)
    residues[rng.random(shape) < 0.3] = np.float32(-2.842171e-14)
    ram_kinds = [("dyadic", f32(rng.integers(0, 2 ** 24, shape) / 256.0)), ("negative residues", f32(residues)),
                 ("both zeros only", f32(zeros)), ("both zeros among values", f32(mixed)),
                 ("arbitrary floats", f32(10.0 ** rng.uniform(-20, 20, shape) * rng.choice([-1.0, 1.0], shape)))]
    for i, (kname, v) in enumerate(ram_kinds):
        blk[:, :, ram[i]] = v
        kinds[kname] = int(ram[i])
    return plan, _filled(plan, blk, counts), counts, kinds


def test_key_ranges_that_drive_the_select():
    rng = np.random.default_rng(33)
    n, cap = 8, 1200
    plan, blk, counts, kinds = _key_range_block(rng, n, cap)
    col = blk[:, :, kinds["many equal at the wanted rank"]]
    assert (col == 3_000_000).sum() > 512 * 8                                       # more than afs::kCand equal values around the median
    assert int(col.max()) - int(col.min()) > 2 ** 22
    for kname, span in (("range 2047", 2047), ("range 2048", 2048), ("range 2049", 2049), ("range 2^22 + 1", 2 ** 22 + 1)):
        c = blk[:, :, kinds[kname]].astype(np.int64)
        assert c.max() - c.min() == span, kname
    assert (blk[:, :, kinds["words >= 2^31"]] >= 2 ** 31).all()
    d = _Device(plan, blk, counts)
    try:
        for group, n_groups, gname in ((None, 1, "one group"), (np.arange(n) % 2, 2, "two groups"), (np.arange(n), n, "singletons")):
            for edges in (np.array([0, cap]), np.array([0, 700, cap])):
                count, quant, _ = _check(d, blk, counts, group, n_groups, edges, f"key ranges, {gname}, {len(edges) - 1} windows")
                assert (count.max() > SMALL_MAX) == (gname != "singletons")
        # one column alone, the levels that meet the equal values
        for kname, j in kinds.items():
            _check(d, blk, counts, None, 1, np.array([0, cap]), kname, (0.3, 0.5, 0.7), [j])
    finally:
        d.close()


# ------------------------------------------------------------------------------------ 4. the other series analyzers
def test_cross_checks_with_the_series_window_analyzer_and_the_whole_run_summary():
    import torch

    from tests.test_gpu_analyzer_synthetic import _series

    plan = _plan("lb_two_servers")
    S = plan.n_series
    ram = ram_columns(S, plan.n_edges)
    rng = np.random.default_rng(4)
    n, cap = 12, 900
    blk, counts = _make(plan, rng, n, cap, _ticks(rng, n, cap), "signed")

    def decode(words):
        return np.where(ram, words.view(np.float32).astype(np.float64), words.astype(np.float64))

    d = _Device(plan, blk, counts)
    try:
        for group, n_groups in ((None, 1), (np.arange(n) % 3, 3), (np.arange(n), n)):
            for edges in (np.array([0, cap]), tick_window_edges(128, cap)):
                W = len(edges) - 1
                count, quant, _ = d.run(group, n_groups, edges, (0.0, 1.0))
                outs = {k: torch.zeros((n_groups, W, S), dtype=torch.int32, device=d.dev) for k in ("min", "max")}
                cnt = torch.zeros((n_groups, W), dtype=torch.int32, device=d.dev)
                mean = torch.zeros((n_groups, W, S), dtype=torch.float64, device=d.dev)
                grp_t = d.group_tensor(group)
                d.eng.summarize_series_windows(n, n_groups, edges, samples_ptr=d.blk_t.data_ptr(), tick_capacity=cap,
                                               counts_ptr=d.counts_t.data_ptr(), count_ptr=cnt.data_ptr(), mean_ptr=mean.data_ptr(),
                                               min_ptr=outs["min"].data_ptr(), max_ptr=outs["max"].data_ptr(),
                                               group_ptr=grp_t.data_ptr() if grp_t is not None else 0)
                assert np.array_equal(count, cnt.cpu().numpy().view(np.uint32))
                live = count > 0
                mn, mx = (decode(outs[k].cpu().numpy().view(np.uint32)) for k in ("min", "max"))
                assert (quant[live][:, :, 0] == mn[live]).all() and (quant[live][:, :, 1] == mx[live]).all()
                assert np.isnan(quant[~live]).all()
        # a single scenario, one window, level 1: the whole-run series_max
        whole = _series(plan, _filled(plan, blk, counts), counts, want=("series_max",))["series_max"]
        _, quant, _ = d.run(np.arange(n), n, np.array([0, cap]), (1.0,))
        some = np.minimum(counts[:, _abi.CNT_TICKS], cap) > 0
        assert (quant[some, 0, :, 0] == decode(whole.view(np.uint32))[some]).all() and some.sum() == n - 1
    finally:
        d.close()


# ------------------------------------------------------------------------------------ 5. independence
def test_a_cell_does_not_depend_on_the_rest_of_the_call():
    plan = _plan("lb_two_servers")
    S = plan.n_series
    rng = np.random.default_rng(5)
    n, cap = 10, 1000
    ticks = _ticks(rng, n, cap)                                           # 0, cap, cap + 50, 1 ...
    ticks[4:] = cap - rng.integers(0, 50, n - 4)                          # ... and six nearly full ones
    blk, counts = _make(plan, rng, n, cap, ticks, "block", dyadic=False)
    group = np.arange(n) % 3                                              # groups 1 and 2 hold over 2 600 values in the second window: large
    edges = np.array([0, 100, cap])
    d = _Device(plan, blk, counts)
    try:
        count, base, _ = _check(d, blk, counts, group, 3, edges, "base")
        assert count.max() > SMALL_MAX and count.min() <= SMALL_MAX
        _, again, _ = d.run(group, 3, edges)
        assert again.tobytes() == base.tobytes()                          # two runs of one call
        # levels: a permutation with a duplicate, a subset
        perm = [5, 2, 2, 0, 4, 1, 3]
        _, got, _ = d.run(group, 3, edges, [LEVELS[i] for i in perm])
        assert got.tobytes() == np.ascontiguousarray(base[:, :, :, perm]).tobytes()
        _, got, _ = d.run(group, 3, edges, [LEVELS[3]])
        assert got.tobytes() == np.ascontiguousarray(base[:, :, :, 3:4]).tobytes()
        # columns: a permutation with duplicates, one column, without count
        cols = [S - 1, 0, 5, S - 1, 8, 5]
        _, got, _ = d.run(group, 3, edges, columns=cols, with_count=False)
        assert got.tobytes() == np.ascontiguousarray(base[:, :, cols]).tobytes()
        _, got, _ = d.run(group, 3, edges, [LEVELS[1], LEVELS[4]], columns=[7])
        assert got.tobytes() == np.ascontiguousarray(base[:, :, 7:8][:, :, :, [1, 4]]).tobytes()
        # regrouped: group 1 alone, under another id and beside other groups
        regroup = np.where(group == 1, 4, np.where(group == 0, -1, 0))
        _, got, _ = d.run(regroup, 5, edges)
        assert got[4].tobytes() == base[1].tobytes() and np.isnan(got[1:4]).all()
        # another window count: the third window is the same (large) cell as the second was, the last one is empty
        _, got, _ = d.run(group, 3, np.array([0, 40, 100, cap, cap + 5]))
        assert np.ascontiguousarray(got[:, 2]).tobytes() == np.ascontiguousarray(base[:, 1]).tobytes() and np.isnan(got[:, 3]).all()
    finally:
        d.close()
    # the same scenarios inside a batch six times as large
    big, big_counts = _make(plan, rng, 6 * n, cap, rng.integers(0, cap + 1, 6 * n), "block", dyadic=False)
    where = np.arange(n) * 6 + 2
    big[where], big_counts[where] = blk, counts
    big_group = np.full(6 * n, -1)
    big_group[where] = group
    big_group[big_group < 0] = 3 + np.arange(5 * n) % 2
    d = _Device(plan, big, big_counts)
    try:
        _, got, _ = d.run(big_group, 5, edges)
        assert np.ascontiguousarray(got[:3]).tobytes() == base.tobytes()
    finally:
        d.close()


# ------------------------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_outputs_alone():
    import torch

    from asyncflow_amd.engine import Engine, load_library

    plan = _plan("lb_two_servers")
    S = plan.n_series
    rng = np.random.default_rng(6)
    blk, counts = _make(plan, rng, 3, 50, [50, 20, 0])
    lib = load_library()
    dev = torch.device("cuda", 0)
    blk_t = torch.as_tensor(blk.view(np.int32), device=dev)
    counts_t = torch.as_tensor(counts.view(np.int32), device=dev)
    outs = torch.full((8192,), PATTERN, dtype=torch.int32, device=dev)
    grp_bad = torch.as_tensor(np.array([0, 2, 0], dtype=np.int32), device=dev)
    long_counts = counts.copy()                                           # three scenarios of 2^31 - 1 ticks each: the host sizes the
    long_counts[:, _abi.CNT_TICKS] = 2 ** 31 - 1                          # cells from the counts and refuses before any row is read
    long_t = torch.as_tensor(long_counts.view(np.int32), device=dev)
    eng = Engine(plan, 0)
    plan_only = Engine(plan, _abi.DEVICE_PLAN_ONLY)
    try:
        def call(edges=(0, 10), levels=(0.5,), columns=None, n_columns=None, samples=True, n_groups=1, n_windows=None, n_levels=None,
                 group=None, cap=50, engine=eng, counts_t=counts_t):
            e = (C.c_uint32 * len(edges))(*edges)
            q = (C.c_double * max(len(levels), 1))(*levels)
            c = (C.c_uint32 * len(columns))(*columns) if columns is not None else None
            out = _abi.AfOutputs(0, None, cap, C.c_void_p(blk_t.data_ptr() if samples else None), C.c_void_p(counts_t.data_ptr()))
            req = _abi.AfSeriesQuantiles(3, n_groups, len(edges) - 1 if n_windows is None else n_windows,
                                         C.c_void_p(group.data_ptr()) if group is not None else None, e,
                                         len(levels) if n_levels is None else n_levels, q,
                                         (len(columns) if columns is not None else 0) if n_columns is None else n_columns, c,
                                         C.c_void_p(outs.data_ptr()), C.c_void_p(outs.data_ptr() + 1024), 0.0, 0)
            rc = lib.af_engine_summarize_series_quantiles(engine._h, C.byref(out), C.byref(req))  # noqa: SLF001
            return rc, lib.af_last_error().decode()

        invalid = [dict(levels=(), n_levels=0), dict(levels=tuple(np.linspace(0, 1, 17))), dict(levels=(float("nan"),)),
                   dict(levels=(0.5, 1.0000001)), dict(levels=(-1e-9,)), dict(edges=(0, 10, 10)), dict(edges=(10, 5)),
                   dict(edges=(0,), n_windows=0), dict(columns=(0, S)), dict(columns=(1,), n_columns=0), dict(n_columns=2),
                   dict(group=grp_bad, n_groups=2), dict(samples=False)]
        for kw in invalid:
            rc, msg = call(**kw)
            assert rc == _abi.AF_ERR_INVALID and msg, kw
        # a cell of 3 * (2^31 - 1) >= 2^32 values: one group, one window over a capacity of 2^31 - 1 ticks
        huge_cell = dict(counts_t=long_t, cap=2 ** 31 - 1, edges=(0, 2 ** 31 - 1))
        for kw, text in ((dict(n_groups=0xFFFFFFFF), "2^32 - 1"), (dict(cap=0x80000000), "2^31"), (huge_cell, "2^32 or more samples")):
            rc, msg = call(**kw)
            assert rc == _abi.AF_ERR_CAPACITY and text in msg, (kw, msg)
        assert call(engine=plan_only)[0] == _abi.AF_ERR_NO_DEVICE
        assert (outs.cpu().numpy() == PATTERN).all(), "a refused call wrote to an output"
        rc, msg = call()
        assert rc == _abi.AF_OK, msg
        host = outs.cpu().numpy()
        assert host[0] == 10 + 10 + 0 and (host[256:256 + 2 * S] != PATTERN).any()
    finally:
        eng.close()
        plan_only.close()


# ------------------------------------------------------------------------------------ 7. scratch
def _scratch_bound(plan, n, n_groups, n_win, n_levels, n_columns, n_distinct, n_small, n_large) -> int:
    """include/asyncflow_hip.h: 4 B per edge + 8 B per level + 4 B per group + 4 B per scenario + 5 B per padded series + 8 U +
    4 C + 8 B per cell of at most 2 048 values + 5 376 B of alignment, and only where L > 0: 4 B per cell + 8 L +
    min(L, max(1, floor(128 MiB / (U * K)))) * U * K, K = 2 * n_levels * 8 208 + 12."""
    bound = (4 * (n_win + 1) + 8 * n_levels + 4 * (n_groups + 1) + 4 * n + 5 * plan.series_pitch + 8 * n_distinct + 4 * n_columns
             + 8 * n_small + 5376)
    if n_large:
        k = 2 * n_levels * 8208 + 12
        bound += 4 * n_groups * n_win + 8 * n_large + min(n_large, max(1, HIST_BUDGET // (n_distinct * k))) * n_distinct * k
    return bound


def test_scratch_of_many_tiny_singleton_cells():
    """10^5 singleton cells of 0 to 5 values."""
    plan = _plan("single_server")
    S, n_edges = plan.n_series, plan.n_edges
    ram = ram_columns(S, n_edges)
    rng = np.random.default_rng(7)
    n, cap = 100_000, 5
    ticks = rng.integers(0, cap + 1, n)
    blk, counts = _make(plan, rng, n, cap, ticks)
    d = _Device(plan, blk, counts)
    try:
        count, quant, scratch = d.run(np.arange(n), n, np.array([0, cap]))
    finally:
        d.close()
    bound = _scratch_bound(plan, n, n, 1, len(LEVELS), S, S, n, 0)
    print(f"10^5 singleton cells: scratch_bytes {scratch}, bound {bound}")
    assert 0 < scratch <= bound < 2_000_000
    assert np.array_equal(count[:, 0], ticks)
    # the host definition, the scenarios of one tick count at a time: a column of k scenarios is k series of the definition
    # (n_edges = k: integer series; rows 2, 5, 8, ... of 3 k series without edges: ram_in_use)
    for m in range(cap + 1):
        idx = np.nonzero(ticks == m)[0]
        k = len(idx)
        assert k > 1000
        for j in range(S):
            col = blk[idx, :m, j]                                         # [k, m]
            if ram[j]:
                wide = np.zeros((3 * k, m), dtype=np.uint32)
                wide[2::3] = col
                _, want = series_window_quantiles(wide, [0, max(m, 1)], 0, LEVELS, np.arange(2, 3 * k, 3))
            else:
                _, want = series_window_quantiles(col, [0, max(m, 1)], k, LEVELS)
            _same_bits(np.ascontiguousarray(quant[idx, 0, j]), want[0], f"{m} ticks, series {j}")


def test_scratch_of_one_large_group():
    """One group of 64 x 1 501."""
    plan = _plan("lb_two_servers")
    S = plan.n_series
    rng = np.random.default_rng(8)
    n, cap = 64, 1501
    blk, counts = _make(plan, rng, n, cap, np.full(n, cap), "signed")
    d = _Device(plan, blk, counts)
    try:
        count, _, scratch = _check(d, blk, counts, None, 1, np.array([0, cap]), "64 x 1501")
    finally:
        d.close()
    bound = _scratch_bound(plan, n, 1, 1, len(LEVELS), S, S, 0, 1)
    print(f"one group of 64 x 1501: scratch_bytes {scratch}, bound {bound}")
    assert count[0, 0] == 64 * 1501 and S * 12 * 8192 <= scratch <= bound < 1_300_000


# ------------------------------------------------------------------------------------ 8. through the Python API
def _grid_run(which):
    from asyncflow_amd import expand_grid
    from asyncflow_amd.runner import SimulationRunner

    payload = lb_with_events(horizon=60, scale=0.1) if which == "lb_with_events" else lb_two_servers(horizon=20)
    users = "rqs_input.avg_active_users.mean"
    grid = expand_grid({users: [40.0, 120.0, 300.0], "topology_graph.edges[*].latency.mean": [0.002, 0.006]},
                       replicas=4, order_by_load=users)
    return SimulationRunner(simulation_input=payload, **grid.runner_kwargs()).run(), grid


def _api_cells(res, ids, n_groups, edges, levels, cols):
    W = len(edges) - 1
    count = np.zeros((n_groups, W), dtype=np.int64)
    quant = np.full((n_groups, W, len(cols), len(levels)), np.nan)
    words = [res[s]._samples for s in range(len(res))]  # noqa: SLF001
    for g in range(n_groups):
        members = np.nonzero(ids == g)[0]
        for w in range(W):
            seg = [words[s][:, min(edges[w], words[s].shape[1]):min(edges[w + 1], words[s].shape[1])] for s in members]
            cell = np.concatenate(seg, axis=1)
            c, q = series_window_quantiles(cell, [0, max(cell.shape[1], 1)], res.plan.n_edges, levels, cols)
            count[g, w], quant[g, w] = c[0], q[0]
    return count, quant


@pytest.mark.parametrize("which", ["lb_with_events", "lb_two_servers"])
def test_grid_through_the_python_api(which):
    from asyncflow_amd.results import window_bands_by_group

    res, grid = _grid_run(which)
    names = res.series_names()
    S = len(names)
    levels = (0.5, 0.95, 0.99)
    per_window = int(round(2.0 / res.plan.sample_period))
    edges = tick_window_edges(per_window, res.plan.tick_count)
    a = res.series_quantile_summary(levels, 2.0, by=grid)
    assert tuple(a["quantiles"].shape) == (6, len(edges) - 1, S, 3) and a["replicas"].tolist() == [4] * 6
    assert a["series"] == names and np.array_equal(a["tick_edges"], edges) and a["levels"].tolist() == list(levels)
    assert np.array_equal(a["times"], edges[:-1] * res.plan.sample_period) and a["scratch_bytes"] > 0 and a["series_quantile_ms"] > 0
    want_count, want = _api_cells(res, grid.point, 6, edges, levels, np.arange(S))
    assert np.array_equal(a["count"].cpu().numpy(), want_count)
    _same_bits(a["quantiles"].cpu().numpy(), want, f"{which}, by=grid")
    # a selection by name, in another order; one window over the run with a window past it: four replicas of lb_with_events
    # (60 s) make large cells, four of lb_two_servers (20 s: 1 596 values) small ones
    sel = [names[-1], names[0], names[7]]
    edges_b = np.array([0, res.plan.tick_count, res.plan.tick_count + 40])
    b = res.series_quantile_summary(levels, tick_edges=edges_b, by=grid, series=sel)
    assert b["series"] == sel and (int(b["count"].max()) > SMALL_MAX) == (which == "lb_with_events")
    want_count, want = _api_cells(res, grid.point, 6, edges_b, levels, np.array([S - 1, 0, 7]))
    assert np.array_equal(b["count"].cpu().numpy(), want_count)
    _same_bits(b["quantiles"].cpu().numpy(), want, f"{which}, selected series")
    assert np.isnan(b["quantiles"][:, 1].cpu().numpy()).all()
    # every scenario its own group is its own host definition
    per = res.series_quantile_summary(levels, ticks_per_window=per_window, by="scenario", series=[1, 8])
    got = per["quantiles"].cpu().numpy()
    for s in range(len(res)):
        host = res[s].get_series_window_quantiles(levels, 2.0, series=[1, 8])
        _same_bits(got[s], host["quantiles"], f"scenario {s}")
    # bands over the replicas
    bands = res.series_quantile_bands(levels, tick_edges=np.concatenate([edges, [edges[-1] + 40]]), by=grid, series=[1, 8], level=0.9, q=(0.1, 0.75))
    host_per = np.stack([res[s].get_series_window_quantiles(levels, tick_edges=bands["tick_edges"], series=[1, 8])["quantiles"] for s in range(len(res))])
    host_cnt = np.stack([res[s].get_series_window_quantiles(levels, tick_edges=bands["tick_edges"], series=[1, 8])["count"] for s in range(len(res))])
    import torch

    ref = window_bands_by_group(torch.as_tensor(host_per).flatten(2), grid.point, 6, 0.9, (0.1, 0.75), valid=torch.as_tensor(host_cnt > 0))
    for k in ("mean", "std", "ci_halfwidth", "q_lo", "q_hi"):
        assert bands[k].shape == (6, len(edges), 2, 3)
        assert np.array_equal(bands[k].reshape(6, len(edges), 6), ref[k], equal_nan=True), k
    assert np.array_equal(bands["n"], ref["n"]) and (bands["n"][:, -1] == 0).all() and (bands["n"][:, :-1] == 4).all()
    pooled = res.series_quantile_summary(levels, tick_edges=bands["tick_edges"], by=grid, series=[1, 8])
    assert np.array_equal(bands["pooled"], pooled["quantiles"].cpu().numpy(), equal_nan=True)
    assert np.array_equal(bands["pooled_count"], pooled["count"].cpu().numpy())


def _round_trip(path: str) -> None:
    from asyncflow_amd.results import load_summary

    res, grid = _grid_run("lb_with_events")
    names = res.series_names()
    levels = (0.5, 0.999)
    sel = [names[1], names[-1]]
    pooled = res.series_quantile_summary(levels, 2.0, by=grid, series=sel)
    written = res.save_series_quantile_summary(path, grid, levels=levels, series=sel, window_s=2.0)
    back = load_summary(path)
    assert set(back) == set(written)
    for k, v in written.items():
        assert np.array_equal(np.asarray(back[k], dtype=v.dtype), v, equal_nan=v.dtype.kind == "f"), k
    for k, v in grid.point_columns().items():
        assert np.array_equal(back[f"param:{k}"], v)
    quant = pooled["quantiles"].cpu().numpy()
    for c, sname in enumerate(sel):
        for i, lv in enumerate(levels):
            assert np.array_equal(back[f"series_quantile:{sname}:{lv!r}"], quant[:, :, c, i], equal_nan=True), (sname, lv)
    assert np.array_equal(back["series_quantile_count"], pooled["count"].cpu().numpy()) and back["replicas"].tolist() == [4] * 6
    assert np.array_equal(back["series_quantile_tick_edges"], pooled["tick_edges"])
    assert np.array_equal(back["series_quantile_times"], pooled["times"]) and back["series_quantile_levels"].tolist() == list(levels)


def test_save_series_quantile_summary_npz(tmp_path):
    _round_trip(str(tmp_path / "series_quantiles.npz"))


def test_save_series_quantile_summary_parquet(tmp_path):
    pytest.importorskip("pyarrow")
    _round_trip(str(tmp_path / "series_quantiles.parquet"))
