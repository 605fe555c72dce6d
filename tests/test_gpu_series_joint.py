"""Joint moments of pairs of the sampled series per (group, window of ticks, pair) on the MI355X
(af_engine_summarize_series_joint): synthetic sample blocks handed straight to the entry -- the padding words and the rows at
or past a scenario's ticks hold 0xFFFFFFFF, which shows as a wrong sum if it is read -- with every output in one buffer
between sentinels.  The reference is the host definition, results.series_joint_sums of every scenario, pooled over the members
of a group with Python integers.  Every output is an exact integer and is compared with ==.

n = 23 scenarios of capacity 700 (0 ticks, all, more than stored, 1 among them); the plans of 6, 12 and 42 series (rows staged
in LDS) and one of 262 (rows wider than the staging takes: both words from global memory) on every window shape and grouping;
lags 0, 1, 2, 63, 64, 65, 199, 200, 699, 700 and 5 000 -- in LDS while 64 + lag rows fit a wave's share, from global memory
beyond --; a column with itself, two columns of one 16-byte group, the first and the last integer column in both orders."""

from __future__ import annotations

import ctypes as C
import warnings

import numpy as np
import pytest

from asyncflow_amd import _abi
from asyncflow_amd.results import (JOINT_STATISTICS, JOINT_SUMS, autocorrelation_time, check_series_pairs, load_summary,
                                   series_joint_statistics, series_joint_sums, tick_window_edges)
from oracle.scenarios import lb_with_events
from tests.test_gpu_series_combined import _big_block
from tests.test_gpu_series_histogram import CAP, FILL, N, _hist_block
from tests.test_gpu_series_windows import WIDE, _groupings, _plan, _shapes, _ticks, _wide_plan, _wide_shapes, ram_columns

pytestmark = pytest.mark.gpu

PATTERN = 0x5A5A5A5A
LAGS = (0, 1, 2, 63, 64, 65, 199, 200, 699, 700, 5000)
OUTPUTS = ("n", "sx", "sy", "sxx", "syy", "sxy")
WORDS = {"n": 1, "sx": 2, "sy": 2, "sxx": 4, "syy": 4, "sxy": 4}          # 32-bit words per (group, window, pair)
WIDE_NAME = "wide_fanout52"                                                # 262 series, 66 16-byte groups a row


def _pairs(plan):
    """(a, b, lag) int64 vectors: at every lag a column with itself, two columns of one 16-byte group and the first with the
    last integer column; the last with the first at four lags > 0; on rows of more than 64 groups also columns on either side of
    the 64th group."""
    S = plan.n_series
    ram = ram_columns(S, plan.n_edges)
    ints = np.nonzero(~ram)[0]
    g0, g1 = next((j, j + 1) for j in range(S - 1) if j // 4 == (j + 1) // 4 and not ram[j] and not ram[j + 1])
    first, last, own = int(ints[0]), int(ints[-1]), int(ints[len(ints) // 2])
    out = [(own, own, lag) for lag in LAGS] + [(g0, g1, lag) for lag in LAGS] + [(first, last, lag) for lag in LAGS]
    out += [(last, first, lag) for lag in (1, 2, 65, 199)]
    if plan.series_pitch // 4 > 64:
        below, above = int(ints[ints < 256][-1]), int(ints[ints >= 256][0])
        out += [(below, above, lag) for lag in (0, 1, 64)] + [(above, below, 1), (above, above, 2), (above, first, 700)]
    assert len(out) <= _abi.MAX_SERIES_PAIRS and first // 4 == 0 and last == S - 2
    arr = np.array(out, dtype=np.int64)
    return arr[:, 0].copy(), arr[:, 1].copy(), arr[:, 2].copy()


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

    def run(self, edges, pairs, group=None, n_groups=1, outputs=OUTPUTS):
        """The requested outputs -- n int64, the sums as Python integers, [G, W, P] each --, their raw words and
        scratch_bytes; every output has its place in one buffer between sentinels, and no word outside the requested ones may
        change."""
        torch = self.torch
        W, P = len(edges) - 1, len(pairs[0])
        cells = n_groups * W * P
        guard, at, off = 64, 64, {}
        for k in OUTPUTS:
            off[k] = at
            at += cells * WORDS[k] + (cells * WORDS[k] & 1) + guard   # (even offsets: the 64-bit outputs are 8-byte aligned)
        assert at * 4 < 72 << 20, "an output buffer of a test stays below about 64 MB"
        buf = torch.full((at,), PATTERN, dtype=torch.int32, device=self.dev)
        grp_t = None
        if group is not None:
            ids = np.asarray(group, dtype=np.int64)
            grp_t = torch.as_tensor(np.where(ids < 0, _abi.POOL_SKIP, ids).astype(np.uint32).view(np.int32), device=self.dev)
        torch.cuda.synchronize(self.dev)                      # (the engine has a stream of its own)
        _, scratch = self.eng.summarize_series_joint(
            self.n, n_groups, edges, *pairs, samples_ptr=self.blk_t.data_ptr(), tick_capacity=self.cap, counts_ptr=self.counts_t.data_ptr(),
            group_ptr=0 if grp_t is None else grp_t.data_ptr(), **{f"{k}_ptr": buf.data_ptr() + 4 * off[k] for k in outputs})
        host = buf.cpu().numpy().view(np.uint32)
        written = np.zeros(at, dtype=bool)
        out, raw = {}, {}
        for k in outputs:
            written[off[k]:off[k] + cells * WORDS[k]] = True
            part = host[off[k]:off[k] + cells * WORDS[k]]
            raw[k] = part.tobytes()
            if k == "n":
                out[k] = part.astype(np.int64).reshape(n_groups, W, P)
            else:
                w64 = part.view(np.uint64).astype(object).reshape(n_groups, W, P, WORDS[k] // 2)
                out[k] = w64[..., 0] if WORDS[k] == 2 else w64[..., 0] + w64[..., 1] * (1 << 64)
        assert (host[~written] == PATTERN).all(), f"a word outside the requested outputs {outputs} was written"
        return out, raw, scratch


def _scenario_sums(plan, blk, counts, pairs, edges):
    """The host definition of every scenario of a block."""
    out = []
    for s in range(blk.shape[0]):
        m = min(int(counts[s, _abi.CNT_TICKS]), blk.shape[1])
        out.append(series_joint_sums(np.ascontiguousarray(blk[s, :m, :plan.n_series].T), edges, plan.n_edges, pairs))
    return out


def _pool(per, ids, n_groups):
    """The members' sums added with Python integers."""
    shape = (n_groups, *per[0]["n"].shape)
    out = {"n": np.zeros(shape, dtype=np.int64)}
    for k in JOINT_SUMS:
        out[k] = np.zeros(shape, dtype=object)
        out[k][...] = 0
    for s, one in enumerate(per):
        g = 0 if ids is None else int(ids[s])
        if g < 0:
            continue
        for k in out:
            out[k][g] = out[k][g] + one[k]
    return out


def _equal(got, want, what):
    for k in got:
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        d = got[k] != want[k]
        assert not d.any(), (what, k, np.argwhere(d)[:5], got[k][d][:5], want[k][d][:5])


def _check_plan(plan, name, blk, counts, shapes):
    pairs = _pairs(plan)
    lag = pairs[2]
    seen = np.zeros(4, dtype=np.int64)          # cells with samples, empty cells, non-zero high words, lagged cells with samples
    d = _Device(plan, blk, counts)
    try:
        for what, edges in shapes:
            per = _scenario_sums(plan, blk, counts, pairs, edges)
            groupings = _groupings(N)
            if what == "one tick each":         # (the other groupings: outputs of more than 64 MB; singletons below)
                groupings = [g for g in groupings if g[2] in ("interleaved", "one group (NULL)")]
            for group, n_groups, gname in groupings:
                want = _pool(per, group, n_groups)
                got, _, _ = d.run(edges, pairs, group, n_groups)
                _equal(got, want, f"{name}, {what}, {gname}")
                seen += [int((want["n"] > 0).sum()), int((want["n"] == 0).sum()), int(sum(v >> 64 != 0 for v in want["sxy"].ravel())),
                         int((want["n"][:, :, lag > 0] > 0).sum())]
                if what == "one tick each":
                    assert not want["n"][:, :, lag > 0].any() and want["n"][:, :, lag == 0].any()
                if what == "200 ticks":         # lag 199 leaves one pair to every member with all 200 rows, lag 200 none
                    rows = np.array([np.diff(np.minimum(edges, min(int(c), CAP))) for c in counts[:, _abi.CNT_TICKS]])
                    ids = np.zeros(N, dtype=np.int64) if group is None else np.asarray(group)
                    for g in range(n_groups):
                        assert (got["n"][g][:, lag == 199] == (rows[ids == g] == 200).sum(axis=0)[:, None]).all()
                        assert not got["n"][g][:, lag >= 200].any()
            if what == "one tick each":         # singletons: n and sxy alone
                group, n_groups, gname = next(g for g in _groupings(N) if g[2] == "singletons")
                got, _, _ = d.run(edges, pairs, group, n_groups, outputs=("n", "sxy"))
                want = _pool(per, group, n_groups)
                _equal(got, {k: want[k] for k in got}, f"{name}, {what}, {gname}")
    finally:
        d.close()
    return seen


# ------------------------------------------------------------------------------------ 1. against the host definition
@pytest.mark.parametrize("big", [False, True], ids=["counts", "words to 2^32"])
@pytest.mark.parametrize("name", ["single_server", "lb_two_servers", "fanout8"])
def test_synthetic_blocks_equal_the_host_definition(name, big):
    plan = _plan(name)
    assert plan.n_series == {"single_server": 6, "lb_two_servers": 12, "fanout8": 42}[name] and plan.series_pitch <= 60
    rng = np.random.default_rng(len(name) + 100 * big)
    ticks = _ticks(rng, N, CAP)
    assert ticks[0] == 0 and ticks[1] == CAP and ticks[2] > CAP and ticks[3] == 1
    blk, counts = (_big_block if big else _hist_block)(plan, rng, N, CAP, ticks)
    assert (blk[:, :, plan.n_series:] == FILL).all() and (blk[0] == FILL).all() and (blk[3, 1:] == FILL).all()
    seen = _check_plan(plan, name, blk, counts, _shapes(CAP))
    assert seen[0] > 0 and seen[1] > 0 and seen[3] > 0 and (seen[2] > 0) == big, seen      # (a dropped carry fails where big)


def test_wide_rows_equal_the_host_definition():
    plan = _wide_plan(WIDE_NAME)
    assert (plan.n_series, plan.series_pitch) == WIDE[WIDE_NAME] and plan.series_pitch // 4 == 66
    rng = np.random.default_rng(plan.n_series)
    blk, counts = _big_block(plan, rng, N, CAP, _ticks(rng, N, CAP))
    a, b, _ = _pairs(plan)
    assert ((a < 256) & (b >= 256)).any() and ((a >= 256) & (b < 256)).any() and ((a >= 256) & (b >= 256)).any()
    shapes = [*_wide_shapes(CAP), ("200 ticks", tick_window_edges(200, CAP))]
    seen = _check_plan(plan, WIDE_NAME, blk, counts, shapes)
    assert (seen > 0).all(), seen


# ------------------------------------------------------------------------------------ 2. the outputs depend on the data alone
def test_a_pair_does_not_depend_on_the_others_on_the_batch_or_on_the_run():
    plan = _plan("lb_two_servers")
    rng = np.random.default_rng(5)
    n, cap = 8, 512
    blk, counts = _big_block(plan, rng, n, cap, _ticks(rng, n, cap))
    ints = np.nonzero(~ram_columns(plan.n_series, plan.n_edges))[0]
    lags = np.array([0, 1, 2, 3, 5, 63, 64, 65, 100, 199, 200, 255, 256, 300, 511, 512])
    a = np.array([int(ints[i % len(ints)]) for i in range(64)])
    b = np.array([int(ints[(i * 3 + 1) % len(ints)]) for i in range(64)])
    lag = lags[np.arange(64) % 16][rng.permutation(64)]
    big, big_counts = _big_block(plan, rng, 10 * n, cap, rng.integers(0, cap + 1, 10 * n))
    where = np.arange(n) * 10 + 3
    big[where], big_counts[where] = blk, counts
    d, d_big = _Device(plan, blk, counts), _Device(plan, big, big_counts)

    def words(raw, k, G, W, P):
        return np.frombuffer(raw[k], dtype=np.uint32).reshape(G, W, P, WORDS[k])

    try:
        for edges in (tick_window_edges(200, cap), tick_window_edges(7, cap), np.array([0, cap])):
            W = len(edges) - 1
            for group, G in ((np.arange(n), n), (np.arange(n) % 3, 3)):
                _, full, _ = d.run(edges, (a, b, lag), group, G)
                _, again, _ = d.run(edges, (a, b, lag), group, G)
                assert all(full[k] == again[k] for k in OUTPUTS)                                   # the call twice
                perm = rng.permutation(64)
                _, mixed, _ = d.run(edges, (a[perm], b[perm], lag[perm]), group, G)                # the 64 pairs permuted
                for k in OUTPUTS:
                    assert np.array_equal(words(mixed, k, G, W, 64), words(full, k, G, W, 64)[:, :, perm]), k
                for p in (0, 17, 40, 63):                                                          # a pair alone
                    _, alone, _ = d.run(edges, (a[[p]], b[[p]], lag[[p]]), group, G)
                    for k in OUTPUTS:
                        assert np.array_equal(words(alone, k, G, W, 1), words(full, k, G, W, 64)[:, :, [p]]), (k, p)
            # the same scenarios inside a batch ten times as large
            _, alone, _ = d.run(edges, (a, b, lag), np.arange(n), n)
            _, inside, _ = d_big.run(edges, (a, b, lag), np.arange(10 * n), 10 * n)
            for k in OUTPUTS:
                assert np.array_equal(words(alone, k, n, W, 64), words(inside, k, 10 * n, W, 64)[where]), k
            ids = np.full(10 * n, -1)
            ids[where] = np.arange(n) % 3                                                          # as members of groups
            _, x, _ = d.run(edges, (a, b, lag), np.arange(n) % 3, 3)
            _, y, _ = d_big.run(edges, (a, b, lag), ids, 3)
            assert all(x[k] == y[k] for k in OUTPUTS)
        got, _, _ = d.run(edges, (a, b, lag), np.arange(n) % 3, 3)
        _equal(got, _pool(_scenario_sums(plan, blk, counts, (a, b, lag), edges), np.arange(n) % 3, 3), "64 pairs of a call")
    finally:
        d.close()
        d_big.close()


# ------------------------------------------------------------------------------------ 3. many waves, runs of windows
@pytest.mark.parametrize("name", ["lb_two_servers", WIDE_NAME])
def test_many_waves_add_into_one_cell(name):
    """300 scenarios in one group and one window: 300 records fold into every cell."""
    plan = _wide_plan(name) if name in WIDE else _plan(name)
    rng = np.random.default_rng(300)
    n, cap = 300, 70 if name in WIDE else 200                          # (rows of 1 040 bytes: a smaller block)
    blk, counts = _big_block(plan, rng, n, cap, _ticks(rng, n, cap))
    pairs = _pairs(plan)
    d = _Device(plan, blk, counts)
    try:
        for what, edges in (("one window", np.array([0, cap])), ("65 ticks", tick_window_edges(65, cap))):
            per = _scenario_sums(plan, blk, counts, pairs, edges)
            for group, n_groups in ((None, 1), (np.arange(n) % 3, 3)):
                got, _, _ = d.run(edges, pairs, group, n_groups)
                want = _pool(per, group, n_groups)
                _equal(got, want, f"{name}, {what}, {n_groups} groups")
        assert max(v >> 64 for v in want["sxy"].ravel()) > 100
    finally:
        d.close()


def test_work_items_of_several_windows():
    """The engine gives a wave max(1, W / ceil(32768 / n)) consecutive windows: 300 scenarios and 700 windows of one tick are
    runs of 6 windows with a last run of 4; 140 windows of 5 ticks stay one window a wave."""
    plan = _plan("single_server")
    n, cap = 300, 700
    assert max(1, cap // -(-32768 // n)) == 6 and cap % 6 == 4
    rng = np.random.default_rng(6)
    blk, counts = _hist_block(plan, rng, n, cap, _ticks(rng, n, cap), top=4)
    a, b, lag = _pairs(plan)
    keep = np.isin(lag, (0, 1, 2, 5000))
    pairs = (a[keep], b[keep], lag[keep])
    group = np.arange(n) % 5
    d = _Device(plan, blk, counts)
    try:
        for what, edges in (("one tick each", np.arange(cap + 1)), ("350 windows of 2 ticks", tick_window_edges(2, cap))):
            got, _, _ = d.run(edges, pairs, group, 5)
            want = _pool(_scenario_sums(plan, blk, counts, pairs, edges), group, 5)
            _equal(got, want, what)
        assert want["n"][:, :, pairs[2] == 1].any() and not want["n"][:, :, pairs[2] == 2].any()
    finally:
        d.close()


# ------------------------------------------------------------------------------------ 4. NULL outputs, scratch
def test_null_outputs_are_skipped():
    plan = _plan("single_server")
    rng = np.random.default_rng(2)
    n, cap = 9, 300
    blk, counts = _big_block(plan, rng, n, cap, _ticks(rng, n, cap))
    pairs = _pairs(plan)
    d = _Device(plan, blk, counts)
    try:
        for edges in (tick_window_edges(100, cap), tick_window_edges(9, cap)):
            for group, G in ((np.arange(n) % 2, 2), (np.arange(n), n)):
                _, full, _ = d.run(edges, pairs, group, G)
                for outputs in (("n", "sxy"), ("n", "sxy", "sx"), ("n", "sxy", "sy", "syy"), ("n", "sxy", "sxx"), ("n", "sx", "sy", "sxx", "sxy")):
                    got, raw, _ = d.run(edges, pairs, group, G, outputs=outputs)
                    assert set(got) == set(outputs)           # (run() asserts that the guard words and the skipped outputs stay)
                    for k in outputs:
                        assert raw[k] == full[k], (outputs, k)
    finally:
        d.close()


def test_scratch_stays_within_the_bound_of_the_header():
    """include/asyncflow_hip.h: 4 B per edge + 16 B per pair + 4 B per group + 4 B per scenario + 1 536 B of alignment, and --
    unless every group holds at most one scenario -- 52 B per (scenario, window, pair)."""
    plan = _plan("fanout8")
    rng = np.random.default_rng(3)
    n, cap = 40, 400
    blk, counts = _hist_block(plan, rng, n, cap, rng.integers(0, cap + 1, n))
    pairs = _pairs(plan)
    edges = tick_window_edges(20, cap)
    W, P = len(edges) - 1, len(pairs[0])
    for group, G, records in ((np.arange(n) % 7, 7, True), (np.arange(n) * 3, 3 * n, False)):
        d = _Device(plan, blk, counts)                                  # (a fresh engine: the scratch of this call alone)
        try:
            _, _, scratch = d.run(edges, pairs, group, G)
        finally:
            d.close()
        bound = 4 * (W + 1) + 16 * P + 4 * (G + 1) + 4 * n + 1536 + (52 * n * W * P if records else 0)
        print(f"{G} groups: scratch_bytes {scratch}, bound {bound}")
        assert (52 * n * W * P if records else 0) < scratch <= bound
        assert records or scratch < 52 * n * W * P


# ------------------------------------------------------------------------------------ 5. refusals
def test_device_argument_checks():
    """Error codes from calls that return before anything is written: no output word is touched."""
    import torch

    from asyncflow_amd.engine import PLAN_ONLY, Engine, load_library

    plan = _plan("lb_two_servers")
    S = plan.n_series
    ram = np.nonzero(ram_columns(S, plan.n_edges))[0]
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
    outs = torch.full((16 * 1024,), PATTERN, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    eng, planner = Engine(plan, 0), Engine(plan, PLAN_ONLY)
    pu = C.POINTER(C.c_uint32)
    try:
        def call(edges, a=(0, 1), b=(1, 0), lag=(0, 3), n_pairs=None, samples=True, counts_p=counts_t, n_windows=None, cap=50, engine=eng,
                 n_groups=2, group=None, n_out=True, sxy=True, cols=True):
            e = (C.c_uint32 * len(edges))(*edges) if edges is not None else None
            arr = [(C.c_uint32 * max(len(v), 1))(*v) for v in (a, b, lag)]
            out = _abi.AfOutputs(0, None, cap, C.c_void_p(blk_t.data_ptr() if samples else None),
                                 C.c_void_p(counts_p.data_ptr() if counts_p is not None else None))
            base = outs.data_ptr()
            req = _abi.AfSeriesJoint(
                3, n_groups, (len(edges) - 1 if n_windows is None else n_windows), C.c_void_p(group.data_ptr() if group is not None else None),
                C.cast(e, pu) if e is not None else None, len(a) if n_pairs is None else n_pairs, C.cast(arr[0], pu), C.cast(arr[1], pu),
                C.cast(arr[2], pu) if cols else None, C.c_void_p(base) if n_out else None, C.c_void_p(base + 4096), C.c_void_p(base + 8192),
                C.c_void_p(base + 12288), C.c_void_p(base + 16384), C.c_void_p(base + 20480) if sxy else None, 0.0, 0)
            rc = lib.af_engine_summarize_series_joint(engine._h, C.byref(out), C.byref(req))  # noqa: SLF001
            return rc, lib.af_last_error().decode()

        INV, CAPACITY = _abi.AF_ERR_INVALID, _abi.AF_ERR_CAPACITY
        refused = [
            (call([0, 10], a=(), b=(), lag=()), INV, "n_pairs"),
            (call([0, 10], a=[0] * 65, b=[0] * 65, lag=[0] * 65), INV, "n_pairs"),
            (call([0, 10], cols=False), INV, "a, b and lag"),
            (call([0, 10], a=(0, S)), INV, "names series"),
            (call([0, 10], b=(S + 7, 0)), INV, "names series"),
            (call([0, 10], a=(0, int(ram[0]))), INV, "ram_in_use"),
            (call([0, 10], b=(int(ram[-1]), 0)), INV, "ram_in_use"),
            (call([0, 10], lag=(0, 0x80000000)), INV, "below 2^31"),
            (call([0, 10], lag=(0xFFFFFFFF, 0)), INV, "below 2^31"),
            (call(None, n_windows=1), INV, "tick_edges"),
            (call([0, 10, 10]), INV, "strictly increasing"),
            (call([10, 5]), INV, "strictly increasing"),
            (call([0], n_windows=0), INV, "n_windows"),
            (call([0, 10], group=bad_group), INV, "group id out of range"),
            (call([0, 10], samples=False), INV, "samples"),
            (call([0, 10], counts_p=None), INV, "counts"),
            (call([0, 10], n_out=False), INV, "n and sxy"),
            (call([0, 10], sxy=False), INV, "n and sxy"),
            (call([0, 0x7FFFFFFF], counts_p=huge_t, cap=0x7FFFFFFF, n_groups=1), CAPACITY, "2^32 or more"),
            (call([0, 10], n_groups=0xFFFFFFFF), CAPACITY, "2^32 - 1"),
            (call([0, 10], cap=0x80000000), CAPACITY, "2^31"),
            (call([0, 10], engine=planner), _abi.AF_ERR_NO_DEVICE, "planning-only"),
        ]
        for i, ((rc, msg), code, reason) in enumerate(refused):
            assert rc == code and reason in msg, (i, rc, msg, code, reason)
        torch.cuda.synchronize(dev)
        assert (outs.cpu().numpy().view(np.uint32) == PATTERN).all(), "a refused call touched an output"
        assert call([0, 10], n_groups=1, lag=(0, 0x7FFFFFFF))[0] == _abi.AF_OK
        host = outs.cpu().numpy().view(np.uint32)
        assert host[:3].tolist() == [10 + 10 + 0, 0, PATTERN] and host[1024 + 2 * 1] == 0 and host[1024 + 4] == PATTERN
    finally:
        eng.close()
        planner.close()


# ------------------------------------------------------------------------------------ 6. through the Python API
@pytest.fixture(scope="module")
def event_run():
    from asyncflow_amd.runner import SimulationRunner

    payload = lb_with_events(horizon=60, scale=0.1)
    seeds = 0xE7C50000 + np.arange(64, dtype=np.uint64)
    res = SimulationRunner(simulation_input=payload, seeds=seeds).run()
    words = [np.ascontiguousarray(res[s]._samples).view(np.uint32) for s in range(len(res))]  # noqa: SLF001
    return res, np.arange(64) % 4, words


def _bits(x) -> bytes:
    return np.ascontiguousarray(x, dtype=np.float64).tobytes()


def test_event_workload_through_the_python_api(event_run, tmp_path):
    res, ids, words = event_run
    names = res.series_names()
    ne = res.plan.n_edges
    edges = tick_window_edges(int(round(10.0 / res.plan.sample_period)), res.plan.tick_count)
    q = [nm for nm in names if nm.endswith(":ready_queue_len")]
    e = [nm for nm in names if nm.endswith(":edge_concurrent_connection")]
    z = [nm for nm in names if nm.endswith(":event_loop_io_sleep")]
    pairs = {"queues": (q[0], q[1]), "sleepers": (z[0], z[1]), "sleepers+5": (z[0], z[1], 5), "sleepers-5": (z[1], z[0], 5),
             "edge leads": (e[1], z[0], 2), "acf40": (z[0], z[0], 40), "far": (z[0], z[1], 2000)}
    labels, a, b, lag = check_series_pairs(pairs, names, ne)
    for by, gid, G in ((ids, ids, 4), ("scenario", np.arange(64), 64)):
        got = res.series_joint_summary(pairs, 10.0, by=by)
        want = _pool([series_joint_sums(w, edges, ne, (a, b, lag)) for w in words], gid, G)
        _equal({k: got[k] for k in ("n", *JOINT_SUMS)}, want, f"by {G} groups")
        st = series_joint_statistics(want, exact=True)
        for k in JOINT_STATISTICS:
            assert _bits(got[k]) == _bits(st[k]), k
        assert got["labels"] == labels and got["lag"].tolist() == lag.tolist() and np.array_equal(got["tick_edges"], edges)
        assert got["replicas"].tolist() == [64 // G] * G and got["series_joint_ms"] > 0 and got["scratch_bytes"] > 0
        assert np.array_equal(got["times"], edges[:-1] * res.plan.sample_period)
    assert np.isfinite(got["corr"]).any() and not got["n"][:, :, labels.index("far")].any()
    mine = res[5].get_series_joint(pairs, 10.0)
    for k in ("n", *JOINT_SUMS):
        assert (got[k][5] == mine[k]).all(), k
    # a small grid with replicas: the autocorrelation of the servers' series, 164 pairs in three calls of at most 64
    out = res.series_autocorrelation_summary(["*:ready_queue_len", "*:event_loop_io_sleep"], 40, 20.0, by=ids)
    edges20 = tick_window_edges(int(round(20.0 / res.plan.sample_period)), res.plan.tick_count)
    cols = [names.index(nm) for nm in q + z]
    assert out["series"] == q + z and out["calls"] == -(-len(cols) * 41 // 64) > 1 and out["acf"].shape == (4, len(edges20) - 1, len(cols), 41)
    lags = np.arange(41)
    for i, c in enumerate(cols):
        want = _pool([series_joint_sums(w, edges20, ne, (np.full(41, c), np.full(41, c), lags)) for w in words], ids, 4)
        assert _bits(out["acf"][:, :, i]) == _bits(series_joint_statistics(want, exact=True)["corr"]) and np.array_equal(out["n"][:, :, i], want["n"])
    tau = autocorrelation_time(out["acf"], out["n"][..., 0])
    assert _bits(out["tau"]) == _bits(tau["tau"]) and _bits(out["ess"]) == _bits(tau["ess"]) and np.array_equal(out["tau_truncated"], tau["tau_truncated"])
    assert np.nanmax(out["tau"][:, :, len(q):]) > 1.0 and (out["acf"][..., 0][~np.isnan(out["acf"][..., 0])] == 1.0).all()
    # bands over the replicas
    per = res.series_joint_summary(pairs, 10.0, by="scenario")
    pooled = res.series_joint_summary(pairs, 10.0, by=ids)
    for of in ("corr", "cov"):
        bands = res.series_joint_bands(pairs, 10.0, by=ids, of=of, level=0.9, q=(0.1, 0.75))
        assert bands["mean"].shape == (4, len(edges) - 1, len(labels)) and bands["labels"] == labels
        assert _bits(bands["pooled"]) == _bits(pooled[of])
        for g in range(4):
            mem = per[of][ids == g]
            assert np.array_equal(bands["n"][g], (~np.isnan(mem)).sum(axis=0))
            with warnings.catch_warnings():                  # (a pair without a sample is NaN in every replica)
                warnings.simplefilter("ignore", RuntimeWarning)
                np.testing.assert_allclose(bands["mean"][g], np.nanmean(mem, axis=0), rtol=1e-12, atol=1e-15)
                np.testing.assert_allclose(bands["q_hi"][g], np.nanquantile(mem, 0.75, axis=0), rtol=1e-12, atol=1e-15)
    # the saved file
    for ext in ("npz", "parquet"):
        if ext == "parquet":
            try:
                import pyarrow  # noqa: F401
            except ImportError:
                continue
        path = str(tmp_path / f"series_joint.{ext}")
        written = res.save_series_joint_summary(path, ids, pairs=pairs, window_s=10.0)
        back = load_summary(path)
        assert set(back) == set(written)
        for k, v in written.items():
            assert np.array_equal(np.asarray(back[k], dtype=v.dtype), v, equal_nan=True), k
        bands = res.series_joint_bands(pairs, 10.0, by=ids)
        assert back["replicas"].tolist() == [16] * 4
        for p, name in enumerate(labels):
            assert _bits(back[f"series_joint_corr:{name}"]) == _bits(pooled["corr"][:, :, p]) and _bits(back[f"series_joint_cov:{name}"]) == _bits(pooled["cov"][:, :, p])
            assert np.array_equal(back[f"series_joint_n:{name}"], pooled["n"][:, :, p])
            assert _bits(back[f"series_joint_q05:{name}"]) == _bits(bands["q_lo"][:, :, p]) and _bits(back[f"series_joint_q95:{name}"]) == _bits(bands["q_hi"][:, :, p])
        assert np.array_equal(back["series_joint_tick_edges"], edges) and np.array_equal(back["series_joint_times"], edges[:-1] * res.plan.sample_period)
