"""Warm-up truncation of the sampled series per (group, window of ticks, column) on the MI355X
(af_engine_summarize_series_warmup): synthetic sample blocks handed straight to the entry -- the padding words and the rows at
or past a scenario's ticks hold 0xFFFFFFFF, which shows as a wrong sum if it is read -- with every output in one buffer between
sentinels.  The reference is the host definition, results.series_warmup_sums of the members of every group.  Every output is
an exact integer and is compared with ==.

n = 23 scenarios of capacity 700; the plans of 6, 12 and 42 series (rows staged in LDS) and one of 262 (the global form) on
every window shape and grouping with B in 1, 2, 5, 7, 64, 65, 350, 351, 700 and 701 ticks: a batch inside a 64-row step, one
that straddles it, a window of one batch and of none.  Two tick vectors: one without a short scenario (groups of equal and of
unequal lengths) and one with scenarios of 0 ticks and of 1 tick (J = 0 for their groups)."""

from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

from asyncflow_amd import _abi
from asyncflow_amd.results import (WARMUP_STATISTICS, WARMUP_SUMS, load_summary, series_warmup_cut, series_warmup_statistics, series_warmup_sums,
                                   warmup_truncation)
from oracle.scenarios import lb_with_events
from tests.test_gpu_series_combined import _big_block
from tests.test_gpu_series_histogram import CAP, FILL, N, _hist_block
from tests.test_gpu_series_windows import WIDE, _groupings, _plan, _shapes, _wide_plan, _wide_shapes, ram_columns

pytestmark = pytest.mark.gpu

PATTERN = 0x5A5A5A5A
BATCHES = (1, 2, 5, 7, 64, 65, 350, 351, 700, 701)
OUTPUTS = ("batches", "trunc", "s1", "s2", "s1_all", "s2_all")
WORDS = {"batches": 1, "trunc": 1, "s1": 4, "s2": 6, "s1_all": 4, "s2_all": 6}   # 32-bit words per (group, window[, column])
WIDE_NAME = "wide_fanout52"                                                       # 262 series, 66 16-byte groups a row


def _tick_vectors(n, cap):
    """Without a short scenario -- all rows, more than stored, 699, 650: the interleaved groups 0, 2 and 4 have members of
    equal lengths, 1 and 5 of unequal ones --, and with scenarios of 0 ticks, 1 tick, 64, 65 and 333."""
    long = np.full(n, cap)
    long[2], long[7], long[11] = cap + 50, cap - 1, cap - 50
    short = long.copy()
    short[0], short[3], short[5], short[6], short[12] = 0, 1, 64, 65, 333
    return long, short


def _columns(plan, every=False):
    """The first and the last integer series, two columns of one 16-byte group, a duplicate; `every`: all integer series up to
    64 columns in all."""
    S = plan.n_series
    ram = ram_columns(S, plan.n_edges)
    ints = np.nonzero(~ram)[0]
    g0, g1 = next((j, j + 1) for j in range(S - 1) if j // 4 == (j + 1) // 4 and not ram[j] and not ram[j + 1])
    cols = [int(ints[-1]), int(ints[0]), g1, g0, int(ints[-1])]
    if every:
        cols += [int(j) for j in ints[:_abi.MAX_SERIES_WARMUP_COLUMNS - len(cols)]]
    assert len(cols) <= _abi.MAX_SERIES_WARMUP_COLUMNS and ints[0] // 4 == 0 and ints[-1] == S - 2
    return np.array(cols, dtype=np.int64)


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

    def run(self, edges, cols, batch, group=None, n_groups=1, outputs=OUTPUTS):
        """The requested outputs -- batches [G, W] and trunc [G, W, C] int64, the sums as Python integers [G, W, C] --, their
        raw words and scratch_bytes; every output has its place in one buffer between sentinels, and no word outside the
        requested ones may change."""
        torch = self.torch
        W, Cn = len(edges) - 1, len(cols)
        guard, at, off, size = 64, 64, {}, {}
        for k in OUTPUTS:
            size[k] = n_groups * W * (1 if k == "batches" else Cn) * WORDS[k]
            off[k] = at
            at += size[k] + (size[k] & 1) + guard                 # (even offsets: the 64-bit outputs are 8-byte aligned)
        assert at * 4 < 72 << 20, "an output buffer of a test stays below about 64 MB"
        buf = torch.full((at,), PATTERN, dtype=torch.int32, device=self.dev)
        grp_t = None
        if group is not None:
            ids = np.asarray(group, dtype=np.int64)
            grp_t = torch.as_tensor(np.where(ids < 0, _abi.POOL_SKIP, ids).astype(np.uint32).view(np.int32), device=self.dev)
        torch.cuda.synchronize(self.dev)                          # (the engine has a stream of its own)
        _, scratch = self.eng.summarize_series_warmup(
            self.n, n_groups, edges, cols, batch, samples_ptr=self.blk_t.data_ptr(), tick_capacity=self.cap, counts_ptr=self.counts_t.data_ptr(),
            group_ptr=0 if grp_t is None else grp_t.data_ptr(), **{f"{k}_ptr": buf.data_ptr() + 4 * off[k] for k in outputs})
        host = buf.cpu().numpy().view(np.uint32)
        written = np.zeros(at, dtype=bool)
        out, raw = {}, {}
        for k in outputs:
            written[off[k]:off[k] + size[k]] = True
            part = host[off[k]:off[k] + size[k]]
            raw[k] = part.tobytes()
            if k == "batches":
                out[k] = part.astype(np.int64).reshape(n_groups, W)
            elif k == "trunc":
                out[k] = part.astype(np.int64).reshape(n_groups, W, Cn)
            else:
                w64 = part.view(np.uint64).astype(object).reshape(n_groups, W, Cn, WORDS[k] // 2)
                out[k] = sum(w64[..., i] * (1 << (64 * i)) for i in range(WORDS[k] // 2))
        assert (host[~written] == PATTERN).all(), f"a word outside the requested outputs {outputs} was written"
        return out, raw, scratch


def _members(plan, blk, counts):
    """Every scenario's stored words [n_series, m_s]."""
    return [np.ascontiguousarray(blk[s, :min(int(counts[s, _abi.CNT_TICKS]), blk.shape[1]), :plan.n_series].T) for s in range(blk.shape[0])]


def _want(plan, members, group, n_groups, edges, batch, cols):
    """The host definition of every group."""
    ids = np.zeros(len(members), dtype=np.int64) if group is None else np.asarray(group)
    per = [series_warmup_sums([members[s] for s in np.nonzero(ids == g)[0]], edges, plan.n_edges, batch, cols) for g in range(n_groups)]
    return {k: np.stack([p[k] for p in per]) for k in OUTPUTS}


def _equal(got, want, what):
    for k in got:
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        d = got[k] != want[k]
        assert not d.any(), (what, k, np.argwhere(d)[:5], got[k][d][:5], want[k][d][:5])


def _check_shape(plan, name, blocks, what, edges, si):
    """Every B on one window shape: the groupings and the two tick vectors in turn, every grouping twice; two of the calls
    with all integer columns (up to 64)."""
    seen = np.zeros(4, dtype=np.int64)          # cells with J = 0, with J > 0, with d* > 0, groups that a short member emptied
    groupings = _groupings(N)
    devices = [(_Device(plan, blk, counts), _members(plan, blk, counts)) for blk, counts in blocks]
    try:
        for bi, batch in enumerate(BATCHES):
            group, n_groups, gname = groupings[(bi + si) % len(groupings)]
            which = 1 if bi % 3 == 1 else 0
            every = bi in (2, 5) and len(edges) <= 40
            cols = _columns(plan, every)
            d, members = devices[which]
            want = _want(plan, members, group, n_groups, edges, batch, cols)
            got, _, _ = d.run(edges, cols, batch, group, n_groups)
            _equal(got, want, f"{name}, {what}, {gname}, B = {batch}, ticks {which}")
            seen += [int((want["batches"] == 0).sum()), int((want["batches"] > 0).sum()), int((want["trunc"] > 0).sum()),
                     int(which == 1 and (want["batches"][0] == 0).all())]
        if what == "one tick each":              # the singletons at B = 1, where every member's window is one batch
            group, n_groups, gname = groupings[3]
            cols = _columns(plan)[:4]
            for which, (d, members) in enumerate(devices):
                want = _want(plan, members, group, n_groups, edges, 1, cols)
                got, _, _ = d.run(edges, cols, 1, group, n_groups)
                _equal(got, want, f"{name}, {what}, {gname}, B = 1, ticks {which}")
                assert (want["batches"] == 1).any() and (want["s1_all"] > 0).any()
    finally:
        for d, _ in devices:
            d.close()
    return seen


@functools.lru_cache(maxsize=None)
def _blocks(name, big):
    """The two blocks of a plan, one per tick vector; made once and shared by the window shapes (never written to)."""
    plan = _wide_plan(name) if name in WIDE else _plan(name)
    rng = np.random.default_rng(len(name) + 100 * big)
    make = _big_block if big else _hist_block
    out = []
    for ticks in _tick_vectors(N, CAP):
        blk, counts = make(plan, rng, N, CAP, ticks)
        assert (blk[:, :, plan.n_series:] == FILL).all() and (blk[7, CAP - 1:] == FILL).all()
        out.append((blk, counts))
    assert (out[1][0][0] == FILL).all() and (out[1][0][3, 1:] == FILL).all()
    return plan, out


# ------------------------------------------------------------------------------------ 1. against the host definition
@pytest.mark.parametrize("si", range(7), ids=[s[0] for s in _shapes(CAP)])
@pytest.mark.parametrize("name", ["single_server", "lb_two_servers", "fanout8"])
def test_synthetic_blocks_equal_the_host_definition(name, si):
    plan, blocks = _blocks(name, si % 2 == 1)              # words to 2^32 - 2 on every other shape
    assert plan.n_series == {"single_server": 6, "lb_two_servers": 12, "fanout8": 42}[name] and plan.series_pitch <= 60
    what, edges = _shapes(CAP)[si]
    seen = _check_shape(plan, name, blocks, what, edges, si)
    assert seen[0] > 0 and seen[1] > 0 and (seen[2] > 0 or what == "one tick each") and seen[3] > 0, seen      # (J <= 1 there: D = 0)


@pytest.mark.parametrize("si", range(6), ids=[s[0] for s in _wide_shapes(CAP)])
def test_wide_rows_equal_the_host_definition(si):
    plan, blocks = _blocks(WIDE_NAME, True)
    assert (plan.n_series, plan.series_pitch) == WIDE[WIDE_NAME] and plan.series_pitch // 4 == 66
    cols = _columns(plan)
    assert (cols < 256).any() and (cols >= 256).any()
    what, edges = _wide_shapes(CAP)[si]
    seen = _check_shape(plan, WIDE_NAME, blocks, what, edges, si)
    assert seen[0] > 0 and seen[1] > 0 and (seen[2] > 0 or what == "one tick each") and seen[3] > 0, seen


# ------------------------------------------------------------------------------------ 2. planted ties
def test_planted_ties_take_the_smaller_d():
    """A constant column has A = 0 at every d: d* = 0.  A column that is constant from row 100 on has A = 0 from the batch
    that holds no earlier row: d* = ceil(100 / B), the smallest such d, while it lies within the search limit."""
    plan = _plan("lb_two_servers")
    rng = np.random.default_rng(12)
    n, cap = 8, 512
    blk, counts = _hist_block(plan, rng, n, cap, np.full(n, cap))
    ints = np.nonzero(~ram_columns(plan.n_series, plan.n_edges))[0]
    flat, late, free = int(ints[1]), int(ints[4]), int(ints[2])
    blk[:, :, flat] = 5
    blk[:, :100, late] = rng.integers(0, 1000, (n, 100))
    blk[:, 99, late] = 1000 + np.arange(n)                         # (row 99 differs from what follows in every scenario)
    blk[:, 100:, late] = 9
    cols = np.array([flat, late, free, late])
    members = _members(plan, blk, counts)
    d = _Device(plan, blk, counts)
    try:
        for batch in (1, 2, 5, 7, 64):
            for group, G in ((None, 1), (np.arange(n), n), (np.arange(n) % 3, 3)):
                for edges in (np.array([0, cap]), np.array([0, 300, cap])):
                    got, _, _ = d.run(edges, cols, batch, group, G)
                    _equal(got, _want(plan, members, group, G, edges, batch, cols), f"B = {batch}, {G} groups")
                    assert not got["trunc"][:, :, 0].any() and (got["trunc"][:, 0, 1] == -(-100 // batch)).all()
                    assert (got["trunc"][:, 0, 3] == got["trunc"][:, 0, 1]).all()
                    if len(edges) == 3:                             # the second window is constant in both planted columns
                        assert not got["trunc"][:, 1, [0, 1, 3]].any()
    finally:
        d.close()


# ------------------------------------------------------------------------------------ 3. long sequences: the upper limbs
def _largest_product(y):
    """The largest product the comparisons of the walk over `y` form."""
    J = len(y)
    s1, s2 = sum(y), sum(v * v for v in y)
    best, largest = (J * s2 - s1 * s1, J ** 3), 0
    for d in range(1, J // 2 + 1):
        s1 -= y[d - 1]
        s2 -= y[d - 1] ** 2
        m = J - d
        a = m * s2 - s1 * s1
        left, right = a * best[1], best[0] * m ** 3
        largest = max(largest, left, right)
        if left < right:
            best = (a, m ** 3)
    return largest


def test_long_block_compares_products_past_128_bits():
    """4 scenarios x 32 768 rows of the 6-series plan, the words 0xFFFFFFFF or random, a third as large over the first seventh
    of the rows: the compared products A m^3 pass 2^128 (asserted from the test's own walk), so the upper limbs of the device's
    256-bit values decide."""
    plan = _plan("single_server")
    rng = np.random.default_rng(32768)
    n, cap = 4, 32768
    S = plan.n_series
    ints = np.nonzero(~ram_columns(S, plan.n_edges))[0]
    blk = np.full((n, cap, plan.series_pitch), FILL, dtype=np.uint32)
    body = np.where(rng.random((n, cap, S)) < 0.5, 0xFFFFFFFF, rng.integers(0, 2 ** 32, (n, cap, S))).astype(np.uint32)
    body[:, : cap // 7] //= 3
    blk[:, :, :S] = body
    counts = np.zeros((n, _abi.CNT_SLOTS), dtype=np.uint32)
    counts[:, _abi.CNT_TICKS] = cap
    cols = np.array([int(ints[0]), int(ints[-1])])
    members = _members(plan, blk, counts)
    edges = np.array([0, cap])
    d = _Device(plan, blk, counts)
    bits = []
    try:
        for batch in (1, 2):
            for group, G in ((None, 1), (np.arange(n), n)):
                got, _, _ = d.run(edges, cols, batch, group, G)
                _equal(got, _want(plan, members, group, G, edges, batch, cols), f"B = {batch}, {G} groups")
                assert (got["batches"] == cap // batch).all() and got["trunc"].any() and (got["trunc"] < got["batches"][:, :, None] // 2).all()
                rows = sum(m[cols[0]].astype(object) for m in (members if G == 1 else members[:1]))
                y = [int(v) for v in rows.reshape(-1, batch).sum(axis=1)]
                assert warmup_truncation(y)[0] == got["trunc"][0, 0, 0]
                bits.append(_largest_product(y).bit_length())
    finally:
        d.close()
    print(f"largest compared products: {bits} bits")
    assert min(bits) > 128 and max(bits) < 253


# ------------------------------------------------------------------------------------ 4. NULL outputs, scratch
def test_null_outputs_are_skipped():
    plan = _plan("single_server")
    rng = np.random.default_rng(2)
    n, cap = 9, 300
    blk, counts = _big_block(plan, rng, n, cap, np.array([300, 300, 299, 350, 300, 120, 300, 300, 300]))
    cols = _columns(plan, True)
    d = _Device(plan, blk, counts)
    try:
        for edges in (np.array([0, 100, 200, 300]), np.arange(0, 301, 15)):
            for group, G in ((np.arange(n) % 2, 2), (np.arange(n), n)):
                _, full, _ = d.run(edges, cols, 5, group, G)
                for outputs in (("batches", "trunc"), ("batches", "trunc", "s1"), ("batches", "trunc", "s2", "s2_all"),
                                ("batches", "trunc", "s1_all"), ("batches", "trunc", "s1", "s2", "s1_all")):
                    got, raw, _ = d.run(edges, cols, 5, group, G, outputs=outputs)
                    assert set(got) == set(outputs)        # (run() asserts that the guard words and the skipped outputs stay)
                    for k in outputs:
                        assert raw[k] == full[k], (outputs, k)
    finally:
        d.close()


def test_scratch_stays_within_the_bound_of_the_header():
    """include/asyncflow_hip.h: 8 B per (group, column, batch) -- batch over sum_w floor((min(b[w + 1], cap) - min(b[w], cap)) /
    B) --, 4 B per (group, window), 8 B per edge, 4 B per column + 1 280 B of alignment."""
    plan = _plan("fanout8")
    rng = np.random.default_rng(3)
    n, cap = 40, 400
    blk, counts = _hist_block(plan, rng, n, cap, rng.integers(0, cap + 1, n))
    cols = _columns(plan, True)
    edges = np.array([0, 20, 41, 200, 390, 450, 900])
    W, Cn = len(edges) - 1, len(cols)
    for batch in (5, 1, 64):
        n_batches = int((np.diff(np.minimum(edges, cap)) // batch).sum())
        for group, G in ((np.arange(n) % 7, 7), (np.arange(n) * 3, 3 * n)):
            d = _Device(plan, blk, counts)                          # (a fresh engine: the scratch of this call alone)
            try:
                _, _, scratch = d.run(edges, cols, batch, group, G)
            finally:
                d.close()
            sums = 8 * G * Cn * n_batches
            bound = sums + 4 * G * W + 8 * (W + 1) + 4 * Cn + 1280
            print(f"B = {batch}, {G} groups: scratch_bytes {scratch}, bound {bound}")
            assert sums < scratch <= bound
            assert sums <= 8 * max(G, n) * Cn * (cap // batch)      # at most 8 B per (scenario or group, column, batch)


# ------------------------------------------------------------------------------------ 5. refusals
def test_device_argument_checks():
    """Error codes from calls that return before anything is written: no output word is touched."""
    import torch

    from asyncflow_amd.engine import PLAN_ONLY, Engine, load_library

    plan = _plan("lb_two_servers")
    S = plan.n_series
    ram = np.nonzero(ram_columns(S, plan.n_edges))[0]
    rng = np.random.default_rng(1)
    blk, counts = _hist_block(plan, rng, 3, 50, [50, 20, 50])
    lib = load_library()
    dev = torch.device("cuda", 0)
    blk_t = torch.as_tensor(blk.view(np.int32), device=dev)
    counts_t = torch.as_tensor(counts.view(np.int32), device=dev)
    bad_group = torch.as_tensor(np.array([0, 2, 0], dtype=np.int32), device=dev)
    outs = torch.full((16 * 1024,), PATTERN, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    eng, planner = Engine(plan, 0), Engine(plan, PLAN_ONLY)
    pu = C.POINTER(C.c_uint32)
    try:
        def call(edges, cols=(0, 1), n_columns=None, batch=5, samples=True, counts_p=counts_t, n_windows=None, cap=50, engine=eng,
                 n_groups=2, group=None, batches=True, trunc=True, columns=True, n=3):
            e = (C.c_uint32 * len(edges))(*edges) if edges is not None else None
            arr = (C.c_uint32 * max(len(cols), 1))(*cols)
            out = _abi.AfOutputs(0, None, cap, C.c_void_p(blk_t.data_ptr() if samples else None),
                                 C.c_void_p(counts_p.data_ptr() if counts_p is not None else None))
            base = outs.data_ptr()
            req = _abi.AfSeriesWarmup(
                n, n_groups, (len(edges) - 1 if n_windows is None else n_windows), C.c_void_p(group.data_ptr() if group is not None else None),
                C.cast(e, pu) if e is not None else None, len(cols) if n_columns is None else n_columns, C.cast(arr, pu) if columns else None,
                batch, C.c_void_p(base) if batches else None, C.c_void_p(base + 4096) if trunc else None, C.c_void_p(base + 8192),
                C.c_void_p(base + 12288), C.c_void_p(base + 16384), C.c_void_p(base + 20480), 0.0, 0)
            rc = lib.af_engine_summarize_series_warmup(engine._h, C.byref(out), C.byref(req))  # noqa: SLF001
            return rc, lib.af_last_error().decode()

        INV, CAPACITY = _abi.AF_ERR_INVALID, _abi.AF_ERR_CAPACITY
        refused = [
            (call([0, 10], batch=0), INV, "batch must be at least 1"),
            (call([0, 10], columns=False), INV, "columns is required"),
            (call([0, 10], cols=(0, int(ram[0]))), INV, "ram_in_use"),
            (call([0, 10], cols=(int(ram[-1]),)), INV, "ram_in_use"),
            (call([0, 10], cols=()), INV, "n_columns"),
            (call([0, 10], cols=[0] * 65), INV, "n_columns"),
            (call([0, 10], cols=(0, S)), INV, "names series"),
            (call([0, 10], cols=(S + 7,)), INV, "names series"),
            (call(None, n_windows=1), INV, "tick_edges"),
            (call([0, 10, 10]), INV, "strictly increasing"),
            (call([10, 5]), INV, "strictly increasing"),
            (call([0], n_windows=0), INV, "n_windows"),
            (call([0, 10], n=0), INV, "n_scenarios"),
            (call([0, 10], group=bad_group), INV, "group id out of range"),
            (call([0, 10], samples=False), INV, "samples"),
            (call([0, 10], counts_p=None), INV, "counts"),
            (call([0, 10], batches=False), INV, "batches and trunc"),
            (call([0, 10], trunc=False), INV, "batches and trunc"),
            (call([0, 10], batch=0x80000000), CAPACITY, "n_scenarios * batch"),
            (call([0, 10], batch=0xFFFFFFFF), CAPACITY, "n_scenarios * batch"),
            (call([0, 0x7FFFFFFF], cap=0x7FFFFFFF, batch=1, n_groups=1), CAPACITY, "2^25 or more batches"),
            (call([0, 5, 5 + (1 << 26)], cap=0x7FFFFFFF, batch=2, n_groups=1), CAPACITY, "window 1 holds 2^25"),
            (call([0, 10], n_groups=0xFFFFFFFF), CAPACITY, "2^32 - 1"),
            (call([0, 10], cap=0x80000000), CAPACITY, "2^31"),
            (call([0, 10], engine=planner), _abi.AF_ERR_NO_DEVICE, "planning-only"),
        ]
        for i, ((rc, msg), code, reason) in enumerate(refused):
            assert rc == code and reason in msg, (i, rc, msg, code, reason)
        torch.cuda.synchronize(dev)
        assert (outs.cpu().numpy().view(np.uint32) == PATTERN).all(), "a refused call touched an output"
        # the limits themselves are accepted: n * B = 2^32 exactly is refused only past it (3 scenarios: 3 * 0x55555555 < 2^32)
        assert call([0, 10], n_groups=1, batch=0x55555555)[0] == _abi.AF_OK
        assert call([0, 10, 50], n_groups=1, batch=5)[0] == _abi.AF_OK
        host = outs.cpu().numpy().view(np.uint32)
        assert host[:3].tolist() == [2, 2, PATTERN] and host[1024 + 4] == PATTERN           # member 1 stored 20 rows: min(8, 2)
        want = series_warmup_sums([np.ascontiguousarray(blk[s, :m, :S].T) for s, m in enumerate((50, 20, 50))], [0, 10, 50], plan.n_edges, 5, [0, 1])
        assert host[1024:1028].tolist() == want["trunc"].reshape(-1).tolist()
    finally:
        eng.close()
        planner.close()


# ------------------------------------------------------------------------------------ 6. through the Python API
@pytest.fixture(scope="module")
def event_run():
    from asyncflow_amd.runner import SimulationRunner

    payload = lb_with_events(horizon=60, scale=0.1)
    seeds = 0xE7C50000 + np.arange(48, dtype=np.uint64)
    res = SimulationRunner(simulation_input=payload, seeds=seeds).run()
    words = [np.ascontiguousarray(res[s]._samples).view(np.uint32) for s in range(len(res))]  # noqa: SLF001
    return res, np.arange(48) % 4, words


def _bits(x) -> bytes:
    return np.ascontiguousarray(x, dtype=np.float64).tobytes()


def test_event_workload_through_the_python_api(event_run, tmp_path):
    res, ids, words = event_run
    names = res.series_names()
    ne, period, T = res.plan.n_edges, res.plan.sample_period, res.plan.tick_count
    ints = np.nonzero(~ram_columns(len(names), ne))[0]
    down = int(round(18.0 / period))                                # srv-1 goes down at 18 s and comes back at 24 s
    shapes = [None, np.array([0, down, int(round(24.0 / period)), T])]
    for edges in shapes:
        b = np.array([0, max(T, 1)]) if edges is None else edges
        for by, gid, G in ((None, np.zeros(48, dtype=np.int64), 1), (ids, ids, 4), ("scenario", np.arange(48), 48)):
            got = res.series_warmup_summary(5, tick_edges=edges) if by is None else res.series_warmup_summary(5, tick_edges=edges, by=by)
            per = [series_warmup_sums([words[s] for s in np.nonzero(gid == g)[0]], b, ne, 5, ints) for g in range(G)]
            want = {k: np.stack([p[k] for p in per]) for k in OUTPUTS}
            _equal({k: got[k] for k in OUTPUTS}, want, f"by {G} groups")
            st = series_warmup_statistics(want, 5, np.full(G, 48 // G), period, b)
            for k in WARMUP_STATISTICS:
                assert _bits(got[k]) == _bits(st[k]), k
            assert np.array_equal(got["converged"], st["converged"]) and np.array_equal(got["warmup_tick"], st["warmup_tick"])
            assert _bits(got["cut"]) == _bits(series_warmup_cut(st)) and got["series"] == [names[j] for j in ints]
            assert got["replicas"].tolist() == [48 // G] * G and got["series_warmup_ms"] > 0 and got["scratch_bytes"] > 0 and got["calls"] == 1
            assert np.array_equal(got["tick_edges"], b) and np.array_equal(got["times"], b[:-1] * period)
        assert (got["batches"] > 0).all() and got["converged"].any()
    mine = res[5].get_series_warmup(5, tick_edges=shapes[1])
    for k in OUTPUTS:
        assert (got[k][5] == mine[k]).all(), k
    # a selection by name with a duplicate, another batch
    sel = ["srv-1:ready_queue_len", "srv-2:event_loop_io_sleep", "srv-1:ready_queue_len"]
    part = res.series_warmup_summary(7, tick_edges=shapes[1], by=ids, series=sel)
    full = res.series_warmup_summary(7, tick_edges=shapes[1], by=ids)
    for c, nm in enumerate(sel):
        assert (part["trunc"][:, :, c] == full["trunc"][:, :, full["series"].index(nm)]).all()
    # bands over the replicas
    per = res.series_warmup_summary(5, tick_edges=shapes[1], by="scenario")
    pooled = res.series_warmup_summary(5, tick_edges=shapes[1], by=ids)
    bands = res.series_warmup_bands(5, tick_edges=shapes[1], by=ids, level=0.9, q=(0.1, 0.75))
    assert bands["mean"].shape == (4, 3, len(ints)) and bands["series"] == pooled["series"]
    assert _bits(bands["pooled"]) == _bits(pooled["warmup_s"]) and np.array_equal(bands["pooled_converged"], pooled["converged"])
    for g in range(4):
        mem = per["warmup_s"][ids == g]
        np.testing.assert_allclose(bands["mean"][g], mem.mean(axis=0), rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(bands["q_hi"][g], np.quantile(mem, 0.75, axis=0), rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(bands["converged_share"][g], per["converged"][ids == g].mean(axis=0), rtol=1e-15)
    assert (bands["n"] == 12).all()
    # the saved file
    for ext in ("npz", "parquet"):
        if ext == "parquet":
            try:
                import pyarrow  # noqa: F401
            except ImportError:
                continue
        path = str(tmp_path / f"series_warmup.{ext}")
        written = res.save_series_warmup_summary(path, ids, batch=5, tick_edges=shapes[1], series=sel[:2])
        back = load_summary(path)
        assert set(back) == set(written)
        for k, v in written.items():
            assert np.array_equal(np.asarray(back[k], dtype=v.dtype), v, equal_nan=True), k
        assert back["replicas"].tolist() == [12] * 4 and np.array_equal(back["series_warmup_batches"], pooled["batches"])
        for nm in sel[:2]:
            c = pooled["series"].index(nm)
            assert _bits(back[f"series_warmup_s:{nm}"]) == _bits(pooled["warmup_s"][:, :, c])
            assert np.array_equal(back[f"series_warmup_tick:{nm}"], pooled["warmup_tick"][:, :, c])
        assert np.array_equal(back["series_warmup_tick_edges"], shapes[1])
