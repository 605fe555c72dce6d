"""Combinations across the sampled series per (group, window of ticks, combination) on the MI355X
(af_engine_summarize_series_combined): synthetic sample blocks handed straight to the entry -- the padding words and the rows at
or past a scenario's ticks hold 0xFFFFFFFF, which shows as a max of 2^32 - 1, a wrong sum or a broken under + sum(hist) + over
== count if it is read -- with every output in one buffer between sentinels.  The reference is the host definition: the
per-tick values are results.series_combined_values of every scenario; the cells are reduced from them with exact integer
arithmetic (a ram value of these blocks is a multiple of 2^-45, so its sums are kept exactly as two integers).  Every integer
is compared with ==, min / max and the integer means on their bits; the mean of a ram combination on its bits wherever every
value of the cell is a multiple of 1/256 (every partial sum is exact), else within (count - 1) * 2^-53 relative of the exactly
rounded sum / count.

n = 23 scenarios of capacity 700 (0 ticks, all, more than stored, 1 among them); the plans of 32, 21 and 5 rows a step and
every wide plan on every window shape and grouping; one column, two of one 16-byte group, the first and the last group, all
integer, all ram, every third, and for rows of more than 64 groups sets across and past the 64th; all four ops on each."""

from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest

from asyncflow_amd import _abi
from asyncflow_amd.results import load_summary, series_combined_values, series_histogram_quantiles, tick_window_edges
from oracle.scenarios import lb_with_events
from tests.test_gpu_series_histogram import FILL, N, CAP, _hist_block
from tests.test_gpu_series_windows import WIDE, _block, _groupings, _plan, _shapes, _ticks, _wide_plan, _wide_shapes, ram_columns
from tests.test_series_combined_cpu import _pooled_host

pytestmark = pytest.mark.gpu

PATTERN = 0x5A5A5A5A
OPS = ("sum", "min", "max", "spread")
U32 = ("count", "above", "hist", "under", "over")
F64 = ("mean", "min", "max")
WIDTHS = (1.0, 3.0, 0.25, 0.1, 1.0 / 3.0)
SCALE = 2 ** 45                      # the ram values of the synthetic blocks are multiples of 2^-45


def _big_block(plan, rng, n, cap, ticks):
    """_hist_block with integer words that reach 2^31 and 2^32 - 2: sums of three or more columns pass 2^32."""
    blk, counts = _hist_block(plan, rng, n, cap, ticks)
    S = plan.n_series
    ints = np.nonzero(~ram_columns(S, plan.n_edges))[0]
    u = rng.random((n, cap, len(ints)))
    big = np.where(u < 0.3, 0xFFFFFFFE, rng.integers(2 ** 31, 2 ** 32 - 1, (n, cap, len(ints)))).astype(np.uint32)
    keep = blk[:, :, ints]
    blk[:, :, ints] = np.where(u < 0.6, big, keep)
    for s in range(n):
        blk[s, min(int(counts[s, _abi.CNT_TICKS]), cap):] = FILL
    return blk, counts


def _column_sets(plan):
    """(name, columns): one column; two of one 16-byte group; the first and the last group of a row; all integer; all ram;
    every third; and for rows of more than 64 groups a set that straddles the 64th group and one wholly past it."""
    S = plan.n_series
    ram = ram_columns(S, plan.n_edges)
    ints, rams = np.nonzero(~ram)[0], np.nonzero(ram)[0]
    pair = next([j, j + 1] for j in range(S - 1) if j // 4 == (j + 1) // 4 and not ram[j] and not ram[j + 1])
    sets = [("one column", [int(ints[1])]), ("one ram column", [int(rams[0])]), ("one group", pair),
            ("first and last group", [int(ints[0]), int(ints[-1])]), ("first and last ram", [int(rams[0]), int(rams[-1])]),
            ("all integer", ints.tolist()), ("all ram", rams.tolist()), ("every third", ints[::3].tolist()), ("every third ram", rams[::3].tolist())]
    sets = [(what, sorted(set(cols))) for what, cols in sets]          # (a plan of one server has one ram column)
    assert rams[-1] == S - 1 and (S - 1) // 4 == plan.series_pitch // 4 - 1 and ints[0] // 4 == 0
    if plan.series_pitch // 4 > 64:
        for kind, cols in (("integer", ints), ("ram", rams)):
            past = cols[cols >= 256]
            if len(past):
                sets += [(f"across the passes, {kind}", [int(cols[0]), int(cols[cols < 256][-1]), *past.tolist()]), (f"past the 64th group, {kind}", past.tolist())]
        assert len(sets) > 9
    return sets


def _combos(plan):
    combos = [(op, np.asarray(cols, dtype=np.int64)) for _, cols in _column_sets(plan) for op in OPS]
    assert len(combos) <= _abi.MAX_SERIES_COMBINATIONS
    return combos


def _binning(combos, rng):
    Cn = len(combos)
    thr = np.array([(0.0, 1.0, 0.5, -1.0, 64.0, 2.0 ** 32)[c % 6] for c in range(Cn)])
    lo = np.array([(0.0, 2.0, -1.0, 0.5, 3.0)[(c // 5) % 5] for c in range(Cn)])
    width = np.array([WIDTHS[c % 5] for c in range(Cn)])
    return thr, lo, width


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

    def run(self, edges, combos, group=None, n_groups=1, thr=None, bins=0, lo=None, width=None, outputs=None):
        """The requested outputs (u32 arrays, f64 arrays) and scratch_bytes; every output has its place in one buffer between
        sentinels, and no word outside the requested ones may change."""
        torch = self.torch
        W, Cn = len(edges) - 1, len(combos)
        outputs = outputs or (("count", "mean", "min", "max", "above") + (("hist", "under", "over") if bins else ()))
        shape = {"count": (n_groups, W), "hist": (n_groups, W, Cn, bins)}
        shape.update({k: (n_groups, W, Cn) for k in ("mean", "min", "max", "above", "under", "over")})
        guard, at, off = 64, 64, {}
        for k in (*F64, *U32):
            off[k] = at
            words = int(np.prod(shape[k])) * (2 if k in F64 else 1)
            at += words + (words & 1) + guard                 # (even offsets: the f64 outputs are 8-byte aligned)
        assert at * 4 < 72 << 20, "an output buffer of a test stays below about 64 MB"
        buf = torch.full((at,), PATTERN, dtype=torch.int32, device=self.dev)
        grp_t = None
        if group is not None:
            ids = np.asarray(group, dtype=np.int64)
            grp_t = torch.as_tensor(np.where(ids < 0, _abi.POOL_SKIP, ids).astype(np.uint32).view(np.int32), device=self.dev)
        torch.cuda.synchronize(self.dev)                      # (the engine has a stream of its own)
        ptr = {"mean": "mean_ptr", "min": "min_ptr", "max": "max_ptr"}
        _, scratch = self.eng.summarize_series_combined(
            self.n, n_groups, edges, [_abi.COMBINE_OPS[op] for op, _ in combos], [c for _, c in combos], samples_ptr=self.blk_t.data_ptr(),
            tick_capacity=self.cap, counts_ptr=self.counts_t.data_ptr(), group_ptr=0 if grp_t is None else grp_t.data_ptr(), thresholds=thr,
            bins=bins, lo=lo, width=width, **{ptr.get(k, f"{k}_ptr"): buf.data_ptr() + 4 * off[k] for k in outputs})
        host = buf.cpu().numpy().view(np.uint32)
        written = np.zeros(at, dtype=bool)
        out = {}
        for k in outputs:
            words = int(np.prod(shape[k])) * (2 if k in F64 else 1)
            written[off[k]:off[k] + words] = True
            part = host[off[k]:off[k] + words]
            out[k] = (part.view(np.float64) if k in F64 else part).reshape(shape[k])
        assert (host[~written] == PATTERN).all(), f"a word outside the requested outputs {outputs} was written"
        return out, scratch


def _keys(x):
    bits = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(bits >> np.uint64(63) != 0, ~bits, bits | np.uint64(1 << 63))


def _unkeys(k):
    return np.where(k >> np.uint64(63) != 0, k & np.uint64((1 << 63) - 1), ~k).astype(np.uint64).view(np.float64)


def _reduceat(fn, arr, r):
    padded = np.concatenate([arr, np.zeros((arr.shape[0], 1), dtype=arr.dtype)], axis=1)
    return fn.reduceat(padded, r, axis=1)[:, :-1]


def _tick_values(plan, blk, counts, combos):
    """Per scenario the host definition's per-tick values of every combination: (V uint64 [C, m], X float64 [C, m])."""
    out = []
    for s in range(blk.shape[0]):
        m = min(int(counts[s, _abi.CNT_TICKS]), blk.shape[1])
        words = np.ascontiguousarray(blk[s, :m, :plan.n_series].T)
        V, X = np.zeros((len(combos), m), dtype=np.uint64), np.zeros((len(combos), m))
        for c, (op, cols) in enumerate(combos):
            v = series_combined_values(words, plan.n_edges, op, cols)
            if v.dtype == np.uint64:
                V[c] = v
            X[c] = v.astype(np.float64)
        out.append((V, X))
    return out


def _want(plan, values, combos, edges, groupings, thr=None, bins=0, lo=None, width=None, fsum=False):
    """The cells of every (group ids, n_groups, ...) of `groupings` from the per-tick values; see the module docstring.
    fsum=True (ram values that are no multiples of 2^-45): the ram means by math.fsum over the cell's values."""
    Cn = len(combos)
    is_ram = np.array([bool(ram_columns(plan.n_series, plan.n_edges)[c[0]]) for _, c in combos])
    b = np.asarray(edges, dtype=np.int64)
    W = len(b) - 1
    thr = np.zeros(Cn) if thr is None else np.asarray(thr, dtype=np.float64)
    lo = np.zeros(Cn) if lo is None else np.broadcast_to(np.asarray(lo, dtype=np.float64), (Cn,))
    width = np.ones(Cn) if width is None else np.broadcast_to(np.asarray(width, dtype=np.float64), (Cn,))
    accs = []
    for _, G, *_ in groupings:
        accs.append({"count": np.zeros((G, W), dtype=np.int64), "isum": np.zeros((G, W, Cn), dtype=np.uint64), "hi": np.zeros((G, W, Cn), dtype=np.int64),
                     "lo": np.zeros((G, W, Cn), dtype=np.int64), "fine": np.zeros((G, W, Cn), dtype=np.int64),
                     "kmn": np.full((G, W, Cn), 2 ** 64 - 1, dtype=np.uint64), "kmx": np.zeros((G, W, Cn), dtype=np.uint64),
                     "above": np.zeros((G, W, Cn), dtype=np.int64), "table": np.zeros((G, W, Cn, bins + 2), dtype=np.int64),
                     "terms": [[[] for _ in range(W)] for _ in range(G)] if fsum else None})
    for s, (V, X) in enumerate(values):
        m = X.shape[1]
        r = np.minimum(b, m)
        cnt = np.diff(r)
        live = (cnt > 0)[None, :]
        part = {"count": cnt, "isum": np.where(live, _reduceat(np.add, V, r), 0).T.astype(np.uint64)}
        whole = np.floor(X)
        frac = (X - whole) * float(SCALE)
        if not fsum:
            assert (frac[is_ram] == np.floor(frac[is_ram])).all(), "the ram values of this block are no multiples of 2^-45"
        part["hi"] = np.where(live, _reduceat(np.add, np.where(is_ram[:, None], whole, 0).astype(np.int64), r), 0).T
        part["lo"] = np.where(live, _reduceat(np.add, np.where(is_ram[:, None], frac, 0).astype(np.int64), r), 0).T
        part["fine"] = np.where(live, _reduceat(np.add, (X * 256.0 != np.floor(X * 256.0)).astype(np.int64), r), 0).T
        keys = _keys(X)
        part["kmn"] = np.where(live, _reduceat(np.minimum, keys, r), np.uint64(2 ** 64 - 1)).T
        part["kmx"] = np.where(live, _reduceat(np.maximum, keys, r), np.uint64(0)).T
        part["above"] = np.where(live, _reduceat(np.add, (X > thr[:, None]).astype(np.int64), r), 0).T
        if bins:
            xs = X[:, r[0]:r[-1]]
            below = xs < lo[:, None]
            t = (xs - lo[:, None]) / width[:, None]
            past = ~below & (t >= float(bins))
            entry = np.where(below, bins, np.where(past, bins + 1, np.where(below | past, 0.0, t).astype(np.int64)))
            win = np.searchsorted(r, np.arange(r[0], r[-1]), side="right") - 1
            flat = (win[None, :] * Cn + np.arange(Cn)[:, None]) * (bins + 2) + entry
            part["table"] = np.bincount(flat.ravel(), minlength=W * Cn * (bins + 2)).reshape(W, Cn, bins + 2)
        for (ids, _G, *_), acc in zip(groupings, accs):
            g = 0 if ids is None else int(ids[s])
            if g < 0:
                continue
            for k in ("count", "isum", "hi", "lo", "fine", "above"):
                acc[k][g] += part[k]
            acc["kmn"][g] = np.minimum(acc["kmn"][g], part["kmn"])
            acc["kmx"][g] = np.maximum(acc["kmx"][g], part["kmx"])
            if bins:
                acc["table"][g] += part["table"]
            if fsum:
                for w in np.nonzero(cnt > 0)[0]:
                    acc["terms"][g][w].append(X[:, r[w]:r[w + 1]])
    outs = []
    for acc in accs:
        count = acc["count"]
        empty = count == 0
        n = count[:, :, None].astype(np.float64)
        exact = acc["hi"].astype(object) * SCALE + acc["lo"].astype(object)                 # the ram sums as Python integers
        ram_sum = np.array([0.0 + t / SCALE for t in exact.ravel()], dtype=np.float64).reshape(exact.shape)   # (int / int: correctly rounded)
        if fsum:
            for g, w in np.argwhere(~empty):
                cell = np.concatenate(acc["terms"][g][w], axis=1)
                ram_sum[g, w] = [0.0 + math.fsum(row.tolist()) for row in cell]
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = np.where(is_ram, ram_sum, acc["isum"].astype(np.float64)) / n
        mean[empty] = np.nan
        mn, mx = _unkeys(acc["kmn"]), _unkeys(acc["kmx"])
        mn[empty] = mx[empty] = np.nan
        out = {"count": count, "mean": mean, "min": mn, "max": mx, "above": acc["above"], "exact": (acc["fine"] == 0) & (not fsum), "is_ram": is_ram}
        if bins:
            out.update(hist=acc["table"][..., :bins], under=acc["table"][..., bins], over=acc["table"][..., bins + 1])
        outs.append(out)
    return outs


def _equal(got, want, what, stats=None):
    for k in U32:
        if k in got:
            assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
            g = got[k].astype(np.int64)
            assert np.array_equal(g, want[k]), (what, k, np.argwhere(g != want[k])[:5], g[g != want[k]][:5], want[k][g != want[k]][:5])
    for k in ("min", "max"):
        if k in got:
            d = got[k].view(np.uint64) != want[k].view(np.uint64)
            d &= ~(np.isnan(got[k]) & np.isnan(want[k]))
            assert not d.any(), (what, k, np.argwhere(d)[:5], got[k][d][:5], want[k][d][:5])
    if "mean" in got:
        gm, wm = got["mean"], want["mean"]
        empty = (want["count"] == 0)[:, :, None]
        assert np.isnan(gm[np.broadcast_to(empty, gm.shape)]).all(), what
        bitwise = (~want["is_ram"][None, None, :] | want["exact"]) & ~empty
        d = (gm.view(np.uint64) != wm.view(np.uint64)) & bitwise
        assert not d.any(), (what, "mean", np.argwhere(d)[:5], gm[d][:5], wm[d][:5])
        loose = ~bitwise & ~empty
        if loose.any():
            n = np.broadcast_to(want["count"][:, :, None].astype(np.float64), gm.shape)
            err, bound = np.abs(gm - wm)[loose], ((n - 1.0) * 2.0 ** -53 * np.abs(wm))[loose]
            worst = float(np.max(err / np.maximum(bound, 1e-300))) if (err > 0).any() else 0.0
            print(f"{what}: {int(loose.sum())} ram means with inexact partial sums, largest error / ((count - 1) 2^-53 |mean|) = {worst:.3g}")
            assert (err <= bound).all(), (what, "ram mean", np.argwhere(loose)[err > bound][:5], gm[loose][err > bound][:5], wm[loose][err > bound][:5])
        if stats is not None:
            stats += [int(bitwise[:, :, want["is_ram"]].sum()), int(loose.sum())]
    if "hist" in got and "under" in got and "over" in got and "count" in got:
        total = got["under"].astype(np.int64) + got["hist"].astype(np.int64).sum(axis=-1) + got["over"]
        assert np.array_equal(total, np.broadcast_to(got["count"].astype(np.int64)[:, :, None], total.shape)), (what, "under + hist + over != count")


def _check_plan(plan, name, blk, counts, shapes, rng, bins=16):
    combos = _combos(plan)
    thr, lo, width = _binning(combos, rng)
    values = _tick_values(plan, blk, counts, combos)
    seen = np.zeros(5, dtype=np.int64)
    d = _Device(plan, blk, counts)
    try:
        for what, edges in shapes:
            groupings = _groupings(N)
            b = bins
            if what == "one tick each":                 # (the other groupings with a histogram: outputs of more than 64 MB)
                groupings = [g for g in groupings if g[2] in ("interleaved", "one group (NULL)")]
            wants = _want(plan, values, combos, edges, groupings, thr, b, lo, width)
            for (group, n_groups, gname), want in zip(groupings, wants):
                got, _ = d.run(edges, combos, group, n_groups, thr, b, lo, width)
                _equal(got, want, f"{name}, {what}, {gname}")
                seen += [int((want["under"] > 0).sum()), int((want["over"] > 0).sum()), int((want["count"] == 0).sum()),
                         int((want["above"] > 0).sum()), int((np.nan_to_num(want["max"]) >= 2.0 ** 32).sum())]
            if what == "one tick each":                 # singletons without the histogram
                group, n_groups, gname = next(g for g in _groupings(N) if g[2] == "singletons")
                got, _ = d.run(edges, combos, group, n_groups, thr)
                _equal(got, _want(plan, values, combos, edges, [(group, n_groups)], thr)[0], f"{name}, {what}, {gname}, no bins")
    finally:
        d.close()
    return seen


# ------------------------------------------------------------------------------------ 1. against the host definition
@pytest.mark.parametrize("big", [False, True], ids=["counts", "words to 2^32"])
@pytest.mark.parametrize("name", ["single_server", "lb_two_servers", "fanout8"])
def test_synthetic_blocks_equal_the_host_definition(name, big):
    plan = _plan(name)
    assert 64 // min(plan.series_pitch // 4, 64) == {"single_server": 32, "lb_two_servers": 21, "fanout8": 5}[name]
    rng = np.random.default_rng(len(name) + 100 * big)
    ticks = _ticks(rng, N, CAP)
    assert ticks[0] == 0 and ticks[1] == CAP and ticks[2] > CAP and ticks[3] == 1
    blk, counts = (_big_block if big else _hist_block)(plan, rng, N, CAP, ticks)
    seen = _check_plan(plan, name, blk, counts, _shapes(CAP), rng)
    assert (seen[:4] > 0).all() and (seen[4] > 0) == big, seen


# ------------------------------------------------------------------------------------ 2. wide plans
@pytest.mark.parametrize("name", list(WIDE))
def test_wide_rows_equal_the_host_definition(name):
    plan = _wide_plan(name)
    assert (plan.n_series, plan.series_pitch) == WIDE[name]
    rng = np.random.default_rng(plan.n_series)
    blk, counts = _big_block(plan, rng, N, CAP, _ticks(rng, N, CAP))
    if plan.series_pitch // 4 > 64:
        assert any("past the 64th group" in s[0] for s in _column_sets(plan)) and any("across the passes" in s[0] for s in _column_sets(plan))
    seen = _check_plan(plan, name, blk, counts, _wide_shapes(CAP), rng)
    assert (seen > 0).all(), seen


# ------------------------------------------------------------------------------------ 3. dyadic ram values: every mean on its bits
def test_dyadic_ram_values_every_mean_on_its_bits():
    """Multiples of 1/256 below 2^16 (no residue): every partial sum is exact, every mean is compared on its bits."""
    plan = _plan("fanout8")
    rng = np.random.default_rng(8)
    blk, counts = _block(plan, rng, N, CAP, _ticks(rng, N, CAP))
    blk[:, :, plan.n_series:] = FILL
    for s in range(N):
        blk[s, min(int(counts[s, _abi.CNT_TICKS]), CAP):] = FILL
    combos = _combos(plan)
    values = _tick_values(plan, blk, counts, combos)
    stats: list = []
    d = _Device(plan, blk, counts)
    try:
        for what, edges in _shapes(CAP):
            groupings = [g for g in _groupings(N) if what != "one tick each" or g[2] == "interleaved"]
            for (group, n_groups, gname), want in zip(groupings, _want(plan, values, combos, edges, groupings)):
                got, _ = d.run(edges, combos, group, n_groups)
                _equal(got, want, f"dyadic, {what}, {gname}", stats)
    finally:
        d.close()
    assert sum(stats[0::2]) > 0 and sum(stats[1::2]) == 0


# ------------------------------------------------------------------------------------ 4. arbitrary floats
def test_arbitrary_float_values_against_fsum_run_to_run_and_batch_independence():
    plan = _plan("lb_two_servers")
    rng = np.random.default_rng(5)
    n, cap = 8, 512
    blk, counts = _block(plan, rng, n, cap, _ticks(rng, n, cap), dyadic=False)
    combos = _combos(plan)
    values = _tick_values(plan, blk, counts, combos)
    edges = tick_window_edges(200, cap)
    for group, n_groups in ((None, 1), (np.arange(n) % 3, 3), (np.arange(n), n)):
        d = _Device(plan, blk, counts)
        try:
            got, _ = d.run(edges, combos, group, n_groups)
            again, _ = d.run(edges, combos, group, n_groups)
        finally:
            d.close()
        for k in got:
            assert got[k].tobytes() == again[k].tobytes(), k              # the same call twice: identical bytes
        _equal(got, _want(plan, values, combos, edges, [(group, n_groups)], fsum=True)[0], f"arbitrary floats, {n_groups} groups")
    # the same scenarios inside a batch ten times as large: identical bytes for their cells
    big, big_counts = _block(plan, rng, 10 * n, cap, rng.integers(0, cap + 1, 10 * n), dyadic=False)
    where = np.arange(n) * 10 + 3
    big[where], big_counts[where] = blk, counts
    d, d_big = _Device(plan, blk, counts), _Device(plan, big, big_counts)
    try:
        for edges in (tick_window_edges(200, cap), tick_window_edges(7, cap), np.array([0, cap])):
            alone, _ = d.run(edges, combos, np.arange(n), n, None, 16, 0.0, 1000.0)
            inside, _ = d_big.run(edges, combos, np.arange(10 * n), 10 * n, None, 16, 0.0, 1000.0)
            for k in alone:
                assert alone[k].tobytes() == np.ascontiguousarray(inside[k][where]).tobytes(), k
            ids = np.full(10 * n, -1)
            ids[where] = np.arange(n) % 3                                  # as members of groups: the same fold
            a, _ = d.run(edges, combos, np.arange(n) % 3, 3)
            b, _ = d_big.run(edges, combos, ids, 3)
            for k in a:
                assert a[k].tobytes() == b[k].tobytes(), k
    finally:
        d.close()
        d_big.close()


# ------------------------------------------------------------------------------------ 5. many combinations, many waves
def test_64_combinations_with_1024_bins():
    """64 combinations of 1 024 bins: 1 026 words a combination, three a pass of the kernel."""
    plan = _wide_plan("wide_fanout16")
    rng = np.random.default_rng(1024)
    blk, counts = _hist_block(plan, rng, N, CAP, _ticks(rng, N, CAP), top=300)
    S = plan.n_series
    ints = np.nonzero(~ram_columns(S, plan.n_edges))[0]
    combos = [(OPS[c % 4], np.sort(rng.choice(ints, size=1 + c % 5, replace=False))) for c in range(64)]
    values = _tick_values(plan, blk, counts, combos)
    lo, width = np.zeros(64), np.ones(64)
    lo[-1], width[-1] = 100.0, 0.5
    edges = np.array([0, 300, CAP])
    d = _Device(plan, blk, counts)
    try:
        for group, G in ((None, 1), (np.arange(N) % 2, 2)):
            got, _ = d.run(edges, combos, group, G, None, 1024, lo, width)
            want = _want(plan, values, combos, edges, [(group, G)], None, 1024, lo, width)[0]
            _equal(got, want, f"64 combinations of 1 024 bins, {G} groups")
        assert want["hist"][..., 600:].sum() > 0 and want["under"][..., -1].sum() > 0
        few, _ = d.run(edges, combos[:3], group, G, None, 1024, lo[:3], width[:3])   # a pass alone
        for k in ("mean", "min", "max", "above", "hist", "under", "over"):
            assert few[k].tobytes() == np.ascontiguousarray(got[k][:, :, :3]).tobytes(), k
    finally:
        d.close()


@pytest.mark.parametrize("name", ["lb_two_servers", "single_server"])
def test_many_waves_add_into_one_cell(name):
    """300 scenarios of 64 ticks in one group: 300 waves add into every cell -- directly (windows of at most 64 ticks) --, and
    300 scenarios of 200 ticks through their LDS histograms; work items of several windows."""
    plan = _plan(name)
    rng = np.random.default_rng(300)
    combos = _combos(plan)
    thr, lo, width = _binning(combos, rng)
    for n, cap, shapes in ((300, 64, (("one window", np.array([0, 64])), ("20 ticks", tick_window_edges(20, 64)), ("one tick each", np.arange(65)),
                                      ("uneven", np.array([1, 40, 41, 64, 90])))),
                           (300, 200, (("one window", np.array([0, 200])), ("65 ticks", tick_window_edges(65, 200))))):
        blk, counts = _hist_block(plan, rng, n, cap, _ticks(rng, n, cap), top=8)
        values = _tick_values(plan, blk, counts, combos)
        d = _Device(plan, blk, counts)
        try:
            for what, edges in shapes:
                groupings = [(None, 1), (np.arange(n) % 3, 3)]
                for (group, n_groups), want in zip(groupings, _want(plan, values, combos, edges, groupings, thr, 8, lo, width)):
                    got, _ = d.run(edges, combos, group, n_groups, thr, 8, lo, width)
                    _equal(got, want, f"{name}, {cap} ticks, {what}, {n_groups} groups")
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
    combos = _combos(plan)[:8]
    values = _tick_values(plan, blk, counts, combos)
    edges = np.arange(cap + 1)
    group = np.arange(n) % 5
    d = _Device(plan, blk, counts)
    try:
        got, _ = d.run(edges, combos, group, 5, None, 4)
    finally:
        d.close()
    _equal(got, _want(plan, values, combos, edges, [(group, 5)], None, 4)[0], "700 windows of one tick")


# ------------------------------------------------------------------------------------ 6. independence, NULL outputs, scratch
def test_a_combination_does_not_depend_on_the_others():
    plan = _plan("fanout8")
    rng = np.random.default_rng(5)
    n, cap = 8, 256
    blk, counts = _hist_block(plan, rng, n, cap, _ticks(rng, n, cap))
    combos = _combos(plan)
    thr, lo, width = _binning(combos, rng)
    d = _Device(plan, blk, counts)
    try:
        for edges in (tick_window_edges(100, cap), tick_window_edges(7, cap)):
            for group, G in ((np.arange(n), n), (np.arange(n) % 2, 2)):
                full, _ = d.run(edges, combos, group, G, thr, 16, lo, width)
                perm = rng.permutation(len(combos))
                mixed, _ = d.run(edges, [combos[i] for i in perm], group, G, thr[perm], 16, lo[perm], width[perm])
                for k in ("mean", "min", "max", "above", "hist", "under", "over"):
                    assert mixed[k].tobytes() == np.ascontiguousarray(full[k][:, :, perm]).tobytes(), k
                assert mixed["count"].tobytes() == full["count"].tobytes()
                for c in (0, 5, 26, len(combos) - 1):                                  # alone, and twice in one call
                    sel = [c, c]
                    alone, _ = d.run(edges, [combos[i] for i in sel], group, G, thr[sel], 16, lo[sel], width[sel])
                    for k in ("mean", "min", "max", "above", "hist", "under", "over"):
                        assert alone[k].tobytes() == np.ascontiguousarray(full[k][:, :, sel]).tobytes(), (k, c)
    finally:
        d.close()


def test_null_outputs_are_skipped():
    plan = _plan("single_server")
    rng = np.random.default_rng(2)
    n, cap = 9, 300
    blk, counts = _hist_block(plan, rng, n, cap, _ticks(rng, n, cap))
    combos = _combos(plan)[:10]
    d = _Device(plan, blk, counts)
    try:
        for edges in (tick_window_edges(100, cap), tick_window_edges(9, cap)):
            for group, G in ((np.arange(n) % 2, 2), (np.arange(n), n)):
                full, _ = d.run(edges, combos, group, G, None, 32, 1.0, 2.0)
                for outputs in (("mean",), ("mean", "count"), ("mean", "max"), ("mean", "min", "above"), ("mean", "hist"),
                                ("mean", "hist", "under"), ("mean", "hist", "over", "count")):
                    bins = 32 if "hist" in outputs else 0
                    got, _ = d.run(edges, combos, group, G, None, bins, 1.0 if bins else None, 2.0 if bins else None, outputs=outputs)
                    assert set(got) == set(outputs)       # (run() asserts that the guard words and the skipped outputs stay)
                    for k in got:
                        assert got[k].tobytes() == full[k].tobytes(), (outputs, k)
    finally:
        d.close()


def test_scratch_stays_within_the_bound_of_the_header():
    """include/asyncflow_hip.h: 4 B per edge + 40 B per combination + 4 B per listed column + 4 B per group + 4 B per scenario +
    2 560 B of alignment, and -- unless every group holds at most one scenario -- 36 B per (scenario, window, combination)."""
    plan = _plan("fanout8")
    rng = np.random.default_rng(3)
    n, cap = 40, 400
    blk, counts = _hist_block(plan, rng, n, cap, rng.integers(0, cap + 1, n))
    combos = _combos(plan)
    edges = tick_window_edges(20, cap)
    W, Cn, listed = len(edges) - 1, len(combos), sum(len(c) for _, c in combos)
    for group, G, records in ((np.arange(n) % 7, 7, True), (np.arange(n) * 3, 3 * n, False)):
        d = _Device(plan, blk, counts)                                  # (a fresh engine: the scratch of this call alone)
        try:
            _, scratch = d.run(edges, combos, group, G, None, 8)
        finally:
            d.close()
        bound = 4 * (W + 1) + 40 * Cn + 4 * listed + 4 * (G + 1) + 4 * n + 2560 + (36 * n * W * Cn if records else 0)
        print(f"{G} groups: scratch_bytes {scratch}, bound {bound}")
        assert (36 * n * W * Cn if records else 0) < scratch <= bound
        assert records or scratch < 36 * n * W * Cn


# ------------------------------------------------------------------------------------ 7. refusals
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
    outs = torch.full((64 * 1024,), PATTERN, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    eng, planner = Engine(plan, 0), Engine(plan, PLAN_ONLY)
    pd, pu = C.POINTER(C.c_double), C.POINTER(C.c_uint32)
    try:
        def call(edges, ops=(0, 3), lists=((0, 1), (0, 1, 3)), n_combos=None, thr=None, bins=0, lo=None, width=None, samples=True,
                 counts_p=counts_t, n_windows=None, cap=50, engine=eng, n_groups=2, group=None, mean=True, hist=None, under=False,
                 start=None):
            e = (C.c_uint32 * len(edges))(*edges) if edges is not None else None
            op = (C.c_uint32 * max(len(ops), 1))(*ops)
            st = start if start is not None else [0, *np.cumsum([len(x) for x in lists]).tolist()]
            st_a = (C.c_uint32 * len(st))(*st)
            flat = [j for x in lists for j in x]
            col = (C.c_uint32 * max(len(flat), 1))(*flat)
            arr = {k: (C.c_double * len(v))(*v) if v is not None else None for k, v in (("thr", thr), ("lo", lo), ("width", width))}
            out = _abi.AfOutputs(0, None, cap, C.c_void_p(blk_t.data_ptr() if samples else None),
                                 C.c_void_p(counts_p.data_ptr() if counts_p is not None else None))
            base = outs.data_ptr()
            want_hist = bins > 0 if hist is None else hist
            req = _abi.AfSeriesCombined(
                3, n_groups, (len(edges) - 1 if n_windows is None else n_windows), C.c_void_p(group.data_ptr() if group is not None else None),
                C.cast(e, pu) if e is not None else None, len(ops) if n_combos is None else n_combos, C.cast(op, pu), C.cast(st_a, pu), C.cast(col, pu),
                C.cast(arr["thr"], pd) if thr is not None else None, bins, C.cast(arr["lo"], pd) if lo is not None else None,
                C.cast(arr["width"], pd) if width is not None else None, C.c_void_p(base), C.c_void_p(base + 4096) if mean else None,
                C.c_void_p(base + 8192), C.c_void_p(base + 12288), C.c_void_p(base + 16384), C.c_void_p(base + 65536) if want_hist else None,
                C.c_void_p(base + 20480) if (want_hist or under) else None, C.c_void_p(base + 24576) if want_hist else None, 0.0, 0)
            rc = lib.af_engine_summarize_series_combined(engine._h, C.byref(out), C.byref(req))  # noqa: SLF001
            return rc, lib.af_last_error().decode()

        nan, inf = float("nan"), float("inf")
        INV, CAPACITY = _abi.AF_ERR_INVALID, _abi.AF_ERR_CAPACITY
        refused = [
            (call([0, 10], ops=(), lists=()), INV, "n_combos"),
            (call([0, 10], ops=[0] * 65, lists=[(0,)] * 65), INV, "n_combos"),
            (call([0, 10], ops=(0, 4)), INV, "unknown op"),
            (call([0, 10], lists=((0, 1), ())), INV, "no columns"),
            (call([0, 10], lists=((0, 1), (3, 1))), INV, "strictly increasing"),
            (call([0, 10], lists=((0, 1), (1, 1))), INV, "strictly increasing"),
            (call([0, 10], lists=((0, 1), (1, S))), INV, "names series"),
            (call([0, 10], lists=((0, 1), (0, int(ram[0])))), INV, "mixes"),
            (call([0, 10], lists=((0, 1), (int(ram[0]) - 1, int(ram[0]), int(ram[1])))), INV, "mixes"),
            (call([0, 10], start=[1, 2, 4]), INV, "col_start"),
            (call([0, 10], thr=[0.0, nan]), INV, "NaN"),
            (call([0, 10], bins=1025), INV, "n_bins"),
            (call([0, 10], bins=8, lo=[0.0, 0.0], width=[1.0, 0.0]), INV, "width"),
            (call([0, 10], bins=8, lo=[0.0, 0.0], width=[-1.0, 1.0]), INV, "width"),
            (call([0, 10], bins=8, lo=[0.0, 0.0], width=[1.0, nan]), INV, "width"),
            (call([0, 10], bins=8, lo=[0.0, 0.0], width=[inf, 1.0]), INV, "width"),
            (call([0, 10], bins=8, lo=[0.0, nan], width=[1.0, 1.0]), INV, "lo"),
            (call([0, 10], bins=8, lo=[-inf, 0.0], width=[1.0, 1.0]), INV, "lo"),
            (call([0, 10], bins=8, lo=[0.0, 0.0]), INV, "together"),
            (call([0, 10], bins=8, width=[1.0, 1.0]), INV, "together"),
            (call([0, 10], bins=0, hist=True), INV, "given together"),
            (call([0, 10], bins=0, under=True), INV, "given together"),
            (call([0, 10], bins=8, hist=False), INV, "given together"),
            (call(None, n_windows=1), INV, "tick_edges"),
            (call([0, 10, 10]), INV, "strictly increasing"),
            (call([10, 5]), INV, "strictly increasing"),
            (call([0], n_windows=0), INV, "n_windows"),
            (call([0, 10], group=bad_group), INV, "group id out of range"),
            (call([0, 10], samples=False), INV, "samples"),
            (call([0, 10], counts_p=None), INV, "counts"),
            (call([0, 10], mean=False), INV, "mean"),
            (call([0, 0x7FFFFFFF], counts_p=huge_t, cap=0x7FFFFFFF, n_groups=1), CAPACITY, "2^32 or more"),
            (call([0, 0x7FFFFFFF], counts_p=huge_t, cap=0x7FFFFFFF, n_groups=3, group=torch.as_tensor(np.arange(3, dtype=np.int32), device=dev)),
             CAPACITY, "longest column list"),
            (call([0, 10], n_groups=0xFFFFFFFF), CAPACITY, "2^32 - 1"),
            (call([0, 10], cap=0x80000000), CAPACITY, "2^31"),
            (call([0, 10], engine=planner), _abi.AF_ERR_NO_DEVICE, "planning-only"),
        ]
        for i, ((rc, msg), code, reason) in enumerate(refused):
            assert rc == code and reason in msg, (i, rc, msg, code, reason)
        torch.cuda.synchronize(dev)
        assert (outs.cpu().numpy().view(np.uint32) == PATTERN).all(), "a refused call touched an output"
        assert call([0, 10], n_groups=1, bins=8)[0] == _abi.AF_OK
        host = outs.cpu().numpy().view(np.uint32)
        assert host[0] == 10 + 10 + 0 and host[1] == PATTERN
        assert host[16384:16384 + 2 * 8].sum() + host[5120:5122].sum() + host[6144:6146].sum() == 2 * 20     # under + hist + over == count, twice
    finally:
        eng.close()
        planner.close()


# ------------------------------------------------------------------------------------ 8. through the Python API
COMBOS = {"imbalance": ("spread", "*:ready_queue_len"), "queued": ("sum", "*:ready_queue_len"), "fleet_ram": ("sum", "*:ram_in_use"),
          "open": ("sum", "*:edge_concurrent_connection"), "ram_gap": ("spread", "*:ram_in_use"), "busiest": ("max", ["*:ready_queue_len", "*:event_loop_io_sleep"])}


@pytest.fixture(scope="module")
def event_run():
    from asyncflow_amd.runner import SimulationRunner

    payload = lb_with_events(horizon=60, scale=0.1)
    seeds = 0xE7C50000 + np.arange(12, dtype=np.uint64)
    res = SimulationRunner(simulation_input=payload, seeds=seeds).run()
    words = [np.ascontiguousarray(res[s]._samples).view(np.uint32) for s in range(len(res))]  # noqa: SLF001
    return res, np.arange(12) % 3, words


def _api_equal(a, want, what, n_groups, ram):
    """A summary of the Python API against _pooled_host: integers ==, min / max and the integer means as values with NaN in
    the same places, the means of the ram combinations (`ram`) within (count - 1) * 2^-53 relative of fsum / count."""
    for k in ("count", "above", "hist", "under", "over"):
        if k in want:
            got = a[k].cpu().numpy()
            assert got.dtype == np.int64 and np.array_equal(got[:n_groups], want[k]), (what, k)
    for k in ("min", "max"):
        assert np.array_equal(a[k].cpu().numpy()[:n_groups], want[k], equal_nan=True), (what, k)
    got, n = a["mean"].cpu().numpy()[:n_groups], want["count"][:, :, None].astype(np.float64)
    assert np.array_equal(got[:, :, ~ram], want["mean"][:, :, ~ram], equal_nan=True), what
    assert np.array_equal(np.isnan(got), np.isnan(want["mean"])), what
    err = np.nan_to_num(np.abs(got - want["mean"])[:, :, ram])
    bound = np.nan_to_num((n - 1.0) * 2.0 ** -53 * np.abs(want["mean"][:, :, ram]))
    print(f"{what}: largest ram-mean error / bound = {float(np.max(err / np.maximum(bound, 1e-300))):.3g}")
    assert (err <= bound).all(), what


def test_event_workload_through_the_python_api(event_run, tmp_path):
    res, ids, words = event_run
    names = res.series_names()
    ne = res.plan.n_edges
    period = res.plan.sample_period
    per10 = int(round(10.0 / period))
    edges = tick_window_edges(per10, res.plan.tick_count)
    thr = {"queued": 0.5, "fleet_ram": 100.0}
    from asyncflow_amd.results import check_series_combinations

    labels, ops, columns = check_series_combinations(COMBOS, names, ne)
    pairs = list(zip(ops, columns))
    thr_v = np.array([thr.get(k, 0.0) for k in labels])
    for by, gid, G in ((ids, ids, 3), ("scenario", np.arange(12), 12)):
        a = res.series_combined_summary(COMBOS, 10.0, by=by, thresholds=thr, bins=64)
        want, one = _pooled_host(words, gid, G, edges, ne, pairs, thr_v, 64, None, None)
        assert a["names"] == labels and a["ops"] == ops and np.array_equal(a["tick_edges"], edges) and a["replicas"].tolist() == [12 // G] * G
        assert all(np.array_equal(x, y) for x, y in zip(a["columns"], columns)) and np.array_equal(a["times"], edges[:-1] * period)
        assert np.array_equal(a["bin_edges"], one["bin_edges"]) and np.array_equal(a["ram"], one["ram"])
        assert a["series_combined_ms"] > 0 and a["scratch_bytes"] > 0 and tuple(a["hist"].shape) == (G, len(edges) - 1, len(labels), 64)
        _api_equal(a, want, f"by {G} groups", G, one["ram"])
        share = a["above_share"].cpu().numpy()
        assert np.array_equal(share, want["above"] / want["count"][:, :, None].astype(np.float64), equal_nan=True)
    assert want["above"][:, :, labels.index("fleet_ram")].sum() > 0 and want["max"][:, :, labels.index("open")].max() > 0
    # one scenario alone is the host definition of the scenario
    mine = res[5].get_series_combined(COMBOS, 10.0, thresholds=thr_v, bins=64)
    for k in ("count", "above", "hist", "under", "over"):
        assert np.array_equal(a[k].cpu().numpy()[5], mine[k]), k
    for k in ("min", "max"):
        assert np.array_equal(a[k].cpu().numpy()[5], mine[k], equal_nan=True), k
    # exact quantiles of the integer combinations off the histogram
    ints = {k: v for k, v in COMBOS.items() if not k.endswith("ram") and k != "ram_gap"}
    h = res.series_combined_summary(ints, 10.0, by=ids, bins=1024)
    assert int(h["over"].sum()) == 0 and not h["ram"].any()
    q = series_histogram_quantiles(h, (0.5, 0.95, 0.99))
    i_labels, i_ops, i_cols = check_series_combinations(ints, names, ne)
    for c, (op, col) in enumerate(zip(i_ops, i_cols)):
        for g in range(3):
            for w in range(len(edges) - 1):
                v = np.concatenate([series_combined_values(words[s], ne, op, col)[int(edges[w]):int(edges[w + 1])] for s in np.nonzero(ids == g)[0]]).astype(np.float64)
                assert q[g, w, c].tobytes() == np.quantile(v, (0.5, 0.95, 0.99)).tobytes(), (c, g, w)
    # bands over the replicas
    per = res.series_combined_summary(COMBOS, 10.0, by="scenario", thresholds=thr)
    pooled = res.series_combined_summary(COMBOS, 10.0, by=ids, thresholds=thr)
    for of in ("mean", "max", "min", "above_share"):
        bands = res.series_combined_bands(COMBOS, 10.0, by=ids, thresholds=thr, of=of, level=0.9, q=(0.1, 0.75))
        assert bands["mean"].shape == (3, len(edges) - 1, len(labels)) and (bands["n"] == 4).all() and bands["names"] == labels
        assert bands["pooled"].tobytes() == pooled[of].cpu().numpy().tobytes()
        mem = per[of].cpu().numpy()
        for g in range(3):
            np.testing.assert_allclose(bands["mean"][g], mem[ids == g].mean(axis=0), rtol=1e-12, atol=1e-15)
            np.testing.assert_allclose(bands["q_lo"][g], np.quantile(mem[ids == g], 0.1, axis=0), rtol=1e-12, atol=1e-15)
            np.testing.assert_allclose(bands["q_hi"][g], np.quantile(mem[ids == g], 0.75, axis=0), rtol=1e-12, atol=1e-15)
    # the saved file
    for ext in ("npz", "parquet"):
        if ext == "parquet":
            try:
                import pyarrow  # noqa: F401
            except ImportError:
                continue
        path = str(tmp_path / f"series_combined.{ext}")
        written = res.save_series_combined_summary(path, ids, combos=COMBOS, window_s=10.0, thresholds=thr, bins=64)
        back = load_summary(path)
        assert set(back) == set(written)
        for k, v in written.items():
            assert np.array_equal(np.asarray(back[k], dtype=v.dtype), v, equal_nan=True), k
        want, _ = _pooled_host(words, ids, 3, edges, ne, pairs, thr_v, 64, None, None)
        bands = res.series_combined_bands(COMBOS, 10.0, by=ids, thresholds=thr)
        assert back["replicas"].tolist() == [4, 4, 4] and np.array_equal(back["series_combined_count"], want["count"])
        for c, name in enumerate(labels):
            assert np.array_equal(back[f"series_combined_hist:{name}"], want["hist"][:, :, c]) and np.array_equal(back[f"series_combined_max:{name}"], want["max"][:, :, c])
            assert np.array_equal(back[f"series_combined_min:{name}"], want["min"][:, :, c]) and np.array_equal(back[f"series_combined_under:{name}"], want["under"][:, :, c])
            assert np.array_equal(back[f"series_combined_above:{name}"], want["above"][:, :, c] / want["count"].astype(np.float64))
            assert back[f"series_combined_q95:{name}"].tobytes() == np.ascontiguousarray(bands["q_hi"][:, :, c]).tobytes()
            assert back[f"series_combined_mean:{name}"].tobytes() == np.ascontiguousarray(pooled["mean"].cpu().numpy()[:, :, c]).tobytes()
        assert np.array_equal(back["series_combined_tick_edges"], edges) and np.array_equal(back["series_combined_times"], edges[:-1] * period)
