"""Sampled-series analyzer per (group, window of ticks) on the MI355X (af_engine_summarize_series_windows): synthetic sample
blocks handed straight to the entry -- padding words and the rows past a scenario's ticks filled with garbage -- against the
host definition bit for bit, on plans of 6, 12 and 42 series; arbitrary float32 RAM values against math.fsum; run-to-run and
batch independence; NULL outputs; the scratch bound; then event workloads through the Python API, bands, the on-disk summary
in both formats (tests of their own) and 14.4 M (cell, series) entries of singleton groups.  RAM values of either sign,
signed zeros and the -2^-45 residues (min / max of a ram_in_use column are the FLOAT minimum / maximum, -0.0 below +0.0);
the same blocks through af_engine_summarize; rows of 21, 26, 63, 64, 65, 66 and 81 16-byte groups; runs of several windows
per wave feeding the records; the fixture with negative residues through the Python API."""

from __future__ import annotations

import ctypes as C
import json
import math
from pathlib import Path

import numpy as np
import pytest

from asyncflow_amd import _abi
from asyncflow_amd.plan import lower
from asyncflow_amd.results import series_window_stats, tick_window_edges
from oracle.scenarios import deep_chain, lb_two_servers, lb_with_events, single_server, wide_fanout

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GARBAGE = 0xDEADBEEF


def ram_columns(n_series: int, n_edges: int) -> np.ndarray:
    """The ram_in_use columns (float32 words), stated here and not taken from the package: the edges come first, then
    ready_queue_len, event_loop_io_sleep, ram_in_use per server (include/asyncflow_hip.h)."""
    return np.array([j >= n_edges and (j - n_edges) % 3 == 2 for j in range(n_series)], dtype=bool)


def _plan(name: str):
    if name == "single_server":
        return lower(single_server(horizon=50))
    if name == "lb_two_servers":
        return lower(lb_two_servers(horizon=20))
    z = np.load(ROOT / "tests" / "golden" / "fanout8_t20.npz")          # the 8-server fan-out: 42 series
    return lower(json.loads(str(z["payload_json"])))


def _block(plan, rng, n: int, cap: int, ticks, dyadic: bool = True):
    """Sample blocks [n, cap, pitch] of words: integer columns uniform in [0, 2^20], ram columns random multiples of 1/256
    below 2^16 (or, dyadic=False, arbitrary non-negative float32 over many binades); padding words and the rows at and past
    a scenario's min(ticks, cap) hold garbage.  Returns the block and the counts."""
    S, pitch = plan.n_series, plan.series_pitch
    ram = ram_columns(S, plan.n_edges)
    blk = np.full((n, cap, pitch), GARBAGE, dtype=np.uint32)
    body = rng.integers(0, 2 ** 20 + 1, (n, cap, S)).astype(np.uint32)
    if dyadic:
        f = (rng.integers(0, 2 ** 24, (n, cap, int(ram.sum()))) / 256.0).astype(np.float32)
    else:
        f = (rng.lognormal(0.0, 6.0, (n, cap, int(ram.sum()))) * (rng.random((n, cap, int(ram.sum()))) > 0.1)).astype(np.float32)
    body[:, :, ram] = f.view(np.uint32)
    blk[:, :, :S] = body
    counts = np.zeros((n, _abi.CNT_SLOTS), dtype=np.uint32)
    counts[:, _abi.CNT_TICKS] = ticks
    for s in range(n):
        blk[s, min(int(counts[s, _abi.CNT_TICKS]), cap):] = rng.integers(0, 2 ** 32, dtype=np.uint32) | np.uint32(0x7F800000)
    return blk, counts


def _run(plan, blk, counts, group, n_groups, tick_edges, thresholds=None, outputs=("min", "max", "above")):
    """The block through af_engine_summarize_series_windows on a fresh engine.  Every output lies inside one buffer with a
    sentinel on each side; returns the outputs as numpy, the scratch size and whether all sentinels stayed."""
    import torch

    from asyncflow_amd.engine import Engine

    n, cap, _ = blk.shape
    S, W = plan.n_series, len(tick_edges) - 1
    dev = torch.device("cuda", 0)
    blk_t = torch.as_tensor(blk.view(np.int32), device=dev)
    counts_t = torch.as_tensor(counts.view(np.int32), device=dev)
    grp_t = None
    if group is not None:
        g = np.asarray(group, dtype=np.int64)
        grp_t = torch.as_tensor(np.where(g < 0, _abi.POOL_SKIP, g).astype(np.uint32).view(np.int32), device=dev)
    cells = n_groups * W
    guard = 64                                                       # int32 words of sentinel between the outputs
    sizes = {"count": cells, "mean": 2 * cells * S, "min": cells * S, "max": cells * S, "above": cells * S}
    off, at = {}, guard
    for k, sz in sizes.items():
        off[k] = at
        at += sz + guard + (sz + guard) % 2                           # (keeps every output 8-byte aligned)
    buf = torch.full((at,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    ptr = {k: buf.data_ptr() + 4 * o for k, o in off.items()}
    eng = Engine(plan, 0)
    try:
        _, scratch = eng.summarize_series_windows(
            n, n_groups, tick_edges, samples_ptr=blk_t.data_ptr(), tick_capacity=cap, counts_ptr=counts_t.data_ptr(),
            count_ptr=ptr["count"], mean_ptr=ptr["mean"], min_ptr=ptr["min"] if "min" in outputs else 0,
            max_ptr=ptr["max"] if "max" in outputs else 0, above_ptr=ptr["above"] if "above" in outputs else 0,
            group_ptr=grp_t.data_ptr() if grp_t is not None else 0, thresholds=thresholds)
    finally:
        eng.close()
    host = buf.cpu().numpy()
    written = np.zeros(at, dtype=bool)
    out = {}
    for k, sz in sizes.items():
        if k in ("count", "mean") or k in outputs:
            written[off[k]:off[k] + sz] = True
            out[k] = host[off[k]:off[k] + sz].view(np.uint32)
    out["count"] = out["count"].reshape(n_groups, W)
    out["mean"] = out["mean"].view(np.float64).reshape(n_groups, W, S)
    for k in outputs:
        out[k] = out[k].reshape(n_groups, W, S)
    return out, scratch, bool((host[~written] == 0x5A5A5A5A).all())


def _reduceat(fn, arr, r):
    """fn over the columns [r[w], r[w + 1]) of arr [S, len] for every w (an empty range: anything)."""
    padded = np.concatenate([arr, np.zeros((arr.shape[0], 1), dtype=arr.dtype)], axis=1)
    return fn.reduceat(padded, r, axis=1)[:, :-1]


def _want(plan, blk, counts, group, n_groups, tick_edges, thresholds=None, fsum: bool = False):
    """The definition on the host, independent of results.series_window_stats: per scenario exact window sums (integers; the
    dyadic float values add exactly in float64 in any order), minima / maxima and counts above the threshold by
    ufunc.reduceat, then the members of a group combined.  Minima and maxima: the words of an integer column as they are;
    a ram word as an integer that orders like its float value, straight from sign and magnitude -- a negative float
    -(magnitude bits) - 1, so that -0.0 is -1, below +0.0 --, reduced and mapped back to the word.  fsum=True: the float means
    by math.fsum over the cell, and "abs_mean", math.fsum of the absolute values / count."""
    n, cap, _ = blk.shape
    S = plan.n_series
    ram = ram_columns(S, plan.n_edges)
    b = np.asarray(tick_edges, dtype=np.int64)
    W = len(b) - 1
    thr = np.zeros(S) if thresholds is None else np.asarray(thresholds, dtype=np.float64)
    group = np.zeros(n, dtype=np.int64) if group is None else np.asarray(group)
    count = np.zeros((n_groups, W), dtype=np.int64)
    isum = np.zeros((n_groups, W, S), dtype=np.int64)
    fsm = np.zeros((n_groups, W, S))
    terms = [[[] for _ in range(W)] for _ in range(n_groups)]
    mn = np.full((n_groups, W, S), 2 ** 40, dtype=np.int64)
    mx = np.full((n_groups, W, S), -2 ** 40, dtype=np.int64)
    above = np.zeros((n_groups, W, S), dtype=np.int64)
    for s in range(n):
        g = int(group[s])
        if g < 0:
            continue
        m = min(int(counts[s, _abi.CNT_TICKS]), cap)
        words = np.ascontiguousarray(blk[s, :m, :S].T)                # [S, m]
        r = np.minimum(b, m)
        c = np.diff(r)
        live = c > 0
        values = words.astype(np.float64)
        values[ram] = words[ram].view(np.float32).astype(np.float64)
        count[g] += c
        isum[g] += np.where(live, _reduceat(np.add, words.astype(np.int64), r), 0).T
        fsm[g] += np.where(live, _reduceat(np.add, values, r), 0.0).T
        above[g] += np.where(live, _reduceat(np.add, (values > thr[:, None]).astype(np.int64), r), 0).T
        order = words.astype(np.int64)
        negative = ram[:, None] & (words >> 31 != 0)
        order[negative] = -(words[negative] & np.uint32(0x7FFFFFFF)).astype(np.int64) - 1
        mn[g] = np.minimum(mn[g], np.where(live, _reduceat(np.minimum, order, r), 2 ** 40).T)
        mx[g] = np.maximum(mx[g], np.where(live, _reduceat(np.maximum, order, r), -2 ** 40).T)
        if fsum:
            for w in np.nonzero(live)[0]:
                terms[g][w].append(values[:, r[w]:r[w + 1]])
    empty = count == 0
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(ram, fsm, isum.astype(np.float64)) / count[:, :, None].astype(np.float64)
    mean[empty] = np.nan
    mn[empty] = mx[empty] = 0
    assert (mn[~empty] < 2 ** 32).all() and (mx[~empty] >= -2 ** 31).all() and (mn[:, :, ~ram] >= 0).all()
    mn, mx = (np.where(v < 0, (-v - 1) | 0x80000000, v).astype(np.uint32) for v in (mn, mx))
    out = {"count": count, "mean": mean, "min": mn, "max": mx, "above": above.astype(np.uint32)}
    if fsum:
        out["abs_mean"] = np.abs(mean)
        for g in range(n_groups):
            for w in range(W):
                if count[g, w]:
                    cell = np.concatenate(terms[g][w], axis=1)
                    mean[g, w, ram] = [math.fsum(row.tolist()) / cell.shape[1] for row in cell[ram]]
                    out["abs_mean"][g, w, ram] = [math.fsum(np.abs(row).tolist()) / cell.shape[1] for row in cell[ram]]
    return out


def _same(got, want, what, ram=None, float_tol: bool = False, zero_sums: list | None = None):
    """zero_sums (signed data): a cell whose exact sum is zero compares as a value -- the sign of a zero sum is not part of
    the definition --; their number and that of the non-empty entries of the ram columns are added to the list."""
    assert np.array_equal(got["count"], want["count"].astype(np.uint32)), what
    for k in ("min", "max", "above"):
        if k in got:
            assert np.array_equal(got[k], want[k]), (what, k, np.argwhere(got[k] != want[k])[:5])
    if not float_tol:
        differ = got["mean"].view(np.uint64) != want["mean"].view(np.uint64)
        if zero_sums is not None:
            zero = want["mean"] == 0.0
            assert (got["mean"][zero] == 0.0).all(), what
            differ &= ~zero
            zero_sums.append((int(zero[:, :, ram].sum()), int((want["count"] > 0).sum()) * int(ram.sum())))
        bad = [t for t in np.argwhere(differ) if not (np.isnan(got["mean"][tuple(t)]) and np.isnan(want["mean"][tuple(t)]))]
        assert not bad, (what, bad[:5])
        return
    exact = ~ram
    assert np.array_equal(got["mean"][:, :, exact], want["mean"][:, :, exact], equal_nan=True), what
    n = want["count"][:, :, None].astype(np.float64)
    err = np.abs(got["mean"][:, :, ram] - want["mean"][:, :, ram])
    scale = want["abs_mean"][:, :, ram]                                # (fsum |x| / n: signed terms cancel in the mean)
    print(f"{what}: largest float-mean error / (n * 2^-52 * fsum|x| / n) = "
          f"{np.nanmax(err / np.maximum(n * 2.0 ** -52 * scale, 1e-300)):.3g}, largest cell {int(n.max())}")
    assert n.max() <= 4096
    assert ((err <= n * 2.0 ** -52 * scale) | (want["count"] == 0)[:, :, None]).all(), what
    assert np.isnan(got["mean"][want["count"] == 0]).all()


def _ticks(rng, n: int, cap: int) -> np.ndarray:
    t = rng.integers(1, cap + 1, n)
    t[0], t[1], t[2], t[3] = 0, cap, cap + 50, 1                       # no tick at all, all of them, more than were stored
    return t


def _thresholds(plan, blk) -> np.ndarray:
    """Per series: 0.0, a value that occurs in the data (strictly greater decides), 0.5 on an integer column, a value on a
    ram column."""
    S = plan.n_series
    ram = ram_columns(S, plan.n_edges)
    thr = np.zeros(S)
    for j in range(1, S):
        w = blk[1, 0, j]                                               # (scenario 1 stored every tick)
        thr[j] = float(np.uint32(w).view(np.float32)) if ram[j] else float(w)
    thr[1] = 0.5
    assert not ram[0] and not ram[1] and ram.any() and (thr[ram] > 0).all()
    return thr


def _groupings(n: int):
    """One group (NULL and explicit), interleaved ids with an empty group and scenarios left out, singletons, singletons
    among groups without a member."""
    interleaved = np.array([(i * 7) % 6 for i in range(n)])
    interleaved[interleaved == 3] = 4                                  # group 3 is empty
    interleaved[[i for i in (2, 9, 20) if i < n]] = -1                 # and three scenarios (of 23) are left out
    sparse = np.arange(n) * 2                                          # singletons, every other group without a member
    sparse[5] = -1
    return [(None, 1, "one group (NULL)"), (np.zeros(n, dtype=np.int64), 1, "one group"), (interleaved, 6, "interleaved"),
            (np.arange(n), n, "singletons"), (sparse, 2 * n, "singletons and empty groups")]


def _shapes(cap: int):
    return [("one window", np.array([0, cap])), ("one tick each", np.arange(cap + 1)), ("20 ticks", tick_window_edges(20, cap)),
            ("64 ticks", tick_window_edges(64, cap)), ("65 ticks", tick_window_edges(65, cap)),
            ("200 ticks", tick_window_edges(200, cap)),
            ("uneven", np.array([3, 4, 10, 75, 76, 300, 650, cap - 1, cap, cap + 9, cap + 10, 5 * cap]))]


@pytest.mark.parametrize("name", ["single_server", "lb_two_servers", "fanout8"])
def test_synthetic_blocks_equal_the_host_definition(name):
    plan = _plan(name)
    assert (plan.n_series, plan.series_pitch) == {"single_server": (6, 8), "lb_two_servers": (12, 12), "fanout8": (42, 44)}[name]
    rng = np.random.default_rng(len(name))
    n, cap = 23, 700
    blk, counts = _block(plan, rng, n, cap, _ticks(rng, n, cap))
    assert (blk[1, :, plan.n_series:] == GARBAGE).all()                 # (scenario 1 stored every tick: its padding words)
    groupings, shapes = _groupings(n), _shapes(cap)
    thr = _thresholds(plan, blk)
    for what, edges in shapes:
        for group, n_groups, gname in groupings:
            if what == "one tick each" and gname not in ("interleaved", "singletons"):
                continue
            for t in (None, thr):
                got, _, intact = _run(plan, blk, counts, group, n_groups, edges, t)
                want = _want(plan, blk, counts, group, n_groups, edges, t)
                _same(got, want, f"{name}, {what}, {gname}, thresholds {'set' if t is not None else 'none'}")
                assert intact
    # singletons are the host definition of the package itself, scenario by scenario
    edges = shapes[-1][1]
    got, _, _ = _run(plan, blk, counts, np.arange(n), n, edges, thr)
    assert (got["count"][:, -2:] == 0).all() and np.isnan(got["mean"][:, -2:]).all() and (got["count"][0] == 0).all()
    for s in range(n):
        m = min(int(counts[s, _abi.CNT_TICKS]), cap)
        host = series_window_stats(np.ascontiguousarray(blk[s, :m, :plan.n_series].T), edges, plan.n_edges, thr)
        _same({k: v[s:s + 1] for k, v in got.items()}, {k: v[None] for k, v in host.items()}, f"{name}, scenario {s}")


# ------------------------------------------------------------------------------------ RAM values of either sign
RESIDUE = np.float32(-(2.0 ** -45))        # what the reference's float arithmetic leaves in ram_in_use (-2.8e-14)
NEG_ZERO = np.uint32(0x80000000)


def _signed_block(plan, rng, n: int, cap: int, ticks, flip: int = 0, dyadic: bool = True):
    """_block with ram values of either sign.  The ram columns alternate between two kinds (`flip` swaps them), both chosen so
    that every float64 sum over a cell of fewer than 2^14 values is EXACT in any order:
      wide     multiples of 1/256 in (-2^16, 2^16): a sum stays below 2^30 with its last bit at 2^-8;
      residue  multiples of 2^-30 in (-2^-6, 2^-6) with one sample in 16 replaced by -2^-45: a sum stays below 2^8 with its
               last bit at 2^-45, 53 bits.  (A residue among values of the wide kind would need 61.)
    Both: one sample in 2 000 is +0.0 and one is -0.0.  Where the scenarios stored the rows, in every ram column:
      rows 100-119 of every scenario, and rows 20-39 of scenario 1: negative values only;
      rows 120-139 of every scenario, and rows 60-79 of scenario 1: negative values after one -0.0, the largest value;
      rows 140-141 of every scenario, and rows 40-59 of scenario 1: +0.0 and -0.0 only, at least one of each.
    Blocks of fewer than 700 rows -- where a window of one tick makes every lone zero a cell whose sum is zero, and fewer than
    1 % of the cells should be such -- hold FOUR zeros per ram column, all in scenario 1: none is sprinkled, rows 140-141 are
    zeros in scenario 1 alone, rows 40-59 are ordinary values, and of rows 120-139 only scenario 1 starts with -0.0 (the others
    are negative throughout: -0.0 is still the largest value of the window in every group that holds scenario 1).
    dyadic=False: arbitrary float32 over many binades with random signs, no special rows."""
    blk, counts = _block(plan, rng, n, cap, ticks, dyadic=dyadic)
    S = plan.n_series
    ram = np.nonzero(ram_columns(S, plan.n_edges))[0]
    shape = (n, cap)
    for i, j in enumerate(ram):
        if not dyadic:
            v = (blk[:, :, j] | (rng.integers(0, 2, shape).astype(np.uint32) << 31)).view(np.float32)     # (a random sign bit)
        else:
            if (i + flip) % 2 == 0:
                v = (rng.integers(-2 ** 24 + 1, 2 ** 24, shape) / 256.0).astype(np.float32)
                filler = np.float32(-1.0 / 256.0)
            else:
                v = (rng.integers(-2 ** 24 + 1, 2 ** 24, shape) * 2.0 ** -30).astype(np.float32)
                v[rng.random(shape) < 1 / 16] = RESIDUE
                filler = RESIDUE
            small = cap < 700
            u = rng.random(shape)
            if small:
                v[v == 0] = filler
            else:
                v[u < 0.0005] = np.float32(0.0)
                v[u > 0.9995] = np.float32(-0.0)

            def zone(rows, scen, kind):
                part = v[scen, rows]
                if kind == "negative":
                    part[...] = -np.abs(part)
                    part[part == 0] = filler
                elif kind == "negative and -0.0":
                    part[...] = -np.abs(part)
                    part[part == 0] = filler
                    part[..., 0] = np.float32(-0.0)
                else:
                    part[...] = np.where(rng.random(part.shape) < 0.5, np.float32(0.0), np.float32(-0.0))
                    part[..., 0], part[..., 1] = np.float32(0.0), np.float32(-0.0)
                v[scen, rows] = part

            assert cap >= 142
            zone(slice(100, 120), slice(None), "negative")
            zone(slice(120, 140), slice(None), "negative" if small else "negative and -0.0")
            zone(slice(140, 142), 1 if small else slice(None), "zeros")
            zone(slice(20, 40), 1, "negative")
            zone(slice(60, 80), 1, "negative and -0.0")
            if small:
                v[1, 120] = np.float32(-0.0)
            else:
                zone(slice(40, 60), 1, "zeros")
        live = np.arange(cap)[None, :] < np.minimum(counts[:, _abi.CNT_TICKS], cap)[:, None]
        blk[:, :, j] = np.where(live, v.view(np.uint32), blk[:, :, j])     # (the rows past a scenario's ticks keep their garbage)
    return blk, counts


def _signed_thresholds(plan, blk, second: bool) -> np.ndarray:
    """_thresholds for signed blocks: integer columns as there (0.0, a value that occurs, 0.5).  The ram columns, in turn:
    -0.0 (+0.0 is not above it: the values compare as f64), a NEGATIVE value that occurs in the data, a value of either sign
    that occurs; `second` starts the turn at the negative value (a plan with one ram column sees both)."""
    S = plan.n_series
    ram = ram_columns(S, plan.n_edges)
    thr = np.zeros(S)
    for j in range(1, S):
        thr[j] = float(blk[1, 0, j])
    thr[1] = 0.5
    for i, j in enumerate(np.nonzero(ram)[0]):
        col = blk[1, :, j].view(np.float32).astype(np.float64)              # (scenario 1 stored every tick)
        turn = (i + (1 if second else 0)) % 3
        thr[j] = -0.0 if turn == 0 else float(col[col < 0][7]) if turn == 1 else float(col[5])
    assert not ram[0] and not ram[1]
    assert (np.signbit(thr[ram]) & (thr[ram] == 0)).any() or second
    assert (thr[ram] < 0).any() or not second
    return thr


def _zero_sum_share(zero_sums) -> float:
    zero, entries = (sum(t[i] for t in zero_sums) for i in (0, 1))
    return zero / entries


@pytest.mark.parametrize(("name", "flip"), [("single_server", 0), ("single_server", 1), ("lb_two_servers", 0), ("fanout8", 0)])
def test_signed_ram_values_equal_the_host_definition(name, flip):
    """The shapes and groupings of test_synthetic_blocks_equal_the_host_definition on _signed_block: count, min, max and
    above exact, the mean bit-equal (a cell whose exact sum is zero: as a value; fewer than 1 % of the entries)."""
    plan = _plan(name)
    ram = ram_columns(plan.n_series, plan.n_edges)
    rng = np.random.default_rng(1000 + len(name) + flip)
    n, cap = 23, 700
    blk, counts = _signed_block(plan, rng, n, cap, _ticks(rng, n, cap), flip)
    assert n * cap < 2 ** 14                                             # (_signed_block: every sum is exact)
    first = int(np.nonzero(ram)[0][0])
    thr_a, thr_b = _signed_thresholds(plan, blk, False), _signed_thresholds(plan, blk, True)
    assert thr_a[first] == 0 and np.signbit(thr_a[first]) and thr_b[first] < 0
    assert (blk[:, :, first] == 0).any() and (blk[:, :, first] == NEG_ZERO).any()
    zero_sums: list = []
    for what, edges in _shapes(cap):
        for group, n_groups, gname in _groupings(n):
            if what == "one tick each" and gname not in ("interleaved", "singletons"):
                continue
            for t, tname in ((None, "none"), (thr_a, "-0.0 first"), (thr_b, "negative first")):
                if tname == "negative first" and what not in ("20 ticks", "uneven"):
                    continue
                got, _, intact = _run(plan, blk, counts, group, n_groups, edges, t)
                want = _want(plan, blk, counts, group, n_groups, edges, t)
                _same(got, want, f"{name}, {what}, {gname}, thresholds {tname}", ram, zero_sums=zero_sums)
                assert intact
                if what == "20 ticks" and gname in ("one group", "singletons") and t is None:
                    # the rows _signed_block made: windows 5 / 6 of every scenario, windows 1 / 3 / 2 of scenario 1
                    g = 0 if gname == "one group" else 1                  # (scenario 1 stored every tick)
                    mx, mn = want["max"][:, :, ram], want["min"][:, :, ram]
                    assert (mx[g, 5] > NEG_ZERO).all() and (mx[g, 6] == NEG_ZERO).all() and (mn[g, 6] > NEG_ZERO).all()
                    if gname == "singletons":
                        assert (mx[1, 1] > NEG_ZERO).all() and (mx[1, 3] == NEG_ZERO).all() and (mn[1, 3] > NEG_ZERO).all()
                        assert (mx[1, 2] == 0).all() and (mn[1, 2] == NEG_ZERO).all() and (want["mean"][1, 2][ram] == 0).all()
                        assert want["count"][3, 0] == 1 and want["count"][3, 1] == 0          # (scenario 3 stored one tick)
                if t is thr_a and what == "one window" and gname == "one group":
                    # +0.0 is not above -0.0: the count above -0.0 is the count of the positive values
                    values = np.concatenate([blk[s, :min(int(counts[s, _abi.CNT_TICKS]), cap), first] for s in range(n)]).view(np.float32)
                    assert (values == 0).sum() > 2 and want["above"][0, 0, first] == (values > 0).sum()
    share = _zero_sum_share(zero_sums)
    print(f"{name}, flip {flip}: cells whose exact sum is zero: {100 * share:.3f} % of the non-empty entries of the ram columns")
    assert 0 < share < 0.01


def test_signed_arbitrary_float_values_against_fsum():
    plan = _plan("lb_two_servers")
    ram = ram_columns(plan.n_series, plan.n_edges)
    rng = np.random.default_rng(6)
    n, cap = 8, 512
    blk, counts = _signed_block(plan, rng, n, cap, _ticks(rng, n, cap), dyadic=False)
    assert (blk[1, :, :plan.n_series][:, ram] >> 31).mean() > 0.3
    edges = tick_window_edges(200, cap)
    for group, n_groups in ((None, 1), (np.arange(n) % 3, 3), (np.arange(n), n)):
        got, _, intact = _run(plan, blk, counts, group, n_groups, edges)
        assert intact
        _same(got, _want(plan, blk, counts, group, n_groups, edges, fsum=True), f"signed arbitrary floats, {n_groups} groups", ram, float_tol=True)


# ------------------------------------------------------------------------------------ the two series kernels agree
def _agrees_with_the_whole_run_kernel(plan, blk, counts, what):
    """One window [0, cap], every scenario a group of its own: max words and mean bytes of af_engine_summarize's series_max /
    series_mean (af_series_kernel) on the same buffers."""
    from tests.test_gpu_analyzer_synthetic import _series

    n, cap, _ = blk.shape
    got, _, intact = _run(plan, blk, counts, np.arange(n), n, np.array([0, cap]))
    assert intact
    whole = _series(plan, blk, counts)
    some = np.minimum(counts[:, _abi.CNT_TICKS], cap) > 0
    assert some.sum() >= n - 1 and not some.all()
    assert np.array_equal(got["max"][:, 0], whole["series_max"]), (what, np.argwhere(got["max"][:, 0] != whole["series_max"])[:5])
    assert got["mean"][some, 0].tobytes() == whole["series_mean"][some].tobytes(), what
    assert np.isnan(got["mean"][~some]).all() and np.isnan(whole["series_mean"][~some]).all()


@pytest.mark.parametrize(("name", "flip"), [("single_server", 0), ("single_server", 1), ("lb_two_servers", 0), ("fanout8", 0)])
def test_one_window_of_signed_values_is_the_whole_run_summary(name, flip):
    plan = _plan(name)
    rng = np.random.default_rng(1000 + len(name) + flip)
    n, cap = 23, 700
    blk, counts = _signed_block(plan, rng, n, cap, _ticks(rng, n, cap), flip)
    _agrees_with_the_whole_run_kernel(plan, blk, counts, f"{name}, flip {flip}")


# ------------------------------------------------------------------------------------ wide rows
WIDE = {"wide_fanout16": (82, 84),     # 21 16-byte groups a row: three rows a step, lane 63 idle, a tree over 3 of 4
        "wide_fanout20": (102, 104),   # 26 groups: two rows a step
        "wide_fanout50": (252, 252),   # 63 groups: one row a step, lane 63 idle
        "deep_chain62": (256, 256),    # 64 groups: every lane, one pass
        "wide_fanout51": (257, 260),   # 65 groups: a second pass over the rows for one group that holds one series
        "wide_fanout52": (262, 264),   # 66 groups
        "wide_fanout64": (322, 324)}   # 81 groups


def _wide_plan(name: str):
    return lower(deep_chain(62) if name == "deep_chain62" else wide_fanout(int(name[len("wide_fanout"):])))


def _wide_shapes(cap: int):
    return [("one window", np.array([0, cap])), ("one tick each", np.arange(cap + 1)), ("7 ticks", tick_window_edges(7, cap)),
            ("64 ticks", tick_window_edges(64, cap)), ("65 ticks", tick_window_edges(65, cap)),
            ("uneven", np.array([3, 4, 10, 75, 76, 120, cap - 1, cap, cap + 9, cap + 10, 5 * cap]))]


@pytest.mark.parametrize("name", list(WIDE))
def test_wide_rows_equal_the_host_definition(name):
    plan = _wide_plan(name)
    assert (plan.n_series, plan.series_pitch) == WIDE[name]
    ram = ram_columns(plan.n_series, plan.n_edges)
    rng = np.random.default_rng(2000 + plan.n_series)
    n, cap = 7, 150
    blk, counts = _signed_block(plan, rng, n, cap, _ticks(rng, n, cap))
    assert blk.nbytes <= 1_400_000 and (blk[1, :, plan.n_series:] == GARBAGE).all()
    thr = _signed_thresholds(plan, blk, False)
    zero_sums: list = []
    for what, edges in _wide_shapes(cap):
        for group, n_groups, gname in _groupings(n):
            for t in (None, thr):
                got, _, intact = _run(plan, blk, counts, group, n_groups, edges, t)
                want = _want(plan, blk, counts, group, n_groups, edges, t)
                _same(got, want, f"{name}, {what}, {gname}, thresholds {'set' if t is not None else 'none'}", ram, zero_sums=zero_sums)
                assert intact
    assert (blk[1, :, :plan.n_series][:, ram] << 1 == 0).sum(axis=0).tolist() == [4] * int(ram.sum())     # (rows 60, 120, 140, 141)
    share = _zero_sum_share(zero_sums)
    print(f"{name}: cells whose exact sum is zero: {100 * share:.3f} % of the non-empty entries of the ram columns")
    assert 0 < share < 0.01
    _agrees_with_the_whole_run_kernel(plan, blk, counts, name)


# ------------------------------------------------------------------------------------ runs of windows into the records
@pytest.mark.parametrize("flip", [0, 1])                               # (the plan's one ram column: of either kind of _signed_block)
@pytest.mark.parametrize(("n", "cap", "run", "last"), [(64, 1501, 2, 1), (300, 700, 6, 4)])
def test_runs_of_several_windows_feed_the_records(n, cap, run, last, flip):
    """One tick per window.  The engine gives a wave max(1, W / ceil(32768 / n)) consecutive windows (engine.hip,
    af_engine_summarize_series_windows: "runs as long as leave the chip some 32 768 waves"); the cases are chosen for THAT
    rule -- runs of 2 windows with a last run of 1, runs of 6 with a last run of 4 -- and cover less if it changes."""
    plan = _plan("single_server")
    ram = ram_columns(plan.n_series, plan.n_edges)
    W = cap
    assert max(1, W // -(-32768 // n)) == run and W % run == last
    rng = np.random.default_rng(n + flip)
    blk, counts = _signed_block(plan, rng, n, cap, _ticks(rng, n, cap), flip)
    assert ((blk[1, :, :plan.n_series][:, ram] == RESIDUE.view(np.uint32)).sum() > 20) == (flip == 1)
    edges = np.arange(cap + 1)
    interleaved = np.arange(n) * 7 % 6
    interleaved[interleaved == 3] = 4                                  # five groups with members, group 3 is empty
    interleaved[[2, 9, 20]] = -1                                       # three scenarios are left out
    zero_sums: list = []
    for group, n_groups, gname in ((interleaved, 6, "interleaved"), (None, 1, "one group (NULL)"), (np.arange(n), n, "singletons")):
        got, scratch, intact = _run(plan, blk, counts, group, n_groups, edges)
        assert intact
        assert (scratch >= 20 * n * W * plan.n_series) == (gname != "singletons")     # (the records, or the direct path)
        _same(got, _want(plan, blk, counts, group, n_groups, edges), f"n = {n}, {W} windows, {gname}", ram, zero_sums=zero_sums)
    assert _zero_sum_share(zero_sums) < 0.01


# ------------------------------------------------------------------------------------ the fixture through the Python API
def test_fixture_with_negative_residues_through_the_python_api():
    """tests/golden/frac_ram_waiting_put_t20.npz: 179 of the 399 samples of series 8 are -2.84e-14.  Windows of 40 ticks: the
    largest value of series 8 is 200.6 or 300.9 MB in every window, the smallest the residue."""
    from asyncflow_amd.runner import SimulationRunner

    fx = np.load(ROOT / "tests" / "golden" / "frac_ram_waiting_put_t20.npz", allow_pickle=False)
    payload, seed = json.loads(str(fx["payload_json"])), int(fx["seed"])
    words = fx["samples"].view(np.uint32)
    res = SimulationRunner(simulation_input=payload, seeds=[seed, seed + 1]).run()
    assert np.array_equal(res[0]._samples, words)  # noqa: SLF001
    ram = ram_columns(res.plan.n_series, res.plan.n_edges)
    a = res.series_window_summary(ticks_per_window=40, by="scenario")
    mx, mn = a["max"].cpu().numpy(), a["min"].cpu().numpy()
    assert mx.shape == (2, 10, 12) and ram[8]
    for s in range(2):
        samples = res[s]._samples  # noqa: SLF001
        values = samples.astype(np.float64)
        values[ram] = samples[ram].view(np.float32).astype(np.float64)
        for w in range(10):
            seg = values[:, 40 * w:40 * (w + 1)]
            assert np.array_equal(mx[s, w], seg.max(axis=1)) and np.array_equal(mn[s, w], seg.min(axis=1)), (s, w)
    residue = float(np.float32(-2.842171e-14))
    assert (mn[0, :, 8] == residue).all() and -2.9e-14 < residue < -2.8e-14
    assert [round(float(v), 1) for v in mx[0, :, 8]] == [200.6, 300.9, 300.9, 200.6, 200.6, 200.6, 300.9, 200.6, 200.6, 200.6]
    # one window over the whole run is the per-scenario series summary
    whole = res.series_window_summary(tick_edges=[0, res.plan.tick_count], by="scenario")
    summ = res.summary(rps=False, series=True)
    assert np.array_equal(whole["max_words"][:, 0].cpu().numpy(), summ["series_max"].cpu().numpy())
    assert whole["max"][0, 0, 8] > 300.0
    # the band over the two seeds is the band of their float maxima
    bands = res.series_window_bands(ticks_per_window=40, of="max")
    assert (bands["n"] == 2).all()
    np.testing.assert_allclose(bands["mean"][0], mx.mean(axis=0), rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(bands["std"][0], mx.std(axis=0, ddof=1), rtol=1e-12, atol=1e-300)
    assert (bands["mean"][0, :, 8] > 200.0).all()


def test_long_windows_and_long_runs():
    plan = _plan("lb_two_servers")
    rng = np.random.default_rng(41)
    n, cap = 6, 9000
    ticks = np.array([9000, 8191, 4097, 12000, 0, 4096])
    blk, counts = _block(plan, rng, n, cap, ticks)
    for edges in (tick_window_edges(4096, cap), np.array([0, cap]), np.array([5, 4101, 8197, 8198])):
        for group, n_groups in ((None, 1), (np.arange(n), n), (np.array([1, 0, 1, -1, 0, 1]), 3)):
            got, _, intact = _run(plan, blk, counts, group, n_groups, edges)
            _same(got, _want(plan, blk, counts, group, n_groups, edges), f"edges {edges.tolist()}, groups {n_groups}")
            assert intact


def test_arbitrary_float_values_run_to_run_and_batch_independence():
    plan = _plan("lb_two_servers")
    ram = ram_columns(plan.n_series, plan.n_edges)
    rng = np.random.default_rng(5)
    n, cap = 8, 512
    blk, counts = _block(plan, rng, n, cap, _ticks(rng, n, cap), dyadic=False)
    edges = tick_window_edges(200, cap)
    for group, n_groups in ((None, 1), (np.arange(n) % 3, 3), (np.arange(n), n)):
        got, _, _ = _run(plan, blk, counts, group, n_groups, edges)
        again, _, _ = _run(plan, blk, counts, group, n_groups, edges)
        for k in got:
            assert got[k].tobytes() == again[k].tobytes(), k              # the same call twice: identical bytes
        _same(got, _want(plan, blk, counts, group, n_groups, edges, fsum=True), f"arbitrary floats, {n_groups} groups", ram, float_tol=True)
    # the same scenarios inside a batch ten times as large: identical bytes for their cells
    for edges in (tick_window_edges(200, cap), tick_window_edges(7, cap), np.array([0, cap])):
        alone, _, _ = _run(plan, blk, counts, np.arange(n), n, edges)
        big, big_counts = _block(plan, rng, 10 * n, cap, rng.integers(0, cap + 1, 10 * n), dyadic=False)
        where = np.arange(n) * 10 + 3
        big[where], big_counts[where] = blk, counts
        inside, _, _ = _run(plan, big, big_counts, np.arange(10 * n), 10 * n, edges)
        for k in alone:
            assert alone[k].tobytes() == np.ascontiguousarray(inside[k][where]).tobytes(), k


def test_null_outputs_are_skipped():
    plan = _plan("single_server")
    rng = np.random.default_rng(2)
    n, cap = 9, 300
    blk, counts = _block(plan, rng, n, cap, _ticks(rng, n, cap))
    edges = tick_window_edges(64, cap)
    for group, n_groups in ((np.arange(n) % 2, 2), (np.arange(n), n)):
        full, _, intact = _run(plan, blk, counts, group, n_groups, edges)
        assert intact
        for outputs in ((), ("max",), ("min", "above")):
            got, _, intact = _run(plan, blk, counts, group, n_groups, edges, outputs=outputs)
            assert intact, f"a NULL output was written to (outputs {outputs})"
            assert set(got) == {"count", "mean", *outputs}
            for k in got:
                assert got[k].tobytes() == full[k].tobytes(), k


def _scratch_bound(n, n_groups, n_win, n_series, records: bool) -> int:
    """include/asyncflow_hip.h: 4 B per edge + 8 B per series + 4 B per group + 4 B per scenario + 2 KB of alignment, and
    -- unless every group holds at most one scenario -- 20 B per (scenario, window, series)."""
    return 4 * (n_win + 1) + 8 * n_series + 4 * (n_groups + 1) + 4 * n + 2048 + (20 * n * n_win * n_series if records else 0)


def test_scratch_stays_within_the_bound_of_the_header():
    plan = _plan("fanout8")
    rng = np.random.default_rng(3)
    n, cap = 40, 400
    blk, counts = _block(plan, rng, n, cap, rng.integers(0, cap + 1, n))
    edges = tick_window_edges(20, cap)
    W, S = len(edges) - 1, plan.n_series
    _, scratch, _ = _run(plan, blk, counts, np.arange(n) % 7, 7, edges)
    print(f"groups of several: scratch_bytes {scratch}, bound {_scratch_bound(n, 7, W, S, True)}")
    assert 20 * n * W * S <= scratch <= _scratch_bound(n, 7, W, S, True)
    _, scratch, _ = _run(plan, blk, counts, np.arange(n) * 3, 3 * n, edges)
    print(f"singletons: scratch_bytes {scratch}, bound {_scratch_bound(n, 3 * n, W, S, False)}")
    assert 0 < scratch <= _scratch_bound(n, 3 * n, W, S, False) < 20 * n * W * S


def test_device_argument_checks():
    """Error codes from calls that return before any kernel is launched."""
    import torch

    from asyncflow_amd.engine import Engine, EngineError, load_library

    plan = _plan("lb_two_servers")
    rng = np.random.default_rng(1)
    blk, counts = _block(plan, rng, 3, 50, [50, 20, 0])
    with pytest.raises(EngineError, match="group id out of range"):
        _run(plan, blk, counts, [0, 2, 0], 2, [0, 50])
    lib = load_library()
    dev = torch.device("cuda", 0)
    blk_t = torch.as_tensor(blk.view(np.int32), device=dev)
    counts_t = torch.as_tensor(counts.view(np.int32), device=dev)
    outs = torch.zeros(4096, dtype=torch.int32, device=dev)
    eng = Engine(plan, 0)
    try:
        def call(edges, thr=None, samples=True, n_groups=1, n_windows=None):
            e = (C.c_uint32 * len(edges))(*edges)
            t = (C.c_double * len(thr))(*thr) if thr is not None else None
            out = _abi.AfOutputs(0, None, 50, C.c_void_p(blk_t.data_ptr() if samples else None), C.c_void_p(counts_t.data_ptr()))
            req = _abi.AfSeriesWindows(3, n_groups, len(edges) - 1 if n_windows is None else n_windows, None, e, t,
                                       C.c_void_p(outs.data_ptr()), C.c_void_p(outs.data_ptr() + 1024), None, None, None, 0.0, 0)
            rc = lib.af_engine_summarize_series_windows(eng._h, C.byref(out), C.byref(req))  # noqa: SLF001
            return rc, lib.af_last_error().decode()

        assert call([0, 10, 10])[0] == _abi.AF_ERR_INVALID and "strictly increasing" in call([0, 10, 10])[1]
        assert call([10, 5])[0] == _abi.AF_ERR_INVALID
        assert call([0], n_windows=0)[0] == _abi.AF_ERR_INVALID
        rc, msg = call([0, 10], thr=[0.0] * 5 + [float("nan")] + [0.0] * 6)
        assert rc == _abi.AF_ERR_INVALID and "NaN" in msg
        rc, msg = call([0, 10], samples=False)
        assert rc == _abi.AF_ERR_INVALID and "samples" in msg
        rc, msg = call([0, 10], n_groups=0xFFFFFFFF)
        assert rc == _abi.AF_ERR_CAPACITY and "2^32" in msg
        assert call([0, 10])[0] == _abi.AF_OK and (outs[:1].cpu().numpy() == 10 + 10 + 0).all()
    finally:
        eng.close()


def _cells_on_the_host(res, ids, n_groups, edges, thr=None):
    """results.series_window_stats on every cell's samples: the members' window rows concatenated in scenario order."""
    W, S = len(edges) - 1, res.plan.n_series
    out = {"count": np.zeros((n_groups, W), dtype=np.int64), "mean": np.full((n_groups, W, S), np.nan),
           "min": np.zeros((n_groups, W, S), dtype=np.uint32), "max": np.zeros((n_groups, W, S), dtype=np.uint32),
           "above": np.zeros((n_groups, W, S), dtype=np.uint32)}
    words = [res[s]._samples for s in range(len(res))]  # noqa: SLF001
    for g in range(n_groups):
        members = np.nonzero(ids == g)[0]
        for w in range(W):
            seg = [words[s][:, min(edges[w], words[s].shape[1]):min(edges[w + 1], words[s].shape[1])] for s in members]
            cell = np.concatenate(seg, axis=1) if seg else np.zeros((S, 0), dtype=np.uint32)
            st = series_window_stats(cell, [0, max(cell.shape[1], 1)], res.plan.n_edges, thr)
            for k in out:
                out[k][g, w] = st[k][0]
    return out


def _api_as_numpy(a):
    return {"count": a["count"].cpu().numpy().astype(np.uint32), "mean": a["mean"].cpu().numpy(),
            "min": a["min_words"].cpu().numpy().view(np.uint32), "max": a["max_words"].cpu().numpy().view(np.uint32),
            "above": a["above"].cpu().numpy().view(np.uint32)}


def test_event_workload_through_the_python_api():
    from statistics import NormalDist

    from asyncflow_amd import expand_grid
    from asyncflow_amd.runner import SimulationRunner

    payload = lb_with_events(horizon=60, scale=0.1)
    # ---- 64 seeds: one group, six groups, singletons
    seeds = 0xE7E70000 + np.arange(64, dtype=np.uint64)
    res = SimulationRunner(simulation_input=payload, seeds=seeds).run()
    names = res.series_names()
    per_window = int(round(2.0 / res.plan.sample_period))
    edges = tick_window_edges(per_window, res.plan.tick_count)
    thr = {names[0]: 0.5, next(k for k in names if k.endswith("ram_in_use")): 64.0}
    thr_vec = res._series_thresholds(thr)  # noqa: SLF001
    for by, ids, g in ((None, np.zeros(64, dtype=np.int64), 1), (np.arange(64) % 6, np.arange(64) % 6, 6)):
        a = res.series_window_summary(2.0, by=by, thresholds=thr)
        assert np.array_equal(a["tick_edges"], edges) and a["series"] == names and a["replicas"].tolist() == np.bincount(ids).tolist()
        assert np.array_equal(a["times"], edges[:-1] * res.plan.sample_period) and a["count"].dtype.is_floating_point is False
        _same(_api_as_numpy(a), _cells_on_the_host(res, ids, g, edges, thr_vec), f"by={by!r}")
        b = res.series_window_summary(ticks_per_window=per_window, by=by, thresholds=thr_vec)
        for k in ("count", "mean", "min_words", "max_words", "above"):
            assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
    a = res.series_window_summary(2.0, by="scenario")
    got = _api_as_numpy(a)
    for s in range(64):
        host = res[s].get_series_window_stats(2.0)
        _same({k: v[s:s + 1] for k, v in got.items()}, {k: v[None] for k, v in host.items()}, f"scenario {s}")
    # the decoded values: counts as they are, the ram columns from their float32 bits, NaN where the window is empty
    ram = ram_columns(len(names), res.plan.n_edges)
    cnt = a["count"].cpu().numpy()
    assert (cnt > 0).all()
    mx = a["max"].cpu().numpy()
    assert np.array_equal(mx[:, :, ~ram], got["max"][:, :, ~ram].astype(np.float64))
    assert np.array_equal(mx[:, :, ram], got["max"][:, :, ram].view(np.float32).astype(np.float64))
    assert np.array_equal(a["above_share"].cpu().numpy(), got["above"] / cnt[:, :, None])
    past = res.series_window_summary(tick_edges=[0, 5, res.plan.tick_count + 5, res.plan.tick_count + 9], by="scenario")
    for k in ("mean", "min", "max", "above_share"):
        assert np.isnan(past[k][:, 2].cpu().numpy()).all() and not np.isnan(past[k][:, :2].cpu().numpy()).any()
    assert (past["count"][:, 2] == 0).all() and (past["min_words"][:, 2] == 0).all()

    # ---- one window over the whole run is the per-scenario series summary
    whole = res.series_window_summary(tick_edges=[0, res.plan.tick_count], by="scenario")
    summ = res.summary(rps=False, series=True)
    assert whole["mean"][:, 0].cpu().numpy().tobytes() == summ["series_mean"].cpu().numpy().tobytes()
    assert np.array_equal(whole["max_words"][:, 0].cpu().numpy(), summ["series_max"].cpu().numpy())

    # ---- a 3 x 2 grid with 4 replicas: by=Sweep, bands over the replicas, the on-disk summary
    users = "rqs_input.avg_active_users.mean"
    grid = expand_grid({users: [40.0, 120.0, 300.0], "topology_graph.edges[*].latency.mean": [0.002, 0.006]},
                       replicas=4, order_by_load=users)
    res = SimulationRunner(simulation_input=payload, **grid.runner_kwargs()).run()
    a = res.series_window_summary(2.0, by=grid)
    assert tuple(a["mean"].shape) == (6, len(edges) - 1, len(names)) and a["replicas"].tolist() == [4] * 6
    _same(_api_as_numpy(a), _cells_on_the_host(res, grid.point, 6, edges), "by=grid")
    z = NormalDist().inv_cdf(0.95)
    edges_b = np.concatenate([edges, [edges[-1] + 40]])              # the last window lies past the run: no replica has a sample
    for of in ("mean", "max", "above_share"):
        bands = res.series_window_bands(tick_edges=edges_b, by=grid, of=of, level=0.9, q=(0.1, 0.75))
        per = res.series_window_summary(tick_edges=edges_b, by="scenario")
        values, counts = per[of].cpu().numpy(), per["count"].cpu().numpy()
        for g in range(6):
            members = np.nonzero(grid.point == g)[0]
            for w in range(len(edges_b) - 1):
                body = values[members, w][counts[members, w] > 0]
                assert bands["n"][g, w] == body.shape[0]
                if body.shape[0] == 0:
                    for k in ("mean", "std", "ci_halfwidth", "q_lo", "q_hi"):
                        assert np.isnan(bands[k][g, w]).all(), (k, g, w)
                    continue
                sd = body.std(axis=0, ddof=1)
                np.testing.assert_allclose(bands["mean"][g, w], body.mean(axis=0), rtol=1e-12, atol=0.0)
                np.testing.assert_allclose(bands["std"][g, w], sd, rtol=1e-12, atol=0.0)
                np.testing.assert_allclose(bands["ci_halfwidth"][g, w], z * sd / np.sqrt(body.shape[0]), rtol=1e-12, atol=0.0)
                np.testing.assert_allclose(bands["q_lo"][g, w], np.quantile(body, 0.1, axis=0), rtol=1e-12, atol=0.0)
                np.testing.assert_allclose(bands["q_hi"][g, w], np.quantile(body, 0.75, axis=0), rtol=1e-12, atol=0.0)
        assert (bands["n"][:, -1] == 0).all() and (bands["n"][:, :-1] == 4).all()
        pooled = res.series_window_summary(tick_edges=edges_b, by=grid)[of].cpu().numpy()
        assert np.array_equal(bands["pooled"], pooled, equal_nan=True) and np.isnan(bands["pooled"][:, -1]).all()
    with pytest.raises(ValueError, match="of must be"):
        res.series_window_bands(2.0, of="min")
    with pytest.raises(ValueError, match="by must be"):
        res.series_window_summary(2.0, by="point")

    res2 = SimulationRunner(simulation_input=lb_two_servers(horizon=10), seeds=seeds[:4], collect_samples=False).run()
    for call in (res2.series_window_summary, res2.series_window_bands):
        with pytest.raises(RuntimeError, match="kept no sampled series"):
            call()


def _round_trip(path: str) -> None:
    """save_series_window_summary of a 3 x 2 grid with 4 replicas, one row per point, read back by load_summary."""
    from asyncflow_amd import expand_grid
    from asyncflow_amd.results import load_summary
    from asyncflow_amd.runner import SimulationRunner

    users = "rqs_input.avg_active_users.mean"
    grid = expand_grid({users: [40.0, 120.0, 300.0], "topology_graph.edges[*].latency.mean": [0.002, 0.006]},
                       replicas=4, order_by_load=users)
    res = SimulationRunner(simulation_input=lb_with_events(horizon=60, scale=0.1), **grid.runner_kwargs()).run()
    names = res.series_names()
    edges = tick_window_edges(int(round(2.0 / res.plan.sample_period)), res.plan.tick_count)
    thr = {names[0]: 0.5, next(k for k in names if k.endswith("ram_in_use")): 64.0}
    pooled = res.series_window_summary(2.0, by=grid, thresholds=thr)
    bands = res.series_window_bands(2.0, by=grid, thresholds=thr, of="mean", q=(0.05, 0.95))
    written = res.save_series_window_summary(path, grid, window_s=2.0, thresholds=thr)
    back = load_summary(path)
    assert set(back) == set(written)
    for k, v in written.items():
        assert np.array_equal(np.asarray(back[k], dtype=v.dtype), v, equal_nan=v.dtype.kind == "f"), k
    for k, v in grid.point_columns().items():
        assert np.array_equal(back[f"param:{k}"], v)
    for j, sname in enumerate(names):
        for col, want in (("mean", pooled["mean"]), ("max", pooled["max"]), ("above", pooled["above_share"])):
            assert np.array_equal(back[f"series_window_{col}:{sname}"], want.cpu().numpy()[:, :, j], equal_nan=True), (col, sname)
        assert np.array_equal(back[f"series_window_q05:{sname}"], bands["q_lo"][:, :, j], equal_nan=True)
        assert np.array_equal(back[f"series_window_q95:{sname}"], bands["q_hi"][:, :, j], equal_nan=True)
        assert back[f"series_window_q95:{sname}"].shape == (6, len(edges) - 1)
    assert np.array_equal(back["series_window_tick_edges"], edges) and back["replicas"].tolist() == [4] * 6
    assert np.array_equal(back["series_window_times"], edges[:-1] * res.plan.sample_period)


def test_save_series_window_summary_npz(tmp_path):
    _round_trip(str(tmp_path / "series_windows.npz"))


def test_save_series_window_summary_parquet(tmp_path):
    pytest.importorskip("pyarrow")
    _round_trip(str(tmp_path / "series_windows.parquet"))


def test_many_singleton_cells():
    """2 000 LB-2 replicas at T = 600 s, 600 windows of 1 s, every replica its own group: 14.4 M (cell, series) entries, written
    by the streaming pass itself; no per-record scratch."""
    from asyncflow_amd.runner import SimulationRunner

    n = 2000
    seeds = 0xC0FFEE00 + np.arange(n, dtype=np.uint64)
    res = SimulationRunner(simulation_input=lb_two_servers(horizon=600), seeds=seeds, collect_clock=False).run()
    a = res.series_window_summary(1.0, by="scenario")
    S = res.plan.n_series
    assert tuple(a["mean"].shape) == (n, 600, S) and n * 600 * S == 14_400_000
    bound = _scratch_bound(n, n, 600, S, False)
    print(f"scratch_bytes {a['scratch_bytes']} bound {bound} series_window_ms {a['series_window_ms']:.2f}")
    assert 0 < a["scratch_bytes"] <= bound
    assert int(a["count"].sum()) == int(np.minimum(res.counts[:, _abi.CNT_TICKS], res.plan.tick_count).sum())
    got = _api_as_numpy(a)
    rng = np.random.default_rng(77)
    for s in rng.choice(n, 32, replace=False):
        host = res[int(s)].get_series_window_stats(1.0)
        _same({k: v[s:s + 1] for k, v in got.items()}, {k: v[None] for k, v in host.items()}, f"scenario {s}")
