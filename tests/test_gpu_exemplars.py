"""The k slowest requests per window and group on the MI355X (af_engine_summarize_exemplars, asyncflow_amd/csrc/af_exemplars.hpp):
every output word of every cell against the host definition (results.latency_exemplars).  Synthetic clocks through the C ABI on
a single-server plan: the wave and unroll seams of the row walk, k on both sides of the cells' sizes, latency orders in which
every chunk displaces the list, ties across the k-th place and a member seam, signed zeros, subnormals, negative and infinite
latencies, NaN rows, rows behind the stored ones, window counts on both sides of the kernel's LDS switch, times on the edges, both
window rules, group arrangements, the optional outputs, every refusal, the state met on arrival, the independence of the launch
and the identities with the windowed analyzers.  Every output of a call lies in ONE buffer with sentinel words on both sides of
each.  An event workload goes through the Python API."""

from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from asyncflow_amd import _abi
from asyncflow_amd.plan import lower
from asyncflow_amd.results import latency_exemplars, load_summary, ram_columns
from oracle.scenarios import lb_with_events, single_server

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
LDS_WINDOWS = int(re.search(r"constexpr\s+uint32_t\s+kLdsExemplarWindows\s*=\s*(\d+)\s*;",
                            (ROOT / "asyncflow_amd" / "csrc" / "af_exemplars.hpp").read_text()).group(1))
P = 2.0 ** -5
ROWS = [0, 1, 63, 64, 65, 129, 1025]                # the wave and unroll seams of the row walk
KS = (1, 2, 63, 64)
ORDERS = ("ascending", "descending", "random", "equal", "ties")
SENTINEL = 0x5A5A5A5A
GUARD = 16                                          # sentinel words on both sides of every output
KEYS = ("total", "kept", "scenario", "row", "clock", "state")
ONES = 0xFFFFFFFF


@pytest.fixture(scope="module")
def plan():
    p = lower(single_server(horizon=50, period=P))
    assert p.sample_period == P and p.n_series == 6
    return p


@pytest.fixture(scope="module")
def eng(plan):
    from asyncflow_amd.engine import Engine

    e = Engine(plan, 0)
    yield e
    e.close()


def _clock(rng, m, order, horizon=40.0):
    """m rows with finish times over (0, horizon] in completion order and latencies in the given order along the rows."""
    finish = np.sort(rng.integers(1, int(horizon * 64), m) / 64.0)
    lat = {"ascending": np.arange(m) / 128.0,                     # every chunk of rows displaces the kept list
           "descending": np.arange(m, 0, -1) / 128.0,
           "random": rng.integers(0, 4096, m) / 256.0,
           "equal": np.full(m, 0.75),
           "ties": rng.integers(0, 3, m) * 0.5}[order]            # long runs of equal latencies across the k-th place
    return np.stack([finish - lat, finish], axis=1)


class _Batch:
    """Clocks, counts and (optionally) sample rows on the device; rows behind a scenario's stored ones hold huge latencies that
    would win every cell if they were read."""

    def __init__(self, clocks, cap=None, counts_extra=0, ticks=None, tick_cap=0, n_series=6):
        import torch

        n = len(clocks)
        self.n, self.S = n, n_series
        self.cap = cap or max(max((len(x) for x in clocks), default=1), 1) + 3
        clock = np.empty((n, self.cap, 2))
        clock[:, :, 0], clock[:, :, 1] = 1.0, 1.0e9
        counts = np.zeros((n, _abi.CNT_SLOTS), dtype=np.uint32)
        self.stored = []
        for i, rows in enumerate(clocks):
            rows = np.asarray(rows, dtype=np.float64).reshape(-1, 2)
            counts[i, _abi.CNT_COMPLETED] = rows.shape[0] + counts_extra
            keep = rows[: self.cap]
            clock[i, : keep.shape[0]] = keep
            self.stored.append(clock[i, : min(rows.shape[0] + counts_extra, self.cap)].copy())
        self.dev = torch.device("cuda", 0)
        self.tick_cap, self.samples_t, self.words = int(tick_cap), None, None
        if tick_cap:
            pitch = (n_series + 3) & ~3
            rng = np.random.default_rng(99)
            raw = rng.integers(0, 50, (n, tick_cap, pitch)).astype(np.uint32)
            raw[:, :, 5] = rng.random((n, tick_cap)).astype(np.float32).view(np.uint32) | np.uint32(0x40000000)   # ram_in_use: f32 bits
            raw[:, :, n_series:] = 0xDEADBEEF                                       # the padding of the pitch is never read
            self.samples_t = torch.as_tensor(raw.view(np.int32), device=self.dev)
            for i in range(n):
                counts[i, _abi.CNT_TICKS] = ticks[i]
            self.words = [np.ascontiguousarray(raw[i, : min(int(ticks[i]), tick_cap), :n_series].T) for i in range(n)]
        self.clock_t = torch.as_tensor(clock, device=self.dev)
        self.counts_t = torch.as_tensor(counts.view(np.int32), device=self.dev)

    def layout(self, cells, k, want):
        sizes = {"total": 2 * cells, "kept": cells, "scenario": cells * k, "row": cells * k, "clock": 4 * cells * k, "state": cells * k * self.S}
        off, at = {}, GUARD
        for key in KEYS:
            if key in want:
                off[key] = (at, sizes[key])
                at += ((sizes[key] + 3) & ~3) + GUARD            # (multiples of four words: the pairs stay 16-byte aligned)
        return off, at

    def run(self, eng, group, n_groups, edges, k, window_of="finish", *, want=KEYS, buf=None):
        """One call; returns the outputs (numpy) after checking that no word outside them changed."""
        import torch

        want = tuple(key for key in want if key != "state" or self.tick_cap)
        n_win = 1 if edges is None else len(edges) - 1
        cells = n_groups * n_win
        off, total = self.layout(cells, k, want)
        if buf is None:
            buf = torch.full((total,), SENTINEL, dtype=torch.int32, device=self.dev)
        grp_t = None
        if group is not None:
            grp = np.asarray(group, dtype=np.int64)
            grp_t = torch.as_tensor(np.where(grp < 0, _abi.POOL_SKIP, grp).astype(np.uint32).view(np.int32), device=self.dev)
        ptr = {key: buf.data_ptr() + 4 * o for key, (o, _) in off.items()}
        state = "state" in want
        torch.cuda.synchronize(self.dev)
        ms, scratch = eng.summarize_exemplars(
            self.n, n_groups, k, edges=edges, window_of=window_of, clock_ptr=self.clock_t.data_ptr(), clock_capacity=self.cap,
            counts_ptr=self.counts_t.data_ptr(), total_ptr=ptr["total"], kept_ptr=ptr.get("kept", 0), scenario_ptr=ptr["scenario"],
            row_ptr=ptr["row"], pair_ptr=ptr["clock"], state_ptr=ptr.get("state", 0),
            samples_ptr=self.samples_t.data_ptr() if state else 0, tick_capacity=self.tick_cap if state else 0, sample_period=P,
            group_ptr=grp_t.data_ptr() if grp_t is not None else 0)
        assert ms >= 0.0 and scratch >= self.n * n_win * (12 * k + 4)
        words = buf.cpu().numpy().view(np.uint32)
        inside = np.zeros(total, dtype=bool)
        out = {}
        for key, (o, size) in off.items():
            inside[o: o + size] = True
            out[key] = words[o: o + size].copy()
        assert (words[~inside] == SENTINEL).all(), "a word outside the outputs changed"
        out["total"] = out["total"].view(np.uint64).reshape(n_groups, n_win)
        out["clock"] = out["clock"].view(np.uint64).reshape(n_groups, n_win, k, 2)
        for key, shape in (("kept", ()), ("scenario", (k,)), ("row", (k,)), ("state", (k, self.S))):
            if key in out:
                out[key] = out[key].reshape((n_groups, n_win) + shape)
        out["buf"] = buf
        return out

    def check(self, got, group, n_groups, edges, k, window_of="finish"):
        """Every word of every cell of `got` against the host definition."""
        grp = np.zeros(self.n, dtype=np.int64) if group is None else np.asarray(group, dtype=np.int64)
        for g in range(n_groups):
            ids = [s for s in range(self.n) if grp[s] == g]
            kw = {"samples": [self.words[s] for s in ids], "sample_period": P} if "state" in got and ids else {}
            want = latency_exemplars([self.stored[s] for s in ids], k, edges, window_of, scenario_ids=ids, **kw)
            assert np.array_equal(got["total"][g], want["total"]), (g, got["total"][g], want["total"])
            if "kept" in got:
                assert np.array_equal(got["kept"][g], want["kept"]), g
            for key in ("scenario", "row"):
                assert np.array_equal(got[key][g], want[key]), (key, g, k, window_of)
            assert np.array_equal(got["clock"][g], want["clock"].view(np.uint64)), (g, k, window_of)
            if "state" in got:
                assert np.array_equal(got["state"][g], want["state"]) if ids else (got["state"][g] == ONES).all(), (g, k)
        return got


@pytest.mark.parametrize("order", ORDERS)
def test_row_counts_k_and_latency_orders(eng, order):
    rng = np.random.default_rng(ORDERS.index(order))
    b = _Batch([_clock(rng, m, order) for m in ROWS])
    seen = 0
    for k in KS:
        for group, G in ((np.arange(b.n), b.n), (None, 1), ([0, 2, 2, -1, 0, 2, 4], 5)):   # singletons; one group; uneven, an empty group, a skip
            for edges in (None, [0.0, 40.0], [0.5, 19.0, 41.0]):
                for window_of in ("finish",) if edges is None else ("finish", "arrival"):
                    got = b.check(b.run(eng, group, G, edges, k, window_of), group, G, edges, k, window_of)
                    seen += int((got["total"] > k).sum())
    assert seen > 50                                                  # cells that hold more rows than are kept
    if order in ("equal", "ties"):                                    # equal latencies straddle the k-th place and the member seam
        got = b.run(eng, None, 1, None, 64)
        lat = got["clock"][0, 0, :, 1].view(np.float64) - got["clock"][0, 0, :, 0].view(np.float64)
        assert lat[0] == lat[63] and len(set(got["scenario"][0, 0].tolist())) >= 2


@pytest.mark.parametrize("k", KS)
def test_cells_with_fewer_than_k_exactly_k_and_one_more(eng, k):
    m = 3 * k + 5
    rng = np.random.default_rng(40 + k)
    rows = [np.stack([np.arange(1, m + 1) - lat, np.arange(1, m + 1).astype(np.float64)], axis=1)
            for lat in (rng.integers(0, 8, m) / 8.0, np.full(m, 0.5), np.arange(m) / 64.0)]
    b = _Batch(rows)
    edges = [0.0, max(k - 1, 0) + 0.0, 2 * k - 1.0, 3 * k + 0.0, 3 * k + 5.0]
    if k == 1:
        edges = [-1.0, 0.0, 1.0, 3.0, 8.0]                            # windows of 0, 1, 2 rows
    got = b.check(b.run(eng, np.arange(3), 3, edges, k), np.arange(3), 3, edges, k)
    assert got["total"][0, :3].tolist() == [k - 1, k, k + 1] and got["kept"][0, :3].tolist() == [k - 1, k, k]
    for group, G in ((None, 1), ([0, 1, 0], 2)):
        b.check(b.run(eng, group, G, edges, k), group, G, edges, k)
        b.check(b.run(eng, group, G, [e - 0.25 for e in edges], k, "arrival"), group, G, [e - 0.25 for e in edges], k, "arrival")


def test_special_values_and_rows_behind_the_stored_ones(eng):
    nan, inf = float("nan"), float("inf")
    a = np.array([[1.0, 3.0], [2.0, 4.0], [1.0, 1.0], [5.0, 5.0], [0.5, inf], [nan, 2.0], [2.0, nan], [3.0, 2.0], [-inf, 1.0],
                  [4.0, 4.0], [inf, inf], [1.0, 2.0], [6.0, 2.0], [1.0, inf]])
    z = np.array([[0.0, 2.0], [0.0, -0.0], [-0.0, 0.0], [2.0, 4.0], [1.5, 3.5], [1e-310, 3e-310], [0.0, 5e-324], [5e-324, 0.0],
                  [3.0, 3.0 - 2.0 ** -50], [-1e300, 1e300]])
    rng = np.random.default_rng(7)
    noisy = _clock(rng, 300, "random", 6.0)
    noisy[rng.choice(300, 40, replace=False), 0] = nan
    noisy[rng.choice(300, 40, replace=False), 1] = nan
    noisy[rng.choice(300, 30, replace=False), 1] = inf
    noisy[rng.choice(300, 60, replace=False)] *= -1.0                 # negative times: finish < start, negative latencies
    clocks = [a, z, np.zeros((0, 2)), noisy, np.array([[7.0, 9.0]] * 70)]
    for extra in (0, 2, 1000):                                        # counts at and above the clock capacity
        b = _Batch(clocks, cap=303, counts_extra=extra)
        for k in (1, 3, 64):
            for group, G in ((None, 1), (np.arange(5), 5), ([1, 1, 0, -1, 0], 3)):
                for edges, window_of in ((None, "finish"), ([0.0, 1.0, 2.0, 4.0, 5.0], "finish"), ([0.0, 1.0, 2.0, 4.0, 5.0], "arrival"),
                                         ([-6.0, -2.0, 2.0 ** -50, 3.0, 1e9], "finish"), ([-1e301, 0.0, 1e-310, 5.0], "arrival")):
                    b.check(b.run(eng, group, G, edges, k, window_of), group, G, edges, k, window_of)
    got = b.run(eng, np.arange(5), 5, None, 3)
    assert int(got["total"][4, 0]) == 303 and got["row"][4, 0, 0] == 70              # counts above the capacity: the capacity's rows
    got = _Batch(clocks, cap=303).run(eng, np.arange(5), 5, None, 3)
    assert got["row"][0, 0].tolist() == [4, 8, 13] and got["total"][0, 0] == 11      # the +inf latencies first, by row
    assert got["row"][1, 0].tolist() == [9, 0, 3] and got["total"][1, 0] == 10
    assert int(got["total"][4, 0]) == 70 and got["row"][4, 0].tolist() == [0, 1, 2]  # the rows behind the stored ones are not read


@pytest.mark.parametrize("n_win", [1, 2, 63, 600, LDS_WINDOWS, LDS_WINDOWS + 1])
def test_window_counts_on_both_sides_of_the_lds_switch(eng, n_win):
    rng = np.random.default_rng(n_win)
    edges = np.arange(n_win + 1) * 0.5 + 1.0
    clocks = []
    for m in (1025, 129, 64):
        t = rng.integers(0, 2 * (n_win + 4), m) * 0.25 + rng.choice([0.0, 0.0, 2.0 ** -20, -2.0 ** -20], m)   # on the edges, beside them,
        lat = rng.integers(0, 5, m) * 0.125                                                                  # before e[0], past e[W]
        clocks.append(np.stack([t - lat, t], axis=1))                 # NOT in completion order: 64 distinct windows in a chunk
    b = _Batch(clocks)
    if n_win >= 63:
        w = np.searchsorted(edges, clocks[0][:64, 1], side="left")
        assert len(set(w.tolist())) >= (40 if n_win > 63 else 30)
    for k in (2, 64) if n_win <= 600 else (2,):
        for group, G in (([0, 0, 1], 2), (None, 1)):
            for window_of in ("finish", "arrival"):
                got = b.check(b.run(eng, group, G, edges, k, window_of), group, G, edges, k, window_of)
    assert int(got["total"].sum()) > 0


def test_whole_run_is_one_window(eng):
    rng = np.random.default_rng(3)
    b = _Batch([_clock(rng, m, "random") for m in (700, 0, 65)])
    for k in (1, 16, 64):
        got = b.check(b.run(eng, [0, 0, 1], 2, None, k), [0, 0, 1], 2, None, k)
    assert got["total"][:, 0].tolist() == [700, 65]


def test_optional_outputs_present_and_absent(eng):
    rng = np.random.default_rng(4)
    ticks = [300, 200, 0]
    b = _Batch([_clock(rng, m, "random", 9.0) for m in (200, 64, 10)], ticks=ticks, tick_cap=256)
    edges, group = [0.0, 3.0, 3.5, 9.0], [0, 1, 0]
    for drop in ((), ("kept",), ("state",), ("kept", "state")):
        want = tuple(key for key in KEYS if key not in drop)
        got = b.run(eng, group, 2, edges, 5, want=want)
        assert set(got) - {"buf"} == set(want)
        b.check(got, group, 2, edges, 5)


def test_state_met_on_arrival(eng):
    t_s = [40, 64, 100, 0]                                            # below, at and above the tick capacity; no ticks
    starts = np.concatenate([np.arange(-2, 70) * P, np.arange(0, 70) * P + P * 2.0 ** -30, np.arange(1, 70) * P - P * 2.0 ** -30,
                             [np.nan, -0.0, 1e300, 40 * P, 41 * P, 64 * P, 65 * P]])
    clocks = [np.stack([starts, starts + 1.0 + np.arange(len(starts)) * 2.0 ** -10], axis=1) for _ in t_s]
    b = _Batch(clocks, ticks=t_s, tick_cap=64)
    for k, group, G, edges, window_of in ((64, np.arange(4), 4, None, "finish"), (64, None, 1, [-1.0, 0.5, 1.0, 1.5, 3.0], "arrival"),
                                          (7, [0, 0, 1, 1], 2, [0.0, 1.0, 2.0, 2.5], "arrival"), (64, [0, -1, 0, 0], 1, [1.0, 2.0, 4.0], "finish")):
        got = b.check(b.run(eng, group, G, edges, k, window_of), group, G, edges, k, window_of)
        assert not (got["state"] == 0xDEADBEEF).any()
    got = b.run(eng, np.arange(4), 4, [-1.0, 5.0], 64, "arrival")
    some = got["state"][:3][got["scenario"][:3] != ONES]
    assert (some[:, 0] != ONES).any() and (some[:, 0] == ONES).any()                  # rows with a state and rows without one
    assert ((some[:, 5] >> 30) == 1).any()                                             # the ram_in_use words stay f32 bits
    assert (got["state"][3] == ONES).all()                                             # a scenario without ticks has no state


def test_refusals_leave_every_output_word_alone(eng, plan):
    import torch

    from asyncflow_amd.engine import PLAN_ONLY, Engine

    rng = np.random.default_rng(15)
    b = _Batch([_clock(rng, 40, "random") for _ in range(3)], ticks=[50, 50, 50], tick_cap=64)
    lib, dev = eng._lib, b.dev  # noqa: SLF001
    k, cells = 4, 3 * 2
    off, total = b.layout(cells, k, KEYS)
    buf = torch.full((total,), SENTINEL, dtype=torch.int32, device=dev)
    grp_ok = torch.zeros(3, dtype=torch.int32, device=dev)
    grp_bad = torch.as_tensor(np.array([0, 3, 1], dtype=np.int32), device=dev)

    def call(handle=None, *, n=3, n_groups=3, edges=(0.0, 10.0, 64.0), by_arrival=0, kk=k, period=P, group=grp_ok, clock=True, counts=True,
             samples=True, tick_cap=64, drop=(), n_win=None, misalign=False):
        e = np.ascontiguousarray(edges, dtype=np.float64) if edges is not None else None
        out = _abi.AfOutputs(b.cap, C.c_void_p(b.clock_t.data_ptr() if clock else None), tick_cap,
                             C.c_void_p(b.samples_t.data_ptr() if samples else None), C.c_void_p(b.counts_t.data_ptr() if counts else None))
        p = {key: C.c_void_p(None if key in drop else buf.data_ptr() + 4 * off[key][0] + (8 if misalign and key == "clock" else 0)) for key in KEYS}
        req = _abi.AfExemplars(n, n_groups, (e.shape[0] - 1 if e is not None else 0) if n_win is None else n_win,
                               C.c_void_p(group.data_ptr() if group is not None else None),
                               e.ctypes.data_as(C.POINTER(C.c_double)) if e is not None else None, by_arrival, kk, period,
                               p["total"], p["kept"], p["scenario"], p["row"], p["clock"], p["state"], 0.0, 0)
        torch.cuda.synchronize(dev)
        rc = lib.af_engine_summarize_exemplars(handle or eng._h, C.byref(out), C.byref(req))  # noqa: SLF001
        assert (buf.cpu().numpy().view(np.uint32) == SENTINEL).all(), "a refused call wrote an output word"
        return rc

    inv, cap_err = _abi.AF_ERR_INVALID, _abi.AF_ERR_CAPACITY
    assert call(n=0) == inv and call(n_groups=0) == inv
    assert call(kk=0) == inv and call(kk=65) == inv and b"AF_MAX_EXEMPLARS" in lib.af_last_error()
    assert call(edges=(0.0, 10.0, 10.0)) == inv and b"strictly increasing" in lib.af_last_error()
    assert call(edges=(5.0, 4.0, 9.0)) == inv
    assert call(edges=(0.0, float("inf"), float("inf"))) == inv and b"not finite" in lib.af_last_error()
    assert call(edges=(0.0, float("nan"), 3.0)) == inv
    assert call(edges=None, n_win=2) == inv                            # windows without edges
    assert call(edges=(0.0, 1.0), n_win=0) == inv                      # edges without windows
    assert call(edges=None, by_arrival=1) == inv and b"arrival" in lib.af_last_error()
    assert call(group=grp_bad) == inv and b"group id" in lib.af_last_error()
    assert call(clock=False) == inv and call(counts=False) == inv
    for key in ("total", "scenario", "row", "clock"):
        assert call(drop=(key,)) == inv, key
    assert call(misalign=True) == inv
    assert call(samples=False) == inv and call(tick_cap=0) == inv
    for bad in (0.0, -P, float("nan"), float("inf"), -float("inf")):
        assert call(period=bad) == inv, bad
    wide = np.arange(2 ** 20 + 1, dtype=np.float64)
    assert call(n_groups=2 ** 10, edges=wide, kk=64, group=None) == cap_err              # n_groups * W' * k = 2^36
    assert call(n_groups=1, n=2 ** 12, edges=wide, kk=1, group=None) == cap_err          # n_scenarios * W' * k = 2^32
    plan_only = Engine(plan, PLAN_ONLY)
    try:
        assert call(plan_only._h) == _abi.AF_ERR_NO_DEVICE  # noqa: SLF001
    finally:
        plan_only.close()
    ok = b.run(eng, [0, 1, 2], 3, [0.0, 10.0, 64.0], k)
    b.check(ok, [0, 1, 2], 3, [0.0, 10.0, 64.0], k)


def test_sample_period_is_used_with_state_only(eng):
    import torch

    rng = np.random.default_rng(17)
    b = _Batch([_clock(rng, 40, "random")])
    off, total = b.layout(1, 2, ("total", "scenario", "row", "clock"))
    buf = torch.full((total,), SENTINEL, dtype=torch.int32, device=b.dev)
    p = {key: buf.data_ptr() + 4 * o for key, (o, _) in off.items()}
    eng.summarize_exemplars(1, 1, 2, clock_ptr=b.clock_t.data_ptr(), clock_capacity=b.cap, counts_ptr=b.counts_t.data_ptr(),
                            total_ptr=p["total"], scenario_ptr=p["scenario"], row_ptr=p["row"], pair_ptr=p["clock"], sample_period=float("nan"))
    assert buf.cpu().numpy().view(np.uint32)[off["total"][0]] == 40


def test_cells_do_not_depend_on_the_launch_or_the_batch(eng):
    rng = np.random.default_rng(16)
    ticks = [64, 30, 64, 64, 10]
    mine = [_clock(rng, m, o) for m, o in zip((900, 300, 64, 1025, 10), ("random", "ties", "equal", "ascending", "random"))]
    others = [_clock(rng, m, "ties") for m in (500, 0, 129, 700)]
    edges, k = [0.0, 7.0, 7.5, 25.0, 41.0], 9
    a = _Batch(mine, cap=1100, ticks=ticks, tick_cap=64)
    first = a.check(a.run(eng, np.arange(5), 5, edges, k), np.arange(5), 5, edges, k)
    again = a.run(eng, np.arange(5), 5, edges, k, buf=first["buf"])       # the same buffers, written a second time
    order = [3, 0, 4, 2, 1]
    mixed = _Batch([others[0], mine[3], others[1], mine[0], mine[4], others[2], mine[2], mine[1], others[3]], cap=1100,
                   ticks=[64, ticks[3], 64, ticks[0], ticks[4], 64, ticks[2], ticks[1], 64], tick_cap=64)
    mixed.samples_t[[1, 3, 4, 6, 7]] = a.samples_t[order]
    for w, o in zip([1, 3, 4, 6, 7], order):
        mixed.words[w] = a.words[o]
    where = np.array([1, 3, 4, 6, 7])
    other = mixed.check(mixed.run(eng, np.arange(9), 9, edges, k), np.arange(9), 9, edges, k)
    for key in ("total", "kept", "row", "clock", "state"):
        assert np.array_equal(first[key], again[key]), key
        assert np.array_equal(first[key][order], other[key][where]), key      # alone and inside a batch of singletons: the same words
    assert np.array_equal(first["scenario"], again["scenario"])
    solo = _Batch([mine[3]], cap=1100, ticks=[ticks[3]], tick_cap=64)
    solo.samples_t[0] = a.samples_t[3]
    solo.words[0] = a.words[3]
    alone = solo.check(solo.run(eng, None, 1, edges, k), None, 1, edges, k)
    for key in ("total", "kept", "row", "clock", "state"):
        assert np.array_equal(alone[key][0], first[key][3]), key


@pytest.mark.parametrize("window_of", ["finish", "arrival"])
def test_slot_zero_is_the_windowed_analyzers_max_and_total_is_its_total(eng, window_of):
    import torch

    rng = np.random.default_rng(18)
    b = _Batch([_clock(rng, m, "random") for m in (1025, 300, 0, 64, 129)])          # sorted by finish: the by-finish call needs it
    edges = np.array([0.0, 3.0, 3.25, 10.0, 26.0, 40.0, 50.0])
    for group, G in ((None, 1), (np.arange(5), 5), ([0, 1, -1, 1, 0], 2)):
        got = b.check(b.run(eng, group, G, edges, 1, window_of), group, G, edges, 1, window_of)
        stats = torch.empty((G, 6, 8), dtype=torch.float64, device=b.dev)
        grp_t = None
        if group is not None:
            grp = np.asarray(group, dtype=np.int64)
            grp_t = torch.as_tensor(np.where(grp < 0, _abi.POOL_SKIP, grp).astype(np.uint32).view(np.int32), device=b.dev)
        eng.summarize_windows(b.n, G, edges, clock_ptr=b.clock_t.data_ptr(), clock_capacity=b.cap, counts_ptr=b.counts_t.data_ptr(),
                              stats_ptr=stats.data_ptr(), group_ptr=grp_t.data_ptr() if grp_t is not None else 0, window_of=window_of)
        st = stats.cpu().numpy()
        assert np.array_equal(got["total"].astype(np.float64), st[:, :, 0])
        pair = got["clock"][:, :, 0, :].view(np.float64)
        lat = pair[..., 1] - pair[..., 0]
        some = got["kept"] == 1
        assert some.any() and (~some).any()
        assert np.array_equal(lat[some].view(np.uint64), st[:, :, 7][some].view(np.uint64))   # bit for bit


def test_event_workload_through_the_python_api(tmp_path):
    from asyncflow_amd import expand_grid
    from asyncflow_amd.runner import SimulationRunner

    payload = lb_with_events(horizon=60, scale=0.1)
    users = "rqs_input.avg_active_users.mean"
    grid = expand_grid({users: [60.0, 200.0]}, replicas=3, order_by_load=users)
    res = SimulationRunner(simulation_input=payload, **grid.runner_kwargs()).run()
    plan, n = res.plan, len(res)
    per = [res[s] for s in range(n)]
    ram = ram_columns(plan.n_series, plan.n_edges)

    def check(summ, ids, n_groups, k, edges, window_of, with_state):
        for g in range(n_groups):
            members = [s for s in range(n) if ids[s] == g]
            kw = {"samples": [per[s]._samples for s in members], "sample_period": plan.sample_period} if with_state else {}  # noqa: SLF001
            want = latency_exemplars([per[s].rqs_clock for s in members], k, edges, window_of, scenario_ids=members, **kw)
            kept = want["kept"].astype(np.int64)
            empty = np.arange(k)[None, :] >= kept[:, None]
            assert np.array_equal(summ["total"][g], want["total"].astype(np.int64)) and np.array_equal(summ["kept"][g], kept)
            assert np.array_equal(summ["scenario"][g], np.where(empty, -1, want["scenario"].astype(np.int64)))
            assert np.array_equal(summ["row"][g], np.where(empty, -1, want["row"].astype(np.int64)))
            pair = np.where(empty[..., None], np.nan, want["clock"])
            assert np.array_equal(summ["start"][g], pair[..., 0], equal_nan=True) and np.array_equal(summ["finish"][g], pair[..., 1], equal_nan=True)
            assert np.array_equal(summ["latency"][g], pair[..., 1] - pair[..., 0], equal_nan=True)
            if with_state:
                w = want["state"]
                val = w.astype(np.float64)
                val[..., ram] = w[..., ram].view(np.float32).astype(np.float64)
                assert np.array_equal(summ["state"][g], np.where(w == ONES, np.nan, val), equal_nan=True)

    a = res.exemplar_summary(8, 10.0, by=grid, with_state=True)
    assert a["scenario"].shape == (2, 6, 8) and a["state"].shape == (2, 6, 8, plan.n_series) and a["replicas"].tolist() == [3, 3]
    assert a["series_names"] == res.series_names() and a["window_of"] == "finish" and a["scenario"].dtype == np.int64
    check(a, grid.point, 2, 8, a["edges"], "finish", True)
    assert np.isfinite(a["state"]).any()
    for g, w, j in ((0, 1, 0), (1, 5, 7), (1, 0, 3)):                      # batch[s].rqs_clock[row] is the returned pair
        s, r = int(a["scenario"][g, w, j]), int(a["row"][g, w, j])
        assert s >= 0 and res[s].rqs_clock[r].tolist() == [a["start"][g, w, j], a["finish"][g, w, j]]
    arr = res.exemplar_summary(64, edges=[0.0, 9.5, 16.0, 16.5, 61.0, 90.0], by="scenario", window_of="arrival", with_state=True)
    check(arr, np.arange(n), n, 64, arr["edges"], "arrival", True)
    assert (arr["kept"][:, 4] == 0).all() and (arr["row"][:, 4] == -1).all() and np.isnan(arr["state"][:, 4]).all()
    whole = res.exemplar_summary()                                          # k = 16, the whole run, one group
    assert whole["edges"] is None and whole["row"].shape == (1, 1, 16) and "state" not in whole
    check(whole, np.zeros(n, dtype=np.int64), 1, 16, None, "finish", False)
    skip = np.where(np.arange(n) % 4 == 0, -1, grid.point)
    check(res.exemplar_summary(3, 20.0, by=skip), skip, 2, 3, np.array([0.0, 20.0, 40.0, 60.0]), "finish", False)
    one = per[2].get_slowest_requests(5, window_s=10.0)
    own = res.exemplar_summary(5, 10.0, by="scenario")
    for key in ("row", "start", "finish", "latency", "total", "kept"):
        assert np.array_equal(one[key], own[key][2], equal_nan=True), key
    with pytest.raises(ValueError, match="arrival"):
        res.exemplar_summary(4, window_of="arrival")
    with pytest.raises(ValueError, match="k must be"):
        res.exemplar_summary(65)
    for name in ("exemplars.npz", "exemplars.parquet"):                    # the dump, in both formats
        written = res.save_exemplar_summary(str(tmp_path / name), grid, k=8, window_s=10.0, window_of="arrival", with_state=True)
        back = load_summary(str(tmp_path / name))
        assert set(back) == set(written) and str(back["window_of"]) == "arrival"
        for key, v in written.items():
            if v.dtype.kind in "US":
                assert np.asarray(back[key]).tolist() == v.tolist(), (name, key)
            else:
                assert np.array_equal(np.asarray(back[key], dtype=v.dtype).reshape(v.shape), v, equal_nan=v.dtype.kind == "f"), (name, key)
        by_arr = res.exemplar_summary(8, 10.0, by=grid, window_of="arrival", with_state=True)
        assert np.array_equal(written["exemplar_row"], by_arr["row"]) and np.array_equal(written["exemplar_state"], by_arr["state"], equal_nan=True)
        assert np.array_equal(written["window_edges"], by_arr["edges"])
