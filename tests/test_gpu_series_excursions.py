"""Excursions of the sampled series above a threshold per (scenario, window of ticks, series) on the MI355X
(af_engine_summarize_series_excursions): synthetic sample blocks handed straight to the entry -- the padding words and the
rows at or past a scenario's ticks hold 0xFFFFFFFF, a word that would be above every threshold and the peak of its cell if it
were read -- with every output in one buffer between sentinels.  Every comparison is == on integers against the host
definition (results.series_window_excursions); there is no tolerance anywhere.

Constructed run patterns around the rows a wave takes per step (R = 32, 21, 5, 3, 2, 1, and a plan whose rows need a second
pass), random blocks on every window shape, work items of several windows, the identities with
af_engine_summarize_series_windows, independence of batch, position and call, NULL outputs, the scratch bound, the refusals,
and an event workload through the Python API with bands and the on-disk summary."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from asyncflow_amd import _abi
from asyncflow_amd.results import series_window_excursions, tick_window_edges
from oracle.scenarios import lb_with_events
from tests.test_gpu_series_windows import WIDE, _block, _plan, _shapes, _signed_block, _ticks, _wide_plan, _wide_shapes, ram_columns

pytestmark = pytest.mark.gpu

FILL = 0xFFFFFFFF
PATTERN = 0x5A5A5A5A
OUTS = ("count", "above", "runs", "longest", "longest_start", "first", "last", "peak_tick")
TICKS = ("longest_start", "first", "last", "peak_tick")


def _plans(name):
    return _wide_plan(name) if name in WIDE else _plan(name)


def _filled(plan, blk, counts):
    """The block with 0xFFFFFFFF in every padding word and in every row at or past a scenario's min(ticks, capacity)."""
    blk = blk.copy()
    blk[:, :, plan.n_series:] = FILL
    for s in range(blk.shape[0]):
        blk[s, min(int(counts[s, _abi.CNT_TICKS]), blk.shape[1]):] = FILL
    return blk


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

    def run(self, edges, thr=None, outputs=OUTS):
        """The requested outputs as uint32 arrays and scratch_bytes; all eight outputs have their place in one buffer between
        sentinels, and no word outside the requested ones may change."""
        W, S = len(edges) - 1, self.plan.n_series
        guard, at, off = 64, 64, {}
        for k in OUTS:
            off[k] = at
            at += self.n * W * (1 if k == "count" else S) + guard
        buf = self.torch.full((at,), PATTERN, dtype=self.torch.int32, device=self.dev)
        self.torch.cuda.synchronize(self.dev)         # (the engine has a stream of its own and this entry reads nothing back first)
        _, scratch = self.eng.summarize_series_excursions(
            self.n, edges, samples_ptr=self.blk_t.data_ptr(), tick_capacity=self.cap, counts_ptr=self.counts_t.data_ptr(),
            thresholds=thr, **{f"{k}_ptr": buf.data_ptr() + 4 * off[k] for k in outputs})
        host = buf.cpu().numpy().view(np.uint32)
        written = np.zeros(at, dtype=bool)
        out = {}
        for k in outputs:
            size = self.n * W * (1 if k == "count" else S)
            written[off[k]:off[k] + size] = True
            out[k] = host[off[k]:off[k] + size].reshape((self.n, W) if k == "count" else (self.n, W, S))
        assert (host[~written] == PATTERN).all(), f"a word outside the requested outputs {outputs} was written"
        return out, scratch

    def series_windows(self, edges, thr=None):
        """af_engine_summarize_series_windows on the same block with singleton groups: count, maxv, above."""
        torch, n, W, S = self.torch, self.n, len(edges) - 1, self.plan.n_series
        count = torch.empty((n, W), dtype=torch.int32, device=self.dev)
        mean = torch.empty((n, W, S), dtype=torch.float64, device=self.dev)
        mx, ab = (torch.empty((n, W, S), dtype=torch.int32, device=self.dev) for _ in range(2))
        grp = torch.arange(n, dtype=torch.int32, device=self.dev)
        self.eng.summarize_series_windows(n, n, edges, samples_ptr=self.blk_t.data_ptr(), tick_capacity=self.cap,
                                          counts_ptr=self.counts_t.data_ptr(), count_ptr=count.data_ptr(), mean_ptr=mean.data_ptr(),
                                          max_ptr=mx.data_ptr(), above_ptr=ab.data_ptr(), group_ptr=grp.data_ptr(), thresholds=thr)
        return {k: v.cpu().numpy().view(np.uint32) for k, v in (("count", count), ("max", mx), ("above", ab))}


def _host(plan, blk, counts, edges, thr=None):
    """results.series_window_excursions of every scenario's stored rows; int64, -1 for none."""
    n, cap, _ = blk.shape
    out = {k: [] for k in OUTS}
    for s in range(n):
        m = min(int(counts[s, _abi.CNT_TICKS]), cap)
        one = series_window_excursions(np.ascontiguousarray(blk[s, :m, :plan.n_series].T), edges, plan.n_edges, thr)
        for k in OUTS:
            out[k].append(one[k])
    return {k: np.stack(v) for k, v in out.items()}


def _as_words(want):
    """-1 is AF_TICK_NONE."""
    return {k: (v & 0xFFFFFFFF).astype(np.uint32) for k, v in want.items()}


def _equal(got, want, what):
    words = _as_words(want)
    for k in got:
        assert got[k].shape == words[k].shape, (what, k)
        assert np.array_equal(got[k], words[k]), (what, k, np.argwhere(got[k] != words[k])[:5], got[k][got[k] != words[k]][:5],
                                                  words[k][got[k] != words[k]][:5])
    for k in TICKS:
        if k in got:
            assert ((got[k] == _abi.TICK_NONE) == (want[k] == -1)).all(), (what, k)


def _check(d, blk, counts, edges, thr, what):
    got, scratch = d.run(edges, thr)
    want = _host(d.plan, blk, counts, edges, thr)
    _equal(got, want, what)
    return got, want, scratch


def _rows_per_step(plan) -> int:
    return 64 // min(plan.series_pitch // 4, 64)


# ------------------------------------------------------------------------------------ 1. constructed run patterns
ABOVE, BELOW, PEAK, THR = 100, 1, 200, 50.0
#: the rows a wave takes per step, 64 / min(pitch / 4, 64): single_server's rows are two 16-byte groups, 32 rows a step
ROWS = {"single_server": 32, "lb_two_servers": 21, "fanout8": 5, "wide_fanout16": 3, "wide_fanout20": 2, "wide_fanout50": 1,
        "wide_fanout51": 1}


def _patterned(plan, rng, R: int):
    """A block whose scenarios each hold one run pattern in two columns -- integer column 0 and the LAST ram column (of
    wide_fanout51 the one column of the second pass over the rows) --: a run of `length` ticks at `start` and, where it fits,
    a second one of the same length `gap` ticks behind it (a tie for the longest run); the first tick of the first run and
    the last tick of the last run hold the peak value (a tie for the peak), every other above tick 100, the rest 1.  Lengths
    {1, R - 1, R, R + 1, 2 R, 2 R + 1}, starts {0, 1, R - 1, R, m_s - length}, gaps {1, R}.  Integer column 1 is above
    throughout, integer column 2 never; the other columns are random.  One more scenario stored no tick, and the ticks m_s
    differ between the scenarios.  Returns the block, the counts, the thresholds and the runs of every scenario."""
    S = plan.n_series
    ram = np.nonzero(ram_columns(S, plan.n_edges))[0]
    assert not ram_columns(S, plan.n_edges)[:3].any() and len(ram) >= 1
    cap = 400 if R >= 32 else 160
    lengths = sorted({x for x in (1, R - 1, R, R + 1, 2 * R, 2 * R + 1) if x >= 1})
    cases = []
    for i, length in enumerate(lengths):
        m = cap - 5 * (i % 3)
        for start in sorted({0, 1, R - 1, R, m - length}):
            for gap in sorted({1, R}):
                cases.append((m, start, length, gap))
    n = len(cases) + 1
    assert n <= 64
    blk, counts = _block(plan, rng, n, cap, [c[0] for c in cases] + [0])
    runs = []
    for s, (m, start, length, gap) in enumerate(cases):
        mine = [(start, length)]
        if start + 2 * length + gap <= m:
            mine.append((start + length + gap, length))
        col = np.full(cap, BELOW, dtype=np.uint32)
        for a, ln in mine:
            col[a:a + ln] = ABOVE
        col[mine[0][0]] = col[mine[-1][0] + mine[-1][1] - 1] = PEAK
        blk[s, :, 0] = col
        blk[s, :, ram[-1]] = col.astype(np.float32).view(np.uint32)
        blk[s, :, 1], blk[s, :, 2] = ABOVE, BELOW
        runs.append(mine)
    runs.append([])
    thr = np.zeros(S)
    thr[[0, 1, 2, ram[-1]]] = THR
    thr[3:ram[-1]] = 2.0 ** 19                                          # (the random integer columns: half of the ticks above;
    thr[ram[:-1]] = 2.0 ** 15                                          #  the random ram columns likewise)
    return _filled(plan, blk, counts), counts, thr, runs, cap


@pytest.mark.parametrize("name", list(ROWS))
def test_constructed_run_patterns(name):
    plan = _plans(name)
    R = ROWS[name]
    assert _rows_per_step(plan) == R and (plan.series_pitch // 4 > 64) == (name == "wide_fanout51")
    S = plan.n_series
    last_ram = int(np.nonzero(ram_columns(S, plan.n_edges))[0][-1])
    assert last_ram == S - 1 and (name != "wide_fanout51" or last_ram // 4 == 64)       # the second pass holds that column
    rng = np.random.default_rng(R + S)
    blk, counts, thr, runs, cap = _patterned(plan, rng, R)
    n = blk.shape[0]
    m = np.minimum(counts[:, _abi.CNT_TICKS].astype(np.int64), cap)
    shapes = [("one window", np.array([0, cap])), (f"{R} ticks from tick 3", np.arange(3, cap + R + 1, max(R, 2))),
              ("7 ticks", tick_window_edges(7, cap)), ("uneven", _wide_shapes(cap)[-1][1])]
    # ---- the host result really contains the cases (a later edit of the generator cannot quietly lose them)
    whole = _host(plan, blk, counts, shapes[0][1], thr)
    for j in (0, last_ram):
        w = {k: v[:, 0, j] for k, v in whole.items() if k != "count"}
        assert [int(x) for x in w["runs"]] == [len(r) for r in runs] and [int(x) for x in w["above"]] == [sum(ln for _, ln in r) for r in runs]
        end = w["longest_start"] + w["longest"] - 1
        some = w["runs"] > 0
        if R > 1:
            assert (some & (w["longest_start"] // R != end // R)).any(), "no run crosses a step boundary"
        assert (some & (w["last"] == m - 1)).any(), "no run ends at m_s - 1 (open)"
        assert ((w["runs"] == 2) & (w["above"] == 2 * w["longest"])).any(), "no tie for the longest run"
        assert (w["longest_start"][w["runs"] == 2] == [r[0][0] for r in runs if len(r) == 2]).all()     # the earliest wins
        peaks = [(blk[s, :m[s], j] == blk[s, :m[s], j].max()).sum() for s in range(n) if m[s]]
        assert max(peaks) > 1 and (w["peak_tick"][:-1] == [r[0][0] for r in runs[:-1]]).all(), "no tie for the peak"
    assert (whole["above"][:-1, 0, 1] == m[:-1]).all() and (whole["runs"][:-1, 0, 1] == 1).all() and (whole["above"][:, 0, 2] == 0).all()
    assert m[-1] == 0 and (whole["count"][-1] == 0).all() and (whole["peak_tick"][-1] == -1).all()
    split = _host(plan, blk, counts, shapes[2][1], thr)
    b = np.minimum(shapes[2][1].astype(np.int64)[None, :], m[:, None])      # [n, W + 1]
    here, nxt = split["last"][:, :-1, 0], split["first"][:, 1:, 0]
    assert ((here >= 0) & (here == b[:, 1:-1] - 1) & (nxt == b[:, 1:-1])).any(), "no run crosses a window edge"
    uneven = _host(plan, blk, counts, shapes[3][1], thr)
    assert (uneven["count"][m > 0] == 0).any() and (uneven["count"][m > 0] > 0).any(), "no empty cell of a scenario with ticks"
    # ---- the device
    d = _Device(plan, blk, counts)
    try:
        for what, edges in shapes:
            _check(d, blk, counts, edges, thr, f"{name}, {what}")
        _check(d, blk, counts, shapes[1][1], None, f"{name}, thresholds NULL")
    finally:
        d.close()


# ------------------------------------------------------------------------------------ 2. random blocks
def _random_thresholds(plan, kind: str):
    """None (0.0 each); half of the ticks above; few of them above."""
    S = plan.n_series
    ram = ram_columns(S, plan.n_edges)
    mid = np.where(ram, 2.0 ** 15 if kind == "block" else 0.0, 2.0 ** 19)
    high = np.where(ram, 0.9 * 2.0 ** 16 if kind == "block" else 2.0 ** -8, 0.9 * 2.0 ** 20)
    if kind != "block":
        mid[np.nonzero(ram)[0][::2]] = -0.0
    return [None, mid, high]


@pytest.mark.parametrize(("name", "kind"), [("single_server", "block"), ("single_server", "signed0"), ("single_server", "signed1"),
                                            ("lb_two_servers", "signed0"), ("fanout8", "signed1"), ("wide_fanout16", "signed0"),
                                            ("wide_fanout20", "block"), ("wide_fanout50", "signed1"), ("deep_chain62", "signed0"),
                                            ("wide_fanout51", "signed1"), ("wide_fanout64", "signed0")])
def test_random_blocks_equal_the_host_definition(name, kind):
    plan = _plans(name)
    rng = np.random.default_rng(len(name) + len(kind) + plan.n_series)
    n, cap = (6, 150) if name in WIDE else (10, 260)
    ticks = _ticks(rng, n, cap)
    assert ticks[0] == 0 and ticks[2] > cap
    if kind == "block":
        blk, counts = _block(plan, rng, n, cap, ticks)
    else:
        blk, counts = _signed_block(plan, rng, n, cap, ticks, flip=int(kind[-1]))
    blk = _filled(plan, blk, counts)
    # the window shapes of the series-window tests: the narrow plans' where the capacity lets their edges increase, and the wide plans'
    shapes = _wide_shapes(cap)
    if name not in WIDE:
        shapes += [(w, e) for w, e in _shapes(cap) if w not in dict(shapes) and (np.diff(e.astype(np.int64)) > 0).all()]
    assert len(shapes) == (6 if name in WIDE else 8)
    d = _Device(plan, blk, counts)
    try:
        seen = np.zeros(3, dtype=np.int64)
        for what, edges in shapes:
            for i, thr in enumerate(_random_thresholds(plan, kind)):
                if what == "one tick each" and i == 2:
                    continue
                got, want, _ = _check(d, blk, counts, edges, thr, f"{name}, {kind}, {what}, thresholds {i}")
                seen += [int((want["runs"] > 1).sum()), int((want["longest"] > 1).sum()), int((want["first"] == -1).sum())]
        assert (seen > 0).all(), seen                                   # cells of several runs, runs of several ticks, cells without one
    finally:
        d.close()


# ------------------------------------------------------------------------------------ 3. work items of several windows
@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize(("n", "cap", "run", "last"), [(64, 1501, 2, 1), (300, 700, 6, 4)])
def test_work_items_of_several_windows(n, cap, run, last, flip):
    """One tick per window, the sizes of test_runs_of_several_windows_feed_the_records: the engine gives a wave
    max(1, W / ceil(32768 / n)) consecutive windows, so runs of 2 windows with a last run of 1 and runs of 6 with a last run of
    4 start and end inside a step.  A window of one tick has a closed form -- above = runs = longest = (the tick is above),
    every tick output the tick itself or NONE --, stated here for all scenarios; six of them also go through the host
    definition."""
    plan = _plan("single_server")
    S = plan.n_series
    W = cap
    assert max(1, W // -(-32768 // n)) == run and W % run == last
    rng = np.random.default_rng(n + flip)
    blk, counts = _signed_block(plan, rng, n, cap, _ticks(rng, n, cap), flip)
    blk = _filled(plan, blk, counts)
    ram = ram_columns(S, plan.n_edges)
    thr = np.where(ram, 0.0, 2.0 ** 19)
    edges = np.arange(cap + 1)
    d = _Device(plan, blk, counts)
    try:
        got, _ = d.run(edges, thr)
    finally:
        d.close()
    m = np.minimum(counts[:, _abi.CNT_TICKS].astype(np.int64), cap)
    live = np.arange(cap)[None, :] < m[:, None]                                            # [n, W]
    with np.errstate(invalid="ignore"):
        values = np.where(ram, blk[:, :, :S].view(np.float32).astype(np.float64), blk[:, :, :S].astype(np.float64))
    above = live[:, :, None] & (values > thr)
    tick = np.broadcast_to(np.arange(cap, dtype=np.int64)[None, :, None], above.shape)
    want = {"count": live.astype(np.int64), "above": above.astype(np.int64), "runs": above.astype(np.int64),
            "longest": above.astype(np.int64), "longest_start": np.where(above, tick, -1), "first": np.where(above, tick, -1),
            "last": np.where(above, tick, -1), "peak_tick": np.where(live[:, :, None], tick, -1)}
    _equal(got, want, f"n = {n}, {W} windows of one tick")
    some = [0, 1, 2, 3, n // 2, n - 1]
    part = _host(plan, blk[some], counts[some], edges, thr)
    _equal({k: v[some] for k, v in got.items()}, part, "the host definition")


# ------------------------------------------------------------------------------------ 4. against the series-window analyzer
@pytest.mark.parametrize("name", ["lb_two_servers", "wide_fanout51"])
def test_above_count_and_peak_agree_with_the_series_window_analyzer(name):
    plan = _plans(name)
    S = plan.n_series
    rng = np.random.default_rng(41 + S)
    n, cap = 9, 150
    blk, counts = _signed_block(plan, rng, n, cap, _ticks(rng, n, cap))
    blk = _filled(plan, blk, counts)
    thr = _random_thresholds(plan, "signed")[1]
    d = _Device(plan, blk, counts)
    try:
        for what, edges in _wide_shapes(cap):
            got, _ = d.run(edges, thr)
            win = d.series_windows(edges, thr)
            assert got["above"].tobytes() == win["above"].tobytes() and got["count"].tobytes() == win["count"].tobytes(), what
            full = got["count"] > 0
            assert ((got["peak_tick"] == _abi.TICK_NONE) == ~full[:, :, None]).all(), what
            s, w, j = np.nonzero(np.broadcast_to(full[:, :, None], got["peak_tick"].shape))
            assert s.size and np.array_equal(blk[s, got["peak_tick"][s, w, j], j], win["max"][s, w, j]), what   # (equal words: equal keys)
    finally:
        d.close()


# ------------------------------------------------------------------------------------ 5. independence
def test_cells_do_not_depend_on_batch_position_or_call():
    plan = _plan("lb_two_servers")
    rng = np.random.default_rng(5)
    n, cap = 8, 256
    blk, counts = _block(plan, rng, n, cap, _ticks(rng, n, cap))
    blk = _filled(plan, blk, counts)
    thr = _random_thresholds(plan, "block")[1]
    big, big_counts = _block(plan, rng, 8 * n, cap, rng.integers(0, cap + 1, 8 * n))
    where = np.arange(n) * 8 + 3
    big[where], big_counts[where] = blk, counts
    big = _filled(plan, big, big_counts)
    d, d_big = _Device(plan, blk, counts), _Device(plan, big, big_counts)
    singles = [_Device(plan, blk[s:s + 1], counts[s:s + 1]) for s in range(n)]
    try:
        for edges in (tick_window_edges(100, cap), tick_window_edges(7, cap), np.array([0, cap])):
            alone, _ = d.run(edges, thr)
            again, _ = d.run(edges, thr)
            inside, _ = d_big.run(edges, thr)
            for k in OUTS:
                assert alone[k].tobytes() == again[k].tobytes(), k                                     # the same call twice
                assert alone[k].tobytes() == np.ascontiguousarray(inside[k][where]).tobytes(), k      # elsewhere in a larger batch
            for s, one in enumerate(singles):                                                          # alone in a batch
                mine, _ = one.run(edges, thr)
                for k in OUTS:
                    assert mine[k][0].tobytes() == alone[k][s].tobytes(), (k, s)
    finally:
        for x in (d, d_big, *singles):
            x.close()


# ------------------------------------------------------------------------------------ 6. NULL outputs, scratch
def test_null_outputs_are_skipped():
    plan = _plan("single_server")
    rng = np.random.default_rng(2)
    n, cap = 9, 300
    blk, counts = _block(plan, rng, n, cap, _ticks(rng, n, cap))
    blk = _filled(plan, blk, counts)
    thr = _random_thresholds(plan, "block")[1]
    edges = tick_window_edges(64, cap)
    d = _Device(plan, blk, counts)
    try:
        full, _ = d.run(edges, thr)
        for outputs in ((), ("count",), ("longest",), ("runs", "last"), ("above", "first", "peak_tick"), ("longest_start",), OUTS[1:]):
            got, _ = d.run(edges, thr, outputs=outputs)                 # (asserts that the guard words and the skipped outputs stay)
            assert set(got) == set(outputs)
            for k in got:
                assert got[k].tobytes() == full[k].tobytes(), (outputs, k)
    finally:
        d.close()


def test_scratch_stays_within_the_bound_of_the_header():
    """include/asyncflow_hip.h: 4 B per edge + 8 B per series + 512 B of alignment -- no per-cell records."""
    plan = _plan("fanout8")
    rng = np.random.default_rng(3)
    n, cap = 40, 400
    blk, counts = _block(plan, rng, n, cap, rng.integers(0, cap + 1, n))
    for edges in (tick_window_edges(20, cap), np.arange(cap + 1)):
        d = _Device(plan, _filled(plan, blk, counts), counts)           # (a fresh engine: the scratch of this call alone)
        try:
            _, scratch = d.run(edges)
        finally:
            d.close()
        bound = 4 * len(edges) + 8 * plan.n_series + 512
        print(f"{len(edges) - 1} windows: scratch_bytes {scratch}, bound {bound}")
        assert 0 < scratch <= bound < 4 * n * (len(edges) - 1) * plan.n_series


# ------------------------------------------------------------------------------------ 7. refusals
def test_device_argument_checks():
    """Error codes from calls that return before any kernel is launched; no output word is touched."""
    import torch

    from asyncflow_amd.engine import PLAN_ONLY, Engine, load_library

    plan = _plan("lb_two_servers")
    rng = np.random.default_rng(1)
    blk, counts = _block(plan, rng, 3, 50, [50, 20, 0])
    lib = load_library()
    dev = torch.device("cuda", 0)
    blk_t = torch.as_tensor(blk.view(np.int32), device=dev)
    counts_t = torch.as_tensor(counts.view(np.int32), device=dev)
    outs = torch.full((8 * 1024,), PATTERN, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    eng, planner = Engine(plan, 0), Engine(plan, PLAN_ONLY)
    try:
        def call(edges, thr=None, samples=True, counts_ok=True, n_windows=None, cap=50, engine=eng, n=3):
            e = (C.c_uint32 * len(edges))(*edges)
            t = (C.c_double * len(thr))(*thr) if thr is not None else None
            out = _abi.AfOutputs(0, None, cap, C.c_void_p(blk_t.data_ptr() if samples else None),
                                 C.c_void_p(counts_t.data_ptr() if counts_ok else None))
            req = _abi.AfSeriesExcursions(n, len(edges) - 1 if n_windows is None else n_windows, e, t,
                                          *(C.c_void_p(outs.data_ptr() + 4096 * i) for i in range(8)), 0.0, 0)
            rc = lib.af_engine_summarize_series_excursions(engine._h, C.byref(out), C.byref(req))  # noqa: SLF001
            return rc, lib.af_last_error().decode()

        refused = [
            (call([0], n_windows=0), _abi.AF_ERR_INVALID, "n_windows"),
            (call([0, 10], n=0), _abi.AF_ERR_INVALID, "n_scenarios"),
            (call([0, 10, 10]), _abi.AF_ERR_INVALID, "strictly increasing"),
            (call([10, 5]), _abi.AF_ERR_INVALID, "strictly increasing"),
            (call([0, 10], thr=[0.0] * 5 + [float("nan")] + [0.0] * 6), _abi.AF_ERR_INVALID, "NaN"),
            (call([0, 10], samples=False), _abi.AF_ERR_INVALID, "samples"),
            (call([0, 10], counts_ok=False), _abi.AF_ERR_INVALID, "counts"),
            (call([0, 10], cap=0), _abi.AF_ERR_INVALID, "tick_capacity above 0"),
            (call([0, 10], cap=0x80000000), _abi.AF_ERR_CAPACITY, "2^31"),
            (call([0, 10], engine=planner), _abi.AF_ERR_NO_DEVICE, "planning-only"),
        ]
        for (rc, msg), code, reason in refused:
            assert rc == code and reason in msg, (rc, msg, code, reason)
        torch.cuda.synchronize(dev)
        assert (outs.cpu().numpy().view(np.uint32) == PATTERN).all(), "a refused call touched an output"
        assert call([0, 10])[0] == _abi.AF_OK
        host = outs.cpu().numpy().view(np.uint32)
        assert host[:3].tolist() == [10, 10, 0] and host[3] == PATTERN
    finally:
        eng.close()
        planner.close()


# ------------------------------------------------------------------------------------ 8. through the Python API
def _event_run():
    from asyncflow_amd.runner import SimulationRunner

    payload = lb_with_events(horizon=60, scale=0.1)                     # srv-1 is down from 18 s to 24 s (the last event ends at 54 s)
    seeds = 0xE7C50000 + np.arange(16, dtype=np.uint64)
    res = SimulationRunner(simulation_input=payload, seeds=seeds).run()
    names = res.series_names()
    queue = "srv-2:ready_queue_len"
    assert queue in names
    first = int(round(18.0 / res.plan.sample_period))                   # the outage's first tick
    edges = np.array([first, first + int(round(6.0 / res.plan.sample_period)), res.plan.tick_count, res.plan.tick_count + 40])
    thr = {queue: 0.5, next(k for k in names if k.endswith("ram_in_use")): 64.0}
    return res, names, queue, edges, thr, np.arange(16) % 2


def test_event_workload_through_the_python_api():
    res, names, queue, edges, thr, ids = _event_run()
    thr_vec = res._series_thresholds(thr)  # noqa: SLF001
    period = res.plan.sample_period
    a = res.series_excursion_summary(thr, tick_edges=edges)
    assert a["series"] == names and np.array_equal(a["tick_edges"], edges) and np.array_equal(a["thresholds"], thr_vec)
    assert np.array_equal(a["times"], edges[:-1] * period) and tuple(a["above"].shape) == (16, 3, len(names))
    per = [res[s].get_series_excursions(thr_vec, tick_edges=edges) for s in range(16)]
    got = {k: a[k].cpu().numpy() for k in (*OUTS, "above_s", "longest_s", "first_s", "peak_s", "recovered_s", "open", "exceeded")}
    for k in OUTS:
        assert got[k].dtype == np.int64 and np.array_equal(got[k], np.stack([p[k] for p in per])), k
    j = names.index(queue)
    print("longest run of srv-2's ready queue above 0.5 in the outage window, ticks per replica:", got["longest"][:, 0, j].tolist())
    assert (got["longest"][:, 0, j] > 0).any()
    # the derived tensors, stated from the integers
    hi = np.minimum(edges[1:].astype(np.int64)[None, :], np.minimum(res.counts[:, _abi.CNT_TICKS].astype(np.int64), res.plan.tick_count)[:, None])
    exceeded = got["first"] >= 0
    still = exceeded & (got["last"] == hi[:, :, None] - 1)
    assert np.array_equal(got["exceeded"], exceeded) and np.array_equal(got["open"], still) and still.any() and (exceeded & ~still).any()
    assert np.array_equal(got["above_s"], got["above"] * period) and np.array_equal(got["longest_s"], got["longest"] * period)
    assert np.array_equal(got["first_s"], np.where(exceeded, got["first"] * period, np.nan), equal_nan=True)
    assert np.array_equal(got["peak_s"], np.where(got["peak_tick"] >= 0, got["peak_tick"] * period, np.nan), equal_nan=True)
    assert np.array_equal(got["recovered_s"], np.where(exceeded & ~still, (got["last"] + 1) * period, np.nan), equal_nan=True)
    assert (got["count"][:, 2] == 0).all() and np.isnan(got["peak_s"][:, 2]).all() and not exceeded[:, 2].any()
    # the default: ONE window over the whole run
    whole = res.series_excursion_summary(thr)
    assert whole["tick_edges"].tolist() == [0, res.plan.tick_count] and tuple(whole["count"].shape) == (16, 1)
    assert np.array_equal(whole["runs"].cpu().numpy()[:, 0], np.stack([res[s].get_series_excursions(thr_vec)["runs"][0] for s in range(16)]))
    by_seconds = res.series_excursion_summary(thr, 6.0)
    assert np.array_equal(by_seconds["tick_edges"], tick_window_edges(int(round(6.0 / period)), res.plan.tick_count))

    # ---- bands over the replicas of the two groups, from the per-scenario values with the stated valid masks
    for of, valid in (("recovered_s", exceeded & ~still), ("first_s", exceeded), ("longest_s", None), ("runs", None)):
        bands = res.series_excursion_bands(thr, tick_edges=edges, by=ids, of=of, level=0.9, q=(0.1, 0.75))
        values = got[of].astype(np.float64)
        ok = np.broadcast_to((got["count"] > 0)[:, :, None], values.shape) if valid is None else valid
        assert bands["of"] == of and bands["mean"].shape == (2, 3, len(names)) and bands["replicas"].tolist() == [8, 8]
        for g in range(2):
            members = np.nonzero(ids == g)[0]
            for w in range(3):
                for c in range(len(names)):
                    body = values[members, w, c][ok[members, w, c]]
                    assert bands["n"][g, w, c] == body.shape[0], (of, g, w, c)
                    if body.shape[0] == 0:
                        assert all(np.isnan(bands[k][g, w, c]) for k in ("mean", "std", "ci_halfwidth", "q_lo", "q_hi"))
                        continue
                    np.testing.assert_allclose(bands["mean"][g, w, c], body.mean(), rtol=1e-12, atol=0.0)
                    np.testing.assert_allclose(bands["q_lo"][g, w, c], np.quantile(body, 0.1), rtol=1e-12, atol=0.0)
                    np.testing.assert_allclose(bands["q_hi"][g, w, c], np.quantile(body, 0.75), rtol=1e-12, atol=0.0)
                    if body.shape[0] > 1:
                        np.testing.assert_allclose(bands["std"][g, w, c], body.std(ddof=1), rtol=1e-9, atol=1e-12)
                # the shares: integer counts of members, divided once
                base = int((got["count"][members, w] > 0).sum())
                for name, mask in (("exceed_share", exceeded), ("open_share", still)):
                    want = mask[members, w].sum(axis=0) / base if base else np.full(len(names), np.nan)
                    assert np.array_equal(bands[name][g, w], want, equal_nan=True), (name, g, w)
        assert np.isnan(bands["exceed_share"][:, 2]).all() and (bands["n"][:, 2] == 0).all()
    with pytest.raises(ValueError, match="of must be one of"):
        res.series_excursion_bands(thr, of="last")
    with pytest.raises(ValueError, match="unknown series"):
        res.series_excursion_summary({"srv-9:ready_queue_len": 1.0})


def _round_trip(path: str) -> None:
    from asyncflow_amd.results import load_summary

    res, names, _, edges, thr, ids = _event_run()
    longest = res.series_excursion_bands(thr, tick_edges=edges, by=ids, of="longest_s")
    back_s = res.series_excursion_bands(thr, tick_edges=edges, by=ids, of="recovered_s")
    written = res.save_series_excursion_summary(path, ids, thresholds=thr, tick_edges=edges)
    back = load_summary(path)
    assert set(back) == set(written)
    for k, v in written.items():
        assert np.array_equal(np.asarray(back[k], dtype=v.dtype), v, equal_nan=v.dtype.kind == "f"), k
    for j, sname in enumerate(names):
        for col, want in (("longest_s", longest["mean"]), ("q05", longest["q_lo"]), ("q95", longest["q_hi"]), ("recovered_s", back_s["mean"]),
                          ("exceed_share", longest["exceed_share"]), ("open_share", longest["open_share"])):
            if col in ("longest_s", "recovered_s"):                      # (means: the device adds the replicas in no fixed order)
                np.testing.assert_allclose(back[f"series_excursion_{col}:{sname}"], want[:, :, j], rtol=1e-12, atol=0.0, equal_nan=True)
            else:
                assert np.array_equal(back[f"series_excursion_{col}:{sname}"], want[:, :, j], equal_nan=True), (col, sname)
        assert back[f"series_excursion_q95:{sname}"].shape == (2, 3)
    assert np.array_equal(back["series_excursion_tick_edges"], edges) and back["replicas"].tolist() == [8, 8]
    assert np.array_equal(back["series_excursion_times"], edges[:-1] * res.plan.sample_period)
    assert np.array_equal(back["series_excursion_thresholds"], res._series_thresholds(thr))  # noqa: SLF001


def test_save_series_excursion_summary_npz(tmp_path):
    _round_trip(str(tmp_path / "series_excursions.npz"))


def test_save_series_excursion_summary_parquet(tmp_path):
    pytest.importorskip("pyarrow")
    _round_trip(str(tmp_path / "series_excursions.parquet"))
