"""Every analyzer entry point, the run and the results object at STRIDES PAST 2^32 ("Strides past 2^32").

The other GPU tests of the analyzers run on buffers whose every byte, word and row offset fits in 32 bits; the batches the project
is used on do not.  A product ``s * clock_cap`` or ``s * tick_cap * pitch`` that wraps lands inside the same allocation on another
scenario's valid rows: wrong numbers, no fault.  This module runs the probe table of tests/test_gpu_scratch_history.py -- the same
24 scenarios, the same host definitions -- on device buffers re-strided so that those offsets pass 2^31 and 2^32:

* ``clock`` [24, CAP, 2] f64 and ``samples`` [24, TCAP, pitch] words hold the compact rows in ``[:, :cap]`` / ``[:, :tick_cap]``
  and PLAUSIBLE values everywhere else -- the clock row (0.25, 0.75), the sample word 7 --, so that a kernel that reads from a
  wrapped offset counts something (a NaN row is dropped by several analyzers and would hide the read);
* the arrival rows are strided by DCAP; behind a scenario's last arrival they hold +inf up to the capacity: the padding rule of
  af_pregen.hpp (``o[i] = AF_INF`` for ``k_final <= i < n_draw``) and of ``results.arrival_times`` ("ascending with +inf behind
  the last arrival"), which the analyzers that search the rows rely on;
* one wide arena at a time: ``clock`` (with the wide arrival rows of the pairs), ``draws``, ``samples``, ``both``; then the
  conditional tiers, which skip with the numbers when the memory is not free.

Every output is compared with the host definition (computed with the COMPACT capacities) and with the compact batch's own fresh
result, word for word, between sentinel words."""

from __future__ import annotations

import gc
from typing import Any

import numpy as np
import pytest

from asyncflow_amd import _abi
from asyncflow_amd import results as R
from tests import test_gpu_scratch_history as H
from tests.test_gpu_scratch_history import GUARD, NAMES, SENTINEL, Batch, Probe, build_probes, equals_host, same_words

pytestmark = pytest.mark.gpu

N, S_MAX = 24, 23
CAP = (1 << 26) + 29                      # clock rows per scenario, always
TCAP = 20_000_003                         # sample rows per scenario, always
DCAP = -(-(1 << 31) // S_MAX) | 1         # arrival rows per scenario: the smallest odd value with 23 * DCAP >= 2^31 doubles
WIDEST = 187_000_003                      # clock rows and per-tick output words per scenario, where the memory is free
FILL_ROW, FILL_WORD = (0.25, 0.75), 7
GIB = 1 << 30
MARGIN = 8 * GIB

CLOCK_ONLY = [n for n in NAMES if n.split("-")[0] in ("pooled", "windows", "quantiles", "arrival_windows", "arrival_quantiles", "inflight",
                                                       "latency_histogram", "alerts", "pairs")]
SAMPLES_ONLY = [n for n in NAMES if n.startswith("series_")]
BOTH = [n for n in NAMES if n.split("-")[0] in ("state_windows", "state_quantiles", "exemplars", "summarize", "run_summarized")]
NEITHER = [n for n in NAMES if n.split("-")[0] == "arrivals"]
# their per-tick outputs [n, tick_cap] take the batch's tick capacity: at TCAP they are 1.9 GB each and stay on the device (run_on)
PER_TICK = ["inflight", "alerts"]
assert set(PER_TICK) <= set(CLOCK_ONLY)
assert sorted(CLOCK_ONLY + SAMPLES_ONLY + BOTH + NEITHER) == sorted(NAMES)
# (in this order: one wide arena at a time, the wide clock released before the wide samples are built)
PLACED = [("clock", k) for k in CLOCK_ONLY + BOTH] + [("draws", k) for k in NEITHER] + [("samples", k) for k in SAMPLES_ONLY + BOTH + PER_TICK] + \
    [("both", k) for k in BOTH + PER_TICK]
WIDEST_CLOCK = CLOCK_ONLY + BOTH


def first_s(stride: int, limit: int) -> int:
    """The first scenario whose offset ``s * stride`` is at or past ``limit``."""
    return -(-limit // stride)


# ---- the wide batch ----------------------------------------------------------------------------------------------------------------
_STATE: dict[str, Any] = {"where": None, "clock": None, "samples": None, "rows": [], "wide": {}, "probes": {}, "low_free": None}


def compact() -> Batch:
    b = H.batch()
    if "peak_from" not in _STATE:                                 # the peak of THIS module: the process may have run others before
        for name in NAMES:                                        # what the compact batch keeps for good is allocated before any arena:
            H.fresh(name)                                         # in the rounded-up tail of an arena's segment it would keep all of it reserved
        b.torch.cuda.synchronize(b.dev)
        b.torch.cuda.empty_cache()
        b.torch.cuda.reset_peak_memory_stats(b.dev)
        _STATE["peak_from"] = int(b.torch.cuda.memory_allocated(b.dev))
        _STATE["free_at_start"] = int(b.torch.cuda.mem_get_info(b.dev)[0])
    return b


def torch_of():
    return compact().torch


def free_memory() -> tuple[int, int]:
    t = torch_of()
    t.cuda.empty_cache()
    free, total = t.cuda.mem_get_info(compact().dev)
    _STATE["low_free"] = free if _STATE["low_free"] is None else min(_STATE["low_free"], free)
    return int(free), int(total)


def claim(need: int, what: str, always: bool) -> None:
    """An always-run tier FAILS without its memory; a conditional one skips.  Both say the numbers."""
    free, total = free_memory()
    if free < need + MARGIN:
        msg = f"{what} needs {need / GIB:.1f} GiB and {MARGIN // GIB} GiB beside it; {free / GIB:.1f} GiB of {total / GIB:.1f} GiB are free"
        if always:
            pytest.fail(msg)
        pytest.skip(msg)


def fill_clock(t: Any) -> None:
    t[..., 0] = FILL_ROW[0]
    t[..., 1] = FILL_ROW[1]


def wide_clock(cap: int, always: bool = True) -> Any:
    b, t = compact(), torch_of()
    claim(N * cap * 16, f"the clock rows [24, {cap}, 2]", always)
    x = t.empty((N, cap, 2), dtype=t.float64, device=b.dev)
    fill_clock(x)
    x[:, :b.cap] = b.clock_t
    return x


def wide_samples() -> Any:
    b, t = compact(), torch_of()
    claim(N * TCAP * b.plan.series_pitch * 4, f"the sample rows [24, {TCAP}, {b.plan.series_pitch}]", True)
    x = t.full((N, TCAP, b.plan.series_pitch), FILL_WORD, dtype=t.int32, device=b.dev)
    x[:, :b.tick_cap] = b.samples_t
    return x


class LazyRows:
    """The pairs' time rows at the stride DCAP, built when the pairs are called and dropped with the arena.  Behind a row's arrivals
    lies +inf, not a plausible time: the analyzer searches a row as ascending with +inf behind the last arrival (the padding rule),
    and a finite fill would break the input's contract.  The price: a wrapped row base shows only where it lands on the FINITE front
    of another row or in its +inf -- there no request finds its arrival, and the pair's counts differ from the host's wherever the
    pair has a match; a base that lands on the same values by accident is what the odd capacity is chosen against."""

    def __init__(self, host: np.ndarray) -> None:
        self.host, self.t = host, None

    def data_ptr(self) -> int:
        if self.t is None:
            b, t = compact(), torch_of()
            claim(self.host.shape[0] * DCAP * 8, f"the arrival rows [{self.host.shape[0]}, {DCAP}]", True)
            self.t = t.full((self.host.shape[0], DCAP), float("inf"), dtype=t.float64, device=b.dev)   # (the padding rule: +inf behind the last)
            self.t[:, :self.host.shape[1]] = t.as_tensor(self.host, device=b.dev)
            _STATE["rows"].append(self)
        return self.t.data_ptr()


class Wide(Batch):
    """The compact batch with other device buffers: everything on the host, the groupings and the edges are the compact batch's."""

    def __init__(self, b: Batch, clock: Any = None, samples: Any = None, wide_draws: bool = False) -> None:
        self.__dict__.update({k: v for k, v in b.__dict__.items() if k != "run_out"})
        self.wide_clock, self.wide_samples, self.wide_draws = clock is not None, samples is not None, wide_draws
        self.compact_cap = b.cap
        if clock is not None:
            self.clock_t, self.cap = clock, int(clock.shape[1])
        if samples is not None:
            self.samples_t, self.tick_cap = samples, int(samples.shape[1])
        assert np.array_equal(self.tick_edges, b.tick_edges) and int(self.tick_edges[-1]) == b.tick_cap + 9   # (just past every t_s)

    def draw_capacity(self, gen_cap: int) -> int:
        return DCAP if self.wide_draws else gen_cap

    @property
    def run_draw_capacity(self) -> int:
        return self.compact_cap

    def time_rows(self, ia: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
        if not self.wide_draws:
            return super().time_rows(ia)
        # a row per scenario in REVERSE order: the pairs of scenario 0 read row 23, past 2^31 doubles and 2^32 bytes
        time_row = (self.n - 1 - np.asarray(ia)).astype(np.int64)
        assert int(time_row.max()) * DCAP >= 1 << 31 and int(time_row.max()) * DCAP * 8 >= 1 << 32
        return np.arange(self.n)[::-1].copy(), time_row

    def arrival_rows(self, host: np.ndarray) -> Any:
        return LazyRows(host) if self.wide_draws else super().arrival_rows(host)

    def run_buffers(self) -> tuple[Any, Any]:
        """The run of run_summarized writes into the wide arena itself (the very rows it holds); a compact side gets rows of its own."""
        if "run_out" not in self.__dict__:
            t = self.torch
            self.run_out = (self.clock_t if self.wide_clock else t.empty_like(self.clock_t), self.samples_t if self.wide_samples else t.zeros_like(self.samples_t))
        return self.run_out


def release(*keys: str) -> None:
    t = torch_of()
    for k in keys:
        _STATE[k] = None
    for rows in _STATE["rows"]:
        rows.t = None
    _STATE["rows"] = []
    _STATE["wide"].clear()
    _STATE["probes"].clear()
    gc.collect()
    t.cuda.synchronize(compact().dev)
    t.cuda.empty_cache()


def release_all() -> None:
    """No placement and no arena: for the tests that bring buffers of their own."""
    _STATE["where"] = None
    release("clock", "samples", "widest")


def placed(where: str) -> tuple[Wide, dict[str, Probe]]:
    """The wide batch of a placement and its probes; the arenas of another placement are released first."""
    if _STATE["where"] != where:
        _STATE["where"] = None
        release(*[k for k, keep in (("clock", where in ("clock", "both")), ("samples", where in ("samples", "both"))) if not keep], "widest")
        if where in ("clock", "both") and _STATE["clock"] is None:
            _STATE["clock"] = wide_clock(CAP)
        if where in ("samples", "both") and _STATE["samples"] is None:
            _STATE["samples"] = wide_samples()
        if where == "widest":
            _STATE["widest"] = wide_clock(WIDEST, always=False)
        _STATE["where"] = where
    if where not in _STATE["wide"]:
        b = compact()
        clock = _STATE["widest"] if where == "widest" else _STATE["clock"] if where in ("clock", "both") else None
        _STATE["wide"][where] = wb = Wide(b, clock, _STATE["samples"] if where in ("samples", "both") else None, wide_draws=where in ("clock", "draws"))
        _STATE["probes"][where] = {p.name: p for p in build_probes(wb)}
    return _STATE["wide"][where], _STATE["probes"][where]


def arena_intact(wb: Wide) -> None:
    """The prefix of a wide arena holds the compact rows bit for bit, everything behind it the fill: on the device."""
    b, t = compact(), torch_of()
    if wb.wide_clock:
        x = wb.clock_t
        assert t.equal(x[:, :b.cap].view(t.int64), b.clock_t.view(t.int64)), "the compact clock rows in the wide arena changed"
        assert bool(((x[:, b.cap:, 0] == FILL_ROW[0]) & (x[:, b.cap:, 1] == FILL_ROW[1])).all()), "a clock row behind the compact capacity changed"
    if wb.wide_samples:
        x = wb.samples_t
        assert t.equal(x[:, :b.tick_cap], b.samples_t), "the compact sample rows in the wide arena changed"
        assert bool((x[:, b.tick_cap:] == FILL_WORD).all()), "a sample word behind the compact capacity changed"


def run_on(b: Batch, eng: Any, p: Probe, ref: Probe) -> dict[str, np.ndarray]:
    """tests.test_gpu_scratch_history.run on the batch `b`: one call with every output between sentinel words, the outputs as uint32
    words IN THE COMPACT SHAPES of `ref`.  A per-tick output [n, wide tick_cap] stays on the device: its columns [:, :tick_cap] come
    back, every other word must still hold the sentinel."""
    t = b.torch
    off, total = p.layout()
    buf = t.full((total,), SENTINEL, dtype=t.int32, device=b.dev)
    ptrs = {k: buf.data_ptr() + 4 * o for k, (o, _) in off.items()}
    t.cuda.synchronize(b.dev)
    p.call(eng, ptrs)
    t.cuda.synchronize(b.dev)
    out, at = {}, 0
    for (k, _, shape), (k_ref, _, small) in zip(p.outs, ref.outs):
        o, size = off[k]
        assert k == k_ref and o - at >= GUARD
        assert bool((buf[at:o] == SENTINEL).all()), f"{p.name}: a word in front of {k} changed"
        at = o + size
        if tuple(shape) == tuple(small):
            out[k] = buf[o:o + size].cpu().numpy().view(np.uint32).copy()
            continue
        assert len(shape) == 2 and shape[0] == small[0] and shape[1] > small[1], (k, shape, small)
        x = buf[o:o + size].view(shape)
        assert bool((x[:, small[1]:] == SENTINEL).all()), f"{p.name}: {k} was written at or past tick {small[1]}"
        out[k] = x[:, :small[1]].contiguous().cpu().numpy().view(np.uint32).reshape(-1).copy()
    assert total - at >= GUARD and bool((buf[at:] == SENTINEL).all()), f"{p.name}: a word behind the last output changed"
    free_memory()
    return out


def check(where: str, name: str) -> None:
    wb, table = placed(where)
    ref, small = H.probes()[name], H.fresh(name)[0]
    if name in PER_TICK:                                          # three outputs per tick each, at the batch's tick capacity
        assert sum(shape[-1] == wb.tick_cap for _, _, shape in table[name].outs) == 3 and wb.tick_cap == (TCAP if where in ("samples", "both") else compact().tick_cap)
    eng = wb.engine()
    try:
        got = run_on(wb, eng, table[name], ref)
    finally:
        eng.close()
    equals_host(f"{name}, wide {where}", ref, got)
    same_words(got, small, f"{name}: wide {where} and the compact batch")
    if name == "run_summarized":
        arena_intact(wb)                                          # (the one probe that writes the arena: the same rows again)
        free_memory()


# ---- 1. the capacities ---------------------------------------------------------------------------------------------------------------
def test_the_capacities_pass_2_31_and_2_32():
    b = compact()
    pitch = b.plan.series_pitch
    assert b.n == N and pitch == 12
    for c in (CAP, TCAP, DCAP, WIDEST):
        assert c % 2 == 1 and c & (c - 1) and c < 1 << 31        # odd, no power of two, under every entry point's capacity rule
    assert b.cap < CAP and b.tick_cap < TCAP and b.res._arrival_sweep()[2] < DCAP  # noqa: SLF001
    # wide clock: the byte offset s * CAP * 16 passes 2^32 from s = 4, the double index s * CAP * 2 passes 2^31 from s = 16
    assert first_s(CAP * 16, 1 << 32) == 4 and first_s(CAP * 2, 1 << 31) == 16
    # wide samples: the word index s * TCAP * pitch passes 2^31 from s = 9 and 2^32 from s = 18
    assert first_s(TCAP * pitch, 1 << 31) == 9 and first_s(TCAP * pitch, 1 << 32) == 18
    # wide draws: the double index passes 2^31 at s = 23 for this and for no smaller odd capacity; the byte offset passes 2^32 from s = 6
    assert S_MAX * DCAP >= 1 << 31 > S_MAX * (DCAP - 2) and first_s(DCAP * 8, 1 << 32) == 6 <= S_MAX
    # widest: the ROW index s * WIDEST passes 2^32 at s = 23, the double index from s = 12; a per-tick row 23 starts past word 2^32
    assert first_s(WIDEST, 1 << 32) == S_MAX and first_s(WIDEST * 2, 1 << 32) == 12
    # the always-run arenas together stay under the module's bound
    assert N * CAP * 16 + N * TCAP * pitch * 4 < 48 * GIB


# ---- 2. every probe -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(("where", "name"), PLACED, ids=[f"{w}-{k}" for w, k in PLACED])
def test_wide_strides_equal_the_host_definition(where, name):
    check(where, name)


def test_wide_arrival_rows_hold_the_host_rows_and_the_padding():
    """The arrival rows themselves at the stride DCAP: the compact host row in front, and behind it +inf up to the capacity -- the
    padding rule of af_pregen.hpp and results.arrival_times, over the whole wider row."""
    wb, _ = placed("draws")
    b, t = compact(), torch_of()
    seeds, cols, gen_cap = b.res._arrival_sweep()  # noqa: SLF001
    host = H._host_arrivals(b, gen_cap)  # noqa: SLF001
    assert not any(f for _, f in host), "a compact row is full: the wider row would hold more arrivals"
    claim(N * DCAP * 8, f"the arrival rows [24, {DCAP}]", True)
    rows = t.full((N, DCAP), 0.25, dtype=t.float64, device=b.dev)
    out = t.zeros((3, H.N_WIN), dtype=t.int64, device=b.dev)
    eng = wb.engine()
    try:
        t.cuda.synchronize(b.dev)
        eng.summarize_arrivals(seeds, cols, 3, b.edges, draw_capacity=DCAP, arrivals_ptr=out.data_ptr(), group_ptr=b.group_ptr(b.three), times_ptr=rows.data_ptr())
        t.cuda.synchronize(b.dev)
    finally:
        eng.close()
    front = rows[:, :gen_cap].contiguous().cpu().numpy()
    assert np.array_equal(front.view(np.uint64), np.stack([r for r, _ in host]).view(np.uint64))
    assert bool((rows[:, gen_cap:] == float("inf")).all())
    assert np.array_equal(out.cpu().numpy().view(np.uint64), H.probes()["arrivals"].host()["arrivals"])
    free_memory()


# ---- 4. the run ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernels", ["stage_parallel", "next_event"])
def test_the_run_at_wide_strides(kernels):
    """af_engine_run into freshly filled wide buffers.  Neither kernel family documents a write behind a scenario's rows -- the
    stage-parallel kernel stores clock row `at < clock_cap` of a completion and flushes the tick rows below min(n_ticks, tick_cap),
    the next-event kernels store row n_comp < clock_cap and row n_ticks < tick_cap (af_flow.hpp, af_core.hpp) --: NOTHING is
    excluded, every row from `completed` / `ticks` on must still hold the fill."""
    wb, _ = placed("both")
    b, t = compact(), torch_of()
    clock, samples = wb.clock_t, wb.samples_t
    fill_clock(clock)
    samples.fill_(FILL_WORD)
    counts, small_counts = t.zeros_like(b.counts_t), t.zeros_like(b.counts_t)
    small_clock, small_samples = t.empty_like(b.clock_t), t.zeros_like(b.samples_t)
    eng = b.Engine(b.plan, b.dev.index or 0, **{**b.engine_kw, "flow": kernels == "stage_parallel"})
    try:
        t.cuda.synchronize(b.dev)
        # the compact run of the same engine: all eight counts (the high-water mark of live requests is the kernel family's own)
        eng.run(b.res.seeds, b.run_cols, clock_ptr=small_clock.data_ptr(), clock_capacity=b.cap, samples_ptr=small_samples.data_ptr(),
                tick_capacity=b.tick_cap, counts_ptr=small_counts.data_ptr(), draw_capacity=b.cap)
        st = eng.run(b.res.seeds, b.run_cols, clock_ptr=clock.data_ptr(), clock_capacity=CAP, samples_ptr=samples.data_ptr(), tick_capacity=TCAP,
                     counts_ptr=counts.data_ptr(), draw_capacity=b.cap)
        t.cuda.synchronize(b.dev)
        on_flow = int(b.res.engine_stats.flow_scenarios)          # (the batch's own share of the stage-parallel kernel)
        assert on_flow > 0 and int(st.flow_scenarios) == (on_flow if kernels == "stage_parallel" else 0), (kernels, int(st.flow_scenarios), on_flow)
        assert t.equal(counts, small_counts), "the wide run counted something else than the compact run"
        assert R.differing_scenarios(counts, clock, samples, small_counts, small_clock, small_samples).size == 0
        assert R.differing_scenarios(counts, clock, samples, b.counts_t, b.clock_t, b.samples_t).size == 0
        c = counts.to(t.int64) & 0xFFFFFFFF
        live = t.arange(CAP, device=b.dev)[None, :] < c[:, _abi.CNT_COMPLETED, None]
        assert bool((((clock[..., 0] == FILL_ROW[0]) & (clock[..., 1] == FILL_ROW[1])) | live).all()), "a clock row behind the completed ones was written"
        live = t.arange(TCAP, device=b.dev)[None, :] < c[:, _abi.CNT_TICKS, None]
        assert bool(((samples == FILL_WORD).all(dim=2) | live).all()), "a sample row behind the ticks was written"
    finally:
        eng.close()
        clock[:, :b.cap] = b.clock_t                              # the arena as the other tests of the placement find it
        samples[:, :b.tick_cap] = b.samples_t
        fill_clock(clock[:, b.cap:])
        samples[:, b.tick_cap:] = FILL_WORD
    free_memory()


# ---- 5. the Python surface -------------------------------------------------------------------------------------------------------------
def test_the_results_object_over_wide_buffers():
    """BatchedResults takes foreign buffers through its constructor, as SimulationRunner.run() builds it: no private hook."""
    wb, _ = placed("both")
    b = compact()
    res = b.res
    wide = R.BatchedResults(b.plan, res.seeds, b.counts_t, wb.clock_t, wb.samples_t, res.engine_stats, res.wall_s, res.overrides, draw_capacity=res.draw_capacity)
    calls = [("window_summary", lambda r: r.window_summary(10.0, by=b.grid)),
             ("quantile_summary", lambda r: r.quantile_summary(H.LEVELS, thresholds=H.SLO_THR, edges=b.edges, by=b.grid)),
             ("series_window_summary", lambda r: r.series_window_summary(10.0, by=b.grid)),
             ("in_flight_summary", lambda r: r.in_flight_summary(10.0, by=b.grid)),
             ("latency_histogram_summary", lambda r: r.latency_histogram_summary(10.0, by=b.grid))]
    try:
        for k, fn in calls:
            a, c = H._arrays(fn(wide)), H._arrays(fn(res))  # noqa: SLF001
            assert a, k
            H._same_arrays(a, c, f"{k}: wide and compact buffers")  # noqa: SLF001
        one, ref = wide[S_MAX], res[S_MAX]
        assert np.array_equal(one.rqs_clock.view(np.uint64), ref.rqs_clock.view(np.uint64)) and one.rqs_clock.shape[0] > 0
        sampled, sampled_ref = one.get_sampled_metrics(), ref.get_sampled_metrics()
        assert set(sampled) == set(sampled_ref) and sampled
        for metric, per in sampled_ref.items():
            assert set(sampled[metric]) == set(per)
            for k, v in per.items():
                assert len(v) > 0 and np.array_equal(np.asarray(sampled[metric][k]), np.asarray(v)), (metric, k)
    finally:
        wide.close()
        res.close()
    arena_intact(wb)
    free_memory()


# ---- the widest tiers: where the memory is free ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", WIDEST_CLOCK)
def test_widest_clock_rows_equal_the_host_definition(name):
    """Clock rows at the stride 187 000 003: the row index of scenario 23 passes 2^32."""
    check("widest", name)


def _per_tick(call: str, key: str) -> None:
    """One per-tick output [24, WIDEST] u32 of a call over the compact clock rows; row 23 starts past word 2^32."""
    release_all()
    b, t = compact(), torch_of()
    assert S_MAX * WIDEST >= 1 << 32
    claim(N * WIDEST * 4, f"the per-tick output [24, {WIDEST}]", False)
    want = H.probes()[call].host()
    Wt = len(b.tick_edges) - 1
    big = t.full((N, WIDEST), SENTINEL, dtype=t.int32, device=b.dev)
    count = t.full((N if call == "alerts" else 3, Wt), SENTINEL, dtype=t.int32, device=b.dev)
    total = t.zeros((3, Wt), dtype=t.int64, device=b.dev)
    eng = b.engine()
    try:
        t.cuda.synchronize(b.dev)
        if call == "inflight":
            eng.summarize_inflight(N, 3, b.tick_edges, b.period, tick_capacity=WIDEST, count_ptr=count.data_ptr(), sum_ptr=total.data_ptr(),
                                   in_flight_ptr=big.data_ptr(), group_ptr=b.group_ptr(b.three), threshold=3, bins=0, lo=0, **b.clock_kw)
        else:
            look = int(round(1.0 / b.period))                     # (the rules and the objective of the table's probe)
            slo = float(np.quantile(np.concatenate([r[:, 1] - r[:, 0] for r in b.rows]), 0.9))
            eng.summarize_alerts(N, 3, b.tick_edges, b.period, slo, [(look, look, 1, 5, 1, 1), (5 * look, look, 1, 8, 5, 2)], tick_capacity=WIDEST,
                                 group_ptr=b.group_ptr(b.three), delay_bins=8, delay_width=4, ptrs={"count": count.data_ptr(), key: big.data_ptr()}, **b.clock_kw)
        t.cuda.synchronize(b.dev)
    finally:
        eng.close()
    assert np.array_equal(count.cpu().numpy().view(np.uint32).reshape(-1), np.asarray(want["count"]).astype(np.uint32).reshape(-1))
    if call == "inflight":
        assert np.array_equal(total.cpu().numpy().view(np.uint64).reshape(-1), np.asarray(want["sum"]).astype(np.uint64).reshape(-1))
    host = np.asarray(want[key]).astype(np.uint32).reshape(N, b.tick_cap)       # (the sentinel from a scenario's t_s on)
    assert all((host[s, :b.ticks[s]] != SENTINEL).any() and (host[s, b.ticks[s]:] == SENTINEL).all() for s in range(N))
    assert t.equal(big[:, :b.tick_cap], t.as_tensor(host.view(np.int32), device=b.dev)), f"{call}: the first t_s words of a row of {key} differ"
    assert bool((big[:, b.tick_cap:] == SENTINEL).all()), f"{call}: {key} was written past a scenario's ticks"
    free_memory()


def test_widest_per_tick_in_flight():
    _per_tick("inflight", "in_flight")


def test_widest_per_tick_firing():
    _per_tick("alerts", "firing")


def _sparse_groups(n_groups: int) -> tuple[np.ndarray, np.ndarray]:
    used = np.array([0, 1, n_groups // 4, n_groups // 2, n_groups // 2 + 1, n_groups - 2, n_groups - 1], dtype=np.int64)
    ids = used[np.arange(N) % used.shape[0]]
    ids[[3, 10]] = -1
    return ids, used


def test_sparse_latency_histogram_cells_past_2_31_words():
    """Capacity rule, as the comment of af_latency_histogram_t in include/asyncflow_hip.h has it ("Refused, no output touched: ...
    n_groups * W' * n_bins >= 2^32, a group whose members hold 2^32 or more stored rows together (AF_ERR_CAPACITY)"; the rule with
    2^32 - 1 further down that file is af_state_bins_t's).  `hist`, the
    largest output, has n_groups * 6 * 1024 words: past 2^31 from n_groups = 349 526.  An empty cell is all zero."""
    release_all()
    b, t = compact(), torch_of()
    W, B, G = H.N_WIN, 32 << 5, 349_527
    C = G * W
    assert 1 << 31 < C * B < 1 << 32
    claim(C * B * 4 + C * 20, f"the histograms [{C}, {B}]", False)
    ids, used = _sparse_groups(G)
    hist = t.full((C, B), SENTINEL, dtype=t.int32, device=b.dev)
    count = t.full((C,), SENTINEL, dtype=t.int64, device=b.dev)
    under, over, nan = (t.full((C,), SENTINEL, dtype=t.int32, device=b.dev) for _ in range(3))
    eng = b.engine()
    try:
        t.cuda.synchronize(b.dev)
        eng.summarize_latency_histogram(N, G, edges=b.edges, window_of="arrival", count_ptr=count.data_ptr(), hist_ptr=hist.data_ptr(), under_ptr=under.data_ptr(),
                                        over_ptr=over.data_ptr(), nan_ptr=nan.data_ptr(), group_ptr=b.group_ptr(ids), **b.clock_kw)
        t.cuda.synchronize(b.dev)
    finally:
        eng.close()
    cells = t.as_tensor((used[:, None] * W + np.arange(W)[None, :]).reshape(-1), device=b.dev)
    host = [R.latency_histogram([b.rows[s] for s in b.members(ids, g)], b.edges, "arrival") for g in used]
    for k, x in (("count", count), ("hist", hist), ("under", under), ("over", over), ("nan", nan)):
        got = x[cells].cpu().numpy()
        want = np.concatenate([h[k] for h in host])
        assert want.any() or k in ("under", "over", "nan")
        assert np.array_equal(got.view(np.uint64 if k == "count" else np.uint32).astype(np.uint64), want.astype(np.uint64)), k
        x[cells] = 0
        assert not bool(x.any()), f"an unused cell of {k} is not zero"
    free_memory()


def test_sparse_exemplar_cells_past_2_31_words():
    """Capacity rule (include/asyncflow_hip.h, af_exemplars_t): n_groups * W' * k >= 2^32 is refused.  `state`, the largest
    output, has n_groups * 6 * 64 * 12 words: past 2^31 from n_groups = 466 034, where n_groups * W' * k is 2^27.4.  An empty cell:
    total = kept = 0 and every byte of its slots 0xFF."""
    release_all()
    b, t = compact(), torch_of()
    W, K, S, G = H.N_WIN, 64, b.S, 466_035
    C = G * W
    assert S == 12 and C * K * S > 1 << 31 and C * K < 1 << 32
    claim(C * K * (S * 4 + 16 + 8) + C * 12, f"the exemplars [{C}, {K}]", False)
    ids, used = _sparse_groups(G)
    total = t.full((C,), SENTINEL, dtype=t.int64, device=b.dev)
    kept = t.full((C,), SENTINEL, dtype=t.int32, device=b.dev)
    scen, row = (t.full((C, K), SENTINEL, dtype=t.int32, device=b.dev) for _ in range(2))
    pair = t.zeros((C, K, 2), dtype=t.int64, device=b.dev)
    state = t.full((C, K, S), SENTINEL, dtype=t.int32, device=b.dev)
    eng = b.engine()
    try:
        t.cuda.synchronize(b.dev)
        eng.summarize_exemplars(N, G, K, edges=b.edges, total_ptr=total.data_ptr(), kept_ptr=kept.data_ptr(), scenario_ptr=scen.data_ptr(), row_ptr=row.data_ptr(),
                                pair_ptr=pair.data_ptr(), state_ptr=state.data_ptr(), samples_ptr=b.samples_t.data_ptr(), tick_capacity=b.tick_cap,
                                sample_period=b.period, group_ptr=b.group_ptr(ids), **b.clock_kw)
        t.cuda.synchronize(b.dev)
    finally:
        eng.close()
    cells = t.as_tensor((used[:, None] * W + np.arange(W)[None, :]).reshape(-1), device=b.dev)
    host = [R.latency_exemplars([b.rows[s] for s in b.members(ids, g)], K, b.edges, "finish", scenario_ids=b.members(ids, g),
                                samples=[b.words[s] for s in b.members(ids, g)], sample_period=b.period) for g in used]
    for k, x, empty in (("total", total, 0), ("kept", kept, 0), ("scenario", scen, -1), ("row", row, -1), ("clock", pair, -1), ("state", state, -1)):
        got = x[cells].cpu().numpy()
        want = np.ascontiguousarray(np.concatenate([h[k] for h in host]))
        if want.dtype.kind == "f":
            got, want = got.view(np.uint64), want.view(np.uint64)
        else:
            bits = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
            got, want = got.view(bits), want.astype(bits)
        assert got.shape == want.shape and np.array_equal(got, want), k
        x[cells] = empty
        assert bool((x == empty).all()), f"an unused cell of {k} does not hold what an empty cell holds"
    assert sum(int(h["kept"].sum()) for h in host) > 0
    free_memory()


# ---- the module's memory ------------------------------------------------------------------------------------------------------------
def test_the_peak_stays_below_100_GiB():
    """Last.  Two figures, both under the bound: what the tensors of this module took at their peak (temporaries included, the
    engines' own buffers not), and what the device had less free than at the module's start at its lowest -- read after every call
    while its engine, with the arrival rows and the pool it allocated itself, was still open (temporaries of a comparison not
    included)."""
    t = torch_of()
    release_all()
    peak = int(t.cuda.max_memory_allocated(compact().dev))
    free, total = free_memory()
    taken = _STATE["free_at_start"] - _STATE["low_free"]
    print(f"\npeak torch.cuda.max_memory_allocated: {peak / GIB:.2f} GiB; free at the start {_STATE['free_at_start'] / GIB:.2f}, at the lowest after a call "
          f"{_STATE['low_free'] / GIB:.2f} of {total / GIB:.2f} GiB: {taken / GIB:.2f} "
          f"GiB taken; free now: {free / GIB:.2f} GiB, "
          f"of which torch holds {t.cuda.memory_allocated(compact().dev) / GIB:.2f} GiB in tensors and {t.cuda.memory_reserved(compact().dev) / GIB:.2f} GiB reserved")
    assert peak < 100 * GIB, f"{peak / GIB:.2f} GiB"
    assert taken < 100 * GIB, f"{taken / GIB:.2f} GiB"
