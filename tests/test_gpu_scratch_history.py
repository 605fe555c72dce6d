"""Every analyzer entry point against its host definition WHATEVER ITS SCRATCH HELD BEFORE.

All analyzer calls of one engine lay their device scratch over one pool (af_engine::d_pool, engine.hip), which a results object
shares between its ``*_summary`` methods: a call finds there what the call before it left.  This module holds one table of probe
calls -- one or two per entry point, each on its analyzer's scratch-heavy path -- over one small simulated batch, and runs each
of them

* on a fresh engine, against the host definition, every output word (a);
* on a pool twice as large as it needs that ``af_probe_scratch`` filled with 0xFFFFFFFF (the NONE / SKIP sentinel, the largest
  count, a NaN), with zeros, and with 0x3FF00000 (as a pair of words a float64 about 1.0, as one word a large count) (b);
* on a pool that is too small at 0 bytes, 256 bytes, half and all but 256 bytes of what the call needs, so that it grows -- in the
  windowed family in the middle of the call -- and the grown pool is full of 0xFFFFFFFF too (c);
* after every other probe on one engine (d); ``af_engine_run`` and ``af_engine_summarize_arrivals`` in turn on one engine,
  which share the arrival buffers and flags (e); and through the Python API in two call orders and with an engine per call (f).
  ``af_engine_summarize`` and ``af_engine_run_summarized`` take nothing from the pool: (b) and (c) cannot reach them, (d) does.

(b) to (e) compare raw output words with those of (a), bit for bit.  Every output of a call lies in one buffer between sentinel
words."""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Any, Callable

import numpy as np
import pytest

from asyncflow_amd import _abi, expand_grid
from asyncflow_amd import results as R
from oracle import analyzer_oracle as ao
from oracle.scenarios import lb_with_events

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
GUARD = 16                  # sentinel words on both sides of every output (a multiple of 4: outputs stay 16-byte aligned)
WORDS = (0xFFFFFFFF, 0x00000000, 0x3FF00000)
USERS = "rqs_input.avg_active_users.mean"
N_WIN = 6
LEVELS, SLO_THR = (0.5, 0.9, 0.999, 0.0, 1.0), (0.02, 0.05)
SERIES_LEVELS = (0.5, 0.95, 0.99)
STATE_BINS = 4
HIST_BINS, HIST_MAX = 64, 0.128
PAIR_BINNING = (3, -16, 16)               # sub_bits, min_exp, octaves: 128 bins
LARGE_LATENCY_CELL = 8192                 # above it a latency cell takes the radix-select / tiled passes
LARGE_SERIES_CELL = 2048                  # above it a series cell takes the histogram-pass select


def _r256(x: int) -> int:
    return (int(x) + 255) & ~255


@dataclass
class Probe:
    """One call: its outputs ``(name, dtype, shape)``, the call itself (``call(engine, {name: device pointer}) -> scratch_bytes``
    or None where the entry point reports none), the host definition (``want() -> {name: array}``; a uint32 output may hold
    SENTINEL where the call must leave the word alone) and what makes it take the scratch-heavy path."""

    name: str
    outs: list[tuple[str, Any, tuple[int, ...]]]
    call: Callable[[Any, dict[str, int]], int | None]
    want: Callable[[], dict[str, np.ndarray]]
    path: Callable[[], None] = lambda: None
    uses_pool: bool = True
    first_part: int = 0                   # the windowed family: bytes of the first part of the scratch (0: not of that family)
    refused: Callable[[Any, dict[str, int]], int] | None = None   # an AF_ERR_INVALID variant of the call (raw return code)
    cache: dict = field(default_factory=dict)

    def layout(self) -> tuple[dict[str, tuple[int, int]], int]:
        off, at = {}, GUARD
        for k, dt, shape in self.outs:
            size = int(np.prod(shape)) * np.dtype(dt).itemsize // 4
            off[k] = (at, size)
            at += ((size + 3) & ~3) + GUARD
        return off, at

    def host(self) -> dict[str, np.ndarray]:
        if "want" not in self.cache:
            self.cache["want"] = self.want()
        return self.cache["want"]


class Batch:
    """The simulated batch, on the device and on the host, and what the probes share."""

    def __init__(self) -> None:
        import torch

        from asyncflow_amd.engine import Engine
        from asyncflow_amd.plan import lower
        from asyncflow_amd.runner import SimulationRunner, resolve_sweep

        payload = lb_with_events(horizon=60, scale=0.1)
        self.edge_axis = f"topology_graph.edges[{lower(payload).edge_ids[0]}].latency.mean"
        self.grid = expand_grid({self.edge_axis: [0.002, 0.006], USERS: [60.0, 200.0]}, replicas=6, common_seeds=True)
        self.runner = SimulationRunner(simulation_input=payload, **self.grid.runner_kwargs())
        self.res = res = self.runner.run()
        self.plan = plan = res.plan
        self.n = n = len(res)
        assert n == 24
        self.dev = res._counts_t.device  # noqa: SLF001
        self.clock_t, self.samples_t, self.counts_t = res._clock_t, res._samples_t, res._counts_t  # noqa: SLF001
        self.cap, self.tick_cap = int(self.clock_t.shape[1]), int(self.samples_t.shape[1])
        self.period = float(plan.sample_period)
        self.rows = [res[s].rqs_clock for s in range(n)]
        self.words = [res[s]._samples for s in range(n)]  # noqa: SLF001   uint32 [n_series, ticks]
        self.ticks = [w.shape[1] for w in self.words]
        self.S = plan.n_series
        over = resolve_sweep(plan, self.runner.sweep, n)
        self.run_cols = [(c, i, v) for c, i, v, _ in over]
        cap, fifo, clock_cap = self.runner._capacities(over)  # noqa: SLF001
        assert clock_cap == self.cap
        self.engine_kw = self.runner._engine_kw(cap, fifo)  # noqa: SLF001
        self.Engine = Engine
        self.torch = torch
        # groupings: all in one; three groups, the middle one empty, two scenarios in none; singletons
        self.one = np.zeros(n, dtype=np.int64)
        self.three = np.where(np.arange(n) % 2 == 0, 0, 2).astype(np.int64)
        self.three[[3, 10]] = -1
        self.single = np.arange(n, dtype=np.int64)
        self.edges = np.linspace(0.0, float(plan.total_time), N_WIN + 1)
        self.whole = np.array([0.0, float(plan.total_time)])
        t = self.tick_cap
        self.tick_edges = np.array([0, t // 7, t // 3, t // 2, (2 * t) // 3, t - 5, t + 9], dtype=np.uint32)   # (the last past every t_s)
        self.tick_whole = np.array([0, t], dtype=np.uint32)
        self._groups: dict[bytes, Any] = {}
        # series: the ready queue of server 0, the I/O queue of server 1 (integers), the RAM of server 0 (float32 words)
        self.col_ready, self.col_io, self.col_ram = plan.n_edges, plan.n_edges + 3 + 1, plan.n_edges + 2
        assert R.ram_columns(self.S, plan.n_edges)[self.col_ram] and not R.ram_columns(self.S, plan.n_edges)[[self.col_ready, self.col_io]].any()
        self.int_cols = np.nonzero(~R.ram_columns(self.S, plan.n_edges))[0]

    def engine(self):
        return self.Engine(self.plan, self.dev.index or 0, **self.engine_kw)

    def group_ptr(self, ids: np.ndarray) -> int:
        key = np.asarray(ids, dtype=np.int64).tobytes()
        if key not in self._groups:
            self._groups[key] = self.u32(np.where(ids < 0, _abi.POOL_SKIP, ids))
        return self._groups[key].data_ptr()

    def u32(self, v: Any):
        return self.torch.as_tensor(np.ascontiguousarray(v).astype(np.uint32).view(np.int32), device=self.dev)

    @property
    def clock_kw(self) -> dict[str, int]:
        return {"clock_ptr": self.clock_t.data_ptr(), "clock_capacity": self.cap, "counts_ptr": self.counts_t.data_ptr()}

    @property
    def series_kw(self) -> dict[str, int]:
        return {"samples_ptr": self.samples_t.data_ptr(), "tick_capacity": self.tick_cap, "counts_ptr": self.counts_t.data_ptr()}

    def members(self, ids: np.ndarray, g: int) -> np.ndarray:
        return np.nonzero(np.asarray(ids) == g)[0]

    # ---- what a batch of other strides answers differently (tests/test_gpu_wide_strides.py)
    def draw_capacity(self, gen_cap: int) -> int:
        """The stride of the arrival rows on the device; the host definitions keep the run's own `gen_cap`."""
        return gen_cap

    @property
    def run_draw_capacity(self) -> int:
        """The draw capacity of the run of the run_summarized probe."""
        return self.cap

    def time_rows(self, ia: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
        """The scenario whose arrival times row r of the pairs' time rows holds, and the row that every pair reads."""
        return np.unique(ia, return_inverse=True)

    def arrival_rows(self, host: np.ndarray) -> Any:
        """The pairs' time rows [rows, draw_capacity] on the device."""
        return self.torch.as_tensor(host, device=self.dev)

    def run_buffers(self) -> tuple[Any, Any]:
        """The clock and sample rows that the run of the run_summarized probe writes, of this batch's capacities."""
        if "run_out" not in self.__dict__:
            self.run_out = (self.torch.empty_like(self.clock_t), self.torch.zeros_like(self.samples_t))
        return self.run_out


# ---- host definitions over the groups ------------------------------------------------------------------------------------------
def latency_cells(b: Batch, kind: str, ids: np.ndarray, n_groups: int, edges: Any) -> list[np.ndarray]:
    """The latencies of every cell (group, window or key), the members' in ascending scenario order: what numpy is given."""
    def of(s: int) -> list[np.ndarray]:
        ck = b.rows[s]
        if kind == "whole":
            return [ck[:, 1] - ck[:, 0]]
        if kind == "state":
            return R.latency_state_cells(ck, b.words[s], b.plan.n_edges, b.period, b.col_ready, STATE_BINS, 0.0, 1.0, edges)
        return R._window_latencies(ck, R.check_edges(edges), kind)  # noqa: SLF001
    per = {s: of(s) for s in range(b.n) if ids[s] >= 0}
    n_cell = len(next(iter(per.values())))
    return [np.concatenate([per[s][c] for s in b.members(ids, g)] + [np.zeros(0)]) for g in range(n_groups) for c in range(n_cell)]


def stats_of(cells: list[np.ndarray]) -> dict[str, np.ndarray]:
    return {"stats": np.stack([R.latency_stats_row(np.ascontiguousarray(x)) for x in cells])}


def quantiles_of(cells: list[np.ndarray]) -> dict[str, np.ndarray]:
    return {"count": np.array([x.shape[0] for x in cells], dtype=np.uint32),
            "quantiles": np.stack([R.latency_quantiles(x, LEVELS) for x in cells]),
            "within": np.stack([R.latency_within(x, SLO_THR) for x in cells]).astype(np.uint32)}


def series_cells(b: Batch, ids: np.ndarray, n_groups: int, tick_edges: np.ndarray) -> list[np.ndarray]:
    """The sample words [n_series, m] of every (group, window): the members' window rows side by side in scenario order."""
    out = []
    for g in range(n_groups):
        for w in range(len(tick_edges) - 1):
            seg = [b.words[s][:, min(int(tick_edges[w]), b.ticks[s]):min(int(tick_edges[w + 1]), b.ticks[s])] for s in b.members(ids, g)]
            out.append(np.concatenate(seg + [np.zeros((b.S, 0), dtype=np.uint32)], axis=1))
    return out


def per_cell(cells: list[np.ndarray], fn: Callable[[np.ndarray], dict[str, np.ndarray]], keys: tuple[str, ...]) -> dict[str, np.ndarray]:
    """fn on every cell as ONE window [0, m) (an empty cell: the window [0, 1) of no row)."""
    got = [fn(c) for c in cells]
    return {k: np.stack([np.asarray(x[k])[0] for x in got]) for k in keys}


def wide(values: Any, words: int) -> np.ndarray:
    """Python integers as `words` uint64 words each, the low word first."""
    flat = [int(v) for v in np.asarray(values, dtype=object).reshape(-1)]
    return np.array([[(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(words)] for v in flat], dtype=np.uint64)


# ---- the probes ------------------------------------------------------------------------------------------------------------------
def build_probes(b: Batch) -> list[Probe]:
    n, S, f64, u32, u64 = b.n, b.S, np.float64, np.uint32, np.uint64
    probes: list[Probe] = []
    big_lat = lambda cells: lambda: _assert(max(x.shape[0] for x in cells()) > LARGE_LATENCY_CELL, "no cell above 8 192 latencies")  # noqa: E731
    small_lat = lambda cells: lambda: _assert(0 < max(x.shape[0] for x in cells()) <= LARGE_LATENCY_CELL and min(x.shape[0] for x in cells()) == 0,  # noqa: E731
                                              "the cells of three groups x six windows are not all small, one of them empty")

    def cached(fn):
        box: dict = {}

        def get():
            if "v" not in box:
                box["v"] = fn()
            return box["v"]
        return get

    def first_part(n_win: int, n_edge: int | None = None) -> int:
        return _r256((n_win + 1 if n_edge is None else max(n_edge, 1)) * 8) + _r256(4) + _r256(n * (n_win + 1) * 4)

    for tag, ids, G, win_edges in (("one_group", b.one, 1, b.whole), ("three_groups", b.three, 3, b.edges)):
        big = tag == "one_group"
        W = len(win_edges) - 1
        gp = b.group_ptr(ids)
        # pooled
        cells = cached(lambda ids=ids, G=G: latency_cells(b, "whole", ids, G, None))
        probes.append(Probe(f"pooled-{tag}", [("stats", f64, (G, 8))],
                            lambda e, p, G=G, gp=gp: _unreported(e.summarize_pooled(n, G, stats_ptr=p["stats"], group_ptr=gp, **b.clock_kw)),
                            lambda cells=cells: stats_of(cells()), big_lat(cells) if big else lambda: None,
                            refused=lambda e, p, G=G, gp=gp: e._lib.af_engine_summarize_pooled(  # noqa: SLF001
                                e._h, C.byref(_abi.AfOutputs(b.cap, C.c_void_p(b.clock_t.data_ptr()), 0, None, C.c_void_p(b.counts_t.data_ptr()))),  # noqa: SLF001
                                C.byref(_abi.AfPooled(n, 0, C.c_void_p(gp), C.c_void_p(p["stats"]), 0.0)))))
        # windows by finish and by arrival time
        for by in ("finish", "arrival"):
            cells = cached(lambda ids=ids, G=G, by=by, e=win_edges: latency_cells(b, by, ids, G, e))
            name = "windows" if by == "finish" else "arrival_windows"
            probes.append(Probe(f"{name}-{tag}", [("stats", f64, (G, W, 8))],
                                lambda e, p, G=G, gp=gp, by=by, ed=win_edges: e.summarize_windows(n, G, ed, stats_ptr=p["stats"], group_ptr=gp, window_of=by, **b.clock_kw)[1],
                                lambda cells=cells: stats_of(cells()), big_lat(cells) if big else small_lat(cells), first_part=first_part(W),
                                refused=lambda e, p, G=G, gp=gp, by=by: _raises_invalid(
                                    lambda: e.summarize_windows(n, G, [0.0, 5.0, 5.0], stats_ptr=p["stats"], group_ptr=gp, window_of=by, **b.clock_kw))))
            q_edges = None if big and by == "finish" else win_edges          # (the whole run without windows: the pooled layout)
            name = "quantiles" if by == "finish" else "arrival_quantiles"
            probes.append(Probe(f"{name}-{tag}", [("count", u32, (G, W)), ("quantiles", f64, (G, W, len(LEVELS))), ("within", u32, (G, W, len(SLO_THR)))],
                                lambda e, p, G=G, gp=gp, by=by, ed=q_edges: e.summarize_quantiles(
                                    n, G, LEVELS, edges=ed, thresholds=SLO_THR, count_ptr=p["count"], quantiles_ptr=p["quantiles"], within_ptr=p["within"],
                                    group_ptr=gp, window_of=by, **b.clock_kw)[1],
                                lambda cells=cells: quantiles_of(cells()), big_lat(cells) if big else small_lat(cells),
                                first_part=0 if q_edges is None else first_part(W),
                                refused=lambda e, p, G=G, gp=gp, by=by, ed=q_edges: _quantiles_refused(b, e, p, G, gp, by, ed)))
        # by the state met on arrival: the keys of a group are (arrival window, bin of the ready queue of server 0)
        st_edges = None if big else win_edges
        K = (1 if big else W) * STATE_BINS
        cells = cached(lambda ids=ids, G=G, e=st_edges: latency_cells(b, "state", ids, G, e))
        state_kw = {"column": b.col_ready, "bins": STATE_BINS, "sample_period": b.period}
        probes.append(Probe(f"state_windows-{tag}", [("stats", f64, (G, K, 8))],
                            lambda e, p, G=G, gp=gp, ed=st_edges: e.summarize_state_windows(
                                n, G, edges=ed, stats_ptr=p["stats"], group_ptr=gp, samples_ptr=b.samples_t.data_ptr(), tick_capacity=b.tick_cap,
                                **state_kw, **b.clock_kw)[1],
                            lambda cells=cells: stats_of(cells()), big_lat(cells) if big else small_lat(cells),
                            first_part=first_part(K, 0 if big else W + 1),
                            refused=lambda e, p, G=G, gp=gp, ed=st_edges: _raises_invalid(lambda: e.summarize_state_windows(
                                n, G, edges=ed, stats_ptr=p["stats"], group_ptr=gp, samples_ptr=0, tick_capacity=b.tick_cap, **state_kw, **b.clock_kw))))
        probes.append(Probe(f"state_quantiles-{tag}", [("count", u32, (G, K)), ("quantiles", f64, (G, K, len(LEVELS))), ("within", u32, (G, K, len(SLO_THR)))],
                            lambda e, p, G=G, gp=gp, ed=st_edges: e.summarize_state_quantiles(
                                n, G, LEVELS, thresholds=SLO_THR, edges=ed, count_ptr=p["count"], quantiles_ptr=p["quantiles"], within_ptr=p["within"],
                                group_ptr=gp, samples_ptr=b.samples_t.data_ptr(), tick_capacity=b.tick_cap, **state_kw, **b.clock_kw)[1],
                            lambda cells=cells: quantiles_of(cells()), big_lat(cells) if big else small_lat(cells),
                            first_part=first_part(K, 0 if big else W + 1)))

    # ---- the sampled series
    te, tw, gp3 = b.tick_edges, b.tick_whole, b.group_ptr(b.three)
    Wt = len(te) - 1
    q_cols = np.array([b.col_io, b.col_ram, b.col_ready])
    cells_q = cached(lambda: series_cells(b, b.one, 1, tw))
    probes.append(Probe("series_quantiles-one_group", [("count", u32, (1, 1)), ("quantiles", f64, (1, 1, len(q_cols), len(SERIES_LEVELS)))],
                        lambda e, p: e.summarize_series_quantiles(n, 1, tw, SERIES_LEVELS, quantiles_ptr=p["quantiles"], count_ptr=p["count"],
                                                                  group_ptr=b.group_ptr(b.one), columns=q_cols, **b.series_kw)[1],
                        lambda: dict(zip(("count", "quantiles"), R.series_window_quantiles(cells_q()[0], [0, max(cells_q()[0].shape[1], 1)], b.plan.n_edges,
                                                                                           SERIES_LEVELS, q_cols))),
                        lambda: _assert(cells_q()[0].shape[1] > LARGE_SERIES_CELL, "no cell above 2 048 series values"),
                        refused=lambda e, p: _raises_invalid(lambda: e.summarize_series_quantiles(
                            n, 1, tw, SERIES_LEVELS, quantiles_ptr=p["quantiles"], count_ptr=p["count"], group_ptr=b.group_ptr(b.one), columns=q_cols,
                            samples_ptr=0, tick_capacity=b.tick_cap, counts_ptr=b.counts_t.data_ptr()))))
    for tag, ids, G in (("three_groups", b.three, 3), ("singletons", b.single, n)):
        cells_s = cached(lambda ids=ids, G=G: series_cells(b, ids, G, te))
        probes.append(Probe(f"series_windows-{tag}", [("count", u32, (G, Wt)), ("mean", f64, (G, Wt, S)), ("min", u32, (G, Wt, S)), ("max", u32, (G, Wt, S)),
                                                      ("above", u32, (G, Wt, S))],
                            lambda e, p, ids=ids, G=G: e.summarize_series_windows(n, G, te, count_ptr=p["count"], mean_ptr=p["mean"], min_ptr=p["min"],
                                                                                  max_ptr=p["max"], above_ptr=p["above"], group_ptr=b.group_ptr(ids), **b.series_kw)[1],
                            lambda cells_s=cells_s: per_cell(cells_s(), lambda x: R.series_window_stats(x, [0, max(x.shape[1], 1)], b.plan.n_edges),
                                                             ("count", "mean", "min", "max", "above")),
                            refused=lambda e, p, ids=ids, G=G: _raises_invalid(lambda: e.summarize_series_windows(
                                n, G, te, count_ptr=p["count"], mean_ptr=p["mean"], group_ptr=b.group_ptr(ids), samples_ptr=0, tick_capacity=b.tick_cap,
                                counts_ptr=b.counts_t.data_ptr()))))
    ex_keys = ("count", "above", "runs", "longest", "longest_start", "first", "last", "peak_tick")
    probes.append(Probe("series_excursions", [("count", u32, (n, Wt))] + [(k, u32, (n, Wt, S)) for k in ex_keys[1:]],
                        lambda e, p: e.summarize_series_excursions(n, te, **{f"{k}_ptr": p[k] for k in ex_keys}, **b.series_kw)[1],
                        lambda: {k: np.stack([R.series_window_excursions(b.words[s], te, b.plan.n_edges)[k] for s in range(n)]) & 0xFFFFFFFF for k in ex_keys},
                        refused=lambda e, p: _raises_invalid(lambda: e.summarize_series_excursions(
                            n, te, **{f"{k}_ptr": p[k] for k in ex_keys}, samples_ptr=0, tick_capacity=b.tick_cap, counts_ptr=b.counts_t.data_ptr()))))
    h_bins = 16

    def hist_want():
        per = [R.series_window_histogram(b.words[s], te, b.plan.n_edges, h_bins) for s in range(n)]
        out = {k: np.zeros((3,) + per[0][k].shape, dtype=np.int64) for k in ("count", "hist", "under", "over")}
        for s in range(n):
            if b.three[s] >= 0:
                for k in out:
                    out[k][b.three[s]] += per[s][k]
        return out
    probes.append(Probe("series_histogram", [("count", u32, (3, Wt)), ("hist", u32, (3, Wt, S, h_bins)), ("under", u32, (3, Wt, S)), ("over", u32, (3, Wt, S))],
                        lambda e, p: e.summarize_series_histogram(n, 3, te, h_bins, hist_ptr=p["hist"], count_ptr=p["count"], under_ptr=p["under"],
                                                                  over_ptr=p["over"], group_ptr=gp3, **b.series_kw)[1],
                        hist_want,
                        refused=lambda e, p: _raises_invalid(lambda: e.summarize_series_histogram(
                            n, 3, te, h_bins, hist_ptr=p["hist"], count_ptr=p["count"], under_ptr=p["under"], over_ptr=p["over"], group_ptr=gp3,
                            samples_ptr=0, tick_capacity=b.tick_cap, counts_ptr=b.counts_t.data_ptr()))))
    ready = np.array([b.plan.n_edges + 3 * v for v in range(len(b.plan.server_ids))])
    combos = [("sum", ready), ("max", ready), ("spread", ready), ("min", np.array([b.col_io]))]
    c_bins, NC = 8, len(combos)
    cells_c = cached(lambda: series_cells(b, b.three, 3, te))
    c_keys = ("count", "mean", "min", "max", "above", "hist", "under", "over")
    probes.append(Probe("series_combined", [("count", u32, (3, Wt)), ("mean", f64, (3, Wt, NC)), ("min", f64, (3, Wt, NC)), ("max", f64, (3, Wt, NC)),
                                            ("above", u32, (3, Wt, NC)), ("hist", u32, (3, Wt, NC, c_bins)), ("under", u32, (3, Wt, NC)), ("over", u32, (3, Wt, NC))],
                        lambda e, p: e.summarize_series_combined(n, 3, te, [_abi.COMBINE_OPS[o] for o, _ in combos], [c for _, c in combos],
                                                                 **{f"{k}_ptr": p[k] for k in c_keys}, group_ptr=gp3, bins=c_bins, **b.series_kw)[1],
                        lambda: per_cell(cells_c(), lambda x: R.series_combined_window_stats(x, [0, max(x.shape[1], 1)], b.plan.n_edges, combos, bins=c_bins), c_keys),
                        refused=lambda e, p: _raises_invalid(lambda: e.summarize_series_combined(
                            n, 3, te, [99], [ready], **{f"{k}_ptr": p[k] for k in c_keys}, group_ptr=gp3, bins=c_bins, **b.series_kw))))
    j_pairs = (np.array([b.col_ready, b.col_io, b.col_ready]), np.array([b.col_io, b.col_io, b.col_ready]), np.array([2, 1, 0]))
    NP = 3

    def joint_want():
        per = [R.series_joint_sums(b.words[s], te, b.plan.n_edges, j_pairs) for s in range(n)]
        out = {}
        for k in ("n", "sx", "sy", "sxx", "syy", "sxy"):
            tot = np.zeros((3, Wt, NP), dtype=object)
            tot[...] = 0
            for s in range(n):
                if b.three[s] >= 0:
                    tot[b.three[s]] = tot[b.three[s]] + per[s][k].astype(object)
            out[k] = tot.astype(np.uint32) if k == "n" else wide(tot, 1 if k in ("sx", "sy") else 2)
        return out
    j_keys = ("n", "sx", "sy", "sxx", "syy", "sxy")
    probes.append(Probe("series_joint", [("n", u32, (3, Wt, NP)), ("sx", u64, (3, Wt, NP)), ("sy", u64, (3, Wt, NP)), ("sxx", u64, (3, Wt, NP, 2)),
                                         ("syy", u64, (3, Wt, NP, 2)), ("sxy", u64, (3, Wt, NP, 2))],
                        lambda e, p: e.summarize_series_joint(n, 3, te, *j_pairs, **{f"{k}_ptr": p[k] for k in j_keys}, group_ptr=gp3, **b.series_kw)[1],
                        joint_want,
                        refused=lambda e, p: _raises_invalid(lambda: e.summarize_series_joint(
                            n, 3, te, np.array([b.col_ram, b.col_io, b.col_ready]), j_pairs[1], j_pairs[2], **{f"{k}_ptr": p[k] for k in j_keys}, group_ptr=gp3, **b.series_kw))))
    w_cols = np.array([b.col_io, b.col_ready])

    def warmup_want():
        out: dict[str, list] = {k: [] for k in ("batches", "trunc", "s1", "s2", "s1_all", "s2_all")}
        for g in range(3):
            one = R.series_warmup_sums([b.words[s] for s in b.members(b.three, g)], te, b.plan.n_edges, 5, w_cols)
            for k in out:
                out[k].append(one[k])
        res = {"batches": np.stack(out["batches"]).astype(np.uint32), "trunc": np.stack(out["trunc"]).astype(np.uint32)}
        for k, words in (("s1", 2), ("s2", 3), ("s1_all", 2), ("s2_all", 3)):
            res[k] = wide(np.stack(out[k]), words)
        return res
    w_keys = ("batches", "trunc", "s1", "s2", "s1_all", "s2_all")
    probes.append(Probe("series_warmup", [("batches", u32, (3, Wt)), ("trunc", u32, (3, Wt, 2)), ("s1", u64, (3, Wt, 2, 2)), ("s2", u64, (3, Wt, 2, 3)),
                                          ("s1_all", u64, (3, Wt, 2, 2)), ("s2_all", u64, (3, Wt, 2, 3))],
                        lambda e, p: e.summarize_series_warmup(n, 3, te, w_cols, 5, **{f"{k}_ptr": p[k] for k in w_keys}, group_ptr=gp3, **b.series_kw)[1],
                        warmup_want,
                        refused=lambda e, p: _raises_invalid(lambda: e.summarize_series_warmup(
                            n, 3, te, np.array([b.col_ram]), 5, **{f"{k}_ptr": p[k] for k in w_keys}, group_ptr=gp3, **b.series_kw))))

    # ---- the clock rows per tick, per window, per request
    f_bins = 12
    flight = cached(lambda: [R.in_flight_series(b.rows[s], b.ticks[s], b.period) for s in range(n)])

    def per_tick(host_rows: list[np.ndarray]) -> np.ndarray:
        out = np.full((n, b.tick_cap), SENTINEL, dtype=np.uint32)
        for s in range(n):
            out[s, :b.ticks[s]] = host_rows[s]
        return out

    def inflight_want():
        cells = [R.in_flight_window_stats([flight()[s]["in_flight"] for s in b.members(b.three, g)], te, 3, f_bins, 1) for g in range(3)]
        out = {k: np.stack([np.asarray(c[k]) for c in cells]).astype(np.uint64 if k == "sum" else np.uint32)
               for k in ("count", "sum", "min", "max", "above", "hist", "under")}
        out.update({k: per_tick([f[k] for f in flight()]) for k in ("in_flight", "started", "finished")})
        return out
    f_keys = ("count", "sum", "min", "max", "above", "hist", "under", "in_flight", "started", "finished")
    probes.append(Probe("inflight", [("count", u32, (3, Wt)), ("sum", u64, (3, Wt)), ("min", u32, (3, Wt)), ("max", u32, (3, Wt)), ("above", u32, (3, Wt)),
                                     ("hist", u32, (3, Wt, f_bins)), ("under", u32, (3, Wt))] + [(k, u32, (n, b.tick_cap)) for k in f_keys[7:]],
                        lambda e, p: e.summarize_inflight(n, 3, te, b.period, tick_capacity=b.tick_cap, **{f"{k}_ptr": p[k] for k in f_keys}, group_ptr=gp3,
                                                          threshold=3, bins=f_bins, lo=1, **b.clock_kw)[1],
                        inflight_want,
                        refused=lambda e, p: _raises_invalid(lambda: e.summarize_inflight(
                            n, 3, te, float("nan"), tick_capacity=b.tick_cap, **{f"{k}_ptr": p[k] for k in f_keys}, group_ptr=gp3, threshold=3, bins=f_bins,
                            lo=1, **b.clock_kw))))
    K_EX = 64

    def exemplars_want():
        parts = [R.latency_exemplars([b.rows[s] for s in b.members(b.three, g)], K_EX, b.edges, "finish", scenario_ids=b.members(b.three, g) if len(b.members(b.three, g)) else None,
                                     samples=[b.words[s] for s in b.members(b.three, g)], sample_period=b.period) for g in range(3)]
        for x in parts:                                           # (a group without a member: no state of any series)
            if x["state"].shape[-1] == 0:
                x["state"] = np.full(x["state"].shape[:2] + (S,), 0xFFFFFFFF, dtype=np.uint32)
        out = {k: np.concatenate([x[k] for x in parts]) for k in ("total", "kept", "scenario", "row", "state")}
        out["pair"] = np.concatenate([x["clock"] for x in parts])
        return out
    x_keys = ("total", "kept", "scenario", "row", "pair", "state")
    C_EX = 3 * N_WIN
    probes.append(Probe("exemplars", [("total", u64, (C_EX,)), ("kept", u32, (C_EX,)), ("scenario", u32, (C_EX, K_EX)), ("row", u32, (C_EX, K_EX)),
                                      ("pair", f64, (C_EX, K_EX, 2)), ("state", u32, (C_EX, K_EX, S))],
                        lambda e, p: e.summarize_exemplars(n, 3, K_EX, edges=b.edges, **{f"{k}_ptr": p[k] for k in x_keys}, samples_ptr=b.samples_t.data_ptr(),
                                                           tick_capacity=b.tick_cap, sample_period=b.period, group_ptr=gp3, **b.clock_kw)[1],
                        exemplars_want,
                        refused=lambda e, p: _raises_invalid(lambda: e.summarize_exemplars(
                            n, 3, K_EX, edges=b.edges, **{f"{k}_ptr": p[k] for k in x_keys}, samples_ptr=b.samples_t.data_ptr(), tick_capacity=b.tick_cap,
                            sample_period=0.0, group_ptr=gp3, **b.clock_kw))))
    LB = 32 << 5

    def lhist_want():
        parts = [R.latency_histogram([b.rows[s] for s in b.members(b.three, g)], b.edges, "arrival") for g in range(3)]
        return {k: np.concatenate([x[k] for x in parts]) for k in ("count", "hist", "under", "over", "nan")}
    l_keys = ("count", "hist", "under", "over", "nan")
    probes.append(Probe("latency_histogram", [("count", u64, (C_EX,)), ("hist", u32, (C_EX, LB)), ("under", u32, (C_EX,)), ("over", u32, (C_EX,)), ("nan", u32, (C_EX,))],
                        lambda e, p: e.summarize_latency_histogram(n, 3, edges=b.edges, window_of="arrival", **{f"{k}_ptr": p[k] for k in l_keys}, group_ptr=gp3,
                                                                   **b.clock_kw)[1],
                        lhist_want,
                        refused=lambda e, p: _raises_invalid(lambda: e.summarize_latency_histogram(
                            n, 3, edges=b.edges, window_of="arrival", **{f"{k}_ptr": p[k] for k in l_keys}, group_ptr=gp3, clock_ptr=0, clock_capacity=b.cap,
                            counts_ptr=b.counts_t.data_ptr()))))
    # alerts: the objective is the 0.9 quantile of all latencies, the look-back one second and five
    look = int(round(1.0 / b.period))
    slo = float(np.quantile(np.concatenate([r[:, 1] - r[:, 0] for r in b.rows]), 0.9))
    rules = [(look, look, 1, 5, 1, 1), (5 * look, look, 1, 8, 5, 2)]
    d_bins, d_width = 8, 4
    alerts = cached(lambda: [R.scenario_alerts(b.rows[s], b.ticks[s], b.period, slo, rules, te) for s in range(n)])
    a_cells, a_g32, a_g64, a_ticks = ("fired", "episodes", "longest", "longest_start", "first", "last"), ("members", "fired_members", "open_members"), \
        ("fire_ticks", "fire_episodes"), ("total", "bad", "firing")
    from tests.alerts_util import firing_words

    def alerts_want():
        host = alerts()
        out = {"count": np.stack([h["count"] for h in host]).astype(np.uint32)}
        out.update({k: (np.stack([h[k] for h in host]) & 0xFFFFFFFF).astype(np.uint32) for k in a_cells})
        cells = R.alert_cells(host, b.three, 3, d_bins, d_width)
        out.update({k: cells[k].astype(np.uint32) for k in a_g32 + ("delay_hist",)}, **{k: cells[k].astype(np.uint64) for k in a_g64})
        out.update({k: per_tick([firing_words(h["firing"]) if k == "firing" else h[k] for h in host]) for k in a_ticks})
        return out
    R2 = len(rules)
    a_outs = [("count", u32, (n, Wt))] + [(k, u32, (n, Wt, R2)) for k in a_cells] + [(k, u32, (3, Wt, R2)) for k in a_g32] + \
        [(k, u64, (3, Wt, R2)) for k in a_g64] + [("delay_hist", u32, (3, Wt, R2, d_bins))] + [(k, u32, (n, b.tick_cap)) for k in a_ticks]
    probes.append(Probe("alerts", a_outs,
                        lambda e, p: e.summarize_alerts(n, 3, te, b.period, slo, rules, tick_capacity=b.tick_cap, group_ptr=gp3, delay_bins=d_bins,
                                                        delay_width=d_width, ptrs=dict(p), **b.clock_kw)[1],
                        alerts_want,
                        refused=lambda e, p: _raises_invalid(lambda: e.summarize_alerts(
                            n, 3, te, b.period, slo, [(look, 0, 1, 5, 1, 1)], tick_capacity=b.tick_cap, group_ptr=gp3, delay_bins=d_bins, delay_width=d_width,
                            ptrs=dict(p), **b.clock_kw))))

    # ---- arrivals, and pairs through them
    gen_seeds, gen_cols, gen_cap = b.res._arrival_sweep()  # noqa: SLF001
    draw_cap = b.draw_capacity(gen_cap)
    arrivals = cached(lambda: _host_arrivals(b, gen_cap))

    def arrivals_want():
        rb = np.stack([R.arrival_window_counts(t, b.edges) for t, _ in arrivals()])
        per = np.diff(rb, axis=1)
        return {"arrivals": np.stack([per[b.members(b.three, g)].sum(axis=0) for g in range(3)]).astype(np.uint64), "row_bounds": rb.astype(np.uint32),
                "generated": np.array([np.isfinite(t).sum() for t, _ in arrivals()], dtype=np.uint32), "flags": np.array([f for _, f in arrivals()], dtype=np.uint32)}
    probes.append(Probe("arrivals", [("arrivals", u64, (3, N_WIN)), ("row_bounds", u32, (n, N_WIN + 1)), ("generated", u32, (n,)), ("flags", u32, (n,))],
                        lambda e, p: e.summarize_arrivals(gen_seeds, gen_cols, 3, b.edges, draw_capacity=draw_cap, arrivals_ptr=p["arrivals"], group_ptr=gp3,
                                                          row_bounds_ptr=p["row_bounds"], generated_ptr=p["generated"], flags_ptr=p["flags"])[1],
                        arrivals_want,
                        refused=lambda e, p: _raises_invalid(lambda: e.summarize_arrivals(
                            gen_seeds, gen_cols, 3, [0.0, 7.0, 7.0], draw_capacity=draw_cap, arrivals_ptr=p["arrivals"], group_ptr=gp3,
                            row_bounds_ptr=p["row_bounds"], generated_ptr=p["generated"], flags_ptr=p["flags"]))))
    # as arrival_summary calls it: the bounds that the group sums read lie in the pool, the flags in the engine's own buffer
    own_part = _r256((N_WIN + 1) * 8) + _r256(n * (N_WIN + 1) * 4)
    probes.append(Probe("arrivals-own_scratch", [("arrivals", u64, (3, N_WIN)), ("generated", u32, (n,))],
                        lambda e, p: e.summarize_arrivals(gen_seeds, gen_cols, 3, b.edges, draw_capacity=draw_cap, arrivals_ptr=p["arrivals"], group_ptr=gp3,
                                                          generated_ptr=p["generated"])[1],
                        lambda: {k: arrivals_want()[k] for k in ("arrivals", "generated")},
                        lambda: _assert(fresh("arrivals-own_scratch")[1] == own_part, "the bounds [n, W + 1] do not lie in the pool")))
    pr = b.grid.pairs(b.edge_axis, 0.002, 0.006)
    ia, ib = pr["a"], pr["b"]
    NPR = int(ia.shape[0])
    p_ids = np.where(pr["by"] == 0, 0, 2).astype(np.int64)
    p_ids[[1, 8]] = -1
    t_rows, time_row = b.time_rows(ia)
    times_t = b.arrival_rows(np.stack([arrivals()[s][0] for s in t_rows]))
    pa_t, pb_t, tr_t, pg_t = b.u32(ia), b.u32(ib), b.u32(time_row.reshape(-1)), b.u32(np.where(p_ids < 0, _abi.POOL_SKIP, p_ids))
    p_thr = (0.0, 0.004)
    PB = PAIR_BINNING[2] << PAIR_BINNING[0]

    def pairs_want():
        kw = dict(zip(("sub_bits", "min_exp", "octaves"), PAIR_BINNING))
        per = [R.latency_pairs(b.rows[ia[p]], b.rows[ib[p]], arrivals()[ia[p]][0], b.edges, thresholds=p_thr, **kw) for p in range(NPR)]
        cells = R.latency_pair_cells(per, p_ids, 3)
        five = ("both", "only_a", "only_b", "neither", "nan")
        return {"pair_counts": np.stack([np.stack([x[k] for k in five], axis=-1) for x in per]).astype(np.uint32),
                "pair_sums": np.stack([np.stack([x["sum_d"], x["sum_a"]], axis=-1) for x in per]),
                "unmatched": np.array([[x["unmatched_a"], x["unmatched_b"]] for x in per], dtype=np.uint32),
                "cell_counts": np.stack([cells[k] for k in five + ("slower", "faster", "equal")], axis=-1).astype(np.uint64),
                "above": cells["above"].astype(np.uint64), "extremes": np.stack([cells["min_d"], cells["max_d"]], axis=-1),
                "hist": np.stack([cells["hist_pos"], cells["hist_neg"]], axis=2).astype(np.uint32),
                "tails": np.stack([cells[k] for k in ("under_pos", "under_neg", "over_pos", "over_neg")], axis=-1).astype(np.uint32)}
    pr_keys = ("pair_counts", "pair_sums", "unmatched", "cell_counts", "above", "extremes", "hist", "tails")

    def pairs_call(e, p, thresholds=p_thr):
        return e.summarize_pairs(n, NPR, 3, pair_a_ptr=pa_t.data_ptr(), pair_b_ptr=pb_t.data_ptr(), times_ptr=times_t.data_ptr(), time_row_ptr=tr_t.data_ptr(),
                                 n_time_rows=int(t_rows.shape[0]), draw_capacity=draw_cap, **{f"{k}_ptr": p[k] for k in pr_keys}, group_ptr=pg_t.data_ptr(),
                                 edges=b.edges, thresholds=thresholds, **dict(zip(("sub_bits", "min_exp", "octaves"), PAIR_BINNING)), **b.clock_kw)[1]
    probes.append(Probe("pairs", [("pair_counts", u32, (NPR, N_WIN, 5)), ("pair_sums", f64, (NPR, N_WIN, 2)), ("unmatched", u32, (NPR, 2)),
                                  ("cell_counts", u64, (C_EX, 8)), ("above", u64, (C_EX, len(p_thr))), ("extremes", f64, (C_EX, 2)), ("hist", u32, (C_EX, 2, PB)),
                                  ("tails", u32, (C_EX, 4))],
                        pairs_call, pairs_want,
                        refused=lambda e, p: _raises_invalid(lambda: e.summarize_pairs(
                            n, NPR, 3, pair_a_ptr=pa_t.data_ptr(), pair_b_ptr=pb_t.data_ptr(), times_ptr=times_t.data_ptr(), time_row_ptr=tr_t.data_ptr(),
                            n_time_rows=0, draw_capacity=draw_cap, **{f"{k}_ptr": p[k] for k in pr_keys}, group_ptr=pg_t.data_ptr(), edges=b.edges,
                            thresholds=p_thr, **dict(zip(("sub_bits", "min_exp", "octaves"), PAIR_BINNING)), **b.clock_kw))))

    # ---- the per-scenario summary, of a finished run and in one call with the run
    T = int(b.plan.total_time)
    s_outs = [("stats", f64, (n, 8)), ("rps", np.float32, (n, T)), ("hist", u32, (n, HIST_BINS)), ("series_mean", f64, (n, S)), ("series_max", u32, (n, S))]

    def summary_want():
        mm = [ao.series_mean_max(b.words[s], b.plan.n_edges) for s in range(n)]
        return {"stats": np.stack([ao.latency_stats(r) for r in b.rows]), "rps": np.stack([ao.throughput_series(r, T)[1] for r in b.rows]).astype(np.float32),
                "hist": np.stack([ao.latency_histogram(r, HIST_BINS, HIST_MAX) for r in b.rows]).astype(np.uint32),
                "series_mean": np.stack([m for m, _ in mm]), "series_max": np.stack([x for _, x in mm]).astype(np.uint32)}
    summary_want = cached(summary_want)

    def summ_kw(p):
        return {"stats_ptr": p["stats"], "rps_ptr": p["rps"], "rps_buckets": T, "hist_ptr": p["hist"], "hist_bins": HIST_BINS, "hist_max": HIST_MAX,
                "series_mean_ptr": p["series_mean"], "series_max_ptr": p["series_max"]}
    probes.append(Probe("summarize", s_outs,
                        lambda e, p: _unreported(e.summarize(n, samples_ptr=b.samples_t.data_ptr(), tick_capacity=b.tick_cap, **summ_kw(p), **b.clock_kw)),
                        summary_want, uses_pool=False,
                        refused=lambda e, p: _raises_invalid(lambda: e.summarize(0, samples_ptr=b.samples_t.data_ptr(), tick_capacity=b.tick_cap, **summ_kw(p), **b.clock_kw))))

    def run_summarized(e, p):
        counts = b.torch.zeros_like(b.counts_t)                   # (a run adds to its counts)
        run_clock, run_samples = b.run_buffers()
        b.torch.cuda.synchronize(b.dev)
        e.run(b.res.seeds, b.run_cols, clock_ptr=run_clock.data_ptr(), clock_capacity=b.cap, samples_ptr=run_samples.data_ptr(),
              tick_capacity=b.tick_cap, counts_ptr=counts.data_ptr(), draw_capacity=b.run_draw_capacity, summary=summ_kw(p))
        b.torch.cuda.synchronize(b.dev)
        assert b.torch.equal(counts, b.counts_t), "the run of af_engine_run_summarized counted something else than the batch's run"
        return None
    probes.append(Probe("run_summarized", s_outs, run_summarized, summary_want, uses_pool=False))
    return probes


def _unreported(_result: Any) -> None:
    """The scratch size of an entry point that reports none."""
    return None


def _assert(cond: bool, what: str) -> None:
    assert cond, what


def _raises_invalid(call: Callable[[], Any]) -> int:
    """The return code of a call the library must refuse (the methods of Engine raise EngineError with the code in its text)."""
    from asyncflow_amd.engine import EngineError

    with pytest.raises(EngineError, match=rf"failed \({_abi.AF_ERR_INVALID}\)"):
        call()
    return _abi.AF_ERR_INVALID


def _quantiles_refused(b: Batch, e: Any, p: dict[str, int], n_groups: int, gp: int, by: str, edges: Any) -> int:
    """A NaN threshold, which Engine.summarize_quantiles checks itself: through the C ABI."""
    name = "af_engine_summarize_arrival_quantiles" if by == "arrival" else "af_engine_summarize_quantiles"
    pd = C.POINTER(C.c_double)
    q, th = np.asarray(LEVELS, dtype=np.float64), np.array([0.02, float("nan")])
    ed = None if edges is None else np.ascontiguousarray(edges, dtype=np.float64)
    out = _abi.AfOutputs(b.cap, C.c_void_p(b.clock_t.data_ptr()), 0, None, C.c_void_p(b.counts_t.data_ptr()))
    req = _abi.AfQuantiles(b.n, n_groups, 0 if ed is None else ed.shape[0] - 1, C.c_void_p(gp), None if ed is None else ed.ctypes.data_as(pd),
                           q.shape[0], q.ctypes.data_as(pd), 2, th.ctypes.data_as(pd), C.c_void_p(p["count"]), C.c_void_p(p["quantiles"]),
                           C.c_void_p(p["within"]), 0.0, 0)
    return getattr(e._lib, name)(e._h, C.byref(out), C.byref(req))  # noqa: SLF001


def _host_arrivals(b: Batch, cap: int) -> list[tuple[np.ndarray, int]]:
    """results.arrival_times of every scenario: the host definition of the arrival rows."""
    from oracle.rng_adapter import GeneratorRNG

    users = np.asarray(b.res.overrides[USERS], dtype=np.float64)
    p = b.plan
    return [R.arrival_times(GeneratorRNG(int(b.res.seeds[s])), p.gen_users_dist, float(users[s]), p.gen_users_sigma, p.gen_rpm_mean, p.gen_window_s,
                            p.total_time, cap) for s in range(b.n)]


# ---- running a probe ---------------------------------------------------------------------------------------------------------------
_STATE: dict[str, Any] = {}


def batch() -> Batch:
    if "batch" not in _STATE:
        _STATE["batch"] = Batch()
        _STATE["probes"] = {p.name: p for p in build_probes(_STATE["batch"])}
    return _STATE["batch"]


def probes() -> dict[str, Probe]:
    batch()
    return _STATE["probes"]


def _names() -> list[str]:
    """The ids of the table (without a device: the names alone)."""
    tags = ("one_group", "three_groups")
    lat = [f"{k}-{t}" for t in tags for k in ("pooled", "windows", "quantiles", "arrival_windows", "arrival_quantiles", "state_windows", "state_quantiles")]
    return lat + ["series_quantiles-one_group", "series_windows-three_groups", "series_windows-singletons", "series_excursions", "series_histogram",
                  "series_combined", "series_joint", "series_warmup", "inflight", "exemplars", "latency_histogram", "alerts", "arrivals", "arrivals-own_scratch", "pairs", "summarize",
                  "run_summarized"]


NAMES = _names()


def run(eng: Any, p: Probe, refused: bool = False) -> tuple[dict[str, np.ndarray], int | None]:
    """One call with every output between sentinel words: the outputs as uint32 words and what the call says of the scratch."""
    b = batch()
    off, total = p.layout()
    buf = b.torch.full((total,), SENTINEL, dtype=b.torch.int32, device=b.dev)
    ptrs = {k: buf.data_ptr() + 4 * o for k, (o, _) in off.items()}
    b.torch.cuda.synchronize(b.dev)
    if refused:
        assert p.refused(eng, ptrs) == _abi.AF_ERR_INVALID
        scratch = None
    else:
        scratch = p.call(eng, ptrs)
    b.torch.cuda.synchronize(b.dev)
    words = buf.cpu().numpy().view(np.uint32)
    inside = np.zeros(total, dtype=bool)
    out = {}
    for k, (o, size) in off.items():
        inside[o:o + size] = True
        out[k] = words[o:o + size].copy()
    assert (words[~inside] == SENTINEL).all(), f"{p.name}: a word outside the outputs changed"
    if refused:
        assert (words == SENTINEL).all(), f"{p.name}: a refused call wrote an output word"
    return out, scratch


def pool_size(eng: Any) -> int:
    """The pool's size as a call that needs next to none of it reports it (the pooled analyzer reports none itself)."""
    b = batch()
    out = b.torch.empty(64, dtype=b.torch.float64, device=b.dev)
    return eng.summarize_series_windows(1, 1, [0, 1], count_ptr=out.data_ptr(), mean_ptr=out.data_ptr() + 64, **b.series_kw)[1]


def fresh(name: str) -> tuple[dict[str, np.ndarray], int]:
    """(a), once per probe: the probe as the first call of a new engine; its words and S, the bytes of scratch it needs."""
    p = probes()[name]
    if "fresh" not in p.cache:
        eng = batch().engine()
        try:
            out, scratch = run(eng, p)
            if p.uses_pool and scratch is None:
                scratch = pool_size(eng)
                tiny = batch().engine()
                try:
                    assert pool_size(tiny) < scratch, "the call that reads the pool's size grew the pool"
                finally:
                    tiny.close()
            p.cache["fresh"] = (out, scratch or 0)
        finally:
            eng.close()
    return p.cache["fresh"]


def same_words(got: dict[str, np.ndarray], want: dict[str, np.ndarray], what: str) -> None:
    for k, v in want.items():
        bad = np.flatnonzero(got[k] != v)
        assert bad.size == 0, (what, k, f"{bad.size} of {v.size} words differ, the first at {bad[:6].tolist()}: {got[k][bad[:6]].tolist()} for {v[bad[:6]].tolist()}")


def scratch_after(eng: Any, p: Probe, scratch: int | None) -> int | None:
    if not p.uses_pool:
        return None
    return pool_size(eng) if scratch is None else scratch


def equals_host(name: str, p: Probe, got: dict[str, np.ndarray]) -> None:
    """Every output word of a call against the probe's host definition: floats by bit pattern, NaN in the same places."""
    want = p.host()
    assert set(want) == {k for k, _, _ in p.outs}
    for k, dt, shape in p.outs:
        w = np.ascontiguousarray(np.asarray(want[k]).reshape(shape))
        g = got[k].view(dt).reshape(shape)
        if np.dtype(dt).kind == "f":
            w = w.astype(dt)
            nan = np.isnan(w)
            assert np.array_equal(np.isnan(g), nan), (name, k, "NaN in other places")
            bits = {4: np.uint32, 8: np.uint64}[np.dtype(dt).itemsize]
            bad = np.argwhere((g.view(bits) != w.view(bits)) & ~nan)
            assert bad.shape[0] == 0, (name, k, bad[:5].tolist(), [float(g[tuple(t)]) for t in bad[:5]], [float(w[tuple(t)]) for t in bad[:5]])
        else:
            w = w.astype(np.uint64)
            assert (w <= np.iinfo(dt).max).all()
            bad = np.argwhere(g.astype(np.uint64) != w)
            assert bad.shape[0] == 0, (name, k, bad[:5].tolist(), [int(g[tuple(t)]) for t in bad[:5]], [int(w[tuple(t)]) for t in bad[:5]])


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_fresh_engine_equals_the_host_definition(name):
    p = probes()[name]
    p.path()                                                      # the scratch-heavy path, from the cell sizes of the batch
    got, scratch = fresh(name)
    equals_host(name, p, got)
    if p.uses_pool:
        assert scratch > 0
    if p.first_part:
        assert scratch >= 8 * p.first_part, (name, scratch, p.first_part)


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("word", WORDS, ids=[f"{w:08X}" for w in WORDS])
@pytest.mark.parametrize("name", NAMES)
def test_roomy_poisoned_scratch(name, word):
    p = probes()[name]
    want, S = fresh(name)
    room = 2 * S + 4096
    eng = batch().engine()
    try:
        eng.probe_scratch(room, word)
        got, scratch = run(eng, p)
        same_words(got, want, f"{name} on a pool of 0x{word:08X}")
        if p.uses_pool:
            assert scratch_after(eng, p, scratch) == room
    finally:
        eng.close()


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_growth_at_every_point_poisoned(name):
    p = probes()[name]
    want, S = fresh(name)
    caps = [0, 256, (S // 2) & ~255, max(S - 256, 0)]
    if p.first_part:                                              # the scratch moves in the middle of the call
        assert S >= 8 * p.first_part and p.first_part <= caps[2] < S, (name, S, p.first_part)
    for cap in caps:
        eng = batch().engine()
        try:
            eng.probe_scratch(cap, 0xFFFFFFFF)
            got, scratch = run(eng, p)
            same_words(got, want, f"{name} from a pool of {cap} bytes")
            if p.uses_pool:
                assert scratch_after(eng, p, scratch) == S, (name, cap)
        finally:
            eng.close()


# ---- (d) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("before", NAMES)
def test_after_every_other_analyzer(before):
    y = probes()[before]
    eng = batch().engine()
    try:
        for name in NAMES:
            run(eng, y)
            got, _ = run(eng, probes()[name])
            same_words(got, fresh(name)[0], f"{name} after {before}")
    finally:
        eng.close()


# ---- (e) ---------------------------------------------------------------------------------------------------------------------------
def _sweep_run(eng: Any, rows: slice) -> dict[str, np.ndarray]:
    """af_engine_run of the batch's sweep (of its scenarios `rows`): the counts, and the clock and sample rows that they count."""
    b = batch()
    t = b.torch
    seeds = np.ascontiguousarray(b.res.seeds[rows])
    n = seeds.shape[0]
    cols = [(c, i, np.ascontiguousarray(v[rows])) for c, i, v in b.run_cols]
    counts = t.zeros((n, _abi.CNT_SLOTS), dtype=t.int32, device=b.dev)
    clock = t.full((n, b.cap, 2), -1.0, dtype=t.float64, device=b.dev)
    samples = t.zeros((n, b.tick_cap, b.plan.series_pitch), dtype=t.int32, device=b.dev)
    t.cuda.synchronize(b.dev)
    eng.run(seeds, cols, clock_ptr=clock.data_ptr(), clock_capacity=b.cap, samples_ptr=samples.data_ptr(), tick_capacity=b.tick_cap,
            counts_ptr=counts.data_ptr(), draw_capacity=b.cap)
    t.cuda.synchronize(b.dev)
    return {"counts": counts.cpu().numpy().view(np.uint32), "clock": clock.cpu().numpy().view(np.uint64), "samples": samples.cpu().numpy().view(np.uint32)}


def test_run_and_arrivals_share_their_buffers():
    """d_arr and d_arr_flags: the probe without a flags output writes the engine's own flags, as a run does."""
    b = batch()
    both = [(probes()[k], fresh(k)[0]) for k in ("arrivals-own_scratch", "arrivals")]
    eng = b.engine()
    try:
        for p, want in both:
            same_words(run(eng, p)[0], want, f"{p.name} before any run")
        first = _sweep_run(eng, slice(None))
        for p, want in both:
            same_words(run(eng, p)[0], want, f"{p.name} after a run")
        second = _sweep_run(eng, slice(None))
        for k in first:
            assert np.array_equal(first[k], second[k]), f"{k} of a run after summarize_arrivals differ from the run before it"
        same_words(run(eng, both[0][0])[0], both[0][1], "arrivals-own_scratch between two runs")
        third = _sweep_run(eng, slice(None))
        for k in first:
            assert np.array_equal(first[k], third[k]), f"{k} of a run after summarize_arrivals with the engine's own flags differ"
        _sweep_run(eng, slice(0, b.n // 2))
        for p, want in both:
            same_words(run(eng, p)[0], want, f"{p.name} after a run of half the scenarios")
    finally:
        eng.close()


# ---- (f) ---------------------------------------------------------------------------------------------------------------------------
def _api_calls(b: Batch) -> list[tuple[str, Callable[[Any], dict]]]:
    """Every *_summary method of a results object in the README's order."""
    g, te = b.grid, b.tick_edges
    names = b.res.series_names()
    ready, io, ram = names[b.col_ready], names[b.col_io], names[b.col_ram]
    pr = g.pairs(b.edge_axis, 0.002, 0.006)
    look = int(round(1.0 / b.period))
    return [
        ("summary", lambda r: r.summary(rps=True, hist_bins=HIST_BINS, hist_max=HIST_MAX, series=True)),
        ("pooled_summary", lambda r: r.pooled_summary(g)),
        ("window_summary", lambda r: r.window_summary(edges=b.edges, by=g, row_bounds=True)),
        ("window_summary-arrival", lambda r: r.window_summary(edges=b.edges, by=g, window_of="arrival")),
        ("arrival_summary", lambda r: r.arrival_summary(edges=b.edges, by=g, thresholds=SLO_THR)),
        ("in_flight_summary", lambda r: r.in_flight_summary(tick_edges=te, by=g, threshold=3, bins=12)),
        ("exemplar_summary", lambda r: r.exemplar_summary(64, edges=b.edges, by=g, with_state=True)),
        ("latency_histogram_summary", lambda r: r.latency_histogram_summary(edges=b.edges, by=g, window_of="arrival")),
        ("paired_summary", lambda r: r.paired_summary(pr["a"], pr["b"], edges=b.edges, by=pr["by"], thresholds=[0.0, 0.004])),
        ("alert_summary", lambda r: r.alert_summary(0.05, [(look, look, 1, 5, 1, 1), (5 * look, look, 1, 8, 5, 2)], tick_edges=te, by=g, delay_bins=8,
                                                    delay_width_s=4 * b.period, per_tick=True)),
        ("state_summary", lambda r: r.state_summary(ready, STATE_BINS, edges=b.edges, by=g)),
        ("state_quantile_summary", lambda r: r.state_quantile_summary(ready, LEVELS, thresholds=SLO_THR, bins=STATE_BINS, by=None)),
        ("series_window_summary", lambda r: r.series_window_summary(tick_edges=te, by=g)),
        ("series_quantile_summary", lambda r: r.series_quantile_summary(SERIES_LEVELS, tick_edges=b.tick_whole, by=None, series=[io, ram])),
        ("series_excursion_summary", lambda r: r.series_excursion_summary({ready: 0.5}, tick_edges=te)),
        ("series_histogram_summary", lambda r: r.series_histogram_summary(16, tick_edges=te, by=g)),
        ("series_combined_summary", lambda r: r.series_combined_summary({"queued": ("sum", "*:ready_queue_len"), "imbalance": ("spread", "*:ready_queue_len")},
                                                                        tick_edges=te, by=g, bins=8)),
        ("series_joint_summary", lambda r: r.series_joint_summary({"queues": (ready, io, 2)}, tick_edges=te, by=g)),
        ("series_autocorrelation_summary", lambda r: r.series_autocorrelation_summary([ready, io], 40, tick_edges=te, by=g)),
        ("series_warmup_summary", lambda r: r.series_warmup_summary(5, tick_edges=te, by=g, series=[io, ready])),
        ("quantile_summary", lambda r: r.quantile_summary(LEVELS, thresholds=SLO_THR, by=None)),
        ("quantile_summary-arrival", lambda r: r.quantile_summary(LEVELS, thresholds=SLO_THR, edges=b.edges, by=g, window_of="arrival")),
    ]


def _arrays(d: dict) -> dict[str, np.ndarray]:
    out = {}
    for k, v in d.items():
        if k.endswith("_ms") or k == "scratch_bytes":
            continue
        if hasattr(v, "cpu"):
            out[k] = v.cpu().numpy().copy()
        elif isinstance(v, np.ndarray):                          # (the exact sums too: object arrays of Python integers)
            out[k] = v.copy()
    return out


def _same_arrays(a: dict[str, np.ndarray], c: dict[str, np.ndarray], what: str) -> None:
    assert set(a) == set(c), what
    for k, v in a.items():
        assert v.dtype == c[k].dtype and np.array_equal(v, c[k], equal_nan=v.dtype.kind == "f"), (what, k)


def test_every_summary_through_the_python_api_in_both_orders():
    b = batch()
    res, calls = b.res, _api_calls(b)
    res.close()
    forward = {k: _arrays(fn(res)) for k, fn in calls}
    backward = {k: _arrays(fn(res)) for k, fn in reversed(calls)}
    alone = {}
    for k, fn in calls:
        res.close()                                               # (its _summ_engine is None again)
        assert res._summ_engine is None  # noqa: SLF001
        alone[k] = _arrays(fn(res))
    res.close()
    for k, _ in calls:
        assert forward[k], k
        _same_arrays(forward[k], backward[k], f"{k}: README order and the reverse")
        _same_arrays(forward[k], alone[k], f"{k}: a shared engine and one of its own")


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_probe_scratch_is_refused_on_a_plan_only_engine():
    from asyncflow_amd.engine import PLAN_ONLY, Engine

    b = batch()
    eng = Engine(b.plan, PLAN_ONLY)
    try:
        assert eng._lib.af_probe_scratch(eng._h, 4096, 0xFFFFFFFF) == _abi.AF_ERR_NO_DEVICE  # noqa: SLF001
    finally:
        eng.close()


REFUSED = [n for n in NAMES if n.endswith("three_groups") or "-" not in n]


@pytest.mark.parametrize("name", [n for n in REFUSED if n not in ("run_summarized", "state_quantiles-three_groups")])
def test_a_refused_call_on_a_poisoned_engine_leaves_every_output_word_alone(name):
    p = probes()[name]
    assert p.refused is not None
    want, S = fresh(name)
    eng = batch().engine()
    try:
        eng.probe_scratch(S // 2 & ~255, 0xFFFFFFFF)
        run(eng, p, refused=True)
        same_words(run(eng, p)[0], want, f"{name} after a refused call")
    finally:
        eng.close()


def test_the_table_names_every_entry_point():
    called = {"af_engine_summarize", "af_engine_run_summarized"} | {s for s in _abi.EXPORTED_SYMBOLS if s.startswith("af_engine_summarize_")}
    covered = {n.split("-")[0] for n in NAMES}
    assert {"af_engine_" + (k if k in ("summarize", "run_summarized") else "summarize_" + k) for k in covered} == called
    assert set(probes()) == set(NAMES)
