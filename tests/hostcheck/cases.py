"""Case and result files of the sanitized stand-alone program (sancheck_main.cpp), and the same case through the -O2 library.

A case is ONE run of hc_simulate, hc_flow_simulate or hc_arrivals: the lowered plan, the seed, the override triples, the
mode with its knobs and every capacity.  `write_case` serialises it into a flat file of 8-byte little-endian words (scalars
one word each -- integers as int64, reals as f64 --, arrays as a length word and one word per element); `read_result` reads
what the program wrote; `run_library` runs the same case through tests/hostcheck/libaf_hostcheck.so with buffers of the
same sizes and returns the same structure, so that the two can be compared word for word.  Data only: no program text.
"""

from __future__ import annotations

import ctypes as C
import struct
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

from asyncflow_amd import _abi
from asyncflow_amd.plan import DevicePlan
from tests.hostcheck import build as hc

MAGIC = int.from_bytes(b"ASAFCAS1", "little")
NEXT_EVENT, FLOW, ARRIVALS = 0, 1, 2
# what Result.variant means for a next-event case (hostcheck.cpp: g_sim_variant)
SIM_LEAN, SIM_SIMPY_ORDER, SIM_TWO_PASS_RERUN = 0, 1, 2


@dataclass
class Case:
    mode: int
    seed: int = 0
    plan: DevicePlan | None = None                      # (an arrivals case has none)
    overrides: list[tuple[str, int, float]] = field(default_factory=list)
    two_pass: bool = False                              # next-event lane: lean first, SimPy-order rerun on demand
    ipl: int = 1                                        # flow kernel
    ring_rows: int = 64
    robust: bool = False
    far: bool = True
    compact: bool = False                               # general servers: the compact first launch, not the second chance
    long_list_entries: int = 256
    long_list: int | None = None
    cap: int = 4096                                     # next-event lane: live requests, waiters per queue
    fcap: int = 4096
    clock_capacity: int | None = None                   # None: plan.clock_capacity()
    draw_capacity: int | None = None                    # None: plan.clock_capacity()
    tick_cap: int | None = None                         # None: the plan's tick count
    samples: bool = True
    hist_bins: int = 0                                  # online histogram / RPS (0: off)
    hist_max: float = 1.0
    rps_buckets: int = 0
    quantum_bits: int = 0
    which: int = 0                                      # arrivals: 0 sequential, 1 / 2 per-lane sampler
    dist: int = 0
    mean: float = 0.0
    sigma: float = 0.0
    rpm: float = 0.0
    window_s: float = 1.0
    horizon: float = 1.0
    n_draw: int = 0

    def caps(self) -> tuple[int, int, int]:
        """(clock_capacity, draw_capacity, tick_cap) with the defaults filled in"""
        if self.plan is None:
            return 0, 0, 0
        full = int(self.plan.clock_capacity())
        return (full if self.clock_capacity is None else self.clock_capacity,
                full if self.draw_capacity is None else self.draw_capacity,
                max(self.plan.tick_count, 1) if self.tick_cap is None else self.tick_cap)


@dataclass
class Result:
    rc: int
    variant: int            # flow: dispatch id (hc_flow_variant); next-event: SIM_*; arrivals: which
    arr_n: int
    arr_flags: int
    counts: np.ndarray      # u32 [CNT_SLOTS]
    clock: np.ndarray       # f64 [2 * clock_capacity]
    samples: np.ndarray     # u32 [tick_cap * pitch] (empty: samples off)
    hist: np.ndarray        # u32 [hist_bins]
    rps: np.ndarray         # u32 [rps_buckets]
    arrivals: np.ndarray    # f64 [n_draw]

    def words(self) -> dict[str, np.ndarray]:
        """every output as integer words (clock rows and arrival times by bit pattern)"""
        return {"head": np.asarray([self.rc, self.variant, self.arr_n, self.arr_flags], dtype=np.int64), "counts": self.counts,
                "clock": self.clock.view(np.uint64), "samples": self.samples, "hist": self.hist, "rps": self.rps,
                "arrivals": self.arrivals.view(np.uint64)}


_EMPTY_PLAN_ARRAYS = 21


def _ints(values) -> bytes:
    a = np.asarray(values, dtype=np.int64).ravel()
    return struct.pack("<q", a.size) + a.astype("<i8").tobytes()


def _reals(values) -> bytes:
    a = np.asarray(values, dtype=np.float64).ravel()
    return struct.pack("<q", a.size) + a.astype("<f8").tobytes()


def write_case(path: Path, case: Case) -> None:
    i = lambda v: struct.pack("<q", int(v))  # noqa: E731
    d = lambda v: struct.pack("<d", float(v))  # noqa: E731
    out = [struct.pack("<Q", MAGIC), i(case.mode)]
    p = case.plan
    if p is None:
        out += [d(0.0), d(0.0), i(0), i(0), d(0.0), d(0.0), d(0.0), d(0.0), i(-1), i(0), i(0), i(-1), i(0), i(0)]
        out += [_ints([])] * _EMPTY_PLAN_ARRAYS
    else:
        out += [d(p.total_time), d(p.sample_period), i(p.metrics_mask), i(p.gen_users_dist), d(p.gen_users_mean), d(p.gen_users_sigma),
                d(p.gen_rpm_mean), d(p.gen_window_s), i(p.gen_out_edge), i(p.n_edges), i(p.n_servers), i(p.client_out_edge),
                i(int(p.has_lb)), i(p.lb_algo)]
        out += [_ints(p.lb_edges), _ints(p.edge_target_kind), _ints(p.edge_target_idx), _ints(p.edge_dist), _reals(p.edge_mean),
                _reals(p.edge_sigma), _reals(p.edge_dropout), _ints(p.srv_cores), _reals(p.srv_ram_mb), _ints(p.srv_out_edge),
                _ints(p.srv_ep_begin), _ints(p.ep_step_begin), _reals(p.ep_ram), _ints(p.step_kind), _reals(p.step_time),
                _reals(p.emark_time), _ints(p.emark_edge), _reals(p.emark_delta), _reals(p.smark_time), _ints(p.smark_lb_edge),
                _ints(p.smark_down)]
    ccap, dcap, tcap = case.caps()
    out += [struct.pack("<Q", case.seed & (2**64 - 1)),
            _ints([_abi.PARAM_CODES[o[0]] for o in case.overrides]), _ints([o[1] for o in case.overrides]),
            _reals([o[2] for o in case.overrides]),
            i(case.two_pass), i(case.ipl), i(case.ring_rows), i(case.robust), i(case.far), i(case.compact), i(case.long_list_entries),
            i(-1 if case.long_list is None else case.long_list), i(case.cap), i(case.fcap), i(ccap), i(dcap), i(tcap),
            i(case.samples), i(case.hist_bins), d(case.hist_max), i(case.rps_buckets), i(case.quantum_bits),
            i(case.which), i(case.dist), d(case.mean), d(case.sigma), d(case.rpm), d(case.window_s), d(case.horizon), i(case.n_draw)]
    Path(path).write_bytes(b"".join(out))


def read_result(path: Path) -> Result:
    data = Path(path).read_bytes()
    rc, variant, arr_n, arr_flags = struct.unpack_from("<qqqq", data, 0)
    at = 32
    arrays = []
    for dtype in ("<u4", "<f8", "<u4", "<u4", "<u4", "<f8"):
        (n,) = struct.unpack_from("<q", data, at)
        at += 8
        arrays.append(np.frombuffer(data, dtype=dtype, count=n, offset=at).copy())
        at += n * np.dtype(dtype).itemsize
    assert at == len(data), (at, len(data))
    return Result(rc, variant, arr_n, arr_flags, *arrays)


def run_library(case: Case) -> Result:
    """The same case through the -O2 library, with output buffers of the same sizes."""
    L = hc.lib()
    u32p, f64p = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    empty_u, empty_d = np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.float64)
    if case.mode == ARRIVALS:
        out = np.zeros(case.n_draw, dtype=np.float64)
        flags = C.c_uint32(0)
        L.hc_set_test_quantum(case.quantum_bits)
        try:
            n = L.hc_arrivals(case.which, C.c_uint64(case.seed), case.dist, case.mean, case.sigma, case.rpm, case.window_s,
                              case.horizon, case.n_draw, out.ctypes.data_as(f64p), C.byref(flags))
        finally:
            L.hc_set_test_quantum(0)
        return Result(0, case.which, int(n), int(flags.value), np.zeros(_abi.CNT_SLOTS, dtype=np.uint32), empty_d, empty_u, empty_u,
                      empty_u, out)
    plan = case.plan
    cplan = plan.as_ctypes()
    params = np.asarray([_abi.PARAM_CODES[o[0]] for o in case.overrides], dtype=np.uint32)
    idxs = np.asarray([o[1] for o in case.overrides], dtype=np.uint32)
    vals = np.asarray([o[2] for o in case.overrides], dtype=np.float64)
    ccap, dcap, tcap = case.caps()
    clock = np.zeros(2 * ccap, dtype=np.float64)
    samples = np.zeros(tcap * plan.series_pitch if case.samples else 0, dtype=np.uint32)
    counts = np.zeros(_abi.CNT_SLOTS, dtype=np.uint32)
    hist = np.zeros(case.hist_bins, dtype=np.uint32)
    rps = np.zeros(case.rps_buckets, dtype=np.uint32)
    sp = samples.ctypes.data_as(u32p) if case.samples else None
    L.hc_set_test_quantum(case.quantum_bits)
    L.hc_set_two_pass(int(case.two_pass))
    L.hc_set_online(hist.ctypes.data_as(u32p) if case.hist_bins else None, case.hist_bins, case.hist_max,
                    rps.ctypes.data_as(u32p) if case.rps_buckets else None, case.rps_buckets)
    try:
        head = (C.byref(cplan), C.c_uint64(case.seed), len(case.overrides), params.ctypes.data_as(u32p), idxs.ctypes.data_as(u32p),
                vals.ctypes.data_as(f64p))
        if case.mode == NEXT_EVENT:
            rc = L.hc_simulate(*head, case.cap, case.fcap, ccap, clock.ctypes.data_as(f64p), tcap, sp, counts.ctypes.data_as(u32p), dcap)
            variant = L.hc_sim_variant()
        else:
            word = case.ipl | (0 if case.far else 0x200) | (0x400 if case.compact else 0)
            if case.robust:
                word |= 0x100 | (case.long_list_entries << 16) | ((0 if case.long_list is None else case.long_list + 1) << 12)
            rc = L.hc_flow_simulate(*head, word, case.ring_rows, ccap, clock.ctypes.data_as(f64p), tcap, sp,
                                    counts.ctypes.data_as(u32p), dcap)
            variant = L.hc_flow_variant()
    finally:
        L.hc_set_online(None, 0, 1.0, None, 0)
        L.hc_set_two_pass(0)
        L.hc_set_test_quantum(0)
    return Result(int(rc), int(variant), 0, 0, counts, clock, samples, hist, rps, empty_d)
