"""The kernels' host instantiation under AddressSanitizer + UBSan, as a stand-alone program (tests/hostcheck/sancheck_main.cpp).

The bit-exact suites cannot see an access one word past an LDS region (on the GPU the next bytes belong to the neighbouring
wave's plan blob), a store behind a global buffer at its capacity edge (inside ctypes it lands in the allocator's slack), or
a double -> integer conversion out of range (undefined on the host, saturating on gfx950).  Here every case is written to a
data file (tests/hostcheck/cases.py), run through the sanitized program as a child process -- every buffer an allocation of
exactly the size the kernel is told, the LDS block exactly blob + n_words --, and

* the child exits 0 with neither an AddressSanitizer nor a UBSan report;
* every output word equals what the -O2 library returns for the same case (clock rows by bit pattern): -O1 against -O2.

The comparison with the oracle stays in test_hostcheck.py, test_flow_hostcheck.py and test_pregen_hostcheck.py.  The last
tests assert what the cases cover: all 30 Flow<> dispatch branches, both next-event lanes and a two-pass rerun, every
AF_PARAM code, the capacity edges, every hand-back reason.
"""

from __future__ import annotations

import os
import random
import subprocess
from functools import lru_cache

import numpy as np
import pytest

from asyncflow_amd import _abi
from asyncflow_amd.plan import lower
from asyncflow_amd.workloads import (fanout8, lb_two_servers, lb_two_servers_two_endpoints, lb_with_events, single_server,
                                     single_server_with_spike)
from oracle.scenarios import deep_chain, flow_payload, fractional_ram_fuzz, gateway_lb, overload, server_chain, tie_storm, wide_fanout
from tests.hostcheck import build as hc
from tests.hostcheck import cases as cs
from tests.hostcheck.cases import ARRIVALS, FLOW, NEXT_EVENT, Case

_problem = hc.sanitizer_link_problem()
pytestmark = pytest.mark.skipif(_problem is not None, reason=str(_problem))

TIMEOUT_S = 240
POISSON, NORMAL = 0, 1
WHY = {"tie": 1 << 9, "list": 1 << 10, "ring": 1 << 11, "ram": 1 << 12}
# Every AF_PARAM code, on lb_with_events(horizon=10): edges 0 gen -> client, 1 client -> LB, 2 / 3 LB -> servers, 4 / 5 servers -> client.
# The first spike (mark slots 0 / 1) moves to edge 4 with another height and an earlier start; the two outages swap their servers
# (server-mark slots 0 / 1 and 2 / 3); four cores and four times the RAM grow the per-server rings of the stage-parallel kernel.
ALL_OVERRIDES = [("gen_users_mean", 0, 150.0), ("gen_users_sigma", 0, 20.0), ("gen_rpm_mean", 0, 35.0), ("edge_mean", 1, 0.01),
                 ("edge_sigma", 1, 0.5), ("edge_dropout", 2, 0.2), ("step_time", 0, 0.004), ("gen_window", 0, 2.0),
                 ("srv_cores", 0, 4.0), ("srv_ram_mb", 1, 8192.0), ("emark_time", 0, 1.513), ("emark_delta", 0, 0.02),
                 ("emark_delta", 1, -0.02), ("emark_edge", 0, 4.0), ("emark_edge", 1, 4.0), ("smark_time", 0, 2.913),
                 ("smark_lb_edge", 0, 3.0), ("smark_lb_edge", 1, 3.0), ("smark_lb_edge", 2, 2.0), ("smark_lb_edge", 3, 2.0),
                 ("smark_down", 0, 1.0)]


def _single_endpoint(payload: dict) -> dict:
    for s in payload["topology_graph"]["nodes"]["servers"]:
        s["endpoints"] = s["endpoints"][:1]
    return payload


def _least_connections(payload: dict) -> dict:
    payload["topology_graph"]["nodes"]["load_balancer"]["algorithms"] = "least_connection"
    return payload


def _continuous_chain(horizon: int) -> dict:
    p = server_chain("exponential", 0.003, cores=2, horizon=horizon)
    for s in p["topology_graph"]["nodes"]["servers"]:        # (server_chain's dyadic step times are tie makers)
        for st in s["endpoints"][0]["steps"]:
            op = st["step_operation"]
            for k in ("cpu_time", "io_waiting_time"):
                if k in op:
                    op[k] = op[k] * 0.013
    p["rqs_input"]["avg_active_users"]["mean"] = 80
    return p


def _many_ram_slots(horizon: int) -> dict:
    """A saturated server (1 400 requests per second on 1 000 per second of core) whose requests need 1 MB each: 2 048 RAM slots are
    more than the ring of departure times remembers, and soon more requests are inside than it has entries."""
    p = single_server(users=700, rpm=120, horizon=horizon)
    p["topology_graph"]["nodes"]["servers"][0]["endpoints"][0]["steps"][1]["step_operation"]["necessary_ram"] = 1
    return p


@lru_cache(maxsize=None)
def _generated(horizon: int, seed: int) -> int:
    """arrivals of LB-2 over `horizon` s (what draw_capacity is set against)"""
    got = cs.run_library(Case(NEXT_EVENT, seed=seed, plan=lower(lb_two_servers(horizon=horizon))))
    assert not int(got.counts[_abi.CNT_FLAGS]) & _abi.FATAL_FLAGS
    return int(got.counts[_abi.CNT_GENERATED])


@lru_cache(maxsize=None)
def _arrivals_exactly_full() -> int:
    return cs.run_library(Case(ARRIVALS, seed=7, dist=POISSON, mean=50.0, rpm=60.0, window_s=5.0, horizon=30.0, n_draw=4000)).arr_n


def _flow_cases() -> dict[str, Case]:
    lb2, lb2_lc = lower(lb_two_servers(horizon=6)), lower(lb_two_servers(horizon=6, algo="least_connection"))
    events = lower(lb_with_events(users=300, horizon=10, scale=10 / 600))
    gw = dict(users=150, horizon=6)
    c: dict[str, Case] = {}
    # ---- the 30 instantiations: chain x general servers x least connections x second chance, ipl 1 / 2 / 4, lean forms
    gen_lc_chain = lower(gateway_lb(front=1, general=True, algo="least_connection", spike=True, **gw))
    gen_chain = lower(gateway_lb(front=2, general=True, backend=True, **gw))
    lc_chain = lower(gateway_lb(front=1, algo="least_connection", spike=True, **gw))
    chain5 = lower(deep_chain(5, users=150, horizon=6, fan=True))
    chain = lower(_continuous_chain(6))
    gen16_lc = lower(wide_fanout(16, "least_connection", horizon=10, users=40))
    gen = lower(lb_two_servers_two_endpoints(users=400, horizon=6))
    second = dict(robust=True, ring_rows=0, long_list_entries=512)
    c["v00-chain-general-lc-compact"] = Case(FLOW, 5, gen_lc_chain, ipl=1, ring_rows=32, compact=True)
    c["v01-chain-general-lc-second"] = Case(FLOW, 5, gen_lc_chain, **second)
    c["v02-chain-general-compact"] = Case(FLOW, 6, gen_chain, ipl=1, ring_rows=32, compact=True)
    c["v03-chain-general-second"] = Case(FLOW, 6, gen_chain, **second)
    c["v04-chain-lc-second"] = Case(FLOW, 5, lc_chain, **second)
    c["v05-chain-lc-ipl1"] = Case(FLOW, 5, lc_chain, ipl=1, ring_rows=64)
    c["v06-chain-lc-ipl2"] = Case(FLOW, 6, lc_chain, ipl=2, ring_rows=64)
    c["v07-chain-lc-ipl4"] = Case(FLOW, 6, lc_chain, ipl=4, ring_rows=0)
    c["v08-chain5-second"] = Case(FLOW, 3, chain5, **second)
    c["v09-chain-ipl1"] = Case(FLOW, 7, chain, ipl=1, ring_rows=64)
    c["v10-chain5-ipl2"] = Case(FLOW, 3, chain5, ipl=2, ring_rows=64)
    c["v11-chain-ipl4"] = Case(FLOW, 7, chain, ipl=4, ring_rows=0)
    c["v12-general16-lc-compact"] = Case(FLOW, 83, gen16_lc, ipl=1, ring_rows=0, compact=True)
    c["v13-general-compact"] = Case(FLOW, 0x5EED0000, gen, ipl=1, ring_rows=32, compact=True)
    c["v14-general16-lc-second"] = Case(FLOW, 83, gen16_lc, robust=True, ring_rows=0, long_list_entries=1024)
    c["v15-general-second"] = Case(FLOW, 0x5EED0000, gen, robust=True, ring_rows=0)
    c["v16-lc-second"] = Case(FLOW, 5, lb2_lc, **second)
    c["v17-second"] = Case(FLOW, 5, lb2, **second)
    c["v18-lc-ipl1"] = Case(FLOW, 5, lb2_lc, ipl=1, ring_rows=64)
    c["v19-lc-ipl2"] = Case(FLOW, 5, lb2_lc, ipl=2, ring_rows=0)
    c["v20-lc16-ipl4"] = Case(FLOW, 81, lower(_single_endpoint(wide_fanout(16, "least_connection", horizon=10, users=40))), ipl=4,
                              ring_rows=128)
    c["v21-ipl1-near-only"] = Case(FLOW, 5, lb2, ipl=1, ring_rows=64, far=False)
    c["v22-ipl1-lean"] = Case(FLOW, 5, lb2, ipl=1, ring_rows=64)
    c["v23-ipl1-marks"] = Case(FLOW, 42, events, ipl=1, ring_rows=64)
    c["v24-ipl1-online"] = Case(FLOW, 5, lb2, ipl=1, ring_rows=64, hist_bins=128, hist_max=0.5, rps_buckets=6)
    c["v25-ipl2-near-only"] = Case(FLOW, 0, lower(single_server(horizon=10)), ipl=2, ring_rows=64, far=False)
    c["v26-ipl2-lean"] = Case(FLOW, 11, lower(fanout8(horizon=12)), ipl=2, ring_rows=256)
    c["v27-ipl2-marks-spike"] = Case(FLOW, 0x5EED0002, lower(single_server_with_spike(horizon=12, scale=0.02)), ipl=2, ring_rows=64)
    c["v28-ipl2-hbm-ring"] = Case(FLOW, 5, lb2, ipl=2, ring_rows=0)
    c["v29-rr16-ipl4"] = Case(FLOW, 77, lower(_single_endpoint(wide_fanout(16, "round_robin", horizon=10, users=100))), ipl=4,
                              ring_rows=0)
    # ---- overrides: every AF_PARAM code; srv_cores / srv_ram_mb grow the rings of core-release and departure times
    c["ovr-all-ipl1"] = Case(FLOW, 9, events, ipl=1, ring_rows=64, overrides=ALL_OVERRIDES)
    c["ovr-all-second"] = Case(FLOW, 9, events, overrides=ALL_OVERRIDES, **second)
    # ---- capacity edges
    n = _generated(6, 5)
    c["cap-clock"] = Case(FLOW, 5, lb2, ipl=1, ring_rows=64, clock_capacity=10)
    c["cap-clock-second"] = Case(FLOW, 5, lb2, clock_capacity=65, **second)
    c["cap-ticks"] = Case(FLOW, 5, lb2, ipl=2, ring_rows=64, tick_cap=7)
    c["cap-ticks-hbm-ring"] = Case(FLOW, 5, lb2, ipl=2, ring_rows=0, tick_cap=7)
    c["cap-draws-exact"] = Case(FLOW, 5, lb2, ipl=1, ring_rows=64, draw_capacity=n)
    c["cap-draws-one-fewer"] = Case(FLOW, 5, lb2, ipl=1, ring_rows=64, draw_capacity=n - 1)
    c["no-samples"] = Case(FLOW, 5, lb2, ipl=1, ring_rows=64, samples=False)
    c["no-samples-hbm-ring"] = Case(FLOW, 5, lb2, ipl=4, ring_rows=0, samples=False)
    c["online-hbm-ring-one-bin"] = Case(FLOW, 42, events, ipl=2, ring_rows=0, hist_bins=1, hist_max=0.001, rps_buckets=3)
    # ---- hand-backs
    c["back-list"] = Case(FLOW, 11, lower(fanout8(horizon=8)), ipl=1, ring_rows=256)
    c["back-list-short-long-lists"] = Case(FLOW, 11, lower(fanout8(horizon=8)), robust=True, ring_rows=0, long_list_entries=64)
    for which in range(4):
        c[f"back-list-only-list-{which}-long"] = Case(FLOW, 0x5EED0002, lower(single_server_with_spike(heavy=True, horizon=12, scale=0.02)),
                                                      robust=True, ring_rows=0, long_list_entries=1024, long_list=which)
    c["back-ring-near-only"] = Case(FLOW, 11, lower(fanout8(horizon=8)), ipl=2, ring_rows=8, far=False)
    c["back-ring-saturated"] = Case(FLOW, 3, lower(single_server(users=700, rpm=120, horizon=6)), ipl=4, ring_rows=8)
    c["back-ram"] = Case(FLOW, 3, lower(_many_ram_slots(6)), robust=True, ring_rows=0, long_list_entries=1024)
    c["back-tie-quantised"] = Case(FLOW, 1, lower(lb_two_servers(horizon=8)), ipl=2, ring_rows=256, quantum_bits=12,
                                   clock_capacity=4 * lb2.clock_capacity(), draw_capacity=4 * lb2.clock_capacity())
    # ---- special payloads
    c["ties-quantised-second"] = Case(FLOW, 1, lower(lb_two_servers(horizon=8)), robust=True, ring_rows=0, quantum_bits=12,
                                      clock_capacity=4 * lb2.clock_capacity(), draw_capacity=4 * lb2.clock_capacity())
    c["ties-general-storm"] = Case(FLOW, 91, lower(tie_storm(random.Random(7030), horizon=6)), robust=True, ring_rows=0,
                                   long_list_entries=1024)
    c["spike-heavy-long-lists"] = Case(FLOW, 0x5EED0002, lower(single_server_with_spike(heavy=True, horizon=12, scale=0.02)),
                                       robust=True, ring_rows=0, long_list_entries=1024)
    c["outage-lc-second"] = Case(FLOW, 42, lower(_least_connections(lb_with_events(users=300, horizon=10, scale=10 / 600))), **second)
    c["fuzz-feed-forward"] = Case(FLOW, 903, lower(flow_payload(random.Random(31003), horizon=5)), ipl=4, ring_rows=1024)
    return c


def _next_event_cases() -> dict[str, Case]:
    lb2 = lower(lb_two_servers(horizon=6))
    events = lower(lb_with_events(users=300, horizon=10, scale=10 / 600))
    n = _generated(6, 5)
    c: dict[str, Case] = {}
    c["ne-simpy-order"] = Case(NEXT_EVENT, 5, lb2)
    c["ne-lean"] = Case(NEXT_EVENT, 5, lb2, two_pass=True)
    c["ne-two-pass-rerun"] = Case(NEXT_EVENT, 1, lower(lb_two_servers(horizon=8)), two_pass=True, quantum_bits=12, hist_bins=128,
                                  hist_max=0.5, rps_buckets=8, clock_capacity=4 * lb2.clock_capacity(),
                                  draw_capacity=4 * lb2.clock_capacity())
    c["ne-online"] = Case(NEXT_EVENT, 3, lb2, hist_bins=128, hist_max=0.5, rps_buckets=6)
    c["ne-ovr-all"] = Case(NEXT_EVENT, 9, events, overrides=ALL_OVERRIDES)
    c["ne-ovr-all-lean"] = Case(NEXT_EVENT, 9, events, overrides=ALL_OVERRIDES, two_pass=True)
    c["ne-cap-clock"] = Case(NEXT_EVENT, 5, lb2, clock_capacity=10)
    c["ne-cap-ticks"] = Case(NEXT_EVENT, 5, lb2, tick_cap=7)
    c["ne-cap-draws-exact"] = Case(NEXT_EVENT, 5, lb2, draw_capacity=n)
    c["ne-cap-draws-one-fewer"] = Case(NEXT_EVENT, 5, lb2, draw_capacity=n - 1)
    c["ne-cap-pool"] = Case(NEXT_EVENT, 11, lower(fanout8(horizon=6)), cap=16, fcap=4096)      # ~40 messages in flight per edge
    c["ne-cap-fifo"] = Case(NEXT_EVENT, 5, lower(overload(horizon=8)), cap=4096, fcap=8)
    c["ne-cap-pool-fifo-lean"] = Case(NEXT_EVENT, 5, lower(overload(horizon=8)), cap=16, fcap=8, two_pass=True)
    c["ne-no-samples"] = Case(NEXT_EVENT, 5, lb2, samples=False)
    c["ne-ties-quantised"] = Case(NEXT_EVENT, 1, lower(lb_two_servers(horizon=8)), quantum_bits=12,
                                  clock_capacity=4 * lb2.clock_capacity(), draw_capacity=4 * lb2.clock_capacity())
    for k in (0, 3, 7, 12):          # decimal RAM needs: waiting Container.put, every event on the SimPy-order path
        c[f"ne-fractional-ram-{k}"] = Case(NEXT_EVENT, 900 + k, lower(fractional_ram_fuzz(random.Random(424200 + k), horizon=8)),
                                          cap=16384, fcap=16384)
    c["ne-fractional-ram-lean-first"] = Case(NEXT_EVENT, 903, lower(fractional_ram_fuzz(random.Random(424203), horizon=8)),
                                             cap=16384, fcap=16384, two_pass=True)
    c["ne-spike"] = Case(NEXT_EVENT, 0x5EED0002, lower(single_server_with_spike(horizon=12, scale=0.02)))
    c["ne-outage"] = Case(NEXT_EVENT, 42, events)
    c["ne-16-servers-rr"] = Case(NEXT_EVENT, 77, lower(wide_fanout(16, "round_robin", horizon=10, users=100)))
    c["ne-16-servers-lc"] = Case(NEXT_EVENT, 77, lower(wide_fanout(16, "least_connection", horizon=10, users=40)))
    c["ne-chain5"] = Case(NEXT_EVENT, 3, lower(deep_chain(5, users=150, horizon=6, fan=True)))
    c["ne-core-re-entry"] = Case(NEXT_EVENT, 0x5EED0000, lower(lb_two_servers_two_endpoints(users=400, horizon=6)))
    return c


def _arrival_cases() -> dict[str, Case]:
    """the edge cases of tests/test_pregen_hostcheck.py, each through the sequential sampler and both per-lane forms"""
    full = dict(seed=7, dist=POISSON, mean=50.0, sigma=0.0, rpm=60.0, window_s=5.0, horizon=30.0)
    edges = {
        "overflow": dict(full, n_draw=200),
        "exactly-full": dict(full, n_draw=_arrivals_exactly_full()),
        "no-users": dict(seed=3, dist=POISSON, mean=0.0, sigma=0.0, rpm=60.0, window_s=1.0, horizon=20.0, n_draw=64),
        "window-beyond-horizon": dict(seed=11, dist=NORMAL, mean=30.0, sigma=10.0, rpm=30.0, window_s=500.0, horizon=20.0, n_draw=1024),
        "rate-outside-fast-division": dict(seed=13, dist=POISSON, mean=3.0, sigma=0.0, rpm=1e-19 * 60.0, window_s=10.0, horizon=50.0,
                                           n_draw=64),
        "quantised-gaps": dict(seed=1003, dist=POISSON, mean=30.0, sigma=0.0, rpm=60.0, window_s=1.0, horizon=16.0, n_draw=1024,
                               quantum_bits=4),
    }
    return {f"arr-{name}-{which}": Case(ARRIVALS, which=which, **kw) for name, kw in edges.items() for which in (0, 1, 2)}


@lru_cache(maxsize=None)
def all_cases() -> dict[str, Case]:
    return {**_flow_cases(), **_next_event_cases(), **_arrival_cases()}


CASE_NAMES = sorted(all_cases()) if _problem is None else []
_results: dict[str, cs.Result] = {}


@pytest.fixture(scope="module")
def program():
    return hc.build_sanitized()


def _run_program(program, *args):
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}
    return subprocess.run([str(program), *map(str, args)], capture_output=True, text=True, env={**env, **hc.SAN_ENV},
                          timeout=TIMEOUT_S, check=False)


def test_selfcheck_proves_the_instrumentation_is_live(program):
    r = _run_program(program, "--selfcheck")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "word behind the lds block poisoned=1" in r.stdout and "word behind the clock buffer poisoned=1" in r.stdout
    assert "lds last word poisoned=0" in r.stdout and "clock last word poisoned=0" in r.stdout


@pytest.mark.parametrize("name", CASE_NAMES)
def test_sanitized_run_is_clean_and_equals_the_library(program, tmp_path, name):
    case = all_cases()[name]
    cs.write_case(tmp_path / "case.bin", case)
    r = _run_program(program, tmp_path / "case.bin", tmp_path / "result.bin")
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-6000:]
    assert r.returncode == 0, (r.returncode, r.stderr[-6000:])
    got = cs.read_result(tmp_path / "result.bin")
    want = cs.run_library(case)
    for (key, g), w in zip(got.words().items(), want.words().values()):
        assert g.dtype.kind in "iu" and g.shape == w.shape and np.array_equal(g, w), (name, key)
    _results[name] = got


# ---- what the cases cover (from the recorded ids and flags of the runs above) ------------------------------------------
def _need_all_results():
    missing = [n for n in CASE_NAMES if n not in _results]
    if missing:
        pytest.fail(f"{len(missing)} cases did not finish (first: {missing[0]}): coverage cannot be shown")


def _flags(name: str) -> int:
    return int(_results[name].counts[_abi.CNT_FLAGS])


def _why(name: str) -> set[str]:
    f = _flags(name)
    return {k for k, bit in WHY.items() if f & bit} if f & hc.FLOW_FALLBACK else set()


def test_every_dispatch_branch_and_lane_was_taken():
    _need_all_results()
    cases = all_cases()
    flow_ids = {r.variant for n, r in _results.items() if cases[n].mode == FLOW and r.rc == 0}
    assert flow_ids == set(range(30)), sorted(set(range(30)) - flow_ids)
    for k in range(30):                                 # ... and each by the case named for it
        name = next(n for n in CASE_NAMES if n.startswith(f"v{k:02d}-"))
        assert _results[name].variant == k, (name, _results[name].variant)
    assert _results["ne-lean"].variant == cs.SIM_LEAN and _results["ne-simpy-order"].variant == cs.SIM_SIMPY_ORDER
    assert _results["ne-two-pass-rerun"].variant == cs.SIM_TWO_PASS_RERUN
    assert {r.variant for n, r in _results.items() if cases[n].mode == ARRIVALS} == {0, 1, 2}
    # the instantiations ran their scenarios to the end rather than handing them back at once
    stayed = [n for n in CASE_NAMES if n.startswith("v") and not _flags(n) & hc.FLOW_FALLBACK]
    assert len(stayed) >= 26, sorted(set(n for n in CASE_NAMES if n.startswith("v")) - set(stayed))
    for n in stayed:
        assert int(_results[n].counts[_abi.CNT_COMPLETED]) > 100, n


def test_every_override_code_appears():
    cases = all_cases()
    for mode in (FLOW, NEXT_EVENT):
        seen = {o[0] for c in cases.values() if c.mode == mode for o in c.overrides}
        assert seen == set(_abi.PARAM_CODES), set(_abi.PARAM_CODES) - seen
    _need_all_results()
    for name in ("ovr-all-ipl1", "ovr-all-second", "ne-ovr-all", "ne-ovr-all-lean"):
        assert not _flags(name) & (_abi.FATAL_FLAGS | hc.FLOW_FALLBACK), name
        assert int(_results[name].counts[_abi.CNT_MARKS]) > 0 and int(_results[name].counts[_abi.CNT_DROPPED]) > 0, name


def test_capacity_edges_were_reached():
    _need_all_results()
    cases = all_cases()
    for name in ("cap-clock", "cap-clock-second", "ne-cap-clock"):
        assert _flags(name) & _abi.FLAG_CLOCK_OVERFLOW, name
        assert int(_results[name].counts[_abi.CNT_COMPLETED]) > cases[name].clock_capacity
    for name in ("cap-ticks", "cap-ticks-hbm-ring", "ne-cap-ticks"):
        assert int(_results[name].counts[_abi.CNT_TICKS]) > cases[name].tick_cap == 7, name
        assert _results[name].samples.size == 7 * cases[name].plan.series_pitch and _results[name].samples.any(), name
    for name in ("cap-draws-exact", "ne-cap-draws-exact"):
        assert not _flags(name) & _abi.FLAG_DRAW_OVERFLOW and int(_results[name].counts[_abi.CNT_GENERATED]) == cases[name].draw_capacity
    for name in ("cap-draws-one-fewer", "ne-cap-draws-one-fewer"):
        assert _flags(name) & _abi.FLAG_DRAW_OVERFLOW and int(_results[name].counts[_abi.CNT_GENERATED]) == cases[name].draw_capacity
    assert _flags("ne-cap-pool") & _abi.FLAG_POOL_OVERFLOW and _flags("ne-cap-fifo") & _abi.FLAG_FIFO_OVERFLOW
    assert _flags("ne-cap-pool-fifo-lean") & (_abi.FLAG_POOL_OVERFLOW | _abi.FLAG_FIFO_OVERFLOW)
    for name in ("v28-ipl2-hbm-ring", "v19-lc-ipl2", "cap-ticks-hbm-ring"):     # ring_rows = 0: the sample rows are the accumulators
        assert cases[name].ring_rows == 0 and cases[name].samples and _results[name].samples.any(), name
    for name in ("no-samples", "no-samples-hbm-ring", "ne-no-samples"):
        assert _results[name].samples.size == 0 and int(_results[name].counts[_abi.CNT_TICKS]) > 0, name
    for name in ("v24-ipl1-online", "online-hbm-ring-one-bin", "ne-online", "ne-two-pass-rerun"):
        assert int(_results[name].hist.sum()) == int(_results[name].counts[_abi.CNT_COMPLETED]) > 0 and _results[name].rps.any(), name
    assert _results["arr-overflow-1"].arr_flags == _abi.FLAG_DRAW_OVERFLOW and _results["arr-overflow-1"].arr_n == 200
    assert _results["arr-exactly-full-1"].arr_flags == 0 and _results["arr-exactly-full-1"].arr_n == cases["arr-exactly-full-1"].n_draw
    assert _results["arr-no-users-2"].arr_n == 0


def test_every_hand_back_reason_was_seen():
    _need_all_results()
    assert _why("back-list") == {"list"} and "list" in _why("back-list-short-long-lists")
    for which in range(4):          # one list of 1 024 entries, 256 in the others: rate x spike messages do not fit those
        assert _why(f"back-list-only-list-{which}-long") == {"list"}, which
    assert "ring" in _why("back-ring-near-only") and "ring" in _why("back-ring-saturated")
    assert "ram" in _why("back-ram")
    assert "tie" in _why("back-tie-quantised")
    for name in ("spike-heavy-long-lists", "outage-lc-second"):
        assert not _why(name), (name, _why(name))
    # (the second-chance form orders equal delivery times by send time; a tie it cannot order ends the run, after hundreds it could)
    assert _why("ties-quantised-second") <= {"tie"} and int(_results["ties-quantised-second"].counts[_abi.CNT_COMPLETED]) > 100
