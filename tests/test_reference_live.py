"""Differential tests against the reference's own outputs, recorded (oracle/make_reference_live.py).

tests/golden/reference_live/cases.npz holds what the UNMODIFIED reference computed on every case below: counts, every
(start, finish) pair and every sampled series, the exception it raised where it refuses a payload, its validated model of
each example YAML and what its analyzer reports.  The oracle is held to those bit for bit wherever the suite runs;
`python oracle/make_reference_live.py --check` runs the reference again and compares it with the committed file.
"""

from __future__ import annotations

import json
import random

import numpy as np
import pytest

from asyncflow_amd.plan import lower
from oracle import oracle_lib as ol
from oracle.make_reference_live import case_key
from oracle.scenarios import overload, random_payload, server_chain, tie_storm, wide_fanout
from tests.conftest import GOLDEN_DIR

pytestmark = pytest.mark.filterwarnings("ignore::DeprecationWarning")

_RECORDED = np.load(GOLDEN_DIR / "reference_live" / "cases.npz", allow_pickle=False)


def _recorded(payload: dict, seed: int) -> str:
    """The key of (payload, seed) in the recorded file; the payload is held to the recorded input, key by key."""
    key = case_key(payload, seed)
    assert f"{key}.payload_json" in _RECORDED.files, "no recorded reference output for this payload (oracle/make_reference_live.py)"
    assert json.loads(str(_RECORDED[f"{key}.payload_json"])) == json.loads(json.dumps(payload))
    return key


def _same(payload: dict, seed: int) -> None:
    key = _recorded(payload, seed)
    assert f"{key}.raised" not in _RECORDED.files, str(_RECORDED[f"{key}.raised"])
    res = ol.simulate(lower(payload), seed)
    assert tuple(int(v) for v in _RECORDED[f"{key}.counts"]) == (res.generated, res.completed, res.dropped, res.ticks)
    assert np.array_equal(_RECORDED[f"{key}.clock"], res.clock)
    assert np.array_equal(_RECORDED[f"{key}.samples"], res.samples)


@pytest.mark.parametrize("case", range(12))
def test_fuzzed_payloads_match_reference(case):
    rng = random.Random(1000 + case)
    _same(random_payload(rng, horizon=8), 500 + case)


def test_exact_timestamp_ties_follow_simpy_interleaving():
    """Deterministic step times under queueing give EXACT ties; SimPy then runs the
    zero-time steps of the tied cascades breadth-first (eid order)."""
    payload = overload(horizon=12)
    res = ol.simulate(lower(payload), 5)
    assert res.ties > 0
    _same(payload, 5)


@pytest.mark.parametrize("case", range(30))
def test_tie_storms_match_reference(case):
    """Payloads built so that thousands of timed events share an instant (grant bursts, integer
    edge latencies incl. zero, ticks on timeline marks)."""
    _same(tie_storm(random.Random(777000 + case), horizon=12), 5 + case)


@pytest.mark.parametrize(("n_srv", "algo"), [(9, "round_robin"), (20, "least_connection")])
def test_wide_fanout_matches_reference(n_srv, algo):
    _same(wide_fanout(n_srv, algo), 1)


@pytest.mark.parametrize(("dist", "mean"), [("exponential", 0.003), ("poisson", 0.7), ("normal", 0.001)])
def test_server_chain_matches_reference(dist, mean):
    _same(server_chain(dist, mean), 2)


def test_baseline_workloads_equal_the_reference_yaml():
    """asyncflow_amd/workloads.py restates the reference's example YAMLs value for value: ours, normalized with every
    default applied, equal the reference's own validated model of each YAML (recorded as dumped by its Pydantic models)."""
    from asyncflow_amd import workloads as w
    from asyncflow_amd.payload import normalize_payload

    theirs_all = json.loads(str(_RECORDED["yaml_models"]))
    cases = {
        "single_server.yml": w.single_server(horizon=500),
        "two_servers_lb.yml": w.lb_two_servers(),
        "event_inj_lb.yml": w.lb_with_events(users=120, horizon=600),
        "event_inj_single_server.yml": w.single_server_with_spike(),
        "heavy_inj_single_server.yml": w.single_server_with_spike(heavy=True),
    }
    assert set(theirs_all) == set(cases)
    for name, ours in cases.items():
        assert normalize_payload(ours) == normalize_payload(theirs_all[name]), name


def test_results_feed_the_reference_plot_helpers():
    """ScenarioResults' drop-in accessors report what the reference's own ResultsAnalyzer and ram plot helper
    (src/asyncflow/metrics/analyzer.py:264-589, run through to_reference_analyzer() on the same arrays, recorded) report."""
    from asyncflow_amd import _abi
    from asyncflow_amd.results import ScenarioResults

    fx = np.load(GOLDEN_DIR / "lb2_rr_t30.npz", allow_pickle=False)
    plan = lower(json.loads(str(fx["payload_json"])))
    counts = np.zeros(_abi.CNT_SLOTS, dtype=np.uint32)
    counts[_abi.CNT_GENERATED], counts[_abi.CNT_COMPLETED] = int(fx["generated"]), int(fx["completed"])
    counts[_abi.CNT_TICKS] = int(fx["ticks"])
    sc = ScenarioResults(plan, counts, fx["clock"], fx["samples"])
    theirs = json.loads(str(_RECORDED["analyzer_lb2_rr_t30"]))
    assert theirs["latency_stats"] == sc.get_latency_stats()
    assert theirs["throughput"] == list(sc.get_throughput_series()[1])
    assert theirs["server_ids"] == sc.list_server_ids()
    sid = theirs["ram_plot_server"]
    assert sid == plan.server_ids[0] and theirs["ram_plot_ydata"]
    assert np.array_equal(np.asarray(theirs["ram_plot_ydata"], dtype=np.float64),
                          np.asarray(sc.get_sampled_metrics()["ram_in_use"][sid], dtype=np.float64))


# ------------------------------------------------------------- documented deviations, shown on the reference itself
def test_reference_raises_negative_delay_where_the_engine_reports_a_flag():
    """edge.py:107: `yield self.env.timeout(effective)` with effective = transit + spike < 0 -> simpy raises ValueError
    ("Negative delay"); the oracle (and the engine: tests/test_hostcheck.py) carry AF_FLAG_NEGATIVE_DELAY instead, and
    asyncflow_amd.SimulationRunner raises the same ValueError for such a scenario."""
    from asyncflow_amd import _abi
    from oracle.scenarios import negative_spike_residue

    payload = negative_spike_residue(horizon=10)
    key = _recorded(payload, 3)
    assert f"{key}.raised" in _RECORDED.files and str(_RECORDED[f"{key}.raised"]).startswith("ValueError: Negative delay")
    assert int(ol.simulate(lower(payload), 3).counts[_abi.CNT_FLAGS]) & _abi.FLAG_NEGATIVE_DELAY
    early = negative_spike_residue(horizon=6, shift=2.0)          # no residue yet: reference and oracle agree bit for bit
    _same(early, 3)


def test_reference_blocks_a_ram_starved_server_and_so_does_the_oracle():
    """server.py:146-149: a request whose endpoint needs more RAM than `ram_mb` waits in `RAM.get()` for good, and -- the
    container's gets being FIFO -- so does everything that reaches that server after it: observably, those requests
    never complete.  Oracle / engine: the same clock and samples, plus the informational AF_FLAG_RAM_STARVED."""
    from asyncflow_amd import _abi
    from oracle.scenarios import ram_starved

    payload = ram_starved(30)
    _same(payload, 1)
    assert int(ol.simulate(lower(payload), 1).counts[_abi.CNT_FLAGS]) & _abi.FLAG_RAM_STARVED


def test_reference_delays_a_response_whose_ram_put_fails_by_one_rounding_and_so_does_the_oracle():
    """server.py:270-276 on simpy's Container (`_do_put`: `if self._capacity - self._level >= event.amount`): with a need of
    100.3 MB, 2048 - fl(2048 - 100.3) is one ulp short of 100.3, the put WAITS for the next get on that Container and the
    response is sent then.  Round 5 reported it; since round 6 the oracle (and the engine) model the put queue, bit for bit."""
    from asyncflow_amd import _abi
    from oracle.scenarios import fractional_ram, ram_put_deadlock

    blocked, dyadic = fractional_ram(False), fractional_ram(True)
    res = ol.simulate(lower(blocked), 22)
    assert res.put_waits > 100 and int(res.counts[_abi.CNT_FLAGS]) == 0
    _same(blocked, 22)
    _same(dyadic, 21)
    assert ol.simulate(lower(dyadic), 21).put_waits == 0
    for seed in (4, 8, 11):          # a waiting put facing a waiter that does not fit: the server's RAM is dead from then on
        dead = ol.simulate(lower(ram_put_deadlock(20)), seed)
        assert dead.put_waits >= 2 and int(dead.counts[_abi.CNT_FLAGS]) & _abi.FLAG_RAM_STARVED
        _same(ram_put_deadlock(20), seed)


@pytest.mark.parametrize("case", range(24))
def test_fractional_ram_fuzz_matches_reference(case):
    """Decimal RAM needs on tight budgets, half of them on dyadic step times: waiting puts, several behind one, dead-locked
    RAM containers, all inside tie storms (160 more cases of this family were run when the put queue was written)."""
    from oracle.scenarios import fractional_ram_fuzz

    _same(fractional_ram_fuzz(random.Random(424200 + case), horizon=10), 900 + case)


@pytest.mark.parametrize("kw", [dict(front=1), dict(front=2, algo="least_connection", backend=True, spike=True), dict(front=1, general=True)])
def test_gateway_in_front_of_the_load_balancer_matches_reference(kw):
    """client -> server chain -> LB -> servers [-> backend] -> client (`graph.py:100-159` validates it): the oracle against the
    reference's recorded outputs, bit for bit -- the topology the stage-parallel kernel took in in round 5."""
    from oracle.scenarios import gateway_lb

    _same(gateway_lb(horizon=12, **kw), 5)
