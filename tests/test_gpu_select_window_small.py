"""select()'s lane window on the device (af_flow.hpp: Flow::select_regs, the DPP forms of engine.hip): 64 seeds of LB-2 at the
three points that decide it -- its own parameters (full 64-entry lists, the window ranks nearly every call), every edge at
50 ms with 1000 users (the proof fails in nearly every call: the bucket rank behind it) and 20 ms with 400 users (both
outcomes, carried-over entries between newcomers) -- on the plan-specialised and on the generic kernel, every scenario
against the oracle: counts, clock bit patterns, every sample.  No scenario is handed back."""

from __future__ import annotations

import numpy as np
import pytest

from asyncflow_amd.plan import lower
from asyncflow_amd.workloads import lb_two_servers
from oracle import oracle_lib as ol

pytestmark = pytest.mark.gpu

SEEDS = 0x5E1EC700 + np.arange(64, dtype=np.uint64)
POINTS = {"own": (400, None), "users1000_edges50ms": (1000, 0.05), "users400_edges20ms": (400, 0.02)}


def _payload(point: str) -> dict:
    users, mean = POINTS[point]
    p = lb_two_servers(users=users, horizon=20)
    if mean is not None:
        for e in p["topology_graph"]["edges"]:
            e["latency"]["mean"] = mean
    return p


@pytest.fixture(scope="module")
def oracle_runs():
    runs = {}
    for point in POINTS:
        plan = lower(_payload(point))
        runs[point] = [ol.simulate(plan, int(s)) for s in SEEDS]
    return runs


@pytest.mark.parametrize("kernels", ["specialised", "generic"])
@pytest.mark.parametrize("point", list(POINTS))
def test_lb2_64_seeds_equal_the_oracle(point, kernels, oracle_runs):
    from asyncflow_amd.runner import SimulationRunner

    res = SimulationRunner(simulation_input=_payload(point), seeds=SEEDS, device=0, flow=True, specialise=kernels == "specialised").run()
    st = res.engine_stats
    assert st.flow_scenarios == len(SEEDS) and st.flow_fallback == 0
    assert (st.specialised_launches >= 1) == (kernels == "specialised")
    want_all = oracle_runs[point]
    assert sum(int(w.counts[0]) for w in want_all) > 0
    for i, want in enumerate(want_all):
        got = res[i]
        assert np.array_equal(got.counts[:5].astype(np.uint64), want.counts[:5]), (i, got.counts, want.counts)
        assert np.array_equal(got.rqs_clock.view(np.uint64), want.clock.view(np.uint64)), f"scenario {i}: rqs_clock differs"
        assert np.array_equal(got._samples, want.samples), f"scenario {i}: sampled series differ"  # noqa: SLF001
