"""select()'s window width per station list on the device (af_flow.hpp: Flow::select_regs, AF_SELECT_WINDOW_S0 .. _S3; the
plan-specialised build of the lean form gets its widths from flow_jit_spec_string): 64 seeds of LB-2 at the three points of
tests/test_gpu_select_window_small.py -- its own parameters (the window ranks most calls), every edge at 50 ms with 1000 users
(the proof fails in nearly every call: the bucket rank) and 20 ms with 400 users (both, in turn, inside one wave) -- on the
plan-specialised kernel, on the generic kernel, and on the plan-specialised kernel with every list's window forced to ONE lane
through ASYNCFLOW_JIT_EXTRA_FLAGS, where the proof fails often at every point and both ranks run beside each other.  Every
scenario against the oracle: counts, clock bit patterns, every sample.  No scenario is handed back."""

from __future__ import annotations

import numpy as np
import pytest

from asyncflow_amd.plan import lower
from asyncflow_amd.workloads import lb_two_servers
from oracle import oracle_lib as ol

pytestmark = pytest.mark.gpu

SEEDS = 0x5E1EC900 + np.arange(64, dtype=np.uint64)
POINTS = {"own": (400, None), "users1000_edges50ms": (1000, 0.05), "users400_edges20ms": (400, 0.02)}
WIDTH_ONE = " ".join(f"-DAF_SELECT_WINDOW_S{s}=1" for s in range(4))


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


@pytest.mark.parametrize("kernels", ["specialised", "generic", "specialised_width_one"])
@pytest.mark.parametrize("point", list(POINTS))
def test_lb2_64_seeds_equal_the_oracle(point, kernels, oracle_runs, monkeypatch):
    from asyncflow_amd import jit
    from asyncflow_amd.runner import SimulationRunner

    if kernels == "specialised_width_one":
        # (asyncflow_amd/jit.py reads the variable when it is imported: the flags it made of it are set alongside)
        monkeypatch.setenv("ASYNCFLOW_JIT_EXTRA_FLAGS", WIDTH_ONE)
        monkeypatch.setattr(jit, "_FLAGS", (*jit._FLAGS, *WIDTH_ONE.split()))  # noqa: SLF001
    res = SimulationRunner(simulation_input=_payload(point), seeds=SEEDS, device=0, flow=True, specialise=kernels != "generic").run()
    st = res.engine_stats
    assert st.flow_scenarios == len(SEEDS) and st.flow_fallback == 0
    assert (st.specialised_launches >= 1) == (kernels != "generic")
    want_all = oracle_runs[point]
    assert sum(int(w.counts[0]) for w in want_all) > 0
    for i, want in enumerate(want_all):
        got = res[i]
        assert np.array_equal(got.counts[:5].astype(np.uint64), want.counts[:5]), (i, got.counts, want.counts)
        assert np.array_equal(got.rqs_clock.view(np.uint64), want.clock.view(np.uint64)), f"scenario {i}: rqs_clock differs"
        assert np.array_equal(got._samples, want.samples), f"scenario {i}: sampled series differ"  # noqa: SLF001
