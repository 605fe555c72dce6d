"""The three places that draw (the arrival generator, the edges of the stage-parallel kernel, the pre-generated edge draws of
the next-event kernels) on the smallest plan that goes through all of them: every scenario against the oracle, on the
plan-specialised, the generic and the next-event kernels (the device's draw instructions changed, its bits
must not)."""

from __future__ import annotations

import numpy as np
import pytest

from asyncflow_amd.plan import lower
from oracle import oracle_lib as ol
from oracle.scenarios import single_server

pytestmark = pytest.mark.gpu

SEEDS = 0xD7A30000 + np.arange(64, dtype=np.uint64)


@pytest.fixture(scope="module")
def oracle_runs():
    plan = lower(single_server(horizon=20))
    return [ol.simulate(plan, int(s)) for s in SEEDS]


@pytest.mark.parametrize("kernels", ["specialised", "generic", "next-event"])
def test_single_server_64_seeds_equal_the_oracle(kernels, oracle_runs):
    from asyncflow_amd.runner import SimulationRunner

    kw = {"specialised": {"flow": True, "specialise": True}, "generic": {"flow": True, "specialise": False},
          "next-event": {"flow": False, "specialise": False}}[kernels]
    res = SimulationRunner(simulation_input=single_server(horizon=20), seeds=SEEDS, device=0, **kw).run()
    st = res.engine_stats
    if kernels == "next-event":
        assert st.flow_scenarios == 0
    else:
        assert st.flow_scenarios == len(SEEDS) and st.flow_fallback == 0
        assert (st.specialised_launches >= 1) == (kernels == "specialised")
    assert sum(int(w.counts[0]) for w in oracle_runs) > 0
    for i, want in enumerate(oracle_runs):
        got = res[i]
        assert np.array_equal(got.counts[:5].astype(np.uint64), want.counts[:5]), (i, got.counts, want.counts)
        assert np.array_equal(got.rqs_clock.view(np.uint64), want.clock.view(np.uint64)), f"scenario {i}: rqs_clock differs"
        assert np.array_equal(got._samples, want.samples), f"scenario {i}: sampled series differ"  # noqa: SLF001
