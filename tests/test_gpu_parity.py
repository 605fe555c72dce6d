"""Parity tests proper: the HIP engine (through the C ABI) vs the oracle, on a real MI355X.

This file pins the sequential next-event kernels (af_core.hpp; `flow=False`): they run every plan and
take over whatever the stage-parallel kernel hands back.  The reference-generated fixtures are asserted on
BOTH kernel families (`flow` parametrised): the stage-parallel kernel -- the one bench.py times -- is compared
with what the unmodified reference produced directly, not only through the oracle.  tests/test_gpu_flow.py
pins the rest of the stage-parallel kernel and the hand-over between the two."""

from __future__ import annotations

import json
import random

import numpy as np
import pytest

from asyncflow_amd import _abi
from asyncflow_amd.plan import lower
from oracle import oracle_lib as ol
from oracle.scenarios import (fanout8, lb_two_servers, lb_with_events, overload, random_payload, server_chain,
                              single_server, tie_storm, wide_fanout)
from tests.conftest import GOLDEN_DIR, golden_names

pytestmark = pytest.mark.gpu


def _runner(payload, **kw):
    from asyncflow_amd.runner import SimulationRunner

    kw.setdefault("flow", False)
    return SimulationRunner(simulation_input=payload, **kw)


def _assert_scenario(got, want):
    assert np.array_equal(got.counts[:5].astype(np.uint64), want.counts[:5]), (got.counts, want.counts)
    assert np.array_equal(got.rqs_clock.view(np.uint64), want.clock.view(np.uint64)), "rqs_clock differs"
    assert np.array_equal(got._samples, want.samples), "sampled series differ"  # noqa: SLF001


# ---------------------------------------------------------------- spec pinning
def test_device_math_matches_oracle_bit_for_bit():
    from asyncflow_amd.engine import probe_math

    L = ol.lib()
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.random(20000), 1.0 - rng.random(2000) * 1e-9, np.exp(rng.uniform(-300, 300, 4000))])
    assert np.array_equal(probe_math(1, x), np.array([L.orc_x_log(float(v)) for v in x]))
    # af_log_unit: the logarithm of the exponential variates (argument 1 - u in [2^-53, 1]) without af_log's special cases
    xu = np.concatenate([1.0 - rng.random(20000), 1.0 - rng.random(2000) * 1e-9, rng.random(2000) * 1e-9 + 2.0 ** -53,
                         [1.0, 2.0 ** -53, 1.0 - 2.0 ** -53, 0.5, 0.7071067811865476, 0.7071067811865475]])
    assert np.array_equal(probe_math(7, xu).view(np.uint64), np.array([L.orc_x_log(float(v)) for v in xu]).view(np.uint64))
    e = np.concatenate([rng.uniform(-30, 30, 20000), rng.uniform(-700, 700, 2000)])
    assert np.array_equal(probe_math(2, e), np.array([L.orc_x_exp(float(v)) for v in e]))
    p = np.concatenate([rng.random(20000), rng.random(2000) * 1e-12])
    p = p[(p > 0) & (p < 1)]
    assert np.array_equal(probe_math(3, p), np.array([L.orc_x_norminv(float(v)) for v in p]))
    s = np.exp(rng.uniform(-50, 50, 20000))
    assert np.array_equal(probe_math(4, s), np.sqrt(s))            # IEEE sqrt
    a, b = rng.normal(size=20000), np.exp(rng.uniform(-20, 20, 20000))
    assert np.array_equal(probe_math(5, a, b), a / b)              # IEEE division
    idx = np.arange(5000, dtype=np.float64)
    for stream, j in ((0, 0), (3, 1), (0x1001, 5)):
        got = probe_math(0, idx, np.full_like(idx, stream * 65536 + j), seed=0x5EED0007)
        want = np.array([L.orc_x_uniform(0x5EED0007, stream, int(i), j) for i in idx])
        assert np.array_equal(got, want)
    means = np.array([0.003, 0.7, 5.0, 16.0, 33.0, 400.0, 1000.0] * 50)
    got = probe_math(6, means, np.arange(len(means), dtype=np.float64) + 7 * 65536, seed=11)
    want = np.array([L.orc_x_poisson(float(m), 11, 7, i, 0) for i, m in enumerate(means)], dtype=np.float64)
    assert np.array_equal(got, want)


# ------------------------------------------------------------- golden fixtures
@pytest.mark.parametrize("flow", [True, False], ids=["flow", "next-event"])
@pytest.mark.parametrize("name", golden_names())
def test_engine_reproduces_reference_fixtures(name, flow):
    """Every fixture written by the UNMODIFIED reference (oracle/make_golden.py) on both kernel families.  flow=True is
    the engine's default path: af_flow_kernel for the feed-forward plans (lb2_rr_t30 / _t600, lb2_lc_t20, lb2_events_t60,
    fanout8_t20, single_server_t30), its hand-over to the next-event kernels for the plans outside its range
    (stress_mixed_t40, overload_t30: several endpoints per server, Poisson latencies)."""
    fx = np.load(GOLDEN_DIR / f"{name}.npz", allow_pickle=False)
    payload = json.loads(str(fx["payload_json"]))
    seed = int(fx["seed"])
    res = _runner(payload, seeds=[seed, seed + 1, seed], flow=flow).run()
    st = res.engine_stats
    if flow and not res.flow_reason:
        assert st.flow_scenarios == 3, "a feed-forward plan must run on the stage-parallel kernel"
    else:
        assert st.flow_scenarios == 0
    plan = lower(payload)
    want = ol.simulate(plan, seed)
    _assert_scenario(res[0], want)
    _assert_scenario(res[2], want)                      # same seed -> same result, any lane
    _assert_scenario(res[1], ol.simulate(plan, seed + 1))
    # ... and identical to what the unmodified reference produced (exact timestamp ties included)
    got = res[0]
    assert not got.flags & _abi.FLAG_TIME_TIE
    assert np.array_equal(got.rqs_clock, fx["clock"]) and np.array_equal(got._samples, fx["samples"])  # noqa: SLF001
    assert (got.total_generated, got.total_completed, got.total_dropped) == (
        int(fx["generated"]), int(fx["completed"]), int(fx["dropped"]))
    stats = got.get_latency_stats()
    keys = ("total_requests", "mean", "median", "std_dev", "p95", "p99", "min", "max")
    assert [stats[k] for k in keys] == list(fx["latency_stats"])   # same numpy calls as the analyzer
    assert got.get_throughput_series()[1] == list(fx["rps"])


# --------------------------------------------------------------------- batches
def test_lb2_batch_matches_oracle_everywhere_sampled():
    payload = lb_two_servers(horizon=30)
    seeds = 0x5EED0000 + np.arange(200, dtype=np.uint64)     # not a multiple of 64: ragged last wave
    res = _runner(payload, seeds=seeds, lanes_per_wave=64).run()
    assert res.engine_stats.state_in_lds == 1 and res.engine_stats.waves == 4
    plan = lower(payload)
    for i in (0, 1, 63, 64, 127, 199):
        _assert_scenario(res[i], ol.simulate(plan, int(seeds[i])))
    want_counts = np.array([ol.simulate(plan, int(s), want_clock=False, want_samples=False).counts[:5] for s in seeds])
    assert np.array_equal(res.counts[:, :5].astype(np.uint64), want_counts)


def test_global_state_mode_is_bit_identical_to_lds_mode():
    payload = lb_with_events(users=150, horizon=30, scale=0.05)
    seeds = np.arange(70, dtype=np.uint64) + 5
    a = _runner(payload, seeds=seeds).run()
    b = _runner(payload, seeds=seeds, force_global_state=True).run()
    assert a.engine_stats.state_in_lds == 1 and b.engine_stats.state_in_lds == 0
    assert np.array_equal(a.counts, b.counts)
    for i in (0, 69):
        assert np.array_equal(a[i].rqs_clock, b[i].rqs_clock) and np.array_equal(a[i]._samples, b[i]._samples)  # noqa: SLF001


def test_large_state_falls_back_to_hbm_and_still_matches():
    payload = fanout8(horizon=20)                           # ~200 requests in flight: does not fit LDS
    seeds = np.arange(64, dtype=np.uint64) + 11
    res = _runner(payload, seeds=seeds, lanes_per_wave=64).run()
    assert res.engine_stats.state_in_lds == 0
    plan = lower(payload)
    for i in (0, 33):
        _assert_scenario(res[i], ol.simulate(plan, int(seeds[i])))
    narrow = _runner(payload, seeds=seeds).run()            # few scenarios -> narrow waves -> fits LDS
    assert narrow.engine_stats.state_in_lds == 1 and narrow.engine_stats.lanes_per_wave < 64
    assert np.array_equal(narrow.counts, res.counts)
    assert np.array_equal(narrow[33].rqs_clock, res[33].rqs_clock)


@pytest.mark.parametrize("lanes", [1, 2, 8, 32, 64])
def test_lanes_per_wave_does_not_change_results(lanes):
    payload = lb_with_events(users=150, horizon=20, scale=0.03)
    seeds = np.arange(77, dtype=np.uint64) + 900
    ref = _runner(payload, seeds=seeds, lanes_per_wave=4).run()
    res = _runner(payload, seeds=seeds, lanes_per_wave=lanes).run()
    assert res.engine_stats.lanes_per_wave == lanes
    assert np.array_equal(ref.counts, res.counts)
    for i in (0, 40, 76):
        assert np.array_equal(ref[i].rqs_clock, res[i].rqs_clock) and np.array_equal(ref[i]._samples, res[i]._samples)  # noqa: SLF001


def test_parameter_sweep_columns():
    payload = lb_two_servers(horizon=20)
    n = 96
    users = np.repeat([10.0, 200.0, 480.0], n // 3)
    lat = np.tile([0.0005, 0.004, 0.02, 0.05], n // 4)
    seeds = 0xC0F30000 + np.arange(n, dtype=np.uint64)
    sweep = {"rqs_input.avg_active_users.mean": users, "topology_graph.edges[*].latency.mean": lat}
    res = _runner(payload, seeds=seeds, sweep=sweep).run()
    for i in (0, 17, 50, 95):
        plan = lower(payload)
        ol.apply_overrides(plan, {("gen_users_mean", 0): users[i], **{("edge_mean", e): lat[i] for e in range(6)}})
        _assert_scenario(res[i], ol.simulate(plan, int(seeds[i])))
    gen = res.counts[:, _abi.CNT_GENERATED].astype(np.float64)
    assert gen[users == 480.0].mean() > 30 * gen[users == 10.0].mean()


@pytest.mark.parametrize("flow", [False, True], ids=["next-event", "flow"])
def test_sweep_larger_than_the_draw_budget_runs_in_chunks_with_identical_results(flow):
    """flow=True: the stage-parallel kernel over several chunks -- output and column pointers offset by the chunk's start, and
    (a users column) the heaviest-first launch order of a chunk that does not start at scenario 0."""
    payload = lb_two_servers(horizon=20)
    n = 150
    users = np.linspace(20.0, 400.0, n)
    seeds = 0xABCD0000 + np.arange(n, dtype=np.uint64)
    sweep = {"rqs_input.avg_active_users.mean": users}
    whole = _runner(payload, seeds=seeds, sweep=sweep, flow=flow).run()
    # 1 MiB of draws per chunk: (1 + 6 edges) * clock_capacity * 8 B per scenario -> a handful of scenarios
    # (flow=True: the stage-parallel kernel pre-generates arrival times only, clock_capacity * 8 B per scenario -> fewer chunks)
    parts = _runner(payload, seeds=seeds, sweep=sweep, draw_memory_mb=1, flow=flow,
                    clock_capacity=whole._clock_t.shape[1]).run()  # noqa: SLF001
    assert whole.engine_stats.chunks == 1
    if flow:
        assert parts.engine_stats.chunks > 1 and parts.engine_stats.flow_scenarios == n
    else:
        assert parts.engine_stats.chunks > 3
    assert np.array_equal(whole.counts, parts.counts)
    for i in range(n):
        assert np.array_equal(whole[i].rqs_clock, parts[i].rqs_clock)
    assert np.array_equal(whole._samples_t.cpu().numpy(), parts._samples_t.cpu().numpy())  # noqa: SLF001


@pytest.mark.parametrize("case", range(6))
def test_fuzzed_payloads(case):
    rng = random.Random(9000 + case)
    payload = random_payload(rng, horizon=8)
    seeds = np.arange(3, dtype=np.uint64) + 100 * case
    res = _runner(payload, seeds=seeds).run()
    plan = lower(payload)
    for i in range(3):
        _assert_scenario(res[i], ol.simulate(plan, int(seeds[i])))


@pytest.mark.parametrize(("n_srv", "algo"), [(9, "round_robin"), (24, "least_connection")])
def test_more_than_eight_servers_behind_the_load_balancer(n_srv, algo):
    payload = wide_fanout(n_srv, algo)
    seeds = np.arange(6, dtype=np.uint64) + 1
    res = _runner(payload, seeds=seeds).run()
    plan = lower(payload)
    for i in range(6):
        _assert_scenario(res[i], ol.simulate(plan, int(seeds[i])))


@pytest.mark.parametrize(("dist", "mean"), [("exponential", 0.003), ("poisson", 0.7), ("normal", 0.001)])
def test_server_to_server_chain_with_zero_delay_hops(dist, mean):
    payload = server_chain(dist, mean)
    seeds = np.arange(6, dtype=np.uint64) + 1
    res = _runner(payload, seeds=seeds).run()
    plan = lower(payload)
    for i in range(6):
        _assert_scenario(res[i], ol.simulate(plan, int(seeds[i])))
    assert not int(np.bitwise_or.reduce(res.flags)) & _abi.FLAG_TIME_TIE


def test_plan_specialised_kernels_give_identical_results():
    """asyncflow_amd/jit.py: the same source compiled with the plan's shape as constants."""
    for payload, kw in ((lb_two_servers(horizon=20), {}),
                        (lb_with_events(users=150, horizon=30, scale=0.05), {}),
                        (tie_storm(random.Random(777003), horizon=12), {"expect_shared_instants": True})):
        seeds = np.arange(70, dtype=np.uint64) + 31
        generic = _runner(payload, seeds=seeds, specialise=False, **kw).run()
        special = _runner(payload, seeds=seeds, specialise=True, **kw).run()
        assert generic.engine_stats.specialised_launches == 0 and special.engine_stats.specialised_launches >= 1
        assert np.array_equal(generic.counts, special.counts)
        for i in (0, 33, 69):
            assert np.array_equal(generic[i].rqs_clock, special[i].rqs_clock)
            assert np.array_equal(generic[i]._samples, special[i]._samples)  # noqa: SLF001
        plan = lower(payload)
        _assert_scenario(special[5], ol.simulate(plan, int(seeds[5])))


def test_fuzz_sweep_of_topologies_all_scenarios_checked():
    """60 random topologies x 5 seeds, every scenario compared with the oracle (all distributions,
    multi-core servers, RAM queues, LB algorithms, spikes and outages)."""
    checked = shared = negative = 0
    for case in range(60):
        payload = random_payload(random.Random(31000 + case), horizon=6)
        seeds = np.arange(5, dtype=np.uint64) + 17 * case
        # (topology 12 has overlapping spikes with a negative f64 residue under zero transit times: the reference RAISES
        # "Negative delay" there -- confirmed on the live reference --, the engine reports AF_FLAG_NEGATIVE_DELAY like the oracle)
        res = _runner(payload, seeds=seeds, lanes_per_wave=[0, 1, 2, 8][case % 4], on_negative_delay="flag").run()
        plan = lower(payload)
        shared += int(res.engine_stats.shared_instant_scenarios)
        for i in range(5):
            want = ol.simulate(plan, int(seeds[i]))
            _assert_scenario(res[i], want)
            assert (int(res.flags[i]) & _abi.FLAG_NEGATIVE_DELAY) == (int(want.counts[_abi.CNT_FLAGS]) & _abi.FLAG_NEGATIVE_DELAY)
            negative += bool(int(res.flags[i]) & _abi.FLAG_NEGATIVE_DELAY)
            checked += 1
        assert not int(np.bitwise_or.reduce(res.flags)) & _abi.FLAG_TIME_TIE
    assert checked == 300 and shared > 0 and negative == 5


def test_shared_timestamps_follow_simpy_order():
    """Instants shared by several timed events run through the kernel's SimPy-order path."""
    payload = overload(horizon=12)
    res = _runner(payload, seeds=[5]).run()
    plan = lower(payload)
    want = ol.simulate(plan, 5)
    assert want.ties > 0
    _assert_scenario(res[0], want)
    assert not res[0].flags & _abi.FLAG_TIME_TIE
    ties = 0
    for case in range(24):                               # one launch per topology, 8 seeds each
        payload = tie_storm(random.Random(777000 + case), horizon=12)
        seeds = np.arange(8, dtype=np.uint64) + 5 + case
        res = _runner(payload, seeds=seeds, lanes_per_wave=[1, 4, 64][case % 3]).run()
        plan = lower(payload)
        for i in (0, 3, 7):
            want = ol.simulate(plan, int(seeds[i]))
            ties += want.ties
            _assert_scenario(res[i], want)
        assert not int(np.bitwise_or.reduce(res.flags)) & _abi.FLAG_TIME_TIE
    assert ties > 3000


def test_handover_between_kernel_variants_is_invisible():
    """Lean kernel first + hand-over of the scenarios that meet a shared instant == SimPy-order
    kernel from the start; the runner remembers that a payload produces such instants."""
    payload = tie_storm(random.Random(777003), horizon=12)
    seeds = np.arange(40, dtype=np.uint64) + 900
    two_pass = _runner(payload, seeds=seeds, expect_shared_instants=False).run()
    direct = _runner(payload, seeds=seeds, expect_shared_instants=True).run()
    assert two_pass.engine_stats.shared_instant_scenarios > 0 and direct.engine_stats.shared_instant_scenarios == 0
    assert np.array_equal(two_pass.counts, direct.counts)
    for i in range(40):
        assert np.array_equal(two_pass[i].rqs_clock, direct[i].rqs_clock)
        assert np.array_equal(two_pass[i]._samples, direct[i]._samples)  # noqa: SLF001
    plan = lower(payload)
    for i in (0, 17, 39):
        _assert_scenario(direct[i], ol.simulate(plan, int(seeds[i])))
    auto1 = _runner(payload, seeds=seeds).run()           # None: lean first, remembered per payload
    auto2 = _runner(payload, seeds=seeds).run()
    assert auto2.engine_stats.shared_instant_scenarios == 0 and np.array_equal(auto1.counts, auto2.counts)
    calm = _runner(lb_two_servers(horizon=20), seeds=seeds).run()
    assert calm.engine_stats.shared_instant_scenarios == 0


def test_a_chunk_in_pieces_with_reruns_equals_the_chunk_in_one_piece(monkeypatch):
    """AF_SEQ_PIECE=3: one chunk of 7 scenarios as pieces of 3, 3 and 1 over an identity list.  Every scenario of this payload
    meets shared instants (seeds 900..939 on the CPU oracle: 25 to 139 each), so every piece has its second pass on the
    SimPy-order kernel, which starts from cleared online counters."""
    from oracle import analyzer_oracle as ao

    payload = tie_storm(random.Random(777003), horizon=12)
    seeds = np.arange(7, dtype=np.uint64) + 900
    kw = {"seeds": seeds, "expect_shared_instants": False, "online_summary": {"hist_bins": 512, "hist_max": 0.256}}
    plain = _runner(payload, **kw).run()
    monkeypatch.setenv("AF_SEQ_PIECE", "3")
    pieces = _runner(payload, **kw).run()
    monkeypatch.delenv("AF_SEQ_PIECE")
    assert plain.engine_stats.chunks == 1 and pieces.engine_stats.chunks == 1
    assert plain.engine_stats.shared_instant_scenarios == 7 and pieces.engine_stats.shared_instant_scenarios == 7
    assert np.array_equal(plain.counts, pieces.counts)
    for i in range(7):
        assert np.array_equal(plain[i].rqs_clock.view(np.uint64), pieces[i].rqs_clock.view(np.uint64)), f"scenario {i}: rqs_clock"
    assert np.array_equal(plain._samples_t.cpu().numpy(), pieces._samples_t.cpu().numpy())  # noqa: SLF001
    for res in (plain, pieces):
        hist = res.online_hist.cpu().numpy().view(np.uint32)
        rps = res.online_rps.cpu().numpy()
        for i in range(7):
            ck = res[i].rqs_clock
            assert np.array_equal(hist[i], ao.latency_histogram(ck, 512, 0.256)), f"scenario {i}: online histogram"
            assert np.array_equal(rps[i].astype(np.float64), ao.throughput_series(ck, 12)[1]), f"scenario {i}: online rps"
    _assert_scenario(pieces[4], ol.simulate(lower(payload), 904))      # in the second piece


# ------------------------------------------------------------------ edge cases
def test_overflow_is_reported_and_auto_grow_recovers():
    payload = overload(horizon=8)
    with pytest.raises(OverflowError):
        _runner(payload, seeds=[1, 2], request_capacity=16, fifo_capacity=8, auto_grow=False).run()
    with pytest.warns(RuntimeWarning):
        res = _runner(payload, seeds=[1, 2], request_capacity=64, fifo_capacity=16).run()
    _assert_scenario(res[1], ol.simulate(lower(payload), 2))
    # a backlog that grows with the horizon, pools far too small: the queue goes to the pool's size on its second overflow,
    # the pool fourfold per run -- the sweep ends within MAX_ATTEMPTS runs instead of raising with room left to grow
    long = overload(horizon=30)
    with pytest.warns(RuntimeWarning):
        res = _runner(long, seeds=[3], request_capacity=16, fifo_capacity=8).run()
    _assert_scenario(res[0], ol.simulate(lower(long), 3))


def test_single_run_is_a_drop_in_for_the_reference_call(tmp_path):
    import yaml

    from asyncflow_amd.runner import SimulationRunner

    path = tmp_path / "scenario.yml"
    path.write_text(yaml.safe_dump(single_server(horizon=10)))
    results = SimulationRunner.from_yaml(env=None, yaml_path=path).run()
    stats = results.get_latency_stats()
    assert set(stats) == {"total_requests", "mean", "median", "std_dev", "p95", "p99", "min", "max"}
    ts, rps = results.get_throughput_series()
    assert ts == [float(k) for k in range(1, 11)] and sum(rps) == stats["total_requests"]
    sm = results.get_sampled_metrics()
    assert set(sm) == {"ready_queue_len", "event_loop_io_sleep", "ram_in_use", "edge_concurrent_connection"}
    t, v = results.get_series("ram_in_use", "srv-1")
    assert len(t) == len(v) == lower(single_server(horizon=10)).tick_count
    assert results.list_server_ids() == ["srv-1"]


def test_zero_load_and_disabled_metrics():
    payload = lb_two_servers(users=0, horizon=6)
    payload["sim_settings"]["enabled_sample_metrics"] = ["edge_concurrent_connection"]
    res = _runner(payload, seeds=[1, 2]).run()
    assert res.counts[:, _abi.CNT_GENERATED].sum() == 0
    assert res[0].get_latency_stats() == {}
    assert set(res[0].get_sampled_metrics()) == {"edge_concurrent_connection"}


# ------------------------------------------------- full-size, size-independent
def test_full_horizon_properties_and_statistical_parity_with_simpy():
    """BASELINE config 2 at the full 600 s horizon (fewer replicas than 10 000: the
    bench runs those).  Invariants + the pooled p50/p95 of the stock numpy-seeded
    SimPy reference (mean 24.04 ms, p50 23.18, p95 33.65, p99 39.68)."""
    payload = lb_two_servers()
    n = 256
    res = _runner(payload, replicas=n, specialise=True).run()      # the kernels bench.py measures
    assert res.engine_stats.specialised_launches >= 1
    c = res.counts.astype(np.int64)
    gen, comp, drop, ev, ticks = (c[:, k] for k in range(5))
    assert np.all(ticks == 11999)
    assert np.all(comp + drop <= gen) and np.all(gen - comp - drop <= 64)     # the rest is in flight at T
    assert abs(gen.mean() - 80000) < 4 * 1300 / np.sqrt(n) + 200
    assert abs(ev.sum() / gen.sum() - 6.84) < 0.05                              # request-events per request
    summ = res.summary()
    stats = summ["stats"].cpu().numpy()
    mean, p50, p95, p99 = stats[:, 1].mean(), stats[:, 2].mean(), stats[:, 4].mean(), stats[:, 5].mean()
    assert abs(mean - 24.04e-3) / 24.04e-3 < 0.01
    assert abs(p50 - 23.18e-3) / 23.18e-3 < 0.01
    assert abs(p95 - 33.65e-3) / 33.65e-3 < 0.01
    assert abs(p99 - 39.68e-3) / 39.68e-3 < 0.02
    assert abs(summ["rps"].sum(dim=1).cpu().numpy() - comp).max() == 0
    for i in (0, n - 1):
        s = res[i]
        clock = s.rqs_clock
        assert np.all(np.diff(clock[:, 1]) >= 0) and np.all(clock[:, 1] >= clock[:, 0]) and clock[:, 1].max() < 600.0
        host = s.get_latency_stats()
        assert [host[k] for k in ("mean", "median", "std_dev", "p95", "p99", "min", "max")] == stats[i, 1:].tolist()   # numpy on the host == the HIP analyzer, bit for bit
        sm = s.get_sampled_metrics()
        assert max(sm["ram_in_use"]["srv-1"]) <= 2048 and min(sm["edge_concurrent_connection"]["lb-srv1"]) >= 0
        assert np.array_equal(clock, ol.simulate(lower(payload), int(res.seeds[i])).clock)
