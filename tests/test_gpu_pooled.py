"""Pooled analyzer on the MI355X (af_engine_summarize_pooled): per group of scenarios the eight latency statistics of the
concatenated latencies, bit-equal to numpy's -- singleton groups equal the per-scenario analyzer, synthetic clocks cover the
seams of numpy's 8 / 128 / 8 192-element blocks, one group spans a whole batch, a sweep's points through the Python API."""

from __future__ import annotations

import numpy as np
import pytest

from asyncflow_amd import _abi
from asyncflow_amd.plan import lower
from oracle.scenarios import lb_two_servers, single_server

pytestmark = pytest.mark.gpu


def _np_stats(lat: np.ndarray) -> np.ndarray:
    """oracle/analyzer_oracle.py::latency_stats on a latency array (vectorised: the pooled arrays are large)."""
    lat = np.ascontiguousarray(lat, dtype=np.float64)
    if lat.size == 0:
        return np.array([0.0] + [np.nan] * 7)
    return np.array([float(lat.size), float(np.mean(lat)), float(np.median(lat)), float(np.std(lat)),
                     float(np.percentile(lat, 95)), float(np.percentile(lat, 99)), float(np.min(lat)), float(np.max(lat))])


def _check(got: np.ndarray, want: np.ndarray, what="") -> None:
    if want[0] > 0:
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (what, got, want, got - want)
    else:
        assert got[0] == 0 and np.isnan(got[1:]).all(), (what, got)


def _pooled_synthetic(lats_list, group, n_groups, cap_limit=None, random_starts=False, seed=3):
    """Hand-made rqs_clock rows fed straight to af_engine_summarize_pooled.  Returns the stored latency arrays per
    scenario (finish - start as numpy computes it) and the stats [G, 8]."""
    import torch

    from asyncflow_amd.engine import Engine

    plan = lower(single_server(horizon=50))
    n = len(lats_list)
    cap = cap_limit or max(max((len(x) for x in lats_list), default=1), 1)
    rng = np.random.default_rng(seed)
    clock = np.full((n, cap, 2), np.nan)
    counts = np.zeros((n, _abi.CNT_SLOTS), dtype=np.uint32)
    stored = []
    for i, lat in enumerate(lats_list):
        lat = np.asarray(lat, dtype=np.float64)
        start = rng.uniform(0.0, 49.0, size=lat.size) if random_starts else np.zeros(lat.size)
        rows = np.stack([start, start + lat], axis=1) if lat.size else np.zeros((0, 2))
        counts[i, _abi.CNT_COMPLETED] = lat.size
        keep = rows[:cap]
        clock[i, : keep.shape[0]] = keep
        stored.append(keep[:, 1] - keep[:, 0])
    dev = torch.device("cuda", 0)
    clock_t = torch.as_tensor(clock, device=dev)
    counts_t = torch.as_tensor(counts.view(np.int32), device=dev)
    grp = np.asarray(group, dtype=np.int64)
    grp_t = torch.as_tensor(np.where(grp < 0, _abi.POOL_SKIP, grp).astype(np.uint32).view(np.int32), device=dev)
    stats = torch.empty((n_groups, 8), dtype=torch.float64, device=dev)
    eng = Engine(plan, 0)
    try:
        eng.summarize_pooled(n, n_groups, clock_ptr=clock_t.data_ptr(), clock_capacity=cap, counts_ptr=counts_t.data_ptr(),
                             stats_ptr=stats.data_ptr(), group_ptr=grp_t.data_ptr())
    finally:
        eng.close()
    return stored, stats.cpu().numpy()


def _want(stored, group, n_groups):
    group = np.asarray(group)
    return [_np_stats(np.concatenate([stored[s] for s in np.nonzero(group == g)[0]] or [np.zeros(0)])) for g in range(n_groups)]


def test_seams_of_numpy_blocks_across_scenarios():
    rng = np.random.default_rng(11)
    # member sizes so that the concatenation reaches and crosses 8-, 128- and 8 192-element boundaries at the seams
    sizes = [0, 3, 5, 8, 1, 120, 7, 128, 0, 8000, 191, 1, 8192, 64, 63, 1, 12000, 4, 16384, 9, 255, 8191, 2]
    lats = [rng.lognormal(-3.0, 0.8, k) for k in sizes]
    n = len(lats)
    one = np.zeros(n, dtype=np.int64)
    stored, stats = _pooled_synthetic(lats, one, 1, random_starts=True)
    _check(stats[0], _want(stored, one, 1)[0], "one group")
    # interleaved ids, a skipped scenario, an empty group (3), groups of every size
    grp = np.array([(i * 7) % 5 for i in range(n)])
    grp[grp == 3] = 4
    grp[[2, 9]] = -1
    stored, stats = _pooled_synthetic(lats, grp, 5, random_starts=True)
    for g, w in enumerate(_want(stored, grp, 5)):
        _check(stats[g], w, f"group {g}")
    assert stats[3, 0] == 0


def test_one_group_of_twenty_thousand_tiny_members_and_odd_values():
    rng = np.random.default_rng(5)
    n = 20_000
    k = rng.integers(0, 4, n)
    lats = [rng.exponential(0.02, int(m)) for m in k]
    stored, stats = _pooled_synthetic(lats, np.zeros(n, dtype=np.int64), 1)
    _check(stats[0], _want(stored, np.zeros(n), 1)[0], "0-3 completions each")
    # ties across members, many exact zeros, the whole exponent range
    vals = np.concatenate([np.zeros(5000), np.full(3000, 0.125), 2.0 ** rng.integers(-1074, 500, 4000),
                           rng.exponential(1.0, 3000), [5e-324, 2.0 ** -1022, 1e150]])   # (squares stay finite)
    rng.shuffle(vals)
    lats = np.array_split(vals, 997)
    grp = np.arange(len(lats)) % 3
    stored, stats = _pooled_synthetic(lats, grp, 3)
    for g, w in enumerate(_want(stored, grp, 3)):
        _check(stats[g], w, f"odd values, group {g}")
    # all-empty groups, and a group id of 0xFFFFFFFF for every scenario but one
    stored, stats = _pooled_synthetic([[], [], [0.5, 0.25]], [0, 1, -1], 2)
    for g, w in enumerate(_want(stored, [0, 1, -1], 2)):
        _check(stats[g], w, f"empty group {g}")
    assert np.isnan(stats[:, 1:]).all() and (stats[:, 0] == 0).all()


def test_candidates_that_part_in_the_last_key_bits_and_a_constant_group():
    """0.05 + k ulp, k < 4096: every key shares its upper 52 bits, so the select takes five digit levels and stops at
    shift 2 with a handful of distinct candidates per rank -- no tie runs it down to shift 0, as the constant group does."""
    rng = np.random.default_rng(31)
    n = 9000
    for name, lat in (("last bits", 0.05 + rng.integers(0, 4096, n) * np.spacing(0.05)), ("constant", np.full(n, 0.0625))):
        stored, stats = _pooled_synthetic([lat], [0], 1)
        assert stored[0].size == n and (name == "constant" or np.unique(stored[0]).size > 3000)
        _check(stats[0], _np_stats(stored[0]), name)


def test_counts_above_the_clock_capacity_clamp():
    rng = np.random.default_rng(9)
    lats = [rng.exponential(0.03, 1000), rng.exponential(0.03, 700), rng.exponential(0.03, 50)]
    stored, stats = _pooled_synthetic(lats, [0, 0, 0], 1, cap_limit=300, random_starts=True)
    assert [s.size for s in stored] == [300, 300, 50]
    _check(stats[0], _want(stored, [0, 0, 0], 1)[0])


def test_singleton_groups_equal_the_per_scenario_analyzer():
    from asyncflow_amd.runner import SimulationRunner

    seeds = 0x5EED0000 + np.arange(64, dtype=np.uint64)
    res = SimulationRunner(simulation_input=lb_two_servers(horizon=60), seeds=seeds).run()
    per = res.summary(rps=False)["stats"].cpu().numpy()
    pooled = res.pooled_summary(np.arange(len(res)))
    assert pooled["replicas"].tolist() == [1] * len(res)
    assert np.array_equal(pooled["stats"].cpu().numpy().view(np.uint64), per.view(np.uint64))
    # hand-made clocks too (sizes around the analyzer's piece and leaf boundaries)
    rng = np.random.default_rng(2)
    lats = [rng.lognormal(-4.0, 1.0, k) for k in (1, 7, 8, 9, 127, 128, 129, 8191, 8192, 8193, 20000, 0)]
    stored, stats = _pooled_synthetic(lats, np.arange(len(lats)), len(lats), random_starts=True)
    for i, s in enumerate(stored):
        _check(stats[i], _np_stats(s), f"scenario {i}")


def test_one_group_over_a_large_batch_is_spread_over_the_chip():
    import torch

    from asyncflow_amd.runner import SimulationRunner

    seeds = 0xB16B0000 + np.arange(2100, dtype=np.uint64)
    res = SimulationRunner(simulation_input=lb_two_servers(horizon=600), seeds=seeds).run()
    a = res.pooled_summary()
    b = res.pooled_summary()
    got = a["stats"].cpu().numpy()[0]
    assert np.array_equal(got.view(np.uint64), b["stats"].cpu().numpy()[0].view(np.uint64))   # run-to-run identical
    clock = res._clock_t                                                                       # noqa: SLF001
    m = torch.as_tensor(res.counts[:, _abi.CNT_COMPLETED].astype(np.int64), device=clock.device).clamp(max=clock.shape[1])
    live = torch.arange(clock.shape[1], device=clock.device)[None, :] < m[:, None]
    lat = (clock[..., 1] - clock[..., 0])[live].cpu().numpy()                                 # scenario-major, in row order
    assert lat.size >= 150_000_000, lat.size
    _check(got, _np_stats(lat), "one group of 2 100 LB-2 replicas at T = 600")


def test_sweep_points_through_the_python_api(tmp_path):
    from asyncflow_amd import expand_grid
    from asyncflow_amd.results import load_summary
    from asyncflow_amd.runner import SimulationRunner

    users = "rqs_input.avg_active_users.mean"
    grid = expand_grid({users: [40.0, 120.0, 300.0], "topology_graph.edges[*].latency.mean": [0.002, 0.006]},
                       replicas=4, order_by_load=users)
    res = SimulationRunner(simulation_input=lb_two_servers(horizon=40), summary=True, **grid.runner_kwargs()).run()
    assert not np.array_equal(grid.point, np.sort(grid.point))          # members of a point are not contiguous
    cached = {k: (v.clone() if hasattr(v, "clone") else v) for k, v in res.summary().items()}
    p1 = res.pooled_summary(by=grid)
    p2 = res.pooled_summary(by=grid)
    st = p1["stats"].cpu().numpy()
    assert np.array_equal(st.view(np.uint64), p2["stats"].cpu().numpy().view(np.uint64))
    for g in range(st.shape[0]):
        members = np.nonzero(grid.point == g)[0]
        lat = np.concatenate([res[s].rqs_clock[:, 1] - res[s].rqs_clock[:, 0] for s in members])
        _check(st[g], _np_stats(lat), f"point {g}")
    assert p1["replicas"].tolist() == [4] * 6
    # the run's own summary is untouched by the pooled calls
    after = res.summary()
    for k in ("stats", "rps"):
        assert np.array_equal(after[k].cpu().numpy().view(np.uint8), cached[k].cpu().numpy().view(np.uint8)), k

    # aggregate(by=): per point, against numpy group-bys of the per-scenario statistics and of the RPS windows
    agg = res.aggregate(by=grid)
    per = cached["stats"].cpu().numpy()
    rps = cached["rps"].cpu().numpy().astype(np.float64)
    from statistics import NormalDist

    z = NormalDist().inv_cdf(0.975)
    for g in range(6):
        members = np.nonzero(grid.point == g)[0]
        body = per[members][per[members, 0] > 0]
        assert agg["n"][g] == body.shape[0]
        np.testing.assert_allclose(agg["mean"][g], body.mean(axis=0), rtol=1e-12)
        sd = body.std(axis=0, ddof=1)
        np.testing.assert_allclose(agg["std"][g], sd, rtol=1e-12)
        np.testing.assert_allclose(agg["ci_halfwidth"][g], z * sd / np.sqrt(body.shape[0]), rtol=1e-12)
        np.testing.assert_allclose(agg["rps_mean"][g], rps[members].mean(axis=0), rtol=1e-12)
        np.testing.assert_allclose(agg["rps_p05"][g], np.quantile(rps[members], 0.05, axis=0), rtol=1e-12)
        np.testing.assert_allclose(agg["rps_p95"][g], np.quantile(rps[members], 0.95, axis=0), rtol=1e-12)
    assert np.array_equal(agg["pooled"].view(np.uint64), st.view(np.uint64))
    # without by=: the whole-batch aggregate as before
    assert set(res.aggregate()) == {"n", "keys", "mean", "std", "ci_halfwidth", "level", "rps_mean", "rps_p05", "rps_p95"}

    # one row per point, both formats
    cols_p = grid.point_columns()
    for name in ("points.npz", "points.parquet"):
        written = res.save_point_summary(str(tmp_path / name), grid)
        back = load_summary(str(tmp_path / name))
        assert set(back) == set(written)
        for k, v in written.items():
            assert np.array_equal(np.asarray(back[k], dtype=v.dtype), v, equal_nan=v.dtype.kind == "f"), (name, k)
        for k, v in cols_p.items():
            assert np.array_equal(back[f"param:{k}"], v)
        assert np.array_equal(back["pooled:p95"], st[:, 4], equal_nan=True)
        assert back["rps_p95"].shape == (6, 40)


def test_pooled_summary_needs_the_clock_and_checks_groups():
    from asyncflow_amd.runner import SimulationRunner

    payload = lb_two_servers(horizon=10)
    seeds = 0x5EED0000 + np.arange(8, dtype=np.uint64)
    res = SimulationRunner(simulation_input=payload, seeds=seeds, collect_clock=False).run()
    with pytest.raises(RuntimeError, match="kept no rqs_clock"):
        res.pooled_summary()
    with pytest.raises(RuntimeError, match="kept no rqs_clock"):
        res.aggregate(by=np.zeros(8, dtype=np.int64))
    res = SimulationRunner(simulation_input=payload, seeds=seeds).run()
    with pytest.raises(ValueError, match="one id per scenario"):
        res.pooled_summary(np.zeros(7, dtype=np.int64))
