"""Arrivals per window on the host: the definitions `af_engine_summarize_arrivals` is held to.

`asyncflow_amd.results.arrival_times` restates the reference's windowed sampler with its two clocks; it must give, bit for bit,
what `af::gen_next_gap` -- the sequential statement the oracle and the device follow -- gives (tests/hostcheck), and through the
oracle what a simulated run consumed: as many arrivals as it counts, and every `start` of its clock among them.
`arrival_window_counts` is the bucket rule.  The per-row logic of the kernel (asyncflow_amd/csrc/af_arrival_counts.hpp) runs here
as a stand-alone program under AddressSanitizer + UBSan on the same hand-made rows."""

from __future__ import annotations

import ctypes as C
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from asyncflow_amd import _abi
from asyncflow_amd.plan import lower
from asyncflow_amd.results import arrival_times, arrival_window_counts, spec_log
from oracle import oracle_lib as ol
from oracle import ref_env
from oracle.rng_adapter import GeneratorRNG
from oracle.scenarios import lb_two_servers, overload, single_server
from tests.hostcheck import build as hc

ROOT = Path(__file__).resolve().parent.parent
POISSON, NORMAL = 0, 1
INF = float("inf")


def _same(seed, **kw):
    """arrival_times against the three host instantiations of the sampler; -> (arrivals, flags)"""
    got, flags = arrival_times(GeneratorRNG(seed), kw["dist"], kw["mean"], kw["sigma"], kw["rpm"], kw["window_s"], kw["horizon"], kw["n_draw"])
    assert got.shape == (kw["n_draw"],) and got.dtype == np.float64
    for which in (0, 1, 2):
        n, want, f = hc.arrivals(which, seed, **kw)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (which, seed, kw)
        assert (int(np.isfinite(got).sum()), flags) == (n, f), (which, seed, kw)
    m = int(np.isfinite(got).sum())
    assert np.all(np.diff(got[:m]) > 0.0) and np.all(np.isposinf(got[m:]))     # ascending, +inf behind the last arrival
    return m, flags


@pytest.mark.parametrize("dist", [POISSON, NORMAL])
def test_arrival_times_are_the_sequential_sampler_bit_for_bit(dist):
    rng = np.random.default_rng(20261020 + dist)
    total = 0
    for case in range(24):
        horizon = float(rng.choice([5, 30, 61]))
        window = float(rng.choice([1, 2, 7, 60]))
        mean = float(rng.choice([0.3, 3, 40]))            # 0.3 users: most sampling windows are empty, the sampler's clock jumps
        rpm = float(rng.choice([5, 20, 90]))
        expected = mean * rpm / 60.0 * horizon
        n_draw = int(expected * 1.5 + 6.0 * np.sqrt(expected + 1.0) + 64)
        n, flags = _same(int(rng.integers(1, 2**62)) + case, dist=dist, mean=mean, sigma=mean * 0.4, rpm=rpm, window_s=window,
                         horizon=horizon, n_draw=n_draw)
        assert flags == 0
        total += n
    assert total > 3000


def test_arrival_times_edge_cases():
    kw = dict(dist=POISSON, mean=50.0, sigma=0.0, rpm=60.0, window_s=5.0, horizon=30.0)
    n, flags = _same(7, **kw, n_draw=200)                                   # the row fills up: the prefix, and the flag
    assert (n, flags) == (200, _abi.FLAG_DRAW_OVERFLOW)
    n_exact, flags = _same(7, **kw, n_draw=4000)
    assert flags == 0 and 200 < n_exact < 4000
    assert _same(7, **kw, n_draw=n_exact) == (n_exact, 0)                   # exactly full is not an overflow
    assert _same(7, **kw, n_draw=n_exact - 1) == (n_exact - 1, _abi.FLAG_DRAW_OVERFLOW)
    assert _same(3, dist=POISSON, mean=0.0, sigma=0.0, rpm=60.0, window_s=1.0, horizon=20.0, n_draw=64) == (0, 0)
    n, _ = _same(11, dist=NORMAL, mean=30.0, sigma=10.0, rpm=30.0, window_s=500.0, horizon=20.0, n_draw=1024)   # a window longer than the horizon
    assert n > 100
    n, _ = _same(12, dist=POISSON, mean=0.3, sigma=0.0, rpm=30.0, window_s=1.0, horizon=120.0, n_draw=256)      # most windows empty
    assert 0 < n < 60
    with pytest.raises(ValueError, match="poisson"):
        arrival_times(GeneratorRNG(1), "uniform", 1.0, 0.0, 1.0, 1.0, 1.0, 8)


def test_spec_log_is_the_oracles_logarithm():
    rng = np.random.default_rng(5)
    x = np.concatenate([1.0 - rng.random(4000), rng.random(500) * 1e-12, [1.0, 1e-15, 1.0 - 1e-15, 5e-324, 2.5, 1e300]])
    lib = ol.lib()
    for v in x:
        assert spec_log(float(v)) == lib.orc_x_log(float(v)), v
    for bad in (0.0, -1.0, INF, float("nan")):
        with pytest.raises(ValueError):
            spec_log(bad)


def _plan_row(plan, seed, n_draw):
    return arrival_times(GeneratorRNG(seed), plan.gen_users_dist, plan.gen_users_mean, plan.gen_users_sigma, plan.gen_rpm_mean,
                         plan.gen_window_s, plan.total_time, n_draw)


@pytest.mark.parametrize("payload", [single_server(50), lb_two_servers(40), overload(30)], ids=["single_server", "lb_two_servers", "overload"])
@pytest.mark.parametrize("seed", [1, 42, 777])
def test_a_simulated_run_consumed_exactly_these_arrivals(payload, seed):
    plan = lower(payload)
    res = ol.simulate(plan, seed)
    times, flags = _plan_row(plan, seed, plan.clock_capacity())
    assert flags == 0
    m = int(np.isfinite(times).sum())
    assert m == res.generated
    assert np.isin(res.clock[:, 0].view(np.uint64), times[:m].view(np.uint64)).all()      # every start, bit for bit
    assert res.completed + res.dropped <= m
    # the cohorts' completions never exceed their arrivals, in any window
    edges = np.linspace(0.0, plan.total_time, 11)
    sent = np.diff(arrival_window_counts(times, edges))
    done = np.diff(np.searchsorted(np.sort(res.clock[:, 0]), edges, side="right"))
    assert np.all(done <= sent) and int(sent.sum()) == m


def test_overload_loses_most_of_what_it_is_sent():
    plan = lower(overload(30))
    res = ol.simulate(plan, 1)
    times, _ = _plan_row(plan, 1, plan.clock_capacity())
    assert (int(np.isfinite(times).sum()), res.completed, res.dropped) == (3718, 719, 59)


@pytest.fixture
def reference_importable():
    """The reference on sys.path for ONE test: asyncflow_amd.payload validates with the reference's models wherever they are
    importable, so leaving them behind would change what every later test of this process sees."""
    import sys

    path, modules = list(sys.path), set(sys.modules)
    ref_env.install()
    yield
    sys.path[:] = path
    for name in set(sys.modules) - modules:
        if name == "asyncflow" or name.startswith("asyncflow."):
            del sys.modules[name]


@pytest.mark.skipif(not ref_env.reference_available(), reason="the reference checkout is not on this machine")
@pytest.mark.filterwarnings("ignore::DeprecationWarning")
@pytest.mark.parametrize("dist", ["poisson", "normal"])
def test_against_the_references_own_sampler(dist, reference_importable):
    import types

    from asyncflow.samplers import gaussian_poisson, poisson_poisson
    from asyncflow.schemas.settings.simulation import SimulationSettings
    from asyncflow.schemas.workload.rqs_generator import RqsGenerator

    users = {"mean": 0.8, "distribution": "poisson"} if dist == "poisson" else {"mean": 12.0, "distribution": "normal", "variance": 5.0}
    gen = RqsGenerator.model_validate({"id": "rqs-1", "avg_active_users": users, "avg_request_per_minute_per_user": {"mean": 45.0},
                                       "user_sampling_window": 3})
    settings = SimulationSettings.model_validate({"total_simulation_time": 40})
    module, fn = (poisson_poisson, poisson_poisson.poisson_poisson_sampling) if dist == "poisson" else \
                 (gaussian_poisson, gaussian_poisson.gaussian_poisson_sampling)
    saved = module.math
    module.math = types.SimpleNamespace(log=ol.lib().orc_x_log)        # the one substitution of the golden runs (oracle/reference_runner.py)
    try:
        for seed in (1, 42, 777):
            t, ref = 0.0, []
            for gap in fn(gen, settings, rng=GeneratorRNG(seed)):
                t = t + gap                                            # rqs_generator.py: env.now + gap
                ref.append(t)
            got, flags = arrival_times(GeneratorRNG(seed), dist, users["mean"], users.get("variance", 0.0), 45.0, 3.0, 40.0, len(ref) + 5)
            assert flags == 0 and len(ref) > 10
            assert np.array_equal(got[: len(ref)].view(np.uint64), np.asarray(ref).view(np.uint64)) and np.all(np.isposinf(got[len(ref):]))
    finally:
        module.math = saved


# ---- the bucket rule on hand-made rows -----------------------------------------------------------------------------------
def _row(values, n_draw):
    out = np.full(n_draw, INF)
    out[: len(values)] = values
    return out


HAND_MADE = [
    # (row, n_draw, edges, bounds)
    ([1.0, 2.0, 3.0], 4, [0.0, 2.0, 4.0], [0, 2, 3]),                          # an arrival ON an edge belongs to the window that ends there
    ([1.0, 2.0, 2.0, 2.0, 3.0], 8, [1.0, 2.0, 2.5], [1, 4, 4]),                # duplicates on an edge; the first edge on an arrival
    ([0.5, 0.5, 1.5, 1.5, 1.5, 9.0], 6, [0.5, 1.5], [2, 5]),                   # duplicates across an edge, a full row
    ([1.0, 2.0, 3.0, 4.0, 5.0], 5, [2.5, 3.5, 4.5], [2, 3, 4]),                # e[0] above some arrivals, e[W] below some
    ([], 3, [0.0, 1.0, 2.0], [0, 0, 0]),                                       # an empty row
    ([5.0], 1, [0.0, 1.0], [0, 0]),                                            # everything beyond the last edge
    ([5.0], 2, [6.0, 7.0, 8.0], [1, 1, 1]),                                    # everything before the first
    ([0.0, 5e-324, 1.0], 3, [-1.0, 0.0, 5e-324, 1.0], [0, 1, 2, 3]),           # an arrival at time zero; a subnormal step
]


@pytest.mark.parametrize(("values", "n_draw", "edges", "bounds"), HAND_MADE)
def test_arrival_window_counts_on_hand_made_rows(values, n_draw, edges, bounds):
    got = arrival_window_counts(_row(values, n_draw), edges)
    assert got.dtype == np.int64 and got.tolist() == bounds
    assert got.tolist() == np.searchsorted(np.asarray(values, dtype=np.float64), edges, side="right").tolist()


def test_arrival_window_counts_refusals():
    with pytest.raises(ValueError):
        arrival_window_counts([2.0, 1.0], [0.0, 3.0])
    with pytest.raises(ValueError):
        arrival_window_counts([1.0], [0.0, 0.0])


# ---- the kernel's per-row logic as a stand-alone program under the sanitizers ---------------------------------------------
SRC = hc.HERE / "arrival_counts_main.cpp"
HEADER = ROOT / "asyncflow_amd" / "csrc" / "af_arrival_counts.hpp"


def _sanitized_program() -> Path:
    """tests/hostcheck/build/arrival_counts: arrival_counts_main.cpp with the sanitizer flags of the other host programs, cached
    by mtime."""
    exe = hc.SAN_DIR / "arrival_counts"
    hc.SAN_DIR.mkdir(exist_ok=True)
    if not exe.exists() or exe.stat().st_mtime < max(SRC.stat().st_mtime, HEADER.stat().st_mtime):
        subprocess.run(["g++", *hc.SAN_FLAGS, "-Wall", "-o", str(exe), str(SRC)], check=True, capture_output=True, text=True)
    return exe


def _run_rows(cases):
    """cases: (row [n_draw], edges [W + 1], force) -> per case (length, streamed, bounds)"""
    text = []
    for row, edges, force in cases:
        words = np.concatenate([np.asarray(row, dtype=np.float64), np.asarray(edges, dtype=np.float64)]).view(np.uint64)
        text.append(f"{len(row)} {len(edges) - 1} {force}\n" + " ".join(f"{int(w):x}" for w in words) + "\n")
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS", "LD_PRELOAD")}
    r = subprocess.run([str(_sanitized_program())], input="".join(text).encode(), capture_output=True, env={**env, **hc.SAN_ENV},
                       timeout=240, check=False)
    err = r.stderr.decode()
    assert "ERROR: AddressSanitizer" not in err and "runtime error:" not in err, err[-4000:]
    assert r.returncode == 0, (r.returncode, err[-4000:])
    lines = r.stdout.decode().splitlines()
    assert len(lines) == len(cases)
    return [(int(w[0]), int(w[1]), [int(v) for v in w[2:]]) for w in (ln.split() for ln in lines)]


@pytest.mark.skipif(hc.sanitizer_link_problem() is not None, reason=str(hc.sanitizer_link_problem()))
def test_row_logic_under_the_sanitizers():
    rng = np.random.default_rng(99)
    cases, want = [], []
    for values, n_draw, edges, bounds in HAND_MADE:
        for force in (0, 1, 2):
            cases.append((_row(values, n_draw), edges, force))
            want.append((len(values), bounds))
    # rows around the wave's seams with many and few windows: both sides of the rule, edges on arrivals, duplicates, outside edges
    for m in (0, 1, 63, 64, 65, 255, 256, 257, 1000):
        for n_win in (1, 2, 63, 64, 65, 600):
            vals = np.sort(rng.integers(0, 4 * n_win + 8, m).astype(np.float64) / 4.0)
            edges = np.arange(n_win + 1) * 1.0 + rng.choice([0.0, 0.25, -3.0, 2.0])
            for n_draw in (m, m + 1, m + 70):
                if n_draw == 0:
                    continue
                for force in (0, 1, 2):
                    cases.append((_row(vals, n_draw), edges, force))
                    want.append((m, np.searchsorted(vals, edges, side="right").tolist()))
    got = _run_rows(cases)
    streamed = set()
    for (row, edges, force), (m, s, b), (wm, wb) in zip(cases, got, want):
        assert (m, b) == (wm, wb), (len(row), len(edges), force)
        streamed.add(s)
    assert streamed == {0, 1}                                                   # the rule took both ways


# ---- the ABI ------------------------------------------------------------------------------------------------------------------
def test_symbol_is_exported_and_the_struct_matches_the_header():
    header = (ROOT / "include" / "asyncflow_hip.h").read_text()
    assert "af_engine_summarize_arrivals" in _abi.EXPORTED_SYMBOLS
    assert re.search(r"int\s+af_engine_summarize_arrivals\(af_engine_t\*\s*\w+,\s*const af_sweep_t\*\s*\w+,\s*af_arrivals_t\*\s*\w+\);", header)
    assert re.search(r"#define\s+AF_ABI_VERSION\s+7\b", header) and _abi.AF_ABI_VERSION == 7
    body = re.search(r"typedef struct af_arrivals \{(.*?)\} af_arrivals_t;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "double": C.c_double}
    fields = []
    for decl in (d.strip() for d in body.split(";") if d.strip()):
        m = re.fullmatch(r"(const\s+)?(\w+)\s*(\*?)\s*(\w+)", decl)
        assert m, decl
        fields.append((m.group(4), "pointer" if m.group(3) else ctype[m.group(2)]))
    mirror = [(name, "pointer" if t in (C.c_void_p, C.POINTER(C.c_double)) else t) for name, t in _abi.AfArrivals._fields_]   # noqa: SLF001
    assert fields == mirror
    from asyncflow_amd import build as af_build
    from asyncflow_amd.engine import load_library

    af_build.build()
    lib = load_library()
    assert hasattr(lib, "af_engine_summarize_arrivals")
    # refusals that need no device: a planning-only engine, NULL arguments
    plan = lower(single_server(horizon=5)).as_ctypes()
    h = C.c_void_p()
    assert lib.af_engine_create(C.byref(plan), _abi.DEVICE_PLAN_ONLY, None, C.byref(h)) == _abi.AF_OK
    try:
        seeds = (C.c_uint64 * 1)(1)
        edges = (C.c_double * 2)(0.0, 1.0)
        sweep = _abi.AfSweep(1, seeds, 0, None, 64)
        req = _abi.AfArrivals(1, 1, 1, None, edges, None, 0, C.c_void_p(8), None, None, None, 0.0, 0)
        assert lib.af_engine_summarize_arrivals(h, C.byref(sweep), C.byref(req)) == _abi.AF_ERR_NO_DEVICE
        assert lib.af_engine_summarize_arrivals(h, None, C.byref(req)) == _abi.AF_ERR_INVALID
    finally:
        lib.af_engine_destroy(h)
