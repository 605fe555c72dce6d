"""select()'s lane window (af_flow.hpp: Flow::select_regs, AF_SELECT_WINDOW) against the bucket rank it stands in for.

The host instantiation of the kernel is built twice into tests/select_window/build/ -- with the window (the default) and with
-DAF_SELECT_WINDOW=0 -- and the two are held to each other and to the oracle, bit for bit, on runs whose lists are nearly
sorted (the window ranks them), far from sorted (the proof fails and the bucket rank takes over), mixed, short, and full of
equal keys.  A stand-alone program (tests/select_window/select_window_main.cpp) drives the selection itself on crafted
lists, in both builds and once more under AddressSanitizer + UBSan."""

from __future__ import annotations

import hashlib
import subprocess
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import pytest

from asyncflow_amd import _abi
from asyncflow_amd.plan import lower
from asyncflow_amd.workloads import lb_two_servers, lb_with_events, single_server
from oracle import oracle_lib as ol
from tests.hostcheck import build as hc

HERE = Path(__file__).resolve().parent
DIR = HERE / "select_window"
OUT = DIR / "build"
MAIN = DIR / "select_window_main.cpp"
HOST_FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall"]   # tests/hostcheck/build.py's line
FORMS = {"window": [], "bucket": ["-DAF_SELECT_WINDOW=0"]}
SEED = 0x5EED0000


def _digest(extra: str) -> str:
    h = hashlib.sha1(extra.encode())  # noqa: S324 - a change detector
    for p in [*hc._sources(), MAIN]:  # noqa: SLF001
        h.update(p.read_bytes())
    return h.hexdigest()[:16]


def _compile(out: Path, cmd: list[str]) -> Path:
    """`cmd` -> `out`, unless `out` was built by this very command from these very sources."""
    stamp = out.with_suffix(out.suffix + ".stamp")
    want = _digest(" ".join(cmd))
    if not (out.exists() and stamp.exists() and stamp.read_text() == want):
        OUT.mkdir(parents=True, exist_ok=True)
        r = subprocess.run([*cmd, "-o", str(out)], capture_output=True, text=True, check=False)
        assert r.returncode == 0, r.stderr[-4000:]
        stamp.write_text(want)
    return out


@pytest.fixture(scope="module")
def built() -> dict[str, Path]:
    """Both host libraries, both programs and the sanitized program, compiled side by side."""
    jobs = {}
    for form, defs in FORMS.items():
        jobs[f"lib_{form}"] = (OUT / f"libaf_hostcheck_{form}.so", ["g++", *HOST_FLAGS, "-fPIC", "-shared", *defs, str(hc.HERE / "hostcheck.cpp")])
        jobs[f"exe_{form}"] = (OUT / f"select_window_{form}", ["g++", *HOST_FLAGS, *defs, str(MAIN)])
    if hc.sanitizer_link_problem() is None:
        jobs["exe_sanitized"] = (OUT / "select_window_sanitized", ["g++", *hc.SAN_FLAGS, str(MAIN)])
    with ThreadPoolExecutor(len(jobs)) as pool:
        paths = list(pool.map(lambda j: _compile(*j), jobs.values()))
    return dict(zip(jobs, paths))


@pytest.fixture
def host_form(built, monkeypatch):
    """form -> tests.hostcheck.build loads THAT library (its own loader, argument types included)."""
    def use(form: str) -> None:
        monkeypatch.setattr(hc, "LIB", built[f"lib_{form}"])
        monkeypatch.setattr(hc, "_lib", None)
        hc.lib()
    return use


def _lb2(users: float, mean: float | None, horizon: int) -> dict:
    p = lb_two_servers(users=users, horizon=horizon)
    if mean is not None:
        for e in p["topology_graph"]["edges"]:
            e["latency"]["mean"] = mean
    return p


SCENARIOS = {
    "lb2_own_t60": lambda: _lb2(400, None, 60),
    "lb2_users1000_edges50ms_t20": lambda: _lb2(1000, 0.05, 20),      # the proof fails in nearly every call
    "lb2_users400_edges20ms_t40": lambda: _lb2(400, 0.02, 40),        # mixed
    "lb2_users10_t120": lambda: _lb2(10, None, 120),                  # lists far below 64 entries
    "single_server_t60": lambda: single_server(horizon=60),           # no LB station
    "lb2_events_t60": lambda: lb_with_events(users=300, horizon=60, scale=0.1),   # the FEAT_MARKS form
}
FLOW_KW = (dict(ipl=1, far=False), dict(ipl=1, far=True))   # the instantiations that have the window: lean and FEAT_FAR [| MARKS]


def _run_both(host_form, plan, seed: int, **kw):
    got = {}
    for form in FORMS:
        host_form(form)
        got[form] = hc.flow_simulate(plan, seed, **kw)
        assert got[form] is not None, hc.flow_reason()
    w, b = got["window"], got["bucket"]
    assert np.array_equal(w[0], b[0]), (kw, w[0], b[0])                                   # counts, flags and `why` bits included
    assert np.array_equal(w[1].view(np.uint64), b[1].view(np.uint64)), kw                 # rqs_clock
    assert np.array_equal(w[2], b[2]), kw                                                 # every sample word
    return w


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_window_and_bucket_rank_equal_each_other_and_the_oracle(name, host_form):
    plan = lower(SCENARIOS[name]())
    want = ol.simulate(plan, SEED)
    assert not int(want.counts[_abi.CNT_FLAGS]) & _abi.FATAL_FLAGS and int(want.counts[_abi.CNT_COMPLETED]) > 0
    checked = 0
    for kw in FLOW_KW:
        counts, clock, samples = _run_both(host_form, plan, SEED, **kw)
        if int(counts[_abi.CNT_FLAGS]) & hc.FLOW_FALLBACK:     # (the lean form hands a delivery beyond its tick ring back)
            continue
        assert np.array_equal(want.counts[:5].astype(np.uint32), counts[:5]), kw
        assert np.array_equal(want.clock.view(np.uint64), clock.view(np.uint64)), kw
        assert np.array_equal(want.samples, samples), kw
        checked += 1
    assert checked >= 1


def test_equal_keys_inside_a_window_are_handed_back_alike(host_form):
    """The test quantum of test_exact_ties_by_the_thousand_follow_simpy_order: delivery times on a grid, so equal keys sit
    next to each other in the lists.  Both builds hand back the same scenarios with the same `why` bits."""
    tie_bit = next(b for b, n in hc.FLOW_WHY.items() if n == "tie")

    def quantum(bits: int) -> None:      # (the switch lives in the library: each of the two has its own)
        for form in FORMS:
            host_form(form)
            hc.set_test_quantum(bits)

    handed_back = 0
    plan = lower(lb_two_servers(horizon=15))
    quantum(12)
    try:
        for seed in range(4):
            for kw in FLOW_KW:
                counts, _, _ = _run_both(host_form, plan, seed, clock_capacity=4 * plan.clock_capacity(),
                                         draw_capacity=4 * plan.clock_capacity(), **kw)
                handed_back += bool(int(counts[_abi.CNT_FLAGS]) & tie_bit)
    finally:
        quantum(0)
    assert handed_back >= 1


def _lines(exe: Path, *args: str, env: dict | None = None) -> list[str]:
    r = subprocess.run([str(exe), *args], capture_output=True, text=True, check=False, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    return r.stdout.splitlines()


def test_crafted_lists_both_forms_and_the_path_taken(built):
    """Every case equals the scalar restatement in each build and takes the path it must (the program's own checks); the
    output words of the two builds are the same."""
    width = _lines(built["exe_window"], "--width")[0]      # (the lists are crafted around the window's width: the same for both)
    assert int(width) >= 4
    w, b = _lines(built["exe_window"], width), _lines(built["exe_bucket"], width)
    assert len(w) >= 15 * 4 and w == b


def test_crafted_lists_under_the_sanitizers(built):
    if "exe_sanitized" not in built:
        pytest.skip(hc.sanitizer_link_problem())
    import os

    assert _lines(built["exe_sanitized"], env={**os.environ, **hc.SAN_ENV}) == _lines(built["exe_window"])
