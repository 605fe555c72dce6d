"""select()'s lane window with a width of its own per station list (af_flow.hpp: Flow::select_regs, AF_SELECT_WINDOW_S0 .. _S3)
against the bucket rank it stands in for.

The host instantiation of the kernel is built into tests/select_widths/build/ with the default widths, with every list at width
1, 2 and 4 -- narrow windows fail their proof often, so both ranks run inside one scenario --, with four different widths (each
list then has its own copy of select_regs), and without the window at all (-DAF_SELECT_WINDOW=0).  All builds are held to each
other and to the oracle, bit for bit, on the six scenarios of tests/test_flow_select_window.py and on its tie quantum.  A
stand-alone program (tests/select_widths/select_widths_main.cpp) drives the selection itself on crafted lists in every build and
once more under AddressSanitizer + UBSan, and holds every call to the path it must take at the width of its list."""

from __future__ import annotations

import hashlib
import os
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
DIR = HERE / "select_widths"
OUT = DIR / "build"
MAIN = DIR / "select_widths_main.cpp"
HOST_FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall"]   # tests/hostcheck/build.py's line


def _widths(*w: int) -> list[str]:
    return [f"-DAF_SELECT_WINDOW_S{s}={w[s % len(w)]}" for s in range(4)]


FORMS: dict[str, list[str]] = {
    "bucket": ["-DAF_SELECT_WINDOW=0", *_widths(4)],      # (AF_SELECT_WINDOW=0 switches the window off whatever the lists say)
    "default": [],
    "w1": _widths(1),
    "w2": _widths(2),
    "w4": _widths(4),
    "mixed": _widths(2, 4, 1, 6),
}
WANT_WIDTHS = {"bucket": "0 0 0 0", "w1": "1 1 1 1", "w2": "2 2 2 2", "w4": "4 4 4 4", "mixed": "2 4 1 6"}
REFERENCE_FORM = "bucket"
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
    """Every host library, every program and the sanitized program, compiled side by side."""
    jobs = {}
    for form, defs in FORMS.items():
        jobs[f"lib_{form}"] = (OUT / f"libaf_hostcheck_{form}.so", ["g++", *HOST_FLAGS, "-fPIC", "-shared", *defs, str(hc.HERE / "hostcheck.cpp")])
        jobs[f"exe_{form}"] = (OUT / f"select_widths_{form}", ["g++", *HOST_FLAGS, *defs, str(MAIN)])
    if hc.sanitizer_link_problem() is None:
        jobs["exe_sanitized"] = (OUT / "select_widths_sanitized", ["g++", *hc.SAN_FLAGS, *FORMS["mixed"], str(MAIN)])
    with ThreadPoolExecutor(min(len(jobs), os.cpu_count() or 4)) as pool:
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


SCENARIOS = {   # the six of tests/test_flow_select_window.py
    "lb2_own_t60": lambda: _lb2(400, None, 60),
    "lb2_users1000_edges50ms_t20": lambda: _lb2(1000, 0.05, 20),      # the proof fails in nearly every call
    "lb2_users400_edges20ms_t40": lambda: _lb2(400, 0.02, 40),        # mixed
    "lb2_users10_t120": lambda: _lb2(10, None, 120),                  # lists far below 64 entries
    "single_server_t60": lambda: single_server(horizon=60),           # no LB station
    "lb2_events_t60": lambda: lb_with_events(users=300, horizon=60, scale=0.1),   # the FEAT_MARKS form
}
FLOW_KW = (dict(ipl=1, far=False), dict(ipl=1, far=True))   # the instantiations that have the window: lean and FEAT_FAR [| MARKS]


def _run_all(host_form, plan, seed: int, **kw):
    """The run in every build; all equal the build without the window word for word.  Returns that build's outputs."""
    got = {}
    for form in FORMS:
        host_form(form)
        got[form] = hc.flow_simulate(plan, seed, **kw)
        assert got[form] is not None, (form, hc.flow_reason())
    ref = got[REFERENCE_FORM]
    for form, g in got.items():
        assert np.array_equal(g[0], ref[0]), (form, kw, g[0], ref[0])                              # counts, flags and `why` bits included
        assert np.array_equal(g[1].view(np.uint64), ref[1].view(np.uint64)), (form, kw)            # rqs_clock
        assert np.array_equal(g[2], ref[2]), (form, kw)                                            # every sample word
    return ref


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_every_width_equals_the_bucket_rank_and_the_oracle(name, host_form):
    plan = lower(SCENARIOS[name]())
    want = ol.simulate(plan, SEED)
    assert not int(want.counts[_abi.CNT_FLAGS]) & _abi.FATAL_FLAGS and int(want.counts[_abi.CNT_COMPLETED]) > 0
    checked = 0
    for kw in FLOW_KW:
        counts, clock, samples = _run_all(host_form, plan, SEED, **kw)
        if int(counts[_abi.CNT_FLAGS]) & hc.FLOW_FALLBACK:     # (the lean form hands a delivery beyond its tick ring back)
            continue
        assert np.array_equal(want.counts[:5].astype(np.uint32), counts[:5]), kw
        assert np.array_equal(want.clock.view(np.uint64), clock.view(np.uint64)), kw
        assert np.array_equal(want.samples, samples), kw
        checked += 1
    assert checked >= 1


def test_equal_keys_are_handed_back_alike_at_every_width(host_form):
    """The tie quantum of tests/test_flow_select_window.py: delivery times on a grid.  Every build hands back the same scenarios
    with the same `why` bits."""
    tie_bit = next(b for b, n in hc.FLOW_WHY.items() if n == "tie")

    def quantum(bits: int) -> None:      # (the switch lives in the library: each has its own)
        for form in FORMS:
            host_form(form)
            hc.set_test_quantum(bits)

    handed_back = 0
    plan = lower(lb_two_servers(horizon=15))
    quantum(12)
    try:
        for seed in range(4):
            for kw in FLOW_KW:
                counts, _, _ = _run_all(host_form, plan, seed, clock_capacity=4 * plan.clock_capacity(),
                                        draw_capacity=4 * plan.clock_capacity(), **kw)
                handed_back += bool(int(counts[_abi.CNT_FLAGS]) & tie_bit)
    finally:
        quantum(0)
    assert handed_back >= 1


def _lines(exe: Path, *args: str, env: dict | None = None) -> list[str]:
    r = subprocess.run([str(exe), *args], capture_output=True, text=True, check=False, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    return r.stdout.splitlines()


def test_crafted_lists_at_every_width(built):
    """Every case equals the scalar restatement in each build and takes the path it must at the width of its list (the program's
    own checks, from the emulator's counters); all builds print the same output words."""
    ref = _lines(built[f"exe_{REFERENCE_FORM}"])
    assert len(ref) >= 16 * 7
    for form in FORMS:
        widths = _lines(built[f"exe_{form}"], "--widths")[0]
        if form in WANT_WIDTHS:
            assert widths == WANT_WIDTHS[form], form
        else:
            assert "0" not in widths.split(), (form, widths)     # the default: a window in every list
        assert _lines(built[f"exe_{form}"]) == ref, form


def test_crafted_lists_under_the_sanitizers(built):
    if "exe_sanitized" not in built:
        pytest.skip(hc.sanitizer_link_problem())
    assert _lines(built["exe_sanitized"], env={**os.environ, **hc.SAN_ENV}) == _lines(built["exe_mixed"])
