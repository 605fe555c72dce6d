"""The per-row rule, the chunk walk, the rolling condition and the mask steps of the alert analyzer on the host, under
AddressSanitizer + UBSan: tests/hostcheck/alerts_main.cpp is a stand-alone program over the plain-C++ routines of
asyncflow_amd/csrc/af_alerts.hpp (afal::row_tick, afal::rolling, afal::alert_cond, afal::hold_step, afal::cell_step and
afal::scenario_alerts: chunk by chunk with the prefix carried across the seams, step by step with the runs carried across the
64-tick seams).  It runs as a child process and everything it prints is compared with the host definition,
`asyncflow_amd.results.scenario_alerts`."""

from __future__ import annotations

import os
import re
import subprocess

import numpy as np
import pytest

from asyncflow_amd.results import scenario_alerts
from tests.alerts_util import HOLDS, SLO, P, firing_words, rows_in_phases, rules_32, rules_few
from tests.hostcheck import build as hc

_problem = hc.sanitizer_link_problem()
pytestmark = pytest.mark.skipif(_problem is not None, reason=str(_problem))

SRC = hc.HERE / "alerts_main.cpp"
HEADER = hc.ROOT / "asyncflow_amd/csrc/af_alerts.hpp"
CHUNK = int(re.search(r"constexpr uint32_t kChunkTicks = (\d+);", HEADER.read_text()).group(1))
CELLS = ("fired", "episodes", "longest", "longest_start", "first", "last")


@pytest.fixture(scope="module")
def program():
    exe = hc.SAN_DIR / "alerts_check"
    hc.SAN_DIR.mkdir(exist_ok=True)
    if not exe.exists() or exe.stat().st_mtime < max(SRC.stat().st_mtime, HEADER.stat().st_mtime):
        subprocess.run(["g++", *hc.SAN_FLAGS, "-Wall", "-o", str(exe), str(SRC)], check=True, capture_output=True, text=True)
    return exe


def _run(program, args: list[str], text: str) -> list[str]:
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}
    r = subprocess.run([str(program), *args], input=text.encode(), capture_output=True, env={**env, **hc.SAN_ENV}, timeout=240, check=False)
    err = r.stderr.decode()
    assert "ERROR: AddressSanitizer" not in err and "runtime error:" not in err, err[-4000:]
    assert r.returncode == 0, (r.returncode, err[-4000:])
    return r.stdout.decode().split("\n")


def _case(rows, t_s, chunk, rules, edges, period=P, slo=SLO) -> str:
    words = np.concatenate([[period, slo], np.asarray(rows, dtype=np.float64).reshape(-1)]).view(np.uint64)
    return (f"{len(rows)} {t_s} {chunk} {len(rules)} {len(edges) - 1}\n" + " ".join(f"{int(w):x}" for w in words) + "\n"
            + " ".join(str(int(v)) for r in rules for v in r) + "\n" + " ".join(str(int(e)) for e in edges) + "\n")


def _check(program, cases) -> None:
    lines = _run(program, [], "".join(_case(*c) for c in cases))
    assert len(lines) == 11 * len(cases) + 1 and lines[-1] == ""
    for j, c in enumerate(cases):
        rows, t_s, chunk, rules, edges = c[:5]
        want = scenario_alerts(rows, t_s, *(c[5:] or (P, SLO)), rules, edges)
        got = [np.array(line.split(), dtype=np.uint64) for line in lines[11 * j: 11 * j + 11]]
        assert int(got[0][0]) == (chunk or CHUNK)
        assert np.array_equal(got[1], want["total"]) and np.array_equal(got[2], want["bad"]), (j, "total / bad")
        assert np.array_equal(got[3], firing_words(want["firing"]).astype(np.uint64)), (j, "firing")
        assert np.array_equal(got[4], want["count"].astype(np.uint64)), (j, "count")
        for k, key in enumerate(CELLS):
            words = want[key].astype(np.int64).reshape(-1) & 0xFFFFFFFF                  # (-1: AF_TICK_NONE)
            assert np.array_equal(got[5 + k], words.astype(np.uint64)), (j, key, t_s, chunk)


def test_tick_counts_around_small_forced_chunks(program):
    rng = np.random.default_rng(21)
    rules = rules_few(8)
    cases = [(np.zeros((0, 2)), 0, 0, rules, [0, 5]), (np.zeros((0, 2)), 7, 3, rules, [0, 3, 9]), (np.array([[0.0, 1.0]]), 0, 4, rules, [2, 3])]
    for period in (P, 0.01, 1.0 / 3.0):
        for m, t_s, chunk in ((1, 1, 1), (40, 9, 4), (300, 33, 8), (900, 100, 7), (900, 100, 100), (900, 100, 101), (500, 64, 1), (2000, 501, 250)):
            rows = rows_in_phases(rng, m, t_s, 11) * (period / P)
            cases.append((rows, t_s, chunk, rules, [0, 1, 7, 8, 9, 64, 65, 100, 600], period, SLO * period / P))
    _check(program, cases)


def test_runs_across_the_64_tick_seams_and_every_hold(program):
    rng = np.random.default_rng(22)
    cases = []
    for t_s, phase in ((63, 20), (64, 20), (65, 20), (129, 64), (700, 150), (1300, 300)):
        rows = rows_in_phases(rng, 12 * t_s, t_s, phase)
        for edges in ([0, t_s], [0, 63, 64, 65, 128, 300, 301, 640, 2000], list(range(0, t_s + 3, 1 if t_s < 130 else 37))):
            cases.append((rows, t_s, 256, rules_32(256), edges))
    _check(program, cases)
    long_runs = scenario_alerts(cases[-1][0], 1300, P, SLO, rules_32(256), [0, 1300])
    held = {int(h): long_runs["fired"][0, r] for r, h in enumerate(long_runs["rules"][:, 5])}
    assert all(held[h] > 0 for h in HOLDS) and long_runs["longest"].max() > 128             # runs span several steps, hold 200 is met


def test_look_backs_longer_than_the_kernels_chunk_and_than_the_run(program):
    rng = np.random.default_rng(23)
    cases = []
    for t_s in (CHUNK - 1, CHUNK + 1, 2 * CHUNK + 3):
        rows = rows_in_phases(rng, 6000, t_s, 3000)
        cases.append((rows, t_s, 0, rules_few(CHUNK), [0, 100, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 2 * CHUNK + 100]))
    _check(program, cases)


def test_hold_step_masks(program):
    rng = np.random.default_rng(24)
    text, want = "", []
    for hold in HOLDS + (3, 130):
        for density in (0.5, 0.9, 0.99, 1.0):
            n = 6
            cond = rng.random(64 * n) < density
            masks = [sum(1 << j for j in range(64) if cond[64 * k + j]) for k in range(n)]
            text += f"{hold} {n}\n" + " ".join(f"{v:x}" for v in masks) + "\n"
            run, out = 0, []
            firing = np.zeros(64 * n, dtype=bool)
            for k in range(64 * n):
                run = run + 1 if cond[k] else 0
                firing[k] = run >= hold
            out = [f"{sum(1 << j for j in range(64) if firing[64 * k + j]):x}" for k in range(n)]
            want.append(" ".join(out) + f" {run}")
    assert _run(program, ["hold"], text)[:-1] == want
