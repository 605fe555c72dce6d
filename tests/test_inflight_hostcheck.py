"""The per-row logic and the chunk walk of the in-flight analyzer on the host, under AddressSanitizer + UBSan:
tests/hostcheck/inflight_main.cpp is a stand-alone program over the plain-C++ routines of asyncflow_amd/csrc/af_inflight.hpp
(afif::row_ticks: the quotient, the rejections, the clipping; afif::chunk_hit and afif::scenario_series: the walk chunk by chunk
with the carry across the seams; afif::bin_of).  It runs as a child process and everything it prints is compared with
`asyncflow_amd.results.in_flight_series`, the host definition."""

from __future__ import annotations

import os
import re
import subprocess

import numpy as np
import pytest

from asyncflow_amd.results import in_flight_series
from tests.hostcheck import build as hc

_problem = hc.sanitizer_link_problem()
pytestmark = pytest.mark.skipif(_problem is not None, reason=str(_problem))

SRC = hc.HERE / "inflight_main.cpp"
HEADER = hc.ROOT / "asyncflow_amd/csrc/af_inflight.hpp"
CHUNK = int(re.search(r"constexpr uint32_t kChunkTicks = (\d+);", HEADER.read_text()).group(1))


@pytest.fixture(scope="module")
def program():
    exe = hc.SAN_DIR / "inflight_check"
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
    return r.stdout.decode().splitlines()


def _case(rows: np.ndarray, t_s: int, chunk: int, period: float) -> str:
    words = np.concatenate([[period], np.asarray(rows, dtype=np.float64).reshape(-1)]).view(np.uint64)
    return f"{len(rows)} {t_s} {chunk}\n" + " ".join(f"{int(w):x}" for w in words) + "\n"


def _check(program, cases: list[tuple[np.ndarray, int, int, float]]) -> None:
    lines = _run(program, [], "".join(_case(*c) for c in cases))
    assert len(lines) == 4 * len(cases)
    for j, (rows, t_s, chunk, period) in enumerate(cases):
        want = in_flight_series(rows, t_s, period)
        last, used = (int(v) for v in lines[4 * j].split())
        assert used == (chunk or CHUNK)
        for k, key in enumerate(("started", "finished", "in_flight")):
            got = np.array(lines[4 * j + 1 + k].split(), dtype=np.uint64)
            assert got.shape[0] == t_s and np.array_equal(got, want[key].astype(np.uint64)), (j, key, t_s, chunk)
        assert last == (int(want["in_flight"][-1]) if t_s else 0)


def _rows(rng: np.random.Generator, m: int, t_s: int, period: float) -> np.ndarray:
    """Starts on and beside the tick instants from before the first sample to past the last; latencies 0, below a tick, one
    tick, many ticks, past the end; NaN, negative, infinite and reversed rows mixed in."""
    start = rng.integers(-8, 4 * (t_s + 6), m) * (period / 4.0) + rng.choice([0.0, 0.0, period * 2.0 ** -30, -period * 2.0 ** -30], m)
    lat = rng.choice([0.0, period / 4, period / 2, period, 3 * period, 40 * period, (t_s + 50) * period, 1e300, np.inf], m,
                     p=[0.1, 0.1, 0.1, 0.15, 0.2, 0.2, 0.1, 0.025, 0.025])
    rows = np.stack([start, start + lat], axis=1)
    for k, bad in enumerate(([np.nan, 1.0], [1.0, np.nan], [-period, 5 * period], [3 * period, period], [-0.0, 2 * period],
                             [np.inf, np.inf], [period, -np.inf])):
        if m > k:
            rows[rng.integers(0, m)] = bad
    return rows


def test_per_row_rules_and_small_chunks_equal_the_host_definition(program):
    rng = np.random.default_rng(5)
    cases = [(np.zeros((0, 2)), 0, 0, 0.5), (np.zeros((0, 2)), 7, 3, 0.5), (np.array([[0.0, 1.0]]), 0, 4, 0.25)]
    for period in (2.0 ** -5, 0.01, 0.3, 1.0 / 3.0):
        for m, t_s, chunk in ((1, 1, 1), (5, 9, 4), (64, 33, 8), (300, 100, 7), (300, 100, 100), (300, 100, 101), (257, 64, 1), (1000, 501, 250)):
            cases.append((_rows(rng, m, t_s, period), t_s, chunk, period))
    # a request open over whole chunks, one that starts on a seam, one that ends on it
    cases.append((np.array([[0.0, 100.0], [8.0, 16.0], [7.5, 8.0], [16.0, 24.5], [23.9, 24.0]]), 30, 8, 1.0))
    _check(program, cases)


def test_the_kernels_chunk_one_and_two_seams_with_requests_across_them(program):
    rng = np.random.default_rng(6)
    p = 2.0 ** -5
    cases = []
    for t_s in (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 2 * CHUNK + 3):
        rows = _rows(rng, 700, t_s, p)
        seam = [[(CHUNK - 1) * p, (CHUNK + 1) * p], [(CHUNK - 0.5) * p, (CHUNK + 0.25) * p], [CHUNK * p, (CHUNK + 1) * p],
                [(CHUNK - 3) * p, CHUNK * p], [5 * p, (2 * CHUNK + 1) * p], [(2 * CHUNK - 1) * p, (2 * CHUNK) * p],
                [(2 * CHUNK - 1) * p, (2 * CHUNK + 2) * p], [0.0, 1e9]]
        cases.append((np.concatenate([rows, np.array(seam)]), t_s, 0, p))
    _check(program, cases)
    want = in_flight_series(cases[-1][0], cases[-1][1], p)["in_flight"]
    assert want[CHUNK - 1] >= 3 and want[CHUNK] >= 3 and want[2 * CHUNK] >= 3   # requests are open across both seams


def test_bins(program):
    triples = [(v, lo, b) for lo in (0, 3) for b in (1, 2, 5) for v in (0, 1, 2, 3, 4, 7, 8, 9, 2 ** 32 - 1)]
    lines = _run(program, ["bins"], "".join(f"{v} {lo} {b}\n" for v, lo, b in triples))
    assert [int(x) for x in lines] == [b if v < lo else min(v - lo, b - 1) for v, lo, b in triples]
