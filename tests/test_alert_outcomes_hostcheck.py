"""The per-row rule, the arrival rule, the binary search on the tick, the clamp and the chunk walk of the alert-outcome analyzer on
the host, under AddressSanitizer + UBSan: tests/hostcheck/alert_outcomes_main.cpp is a stand-alone program over the plain-C++
routines of asyncflow_amd/csrc/af_alert_outcomes.hpp (afao::outcome_row, afao::arrival_tick, afao::arrival_lower and
afao::scenario_outcome_ticks: chunk by chunk with the prefix carried across the seams).  It runs as a child process and everything
it prints is compared with the host definition, `asyncflow_amd.results.outcome_ticks`.  Nothing is loaded into Python."""

from __future__ import annotations

import os
import re
import subprocess

import numpy as np
import pytest

from asyncflow_amd.results import outcome_ticks
from tests.alert_outcomes_util import SLO, TAU, P, arrival_row, rows_from
from tests.hostcheck import build as hc

_problem = hc.sanitizer_link_problem()
pytestmark = pytest.mark.skipif(_problem is not None, reason=str(_problem))

SRC = hc.HERE / "alert_outcomes_main.cpp"
HEADERS = [hc.ROOT / "asyncflow_amd/csrc" / h for h in ("af_alert_outcomes.hpp", "af_alerts.hpp")]
CHUNK = int(re.search(r"constexpr uint32_t kChunkTicks = (\d+);", HEADERS[1].read_text()).group(1))
assert "kChunkTicks = afal::kChunkTicks" in HEADERS[0].read_text()


@pytest.fixture(scope="module")
def program():
    exe = hc.SAN_DIR / "alert_outcomes_check"
    hc.SAN_DIR.mkdir(exist_ok=True)
    if not exe.exists() or exe.stat().st_mtime < max(SRC.stat().st_mtime, *(h.stat().st_mtime for h in HEADERS)):
        subprocess.run(["g++", *hc.SAN_FLAGS, "-Wall", "-o", str(exe), str(SRC)], check=True, capture_output=True, text=True)
    return exe


def _run(program, args: list[str], text: str) -> list[str]:
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}
    r = subprocess.run([str(program), *args], input=text.encode(), capture_output=True, env={**env, **hc.SAN_ENV}, timeout=240, check=False)
    err = r.stderr.decode()
    assert "ERROR: AddressSanitizer" not in err and "runtime error:" not in err, err[-4000:]
    assert r.returncode == 0, (r.returncode, err[-4000:])
    return r.stdout.decode().split("\n")


def _hex(values) -> str:
    return " ".join(f"{int(w):x}" for w in np.asarray(values, dtype=np.float64).reshape(-1).view(np.uint64))


def _case(rows, arr, t_s, chunk, period=P, slo=SLO, tau=TAU) -> str:
    rows, arr = np.asarray(rows, dtype=np.float64).reshape(-1, 2), np.asarray(arr, dtype=np.float64).reshape(-1)
    return f"{len(rows)} {len(arr)} {t_s} {chunk}\n" + _hex(np.concatenate([[period, slo, tau], rows.reshape(-1), arr])) + "\n"


def _check(program, cases) -> list[dict]:
    lines = _run(program, [], "".join(_case(*c) for c in cases))
    assert len(lines) == 6 * len(cases) + 1 and lines[-1] == ""
    wants = []
    for j, c in enumerate(cases):
        rows, arr, t_s, chunk = c[:4]
        period, slo, tau = c[4:] or (P, SLO, TAU)
        want = outcome_ticks(rows, arr, t_s, period, slo, tau)
        got = [np.array(line.split(), dtype=np.uint64) for line in lines[6 * j: 6 * j + 6]]
        assert got[0].tolist() == [chunk or CHUNK, want["deficit"], want["timed_out"]], (j, got[0], want["deficit"], want["timed_out"])
        for k, key in enumerate(("total", "bad", "timeouts")):
            assert np.array_equal(got[1 + k], want[key]), (j, key, t_s, chunk)
        assert np.array_equal(got[4], np.cumsum(want["total"], dtype=np.uint64)), (j, "PT")
        assert np.array_equal(got[5], np.cumsum(want["bad"], dtype=np.uint64)), (j, "PB")
        wants.append(want)
    return wants


def test_forced_chunks_of_1_3_7_and_100_ticks_and_no_ticks(program):
    rng = np.random.default_rng(51)
    none = np.zeros((0, 2))
    cases = [(none, [], 0, 0), (none, [np.inf] * 3, 0, 3), (np.array([[0.0, 0.25]]), [0.0, np.inf], 0, 1), (none, [], 9, 4)]
    for period, scale in ((P, 1.0), (0.01, 0.01 / P), (1.0 / 3.0, 1.0 / (3.0 * P))):
        for n_arr, m, t_s in ((1, 1, 1), (60, 40, 9), (400, 300, 33), (900, 700, 100), (900, 0, 100), (500, 500, 64)):
            arr = arrival_row(rng, n_arr, t_s, n_arr + 5) * scale
            rows = rows_from(rng, arr, m, TAU * scale)
            for chunk in (1, 3, 7, 100):
                cases.append((rows, arr, t_s, chunk, period, SLO * scale, TAU * scale))
    wants = _check(program, cases)
    assert sum(w["timed_out"] for w in wants) > 1000 and all(w["deficit"] == 0 for w in wants[4:40])   # (the dyadic period: own rows)


def test_arrivals_and_timeouts_on_chunk_seams(program):
    # arrivals whose timeout tick is the last of a chunk, the first of the next, t_s - 1 and t_s; rows that answer half of them
    t_s, chunk = 21, 7
    at = [k * P - TAU for k in (0, 6, 7, 7, 13, 14, 20, 21, 22)] + [k * P - TAU + P / 2 for k in (6, 7, 20, 21)]
    arr = np.sort(np.asarray(at + [np.inf, np.inf]))
    rows = np.array([[arr[1], arr[1] + P / 4], [arr[3], arr[3] + TAU], [arr[6], arr[6] + TAU + P / 8], [arr[8], arr[8] + SLO + P]])
    cases = [(rows, arr, t_s, c) for c in (1, 3, 7, 100, 0)] + [(rows[:0], arr, t_s, 7), (rows, arr[:0], t_s, 7), (rows, np.full(4, np.inf), t_s, 3)]
    wants = _check(program, cases)
    last = outcome_ticks(rows[:0], arr, t_s, P, SLO, TAU)["timeouts"]
    assert last[20] == 2 and last.sum() == 10 and last[[6, 7, 13, 14]].tolist() == [2, 3, 1, 1]     # ticks 21 and 22 are past the run
    assert wants[6]["deficit"] > 0 and wants[7]["deficit"] == wants[6]["deficit"] and wants[0]["deficit"] == 0


def test_look_at_the_kernels_own_chunk(program):
    rng = np.random.default_rng(52)
    cases = []
    for t_s in (CHUNK - 1, CHUNK + 1, 2 * CHUNK + 3):
        arr = arrival_row(rng, 6000, t_s, 6001)
        cases.append((rows_from(rng, arr, 4000), arr, t_s, 0))
    _check(program, cases)


def test_binary_search_bounds_at_an_empty_range_and_at_the_whole_row(program):
    rng = np.random.default_rng(53)
    text, want = "", []
    rows = [np.zeros(0), np.full(5, np.inf), np.array([-10.0, -9.0]), np.arange(64) * P, arrival_row(rng, 300, 40, 310), np.array([3 * P] * 7)]
    for arr in rows:
        bounds = [0, 1, 2, 16, 17, 19, 40, 56, 57, 80, 81, 2 ** 31 - 1]
        text += f"{len(arr)} {len(bounds)}\n{_hex(np.concatenate([[P, TAU], arr]))}\n" + " ".join(map(str, bounds)) + "\n"
        with np.errstate(invalid="ignore"):
            q = np.floor((arr + TAU) / P)
        want.append(" ".join(str(int(np.searchsorted(q, float(b), side="left"))) for b in bounds))
    got = _run(program, ["search"], text)
    assert got[:-1] == want
    assert want[0] == " ".join(["0"] * 12) and want[2].split()[0] == "2" and want[3].split()[0] == "0" and want[3].split()[-1] == "64"
