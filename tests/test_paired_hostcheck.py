"""The per-row rules of the paired-difference analyzer on the host, under AddressSanitizer + UBSan:
tests/hostcheck/paired_main.cpp is a stand-alone program over the plain-C++ routines of asyncflow_amd/csrc/af_paired.hpp
(afpr::lower_bound_from and match_start: the match of one start; arrival_of: the state and delta of one arrival; window_from;
fold64: the fixed-order sum; pair_statement: the sequential statement of one pair).  It runs as a child process -- nothing is
preloaded, nothing is loaded into Python -- and every word it prints is compared with `asyncflow_amd.results.latency_pairs`,
the host definition."""

from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

from asyncflow_amd.results import PAIR_NONE, latency_pairs
from tests import paired_cases as pc
from tests.hostcheck import build as hc

_problem = hc.sanitizer_link_problem()
pytestmark = pytest.mark.skipif(_problem is not None, reason=str(_problem))

SRC = hc.HERE / "paired_main.cpp"
HEADERS = [hc.ROOT / "asyncflow_amd/csrc" / h for h in ("af_paired.hpp", "af_latency_histogram.hpp", "af_exemplars.hpp", "af_arrival_counts.hpp")]
BINNINGS = [(0, -3, 1), (5, -20, 32), (8, -10, 16)]


@pytest.fixture(scope="module")
def program():
    exe = hc.SAN_DIR / "paired_check"
    hc.SAN_DIR.mkdir(exist_ok=True)
    if not exe.exists() or exe.stat().st_mtime < max(p.stat().st_mtime for p in [SRC, *HEADERS]):
        subprocess.run(["g++", *hc.SAN_FLAGS, "-Wall", "-o", str(exe), str(SRC)], check=True, capture_output=True, text=True)
    return exe


def _run(program, args: list[str], text: str) -> list[str]:
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}
    r = subprocess.run([str(program), *args], input=text.encode(), capture_output=True, env={**env, **hc.SAN_ENV}, timeout=240, check=False)
    err = r.stderr.decode()
    assert "ERROR: AddressSanitizer" not in err and "runtime error:" not in err, err[-4000:]
    assert r.returncode == 0, (r.returncode, err[-4000:])
    return r.stdout.decode().splitlines()


def _hex(values) -> str:
    return " ".join(f"{int(w):x}" for w in np.ascontiguousarray(values, dtype=np.float64).reshape(-1).view(np.uint64))


def test_the_search_from_any_guess_is_the_plain_search(program):
    rng = np.random.default_rng(1)
    text, want = "", []
    for m in (0, 1, 2, 5, 64, 257):
        row = np.sort(rng.uniform(0.0, 10.0, m))
        if m > 4:
            row[3] = row[2]
        xs = np.concatenate([row, np.nextafter(row, np.inf), np.nextafter(row, -np.inf), [-1.0, 11.0, np.nan, np.inf, -np.inf, -0.0]])
        for x in xs:
            for guess in (0, 1, m // 2, max(m - 1, 0), m, m + 5, 0xFFFFFFFF):
                text += f"{m} {guess} {_hex([x])}\n{_hex(row)}\n"
                want.append(0 if np.isnan(x) else int(np.searchsorted(row, x, side="left")))
    lines = _run(program, ["search"], text)
    got = [tuple(int(v) for v in ln.split()) for ln in lines]
    assert len(got) == len(want)
    for (galloped, plain), w in zip(got, want):
        assert galloped == plain == w          # (a NaN counts nothing below it: 0, and matches no arrival)


def _cases():
    """(times, clock_a, clock_b, edges, thresholds, binning): rows of length 0, 1, 63, 64, 65 and 300 on both sides, a draw
    capacity that is no multiple of 64, duplicated arrivals with one, two and three claimants, edges on and beside arrivals, no
    edges, and more edges than arrivals."""
    rng = np.random.default_rng(2)
    cases = []
    k = 0
    for m in pc.ROWS:
        for n_draw in sorted({m, m + 7, 320}):
            if n_draw < m or n_draw == 0:
                continue
            times = pc.arrival_row(rng, m, n_draw, duplicates=3)
            for rows_a, rows_b in ((m, m), (max(m - 5, 0), m), (m, 0), (m + 9, m // 2)):
                a = pc.side_rows(rng, times, rows_a, pc.ORDERS[k % 3])
                b = pc.side_rows(rng, times, rows_b, pc.ORDERS[(k // 3) % 3])
                for n_win in (0, 1, 7, max(m, 2) + 3):
                    edges = pc.uneven_edges(n_win, times)
                    cases.append((times, a, b, edges, pc.signed_thresholds((0, 5, 64)[k % 3]), BINNINGS[k % 3]))
                    k += 1
    # a run against itself and the swapped pair
    times = pc.arrival_row(rng, 200, 200)
    a, b = pc.side_rows(rng, times, 180, "shuffle"), pc.side_rows(rng, times, 190, "arrival")
    for x, y in ((a, a), (a, b), (b, a)):
        cases.append((times, x, y, pc.uneven_edges(7, times), pc.signed_thresholds(5), BINNINGS[1]))
    return cases


def test_one_pair_equals_the_host_definition_word_for_word(program):
    cases = _cases()
    text = ""
    for times, a, b, edges, th, (m, e, o) in cases:
        n_win = 0 if edges is None else edges.shape[0] - 1
        text += (f"{times.shape[0]} {a.shape[0]} {b.shape[0]} {n_win} {th.shape[0]} {m} {e} {o}\n"
                 + "\n".join(_hex(v) for v in ([] if edges is None else edges, th, times, a, b)) + "\n")
    lines = _run(program, [], text)
    assert len(lines) == 10 * len(cases)
    seen = {k: 0 for k in ("both", "only_a", "only_b", "neither", "nan", "equal", "unmatched", "over", "under", "hist")}
    for c, (times, a, b, edges, th, (m, e, o)) in enumerate(cases):
        want = latency_pairs(a, b, times, edges, thresholds=th, sub_bits=m, min_exp=e, octaves=o)
        got = lines[10 * c: 10 * c + 10]
        n_draw, n_arr, n_bins = times.shape[0], want["row_a"].shape[0], o << m
        n_win = want["both"].shape[0]
        assert [int(v) for v in got[0].split()] == [want["unmatched_a"], want["unmatched_b"]], c
        for line, key in ((got[1], "row_a"), (got[2], "row_b")):
            slots = np.array(line.split(), dtype=np.uint64).astype(np.uint32)
            assert slots.shape == (n_draw,) and np.array_equal(slots[:n_arr], want[key]) and (slots[n_arr:] == PAIR_NONE).all(), (c, key)
        counts = np.array(got[3].split(), dtype=np.uint64).reshape(n_win, 5)
        for k, key in enumerate(("both", "only_a", "only_b", "neither", "nan")):
            assert np.array_equal(counts[:, k], want[key]), (c, key)
        sums = np.array([int(v, 16) for v in got[4].split()], dtype=np.uint64).view(np.float64).reshape(n_win, 2)
        for k, key in enumerate(("sum_d", "sum_a")):
            assert pc.same_words(sums[:, k], want[key]), (c, key)
        cells = np.array(got[5].split(), dtype=np.uint64).reshape(n_win, 8)
        for k, key in enumerate(("both", "only_a", "only_b", "neither", "nan", "slower", "faster", "equal")):
            assert np.array_equal(cells[:, k], want[key].astype(np.uint64)), (c, key)
        above = np.array(got[6].split(), dtype=np.uint64).reshape(n_win, th.shape[0])
        assert np.array_equal(above, want["above"]), c
        ext = np.array([int(v, 16) for v in got[7].split()], dtype=np.uint64).reshape(n_win, 2)
        assert np.array_equal(ext[:, 0], want["min_d"].view(np.uint64)) and np.array_equal(ext[:, 1], want["max_d"].view(np.uint64)), c
        tails = np.array(got[8].split(), dtype=np.uint64).reshape(n_win, 4)
        for k, key in enumerate(("under_pos", "under_neg", "over_pos", "over_neg")):
            assert np.array_equal(tails[:, k], want[key]), (c, key)
        hist = np.zeros((n_win, 2, n_bins), dtype=np.uint32)
        for quad in got[9].split():
            w, side, b_, n = (int(v) for v in quad.split(":"))
            hist[w, side, b_] = n
        assert np.array_equal(hist[:, 0], want["hist_pos"]) and np.array_equal(hist[:, 1], want["hist_neg"]), c
        ident = want["equal"] + want["under_pos"] + want["under_neg"] + want["over_pos"] + want["over_neg"] + want["nan"] \
            + want["hist_pos"].sum(axis=1, dtype=np.uint64) + want["hist_neg"].sum(axis=1, dtype=np.uint64)
        assert np.array_equal(ident, want["both"].astype(np.uint64)), c
        for key in ("both", "only_a", "only_b", "neither", "nan", "equal"):
            seen[key] += int(want[key].sum() > 0)
        seen["unmatched"] += int(want["unmatched_a"] > 0)
        seen["over"] += int(want["over_pos"].sum() + want["over_neg"].sum() > 0)
        seen["under"] += int(want["under_pos"].sum() + want["under_neg"].sum() > 0)
        seen["hist"] += int(want["hist_pos"].sum() > 0 and want["hist_neg"].sum() > 0)
    assert all(v > 3 for v in seen.values()), seen
