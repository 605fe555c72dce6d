"""The per-row rule, the order and the two networks of the slowest-requests analyzer on the host, under AddressSanitizer + UBSan:
tests/hostcheck/exemplars_main.cpp is a stand-alone program over the plain-C++ routines of asyncflow_amd/csrc/af_exemplars.hpp
(afex::row_cell: latency, canonical key, window, rejections; afex::state_row; afex::sort_wave, afex::merge_sorted and
afex::insert_one over a wave of 64 records).  It runs as a child process -- nothing is preloaded, nothing is loaded into Python -- and everything it prints is
compared with `asyncflow_amd.results.latency_exemplars`, the host definition."""

from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

from asyncflow_amd.results import latency_exemplars
from tests.hostcheck import build as hc

_problem = hc.sanitizer_link_problem()
pytestmark = pytest.mark.skipif(_problem is not None, reason=str(_problem))

SRC = hc.HERE / "exemplars_main.cpp"
HEADER = hc.ROOT / "asyncflow_amd/csrc/af_exemplars.hpp"
EMPTY = (0, 0xFFFFFFFF, 0xFFFFFFFF)


@pytest.fixture(scope="module")
def program():
    exe = hc.SAN_DIR / "exemplars_check"
    hc.SAN_DIR.mkdir(exist_ok=True)
    if not exe.exists() or exe.stat().st_mtime < max(SRC.stat().st_mtime, HEADER.stat().st_mtime):
        subprocess.run(["g++", *hc.SAN_FLAGS, "-Wall", "-o", str(exe), str(SRC)], check=True, capture_output=True, text=True)
    return exe


def _run(program, text: str) -> list[str]:
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}
    r = subprocess.run([str(program)], input=text.encode(), capture_output=True, env={**env, **hc.SAN_ENV}, timeout=240, check=False)
    err = r.stderr.decode()
    assert "ERROR: AddressSanitizer" not in err and "runtime error:" not in err, err[-4000:]
    assert r.returncode == 0, (r.returncode, err[-4000:])
    return r.stdout.decode().splitlines()


def _hex(values) -> str:
    return " ".join(f"{int(w):x}" for w in np.asarray(values, dtype=np.float64).reshape(-1).view(np.uint64))


def _key(lat: float) -> int:
    """The order of the definition as an integer: what `latency_exemplars` sorts by, stated independently of the header."""
    u = int(np.array([0.0 if lat == 0.0 else lat], dtype=np.float64).view(np.uint64)[0])
    return (~u & 0xFFFFFFFFFFFFFFFF) if u >> 63 else (u | 1 << 63)


def _values(rng: np.random.Generator, m: int) -> np.ndarray:
    special = [0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 1e-310, 1.0, -1.0, 1.0 + 2.0 ** -52, 1e300, -1e300]
    return np.where(rng.random(m) < 0.4, rng.choice(special, m), rng.normal(0.0, 3.0, m))


def test_per_row_rule_equals_the_host_definition(program):
    rng = np.random.default_rng(21)
    cases, text = [], ""
    for W, edges in ((0, None), (1, [0.0, 4.0]), (2, [1.0, 2.0, 3.0]), (7, [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 5.0, 8.0]), (63, np.arange(64) * 0.125)):
        for by_arrival in ((0,) if W == 0 else (0, 1)):
            m = 300
            start = rng.choice([0.0, 0.5, 1.0, 2.0, 3.0, 8.0, -1.0, 9.0, np.nan, np.inf], m) + rng.choice([0.0, 0.0, 2.0 ** -40, -2.0 ** -40, 0.3], m)
            with np.errstate(invalid="ignore"):
                rows = np.stack([start, start + _values(rng, m)], axis=1)
            rows[rng.integers(0, m, 5), 1] = np.nan
            cases.append((W, edges, by_arrival, rows))
            text += f"rows {W} {by_arrival} {m}\n" + (_hex(edges) + "\n" if W else "") + _hex(rows) + "\n"
    lines = _run(program, text)
    at = 0
    for W, edges, by_arrival, rows in cases:
        got = [ln.split() for ln in lines[at: at + len(rows)]]
        at += len(rows)
        # every row as its own member of one row: total says whether it is in a cell, and in which window
        for i, (start, finish) in enumerate(rows.tolist()):
            ex = latency_exemplars([np.array([[start, finish]])], 1, edges, "arrival" if by_arrival else "finish")
            w = np.flatnonzero(ex["total"])
            assert int(got[i][0]) == len(w), (W, by_arrival, start, finish)
            if len(w):
                with np.errstate(invalid="ignore", over="ignore"):
                    assert int(got[i][1]) == int(w[0]) and int(got[i][2], 16) == _key(np.float64(finish) - np.float64(start))
            else:
                assert got[i] == ["0", "0", "0"]
    assert at == len(lines)
    keys = sorted({_key(v) for v in _values(rng, 4000)})                      # the key orders like the value
    vals = [np.array([k ^ (1 << 63) if k >> 63 else ~k & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64).view(np.float64)[0] for k in keys]
    assert all(a < b for a, b in zip(vals, vals[1:])) and 0 not in keys and _key(-0.0) == _key(0.0)


def test_state_row_equals_the_tick_rule(program):
    text, want = "", []
    for period in (0.25, 0.01, 1.0 / 3.0):
        for t_s in (0, 1, 7):
            starts = np.concatenate([np.arange(-2, t_s + 4) * period, np.arange(0, t_s + 3) * period + period * 2.0 ** -30,
                                     np.arange(1, t_s + 3) * period - period * 2.0 ** -30, [np.nan, -0.0, np.inf, 1e300, -np.inf]])
            text += f"state {t_s} {len(starts)}\n" + _hex([period]) + " " + _hex(starts) + "\n"
            words = np.arange(t_s, dtype=np.uint32).reshape(1, t_s)      # (the word of row r is r)
            for s in starts:
                ex = latency_exemplars([np.array([[s, s + 1.0]])], 1, samples=[words], sample_period=period)
                want.append(int(ex["state"][0, 0, 0]) if int(ex["kept"][0]) else 0xFFFFFFFF)
    assert [int(x) for x in _run(program, text)] == want


def _records(keys, scen, rows) -> list[tuple[int, int, int]]:
    return list(zip((int(k) for k in keys), (int(s) for s in scen), (int(r) for r in rows)))


def _order(recs):
    return sorted(recs, key=lambda r: (-r[0], r[1], r[2]))


def _parse(lines: list[str]) -> list[tuple[int, int, int]]:
    return [(int(a, 16), int(b), int(c)) for a, b, c in (ln.split() for ln in lines)]


def test_sort_network_orders_any_wave(program):
    rng = np.random.default_rng(22)
    cases = []
    for n in (0, 1, 2, 3, 31, 32, 33, 62, 63, 64):
        for kind in ("ascending", "descending", "equal", "random", "few"):
            keys = {"ascending": np.arange(1, n + 1), "descending": np.arange(n, 0, -1), "equal": np.full(n, 7),
                    "random": rng.integers(1, 2 ** 64, n, dtype=np.uint64), "few": rng.integers(1, 4, n)}[kind]
            scen = rng.integers(0, 3, n) if kind != "equal" else np.zeros(n, dtype=np.int64)
            lanes = rng.permutation(64)[:n]
            rows = rng.permutation(1000)[:n]                                  # (scenario, row) is unique
            cases.append((lanes, _records(keys, scen, rows)))
    text = "".join(f"sort {len(r)}\n" + "".join(f"{ln} {k:x} {s} {w}\n" for ln, (k, s, w) in zip(lanes, r)) for lanes, r in cases)
    lines = _run(program, text)
    assert len(lines) == 64 * len(cases)
    for j, (_, recs) in enumerate(cases):
        assert _parse(lines[64 * j: 64 * j + 64]) == _order(recs) + [EMPTY] * (64 - len(recs)), j


@pytest.mark.parametrize("k", [1, 2, 63, 64])
def test_merge_of_two_lists_keeps_the_first_k_with_ties_across_the_kth_place(program, k):
    """The list holds min(len, k) records in the order; the candidates come in any lanes.  The first k lanes of the result are
    the first k of both -- what the kernels store back -- compared with `latency_exemplars` on clocks that have these latencies."""
    rng = np.random.default_rng(23 + k)
    lengths = sorted({0, 1, max(k - 1, 0), k, min(k + 1, 64)})
    cases = []
    for na in (n for n in lengths if n <= k):
        for nb in lengths + [64]:
            for kind in ("ascending", "descending", "equal", "ties"):
                n = na + nb
                lat = {"ascending": np.arange(n, dtype=np.float64), "descending": np.arange(n, 0, -1).astype(np.float64),
                       "equal": np.full(n, 2.5), "ties": rng.integers(0, 3, n).astype(np.float64) - 1.0}[kind]
                if kind == "ties" and n:
                    lat[rng.integers(0, n)] = -0.0
                cases.append((na, nb, lat, rng.permutation(64)[:nb]))
    text = ""
    for na, nb, lat, lanes in cases:
        # member 0 (scenario 4) brings the list, member 1 (scenario 9) the candidates; a row's latency is lat[...]
        a = _order(_records([_key(v) for v in lat[:na]], [4] * na, range(na)))
        b = _records([_key(v) for v in lat[na:]], [9] * nb, range(nb))
        text += f"merge {na} {nb}\n" + "".join(f"{key:x} {s} {w}\n" for key, s, w in a) + "".join(f"{ln} {key:x} {s} {w}\n" for ln, (key, s, w) in zip(lanes, b))
        # ... and the same candidates put in one by one, in row order (insert_one: the kernel's path for few hits)
        text += f"insert {na} {nb}\n" + "".join(f"{key:x} {s} {w}\n" for key, s, w in a + b)
    lines = _run(program, text)
    assert len(lines) == 128 * len(cases)
    for j, (na, nb, lat, _) in enumerate(cases):
        got = _parse(lines[128 * j: 128 * j + 64])
        assert _parse(lines[128 * j + 64: 128 * j + 128]) == got, (j, na, nb, "insert_one and merge_sorted differ")
        clocks = [np.stack([np.zeros(na), lat[:na]], axis=1), np.stack([np.zeros(nb), lat[na:]], axis=1)]
        want = latency_exemplars(clocks, k, scenario_ids=[4, 9])
        kept = int(want["kept"][0])
        assert kept == min(k, na + nb)
        assert [(s, r) for _, s, r in got[:kept]] == list(zip(want["scenario"][0, :kept].tolist(), want["row"][0, :kept].tolist())), (j, na, nb)
        assert [key for key, _, _ in got[:kept]] == [_key(float(c[1] - c[0])) for c in want["clock"][0, :kept]]
        assert got[na + nb:] == [EMPTY] * (64 - na - nb) if na + nb < 64 else True
