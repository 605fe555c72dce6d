"""The per-row rule of the latency histogram analyzer on the host, under AddressSanitizer + UBSan:
tests/hostcheck/latency_histogram_main.cpp is a stand-alone program over the plain-C++ routines of
asyncflow_amd/csrc/af_latency_histogram.hpp (aflh::make_binning, aflh::bin_of_latency: the bit rule; aflh::row_cell with the window
search of af_exemplars.hpp; aflh::scenario_cells: the sequential statement of a scenario).  It runs as a child process and
everything it prints is compared with `asyncflow_amd.results.latency_bin_index` / `latency_histogram`, the host definition."""

from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

from asyncflow_amd.results import latency_bin_edges, latency_bin_index, latency_histogram
from tests.hostcheck import build as hc

_problem = hc.sanitizer_link_problem()
pytestmark = pytest.mark.skipif(_problem is not None, reason=str(_problem))

SRC = hc.HERE / "latency_histogram_main.cpp"
HEADERS = [hc.ROOT / "asyncflow_amd/csrc/af_latency_histogram.hpp", hc.ROOT / "asyncflow_amd/csrc/af_exemplars.hpp"]
BINNINGS = [(0, -3, 1), (5, -20, 32), (7, -20, 32), (8, -1022, 16), (3, 1000, 23)]


@pytest.fixture(scope="module")
def program():
    exe = hc.SAN_DIR / "latency_histogram_check"
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


def _values(binning, rng) -> np.ndarray:
    """Every edge and its two float neighbours, signed zeros, negatives, infinities, NaNs of both signs, the smallest denormal and
    log-normal values around the bins."""
    m, e, o = binning
    E = latency_bin_edges(m, e, o)
    mid = float(np.clip(e + o / 2.0, -1000, 1000))
    rnd = np.exp2(rng.normal(mid, o / 3.0 + 1.0, 400).clip(-1070, 1023))
    neg_nan = np.array([0xFFF8000000000001], dtype=np.uint64).view(np.float64)
    return np.concatenate([E, np.nextafter(E, np.inf), np.nextafter(E, -np.inf), rnd, neg_nan,
                           [0.0, -0.0, -1.0, -1e-300, -5e-324, np.inf, -np.inf, np.nan, 5e-324, 2.0 ** -1022, np.finfo(np.float64).max]])


def test_the_bit_rule_equals_the_host_definition_and_searchsorted(program):
    rng = np.random.default_rng(3)
    text, want = [], []
    for binning in BINNINGS:
        m, e, o = binning
        x = _values(binning, rng)
        E = latency_bin_edges(m, e, o)
        idx = latency_bin_index(x, m, e, o)
        pos = np.searchsorted(E, x, side="right") - 1
        brute = np.where(np.isnan(x), -3, np.where(pos < 0, -1, np.where(pos >= E.shape[0] - 1, -2, pos)))
        assert np.array_equal(idx, brute), binning
        n_bins = o << m
        want += [n_bins - 1 - int(i) if i < 0 else int(i) for i in idx]          # -1 / -2 / -3 -> n_bins / n_bins + 1 / n_bins + 2
        text += [f"{m} {e} {o} {int(w):x}\n" for w in x.view(np.uint64)]
    lines = _run(program, ["bins"], "".join(text))
    assert [int(v) for v in lines] == want
    refused = [(9, -20, 1), (5, -1023, 4), (5, -20, 0), (5, 1000, 24), (5, -20, 129), (0, -1022, 4097), (8, 0, 17), (0, 2147483647, 1)]
    assert _run(program, ["bins"], "".join(f"{m} {e} {o} 0\n" for m, e, o in refused)) == ["refused"] * len(refused)
    # the widest binnings there are: every normal octave, and 4 096 bins; +0.0 is under in both
    assert _run(program, ["bins"], "0 -1022 2045 0\n8 -10 16 0\n") == ["2045", str(16 << 8)]


def _rows(rng, m: int, binning, t_hi: float) -> np.ndarray:
    """Starts and finishes on and beside the windows' edges, latencies on the bin edges and their neighbours; NaN, negative,
    reversed and infinite rows mixed in."""
    mm, e, o = binning
    E = latency_bin_edges(mm, e, o)
    start = rng.integers(-2, int(4 * t_hi) + 4, m) / 4.0
    pick = E[rng.integers(0, E.shape[0], m)]
    lat = np.where(rng.random(m) < 0.3, np.nextafter(pick, rng.choice([-np.inf, np.inf], m)), pick)
    lat = np.where(rng.random(m) < 0.3, rng.integers(0, 9, m) / 4.0, lat)
    rows = np.stack([start, start + lat], axis=1)
    for k, bad in enumerate(([np.nan, 1.0], [1.0, np.nan], [2.0, 1.0], [np.inf, np.inf], [1.0, np.inf], [-np.inf, 1.0], [1.0, -np.inf],
                             [0.5, 0.5], [-0.0, 0.0], [np.nan, np.nan])):
        if m > k:
            rows[rng.integers(0, m)] = bad
    return rows


def test_cells_of_a_scenario_equal_the_host_definition_in_both_window_modes_and_without_windows(program):
    rng = np.random.default_rng(4)
    cases = []
    for binning in BINNINGS:
        for m in (0, 1, 7, 300):
            rows = _rows(rng, m, binning, 6.0)
            cases.append((rows, None, "finish", binning))
            for edges in ([0.0, 6.0], [0.25, 1.0, 1.5, 4.0, 4.25, 5.0], np.arange(0.0, 6.01, 0.25)):
                for window_of in ("finish", "arrival"):
                    cases.append((rows, np.asarray(edges, dtype=np.float64), window_of, binning))
    text = ""
    for rows, edges, window_of, (m, e, o) in cases:
        n_win = 0 if edges is None else edges.shape[0] - 1
        text += f"{rows.shape[0]} {n_win} {int(window_of == 'arrival')} {m} {e} {o}\n" + ("" if edges is None else _hex(edges)) + "\n" + _hex(rows) + "\n"
    lines = _run(program, [], text)
    assert len(lines) == 6 * len(cases)
    some = 0
    for j, (rows, edges, window_of, (m, e, o)) in enumerate(cases):
        want = latency_histogram([rows], edges, window_of, sub_bits=m, min_exp=e, octaves=o)
        got = lines[6 * j: 6 * j + 6]
        assert int(got[0]) == o << m
        for k, key in enumerate(("count", "under", "over", "nan")):
            assert np.array_equal(np.array(got[1 + k].split(), dtype=np.uint64), want[key].astype(np.uint64)), (j, key)
        hist = np.zeros(want["hist"].shape, dtype=np.uint32)
        for triple in got[5].split():
            w, b, n = (int(v) for v in triple.split(":"))
            hist[w, b] = n
        assert np.array_equal(hist, want["hist"]), j
        assert np.array_equal(want["under"].astype(np.uint64) + want["over"] + want["nan"] + want["hist"].sum(axis=1, dtype=np.uint64), want["count"])
        some += int(want["hist"].sum() > 0) + int(want["nan"].sum() > 0) + int(want["under"].sum() > 0)
    assert some > len(cases)
