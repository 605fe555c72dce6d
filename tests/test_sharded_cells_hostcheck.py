"""The placement rule of the cells across devices on the host, under AddressSanitizer + UBSan: tests/hostcheck/cells_main.cpp is a
stand-alone program over the plain-C++ part of asyncflow_amd/csrc/af_cells.hpp (afc::layout_cells, afc::window_of,
afc::destination -- what af_engine_import_cells lays the cells out with and what af_cells_merge places every element by).  It
runs as a child process and prints the destination of every element of every member's segment; the destinations must be a
permutation onto [0, total) and equal `asyncflow_amd.results.merge_cell_segments`, the host definition."""

from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

from asyncflow_amd.results import merge_cell_segments
from tests.hostcheck import build as hc

_problem = hc.sanitizer_link_problem()
pytestmark = pytest.mark.skipif(_problem is not None, reason=str(_problem))

SRC = hc.HERE / "cells_main.cpp"
HEADER = hc.ROOT / "asyncflow_amd/csrc/af_cells.hpp"
SKIP = 0xFFFFFFFF


@pytest.fixture(scope="module")
def program():
    exe = hc.SAN_DIR / "cells_check"
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
    return r.stdout.decode().split("\n")


def _case_text(ids: np.ndarray, bounds: np.ndarray, n_groups: int) -> str:
    group = np.where(ids < 0, SKIP, ids)
    return f"{len(ids)} {n_groups} {bounds.shape[1] - 1}\n" + " ".join(map(str, group.tolist())) + "\n" + " ".join(map(str, bounds.reshape(-1).tolist())) + "\n"


def _bounds(rng: np.random.Generator, n: int, W: int, most: int) -> np.ndarray:
    """Bounds [n, W + 1] as an export writes them: a first row anywhere, windows of 0 .. most rows, many of them empty."""
    sizes = rng.integers(0, most + 1, (n, W)) * (rng.random((n, W)) < 0.6)
    return (rng.integers(0, 50, (n, 1)) + np.concatenate([np.zeros((n, 1), dtype=np.int64), np.cumsum(sizes, axis=1)], axis=1)).astype(np.uint32)


def _check(program, cases: list[tuple[np.ndarray, np.ndarray, int, int]]) -> None:
    """cases: (ids [n], bounds [n, W + 1], n_groups, shards).  The members are dealt over the shards in interleaved order; every
    exported latency is its own name (member * 2^32 + element), so that the host definition's cells say where each one belongs."""
    rng = np.random.default_rng(99)
    lines = _run(program, "".join(_case_text(ids, b, g) for ids, b, g, _ in cases))
    at = 0
    for ids, bounds, n_groups, shards in cases:
        n, W = len(ids), bounds.shape[1] - 1
        deal = rng.integers(0, shards, n)
        index = [np.nonzero(deal == k)[0] for k in range(shards)]
        length = np.where(ids < 0, 0, bounds[:, -1].astype(np.int64) - bounds[:, 0])
        parts = [(np.concatenate([s * 2.0 ** 32 + np.arange(length[s]) for s in ix] + [np.zeros(0)]), bounds[ix]) for ix in index]
        cells = merge_cell_segments(parts, index, ids, n_groups, W)
        merged = np.concatenate(cells + [np.zeros(0)])
        error, total = (int(x) for x in lines[at].split())
        assert error == 0 and total == merged.shape[0] == int(length.sum())
        seen = np.zeros(total, dtype=bool)
        for s in range(n):
            dest = np.array(lines[at + 1 + s].split(), dtype=np.int64)
            assert dest.shape[0] == length[s], (s, dest.shape[0], int(length[s]))
            assert ((dest >= 0) & (dest < total)).all() and not seen[dest].any() and np.unique(dest).shape[0] == dest.shape[0]
            seen[dest] = True
            assert np.array_equal(merged[dest], s * 2.0 ** 32 + np.arange(length[s])), s
        assert seen.all()                                            # a permutation onto [0, total)
        at += 1 + n
    assert lines[at:] == [""]


def test_random_cases_are_permutations_and_equal_the_host_definition(program):
    rng = np.random.default_rng(7)
    cases = []
    for n, G, W, most, shards in ((1, 1, 1, 9, 1), (5, 2, 1, 40, 2), (9, 3, 4, 17, 2), (30, 3, 4, 33, 3), (12, 12, 7, 5, 3), (40, 5, 60, 3, 2),
                                  (7, 2, 129, 2, 3)):
        ids = rng.integers(0, G, n)
        ids[rng.random(n) < 0.15] = -1
        cases.append((ids, _bounds(rng, n, W, most), G, shards))
    _check(program, cases)


def test_edge_cases(program):
    rng = np.random.default_rng(8)
    # a member without rows, one whose rows all lie outside the windows, a skipped one (its bounds still say rows), odd lengths, an
    # empty group in the middle, every member skipped
    ids = np.array([0, 2, -1, 0, 2, 0])
    bounds = np.array([[0, 0, 0, 0], [7, 7, 7, 7], [0, 3, 5, 9], [2, 3, 3, 8], [0, 1, 4, 4], [5, 5, 6, 11]], dtype=np.uint32)
    cases = [(ids, bounds, 3, 2), (ids, bounds, 3, 3), (np.array([-1, -1]), bounds[:2], 1, 2)]
    # one window (the whole run: a segmented copy) and a window count past the form that keeps the bounds in LDS
    cases.append((np.array([0, 1, 0, -1, 1]), np.array([[0, 5], [0, 0], [0, 3], [0, 9], [0, 1]], dtype=np.uint32), 2, 2))
    cases.append((np.array([1, 0, 1, 0]), _bounds(rng, 4, 4097, 2), 2, 2))
    _check(program, cases)


def test_decreasing_bounds_are_reported(program):
    lines = _run(program, _case_text(np.array([0, 0]), np.array([[0, 4, 3], [0, 1, 2]], dtype=np.uint32), 1))
    assert lines[0].split()[0] == "1" and lines[1:] == [""]
