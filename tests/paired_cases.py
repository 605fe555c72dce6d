"""Synthetic arrival rows and clock rows for the paired-difference tests (tests/test_paired_cpu.py, test_paired_hostcheck.py,
test_gpu_paired.py): the inputs only -- what is expected of them comes from `asyncflow_amd.results.latency_pairs`."""

from __future__ import annotations

import numpy as np

T = 16.0                    # arrival times lie in (0, T)
ROWS = [0, 1, 63, 64, 65, 300]
ORDERS = ("arrival", "reversed", "shuffle")


def arrival_row(rng, m: int, n_draw: int, duplicates: int = 0) -> np.ndarray:
    """n_draw doubles: m ascending arrival times in (0, T), `duplicates` of them repeated bit for bit by their successor, +inf
    behind the last."""
    assert m <= n_draw
    t = np.sort(rng.uniform(0.01, T - 0.01, m))
    if m > 2:
        for k in rng.choice(m - 1, min(duplicates, m - 1), replace=False):
            t[k + 1] = t[k]
        t = np.sort(t)
    return np.concatenate([t, np.full(n_draw - m, np.inf)])


def side_rows(rng, times: np.ndarray, rows: int, order: str = "arrival", hostile: bool = True) -> np.ndarray:
    """`rows` clock rows (start, finish) of one side: starts drawn from the arrivals without repetition while they last,
    log-normal latencies (a few exact multiples of 1/8, so deltas of exactly zero occur between two sides), completion order the
    arrival order, its reverse or a shuffle.  `hostile`: rows that match nothing -- a start one ulp beside an arrival, NaN,
    negative, -0.0 and infinite starts, NaN and infinite finishes, a finish before its start -- and up to three claimants of one
    arrival are written over some of them."""
    A = times[np.isfinite(times)]
    m = A.shape[0]
    if rows == 0:
        return np.zeros((0, 2))
    pick = np.sort(rng.choice(m, min(rows, m), replace=False)) if m else np.zeros(0, dtype=np.int64)
    start = np.concatenate([A[pick], rng.uniform(0.0, T, rows - pick.shape[0])])        # (more rows than arrivals: strays)
    lat = rng.lognormal(-2.0, 1.0, rows)
    lat = np.where(rng.random(rows) < 0.3, rng.integers(0, 9, rows) / 8.0, lat)
    out = np.stack([start, start + lat], axis=1)
    if order == "reversed":
        out = out[::-1]
    elif order == "shuffle":
        out = out[rng.permutation(rows)]
    out = np.ascontiguousarray(out)
    if hostile and rows >= 12 and m >= 4:
        at = [int(v) for v in rng.choice(rows, 12, replace=False)]
        j = int(rng.integers(1, m - 1))
        bad = ([np.nextafter(A[j], np.inf), A[j] + 1.0], [np.nextafter(A[j], -np.inf), A[j] + 1.0], [np.nan, 1.0], [-1.0, 2.0], [-0.0, 1.0],
               [np.inf, np.inf], [-np.inf, 1.0])
        for k, row in zip(at, bad):
            out[k] = row
        out[at[7], 1] = np.nan
        out[at[8], 1] = np.inf
        out[at[9], 1] = out[at[9], 0] - 0.5
        out[at[10], 0], out[at[11], 0] = out[at[9], 0], out[at[9], 0]                   # three claimants of one start
    return out


def uneven_edges(n_win: int, times: np.ndarray | None = None) -> np.ndarray | None:
    """Window edges: None for 0; [0, T] for 1; 7 uneven ones; otherwise n_win windows.  With `times`, some edges are put on an
    arrival and one ulp beside one."""
    if n_win == 0:
        return None
    if n_win == 1:
        e = np.array([0.0, T])
    elif n_win == 7:
        e = np.array([0.5, 1.0, 1.25, 4.0, 9.0, 9.5, 15.0, 15.75])
    else:
        e = np.linspace(0.25, T - 0.25, n_win + 1)
    if times is not None and n_win >= 3:
        A = times[np.isfinite(times)]
        e = e.copy()
        moves = ((1, lambda v: v), (n_win // 2, lambda v: np.nextafter(v, np.inf)), (n_win - 1, lambda v: np.nextafter(v, -np.inf)))
        for k, beside in moves:                       # an interior edge moves onto (or one ulp beside) an arrival between its neighbours
            inside = A[(A > e[k - 1]) & (A < e[k + 1])]
            if inside.shape[0] >= 3:
                e[k] = beside(inside[inside.shape[0] // 2])
        assert (np.diff(e) > 0).all()
    return np.ascontiguousarray(e, dtype=np.float64)


def signed_thresholds(n: int) -> np.ndarray:
    """n finite thresholds of both signs, zero among them."""
    if n == 0:
        return np.zeros(0)
    return np.ascontiguousarray(np.concatenate([[0.0, -0.0][: min(n, 2)], np.linspace(-2.0, 2.0, max(n - 2, 0))])[:n])


def same_words(a, b) -> bool:
    """Two float64 results are equal if their words are equal or both are NaN."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())
