"""Shared by the alert-outcome tests: synthetic arrival rows and clock rows whose starts are drawn from them, and an INDEPENDENT
statement of the definition written only here -- a join of the arrivals to the in-time rows on the u64 pattern of `start`, as a
multiset, in plain Python floats and ints; nothing shared with asyncflow_amd.results."""

from __future__ import annotations

import math
import struct
from collections import Counter

import numpy as np

P = 2.0 ** -5          # a dyadic period: every tick instant and every sum below is exact
SLO = 0.25
TAU = 0.5              # 16 ticks


def arrival_row(rng: np.random.Generator, n_arr: int, t_s: int, cap: int | None = None) -> np.ndarray:
    """n_arr ascending arrival times on a grid of P / 8 from below 0 to past the last tick, two of one bit pattern among them,
    +inf behind the last up to `cap` entries."""
    a = np.sort(rng.integers(-40, 8 * (t_s + 4), n_arr)).astype(np.float64) * (P / 8.0)
    if n_arr > 3:
        a[2] = a[1]                                          # two arrivals of one bit pattern
    out = np.full(max(cap or 0, n_arr), np.inf)
    out[:n_arr] = a
    return out


def rows_from(rng: np.random.Generator, arr: np.ndarray, m: int, tau: float = TAU, odd: bool = True) -> np.ndarray:
    """m rows whose starts are distinct entries of the arrival row (as a multiset: a duplicated arrival may be drawn twice), in
    random order; latencies at, below and above the slo and the timeout; with `odd` a few NaN rows replace drawn ones."""
    fin = np.flatnonzero(np.isfinite(arr))
    pick = rng.permutation(fin)[:m]
    start = arr[pick]
    lat = rng.choice([0.0, P / 4, SLO / 2, SLO, SLO + P / 8, tau, tau + P / 8, 2 * tau, 50.0], pick.shape[0])
    rows = np.stack([start, start + lat], axis=1)
    if odd:
        for k, bad_row in enumerate(([np.nan, 1.0], [1.0, np.nan], [np.nan, np.nan])):
            if rows.shape[0] > 2 * k + 4:
                rows[rng.integers(0, rows.shape[0])] = bad_row
    return rows


def _bits(x: float) -> bytes:
    return struct.pack("<d", x)


def _tick(x: float, period: float, t_s: int) -> int | None:
    q = x / period if math.isfinite(x) else x
    if q != q or q == math.inf or q == -math.inf:
        return None
    k = math.floor(q)
    return k if 0 <= k < t_s else None


def join_outcomes(rows, arrivals, t_s: int, period: float, slo: float, tau: float) -> dict:
    """The definition as a JOIN: every finite arrival is matched to an in-time row with the same u64 pattern of `start` (as a
    multiset); a matched one completes at floor(finish / p), an unmatched one times out at floor((a + tau) / p).  `excess`: the
    in-time rows that found no arrival (0 whenever the rows are the arrival row's own)."""
    total, bad, timeouts, completions = [0] * t_s, [0] * t_s, [0] * t_s, [0] * t_s
    have: Counter = Counter()
    for start, finish in np.asarray(rows, dtype=np.float64).reshape(-1, 2).tolist():
        if start != start or finish != finish:
            continue
        lat = finish - start
        if not lat <= tau:
            continue
        have[_bits(start)] += 1
        k = _tick(finish, period, t_s)
        if k is not None:
            total[k] += 1
            completions[k] += 1
            bad[k] += lat > slo
    for a in np.asarray(arrivals, dtype=np.float64).reshape(-1).tolist():
        if not math.isfinite(a):
            continue
        if have[_bits(a)] > 0:
            have[_bits(a)] -= 1                              # answered in time
            continue
        k = _tick(a + tau, period, t_s)
        if k is not None:
            total[k] += 1
            bad[k] += 1
            timeouts[k] += 1
    return {"total": np.asarray(total, dtype=np.uint32), "bad": np.asarray(bad, dtype=np.uint32), "timeouts": np.asarray(timeouts, dtype=np.uint32),
            "completions": np.asarray(completions, dtype=np.uint32), "timed_out": int(sum(timeouts)), "excess": int(sum(have.values()))}
