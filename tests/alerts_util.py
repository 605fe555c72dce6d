"""Shared by the alert tests: synthetic clock rows whose bad share comes and goes in phases, rule sets in ticks, and a
brute-force statement of the definition -- a plain loop over ticks and rows with Python ints, nothing vectorised, nothing
shared with asyncflow_amd.results."""

from __future__ import annotations

import numpy as np

P = 2.0 ** -5          # a dyadic period: every tick instant is exact
SLO = 0.25
HOLDS = (1, 2, 63, 64, 65, 200)


def rows_in_phases(rng: np.random.Generator, m: int, t_s: int, phase: int = 150, order: str = "random") -> np.ndarray:
    """m rows with finishes from before the first tick to past the last one, several per tick; in every other phase of `phase`
    ticks nine rows in ten are bad, else one in twenty.  NaN, negative, infinite and reversed rows mixed in."""
    tick4 = rng.integers(-8, 4 * (t_s + 3), m)
    finish = tick4 * (P / 4.0)
    odd = ((tick4 // 4) // phase) % 2 == 1
    is_bad = rng.random(m) < np.where(odd, 0.9, 0.05)
    lat = np.where(is_bad, rng.choice([SLO + P / 8, 2 * SLO, 50.0], m), rng.choice([0.0, P / 4, SLO, SLO / 2], m))
    rows = np.stack([finish - lat, finish], axis=1)
    odd_rows = ([np.nan, 1.0], [1.0, np.nan], [-3 * P, 9 * P], [7 * P, 3 * P], [0.0, np.inf], [-np.inf, 2 * P], [np.inf, 5 * P],
                [2 * P, -np.inf], [-0.0, -0.0], [0.0, 2.0 ** 40], [1.0, -P / 2])
    for k, bad_row in enumerate(odd_rows):
        if m > 2 * k + 4:
            rows[rng.integers(0, m)] = bad_row
    if order == "sorted":
        rows = rows[np.argsort(rows[:, 1], kind="stable")]
    return rows


def rules_few(chunk: int) -> list[tuple[int, int, int, int, int, int]]:
    """(long_ticks, short_ticks, num, den, min_total, hold_ticks): every hold of HOLDS, num == 0 and num == den, a look-back
    longer than a chunk, one longer than any run of ticks, a min_total nothing reaches."""
    out = [(1, 1, 0, 1, 0, 1), (5, 5, 1, 1, 0, 1), (60, 5, 1, 2, 1, 1), (60, 5, 1, 10, 3, 2), (10, 10, 0, 1, 2 ** 32 - 1, 1),
           (chunk + 5, 3, 1, 3, 1, 1), (2 ** 32 - 1, 1, 1, 3, 0, 1), (2 ** 32 - 1, 2 ** 32 - 1, 1, 50, 5, 2 ** 32 - 1)]
    out += [(40, 4, 2, 5, 2, h) for h in HOLDS]
    return out


def rules_32(chunk: int) -> list[tuple[int, int, int, int, int, int]]:
    base = rules_few(chunk)
    extra = [(20 + 3 * j, 1 + j % 7, 1 + j % 3, 4 + j % 5, j % 4, 1 + (j * 7) % 40) for j in range(32 - len(base) - 1)]
    return base + extra + [(3, 1, 1, 4, 1, 1)]      # rule 31 fires easily: bit 31 of the firing word


def brute_force(rows, t_s: int, period: float, slo: float, rules, edges) -> dict:
    """The definition, tick by tick and row by row, with Python ints and floats."""
    total, bad = [0] * t_s, [0] * t_s
    for start, finish in np.asarray(rows, dtype=np.float64).reshape(-1, 2).tolist():
        if start != start or finish != finish:
            continue
        with np.errstate(all="ignore"):
            q = float(np.floor(np.float64(finish) / np.float64(period)))
        if not (0.0 <= q < float(t_s)):
            continue
        total[int(q)] += 1
        with np.errstate(all="ignore"):
            if float(np.float64(finish) - np.float64(start)) > slo:
                bad[int(q)] += 1
    n_rules, n_win = len(rules), len(edges) - 1
    cond = [[False] * t_s for _ in range(n_rules)]
    firing = [[False] * t_s for _ in range(n_rules)]
    for r, (long_t, short_t, num, den, min_total, hold) in enumerate(rules):
        for k in range(t_s):
            t_long, b_long = sum(total[max(k - long_t + 1, 0): k + 1]), sum(bad[max(k - long_t + 1, 0): k + 1])
            t_short, b_short = sum(total[max(k - short_t + 1, 0): k + 1]), sum(bad[max(k - short_t + 1, 0): k + 1])
            cond[r][k] = b_long * den > num * t_long and b_short * den > num * t_short and t_long >= min_total
        for k in range(t_s):
            firing[r][k] = k + 1 >= hold and all(cond[r][j] for j in range(k - hold + 1, k + 1))
    cells = {key: [[0 if key in ("fired", "episodes", "longest") else -1] * n_rules for _ in range(n_win)]
             for key in ("fired", "episodes", "longest", "longest_start", "first", "last")}
    count = []
    for w in range(n_win):
        lo, hi = min(edges[w], t_s), min(edges[w + 1], t_s)
        count.append(hi - lo)
        for r in range(n_rules):
            run = 0
            for k in range(lo, hi):
                if not firing[r][k]:
                    run = 0
                    continue
                run += 1
                cells["fired"][w][r] += 1
                cells["episodes"][w][r] += run == 1
                if cells["first"][w][r] < 0:
                    cells["first"][w][r] = k
                cells["last"][w][r] = k
                if run > cells["longest"][w][r]:
                    cells["longest"][w][r], cells["longest_start"][w][r] = run, k - run + 1
    out = {k: np.asarray(v, dtype=np.int64).reshape(n_win, n_rules) for k, v in cells.items()}
    out.update(total=np.asarray(total, dtype=np.int64), bad=np.asarray(bad, dtype=np.int64), count=np.asarray(count, dtype=np.int64),
               cond=np.asarray(cond, dtype=bool).reshape(n_rules, t_s), firing=np.asarray(firing, dtype=bool).reshape(n_rules, t_s))
    return out


def firing_words(firing: np.ndarray) -> np.ndarray:
    """bool [R, t_s] as the device's words [t_s]: bit r = rule r fires."""
    bits = (np.asarray(firing, dtype=np.uint64) << np.arange(firing.shape[0], dtype=np.uint64)[:, None])
    return np.bitwise_or.reduce(bits, axis=0).astype(np.uint32) if firing.shape[0] else np.zeros(firing.shape[1], np.uint32)
