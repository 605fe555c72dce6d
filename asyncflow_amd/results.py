"""Results of a batched run, with the reference analyzer's accessors per scenario.

``ScenarioResults`` restates the compute part of the reference's
``ResultsAnalyzer`` (/root/reference/src/asyncflow/metrics/analyzer.py:75-244)
on the arrays the engine wrote: same numpy calls, same bucket rule, same keys,
so a user of ``SimulationRunner(...).run()`` can keep calling
``get_latency_stats / get_throughput_series / get_sampled_metrics / get_series``.
Plotting (analyzer.py:249-589) is presentation and out of scope: the reference's
own plot helpers accept these objects through ``to_reference_analyzer``.
"""

from __future__ import annotations

import math
from collections import defaultdict
from typing import Any, Iterator

import numpy as np

from . import _abi
from .plan import DevicePlan

LATENCY_KEYS = ("total_requests", "mean", "median", "std_dev", "p95", "p99", "min", "max")
Series = tuple[list[float], list[float]]


def window_edges(window_s: float, total_time: float) -> np.ndarray:
    """Edges ``[0.0, w, w + w, ...]`` of the windows of ``window_s`` seconds up to ``total_time``, accumulated in floating
    point exactly as :meth:`ScenarioResults.get_throughput_series` accumulates its timestamps (the reference's loop,
    analyzer.py:107-125): ``window_edges(w, T)[1:]`` ARE those timestamps, so a window's ``total_requests / w`` is the
    throughput series' value."""
    w = float(window_s)
    if not (np.isfinite(w) and w > 0.0):
        msg = f"window_s must be a positive number of seconds, not {window_s!r}"
        raise ValueError(msg)
    out = [0.0]
    current_end = w
    while current_end <= total_time:
        out.append(current_end)
        current_end += w
    return np.asarray(out, dtype=np.float64)


def check_edges(edges: Any) -> np.ndarray:
    """``edges`` as a float64 vector, or ValueError: at least two values, all finite, strictly increasing."""
    e = np.array(edges, dtype=np.float64)
    if e.ndim != 1 or e.shape[0] < 2:
        msg = f"window edges must be a vector of at least two values, not of shape {e.shape}"
        raise ValueError(msg)
    if not np.isfinite(e).all():
        msg = "window edges must be finite"
        raise ValueError(msg)
    if not (np.diff(e) > 0.0).all():
        msg = "window edges must be strictly increasing"
        raise ValueError(msg)
    return e


def _resolve_edges(window_s: float | None, edges: Any, total_time: float) -> np.ndarray:
    if edges is not None:
        if window_s is not None:
            msg = "pass window_s or edges, not both"
            raise ValueError(msg)
        return check_edges(edges)
    return check_edges(window_edges(1.0 if window_s is None else window_s, total_time))


def latency_stats_row(arr: np.ndarray) -> np.ndarray:
    """The eight statistics of one latency sample in LATENCY_KEYS order, by the reference's numpy calls
    (analyzer.py:83-104); an empty sample: total 0, the rest NaN."""
    if not arr.size:
        return np.array([0.0] + [np.nan] * 7)
    return np.array([float(arr.size), np.mean(arr), np.median(arr), np.std(arr), np.percentile(arr, 95),
                     np.percentile(arr, 99), np.min(arr), np.max(arr)], dtype=np.float64)


WINDOW_OF = ("finish", "arrival")


def check_window_of(window_of: str) -> str:
    """``window_of`` if it is ``"finish"`` or ``"arrival"``, or ValueError."""
    if window_of not in WINDOW_OF:
        msg = f"window_of must be 'finish' or 'arrival', not {window_of!r}"
        raise ValueError(msg)
    return window_of


def _window_latencies(ck: np.ndarray, e: np.ndarray, window_of: str) -> list[np.ndarray]:
    """Per window of ``e`` the latencies of ONE scenario's rows ``ck`` [m, 2] that belong to it, in row order."""
    n_win = e.shape[0] - 1
    finish = ck[:, 1]
    lat = finish - ck[:, 0]
    if window_of == "arrival":
        b = np.searchsorted(e, ck[:, 0], side="left")           # #{edges < start}: window b - 1 where 1 <= b <= W
        order = np.argsort(b, kind="stable")                    # (stable: a window's rows stay in row order)
        r = np.searchsorted(b[order], np.arange(1, n_win + 2), side="left")
        return [lat[order[r[w]:r[w + 1]]] for w in range(n_win)]
    if finish.size > 1 and (np.diff(finish) < 0.0).any():
        msg = "rqs_clock is not in completion order (finish decreases): windows by finish time need it"
        raise ValueError(msg)
    r = np.searchsorted(finish, e, side="right")
    return [lat[r[w]:r[w + 1]] for w in range(n_win)]


def latency_window_stats(clock: np.ndarray, edges: Any, window_of: str = "finish") -> np.ndarray:
    """Latency statistics per time window of ONE scenario's ``rqs_clock`` [m, 2] (start, finish): float64 [W, 8] in
    LATENCY_KEYS order.  Window w holds the rows with ``edges[w] < finish <= edges[w + 1]`` (the bucket rule of the
    throughput series); rows are in completion order, so that is the row range between two ``np.searchsorted(finish,
    edges, side="right")`` positions.  The definition the device analyzer (``af_engine_summarize_windows``) is
    bit-equal to.

    ``window_of="arrival"``: the same bucket rule on column 0, ``lat[(start > edges[w]) & (start <= edges[w + 1])]`` with
    the latencies in row (completion) order -- the cohort of the requests SENT in the window, the one an objective is
    written against (``af_engine_summarize_arrival_windows``).  A start equal to an edge belongs to the window that ends
    there; rows with ``start <= edges[0]`` or ``start > edges[W]`` belong to no window; completion order is not needed and
    not checked.  The cohorts are RIGHT-CENSORED: a request that arrived in a window but had not completed when the run
    ended, or was dropped, is in no row, so ``total`` is the cohort's completions, not its arrivals, and the last windows
    of a run under-report slow requests."""
    e = check_edges(edges)
    ck = np.asarray(clock, dtype=np.float64).reshape(-1, 2)
    return np.stack([latency_stats_row(x) for x in _window_latencies(ck, e, check_window_of(window_of))])


def check_levels(levels: Any) -> np.ndarray:
    """``levels`` as a float64 vector, or ValueError: one dimension, at most ``AF_MAX_QUANTILE_LEVELS``, each in [0, 1]."""
    q = np.array(levels, dtype=np.float64)
    if q.ndim != 1:
        msg = f"quantile levels must be a vector, not of shape {q.shape}"
        raise ValueError(msg)
    if q.shape[0] > _abi.MAX_QUANTILE_LEVELS:
        msg = f"at most {_abi.MAX_QUANTILE_LEVELS} quantile levels a call, not {q.shape[0]}"
        raise ValueError(msg)
    if not ((q >= 0.0) & (q <= 1.0)).all():
        msg = "quantile levels must lie in [0, 1]"
        raise ValueError(msg)
    return q


def check_slo_thresholds(thresholds: Any) -> np.ndarray:
    """``thresholds`` (seconds; None: none) as a float64 vector, or ValueError: one dimension, at most
    ``AF_MAX_SLO_THRESHOLDS``, no NaN (an infinite threshold is fine)."""
    th = np.zeros(0, dtype=np.float64) if thresholds is None else np.array(thresholds, dtype=np.float64)
    if th.ndim != 1:
        msg = f"thresholds must be a vector, not of shape {th.shape}"
        raise ValueError(msg)
    if th.shape[0] > _abi.MAX_SLO_THRESHOLDS:
        msg = f"at most {_abi.MAX_SLO_THRESHOLDS} thresholds a call, not {th.shape[0]}"
        raise ValueError(msg)
    if np.isnan(th).any():
        msg = "thresholds must not be NaN"
        raise ValueError(msg)
    return th


def latency_quantiles(lat: Any, levels: Any) -> np.ndarray:
    """The quantiles ``levels`` (each in [0, 1]) of one latency sample: float64 [len(levels)], NaN each for an empty
    sample.  For the sorted sample x[0] <= ... <= x[n-1]: ``v = (n - 1) * q``, ``lo = floor(v)``, ``hi = min(lo + 1,
    n - 1)``, ``t = v - lo``, ``d = x[hi] - x[lo]``, and ``x[hi] - d * (1 - t)`` where ``t >= 0.5``, else ``x[lo] + d * t``:
    ``np.quantile(lat, levels)`` bit for bit, written out.  The definition the device analyzer
    (``af_engine_summarize_quantiles``) is bit-equal to."""
    q = check_levels(levels)
    x = np.sort(np.asarray(lat, dtype=np.float64).reshape(-1))
    n = x.shape[0]
    if n == 0:
        return np.full(q.shape, np.nan)
    v = np.float64(n - 1) * q
    f = np.floor(v)
    lo = f.astype(np.int64)
    hi = np.minimum(lo + 1, n - 1)
    t = v - f
    a, b = x[lo], x[hi]
    with np.errstate(invalid="ignore"):
        d = b - a
        return np.where(t >= 0.5, b - d * (1.0 - t), a + d * t)


def latency_within(lat: Any, thresholds: Any) -> np.ndarray:
    """How many latencies of one sample meet each objective: ``#{lat <= threshold}``, uint32 [len(thresholds)]."""
    th = check_slo_thresholds(thresholds)
    x = np.asarray(lat, dtype=np.float64).reshape(-1)
    return np.array([np.count_nonzero(x <= t) for t in th], dtype=np.uint32)


def latency_window_quantiles(clock: np.ndarray, edges: Any, levels: Any, thresholds: Any = None,
                             window_of: str = "finish") -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Quantiles and SLO counts per time window of ONE scenario's ``rqs_clock`` [m, 2]: ``(count`` uint32 [W], ``quantiles``
    float64 [W, Q], ``within`` uint32 [W, T]``)``; the windows are :func:`latency_window_stats`'s (``edges[w] < finish <=
    edges[w + 1]``, rows in completion order).  ``edges=None``: the whole run as one window, in any row order.
    ``window_of="arrival"``: that function's windows by start time (right-censored cohorts: ``count`` is the cohort's
    completions, not its arrivals); it needs ``edges`` -- the whole run has no window."""
    q, th = check_levels(levels), check_slo_thresholds(thresholds)
    ck = np.asarray(clock, dtype=np.float64).reshape(-1, 2)
    if edges is None:
        if check_window_of(window_of) == "arrival":
            msg = "window_of='arrival' needs edges: the whole run has no window"
            raise ValueError(msg)
        cells = [ck[:, 1] - ck[:, 0]]
    else:
        cells = _window_latencies(ck, check_edges(edges), check_window_of(window_of))
    n_win = len(cells)
    count = np.array([x.shape[0] for x in cells], dtype=np.uint32)
    quant = np.stack([latency_quantiles(x, q) for x in cells]).reshape(n_win, q.shape[0])
    within = np.stack([latency_within(x, th) for x in cells]).reshape(n_win, th.shape[0])
    return count, quant, within


def spec_log(x: float) -> float:
    """The natural logarithm as the engine's arrival sampler takes it (FreeBSD / fdlibm ``e_log.c``, every operation a
    rounded float64 one in the order written): the gap of an arrival is ``-spec_log(1 - u) / rate``.  ``math.log`` is
    the platform's and differs from it in the last digit now and then.  Positive finite ``x`` only."""
    import struct

    if not (x > 0.0) or x == float("inf"):
        msg = f"spec_log takes a positive finite number, not {x!r}"
        raise ValueError(msg)
    k = 0
    u = struct.unpack("<Q", struct.pack("<d", x))[0]
    hx = u >> 32
    if hx < 0x00100000:                       # subnormal: scale up
        k -= 54
        x *= 18014398509481984.0
        u = struct.unpack("<Q", struct.pack("<d", x))[0]
        hx = u >> 32
    elif hx == 0x3FF00000 and (u & 0xFFFFFFFF) == 0:
        return 0.0
    hx = (hx + (0x3FF00000 - 0x3FE6A09E)) & 0xFFFFFFFF
    k += (hx >> 20) - 0x3FF
    hx = (hx & 0x000FFFFF) + 0x3FE6A09E
    x = struct.unpack("<d", struct.pack("<Q", (hx << 32) | (u & 0xFFFFFFFF)))[0]
    f = x - 1.0
    hfsq = 0.5 * f * f
    s = f / (2.0 + f)
    z = s * s
    w = z * z
    t1 = w * (3.999999999940941908e-01 + w * (2.222219843214978396e-01 + w * 1.531383769920937332e-01))
    t2 = z * (6.666666666666735130e-01 + w * (2.857142874366239149e-01 + w * (1.818357216161805012e-01 + w * 1.479819860511658591e-01)))
    r = t2 + t1
    dk = float(k)
    return s * (hfsq + r) + dk * 1.90821492927058770002e-10 - hfsq + f + dk * 6.93147180369123816490e-01


def arrival_times(rng: Any, dist: Any, mean: float, sigma: float, rpm: float, window_s: float, horizon: float,
                  n_draw: int, *, log: Any = spec_log) -> tuple[np.ndarray, int]:
    """The arrival times of one scenario on the host: the definition ``af_engine_summarize_arrivals`` counts.

    The reference's windowed sampler (samplers/poisson_poisson.py:51-82, gaussian_poisson.py:63-94) with its TWO clocks:
    the sampler's virtual clock ``now`` decides which sampling window a gap falls in and when the horizon is reached -- it
    JUMPS to the window's end over a window nobody is active in and over the gap that crosses a window's end -- while the
    simulation clock ``t`` only ever advances by the gaps that were yielded (rqs_generator.py:97-119: ``env.now + gap``).
    Arrival k is ``t`` after the k-th yielded gap; the two clocks drift apart at every jump.
    ``rng``: duck-typed like the reference's generator -- ``poisson(lam)``, ``normal(mean, sigma)``, ``random()`` -- one
    call per draw in the sampler's order.  ``dist``: ``"poisson"`` / ``"normal"`` (or the codes 0 / 1) of the active
    users, ``mean`` / ``sigma`` theirs, ``rpm`` requests per minute and user, ``window_s`` the user sampling window,
    ``horizon`` the total simulation time.  ``log``: the logarithm of the gap (:func:`spec_log`, the engine's).
    Returns ``times`` float64 [n_draw], ascending with ``+inf`` behind the last arrival, and ``flags``:
    ``FLAG_DRAW_OVERFLOW`` when the sampler had a further arrival for a full row, else 0."""
    normal = dist in (_abi.DIST_CODES["normal"], "normal")
    if not normal and dist not in (_abi.DIST_CODES["poisson"], "poisson"):
        msg = f"active users are 'poisson' or 'normal', not {dist!r}"
        raise ValueError(msg)
    n_draw = int(n_draw)
    times = np.full(n_draw, np.inf, dtype=np.float64)
    rps_per_user = float(rpm) / 60.0
    now = window_end = lam = t = 0.0
    k = 0
    while now < horizon:
        if now >= window_end:
            window_end = now + float(window_s)
            users = max(0.0, float(rng.normal(mean, sigma))) if normal else float(rng.poisson(mean))
            lam = users * rps_per_user
        if lam <= 0.0:
            now = window_end
            continue
        u = max(float(rng.random()), 1e-15)
        dt = -log(1.0 - u) / lam
        if now + dt > horizon:
            break
        if now + dt >= window_end:
            now = window_end
            continue
        if k == n_draw:
            return times, _abi.FLAG_DRAW_OVERFLOW
        now += dt
        t = t + dt
        times[k] = t
        k += 1
    return times, 0


def arrival_window_counts(times: Any, edges: Any) -> np.ndarray:
    """Cumulative arrival counts at the window edges: ``bounds[k] = #{ finite t in times : t <= edges[k] }``
    (``np.searchsorted(side="right")``), int64 [W + 1]; window w holds ``bounds[w + 1] - bounds[w]`` arrivals, those with
    ``edges[w] < t <= edges[w + 1]`` -- an arrival on an edge belongs to the window that ends there, the bucket rule of the
    by-arrival latency windows.  ``times``: ascending, ``+inf`` (ignored) behind the last arrival."""
    e = check_edges(edges)
    t = np.asarray(times, dtype=np.float64).reshape(-1)
    t = t[np.isfinite(t)]
    if t.shape[0] > 1 and np.any(t[1:] < t[:-1]):
        msg = "arrival times must be ascending"
        raise ValueError(msg)
    return np.searchsorted(t, e, side="right").astype(np.int64)


def in_flight_series(clock_rows: Any, ticks: int, period: float) -> dict[str, np.ndarray]:
    """Requests in flight end to end at every sample instant of one scenario: the host definition
    ``af_engine_summarize_inflight`` is held to, word for word.

    ``clock_rows``: float64 [m, 2], the stored ``(start, finish)`` rows; ``ticks``: the scenario's sample rows ``t_s``;
    ``period``: the sample period ``p`` (sample row ``k`` is taken at ``(k + 1) * p``).  The tick of a time is ``q(t) =
    floor(t / p)`` -- one float64 division, then floor, the rule of :func:`latency_state_cells` for ``start`` --, ``a_i =
    q(start_i)``, ``f_i = q(finish_i)``.  Request i is counted in the rows ``a_i <= k < f_i``, clipped to ``[0, t_s)``: the
    samples taken strictly after its start and at or before its finish, as the quotient sees them (the row a request "met
    on arrival", ``q - 1``, does not contain it; the next one does).  Counted nowhere: ``start`` or ``finish`` NaN,
    ``start < 0``, ``f_i <= a_i`` (a request that lived between two samples, or ``finish < start``), ``a_i >= t_s``; the
    comparisons with ``t_s`` are made on the float64 quotients, so a huge ``finish / p`` clips.
    Returns uint32 [t_s] each: ``started[k] = #{a_i == k}``, ``finished[k] = #{f_i == k}`` (a counted row with ``f_i >=
    t_s`` is in none: still in flight at the last sample) and ``in_flight[k] = #{a_i <= k < f_i}``, which is also
    ``cumsum(started - finished)``.  COMPLETED requests only: a dropped request and one still in flight when the run ended
    are in no clock row, so the last seconds of a run under-count (``lost`` of :meth:`BatchedResults.arrival_summary`
    says by how much)."""
    p, t_s = float(period), int(ticks)
    if not (np.isfinite(p) and p > 0.0):
        msg = f"period must be a finite number above 0, not {period!r}"
        raise ValueError(msg)
    if t_s != ticks or not 0 <= t_s < 2 ** 31:
        msg = f"ticks must be a whole number in [0, 2^31), not {ticks!r}"
        raise ValueError(msg)
    ck = np.asarray(clock_rows, dtype=np.float64).reshape(-1, 2)
    start, finish = ck[:, 0], ck[:, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        qa, qf = np.floor(start / p), np.floor(finish / p)
        ok = (start >= 0.0) & ~np.isnan(finish) & (qa < float(t_s)) & (qf > qa)
    a = qa[ok].astype(np.int64)
    f = np.minimum(qf[ok], float(t_s)).astype(np.int64)
    started = np.bincount(a, minlength=t_s)[:t_s]
    finished = np.bincount(f, minlength=t_s + 1)[:t_s]
    in_flight = np.cumsum(started - finished)
    return {"started": started.astype(np.uint32), "finished": finished.astype(np.uint32), "in_flight": in_flight.astype(np.uint32)}


def check_in_flight_bins(threshold: Any, bins: Any, lo: Any) -> tuple[int, int, int]:
    """``threshold``, ``bins`` and ``lo`` of the in-flight statistics as whole numbers, or ValueError: ``threshold`` and ``lo``
    in [0, 2^32), ``bins`` 0 (no histogram) .. 1024 (``AF_MAX_SERIES_HISTOGRAM_BINS``)."""
    out = []
    for name, v, top in (("threshold", threshold, 2 ** 32 - 1), ("bins", bins, 1024), ("lo", lo, 2 ** 32 - 1)):
        if isinstance(v, bool) or int(v) != v or not 0 <= int(v) <= top:
            msg = f"{name} must be a whole number in [0, {top}], not {v!r}"
            raise ValueError(msg)
        out.append(int(v))
    return out[0], out[1], out[2]


def in_flight_window_stats(members: Any, tick_edges: Any, threshold: int = 0, bins: int = 0, lo: int = 0) -> dict[str, np.ndarray]:
    """The statistics of one cell row of ``af_engine_summarize_inflight`` on the host: ``members`` is the ``in_flight``
    vector of every scenario of a group (one array, or a sequence of arrays of their own lengths ``t_s``), window w holds
    the values ``in_flight[s][k]``, ``min(b[w], t_s) <= k < min(b[w + 1], t_s)``, of all of them.  Returns [W] each:
    ``count`` int64, ``sum`` uint64, ``min``, ``max``, ``above`` (the values > ``threshold``) int64 and, with ``bins`` > 0,
    ``hist`` int64 [W, bins] (bin b: the values equal to ``lo + b``; the last bin takes everything above it) and ``under``
    (the values < ``lo``); an empty cell is all zeros."""
    b = check_tick_edges(tick_edges).astype(np.int64)
    thr, n_bins, lo_v = check_in_flight_bins(threshold, bins, lo)
    rows = [np.asarray(members)] if isinstance(members, np.ndarray) and members.ndim == 1 else [np.asarray(v) for v in members]
    n_win = int(b.shape[0] - 1)
    out = {k: np.zeros(n_win, dtype=np.int64) for k in ("count", "min", "max", "above")}
    out["sum"] = np.zeros(n_win, dtype=np.uint64)
    if n_bins:
        out["hist"] = np.zeros((n_win, n_bins), dtype=np.int64)
        out["under"] = np.zeros(n_win, dtype=np.int64)
    for w in range(n_win):
        v = np.concatenate([r[min(int(b[w]), r.shape[0]): min(int(b[w + 1]), r.shape[0])].astype(np.int64) for r in rows] or [np.zeros(0, np.int64)])
        if v.shape[0] == 0:
            continue
        out["count"][w], out["sum"][w], out["min"][w], out["max"][w] = v.shape[0], int(v.sum()), int(v.min()), int(v.max())
        out["above"][w] = int((v > thr).sum())
        if n_bins:
            out["under"][w] = int((v < lo_v).sum())
            out["hist"][w] = np.bincount(np.minimum(v[v >= lo_v] - lo_v, n_bins - 1), minlength=n_bins)
    return out


MAX_ALERT_RULES = 32   # AF_MAX_ALERT_RULES
ALERT_CELL_KEYS = ("fired", "episodes", "longest", "longest_start", "first", "last")
ALERT_GROUP_KEYS = ("members", "fired_members", "open_members", "fire_ticks", "fire_episodes")


def _exact_fraction(x: Any, name: str) -> Any:
    """``x`` as an exact ``Fraction``: ints and Fractions as they are, a float by its ``repr`` (0.999 is 999/1000)."""
    from fractions import Fraction

    if isinstance(x, bool):
        msg = f"{name} must be a number, not {x!r}"
        raise ValueError(msg)
    if isinstance(x, (int, np.integer)):
        return Fraction(int(x))
    if isinstance(x, Fraction):
        return x
    v = float(x)
    if not math.isfinite(v):
        msg = f"{name} must be finite, not {x!r}"
        raise ValueError(msg)
    return Fraction(repr(v))


def alert_rule(long_s: float, short_s: float | None = None, *, bad_share: Any = None, objective: Any = None, burn_rate: Any = None,
               hold_s: float = 0.0, min_total: int = 1) -> dict[str, Any]:
    """One burn-rate alert rule in SECONDS, as an SLO is written: the alert burns where the share of bad requests (latency
    above the call's ``slo_s``) over the last ``long_s`` seconds AND over the last ``short_s`` seconds (default: ``long_s``, a
    single-window rule) is ABOVE the share, with at least ``min_total`` completions in the long look-back, and fires once that
    has held for ``hold_s`` seconds of consecutive evaluations (the ``for:`` clause; 0: at once).  The share is either
    ``bad_share`` or ``burn_rate * (1 - objective)`` -- exactly one of the two ways --, kept as an exact ``Fraction``: ints
    and Fractions as they are, a float by its ``repr`` (``objective=0.999, burn_rate=14.4`` is 9/625).  ValueError if the share
    is below 0, above 1 or has a denominator above 2^32 - 1.  The seconds become ticks where the plan's sample period is
    known (:func:`alert_rule_ticks`).  Returns a dict: ``long_s``, ``short_s``, ``share``, ``hold_s``, ``min_total``."""
    if (bad_share is None) == (objective is None and burn_rate is None) or (objective is None) != (burn_rate is None):
        msg = "pass exactly one of bad_share, or objective together with burn_rate"
        raise ValueError(msg)
    if bad_share is not None:
        share = _exact_fraction(bad_share, "bad_share")
    else:
        share = _exact_fraction(burn_rate, "burn_rate") * (1 - _exact_fraction(objective, "objective"))
    if share < 0 or share > 1 or share.denominator > 0xFFFFFFFF:
        msg = f"the bad share must lie in [0, 1] with a denominator of at most 2^32 - 1, not {share}"
        raise ValueError(msg)
    if isinstance(min_total, bool) or int(min_total) != min_total or not 0 <= int(min_total) <= 0xFFFFFFFF:
        msg = f"min_total must be a whole number in [0, 2^32), not {min_total!r}"
        raise ValueError(msg)
    long_v, short_v, hold_v = float(long_s), float(long_s if short_s is None else short_s), float(hold_s)
    if not (math.isfinite(long_v) and math.isfinite(short_v) and 0.0 < short_v <= long_v):
        msg = f"0 < short_s <= long_s must hold, not short_s = {short_v!r}, long_s = {long_v!r}"
        raise ValueError(msg)
    if not (math.isfinite(hold_v) and hold_v >= 0.0):
        msg = f"hold_s must be a number of seconds >= 0, not {hold_s!r}"
        raise ValueError(msg)
    return {"long_s": long_v, "short_s": short_v, "share": share, "hold_s": hold_v, "min_total": int(min_total)}


def seconds_to_ticks(x: float, sample_period: float) -> int:
    """``x`` seconds as ``round(x / p)`` ticks; ValueError unless ``|ticks * p - x| <= 1e-9 * max(1, x)``."""
    v, p = float(x), float(sample_period)
    if not (math.isfinite(v) and v >= 0.0):
        msg = f"a number of seconds >= 0 is needed, not {x!r}"
        raise ValueError(msg)
    t = int(round(v / p))
    if abs(t * p - v) > 1e-9 * max(1.0, v):
        msg = f"{x!r} s is not a multiple of the sample period ({sample_period!r} s)"
        raise ValueError(msg)
    return t


def alert_rule_ticks(rule: Any, sample_period: float) -> tuple[int, int, int, int, int, int]:
    """A rule as the device takes it, ``(long_ticks, short_ticks, num, den, min_total, hold_ticks)``: a dict of
    :func:`alert_rule` converted with :func:`seconds_to_ticks` (``hold_s = 0`` is ``hold_ticks = 1``), or six whole numbers
    that are ticks already."""
    if isinstance(rule, dict):
        share = rule["share"]
        hold = seconds_to_ticks(rule["hold_s"], sample_period)
        return (seconds_to_ticks(rule["long_s"], sample_period), seconds_to_ticks(rule["short_s"], sample_period),
                int(share.numerator), int(share.denominator), int(rule["min_total"]), max(hold, 1))
    r = tuple(int(v) for v in rule)
    if len(r) != 6 or any(int(v) != v for v in rule):
        msg = f"a rule is alert_rule(...) or six whole numbers (long_ticks, short_ticks, num, den, min_total, hold_ticks), not {rule!r}"
        raise ValueError(msg)
    return r   # type: ignore[return-value]


def check_alert_rules(rules: Any, sample_period: float | None = None) -> np.ndarray:
    """The rules as uint32 [R, 6] (:func:`alert_rule_ticks`), or ValueError: 1 .. 32 rules, ``long_ticks >= short_ticks >= 1``,
    ``den >= 1``, ``num <= den``, ``hold_ticks >= 1``, every field in [0, 2^32)."""
    items = [rules] if isinstance(rules, dict) else list(rules)
    if len(items) == 6 and all(isinstance(v, (int, np.integer)) for v in items):
        items = [tuple(items)]
    if not 1 <= len(items) <= MAX_ALERT_RULES:
        msg = f"1 .. {MAX_ALERT_RULES} rules are needed, not {len(items)}"
        raise ValueError(msg)
    rows = []
    for j, it in enumerate(items):
        if isinstance(it, dict) and sample_period is None:
            msg = "a rule in seconds needs the sample period"
            raise ValueError(msg)
        r = alert_rule_ticks(it, sample_period if sample_period is not None else 1.0)
        long_t, short_t, num, den, min_total, hold = r
        if any(not 0 <= v <= 0xFFFFFFFF for v in r) or short_t < 1 or long_t < short_t or den < 1 or num > den or hold < 1:
            msg = f"rule {j}: long_ticks >= short_ticks >= 1, den >= 1, num <= den and hold_ticks >= 1 must hold, not {r}"
            raise ValueError(msg)
        rows.append(r)
    return np.asarray(rows, dtype=np.uint32).reshape(-1, 6)


def completion_ticks(rows: Any, ticks: int, period: float, slo: float) -> dict[str, np.ndarray]:
    """Completions and bad completions per tick of one scenario: the first half of the host definition
    ``af_engine_summarize_alerts`` is held to, word for word.  ``rows``: float64 [m, 2], the stored ``(start, finish)`` rows;
    ``ticks``: the scenario's sample rows ``t_s``.  The tick of a completion is ``f_i = floor(finish_i / period)``, one float64
    division and then floor (the rule of :func:`in_flight_series`); row i is COUNTED iff ``start_i`` and ``finish_i`` are not NaN
    and ``0 <= f_i < t_s``, compared on the float64 quotient (a huge or infinite quotient clips).  Nothing else is rejected:
    ``start < 0``, ``finish < start`` and a latency below a tick are counted -- a monitor sees every completion.  Row i is BAD
    iff ``finish_i - start_i > slo`` as float64 (``slo = +inf``: nothing is bad; NaN is refused).  Returns uint32 [t_s] each:
    ``total[k] = #{counted i : f_i == k}`` and ``bad[k]``, whatever the order of the rows.  COMPLETED requests only: a
    dropped request and one still in flight when the run ended are in no clock row."""
    p, t_s, s = float(period), int(ticks), float(slo)
    if not (np.isfinite(p) and p > 0.0):
        msg = f"period must be a finite number above 0, not {period!r}"
        raise ValueError(msg)
    if t_s != ticks or not 0 <= t_s < 2 ** 31:
        msg = f"ticks must be a whole number in [0, 2^31), not {ticks!r}"
        raise ValueError(msg)
    if math.isnan(s):
        msg = "slo must not be NaN"
        raise ValueError(msg)
    ck = np.asarray(rows, dtype=np.float64).reshape(-1, 2)
    start, finish = ck[:, 0], ck[:, 1]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        qf = np.floor(finish / p)
        ok = ~np.isnan(start) & ~np.isnan(finish) & (qf >= 0.0) & (qf < float(t_s))
        is_bad = ok & ((finish - start) > s)
    total = np.bincount(qf[ok].astype(np.int64), minlength=t_s)[:t_s]
    bad = np.bincount(qf[is_bad].astype(np.int64), minlength=t_s)[:t_s]
    return {"total": total.astype(np.uint32), "bad": bad.astype(np.uint32)}


def alert_firing(total: Any, bad: Any, rules: Any) -> dict[str, np.ndarray]:
    """The rules of ``af_engine_summarize_alerts`` at every tick of one scenario, on the host.  ``total`` / ``bad``:
    :func:`completion_ticks`; ``rules``: ticks (:func:`check_alert_rules`).  With the prefix sums ``PT[k] = sum(total[:k + 1])``
    and ``PB`` the ROLLING sums of a look-back of L ticks are ``T_L[k] = PT[k] - (PT[k - L] if k >= L else 0)`` and ``B_L``
    likewise -- the first L - 1 ticks see the rows that exist.  ``cond[r, k] = B_long * den > num * T_long and B_short * den
    > num * T_short and T_long >= min_total`` (exact integers) and ``firing[r, k]`` iff ``k + 1 >= hold_ticks`` and ``cond[r,
    j]`` for every ``j`` in ``(k - hold_ticks, k]``: no hysteresis.  Returns ``cond`` and ``firing``, bool [R, ticks]."""
    r6 = check_alert_rules(rules)
    tot, bd = np.asarray(total, dtype=np.uint64).reshape(-1), np.asarray(bad, dtype=np.uint64).reshape(-1)
    if tot.shape != bd.shape:
        msg = "total and bad must have one length"
        raise ValueError(msg)
    t_s = int(tot.shape[0])
    pt, pb = np.cumsum(tot, dtype=np.uint64), np.cumsum(bd, dtype=np.uint64)
    k = np.arange(t_s, dtype=np.int64)

    def roll(p: np.ndarray, look: int) -> np.ndarray:
        back = np.zeros(t_s, dtype=np.uint64)
        if look < t_s:
            back[look:] = p[: t_s - look]
        return p - back

    cond, firing = np.zeros((r6.shape[0], t_s), dtype=bool), np.zeros((r6.shape[0], t_s), dtype=bool)
    for j, (long_t, short_t, num, den, min_total, hold) in enumerate(r6.tolist()):
        tl, bl, ts, bs = roll(pt, long_t), roll(pb, long_t), roll(pt, short_t), roll(pb, short_t)
        n64, d64 = np.uint64(num), np.uint64(den)                        # (each factor is below 2^32: no product wraps)
        c = (bl * d64 > n64 * tl) & (bs * d64 > n64 * ts) & (tl >= np.uint64(min_total))
        last_off = np.maximum.accumulate(np.where(c, -1, k)) if t_s else k
        cond[j], firing[j] = c, c & (k - last_off >= hold)
    return {"cond": cond, "firing": firing}


def alert_window_stats(firing: Any, tick_edges: Any) -> dict[str, np.ndarray]:
    """The cells of one scenario of ``af_engine_summarize_alerts`` on the host.  ``firing``: bool [R, t_s]
    (:func:`alert_firing`); window w is the ticks ``lo = min(b[w], t_s) <= k < hi = min(b[w + 1], t_s)``.  Windows choose where
    firing is reported, never what a rule sees.  Returns int64: ``count``, ``lo``, ``hi`` [W] and, [W, R] each, ``fired`` (the
    firing ticks), ``episodes`` (the maximal runs of firing ticks, clipped at the window's edges: a run across an edge counts in
    both windows), ``longest`` (the longest run), ``longest_start`` (the start of the earliest run of that length), ``first``
    and ``last`` (-1: no such tick; ``last == hi - 1``: still firing at the window's end)."""
    b = check_tick_edges(tick_edges).astype(np.int64)
    f = np.atleast_2d(np.asarray(firing, dtype=bool))
    n_rules, t_s = f.shape
    n_win = int(b.shape[0] - 1)
    lo, hi = np.minimum(b[:-1], t_s), np.minimum(b[1:], t_s)
    out = {k: np.zeros((n_win, n_rules), dtype=np.int64) for k in ("fired", "episodes", "longest")}
    out.update({k: np.full((n_win, n_rules), -1, dtype=np.int64) for k in ("longest_start", "first", "last")})
    out.update(count=hi - lo, lo=lo, hi=hi)
    for w in range(n_win):
        for r in range(n_rules):
            v = f[r, lo[w]: hi[w]]
            at = np.flatnonzero(v)
            if at.size == 0:
                continue
            d = np.diff(np.concatenate([[0], v.astype(np.int8), [0]]))
            starts, ends = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
            lengths = ends - starts
            best = int(np.argmax(lengths))                                # (the first of the longest)
            out["fired"][w, r], out["episodes"][w, r] = at.size, starts.size
            out["longest"][w, r], out["longest_start"][w, r] = int(lengths[best]), int(lo[w] + starts[best])
            out["first"][w, r], out["last"][w, r] = int(lo[w] + at[0]), int(lo[w] + at[-1])
    return out


def alert_cells(members: Any, group_ids: Any, n_groups: int, delay_bins: int = 0, delay_width: int = 1) -> dict[str, np.ndarray]:
    """The group cells of ``af_engine_summarize_alerts`` on the host.  ``members``: :func:`alert_window_stats` of every
    scenario; ``group_ids``: its group (negative: in none).  Returns int64 [G, W, R]: ``members`` (those with ``hi > lo``),
    ``fired_members`` (``first`` is a tick), ``open_members`` (``last == hi - 1``), ``fire_ticks`` (the sum of ``fired``),
    ``fire_episodes`` (the sum of ``episodes``); and with ``delay_bins`` > 0 ``delay_hist`` [G, W, R, delay_bins]: a member that
    fired adds 1 to bin ``min((first - lo) // delay_width, delay_bins - 1)``."""
    stats = list(members)
    ids = np.asarray(group_ids, dtype=np.int64).reshape(-1)
    n_bins, width = int(delay_bins), int(delay_width)
    if len(stats) != ids.shape[0] or (ids >= int(n_groups)).any():
        msg = "one group id below n_groups per member is needed"
        raise ValueError(msg)
    if not 0 <= n_bins <= 1024 or width < 1:
        msg = f"delay_bins must lie in [0, 1024] and delay_width must be >= 1, not {delay_bins!r} and {delay_width!r}"
        raise ValueError(msg)
    n_win, n_rules = stats[0]["fired"].shape if stats else (0, 0)
    out = {k: np.zeros((int(n_groups), n_win, n_rules), dtype=np.int64) for k in ALERT_GROUP_KEYS}
    if n_bins:
        out["delay_hist"] = np.zeros((int(n_groups), n_win, n_rules, n_bins), dtype=np.int64)
    for st, g in zip(stats, ids.tolist()):
        if g < 0:
            continue
        some = (st["hi"] > st["lo"])[:, None]
        did = some & (st["first"] >= 0)
        out["members"][g] += some & np.ones_like(did)
        out["fired_members"][g] += did
        out["open_members"][g] += did & (st["last"] == (st["hi"] - 1)[:, None])
        out["fire_ticks"][g] += st["fired"]
        out["fire_episodes"][g] += st["episodes"]
        if n_bins:
            w_at, r_at = np.nonzero(did)
            bins = np.minimum((st["first"][w_at, r_at] - st["lo"][w_at]) // width, n_bins - 1)
            np.add.at(out["delay_hist"][g], (w_at, r_at, bins), 1)
    return out


def alert_delay_quantiles(summary: dict[str, Any], levels: Any) -> dict[str, np.ndarray]:
    """Brackets of the detection delay read off ``delay_hist`` of :meth:`BatchedResults.alert_summary`: per (group, window,
    rule) and level q the bin that holds the member of rank ``max(ceil(q N), 1)`` among the N members that fired, delays
    ascending -- exact integer ranks, q taken by its ``repr``.  Returns float64 [G, W, R, Q]: ``lo_s <= delay < hi_s`` from
    ``delay_edges_s``; NaN where no member fired; ``hi_s`` is +inf in the last bin, which takes every longer delay."""
    if "delay_hist" not in summary:
        msg = "the summary has no delay_hist: pass delay_bins to alert_summary"
        raise ValueError(msg)
    hist = np.asarray(summary["delay_hist"], dtype=np.int64)
    edges = np.asarray(summary["delay_edges_s"], dtype=np.float64)
    qs = [_exact_fraction(q, "level") for q in np.atleast_1d(np.asarray(levels, dtype=object)).tolist()]
    if any(q < 0 or q > 1 for q in qs):
        msg = "levels must lie in [0, 1]"
        raise ValueError(msg)
    cum = np.cumsum(hist, axis=-1)
    n_fired = cum[..., -1]
    lo_s = np.full(hist.shape[:-1] + (len(qs),), np.nan)
    hi_s = lo_s.copy()
    for cell in np.ndindex(*hist.shape[:-1]):
        n_cell = int(n_fired[cell])
        if n_cell == 0:
            continue
        for j, q in enumerate(qs):
            rank = max(-((-q.numerator * n_cell) // q.denominator), 1)
            b = int(np.searchsorted(cum[cell], rank, side="left"))
            lo_s[cell + (j,)], hi_s[cell + (j,)] = edges[b], edges[b + 1]
    return {"lo_s": lo_s, "hi_s": hi_s, "fired": n_fired}


def scenario_alerts(rows: Any, ticks: int, period: float, slo: float, rules: Any, tick_edges: Any) -> dict[str, np.ndarray]:
    """One scenario through the whole host definition: :func:`completion_ticks`, :func:`alert_firing` and
    :func:`alert_window_stats`, in one dict (``rules`` in ticks, or in seconds against ``period``)."""
    r6 = check_alert_rules(rules, period)
    out = completion_ticks(rows, ticks, period, slo)
    out.update(alert_firing(out["total"], out["bad"], r6))
    out.update(alert_window_stats(out["firing"], tick_edges))
    out["rules"] = r6
    return out


def check_timeout(timeout: Any) -> float:
    """The client timeout in seconds as a float, or ValueError: it must be a finite number above 0."""
    try:
        tau = float(timeout)
    except (TypeError, ValueError):
        tau = math.nan
    if isinstance(timeout, bool) or not (math.isfinite(tau) and tau > 0.0):
        msg = f"timeout must be a finite number of seconds above 0, not {timeout!r}"
        raise ValueError(msg)
    return tau


def outcome_ticks(rows: Any, arrivals: Any, ticks: int, period: float, slo: float, timeout: float) -> dict[str, Any]:
    """Request OUTCOMES per tick of one scenario under a client timeout: the first half of the host definition
    ``af_engine_outcome_alerts`` is held to, word for word.  ``rows``: float64 [m, 2], the stored ``(start, finish)``
    rows; ``arrivals``: the scenario's arrival row, ascending (ValueError otherwise, as :func:`arrival_window_counts`), entries
    that are not finite (the ``+inf`` behind the last arrival) are no arrivals; ``ticks``: the sample rows ``t_s``; ``p =
    period``; ``tau = timeout``, finite and > 0; ``slo`` as in :func:`completion_ticks` (not NaN; ``+inf`` allowed).

    The tick of a time ``x`` is ``q(x) = floor(x / p)``: one float64 division, then floor.  It is in range iff ``0 <= q < t_s``,
    compared on the float64 quotient (the rule of :func:`completion_ticks`).

    - IN-TIME row: ``start_i`` and ``finish_i`` are not NaN and ``lat_i = finish_i - start_i <= tau``: one float64 subtraction,
      a NaN latency is not in time.  A row that is not in time is never seen as a completion: the client gave up at ``start + tau``.
    - ``C[k]`` = the number of in-time rows with ``q(finish_i) == k``;  ``Cbad[k]`` = those of ``C[k]`` with ``lat_i > slo``.
    - ``G[k]`` = the number of in-time rows with ``q(start_i + tau) == k``: one float64 addition, then the tick rule.
    - ``A[k]`` = the number of arrivals ``a`` (finite) with ``q(a + tau) == k``: the same operations.
    - ``timeouts[k] = max(A[k] - G[k], 0)``;  ``deficit = sum_k max(G[k] - A[k], 0)``;  ``timed_out = sum_k timeouts[k]``.
    - ``total[k] = C[k] + timeouts[k]``;  ``bad[k] = Cbad[k] + timeouts[k]``.

    ``deficit`` is 0 whenever the arrival row is the run's own (every stored ``start`` is, bit for bit, one of its arrivals, so a
    row and its arrival land on the same timeout tick); a deficit above 0 says the arrivals do not belong to these rows; the
    result is still defined.  Returns ``total``, ``bad``, ``timeouts``, ``completions`` (= C) uint32 [t_s] and the ints
    ``deficit`` and ``timed_out``."""
    p, t_s, s, tau = float(period), int(ticks), float(slo), check_timeout(timeout)
    if not (np.isfinite(p) and p > 0.0):
        msg = f"period must be a finite number above 0, not {period!r}"
        raise ValueError(msg)
    if t_s != ticks or not 0 <= t_s < 2 ** 31:
        msg = f"ticks must be a whole number in [0, 2^31), not {ticks!r}"
        raise ValueError(msg)
    if math.isnan(s):
        msg = "slo must not be NaN"
        raise ValueError(msg)
    a = np.asarray(arrivals, dtype=np.float64).reshape(-1)
    if a.shape[0] > 1 and not (a[1:] >= a[:-1]).all():
        msg = "arrival times must be ascending"
        raise ValueError(msg)
    ck = np.asarray(rows, dtype=np.float64).reshape(-1, 2)
    start, finish = ck[:, 0], ck[:, 1]

    def per_tick(x: np.ndarray, keep: np.ndarray) -> np.ndarray:
        q = np.floor(x / p)
        ok = keep & (q >= 0.0) & (q < float(t_s))
        return np.bincount(q[ok].astype(np.int64), minlength=t_s)[:t_s].astype(np.int64)

    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        lat = finish - start
        in_time = ~np.isnan(start) & ~np.isnan(finish) & (lat <= tau)
        c = per_tick(finish, in_time)
        c_bad = per_tick(finish, in_time & (lat > s))
        g = per_tick(start + tau, in_time)
        arr = per_tick(a + tau, np.isfinite(a))
    timeouts = np.maximum(arr - g, 0)
    return {"total": (c + timeouts).astype(np.uint32), "bad": (c_bad + timeouts).astype(np.uint32), "timeouts": timeouts.astype(np.uint32),
            "completions": c.astype(np.uint32), "deficit": int(np.maximum(g - arr, 0).sum()), "timed_out": int(timeouts.sum())}


def scenario_outcome_alerts(rows: Any, arrivals: Any, ticks: int, period: float, slo: float, timeout: float, rules: Any,
                            tick_edges: Any) -> dict[str, Any]:
    """One scenario through the whole host definition of ``af_engine_outcome_alerts``: :func:`outcome_ticks`, then
    :func:`alert_firing` and :func:`alert_window_stats` on its ``total`` / ``bad``, in one dict (``rules`` in ticks, or in
    seconds against ``period``)."""
    r6 = check_alert_rules(rules, period)
    out = outcome_ticks(rows, arrivals, ticks, period, slo, timeout)
    out.update(alert_firing(out["total"], out["bad"], r6))
    out.update(alert_window_stats(out["firing"], tick_edges))
    out["rules"] = r6
    return out


def _finish_alert_summary(out: dict[str, Any], r6: np.ndarray, b: np.ndarray, ids: np.ndarray, n_groups: int, period: float,
                          slo: float, delay_bins: int, delay_width: int) -> dict[str, Any]:
    """The derived columns of ``alert_summary`` from the raw device words (int64; a tick that does not exist is -1)."""
    from fractions import Fraction

    out["first_s"] = np.where(out["first"] >= 0, out["first"].astype(np.float64) * period, np.nan)
    out["longest_s"] = out["longest"].astype(np.float64) * period
    out["fired_s"] = out["fired"].astype(np.float64) * period
    with np.errstate(invalid="ignore", divide="ignore"):
        out["fired_share"] = np.where(out["members"] > 0, out["fired_members"] / np.maximum(out["members"], 1).astype(np.float64), np.nan)
    if delay_bins:
        edges = np.arange(delay_bins + 1, dtype=np.float64) * (delay_width * period)
        edges[-1] = np.inf                                               # (the last bin takes every longer delay)
        out["delay_edges_s"], out["delay_width"] = edges, int(delay_width)
    out["rules"] = [{"long_ticks": r[0], "short_ticks": r[1], "share": Fraction(r[2], r[3]), "min_total": r[4], "hold_ticks": r[5]}
                    for r in r6.tolist()]
    out.update(rule_ticks=r6, slo_s=float(slo), tick_edges=b, times=b[:-1].astype(np.float64) * period,
               replicas=np.bincount(ids[ids >= 0], minlength=n_groups))
    return out


def _alert_delay_bins(delay_bins: Any, delay_width_s: Any, period: float) -> tuple[int, int]:
    if isinstance(delay_bins, bool) or int(delay_bins) != delay_bins or not 0 <= int(delay_bins) <= 1024:
        msg = f"delay_bins must be a whole number in [0, 1024], not {delay_bins!r}"
        raise ValueError(msg)
    width = 1 if delay_width_s is None else seconds_to_ticks(delay_width_s, period)
    if width < 1 or width > 0xFFFFFFFF:
        msg = f"delay_width_s must be at least one sample period, not {delay_width_s!r}"
        raise ValueError(msg)
    return int(delay_bins), width


def _save_alert_summary(summ: dict[str, Any], path: str, by: Any) -> dict[str, np.ndarray]:
    """The columns of ``save_alert_summary``, written to ``path``."""
    n_groups = int(summ["replicas"].shape[0])
    cols: dict[str, np.ndarray] = {}
    if hasattr(by, "point_columns"):
        for name, v in by.point_columns().items():
            cols[f"param:{name}"] = np.asarray(v, dtype=np.float64)
    cols["replicas"] = np.asarray(summ["replicas"], dtype=np.int64)
    for k in ALERT_GROUP_KEYS:
        cols[f"alert_{k}"] = np.ascontiguousarray(summ[k][:n_groups]).astype(np.int64)
    cols["alert_fired_share"] = np.ascontiguousarray(summ["fired_share"][:n_groups])
    if "delay_hist" in summ:
        cols["alert_delay_hist"] = np.ascontiguousarray(summ["delay_hist"][:n_groups]).astype(np.int64)
        cols["alert_delay_edges_s"] = np.asarray(summ["delay_edges_s"], dtype=np.float64)
    cols["alert_rule_ticks"] = np.asarray(summ["rule_ticks"], dtype=np.float64).reshape(-1)
    cols["alert_slo_s"] = np.asarray([summ["slo_s"]], dtype=np.float64)
    if "timeout_s" in summ:
        cols["alert_timeout_s"] = np.asarray([summ["timeout_s"]], dtype=np.float64)
    cols["alert_tick_edges"] = np.asarray(summ["tick_edges"], dtype=np.float64)
    cols["alert_times"] = np.asarray(summ["times"], dtype=np.float64)
    _write_columns(path, cols, n_groups)
    return cols


MAX_EXEMPLARS = 64   # AF_MAX_EXEMPLARS


def check_exemplar_k(k: Any) -> int:
    """``k`` as a whole number in 1 .. 64 (``AF_MAX_EXEMPLARS``), or ValueError."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= MAX_EXEMPLARS:
        msg = f"k must be a whole number in [1, {MAX_EXEMPLARS}], not {k!r}"
        raise ValueError(msg)
    return int(k)


def latency_exemplars(members: Any, k: int, edges: Any = None, window_of: str = "finish", *, scenario_ids: Any = None,
                      samples: Any = None, sample_period: float | None = None) -> dict[str, np.ndarray]:
    """The ``k`` SLOWEST requests per time window of one group, WITH THEIR IDENTITY: the definition
    ``af_engine_summarize_exemplars`` equals word for word.  ``members``: the stored clock rows [m_s, 2] (start, finish) of
    the group's scenarios in ascending scenario index (one array is one member); ``scenario_ids``: their indices (default
    0, 1, ...).

    * latency: ``finish - start``, one float64 subtraction; a row whose latency is NaN is in no cell.
    * window: with ``edges`` the bucket rule of :func:`latency_window_stats` on ``t = finish`` (``window_of="finish"``) or
      ``t = start`` (``"arrival"``), ``edges[w] < t <= edges[w + 1]``; rows with ``t <= edges[0]``, ``t > edges[W]`` or ``t``
      NaN are in no cell.  A mask on every row: completion order is neither needed nor checked.  ``edges=None``: one window
      with no condition on time (``window_of="arrival"`` is then refused).  W' = max(W, 1).
    * order within a window: larger latency first, compared as float64 values (``-0.0 == +0.0``, ``+inf`` a value like any
      other); ties by ascending scenario index, then ascending row index.  A total order.

    Returns ``total`` uint64 [W'] (the rows of the window), ``kept`` uint32 [W'] = min(k, total), ``scenario`` and ``row``
    uint32 [W', k] and ``clock`` float64 [W', k, 2] (the stored pair, bit for bit) of the first ``kept`` places; every byte of
    the slots at or past ``kept`` is 0xFF.  With ``samples`` (per member the sampled series as uint32 words [n_series,
    ticks]) and ``sample_period`` also ``state`` uint32 [W', k, n_series]: the raw words of sample row ``q - 1``, ``q =
    floor(start / sample_period)`` (the tick rule of :func:`latency_state_cells`); no state -- ``q < 1``, ``q - 1 >= ticks``,
    ``start`` NaN or negative -- is 0xFFFFFFFF in every word."""
    kk = check_exemplar_k(k)
    check_window_of(window_of)
    e = None if edges is None else check_edges(edges)
    if e is None and window_of == "arrival":
        msg = "window_of='arrival' needs edges: the whole run has no window"
        raise ValueError(msg)
    rows = [np.asarray(members, dtype=np.float64)] if isinstance(members, np.ndarray) and members.ndim == 2 else [np.asarray(m, dtype=np.float64).reshape(-1, 2) for m in members]
    ids = np.arange(len(rows), dtype=np.int64) if scenario_ids is None else np.asarray(scenario_ids, dtype=np.int64)
    if ids.shape != (len(rows),) or (np.diff(ids) <= 0).any():
        msg = "scenario_ids must be one strictly increasing index per member"
        raise ValueError(msg)
    n_win = 1 if e is None else int(e.shape[0] - 1)
    ck = np.concatenate(rows + [np.zeros((0, 2))])
    scen = np.concatenate([np.full(r.shape[0], i, dtype=np.int64) for r, i in zip(rows, ids)] + [np.zeros(0, np.int64)])
    member = np.concatenate([np.full(r.shape[0], j, dtype=np.int64) for j, r in enumerate(rows)] + [np.zeros(0, np.int64)])
    row = np.concatenate([np.arange(r.shape[0], dtype=np.int64) for r in rows] + [np.zeros(0, np.int64)])
    with np.errstate(invalid="ignore", over="ignore"):
        lat = ck[:, 1] - ck[:, 0]
    ok = ~np.isnan(lat)
    w = np.zeros(lat.shape, dtype=np.int64)
    if e is not None:
        eb = np.searchsorted(e, ck[:, 1 if window_of == "finish" else 0], side="left")   # #{edges < t}; a NaN: W + 1
        ok &= (eb >= 1) & (eb <= n_win)
        w = eb - 1
    out = {"total": np.zeros(n_win, dtype=np.uint64), "kept": np.zeros(n_win, dtype=np.uint32),
           "scenario": np.full((n_win, kk), 0xFFFFFFFF, dtype=np.uint32), "row": np.full((n_win, kk), 0xFFFFFFFF, dtype=np.uint32),
           "clock": np.full((n_win, kk, 2), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64).view(np.float64)}
    words = None
    if samples is not None:
        words = [np.ascontiguousarray(s).view(np.uint32) for s in samples]
        period = float(sample_period) if sample_period is not None else float("nan")
        if len(words) != len(rows) or any(x.ndim != 2 or x.shape[0] != words[0].shape[0] for x in words):
            msg = "samples must hold one array of words [n_series, ticks] per member"
            raise ValueError(msg)
        if not (np.isfinite(period) and period > 0.0):
            msg = f"sample_period must be a finite number above 0, not {sample_period!r}"
            raise ValueError(msg)
        out["state"] = np.full((n_win, kk, words[0].shape[0] if words else 0), 0xFFFFFFFF, dtype=np.uint32)
    for c in range(n_win):
        idx = np.flatnonzero(ok & (w == c))
        order = idx[np.lexsort((row[idx], scen[idx], -lat[idx]))][:kk]
        n = int(order.shape[0])
        out["total"][c], out["kept"][c] = idx.shape[0], n
        out["scenario"][c, :n], out["row"][c, :n], out["clock"][c, :n] = scen[order], row[order], ck[order]
        if words is not None:
            for j, i in enumerate(order):
                x = words[int(member[i])]
                start = ck[i, 0]
                q = np.floor(start / period) if start >= 0.0 else 0.0
                if q >= 1.0 and q - 1.0 < float(x.shape[1]):
                    out["state"][c, j] = x[:, int(q - 1.0)]
    return out


MAX_LATENCY_HISTOGRAM_BINS = 4096   # AF_MAX_LATENCY_HISTOGRAM_BINS


def check_latency_bins(sub_bits: Any = 5, min_exp: Any = -20, octaves: Any = 32) -> tuple[int, int, int, int]:
    """The log-linear binning ``(sub_bits, min_exp, octaves, n_bins)`` as whole numbers, or ValueError: ``sub_bits`` m in
    0 .. 8 (2^m bins an octave: a bin is 2^-m wide, relatively), ``min_exp`` e >= -1022 (the first bin starts at 2^e seconds),
    ``octaves`` o >= 1 with e + o <= 1023, and ``n_bins = o << m`` in 1 .. 4096 (``AF_MAX_LATENCY_HISTOGRAM_BINS``)."""
    vals = []
    for name, v in (("sub_bits", sub_bits), ("min_exp", min_exp), ("octaves", octaves)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            msg = f"{name} must be a whole number, not {v!r}"
            raise ValueError(msg)
        vals.append(int(v))
    m, e, o = vals
    if not 0 <= m <= 8:
        msg = f"sub_bits must lie in [0, 8], not {m}"
        raise ValueError(msg)
    if e < -1022 or o < 1 or e + o > 1023:
        msg = f"min_exp must be >= -1022, octaves >= 1 and min_exp + octaves <= 1023, not min_exp {e}, octaves {o}"
        raise ValueError(msg)
    if (o << m) > MAX_LATENCY_HISTOGRAM_BINS:
        msg = f"octaves << sub_bits must be at most {MAX_LATENCY_HISTOGRAM_BINS} bins, not {o << m}"
        raise ValueError(msg)
    return m, e, o, o << m


def latency_bin_edges(sub_bits: int = 5, min_exp: int = -20, octaves: int = 32) -> np.ndarray:
    """The edges E [n_bins + 1] of the log-linear latency bins, float64 seconds, each exact: bin b covers ``[E[b], E[b + 1])``,
    ``E[b] = ldexp(1 + (b & (2^m - 1)) / 2^m, e + (b >> m))``."""
    m, e, _, n_bins = check_latency_bins(sub_bits, min_exp, octaves)
    b = np.arange(n_bins + 1, dtype=np.int64)
    return np.ldexp(1.0 + (b & ((1 << m) - 1)) / float(1 << m), (e + (b >> m)).astype(np.int32))


def latency_bin_index(lat: Any, sub_bits: int = 5, min_exp: int = -20, octaves: int = 32) -> np.ndarray:
    """The bin of every latency by THE BIT RULE, int64 of ``lat``'s shape: with ``bits`` the 64-bit pattern of the float64
    value, ``(bits >> (52 - m)) - ((e + 1023) << m)``; -1 below the first bin (``x < 2^e``: zeros, ``-0.0``, negatives,
    denormals, ``-inf``), -2 at or above the end of the last (``x >= 2^(e + o)``, ``+inf``), -3 for a NaN.  Equal to
    ``np.searchsorted(latency_bin_edges(...), x, side="right") - 1`` inside the bins."""
    m, e, o, _ = check_latency_bins(sub_bits, min_exp, octaves)
    x = np.asarray(lat, dtype=np.float64)
    bits = np.ascontiguousarray(x).reshape(-1).view(np.uint64)
    mag = bits & np.uint64(0x7FFFFFFFFFFFFFFF)
    first, end = np.uint64((e + 1023) << 52), np.uint64((e + o + 1023) << 52)
    idx = (bits >> np.uint64(52 - m)).astype(np.int64) - ((e + 1023) << m)
    out = np.where(mag > np.uint64(0x7FF0000000000000), -3,
                   np.where(((bits >> np.uint64(63)) != 0) | (bits < first), -1, np.where(bits >= end, -2, idx)))
    return out.astype(np.int64).reshape(x.shape)


def latency_histogram(members: Any, edges: Any = None, window_of: str = "finish", *, sub_bits: int = 5, min_exp: int = -20,
                      octaves: int = 32) -> dict[str, np.ndarray]:
    """The log-linear latency histogram per time window of ONE group: the definition
    ``af_engine_summarize_latency_histogram`` equals word for word.  ``members``: the stored clock rows [m_s, 2] (start,
    finish) of the group's scenarios (one array is one member).

    * latency: ``finish - start``, one float64 subtraction, binned by :func:`latency_bin_index`.
    * window: with ``edges`` the bucket rule of :func:`latency_exemplars` on ``t = finish`` (``window_of="finish"``) or ``t =
      start`` (``"arrival"``), ``edges[w] < t <= edges[w + 1]``; rows with ``t <= edges[0]``, ``t > edges[W]`` or ``t`` NaN are
      in no cell.  A mask on every row: completion order is neither needed nor checked.  ``edges=None``: one window with no
      condition on time (``window_of="arrival"`` is then refused).  W' = max(W, 1).

    Returns ``count`` uint64 [W'] (the rows of the window), ``hist`` uint32 [W', n_bins] and ``under``, ``over``, ``nan`` uint32
    [W'] with ``under + over + nan + hist.sum(axis=1) == count``.  Only integer additions: histograms over the same windows
    and binning add word by word."""
    m, e0, o, n_bins = check_latency_bins(sub_bits, min_exp, octaves)
    check_window_of(window_of)
    e = None if edges is None else check_edges(edges)
    if e is None and window_of == "arrival":
        msg = "window_of='arrival' needs edges: the whole run has no window"
        raise ValueError(msg)
    rows = [np.asarray(members, dtype=np.float64)] if isinstance(members, np.ndarray) and members.ndim == 2 else [np.asarray(r, dtype=np.float64).reshape(-1, 2) for r in members]
    ck = np.concatenate(rows + [np.zeros((0, 2))])
    n_win = 1 if e is None else int(e.shape[0] - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        b = latency_bin_index(ck[:, 1] - ck[:, 0], m, e0, o)
    ok = np.ones(b.shape, dtype=bool)
    w = np.zeros(b.shape, dtype=np.int64)
    if e is not None:
        eb = np.searchsorted(e, ck[:, 1 if window_of == "finish" else 0], side="left")   # #{edges < t}; a NaN: W + 1
        ok = (eb >= 1) & (eb <= n_win)
        w = eb - 1
    out = {"count": np.bincount(w[ok], minlength=n_win).astype(np.uint64)}
    inside = ok & (b >= 0)
    out["hist"] = np.bincount(w[inside] * n_bins + b[inside], minlength=n_win * n_bins).reshape(n_win, n_bins).astype(np.uint32)
    for name, code in (("under", -1), ("over", -2), ("nan", -3)):
        out[name] = np.bincount(w[ok & (b == code)], minlength=n_win).astype(np.uint32)
    return out


_LHIST_COUNTS = ("hist", "count", "under", "over", "nan")


def _latency_histogram_parts(summary: Any) -> dict[str, Any]:
    """A latency histogram summary -- what ``latency_histogram_summary`` returns, or the columns :func:`load_summary` reads
    from ``save_latency_histogram_summary``'s file -- with numpy int64 counts: ``hist`` [G, W', B], the others [G, W']."""
    saved = "lhist_hist" in summary
    pre = "lhist_" if saved else ""
    out: dict[str, Any] = {}
    for k in _LHIST_COUNTS:
        v = summary[pre + k]
        out[k] = np.asarray(v.cpu().numpy() if hasattr(v, "cpu") else v).astype(np.int64)
    for k in ("sub_bits", "min_exp", "octaves"):
        out[k] = int(np.asarray(summary[pre + k]).reshape(-1)[0])
    m, e0, o, n_bins = check_latency_bins(out["sub_bits"], out["min_exp"], out["octaves"])
    edges = summary.get("window_edges") if saved else summary.get("edges")
    out["edges"] = None if edges is None else np.asarray(edges, dtype=np.float64)
    out["window_of"] = str(np.asarray(summary["window_of"]).reshape(-1)[0])
    out["replicas"] = np.asarray(summary["replicas"], dtype=np.int64)
    out["bin_edges"] = latency_bin_edges(m, e0, o)
    n_win = 1 if out["edges"] is None else int(out["edges"].shape[0] - 1)
    if out["hist"].ndim != 3 or out["hist"].shape[1:] != (n_win, n_bins) or any(out[k].shape != out["hist"].shape[:2] for k in _LHIST_COUNTS[1:]):
        msg = f"not a latency histogram summary: hist of shape {out['hist'].shape} for {n_win} windows and {n_bins} bins"
        raise ValueError(msg)
    return out


def latency_histogram_quantiles(summary: Any, levels: Any) -> dict[str, np.ndarray]:
    """BRACKETS of any latency quantiles, read off a latency histogram summary after the fact: numpy float64 ``lo`` and ``hi``
    [G, W', L] with ``lo <= np.quantile(valid latencies of the cell, q) < hi`` for every level q in [0, 1].  The sample of a
    cell is its ``N = count - nan`` valid values, ``under`` below bin 0 and ``over`` above the last bin.  ``np.quantile``
    interpolates between the order statistics ``floor((N - 1) q)`` and ``ceil((N - 1) q)``: ``lo`` is the lower edge of the
    bin that holds the first, ``hi`` the upper edge of the bin that holds the second -- ``hi / lo <= (1 + 2^-m)^2`` when they
    lie in the same or in adjacent bins.  In ``under``: ``lo = -inf`` (``hi`` = the first edge); in ``over``: ``hi = +inf``;
    an empty cell: NaN."""
    p = _latency_histogram_parts(summary)
    q = np.array(levels, dtype=np.float64).reshape(-1)
    if not ((q >= 0.0) & (q <= 1.0)).all():
        msg = "quantile levels must lie in [0, 1]"
        raise ValueError(msg)
    E = p["bin_edges"]
    lower = np.concatenate([[-np.inf], E])            # entry 0: under, 1 .. B: the bins, B + 1: over
    upper = np.concatenate([E, [np.inf]])
    cum = np.cumsum(np.concatenate([p["under"][..., None], p["hist"], p["over"][..., None]], axis=2), axis=2)
    n = cum[..., -1]
    shape = n.shape
    lo = np.full((*shape, q.shape[0]), np.nan)
    hi = np.full((*shape, q.shape[0]), np.nan)
    for c in np.ndindex(*shape):
        if n[c] == 0:
            continue
        pos = float(n[c] - 1) * q
        first = np.searchsorted(cum[c], np.floor(pos).astype(np.int64), side="right")
        second = np.searchsorted(cum[c], np.ceil(pos).astype(np.int64), side="right")
        lo[c], hi[c] = lower[first], upper[second]
    return {"lo": lo, "hi": hi, "levels": q}


def _same_latency_histogram_cells(a: dict[str, Any], b: dict[str, Any]) -> None:
    for k in ("sub_bits", "min_exp", "octaves", "window_of"):
        if a[k] != b[k]:
            msg = f"the two latency histograms differ in {k}: {a[k]!r} and {b[k]!r}"
            raise ValueError(msg)
    if (a["edges"] is None) != (b["edges"] is None) or (a["edges"] is not None and not np.array_equal(a["edges"], b["edges"])):
        msg = "the two latency histograms differ in their window edges"
        raise ValueError(msg)
    if a["hist"].shape[0] != b["hist"].shape[0]:
        msg = f"the two latency histograms differ in their number of groups: {a['hist'].shape[0]} and {b['hist'].shape[0]}"
        raise ValueError(msg)


def latency_histogram_merge(a: Any, b: Any, *more: Any) -> dict[str, Any]:
    """The sum of two (or more) latency histogram summaries over the same cells -- two devices, a member split, yesterday's
    saved sweep and today's: the counts add word by word, ``replicas`` too.  Each is what ``latency_histogram_summary``
    returns or what :func:`load_summary` reads from its dump.  Binning, ``edges``, ``window_of`` and the number of groups must
    be equal, otherwise ValueError.  Returns a summary with numpy int64 counts."""
    out = _latency_histogram_parts(a)
    for other in (b, *more):
        p = _latency_histogram_parts(other)
        _same_latency_histogram_cells(out, p)
        for k in _LHIST_COUNTS:
            out[k] = out[k] + p[k]
        out["replicas"] = out["replicas"] + p["replicas"]
    return out


def latency_histogram_regroup(summary: Any, groups: Any = None, windows: Any = None) -> dict[str, Any]:
    """Coarsen a latency histogram summary after the run by summing cells.  ``groups``: for every group its new group, -1 to
    drop it (marginalise a grid axis: map the points that differ only in it to one id).  ``windows``: ranges ``(w0, w1)`` of
    consecutive windows ``w0 <= w < w1``, each starting where the one before it ended, so the result has the edges
    ``edges[w0]`` of every range and ``edges[w1]`` of the last.  Returns a summary (numpy int64 counts): the quantile, merge
    and distance functions work on it."""
    p = _latency_histogram_parts(summary)
    n_groups, n_win = p["hist"].shape[:2]
    if groups is not None:
        ids = np.asarray(groups)
        if ids.shape != (n_groups,) or not np.issubdtype(ids.dtype, np.integer) or ids.max(initial=-1) < 0:
            msg = f"groups must give one whole new group id per group ({n_groups}), at least one of them kept"
            raise ValueError(msg)
        ids = ids.astype(np.int64)
        kept = ids >= 0
        new_n = int(ids.max()) + 1
        for k in _LHIST_COUNTS:
            acc = np.zeros((new_n, *p[k].shape[1:]), dtype=np.int64)
            np.add.at(acc, ids[kept], p[k][kept])
            p[k] = acc
        p["replicas"] = np.bincount(ids[kept], weights=p["replicas"][kept], minlength=new_n).astype(np.int64)
    if windows is not None:
        rng = [(int(a), int(b)) for a, b in windows]
        if not rng or any(not 0 <= a < b <= n_win for a, b in rng) or any(rng[k][1] != rng[k + 1][0] for k in range(len(rng) - 1)):
            msg = f"windows must be ranges (w0, w1) with 0 <= w0 < w1 <= {n_win}, each starting where the one before ended"
            raise ValueError(msg)
        for k in _LHIST_COUNTS:
            p[k] = np.stack([p[k][:, a:b].sum(axis=1) for a, b in rng], axis=1)
        if p["edges"] is not None:
            p["edges"] = p["edges"][[rng[0][0]] + [b for _, b in rng]]
    return p


def latency_histogram_distance(summary: Any, a: Any, b: Any) -> dict[str, Any]:
    """The two-sample Kolmogorov-Smirnov distance between cells ``a`` and ``b`` of a latency histogram summary on the bin
    grid: two grid points, a window before an outage and one after it.  ``a`` and ``b`` are ``(group, window)`` index pairs,
    or arrays [..., 2] of them.  With the cumulative valid counts ``ca_k``, ``cb_k`` (``under`` first, ``over`` last) and
    ``Na``, ``Nb`` the valid values of the cells: ``num = max_k |ca_k Nb - cb_k Na|`` and ``den = Na Nb`` as exact Python
    ints (object arrays for arrays of pairs), ``d = num / den`` float64 -- NaN where either cell is empty."""
    p = _latency_histogram_parts(summary)
    pa, pb = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    if pa.shape != pb.shape or pa.ndim < 1 or pa.shape[-1] != 2:
        msg = f"a and b must be (group, window) pairs of the same shape, not {pa.shape} and {pb.shape}"
        raise ValueError(msg)
    n_groups, n_win = p["hist"].shape[:2]
    for x in (pa, pb):
        if ((x < 0) | (x >= np.array([n_groups, n_win]))).any():
            msg = f"a (group, window) pair lies outside the {n_groups} groups and {n_win} windows"
            raise ValueError(msg)
    cum = np.cumsum(np.concatenate([p["under"][..., None], p["hist"], p["over"][..., None]], axis=2), axis=2)
    shape = pa.shape[:-1]
    num, den, d = np.empty(shape, dtype=object), np.empty(shape, dtype=object), np.full(shape, np.nan)
    for c in np.ndindex(*shape):
        ca, cb = cum[tuple(pa[c])].astype(object), cum[tuple(pb[c])].astype(object)
        na, nb = int(ca[-1]), int(cb[-1])
        num[c], den[c] = int(abs(ca * nb - cb * na).max()), na * nb
        if den[c]:
            d[c] = num[c] / den[c]
    if not shape:
        return {"d": float(d), "num": num[()], "den": den[()]}
    return {"d": d, "num": num, "den": den}


PAIR_NONE = 0xFFFFFFFF          # AF_PAIR_NONE: an arrival without a row
MAX_PAIR_THRESHOLDS = 64        # AF_MAX_PAIR_THRESHOLDS
_PAIR_COUNTS = ("both", "only_a", "only_b", "neither", "nan")
_PAIR_CELL_SUMS = (*_PAIR_COUNTS, "slower", "faster", "equal", "above", "hist_pos", "hist_neg", "under_pos", "under_neg", "over_pos", "over_neg")


def check_pair_thresholds(thresholds: Any) -> np.ndarray:
    """The thresholds of the paired differences as float64 [T]: at most 64, finite, of either sign (seconds of ``d``)."""
    th = np.ascontiguousarray([] if thresholds is None else thresholds, dtype=np.float64).reshape(-1)
    if th.shape[0] > MAX_PAIR_THRESHOLDS or not np.isfinite(th).all():
        msg = f"at most {MAX_PAIR_THRESHOLDS} finite thresholds, not {th.tolist()}"
        raise ValueError(msg)
    return th


def _pair_rows(clock: Any, arrivals: np.ndarray) -> tuple[np.ndarray, int, np.ndarray]:
    """THE MATCH of one side: ``row`` uint32 [m] (``PAIR_NONE``: no row), the unmatched rows and the clock rows [m_x, 2]."""
    ck = np.ascontiguousarray(clock, dtype=np.float64).reshape(-1, 2)
    m = int(arrivals.shape[0])
    start = np.ascontiguousarray(ck[:, 0])
    j = np.searchsorted(arrivals, start, side="left")                 # a NaN start: m
    row = np.full(m, PAIR_NONE, dtype=np.uint32)
    a_bits, s_bits = arrivals.view(np.uint64), start.view(np.uint64)
    for i in range(ck.shape[0]):                                      # ascending i: the smallest row index keeps the arrival
        if j[i] < m and a_bits[j[i]] == s_bits[i] and row[j[i]] == PAIR_NONE:
            row[j[i]] = i
    return row, int(ck.shape[0] - np.count_nonzero(row != PAIR_NONE)), ck


def paired_fixed_sum(values: np.ndarray, mask: np.ndarray, j0: int, j1: int) -> float:
    """THE FIXED-ORDER SUM of ``values[j]`` over ``j0 <= j < j1`` with ``mask[j]``: whole rows of 64 aligned at j = 0, a masked
    entry adds nothing (+0.0), the rows added one after the other from +0.0, then the 64 sums halved five times."""
    if j1 <= j0:
        return 0.0
    lo, hi = (j0 // 64) * 64, -(-j1 // 64) * 64
    v = np.zeros(hi - lo, dtype=np.float64)
    v[j0 - lo: j1 - lo] = np.where(mask[j0:j1], values[j0:j1], 0.0)
    part = np.zeros(64, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in v.reshape(-1, 64):
            part = part + r
        h = 32
        while h:
            part = part[:h] + part[h: 2 * h]
            h //= 2
    return float(part[0])


def latency_pairs(clock_a: Any, clock_b: Any, times: Any, edges: Any = None, *, thresholds: Any = None, sub_bits: int = 5,
                  min_exp: int = -20, octaves: int = 32) -> dict[str, Any]:
    """The latency differences of ONE pair of scenarios that were sent the same requests: the definition
    ``af_engine_summarize_pairs`` equals word for word.  ``clock_a`` / ``clock_b``: the stored clock rows [m_x, 2] (start,
    finish) of side a and b; ``times``: their common arrival row, ascending (``+inf`` entries behind the last arrival are
    dropped: A = the m finite ones).

    * match: row i of side x maps to ``j = np.searchsorted(A, start_i, "left")`` when ``j < m`` and ``A[j]`` has the bit pattern
      of ``start_i`` (the uint64 words are compared: a NaN never matches); ``row_x[j]`` is the smallest such i, ``PAIR_NONE``
      without one; ``unmatched_x`` counts the rows that map nowhere or lose their j to a smaller row index.
    * arrival j: ``state`` 3 both rows set, 1 only a, 2 only b, 0 neither (dropped, or still in flight at the end of the run,
      on one or both sides).  For state 3: ``lat_x = finish - start`` and ``d = lat_b - lat_a``; a NaN ``d`` counts in ``nan``
      and enters nothing else.
    * window: by ``A[j]``, ``edges[w] < A[j] <= edges[w + 1]``: the ranges of j between ``np.searchsorted(A, edges, "right")``
      (``bounds``).  ``edges=None``: one window over every arrival.  W' = max(W, 1).

    Returns per arrival ``row_a``, ``row_b`` uint32 [m], ``state`` uint8 [m], ``d``, ``lat_a`` float64 [m] (NaN unless state 3);
    ``unmatched_a``, ``unmatched_b``; per window uint32 [W'] ``both``, ``only_a``, ``only_b``, ``neither``, ``nan`` and float64
    ``sum_d``, ``sum_a`` (:func:`paired_fixed_sum` over the state-3 arrivals with ``d`` not NaN); and what the pair brings to
    its group's cells (:func:`latency_pair_cells`): ``slower`` (d > 0), ``faster`` (d < 0), ``equal`` (d == 0) uint64 [W'],
    ``above`` uint64 [W', T] (``d > thresholds[t]``), ``min_d`` / ``max_d`` float64 [W'] in float order with -0.0 below +0.0
    (+inf / -inf without a value), ``hist_pos`` / ``hist_neg`` uint32 [W', n_bins] (:func:`latency_bin_index` of d, of -d),
    ``under_pos``, ``under_neg``, ``over_pos``, ``over_neg`` uint32 [W']."""
    sb, e0, o, n_bins = check_latency_bins(sub_bits, min_exp, octaves)
    th = check_pair_thresholds(thresholds)
    e = None if edges is None else check_edges(edges)
    t = np.ascontiguousarray(times, dtype=np.float64).reshape(-1)
    A = np.ascontiguousarray(t[: int(np.searchsorted(t, np.finfo(np.float64).max, side="right"))])
    m = int(A.shape[0])
    row_a, un_a, ca = _pair_rows(clock_a, A)
    row_b, un_b, cb = _pair_rows(clock_b, A)
    has_a, has_b = row_a != PAIR_NONE, row_b != PAIR_NONE
    state = (has_a.astype(np.uint8) | (has_b.astype(np.uint8) << 1)).astype(np.uint8)
    both = state == 3
    lat_a, lat_b = np.full(m, np.nan), np.full(m, np.nan)
    with np.errstate(invalid="ignore", over="ignore"):
        lat_a[both] = ca[row_a[both], 1] - ca[row_a[both], 0]
        lat_b[both] = cb[row_b[both], 1] - cb[row_b[both], 0]
        d = lat_b - lat_a
    ok = both & ~np.isnan(d)
    bounds = np.array([0, m], dtype=np.int64) if e is None else np.searchsorted(A, e, side="right").astype(np.int64)
    n_win = int(bounds.shape[0] - 1)
    out: dict[str, Any] = {"row_a": row_a, "row_b": row_b, "state": state, "d": d, "lat_a": lat_a, "unmatched_a": un_a, "unmatched_b": un_b,
                           "bounds": bounds, "arrivals": A, "edges": e, "thresholds": th, "sub_bits": sb, "min_exp": e0, "octaves": o}
    for k in _PAIR_COUNTS:
        out[k] = np.zeros(n_win, dtype=np.uint32)
    for k in ("slower", "faster", "equal"):
        out[k] = np.zeros(n_win, dtype=np.uint64)
    for k in ("under_pos", "under_neg", "over_pos", "over_neg"):
        out[k] = np.zeros(n_win, dtype=np.uint32)
    out["sum_d"], out["sum_a"] = np.zeros(n_win), np.zeros(n_win)
    out["above"] = np.zeros((n_win, th.shape[0]), dtype=np.uint64)
    out["min_d"], out["max_d"] = np.full(n_win, np.inf), np.full(n_win, -np.inf)
    out["hist_pos"], out["hist_neg"] = np.zeros((n_win, n_bins), dtype=np.uint32), np.zeros((n_win, n_bins), dtype=np.uint32)
    for w in range(n_win):
        j0, j1 = int(bounds[w]), int(bounds[w + 1])
        s = state[j0:j1]
        out["both"][w], out["only_a"][w], out["only_b"][w], out["neither"][w] = (np.count_nonzero(s == c) for c in (3, 1, 2, 0))
        out["nan"][w] = np.count_nonzero(both[j0:j1] & ~ok[j0:j1])
        out["sum_d"][w] = paired_fixed_sum(d, ok, j0, j1)
        out["sum_a"][w] = paired_fixed_sum(lat_a, ok, j0, j1)
        x = d[j0:j1][ok[j0:j1]]
        if x.shape[0] == 0:
            continue
        pos, neg = x[x > 0.0], x[x < 0.0]
        out["slower"][w], out["faster"][w], out["equal"][w] = pos.shape[0], neg.shape[0], np.count_nonzero(x == 0.0)
        out["above"][w] = [np.count_nonzero(x > v) for v in th]
        keys = _double_keys(x)
        out["min_d"][w], out["max_d"][w] = x[np.argmin(keys)], x[np.argmax(keys)]
        for side, v in (("pos", pos), ("neg", -neg)):
            b = latency_bin_index(v, sb, e0, o)
            out[f"hist_{side}"][w] = np.bincount(b[b >= 0], minlength=n_bins)
            out[f"under_{side}"][w], out[f"over_{side}"][w] = np.count_nonzero(b == -1), np.count_nonzero(b == -2)
    return out


def latency_pair_cells(pairs: Any, groups: Any = None, n_groups: int = 1) -> dict[str, np.ndarray]:
    """The cells (group g of pairs, window w) of the paired differences: what every pair of ``pairs`` (each a result of
    :func:`latency_pairs` over the same windows, thresholds and binning) brings, added into the cell of its group
    (``groups``: one id per pair, negative: in no cell; None: all in group 0).  uint64 sums [G, W'] of ``both``, ``only_a``,
    ``only_b``, ``neither``, ``nan``, ``slower``, ``faster``, ``equal``, ``above`` [G, W', T]; uint32 sums of ``hist_pos``,
    ``hist_neg`` [G, W', n_bins], ``under_pos``, ``under_neg``, ``over_pos``, ``over_neg``; ``min_d`` / ``max_d`` float64 in
    float order with -0.0 below +0.0, +inf / -inf for an empty cell; ``replicas`` [G], the pairs of each group.  Integer
    sums, min and max only: the order of the pairs does not matter, and ``equal + under_* + over_* + hist_*.sum(-1) + nan ==
    both``."""
    pairs = list(pairs)
    if not pairs:
        msg = "no pair"
        raise ValueError(msg)
    ids = np.zeros(len(pairs), dtype=np.int64) if groups is None else np.asarray(groups, dtype=np.int64).reshape(-1)
    if ids.shape[0] != len(pairs) or (ids >= n_groups).any():
        msg = f"groups must give one id below {n_groups} per pair"
        raise ValueError(msg)
    first = pairs[0]
    out: dict[str, np.ndarray] = {}
    for k in _PAIR_CELL_SUMS:
        wide = np.uint32 if k.startswith(("hist", "under", "over")) else np.uint64
        out[k] = np.zeros((n_groups, *first[k].shape), dtype=wide)
    n_win = int(first["both"].shape[0])
    out["min_d"], out["max_d"] = np.full((n_groups, n_win), np.inf), np.full((n_groups, n_win), -np.inf)
    for p, g in zip(pairs, ids):
        if g < 0:
            continue
        for k in _PAIR_CELL_SUMS:
            out[k][g] += p[k].astype(out[k].dtype)
        for w in range(n_win):
            if _double_keys(p["min_d"][w: w + 1])[0] < _double_keys(out["min_d"][g, w: w + 1])[0]:
                out["min_d"][g, w] = p["min_d"][w]
            if _double_keys(p["max_d"][w: w + 1])[0] > _double_keys(out["max_d"][g, w: w + 1])[0]:
                out["max_d"][g, w] = p["max_d"][w]
    out["replicas"] = np.bincount(ids[ids >= 0], minlength=n_groups)
    for k in ("edges", "thresholds", "sub_bits", "min_exp", "octaves"):
        out[k] = first[k]
    return out


def _paired_parts(summary: Any) -> dict[str, Any]:
    """The cell arrays of a paired summary -- what ``paired_summary`` / :func:`latency_pair_cells` return or what
    :func:`load_summary` reads from ``save_paired_summary``'s file -- as numpy, the counts int64."""
    saved = "paired_both" in summary
    pre = "paired_" if saved else ""
    out: dict[str, Any] = {}
    for k in _PAIR_CELL_SUMS:     # (paired_summary names the cells' five counts cell_both ...: both ... are its per-pair ones)
        out[k] = np.asarray(summary[f"cell_{k}" if f"cell_{k}" in summary else pre + k]).astype(np.int64)
    for k in ("min_d", "max_d"):
        out[k] = np.asarray(summary[pre + k], dtype=np.float64)
    out["replicas"] = np.asarray(summary["replicas"], dtype=np.int64)
    for k in ("sub_bits", "min_exp", "octaves"):
        out[k] = int(np.asarray(summary[pre + k]).reshape(-1)[0])
    edges = summary.get("window_edges") if saved else summary.get("edges")
    out["edges"] = None if edges is None else np.asarray(edges, dtype=np.float64)
    th = summary.get("paired_thresholds") if saved else summary.get("thresholds")
    out["thresholds"] = np.zeros(0) if th is None else np.asarray(th, dtype=np.float64).reshape(-1)
    _, _, _, n_bins = check_latency_bins(out["sub_bits"], out["min_exp"], out["octaves"])
    if out["hist_pos"].ndim != 3 or out["hist_pos"].shape[2] != n_bins or out["hist_neg"].shape != out["hist_pos"].shape:
        msg = f"not a paired summary: hist_pos of shape {out['hist_pos'].shape} for {n_bins} bins"
        raise ValueError(msg)
    return out


def paired_merge(a: Any, b: Any, *more: Any) -> dict[str, Any]:
    """The cells of two (or more) paired summaries over the same groups, windows, thresholds and binning as one: the counts
    and histograms add word by word, ``replicas`` too, ``min_d`` / ``max_d`` take the min / max in float order (-0.0 below
    +0.0) -- two halves of the pairs, yesterday's saved sweep and today's.  Returns a summary with numpy int64 counts."""
    out = _paired_parts(a)
    for other in (b, *more):
        p = _paired_parts(other)
        for k in ("sub_bits", "min_exp", "octaves"):
            if out[k] != p[k]:
                msg = f"the two paired summaries differ in {k}: {out[k]!r} and {p[k]!r}"
                raise ValueError(msg)
        if (out["edges"] is None) != (p["edges"] is None) or (out["edges"] is not None and not np.array_equal(out["edges"], p["edges"])):
            msg = "the two paired summaries differ in their window edges"
            raise ValueError(msg)
        if not np.array_equal(out["thresholds"], p["thresholds"]) or out["both"].shape != p["both"].shape:
            msg = "the two paired summaries differ in their thresholds or cells"
            raise ValueError(msg)
        for k in _PAIR_CELL_SUMS:
            out[k] = out[k] + p[k]
        out["replicas"] = out["replicas"] + p["replicas"]
        out["min_d"] = np.where(_double_keys(p["min_d"]) < _double_keys(out["min_d"]), p["min_d"], out["min_d"])
        out["max_d"] = np.where(_double_keys(p["max_d"]) > _double_keys(out["max_d"]), p["max_d"], out["max_d"])
    return out


def paired_delta_quantiles(summary: Any, levels: Any) -> dict[str, np.ndarray]:
    """BRACKETS of the quantiles of ``d`` per cell, read off the two-sided histogram of a paired summary: numpy float64 ``lo``
    and ``hi`` [G, W', L] with ``lo <= np.quantile(d of the cell, q, method="lower") < hi`` -- the signed counterpart of
    :func:`latency_histogram_quantiles`.  The sample of a cell is its ``both - nan`` values in the order ``over_neg``, the
    bins of ``hist_neg`` from the last to the first, ``under_neg``, ``equal``, ``under_pos``, the bins of ``hist_pos``,
    ``over_pos``; the order statistic ``floor((N - 1) q)`` lies in one of these entries.  A bin b of the positive side covers
    ``[E[b], E[b + 1])``; on the negative side it covers ``(-E[b + 1], -E[b]]``, so ``hi`` there is the float above ``-E[b]``.
    ``equal``: ``[-0.0, 5e-324)``.  ``over_neg`` has ``lo = -inf``, ``over_pos`` ``hi = +inf`` (a ``d`` of +inf is not below
    it).  An empty cell: NaN."""
    p = _paired_parts(summary)
    q = np.array(levels, dtype=np.float64).reshape(-1)
    if not ((q >= 0.0) & (q <= 1.0)).all():
        msg = "quantile levels must lie in [0, 1]"
        raise ValueError(msg)
    E = latency_bin_edges(p["sub_bits"], p["min_exp"], p["octaves"])
    up = np.nextafter(-E, np.inf)                      # the float above -E[b]
    lower = np.concatenate([[-np.inf], -E[:0:-1], [-E[0]], [-0.0], [0.0], E[:-1], [E[-1]]])
    upper = np.concatenate([[up[-1]], up[-2::-1], [0.0], [5e-324], [E[0]], E[1:], [np.inf]])
    col = lambda k: p[k][..., None]  # noqa: E731
    cum = np.cumsum(np.concatenate([col("over_neg"), p["hist_neg"][..., ::-1], col("under_neg"), col("equal"), col("under_pos"),
                                    p["hist_pos"], col("over_pos")], axis=2), axis=2)
    n = cum[..., -1]
    lo = np.full((*n.shape, q.shape[0]), np.nan)
    hi = np.full((*n.shape, q.shape[0]), np.nan)
    for c in np.ndindex(*n.shape):
        if n[c] == 0:
            continue
        at = np.searchsorted(cum[c], np.floor(float(n[c] - 1) * q).astype(np.int64), side="right")
        lo[c], hi[c] = lower[at], upper[at]
    return {"lo": lo, "hi": hi, "levels": q}


def groups_of_columns(columns: Any) -> tuple[np.ndarray, int]:
    """Group ids from per-scenario parameter columns (one float vector [n] each): scenarios with equal values in every column
    form a group, the groups numbered in ascending lexicographic order of their values -- for a grid with ascending axis
    values the row-major order of its points, so the ids equal ``Sweep.point``.  Returns int64 ids [n] and G."""
    cols = [np.asarray(c, dtype=np.float64).reshape(-1) for c in columns]
    if not cols or any(c.shape != cols[0].shape for c in cols) or any(np.isnan(c).any() for c in cols):
        msg = "parameter columns must be at least one vector per scenario, all of one length, without NaN"
        raise ValueError(msg)
    if cols[0].shape[0] == 0:
        msg = "no scenario is in a group"
        raise ValueError(msg)
    uniq, ids = np.unique(np.stack(cols, axis=1), axis=0, return_inverse=True)
    return np.asarray(ids, dtype=np.int64).reshape(-1), int(uniq.shape[0])


def _groups_of_named_columns(by: Any, overrides: dict[str, np.ndarray]) -> tuple[np.ndarray, int] | None:
    """``by`` given as the name(s) of per-scenario parameter columns (keys of a run's ``overrides``): their groups
    (:func:`groups_of_columns`); any other ``by``: None."""
    names = [by] if isinstance(by, str) and by != "scenario" else list(by) if isinstance(by, (list, tuple)) and by and all(isinstance(x, str) for x in by) else None
    if names is None:
        return None
    missing = [k for k in names if k not in overrides]
    if missing:
        msg = f"by names parameter columns the run does not have: {missing} (it has {sorted(overrides)})"
        raise ValueError(msg)
    return groups_of_columns([overrides[k] for k in names])


def check_tick_edges(tick_edges: Any) -> np.ndarray:
    """``tick_edges`` as a uint32 vector, or ValueError: at least two tick indices, whole, in [0, 2^32), strictly increasing."""
    raw = np.asarray(tick_edges)
    if raw.ndim != 1 or raw.shape[0] < 2:
        msg = f"tick_edges must be a vector of at least two tick indices, not of shape {raw.shape}"
        raise ValueError(msg)
    if raw.dtype.kind not in "iu":
        as_int = np.asarray(raw, dtype=np.float64)
        if not (np.isfinite(as_int).all() and (as_int == np.floor(as_int)).all()):
            msg = "tick_edges must be whole tick indices"
            raise ValueError(msg)
        raw = as_int
    if (raw < 0).any() or (raw > 0xFFFFFFFF).any():
        msg = "tick_edges must lie in [0, 2^32)"
        raise ValueError(msg)
    b = np.ascontiguousarray(raw, dtype=np.uint32)
    if not (np.diff(b.astype(np.int64)) > 0).all():
        msg = "tick_edges must be strictly increasing"
        raise ValueError(msg)
    return b


def ticks_per_window_of(window_s: float, sample_period: float) -> int:
    """``window_s`` seconds as a number of sampler ticks ``m = round(window_s / sample_period)``; ValueError unless
    ``m >= 1`` and ``m * sample_period`` is ``window_s`` to 1e-9 relative."""
    w = float(window_s)
    if not (np.isfinite(w) and w > 0.0):
        msg = f"window_s must be a positive number of seconds, not {window_s!r}"
        raise ValueError(msg)
    m = int(round(w / float(sample_period)))
    if m < 1 or abs(m * float(sample_period) - w) > 1e-9 * w:
        msg = f"window_s = {window_s!r} is not a multiple of the sample period ({sample_period!r} s)"
        raise ValueError(msg)
    return m


def tick_window_edges(ticks_per_window: int, n_ticks: int) -> np.ndarray:
    """Tick edges ``[0, m, 2 m, ..., W m]`` (uint32) of the ``W = ceil(n_ticks / m)`` windows of ``m = ticks_per_window``
    sampler ticks that cover ``n_ticks`` samples; the last window may be short (a window ends where the samples do)."""
    m = int(ticks_per_window)
    if m != ticks_per_window or m < 1:
        msg = f"ticks_per_window must be a positive whole number, not {ticks_per_window!r}"
        raise ValueError(msg)
    n_win = max(-(-int(n_ticks) // m), 1)
    return check_tick_edges(np.arange(n_win + 1, dtype=np.int64) * m)


def _resolve_tick_edges(window_s: float | None, ticks_per_window: int | None, tick_edges: Any, sample_period: float,
                        n_ticks: int) -> np.ndarray:
    if sum(x is not None for x in (window_s, ticks_per_window, tick_edges)) > 1:
        msg = "pass one of window_s, ticks_per_window and tick_edges"
        raise ValueError(msg)
    if tick_edges is not None:
        return check_tick_edges(tick_edges)
    if ticks_per_window is None:
        ticks_per_window = ticks_per_window_of(1.0 if window_s is None else window_s, sample_period)
    return tick_window_edges(ticks_per_window, n_ticks)


def ram_columns(n_series: int, n_edges: int) -> np.ndarray:
    """Boolean [n_series]: the ``ram_in_use`` columns (float32 words) of the sampled series in device order."""
    j = np.arange(n_series)
    return (j >= n_edges) & ((j - n_edges) % 3 == 2)


def series_window_stats(samples: np.ndarray, tick_edges: Any, n_edges: int, thresholds: Any = None) -> dict[str, np.ndarray]:
    """Statistics per window of ticks of ONE scenario's sampled series ``samples`` (uint32 words [n_series, ticks], the
    layout :class:`ScenarioResults` holds).  Sample ``k`` carries the label ``k * sample_period`` -- the reference's
    ``get_series`` (analyzer.py:239-244), although the collector takes it at ``(k + 1) * period`` (collector.py:53) --; window
    ``w`` holds the samples ``min(b[w], ticks) <= k < min(b[w + 1], ticks)`` of ``b = tick_edges``.  Returns ``count`` int64
    [W], ``mean`` float64 [W, S] (integer series: the exact integer sum divided once; ``ram_in_use``: the float32 values
    summed as float64; NaN in an empty window), ``min`` / ``max`` uint32 words [W, S] -- integer series: the smallest /
    largest word; ``ram_in_use``: the float minimum / maximum of the values as float32 bits, -0.0 below +0.0 (the IEEE total
    order, the one ``series_max`` of the whole-run summary has), which on non-negative values is the order of the words --
    and ``above`` uint32 [W, S]: the values ``> thresholds[j]`` (None: 0.0 each, the non-zero samples); an empty window has 0
    in all three.  The definition the device analyzer (``af_engine_summarize_series_windows``) matches."""
    b = check_tick_edges(tick_edges)
    words = np.ascontiguousarray(samples).view(np.uint32)
    if words.ndim != 2:
        msg = f"samples must be words [n_series, ticks], not of shape {words.shape}"
        raise ValueError(msg)
    n_series, ticks = words.shape
    thr = np.zeros(n_series) if thresholds is None else np.asarray(thresholds, dtype=np.float64)
    if thr.shape != (n_series,) or np.isnan(thr).any():
        msg = f"thresholds must be {n_series} values, none of them NaN"
        raise ValueError(msg)
    ram = ram_columns(n_series, n_edges)
    n_win = b.shape[0] - 1
    r = np.minimum(b.astype(np.int64), ticks)
    count = np.diff(r)
    mean = np.full((n_win, n_series), np.nan)
    mn = np.zeros((n_win, n_series), dtype=np.uint32)
    mx = np.zeros((n_win, n_series), dtype=np.uint32)
    above = np.zeros((n_win, n_series), dtype=np.uint32)
    for w in range(n_win):
        if count[w] == 0:
            continue
        seg = words[:, r[w]:r[w + 1]]
        values = seg.astype(np.float64)
        values[ram] = seg[ram].view(np.float32).astype(np.float64)
        mean[w] = np.where(ram, np.mean(values, axis=1), seg.astype(np.int64).sum(axis=1).astype(np.float64) / float(count[w]))
        # (ram_in_use: keys that order like the float values -- a negative value's bits inverted, the others above them)
        key = np.where(ram[:, None], np.where(seg >> 31 != 0, ~seg, seg | np.uint32(0x80000000)), seg)
        kmn, kmx = key.min(axis=1), key.max(axis=1)
        mn[w] = np.where(ram, np.where(kmn >> 31 != 0, kmn & np.uint32(0x7FFFFFFF), ~kmn), kmn)
        mx[w] = np.where(ram, np.where(kmx >> 31 != 0, kmx & np.uint32(0x7FFFFFFF), ~kmx), kmx)
        above[w] = (values > thr[:, None]).sum(axis=1)
    return {"count": count, "mean": mean, "min": mn, "max": mx, "above": above}


def series_window_excursions(samples: np.ndarray, tick_edges: Any, n_edges: int, thresholds: Any = None) -> dict[str, np.ndarray]:
    """Excursions above a threshold per window of ticks of ONE scenario's sampled series ``samples`` (uint32 words
    [n_series, ticks], the layout :class:`ScenarioResults` holds and :func:`series_window_stats` takes).  Window ``w`` holds
    the ticks ``lo <= k < hi``, ``lo = min(b[w], ticks)``, ``hi = min(b[w + 1], ticks)``.  Tick ``k`` of series ``j`` is
    ABOVE when its value as float64 -- the word of an integer series, the float32 value of a ``ram_in_use`` column, as
    ``above`` of :func:`series_window_stats` takes it -- is ``> thresholds[j]`` (None: 0.0 each); a RUN is a maximal stretch
    of consecutive above ticks inside the window: runs are clipped at the window's edges, and one that crosses an edge counts
    in both windows.  Returns int64 arrays, -1 for "no such tick": ``count`` [W] (``hi - lo``) and, [W, S] each, ``above``
    (the above ticks), ``runs``, ``longest`` (ticks of the longest run, 0 if none), ``longest_start`` (first tick of the
    EARLIEST run of that length), ``first`` / ``last`` (smallest / largest above tick; ``last == hi - 1``: still above at
    the window's end, otherwise ``last + 1`` is the tick at which the series had come back for good) and ``peak_tick`` (the
    smallest tick whose key is the window's largest; the key is the word, or of ``ram_in_use`` the float32 bits ``w`` as
    ``~w`` where the sign bit is set, else ``w | 0x80000000``: -0.0 below +0.0).  Ticks are absolute row indices.  The
    definition the device analyzer (``af_engine_summarize_series_excursions``) equals word for word."""
    b = check_tick_edges(tick_edges)
    words = np.ascontiguousarray(samples).view(np.uint32)
    if words.ndim != 2:
        msg = f"samples must be words [n_series, ticks], not of shape {words.shape}"
        raise ValueError(msg)
    n_series, ticks = words.shape
    thr = np.zeros(n_series) if thresholds is None else np.asarray(thresholds, dtype=np.float64)
    if thr.shape != (n_series,) or np.isnan(thr).any():
        msg = f"thresholds must be {n_series} values, none of them NaN"
        raise ValueError(msg)
    ram = ram_columns(n_series, n_edges)
    n_win = b.shape[0] - 1
    r = np.minimum(b.astype(np.int64), ticks)
    out = {k: np.full((n_win, n_series), -1, dtype=np.int64) for k in ("longest_start", "first", "last", "peak_tick")}
    out.update({k: np.zeros((n_win, n_series), dtype=np.int64) for k in ("above", "runs", "longest")})
    out["count"] = np.diff(r)
    rows = np.arange(n_series)
    for w in range(n_win):
        lo, c = int(r[w]), int(r[w + 1] - r[w])
        if c == 0:
            continue
        seg = words[:, lo:lo + c]
        with np.errstate(invalid="ignore"):   # (an integer word read as float32 may be a NaN: not taken)
            values = np.where(ram[:, None], seg.view(np.float32).astype(np.float64), seg.astype(np.float64))
        a = values > thr[:, None]
        rise = a & ~np.concatenate([np.zeros((n_series, 1), dtype=bool), a[:, :-1]], axis=1)
        idx = np.arange(c, dtype=np.int64)
        start = np.maximum.accumulate(np.where(rise, idx, -1), axis=1)    # of the run a tick lies in (where it is above)
        length = np.where(a, idx - start + 1, 0)
        at = length.argmax(axis=1)                                       # (the first maximum: the end of the earliest longest run)
        some = a.any(axis=1)
        out["above"][w] = a.sum(axis=1)
        out["runs"][w] = rise.sum(axis=1)
        out["longest"][w] = length[rows, at]
        out["longest_start"][w] = np.where(some, lo + start[rows, at], -1)
        out["first"][w] = np.where(some, lo + a.argmax(axis=1), -1)
        out["last"][w] = np.where(some, lo + c - 1 - a[:, ::-1].argmax(axis=1), -1)
        key = np.where(ram[:, None], np.where(seg >> 31 != 0, ~seg, seg | np.uint32(0x80000000)), seg)
        out["peak_tick"][w] = lo + key.argmax(axis=1)
    return out


def check_series_levels(levels: Any) -> np.ndarray:
    """``levels`` of a series-quantile call as a float64 vector, or ValueError: one dimension, 1 to
    ``AF_MAX_SERIES_QUANTILE_LEVELS`` (16) of them, each in [0, 1]."""
    q = np.array(levels, dtype=np.float64)
    if q.ndim != 1 or q.shape[0] == 0:
        msg = f"series quantile levels must be a vector of at least one level, not of shape {q.shape}"
        raise ValueError(msg)
    if q.shape[0] > _abi.MAX_SERIES_QUANTILE_LEVELS:
        msg = f"at most {_abi.MAX_SERIES_QUANTILE_LEVELS} series quantile levels a call, not {q.shape[0]}"
        raise ValueError(msg)
    if not ((q >= 0.0) & (q <= 1.0)).all():
        msg = "quantile levels must lie in [0, 1]"
        raise ValueError(msg)
    return q


def _check_series_columns(columns: Any, n_series: int) -> np.ndarray:
    """``columns`` (None: every series) as series indices, or ValueError: one dimension, at least one, each < n_series."""
    if columns is None:
        return np.arange(n_series, dtype=np.int64)
    raw = np.asarray(columns)
    if raw.ndim != 1 or raw.shape[0] == 0 or raw.dtype.kind not in "iu":
        msg = f"series columns must be a non-empty vector of series indices, not {columns!r}"
        raise ValueError(msg)
    col = raw.astype(np.int64)
    if (col < 0).any() or (col >= n_series).any():
        msg = f"series columns must lie in [0, {n_series})"
        raise ValueError(msg)
    return col


def series_window_quantiles(samples: np.ndarray, tick_edges: Any, n_edges: int, levels: Any,
                            columns: Any = None) -> tuple[np.ndarray, np.ndarray]:
    """Exact quantiles per window of ticks of ONE scenario's sampled series ``samples`` (uint32 words [n_series, ticks]):
    ``(count`` int64 [W], ``quantiles`` float64 [W, C, Q]``)``, the windows :func:`series_window_stats`'s.  Every word has
    a 32-bit key: of an integer series the word itself; of a ``ram_in_use`` column the float32 bits ``w`` mapped to ``~w``
    where the sign bit is set, else ``w | 0x80000000`` -- the IEEE total order on non-NaN floats, -0.0 below +0.0.  A
    window's column is sorted BY KEY; ``x[0 .. n-1]`` are the values in that order as float64 (the word, or the float32
    value).  For a level ``q``: ``v = (n - 1) * q``, ``lo = floor(v)``, ``hi = min(lo + 1, n - 1)``, ``t = v - lo``,
    ``d = x[hi] - x[lo]``, and ``x[hi] - d * (1 - t)`` where ``t >= 0.5``, else ``x[lo] + d * t``: ``np.quantile(values,
    levels)`` bit for bit where the window holds no zero, equal under ``==`` everywhere.  An empty window: count 0, NaN.
    Output column ``c`` belongs to ``columns[c]`` (series indices in any order, duplicates allowed; None: every series).
    The definition the device analyzer (``af_engine_summarize_series_quantiles``) is bit-equal to."""
    b = check_tick_edges(tick_edges)
    q = check_series_levels(levels)
    words = np.ascontiguousarray(samples).view(np.uint32)
    if words.ndim != 2:
        msg = f"samples must be words [n_series, ticks], not of shape {words.shape}"
        raise ValueError(msg)
    n_series, ticks = words.shape
    col = _check_series_columns(columns, n_series)
    ram = ram_columns(n_series, n_edges)[col]
    n_win = b.shape[0] - 1
    r = np.minimum(b.astype(np.int64), ticks)
    count = np.diff(r)
    quant = np.full((n_win, col.shape[0], q.shape[0]), np.nan)
    for w in range(n_win):
        n = int(count[w])
        if n == 0:
            continue
        seg = words[col, r[w]:r[w + 1]]
        key = np.sort(np.where(ram[:, None], np.where(seg >> 31 != 0, ~seg, seg | np.uint32(0x80000000)), seg), axis=1)
        back = np.where(key >> 31 != 0, key & np.uint32(0x7FFFFFFF), ~key)
        with np.errstate(invalid="ignore"):   # (an integer word read as float32 may be a NaN: not taken)
            x = np.where(ram[:, None], back.view(np.float32).astype(np.float64), key.astype(np.float64))
        v = np.float64(n - 1) * q
        f = np.floor(v)
        lo = f.astype(np.int64)
        hi = np.minimum(lo + 1, n - 1)
        t = v - f
        lo_v, hi_v = x[:, lo], x[:, hi]
        d = hi_v - lo_v
        quant[w] = np.where(t >= 0.5, hi_v - d * (1.0 - t), lo_v + d * t)
    return count, quant


def check_series_bins(bins: Any, n_columns: int, lo: Any = None, width: Any = None) -> tuple[int, np.ndarray, np.ndarray]:
    """The binning of a series-histogram call as ``(n_bins, lo, width)``, ``lo`` and ``width`` float64 [n_columns], or
    ValueError: ``bins`` a whole number from 1 to ``AF_MAX_SERIES_HISTOGRAM_BINS`` (1 024); ``lo`` / ``width`` None (0.0 /
    1.0 each), a scalar or one value per output column; every ``lo`` finite, every ``width`` finite and above 0."""
    if isinstance(bins, (bool, np.bool_)) or not isinstance(bins, (int, np.integer)):
        msg = f"bins must be a whole number, not {bins!r}"
        raise ValueError(msg)
    n_bins = int(bins)
    if not 1 <= n_bins <= _abi.MAX_SERIES_HISTOGRAM_BINS:
        msg = f"bins must be 1 .. {_abi.MAX_SERIES_HISTOGRAM_BINS}, not {n_bins}"
        raise ValueError(msg)
    out = []
    for name, value, default in (("lo", lo, 0.0), ("width", width, 1.0)):
        v = np.full(n_columns, default) if value is None else np.array(value, dtype=np.float64)
        if v.ndim == 0:
            v = np.full(n_columns, float(v))
        if v.shape != (n_columns,):
            msg = f"{name} must be a scalar or one value per output column ({n_columns}), not of shape {v.shape}"
            raise ValueError(msg)
        if not np.isfinite(v).all():
            msg = f"{name} must be finite"
            raise ValueError(msg)
        out.append(np.ascontiguousarray(v))
    if not (out[1] > 0.0).all():
        msg = "width must be above 0"
        raise ValueError(msg)
    return n_bins, out[0], out[1]


def series_window_histogram(samples: np.ndarray, tick_edges: Any, n_edges: int, bins: int, columns: Any = None,
                            lo: Any = None, width: Any = None) -> dict[str, np.ndarray]:
    """Occupancy histograms per window of ticks of ONE scenario's sampled series ``samples`` (uint32 words [n_series,
    ticks]), the windows :func:`series_window_stats`'s.  Output column ``c`` reads series ``columns[c]`` (any order,
    duplicates allowed; None: every series) with its own binning ``lo[c]``, ``width[c]`` (:func:`check_series_bins`).  A
    value ``x`` -- the word of an integer series, the float32 value of a ``ram_in_use`` column, as float64 -- goes to
    ``under`` where ``x < lo`` (-0.0 is not below 0.0); otherwise ``t = (x - lo) / width`` in float64, to ``over`` where
    ``t >= bins``, else to bin ``floor(t)``.  Returns int64 arrays: ``count`` [W] (the ticks of the window), ``hist``
    [W, C, bins], ``under`` and ``over`` [W, C], with ``under + hist.sum(-1) + over == count``; and ``bin_edges`` float64
    [C, bins + 1] (``lo + k * width``) and ``ram`` bool [C] (the ``ram_in_use`` columns).  The definition the device analyzer
    (``af_engine_summarize_series_histogram``) equals word for word."""
    b = check_tick_edges(tick_edges)
    words = np.ascontiguousarray(samples).view(np.uint32)
    if words.ndim != 2:
        msg = f"samples must be words [n_series, ticks], not of shape {words.shape}"
        raise ValueError(msg)
    n_series, ticks = words.shape
    col = _check_series_columns(columns, n_series)
    n_col = int(col.shape[0])
    n_bins, lo_v, width_v = check_series_bins(bins, n_col, lo, width)
    ram = ram_columns(n_series, n_edges)[col]
    n_win = b.shape[0] - 1
    r = np.minimum(b.astype(np.int64), ticks)
    live = words[col, r[0]:r[-1]]                         # the rows inside the windows
    with np.errstate(invalid="ignore"):                   # (an integer word read as float32 may be a NaN: not taken)
        x = np.where(ram[:, None], live.view(np.float32).astype(np.float64), live.astype(np.float64))
        below = x < lo_v[:, None]
        t = (x - lo_v[:, None]) / width_v[:, None]
        above = ~below & (t >= float(n_bins))
        # the entry of a value among the bins + 2 words of its column: its bin, then under, then over
        entry = np.where(below, n_bins, np.where(above, n_bins + 1, np.where(below | above | np.isnan(t), 0.0, t).astype(np.int64)))
    win = np.searchsorted(r, np.arange(r[0], r[-1]), side="right") - 1     # (the last window that starts at or before the row)
    flat = (win[None, :] * n_col + np.arange(n_col)[:, None]) * (n_bins + 2) + entry
    table = np.bincount(flat.ravel(), minlength=n_win * n_col * (n_bins + 2)).reshape(n_win, n_col, n_bins + 2)
    hist, under, over = (np.ascontiguousarray(v) for v in (table[:, :, :n_bins], table[:, :, n_bins], table[:, :, n_bins + 1]))
    return {"count": np.diff(r), "hist": hist, "under": under, "over": over,
            "bin_edges": lo_v[:, None] + np.arange(n_bins + 1, dtype=np.float64)[None, :] * width_v[:, None], "ram": ram}


def check_state_bins(bins: Any, lo: Any = 0.0, width: Any = 1.0, sample_period: Any = None) -> tuple[int, float, float, float | None]:
    """The binning of a latency-by-state call as ``(n_bins, lo, width, sample_period)``, or ValueError: ``bins`` a whole number
    above 0, ``lo`` finite, ``width`` finite and above 0, ``sample_period`` (unless None) finite and above 0."""
    if isinstance(bins, (bool, np.bool_)) or not isinstance(bins, (int, np.integer)) or int(bins) < 1:
        msg = f"bins must be a whole number above 0, not {bins!r}"
        raise ValueError(msg)
    try:
        lo_f, width_f = float(lo), float(width)
        period_f = None if sample_period is None else float(sample_period)
    except (TypeError, ValueError):
        msg = f"lo, width and sample_period must be numbers, not {lo!r}, {width!r}, {sample_period!r}"
        raise ValueError(msg) from None
    if not np.isfinite(lo_f):
        msg = f"lo must be finite, not {lo!r}"
        raise ValueError(msg)
    if not (np.isfinite(width_f) and width_f > 0.0):
        msg = f"width must be finite and above 0, not {width!r}"
        raise ValueError(msg)
    if period_f is not None and not (np.isfinite(period_f) and period_f > 0.0):
        msg = f"sample_period must be finite and above 0, not {sample_period!r}"
        raise ValueError(msg)
    return int(bins), lo_f, width_f, period_f


def latency_state_cells(clock: np.ndarray, samples: np.ndarray, n_edges: int, sample_period: float, column: int, bins: int,
                        lo: float = 0.0, width: float = 1.0, edges: Any = None) -> list[np.ndarray]:
    """Per cell (arrival window w, bin b), at index ``w * bins + b``, the latencies of ONE scenario's rows ``clock`` [m, 2] that
    belong to it, in row order: the latency of a request by the STATE it met on arrival.  ``samples``: the scenario's sampled
    series as uint32 words [n_series, ticks]; ``column``: the series; ``n_edges``: the plan's (the ``ram_in_use`` columns are
    float32 words, :func:`ram_columns`).  For a row with ``start = clock[i, 0]``:

    * tick: ``q = floor(start / sample_period)`` in float64, ``k = q - 1``.  Sample ``k`` is taken at ``(k + 1) *
      sample_period`` (the collector samples after its timeout), so ``k`` is the last sample taken at or before the arrival
      AS THE FLOAT64 QUOTIENT SEES IT.  No state, no cell: ``q < 1`` (no sample yet), ``k >= ticks``, ``start`` NaN or negative.
    * value: ``x`` = the word as float64 (the float32 value of a ``ram_in_use`` column), as :func:`series_window_histogram`.
    * bin: ``x < lo``: no cell (-0.0 is not below 0.0); ``t = (x - lo) / width`` in float64; ``t >= bins``: the LAST bin (it
      takes the overflow: "queue >= k" is a condition); otherwise bin ``floor(t)``.
    * window: with ``edges`` the rule of ``window_of="arrival"``, ``edges[w] < start <= edges[w + 1]``, else no cell; with
      ``edges=None`` one window with no condition on time.

    The cohorts are right-censored like the arrival windows': a request that had not completed when the run ended, or was
    dropped, is in no row.  The definition the device analyzers (``af_engine_summarize_state_windows`` /
    ``af_engine_summarize_state_quantiles``) equal word for word."""
    n_bins, lo_f, width_f, period = check_state_bins(bins, lo, width, sample_period)
    ck = np.asarray(clock, dtype=np.float64).reshape(-1, 2)
    words = np.ascontiguousarray(samples).view(np.uint32)
    if words.ndim != 2:
        msg = f"samples must be words [n_series, ticks], not of shape {words.shape}"
        raise ValueError(msg)
    n_series, ticks = words.shape
    col = int(_check_series_columns([column], n_series)[0])
    e = None if edges is None else check_edges(edges)
    n_win = 1 if e is None else e.shape[0] - 1
    start = ck[:, 0]
    with np.errstate(invalid="ignore", over="ignore"):
        lat = ck[:, 1] - start
        q = np.floor(start / period)
        ok = (start >= 0.0) & (q >= 1.0) & (q - 1.0 < float(ticks))
        k = np.where(ok, q - 1.0, 0.0).astype(np.int64)
        word = words[col, k] if ticks else np.zeros(k.shape, dtype=np.uint32)
        x = word.view(np.float32).astype(np.float64) if ram_columns(n_series, n_edges)[col] else word.astype(np.float64)
        ok &= x >= lo_f                                          # (a NaN, which no series holds: no cell)
        t = (x - lo_f) / width_f
        b = np.where(t >= float(n_bins), float(n_bins - 1), np.where(ok, t, 0.0)).astype(np.int64)
    w = np.zeros(start.shape, dtype=np.int64)
    if e is not None:
        eb = np.searchsorted(e, start, side="left")              # #{edges < start}: window eb - 1 where 1 <= eb <= W
        ok &= (eb >= 1) & (eb <= n_win)
        w = eb - 1
    key = np.where(ok, w * n_bins + b, n_win * n_bins)           # (rows without a cell: past the last key)
    order = np.argsort(key, kind="stable")                       # (stable: a cell's rows stay in row order)
    r = np.searchsorted(key[order], np.arange(n_win * n_bins + 1), side="left")
    return [lat[order[r[c]:r[c + 1]]] for c in range(n_win * n_bins)]


def latency_state_stats(clock: np.ndarray, samples: np.ndarray, n_edges: int, sample_period: float, column: int, bins: int,
                        lo: float = 0.0, width: float = 1.0, edges: Any = None) -> np.ndarray:
    """The eight latency statistics of every cell of :func:`latency_state_cells`: float64 [W', bins, 8] in LATENCY_KEYS order
    (W' = 1 without ``edges``; an empty cell: total 0, the rest NaN)."""
    cells = latency_state_cells(clock, samples, n_edges, sample_period, column, bins, lo, width, edges)
    return np.stack([latency_stats_row(x) for x in cells]).reshape(-1, int(bins), 8)


def latency_state_quantiles(clock: np.ndarray, samples: np.ndarray, n_edges: int, sample_period: float, column: int, bins: int,
                            levels: Any, thresholds: Any = None, lo: float = 0.0, width: float = 1.0,
                            edges: Any = None) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Quantiles and SLO counts of every cell of :func:`latency_state_cells`: ``(count`` uint32 [W', bins], ``quantiles``
    float64 [W', bins, Q], ``within`` uint32 [W', bins, T]``)`` as :func:`latency_window_quantiles` gives them per window."""
    q, th = check_levels(levels), check_slo_thresholds(thresholds)
    cells = latency_state_cells(clock, samples, n_edges, sample_period, column, bins, lo, width, edges)
    n_bins = int(bins)
    count = np.array([x.shape[0] for x in cells], dtype=np.uint32).reshape(-1, n_bins)
    quant = np.stack([latency_quantiles(x, q) for x in cells]).reshape(-1, n_bins, q.shape[0])
    within = np.stack([latency_within(x, th) for x in cells]).reshape(-1, n_bins, th.shape[0])
    return count, quant, within


def series_names_of(plan: DevicePlan) -> list[str]:
    """Names of the sampled series of a plan in device order: edges, then ready/io/ram per server."""
    names = [f"{e}:edge_concurrent_connection" for e in plan.edge_ids]
    for sid in plan.server_ids:
        names += [f"{sid}:ready_queue_len", f"{sid}:event_loop_io_sleep", f"{sid}:ram_in_use"]
    return names


def _state_series(series: Any, names: list[str]) -> int:
    """ONE series, a name of ``names`` or an index, as its index."""
    if isinstance(series, (str, bytes)):
        series = series.decode() if isinstance(series, bytes) else series
        if series not in names:
            msg = f"unknown series {series!r} (series_names(): {names})"
            raise ValueError(msg)
        return names.index(series)
    if isinstance(series, (bool, np.bool_)) or not isinstance(series, (int, np.integer)):
        msg = f"series must be one name of series_names() or one index, not {series!r}"
        raise ValueError(msg)
    return int(_check_series_columns([int(series)], len(names))[0])


def series_histogram_quantiles(summary: dict[str, Any], levels: Any) -> np.ndarray:
    """Quantiles ``levels`` (any number of them, each in [0, 1]) read off a series histogram ``summary`` -- what
    :func:`series_window_histogram`, :meth:`ScenarioResults.get_series_histogram` or
    :meth:`BatchedResults.series_histogram_summary` returned --: float64 [..., C, Q] on the host.  For integer series binned
    with a whole ``lo`` and ``width == 1`` bin ``k`` holds the value ``lo + k`` alone, so the sorted sample is known from the
    cumulative counts wherever it lies inside the bins, and the quantile is ``np.quantile``'s 'linear' value by the formula
    of :func:`series_window_quantiles` (``v = (n - 1) * q``, ``t = v - floor(v)``, ``x[hi] - d * (1 - t)`` where ``t >=
    0.5``, else ``x[lo] + d * t``): bit-equal to it.  NaN where a rank the level needs (``floor(v)``, and the next one
    where ``t > 0``) lies in ``under`` / ``over``, and in an empty cell.  ValueError for any other binning and for a
    ``ram_in_use`` column."""
    q = np.array(levels, dtype=np.float64)
    if q.ndim != 1 or q.shape[0] == 0 or not ((q >= 0.0) & (q <= 1.0)).all():
        msg = "quantile levels must be a vector of at least one level in [0, 1]"
        raise ValueError(msg)

    def host(x: Any) -> np.ndarray:
        return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)

    hist, under, count = host(summary["hist"]).astype(np.int64), host(summary["under"]).astype(np.int64), host(summary["count"]).astype(np.int64)
    edges = np.asarray(summary["bin_edges"], dtype=np.float64)
    if np.asarray(summary["ram"]).any():
        msg = "quantiles from a histogram need integer series: a ram_in_use column is selected"
        raise ValueError(msg)
    lo_v = edges[:, 0]
    if not ((lo_v == np.floor(lo_v)).all() and (np.diff(edges, axis=1) == 1.0).all()):
        msg = "quantiles from a histogram need a whole lo and width == 1 for every column"
        raise ValueError(msg)
    cum = np.cumsum(hist, axis=-1)                       # [..., C, B]
    n = np.broadcast_to(count[..., None], under.shape)   # [..., C]
    out = np.full(under.shape + (q.shape[0],), np.nan)

    def value(rank: np.ndarray) -> np.ndarray:           # the rank-th smallest value, NaN outside the bins
        k = rank - under
        ok = (n > 0) & (k >= 0) & (k < cum[..., -1])
        idx = (cum <= k[..., None]).sum(axis=-1)
        return np.where(ok, lo_v + idx.astype(np.float64), np.nan)

    for i, level in enumerate(q):
        v = (n - 1).astype(np.float64) * level
        f = np.floor(v)
        t = v - f
        lo_r = f.astype(np.int64)
        hi_r = np.where(t > 0.0, np.minimum(lo_r + 1, n - 1), lo_r)
        lo_x, hi_x = value(lo_r), value(hi_r)
        d = hi_x - lo_x
        out[..., i] = np.where(t >= 0.5, hi_x - d * (1.0 - t), lo_x + d * t)
    return out


COMBINE_OPS = ("sum", "min", "max", "spread")


def check_series_combinations(combos: Any, names: list[str], n_edges: int) -> tuple[list[str], list[str], list[np.ndarray]]:
    """The combinations of a series-combined call as ``(labels, ops, columns)``: ``combos`` is ``{label: (op, selection)}``
    (or an iterable of ``(label, (op, selection))`` pairs), ``op`` one of ``"sum"``, ``"min"``, ``"max"``, ``"spread"`` and
    ``selection`` a list of series names of ``names`` or of indices, ONE ``fnmatch`` pattern over ``names`` (such as
    ``"*:ready_queue_len"``) or a list of such patterns.  ``columns[c]`` is the selection as strictly increasing int64
    series indices.  ValueError for no combination or more than ``AF_MAX_SERIES_COMBINATIONS`` (64), an unknown op, a
    duplicate label, a selection that matches no series, names a series twice or is out of range, and one that mixes
    ``ram_in_use`` columns with integer series."""
    import fnmatch

    items = list(combos.items()) if isinstance(combos, dict) else [(k, v) for k, v in combos]
    if not 1 <= len(items) <= _abi.MAX_SERIES_COMBINATIONS:
        msg = f"a call takes 1 .. {_abi.MAX_SERIES_COMBINATIONS} combinations, not {len(items)}"
        raise ValueError(msg)
    ram = ram_columns(len(names), n_edges)
    labels: list[str] = []
    ops: list[str] = []
    columns: list[np.ndarray] = []
    for label, spec in items:
        label = str(label)
        if label in labels:
            msg = f"combination {label!r} is given twice"
            raise ValueError(msg)
        if not isinstance(spec, (tuple, list)) or len(spec) != 2:
            msg = f"combination {label!r} must be (op, selection), not {spec!r}"
            raise ValueError(msg)
        op, selection = spec
        if op not in COMBINE_OPS:
            msg = f"combination {label!r}: unknown op {op!r} (one of {COMBINE_OPS})"
            raise ValueError(msg)
        sel = [selection] if isinstance(selection, (str, bytes)) else list(np.asarray(selection).tolist() if isinstance(selection, np.ndarray) else selection)
        picked: list[int] = []
        patterns = False
        for x in sel:
            x = x.decode() if isinstance(x, bytes) else x
            if isinstance(x, str) and any(ch in x for ch in "*?["):
                hit = [j for j, nm in enumerate(names) if fnmatch.fnmatchcase(nm, x)]
                if not hit:
                    msg = f"combination {label!r}: pattern {x!r} matches no series (series_names(): {names})"
                    raise ValueError(msg)
                patterns = True
                picked += hit
            elif isinstance(x, str):
                if x not in names:
                    msg = f"combination {label!r}: unknown series {x!r} (series_names(): {names})"
                    raise ValueError(msg)
                picked.append(names.index(x))
            elif isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)) or not 0 <= int(x) < len(names):
                msg = f"combination {label!r}: {x!r} is no series name, pattern or index below {len(names)}"
                raise ValueError(msg)
            else:
                picked.append(int(x))
        if patterns:
            picked = sorted(set(picked))                 # (two patterns may match one series: their union)
        if not picked:
            msg = f"combination {label!r} selects no series"
            raise ValueError(msg)
        if len(set(picked)) != len(picked):
            msg = f"combination {label!r} names a series twice"
            raise ValueError(msg)
        col = np.array(sorted(picked), dtype=np.int64)
        if ram[col].any() and not ram[col].all():
            msg = f"combination {label!r} mixes ram_in_use columns with integer series"
            raise ValueError(msg)
        labels.append(label)
        ops.append(op)
        columns.append(col)
    return labels, ops, columns


def _double_keys(x: np.ndarray) -> np.ndarray:
    """uint64 keys that order like the float64 values ``x`` (no NaN) with -0.0 below +0.0: the IEEE total order."""
    bits = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(bits >> np.uint64(63) != 0, ~bits, bits | np.uint64(1 << 63))


def _combination_columns(op: str, columns: Any, n_series: int, n_edges: int) -> tuple[np.ndarray, bool]:
    if op not in COMBINE_OPS:
        msg = f"unknown op {op!r} (one of {COMBINE_OPS})"
        raise ValueError(msg)
    col = np.asarray(columns)
    if col.ndim != 1 or col.shape[0] == 0 or col.dtype.kind not in "iu":
        msg = "the columns of a combination must be a non-empty vector of series indices"
        raise ValueError(msg)
    col = col.astype(np.int64)
    if col[0] < 0 or col[-1] >= n_series or not (np.diff(col) > 0).all():
        msg = f"the columns of a combination must be strictly increasing series indices below {n_series}"
        raise ValueError(msg)
    ram = ram_columns(n_series, n_edges)[col]
    if ram.any() and not ram.all():
        msg = "a combination mixes ram_in_use columns with integer series"
        raise ValueError(msg)
    return col, bool(ram.all())


def series_combined_values(samples: np.ndarray, n_edges: int, op: str, columns: Any) -> np.ndarray:
    """The per-tick values of ONE combination ``(op, columns)`` across the sampled series of ONE scenario (``samples``:
    uint32 words [n_series, ticks]): ``columns`` strictly increasing series indices, all integer series or all
    ``ram_in_use`` columns.  Integer columns: the words as unsigned 32-bit integers, ``sum`` their exact sum, ``min`` /
    ``max`` the smallest / largest word, ``spread`` their difference, as uint64 [ticks].  ``ram_in_use`` columns: every word
    as the float64 of its float32 value; ``sum`` is added in ascending series index, left to right from the first column's
    value, one rounding per addition (an explicit loop); ``min`` / ``max`` follow the IEEE total order (-0.0 below +0.0);
    ``spread`` is ``max - min`` as one float64 subtraction; float64 [ticks]."""
    words = np.ascontiguousarray(samples).view(np.uint32)
    if words.ndim != 2:
        msg = f"samples must be words [n_series, ticks], not of shape {words.shape}"
        raise ValueError(msg)
    col, is_ram = _combination_columns(op, columns, words.shape[0], n_edges)
    if not is_ram:
        w = words[col].astype(np.uint64)
        if op == "sum":
            acc = np.zeros(words.shape[1], dtype=np.uint64)
            for row in w:
                acc = acc + row                           # (at most 2^32 columns below 2^32: no wrap)
            return acc
        return w.min(axis=0) if op == "min" else w.max(axis=0) if op == "max" else w.max(axis=0) - w.min(axis=0)
    x = words[col].view(np.float32).astype(np.float64)
    if op == "sum":
        acc = x[0].copy()
        for row in x[1:]:                                 # (left to right: np.sum's order is not fixed)
            acc = acc + row
        return acc
    keys = _double_keys(x)
    tick = np.arange(x.shape[1])
    mn, mx = x[np.argmin(keys, axis=0), tick], x[np.argmax(keys, axis=0), tick]
    return mn if op == "min" else mx if op == "max" else mx - mn


def series_combined_window_stats(samples: np.ndarray, tick_edges: Any, n_edges: int, combos: Any, thresholds: Any = None,
                                 bins: int = 0, lo: Any = None, width: Any = None) -> dict[str, np.ndarray]:
    """Statistics per window of ticks of combinations ACROSS the sampled series of ONE scenario (``samples``: uint32 words
    [n_series, ticks]); the windows are :func:`series_window_stats`'s.  ``combos`` is a sequence of ``(op, columns)`` pairs
    (:func:`check_series_combinations` makes them); ``v`` = :func:`series_combined_values` per tick and ``x`` = ``v`` as
    float64.  Returns ``count`` int64 [W]; ``mean`` float64 [W, C] -- an integer combination: the exact integer sum of
    ``v`` over the window, ``float(S) / float(count)``; a ``ram_in_use`` one: ``math.fsum(v) / count`` --; ``min`` / ``max``
    float64 [W, C], the smallest / largest ``x`` in the IEEE total order (-0.0 below +0.0); ``above`` int64 [W, C], the
    ticks with ``x > thresholds[c]`` (None: 0.0 each).  An empty window has NaN in the three float outputs and 0 in
    ``above``.  With ``bins`` above 0 also ``hist`` int64 [W, C, bins], ``under``, ``over`` [W, C] by the rule of
    :func:`series_window_histogram` on ``x`` with ``lo[c]``, ``width[c]`` (:func:`check_series_bins`), ``bin_edges``
    float64 [C, bins + 1] and ``ram`` bool [C], so :func:`series_histogram_quantiles` reads exact quantiles of an integer
    combination off the result.  The definition the device analyzer (``af_engine_summarize_series_combined``) matches:
    bit for bit, but for the ``mean`` of a ``ram_in_use`` combination whose partial sums are not exact, which lies within
    ``(count - 1) * 2^-53`` relative of it."""
    import math

    b = check_tick_edges(tick_edges)
    words = np.ascontiguousarray(samples).view(np.uint32)
    if words.ndim != 2:
        msg = f"samples must be words [n_series, ticks], not of shape {words.shape}"
        raise ValueError(msg)
    n_series, ticks = words.shape
    pairs = [(op, _combination_columns(op, col, n_series, n_edges)) for op, col in combos]
    n_c = len(pairs)
    if not 1 <= n_c <= _abi.MAX_SERIES_COMBINATIONS:
        msg = f"a call takes 1 .. {_abi.MAX_SERIES_COMBINATIONS} combinations, not {n_c}"
        raise ValueError(msg)
    thr = np.zeros(n_c) if thresholds is None else np.asarray(thresholds, dtype=np.float64)
    if thr.shape != (n_c,) or np.isnan(thr).any():
        msg = f"thresholds must be {n_c} values, none of them NaN"
        raise ValueError(msg)
    n_bins = 0
    if bins or lo is not None or width is not None:
        n_bins, lo_v, width_v = check_series_bins(bins, n_c, lo, width)
    n_win = b.shape[0] - 1
    r = np.minimum(b.astype(np.int64), ticks)
    count = np.diff(r)
    mean, mn, mx = (np.full((n_win, n_c), np.nan) for _ in range(3))
    above = np.zeros((n_win, n_c), dtype=np.int64)
    hist = np.zeros((n_win, n_c, n_bins), dtype=np.int64)
    under, over = (np.zeros((n_win, n_c), dtype=np.int64) for _ in range(2))
    for c, (op, (col, is_ram)) in enumerate(pairs):
        v = series_combined_values(words, n_edges, op, col)
        x = v.astype(np.float64)
        keys = _double_keys(x)
        for w in range(n_win):
            if count[w] == 0:
                continue
            seg, xs, ks = v[r[w]:r[w + 1]], x[r[w]:r[w + 1]], keys[r[w]:r[w + 1]]
            total = 0.0 + math.fsum(seg.tolist()) if is_ram else float(sum(int(t) for t in seg.tolist()))
            mean[w, c] = total / float(count[w])
            mn[w, c], mx[w, c] = xs[np.argmin(ks)], xs[np.argmax(ks)]
            above[w, c] = int((xs > thr[c]).sum())
            if n_bins:
                below = xs < lo_v[c]
                t = (xs - lo_v[c]) / width_v[c]
                past = ~below & (t >= float(n_bins))
                inside = ~below & ~past
                under[w, c], over[w, c] = int(below.sum()), int(past.sum())
                hist[w, c] = np.bincount(t[inside].astype(np.int64), minlength=n_bins)
    out = {"count": count, "mean": mean, "min": mn, "max": mx, "above": above}
    if n_bins:
        out.update(hist=hist, under=under, over=over, ram=np.array([p[1][1] for p in pairs], dtype=bool),
                   bin_edges=lo_v[:, None] + np.arange(n_bins + 1, dtype=np.float64)[None, :] * width_v[:, None])
    return out


JOINT_SUMS = ("sx", "sy", "sxx", "syy", "sxy")
JOINT_STATISTICS = ("mean_x", "mean_y", "cov", "corr", "var_x", "var_y")


def _select_series(selection: Any, names: list[str], what: str) -> list[int]:
    """``selection`` -- a series name, an index, an ``fnmatch`` pattern over ``names`` or a list of those -- as series
    indices in the order given (a pattern: its matches ascending), every series once."""
    import fnmatch

    sel = [selection] if isinstance(selection, (str, bytes, int, np.integer)) else list(np.asarray(selection).tolist() if isinstance(selection, np.ndarray) else selection)
    picked: list[int] = []
    for x in sel:
        x = x.decode() if isinstance(x, bytes) else x
        if isinstance(x, str) and any(ch in x for ch in "*?["):
            hit = [j for j, nm in enumerate(names) if fnmatch.fnmatchcase(nm, x)]
            if not hit:
                msg = f"{what}: pattern {x!r} matches no series (series_names(): {names})"
                raise ValueError(msg)
            picked += [j for j in hit if j not in picked]
        elif isinstance(x, str):
            if x not in names:
                msg = f"{what}: unknown series {x!r} (series_names(): {names})"
                raise ValueError(msg)
            picked.append(names.index(x))
        elif isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)) or not 0 <= int(x) < len(names):
            msg = f"{what}: {x!r} is no series name, pattern or index below {len(names)}"
            raise ValueError(msg)
        else:
            picked.append(int(x))
    if not picked:
        msg = f"{what} selects no series"
        raise ValueError(msg)
    if len(set(picked)) != len(picked):
        msg = f"{what} names a series twice"
        raise ValueError(msg)
    return picked


def check_series_pairs(pairs: Any, names: list[str], n_edges: int) -> tuple[list[str], np.ndarray, np.ndarray, np.ndarray]:
    """The pairs of a series-joint call as ``(labels, a, b, lag)``: ``pairs`` is ``{label: (a, b)}`` or ``{label: (a, b,
    lag)}`` (or an iterable of ``(label, spec)``), ``a`` and ``b`` series names of ``names`` or indices, ``lag`` a whole number
    of ticks (default 0): the pair's samples are ``(a at tick k, b at tick k + lag)``.  ``a``, ``b`` and ``lag`` come back as
    int64 vectors.  ValueError for everything ``af_engine_summarize_series_joint`` refuses in a pair -- no pair or more than
    ``AF_MAX_SERIES_PAIRS`` (64), a series that is unknown or out of range, a ``ram_in_use`` column (integer series only in
    this version), a lag that is negative, not whole or not below 2^31 -- and for a duplicate label."""
    items = list(pairs.items()) if isinstance(pairs, dict) else [(k, v) for k, v in pairs]
    if not 1 <= len(items) <= _abi.MAX_SERIES_PAIRS:
        msg = f"a call takes 1 .. {_abi.MAX_SERIES_PAIRS} pairs, not {len(items)}"
        raise ValueError(msg)
    ram = ram_columns(len(names), n_edges)
    labels: list[str] = []
    cols: list[tuple[int, int, int]] = []
    for label, spec in items:
        label = str(label)
        if label in labels:
            msg = f"pair {label!r} is given twice"
            raise ValueError(msg)
        if not isinstance(spec, (tuple, list)) or len(spec) not in (2, 3):
            msg = f"pair {label!r} must be (a, b) or (a, b, lag), not {spec!r}"
            raise ValueError(msg)
        ab = []
        for x in spec[:2]:
            x = x.decode() if isinstance(x, bytes) else x
            if isinstance(x, str):
                if x not in names:
                    msg = f"pair {label!r}: unknown series {x!r} (series_names(): {names})"
                    raise ValueError(msg)
                j = names.index(x)
            elif isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)) or not 0 <= int(x) < len(names):
                msg = f"pair {label!r}: {x!r} is no series name or index below {len(names)}"
                raise ValueError(msg)
            else:
                j = int(x)
            if ram[j]:
                msg = f"pair {label!r}: {names[j]!r} is a ram_in_use column; pairs take integer series only"
                raise ValueError(msg)
            ab.append(j)
        lag = spec[2] if len(spec) == 3 else 0
        if isinstance(lag, (bool, np.bool_)) or not isinstance(lag, (int, np.integer)) or not 0 <= int(lag) < 2 ** 31:
            msg = f"pair {label!r}: the lag must be a whole number of ticks in [0, 2^31), not {lag!r}"
            raise ValueError(msg)
        labels.append(label)
        cols.append((ab[0], ab[1], int(lag)))
    arr = np.array(cols, dtype=np.int64)
    return labels, arr[:, 0].copy(), arr[:, 1].copy(), arr[:, 2].copy()


def _check_pair_columns(pairs: Any, n_series: int, n_edges: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    a, b, lag = (np.asarray(v) for v in pairs)
    if not (a.ndim == b.ndim == lag.ndim == 1 and a.shape == b.shape == lag.shape and 1 <= a.shape[0] <= _abi.MAX_SERIES_PAIRS):
        msg = f"pairs must be (a, b, lag), three vectors of 1 .. {_abi.MAX_SERIES_PAIRS} entries"
        raise ValueError(msg)
    if any(v.dtype.kind not in "iu" for v in (a, b, lag)):
        msg = "the series indices and the lags of the pairs must be integers"
        raise ValueError(msg)
    a, b, lag = a.astype(np.int64), b.astype(np.int64), lag.astype(np.int64)
    ram = ram_columns(n_series, n_edges)
    for col in (a, b):
        if (col < 0).any() or (col >= n_series).any():
            msg = f"the series of a pair must be indices below {n_series}"
            raise ValueError(msg)
        if ram[col].any():
            msg = "a pair names a ram_in_use column; pairs take integer series only"
            raise ValueError(msg)
    if (lag < 0).any() or (lag >= 2 ** 31).any():
        msg = "the lag of a pair must be in [0, 2^31)"
        raise ValueError(msg)
    return a, b, lag


def series_joint_sums(samples: np.ndarray, tick_edges: Any, n_edges: int, pairs: Any) -> dict[str, np.ndarray]:
    """The six sums of pairs of series per window of ticks of ONE scenario's sampled series ``samples`` (uint32 words
    [n_series, ticks]); ``pairs`` is ``(a, b, lag)``, three integer vectors (:func:`check_series_pairs` makes them).  Window
    ``w`` holds the rows ``[r0, r1) = [min(b[w], ticks), min(b[w + 1], ticks))`` of ``b = tick_edges``; the samples of pair
    ``p`` in it are ``(x, y) = (samples[a[p], k], samples[b[p], k + lag[p]])`` for ``k`` in ``[r0, r1 - lag[p])``, the words as
    unsigned integers: both ticks inside the window.  Returns ``n`` int64 [W, P] and ``sx``, ``sy``, ``sxx``, ``syy``,
    ``sxy`` as object arrays [W, P] of Python integers: sum x, sum y, sum x^2, sum y^2, sum x y, exact.  Pooling the members
    of a group is addition of these arrays.  The definition the device analyzer (``af_engine_summarize_series_joint``)
    matches word for word."""
    b = check_tick_edges(tick_edges)
    words = np.ascontiguousarray(samples).view(np.uint32)
    if words.ndim != 2:
        msg = f"samples must be words [n_series, ticks], not of shape {words.shape}"
        raise ValueError(msg)
    n_series, ticks = words.shape
    a, bb, lag = _check_pair_columns(pairs, n_series, n_edges)
    n_win, n_p = b.shape[0] - 1, a.shape[0]
    r = np.minimum(b.astype(np.int64), ticks)
    out: dict[str, np.ndarray] = {"n": np.zeros((n_win, n_p), dtype=np.int64)}
    for k in JOINT_SUMS:
        out[k] = np.zeros((n_win, n_p), dtype=object)
        out[k][...] = 0

    def before(v: np.ndarray) -> np.ndarray:     # before(v)[k] = v[0] + ... + v[k - 1]: fewer than 2^32 terms below 2^32, exact in uint64
        return np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(v, dtype=np.uint64)])

    low = np.uint64(0xFFFFFFFF)
    for p in range(n_p):
        step = int(lag[p])
        pairs_all = max(ticks - step, 0)         # the pairs (k, k + step) of the whole block: k < pairs_all
        x = words[a[p], :pairs_all].astype(np.uint64)
        y = words[bb[p], step:step + pairs_all].astype(np.uint64)
        cnt = np.maximum(r[1:] - r[:-1] - step, 0)
        k0 = np.where(cnt > 0, r[:-1], 0)        # window w holds the pairs k0[w] <= k < k0[w] + cnt[w]
        k1 = k0 + cnt
        out["n"][:, p] = cnt
        for key, v in (("sx", x), ("sy", y)):
            run = before(v)
            out[key][:, p] = (run[k1] - run[k0]).astype(object)
        for key, v in (("sxx", x * x), ("syy", y * y), ("sxy", x * y)):      # 128-bit sums, 32 bits of the products at a time
            top, bottom = before(v >> np.uint64(32)), before(v & low)
            out[key][:, p] = (top[k1] - top[k0]).astype(object) * (1 << 32) + (bottom[k1] - bottom[k0]).astype(object)
    return out


def _joint_integers(v: Any, shape: tuple[int, ...]) -> np.ndarray:
    """A sum of :func:`series_joint_sums` or of the device -- integers of ``shape``, or uint64 words ``shape + (2,)``, low
    word first -- as a flat object array of Python integers."""
    arr = np.asarray(v)
    if arr.shape == (*shape, 2) and arr.shape != shape:
        o = arr.astype(object)
        arr = o[..., 0] + o[..., 1] * (1 << 64)
    if arr.shape != shape:
        msg = f"a sum of shape {arr.shape} next to n of shape {shape}"
        raise ValueError(msg)
    out = np.empty(int(np.prod(shape, dtype=np.int64)), dtype=object)
    out[:] = [int(x) for x in arr.reshape(-1)]
    return out


def series_joint_statistics(sums: dict[str, Any], exact: bool = False) -> dict[str, np.ndarray]:
    """Means, covariance, variances and the Pearson correlation from the six sums ``n``, ``sx``, ``sy``, ``sxx``, ``syy``,
    ``sxy`` (arrays of one shape; a 128-bit sum may also be uint64 words ``[..., 2]``, low word first): the only place where
    floats appear.  With the exact integers ``N = n sxy - sx sy``, ``Dx = n sxx - sx^2``, ``Dy = n syy - sy^2``:

    * ``mean_x = sx / n``, ``mean_y = sy / n``, ``cov = N / n^2``, ``var_x = Dx / n^2``, ``var_y = Dy / n^2`` (the population
      moments): each the correctly rounded float64 of the exact rational (Python's ``int / int``);
    * ``corr = clamp(f(N) / sqrt(f(Dx) * f(Dy)), -1, 1)`` with ``f`` the correctly rounded conversion to float64 and every
      operation IEEE float64; NaN where ``Dx == 0`` or ``Dy == 0`` (a constant column).  A pair ``(a, a, 0)`` of a
      non-constant column has ``corr == 1.0`` exactly.

    Everything is NaN where ``n == 0``.  Returns float64 arrays of the sums' shape.  Cells whose six products ``n sxx``,
    ``n syy``, ``n sxy``, ``sx^2``, ``sy^2``, ``sx sy`` all stay below 2^63 take ``N``, ``Dx``, ``Dy`` in int64; of those, the
    ones with ``|N|``, ``Dx``, ``Dy`` < 2^53 and ``n^2`` < 2^53 divide in float64, and the means divide in float64 where the
    sum is below 2^53 -- the same bits as the definition, which ``exact=True`` applies to every cell."""
    n_in = np.asarray(sums["n"])
    shape = n_in.shape
    n_o = _joint_integers(n_in, shape)
    o = {k: _joint_integers(sums[k], shape) for k in JOINT_SUMS}
    cells = n_o.shape[0]
    out = {k: np.full(cells, np.nan) for k in JOINT_STATISTICS}
    done_mean = np.zeros(cells, dtype=bool)
    done_mom = np.zeros(cells, dtype=bool)
    done_corr = np.zeros(cells, dtype=bool)
    if not exact and cells:
        top = (1 << 63) - 1
        ok = (n_o > 0).astype(bool) & (n_o <= top).astype(bool)
        for k in JOINT_SUMS:
            ok &= (o[k] <= top).astype(bool)
        i = {k: np.where(ok, o[k], 0).astype(np.int64) for k in JOINT_SUMS}
        n = np.where(ok, n_o, 1).astype(np.int64)
        per_n = top // n
        ok &= (i["sxx"] <= per_n) & (i["syy"] <= per_n) & (i["sxy"] <= per_n)
        ok &= (i["sx"] <= top // np.maximum(i["sx"], 1)) & (i["sy"] <= top // np.maximum(i["sy"], 1)) & (i["sy"] <= top // np.maximum(i["sx"], 1))
        for k in JOINT_SUMS:
            i[k] = np.where(ok, i[k], 0)
        n = np.where(ok, n, 1)
        num, dx, dy = n * i["sxy"] - i["sx"] * i["sy"], n * i["sxx"] - i["sx"] * i["sx"], n * i["syy"] - i["sy"] * i["sy"]
        with np.errstate(invalid="ignore", divide="ignore"):
            c = num.astype(np.float64) / np.sqrt(dx.astype(np.float64) * dy.astype(np.float64))
        c = np.where((dx == 0) | (dy == 0), np.nan, np.minimum(np.maximum(c, -1.0), 1.0))
        out["corr"] = np.where(ok, c, np.nan)
        done_corr = ok
        lim = 1 << 53
        small = ok & (np.abs(num) < lim) & (dx < lim) & (dy < lim) & (n < 94906266)     # 94 906 266^2 is the first square above 2^53
        ns = np.where(small, n, 1)
        nn = (ns * ns).astype(np.float64)
        for k, v in (("cov", num), ("var_x", dx), ("var_y", dy)):
            out[k] = np.where(small, v.astype(np.float64) / nn, np.nan)
        done_mom = small
        means = ok & (i["sx"] < lim) & (i["sy"] < lim)
        nf = n.astype(np.float64)
        out["mean_x"] = np.where(means, i["sx"].astype(np.float64) / nf, np.nan)
        out["mean_y"] = np.where(means, i["sy"].astype(np.float64) / nf, np.nan)
        done_mean = means
    for j in np.nonzero(~(done_mean & done_mom & done_corr))[0]:
        n = n_o[j]
        if n <= 0:
            continue
        sx, sy, sxx, syy, sxy = (o[k][j] for k in JOINT_SUMS)
        num, dx, dy = n * sxy - sx * sy, n * sxx - sx * sx, n * syy - sy * sy
        if not done_mean[j]:
            out["mean_x"][j], out["mean_y"][j] = sx / n, sy / n
        if not done_mom[j]:
            out["cov"][j], out["var_x"][j], out["var_y"][j] = num / (n * n), dx / (n * n), dy / (n * n)
        if not done_corr[j] and dx != 0 and dy != 0:
            out["corr"][j] = min(max(float(num) / math.sqrt(float(dx) * float(dy)), -1.0), 1.0)
    return {k: v.reshape(shape) for k, v in out.items()}


def autocorrelation_time(acf: Any, n0: Any) -> dict[str, np.ndarray]:
    """The integrated autocorrelation time of autocorrelation functions ``acf`` [..., L + 1] (lag 0 first) and the
    effective sample size of cells of ``n0`` [...] samples: ``tau = 1 + 2 * (acf[1] + ... + acf[m])``, added left to right in
    float64, with ``m`` the last lag before the first ``l >= 1`` at which ``acf[l] <= 0`` or is NaN (the initial positive
    sequence); ``tau_truncated`` is true where no such lag exists up to ``L`` -- the lags were too few and ``tau`` is a
    lower bound --; ``ess = n0 / tau``.  Where ``acf[0]`` is NaN (an empty cell or a constant series) ``tau`` and ``ess`` are
    NaN and ``tau_truncated`` is false."""
    f = np.asarray(acf, dtype=np.float64)
    if f.ndim < 1 or f.shape[-1] < 1:
        msg = "acf must hold lag 0"
        raise ValueError(msg)
    tail = f[..., 1:]
    stop = ~(tail > 0.0)                                               # (NaN stops too)
    found = stop.any(axis=-1)
    total = np.zeros(f.shape[:-1])
    if tail.shape[-1]:
        m = np.where(found, np.argmax(stop, axis=-1), tail.shape[-1])  # the lags 1 .. m are summed
        keep = np.arange(tail.shape[-1]) < m[..., None]
        total = np.cumsum(np.where(keep, tail, 0.0), axis=-1)[..., -1]
    valid = ~np.isnan(f[..., 0])
    tau = np.where(valid, 1.0 + 2.0 * total, np.nan)
    with np.errstate(invalid="ignore", divide="ignore"):
        ess = np.where(valid, np.asarray(n0, dtype=np.float64) / tau, np.nan)
    return {"tau": tau, "tau_truncated": valid & ~found, "ess": ess}


WARMUP_SUMS = ("s1", "s2", "s1_all", "s2_all")
WARMUP_STATISTICS = ("warmup_s", "mean_all", "mean_steady", "mser_all", "mser_steady")


def check_warmup_batch(batch: Any) -> int:
    """``batch``, the ticks of a batch of the warm-up rule, as an int, or ValueError: a whole number in [1, 2^32)."""
    if isinstance(batch, (bool, np.bool_)) or not isinstance(batch, (int, np.integer)) or not 1 <= int(batch) < 2 ** 32:
        msg = f"batch must be a whole number of ticks in [1, 2^32), not {batch!r}"
        raise ValueError(msg)
    return int(batch)


def _warmup_columns(series: Any, names: list[str], n_edges: int) -> np.ndarray:
    """``series`` -- None (every integer series), names of ``names`` or indices, any order, duplicates allowed -- as int64
    series indices; ValueError for an unknown series, no series, and a ``ram_in_use`` column."""
    ram = ram_columns(len(names), n_edges)
    if series is None:
        return np.nonzero(~ram)[0].astype(np.int64)
    if isinstance(series, (str, bytes, int, np.integer)) and not isinstance(series, (bool, np.bool_)):
        series = [series]
    items = [x.decode() if isinstance(x, bytes) else x for x in series]
    cols: list[int] = []
    for x in items:
        if isinstance(x, str):
            if x not in names:
                msg = f"unknown series {x!r} (series_names(): {names})"
                raise ValueError(msg)
            cols.append(names.index(x))
        elif isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)) or not 0 <= int(x) < len(names):
            msg = f"{x!r} is no series name or index below {len(names)}"
            raise ValueError(msg)
        else:
            cols.append(int(x))
    if not cols:
        msg = "series selects no series"
        raise ValueError(msg)
    for j in cols:
        if ram[j]:
            msg = f"{names[j]!r} is a ram_in_use column; the warm-up rule takes integer series only"
            raise ValueError(msg)
    return np.array(cols, dtype=np.int64)


def warmup_truncation(y: Any) -> tuple[int, int, int, int, int]:
    """The MSER truncation point of ONE sequence of batch sums ``y`` (non-negative integers), in Python integers:
    ``(d, S1(d), S2(d), S1(0), S2(0))`` with ``S1(d) = sum(y[d:])``, ``S2(d) = sum(v * v for v in y[d:])``, ``m = J - d``,
    ``A(d) = m * S2(d) - S1(d) ** 2`` and ``d`` the smallest of ``0 .. J // 2`` that minimises ``A(d) / m ** 3``, compared
    exactly as ``A(d1) * m2 ** 3 < A(d2) * m1 ** 3``.  No batch: all zeros."""
    seq = [int(v) for v in y]
    n_b = len(seq)
    if n_b == 0:
        return 0, 0, 0, 0, 0
    s1 = s1_all = sum(seq)
    s2 = s2_all = sum(v * v for v in seq)
    best = (0, n_b * s2 - s1 * s1, n_b ** 3, s1, s2)                  # d, A, m^3 and the sums at d
    for d in range(1, n_b // 2 + 1):
        s1 -= seq[d - 1]
        s2 -= seq[d - 1] * seq[d - 1]
        m = n_b - d
        a = m * s2 - s1 * s1
        if a * best[2] < best[1] * m ** 3:                            # (strictly: the smaller d wins a tie)
            best = (d, a, m ** 3, s1, s2)
    return best[0], best[3], best[4], s1_all, s2_all


def series_warmup_sums(members: Any, tick_edges: Any, n_edges: int, batch: Any, columns: Any = None) -> dict[str, np.ndarray]:
    """The warm-up truncation (MSER on pooled batch sums) of ONE group per window of ticks and column, in Python integers:
    the definition the device analyzer (``af_engine_summarize_series_warmup``) matches word for word.  ``members`` is one
    scenario's sampled series (uint32 words [n_series, ticks]) or a list of them, one per replica of the group (an empty
    list: a group without a member).  With ``b = tick_edges`` and ``B = batch`` (:func:`check_warmup_batch`): member ``s`` of
    ``m_s`` ticks has the rows ``[r0, r1) = [min(b[w], m_s), min(b[w + 1], m_s))`` of window ``w``; its batch ``j`` is the
    rows ``[b[w] + j B, b[w] + (j + 1) B)``, complete when inside ``[r0, r1)``; ``J`` is the minimum over the members of
    their complete batches (0 without a member; a trailing partial batch is in no cell); ``Y_j`` is the sum over the
    members and the ``B`` rows of batch ``j`` of the word as an unsigned integer; and the truncation point is
    :func:`warmup_truncation` of ``Y_0 .. Y_{J - 1}``.  ``columns``: None (every integer series) or integer series indices,
    any order, duplicates allowed; a ``ram_in_use`` column is refused.  Returns ``batches`` int64 [W] (``J``), ``trunc``
    int64 [W, C] (``d*``), ``s1``, ``s2`` (the sums at ``d*``), ``s1_all``, ``s2_all`` (at ``d = 0``) as object arrays
    [W, C] of Python integers, and ``columns``."""
    b = check_tick_edges(tick_edges).astype(np.int64)
    n_b = check_warmup_batch(batch)
    arrs = [members] if isinstance(members, np.ndarray) else list(members)
    words = [np.ascontiguousarray(m).view(np.uint32) for m in arrs]
    for w in words:
        if w.ndim != 2 or w.shape[0] != words[0].shape[0]:
            msg = f"every member must be words [n_series, ticks] of one plan, not of shape {w.shape}"
            raise ValueError(msg)
    if words:
        n_series = int(words[0].shape[0])
        cols = _warmup_columns(None if columns is None else [int(c) for c in np.asarray(columns).reshape(-1)],
                               [str(j) for j in range(n_series)], n_edges)
    else:
        cols = np.asarray([] if columns is None else columns, dtype=np.int64).reshape(-1)
    n_win, n_c = b.shape[0] - 1, int(cols.shape[0])
    out: dict[str, np.ndarray] = {"batches": np.zeros(n_win, dtype=np.int64), "trunc": np.zeros((n_win, n_c), dtype=np.int64)}
    for k in WARMUP_SUMS:
        out[k] = np.zeros((n_win, n_c), dtype=object)
        out[k][...] = 0
    out["columns"] = cols
    for w in range(n_win):
        complete = [(min(int(b[w + 1]), x.shape[1]) - min(int(b[w]), x.shape[1])) // n_b for x in words]
        n_j = min(complete) if complete else 0
        out["batches"][w] = n_j
        if n_j == 0:
            continue
        lo, hi = int(b[w]), int(b[w]) + n_j * n_b                     # (a member with a complete batch has r0 = b[w])
        for c, col in enumerate(cols):
            parts = [x[col, lo:hi].astype(np.uint64).reshape(n_j, n_b).sum(axis=1, dtype=np.uint64) for x in words]   # B < 2^32 words below 2^32
            if len(words) * n_b <= 2 ** 32:                           # the device's width contract: Y < 2^64, exact in uint64
                y = np.sum(parts, axis=0, dtype=np.uint64).tolist()
            else:
                y = [sum(int(p[j]) for p in parts) for j in range(n_j)]
            d, s1, s2, s1_all, s2_all = warmup_truncation(y)
            out["trunc"][w, c] = d
            out["s1"][w, c], out["s2"][w, c], out["s1_all"][w, c], out["s2_all"][w, c] = s1, s2, s1_all, s2_all
    return out


def _float_of(num: int, den: int) -> float:
    """The correctly rounded float64 of the fraction ``num / den``; NaN for ``den == 0``."""
    from fractions import Fraction

    return float(Fraction(num, den)) if den else float("nan")


def series_warmup_statistics(sums: dict[str, Any], batch: Any, replicas: Any, sample_period: float,
                             tick_edges: Any) -> dict[str, np.ndarray]:
    """What the warm-up sums mean, per cell: ``sums`` holds ``batches`` [..., W], ``trunc`` and ``s1``, ``s2``, ``s1_all``,
    ``s2_all`` [..., W, C] as :func:`series_warmup_sums` or the device returns them; ``replicas`` is the number of members
    ``R`` of the group (a scalar, or one value per leading index).  With ``J = batches``, ``d = trunc``, ``m = J - d``,
    ``B = batch`` and ``b = tick_edges``:

    * ``warmup_tick = b[w] + d * B`` (int64), the first tick of the steady regime; ``warmup_s = warmup_tick *
      sample_period``;
    * ``converged = trunc < batches // 2`` (bool): the usual MSER rule -- a minimum at the search limit means the window is
      too short to show a steady regime;
    * ``mean_all = S1(0) / (J B R)`` and ``mean_steady = S1(d) / (m B R)``: the mean per tick and replica over all complete
      batches and over the steady ones;
    * ``mser_all = A(0) / (J^3 (B R)^2)`` and ``mser_steady = A(d) / (m^3 (B R)^2)`` with ``A = m S2 - S1^2``: the MSER
      statistic of the batch MEANS per tick and replica, ``sum (Z_j - mean)^2 / m^2``.

    Every float is the correctly rounded float64 of its exact fraction (``fractions.Fraction``), NaN where ``J == 0`` (or
    ``R == 0``).  Returns arrays of ``trunc``'s shape."""
    from fractions import Fraction

    n_b = check_warmup_batch(batch)
    b = check_tick_edges(tick_edges).astype(np.int64)
    trunc = np.asarray(sums["trunc"], dtype=np.int64)
    nj = np.asarray(sums["batches"], dtype=np.int64)
    if trunc.ndim < 2 or nj.shape != trunc.shape[:-1] or trunc.shape[-2] != b.shape[0] - 1:
        msg = f"trunc of shape {trunc.shape} next to batches of shape {nj.shape} and {b.shape[0] - 1} windows"
        raise ValueError(msg)
    shape = trunc.shape
    rep = np.broadcast_to(np.asarray(replicas, dtype=np.int64).reshape(np.shape(replicas) + (1,) * (trunc.ndim - np.ndim(replicas))), shape)
    nj_c = np.broadcast_to(nj[..., None], shape)
    tick = b[:-1][:, None] + trunc * n_b
    period = Fraction(float(sample_period))
    flat = {k: [int(v) for v in np.asarray(sums[k], dtype=object).reshape(-1)] for k in WARMUP_SUMS}
    out = {k: np.full(trunc.size, np.nan) for k in WARMUP_STATISTICS}
    for i, (j, d, r, t) in enumerate(zip(nj_c.reshape(-1).tolist(), trunc.reshape(-1).tolist(), rep.reshape(-1).tolist(),
                                         tick.reshape(-1).tolist())):
        if j == 0 or r == 0:
            continue
        m, scale = j - d, n_b * r
        out["warmup_s"][i] = float(t * period)
        out["mean_all"][i] = _float_of(flat["s1_all"][i], j * scale)
        out["mean_steady"][i] = _float_of(flat["s1"][i], m * scale)
        out["mser_all"][i] = _float_of(j * flat["s2_all"][i] - flat["s1_all"][i] ** 2, j ** 3 * scale * scale)
        out["mser_steady"][i] = _float_of(m * flat["s2"][i] - flat["s1"][i] ** 2, m ** 3 * scale * scale)
    res: dict[str, np.ndarray] = {k: v.reshape(shape) for k, v in out.items()}
    res["warmup_tick"] = tick
    res["converged"] = trunc < (nj_c // 2)
    return res


def series_warmup_cut(summary: dict[str, Any]) -> np.ndarray:
    """Where to cut the transient away, per (group, window): the largest ``warmup_s`` of the selected series of ``summary``
    (:func:`series_warmup_statistics`, :meth:`BatchedResults.series_warmup_summary`), NaN if any of them did not converge
    (or the cell holds no batch) -- the ``t0`` to hand to ``edges=[t0, T]`` of the latency analyzers and, as a tick, to
    ``tick_edges`` of the series analyzers.  float64 of ``warmup_s``'s shape without its last axis."""
    s = np.asarray(summary["warmup_s"], dtype=np.float64)
    ok = np.asarray(summary["converged"], dtype=bool).all(axis=-1) & ~np.isnan(s).any(axis=-1)
    if s.shape[-1] == 0:
        return np.full(s.shape[:-1], np.nan)
    return np.where(ok, np.where(np.isnan(s), -np.inf, s).max(axis=-1), np.nan)


def _exemplar_columns(ex: dict[str, np.ndarray], **extra: Any) -> dict[str, Any]:
    """The raw outputs of the exemplars call (leading axes any) as what a user reads: int64 indices with -1 in the empty
    slots, ``start`` / ``finish`` / ``latency`` with NaN there."""
    with_scenario = extra.pop("with_scenario", True)
    kept = np.asarray(ex["kept"]).astype(np.int64)
    k = int(ex["row"].shape[-1])
    empty = np.arange(k) >= kept[..., None]
    pair = np.where(empty[..., None], np.nan, np.asarray(ex["clock"], dtype=np.float64))
    out: dict[str, Any] = {}
    if with_scenario:
        out["scenario"] = np.where(empty, -1, np.asarray(ex["scenario"]).astype(np.int64))
    out["row"] = np.where(empty, -1, np.asarray(ex["row"]).astype(np.int64))
    with np.errstate(invalid="ignore", over="ignore"):
        out.update(start=pair[..., 0], finish=pair[..., 1], latency=pair[..., 1] - pair[..., 0])
    out.update(total=np.asarray(ex["total"]).astype(np.int64), kept=kept, **extra)
    return out


class ScenarioResults:
    """One scenario of a sweep; API of the reference's ``ResultsAnalyzer``."""

    _WINDOW_SIZE_S: float = 1.0

    def __init__(self, plan: DevicePlan, counts: np.ndarray, clock: np.ndarray, samples: np.ndarray | None) -> None:
        self._plan = plan
        self.counts = counts
        self.rqs_clock = clock            # float64 [completed, 2] (start, finish)
        self._samples = samples           # uint32 [n_series, ticks] raw words or None
        self.latencies: np.ndarray | None = None
        self.latency_stats: dict[str, float] | None = None
        self.throughput_series: Series | None = None
        self.sampled_metrics: dict[str, dict[str, list[float]]] | None = None
        self._arrival_times: Any = None   # () -> float64 arrival times: set by BatchedResults for get_arrival_counts

    # ---- counters -------------------------------------------------------------
    @property
    def total_generated(self) -> int:
        return int(self.counts[_abi.CNT_GENERATED])

    @property
    def total_completed(self) -> int:
        return int(self.counts[_abi.CNT_COMPLETED])

    @property
    def total_dropped(self) -> int:
        return int(self.counts[_abi.CNT_DROPPED])

    @property
    def request_events(self) -> int:
        return int(self.counts[_abi.CNT_EVENTS])

    @property
    def flags(self) -> int:
        return int(self.counts[_abi.CNT_FLAGS])

    # ---- analyzer.py:75-142 -----------------------------------------------------
    def process_all_metrics(self) -> None:
        if self.latency_stats is None and len(self.rqs_clock):
            self._process_event_metrics()
        if self.sampled_metrics is None:
            self._extract_sampled_metrics()

    def _process_event_metrics(self) -> None:
        start, finish = self.rqs_clock[:, 0], self.rqs_clock[:, 1]
        arr = finish - start
        self.latencies = arr
        if arr.size:
            self.latency_stats = {
                "total_requests": float(arr.size),
                "mean": float(np.mean(arr)),
                "median": float(np.median(arr)),
                "std_dev": float(np.std(arr)),
                "p95": float(np.percentile(arr, 95)),
                "p99": float(np.percentile(arr, 99)),
                "min": float(np.min(arr)),
                "max": float(np.max(arr)),
            }
        else:
            self.latency_stats = {}
        self.throughput_series = self._throughput(self._WINDOW_SIZE_S)

    def _throughput(self, window_s: float) -> Series:
        """Buckets (k-1, k]*window counting ``finish <= k*window`` (analyzer.py:107-125)."""
        completion = np.sort(self.rqs_clock[:, 1])
        end_time = self._plan.total_time
        timestamps: list[float] = []
        current_end = float(window_s)
        while current_end <= end_time:  # same float accumulation as the reference
            timestamps.append(current_end)
            current_end += float(window_s)
        edges = np.searchsorted(completion, np.asarray(timestamps), side="right")
        counts = np.diff(np.concatenate([[0], edges]))
        return timestamps, [float(c) / float(window_s) for c in counts]

    def _extract_sampled_metrics(self) -> None:
        metrics: dict[str, dict[str, list[float]]] = defaultdict(dict)
        plan, s = self._plan, self._samples
        enabled = set(plan.payload["sim_settings"]["enabled_sample_metrics"])
        servers_sampled = {"ready_queue_len", "event_loop_io_sleep", "ram_in_use"} <= enabled
        E = plan.n_edges
        for v, sid in enumerate(plan.server_ids):
            rows = {
                "ready_queue_len": (E + 3 * v, False),
                "event_loop_io_sleep": (E + 3 * v + 1, False),
                "ram_in_use": (E + 3 * v + 2, True),
            }
            for name, (row, is_float) in rows.items():
                if name not in enabled:
                    continue
                if s is None or not servers_sampled:
                    metrics[name][sid] = []
                elif is_float:
                    metrics[name][sid] = s[row].view(np.float32).astype(np.float64).tolist()
                else:
                    metrics[name][sid] = s[row].view(np.int32).tolist()
        if "edge_concurrent_connection" in enabled:
            for e, eid in enumerate(plan.edge_ids):
                metrics["edge_concurrent_connection"][eid] = [] if s is None else s[e].view(np.int32).tolist()
        self.sampled_metrics = metrics

    # ---- analyzer.py:147-244 (public accessors) -----------------------------------
    def list_server_ids(self) -> list[str]:
        return list(self._plan.server_ids)

    def get_latency_stats(self) -> dict[str, float]:
        self.process_all_metrics()
        return self.latency_stats or {}

    def format_latency_stats(self) -> str:
        stats = self.get_latency_stats()
        if not stats:
            return "Latency stats: (empty)"
        lines = ["════════ LATENCY STATS ════════"]
        lines.extend(f"{k.upper():<20} = {stats[k]:.6f}" for k in LATENCY_KEYS if k in stats)
        return "\n".join(lines)

    def get_throughput_series(self, window_s: float | None = None) -> Series:
        self.process_all_metrics()
        if window_s is None or window_s == self._WINDOW_SIZE_S:
            return self.throughput_series or ([], [])
        return self._throughput(float(window_s))

    def get_latency_window_stats(self, window_s: float | None = None, edges: Any = None, *, window_of: str = "finish") -> np.ndarray:
        """Latency statistics per time window (by finish time; ``window_of="arrival"``: by start time): float64 [W, 8] in
        LATENCY_KEYS order, for windows of ``window_s`` seconds (default 1 s, :func:`window_edges`) or explicit ``edges``:
        :func:`latency_window_stats`."""
        return latency_window_stats(self.rqs_clock, _resolve_edges(window_s, edges, self._plan.total_time), window_of)

    def get_arrival_counts(self, window_s: float | None = None, edges: Any = None) -> np.ndarray:
        """Arrivals per time window, int64 [W]: the requests SENT with ``edges[w] < t <= edges[w + 1]``, completed or not
        (:func:`arrival_window_counts` on the scenario's arrival times, which :meth:`BatchedResults.arrival_times`
        regenerates on the device).  Windows as in :meth:`get_latency_window_stats`.  Only for a scenario taken from a
        run's results: a hand-made object has no arrival times."""
        if self._arrival_times is None:
            msg = "this ScenarioResults does not come from a run: it has no arrival times"
            raise ValueError(msg)
        e = _resolve_edges(window_s, edges, self._plan.total_time)
        return np.diff(arrival_window_counts(self._arrival_times(), e))

    def get_latency_quantiles(self, levels: Any, *, window_s: float | None = None, edges: Any = None,
                              thresholds: Any = None, window_of: str = "finish") -> dict[str, Any]:
        """Any latency quantiles (``levels`` in [0, 1]) and, with ``thresholds`` (seconds), how many requests met each
        objective: :func:`latency_window_quantiles`.  Neither ``window_s`` nor ``edges``: the whole run (``count`` scalar,
        ``quantiles`` [Q], ``within`` [T]); otherwise per window of ``window_s`` seconds or explicit ``edges`` (``count``
        [W], ``quantiles`` [W, Q], ``within`` [W, T]).  ``share`` = within / count (NaN where empty).
        ``window_of="arrival"``: windows by start time (needs windows)."""
        whole = window_s is None and edges is None
        e = None if whole else _resolve_edges(window_s, edges, self._plan.total_time)
        count, quant, within = latency_window_quantiles(self.rqs_clock, e, levels, thresholds, window_of)
        with np.errstate(invalid="ignore", divide="ignore"):
            share = np.where(count[:, None] > 0, within / count[:, None].astype(np.float64), np.nan)
        if whole:
            return {"count": int(count[0]), "quantiles": quant[0], "within": within[0], "share": share[0], "edges": None,
                    "window_of": window_of}
        return {"count": count, "quantiles": quant, "within": within, "share": share, "edges": e, "window_of": window_of}

    def get_series_window_stats(self, window_s: float | None = None, *, ticks_per_window: int | None = None,
                                tick_edges: Any = None, thresholds: Any = None) -> dict[str, np.ndarray]:
        """Statistics of every sampled series per window of ticks (:func:`series_window_stats`): windows of ``window_s``
        seconds (a multiple of the sample period; default 1 s), of ``ticks_per_window`` ticks, or explicit ``tick_edges``.
        Sample ``k`` carries the label ``k * sample_period`` (``get_series``), so a window of ``m`` ticks labelled ``t``
        holds the samples labelled ``t <= label < t + m * sample_period``.  ``min`` / ``max`` of a ``ram_in_use`` series are
        the float minimum / maximum (float32 bits, -0.0 below +0.0), those of the other series the smallest / largest count."""
        if self._samples is None:
            msg = "run(collect_samples=False) kept no sampled series"
            raise RuntimeError(msg)
        b = _resolve_tick_edges(window_s, ticks_per_window, tick_edges, self._plan.sample_period, self._plan.tick_count)
        return series_window_stats(self._samples, b, self._plan.n_edges, thresholds)

    def get_series_window_quantiles(self, levels: Any, window_s: float | None = None, *, ticks_per_window: int | None = None,
                                    tick_edges: Any = None, series: Any = None) -> dict[str, Any]:
        """Exact quantiles ``levels`` (in [0, 1], at most 16) of the sampled series per window of ticks
        (:func:`series_window_quantiles`): ``count`` [W], ``quantiles`` float64 [W, C, Q] (NaN in an empty window),
        ``levels``, ``series`` (the indices of the C selected series) and ``tick_edges``.  Windows as in
        :meth:`get_series_window_stats`; ``series``: None (every series) or series indices, any order."""
        if self._samples is None:
            msg = "run(collect_samples=False) kept no sampled series"
            raise RuntimeError(msg)
        b = _resolve_tick_edges(window_s, ticks_per_window, tick_edges, self._plan.sample_period, self._plan.tick_count)
        col = _check_series_columns(series, int(np.asarray(self._samples).shape[0]))
        count, quant = series_window_quantiles(self._samples, b, self._plan.n_edges, levels, col)
        return {"count": count, "quantiles": quant, "levels": check_series_levels(levels), "series": col, "tick_edges": b}

    def get_series_excursions(self, thresholds: Any, window_s: float | None = None, *, ticks_per_window: int | None = None,
                              tick_edges: Any = None) -> dict[str, np.ndarray]:
        """Excursions of every sampled series above ``thresholds`` (a vector [n_series]; None: 0.0 each) per window of
        ticks (:func:`series_window_excursions`): how many ticks above, how many runs, the longest run and its start, the
        first and the last tick above and the tick of the peak, as int64 (-1: no such tick), and ``tick_edges``.  Windows as
        in :meth:`get_series_window_stats`, but with none of the three given ONE window over the whole run."""
        if self._samples is None:
            msg = "run(collect_samples=False) kept no sampled series"
            raise RuntimeError(msg)
        if window_s is None and ticks_per_window is None and tick_edges is None:
            tick_edges = [0, max(self._plan.tick_count, 1)]
        b = _resolve_tick_edges(window_s, ticks_per_window, tick_edges, self._plan.sample_period, self._plan.tick_count)
        out = series_window_excursions(self._samples, b, self._plan.n_edges, thresholds)
        out["tick_edges"] = b
        return out

    def get_series_histogram(self, bins: int = 64, window_s: float | None = None, *, ticks_per_window: int | None = None,
                             tick_edges: Any = None, series: Any = None, lo: Any = None, width: Any = None) -> dict[str, Any]:
        """Occupancy histograms of the sampled series per window of ticks (:func:`series_window_histogram`): ``count`` [W],
        ``hist`` int64 [W, C, bins], ``under`` / ``over`` [W, C], ``bin_edges`` [C, bins + 1], ``ram``, ``series`` (the
        indices of the C selected series) and ``tick_edges``.  Windows as in :meth:`get_series_window_stats`; ``series``:
        None (every series) or series indices, any order, duplicates allowed; ``lo`` / ``width``: None (0.0 / 1.0), a scalar
        or one value per selected series."""
        if self._samples is None:
            msg = "run(collect_samples=False) kept no sampled series"
            raise RuntimeError(msg)
        b = _resolve_tick_edges(window_s, ticks_per_window, tick_edges, self._plan.sample_period, self._plan.tick_count)
        col = _check_series_columns(series, int(np.asarray(self._samples).shape[0]))
        out: dict[str, Any] = series_window_histogram(self._samples, b, self._plan.n_edges, bins, col, lo, width)
        out.update(series=col, tick_edges=b)
        return out

    def get_series_combined(self, combos: Any, window_s: float | None = None, *, ticks_per_window: int | None = None,
                            tick_edges: Any = None, thresholds: Any = None, bins: int = 0, lo: Any = None,
                            width: Any = None) -> dict[str, Any]:
        """Combinations across the sampled series per window of ticks (:func:`series_combined_window_stats`): ``combos`` is
        ``{label: (op, selection)}`` over :func:`series_names_of` (:func:`check_series_combinations`), such as
        ``{"imbalance": ("spread", "*:ready_queue_len")}``.  Returns ``count`` [W], ``mean``, ``min``, ``max``, ``above``
        [W, C], with ``bins`` the histogram outputs, and ``names``, ``ops``, ``columns`` and ``tick_edges``.  Windows as in
        :meth:`get_series_window_stats`; ``thresholds``: None (0.0) or one value per combination."""
        if self._samples is None:
            msg = "run(collect_samples=False) kept no sampled series"
            raise RuntimeError(msg)
        b = _resolve_tick_edges(window_s, ticks_per_window, tick_edges, self._plan.sample_period, self._plan.tick_count)
        labels, ops, columns = check_series_combinations(combos, series_names_of(self._plan), self._plan.n_edges)
        out: dict[str, Any] = series_combined_window_stats(self._samples, b, self._plan.n_edges, list(zip(ops, columns)), thresholds,
                                                           bins, lo, width)
        out.update(names=labels, ops=ops, columns=columns, tick_edges=b)
        return out

    def get_series_joint(self, pairs: Any, window_s: float | None = None, *, ticks_per_window: int | None = None,
                         tick_edges: Any = None) -> dict[str, Any]:
        """Covariance and correlation of pairs of integer series per window of ticks, lagged or not, from the host
        definition: ``pairs`` is ``{label: (a, b)}`` or ``{label: (a, b, lag)}`` over :func:`series_names_of`
        (:func:`check_series_pairs`), such as ``{"queues": ("srv-1:ready_queue_len", "srv-2:ready_queue_len")}``.  Returns
        the sums of :func:`series_joint_sums` (``n`` and ``sx`` ... ``sxy`` [W, P]), the statistics of
        :func:`series_joint_statistics` (``mean_x``, ``mean_y``, ``cov``, ``corr``, ``var_x``, ``var_y`` [W, P]) and
        ``labels``, ``a``, ``b``, ``lag``, ``tick_edges``.  Windows as in :meth:`get_series_window_stats`."""
        if self._samples is None:
            msg = "run(collect_samples=False) kept no sampled series"
            raise RuntimeError(msg)
        b = _resolve_tick_edges(window_s, ticks_per_window, tick_edges, self._plan.sample_period, self._plan.tick_count)
        labels, ca, cb, lag = check_series_pairs(pairs, series_names_of(self._plan), self._plan.n_edges)
        out: dict[str, Any] = series_joint_sums(self._samples, b, self._plan.n_edges, (ca, cb, lag))
        out.update(series_joint_statistics(out))
        out.update(labels=labels, a=ca, b=cb, lag=lag, tick_edges=b)
        return out

    def get_series_warmup(self, batch: int = 5, window_s: float | None = None, *, ticks_per_window: int | None = None,
                          tick_edges: Any = None, series: Any = None) -> dict[str, Any]:
        """Where this scenario's sampled series leave their initial transient, per window of ticks, from the host
        definition: the MSER rule on batches of ``batch`` ticks (:func:`series_warmup_sums` with this scenario as the only
        member, :func:`series_warmup_statistics`).  ``series``: None (every integer series), names of
        :func:`series_names_of` or indices; no ``ram_in_use`` column.  Windows as in :meth:`get_series_window_stats`; none
        given: one window over the whole run.  Returns ``batches`` [W], ``trunc``, the four sums, ``warmup_tick``,
        ``warmup_s``, ``converged``, ``mean_all``, ``mean_steady``, ``mser_all``, ``mser_steady`` [W, C], ``cut`` [W]
        (:func:`series_warmup_cut`) and ``series`` (the names), ``columns``, ``batch``, ``tick_edges``."""
        if self._samples is None:
            msg = "run(collect_samples=False) kept no sampled series"
            raise RuntimeError(msg)
        n_b = check_warmup_batch(batch)
        if window_s is None and ticks_per_window is None and tick_edges is None:
            tick_edges = [0, max(self._plan.tick_count, 1)]
        b = _resolve_tick_edges(window_s, ticks_per_window, tick_edges, self._plan.sample_period, self._plan.tick_count)
        names = series_names_of(self._plan)
        cols = _warmup_columns(series, names, self._plan.n_edges)
        out: dict[str, Any] = series_warmup_sums(np.asarray(self._samples), b, self._plan.n_edges, n_b, cols)
        out.update(series_warmup_statistics(out, n_b, 1, self._plan.sample_period, b))
        out.update(cut=series_warmup_cut(out), series=[names[j] for j in cols], batch=n_b, tick_edges=b)
        return out

    def get_latency_by_state(self, series: Any, bins: int = 8, lo: float = 0.0, width: float = 1.0, window_s: float | None = None,
                             edges: Any = None, levels: Any = None, thresholds: Any = None) -> dict[str, Any]:
        """Latency by the state the request met on arrival (:func:`latency_state_cells`): the requests that arrived while
        ``series`` (a name ``"<id>:<metric>"`` as in :meth:`BatchedResults.series_names`, or an index) was in bin ``b`` of
        ``bins`` bins of ``width`` from ``lo`` (the last bin takes the overflow).  ``stats`` float64 [W', bins, 8] and ``count``
        [W', bins]; with ``levels`` / ``thresholds`` also ``quantiles`` [W', bins, Q], ``within`` [W', bins, T] and ``share``.
        Windows by ARRIVAL time of ``window_s`` seconds or explicit ``edges``; neither: one window (W' = 1, ``edges`` None).
        ``bin_lo`` [bins] are the bins' lower edges, ``series`` the series index.  Right-censored cohorts, as
        ``window_of="arrival"``."""
        if self._samples is None:
            msg = "run(collect_samples=False) kept no sampled series"
            raise RuntimeError(msg)
        col = _state_series(series, series_names_of(self._plan))
        n_bins, lo_f, width_f, period = check_state_bins(bins, lo, width, self._plan.sample_period)
        e = None if window_s is None and edges is None else _resolve_edges(window_s, edges, self._plan.total_time)
        args = (self.rqs_clock, self._samples, self._plan.n_edges, period, col, n_bins)
        stats = latency_state_stats(*args, lo_f, width_f, e)
        out: dict[str, Any] = {"stats": stats, "count": stats[:, :, 0].astype(np.int64), "keys": LATENCY_KEYS, "edges": e,
                               "bin_lo": lo_f + np.arange(n_bins, dtype=np.float64) * width_f, "series": col}
        if levels is not None or thresholds is not None:
            count, quant, within = latency_state_quantiles(*args, [] if levels is None else levels, thresholds, lo_f, width_f, e)
            with np.errstate(invalid="ignore", divide="ignore"):
                share = np.where(count[:, :, None] > 0, within / count[:, :, None].astype(np.float64), np.nan)
            out.update(quantiles=quant, within=within, share=share, levels=check_levels([] if levels is None else levels),
                       thresholds=check_slo_thresholds(thresholds))
        return out

    def get_sampled_metrics(self) -> dict[str, dict[str, list[float]]]:
        self.process_all_metrics()
        assert self.sampled_metrics is not None
        return self.sampled_metrics

    def get_metric_map(self, key: Any) -> dict[str, list[float]]:
        self.process_all_metrics()
        assert self.sampled_metrics is not None
        name = getattr(key, "value", key)
        return self.sampled_metrics.get(name, {}) or {}

    def get_series(self, key: Any, entity_id: str) -> Series:
        vals = self.get_metric_map(key).get(entity_id, [])
        times = (np.arange(len(vals)) * self._plan.sample_period).tolist()
        return times, vals

    def get_in_flight(self) -> Series:
        """Requests in flight end to end at every sample instant, as a ``Series`` like :meth:`get_series`' (sample ``k``
        carries the label ``k * sample_period``): :func:`in_flight_series` on the scenario's clock rows -- the "in-flight
        requests" of a dashboard, which no sampled series holds.  COMPLETED requests only: dropped requests and those still
        in flight when the run ended are missing, so the last seconds under-count
        (:meth:`BatchedResults.arrival_summary`'s ``lost`` says by how much)."""
        ticks = min(int(self.counts[_abi.CNT_TICKS]), max(int(self._plan.tick_count), 0))
        if self._samples is not None:
            ticks = min(ticks, int(self._samples.shape[1]))
        vals = in_flight_series(self.rqs_clock, ticks, self._plan.sample_period)["in_flight"]
        times = (np.arange(len(vals)) * self._plan.sample_period).tolist()
        return times, vals.astype(np.float64).tolist()

    def get_alerts(self, slo_s: float, rules: Any, window_s: float | None = None, *, ticks_per_window: int | None = None,
                   tick_edges: Any = None, timeout_s: float | None = None) -> dict[str, np.ndarray]:
        """Burn-rate alert rules on this scenario's clock rows, through the host definition (:func:`scenario_alerts`):
        ``total`` / ``bad`` uint32 [ticks], ``cond`` / ``firing`` bool [R, ticks] and the window cells of
        :func:`alert_window_stats` (``fired``, ``episodes``, ``longest``, ``longest_start``, ``first``, ``last`` int64 [W, R], -1:
        no such tick).  ``rules`` and the windows as in :meth:`BatchedResults.alert_summary`.  COMPLETED requests only -- unless
        ``timeout_s`` is given: then a request without an answer within ``timeout_s`` is an error at ``arrival + timeout_s``
        (:func:`scenario_outcome_alerts` on the scenario's arrival times, with ``timeouts``, ``completions``, ``deficit`` and
        ``timed_out`` in the result; only for a scenario taken from a run's results)."""
        ticks = min(int(self.counts[_abi.CNT_TICKS]), max(int(self._plan.tick_count), 0))
        if self._samples is not None:
            ticks = min(ticks, int(self._samples.shape[1]))
        b = _resolve_tick_edges(window_s, ticks_per_window, tick_edges, self._plan.sample_period, self._plan.tick_count)
        if timeout_s is None:
            return scenario_alerts(self.rqs_clock, ticks, self._plan.sample_period, slo_s, rules, b)
        if self._arrival_times is None:
            msg = "this ScenarioResults does not come from a run: it has no arrival times"
            raise ValueError(msg)
        return scenario_outcome_alerts(self.rqs_clock, self._arrival_times(), ticks, self._plan.sample_period, slo_s, timeout_s, rules, b)

    def get_slowest_requests(self, k: int = 16, window_s: float | None = None, edges: Any = None, window_of: str = "finish") -> dict[str, Any]:
        """The ``k`` slowest requests of the scenario, per time window (``window_s`` seconds or explicit ``edges``, by
        ``window_of``) or, with neither, of the whole run: :func:`latency_exemplars` on the scenario's clock rows.  ``row``
        int64 [W', k] indexes ``rqs_clock`` (-1 in an empty slot), ``start`` / ``finish`` / ``latency`` float64 [W', k] (NaN
        in an empty slot), ``total`` and ``kept`` int64 [W'], ``edges`` (None for the whole run) and ``window_of``."""
        e = None if window_s is None and edges is None else _resolve_edges(window_s, edges, self._plan.total_time)
        ex = latency_exemplars([self.rqs_clock], k, e, window_of)
        return _exemplar_columns(ex, edges=e, window_of=window_of, with_scenario=False)

    def get_latency_histogram(self, window_s: float | None = None, edges: Any = None, window_of: str = "finish", *, sub_bits: int = 5,
                              min_exp: int = -20, octaves: int = 32) -> dict[str, Any]:
        """The log-linear latency histogram of the scenario, per time window (``window_s`` seconds or explicit ``edges``, by
        ``window_of``) or, with neither, of the whole run: :func:`latency_histogram` on the scenario's clock rows.  ``hist``
        int64 [W', B], ``count`` / ``under`` / ``over`` / ``nan`` int64 [W'], ``bin_edges`` float64 [B + 1] seconds, ``edges``
        (None for the whole run), ``window_of`` and the binning."""
        e = None if window_s is None and edges is None else _resolve_edges(window_s, edges, self._plan.total_time)
        m, e0, o, _ = check_latency_bins(sub_bits, min_exp, octaves)
        h = latency_histogram([self.rqs_clock], e, window_of, sub_bits=m, min_exp=e0, octaves=o)
        return {**{k: v.astype(np.int64) for k, v in h.items()}, "bin_edges": latency_bin_edges(m, e0, o), "edges": e,
                "window_of": window_of, "sub_bits": m, "min_exp": e0, "octaves": o}

    # ---- bridge to the reference's own analyzer / plots ----------------------------
    def to_reference_analyzer(self) -> Any:
        """Hydrate the reference's ``ResultsAnalyzer`` via duck-typed shims (needs `asyncflow`).

        Same trick as the reference's tests/unit/metrics/test_analyzer.py:34-95.
        """
        from types import SimpleNamespace

        from asyncflow.config.constants import SampledMetricName  # type: ignore[import-not-found]
        from asyncflow.metrics.analyzer import ResultsAnalyzer  # type: ignore[import-not-found]

        sm = self.get_sampled_metrics()
        client = SimpleNamespace(rqs_clock=[SimpleNamespace(start=float(a), finish=float(b)) for a, b in self.rqs_clock])
        servers = [
            SimpleNamespace(
                server_config=SimpleNamespace(id=sid),
                enabled_metrics={SampledMetricName(k): v[sid] for k, v in sm.items() if sid in v},
            )
            for sid in self._plan.server_ids
        ]
        edges = [
            SimpleNamespace(
                edge_config=SimpleNamespace(id=eid),
                enabled_metrics={SampledMetricName(k): v[eid] for k, v in sm.items() if eid in v},
            )
            for eid in self._plan.edge_ids
        ]
        settings = SimpleNamespace(
            total_simulation_time=int(self._plan.total_time), sample_period_s=self._plan.sample_period
        )
        return ResultsAnalyzer(client=client, servers=servers, edges=edges, settings=settings)


class BatchedResults:
    """All scenarios of a sweep; device-resident until a scenario is read."""

    def __init__(self, plan: DevicePlan, seeds: np.ndarray, counts: Any, clock: Any, samples: Any,
                 stats: _abi.AfStats, wall_s: float, overrides: dict[str, np.ndarray] | None = None, *,
                 online_hist: Any = None, online_rps: Any = None, online_hist_max: float = 0.0, draw_capacity: int = 0) -> None:
        self.plan = plan
        self.seeds = seeds
        #: the run's ``draw_capacity`` (0: the clock capacity, as the engine takes it): the arrivals it simulated are the
        #: sampler's first that many (:meth:`arrival_summary` regenerates exactly those)
        self.draw_capacity = int(draw_capacity)
        self._counts_t, self._clock_t, self._samples_t = counts, clock, samples
        self.counts = counts.cpu().numpy().view(np.uint32)
        self.kernel_ms = float(stats.kernel_ms)
        self.engine_stats = stats
        self.wall_s = wall_s
        self.overrides = overrides or {}
        #: kernel-side summary (SimulationRunner(online_summary=...)): int32 [n, bins] / [n, floor(T)] on the device
        self.online_hist, self.online_rps, self.online_hist_max = online_hist, online_rps, float(online_hist_max)
        self._summ_engine: Any = None      # one af_engine_t serves every summary() call of this object
        #: '' when the stage-parallel kernel ran the plan, else why the next-event kernels did (Engine.flow_reason())
        self.flow_reason: str = ""

    def close(self) -> None:
        """Release the analyzer engine kept by :meth:`summary` (also done on garbage collection)."""
        if self._summ_engine is not None:
            self._summ_engine.close()
            self._summ_engine = None

    def __del__(self) -> None:  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def __len__(self) -> int:
        return int(self.counts.shape[0])

    @property
    def flags(self) -> np.ndarray:
        return self.counts[:, _abi.CNT_FLAGS]

    @property
    def request_events(self) -> np.ndarray:
        return self.counts[:, _abi.CNT_EVENTS].astype(np.int64)

    def raise_on_overflow(self) -> None:
        bad = np.nonzero(self.flags & _abi.FATAL_FLAGS)[0]
        if len(bad):
            f = int(np.bitwise_or.reduce(self.flags[bad]))
            why = "; ".join(v for k, v in _abi.FLAG_NAMES.items() if f & k & _abi.FATAL_FLAGS)
            msg = f"{len(bad)} scenario(s) overflowed an engine capacity (first: #{int(bad[0])}): {why}"
            raise OverflowError(msg)

    def raise_on_negative_delay(self) -> None:
        """The reference's error behaviour for a send whose ``transit + spike`` is negative (the residue of overlapping
        spikes under a zero transit time): ``env.timeout`` raises ``ValueError("Negative delay ...")`` (edge.py:107) and
        the run produces nothing.  The engine reports such scenarios (``AF_FLAG_NEGATIVE_DELAY``); this raises for them."""
        bad = np.nonzero(self.flags & _abi.FLAG_NEGATIVE_DELAY)[0]
        if len(bad):
            msg = (f"Negative delay: {len(bad)} scenario(s) sent a message with transit + spike < 0 (first: #{int(bad[0])}, seed "
                   f"{int(self.seeds[bad[0]])}); the reference raises the same error for them "
                   "(SimulationRunner(on_negative_delay='flag') keeps the results and the flag)")
            raise ValueError(msg)

    def __getitem__(self, i: int) -> ScenarioResults:
        i = int(i)
        if not 0 <= i < len(self):
            raise IndexError(i)
        counts = self.counts[i]
        n = min(int(counts[_abi.CNT_COMPLETED]), int(self._clock_t.shape[1])) if self._clock_t is not None else 0
        clock = self._clock_t[i, :n].cpu().numpy() if self._clock_t is not None else np.zeros((0, 2))
        samples = None
        if self._samples_t is not None:  # device layout [tick][series_pitch] -> [series][tick]
            k = min(int(counts[_abi.CNT_TICKS]), int(self._samples_t.shape[1]))
            rows = self._samples_t[i, :k, : self.plan.n_series].cpu().numpy().view(np.uint32)
            samples = np.ascontiguousarray(rows.T)
        one = ScenarioResults(self.plan, counts, clock, samples)
        one._arrival_times = lambda: self.arrival_times(i)   # noqa: SLF001
        return one

    def __iter__(self) -> Iterator[ScenarioResults]:
        return (self[i] for i in range(len(self)))

    # ---- device-side reduction of every scenario at once ---------------------------
    def summary(self, rps: bool = True, hist_bins: int = 0, hist_max: float = 0.0,
                series: bool = False) -> dict[str, Any]:
        """Per-scenario latency stats, 1-s RPS series, optional latency histogram and
        per-series mean/max, computed by the HIP analyzer (``af_engine_summarize``).

        Returns torch tensors on the run's device: ``stats`` float64 [n, 8] in
        LATENCY_KEYS order (= ``ResultsAnalyzer.get_latency_stats`` per scenario,
        metrics/analyzer.py:83-104), ``rps`` float32 [n, floor(T)] (analyzer.py:108-126),
        ``hist`` int32 [n, hist_bins], ``series_mean`` float64 / ``series_max`` int32
        [n, n_series] (the ram_in_use columns of ``series_max`` hold float32 BITS, like the sample
        words they are the maximum of: decode with :meth:`decode_series_max`; it is the FLOAT maximum, also of a
        column that holds negative residues of the reference's float arithmetic).  The latency statistics, RPS windows,
        histogram, ``series_max`` and the ``series_mean`` of the integer series are bit-equal to numpy's (round 6: mean and
        std_dev too -- the kernel adds in numpy's own order, af_summary.hpp).  ``series_mean`` of a ram_in_use column is
        bit-equal to numpy's while the values add exactly (multiples of 1/256 MB below 2^16, every integer RAM need), and
        otherwise within ``n * 2**-52`` of ``math.fsum(x) / n`` relative to ``sum(abs(x)) / n`` (per-thread partial sums in
        a fixed order: the same bytes from run to run and in every batch).
        A run made with ``SimulationRunner(summary=...)`` computed the summary in the engine call of the simulation itself
        (``af_engine_run_summarized``): the same arguments return those tensors.
        """
        import torch

        from .engine import Engine

        pre = getattr(self, "_summary_from_run", None)
        if pre is not None and pre["_kw"] == {"rps": rps, "hist_bins": hist_bins, "hist_max": hist_max, "series": series}:
            return {k: v for k, v in pre.items() if k != "_kw"}

        if self._clock_t is None:
            if self.online_hist is not None:
                return self._summary_from_online()
            msg = "run(collect_clock=False) kept no rqs_clock (pass online_summary=... to keep a kernel-side summary)"
            raise RuntimeError(msg)
        if series and self._samples_t is None:
            msg = "run(collect_samples=False) kept no sampled series"
            raise RuntimeError(msg)
        clock = self._clock_t
        n, cap = int(clock.shape[0]), int(clock.shape[1])
        dev = clock.device
        T = int(self.plan.total_time)
        stats = torch.empty((n, 8), dtype=torch.float64, device=dev)
        rps_t = torch.empty((n, T), dtype=torch.float32, device=dev) if rps and T > 0 else None
        hist_t = torch.empty((n, hist_bins), dtype=torch.int32, device=dev) if hist_bins else None
        smean = torch.empty((n, self.plan.n_series), dtype=torch.float64, device=dev) if series else None
        smax = torch.empty((n, self.plan.n_series), dtype=torch.int32, device=dev) if series else None
        torch.cuda.synchronize(dev)
        if self._summ_engine is None:
            self._summ_engine = Engine(self.plan, dev.index if dev.index is not None else torch.cuda.current_device())
        st = self._summ_engine.summarize(
            n,
            clock_ptr=clock.data_ptr(), clock_capacity=cap,
            samples_ptr=self._samples_t.data_ptr() if self._samples_t is not None else 0,
            tick_capacity=int(self._samples_t.shape[1]) if self._samples_t is not None else 0,
            counts_ptr=self._counts_t.data_ptr(),
            stats_ptr=stats.data_ptr(),
            rps_ptr=rps_t.data_ptr() if rps_t is not None else 0, rps_buckets=T if rps_t is not None else 0,
            hist_ptr=hist_t.data_ptr() if hist_t is not None else 0, hist_bins=hist_bins, hist_max=hist_max,
            series_mean_ptr=smean.data_ptr() if smean is not None else 0,
            series_max_ptr=smax.data_ptr() if smax is not None else 0,
        )
        out: dict[str, Any] = {"stats": stats, "keys": LATENCY_KEYS, "summary_ms": float(st.summary_ms)}
        if rps_t is not None:
            out["rps"] = rps_t
        if hist_t is not None:
            out["hist"] = hist_t
        if series:
            out["series_mean"], out["series_max"] = smean, smax
        return out

    def _summary_from_online(self) -> dict[str, Any]:
        """Latency statistics read from the kernel-side histogram: total exact, everything else accurate
        to one bin (mean / std from bin centres, percentiles by linear interpolation inside the bin,
        min / max = edges of the extreme occupied bins)."""
        import torch

        h = self.online_hist.to(torch.float64)
        n, bins = h.shape
        width = self.online_hist_max / bins
        centres = (torch.arange(bins, device=h.device, dtype=torch.float64) + 0.5) * width
        total = h.sum(dim=1)
        safe = total.clamp(min=1.0)
        mean = (h * centres).sum(dim=1) / safe
        var = (h * (centres.unsqueeze(0) - mean.unsqueeze(1)) ** 2).sum(dim=1) / safe
        cdf = h.cumsum(dim=1)

        def pct(q: float) -> Any:
            target = (q / 100.0) * total
            idx = torch.searchsorted(cdf, target.unsqueeze(1).contiguous(), right=False).squeeze(1).clamp(max=bins - 1)
            below = torch.where(idx > 0, cdf.gather(1, (idx - 1).clamp(min=0).unsqueeze(1)).squeeze(1), torch.zeros_like(total))
            inside = h.gather(1, idx.unsqueeze(1)).squeeze(1).clamp(min=1.0)
            return (idx.to(torch.float64) + ((target - below) / inside).clamp(0.0, 1.0)) * width

        occupied = h > 0
        first = torch.where(occupied.any(dim=1), occupied.to(torch.int64).argmax(dim=1), torch.zeros(n, dtype=torch.int64, device=h.device))
        last = bins - 1 - occupied.flip(dims=[1]).to(torch.int64).argmax(dim=1)
        stats = torch.stack([total, mean, pct(50.0), var.sqrt(), pct(95.0), pct(99.0), first.to(torch.float64) * width,
                             (last.to(torch.float64) + 1.0) * width], dim=1)
        stats = torch.where((total > 0).unsqueeze(1), stats, torch.full_like(stats, float("nan")))
        stats[:, 0] = total
        out: dict[str, Any] = {"stats": stats, "keys": LATENCY_KEYS, "hist": self.online_hist, "approximate": True,
                               "bin_width": width}
        if self.online_rps is not None:
            out["rps"] = self.online_rps.to(torch.float32)
        return out

    def save_summary(self, path: str, *, hist_bins: int = 256, hist_max: float | None = None,
                     series: bool = True) -> dict[str, np.ndarray]:
        """Columnar dump of the sweep: one row per scenario with its seed, parameter
        columns, counts, flags, the 8 latency statistics, the 1-s RPS series, a latency histogram
        and the mean / maximum of every sampled series.  ``.npz`` (numpy) or ``.parquet`` (pyarrow;
        array-valued columns become list columns).  Returns the columns."""
        summ_kwargs: dict[str, Any] = {"rps": True, "series": series and self._samples_t is not None}
        stats0 = None
        if hist_bins:
            if hist_max is None:      # 1.25 x the largest latency of the sweep
                stats0 = self.summary(rps=False)["stats"].cpu().numpy()
                mx = np.nanmax(stats0[:, 7]) if np.isfinite(stats0[:, 7]).any() else 1.0
                hist_max = float(mx) * 1.25 or 1.0
            summ_kwargs.update(hist_bins=hist_bins, hist_max=hist_max)
        summ = self.summary(**summ_kwargs)
        cols: dict[str, np.ndarray] = {"seed": np.asarray(self.seeds, dtype=np.uint64)}
        for k, v in self.overrides.items():
            cols[f"param:{k}"] = np.asarray(v, dtype=np.float64)
        for name, slot in (("generated", _abi.CNT_GENERATED), ("completed", _abi.CNT_COMPLETED),
                           ("dropped", _abi.CNT_DROPPED), ("request_events", _abi.CNT_EVENTS),
                           ("ticks", _abi.CNT_TICKS), ("flags", _abi.CNT_FLAGS)):
            # (counts[CNT_MAX_LIVE] is a diagnostic -- the next-event kernels' high-water mark of live requests; the stage-parallel
            # kernel writes 0, or for general servers its rounds solved at once << 16 | walked event by event, each half
            # saturating at 65 535 -- and is not part of the on-disk summary: one sweep may mix both paths)
            cols[name] = self.counts[:, slot].copy()
        stats = summ["stats"].cpu().numpy()
        for j, k in enumerate(LATENCY_KEYS):
            cols[f"latency:{k}"] = stats[:, j].copy()
        if "rps" in summ:
            cols["rps"] = summ["rps"].cpu().numpy()
        if "hist" in summ:
            cols["latency_hist"] = summ["hist"].cpu().numpy().view(np.uint32)
            cols["latency_hist_edges"] = np.linspace(0.0, float(hist_max), hist_bins + 1)
        if "series_mean" in summ:
            cols["series_mean"] = summ["series_mean"].cpu().numpy()
            cols["series_max"] = self.decode_series_max(summ["series_max"].cpu().numpy())
            cols["series_names"] = np.asarray(self.series_names())
        _write_columns(str(path), cols, len(self))
        return cols

    def decode_series_max(self, words: np.ndarray) -> np.ndarray:
        """``series_max`` words [n, n_series] -> float64 values (counts as they are, the ram_in_use
        columns decoded from their float32 bits)."""
        w = np.ascontiguousarray(words).view(np.uint32)
        out = w.astype(np.float64)
        j = np.arange(w.shape[1])
        ram = (j >= self.plan.n_edges) & ((j - self.plan.n_edges) % 3 == 2)
        out[:, ram] = w[:, ram].view(np.float32).astype(np.float64)
        return out

    def series_names(self) -> list[str]:
        """Names of the sampled series in device order: edges, then ready/io/ram per server."""
        return series_names_of(self.plan)

    def aggregate(self, level: float = 0.95, by: Any = None) -> dict[str, Any]:
        """Monte-Carlo aggregation over the scenarios of the sweep (the reference's roadmap
        item, ROADMAP.md:23-29): mean, standard deviation and normal-approximation confidence
        half-width of every latency statistic, plus the mean RPS band (5th/95th percentile
        across scenarios per 1-s window).  That is one band over the WHOLE batch: right for
        replicas of one point.  ``by`` (a :class:`~asyncflow_amd.sweep.Sweep` or group ids, see
        :func:`resolve_groups`) aggregates per group instead: :func:`aggregate_by_group`."""
        if by is None:
            return aggregate_summary(self.summary(rps=True), level)
        self._require_clock()
        ids, n_groups = resolve_groups(by, len(self))
        out = aggregate_by_group(self.summary(rps=True), ids, n_groups, level)
        out["pooled"] = self.pooled_summary(ids)["stats"].cpu().numpy()
        return out

    def _require_clock(self) -> None:
        if self._clock_t is None:
            msg = "run(collect_clock=False) kept no rqs_clock (pass online_summary=... to keep a kernel-side summary)"
            raise RuntimeError(msg)

    def pooled_summary(self, by: Any = None) -> dict[str, Any]:
        """The eight latency statistics of every GROUP of scenarios, all its latencies taken as ONE sample (a grid
        point's replicas pooled: what one long reference run estimates), computed by the HIP pooled analyzer
        (``af_engine_summarize_pooled``), bit-equal to numpy's on the concatenated latencies of the group's scenarios in
        ascending scenario order.  ``by``: a ``Sweep`` (its ``point``), integer group ids [n] (negative = left out), or
        None (one group).  Returns ``stats`` float64 [G, 8] on the run's device (LATENCY_KEYS order; a group without
        completions: total 0, the rest NaN), ``keys``, ``replicas`` [G] (scenarios per group) and ``pooled_ms``."""
        import torch

        from .engine import Engine

        self._require_clock()
        ids, n_groups = resolve_groups(by, len(self))
        clock = self._clock_t
        dev = clock.device
        stats = torch.empty((n_groups, 8), dtype=torch.float64, device=dev)
        grp = torch.from_numpy(np.where(ids < 0, _abi.POOL_SKIP, ids).astype(np.uint32).view(np.int32)).to(dev)
        torch.cuda.synchronize(dev)
        if self._summ_engine is None:
            self._summ_engine = Engine(self.plan, dev.index if dev.index is not None else torch.cuda.current_device())
        ms = self._summ_engine.summarize_pooled(len(self), n_groups, clock_ptr=clock.data_ptr(),
                                                clock_capacity=int(clock.shape[1]), counts_ptr=self._counts_t.data_ptr(),
                                                stats_ptr=stats.data_ptr(), group_ptr=grp.data_ptr())
        replicas = np.bincount(ids[ids >= 0], minlength=n_groups)
        return {"stats": stats, "keys": LATENCY_KEYS, "replicas": replicas, "pooled_ms": ms}

    def save_point_summary(self, path: str, by: Any, *, level: float = 0.95) -> dict[str, np.ndarray]:
        """Columnar dump with one row per group (grid point): ``param:<axis>`` (for a Sweep), ``replicas``,
        ``pooled:<key>`` (the pooled statistics), ``mean:<key>`` / ``ci_halfwidth:<key>`` (over the group's replicas,
        as :meth:`aggregate`) and the RPS bands ``rps_mean`` / ``rps_p05`` / ``rps_p95`` [G, floor(T)].  ``.npz`` or
        ``.parquet`` like :meth:`save_summary`; :func:`load_summary` reads it back.  Returns the columns."""
        agg = self.aggregate(level, by=by)
        n_groups = int(agg["replicas"].shape[0])
        cols: dict[str, np.ndarray] = {}
        if hasattr(by, "point_columns"):
            for k, v in by.point_columns().items():
                cols[f"param:{k}"] = np.asarray(v, dtype=np.float64)
        cols["replicas"] = np.asarray(agg["replicas"], dtype=np.int64)
        for j, k in enumerate(LATENCY_KEYS):
            cols[f"pooled:{k}"] = agg["pooled"][:, j].copy()
            cols[f"mean:{k}"] = agg["mean"][:, j].copy()
            cols[f"ci_halfwidth:{k}"] = agg["ci_halfwidth"][:, j].copy()
        for k in ("rps_mean", "rps_p05", "rps_p95"):
            if k in agg:
                cols[k] = agg[k]
        _write_columns(str(path), cols, n_groups)
        return cols

    def _window_groups(self, by: Any) -> tuple[np.ndarray, int]:
        if isinstance(by, str):
            if by != "scenario":
                msg = f"by must be None, a Sweep, integer group ids or 'scenario', not {by!r}"
                raise ValueError(msg)
            return np.arange(len(self), dtype=np.int64), len(self)
        return resolve_groups(by, len(self))

    def window_summary(self, window_s: float | None = None, *, edges: Any = None, by: Any = None,
                       row_bounds: bool = False, window_of: str = "finish") -> dict[str, Any]:
        """The eight latency statistics of every (group, time window): the requests that FINISHED in the window
        (``edges[w] < finish <= edges[w + 1]``), over all scenarios of the group taken as one sample -- p95 during an
        outage, how fast it recovers.  Computed by the HIP windowed analyzer (``af_engine_summarize_windows``), bit-equal
        to :func:`latency_window_stats` / numpy on the concatenated latencies.  Windows: ``window_s`` seconds
        (:func:`window_edges`; default 1 s) or explicit ``edges``.  ``by`` as in :meth:`pooled_summary`, or
        ``"scenario"`` (every scenario its own group).  Returns ``stats`` float64 [G, W, 8] on the run's device (an empty
        window: total 0, the rest NaN), ``edges`` [W + 1], ``keys``, ``replicas`` [G], ``window_ms``, ``scratch_bytes``
        and, with ``row_bounds=True``, ``row_bounds`` int32 [n, W + 1] (the windows' row ranges).

        ``window_of="arrival"``: the requests that were SENT in the window (``edges[w] < start <= edges[w + 1]``), the
        cohort an objective is written against -- by finish time the slow requests of an outage are charged to the
        recovery.  ``af_engine_summarize_arrival_windows``, bit-equal to :func:`latency_window_stats` with that keyword;
        ``row_bounds`` are then cumulative arrival counts, not row ranges.  The cohorts are right-censored: a request that
        had not completed when the run ended, or was dropped, is in no row, so ``total`` is the cohort's completions and
        the last windows of a run under-report slow requests.  The returned dict carries ``window_of``."""
        import torch

        from .engine import Engine

        self._require_clock()
        check_window_of(window_of)
        e = _resolve_edges(window_s, edges, self.plan.total_time)
        ids, n_groups = self._window_groups(by)
        n_win = int(e.shape[0] - 1)
        clock = self._clock_t
        dev = clock.device
        stats = torch.empty((n_groups, n_win, 8), dtype=torch.float64, device=dev)
        grp = torch.from_numpy(np.where(ids < 0, _abi.POOL_SKIP, ids).astype(np.uint32).view(np.int32)).to(dev)
        rb = torch.empty((len(self), n_win + 1), dtype=torch.int32, device=dev) if row_bounds else None
        torch.cuda.synchronize(dev)
        if self._summ_engine is None:
            self._summ_engine = Engine(self.plan, dev.index if dev.index is not None else torch.cuda.current_device())
        ms, scratch = self._summ_engine.summarize_windows(
            len(self), n_groups, e, clock_ptr=clock.data_ptr(), clock_capacity=int(clock.shape[1]),
            counts_ptr=self._counts_t.data_ptr(), stats_ptr=stats.data_ptr(), group_ptr=grp.data_ptr(),
            row_bounds_ptr=rb.data_ptr() if rb is not None else 0, window_of=window_of)
        out: dict[str, Any] = {"stats": stats, "edges": e, "keys": LATENCY_KEYS, "window_of": window_of,
                               "replicas": np.bincount(ids[ids >= 0], minlength=n_groups), "window_ms": ms, "scratch_bytes": scratch}
        if rb is not None:
            out["row_bounds"] = rb
        return out

    def window_bands(self, window_s: float | None = None, *, edges: Any = None, by: Any = None, level: float = 0.95,
                     q: tuple[float, float] = (0.05, 0.95), window_of: str = "finish") -> dict[str, Any]:
        """Bands over the replicas of the windowed latency statistics (the reference's roadmap: "confidence intervals and
        bands over time series").  Every scenario's own window statistics (``window_summary(by="scenario")``), then per
        group (``by``) and window, over the group's replicas whose window is not empty (``n`` [G, W] of them): ``mean``,
        unbiased ``std``, normal confidence half-width ``ci_halfwidth`` at ``level`` and the linear quantiles ``q_lo`` /
        ``q_hi`` (``q``) of each of the eight statistics, numpy float64 [G, W, 8] each (NaN where no replica has a
        completion in the window; ``std`` NaN below two).  The same bits in every run (:func:`window_bands_by_group`); ``pooled`` is
        ``window_summary(by=by)["stats"]`` as numpy.  ``window_of`` as in :meth:`window_summary`, for both."""
        e = _resolve_edges(window_s, edges, self.plan.total_time)
        ids, n_groups = self._window_groups(by)
        per = self.window_summary(edges=e, by="scenario", window_of=window_of)["stats"]
        out = window_bands_by_group(per, ids, n_groups, level, q)
        pooled = self.window_summary(edges=e, by=ids, window_of=window_of)
        out["pooled"] = pooled["stats"].cpu().numpy()[:n_groups]
        out["edges"] = e
        out["window_of"] = window_of
        return out

    def save_window_summary(self, path: str, by: Any = None, *, window_s: float | None = None, edges: Any = None,
                            level: float = 0.95, window_of: str = "finish") -> dict[str, np.ndarray]:
        """Columnar dump of the windowed statistics with one row per group (grid point): ``param:<axis>`` (for a Sweep),
        ``replicas``, and per latency key the [G, W] columns ``window_pooled:<key>`` (the group's replicas pooled),
        ``window_mean:<key>``, ``window_q05:<key>`` and ``window_q95:<key>`` (over the replicas, :meth:`window_bands`);
        ``window_edges`` [W + 1] and ``window_of`` (``"finish"`` or ``"arrival"``, as in :meth:`window_summary`) are
        per-file values.  ``.npz`` or ``.parquet``; :func:`load_summary` reads it back."""
        bands = self.window_bands(window_s, edges=edges, by=by, level=level, q=(0.05, 0.95), window_of=window_of)
        n_groups = int(bands["replicas"].shape[0])
        cols: dict[str, np.ndarray] = {}
        if hasattr(by, "point_columns"):
            for k, v in by.point_columns().items():
                cols[f"param:{k}"] = np.asarray(v, dtype=np.float64)
        cols["replicas"] = np.asarray(bands["replicas"], dtype=np.int64)
        for j, k in enumerate(LATENCY_KEYS):
            cols[f"window_pooled:{k}"] = np.ascontiguousarray(bands["pooled"][:, :, j])
            cols[f"window_mean:{k}"] = np.ascontiguousarray(bands["mean"][:, :, j])
            cols[f"window_q05:{k}"] = np.ascontiguousarray(bands["q_lo"][:, :, j])
            cols[f"window_q95:{k}"] = np.ascontiguousarray(bands["q_hi"][:, :, j])
        cols["window_edges"] = np.asarray(bands["edges"], dtype=np.float64)
        cols["window_of"] = np.asarray(window_of)
        _write_columns(str(path), cols, n_groups)
        return cols

    # ---- arrivals per window: the offered load and what became of each cohort ------------------------------------
    #: the sweep keys that change a scenario's arrival times, and their engine columns
    GENERATOR_COLUMNS = {"rqs_input.avg_active_users.mean": "gen_users_mean", "rqs_input.avg_active_users.variance": "gen_users_sigma",
                         "rqs_input.avg_request_per_minute_per_user.mean": "gen_rpm_mean",
                         "rqs_input.user_sampling_window": "gen_window"}

    def _arrival_sweep(self, rows: Any = None) -> tuple[np.ndarray, list[tuple[int, int, np.ndarray]], int]:
        """Seeds, generator columns and draw capacity of the run (of its scenarios ``rows``)."""
        pick = slice(None) if rows is None else rows
        cols = [(_abi.PARAM_CODES[name], 0, np.ascontiguousarray(np.asarray(self.overrides[key], dtype=np.float64)[pick]))
                for key, name in self.GENERATOR_COLUMNS.items() if key in self.overrides]
        cap = self.draw_capacity or (int(self._clock_t.shape[1]) if self._clock_t is not None else 0)
        if cap <= 0:
            msg = "the run's draw capacity is not known (BatchedResults(draw_capacity=...))"
            raise ValueError(msg)
        return np.ascontiguousarray(np.asarray(self.seeds, dtype=np.uint64)[pick]), cols, cap

    def _arrival_engine(self) -> tuple[Any, Any]:
        import torch

        from .engine import Engine

        dev = self._counts_t.device
        torch.cuda.synchronize(dev)
        if self._summ_engine is None:
            self._summ_engine = Engine(self.plan, dev.index if dev.index is not None else torch.cuda.current_device())
        return self._summ_engine, dev

    def arrival_times(self, i: int) -> np.ndarray:
        """The arrival times of scenario ``i``, float64 [generated], ascending: regenerated on the device from its seed
        and generator parameters (``af_engine_summarize_arrivals`` with a ``times`` buffer), bit-equal to what the run
        consumed and to :func:`arrival_times`.  Every ``start`` of the scenario's ``rqs_clock`` is one of them."""
        import torch

        i = int(i)
        if not 0 <= i < len(self):
            raise IndexError(i)
        seeds, cols, cap = self._arrival_sweep(slice(i, i + 1))
        eng, dev = self._arrival_engine()
        times = torch.empty((1, cap), dtype=torch.float64, device=dev)
        arr = torch.empty((1, 1), dtype=torch.int64, device=dev)
        eng.summarize_arrivals(seeds, cols, 1, np.asarray([0.0, max(float(self.plan.total_time), 1.0)]), draw_capacity=cap,
                               arrivals_ptr=arr.data_ptr(), times_ptr=times.data_ptr())
        t = times[0].cpu().numpy()
        return t[np.isfinite(t)]

    def arrival_summary(self, window_s: float | None = None, *, edges: Any = None, by: Any = None,
                        thresholds: Any = None) -> dict[str, Any]:
        """Arrivals per (group, time window), and what became of each window's cohort: the offered load, the share of the
        requests SENT in a window that ever came back, and SLO shares with the ARRIVALS as the denominator -- the
        by-arrival windows of :meth:`window_summary` / :meth:`quantile_summary` only see completions.  The arrival times are
        regenerated on the device from the run's seeds, generator columns and draw capacity
        (``af_engine_summarize_arrivals``: no simulation kernel runs) and counted in exact integers, equal to
        :func:`arrival_window_counts` on :func:`arrival_times`.  Windows and ``by`` as in :meth:`window_summary`.
        Returns, as numpy: ``edges`` [W + 1]; ``arrivals`` uint64 [G, W] (``edges[w] < t <= edges[w + 1]``);
        ``offered_rps`` = arrivals / (members * window width); ``completed`` int64 [G, W], the by-arrival count of the same
        cells (``af_engine_summarize_arrival_windows`` / ``_quantiles``); ``lost`` = arrivals - completed: the requests
        that were DROPPED on an edge OR WERE STILL IN FLIGHT when the run ended -- the two are not told apart (drops per
        window would need the simulation kernel to record them), so the last windows of a run always lose their slow
        requests; ``completion_share`` = completed / arrivals (NaN without arrivals); with ``thresholds`` (seconds):
        ``within`` int64 [G, W, T], the completions within each threshold, and ``within_share`` = within / arrivals;
        ``truncated`` bool [G]: a member's arrival row was full (``FLAG_DRAW_OVERFLOW``) or its clock rows were cut, so its
        counts are lower bounds; ``generated`` [n], ``flags`` [n], ``replicas`` [G], ``arrival_ms``.  Raises when a cell
        of a group that is not truncated holds more completions than arrivals."""
        import torch

        self._require_clock()
        e = _resolve_edges(window_s, edges, self.plan.total_time)
        ids, n_groups = self._window_groups(by)
        n, n_win = len(self), int(e.shape[0] - 1)
        th = check_slo_thresholds(thresholds)
        seeds, cols, cap = self._arrival_sweep()
        eng, dev = self._arrival_engine()
        arr = torch.empty((n_groups, n_win), dtype=torch.int64, device=dev)
        gen = torch.empty(n, dtype=torch.int32, device=dev)
        flg = torch.empty(n, dtype=torch.int32, device=dev)
        grp = torch.from_numpy(np.where(ids < 0, _abi.POOL_SKIP, ids).astype(np.uint32).view(np.int32)).to(dev)
        ms, _scratch = eng.summarize_arrivals(seeds, cols, n_groups, e, draw_capacity=cap, arrivals_ptr=arr.data_ptr(),
                                              group_ptr=grp.data_ptr(), generated_ptr=gen.data_ptr(), flags_ptr=flg.data_ptr())
        arrivals = arr.cpu().numpy().view(np.uint64)
        generated = gen.cpu().numpy().view(np.uint32)
        flags = flg.cpu().numpy().view(np.uint32)
        out: dict[str, Any] = {"edges": e, "arrivals": arrivals, "generated": generated, "flags": flags, "arrival_ms": ms,
                               "replicas": np.bincount(ids[ids >= 0], minlength=n_groups)}
        if th.shape[0]:
            qs = self.quantile_summary([], thresholds=th, edges=e, by=ids, window_of="arrival")
            completed = qs["count"].cpu().numpy().astype(np.int64)
            out["within"] = qs["within"].cpu().numpy().astype(np.int64)
            out["thresholds"] = th
        else:
            completed = self.window_summary(edges=e, by=ids, window_of="arrival")["stats"][:, :, 0].cpu().numpy().astype(np.int64)
        completed = completed[:n_groups]
        cut = ((flags & _abi.FLAG_DRAW_OVERFLOW) != 0) | (self.counts[:, _abi.CNT_COMPLETED] > int(self._clock_t.shape[1]))
        truncated = np.zeros(n_groups, dtype=bool)
        truncated[ids[(ids >= 0) & cut]] = True
        a = arrivals.astype(np.int64)
        bad = (completed > a) & ~truncated[:, None]
        if bad.any():
            g, w = (int(v[0]) for v in np.nonzero(bad))
            msg = (f"group {g}, window {w}: {int(completed[g, w])} completions of {int(a[g, w])} arrivals -- the arrival times "
                   "regenerated are not the ones the run simulated (draw_capacity, seeds or generator columns differ)")
            raise RuntimeError(msg)
        width = np.diff(e)[None, :] * np.maximum(out["replicas"], 1)[:, None]
        some = a > 0
        out["offered_rps"] = a / width
        out["completed"] = completed
        out["lost"] = a - completed
        out["completion_share"] = np.where(some, completed / np.maximum(a, 1), np.nan)
        if th.shape[0]:
            out["within"] = out["within"][:n_groups]
            out["within_share"] = np.where(some[:, :, None], out["within"] / np.maximum(a, 1)[:, :, None], np.nan)
        out["truncated"] = truncated
        return out

    def arrival_bands(self, window_s: float | None = None, *, edges: Any = None, by: Any = None, level: float = 0.95,
                      q: tuple[float, float] = (0.05, 0.95)) -> dict[str, Any]:
        """Bands over the replicas of the offered load and the completion share: every scenario's own
        ``offered_rps`` and ``completion_share`` (``arrival_summary(by="scenario")``), then per group (``by``) and window,
        over the group's replicas with an arrival in the window (``n`` [G, W] of them), ``mean``, ``std``,
        ``ci_halfwidth`` (at ``level``) and the linear quantiles ``q_lo`` / ``q_hi`` (``q``) as
        :func:`window_bands_by_group` gives them: numpy float64 [G, W, 2], column 0 the offered load, 1 the share
        (``keys``).  ``pooled`` is ``arrival_summary(by=by)``."""
        import torch

        e = _resolve_edges(window_s, edges, self.plan.total_time)
        ids, n_groups = self._window_groups(by)
        per = self.arrival_summary(edges=e, by="scenario")
        dev = self._counts_t.device
        body = torch.from_numpy(np.stack([per["offered_rps"], np.nan_to_num(per["completion_share"])], axis=2)).to(dev)
        out = window_bands_by_group(body, ids, n_groups, level, q, valid=torch.from_numpy(per["arrivals"].astype(np.int64) > 0).to(dev))
        out["keys"] = ("offered_rps", "completion_share")
        out["pooled"] = self.arrival_summary(edges=e, by=ids)
        out["edges"] = e
        return out

    def save_arrival_summary(self, path: str, by: Any = None, *, window_s: float | None = None, edges: Any = None,
                             thresholds: Any = None, level: float = 0.95) -> dict[str, np.ndarray]:
        """Columnar dump of the arrivals with one row per group (grid point): ``param:<axis>`` (for a Sweep), ``replicas``,
        ``truncated`` and the [G, W] columns ``arrivals``, ``offered_rps``, ``completed``, ``lost``, ``completion_share``
        (the group's replicas pooled, :meth:`arrival_summary`), ``offered_rps_mean`` / ``_q05`` / ``_q95`` and
        ``completion_share_mean`` / ``_q05`` / ``_q95`` (over the replicas, :meth:`arrival_bands`) and, per threshold j,
        ``within:<j>`` and ``within_share:<j>``; ``window_edges`` [W + 1] and ``slo_thresholds`` [T] are per-file values.
        ``.npz`` or ``.parquet``; :func:`load_summary` reads it back."""
        bands = self.arrival_bands(window_s, edges=edges, by=by, level=level, q=(0.05, 0.95))
        pooled = bands["pooled"] if thresholds is None else self.arrival_summary(edges=bands["edges"], by=by, thresholds=thresholds)
        n_groups = int(bands["replicas"].shape[0])
        cols: dict[str, np.ndarray] = {}
        if hasattr(by, "point_columns"):
            for k, v in by.point_columns().items():
                cols[f"param:{k}"] = np.asarray(v, dtype=np.float64)
        cols["replicas"] = np.asarray(bands["replicas"], dtype=np.int64)
        cols["truncated"] = np.asarray(pooled["truncated"], dtype=bool)
        cols["arrivals"] = pooled["arrivals"].astype(np.int64)
        for k in ("offered_rps", "completed", "lost", "completion_share"):
            cols[k] = np.ascontiguousarray(pooled[k])
        for j, k in enumerate(bands["keys"]):
            cols[f"{k}_mean"] = np.ascontiguousarray(bands["mean"][:, :, j])
            cols[f"{k}_q05"] = np.ascontiguousarray(bands["q_lo"][:, :, j])
            cols[f"{k}_q95"] = np.ascontiguousarray(bands["q_hi"][:, :, j])
        for j in range(int(pooled["within"].shape[2]) if "within" in pooled else 0):
            cols[f"within:{j}"] = np.ascontiguousarray(pooled["within"][:, :, j])
            cols[f"within_share:{j}"] = np.ascontiguousarray(pooled["within_share"][:, :, j])
        cols["window_edges"] = np.asarray(bands["edges"], dtype=np.float64)
        cols["slo_thresholds"] = np.asarray(pooled.get("thresholds", np.zeros(0)), dtype=np.float64)
        _write_columns(str(path), cols, n_groups)
        return cols

    # ---- requests in flight end to end: L of Little's law ---------------------------------------------------------
    def _in_flight_ticks(self) -> int:
        """The tick capacity of the run's sample rows (without samples: the plan's tick count)."""
        return int(self._samples_t.shape[1]) if self._samples_t is not None else max(int(self.plan.tick_count), 1)

    def _in_flight_call(self, b: np.ndarray, ids: np.ndarray, n_groups: int, threshold: int, bins: int, lo: int) -> dict[str, Any]:
        """One ``af_engine_summarize_inflight`` over resolved tick edges and group ids: the raw outputs on the host."""
        import torch

        self._require_clock()
        thr, n_bins, lo_v = check_in_flight_bins(threshold, bins, lo)
        eng, dev = self._arrival_engine()
        n_win, clock = int(b.shape[0] - 1), self._clock_t
        count, mn, mx, ab, under = (torch.empty((n_groups, n_win), dtype=torch.int32, device=dev) for _ in range(5))
        total = torch.empty((n_groups, n_win), dtype=torch.int64, device=dev)
        hist = torch.empty((n_groups, n_win, n_bins), dtype=torch.int32, device=dev) if n_bins else None
        grp = torch.from_numpy(np.where(ids < 0, _abi.POOL_SKIP, ids).astype(np.uint32).view(np.int32)).to(dev)
        ms, scratch = eng.summarize_inflight(
            len(self), n_groups, b, self.plan.sample_period, clock_ptr=clock.data_ptr(), clock_capacity=int(clock.shape[1]),
            tick_capacity=self._in_flight_ticks(), counts_ptr=self._counts_t.data_ptr(), count_ptr=count.data_ptr(),
            sum_ptr=total.data_ptr(), min_ptr=mn.data_ptr(), max_ptr=mx.data_ptr(), above_ptr=ab.data_ptr(),
            hist_ptr=hist.data_ptr() if hist is not None else 0, under_ptr=under.data_ptr() if hist is not None else 0,
            group_ptr=grp.data_ptr(), threshold=thr, bins=n_bins, lo=lo_v)

        def host(t: Any) -> np.ndarray:
            return t.cpu().numpy().view(np.uint32).astype(np.int64)

        out: dict[str, Any] = {"count": host(count), "sum": total.cpu().numpy().view(np.uint64), "min": host(mn), "max": host(mx),
                               "above": host(ab), "in_flight_ms": ms, "scratch_bytes": scratch}
        if hist is not None:
            out["hist"], out["under"] = host(hist), host(under)
        return out

    def in_flight_summary(self, window_s: float | None = None, *, ticks_per_window: int | None = None, tick_edges: Any = None,
                          by: Any = None, threshold: int = 0, bins: int = 0, lo: int = 0) -> dict[str, Any]:
        """Requests IN FLIGHT end to end per (group, window of ticks): the "in-flight requests" of a dashboard and L of
        Little's law -- what sizes a client's connection pool or a global concurrency limit, and what builds up and drains
        around an injected outage.  No sampled series or combination of them holds it (a request in a server's CPU step or
        between two hops is in none).  Computed from the clock rows by ``af_engine_summarize_inflight``, every word equal to
        :func:`in_flight_window_stats` on :func:`in_flight_series` of the group's scenarios: request i is counted at the
        sample instants ``floor(start / p) <= k < floor(finish / p)``.  Windows and ``by`` as in
        :meth:`series_window_summary` (``window_s`` seconds, default 1 s, ``ticks_per_window`` or ``tick_edges``).
        Returns numpy arrays: ``count`` int64 [G, W] (the sample instants of the cell, over its members); ``sum`` uint64;
        ``mean`` = ``float(sum) / float(count)`` (NaN in an empty cell); ``min`` / ``max`` int64 (0 in an empty cell);
        ``above`` int64 and ``above_share`` = the share of the instants with more than ``threshold`` requests in flight
        (NaN in an empty cell); with ``bins`` > 0 ``hist`` int64 [G, W, 1, bins] (bin b: exactly ``lo + b`` requests; the
        LAST bin also holds everything above it, so choose ``bins > max - lo`` for exact quantiles), ``under`` [G, W, 1],
        ``bin_edges`` [1, bins + 1] and ``ram`` -- the layout :func:`series_histogram_quantiles` reads exact quantiles off;
        and ``series`` (``["in_flight"]``), ``tick_edges``, ``times`` (the windows' start labels in seconds), ``replicas``
        [G], ``in_flight_ms``, ``scratch_bytes``.
        COMPLETED requests only: a dropped request and one still in flight when the run ended are in no clock row, so the
        last seconds of a run under-count as the by-arrival cohorts do; ``lost`` of :meth:`arrival_summary` sizes it."""
        b = self._series_tick_edges(window_s, ticks_per_window, tick_edges)
        ids, n_groups = self._window_groups(by)
        out = self._in_flight_call(b, ids, n_groups, threshold, bins, lo)
        some = out["count"] > 0
        cnt = np.maximum(out["count"], 1).astype(np.float64)
        out["mean"] = np.where(some, out["sum"].astype(np.float64) / cnt, np.nan)
        out["above_share"] = np.where(some, out["above"].astype(np.float64) / cnt, np.nan)
        if "hist" in out:
            n_bins = int(out["hist"].shape[2])
            out["hist"], out["under"] = out["hist"][:, :, None, :], out["under"][:, :, None]
            out["bin_edges"] = (float(lo) + np.arange(n_bins + 1, dtype=np.float64))[None, :]
            out["ram"] = np.zeros(1, dtype=bool)
        out.update(series=["in_flight"], threshold=int(threshold), tick_edges=b, times=b[:-1].astype(np.float64) * self.plan.sample_period,
                   replicas=np.bincount(ids[ids >= 0], minlength=n_groups))
        return out

    def in_flight_bands(self, window_s: float | None = None, *, ticks_per_window: int | None = None, tick_edges: Any = None,
                        by: Any = None, threshold: int = 0, of: str = "mean", level: float = 0.95,
                        q: tuple[float, float] = (0.05, 0.95)) -> dict[str, Any]:
        """Bands over the replicas of a windowed in-flight statistic ``of`` (``"mean"``, ``"max"`` or ``"above_share"``), as
        :meth:`series_window_bands` gives them for the sampled series: every scenario's own window values
        (``in_flight_summary(by="scenario")``), then per group (``by``) and window, over the group's replicas whose window
        is not empty (``n`` [G, W] of them), ``mean``, ``std``, ``ci_halfwidth`` (at ``level``) and the linear quantiles
        ``q_lo`` / ``q_hi`` (``q``): numpy float64 [G, W].  ``pooled`` is the grouped call's value of the same statistic."""
        import torch

        if of not in ("mean", "max", "above_share"):
            msg = f"of must be 'mean', 'max' or 'above_share', not {of!r}"
            raise ValueError(msg)
        b = self._series_tick_edges(window_s, ticks_per_window, tick_edges)
        ids, n_groups = self._window_groups(by)
        per = self.in_flight_summary(tick_edges=b, by="scenario", threshold=threshold)
        dev = self._counts_t.device
        body = torch.from_numpy(np.nan_to_num(per[of].astype(np.float64))[:, :, None]).to(dev)
        out = window_bands_by_group(body, ids, n_groups, level, q, valid=torch.from_numpy(per["count"] > 0).to(dev))
        for k in ("mean", "std", "ci_halfwidth", "q_lo", "q_hi"):
            out[k] = out[k][:, :, 0]
        pooled = self.in_flight_summary(tick_edges=b, by=ids, threshold=threshold)
        out["pooled"] = pooled[of][:n_groups].astype(np.float64)
        out.update(of=of, summary=pooled, tick_edges=b, times=per["times"])
        return out

    def save_in_flight_summary(self, path: str, by: Any = None, *, window_s: float | None = None,
                               ticks_per_window: int | None = None, threshold: int = 0, bins: int = 0, lo: int = 0,
                               level: float = 0.95) -> dict[str, np.ndarray]:
        """Columnar dump of the requests in flight with one row per group (grid point): ``param:<axis>`` (for a Sweep),
        ``replicas`` and the [G, W] columns ``in_flight_count``, ``in_flight_mean``, ``in_flight_min``, ``in_flight_max``,
        ``in_flight_above`` (the share above ``threshold``) -- the group's replicas taken together, :meth:`in_flight_summary`
        --, ``in_flight_q05`` / ``in_flight_q95`` (of the replicas' own means, :meth:`in_flight_bands`) and, with ``bins``,
        ``in_flight_hist`` [G, W, bins] and ``in_flight_under``; ``in_flight_tick_edges`` [W + 1], ``in_flight_times`` [W]
        and ``in_flight_binning`` (threshold, lo) are per-file vectors.  ``.npz`` or ``.parquet``; :func:`load_summary`
        reads it back."""
        b = self._series_tick_edges(window_s, ticks_per_window, None)
        bands = self.in_flight_bands(tick_edges=b, by=by, threshold=threshold, level=level, q=(0.05, 0.95))
        pooled = bands["summary"] if not bins else self.in_flight_summary(tick_edges=b, by=by, threshold=threshold, bins=bins, lo=lo)
        n_groups = int(bands["replicas"].shape[0])
        cols: dict[str, np.ndarray] = {}
        if hasattr(by, "point_columns"):
            for k, v in by.point_columns().items():
                cols[f"param:{k}"] = np.asarray(v, dtype=np.float64)
        cols["replicas"] = np.asarray(bands["replicas"], dtype=np.int64)
        for name, key in (("count", "count"), ("mean", "mean"), ("min", "min"), ("max", "max"), ("above", "above_share")):
            cols[f"in_flight_{name}"] = np.ascontiguousarray(pooled[key][:n_groups])
        cols["in_flight_q05"] = np.ascontiguousarray(bands["q_lo"])
        cols["in_flight_q95"] = np.ascontiguousarray(bands["q_hi"])
        if bins:
            cols["in_flight_hist"] = np.ascontiguousarray(pooled["hist"][:n_groups, :, 0, :])
            cols["in_flight_under"] = np.ascontiguousarray(pooled["under"][:n_groups, :, 0])
        cols["in_flight_tick_edges"] = np.asarray(b, dtype=np.float64)
        cols["in_flight_times"] = np.asarray(bands["times"], dtype=np.float64)
        cols["in_flight_binning"] = np.asarray([threshold, lo], dtype=np.float64)
        _write_columns(str(path), cols, n_groups)
        return cols

    def in_flight(self, i: int) -> dict[str, np.ndarray]:
        """The per-tick arrays of scenario ``i``, uint32 [its ticks] each: ``in_flight`` (requests in flight end to end at
        sample instant k), ``started`` and ``finished`` (``in_flight == cumsum(started - finished)``), written by
        ``af_engine_summarize_inflight`` and equal to :func:`in_flight_series` on the scenario's clock rows."""
        import torch

        i = int(i)
        if not 0 <= i < len(self):
            raise IndexError(i)
        self._require_clock()
        eng, dev = self._arrival_engine()
        cap, clock = self._in_flight_ticks(), self._clock_t
        rows = torch.empty((3, cap), dtype=torch.int32, device=dev)   # (rows at or past t_s are not written and not returned)
        count = torch.empty((1, 1), dtype=torch.int32, device=dev)
        total = torch.empty((1, 1), dtype=torch.int64, device=dev)
        eng.summarize_inflight(1, 1, np.asarray([0, cap], dtype=np.uint32), self.plan.sample_period, clock_ptr=clock[i].data_ptr(),
                               clock_capacity=int(clock.shape[1]), tick_capacity=cap, counts_ptr=self._counts_t[i].data_ptr(),
                               count_ptr=count.data_ptr(), sum_ptr=total.data_ptr(), in_flight_ptr=rows[0].data_ptr(),
                               started_ptr=rows[1].data_ptr(), finished_ptr=rows[2].data_ptr())
        t_s = min(int(self.counts[i, _abi.CNT_TICKS]), cap)
        words = rows[:, :t_s].cpu().numpy().view(np.uint32)
        return {"in_flight": words[0].copy(), "started": words[1].copy(), "finished": words[2].copy()}

    def littles_law(self, window_s: float | None = None, *, by: Any = None) -> dict[str, Any]:
        """L, lambda and W of Little's law side by side per (group, window), each from its own exact analyzer -- informational:
        nothing asserts that they agree, and over a window they only do as far as the requests open at its two ends allow.
        Window w is the sample instants ``(k + 1) p`` of its ticks and the arrival cohort ``t0 < start <= t1`` over the same
        span of ``window_s`` seconds (a multiple of the sample period; default 1 s).  Returns numpy float64 [G, W]: ``L``,
        the mean number in flight (:meth:`in_flight_summary`); ``lambda_eff``, the COMPLETIONS of the window's arrival
        cohort per second and replica (``window_summary(window_of="arrival")``: dropped requests and those still in flight at
        the end of the run are in neither side); ``W``, the mean latency of that cohort in seconds (NaN without
        completions); ``ratio`` = ``L / (lambda_eff * W)`` (NaN where that product is 0 or NaN); and ``completed`` int64,
        ``edges`` (seconds) [W + 1], ``tick_edges``, ``replicas`` [G]."""
        b = self._series_tick_edges(window_s, None, None)
        ids, n_groups = self._window_groups(by)
        edges = b.astype(np.float64) * float(self.plan.sample_period)
        inf = self.in_flight_summary(tick_edges=b, by=ids)
        stats = self.window_summary(edges=edges, by=ids, window_of="arrival")["stats"].cpu().numpy()[:n_groups]
        completed = stats[:, :, 0].astype(np.int64)
        width = np.diff(edges)[None, :] * np.maximum(inf["replicas"], 1)[:, None]
        lam = completed / width
        with np.errstate(invalid="ignore", divide="ignore"):
            demand = lam * stats[:, :, 1]
            ratio = np.where(demand > 0.0, inf["mean"][:n_groups] / demand, np.nan)
        return {"L": inf["mean"][:n_groups], "lambda_eff": lam, "W": stats[:, :, 1], "ratio": ratio, "completed": completed,
                "edges": edges, "tick_edges": b, "replicas": inf["replicas"]}

    # ---- burn-rate alert rules per tick over rolling look-backs ---------------------------------------------------
    def _outcome_rows(self, eng: Any, dev: Any) -> tuple[Any, Any, int, int]:
        """The arrival rows of the run on the device, regenerated once per distinct (seed, generator columns) with
        ``af_engine_summarize_arrivals``: ``times`` float64 [rows, draw_capacity], ``time_row`` uint32 [n] (scenarios that were sent
        the same requests share a row), the number of rows and the draw capacity."""
        import torch

        seeds, cols, cap = self._arrival_sweep(None)
        key = np.stack([seeds.view(np.uint64)] + [np.ascontiguousarray(c[2], dtype=np.float64).view(np.uint64) for c in cols], axis=1)
        _, first, time_row = np.unique(key, axis=0, return_index=True, return_inverse=True)
        seeds, cols, cap = self._arrival_sweep(first)
        n_rows = int(first.shape[0])
        times = torch.empty((n_rows, cap), dtype=torch.float64, device=dev)
        arr = torch.empty((n_rows, 1), dtype=torch.int64, device=dev)
        eng.summarize_arrivals(seeds, cols, n_rows, np.asarray([0.0, max(float(self.plan.total_time), 1.0)]),
                               draw_capacity=cap, arrivals_ptr=arr.data_ptr(), times_ptr=times.data_ptr())
        tr = torch.from_numpy(np.ascontiguousarray(time_row.reshape(-1)).astype(np.uint32).view(np.int32)).to(dev)
        return times, tr, n_rows, cap

    def _alert_call(self, b: np.ndarray, ids: np.ndarray, n_groups: int, slo: float, r6: np.ndarray, delay_bins: int,
                    delay_width: int, per_tick: bool, timeout: float | None = None) -> dict[str, Any]:
        """One ``af_engine_summarize_alerts`` -- with ``timeout`` one ``af_engine_outcome_alerts`` -- over resolved tick
        edges, group ids and rules in ticks: the raw outputs on the host, int64 (a tick that does not exist: -1)."""
        import torch

        self._require_clock()
        eng, dev = self._arrival_engine()
        n, n_win, n_rules, clock, cap = len(self), int(b.shape[0] - 1), int(r6.shape[0]), self._clock_t, self._in_flight_ticks()
        t: dict[str, Any] = {"count": torch.empty((n, n_win), dtype=torch.int32, device=dev)}
        for k in ALERT_CELL_KEYS:
            t[k] = torch.empty((n, n_win, n_rules), dtype=torch.int32, device=dev)
        for k in ALERT_GROUP_KEYS:
            t[k] = torch.empty((n_groups, n_win, n_rules), dtype=torch.int64 if k.startswith("fire_") else torch.int32, device=dev)
        if delay_bins:
            t["delay_hist"] = torch.empty((n_groups, n_win, n_rules, delay_bins), dtype=torch.int32, device=dev)
        if per_tick:
            for k in ("total", "bad", "firing"):
                t[k] = torch.zeros((n, cap), dtype=torch.int32, device=dev)   # (rows at or past t_s are not written)
        grp = torch.from_numpy(np.where(ids < 0, _abi.POOL_SKIP, ids).astype(np.uint32).view(np.int32)).to(dev)
        oc: dict[str, Any] | None = None
        extra: dict[str, Any] = {}
        if timeout is not None:
            times, tr, n_rows, draw_cap = self._outcome_rows(eng, dev)
            extra = {k: torch.empty((n,), dtype=torch.int32, device=dev) for k in ("timed_out", "deficit", "flags")}
            if per_tick:
                extra["timeouts"] = torch.zeros((n, cap), dtype=torch.int32, device=dev)
            oc = {"times_ptr": times.data_ptr(), "time_row_ptr": tr.data_ptr(), "n_time_rows": n_rows, "draw_capacity": draw_cap,
                  "timeout": float(timeout), **{k: v.data_ptr() for k, v in extra.items()}}
        torch.cuda.synchronize(dev)
        ms, scratch = eng.summarize_alerts(
            n, n_groups, b, self.plan.sample_period, slo, r6, clock_ptr=clock.data_ptr(), clock_capacity=int(clock.shape[1]),
            tick_capacity=cap, counts_ptr=self._counts_t.data_ptr(), group_ptr=grp.data_ptr(), delay_bins=delay_bins,
            delay_width=delay_width, ptrs={k: v.data_ptr() for k, v in t.items()}, outcomes=oc)
        out: dict[str, Any] = {}
        for k, v in {**t, **extra}.items():
            a = v.cpu().numpy()
            if a.dtype == np.int32 and k not in ("longest_start", "first", "last"):
                a = a.view(np.uint32)
            out[k] = a.astype(np.int64) if k != "firing" else a                # (0xFFFFFFFF is -1; a tick is below 2^31)
        if timeout is not None:
            cut = np.flatnonzero(out["flags"] & _abi.OUTCOME_ROWS_TRUNCATED)
            if cut.shape[0]:
                msg = (f"scenario {int(cut[0])} completed more requests than the clock rows hold: the missing rows would be counted as "
                       "timeouts (run with a larger clock capacity)")
                raise ValueError(msg)
        out.update(alerts_ms=ms, scratch_bytes=scratch)
        return out

    def alert_summary(self, slo_s: float, rules: Any, window_s: float | None = None, *, ticks_per_window: int | None = None,
                      tick_edges: Any = None, by: Any = None, delay_bins: int = 0, delay_width_s: float | None = None,
                      per_tick: bool = False, timeout_s: float | None = None) -> dict[str, Any]:
        """WOULD MY ALERT HAVE FIRED: burn-rate alert rules evaluated at every tick over ROLLING look-backs of the completions,
        as a monitoring system evaluates them at every scrape -- during an injected outage, how many seconds after it began
        (the detection delay, as a distribution over the replicas of a grid point), under plain load (a false alarm), for how
        long and how often (flapping).  The tumbling windows of the other analyzers cannot say.  Computed from the clock rows
        by ``af_engine_summarize_alerts``, every word equal to :func:`completion_ticks`, :func:`alert_firing`,
        :func:`alert_window_stats` and :func:`alert_cells`.

        ``slo_s``: a request is bad when its latency is above it (``inf``: none is).  ``rules``: up to 32 of
        :func:`alert_rule` (seconds, converted against the plan's sample period; ValueError where a duration is no multiple
        of it) or of six whole numbers in ticks.  Windows and ``by`` as in :meth:`in_flight_summary`; they choose where firing is
        REPORTED, never what a rule sees -- a look-back reaches across window edges.  Put a window edge at an event's tick and
        ``delay_hist`` of that window is the detection-delay distribution of each grid point's replicas (``delay_bins`` bins
        of ``delay_width_s`` seconds, default one tick; the last bin takes every longer delay).

        Returns numpy arrays.  Per replica, int64: ``count`` [n, W]; ``fired`` (firing ticks), ``episodes`` (maximal runs of
        firing ticks, clipped at the window's edges), ``longest``, ``longest_start``, ``first``, ``last`` (tick indices, -1:
        none; ``last == hi - 1``: still firing at the window's end) [n, W, R]; float64 ``first_s`` (tick k at ``k *
        sample_period``, NaN: none), ``longest_s``, ``fired_s``.  Per group, int64 [G, W, R]: ``members``, ``fired_members``,
        ``open_members``, ``fire_ticks``, ``fire_episodes``; ``fired_share`` = ``fired_members / members`` (NaN where empty);
        with ``delay_bins`` ``delay_hist`` [G, W, R, delay_bins] and ``delay_edges_s`` (:func:`alert_delay_quantiles` reads
        brackets off them).  ``per_tick=True`` adds ``total``, ``bad`` int64 and ``firing`` uint32 (bit r: rule r fires) [n,
        tick capacity], 0 at and past a scenario's ticks.  And ``rules`` (echoed as ticks and fractions), ``rule_ticks`` [R, 6],
        ``slo_s``, ``tick_edges``, ``times``, ``replicas`` [G], ``alerts_ms``, ``scratch_bytes``.
        Without ``timeout_s`` COMPLETED requests only: a dropped request and one still in flight when the run ended are in no
        clock row, and the last ticks of a run see fewer completions.

        ``timeout_s`` (seconds, finite and > 0) is the CLIENT TIMEOUT that makes drops alertable: a request sent at ``a`` without
        an answer by ``a + timeout_s`` is an error at ``a + timeout_s``, so every arrival produces exactly one event, the bad
        share has the arrivals as its denominator, and ``slo_s=inf`` is a pure availability alert
        (``af_engine_outcome_alerts``; every word equal to :func:`outcome_ticks` and the functions above).  The arrival
        rows are regenerated on the device once per distinct (seed, generator columns); nothing is simulated.  The summary gains
        ``timed_out`` and ``deficit`` int64 [n] (``deficit`` is 0 for a run's own rows), ``flags`` [n], ``timeout_s`` and, with
        ``per_tick``, ``timeouts`` [n, tick capacity]; ``total`` / ``bad`` are then completions in time plus timeouts.
        ValueError names the first scenario whose clock rows were cut: its missing rows would count as timeouts."""
        period = float(self.plan.sample_period)
        slo = float(slo_s)
        if math.isnan(slo):
            msg = "slo_s must not be NaN"
            raise ValueError(msg)
        tau = None if timeout_s is None else check_timeout(timeout_s)
        r6 = check_alert_rules(rules, period)
        n_bins, width = _alert_delay_bins(delay_bins, delay_width_s, period)
        b = self._series_tick_edges(window_s, ticks_per_window, tick_edges)
        ids, n_groups = self._window_groups(by)
        out = self._alert_call(b, ids, n_groups, slo, r6, n_bins, width, bool(per_tick), tau)
        if tau is not None:
            out["timeout_s"] = tau
        return _finish_alert_summary(out, r6, b, ids, n_groups, period, slo, n_bins, width)

    def save_alert_summary(self, path: str, slo_s: float, rules: Any, by: Any = None, **kw: Any) -> dict[str, np.ndarray]:
        """Columnar dump of :meth:`alert_summary` (same keywords) with one row per group (grid point): ``param:<axis>`` (for a
        Sweep), ``replicas`` and the [G, W, R] columns ``alert_members``, ``alert_fired_members``, ``alert_open_members``,
        ``alert_fire_ticks``, ``alert_fire_episodes``, ``alert_fired_share`` and, with ``delay_bins``, ``alert_delay_hist`` [G,
        W, R, bins] with ``alert_delay_edges_s``; ``alert_rule_ticks`` (R x 6, flat), ``alert_slo_s``, ``alert_tick_edges`` and
        ``alert_times`` (with ``timeout_s`` also ``alert_timeout_s``) are per-file vectors.  ``.npz`` or ``.parquet``; :func:`load_summary` reads it back."""
        kw.pop("per_tick", None)
        return _save_alert_summary(self.alert_summary(slo_s, rules, by=by, **kw), str(path), by)

    # ---- the slowest requests per window and group, with their identity -------------------------------------------
    def exemplar_summary(self, k: int = 16, window_s: float | None = None, *, edges: Any = None, by: Any = None,
                         window_of: str = "finish", with_state: bool = False) -> dict[str, Any]:
        """The ``k`` SLOWEST requests of every (group, time window) WITH THEIR IDENTITY -- a dashboard's "exemplars": from
        "p99 rose here" to ``batch[s]``, the replica and the time to open; and the top-k latencies an extreme-value fit of
        the tail starts from.  Computed by ``af_engine_summarize_exemplars``, every word equal to :func:`latency_exemplars`
        on the group's scenarios: larger latency first, ties by ascending scenario index, then row index.  Windows:
        ``window_s`` seconds or explicit ``edges`` by ``window_of`` (``"finish"`` or ``"arrival"``, as in
        :meth:`window_summary`); neither: the whole run as one window (W' = 1, ``edges`` None; ``"arrival"`` is refused).
        ``by`` as in :meth:`window_summary`.  Returns numpy arrays: ``scenario`` and ``row`` int64 [G, W', k]
        (``batch[scenario].rqs_clock[row]`` is the request; -1 in an empty slot), ``start`` / ``finish`` / ``latency``
        float64 [G, W', k] (NaN in an empty slot), ``total`` int64 [G, W'] (the rows of the cell) and ``kept`` = min(k,
        total); with ``with_state=True`` also ``state`` float64 [G, W', k, series] -- the sample row the request met on
        arrival, row ``floor(start / sample_period) - 1`` (the rule of :meth:`state_summary`), the ``ram_in_use`` columns
        decoded from their float32 bits, NaN where there is no state -- and ``series_names``; and ``edges``, ``window_of``,
        ``replicas`` [G], ``exemplar_ms``, ``scratch_bytes``.  COMPLETED requests only."""
        import torch

        self._require_clock()
        kk = check_exemplar_k(k)
        whole = window_s is None and edges is None
        if check_window_of(window_of) == "arrival" and whole:
            msg = "window_of='arrival' needs window_s or edges: the whole run has no window"
            raise ValueError(msg)
        if with_state:
            self._require_samples()
        e = None if whole else _resolve_edges(window_s, edges, self.plan.total_time)
        ids, n_groups = self._window_groups(by)
        n_win = 1 if e is None else int(e.shape[0] - 1)
        eng, dev = self._arrival_engine()
        clock, samples, n_series = self._clock_t, self._samples_t, int(self.plan.n_series)
        total = torch.empty((n_groups, n_win), dtype=torch.int64, device=dev)
        kept = torch.empty((n_groups, n_win), dtype=torch.int32, device=dev)
        scenario, row = (torch.empty((n_groups, n_win, kk), dtype=torch.int32, device=dev) for _ in range(2))
        pair = torch.empty((n_groups, n_win, kk, 2), dtype=torch.float64, device=dev)
        state = torch.empty((n_groups, n_win, kk, n_series), dtype=torch.int32, device=dev) if with_state else None
        grp = torch.from_numpy(np.where(ids < 0, _abi.POOL_SKIP, ids).astype(np.uint32).view(np.int32)).to(dev)
        ms, scratch = eng.summarize_exemplars(
            len(self), n_groups, kk, edges=e, window_of=window_of, clock_ptr=clock.data_ptr(), clock_capacity=int(clock.shape[1]),
            counts_ptr=self._counts_t.data_ptr(), total_ptr=total.data_ptr(), kept_ptr=kept.data_ptr(),
            scenario_ptr=scenario.data_ptr(), row_ptr=row.data_ptr(), pair_ptr=pair.data_ptr(),
            state_ptr=state.data_ptr() if state is not None else 0, samples_ptr=samples.data_ptr() if state is not None else 0,
            tick_capacity=int(samples.shape[1]) if state is not None else 0, sample_period=float(self.plan.sample_period),
            group_ptr=grp.data_ptr())

        def host(t: Any) -> np.ndarray:
            return t.cpu().numpy().view(np.uint32)

        raw = {"total": total.cpu().numpy().view(np.uint64), "kept": host(kept), "scenario": host(scenario), "row": host(row),
               "clock": pair.cpu().numpy()}
        out = _exemplar_columns(raw, edges=e, window_of=window_of, replicas=np.bincount(ids[ids >= 0], minlength=n_groups),
                                exemplar_ms=ms, scratch_bytes=scratch)
        if state is not None:
            w = host(state)
            val = w.astype(np.float64)
            ram = ram_columns(n_series, self.plan.n_edges)
            val[..., ram] = w[..., ram].view(np.float32).astype(np.float64)
            out["state"] = np.where(w == 0xFFFFFFFF, np.nan, val)
            out["series_names"] = self.series_names()
        return out

    def save_exemplar_summary(self, path: str, by: Any = None, *, k: int = 16, window_s: float | None = None, edges: Any = None,
                              window_of: str = "finish", with_state: bool = False) -> dict[str, np.ndarray]:
        """Columnar dump of the slowest requests with one row per group (grid point): ``param:<axis>`` (for a Sweep),
        ``replicas`` and the [G, W', k] columns ``exemplar_scenario``, ``exemplar_row``, ``exemplar_start``,
        ``exemplar_finish``, ``exemplar_latency``, the [G, W'] columns ``exemplar_total`` and ``exemplar_kept`` and, with
        ``with_state``, ``exemplar_state`` [G, W', k, series] with the per-file ``series_names``
        (:meth:`exemplar_summary`); ``window_edges`` [W + 1] (absent for the whole run) and ``window_of`` are per-file
        values, as in :meth:`save_window_summary`.  ``.npz`` or ``.parquet``; :func:`load_summary` reads it back."""
        ex = self.exemplar_summary(k, window_s, edges=edges, by=by, window_of=window_of, with_state=with_state)
        n_groups = int(ex["replicas"].shape[0])
        cols: dict[str, np.ndarray] = {}
        if hasattr(by, "point_columns"):
            for name, v in by.point_columns().items():
                cols[f"param:{name}"] = np.asarray(v, dtype=np.float64)
        cols["replicas"] = np.asarray(ex["replicas"], dtype=np.int64)
        for name in ("scenario", "row", "start", "finish", "latency", "total", "kept"):
            cols[f"exemplar_{name}"] = np.ascontiguousarray(ex[name][:n_groups])
        if with_state:
            cols["exemplar_state"] = np.ascontiguousarray(ex["state"][:n_groups])
            cols["series_names"] = np.asarray(ex["series_names"])
        if ex["edges"] is not None:
            cols["window_edges"] = np.asarray(ex["edges"], dtype=np.float64)
        cols["window_of"] = np.asarray(window_of)
        _write_columns(str(path), cols, n_groups)
        return cols

    # ---- mergeable log-linear latency histograms per window and group ----------------------------------------------
    def _latency_histogram_cells(self, e: np.ndarray | None, ids: np.ndarray, n_groups: int, window_of: str,
                                 binning: tuple[int, int, int, int]) -> dict[str, Any]:
        """The device call: the int64 tensors of ``n_groups`` groups for the group ids ``ids`` [n] (negative: left out)."""
        import torch

        m, e0, o, n_bins = binning
        n_win = 1 if e is None else int(e.shape[0] - 1)
        eng, dev = self._arrival_engine()
        clock = self._clock_t
        count = torch.empty((n_groups, n_win), dtype=torch.int64, device=dev)
        hist = torch.empty((n_groups, n_win, n_bins), dtype=torch.int32, device=dev)
        rest = torch.empty((3, n_groups, n_win), dtype=torch.int32, device=dev)
        grp = torch.from_numpy(np.where(ids < 0, _abi.POOL_SKIP, ids).astype(np.uint32).view(np.int32)).to(dev)
        ms, scratch = eng.summarize_latency_histogram(
            len(self), n_groups, edges=e, window_of=window_of, sub_bits=m, min_exp=e0, octaves=o, clock_ptr=clock.data_ptr(),
            clock_capacity=int(clock.shape[1]), counts_ptr=self._counts_t.data_ptr(), count_ptr=count.data_ptr(),
            hist_ptr=hist.data_ptr(), under_ptr=rest[0].data_ptr(), over_ptr=rest[1].data_ptr(), nan_ptr=rest[2].data_ptr(),
            group_ptr=grp.data_ptr())
        wide = rest.to(torch.int64) & 0xFFFFFFFF     # (the words are uint32)
        return {"hist": hist.to(torch.int64) & 0xFFFFFFFF, "count": count, "under": wide[0], "over": wide[1], "nan": wide[2],
                "latency_histogram_ms": ms, "scratch_bytes": scratch}

    def latency_histogram_summary(self, window_s: float | None = None, *, edges: Any = None, by: Any = None, window_of: str = "finish",
                                  sub_bits: int = 5, min_exp: int = -20, octaves: int = 32) -> dict[str, Any]:
        """The DISTRIBUTION of the latencies of every (group, time window) as a mergeable log-linear histogram -- a latency
        heatmap over time, two cells to compare, quantile brackets at levels chosen afterwards.  Computed by
        ``af_engine_summarize_latency_histogram`` in one streaming pass over the clock rows, every word equal to
        :func:`latency_histogram` on the group's scenarios.  Binning on the bit pattern of the float64 latency
        (:func:`latency_bin_index`): ``octaves`` octaves from ``2 ** min_exp`` seconds with ``2 ** sub_bits`` bins each; the
        default is 1024 bins from 0.95 us to 4096 s, each 3.1 % wide.  Windows: ``window_s`` seconds or explicit ``edges`` by
        ``window_of`` (``"finish"`` or ``"arrival"``, as in :meth:`window_summary`); neither: the whole run as one window
        (W' = 1, ``edges`` None; ``"arrival"`` is refused).  ``by`` as in :meth:`window_summary`, or the name(s) of
        per-scenario parameter columns (:func:`groups_of_columns`).  Returns int64 tensors on the run's device: ``hist``
        [G, W', B] and ``count``, ``under``, ``over``, ``nan`` [G, W'] (``under + over + nan + hist.sum(-1) == count``); and
        numpy ``bin_edges`` [B + 1] (seconds), ``edges``, ``replicas`` [G], ``sub_bits``, ``min_exp``, ``octaves``,
        ``window_of``, ``latency_histogram_ms`` and ``scratch_bytes``.  Only integer additions: summaries over the same cells
        add up (:func:`latency_histogram_merge`), coarsen (:func:`latency_histogram_regroup`), give quantile brackets
        (:func:`latency_histogram_quantiles`) and distances (:func:`latency_histogram_distance`).  COMPLETED requests only."""
        self._require_clock()
        binning = check_latency_bins(sub_bits, min_exp, octaves)
        whole = window_s is None and edges is None
        if check_window_of(window_of) == "arrival" and whole:
            msg = "window_of='arrival' needs window_s or edges: the whole run has no window"
            raise ValueError(msg)
        e = None if whole else _resolve_edges(window_s, edges, self.plan.total_time)
        ids, n_groups = _groups_of_named_columns(by, self.overrides) or self._window_groups(by)
        out = self._latency_histogram_cells(e, ids, n_groups, window_of, binning)
        out.update(bin_edges=latency_bin_edges(*binning[:3]), edges=e, replicas=np.bincount(ids[ids >= 0], minlength=n_groups),
                   sub_bits=binning[0], min_exp=binning[1], octaves=binning[2], window_of=window_of)
        return out

    def save_latency_histogram_summary(self, path: str, by: Any = None, *, window_s: float | None = None, edges: Any = None,
                                       window_of: str = "finish", sub_bits: int = 5, min_exp: int = -20, octaves: int = 32) -> dict[str, np.ndarray]:
        """Columnar dump of the latency histograms with one row per group (grid point): ``param:<axis>`` (for a Sweep),
        ``replicas``, ``lhist_hist`` [G, W', B] and the [G, W'] columns ``lhist_count``, ``lhist_under``, ``lhist_over``,
        ``lhist_nan`` (:meth:`latency_histogram_summary`); ``lhist_sub_bits``, ``lhist_min_exp``, ``lhist_octaves``,
        ``window_edges`` [W + 1] (absent for the whole run) and ``window_of`` are per-file values.  ``.npz`` or ``.parquet``;
        :func:`load_summary` reads it back, and the latency histogram functions (merge, regroup, quantiles, distance) accept
        what it returns."""
        return _save_latency_histogram(self.latency_histogram_summary(window_s, edges=edges, by=by, window_of=window_of, sub_bits=sub_bits,
                                                                      min_exp=min_exp, octaves=octaves), str(path), by)

    # ---- paired latency differences between scenarios that share their seeds ---------------------------------------
    def _check_pairs(self, a: Any, b: Any) -> tuple[np.ndarray, np.ndarray]:
        """The scenario indices of both sides as int64 [P], or ValueError: out of range, or a pair that was not sent the same
        requests -- its seeds or a generator column differ."""
        ia, ib = np.asarray(a, dtype=np.int64).reshape(-1), np.asarray(b, dtype=np.int64).reshape(-1)
        n = len(self)
        if ia.shape != ib.shape or ia.shape[0] == 0 or ((ia < 0) | (ia >= n) | (ib < 0) | (ib >= n)).any():
            msg = f"a and b must be two index vectors of one length > 0 into the {n} scenarios"
            raise ValueError(msg)
        seeds = np.asarray(self.seeds, dtype=np.uint64)
        checks = [("seeds", seeds)] + [(key, np.asarray(self.overrides[key], dtype=np.float64)) for key in self.GENERATOR_COLUMNS if key in self.overrides]
        for name, col in checks:
            bad = np.nonzero(col[ia] != col[ib])[0]
            if bad.shape[0]:
                p = int(bad[0])
                msg = (f"pair {p} (scenarios {int(ia[p])} and {int(ib[p])}) was not sent the same requests: {name} differ "
                       f"({col[ia[p]]!r} and {col[ib[p]]!r}); paired differences need common seeds (expand_grid(common_seeds=True))")
                raise ValueError(msg)
        return ia, ib

    def paired_summary(self, a: Any, b: Any, window_s: float | None = None, *, edges: Any = None, by: Any = None, thresholds: Any = None,
                       sub_bits: int = 5, min_exp: int = -20, octaves: int = 32, with_rows: bool = False) -> dict[str, Any]:
        """The latency difference of the SAME request under two configurations: pair p compares scenarios ``a[p]`` and ``b[p]``,
        which must share their seed and every generator column (otherwise ValueError naming the first offender) and so were sent
        the same requests at the same instants.  The arrival rows of the distinct ``a`` scenarios are regenerated on the device
        (``af_engine_summarize_arrivals`` with a ``times`` buffer: no simulation), the clock rows of both sides are joined
        through them and reduced by ``af_engine_summarize_pairs``; every word equals :func:`latency_pairs` /
        :func:`latency_pair_cells` on ``batch[i].rqs_clock`` and ``batch.arrival_times(i)``.  Windows by ARRIVAL time:
        ``window_s`` seconds or explicit ``edges``; neither: one window over the run.  ``by``: one group id per pair (negative:
        in no cell), ``"pair"`` for singletons, None for one group -- ``Sweep.pairs(...)["by"]`` groups by the remaining axes.
        Returns numpy arrays.  Per (pair, window) [P, W']: ``both``, ``only_a``, ``only_b``, ``neither``, ``nan`` uint32,
        ``sum_d``, ``sum_a`` float64 and ``mean_d`` = sum_d / (both - nan), ``mean_a``, ``relative`` = mean_d / mean_a; per pair
        ``unmatched_a``, ``unmatched_b``; per cell [G, W']: the uint64 sums of the five counts, ``slower``, ``faster``, ``equal``,
        ``above`` [G, W', T], ``min_d``, ``max_d``, ``hist_pos``, ``hist_neg`` uint32 [G, W', B], ``under_pos``, ``under_neg``,
        ``over_pos``, ``over_neg``, named ``cell_both`` ... for the five counts; with ``with_rows`` the join ``row_a`` /
        ``row_b`` uint32 [P, draw_capacity].  ``only_a`` / ``only_b`` / ``neither`` cannot tell a dropped request from one still in
        flight at the end of the run: the last windows always lose requests (the caveat of :meth:`arrival_summary`)."""
        import torch

        self._require_clock()
        ia, ib = self._check_pairs(a, b)
        binning = check_latency_bins(sub_bits, min_exp, octaves)
        th = check_pair_thresholds(thresholds)
        e = None if window_s is None and edges is None else _resolve_edges(window_s, edges, self.plan.total_time)
        n_pairs = int(ia.shape[0])
        if isinstance(by, str):
            if by != "pair":
                msg = f"by must be one group id per pair, 'pair' or None, not {by!r}"
                raise ValueError(msg)
            ids, n_groups = np.arange(n_pairs, dtype=np.int64), n_pairs
        else:
            ids, n_groups = resolve_groups(by, n_pairs)
        rows, time_row = np.unique(ia, return_inverse=True)
        seeds, cols, cap = self._arrival_sweep(rows)
        eng, dev = self._arrival_engine()
        n_rows, n_win, n_bins, n_thr = int(rows.shape[0]), 1 if e is None else int(e.shape[0] - 1), binning[3], int(th.shape[0])
        times = torch.empty((n_rows, cap), dtype=torch.float64, device=dev)
        arr = torch.empty((n_rows, 1), dtype=torch.int64, device=dev)
        arrival_ms, _ = eng.summarize_arrivals(seeds, cols, n_rows, np.asarray([0.0, max(float(self.plan.total_time), 1.0)]),
                                               draw_capacity=cap, arrivals_ptr=arr.data_ptr(), times_ptr=times.data_ptr())

        def u32(v: np.ndarray) -> Any:
            return torch.from_numpy(np.ascontiguousarray(v).astype(np.uint32).view(np.int32)).to(dev)

        pa, pb, tr, grp = u32(ia), u32(ib), u32(time_row.reshape(-1)), u32(np.where(ids < 0, _abi.POOL_SKIP, ids))
        cells = n_groups * n_win
        pair_counts = torch.empty((n_pairs, n_win, 5), dtype=torch.int32, device=dev)
        pair_sums = torch.empty((n_pairs, n_win, 2), dtype=torch.float64, device=dev)
        unmatched = torch.empty((n_pairs, 2), dtype=torch.int32, device=dev)
        cell_counts = torch.empty((cells, 8), dtype=torch.int64, device=dev)
        above = torch.empty((cells, max(n_thr, 1)), dtype=torch.int64, device=dev)
        extremes = torch.empty((cells, 2), dtype=torch.float64, device=dev)
        hist = torch.empty((cells, 2, n_bins), dtype=torch.int32, device=dev)
        tails = torch.empty((cells, 4), dtype=torch.int32, device=dev)
        row_a = torch.empty((n_pairs, cap), dtype=torch.int32, device=dev) if with_rows else None
        row_b = torch.empty((n_pairs, cap), dtype=torch.int32, device=dev) if with_rows else None
        clock = self._clock_t
        ms, scratch = eng.summarize_pairs(
            len(self), n_pairs, n_groups, pair_a_ptr=pa.data_ptr(), pair_b_ptr=pb.data_ptr(), times_ptr=times.data_ptr(),
            time_row_ptr=tr.data_ptr(), n_time_rows=n_rows, draw_capacity=cap, clock_ptr=clock.data_ptr(), clock_capacity=int(clock.shape[1]),
            counts_ptr=self._counts_t.data_ptr(), pair_counts_ptr=pair_counts.data_ptr(), pair_sums_ptr=pair_sums.data_ptr(),
            unmatched_ptr=unmatched.data_ptr(), cell_counts_ptr=cell_counts.data_ptr(), extremes_ptr=extremes.data_ptr(),
            hist_ptr=hist.data_ptr(), tails_ptr=tails.data_ptr(), above_ptr=above.data_ptr() if n_thr else 0,
            row_a_ptr=row_a.data_ptr() if with_rows else 0, row_b_ptr=row_b.data_ptr() if with_rows else 0, group_ptr=grp.data_ptr(),
            edges=e, thresholds=th, sub_bits=binning[0], min_exp=binning[1], octaves=binning[2])
        out: dict[str, Any] = {"edges": e, "thresholds": th, "sub_bits": binning[0], "min_exp": binning[1], "octaves": binning[2],
                               "bin_edges": latency_bin_edges(*binning[:3]), "a": ia, "b": ib, "groups": ids,
                               "replicas": np.bincount(ids[ids >= 0], minlength=n_groups), "pairs_ms": ms, "arrival_ms": arrival_ms,
                               "scratch_bytes": scratch}
        pc = pair_counts.cpu().numpy().view(np.uint32)
        for k, name in enumerate(_PAIR_COUNTS):
            out[name] = np.ascontiguousarray(pc[:, :, k])
        ps = pair_sums.cpu().numpy()
        out["sum_d"], out["sum_a"] = np.ascontiguousarray(ps[:, :, 0]), np.ascontiguousarray(ps[:, :, 1])
        un = unmatched.cpu().numpy().view(np.uint32)
        out["unmatched_a"], out["unmatched_b"] = un[:, 0].copy(), un[:, 1].copy()
        valid = out["both"].astype(np.float64) - out["nan"]
        with np.errstate(invalid="ignore", divide="ignore"):
            out["mean_d"] = np.where(valid > 0, out["sum_d"] / valid, np.nan)
            out["mean_a"] = np.where(valid > 0, out["sum_a"] / valid, np.nan)
            out["relative"] = out["mean_d"] / out["mean_a"]
        cc = cell_counts.cpu().numpy().view(np.uint64).reshape(n_groups, n_win, 8)
        for k, name in enumerate((*(f"cell_{c}" for c in _PAIR_COUNTS), "slower", "faster", "equal")):
            out[name] = np.ascontiguousarray(cc[:, :, k])
        out["above"] = above.cpu().numpy().view(np.uint64).reshape(n_groups, n_win, -1)[:, :, :n_thr].copy()
        ex = extremes.cpu().numpy().reshape(n_groups, n_win, 2)
        out["min_d"], out["max_d"] = np.ascontiguousarray(ex[:, :, 0]), np.ascontiguousarray(ex[:, :, 1])
        hh = hist.cpu().numpy().view(np.uint32).reshape(n_groups, n_win, 2, n_bins)
        out["hist_pos"], out["hist_neg"] = np.ascontiguousarray(hh[:, :, 0]), np.ascontiguousarray(hh[:, :, 1])
        tt = tails.cpu().numpy().view(np.uint32).reshape(n_groups, n_win, 4)
        for k, name in enumerate(("under_pos", "under_neg", "over_pos", "over_neg")):
            out[name] = np.ascontiguousarray(tt[:, :, k])
        if with_rows:
            out["row_a"], out["row_b"] = row_a.cpu().numpy().view(np.uint32), row_b.cpu().numpy().view(np.uint32)
        return out

    def paired_bands(self, a: Any, b: Any, window_s: float | None = None, *, edges: Any = None, by: Any = None, level: float = 0.95,
                     q: tuple[float, float] = (0.05, 0.95)) -> dict[str, Any]:
        """The paired-t comparison: per (group, window), over the group's pairs with a matched request in the window (``n``
        [G, W'] of them), the ``mean`` of the per-pair ``mean_d`` with ``std``, ``ci_halfwidth`` (at ``level``) and the linear
        quantiles ``q_lo`` / ``q_hi`` as :func:`window_bands_by_group` gives them: numpy float64 [G, W', 3], the columns
        ``mean_d``, ``mean_a`` and ``relative`` (``keys``).  The variance is that of the DIFFERENCES: what common seeds buy.
        ``pooled`` is ``paired_summary(a, b, ..., by=by)``."""
        return self._paired_bands_of(self.paired_summary(a, b, window_s, edges=edges, by=by), level, q)

    def _paired_bands_of(self, per: dict[str, Any], level: float, q: tuple[float, float]) -> dict[str, Any]:
        """:meth:`paired_bands` of a paired summary."""
        import torch

        ids, n_groups = per["groups"], int(per["replicas"].shape[0])
        dev = self._counts_t.device
        body = torch.from_numpy(np.nan_to_num(np.stack([per["mean_d"], per["mean_a"], per["relative"]], axis=2))).to(dev)
        valid = torch.from_numpy(per["both"].astype(np.int64) - per["nan"] > 0).to(dev)
        out = window_bands_by_group(body, ids, n_groups, level, q, valid=valid)
        out["keys"] = ("mean_d", "mean_a", "relative")
        out["pooled"] = per
        out["edges"] = per["edges"]
        return out

    def save_paired_summary(self, path: str, a: Any, b: Any, by: Any = None, *, window_s: float | None = None, edges: Any = None,
                            thresholds: Any = None, sub_bits: int = 5, min_exp: int = -20, octaves: int = 32,
                            level: float = 0.95) -> dict[str, np.ndarray]:
        """Columnar dump of the paired differences with one row per group of pairs: ``replicas`` and, prefixed ``paired_``, the
        cell arrays of :meth:`paired_summary` (``both`` ... ``nan``, ``slower``, ``faster``, ``equal``, ``above``, ``min_d``,
        ``max_d``, ``hist_pos``, ``hist_neg``, ``under_*``, ``over_*``) and ``mean_d_mean`` / ``mean_d_ci`` [G, W'] over the pairs
        (:meth:`paired_bands`); ``paired_sub_bits``, ``paired_min_exp``, ``paired_octaves``, ``paired_thresholds`` and
        ``window_edges`` (absent for one window) are per-file values.  ``.npz`` or ``.parquet``; :func:`load_summary` reads it
        back, and :func:`paired_merge` / :func:`paired_delta_quantiles` accept what it returns."""
        summ = self.paired_summary(a, b, window_s, edges=edges, by=by, thresholds=thresholds, sub_bits=sub_bits, min_exp=min_exp, octaves=octaves)
        bands = self._paired_bands_of(summ, level, (0.05, 0.95))
        cols: dict[str, np.ndarray] = {"replicas": np.asarray(summ["replicas"], dtype=np.int64)}
        for k in _PAIR_CELL_SUMS:
            cols[f"paired_{k}"] = np.ascontiguousarray(summ[f"cell_{k}" if k in _PAIR_COUNTS else k]).astype(np.int64)
        for k in ("min_d", "max_d"):
            cols[f"paired_{k}"] = summ[k]
        cols["paired_mean_d_mean"] = np.ascontiguousarray(bands["mean"][:, :, 0])
        cols["paired_mean_d_ci"] = np.ascontiguousarray(bands["ci_halfwidth"][:, :, 0])
        for k in ("sub_bits", "min_exp", "octaves"):
            cols[f"paired_{k}"] = np.asarray(summ[k], dtype=np.int64)
        cols["paired_thresholds"] = summ["thresholds"]
        if summ["edges"] is not None:
            cols["window_edges"] = summ["edges"]
        _write_columns(str(path), cols, int(cols["replicas"].shape[0]))
        return cols

    def quantile_summary(self, levels: Any, *, thresholds: Any = None, window_s: float | None = None, edges: Any = None,
                         by: Any = None, window_of: str = "finish") -> dict[str, Any]:
        """Any latency quantiles and SLO shares of every (group, time window): p99.9 at a grid point, p90 during an
        outage, the share of requests that met a 200 ms objective in every 10 s window.  Computed by the HIP quantile
        analyzer (``af_engine_summarize_quantiles``), bit-equal to :func:`latency_window_quantiles` / ``np.quantile`` on
        the concatenated latencies of the group's scenarios.  ``levels`` in [0, 1] and ``thresholds`` in seconds (None:
        none): any order, duplicates allowed, at most 64 each.  Neither ``window_s`` nor ``edges``: the whole run, one row
        per group (W = 1, ``edges`` None; rows need not be in completion order); otherwise windows as in
        :meth:`window_summary`.  ``by`` as there, ``"scenario"`` included.  Returns, on the run's device, ``quantiles``
        float64 [G, W, Q] (NaN where empty), ``count`` int64 [G, W], ``within`` int64 [G, W, T] and ``share`` float64
        [G, W, T] (= within / count, NaN where empty); ``levels``, ``thresholds``, ``edges``, ``replicas`` [G],
        ``quantile_ms``, ``scratch_bytes`` and ``window_of``.  ``window_of="arrival"``: windows by start time as in
        :meth:`window_summary` (``af_engine_summarize_arrival_quantiles``; right-censored cohorts: ``count`` is the cohort's
        completions); it needs windows -- the whole run has none."""
        import torch

        from .engine import Engine

        self._require_clock()
        q, th = check_levels(levels), check_slo_thresholds(thresholds)
        if q.shape[0] == 0 and th.shape[0] == 0:
            msg = "quantile_summary needs at least one level or one threshold"
            raise ValueError(msg)
        whole = window_s is None and edges is None
        if check_window_of(window_of) == "arrival" and whole:
            msg = "window_of='arrival' needs window_s or edges: the whole run has no window"
            raise ValueError(msg)
        e = None if whole else _resolve_edges(window_s, edges, self.plan.total_time)
        ids, n_groups = self._window_groups(by)
        n_win = 1 if e is None else int(e.shape[0] - 1)
        clock = self._clock_t
        dev = clock.device
        quant = torch.empty((n_groups, n_win, q.shape[0]), dtype=torch.float64, device=dev)
        count = torch.empty((n_groups, n_win), dtype=torch.int32, device=dev)
        within = torch.empty((n_groups, n_win, th.shape[0]), dtype=torch.int32, device=dev)
        grp = torch.from_numpy(np.where(ids < 0, _abi.POOL_SKIP, ids).astype(np.uint32).view(np.int32)).to(dev)
        torch.cuda.synchronize(dev)
        if self._summ_engine is None:
            self._summ_engine = Engine(self.plan, dev.index if dev.index is not None else torch.cuda.current_device())
        ms, scratch = self._summ_engine.summarize_quantiles(
            len(self), n_groups, q, edges=e, thresholds=th, clock_ptr=clock.data_ptr(), clock_capacity=int(clock.shape[1]),
            counts_ptr=self._counts_t.data_ptr(), count_ptr=count.data_ptr(), quantiles_ptr=quant.data_ptr() if q.shape[0] else 0,
            within_ptr=within.data_ptr() if th.shape[0] else 0, group_ptr=grp.data_ptr(), window_of=window_of)
        return _finish_quantile_summary(quant, count, within, q, th, e, ids, n_groups, ms, scratch, window_of)

    def _export_cells(self, e: np.ndarray | None, ids: np.ndarray, window_of: str) -> tuple[Any, Any, float, int]:
        """This run's part of cells that span several runs (``af_engine_export_cells``): the latencies of its scenarios that
        fall into the windows ``e`` (None: the whole run), scenario-major, as a float64 tensor on the run's device, and the
        windows' bounds as an int32 tensor [n, W + 1] (uint32 words).  ``ids`` [n]: a negative id exports nothing for the
        scenario.  Also the call's wall time in ms and the engine's scratch size."""
        import torch

        from .engine import Engine

        self._require_clock()
        clock = self._clock_t
        dev = clock.device
        n, cap = len(self), int(clock.shape[1])
        n_win = 1 if e is None else int(e.shape[0] - 1)
        capacity = int(np.minimum(self.counts[:, _abi.CNT_COMPLETED].astype(np.int64), cap).sum())   # always suffices
        lat = torch.empty(capacity, dtype=torch.float64, device=dev)
        bounds = torch.empty((n, n_win + 1), dtype=torch.int32, device=dev)
        grp = torch.from_numpy(np.where(ids < 0, _abi.POOL_SKIP, 0).astype(np.uint32).view(np.int32)).to(dev)
        torch.cuda.synchronize(dev)
        if self._summ_engine is None:
            self._summ_engine = Engine(self.plan, dev.index if dev.index is not None else torch.cuda.current_device())
        count, ms, scratch = self._summ_engine.export_cells(
            n, edges=e, clock_ptr=clock.data_ptr(), clock_capacity=cap, counts_ptr=self._counts_t.data_ptr(), lat_ptr=lat.data_ptr(),
            lat_capacity=capacity, seg_bounds_ptr=bounds.data_ptr(), group_ptr=grp.data_ptr(), window_of=window_of)
        return lat[:count], bounds, ms, scratch

    def quantile_bands(self, levels: Any, *, thresholds: Any = None, window_s: float | None = None, edges: Any = None,
                       by: Any = None, level: float = 0.95, q: tuple[float, float] = (0.05, 0.95),
                       window_of: str = "finish") -> dict[str, Any]:
        """Bands over the replicas of the quantiles and SLO shares: every scenario's own values
        (``quantile_summary(by="scenario")``), then per group (``by``) and window, over the group's replicas whose window
        is not empty (``n`` [G, W] of them), ``mean``, ``std``, ``ci_halfwidth`` (at ``level``) and the linear quantiles
        ``q_lo`` / ``q_hi`` (``q``) as :func:`window_bands_by_group` gives them: numpy float64 [G, W, Q + T], the levels'
        columns first, then the thresholds' shares.  ``pooled_quantiles`` [G, W, Q], ``pooled_share`` [G, W, T] and
        ``pooled_count`` [G, W] are ``quantile_summary(by=by)`` as numpy.  ``window_of`` as there, for both."""
        import torch

        whole = window_s is None and edges is None
        e = None if whole else _resolve_edges(window_s, edges, self.plan.total_time)
        ids, n_groups = self._window_groups(by)
        per = self.quantile_summary(levels, thresholds=thresholds, edges=e, by="scenario", window_of=window_of)
        out = window_bands_by_group(torch.cat([per["quantiles"], per["share"]], dim=2), ids, n_groups, level, q, valid=per["count"] > 0)
        pooled = self.quantile_summary(levels, thresholds=thresholds, edges=e, by=ids, window_of=window_of)
        out["pooled_quantiles"] = pooled["quantiles"].cpu().numpy()[:n_groups]
        out["pooled_share"] = pooled["share"].cpu().numpy()[:n_groups]
        out["pooled_count"] = pooled["count"].cpu().numpy()[:n_groups]
        out["levels"], out["thresholds"], out["edges"], out["window_of"] = per["levels"], per["thresholds"], e, window_of
        return out

    def save_quantile_summary(self, path: str, by: Any = None, *, levels: Any, thresholds: Any = None,
                              window_s: float | None = None, edges: Any = None, level: float = 0.95,
                              window_of: str = "finish") -> dict[str, np.ndarray]:
        """Columnar dump of the quantiles and SLO shares with one row per group (grid point): ``param:<axis>`` (for a
        Sweep), ``replicas``, ``quantile_count`` [G, W], and per level i / threshold j the [G, W] columns
        ``quantile_pooled:<i>`` / ``share_pooled:<j>`` (the group's replicas pooled) and ``quantile_mean:<i>``,
        ``quantile_q05:<i>``, ``quantile_q95:<i>`` / ``share_mean:<j>``, ``share_q05:<j>``, ``share_q95:<j>`` (over the
        replicas, :meth:`quantile_bands`); ``quantile_levels`` [Q], ``slo_thresholds`` [T] and ``window_edges`` [W + 1]
        (empty for the whole run) and ``window_of`` (``"finish"`` or ``"arrival"``, as in :meth:`quantile_summary`) are
        per-file values.  ``.npz`` or ``.parquet``; :func:`load_summary` reads it back."""
        bands = self.quantile_bands(levels, thresholds=thresholds, window_s=window_s, edges=edges, by=by, level=level, q=(0.05, 0.95),
                                    window_of=window_of)
        n_groups = int(bands["replicas"].shape[0])
        n_lev = int(bands["levels"].shape[0])
        cols: dict[str, np.ndarray] = {}
        if hasattr(by, "point_columns"):
            for k, v in by.point_columns().items():
                cols[f"param:{k}"] = np.asarray(v, dtype=np.float64)
        cols["replicas"] = np.asarray(bands["replicas"], dtype=np.int64)
        cols["quantile_count"] = np.ascontiguousarray(bands["pooled_count"], dtype=np.int64)
        for what, base, cnt, pooled in (("quantile", 0, n_lev, bands["pooled_quantiles"]),
                                        ("share", n_lev, int(bands["thresholds"].shape[0]), bands["pooled_share"])):
            for i in range(cnt):
                cols[f"{what}_pooled:{i}"] = np.ascontiguousarray(pooled[:, :, i])
                cols[f"{what}_mean:{i}"] = np.ascontiguousarray(bands["mean"][:, :, base + i])
                cols[f"{what}_q05:{i}"] = np.ascontiguousarray(bands["q_lo"][:, :, base + i])
                cols[f"{what}_q95:{i}"] = np.ascontiguousarray(bands["q_hi"][:, :, base + i])
        cols["quantile_levels"] = np.asarray(bands["levels"], dtype=np.float64)
        cols["slo_thresholds"] = np.asarray(bands["thresholds"], dtype=np.float64)
        cols["window_edges"] = np.zeros(0, dtype=np.float64) if bands["edges"] is None else np.asarray(bands["edges"], dtype=np.float64)
        cols["window_of"] = np.asarray(window_of)
        _write_columns(str(path), cols, n_groups)
        return cols

    def _state_request(self, series: Any, bins: Any, lo: Any, width: Any, window_s: float | None, edges: Any, by: Any) -> dict[str, Any]:
        """What the two latency-by-state calls share: the checked request and the device buffers of the group ids."""
        import torch

        from .engine import Engine

        self._require_clock()
        self._require_samples()
        col = _state_series(series, self.series_names())
        n_bins, lo_f, width_f, period = check_state_bins(bins, lo, width, self.plan.sample_period)
        e = None if window_s is None and edges is None else _resolve_edges(window_s, edges, self.plan.total_time)
        ids, n_groups = self._window_groups(by)
        dev = self._clock_t.device
        grp = torch.from_numpy(np.where(ids < 0, _abi.POOL_SKIP, ids).astype(np.uint32).view(np.int32)).to(dev)
        torch.cuda.synchronize(dev)
        if self._summ_engine is None:
            self._summ_engine = Engine(self.plan, dev.index if dev.index is not None else torch.cuda.current_device())
        kw = {"column": col, "bins": n_bins, "lo": lo_f, "width": width_f, "sample_period": period, "edges": e,
              "clock_ptr": self._clock_t.data_ptr(), "clock_capacity": int(self._clock_t.shape[1]),
              "samples_ptr": self._samples_t.data_ptr(), "tick_capacity": int(self._samples_t.shape[1]),
              "counts_ptr": self._counts_t.data_ptr(), "group_ptr": grp.data_ptr()}
        return {"kw": kw, "grp": grp, "ids": ids, "n_groups": n_groups, "n_win": 1 if e is None else int(e.shape[0] - 1), "dev": dev,
                "meta": {"edges": e, "bin_lo": lo_f + np.arange(n_bins, dtype=np.float64) * width_f, "series": col,
                         "replicas": np.bincount(ids[ids >= 0], minlength=n_groups)}}

    def state_summary(self, series: Any, bins: int = 8, *, lo: float = 0.0, width: float = 1.0, window_s: float | None = None,
                      edges: Any = None, by: Any = None) -> dict[str, Any]:
        """Latency by the STATE A REQUEST MET ON ARRIVAL: the eight latency statistics of every (group, arrival window, bin of
        ``series`` at the request's arrival tick) -- does p95 rise with the ready queue of a server, with RAM in use, with the
        connections on an edge?  ``series``: one name of :meth:`series_names` or one index; ``bins`` bins of ``width`` from
        ``lo``, the last bin taking the overflow; the sample period is the plan's.  The state of a request is the last sample
        taken at or before its arrival as the float64 quotient ``start / sample_period`` sees it; requests that arrived before
        the first sample, or whose value lies below ``lo``, are in no cell (:func:`latency_state_cells`, the definition the HIP
        kernels of ``af_engine_summarize_state_windows`` equal bit for bit).  Windows by ARRIVAL time of ``window_s`` seconds
        or explicit ``edges``; neither: one window with no condition on time (W' = 1, ``edges`` None).  ``by`` as in
        :meth:`window_summary`.  Returns ``stats`` float64 [G, W', bins, 8] on the run's device (an empty cell: total 0, the rest
        NaN), ``bin_lo`` [bins], ``edges``, ``series`` (the index), ``keys``, ``replicas`` [G], ``state_ms`` and
        ``scratch_bytes``.  The cohorts are right-censored like ``window_of="arrival"``: ``total`` counts completions."""
        import torch

        rq = self._state_request(series, bins, lo, width, window_s, edges, by)
        stats = torch.empty((rq["n_groups"], rq["n_win"], int(bins), 8), dtype=torch.float64, device=rq["dev"])
        ms, scratch = self._summ_engine.summarize_state_windows(len(self), rq["n_groups"], stats_ptr=stats.data_ptr(), **rq["kw"])
        return {"stats": stats, "keys": LATENCY_KEYS, "state_ms": ms, "scratch_bytes": scratch, **rq["meta"]}

    def state_quantile_summary(self, series: Any, levels: Any, *, thresholds: Any = None, bins: int = 8, lo: float = 0.0,
                               width: float = 1.0, window_s: float | None = None, edges: Any = None, by: Any = None) -> dict[str, Any]:
        """Any latency quantiles and SLO shares over the cells of :meth:`state_summary` (``af_engine_summarize_state_quantiles``,
        bit-equal to :func:`latency_state_quantiles` / ``np.quantile`` on the concatenated latencies): ``quantiles`` float64
        [G, W', bins, Q] (NaN where empty), ``count`` int64 [G, W', bins], ``within`` int64 [G, W', bins, T] and ``share`` float64
        (= within / count, NaN where empty) on the run's device; ``levels``, ``thresholds`` and the rest as there."""
        import torch

        q, th = check_levels(levels), check_slo_thresholds(thresholds)
        if q.shape[0] == 0 and th.shape[0] == 0:
            msg = "state_quantile_summary needs at least one level or one threshold"
            raise ValueError(msg)
        rq = self._state_request(series, bins, lo, width, window_s, edges, by)
        shape, dev = (rq["n_groups"], rq["n_win"], int(bins)), rq["dev"]
        quant = torch.empty((*shape, q.shape[0]), dtype=torch.float64, device=dev)
        count = torch.empty(shape, dtype=torch.int32, device=dev)
        within = torch.empty((*shape, th.shape[0]), dtype=torch.int32, device=dev)
        ms, scratch = self._summ_engine.summarize_state_quantiles(
            len(self), rq["n_groups"], q, thresholds=th, count_ptr=count.data_ptr(), quantiles_ptr=quant.data_ptr() if q.shape[0] else 0,
            within_ptr=within.data_ptr() if th.shape[0] else 0, **rq["kw"])
        cnt = count.to(torch.int64) & 0xFFFFFFFF   # (the device's words are uint32)
        wth = within.to(torch.int64) & 0xFFFFFFFF
        nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
        share = torch.where((cnt > 0)[..., None], wth.to(torch.float64) / cnt.clamp(min=1).to(torch.float64)[..., None], nan)
        return {"quantiles": quant, "count": cnt, "within": wth, "share": share, "levels": q, "thresholds": th, "state_ms": ms,
                "scratch_bytes": scratch, **rq["meta"]}

    def save_state_summary(self, path: str, by: Any = None, *, series: Any, bins: int = 8, lo: float = 0.0, width: float = 1.0,
                           window_s: float | None = None, edges: Any = None, levels: Any = None,
                           thresholds: Any = None) -> dict[str, np.ndarray]:
        """Columnar dump of the latency-by-state statistics with one row per group (grid point): ``param:<axis>`` (for a
        Sweep), ``replicas``, per latency key the [G, W', bins] column ``state_pooled:<key>`` (:meth:`state_summary`) and, with
        ``levels`` / ``thresholds``, ``state_count`` and per level i / threshold j ``state_quantile:<i>`` / ``state_share:<j>``
        (:meth:`state_quantile_summary`).  ``state_bin_lo`` [bins], ``state_series`` (the series index), ``window_edges``
        [W' + 1] (empty: one window over all time), ``quantile_levels`` and ``slo_thresholds`` are per-file values.  ``.npz`` or
        ``.parquet``; :func:`load_summary` reads it back.  (Bands over replicas are not written: most cells of one replica are
        empty.)"""
        summ = self.state_summary(series, bins, lo=lo, width=width, window_s=window_s, edges=edges, by=by)
        n_groups = int(summ["replicas"].shape[0])
        cols: dict[str, np.ndarray] = {}
        if hasattr(by, "point_columns"):
            for k, v in by.point_columns().items():
                cols[f"param:{k}"] = np.asarray(v, dtype=np.float64)
        cols["replicas"] = np.asarray(summ["replicas"], dtype=np.int64)
        st = summ["stats"].cpu().numpy()
        for j, k in enumerate(LATENCY_KEYS):
            cols[f"state_pooled:{k}"] = np.ascontiguousarray(st[..., j])
        q, th = check_levels([] if levels is None else levels), check_slo_thresholds(thresholds)
        if q.shape[0] or th.shape[0]:
            qs = self.state_quantile_summary(series, q, thresholds=th, bins=bins, lo=lo, width=width, window_s=window_s, edges=edges, by=by)
            cols["state_count"] = np.ascontiguousarray(qs["count"].cpu().numpy(), dtype=np.int64)
            for i in range(q.shape[0]):
                cols[f"state_quantile:{i}"] = np.ascontiguousarray(qs["quantiles"].cpu().numpy()[..., i])
            for i in range(th.shape[0]):
                cols[f"state_share:{i}"] = np.ascontiguousarray(qs["share"].cpu().numpy()[..., i])
        cols["quantile_levels"], cols["slo_thresholds"] = q, th
        cols["state_bin_lo"] = np.asarray(summ["bin_lo"], dtype=np.float64)
        cols["state_series"] = np.asarray([summ["series"]], dtype=np.float64)
        cols["window_edges"] = np.zeros(0, dtype=np.float64) if summ["edges"] is None else np.asarray(summ["edges"], dtype=np.float64)
        _write_columns(str(path), cols, n_groups)
        return cols

    def _series_thresholds(self, thresholds: Any) -> np.ndarray | None:
        if thresholds is None:
            return None
        names = self.series_names()
        if isinstance(thresholds, dict):
            thr = np.zeros(len(names))
            for k, v in thresholds.items():
                if k not in names:
                    msg = f"unknown series {k!r} in thresholds (series_names(): {names})"
                    raise ValueError(msg)
                thr[names.index(k)] = float(v)
        else:
            thr = np.asarray(thresholds, dtype=np.float64)
            if thr.shape != (len(names),):
                msg = f"thresholds must be a vector of one value per series ({len(names)}) or a dict, not of shape {thr.shape}"
                raise ValueError(msg)
        if np.isnan(thr).any():
            msg = "thresholds must not be NaN"
            raise ValueError(msg)
        return thr

    def _series_tick_edges(self, window_s: float | None, ticks_per_window: int | None, tick_edges: Any) -> np.ndarray:
        return _resolve_tick_edges(window_s, ticks_per_window, tick_edges, self.plan.sample_period, self.plan.tick_count)

    def series_window_summary(self, window_s: float | None = None, *, ticks_per_window: int | None = None,
                              tick_edges: Any = None, by: Any = None, thresholds: Any = None) -> dict[str, Any]:
        """Statistics of every sampled series (``ready_queue_len``, ``event_loop_io_sleep``, ``ram_in_use`` per server,
        ``edge_concurrent_connection`` per edge) of every (group, window of ticks), over all scenarios of the group: how
        long a server's ready queue is DURING an outage, at each grid point.  Computed by the HIP series analyzer
        (``af_engine_summarize_series_windows``), equal to :func:`series_window_stats` on the group's samples.  Windows:
        ``window_s`` seconds (a multiple of the sample period; default 1 s), ``ticks_per_window`` ticks or explicit
        ``tick_edges`` (tick indices); sample ``k`` carries the label ``k * sample_period`` as in ``get_series``.  ``by``
        as in :meth:`window_summary`.  ``thresholds``: None (0.0), a vector [n_series] or ``{series name: value}`` over
        :meth:`series_names` (missing: 0.0).  Returns torch tensors on the run's device: ``count`` int64 [G, W]; ``mean``,
        ``min``, ``max`` and ``above_share`` (values above the threshold / count) float64 [G, W, S], NaN in empty cells;
        the raw ``min_words`` / ``max_words`` / ``above`` int32 (``ram_in_use``: the float32 bits of the float minimum /
        maximum, -0.0 below +0.0, so one window over the whole run has ``max_words`` equal to ``series_max`` of
        :meth:`summary`; the other series: the smallest / largest count); and ``series``, ``tick_edges``, ``times`` (the windows'
        start labels in seconds), ``replicas`` [G], ``series_window_ms``, ``scratch_bytes``."""
        import torch

        from .engine import Engine

        if self._samples_t is None:
            msg = "run(collect_samples=False) kept no sampled series"
            raise RuntimeError(msg)
        b = self._series_tick_edges(window_s, ticks_per_window, tick_edges)
        thr = self._series_thresholds(thresholds)
        ids, n_groups = self._window_groups(by)
        n_win, n_ser = int(b.shape[0] - 1), self.plan.n_series
        samples = self._samples_t
        dev = samples.device
        count = torch.empty((n_groups, n_win), dtype=torch.int32, device=dev)
        mean = torch.empty((n_groups, n_win, n_ser), dtype=torch.float64, device=dev)
        mn, mx, ab = (torch.empty((n_groups, n_win, n_ser), dtype=torch.int32, device=dev) for _ in range(3))
        grp = torch.from_numpy(np.where(ids < 0, _abi.POOL_SKIP, ids).astype(np.uint32).view(np.int32)).to(dev)
        torch.cuda.synchronize(dev)
        if self._summ_engine is None:
            self._summ_engine = Engine(self.plan, dev.index if dev.index is not None else torch.cuda.current_device())
        ms, scratch = self._summ_engine.summarize_series_windows(
            len(self), n_groups, b, samples_ptr=samples.data_ptr(), tick_capacity=int(samples.shape[1]),
            counts_ptr=self._counts_t.data_ptr(), count_ptr=count.data_ptr(), mean_ptr=mean.data_ptr(), min_ptr=mn.data_ptr(),
            max_ptr=mx.data_ptr(), above_ptr=ab.data_ptr(), group_ptr=grp.data_ptr(), thresholds=thr)
        cnt = count.to(torch.int64) & 0xFFFFFFFF
        ram = torch.as_tensor(ram_columns(n_ser, self.plan.n_edges), device=dev)
        empty = (cnt == 0)[:, :, None]
        nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)

        def decode(words: Any) -> Any:   # (as decode_series_max: counts as they are, the ram columns from their float32 bits)
            v = torch.where(ram, words.view(torch.float32).to(torch.float64), (words.to(torch.int64) & 0xFFFFFFFF).to(torch.float64))
            return torch.where(empty, nan, v)

        share = (ab.to(torch.int64) & 0xFFFFFFFF).to(torch.float64) / cnt.to(torch.float64)[:, :, None]
        return {"count": cnt, "mean": mean, "min": decode(mn), "max": decode(mx), "above_share": torch.where(empty, nan, share),
                "min_words": mn, "max_words": mx, "above": ab, "series": self.series_names(), "tick_edges": b,
                "times": b[:-1].astype(np.float64) * self.plan.sample_period,
                "replicas": np.bincount(ids[ids >= 0], minlength=n_groups), "series_window_ms": ms, "scratch_bytes": scratch}

    def series_window_bands(self, window_s: float | None = None, *, ticks_per_window: int | None = None,
                            tick_edges: Any = None, by: Any = None, thresholds: Any = None, of: str = "mean",
                            level: float = 0.95, q: tuple[float, float] = (0.05, 0.95)) -> dict[str, Any]:
        """Bands over the replicas of a windowed series statistic ``of`` (``"mean"``, ``"max"`` or ``"above_share"``): every
        scenario's own window values (``series_window_summary(by="scenario")``), then per group (``by``) and window, over
        the group's replicas whose window is not empty (``n`` [G, W] of them): ``mean``, unbiased ``std``, normal
        confidence half-width ``ci_halfwidth`` at ``level`` and the linear quantiles ``q_lo`` / ``q_hi`` (``q``), numpy
        float64 [G, W, S] each (NaN where no replica has a sample in the window; ``std`` NaN below two).  Reduced on the
        device (:func:`window_bands_by_group`); ``pooled`` is the grouped call's value of the same statistic."""
        if of not in ("mean", "max", "above_share"):
            msg = f"of must be 'mean', 'max' or 'above_share', not {of!r}"
            raise ValueError(msg)
        b = self._series_tick_edges(window_s, ticks_per_window, tick_edges)
        return self._series_window_bands(b, by, thresholds, of, level, q)[0]

    def _series_window_bands(self, b: np.ndarray, by: Any, thresholds: Any, of: str, level: float,
                             q: tuple[float, float]) -> tuple[dict[str, Any], dict[str, Any]]:
        """:meth:`series_window_bands` for resolved tick edges; also returns the grouped summary its ``pooled`` is taken from."""
        ids, n_groups = self._window_groups(by)
        per = self.series_window_summary(tick_edges=b, by="scenario", thresholds=thresholds)
        out = window_bands_by_group(per[of], ids, n_groups, level, q, valid=per["count"] > 0)
        pooled = self.series_window_summary(tick_edges=b, by=ids, thresholds=thresholds)
        out["pooled"] = pooled[of].cpu().numpy()[:n_groups]
        out.update(of=of, series=per["series"], tick_edges=b, times=per["times"])
        return out, pooled

    def save_series_window_summary(self, path: str, by: Any = None, *, window_s: float | None = None,
                                   ticks_per_window: int | None = None, thresholds: Any = None,
                                   level: float = 0.95) -> dict[str, np.ndarray]:
        """Columnar dump of the windowed series statistics with one row per group (grid point): ``param:<axis>`` (for a
        Sweep), ``replicas``, and per series the [G, W] columns ``series_window_mean:<series>``,
        ``series_window_max:<series>``, ``series_window_above:<series>`` (the share above the threshold) -- the group's
        replicas taken together -- and ``series_window_q05:<series>`` / ``series_window_q95:<series>`` (of the replicas'
        own means, :meth:`series_window_bands`); ``series_window_tick_edges`` [W + 1] and ``series_window_times`` [W] are
        per-file vectors.  ``.npz`` or ``.parquet``; :func:`load_summary` reads it back."""
        b = self._series_tick_edges(window_s, ticks_per_window, None)
        bands, pooled = self._series_window_bands(b, by, thresholds, "mean", level, (0.05, 0.95))
        n_groups = int(bands["replicas"].shape[0])
        cols: dict[str, np.ndarray] = {}
        if hasattr(by, "point_columns"):
            for k, v in by.point_columns().items():
                cols[f"param:{k}"] = np.asarray(v, dtype=np.float64)
        cols["replicas"] = np.asarray(bands["replicas"], dtype=np.int64)
        mean, mx, share = (pooled[k].cpu().numpy()[:n_groups] for k in ("mean", "max", "above_share"))
        for j, name in enumerate(bands["series"]):
            cols[f"series_window_mean:{name}"] = np.ascontiguousarray(mean[:, :, j])
            cols[f"series_window_max:{name}"] = np.ascontiguousarray(mx[:, :, j])
            cols[f"series_window_above:{name}"] = np.ascontiguousarray(share[:, :, j])
            cols[f"series_window_q05:{name}"] = np.ascontiguousarray(bands["q_lo"][:, :, j])
            cols[f"series_window_q95:{name}"] = np.ascontiguousarray(bands["q_hi"][:, :, j])
        cols["series_window_tick_edges"] = np.asarray(bands["tick_edges"], dtype=np.float64)
        cols["series_window_times"] = np.asarray(bands["times"], dtype=np.float64)
        _write_columns(str(path), cols, n_groups)
        return cols

    def _require_samples(self) -> None:
        if self._samples_t is None:
            msg = "run(collect_samples=False) kept no sampled series"
            raise RuntimeError(msg)

    def _series_columns(self, series: Any) -> np.ndarray:
        """``series`` (None, names of :meth:`series_names` or indices) as series indices."""
        names = self.series_names()
        if series is None:
            return np.arange(len(names), dtype=np.int64)
        if isinstance(series, (str, bytes)):
            series = [series]
        items = list(series)
        if any(isinstance(x, str) for x in items):
            for x in items:
                if x not in names:
                    msg = f"unknown series {x!r} (series_names(): {names})"
                    raise ValueError(msg)
            items = [names.index(x) for x in items]
        return _check_series_columns(np.asarray(items), len(names))

    def series_quantile_summary(self, levels: Any, window_s: float | None = None, *, ticks_per_window: int | None = None,
                                tick_edges: Any = None, by: Any = None, series: Any = None) -> dict[str, Any]:
        """Exact quantiles of the sampled series of every (group, window of ticks, series), over all scenarios of the
        group: how much RAM covers 99 % of the ticks during an outage, the median ready-queue length of every 10 s window,
        the p95 of edge concurrency.  Computed by the HIP analyzer ``af_engine_summarize_series_quantiles``, bit-equal to
        :func:`series_window_quantiles` on the group's samples side by side.  ``levels`` in [0, 1], at most 16, any order;
        windows and ``by`` as in :meth:`series_window_summary`; ``series``: None (all), names from :meth:`series_names`
        or indices, any order, duplicates allowed.  Returns torch tensors on the run's device: ``quantiles`` float64
        [G, W, C, Q] (NaN in empty cells) and ``count`` int64 [G, W]; and ``levels``, ``series`` (the selected names),
        ``tick_edges``, ``times``, ``replicas`` [G], ``series_quantile_ms``, ``scratch_bytes``."""
        import torch

        from .engine import Engine

        self._require_samples()
        q = check_series_levels(levels)
        col = self._series_columns(series)
        b = self._series_tick_edges(window_s, ticks_per_window, tick_edges)
        ids, n_groups = self._window_groups(by)
        n_win = int(b.shape[0] - 1)
        samples = self._samples_t
        dev = samples.device
        count = torch.empty((n_groups, n_win), dtype=torch.int32, device=dev)
        quant = torch.empty((n_groups, n_win, col.shape[0], q.shape[0]), dtype=torch.float64, device=dev)
        grp = torch.from_numpy(np.where(ids < 0, _abi.POOL_SKIP, ids).astype(np.uint32).view(np.int32)).to(dev)
        torch.cuda.synchronize(dev)
        if self._summ_engine is None:
            self._summ_engine = Engine(self.plan, dev.index if dev.index is not None else torch.cuda.current_device())
        ms, scratch = self._summ_engine.summarize_series_quantiles(
            len(self), n_groups, b, q, samples_ptr=samples.data_ptr(), tick_capacity=int(samples.shape[1]),
            counts_ptr=self._counts_t.data_ptr(), count_ptr=count.data_ptr(), quantiles_ptr=quant.data_ptr(),
            group_ptr=grp.data_ptr(), columns=None if series is None else col)
        names = self.series_names()
        return {"quantiles": quant, "count": count.to(torch.int64) & 0xFFFFFFFF, "levels": q, "series": [names[j] for j in col],
                "tick_edges": b, "times": b[:-1].astype(np.float64) * self.plan.sample_period,
                "replicas": np.bincount(ids[ids >= 0], minlength=n_groups), "series_quantile_ms": ms, "scratch_bytes": scratch}

    def series_quantile_bands(self, levels: Any, window_s: float | None = None, *, ticks_per_window: int | None = None,
                              tick_edges: Any = None, by: Any = None, series: Any = None, level: float = 0.95,
                              q: tuple[float, float] = (0.05, 0.95)) -> dict[str, Any]:
        """Bands over the replicas of the series quantiles: every scenario's own values
        (``series_quantile_summary(by="scenario")``), then per group (``by``) and window, over the group's replicas whose
        window is not empty (``n`` [G, W] of them), ``mean``, ``std``, ``ci_halfwidth`` (at ``level``) and the linear
        quantiles ``q_lo`` / ``q_hi`` (``q``) as :func:`window_bands_by_group` gives them: numpy float64 [G, W, C, Q].
        ``pooled`` [G, W, C, Q] and ``pooled_count`` [G, W] are ``series_quantile_summary(by=by)`` as numpy.
        The bands are reduced on the HOST from the device's per-scenario quantiles: there the sums over the replicas run
        in scenario order, so the bands, like the quantiles, are the same bits in every run (a device ``index_add_`` adds
        floats atomically, in no fixed order)."""
        self._require_samples()
        b = self._series_tick_edges(window_s, ticks_per_window, tick_edges)
        ids, n_groups = self._window_groups(by)
        per = self.series_quantile_summary(levels, tick_edges=b, by="scenario", series=series)
        shape = tuple(per["quantiles"].shape[2:])
        out = window_bands_by_group(per["quantiles"].flatten(2).cpu(), ids, n_groups, level, q, valid=(per["count"] > 0).cpu())
        for k in ("mean", "std", "ci_halfwidth", "q_lo", "q_hi"):
            out[k] = out[k].reshape(out[k].shape[:2] + shape)
        pooled = self.series_quantile_summary(levels, tick_edges=b, by=ids, series=series)
        out["pooled"] = pooled["quantiles"].cpu().numpy()[:n_groups]
        out["pooled_count"] = pooled["count"].cpu().numpy()[:n_groups]
        out.update(levels=per["levels"], series=per["series"], tick_edges=b, times=per["times"])
        return out

    def save_series_quantile_summary(self, path: str, by: Any = None, *, levels: Any, series: Any = None,
                                     window_s: float | None = None, ticks_per_window: int | None = None) -> dict[str, np.ndarray]:
        """Columnar dump of the series quantiles with one row per group (grid point): ``param:<axis>`` (for a Sweep),
        ``replicas``, ``series_quantile_count`` [G, W] and per selected series and level the [G, W] column
        ``series_quantile:<series>:<level>`` (the group's replicas taken together; ``<level>`` as ``repr(float)``);
        ``series_quantile_tick_edges`` [W + 1], ``series_quantile_times`` [W] and ``series_quantile_levels`` [Q] are
        per-file vectors.  ``.npz`` or ``.parquet``; :func:`load_summary` reads it back."""
        self._require_samples()
        b = self._series_tick_edges(window_s, ticks_per_window, None)
        ids, n_groups = self._window_groups(by)
        pooled = self.series_quantile_summary(levels, tick_edges=b, by=ids, series=series)
        cols: dict[str, np.ndarray] = {}
        if hasattr(by, "point_columns"):
            for k, v in by.point_columns().items():
                cols[f"param:{k}"] = np.asarray(v, dtype=np.float64)
        cols["replicas"] = np.asarray(pooled["replicas"], dtype=np.int64)
        cols["series_quantile_count"] = np.ascontiguousarray(pooled["count"].cpu().numpy()[:n_groups], dtype=np.int64)
        quant = pooled["quantiles"].cpu().numpy()[:n_groups]
        for c, name in enumerate(pooled["series"]):
            for i, lv in enumerate(pooled["levels"]):
                cols[f"series_quantile:{name}:{float(lv)!r}"] = np.ascontiguousarray(quant[:, :, c, i])
        cols["series_quantile_tick_edges"] = np.asarray(b, dtype=np.float64)
        cols["series_quantile_times"] = np.asarray(pooled["times"], dtype=np.float64)
        cols["series_quantile_levels"] = np.asarray(pooled["levels"], dtype=np.float64)
        _write_columns(str(path), cols, n_groups)
        return cols

    #: what :meth:`series_excursion_bands` gives bands of
    EXCURSION_BANDS = ("longest_s", "above_s", "runs", "first_s", "recovered_s", "peak_s")

    def _series_excursion_edges(self, window_s: float | None, ticks_per_window: int | None, tick_edges: Any) -> np.ndarray:
        if window_s is None and ticks_per_window is None and tick_edges is None:
            tick_edges = [0, max(self.plan.tick_count, 1)]
        return self._series_tick_edges(window_s, ticks_per_window, tick_edges)

    def series_excursion_summary(self, thresholds: Any, window_s: float | None = None, *, ticks_per_window: int | None = None,
                                 tick_edges: Any = None) -> dict[str, Any]:
        """Excursions of every sampled series above a threshold, per SCENARIO and window of ticks: how long a server's
        ready queue stayed above 50 after another went down, when it had come back (and whether it had by the end of the
        window), how many separate backlogs formed, when the peak was.  Computed by the HIP analyzer
        ``af_engine_summarize_series_excursions`` in one pass over the sample rows, equal word for word to
        :func:`series_window_excursions` of every scenario.  A tick is above when its value ``> threshold``; a run is a
        maximal stretch of consecutive above ticks inside a window (clipped at its edges).  ``thresholds``: None (0.0), a
        vector [n_series] or ``{series name: value}`` over :meth:`series_names` (missing: 0.0).  Windows: ``window_s``
        seconds, ``ticks_per_window`` ticks or explicit ``tick_edges`` as in :meth:`series_window_summary` -- but WITH NONE
        OF THE THREE GIVEN, ONE WINDOW OVER THE WHOLE RUN, ``[0, plan.tick_count]`` (the sibling methods default to windows
        of 1 s).  Returns torch tensors on the run's device: ``count`` int64 [n, W]; ``above``, ``runs``, ``longest`` (ticks),
        ``longest_start``, ``first``, ``last``, ``peak_tick`` (tick indices, -1: none) int64 [n, W, S]; float64 [n, W, S] in
        seconds with the label of ``get_series``, tick ``k`` at ``k * sample_period``: ``above_s``, ``longest_s`` (ticks x
        period), ``first_s``, ``peak_s`` (NaN: none) and ``recovered_s`` = ``(last + 1) * period``, NaN where the series
        never exceeded the threshold AND where the window ends above it; bool [n, W, S]: ``exceeded`` and ``open`` (still
        above at the window's last tick).  And ``series``, ``thresholds``, ``tick_edges``, ``times`` (the windows' start labels
        in seconds), ``series_excursion_ms``, ``scratch_bytes``."""
        import torch

        from .engine import Engine

        thr = self._series_thresholds(thresholds)
        self._require_samples()
        b = self._series_excursion_edges(window_s, ticks_per_window, tick_edges)
        n, n_win, n_ser = len(self), int(b.shape[0] - 1), self.plan.n_series
        samples = self._samples_t
        dev = samples.device
        raw = {k: torch.empty((n, n_win) if k == "count" else (n, n_win, n_ser), dtype=torch.int32, device=dev)
               for k in Engine.EXCURSION_OUTPUTS}
        torch.cuda.synchronize(dev)
        if self._summ_engine is None:
            self._summ_engine = Engine(self.plan, dev.index if dev.index is not None else torch.cuda.current_device())
        ms, scratch = self._summ_engine.summarize_series_excursions(
            n, b, samples_ptr=samples.data_ptr(), tick_capacity=int(samples.shape[1]), counts_ptr=self._counts_t.data_ptr(),
            thresholds=thr, **{f"{k}_ptr": v.data_ptr() for k, v in raw.items()})
        out: dict[str, Any] = {k: raw[k].to(torch.int64) & 0xFFFFFFFF for k in ("count", "above", "runs", "longest")}
        for k in ("longest_start", "first", "last", "peak_tick"):
            out[k] = raw[k].to(torch.int64)              # (0xFFFFFFFF is -1; a tick is below 2^31)
        period = float(self.plan.sample_period)
        nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
        m = (self._counts_t[:, _abi.CNT_TICKS].to(torch.int64) & 0xFFFFFFFF).clamp(max=int(samples.shape[1]))
        hi = torch.minimum(torch.as_tensor(b[1:].astype(np.int64), device=dev)[None, :], m[:, None])      # [n, W]
        exceeded = out["first"] >= 0
        still = exceeded & (out["last"] == (hi - 1)[:, :, None])
        out["above_s"] = out["above"].to(torch.float64) * period
        out["longest_s"] = out["longest"].to(torch.float64) * period
        out["first_s"] = torch.where(exceeded, out["first"].to(torch.float64) * period, nan)
        out["peak_s"] = torch.where(out["peak_tick"] >= 0, out["peak_tick"].to(torch.float64) * period, nan)
        out["recovered_s"] = torch.where(exceeded & ~still, (out["last"] + 1).to(torch.float64) * period, nan)
        out["open"], out["exceeded"] = still, exceeded
        out.update(series=self.series_names(), thresholds=np.zeros(n_ser) if thr is None else thr, tick_edges=b,
                   times=b[:-1].astype(np.float64) * period, series_excursion_ms=ms, scratch_bytes=scratch)
        return out

    def series_excursion_bands(self, thresholds: Any, window_s: float | None = None, *, ticks_per_window: int | None = None,
                               tick_edges: Any = None, by: Any = None, of: str = "longest_s", level: float = 0.95,
                               q: tuple[float, float] = (0.05, 0.95)) -> dict[str, Any]:
        """Bands over the replicas of an excursion statistic ``of`` -- ``"longest_s"``, ``"above_s"``, ``"runs"``,
        ``"first_s"``, ``"recovered_s"`` or ``"peak_s"`` of :meth:`series_excursion_summary` --: per group (``by`` as in
        :meth:`window_summary`), window and series, over the group's replicas that are VALID there, ``mean``, unbiased
        ``std``, ``ci_halfwidth`` at ``level`` and the linear quantiles ``q_lo`` / ``q_hi`` (``q``) as
        :func:`window_bands_by_group` gives them, numpy float64 [G, W, S], and ``n`` [G, W, S], the valid replicas.  Valid:
        a non-empty window (``count > 0``) for ``longest_s``, ``above_s``, ``runs`` and ``peak_s``; ``exceeded`` for
        ``first_s``; ``exceeded & ~open`` -- the replicas that came back inside the window -- for ``recovered_s``.  Also
        ``exceed_share`` and ``open_share`` [G, W, S]: the members that exceeded the threshold / are still above it at the
        window's end, divided by the members with a non-empty window (NaN where there is none).  Windows and their
        default (one window over the whole run) as in :meth:`series_excursion_summary`."""
        if of not in self.EXCURSION_BANDS:
            msg = f"of must be one of {', '.join(repr(k) for k in self.EXCURSION_BANDS)}, not {of!r}"
            raise ValueError(msg)
        per = self.series_excursion_summary(thresholds, window_s, ticks_per_window=ticks_per_window, tick_edges=tick_edges)
        ids, n_groups = self._window_groups(by)
        return self._series_excursion_bands(per, ids, n_groups, of, level, q)

    def _series_excursion_bands(self, per: dict[str, Any], ids: np.ndarray, n_groups: int, of: str, level: float,
                                q: tuple[float, float], shares: bool = True) -> dict[str, Any]:
        """:meth:`series_excursion_bands` of a computed per-scenario summary ``per`` (``shares=False``: without the two
        shares, which do not depend on ``of``)."""
        import torch

        live = per["count"] > 0                                           # [n, W]
        valid = {"first_s": per["exceeded"], "recovered_s": per["exceeded"] & ~per["open"]}.get(of)
        values = per[of].to(torch.float64)
        n, n_win, n_ser = (int(x) for x in values.shape)
        shape = (n_groups, n_win, n_ser)
        if valid is None:
            out = window_bands_by_group(values, ids, n_groups, level, q, valid=live)
            out["n"] = np.repeat(out["n"][:, :, None], n_ser, axis=2)
        else:   # valid per series: every (window, series) pair a window of its own with one column -- one call, one sort
            out = window_bands_by_group(values.reshape(n, n_win * n_ser, 1), ids, n_groups, level, q, valid=valid.reshape(n, n_win * n_ser))
            for k in ("n", "mean", "std", "ci_halfwidth", "q_lo", "q_hi"):
                out[k] = out[k].reshape(shape)
        if shares:
            out.update(self._series_excursion_shares(per, ids, n_groups))
        out.update(of=of, series=per["series"], thresholds=per["thresholds"], tick_edges=per["tick_edges"], times=per["times"])
        return out

    @staticmethod
    def _series_excursion_shares(per: dict[str, Any], ids: np.ndarray, n_groups: int) -> dict[str, np.ndarray]:
        """``exceed_share`` / ``open_share`` [G, W, S]: integer member counts (exact in any order), divided once."""
        import torch

        live = per["count"] > 0
        dev = live.device
        n_win, n_ser = int(live.shape[1]), int(per["exceeded"].shape[2])
        gid = torch.as_tensor(ids, device=dev)
        ok = (gid >= 0)[:, None] & live                                   # (an open or exceeded window is not empty)
        cell = (gid[:, None] * n_win + torch.arange(n_win, device=dev)[None, :])[ok]
        base = torch.bincount(cell, minlength=n_groups * n_win).to(torch.float64)[:, None]
        out = {}
        for name, mask in (("exceed_share", per["exceeded"]), ("open_share", per["open"])):
            members = torch.zeros((n_groups * n_win, n_ser), dtype=torch.int64, device=dev).index_add_(0, cell, mask[ok].to(torch.int64))
            out[name] = (members.to(torch.float64) / base).reshape(n_groups, n_win, n_ser).cpu().numpy()   # (0 / 0: NaN)
        return out

    def save_series_excursion_summary(self, path: str, by: Any = None, *, thresholds: Any, window_s: float | None = None,
                                      ticks_per_window: int | None = None, tick_edges: Any = None,
                                      level: float = 0.95) -> dict[str, np.ndarray]:
        """Columnar dump of the excursions with one row per group (grid point): ``param:<axis>`` (for a Sweep),
        ``replicas``, and per series the [G, W] columns ``series_excursion_longest_s:<series>`` (the mean over the replicas
        of their longest run in seconds), ``series_excursion_q05:<series>`` / ``series_excursion_q95:<series>`` (its
        quantiles over the replicas), ``series_excursion_recovered_s:<series>`` (the mean recovery label over the replicas
        that came back inside the window), ``series_excursion_exceed_share:<series>`` and
        ``series_excursion_open_share:<series>`` (:meth:`series_excursion_bands`); ``series_excursion_tick_edges`` [W + 1],
        ``series_excursion_times`` [W] and ``series_excursion_thresholds`` [S] are per-file vectors.  Windows as in
        :meth:`series_excursion_summary`.  ``.npz`` or ``.parquet``; :func:`load_summary` reads it back."""
        per = self.series_excursion_summary(thresholds, window_s, ticks_per_window=ticks_per_window, tick_edges=tick_edges)
        ids, n_groups = self._window_groups(by)
        longest = self._series_excursion_bands(per, ids, n_groups, "longest_s", level, (0.05, 0.95))
        back = self._series_excursion_bands(per, ids, n_groups, "recovered_s", level, (0.05, 0.95), shares=False)
        cols: dict[str, np.ndarray] = {}
        if hasattr(by, "point_columns"):
            for k, v in by.point_columns().items():
                cols[f"param:{k}"] = np.asarray(v, dtype=np.float64)
        cols["replicas"] = np.asarray(longest["replicas"], dtype=np.int64)
        for j, name in enumerate(per["series"]):
            cols[f"series_excursion_longest_s:{name}"] = np.ascontiguousarray(longest["mean"][:, :, j])
            cols[f"series_excursion_q05:{name}"] = np.ascontiguousarray(longest["q_lo"][:, :, j])
            cols[f"series_excursion_q95:{name}"] = np.ascontiguousarray(longest["q_hi"][:, :, j])
            cols[f"series_excursion_recovered_s:{name}"] = np.ascontiguousarray(back["mean"][:, :, j])
            cols[f"series_excursion_exceed_share:{name}"] = np.ascontiguousarray(longest["exceed_share"][:, :, j])
            cols[f"series_excursion_open_share:{name}"] = np.ascontiguousarray(longest["open_share"][:, :, j])
        cols["series_excursion_tick_edges"] = np.asarray(per["tick_edges"], dtype=np.float64)
        cols["series_excursion_times"] = np.asarray(per["times"], dtype=np.float64)
        cols["series_excursion_thresholds"] = np.asarray(per["thresholds"], dtype=np.float64)
        _write_columns(str(path), cols, n_groups)
        return cols

    def _series_binning(self, name: str, value: Any, col: np.ndarray, default: float) -> Any:
        """``lo`` / ``width`` of a histogram call -- None, a scalar, one value per selected series or ``{series name:
        value}`` (missing: the default) -- as None, a scalar or a vector per selected series."""
        if not isinstance(value, dict):
            return value
        names = self.series_names()
        for k in value:
            if k not in names:
                msg = f"unknown series {k!r} in {name} (series_names(): {names})"
                raise ValueError(msg)
        return np.array([float(value.get(names[j], default)) for j in col], dtype=np.float64)

    def series_histogram_summary(self, bins: int = 64, window_s: float | None = None, *, ticks_per_window: int | None = None,
                                 tick_edges: Any = None, by: Any = None, series: Any = None, lo: Any = None,
                                 width: Any = None) -> dict[str, Any]:
        """Occupancy histograms of the sampled series of every (group, window of ticks, selected series), over all scenarios
        of the group: P(ready queue length = k) per window and grid point.  Computed by the HIP analyzer
        ``af_engine_summarize_series_histogram`` in one pass over the sample rows, equal word for word to
        :func:`series_window_histogram` of the group's scenarios added up.  Windows and ``by`` as in
        :meth:`series_window_summary`; ``series`` as in :meth:`series_quantile_summary` (the same series may appear twice
        with two binnings); ``lo`` / ``width``: None (0.0 / 1.0: the bin of a count is the count), a scalar, one value per
        selected series or ``{series name: value}``.  Returns torch tensors on the run's device: ``hist`` int64 [G, W, C,
        bins], ``under``, ``over`` [G, W, C] (the values below ``lo`` / at or past ``lo + bins * width``) and ``count`` [G,
        W], ``under + hist.sum(-1) + over == count``; and ``bin_edges`` float64 [C, bins + 1], ``ram`` bool [C], ``series``
        (the selected names), ``tick_edges``, ``times``, ``replicas`` [G], ``series_histogram_ms``, ``scratch_bytes``.
        :func:`series_histogram_quantiles` reads quantiles off the result."""
        import torch

        from .engine import Engine

        self._require_samples()
        col = self._series_columns(series)
        n_col = int(col.shape[0])
        n_bins, lo_v, width_v = check_series_bins(bins, n_col, self._series_binning("lo", lo, col, 0.0),
                                                  self._series_binning("width", width, col, 1.0))
        b = self._series_tick_edges(window_s, ticks_per_window, tick_edges)
        ids, n_groups = self._window_groups(by)
        n_win = int(b.shape[0] - 1)
        samples = self._samples_t
        dev = samples.device
        count = torch.empty((n_groups, n_win), dtype=torch.int32, device=dev)
        hist = torch.empty((n_groups, n_win, n_col, n_bins), dtype=torch.int32, device=dev)
        under, over = (torch.empty((n_groups, n_win, n_col), dtype=torch.int32, device=dev) for _ in range(2))
        grp = torch.from_numpy(np.where(ids < 0, _abi.POOL_SKIP, ids).astype(np.uint32).view(np.int32)).to(dev)
        torch.cuda.synchronize(dev)
        if self._summ_engine is None:
            self._summ_engine = Engine(self.plan, dev.index if dev.index is not None else torch.cuda.current_device())
        plain = lo is None and width is None
        ms, scratch = self._summ_engine.summarize_series_histogram(
            len(self), n_groups, b, n_bins, samples_ptr=samples.data_ptr(), tick_capacity=int(samples.shape[1]),
            counts_ptr=self._counts_t.data_ptr(), count_ptr=count.data_ptr(), hist_ptr=hist.data_ptr(),
            under_ptr=under.data_ptr(), over_ptr=over.data_ptr(), group_ptr=grp.data_ptr(),
            columns=None if series is None else col, lo=None if plain else lo_v, width=None if plain else width_v)
        names = self.series_names()
        return {"hist": hist.to(torch.int64) & 0xFFFFFFFF, "under": under.to(torch.int64) & 0xFFFFFFFF,
                "over": over.to(torch.int64) & 0xFFFFFFFF, "count": count.to(torch.int64) & 0xFFFFFFFF,
                "bin_edges": lo_v[:, None] + np.arange(n_bins + 1, dtype=np.float64)[None, :] * width_v[:, None],
                "ram": ram_columns(self.plan.n_series, self.plan.n_edges)[col], "series": [names[j] for j in col],
                "tick_edges": b, "times": b[:-1].astype(np.float64) * self.plan.sample_period,
                "replicas": np.bincount(ids[ids >= 0], minlength=n_groups), "series_histogram_ms": ms, "scratch_bytes": scratch}

    def series_histogram_bands(self, bins: int = 64, window_s: float | None = None, *, ticks_per_window: int | None = None,
                               tick_edges: Any = None, by: Any = None, series: Any = None, lo: Any = None, width: Any = None,
                               level: float = 0.95, q: tuple[float, float] = (0.05, 0.95)) -> dict[str, Any]:
        """Bands over the replicas of the histogram SHARES: every scenario's own ``hist / count``
        (``series_histogram_summary(by="scenario")``), then per group (``by``) and window, over the group's replicas whose
        window is not empty (``n`` [G, W] of them), ``mean``, ``std``, ``ci_halfwidth`` (at ``level``) and the linear
        quantiles ``q_lo`` / ``q_hi`` (``q``) as :func:`window_bands_by_group` gives them: numpy float64 [G, W, C, bins].
        ``pooled`` [G, W, C, bins], ``pooled_under`` / ``pooled_over`` [G, W, C] and ``pooled_count`` [G, W] are the
        histogram of the group's replicas taken together (``series_histogram_summary(by=by)``) as numpy int64.  Reduced on
        the host, in scenario order, as :meth:`series_quantile_bands` is."""
        import torch

        self._require_samples()
        b = self._series_tick_edges(window_s, ticks_per_window, tick_edges)
        ids, n_groups = self._window_groups(by)
        per = self.series_histogram_summary(bins, tick_edges=b, by="scenario", series=series, lo=lo, width=width)
        shape = tuple(per["hist"].shape[2:])
        cnt = per["count"].cpu()
        share = per["hist"].cpu().to(torch.float64) / cnt.to(torch.float64)[:, :, None, None]   # (0 / 0: NaN, not valid)
        out = window_bands_by_group(share.flatten(2), ids, n_groups, level, q, valid=cnt > 0)
        for k in ("mean", "std", "ci_halfwidth", "q_lo", "q_hi"):
            out[k] = out[k].reshape(out[k].shape[:2] + shape)
        pooled = self.series_histogram_summary(bins, tick_edges=b, by=ids, series=series, lo=lo, width=width)
        out["pooled"] = pooled["hist"].cpu().numpy()[:n_groups]
        for k in ("under", "over", "count"):
            out[f"pooled_{k}"] = pooled[k].cpu().numpy()[:n_groups]
        out.update(bin_edges=per["bin_edges"], ram=per["ram"], series=per["series"], tick_edges=b, times=per["times"])
        return out

    def save_series_histogram_summary(self, path: str, by: Any = None, *, bins: int = 64, series: Any = None, lo: Any = None,
                                      width: Any = None, window_s: float | None = None, ticks_per_window: int | None = None,
                                      tick_edges: Any = None) -> dict[str, np.ndarray]:
        """Columnar dump of the series histograms with one row per group (grid point): ``param:<axis>`` (for a Sweep),
        ``replicas``, ``series_hist_count`` [G, W] and per selected series ``series_hist:<series>`` [G, W, bins],
        ``series_hist_under:<series>`` and ``series_hist_over:<series>`` [G, W] (the group's replicas taken together) and
        the per-file vector ``series_hist_bin_edges:<series>`` [bins + 1]; ``series_hist_tick_edges`` [W + 1] and
        ``series_hist_times`` [W] are per-file vectors too.  A series may be selected once.  ``.npz`` or ``.parquet``;
        :func:`load_summary` reads it back."""
        self._require_samples()
        b = self._series_tick_edges(window_s, ticks_per_window, tick_edges)
        ids, n_groups = self._window_groups(by)
        pooled = self.series_histogram_summary(bins, tick_edges=b, by=ids, series=series, lo=lo, width=width)
        if len(set(pooled["series"])) != len(pooled["series"]):
            msg = "a series may be selected once in a saved histogram summary (the columns are named after it)"
            raise ValueError(msg)
        cols: dict[str, np.ndarray] = {}
        if hasattr(by, "point_columns"):
            for k, v in by.point_columns().items():
                cols[f"param:{k}"] = np.asarray(v, dtype=np.float64)
        cols["replicas"] = np.asarray(pooled["replicas"], dtype=np.int64)
        cols["series_hist_count"] = np.ascontiguousarray(pooled["count"].cpu().numpy()[:n_groups], dtype=np.int64)
        hist, under, over = (pooled[k].cpu().numpy()[:n_groups] for k in ("hist", "under", "over"))
        for c, name in enumerate(pooled["series"]):
            cols[f"series_hist:{name}"] = np.ascontiguousarray(hist[:, :, c], dtype=np.int64)
            cols[f"series_hist_under:{name}"] = np.ascontiguousarray(under[:, :, c], dtype=np.int64)
            cols[f"series_hist_over:{name}"] = np.ascontiguousarray(over[:, :, c], dtype=np.int64)
            cols[f"series_hist_bin_edges:{name}"] = np.ascontiguousarray(pooled["bin_edges"][c], dtype=np.float64)
        cols["series_hist_tick_edges"] = np.asarray(b, dtype=np.float64)
        cols["series_hist_times"] = np.asarray(pooled["times"], dtype=np.float64)
        _write_columns(str(path), cols, n_groups)
        return cols

    def _combined_thresholds(self, thresholds: Any, labels: list[str]) -> np.ndarray | None:
        """``thresholds`` of a combined call -- None, one value per combination or ``{label: value}`` (missing: 0.0)."""
        if thresholds is None:
            return None
        if isinstance(thresholds, dict):
            for k in thresholds:
                if k not in labels:
                    msg = f"unknown combination {k!r} in thresholds (combinations: {labels})"
                    raise ValueError(msg)
            thr = np.array([float(thresholds.get(k, 0.0)) for k in labels], dtype=np.float64)
        else:
            thr = np.asarray(thresholds, dtype=np.float64)
        if thr.shape != (len(labels),) or np.isnan(thr).any():
            msg = f"thresholds must be one value per combination ({len(labels)}) or a dict, none of them NaN"
            raise ValueError(msg)
        return thr

    def series_combined_summary(self, combos: Any, window_s: float | None = None, *, ticks_per_window: int | None = None,
                                tick_edges: Any = None, by: Any = None, thresholds: Any = None, bins: int = 0, lo: Any = None,
                                width: Any = None) -> dict[str, Any]:
        """Combinations ACROSS the sampled series per tick -- the RAM of the whole fleet, the requests queued on all servers,
        the imbalance (max - min) between the servers' queues -- and their statistics per (group, window of ticks), over all
        scenarios of the group.  ``combos`` is ``{label: (op, selection)}``: ``op`` one of ``"sum"``, ``"min"``, ``"max"``,
        ``"spread"``; ``selection`` series names or indices, one ``fnmatch`` pattern over :meth:`series_names` or a list of
        patterns (:func:`check_series_combinations`).  Computed by the HIP analyzer
        ``af_engine_summarize_series_combined`` in one pass over the sample rows, equal to
        :func:`series_combined_window_stats` of the group's scenarios taken together.  Windows and ``by`` as in
        :meth:`series_window_summary`; ``thresholds``: None (0.0), one value per combination or ``{label: value}``;
        ``bins`` above 0 adds occupancy histograms of the per-tick values with ``lo`` / ``width`` (None: 0.0 / 1.0, a scalar
        or one value per combination).  Returns torch tensors on the run's device: ``count`` int64 [G, W]; ``mean``,
        ``min``, ``max`` and ``above_share`` float64 [G, W, C], NaN in empty cells; ``above`` int64 [G, W, C]; with ``bins``
        ``hist`` int64 [G, W, C, bins], ``under``, ``over`` [G, W, C], ``bin_edges`` float64 [C, bins + 1] and ``ram``
        bool [C], which :func:`series_histogram_quantiles` reads exact quantiles of an integer combination off; and
        ``names``, ``ops``, ``columns``, ``tick_edges``, ``times``, ``replicas`` [G], ``series_combined_ms``,
        ``scratch_bytes``."""
        import torch

        from .engine import Engine

        self._require_samples()
        labels, ops, columns = check_series_combinations(combos, self.series_names(), self.plan.n_edges)
        n_c = len(labels)
        thr = self._combined_thresholds(thresholds, labels)
        n_bins = 0
        if bins or lo is not None or width is not None:
            n_bins, lo_v, width_v = check_series_bins(bins, n_c, lo, width)
        b = self._series_tick_edges(window_s, ticks_per_window, tick_edges)
        ids, n_groups = self._window_groups(by)
        n_win = int(b.shape[0] - 1)
        samples = self._samples_t
        dev = samples.device
        count = torch.empty((n_groups, n_win), dtype=torch.int32, device=dev)
        mean, mn, mx = (torch.empty((n_groups, n_win, n_c), dtype=torch.float64, device=dev) for _ in range(3))
        ab = torch.empty((n_groups, n_win, n_c), dtype=torch.int32, device=dev)
        hist = under = over = None
        if n_bins:
            hist = torch.empty((n_groups, n_win, n_c, n_bins), dtype=torch.int32, device=dev)
            under, over = (torch.empty((n_groups, n_win, n_c), dtype=torch.int32, device=dev) for _ in range(2))
        grp = torch.from_numpy(np.where(ids < 0, _abi.POOL_SKIP, ids).astype(np.uint32).view(np.int32)).to(dev)
        torch.cuda.synchronize(dev)
        if self._summ_engine is None:
            self._summ_engine = Engine(self.plan, dev.index if dev.index is not None else torch.cuda.current_device())
        ms, scratch = self._summ_engine.summarize_series_combined(
            len(self), n_groups, b, [_abi.COMBINE_OPS[o] for o in ops], columns, samples_ptr=samples.data_ptr(),
            tick_capacity=int(samples.shape[1]), counts_ptr=self._counts_t.data_ptr(), mean_ptr=mean.data_ptr(),
            count_ptr=count.data_ptr(), min_ptr=mn.data_ptr(), max_ptr=mx.data_ptr(), above_ptr=ab.data_ptr(),
            hist_ptr=hist.data_ptr() if n_bins else 0, under_ptr=under.data_ptr() if n_bins else 0,
            over_ptr=over.data_ptr() if n_bins else 0, group_ptr=grp.data_ptr(), thresholds=thr, bins=n_bins,
            lo=lo_v if n_bins and not (lo is None and width is None) else None,
            width=width_v if n_bins and not (lo is None and width is None) else None)
        cnt = count.to(torch.int64) & 0xFFFFFFFF
        above = ab.to(torch.int64) & 0xFFFFFFFF
        nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
        share = torch.where((cnt == 0)[:, :, None], nan, above.to(torch.float64) / cnt.to(torch.float64)[:, :, None])
        ram = ram_columns(self.plan.n_series, self.plan.n_edges)
        out = {"count": cnt, "mean": mean, "min": mn, "max": mx, "above": above, "above_share": share}
        if n_bins:
            out.update(hist=hist.to(torch.int64) & 0xFFFFFFFF, under=under.to(torch.int64) & 0xFFFFFFFF,
                       over=over.to(torch.int64) & 0xFFFFFFFF,
                       bin_edges=lo_v[:, None] + np.arange(n_bins + 1, dtype=np.float64)[None, :] * width_v[:, None],
                       ram=np.array([bool(ram[c[0]]) for c in columns], dtype=bool))
        out.update(names=labels, ops=ops, columns=columns, tick_edges=b, times=b[:-1].astype(np.float64) * self.plan.sample_period,
                   replicas=np.bincount(ids[ids >= 0], minlength=n_groups), series_combined_ms=ms, scratch_bytes=scratch)
        return out

    def series_combined_bands(self, combos: Any, window_s: float | None = None, *, ticks_per_window: int | None = None,
                              tick_edges: Any = None, by: Any = None, thresholds: Any = None, of: str = "mean",
                              level: float = 0.95, q: tuple[float, float] = (0.05, 0.95)) -> dict[str, Any]:
        """Bands over the replicas of a windowed statistic ``of`` (``"mean"``, ``"max"``, ``"min"`` or ``"above_share"``) of
        the combinations: every scenario's own window values (``series_combined_summary(by="scenario")``), then per group
        (``by``) and window, over the group's replicas whose window is not empty, what :meth:`series_window_bands` gives --
        numpy float64 [G, W, C] each (:func:`window_bands_by_group`); ``pooled`` is the grouped call's value of the same
        statistic."""
        if of not in ("mean", "max", "min", "above_share"):
            msg = f"of must be 'mean', 'max', 'min' or 'above_share', not {of!r}"
            raise ValueError(msg)
        self._require_samples()
        b = self._series_tick_edges(window_s, ticks_per_window, tick_edges)
        return self._series_combined_bands(combos, b, by, thresholds, of, level, q)[0]

    def _series_combined_bands(self, combos: Any, b: np.ndarray, by: Any, thresholds: Any, of: str, level: float,
                               q: tuple[float, float], **hist: Any) -> tuple[dict[str, Any], dict[str, Any]]:
        """:meth:`series_combined_bands` for resolved tick edges; also returns the grouped summary its ``pooled`` is from."""
        ids, n_groups = self._window_groups(by)
        per = self.series_combined_summary(combos, tick_edges=b, by="scenario", thresholds=thresholds)
        out = window_bands_by_group(per[of], ids, n_groups, level, q, valid=per["count"] > 0)
        pooled = self.series_combined_summary(combos, tick_edges=b, by=ids, thresholds=thresholds, **hist)
        out["pooled"] = pooled[of].cpu().numpy()[:n_groups]
        out.update(of=of, names=per["names"], ops=per["ops"], columns=per["columns"], tick_edges=b, times=per["times"])
        return out, pooled

    def save_series_combined_summary(self, path: str, by: Any = None, *, combos: Any, window_s: float | None = None,
                                     ticks_per_window: int | None = None, tick_edges: Any = None, thresholds: Any = None,
                                     bins: int = 0, lo: Any = None, width: Any = None, level: float = 0.95) -> dict[str, np.ndarray]:
        """Columnar dump of the combinations' statistics with one row per group (grid point): ``param:<axis>`` (for a
        Sweep), ``replicas``, ``series_combined_count`` [G, W] and per combination the [G, W] columns
        ``series_combined_mean:<label>``, ``series_combined_min:<label>``, ``series_combined_max:<label>``,
        ``series_combined_above:<label>`` (the share above the threshold) -- the group's replicas taken together -- and
        ``series_combined_q05:<label>`` / ``series_combined_q95:<label>`` (of the replicas' own means,
        :meth:`series_combined_bands`); with ``bins`` also ``series_combined_hist:<label>`` [G, W, bins],
        ``series_combined_under:<label>``, ``series_combined_over:<label>`` [G, W] and the per-file vector
        ``series_combined_bin_edges:<label>`` [bins + 1].  ``series_combined_tick_edges`` [W + 1] and
        ``series_combined_times`` [W] are per-file vectors.  ``.npz`` or ``.parquet``; :func:`load_summary` reads it back."""
        self._require_samples()
        b = self._series_tick_edges(window_s, ticks_per_window, tick_edges)
        hist_kw = {"bins": bins, "lo": lo, "width": width} if bins or lo is not None or width is not None else {}
        bands, pooled = self._series_combined_bands(combos, b, by, thresholds, "mean", level, (0.05, 0.95), **hist_kw)
        n_groups = int(bands["replicas"].shape[0])
        cols: dict[str, np.ndarray] = {}
        if hasattr(by, "point_columns"):
            for k, v in by.point_columns().items():
                cols[f"param:{k}"] = np.asarray(v, dtype=np.float64)
        cols["replicas"] = np.asarray(bands["replicas"], dtype=np.int64)
        cols["series_combined_count"] = np.ascontiguousarray(pooled["count"].cpu().numpy()[:n_groups], dtype=np.int64)
        stat = {k: pooled[k].cpu().numpy()[:n_groups] for k in ("mean", "min", "max", "above_share")}
        tables = {k: pooled[k].cpu().numpy()[:n_groups] for k in ("hist", "under", "over")} if "hist" in pooled else {}
        for c, name in enumerate(bands["names"]):
            cols[f"series_combined_mean:{name}"] = np.ascontiguousarray(stat["mean"][:, :, c])
            cols[f"series_combined_min:{name}"] = np.ascontiguousarray(stat["min"][:, :, c])
            cols[f"series_combined_max:{name}"] = np.ascontiguousarray(stat["max"][:, :, c])
            cols[f"series_combined_above:{name}"] = np.ascontiguousarray(stat["above_share"][:, :, c])
            cols[f"series_combined_q05:{name}"] = np.ascontiguousarray(bands["q_lo"][:, :, c])
            cols[f"series_combined_q95:{name}"] = np.ascontiguousarray(bands["q_hi"][:, :, c])
            if tables:
                cols[f"series_combined_hist:{name}"] = np.ascontiguousarray(tables["hist"][:, :, c], dtype=np.int64)
                cols[f"series_combined_under:{name}"] = np.ascontiguousarray(tables["under"][:, :, c], dtype=np.int64)
                cols[f"series_combined_over:{name}"] = np.ascontiguousarray(tables["over"][:, :, c], dtype=np.int64)
                cols[f"series_combined_bin_edges:{name}"] = np.ascontiguousarray(pooled["bin_edges"][c], dtype=np.float64)
        cols["series_combined_tick_edges"] = np.asarray(b, dtype=np.float64)
        cols["series_combined_times"] = np.asarray(bands["times"], dtype=np.float64)
        _write_columns(str(path), cols, n_groups)
        return cols

    def _series_joint_call(self, ca: np.ndarray, cb: np.ndarray, lag: np.ndarray, b: np.ndarray, ids: np.ndarray,
                           n_groups: int) -> tuple[dict[str, np.ndarray], float, int]:
        """One call of ``af_engine_summarize_series_joint``: the sums as numpy arrays [G, W, P] (``n`` int64, the others
        Python integers), the call's wall time in ms and the engine's scratch size."""
        import torch

        from .engine import Engine

        samples = self._samples_t
        dev = samples.device
        n_win, n_p = int(b.shape[0] - 1), int(ca.shape[0])
        cnt = torch.empty((n_groups, n_win, n_p), dtype=torch.int32, device=dev)
        one = {k: torch.empty((n_groups, n_win, n_p), dtype=torch.int64, device=dev) for k in ("sx", "sy")}
        two = {k: torch.empty((n_groups, n_win, n_p, 2), dtype=torch.int64, device=dev) for k in ("sxx", "syy", "sxy")}
        grp = torch.from_numpy(np.where(ids < 0, _abi.POOL_SKIP, ids).astype(np.uint32).view(np.int32)).to(dev)
        torch.cuda.synchronize(dev)
        if self._summ_engine is None:
            self._summ_engine = Engine(self.plan, dev.index if dev.index is not None else torch.cuda.current_device())
        ms, scratch = self._summ_engine.summarize_series_joint(
            len(self), n_groups, b, ca, cb, lag, samples_ptr=samples.data_ptr(), tick_capacity=int(samples.shape[1]),
            counts_ptr=self._counts_t.data_ptr(), n_ptr=cnt.data_ptr(), sx_ptr=one["sx"].data_ptr(), sy_ptr=one["sy"].data_ptr(),
            sxx_ptr=two["sxx"].data_ptr(), syy_ptr=two["syy"].data_ptr(), sxy_ptr=two["sxy"].data_ptr(), group_ptr=grp.data_ptr())
        out: dict[str, np.ndarray] = {"n": cnt.cpu().numpy().view(np.uint32).astype(np.int64)}
        for k, t in one.items():
            out[k] = t.cpu().numpy().view(np.uint64).astype(object)
        for k, t in two.items():
            w = t.cpu().numpy().view(np.uint64).astype(object)
            out[k] = w[..., 0] + w[..., 1] * (1 << 64)
        return out, ms, scratch

    def series_joint_summary(self, pairs: Any, window_s: float | None = None, *, ticks_per_window: int | None = None,
                             tick_edges: Any = None, by: Any = None) -> dict[str, Any]:
        """How two sampled series move together per (group, window of ticks), over all scenarios of the group: do the
        servers' queues rise together or in turn, does an edge's concurrency lead a server's queue and by how many ticks.
        ``pairs`` is ``{label: (a, b)}`` or ``{label: (a, b, lag)}``, ``a`` and ``b`` names of :meth:`series_names` or indices
        of INTEGER series (no ``ram_in_use`` column), at most 64 (:func:`check_series_pairs`); the samples of a pair are
        ``(a at tick k, b at tick k + lag)`` with both ticks in the same window of the same scenario.  The HIP analyzer
        ``af_engine_summarize_series_joint`` returns six exact integer sums per cell in one pass over the sample rows --
        equal to :func:`series_joint_sums` added over the group's scenarios --, and :func:`series_joint_statistics` turns
        them into floats on the host.  Windows and ``by`` as in :meth:`series_window_summary`.  Returns numpy arrays
        [G, W, P]: ``n`` int64, the sums ``sx``, ``sy``, ``sxx``, ``syy``, ``sxy`` as Python integers (they pass 64 bits),
        ``mean_x``, ``mean_y``, ``cov``, ``corr``, ``var_x``, ``var_y`` float64 (NaN in empty cells; ``corr`` NaN too where
        a column is constant); and ``labels``, ``a``, ``b``, ``lag``, ``tick_edges``, ``times``, ``replicas`` [G],
        ``series_joint_ms``, ``scratch_bytes``."""
        self._require_samples()
        labels, ca, cb, lag = check_series_pairs(pairs, self.series_names(), self.plan.n_edges)
        b = self._series_tick_edges(window_s, ticks_per_window, tick_edges)
        ids, n_groups = self._window_groups(by)
        out: dict[str, Any]
        out, ms, scratch = self._series_joint_call(ca, cb, lag, b, ids, n_groups)
        out.update(series_joint_statistics(out))
        out.update(labels=labels, a=ca, b=cb, lag=lag, tick_edges=b, times=b[:-1].astype(np.float64) * self.plan.sample_period,
                   replicas=np.bincount(ids[ids >= 0], minlength=n_groups), series_joint_ms=ms, scratch_bytes=scratch)
        return out

    def series_autocorrelation_summary(self, series: Any, max_lag: int, window_s: float | None = None, *,
                                       ticks_per_window: int | None = None, tick_edges: Any = None, by: Any = None) -> dict[str, Any]:
        """The autocorrelation function of sampled series per (group, window of ticks) and what a time average over the
        window is worth: ``series`` are names of :meth:`series_names`, indices, one ``fnmatch`` pattern or a list of those
        (integer series only); the lags are ``0 .. max_lag`` ticks, issued to ``af_engine_summarize_series_joint`` as calls
        of at most 64 pairs ``(c, c, l)``.  ``acf`` float64 [G, W, C, max_lag + 1]: ``acf[l]`` is the PEARSON correlation of
        ``(x_k, x_{k + l})`` over the overlapping ticks of each window, each side with its own mean and variance over the
        ticks it covers; it is NOT the estimator that divides the lagged products about the full-sample mean by the
        full-sample variance -- the two differ by O(l / n) in a window of n ticks.  ``n`` int64 [G, W, C, max_lag + 1] are
        the pairs per lag.  ``tau`` [G, W, C] is the integrated autocorrelation time ``1 + 2 * sum(acf[1 .. m])``, ``m`` the
        last lag before the first ``acf[l] <= 0`` or NaN; ``tau_truncated`` is true where no such lag was found up to
        ``max_lag`` (the lags were too few; ``tau`` is then a lower bound); ``ess = n[..., 0] / tau`` is the number of
        independent samples the window's mean is worth (:func:`autocorrelation_time`).  Also ``series`` (the names),
        ``columns``, ``lags``, ``tick_edges``, ``times``, ``replicas``, ``series_joint_ms`` (all calls), ``calls``."""
        self._require_samples()
        if isinstance(max_lag, (bool, np.bool_)) or not isinstance(max_lag, (int, np.integer)) or not 0 <= int(max_lag) < 2 ** 31:
            msg = f"max_lag must be a whole number of ticks in [0, 2^31), not {max_lag!r}"
            raise ValueError(msg)
        names = self.series_names()
        cols = _select_series(series, names, "series")
        ram = ram_columns(len(names), self.plan.n_edges)
        for j in cols:
            if ram[j]:
                msg = f"{names[j]!r} is a ram_in_use column; the autocorrelation takes integer series only"
                raise ValueError(msg)
        b = self._series_tick_edges(window_s, ticks_per_window, tick_edges)
        ids, n_groups = self._window_groups(by)
        n_lag, n_win = int(max_lag) + 1, int(b.shape[0] - 1)
        every = [(c, lag) for c in cols for lag in range(n_lag)]
        acf = np.empty((n_groups, n_win, len(every)))
        cnt = np.empty((n_groups, n_win, len(every)), dtype=np.int64)
        total_ms, scratch, calls = 0.0, 0, 0
        for at in range(0, len(every), _abi.MAX_SERIES_PAIRS):
            part = every[at:at + _abi.MAX_SERIES_PAIRS]
            col = np.array([c for c, _ in part], dtype=np.int64)
            sums, ms, scratch = self._series_joint_call(col, col, np.array([lag for _, lag in part], dtype=np.int64), b, ids, n_groups)
            acf[:, :, at:at + len(part)] = series_joint_statistics(sums)["corr"]
            cnt[:, :, at:at + len(part)] = sums["n"]
            total_ms += ms
            calls += 1
        acf = acf.reshape(n_groups, n_win, len(cols), n_lag)
        cnt = cnt.reshape(n_groups, n_win, len(cols), n_lag)
        out: dict[str, Any] = {"acf": acf, "n": cnt}
        out.update(autocorrelation_time(acf, cnt[..., 0]))
        out.update(series=[names[j] for j in cols], columns=np.array(cols, dtype=np.int64), lags=np.arange(n_lag), tick_edges=b,
                   times=b[:-1].astype(np.float64) * self.plan.sample_period, replicas=np.bincount(ids[ids >= 0], minlength=n_groups),
                   series_joint_ms=total_ms, scratch_bytes=scratch, calls=calls)
        return out

    def series_joint_bands(self, pairs: Any, window_s: float | None = None, *, ticks_per_window: int | None = None,
                           tick_edges: Any = None, by: Any = None, of: str = "corr", level: float = 0.95,
                           q: tuple[float, float] = (0.05, 0.95)) -> dict[str, Any]:
        """Bands over the replicas of ``of`` (``"corr"`` or ``"cov"``) of the pairs: every scenario's own window values
        (``series_joint_summary(by="scenario")``), then per group (``by``), window and pair, over the group's replicas whose
        value is not NaN, what :meth:`series_window_bands` gives -- numpy float64 [G, W, P] each
        (:func:`window_bands_by_group`, pair by pair: a pair's value may be NaN where another's is not); ``n`` int64
        [G, W, P] are the replicas that count; ``pooled`` is the grouped call's value of the same statistic."""
        if of not in ("corr", "cov"):
            msg = f"of must be 'corr' or 'cov', not {of!r}"
            raise ValueError(msg)
        self._require_samples()
        b = self._series_tick_edges(window_s, ticks_per_window, tick_edges)
        return self._series_joint_bands(pairs, b, by, of, level, q)[0]

    def _series_joint_bands(self, pairs: Any, b: np.ndarray, by: Any, of: str, level: float,
                            q: tuple[float, float]) -> tuple[dict[str, Any], dict[str, Any]]:
        """:meth:`series_joint_bands` for resolved tick edges; also returns the grouped summary its ``pooled`` is from."""
        import torch

        ids, n_groups = self._window_groups(by)
        per = self.series_joint_summary(pairs, tick_edges=b, by="scenario")
        values = torch.from_numpy(np.ascontiguousarray(per[of]))       # (the statistics are made on the host)
        parts = [window_bands_by_group(values[:, :, p:p + 1], ids, n_groups, level, q, valid=~torch.isnan(values[:, :, p]))
                 for p in range(values.shape[2])]
        out: dict[str, Any] = {k: np.concatenate([x[k] for x in parts], axis=2) for k in ("mean", "std", "ci_halfwidth", "q_lo", "q_hi")}
        out["n"] = np.stack([x["n"] for x in parts], axis=2)
        out.update(replicas=parts[0]["replicas"], level=level, q=parts[0]["q"])
        pooled = self.series_joint_summary(pairs, tick_edges=b, by=ids)
        out["pooled"] = pooled[of][:n_groups]
        out.update(of=of, labels=per["labels"], a=per["a"], b=per["b"], lag=per["lag"], tick_edges=b, times=per["times"])
        return out, pooled

    def save_series_joint_summary(self, path: str, by: Any = None, *, pairs: Any, window_s: float | None = None,
                                  ticks_per_window: int | None = None, tick_edges: Any = None, level: float = 0.95) -> dict[str, np.ndarray]:
        """Columnar dump of the pairs' statistics with one row per group (grid point): ``param:<axis>`` (for a Sweep),
        ``replicas`` and per pair the [G, W] columns ``series_joint_corr:<label>``, ``series_joint_cov:<label>``,
        ``series_joint_n:<label>`` -- the group's replicas taken together -- and ``series_joint_q05:<label>`` /
        ``series_joint_q95:<label>`` (of the replicas' own correlations, :meth:`series_joint_bands`).
        ``series_joint_tick_edges`` [W + 1] and ``series_joint_times`` [W] are per-file vectors.  ``.npz`` or ``.parquet``;
        :func:`load_summary` reads it back."""
        self._require_samples()
        b = self._series_tick_edges(window_s, ticks_per_window, tick_edges)
        bands, pooled = self._series_joint_bands(pairs, b, by, "corr", level, (0.05, 0.95))
        n_groups = int(bands["replicas"].shape[0])
        cols: dict[str, np.ndarray] = {}
        if hasattr(by, "point_columns"):
            for k, v in by.point_columns().items():
                cols[f"param:{k}"] = np.asarray(v, dtype=np.float64)
        cols["replicas"] = np.asarray(bands["replicas"], dtype=np.int64)
        for p, name in enumerate(bands["labels"]):
            cols[f"series_joint_corr:{name}"] = np.ascontiguousarray(pooled["corr"][:n_groups, :, p])
            cols[f"series_joint_cov:{name}"] = np.ascontiguousarray(pooled["cov"][:n_groups, :, p])
            cols[f"series_joint_n:{name}"] = np.ascontiguousarray(pooled["n"][:n_groups, :, p], dtype=np.int64)
            cols[f"series_joint_q05:{name}"] = np.ascontiguousarray(bands["q_lo"][:, :, p])
            cols[f"series_joint_q95:{name}"] = np.ascontiguousarray(bands["q_hi"][:, :, p])
        cols["series_joint_tick_edges"] = np.asarray(b, dtype=np.float64)
        cols["series_joint_times"] = np.asarray(bands["times"], dtype=np.float64)
        _write_columns(str(path), cols, n_groups)
        return cols

    def _series_warmup_call(self, cols: np.ndarray, batch: int, b: np.ndarray, ids: np.ndarray,
                            n_groups: int) -> tuple[dict[str, np.ndarray], float, int]:
        """One call of ``af_engine_summarize_series_warmup`` (at most 64 columns): ``batches`` int64 [G, W], ``trunc`` int64
        [G, W, C] and the four sums as Python integers [G, W, C], the call's wall time in ms and the engine's scratch size."""
        import torch

        from .engine import Engine

        samples = self._samples_t
        dev = samples.device
        n_win, n_c = int(b.shape[0] - 1), int(cols.shape[0])
        nb = torch.empty((n_groups, n_win), dtype=torch.int32, device=dev)
        trunc = torch.empty((n_groups, n_win, n_c), dtype=torch.int32, device=dev)
        wide = {k: torch.empty((n_groups, n_win, n_c, 2 if k.startswith("s1") else 3), dtype=torch.int64, device=dev) for k in WARMUP_SUMS}
        grp = torch.from_numpy(np.where(ids < 0, _abi.POOL_SKIP, ids).astype(np.uint32).view(np.int32)).to(dev)
        torch.cuda.synchronize(dev)
        if self._summ_engine is None:
            self._summ_engine = Engine(self.plan, dev.index if dev.index is not None else torch.cuda.current_device())
        ms, scratch = self._summ_engine.summarize_series_warmup(
            len(self), n_groups, b, cols, batch, samples_ptr=samples.data_ptr(), tick_capacity=int(samples.shape[1]),
            counts_ptr=self._counts_t.data_ptr(), batches_ptr=nb.data_ptr(), trunc_ptr=trunc.data_ptr(), group_ptr=grp.data_ptr(),
            **{f"{k}_ptr": t.data_ptr() for k, t in wide.items()})
        out: dict[str, np.ndarray] = {"batches": nb.cpu().numpy().view(np.uint32).astype(np.int64),
                                      "trunc": trunc.cpu().numpy().view(np.uint32).astype(np.int64)}
        for k, t in wide.items():
            w = t.cpu().numpy().view(np.uint64).astype(object)
            out[k] = sum(w[..., i] * (1 << (64 * i)) for i in range(w.shape[-1]))
        return out, ms, scratch

    def series_warmup_summary(self, batch: int = 5, window_s: float | None = None, *, ticks_per_window: int | None = None,
                              tick_edges: Any = None, by: Any = None, series: Any = None) -> dict[str, Any]:
        """Where the sampled series leave their initial transient, per (group, window of ticks, series): every sweep starts
        from an empty system, and replicas shrink the band around a mean that still averages the ramp-up in.  The MSER rule
        (White 1997; ``batch = 5`` is MSER-5) in pooled form: the batch sums ``Y_j`` of ``batch`` ticks are added over the
        group's replicas, and the truncation point ``d*`` is the smallest ``d <= J / 2`` that minimises the variance of the
        remaining batch means over their number.  The HIP analyzer ``af_engine_summarize_series_warmup`` computes it in
        exact integers, equal word for word to :func:`series_warmup_sums` of the group's members;
        :func:`series_warmup_statistics` makes the floats on the host.  One short member shortens a cell for all
        (``batches``); leave a broken replica out with group id -1.  ``series``: None (every integer series), names of
        :meth:`series_names` or indices, any order, duplicates allowed, no ``ram_in_use`` column; more than 64 are split
        into several calls.  Windows and ``by`` as in :meth:`series_window_summary`; no window given: one window over the
        whole run; a window that starts at an injected event answers how long the system takes to reach its new regime.
        Returns numpy arrays: ``batches`` int64 [G, W]; ``trunc``, ``warmup_tick`` int64, ``warmup_s``, ``mean_all``,
        ``mean_steady``, ``mser_all``, ``mser_steady`` float64 and ``converged`` bool [G, W, C]; the sums ``s1``, ``s2``,
        ``s1_all``, ``s2_all`` as Python integers [G, W, C]; ``cut`` [G, W] (:func:`series_warmup_cut`: the ``t0`` for
        ``edges=[t0, T]``); and ``series`` (the names), ``columns``, ``batch``, ``tick_edges``, ``times``, ``replicas`` [G],
        ``series_warmup_ms`` (all calls), ``scratch_bytes``, ``calls``."""
        self._require_samples()
        n_b = check_warmup_batch(batch)
        names = self.series_names()
        cols = _warmup_columns(series, names, self.plan.n_edges)
        if window_s is None and ticks_per_window is None and tick_edges is None:
            tick_edges = [0, max(self.plan.tick_count, 1)]
        b = self._series_tick_edges(window_s, ticks_per_window, tick_edges)
        ids, n_groups = self._window_groups(by)
        parts, total_ms, scratch = [], 0.0, 0
        for at in range(0, len(cols), _abi.MAX_SERIES_WARMUP_COLUMNS):
            part, ms, scratch = self._series_warmup_call(cols[at:at + _abi.MAX_SERIES_WARMUP_COLUMNS], n_b, b, ids, n_groups)
            parts.append(part)
            total_ms += ms
        out: dict[str, Any] = {"batches": parts[0]["batches"]}
        for k in ("trunc", *WARMUP_SUMS):
            out[k] = np.concatenate([p[k] for p in parts], axis=2)
        replicas = np.bincount(ids[ids >= 0], minlength=n_groups)
        out.update(series_warmup_statistics(out, n_b, replicas, self.plan.sample_period, b))
        out.update(cut=series_warmup_cut(out), series=[names[j] for j in cols], columns=cols, batch=n_b, tick_edges=b,
                   times=b[:-1].astype(np.float64) * self.plan.sample_period, replicas=replicas, series_warmup_ms=total_ms,
                   scratch_bytes=scratch, calls=len(parts))
        return out

    def series_warmup_bands(self, batch: int = 5, window_s: float | None = None, *, ticks_per_window: int | None = None,
                            tick_edges: Any = None, by: Any = None, series: Any = None, level: float = 0.95,
                            q: tuple[float, float] = (0.05, 0.95)) -> dict[str, Any]:
        """How much the warm-up time varies from replica to replica: every scenario's own ``warmup_s``
        (``series_warmup_summary(by="scenario")``), then per group (``by``), window and series, over the group's replicas
        that hold a batch in the window, what :meth:`series_window_bands` gives -- numpy float64 [G, W, C] each
        (:func:`window_bands_by_group`); ``n`` int64 [G, W] are the replicas that count; ``converged_share`` [G, W, C] is
        the share of those whose own truncation point lies below the search limit (NaN without one); ``pooled`` is the
        grouped call's ``warmup_s`` and ``pooled_converged`` its ``converged``."""
        self._require_samples()
        if window_s is None and ticks_per_window is None and tick_edges is None:
            tick_edges = [0, max(self.plan.tick_count, 1)]
        b = self._series_tick_edges(window_s, ticks_per_window, tick_edges)
        return self._series_warmup_bands(batch, b, by, series, level, q)[0]

    def _series_warmup_bands(self, batch: int, b: np.ndarray, by: Any, series: Any, level: float,
                             q: tuple[float, float]) -> tuple[dict[str, Any], dict[str, Any]]:
        """:meth:`series_warmup_bands` for resolved tick edges; also returns the grouped summary its ``pooled`` is from."""
        import torch

        ids, n_groups = self._window_groups(by)
        per = self.series_warmup_summary(batch, tick_edges=b, by="scenario", series=series)
        valid = per["batches"] > 0
        out = window_bands_by_group(torch.from_numpy(np.ascontiguousarray(per["warmup_s"])), ids, n_groups, level, q,
                                    valid=torch.from_numpy(valid))
        share = np.full((n_groups, *per["converged"].shape[1:]), np.nan)
        for g in range(n_groups):
            mem = ids == g
            cnt = valid[mem].sum(axis=0)                                                   # [W]
            hit = (per["converged"][mem] & valid[mem][:, :, None]).sum(axis=0)             # [W, C]
            share[g] = np.where(cnt[:, None] > 0, hit / np.maximum(cnt, 1)[:, None], np.nan)
        out["converged_share"] = share
        pooled = self.series_warmup_summary(batch, tick_edges=b, by=ids, series=series)
        out["pooled"] = pooled["warmup_s"][:n_groups]
        out["pooled_converged"] = pooled["converged"][:n_groups]
        out.update(series=per["series"], columns=per["columns"], batch=per["batch"], tick_edges=b, times=per["times"])
        return out, pooled

    def save_series_warmup_summary(self, path: str, by: Any = None, *, batch: int = 5, window_s: float | None = None,
                                   ticks_per_window: int | None = None, tick_edges: Any = None, series: Any = None,
                                   level: float = 0.95) -> dict[str, np.ndarray]:
        """Columnar dump of the warm-up truncation with one row per group (grid point): ``param:<axis>`` (for a Sweep),
        ``replicas``, ``series_warmup_batches`` and ``series_warmup_cut`` [G, W] and per series the [G, W] columns
        ``series_warmup_tick:<name>``, ``series_warmup_s:<name>``, ``series_warmup_converged:<name>`` (0 / 1),
        ``series_warmup_mean_all:<name>``, ``series_warmup_mean_steady:<name>`` -- the group's replicas taken together --
        and ``series_warmup_q05:<name>`` / ``series_warmup_q95:<name>`` / ``series_warmup_converged_share:<name>`` (of the
        replicas' own warm-up times, :meth:`series_warmup_bands`).  ``series_warmup_tick_edges`` [W + 1],
        ``series_warmup_times`` [W] and ``series_warmup_batch`` [1] are per-file vectors.  ``.npz`` or ``.parquet``;
        :func:`load_summary` reads it back."""
        self._require_samples()
        if window_s is None and ticks_per_window is None and tick_edges is None:
            tick_edges = [0, max(self.plan.tick_count, 1)]
        b = self._series_tick_edges(window_s, ticks_per_window, tick_edges)
        bands, pooled = self._series_warmup_bands(batch, b, by, series, level, (0.05, 0.95))
        n_groups = int(bands["replicas"].shape[0])
        cols: dict[str, np.ndarray] = {}
        if hasattr(by, "point_columns"):
            for k, v in by.point_columns().items():
                cols[f"param:{k}"] = np.asarray(v, dtype=np.float64)
        cols["replicas"] = np.asarray(bands["replicas"], dtype=np.int64)
        cols["series_warmup_batches"] = np.ascontiguousarray(pooled["batches"][:n_groups], dtype=np.int64)
        cols["series_warmup_cut"] = np.ascontiguousarray(pooled["cut"][:n_groups], dtype=np.float64)
        for c, name in enumerate(bands["series"]):
            cols[f"series_warmup_tick:{name}"] = np.ascontiguousarray(pooled["warmup_tick"][:n_groups, :, c], dtype=np.int64)
            cols[f"series_warmup_s:{name}"] = np.ascontiguousarray(pooled["warmup_s"][:n_groups, :, c])
            cols[f"series_warmup_converged:{name}"] = np.ascontiguousarray(pooled["converged"][:n_groups, :, c], dtype=np.int64)
            cols[f"series_warmup_mean_all:{name}"] = np.ascontiguousarray(pooled["mean_all"][:n_groups, :, c])
            cols[f"series_warmup_mean_steady:{name}"] = np.ascontiguousarray(pooled["mean_steady"][:n_groups, :, c])
            cols[f"series_warmup_q05:{name}"] = np.ascontiguousarray(bands["q_lo"][:, :, c])
            cols[f"series_warmup_q95:{name}"] = np.ascontiguousarray(bands["q_hi"][:, :, c])
            cols[f"series_warmup_converged_share:{name}"] = np.ascontiguousarray(bands["converged_share"][:, :, c])
        cols["series_warmup_tick_edges"] = np.asarray(b, dtype=np.float64)
        cols["series_warmup_times"] = np.asarray(bands["times"], dtype=np.float64)
        cols["series_warmup_batch"] = np.asarray([pooled["batch"]], dtype=np.float64)
        _write_columns(str(path), cols, n_groups)
        return cols

    def differing_scenarios(self, other: "BatchedResults", chunk: int = 512) -> np.ndarray:
        """Indices of the scenarios whose results differ from ``other``'s, compared ON THE DEVICE over the whole batch
        (see :func:`differing_scenarios`): two runs of one sweep by different kernel families must return an empty array."""
        return differing_scenarios(self._counts_t, self._clock_t, self._samples_t,
                                   other._counts_t, other._clock_t, other._samples_t, chunk)  # noqa: SLF001


def differing_scenarios(counts_a: Any, clock_a: Any, samples_a: Any, counts_b: Any, clock_b: Any, samples_b: Any,
                        chunk: int = 512) -> np.ndarray:
    """Whole-batch comparison of two result sets of one sweep without leaving HBM (10 000 LB-2 scenarios at T = 600 s
    are 2 x 18 GB): the counts (generated, completed, dropped, request-events, ticks, flags, timeline marks), every
    ``rqs_clock`` row a scenario completed (client.py:62-69) as BIT PATTERNS, and every sample word of every tick the
    scenario reached (collector.py:50-66).  Rows behind a scenario's own counts are uninitialised memory and not looked
    at.  Returns the differing scenario indices (sorted int64 array; empty = bit-identical)."""
    import torch

    n = int(counts_a.shape[0])
    if int(counts_b.shape[0]) != n:
        msg = f"batches of {n} and {int(counts_b.shape[0])} scenarios"
        raise ValueError(msg)
    ca, cb = counts_a.to(torch.int64) & 0xFFFFFFFF, counts_b.to(torch.int64) & 0xFFFFFFFF
    cols = [_abi.CNT_GENERATED, _abi.CNT_COMPLETED, _abi.CNT_DROPPED, _abi.CNT_EVENTS, _abi.CNT_TICKS, _abi.CNT_FLAGS, _abi.CNT_MARKS]
    bad = (ca[:, cols] != cb[:, cols]).any(dim=1)
    if (clock_a is None) != (clock_b is None) or (samples_a is None) != (samples_b is None):
        msg = "one batch kept an output the other did not"
        raise ValueError(msg)
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        if clock_a is not None:
            cap = min(int(clock_a.shape[1]), int(clock_b.shape[1]))
            done = ca[lo:hi, _abi.CNT_COMPLETED].clamp(max=cap)
            live = torch.arange(cap, device=done.device)[None, :] < done[:, None]
            x = clock_a[lo:hi, :cap].view(torch.int64)
            y = clock_b[lo:hi, :cap].view(torch.int64)
            bad[lo:hi] |= ((x != y).any(dim=2) & live).any(dim=1)
        if samples_a is not None:
            cap = min(int(samples_a.shape[1]), int(samples_b.shape[1]))
            pitch = min(int(samples_a.shape[2]), int(samples_b.shape[2]))
            ticks = ca[lo:hi, _abi.CNT_TICKS].clamp(max=cap)
            live = torch.arange(cap, device=ticks.device)[None, :] < ticks[:, None]
            bad[lo:hi] |= ((samples_a[lo:hi, :cap, :pitch] != samples_b[lo:hi, :cap, :pitch]).any(dim=2) & live).any(dim=1)
    return torch.nonzero(bad).reshape(-1).cpu().numpy()


def aggregate_summary(summ: dict[str, Any], level: float = 0.95) -> dict[str, Any]:
    """Monte-Carlo aggregation of a ``summary()`` dict (see :meth:`BatchedResults.aggregate`)."""
    from statistics import NormalDist

    import torch

    st = summ["stats"]                                  # [n, 8] on the run's device: reduced there,
    ok = st[:, 0] > 0                                   # only the 8-vectors and the [T] bands come back
    z = NormalDist().inv_cdf(0.5 + level / 2.0)
    k = int(ok.sum())
    body = st[ok]
    nan8 = np.full(8, np.nan)
    mean = body.mean(dim=0).cpu().numpy() if k else nan8
    sd = body.std(dim=0, unbiased=True).cpu().numpy() if k > 1 else nan8
    out: dict[str, Any] = {
        "n": k,
        "keys": LATENCY_KEYS,
        "mean": dict(zip(LATENCY_KEYS, mean.tolist())),
        "std": dict(zip(LATENCY_KEYS, sd.tolist())),
        "ci_halfwidth": dict(zip(LATENCY_KEYS, (z * sd / np.sqrt(max(k, 1))).tolist())),
        "level": level,
    }
    if "rps" in summ:
        r = summ["rps"].to(torch.float64)
        out["rps_mean"] = r.mean(dim=0).cpu().numpy()
        q = torch.quantile(r, torch.tensor([0.05, 0.95], dtype=torch.float64, device=r.device), dim=0)
        out["rps_p05"], out["rps_p95"] = q[0].cpu().numpy(), q[1].cpu().numpy()
    return out


def resolve_groups(by: Any, n: int) -> tuple[np.ndarray, int]:
    """Group id of every scenario and the number of groups G for ``by``: None (one group), a Sweep (its grid points,
    G = points of the grid) or an integer array [n] (negative = left out, G = largest id + 1).  Returns int64 ids [n]."""
    if by is None:
        return np.zeros(n, dtype=np.int64), 1
    if hasattr(by, "point") and hasattr(by, "shape"):
        ids = np.asarray(by.point)
        n_groups = int(np.prod(by.shape)) if by.shape else 1
    else:
        ids = np.asarray(by)
        n_groups = None
    if ids.ndim != 1 or ids.shape[0] != n:
        msg = f"group ids must be a vector of one id per scenario ({n}), not of shape {ids.shape}"
        raise ValueError(msg)
    if not (np.issubdtype(ids.dtype, np.integer) and ids.dtype != np.bool_):
        msg = f"group ids must be integers, not {ids.dtype}"
        raise TypeError(msg)
    ids = ids.astype(np.int64)
    if n_groups is None:
        n_groups = int(ids.max()) + 1 if n and ids.max() >= 0 else 0
    if n_groups == 0:
        msg = "no scenario is in a group"
        raise ValueError(msg)
    if ids.max(initial=-1) >= n_groups:
        msg = f"group id {int(ids.max())} out of range for {n_groups} groups"
        raise ValueError(msg)
    return ids, n_groups


def _sum_rows_by_cell(index: Any, body: Any, cells: int) -> Any:
    """Per cell the float64 sum of its rows of ``body`` [N, K] (``index`` [N]: the row's cell), on ``body``'s device and the same
    bits in every run: the rows are sorted by cell (stably: a cell's rows stay in row order) and every cell is added up as a
    fixed binary tree -- row 0 + row 1, row 2 + row 3, ... level after level, ceil(log2(largest cell)) elementwise steps, no
    atomics.  The tree depends on the cells' sizes alone, so a sweep on one device and on several give the same words.  (A device
    ``index_add_`` adds floats atomically, in no fixed order: an ulp of difference from run to run.)  An empty cell: 0."""
    import torch

    dev = body.device
    cells = int(cells)
    idx, order = torch.sort(index.to(torch.int64), stable=True)
    v = body.to(torch.float64)[order]
    c = torch.bincount(idx, minlength=cells)                     # rows per cell, at this level of the tree
    out = torch.zeros((cells, int(body.shape[1])), dtype=torch.float64, device=dev)
    if v.shape[0] == 0:
        return out
    cell_ids = torch.arange(cells, device=dev)
    for _ in range((int(c.max()) - 1).bit_length()):
        cell = torch.repeat_interleave(cell_ids, c)
        rank = torch.arange(v.shape[0], device=dev) - (torch.cumsum(c, 0) - c)[cell]
        first = rank % 2 == 0
        paired = first & (rank + 1 < c[cell])                    # the row has a right neighbour in its cell
        v = torch.where(paired[:, None], v + torch.roll(v, -1, 0), v)[first]
        c = (c + 1) // 2
    out[c > 0] = v + 0.0                                         # (one row per non-empty cell, in cell order; -0.0 + 0.0 = 0.0 as a sum from 0 gives)
    return out


def aggregate_by_group(summ: dict[str, Any], ids: np.ndarray, n_groups: int, level: float = 0.95) -> dict[str, Any]:
    """:func:`aggregate_summary` per group (``ids`` from :func:`resolve_groups`): for every group the mean, unbiased
    standard deviation and normal confidence half-width of each per-replica statistic over its scenarios with >= 1
    completion (``n`` [G] of them), and per 1-s window the mean and the 5th / 95th linear quantiles of the RPS over
    the group's scenarios.  Reduced on the device, no loop over groups; the float sums as fixed trees (:func:`_sum_rows_by_cell`): the
    same bits in every run.  Returned as numpy arrays [G, 8] / [G, T]."""
    from statistics import NormalDist

    import torch

    st = summ["stats"]
    dev = st.device
    gid = torch.as_tensor(ids, device=dev)
    member = gid >= 0
    ok = member & (st[:, 0] > 0)
    z = NormalDist().inv_cdf(0.5 + level / 2.0)
    g_ok, body = gid[ok], st[ok]
    k = torch.bincount(g_ok, minlength=n_groups).to(torch.float64)
    total = _sum_rows_by_cell(g_ok, body, n_groups)
    mean = total / k[:, None]
    dev2 = _sum_rows_by_cell(g_ok, (body - mean[g_ok]) ** 2, n_groups)
    sd = torch.where((k > 1)[:, None], (dev2 / (k - 1.0).clamp(min=1.0)[:, None]).sqrt(), torch.full_like(dev2, float("nan")))
    mean = torch.where((k > 0)[:, None], mean, torch.full_like(mean, float("nan")))
    out: dict[str, Any] = {
        "n": k.to(torch.int64).cpu().numpy(),
        "replicas": np.bincount(ids[ids >= 0], minlength=n_groups),
        "keys": LATENCY_KEYS,
        "mean": mean.cpu().numpy(),
        "std": sd.cpu().numpy(),
        "ci_halfwidth": (z * sd / k.clamp(min=1.0).sqrt()[:, None]).cpu().numpy(),
        "level": level,
    }
    if "rps" in summ:
        r = summ["rps"].to(torch.float64)[member]
        g = gid[member]
        T = int(r.shape[1])
        c = torch.bincount(g, minlength=n_groups)
        out["rps_mean"] = (_sum_rows_by_cell(g, r, n_groups) / c.to(torch.float64)[:, None]).cpu().numpy()
        # every window sorted by value, then (stably) by group: each group's values ascending in one segment
        v, order = torch.sort(r, dim=0, stable=True)
        gs = g[order]
        gs, order2 = torch.sort(gs, dim=0, stable=True)
        v = torch.gather(v, 0, order2)
        start = torch.cumsum(c, 0) - c
        for name, q in (("rps_p05", 0.05), ("rps_p95", 0.95)):
            pos = (c - 1).clamp(min=0).to(torch.float64) * q
            lo = pos.floor().to(torch.int64)
            hi = torch.minimum(lo + 1, (c - 1).clamp(min=0))
            t = (pos - lo.to(torch.float64))[:, None]
            if v.shape[0] == 0:
                band = torch.full((n_groups, T), float("nan"), dtype=torch.float64, device=dev)
            else:
                a = v[(start + lo).clamp(max=v.shape[0] - 1)]
                b = v[(start + hi).clamp(max=v.shape[0] - 1)]
                d = b - a
                band = torch.where(t >= 0.5, b - d * (1.0 - t), a + d * t)   # (numpy's _lerp)
                band = torch.where((c > 0)[:, None], band, torch.full_like(band, float("nan")))
            out[name] = band.cpu().numpy()
    return out


def window_bands_by_group(per: Any, ids: np.ndarray, n_groups: int, level: float = 0.95,
                          q: tuple[float, float] = (0.05, 0.95), valid: Any = None) -> dict[str, Any]:
    """Bands of per-scenario window statistics ``per`` (torch float64 [n, W, K]) over the scenarios of every group
    (``ids`` from :func:`resolve_groups`), per window, over the scenarios whose window is ``valid`` (torch bool [n, W];
    None: the latency statistics' rule, ``per[:, :, 0] > 0``, the windows that hold a completion): see
    :meth:`BatchedResults.window_bands` (K = 8) and :meth:`BatchedResults.series_window_bands` (K = the sampled series).
    Reduced on ``per``'s device without a loop over groups or windows, the float sums as fixed trees (:func:`_sum_rows_by_cell`):
    the same bits in every run."""
    from statistics import NormalDist

    import torch

    dev = per.device
    n_win, n_col = int(per.shape[1]), int(per.shape[2])
    cells = n_groups * n_win
    gid = torch.as_tensor(ids, device=dev)
    key = gid[:, None] * n_win + torch.arange(n_win, device=dev)[None, :]            # cell of (scenario, window)
    ok = (gid >= 0)[:, None] & (per[:, :, 0] > 0 if valid is None else valid)
    k_ok, body = key[ok], per[ok]                                                    # [N], [N, K]
    z = NormalDist().inv_cdf(0.5 + level / 2.0)
    c = torch.bincount(k_ok, minlength=cells)
    k = c.to(torch.float64)
    nan = torch.full((cells, n_col), float("nan"), dtype=torch.float64, device=dev)
    total = _sum_rows_by_cell(k_ok, body, cells)
    mean = total / k[:, None]
    dev2 = _sum_rows_by_cell(k_ok, (body - mean[k_ok]) ** 2, cells)
    sd = torch.where((k > 1)[:, None], (dev2 / (k - 1.0).clamp(min=1.0)[:, None]).sqrt(), nan)
    mean = torch.where((k > 0)[:, None], mean, nan)
    shape = (n_groups, n_win, n_col)
    out: dict[str, Any] = {
        "n": c.reshape(n_groups, n_win).cpu().numpy(),
        "replicas": np.bincount(ids[ids >= 0], minlength=n_groups),
        "mean": mean.reshape(shape).cpu().numpy(),
        "std": sd.reshape(shape).cpu().numpy(),
        "ci_halfwidth": (z * sd / k.clamp(min=1.0).sqrt()[:, None]).reshape(shape).cpu().numpy(),
        "level": level,
        "q": (float(q[0]), float(q[1])),
    }
    if valid is None:
        out["keys"] = LATENCY_KEYS
    # every statistic sorted by value, then (stably) by cell: each cell's values ascending in one segment
    v, order = torch.sort(body, dim=0, stable=True)
    ks, order2 = torch.sort(k_ok[order], dim=0, stable=True)
    v = torch.gather(v, 0, order2)
    start = torch.cumsum(c, 0) - c
    for name, qq in (("q_lo", float(q[0])), ("q_hi", float(q[1]))):
        if v.shape[0] == 0:
            out[name] = nan.reshape(shape).cpu().numpy()
            continue
        pos = (c - 1).clamp(min=0).to(torch.float64) * qq
        lo = pos.floor().to(torch.int64)
        hi = torch.minimum(lo + 1, (c - 1).clamp(min=0))
        t = (pos - lo.to(torch.float64))[:, None]
        a = v[(start + lo).clamp(max=v.shape[0] - 1)]
        b = v[(start + hi).clamp(max=v.shape[0] - 1)]
        d = b - a
        band = torch.where(t >= 0.5, b - d * (1.0 - t), a + d * t)   # (numpy's _lerp)
        out[name] = torch.where((c > 0)[:, None], band, nan).reshape(shape).cpu().numpy()
    return out


def _write_columns(path: str, cols: dict[str, np.ndarray], n: int) -> None:
    """``.parquet`` (pyarrow; [n, k] columns become list columns, vectors of another length schema metadata) or ``.npz``."""
    if path.endswith(".parquet"):
        import pyarrow as pa
        import pyarrow.parquet as pq

        table = {k: (pa.array(v.tolist()) if v.ndim > 2 else pa.array(list(v)) if v.ndim == 2 and v.shape[0] == n else pa.array(v))
                 for k, v in cols.items() if v.shape[:1] == (n,)}
        meta = {k: ",".join(map(str, np.atleast_1d(v).tolist())) for k, v in cols.items() if v.shape[:1] != (n,)}
        pq.write_table(pa.table(table).replace_schema_metadata(meta), path)
    else:
        np.savez_compressed(path, **cols)


def _save_latency_histogram(summ: dict[str, Any], path: str, by: Any) -> dict[str, np.ndarray]:
    """The columns of ``save_latency_histogram_summary``, written to ``path``."""
    p = _latency_histogram_parts(summ)
    n_groups = int(p["replicas"].shape[0])
    cols: dict[str, np.ndarray] = {}
    if hasattr(by, "point_columns"):
        for name, v in by.point_columns().items():
            cols[f"param:{name}"] = np.asarray(v, dtype=np.float64)
    cols["replicas"] = p["replicas"]
    for k in _LHIST_COUNTS:
        cols[f"lhist_{k}"] = np.ascontiguousarray(p[k])
    for k in ("sub_bits", "min_exp", "octaves"):
        cols[f"lhist_{k}"] = np.asarray(p[k], dtype=np.int64)
    if p["edges"] is not None:
        cols["window_edges"] = p["edges"]
    cols["window_of"] = np.asarray(p["window_of"])
    _write_columns(path, cols, n_groups)
    return cols


def _finish_quantile_summary(quant: Any, count: Any, within: Any, q: np.ndarray, th: np.ndarray, e: np.ndarray | None, ids: np.ndarray,
                             n_groups: int, ms: float, scratch: int, window_of: str) -> dict[str, Any]:
    """What ``quantile_summary`` returns, from the device's words: the counts as int64 and the shares."""
    import torch

    cnt = count.to(torch.int64) & 0xFFFFFFFF   # (the device's words are uint32)
    wth = within.to(torch.int64) & 0xFFFFFFFF
    nan = torch.full((), float("nan"), dtype=torch.float64, device=quant.device)
    share = torch.where((cnt > 0)[:, :, None], wth.to(torch.float64) / cnt.clamp(min=1).to(torch.float64)[:, :, None], nan)
    return {"quantiles": quant, "count": cnt, "within": wth, "share": share, "levels": q, "thresholds": th, "edges": e,
            "replicas": np.bincount(ids[ids >= 0], minlength=n_groups), "quantile_ms": ms, "scratch_bytes": scratch,
            "window_of": window_of}


def sweep_order_segments(bounds: Any, index: Any, ids: Any) -> tuple[np.ndarray, np.ndarray, int]:
    """The exports of several runs (:meth:`BatchedResults._export_cells`) as ONE list of segments in the order of the whole
    sweep.  ``bounds[k]``: run k's window bounds, uint32 [n_k, W + 1]; ``index[k]`` [n_k]: its scenarios' places in the
    sweep; ``ids`` [n]: the sweep's group ids (negative: nothing was exported for the scenario).  A run's export holds its
    scenarios' segments one after the other, ``bounds[s][W] - bounds[s][0]`` latencies each, and the exports are
    concatenated in run order.  Returns the bounds [n, W + 1] and the segments' first elements uint64 [n] in sweep order,
    and the length of the concatenation."""
    ids = np.asarray(ids)
    n = int(sum(len(ix) for ix in index))
    width = int(np.asarray(bounds[0]).shape[1])
    out_b = np.zeros((n, width), dtype=np.uint32)
    begin = np.zeros(n, dtype=np.uint64)
    base = 0
    for b, ix in zip(bounds, index):
        b, ix = np.asarray(b, dtype=np.uint32), np.asarray(ix, dtype=np.int64)
        length = np.where(ids[ix] < 0, 0, b[:, -1].astype(np.int64) - b[:, 0].astype(np.int64))
        out_b[ix] = b
        begin[ix] = (base + np.cumsum(length) - length).astype(np.uint64)
        base += int(length.sum())
    return out_b, begin, base


def merge_cell_segments(parts: Any, index: Any, ids: Any, n_groups: int, W: int) -> list[np.ndarray]:
    """Host definition of the cells across devices (``af_engine_import_cells``): ``parts[k] = (lat, bounds)`` is run k's
    export, ``index`` / ``ids`` as in :func:`sweep_order_segments`, ``W`` the number of windows (0: the whole run, one cell
    per group).  Returns the ``n_groups * max(W, 1)`` cells, cell ``g * max(W, 1) + w`` the concatenation, in ascending
    sweep index over the members of group g, of the members' window w: the arrays the statistics are numpy's on."""
    ids = np.asarray(ids)
    wc = max(int(W), 1)
    bounds, begin, total = sweep_order_segments([p[1] for p in parts], index, ids)
    lat = np.concatenate([np.asarray(p[0], dtype=np.float64).reshape(-1) for p in parts]) if parts else np.zeros(0)
    if lat.shape[0] != total or bounds.shape[1] != wc + 1:
        msg = f"the exports hold {lat.shape[0]} latencies and {bounds.shape[1] - 1} windows, their bounds say {total} and the request {wc}"
        raise ValueError(msg)
    cells: list[list[np.ndarray]] = [[] for _ in range(int(n_groups) * wc)]
    for s in range(ids.shape[0]):
        if ids[s] < 0:
            continue
        at = int(begin[s]) - int(bounds[s, 0])
        for w in range(wc):
            cells[int(ids[s]) * wc + w].append(lat[at + int(bounds[s, w]): at + int(bounds[s, w + 1])])
    return [np.concatenate(c) if c else np.zeros(0, dtype=np.float64) for c in cells]


class ShardedResults:
    """A sweep run on several devices by ONE process (``SimulationRunner(devices=[...])``): the shards'
    :class:`BatchedResults` behind the indices of the original sweep."""

    def __init__(self, shards: list[BatchedResults], index: list[np.ndarray], wall_s: float) -> None:
        self.shards, self.index, self.wall_s = shards, index, wall_s
        n = sum(len(ix) for ix in index)
        self._where = np.zeros((n, 2), dtype=np.int64)
        for k, ix in enumerate(index):
            self._where[ix, 0] = k
            self._where[ix, 1] = np.arange(len(ix))
        self.plan = shards[0].plan
        self.counts = np.zeros((n, _abi.CNT_SLOTS), dtype=np.uint32)
        self.seeds = np.zeros(n, dtype=np.uint64)
        for k, ix in enumerate(index):
            self.counts[ix] = shards[k].counts
            self.seeds[ix] = shards[k].seeds
        self.kernel_ms = max(s.kernel_ms for s in shards)
        self.flow_reason = shards[0].flow_reason
        #: per-scenario parameter columns, in the order of the original sweep
        self.overrides: dict[str, np.ndarray] = {}
        for key in shards[0].overrides:
            col = np.zeros(n, dtype=np.float64)
            for k, ix in enumerate(index):
                col[ix] = shards[k].overrides[key]
            self.overrides[key] = col

    @property
    def engine_stats(self) -> list[_abi.AfStats]:
        """One ``af_stats_t`` per shard (per device), in shard order."""
        return [s.engine_stats for s in self.shards]

    def series_names(self) -> list[str]:
        return self.shards[0].series_names()

    def decode_series_max(self, words: np.ndarray) -> np.ndarray:
        return self.shards[0].decode_series_max(words)

    def save_summary(self, path: str, **kw: Any) -> dict[str, np.ndarray]:
        """:meth:`BatchedResults.save_summary` over every shard: the shards' columns are merged behind the indices of
        the original sweep and written once (``.npz`` / ``.parquet``)."""
        import tempfile

        if kw.get("hist_bins", 256) and kw.get("hist_max") is None:      # one histogram range for the whole sweep
            mx = 0.0
            for s in self.shards:
                st = s.summary(rps=False)["stats"].cpu().numpy()[:, 7]
                mx = max(mx, float(np.nanmax(st)) if np.isfinite(st).any() else 0.0)
            kw["hist_max"] = mx * 1.25 or 1.0
        n = len(self)
        cols: dict[str, np.ndarray] = {}
        with tempfile.TemporaryDirectory() as tmp:
            for k, (s, ix) in enumerate(zip(self.shards, self.index)):
                part = s.save_summary(f"{tmp}/shard{k}.npz", **kw)
                for name, v in part.items():
                    if v.shape[:1] == (len(ix),) and name not in ("latency_hist_edges", "series_names"):
                        if name not in cols:
                            cols[name] = np.zeros((n, *v.shape[1:]), dtype=v.dtype)
                        cols[name][ix] = v
                    else:
                        cols[name] = v
        path = str(path)
        if path.endswith(".parquet"):
            import pyarrow as pa
            import pyarrow.parquet as pq

            table = {k: (pa.array(list(v)) if v.ndim == 2 and v.shape[0] == n else pa.array(v))
                     for k, v in cols.items() if v.shape[:1] == (n,)}
            meta = {k: ",".join(map(str, v.tolist())) for k, v in cols.items() if v.shape[:1] != (n,)}
            pq.write_table(pa.table(table).replace_schema_metadata(meta), path)
        else:
            np.savez_compressed(path, **cols)
        return cols

    def __len__(self) -> int:
        return int(self.counts.shape[0])

    def __getitem__(self, i: int) -> ScenarioResults:
        k, j = self._where[int(i)]
        return self.shards[int(k)][int(j)]

    def __iter__(self) -> Iterator[ScenarioResults]:
        return (self[i] for i in range(len(self)))

    @property
    def flags(self) -> np.ndarray:
        return self.counts[:, _abi.CNT_FLAGS]

    @property
    def request_events(self) -> np.ndarray:
        return self.counts[:, _abi.CNT_EVENTS].astype(np.int64)

    def raise_on_overflow(self) -> None:
        for s in self.shards:
            s.raise_on_overflow()

    def raise_on_negative_delay(self) -> None:
        for s in self.shards:
            s.raise_on_negative_delay()

    def summary(self, **kw: Any) -> dict[str, Any]:
        """Per-scenario summaries of every shard (each computed on its own device), concatenated on the
        first shard's device in the order of the original sweep."""
        import torch

        parts = [s.summary(**kw) for s in self.shards]
        dev = parts[0]["stats"].device
        order = torch.as_tensor(np.argsort(np.concatenate(self.index), kind="stable"), device=dev)
        out: dict[str, Any] = {"keys": LATENCY_KEYS}
        for key in ("stats", "rps", "hist", "series_mean", "series_max"):
            if key in parts[0]:
                out[key] = torch.cat([p[key].to(dev) for p in parts], dim=0).index_select(0, order)
        return out

    def aggregate(self, level: float = 0.95, by: Any = None) -> dict[str, Any]:
        if by is not None:
            msg = "aggregate(by=...) of a sweep run on several devices: pooling across devices is not implemented"
            raise NotImplementedError(msg)
        return aggregate_summary(self.summary(rps=True), level)

    def pooled_summary(self, by: Any = None) -> dict[str, Any]:
        msg = "pooled_summary() of a sweep run on several devices: pooling across devices is not implemented"
        raise NotImplementedError(msg)

    def save_point_summary(self, path: str, by: Any, **kw: Any) -> dict[str, np.ndarray]:
        msg = "save_point_summary() of a sweep run on several devices: pooling across devices is not implemented"
        raise NotImplementedError(msg)

    def window_summary(self, *a: Any, **kw: Any) -> dict[str, Any]:
        msg = "window_summary() of a sweep run on several devices: windows across devices are not implemented"
        raise NotImplementedError(msg)

    def window_bands(self, *a: Any, **kw: Any) -> dict[str, Any]:
        msg = "window_bands() of a sweep run on several devices: windows across devices are not implemented"
        raise NotImplementedError(msg)

    def save_window_summary(self, *a: Any, **kw: Any) -> dict[str, np.ndarray]:
        msg = "save_window_summary() of a sweep run on several devices: windows across devices are not implemented"
        raise NotImplementedError(msg)

    def series_window_summary(self, *a: Any, **kw: Any) -> dict[str, Any]:
        msg = "series_window_summary() of a sweep run on several devices: windows across devices are not implemented"
        raise NotImplementedError(msg)

    def series_window_bands(self, *a: Any, **kw: Any) -> dict[str, Any]:
        msg = "series_window_bands() of a sweep run on several devices: windows across devices are not implemented"
        raise NotImplementedError(msg)

    def save_series_window_summary(self, *a: Any, **kw: Any) -> dict[str, np.ndarray]:
        msg = "save_series_window_summary() of a sweep run on several devices: windows across devices are not implemented"
        raise NotImplementedError(msg)

    def series_quantile_summary(self, *a: Any, **kw: Any) -> dict[str, Any]:
        msg = "series_quantile_summary() of a sweep run on several devices: windows across devices are not implemented"
        raise NotImplementedError(msg)

    def series_quantile_bands(self, *a: Any, **kw: Any) -> dict[str, Any]:
        msg = "series_quantile_bands() of a sweep run on several devices: windows across devices are not implemented"
        raise NotImplementedError(msg)

    def save_series_quantile_summary(self, *a: Any, **kw: Any) -> dict[str, np.ndarray]:
        msg = "save_series_quantile_summary() of a sweep run on several devices: windows across devices are not implemented"
        raise NotImplementedError(msg)

    def series_excursion_summary(self, *a: Any, **kw: Any) -> dict[str, Any]:
        msg = "series_excursion_summary() of a sweep run on several devices: windows across devices are not implemented"
        raise NotImplementedError(msg)

    def series_excursion_bands(self, *a: Any, **kw: Any) -> dict[str, Any]:
        msg = "series_excursion_bands() of a sweep run on several devices: windows across devices are not implemented"
        raise NotImplementedError(msg)

    def save_series_excursion_summary(self, *a: Any, **kw: Any) -> dict[str, np.ndarray]:
        msg = "save_series_excursion_summary() of a sweep run on several devices: windows across devices are not implemented"
        raise NotImplementedError(msg)

    def series_histogram_summary(self, *a: Any, **kw: Any) -> dict[str, Any]:
        msg = "series_histogram_summary() of a sweep run on several devices: windows across devices are not implemented"
        raise NotImplementedError(msg)

    def series_histogram_bands(self, *a: Any, **kw: Any) -> dict[str, Any]:
        msg = "series_histogram_bands() of a sweep run on several devices: windows across devices are not implemented"
        raise NotImplementedError(msg)

    def save_series_histogram_summary(self, *a: Any, **kw: Any) -> dict[str, np.ndarray]:
        msg = "save_series_histogram_summary() of a sweep run on several devices: windows across devices are not implemented"
        raise NotImplementedError(msg)

    def series_combined_summary(self, *a: Any, **kw: Any) -> dict[str, Any]:
        msg = "series_combined_summary() of a sweep run on several devices: windows across devices are not implemented"
        raise NotImplementedError(msg)

    def series_combined_bands(self, *a: Any, **kw: Any) -> dict[str, Any]:
        msg = "series_combined_bands() of a sweep run on several devices: windows across devices are not implemented"
        raise NotImplementedError(msg)

    def save_series_combined_summary(self, *a: Any, **kw: Any) -> dict[str, np.ndarray]:
        msg = "save_series_combined_summary() of a sweep run on several devices: windows across devices are not implemented"
        raise NotImplementedError(msg)

    def series_joint_summary(self, *a: Any, **kw: Any) -> dict[str, Any]:
        msg = "series_joint_summary() of a sweep run on several devices: windows across devices are not implemented"
        raise NotImplementedError(msg)

    def series_autocorrelation_summary(self, *a: Any, **kw: Any) -> dict[str, Any]:
        msg = "series_autocorrelation_summary() of a sweep run on several devices: windows across devices are not implemented"
        raise NotImplementedError(msg)

    def series_joint_bands(self, *a: Any, **kw: Any) -> dict[str, Any]:
        msg = "series_joint_bands() of a sweep run on several devices: windows across devices are not implemented"
        raise NotImplementedError(msg)

    def save_series_joint_summary(self, *a: Any, **kw: Any) -> dict[str, np.ndarray]:
        msg = "save_series_joint_summary() of a sweep run on several devices: windows across devices are not implemented"
        raise NotImplementedError(msg)

    def series_warmup_summary(self, *a: Any, **kw: Any) -> dict[str, Any]:
        msg = "series_warmup_summary() of a sweep run on several devices: windows across devices are not implemented"
        raise NotImplementedError(msg)

    def series_warmup_bands(self, *a: Any, **kw: Any) -> dict[str, Any]:
        msg = "series_warmup_bands() of a sweep run on several devices: windows across devices are not implemented"
        raise NotImplementedError(msg)

    def save_series_warmup_summary(self, *a: Any, **kw: Any) -> dict[str, np.ndarray]:
        msg = "save_series_warmup_summary() of a sweep run on several devices: windows across devices are not implemented"
        raise NotImplementedError(msg)

    def state_summary(self, *a: Any, **kw: Any) -> dict[str, Any]:
        msg = "state_summary() of a sweep run on several devices: windows across devices are not implemented"
        raise NotImplementedError(msg)

    def state_quantile_summary(self, *a: Any, **kw: Any) -> dict[str, Any]:
        msg = "state_quantile_summary() of a sweep run on several devices: windows across devices are not implemented"
        raise NotImplementedError(msg)

    def save_state_summary(self, *a: Any, **kw: Any) -> dict[str, np.ndarray]:
        msg = "save_state_summary() of a sweep run on several devices: windows across devices are not implemented"
        raise NotImplementedError(msg)

    def arrival_summary(self, *a: Any, **kw: Any) -> dict[str, Any]:
        msg = "arrival_summary() of a sweep run on several devices: windows across devices are not implemented"
        raise NotImplementedError(msg)

    def arrival_bands(self, *a: Any, **kw: Any) -> dict[str, Any]:
        msg = "arrival_bands() of a sweep run on several devices: windows across devices are not implemented"
        raise NotImplementedError(msg)

    def save_arrival_summary(self, *a: Any, **kw: Any) -> dict[str, np.ndarray]:
        msg = "save_arrival_summary() of a sweep run on several devices: windows across devices are not implemented"
        raise NotImplementedError(msg)

    def arrival_times(self, i: int) -> np.ndarray:
        k, j = self._where[int(i)]
        return self.shards[int(k)].arrival_times(int(j))

    def in_flight_summary(self, *a: Any, **kw: Any) -> dict[str, Any]:
        msg = "in_flight_summary() of a sweep run on several devices: windows across devices are not implemented"
        raise NotImplementedError(msg)

    def in_flight_bands(self, *a: Any, **kw: Any) -> dict[str, Any]:
        msg = "in_flight_bands() of a sweep run on several devices: windows across devices are not implemented"
        raise NotImplementedError(msg)

    def save_in_flight_summary(self, *a: Any, **kw: Any) -> dict[str, np.ndarray]:
        msg = "save_in_flight_summary() of a sweep run on several devices: windows across devices are not implemented"
        raise NotImplementedError(msg)

    def littles_law(self, *a: Any, **kw: Any) -> dict[str, Any]:
        msg = "littles_law() of a sweep run on several devices: windows across devices are not implemented"
        raise NotImplementedError(msg)

    def in_flight(self, i: int) -> dict[str, np.ndarray]:
        k, j = self._where[int(i)]
        return self.shards[int(k)].in_flight(int(j))

    def exemplar_summary(self, *a: Any, **kw: Any) -> dict[str, Any]:
        msg = "exemplar_summary() of a sweep run on several devices: windows across devices are not implemented"
        raise NotImplementedError(msg)

    def save_exemplar_summary(self, *a: Any, **kw: Any) -> dict[str, np.ndarray]:
        msg = "save_exemplar_summary() of a sweep run on several devices: windows across devices are not implemented"
        raise NotImplementedError(msg)

    def paired_summary(self, *a: Any, **kw: Any) -> dict[str, Any]:
        msg = ("paired_summary() of a sweep run on several devices: the two sides of a pair may sit on different devices, and sharing "
               "arrival rows across devices is not implemented")
        raise NotImplementedError(msg)

    def paired_bands(self, *a: Any, **kw: Any) -> dict[str, Any]:
        msg = "paired_bands() of a sweep run on several devices: pairs across devices are not implemented"
        raise NotImplementedError(msg)

    def save_paired_summary(self, *a: Any, **kw: Any) -> dict[str, np.ndarray]:
        msg = "save_paired_summary() of a sweep run on several devices: pairs across devices are not implemented"
        raise NotImplementedError(msg)

    def _histogram_groups(self, by: Any) -> tuple[np.ndarray, int]:
        """The GLOBAL group ids of ``by``, in the order of the original sweep: None, a Sweep, integer ids [n], ``"scenario"`` or
        the name(s) of per-scenario parameter columns -- resolved once, as the unsharded run resolves them."""
        n = len(self)
        named = _groups_of_named_columns(by, self.overrides)
        if named is not None:
            return named
        if isinstance(by, str):
            return np.arange(n, dtype=np.int64), n
        return resolve_groups(by, n)

    def latency_histogram_summary(self, window_s: float | None = None, *, edges: Any = None, by: Any = None, window_of: str = "finish",
                                  sub_bits: int = 5, min_exp: int = -20, octaves: int = 32) -> dict[str, Any]:
        """:meth:`BatchedResults.latency_histogram_summary` of a sweep run on several devices -- the grouped latency analyzer
        that works there, because histograms merge by integer addition.  ``by`` is resolved once over the whole sweep; every
        shard computes its members' contribution to the GLOBAL groups on its own device (explicit group ids through its
        ``index``), and the counts are added on the first shard's device.  Same arguments, same result as the unsharded run."""
        binning = check_latency_bins(sub_bits, min_exp, octaves)
        whole = window_s is None and edges is None
        if check_window_of(window_of) == "arrival" and whole:
            msg = "window_of='arrival' needs window_s or edges: the whole run has no window"
            raise ValueError(msg)
        e = None if whole else _resolve_edges(window_s, edges, self.plan.total_time)
        ids, n_groups = self._histogram_groups(by)
        out: dict[str, Any] = {}
        for shard, ix in zip(self.shards, self.index):
            shard._require_clock()  # noqa: SLF001
            part = shard._latency_histogram_cells(e, ids[np.asarray(ix)], n_groups, window_of, binning)  # noqa: SLF001
            if not out:
                out = part
                continue
            dev = out["hist"].device
            for k in _LHIST_COUNTS:
                out[k] = out[k] + part[k].to(dev)
            out["latency_histogram_ms"] += part["latency_histogram_ms"]
            out["scratch_bytes"] = max(out["scratch_bytes"], part["scratch_bytes"])
        out.update(bin_edges=latency_bin_edges(*binning[:3]), edges=e, replicas=np.bincount(ids[ids >= 0], minlength=n_groups),
                   sub_bits=binning[0], min_exp=binning[1], octaves=binning[2], window_of=window_of)
        return out

    def alert_summary(self, slo_s: float, rules: Any, window_s: float | None = None, *, ticks_per_window: int | None = None,
                      tick_edges: Any = None, by: Any = None, delay_bins: int = 0, delay_width_s: float | None = None,
                      per_tick: bool = False, timeout_s: float | None = None) -> dict[str, Any]:
        """:meth:`BatchedResults.alert_summary` of a sweep run on several devices: the group cells are integer sums, so every
        shard adds its members' part of the GLOBAL groups on its own device (``by`` is resolved once over the whole sweep, as
        in :meth:`latency_histogram_summary`) and the parts are added; the per-replica arrays go behind the indices of the
        original sweep.  With ``timeout_s`` every shard regenerates its own arrival rows.  Same arguments, same result as the
        unsharded run."""
        period = float(self.plan.sample_period)
        slo = float(slo_s)
        if math.isnan(slo):
            msg = "slo_s must not be NaN"
            raise ValueError(msg)
        tau = None if timeout_s is None else check_timeout(timeout_s)
        r6 = check_alert_rules(rules, period)
        n_bins, width = _alert_delay_bins(delay_bins, delay_width_s, period)
        b = _resolve_tick_edges(window_s, ticks_per_window, tick_edges, period, self.plan.tick_count)
        ids, n_groups = self._histogram_groups(by)
        n = len(self)
        out: dict[str, Any] = {"alerts_ms": 0.0, "scratch_bytes": 0}
        for shard, ix in zip(self.shards, self.index):
            ix = np.asarray(ix)
            part = shard._alert_call(b, ids[ix], n_groups, slo, r6, n_bins, width, bool(per_tick), tau)  # noqa: SLF001
            out["alerts_ms"] += part.pop("alerts_ms")
            out["scratch_bytes"] = max(out["scratch_bytes"], part.pop("scratch_bytes"))
            for k, v in part.items():
                if k in ALERT_GROUP_KEYS or k == "delay_hist":
                    out[k] = out[k] + v if k in out else v
                else:
                    if k not in out:
                        out[k] = np.zeros((n, *v.shape[1:]), dtype=v.dtype)
                    out[k][ix] = v
        if tau is not None:
            out["timeout_s"] = tau
        return _finish_alert_summary(out, r6, b, ids, n_groups, period, slo, n_bins, width)

    def save_alert_summary(self, path: str, slo_s: float, rules: Any, by: Any = None, **kw: Any) -> dict[str, np.ndarray]:
        """:meth:`BatchedResults.save_alert_summary` over every shard, added up and written once."""
        kw.pop("per_tick", None)
        return _save_alert_summary(self.alert_summary(slo_s, rules, by=by, **kw), str(path), by)

    def save_latency_histogram_summary(self, path: str, by: Any = None, **kw: Any) -> dict[str, np.ndarray]:
        """:meth:`BatchedResults.save_latency_histogram_summary` over every shard, added up and written once."""
        return _save_latency_histogram(self.latency_histogram_summary(kw.pop("window_s", None), by=by, **kw), str(path), by)

    def quantile_summary(self, *a: Any, **kw: Any) -> dict[str, Any]:
        msg = "quantile_summary() of a sweep run on several devices: quantiles across devices are not implemented"
        raise NotImplementedError(msg)

    def quantile_bands(self, *a: Any, **kw: Any) -> dict[str, Any]:
        msg = "quantile_bands() of a sweep run on several devices: quantiles across devices are not implemented"
        raise NotImplementedError(msg)

    def save_quantile_summary(self, *a: Any, **kw: Any) -> dict[str, np.ndarray]:
        msg = "save_quantile_summary() of a sweep run on several devices: quantiles across devices are not implemented"
        raise NotImplementedError(msg)


class ShardedCellResults(ShardedResults):
    """What ``SimulationRunner(devices=[...])`` returns: a :class:`ShardedResults` whose shards are live runs of ONE process, so
    that the cells of the exact grouped latency analyzers can cross the devices (csrc/af_cells.hpp).  A plain
    :class:`ShardedResults` -- shards put behind an index by hand -- keeps refusing them."""

    # ---- the exact grouped latency analyzers: cells across devices (csrc/af_cells.hpp) ------------------------------------------
    # A cell's sample is ONE array in a fixed order (ascending scenario index, then row order), and the members of a group sit on
    # several devices.  Every shard exports, on its own device, only the latencies that fall into the windows (8 B each); the
    # exports are concatenated on the first shard's device, their bounds and places reordered into sweep order on the host
    # (metadata only), and the first shard's analyzer engine merges them into the very array the unsharded call compacts and
    # reduces it with the same kernels: every word equals the unsharded run's.  The bands and the dumps compose from these
    # exactly as BatchedResults' do: they ARE its methods.

    def _require_clock(self) -> None:
        for s in self.shards:
            s._require_clock()  # noqa: SLF001

    def _window_groups(self, by: Any) -> tuple[np.ndarray, int]:
        return self._histogram_groups(by)

    def _behind_index(self, parts: list[Any]) -> Any:
        """Per-scenario tensors of the shards, concatenated on the first shard's device in the order of the original sweep."""
        import torch

        dev = parts[0].device
        order = torch.as_tensor(np.argsort(np.concatenate(self.index), kind="stable"), device=dev)
        return torch.cat([p.to(dev) for p in parts], dim=0).index_select(0, order)

    def _summarize_cells(self, e: np.ndarray | None, ids: np.ndarray, n_groups: int, window_of: str, *, stats: bool = False,
                         levels: np.ndarray | None = None, thresholds: np.ndarray | None = None) -> dict[str, Any]:
        """Export on every shard's device, concatenate on the first's, merge and reduce there (``af_engine_import_cells``).
        Returns the outputs asked for (``stats`` [G, W, 8]; ``count`` [G, W], ``quantiles`` [G, W, Q], ``within`` [G, W, T]
        with ``levels``), the bounds in sweep order (``row_bounds`` uint32 [n, W + 1]), ``ms`` (exports + reduction) and
        ``scratch_bytes`` (the largest of the engines')."""
        import torch

        from .engine import Engine

        parts = [shard._export_cells(e, ids[np.asarray(ix)], window_of) for shard, ix in zip(self.shards, self.index)]  # noqa: SLF001
        first = self.shards[0]
        dev = first._clock_t.device  # noqa: SLF001
        lat = torch.cat([p[0].to(dev) for p in parts])
        bounds, begin, n_lat = sweep_order_segments([p[1].cpu().numpy().view(np.uint32) for p in parts], self.index, ids)
        parts = [(None, None, p[2], p[3]) for p in parts]      # the exports are not needed any more: their devices get the memory back
        n_win = 0 if e is None else int(e.shape[0] - 1)
        wc = max(n_win, 1)
        out: dict[str, Any] = {"row_bounds": bounds}
        kw: dict[str, Any] = {}
        if stats:
            out["stats"] = torch.empty((n_groups, wc, 8), dtype=torch.float64, device=dev)
            kw["stats_ptr"] = out["stats"].data_ptr()
        if levels is not None:
            q, th = levels, thresholds if thresholds is not None else np.zeros(0)
            out["quantiles"] = torch.empty((n_groups, wc, q.shape[0]), dtype=torch.float64, device=dev)
            out["count"] = torch.empty((n_groups, wc), dtype=torch.int32, device=dev)
            out["within"] = torch.empty((n_groups, wc, th.shape[0]), dtype=torch.int32, device=dev)
            kw.update(levels=q, thresholds=th, count_ptr=out["count"].data_ptr(), quantiles_ptr=out["quantiles"].data_ptr() if q.shape[0] else 0,
                      within_ptr=out["within"].data_ptr() if th.shape[0] else 0)
        torch.cuda.synchronize(dev)
        if first._summ_engine is None:  # noqa: SLF001
            first._summ_engine = Engine(first.plan, dev.index if dev.index is not None else torch.cuda.current_device())  # noqa: SLF001
        group = np.where(ids < 0, _abi.POOL_SKIP, ids).astype(np.uint32)
        ms, scratch = first._summ_engine.import_cells(n_groups, n_win, bounds, begin, lat_ptr=lat.data_ptr(), n_lat=n_lat,  # noqa: SLF001
                                                         group=group, **kw)
        out["ms"] = ms + sum(p[2] for p in parts)
        out["scratch_bytes"] = max([scratch] + [p[3] for p in parts])
        return out

    def pooled_summary(self, by: Any = None) -> dict[str, Any]:
        """:meth:`BatchedResults.pooled_summary` of a sweep run on several devices: ``by`` is resolved once over the whole sweep,
        every shard exports its members' latencies on its own device, and the first shard's device merges and reduces them
        (one cell per group).  Same arguments, same keys, every word equal to the unsharded run's."""
        self._require_clock()
        ids, n_groups = self._histogram_groups(by)
        got = self._summarize_cells(None, ids, n_groups, "finish", stats=True)
        return {"stats": got["stats"][:, 0, :], "keys": LATENCY_KEYS, "replicas": np.bincount(ids[ids >= 0], minlength=n_groups), "pooled_ms": got["ms"]}

    def window_summary(self, window_s: float | None = None, *, edges: Any = None, by: Any = None,
                       row_bounds: bool = False, window_of: str = "finish") -> dict[str, Any]:
        """:meth:`BatchedResults.window_summary` of a sweep run on several devices, with its arguments and keys; every word
        equals the unsharded run's.  ``by="scenario"``: every shard runs its own call and the rows go behind the indices of
        the original sweep.  Otherwise the cells cross the shards: each exports the windowed latencies of its members on its
        own device, the first shard's device holds the import and the merged cells (16 B per windowed latency) and reduces
        them.  The returned tensors lie on the first shard's device."""
        import torch

        self._require_clock()
        check_window_of(window_of)
        e = _resolve_edges(window_s, edges, self.plan.total_time)
        ids, n_groups = self._histogram_groups(by)
        out: dict[str, Any] = {"edges": e, "keys": LATENCY_KEYS, "window_of": window_of, "replicas": np.bincount(ids[ids >= 0], minlength=n_groups)}
        if isinstance(by, str) and by == "scenario":
            parts = [s.window_summary(edges=e, by="scenario", row_bounds=row_bounds, window_of=window_of) for s in self.shards]
            out.update(stats=self._behind_index([p["stats"] for p in parts]), window_ms=sum(p["window_ms"] for p in parts),
                       scratch_bytes=max(p["scratch_bytes"] for p in parts))
            if row_bounds:
                out["row_bounds"] = self._behind_index([p["row_bounds"] for p in parts])
            return out
        got = self._summarize_cells(e, ids, n_groups, window_of, stats=True)
        out.update(stats=got["stats"], window_ms=got["ms"], scratch_bytes=got["scratch_bytes"])
        if row_bounds:
            out["row_bounds"] = torch.from_numpy(got["row_bounds"].view(np.int32)).to(got["stats"].device)
        return out

    def quantile_summary(self, levels: Any, *, thresholds: Any = None, window_s: float | None = None, edges: Any = None,
                         by: Any = None, window_of: str = "finish") -> dict[str, Any]:
        """:meth:`BatchedResults.quantile_summary` of a sweep run on several devices, with its arguments and keys; every word
        equals the unsharded run's.  The cells cross the shards as in :meth:`window_summary` (``by="scenario"``: per shard)."""
        self._require_clock()
        q, th = check_levels(levels), check_slo_thresholds(thresholds)
        if q.shape[0] == 0 and th.shape[0] == 0:
            msg = "quantile_summary needs at least one level or one threshold"
            raise ValueError(msg)
        whole = window_s is None and edges is None
        if check_window_of(window_of) == "arrival" and whole:
            msg = "window_of='arrival' needs window_s or edges: the whole run has no window"
            raise ValueError(msg)
        e = None if whole else _resolve_edges(window_s, edges, self.plan.total_time)
        ids, n_groups = self._histogram_groups(by)
        if isinstance(by, str) and by == "scenario":
            parts = [s.quantile_summary(q, thresholds=th, edges=e, by="scenario", window_of=window_of) for s in self.shards]
            out = {k: self._behind_index([p[k] for p in parts]) for k in ("quantiles", "count", "within", "share")}
            out.update(levels=q, thresholds=th, edges=e, replicas=np.bincount(ids[ids >= 0], minlength=n_groups),
                       quantile_ms=sum(p["quantile_ms"] for p in parts), scratch_bytes=max(p["scratch_bytes"] for p in parts), window_of=window_of)
            return out
        got = self._summarize_cells(e, ids, n_groups, window_of, levels=q, thresholds=th)
        return _finish_quantile_summary(got["quantiles"], got["count"], got["within"], q, th, e, ids, n_groups, got["ms"], got["scratch_bytes"],
                                        window_of)

    aggregate = BatchedResults.aggregate
    save_point_summary = BatchedResults.save_point_summary
    window_bands = BatchedResults.window_bands
    save_window_summary = BatchedResults.save_window_summary
    quantile_bands = BatchedResults.quantile_bands
    save_quantile_summary = BatchedResults.save_quantile_summary


def load_summary(path: str) -> dict[str, np.ndarray]:
    """Read a sweep summary written by :meth:`BatchedResults.save_summary` (``.npz`` or ``.parquet``)
    back into the same columns: one row per scenario (``seed``, ``param:*``, counts, ``latency:*``,
    ``rps`` [n, floor(T)], ``latency_hist`` [n, bins], ``series_mean`` / ``series_max`` [n, n_series])
    plus the per-sweep vectors (``latency_hist_edges``, ``series_names``)."""
    path = str(path)
    if path.endswith(".parquet"):
        import pyarrow.parquet as pq

        table = pq.read_table(path)
        cols: dict[str, np.ndarray] = {}
        for name in table.column_names:
            col = table.column(name).to_pylist()
            cols[name] = np.asarray(col, dtype=np.uint64 if name == "seed" else None)
        for k, v in (table.schema.metadata or {}).items():
            key, text = k.decode(), v.decode()
            if key == "series_names":
                cols[key] = np.asarray(text.split(","))
            elif key == "window_of":
                cols[key] = np.asarray(text)
            else:
                cols[key] = np.asarray([float(x) for x in text.split(",")] if text else [], dtype=np.float64)
        return cols
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}
