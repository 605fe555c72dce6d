"""The whole-run analyzer (af_engine_summarize) on hand-made device buffers: `series_mean`, `series_max`, `hist` and `rps`
against references stated here with numpy, exact integers and math.fsum -- every column layout of af_series_kernel (6, 12, 42
and 82 series), tick counts around one pass of a workgroup, integer sums beyond 2^32, RAM values that add exactly, arbitrary
float32 values and the negative residues the reference's float arithmetic leaves; latencies on and beside every bin edge,
finishes on and beside every window edge in every arrangement of an 8-lane group; the request at the documented LDS cap and
every refusal of the argument check.  Every output lies inside one buffer with sentinel words on both sides."""

from __future__ import annotations

import ctypes as C
import json
import math
from pathlib import Path

import numpy as np
import pytest

from asyncflow_amd import _abi
from asyncflow_amd.plan import lower
from oracle import analyzer_oracle as ao
from oracle.scenarios import lb_two_servers, single_server, wide_fanout

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GARBAGE = 0xDEADBEEF                       # padding words: the sign bit set
SENTINEL = 0x5A5A5A5A
GUARD = 64                                 # int32 words of sentinel between the outputs
SERIES_THREADS = 256                       # af_summary.hpp: kSeriesThreads
SHAPES = {"single_server": (6, 8), "lb_two_servers": (12, 12), "fanout8": (42, 44), "wide_fanout16": (82, 84)}


@pytest.fixture(params=["eight_waves", "four_waves"])
def last_pass(request, monkeypatch):
    """The forms of the analyzer's latency kernel: compiled for eight waves per SIMD (the default) or for four
    (AF_SUMMARY_WPE=4: `af_summary_kernel<4>`, eight loads in flight per thread instead of four)."""
    if request.param == "four_waves":
        monkeypatch.setenv("AF_SUMMARY_WPE", "4")
    else:
        monkeypatch.delenv("AF_SUMMARY_WPE", raising=False)
    return request.param


def ram_columns(n_series: int, n_edges: int) -> np.ndarray:
    """The ram_in_use columns (float32 words), stated here and not taken from the package: the edges come first, then
    ready_queue_len, event_loop_io_sleep, ram_in_use per server (include/asyncflow_hip.h)."""
    return np.array([j >= n_edges and (j - n_edges) % 3 == 2 for j in range(n_series)], dtype=bool)


def _plan(name: str):
    if name == "single_server":
        return lower(single_server(horizon=50))
    if name == "lb_two_servers":
        return lower(lb_two_servers(horizon=20))
    if name == "wide_fanout16":
        return lower(wide_fanout(16))
    z = np.load(ROOT / "tests" / "golden" / "fanout8_t20.npz")          # the 8-server fan-out: 42 series
    return lower(json.loads(str(z["payload_json"])))


def _block(plan, rng, n: int, cap: int, ticks, dyadic: bool = True):
    """Sample blocks [n, cap, pitch] of words (as tests/test_gpu_series_windows.py::_block): integer columns uniform in
    [0, 2^20], ram columns random multiples of 1/256 below 2^16 (or, dyadic=False, arbitrary non-negative float32 over many
    binades); padding words hold 0xDEADBEEF (sign bit set), the rows at and past a scenario's min(ticks, cap) random words
    whose exponent field is all ones, of either sign.  Returns the block and the counts."""
    S, pitch = plan.n_series, plan.series_pitch
    ram = ram_columns(S, plan.n_edges)
    blk = np.full((n, cap, pitch), GARBAGE, dtype=np.uint32)
    body = rng.integers(0, 2 ** 20 + 1, (n, cap, S)).astype(np.uint32)
    if dyadic:
        f = (rng.integers(0, 2 ** 24, (n, cap, int(ram.sum()))) / 256.0).astype(np.float32)
    else:
        f = (rng.lognormal(0.0, 6.0, (n, cap, int(ram.sum()))) * (rng.random((n, cap, int(ram.sum()))) > 0.1)).astype(np.float32)
    body[:, :, ram] = f.view(np.uint32)
    blk[:, :, :S] = body
    counts = np.zeros((n, _abi.CNT_SLOTS), dtype=np.uint32)
    counts[:, _abi.CNT_TICKS] = ticks
    for s in range(n):
        m = min(int(counts[s, _abi.CNT_TICKS]), cap)
        blk[s, m:] = rng.integers(0, 2 ** 32, (cap - m, pitch), dtype=np.uint32) | np.uint32(0x7F800000)
    return blk, counts


def _summarize(plan, n, counts, *, clock=None, samples=None, want=("stats", "rps", "hist", "series_mean", "series_max"),
               rps_buckets=0, hist_bins=0, hist_max=0.0, n_request=None, room=None):
    """One call of af_engine_summarize (the C entry) on a fresh engine.  Room for all five outputs lies in one buffer of
    sentinel words, a guard before and after each; only the outputs in `want` are handed over.  Returns the return code, the
    message, the outputs read back (those in `want`) and whether every other word of the buffer still holds the sentinel."""
    import torch

    from asyncflow_amd.engine import Engine, load_library

    lib = load_library()
    dev = torch.device("cuda", 0)
    S = plan.n_series
    B, H = (room or (max(rps_buckets, 1), max(hist_bins, 1)))
    sizes = {"stats": 2 * 8 * n, "rps": n * B, "hist": n * H, "series_mean": 2 * n * S, "series_max": n * S}
    off, at = {}, GUARD
    for k, sz in sizes.items():
        off[k] = at
        at += sz + GUARD + (sz + GUARD) % 2                              # (keeps every output 8-byte aligned)
    buf = torch.full((at,), SENTINEL, dtype=torch.int32, device=dev)
    ptr = {k: (buf.data_ptr() + 4 * o if k in want else None) for k, o in off.items()}
    clock_t = torch.as_tensor(clock, device=dev) if clock is not None else None
    samples_t = torch.as_tensor(samples.view(np.int32), device=dev) if samples is not None else None
    counts_t = torch.as_tensor(np.ascontiguousarray(counts).view(np.int32), device=dev)
    out = _abi.AfOutputs(int(clock.shape[1]) if clock is not None else 0, C.c_void_p(clock_t.data_ptr() if clock is not None else None),
                         int(samples.shape[1]) if samples is not None else 0,
                         C.c_void_p(samples_t.data_ptr() if samples is not None else None), C.c_void_p(counts_t.data_ptr()))
    req = _abi.AfSummary(int(n if n_request is None else n_request), int(rps_buckets), int(hist_bins), float(hist_max),
                         C.c_void_p(ptr["stats"]), C.c_void_p(ptr["rps"]), C.c_void_p(ptr["hist"]),
                         C.c_void_p(ptr["series_mean"]), C.c_void_p(ptr["series_max"]))
    eng = Engine(plan, 0)
    try:
        rc = lib.af_engine_summarize(eng._h, C.byref(out), C.byref(req))  # noqa: SLF001
        msg = (lib.af_last_error() or b"").decode() if rc != _abi.AF_OK else ""
        torch.cuda.synchronize(dev)
    finally:
        eng.close()
    host = buf.cpu().numpy()
    written = np.zeros(at, dtype=bool)
    got = {}
    if rc == _abi.AF_OK:
        used = {"stats": 2 * 8 * n, "rps": n * rps_buckets, "hist": n * hist_bins, "series_mean": 2 * n * S, "series_max": n * S}
        for k in want:
            written[off[k]:off[k] + used[k]] = True
            got[k] = host[off[k]:off[k] + used[k]].view(np.uint32)
        if "stats" in got:
            got["stats"] = got["stats"].view(np.float64).reshape(n, 8)
        if "rps" in got:
            got["rps"] = got["rps"].view(np.float32).reshape(n, rps_buckets)
        if "hist" in got:
            got["hist"] = got["hist"].reshape(n, hist_bins)
        if "series_mean" in got:
            got["series_mean"] = got["series_mean"].view(np.float64).reshape(n, S)
        if "series_max" in got:
            got["series_max"] = got["series_max"].reshape(n, S)
    return rc, msg, got, bool((host[~written] == np.int32(SENTINEL)).all())


def _series(plan, blk, counts, want=("series_mean", "series_max")):
    rc, msg, got, intact = _summarize(plan, blk.shape[0], counts, samples=blk, want=want)
    assert rc == _abi.AF_OK, msg
    assert intact, "a word outside the requested outputs was written"
    return got


# ------------------------------------------------------------------------------------------------ series mean and max
def _layout(plan) -> tuple[int, int, int]:
    pq = plan.series_pitch // 4
    stride = (SERIES_THREADS // pq) * pq
    return pq, stride, stride // pq


def _tick_counts(plan, rng, n: int, cap: int) -> np.ndarray:
    """No tick, one, two; one row fewer than / as many as / one more than a pass of the workgroup takes, two passes and one
    more row; every stored row; more than were stored (the clamp); the rest anywhere."""
    _, _, per = _layout(plan)
    fixed = [0, 1, 2, per - 1, per, per + 1, 2 * per, 2 * per + 1, cap, cap + 200]
    return np.array(fixed + rng.integers(1, cap + 1, n - len(fixed)).tolist())


def _values(plan, blk, s, m):
    """Scenario s of a block: its first m rows as words [S, m] and the ram columns' values as float64."""
    words = np.ascontiguousarray(blk[s, :m, :plan.n_series].T)
    ram = ram_columns(plan.n_series, plan.n_edges)
    return words, words[ram].view(np.float32).astype(np.float64)


def _max_want(words, values, ram):
    """Word maximum of the integer columns, the float maximum of the ram columns as float32 bits; no tick: 0."""
    mx = np.zeros(words.shape[0], dtype=np.uint32)
    if words.shape[1]:
        mx = words.max(axis=1)
        mx[ram] = values.max(axis=1).astype(np.float32).view(np.uint32)
    return mx


def _check_series(plan, blk, counts, got, what, exact_floats: bool):
    """Integer columns: the mean bit-equal to float(exact integer sum) / float(ticks).  RAM columns, exact_floats: multiples
    of 1/256 -- the exact rational sum (an integer count of 1/256ths) divided once; else within ticks * 2^-52 * sum|x| / ticks
    of math.fsum(x) / ticks (a sequential f64 sum of n terms errs by at most (n - 1) * 2^-53 * sum|x| to first order: this is
    twice that).  The maximum bit for bit."""
    n, cap, _ = blk.shape
    ram = ram_columns(plan.n_series, plan.n_edges)
    worst = 0.0
    for s in range(n):
        m = min(int(counts[s, _abi.CNT_TICKS]), cap)
        words, values = _values(plan, blk, s, m)
        assert np.array_equal(got["series_max"][s], _max_want(words, values, ram)), (what, s, m, "max")
        mean = got["series_mean"][s]
        if m == 0:
            assert np.isnan(mean).all(), (what, s)
            continue
        isum = [sum(int(w) for w in row) for row in words[~ram]]
        want_int = np.array([float(t) / float(m) for t in isum])
        assert np.array_equal(mean[~ram].view(np.uint64), want_int.view(np.uint64)), (what, s, m, "integer mean")
        if exact_floats:
            q = values * 256.0
            assert np.array_equal(q, np.floor(q))
            want_f = np.array([float(sum(int(v) for v in row)) / 256.0 / float(m) for row in q])
            assert np.array_equal(mean[ram].view(np.uint64), want_f.view(np.uint64)), (what, s, m, "ram mean")
        else:
            for got_mean, row in zip(mean[ram], values):
                ref = math.fsum(row.tolist()) / m
                bound = m * 2.0 ** -52 * math.fsum(np.abs(row).tolist()) / m
                worst = max(worst, abs(got_mean - ref) / bound if bound else 0.0)
                assert abs(got_mean - ref) <= bound, (what, s, m, got_mean, ref, bound)
    if not exact_floats:
        print(f"{what}: largest |mean - fsum / n| / bound = {worst:.3g}")


def _wide_integer_column(blk, counts, rng, cap):
    """Column 0 (an edge's connection count in every plan): words up to 2^31 - 1; 700 of them add up to far beyond 2^32."""
    n = blk.shape[0]
    for s in range(n):
        m = min(int(counts[s, _abi.CNT_TICKS]), cap)
        blk[s, :m, 0] = rng.integers(0, 2 ** 31, m).astype(np.uint32)
        if m:
            blk[s, rng.integers(0, m), 0] = 2 ** 31 - 1
    full = int(np.argmax(np.minimum(counts[:, _abi.CNT_TICKS], cap)))
    assert int(blk[full, :cap, 0].astype(np.int64).sum()) > 2 ** 32


def _windows_whole_run(plan, blk, counts):
    """af_engine_summarize_series_windows with the single window [0, cap] and singleton groups: mean and max words."""
    import torch

    from asyncflow_amd.engine import Engine

    n, cap, _ = blk.shape
    S = plan.n_series
    dev = torch.device("cuda", 0)
    blk_t = torch.as_tensor(blk.view(np.int32), device=dev)
    counts_t = torch.as_tensor(counts.view(np.int32), device=dev)
    grp = torch.arange(n, dtype=torch.int32, device=dev)
    count = torch.zeros((n, 1), dtype=torch.int32, device=dev)
    mean = torch.zeros((n, 1, S), dtype=torch.float64, device=dev)
    mx = torch.zeros((n, 1, S), dtype=torch.int32, device=dev)
    eng = Engine(plan, 0)
    try:
        eng.summarize_series_windows(n, n, [0, cap], samples_ptr=blk_t.data_ptr(), tick_capacity=cap, counts_ptr=counts_t.data_ptr(),
                                     count_ptr=count.data_ptr(), mean_ptr=mean.data_ptr(), max_ptr=mx.data_ptr(), group_ptr=grp.data_ptr())
    finally:
        eng.close()
    return mean.cpu().numpy()[:, 0], mx.cpu().numpy().view(np.uint32)[:, 0]


@pytest.mark.parametrize("name", list(SHAPES))
def test_series_mean_and_max_of_values_that_add_exactly(name):
    plan = _plan(name)
    assert (plan.n_series, plan.series_pitch) == SHAPES[name]
    rng = np.random.default_rng(100 + len(name))
    n, cap = 24, 700
    blk, counts = _block(plan, rng, n, cap, _tick_counts(plan, rng, n, cap))
    _wide_integer_column(blk, counts, rng, cap)
    got = _series(plan, blk, counts)
    _check_series(plan, blk, counts, got, name, exact_floats=True)
    # the series-windows analyzer over the whole run, every scenario a group of its own: the same bytes
    w_mean, w_max = _windows_whole_run(plan, blk, counts)
    some = np.minimum(counts[:, _abi.CNT_TICKS], cap) > 0
    assert got["series_mean"][some].tobytes() == w_mean[some].tobytes() and np.isnan(w_mean[~some]).all()
    assert np.array_equal(got["series_max"], w_max)
    # NULL outputs: the other buffer and every sentinel stay untouched (_series asserts it)
    only_mean = _series(plan, blk, counts, want=("series_mean",))
    only_max = _series(plan, blk, counts, want=("series_max",))
    assert set(only_mean) == {"series_mean"} and set(only_max) == {"series_max"}
    assert only_mean["series_mean"].tobytes() == got["series_mean"].tobytes()
    assert only_max["series_max"].tobytes() == got["series_max"].tobytes()


def test_series_of_a_run_of_60000_ticks():
    plan = _plan("lb_two_servers")
    rng = np.random.default_rng(60)
    for dyadic in (True, False):
        blk, counts = _block(plan, rng, 1, 60_000, [60_000], dyadic=dyadic)
        _wide_integer_column(blk, counts, rng, 60_000)
        _check_series(plan, blk, counts, _series(plan, blk, counts), f"60 000 ticks, dyadic={dyadic}", exact_floats=dyadic)


@pytest.mark.parametrize("name", list(SHAPES))
def test_series_of_arbitrary_float_values_run_to_run_and_batch_independence(name):
    plan = _plan(name)
    rng = np.random.default_rng(200 + len(name))
    n, cap = 24, 700
    blk, counts = _block(plan, rng, n, cap, _tick_counts(plan, rng, n, cap), dyadic=False)
    got = _series(plan, blk, counts)
    _check_series(plan, blk, counts, got, name, exact_floats=False)
    again = _series(plan, blk, counts)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k                  # the same call twice: identical bytes
    # the same scenarios inside a batch ten times as large: identical bytes for their rows
    big, big_counts = _block(plan, rng, 10 * n, cap, rng.integers(0, cap + 1, 10 * n), dyadic=False)
    where = np.arange(n) * 10 + 3
    big[where], big_counts[where] = blk, counts
    inside = _series(plan, big, big_counts)
    for k in got:
        assert got[k].tobytes() == np.ascontiguousarray(inside[k][where]).tobytes(), k


@pytest.mark.parametrize("name", list(SHAPES))
def test_series_max_is_the_float_maximum_when_ram_values_are_negative(name):
    """The reference's float arithmetic leaves residues such as -2.8e-14 MB in ram_in_use (tests/golden/
    frac_ram_waiting_put_t20.npz holds 179 of them); as words they are larger than every positive value.  Scenario s, all of
    its ram columns: s % 5 = 0: one sample of -2^-45 among dyadic positives; 1: 179 of them; 2: all but one; 3: every sample
    negative, distinct magnitudes (the maximum is the one closest to zero); 4: every sample +0.0.  (No -0.0: the engine does
    not produce it, and a tie of +0 and -0 has no defined winner.)"""
    plan = _plan(name)
    _, _, per = _layout(plan)
    ram = ram_columns(plan.n_series, plan.n_edges)
    rng = np.random.default_rng(300 + len(name))
    cap = 700
    ticks = np.array([700, 333, per + 1, 1, 5, 2, 700, 2 * per + 1, per + 1, per - 1, per, 900, 2, per - 1, 2 * per, 3, 180, 700, 700, 64])
    n = len(ticks)
    blk, counts = _block(plan, rng, n, cap, ticks)
    residue = np.float32(-(2.0 ** -45))
    for s in range(n):
        m = min(int(ticks[s]), cap)
        kind = s % 5
        for j in np.nonzero(ram)[0]:
            col = blk[s, :m, j].view(np.float32)                           # (a view into the block)
            if kind in (0, 1, 2):
                k = {0: 1, 1: 179, 2: m - 1}[kind]
                assert 1 <= k < m, (s, m)
                col[rng.choice(m, k, replace=False)] = residue
                assert (col < 0).sum() == k and (col >= 0).sum() == m - k
            elif kind == 3:
                col[:] = -((1 + rng.permutation(m)).astype(np.float32) / np.float32(256.0)) * np.float32(2.0 ** float(rng.integers(-30, 10)))
                assert np.unique(col).size == m and (col < 0).all()
            else:
                col[:] = np.float32(0.0)
        assert not (blk[s, :m, :plan.n_series][:, ram] == 0x80000000).any()
    got = _series(plan, blk, counts)
    for s in range(n):                                                      # stated once more, plainly
        m = min(int(ticks[s]), cap)
        values = blk[s, :m, :plan.n_series][:, ram].view(np.float32)
        assert np.array_equal(got["series_max"][s, ram], values.max(axis=0).astype(np.float32).view(np.uint32)), (s, s % 5, m)
    _check_series(plan, blk, counts, got, name, exact_floats=False)


def test_series_of_the_fractional_ram_fixture():
    """tests/golden/frac_ram_waiting_put_t20.npz, written by the unmodified reference: 179 of the 399 samples of series 8 are
    -2.84e-14.  Its sample words as a block against the analyzer oracle, then its payload and seed through the runner."""
    from asyncflow_amd.runner import SimulationRunner

    fx = np.load(ROOT / "tests" / "golden" / "frac_ram_waiting_put_t20.npz", allow_pickle=False)
    payload = json.loads(str(fx["payload_json"]))
    plan = lower(payload)
    words = fx["samples"]
    assert words.shape == (12, 399) and (plan.n_series, plan.series_pitch) == (12, 12)
    ram = ram_columns(plan.n_series, plan.n_edges)
    neg = (words[8].view(np.float32) < 0)
    assert ram[8] and neg.sum() == 179 and words[8].max() == words[8][neg].max()      # as words they are the column's largest
    blk = np.ascontiguousarray(words.T)[None]
    counts = np.zeros((1, _abi.CNT_SLOTS), dtype=np.uint32)
    counts[0, _abi.CNT_TICKS] = 399
    got = _series(plan, blk, counts)
    mean, mx = ao.series_mean_max(words, plan.n_edges)
    assert np.array_equal(got["series_max"][0], mx), (got["series_max"][0].view(np.float32), mx.view(np.float32))
    assert np.array_equal(got["series_mean"][0, ~ram].view(np.uint64), mean[~ram].view(np.uint64))
    _check_series(plan, blk, counts, got, "fixture", exact_floats=False)
    for j in np.nonzero(ram)[0]:
        v = words[j].view(np.float32).astype(np.float64)
        assert abs(got["series_mean"][0, j] - mean[j]) <= 2 * 399 * 2.0 ** -52 * np.abs(v).sum() / 399    # (the oracle's own sum errs too)
    # the run itself (the parity tests hold its samples to the fixture's)
    res = SimulationRunner(simulation_input=payload, seeds=[int(fx["seed"])]).run()
    assert np.array_equal(res[0]._samples, words)  # noqa: SLF001
    peak = res.decode_series_max(res.summary(rps=False, series=True)["series_max"].cpu().numpy())
    sampled = res[0].get_sampled_metrics()
    for v, sid in enumerate(res.plan.server_ids):
        assert peak[0, res.plan.n_edges + 3 * v + 2] == max(sampled["ram_in_use"][sid]) > 100.0, sid


# ------------------------------------------------------------------------------------------------------- histogram
def _latency_plan():
    return lower(single_server(horizon=50))


def _clock_batch(rows_list):
    """[(start, finish)] per scenario -> clock [n, cap, 2] (NaN past a scenario's rows) and counts."""
    n = len(rows_list)
    cap = max(r.shape[0] for r in rows_list)
    clock = np.full((n, cap, 2), np.nan)
    counts = np.zeros((n, _abi.CNT_SLOTS), dtype=np.uint32)
    for i, r in enumerate(rows_list):
        clock[i, :r.shape[0]] = r
        counts[i, _abi.CNT_COMPLETED] = r.shape[0]
    return clock, counts


def _edge_latencies(bins: int, hist_max: float) -> np.ndarray:
    """k / scale for every k in 0 .. bins + 1 with its two nearest doubles on each side (none below zero), and 0.0, the
    smallest subnormal, 10 * hist_max, 1e300."""
    scale = np.float64(bins) / np.float64(hist_max)
    e = np.arange(bins + 2, dtype=np.float64) / scale
    d1, d2 = np.nextafter(e, -np.inf), np.nextafter(np.nextafter(e, -np.inf), -np.inf)
    u1, u2 = np.nextafter(e, np.inf), np.nextafter(np.nextafter(e, np.inf), np.inf)
    lat = np.concatenate([e, d1, d2, u1, u2, [0.0, 5e-324, 10.0 * hist_max, 1e300]])
    return lat[lat >= 0.0]


def _hist_want(lat, bins, hist_max):
    b = np.minimum(np.floor(lat * (np.float64(bins) / np.float64(hist_max))), bins - 1)
    return np.bincount(b.astype(np.int64), minlength=bins).astype(np.uint32)


HIST_PAIRS = [(1, 1.0), (2, 0.3), (64, 0.128), (2048, 0.256), (8192, 1.0), (8192, 0.7)]


@pytest.mark.parametrize(("bins", "hist_max"), HIST_PAIRS)
def test_histogram_on_and_beside_every_bin_edge(bins, hist_max, last_pass):
    """The definition: bin = min(floor(fl(lat * fl(bins / hist_max))), bins - 1)."""
    rng = np.random.default_rng(bins)
    lat = rng.permutation(_edge_latencies(bins, hist_max))
    scale = np.float64(bins) / np.float64(hist_max)
    if math.frexp(float(scale))[0] != 0.5:      # not a power of two: the products round, and near-miss formulas differ on edges
        by_width = np.minimum(np.floor(lat / (np.float64(hist_max) / np.float64(bins))), bins - 1)
        differ = int((by_width != np.minimum(np.floor(lat * scale), bins - 1)).sum())
        print(f"{bins} bins over {hist_max} s: 'divide by the bin width' puts {differ} of {lat.size} latencies into another bin")
        if (bins, hist_max) == (2, 0.3):      # two bins: four edges, none of them rounds differently -- noticed if the inputs change
            assert differ == 0
        else:
            assert differ >= 1
    starts = rng.uniform(0.0, 40.0, lat.size)
    moved = np.stack([starts, starts + lat], axis=1)              # finish - start rounds: the latency is what the subtraction gives
    equal = np.full(200_001, hist_max / 3.0)                      # one bin takes every atomic
    rows = [np.stack([np.zeros(lat.size), lat], axis=1), moved, np.stack([np.zeros(equal.size), equal], axis=1)]
    assert np.array_equal(rows[0][:, 1] - rows[0][:, 0], lat) and ((moved[:, 1] - moved[:, 0]) != lat).any()
    clock, counts = _clock_batch(rows)
    rc, msg, got, intact = _summarize(_latency_plan(), 3, counts, clock=clock, want=("stats", "hist"), hist_bins=bins, hist_max=hist_max)
    assert rc == _abi.AF_OK, msg
    assert intact
    for i, r in enumerate(rows):
        want = _hist_want(r[:, 1] - r[:, 0], bins, hist_max)
        assert np.array_equal(got["hist"][i], want), (i, np.nonzero(got["hist"][i] != want)[0][:8])
        assert int(got["hist"][i].astype(np.int64).sum()) == r.shape[0] == int(got["stats"][i, 0])
        assert np.array_equal(got["hist"][i], ao.latency_histogram(r, bins, hist_max))
    assert got["hist"][2].max() == 200_001


# ------------------------------------------------------------------------------------------------------ RPS windows
RPS_BUCKETS = (1, 7, 50, 600)
RPS_ROWS = [*range(1, 18), 63, 64, 65, 511, 512, 513, 8191, 8192, 8193]


def _in_bucket(rng, b: int) -> float:
    """A finish in window (b - 1, b], b >= 1: its right edge, the double below it, the double above its left edge, its middle
    -- and 0.0 exactly for the first window."""
    pick = rng.integers(0, 5 if b == 1 else 4)
    return [float(b), float(np.nextafter(float(b), -np.inf)), float(np.nextafter(float(b - 1), np.inf)), b - 0.5, 0.0][pick]


def _beyond(rng, b: int) -> float:
    return [float(np.nextafter(float(b), np.inf)), b + 1.0, b + 2.0, 1e6, 5e9, 1e300][rng.integers(0, 6)]


def _rps_rows() -> list[np.ndarray]:
    """Per scenario of RPS_ROWS rows: blocks of eight consecutive rows, each arranged for one of the bucket counts B -- all in
    the same bucket; the first row different from the other seven; alternating between two buckets; eight distinct buckets;
    the first row beyond the last bucket and the rest inside; all beyond.  The three long scenarios end with every integer
    0 .. 602 and its neighbours on both sides, 0.0, 1e6, 5e9 and 1e300."""
    rng = np.random.default_rng(8)
    ints = np.arange(0, 603, dtype=np.float64)
    pool = np.concatenate([ints, np.nextafter(ints, -np.inf)[1:], np.nextafter(ints, np.inf), [0.0, 1e6, 5e9, 1e300]])
    out = []
    for r in RPS_ROWS:
        fin: list[float] = []
        while len(fin) < r:
            B = int(rng.choice(RPS_BUCKETS))
            a, b = (int(x) for x in rng.integers(1, B + 1, 2))
            kind = rng.integers(0, 6)
            if kind == 0:
                fin += [_in_bucket(rng, a) for _ in range(8)]
            elif kind == 1:
                fin += [_in_bucket(rng, a)] + [_in_bucket(rng, b) for _ in range(7)]
            elif kind == 2:
                fin += [_in_bucket(rng, a if t % 2 else b) for t in range(8)]
            elif kind == 3:
                fin += [_in_bucket(rng, 1 + (a + t) % max(B, 8)) for t in range(8)]
            elif kind == 4:
                fin += [_beyond(rng, B)] + [_in_bucket(rng, b) for _ in range(7)]
            else:
                fin += [_beyond(rng, B) for _ in range(8)]
        fin_a = np.array(fin[:r])
        if r > 8000:
            fin_a[-pool.size:] = rng.permutation(pool)
        assert (fin_a >= 0.0).all() and np.isfinite(fin_a).all()
        out.append(np.stack([np.zeros(r), fin_a], axis=1))
    return out


_RPS_CACHE: dict = {}


def _rps_case():
    """The rows and, per bucket count, both references -- computed once, shared by the kernel forms, left unchanged."""
    if not _RPS_CACHE:
        rows = _rps_rows()
        want = {}
        for B in RPS_BUCKETS:
            per = []
            for r in rows:
                k = np.maximum(np.ceil(r[:, 1]), 1.0)
                k = k[k <= B].astype(np.int64)
                by_count = np.bincount(k - 1, minlength=B).astype(np.float64)
                oracle = ao.throughput_series(r, B)[1]
                assert np.array_equal(by_count, oracle)
                per.append(by_count)
            want[B] = np.stack(per)
        _RPS_CACHE["rows"], _RPS_CACHE["want"] = rows, want
    return _RPS_CACHE["rows"], _RPS_CACHE["want"]


@pytest.mark.parametrize("buckets", RPS_BUCKETS)
def test_rps_windows_on_and_beside_every_window_edge(buckets, last_pass):
    rows, want = _rps_case()
    clock, counts = _clock_batch(rows)
    n = len(rows)
    rc, msg, got, intact = _summarize(_latency_plan(), n, counts, clock=clock, want=("stats", "rps"), rps_buckets=buckets)
    assert rc == _abi.AF_OK, msg
    assert intact
    assert want[buckets].max() < 2 ** 24                                # (float32 holds every count)
    for i in range(n):
        assert np.array_equal(got["rps"][i].astype(np.float64), want[buckets][i]), (RPS_ROWS[i], np.nonzero(got["rps"][i] != want[buckets][i])[0][:8])
    assert np.array_equal(got["stats"][:, 0], np.array(RPS_ROWS, dtype=np.float64))
    inside = sum(int((np.maximum(np.ceil(r[:, 1]), 1.0) <= buckets).sum()) for r in rows)
    assert 0 < inside < sum(RPS_ROWS) and int(got["rps"].astype(np.float64).sum()) == inside


# ------------------------------------------------------------------------------------------------- the documented cap
def test_a_request_at_the_documented_lds_cap_and_one_word_beyond(last_pass):
    """include/asyncflow_hip.h: rps_buckets + hist_bins <= 24 576 words of LDS beside the kernel's own."""
    rng = np.random.default_rng(24576)
    bins, buckets, hist_max = 8192, 16_384, 0.7
    m = 20_000
    on_edges = np.stack([np.zeros(buckets + 3), np.arange(buckets + 3, dtype=np.float64)], axis=1)   # a finish on every window edge, three beyond
    starts = rng.uniform(0.0, buckets + 6.0, m - on_edges.shape[0])
    lat = rng.choice(_edge_latencies(bins, hist_max), starts.size)       # latencies on and beside bin edges, from anywhere in the run
    rows = rng.permutation(np.concatenate([on_edges, np.stack([starts, starts + lat], axis=1)]))
    assert rows.shape == (m, 2)
    clock, counts = _clock_batch([rows])
    rc, msg, got, intact = _summarize(_latency_plan(), 1, counts, clock=clock, want=("stats", "rps", "hist"), rps_buckets=buckets,
                                      hist_bins=bins, hist_max=hist_max)
    assert rc == _abi.AF_OK, msg
    assert intact
    fin = rows[:, 1]
    k = np.maximum(np.ceil(fin), 1.0)
    assert (k > buckets).any()
    assert np.array_equal(got["rps"][0].astype(np.float64), np.bincount(k[k <= buckets].astype(np.int64) - 1, minlength=buckets))
    assert np.array_equal(got["hist"][0], _hist_want(fin - rows[:, 0], bins, hist_max)) and int(got["hist"][0].sum()) == m
    assert np.array_equal(got["stats"][0].view(np.uint64), ao.latency_stats(rows).view(np.uint64))
    # one word more is refused before any launch
    rc, msg, _, intact = _summarize(_latency_plan(), 1, counts, clock=clock, want=("stats", "rps", "hist"), rps_buckets=buckets + 1,
                                    hist_bins=bins, hist_max=hist_max)
    assert rc == _abi.AF_ERR_CAPACITY and "24576" in msg, (rc, msg)
    assert intact


# ------------------------------------------------------------------------------------- every refusal of the argument check
def test_every_refusal_of_the_argument_check_leaves_the_outputs_untouched():
    plan = _plan("lb_two_servers")
    rng = np.random.default_rng(1)
    blk, counts = _block(plan, rng, 2, 40, [40, 13])
    counts[:, _abi.CNT_COMPLETED] = [5, 3]
    clock = np.cumsum(rng.exponential(0.1, (2, 8, 2)), axis=2)
    nan = float("nan")
    room = (16, 8200)
    cases = [
        ("rps without stats", dict(clock=clock, want=("rps",), rps_buckets=10), "stats is required"),
        ("hist without stats", dict(clock=clock, want=("hist",), hist_bins=8, hist_max=1.0), "stats is required"),
        ("no bin", dict(clock=clock, want=("stats", "hist"), hist_bins=0, hist_max=1.0), "hist_bins must be 1..8192"),
        ("8 193 bins", dict(clock=clock, want=("stats", "hist"), hist_bins=8193, hist_max=1.0), "hist_bins must be 1..8192"),
        ("hist_max 0", dict(clock=clock, want=("stats", "hist"), hist_bins=8, hist_max=0.0), "hist_max > 0"),
        ("hist_max < 0", dict(clock=clock, want=("stats", "hist"), hist_bins=8, hist_max=-1.0), "hist_max > 0"),
        ("hist_max NaN", dict(clock=clock, want=("stats", "hist"), hist_bins=8, hist_max=nan), "hist_max > 0"),
        ("no bucket", dict(clock=clock, want=("stats", "rps"), rps_buckets=0), "zero buckets"),
        ("series mean without samples", dict(clock=clock, want=("series_mean",)), "needs outputs.samples"),
        ("series max without samples", dict(want=("series_max",)), "needs outputs.samples"),
        ("stats without a clock", dict(samples=blk, want=("stats",)), "needs outputs.clock"),
        ("rps without a clock", dict(samples=blk, want=("stats", "rps"), rps_buckets=10), "needs outputs.clock"),
        ("no scenario", dict(clock=clock, samples=blk, want=("stats", "series_mean", "series_max"), n_request=0), "empty summary request"),
    ]
    for what, kw, text in cases:
        rc, msg, _, intact = _summarize(plan, 2, counts, room=room, **kw)
        assert rc == _abi.AF_ERR_INVALID and text in msg, (what, rc, msg)
        assert intact, what
    # ... and the same buffers are accepted once the request is whole
    rc, msg, got, intact = _summarize(plan, 2, counts, clock=clock, samples=blk, rps_buckets=10, hist_bins=8, hist_max=1.0, room=room)
    assert rc == _abi.AF_OK and intact, msg
    assert got["stats"][:, 0].tolist() == [5.0, 3.0] and got["hist"].sum(axis=1).tolist() == [5, 3]
