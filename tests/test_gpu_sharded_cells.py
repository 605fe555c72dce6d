"""Cells across devices (asyncflow_amd/csrc/af_cells.hpp) on ONE MI355X, both shards on device 0 as in tests/test_gpu_multi.py:
the exact grouped latency analyzers of a sweep run with ``devices=[0, 0]`` against the same sweep run unsharded, bit for bit;
``af_engine_export_cells`` / ``af_engine_import_cells`` through the C ABI on hand-made clock buffers against the one-device
entry points on the concatenated buffers and against numpy on `results.merge_cell_segments`; their refusals; and both calls
whatever the scratch pool held before.  Every output of a C call lies in one buffer between sentinel words."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from asyncflow_amd import _abi, expand_grid
from asyncflow_amd import results as R
from asyncflow_amd.plan import lower
from asyncflow_amd.sweep import Sweep
from asyncflow_amd.workloads import lb_two_servers

pytestmark = pytest.mark.gpu

USERS = "rqs_input.avg_active_users.mean"
LEVELS, SLO_THR = (0.5, 0.9, 0.999, 0.0, 1.0), (0.02, 0.05)
SENTINEL = 0x5A5A5A5A
GUARD = 16                                     # sentinel words on both sides of every output (outputs stay 16-byte aligned)
TINY_MAX, SMALL_MAX = 512, 8192                # af_windowed.hpp: kTinyMax, kSmallMax -- the tiers of the reduction


# ---- sweep against sweep -----------------------------------------------------------------------------------------------------------
def _same(got: dict, want: dict, what: str) -> None:
    """Every array of two result dicts, word for word (floats as their bit patterns, NaNs included); the timings and the scratch
    sizes are the only keys that may differ."""
    assert set(got) == set(want), (what, sorted(set(got) ^ set(want)))
    for k, w in want.items():
        if k.endswith("_ms") or k == "scratch_bytes":
            continue
        g = got[k]
        if hasattr(w, "cpu"):
            assert hasattr(g, "cpu") and g.dtype == w.dtype and tuple(g.shape) == tuple(w.shape), (what, k)
            g, w = g.cpu().numpy(), w.cpu().numpy()
        if isinstance(w, np.ndarray):
            g = np.asarray(g)
            assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
            if w.dtype.kind == "f":
                g, w = g.view(np.uint64 if w.dtype.itemsize == 8 else np.uint32), w.view(np.uint64 if w.dtype.itemsize == 8 else np.uint32)
            assert np.array_equal(g, w), (what, k, int((g != w).sum()))
        else:
            assert g == w, (what, k, g, w)


def _permuted(grid: Sweep, seed: int) -> Sweep:
    perm = np.random.default_rng(seed).permutation(len(grid))
    return Sweep(columns={k: np.ascontiguousarray(v[perm]) for k, v in grid.columns.items()}, seeds=np.ascontiguousarray(grid.seeds[perm]),
                 point=grid.point[perm], replica=grid.replica[perm], shape=grid.shape, axes=grid.axes)


def test_sharded_sweep_equals_the_unsharded_sweep(tmp_path):
    from asyncflow_amd.runner import SimulationRunner

    payload = lb_two_servers(horizon=20)
    grid = _permuted(expand_grid({USERS: [60.0, 150.0, 400.0]}, replicas=10), 3)
    n = len(grid)
    assert n == 30
    one = SimulationRunner(simulation_input=payload, **grid.runner_kwargs()).run()
    two = SimulationRunner(simulation_input=payload, **grid.runner_kwargs(), devices=[0, 0]).run()
    assert isinstance(two, R.ShardedCellResults) and len(two.shards) == 2 and np.array_equal(two.counts[:, :6], one.counts[:, :6])
    some = np.where(np.arange(n) % 7 == 3, -1, grid.point)
    for ids in (grid.point, some):                                   # otherwise nothing crosses a shard
        for g in range(3):
            assert all((ids[np.asarray(ix)] == g).any() for ix in two.index), (g, [ids[np.asarray(ix)].tolist() for ix in two.index])
    totals: list[np.ndarray] = []

    def both(what: str, call) -> dict:
        want, got = call(one), call(two)
        _same(got, want, what)
        for k in ("stats", "count"):
            if k in want:
                t = want[k].cpu().numpy()
                totals.append((t[..., 0] if k == "stats" else t).reshape(-1).astype(np.int64))
        return got

    for by, tag in ((grid, "grid"), (some, "ids"), (None, "none")):
        both(f"pooled_summary by {tag}", lambda r, by=by: r.pooled_summary(by))
    for window_of in ("finish", "arrival"):
        both(f"window_summary 5 s by grid, {window_of}", lambda r, w=window_of: r.window_summary(5.0, by=grid, window_of=w, row_bounds=True))
        both(f"window_summary edges, {window_of}", lambda r, w=window_of: r.window_summary(edges=[2.0, 7.5, 7.75, 19.0], by=some, window_of=w, row_bounds=True))
        both(f"window_summary 0.25 s by none, {window_of}", lambda r, w=window_of: r.window_summary(0.25, window_of=w))
        both(f"quantile_summary 5 s, {window_of}", lambda r, w=window_of: r.quantile_summary(LEVELS, thresholds=SLO_THR, window_s=5.0, by=grid, window_of=w))
        both(f"window_bands, {window_of}", lambda r, w=window_of: r.window_bands(5.0, by=grid, window_of=w))
        both(f"quantile_bands, {window_of}", lambda r, w=window_of: r.quantile_bands(LEVELS, thresholds=SLO_THR, window_s=5.0, by=some, window_of=w))
    both("quantile_summary, the whole run by grid", lambda r: r.quantile_summary(LEVELS, thresholds=SLO_THR, by=grid))
    both("quantile_summary, the whole run in one group", lambda r: r.quantile_summary(LEVELS, thresholds=SLO_THR))
    both("quantile_summary by scenario", lambda r: r.quantile_summary(LEVELS, thresholds=SLO_THR, window_s=5.0, by="scenario"))
    both("window_summary by scenario", lambda r: r.window_summary(5.0, by="scenario", row_bounds=True))
    both("quantile_bands, the whole run", lambda r: r.quantile_bands(LEVELS, thresholds=SLO_THR, by=grid))
    _same(two.aggregate(by=grid), one.aggregate(by=grid), "aggregate by grid")
    sizes = np.concatenate(totals)
    assert ((sizes > 0) & (sizes <= TINY_MAX)).any() and ((sizes > TINY_MAX) & (sizes <= SMALL_MAX)).any() and (sizes > SMALL_MAX).any(), \
        "the cases do not give every reduction tier a merged cell"
    # the three dumps, read back
    for name, call in (("point", lambda r, p: r.save_point_summary(p, grid)),
                       ("window", lambda r, p: r.save_window_summary(p, grid, window_s=5.0, window_of="arrival")),
                       ("quantile", lambda r, p: r.save_quantile_summary(p, grid, levels=LEVELS, thresholds=SLO_THR, window_s=5.0))):
        call(one, str(tmp_path / f"{name}_one.npz"))
        call(two, str(tmp_path / f"{name}_two.npz"))
        want, got = R.load_summary(str(tmp_path / f"{name}_one.npz")), R.load_summary(str(tmp_path / f"{name}_two.npz"))
        assert set(got) == set(want) and len(want) > 3
        for k, v in want.items():
            assert got[k].dtype == v.dtype and got[k].shape == v.shape, (name, k)
            assert got[k].tobytes() == v.tobytes(), (name, k)


def test_ragged_shards_on_three_devices():
    from asyncflow_amd.runner import SimulationRunner

    payload = lb_two_servers(horizon=20)
    seeds = np.arange(7, dtype=np.uint64) + 900
    sweep = {USERS: np.array([300.0, 60.0, 90.0, 500.0, 120.0, 60.0, 200.0])}
    one = SimulationRunner(simulation_input=payload, seeds=seeds, sweep=sweep).run()
    three = SimulationRunner(simulation_input=payload, seeds=seeds, sweep=sweep, devices=[0, 0, 0]).run()
    assert len(three.shards) == 3 and len({len(ix) for ix in three.index}) > 1
    ids = np.array([0, 1, 0, 1, -1, 0, 1])
    for window_of in ("finish", "arrival"):
        _same(three.window_summary(2.0, by=ids, window_of=window_of, row_bounds=True), one.window_summary(2.0, by=ids, window_of=window_of, row_bounds=True), window_of)
        _same(three.quantile_summary(LEVELS, thresholds=SLO_THR, window_s=4.0, by=ids, window_of=window_of),
              one.quantile_summary(LEVELS, thresholds=SLO_THR, window_s=4.0, by=ids, window_of=window_of), window_of)
    _same(three.pooled_summary(ids), one.pooled_summary(ids), "pooled")
    _same(three.quantile_summary(LEVELS, by=USERS), one.quantile_summary(LEVELS, by=R.groups_of_columns([sweep[USERS]])[0]), "by a named column")


# ---- through the C ABI on fabricated clock buffers -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan():
    from oracle.scenarios import lb_two_servers as oracle_lb2

    return lower(oracle_lb2(horizon=20))


class Shard:
    """One device's outputs, hand-made: rows[s] [m_s, 2]; the clock buffer's unused rows hold NaN, and `over` scenarios claim more
    completions than the buffer has rows."""

    def __init__(self, rows: list[np.ndarray], cap: int, over: tuple[int, ...] = ()) -> None:
        import torch

        self.rows, self.n, self.cap = rows, len(rows), cap
        clock = np.full((self.n, cap, 2), np.nan)
        counts = np.zeros((self.n, _abi.CNT_SLOTS), dtype=np.uint32)
        for s, r in enumerate(rows):
            assert r.shape[0] <= cap
            clock[s, :r.shape[0]] = r
            counts[s, _abi.CNT_COMPLETED] = r.shape[0] + (5 if s in over and r.shape[0] == cap else 0)
        self.dev = torch.device("cuda", 0)
        self.clock_t = torch.as_tensor(clock, device=self.dev)
        self.counts_t = torch.as_tensor(counts.view(np.int32), device=self.dev)

    def outputs(self) -> _abi.AfOutputs:
        return _abi.AfOutputs(self.cap, C.c_void_p(self.clock_t.data_ptr()), 0, None, C.c_void_p(self.counts_t.data_ptr()))


def _guarded(sizes: dict[str, int]):
    """One int32 buffer of sentinel words with room for every output (sizes in words) between guards: the buffer, the outputs'
    word offsets."""
    import torch

    off, at = {}, GUARD
    for k, sz in sizes.items():
        off[k] = at
        at += ((sz + 3) & ~3) + GUARD
    return torch.full((at,), SENTINEL, dtype=torch.int32, device=torch.device("cuda", 0)), off


def _read(buf, off: dict[str, int], sizes: dict[str, int], written: bool) -> tuple[dict[str, np.ndarray], bool]:
    """The outputs' words and whether every other word (written=False: every word) still holds the sentinel."""
    import torch

    torch.cuda.synchronize()
    host = buf.cpu().numpy().view(np.uint32)
    inside = np.zeros(host.shape[0], dtype=bool)
    out = {}
    for k, o in off.items():
        inside[o:o + sizes[k]] = written
        out[k] = host[o:o + sizes[k]].copy()
    return out, bool((host[~inside] == SENTINEL).all())


def _export(eng, lib, sh: Shard, ids: np.ndarray, edges, by: str, capacity: int | None = None):
    """af_engine_export_cells of one shard (ids: this shard's; negative = skipped) into guarded buffers of exactly the capacity that
    always suffices (or of `capacity` elements).  Returns the return code, the exported latencies, the bounds, and whether nothing else changed."""
    import torch

    n_win = 0 if edges is None else len(edges) - 1
    capacity = sum(r.shape[0] for r in sh.rows) if capacity is None else capacity
    sizes = {"lat": 2 * capacity, "bounds": sh.n * (max(n_win, 1) + 1)}
    buf, off = _guarded(sizes)
    grp = torch.as_tensor(np.where(ids < 0, _abi.POOL_SKIP, 0).astype(np.uint32).view(np.int32), device=sh.dev)
    e = None if edges is None else np.ascontiguousarray(edges, dtype=np.float64)
    out = sh.outputs()
    req = _abi.AfCellsExport(sh.n, n_win, int(by == "arrival"), C.c_void_p(grp.data_ptr()), None if e is None else e.ctypes.data_as(C.POINTER(C.c_double)),
                             C.c_void_p(buf.data_ptr() + 4 * off["lat"]), capacity, C.c_void_p(buf.data_ptr() + 4 * off["bounds"]), 0, 0.0, 0)
    rc = lib.af_engine_export_cells(eng._h, C.byref(out), C.byref(req))  # noqa: SLF001
    if rc != _abi.AF_OK:
        return rc, None, None, _read(buf, off, sizes, False)[1]
    used = {"lat": 2 * int(req.lat_count), "bounds": sizes["bounds"]}
    got, clean = _read(buf, off, used, True)
    return rc, got["lat"].view(np.float64), got["bounds"].reshape(sh.n, -1), clean


def _cell_sizes(G: int, wc: int) -> dict[str, int]:
    C_ = G * wc
    return {"stats": 2 * 8 * C_, "count": C_, "quantiles": 2 * C_ * len(LEVELS), "within": C_ * len(SLO_THR)}


def _decode(got: dict[str, np.ndarray], G: int, wc: int) -> dict[str, np.ndarray]:
    return {"stats": got["stats"].view(np.uint64).reshape(G, wc, 8), "count": got["count"].reshape(G, wc),
            "quantiles": got["quantiles"].view(np.uint64).reshape(G, wc, len(LEVELS)), "within": got["within"].reshape(G, wc, len(SLO_THR))}


def _summarize_cells(eng, lib, lat: np.ndarray, bounds: np.ndarray, begin: np.ndarray, group: np.ndarray, G: int, n_win: int, n_lat: int | None = None):
    """af_engine_import_cells with every output.  Returns the return code, the outputs as words, and whether nothing else changed
    (a refused call: whether NO word changed)."""
    import torch

    wc = max(n_win, 1)
    sizes = _cell_sizes(G, wc)
    buf, off = _guarded(sizes)
    lat_t = torch.as_tensor(np.concatenate([lat, np.zeros(1)]), device=torch.device("cuda", 0))   # (never empty: a pointer to give)
    q, th = np.asarray(LEVELS, dtype=np.float64), np.asarray(SLO_THR, dtype=np.float64)
    pd, pu32 = C.POINTER(C.c_double), C.POINTER(C.c_uint32)
    b = np.ascontiguousarray(bounds, dtype=np.uint32)
    bg = np.ascontiguousarray(begin, dtype=np.uint64)
    g = np.ascontiguousarray(group, dtype=np.uint32)
    ptr = {k: C.c_void_p(buf.data_ptr() + 4 * o) for k, o in off.items()}
    req = _abi.AfCells(b.shape[0], G, n_win, g.ctypes.data_as(pu32), b.ctypes.data_as(pu32), bg.ctypes.data_as(C.POINTER(C.c_uint64)),
                       C.c_void_p(lat_t.data_ptr()), lat.shape[0] if n_lat is None else n_lat, ptr["stats"], len(LEVELS), q.ctypes.data_as(pd),
                       len(SLO_THR), th.ctypes.data_as(pd), ptr["count"], ptr["quantiles"], ptr["within"], 0.0, 0)
    rc = lib.af_engine_import_cells(eng._h, C.byref(req))  # noqa: SLF001
    got, clean = _read(buf, off, sizes, rc == _abi.AF_OK)
    return rc, (_decode(got, G, wc) if rc == _abi.AF_OK else None), clean, int(req.scratch_bytes)


def _one_device(eng, shards: list[Shard], index: list[np.ndarray], ids: np.ndarray, G: int, edges, by: str) -> dict[str, np.ndarray]:
    """The one-device entry points (af_engine_summarize_windows / _quantiles, or their by-arrival forms) on the shards' clock
    buffers concatenated in member order."""
    import torch

    n, cap = len(ids), shards[0].cap
    dev = shards[0].dev
    clock = torch.empty((n, cap, 2), dtype=torch.float64, device=dev)
    counts = torch.empty((n, _abi.CNT_SLOTS), dtype=torch.int32, device=dev)
    for sh, ix in zip(shards, index):
        where = torch.as_tensor(np.asarray(ix), device=dev)
        clock[where] = sh.clock_t
        counts[where] = sh.counts_t
    grp = torch.as_tensor(np.where(ids < 0, _abi.POOL_SKIP, ids).astype(np.uint32).view(np.int32), device=dev)
    wc = 1 if edges is None else len(edges) - 1
    sizes = _cell_sizes(G, wc)
    buf, off = _guarded(sizes)
    ptr = {k: buf.data_ptr() + 4 * o for k, o in off.items()}
    kw = {"clock_ptr": clock.data_ptr(), "clock_capacity": cap, "counts_ptr": counts.data_ptr(), "group_ptr": grp.data_ptr()}
    torch.cuda.synchronize()
    if edges is None:
        eng.summarize_pooled(n, G, stats_ptr=ptr["stats"], **kw)
    else:
        eng.summarize_windows(n, G, edges, stats_ptr=ptr["stats"], window_of=by, **kw)
    eng.summarize_quantiles(n, G, LEVELS, edges=edges, thresholds=SLO_THR, count_ptr=ptr["count"], quantiles_ptr=ptr["quantiles"], within_ptr=ptr["within"],
                            window_of=by, **kw)
    got, clean = _read(buf, off, sizes, True)
    assert clean
    return _decode(got, G, wc)


def _numpy(cells: list[np.ndarray], G: int, wc: int) -> dict[str, np.ndarray]:
    return {"stats": np.stack([R.latency_stats_row(np.ascontiguousarray(x)) for x in cells]).view(np.uint64).reshape(G, wc, 8),
            "count": np.array([x.shape[0] for x in cells], dtype=np.uint32).reshape(G, wc),
            "quantiles": np.stack([R.latency_quantiles(x, LEVELS) for x in cells]).view(np.uint64).reshape(G, wc, len(LEVELS)),
            "within": np.stack([R.latency_within(x, SLO_THR) for x in cells]).astype(np.uint32).reshape(G, wc, len(SLO_THR))}


def _equal(got: dict[str, np.ndarray], want: dict[str, np.ndarray], what: str, nan_payload_free: bool = False) -> None:
    """Every output word (the floats as their u64 patterns).  nan_payload_free, for the comparison with numpy alone: a NaN of the
    reference stands for any NaN in the same place -- numpy does not promise the payload the device writes for an empty cell."""
    for k, w in want.items():
        g = got[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        if nan_payload_free and k in ("stats", "quantiles"):
            nan = np.isnan(w.view(np.float64))
            assert np.array_equal(np.isnan(g.view(np.float64)), nan), (what, k, "NaN in other places")
            g, w = g[~nan], w[~nan]
        assert np.array_equal(g, w), (what, k, int((g != w).sum()))


def _rows(rng: np.random.Generator, m: int, horizon: float, on_edges: bool) -> np.ndarray:
    """m rows in completion order with unsorted starts; on_edges: finishes and starts on quarter seconds, so that many lie
    exactly on a window edge."""
    finish = np.sort(rng.random(m) * horizon)
    lat = rng.random(m) * 0.06
    if on_edges:
        finish = np.round(finish * 4.0) / 4.0
        lat = rng.integers(0, 5, m) * 0.25 * (rng.random(m) < 0.5) + lat * (rng.random(m) < 0.5)
    return np.stack([finish - lat, finish], axis=1)


def _check(plan, rows: list[np.ndarray], deal: np.ndarray, ids: np.ndarray, G: int, edges, by: str, cap: int, over: tuple[int, ...] = ()) -> dict[str, np.ndarray]:
    """Export every shard, import, and compare every word with the one-device call and with numpy on the host definition."""
    from asyncflow_amd.engine import Engine, load_library

    lib = load_library()
    index = [np.nonzero(deal == k)[0] for k in range(int(deal.max()) + 1)]
    shards = [Shard([rows[s] for s in ix], cap, tuple(j for j, s in enumerate(ix) if s in over)) for ix in index]
    n_win = 0 if edges is None else len(edges) - 1
    eng = Engine(plan, 0)
    try:
        parts = []
        for sh, ix in zip(shards, index):
            rc, lat, bounds, clean = _export(eng, lib, sh, ids[ix], edges, by)
            assert rc == _abi.AF_OK and clean, (lib.af_last_error(), clean)
            parts.append((lat, bounds))
        bounds, begin, n_lat = R.sweep_order_segments([p[1] for p in parts], index, ids)
        lat = np.concatenate([p[0] for p in parts])
        assert lat.shape[0] == n_lat
        group = np.where(ids < 0, _abi.POOL_SKIP, ids).astype(np.uint32)
        rc, got, clean, _ = _summarize_cells(eng, lib, lat, bounds, begin, group, G, n_win)
        assert rc == _abi.AF_OK and clean, (lib.af_last_error(), clean)
        want = _one_device(eng, shards, index, ids, G, edges, by)
    finally:
        eng.close()
    what = f"{len(index)} shards, {n_win} windows by {by}"
    _equal(got, want, what + ": against the one-device call")
    _equal(got, _numpy(R.merge_cell_segments(parts, index, ids, G, n_win), G, max(n_win, 1)), what + ": against numpy", nan_payload_free=True)
    return got


@pytest.mark.parametrize("n_shards", [2, 3])
def test_fabricated_shards_through_the_c_abi(plan, n_shards):
    rng = np.random.default_rng(40 + n_shards)
    n, G, cap = 13, 4, 700                                                           # (group 3 has no member: empty cells)
    sizes = [0, 17, 700, 33, 1, 258, 64, 129, 511, 700, 2, 95, 400]
    rows = [_rows(rng, m, 6.0, on_edges=s % 2 == 0) for s, m in enumerate(sizes)]
    rows[3] = np.stack([np.full(33, 8.0) - 0.01, np.full(33, 8.0)], axis=1)          # every row outside the windows below
    ids = rng.integers(0, G - 1, n)
    ids[[5, 8]] = -1                                                                 # skipped, with rows
    deal = np.arange(n) % n_shards                                                   # interleaved
    edges = [0.5, 1.0, 1.25, 3.0, 5.5]
    for by in ("finish", "arrival"):
        got = _check(plan, rows, deal, ids, G, edges, by, cap, over=(2, 9))
        assert got["count"].sum() > 0 and (got["count"] == 0).any()
    _check(plan, rows, deal, ids, G, None, "finish", cap, over=(2, 9))               # the whole run: a segmented copy
    # segments of odd length at odd offsets: the 16-byte loads see a misaligned head and an odd tail
    lengths = [p.shape[0] for p in rows]
    assert any(m % 2 for m in lengths) and any(sum(lengths[:k]) % 2 for k in range(1, n))


def test_more_windows_than_the_lds_form_holds(plan):
    rng = np.random.default_rng(77)
    rows = [_rows(rng, m, 10.0, on_edges=False) for m in (3000, 2999, 0, 1777)]
    edges = np.linspace(0.25, 9.75, 4098)                                            # 4 097 windows
    for by in ("finish", "arrival"):
        got = _check(plan, rows, np.array([0, 1, 1, 0]), np.array([1, 0, 1, 0]), 2, edges, by, 3000)
        assert got["count"].shape == (2, 4097) and got["count"].sum() > 7000


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_every_output_word_alone(plan):
    from asyncflow_amd.engine import Engine, load_library

    lib = load_library()
    rng = np.random.default_rng(5)
    rows = [_rows(rng, m, 6.0, on_edges=True) for m in (40, 0, 77, 12)]
    sh = Shard(rows, 80)
    ids = np.array([0, 1, 1, 0])
    edges = [0.0, 2.0, 6.0]
    eng = Engine(plan, 0)
    try:
        rc, lat, bounds, clean = _export(eng, lib, sh, ids, edges, "finish")
        assert rc == _abi.AF_OK and clean
        length = bounds[:, -1].astype(np.int64) - bounds[:, 0]
        assert length[0] > 1 and length[2] > 1 and lat.shape[0] == length.sum()
        for kw in ({"edges": edges, "by": "finish"}, {"edges": edges, "by": "arrival"}, {"edges": None, "by": "finish"}):
            rc, needed, _, clean = _export(eng, lib, sh, ids, **kw)
            assert rc == _abi.AF_OK and clean and needed.shape[0] > 0
            rc, _, _, clean = _export(eng, lib, sh, ids, capacity=needed.shape[0], **kw)         # exactly what is needed
            assert rc == _abi.AF_OK and clean
            rc, _, _, clean = _export(eng, lib, sh, ids, capacity=needed.shape[0] - 1, **kw)     # ... and one element short
            assert rc == _abi.AF_ERR_CAPACITY and clean and b"lat_capacity" in lib.af_last_error(), kw
        seg_bounds, begin, n_lat = R.sweep_order_segments([bounds], [np.arange(4)], ids)
        group = ids.astype(np.uint32)
        ok = _summarize_cells(eng, lib, lat, seg_bounds, begin, group, 2, 2)
        assert ok[0] == _abi.AF_OK and ok[2]
        rc, _, clean, _ = _summarize_cells(eng, lib, lat, seg_bounds, begin, group, 2, 2, n_lat=n_lat - 1)      # a segment past n_lat
        assert rc == _abi.AF_ERR_INVALID and clean and b"n_lat" in lib.af_last_error()
        overlap = begin.copy()
        overlap[2] = begin[0] + np.uint64(length[0] - 1)                             # its first element is scenario 0's last
        rc, _, clean, _ = _summarize_cells(eng, lib, lat, seg_bounds, overlap, group, 2, 2)
        assert rc == _abi.AF_ERR_INVALID and clean and b"overlap" in lib.af_last_error()
        bad = group.copy()
        bad[3] = 2                                                                   # a group id out of range
        rc, _, clean, _ = _summarize_cells(eng, lib, lat, seg_bounds, begin, bad, 2, 2)
        assert rc == _abi.AF_ERR_INVALID and clean and b"group id out of range" in lib.af_last_error()
        again = _summarize_cells(eng, lib, lat, seg_bounds, begin, group, 2, 2)      # ... and the engine is as good as before
        _equal(again[1], ok[1], "after the refusals")
    finally:
        eng.close()


# ---- whatever the scratch held before --------------------------------------------------------------------------------------------------
def test_both_entry_points_whatever_the_scratch_held(plan):
    from asyncflow_amd.engine import Engine, load_library

    lib = load_library()
    rng = np.random.default_rng(6)
    rows = [_rows(rng, m, 6.0, on_edges=True) for m in (300, 0, 6000, 700, 5000, 513)]   # cells of every tier
    sh = Shard(rows, 6000)
    ids = np.array([0, 1, 1, 0, 1, -1])
    group = np.where(ids < 0, _abi.POOL_SKIP, ids).astype(np.uint32)

    def run(eng, edges, by):
        rc, lat, bounds, clean = _export(eng, lib, sh, ids, edges, by)
        assert rc == _abi.AF_OK and clean
        seg_bounds, begin, _ = R.sweep_order_segments([bounds], [np.arange(len(ids))], ids)
        rc, got, clean, scratch = _summarize_cells(eng, lib, lat, seg_bounds, begin, group, 2, 0 if edges is None else len(edges) - 1)
        assert rc == _abi.AF_OK and clean
        return {"lat": lat.view(np.uint64), "bounds": bounds, **got}, scratch

    for edges, by in (([0.0, 0.5, 6.0], "finish"), ([0.0, 0.5, 6.0], "arrival"), (None, "finish")):
        eng = Engine(plan, 0)
        try:
            fresh, S = run(eng, edges, by)
        finally:
            eng.close()
        assert S > 0 and fresh["count"].max() > SMALL_MAX and ((fresh["count"] > TINY_MAX) & (fresh["count"] <= SMALL_MAX)).any()
        for size in (2 * S + 4096, 256):                             # a roomy pool full of 0xFFFFFFFF, and one too small for either call
            eng = Engine(plan, 0)
            try:
                eng.probe_scratch(size, 0xFFFFFFFF)
                got, _ = run(eng, edges, by)
            finally:
                eng.close()
            for k, w in fresh.items():
                assert np.array_equal(got[k], w), (by, size, k)
