"""Cells across devices, CPU side: the host definition `results.merge_cell_segments` against direct numpy masking of every
scenario's rows, the reordering of the shards' bounds and segment places into sweep order, the two new structs against the
header, and what a ShardedResults still refuses."""

from __future__ import annotations

import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from asyncflow_amd import _abi
from asyncflow_amd import build as af_build
from asyncflow_amd.results import BatchedResults, ShardedCellResults, ShardedResults, _window_latencies, check_edges, merge_cell_segments, sweep_order_segments

ROOT = Path(__file__).resolve().parent.parent


def _rows(rng: np.random.Generator, m: int, horizon: float) -> np.ndarray:
    """m clock rows in completion order: finish non-decreasing, start unsorted, some values exactly on quarter seconds."""
    finish = np.sort(np.round(rng.random(m) * horizon * 4.0) / 4.0 if m % 2 else rng.random(m) * horizon)
    return np.stack([finish - rng.random(m) * 3.0, finish], axis=1)


def _export(rows: list[np.ndarray], edges: np.ndarray | None, window_of: str, ids: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """What af_engine_export_cells writes for these scenarios, stated with numpy: the bounds (np.searchsorted on the sorted
    column), and the latencies inside the windows, window after window, a window's in row order; nothing for a negative id."""
    lat, bounds = [], []
    for ck, g in zip(rows, ids):
        if edges is None:
            bounds.append([0, ck.shape[0]])
            per = [ck[:, 1] - ck[:, 0]]
        else:
            t = ck[:, 1] if window_of == "finish" else np.sort(ck[:, 0])
            bounds.append(np.searchsorted(t, edges, side="right"))
            per = _window_latencies(ck, edges, window_of)
        if g >= 0:
            lat.extend(per)
    return np.concatenate(lat + [np.zeros(0)]), np.asarray(bounds, dtype=np.uint32)


@pytest.mark.parametrize("window_of", ["finish", "arrival"])
@pytest.mark.parametrize("shards", [2, 3])
def test_merge_equals_masking_every_scenarios_rows(window_of, shards):
    rng = np.random.default_rng(shards * 10 + len(window_of))
    n, G, horizon = 17, 3, 20.0
    rows = [_rows(rng, int(m), horizon) for m in rng.integers(0, 60, n)]
    rows[4] = np.zeros((0, 2))                                       # a scenario without rows
    rows[9] = np.stack([np.full(5, 30.0), np.full(5, 31.0)], axis=1)    # ... and one whose rows all lie outside the windows
    ids = rng.integers(0, G, n)
    ids[[2, 11]] = -1
    deal = rng.integers(0, shards, n)
    deal[:shards] = np.arange(shards)                                # (no shard is empty)
    index = [np.nonzero(deal == k)[0] for k in range(shards)]        # interleaved
    for edges in (None, check_edges([2.0, 7.5, 7.75, 19.0]), check_edges(np.arange(0.0, 20.25, 0.25))):
        if edges is None and window_of == "arrival":
            continue
        parts = [_export([rows[s] for s in ix], edges, window_of, ids[ix]) for ix in index]
        W = 0 if edges is None else edges.shape[0] - 1
        cells = merge_cell_segments(parts, index, ids, G, W)
        assert len(cells) == G * max(W, 1)
        for g in range(G):
            members = np.nonzero(ids == g)[0]
            for w in range(max(W, 1)):
                want = []
                for s in members:                                    # ascending scenario index, then row order
                    ck = rows[s]
                    t = ck[:, 1] if window_of == "finish" else ck[:, 0]
                    mask = np.ones(ck.shape[0], dtype=bool) if edges is None else (t > edges[w]) & (t <= edges[w + 1])
                    want.append((ck[:, 1] - ck[:, 0])[mask])
                want = np.concatenate(want + [np.zeros(0)])
                assert np.array_equal(cells[g * max(W, 1) + w].view(np.uint64), want.view(np.uint64)), (g, w)


def test_bounds_and_begins_go_to_sweep_order():
    ids = np.array([0, -1, 1, 0, 1, 0])
    index = [np.array([4, 0, 3]), np.array([5, 1, 2])]               # each shard's scenarios in ITS order
    bounds = [np.array([[1, 3, 4], [0, 0, 2], [5, 5, 5]], dtype=np.uint32), np.array([[2, 2, 7], [0, 9, 9], [3, 4, 4]], dtype=np.uint32)]
    b, begin, total = sweep_order_segments(bounds, index, ids)
    assert b.dtype == np.uint32 and begin.dtype == np.uint64
    assert b.tolist() == [[0, 0, 2], [0, 9, 9], [3, 4, 4], [5, 5, 5], [1, 3, 4], [2, 2, 7]]
    # shard 0 exports 3 + 2 + 0 latencies for its scenarios 4, 0, 3; shard 1 then 5, none for the skipped scenario 1, and 1
    assert begin.tolist() == [3, 10, 10, 5, 0, 5] and total == 11
    with pytest.raises(ValueError, match="latencies"):
        merge_cell_segments([(np.zeros(4), bounds[0]), (np.zeros(6), bounds[1])], index, ids, 2, 2)


def test_structs_have_the_headers_field_order(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "a host C compiler is needed for the layout probe"
    want = {"af_cells_export_t": (_abi.AfCellsExport, ["n_scenarios", "n_windows", "by_arrival", "group", "edges", "lat", "lat_capacity", "seg_bounds",
                                                        "lat_count", "elapsed_ms", "scratch_bytes"]),
            "af_cells_t": (_abi.AfCells, ["n_scenarios", "n_groups", "n_windows", "group", "seg_bounds", "seg_begin", "lat", "n_lat", "stats", "n_levels",
                                          "levels", "n_thresholds", "thresholds", "count", "quantiles", "within", "elapsed_ms", "scratch_bytes"])}
    body = ""
    for name, (struct, fields) in want.items():
        assert [f for f, _ in struct._fields_] == fields  # noqa: SLF001
        body += f'printf("%zu", sizeof({name}));\n' + "".join(f'printf(" %zu", offsetof({name}, {f}));\n' for f in fields) + 'printf("\\n");\n'
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "asyncflow_hip.h"\nint main(void) {\n' + body + "return 0; }\n")
    exe = tmp_path / "probe"
    subprocess.run([cc, "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    for line, (struct, fields) in zip(lines, want.values()):
        assert [int(x) for x in line.split()] == [C.sizeof(struct), *(getattr(struct, f).offset for f in fields)]


def test_the_abi_is_still_seven_and_names_the_new_entries():
    header = (ROOT / "include" / "asyncflow_hip.h").read_text()
    assert re.search(r"#define\s+AF_ABI_VERSION\s+7\b", header) and _abi.AF_ABI_VERSION == 7
    for name, arg in (("af_engine_export_cells", r"const\s+af_outputs_t\s*\*\s*\w+\s*,\s*af_cells_export_t\s*\*"), ("af_engine_import_cells", r"af_cells_t\s*\*")):
        assert re.search(rf"int\s+{name}\s*\(\s*af_engine_t\s*\*\s*\w+\s*,\s*{arg}", header), name
        assert name in _abi.EXPORTED_SYMBOLS
    af_build.build()
    from asyncflow_amd.engine import load_library

    lib = load_library()
    assert lib.af_abi_version() == 7
    assert lib.af_engine_export_cells.argtypes[2] is C.POINTER(_abi.AfCellsExport) and lib.af_engine_import_cells.argtypes[1] is C.POINTER(_abi.AfCells)
    from asyncflow_amd import jit

    assert "af_cells.hpp" in af_build.SOURCES and "af_cells.hpp" in jit._SOURCES  # noqa: SLF001


def test_entries_refuse_bad_requests_without_a_device():
    from asyncflow_amd.engine import PLAN_ONLY, Engine, load_library
    from asyncflow_amd.plan import lower
    from oracle.scenarios import lb_two_servers

    lib = load_library()
    eng = Engine(lower(lb_two_servers(horizon=20)), PLAN_ONLY)
    try:
        out = _abi.AfOutputs(4, None, 0, None, None)
        ex = _abi.AfCellsExport(4, 0, 0, None, None, None, 0, None, 0, 0.0, 0)
        assert lib.af_engine_export_cells(None, C.byref(out), C.byref(ex)) == _abi.AF_ERR_INVALID
        assert lib.af_engine_export_cells(eng._h, C.byref(out), None) == _abi.AF_ERR_INVALID  # noqa: SLF001
        assert lib.af_engine_export_cells(eng._h, C.byref(out), C.byref(ex)) == _abi.AF_ERR_NO_DEVICE  # noqa: SLF001
        cr = _abi.AfCells()
        assert lib.af_engine_import_cells(None, C.byref(cr)) == _abi.AF_ERR_INVALID
        assert lib.af_engine_import_cells(eng._h, C.byref(cr)) == _abi.AF_ERR_NO_DEVICE  # noqa: SLF001
    finally:
        eng.close()


def test_the_exact_analyzers_are_shared_and_the_rest_still_refuses():
    assert issubclass(ShardedCellResults, ShardedResults)
    sh = ShardedCellResults.__new__(ShardedCellResults)
    for name in ("aggregate", "save_point_summary", "window_bands", "save_window_summary", "quantile_bands", "save_quantile_summary"):
        assert getattr(ShardedCellResults, name) is getattr(BatchedResults, name), name  # one body, not a copy
    for name in ("pooled_summary", "window_summary", "quantile_summary"):
        assert "several devices" in getattr(ShardedCellResults, name).__doc__
    plain = ShardedResults.__new__(ShardedResults)                   # shards put behind an index by hand: as before
    for name in ("pooled_summary", "window_summary", "window_bands", "quantile_summary", "quantile_bands", "save_window_summary"):
        with pytest.raises(NotImplementedError, match="several devices"):
            getattr(plain, name)(None)
    with pytest.raises(NotImplementedError, match="several devices"):
        plain.save_point_summary("points.npz", None)
    refused = ("state_summary", "state_quantile_summary", "save_state_summary", "paired_summary", "paired_bands", "save_paired_summary",
               "exemplar_summary", "save_exemplar_summary", "arrival_summary", "arrival_bands", "save_arrival_summary", "in_flight_summary",
               "in_flight_bands", "save_in_flight_summary", "littles_law", "series_window_summary", "series_quantile_summary",
               "series_excursion_summary", "series_histogram_summary", "series_combined_summary", "series_joint_summary", "series_warmup_summary")
    for name in refused:
        with pytest.raises(NotImplementedError, match="several devices"):
            getattr(sh, name)()
