"""Pooled analyzer, CPU side: the C entry point and its struct, argument checks, group resolution, Sweep.point_columns."""

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
from asyncflow_amd.plan import lower
from asyncflow_amd.results import resolve_groups
from asyncflow_amd.sweep import expand_grid
from oracle.scenarios import lb_two_servers

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def lib():
    af_build.build()
    from asyncflow_amd.engine import load_library

    return load_library()


def test_header_declares_and_library_exports_the_pooled_entry(lib):
    header = (ROOT / "include" / "asyncflow_hip.h").read_text()
    assert re.search(r"int\s+af_engine_summarize_pooled\s*\(\s*af_engine_t\s*\*", header)
    assert "af_engine_summarize_pooled" in _abi.EXPORTED_SYMBOLS
    assert hasattr(lib, "af_engine_summarize_pooled")
    assert lib.af_engine_summarize_pooled.argtypes[2] is C.POINTER(_abi.AfPooled)


def test_af_pooled_layout_matches_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "a host C compiler is needed for the layout probe"
    src = tmp_path / "probe.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "asyncflow_hip.h"\n'
        'int main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(af_pooled_t), offsetof(af_pooled_t, n_scenarios), '
        "offsetof(af_pooled_t, n_groups), offsetof(af_pooled_t, group), offsetof(af_pooled_t, stats), "
        "offsetof(af_pooled_t, elapsed_ms)); return 0; }\n")
    exe = tmp_path / "probe"
    subprocess.run([cc, "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    P = _abi.AfPooled
    want = [C.sizeof(P), P.n_scenarios.offset, P.n_groups.offset, P.group.offset, P.stats.offset, P.elapsed_ms.offset]
    assert got == want


def test_pooled_entry_refuses_bad_requests_without_a_device(lib):
    from asyncflow_amd.engine import PLAN_ONLY, Engine, EngineUnavailableError

    eng = Engine(lower(lb_two_servers(horizon=20)), PLAN_ONLY)
    try:
        out = _abi.AfOutputs(4, None, 0, None, None)
        req = _abi.AfPooled(4, 1, None, None, 0.0)
        assert lib.af_engine_summarize_pooled(None, C.byref(out), C.byref(req)) == _abi.AF_ERR_INVALID
        assert lib.af_engine_summarize_pooled(eng._h, C.byref(out), None) == _abi.AF_ERR_INVALID  # noqa: SLF001
        assert lib.af_engine_summarize_pooled(eng._h, C.byref(out), C.byref(req)) == _abi.AF_ERR_NO_DEVICE  # noqa: SLF001
        assert b"planning-only" in lib.af_last_error()
        with pytest.raises(EngineUnavailableError, match="planning-only"):
            eng.summarize_pooled(4, 1, clock_ptr=0, clock_capacity=4, counts_ptr=0, stats_ptr=0)
    finally:
        eng.close()


def test_group_resolution():
    ids, g = resolve_groups(None, 5)
    assert g == 1 and ids.tolist() == [0] * 5
    ids, g = resolve_groups(np.array([3, -1, 0, 3], dtype=np.int32), 4)
    assert g == 4 and ids.dtype == np.int64 and ids.tolist() == [3, -1, 0, 3]
    grid = expand_grid({"a": [1.0, 2.0, 3.0], "b": [10.0, 20.0]}, replicas=2)
    ids, g = resolve_groups(grid, len(grid))
    assert g == 6 and np.array_equal(ids, grid.point)
    with pytest.raises(ValueError, match="one id per scenario"):
        resolve_groups(np.zeros(3, dtype=np.int64), 4)
    with pytest.raises(ValueError, match="one id per scenario"):
        resolve_groups(np.zeros((2, 2), dtype=np.int64), 4)
    with pytest.raises(TypeError, match="integers"):
        resolve_groups(np.zeros(4), 4)
    with pytest.raises(TypeError, match="integers"):
        resolve_groups(np.ones(4, dtype=bool), 4)
    with pytest.raises(ValueError, match="no scenario"):
        resolve_groups(-np.ones(4, dtype=np.int64), 4)


def test_sweep_point_columns_are_row_major():
    grid = expand_grid({"users": [10.0, 20.0, 30.0], "rtt": [0.001, 0.002]}, replicas=3, order_by_load="users")
    cols = grid.point_columns()
    assert list(cols) == ["users", "rtt"]
    assert cols["users"].tolist() == [10.0, 10.0, 20.0, 20.0, 30.0, 30.0]
    assert cols["rtt"].tolist() == [0.001, 0.002] * 3
    # every scenario's columns are those of its point, scenarios sorted or not
    for k, v in cols.items():
        assert np.array_equal(v[grid.point], grid.columns[k])
