"""ctypes binding of the HIP engine (include/asyncflow_hip.h).

There is NO CPU fallback: if the shared library is missing or no MI355X is
visible, :class:`EngineUnavailableError` is raised.
"""

from __future__ import annotations

import ctypes as C
import math
import os
from pathlib import Path
from typing import Any, Sequence

import numpy as np

from . import _abi
from . import build as af_build
from .build import LIB_PATH
from .plan import DevicePlan


class EngineUnavailableError(RuntimeError):
    """The HIP library or the GPU is missing (the engine never falls back to the CPU)."""


class EngineError(RuntimeError):
    """A C-ABI call failed; the message is ``af_last_error()``."""


_lib: C.CDLL | None = None


def _load_hip_runtime() -> None:
    """Make ONE HIP runtime globally visible before dlopen()ing the engine.

    libasyncflow_hip.so is linked with --no-hip-rt: its hip* symbols bind to the
    runtime already in the process.  Under PyTorch that must be the copy torch
    bundles (torch/lib/libamdhip64.so), otherwise torch tensors and the engine
    would live in two different HIP/HSA runtimes.  Without torch, the system ROCm
    runtime is used; a C/C++ host links its own.
    """
    candidates: list[str] = []
    try:
        import torch

        candidates.append(str(Path(torch.__file__).resolve().parent / "lib" / "libamdhip64.so"))
    except Exception:  # noqa: BLE001 - torch is plumbing, not a requirement of the C ABI
        pass
    candidates += ["libamdhip64.so.7", "/opt/rocm/lib/libamdhip64.so", "libamdhip64.so"]
    for cand in candidates:
        if cand.startswith("/") and not Path(cand).exists():
            continue
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            continue
        else:
            return
    msg = "no HIP runtime (libamdhip64) could be loaded"
    raise EngineUnavailableError(msg)


def load_library(path: str | Path | None = None) -> C.CDLL:
    global _lib  # noqa: PLW0603
    if _lib is None:
        override = path or os.environ.get("ASYNCFLOW_HIP_LIB")            # env override: A/B builds in experiments
        p = Path(override or LIB_PATH)
        if not override and af_build.needs_build():
            # Build on demand: the library is git-ignored, so a fresh checkout (or a tree whose sources changed since the
            # last build -- content hash, not mtime) has none.  Without hipcc a stale library is an error as well: running
            # other code than the sources say is worse than not running.
            if not af_build.have_hipcc():
                if p.exists() and not af_build.STAMP_PATH.exists():
                    # a library shipped prebuilt (or built by a tree that wrote no stamp): nothing says it is stale, and nothing
                    # here could rebuild it -- load it; the ABI version is checked below either way
                    import warnings

                    warnings.warn(f"{p} has no build stamp and hipcc is not available: loading it as it is", RuntimeWarning, stacklevel=2)
                else:
                    what = "not found" if not p.exists() else "was built from other sources than the tree holds"
                    msg = (f"{p} {what} and hipcc is not available to rebuild it (`python -m asyncflow_amd.build`, "
                           "hipcc --offload-arch=gfx950). asyncflow_amd has no CPU fallback.")
                    raise EngineUnavailableError(msg)
            else:
                try:
                    af_build.build()
                except (RuntimeError, OSError) as exc:      # hipcc failed / a read-only tree
                    msg = f"building {p} failed: {type(exc).__name__}: {exc}"
                    raise EngineUnavailableError(msg) from exc
        if not p.exists():
            msg = f"{p} not found. asyncflow_amd has no CPU fallback."
            raise EngineUnavailableError(msg)
        _load_hip_runtime()
        try:
            lib = C.CDLL(str(p))
        except OSError as exc:
            msg = f"cannot load {p}: {exc}"
            raise EngineUnavailableError(msg) from exc
        if lib.af_abi_version() != _abi.AF_ABI_VERSION:
            msg = "libasyncflow_hip.so was built against another ABI version; rebuild it"
            raise EngineUnavailableError(msg)
        _lib = _abi.declare(lib)
    return _lib


def _check(lib: C.CDLL, rc: int, what: str) -> None:
    if rc == _abi.AF_OK:
        return
    text = (lib.af_last_error() or b"").decode(errors="replace")
    if rc == _abi.AF_ERR_NO_DEVICE:
        raise EngineUnavailableError(f"{what}: {text}")
    raise EngineError(f"{what} failed ({rc}): {text}")


def flow_mode(flow: bool | str) -> int:
    """`af_engine_options_t.flow_mode` of the `flow=` keyword: True = the engine's choice (0), False = never (1),
    "always" = whenever the plan is in the stage-parallel kernel's range (2)."""
    if flow == "always":
        return 2
    if isinstance(flow, str):
        msg = f"flow must be True, False or 'always', not {flow!r}"
        raise ValueError(msg)
    return 0 if flow else 1


PLAN_ONLY = _abi.DEVICE_PLAN_ONLY   # Engine(plan, PLAN_ONLY): a planning-only engine (include/asyncflow_hip.h, AF_DEVICE_PLAN_ONLY)


class Engine:
    """One ``af_engine_t``: a lowered plan resident on one GPU."""

    def __init__(self, plan: DevicePlan, device: int = 0, *, request_capacity: int = 0,
                 fifo_capacity: int = 0, force_global_state: bool = False, lanes_per_wave: int = 0,
                 draw_memory_mb: int = 0, expect_shared_instants: bool = False, flow: bool | str = True,
                 flow_list_entries: int = 0, flow_ring_rows: int = 0) -> None:
        self._lib = load_library()
        self.plan = plan
        self.device = device
        self._cplan = plan.as_ctypes()
        opts = _abi.AfEngineOptions(request_capacity, fifo_capacity, int(force_global_state), int(lanes_per_wave),
                                    int(draw_memory_mb), int(expect_shared_instants), flow_mode(flow),
                                    int(flow_list_entries), int(flow_ring_rows))
        handle = C.c_void_p()
        _check(self._lib, self._lib.af_engine_create(C.byref(self._cplan), device, C.byref(opts), C.byref(handle)),
               "af_engine_create")
        self._h = handle
        self._jit_spec: bytes | None = None
        self._jit_image: bytes | None = None

    def _sweep_structs(self, seeds, overrides, clock_ptr, clock_capacity, samples_ptr, tick_capacity, counts_ptr,
                       draw_capacity, online_hist_ptr, online_hist_bins, online_hist_max, online_rps_ptr,
                       online_rps_buckets):
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
        n = int(seeds.shape[0])
        cols = [np.ascontiguousarray(v, dtype=np.float64) for _, _, v in overrides]
        for c in cols:
            if c.shape != (n,):
                msg = f"override column has shape {c.shape}, expected ({n},)"
                raise ValueError(msg)
        ov = (_abi.AfOverride * max(len(cols), 1))()
        for k, (param, index, _) in enumerate(overrides):
            ov[k].param, ov[k].index = int(param), int(index)
            ov[k].values = cols[k].ctypes.data_as(C.POINTER(C.c_double))
        sweep = _abi.AfSweep(n, seeds.ctypes.data_as(C.POINTER(C.c_uint64)), len(cols), ov, int(draw_capacity))
        out = _abi.AfOutputs(int(clock_capacity), C.c_void_p(clock_ptr or None), int(tick_capacity),
                             C.c_void_p(samples_ptr or None), C.c_void_p(counts_ptr),
                             int(online_hist_bins), float(online_hist_max), C.c_void_p(online_hist_ptr or None),
                             int(online_rps_buckets), C.c_void_p(online_rps_ptr or None))
        return sweep, out, (seeds, cols, ov)     # the last item keeps the host arrays alive

    def run(self, seeds: np.ndarray, overrides: Sequence[tuple[int, int, np.ndarray]], *,
            clock_ptr: int, clock_capacity: int, samples_ptr: int, tick_capacity: int, counts_ptr: int,
            draw_capacity: int = 0, specialise: bool = False, online_hist_ptr: int = 0, online_hist_bins: int = 0,
            online_hist_max: float = 0.0, online_rps_ptr: int = 0, online_rps_buckets: int = 0,
            specialise_build: bool = True, summary: dict | None = None) -> _abi.AfStats:
        """Launch the sweep; output pointers are DEVICE addresses owned by the caller.

        ``specialise``: build (or fetch from the cache) kernels with this plan's shape as compile-time
        constants and use them for this sweep (asyncflow_amd/jit.py; worth it for long sweeps);
        ``specialise_build=False``: only from the cache, never a hipcc run.
        ``summary``: the keyword arguments of :meth:`summarize` that name its outputs (``stats_ptr``, ``rps_ptr``,
        ``rps_buckets``, ``hist_ptr``, ``hist_bins``, ``hist_max``, ``series_mean_ptr``, ``series_max_ptr``): run and
        analyzer in ONE call (``af_engine_run_summarized``) -- the same results as ``run`` then ``summarize``, with the
        analyzer of the stage-parallel kernel's full residency rounds hidden beside its last, partial one.
        """
        sweep, out, _keep = self._sweep_structs(seeds, overrides, clock_ptr, clock_capacity, samples_ptr, tick_capacity,
                                                counts_ptr, draw_capacity, online_hist_ptr, online_hist_bins,
                                                online_hist_max, online_rps_ptr, online_rps_buckets)
        if specialise:
            self._specialise(sweep, out, build=specialise_build)
        if summary is not None:
            summ = _abi.AfSummary(int(seeds.shape[0]) if hasattr(seeds, "shape") else len(seeds), int(summary.get("rps_buckets", 0)),
                                  int(summary.get("hist_bins", 0)), float(summary.get("hist_max", 0.0)),
                                  C.c_void_p(summary.get("stats_ptr") or None), C.c_void_p(summary.get("rps_ptr") or None),
                                  C.c_void_p(summary.get("hist_ptr") or None), C.c_void_p(summary.get("series_mean_ptr") or None),
                                  C.c_void_p(summary.get("series_max_ptr") or None))
            _check(self._lib, self._lib.af_engine_run_summarized(self._h, C.byref(sweep), C.byref(out), C.byref(summ)),
                   "af_engine_run_summarized")
            return self.stats()
        _check(self._lib, self._lib.af_engine_run(self._h, C.byref(sweep), C.byref(out)), "af_engine_run")
        return self.stats()

    def prepare(self, seeds: np.ndarray, overrides: Sequence[tuple[int, int, np.ndarray]], **kw) -> None:
        """Build / load the plan-specialised kernels for a sweep of this shape without running it
        (same keyword arguments as :meth:`run`)."""
        kw.pop("specialise", None)
        defaults = {"draw_capacity": 0, "online_hist_ptr": 0, "online_hist_bins": 0, "online_hist_max": 0.0,
                    "online_rps_ptr": 0, "online_rps_buckets": 0}
        defaults.update(kw)
        sweep, out, _keep = self._sweep_structs(seeds, overrides, defaults["clock_ptr"], defaults["clock_capacity"],
                                                defaults["samples_ptr"], defaults["tick_capacity"], defaults["counts_ptr"],
                                                defaults["draw_capacity"], defaults["online_hist_ptr"],
                                                defaults["online_hist_bins"], defaults["online_hist_max"],
                                                defaults["online_rps_ptr"], defaults["online_rps_buckets"])
        self._specialise(sweep, out)

    def jit_spec(self, seeds: np.ndarray, overrides: Sequence[tuple[int, int, np.ndarray]], **kw) -> str:
        """The ``-D`` flags of the plan-specialised kernels a sweep of this shape launches (same keyword arguments as
        :meth:`run`; of the pointers only their PRESENCE enters).  Works on a planning-only engine
        (``device=PLAN_ONLY``: no GPU needed) for sweeps the stage-parallel kernel runs."""
        kw.pop("specialise", None)
        defaults = {"draw_capacity": 0, "online_hist_ptr": 0, "online_hist_bins": 0, "online_hist_max": 0.0,
                    "online_rps_ptr": 0, "online_rps_buckets": 0}
        defaults.update(kw)
        sweep, out, _keep = self._sweep_structs(seeds, overrides, defaults["clock_ptr"], defaults["clock_capacity"],
                                                defaults["samples_ptr"], defaults["tick_capacity"], defaults["counts_ptr"],
                                                defaults["draw_capacity"], defaults["online_hist_ptr"],
                                                defaults["online_hist_bins"], defaults["online_hist_max"],
                                                defaults["online_rps_ptr"], defaults["online_rps_buckets"])
        return self._spec_of(sweep, out).decode()

    def _spec_of(self, sweep: _abi.AfSweep, out: _abi.AfOutputs) -> bytes:
        buf = C.create_string_buffer(2048)
        _check(self._lib, self._lib.af_engine_jit_spec(self._h, C.byref(sweep), C.byref(out), buf, len(buf)),
               "af_engine_jit_spec")
        return buf.value

    def _specialise(self, sweep: _abi.AfSweep, out: _abi.AfOutputs, build: bool = True) -> None:
        import warnings

        from . import jit

        spec = self._spec_of(sweep, out)
        if spec == self._jit_spec:
            return
        try:
            image = jit.code_object(spec.decode(), build=build)
        except jit.JitUnavailableError as exc:      # not an error: the generic kernels do the same job
            if not build:
                # too short a sweep to wait for the compiler: it runs on the generic kernels, and the build goes on beside it
                # for the next sweep of this shape (asyncflow_amd/jit.py::build_in_background)
                jit.build_in_background(spec.decode())
                return
            warnings.warn(f"plan-specialised kernels unavailable, using the generic ones: {exc}", RuntimeWarning,
                          stacklevel=3)
            return
        self._jit_image = image                     # keep the bytes alive while the module is loaded
        _check(self._lib, self._lib.af_engine_set_kernels(self._h, spec, image, len(image)), "af_engine_set_kernels")
        self._jit_spec = spec

    def summarize(self, n: int, *, clock_ptr: int, clock_capacity: int, samples_ptr: int, tick_capacity: int,
                  counts_ptr: int, stats_ptr: int = 0, rps_ptr: int = 0, rps_buckets: int = 0, hist_ptr: int = 0,
                  hist_bins: int = 0, hist_max: float = 0.0, series_mean_ptr: int = 0,
                  series_max_ptr: int = 0) -> _abi.AfStats:
        """Batched analyzer on the device over the outputs of a finished run (DEVICE pointers)."""
        out = _abi.AfOutputs(int(clock_capacity), C.c_void_p(clock_ptr or None), int(tick_capacity),
                             C.c_void_p(samples_ptr or None), C.c_void_p(counts_ptr))
        summ = _abi.AfSummary(int(n), int(rps_buckets), int(hist_bins), float(hist_max),
                              C.c_void_p(stats_ptr or None), C.c_void_p(rps_ptr or None), C.c_void_p(hist_ptr or None),
                              C.c_void_p(series_mean_ptr or None), C.c_void_p(series_max_ptr or None))
        _check(self._lib, self._lib.af_engine_summarize(self._h, C.byref(out), C.byref(summ)), "af_engine_summarize")
        return self.stats()

    def summarize_pooled(self, n: int, n_groups: int, *, clock_ptr: int, clock_capacity: int, counts_ptr: int,
                         stats_ptr: int, group_ptr: int = 0) -> float:
        """Pooled analyzer on the device (``af_engine_summarize_pooled``): the eight latency statistics of every group of
        scenarios, its latencies taken as one sample, into ``stats`` [n_groups, 8] f64.  ``group_ptr``: DEVICE uint32 [n]
        group ids (``_abi.POOL_SKIP`` leaves a scenario out), 0 = all in group 0.  Returns the call's wall time in ms."""
        out = _abi.AfOutputs(int(clock_capacity), C.c_void_p(clock_ptr or None), 0, None, C.c_void_p(counts_ptr))
        req = _abi.AfPooled(int(n), int(n_groups), C.c_void_p(group_ptr or None), C.c_void_p(stats_ptr or None), 0.0)
        _check(self._lib, self._lib.af_engine_summarize_pooled(self._h, C.byref(out), C.byref(req)), "af_engine_summarize_pooled")
        return float(req.elapsed_ms)

    def summarize_windows(self, n: int, n_groups: int, edges: Any, *, clock_ptr: int, clock_capacity: int, counts_ptr: int,
                          stats_ptr: int, group_ptr: int = 0, row_bounds_ptr: int = 0, window_of: str = "finish") -> tuple[float, int]:
        """Windowed analyzer on the device (``af_engine_summarize_windows``): the eight latency statistics of every
        (group, window by finish time) into ``stats`` [n_groups, W, 8] f64, W = len(edges) - 1 (``edges``: HOST float64,
        strictly increasing).  ``group_ptr`` as in :meth:`summarize_pooled`; ``row_bounds_ptr``: optional DEVICE uint32
        [n, W + 1] for the windows' row ranges.  ``window_of="arrival"``: windows by start time
        (``af_engine_summarize_arrival_windows``; ``row_bounds`` then receives cumulative arrival counts).  Returns the
        call's wall time in ms and the engine's scratch size in bytes."""
        from .results import check_window_of

        name = "af_engine_summarize_arrival_windows" if check_window_of(window_of) == "arrival" else "af_engine_summarize_windows"
        e = np.ascontiguousarray(edges, dtype=np.float64)
        if e.ndim != 1 or e.shape[0] < 2:
            msg = f"window edges must be a vector of at least two values, not of shape {e.shape}"
            raise ValueError(msg)
        out = _abi.AfOutputs(int(clock_capacity), C.c_void_p(clock_ptr or None), 0, None, C.c_void_p(counts_ptr))
        req = _abi.AfWindows(int(n), int(n_groups), int(e.shape[0] - 1), C.c_void_p(group_ptr or None),
                             e.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p(stats_ptr or None),
                             C.c_void_p(row_bounds_ptr or None), 0.0, 0)
        _check(self._lib, getattr(self._lib, name)(self._h, C.byref(out), C.byref(req)), name)
        return float(req.elapsed_ms), int(req.scratch_bytes)

    def summarize_quantiles(self, n: int, n_groups: int, levels: Any, *, edges: Any = None, thresholds: Any = None,
                            clock_ptr: int, clock_capacity: int, counts_ptr: int, count_ptr: int = 0, quantiles_ptr: int = 0,
                            within_ptr: int = 0, group_ptr: int = 0, window_of: str = "finish") -> tuple[float, int]:
        """Quantile analyzer on the device (``af_engine_summarize_quantiles``): per (group, window by finish time)
        ``count`` uint32 [n_groups, W], ``quantiles`` f64 [n_groups, W, Q] and ``within`` uint32 [n_groups, W, T] (the
        latencies <= each threshold); a NULL pointer skips an output.  ``levels``: HOST float64 in [0, 1]; ``thresholds``:
        HOST float64 seconds or None; ``edges``: HOST float64, strictly increasing, W = len(edges) - 1, or None: the whole
        run, one cell per group (W = 1).  ``group_ptr`` as in :meth:`summarize_pooled`.  ``window_of="arrival"``: windows
        by start time (``af_engine_summarize_arrival_quantiles``; needs ``edges``).  Returns the call's wall time in ms and
        the engine's scratch size in bytes."""
        from .results import check_levels, check_slo_thresholds, check_window_of

        name = "af_engine_summarize_arrival_quantiles" if check_window_of(window_of) == "arrival" else "af_engine_summarize_quantiles"
        if name == "af_engine_summarize_arrival_quantiles" and edges is None:
            msg = "window_of='arrival' needs windows: the whole run has none"
            raise ValueError(msg)
        q, th = np.ascontiguousarray(check_levels(levels)), np.ascontiguousarray(check_slo_thresholds(thresholds))
        if q.shape[0] == 0 and th.shape[0] == 0:
            msg = "at least one quantile level or one threshold is needed"
            raise ValueError(msg)
        e = None
        if edges is not None:
            e = np.ascontiguousarray(edges, dtype=np.float64)
            if e.ndim != 1 or e.shape[0] < 2:
                msg = f"window edges must be a vector of at least two values, not of shape {e.shape}"
                raise ValueError(msg)
        pd = C.POINTER(C.c_double)
        out = _abi.AfOutputs(int(clock_capacity), C.c_void_p(clock_ptr or None), 0, None, C.c_void_p(counts_ptr))
        req = _abi.AfQuantiles(int(n), int(n_groups), 0 if e is None else int(e.shape[0] - 1), C.c_void_p(group_ptr or None),
                               e.ctypes.data_as(pd) if e is not None else None,
                               int(q.shape[0]), q.ctypes.data_as(pd) if q.shape[0] else None,
                               int(th.shape[0]), th.ctypes.data_as(pd) if th.shape[0] else None,
                               C.c_void_p(count_ptr or None), C.c_void_p(quantiles_ptr or None), C.c_void_p(within_ptr or None), 0.0, 0)
        _check(self._lib, getattr(self._lib, name)(self._h, C.byref(out), C.byref(req)), name)
        return float(req.elapsed_ms), int(req.scratch_bytes)

    def export_cells(self, n: int, *, edges: Any = None, clock_ptr: int, clock_capacity: int, counts_ptr: int, lat_ptr: int,
                     lat_capacity: int, seg_bounds_ptr: int, group_ptr: int = 0, window_of: str = "finish") -> tuple[int, float, int]:
        """The exporting side of the cells across devices (``af_engine_export_cells``): the latencies of the ``n`` scenarios
        that fall into the windows, scenario after scenario and window after window, into ``lat`` (DEVICE float64
        [lat_capacity], the caller's), and the windows' bounds into ``seg_bounds`` (DEVICE uint32 [n, W + 1]; ``edges``
        None: the whole run, W = 1 and the bounds (0, stored rows)).  ``group_ptr``: DEVICE uint32 [n], only
        ``_abi.POOL_SKIP`` matters (nothing is exported for the scenario).  ``window_of`` as in :meth:`summarize_windows`.
        Returns the elements written, the call's wall time in ms and the engine's scratch size in bytes."""
        from .results import check_window_of

        by_arrival = check_window_of(window_of) == "arrival"
        e = None
        if edges is not None:
            e = np.ascontiguousarray(edges, dtype=np.float64)
            if e.ndim != 1 or e.shape[0] < 2:
                msg = f"window edges must be a vector of at least two values, not of shape {e.shape}"
                raise ValueError(msg)
        out = _abi.AfOutputs(int(clock_capacity), C.c_void_p(clock_ptr or None), 0, None, C.c_void_p(counts_ptr))
        req = _abi.AfCellsExport(int(n), 0 if e is None else int(e.shape[0] - 1), int(by_arrival), C.c_void_p(group_ptr or None),
                                 e.ctypes.data_as(C.POINTER(C.c_double)) if e is not None else None, C.c_void_p(lat_ptr or None),
                                 int(lat_capacity), C.c_void_p(seg_bounds_ptr or None), 0, 0.0, 0)
        _check(self._lib, self._lib.af_engine_export_cells(self._h, C.byref(out), C.byref(req)), "af_engine_export_cells")
        return int(req.lat_count), float(req.elapsed_ms), int(req.scratch_bytes)

    def import_cells(self, n_groups: int, n_windows: int, seg_bounds: Any, seg_begin: Any, *, lat_ptr: int, n_lat: int,
                        group: Any = None, stats_ptr: int = 0, levels: Any = None, thresholds: Any = None, count_ptr: int = 0,
                        quantiles_ptr: int = 0, within_ptr: int = 0) -> tuple[float, int]:
        """The importing side (``af_engine_import_cells``): the exported segments in ``lat`` (DEVICE float64 [n_lat], on
        this engine's device) are merged into the cells of the members' groups and reduced.  ``seg_bounds``: HOST uint32
        [n, Wc + 1] and ``seg_begin``: HOST uint64 [n], the members in the order the cells concatenate them (Wc =
        max(n_windows, 1)); ``group``: HOST uint32 [n] (``_abi.POOL_SKIP`` leaves a member out) or None.  Outputs, each
        optional: ``stats_ptr`` f64 [n_groups, Wc, 8] as :meth:`summarize_windows`; ``count_ptr`` / ``quantiles_ptr`` /
        ``within_ptr`` with ``levels`` / ``thresholds`` as :meth:`summarize_quantiles`.  Returns the call's wall time in ms
        and the engine's scratch size in bytes."""
        from .results import check_levels, check_slo_thresholds

        wc = max(int(n_windows), 1)
        b = np.ascontiguousarray(seg_bounds, dtype=np.uint32)
        if b.ndim != 2 or b.shape[1] != wc + 1:
            msg = f"seg_bounds must be [n, {wc + 1}], not of shape {b.shape}"
            raise ValueError(msg)
        n = int(b.shape[0])
        begin = np.ascontiguousarray(seg_begin, dtype=np.uint64)
        g = None if group is None else np.ascontiguousarray(group, dtype=np.uint32)
        if begin.shape != (n,) or (g is not None and g.shape != (n,)):
            msg = f"seg_begin and group must be vectors of {n} members"
            raise ValueError(msg)
        q = np.ascontiguousarray(check_levels([] if levels is None else levels))
        th = np.ascontiguousarray(check_slo_thresholds(thresholds))
        pd, pu32 = C.POINTER(C.c_double), C.POINTER(C.c_uint32)
        req = _abi.AfCells(n, int(n_groups), int(n_windows), g.ctypes.data_as(pu32) if g is not None else None, b.ctypes.data_as(pu32),
                           begin.ctypes.data_as(C.POINTER(C.c_uint64)), C.c_void_p(lat_ptr or None), int(n_lat), C.c_void_p(stats_ptr or None),
                           int(q.shape[0]), q.ctypes.data_as(pd) if q.shape[0] else None,
                           int(th.shape[0]), th.ctypes.data_as(pd) if th.shape[0] else None,
                           C.c_void_p(count_ptr or None), C.c_void_p(quantiles_ptr or None), C.c_void_p(within_ptr or None), 0.0, 0)
        _check(self._lib, self._lib.af_engine_import_cells(self._h, C.byref(req)), "af_engine_import_cells")
        return float(req.elapsed_ms), int(req.scratch_bytes)

    def summarize_arrivals(self, seeds: Any, overrides: Sequence[tuple[int, int, np.ndarray]], n_groups: int, edges: Any, *,
                           draw_capacity: int, arrivals_ptr: int, group_ptr: int = 0, row_bounds_ptr: int = 0,
                           generated_ptr: int = 0, flags_ptr: int = 0, times_ptr: int = 0, times_given: bool = False,
                           n: int | None = None) -> tuple[float, int]:
        """Arrivals per window and group on the device (``af_engine_summarize_arrivals``): ``arrivals`` uint64
        [n_groups, W], W = len(edges) - 1, the arrival times ``t`` of each group's scenarios with ``edges[w] < t <=
        edges[w + 1]``.  ``seeds`` / ``overrides`` / ``draw_capacity``: the sweep as :meth:`run` takes it (pass the run's
        ``draw_capacity``); nothing is simulated.  ``group_ptr``: DEVICE uint32 [n] (``_abi.POOL_SKIP`` leaves a scenario
        out), 0 = every scenario its own group (``n_groups`` must then be n).  Optional DEVICE outputs: ``row_bounds_ptr``
        uint32 [n, W + 1] (cumulative arrival counts at the edges), ``generated_ptr`` uint32 [n], ``flags_ptr`` uint32 [n]
        (``FLAG_DRAW_OVERFLOW``).  ``times_ptr``: DEVICE float64 [n, draw_capacity]; with ``times_given=False`` it receives
        the generated arrival times (+inf behind the last), with ``times_given=True`` its rows are counted instead of
        generated ones (``seeds`` may then be None with ``n`` given).  Returns the call's wall time in ms and the engine's
        scratch size in bytes."""
        e = np.ascontiguousarray(edges, dtype=np.float64)
        if e.ndim != 1 or e.shape[0] < 2:
            msg = f"window edges must be a vector of at least two values, not of shape {e.shape}"
            raise ValueError(msg)
        if seeds is None:
            if n is None or not (times_given and times_ptr):
                msg = "summarize_arrivals without seeds needs n, times_ptr and times_given=True"
                raise ValueError(msg)
            sweep, _keep = _abi.AfSweep(int(n), None, 0, None, int(draw_capacity)), None
        else:
            sweep, _out, _keep = self._sweep_structs(seeds, overrides, 0, 0, 0, 0, 0, draw_capacity, 0, 0, 0.0, 0, 0)
        req = _abi.AfArrivals(int(sweep.n_scenarios), int(n_groups), int(e.shape[0] - 1), C.c_void_p(group_ptr or None),
                              e.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p(times_ptr or None), int(bool(times_given)),
                              C.c_void_p(arrivals_ptr or None), C.c_void_p(row_bounds_ptr or None),
                              C.c_void_p(generated_ptr or None), C.c_void_p(flags_ptr or None), 0.0, 0)
        _check(self._lib, self._lib.af_engine_summarize_arrivals(self._h, C.byref(sweep), C.byref(req)), "af_engine_summarize_arrivals")
        return float(req.elapsed_ms), int(req.scratch_bytes)

    def summarize_inflight(self, n: int, n_groups: int, tick_edges: Any, sample_period: float, *, clock_ptr: int,
                           clock_capacity: int, tick_capacity: int, counts_ptr: int, count_ptr: int, sum_ptr: int,
                           min_ptr: int = 0, max_ptr: int = 0, above_ptr: int = 0, hist_ptr: int = 0, under_ptr: int = 0,
                           in_flight_ptr: int = 0, started_ptr: int = 0, finished_ptr: int = 0, group_ptr: int = 0,
                           threshold: int = 0, bins: int = 0, lo: int = 0) -> tuple[float, int]:
        """Requests in flight on the device (``af_engine_summarize_inflight``): request i of a scenario's clock rows is
        counted in the sample rows ``floor(start / sample_period) <= k < floor(finish / sample_period)`` (the host definition
        is :func:`asyncflow_amd.results.in_flight_series`).  Per (group, window of ticks) ``count`` uint32, ``sum`` uint64 and,
        each skipped by a pointer of 0, ``min`` / ``max`` / ``above`` (the values > ``threshold``) uint32 [n_groups, W], W =
        len(tick_edges) - 1; with ``hist_ptr`` also ``hist`` uint32 [n_groups, W, bins] (bin b: the values equal to ``lo + b``,
        the last bin takes everything above it) and ``under`` uint32 [n_groups, W]; per scenario ``in_flight`` / ``started``
        / ``finished`` uint32 [n, tick_capacity] (rows at or past a scenario's ticks are left untouched).  ``tick_edges``:
        HOST uint32 tick indices, strictly increasing; ``group_ptr`` as in :meth:`summarize_pooled`.  COMPLETED requests
        only: dropped requests and requests still in flight at the end of the run are in no clock row.  Returns the call's
        wall time in ms and the engine's scratch size in bytes."""
        from .results import check_in_flight_bins, check_tick_edges

        b = check_tick_edges(tick_edges)
        threshold, bins, lo = check_in_flight_bins(threshold, bins, lo)
        out = _abi.AfOutputs(int(clock_capacity), C.c_void_p(clock_ptr or None), int(tick_capacity), None, C.c_void_p(counts_ptr or None))
        req = _abi.AfInflight(int(n), int(n_groups), int(b.shape[0] - 1), C.c_void_p(group_ptr or None),
                              b.ctypes.data_as(C.POINTER(C.c_uint32)), float(sample_period), int(threshold), int(bins), int(lo),
                              C.c_void_p(count_ptr or None), C.c_void_p(sum_ptr or None), C.c_void_p(min_ptr or None),
                              C.c_void_p(max_ptr or None), C.c_void_p(above_ptr or None), C.c_void_p(hist_ptr or None),
                              C.c_void_p(under_ptr or None), C.c_void_p(in_flight_ptr or None), C.c_void_p(started_ptr or None),
                              C.c_void_p(finished_ptr or None), 0.0, 0)
        _check(self._lib, self._lib.af_engine_summarize_inflight(self._h, C.byref(out), C.byref(req)), "af_engine_summarize_inflight")
        return float(req.elapsed_ms), int(req.scratch_bytes)

    def summarize_alerts(self, n: int, n_groups: int, tick_edges: Any, sample_period: float, slo: float, rules: Any, *,
                         clock_ptr: int, clock_capacity: int, tick_capacity: int, counts_ptr: int, group_ptr: int = 0,
                         delay_bins: int = 0, delay_width: int = 1, ptrs: dict[str, int] | None = None,
                         outcomes: dict[str, Any] | None = None) -> tuple[float, int]:
        """Burn-rate alert rules per tick on the device (``af_engine_summarize_alerts``; the host definitions are
        :func:`asyncflow_amd.results.completion_ticks`, :func:`~asyncflow_amd.results.alert_firing`,
        :func:`~asyncflow_amd.results.alert_window_stats` and :func:`~asyncflow_amd.results.alert_cells`).  ``rules``: rows of
        ``(long_ticks, short_ticks, num, den, min_total, hold_ticks)``; ``slo``: a request is bad when its latency is above it.
        ``ptrs`` maps output names of ``af_alerts_t`` to device pointers; an output without a pointer is skipped: ``count``
        uint32 [n, W]; ``fired``, ``episodes``, ``longest``, ``longest_start``, ``first``, ``last`` uint32 [n, W, R];
        ``members``, ``fired_members``, ``open_members`` uint32 and ``fire_ticks``, ``fire_episodes`` uint64 [n_groups, W, R];
        ``delay_hist`` uint32 [n_groups, W, R, delay_bins]; ``total``, ``bad``, ``firing`` uint32 [n, tick_capacity] (rows at or
        past a scenario's ticks are left untouched).  ``tick_edges``: HOST uint32 tick indices, strictly increasing;
        ``group_ptr`` as in :meth:`summarize_pooled`.  COMPLETED requests only: dropped requests and requests still in flight
        at the end of the run are in no clock row -- unless ``outcomes`` is given: then the call is
        ``af_engine_outcome_alerts`` (host definition: :func:`asyncflow_amd.results.outcome_ticks`), a request without an
        answer within ``timeout`` seconds is an error at ``arrival + timeout``, and ``total`` / ``bad`` hold completions in time
        plus timeouts.  ``outcomes`` maps the fields of ``af_alert_outcomes_t``: ``times_ptr`` DEVICE float64 [n_time_rows,
        draw_capacity] (as :meth:`summarize_arrivals` hands them out), ``time_row_ptr`` DEVICE uint32 [n] (0: scenario s reads
        row s), ``n_time_rows``, ``draw_capacity``, ``timeout``, and the optional DEVICE outputs ``timeouts`` uint32 [n,
        tick_capacity], ``timed_out``, ``deficit``, ``flags`` uint32 [n] (``_abi.OUTCOME_ROWS_TRUNCATED``,
        ``_abi.OUTCOME_DEFICIT``).  Returns the call's wall time in ms and the engine's scratch size in bytes."""
        from .results import check_tick_edges

        b = check_tick_edges(tick_edges)
        rows = np.ascontiguousarray(rules, dtype=np.uint32).reshape(-1, 6)
        p = dict(ptrs or {})
        names = ("count", "fired", "episodes", "longest", "longest_start", "first", "last", "members", "fired_members",
                 "open_members", "fire_ticks", "fire_episodes", "delay_hist", "total", "bad", "firing")
        unknown = set(p) - set(names)
        if unknown:
            msg = f"unknown alert outputs {sorted(unknown)}"
            raise ValueError(msg)
        out = _abi.AfOutputs(int(clock_capacity), C.c_void_p(clock_ptr or None), int(tick_capacity), None, C.c_void_p(counts_ptr or None))
        req = _abi.AfAlerts(int(n), int(n_groups), int(b.shape[0] - 1), int(rows.shape[0]), C.c_void_p(group_ptr or None),
                            b.ctypes.data_as(C.POINTER(C.c_uint32)), rows.ctypes.data_as(C.POINTER(_abi.AfAlertRule)),
                            float(sample_period), float(slo), int(delay_bins), int(delay_width),
                            *(C.c_void_p(p.get(k) or None) for k in names), 0.0, 0)
        if outcomes is None:
            _check(self._lib, self._lib.af_engine_summarize_alerts(self._h, C.byref(out), C.byref(req)), "af_engine_summarize_alerts")
            return float(req.elapsed_ms), int(req.scratch_bytes)
        oc = dict(outcomes)
        keys = ("times_ptr", "time_row_ptr", "n_time_rows", "draw_capacity", "timeout", "timeouts", "timed_out", "deficit", "flags")
        unknown = set(oc) - set(keys)
        if unknown:
            msg = f"unknown alert outcome fields {sorted(unknown)}"
            raise ValueError(msg)
        ocs = _abi.AfAlertOutcomes(C.c_void_p(oc.get("times_ptr") or None), C.c_void_p(oc.get("time_row_ptr") or None),
                                   int(oc.get("n_time_rows", 0)), int(oc.get("draw_capacity", 0)), float(oc.get("timeout", math.nan)),
                                   *(C.c_void_p(oc.get(k) or None) for k in ("timeouts", "timed_out", "deficit", "flags")))
        _check(self._lib, self._lib.af_engine_outcome_alerts(self._h, C.byref(out), C.byref(ocs), C.byref(req)),
               "af_engine_outcome_alerts")
        return float(req.elapsed_ms), int(req.scratch_bytes)

    def summarize_exemplars(self, n: int, n_groups: int, k: int, *, edges: Any = None, window_of: str = "finish", clock_ptr: int,
                            clock_capacity: int, counts_ptr: int, total_ptr: int, scenario_ptr: int, row_ptr: int, pair_ptr: int,
                            kept_ptr: int = 0, state_ptr: int = 0, samples_ptr: int = 0, tick_capacity: int = 0,
                            sample_period: float = 0.0, group_ptr: int = 0) -> tuple[float, int]:
        """The ``k`` slowest requests per (group, time window) with their identity, on the device
        (``af_engine_summarize_exemplars``; the host definition is :func:`asyncflow_amd.results.latency_exemplars`): larger
        latency first, ties by ascending scenario index, then row index.  With W' = len(edges) - 1 windows (``edges=None``: one
        window over all time) and C = n_groups * W' cells: ``total`` uint64 [C], ``kept`` uint32 [C] (skipped by a pointer of
        0), ``scenario`` / ``row`` uint32 [C, k], ``pair`` float64 [C, k, 2] (the stored start / finish, 16-byte aligned) and,
        with ``state_ptr`` (needs ``samples_ptr``, ``tick_capacity`` and ``sample_period``), ``state`` uint32 [C, k,
        n_series]: the sample row the request met on arrival.  Every byte of the slots at or past ``kept`` is 0xFF.
        ``window_of``: ``"finish"`` or ``"arrival"`` (needs edges); ``group_ptr`` as in :meth:`summarize_pooled`.  Returns the
        call's wall time in ms and the engine's scratch size in bytes."""
        from .results import check_edges, check_exemplar_k, check_window_of

        by_arrival = check_window_of(window_of) == "arrival"
        e = None if edges is None else check_edges(edges)
        if e is None and by_arrival:
            msg = "window_of='arrival' needs edges: the whole run has no window"
            raise ValueError(msg)
        out = _abi.AfOutputs(int(clock_capacity), C.c_void_p(clock_ptr or None), int(tick_capacity), C.c_void_p(samples_ptr or None),
                             C.c_void_p(counts_ptr or None))
        req = _abi.AfExemplars(int(n), int(n_groups), 0 if e is None else int(e.shape[0] - 1), C.c_void_p(group_ptr or None),
                               None if e is None else e.ctypes.data_as(C.POINTER(C.c_double)), 1 if by_arrival else 0,
                               check_exemplar_k(k), float(sample_period), C.c_void_p(total_ptr or None), C.c_void_p(kept_ptr or None),
                               C.c_void_p(scenario_ptr or None), C.c_void_p(row_ptr or None), C.c_void_p(pair_ptr or None),
                               C.c_void_p(state_ptr or None), 0.0, 0)
        _check(self._lib, self._lib.af_engine_summarize_exemplars(self._h, C.byref(out), C.byref(req)), "af_engine_summarize_exemplars")
        return float(req.elapsed_ms), int(req.scratch_bytes)

    def summarize_latency_histogram(self, n: int, n_groups: int, *, edges: Any = None, window_of: str = "finish", sub_bits: int = 5,
                                    min_exp: int = -20, octaves: int = 32, clock_ptr: int, clock_capacity: int, counts_ptr: int,
                                    count_ptr: int, hist_ptr: int, under_ptr: int = 0, over_ptr: int = 0, nan_ptr: int = 0,
                                    group_ptr: int = 0) -> tuple[float, int]:
        """Log-linear latency histograms per (group, time window) on the device (``af_engine_summarize_latency_histogram``;
        the host definition is :func:`asyncflow_amd.results.latency_histogram`).  Binning on the bit pattern of the float64
        latency: ``octaves`` octaves from ``2 ** min_exp`` seconds, ``2 ** sub_bits`` bins each, B = ``octaves << sub_bits``
        bins (at most 4096).  With W' = len(edges) - 1 windows (``edges=None``: one window over all time) and C = n_groups * W'
        cells: ``count`` uint64 [C] (the rows of the cell), ``hist`` uint32 [C, B] and, each skipped by a pointer of 0,
        ``under`` / ``over`` / ``nan`` uint32 [C] (latencies below the first bin, at or above the last bin's end, NaN).
        ``window_of``: ``"finish"`` or ``"arrival"`` (needs edges); ``group_ptr`` as in :meth:`summarize_pooled`.  Returns the
        call's wall time in ms and the engine's scratch size in bytes."""
        from .results import check_edges, check_latency_bins, check_window_of

        by_arrival = check_window_of(window_of) == "arrival"
        m, e0, o, _ = check_latency_bins(sub_bits, min_exp, octaves)
        e = None if edges is None else check_edges(edges)
        if e is None and by_arrival:
            msg = "window_of='arrival' needs edges: the whole run has no window"
            raise ValueError(msg)
        out = _abi.AfOutputs(int(clock_capacity), C.c_void_p(clock_ptr or None), 0, None, C.c_void_p(counts_ptr or None))
        req = _abi.AfLatencyHistogram(int(n), int(n_groups), 0 if e is None else int(e.shape[0] - 1), C.c_void_p(group_ptr or None),
                                      None if e is None else e.ctypes.data_as(C.POINTER(C.c_double)), 1 if by_arrival else 0,
                                      m, e0, o, C.c_void_p(count_ptr or None), C.c_void_p(hist_ptr or None),
                                      C.c_void_p(under_ptr or None), C.c_void_p(over_ptr or None), C.c_void_p(nan_ptr or None), 0.0, 0)
        _check(self._lib, self._lib.af_engine_summarize_latency_histogram(self._h, C.byref(out), C.byref(req)),
               "af_engine_summarize_latency_histogram")
        return float(req.elapsed_ms), int(req.scratch_bytes)

    def summarize_pairs(self, n: int, n_pairs: int, n_groups: int, *, pair_a_ptr: int, pair_b_ptr: int, times_ptr: int, time_row_ptr: int,
                        n_time_rows: int, draw_capacity: int, clock_ptr: int, clock_capacity: int, counts_ptr: int, pair_counts_ptr: int,
                        pair_sums_ptr: int, unmatched_ptr: int, cell_counts_ptr: int, extremes_ptr: int, hist_ptr: int, tails_ptr: int,
                        above_ptr: int = 0, row_a_ptr: int = 0, row_b_ptr: int = 0, group_ptr: int = 0, edges: Any = None,
                        thresholds: Any = None, sub_bits: int = 5, min_exp: int = -20, octaves: int = 32) -> tuple[float, int]:
        """Paired latency differences under common seeds on the device (``af_engine_summarize_pairs``; the host definition is
        :func:`asyncflow_amd.results.latency_pairs` / :func:`~asyncflow_amd.results.latency_pair_cells`).  Pair p compares
        scenarios ``pair_a[p]`` and ``pair_b[p]`` of the ``n`` scenarios behind ``clock_ptr`` / ``counts_ptr`` through the arrival
        row ``times[time_row[p]]`` (DEVICE float64 [n_time_rows, draw_capacity], as :meth:`summarize_arrivals` writes them).  All
        ids are DEVICE uint32 [n_pairs]; ``group_ptr`` as in :meth:`summarize_pooled` (0: all in group 0).  With W' = len(edges) - 1
        windows by arrival time (``edges=None``: one window), T = len(thresholds), B = ``octaves << sub_bits`` and C = n_groups *
        W': ``pair_counts`` uint32 [n_pairs, W', 5] (both, only_a, only_b, neither, nan), ``pair_sums`` float64 [n_pairs, W', 2]
        (sum_d, sum_a), ``unmatched`` uint32 [n_pairs, 2], ``cell_counts`` uint64 [C, 8] (the five counts, slower, faster, equal),
        ``above`` uint64 [C, T], ``extremes`` float64 [C, 2] (min_d, max_d), ``hist`` uint32 [C, 2, B] (d > 0, d < 0), ``tails``
        uint32 [C, 4] (under_pos, under_neg, over_pos, over_neg) and, optional, ``row_a`` / ``row_b`` uint32 [n_pairs,
        draw_capacity].  Returns the call's wall time in ms and the engine's scratch size in bytes."""
        from .results import check_edges, check_latency_bins, check_pair_thresholds

        m, e0, o, _ = check_latency_bins(sub_bits, min_exp, octaves)
        e = None if edges is None else check_edges(edges)
        th = check_pair_thresholds(thresholds)
        out = _abi.AfOutputs(int(clock_capacity), C.c_void_p(clock_ptr or None), 0, None, C.c_void_p(counts_ptr or None))
        req = _abi.AfPairs(int(n), int(n_pairs), int(n_groups), 0 if e is None else int(e.shape[0] - 1), C.c_void_p(pair_a_ptr or None),
                           C.c_void_p(pair_b_ptr or None), C.c_void_p(group_ptr or None),
                           None if e is None else e.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p(times_ptr or None),
                           C.c_void_p(time_row_ptr or None), int(n_time_rows), int(draw_capacity),
                           th.ctypes.data_as(C.POINTER(C.c_double)) if th.shape[0] else None, int(th.shape[0]), m, e0, o,
                           C.c_void_p(pair_counts_ptr or None), C.c_void_p(pair_sums_ptr or None), C.c_void_p(unmatched_ptr or None),
                           C.c_void_p(cell_counts_ptr or None), C.c_void_p(above_ptr or None), C.c_void_p(extremes_ptr or None),
                           C.c_void_p(hist_ptr or None), C.c_void_p(tails_ptr or None), C.c_void_p(row_a_ptr or None),
                           C.c_void_p(row_b_ptr or None), 0.0, 0)
        _check(self._lib, self._lib.af_engine_summarize_pairs(self._h, C.byref(out), C.byref(req)), "af_engine_summarize_pairs")
        return float(req.elapsed_ms), int(req.scratch_bytes)

    def _state_request(self, column: int, bins: int, lo: float, width: float, sample_period: float, edges: Any) -> tuple[Any, Any]:
        """``af_state_bins_t`` and the checked edges (or None) of the two latency-by-state calls."""
        from .results import _check_series_columns, check_state_bins

        n_bins, lo_f, width_f, period = check_state_bins(bins, lo, width, sample_period)
        col = int(_check_series_columns([column], self.plan.n_series)[0])
        e = None
        if edges is not None:
            e = np.ascontiguousarray(edges, dtype=np.float64)
            if e.ndim != 1 or e.shape[0] < 2:
                msg = f"window edges must be a vector of at least two values, not of shape {e.shape}"
                raise ValueError(msg)
        return _abi.AfStateBins(col, n_bins, lo_f, width_f, period), e

    def summarize_state_windows(self, n: int, n_groups: int, *, column: int, bins: int, sample_period: float, lo: float = 0.0,
                                width: float = 1.0, edges: Any = None, clock_ptr: int, clock_capacity: int, samples_ptr: int,
                                tick_capacity: int, counts_ptr: int, stats_ptr: int, group_ptr: int = 0,
                                row_bounds_ptr: int = 0) -> tuple[float, int]:
        """Latency by the state met on arrival on the device (``af_engine_summarize_state_windows``): the eight latency
        statistics of every (group, arrival window, bin of series ``column`` at the request's arrival tick) into ``stats``
        [n_groups, W', bins, 8] f64.  ``bins`` bins of ``width`` from ``lo`` (the last takes the overflow); ``sample_period``:
        the plan's; ``edges``: HOST float64, strictly increasing, W' = len(edges) - 1, or None: one window with no condition
        on time (W' = 1).  ``group_ptr`` as in :meth:`summarize_pooled`; ``row_bounds_ptr``: optional DEVICE uint32
        [n, W' * bins + 1] for the cumulative cell counts per scenario.  Returns the call's wall time in ms and the engine's
        scratch size in bytes."""
        sb, e = self._state_request(column, bins, lo, width, sample_period, edges)
        out = _abi.AfOutputs(int(clock_capacity), C.c_void_p(clock_ptr or None), int(tick_capacity), C.c_void_p(samples_ptr or None),
                             C.c_void_p(counts_ptr or None))
        req = _abi.AfWindows(int(n), int(n_groups), 0 if e is None else int(e.shape[0] - 1), C.c_void_p(group_ptr or None),
                             e.ctypes.data_as(C.POINTER(C.c_double)) if e is not None else None, C.c_void_p(stats_ptr or None),
                             C.c_void_p(row_bounds_ptr or None), 0.0, 0)
        _check(self._lib, self._lib.af_engine_summarize_state_windows(self._h, C.byref(out), C.byref(sb), C.byref(req)),
               "af_engine_summarize_state_windows")
        return float(req.elapsed_ms), int(req.scratch_bytes)

    def summarize_state_quantiles(self, n: int, n_groups: int, levels: Any, *, thresholds: Any = None, column: int, bins: int,
                                  sample_period: float, lo: float = 0.0, width: float = 1.0, edges: Any = None, clock_ptr: int,
                                  clock_capacity: int, samples_ptr: int, tick_capacity: int, counts_ptr: int, count_ptr: int = 0,
                                  quantiles_ptr: int = 0, within_ptr: int = 0, group_ptr: int = 0) -> tuple[float, int]:
        """Quantiles and SLO counts over the cells of :meth:`summarize_state_windows`
        (``af_engine_summarize_state_quantiles``): ``count`` uint32 [n_groups, W', bins], ``quantiles`` f64
        [n_groups, W', bins, Q] and ``within`` uint32 [n_groups, W', bins, T]; a pointer of 0 skips an output.  ``levels`` and
        ``thresholds`` as in :meth:`summarize_quantiles`, the rest as in :meth:`summarize_state_windows`.  Returns the call's
        wall time in ms and the engine's scratch size in bytes."""
        from .results import check_levels, check_slo_thresholds

        q, th = np.ascontiguousarray(check_levels(levels)), np.ascontiguousarray(check_slo_thresholds(thresholds))
        if q.shape[0] == 0 and th.shape[0] == 0:
            msg = "at least one quantile level or one threshold is needed"
            raise ValueError(msg)
        sb, e = self._state_request(column, bins, lo, width, sample_period, edges)
        pd = C.POINTER(C.c_double)
        out = _abi.AfOutputs(int(clock_capacity), C.c_void_p(clock_ptr or None), int(tick_capacity), C.c_void_p(samples_ptr or None),
                             C.c_void_p(counts_ptr or None))
        req = _abi.AfQuantiles(int(n), int(n_groups), 0 if e is None else int(e.shape[0] - 1), C.c_void_p(group_ptr or None),
                               e.ctypes.data_as(pd) if e is not None else None,
                               int(q.shape[0]), q.ctypes.data_as(pd) if q.shape[0] else None,
                               int(th.shape[0]), th.ctypes.data_as(pd) if th.shape[0] else None,
                               C.c_void_p(count_ptr or None), C.c_void_p(quantiles_ptr or None), C.c_void_p(within_ptr or None), 0.0, 0)
        _check(self._lib, self._lib.af_engine_summarize_state_quantiles(self._h, C.byref(out), C.byref(sb), C.byref(req)),
               "af_engine_summarize_state_quantiles")
        return float(req.elapsed_ms), int(req.scratch_bytes)

    def summarize_series_windows(self, n: int, n_groups: int, tick_edges: Any, *, samples_ptr: int, tick_capacity: int,
                                 counts_ptr: int, count_ptr: int, mean_ptr: int, min_ptr: int = 0, max_ptr: int = 0,
                                 above_ptr: int = 0, group_ptr: int = 0, thresholds: Any = None) -> tuple[float, int]:
        """Sampled-series analyzer on the device (``af_engine_summarize_series_windows``): per (group, window of ticks)
        ``count`` uint32 [n_groups, W] and, per series, ``mean`` f64 and ``min`` / ``max`` / ``above`` uint32 words
        [n_groups, W, n_series], W = len(tick_edges) - 1.  ``tick_edges``: HOST uint32, strictly increasing TICK INDICES
        (sample k carries the label k * sample_period, as the reference's ``get_series`` gives it); ``thresholds``: HOST
        float64 [n_series] or None (0.0 each).  ``group_ptr`` as in :meth:`summarize_pooled`.  Returns the call's wall time
        in ms and the engine's scratch size in bytes."""
        from .results import check_tick_edges

        b = check_tick_edges(tick_edges)
        thr = None
        if thresholds is not None:
            thr = np.ascontiguousarray(thresholds, dtype=np.float64)
            if thr.shape != (self.plan.n_series,):
                msg = f"thresholds must be a vector of one value per series ({self.plan.n_series}), not of shape {thr.shape}"
                raise ValueError(msg)
            if np.isnan(thr).any():
                msg = "thresholds must not be NaN"
                raise ValueError(msg)
        out = _abi.AfOutputs(0, None, int(tick_capacity), C.c_void_p(samples_ptr or None), C.c_void_p(counts_ptr or None))
        req = _abi.AfSeriesWindows(int(n), int(n_groups), int(b.shape[0] - 1), C.c_void_p(group_ptr or None),
                                   b.ctypes.data_as(C.POINTER(C.c_uint32)),
                                   thr.ctypes.data_as(C.POINTER(C.c_double)) if thr is not None else None,
                                   C.c_void_p(count_ptr or None), C.c_void_p(mean_ptr or None), C.c_void_p(min_ptr or None),
                                   C.c_void_p(max_ptr or None), C.c_void_p(above_ptr or None), 0.0, 0)
        _check(self._lib, self._lib.af_engine_summarize_series_windows(self._h, C.byref(out), C.byref(req)),
               "af_engine_summarize_series_windows")
        return float(req.elapsed_ms), int(req.scratch_bytes)

    #: the outputs of :meth:`summarize_series_excursions`, in the order of ``af_series_excursions_t``
    EXCURSION_OUTPUTS = ("count", "above", "runs", "longest", "longest_start", "first", "last", "peak_tick")

    def summarize_series_excursions(self, n: int, tick_edges: Any, *, samples_ptr: int, tick_capacity: int, counts_ptr: int,
                                    count_ptr: int = 0, above_ptr: int = 0, runs_ptr: int = 0, longest_ptr: int = 0,
                                    longest_start_ptr: int = 0, first_ptr: int = 0, last_ptr: int = 0, peak_tick_ptr: int = 0,
                                    thresholds: Any = None) -> tuple[float, int]:
        """Excursion analyzer on the device (``af_engine_summarize_series_excursions``): per (scenario, window of ticks)
        ``count`` uint32 [n, W] and, per series, uint32 [n, W, n_series] each: ``above`` (the ticks above the threshold),
        ``runs`` (the maximal stretches of such ticks, clipped at the window's edges), ``longest`` (ticks) and
        ``longest_start``, ``first``, ``last`` and ``peak_tick`` (absolute tick indices, ``_abi.TICK_NONE`` for none); a
        pointer of 0 skips an output.  ``tick_edges`` and ``thresholds`` as in :meth:`summarize_series_windows`.  Returns
        the call's wall time in ms and the engine's scratch size in bytes."""
        from .results import check_tick_edges

        b = check_tick_edges(tick_edges)
        thr = None
        if thresholds is not None:
            thr = np.ascontiguousarray(thresholds, dtype=np.float64)
            if thr.shape != (self.plan.n_series,):
                msg = f"thresholds must be a vector of one value per series ({self.plan.n_series}), not of shape {thr.shape}"
                raise ValueError(msg)
            if np.isnan(thr).any():
                msg = "thresholds must not be NaN"
                raise ValueError(msg)
        out = _abi.AfOutputs(0, None, int(tick_capacity), C.c_void_p(samples_ptr or None), C.c_void_p(counts_ptr or None))
        ptrs = (count_ptr, above_ptr, runs_ptr, longest_ptr, longest_start_ptr, first_ptr, last_ptr, peak_tick_ptr)
        req = _abi.AfSeriesExcursions(int(n), int(b.shape[0] - 1), b.ctypes.data_as(C.POINTER(C.c_uint32)),
                                      thr.ctypes.data_as(C.POINTER(C.c_double)) if thr is not None else None,
                                      *(C.c_void_p(p or None) for p in ptrs), 0.0, 0)
        _check(self._lib, self._lib.af_engine_summarize_series_excursions(self._h, C.byref(out), C.byref(req)),
               "af_engine_summarize_series_excursions")
        return float(req.elapsed_ms), int(req.scratch_bytes)

    def summarize_series_quantiles(self, n: int, n_groups: int, tick_edges: Any, levels: Any, *, samples_ptr: int,
                                   tick_capacity: int, counts_ptr: int, quantiles_ptr: int, count_ptr: int = 0,
                                   group_ptr: int = 0, columns: Any = None) -> tuple[float, int]:
        """Series-quantile analyzer on the device (``af_engine_summarize_series_quantiles``): per (group, window of ticks)
        ``count`` uint32 [n_groups, W] (0 skips it) and ``quantiles`` f64 [n_groups, W, C, Q], W = len(tick_edges) - 1.
        ``tick_edges``: HOST uint32 tick indices, strictly increasing; ``levels``: HOST float64 in [0, 1], 1 to 16 of them;
        ``columns``: series indices (any order, duplicates allowed) or None: every series, C = n_series.  ``group_ptr`` as
        in :meth:`summarize_pooled`.  Returns the call's wall time in ms and the engine's scratch size in bytes."""
        from .results import _check_series_columns, check_series_levels, check_tick_edges

        b = check_tick_edges(tick_edges)
        q = np.ascontiguousarray(check_series_levels(levels))
        col = None if columns is None else np.ascontiguousarray(_check_series_columns(columns, self.plan.n_series), dtype=np.uint32)
        out = _abi.AfOutputs(0, None, int(tick_capacity), C.c_void_p(samples_ptr or None), C.c_void_p(counts_ptr or None))
        req = _abi.AfSeriesQuantiles(int(n), int(n_groups), int(b.shape[0] - 1), C.c_void_p(group_ptr or None),
                                     b.ctypes.data_as(C.POINTER(C.c_uint32)), int(q.shape[0]), q.ctypes.data_as(C.POINTER(C.c_double)),
                                     0 if col is None else int(col.shape[0]),
                                     col.ctypes.data_as(C.POINTER(C.c_uint32)) if col is not None else None,
                                     C.c_void_p(count_ptr or None), C.c_void_p(quantiles_ptr or None), 0.0, 0)
        _check(self._lib, self._lib.af_engine_summarize_series_quantiles(self._h, C.byref(out), C.byref(req)),
               "af_engine_summarize_series_quantiles")
        return float(req.elapsed_ms), int(req.scratch_bytes)

    def summarize_series_histogram(self, n: int, n_groups: int, tick_edges: Any, bins: int, *, samples_ptr: int,
                                   tick_capacity: int, counts_ptr: int, hist_ptr: int, count_ptr: int = 0, under_ptr: int = 0,
                                   over_ptr: int = 0, group_ptr: int = 0, columns: Any = None, lo: Any = None,
                                   width: Any = None) -> tuple[float, int]:
        """Series-histogram analyzer on the device (``af_engine_summarize_series_histogram``): per (group, window of ticks)
        ``count`` uint32 [n_groups, W] and, per output column, ``hist`` uint32 [n_groups, W, C, bins] and ``under`` / ``over``
        uint32 [n_groups, W, C], W = len(tick_edges) - 1; a pointer of 0 skips ``count``, ``under`` or ``over``.
        ``tick_edges``: HOST uint32 tick indices, strictly increasing; ``columns``: series indices (any order, duplicates
        allowed) or None: every series, C = n_series; ``lo`` / ``width``: HOST float64 [C] each, one binning per output
        column, or both None (0.0 and 1.0: the bin of a count is the count).  ``group_ptr`` as in :meth:`summarize_pooled`.
        Returns the call's wall time in ms and the engine's scratch size in bytes."""
        from .results import _check_series_columns, check_series_bins, check_tick_edges

        b = check_tick_edges(tick_edges)
        col = None if columns is None else np.ascontiguousarray(_check_series_columns(columns, self.plan.n_series), dtype=np.uint32)
        n_col = self.plan.n_series if col is None else int(col.shape[0])
        n_bins, lo_v, width_v = check_series_bins(bins, n_col, lo, width)
        plain = lo is None and width is None
        pd = C.POINTER(C.c_double)
        out = _abi.AfOutputs(0, None, int(tick_capacity), C.c_void_p(samples_ptr or None), C.c_void_p(counts_ptr or None))
        req = _abi.AfSeriesHistogram(int(n), int(n_groups), int(b.shape[0] - 1), C.c_void_p(group_ptr or None),
                                     b.ctypes.data_as(C.POINTER(C.c_uint32)), 0 if col is None else int(col.shape[0]),
                                     col.ctypes.data_as(C.POINTER(C.c_uint32)) if col is not None else None, n_bins,
                                     None if plain else lo_v.ctypes.data_as(pd), None if plain else width_v.ctypes.data_as(pd),
                                     C.c_void_p(count_ptr or None), C.c_void_p(hist_ptr or None), C.c_void_p(under_ptr or None),
                                     C.c_void_p(over_ptr or None), 0.0, 0)
        _check(self._lib, self._lib.af_engine_summarize_series_histogram(self._h, C.byref(out), C.byref(req)),
               "af_engine_summarize_series_histogram")
        return float(req.elapsed_ms), int(req.scratch_bytes)

    def summarize_series_combined(self, n: int, n_groups: int, tick_edges: Any, ops: Any, columns: Any, *, samples_ptr: int,
                                  tick_capacity: int, counts_ptr: int, mean_ptr: int, count_ptr: int = 0, min_ptr: int = 0,
                                  max_ptr: int = 0, above_ptr: int = 0, hist_ptr: int = 0, under_ptr: int = 0, over_ptr: int = 0,
                                  group_ptr: int = 0, thresholds: Any = None, bins: int = 0, lo: Any = None,
                                  width: Any = None) -> tuple[float, int]:
        """Combinations across the series on the device (``af_engine_summarize_series_combined``): combination ``c`` is
        ``ops[c]`` (an ``AF_COMBINE_*`` code) over the series ``columns[c]`` (strictly increasing indices, all integer
        series or all ``ram_in_use`` columns) of one sample row.  Per (group, window of ticks) ``count`` uint32 [n_groups, W]
        and per combination ``mean``, ``min``, ``max`` float64 and ``above`` uint32 [n_groups, W, C]; with ``bins`` above 0
        also ``hist`` uint32 [n_groups, W, C, bins] and ``under`` / ``over`` uint32 [n_groups, W, C].  A pointer of 0 skips
        every output but ``mean``.  ``tick_edges``: HOST uint32 tick indices, strictly increasing; ``thresholds``, ``lo``,
        ``width``: HOST float64 [C] or None (0.0, 0.0 and 1.0 each).  ``group_ptr`` as in :meth:`summarize_pooled`.
        The library checks the combinations.  Returns the call's wall time in ms and the engine's scratch size in bytes."""
        from .results import check_series_bins, check_tick_edges

        b = check_tick_edges(tick_edges)
        op = np.ascontiguousarray(ops, dtype=np.uint32).reshape(-1)
        lists = [np.ascontiguousarray(c, dtype=np.uint32).reshape(-1) for c in columns]
        if len(lists) != op.shape[0]:
            msg = f"{op.shape[0]} ops for {len(lists)} column lists"
            raise ValueError(msg)
        n_c = int(op.shape[0])
        start = np.ascontiguousarray(np.concatenate([[0], np.cumsum([x.shape[0] for x in lists])]), dtype=np.uint32)
        cols = np.ascontiguousarray(np.concatenate(lists) if lists else np.zeros(0), dtype=np.uint32)
        pd, pu = C.POINTER(C.c_double), C.POINTER(C.c_uint32)
        thr = None if thresholds is None else np.ascontiguousarray(thresholds, dtype=np.float64)
        if thr is not None and thr.shape != (n_c,):
            msg = f"thresholds must be one value per combination ({n_c}), not of shape {thr.shape}"
            raise ValueError(msg)
        n_bins, lo_v, width_v = 0, None, None
        if bins or lo is not None or width is not None:
            n_bins, lo_v, width_v = check_series_bins(bins, n_c, lo, width)
        plain = lo is None and width is None
        out = _abi.AfOutputs(0, None, int(tick_capacity), C.c_void_p(samples_ptr or None), C.c_void_p(counts_ptr or None))
        req = _abi.AfSeriesCombined(int(n), int(n_groups), int(b.shape[0] - 1), C.c_void_p(group_ptr or None), b.ctypes.data_as(pu),
                                    n_c, op.ctypes.data_as(pu), start.ctypes.data_as(pu), cols.ctypes.data_as(pu),
                                    None if thr is None else thr.ctypes.data_as(pd), n_bins,
                                    None if plain else lo_v.ctypes.data_as(pd), None if plain else width_v.ctypes.data_as(pd),
                                    C.c_void_p(count_ptr or None), C.c_void_p(mean_ptr or None), C.c_void_p(min_ptr or None),
                                    C.c_void_p(max_ptr or None), C.c_void_p(above_ptr or None), C.c_void_p(hist_ptr or None),
                                    C.c_void_p(under_ptr or None), C.c_void_p(over_ptr or None), 0.0, 0)
        _check(self._lib, self._lib.af_engine_summarize_series_combined(self._h, C.byref(out), C.byref(req)),
               "af_engine_summarize_series_combined")
        return float(req.elapsed_ms), int(req.scratch_bytes)

    #: the outputs of :meth:`summarize_series_joint`, in the order of ``af_series_joint_t``
    JOINT_OUTPUTS = ("n", "sx", "sy", "sxx", "syy", "sxy")

    def summarize_series_joint(self, n: int, n_groups: int, tick_edges: Any, a: Any, b: Any, lag: Any, *, samples_ptr: int,
                               tick_capacity: int, counts_ptr: int, n_ptr: int, sxy_ptr: int, sx_ptr: int = 0, sy_ptr: int = 0,
                               sxx_ptr: int = 0, syy_ptr: int = 0, group_ptr: int = 0) -> tuple[float, int]:
        """Joint moments of pairs of series on the device (``af_engine_summarize_series_joint``): pair ``p`` is the integer
        series ``a[p]`` at a row and ``b[p]`` ``lag[p]`` rows later, both inside one window.  Per (group, window of ticks,
        pair) ``n`` uint32 [n_groups, W, P], ``sx`` / ``sy`` uint64 of the same shape and ``sxx`` / ``syy`` / ``sxy`` uint64
        [n_groups, W, P, 2] (128-bit sums, low word first); a pointer of 0 skips every output but ``n`` and ``sxy``.
        ``tick_edges``: HOST uint32 tick indices, strictly increasing.  ``group_ptr`` as in :meth:`summarize_pooled`.  The
        library checks the pairs.  Returns the call's wall time in ms and the engine's scratch size in bytes."""
        from .results import check_tick_edges

        e = check_tick_edges(tick_edges)
        cols = [np.ascontiguousarray(v, dtype=np.uint32).reshape(-1) for v in (a, b, lag)]
        if not cols[0].shape == cols[1].shape == cols[2].shape:
            msg = f"a, b and lag must have one entry per pair each, not {[int(c.shape[0]) for c in cols]}"
            raise ValueError(msg)
        pu = C.POINTER(C.c_uint32)
        out = _abi.AfOutputs(0, None, int(tick_capacity), C.c_void_p(samples_ptr or None), C.c_void_p(counts_ptr or None))
        req = _abi.AfSeriesJoint(int(n), int(n_groups), int(e.shape[0] - 1), C.c_void_p(group_ptr or None), e.ctypes.data_as(pu),
                                 int(cols[0].shape[0]), *(c.ctypes.data_as(pu) for c in cols),
                                 *(C.c_void_p(p or None) for p in (n_ptr, sx_ptr, sy_ptr, sxx_ptr, syy_ptr, sxy_ptr)), 0.0, 0)
        _check(self._lib, self._lib.af_engine_summarize_series_joint(self._h, C.byref(out), C.byref(req)),
               "af_engine_summarize_series_joint")
        return float(req.elapsed_ms), int(req.scratch_bytes)

    def summarize_series_warmup(self, n: int, n_groups: int, tick_edges: Any, columns: Any, batch: int = 5, *, samples_ptr: int,
                                tick_capacity: int, counts_ptr: int, batches_ptr: int, trunc_ptr: int, s1_ptr: int = 0,
                                s2_ptr: int = 0, s1_all_ptr: int = 0, s2_all_ptr: int = 0, group_ptr: int = 0) -> tuple[float, int]:
        """Warm-up truncation of integer series on the device (``af_engine_summarize_series_warmup``): the MSER rule on
        batches of ``batch`` ticks, pooled over the members of a group.  Per (group, window of ticks) ``batches`` uint32
        [n_groups, W]; per column also ``trunc`` uint32 [n_groups, W, C], ``s1`` / ``s1_all`` uint64 [n_groups, W, C, 2] and
        ``s2`` / ``s2_all`` uint64 [n_groups, W, C, 3] (the sums at the truncation point and at 0, low word first); a pointer
        of 0 skips every output but ``batches`` and ``trunc``.  ``tick_edges``: HOST uint32 tick indices, strictly
        increasing; ``columns``: HOST series indices, any order.  ``group_ptr`` as in :meth:`summarize_pooled`.  The library
        checks the columns.  Returns the call's wall time in ms and the engine's scratch size in bytes."""
        from .results import check_tick_edges, check_warmup_batch

        e = check_tick_edges(tick_edges)
        n_b = check_warmup_batch(batch)
        raw = np.asarray(columns)
        if raw.ndim != 1 or raw.dtype.kind not in "iu" or (raw.size and (raw.min() < 0 or raw.max() > 0xFFFFFFFF)):
            msg = "columns must be a vector of series indices"
            raise ValueError(msg)
        cols = np.ascontiguousarray(raw, dtype=np.uint32)
        pu = C.POINTER(C.c_uint32)
        out = _abi.AfOutputs(0, None, int(tick_capacity), C.c_void_p(samples_ptr or None), C.c_void_p(counts_ptr or None))
        req = _abi.AfSeriesWarmup(int(n), int(n_groups), int(e.shape[0] - 1), C.c_void_p(group_ptr or None), e.ctypes.data_as(pu),
                                  int(cols.shape[0]), cols.ctypes.data_as(pu), n_b,
                                  *(C.c_void_p(p or None) for p in (batches_ptr, trunc_ptr, s1_ptr, s2_ptr, s1_all_ptr, s2_all_ptr)), 0.0, 0)
        _check(self._lib, self._lib.af_engine_summarize_series_warmup(self._h, C.byref(out), C.byref(req)),
               "af_engine_summarize_series_warmup")
        return float(req.elapsed_ms), int(req.scratch_bytes)

    def gather(self, comm: "C.c_void_p | int", world_size: int, n_local: int, local: dict, gathered: dict, *,
               rps_buckets: int = 0, hist_bins: int = 0) -> _abi.AfStats:
        """``af_engine_gather``: ONE grouped RCCL all-gather of the per-scenario summaries.

        ``local`` / ``gathered`` map ``stats | rps | hist | series_mean | series_max`` to DEVICE pointers
        (0 / missing = not gathered); every rank passes the same ``n_local`` (pad the last shard)."""
        def summ(n: int, ptrs: dict) -> _abi.AfSummary:
            return _abi.AfSummary(int(n), int(rps_buckets), int(hist_bins), 0.0,
                                  C.c_void_p(ptrs.get("stats") or None), C.c_void_p(ptrs.get("rps") or None),
                                  C.c_void_p(ptrs.get("hist") or None), C.c_void_p(ptrs.get("series_mean") or None),
                                  C.c_void_p(ptrs.get("series_max") or None))

        a, b = summ(n_local, local), summ(n_local * world_size, gathered)
        _check(self._lib, self._lib.af_engine_gather(self._h, comm, int(world_size), C.byref(a), C.byref(b)), "af_engine_gather")
        return self.stats()

    def probe_scratch(self, bytes: int, word: int) -> None:  # noqa: A002
        """Test probe (``af_probe_scratch``): the engine's scratch pool becomes exactly ``bytes`` large and every 32-bit word
        of it ``word``; every later growth of the pool starts as ``word`` too."""
        _check(self._lib, self._lib.af_probe_scratch(self._h, C.c_uint64(int(bytes)), C.c_uint32(int(word) & 0xFFFFFFFF)),
               "af_probe_scratch")

    def flow_reason(self) -> str:
        """'' when the stage-parallel kernel can run this plan, else why it always runs on the next-event kernels."""
        return (self._lib.af_engine_flow_reason(self._h) or b"").decode()

    def stats(self) -> _abi.AfStats:
        st = _abi.AfStats()
        _check(self._lib, self._lib.af_engine_stats(self._h, C.byref(st)), "af_engine_stats")
        return st

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.af_engine_destroy(self._h)
            self._h = None

    def __del__(self) -> None:  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def probe_math(kind: int, x: np.ndarray, y: np.ndarray | None = None, seed: int = 0, device: int = 0) -> np.ndarray:
    """Evaluate the engine's own RNG/math on the GPU (spec pinning, tests only)."""
    lib = load_library()
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(x)
    pd = C.POINTER(C.c_double)
    yp = None
    if y is not None:
        y = np.ascontiguousarray(y, dtype=np.float64)
        yp = y.ctypes.data_as(pd)
    _check(lib, lib.af_probe_math(device, kind, C.c_uint64(seed), x.ctypes.data_as(pd), yp, out.ctypes.data_as(pd), x.size),
           "af_probe_math")
    return out
