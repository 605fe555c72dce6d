"""Record what the UNMODIFIED reference computes on the cases of tests/test_reference_live.py.

ORACLE / TEST INFRASTRUCTURE ONLY.  Needs the reference sources (oracle/ref_env.py):

    python oracle/make_reference_live.py            # (re)write tests/golden/reference_live/cases.npz
    python oracle/make_reference_live.py --check    # run the reference again, compare with the committed file

tests/test_reference_live.py holds the oracle to these recorded outputs wherever it runs, without the reference.  Per case
(key = ``case_key(payload, seed)``) the file holds:

* ``<key>.payload_json``   the exact input dict;
* ``<key>.counts``         int64 [generated, completed, dropped, ticks];
* ``<key>.clock``          float64 [completed, 2] = ClientRuntime.rqs_clock (start, finish);
* ``<key>.samples``        uint32 [n_series, ticks] sampled series (ram rows: float32 bits);
* ``<key>.raised``         (cases the reference refuses) ``"<exception type>: <message>"`` instead of the arrays above.

and, outside the per-case keys, ``yaml_models`` (the reference's validated model of each example YAML, dumped as JSON) and
``analyzer_lb2_rr_t30`` (what the reference's ResultsAnalyzer and plot helpers report on tests/golden/lb2_rr_t30.npz).
"""

from __future__ import annotations

import argparse
import hashlib
import json
import random
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from oracle import ref_env  # noqa: E402

FIXTURE = ROOT / "tests" / "golden" / "reference_live" / "cases.npz"   # (a folder of its own: not a parity fixture of tests/golden/*.npz)
YAML_CASES = ("single_server.yml", "two_servers_lb.yml", "event_inj_lb.yml", "event_inj_single_server.yml",
              "heavy_inj_single_server.yml")


def case_key(payload: dict, seed: int) -> str:
    return hashlib.sha1((json.dumps(payload, sort_keys=True) + f"\n{seed}").encode()).hexdigest()[:16]


def cases() -> list[tuple[dict, int]]:
    """Every (payload, seed) that tests/test_reference_live.py compares with the reference."""
    from oracle import scenarios as sc

    out = [(sc.random_payload(random.Random(1000 + case), horizon=8), 500 + case) for case in range(12)]
    out.append((sc.overload(horizon=12), 5))
    out += [(sc.tie_storm(random.Random(777000 + case), horizon=12), 5 + case) for case in range(30)]
    out += [(sc.wide_fanout(9, "round_robin"), 1), (sc.wide_fanout(20, "least_connection"), 1)]
    out += [(sc.server_chain(d, m), 2) for d, m in (("exponential", 0.003), ("poisson", 0.7), ("normal", 0.001))]
    out += [(sc.negative_spike_residue(horizon=10), 3), (sc.negative_spike_residue(horizon=6, shift=2.0), 3)]
    out.append((sc.ram_starved(30), 1))
    out += [(sc.fractional_ram(False), 22), (sc.fractional_ram(True), 21)]
    out += [(sc.ram_put_deadlock(20), seed) for seed in (4, 8, 11)]
    out += [(sc.fractional_ram_fuzz(random.Random(424200 + case), horizon=10), 900 + case) for case in range(24)]
    out += [(sc.gateway_lb(horizon=12, **kw), 5) for kw in (dict(front=1), dict(front=2, algo="least_connection", backend=True, spike=True),
                                                             dict(front=1, general=True))]
    return out


def record_case(payload: dict, seed: int) -> dict[str, np.ndarray]:
    from oracle.reference_runner import run_reference

    key = case_key(payload, seed)
    out = {f"{key}.payload_json": np.array(json.dumps(payload, sort_keys=True))}
    try:
        ref = run_reference(payload, seed)
    except ValueError as exc:          # (simpy's "Negative delay": the reference yields no results)
        out[f"{key}.raised"] = np.array(f"{type(exc).__name__}: {exc}")
        return out
    out[f"{key}.counts"] = np.array([ref.generated, ref.completed, ref.dropped, ref.ticks], dtype=np.int64)
    out[f"{key}.clock"] = np.asarray(ref.clock, dtype=np.float64)
    out[f"{key}.samples"] = np.asarray(ref.samples, dtype=np.uint32)
    return out


def record_yaml_models() -> np.ndarray:
    import yaml
    from asyncflow.schemas.payload import SimulationPayload

    data = ref_env.REFERENCE_ROOT / "examples" / "yaml_input" / "data"
    models = {name: SimulationPayload.model_validate(yaml.safe_load((data / name).read_text())).model_dump(mode="json")
              for name in YAML_CASES}
    for m in models.values():          # (the metric selections and the LB's servers are sets: dumped in hash order, recorded sorted)
        for k in ("enabled_sample_metrics", "enabled_event_metrics"):
            m["sim_settings"][k] = sorted(m["sim_settings"][k])
        lb = m["topology_graph"]["nodes"].get("load_balancer")
        if lb:
            lb["server_covered"] = sorted(lb["server_covered"])
    return np.array(json.dumps(models, sort_keys=True))


def record_analyzer() -> np.ndarray:
    """The reference's ResultsAnalyzer and ram plot helper on the engine arrays of tests/golden/lb2_rr_t30.npz."""
    import matplotlib

    matplotlib.use("Agg")
    import matplotlib.pyplot as plt

    from asyncflow_amd import _abi
    from asyncflow_amd.plan import lower
    from asyncflow_amd.results import ScenarioResults

    fx = np.load(ROOT / "tests" / "golden" / "lb2_rr_t30.npz", allow_pickle=False)
    plan = lower(json.loads(str(fx["payload_json"])))
    counts = np.zeros(_abi.CNT_SLOTS, dtype=np.uint32)
    counts[_abi.CNT_GENERATED], counts[_abi.CNT_COMPLETED] = int(fx["generated"]), int(fx["completed"])
    counts[_abi.CNT_TICKS] = int(fx["ticks"])
    an = ScenarioResults(plan, counts, fx["clock"], fx["samples"]).to_reference_analyzer()
    fig, ax = plt.subplots()
    an.plot_single_server_ram(ax, plan.server_ids[0])
    ram = [float(v) for v in np.asarray(ax.get_lines()[0].get_ydata(), dtype=np.float64)]
    plt.close(fig)
    return np.array(json.dumps({
        "latency_stats": {str(getattr(k, "value", k)): float(v) for k, v in an.get_latency_stats().items()},
        "throughput": [float(v) for v in an.get_throughput_series()[1]],
        "server_ids": list(an.list_server_ids()),
        "ram_plot_server": plan.server_ids[0],
        "ram_plot_ydata": ram,
    }))


def record_all() -> dict[str, np.ndarray]:
    ref_env.install()
    out: dict[str, np.ndarray] = {}
    for payload, seed in cases():
        out.update(record_case(payload, seed))
    out["yaml_models"] = record_yaml_models()
    out["analyzer_lb2_rr_t30"] = record_analyzer()
    out["simpy_flavour"] = np.array(ref_env.simpy_flavour())
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    fx = record_all()
    if args.check:
        old = np.load(FIXTURE, allow_pickle=False)
        bad = sorted(k for k in fx if k not in old.files or not np.array_equal(old[k], fx[k]))
        print(f"{FIXTURE.name}: {'identical' if not bad else 'DIFFERENT: ' + ', '.join(bad[:8])}")
        return 1 if bad else 0
    np.savez_compressed(FIXTURE, **fx)
    print(f"{len(fx)} arrays -> {FIXTURE.relative_to(ROOT)} ({FIXTURE.stat().st_size} B)")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
