"""The host definitions of the alert analyzer (asyncflow_amd.results: completion_ticks, alert_firing, alert_window_stats,
alert_cells, alert_rule, alert_delay_quantiles) against a brute-force loop over ticks and rows on hand-made clock rows."""

from __future__ import annotations

from fractions import Fraction

import numpy as np
import pytest

from asyncflow_amd import alert_cells, alert_delay_quantiles, alert_firing, alert_rule, alert_window_stats, completion_ticks
from asyncflow_amd.results import alert_rule_ticks, check_alert_rules, scenario_alerts, seconds_to_ticks
from tests.alerts_util import HOLDS, SLO, P, brute_force, firing_words, rows_in_phases, rules_32, rules_few

CELLS = ("fired", "episodes", "longest", "longest_start", "first", "last")


def _same(rows, t_s, rules, edges, slo=SLO, period=P):
    got = scenario_alerts(rows, t_s, period, slo, rules, edges)
    want = brute_force(rows, t_s, period, slo, rules, edges)
    for k in ("total", "bad", "count", "cond", "firing") + CELLS:
        assert np.array_equal(np.asarray(got[k]).astype(np.int64), want[k].astype(np.int64)), k
    return got


def test_random_rows_every_rule_kind_and_window_arrangement():
    rng = np.random.default_rng(1)
    for m, t_s, phase in ((0, 0, 10), (0, 9, 10), (5, 0, 10), (1, 1, 10), (700, 130, 23), (3000, 520, 150), (64, 65, 5)):
        rows = rows_in_phases(rng, m, t_s, phase)
        for edges in ([0, t_s + 1], list(range(0, t_s + 4)), [3, 64, 65, 200, 239, 10 ** 6], [t_s, t_s + 5, 2 ** 32 - 1]):
            got = _same(rows, t_s, rules_few(100), edges)
    got = _same(rows_in_phases(rng, 3000, 520, 150), 520, rules_32(100), [0, 100, 150, 151, 300, 520])
    assert got["firing"][31].any() and (firing_words(got["firing"]) >> 31).any()
    assert {int(h) for h in got["rules"][:, 5]} >= set(HOLDS)
    fired = got["firing"].any(axis=1)
    assert fired[0] and not fired[1] and not fired[4]                    # num == 0 fires; num == den and a huge min_total never


def test_the_partial_look_back_at_the_start_and_single_window_rules():
    rows = [[0.0, 0.5 * P], [0.0, 0.6 * P], [0.0, 1.5 * P], [0.0, 4.5 * P]]        # ticks 0, 0, 1, 4; all bad with slo -1
    t = completion_ticks(rows, 6, P, -1.0)
    assert t["total"].tolist() == [2, 0 + 1, 0, 0, 1, 0] and t["bad"].tolist() == t["total"].tolist()
    f = alert_firing(t["total"], t["bad"], [(3, 3, 1, 2, 0, 1), (3, 1, 1, 2, 0, 1), (3, 3, 1, 2, 3, 1)])
    assert f["cond"][0].tolist() == [True, True, True, True, True, True]      # ticks 0 .. 2 see only the rows that exist
    assert f["cond"][1].tolist() == [True, True, False, False, True, False]   # the short look-back of one tick is empty
    assert f["cond"][2].tolist() == [False, True, True, False, False, False]  # T_long: 2 3 3 1 1 1
    _same(rows, 6, [(3, 3, 1, 2, 0, 1), (3, 1, 1, 2, 0, 1), (3, 3, 1, 2, 3, 1)], [0, 6], slo=-1.0)


def test_num_zero_fires_on_any_bad_request_and_num_equal_den_never():
    rows = [[0.0, 2.5 * P], [2.0 * P, 2.6 * P], [0.0, 7.5 * P]]                   # latencies 2.5 P, 0.6 P, 7.5 P
    t = completion_ticks(rows, 10, P, 2 * P)
    assert t["bad"].tolist() == [0, 0, 1, 0, 0, 0, 0, 1, 0, 0]
    f = alert_firing(t["total"], t["bad"], [(2, 2, 0, 1, 0, 1), (2, 2, 1, 1, 0, 1), (2, 2, 7, 7, 0, 1)])
    assert f["firing"][0].tolist() == [False, False, True, True, False, False, False, True, True, False]
    assert not f["firing"][1].any() and not f["firing"][2].any()
    assert not completion_ticks(rows, 10, P, np.inf)["bad"].any()
    with pytest.raises(ValueError, match="NaN"):
        completion_ticks(rows, 10, P, np.nan)


def test_hold_ticks_one_two_and_longer_than_the_run():
    total = np.array([1] * 12)
    bad = np.array([0, 1, 1, 1, 0, 1, 0, 1, 1, 1, 1, 1])
    f = alert_firing(total, bad, [(1, 1, 0, 1, 1, h) for h in (1, 2, 3, 5, 6, 13)])
    assert f["firing"][0].tolist() == bad.astype(bool).tolist()
    assert np.flatnonzero(f["firing"][1]).tolist() == [2, 3, 8, 9, 10, 11]
    assert np.flatnonzero(f["firing"][2]).tolist() == [3, 9, 10, 11]
    assert np.flatnonzero(f["firing"][3]).tolist() == [11] and not f["firing"][4].any() and not f["firing"][5].any()
    assert alert_firing(np.ones(3), np.ones(3), [(1, 1, 0, 1, 0, 4)])["firing"].sum() == 0      # k + 1 >= hold_ticks


def test_runs_are_clipped_at_window_edges_and_count_in_both():
    firing = np.zeros((2, 20), dtype=bool)
    firing[0, 3:12] = True
    firing[0, 15:17] = True
    firing[1, 19] = True
    s = alert_window_stats(firing, [0, 5, 10, 18, 25, 40])
    assert s["count"].tolist() == [5, 5, 8, 2, 0] and s["lo"].tolist() == [0, 5, 10, 18, 20]
    assert s["fired"][:, 0].tolist() == [2, 5, 4, 0, 0] and s["episodes"][:, 0].tolist() == [1, 1, 2, 0, 0]
    assert s["longest"][:, 0].tolist() == [2, 5, 2, 0, 0] and s["longest_start"][:, 0].tolist() == [3, 5, 10, -1, -1]   # 10: the earliest of two
    assert s["first"][:, 0].tolist() == [3, 5, 10, -1, -1] and s["last"][:, 0].tolist() == [4, 9, 16, -1, -1]
    assert s["last"][3, 1] == 19 == s["hi"][3] - 1 and s["fired"][:, 1].tolist() == [0, 0, 0, 1, 0]
    empty = alert_window_stats(np.zeros((3, 0), dtype=bool), [0, 4])
    assert empty["count"].tolist() == [0] and (empty["first"] == -1).all() and (empty["fired"] == 0).all()


def test_odd_rows_and_row_order():
    rows = np.array([[np.nan, P], [P, np.nan], [-5 * P, 1.5 * P], [9 * P, 2.5 * P], [0.0, np.inf], [-np.inf, 3.5 * P], [np.inf, 3.6 * P],
                     [0.0, -0.5 * P], [-0.0, -0.0], [0.0, 2.0 ** 60], [0.0, 4.0 * P], [0.0, 5.0 * P - 2.0 ** -40]])
    t = completion_ticks(rows, 5, P, 2 * P)
    assert t["total"].tolist() == [1, 1, 1, 2, 2]                        # NaN, +-inf finish, negative and huge quotients: nowhere
    assert t["bad"].tolist() == [0, 1, 0, 1, 2]                          # start < 0 and finish < start count; -inf start is bad, +inf is not
    rng = np.random.default_rng(3)
    rows = rows_in_phases(rng, 900, 200, 31)
    a = scenario_alerts(rows, 200, P, SLO, rules_few(64), [0, 70, 200])
    for perm in (np.argsort(rows[:, 1], kind="stable"), rng.permutation(900), np.arange(900)[::-1]):
        b = scenario_alerts(rows[perm], 200, P, SLO, rules_few(64), [0, 70, 200])
        for k in ("total", "bad", "firing") + CELLS:
            assert np.array_equal(a[k], b[k]), k


def test_group_cells_and_the_delay_histogram():
    rng = np.random.default_rng(4)
    edges, rules = [0, 50, 90, 260, 400], rules_few(64)
    stats = [scenario_alerts(rows_in_phases(rng, 1500, t, 40), t, P, SLO, rules, edges) for t in (260, 300, 0, 75, 300, 300)]
    ids = np.array([0, 1, 1, 0, -1, 1])
    for bins, width in ((0, 1), (4, 1), (3, 7), (1024, 1)):
        got = alert_cells(stats, ids, 3, bins, width)
        for g in range(3):
            mine = [s for s, i in zip(stats, ids) if i == g]
            for w in range(4):
                for r in range(len(rules)):
                    live = [s for s in mine if s["hi"][w] > s["lo"][w]]
                    did = [s for s in live if s["first"][w, r] >= 0]
                    assert got["members"][g, w, r] == len(live) and got["fired_members"][g, w, r] == len(did)
                    assert got["open_members"][g, w, r] == sum(s["last"][w, r] == s["hi"][w] - 1 for s in did)
                    assert got["fire_ticks"][g, w, r] == sum(int(s["fired"][w, r]) for s in mine)
                    assert got["fire_episodes"][g, w, r] == sum(int(s["episodes"][w, r]) for s in mine)
                    if bins:
                        want = [0] * bins
                        for s in did:
                            want[min(int(s["first"][w, r] - s["lo"][w]) // width, bins - 1)] += 1
                        assert got["delay_hist"][g, w, r].tolist() == want
        assert (got["members"][2] == 0).all()
    assert alert_cells(stats, ids, 3, 3, 7)["delay_hist"][..., -1].sum() > 0          # the overflow bin is hit


def test_alert_rule_keeps_exact_fractions_and_refuses():
    assert alert_rule(60, 5, objective=0.999, burn_rate=14.4)["share"] == Fraction(9, 625)
    assert alert_rule(60, bad_share=0.1)["share"] == Fraction(1, 10) and alert_rule(60, bad_share=Fraction(2, 7))["share"] == Fraction(2, 7)
    assert alert_rule(60, bad_share=1)["share"] == 1 and alert_rule(60, bad_share=0)["share"] == 0
    r = alert_rule(60.0, 5.0, bad_share=0.25, hold_s=0.15, min_total=20)
    assert alert_rule_ticks(r, 0.05) == (1200, 100, 1, 4, 20, 3)
    assert alert_rule_ticks(alert_rule(1.0, bad_share=0.5), 0.05) == (20, 20, 1, 2, 1, 1)     # hold_s = 0: one evaluation
    assert check_alert_rules([r, (7, 3, 1, 2, 0, 4)], 0.05).tolist() == [[1200, 100, 1, 4, 20, 3], [7, 3, 1, 2, 0, 4]]
    for kw in ({}, {"bad_share": 0.1, "objective": 0.9, "burn_rate": 2}, {"objective": 0.9}, {"burn_rate": 2.0}, {"bad_share": 1.5},
               {"bad_share": -0.1}, {"objective": 0.9, "burn_rate": 11}, {"bad_share": Fraction(1, 2 ** 32 + 1)},
               {"bad_share": 1e-12}, {"bad_share": 0.5, "min_total": -1}, {"bad_share": 0.5, "hold_s": -1.0}, {"bad_share": float("nan")}):
        with pytest.raises(ValueError):
            alert_rule(60, 5, **kw)
    with pytest.raises(ValueError):
        alert_rule(5, 60, bad_share=0.5)                                 # short above long
    for bad in ((0, 0, 1, 2, 0, 1), (3, 4, 1, 2, 0, 1), (4, 4, 1, 0, 0, 1), (4, 4, 3, 2, 0, 1), (4, 4, 1, 2, 0, 0), (4, 4, 1, 2, 2 ** 32, 1)):
        with pytest.raises(ValueError):
            check_alert_rules([bad])
    with pytest.raises(ValueError):
        check_alert_rules([(4, 4, 1, 2, 0, 1)] * 33)
    with pytest.raises(ValueError):
        check_alert_rules([])


def test_seconds_become_ticks_or_are_refused():
    assert seconds_to_ticks(60.0, 0.05) == 1200 and seconds_to_ticks(0.0, 0.05) == 0 and seconds_to_ticks(0.3, 0.01) == 30
    for bad in (0.07, 0.0501, 1.02):
        with pytest.raises(ValueError, match="multiple"):
            seconds_to_ticks(bad, 0.05)
    with pytest.raises(ValueError, match="multiple"):
        check_alert_rules([alert_rule(1.03, bad_share=0.5)], 0.05)
    with pytest.raises(ValueError):
        check_alert_rules([alert_rule(1.0, 0.01, bad_share=0.5)], 0.05)   # a short look-back below one tick


def test_delay_quantiles_on_a_histogram_built_by_hand():
    hist = np.zeros((2, 1, 2, 4), dtype=np.int64)
    hist[0, 0, 0] = [1, 0, 3, 0]           # delays in ranks: bin 0, then bin 2 three times
    hist[0, 0, 1] = [0, 0, 0, 5]           # all in the overflow bin
    hist[1, 0, 0] = [2, 2, 0, 0]
    edges = np.array([0.0, 0.5, 1.0, 1.5, np.inf])
    q = alert_delay_quantiles({"delay_hist": hist, "delay_edges_s": edges}, [0.0, 0.25, 0.26, 0.5, 1.0])
    assert q["lo_s"][0, 0, 0].tolist() == [0.0, 0.0, 1.0, 1.0, 1.0] and q["hi_s"][0, 0, 0].tolist() == [0.5, 0.5, 1.5, 1.5, 1.5]
    assert q["lo_s"][0, 0, 1].tolist() == [1.5] * 5 and np.isinf(q["hi_s"][0, 0, 1]).all()
    assert q["lo_s"][1, 0, 0].tolist() == [0.0, 0.0, 0.0, 0.0, 0.5] and q["hi_s"][1, 0, 0].tolist() == [0.5, 0.5, 0.5, 0.5, 1.0]
    assert np.isnan(q["lo_s"][1, 0, 1]).all() and np.isnan(q["hi_s"][1, 0, 1]).all() and q["fired"].tolist() == [[[4, 5]], [[4, 0]]]
    with pytest.raises(ValueError):
        alert_delay_quantiles({"delay_hist": hist, "delay_edges_s": edges}, [1.5])
    with pytest.raises(ValueError, match="delay_bins"):
        alert_delay_quantiles({}, [0.5])
