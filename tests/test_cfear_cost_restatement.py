"""tests/cfear_cost_np.py, the arithmetic contract of rsx_cfear_params.cost / loss / weights, without a GPU: with (0, 0, 0) it is
tests/cfear_np.py and tests/cfear_track_np.py field for field; the 17 other combinations register what the default registers;
the wall that point-to-line cannot register, point-to-point and point-to-distribution can; and no decision of any case that the
GPU tests compare lies within 1e-9 of its threshold, so that they leave out none.
PARITY UNPINNED w.r.t. CFEAR's own code, which is not in the reference checkout."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cfear_cost_cases as ccases  # noqa: E402
import cfear_cost_np as cc  # noqa: E402
import cfear_mocomp_cases as mcases  # noqa: E402
import cfear_mocomp_np as cm  # noqa: E402
import cfear_np as cf  # noqa: E402
import cfear_track_cases as cases  # noqa: E402

DEFAULT = (0, 0, 0)
IDS = [cc.name_of(c) for c in ccases.OTHERS]


def _same(a, b):
    """every field of b in a, compared with =="""
    return all(a[f] == b[f] for f in b)


def test_the_default_combination_is_todays_restatement():
    """1a"""
    for c, got in zip(cases.pair_cases(), ccases.pair_wants(DEFAULT)):
        want = cf.register(c[1], c[2], init=c[3] if c[3] is not None else ccases.ID, **c[4])
        assert set(got) == set(want) and _same(got, want), (c[0], got, want)
        assert got["status"] == c[5]
    assert all(a is b for a, b in zip(ccases.joint_jobs(DEFAULT), cases.joint_jobs()))
    for j, got, want in zip(cases.joint_jobs(), ccases.joint_wants(DEFAULT), cases.joint_wants()):
        assert set(got) == set(want) and _same(got, want), (j[0], got, want)
    # and the trackers: plain, and compensated
    recs, taus = mcases.small_timed()
    for got, want in zip(ccases.small_track(DEFAULT, 0), cases.small_track()):
        assert _same(got, dict(want, reg=dict(want["reg"], reserved=0))), (got, want)
    for got, want in zip(ccases.small_track(DEFAULT, 1), mcases.small_track()):
        assert _same(got, want), (got, want)


@pytest.mark.parametrize("combo", ccases.OTHERS, ids=IDS)
def test_the_other_combinations_on_the_pairs(combo):
    """1b, 1c"""
    by_name = {c[0]: (c, w) for c, w in zip(cases.pair_cases(), ccases.pair_wants(combo))}
    moved = by_name["room moved"][1]
    print(f"{cc.name_of(combo)}: room moved in {moved['iterations']} iterations; " +
          ", ".join(f"{n} {w['status']}/{w['iterations']}" for n, (_, w) in by_name.items()))
    assert moved["status"] == 0 and max(abs(moved[f] - v) for f, v in zip(("x", "y", "yaw"), (0.4, -0.3, 0.02))) < 1e-4
    assert moved["correspondences"] == 54 and moved["iterations"] == 3
    far = by_name["100 m apart"][1]
    assert far["status"] == 4 and (far["x"], far["y"], far["yaw"]) == (0.5, 0.25, 0.125)
    assert by_name["empty src"][1]["status"] == 1 and by_name["empty dst"][1]["status"] == 1
    assert by_name["src over the cap"][1]["status"] == 2
    assert by_name["dst at the cap"][1]["status"] == 4  # (a dst of exactly the cap is searched: nothing within the radius)
    # what the feature is for: a wall whose records share one normal
    wall = by_name["normals (1, 0)"][1]
    assert wall["status"] == (5 if combo[0] == cc.COST_P2L else 0), wall
    if combo[0] != cc.COST_P2L:
        assert wall["correspondences"] == 54 and max(abs(wall[f]) for f in ("x", "y", "yaw")) < 1e-9
    for name, (c, w) in by_name.items():
        assert all(math.isfinite(w[f]) for f in ("x", "y", "yaw", "cost")), (name, w)


def test_the_wall_is_degenerate_under_point_to_line_alone():
    """1c, the default beside the others"""
    i = [c[0] for c in cases.pair_cases()].index("normals (1, 0)")
    assert ccases.pair_wants(DEFAULT)[i]["status"] == 5
    assert ccases.pair_wants((cc.COST_P2P, 0, 0))[i]["status"] == 0 and ccases.pair_wants((cc.COST_P2D, 0, 0))[i]["status"] == 0


@pytest.mark.parametrize("combo", ccases.COMBINATIONS, ids=[cc.name_of(c) for c in ccases.COMBINATIONS])
def test_every_margin_is_at_least_1e_9(combo):
    """1d: the GPU tests leave out a case whose margin is below 1e-9; none is"""
    worst = math.inf
    for c, w in zip(cases.pair_cases(), ccases.pair_wants(combo)):
        assert w["margin"] >= 1e-9, (c[0], w)
        worst = min(worst, w["margin"])
    for j, w in zip(ccases.joint_jobs(combo), ccases.joint_wants(combo)):
        assert w["margin"] >= 1e-9 and (w["status"] == j[5] or (j[5] == 0 and w["status"] == 8)), (j[0], w)  # (8: a limit cycle)
        worst = min(worst, w["margin"])
    if combo in ccases.TRACKED:
        for compensate in (0, 1):
            for i, w in enumerate(ccases.small_track(combo, compensate)):
                assert w["margin"] >= 1e-9, (compensate, i, w)
                worst = min(worst, w["margin"])
    print(f"{cc.name_of(combo)}: smallest margin {worst:.2e}")


def test_the_tracker_subclass():
    """1e: the small sequence under P2P + Cauchy + weights; feeding it in pieces, with other work in between, changes nothing"""
    combo = ccases.TRACKED[0]
    recs, taus = mcases.small_timed()
    for compensate in (0, 1):
        whole = ccases.small_track(combo, compensate)
        assert all(w["reg"]["status"] in (0, 8) for w in whole[1:]) and whole[0]["keyframe"] == 1  # (8: a limit cycle, the pose still returned)
        assert max(w["n_keyframes"] for w in whole) == 3  # the ring fills
        t = cc.CostTracker(compensate=compensate, **cases.SMALL_TRACK, **ccases.as_kw(combo))
        other = cc.CostTracker(compensate=compensate, **cases.SMALL_TRACK, **ccases.as_kw(combo))
        parts = []
        for a, b in ((0, 1), (1, 3), (3, 8)):
            parts += [t.push(recs[i], taus[i] if compensate else None) for i in range(a, b)]
            other.push(recs[a], taus[a] if compensate else None)  # (another sequence in between: no shared state)
        for p, w in zip(parts, whole):
            assert _same(p, w) and _same(p["reg"], w["reg"])
        # the objective matters: not the default's track, though near it
        base = ccases.small_track(DEFAULT, compensate)
        assert any(w["x"] != b["x"] for w, b in zip(whole, base))
        assert max(math.hypot(w["x"] - b["x"], w["y"] - b["y"]) for w, b in zip(whole, base)) < 0.5
    # compensation leaves the second halves of the records alone: the weights read the input's
    c, _ = cm.compensate(recs[1], taus[1], (0.5, 0.1, 0.02))
    for f in ("lambda_max", "lambda_min", "n_points"):
        assert np.array_equal(c[f], recs[1][f])


def test_validity_and_weights_by_hand():
    """records the validity test refuses are skipped and counted out; the weights are the products of the rule"""
    room = cases.as_records(cases.room64())
    moved = cf.transform(room, (0.4, -0.3, 0.02))
    bad = ccases.poisoned(moved)
    n_bad = len(np.arange(2, len(room), 5))
    clean = cc.register(room, moved, cost=cc.COST_P2D)
    got = cc.register(room, bad, cost=cc.COST_P2D)
    assert clean["correspondences"] == 54 and got["correspondences"] == 54 - n_bad and got["status"] == 0
    assert max(abs(got[f] - v) for f, v in zip(("x", "y", "yaw"), (0.4, -0.3, 0.02))) < 1e-4
    assert _same(cc.register(room, bad, loss=cc.LOSS_CAUCHY), cc.register(room, moved, loss=cc.LOSS_CAUCHY))  # P2L, no weights: not read
    assert cc.register(ccases.poisoned(room), moved, weights=1)["correspondences"] == 54 - n_bad
    assert cc.register(room, bad, weights=1)["correspondences"] == 54 - n_bad
    assert not cc.valid(1.0, 0.0) and not cc.valid(1.0, -1.0) and not cc.valid(1.0, math.nan) and not cc.valid(math.inf, 1.0)
    assert not cc.valid(0.5, 1.0) and cc.valid(1.0, 1.0)
    # one correspondence's weight by hand: identical sets but for lambda and n_points of the src -> w_dir = 1
    src = room.copy()
    src["lambda_max"], src["lambda_min"], src["n_points"] = 3.0, 1.0, 18   # p_i = log 4; dst: p_j = log 3, N_j = 6
    v = (2.0 * math.log(3.0) / (math.log(4.0) + math.log(3.0))) * (2.0 * 6.0 / 24.0)
    a = cc.register(src, moved, weights=1, loss=cc.LOSS_NONE, max_iterations=1)
    b = cc.register(src, moved, loss=cc.LOSS_NONE, max_iterations=1)
    w_dir = math.cos(0.02)  # the first linearisation is at the identity: the normals differ by the motion's yaw
    assert abs(a["cost"] / b["cost"] - v * w_dir) < 1e-6, (a["cost"] / b["cost"], v * w_dir)
