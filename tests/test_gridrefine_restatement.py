"""The refinement's restatement (tests/gridrefine_np.py): its vectorised evaluation against the rule written as a loop over the points
with the ordered sums, the polynomials it turns the pose by, the tie and edge cases, and the property the refinement is built for -- a
pose that the correlative matching leaves up to half a cell off ends within a twentieth of a cell of the truth.  No GPU."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gridmap_cases as gc  # noqa: E402
import gridmap_np as gm  # noqa: E402
import gridmatch_cases as gxc  # noqa: E402
import gridmatch_np as gx  # noqa: E402
import gridrefine_cases as grc  # noqa: E402
import gridrefine_np as gr  # noqa: E402
import kstrongest_np as ks  # noqa: E402
import mocomp_np as mc  # noqa: E402


def test_vectorised_evaluation_equals_the_loop():
    """a 64 x 64 random plane, clouds of 0 .. 300 points at every prior of border_priors (in the map, on and outside every border),
    non-finite points in them: the eleven sums byte for byte, and the counts"""
    L, clouds, priors, p = grc.random_case(64, 64)
    framed = gr.frame(L, p)
    seen = set()
    for i, (pts, t) in enumerate(zip(clouds, priors)):
        if len(pts) > 300:
            continue
        pts = pts.copy()
        if len(pts) > 5:
            pts[3] = (np.nan, 1.0)
            pts[5] = (2.0, np.inf)
        fast, slow = gr.evaluate(framed, pts, t, p), gr.evaluate_naive(L, pts, t, p)
        assert fast[0].dtype == np.float64 and fast[0].tobytes() == slow[0].tobytes(), i
        assert fast[1:] == slow[1:], i
        seen.add((fast[1] == len(pts), fast[2] == fast[1], fast[1] > 0))
    assert len(seen) >= 4          # all placed and not, all inside and not, none placed
    # and a job at the cap, where a partial sum has 32 terms
    pts, t = clouds[-9], priors[-9]
    assert len(pts) == gr.MAX_POINTS
    fast, slow = gr.evaluate(framed, pts, t, p), gr.evaluate_naive(L, pts, t, p)
    assert fast[0].tobytes() == slow[0].tobytes() and fast[1:] == slow[1:] and fast[1] == gr.MAX_POINTS


def test_the_order_of_the_sums_is_the_stated_one():
    """256 partials over points t, t + 256, ..., then the adjacent tree: against that order written out, on terms whose sum depends on it"""
    rng = np.random.default_rng(1)
    terms = (rng.standard_normal((700, 2)) * 10.0 ** rng.integers(-8, 8, (700, 2))).astype(np.float64)
    part = [np.float64(0.0)] * 256
    for k in range(700):
        part[k % 256] = part[k % 256] + terms[k, 0]
    while len(part) > 1:
        part = [part[2 * i] + part[2 * i + 1] for i in range(len(part) // 2)]
    got = gr.ordered_sum(terms)
    assert got[0].tobytes() == part[0].tobytes()
    assert got[0] != np.sum(terms[:, 0]) or got[1] != np.sum(terms[:, 1])          # (the order matters on these terms)
    assert gr.ordered_sum(np.zeros((0, 3))).tolist() == [0.0, 0.0, 0.0]


def test_the_pose_is_turned_by_mocomp_polynomials(monkeypatch):
    calls = []
    real = mc.poly

    def spy(th):
        calls.append(float(th))
        return real(th)

    monkeypatch.setattr(mc, "poly", spy)
    L, clouds, priors, p, _ = grc.smooth_case(64, 64)
    r = gr.refine(L, clouds[1], priors[1], p, gr.params())
    assert len(calls) == r["evaluations"] - 1 and r["accepted"] >= 3
    assert max(abs(c) for c in calls) <= gr.DEFAULTS["max_rotation_step"] < mc.TH_MAX


def test_edges():
    """an all-zero plane: EMPTY, the prior bit for bit; a constant plane: a zero gradient, so the first pivot fails: SINGULAR after one
    evaluation, the prior bit for bit; 0 points: EMPTY; 1 point: a record like any other"""
    L, clouds, priors, p = grc.edge_case("zero")
    r = grc.reference(L, clouds, priors, p, gr.params())[0]
    assert r["status"] == gr.STATUS_EMPTY and r["evaluations"] == 1 and r["accepted"] == 0 and r["transform"].tobytes() == priors[0].tobytes()
    assert r["score"] == 0 and r["cost"] == r["cost_initial"] == 255.0 * 255.0 * 200 and r["n_points"] == 200
    L, clouds, priors, p = grc.edge_case("constant")
    r = grc.reference(L, clouds, priors, p, gr.params())[0]
    assert r["status"] == gr.STATUS_SINGULAR and r["evaluations"] == 1 and r["accepted"] == 0 and r["transform"].tobytes() == priors[0].tobytes()
    assert r["score"] == 7.0 * 100 and r["n_points"] == r["n_inside"] == 100 and not r["hessian"].any()
    Lr, cr, pr, p = grc.random_case(64, 64)
    res = grc.random_reference(64, 64)
    for i in range(9):          # 0 points
        assert res[i]["status"] == gr.STATUS_EMPTY and res[i]["transform"].tobytes() == pr[i].tobytes() and res[i]["cost"] == 0.0
    one = res[9]                 # 1 point in the map
    assert len(cr[9]) == 1 and one["n_points"] == 1 and one["evaluations"] >= 2 and one["cost"] <= one["cost_initial"]
    # cost never rises, and without an accepted step the prior comes back
    assert (res["cost"] <= res["cost_initial"]).all()
    for r, t in zip(res, pr):
        assert (r["transform"].tobytes() == t.tobytes()) == (r["accepted"] == 0)
    # max_evaluations 1: the budget runs out before a step
    first = grc.random_reference(64, 64, 1)
    assert set(first["status"].tolist()) == {gr.STATUS_EMPTY, gr.STATUS_MAX} and (first["evaluations"] == 1).all()
    assert first["cost"].tobytes() == res["cost_initial"].tobytes()


def test_status_and_place_in_the_batch():
    """a non-finite prior is skipped and leaves its neighbours alone; non-finite points are skipped without a status; a job above the cap
    is refused by the host entry's restatement and skipped by the device entry's; a job's record does not depend on its place"""
    L, clouds, priors, p = grc.random_case(64, 64)
    want = grc.random_reference(64, 64)
    pick = [72, 45, 0, 63, 73, 36]
    sub_c, sub_p = [clouds[i] for i in pick], priors[pick].copy()
    res = grc.reference(L, sub_c, sub_p, p, gr.params())
    assert res.tobytes() == want[pick].tobytes()
    assert grc.reference(L, sub_c[::-1], sub_p[::-1], p, gr.params()).tobytes() == want[pick[::-1]].tobytes()
    for bad in (np.nan, np.inf, -np.inf):
        sub_p[3, 4] = bad
        res = grc.reference(L, sub_c, sub_p, p, gr.params())
        assert res[3]["status"] == gr.STATUS_TRANSFORM and res[3].tobytes().count(b"\0") == 151
        keep = [0, 1, 2, 4, 5]
        assert res[keep].tobytes() == want[pick][keep].tobytes()
    pts = clouds[72].copy()
    pts[[0, 17, 64, 299]] = [(np.nan, 0.0), (1.0, np.inf), (-np.inf, np.nan), (np.nan, np.nan)]
    r = grc.reference(L, [pts], priors[72:73], p, gr.params())[0]
    assert r["status"] in (0, gr.STATUS_MAX) and r["n_points"] == 296 and np.isfinite(r["cost"]) and np.isfinite(r["hessian"]).all()
    big = [np.zeros((gr.MAX_POINTS + 1, 2), dtype=np.float32)]
    with pytest.raises(ValueError):
        grc.reference(L, big, priors[:1], p, gr.params())
    res = grc.reference(L, big, priors[:1], p, gr.params(), device_entry=True)
    assert res[0]["status"] == gr.STATUS_POINTS and res[0].tobytes().count(b"\0") == 151


def test_the_cases_do_what_they_are_there_for():
    """the random planes reach the reject path, lambda growth and MAX; the smooth planes the accept path"""
    for width, height in grc.SIZES:
        rnd, smooth = grc.random_reference(width, height), grc.smooth_reference(width, height)
        assert (rnd["evaluations"] > rnd["accepted"] + 1).any() and (rnd["status"] == gr.STATUS_MAX).any() and (rnd["status"] == 0).any()
        assert (smooth["accepted"] >= 3).any() and (smooth["status"] == 0).any()
        assert (smooth["cost"][1:8] < smooth["cost_initial"][1:8]).all()


@pytest.fixture(scope="module")
def drive():
    synth = importlib.import_module("navtech_radar_slam_amd.synth")
    imgs, T, p, pts, priors = gxc.end_to_end(synth, ks.extract)
    planes = gm.add_batch(gm.zeros(p), imgs[gxc.E2E_SCANS], T[gxc.E2E_SCANS], p, col_offset=gc.META)
    return planes, p, pts, priors


@pytest.mark.parametrize("mode", [0, 1])
def test_a_pose_is_refined_below_the_cell(drive, mode):
    """scan 3 of the synthetic drive against the map of scans 0, 1, 2, 4, 5 (cells of 1 m), from the truth and from five starts up to
    (1.5, 1.2) m and 0.01 rad off: every start ends within 0.05 m and 0.002 rad of the truth in at most 32 evaluations, with a lower cost
    where it was off.  The limits are conditions with a margin over a prototype's 0.011 m and 0.0005 rad.  What the restatement gives
    (distance, |x|, |y| [m], yaw [rad], evaluations, over the six starts):
      mean:  0.0074 .. 0.0076 m (x 0.0044 .. 0.0046, y 0.0058 .. 0.0061), 0.00015 rad, 5 .. 19 evaluations, all converged
      hits:  0.0109 .. 0.0115 m (x 0.0099 .. 0.0103, y 0.0044 .. 0.0056), 0.00049 .. 0.00052 rad, 18 .. 32 evaluations, three of them MAX"""
    planes, p, pts, priors = drive
    truth = grc.e2e_truth(priors)
    L = gx.likelihood(planes, mode)
    res = grc.reference(L, [pts] * len(grc.E2E_STARTS), grc.e2e_starts(truth), p, gr.params())
    worst = [0.0, 0.0]
    for r, off in zip(res, grc.E2E_STARTS):
        dist, dyaw = grc.pose_error(r["transform"], truth)
        print(mode, off, dist, r["transform"][2] - truth[0], r["transform"][5] - truth[1], dyaw, int(r["evaluations"]), int(r["status"]))
        worst = [max(worst[0], dist), max(worst[1], dyaw)]
        assert dist < grc.E2E_LIMIT_M and dyaw < grc.E2E_LIMIT_RAD, (off, dist, dyaw)
        assert r["evaluations"] <= grc.E2E_EVALUATIONS and r["status"] in (0, gr.STATUS_MAX)
        if off != (0.0, 0.0, 0.0):
            assert r["cost"] < r["cost_initial"]
        assert r["cost"] <= r["cost_initial"]
        # the curvature: positive definite at the returned pose
        h = r["hessian"]
        assert np.linalg.eigvalsh(np.array([[h[0], h[1], h[2]], [h[1], h[3], h[4]], [h[2], h[4], h[5]]])).min() > 0
    assert worst[0] < (0.008, 0.012)[mode] and worst[1] < (0.0002, 0.0006)[mode]          # (the figures of the docstring)


@pytest.mark.parametrize("mode", [0, 1])
def test_match_then_refine(drive, mode):
    """the chain: a prior (3.4, -2.3) m and 0.034 rad off; the correlative matching alone leaves more than 0.25 m (it can only undo whole
    cells and whole steps: 0.5 m and 0.004 / 0.006 rad are left); the refinement of its transform lands within the limits above"""
    planes, p, pts, priors = drive
    truth = grc.e2e_truth(priors)
    L = gx.likelihood(planes, mode)
    ex, ey, eth = grc.CHAIN_ERROR
    prior = gc.matrices([(truth[0] + ex, truth[1] + ey, truth[2] + eth)])
    m, _ = gxc.reference(L, [pts], prior, p, gx.params(**gxc.E2E_WINDOW))
    left, left_yaw = grc.pose_error(m[0]["transform"], truth)
    assert m[0]["status"] == 0 and left > 0.25 and left_yaw > 0.002
    r = grc.reference(L, [pts], m["transform"], p, gr.params())[0]
    dist, dyaw = grc.pose_error(r["transform"], truth)
    print(mode, left, left_yaw, dist, dyaw, int(r["evaluations"]))
    assert dist < grc.E2E_LIMIT_M and dyaw < grc.E2E_LIMIT_RAD and r["evaluations"] <= grc.E2E_EVALUATIONS and r["cost"] < r["cost_initial"]
