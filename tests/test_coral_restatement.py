"""tests/coral_np.py, the arithmetic contract of csrc/coral.hip, against a scalar double loop and against what the measure is for.
No GPU: the restatement only."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coral_cases as cc  # noqa: E402
import coral_np as co  # noqa: E402


def double_loop(a, b, T=None, radius=3.5, min_points=6, min_other=1):
    """The rules of coral_np.py as an O(n^2) loop over all pairs in Python floats: no grid and no cell table -- a neighbour set is
    taken by distance alone and ordered by (cell, joint index), which is the walk order (the cell number is (iy + 64) * 128 +
    (ix + 64), so ascending cells inside a 3 x 3 block are dy outer, dx inner; and two valid points within r of each other lie in
    adjacent cells, because the cell side is r).  -> points (n,) POINT_DTYPE"""
    xy = co.joint_cloud(a, b, T)
    n, n_a = len(xy), len(np.asarray(a).reshape(-1, 2))
    r, r2 = float(radius), float(radius) * float(radius)
    cell = [None] * n
    for i in range(n):
        x, y = float(xy[i, 0]), float(xy[i, 1])
        if math.isfinite(x) and math.isfinite(y):
            fx, fy = math.floor(x / r), math.floor(y / r)
            if -64 <= fx < 64 and -64 <= fy < 64:
                cell[i] = (fy + 64) * 128 + (fx + 64)
    pts = np.zeros(n, dtype=co.POINT_DTYPE)
    for p in range(n):
        if cell[p] is None:
            continue
        px, py = float(xy[p, 0]), float(xy[p, 1])
        nb = []
        for q in range(n):
            if cell[q] is None:
                continue
            ex, ey = float(xy[q, 0]) - px, float(xy[q, 1]) - py
            if ex * ex + ey * ey <= r2:
                nb.append((cell[q], q))
        nb.sort()
        joint = [q for _, q in nb]
        sep = [q for q in joint if (q >= n_a) == (p >= n_a)]
        pts["m_joint"][p], pts["m_separate"][p] = len(joint), len(sep)
        if not (len(sep) >= min_points and len(joint) - len(sep) >= min_other):
            continue
        for members, field in ((sep, "det_separate"), (joint, "det_joint")):
            m = len(members)
            sx = sy = 0.0
            for q in members:
                sx = sx + float(xy[q, 0])
                sy = sy + float(xy[q, 1])
            mx, my = sx / m, sy / m
            sxx = syy = sxy = 0.0
            for q in members:
                ex, ey = float(xy[q, 0]) - mx, float(xy[q, 1]) - my
                sxx = sxx + ex * ex
                syy = syy + ey * ey
                sxy = sxy + ex * ey
            sxx, syy, sxy = sxx / (m - 1), syy / (m - 1), sxy / (m - 1)
            pts[field][p] = sxx * syy - sxy * sxy
    return pts


@pytest.mark.parametrize("seed, n_a, n_b, extent, T", [
    (1, 300, 280, 14.0, None),
    (2, 150, 300, 9.0, co.pose_matrix((0.4, -0.7, 0.3))),
    (3, 300, 300, 3.4, (0.0, -1.0, 1.0, 1.0, 0.0, -2.0)),   # dense: every neighbourhood holds hundreds of points
    (4, 40, 7, 30.0, None),                                 # sparse: most points are not scored
])
def test_restatement_equals_the_double_loop(seed, n_a, n_b, extent, T):
    a, b = cc.random_cloud(seed, n_a, extent), cc.random_cloud(100 + seed, n_b, extent)
    res, pts = co.quality(a, b, T)
    want = double_loop(a, b, T)
    assert np.array_equal(pts["m_joint"], want["m_joint"]) and np.array_equal(pts["m_separate"], want["m_separate"])
    # (bit-equal: the same additions in the same order)
    assert np.array_equal(pts["det_joint"].view(np.uint64), want["det_joint"].view(np.uint64))
    assert np.array_equal(pts["det_separate"].view(np.uint64), want["det_separate"].view(np.uint64))
    scored = (want["m_separate"] >= 6) & (want["m_joint"] - want["m_separate"] >= 1)
    assert res["n_scored"] == scored.sum() and res["n_scored_a"] == scored[:n_a].sum() and res["n_valid"] == n_a + n_b
    assert not pts["det_joint"][~scored].any() and not pts["det_separate"][~scored].any()
    if scored.any():
        hj = np.mean([0.5 * math.log(max(d, 1e-6)) + co.H_CONST for d in want["det_joint"][scored]])
        hs = np.mean([0.5 * math.log(max(d, 1e-6)) + co.H_CONST for d in want["det_separate"][scored]])
        assert abs(res["h_joint"] - hj) < 1e-12 and abs(res["h_separate"] - hs) < 1e-12 and abs(res["quality"] - (hj - hs)) < 1e-12
        assert res["status"] == 0
    else:
        assert res["status"] == co.STATUS_EMPTY and res["quality"] == 0.0


def test_a_cloud_against_itself():
    """A == B under the identity.  The joint neighbourhood of a point is its separate one with every member twice: the same mean,
    twice the scatter, 2 m members.  So S_joint = 2 (m - 1) / (2 m - 1) S_separate, det_joint = (2 (m - 1) / (2 m - 1))^2
    det_separate, and a point's entropy difference is 0.5 log of that factor = log(1 - 1 / (2 m - 1)): negative, and largest in
    size at the smallest m a scored point can have, m = min_points = 6: |log(10 / 11)| = 0.0953.  That is the bound for ANY cloud.
    Q is the mean of the points' differences, so |Q| < 0.05 holds for a cloud whose neighbourhoods hold 11 points or more on
    average (log(1 - 1 / 21) = -0.0488); the scans used here have a median above 20.  Both are asserted, and Q itself against the
    formula on the counts (1e-9: the rounding of ~10^3 sums of ~40 terms, far below)."""
    clouds, _ = cc.small_clouds()
    for a in (clouds[0], clouds[5]):
        res, pts = co.quality(a, a)
        n = len(a)
        assert res["status"] == 0 and res["n_valid"] == 2 * n
        can = pts["m_separate"] >= 6
        assert res["n_scored"] == can.sum() and np.array_equal(pts["det_separate"] != 0.0, can)  # every such point is scored
        assert np.array_equal(pts["m_joint"], 2 * pts["m_separate"])
        m = pts["m_separate"][can].astype(np.float64)
        assert np.median(m) > 20
        floored = (pts["det_separate"][can] <= 1e-6) | (pts["det_joint"][can] <= 1e-6)
        assert not floored.any()
        want = np.mean(np.log(1.0 - 1.0 / (2.0 * m - 1.0)))
        assert abs(res["quality"] - want) < 1e-9
        assert -math.log(11.0 / 10.0) <= res["quality"] < 0.0
        assert abs(res["quality"]) < 0.05


@pytest.mark.parametrize("i, j", [(0, 1), (0, 3), (2, 7)])
def test_quality_grows_with_misalignment(i, j):
    true, _ = cc.small_want(i, j)
    half, _ = cc.small_want(i, j, dx=0.5)
    far, _ = cc.small_want(i, j, dx=3.0)
    assert true["quality"] < half["quality"] < far["quality"]
    assert true["n_scored"] >= 0.99 * 1536 and true["n_valid"] == 1536 and true["status"] == 0


def test_points_outside_the_grid_set_range_and_change_nothing_else():
    a, b = cc.random_cloud(5, 200, 10.0), cc.random_cloud(6, 180, 10.0)
    T = co.pose_matrix((0.2, 0.1, -0.05))
    res, pts = co.quality(a, b, T)
    assert res["status"] == 0
    junk = np.array([[np.nan, 1.0], [2.0, np.inf], [-np.inf, np.nan], [64 * 3.5, 0.0], [0.0, -64 * 3.5 - 1e-3], [1e30, -1e30]], dtype=np.float32)
    junk_b = junk.copy()   # (B's points are judged where T puts them: the two at the grid's border go well outside)
    junk_b[3:5] = [[300.0, 0.0], [0.0, -300.0]]
    a2, b2 = np.concatenate([a[:50], junk, a[50:]]), np.concatenate([junk_b[::-1], b])
    res2, pts2 = co.quality(a2, b2, T)
    assert res2["status"] == co.STATUS_RANGE
    keep = np.r_[0:50, 56:206, 212:392]
    assert np.array_equal(pts2[keep].view(np.uint8), pts.view(np.uint8))
    assert not pts2[np.r_[50:56, 206:212]].view(np.uint8).any()
    for f in ("quality", "h_joint", "h_separate", "n_scored", "n_scored_a", "n_valid"):
        assert res2[f] == res[f], f
    # the largest cell is inside, its upper border is outside
    edge = np.array([[np.nextafter(np.float32(64 * 3.5), np.float32(0.0)), -64 * 3.5]], dtype=np.float32)
    assert co.quality(edge, edge)[0]["status"] == co.STATUS_EMPTY
    # a non-finite transform: every point of B is invalid, A is judged alone
    res3, pts3 = co.quality(a, b, (1.0, 0.0, np.nan, 0.0, 1.0, 0.0))
    assert res3["status"] == co.STATUS_RANGE | co.STATUS_EMPTY and res3["n_valid"] == len(a) and not pts3[len(a):].view(np.uint8).any()
    assert np.array_equal(pts3["m_joint"][:len(a)], pts3["m_separate"][:len(a)])


def test_min_other_zero_scores_points_without_overlap():
    a = cc.random_cloud(7, 250, 8.0)
    b = cc.random_cloud(8, 250, 8.0) + np.float32(100.0)
    res, pts = co.quality(a, b)
    assert res["status"] == co.STATUS_EMPTY and res["n_scored"] == 0 and (pts["m_joint"] == pts["m_separate"]).all()
    res0, pts0 = co.quality(a, b, min_other=0)
    assert res0["status"] == 0 and res0["n_scored"] == (pts0["m_separate"] >= 6).sum() > 400
    # joint set == separate set: the same sums, the same determinants, a quality of exactly 0
    assert np.array_equal(pts0["det_joint"].view(np.uint64), pts0["det_separate"].view(np.uint64)) and res0["quality"] == 0.0


def test_over_the_cap_is_refused_with_a_zero_result():
    a = np.zeros((co.MAX_POINTS + 1, 2), dtype=np.float32)
    res, pts = co.quality(a, a[:3])
    assert res["status"] == co.STATUS_POINTS and not pts.view(np.uint8).any() and len(pts) == co.MAX_POINTS + 4
    assert res["n_valid"] == 0 and res["quality"] == 0.0
