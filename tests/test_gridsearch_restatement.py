"""The wide-window search's restatement (tests/gridsearch_np.py): a bound is no smaller than any score of its block, the pruned rule
gives the winner that scoring every candidate gives, within match's caps the shared fields are gridmatch_np.pick's bytes, the tie
order and min_score, and the property the search is built for -- a scan is found again tens of metres from its prior at a few
percent of the exhaustive cost.  No GPU."""
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
import gridsearch_cases as gsc  # noqa: E402
import gridsearch_np as gs  # noqa: E402
import kstrongest_np as ks  # noqa: E402


def _transform(prior, k, u, v, p, mp):
    c32, s32 = gx.tables(mp)
    c, s, res = np.float64(c32[k + mp["angle_steps"]]), np.float64(s32[k + mp["angle_steps"]]), np.float64(p["resolution"])
    r00, r01, tx, r10, r11, ty = (np.float64(q) for q in prior)
    return np.array([r00 * c + r01 * s, r01 * c - r00 * s, tx + np.float64(u) * res, r10 * c + r11 * s, r11 * c - r10 * s, ty + np.float64(v) * res])


def _check_against_exhaustive(L, pts, prior, p, mp, what):
    """bound >= block maximum for every block; winner, score and transform of the pruned rule equal the exhaustive pick; within match's
    caps the shared fields are gridmatch_np.pick's bytes -> the record, the share of blocks refined"""
    K, U, V = gs.window(mp)
    vol = gs.volume(L, pts, prior, p, mp)
    r, bnd, refined, T0 = gs.search(L, pts, prior, p, mp)
    assert bnd.dtype == np.uint32 and bnd.shape == (2 * K + 1,) + gs.blocks(mp) and (bnd >= gs.block_max(vol, mp)).all(), what
    assert r["n_blocks"] == bnd.size and r["n_refined"] == np.count_nonzero(bnd >= max(T0, 1)) == np.count_nonzero(refined)
    assert r["score_prior"] == vol[K, V, U] and r["reserved"] == 0
    want = gs.pick_exhaustive(vol, mp)
    if want is None:
        assert r["status"] == (gs.STATUS_EMPTY if mp["min_score"] == 0 else gs.STATUS_BELOW), what
        assert (r["k"], r["u"], r["v"], r["score"], r["bound_runner_up"]) == (0, 0, 0, 0, 0) and r["transform"].tobytes() == np.asarray(prior).tobytes()
    else:
        k, u, v, score = want
        assert (int(r["k"]), int(r["u"]), int(r["v"]), int(r["score"]), int(r["status"])) == (k, u, v, score, 0), what
        assert r["transform"].tobytes() == _transform(prior, k, u, v, p, mp).tobytes(), what
        assert T0 <= score <= bnd[k + K, (v + V) // 8, (u + U) // 8] and refined[k + K, (v + V) // 8, (u + U) // 8]
    if K <= 64 and U <= 32 and V <= 32 and mp["min_score"] == 0:
        m = gx.pick(gx.volume(L, pts, prior, p, gsc.as_match(mp)), pts, prior, p, gsc.as_match(mp))
        for f in gs.SHARED:
            assert r[f].tobytes() == m[f].tobytes(), (what, f, r[f], m[f])
    return r, np.count_nonzero(refined) / refined.size


@pytest.mark.parametrize("K,U,V", gsc.RESTATED)
def test_pruned_rule_equals_the_exhaustive_pick(K, U, V):
    """64 x 64 random planes, 40 points (two of them not finite) at every prior of border_priors (in the map, on and outside every
    border)"""
    p = gc.small_params(64, 64)
    rng = np.random.default_rng(200 + K + U + V)
    L = gxc.plane(9, p)
    names, priors = gxc.border_priors(p)
    mp = gsc.window(K, U, V, angle_step=0.07)
    found = 0
    for name, t in zip(names, priors):
        pts = gxc.cloud(rng, 40, p)
        pts[3] = (np.nan, 1.0)
        pts[5] = (2.0, np.inf)
        r, _ = _check_against_exhaustive(L, pts, t, p, mp, (name, K, U, V))
        assert r["n_points"] <= 38
        found += int(r["status"] == 0)
    assert found >= 5


def test_margin_follows_the_window():
    """PL = max(64, U, V): a point 100 cells outside the map is placed, and scored, only by a window that can bring it in"""
    p = gc.gm.params(width=64, height=64, resolution=0.5, origin_x=0.0, origin_y=0.0)
    L = np.full((64, 64), 9, dtype=np.uint8)
    pts = np.array([[0.0, 0.0]], dtype=np.float32)
    prior = gc.matrices([(-50.0 + 0.25, 10.25, 0.0)])[0]      # cell (-100, 20)
    for U, placed in ((64, 0), (99, 0), (100, 1), (256, 1)):
        mp = gsc.window(0, U, 2)
        r, _ = _check_against_exhaustive(L, pts, prior, p, mp, U)
        assert r["n_points"] == placed and r["status"] == (0 if placed else gs.STATUS_EMPTY)
        if placed:
            assert (int(r["u"]), int(r["v"]), int(r["score"])) == (100, 0, 9)


def test_ties():
    # a zero plane: EMPTY at (0, 0, 0), nothing refined
    L, clouds, priors, p, mm = gxc.tie_zero()
    mp = gsc.window(mm["angle_steps"], mm["x_cells"], mm["y_cells"], mm["angle_step"])
    r, share = _check_against_exhaustive(L, clouds[0], priors[0], p, mp, "zero")
    assert r["status"] == gs.STATUS_EMPTY and (r["k"], r["u"], r["v"], r["n_refined"]) == (0, 0, 0, 0) and r["n_points"] == 200
    # a constant plane: every score and every bound is 7 n = T0: every block is refined (pruning is strict) and (0, 0, 0) wins
    L, clouds, priors, p, mm = gxc.tie_constant()
    mp = gsc.window(mm["angle_steps"], mm["x_cells"], mm["y_cells"], mm["angle_step"])
    r, share = _check_against_exhaustive(L, clouds[0], priors[0], p, mp, "constant")
    bnd = gs.bounds(L, clouds[0], priors[0], p, mp)
    assert (bnd == 700).all() and share == 1.0 and (r["k"], r["u"], r["v"], r["score"], r["status"]) == (0, 0, 0, 700, 0)
    # two rotations tie: the smallest linear index
    L, clouds, priors, p, mm = gxc.tie_rotation()
    mp = gsc.window(mm["angle_steps"], mm["x_cells"], mm["y_cells"], mm["angle_step"])
    r, _ = _check_against_exhaustive(L, clouds[0], priors[0], p, mp, "rotation")
    assert (r["k"], r["u"], r["v"], r["score"]) == (-1, 0, 0, 200)


def test_min_score():
    """one above the peak: BELOW, the prior returned; equal to the peak: the peak"""
    L, clouds, priors, p, mp = gsc.peaked()
    r, _ = _check_against_exhaustive(L, clouds[0], priors[0], p, mp, "no floor")
    assert (r["k"], r["u"], r["v"], r["score"], r["status"], r["score_prior"]) == (0, 5, -3, 200, 0, 0)
    r, _ = _check_against_exhaustive(L, clouds[0], priors[0], p, dict(mp, min_score=200), "at the peak")
    assert (r["k"], r["u"], r["v"], r["score"], r["status"]) == (0, 5, -3, 200, 0) and r["n_refined"] >= 1
    r, _ = _check_against_exhaustive(L, clouds[0], priors[0], p, dict(mp, min_score=201), "above the peak")
    assert (r["k"], r["u"], r["v"], r["score"], r["status"], r["n_refined"]) == (0, 0, 0, 0, gs.STATUS_BELOW, 0)
    assert r["transform"].tobytes() == priors[0].tobytes() and r["n_points"] == 1 and r["n_blocks"] == 3 * 2 * 3
    # a floor that the pooled bound reaches and no score does: blocks are refined, nothing is found
    L2 = L.copy()
    L2[L2 == 200] = 0
    L2[10, 10], L2[12, 12] = 150, 150
    pts = np.array([[0.0, 0.0], [0.5, 0.5]], dtype=np.float32)     # a cell apart both ways: the two cells 150 are two apart
    prior = gc.matrices([(5.25, 5.25, 0.0)])[0]
    r, _ = _check_against_exhaustive(L2, pts, prior, p, dict(gsc.window(0, 9, 6), min_score=300), "bound only")
    assert r["status"] == gs.STATUS_BELOW and r["n_refined"] >= 1 and r["score"] == 0


@pytest.fixture(scope="module")
def drive():
    synth = importlib.import_module("navtech_radar_slam_amd.synth")
    imgs, T, p, pts, priors = gxc.end_to_end(synth, ks.extract)
    planes = gm.add_batch(gm.zeros(p), imgs[gxc.E2E_SCANS], T[gxc.E2E_SCANS], p, col_offset=gc.META)
    return planes, p, pts, priors


@pytest.mark.parametrize("mode", [0, 1])
def test_a_scan_is_found_again_tens_of_metres_away(drive, mode):
    """scan 3 of the synthetic drive against the map of scans 0, 1, 2, 4, 5, the prior of gridmatch's first case moved by another
    (17, -13) m: K = 8, U = V = 32 finds it at (-3, -20, 15) with the score the exhaustive matcher gives at its own small window, and
    refines at most 5 % of the blocks (measured: 27 and 17 of 1377; the cap keeps a vacuous bound from passing)"""
    planes, p, pts, priors = drive
    case = gsc.E2E_NEAR
    mp = gsc.e2e_params(case)
    prior = gsc.moved(priors[case["prior"]], *case["move"])
    r, bnd, refined, T0 = gs.search(gx.likelihood(planes, mode), pts, prior, p, mp)
    print("mode", mode, "refined", int(r["n_refined"]), "of", int(r["n_blocks"]), "T0", T0, "score", int(r["score"]), "bound_runner_up", int(r["bound_runner_up"]))
    assert (int(r["k"]), int(r["u"]), int(r["v"])) == case["winner"] and r["status"] == 0
    assert int(r["score"]) == case["scores"][mode] and r["n_blocks"] == 1377
    assert 1 <= r["n_refined"] <= case["share"] * r["n_blocks"]


def test_a_scan_is_found_again_in_a_window_of_128_cells(drive):
    """the exact prior moved by (71, -52) m, U = V = 128: found again with at most 1 % of 18 513 blocks refined (measured: 41)"""
    planes, p, pts, priors = drive
    case = gsc.E2E_FAR
    mp = gsc.e2e_params(case)
    prior = gsc.moved(priors[case["prior"]], *case["move"])
    r, bnd, refined, T0 = gs.search(gx.likelihood(planes, 0), pts, prior, p, mp)
    print("refined", int(r["n_refined"]), "of", int(r["n_blocks"]), "T0", T0, "score", int(r["score"]), "bound_runner_up", int(r["bound_runner_up"]))
    assert (int(r["k"]), int(r["u"]), int(r["v"])) == case["winner"] and r["status"] == 0
    assert r["n_blocks"] == 18513 and 1 <= r["n_refined"] <= case["share"] * r["n_blocks"]
    assert np.allclose(r["transform"], priors[case["prior"]], atol=1e-9)
