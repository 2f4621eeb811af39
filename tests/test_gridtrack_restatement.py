"""The grid-map tracker's rule as restated in tests/gridtrack_np.py (include/rsx.h, rsx_gridmap_tracker_*), without a GPU: the glue against
its definitions, what the renormalisation is there for, the drive of the synthetic sequence against the truth, the lost rule, and that
the restatement itself does not depend on how a sequence is cut into pushes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gridmap_cases as gc  # noqa: E402
import gridmatch_cases as gxc  # noqa: E402
import gridrefine_cases as grc  # noqa: E402
import gridtrack_cases as gtc  # noqa: E402
import gridtrack_np as gt  # noqa: E402


def _matrix(T):
    return [[T[0], T[1], T[2]], [T[3], T[4], T[5]], [0.0, 0.0, 1.0]]


def test_the_glue_against_its_definitions():
    """mul is the product of the 3 x 3 matrices with the stated association of the translation's sum, inv the inverse of a rigid motion
    (the transpose, and minus the transpose times the translation), renorm the Newton step written out -- as loops over the entries"""
    rng = np.random.default_rng(1)
    for _ in range(20):
        A, B = rng.normal(size=6), rng.normal(size=6)
        a, b = _matrix(A), _matrix(B)
        want = []
        for i in range(2):
            for j in range(3):
                s = np.float64(a[i][0]) * np.float64(b[0][j]) + np.float64(a[i][1]) * np.float64(b[1][j])
                want.append(s + np.float64(a[i][2]) if j == 2 else s)
        assert np.array(gt.mul(A, B)).tobytes() == np.array(want).tobytes()
        want = []
        for i in range(2):
            row = [np.float64(a[0][i]), np.float64(a[1][i])]                  # the transpose
            want += row + [-(row[0] * np.float64(a[0][2]) + row[1] * np.float64(a[1][2]))]
        assert np.array(gt.inv(A)).tobytes() == np.array(want).tobytes()
        n2 = np.float64(0.0)
        for v in (A[0], A[3]):
            n2 = n2 + np.float64(v) * np.float64(v)
        f = np.float64(1.5) - np.float64(0.5) * n2
        want = [A[0] * f, -(A[3] * f), A[2], A[3] * f, A[0] * f, A[5]]
        assert np.array(gt.renorm(A)).tobytes() == np.array(want).tobytes()
    # a rigid motion: inv is the inverse, mul(P, identity) is P bit for bit
    T = gc.matrices([(3.0, -4.0, 0.7)])[0]
    assert np.allclose(gt.mul(T, gt.inv(T)), gt.IDENTITY, atol=1e-15) and np.allclose(gt.mul(gt.inv(T), T), gt.IDENTITY, atol=1e-15)
    assert np.array(gt.mul(T, gt.IDENTITY)).tobytes() == T.tobytes()


@pytest.mark.parametrize("scale", [1.0 - 1e-4, 1.0 + 1e-4])
def test_renorm_restores_the_unit_norm(scale):
    """a rotation scaled by 1 +- 1e-4: within 1e-7 of unit norm after one step (the Newton step's error is 1.5 e^2 = 1.5e-8), the second
    column rebuilt from the first, the translation untouched"""
    for yaw in (0.0, 0.4, -2.5, 3.0):
        T = gc.matrices([(5.0, -7.0, yaw)])[0]
        T[[0, 1, 3, 4]] *= scale
        R = gt.renorm(T)
        assert abs(np.hypot(R[0], R[3]) - 1.0) < 1e-7 and abs(gt.det(R) - 1.0) < 2e-7
        assert R[1] == -R[3] and R[4] == R[0] and R[2] == T[2] and R[5] == T[5]
        assert abs(np.arctan2(R[3], R[0]) - np.arctan2(T[3], T[0])) < 1e-15


@pytest.mark.parametrize("mode", [0, 1])
def test_the_drive_is_tracked(mode):
    """synth.polar_sequence(11, 16), k-strongest clouds of 4800 points, against the map of scans 0, 3, .., 15 at their true poses (384 x
    384 cells of 1 m), the window K = U = V = 2 of 0.01 rad, the refinement's defaults, from scan 0's true pose: every scan ends within
    grc.E2E_LIMIT_M = 0.05 m and grc.E2E_LIMIT_RAD = 0.002 rad of the truth (the conditions of the refinement's drive test), no scan is
    lost, and the pose is still a rotation.  A prototype's worst: 0.021 m and 0.00048 rad on the mean, 0.026 m and 0.00061 rad on the
    hits; the matcher's winner sits at k = +-2 on most scans (the yaw rate changes by more than 0.02 rad between scans)"""
    _, _, _, clouds, poses = gtc.drive()
    rec = gtc.drive_reference(mode)
    assert len(rec) == gtc.DRIVE_SCANS and all(len(c) == 4800 for c in clouds)
    worst = [0.0, 0.0]
    for i, r in enumerate(rec):
        dist, dyaw = grc.pose_error(r["transform"], poses[i])
        print(mode, i, dist, dyaw, int(r["match"]["k"]), int(r["match"]["u"]), int(r["match"]["v"]), int(r["refine"]["evaluations"]))
        worst = [max(worst[0], dist), max(worst[1], dyaw)]
        assert dist < grc.E2E_LIMIT_M and dyaw < grc.E2E_LIMIT_RAD, (i, dist, dyaw)
        assert r["flags"] == 0 and r["match"]["status"] == 0
    print(mode, "worst", worst)
    assert rec[0]["start"].tobytes() == gc.matrices(poses[:1])[0].tobytes()        # scan 0 is matched from the reset pose bit for bit
    assert abs(gt.det(rec[-1]["transform"]) - 1.0) < 1e-13


def test_the_renormalisation_is_load_bearing():
    """a local copy of the loop with the renormalisation left out (the identity in its place): after 10 scans of the drive the
    determinant is more than 1e-6 away from 1 (a prototype: 1 + 6.6e-5, and growing), because match turns the prior by fp32-rounded (c, s)
    and the chain inv, mul compounds it; with the step it stays within 1e-13"""
    _, T, p, clouds, _ = gtc.drive()
    L = gtc.drive_plane(0)
    st = gt.State(T[0])
    for xy in clouds[:10]:
        gt.step(L, xy, st, p, gt.params(), renormalise=lambda t: [np.float64(v) for v in t])
    print("det without renorm", gt.det(st.P))
    assert abs(gt.det(st.P) - 1.0) > 1e-6
    assert abs(gt.det(gtc.drive_reference(0)[9]["transform"]) - 1.0) < 1e-13


def _lost_case():
    rng = np.random.default_rng(7)
    p = gc.small_params(64, 64)
    L = gxc.plane(77, p)
    pose = gtc.reset_poses(p)[:1]
    return L, gtc.sequence(rng, [200, 200, 200, 200, 200], p, shrink=0.5), pose, p


def test_an_empty_cloud_is_lost_and_the_next_scan_continues():
    """an empty cloud in mid-sequence: the match is EMPTY, so the scan is LOST with P = start (the prediction), M unchanged, a zero
    refine record; the scan after it is predicted with the same motion and tracked"""
    L, seq, pose, p = _lost_case()
    seq[2] = np.zeros((0, 2), dtype=np.float32)
    st = gt.State(pose[0])
    tp = gt.params()
    recs = []
    for i, xy in enumerate(seq):
        before = st.copy()
        recs.append(gt.step(L, xy, st, p, tp))
        if i == 2:
            assert recs[-1]["flags"] == gt.LOST and recs[-1]["match"]["status"] == gt.gx.STATUS_EMPTY
            assert np.array(st.P).tobytes() == recs[-1]["start"].tobytes() == np.array(gt.renorm(gt.mul(before.P, before.M))).tobytes()
            assert np.array(st.M).tobytes() == np.array(before.M).tobytes() and st.n == 3
            assert recs[-1]["refine"].tobytes() == bytes(152) and recs[-1]["transform"].tobytes() == recs[-1]["start"].tobytes()
    assert [int(r["flags"]) for r in recs] == [0, 0, gt.LOST, 0, 0]
    assert recs[3]["start"].tobytes() == np.array(gt.renorm(gt.mul(recs[2]["transform"], gt.mul(gt.inv(recs[0]["transform"]), recs[1]["transform"])))).tobytes()


def test_a_min_score_above_the_best_score_is_lost():
    """min_score above what 200 points can score: every scan is LOST although its match found something, and dead-reckons with the
    identity motion (no motion was ever composed).  At the first scan's own score that scan is tracked as without a min_score"""
    L, seq, pose, p = _lost_case()
    free = gtc.reference(L, [seq], pose, p, gt.params())[0]
    recs, st = gtc.reference(L, [seq], pose, p, gt.params(min_score=200 * 255 + 1))
    assert (recs["flags"] == gt.LOST).all() and (recs["match"]["status"] == 0).all() and (recs["match"]["score"] > 0).all()
    assert all(r["refine"].tobytes() == bytes(152) and r["transform"].tobytes() == r["start"].tobytes() for r in recs)
    assert recs[0]["start"].tobytes() == pose[0].tobytes()
    for i in range(1, len(recs)):
        assert recs[i]["start"].tobytes() == np.array(gt.renorm(gt.mul(recs[i - 1]["transform"], gt.IDENTITY))).tobytes()
        assert np.allclose(recs[i]["transform"], pose[0], rtol=0, atol=1e-5)
    assert np.array(st[0].M).tobytes() == np.array(gt.IDENTITY).tobytes() and st[0].n == 5
    # at the best score itself the scans that reach it are tracked
    recs, _ = gtc.reference(L, [seq], pose, p, gt.params(min_score=int(free["match"]["score"][0])))
    assert recs[0]["flags"] == 0 and recs[0].tobytes() == free[0].tobytes()


def test_the_restatement_does_not_depend_on_the_cut():
    """one push, one scan per push, a cut after scan 0, and sequences side by side or alone: the same records"""
    L, seqs, poses, p = gtc.distinct_sequences()
    whole = gtc.distinct_reference()
    tp = gt.params()
    for q in (0, 2, 4):
        for cuts in ([1] * len(seqs[q]), [1, len(seqs[q]) - 1]):
            st, got, at = gtc.states(poses[q:q + 1]), [], 0
            for n in cuts:
                got.append(gt.push(L, [seqs[q][at:at + n]], st, p, tp))
                at += n
            assert np.concatenate(got).tobytes() == whole[q].tobytes(), (q, cuts)
    assert len(whole[1]) == 0 and [len(w) for w in whole] == gtc.SCANS
