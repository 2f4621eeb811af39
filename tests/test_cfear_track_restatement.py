"""tests/cfear_track_np.py, the arithmetic contract of csrc/cfear_track.hip, against what it must mean.  CPU only.

Measured with this file (k-strongest k = 12, z_min = 60, min_separation = 0, the defaults of cfear_np and cfear_track_np):
  synth.polar_sequence(11, 6): keyframes at scans 0, 2, 4, a ring of 3 at scan 5, every status 0, 518 / 499 / 994 / 920 / 1422
    correspondences, absolute error at most 0.030 m, smallest decision margin 8.6e-9
  the small sequence (keyframe_distance 0.5): 23 - 29 records a scan, keyframes at 0, 2, 4, 5, 7 (the ring is full at 4 and evicts at
    5 and 7), every status 0, smallest margin 1.0e-7; with 1 keyframe, thresholds 0, no prediction: one status 8 (scan 3), 2.1e-7
PARITY UNPINNED w.r.t. CFEAR's own code, which is not in the reference checkout."""
import math
import os
import sys

import numpy as np

from navtech_radar_slam_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cfear_np as cf  # noqa: E402
import cfear_track_cases as cases  # noqa: E402
import cfear_track_np as ct  # noqa: E402


def test_compose_and_between_are_inverse_to_rounding():
    a, b = (3.0, -2.0, 0.7), (0.5, 0.25, -0.2)
    assert max(abs(u - v) for u, v in zip(ct.between(a, ct.compose(a, b)), b)) < 1e-15
    assert ct.compose((1.0, 2.0, math.pi / 2), (1.0, 0.0, 0.0))[:2] == (1.0 + (math.cos(math.pi / 2) * 1.0 - 0.0), 3.0)


def test_room_seen_from_three_poses_is_recovered_with_two_keyframes():
    views = cases.room_views()
    res = ct.register_keyframes(views[2], views[:2], cases.ROOM_POSES[:2], init=cases.ROOM_POSES[1])
    assert res["status"] == 0 and res["correspondences"] == 2 * len(views[2])
    assert max(abs(res[f] - w) for f, w in zip(("x", "y", "yaw"), cases.ROOM_POSES[2])) < 1e-9, res
    # K = 1 at the identity pose is the pair rule, bit for bit
    one = ct.register_keyframes(views[1], views[:1], [(0.0, 0.0, 0.0)])
    pair = cf.register(views[1], views[0])
    assert all(one[f] == pair[f] for f in ("x", "y", "yaw", "cost", "iterations", "correspondences", "status", "margin")), (one, pair)


def test_statuses_of_the_joint_registration():
    for job, want in zip(cases.joint_jobs(), cases.joint_wants()):
        assert want["status"] == job[5], (job[0], want)
        if job[5] in (1, 2, 4):
            assert (want["x"], want["y"], want["yaw"], want["iterations"]) == tuple(job[4]) + (0,), job[0]
    empty = cases.joint_wants()[3]
    full = cases.joint_wants()[2]
    assert all(empty[f] == full[f] for f in ("x", "y", "yaw", "cost", "correspondences"))  # an empty keyframe is skipped
    room = cases.as_records(cases.room64())
    assert ct.register_keyframes(room[:0], [room], [(0.0, 0.0, 0.0)])["status"] == 1


def test_keyframe_flags_and_ring_sizes_on_a_crafted_motion():
    tr = ct.track(cases.crafted_scans(), n_keyframes=2)
    assert tuple(r["keyframe"] for r in tr) == cases.CRAFTED_FLAGS
    assert tuple(r["n_keyframes"] for r in tr) == cases.CRAFTED_USED
    for r, p in zip(tr, cases.CRAFTED_POSES):  # (float32 records of an exact motion: 1e-5 m is their rounding at 25 m)
        assert r["reg"]["status"] == 0 and max(abs(r["x"] - p[0]), abs(r["y"] - p[1]), abs(r["yaw"] - p[2])) < 1e-5, (r, p)
    assert tr[0]["reg"] == dict(x=0.0, y=0.0, yaw=0.0, cost=0.0, iterations=0, correspondences=0, status=0, margin=math.inf)
    assert min(r["margin"] for r in tr) >= 1e-9


def test_a_scan_100_m_away_re_anchors():
    scans = cases.crafted_scans()[:3]
    far = cases.as_records(cases.seen_from(cases.room64(), (100.0, 0.0, 0.0)))
    tr = ct.track(scans + [far, far, cf.transform(far, (-0.2, 0.0, 0.0))[:0]])
    assert [r["keyframe"] for r in tr] == [1, 0, 0, 2, 0, 0] and [r["n_keyframes"] for r in tr] == [0, 1, 1, 1, 1, 1]
    assert tr[3]["reg"]["status"] == 4 and tr[4]["reg"]["status"] == 0 and tr[5]["reg"]["status"] == 1
    start = ct.compose((tr[2]["x"], tr[2]["y"], tr[2]["yaw"]), ct.between((tr[1]["x"], tr[1]["y"], tr[1]["yaw"]), (tr[2]["x"], tr[2]["y"], tr[2]["yaw"])))
    assert (tr[3]["x"], tr[3]["y"], tr[3]["yaw"]) == start  # P = the prediction, and the ring is this scan there
    assert max(abs(tr[4][f] - tr[3][f]) for f in ("x", "y", "yaw")) < 1e-6  # the same scan again: registered to itself
    assert (tr[5]["x"], tr[5]["y"], tr[5]["yaw"]) == ct.compose((tr[4]["x"], tr[4]["y"], tr[4]["yaw"]), ct.between(
        (tr[3]["x"], tr[3]["y"], tr[3]["yaw"]), (tr[4]["x"], tr[4]["y"], tr[4]["yaw"])))  # an empty scan: the prediction, flag 0


def test_drive_track_is_what_the_gpu_tests_rely_on():
    recs, poses = cases.drive()
    tr = cases.drive_track()
    assert [r["keyframe"] for r in tr] == [1, 0, 1, 0, 1, 0] and [r["n_keyframes"] for r in tr] == [0, 1, 1, 2, 2, 3]
    assert all(r["reg"]["status"] == 0 for r in tr) and tr[5]["reg"]["correspondences"] == 1422
    for i, r in enumerate(tr):
        truth = synth.relative_pose(poses[0], poses[i])
        print(f"scan {i}: {r['reg']['correspondences']} correspondences, {r['reg']['iterations']} iterations, margin {r['margin']:.1e}, "
              f"{math.hypot(r['x'] - truth[0], r['y'] - truth[1]):.3f} m off")
        assert math.hypot(r["x"] - truth[0], r["y"] - truth[1]) <= 0.03
        if i:
            p, q = tr[i - 1], r
            rel = ct.between((p["x"], p["y"], p["yaw"]), (q["x"], q["y"], q["yaw"]))
            t = synth.relative_pose(poses[i - 1], poses[i])
            assert math.hypot(rel[0] - t[0], rel[1] - t[1]) < 0.25 and abs(rel[2] - t[2]) < 1e-2
    assert min(r["margin"] for r in tr) >= 1e-9
    assert min(w["margin"] for w in cases.joint_wants()) >= 1e-9


def test_small_sequence_fills_and_evicts_the_ring():
    recs, _ = cases.small()
    assert all(23 <= len(r) <= 29 for r in recs)
    tr = cases.small_track()
    assert [r["keyframe"] for r in tr] == [1, 0, 1, 0, 1, 1, 0, 1] and [r["n_keyframes"] for r in tr] == [0, 1, 1, 2, 2, 3, 3, 3]
    assert min(r["margin"] for r in tr) >= 1e-9


def test_one_keyframe_without_thresholds_or_prediction_is_the_pair_rule():
    """Every scan is a keyframe and the start is the previous pose, so scan i is registered to scan i - 1 alone from the relative pose
    (0, 0, 0): cfear_np.register on the pair, in the map frame instead of scan i - 1's.  Gauss-Newton does not depend on a rigid change
    of the frame (the parameters change linearly, the step's norm is kept), so the two differ by rounding alone: 1e-16 x coordinates of
    50 m, through the 3 x 3 solve, per iteration -- 1e-9 leaves three orders of magnitude; counts and statuses are equal."""
    recs, _ = cases.small()
    tr = cases.small_pairs_track()
    assert all(r["keyframe"] == 1 for r in tr) and [r["reg"]["status"] for r in tr].count(8) == 1
    assert min(r["margin"] for r in tr) >= 1e-9
    for i in range(1, len(recs)):
        pair = cf.register(recs[i], recs[i - 1])
        rel = ct.between((tr[i - 1]["x"], tr[i - 1]["y"], tr[i - 1]["yaw"]), (tr[i]["x"], tr[i]["y"], tr[i]["yaw"]))
        d = max(abs(rel[0] - pair["x"]), abs(rel[1] - pair["y"]), abs(rel[2] - pair["yaw"]), abs(tr[i]["reg"]["cost"] - pair["cost"]))
        print(f"pair {i}: status {pair['status']}, {pair['iterations']} iterations, |tracker - pair| {d:.1e}")
        assert all(tr[i]["reg"][f] == pair[f] for f in ("status", "iterations", "correspondences")), (i, tr[i]["reg"], pair)
        assert d < 1e-9
