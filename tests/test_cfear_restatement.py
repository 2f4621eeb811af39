"""tests/cfear_np.py, the arithmetic contract of csrc/cfear.hip, against what it must mean: geometry on crafted clouds, an exact
rigid motion recovered, and CFEAR's chain (k-strongest keypoints -> surface points -> point-to-line registration) on the
synthetic drive against the true poses.  CPU only.

Measured with this file on synth.polar_sequence(11, 4), k-strongest k = 12, z_min = 60, min_separation = 0, the defaults of
cfear_np (radius 3.5, min_points 6, max_condition 1e5, 30 deg, Huber 0.1, identity start): 4800 keypoints per scan, 624 / 632 /
628 / 628 surface points, at most 69 neighbours; the three pairs: 505 / 496 / 522 correspondences, 18 / 15 / 17 iterations,
every status 0, errors 0.032 m 1.2e-4 rad / 0.012 m 4.8e-4 rad / 0.012 m 5.1e-5 rad (worst 0.032 m / 4.8e-4 rad; the bounds are
those test_gpu_odometry.py holds cen2019 to, 0.25 m / 1e-2 rad), smallest decision margin 2.5e-8.
PARITY UNPINNED w.r.t. CFEAR's own code, which is not in the reference checkout."""
import math
import os
import sys

import numpy as np
import pytest

from navtech_radar_slam_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cfear_np as cf  # noqa: E402
import kstrongest_np as ksn  # noqa: E402


def test_wall_normals_are_perpendicular_and_face_the_origin():
    # four walls of a room around the sensor, a few centimetres thick (an exactly straight wall has lambda_min = 0: see below)
    for wall in range(4):
        th = wall * math.pi / 2
        pts = []
        for i in range(60):
            along, off = -3.0 + 0.1 * i, 10.0 + 0.02 * ((i * 7) % 5 - 2)
            pts.append((math.cos(th) * off - math.sin(th) * along, math.sin(th) * off + math.cos(th) * along))
        rec, status = cf.surface_points(np.array(pts, dtype=np.float32))
        assert status == 0 and len(rec) >= 1
        for r in rec:
            n = np.array([r["nx"], r["ny"]], dtype=np.float64)
            assert abs(np.linalg.norm(n) - 1.0) < 1e-6
            assert abs(n @ np.array([-math.sin(th), math.cos(th)])) < 0.05, (wall, r)   # perpendicular to the wall
            assert n @ np.array([r["x"], r["y"]], dtype=np.float64) < 0                  # faces the origin
            assert r["lambda_max"] > 100 * r["lambda_min"] > 0


def _blob(n):
    return np.array([(5.2 + 0.3 * (i % 3) + 0.01 * i, 8.1 + 0.25 * (i // 3)) for i in range(n)], dtype=np.float32)


def test_min_points_is_the_threshold():
    rec, _ = cf.surface_points(_blob(5))
    assert len(rec) == 0
    rec, _ = cf.surface_points(_blob(6))
    assert len(rec) == 1 and rec["n_points"][0] == 6
    rec, _ = cf.surface_points(_blob(6), min_points=7)
    assert len(rec) == 0


def test_exactly_collinear_points_are_rejected():
    for pts in ([(0.25 * i, 2.0) for i in range(8)], [(4.0 + 0.125 * i, 4.0 + 0.125 * i) for i in range(8)],
                [(1.5, 1.5)] * 8):  # (and eight copies of one point)
        rec, status = cf.surface_points(np.array(pts, dtype=np.float32))
        assert len(rec) == 0 and status == 0


def test_out_of_grid_and_non_finite_points_set_the_status_bit():
    pts = np.concatenate([_blob(6), np.array([(300.0, 0.0), (np.nan, 1.0), (0.0, -np.inf)], dtype=np.float32)])
    rec, status = cf.surface_points(pts)
    alone, _ = cf.surface_points(_blob(6))
    assert status == cf.STATUS_RANGE and rec.tobytes() == alone.tobytes()


SP64 = np.dtype([("x", "<f8"), ("y", "<f8"), ("nx", "<f8"), ("ny", "<f8")])


def _room():
    """surface points of a room with two oblique walls, fp64 (so that a rigid motion of them is exact to rounding)"""
    out = []
    for th, off in ((0.0, 12.0), (math.pi / 2, 9.0), (math.pi, 14.0), (-math.pi / 2, 11.0), (0.7, 20.0), (2.4, 17.0)):
        for i in range(9):
            along = -8.0 + 2.0 * i
            out.append((math.cos(th) * off - math.sin(th) * along, math.sin(th) * off + math.cos(th) * along, -math.cos(th), -math.sin(th)))
    return np.array(out, dtype=SP64)


def test_noise_free_rigid_motion_is_recovered():
    src = _room()
    for pose in ((0.4, -0.3, 0.02), (-0.8, 0.5, -0.05), (0.0, 0.0, 0.0)):
        dst = cf.transform(src, pose)
        res = cf.register(src, dst)
        assert res["status"] == 0 and res["correspondences"] == len(src)
        assert max(abs(res["x"] - pose[0]), abs(res["y"] - pose[1]), abs(res["yaw"] - pose[2])) < 1e-9, res
        # the cost is that of the LAST linearisation, one step (< step_epsilon = 1e-6) from the end: residuals below 1e-6 x (1 + a
        # lever of 25 m), 54 of them
        assert res["cost"] < 54 * 0.5 * 2.6e-5 ** 2


def test_statuses():
    src = _room()
    assert cf.register(src[:0], src)["status"] == 1 and cf.register(src, src[:0])["status"] == 1
    big = np.zeros(cf.MAX_SURFACE_POINTS + 1, dtype=SP64)
    assert cf.register(big, src)["status"] == 2
    far = cf.transform(src, (100.0, 0.0, 0.0))
    res = cf.register(src, far, init=(0.5, 0.25, 0.125))
    assert res["status"] == 4 and (res["x"], res["y"], res["yaw"], res["iterations"]) == (0.5, 0.25, 0.125, 0)
    flat = src.copy()
    flat["nx"], flat["ny"] = 1.0, 0.0
    assert cf.register(flat, flat)["status"] == 5
    res = cf.register(src, cf.transform(src, (0.4, -0.3, 0.02)), max_iterations=2)
    assert res["status"] == 8 and res["iterations"] == 2


@pytest.fixture(scope="module")
def drive(oracle):
    imgs, az, poses, _ = synth.polar_sequence(11, 4)
    recs, n_kp = [], []
    for i in range(4):
        tg = ksn.extract(imgs[i], k=12, z_min=60, min_separation=0)
        rec, status = cf.surface_points(ksn.to_cartesian(tg, az[i] if np.ndim(az) == 2 else az, synth.RADAR_RESOLUTION))
        assert status == 0
        recs.append(rec)
        n_kp.append(len(tg))
    return recs, n_kp, poses


def test_synthetic_drive_registers_within_the_odometry_bounds(drive, oracle):
    recs, n_kp, poses = drive
    print(f"keypoints {n_kp}, surface points {[len(r) for r in recs]}, most neighbours {max(int(r['n_points'].max()) for r in recs)}")
    assert n_kp == [4800] * 4 and all(500 < len(r) <= cf.MAX_SURFACE_POINTS for r in recs)
    margin = math.inf
    for i in range(1, 4):
        res = cf.register(recs[i], recs[i - 1])
        truth = synth.relative_pose(poses[i - 1], poses[i])
        et, ey = float(np.hypot(res["x"] - truth[0], res["y"] - truth[1])), abs(float(res["yaw"] - truth[2]))
        print(f"pair {i}: {res['correspondences']} correspondences, {res['iterations']} iterations, status {res['status']}, "
              f"{et:.3f} m {ey:.1e} rad, margin {res['margin']:.1e}")
        assert res["status"] == 0
        assert et < 0.25 and ey < 1e-2
        margin = min(margin, res["margin"])
    assert margin > 1e-9  # what tests/test_gpu_cfear.py relies on: no pair of this drive is left out of the comparison
