"""Inputs shared by the CFEAR motion-compensation tests (tests/test_cfear_mocomp_restatement.py, tests/test_gpu_cfear_mocomp.py,
tests/test_gpu_odometry_cfear_mocomp.py): the distorted room drives with the restatement's tracks, the crafted clouds of the timed
surface points, the small sequence's keypoints with their rows.  Everything is computed once per process (functools.lru_cache)
and must be left unchanged by its users."""
import functools
import os
import sys

import numpy as np

from navtech_radar_slam_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cfear_mocomp_np as cm  # noqa: E402
import cfear_track_cases as cases  # noqa: E402
import cfear_track_np as ct  # noqa: E402
import kstrongest_np as ksn  # noqa: E402

DRIVES = {"constant": cm.CONSTANT_DRIVE, "accelerating": cm.ACCEL_DRIVE}
SMALL_ROWS, SMALL_COLS = 64, 512


@functools.lru_cache(maxsize=None)
def drive(name):
    """-> (records per scan, tau per scan, the scans' true start poses) of the distorted room under DRIVES[name]"""
    return cm.distorted_views(cases.room64(), DRIVES[name])


@functools.lru_cache(maxsize=None)
def drive_track(name, compensate=1, **params):
    scans, taus, _ = drive(name)
    return cm.track(scans, taus, compensate=compensate, **params)


@functools.lru_cache(maxsize=None)
def small_keypoints():
    """-> per scan of cases.small()'s sequence: (xy (n, 2) float32, azimuth rows (n,) int32), and the images and azimuths"""
    imgs, az, _, _ = synth.polar_sequence(3, 8, rows=SMALL_ROWS, cols=SMALL_COLS, n_buildings=120, n_poles=200, world_radius=40.0)
    out = []
    for i in range(8):
        tg = ksn.extract(imgs[i], k=12, z_min=60, min_separation=0)
        xy = ksn.to_cartesian(tg, az[i] if np.ndim(az) == 2 else az, synth.RADAR_RESOLUTION)
        out.append((np.ascontiguousarray(xy, dtype=np.float32), np.ascontiguousarray(np.asarray(tg)[:, 0], dtype=np.int32)))
    return tuple(out), imgs, az


@functools.lru_cache(maxsize=None)
def small_timed():
    """-> (records per scan, tau per scan) of the small sequence through the restatement's timed surface points"""
    recs, taus = [], []
    for xy, rows in small_keypoints()[0]:
        rec, tau, status = cm.surface_points_timed(xy, rows, SMALL_ROWS)
        assert status == 0
        recs.append(rec)
        taus.append(tau)
    return recs, taus


@functools.lru_cache(maxsize=None)
def small_track(compensate=1):
    recs, taus = small_timed()
    return cm.track(recs, taus, compensate=compensate, **cases.SMALL_TRACK)


def seam_cloud(n_rows=401):
    """one cluster of 12 points on a wall at x = 20 m whose rows straddle the seam (rows n_rows - 3 .. n_rows - 1 and 0 .. 2), and a
    second cluster well inside the revolution; n_rows odd -> (xy, rows, n_rows)"""
    xy, rows = [], []
    for k in range(12):
        xy.append((20.0 + 0.01 * (k % 3), -1.1 + 0.2 * k))
        rows.append((n_rows - 3 + k // 2) % n_rows)
    for k in range(12):
        xy.append((-30.0 + 0.2 * k, 25.0 + 0.02 * (k % 2)))
        rows.append(150 + k // 3)
    return np.array(xy, dtype=np.float32), np.array(rows, dtype=np.int32), n_rows


def crowded_cloud(n=16384, n_rows=65536):
    """RSX_CFEAR_MAX_POINTS points in one cell, rows over the whole revolution (the integer sum of the row distances is at its
    largest) -> (xy, rows, n_rows)"""
    rng = np.random.default_rng(5)
    xy = np.stack([rng.uniform(0.2, 3.3, n), rng.uniform(0.2, 3.3, n)], axis=1).astype(np.float32)
    rows = rng.integers(0, n_rows, n).astype(np.int32)
    return xy, rows, n_rows


PASS2_MIN_CORRESPONDENCES = 60


@functools.lru_cache(maxsize=None)
def pass2_failure():
    """Two scans on which, with min_correspondences = PASS2_MIN_CORRESPONDENCES, pass 1 succeeds and only pass 2 fails -> (scans, taus,
    min_correspondences).  The first two scans of the constant drive; the second carries nine more records: copies of its records of
    the wall at x = -14 m with the normal turned by 29 deg and the time 1.  In pass 1 they correspond to the keyframe's records of
    that wall (29 deg <= 30 deg: 54 + 9 correspondences); pass 2 turns their normals by wz (1 - tau of the wall, about 0.5) = 1.7 deg
    more, past the 30 deg of cos_max_normal_angle: 54 correspondences, status 4."""
    import math
    scans, taus, _ = drive("constant")
    wall = scans[1][18:27].copy()
    c, s = math.cos(math.radians(29.0)), math.sin(math.radians(29.0))
    nx, ny = wall["nx"].astype(np.float64), wall["ny"].astype(np.float64)
    wall["nx"], wall["ny"] = c * nx - s * ny, s * nx + c * ny
    return ([scans[0], np.concatenate([scans[1], wall])], [taus[0], np.concatenate([taus[1], np.ones(9, dtype=np.float32)])],
            PASS2_MIN_CORRESPONDENCES)


@functools.lru_cache(maxsize=None)
def point_level(name):
    """the point-level study: walls -> points with rows -> timed surface points -> tracker -> (track without, track with compensation,
    records per scan)"""
    clouds, rows, _ = cm.wall_points(DRIVES[name], n_rows=400)
    recs, taus = [], []
    for c, a in zip(clouds, rows):
        r, t, status = cm.surface_points_timed(c, a, 400)
        assert status == 0
        recs.append(r)
        taus.append(t)
    return cm.track(recs, taus, compensate=0), cm.track(recs, taus, compensate=1), tuple(len(r) for r in recs)
