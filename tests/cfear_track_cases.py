"""Inputs shared by the CFEAR tracking tests (tests/test_cfear_track_restatement.py, tests/test_gpu_cfear_track.py,
tests/test_gpu_odometry_cfear_track.py, tests/test_gpu_cfear_pair_pin.py and its recorder tools/make_cfear_pairs_golden.py): surface points of the synthetic sequences through the CPU chain k-strongest ->
cfear_np.surface_points, the room of test_cfear_restatement.py as records, and the restatement's tracks.  Everything is
computed once per process (functools.lru_cache) and must be left unchanged by its users."""
import functools
import math
import os
import sys

import numpy as np

from navtech_radar_slam_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cfear_np as cf  # noqa: E402
import cfear_track_np as ct  # noqa: E402
import kstrongest_np as ksn  # noqa: E402

SP64 = np.dtype([("x", "<f8"), ("y", "<f8"), ("nx", "<f8"), ("ny", "<f8")])
SMALL_TRACK = dict(keyframe_distance=0.5)  # the ring fills and evicts within the 8 scans of small()


def as_records(a):
    out = np.zeros(len(a), dtype=cf.SP_DTYPE)
    for f in ("x", "y", "nx", "ny"):
        out[f] = a[f]
    out["lambda_max"], out["lambda_min"], out["n_points"] = 1.0, 0.5, 6
    return out


def room64():
    """surface points of a room with two oblique walls, fp64 (a rigid motion of them is exact to rounding)"""
    out = []
    for th, off in ((0.0, 12.0), (math.pi / 2, 9.0), (math.pi, 14.0), (-math.pi / 2, 11.0), (0.7, 20.0), (2.4, 17.0)):
        for i in range(9):
            along = -8.0 + 2.0 * i
            out.append((math.cos(th) * off - math.sin(th) * along, math.sin(th) * off + math.cos(th) * along, -math.cos(th), -math.sin(th)))
    return np.array(out, dtype=SP64)


def seen_from(rec, pose):
    """records given in the map frame as a sensor at `pose` sees them: p' = R(-yaw) (p - t)"""
    x, y, yaw = pose
    c, s = math.cos(yaw), math.sin(yaw)
    out = rec.copy()
    px, py = rec["x"].astype(np.float64) - x, rec["y"].astype(np.float64) - y
    nx, ny = rec["nx"].astype(np.float64), rec["ny"].astype(np.float64)
    out["x"], out["y"] = c * px + s * py, c * py - s * px
    out["nx"], out["ny"] = c * nx + s * ny, c * ny - s * nx
    return out


def _chain(imgs, az, n):
    out = []
    for i in range(n):
        tg = ksn.extract(imgs[i], k=12, z_min=60, min_separation=0)
        rec, status = cf.surface_points(ksn.to_cartesian(tg, az[i] if np.ndim(az) == 2 else az, synth.RADAR_RESOLUTION))
        assert status == 0
        out.append(rec)
    return out


@functools.lru_cache(maxsize=None)
def drive_images(n=6):
    return synth.polar_sequence(11, n)


@functools.lru_cache(maxsize=None)
def drive(n=6):
    """-> (records of the n scans of the synthetic drive, true poses)"""
    imgs, az, poses, _ = drive_images(n)
    return _chain(imgs, az, n), poses


@functools.lru_cache(maxsize=None)
def small():
    """-> (records of the 8 scans of the small sequence, true poses)"""
    imgs, az, poses, _ = synth.polar_sequence(3, 8, rows=64, cols=512, n_buildings=120, n_poles=200, world_radius=40.0)
    return _chain(imgs, az, 8), poses


@functools.lru_cache(maxsize=None)
def drive_track():
    return ct.track(drive()[0])


@functools.lru_cache(maxsize=None)
def small_track():
    return ct.track(small()[0], **SMALL_TRACK)


@functools.lru_cache(maxsize=None)
def small_pairs_track():
    return ct.track(small()[0], n_keyframes=1, keyframe_distance=0.0, keyframe_rotation=0.0, predict=0)


@functools.lru_cache(maxsize=None)
def pair_cases():
    """the pairs of tests/test_gpu_cfear.py: (name, src, dst, init, parameter overrides, expected status)"""
    recs = drive()[0]
    room = as_records(room64())
    flat = room.copy()
    flat["nx"], flat["ny"] = 1.0, 0.0
    over = np.zeros(cf.MAX_SURFACE_POINTS + 1, dtype=cf.SP_DTYPE)
    over["nx"] = 1.0
    return tuple((f"drive pair {i}", recs[i], recs[i - 1], None, {}, 0) for i in (1, 2, 3)) + (
        ("identical sets", recs[0], recs[0], None, {}, 0),
        ("room moved", room, cf.transform(room, (0.4, -0.3, 0.02)), None, {}, 0),
        ("non-identity init", recs[1], recs[0], (0.9, 0.1, 0.05), {}, 0),
        ("100 m apart", room, cf.transform(room, (100.0, 0.0, 0.0)), (0.5, 0.25, 0.125), {}, 4),
        ("normals (1, 0)", flat, flat, None, {}, 5),
        ("two iterations", recs[1], recs[0], None, {"max_iterations": 2}, 8),
        ("empty src", room[:0], room, (1.0, 2.0, 0.5), {}, 1),
        ("empty dst", room, room[:0], None, {}, 1),
        ("src over the cap", over, room, (1.0, 2.0, 0.5), {}, 2),
        ("dst at the cap", room, over[:-1], None, {}, 4),
    )


def pair_groups():
    """pair_cases() grouped by their parameter overrides, in first-seen order: [(sorted override items, cases, inits (n, 3))]"""
    by_params = {}
    for c in pair_cases():
        by_params.setdefault(tuple(sorted(c[4].items())), []).append(c)
    return [(key, cs, np.array([c[3] if c[3] is not None else (0.0, 0.0, 0.0) for c in cs])) for key, cs in by_params.items()]


ROOM_POSES = ((0.0, 0.0, 0.0), (0.9, -0.4, 0.03), (1.7, -0.6, 0.07))  # two keyframes and the scan


def room_views():
    """the room seen from ROOM_POSES, fp64 (tests of the restatement) """
    return [seen_from(room64(), p) for p in ROOM_POSES]


@functools.lru_cache(maxsize=None)
def joint_jobs():
    """(name, src, keyframes, poses, init, expected status) of the joint registrations compared with the restatement"""
    recs, _ = drive()
    tr = drive_track()
    pose = [(r["x"], r["y"], r["yaw"]) for r in tr]
    views = [as_records(v) for v in room_views()]
    room = as_records(room64())
    over = np.zeros(cf.MAX_SURFACE_POINTS + 1, dtype=cf.SP_DTYPE)
    over["nx"] = 1.0
    return (
        ("drive K = 2", recs[3], (recs[0], recs[2]), (pose[0], pose[2]), pose[2], 0),
        ("drive K = 3", recs[5], (recs[0], recs[2], recs[4]), (pose[0], pose[2], pose[4]), pose[4], 0),
        ("room from three poses", views[2], (views[0], views[1]), ROOM_POSES[:2], ROOM_POSES[1], 0),
        ("an empty keyframe among full ones", views[2], (views[0], room[:0], views[1]), (ROOM_POSES[0], (5.0, 5.0, 1.0), ROOM_POSES[1]), ROOM_POSES[1], 0),
        ("all keyframes empty", views[2], (room[:0], room[:0]), ROOM_POSES[:2], (1.0, 2.0, 0.5), 1),
        ("a keyframe over the cap", views[2], (views[0], over), ROOM_POSES[:2], (1.0, 2.0, 0.5), 2),
        ("100 m apart", room, (cf.transform(room, (100.0, 0.0, 0.0)), cf.transform(room, (100.0, 3.0, 0.0))), ((0.0, 0.0, 0.0), (0.0, 3.0, 0.0)),
         (0.5, 0.25, 0.125), 4),
    )


@functools.lru_cache(maxsize=None)
def joint_wants():
    return tuple(ct.register_keyframes(j[1], list(j[2]), list(j[3]), init=j[4]) for j in joint_jobs())


CRAFTED_POSES = ((0.0, 0.0, 0.0), (0.6, 0.0, 0.0), (1.2, 0.0, 0.0), (1.8, 0.0, 0.0), (2.0, 0.0, 0.02), (2.1, 0.0, 0.12), (2.3, 0.1, 0.12),
                 (3.7, 0.1, 0.12))
# by hand, n_keyframes = 2, 1.5 m / 5 deg = 0.0873 rad, always against the NEWEST keyframe: scan 3 is 1.8 m from keyframe 0; scan 4 is
# 0.2 m / 0.02 rad from keyframe 3; scan 5 0.3 m but 0.12 rad; scan 6 0.22 m / 0 rad from keyframe 5; scan 7 1.6 m from it
CRAFTED_FLAGS = (1, 0, 0, 1, 0, 1, 0, 1)
CRAFTED_USED = (0, 1, 1, 1, 2, 2, 2, 2)  # the ring's size when the scan was registered


def crafted_scans():
    return [as_records(seen_from(room64(), p)) for p in CRAFTED_POSES]
