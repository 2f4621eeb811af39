"""Case builders shared by the tracker tests (tests/test_gridtrack_restatement.py, tests/test_gpu_gridtrack.py): planes, clouds, reset
poses and the parameters as dicts of tests/gridmap_np.py and tests/gridtrack_np.py.  The maps, clouds and border priors are those of
tests/gridmatch_cases.py; a reference is computed once per case and shared (functools.lru_cache): nobody writes into it."""
import functools
import importlib

import numpy as np

import gridmap_cases as gc
import gridmap_np as gm
import gridmatch_cases as gxc
import gridmatch_np as gx
import gridtrack_np as gt
import kstrongest_np as ks

SIZES = gxc.SIZES
N_POINTS = [0, 1, 63, 64, 65, 255, 256, 257, 300, 8192]     # the slot-part boundaries, the 256-partial boundary, the cap
WINDOWS = [(0, 0, 0), (1, 3, 0), (2, 2, 2), (8, 8, 8)]      # (K, U, V)


def window(K, U, V, **kw):
    return gt.params(angle_steps=K, x_cells=U, y_cells=V, angle_step=0.013, **kw)


def skewed(priors):
    """the poses with their rotation parts scaled by 1 - 8e-6 .. 1 + 8e-6: finite, and not exactly orthonormal"""
    out = np.array(priors, dtype=np.float64).reshape(-1, 6).copy()
    for i in range(len(out)):
        out[i, [0, 1, 3, 4]] *= 1.0 + 2e-6 * ((i % 9) - 4)
    return out


def reset_poses(p):
    """gxc.border_priors (in, on and outside every border), skewed"""
    _, priors = gxc.border_priors(p)
    return skewed(priors)


def with_non_finite(pts, rng):
    """a copy with a NaN or an infinity in about one point of sixteen"""
    pts = pts.copy()
    if len(pts) > 3:
        idx = rng.choice(len(pts), size=max(1, len(pts) // 16), replace=False)
        bad = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)
        pts[idx, rng.integers(0, 2, len(idx))] = bad[rng.integers(0, 3, len(idx))]
    return pts


def sequence(rng, sizes, p, shrink=1.0):
    """one sequence's scans: clouds of the given sizes (gxc.cloud), shrunk towards the sensor"""
    return [(gxc.cloud(rng, n, p) * np.float32(shrink)).astype(np.float32) for n in sizes]


def states(poses):
    return [gt.State(t) for t in poses]


def reference(L, clouds_per_sequence, poses, p, tp, device_entry=False, **hooks):
    """-> (records of one push of everything, the states after it)"""
    st = states(poses)
    return gt.push(L, clouds_per_sequence, st, p, tp, device_entry=device_entry, **hooks), st


def split(records, clouds_per_sequence):
    """the records of a push, per sequence"""
    out, at = [], 0
    for seq in clouds_per_sequence:
        out.append(records[at:at + len(seq)])
        at += len(seq)
    return out


# ---- cloud sizes ----

@functools.lru_cache(maxsize=None)
def sizes_case(width, height):
    """a sequence of two scans for every N of N_POINTS, from the middle of the map, with non-finite points in the second scan
    -> L, clouds_per_sequence, poses, p"""
    rng = np.random.default_rng(4000 + width)
    p = gc.small_params(width, height)
    poses = skewed(np.repeat(gxc.border_priors(p)[1][:1], len(N_POINTS), axis=0))
    seqs = []
    for n in N_POINTS:
        a, b = sequence(rng, [n, n], p, shrink=0.6)
        seqs.append([a, with_non_finite(b, rng)])
    return gxc.plane(5000 + width, p), seqs, poses, p


@functools.lru_cache(maxsize=None)
def sizes_reference(width, height):
    L, seqs, poses, p = sizes_case(width, height)
    return reference(L, seqs, poses, p, gt.params())[0]


# ---- windows and predict ----

@functools.lru_cache(maxsize=None)
def window_case(K):
    """three sequences of three scans of 300, 65 and 257 points; with the largest window a fourth of one scan at the cap of points, which
    fills the volume's 4913 words from 8192 cells -> L, clouds_per_sequence, poses, p"""
    rng = np.random.default_rng(4100 + K)
    p = gc.small_params(64, 64)
    seqs = [sequence(rng, [300, 65, 257], p, shrink=0.5) for _ in range(3)]
    if K == 8:
        seqs.append(sequence(rng, [8192], p, shrink=0.5))
    poses = reset_poses(p)[[0, 1, 4, 0][:len(seqs)]]
    return gxc.plane(5100, p), seqs, poses, p


# ---- reset poses ----

@functools.lru_cache(maxsize=None)
def border_case(width, height):
    """one sequence of three scans of 300 points from every reset pose -> L, clouds_per_sequence, poses, p"""
    rng = np.random.default_rng(4200 + width)
    p = gc.small_params(width, height)
    poses = reset_poses(p)
    return gxc.plane(5200 + width, p), [sequence(rng, [300, 300, 300], p) for _ in poses], poses, p


@functools.lru_cache(maxsize=None)
def border_reference(width, height):
    L, seqs, poses, p = border_case(width, height)
    return reference(L, seqs, poses, p, gt.params())[0]


# ---- sequences side by side, and cuts ----

N_DISTINCT = 7
SCANS = [5, 0, 3, 1, 4, 2, 5]      # of distinct sequence i


@functools.lru_cache(maxsize=None)
def distinct_sequences():
    """seven sequences of 5, 0, 3, 1, 4, 2 and 5 scans of 40 .. 300 points on the 192 x 128 map -> L, clouds_per_sequence, poses, p"""
    rng = np.random.default_rng(4300)
    p = gc.small_params(192, 128)
    seqs = [sequence(rng, [int(v) for v in rng.integers(40, 301, n)], p, shrink=0.5) for n in SCANS]
    poses = reset_poses(p)[[0, 1, 2, 3, 4, 0, 2]]
    return gxc.plane(5300, p), seqs, poses, p


@functools.lru_cache(maxsize=None)
def distinct_reference():
    L, seqs, poses, p = distinct_sequences()
    return split(reference(L, seqs, poses, p, gt.params())[0], seqs)


def side_by_side(n_sequences):
    """n_sequences sequences: sequence q is distinct sequence (3 q + 2) % 7, so that equal inputs sit at different indices
    -> L, clouds_per_sequence, poses, p, records per sequence (the reference)"""
    L, seqs, poses, p = distinct_sequences()
    ref = distinct_reference()
    pick = [(3 * q + 2) % N_DISTINCT for q in range(n_sequences)]
    return L, [seqs[i] for i in pick], poses[pick], p, [ref[i] for i in pick]


# ---- the drive: tests/gridmatch_cases.end_to_end's scene, sixteen scans long ----

DRIVE_SCANS, DRIVE_MAP_SCANS = 16, [0, 3, 6, 9, 12, 15]


@functools.lru_cache(maxsize=None)
def drive():
    """synth.polar_sequence(11, 16); a map of 384 x 384 cells of 1 m centred on the floor of the mean position, range_halfwidth 8, to be
    built from scans 0, 3, .., 15 at their true poses; the clouds: the default k-strongest targets of every scan (4800 points) at
    (bin + 0.5) 0.0595 along 2 pi row / 400, fp64 rounded to fp32 -> imgs, transforms (16, 6), p, clouds, poses (16, 3)"""
    synth = importlib.import_module("navtech_radar_slam_amd.synth")
    imgs, _, poses, _ = synth.polar_sequence(11, DRIVE_SCANS)
    centre = poses[:, :2].mean(axis=0)
    p = gc.gm.params(width=384, height=384, resolution=1.0, origin_x=float(np.floor(centre[0])) - 192.0, origin_y=float(np.floor(centre[1])) - 192.0,
                     range_halfwidth=8)
    clouds = []
    for img in imgs:
        tg = ks.extract(img, col_offset=11)
        rho = (tg[:, 1].astype(np.float64) + 0.5) * 0.0595
        phi = tg[:, 0].astype(np.float64) * 2.0 * np.pi / 400.0
        clouds.append(np.stack([rho * np.cos(phi), rho * np.sin(phi)], axis=1).astype(np.float32))
    return imgs, gc.matrices(poses), p, clouds, poses


@functools.lru_cache(maxsize=None)
def drive_planes():
    imgs, T, p, _, _ = drive()
    return gm.add_batch(gm.zeros(p), imgs[DRIVE_MAP_SCANS], T[DRIVE_MAP_SCANS], p, col_offset=gc.META)


@functools.lru_cache(maxsize=None)
def drive_plane(mode):
    """the likelihood plane: the mean (0) or the hits (1) of the drive's map"""
    return gx.likelihood(drive_planes(), mode)


@functools.lru_cache(maxsize=None)
def drive_reference(mode):
    """the drive tracked from scan 0's true pose with the default parameters -> records (16,)"""
    _, T, p, clouds, _ = drive()
    return reference(drive_plane(mode), [clouds], T[:1], p, gt.params())[0]
