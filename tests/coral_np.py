"""CorAl alignment quality of a pair of clouds (Adolfsson et al., "CorAl: Introspection for robust radar and lidar perception in
diverse environments using differential entropy") restated in Python / numpy: the arithmetic contract that csrc/coral.hip
implements (include/rsx.h, rsx_coral_*).  TEST INFRASTRUCTURE ONLY.  CorAl's own code is not part of the reference checkout:
PARITY UNPINNED, this file is the definition.

One job: cloud A (n_a points, float32 x, y, A's frame), cloud B (n_b points, B's frame), T = (r00, r01, tx, r10, r11, ty) taking B
into A's frame (six doubles: a matrix, so that nothing here evaluates a sine), radius r, min_points, min_other, det_min.
  1. all arithmetic is fp64 on float32 inputs, nothing fused, every sum sequential in the order stated here
  2. the joint cloud: index i < n_a is A's point i; index n_a + k is B's point k moved, x' = (r00 bx + r01 by) + tx,
     y' = (r10 bx + r11 by) + ty, each rounded to float32 once; from there on an ordinary float32 input
  3. cell of a point: ix = floor(x / r), iy = floor(y / r); a point with ix or iy outside [-64, 64) (non-finite included) is
     ignored by everything and sets STATUS_RANGE; the others are VALID
  4. the walk of a valid point p: the 3 x 3 block of cells around p's cell, dy = -1, 0, 1 outer, dx = -1, 0, 1 inner, ascending
     joint index inside a cell, cells off the 128 x 128 grid skipped; a visited q is a neighbour iff ex ex + ey ey <= r r with
     e = q - p (p is its own neighbour).  The JOINT set: all neighbours in walk order; the SEPARATE set: those of p's own cloud
  5. pass 1: m_joint, m_sep and the coordinate sums of both sets; p is SCORED iff m_sep >= min_points and
     m_joint - m_sep >= min_other (CorAl's "overlap only")
  6. pass 2 (scored points, each set): mu = sum / m; sxx += ex ex, syy += ey ey, sxy += ex ey with e = q - mu in walk order;
     each divided by (m - 1); det = sxx syy - sxy sxy
  7. one 24-byte record per joint index: det_separate, det_joint (0.0 unless scored), m_separate, m_joint (every valid point);
     all zero for an invalid point
  8. h(det) = 0.5 log(max(det, det_min)) + (1 + log(2 pi)); h_joint, h_separate = the means of h over the scored points,
     quality = h_joint - h_separate; all three 0.0 with STATUS_EMPTY when nothing is scored.  The logarithm and the order of this
     last sum are the device's own: the only part compared with a tolerance
  9. a cloud of more than MAX_POINTS points: STATUS_POINTS, nothing computed, a zero result

The sums are taken with np.add.accumulate, which adds strictly left to right (out[i] = out[i - 1] + in[i]): the same additions as
a scalar loop.  A point that is visited but is no neighbour adds +0.0, which changes no partial sum (one that starts at +0.0 is
never -0.0).  tests/test_coral_restatement.py holds this file to a scalar double loop bit for bit."""
import math

import numpy as np

STATUS_RANGE = 1   # RSX_CORAL_STATUS_RANGE
STATUS_POINTS = 2  # RSX_CORAL_STATUS_POINTS
STATUS_EMPTY = 4   # RSX_CORAL_STATUS_EMPTY
MAX_POINTS = 8192  # RSX_CORAL_MAX_POINTS, per cloud
GRID = 128
HALF = 64

POINT_DTYPE = np.dtype([("det_separate", "<f8"), ("det_joint", "<f8"), ("m_separate", "<i4"), ("m_joint", "<i4")])
RESULT_DTYPE = np.dtype([("quality", "<f8"), ("h_joint", "<f8"), ("h_separate", "<f8"), ("n_scored", "<i4"), ("n_scored_a", "<i4"),
                         ("n_valid", "<i4"), ("status", "<i4")])
assert POINT_DTYPE.itemsize == 24 and RESULT_DTYPE.itemsize == 40

IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
H_CONST = 1.0 + math.log(2.0 * math.pi)
_ROWS = 256  # points of one cell handled at a time (bounds the temporaries at _ROWS x the block's population)


def pose_matrix(pose):
    """(x, y, yaw) -> (r00, r01, tx, r10, r11, ty), with math.cos / math.sin (what Coral.quality(poses=...) does on the host)"""
    x, y, yaw = (float(v) for v in pose)
    c, s = math.cos(yaw), math.sin(yaw)
    return (c, -s, x, s, c, y)


def joint_cloud(a, b, T=None):
    """-> (n_a + n_b, 2) float32: A, then B moved by T (rule 2)"""
    a = np.asarray(a, dtype=np.float32).reshape(-1, 2)
    b = np.asarray(b, dtype=np.float32).reshape(-1, 2)
    t = [float(v) for v in (IDENTITY if T is None else T)]
    bx, by = b[:, 0].astype(np.float64), b[:, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        mx = ((t[0] * bx + t[1] * by) + t[2]).astype(np.float32)
        my = ((t[3] * bx + t[4] * by) + t[5]).astype(np.float32)
    return np.concatenate([a, np.stack([mx, my], axis=1)]) if len(b) else a.copy()


def cells_of(xy, r):
    """-> (cell (n,) int64, -1 for a point outside the grid; valid (n,) bool) (rule 3)"""
    with np.errstate(all="ignore"):
        fx = np.floor(xy[:, 0].astype(np.float64) / r)
        fy = np.floor(xy[:, 1].astype(np.float64) / r)
        valid = (fx >= -HALF) & (fx < HALF) & (fy >= -HALF) & (fy < HALF)  # (NaN compares false)
    cell = np.full(len(xy), -1, dtype=np.int64)
    cell[valid] = (fy[valid].astype(np.int64) + HALF) * GRID + (fx[valid].astype(np.int64) + HALF)
    return cell, valid


def _seq_sum(v):
    """row-wise sequential sums of v (k, c) -> (k,)"""
    return np.add.accumulate(v, axis=1)[:, -1]


def quality(a, b, T=None, radius=3.5, min_points=6, min_other=1, det_min=1e-6):
    """-> (result: a RESULT_DTYPE scalar, points (n_a + n_b,) POINT_DTYPE)"""
    a = np.asarray(a, dtype=np.float32).reshape(-1, 2)
    b = np.asarray(b, dtype=np.float32).reshape(-1, 2)
    n_a, n = len(a), len(a) + len(b)
    res = np.zeros((), dtype=RESULT_DTYPE)
    pts = np.zeros(n, dtype=POINT_DTYPE)
    if len(a) > MAX_POINTS or len(b) > MAX_POINTS:
        res["status"] = STATUS_POINTS
        return res, pts
    r = float(radius)
    r2 = r * r
    xy = joint_cloud(a, b, T)
    cell, valid = cells_of(xy, r)
    status = 0 if bool(valid.all()) else STATUS_RANGE
    X, Y = xy[:, 0].astype(np.float64), xy[:, 1].astype(np.float64)
    is_b = np.arange(n) >= n_a
    order = np.argsort(cell, kind="stable")          # by cell, inside a cell by joint index
    order = order[cell[order] >= 0]
    sc = cell[order]
    occupied, first = np.unique(sc, return_index=True)
    last = np.append(first[1:], len(sc))
    where = {int(c): (int(f), int(l)) for c, f, l in zip(occupied, first, last)}
    scored = np.zeros(n, dtype=bool)
    for c in occupied:
        iy, ix = divmod(int(c), GRID)
        cand = []
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                jx, jy = ix + dx, iy + dy
                if 0 <= jx < GRID and 0 <= jy < GRID and jy * GRID + jx in where:
                    f, l = where[jy * GRID + jx]
                    cand.append(order[f:l])
        cand = np.concatenate(cand)
        qx, qy, qb = X[cand][None, :], Y[cand][None, :], is_b[cand][None, :]
        f, l = where[int(c)]
        for lo in range(f, l, _ROWS):
            p = order[lo:min(lo + _ROWS, l)]
            ex, ey = qx - X[p][:, None], qy - Y[p][:, None]
            sets = {}
            near = ex * ex + ey * ey <= r2
            sets["joint"] = near
            sets["separate"] = near & (qb == is_b[p][:, None])
            m = {k: v.sum(axis=1) for k, v in sets.items()}
            pts["m_joint"][p], pts["m_separate"][p] = m["joint"], m["separate"]
            sc_p = (m["separate"] >= min_points) & (m["joint"] - m["separate"] >= min_other)
            scored[p] = sc_p
            if not sc_p.any():
                continue
            rows = np.nonzero(sc_p)[0]
            for k, field in (("separate", "det_separate"), ("joint", "det_joint")):
                s, mm = sets[k][rows], m[k][rows].astype(np.float64)
                mx = _seq_sum(np.where(s, qx, 0.0)) / mm
                my = _seq_sum(np.where(s, qy, 0.0)) / mm
                ux, uy = qx - mx[:, None], qy - my[:, None]
                sxx = _seq_sum(np.where(s, ux * ux, 0.0)) / (mm - 1.0)
                syy = _seq_sum(np.where(s, uy * uy, 0.0)) / (mm - 1.0)
                sxy = _seq_sum(np.where(s, ux * uy, 0.0)) / (mm - 1.0)
                pts[field][p[rows]] = sxx * syy - sxy * sxy
    idx = np.nonzero(scored)[0]
    res["n_valid"] = int(valid.sum())
    res["n_scored"] = len(idx)
    res["n_scored_a"] = int((idx < n_a).sum())
    if len(idx) == 0:
        status |= STATUS_EMPTY
    else:
        hj = hs = 0.0
        for i in idx:
            hj = hj + (0.5 * math.log(max(float(pts["det_joint"][i]), det_min)) + H_CONST)
            hs = hs + (0.5 * math.log(max(float(pts["det_separate"][i]), det_min)) + H_CONST)
        res["h_joint"], res["h_separate"] = hj / len(idx), hs / len(idx)
        res["quality"] = res["h_joint"] - res["h_separate"]
    res["status"] = status
    return res, pts
