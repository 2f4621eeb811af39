"""numpy restatement of the sub-cell refinement of a pose in the grid map (include/rsx.h, rsx_gridmap_refine_*): the arithmetic
contract of csrc/gridrefine.hip.  None of this is in the reference checkout -- parity unpinned.  Levenberg-Marquardt with an accept
test on the bilinearly interpolated likelihood plane (Hector SLAM's matcher; what Olson's and Cartographer's matchers put behind the
correlative stage).  Everything is fp64 on plain operations, nothing fused, and the ORDER of every sum is part of the rule: partial
p[t], t = 0 .. 255, is the sequential sum over points t, t + 256, ... from 0.0, and the total is the balanced adjacent tree over the
256 partials.

A job: points [n, 2] float32 and a prior (r00, r01, tx, r10, r11, ty) taking the cloud's frame into the map frame; the likelihood plane
L is uint8 [height][width] (row = y), cells outside the map read 0; the map's geometry comes as a dict of tests/gridmap_np.py (width,
height, resolution, origin_x, origin_y)."""
import numpy as np

import mocomp_np as mc

MAX_POINTS = 8192
STATUS_TRANSFORM, STATUS_POINTS, STATUS_EMPTY, STATUS_SINGULAR, STATUS_MAX = 1, 2, 4, 16, 32
DEFAULTS = dict(damping=1e-3, max_shift_step=1.0, max_rotation_step=0.02, shift_tolerance=1e-3, rotation_tolerance=1e-5, max_evaluations=32)
PLACE = 64          # cells outside the map up to which a point is placed
LANES = 256         # partial sums
LAMBDA_MIN, LAMBDA_MAX = 1e-9, 1e6
_PAD = 72           # the frame of zeros of the vectorised form: a placed point's four bytes lie at most 65 cells outside the map
N_SUMS = 11         # cost, score, g0 g1 g2, H00 H01 H02 H11 H12 H22

RESULT = np.dtype([("transform", np.float64, 6), ("hessian", np.float64, 6), ("cost_initial", np.float64), ("cost", np.float64),
                   ("score_initial", np.float64), ("score", np.float64), ("evaluations", np.int32), ("accepted", np.int32),
                   ("n_points", np.int32), ("n_inside", np.int32), ("status", np.int32), ("reserved", np.int32)])   # rsx_gridmap_refine_result, 152 bytes
PARAMS = np.dtype([("damping", np.float64), ("max_shift_step", np.float64), ("max_rotation_step", np.float64), ("shift_tolerance", np.float64),
                   ("rotation_tolerance", np.float64), ("max_evaluations", np.int32), ("reserved", np.int32)])      # rsx_gridmap_refine_params, 48 bytes


def params(**kw):
    p = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in p:
            raise TypeError("no parameter " + k)
        p[k] = v
    return p


def frame(L, p):
    L = np.asarray(L, dtype=np.uint8)
    assert L.shape == (p["height"], p["width"])
    framed = np.zeros((p["height"] + 2 * _PAD, p["width"] + 2 * _PAD), dtype=np.uint8)
    framed[_PAD:_PAD + p["height"], _PAD:_PAD + p["width"]] = L
    return framed


def ordered_sum(terms):
    """terms [n, m] float64 -> [m]: partial t = the sequential sum over rows t, t + 256, ... from 0.0 (a missing row adds 0.0, which
    changes no partial: none is ever -0.0), then a[i] = a[2 i] + a[2 i + 1] eight times"""
    n, m = terms.shape
    rounds = -(-n // LANES)
    padded = np.zeros((max(rounds, 1) * LANES, m), dtype=np.float64)
    padded[:n] = terms
    padded = padded.reshape(-1, LANES, m)
    a = np.zeros((LANES, m), dtype=np.float64)
    for row in padded:
        a = a + row
    while len(a) > 1:
        a = a[0::2] + a[1::2]
    return a[0]


def evaluate(framed, xy, pose, p):
    """one evaluation at a pose -> (sums [11] float64, n_points, n_inside).  Vectorised over the points"""
    xy = np.asarray(xy, dtype=np.float32).reshape(-1, 2)
    x, y = xy[:, 0].astype(np.float64), xy[:, 1].astype(np.float64)
    r00, r01, tx, r10, r11, ty = (np.float64(v) for v in pose)
    inv_res = np.float64(1.0) / np.float64(p["resolution"])
    W, H = p["width"], p["height"]
    with np.errstate(all="ignore"):
        finite = np.isfinite(x) & np.isfinite(y)
        rx, ry = r00 * x + r01 * y, r10 * x + r11 * y
        fx, fy = ((rx + tx) - np.float64(p["origin_x"])) * inv_res, ((ry + ty) - np.float64(p["origin_y"])) * inv_res
        placed = finite & (fx >= -PLACE) & (fx < W + PLACE) & (fy >= -PLACE) & (fy < H + PLACE)      # (a NaN fails)
        fxp, fyp = np.where(placed, fx, 0.0), np.where(placed, fy, 0.0)
        px, py = fxp - 0.5, fyp - 0.5
        fi, fj = np.floor(px), np.floor(py)
        a, b = px - fi, py - fj
        i0, j0 = fi.astype(np.int64) + _PAD, fj.astype(np.int64) + _PAD
        l00, l01 = framed[j0, i0].astype(np.float64), framed[j0, i0 + 1].astype(np.float64)
        l10, l11 = framed[j0 + 1, i0].astype(np.float64), framed[j0 + 1, i0 + 1].astype(np.float64)
        top, bot = (1.0 - a) * l00 + a * l01, (1.0 - a) * l10 + a * l11
        M = (1.0 - b) * top + b * bot
        gx = (1.0 - b) * (l01 - l00) + b * (l11 - l10)
        gy = (1.0 - a) * (l10 - l00) + a * (l11 - l01)
        jt = (gy * rx - gx * ry) * inv_res
        M, gx, gy, jt = (np.where(placed, v, 0.0) for v in (M, gx, gy, jt))
        r = np.where(placed, 255.0 - M, np.where(finite, 255.0, 0.0))
        terms = np.stack([r * r, M, gx * r, gy * r, jt * r, gx * gx, gx * gy, gx * jt, gy * gy, gy * jt, jt * jt], axis=1)
        terms[~finite] = 0.0
    inside = placed & (np.floor(fx) >= 0) & (np.floor(fx) < W) & (np.floor(fy) >= 0) & (np.floor(fy) < H)
    return ordered_sum(terms), int(np.count_nonzero(placed)), int(np.count_nonzero(inside))


def evaluate_naive(L, xy, pose, p):
    """the same by the rule as it is written: a loop over the points, 256 partial sums, the tree"""
    xy = np.asarray(xy, dtype=np.float32).reshape(-1, 2)
    f = np.float64
    r00, r01, tx, r10, r11, ty = (f(v) for v in pose)
    inv_res = f(1.0) / f(p["resolution"])
    ox, oy, W, H = f(p["origin_x"]), f(p["origin_y"]), p["width"], p["height"]

    def cell(j, i):
        return f(L[j][i]) if 0 <= i < W and 0 <= j < H else f(0.0)

    part = [[f(0.0)] * N_SUMS for _ in range(LANES)]
    n_points = n_inside = 0
    with np.errstate(all="ignore"):
        for k in range(len(xy)):
            x, y = f(xy[k, 0]), f(xy[k, 1])
            if not (np.isfinite(x) and np.isfinite(y)):
                continue
            rx, ry = r00 * x + r01 * y, r10 * x + r11 * y
            fx, fy = ((rx + tx) - ox) * inv_res, ((ry + ty) - oy) * inv_res
            if fx >= -PLACE and fx < W + PLACE and fy >= -PLACE and fy < H + PLACE:
                n_points += 1
                n_inside += 0 <= np.floor(fx) < W and 0 <= np.floor(fy) < H
                px, py = fx - f(0.5), fy - f(0.5)
                i0, j0 = int(np.floor(px)), int(np.floor(py))
                a, b = px - f(i0), py - f(j0)
                l00, l01, l10, l11 = cell(j0, i0), cell(j0, i0 + 1), cell(j0 + 1, i0), cell(j0 + 1, i0 + 1)
                top, bot = (f(1.0) - a) * l00 + a * l01, (f(1.0) - a) * l10 + a * l11
                M = (f(1.0) - b) * top + b * bot
                gx = (f(1.0) - b) * (l01 - l00) + b * (l11 - l10)
                gy = (f(1.0) - a) * (l10 - l00) + a * (l11 - l01)
                jt = (gy * rx - gx * ry) * inv_res
                r = f(255.0) - M
            else:
                M = gx = gy = jt = f(0.0)
                r = f(255.0)
            terms = (r * r, M, gx * r, gy * r, jt * r, gx * gx, gx * gy, gx * jt, gy * gy, gy * jt, jt * jt)
            acc = part[k % LANES]
            for q in range(N_SUMS):
                acc[q] = acc[q] + terms[q]
    a = part
    while len(a) > 1:
        a = [[a[2 * i][q] + a[2 * i + 1][q] for q in range(N_SUMS)] for i in range(len(a) // 2)]
    return np.array(a[0], dtype=np.float64), n_points, n_inside


def solve(s, lam):
    """(H + lam diag H) delta = g by LDL^T written out -> delta [3], or None when a pivot is not > 0 (a NaN fails)"""
    f = np.float64
    g0, g1, g2, h00, h01, h02, h11, h12, h22 = (f(v) for v in s[2:11])
    with np.errstate(all="ignore"):
        damp = f(1.0) + f(lam)
        a00, a11, a22, a01, a02, a12 = h00 * damp, h11 * damp, h22 * damp, h01, h02, h12
        d0 = a00
        if not d0 > 0:
            return None
        l10, l20 = a01 / d0, a02 / d0
        d1 = a11 - l10 * a01
        if not d1 > 0:
            return None
        e = a12 - l20 * a01
        l21 = e / d1
        d2 = (a22 - l20 * a02) - l21 * e
        if not d2 > 0:
            return None
        z0 = g0
        z1 = g1 - l10 * z0
        z2 = (g2 - l20 * z0) - l21 * z1
        w0, w1, w2 = z0 / d0, z1 / d1, z2 / d2
        t2 = w2
        t1 = w1 - l21 * t2
        t0 = (w0 - l10 * t1) - l20 * t2
    return t0, t1, t2


def clamp(v, m):
    """by two comparisons: a NaN passes through"""
    if v > m:
        v = m
    if v < -m:
        v = -m
    return v


def refine(L, xy, prior, p, rp, evaluate_fn=None):
    """one job that is not skipped -> a RESULT scalar"""
    f = np.float64
    framed = frame(L, p)
    ev = (lambda pose: evaluate(framed, xy, pose, p)) if evaluate_fn is None else (lambda pose: evaluate_fn(L, xy, pose, p))
    res = f(p["resolution"])
    pose = [f(v) for v in prior]
    s, n_points, n_inside = ev(pose)
    cost_initial, score_initial = s[0], s[1]
    evaluations, accepted, status = 1, 0, 0
    lam = f(rp["damping"])
    m_shift, m_rot = f(rp["max_shift_step"]), f(rp["max_rotation_step"])
    if score_initial == 0:
        status = STATUS_EMPTY
    else:
        status = STATUS_MAX
        with np.errstate(all="ignore"):
            while evaluations < rp["max_evaluations"]:
                delta = solve(s, lam)
                if delta is None:
                    status = STATUS_SINGULAR
                    break
                d0, d1, d2 = clamp(delta[0], m_shift), clamp(delta[1], m_shift), clamp(delta[2], m_rot)
                r00, r01, tx, r10, r11, ty = pose
                sn, cs, _, _ = (f(v) for v in mc.poly(d2))
                trial = [cs * r00 - sn * r10, cs * r01 - sn * r11, tx + d0 * res, sn * r00 + cs * r10, sn * r01 + cs * r11, ty + d1 * res]
                s2, np2, ni2 = ev(trial)
                evaluations += 1
                if s2[0] < s[0]:
                    pose, s, n_points, n_inside = trial, s2, np2, ni2
                    accepted += 1
                    lam = max(lam / f(10.0), f(LAMBDA_MIN))
                    if max(abs(d0), abs(d1)) < rp["shift_tolerance"] and abs(d2) < rp["rotation_tolerance"]:
                        status = 0
                        break
                else:
                    lam = f(10.0) * lam
                    if lam > LAMBDA_MAX:
                        status = 0
                        break
    r = np.zeros((), dtype=RESULT)
    r["transform"] = pose
    r["hessian"] = s[5:11]
    r["cost_initial"], r["cost"], r["score_initial"], r["score"] = cost_initial, s[0], score_initial, s[1]
    r["evaluations"], r["accepted"], r["n_points"], r["n_inside"], r["status"] = evaluations, accepted, n_points, n_inside, status
    return r


def refine_batch(L, xy, offsets, priors, p, rp, device_entry=False, evaluate_fn=None):
    """-> results [n] of RESULT.  A non-finite prior is skipped (STATUS_TRANSFORM: a zero record but for the status); a job above the
    cap is refused by the host entry (ValueError) and skipped with STATUS_POINTS by the device entry"""
    xy = np.asarray(xy, dtype=np.float32).reshape(-1, 2)
    priors = np.asarray(priors, dtype=np.float64).reshape(-1, 6)
    results = np.zeros(len(priors), dtype=RESULT)
    for i in range(len(priors)):
        pts = xy[offsets[i]:offsets[i + 1]]
        status = (0 if np.all(np.isfinite(priors[i])) else STATUS_TRANSFORM) | (STATUS_POINTS if len(pts) > MAX_POINTS else 0)
        if status & STATUS_POINTS and not device_entry:
            raise ValueError("job %d has %d points" % (i, len(pts)))
        if status:
            results[i]["status"] = status
            continue
        results[i] = refine(L, pts, priors[i], p, rp, evaluate_fn=evaluate_fn)
    return results
