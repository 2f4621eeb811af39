"""numpy restatement of the correlative scan-to-map matching (include/rsx.h, rsx_gridmap_match_* and rsx_gridmap_likelihood_*): the
arithmetic contract of csrc/gridmatch.hip.  None of this is in the reference checkout -- parity unpinned.  fp64 on plain operations up
to the cell of a point, integers from there on.

A job: points [n, 2] float32 and a prior (r00, r01, tx, r10, r11, ty) taking the cloud's frame into the map frame; the likelihood plane
L is uint8 [height][width] (row = y); the map's geometry comes as a dict of tests/gridmap_np.py (width, height, resolution, origin_x,
origin_y).  Candidates (k, v, u), |k| <= K, |v| <= V, |u| <= U; the volume is uint32 [2K + 1][2V + 1][2U + 1]."""
import math

import numpy as np

import gridmap_np as gm

MAX_POINTS = 8192
STATUS_TRANSFORM, STATUS_POINTS, STATUS_EMPTY = 1, 2, 4
DEFAULTS = dict(angle_step=0.01, angle_steps=8, x_cells=8, y_cells=8)
PLACE = 64     # cells outside the map up to which a point is placed
_PAD = 96      # PLACE + the largest shift: the frame of zeros of the vectorised form
_CHUNK = 1024  # points per gather (memory only)

RESULT = np.dtype([("transform", np.float64, 6), ("k", np.int32), ("u", np.int32), ("v", np.int32), ("score", np.uint32),
                   ("score_prior", np.uint32), ("score_runner_up", np.uint32), ("n_points", np.int32), ("n_inside", np.int32),
                   ("status", np.int32), ("reserved", np.int32)])   # rsx_gridmap_match_result, 88 bytes


def params(**kw):
    p = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in p:
            raise TypeError("no parameter " + k)
        p[k] = v
    return p


def tables(mp):
    """c[k + K], s[k + K] = cos, sin of (double)k * angle_step: fp64, rounded once to fp32"""
    K = mp["angle_steps"]
    ang = [float(k) * float(mp["angle_step"]) for k in range(-K, K + 1)]
    return (np.array([math.cos(t) for t in ang], dtype=np.float64).astype(np.float32),
            np.array([math.sin(t) for t in ang], dtype=np.float64).astype(np.float32))


def likelihood(planes, mode, min_observations=1):
    """the likelihood plane from the count planes: render's byte; the hit ratio with -1 (unknown) as 0"""
    if mode == 0:
        return gm.render_mean(planes, min_observations)
    return np.maximum(gm.render_hits(planes, min_observations), 0).astype(np.uint8)


def cells(xy, prior, c, s, p):
    """steps 1 - 5 for one rotation (c, s: the table values, fp32) -> ix, iy (int64) of the PLACED points"""
    xy = np.asarray(xy, dtype=np.float32).reshape(-1, 2)
    x, y = xy[:, 0].astype(np.float64), xy[:, 1].astype(np.float64)
    c, s = np.float64(c), np.float64(s)
    r00, r01, tx, r10, r11, ty = (np.float64(v) for v in prior)
    inv_res = np.float64(1.0) / np.float64(p["resolution"])
    with np.errstate(all="ignore"):
        rx, ry = c * x - s * y, s * x + c * y
        mx, my = r00 * rx + r01 * ry + tx, r10 * rx + r11 * ry + ty
        fx, fy = (mx - np.float64(p["origin_x"])) * inv_res, (my - np.float64(p["origin_y"])) * inv_res
        placed = (fx >= -PLACE) & (fx < p["width"] + PLACE) & (fy >= -PLACE) & (fy < p["height"] + PLACE)   # (a NaN fails)
    return np.floor(fx[placed]).astype(np.int64), np.floor(fy[placed]).astype(np.int64)


def volume(L, xy, prior, p, mp):
    """uint32 [2K + 1][2V + 1][2U + 1]: score(k, v, u) = the sum of L[iy + v][ix + u] over the placed points whose shifted cell is
    inside the map.  Vectorised: L in a frame of zeros, the window of shifts around every point's cell gathered and summed."""
    K, U, V = mp["angle_steps"], mp["x_cells"], mp["y_cells"]
    L = np.asarray(L, dtype=np.uint8)
    assert L.shape == (p["height"], p["width"])
    framed = np.zeros((p["height"] + 2 * _PAD, p["width"] + 2 * _PAD), dtype=np.uint8)
    framed[_PAD:_PAD + p["height"], _PAD:_PAD + p["width"]] = L
    windows = np.lib.stride_tricks.sliding_window_view(framed, (2 * V + 1, 2 * U + 1))   # windows[y, x] = framed[y : y + nv, x : x + nu]
    c, s = tables(mp)
    out = np.zeros((2 * K + 1, 2 * V + 1, 2 * U + 1), dtype=np.uint32)
    for kk in range(2 * K + 1):
        ix, iy = cells(xy, prior, c[kk], s[kk], p)
        for a in range(0, len(ix), _CHUNK):
            out[kk] += windows[iy[a:a + _CHUNK] + _PAD - V, ix[a:a + _CHUNK] + _PAD - U].sum(axis=0, dtype=np.uint32)
    return out


def volume_naive(L, xy, prior, p, mp):
    """the same by the rule as it is written: a loop over the candidates and the points"""
    K, U, V = mp["angle_steps"], mp["x_cells"], mp["y_cells"]
    c, s = tables(mp)
    out = np.zeros((2 * K + 1, 2 * V + 1, 2 * U + 1), dtype=np.uint32)
    for k in range(-K, K + 1):
        ix, iy = cells(xy, prior, c[k + K], s[k + K], p)
        for v in range(-V, V + 1):
            for u in range(-U, U + 1):
                total = 0
                for x, y in zip(ix.tolist(), iy.tolist()):
                    if 0 <= x + u < p["width"] and 0 <= y + v < p["height"]:
                        total += int(L[y + v][x + u])
                out[k + K, v + V, u + U] = total
    return out


def pick(vol, xy, prior, p, mp):
    """the result record of one job from its volume (a RESULT scalar)"""
    K, U, V = mp["angle_steps"], mp["x_cells"], mp["y_cells"]
    r = np.zeros((), dtype=RESULT)
    kk, vv, uu = np.meshgrid(np.arange(-K, K + 1), np.arange(-V, V + 1), np.arange(-U, U + 1), indexing="ij")
    flat = vol.reshape(-1).astype(np.int64)
    # the highest score, then the smallest |k|, then the smallest u u + v v, then the smallest linear index
    order = np.lexsort((np.arange(flat.size), (uu * uu + vv * vv).reshape(-1), np.abs(kk).reshape(-1), -flat))
    best = int(order[0])
    k, v, u = int(kk.reshape(-1)[best]), int(vv.reshape(-1)[best]), int(uu.reshape(-1)[best])
    far = (np.abs(kk - k) > 1) | (np.abs(vv - v) > 1) | (np.abs(uu - u) > 1)
    c32, s32 = tables(mp)
    c, s = np.float64(c32[k + K]), np.float64(s32[k + K])
    ix, iy = cells(xy, prior, c32[k + K], s32[k + K], p)
    r["k"], r["u"], r["v"] = k, u, v
    r["score"], r["score_prior"] = flat[best], vol[K, V, U]
    r["score_runner_up"] = vol[far].max() if far.any() else 0
    r["n_points"] = len(ix)
    r["n_inside"] = np.count_nonzero((ix + u >= 0) & (ix + u < p["width"]) & (iy + v >= 0) & (iy + v < p["height"]))
    r00, r01, tx, r10, r11, ty = (np.float64(q) for q in prior)
    if flat[best] == 0:
        r["status"] = STATUS_EMPTY
        r["transform"] = (r00, r01, tx, r10, r11, ty)
    else:
        res = np.float64(p["resolution"])
        r["transform"] = (r00 * c + r01 * s, r01 * c - r00 * s, tx + np.float64(u) * res,
                          r10 * c + r11 * s, r11 * c - r10 * s, ty + np.float64(v) * res)
    return r


def match_batch(L, xy, offsets, priors, p, mp, device_entry=False, volume_fn=volume):
    """-> (results [n] of RESULT, volumes uint32 [n, 2K + 1, 2V + 1, 2U + 1]).  A non-finite prior is skipped (STATUS_TRANSFORM: a
    zero record, zero scores); a job above the cap is refused by the host entry (ValueError) and skipped with STATUS_POINTS by the
    device entry"""
    xy = np.asarray(xy, dtype=np.float32).reshape(-1, 2)
    priors = np.asarray(priors, dtype=np.float64).reshape(-1, 6)
    n = len(priors)
    K, U, V = mp["angle_steps"], mp["x_cells"], mp["y_cells"]
    results = np.zeros(n, dtype=RESULT)
    vols = np.zeros((n, 2 * K + 1, 2 * V + 1, 2 * U + 1), dtype=np.uint32)
    for i in range(n):
        pts = xy[offsets[i]:offsets[i + 1]]
        status = (0 if np.all(np.isfinite(priors[i])) else STATUS_TRANSFORM) | (STATUS_POINTS if len(pts) > MAX_POINTS else 0)
        if status & STATUS_POINTS and not device_entry:
            raise ValueError("job %d has %d points" % (i, len(pts)))
        if status:
            results[i]["status"] = status
            continue
        vols[i] = volume_fn(L, pts, priors[i], p, mp)
        results[i] = pick(vols[i], pts, priors[i], p, mp)
    return results, vols

