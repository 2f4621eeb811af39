"""numpy restatement of the wide-window correlative search pruned by bounds (include/rsx.h, rsx_gridmap_search_*): the arithmetic
contract of csrc/gridsearch.hip.  None of this is in the reference checkout -- parity unpinned.  fp64 on plain operations up to the
cell of a point, integers from there on.

Jobs, priors, tables and the likelihood plane are those of tests/gridmatch_np.py; the placement margin is PL = max(64, U, V).
Candidates (k, v, u), |k| <= K <= 180, |v| <= V <= 256, |u| <= U <= 256.  Two ways to the winner: volume() + pick_exhaustive(), every
candidate scored; and search(), the rule of the kernels -- bounds of 8 x 8 blocks from the pooled plane, a seed block per rotation,
the threshold T0, exact scores of the refined blocks only.  They give the same winner (tests/test_gridsearch_restatement.py)."""
import numpy as np

import gridmatch_np as gx

MAX_POINTS = gx.MAX_POINTS
MAX_ANGLE_STEPS, MAX_CELLS, BLOCK = 180, 256, 8
STATUS_TRANSFORM, STATUS_POINTS, STATUS_EMPTY, STATUS_BELOW = 1, 2, 4, 8
DEFAULTS = dict(angle_step=0.01, angle_steps=32, x_cells=64, y_cells=64, min_score=0)
_CHUNK = 1024  # points per gather (memory only)

RESULT = np.dtype([("transform", np.float64, 6), ("k", np.int32), ("u", np.int32), ("v", np.int32), ("score", np.uint32),
                   ("score_prior", np.uint32), ("bound_runner_up", np.uint32), ("n_points", np.int32), ("n_inside", np.int32),
                   ("status", np.int32), ("n_blocks", np.int32), ("n_refined", np.int32), ("reserved", np.int32)])   # rsx_gridmap_search_result, 96 bytes
SHARED = ("transform", "k", "u", "v", "score", "score_prior", "n_points", "n_inside", "status")   # equal to rsx_gridmap_match_result's


def params(**kw):
    p = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in p:
            raise TypeError("no parameter " + k)
        p[k] = v
    return p


def window(mp):
    return mp["angle_steps"], mp["x_cells"], mp["y_cells"]


def margin(mp):
    """PL: cells outside the map up to which a point is placed"""
    return max(64, mp["x_cells"], mp["y_cells"])


def blocks(mp):
    """-> nbv, nbu"""
    return (2 * mp["y_cells"] + 1 + BLOCK - 1) // BLOCK, (2 * mp["x_cells"] + 1 + BLOCK - 1) // BLOCK


def cells(xy, prior, c, s, p, PL):
    """steps 1 - 5 of include/rsx.h for one rotation with the placement margin PL -> ix, iy (int64) of the PLACED points"""
    xy = np.asarray(xy, dtype=np.float32).reshape(-1, 2)
    x, y = xy[:, 0].astype(np.float64), xy[:, 1].astype(np.float64)
    c, s = np.float64(c), np.float64(s)
    r00, r01, tx, r10, r11, ty = (np.float64(v) for v in prior)
    inv_res = np.float64(1.0) / np.float64(p["resolution"])
    with np.errstate(all="ignore"):
        rx, ry = c * x - s * y, s * x + c * y
        mx, my = r00 * rx + r01 * ry + tx, r10 * rx + r11 * ry + ty
        fx, fy = (mx - np.float64(p["origin_x"])) * inv_res, (my - np.float64(p["origin_y"])) * inv_res
        placed = (fx >= -PL) & (fx < p["width"] + PL) & (fy >= -PL) & (fy < p["height"] + PL)   # (a NaN fails)
    return np.floor(fx[placed]).astype(np.int64), np.floor(fy[placed]).astype(np.int64)


def _pad(mp):
    """the frame of zeros of the vectorised forms: PL, the largest shift, and a block's width beyond it"""
    return margin(mp) + max(mp["x_cells"], mp["y_cells"]) + 2 * BLOCK


def framed(L, p, pad):
    L = np.asarray(L, dtype=np.uint8)
    assert L.shape == (p["height"], p["width"])
    out = np.zeros((p["height"] + 2 * pad, p["width"] + 2 * pad), dtype=np.uint8)
    out[pad:pad + p["height"], pad:pad + p["width"]] = L
    return out


def pooled(L, p, pad):
    """P[y][x] = max of L[y + a][x + b] over 0 <= a, b < 8, cells outside the map as 0, for -pad <= y < height + pad - 7 and x
    likewise, in a frame: P[y][x] is at [y + pad][x + pad] (what lies beyond is 0, as P is there)"""
    f = framed(L, p, pad)
    out = np.zeros_like(f)
    out[:f.shape[0] - 7, :f.shape[1] - 7] = np.lib.stride_tricks.sliding_window_view(f, (BLOCK, BLOCK)).max(axis=(2, 3))
    return out


def _gather_sum(windows, rows, cols):
    out = np.zeros(windows.shape[2:], dtype=np.uint32)
    for a in range(0, len(rows), _CHUNK):
        out += windows[rows[a:a + _CHUNK], cols[a:a + _CHUNK]].sum(axis=0, dtype=np.uint32)
    return out


def volume(L, xy, prior, p, mp):
    """uint32 [2K + 1][2V + 1][2U + 1]: every candidate scored, gridmatch_np.volume with this rule's margin and a frame of its own"""
    K, U, V = window(mp)
    PL, pad = margin(mp), _pad(mp)
    windows = np.lib.stride_tricks.sliding_window_view(framed(L, p, pad), (2 * V + 1, 2 * U + 1))
    c, s = gx.tables(mp)
    out = np.zeros((2 * K + 1, 2 * V + 1, 2 * U + 1), dtype=np.uint32)
    for kk in range(2 * K + 1):
        ix, iy = cells(xy, prior, c[kk], s[kk], p, PL)
        out[kk] = _gather_sum(windows, iy + pad - V, ix + pad - U)
    return out


def order_key(score, k, u, v, index):
    """the tie order as a tuple that sorts ascending: the highest score, then the smallest |k|, the smallest u u + v v, the smallest
    linear index"""
    return (-int(score), abs(int(k)), int(u) * int(u) + int(v) * int(v), int(index))


def pick_exhaustive(vol, mp):
    """the winner of a whole volume by the tie order -> (k, u, v, score), or None when no candidate reaches max(min_score, 1)"""
    K, U, V = window(mp)
    floor = max(int(mp["min_score"]), 1)
    kk, vv, uu = np.meshgrid(np.arange(-K, K + 1), np.arange(-V, V + 1), np.arange(-U, U + 1), indexing="ij")
    flat = vol.reshape(-1).astype(np.int64)
    top = int(flat.max())
    if top < floor:
        return None
    at = np.flatnonzero(flat == top)
    best = min(at.tolist(), key=lambda i: order_key(top, kk.reshape(-1)[i], uu.reshape(-1)[i], vv.reshape(-1)[i], i))
    return int(kk.reshape(-1)[best]), int(uu.reshape(-1)[best]), int(vv.reshape(-1)[best]), top


def block_max(vol, mp):
    """uint32 [2K + 1][nbv][nbu]: the highest score of every block of a volume"""
    nbv, nbu = blocks(mp)
    padded = np.zeros((vol.shape[0], BLOCK * nbv, BLOCK * nbu), dtype=np.uint32)
    padded[:, :vol.shape[1], :vol.shape[2]] = vol
    return padded.reshape(vol.shape[0], nbv, BLOCK, nbu, BLOCK).max(axis=(2, 4))


def placed_cells(xy, prior, p, mp):
    """cells() for every rotation of the window -> list of (ix, iy), [k + K]"""
    c, s = gx.tables(mp)
    return [cells(xy, prior, c[kk], s[kk], p, margin(mp)) for kk in range(2 * mp["angle_steps"] + 1)]


def bounds(L, xy, prior, p, mp, placed=None):
    """uint32 [2K + 1][nbv][nbu]: bound(k, bv, bu) = the sum over the placed points of P[iy - V + 8 bv][ix - U + 8 bu]"""
    K, U, V = window(mp)
    nbv, nbu = blocks(mp)
    PL, pad = margin(mp), _pad(mp)
    P = pooled(L, p, pad)
    windows = np.lib.stride_tricks.sliding_window_view(P, (BLOCK * (nbv - 1) + 1, BLOCK * (nbu - 1) + 1))[:, :, ::BLOCK, ::BLOCK]
    out = np.zeros((2 * K + 1, nbv, nbu), dtype=np.uint32)
    for kk, (ix, iy) in enumerate(placed if placed is not None else placed_cells(xy, prior, p, mp)):
        out[kk] = _gather_sum(windows, iy + pad - V, ix + pad - U)
    return out


def _block_scores(win8, full, ix, iy, mp, pad, wanted):
    """exact scores of the blocks `wanted` (list of (bv, bu)) of one rotation -> {(bv, bu): int64 [8][8], [a][b] = score(v = -V + 8 bv
    + a, u = -U + 8 bu + b), -1 outside the window}.  Integer sums: gathering block by block or the rotation's whole slice at once
    (cheaper when many blocks are wanted) gives the same numbers"""
    K, U, V = window(mp)
    nbv, nbu = blocks(mp)
    out = {}
    whole = None
    if 4 * len(wanted) > nbv * nbu:
        whole = np.full((BLOCK * nbv, BLOCK * nbu), -1, dtype=np.int64)
        whole[:2 * V + 1, :2 * U + 1] = _gather_sum(full, iy + pad - V, ix + pad - U)
    for bv, bu in wanted:
        if whole is not None:
            out[(bv, bu)] = whole[BLOCK * bv:BLOCK * bv + BLOCK, BLOCK * bu:BLOCK * bu + BLOCK]
            continue
        sc = _gather_sum(win8, iy + pad - V + BLOCK * bv, ix + pad - U + BLOCK * bu).astype(np.int64)
        sc[np.arange(BLOCK) - V + BLOCK * bv > V, :] = -1
        sc[:, np.arange(BLOCK) - U + BLOCK * bu > U] = -1
        out[(bv, bu)] = sc
    return out


def search(L, xy, prior, p, mp, bnd=None):
    """one job by the rule -> (record (a RESULT scalar), bounds uint32 [2K + 1][nbv][nbu], refined bool [2K + 1][nbv][nbu], T0)"""
    K, U, V = window(mp)
    nbv, nbu = blocks(mp)
    nu, nv = 2 * U + 1, 2 * V + 1
    pad = _pad(mp)
    min_score = int(mp["min_score"])
    Lf = framed(L, p, pad)
    win8 = np.lib.stride_tricks.sliding_window_view(Lf, (BLOCK, BLOCK))
    full = np.lib.stride_tricks.sliding_window_view(Lf, (nv, nu))
    c32, s32 = gx.tables(mp)
    placed = placed_cells(xy, prior, p, mp)
    if bnd is None:
        bnd = bounds(L, xy, prior, p, mp, placed)
    # the seeds: the block of every k with the highest bound (the first of equal ones), scored exactly
    seeds, seed_scores = [], []
    for kk, (ix, iy) in enumerate(placed):
        bi = int(np.argmax(bnd[kk].reshape(-1)))
        blk = (bi // nbu, bi % nbu)
        seed_scores.append(_block_scores(win8, full, ix, iy, mp, pad, [blk]))
        seeds.append(int(seed_scores[kk][blk].max()))
    ix0, iy0 = placed[K]
    score_prior = int(Lf[iy0 + pad, ix0 + pad].sum(dtype=np.int64))
    T0 = max(min_score, score_prior, max(seeds))
    refined = bnd >= max(T0, 1)
    # the winner: the best candidate by the tie order with score >= max(min_score, 1) among the refined blocks
    floor = max(min_score, 1)
    best = None
    for kk, (ix, iy) in enumerate(placed):
        wanted = [(int(a), int(b)) for a, b in np.argwhere(refined[kk])]
        scores = seed_scores[kk] if all(blk in seed_scores[kk] for blk in wanted) else _block_scores(win8, full, ix, iy, mp, pad, wanted)
        for (bv, bu) in wanted:
            sc = scores[(bv, bu)]
            top = int(sc.max())
            if top < floor or (best is not None and -top > best[0][0]):
                continue
            for a, b in np.argwhere(sc == top):
                v, u = -V + BLOCK * bv + int(a), -U + BLOCK * bu + int(b)
                key = order_key(top, kk - K, u, v, (kk * nv + v + V) * nu + u + U)
                if best is None or key < best[0]:
                    best = (key, kk - K, u, v, top)
    r = np.zeros((), dtype=RESULT)
    r["score_prior"], r["n_blocks"], r["n_refined"] = score_prior, (2 * K + 1) * nbv * nbu, np.count_nonzero(refined)
    r00, r01, tx, r10, r11, ty = (np.float64(q) for q in prior)
    if best is None:
        k = u = v = 0
        r["status"] = STATUS_EMPTY if min_score == 0 else STATUS_BELOW
        r["transform"] = (r00, r01, tx, r10, r11, ty)
    else:
        _, k, u, v, top = best
        c, s, res = np.float64(c32[k + K]), np.float64(s32[k + K]), np.float64(p["resolution"])
        r["score"] = top
        r["transform"] = (r00 * c + r01 * s, r01 * c - r00 * s, tx + np.float64(u) * res,
                          r10 * c + r11 * s, r11 * c - r10 * s, ty + np.float64(v) * res)
        ak, abv, abu = np.meshgrid(np.arange(2 * K + 1), np.arange(nbv), np.arange(nbu), indexing="ij")
        far = (np.abs(ak - (k + K)) > 1) | (np.abs(abv - (v + V) // BLOCK) > 1) | (np.abs(abu - (u + U) // BLOCK) > 1)
        r["bound_runner_up"] = bnd[far].max() if far.any() else 0
    ix, iy = placed[k + K]
    r["k"], r["u"], r["v"] = k, u, v
    r["n_points"] = len(ix)
    r["n_inside"] = np.count_nonzero((ix + u >= 0) & (ix + u < p["width"]) & (iy + v >= 0) & (iy + v < p["height"]))
    return r, bnd, refined, T0


def search_batch(L, xy, offsets, priors, p, mp, device_entry=False):
    """-> (results [n] of RESULT, bounds uint32 [n, 2K + 1, nbv, nbu]).  A non-finite prior is skipped (STATUS_TRANSFORM: a zero
    record, zero bounds); a job above the cap is refused by the host entry (ValueError) and skipped with STATUS_POINTS by the device
    entry"""
    xy = np.asarray(xy, dtype=np.float32).reshape(-1, 2)
    priors = np.asarray(priors, dtype=np.float64).reshape(-1, 6)
    n = len(priors)
    results = np.zeros(n, dtype=RESULT)
    bnds = np.zeros((n, 2 * mp["angle_steps"] + 1) + blocks(mp), dtype=np.uint32)
    for i in range(n):
        pts = xy[offsets[i]:offsets[i + 1]]
        status = (0 if np.all(np.isfinite(priors[i])) else STATUS_TRANSFORM) | (STATUS_POINTS if len(pts) > MAX_POINTS else 0)
        if status & STATUS_POINTS and not device_entry:
            raise ValueError("job %d has %d points" % (i, len(pts)))
        if status:
            results[i]["status"] = status
            continue
        results[i], bnds[i] = search(L, pts, priors[i], p, mp)[:2]
    return results, bnds
