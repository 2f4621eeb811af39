"""numpy restatement of the radar grid map (include/rsx.h, rsx_gridmap_*): the arithmetic contract of csrc/gridmap.hip.  None of this is
in the reference checkout -- parity unpinned.  It states the RULE (the bin by its two inequalities, the row by np.argmax over every
row); the kernel's search for the bin and the row is its own.  Everything is fp64 on plain operations; the planes hold integers.

State: three uint32 planes [height][width] (row = y): sum of the samples, number of scans that observed the cell, number of those whose
sample was >= hit_threshold.  A pose is six doubles (r00, r01, tx, r10, r11, ty) taking the sensor frame into the map frame; azimuth 0
is +x, row a sits at 2 pi a / rows, bin j covers [j rr, (j + 1) rr)."""
import math

import numpy as np

DEFAULTS = dict(width=1024, height=1024, resolution=0.5, origin_x=-256.0, origin_y=-256.0, range_resolution=0.0595, min_range_bins=58,
                range_halfwidth=4, hit_threshold=120, max_range=0.0)
_CHUNK = 1 << 15   # cells per argmax block (memory only)


def params(**kw):
    p = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in p:
            raise TypeError("no parameter " + k)
        p[k] = v
    return p


def tables(rows):
    """c[a], s[a] = cos, sin of 2 pi a / rows: fp64, rounded once to fp32 (the kernel widens them back)"""
    ang = [2.0 * math.pi * float(a) / float(rows) for a in range(rows)]
    return (np.array([math.cos(t) for t in ang], dtype=np.float64).astype(np.float32),
            np.array([math.sin(t) for t in ang], dtype=np.float64).astype(np.float32))


def zeros(p):
    return tuple(np.zeros((p["height"], p["width"]), dtype=np.uint32) for _ in range(3))


def _window(T, p, cols):
    """a box of cells that holds every cell the scan can observe (a generous margin; outside it the rule below observes nothing):
    only there is the rule evaluated -- for speed, it changes no value"""
    res, W, H = p["resolution"], p["width"], p["height"]
    reach = (cols + 2) * p["range_resolution"] * 1.001 + 2.0 * res
    if not np.isfinite(reach + abs(T[2]) + abs(T[5])):
        return 0, W, 0, H
    x0 = int(np.clip(math.floor((T[2] - reach - p["origin_x"]) / res) - 1, 0, W))
    x1 = int(np.clip(math.ceil((T[2] + reach - p["origin_x"]) / res) + 1, 0, W))
    y0 = int(np.clip(math.floor((T[5] - reach - p["origin_y"]) / res) - 1, 0, H))
    y1 = int(np.clip(math.ceil((T[5] + reach - p["origin_y"]) / res) + 1, 0, H))
    return x0, x1, y0, y1


def geometry(T, p, rows, cols, tabs=None):
    """steps 1 - 6 of the rule for ONE scan: -> dict with the flat cell indices (iy * width + ix) of the observed cells and, per
    observed cell, the bin j, the row a, d2, px, py and the two largest dot products (best, second)"""
    T = np.asarray(T, dtype=np.float64)
    r00, r01, tx, r10, r11, ty = (np.float64(v) for v in T)
    c32, s32 = tabs if tabs is not None else tables(rows)
    c, s = c32.astype(np.float64), s32.astype(np.float64)
    rr, res = np.float64(p["range_resolution"]), np.float64(p["resolution"])
    x0, x1, y0, y1 = _window(T, p, cols)
    edges = (np.arange(cols + 1, dtype=np.float64) * rr) ** 2          # (j rr)^2, j rr formed in fp64 and squared
    with np.errstate(all="ignore"):
        mx = np.float64(p["origin_x"]) + (np.arange(x0, x1, dtype=np.float64) + 0.5) * res
        my = np.float64(p["origin_y"]) + (np.arange(y0, y1, dtype=np.float64) + 0.5) * res
        dx, dy = np.broadcast_arrays((mx - tx)[None, :], (my - ty)[:, None])
        px = r00 * dx + r10 * dy
        py = r01 * dx + r11 * dy
        d2 = px * px + py * py
        j = np.searchsorted(edges, d2.ravel(), side="right").reshape(d2.shape) - 1   # edges[j] <= d2 < edges[j + 1]
        obs = (d2 >= 0.0) & (j >= p["min_range_bins"]) & (j < cols)                  # (a NaN d2 observes nothing)
        if p["max_range"] > 0:
            obs &= ~(d2 > np.float64(p["max_range"]) * np.float64(p["max_range"]))
    iy, ix = np.nonzero(obs)
    px, py, d2, j = px[iy, ix], py[iy, ix], d2[iy, ix], j[iy, ix]
    a = np.zeros(len(px), dtype=np.int64)
    best, second = np.zeros(len(px)), np.full(len(px), -np.inf)
    for k in range(0, len(px), _CHUNK):
        dot = c[None, :] * px[k:k + _CHUNK, None] + s[None, :] * py[k:k + _CHUNK, None]
        a[k:k + _CHUNK] = np.argmax(dot, axis=1)                                     # ties: the smallest a
        if rows > 1:
            top = np.partition(dot, rows - 2, axis=1)
            best[k:k + _CHUNK], second[k:k + _CHUNK] = top[:, rows - 1], top[:, rows - 2]
        else:
            best[k:k + _CHUNK] = dot[:, 0]
    return dict(cell=(iy + y0) * p["width"] + (ix + x0), j=j.astype(np.int64), a=a, d2=d2, px=px, py=py, best=best, second=second,
                edges=edges)


def add_batch(planes, imgs, transforms, p, cols=None, col_offset=0):
    """imgs [n, rows, row_stride] uint8 (samples at [col_offset, col_offset + cols) of a row), transforms [n, 6] -> the planes, updated
    in place and returned"""
    imgs = np.asarray(imgs)
    n, rows = imgs.shape[0], imgs.shape[1]
    cols = imgs.shape[2] - col_offset if cols is None else cols
    transforms = np.asarray(transforms, dtype=np.float64).reshape(n, 6)
    tabs = tables(rows)
    hw, lo_bin = p["range_halfwidth"], p["min_range_bins"]
    psum, pcnt, phit = (q.reshape(-1) for q in planes)
    for i in range(n):
        g = geometry(transforms[i], p, rows, cols, tabs)
        power = imgs[i][:, col_offset:col_offset + cols]
        v = np.zeros(len(g["j"]), dtype=np.uint32)
        for d in range(-hw, hw + 1):                      # the maximum over bins j - hw .. j + hw inside [min_range_bins, cols - 1]
            b = g["j"] + d
            ok = (b >= lo_bin) & (b <= cols - 1)
            v[ok] = np.maximum(v[ok], power[g["a"][ok], b[ok]])
        pcnt[g["cell"]] += np.uint32(1)                   # (a cell appears once per scan)
        psum[g["cell"]] += v
        phit[g["cell"]] += (v >= p["hit_threshold"]).astype(np.uint32)
    return planes


def render_mean(planes, min_observations=1):
    """uint8 (2 sum + cnt) / (2 cnt) on integers; 0 where cnt < min_observations (or 0)"""
    s, c = planes[0].astype(np.uint64), planes[1].astype(np.uint64)
    ok = (c >= max(min_observations, 1))
    out = np.zeros(s.shape, dtype=np.uint8)
    out[ok] = np.minimum((2 * s[ok] + c[ok]) // (2 * c[ok]), 255).astype(np.uint8)
    return out


def render_hits(planes, min_observations=1):
    """int8, nav_msgs/OccupancyGrid: -1 where cnt < min_observations (or 0), else (200 hit + cnt) / (2 cnt) in 0 .. 100"""
    c, h = planes[1].astype(np.uint64), planes[2].astype(np.uint64)
    ok = (c >= max(min_observations, 1))
    out = np.full(c.shape, -1, dtype=np.int8)
    out[ok] = ((200 * h[ok] + c[ok]) // (2 * c[ok])).astype(np.int8)
    return out
