"""Case builders shared by the grid-map tests (tests/test_gridmap_restatement.py, tests/test_gpu_gridmap.py): each returns images
[n, rows, 11 + cols] uint8 (the power samples behind 11 metadata bytes, as host/odometry hands them on), transforms (n, 6) float64
and the parameters as a dict of tests/gridmap_np.py.  Small shapes: a scan of `cols` bins at 0.25 m per bin reaches about as far as the
map is wide, so footprints are cut by the map's borders and by each other."""
import math

import numpy as np

import gridmap_np as gm

META = 11


def matrices(poses):
    """(n, 3) x, y, yaw -> (n, 6) r00, r01, tx, r10, r11, ty (what coral.pose_matrices gives; restated here so that the CPU tests do
    not need the library)"""
    out = np.zeros((len(poses), 6))
    for i, (x, y, yaw) in enumerate(poses):
        c, s = math.cos(float(yaw)), math.sin(float(yaw))
        out[i] = (c, -s, x, s, c, y)
    return out


def images(rng, n, rows, cols, meta=META):
    """speckle below the default threshold with one sample in eight strong: sums, counts and hits all vary"""
    img = rng.integers(0, 256, size=(n, rows, meta + cols), dtype=np.uint8)
    weak = rng.random((n, rows, cols)) > 0.125
    img[:, :, meta:][weak] //= 3
    return img


def small_params(width, height, **kw):
    p = dict(width=width, height=height, resolution=0.5, origin_x=-13.25, origin_y=7.5, range_resolution=0.25, min_range_bins=5,
             range_halfwidth=2, hit_threshold=120, max_range=0.0)
    p.update(kw)
    return gm.params(**p)


def random_case(seed, rows, cols, width, height, n, **kw):
    """n scans at arbitrary poses in and around the map"""
    rng = np.random.default_rng(seed)
    p = small_params(width, height, **kw)
    w, h = width * p["resolution"], height * p["resolution"]
    poses = np.stack([p["origin_x"] + rng.uniform(-0.2, 1.2, n) * w, p["origin_y"] + rng.uniform(-0.2, 1.2, n) * h, rng.uniform(-np.pi, np.pi, n)], axis=1)
    return images(rng, n, rows, cols), matrices(poses), p


def border_cases(rows=64, cols=96, width=192, height=128):
    """a sensor just inside and just outside each border and each corner of the map (the footprint cut by it), and one far outside:
    -> list of (name, images, transforms, params)"""
    rng = np.random.default_rng(5)
    p = small_params(width, height)
    x0, y0 = p["origin_x"], p["origin_y"]
    x1, y1 = x0 + width * p["resolution"], y0 + height * p["resolution"]
    xm, ym = 0.5 * (x0 + x1), 0.5 * (y0 + y1)
    spots = {"left": (x0, ym), "right": (x1, ym), "bottom": (xm, y0), "top": (xm, y1), "corner00": (x0, y0), "corner10": (x1, y0),
             "corner01": (x0, y1), "corner11": (x1, y1)}
    out = []
    for name, (x, y) in spots.items():
        poses = [(x + dx, y + dy, yaw) for dx, dy, yaw in ((0.3, 0.2, 0.4), (-0.3, -0.2, -2.0), (-7.1, 5.3, 3.0))]
        out.append((name, images(rng, 3, rows, cols), matrices(poses), p))
    reach = cols * p["range_resolution"]
    far = [(x1 + reach + 1.0, ym, 0.3), (xm, y0 - reach - 1.0, 1.0), (1e6, -1e7, 2.0)]
    out.append(("far", images(rng, 3, rows, cols), matrices(far), p))
    return out


def tile_cases(rows=64, cols=96, width=192, height=128):
    """with max_range 6 m a footprint is smaller than the map's 16 m tiles: five scans around one spot (the same tiles), and five
    scans spread so that each falls on a tile of its own"""
    rng = np.random.default_rng(6)
    p = small_params(width, height, max_range=6.0)
    x0, y0 = p["origin_x"], p["origin_y"]
    same = [(x0 + 40.0 + 0.37 * i, y0 + 24.0 - 0.21 * i, 0.7 * i) for i in range(5)]
    apart = [(x0 + 8.0 + 16.0 * i, y0 + 8.0 + 16.0 * (i % 3), -0.9 * i) for i in range(5)]
    return [("same", images(rng, 5, rows, cols), matrices(same), p), ("apart", images(rng, 5, rows, cols), matrices(apart), p)]


def tie_case(rows, on_corner):
    """range_resolution 0.25, resolution 0.5, yaw 0, the sensor on a cell corner or on a cell centre: dx and dy are multiples of 0.25,
    every product exact.  On a CENTRE the squared distances 0.25 (k^2 + l^2) meet the bin edges (0.25 j)^2 wherever (k, l, j / 2) is a
    Pythagorean triple or l = 0; on a CORNER they are 0.0625 (odd^2 + odd^2), which is 2 modulo 8 and never a square: no cell lies on
    an edge there.  Rows of 4 put the diagonals px = +-py on the bisector of two beams (fp32 cos(pi / 2) = 6e-17 is absorbed)."""
    rng = np.random.default_rng(7)
    p = gm.params(width=64, height=64, resolution=0.5, origin_x=-16.0, origin_y=-16.0, range_resolution=0.25, min_range_bins=0, range_halfwidth=1,
                  hit_threshold=120, max_range=0.0)
    at = 0.0 if on_corner else 0.25
    return images(rng, 1, rows, 96), matrices([(at, at, 0.0)]), p


def exact_ties(T, p, rows, cols):
    """-> (cells whose d2 equals a bin edge exactly, cells whose two best rows tie exactly), counted over the observed cells"""
    g = gm.geometry(T, p, rows, cols)
    on_edge = int(np.count_nonzero(g["edges"][g["j"]] == g["d2"]))
    tied = int(np.count_nonzero(g["best"] == g["second"])) if rows > 1 else 0
    return on_edge, tied


def cell_margins(T, p, rows, cols):
    """for EVERY cell of the map and one scan, in metres: the distance of the cell centre to the nearest edge of any range bin, to the
    nearest of the edges that decide whether the cell is observed (the first bin used, the end of the last bin, max_range), and to the
    nearest bisector of two beams -- plain fp64 geometry, nothing of the rule's arithmetic: a pose moved by less than a margin keeps the
    cell's bin, its being observed, its row"""
    r00, r01, tx, r10, r11, ty = T
    mx = p["origin_x"] + (np.arange(p["width"]) + 0.5) * p["resolution"]
    my = p["origin_y"] + (np.arange(p["height"]) + 0.5) * p["resolution"]
    dx, dy = np.meshgrid(mx - tx, my - ty)
    px, py = r00 * dx + r10 * dy, r01 * dx + r11 * dy
    rho, rr = np.hypot(px, py), p["range_resolution"]
    b = rho / rr
    any_edge = np.abs(b - np.round(b)) * rr
    rings = [p["min_range_bins"] * rr, cols * rr] + ([p["max_range"]] if p["max_range"] > 0 else [])
    seen_edge = np.min([np.abs(rho - r) for r in rings], axis=0)
    u = np.arctan2(py, px) * rows / (2 * np.pi)
    beam = (0.5 - np.abs(u - np.round(u))) * (2 * np.pi / rows) * rho
    return any_edge, seen_edge, beam
