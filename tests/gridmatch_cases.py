"""Case builders shared by the correlative-matching tests (tests/test_gridmatch_restatement.py, tests/test_gpu_gridmatch.py): likelihood
planes, clouds, priors and the parameters as dicts of tests/gridmap_np.py and tests/gridmatch_np.py.  Small maps (cells of 0.5 m), so
that a cloud as wide as the map leaves it under some candidates and not under others."""
import math

import numpy as np

import gridmap_cases as gc
import gridmatch_np as gx

SIZES = [(64, 64), (192, 128)]
N_POINTS = [0, 1, 63, 64, 65, 300, 8192]
WINDOWS = [(0, 0, 0), (1, 3, 0), (5, 0, 7), (2, 32, 32), (64, 1, 1)]   # (K, U, V)


def window(K, U, V, angle_step=0.013):
    return gx.params(angle_steps=K, x_cells=U, y_cells=V, angle_step=angle_step)


def plane(seed, p):
    return np.random.default_rng(seed).integers(0, 256, size=(p["height"], p["width"]), dtype=np.uint8)


def cloud(rng, n, p):
    """n points of the sensor frame in a disc of 0.45 map widths in radius: nearly as wide as the map, so that a prior near a border
    puts part of the cloud outside"""
    r = 0.45 * p["width"] * p["resolution"] * np.sqrt(rng.random(n))
    phi = rng.uniform(-np.pi, np.pi, n)
    return np.stack([r * np.cos(phi), r * np.sin(phi)], axis=1).astype(np.float32)


def border_priors(p):
    """-> (names, (9, 6) priors): the sensor in the middle of the map; ON each border (half the cloud outside, and a few cells more or
    fewer with the shifts); and OUTSIDE each border by the cloud's radius and 20 cells, where the far points are no longer placed (more
    than 64 cells out) and the nearest ones, 20 cells out, enter the map only under the largest shifts"""
    res, W, H = p["resolution"], p["width"], p["height"]
    x0, y0 = p["origin_x"], p["origin_y"]
    x1, y1 = x0 + W * res, y0 + H * res
    xm, ym = 0.5 * (x0 + x1) + 0.13, 0.5 * (y0 + y1) - 0.21
    out = 0.45 * W * res + 20 * res
    spots = {"in": (xm, ym, 0.4), "on_left": (x0 + 0.1, ym, -1.0), "on_right": (x1 - 0.2, ym, 2.0), "on_bottom": (xm, y0 - 0.1, 0.1),
             "on_top": (xm, y1 + 0.2, -2.5), "out_left": (x0 - out, ym, 0.7), "out_right": (x1 + out, ym, -0.3),
             "out_bottom": (xm, y0 - out, 3.0), "out_top": (xm, y1 + out, 1.3)}
    return list(spots), gc.matrices(list(spots.values()))


def volume_case(seed, width, height, K, U, V):
    """every N of N_POINTS at every prior of border_priors, one job each: -> L, clouds (list), priors (n, 6), p, mp"""
    rng = np.random.default_rng(seed)
    p = gc.small_params(width, height)
    _, priors = border_priors(p)
    clouds, pri = [], []
    for n in N_POINTS:
        for t in priors:
            clouds.append(cloud(rng, n, p))
            pri.append(t)
    return plane(seed + 1, p), clouds, np.array(pri), p, window(K, U, V)


def ragged(clouds):
    off = np.zeros(len(clouds) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(c) for c in clouds])
    xy = np.concatenate(clouds) if clouds else np.zeros((0, 2), dtype=np.float32)
    return np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2), off


def reference(L, clouds, priors, p, mp, device_entry=False):
    xy, off = ragged(clouds)
    return gx.match_batch(L, xy, off, priors, p, mp, device_entry=device_entry)


# ---- the tie order ----

def tie_zero():
    """an all-zero plane: every score is 0 -> (0, 0, 0) with EMPTY"""
    p = gc.small_params(64, 64)
    rng = np.random.default_rng(21)
    _, priors = border_priors(p)
    return np.zeros((64, 64), dtype=np.uint8), [cloud(rng, 200, p)], priors[:1], p, window(3, 4, 5)


def tie_constant():
    """a constant plane and a cloud so small that every point is inside the map under every candidate: every score is 7 n ->
    (0, 0, 0), by the smallest |k| and then the smallest u u + v v (the smallest linear index alone would give (-K, -V, -U))"""
    p = gc.small_params(64, 64)
    rng = np.random.default_rng(22)
    _, priors = border_priors(p)
    pts = (cloud(rng, 100, p) * np.float32(0.25)).astype(np.float32)   # within 3.6 m = 7.2 cells of the middle of a map 64 cells wide
    return np.full((64, 64), 7, dtype=np.uint8), [pts], priors[:1], p, window(3, 4, 5)


def tie_rotation():
    """one point on the x axis, no shifts, K = 1, angle_step 0.2: k = -1 and k = +1 turn it into two different cells, both 200, k = 0
    leaves it on a 0: the scores are 200, 0, 200 -> k = -1, the smallest linear index"""
    p = gc.gm.params(width=64, height=64, resolution=0.5, origin_x=0.0, origin_y=0.0)
    mp = window(1, 0, 0, angle_step=0.2)
    pts = np.array([[4.0, 0.0]], dtype=np.float32)
    prior = gc.matrices([(10.25, 10.25, 0.0)])
    c, s = gx.tables(mp)
    L = np.zeros((64, 64), dtype=np.uint8)
    landed = []
    for kk in (0, 2):
        ix, iy = gx.cells(pts, prior[0], c[kk], s[kk], p)
        L[iy[0], ix[0]] = 200
        landed.append((int(ix[0]), int(iy[0])))
    ix, iy = gx.cells(pts, prior[0], c[1], s[1], p)
    assert landed[0] != landed[1] and (int(ix[0]), int(iy[0])) not in landed
    return L, [pts], prior, p, mp


TIES = {"zero": (tie_zero, (0, 0, 0)), "constant": (tie_constant, (0, 0, 0)), "rotation": (tie_rotation, (-1, 0, 0))}   # -> (k, u, v)


# ---- end to end: a scan localised in a map built from its neighbours ----

E2E_ERRORS = [(3.0, -2.0, 0.03), (-5.0, 4.0, -0.05), (0.0, 0.0, 0.0)]      # prior minus truth: x, y [m], yaw [rad]
E2E_WINNERS = [(-3, -3, 2), (5, 5, -4), (0, 0, 0)]                          # (k, u, v)
E2E_WINDOW = dict(angle_steps=8, x_cells=8, y_cells=8, angle_step=0.01)
E2E_SCANS, E2E_QUERY = [0, 1, 2, 4, 5], 3


def end_to_end(synth, extract):
    """synth: the package's synth module; extract: tests/kstrongest_np.extract.  synth.polar_sequence(11, 6); a map of 384 x 384 cells
    of 1 m centred on the floor of the mean position, range_halfwidth 8, to be built from scans 0, 1, 2, 4, 5 at their true poses; the
    cloud: the default k-strongest targets of scan 3 at (bin + 0.5) 0.0595 along 2 pi row / 400, fp64 rounded to fp32
    -> imgs, transforms (6, 6), p, cloud (n, 2) float32, priors (3, 6)"""
    imgs, _, poses, _ = synth.polar_sequence(11, 6)
    centre = poses[:, :2].mean(axis=0)
    p = gc.gm.params(width=384, height=384, resolution=1.0, origin_x=float(np.floor(centre[0])) - 192.0, origin_y=float(np.floor(centre[1])) - 192.0,
                     range_halfwidth=8)
    tg = extract(imgs[E2E_QUERY], col_offset=11)
    rho = (tg[:, 1].astype(np.float64) + 0.5) * 0.0595
    phi = tg[:, 0].astype(np.float64) * 2.0 * np.pi / 400.0
    pts = np.stack([rho * np.cos(phi), rho * np.sin(phi)], axis=1).astype(np.float32)
    x, y, yaw = (float(v) for v in poses[E2E_QUERY])
    priors = gc.matrices([(x + ex, y + ey, yaw + eth) for ex, ey, eth in E2E_ERRORS])
    return imgs, gc.matrices(poses), p, pts, priors
