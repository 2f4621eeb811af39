"""CFEAR oriented surface points and point-to-line scan registration (Adolfsson et al., CFEAR radar odometry) restated in
plain Python / numpy: the arithmetic contract that csrc/cfear.hip implements (include/rsx.h, rsx_cfear_*).  TEST
INFRASTRUCTURE ONLY.  CFEAR's own code is not part of the reference checkout: PARITY UNPINNED, this file is the definition.

Surface points of one cloud (n points, float32 x, y, sensor frame, input order; radius r, min_points, max_condition):
  1. all arithmetic is fp64 on the float32 inputs, nothing fused, every sum sequential in the order stated here
  2. cell of a point: ix = floor(x / r), iy = floor(y / r) (the cell side is the radius: a 3 x 3 block covers the radius)
  3. a point with ix or iy outside [-64, 64) (a non-finite coordinate included) is ignored and sets STATUS_RANGE
  4. occupied cells in ascending (iy, ix); c = mean of the cell's own points (ascending input index); neighbours = the
     points p of the 3 x 3 block with (p - c).(p - c) <= r * r, visited dy = -1, 0, 1 outer, dx = -1, 0, 1 inner, ascending
     input index inside a cell
  5. fewer than min_points neighbours: no surface point
  6. mu = the neighbours' mean; S = sum (p - mu)(p - mu)^T / (m - 1)
  7. h = (sxx + syy) / 2, d = (sxx - syy) / 2, s = sqrt(d * d + sxy * sxy); lmax = h + s, lmin = h - s;
     kept iff lmin > 0 and lmax <= max_condition * lmin
  8. the normal, the eigenvector of lmin, from the row of (S - lmin I) with the larger pivot -- PINNED:
         a = sxx - lmin, b = syy - lmin;  a >= b: v = (sxy, -a)   (row 1: a vx + sxy vy = 0)
                                          else:   v = (-b, sxy)   (row 2: sxy vx + b vy = 0)
     v = (1, 0) when that v is exactly (0, 0) (an isotropic set); n = v / sqrt(vx * vx + vy * vy); n = -n when n.mu > 0
  9. one 32-byte record per kept cell in cell order: float32 x, y, nx, ny, lambda_max, lambda_min (one rounding each from
     fp64), int32 n_points, int32 cell = (iy + 64) * 128 + (ix + 64)
 10. two cells that see the same neighbour set give the same record but for `cell`; both are kept

Registration of a pair (src = the later scan's records, dst = the earlier one's, start pose; dst = R(yaw) src + (x, y)):
fp64 from the float32 records.  Per iteration, q = R mu_i + t and m = R n_i for every src record; its correspondence is the
dst record of smallest d2 = |q - mu_j|^2 among those with d2 <= r^2 and m.n_j >= cos_max (lowest j on a tie); fewer than
min_correspondences: status 4, the pose reached so far.  e = n_j.(q - mu_j), w = 1 when |e| <= delta else delta / |e|,
J = (n_jx, n_jy, n_j.(R' mu_i)); H = sum w J J^T, g = sum w J e, the step solves H step = -g by LDL^T without pivoting in
the order (x, y, yaw); a pivot not > 1e-12 x its original diagonal entry: status 5, the pose reached so far.  Otherwise
pose += step, iterations += 1; stop when ||step|| < step_epsilon (checked first), or at max_iterations (status 8).
cost = the Huber loss (e^2 / 2 inside delta, delta (|e| - delta / 2) outside) and correspondences are those of the last
linearisation made, whatever the status.  Sums here run in ascending src index; the kernel's order differs (per thread, then a
tree), which the comparison tolerance absorbs."""
import math

import numpy as np

STATUS_RANGE = 1        # RSX_CFEAR_STATUS_RANGE
STATUS_POINTS = 2       # RSX_CFEAR_STATUS_POINTS: more than MAX_POINTS points (device entries; the host entries refuse)
MAX_POINTS = 16384      # RSX_CFEAR_MAX_POINTS
MAX_SURFACE_POINTS = 4096  # RSX_CFEAR_MAX_SURFACE_POINTS
GRID = 128
HALF = 64

SP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("lambda_max", "<f4"), ("lambda_min", "<f4"),
                     ("n_points", "<i4"), ("cell", "<i4")])
assert SP_DTYPE.itemsize == 32

COS30 = 0.8660254037844387  # cos(30 deg) rounded to fp64: the default cos_max_normal_angle


def surface_points(xy, radius=3.5, min_points=6, max_condition=1e5):
    """xy: (n, 2) float32 -> (records (k,) SP_DTYPE, status word)"""
    xy = np.asarray(xy, dtype=np.float32).reshape(-1, 2)
    r = float(radius)
    r2 = r * r
    status = 0
    cells = {}
    for i in range(len(xy)):
        x, y = float(xy[i, 0]), float(xy[i, 1])
        if not (math.isfinite(x) and math.isfinite(y)):
            status |= STATUS_RANGE
            continue
        fx, fy = math.floor(x / r), math.floor(y / r)
        if not (-HALF <= fx < HALF and -HALF <= fy < HALF):
            status |= STATUS_RANGE
            continue
        cells.setdefault((fy + HALF) * GRID + (fx + HALF), []).append(i)
    out = []
    for cell in sorted(cells):
        iy, ix = divmod(cell, GRID)
        sx = sy = 0.0
        for i in cells[cell]:
            sx = sx + float(xy[i, 0])
            sy = sy + float(xy[i, 1])
        cx, cy = sx / len(cells[cell]), sy / len(cells[cell])
        nb = []
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                jx, jy = ix + dx, iy + dy
                if not (0 <= jx < GRID and 0 <= jy < GRID):
                    continue
                for i in cells.get(jy * GRID + jx, ()):
                    ex, ey = float(xy[i, 0]) - cx, float(xy[i, 1]) - cy
                    if ex * ex + ey * ey <= r2:
                        nb.append(i)
        m = len(nb)
        if m < min_points:
            continue
        sx = sy = 0.0
        for i in nb:
            sx = sx + float(xy[i, 0])
            sy = sy + float(xy[i, 1])
        mx, my = sx / m, sy / m
        sxx = syy = sxy = 0.0
        for i in nb:
            ex, ey = float(xy[i, 0]) - mx, float(xy[i, 1]) - my
            sxx = sxx + ex * ex
            syy = syy + ey * ey
            sxy = sxy + ex * ey
        sxx, syy, sxy = sxx / (m - 1), syy / (m - 1), sxy / (m - 1)
        h = (sxx + syy) / 2.0
        d = (sxx - syy) / 2.0
        s = math.sqrt(d * d + sxy * sxy)
        lmax, lmin = h + s, h - s
        if not (lmin > 0.0 and lmax <= max_condition * lmin):
            continue
        a, b = sxx - lmin, syy - lmin
        if a >= b:
            vx, vy = sxy, -a
        else:
            vx, vy = -b, sxy
        if vx == 0.0 and vy == 0.0:
            vx, vy = 1.0, 0.0
        nn = math.sqrt(vx * vx + vy * vy)
        nx, ny = vx / nn, vy / nn
        if nx * mx + ny * my > 0.0:
            nx, ny = -nx, -ny
        out.append((mx, my, nx, ny, lmax, lmin, m, cell))
    rec = np.zeros(len(out), dtype=SP_DTYPE)
    for k, o in enumerate(out):
        rec[k] = tuple(np.float32(v) for v in o[:6]) + (o[6], o[7])
    return rec, status


def _differ(dst, a, b):
    return any(dst[f][a] != dst[f][b] for f in ("x", "y", "nx", "ny"))


def register(src, dst, init=(0.0, 0.0, 0.0), radius=3.5, cos_max_normal_angle=COS30, huber_delta=0.1, step_epsilon=1e-6,
             max_iterations=50, min_correspondences=6):
    """src, dst: SP_DTYPE records -> dict(x, y, yaw, cost, iterations, correspondences, status, margin)"""
    x, y, yaw = (float(v) for v in init)
    res = dict(x=x, y=y, yaw=yaw, cost=0.0, iterations=0, correspondences=0, status=0, margin=math.inf)
    if len(src) == 0 or len(dst) == 0:
        res["status"] = 1
        return res
    if len(src) > MAX_SURFACE_POINTS or len(dst) > MAX_SURFACE_POINTS:
        res["status"] = 2
        return res
    sx, sy = src["x"].astype(np.float64), src["y"].astype(np.float64)
    snx, sny = src["nx"].astype(np.float64), src["ny"].astype(np.float64)
    dx_, dy_ = dst["x"].astype(np.float64), dst["y"].astype(np.float64)
    dnx, dny = dst["nx"].astype(np.float64), dst["ny"].astype(np.float64)
    r2 = float(radius) * float(radius)
    delta = float(huber_delta)
    margin = math.inf
    it = 0
    status = 0
    while True:
        c, s = math.cos(yaw), math.sin(yaw)
        H = np.zeros((3, 3))
        g = np.zeros(3)
        cost = 0.0
        nc = 0
        for i in range(len(src)):
            qx, qy = (c * sx[i] - s * sy[i]) + x, (s * sx[i] + c * sy[i]) + y
            mx, my = c * snx[i] - s * sny[i], s * snx[i] + c * sny[i]
            ex, ey = qx - dx_, qy - dy_
            d2 = ex * ex + ey * ey
            dot = mx * dnx + my * dny
            margin = min(margin, float(np.min(np.abs(d2 - r2))), float(np.min(np.abs(dot - cos_max_normal_angle))))
            ok = (d2 <= r2) & (dot >= cos_max_normal_angle)
            if not ok.any():
                continue
            cand = np.nonzero(ok)[0]
            j = int(cand[np.argmin(d2[cand])])  # (argmin returns the first minimum: the lowest j on a tie)
            for k in cand:
                if k != j and _differ(dst, j, k):
                    margin = min(margin, float(d2[k] - d2[j]))
            e = dnx[j] * ex[j] + dny[j] * ey[j]
            margin = min(margin, abs(abs(e) - delta))
            w = 1.0 if abs(e) <= delta else delta / abs(e)
            J = np.array([dnx[j], dny[j], dnx[j] * (-s * sx[i] - c * sy[i]) + dny[j] * (c * sx[i] - s * sy[i])])
            H += w * np.outer(J, J)
            g += w * J * e
            cost += 0.5 * e * e if abs(e) <= delta else delta * (abs(e) - 0.5 * delta)
            nc += 1
        res["cost"], res["correspondences"] = cost, nc
        if nc < min_correspondences:
            status = 4
            break
        # LDL^T without pivoting, order (x, y, yaw)
        d0 = H[0, 0]
        piv = [(d0, H[0, 0])]
        bad = not d0 > 1e-12 * H[0, 0]
        if not bad:
            l10, l20 = H[1, 0] / d0, H[2, 0] / d0
            d1 = H[1, 1] - l10 * H[1, 0]
            piv.append((d1, H[1, 1]))
            bad = not d1 > 1e-12 * H[1, 1]
        if not bad:
            l21 = (H[2, 1] - l20 * H[1, 0]) / d1
            d2_ = (H[2, 2] - l20 * H[2, 0]) - l21 * l21 * d1
            piv.append((d2_, H[2, 2]))
            bad = not d2_ > 1e-12 * H[2, 2]
        for p, diag in piv:
            # (a pivot that is exactly 0 on a diagonal entry that is exactly 0 is decided by exact arithmetic -- every product with
            # a zero normal component is 0 in any order of summation -- so it has no margin to report)
            if not (p == 0.0 and diag == 0.0):
                margin = min(margin, abs(p - 1e-12 * diag))
        if bad:
            status = 5
            break
        z0 = -g[0]
        z1 = -g[1] - l10 * z0
        z2 = (-g[2] - l20 * z0) - l21 * z1
        t2 = z2 / d2_
        t1 = z1 / d1 - l21 * t2
        t0 = (z0 / d0 - l10 * t1) - l20 * t2
        x, y, yaw = x + t0, y + t1, yaw + t2
        it += 1
        norm = math.sqrt((t0 * t0 + t1 * t1) + t2 * t2)
        margin = min(margin, abs(norm - step_epsilon))
        if norm < step_epsilon:
            break
        if it >= max_iterations:
            status = 8
            break
    res.update(x=x, y=y, yaw=yaw, iterations=it, status=status, margin=margin)
    return res


def transform(rec, pose):
    """the records moved rigidly: p' = R(yaw) p + (x, y), n' = R n (float32 again: a new input, not an exact motion)"""
    x, y, yaw = pose
    c, s = math.cos(yaw), math.sin(yaw)
    out = rec.copy()
    px, py = rec["x"].astype(np.float64), rec["y"].astype(np.float64)
    nx, ny = rec["nx"].astype(np.float64), rec["ny"].astype(np.float64)
    out["x"], out["y"] = c * px - s * py + x, s * px + c * py + y
    out["nx"], out["ny"] = c * nx - s * ny, s * nx + c * ny
    return out
