"""Motion (deskewing) and Doppler compensation of radar keypoints, restated in vectorised numpy: the arithmetic contract
that csrc/mocomp.hip implements.  TEST INFRASTRUCTURE ONLY.

PARITY UNPINNED: upstream's deskewing / Doppler options (ORORA, yeti_radar_odometry --doppler) are absent from the
reference checkout, so this is the written model of include/rsx.h:
  * Time: the keypoint on azimuth row a was measured tau = ((a + 0.5) / rows) * dt_scan after its scan's start.
  * Doppler (first): r = sqrt(x x + y y); r != 0: cx = x / r, sy = y / r, rc = r + beta * (vx * cx + vy * sy),
    (x, y) <- (rc * cx, rc * sy).  r == 0 leaves the point.  The sign convention of beta could not be checked on hardware.
  * Deskew: th = wz * tau; p0 = exp(tau w) p:
        x0 = (cs * x - sn * y) + (A * vx - B * vy) * tau,   y0 = (sn * x + cs * y) + (B * vx + A * vy) * tau.
  * sn, cs, A = sin th / th, B = (1 - cos th) / th are the polynomials of `poly` (Horner in u = th * th, coefficients
    (+-1.0) / k! rounded once); every product and sum stands where it is written, nothing is fused.  Truncation below 2^-53
    relative for |th| <= 0.5 (proof: csrc/mocomp.hip).  No transcendental function is evaluated.
  * A point with not |th| <= 0.5 (deskewing on) is left as measured, Doppler included, and flags its scan (STATUS_ANGLE).
  * Velocity of a pose (x, y, yaw), dst = R(yaw) src + (x, y) = exp(dt_scan w) src: th = yaw,
        d = A A + B B, vx = ((A x + B y) / d) / dt_scan, vy = ((A y - B x) / d) / dt_scan, wz = yaw / dt_scan;
    a pose with not |yaw| <= 0.5 or a non-finite x, y has none: its pair is left as measured (STATUS_ANGLE).
  * fp64 on fp32 inputs, results rounded to fp32 once.
"""
import numpy as np

DESKEW, DOPPLER = 1, 2
STATUS_ANGLE = 1
TH_MAX = 0.5
DEFAULTS = dict(dt_scan=0.25, beta=0.049, rows=400)


def _fact(n):
    r = 1
    for k in range(2, n + 1):
        r *= k
    return float(r)


# q(u) = sum_k coefficient_k u^k, k = 1 ..: sin th = th + th q_S, A = 1 + q_S; cos th = 1 + q_C; B = th / 2 + th q_D
S_COEF = [(-1.0 if k & 1 else 1.0) / _fact(2 * k + 1) for k in range(1, 7)]   # -1/3! .. +1/13!
C_COEF = [(-1.0 if k & 1 else 1.0) / _fact(2 * k) for k in range(1, 8)]       # -1/2! .. -1/14!
D_COEF = [(-1.0 if k & 1 else 1.0) / _fact(2 * k + 2) for k in range(1, 7)]   # -1/4! .. +1/14!


def _horner(coef, u):
    r = np.full_like(u, coef[-1])
    for c in coef[-2::-1]:
        r = c + u * r
    return r


def poly(th):
    """-> sn, cs, A, B at th (float64 array), the kernel's operation order"""
    th = np.asarray(th, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        u = th * th
        qs = u * _horner(S_COEF, u)
        A = 1.0 + qs
        sn = th + th * qs
        cs = 1.0 + u * _horner(C_COEF, u)
        B = 0.5 * th + th * (u * _horner(D_COEF, u))
    return sn, cs, A, B


def pose_of(vx, vy, wz, dt_scan):
    """exp(dt_scan w) -> x, y, yaw (|wz dt_scan| <= 0.5)"""
    th = np.float64(wz) * dt_scan
    _, _, A, B = poly(th)
    return (A * vx - B * vy) * dt_scan, (B * vx + A * vy) * dt_scan, th


def velocity_of(x, y, yaw, dt_scan):
    """log(pose) / dt_scan -> vx, vy, wz, ok (arrays); ok False: the pose has no velocity here"""
    x, y, yaw = (np.asarray(v, dtype=np.float64) for v in (x, y, yaw))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        ok = (np.abs(yaw) <= TH_MAX) & np.isfinite(x) & np.isfinite(y)
        _, _, A, B = poly(yaw)
        d = A * A + B * B
        vx = ((A * x + B * y) / d) / dt_scan
        vy = ((A * y - B * x) / d) / dt_scan
        wz = yaw / dt_scan
    return vx, vy, wz, ok


def compensate(xy, rows_idx, vx, vy, wz, flags, dt_scan=0.25, beta=0.049, rows=400):
    """xy (n, 2) float32, rows_idx (n,) int, one velocity (scalars or (n,) arrays) -> (n, 2) float32, bad (n,) bool"""
    assert flags in (1, 2, 3)
    xy = np.asarray(xy, dtype=np.float32).reshape(-1, 2)
    x, y = xy[:, 0].astype(np.float64), xy[:, 1].astype(np.float64)
    a = np.asarray(rows_idx).astype(np.float64)
    vx, vy, wz = (np.broadcast_to(np.asarray(v, dtype=np.float64), x.shape) for v in (vx, vy, wz))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        tau = ((a + 0.5) / float(rows)) * dt_scan
        th = wz * tau
        bad = ~(np.abs(th) <= TH_MAX) if flags & DESKEW else np.zeros(x.shape, dtype=bool)
        if flags & DOPPLER:
            r = np.sqrt(x * x + y * y)
            nz = r != 0.0
            rr = np.where(nz, r, 1.0)
            cx, sy = x / rr, y / rr
            rc = r + beta * (vx * cx + vy * sy)
            x, y = np.where(nz, rc * cx, x), np.where(nz, rc * sy, y)
        if flags & DESKEW:
            sn, cs, A, B = poly(th)
            x, y = (cs * x - sn * y) + (A * vx - B * vy) * tau, (sn * x + cs * y) + (B * vx + A * vy) * tau
        out = np.stack([x, y], axis=1).astype(np.float32)
    out[bad] = xy[bad]
    return out, bad


def points_batch(xy, rows_idx, offsets, w, flags, **kw):
    """the contract of rsx_mocomp_points_batch -> out_xy (M, 2) float32, status (n_scans,) int32"""
    xy = np.asarray(xy, dtype=np.float32).reshape(-1, 2)
    off = np.asarray(offsets, dtype=np.int64)
    w = np.asarray(w, dtype=np.float64).reshape(-1, 3)
    out = np.empty_like(xy)
    status = np.zeros(len(off) - 1, dtype=np.int32)
    for i in range(len(off) - 1):
        sl = slice(off[i], off[i + 1])
        out[sl], bad = compensate(xy[sl], np.asarray(rows_idx)[sl], w[i, 0], w[i, 1], w[i, 2], flags, **kw)
        status[i] = STATUS_ANGLE if bad.any() else 0
    return out, status


def matches_batch(src, dst, a_cur, a_prev, offsets, pose, flags, dt_scan=0.25, **kw):
    """the contract of rsx_mocomp_matches_batch -> out_src, out_dst (M, 2) float32, status (n_pairs,) int32"""
    src = np.asarray(src, dtype=np.float32).reshape(-1, 2)
    dst = np.asarray(dst, dtype=np.float32).reshape(-1, 2)
    off = np.asarray(offsets, dtype=np.int64)
    pose = np.asarray(pose, dtype=np.float64).reshape(-1, 3)
    osrc, odst = src.copy(), dst.copy()
    status = np.zeros(len(off) - 1, dtype=np.int32)
    for i in range(len(off) - 1):
        sl = slice(off[i], off[i + 1])
        vx, vy, wz, ok = velocity_of(pose[i, 0], pose[i, 1], pose[i, 2], dt_scan)
        if not ok:
            status[i] = STATUS_ANGLE
            continue
        osrc[sl], b1 = compensate(src[sl], np.asarray(a_cur)[sl], vx, vy, wz, flags, dt_scan=dt_scan, **kw)
        odst[sl], b2 = compensate(dst[sl], np.asarray(a_prev)[sl], vx, vy, wz, flags, dt_scan=dt_scan, **kw)
        status[i] = STATUS_ANGLE if (b1.any() or b2.any()) else 0
    return osrc, odst, status


def same_bits(a, b):
    """fp32 arrays equal bit for bit, NaNs matching NaNs whatever their payload"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))
