"""Rigid RANSAC and motion-compensated RANSAC (Burnett et al. 2021) on 2-D matches, restated in vectorised numpy: the
arithmetic contract that csrc/ransac.hip implements.  TEST INFRASTRUCTURE ONLY.

PARITY UNPINNED: upstream (yeti_radar_odometry's `Ransac` and `MotionDistortedRansac`, through the reference's ORORA
submodule) is absent from the reference checkout, so this follows the published methods as recalled.  Where upstream had
to be replaced by a choice, the choice is part of this contract:
  * 2-D (x, y, yaw) instead of 6-DoF; no Doppler term; no robust weighting in the Gauss-Newton refit.
  * Conventions of rsx_orora_register_batch: p = src, q = dst, dst = R src + t.  In MC mode every match carries
    dt = (time p was measured) - (time q was measured) in seconds and q = exp(dt w) p for the body velocity w = (vx, vy, wz).
  * The sampler is counter based (below): a pair's result depends on (seed, K) and its matches only.
  * All arithmetic is fp64 on fp32 inputs, every product and sum where it is written (the kernel is built with
    -ffp-contract=off).  Sums over a set of matches run in the kernel's order (block_sum): thread t of 256 adds its matches
    t, t + 256, ... in ascending order, the 64 lanes of a wave combine by an xor butterfly (32, 16, .. 1), the four waves are
    added in ascending order.
  * Rigid fit of a set: centroids, then C = sum a.b, S = sum a x b of the centred points, (c, s) = (C, S) / sqrt(C C + S S)
    (identity rotation when that norm is 0), t = qbar - R pbar, yaw = atan2(s, c).  No sin / cos is evaluated.
  * MC residual r = q - (R(th) p + V(th) (vx, vy) dt), th = wz dt, V = [[A, -B], [B, A]], A = sin th / th, B = (1 - cos th) / th;
    below |th| < 1e-3 (SERIES_BELOW) A, B and their derivatives come from their series up to th^5.
  * Gauss-Newton with analytic Jacobians, 3x3 normal equations by Cramer's rule.  The system is singular when
    not det > 1e-12 a00 a11 a22 (Hadamard's bound on an SPD determinant, scaled); a singular system or a non-finite step
    makes a hypothesis void (0 inliers) and ends a refit with the model it started from.
  * Selection: inlier <=> |r|^2 < tolerance^2; h_stop = first h with count_h > inlier_ratio K (H - 1 if none); the winner
    is the hypothesis with the most inliers among h <= h_stop, the lowest h on a tie.
  * Reported: `inliers` and the mask are the winner's; the model is the refit over them; `hypotheses` = h_stop + 1.
"""
import numpy as np

MASK64 = (1 << 64) - 1
# splitmix64: the increment and the two multipliers of its output function, shifts 30, 27, 31
SM_GAMMA, SM_M1, SM_M2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
SERIES_BELOW = 1e-3
SINGULAR_REL = 1e-12
MAX_K = 16384
NT = 256

DEFAULTS = dict(tolerance=0.35, inlier_ratio=0.90, max_iterations=100, max_gn_iterations=10, gn_epsilon=1e-5, seed=0, dt_scan=0.25)


def mix(z):
    z = (z + SM_GAMMA) & MASK64
    z = ((z ^ (z >> 30)) * SM_M1) & MASK64
    z = ((z ^ (z >> 27)) * SM_M2) & MASK64
    return z ^ (z >> 31)


def sample(seed, h, K):
    """the two distinct match indices of hypothesis h of a pair of K >= 2 matches"""
    a = mix(seed ^ mix(2 * h)) % K
    b = mix(seed ^ mix(2 * h + 1)) % (K - 1)
    return a, b + (b >= a)


def block_sum(v):
    """sum over the last axis (matches) in the kernel's order; v (..., K) float64"""
    v = np.asarray(v, dtype=np.float64)
    K = v.shape[-1]
    J = max(1, -(-K // NT))
    pad = np.zeros(v.shape[:-1] + (J * NT,))
    pad[..., :K] = v
    a = pad.reshape(v.shape[:-1] + (J, NT))
    t = np.zeros(v.shape[:-1] + (NT,))
    for j in range(J):
        t = t + a[..., j, :]
    w = t.reshape(v.shape[:-1] + (NT // 64, 64))
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        w = w + w[..., lane ^ off]
    r = np.zeros(v.shape[:-1])
    for k in range(NT // 64):
        r = r + w[..., k, 0]
    return r


def _seq_sum(v):
    """(0 + v[..., 0]) + v[..., 1] + ...: the order of a 2-match subset"""
    r = np.zeros(v.shape[:-1])
    for k in range(v.shape[-1]):
        r = r + v[..., k]
    return r


def rigid_fit(px, py, qx, qy, m, n, sum_fn):
    """rigid fit over the matches where m (bool, broadcast against the points) -> c, s, tx, ty"""
    z = lambda v: np.where(m, v, 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        pbx, pby, qbx, qby = sum_fn(z(px)) / n, sum_fn(z(py)) / n, sum_fn(z(qx)) / n, sum_fn(z(qy)) / n
        ax, ay = px - pbx[..., None], py - pby[..., None]
        bx, by = qx - qbx[..., None], qy - qby[..., None]
        C = sum_fn(z(ax * bx + ay * by))
        S = sum_fn(z(ax * by - ay * bx))
        nrm = np.sqrt(C * C + S * S)
        ok = nrm > 0.0
        c = np.where(ok, C / np.where(ok, nrm, 1.0), 1.0)
        s = np.where(ok, S / np.where(ok, nrm, 1.0), 0.0)
    tx = qbx - (c * pbx - s * pby)
    ty = qby - (s * pbx + c * pby)
    return c, s, tx, ty


def rigid_residual2(px, py, qx, qy, c, s, tx, ty):
    ex = qx - ((c * px - s * py) + tx)
    ey = qy - ((s * px + c * py) + ty)
    return ex * ex + ey * ey


def v_coeffs(th, s, c):
    """A, B, dA/dth, dB/dth of V(th)"""
    th2 = th * th
    small = np.abs(th) < SERIES_BELOW
    d = np.where(small, 1.0, th)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        A = np.where(small, 1.0 - th2 / 6.0 + th2 * th2 / 120.0, s / d)
        B = np.where(small, th / 2.0 - th2 * th / 24.0 + th2 * th2 * th / 720.0, (1.0 - c) / d)
        Ap = np.where(small, -th / 3.0 + th2 * th / 30.0, (c - A) / d)
        Bp = np.where(small, 0.5 - th2 / 8.0 + th2 * th2 / 144.0, (s - B) / d)
    return A, B, Ap, Bp


def mc_terms(px, py, qx, qy, dt, vx, vy, wz, jac=False):
    """residual (ex, ey) of the matches under w = (vx, vy, wz) (broadcast), and with jac the three Jacobian columns of the prediction"""
    with np.errstate(invalid="ignore", over="ignore"):
        th = wz * dt
        s, c = np.sin(th), np.cos(th)
        A, B, Ap, Bp = v_coeffs(th, s, c)
        rx, ry = c * px - s * py, s * px + c * py
        ex = qx - (rx + (A * vx - B * vy) * dt)
        ey = qy - (ry + (B * vx + A * vy) * dt)
        if not jac:
            return ex, ey
        j0x, j0y = A * dt, B * dt
        j1x, j1y = -B * dt, A * dt
        j2x = dt * ((-s * px - c * py) + (Ap * vx - Bp * vy) * dt)
        j2y = dt * (rx + (Bp * vx + Ap * vy) * dt)
    return ex, ey, (j0x, j0y, j1x, j1y, j2x, j2y)


def gn_step(sums):
    """one Gauss-Newton step from the 9 sums a00 a01 a02 a11 a12 a22 g0 g1 g2 (leading axis) -> d0, d1, d2, void"""
    a00, a01, a02, a11, a12, a22, g0, g1, g2 = sums
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        c00 = a11 * a22 - a12 * a12
        c01 = a02 * a12 - a01 * a22
        c02 = a01 * a12 - a02 * a11
        det = a00 * c00 + a01 * c01 + a02 * c02
        ok = det > SINGULAR_REL * (a00 * a11 * a22)
        c11 = a00 * a22 - a02 * a02
        c12 = a01 * a02 - a00 * a12
        c22 = a00 * a11 - a01 * a01
        d0 = (c00 * g0 + c01 * g1 + c02 * g2) / det
        d1 = (c01 * g0 + c11 * g1 + c12 * g2) / det
        d2 = (c02 * g0 + c12 * g1 + c22 * g2) / det
    ok = ok & np.isfinite(d0) & np.isfinite(d1) & np.isfinite(d2)
    return d0, d1, d2, ~ok


def normal_sums(px, py, qx, qy, dt, vx, vy, wz, m, sum_fn):
    ex, ey, (j0x, j0y, j1x, j1y, j2x, j2y) = mc_terms(px, py, qx, qy, dt, vx, vy, wz, jac=True)
    z = lambda v: np.where(m, v, 0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        terms = (j0x * j0x + j0y * j0y, j0x * j1x + j0y * j1y, j0x * j2x + j0y * j2y, j1x * j1x + j1y * j1y, j1x * j2x + j1y * j2y,
                 j2x * j2x + j2y * j2y, j0x * ex + j0y * ey, j1x * ex + j1y * ey, j2x * ex + j2y * ey)
        return [sum_fn(z(t)) for t in terms]


def gauss_newton(px, py, qx, qy, dt, m, w0, max_gn, eps, sum_fn):
    """Gauss-Newton over the matches where m, for a batch of problems (leading axes of w0 / m) -> vx, vy, wz, void, iterations.
    A problem that turns void keeps the model it had."""
    vx, vy, wz = (np.array(v, dtype=np.float64) for v in w0)
    active = np.ones(vx.shape, dtype=bool)
    void = np.zeros(vx.shape, dtype=bool)
    its = np.zeros(vx.shape, dtype=np.int32)
    for _ in range(max_gn):
        if not active.any():
            break
        sums = normal_sums(px, py, qx, qy, dt, vx[..., None], vy[..., None], wz[..., None], m, sum_fn)
        d0, d1, d2, bad = gn_step(sums)
        void |= active & bad
        active &= ~bad
        vx = np.where(active, vx + d0, vx)
        vy = np.where(active, vy + d1, vy)
        wz = np.where(active, wz + d2, wz)
        its += active
        with np.errstate(invalid="ignore", over="ignore"):
            active &= ~(np.sqrt(d0 * d0 + d1 * d1 + d2 * d2) < eps)
    return vx, vy, wz, void, its


def select(counts, K, inlier_ratio):
    """-> (h_stop, winner) of the per-hypothesis inlier counts"""
    counts = np.asarray(counts)
    over = np.nonzero(counts > inlier_ratio * K)[0]
    h_stop = int(over[0]) if len(over) else len(counts) - 1
    return h_stop, int(np.argmax(counts[:h_stop + 1]))


def pose_of(vx, vy, wz, dt_scan):
    """exp(dt_scan w) -> x, y, yaw"""
    th = np.float64(wz * dt_scan)
    A, B, _, _ = v_coeffs(th, np.sin(th), np.cos(th))
    return float((A * vx - B * vy) * dt_scan), float((B * vx + A * vy) * dt_scan), float(th)


def estimate(src, dst, dt=None, mc=False, debug=False, **kw):
    """one pair: src, dst (K, 2) float32, dt (K,) float32 in MC mode -> dict of the fields of rsx_ransac_result + `mask`
    (bool (K,)); with debug also `counts` (H,), `models`, and `margin` = min over the evaluated hypotheses and the
    matches of | |r| - tolerance |."""
    prm = dict(DEFAULTS)
    prm.update(kw)
    tol, H = float(prm["tolerance"]), int(prm["max_iterations"])
    src = np.asarray(src, dtype=np.float32).reshape(-1, 2)
    dst = np.asarray(dst, dtype=np.float32).reshape(-1, 2)
    K = len(src)
    res = dict(x=0.0, y=0.0, yaw=0.0, vx=0.0, vy=0.0, wz=0.0, inliers=0, hypotheses=0, gn_iterations=0, status=0,
               mask=np.zeros(K, dtype=bool))
    if K < 2 or K > MAX_K:
        res["status"] = 1 if K < 2 else 2
        return res
    px, py, qx, qy = (v.astype(np.float64) for v in (src[:, 0], src[:, 1], dst[:, 0], dst[:, 1]))
    tm = np.asarray(dt, dtype=np.float32).astype(np.float64) if mc else None
    ab = np.array([sample(int(prm["seed"]), h, K) for h in range(H)], dtype=np.int64)  # (H, 2)
    sub = lambda v: v[ab]
    every = np.ones((H, 2), dtype=bool)
    tol2 = tol * tol
    if not mc:
        c, s, tx, ty = rigid_fit(sub(px), sub(py), sub(qx), sub(qy), every, 2.0, _seq_sum)
        r2 = rigid_residual2(px[None], py[None], qx[None], qy[None], c[:, None], s[:, None], tx[:, None], ty[:, None])
        void = np.zeros(H, dtype=bool)
        models = (c, s, tx, ty)
    else:
        z = np.zeros(H)
        vx, vy, wz, void, _ = gauss_newton(sub(px), sub(py), sub(qx), sub(qy), sub(tm), every, (z, z, z), int(prm["max_gn_iterations"]),
                                           float(prm["gn_epsilon"]), _seq_sum)
        ex, ey = mc_terms(px[None], py[None], qx[None], qy[None], tm[None], vx[:, None], vy[:, None], wz[:, None])
        with np.errstate(invalid="ignore", over="ignore"):
            r2 = ex * ex + ey * ey
        models = (vx, vy, wz)
    with np.errstate(invalid="ignore"):
        inl = (r2 < tol2) & ~void[:, None]
    counts = inl.sum(axis=1)
    h_stop, win = select(counts, K, float(prm["inlier_ratio"]))
    res["hypotheses"] = h_stop + 1
    if debug:
        with np.errstate(invalid="ignore"):
            gap = np.abs(np.sqrt(r2[:h_stop + 1][~void[:h_stop + 1]]) - tol)
        res.update(counts=counts, models=models, void=void, margin=float(np.nanmin(gap)) if gap.size else np.inf)
    if counts[win] < 2:
        res["status"] = 4
        return res
    m = inl[win]
    res["mask"], res["inliers"] = m, int(counts[win])
    n = float(counts[win])
    if not mc:
        c, s, tx, ty = rigid_fit(px, py, qx, qy, m, n, block_sum)
        res.update(x=float(tx), y=float(ty), yaw=float(np.arctan2(s, c)))
    else:
        w0 = (vx[win], vy[win], wz[win])
        fx, fy, fw, bad, its = gauss_newton(px, py, qx, qy, tm, m, w0, int(prm["max_gn_iterations"]), float(prm["gn_epsilon"]), block_sum)
        if bad:
            fx, fy, fw, its = w0[0], w0[1], w0[2], 0
        x, y, yaw = pose_of(float(fx), float(fy), float(fw), float(prm["dt_scan"]))
        res.update(x=x, y=y, yaw=yaw, vx=float(fx), vy=float(fy), wz=float(fw), gn_iterations=int(its))
    return res


def estimate_batch(src, dst, offsets, dt=None, mc=False, debug=False, **kw):
    off = np.asarray(offsets, dtype=np.int64)
    return [estimate(src[off[i]:off[i + 1]], dst[off[i]:off[i + 1]], None if dt is None else dt[off[i]:off[i + 1]], mc=mc, debug=debug, **kw)
            for i in range(len(off) - 1)]


def velocity_of(x, y, yaw, dt_scan):
    """log(pose) / dt_scan: the body velocity whose exp over dt_scan is the pose"""
    th = np.float64(yaw)
    A, B, _, _ = v_coeffs(th, np.sin(th), np.cos(th))
    d = A * A + B * B
    return float((A * x + B * y) / d / dt_scan), float((-B * x + A * y) / d / dt_scan), float(th / dt_scan)
