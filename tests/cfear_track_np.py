"""CFEAR scan-to-keyframes registration and the keyframe tracker (Adolfsson et al., CFEAR radar odometry) restated in plain
Python / numpy, fp64: the arithmetic contract that csrc/cfear_track.hip implements (include/rsx.h,
rsx_cfear_register_keyframes_batch and rsx_cfear_tracker_*).  TEST INFRASTRUCTURE ONLY.  It builds on tests/cfear_np.py (the
pair rule) and changes nothing there.  PARITY UNPINNED: CFEAR's own code is not part of the reference checkout.

Poses are (x, y, yaw) with  map = R(yaw) p + (x, y).  Two operations, in this order of arithmetic (c, s = cos, sin(A.yaw)):
  compose(A, B)  = A o B       = (A.x + (c * B.x - s * B.y),  A.y + (s * B.x + c * B.y),  A.yaw + B.yaw)
  between(A, B)  = A^-1 o B    = (c * dx + s * dy,  c * dy - s * dx,  B.yaw - A.yaw)   with dx = B.x - A.x, dy = B.y - A.y
No yaw is ever wrapped: a pose's yaw is the sum of the steps that led to it.

Joint registration (register_keyframes): src records, K keyframes (1 <= K <= MAX_KEYFRAMES), each with records and a pose
P_k = (x_k, y_k, yaw_k) in the map frame, a start pose; the result is the scan's pose P = (x, y, yaw) in the map frame.
Per iteration and per keyframe k the scan's pose is taken in the keyframe's own frame:
  c_k, s_k = cos, sin(yaw_k);  yaw_r = yaw - yaw_k;  u = (x - x_k, y - y_k);  t_r = (c_k u_x + s_k u_y, c_k u_y - s_k u_x)
  q = R(yaw_r) mu_i + t_r,  m = R(yaw_r) n_i
and the correspondence of src record i in keyframe k is the pair rule's: the smallest d2 = |q - mu_j|^2 among the keyframe's
records with d2 <= r^2 and m.n_j >= cos_max, the lowest j on a tie, none allowed.  e = n_j.(q - mu_j), the Huber weight as in the
pair rule, J = (c_k n_jx - s_k n_jy, s_k n_jx + c_k n_jy, n_j.(R'(yaw_r) mu_i)).  H, g, the cost and the correspondence count are
summed over all (i, k), i outer and k inner; then the pair rule's LDL^T, pivot rule, step test and statuses 4 / 5 / 8.
Status 1: the src is empty or every keyframe is (an empty keyframe among others is skipped); status 2: any side holds more
than MAX_SURFACE_POINTS records.  With K = 1 and P_1 = (0, 0, 0) every expression reduces exactly to the pair rule's
(c_k = 1, s_k = 0, x - 0 = x, 1 * v = v, v + 0 * w = v for finite w).
`margin` is the pair rule's: the smallest distance of any decision made from its threshold.

Tracker (track / Tracker): state = the pose P of the last scan, the last motion M (the identity at first), a ring of at most
n_keyframes (records, pose) entries, oldest first.
  scan 0: P = (0, 0, 0); it is the first keyframe (flag 1); its registration result is all zero, n_keyframes used 0
  scan i: start = compose(P, M) when predict else P; registered against the whole ring (n_keyframes used = its size)
    status 0 or 8: M = between(P, P_new), P = P_new; the scan becomes a keyframe (flag 1) when, against the NEWEST keyframe's
      pose, hypot(x - x_kf, y - y_kf) > keyframe_distance or |remainder(yaw - yaw_kf, 2 pi)| > keyframe_rotation; a new keyframe
      evicts the oldest when the ring is full
    status 1, 2, 4 or 5: P = start, M unchanged; a scan of 1 .. MAX_SURFACE_POINTS records becomes the ring's ONLY entry, at
      `start` (flag 2, re-anchored); otherwise flag 0 and the ring stays
The two keyframe comparisons enter the scan's margin."""
import math

import numpy as np

import cfear_np as cf

MAX_KEYFRAMES = 4  # RSX_CFEAR_MAX_KEYFRAMES
MAX_SURFACE_POINTS = cf.MAX_SURFACE_POINTS
TWO_PI = 2.0 * math.pi

TRACK_DEFAULTS = dict(n_keyframes=3, keyframe_distance=1.5, keyframe_rotation=math.radians(5.0), predict=1)


def compose(a, b):
    c, s = math.cos(a[2]), math.sin(a[2])
    return (a[0] + (c * b[0] - s * b[1]), a[1] + (s * b[0] + c * b[1]), a[2] + b[2])


def between(a, b):
    c, s = math.cos(a[2]), math.sin(a[2])
    dx, dy = b[0] - a[0], b[1] - a[1]
    return (c * dx + s * dy, c * dy - s * dx, b[2] - a[2])


def _f64(rec):
    return tuple(rec[f].astype(np.float64) for f in ("x", "y", "nx", "ny"))


def _search(qx, qy, mx, my, kf, r2, cos_max, rows=256):
    """the pair rule's correspondence of every query in one keyframe -> (j or -1 per query, margin)"""
    kx, ky, knx, kny = kf
    best = np.full(len(qx), -1, dtype=np.int64)
    margin = math.inf
    for a in range(0, len(qx), rows):
        b = min(a + rows, len(qx))
        ex, ey = qx[a:b, None] - kx[None, :], qy[a:b, None] - ky[None, :]
        d2 = ex * ex + ey * ey
        dot = mx[a:b, None] * knx[None, :] + my[a:b, None] * kny[None, :]
        margin = min(margin, float(np.min(np.abs(d2 - r2))), float(np.min(np.abs(dot - cos_max))))
        ok = (d2 <= r2) & (dot >= cos_max)
        masked = np.where(ok, d2, np.inf)
        j = np.argmin(masked, axis=1)  # (the first minimum: the lowest j on a tie)
        has = ok.any(axis=1)
        best[a:b] = np.where(has, j, -1)
        if has.any():
            jj = np.where(has, j, 0)
            differ = (kx[None, :] != kx[jj][:, None]) | (ky[None, :] != ky[jj][:, None]) | (knx[None, :] != knx[jj][:, None]) | \
                     (kny[None, :] != kny[jj][:, None])
            other = ok & differ & has[:, None]
            if other.any():
                margin = min(margin, float(np.min(np.where(other, d2 - masked[np.arange(b - a), jj][:, None], np.inf))))
    return best, margin


def register_keyframes(src, keyframes, poses, init=(0.0, 0.0, 0.0), radius=3.5, cos_max_normal_angle=cf.COS30, huber_delta=0.1,
                       step_epsilon=1e-6, max_iterations=50, min_correspondences=6):
    """src: records; keyframes: list of K record arrays; poses: K x (x, y, yaw)
    -> dict(x, y, yaw, cost, iterations, correspondences, status, margin)"""
    assert 1 <= len(keyframes) <= MAX_KEYFRAMES and len(poses) == len(keyframes)
    x, y, yaw = (float(v) for v in init)
    res = dict(x=x, y=y, yaw=yaw, cost=0.0, iterations=0, correspondences=0, status=0, margin=math.inf)
    if len(src) == 0 or all(len(k) == 0 for k in keyframes):
        res["status"] = 1
        return res
    if len(src) > MAX_SURFACE_POINTS or any(len(k) > MAX_SURFACE_POINTS for k in keyframes):
        res["status"] = 2
        return res
    sx, sy, snx, sny = _f64(src)
    kfs = [(_f64(k), tuple(float(v) for v in p)) for k, p in zip(keyframes, poses) if len(k)]
    r2 = float(radius) * float(radius)
    delta = float(huber_delta)
    margin = math.inf
    it = 0
    status = 0
    while True:
        per_kf = []
        for kf, (xk, yk, yawk) in kfs:
            ck, sk = math.cos(yawk), math.sin(yawk)
            yaw_r = yaw - yawk
            ux, uy = x - xk, y - yk
            tx, ty = ck * ux + sk * uy, ck * uy - sk * ux
            c, s = math.cos(yaw_r), math.sin(yaw_r)
            qx, qy = (c * sx - s * sy) + tx, (s * sx + c * sy) + ty
            mx, my = c * snx - s * sny, s * snx + c * sny
            best, mg = _search(qx, qy, mx, my, kf, r2, cos_max_normal_angle)
            margin = min(margin, mg)
            per_kf.append((kf, ck, sk, c, s, qx, qy, best))
        H = np.zeros((3, 3))
        g = np.zeros(3)
        cost = 0.0
        nc = 0
        for i in range(len(src)):
            for kf, ck, sk, c, s, qx, qy, best in per_kf:
                j = int(best[i])
                if j < 0:
                    continue
                nx, ny = kf[2][j], kf[3][j]
                e = nx * (qx[i] - kf[0][j]) + ny * (qy[i] - kf[1][j])
                margin = min(margin, abs(abs(e) - delta))
                w = 1.0 if abs(e) <= delta else delta / abs(e)
                J = np.array([ck * nx - sk * ny, sk * nx + ck * ny, nx * (-s * sx[i] - c * sy[i]) + ny * (c * sx[i] - s * sy[i])])
                H += w * np.outer(J, J)
                g += w * J * e
                cost += 0.5 * e * e if abs(e) <= delta else delta * (abs(e) - 0.5 * delta)
                nc += 1
        res["cost"], res["correspondences"] = cost, nc
        if nc < min_correspondences:
            status = 4
            break
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
            if not (p == 0.0 and diag == 0.0):  # (decided by exact arithmetic: see cfear_np.register)
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
    res.update(x=float(x), y=float(y), yaw=float(yaw), cost=float(res["cost"]), iterations=it, status=status, margin=margin)
    return res


class Tracker:
    """the tracker's state over one sequence; push(records of one scan) -> dict(x, y, yaw, reg, keyframe, n_keyframes, margin)"""

    def __init__(self, n_keyframes=3, keyframe_distance=1.5, keyframe_rotation=math.radians(5.0), predict=1, **cfear_params):
        assert 1 <= n_keyframes <= MAX_KEYFRAMES and keyframe_distance >= 0.0 and keyframe_rotation >= 0.0
        self.n_keyframes, self.keyframe_distance, self.keyframe_rotation, self.predict = n_keyframes, keyframe_distance, keyframe_rotation, predict
        self.cfear_params = cfear_params
        self.reset()

    def reset(self):
        self.P, self.M, self.ring, self.started = (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), [], False

    def push(self, rec):
        zero = dict(x=0.0, y=0.0, yaw=0.0, cost=0.0, iterations=0, correspondences=0, status=0, margin=math.inf)
        if not self.started:
            self.started = True
            self.P, self.M, self.ring = (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), [(rec, (0.0, 0.0, 0.0))]
            return dict(x=0.0, y=0.0, yaw=0.0, reg=zero, keyframe=1, n_keyframes=0, margin=math.inf)
        start = compose(self.P, self.M) if self.predict else self.P
        used = len(self.ring)
        reg = register_keyframes(rec, [r for r, _ in self.ring], [p for _, p in self.ring], init=start, **self.cfear_params)
        margin = reg["margin"]
        flag = 0
        if reg["status"] in (0, 8):
            new = (reg["x"], reg["y"], reg["yaw"])
            self.M = between(self.P, new)
            self.P = new
            kf = self.ring[-1][1]
            dist = math.hypot(new[0] - kf[0], new[1] - kf[1])
            rot = abs(math.remainder(new[2] - kf[2], TWO_PI))
            margin = min(margin, abs(dist - self.keyframe_distance), abs(rot - self.keyframe_rotation))
            if dist > self.keyframe_distance or rot > self.keyframe_rotation:
                flag = 1
                if len(self.ring) == self.n_keyframes:
                    self.ring.pop(0)
                self.ring.append((rec, new))
        else:
            self.P = start
            if 1 <= len(rec) <= MAX_SURFACE_POINTS:
                flag = 2
                self.ring = [(rec, start)]
        return dict(x=self.P[0], y=self.P[1], yaw=self.P[2], reg=reg, keyframe=flag, n_keyframes=used, margin=margin)


def track(scans, **params):
    """scans: list of record arrays of one sequence -> list of Tracker.push results"""
    t = Tracker(**params)
    return [t.push(s) for s in scans]
