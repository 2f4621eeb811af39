"""CFEAR's family of registration objectives -- three costs, three losses, optional per-correspondence weights -- restated in plain
Python / numpy, fp64: the arithmetic contract of rsx_cfear_params.cost / loss / weights (include/rsx.h; csrc/cfear_track.hip, the
GENERAL instances).  TEST INFRASTRUCTURE ONLY.  It builds on tests/cfear_np.py, tests/cfear_track_np.py and tests/cfear_mocomp_np.py
and changes nothing there.  PARITY UNPINNED: CFEAR's own code is not part of the reference checkout.

Everything but the term a correspondence adds is cfear_track_np.register_keyframes': the frames, the correspondence rule (nearest
record within the radius whose normal passes, lowest index on a tie), the order of the sums (record outer, keyframe inner), the
LDL^T solve, the pivot and step tests, the statuses.  For a correspondence (src record i, dst record j of keyframe k):
  d = q - mu_j;  m = the src normal in the keyframe's frame;  t_j = (-n_jy, n_jx);  p' = R'(yaw_r) mu_i = (-s x_i - c y_i, c x_i - s y_i)
  a row along u with scale sc:  e = sc (u.d),  J = (sc (c_k u_x - s_k u_y), sc (s_k u_x + c_k u_y), sc (u.p'))
cost 0 (P2L): one row (n_j, 1).  1 (P2P): (n_j, 1) then (t_j, 1).  2 (P2D): (n_j, 1 / sqrt(lambda_min_j)) then
  (t_j, 1 / sqrt(lambda_max_j)); a dst record is VALID when lambda_min > 0, lambda_max >= lambda_min and both are finite, and under
  P2D a correspondence with an invalid dst record is skipped and not counted.
s2 = the sum of the rows' e^2 (one row: e e), a = sqrt(s2) (one row: |e|), delta = huber_delta:
loss 0 (Huber): w = 1 if a <= delta else delta / a;  rho = 0.5 s2 inside (one row: 0.5 e e), delta (a - 0.5 delta) outside
  1 (Cauchy): w = 1 / (1 + s2 / delta^2);  rho = (delta^2 / 2) log(1 + s2 / delta^2)
  2 (none):   w = 1;  rho = 0.5 s2
weights 0: v = 1.  1: v = (w_dir w_plan) w_num with w_dir = max(m.n_j, 0), w_plan = 2 min(p_i, p_j) / (p_i + p_j) where
  p = log(1 + lambda_max / lambda_min) of a record, w_num = 2 min(N_i, N_j) / (N_i + N_j) with N = n_points; a correspondence whose
  src or dst record is invalid is skipped and not counted.  (p_i + p_j = 0 or N_i + N_j = 0 gives a NaN or infinite weight as the
  arithmetic has it: the surface-point rule writes lambda_max >= lambda_min > 0 and n_points >= 2.)
H += (v w) J J^T and g += (v w) J e per row, n first, then t;  cost += v rho;  count += 1.
With (0, 0, 0) every expression is cfear_track_np's bit for bit (1 x = x).  `margin` is cfear_np's, the Huber threshold's on a;
Cauchy and none decide nothing.  Validity is decided on the float32 inputs exactly: no margin."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cfear_np as cf  # noqa: E402
import cfear_track_np as ct  # noqa: E402
import cfear_mocomp_np as cm  # noqa: E402

COST_P2L, COST_P2P, COST_P2D = 0, 1, 2        # RSX_CFEAR_COST_*
LOSS_HUBER, LOSS_CAUCHY, LOSS_NONE = 0, 1, 2  # RSX_CFEAR_LOSS_*
COST_NAMES, LOSS_NAMES = ("p2l", "p2p", "p2d"), ("huber", "cauchy", "none")
COMBINATIONS = tuple((c, l, w) for c in (0, 1, 2) for l in (0, 1, 2) for w in (0, 1))  # (0, 0, 0), today's, comes first
TWO_PI = ct.TWO_PI


def name_of(combo):
    return f"{COST_NAMES[combo[0]]}/{LOSS_NAMES[combo[1]]}/{'weights' if combo[2] else 'no weights'}"


def _extras(rec):
    return rec["lambda_max"].astype(np.float64), rec["lambda_min"].astype(np.float64), rec["n_points"].astype(np.float64)


def valid(lmax, lmin):
    """the validity test of a record's eigenvalues (P2D's dst records; with weights both records)"""
    return bool(lmin > 0.0 and lmax >= lmin and math.isfinite(lmax) and math.isfinite(lmin))


def register_keyframes(src, keyframes, poses, init=(0.0, 0.0, 0.0), radius=3.5, cos_max_normal_angle=cf.COS30, huber_delta=0.1,
                       step_epsilon=1e-6, max_iterations=50, min_correspondences=6, cost=0, loss=0, weights=0):
    """cfear_track_np.register_keyframes with the objective chosen by (cost, loss, weights)
    -> dict(x, y, yaw, cost, iterations, correspondences, status, margin)"""
    assert cost in (0, 1, 2) and loss in (0, 1, 2) and weights in (0, 1)
    assert 1 <= len(keyframes) <= ct.MAX_KEYFRAMES and len(poses) == len(keyframes)
    x, y, yaw = (float(v) for v in init)
    res = dict(x=x, y=y, yaw=yaw, cost=0.0, iterations=0, correspondences=0, status=0, margin=math.inf)
    if len(src) == 0 or all(len(k) == 0 for k in keyframes):
        res["status"] = 1
        return res
    if len(src) > ct.MAX_SURFACE_POINTS or any(len(k) > ct.MAX_SURFACE_POINTS for k in keyframes):
        res["status"] = 2
        return res
    sx, sy, snx, sny = ct._f64(src)
    s_lmax, s_lmin, s_n = _extras(src)
    kfs = [(ct._f64(k), _extras(k), tuple(float(v) for v in p)) for k, p in zip(keyframes, poses) if len(k)]
    r2 = float(radius) * float(radius)
    delta = float(huber_delta)
    dd = delta * delta
    margin = math.inf
    it = 0
    status = 0
    while True:
        per_kf = []
        for kf, ext, (xk, yk, yawk) in kfs:
            ck, sk = math.cos(yawk), math.sin(yawk)
            yaw_r = yaw - yawk
            ux, uy = x - xk, y - yk
            tx, ty = ck * ux + sk * uy, ck * uy - sk * ux
            c, s = math.cos(yaw_r), math.sin(yaw_r)
            qx, qy = (c * sx - s * sy) + tx, (s * sx + c * sy) + ty
            mx, my = c * snx - s * sny, s * snx + c * sny
            best, mg = ct._search(qx, qy, mx, my, kf, r2, cos_max_normal_angle)
            margin = min(margin, mg)
            per_kf.append((kf, ext, ck, sk, c, s, qx, qy, mx, my, best))
        H = np.zeros((3, 3))
        g = np.zeros(3)
        total = 0.0
        nc = 0
        for i in range(len(src)):
            for kf, ext, ck, sk, c, s, qx, qy, mx, my, best in per_kf:
                j = int(best[i])
                if j < 0:
                    continue
                nx, ny = kf[2][j], kf[3][j]
                sc0 = sc1 = v = 1.0
                if cost == COST_P2D or weights:
                    lmax_j, lmin_j = ext[0][j], ext[1][j]
                    if not valid(lmax_j, lmin_j):
                        continue
                    if cost == COST_P2D:
                        sc0, sc1 = 1.0 / math.sqrt(lmin_j), 1.0 / math.sqrt(lmax_j)
                    if weights:
                        if not valid(s_lmax[i], s_lmin[i]):
                            continue
                        w_dir = max(mx[i] * nx + my[i] * ny, 0.0)
                        p_i, p_j = math.log(1.0 + s_lmax[i] / s_lmin[i]), math.log(1.0 + lmax_j / lmin_j)
                        n_i, n_j = s_n[i], ext[2][j]
                        with np.errstate(invalid="ignore", divide="ignore"):
                            w_plan = np.float64(2.0 * min(p_i, p_j)) / np.float64(p_i + p_j)
                            w_num = np.float64(2.0 * min(n_i, n_j)) / np.float64(n_i + n_j)
                        v = float((w_dir * w_plan) * w_num)
                ex, ey = qx[i] - kf[0][j], qy[i] - kf[1][j]
                ppx, ppy = -s * sx[i] - c * sy[i], c * sx[i] - s * sy[i]
                e0 = sc0 * (nx * ex + ny * ey)
                rows = [(np.array([sc0 * (ck * nx - sk * ny), sc0 * (sk * nx + ck * ny), sc0 * (nx * ppx + ny * ppy)]), e0)]
                if cost == COST_P2L:
                    s2, a, half = e0 * e0, abs(e0), 0.5 * e0 * e0
                else:
                    ux_, uy_ = -ny, nx
                    e1 = sc1 * (ux_ * ex + uy_ * ey)
                    rows.append((np.array([sc1 * (ck * ux_ - sk * uy_), sc1 * (sk * ux_ + ck * uy_), sc1 * (ux_ * ppx + uy_ * ppy)]), e1))
                    s2 = e0 * e0 + e1 * e1
                    a, half = math.sqrt(s2), 0.5 * s2
                if loss == LOSS_HUBER:
                    margin = min(margin, abs(a - delta))
                    w = 1.0 if a <= delta else delta / a
                    rho = half if a <= delta else delta * (a - 0.5 * delta)
                elif loss == LOSS_CAUCHY:
                    z = 1.0 + s2 / dd
                    w = 1.0 / z
                    rho = (0.5 * dd) * math.log(z)
                else:
                    w, rho = 1.0, half
                vw = v * w
                for J, e in rows:
                    H += vw * np.outer(J, J)
                    g += vw * J * e
                total += v * rho
                nc += 1
        res["cost"], res["correspondences"] = total, nc
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


def register(src, dst, init=(0.0, 0.0, 0.0), **params):
    """a pair: dst as the one keyframe at the identity pose (with (0, 0, 0): cfear_np.register's result, field for field)"""
    return register_keyframes(src, [dst], [(0.0, 0.0, 0.0)], init=init, **params)


class CostTracker(cm.CompTracker):
    """cfear_mocomp_np.CompTracker with the objective chosen by cost / loss / weights among the registration parameters; push(records,
    tau).  The rules of the tracker and of the two passes are CompTracker's, restated here with this file's registration; the
    compensated copies keep the eigenvalues and counts of the records they were made from"""

    def _register(self, rec, init):
        return register_keyframes(rec, [r for r, _ in self.ring], [p for _, p in self.ring], init=init, **self.cfear_params)

    def _decide(self, rec, reg, margin, fail_pose, fail_motion):
        """after the last registration of a scan: the success and failure rules of cfear_track_np -> (flag, margin)"""
        flag = 0
        if reg["status"] in (0, 8):
            new = (reg["x"], reg["y"], reg["yaw"])
            self.M = ct.between(self.P, new)
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
            self.P = fail_pose
            if fail_motion is not None:
                self.M = fail_motion
            if 1 <= len(rec) <= ct.MAX_SURFACE_POINTS:
                flag = 2
                self.ring = [(rec, fail_pose)]
        return flag, margin

    def push(self, rec, tau=None):
        zero = dict(x=0.0, y=0.0, yaw=0.0, cost=0.0, iterations=0, correspondences=0, status=0, margin=math.inf, reserved=0)
        if self.compensate:
            assert tau is not None and len(tau) == len(rec)
        if not self.started:
            self.started = True
            self.P, self.M, self.ring = (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), [(rec, (0.0, 0.0, 0.0))]
            if self.compensate:
                self.first, self.first_tau = True, np.asarray(tau, dtype=np.float32).copy()
            return dict(x=0.0, y=0.0, yaw=0.0, reg=zero, keyframe=1, n_keyframes=0, margin=math.inf)
        start = ct.compose(self.P, self.M) if self.predict else self.P
        used = len(self.ring)
        if not self.compensate:
            reg = self._register(rec, start)
            reg["reserved"] = 0
            flag, margin = self._decide(rec, reg, reg["margin"], start, None)
            return dict(x=self.P[0], y=self.P[1], yaw=self.P[2], reg=reg, keyframe=flag, n_keyframes=used, margin=margin)
        c0, _ = cm.compensate(rec, tau, self.M)
        reg = self._register(c0, start)
        reg["reserved"] = 0
        margin = reg["margin"]
        first, self.first = self.first, False
        if reg["status"] not in (0, 8):
            flag, margin = self._decide(c0, reg, margin, start, None)
            return dict(x=self.P[0], y=self.P[1], yaw=self.P[2], reg=reg, keyframe=flag, n_keyframes=used, margin=margin)
        p1 = (reg["x"], reg["y"], reg["yaw"])
        m1 = ct.between(self.P, p1)
        if first:
            kf, pose = self.ring[0]
            self.ring = [(cm.compensate(kf, self.first_tau, m1)[0], pose)]
        c1, _ = cm.compensate(rec, tau, m1)
        it1 = reg["iterations"]
        reg = self._register(c1, p1)
        reg["reserved"] = it1
        flag, margin = self._decide(c1, reg, min(margin, reg["margin"]), p1, m1)
        return dict(x=self.P[0], y=self.P[1], yaw=self.P[2], reg=reg, keyframe=flag, n_keyframes=used, margin=margin)


def track(scans, taus=None, compensate=0, **params):
    """scans (and, with compensate, taus): the record / time arrays of one sequence -> list of CostTracker.push results"""
    t = CostTracker(compensate=compensate, **params)
    return [t.push(s, taus[i] if taus is not None else None) for i, s in enumerate(scans)]
