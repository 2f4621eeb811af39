"""CFEAR motion compensation restated in plain Python / numpy: the arithmetic contract of the timed surface points, the
compensation of records and the two-pass tracker (include/rsx.h, rsx_cfear_surface_points_timed_batch,
rsx_cfear_compensate_batch, rsx_cfear_tracker_push_timed; csrc/cfear.hip, csrc/cfear_track.hip).  TEST INFRASTRUCTURE ONLY.  It
builds on tests/cfear_np.py, tests/cfear_track_np.py and tests/mocomp_np.py and changes nothing there.  PARITY UNPINNED: CFEAR's
own code is not part of the reference checkout.

Time of a record (surface_points_timed): the neighbours of a kept cell in the order of cfear_np.surface_points (rule 4), their
azimuth rows a_1 .. a_m of n_rows, h = n_rows // 2:
  d_k = ((a_k - a_1 + h) mod n_rows) - h   (the mod non-negative);  S = sum d_k (integers)
  u = (float(a_1) + float(S) / float(m)) + 0.5;  u < 0: u + n_rows, else u >= n_rows: u - n_rows;  tau = float32(u / n_rows)
a circular mean: neighbours on both sides of the row 0 / row n_rows - 1 seam give a time near the seam.

Compensation (compensate) of records measured at tau under motion = (x, y, yaw) over one scan period (dst = R(yaw) src + (x, y)):
  (vx, vy, wz) = mocomp_np.velocity_of(motion, dt_scan = 1);  th = wz * tau;  sn, cs, A, B = mocomp_np.poly(th)
  x' = (cs x - sn y) + (A vx - B vy) tau;  y' = (sn x + cs y) + (B vx + A vy) tau;  n' = (cs nx - sn ny, sn nx + cs ny)
fp64 in this order on the float32 fields, rounded to float32 once; every other field is copied.  A motion without a velocity
(not |yaw| <= 0.5, or not finite) leaves the records and gives status 1; a motion that is exactly (0, 0, 0) copies the records.

Tracker with compensate = 1 (CompTracker.push(records, tau); state as cfear_track_np.Tracker plus `first` and the first scan's tau):
  scan 0: the first keyframe as measured; first = True
  scan i: pass 1: C0 = comp(scan, M); reg1 = register_keyframes(C0, ring, init = start)   (start as in cfear_track_np)
    reg1 status 1, 2, 4, 5: cfear_track_np's failure rule with C0 as the scan; first = False; reg = reg1
    reg1 status 0, 8: P1 = its pose, M1 = between(P, P1); if first: the ring's only keyframe becomes comp(its records, its tau, M1)
      at its pose, first = False; C1 = comp(scan, M1); reg2 = register_keyframes(C1, ring, init = P1)
        reg2 status 0, 8: M = between(P, P2), P = P2, the keyframe decision with C1 as the keyframe's records
        reg2 fails: P = P1, M = M1; C1 becomes the ring's only entry at P1 (flag 2)
      reg = reg2 with reg["reserved"] = the iterations of pass 1
The margin of a scan is the smallest over both passes and the keyframe decision.

Generators: distorted_views (the room of cfear_track_cases.room64 seen from a sensor that moves WHILE it scans: every record
measured at the time its bearing implies) and wall_points (the same walls sampled as points with azimuth rows, for the study of
what averaging the neighbours' times costs)."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cfear_np as cf  # noqa: E402
import cfear_track_np as ct  # noqa: E402
import mocomp_np as mc  # noqa: E402

TWO_PI = 2.0 * math.pi


def record_tau(rows_nb, n_rows):
    """rows of a record's neighbours in the contract's order -> tau (np.float32)"""
    a1, h, m = int(rows_nb[0]), n_rows // 2, len(rows_nb)
    s = sum(((int(a) - a1 + h) % n_rows) - h for a in rows_nb)  # (Python's % is non-negative for a positive modulus)
    u = (float(a1) + float(s) / float(m)) + 0.5
    if u < 0.0:
        u = u + float(n_rows)
    elif u >= float(n_rows):
        u = u - float(n_rows)
    return np.float32(u / float(n_rows))


def surface_points_timed(xy, rows, n_rows, radius=3.5, min_points=6, max_condition=1e5):
    """xy (n, 2) float32, rows (n,) int in [0, n_rows) -> (records, tau (k,) float32, status): cfear_np.surface_points' records, and
    the time of each from the rows of the neighbours it was built from"""
    xy = np.asarray(xy, dtype=np.float32).reshape(-1, 2)
    rows = np.asarray(rows).astype(np.int64)
    assert len(rows) == len(xy) and 1 <= n_rows <= 65536 and (len(rows) == 0 or (rows.min() >= 0 and rows.max() < n_rows))
    rec, status = cf.surface_points(xy, radius=radius, min_points=min_points, max_condition=max_condition)
    r = float(radius)
    r2 = r * r
    cells = {}
    for i in range(len(xy)):
        x, y = float(xy[i, 0]), float(xy[i, 1])
        if not (math.isfinite(x) and math.isfinite(y)):
            continue
        fx, fy = math.floor(x / r), math.floor(y / r)
        if -cf.HALF <= fx < cf.HALF and -cf.HALF <= fy < cf.HALF:
            cells.setdefault((fy + cf.HALF) * cf.GRID + (fx + cf.HALF), []).append(i)
    tau = np.zeros(len(rec), dtype=np.float32)
    for k, cell in enumerate(rec["cell"]):
        iy, ix = divmod(int(cell), cf.GRID)
        own = cells[int(cell)]
        sx = sy = 0.0
        for i in own:
            sx = sx + float(xy[i, 0])
            sy = sy + float(xy[i, 1])
        cx, cy = sx / len(own), sy / len(own)
        nb = []
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                jx, jy = ix + dx, iy + dy
                if not (0 <= jx < cf.GRID and 0 <= jy < cf.GRID):
                    continue
                for i in cells.get(jy * cf.GRID + jx, ()):
                    ex, ey = float(xy[i, 0]) - cx, float(xy[i, 1]) - cy
                    if ex * ex + ey * ey <= r2:
                        nb.append(i)
        assert len(nb) == rec["n_points"][k]
        tau[k] = record_tau(rows[nb], n_rows)
    return rec, tau, status


def compensate(rec, tau, motion):
    """records (SP_DTYPE), tau (n,) float32, motion (x, y, yaw) -> (records, status 0 / 1)"""
    rec = np.asarray(rec, dtype=cf.SP_DTYPE)
    mx, my, myaw = (float(v) for v in motion)
    if mx == 0.0 and my == 0.0 and myaw == 0.0:
        return rec.copy(), 0
    vx, vy, wz, ok = mc.velocity_of(mx, my, myaw, 1.0)
    if not ok:
        return rec.copy(), 1
    t = np.asarray(tau, dtype=np.float32).astype(np.float64)
    assert t.shape == rec.shape
    x, y, nx, ny = (rec[f].astype(np.float64) for f in ("x", "y", "nx", "ny"))
    with np.errstate(invalid="ignore", over="ignore"):
        th = wz * t
        sn, cs, A, B = mc.poly(th)
        out = rec.copy()
        out["x"] = ((cs * x - sn * y) + (A * vx - B * vy) * t).astype(np.float32)
        out["y"] = ((sn * x + cs * y) + (B * vx + A * vy) * t).astype(np.float32)
        out["nx"] = (cs * nx - sn * ny).astype(np.float32)
        out["ny"] = (sn * nx + cs * ny).astype(np.float32)
    return out, 0


def compensate_batch(rec, tau, offsets, motions):
    """the contract of rsx_cfear_compensate_batch -> (records, status (n_scans,) int32)"""
    off = np.asarray(offsets, dtype=np.int64)
    motions = np.asarray(motions, dtype=np.float64).reshape(-1, 3)
    out = np.asarray(rec, dtype=cf.SP_DTYPE).copy()
    status = np.zeros(len(off) - 1, dtype=np.int32)
    for i in range(len(off) - 1):
        sl = slice(off[i], off[i + 1])
        out[sl], status[i] = compensate(out[sl], np.asarray(tau)[sl], motions[i])
    return out, status


class CompTracker(ct.Tracker):
    """cfear_track_np.Tracker with compensate; push(records, tau).  compensate = 0: Tracker.push(records)"""

    def __init__(self, compensate=0, **params):
        assert compensate in (0, 1)
        self.compensate = compensate
        super().__init__(**params)

    def reset(self):
        super().reset()
        self.first, self.first_tau = False, None

    def push(self, rec, tau=None):
        if not self.compensate:
            out = super().push(rec)
            out["reg"] = dict(out["reg"], reserved=0)
            return out
        assert tau is not None and len(tau) == len(rec)
        if not self.started:
            out = super().push(rec)
            out["reg"] = dict(out["reg"], reserved=0)
            self.first, self.first_tau = True, np.asarray(tau, dtype=np.float32).copy()
            return out
        start = ct.compose(self.P, self.M) if self.predict else self.P
        used = len(self.ring)
        c0, _ = compensate(rec, tau, self.M)
        reg = ct.register_keyframes(c0, [r for r, _ in self.ring], [p for _, p in self.ring], init=start, **self.cfear_params)
        reg["reserved"] = 0
        margin = reg["margin"]
        flag = 0
        first, self.first = self.first, False
        if reg["status"] not in (0, 8):
            self.P = start
            if 1 <= len(c0) <= ct.MAX_SURFACE_POINTS:
                flag = 2
                self.ring = [(c0, start)]
            return dict(x=self.P[0], y=self.P[1], yaw=self.P[2], reg=reg, keyframe=flag, n_keyframes=used, margin=margin)
        p1 = (reg["x"], reg["y"], reg["yaw"])
        m1 = ct.between(self.P, p1)
        if first:
            kf, pose = self.ring[0]
            self.ring = [(compensate(kf, self.first_tau, m1)[0], pose)]
        c1, _ = compensate(rec, tau, m1)
        it1 = reg["iterations"]
        reg = ct.register_keyframes(c1, [r for r, _ in self.ring], [p for _, p in self.ring], init=p1, **self.cfear_params)
        reg["reserved"] = it1
        margin = min(margin, reg["margin"])
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
                self.ring.append((c1, new))
        else:
            self.P, self.M = p1, m1
            if 1 <= len(c1) <= ct.MAX_SURFACE_POINTS:
                flag = 2
                self.ring = [(c1, p1)]
        return dict(x=self.P[0], y=self.P[1], yaw=self.P[2], reg=reg, keyframe=flag, n_keyframes=used, margin=margin)


def track(scans, taus, compensate=1, **params):
    """scans, taus: lists of record / time arrays of one sequence -> list of CompTracker.push results"""
    t = CompTracker(compensate=compensate, **params)
    return [t.push(s, u) for s, u in zip(scans, taus)]


# ---- generators ----
def _pose_at(tau, motion):
    """the sensor's pose at the fraction tau of a scan period, in the frame of the period's start: exp(tau w), exp(w) = motion"""
    vx, vy, wz, ok = mc.velocity_of(motion[0], motion[1], motion[2], 1.0)
    assert ok
    x, y, th = mc.pose_of(float(vx), float(vy), float(wz), tau)
    return float(x), float(y), float(th)


def _bearing_tau(px, py):
    """the fraction of the revolution at which the beam points at (px, py): bearing / 2 pi in [0, 1)"""
    return (math.atan2(py, px) % TWO_PI) / TWO_PI


def drive_poses(motions):
    """per-scan body motions -> the poses at which the scans START (scan 0 at the origin)"""
    poses = [(0.0, 0.0, 0.0)]
    for m in motions[:-1]:
        poses.append(ct.compose(poses[-1], m))
    return poses


def distorted_views(room, motions, iterations=30):
    """room: fp64 records in the map frame (cfear_track_cases.room64()); motions[i]: the body motion DURING scan i
    -> (records per scan (SP_DTYPE), tau per scan (float32), the scans' start poses).
    Record j of scan i is seen from the pose the sensor has at the time tau its bearing implies; tau solves
    tau = bearing(view(p, start_i o exp(tau w_i))) / 2 pi by fixed-point iteration from 0.5."""
    import cfear_track_cases as cases
    starts = drive_poses(motions)
    scans, taus = [], []
    for start, m in zip(starts, motions):
        out = np.zeros(len(room), dtype=cases.SP64)
        tau = np.zeros(len(room), dtype=np.float32)
        for j in range(len(room)):
            one = room[j:j + 1]
            t = 0.5
            for _ in range(iterations):
                v = cases.seen_from(one, ct.compose(start, _pose_at(t, m)))
                t = _bearing_tau(float(v["x"][0]), float(v["y"][0]))
            tau[j] = np.float32(t)
            out[j] = cases.seen_from(one, ct.compose(start, _pose_at(float(tau[j]), m)))[0]
        scans.append(cases.as_records(out))
        taus.append(tau)
    return scans, taus, starts


WALLS = ((0.0, 12.0), (math.pi / 2, 9.0), (math.pi, 14.0), (-math.pi / 2, 11.0), (0.7, 20.0), (2.4, 17.0))  # room64's: (normal angle, offset)


def wall_points(motions, n_rows=400, spacing=0.35, half_length=9.0, roughness=0.05, seed=1, iterations=30):
    """the walls of room64 sampled every `spacing` m as POINTS (`roughness`: the standard deviation of their depth in the wall, so that
    a neighbourhood is not exactly collinear, which the condition test refuses), each measured on the azimuth row its bearing implies
    while the sensor moves -> (xy per scan (n, 2) float32, rows per scan (n,) int32, the scans' start poses)"""
    rng = np.random.default_rng(seed)
    pts = []
    for th, off in WALLS:
        for along in np.arange(-half_length, half_length + 1e-9, spacing):
            d = off + roughness * rng.standard_normal()
            pts.append((math.cos(th) * d - math.sin(th) * along, math.sin(th) * d + math.cos(th) * along))
    pts = np.array(pts)
    starts = drive_poses(motions)
    clouds, rows = [], []
    for start, m in zip(starts, motions):
        xy = np.zeros((len(pts), 2), dtype=np.float32)
        a = np.zeros(len(pts), dtype=np.int32)
        for j, (wx, wy) in enumerate(pts):
            t = 0.5
            for _ in range(iterations):
                x, y, yaw = ct.compose(start, _pose_at(t, m))
                c, s = math.cos(yaw), math.sin(yaw)
                px, py = c * (wx - x) + s * (wy - y), c * (wy - y) - s * (wx - x)
                t = _bearing_tau(px, py)
            a[j] = min(int(t * n_rows), n_rows - 1)
            xy[j] = (px, py)
        clouds.append(xy)
        rows.append(a)
    return clouds, rows, starts


def end_error(track_result, motions):
    """|tracked position of the last scan - true position| in the first scan's frame.  The tracker's pose of scan i is the pose at
    which scan i is in register with scan 0: with every scan brought to its own start, the start pose of scan i"""
    truth = drive_poses(motions)[-1]
    last = track_result[-1]
    return math.hypot(last["x"] - truth[0], last["y"] - truth[1])


def worst_relative_error(track_result, motions):
    starts = drive_poses(motions)
    worst = 0.0
    for i in range(1, len(track_result)):
        a, b = track_result[i - 1], track_result[i]
        rel = ct.between((a["x"], a["y"], a["yaw"]), (b["x"], b["y"], b["yaw"]))
        want = ct.between(starts[i - 1], starts[i])
        worst = max(worst, math.hypot(rel[0] - want[0], rel[1] - want[1]))
    return worst


CONSTANT_DRIVE = tuple((1.0, 0.2, 0.06) for _ in range(9))
ACCEL_DRIVE = tuple((0.4 + 0.15 * i, 0.05 * i, 0.0) for i in range(5)) + tuple((1.0, 0.25, 0.04 + 0.02 * i) for i in range(5))
