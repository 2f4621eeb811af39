"""Ground-truth match sets for the motion / Doppler compensation (tests/mocomp_np.py, csrc/mocomp.hip), built ONCE so that
the CPU test (tests/test_mocomp_restatement.py) and the GPU tests see the same data.  TEST INFRASTRUCTURE ONLY.

Forward model: static world points, a sensor moving at a constant body velocity w = (vx, vy, wz) through two consecutive
scans that start dt_scan apart.  A point is measured when the beam passes it: on the azimuth row a its bearing falls in at
that moment, tau = (a + 0.5) / rows * dt_scan after its scan's start, at the position it has in the sensor frame of that
moment, exp(-(t0 + tau) w) P (sin and cos from numpy: independent of the polynomials under test); its range is then shortened
by beta (vx cos phi + vy sin phi) -- the Doppler shift the correction of include/rsx.h removes.  A share of the matches is
replaced by random points as in synth.orora_pairs.  Inliers carry no other noise: compensated with the true w they satisfy
dst = exp(dt_scan w) src to fp32 rounding.
"""
import numpy as np

ROWS, DT_SCAN, BETA = 400, 0.25, 0.049
SEED, N_PAIRS = 5201, 6
# error of a pose against the truth: translation error plus the yaw error seen at 50 m, the middle of the range band
LEVER = 50.0

# Worst pose errors (pose_error, metres) of the oracle chain on default_set(), measured on the CPU with
# the oracle only: uncompensated 0.130684, after one round of compensation (both corrections) 0.0021215.  The bound every
# implementation is held to (tests/test_mocomp_restatement.py and tests/test_gpu_odometry_mocomp.py) is 1.5 x the oracle's compensated value.
ORACLE_UNCOMPENSATED_WORST, ORACLE_COMPENSATED_WORST = 0.130684, 0.0021215
COMPENSATED_BOUND = 1.5 * ORACLE_COMPENSATED_WORST


def _exp_inv(px, py, vx, vy, wz, t):
    """exp(-t w) applied to the points: the inverse of p0 = R(th) p + V(th) (vx, vy) t, th = wz t"""
    th = wz * t
    small = np.abs(th) < 1e-9
    d = np.where(small, 1.0, th)
    A = np.where(small, 1.0, np.sin(th) / d)
    B = np.where(small, th / 2.0, (1.0 - np.cos(th)) / d)
    ux, uy = px - (A * vx - B * vy) * t, py - (B * vx + A * vy) * t
    c, s = np.cos(th), np.sin(th)
    return c * ux + s * uy, -s * ux + c * uy


def _measure(Px, Py, w, t0, rows, dt_scan, beta):
    """world points (in the frame of the sensor at time 0) as one scan starting at t0 sees them -> xy float64, row"""
    vx, vy, wz = w
    x, y = _exp_inv(Px, Py, vx, vy, wz, t0)
    a = np.zeros(len(Px), dtype=np.int64)
    for _ in range(6):   # the row whose time the bearing at that time falls in
        phi = np.mod(np.arctan2(y, x), 2 * np.pi)
        a = np.minimum((phi / (2 * np.pi) * rows).astype(np.int64), rows - 1)
        tau = (a + 0.5) / rows * dt_scan
        x, y = _exp_inv(Px, Py, vx, vy, wz, t0 + tau)
    r = np.hypot(x, y)
    rm = r - beta * (vx * x / r + vy * y / r)
    return np.stack([rm * x / r, rm * y / r], axis=1), a


def true_pose(w, dt_scan=DT_SCAN):
    vx, vy, wz = w
    th = wz * dt_scan
    A = np.sin(th) / th if abs(th) > 1e-9 else 1.0
    B = (1.0 - np.cos(th)) / th if abs(th) > 1e-9 else th / 2.0
    return np.array([(A * vx - B * vy) * dt_scan, (B * vx + A * vy) * dt_scan, th])


def pose_error(est, truth):
    return float(np.hypot(est[0] - truth[0], est[1] - truth[1]) + LEVER * abs(est[2] - truth[2]))


def moving_pairs(seed=SEED, n_pairs=N_PAIRS, k_range=(300, 600), outlier_range=(0.2, 0.4), speed=(10.0, 20.0), max_wz=0.3,
                 rows=ROWS, dt_scan=DT_SCAN, beta=BETA, max_range=120.0):
    """-> dict: src, dst (M,2) float32 (src = the later scan), a_cur, a_prev (M,) int32, offsets int64, w (n_pairs,3), pose
    (n_pairs,3) = exp(dt_scan w), inlier (M,) bool"""
    rng = np.random.default_rng(seed)
    ks = rng.integers(k_range[0], k_range[1] + 1, n_pairs)
    off = np.zeros(n_pairs + 1, dtype=np.int64)
    off[1:] = np.cumsum(ks)
    m = int(off[-1])
    out = dict(src=np.empty((m, 2), np.float32), dst=np.empty((m, 2), np.float32), a_cur=np.empty(m, np.int32), a_prev=np.empty(m, np.int32),
               offsets=off, w=np.empty((n_pairs, 3)), pose=np.empty((n_pairs, 3)), inlier=np.ones(m, dtype=bool))
    for i in range(n_pairs):
        k = int(ks[i])
        v, head = rng.uniform(*speed), rng.uniform(-0.2, 0.2)
        w = (v * np.cos(head), v * np.sin(head), rng.uniform(-max_wz, max_wz))
        r, th = rng.uniform(8.0, max_range, k), rng.uniform(0.0, 2 * np.pi, k)
        Px, Py = r * np.cos(th), r * np.sin(th)
        prev, a_prev = _measure(Px, Py, w, 0.0, rows, dt_scan, beta)
        cur, a_cur = _measure(Px, Py, w, dt_scan, rows, dt_scan, beta)
        n_out = int(rng.uniform(*outlier_range) * k)
        idx = rng.choice(k, n_out, replace=False)
        ro, to = rng.uniform(8.0, max_range, n_out), rng.uniform(0.0, 2 * np.pi, n_out)
        prev[idx] = np.stack([ro * np.cos(to), ro * np.sin(to)], axis=1)
        a_prev[idx] = np.minimum((to / (2 * np.pi) * rows).astype(np.int64), rows - 1)
        sl = slice(off[i], off[i + 1])
        out["src"][sl], out["dst"][sl], out["a_cur"][sl], out["a_prev"][sl] = cur, prev, a_cur, a_prev
        out["inlier"][off[i] + idx] = False
        out["w"][i], out["pose"][i] = w, true_pose(w, dt_scan)
    return out


_CACHE = {}


def default_set():
    """the set of the accuracy tests (built once per process; treat as read-only)"""
    if "set" not in _CACHE:
        _CACHE["set"] = moving_pairs()
    return _CACHE["set"]
