"""The numpy restatement of rigid RANSAC and motion-compensated RANSAC (tests/ransac_np.py, the contract of csrc/ransac.hip;
PARITY UNPINNED, upstream's sources are absent) against independent scalar code: a per-match loop in the kernel's summation
order, the sampler's literals, the selection rule as upstream's sequential loop, the Jacobian by central differences, and
recovery of the truth.

Measured on the CPU with the seeds below (fp32 inputs, coordinates up to 150 m, so half an ulp of a position is 7.6e-6 m):
  * rigid, noise-free inliers, 20-60 % outliers, 40 pairs of 300-1500 matches: worst 3.04e-7 m / 2.6e-9 rad;
  * MC, 20 sets of 600 matches, 40 % outliers, 5-20 m/s, |wz| <= 0.5 rad/s: worst velocity component 1.37e-6.
The bounds asserted are 10x those, the margin for the rounding of the inputs' positions."""
import math
import os
import sys

import numpy as np

from navtech_radar_slam_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ransac_np as rn  # noqa: E402

RIGID_T_MEASURED, RIGID_YAW_MEASURED, MC_W_MEASURED = 3.04e-7, 2.6e-9, 1.37e-6


# ---- an independent scalar version: thread / wave structure of the kernel, python floats ----
def _kernel_sum(vals):
    """vals[i] or None (not in the set), summed as the workgroup does: thread t adds i = t, t + 256, ..; xor butterfly; 4 waves"""
    t = [0.0] * 256
    for i, v in enumerate(vals):
        if v is not None:
            t[i % 256] += v
    total = 0.0
    for w in range(4):
        lanes = t[64 * w:64 * w + 64]
        for off in (32, 16, 8, 4, 2, 1):
            lanes = [lanes[k] + lanes[k ^ off] for k in range(64)]
        total = lanes[0] if w == 0 else total + lanes[0]
    return total


def _coeffs(th):
    s, c = float(np.sin(th)), float(np.cos(th))
    if abs(th) < 1e-3:
        t2 = th * th
        return s, c, 1.0 - t2 / 6.0 + t2 * t2 / 120.0, th / 2.0 - t2 * th / 24.0 + t2 * t2 * th / 720.0, -th / 3.0 + t2 * th / 30.0, 0.5 - t2 / 8.0 + t2 * t2 / 144.0
    A, B = s / th, (1.0 - c) / th
    return s, c, A, B, (c - A) / th, (s - B) / th


def _mc_match(p, q, dt, w):
    """residual and the 2 x 3 Jacobian of the prediction of one match"""
    vx, vy, wz = w
    s, c, A, B, Ap, Bp = _coeffs(wz * dt)
    rx, ry = c * p[0] - s * p[1], s * p[0] + c * p[1]
    e = (q[0] - (rx + (A * vx - B * vy) * dt), q[1] - (ry + (B * vx + A * vy) * dt))
    J = ((A * dt, B * dt), (-B * dt, A * dt),
         (dt * ((-s * p[0] - c * p[1]) + (Ap * vx - Bp * vy) * dt), dt * (rx + (Bp * vx + Ap * vy) * dt)))
    return e, J


def _gn(P, Q, T, idx, w, max_gn, eps, summer):
    """-> w, void, steps"""
    w0, it = w, 0
    while it < max_gn:
        terms = {}
        for i in idx:
            e, J = _mc_match(P[i], Q[i], T[i], w)
            d = lambda u, v: u[0] * v[0] + u[1] * v[1]
            terms[i] = (d(J[0], J[0]), d(J[0], J[1]), d(J[0], J[2]), d(J[1], J[1]), d(J[1], J[2]), d(J[2], J[2]), d(J[0], e), d(J[1], e), d(J[2], e))
        a00, a01, a02, a11, a12, a22, g0, g1, g2 = (summer([terms[i][k] if i in terms else None for i in range(len(P))]) for k in range(9))
        c00, c01, c02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
        det = a00 * c00 + a01 * c01 + a02 * c02
        if not det > 1e-12 * (a00 * a11 * a22):
            return w0, True, 0
        c11, c12, c22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
        d = ((c00 * g0 + c01 * g1 + c02 * g2) / det, (c01 * g0 + c11 * g1 + c12 * g2) / det, (c02 * g0 + c12 * g1 + c22 * g2) / det)
        if not all(math.isfinite(v) for v in d):
            return w0, True, 0
        w = (w[0] + d[0], w[1] + d[1], w[2] + d[2])
        it += 1
        if math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) < eps:
            break
    return w, False, it


def _rigid(P, Q, idx, summer):
    n = float(len(idx))
    pick = lambda f: summer([f(i) if i in idx else None for i in range(len(P))])
    pbx, pby, qbx, qby = pick(lambda i: P[i][0]) / n, pick(lambda i: P[i][1]) / n, pick(lambda i: Q[i][0]) / n, pick(lambda i: Q[i][1]) / n
    C = pick(lambda i: (P[i][0] - pbx) * (Q[i][0] - qbx) + (P[i][1] - pby) * (Q[i][1] - qby))
    S = pick(lambda i: (P[i][0] - pbx) * (Q[i][1] - qby) - (P[i][1] - pby) * (Q[i][0] - qbx))
    nrm = math.sqrt(C * C + S * S)
    c, s = (C / nrm, S / nrm) if nrm > 0.0 else (1.0, 0.0)
    return c, s, qbx - (c * pbx - s * pby), qby - (s * pbx + c * pby)


def scalar_estimate(src, dst, dt, mc, tolerance=0.35, inlier_ratio=0.9, H=100, max_gn=10, eps=1e-5, seed=0, dt_scan=0.25):
    """upstream's shape: a sequential loop over the hypotheses with the early exit, a per-match loop inside.  Everything is
    written again here except the sampler: rn.sample is shared, and test_sampler pins it with literals and splitmix64's
    published outputs."""
    P = [(float(a), float(b)) for a, b in src]
    Q = [(float(a), float(b)) for a, b in dst]
    T = [float(t) for t in dt] if mc else None
    K = len(P)
    best, best_inl, best_model, evaluated = -1, None, None, 0
    for h in range(H):
        evaluated += 1
        a, b = rn.sample(seed, h, K)
        two = lambda vals, a=a, b=b: (0.0 + vals[a]) + vals[b]   # the 2 sampled matches, in sampling order
        inl = []
        if not mc:
            model = _rigid(P, Q, {a, b}, two)
            c, s, tx, ty = model
            for i in range(K):
                ex, ey = Q[i][0] - ((c * P[i][0] - s * P[i][1]) + tx), Q[i][1] - ((s * P[i][0] + c * P[i][1]) + ty)
                if ex * ex + ey * ey < tolerance * tolerance:
                    inl.append(i)
        else:
            model, void, _ = _gn(P, Q, T, [a, b], (0.0, 0.0, 0.0), max_gn, eps, two)
            if void:
                model = None   # _gn hands back the start; a void hypothesis has no inliers whatever its model
            else:
                for i in range(K):
                    e, _ = _mc_match(P[i], Q[i], T[i], model)
                    if e[0] * e[0] + e[1] * e[1] < tolerance * tolerance:
                        inl.append(i)
        if len(inl) > best:
            best, best_inl, best_model = len(inl), inl, model
        if len(inl) > inlier_ratio * K:
            break
    out = dict(hypotheses=evaluated, inliers=best, mask=np.zeros(K, dtype=bool), status=0)
    if best < 2:
        out.update(status=4, inliers=0)
        return out
    out["mask"][best_inl] = True
    if not mc:
        c, s, tx, ty = _rigid(P, Q, set(best_inl), _kernel_sum)
        out.update(x=tx, y=ty, yaw=math.atan2(s, c))
    else:
        w, void, its = _gn(P, Q, T, best_inl, best_model, max_gn, eps, _kernel_sum)
        out.update(vx=w[0], vy=w[1], wz=w[2], gn_iterations=its)
    return out


def test_vectorised_restatement_equals_scalar_loop_rigid():
    """Rigid mode evaluates no sin / cos, and both versions add in the kernel's order (thread-strided partial sums, xor
    butterfly, waves ascending): equal to the last bit."""
    src, dst, off, _ = synth.orora_pairs(3, 4, k_range=(40, 330))
    for i in range(4):
        s, d = src[off[i]:off[i + 1]], dst[off[i]:off[i + 1]]
        for kw in (dict(), dict(seed=9, tolerance=0.2, max_iterations=17)):
            got = rn.estimate(s, d, **kw)
            want = scalar_estimate(s, d, None, False, tolerance=kw.get("tolerance", 0.35), H=kw.get("max_iterations", 100), seed=kw.get("seed", 0))
            assert (got["status"], got["hypotheses"], got["inliers"]) == (want["status"], want["hypotheses"], want["inliers"])
            assert np.array_equal(got["mask"], want["mask"])
            assert (got["x"], got["y"], got["yaw"]) == (want["x"], want["y"], want["yaw"])


def test_vectorised_restatement_equals_scalar_loop_mc():
    """MC mode: numpy's array sin / cos may differ from its scalar ones in the last bit, so the models are compared within
    1e-11 (a few ulp of 20 m/s through a 3 x 3 solve); the inlier sets are identical (margins on this data: > 1e-4 m)."""
    src, dst, dt, off, _, _ = synth.motion_distorted_pairs(8, 2, k=150)
    for i in range(2):
        s, d, t = src[off[i]:off[i + 1]], dst[off[i]:off[i + 1]], dt[off[i]:off[i + 1]]
        got = rn.estimate(s, d, t, mc=True, max_iterations=25, debug=True)
        assert got["margin"] > 1e-6
        want = scalar_estimate(s, d, t, True, H=25)
        assert (got["status"], got["hypotheses"], got["inliers"], got["gn_iterations"]) == (0, want["hypotheses"], want["inliers"], want["gn_iterations"])
        assert np.array_equal(got["mask"], want["mask"])
        assert max(abs(got[f] - want[f]) for f in ("vx", "vy", "wz")) < 1e-11


def test_sampler():
    assert (rn.SM_GAMMA, rn.SM_M1, rn.SM_M2) == (0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB)
    assert rn.mix(0) == 0xE220A8397B1DCDAF and rn.mix(1) == 0x910A2DEC89025CC1   # splitmix64's first outputs for the states 0 and 1
    assert rn.sample(0, 0, 2) == (1, 0)
    assert rn.sample(1, 7, 600) == (5, 135)
    assert rn.sample(0xDEADBEEF, 99, 16384) == (13780, 16252)
    for K in (2, 3, 5, 600, 16384):
        for seed in (0, 1, 2 ** 63 + 5):
            for h in range(200):
                a, b = rn.sample(seed, h, K)
                assert a != b and 0 <= a < K and 0 <= b < K
    # a pair's result does not depend on where it stands in a batch
    src, dst, off, _ = synth.orora_pairs(4, 3, k_range=(30, 60))
    alone = rn.estimate(src[off[1]:off[2]], dst[off[1]:off[2]], seed=5)
    batch = rn.estimate_batch(src, dst, off, seed=5)[1]
    assert alone["x"] == batch["x"] and np.array_equal(alone["mask"], batch["mask"])


def _sequential_selection(counts, K, ratio):
    best, win, n = -1, -1, 0
    for h, c in enumerate(counts):
        n += 1
        if c > best:
            best, win = c, h
        if c > ratio * K:
            break
    return n - 1, win


def test_selection_rule_equals_the_sequential_loop():
    rng = np.random.default_rng(2)
    cases = [([3, 7, 7, 2], 10, 0.9), ([5, 5, 5], 10, 0.9), ([0, 0, 0], 10, 0.9),           # ties: the lowest h
             ([2, 9, 10, 10], 10, 0.85), ([10, 10], 10, 0.9), ([1, 2, 10, 3, 10], 10, 0.9),  # early stops; a later equal count is not seen
             ([9, 10], 10, 0.9), ([10], 10, 1.0), ([4, 9, 8, 9], 10, 0.9)]                   # 9 is not above 0.9 x 10
    cases += [(rng.integers(0, 21, 50).tolist(), 20, r) for r in (0.5, 0.9, 0.95, 1.0) for _ in range(50)]
    for counts, K, ratio in cases:
        assert rn.select(counts, K, ratio) == _sequential_selection(counts, K, ratio), (counts, K, ratio)
    assert rn.select([2, 9, 10, 10], 10, 0.85) == (1, 1) and rn.select([3, 7, 7, 2], 10, 0.9) == (3, 1)


def test_mc_jacobian_equals_central_differences():
    rng = np.random.default_rng(6)
    for _ in range(200):
        p, q = rng.uniform(-150, 150, 2), rng.uniform(-150, 150, 2)
        dt = rng.uniform(0.2, 0.3)
        w = np.array([rng.uniform(-20, 20), rng.uniform(-3, 3), rng.choice([rng.uniform(-0.6, 0.6), rng.uniform(-3e-3, 3e-3), 0.0])])
        _, _, J = rn.mc_terms(p[0], p[1], q[0], q[1], dt, *w, jac=True)
        J = np.array(J).reshape(3, 2)
        for k, step in enumerate((1e-4, 1e-4, 1e-6)):
            hi, lo = w.copy(), w.copy()
            hi[k] += step
            lo[k] -= step
            eh, el = rn.mc_terms(p[0], p[1], q[0], q[1], dt, *hi), rn.mc_terms(p[0], p[1], q[0], q[1], dt, *lo)
            num = -(np.array(eh) - np.array(el)) / (2 * step)   # the prediction's derivative: the residual is q - prediction
            assert np.allclose(J[k], num, rtol=1e-6, atol=1e-6), (k, w, J[k], num)
    # both sides of the series switch agree
    for th in (rn.SERIES_BELOW * (1 - 1e-9), rn.SERIES_BELOW * (1 + 1e-9)):
        a = rn.v_coeffs(np.float64(th), np.sin(th), np.cos(th))
        assert np.allclose(a, (np.sin(th) / th, (1 - np.cos(th)) / th, -th / 3, 0.5), rtol=0, atol=2e-7)


def clean_pairs(seed, n):
    """orora_pairs without the noise: exact rigid inliers, 20-60 % outliers, fp32 inputs"""
    rng = np.random.default_rng(seed)
    S, D, off, T = [], [], [0], []
    for _ in range(n):
        k = int(rng.integers(300, 1501))
        r, th = rng.uniform(4, 150, k), rng.uniform(0, 2 * np.pi, k)
        s = np.stack([r * np.cos(th), r * np.sin(th)], 1)
        yaw, t = rng.uniform(-0.2, 0.2), rng.uniform(-2.5, 2.5, 2)
        c, sn = np.cos(yaw), np.sin(yaw)
        d = s @ np.array([[c, sn], [-sn, c]]) + t
        no = int(rng.uniform(0.2, 0.6) * k)
        oi = rng.choice(k, no, replace=False)
        ro, to = rng.uniform(4, 150, no), rng.uniform(0, 2 * np.pi, no)
        d[oi] = np.stack([ro * np.cos(to), ro * np.sin(to)], 1)
        S.append(s), D.append(d), off.append(off[-1] + k), T.append((t[0], t[1], yaw))
    return np.concatenate(S).astype(np.float32), np.concatenate(D).astype(np.float32), np.array(off), np.array(T)


def test_truth_recovery_rigid():
    src, dst, off, truth = clean_pairs(31, 40)
    res = rn.estimate_batch(src, dst, off)
    et = max(math.hypot(r["x"] - t[0], r["y"] - t[1]) for r, t in zip(res, truth))
    ey = max(abs(r["yaw"] - t[2]) for r, t in zip(res, truth))
    print(f"rigid truth recovery: worst {et:.3e} m {ey:.3e} rad")
    assert all(r["status"] == 0 for r in res)
    assert et < 10 * RIGID_T_MEASURED and ey < 10 * RIGID_YAW_MEASURED


def test_truth_recovery_mc_and_what_it_is_for():
    src, dst, dt, off, truth, inl = synth.motion_distorted_pairs(5, 20)
    assert src.dtype == np.float32 and off[1] == 600 and abs(inl.mean() - 0.6) < 1e-9
    assert np.all(np.hypot(truth[:, 0], truth[:, 1]) >= 5) and np.all(np.hypot(truth[:, 0], truth[:, 1]) <= 20) and np.all(np.abs(truth[:, 2]) <= 0.5)
    mc = rn.estimate_batch(src, dst, off, dt=dt, mc=True)
    rigid = rn.estimate_batch(src, dst, off)
    worst = max(abs(r[f] - t[k]) for r, t in zip(mc, truth) for k, f in enumerate(("vx", "vy", "wz")))
    print(f"MC truth recovery: worst velocity component {worst:.3e}")
    assert worst < 10 * MC_W_MEASURED
    for i, (m, r, t) in enumerate(zip(mc, rigid, truth)):
        assert m["status"] == 0 and np.array_equal(m["mask"], inl[off[i]:off[i + 1]])
        x, y, yaw = rn.pose_of(*t, 0.25)
        em = max(math.hypot(m["x"] - x, m["y"] - y), abs(m["yaw"] - yaw))
        er = max(math.hypot(r["x"] - x, r["y"] - y), abs(r["yaw"] - yaw))
        assert em < er, (i, em, er)   # the rigid model cannot absorb the per-match times
        v = rn.velocity_of(m["x"], m["y"], m["yaw"], 0.25)   # the documented way back from the pose
        assert max(abs(a - b) for a, b in zip(v, (m["vx"], m["vy"], m["wz"]))) < 1e-12
