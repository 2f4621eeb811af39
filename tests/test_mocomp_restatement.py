"""The motion / Doppler compensation contract (tests/mocomp_np.py, what csrc/mocomp.hip implements) on the CPU: the
polynomials against a 50-digit evaluation, the velocity map's round trip, and the model against ground truth -- static points
seen from a moving sensor (tests/mocomp_cases.py) -- alone and in the two-pass scheme of rsx_odometry_set_compensation
(estimate, compensate with the estimate, estimate again) with the oracle's max-clique selection and ORORA as the estimator."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mocomp_cases as mc  # noqa: E402
import mocomp_np as mn  # noqa: E402

from mocomp_cases import COMPENSATED_BOUND, ORACLE_COMPENSATED_WORST, ORACLE_UNCOMPENSATED_WORST  # noqa: E402


def _exact(th):
    """sin, cos, sin th / th, (1 - cos th) / th to 50 digits (the last through 2 sin^2(th / 2) / th: no cancellation)"""
    import mpmath
    mpmath.mp.dps = 50
    t = mpmath.mpf(float(th))
    if th == 0.0:
        return mpmath.mpf(0), mpmath.mpf(1), mpmath.mpf(1), mpmath.mpf(0)
    return mpmath.sin(t), mpmath.cos(t), mpmath.sin(t) / t, 2 * mpmath.sin(t / 2) ** 2 / t


def test_polynomials_within_one_ulp():
    import mpmath
    rng = np.random.default_rng(7)
    ths = np.concatenate([np.linspace(-0.5, 0.5, 20001), rng.uniform(-0.5, 0.5, 6000), rng.uniform(-1e-3, 1e-3, 2000),
                          [0.0, 0.5, -0.5, 1e-300, -1e-160, 1e-9, 2.0 ** -27, np.nextafter(0.5, 0)]])
    got = mn.poly(ths)
    worst = [0.0] * 4
    for i, th in enumerate(ths):
        for j, want in enumerate(_exact(th)):
            g, w = float(got[j][i]), float(want)
            ulp = float(np.spacing(abs(w))) if w != 0.0 else 5e-324
            worst[j] = max(worst[j], abs(float((mpmath.mpf(g) - want) / mpmath.mpf(ulp))))
    print("worst error [ulp] of sin, cos, A, B:", ", ".join(f"{v:.3f}" for v in worst))
    assert max(worst) <= 1.0, worst


def test_truncation_alone_is_below_half_an_ulp():
    """the bound proved in csrc/mocomp.hip: the polynomials in exact rational arithmetic against the functions, relative"""
    from fractions import Fraction

    import mpmath
    mpmath.mp.dps = 60
    for th in (0.5, -0.5, 0.49, 0.3, 0.125):
        t = Fraction(th)
        u = t * t
        q = lambda coef: sum(Fraction(c) * u ** (k + 1) for k, c in enumerate(coef))
        exact_coef = lambda coef, f: [Fraction(-1 if (k + 1) & 1 else 1, f(k + 1)) for k in range(len(coef))]
        import math
        qs = q(exact_coef(mn.S_COEF, lambda k: math.factorial(2 * k + 1)))
        qc = q(exact_coef(mn.C_COEF, lambda k: math.factorial(2 * k)))
        qd = q(exact_coef(mn.D_COEF, lambda k: math.factorial(2 * k + 2)))
        vals = (t + t * qs, 1 + qc, 1 + qs, t / 2 + t * qd)
        for v, want in zip(vals, _exact(th)):
            rel = abs((mpmath.mpf(v.numerator) / mpmath.mpf(v.denominator) - want) / want)
            assert rel < mpmath.mpf(2) ** -53, (th, float(rel))


def test_velocity_map_round_trip():
    rng = np.random.default_rng(11)
    v, wz = rng.uniform(-25.0, 25.0, (4000, 2)), rng.uniform(-1.99, 1.99, 4000)
    wz[:3] = (0.0, 2.0, -2.0)
    for dt in (0.25, 0.1):
        x, y, yaw = mn.pose_of(v[:, 0], v[:, 1], wz * (0.25 / dt), dt)
        vx, vy, w2, ok = mn.velocity_of(x, y, yaw, dt)
        assert ok.all()
        assert max(np.abs(vx - v[:, 0]).max(), np.abs(vy - v[:, 1]).max(), np.abs(w2 - wz * (0.25 / dt)).max()) < 1e-13
        # and the reverse: log, then exp
        px, py, pyaw = rng.uniform(-6.0, 6.0, 4000), rng.uniform(-6.0, 6.0, 4000), rng.uniform(-0.5, 0.5, 4000)
        vx, vy, w2, ok = mn.velocity_of(px, py, pyaw, dt)
        x, y, yaw = mn.pose_of(vx, vy, w2, dt)
        assert ok.all() and max(np.abs(x - px).max(), np.abs(y - py).max(), np.abs(yaw - pyaw).max()) < 1e-13
    # agrees with the closed forms of tests/ransac_np.py (library sin / cos) to the same 1e-13 (values up to 6.25 m: a few ulps)
    import ransac_np as rn
    for i in range(50):
        a = rn.pose_of(v[i, 0], v[i, 1], wz[i], 0.25)
        b = mn.pose_of(v[i, 0], v[i, 1], wz[i], 0.25)
        assert max(abs(p - float(q)) for p, q in zip(a, b)) < 1e-13
    _, _, _, ok = mn.velocity_of([1.0, np.inf, 1.0, np.nan], [0.0, 0.0, 0.0, 0.0], [0.6, 0.1, np.nan, 0.1], 0.25)
    assert not ok.any()


def test_points_left_alone():
    xy = np.array([[0.0, 0.0], [10.0, -3.0], [np.nan, 1.0], [5.0, 5.0]], dtype=np.float32)
    rows = np.array([0, 399, 7, 200])
    out, bad = mn.compensate(xy, rows, 12.0, -1.0, 0.1, mn.DOPPLER)
    assert not bad.any() and out[0].tolist() == [0.0, 0.0] and np.isnan(out[2]).all() and not np.array_equal(out[1], xy[1])
    # wz tau just above 1/2 on row 399, just below on row 200: the first is left as measured, Doppler included
    wz = 0.5 / (((399 + 0.5) / 400) * 0.25) * (1 + 1e-12)
    out, bad = mn.compensate(xy, rows, 12.0, -1.0, wz, mn.DESKEW | mn.DOPPLER)
    assert bad.tolist() == [False, True, False, False] and np.array_equal(out[1], xy[1]) and not np.array_equal(out[3], xy[3])
    o, st = mn.points_batch(xy, rows, [0, 1, 1, 4], [[12.0, -1.0, wz], [0, 0, 0], [12.0, -1.0, wz]], mn.DESKEW)
    assert st.tolist() == [0, 0, 1]


def test_true_velocity_restores_the_rigid_relation():
    S = mc.default_set()
    off = S["offsets"]
    assert np.abs(S["src"]).max() < 128.0 and np.abs(S["dst"]).max() < 128.0
    # four roundings to fp32 meet in a residual (src and dst as given, src and dst as written), each at most half an ulp of
    # a coordinate below 128 m (2^-18 m) in x and in y
    bound = 4 * np.sqrt(2.0) * 2.0 ** -18
    worst = 0.0
    for i in range(len(off) - 1):
        sl = slice(off[i], off[i + 1])
        w = S["w"][i]
        s0, b1 = mn.compensate(S["src"][sl], S["a_cur"][sl], *w, mn.DESKEW | mn.DOPPLER, dt_scan=mc.DT_SCAN, beta=mc.BETA, rows=mc.ROWS)
        d0, b2 = mn.compensate(S["dst"][sl], S["a_prev"][sl], *w, mn.DESKEW | mn.DOPPLER, dt_scan=mc.DT_SCAN, beta=mc.BETA, rows=mc.ROWS)
        assert not b1.any() and not b2.any()
        x, y, yaw = S["pose"][i]
        c, s = np.cos(yaw), np.sin(yaw)
        px = c * s0[:, 0].astype(np.float64) - s * s0[:, 1] + x
        py = s * s0[:, 0].astype(np.float64) + c * s0[:, 1] + y
        e = np.hypot(px - d0[:, 0], py - d0[:, 1])[S["inlier"][sl]]
        worst = max(worst, float(e.max()))
        # without the compensation the same relation is off by a hundred times that bound and more (centimetres to decimetres:
        # the two measurements of a point lie a few rows apart, so most of the distortion is common to both)
        raw = np.hypot(c * S["src"][sl][:, 0].astype(np.float64) - s * S["src"][sl][:, 1] + x - S["dst"][sl][:, 0],
                       s * S["src"][sl][:, 0].astype(np.float64) + c * S["src"][sl][:, 1] + y - S["dst"][sl][:, 1])[S["inlier"][sl]]
        assert raw.max() > 100 * bound
    print(f"worst residual of an inlier under the true velocity: {worst:.3e} m (bound {bound:.3e})")
    assert worst < bound


def oracle_two_pass(po, S, flags):
    """oracle PMC + ORORA, the restatement with the poses of that pass, the oracle again -> first and second results"""
    tau = po.orora_default_params().tim_noise_bound

    def estimate(src, dst):
        member, info = po.pmc_select_batch(src, dst, S["offsets"], tau)
        s, d, o = po.pmc_compact(src, dst, S["offsets"], member)
        return po.orora_register_batch(s, d, o), info

    r1, i1 = estimate(S["src"], S["dst"])
    pose1 = np.stack([r1["x"], r1["y"], r1["yaw"]], axis=1)
    s2, d2, st = mn.matches_batch(S["src"], S["dst"], S["a_cur"], S["a_prev"], S["offsets"], pose1, flags, dt_scan=mc.DT_SCAN, beta=mc.BETA,
                                  rows=mc.ROWS)
    assert not st.any()
    r2, i2 = estimate(s2, d2)
    return r1, r2, i1, i2


def test_two_pass_scheme_against_the_truth(oracle):
    S = mc.default_set()
    r1, r2, _, _ = oracle_two_pass(oracle, S, mn.DESKEW | mn.DOPPLER)
    e1 = [mc.pose_error((r1["x"][i], r1["y"][i], r1["yaw"][i]), S["pose"][i]) for i in range(mc.N_PAIRS)]
    e2 = [mc.pose_error((r2["x"][i], r2["y"][i], r2["yaw"][i]), S["pose"][i]) for i in range(mc.N_PAIRS)]
    print("uncompensated:", " ".join(f"{e:.6f}" for e in e1), " worst", f"{max(e1):.6f}")
    print("compensated:  ", " ".join(f"{e:.6f}" for e in e2), " worst", f"{max(e2):.6f}")
    assert np.all(r1["status"] == 0) and np.all(r2["status"] == 0)
    for a, b in zip(e1, e2):
        assert b < a                    # strictly better on every pair
        assert a >= 3.0 * b             # the set was chosen so that the gain is at least threefold
    assert max(e2) <= COMPENSATED_BOUND
    # the recorded values are the oracle's own (they are what DESIGN.md section 4.6d quotes)
    assert abs(max(e1) - ORACLE_UNCOMPENSATED_WORST) < 1e-4 and abs(max(e2) - ORACLE_COMPENSATED_WORST) < 1e-6
