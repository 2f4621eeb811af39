"""tests/cfear_mocomp_np.py, the arithmetic contract of CFEAR's motion compensation (timed surface points, compensation of
records, the two-pass tracker), against what it must mean.  CPU only.

Measured with this file (the room of cfear_track_cases.room64, 54 records a scan, each measured at the time its bearing implies):
  drive                                   | what                    | no compensation | two passes
  constant (1.0, 0.2, 0.06 rad) per scan, | worst relative error    | 0.0115 m        | 0.0022 m
    9 scans                               | end of trajectory       | 0.0724 m        | 0.0047 m
  accelerating, then turning in, 10 scans | end of trajectory       | 0.3068 m        | 0.0172 m
  pass 2 takes 2 - 4 iterations; the smallest decision margin is 7.8e-8 (constant: 1.0e-7).
The asserted bounds are twice the compensated figures (libm differences), and far below the uncompensated ones.
Point level (the same walls as points every 0.35 m with 5 cm of roughness, 400 rows, a record's time the circular mean of its
neighbours' rows; 37 - 45 records a scan): end of trajectory 0.0276 m -> 0.0210 m (constant), 0.3092 m -> 0.0152 m (accelerating):
averaging the neighbours' times costs little against the records' own times.
PARITY UNPINNED w.r.t. CFEAR's own code, which is not in the reference checkout."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cfear_mocomp_cases as mcases  # noqa: E402
import cfear_mocomp_np as cm  # noqa: E402
import cfear_np as cf  # noqa: E402
import cfear_track_cases as cases  # noqa: E402
import cfear_track_np as ct  # noqa: E402
import mocomp_np as mc  # noqa: E402

# twice the restatement's own compensated figures (see above)
END_BOUND = {"constant": 2 * 0.0047, "accelerating": 2 * 0.0172}
REL_BOUND = {"constant": 2 * 0.0022}


def test_zero_motion_is_the_identity_on_bytes():
    rec = cases.as_records(cases.room64())
    rec["x"][0], rec["y"][1] = -0.0, -0.0  # (a product with cs = 1 and a sum with 0 would turn -0 into +0)
    rec["nx"][2] = np.float32("nan")
    tau = np.linspace(0.0, 1.0, len(rec)).astype(np.float32)
    out, status = cm.compensate(rec, tau, (0.0, 0.0, 0.0))
    assert status == 0 and out.tobytes() == rec.tobytes()
    # every other field is copied, whatever the motion; a motion without a velocity leaves the records and flags them
    out, status = cm.compensate(rec, tau, (0.3, -0.1, 0.02))
    assert status == 0 and all(np.array_equal(out[f], rec[f]) for f in ("lambda_max", "lambda_min", "n_points", "cell"))
    assert not np.array_equal(out["x"][3:], rec["x"][3:])
    for bad in ((0.1, 0.0, 0.5000001), (0.1, 0.0, float("nan")), (float("inf"), 0.0, 0.0)):
        out, status = cm.compensate(rec, tau, bad)
        assert status == 1 and out.tobytes() == rec.tobytes()
    assert cm.compensate(rec, tau, (0.1, 0.0, 0.5))[1] == 0


def test_compensation_is_mocomps_deskew_of_the_mean_and_a_rotation_of_the_normal():
    rec = cases.as_records(cases.room64())
    rows = np.arange(len(rec)) * 7 % 400
    tau = ((rows + 0.5) / 400.0).astype(np.float32)
    motion = (0.8, -0.2, 0.05)
    out, _ = cm.compensate(rec, tau, motion)
    vx, vy, wz, ok = mc.velocity_of(*motion, 1.0)
    want, bad = mc.compensate(np.stack([rec["x"], rec["y"]], axis=1), rows, vx, vy, wz, mc.DESKEW, dt_scan=1.0, rows=400)
    assert ok and not bad.any()
    # (mocomp takes tau in fp64 from the row, here it is a float32: equal to a few ulp of the float32 result)
    assert np.allclose(np.stack([out["x"], out["y"]], axis=1), want, rtol=0, atol=1e-5)
    assert np.allclose(np.hypot(out["nx"], out["ny"]), 1.0, atol=1e-6)
    # a point measured at the end of the period under exp(w) = motion lands where the motion takes it
    one = rec[:1].copy()
    moved, _ = cm.compensate(one, np.ones(1, dtype=np.float32), motion)
    c, s = math.cos(motion[2]), math.sin(motion[2])
    assert abs(moved["x"][0] - (c * one["x"][0] - s * one["y"][0] + motion[0])) < 1e-5
    assert abs(moved["y"][0] - (s * one["x"][0] + c * one["y"][0] + motion[1])) < 1e-5


def test_compensate_0_equals_the_plain_tracker():
    for name in mcases.DRIVES:
        scans, taus, _ = mcases.drive(name)
        plain = ct.track(scans)
        off = mcases.drive_track(name, compensate=0)
        for a, b in zip(off, plain):
            assert (a["x"], a["y"], a["yaw"], a["keyframe"], a["n_keyframes"]) == (b["x"], b["y"], b["yaw"], b["keyframe"], b["n_keyframes"])
            assert all(a["reg"][f] == b["reg"][f] for f in b["reg"]) and a["reg"]["reserved"] == 0


def test_timed_surface_points_keep_the_records_and_take_a_circular_mean():
    xy, rows, n_rows = mcases.seam_cloud()
    rec, tau, status = cm.surface_points_timed(xy, rows, n_rows)
    plain, _ = cf.surface_points(xy)
    assert status == 0 and rec.tobytes() == plain.tobytes() and len(rec) == 4
    seam = tau[rec["x"] > 0]
    far = tau[rec["x"] < 0]
    assert len(seam) == 2 and len(far) == 2
    for t in seam:  # within 2 / n_rows of the seam, not at 0.5 where a plain mean of the rows puts it
        assert min(float(t), 1.0 - float(t)) <= 2.0 / n_rows, t
    plain_mean = (float(np.mean(rows[:12])) + 0.5) / n_rows
    assert 0.4 < plain_mean < 0.6
    for t in far:  # away from the seam the circular mean is the plain mean
        assert abs(float(t) - (float(np.mean(rows[12:])) + 0.5) / n_rows) < 1e-6
    # one row only, an even count, the first neighbour on either side of the seam
    assert cm.record_tau(np.zeros(6, dtype=np.int64), 1) == np.float32(0.5)
    assert cm.record_tau(np.array([399, 0]), 400) == np.float32(0.0) and cm.record_tau(np.array([0, 399]), 400) == np.float32(0.0)
    assert cm.record_tau(np.array([398, 399]), 400) == np.float32(399.0 / 400.0)
    assert cm.record_tau(np.array([0, 200]), 400) == np.float32(300.5 / 400.0)  # (opposite rows: d = -h, the mean lands before row 0 and is wrapped)


@pytest.mark.parametrize("name", list(mcases.DRIVES))
def test_two_passes_beat_no_compensation_on_the_room_drives(name):
    drive = mcases.DRIVES[name]
    off, on = mcases.drive_track(name, compensate=0), mcases.drive_track(name)
    e_off, e_on = cm.end_error(off, drive), cm.end_error(on, drive)
    r_off, r_on = cm.worst_relative_error(off, drive), cm.worst_relative_error(on, drive)
    print(f"{name}: end of trajectory {e_off:.4f} m -> {e_on:.4f} m, worst relative {r_off:.4f} m -> {r_on:.4f} m, "
          f"pass 1 iterations {[r['reg']['reserved'] for r in on]}, pass 2 {[r['reg']['iterations'] for r in on]}, "
          f"margin {min(r['margin'] for r in on):.1e}")
    assert all(r["reg"]["status"] == 0 for r in on) and all(r["reg"]["status"] == 0 for r in off)
    assert e_on < END_BOUND[name] < e_off
    if name in REL_BOUND:
        assert r_on < REL_BOUND[name] < r_off
    assert all(2 <= r["reg"]["iterations"] <= 4 for r in on[1:])
    assert min(r["margin"] for r in on) >= 1e-9 and min(r["margin"] for r in off) >= 1e-9


def test_the_first_keyframe_is_compensated_once_the_first_motion_is_known():
    scans, taus, _ = mcases.drive("constant")
    t = cm.CompTracker(compensate=1)
    t.push(scans[0], taus[0])
    assert t.first and t.ring[0][0].tobytes() == scans[0].tobytes()
    r = t.push(scans[1], taus[1])
    assert not t.first and r["reg"]["status"] == 0 and r["reg"]["reserved"] >= 1
    want, _ = cm.compensate(scans[0], taus[0], ct.between((0.0, 0.0, 0.0), ct.compose((0.0, 0.0, 0.0), t.M)))
    # (the keyframe was compensated with pass 1's motion, not the final one: centimetres from it, where the measured scan is decimetres)
    got = t.ring[0][0]
    assert max(np.abs(got["x"] - want["x"]).max(), np.abs(got["y"] - want["y"]).max()) < 0.05
    assert max(np.abs(scans[0]["x"] - want["x"]).max(), np.abs(scans[0]["y"] - want["y"]).max()) > 0.3
    assert t.ring[0][1] == (0.0, 0.0, 0.0)


def test_pass_failures():
    scans, taus, _ = mcases.drive("constant")
    far = cases.as_records(cases.seen_from(cases.room64(), (100.0, 0.0, 0.0)))
    ftau = np.full(len(far), 0.5, dtype=np.float32)
    # pass 1 fails: the failure rule with C0, reg = reg1 (reserved 0)
    t = cm.CompTracker(compensate=1)
    for i in range(3):
        t.push(scans[i], taus[i])
    M, P = t.M, t.P
    r = t.push(far, ftau)
    assert r["reg"]["status"] == 4 and r["keyframe"] == 2 and r["reg"]["reserved"] == 0 and t.M == M
    assert (r["x"], r["y"], r["yaw"]) == ct.compose(P, M) and len(t.ring) == 1
    assert t.ring[0][0].tobytes() == cm.compensate(far, ftau, M)[0].tobytes()
    # only pass 2 fails: min_correspondences between what the two passes find (mcases.pass2_failure: 63 and 54)
    scans2, taus2, mcorr = mcases.pass2_failure()
    t = cm.CompTracker(compensate=1, min_correspondences=mcorr)
    t.push(scans2[0], taus2[0])
    r = t.push(scans2[1], taus2[1])
    assert r["reg"]["status"] == 4 and r["reg"]["reserved"] >= 1 and r["keyframe"] == 2 and len(t.ring) == 1
    assert (r["x"], r["y"], r["yaw"]) == t.P and t.ring[0][1] == t.P and t.M == ct.between((0.0, 0.0, 0.0), t.P)


def test_point_level_compensation_does_not_lose():
    for name, drive in mcases.DRIVES.items():
        off, on, n_rec = mcases.point_level(name)
        e_off, e_on = cm.end_error(off, drive), cm.end_error(on, drive)
        print(f"{name}, points: {min(n_rec)} - {max(n_rec)} records a scan, end of trajectory {e_off:.4f} m -> {e_on:.4f} m")
        assert e_on <= e_off
