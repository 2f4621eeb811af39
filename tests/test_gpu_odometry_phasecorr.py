"""Phase correlation in the windowed odometry (rsx_odometry_set_phasecorr), as the estimator and as the fallback for the pairs the
selected estimator failed on.  The contract is BYTE EQUALITY with the stand-alone entry: a phase-correlation record carries the
rsx_phasecorr_result that Phasecorr(rows, cols, same params).register_batch(imgs, [(i, i - 1)]) returns for the pair, wherever the pair
lies in a window, a set or a call.  "Same params" includes range_resolution: the setter overwrites it with the handle's
radar_resolution (a float, 0.0595f), so the stand-alone handle is made with that value widened to double.

The small case (synth.polar_sequence(3, 6) at 64 x 512, N = 64 at 0.9 m per pixel: the disc of 32 x 0.9 m fits 511 bins of 0.0595 m)
is the shape tests/test_gpu_odometry_cfear.py cuts, and N = 64 is the smallest size the transforms are built for; it is too coarse to
hold the results to the truth, so nothing here does.  The restatement tests/phasecorr_np.py gives five distinct results on its five
consecutive pairs (x 0.10 .. 0.58 m, peak 0.31 .. 0.40, peak_ratio 0.19 .. 0.23, every status and half_turn 0); the fixture asserts
that the stand-alone results are distinct with status 0, so that equality cannot hold trivially."""
import os
import subprocess

import numpy as np
import pytest

from navtech_radar_slam_amd import synth

pytestmark = pytest.mark.gpu
HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "navtech-radar-slam_amd", "host")
OFF = synth.OXFORD_META
SMALL = dict(n=64, resolution=0.9)
K = 12


def _standalone(rows, cols, imgs, pairs, od, **fields):
    """the stand-alone entry with the parameters handle `od` runs phase correlation with"""
    from navtech_radar_slam_amd import phasecorr
    h = phasecorr.Phasecorr(rows, cols, phasecorr.params(range_resolution=float(od.params.radar_resolution), **fields))
    res = h.register_batch(imgs, pairs, col_offset=OFF)
    h.close()
    return res


def _small_odometry(**kw):
    from navtech_radar_slam_amd import odometry
    kw.setdefault("estimator", "phasecorr")
    kw.setdefault("phasecorr", SMALL)
    return odometry.Odometry(64, 512, keypoints="kstrongest", **kw)


def _check_records(res, want, first=1):
    """records first .. of `res` are the phase-correlation records of the stand-alone results `want`"""
    got = res[first:]
    assert len(got) == len(want)
    for f, g in (("x", "x"), ("y", "y"), ("yaw", "theta")):
        assert got[f].tobytes() == want[g].tobytes(), (f, got[f], want[g])
    assert np.array_equal(got["iterations"], -1 - want["half_turn"])
    assert np.array_equal(got["rot_inliers"], np.rint(want["peak"] * 1e6).astype(np.int32))
    assert np.array_equal(got["trans_inliers"], np.rint(want["peak_ratio"] * 1e6).astype(np.int32))


@pytest.fixture(scope="module")
def small():
    """(imgs, az, the stand-alone results of the ten ordered neighbour pairs as {(src, dst): record})"""
    imgs, az, _, _ = synth.polar_sequence(3, 6, rows=64, cols=512, n_buildings=120, n_poles=200, world_radius=40.0)
    assert OFF + 512 == imgs.shape[2] and 32 * 0.9 <= 511 * synth.RADAR_RESOLUTION
    pairs = [(i, i - 1) for i in range(1, 6)] + [(i - 1, i) for i in range(1, 6)]
    od = _small_odometry()
    res = _standalone(64, 512, imgs, pairs, od, **SMALL)
    od.close()
    assert not res["status"].any() and len({r.tobytes() for r in res}) == len(pairs), res
    print("stand-alone, five consecutive pairs:", res[:5])
    return imgs, az, dict(zip(pairs, res))


def test_estimate_equals_the_standalone_entry(small):
    from navtech_radar_slam_amd import odometry
    imgs, az, alone = small
    od = _small_odometry()
    res, xy = od.push(imgs, az, want_xy=True)
    od.close()
    want = np.array([alone[(i, i - 1)] for i in range(1, 6)])
    _check_records(res, want)
    assert res["status"].tolist() == [3, 0, 0, 0, 0, 0] and not res["n_matches"].any()
    # the extractor is untouched: the keypoints of the same handle with another estimator
    ref = odometry.Odometry(64, 512, keypoints="kstrongest", estimator="cfear")
    ref_res, ref_xy = ref.push(imgs, az, want_xy=True)
    ref.close()
    assert np.array_equal(res["n_keypoints"], ref_res["n_keypoints"]) and res["n_keypoints"].min() > 0
    assert all(a.tobytes() == b.tobytes() for a, b in zip(xy, ref_xy))


def test_cutting_the_sequence_into_calls_changes_nothing(small):
    imgs, az, _ = small
    od = _small_odometry()
    whole = od.push(imgs, az)
    od.reset()
    parts = np.concatenate([od.push(imgs[a:b], az) for a, b in ((0, 1), (1, 3), (3, 6))])
    od.close()
    assert parts.tobytes() == whole.tobytes()


def test_more_than_two_windows(small):
    """2 windows + 2 scans, the six scans walked back and forth: every set, both lanes and the carry; then cut at scan 70"""
    from navtech_radar_slam_amd import _rsx
    imgs, az, alone = small
    n = 2 * _rsx.lib().rsx_odometry_window() + 2
    walk = [0, 1, 2, 3, 4, 5, 4, 3, 2, 1]
    seq = [walk[i % 10] for i in range(n)]
    long_imgs = np.ascontiguousarray(imgs[seq])
    od = _small_odometry()
    res = od.push(long_imgs, az)
    want = np.array([alone[(seq[i], seq[i - 1])] for i in range(1, n)])
    _check_records(res, want)
    assert res["status"][0] == 3 and not res["status"][1:].any() and not res["n_matches"].any()
    assert {(seq[i], seq[i - 1]) for i in range(1, n)} == set(alone)
    od.reset()
    parts = np.concatenate([od.push(long_imgs[:70], az), od.push(long_imgs[70:], az)])
    od.close()
    assert parts.tobytes() == res.tobytes()


def test_gates(small):
    imgs, az, alone = small
    want = np.array([alone[(i, i - 1)] for i in range(1, 6)])
    ratio, theta = np.sort(want["peak_ratio"]), np.sort(np.abs(want["theta"]))
    assert ratio[2] < ratio[3] and theta[2] < theta[3]
    max_ratio, max_rot = 0.5 * (ratio[2] + ratio[3]), 0.5 * (theta[2] + theta[3])
    over_ratio, over_rot = want["peak_ratio"] > max_ratio, np.abs(want["theta"]) > max_rot
    assert over_ratio.sum() == 2 and over_rot.sum() == 2
    od = _small_odometry()
    plain = od.push(imgs, az)
    for fields, status in ((dict(max_peak_ratio=max_ratio), 18 * over_ratio), (dict(max_rotation=max_rot), 17 * over_rot),
                           (dict(max_peak_ratio=max_ratio, max_rotation=max_rot), (16 | over_rot | 2 * over_ratio) * (over_rot | over_ratio)),
                           (dict(min_peak=2.0), np.full(5, 18))):   # (no peak reaches 2: every pair fails that gate)
        od.reset()
        od.set_phasecorr(dict(SMALL, **fields))
        got = od.push(imgs, az)
        assert got["status"].tolist() == [3] + np.asarray(status).astype(int).tolist(), (fields, got["status"])
        for f in ("x", "y", "yaw", "iterations", "rot_inliers", "trans_inliers", "n_keypoints", "n_matches"):
            assert got[f].tobytes() == plain[f].tobytes(), (fields, f)
    od.close()


def _dim(imgs, i, z_min=60):
    """scan i with its power samples scaled so that their maximum lies below z_min: the extractor finds nothing in it"""
    out = imgs.copy()
    power = out[i, :, OFF:].astype(np.float64)
    out[i, :, OFF:] = np.floor(power * ((z_min - 1) / power.max())).astype(np.uint8)
    assert out[i, :, OFF:].max() < z_min and out[i, :, OFF:].max() > 0
    return out


def _fallback_case(rows, cols, imgs, az, poses, pc_fields, **kw):
    """-> (plain, with fallback) on `imgs` with scan 3 dimmed; asserts that exactly pairs 3 and 4 are replaced, by the stand-alone results"""
    from navtech_radar_slam_amd import odometry
    dim = _dim(imgs, 3)
    od = odometry.Odometry(rows, cols, keypoints="kstrongest", **kw)
    plain = od.push(dim, az)
    failed = (plain["status"] != 0) & ~((kw.get("estimator") == "cfear") & (plain["status"] == 8))
    assert failed.tolist() == [True, False, False, True, True, False], plain["status"]   # (record 0: the first scan, status 3)
    assert plain["n_keypoints"][3] == 0
    od.reset()
    od.set_phasecorr(dict(pc_fields, mode=1))
    got = od.push(dim, az)
    want = _standalone(rows, cols, dim, [(3, 2), (4, 3)], od, **pc_fields)
    od.close()
    assert not want["status"].any()
    for i in (0, 1, 2, 5):
        assert got[i].tobytes() == plain[i].tobytes(), (i, got[i], plain[i])
    _check_records(got[3:5], want, first=0)
    assert np.all(got["iterations"][3:5] < 0) and not got["status"][3:5].any()
    assert np.array_equal(got["n_matches"], plain["n_matches"]) and np.array_equal(got["n_keypoints"], plain["n_keypoints"])
    for i in (3, 4):
        truth = synth.relative_pose(poses[i - 1], poses[i])
        print(f"{kw.get('estimator', 'orora')} pair {i} replaced: error {np.hypot(got['x'][i] - truth[0], got['y'][i] - truth[1]):.3f} m "
              f"{abs(got['yaw'][i] - truth[2]):.4f} rad, peak {want['peak'][i - 3]:.3f} ratio {want['peak_ratio'][i - 3]:.3f}")
    return plain, got


@pytest.fixture(scope="module")
def drive():
    return synth.polar_sequence(3, 6)


def test_fallback_replaces_failed_pairs_and_nothing_else(drive):
    from navtech_radar_slam_amd import odometry
    imgs, az, poses, _ = drive
    plain, _ = _fallback_case(400, 3360, imgs, az, poses, {})
    assert plain["status"].tolist() == [3, 0, 0, 1, 1, 0]
    # no pair fails on the undimmed sequence: fallback on gives the bytes of fallback off
    od = odometry.Odometry(400, 3360, keypoints="kstrongest")
    off = od.push(imgs, az)
    assert off["status"].tolist() == [3, 0, 0, 0, 0, 0]
    od.reset()
    od.set_phasecorr(dict(mode=1))
    on = od.push(imgs, az)
    od.reset()
    od.set_phasecorr(off=True)
    again = od.push(imgs, az)
    od.close()
    assert on.tobytes() == off.tobytes() == again.tobytes()


def test_fallback_beside_ransac(drive):
    imgs, az, poses, _ = drive
    _fallback_case(400, 3360, imgs, az, poses, {}, estimator="ransac")


def test_fallback_beside_cfear(small):
    from navtech_radar_slam_amd import kstrongest
    imgs, az, _ = small
    poses = synth.polar_sequence(3, 6, rows=64, cols=512, n_buildings=120, n_poles=200, world_radius=40.0)[2]
    _fallback_case(64, 512, imgs, az, poses, SMALL, estimator="cfear", kstrongest=kstrongest.params(k=K, min_separation=0))


def test_switching_rules(small):
    from navtech_radar_slam_amd import _rsx, odometry
    imgs, az, _ = small
    od = odometry.Odometry(64, 512, keypoints="kstrongest")
    fresh = od.push(imgs[:3], az)
    with pytest.raises(_rsx.RsxError, match="holds a scan"):
        od.set_phasecorr(SMALL)
    od.reset()
    od.set_compensation("both")
    for mode in (0, 1):
        with pytest.raises(_rsx.RsxError, match="compensation"):
            od.set_phasecorr(dict(SMALL, mode=mode))
    od.set_compensation(None)
    with pytest.raises(_rsx.RsxError, match="rsx_odometry_set_phasecorr"):
        _rsx.check(_rsx.lib().rsx_odometry_set_estimator(od._h, _rsx.ESTIMATOR_PHASECORR, None))
    for bad in (dict(n=100), dict(n=64, resolution=0.0), dict(n=256, resolution=0.9), dict(SMALL, max_peak_ratio=-1.0), dict(SMALL, mode=2)):
        with pytest.raises(_rsx.RsxError) as e:   # a bad N, a bad resolution, a disc of 128 x 0.9 m in 511 bins of 0.0595 m, a bad gate, a bad mode
            od.set_phasecorr(bad)
        assert e.value.status == -1
    od.set_cfear()
    od.set_cfear_tracking()
    for mode in (0, 1):
        with pytest.raises(_rsx.RsxError, match="tracker"):
            od.set_phasecorr(dict(SMALL, mode=mode))
    od.set_cfear_tracking(off=True)
    od.set_phasecorr(dict(SMALL, mode=1))   # the fallback beside CFEAR pairs
    with pytest.raises(_rsx.RsxError, match="fallback"):
        od.set_cfear_tracking()
    od.set_cfear(off=True)                  # ORORA, the fallback still beside it
    with pytest.raises(_rsx.RsxError, match="phase correlation"):
        od.set_compensation("motion")
    od.set_phasecorr(SMALL)                 # ESTIMATE in place of the fallback
    with pytest.raises(_rsx.RsxError, match="phase correlation"):
        od.set_compensation("motion")
    with pytest.raises(_rsx.RsxError, match="CFEAR"):
        od.set_cfear_tracking()
    got = od.push(imgs[:2], az)
    assert got["iterations"][1] < 0 and got["n_keypoints"][1] == fresh["n_keypoints"][1]
    with pytest.raises(_rsx.RsxError, match="holds a scan"):
        od.set_phasecorr(off=True)
    od.reset()
    od.set_phasecorr(off=True)              # NULL: the state before == a fresh default handle
    assert od.push(imgs[:3], az).tobytes() == fresh.tobytes()
    od.reset()
    od.set_phasecorr(SMALL)
    od.set_estimator("ransac")              # leaves ESTIMATE as it leaves any other estimator
    ransac = od.push(imgs[:3], az)
    od.close()
    ref = odometry.Odometry(64, 512, keypoints="kstrongest", estimator="ransac")
    assert ransac.tobytes() == ref.push(imgs[:3], az).tobytes() and np.all(ransac["iterations"][1:] >= 0)
    ref.close()


def test_host_entry_on_png_files(tmp_path):
    """host/odometry --estimator phasecorr on PNG files prints the composition of the library's records"""
    from PIL import Image
    from navtech_radar_slam_amd import odometry
    from oracle import odometry_chain
    imgs, az, _, stamps = synth.polar_sequence(11, 4)
    d = tmp_path / "seq" / "polar_oxford_form"
    d.mkdir(parents=True)
    for img, st in zip(imgs, stamps):
        Image.fromarray(img, mode="L").save(str(d / f"{int(st)}.png"))
    exe = [os.path.join(HOST, "odometry"), f"seq_dir:={tmp_path / 'seq'}", "do_slam:=true"]
    r = subprocess.run(exe + ["--estimator", "phasecorr", "--pc-n", "64", "--pc-resolution", "2.0", "--window", "3"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [line.split() for line in r.stdout.strip().splitlines()]
    got = np.array([[float(v) for v in x[1:]] for x in rows])
    assert got.shape == (4, 5) and np.array_equal(np.array([int(x[0]) for x in rows], dtype=np.int64), stamps)
    od = odometry.Odometry(400, 3360, estimator="phasecorr", phasecorr=dict(n=64, resolution=2.0))
    res = od.push(imgs, az)
    od.close()
    assert np.all(res["iterations"][1:] < 0)
    pose, lib_pose = np.zeros(3), [np.zeros(3)]
    for i in range(1, 4):
        if res["status"][i] == 0:
            pose = odometry_chain.compose(pose, (res["x"][i], res["y"][i], res["yaw"][i]))
        lib_pose.append(pose.copy())
    assert np.allclose(got[:, 0:3], np.stack(lib_pose), atol=2e-6), np.abs(got[:, 0:3] - np.stack(lib_pose)).max()
    assert np.array_equal(got[:, 3], res["n_keypoints"]) and not got[:, 4].any()
    bad = subprocess.run(exe + ["--estimator", "phasecorr", "--compensate", "both"], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0
