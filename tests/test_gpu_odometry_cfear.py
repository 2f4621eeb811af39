"""The file-based odometry path with CFEAR's own pipeline (rsx_odometry_set_cfear: k-strongest keypoints with min_separation = 0,
oriented surface points, point-to-line registration; no Cartesian image, descriptors or matcher) on a MOVING sensor with known
poses: the windowed pipeline against the CPU chain tests/kstrongest_np.py -> tests/cfear_np.py, against the true poses, and
through the C++ entry host/odometry --estimator cfear.

Four scans of synth.polar_sequence(11, 4).  Measured with the CPU chain (tests/test_cfear_restatement.py): 4800 keypoints per
scan, 505 / 496 / 522 correspondences, 18 / 15 / 17 iterations, every pair status 0, worst pair 0.032 m / 4.8e-4 rad; per pair the
bounds are those test_gpu_odometry.py holds cen2019 to (0.25 m / 1e-2 rad).  A pair whose restatement margin is below 1e-9 would
be left out of the pose comparison; none is (asserted in the `chain` fixture).
PARITY UNPINNED w.r.t. CFEAR's own code, which is not in the reference checkout."""
import os
import subprocess
import sys

import numpy as np
import pytest

from navtech_radar_slam_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cfear_np as cf  # noqa: E402
import kstrongest_np as ksn  # noqa: E402

pytestmark = pytest.mark.gpu
HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "navtech-radar-slam_amd", "host")
N_SCANS = 4
K = 12


@pytest.fixture(scope="module")
def sequence():
    return synth.polar_sequence(11, N_SCANS)


@pytest.fixture(scope="module")
def chain(sequence, oracle):
    from oracle import odometry_chain
    imgs, az, poses, _ = sequence
    out, prev, pose = [], None, np.zeros(3)
    for i in range(N_SCANS):
        tg = ksn.extract(imgs[i], k=K, z_min=60, min_separation=0)
        xy = ksn.to_cartesian(tg, az[i] if np.ndim(az) == 2 else az, synth.RADAR_RESOLUTION)
        sp, status = cf.surface_points(xy)
        assert status == 0
        rec = {"n_keypoints": len(tg), "result": None, "xy": xy}
        if prev is not None:
            r = cf.register(sp, prev)
            assert r["status"] == 0 and r["margin"] >= 1e-9, r
            rec["result"] = r
            pose = odometry_chain.compose(pose, (r["x"], r["y"], r["yaw"]))
        rec["pose"] = pose.copy()
        out.append(rec)
        prev = sp
    return out


def _odometry(**kw):
    from navtech_radar_slam_amd import kstrongest, odometry
    return odometry.Odometry(400, 3360, keypoints="kstrongest", kstrongest=kstrongest.params(k=K, min_separation=0), estimator="cfear", **kw)


def test_windowed_pipeline_equals_chain_and_truth(sequence, chain):
    imgs, az, poses, _ = sequence
    res, xy = _odometry().push(imgs, az, want_xy=True)
    assert res["status"][0] == 3 and np.all(res["status"][1:] == 0)
    worst_t = worst_y = worst_d = 0.0
    for i in range(N_SCANS):
        want = chain[i]
        assert res["n_keypoints"][i] == want["n_keypoints"]
        assert np.allclose(xy[i], want["xy"], rtol=1e-5, atol=1e-4)
        if i == 0:
            assert res["n_matches"][0] == 0
            continue
        w = want["result"]
        assert res["n_matches"][i] == res["rot_inliers"][i] == res["trans_inliers"][i] == w["correspondences"], (i, res[i], w)
        assert res["iterations"][i] == w["iterations"] and res["status"][i] == w["status"], (i, res[i], w)
        d = max(abs(res[f][i] - w[f]) for f in ("x", "y", "yaw"))
        worst_d = max(worst_d, d)
        assert d < 1e-4, (i, res[i], w)
        truth = synth.relative_pose(poses[i - 1], poses[i])
        et, ey = float(np.hypot(res["x"][i] - truth[0], res["y"][i] - truth[1])), abs(float(res["yaw"][i] - truth[2]))
        assert et < 0.25 and ey < 1e-2, (i, et, ey)
        worst_t, worst_y = max(worst_t, et), max(worst_y, ey)
    print(f"cfear odometry: |GPU - chain| {worst_d:.2e}, worst pair {worst_t:.3f} m {worst_y:.2e} rad")


def test_cutting_the_sequence_into_calls_changes_nothing():
    imgs, az, _, _ = synth.polar_sequence(3, 6, rows=64, cols=512, n_buildings=120, n_poles=200, world_radius=40.0)
    from navtech_radar_slam_amd import kstrongest, odometry
    od = odometry.Odometry(64, 512, keypoints="kstrongest", kstrongest=kstrongest.params(k=K, min_separation=0), estimator="cfear")
    whole = od.push(imgs, az)
    assert whole["status"][0] == 3 and np.all(whole["n_keypoints"] == 768)
    print("small sequence:", whole["status"].tolist(), whole["n_matches"].tolist(), whole["iterations"].tolist())
    assert np.any(whole["n_matches"][1:] > 0)
    od.reset()
    parts = np.concatenate([od.push(imgs[a:b], az[a:b] if np.ndim(az) == 2 else az) for a, b in ((0, 1), (1, 3), (3, 6))])
    assert parts.tobytes() == whole.tobytes()


def test_switching_rules(sequence):
    from navtech_radar_slam_amd import _rsx, cfear, kstrongest, odometry
    imgs, az, _, _ = sequence
    od = odometry.Odometry(400, 3360)
    fresh = od.push(imgs[:3], az)
    with pytest.raises(_rsx.RsxError, match="holds a scan"):
        od.set_cfear()
    od.reset()
    od.set_compensation("both")
    with pytest.raises(_rsx.RsxError, match="compensation"):
        od.set_cfear()
    od.set_compensation(None)
    with pytest.raises(_rsx.RsxError, match="rsx_odometry_set_cfear"):
        _rsx.check(_rsx.lib().rsx_odometry_set_estimator(od._h, _rsx.ESTIMATOR_CFEAR, None))
    for bad in (dict(radius=0.0), dict(cos_max_normal_angle=2.0), dict(max_iterations=0)):
        with pytest.raises(_rsx.RsxError):
            od.set_cfear(cfear.params(**bad))
    od.set_cfear()
    with pytest.raises(_rsx.RsxError, match="CFEAR"):
        od.set_compensation("motion")
    got = od.push(imgs[:2], az)  # cen2019 keypoints + CFEAR: the setter is independent of the extractor
    assert got["n_keypoints"][1] == fresh["n_keypoints"][1] and got["status"][0] == 3
    with pytest.raises(_rsx.RsxError, match="holds a scan"):
        od.set_cfear(off=True)
    od.reset()
    od.set_cfear(off=True)  # NULL: back to ORORA == a fresh default handle
    assert od.push(imgs[:3], az).tobytes() == fresh.tobytes()
    od.reset()
    od.set_kstrongest(kstrongest.params(k=K, min_separation=0))
    od.set_cfear(cfear.params(max_iterations=2))
    two = od.push(imgs[:2], az)
    assert two["status"][1] == 8 and two["iterations"][1] == 2


def test_host_entry_on_png_files(sequence, chain, tmp_path):
    """host/odometry --keypoints kstrongest --min-separation 0 --estimator cfear on PNG files prints the poses the library gives"""
    from PIL import Image
    from oracle import odometry_chain
    imgs, az, poses, stamps = sequence
    d = tmp_path / "seq" / "polar_oxford_form"
    d.mkdir(parents=True)
    for img, st in zip(imgs, stamps):
        Image.fromarray(img, mode="L").save(str(d / f"{int(st)}.png"))

    def run(*flags):
        r = subprocess.run([os.path.join(HOST, "odometry"), f"seq_dir:={tmp_path / 'seq'}", "do_slam:=true", "--keypoints", "kstrongest", "--k", str(K),
                            "--min-separation", "0", *flags], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        rows = [line.split() for line in r.stdout.strip().splitlines()]
        return np.array([[float(v) for v in x[1:]] for x in rows]), np.array([int(x[0]) for x in rows], dtype=np.int64)

    got, got_stamps = run("--estimator", "cfear", "--window", "3")
    assert got.shape == (N_SCANS, 5) and np.array_equal(got_stamps, stamps)
    res = _odometry().push(imgs, az)
    pose, lib_pose = np.zeros(3), [np.zeros(3)]
    for i in range(1, N_SCANS):
        pose = odometry_chain.compose(pose, (res["x"][i], res["y"][i], res["yaw"][i]))
        lib_pose.append(pose.copy())
    assert np.allclose(got[:, 0:3], np.stack(lib_pose), atol=2e-6), np.abs(got[:, 0:3] - np.stack(lib_pose)).max()
    assert np.allclose(got[:, 0:3], np.stack([c["pose"] for c in chain]), atol=2e-4)
    assert np.array_equal(got[:, 3], res["n_keypoints"]) and np.array_equal(got[:, 4], res["n_matches"])
    other, _ = run("--estimator", "cfear", "--cfear-max-iterations", "2", "--cfear-radius", "3.0", "--cfear-normal-angle", "20", "--cfear-huber", "0.2",
                   "--max_frames", "2")
    from navtech_radar_slam_amd import cfear
    import math
    want = _odometry(cfear=cfear.params(max_iterations=2, radius=3.0, cos_max_normal_angle=math.cos(20.0 * 3.14159265358979323846 / 180.0),
                                        huber_delta=0.2)).push(imgs[:2], az)
    assert np.allclose(other[1, 0:3], [want["x"][1], want["y"][1], want["yaw"][1]], atol=2e-6) and other[1, 4] == want["n_matches"][1]
    bad = subprocess.run([os.path.join(HOST, "odometry"), f"seq_dir:={tmp_path / 'seq'}", "--estimator", "cfear", "--compensate", "both"],
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0
