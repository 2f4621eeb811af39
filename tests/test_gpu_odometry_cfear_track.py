"""The file-based odometry path with CFEAR's keyframe tracker (rsx_odometry_set_cfear_tracking: every scan registered jointly
against the last keyframes from a constant-velocity prediction) on a MOVING sensor with known poses: the windowed pipeline against
the CPU chain tests/kstrongest_np.py -> tests/cfear_np.py -> tests/cfear_track_np.py, against the true poses, and through the C++
entry host/odometry --estimator cfear --cfear-keyframes 3.

Six scans of synth.polar_sequence(11, 6).  Measured with the CPU chain (tests/test_cfear_track_restatement.py): keyframes at scans
0, 2, 4; 518 / 499 / 994 / 920 / 1422 correspondences, every status 0, smallest decision margin 8.6e-9; per pair the bounds are those
test_gpu_odometry.py holds cen2019 to (0.25 m / 1e-2 rad).  A scan whose restatement margin is below 1e-9 would be left out of the
pose comparison; none is (asserted).
PARITY UNPINNED w.r.t. CFEAR's own code, which is not in the reference checkout."""
import os
import subprocess
import sys

import numpy as np
import pytest

from navtech_radar_slam_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cfear_track_cases as cases  # noqa: E402
import cfear_track_np as ct  # noqa: E402

pytestmark = pytest.mark.gpu
HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "navtech-radar-slam_amd", "host")
N_SCANS = 6
K = 12


def _odometry(rows=400, cols=3360, **kw):
    from navtech_radar_slam_amd import kstrongest, odometry
    kw.setdefault("cfear_track", True)
    return odometry.Odometry(rows, cols, keypoints="kstrongest", kstrongest=kstrongest.params(k=K, min_separation=0), estimator="cfear", **kw)


def _pose(r):
    return (r["x"], r["y"], r["yaw"])


def test_windowed_pipeline_equals_chain_and_truth():
    imgs, az, poses, _ = cases.drive_images(N_SCANS)
    track = cases.drive_track()
    assert min(w["margin"] for w in track) >= 1e-9  # none is left out
    res = _odometry().push(imgs, az)
    assert res["status"][0] == 3 and res["n_matches"][0] == 0 and np.all(res["n_keypoints"] == 4800)
    worst_t = worst_y = worst_d = 0.0
    for i in range(1, N_SCANS):
        w = track[i]["reg"]
        assert res["n_matches"][i] == res["rot_inliers"][i] == res["trans_inliers"][i] == w["correspondences"], (i, res[i], w)
        assert res["iterations"][i] == w["iterations"] and res["status"][i] == w["status"] == 0, (i, res[i], w)
        rel = ct.between(_pose(track[i - 1]), _pose(track[i]))
        d = max(abs(res[f][i] - v) for f, v in zip(("x", "y", "yaw"), rel))
        worst_d = max(worst_d, d)
        assert d < 1e-4, (i, res[i], rel)
        truth = synth.relative_pose(poses[i - 1], poses[i])
        et, ey = float(np.hypot(res["x"][i] - truth[0], res["y"][i] - truth[1])), abs(float(res["yaw"][i] - truth[2]))
        assert et < 0.25 and ey < 1e-2, (i, et, ey)
        worst_t, worst_y = max(worst_t, et), max(worst_y, ey)
    print(f"cfear tracking odometry: |GPU - chain| {worst_d:.2e}, worst pair {worst_t:.3f} m {worst_y:.2e} rad")
    # the joint registration is at work: scan 5 was registered against three keyframes
    assert res["n_matches"][5] == 1422


def test_cutting_the_sequence_into_calls_changes_nothing():
    from navtech_radar_slam_amd import cfear
    imgs, az, _, _ = synth.polar_sequence(3, 8, rows=64, cols=512, n_buildings=120, n_poles=200, world_radius=40.0)
    od = _odometry(64, 512, cfear_track=cfear.track_params(**cases.SMALL_TRACK))
    whole = od.push(imgs, az)
    want = cases.small_track()
    print("small sequence:", whole["status"].tolist(), whole["n_matches"].tolist(), whole["iterations"].tolist())
    assert whole["status"][0] == 3 and whole["n_matches"][1:].tolist() == [w["reg"]["correspondences"] for w in want[1:]]
    assert whole["iterations"][1:].tolist() == [w["reg"]["iterations"] for w in want[1:]]
    for i in range(1, 8):
        rel = ct.between(_pose(want[i - 1]), _pose(want[i]))
        assert max(abs(whole[f][i] - v) for f, v in zip(("x", "y", "yaw"), rel)) < 1e-4, i
    for cuts in (((0, 1), (1, 3), (3, 8)), ((0, 4), (4, 5), (5, 8))):
        od.reset()
        parts = np.concatenate([od.push(imgs[a:b], az[a:b] if np.ndim(az) == 2 else az) for a, b in cuts])
        assert parts.tobytes() == whole.tobytes(), cuts
    od.reset()  # a new sequence: the tracker starts again
    assert od.push(imgs, az).tobytes() == whole.tobytes()


def test_switching_rules():
    from navtech_radar_slam_amd import _rsx, cfear, kstrongest, odometry
    imgs, az, _, _ = synth.polar_sequence(11, 4)
    od = odometry.Odometry(400, 3360, keypoints="kstrongest", kstrongest=kstrongest.params(k=K, min_separation=0))
    with pytest.raises(_rsx.RsxError, match="rsx_odometry_set_cfear first"):
        od.set_cfear_tracking()  # refused before set_cfear
    od.set_cfear_tracking(off=True)  # (NULL is always "pairs")
    od.set_cfear()
    pairs = od.push(imgs, az)  # today's bytes
    with pytest.raises(_rsx.RsxError, match="holds a scan"):
        od.set_cfear_tracking()
    with pytest.raises(_rsx.RsxError, match="holds a scan"):
        od.set_cfear_tracking(off=True)
    od.reset()
    for bad, word in ((dict(n_keyframes=0), "n_keyframes"), (dict(n_keyframes=5), "n_keyframes"), (dict(keyframe_distance=-1.0), "keyframe_distance"),
                      (dict(search=2), "search")):
        with pytest.raises(_rsx.RsxError, match=word):
            od.set_cfear_tracking(cfear.track_params(**bad))
    od.set_cfear_tracking()
    tracked = od.push(imgs, az)
    assert tracked["status"].tolist() == [3, 0, 0, 0] and tracked.tobytes() != pairs.tobytes()
    assert tracked["n_matches"][3] > pairs["n_matches"][3]  # two keyframes at scan 3
    od.reset()
    od.set_cfear_tracking(off=True)  # NULL: back to pairs
    assert od.push(imgs, az).tobytes() == pairs.tobytes()
    od.reset()
    od.set_cfear_tracking(cfear.track_params(search=1))  # brute force: the same bytes
    assert od.push(imgs, az).tobytes() == tracked.tobytes()
    od.reset()
    od.set_cfear(off=True)  # leaving CFEAR leaves tracking
    od.set_cfear()
    assert od.push(imgs, az).tobytes() == pairs.tobytes()


def test_host_entry_on_png_files(tmp_path):
    """host/odometry --estimator cfear --cfear-keyframes 3 --window 3 on PNG files prints the poses the library gives"""
    from PIL import Image
    from oracle import odometry_chain
    imgs, az, poses, stamps = cases.drive_images(N_SCANS)
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

    got, got_stamps = run("--estimator", "cfear", "--cfear-keyframes", "3", "--window", "3")
    assert got.shape == (N_SCANS, 5) and np.array_equal(got_stamps, stamps)
    res = _odometry().push(imgs, az)
    pose, lib_pose = np.zeros(3), [np.zeros(3)]
    for i in range(1, N_SCANS):
        pose = odometry_chain.compose(pose, (res["x"][i], res["y"][i], res["yaw"][i]))
        lib_pose.append(pose.copy())
    assert np.allclose(got[:, 0:3], np.stack(lib_pose), atol=2e-6), np.abs(got[:, 0:3] - np.stack(lib_pose)).max()
    assert np.allclose(got[:, 0:3], np.array([_pose(w) for w in cases.drive_track()]), atol=2e-4)
    assert np.array_equal(got[:, 3], res["n_keypoints"]) and np.array_equal(got[:, 4], res["n_matches"])
    from navtech_radar_slam_amd import cfear
    import math
    other, _ = run("--estimator", "cfear", "--cfear-keyframes", "2", "--cfear-keyframe-distance", "0.5", "--cfear-keyframe-rotation", "2",
                   "--cfear-no-prediction", "--max_frames", "4")
    want = _odometry(cfear_track=cfear.track_params(n_keyframes=2, keyframe_distance=0.5, keyframe_rotation=2.0 * 3.14159265358979323846 / 180.0,
                                                    predict=0)).push(imgs[:4], az)
    assert math.isclose(other[3, 4], want["n_matches"][3]) and want["n_matches"][3] != res["n_matches"][3]
    bad = subprocess.run([os.path.join(HOST, "odometry"), f"seq_dir:={tmp_path / 'seq'}", "--cfear-keyframes", "3"], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "--estimator cfear" in bad.stdout + bad.stderr
