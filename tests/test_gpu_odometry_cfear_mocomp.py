"""The file-based odometry path with CFEAR's keyframe tracker and its motion compensation (rsx_odometry_set_cfear_tracking with
compensate = 1: surface points with times from the extractor's azimuth rows, every scan registered twice) against the chain
kstrongest_np -> cfear_mocomp_np.surface_points_timed -> cfear_mocomp_np.track on the 8-scan small sequence (64 rows x 512 columns).

Status, iterations and correspondences equal the chain's, the relative motions agree within 1e-4 (the project's pose tolerance); no
scan is left out: the chain's smallest decision margin is asserted to be at least 1e-9.  Pushed whole or in calls of 1, 3 and 8 scans the
BYTES are equal; with compensation off the results are those of the tracker without it.
PARITY UNPINNED w.r.t. CFEAR's own code, which is not in the reference checkout."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cfear_mocomp_cases as mcases  # noqa: E402
import cfear_track_cases as cases  # noqa: E402
import cfear_track_np as ct  # noqa: E402

pytestmark = pytest.mark.gpu
K = 12


def _odometry(**kw):
    from navtech_radar_slam_amd import kstrongest, odometry
    return odometry.Odometry(mcases.SMALL_ROWS, mcases.SMALL_COLS, keypoints="kstrongest", kstrongest=kstrongest.params(k=K, min_separation=0),
                             estimator="cfear", **kw)


def _pose(r):
    return (r["x"], r["y"], r["yaw"])


def _pushes(od, imgs, az, size):
    return np.concatenate([od.push(imgs[a:a + size], az[a:a + size] if np.ndim(az) == 2 else az) for a in range(0, len(imgs), size)])


def test_compensated_odometry_equals_the_chain_however_it_is_cut():
    from navtech_radar_slam_amd import cfear
    _, imgs, az = mcases.small_keypoints()
    want = mcases.small_track()
    assert min(w["margin"] for w in want) >= 1e-9  # none is left out
    od = _odometry(cfear_track=cfear.track_params(**cases.SMALL_TRACK), cfear_compensate=True)
    whole, xy = od.push(imgs, az, want_xy=True)
    print("compensated small sequence:", whole["status"].tolist(), whole["n_matches"].tolist(), whole["iterations"].tolist())
    assert whole["status"][0] == 3
    assert whole["status"][1:].tolist() == [w["reg"]["status"] for w in want[1:]]
    assert whole["n_matches"][1:].tolist() == [w["reg"]["correspondences"] for w in want[1:]]
    assert whole["iterations"][1:].tolist() == [w["reg"]["iterations"] for w in want[1:]]
    for i in range(1, 8):
        rel = ct.between(_pose(want[i - 1]), _pose(want[i]))
        assert max(abs(whole[f][i] - v) for f, v in zip(("x", "y", "yaw"), rel)) < 1e-4, (i, whole[i], rel)
    for size in (1, 3, 8):
        od.reset()
        assert _pushes(od, imgs, az, size).tobytes() == whole.tobytes(), size
    # compensation is at work, and off it gives the tracker's results of today; the published cloud is the same either way
    plain = _odometry(cfear_track=cfear.track_params(**cases.SMALL_TRACK))
    off, xy_off = plain.push(imgs, az, want_xy=True)
    assert off.tobytes() != whole.tobytes() and len(xy) == len(xy_off) and all(np.array_equal(a, b) for a, b in zip(xy, xy_off))
    same = _odometry(cfear_track=cfear.track_params(compensate=0, **cases.SMALL_TRACK), cfear_compensate=False)
    assert same.push(imgs, az).tobytes() == off.tobytes()
    track = cases.small_track()
    assert off["n_matches"][1:].tolist() == [w["reg"]["correspondences"] for w in track[1:]]
    assert off["iterations"][1:].tolist() == [w["reg"]["iterations"] for w in track[1:]]


def test_switching_rules():
    from navtech_radar_slam_amd import _rsx, cfear, kstrongest, odometry
    with pytest.raises(ValueError, match="cfear"):
        odometry.Odometry(mcases.SMALL_ROWS, mcases.SMALL_COLS, cfear_compensate=True)
    od = _odometry(cfear_compensate=True)  # (it implies the tracker, at its defaults)
    with pytest.raises(_rsx.RsxError, match="no matches to compensate"):
        od.set_compensation("motion")
    with pytest.raises(_rsx.RsxError, match="compensate"):
        od.set_cfear_tracking(cfear.track_params(compensate=2))
    od.set_cfear_tracking(off=True)
    _, imgs, az = mcases.small_keypoints()
    pairs = od.push(imgs[:3], az[:3] if np.ndim(az) == 2 else az)
    want = _odometry().push(imgs[:3], az[:3] if np.ndim(az) == 2 else az)
    assert pairs.tobytes() == want.tobytes()  # back to consecutive pairs: nothing of the compensation stays
