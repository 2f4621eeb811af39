"""The file-based odometry path with the RANSAC estimators (rsx_odometry_set_estimator) on a moving sensor: the windowed
pipeline against the CPU chain -- oracle/odometry_chain.run's steps up to the cross-checked matches, then the numpy
restatement tests/ransac_np.py in place of the max-clique selection and ORORA (written out below) -- for every cut of the
sequence into calls, and the switching rules.  MC time model (include/rsx.h): dt = (float)(dt_scan (1 + (a_cur - a_prev) /
rows)) from the azimuth rows of a match's two keypoints.  PARITY UNPINNED w.r.t. upstream (its sources are absent)."""
import os
import sys

import numpy as np
import pytest

from navtech_radar_slam_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ransac_np as rn  # noqa: E402

pytestmark = pytest.mark.gpu
N_SCANS, ROWS, DT_SCAN = 7, 400, 0.25


def chain_ransac(images, azimuths, mc, resolution=synth.RADAR_RESOLUTION, col_offset=11, ratio=0.8, W=964, cart_res=0.2592):
    from oracle import pyoracle as po
    n, rows, stride = images.shape
    fe = po.FrontendRef(rows=rows, cols=stride - col_offset, W=W, cart_res=cart_res)
    out, prev = [], None
    for i in range(n):
        tg = po.cen2019_extract(images[i], col_offset=col_offset, max_points=10000, min_range=58)[:16384]
        xy = po.cen2019_to_cartesian(tg, azimuths, resolution)
        fe.cartesian(images[i], azimuths, resolution, col_offset=col_offset)
        desc, valid = fe.describe(xy)
        rec = {"n_keypoints": len(tg), "n_matches": 0, "result": None}
        if prev is not None:
            fwd, _, _ = fe.match(prev[1], prev[2], desc, valid, ratio=ratio)
            bwd, _, _ = fe.match(desc, valid, prev[1], prev[2], ratio=ratio)
            ii = np.nonzero(fwd >= 0)[0]
            ii = ii[bwd[fwd[ii]] == ii]
            src, dst = xy[fwd[ii]], prev[0][ii]
            a_cur, a_prev = np.asarray(tg)[fwd[ii], 0].astype(np.int64), np.asarray(prev[3])[ii, 0].astype(np.int64)
            dt = (DT_SCAN * (1.0 + (a_cur - a_prev) / float(rows))).astype(np.float32)
            rec["n_matches"] = len(ii)
            rec["result"] = rn.estimate(src, dst, dt if mc else None, mc=mc, debug=True)
        out.append(rec)
        prev = (xy, desc, valid, tg)
    return out


@pytest.fixture(scope="module")
def sequence():
    return synth.polar_sequence(11, N_SCANS)


@pytest.mark.parametrize("estimator", ["ransac", "mcransac"])
def test_pipeline_equals_chain_for_every_window_cut(sequence, oracle, estimator):
    from navtech_radar_slam_amd import odometry
    imgs, az, poses, _ = sequence
    chain = chain_ransac(imgs, az, estimator == "mcransac")
    od = odometry.Odometry(ROWS, 3360, estimator=estimator)
    whole = od.push(imgs, az)
    assert whole["status"][0] == 3
    worst = 0.0
    for i in range(N_SCANS):
        want = chain[i]
        assert whole["n_keypoints"][i] == want["n_keypoints"] and whole["n_matches"][i] == want["n_matches"], (i, whole[i])
        if i == 0:
            continue
        w = want["result"]
        assert w["margin"] > 1e-9, (i, w["margin"])   # no match on the threshold: the counts below are exact
        assert (whole["status"][i], whole["iterations"][i], whole["rot_inliers"][i], whole["trans_inliers"][i]) == (w["status"], w["hypotheses"], w["inliers"], w["inliers"]), (i, whole[i], w)
        worst = max(worst, max(abs(whole[f][i] - w[f]) for f in ("x", "y", "yaw")))
        truth = synth.relative_pose(poses[i - 1], poses[i])
        assert w["status"] == 0 and np.hypot(whole["x"][i] - truth[0], whole["y"][i] - truth[1]) < 0.25 and abs(whole["yaw"][i] - truth[2]) < 1e-2
    print(f"{estimator}: max |pose - chain| {worst:.3e}")
    assert worst < 1e-4
    # the same scans as two calls and scan by scan
    od.reset()
    two = np.concatenate([od.push(imgs[:3], az), od.push(imgs[3:], az)])
    assert np.array_equal(two, whole)
    od.reset()
    single = np.concatenate([od.push(imgs[i:i + 1], az) for i in range(N_SCANS)])
    assert np.array_equal(single, whole)


def test_switching_rules_and_the_default_path(sequence):
    from navtech_radar_slam_amd import _rsx, odometry, ransac
    imgs, az, _, _ = sequence
    fresh = odometry.Odometry(ROWS, 3360).push(imgs[:5], az)
    od = odometry.Odometry(ROWS, 3360)
    od.push(imgs[:2], az)
    for name in ("ransac", "mcransac", "orora"):
        with pytest.raises(_rsx.RsxError):
            od.set_estimator(name)   # holds a scan
    od.reset()
    with pytest.raises(_rsx.RsxError):
        od.set_estimator("ransac", ransac.default_params(tolerance=-1.0))
    assert _rsx.lib().rsx_odometry_set_estimator(od._h, 3, None) == -1
    od.set_estimator("ransac", ransac.default_params(seed=3))
    r3 = od.push(imgs[:5], az)
    od.reset()
    od.set_estimator("mcransac")
    mc = od.push(imgs[:5], az)
    assert np.all(mc["status"][1:] == 0) and np.all(r3["status"][1:] == 0)
    assert not np.array_equal(r3[["x", "y", "yaw"]], fresh[["x", "y", "yaw"]])
    od.reset()
    od.set_estimator("orora")
    back = od.push(imgs[:5], az)
    assert back.tobytes() == fresh.tobytes()   # the default path after a round trip through both RANSAC estimators
    # independent of the extractor choice
    od = odometry.Odometry(ROWS, 3360, keypoints="cen2018", estimator="mcransac")
    got = od.push(imgs[:3], az)
    assert np.all(got["status"][1:] == 0) and np.all(got["rot_inliers"][1:] == got["trans_inliers"][1:])
