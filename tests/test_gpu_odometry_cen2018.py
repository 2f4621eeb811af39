"""The file-based odometry path with cen2018 keypoints (rsx_odometry_set_cen2018) on a MOVING sensor with known poses: the
windowed pipeline against the CPU chain with the extractor swapped (cen2018 restatement keypoints, then the oracle's front
end, cross-checked ratio matches, max-clique selection and ORORA: oracle/odometry_chain.run's steps), against the true
poses, and through the C++ entry host/odometry --keypoints cen2018.

Truth bounds, measured with the CPU chain below on synth.polar_sequence(11, 22) (10.7 k keypoints and 770-1020 cross-checked
matches per scan): worst pair 0.083 m / 5.6e-3 rad, accumulated 0.454 m / 2.53e-2 rad after 21 pairs.  Per pair the bounds
are those test_gpu_odometry.py holds cen2019 to (0.25 m / 1e-2 rad); accumulated 0.9 m / 4e-2 rad, since the accumulated yaw
error on this data (2.53e-2 rad) is above cen2019's (1.6e-2 rad) and its 2.5e-2 bound.  They pin source / destination order, the yaw
sign and the composition, which a parked sensor cannot (a swapped pair or a flipped sign is off by metres after 21 pairs).
PARITY UNPINNED w.r.t. the reference (the ORORA submodule is absent)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from navtech_radar_slam_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cen2018_np as c18  # noqa: E402

pytestmark = pytest.mark.gpu
HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "navtech-radar-slam_amd", "host")
N_SCANS = 22


def chain_cen2018(images, azimuths, resolution=synth.RADAR_RESOLUTION, col_offset=11, max_keypoints=16384, ratio=0.8,
                  W=964, cart_res=0.2592):
    """oracle/odometry_chain.run with cen2018 (tests/cen2018_np.py) in place of cen2019"""
    from oracle import odometry_chain
    from oracle import pyoracle as po
    images = np.asarray(images)
    az = np.asarray(azimuths, dtype=np.float32)
    n, rows, stride = images.shape
    fe = po.FrontendRef(rows=rows, cols=stride - col_offset, W=W, cart_res=cart_res)
    out, prev, pose = [], None, np.zeros(3)
    for i in range(n):
        azi = az[i] if az.ndim == 2 else az
        tg = c18.extract(images[i], col_offset=col_offset)
        nk = len(tg)
        tg = tg[:max_keypoints]
        xy = c18.to_cartesian(tg, azi, resolution)
        fe.cartesian(images[i], azi, resolution, col_offset=col_offset)
        desc, valid = fe.describe(xy)
        rec = {"n_keypoints": nk, "n_matches": 0, "result": None, "xy": xy, "targets": tg}
        if prev is not None:
            fwd, _, _ = fe.match(prev[1], prev[2], desc, valid, ratio=ratio)
            bwd, _, _ = fe.match(desc, valid, prev[1], prev[2], ratio=ratio)
            ii = np.nonzero(fwd >= 0)[0]
            ii = ii[bwd[fwd[ii]] == ii]
            src, dst = xy[fwd[ii]], prev[0][ii]
            rec["n_matches"] = len(ii)
            tau = po.orora_default_params().tim_noise_bound
            member, _ = po.pmc_select_batch(src, dst, np.array([0, len(ii)], dtype=np.int64), tau)
            src, dst = src[member.astype(bool)], dst[member.astype(bool)]
            r = po.orora_register_batch(src, dst, np.array([0, len(src)], dtype=np.int64))[0]
            rec["result"] = r
            if r["status"] == 0:
                pose = odometry_chain.compose(pose, (r["x"], r["y"], r["yaw"]))
        rec["pose"] = pose.copy()
        out.append(rec)
        prev = (xy, desc, valid)
    return out


@pytest.fixture(scope="module")
def sequence():
    return synth.polar_sequence(11, N_SCANS)


@pytest.fixture(scope="module")
def chain(sequence, oracle):
    imgs, az, _, _ = sequence
    for i in range(len(imgs)):  # the exemption of tests/test_gpu_cen2018.py is not needed on this data: no fragile row
        _, dbg = c18.extract(imgs[i], debug=True)
        assert len(c18.fragile_rows(dbg, 58)) == 0, i
    return chain_cen2018(imgs, az)


def _check(res, xy, chain, poses):
    assert res["status"][0] == 3 and np.all(res["status"][1:] == 0)
    acc = [np.zeros(3)]
    worst_t = worst_y = 0.0
    for i in range(N_SCANS):
        want = chain[i]
        assert res["n_keypoints"][i] == want["n_keypoints"] and res["n_matches"][i] == want["n_matches"], (i, res[i], want["n_keypoints"], want["n_matches"])
        if xy is not None:
            assert np.allclose(xy[i], want["xy"], rtol=1e-5, atol=1e-4)
        if i == 0:
            continue
        w = want["result"]
        assert max(abs(res[f][i] - w[f]) for f in ("x", "y", "yaw")) < 1e-4, (i, res[i], w)
        acc.append(synth.compose_pose(acc[-1], (res["x"][i], res["y"][i], res["yaw"][i])))
        truth = synth.relative_pose(poses[i - 1], poses[i])
        worst_t = max(worst_t, float(np.hypot(res["x"][i] - truth[0], res["y"][i] - truth[1])))
        worst_y = max(worst_y, abs(float(res["yaw"][i] - truth[2])))
    print(f"cen2018 odometry: worst pair {worst_t:.3f} m {worst_y:.2e} rad; accumulated "
          f"{np.hypot(*(acc[-1][:2] - poses[-1][:2])):.3f} m {abs(acc[-1][2] - poses[-1][2]):.2e} rad")
    assert worst_t < 0.25 and worst_y < 1e-2
    assert np.hypot(*(acc[-1][:2] - poses[-1][:2])) < 0.9 and abs(acc[-1][2] - poses[-1][2]) < 4e-2
    assert min(res["n_matches"][1:]) > 500
    return acc


def test_windowed_pipeline_equals_chain_and_truth(sequence, chain):
    from navtech_radar_slam_amd import odometry
    imgs, az, poses, _ = sequence
    od = odometry.Odometry(400, 3360, keypoints="cen2018")
    res, xy = od.push(imgs, az, want_xy=True)
    _check(res, xy, chain, poses)


def test_window_splits_and_device_images_change_nothing(sequence, chain):
    import torch
    from navtech_radar_slam_amd import odometry
    imgs, az, poses, _ = sequence
    od = odometry.Odometry(400, 3360, keypoints="cen2018")
    whole = od.push(imgs, az)
    od.reset()
    parts = np.concatenate([od.push(imgs[a:b], az) for a, b in ((0, 1), (1, 8), (8, 9), (9, N_SCANS))])
    assert np.array_equal(parts, whole)
    od.reset()
    d = torch.from_numpy(np.ascontiguousarray(imgs)).cuda()
    dev = od.push(imgs, az, device_ptr=d.data_ptr())
    assert np.array_equal(dev, whole)
    _check(whole, None, chain, poses)


def test_switching_rules(sequence):
    from navtech_radar_slam_amd import _rsx, cen2018, odometry
    imgs, az, _, _ = sequence
    od = odometry.Odometry(400, 3360, keypoints="cen2018")
    od.push(imgs[:2], az)
    with pytest.raises(_rsx.RsxError):
        od.set_cen2018(off=True)  # holds a scan
    with pytest.raises(_rsx.RsxError):
        od.set_cen2018(cen2018.params(zq=2.0))
    od.reset()
    with pytest.raises(_rsx.RsxError):
        od.set_cen2018(cen2018.params(sigma_gauss=4))
    od.set_cen2018(off=True)
    back = od.push(imgs[:6], az)
    fresh = odometry.Odometry(400, 3360).push(imgs[:6], az)
    assert np.array_equal(back, fresh)
    od.reset()
    od.set_cen2018(cen2018.params(zq=4.0, sigma_gauss=9))
    got = od.push(imgs[:2], az)
    assert got["n_keypoints"][0] == len(c18.extract(imgs[0], zq=4.0, sigma_gauss=9))


def _run_entry(seq_dir, *flags):
    r = subprocess.run([os.path.join(HOST, "odometry"), f"seq_dir:={seq_dir}", "do_slam:=true", *flags], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [line.split() for line in r.stdout.strip().splitlines()]
    return np.array([[float(v) for v in x[1:]] for x in rows]), np.array([int(x[0]) for x in rows], dtype=np.int64)


def test_host_entry_on_png_files(sequence, chain, tmp_path):
    """host/odometry --keypoints cen2018 on PNG files == the pipeline (windowed and --per-scan)"""
    from PIL import Image
    imgs, az, poses, stamps = sequence
    d = tmp_path / "seq" / "polar_oxford_form"
    d.mkdir(parents=True)
    for img, st in zip(imgs, stamps):
        Image.fromarray(img, mode="L").save(str(d / f"{int(st)}.png"))
    seq = tmp_path / "seq"
    got, got_stamps = _run_entry(seq, "--keypoints", "cen2018", "--zq", "3", "--sigma-gauss", "17", "--window", "7")
    assert got.shape == (N_SCANS, 5) and np.array_equal(got_stamps, stamps)
    want_pose = np.stack([c["pose"] for c in chain])
    assert np.allclose(got[:, 0:3], want_pose, atol=2e-4), np.abs(got[:, 0:3] - want_pose).max()
    assert np.array_equal(got[:, 3], [c["n_keypoints"] for c in chain]) and np.array_equal(got[:, 4], [c["n_matches"] for c in chain])
    per_scan, _ = _run_entry(seq, "--keypoints", "cen2018", "--per-scan")
    assert np.allclose(per_scan, got, atol=2e-6)
    other, _ = _run_entry(seq, "--keypoints", "cen2018", "--zq", "4.5", "--sigma-gauss", "9", "--max_frames", "2")
    assert other[0, 3] == len(c18.extract(imgs[0], zq=4.5, sigma_gauss=9))
    bad = subprocess.run([os.path.join(HOST, "odometry"), f"seq_dir:={seq}", "--keypoints", "orb"], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0
