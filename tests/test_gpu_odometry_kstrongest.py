"""The file-based odometry path with k-strongest keypoints (rsx_odometry_set_kstrongest) on a MOVING sensor with known poses:
the windowed pipeline against the CPU chain with the extractor swapped (k-strongest restatement keypoints, then the oracle's
front end, cross-checked ratio matches, max-clique selection and ORORA: oracle/odometry_chain.run's steps), against the true
poses, and through the C++ entry host/odometry --keypoints kstrongest.

Six scans of synth.polar_sequence(11, 6) with k = 12, min_separation = 5 (the CPU chain takes about ten seconds on them).
Measured with the CPU chain below: 4800 keypoints per scan, 605 / 694 / 557 / 685 / 631 cross-checked matches on the five pairs
(the smallest: 557), every pair status 0, worst pair over all five pairs 0.017 m / 3.1e-3 rad.  Per pair the bounds are those
test_gpu_odometry.py holds cen2019 to (0.25 m / 1e-2 rad), and every pair must keep more than half the chain's smallest match
count (more than 278).
PARITY UNPINNED w.r.t. the reference (the ORORA submodule is absent; k-strongest is not part of it)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from navtech_radar_slam_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cen2018_np as c18  # noqa: E402
import kstrongest_np as ksn  # noqa: E402

pytestmark = pytest.mark.gpu
HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "navtech-radar-slam_amd", "host")
N_SCANS = 6
K, SEP = 12, 5
CHAIN_MIN_MATCHES = 557  # the smallest n_matches of the CPU chain on these six scans (asserted in the `chain` fixture)


def chain_kstrongest(images, azimuths, resolution=synth.RADAR_RESOLUTION, col_offset=11, max_keypoints=16384, ratio=0.8,
                     W=964, cart_res=0.2592, **params):
    """oracle/odometry_chain.run with k-strongest (tests/kstrongest_np.py) in place of cen2019"""
    from oracle import odometry_chain
    from oracle import pyoracle as po
    images = np.asarray(images)
    az = np.asarray(azimuths, dtype=np.float32)
    n, rows, stride = images.shape
    fe = po.FrontendRef(rows=rows, cols=stride - col_offset, W=W, cart_res=cart_res)
    out, prev, pose = [], None, np.zeros(3)
    for i in range(n):
        azi = az[i] if az.ndim == 2 else az
        tg = ksn.extract(images[i], col_offset=col_offset, **params)
        nk = len(tg)
        tg = tg[:max_keypoints]
        xy = ksn.to_cartesian(tg, azi, resolution)
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
    imgs, az, poses, _ = sequence
    out = chain_kstrongest(imgs, az, k=K, min_separation=SEP)
    worst_t = worst_y = 0.0
    for i in range(1, N_SCANS):
        r, truth = out[i]["result"], synth.relative_pose(poses[i - 1], poses[i])
        assert r["status"] == 0
        worst_t = max(worst_t, float(np.hypot(r["x"] - truth[0], r["y"] - truth[1])))
        worst_y = max(worst_y, abs(float(r["yaw"] - truth[2])))
    print(f"k-strongest CPU chain: matches {[c['n_matches'] for c in out[1:]]}, worst pair {worst_t:.3f} m {worst_y:.2e} rad")
    assert min(c["n_matches"] for c in out[1:]) == CHAIN_MIN_MATCHES
    return out


def _check(res, xy, chain, poses):
    assert res["status"][0] == 3 and np.all(res["status"][1:] == 0)
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
        truth = synth.relative_pose(poses[i - 1], poses[i])
        worst_t = max(worst_t, float(np.hypot(res["x"][i] - truth[0], res["y"][i] - truth[1])))
        worst_y = max(worst_y, abs(float(res["yaw"][i] - truth[2])))
    print(f"k-strongest odometry: worst pair {worst_t:.3f} m {worst_y:.2e} rad")
    assert worst_t < 0.25 and worst_y < 1e-2
    assert min(res["n_matches"][1:]) > CHAIN_MIN_MATCHES // 2


def _odometry(**kw):
    from navtech_radar_slam_amd import kstrongest, odometry
    return odometry.Odometry(400, 3360, keypoints="kstrongest", kstrongest=kstrongest.params(k=K, min_separation=SEP), **kw)


def test_windowed_pipeline_equals_chain_and_truth(sequence, chain):
    imgs, az, poses, _ = sequence
    res, xy = _odometry().push(imgs, az, want_xy=True)
    _check(res, xy, chain, poses)


def test_window_splits_and_device_images_change_nothing(sequence, chain):
    import torch
    imgs, az, poses, _ = sequence
    od = _odometry()
    whole = od.push(imgs, az)
    od.reset()
    parts = np.concatenate([od.push(imgs[a:b], az) for a, b in ((0, 1), (1, 4), (4, 6))])
    assert np.array_equal(parts, whole)
    od.reset()
    d = torch.from_numpy(np.ascontiguousarray(imgs)).cuda()
    dev = od.push(imgs, az, device_ptr=d.data_ptr())
    assert np.array_equal(dev, whole)
    _check(whole, None, chain, poses)


def test_switching_rules(sequence):
    from navtech_radar_slam_amd import _rsx, cen2018, kstrongest, odometry
    imgs, az, _, _ = sequence
    od = _odometry()
    od.push(imgs[:2], az)
    with pytest.raises(_rsx.RsxError):
        od.set_kstrongest(off=True)  # holds a scan
    with pytest.raises(_rsx.RsxError):
        od.set_kstrongest(kstrongest.params(k=3))
    od.reset()
    for bad in (dict(k=0), dict(k=129), dict(z_min=256), dict(min_range=-1), dict(max_range=-1), dict(min_separation=33)):
        with pytest.raises(_rsx.RsxError):
            od.set_kstrongest(kstrongest.params(**bad))
    od.set_kstrongest(off=True)  # kstrongest -> off == a fresh cen2019 handle
    back = od.push(imgs[:4], az)
    fresh = odometry.Odometry(400, 3360).push(imgs[:4], az)
    assert np.array_equal(back, fresh)
    # cen2018 -> kstrongest -> cen2018: each takes effect
    od.reset()
    od.set_cen2018(cen2018.params(zq=4.0, sigma_gauss=9))
    n18 = len(c18.extract(imgs[0], zq=4.0, sigma_gauss=9))
    assert od.push(imgs[:1], az)["n_keypoints"][0] == n18
    od.reset()
    od.set_kstrongest(kstrongest.params(k=7, z_min=110, min_separation=0))  # the plain rule
    assert od.push(imgs[:1], az)["n_keypoints"][0] == len(ksn.extract(imgs[0], k=7, z_min=110, min_separation=0)) != n18
    od.reset()
    od.set_cen2018(cen2018.params(zq=4.0, sigma_gauss=9))
    assert od.push(imgs[:1], az)["n_keypoints"][0] == n18
    od.reset()
    od.set_cen2018(off=True)  # NULL in either setter: back to cen2019
    assert np.array_equal(od.push(imgs[:1], az), fresh[:1])


def _run_entry(seq_dir, *flags):
    r = subprocess.run([os.path.join(HOST, "odometry"), f"seq_dir:={seq_dir}", "do_slam:=true", *flags], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [line.split() for line in r.stdout.strip().splitlines()]
    return np.array([[float(v) for v in x[1:]] for x in rows]), np.array([int(x[0]) for x in rows], dtype=np.int64)


def test_host_entry_on_png_files(sequence, chain, tmp_path):
    """host/odometry --keypoints kstrongest on PNG files == the chain (windowed and --per-scan)"""
    from PIL import Image
    imgs, az, poses, stamps = sequence
    d = tmp_path / "seq" / "polar_oxford_form"
    d.mkdir(parents=True)
    for img, st in zip(imgs, stamps):
        Image.fromarray(img, mode="L").save(str(d / f"{int(st)}.png"))
    seq = tmp_path / "seq"
    got, got_stamps = _run_entry(seq, "--keypoints", "kstrongest", "--k", str(K), "--min-separation", str(SEP), "--window", "4")
    assert got.shape == (N_SCANS, 5) and np.array_equal(got_stamps, stamps)
    want_pose = np.stack([c["pose"] for c in chain])
    assert np.allclose(got[:, 0:3], want_pose, atol=2e-4), np.abs(got[:, 0:3] - want_pose).max()
    assert np.array_equal(got[:, 3], [c["n_keypoints"] for c in chain]) and np.array_equal(got[:, 4], [c["n_matches"] for c in chain])
    per_scan, _ = _run_entry(seq, "--keypoints", "kstrongest", "--k", str(K), "--min-separation", str(SEP), "--per-scan")
    assert np.allclose(per_scan, got, atol=2e-6)
    other, _ = _run_entry(seq, "--keypoints", "kstrongest", "--k", "5", "--z-min", "80", "--min-separation", "0", "--max_frames", "2")
    assert other[0, 3] == len(ksn.extract(imgs[0], k=5, z_min=80, min_separation=0))
    bad = subprocess.run([os.path.join(HOST, "odometry"), f"seq_dir:={seq}", "--keypoints", "orb"], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0
