"""The file-based odometry path with CA-CFAR / BFAR keypoints (rsx_odometry_set_cfar) on a MOVING sensor with known poses: the
windowed pipeline against the CPU chain with the extractor swapped (tests/keypoint_chain.py: CFAR restatement keypoints, then
the oracle's front end, cross-checked ratio matches, max-clique selection and ORORA), against the true poses, the slot's wiring
against k-strongest at A = 0, and the C++ entry host/odometry --keypoints cfar.

Four scans of synth.polar_sequence(11, 4) with the defaults (a = 3, b = 20, t = 20, g = 2, cell averaging, k = 12, s = 5).
Measured with the CPU chain below: 4800 / 4796 / 4800 / 4800 keypoints, 434 / 538 / 446 cross-checked matches on the three
pairs, every pair status 0, worst pair 0.021 m / 2.6e-3 rad.
Per pair the bounds are those every other extractor is held to (0.25 m / 1e-2 rad).
PARITY UNPINNED w.r.t. the reference (the ORORA submodule is absent; CFAR is not part of it)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from navtech_radar_slam_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cen2018_np as c18  # noqa: E402
import cfar_np as cfn  # noqa: E402
import keypoint_chain  # noqa: E402
import kstrongest_np as ksn  # noqa: E402

pytestmark = pytest.mark.gpu
HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "navtech-radar-slam_amd", "host")
N_SCANS = 4
CHAIN_MATCHES = [434, 538, 446]  # n_matches of the CPU chain on the three pairs (asserted in the `chain` fixture)


@pytest.fixture(scope="module")
def sequence():
    return synth.polar_sequence(11, N_SCANS)


@pytest.fixture(scope="module")
def chain(sequence, oracle):
    imgs, az, poses, _ = sequence
    out = keypoint_chain.run(lambda img: cfn.extract(img, scale_q8=768, offset=20), imgs, az)
    status, worst_t, worst_y = keypoint_chain.pair_errors(out, poses)
    print(f"CFAR CPU chain: matches {[c['n_matches'] for c in out[1:]]}, worst pair {worst_t:.3f} m {worst_y:.2e} rad")
    assert status == [0] * (N_SCANS - 1)
    assert worst_t < 0.25 and worst_y < 1e-2
    assert [c["n_matches"] for c in out[1:]] == CHAIN_MATCHES
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
    print(f"CFAR odometry: worst pair {worst_t:.3f} m {worst_y:.2e} rad")
    assert worst_t < 0.25 and worst_y < 1e-2


def _odometry(**kw):
    from navtech_radar_slam_amd import odometry
    return odometry.Odometry(400, 3360, keypoints="cfar", **kw)


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
    parts = np.concatenate([od.push(imgs[a:b], az) for a, b in ((0, 1), (1, 3), (3, 4))])
    assert parts.tobytes() == whole.tobytes()
    od.reset()
    d = torch.from_numpy(np.ascontiguousarray(imgs)).cuda()
    dev = od.push(imgs, az, device_ptr=d.data_ptr())
    assert dev.tobytes() == whole.tobytes()
    _check(whole, None, chain, poses)


@pytest.mark.parametrize("config", ["orora", "ransac", "cfear_track"])
def test_slot_wiring_equals_kstrongest_at_scale_zero(sequence, config):
    """A = 0, B = 59 is k-strongest with z_min = 60: the same bytes out of the pipeline whatever stands behind the extractor"""
    from navtech_radar_slam_amd import cfar, cfear, kstrongest, odometry
    imgs, az, _, _ = sequence
    s = 0 if config == "cfear_track" else 5
    kw = {"orora": {}, "ransac": dict(estimator="ransac"),
          "cfear_track": dict(estimator="cfear", cfear_track=cfear.track_params(n_keyframes=3))}[config]
    got = odometry.Odometry(400, 3360, keypoints="cfar", cfar=cfar.params(k=12, scale_q8=0, offset=59, min_separation=s), **kw).push(imgs, az)
    want = odometry.Odometry(400, 3360, keypoints="kstrongest", kstrongest=kstrongest.params(k=12, z_min=60, min_separation=s), **kw).push(imgs, az)
    assert got.tobytes() == want.tobytes()
    assert np.all(got["n_keypoints"] > 0) and np.all(got["status"][1:] == 0)


def test_switching_rules(sequence):
    from navtech_radar_slam_amd import _rsx, cen2018, cfar, kstrongest, odometry
    imgs, az, _, _ = sequence
    od = _odometry()
    od.push(imgs[:2], az)
    with pytest.raises(_rsx.RsxError):
        od.set_cfar(off=True)  # holds a scan
    with pytest.raises(_rsx.RsxError):
        od.set_cfar(cfar.params(k=3))
    od.reset()
    for bad in (dict(k=0), dict(k=129), dict(train=0), dict(train=65), dict(guard=17), dict(scale_q8=65536), dict(scale_q8=-1), dict(offset=256),
                dict(mode=3), dict(min_range=-1), dict(max_range=-1), dict(min_separation=33)):
        with pytest.raises(_rsx.RsxError):
            od.set_cfar(cfar.params(**bad))
    od.set_cfar(off=True)  # cfar -> off == a fresh cen2019 handle
    back = od.push(imgs[:3], az)
    fresh = odometry.Odometry(400, 3360).push(imgs[:3], az)
    assert back.tobytes() == fresh.tobytes()
    # kstrongest -> cfar -> cen2018: each takes effect
    od.reset()
    od.set_kstrongest(kstrongest.params(k=7, z_min=110, min_separation=0))
    nks = len(ksn.extract(imgs[0], k=7, z_min=110, min_separation=0))
    assert od.push(imgs[:1], az)["n_keypoints"][0] == nks
    od.reset()
    od.set_cfar(cfar.params(k=9, scale_q8=1024, offset=20, mode=cfar.CFAR_GO))
    ncf = len(cfn.extract(imgs[0], k=9, scale_q8=1024, offset=20, mode=1))
    assert od.push(imgs[:1], az)["n_keypoints"][0] == ncf
    od.reset()
    od.set_cen2018(cen2018.params(zq=4.0, sigma_gauss=9))
    n18 = len(c18.extract(imgs[0], zq=4.0, sigma_gauss=9))
    assert od.push(imgs[:1], az)["n_keypoints"][0] == n18
    assert len({nks, ncf, n18}) == 3 and min(nks, ncf, n18) > 0


def _run_entry(seq_dir, *flags):
    r = subprocess.run([os.path.join(HOST, "odometry"), f"seq_dir:={seq_dir}", "do_slam:=true", *flags], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [line.split() for line in r.stdout.strip().splitlines()]
    return np.array([[float(v) for v in x[1:]] for x in rows]), np.array([int(x[0]) for x in rows], dtype=np.int64)


def test_host_entry_on_png_files(sequence, chain, tmp_path):
    """host/odometry --keypoints cfar on PNG files == the chain (windowed and --per-scan)"""
    from PIL import Image
    imgs, az, poses, stamps = sequence
    d = tmp_path / "seq" / "polar_oxford_form"
    d.mkdir(parents=True)
    for img, st in zip(imgs, stamps):
        Image.fromarray(img, mode="L").save(str(d / f"{int(st)}.png"))
    seq = tmp_path / "seq"
    got, got_stamps = _run_entry(seq, "--keypoints", "cfar", "--window", "3")
    assert got.shape == (N_SCANS, 5) and np.array_equal(got_stamps, stamps)
    want_pose = np.stack([c["pose"] for c in chain])
    assert np.allclose(got[:, 0:3], want_pose, atol=2e-4), np.abs(got[:, 0:3] - want_pose).max()
    assert np.array_equal(got[:, 3], [c["n_keypoints"] for c in chain]) and np.array_equal(got[:, 4], [c["n_matches"] for c in chain])
    per_scan, _ = _run_entry(seq, "--keypoints", "cfar", "--per-scan")
    assert np.allclose(per_scan[:, 0:3], want_pose, atol=2e-4)
    assert np.allclose(per_scan, got, atol=2e-6)
    other, _ = _run_entry(seq, "--keypoints", "cfar", "--cfar-mode", "go", "--cfar-scale", "4", "--cfar-offset", "20", "--max_frames", "1")
    assert other[0, 3] == len(cfn.extract(imgs[0], scale_q8=1024, offset=20, mode=1))
    bad = subprocess.run([os.path.join(HOST, "odometry"), f"seq_dir:={seq}", "--keypoints", "cfar", "--cfar-mode", "xx"], capture_output=True, text=True,
                         timeout=120)
    assert bad.returncode != 0
