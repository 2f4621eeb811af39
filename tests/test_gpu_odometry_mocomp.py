"""The file-based odometry path with motion / Doppler compensation (rsx_odometry_set_compensation): every pair estimated,
its matches compensated with that estimate (csrc/mocomp.hip) and estimated again, against the same two passes on the CPU --
oracle/odometry_chain.run's steps up to the cross-checked matches, then the oracle's max-clique selection + ORORA (or
tests/ransac_np.py), the restatement tests/mocomp_np.py, and the estimator again -- for every cut of the sequence into calls;
the published cloud; the switching rules; and the accuracy of the scheme on ground-truth pairs (tests/mocomp_cases.py).
The polar sequence's scans are synthesised as snapshots, so its poses cannot show an accuracy gain and nothing is asserted
about one there.  PARITY UNPINNED w.r.t. upstream (its sources are absent)."""
import os
import sys

import numpy as np
import pytest

from navtech_radar_slam_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mocomp_cases as mc  # noqa: E402
import mocomp_np as mn  # noqa: E402
import ransac_np as rn  # noqa: E402

pytestmark = pytest.mark.gpu
N_SCANS, ROWS, DT_SCAN, BETA = 7, 400, 0.25, 0.049
FLAGS = {"motion": 1, "doppler": 2, "both": 3}


@pytest.fixture(scope="module")
def sequence():
    return synth.polar_sequence(11, N_SCANS)


@pytest.fixture(scope="module")
def matched(sequence, oracle):
    """the chain up to the cross-checked matches, once: per scan (targets, xy, src, dst, a_cur, a_prev)"""
    po = oracle
    images, azimuths, _, _ = sequence
    n, rows, stride = images.shape
    fe = po.FrontendRef(rows=rows, cols=stride - 11, W=964, cart_res=0.2592)
    out, prev = [], None
    for i in range(n):
        tg = np.asarray(po.cen2019_extract(images[i], col_offset=11, max_points=10000, min_range=58))
        nk = len(tg)
        tg = tg[:16384]
        xy = po.cen2019_to_cartesian(tg, azimuths, synth.RADAR_RESOLUTION)
        fe.cartesian(images[i], azimuths, synth.RADAR_RESOLUTION, col_offset=11)
        desc, valid = fe.describe(xy)
        rec = {"n_keypoints": nk, "targets": tg, "xy": xy, "src": None}
        if prev is not None:
            fwd, _, _ = fe.match(prev[1], prev[2], desc, valid, ratio=0.8)
            bwd, _, _ = fe.match(desc, valid, prev[1], prev[2], ratio=0.8)
            ii = np.nonzero(fwd >= 0)[0]
            ii = ii[bwd[fwd[ii]] == ii]
            rec.update(src=xy[fwd[ii]], dst=prev[0][ii], a_cur=tg[fwd[ii], 0].astype(np.int32), a_prev=prev[3][ii, 0].astype(np.int32))
        out.append(rec)
        prev = (xy, desc, valid, tg)
    return out


def _estimate(po, estimator, src, dst):
    """one pair through the CPU estimator -> dict(x, y, yaw, status, counts = what rsx_odometry_scan.reg carries, n_selected)"""
    if estimator == "orora":
        off = np.array([0, len(src)], dtype=np.int64)
        member, info = po.pmc_select_batch(src, dst, off, po.orora_default_params().tim_noise_bound)
        s, d, o = po.pmc_compact(src, dst, off, member)
        r = po.orora_register_batch(s, d, o)[0]
        return dict(x=r["x"], y=r["y"], yaw=r["yaw"], status=int(r["status"]), n_selected=int(info[0]["size"]),
                    counts=(int(r["iterations"]), int(r["rot_inliers"]), int(r["trans_inliers"])))
    r = rn.estimate(src, dst, None, mc=False, debug=True)
    assert r["margin"] > 1e-9, r["margin"]   # no match on the threshold: the counts are exact
    return dict(x=r["x"], y=r["y"], yaw=r["yaw"], status=r["status"], n_selected=len(src), counts=(r["hypotheses"], r["inliers"], r["inliers"]))


def two_pass_chain(po, matched, estimator, flags):
    out = []
    for rec in matched:
        if rec["src"] is None:
            out.append(None)
            continue
        r1 = _estimate(po, estimator, rec["src"], rec["dst"])
        r2, s2, d2 = r1, rec["src"], rec["dst"]
        if r1["status"] == 0:
            s2, d2, _ = mn.matches_batch(rec["src"], rec["dst"], rec["a_cur"], rec["a_prev"], [0, len(rec["src"])], [[r1["x"], r1["y"], r1["yaw"]]],
                                         flags, dt_scan=DT_SCAN, beta=BETA, rows=ROWS)
            r2 = _estimate(po, estimator, s2, d2)
        out.append(dict(first=r1, second=r2, src2=s2, dst2=d2))
    return out


@pytest.mark.parametrize("estimator", ["orora", "ransac"])
def test_pipeline_equals_two_pass_chain_for_every_window_cut(sequence, matched, oracle, estimator):
    from navtech_radar_slam_amd import _rsx, odometry, orora
    imgs, az, _, _ = sequence
    chain = two_pass_chain(oracle, matched, estimator, 3)
    od = odometry.Odometry(ROWS, 3360, estimator=estimator, compensate="both")
    whole = od.push(imgs, az)
    plain = odometry.Odometry(ROWS, 3360, estimator=estimator).push(imgs, az)
    assert whole["status"][0] == 3
    worst = 0.0
    for i in range(N_SCANS):
        assert whole["n_keypoints"][i] == matched[i]["n_keypoints"]
        if i == 0:
            continue
        want = chain[i]["second"]
        assert whole["n_matches"][i] == len(matched[i]["src"]) and want["status"] == 0
        got = (int(whole["iterations"][i]), int(whole["rot_inliers"][i]), int(whole["trans_inliers"][i]))
        assert whole["status"][i] == 0 and got == want["counts"], (i, whole[i], want)
        worst = max(worst, max(abs(whole[f][i] - want[f]) for f in ("x", "y", "yaw")))
    print(f"{estimator}: max |pose - two-pass chain| {worst:.3e}")
    assert worst < 1e-4
    assert not np.array_equal(whole[["x", "y", "yaw"]][1:], plain[["x", "y", "yaw"]][1:])   # the second pass is what is reported
    if estimator == "orora":
        # selection sizes of both passes: the library's selection on the chain's matches of each pass
        src1 = np.concatenate([m["src"] for m in matched[1:]])
        dst1 = np.concatenate([m["dst"] for m in matched[1:]])
        src2 = np.concatenate([c["src2"] for c in chain[1:]])
        dst2 = np.concatenate([c["dst2"] for c in chain[1:]])
        off = np.zeros(N_SCANS, dtype=np.int64)
        off[1:] = np.cumsum([len(m["src"]) for m in matched[1:]])
        reg = orora.Orora()
        for (s, d), key in (((src1, dst1), "first"), ((src2, dst2), "second")):
            _, info = reg.max_clique_batch(s, d, off)
            assert info["size"].tolist() == [c[key]["n_selected"] for c in chain[1:]], key
        prm = orora.default_params()
        prm.flags |= _rsx.ORORA_PMC
        r2 = reg.register_batch(src2, dst2, off, prm)
        assert [(int(r["iterations"]), int(r["rot_inliers"]), int(r["trans_inliers"])) for r in r2] == [c["second"]["counts"] for c in chain[1:]]
    # the same scans as two calls and scan by scan
    od.reset()
    two = np.concatenate([od.push(imgs[:3], az), od.push(imgs[3:], az)])
    assert two.tobytes() == whole.tobytes()
    od.reset()
    single = np.concatenate([od.push(imgs[i:i + 1], az) for i in range(N_SCANS)])
    assert single.tobytes() == whole.tobytes()


@pytest.mark.parametrize("mode", ["both", "motion", "doppler"])
def test_published_cloud_is_the_restatement_under_the_pipelines_own_velocities(sequence, matched, mode):
    from navtech_radar_slam_amd import odometry
    imgs, az, _, _ = sequence
    raw_rec, raw_xy = odometry.Odometry(ROWS, 3360).push(imgs, az, want_xy=True)
    od = odometry.Odometry(ROWS, 3360, compensate=mode)
    rec, xy = od.push(imgs, az, want_xy=True)
    moved = 0
    for i in range(N_SCANS):
        # the uncompensated cloud is the chain's up to the last bit of the device's fp32 sin / cos (the rule of
        # tests/test_gpu_odometry.py), keypoint for keypoint: the chain's azimuth rows belong to the pipeline's points
        assert raw_xy[i].shape == matched[i]["xy"].shape
        assert np.array_equal(raw_xy[i], matched[i]["xy"]) or np.allclose(raw_xy[i], matched[i]["xy"], rtol=1e-5, atol=1e-4)
        rows = matched[i]["targets"][:len(raw_xy[i]), 0]
        if i == 0 or rec["status"][i] != 0:
            want = raw_xy[i]
        else:
            vx, vy, wz, ok = mn.velocity_of(rec["x"][i], rec["y"][i], rec["yaw"][i], DT_SCAN)
            assert ok
            want, bad = mn.compensate(raw_xy[i], rows, float(vx), float(vy), float(wz), FLAGS[mode], dt_scan=DT_SCAN, beta=BETA, rows=ROWS)
            assert not bad.any()
            moved += int(np.sum(np.any(want != raw_xy[i], axis=1)))
        assert mn.same_bits(xy[i], want), (mode, i)
    assert moved > 1000
    assert np.array_equal(rec["n_keypoints"], raw_rec["n_keypoints"]) and np.array_equal(rec["n_matches"], raw_rec["n_matches"])
    # cut into two calls, and with a shorter max_xy: the same records and clouds
    od.reset()
    r_a, xy_a = od.push(imgs[:4], az, want_xy=True)
    r_b, xy_b = od.push(imgs[4:], az, want_xy=True, max_xy=100)
    assert np.concatenate([r_a, r_b]).tobytes() == rec.tobytes()
    assert all(np.array_equal(a, b) for a, b in zip(xy_a, xy[:4])) and all(np.array_equal(a, b[:100]) for a, b in zip(xy_b, xy[4:]))


def test_switching_rules_and_the_default_path(sequence):
    from navtech_radar_slam_amd import _rsx, mocomp, odometry
    imgs, az, _, _ = sequence
    fresh, fresh_xy = odometry.Odometry(ROWS, 3360).push(imgs[:5], az, want_xy=True)
    od = odometry.Odometry(ROWS, 3360)
    od.set_compensation(None)                       # off is the default: still the default bytes
    got, got_xy = od.push(imgs[:5], az, want_xy=True)
    assert got.tobytes() == fresh.tobytes() and all(np.array_equal(a, b) for a, b in zip(got_xy, fresh_xy))
    for mode in ("both", None):
        with pytest.raises(_rsx.RsxError):
            od.set_compensation(mode)               # holds a scan
    od.reset()
    for flags in (0, 4):
        with pytest.raises(_rsx.RsxError):
            od.set_compensation(mocomp.default_params(flags=flags))
    with pytest.raises(_rsx.RsxError):
        od.set_compensation("both", dt_scan=0.0)
    od.set_estimator("mcransac")
    with pytest.raises(_rsx.RsxError):
        od.set_compensation("both")                 # MC-RANSAC has its own motion model
    od.set_estimator("ransac")
    od.set_compensation("motion")
    with pytest.raises(_rsx.RsxError):
        od.set_estimator("mcransac")
    on = od.push(imgs[:5], az)
    assert np.all(on["status"][1:] == 0)
    od.reset()
    od.set_estimator("orora")
    od.set_compensation("both", beta=-0.049)
    neg = od.push(imgs[:5], az)
    od.reset()
    od.set_compensation("both")
    pos = od.push(imgs[:5], az)
    assert np.all(neg["status"][1:] == 0) and not np.array_equal(neg[["x", "y", "yaw"]], pos[["x", "y", "yaw"]])
    assert not np.array_equal(pos[["x", "y", "yaw"]], fresh[["x", "y", "yaw"]])
    od.reset()
    od.set_compensation(None)
    back, back_xy = od.push(imgs[:5], az, want_xy=True)
    assert back.tobytes() == fresh.tobytes() and all(np.array_equal(a, b) for a, b in zip(back_xy, fresh_xy))
    with pytest.raises(ValueError):
        odometry.Odometry(ROWS, 3360, compensate="deskew")
    with pytest.raises(_rsx.RsxError):
        odometry.Odometry(ROWS, 3360, estimator="mcransac", compensate="both")
    assert _rsx.lib().rsx_odometry_set_compensation(None, None) == -1


def test_two_pass_scheme_on_the_gpu_against_the_truth():
    """rsx_orora_register_batch + rsx_mocomp_matches_batch + rsx_orora_register_batch on the ground-truth pairs: the bound of
    tests/test_mocomp_restatement.py (1.5 x the CPU oracle's worst compensated error)."""
    from navtech_radar_slam_amd import _rsx, mocomp, orora
    S = mc.default_set()
    reg, mo = orora.Orora(), mocomp.Mocomp()
    prm = orora.default_params()
    prm.flags |= _rsx.ORORA_PMC
    r1 = reg.register_batch(S["src"], S["dst"], S["offsets"], prm)
    pose1 = np.stack([r1["x"], r1["y"], r1["yaw"]], axis=1)
    s2, d2, st = mo.matches_batch(S["src"], S["dst"], S["a_cur"], S["a_prev"], S["offsets"], pose1,
                                  mocomp.default_params(rows=mc.ROWS, dt_scan=mc.DT_SCAN, beta=mc.BETA))
    r2 = reg.register_batch(s2, d2, S["offsets"], prm)
    assert not st.any() and np.all(r1["status"] == 0) and np.all(r2["status"] == 0)
    e1 = [mc.pose_error((r1["x"][i], r1["y"][i], r1["yaw"][i]), S["pose"][i]) for i in range(mc.N_PAIRS)]
    e2 = [mc.pose_error((r2["x"][i], r2["y"][i], r2["yaw"][i]), S["pose"][i]) for i in range(mc.N_PAIRS)]
    print("uncompensated:", " ".join(f"{e:.6f}" for e in e1), " worst", f"{max(e1):.6f}")
    print("compensated:  ", " ".join(f"{e:.6f}" for e in e2), " worst", f"{max(e2):.6f}")
    assert all(b < a for a, b in zip(e1, e2))
    assert max(e2) <= mc.COMPENSATED_BOUND
