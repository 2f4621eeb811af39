"""GPU parity of rigid RANSAC and motion-compensated RANSAC (csrc/ransac.hip through the C-ABI) against the numpy
restatement tests/ransac_np.py (the contract; PARITY UNPINNED w.r.t. upstream, whose sources are absent).

Per pair: status, hypotheses and inliers equal, the inlier mask identical, pose and velocity within 1e-4 (the project's pose
tolerance; the kernel adds in the restatement's order, so the measured difference -- printed -- is near 1e-12 and below).
Guard band: the device's sin / cos / atan2 may differ from numpy's in the last bit, so a pair is left out of the comparison
when, under the restatement, an evaluated hypothesis has a match with | |r| - tolerance | < 1e-9 m; at most 1 % of a test's
pairs may be left out, which each test asserts.  On synth.orora_pairs(777, 200) with seed 1 the smallest such margin is
1.23e-7 m (none left out); with seed 0 it is 2.8e-8 m."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from navtech_radar_slam_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ransac_np as rn  # noqa: E402

pytestmark = pytest.mark.gpu
POSE_TOL, GUARD = 1e-4, 1e-9
FIELDS = ("x", "y", "yaw", "vx", "vy", "wz")


@pytest.fixture(scope="module")
def est():
    from navtech_radar_slam_amd import _rsx, ransac
    assert _rsx.device_count() >= 1
    return ransac.Ransac()


def _params(mc=False, **kw):
    from navtech_radar_slam_amd import ransac
    return ransac.default_params(mc=mc, **kw)


def _compare(got, mask, want, off, what, max_left_out=0.01):
    """-> the largest pose / velocity difference; asserts everything else"""
    left_out, worst = 0, 0.0
    for i, w in enumerate(want):
        if w.get("margin", np.inf) < GUARD:
            left_out += 1
            continue
        g = got[i]
        assert (g["status"], g["hypotheses"], g["inliers"], g["gn_iterations"]) == (w["status"], w["hypotheses"], w["inliers"], w["gn_iterations"]), (what, i, g, w)
        assert np.array_equal(mask[off[i]:off[i + 1]], w["mask"]), (what, i)
        worst = max(worst, max(abs(float(g[f]) - w[f]) for f in FIELDS))
    print(f"{what}: {len(want)} pairs, {left_out} left out, max |pose / velocity difference| {worst:.3e}")
    assert left_out <= max_left_out * len(want)
    assert worst < POSE_TOL
    return worst


def test_rigid_matches_restatement(est):
    src, dst, off, truth = synth.orora_pairs(777, 200)
    want = rn.estimate_batch(src, dst, off, debug=True, seed=1)
    assert min(w["margin"] for w in want) > 1e-7
    got, mask = est.estimate_batch(src, dst, off, params=_params(seed=1))
    _compare(got, mask, want, off, "rigid, orora_pairs(777, 200)", max_left_out=0.0)
    assert np.all(got["status"] == 0) and np.all(got["vx"] == 0)
    assert np.median(np.hypot(got["x"] - truth[:, 0], got["y"] - truth[:, 1])) < 0.05   # noisy data: the truth only roughly
    # other parameters
    kw = dict(seed=12345678901234567, tolerance=0.2, inlier_ratio=0.25, max_iterations=1024)
    want = rn.estimate_batch(src[:off[40]], dst[:off[40]], off[:41], debug=True, **kw)
    got, mask = est.estimate_batch(src[:off[40]], dst[:off[40]], off[:41], params=_params(**kw))
    _compare(got, mask, want, off, "rigid, 1024 hypotheses, ratio 0.25")
    assert got["hypotheses"].min() < 1024   # the early stop is taken


def test_mc_matches_restatement(est):
    src, dst, dt, off, truth, inl = synth.motion_distorted_pairs(5, 20)
    want = rn.estimate_batch(src, dst, off, dt=dt, mc=True, debug=True)
    got, mask = est.estimate_batch(src, dst, off, dt=dt, params=_params(mc=True))
    _compare(got, mask, want, off, "MC, motion_distorted_pairs(5, 20)")
    assert np.array_equal(mask, inl)
    assert max(np.abs(got[f] - truth[:, k]).max() for k, f in enumerate(("vx", "vy", "wz"))) < 1.4e-5   # tests/test_ransac_restatement.py
    # the rigid estimator on the same sets, and MC on noisy rigid pairs with one dt (a rigid motion is a constant-velocity one)
    want = rn.estimate_batch(src, dst, off, debug=True)
    got, mask = est.estimate_batch(src, dst, off)
    _compare(got, mask, want, off, "rigid on the motion-distorted sets")
    src, dst, off, _ = synth.orora_pairs(777, 60)
    dt = np.full(len(src), 0.25, dtype=np.float32)
    kw = dict(seed=1, dt_scan=0.3, max_gn_iterations=4, gn_epsilon=1e-9)
    want = rn.estimate_batch(src, dst, off, dt=dt, mc=True, debug=True, **kw)
    got, mask = est.estimate_batch(src, dst, off, dt=dt, params=_params(mc=True, **kw))
    _compare(got, mask, want, off, "MC on orora_pairs(777, 60)")


def _edge_batch():
    rng = np.random.default_rng(17)
    c, s = np.cos(0.05), np.sin(0.05)

    def rigid(k, outliers=0):
        p = rng.uniform(-80, 80, (k, 2))
        q = p @ np.array([[c, s], [-s, c]]) + [0.5, 0.25]
        q[:outliers] = rng.uniform(-80, 80, (outliers, 2))
        return p, q
    sets = [rigid(0), rigid(1), rigid(2), rigid(3), rigid(400, 400), rigid(500, 150), rigid(16384, 6000), rigid(16385), rigid(300)]
    p, q = rigid(8, 3)                         # duplicated points: every match twice (a sampled pair of twins is a singular MC system)
    sets.append((np.repeat(p, 2, axis=0), np.repeat(q, 2, axis=0)))
    p = np.tile(rng.uniform(-80, 80, (1, 2)), (5, 1))   # one source point, scattered destinations: no hypothesis has 2 inliers (rigid)
    sets.append((p, rng.uniform(-80, 80, (5, 2))))
    names = ["K=0", "K=1", "K=2", "K=3", "all outliers", "30 % outliers", "K=16384", "K=16385", "clean: stops at h=0", "duplicates", "one source point"]
    off = np.concatenate([[0], np.cumsum([len(a) for a, _ in sets])]).astype(np.int64)
    return (np.concatenate([a for a, _ in sets]).astype(np.float32), np.concatenate([b for _, b in sets]).astype(np.float32), off, names)


def test_edge_cases(est):
    src, dst, off, names = _edge_batch()
    rng = np.random.default_rng(3)
    dt = (0.25 * (1.0 + rng.integers(-3, 4, len(src)) / 400.0)).astype(np.float32)
    for mc in (False, True):
        want = rn.estimate_batch(src, dst, off, dt=dt if mc else None, mc=mc, debug=True)
        # 11 pairs: the 1 % rule leaves none out, so every named case is compared (smallest margin here: 1.5e-4 m)
        assert min(w.get("margin", np.inf) for w in want) > 1e-6
        got, mask = est.estimate_batch(src, dst, off, dt=dt if mc else None, params=_params(mc=mc))
        st = dict(zip(names, got["status"]))
        assert (st["K=0"], st["K=1"], st["K=2"], st["K=3"], st["K=16384"], st["K=16385"]) == (1, 1, 0, 0, 0, 2), st
        assert got["hypotheses"][names.index("clean: stops at h=0")] == 1 and got["hypotheses"][names.index("K=2")] == 1
        assert st["one source point"] == 4 and not mask[off[-2]:].any()
        for i in np.nonzero(got["status"] != 0)[0]:
            assert all(got[f][i] == 0 for f in FIELDS) and got["inliers"][i] == 0 and not mask[off[i]:off[i + 1]].any()
        if mc:   # duplicated matches sampled together: a singular 2-match system, a void hypothesis
            assert want[names.index("duplicates")]["void"].any() and want[names.index("one source point")]["void"].all()
        _compare(got, mask, want, off, f"edge cases, mc={mc}", max_left_out=0.0)
    # every dt equal to 0: no velocity is observable, every hypothesis is void -- under the restatement and on the device
    s0, d0, o0, z0 = src[off[5]:off[6]], dst[off[5]:off[6]], np.array([0, 500], dtype=np.int64), np.zeros(500, np.float32)
    want = rn.estimate_batch(s0, d0, o0, dt=z0, mc=True, debug=True)
    assert want[0]["void"].all() and (want[0]["status"], want[0]["hypotheses"]) == (4, 100)
    got, mask = est.estimate_batch(s0, d0, o0, dt=z0, params=_params(mc=True))
    _compare(got, mask, want, o0, "MC, every dt = 0", max_left_out=0.0)
    assert got["status"][0] == 4 and got["hypotheses"][0] == 100 and not mask.any()


def test_host_entry_device_entry_batch_position_and_two_streams(est):
    import torch
    from navtech_radar_slam_amd import _rsx
    src, dst, dt, off, _, _ = synth.motion_distorted_pairs(9, 12, k=700)
    for mc in (False, True):
        prm = _params(mc=mc, seed=4)
        host, hmask = est.estimate_batch(src, dst, off, dt=dt if mc else None, params=prm)
        # one pair alone, and the batch in another order
        for i in (0, 5, 11):
            one, m1 = est.estimate(src[off[i]:off[i + 1]], dst[off[i]:off[i + 1]], dt[off[i]:off[i + 1]] if mc else None, prm)
            assert one.tobytes() == host[i].tobytes() and np.array_equal(m1, hmask[off[i]:off[i + 1]])
        perm = np.random.default_rng(1).permutation(12)
        idx = np.concatenate([np.arange(off[i], off[i + 1]) for i in perm])
        shuf, _ = est.estimate_batch(src[idx], dst[idx], off, dt=dt[idx] if mc else None, params=prm)   # (every pair has 700 matches)
        assert shuf.tobytes() == host[perm].tobytes()
        # the device entry, on two streams of one handle at once
        d = [torch.from_numpy(a).cuda() for a in (src, dst, dt, off)]
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        outs = [torch.zeros(12 * _rsx.RANSAC_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda") for _ in streams]
        inls = [torch.zeros(len(src), dtype=torch.uint8, device="cuda") for _ in streams]
        torch.cuda.synchronize()
        for _ in range(3):
            for st, o, m in zip(streams, outs, inls):
                est.estimate_batch_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr() if mc else None, d[3].data_ptr(), 12, o.data_ptr(),
                                          m.data_ptr(), params=prm, stream=st.cuda_stream)
        torch.cuda.synchronize()
        for o, m in zip(outs, inls):
            assert o.cpu().numpy().tobytes() == host.tobytes() and np.array_equal(m.cpu().numpy().astype(bool), hmask)


def test_bad_arguments(est):
    from navtech_radar_slam_amd import _rsx
    src, dst, off, _ = synth.orora_pairs(1, 2, k_range=(10, 20))
    dt = np.full(len(src), 0.25, dtype=np.float32)
    for kw in (dict(tolerance=0.0), dict(tolerance=-1.0), dict(tolerance=float("nan")), dict(inlier_ratio=0.0), dict(inlier_ratio=1.01),
               dict(max_iterations=0), dict(max_iterations=1025), dict(flags=2)):
        with pytest.raises(_rsx.RsxError) as e:
            est.estimate_batch(src, dst, off, params=_params(**kw))
        assert e.value.status == -1, kw
    for kw in (dict(max_gn_iterations=0), dict(dt_scan=0.0), dict(gn_epsilon=-1.0)):
        with pytest.raises(_rsx.RsxError):
            est.estimate_batch(src, dst, off, dt=dt, params=_params(mc=True, **kw))
    with pytest.raises(_rsx.RsxError):
        est.estimate_batch(src, dst, off, params=_params(mc=True))          # motion compensated without dt
    for bad in ([0, 20, 10], [1, 5, 10], [0, -1, 10]):
        with pytest.raises(_rsx.RsxError):
            est.estimate_batch(src, dst, np.array(bad, dtype=np.int64))
    L = _rsx.lib()
    # offsets that decrease in the middle, or go negative: refused before anything is written
    s3, d3, o3, _ = synth.orora_pairs(12, 3, k_range=(40, 80))
    m = int(o3[-1])
    res, inl = np.full(3, 7, dtype=_rsx.RANSAC_RESULT_DTYPE), np.full(m, 0xA5, dtype=np.uint8)
    for bad in ([0, 60, 40, m], [0, -1, 40, m], [0, 40, 60, -1]):
        bad = np.array(bad, dtype=np.int64)
        assert L.rsx_ransac_estimate_batch(est._h, s3.ctypes.data, d3.ctypes.data, None, bad.ctypes.data, 3, None, res.ctypes.data, inl.ctypes.data) == -1
        assert b"offsets" in L.rsx_last_error_string(), bad
    assert (res.view(np.uint8) == np.full(3, 7, dtype=_rsx.RANSAC_RESULT_DTYPE).view(np.uint8)).all() and (inl == 0xA5).all()
    assert L.rsx_ransac_estimate_batch(est._h, s3.ctypes.data, d3.ctypes.data, None, o3.ctypes.data, 3, None, res.ctypes.data, inl.ctypes.data) == 0
    want, wmask = est.estimate_batch(s3, d3, o3)
    assert res.tobytes() == want.tobytes() and np.array_equal(inl.astype(bool), wmask.astype(bool)) and np.all(res["status"] == 0)
    assert L.rsx_ransac_estimate_batch(None, None, None, None, None, 1, None, None, None) == -1
    assert L.rsx_ransac_estimate_batch_device(None, None, None, None, None, 1, None, None, None, None) == -1
    assert L.rsx_ransac_default_params(None) == -1 and L.rsx_ransac_create(0, None) == -1
    h = C.c_void_p(1)
    assert L.rsx_ransac_create(10 ** 6, C.byref(h)) == -2 and not h.value
    got, mask = est.estimate_batch(src, dst, off)                            # the handle still works; ratio 1.0 is allowed
    assert np.all(got["status"] == 0)
    assert est.estimate_batch(src, dst, off, params=_params(inlier_ratio=1.0), want_mask=False)["hypotheses"].tolist() == [100, 100]


def test_lifecycle():
    """create / use / destroy cycles of the handle (tests/test_gpu_lifecycle.py covers the older ones)"""
    from navtech_radar_slam_amd import ransac
    src, dst, off, _ = synth.orora_pairs(2, 3, k_range=(50, 90))
    first = None
    for _ in range(20):
        r = ransac.Ransac()
        got, mask = r.estimate_batch(src, dst, off)
        first = got if first is None else first
        assert got.tobytes() == first.tobytes()
        r.close()
        r.close()
    assert ransac.Ransac()._L.rsx_ransac_destroy(None) == 0
