"""csrc/coral.hip (rsx_coral_*, rsx_kfstore_alignment_quality) against tests/coral_np.py, the arithmetic contract.

What is compared, and how closely.  The per-point records (two determinants, two counts) are compared BYTE FOR BYTE: the device
makes the same fp64 additions in the same order.  h_joint and h_separate are compared to 1e-9 absolute and quality to 2e-9: a term
is |0.5 log det| <= 7 for det in [1e-6, ~600] (plus the constant 2.84); a device logarithm is within a few ulp of the host's, i.e.
a few 1e-15 on a term; a sum of n terms taken in any order errs by at most about n * 2^-53 * sum|term|, so the mean errs by at most
about n * 2^-53 * mean|term| = 16384 * 1.1e-16 * 7 = 1.3e-11.  1e-9 leaves two orders of magnitude of margin; quality is the
difference of two such means, hence 2e-9.  The integer fields and the status are compared exactly."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coral_cases as cc  # noqa: E402
import coral_np as co  # noqa: E402

pytestmark = pytest.mark.gpu
R = 3.5
QUARTER = (0.0, -1.0, 2.0, 1.0, 0.0, -1.5)  # the exact quarter turn
GENERAL = co.pose_matrix((0.8, -0.35, 0.21))


@pytest.fixture(scope="module")
def handle():
    from navtech_radar_slam_amd import coral
    h = coral.Coral()
    yield h
    h.close()


def _want(jobs, **kw):
    return [co.quality(a, b, T, **kw) for a, b, T in jobs]


def _check(name, res, pts, want):
    wres, wpts = want
    err = [abs(float(res[f]) - float(wres[f])) for f in ("h_joint", "h_separate", "quality")]
    print(f"{name}: scored {int(res['n_scored'])} / valid {int(res['n_valid'])}, status {int(res['status'])}, |dh_joint| {err[0]:.3g}, "
          f"|dh_separate| {err[1]:.3g}, |dQ| {err[2]:.3g}")
    for f in ("n_scored", "n_scored_a", "n_valid", "status"):
        assert res[f] == wres[f], (name, f, res[f], wres[f])
    if pts is not None:
        assert len(pts) == len(wpts), name
        assert pts.tobytes() == wpts.tobytes(), (name, np.nonzero(pts.view(np.uint8).reshape(-1, 24) != wpts.view(np.uint8).reshape(-1, 24))[0][:5])
    assert err[0] <= 1e-9 and err[1] <= 1e-9 and err[2] <= 2e-9, (name, err)


def _run(handle, jobs, names, params=None, null_transforms=False, **kw):
    res, pts = handle.quality([j[0] for j in jobs], [j[1] for j in jobs],
                              transforms=None if null_transforms else [co.IDENTITY if j[2] is None else j[2] for j in jobs], params=params, points=True)
    for i, w in enumerate(_want(jobs, **kw)):
        _check(names[i], res[i], pts[i], w)
    return res, pts


def _lattice(n, step, x0=0.0, y0=0.0):
    return np.array([(x0 + step * i, y0 + step * j) for j in range(n) for i in range(n)], dtype=np.float32)


def _corners(seed):
    """points in the grid's edge cells (ix, iy in {-64, 63}): the 3 x 3 block is clipped on one or two sides"""
    rng = np.random.default_rng(seed)
    out = []
    for cx, cy in ((-64, -64), (63, 63), (-64, 63), (63, -64), (0, 63), (-64, 5)):
        out.append(np.stack([rng.uniform(cx * R + 0.01, cx * R + R - 0.01, 14), rng.uniform(cy * R + 0.01, cy * R + R - 0.01, 14)], axis=1))
        out.append(np.stack([rng.uniform(cx * R - R, cx * R + 2 * R, 10), rng.uniform(cy * R - R, cy * R + 2 * R, 10)], axis=1))  # some fall outside
    return np.concatenate(out).astype(np.float32)


JUNK = np.array([[np.nan, 1.0], [2.0, np.inf], [-np.inf, np.nan], [300.0, 0.0], [0.0, -300.0], [3e38, -3e38], [224.0, 0.0], [-224.5, 1.0]],
                dtype=np.float32)


def _crafted():
    rc = cc.random_cloud
    blob = np.array([(5.2 + 0.3 * (i % 3) + 0.01 * i, 8.1 + 0.25 * (i // 3)) for i in range(5)], dtype=np.float32)
    none = np.zeros((0, 2), dtype=np.float32)
    border = _lattice(9, 1.75, -7.0, -7.0)  # 1.75 = r / 2: every other point lies ON a cell border, negative multiples of r included
    return {
        "empty, empty": (none, none, None),
        "one point a side": (rc(1, 1), rc(2, 1), None),
        "A empty": (none, rc(3, 40, 6.0), None),
        "B empty": (rc(3, 40, 6.0), none, GENERAL),
        "5 + 5, below min_points": (blob, blob + np.float32(0.1), None),
        "1000 + 37": (rc(4, 1000, 30.0), rc(5, 37, 30.0), GENERAL),
        "cell borders": (border, border, (1.0, 0.0, 1.75, 0.0, 1.0, -3.5)),
        # the lattice is dyadic, so B = A + (3.5, 0) has pairs at distance EXACTLY r (d2 == r * r == 12.25 in fp64): neighbours
        "pairs exactly r apart": (_lattice(6, 0.5), _lattice(6, 0.5), (1.0, 0.0, 3.5, 0.0, 1.0, 0.0)),
        "grid edge cells": (_corners(6), _corners(7), None),
        "non-finite and outside, both sides": (np.concatenate([rc(8, 60, 8.0), JUNK, rc(9, 60, 8.0)]), np.concatenate([JUNK[::-1], rc(10, 90, 8.0)]), None),
        "non-finite transform": (rc(11, 80, 8.0), rc(12, 80, 8.0), (1.0, 0.0, np.nan, 0.0, 1.0, np.inf)),
        "identity": (rc(13, 300, 10.0), rc(14, 300, 10.0), co.IDENTITY),
        "quarter turn": (rc(13, 300, 10.0), rc(14, 300, 10.0), QUARTER),
        "general pose": (rc(13, 300, 10.0), rc(14, 300, 10.0), GENERAL),
        "far apart": (rc(15, 200, 8.0), rc(16, 200, 8.0), (1.0, 0.0, 120.0, 0.0, 1.0, 0.0)),
    }


def test_crafted_jobs_equal_the_restatement(handle):
    crafted = _crafted()
    names, jobs = list(crafted), list(crafted.values())
    res, pts = _run(handle, jobs, names)
    by = dict(zip(names, res))
    assert by["empty, empty"]["status"] == co.STATUS_EMPTY and by["5 + 5, below min_points"]["status"] == co.STATUS_EMPTY
    assert by["one point a side"]["n_valid"] == 2 and by["A empty"]["n_valid"] == 40
    assert by["1000 + 37"]["n_scored"] > 100 and by["grid edge cells"]["n_scored"] > 50 and by["grid edge cells"]["status"] == co.STATUS_RANGE
    assert by["non-finite and outside, both sides"]["status"] == co.STATUS_RANGE and by["non-finite and outside, both sides"]["n_valid"] == 210
    assert by["non-finite transform"]["status"] == co.STATUS_RANGE | co.STATUS_EMPTY and by["far apart"]["status"] == co.STATUS_EMPTY
    # a pair at distance exactly r counts: A's point (0, 0) sees its own lattice but for the far corner (2.5, 2.5), and of B only
    # (3.5, 0), which is exactly r away ((3.5, 0.5) is past r)
    k = names.index("pairs exactly r apart")
    assert pts[k]["m_separate"][0] == 35 and pts[k]["m_joint"][0] == 35 + 1
    # min_other = 0 scores the points without overlap; another radius moves every cell border (2.5: pairs (1.5, 2.0) apart are at r)
    from navtech_radar_slam_amd import coral
    _run(handle, [crafted["far apart"]], ["far apart, min_other 0"], params=coral.params(min_other=0), min_other=0)
    _, p25 = _run(handle, [(_lattice(6, 0.5), _lattice(6, 0.5), (1.0, 0.0, 1.5, 0.0, 1.0, 2.0))], ["radius 2.5, pairs exactly r apart"],
                  params=coral.params(radius=2.5, min_points=4, det_min=1e-3), radius=2.5, min_points=4, det_min=1e-3)
    assert p25[0]["m_joint"][0] > p25[0]["m_separate"][0]
    # transforms NULL is the identity
    same = [(a, b, None) for a, b, _ in jobs[:6]]
    r0, p0 = _run(handle, same, names[:6], null_transforms=True)
    r1, p1 = _run(handle, same, names[:6])
    assert r0.tobytes() == r1.tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(p0, p1))
    # poses are turned into matrices on the host
    pose = (0.8, -0.35, 0.21)
    rp = handle.quality([jobs[5][0]], [jobs[5][1]], poses=[pose])
    assert rp.tobytes() == res[5:6].tobytes()


def test_the_cap_and_one_below(handle):
    """8192 + 8192: the sort has no padding; 8191 + 8192: one padded key"""
    a, b = cc.random_cloud(20, 8192, 80.0), cc.random_cloud(21, 8192, 80.0)
    res, _ = _run(handle, [(a, b, GENERAL), (a[:8191], b, GENERAL)], ["8192 + 8192", "8191 + 8192"])
    assert res["n_valid"].tolist() == [16384, 16383] and (res["n_scored"] > 14000).all()


def test_one_crowded_cell(handle):
    """2048 + 2048 points in ONE cell: the longest walk (every point visits all 4096, twice)"""
    rng = np.random.default_rng(22)
    a = rng.uniform(0.05, 3.45, size=(2048, 2)).astype(np.float32)
    b = rng.uniform(0.05, 3.45, size=(2048, 2)).astype(np.float32)
    res, pts = _run(handle, [(a, b, None)], ["2048 + 2048 in one cell"])
    assert res["n_scored"][0] == 4096 and pts[0]["m_joint"].max() > 3000


@pytest.mark.parametrize("i, j", [(0, 1), (0, 3), (2, 7)])
def test_scan_pairs_equal_the_restatement_and_separate(handle, i, j):
    clouds, poses = cc.small_clouds()
    p = cc.true_pose(poses, i, j)
    shifts = ((0.0, 0.0, 0.0), (0.5, 0.0, 0.0), (3.0, 0.0, 0.0))
    res, pts = handle.quality([clouds[i]] * 3, [clouds[j]] * 3, transforms=[co.pose_matrix(p + np.array(s)) for s in shifts], points=True)
    for k, s in enumerate(shifts):
        _check(f"pair ({i}, {j}) + {s}", res[k], pts[k], cc.small_want(i, j, *s))
    assert res["quality"][0] < res["quality"][1] < res["quality"][2] and res["n_scored"][0] >= 0.99 * 1536


def test_a_job_does_not_depend_on_its_place(handle):
    rc = cc.random_cloud
    none = np.zeros((0, 2), dtype=np.float32)
    jobs = [(rc(30, 500, 12.0), rc(31, 450, 12.0), GENERAL), (rc(32, 64, 5.0), rc(33, 64, 5.0), QUARTER), (none, none, GENERAL), (none, rc(34, 30, 4.0), None),
            (rc(35, 900, 16.0), rc(36, 1100, 16.0), None), (none, none, None), (rc(37, 300, 9.0), rc(38, 7, 9.0), GENERAL)]
    T = [co.IDENTITY if t is None else t for _, _, t in jobs]
    res, pts = handle.quality([j[0] for j in jobs], [j[1] for j in jobs], transforms=T, points=True)
    res_only = handle.quality([j[0] for j in jobs], [j[1] for j in jobs], transforms=T)   # out_points NULL
    assert res_only.tobytes() == res.tobytes()
    for k, (a, b, _) in enumerate(jobs):
        r1, p1 = handle.quality([a], [b], transforms=[T[k]], points=True)
        assert r1.tobytes() == res[k:k + 1].tobytes() and p1[0].tobytes() == pts[k].tobytes(), k
        assert handle.quality([a], [b], transforms=[T[k]]).tobytes() == r1.tobytes(), k
    for k, w in enumerate(_want(jobs)):
        _check(f"job {k}", res[k], pts[k], w)


def test_device_entry_strides_streams_and_the_cap(handle):
    import torch
    from navtech_radar_slam_amd import _rsx
    from navtech_radar_slam_amd.cfear import ragged
    rc = cc.random_cloud
    A, B = [rc(40, 700, 14.0), rc(41, 0, 1.0), rc(42, 333, 9.0)], [rc(43, 650, 14.0), rc(44, 20, 3.0), rc(45, 400, 9.0)]
    T = np.array([GENERAL, co.IDENTITY, QUARTER], dtype=np.float64)
    want_res, want_pts = handle.quality(A, B, transforms=T, points=True)
    want_pts = np.concatenate(want_pts)
    a, a_off = ragged(A, np.float32, 2)
    b, b_off = ragged(B, np.float32, 2)
    a4, b4 = np.full((len(a), 4), 7.5, dtype=np.float32), np.full((len(b), 4), -3.25, dtype=np.float32)  # z and intensity are not read
    a4[:, :2], b4[:, :2] = a, b
    dev = {k: torch.from_numpy(v).cuda() for k, v in dict(a=a, b=b, a4=a4, b4=b4, a_off=a_off, b_off=b_off, T=T).items()}

    def outs():
        return torch.full((3 * 40,), 99, dtype=torch.uint8, device="cuda"), torch.full((len(want_pts) * 24,), 99, dtype=torch.uint8, device="cuda")

    # point_stride 4 on a float4 buffer == point_stride 2, on two streams of one handle with no synchronisation in between
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    results = [outs(), outs()]
    torch.cuda.synchronize()
    for s, (d_res, d_pts), (ka, kb, stride) in zip(streams, results, (("a", "b", 2), ("a4", "b4", 4))):
        handle.quality_device(dev[ka].data_ptr(), dev["a_off"].data_ptr(), dev[kb].data_ptr(), dev["b_off"].data_ptr(), 3, d_res.data_ptr(),
                              d_transforms=dev["T"].data_ptr(), d_points=d_pts.data_ptr(), point_stride=stride, stream=s.cuda_stream)
    torch.cuda.synchronize()
    for d_res, d_pts in results:
        assert d_res.cpu().numpy().tobytes() == want_res.tobytes() and d_pts.cpu().numpy().tobytes() == want_pts.tobytes()
    # d_transforms and d_points NULL, the handle's own stream
    d_res, _ = outs()
    torch.cuda.synchronize()
    handle.quality_device(dev["a"].data_ptr(), dev["a_off"].data_ptr(), dev["b"].data_ptr(), dev["b_off"].data_ptr(), 3, d_res.data_ptr())
    ident = handle.quality(A, B)   # (synchronises the handle's stream)
    assert d_res.cpu().numpy().tobytes() == ident.tobytes()
    # the device entry trusts its offsets: 8193 points on one side give STATUS_POINTS, a zero result and zero records; the host
    # entry refuses such a job
    big = rc(46, co.MAX_POINTS + 1, 50.0)
    for side in (0, 1):
        pair = [big, big[:100]] if side == 0 else [big[:100], big]
        d = [torch.from_numpy(c).cuda() for c in pair]
        offs = [torch.tensor([0, len(c)], dtype=torch.int64, device="cuda") for c in pair]
        d_res = torch.full((40,), 99, dtype=torch.uint8, device="cuda")
        d_pts = torch.full(((co.MAX_POINTS + 101) * 24,), 99, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        handle.quality_device(d[0].data_ptr(), offs[0].data_ptr(), d[1].data_ptr(), offs[1].data_ptr(), 1, d_res.data_ptr(), d_points=d_pts.data_ptr())
        handle.quality(A[:1], B[:1])
        got = d_res.cpu().numpy().view(_rsx.CORAL_RESULT_DTYPE)[0]
        wres, wpts = co.quality(pair[0], pair[1])
        assert got.tobytes() == wres.tobytes() and got["status"] == co.STATUS_POINTS
        assert not d_pts.cpu().numpy().any()
        with pytest.raises(_rsx.RsxError, match="more than 8192"):
            handle.quality([pair[0]], [pair[1]])


def test_keyframe_store_alignment_quality(handle):
    from navtech_radar_slam_amd import _rsx, coral, loopverify
    clouds, poses = cc.small_clouds()
    store = loopverify.KeyframeStore()
    try:
        rng = np.random.default_rng(50)
        for c in (clouds[0], clouds[3], np.zeros((0, 2), dtype=np.float32)):
            store.add(np.concatenate([c, rng.uniform(-1, 1, size=(len(c), 2)).astype(np.float32)], axis=1))   # z and intensity are not read
        T = co.pose_matrix(cc.true_pose(poses, 0, 3))
        for ia, ib, t, p in ((0, 1, T, None), (1, 0, None, None), (0, 0, None, coral.params(radius=2.0, min_points=4)), (0, 2, T, None), (2, 2, None, None)):
            got = store.alignment_quality(ia, ib, t, handle, params=p)
            want = handle.quality([store.get(ia)[:, :2]], [store.get(ib)[:, :2]], transforms=None if t is None else [t], params=p)
            assert got.tobytes() == want[0].tobytes(), (ia, ib)
        _check("keyframes 0 and 3", store.alignment_quality(0, 1, T, handle), None, cc.small_want(0, 3))
        for ia, ib in ((-1, 0), (0, 3), (3, 3), (0, -2)):
            with pytest.raises(_rsx.RsxError) as e:
                store.alignment_quality(ia, ib, None, handle)
            assert e.value.status == -1
    finally:
        store.close()


def test_bad_arguments(handle):
    from navtech_radar_slam_amd import _rsx
    from test_coral_abi import check_argument_rules
    check_argument_rules(_rsx, handle.handle)
    assert handle.quality([], []).shape == (0,)   # no job: nothing to do
