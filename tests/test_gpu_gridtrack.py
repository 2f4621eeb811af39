"""The grid-map tracker on the GPU (csrc/gridtrack.hip through navtech_radar_slam_amd.gridmap.GridTracker) against its restatement
(tests/gridtrack_np.py): every record byte for byte, no tolerance -- the glue is fp64 on plain operations in a stated order, the match is
integers, the refinement's sums have a stated order, so a difference is a bug."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gridmap_cases as gc  # noqa: E402
import gridmatch_cases as gxc  # noqa: E402
import gridmatch_np as gx  # noqa: E402
import gridrefine_cases as grc  # noqa: E402
import gridtrack_cases as gtc  # noqa: E402
import gridtrack_np as gt  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rsx():
    import __graft_entry__ as ge
    from navtech_radar_slam_amd import _rsx
    if not os.path.exists(_rsx.LIB_PATH):
        ge.build()
    return _rsx


def _map(p, L=None, rows=64, cols=96):
    from navtech_radar_slam_amd import gridmap
    m = gridmap.GridMap(rows, cols, gridmap.params(**p))
    if L is not None:
        m.set_likelihood(L)
    return m


def _tracker(m, poses):
    t = m.tracker(len(poses))
    t.reset(poses)
    return t


def _fields(tp):
    """the restatement's parameter dict as the keywords of gridmap.track_params"""
    return dict(tp["match"], **tp["refine"], min_score=tp["min_score"], predict=tp["predict"])


def _same(got, want, what=""):
    assert got.dtype.itemsize == want.dtype.itemsize == 344 and len(got) == len(want), (what, len(got), len(want))
    for i in range(len(got)):
        assert got[i].tobytes() == want[i].tobytes(), (what, "scan", i, got[i], want[i])


def _same_state(t, states):
    P, M, n = t.state()
    for q, st in enumerate(states):
        assert P[q].tobytes() == np.array(st.P).tobytes() and M[q].tobytes() == np.array(st.M).tobytes() and n[q] == st.n, ("state", q)


@pytest.mark.parametrize("width,height", gtc.SIZES)
def test_cloud_sizes(rsx, width, height):
    """a sequence of two scans for every N of 0, 1, 63, 64, 65, 255, 256, 257, 300, 8192 (the slot-part boundaries, the 256 partials of
    the refinement's sums, the cap), side by side, NaN and infinite points in every second scan"""
    L, seqs, poses, p = gtc.sizes_case(width, height)
    want = gtc.sizes_reference(width, height)
    assert (want["flags"] == 0).any() and (want["flags"] == gt.LOST).any() and (want["match"]["n_points"][1::2] < gtc.N_POINTS).any()
    m = _map(p, L)
    t = _tracker(m, poses)
    _same(t.push(seqs), want, (width, height))
    m.close()


@pytest.mark.parametrize("predict", [0, 1])
@pytest.mark.parametrize("K,U,V", gtc.WINDOWS)
def test_windows(rsx, K, U, V, predict):
    """no window at all, an uneven one, the default, and the largest, whose 4913 scores fill the volume (one scan of it with 8192 points);
    with and without the prediction"""
    L, seqs, poses, p = gtc.window_case(K)
    tp = gtc.window(K, U, V, predict=predict)
    want, states = gtc.reference(L, seqs, poses, p, tp)
    assert (want["flags"] == 0).any()
    m = _map(p, L)
    t = _tracker(m, poses)
    _same(t.push(seqs, **_fields(tp)), want, (K, U, V, predict))
    _same_state(t, states)
    m.close()


@pytest.mark.parametrize("width,height", gtc.SIZES)
def test_reset_poses(rsx, width, height):
    """a sequence from every pose of gxc.border_priors -- in the map, on every border, outside every border -- none exactly orthonormal:
    scan 0 starts from the reset pose bit for bit; outside, the scans are lost and dead-reckon"""
    L, seqs, poses, p = gtc.border_case(width, height)
    want = gtc.border_reference(width, height)
    per = gtc.split(want, seqs)
    assert all(w[0]["start"].tobytes() == poses[q].tobytes() for q, w in enumerate(per))
    assert (want["flags"] == gt.LOST).any() and (want["flags"] == 0).any() and (want["match"]["n_inside"] < want["match"]["n_points"]).any()
    m = _map(p, L)
    t = _tracker(m, poses)
    _same(t.push(seqs), want, (width, height))
    m.close()


def test_the_stand_alone_entries_chained_on_the_host(rsx):
    """GridMap.match, then GridMap.refine, with the glue in numpy: the host loop that the tracker replaces gives the tracker's bytes in
    match, refine, start and transform"""
    L, seqs, poses, p = gtc.window_case(2)
    tp = gt.params()
    m = _map(p, L)
    chained, _ = gtc.reference(L, seqs, poses, p, tp,
                               match_fn=lambda xy, prior: m.match([xy], np.array([prior]), **tp["match"])[0],
                               refine_fn=lambda xy, prior: m.refine([xy], np.array([prior]), **tp["refine"])[0])
    t = _tracker(m, poses)
    got = t.push(seqs)
    assert (got["flags"] == 0).any()
    for name in ("match", "refine", "start", "transform"):
        for i in range(len(got)):
            assert got[name][i].tobytes() == chained[name][i].tobytes(), (name, i)
    _same(got, chained, "chained")
    m.close()


@pytest.mark.parametrize("n_sequences", [1, 3, 70])
def test_sequences_and_cuts(rsx, n_sequences):
    """sequences of 0 .. 5 scans side by side, in one push, one scan per push, and cut after scan 0: the same bytes per sequence, which
    are those of the sequence alone in the restatement -- whatever its index and its neighbours (equal inputs sit at several indices)"""
    L, seqs, poses, p, ref = gtc.side_by_side(n_sequences)
    m = _map(p, L)
    longest = max(len(s) for s in seqs)
    for name, cuts in (("one push", [longest]), ("one scan per push", [1] * longest), ("after scan 0", [1, longest - 1])):
        t = _tracker(m, poses)
        got, at = [[] for _ in seqs], 0
        for n in cuts:
            part = [s[at:at + n] for s in seqs]
            for q, r in enumerate(gtc.split(t.push(part), part)):
                got[q].append(r)
            at += n
        for q in range(n_sequences):
            _same(np.concatenate(got[q]), ref[q], (name, "sequence", q))
        counts = t.state()[2]
        assert counts.tolist() == [len(s) for s in seqs]
        t.close()
    if n_sequences > gtc.N_DISTINCT:
        assert ref[0].tobytes() == ref[gtc.N_DISTINCT].tobytes() and len(ref[0]) > 0
    m.close()


def test_min_score_and_set_pose(rsx):
    """a scan of few points in mid-sequence scores below min_score: LOST, the sequence dead-reckons on; set_pose then starts it again
    (M the identity, n 0) and the scans after it are tracked as from a reset"""
    rng = np.random.default_rng(31)
    p = gc.small_params(64, 64)
    L = gxc.plane(32, p)
    pose = gtc.reset_poses(p)[:1]
    seq = gtc.sequence(rng, [300, 300, 20, 300], p, shrink=0.5)
    free = gtc.reference(L, [seq], pose, p, gt.params())[0]
    threshold = int(free["match"]["score"][2]) + 1
    assert threshold <= free["match"]["score"][[0, 1, 3]].min()
    tp = gt.params(min_score=threshold)
    states = gtc.states(pose)
    want = gt.push(L, [seq], states, p, tp)
    assert want["flags"].tolist()[:3] == [0, 0, gt.LOST] and want[2]["match"]["status"] == 0
    m = _map(p, L)
    t = _tracker(m, pose)
    _same(t.push([seq], **_fields(tp)), want, "min_score")
    _same_state(t, states)
    again = gtc.reset_poses(p)[1]
    t.set_pose(0, again)
    states[0] = gt.State(again)
    _same_state(t, states)
    more = gtc.sequence(rng, [300, 300], p, shrink=0.5)
    want = gt.push(L, [more], states, p, tp)
    assert want[0]["start"].tobytes() == again.tobytes()
    _same(t.push([more], **_fields(tp)), want, "after set_pose")
    _same_state(t, states)
    m.close()


def test_device_entry(rsx):
    """point_stride 4, a cloud whose base address is 4 modulo 16, n_scans in device memory: the host entry's bytes; a scan of 8193 points
    is LOST with POINTS (the host entry refuses it) and the sequences beside it are what they are without it"""
    import torch
    rng = np.random.default_rng(41)
    p = gc.small_params(192, 128)
    L = gxc.plane(42, p)
    poses = gtc.reset_poses(p)[[0, 1, 0]]
    seqs = [gtc.sequence(rng, [300, 257], p, shrink=0.5), [gxc.cloud(rng, 100, p), gxc.cloud(rng, gx.MAX_POINTS + 1, p), gxc.cloud(rng, 100, p)],
            gtc.sequence(rng, [65, 300, 64], p, shrink=0.5)]
    want, states = gtc.reference(L, seqs, poses, p, gt.params(), device_entry=True)
    per = gtc.split(want, seqs)
    assert per[1][1]["flags"] == gt.LOST and per[1][1]["match"]["status"] == gx.STATUS_POINTS and per[1][1]["match"]["score"] == 0
    alone = gtc.reference(L, [seqs[0], [], seqs[2]], poses, p, gt.params())[0]
    assert np.concatenate([per[0], per[2]]).tobytes() == alone.tobytes()
    m = _map(p, L)
    t = _tracker(m, poses)
    with pytest.raises(rsx.RsxError):
        t.push(seqs)
    _same_state(t, gtc.states(poses))                  # (the refused push changed nothing)
    xy, off = gxc.ragged([c for s in seqs for c in s])
    packed = rng.random((len(xy), 4)).astype(np.float32)          # z and w: anything
    packed[:, :2] = xy
    raw = torch.zeros(4 * len(xy) + 8, dtype=torch.float32, device="cuda")
    shift = (4 - (raw.data_ptr() % 16) // 4 + 1) % 4               # floats to skip for an address of 4 modulo 16
    d_xy = raw[shift:shift + 4 * len(xy)].view(len(xy), 4)
    d_xy.copy_(torch.from_numpy(packed))
    assert d_xy.data_ptr() % 16 == 4 and d_xy.stride(0) == 4
    d_off = torch.from_numpy(off).cuda()
    d_n = torch.tensor([len(s) for s in seqs], dtype=torch.int32, device="cuda")
    d_res = torch.full((len(want) * 344,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()      # (the buffers are filled before a stream of the handle's own choosing writes them)
    t.push_device(d_xy, d_off, d_n, d_res, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _same(d_res.cpu().numpy().view(gt.RESULT), want, "device")
    _same_state(t, states)
    m.close()


def test_a_changed_plane_is_seen_by_the_next_push(rsx):
    """a push reads the likelihood plane as it stands: after set_likelihood with another image, and after likelihood_field, the next push
    of the same tracker equals the restatement on the new plane"""
    rng = np.random.default_rng(51)
    p = gc.small_params(64, 64)
    L1, L2 = gxc.plane(52, p), gxc.plane(53, p)
    pose = gtc.reset_poses(p)[:1]
    parts = [gtc.sequence(rng, [300, 200], p, shrink=0.5) for _ in range(3)]
    m = _map(p, L1)
    t = _tracker(m, pose)
    states = gtc.states(pose)
    tp = gt.params()
    _same(t.push([parts[0]]), gt.push(L1, [parts[0]], states, p, tp), "first plane")
    m.set_likelihood(L2)
    on_the_old_plane = gt.push(L1, [parts[1]], [s.copy() for s in states], p, tp)
    want = gt.push(L2, [parts[1]], states, p, tp)
    assert want.tobytes() != on_the_old_plane.tobytes()
    _same(t.push([parts[1]]), want, "second plane")
    m.likelihood_field(threshold=200, radius=3)
    L3 = m.likelihood()
    assert L3.tobytes() != L2.tobytes()
    _same(t.push([parts[2]]), gt.push(L3, [parts[2]], states, p, tp), "field")
    _same_state(t, states)
    m.close()


def test_argument_rules_leave_the_state_alone(rsx):
    """each of: no likelihood yet, K = 9, U = 9, V = 9, a reserved word that is not 0, a predict that is neither 0 nor 1, a refinement
    parameter outside its rule, a non-finite reset pose, a sequence index out of range -- gives RSX_ERR_BAD_ARG, writes no record and
    leaves the state as it was"""
    from navtech_radar_slam_amd import gridmap
    rng = np.random.default_rng(61)
    p = gc.small_params(64, 64)
    L = gxc.plane(62, p)
    poses = gtc.reset_poses(p)[:2]
    seqs = [gtc.sequence(rng, [100], p, shrink=0.5) for _ in range(2)]
    m = _map(p)
    t = _tracker(m, poses)
    lib = rsx.lib()
    xy, off = gxc.ragged([c for s in seqs for c in s])
    n_scans = np.array([1, 1], dtype=np.int32)

    def refused(params):
        out = np.full(2, 0xAB, dtype=np.uint8).repeat(344)
        st = lib.rsx_gridmap_tracker_push(t.handle, xy.ctypes.data, off.ctypes.data, n_scans.ctypes.data, C.byref(params) if params is not None else None,
                                          out.ctypes.data)
        assert st == -1 and (out == 0xAB).all(), st
        _same_state(t, gtc.states(poses))

    refused(None)                                      # no likelihood yet
    assert b"likelihood" in lib.rsx_last_error_string()
    m.set_likelihood(L)
    bad = [gridmap.track_params(angle_steps=9), gridmap.track_params(x_cells=9), gridmap.track_params(y_cells=9), gridmap.track_params(predict=2),
           gridmap.track_params(max_evaluations=0), gridmap.track_params(damping=0.0)]
    for k in range(2):
        q = gridmap.default_track_params()
        q.reserved[k] = 1
        bad.append(q)
    q = gridmap.default_track_params()
    q.match.reserved = 1
    bad.append(q)
    q = gridmap.default_track_params()
    q.refine.reserved = 1
    bad.append(q)
    for q in bad:
        refused(q)
    for value in (np.nan, np.inf, -np.inf):
        for entry in (0, 2, 11):
            broken = poses.copy()
            broken.reshape(-1)[entry] = value
            with pytest.raises(rsx.RsxError):
                t.reset(broken)
            _same_state(t, gtc.states(poses))
            with pytest.raises(rsx.RsxError):
                t.set_pose(1, broken.reshape(-1)[entry - entry % 6:entry - entry % 6 + 6])
            _same_state(t, gtc.states(poses))
    for index in (-1, 2, 4096):
        with pytest.raises(rsx.RsxError):
            t.set_pose(index, poses[0])
        _same_state(t, gtc.states(poses))
    h = C.c_void_p(1)
    for n in (0, -1, 4097):
        assert lib.rsx_gridmap_tracker_create(m.handle, n, C.byref(h)) == -1 and not h.value
        h.value = 1
    # and the tracker still works
    _same(t.push(seqs), gtc.reference(L, seqs, poses, p, gt.params())[0], "after the refusals")
    m.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_the_drive(rsx, mode):
    """the drive of tests/test_gridtrack_restatement.py on the GPU, on the mean and on the hits: sixteen scans of 4800 points in one push,
    the bytes of the restatement, every scan within 0.05 m and 0.002 rad of the truth, none lost, the pose still a rotation"""
    imgs, T, p, clouds, poses = gtc.drive()
    want = gtc.drive_reference(mode)
    m = _map(p, rows=400, cols=3360)
    m.add(imgs[gtc.DRIVE_MAP_SCANS], T[gtc.DRIVE_MAP_SCANS])
    m.update_likelihood(mode)
    assert m.likelihood().tobytes() == gtc.drive_plane(mode).tobytes()
    t = _tracker(m, T[:1])
    got = t.push([clouds])
    _same(got, want, "drive")
    for i, r in enumerate(got):
        dist, dyaw = grc.pose_error(r["transform"], poses[i])
        assert dist < grc.E2E_LIMIT_M and dyaw < grc.E2E_LIMIT_RAD and r["flags"] == 0, (i, dist, dyaw)
    assert abs(gt.det(got[-1]["transform"]) - 1.0) < 1e-13
    m.close()
