"""csrc/cfear_track.hip through the C-ABI (rsx_cfear_register_keyframes_batch, rsx_cfear_tracker_*) against its arithmetic
contract tests/cfear_track_np.py.

Status, iterations, correspondences, keyframe flags and ring sizes equal the restatement's; pose and cost within 1e-4 (the
project's pose tolerance: the kernel sums in another order and uses the device's sin / cos).  A case may be left out of that
comparison only when the restatement reports a decision margin below 1e-9, at most 1 % of a test's cases -- and the inputs are
chosen so that NONE is: every margin is asserted to be at least 1e-9 (tests/test_cfear_track_restatement.py asserts the same
without a GPU).  Where two GPU results are compared (K = 1 at the identity against rsx_cfear_register_batch, the cell index
against brute force, a batch against its parts, one push against several) the BYTES are equal.
PARITY UNPINNED w.r.t. CFEAR's own code, which is not in the reference checkout."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

from navtech_radar_slam_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cfear_np as cf  # noqa: E402
import cfear_track_cases as cases  # noqa: E402
import cfear_track_np as ct  # noqa: E402

pytestmark = pytest.mark.gpu
ID = (0.0, 0.0, 0.0)


@pytest.fixture(scope="module")
def handle():
    from navtech_radar_slam_amd import cfear
    h = cfear.Cfear()
    yield h
    h.close()


def _search(s):
    from navtech_radar_slam_amd import cfear
    return cfear.track_params(search=s)


def test_one_keyframe_at_the_identity_is_the_pair_kernel(handle):
    """2a: K = 1, pose (0, 0, 0), either search: the bytes of rsx_cfear_register_batch"""
    from navtech_radar_slam_amd import cfear
    for key, cs, init in cases.pair_groups():
        prm = cfear.params(**dict(key))
        pair = handle.register([c[1] for c in cs], [c[2] for c in cs], init, prm)
        assert [int(p["status"]) for p in pair] == [c[5] for c in cs]
        for s in (0, 1):
            got = handle.register_keyframes([c[1] for c in cs], [[c[2]] for c in cs], [[ID] for _ in cs], init, prm, _search(s))
            for c, g, p in zip(cs, got, pair):
                assert g.tobytes() == p.tobytes(), (c[0], s, g, p)
    # init = NULL is the identity
    c = cases.pair_cases()[0]
    assert handle.register_keyframes([c[1]], [[c[2]]], [[ID]]).tobytes() == handle.register([c[1]], [c[2]]).tobytes()


def _turned(rec, angle):
    out = rec.copy()
    c, s = math.cos(angle), math.sin(angle)
    nx, ny = rec["nx"].astype(np.float64), rec["ny"].astype(np.float64)
    out["nx"], out["ny"] = c * nx - s * ny, s * nx + c * ny
    return out


def _index_cases():
    """(name, src, keyframes, poses, init): what the cell index could get wrong and brute force cannot"""
    rng = np.random.default_rng(17)

    def cloud(n, lo, hi):
        a = np.zeros(n, dtype=cases.SP64)
        a["x"], a["y"] = rng.uniform(lo, hi, n), rng.uniform(lo, hi, n)
        th = rng.uniform(-math.pi, math.pi, n)
        a["nx"], a["ny"] = np.cos(th), np.sin(th)
        return cases.as_records(a)

    j = cases.joint_jobs()[1]
    # means exactly on cell edges (multiples of r = 3.5), and a second keyframe exactly r away from the first: d2 == r * r
    edge = np.zeros(13 * 13, dtype=cases.SP64)
    ii, jj = np.meshgrid(np.arange(-6, 7), np.arange(-6, 7))
    edge["x"], edge["y"] = 3.5 * ii.ravel(), 3.5 * jj.ravel()
    edge["nx"], edge["ny"] = np.cos(0.3 * (ii + 2 * jj).ravel()), np.sin(0.3 * (ii + 2 * jj).ravel())
    edge = cases.as_records(edge)
    shifted = edge.copy()
    shifted["x"] += np.float32(3.5)
    # +-224.5 m: outside the +-64 cells, binned into the border cells
    far = cloud(400, -2.0, 2.0)
    for q, (sx, sy) in enumerate(((1, 1), (-1, 1), (1, -1), (-1, -1))):
        far["x"][q::4] += np.float32(224.5 * sx)
        far["y"][q::4] += np.float32(224.5 * sy)
    # every record twice, the copies with another normal: the lower index must win the tie of the distances
    base = cloud(300, -40.0, 40.0)
    dup = np.concatenate([_turned(base, 0.1), base, _turned(base, -0.1)])[rng.permutation(900)]
    big = cloud(4096, -200.0, 200.0)
    crowd = cloud(4096, 0.0, 3.5)
    kp = (120.0, -80.0, 2.5)

    def view(pose):
        return cases.as_records(cases.seen_from(cases.room64(), pose))

    return (
        ("drive K = 3", j[1], j[2], j[3], j[4]),
        ("cell edges", edge, (edge, shifted), (ID, ID), ID),
        ("cell edges moved", edge, (edge, shifted), (ID, (0.0, 3.5, 0.0)), (0.05, -0.02, 0.01)),
        ("+-224.5 m", cf.transform(far, (0.1, -0.1, 0.0)), (far,), (ID,), ID),
        ("duplicates", cf.transform(base, (0.2, 0.1, 0.01)), (dup,), (ID,), ID),
        ("4096 records", cf.transform(big[::7], (0.3, -0.2, 0.001)), (big, big[:100]), (ID, ID), ID),
        ("4096 records in one cell", cf.transform(crowd[::9], (0.01, 0.02, 0.0)), (crowd,), (ID,), ID),
        ("keyframe pose (120, -80, 2.5)", view(ct.compose(kp, (0.5, 0.3, 0.04))), (view(kp), view(ct.compose(kp, (0.2, 0.1, 0.02)))),
         (kp, ct.compose(kp, (0.2, 0.1, 0.02))), ct.compose(kp, (0.2, 0.1, 0.02))),
    )


def test_cell_index_and_brute_force_give_the_same_bytes(handle):
    """2b"""
    ic = _index_cases()
    args = ([c[1] for c in ic], [list(c[2]) for c in ic], [list(c[3]) for c in ic], np.array([c[4] for c in ic]))
    cells, brute = (handle.register_keyframes(*args, track=_search(s)) for s in (0, 1))
    for c, a, b in zip(ic, cells, brute):
        print(f"{c[0]}: status {a['status']}, {a['iterations']} iterations, {a['correspondences']} correspondences")
        assert a.tobytes() == b.tobytes(), (c[0], a, b)
    by_name = {c[0]: a for c, a in zip(ic, cells)}
    # the cases do what they are there for: correspondences found at the grid's border, in the crowded cell, at the far pose
    assert by_name["+-224.5 m"]["correspondences"] == 400 and by_name["+-224.5 m"]["status"] in (0, 8)
    assert by_name["4096 records in one cell"]["correspondences"] > 400 and by_name["4096 records"]["correspondences"] > 500
    assert by_name["cell edges"]["correspondences"] >= 2 * 13 * 12
    far = by_name["keyframe pose (120, -80, 2.5)"]
    want = ct.compose((120.0, -80.0, 2.5), (0.5, 0.3, 0.04))
    assert far["status"] == 0 and max(abs(far["x"] - want[0]), abs(far["y"] - want[1]), abs(far["yaw"] - want[2])) < 1e-4
    # the duplicates: the restatement's brute-force rule (lowest index on a tie) decides the same
    d = ic[4]
    w = ct.register_keyframes(d[1], list(d[2]), list(d[3]), init=d[4])
    g = by_name["duplicates"]
    assert (g["status"], g["iterations"], g["correspondences"]) == (w["status"], w["iterations"], w["correspondences"])
    assert max(abs(g[f] - w[f]) for f in ("x", "y", "yaw", "cost")) < 1e-4


def _compare(name, got, want, left_out):
    d = max(abs(got["x"] - want["x"]), abs(got["y"] - want["y"]), abs(got["yaw"] - want["yaw"]), abs(got["cost"] - want["cost"]))
    print(f"{name}: status {got['status']}, {got['iterations']} iterations, {got['correspondences']} correspondences, "
          f"|GPU - restatement| {d:.2e}, margin {want['margin']:.1e}")
    if want["margin"] < 1e-9:
        left_out.append(name)
        return
    assert (got["status"], got["iterations"], got["correspondences"]) == (want["status"], want["iterations"], want["correspondences"]), (name, got, want)
    assert d < 1e-4, (name, got, want)


def _job_args(jobs):
    return [j[1] for j in jobs], [list(j[2]) for j in jobs], [list(j[3]) for j in jobs], np.array([j[4] for j in jobs])


def test_joint_jobs_equal_the_restatement(handle):
    """2c"""
    import torch
    from navtech_radar_slam_amd import _rsx, cfear
    jobs, wants = cases.joint_jobs(), cases.joint_wants()
    host = [j for j in jobs]
    batch = handle.register_keyframes(*_job_args(host))
    left_out = []
    for j, g, w in zip(jobs, batch, wants):
        assert w["status"] == j[5] and w["margin"] >= 1e-9, (j[0], w)  # the restatement alone leaves out none
        _compare(j[0], g, w, left_out)
        if j[5] in (1, 2, 4):
            assert (g["x"], g["y"], g["yaw"]) == tuple(j[4]), (j[0], g)  # the start pose
    assert len(left_out) <= len(jobs) // 100, left_out
    room = batch[2]
    assert max(abs(room[f] - w) for f, w in zip(("x", "y", "yaw"), cases.ROOM_POSES[2])) < 1e-4
    # a job's bytes do not depend on its place in the batch
    order = list(range(len(jobs)))[::-1]
    back = handle.register_keyframes(*_job_args([host[i] for i in order]))
    assert back[::-1].tobytes() == batch.tobytes()
    for i in (0, 2, len(jobs) - 1):
        assert handle.register_keyframes(*_job_args([host[i]])).tobytes() == batch[i:i + 1].tobytes()
    # two streams on one handle, no synchronisation in between: the batch's bytes
    src, kfs, poses, init = _job_args(host)
    s, so = cfear.ragged(src, _rsx.CFEAR_SURFACE_POINT_DTYPE)
    k, ko = cfear.ragged([a for job in kfs for a in job], _rsx.CFEAR_SURFACE_POINT_DTYPE)
    jo = np.zeros(len(jobs) + 1, dtype=np.int64)
    jo[1:] = np.cumsum([len(job) for job in kfs])
    kp = np.concatenate([np.asarray(p, dtype=np.float64).reshape(-1, 3) for p in poses])
    dev = [torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a).cuda() for a in (s, so, k, ko, jo, kp, init)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [torch.zeros(len(jobs) * 48, dtype=torch.uint8, device="cuda") for _ in streams]
    torch.cuda.synchronize()
    for st, o in zip(streams, outs):
        handle.register_keyframes_device(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), dev[4].data_ptr(),
                                         dev[5].data_ptr(), len(jobs), o.data_ptr(), d_init=dev[6].data_ptr(), stream=st.cuda_stream)
    torch.cuda.synchronize()
    for o in outs:
        assert o.cpu().numpy().tobytes() == batch.tobytes()
    # the device entry trusts its offsets: no keyframe -> status 1, more than 4 -> status 2, the start pose both times
    jo2 = torch.tensor([0, 0, 5], dtype=torch.int64, device="cuda")
    ko2 = torch.tensor([0, 1, 2, 3, 4, 5], dtype=torch.int64, device="cuda")
    so2 = torch.tensor([0, 3, 6], dtype=torch.int64, device="cuda")
    kp2 = torch.zeros(15, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    handle.register_keyframes_device(dev[0].data_ptr(), so2.data_ptr(), dev[2].data_ptr(), ko2.data_ptr(), jo2.data_ptr(), kp2.data_ptr(), 2,
                                     outs[0].data_ptr(), d_init=dev[6].data_ptr())
    handle.register([host[2][1]], [host[2][1]])  # (synchronises the handle's stream)
    got = outs[0].cpu().numpy()[:96].view(_rsx.CFEAR_RESULT_DTYPE)
    assert [int(g["status"]) for g in got] == [1, 2]
    assert all((g["x"], g["y"], g["yaw"]) == tuple(init[i]) for i, g in enumerate(got))


def _check_track(name, got, want, left_out):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        if w["margin"] < 1e-9:
            left_out.append((name, i))
            continue
        assert (g["keyframe"], g["n_keyframes"]) == (w["keyframe"], w["n_keyframes"]), (name, i, g, w)
        _compare(f"{name} scan {i}", g["reg"], w["reg"], left_out)
        assert max(abs(g[f] - w[f]) for f in ("x", "y", "yaw")) < 1e-4, (name, i, g, w)


def test_tracker_equals_the_restatement():
    """2d: the drive at the defaults, the small sequence with keyframe_distance 0.5 (the ring fills and evicts), the crafted motion
    with two keyframes, the re-anchored sequence; brute force gives the same bytes"""
    from navtech_radar_slam_amd import cfear
    recs, poses = cases.drive()
    far = cases.as_records(cases.seen_from(cases.room64(), (100.0, 0.0, 0.0)))
    anchor = cases.crafted_scans()[:3] + [far, far]
    runs = (("drive", recs, {}, cases.drive_track()), ("small", cases.small()[0], cases.SMALL_TRACK, cases.small_track()),
            ("one keyframe, thresholds 0", cases.small()[0], dict(n_keyframes=1, keyframe_distance=0.0, keyframe_rotation=0.0, predict=0),
             cases.small_pairs_track()),
            ("crafted", cases.crafted_scans(), dict(n_keyframes=2), ct.track(cases.crafted_scans(), n_keyframes=2)),
            ("re-anchor", anchor, {}, ct.track(anchor)))
    left_out, n = [], 0
    got = {}
    for name, scans, tp, want in runs:
        assert min(w["margin"] for w in want) >= 1e-9, name  # the restatement alone leaves out none
        t = cfear.Tracker(track=cfear.track_params(**tp))
        got[name] = t.push(scans)
        t.close()
        b = cfear.Tracker(track=cfear.track_params(search=1, **tp))
        assert b.push(scans).tobytes() == got[name].tobytes(), name
        b.close()
        _check_track(name, got[name], want, left_out)
        n += len(scans)
    assert len(left_out) <= n // 100, left_out
    d = got["drive"]
    assert list(d["keyframe"]) == [1, 0, 1, 0, 1, 0] and d["n_keyframes"][5] == 3 and not d["reg"]["status"].any()
    assert d["reg"]["correspondences"][5] == 1422 and d[0].tobytes() == bytes(48 + 24) + np.array([1, 0], dtype=np.int32).tobytes()
    for i in range(6):
        truth = synth.relative_pose(poses[0], poses[i])
        assert math.hypot(d["x"][i] - truth[0], d["y"][i] - truth[1]) <= 0.03, i
        if i:
            rel = ct.between(tuple(d[f][i - 1] for f in ("x", "y", "yaw")), tuple(d[f][i] for f in ("x", "y", "yaw")))
            t = synth.relative_pose(poses[i - 1], poses[i])
            et, ey = math.hypot(rel[0] - t[0], rel[1] - t[1]), abs(rel[2] - t[2])
            print(f"pair {i}: {et:.3f} m {ey:.1e} rad")
            assert et < 0.25 and ey < 1e-2
    assert list(got["small"]["keyframe"]) == [1, 0, 1, 0, 1, 1, 0, 1] and list(got["small"]["n_keyframes"]) == [0, 1, 1, 2, 2, 3, 3, 3]
    assert list(got["re-anchor"]["keyframe"]) == [1, 0, 0, 2, 0] and got["re-anchor"]["reg"]["status"][3] == 4
    assert list(got["crafted"]["keyframe"]) == list(cases.CRAFTED_FLAGS)


def test_pushes_sequences_and_reset():
    """2d: a sequence cut into pushes, two sequences in one handle, reset"""
    from navtech_radar_slam_amd import _rsx, cfear
    recs = cases.drive()[0]
    small, crafted = cases.small()[0], cases.crafted_scans()
    t = cfear.Tracker()
    whole = t.push(recs)
    t.reset()
    parts = np.concatenate([t.push(recs[:1]), t.push(recs[1:3]), t.push(recs[3:])])
    assert parts.tobytes() == whole.tobytes()
    assert len(t.push([])) == 0
    # reset restarts the sequence, and only reset lets the parameters change
    with pytest.raises(_rsx.RsxError, match="parameters differ"):
        t.track = cfear.track_params(n_keyframes=2)
        t.push(recs[:1])
    t.reset(track=cfear.track_params(**cases.SMALL_TRACK))
    alone = [t.push(small)]
    t.reset(track=cfear.track_params(**cases.SMALL_TRACK))
    alone.append(t.push(crafted))
    t.close()
    assert alone[0][0]["keyframe"] == 1 and alone[0][0]["n_keyframes"] == 0
    two = cfear.Tracker(2, track=cfear.track_params(**cases.SMALL_TRACK))
    both = two.push([small, crafted])
    assert both[0].tobytes() == alone[0].tobytes() and both[1].tobytes() == alone[1].tobytes()
    # ... and cut differently per sequence, one of them pausing
    two.reset(track=cfear.track_params(**cases.SMALL_TRACK))
    a = two.push([small[:3], crafted[:1]])
    b = two.push([[], crafted[1:5]])
    c = two.push([small[3:], crafted[5:]])
    assert np.concatenate([a[0], b[0], c[0]]).tobytes() == alone[0].tobytes()
    assert np.concatenate([a[1], b[1], c[1]]).tobytes() == alone[1].tobytes()
    two.close()


def test_bad_arguments(handle):
    """2e"""
    from navtech_radar_slam_amd import _rsx, cfear
    room = cases.as_records(cases.room64())
    t = cfear.Tracker()
    for bad, word in ((dict(n_keyframes=0), "n_keyframes"), (dict(n_keyframes=5), "n_keyframes"), (dict(keyframe_distance=-0.5), "keyframe_distance"),
                      (dict(keyframe_rotation=-0.1), "keyframe_rotation"), (dict(keyframe_distance=float("nan")), "keyframe_distance"),
                      (dict(search=2), "search"), (dict(predict=2), "predict")):
        with pytest.raises(_rsx.RsxError, match=word) as e:
            handle.register_keyframes([room], [[room]], [[ID]], track=cfear.track_params(**bad))
        assert e.value.status == -1
        t.track = cfear.track_params(**bad)
        with pytest.raises(_rsx.RsxError, match=word):
            t.push([room])
    tp = cfear.default_track_params()
    tp.reserved[1] = 7
    with pytest.raises(_rsx.RsxError, match="reserved"):
        handle.register_keyframes([room], [[room]], [[ID]], track=tp)
    t.track = tp
    with pytest.raises(_rsx.RsxError, match="reserved"):
        t.push([room])
    with pytest.raises(_rsx.RsxError, match="radius"):
        handle.register_keyframes([room], [[room]], [[ID]], params=cfear.params(radius=0.0))
    # more than 4 keyframes, or none, in a host job
    with pytest.raises(_rsx.RsxError, match="keyframes"):
        handle.register_keyframes([room], [[room] * 5], [[ID] * 5])
    with pytest.raises(_rsx.RsxError, match="keyframes"):
        handle.register_keyframes([room, room], [[room], []], [[ID], np.zeros((0, 3))])
    # offsets that do not start at 0 or decrease
    L = _rsx.lib()
    rec = np.zeros(8, dtype=_rsx.CFEAR_SURFACE_POINT_DTYPE)
    good, jobs, poses = np.array([0, 4, 8], dtype=np.int64), np.array([0, 1, 2], dtype=np.int64), np.zeros((2, 3))
    out = np.zeros(2, dtype=_rsx.CFEAR_RESULT_DTYPE)
    tout = np.zeros(2, dtype=_rsx.CFEAR_TRACK_RESULT_DTYPE)
    for off in ([0, 5, 3], [1, 2, 3]):
        o = np.array(off, dtype=np.int64)
        for so, ko, jo in ((o, good, jobs), (good, o, jobs), (good, good, o)):
            assert L.rsx_cfear_register_keyframes_batch(handle._h, rec.ctypes.data, so.ctypes.data, rec.ctypes.data, ko.ctypes.data, jo.ctypes.data,
                                                        poses.ctypes.data, 2, None, None, None, out.ctypes.data) == -1
            assert b"offsets" in L.rsx_last_error_string() or b"keyframes" in L.rsx_last_error_string()
        t.reset()
        assert L.rsx_cfear_tracker_push(t._h, rec.ctypes.data, o.ctypes.data, np.array([2], dtype=np.int32).ctypes.data, None, None, tout.ctypes.data) == -1
        assert b"offsets" in L.rsx_last_error_string()
    assert L.rsx_cfear_tracker_push(t._h, rec.ctypes.data, good.ctypes.data, np.array([-1], dtype=np.int32).ctypes.data, None, None, tout.ctypes.data) == -1
    h = ctypes.c_void_p()
    for n in (0, 4097):
        assert L.rsx_cfear_tracker_create(0, n, ctypes.byref(h)) == -1 and not h.value
    t.close()
