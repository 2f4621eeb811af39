"""CFEAR motion compensation through the C-ABI (rsx_cfear_surface_points_timed_batch, rsx_cfear_compensate_batch,
rsx_cfear_tracker_push_timed and their device forms) against its arithmetic contract tests/cfear_mocomp_np.py.

Timed surface points: the records are the untimed entry's bytes, the times equal the restatement's bit for bit.  Compensation: bit
for bit (fp64 polynomials, nothing fused, one rounding to float).  Tracker: status, both iteration counts, correspondences,
keyframe flags and ring sizes equal the restatement's; pose and cost within 1e-4 (the project's pose tolerance, as in
tests/test_gpu_cfear_track.py: the kernel sums in another order and uses the device's sin / cos).  No case is left out for a small
decision margin: every margin of the restatement is asserted to be at least 1e-9.  Where two GPU results are compared (a sequence
cut into pushes, 16 sequences side by side, host against device entry, compensate = 0 against the untimed push) the BYTES are equal.
PARITY UNPINNED w.r.t. CFEAR's own code, which is not in the reference checkout."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cfear_mocomp_cases as mcases  # noqa: E402
import cfear_mocomp_np as cm  # noqa: E402
import cfear_np as cf  # noqa: E402
import cfear_track_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handle():
    from navtech_radar_slam_amd import cfear
    h = cfear.Cfear()
    yield h
    h.close()


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1) if a.dtype.fields else a).cuda()


def _same_f32(a, b):
    return np.asarray(a, dtype=np.float32).tobytes() == np.asarray(b, dtype=np.float32).tobytes()


def test_timed_surface_points(handle):
    import torch
    from navtech_radar_slam_amd import _rsx, cfear
    small = mcases.small_keypoints()[0]
    batches = (("small", [xy for xy, _ in small], [a for _, a in small], mcases.SMALL_ROWS),)
    for name, maker in (("seam, 401 rows", mcases.seam_cloud), ("16384 points in one cell", mcases.crowded_cloud)):
        xy, rows, n_rows = maker()
        batches += ((name, [xy], [rows], n_rows),)
    for name, clouds, rows, n_rows in batches:
        rec, tau, counts, status = handle.surface_points_timed(clouds, rows, n_rows)
        plain, pcounts, pstatus = handle.surface_points(clouds)
        assert np.array_equal(counts, pcounts) and np.array_equal(status, pstatus) and not status.any(), name
        for i, (xy, a) in enumerate(zip(clouds, rows)):
            want_rec, want_tau, _ = cm.surface_points_timed(xy, a, n_rows)
            assert rec[i].tobytes() == plain[i].tobytes() == want_rec.tobytes(), (name, i)
            assert _same_f32(tau[i], want_tau), (name, i, tau[i], want_tau)
        print(f"{name}: {[len(r) for r in rec]} records")
        # the device entry: the same bytes, slots past a scan's count untouched
        xy, off = cfear.ragged(clouds, np.float32, 2)
        a, _ = cfear.ragged(rows, np.int32)
        n, cap = len(clouds), 64 if name == "small" else 8
        d = [_dev(v) for v in (xy, a, off)]
        d_rec = torch.full((n * cap * 32,), 0xAB, dtype=torch.uint8, device="cuda")
        d_tau = torch.full((n * cap,), -1.0, dtype=torch.float32, device="cuda")
        d_cnt = torch.zeros(n, dtype=torch.int32, device="cuda")
        d_st = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        handle.surface_points_timed_device(d[0].data_ptr(), d[1].data_ptr(), n_rows, d[2].data_ptr(), n, d_rec.data_ptr(), d_tau.data_ptr(), cap,
                                           d_cnt.data_ptr(), d_st.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        g_rec = d_rec.cpu().numpy().view(_rsx.CFEAR_SURFACE_POINT_DTYPE).reshape(n, cap)
        g_tau = d_tau.cpu().numpy().reshape(n, cap)
        assert np.array_equal(d_cnt.cpu().numpy(), counts) and not d_st.cpu().numpy().any()
        for i in range(n):
            k = min(int(counts[i]), cap)
            assert g_rec[i, :k].tobytes() == rec[i][:k].tobytes() and _same_f32(g_tau[i, :k], tau[i][:k]), (name, i)
            assert (g_tau[i, k:] == -1.0).all() and (g_rec[i, k:].view(np.uint8) == 0xAB).all()
    # what the crafted clouds are there for
    rec, tau, _, _ = handle.surface_points_timed([mcases.seam_cloud()[0]], [mcases.seam_cloud()[1]], 401)
    seam = tau[0][rec[0]["x"] > 0]
    assert len(seam) == 2 and all(min(float(t), 1.0 - float(t)) <= 2.0 / 401 for t in seam)
    xy, rows, n_rows = mcases.crowded_cloud()
    rec, tau, _, _ = handle.surface_points_timed([xy], [rows], n_rows)
    assert len(rec[0]) == 1 and rec[0]["n_points"][0] > 8000
    # the host entry checks the rows and n_rows, as the untimed entry checks its arguments
    xy, rows, _ = mcases.seam_cloud()
    for bad_rows, n_rows, word in ((np.where(np.arange(len(rows)) == 5, 401, rows), 401, "rows"), (np.where(np.arange(len(rows)) == 0, -1, rows), 401, "rows"),
                                   (rows, 0, "n_rows"), (rows, 65537, "n_rows")):
        with pytest.raises(_rsx.RsxError, match=word) as e:
            handle.surface_points_timed([xy], [bad_rows.astype(np.int32)], n_rows)
        assert e.value.status == -1


def _compensate_batch():
    """257 scans: an empty one, one of 4096 records, the rest 0 .. 40; motions: zero, |yaw| = 0.5, just above it, NaN, infinite x among
    ordinary ones"""
    rng = np.random.default_rng(23)
    sizes = [int(v) for v in rng.integers(0, 41, 257)]
    sizes[0], sizes[3], sizes[200] = 7, 0, 4096
    recs, taus = [], []
    for n in sizes:
        r = np.zeros(n, dtype=cf.SP_DTYPE)
        r["x"], r["y"] = rng.uniform(-200, 200, n), rng.uniform(-200, 200, n)
        th = rng.uniform(-np.pi, np.pi, n)
        r["nx"], r["ny"] = np.cos(th), np.sin(th)
        r["lambda_max"], r["lambda_min"] = rng.uniform(0.1, 9, n), rng.uniform(0.001, 0.1, n)
        r["n_points"], r["cell"] = rng.integers(6, 99, n), rng.integers(0, 16384, n)
        recs.append(r)
        taus.append(rng.uniform(0.0, 1.0, n).astype(np.float32))
    recs[0]["x"][0], recs[0]["y"][1], taus[0][2], taus[0][3] = -0.0, -0.0, 0.0, 1.0
    motions = np.stack([rng.uniform(-3, 3, 257), rng.uniform(-1, 1, 257), rng.uniform(-0.5, 0.5, 257)], axis=1)
    motions[0] = 0.0
    motions[1] = (1.0, 0.2, 0.5)
    motions[2] = (1.0, 0.2, -0.5)
    motions[4] = (1.0, 0.2, np.nextafter(0.5, 1.0))
    motions[5] = (1.0, 0.2, -0.50001)
    motions[6] = (np.nan, 0.0, 0.0)
    motions[7] = (0.0, 0.0, np.nan)
    motions[8] = (np.inf, 0.0, 0.1)
    motions[9] = (0.0, 0.0, 0.3)
    motions[200] = (2.5, -0.4, 0.21)
    return recs, taus, motions


def test_compensate(handle):
    import torch
    from navtech_radar_slam_amd import _rsx, cfear
    recs, taus, motions = _compensate_batch()
    flat, off = cfear.ragged(recs, _rsx.CFEAR_SURFACE_POINT_DTYPE)
    tau = np.concatenate(taus)
    want, want_status = cm.compensate_batch(flat, tau, off, motions)
    got, status = handle.compensate(recs, taus, motions)
    assert np.array_equal(status, want_status)
    assert list(status[:10]) == [0, 0, 0, 0, 1, 1, 1, 1, 1, 0]
    for i in range(257):
        assert got[i].tobytes() == want[off[i]:off[i + 1]].tobytes(), (i, motions[i])
        if status[i] or i == 0:
            assert got[i].tobytes() == recs[i].tobytes(), i  # zero motion, or no velocity: the input's bytes
    assert got[200].tobytes() != recs[200].tobytes() and len(got[200]) == 4096
    # the device entry, in place, without a status array and with one
    d = [_dev(v) for v in (flat, tau, off, motions)]
    d_st = torch.full((257,), 7, dtype=torch.int32, device="cuda")
    out = torch.zeros_like(d[0])
    torch.cuda.synchronize()
    s = torch.cuda.current_stream().cuda_stream
    handle.compensate_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), 257, d[3].data_ptr(), out.data_ptr(), d_st.data_ptr(), stream=s)
    handle.compensate_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), 257, d[3].data_ptr(), d[0].data_ptr(), stream=s)
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == want.tobytes() and d[0].cpu().numpy().tobytes() == want.tobytes()
    assert np.array_equal(d_st.cpu().numpy(), want_status)
    assert len(handle.compensate([], [], np.zeros((0, 3)))[0]) == 0


def _check(name, got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        r, v = g["reg"], w["reg"]
        d = max(abs(g["x"] - w["x"]), abs(g["y"] - w["y"]), abs(g["yaw"] - w["yaw"]), abs(r["x"] - v["x"]), abs(r["y"] - v["y"]),
                abs(r["yaw"] - v["yaw"]), abs(r["cost"] - v["cost"]))
        print(f"{name} scan {i}: status {r['status']}, iterations {r['reserved']} + {r['iterations']}, {r['correspondences']} correspondences, "
              f"flag {g['keyframe']}, ring {g['n_keyframes']}, |GPU - restatement| {d:.2e}, margin {w['margin']:.1e}")
        assert w["margin"] >= 1e-9, (name, i, w["margin"])  # the restatement leaves out none
        assert (g["keyframe"], g["n_keyframes"]) == (w["keyframe"], w["n_keyframes"]), (name, i, g, w)
        assert (r["status"], r["iterations"], r["reserved"], r["correspondences"]) == (v["status"], v["iterations"], v["reserved"], v["correspondences"]), (name, i, g, w)
        assert d < 1e-4, (name, i, g, w)


def _tracker(n=1, **tp):
    from navtech_radar_slam_amd import cfear
    prm = cfear.params(min_correspondences=tp.pop("min_correspondences")) if "min_correspondences" in tp else None
    return cfear.Tracker(n, params=prm, track=cfear.track_params(compensate=1, **tp))


def _push_device(t, scans, taus):
    """one sequence through rsx_cfear_tracker_push_timed_device"""
    import torch
    from navtech_radar_slam_amd import _rsx, cfear
    rec, off = cfear.ragged(scans, _rsx.CFEAR_SURFACE_POINT_DTYPE)
    d = [_dev(v) for v in (rec, np.concatenate(taus), off, np.array([len(scans)], dtype=np.int32))]
    out = torch.zeros(len(scans) * 80, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    t.push_timed_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(_rsx.CFEAR_TRACK_RESULT_DTYPE)


@pytest.mark.parametrize("name", list(mcases.DRIVES))
def test_tracker_equals_the_restatement_on_the_room_drives(name):
    scans, taus, _ = mcases.drive(name)
    want = mcases.drive_track(name)
    t = _tracker()
    whole = t.push_timed(scans, taus)
    _check(name, whole, want)
    drive = mcases.DRIVES[name]
    e_on, e_off = cm.end_error(whole, drive), cm.end_error(mcases.drive_track(name, compensate=0), drive)
    print(f"{name}: end of trajectory {e_on:.4f} m with compensation, {e_off:.4f} m without")
    assert e_on < e_off
    # the device form, the brute-force search, and the sequence cut after scan 0, after scan 1 and in the middle: the same bytes
    t.reset(track=t.track)
    assert _push_device(t, scans, taus).tobytes() == whole.tobytes()
    for cuts in ((1,), (2,), (1, 2, 5), (5,)):
        t.reset(track=t.track)
        edges = (0,) + cuts + (len(scans),)
        parts = [t.push_timed(scans[a:b], taus[a:b]) for a, b in zip(edges, edges[1:])]
        assert np.concatenate(parts).tobytes() == whole.tobytes(), cuts
    t.close()
    b = _tracker(search=1)
    assert b.push_timed(scans, taus).tobytes() == whole.tobytes()
    b.close()


def test_sixteen_sequences_at_once():
    from navtech_radar_slam_amd import cfear
    seqs = [mcases.drive("constant"), mcases.drive("accelerating"), mcases.pass2_failure()[:2], (mcases.small_timed())]
    alone = []
    for scans, taus in ((s[0], s[1]) for s in seqs):
        t = _tracker()
        alone.append(t.push_timed(list(scans), list(taus)))
        t.close()
    many = _tracker(16)
    got = many.push_timed([list(seqs[q % 4][0]) for q in range(16)], [list(seqs[q % 4][1]) for q in range(16)])
    for q in range(16):
        assert got[q].tobytes() == alone[q % 4].tobytes(), q
    # ... and cut differently per sequence, the cut between scan 0 and scan 1 included, one sequence pausing
    many.reset(track=many.track)
    cut = [1 + q % 3 for q in range(16)]
    a = many.push_timed([list(seqs[q % 4][0][:cut[q]]) for q in range(16)], [list(seqs[q % 4][1][:cut[q]]) for q in range(16)])
    b = many.push_timed([[] if q == 5 else list(seqs[q % 4][0][cut[q]:]) for q in range(16)], [[] if q == 5 else list(seqs[q % 4][1][cut[q]:]) for q in range(16)])
    c = many.push_timed([list(seqs[1][0][cut[5]:]) if q == 5 else [] for q in range(16)], [list(seqs[1][1][cut[5]:]) if q == 5 else [] for q in range(16)])
    for q in range(16):
        assert np.concatenate([a[q], b[q], c[q]]).tobytes() == alone[q % 4].tobytes(), q
    many.close()


def test_pass_failures_equal_the_restatement():
    scans, taus, _ = mcases.drive("constant")
    far = cases.as_records(cases.seen_from(cases.room64(), (100.0, 0.0, 0.0)))
    ftau = np.full(len(far), 0.5, dtype=np.float32)
    over = np.zeros(cf.MAX_SURFACE_POINTS + 1, dtype=cf.SP_DTYPE)
    over["nx"] = 1.0
    otau = np.zeros(len(over), dtype=np.float32)
    # pass 1 fails (status 4: re-anchored with the compensated scan; status 2 and 1: nothing to re-anchor with), then goes on
    seq = (list(scans[:3]) + [far, far, over, far[:0]], list(taus[:3]) + [ftau, ftau, otau, ftau[:0]])
    want = cm.track(*seq)
    assert [w["reg"]["status"] for w in want] == [0, 0, 0, 4, 0, 2, 1] and [w["keyframe"] for w in want] == [1, 0, 1, 2, 0, 0, 0]
    t = _tracker()
    got = t.push_timed(*seq)
    _check("pass 1 fails", got, want)
    t.reset(track=t.track)
    assert np.concatenate([t.push_timed(seq[0][:4], seq[1][:4]), t.push_timed(seq[0][4:], seq[1][4:])]).tobytes() == got.tobytes()
    t.close()
    # pass 1 fails on scan 1: `first` is cleared, the first scan is never compensated
    want = cm.track([scans[0], far, far], [taus[0], ftau, ftau])
    assert [w["reg"]["status"] for w in want] == [0, 4, 0]
    t = _tracker()
    _check("pass 1 fails on scan 1", t.push_timed([scans[0], far, far], [taus[0], ftau, ftau]), want)
    t.close()
    # only pass 2 fails (scan 1); the same records once more register against the ring that scan 1 re-anchored
    s2, t2, mcorr = mcases.pass2_failure()
    s2, t2 = list(s2) + [s2[1]], list(t2) + [t2[1]]
    want = cm.track(s2, t2, min_correspondences=mcorr)
    assert [w["reg"]["status"] for w in want] == [0, 4, 0] and want[2]["reg"]["correspondences"] == 63
    assert want[1]["reg"]["status"] == 4 and want[1]["reg"]["reserved"] >= 1 and want[1]["keyframe"] == 2 and want[1]["reg"]["correspondences"] == 54
    t = _tracker(min_correspondences=mcorr)
    got = t.push_timed(s2, t2)
    _check("only pass 2 fails", got, want)
    for cut in (1, 2):
        t.reset(params=t.params, track=t.track)
        assert np.concatenate([t.push_timed(s2[:cut], t2[:cut]), t.push_timed(s2[cut:], t2[cut:])]).tobytes() == got.tobytes(), cut
    t.close()


def test_compensate_0_is_the_untimed_push_and_the_refusals():
    from navtech_radar_slam_amd import _rsx, cfear
    scans, taus, _ = mcases.drive("accelerating")
    t = cfear.Tracker()
    plain = t.push(scans)
    t.reset()
    assert t.push_timed(scans, taus).tobytes() == plain.tobytes()
    t.reset()
    assert np.concatenate([t.push_timed(scans[:1], taus[:1]), t.push(scans[1:4]), t.push_timed(scans[4:], taus[4:])]).tobytes() == plain.tobytes()
    t.reset()
    assert _push_device(t, scans, taus).tobytes() == plain.tobytes()
    assert cfear.default_track_params().compensate == 0
    # the untimed pushes refuse compensate = 1; compensate = 2 and the reserved words are refused everywhere
    t.reset(track=cfear.track_params(compensate=1))
    with pytest.raises(_rsx.RsxError, match="compensate") as e:
        t.push(scans[:1])
    assert e.value.status == -1
    out = np.zeros(1, dtype=_rsx.CFEAR_TRACK_RESULT_DTYPE)
    rec1, off1 = cfear.ragged(scans[:1], _rsx.CFEAR_SURFACE_POINT_DTYPE)
    d = [_dev(v) for v in (rec1, off1, np.array([1], dtype=np.int32), out)]
    with pytest.raises(_rsx.RsxError, match="compensate"):
        t.push_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr())
    assert len(t.push_timed(scans[:1], taus[:1])) == 1  # (the refusals left the sequence untouched)
    for bad in (2, -1):
        t.reset(track=cfear.track_params(compensate=bad))
        for push in (lambda: t.push(scans[:1]), lambda: t.push_timed(scans[:1], taus[:1])):
            with pytest.raises(_rsx.RsxError, match="compensate"):
                push()
    tp = cfear.track_params(compensate=1)
    tp.reserved[1] = 7
    t.reset(track=tp)
    with pytest.raises(_rsx.RsxError, match="reserved"):
        t.push_timed(scans[:1], taus[:1])
    assert ctypes.sizeof(_rsx.CfearTrackParams) == 40 and _rsx.CfearTrackParams.compensate.offset == 36
    L = _rsx.lib()
    rec, off = cfear.ragged(scans[:1], _rsx.CFEAR_SURFACE_POINT_DTYPE)
    assert L.rsx_cfear_tracker_push_timed(t._h, rec.ctypes.data, None, off.ctypes.data, np.array([1], dtype=np.int32).ctypes.data, None, None,
                                          out.ctypes.data) == -1
    t.close()
