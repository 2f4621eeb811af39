"""csrc/cfear.hip through the C-ABI (rsx_cfear_*) against its arithmetic contract tests/cfear_np.py.

Surface points: the records, counts and status words equal the restatement's BYTE FOR BYTE (fp64 IEEE arithmetic in a fixed
order on both sides).  Registration: status, iterations and correspondences equal, pose and cost within 1e-4 (the project's
pose tolerance; the kernel sums in another order and uses the device's sin / cos).  A pair may be left out of that comparison
only when the restatement reports a decision margin below 1e-9, at most 1 % of a test's pairs -- and the inputs here are chosen so
that NONE is: every margin is asserted to be at least 1e-9.
PARITY UNPINNED w.r.t. CFEAR's own code, which is not in the reference checkout."""
import math
import os
import sys

import numpy as np
import pytest

from navtech_radar_slam_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cfear_np as cf  # noqa: E402
import kstrongest_np as ksn  # noqa: E402

pytestmark = pytest.mark.gpu
F32_NEXT = float(np.nextafter(np.float32(5.0), np.float32(6.0)))


def _blob(n, x0=5.2, y0=8.1):
    return [(x0 + 0.3 * (i % 3) + 0.01 * i, y0 + 0.25 * (i // 3)) for i in range(n)]


def _crafted():
    rng = np.random.default_rng(5)
    square = [(1.0, 1.0), (2.0, 1.0), (1.0, 2.0), (2.0, 2.0)]  # centroid (1.5, 1.5), exact
    lattice = [(-7.0 + 0.875 * i, -7.0 + 0.4375 * j) for j in range(33) for i in range(17)]  # 0.875 = r / 4: points ON the cell edges
    clouds = {
        "empty": [],
        "one point": [(1.0, 2.0)],
        "min_points - 1": _blob(5),
        "min_points": _blob(6),
        # the 5th and 6th neighbour at distance exactly r = 3.5 from the centroid (12.25 == r * r): a record iff both are included
        "exactly r": square + [(5.0, 1.5), (1.5, -2.0)],
        "just past r": square + [(F32_NEXT, 1.5), (1.5, -2.0)],
        "cell edges": lattice,
        "isotropic": [(-3.5 + 0.875 * i, -3.5 + 0.875 * j) for j in range(9) for i in range(9)],
        "outside and NaN": _blob(6) + [(300.0, 0.0), (np.nan, 1.0), (0.0, -np.inf), (224.0, 0.0), (-224.0, 0.5), (3e38, -3e38)],
        "grid corners": _blob(6, -224.0, -224.0) + _blob(6, 222.0, 222.0),
        "collinear": [(0.25 * i, 2.0) for i in range(8)] + [(40.0 + 0.125 * i, 40.0 + 0.125 * i) for i in range(8)],
        "duplicates": _blob(6) * 2 + [(-20.5, 1.5)] * 8,
        "same neighbour set": [(3.4, 1.0), (3.45, 1.2), (3.3, 1.4), (3.6, 1.1), (3.55, 1.3), (3.7, 1.5)],
        "crowded block": rng.uniform(-3.5, 7.0, size=(900, 2)).tolist(),
    }
    return {k: np.array(v, dtype=np.float32).reshape(-1, 2) for k, v in clouds.items()}


@pytest.fixture(scope="module")
def handle():
    from navtech_radar_slam_amd import cfear
    h = cfear.Cfear()
    yield h
    h.close()


def _equal(got, count, status, want, want_status, name):
    assert count == len(want) and status == want_status, (name, count, len(want), status, want_status)
    assert got.tobytes() == want.tobytes(), name


def test_crafted_clouds_equal_the_restatement(handle):
    clouds = _crafted()
    want = {k: cf.surface_points(v) for k, v in clouds.items()}
    # what the cases are there for, in the restatement itself
    assert len(want["min_points - 1"][0]) == 0 and len(want["min_points"][0]) == 1
    assert [int(n) for n in want["exactly r"][0]["n_points"]] == [6] and len(want["just past r"][0]) == 0
    assert want["outside and NaN"][1] == cf.STATUS_RANGE and len(want["outside and NaN"][0]) == 1
    assert len(want["grid corners"][0]) >= 2 and want["grid corners"][1] == 0
    assert len(want["collinear"][0]) == 0
    same = want["same neighbour set"][0]
    assert len(same) == 2 and same[0]["cell"] != same[1]["cell"] and same[["x", "y", "nx", "ny"]][0] == same[["x", "y", "nx", "ny"]][1]
    assert int(want["crowded block"][0]["n_points"].max()) > 256
    names = list(clouds)
    recs, counts, status = handle.surface_points([clouds[k] for k in names])
    for i, k in enumerate(names):
        _equal(recs[i], counts[i], status[i], want[k][0], want[k][1], k)
    # other parameters: a smaller radius (more cells), another threshold
    from navtech_radar_slam_amd import cfear
    recs, counts, status = handle.surface_points([clouds["crowded block"], clouds["cell edges"]], cfear.params(radius=0.875, min_points=3, max_condition=50.0))
    for got, c, s, k in zip(recs, counts, status, ("crowded block", "cell edges")):
        w = cf.surface_points(clouds[k], radius=0.875, min_points=3, max_condition=50.0)
        _equal(got, c, s, w[0], w[1], k)


@pytest.fixture(scope="module")
def small(oracle):
    imgs, az, _, _ = synth.polar_sequence(3, 2, rows=64, cols=512, n_buildings=120, n_poles=200, world_radius=40.0)
    return [ksn.to_cartesian(ksn.extract(imgs[i], k=12, z_min=60, min_separation=0), az[i] if np.ndim(az) == 2 else az, synth.RADAR_RESOLUTION)
            for i in range(2)]


@pytest.fixture(scope="module")
def drive(oracle):
    """the four scans of the synthetic drive: k-strongest clouds, the restatement's surface points, the true poses"""
    imgs, az, poses, _ = synth.polar_sequence(11, 4)
    xy = [ksn.to_cartesian(ksn.extract(imgs[i], k=12, z_min=60, min_separation=0), az[i] if np.ndim(az) == 2 else az, synth.RADAR_RESOLUTION)
          for i in range(4)]
    return xy, [cf.surface_points(c) for c in xy], poses


def test_kstrongest_clouds_equal_the_restatement(handle, small, drive):
    clouds = small + [drive[0][0]]
    assert [len(c) for c in clouds] == [768, 768, 4800]
    recs, counts, status = handle.surface_points(clouds)
    want = [cf.surface_points(c) for c in small] + [drive[1][0]]
    print("records:", [len(w[0]) for w in want])
    assert len(want[0][0]) > 10 and len(want[2][0]) > 500
    for i in range(3):
        _equal(recs[i], counts[i], status[i], want[i][0], want[i][1], i)
    # truncation: the count reports every record, the first max_records are written
    recs, counts, _ = handle.surface_points(clouds, max_records=100)
    assert list(counts) == [len(w[0]) for w in want]
    assert recs[2].tobytes() == want[2][0][:100].tobytes() and recs[0].tobytes() == want[0][0][:100].tobytes()


def test_ragged_batch_entries_and_streams_agree(handle, small, drive):
    import torch
    from navtech_radar_slam_amd import _rsx, cfear
    clouds = [small[0][:0], small[0][:5], small[0], drive[0][0], small[1][:1]]
    assert [len(c) for c in clouds] == [0, 5, 768, 4800, 1]
    M = 1024
    batch = handle.surface_points(clouds, max_records=M, raw=True)
    for i, c in enumerate(clouds):
        alone = handle.surface_points([c], max_records=M, raw=True)
        assert alone[0][0].tobytes() == batch[0][i].tobytes() and alone[1][0] == batch[1][i] and alone[2][0] == batch[2][i], i
    xy, off = cfear.ragged(clouds, np.float32, 2)
    d_xy, d_off = torch.from_numpy(xy).cuda(), torch.from_numpy(off).cuda()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [(torch.zeros(len(clouds) * M * 32, dtype=torch.uint8, device="cuda"), torch.full((len(clouds),), 99, dtype=torch.int32, device="cuda"),
             torch.full((len(clouds),), 99, dtype=torch.int32, device="cuda")) for _ in streams]
    torch.cuda.synchronize()
    for s, (d_rec, d_cnt, d_st) in zip(streams, outs):  # two streams on one handle, no synchronisation in between
        handle.surface_points_device(d_xy.data_ptr(), d_off.data_ptr(), len(clouds), d_rec.data_ptr(), M, d_cnt.data_ptr(), d_st.data_ptr(),
                                     stream=s.cuda_stream)
    torch.cuda.synchronize()
    for d_rec, d_cnt, d_st in outs:
        assert d_rec.cpu().numpy().tobytes() == batch[0].tobytes()
        assert np.array_equal(d_cnt.cpu().numpy(), batch[1]) and np.array_equal(d_st.cpu().numpy(), batch[2])
    # the device entry trusts its offsets: a scan above the cap gets the status bit and no record, the host entry refuses it
    big = np.zeros((cf.MAX_POINTS + 1, 2), dtype=np.float32)
    d_big, d_boff = torch.from_numpy(big).cuda(), torch.tensor([0, len(big)], dtype=torch.int64, device="cuda")
    d_rec, d_cnt, d_st = outs[0]
    torch.cuda.synchronize()
    handle.surface_points_device(d_big.data_ptr(), d_boff.data_ptr(), 1, d_rec.data_ptr(), M, d_cnt.data_ptr(), d_st.data_ptr())
    handle.surface_points([clouds[1]])  # (synchronises the handle's stream)
    assert d_cnt[0].item() == 0 and d_st[0].item() == cf.STATUS_POINTS
    with pytest.raises(_rsx.RsxError, match="more than 16384"):
        handle.surface_points([big])


SP64 = np.dtype([("x", "<f8"), ("y", "<f8"), ("nx", "<f8"), ("ny", "<f8")])


def _as_records(a):
    out = np.zeros(len(a), dtype=cf.SP_DTYPE)
    for f in ("x", "y", "nx", "ny"):
        out[f] = a[f]
    out["lambda_max"], out["lambda_min"], out["n_points"] = 1.0, 0.5, 6
    return out


def _room():
    out = []
    for th, off in ((0.0, 12.0), (math.pi / 2, 9.0), (math.pi, 14.0), (-math.pi / 2, 11.0), (0.7, 20.0), (2.4, 17.0)):
        for i in range(9):
            along = -8.0 + 2.0 * i
            out.append((math.cos(th) * off - math.sin(th) * along, math.sin(th) * off + math.cos(th) * along, -math.cos(th), -math.sin(th)))
    return _as_records(np.array(out, dtype=SP64))


def _cases(drive):
    """(name, src, dst, init, restatement / parameter overrides, expected status)"""
    _, sp, _ = drive
    recs = [s[0] for s in sp]
    room = _room()
    flat = room.copy()
    flat["nx"], flat["ny"] = 1.0, 0.0
    over = np.zeros(cf.MAX_SURFACE_POINTS + 1, dtype=cf.SP_DTYPE)
    over["nx"] = 1.0
    cases = [(f"drive pair {i}", recs[i], recs[i - 1], None, {}, 0) for i in (1, 2, 3)]
    cases += [
        ("identical sets", recs[0], recs[0], None, {}, 0),
        ("room moved", room, cf.transform(room, (0.4, -0.3, 0.02)), None, {}, 0),
        ("non-identity init", recs[1], recs[0], (0.9, 0.1, 0.05), {}, 0),
        ("100 m apart", room, cf.transform(room, (100.0, 0.0, 0.0)), (0.5, 0.25, 0.125), {}, 4),
        ("normals (1, 0)", flat, flat, None, {}, 5),
        ("two iterations", recs[1], recs[0], None, {"max_iterations": 2}, 8),
        ("empty src", room[:0], room, (1.0, 2.0, 0.5), {}, 1),
        ("empty dst", room, room[:0], None, {}, 1),
        ("src over the cap", over, room, (1.0, 2.0, 0.5), {}, 2),
        ("dst at the cap", room, over[:-1], None, {}, 4),
    ]
    return cases


def _compare(name, got, want, left_out):
    d = max(abs(got["x"] - want["x"]), abs(got["y"] - want["y"]), abs(got["yaw"] - want["yaw"]), abs(got["cost"] - want["cost"]))
    print(f"{name}: status {got['status']}, {got['iterations']} iterations, {got['correspondences']} correspondences, "
          f"|GPU - restatement| {d:.2e}, margin {want['margin']:.1e}")
    if want["margin"] < 1e-9:
        left_out.append(name)
        return
    assert (got["status"], got["iterations"], got["correspondences"]) == (want["status"], want["iterations"], want["correspondences"]), (name, got, want)
    assert d < 1e-4, (name, got, want)


def test_registration_equals_the_restatement(handle, drive):
    from navtech_radar_slam_amd import cfear
    left_out, n = [], 0
    by_params = {}
    for case in _cases(drive):
        by_params.setdefault(tuple(sorted(case[4].items())), []).append(case)
    for key, cases in by_params.items():
        init = np.array([c[3] if c[3] is not None else (0.0, 0.0, 0.0) for c in cases])
        got = handle.register([c[1] for c in cases], [c[2] for c in cases], init, cfear.params(**dict(key)))
        for c, g in zip(cases, got):
            want = cf.register(c[1], c[2], init=c[3] if c[3] is not None else (0.0, 0.0, 0.0), **c[4])
            assert want["status"] == c[5], (c[0], want)
            assert want["margin"] >= 1e-9, (c[0], want["margin"])  # the restatement alone leaves out none
            _compare(c[0], g, want, left_out)
            if c[5] in (1, 2, 4):
                assert (g["x"], g["y"], g["yaw"]) == tuple(c[3] if c[3] is not None else (0.0, 0.0, 0.0)), (c[0], g)  # the start pose
            n += 1
    assert len(left_out) <= n // 100, left_out
    # init = NULL is the identity
    c = _cases(drive)[0]
    a = handle.register([c[1]], [c[2]])
    b = handle.register([c[1]], [c[2]], np.zeros((1, 3)))
    assert a.tobytes() == b.tobytes()


def test_drive_pairs_meet_the_odometry_bounds(handle, drive):
    _, sp, poses = drive
    got = handle.register([sp[i][0] for i in (1, 2, 3)], [sp[i - 1][0] for i in (1, 2, 3)])
    for i, g in zip((1, 2, 3), got):
        truth = synth.relative_pose(poses[i - 1], poses[i])
        et, ey = float(np.hypot(g["x"] - truth[0], g["y"] - truth[1])), abs(float(g["yaw"] - truth[2]))
        print(f"pair {i}: {et:.3f} m {ey:.1e} rad")
        assert g["status"] == 0 and et < 0.25 and ey < 1e-2


def test_registration_batch_position_entries_and_streams(handle, drive):
    import torch
    from navtech_radar_slam_amd import _rsx, cfear
    cases = [c for c in _cases(drive) if not c[4]]
    src, dst = [c[1] for c in cases], [c[2] for c in cases]
    init = np.array([c[3] if c[3] is not None else (0.0, 0.0, 0.0) for c in cases])
    batch = handle.register(src, dst, init)
    order = list(range(len(cases)))[::-1]  # the same pairs at other places of a batch
    back = handle.register([src[i] for i in order], [dst[i] for i in order], init[order])
    assert back[::-1].tobytes() == batch.tobytes()
    for i in (0, 3, len(cases) - 1):
        assert handle.register([src[i]], [dst[i]], init[i:i + 1]).tobytes() == batch[i:i + 1].tobytes()
    s, so = cfear.ragged(src, _rsx.CFEAR_SURFACE_POINT_DTYPE)
    d, do = cfear.ragged(dst, _rsx.CFEAR_SURFACE_POINT_DTYPE)
    dev = [torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a).cuda() for a in (s, so, d, do, init)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [torch.zeros(len(cases) * 48, dtype=torch.uint8, device="cuda") for _ in streams]
    torch.cuda.synchronize()
    for st, o in zip(streams, outs):
        handle.register_device(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), len(cases), o.data_ptr(),
                               d_init=dev[4].data_ptr(), stream=st.cuda_stream)
    torch.cuda.synchronize()
    for o in outs:
        assert o.cpu().numpy().tobytes() == batch.tobytes()


def test_bad_arguments(handle, drive):
    from navtech_radar_slam_amd import _rsx, cfear
    room = _room()
    for bad, word in ((dict(radius=0.0), "radius"), (dict(radius=-1.0), "radius"), (dict(radius=float("nan")), "radius"),
                      (dict(cos_max_normal_angle=1.5), "cos_max_normal_angle"), (dict(cos_max_normal_angle=-1.01), "cos_max_normal_angle"),
                      (dict(max_iterations=0), "max_iterations"), (dict(max_iterations=201), "max_iterations"),
                      (dict(min_points=1), "min_points"), (dict(huber_delta=0.0), "huber_delta")):
        with pytest.raises(_rsx.RsxError, match=word) as e:
            handle.register([room], [room], params=cfear.params(**bad))
        assert e.value.status == -1
        with pytest.raises(_rsx.RsxError, match=word):
            handle.surface_points([np.zeros((3, 2), dtype=np.float32)], cfear.params(**bad))
    L = _rsx.lib()
    xy = np.zeros((8, 2), dtype=np.float32)
    rec = np.zeros(8, dtype=_rsx.CFEAR_SURFACE_POINT_DTYPE)
    cnt = np.zeros(2, dtype=np.int32)
    for off in ([0, 5, 3], [1, 2, 3]):
        o = np.array(off, dtype=np.int64)
        assert L.rsx_cfear_surface_points_batch(handle._h, xy.ctypes.data, o.ctypes.data, 2, None, rec.ctypes.data, 4, cnt.ctypes.data, None) == -1
        assert b"offsets" in L.rsx_last_error_string()
        good = np.array([0, 4, 8], dtype=np.int64)
        out = np.zeros(2, dtype=_rsx.CFEAR_RESULT_DTYPE)
        assert L.rsx_cfear_register_batch(handle._h, rec.ctypes.data, o.ctypes.data, rec.ctypes.data, good.ctypes.data, 2, None, None, out.ctypes.data) == -1
        assert b"offsets" in L.rsx_last_error_string()
        assert L.rsx_cfear_register_batch(handle._h, rec.ctypes.data, good.ctypes.data, rec.ctypes.data, o.ctypes.data, 2, None, None, out.ctypes.data) == -1
        assert b"offsets" in L.rsx_last_error_string()
    for mr in (0, 4097):
        assert L.rsx_cfear_surface_points_batch(handle._h, xy.ctypes.data, np.array([0, 4, 8], dtype=np.int64).ctypes.data, 2, None, rec.ctypes.data, mr,
                                                cnt.ctypes.data, None) == -1
        assert b"max_records" in L.rsx_last_error_string()
