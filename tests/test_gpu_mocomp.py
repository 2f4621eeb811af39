"""rsx_mocomp_points_batch / rsx_mocomp_matches_batch (csrc/mocomp.hip) against their arithmetic contract, the numpy
restatement tests/mocomp_np.py: BIT-IDENTICAL fp32 outputs (the kernels evaluate fixed polynomials, correctly rounded
divisions and square roots, nothing fused; no library sin / cos) for each of the three flag combinations, the status bit and
the untouched points around |wz tau| = 1/2, degenerate inputs, the device entries, and the argument rules.  PARITY UNPINNED
w.r.t. upstream (its sources are absent from the reference checkout)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mocomp_np as mn  # noqa: E402

pytestmark = pytest.mark.gpu
ROWS, DT = 400, 0.25
# points per scan: an empty first scan, 1, the wave size and its neighbours, an empty scan in the middle, 1000, and one scan
# above the 4096 points a sweep of the grid covers
SIZES = [0, 1, 63, 64, 0, 65, 1000, 4100]
WZ_EDGE = 0.5 / (((ROWS - 1 + 0.5) / ROWS) * DT)   # wz tau = 1/2 on the last row (up to rounding)


@pytest.fixture(scope="module")
def mo():
    from navtech_radar_slam_amd import _rsx, mocomp
    assert _rsx.device_count() >= 1
    h = mocomp.Mocomp()
    yield h
    h.close()


@pytest.fixture(scope="module")
def clouds():
    rng = np.random.default_rng(6101)
    off = np.zeros(len(SIZES) + 1, dtype=np.int64)
    off[1:] = np.cumsum(SIZES)
    m = int(off[-1])
    r, th = rng.uniform(2.0, 180.0, m), rng.uniform(0.0, 2 * np.pi, m)
    xy = np.stack([r * np.cos(th), r * np.sin(th)], axis=1).astype(np.float32)
    rows = rng.integers(0, ROWS, m).astype(np.int32)
    w = np.stack([rng.uniform(10, 20, len(SIZES)), rng.uniform(-3, 3, len(SIZES)), rng.uniform(-0.3, 0.3, len(SIZES))], axis=1)
    w[3, 2] = 0.0                          # wz = 0 exactly (64 points)
    w[5, 2] = WZ_EDGE * (1 - 1e-9)         # every |th| just below 1/2 (65 points) ...
    rows[off[5]:off[5] + 3] = (ROWS - 1, ROWS - 1, 0)
    w[6, 2] = -WZ_EDGE * (1 + 1e-9)        # ... and just above it on the last row only (1000 points)
    rows[off[6]:off[6] + 4] = (ROWS - 1, ROWS - 2, ROWS - 1, 0)
    # a point at the origin, points on the axes, NaN and infinite input (scan 7)
    o = off[7]
    xy[o:o + 6] = [[0.0, 0.0], [25.0, 0.0], [0.0, -25.0], [np.nan, 3.0], [4.0, np.nan], [np.inf, 1.0]]
    xy[off[3]] = [0.0, 0.0]
    return xy, rows, off, w


def _params(flags, **kw):
    from navtech_radar_slam_amd import mocomp
    return mocomp.default_params(flags=flags, rows=ROWS, dt_scan=DT, **kw)


@pytest.mark.parametrize("flags", [1, 2, 3])
def test_points_bit_identical_to_the_restatement(mo, clouds, flags):
    xy, rows, off, w = clouds
    got, st = mo.points_batch(xy, rows, off, w, _params(flags))
    want, wst = mn.points_batch(xy, rows, off, w, flags, dt_scan=DT, beta=0.049, rows=ROWS)
    assert np.array_equal(st, wst), (st, wst)
    assert mn.same_bits(got, want), int(np.sum(got.view(np.uint32) != want.view(np.uint32)))
    if flags & 1:
        assert st.tolist() == [0, 0, 0, 0, 0, 0, 1, 0]
        last = rows[off[6]:off[7]] == ROWS - 1
        seg = slice(off[6], off[7])
        assert last.sum() >= 2 and np.array_equal(got[seg][last], xy[seg][last])        # left as measured, Doppler included
        assert not np.any(np.all(got[seg][~last] == xy[seg][~last], axis=1))
        assert not np.any(np.all(got[off[5]:off[6]] == xy[off[5]:off[6]], axis=1))      # just below 1/2: every point moved
    else:
        assert not st.any()
    o = off[7]
    assert got[o].tolist() == [0.0, 0.0] or flags & 1                                   # Doppler alone leaves the origin
    assert np.isnan(got[o + 3]).all() and np.isnan(got[o + 4]).all()                    # NaN stays NaN
    assert np.isfinite(got[o + 6:]).all() and np.isfinite(got[:o]).all()
    # a negative beta and another period / row count
    p2 = _params(flags, beta=-0.02)
    p2.dt_scan, p2.rows = 0.1, 577
    got2, st2 = mo.points_batch(xy, rows, off, w, p2)
    want2, wst2 = mn.points_batch(xy, rows, off, w, flags, dt_scan=0.1, beta=-0.02, rows=577)
    assert np.array_equal(st2, wst2) and mn.same_bits(got2, want2)


def _match_set(seed=6201, sizes=(5, 300, 1500)):
    rng = np.random.default_rng(seed)
    off = np.zeros(len(sizes) + 1, dtype=np.int64)
    off[1:] = np.cumsum(sizes)
    m = int(off[-1])
    mk = lambda: np.stack([rng.uniform(-150, 150, m), rng.uniform(-150, 150, m)], axis=1).astype(np.float32)
    src, dst = mk(), mk()
    a_cur, a_prev = rng.integers(0, ROWS, m).astype(np.int32), rng.integers(0, ROWS, m).astype(np.int32)
    pose = np.stack([rng.uniform(2, 5, len(sizes)), rng.uniform(-0.5, 0.5, len(sizes)), rng.uniform(-0.08, 0.08, len(sizes))], axis=1)
    return src, dst, a_cur, a_prev, off, pose


@pytest.mark.parametrize("flags", [1, 2, 3])
def test_matches_bit_identical_to_the_restatement(mo, flags):
    src, dst, a_cur, a_prev, off, pose = _match_set()
    gs, gd, st = mo.matches_batch(src, dst, a_cur, a_prev, off, pose, _params(flags))
    ws, wd, wst = mn.matches_batch(src, dst, a_cur, a_prev, off, pose, flags, dt_scan=DT, beta=0.049, rows=ROWS)
    assert not st.any() and np.array_equal(st, wst)
    assert mn.same_bits(gs, ws) and mn.same_bits(gd, wd)
    assert not np.any(np.all(gs == src, axis=1))
    # poses without a velocity: the pair is copied through and flagged; yaw = 0 exactly; |yaw| = 1/2 still has one
    pose2 = pose.copy()
    pose2[0] = (1.0, 0.0, 0.500001)
    pose2[1] = (3.0, 0.2, 0.0)
    pose2[2] = (np.nan, 0.0, 0.01)
    gs, gd, st = mo.matches_batch(src, dst, a_cur, a_prev, off, pose2, _params(flags))
    ws, wd, wst = mn.matches_batch(src, dst, a_cur, a_prev, off, pose2, flags, dt_scan=DT, beta=0.049, rows=ROWS)
    assert st.tolist() == [1, 0, 1] and np.array_equal(st, wst)
    assert mn.same_bits(gs, ws) and mn.same_bits(gd, wd)
    assert np.array_equal(gs[:5], src[:5]) and np.array_equal(gd[off[2]:], dst[off[2]:])
    pose2[0] = (1.0, 0.0, -0.5)
    gs, gd, st = mo.matches_batch(src, dst, a_cur, a_prev, off, pose2, _params(flags))
    ws, wd, wst = mn.matches_batch(src, dst, a_cur, a_prev, off, pose2, flags, dt_scan=DT, beta=0.049, rows=ROWS)
    assert np.array_equal(st, wst) and mn.same_bits(gs, ws) and mn.same_bits(gd, wd)


def test_host_entries_equal_device_entries(mo, clouds):
    import torch
    xy, rows, off, w = clouds
    prm = _params(3)
    want, wst = mo.points_batch(xy, rows, off, w, prm)
    d_xy, d_rows, d_off, d_w = (torch.from_numpy(a).cuda() for a in (xy, rows, off, np.ascontiguousarray(w)))
    d_out = torch.full((len(xy), 2), 7.0, dtype=torch.float32, device="cuda")
    d_st = torch.full((len(SIZES),), 99, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        mo.points_batch_device(d_xy.data_ptr(), d_rows.data_ptr(), d_off.data_ptr(), len(SIZES), d_w.data_ptr(), d_out.data_ptr(), d_st.data_ptr(),
                               params=prm, stream=stream.cuda_stream)
    torch.cuda.synchronize()
    assert mn.same_bits(d_out.cpu().numpy(), want) and np.array_equal(d_st.cpu().numpy(), wst)
    # without a status array, on the handle's own stream
    d_out.fill_(7.0)
    torch.cuda.synchronize()
    mo.points_batch_device(d_xy.data_ptr(), d_rows.data_ptr(), d_off.data_ptr(), len(SIZES), d_w.data_ptr(), d_out.data_ptr(), None, params=prm)
    mo.points_batch(xy[:1], rows[:1], [0, 1], w[:1], prm)   # (synchronises the handle's stream)
    assert mn.same_bits(d_out.cpu().numpy(), want)

    src, dst, a_cur, a_prev, moff, pose = _match_set()
    ws, wd, wst = mo.matches_batch(src, dst, a_cur, a_prev, moff, pose, prm)
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (src, dst, a_cur, a_prev, moff, pose)]
    o_s, o_d = torch.zeros_like(d[0]), torch.zeros_like(d[1])
    o_st = torch.full((3,), 99, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    mo.matches_batch_device(*(t.data_ptr() for t in d[:5]), 3, d[5].data_ptr(), o_s.data_ptr(), o_d.data_ptr(), o_st.data_ptr(), params=prm,
                            stream=stream.cuda_stream)
    torch.cuda.synchronize()
    assert mn.same_bits(o_s.cpu().numpy(), ws) and mn.same_bits(o_d.cpu().numpy(), wd) and np.array_equal(o_st.cpu().numpy(), wst)


def test_argument_rules(mo, clouds):
    from navtech_radar_slam_amd import _rsx
    L = _rsx.lib()
    xy, rows, off, w = clouds
    out, st = np.zeros_like(xy), np.zeros(len(SIZES), dtype=np.int32)
    w = np.ascontiguousarray(w)

    def points(p, h=mo._h, a=xy.ctypes.data, o=out.ctypes.data):
        return L.rsx_mocomp_points_batch(h, a, rows.ctypes.data, off.ctypes.data, len(SIZES), w.ctypes.data, C.byref(p) if p is not None else None, o,
                                         st.ctypes.data)

    assert points(_params(3)) == 0
    assert points(None) == 0                                   # NULL: the defaults, both corrections
    assert mn.same_bits(out, mn.points_batch(xy, rows, off, w, 3)[0])
    for flags in (0, 4, 7, -1):
        assert points(_params(flags)) == -1, flags
    bad = _params(3)
    bad.dt_scan = 0.0
    assert points(bad) == -1
    bad = _params(3)
    bad.rows = 0
    assert points(bad) == -1
    bad = _params(3)
    bad.beta = float("nan")
    assert points(bad) == -1 and b"beta" in L.rsx_last_error_string()
    assert points(_params(3), h=None) == -1 and points(_params(3), a=None) == -1 and points(_params(3), o=None) == -1
    assert L.rsx_mocomp_points_batch_device(mo._h, None, None, None, 1, None, None, None, None, None) == -1
    assert L.rsx_mocomp_matches_batch(mo._h, None, None, None, None, None, 1, None, None, None, None, None) == -1
    assert L.rsx_mocomp_matches_batch_device(None, None, None, None, None, None, 1, None, None, None, None, None, None) == -1
    assert L.rsx_mocomp_default_params(None) == -1 and L.rsx_mocomp_create(0, None) == -1 and L.rsx_mocomp_destroy(None) == 0
    bad_off = off.copy()
    bad_off[0] = 1
    assert L.rsx_mocomp_points_batch(mo._h, xy.ctypes.data, rows.ctypes.data, bad_off.ctypes.data, len(SIZES), w.ctypes.data, None, out.ctypes.data,
                                     None) == -1
    # offsets that decrease in the middle, or go negative: both host entries refuse them before anything is written
    decreasing, negative = off.copy(), off.copy()
    decreasing[2] = 100                                        # 0, 0, 100, 64, ..
    negative[1] = -1
    out7, st7 = np.full_like(xy, 7.0), np.full(len(SIZES), 99, dtype=np.int32)
    for bad_off in (decreasing, negative):
        assert L.rsx_mocomp_points_batch(mo._h, xy.ctypes.data, rows.ctypes.data, bad_off.ctypes.data, len(SIZES), w.ctypes.data, None,
                                         out7.ctypes.data, st7.ctypes.data) == -1
        assert b"offsets" in L.rsx_last_error_string()
    assert (out7 == 7.0).all() and (st7 == 99).all()
    assert L.rsx_mocomp_points_batch(mo._h, xy.ctypes.data, rows.ctypes.data, off.ctypes.data, len(SIZES), w.ctypes.data, None, out7.ctypes.data,
                                     st7.ctypes.data) == 0
    assert mn.same_bits(out7, mn.points_batch(xy, rows, off, w, 3)[0])
    src, dst, a_cur, a_prev, moff, pose = _match_set()
    pose, m = np.ascontiguousarray(pose), int(moff[-1])
    os7, od7, mst7 = np.full_like(src, 7.0), np.full_like(dst, 7.0), np.full(3, 99, dtype=np.int32)

    def matches(o):
        return L.rsx_mocomp_matches_batch(mo._h, src.ctypes.data, dst.ctypes.data, a_cur.ctypes.data, a_prev.ctypes.data, o.ctypes.data, 3,
                                          pose.ctypes.data, None, os7.ctypes.data, od7.ctypes.data, mst7.ctypes.data)

    for bad_off in ([0, 60, 40, m], [0, -1, 40, m], [1, 5, 305, m]):
        assert matches(np.array(bad_off, dtype=np.int64)) == -1 and b"offsets" in L.rsx_last_error_string(), bad_off
    assert (os7 == 7.0).all() and (od7 == 7.0).all() and (mst7 == 99).all()
    assert matches(moff) == 0
    ws, wd, wst = mn.matches_batch(src, dst, a_cur, a_prev, moff, pose, 3)
    assert mn.same_bits(os7, ws) and mn.same_bits(od7, wd) and np.array_equal(mst7, wst)
    # zero scans: nothing to do
    assert L.rsx_mocomp_points_batch(mo._h, xy.ctypes.data, rows.ctypes.data, off.ctypes.data, 0, w.ctypes.data, None, out.ctypes.data, None) == 0
    p = _rsx.MocompParams()
    assert L.rsx_mocomp_default_params(C.byref(p)) == 0 and (p.dt_scan, p.beta, p.rows, p.flags) == (0.25, 0.049, 400, 3)
