"""The radar grid map on the GPU (csrc/gridmap.hip through navtech_radar_slam_amd.gridmap) against its restatement (tests/gridmap_np.py):
the three planes byte for byte, every cell, no tolerance."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gridmap_cases as gc  # noqa: E402
import gridmap_np as gm  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rsx():
    import __graft_entry__ as ge
    from navtech_radar_slam_amd import _rsx
    if not os.path.exists(_rsx.LIB_PATH):
        ge.build()
    return _rsx


def _lib_params(p):
    from navtech_radar_slam_amd import gridmap
    return gridmap.params(**p)


def _map(rows, cols, p):
    from navtech_radar_slam_amd import gridmap
    return gridmap.GridMap(rows, cols, _lib_params(p))


def _same(got, want, what=""):
    for name, g, w in zip(("sum", "cnt", "hit"), got, want):
        assert g.dtype == np.uint32 and g.shape == w.shape, (what, name)
        assert g.tobytes() == w.tobytes(), (what, name, int(np.count_nonzero(g != w)), "cells differ")


def _restated(imgs, T, p):
    return gm.add_batch(gm.zeros(p), imgs, T, p, col_offset=gc.META)


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("width,height", [(64, 64), (192, 128)])
@pytest.mark.parametrize("cols", [96, 250])
@pytest.mark.parametrize("rows", [7, 64, 400])
def test_planes_equal_the_restatement(rsx, rows, cols, width, height, n):
    imgs, T, p = gc.random_case(rows * 1000 + cols + width + n, rows, cols, width, height, n)
    m = _map(rows, cols, p)
    m.add(imgs, T)
    want = _restated(imgs, T, p)
    assert want[1].any()
    _same(m.read(), want, (rows, cols, width, height, n))
    m.close()


@pytest.mark.parametrize("hw", [0, 5, 13, 200])
def test_range_halfwidths(rsx, hw):
    """below, just above and well above the nine bytes the kernel loads without a loop; 200: every span clipped at both ends"""
    imgs, T, p = gc.random_case(500 + hw, 64, 96, 64, 64, 2, range_halfwidth=hw)
    m = _map(64, 96, p)
    m.add(imgs, T)
    _same(m.read(), _restated(imgs, T, p), hw)
    m.close()


def test_matrices_are_coral_pose_matrices():
    """the poses of every case here go through the layout coral.pose_matrices produces"""
    from navtech_radar_slam_amd import coral
    poses = np.array([(1.5, -2.0, 0.3), (0.0, 4.0, -2.9), (7.0, 7.0, 0.0)])
    assert gc.matrices(poses).tobytes() == coral.pose_matrices(poses).tobytes()


def test_one_call_equals_three_and_clear(rsx):
    imgs, T, p = gc.random_case(42, 64, 96, 192, 128, 3)
    want = _restated(imgs, T, p)
    a, b = _map(64, 96, p), _map(64, 96, p)
    a.add(imgs, T)
    for i in (2, 0, 1):
        b.add(imgs[i:i + 1], T[i:i + 1])
    _same(a.read(), want, "one call")
    _same(b.read(), want, "three calls")
    a.clear()
    _same(a.read(), gm.zeros(p), "cleared")
    a.add(imgs[:2], T[:2])
    a.add(imgs[2:], T[2:])
    _same(a.read(), want, "after clear")
    a.close()
    b.close()


@pytest.mark.parametrize("case", gc.border_cases(), ids=lambda c: c[0])
def test_borders_and_corners(rsx, case):
    name, imgs, T, p = case
    m = _map(imgs.shape[1], imgs.shape[2] - gc.META, p)
    m.add(imgs, T)
    want = _restated(imgs, T, p)
    assert want[1].any() == (name != "far")       # a sensor far outside leaves the planes unchanged
    _same(m.read(), want, name)
    m.close()


@pytest.mark.parametrize("case", gc.tile_cases(), ids=lambda c: c[0])
def test_scans_on_the_same_and_on_different_tiles(rsx, case):
    name, imgs, T, p = case
    want = _restated(imgs, T, p)
    tiles = [set(map(tuple, np.argwhere(gm.add_batch(gm.zeros(p), imgs[i:i + 1], T[i:i + 1], p, col_offset=gc.META)[1] > 0) // 32)) for i in range(len(T))]
    if name == "same":
        assert set.intersection(*tiles) and want[1].max() == len(T)
    else:
        assert all(not (tiles[i] & tiles[j]) for i in range(len(T)) for j in range(i)) and want[1].max() == 1
    m = _map(imgs.shape[1], imgs.shape[2] - gc.META, p)
    m.add(imgs, T)
    _same(m.read(), want, name)
    m.close()


@pytest.mark.parametrize("rows,on_corner", [(8, True), (8, False), (4, True), (4, False)])
def test_exact_ties_and_boundaries(rsx, rows, on_corner):
    """Cells exactly on a bin edge and exactly on the bisector of two beams.  The case with the sensor on a cell corner and 8 rows holds
    neither (gridmap_cases.tie_case says why): a sensor on a cell centre gives the edges, 4 rows give the bisecting diagonals, and 8 rows
    on a centre give the sensor's own cell (d2 = 0: every row ties).  Each count is asserted, so that a case cannot stop testing what
    it is for."""
    imgs, T, p = gc.tie_case(rows, on_corner)
    on_edge, tied = gc.exact_ties(T[0], p, rows, 96)
    assert (on_edge > 0) == (not on_corner), on_edge
    assert (tied > 0) == (rows == 4 or not on_corner), tied
    if rows == 4:
        assert tied >= 20
    if not on_corner:
        assert on_edge >= 100
    m = _map(rows, 96, p)
    m.add(imgs, T)
    _same(m.read(), _restated(imgs, T, p), (rows, on_corner))
    m.close()


def _padded_device_batch(imgs, rows, cols, torch):
    """the images in a device buffer with a longer row_stride, a padded image stride and a base address that is 3 modulo 16; every
    byte that is not a power sample of [col_offset, col_offset + cols) of a row -- the metadata included -- is 255"""
    n = len(imgs)
    row_stride, img_stride, lead = cols + gc.META + 21, rows * (cols + gc.META + 21) + 77, 3
    host = np.full(lead + n * img_stride + 64, 255, dtype=np.uint8)
    for i in range(n):
        view = host[lead + i * img_stride:lead + i * img_stride + rows * row_stride].reshape(rows, row_stride)
        view[:, gc.META:gc.META + cols] = imgs[i][:, gc.META:]
    buf = torch.from_numpy(host).cuda()
    assert buf.data_ptr() % 16 == 0
    return buf, torch.as_strided(buf, (n, rows, row_stride), (img_stride, row_stride, 1), lead)


def test_device_entry_equals_host_entry(rsx):
    import torch
    rows, cols = 7, 250
    imgs, T, p = gc.random_case(77, rows, cols, 192, 128, 5, min_range_bins=0, range_halfwidth=3)
    host, dev = _map(rows, cols, p), _map(rows, cols, p)
    host.add(imgs, T)
    buf, view = _padded_device_batch(imgs, rows, cols, torch)
    assert view.data_ptr() % 16 == 3
    status = torch.full((5,), -1, dtype=torch.int32, device="cuda")
    dev.add_device(view, torch.from_numpy(T).cuda(), col_offset=gc.META, status=status, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * 5
    want = _restated(imgs, T, p)
    _same(host.read(), want, "host")
    _same(dev.read(), want, "device")         # a read outside the samples would have met a 255
    host.close()
    dev.close()


def test_non_finite_transform(rsx):
    import torch
    rows, cols = 64, 96
    imgs, T, p = gc.random_case(78, rows, cols, 64, 64, 5)
    for k, bad in ((2, np.nan), (0, np.inf), (4, -np.inf)):
        Tb = T.copy()
        Tb[3, k] = bad
        m = _map(rows, cols, p)
        with pytest.raises(rsx.RsxError, match="not finite"):
            m.add(imgs, Tb)
        _same(m.read(), gm.zeros(p), "refused")
        status = torch.full((5,), -1, dtype=torch.int32, device="cuda")
        d_imgs, d_T = torch.from_numpy(imgs).cuda(), torch.from_numpy(Tb).cuda()
        torch.cuda.synchronize()
        m.add_device(d_imgs, d_T, status=status)                              # (on the handle's own stream)
        m.add_device(d_imgs, d_T)                                             # (the status is optional)
        got = m.read()                                                        # (synchronises the handle's stream)
        assert status.cpu().tolist() == [0, 0, 0, rsx.GRIDMAP_STATUS_TRANSFORM, 0]
        keep = [0, 1, 2, 4]
        once = _restated(imgs[keep], T[keep], p)
        _same(got, tuple(2 * q for q in once), (k, bad))
        m.close()


def test_read_windows_and_renders(rsx):
    import torch
    rows, cols = 64, 96
    imgs, T, p = gc.random_case(79, rows, cols, 192, 128, 5)
    T[:, [2, 5]] = T[:1, [2, 5]] + np.arange(5)[:, None] * 0.8                # overlapping footprints: counts of 0 .. 5
    want = _restated(imgs, T, p)
    assert set(np.unique(want[1])) >= {0, 1, 2, 3, 5}
    m = _map(rows, cols, p)
    m.add(imgs, T)
    L = rsx.lib()
    from test_gridmap_abi import check_argument_rules
    check_argument_rules(rsx, m.handle, rows, cols, 192, 128)
    _same(m.read(), want, "after the refused calls")
    for x, y, w, h in ((0, 0, 192, 128), (0, 0, 1, 1), (191, 127, 1, 1), (5, 9, 33, 17), (64, 0, 128, 128), (0, 127, 192, 1)):
        _same(m.read((x, y, w, h)), tuple(q[y:y + h, x:x + w] for q in want), (x, y, w, h))
        only_cnt = np.zeros((h, w), dtype=np.uint32)
        assert L.rsx_gridmap_read(m.handle, x, y, w, h, None, only_cnt.ctypes.data, None) == 0
        assert only_cnt.tobytes() == np.ascontiguousarray(want[1][y:y + h, x:x + w]).tobytes()
        for mo in (1, 3):
            mean, hits = gm.render_mean(want, mo)[y:y + h, x:x + w], gm.render_hits(want, mo)[y:y + h, x:x + w]
            assert m.mean(mo, (x, y, w, h)).tobytes() == np.ascontiguousarray(mean).tobytes()
            assert m.hits(mo, (x, y, w, h)).tobytes() == np.ascontiguousarray(hits).tobytes()
            d_mean = torch.full((h, w), 7, dtype=torch.uint8, device="cuda")
            d_hits = torch.full((h, w), 7, dtype=torch.int8, device="cuda")
            s = torch.cuda.current_stream().cuda_stream
            m.render_device(rsx.GRIDMAP_MEAN, d_mean, mo, (x, y, w, h), stream=s)
            m.render_device(rsx.GRIDMAP_HITS, d_hits, mo, (x, y, w, h), stream=s)
            torch.cuda.synchronize()
            assert d_mean.cpu().numpy().tobytes() == np.ascontiguousarray(mean).tobytes()
            assert d_hits.cpu().numpy().tobytes() == np.ascontiguousarray(hits).tobytes()
    hits = gm.render_hits(want, 3)
    assert hits.min() == -1 and 0 <= hits[want[1] >= 3].min() and hits.max() <= 100
    # the planes in place
    d_sum, d_cnt, d_hit, pitch = m.planes_device()
    assert pitch == 192 * 4 and d_cnt - d_sum == 192 * 128 * 4 and d_hit - d_cnt == 192 * 128 * 4
    m.close()


def test_save_pgm(rsx, tmp_path):
    rows, cols = 64, 96
    imgs, T, p = gc.random_case(80, rows, cols, 192, 128, 3)
    want = _restated(imgs, T, p)
    m = _map(rows, cols, p)
    m.add(imgs, T)
    m.save_pgm(str(tmp_path / "mean.pgm"))
    m.save_pgm(str(tmp_path / "hits.pgm"), mode=rsx.GRIDMAP_HITS, min_observations=2)
    head = b"P5\n192 128\n255\n"
    assert (tmp_path / "mean.pgm").read_bytes() == head + gm.render_mean(want).tobytes()
    h = gm.render_hits(want, 2).astype(np.int16)
    assert (tmp_path / "hits.pgm").read_bytes() == head + np.where(h < 0, 255, 254 - 2 * h).astype(np.uint8).tobytes()
    m.close()


def test_default_map_full_size_scans(rsx):
    """the one case at the workload's shape: the tile list at 1024 tiles, two 400 x 3360 scans whose footprints reach past the map"""
    from navtech_radar_slam_amd import coral, synth
    imgs, _, poses, _ = synth.polar_sequence(11, 2)
    p = gm.params()
    T = coral.pose_matrices(poses + np.array([[60.0, -45.0, 0.7], [60.0, -45.0, 0.7]]))
    m = _map(400, 3360, p)
    m.add(imgs, T)
    want = gm.add_batch(gm.zeros(p), imgs, T, p, col_offset=synth.OXFORD_META)
    assert want[1].max() == 2 and (want[1] == 0).any()
    _same(m.read(), want, "default map")
    m.close()
