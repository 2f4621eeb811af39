"""GPU parity of cen2018 keypoint extraction (csrc/cen2018.hip through the C-ABI) against the numpy restatement of its
arithmetic contract (tests/cen2018_np.py).  mean, sigma, p and the filter taps are bit-identical; the keypoints are
identical row by row, except in a row where the restatement's decision for some pixel flips when nqp or npp moves by one
float ulp (the device's fp64 exp and the host's may differ in the last bit) -- such rows are counted and must be rare."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from navtech_radar_slam_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cen2018_np as c18  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cen():
    from navtech_radar_slam_amd import cen2018
    return cen2018


def compare_rows(got, want, exempt=()):
    """targets equal row by row outside `exempt`; -> the rows that differ"""
    rows = set(got[:, 0].tolist()) | set(want[:, 0].tolist())
    bad = []
    for a in sorted(rows):
        if not np.array_equal(got[got[:, 0] == a], want[want[:, 0] == a]):
            bad.append(a)
    assert set(bad) <= set(int(r) for r in exempt), (bad, list(exempt))
    return bad


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_mulran_shape_against_restatement(cen, oracle, seed):
    img, az, _ = synth.polar_image(seed, n_targets=800 + 200 * seed)
    ex = cen.Cen2018(400, 3360)
    want, dbg = c18.extract(img, debug=True)
    fragile = c18.fragile_rows(dbg, 58)
    print(f"seed {seed}: {len(want)} keypoints, {len(fragile)} rows with a decision within one ulp of an exp")
    assert len(fragile) <= 1
    d = ex.debug_image(img)
    assert np.array_equal(d["mean"], dbg["mean"]) and np.array_equal(d["sigma"], dbg["sigma"])
    assert np.array_equal(d["p"], dbg["p"])
    assert np.allclose(d["y"], dbg["y"], rtol=1e-5, atol=1e-6)
    assert np.array_equal(cen.gauss_weights(17), dbg["w"])
    got, xy, n = ex.extract(img, azimuths=az, resolution=synth.RADAR_RESOLUTION, return_count=True)
    assert n == len(got)
    compare_rows(got, want, fragile)
    if len(fragile) == 0:
        assert np.array_equal(got, want)
    wxy = oracle.cen2019_to_cartesian(got, az, synth.RADAR_RESOLUTION)
    assert np.allclose(xy, wxy, rtol=1e-5, atol=1e-4)
    assert np.array_equal(ex.extract(img), got)  # same handle, same bytes


def test_sequence_scans(cen):
    imgs, az, _, _ = synth.polar_sequence(11, 4)
    ex = cen.Cen2018(400, 3360)
    tg = ex.extract_batch(imgs)
    for i in range(len(imgs)):
        want, dbg = c18.extract(imgs[i], debug=True)
        fr = c18.fragile_rows(dbg, 58)
        assert len(fr) <= 1
        compare_rows(tg[i], want, fr)


def _device_batch(cen, ex, imgs, az, max_targets, **kw):
    import torch
    from navtech_radar_slam_amd import _rsx
    n = imgs.shape[0]
    d_img = torch.from_numpy(np.ascontiguousarray(imgs)).cuda()
    d_az = torch.from_numpy(np.ascontiguousarray(az, dtype=np.float32)).cuda()
    d_tg = torch.zeros((n, max_targets, 2), dtype=torch.int32, device="cuda")
    d_xy = torch.zeros((n, max_targets, 2), dtype=torch.float32, device="cuda")
    d_cn = torch.zeros(n, dtype=torch.int32, device="cuda")
    p = cen.params(**kw)
    s = torch.cuda.current_stream()
    _rsx.check(ex._L.rsx_cen2018_extract_batch_device(ex._h, d_img.data_ptr(), n, imgs.strides[0], imgs.shape[2], 11, C.byref(p),
                                                       d_az.data_ptr(), 1 if az.ndim == 2 else 0, synth.RADAR_RESOLUTION, d_tg.data_ptr(),
                                                       d_xy.data_ptr(), max_targets, d_cn.data_ptr(), C.c_void_p(s.cuda_stream)))
    torch.cuda.synchronize()
    cn = d_cn.cpu().numpy()
    k = np.minimum(cn, max_targets)
    tg, xy = d_tg.cpu().numpy(), d_xy.cpu().numpy()
    return [tg[i, :k[i]] for i in range(n)], [xy[i, :k[i]] for i in range(n)], cn


def test_batch_equals_single_and_device_with_per_image_azimuths(cen):
    imgs = np.stack([synth.polar_image(20 + i, n_targets=500 + 300 * i)[0] for i in range(5)])
    az = np.stack([synth.polar_image(20 + i)[1] + np.float32(0.01 * i) for i in range(5)]).astype(np.float32)
    ex = cen.Cen2018(400, 3360)
    tg, xy = ex.extract_batch(imgs, azimuths=az, resolution=synth.RADAR_RESOLUTION)
    dtg, dxy, _ = _device_batch(cen, ex, imgs, az, 20000)
    for i in range(len(imgs)):
        one, one_xy = ex.extract(imgs[i], azimuths=az[i], resolution=synth.RADAR_RESOLUTION)
        assert np.array_equal(one, tg[i]) and np.array_equal(one_xy, xy[i])
        assert np.array_equal(dtg[i], tg[i]) and np.array_equal(dxy[i], xy[i])


@pytest.mark.parametrize("sg", [1, 3, 17, 33])
@pytest.mark.parametrize("zq", [1.5, 3.0, 6.0])
def test_parameter_ranges(cen, sg, zq):
    img, _, _ = synth.polar_image(40 + sg, rows=48, n_targets=200)
    cols = img.shape[1] - 11
    ex = cen.Cen2018(48, cols)
    for mr in (0, 58, cols - 1, cols, cols + 5):
        want, dbg = c18.extract(img, zq=zq, sigma_gauss=sg, min_range=mr, debug=True)
        fr = c18.fragile_rows(dbg, mr)
        got = ex.extract(img, zq=zq, sigma_gauss=sg, min_range=mr)
        compare_rows(got, want, fr)
        d = ex.debug_image(img, zq=zq, sigma_gauss=sg, min_range=mr)
        assert np.array_equal(d["p"], dbg["p"]) and np.array_equal(d["sigma"], dbg["sigma"])


@pytest.mark.parametrize("rows,cols", [(1, 1), (7, 2), (7, 30), (401, 30), (1, 4000), (7, 4000), (401, 2)])
def test_odd_shapes_and_row_stride(cen, rows, cols):
    rng = np.random.default_rng(rows * 10007 + cols)
    stride = 5 + cols + 9  # col_offset 5, 9 bytes of padding behind every row
    img = rng.gamma(2.0, 14.0, size=(rows, stride)).clip(0, 255).astype(np.uint8)
    for _ in range(rows * 3):
        a, r = int(rng.integers(0, rows)), int(rng.integers(0, cols))
        img[a, 5 + r:5 + min(r + int(rng.integers(1, 8)), cols)] = rng.integers(120, 255)
    ex = cen.Cen2018(rows, cols)
    for sg, mr in ((1, 0), (3, 1), (17, 0)):
        want, dbg = c18.extract(img, col_offset=5, sigma_gauss=sg, min_range=mr, zq=1.5, cols=cols, debug=True)
        fr = c18.fragile_rows(dbg, mr)
        got = ex.extract(img, col_offset=5, sigma_gauss=sg, min_range=mr, zq=1.5)
        compare_rows(got, want, fr)
        d = ex.debug_image(img, col_offset=5, sigma_gauss=sg, min_range=mr, zq=1.5)
        assert np.array_equal(d["p"], dbg["p"]) and np.array_equal(d["mean"], dbg["mean"]) and np.array_equal(d["sigma"], dbg["sigma"])


def test_batch_larger_than_a_sub_batch(cen):
    """300 images of 9 x 500 (> 128, the internal sub-batch), every one against the restatement; a strided batch"""
    rng = np.random.default_rng(77)
    nb, rows, cols = 300, 9, 500
    big = rng.gamma(2.0, 14.0, size=(nb, rows + 1, cols)).clip(0, 255).astype(np.uint8)
    for i in range(nb):
        for _ in range(6):
            a, r = int(rng.integers(0, rows)), int(rng.integers(0, cols - 6))
            big[i, a, r:r + int(rng.integers(1, 6))] = rng.integers(120, 255)
    imgs = big[:, :rows]  # image stride = (rows + 1) * cols
    ex = cen.Cen2018(rows, cols)
    tg, cn = ex.extract_batch(imgs, col_offset=0, sigma_gauss=5, min_range=3, zq=2.0, return_counts=True)
    for i in range(nb):
        want, dbg = c18.extract(imgs[i], col_offset=0, sigma_gauss=5, min_range=3, zq=2.0, debug=True)
        compare_rows(tg[i], want, c18.fragile_rows(dbg, 3))
        assert cn[i] == len(tg[i])


def test_max_targets_truncation(cen):
    img, az, _ = synth.polar_image(5, n_targets=1000)
    ex = cen.Cen2018(400, 3360)
    full = ex.extract(img)
    for mt in (1, 100, len(full) - 1, len(full), len(full) + 10):
        got, n = ex.extract(img, max_targets=mt, return_count=True)
        assert n == len(full) and np.array_equal(got, full[:mt]), mt
    imgs = np.stack([img, synth.polar_image(6, n_targets=1000)[0]])
    tg, cn = ex.extract_batch(imgs, max_targets=500, return_counts=True)
    assert cn[0] == len(full) and np.array_equal(tg[0], full[:500])
    dtg, _, dcn = _device_batch(cen, ex, imgs, np.stack([az, az]), 500)
    assert np.array_equal(dcn, cn) and np.array_equal(dtg[0], full[:500]) and np.array_equal(dtg[1], tg[1])


def test_bad_arguments(cen):
    from navtech_radar_slam_amd import _rsx
    L = _rsx.lib()
    h = C.c_void_p()
    for rows, cols in ((0, 100), (10, 0), (5000, 10), (10, 9000)):
        h.value = 1
        assert L.rsx_cen2018_create(0, rows, cols, C.byref(h)) == -1 and not h.value
    ex = cen.Cen2018(8, 64)
    img = np.zeros((8, 64), dtype=np.uint8)
    out = np.zeros((10, 2), dtype=np.int32)
    n = C.c_int32()
    for zq, sg, mr in ((3.0, 2, 0), (3.0, 0, 0), (3.0, -1, 0), (3.0, 87, 0), (3.0, 3, -1), (float("inf"), 3, 0), (float("nan"), 3, 0)):
        p = _rsx.Cen2018Params(zq, sg, mr, 0)
        assert L.rsx_cen2018_extract(ex._h, img.ctypes.data, 64, 0, C.byref(p), None, 0.05, out.ctypes.data, None, 10, C.byref(n)) == -1
        assert L.rsx_cen2018_extract_batch_device(ex._h, img.ctypes.data, 0, 512, 64, 0, C.byref(p), None, 0, 0.05, out.ctypes.data, None, 10,
                                                  None, None) == -1
    p = _rsx.Cen2018Params(3.0, 3, 0, 0)
    assert L.rsx_cen2018_extract(ex._h, img.ctypes.data, 63, 0, C.byref(p), None, 0.05, out.ctypes.data, None, 10, C.byref(n)) == -1  # stride
    assert L.rsx_cen2018_extract(ex._h, img.ctypes.data, 64, 0, C.byref(p), None, 0.05, out.ctypes.data, out.ctypes.data, 10, C.byref(n)) == -1  # xy, no az
    assert L.rsx_cen2018_extract(None, img.ctypes.data, 64, 0, C.byref(p), None, 0.05, out.ctypes.data, None, 10, C.byref(n)) == -1
    assert L.rsx_cen2018_extract(ex._h, img.ctypes.data, 64, 0, C.byref(p), None, 0.05, out.ctypes.data, None, 10, C.byref(n)) == 0


def _stream_calls(cen, pool, az, serial):
    """nine rsx_cen2018_extract_batch_device calls on a FRESH handle, consecutive calls with different images and batch sizes and
    every call with its own sentinel-filled outputs: rotating over three streams with no host synchronisation in between
    (serial=False), or on one stream with a synchronise after every call"""
    import torch
    from navtech_radar_slam_amd import _rsx
    ex = cen.Cen2018(400, 3360)
    d_az = torch.from_numpy(az).cuda()
    streams = [torch.cuda.Stream() for _ in range(1 if serial else 3)]
    p = cen.default_params()
    calls = []
    for nb, first in ((4, 0), (2, 3), (3, 1), (1, 4), (4, 1), (2, 0), (5, 2), (1, 3), (3, 4)):
        which = [(first + i) % len(pool) for i in range(nb)]
        imgs = np.ascontiguousarray(pool[which])
        calls.append((which, imgs, torch.from_numpy(imgs).cuda(), torch.full((nb, 20000, 2), -1, dtype=torch.int32, device="cuda"),
                      torch.full((nb,), -1, dtype=torch.int32, device="cuda")))
    torch.cuda.synchronize()
    for r, (which, imgs, d_img, tg, cn) in enumerate(calls):
        s = streams[r % len(streams)]
        _rsx.check(ex._L.rsx_cen2018_extract_batch_device(ex._h, d_img.data_ptr(), len(which), imgs.strides[0], imgs.shape[2], 11, C.byref(p),
                                                           d_az.data_ptr(), 0, synth.RADAR_RESOLUTION, tg.data_ptr(), None, 20000,
                                                           cn.data_ptr(), C.c_void_p(s.cuda_stream)))
        if serial:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    out = [(which, tg.cpu().numpy(), cn.cpu().numpy()) for which, _, _, tg, cn in calls]
    ex.close()
    return out


def test_one_handle_two_streams(cen):
    """the same handle used from several streams back to back: each call ordered behind the other's work.  Nine calls rotate over
    three streams; consecutive calls carry different images and batch sizes (a workspace clobbered by an IDENTICAL call would
    go unseen), every call has its own sentinel-filled outputs, and there is no host synchronisation between the calls.  Byte
    for byte what the same calls give one at a time on a fresh handle, and the host entry's keypoints for every image."""
    pool = np.stack([synth.polar_image(60 + i, n_targets=700 + 100 * i)[0] for i in range(5)])
    az = synth.polar_image(60)[1]
    ex = cen.Cen2018(400, 3360)
    want, _ = ex.extract_batch(pool, azimuths=az, resolution=synth.RADAR_RESOLUTION)
    serial = _stream_calls(cen, pool, az, True)
    got = _stream_calls(cen, pool, az, False)
    for (which, t, c), (_, st, sc) in zip(got, serial):
        assert t.tobytes() == st.tobytes() and c.tobytes() == sc.tobytes()
        for i, w in enumerate(which):
            assert c[i] == len(want[w]) and np.array_equal(t[i, :c[i]], want[w])
            assert (t[i, c[i]:] == -1).all()


def test_create_use_destroy_leaves_device_memory_as_it_was(cen):
    import torch
    imgs, az, _, _ = synth.polar_sequence(23, 3)

    def use():
        c = cen.Cen2018()
        c.extract(imgs[0], azimuths=az[0])
        c.extract_batch(imgs, azimuths=az)
        c.debug_image(imgs[1])
        c.close()
    use()
    use()
    for cycle in range(15):
        use()
        torch.cuda.synchronize()
        free, _ = torch.cuda.mem_get_info(0)
        if cycle == 0:
            first = free
    assert abs(first - free) <= 4 << 20, first - free
