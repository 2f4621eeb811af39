"""GPU parity of k-strongest keypoint extraction (csrc/kstrongest.hip through the C-ABI) against the per-row restatement of
its arithmetic contract (tests/kstrongest_np.py).  The rule is integer arithmetic: every comparison is bit equality."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from navtech_radar_slam_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kstrongest_np as ksn  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kst():
    from navtech_radar_slam_amd import kstrongest
    return kstrongest


def _padded(rng, rows, cols, col_offset=5, pad=9, scale=20.0):
    """rows x (col_offset + cols + pad) bytes; metadata and padding are 255, so that a window or a load that strays outside
    the row changes the result"""
    img = np.full((rows, col_offset + cols + pad), 255, dtype=np.uint8)
    img[:, col_offset:col_offset + cols] = rng.gamma(2.0, scale, size=(rows, cols)).clip(0, 254).astype(np.uint8)
    return img


@pytest.mark.parametrize("rows,cols", [(1, 1), (7, 2), (7, 30), (401, 30), (1, 4000), (7, 4000), (3, 8192), (5, 67)])
def test_odd_shapes_row_stride_and_row_ends(kst, rows, cols):
    rng = np.random.default_rng(rows * 10007 + cols)
    img = _padded(rng, rows, cols)
    ex = kst.KStrongest(rows, cols)
    for k, s, z in ((12, 5, 60), (12, 0, 60), (3, 1, 0), (128, 32, 60), (1, 2, 200)):
        im = img.copy()
        for a in range(rows):  # strong bins within s of both ends of the row, right beside the 255 bytes outside it
            for j in rng.integers(0, s + 1, size=2):
                im[a, 5 + min(int(j), cols - 1)] = rng.integers(200, 255)
                im[a, 5 + max(cols - 1 - int(j), 0)] = rng.integers(200, 255)
        want = ksn.extract(im, col_offset=5, cols=cols, k=k, z_min=z, min_range=0, min_separation=s)
        got, n = ex.extract(im, col_offset=5, k=k, z_min=z, min_range=0, min_separation=s, return_count=True)
        assert n == len(want) and np.array_equal(got, want), (k, s, z)
        if rows * cols > 1:
            assert len(want) > 0


@pytest.fixture(scope="module")
def grid_image():
    img, _, _ = synth.polar_image(41, rows=48, n_targets=200)
    return img[:, :11 + 500].copy()


@pytest.mark.parametrize("k", [1, 12, 64, 128])
@pytest.mark.parametrize("s", [0, 1, 5, 32])
@pytest.mark.parametrize("z_min", [0, 60, 255])
def test_parameter_grid(kst, grid_image, k, s, z_min):
    img, cols = grid_image, 500
    ex = kst.KStrongest(48, cols)
    some = 0
    for mr in (0, 58, cols - 1, cols, cols + 5):
        for xr in (0, 100, cols + 7):
            want = ksn.extract(img, k=k, z_min=z_min, min_range=mr, max_range=xr, min_separation=s)
            got = ex.extract(img, k=k, z_min=z_min, min_range=mr, max_range=xr, min_separation=s)
            assert np.array_equal(got, want), (mr, xr)
            some += len(want)
    assert some > 0 or z_min == 255


def _tie_rows(cols):
    rng = np.random.default_rng(9)
    rows = [np.zeros(cols), np.full(cols, 200), np.full(cols, 255)]
    rows.append(rng.choice([100, 180], size=cols, p=[0.6, 0.4]))   # two levels: the top one holds far more than k
    rows.append(rng.choice([100, 180], size=cols, p=[0.98, 0.02]))  # ... the top one fewer than k, the threshold level the rest
    rows.append(rng.choice([59, 60], size=cols))                   # two levels around the floor
    for step in (4, 16):  # threshold-level ties at multiples of 4 and 16 bins, a few stronger bins above them
        v = np.full(cols, 70)
        v[::step] = 150
        v[rng.choice(np.arange(0, cols, step), size=5, replace=False)] = 250
        rows.append(v)
    v = np.full(cols, 70)  # ties at bins 63 / 64 / 65 (two lanes, two chunks of 64 bins) and at the last bin
    v[[63, 64, 65, cols - 1]] = 150
    v[[10, 300]] = 250
    rows.append(v)
    v = np.full(cols, 70)  # the same, spaced for a separation of 1: 63, 65 and the last bin, against 61 and 67
    v[[61, 63, 65, 67, cols - 1]] = 150
    rows.append(v)
    v = np.full(cols, 10)  # fewer than k candidates
    v[[7, 99, 256, 257, cols - 2]] = 100
    rows.append(v)
    rows.append(np.full(cols, 10))  # none above the floor
    v = np.arange(cols) % 256  # every bin beaten by its right neighbour, except at the wrap
    rows.append(v)
    return np.stack(rows).astype(np.uint8)


@pytest.mark.parametrize("s", [0, 1, 5])
def test_ties(kst, s):
    cols = 531
    body = _tie_rows(cols)
    img = np.full((len(body), 5 + cols + 9), 255, dtype=np.uint8)
    img[:, 5:5 + cols] = body
    ex = kst.KStrongest(len(body), cols)
    for k in (1, 2, 3, 4, 5, 12, 64, 128):
        for z in (0, 60):
            want = ksn.extract(img, col_offset=5, cols=cols, k=k, z_min=z, min_range=0, min_separation=s)
            got = ex.extract(img, col_offset=5, k=k, z_min=z, min_range=0, min_separation=s)
            assert np.array_equal(got, want), (k, z, [a for a in range(len(body)) if not np.array_equal(got[got[:, 0] == a], want[want[:, 0] == a])])


@pytest.fixture(scope="module")
def full_size():
    """(images, azimuths (n, 400), the restatement's keypoints with the defaults) of seven 400 x 3360 scans"""
    singles = [synth.polar_image(seed, n_targets=800 + 200 * seed) for seed in (1, 2, 3)]
    seq, az, _, _ = synth.polar_sequence(11, 4)
    imgs = np.concatenate([np.stack([s[0] for s in singles]), seq])
    azs = np.concatenate([np.stack([s[1] for s in singles]), az if az.ndim == 2 else np.tile(az, (len(seq), 1))]).astype(np.float32)
    return imgs, azs, [ksn.extract(im) for im in imgs]


def test_mulran_shape_against_restatement(kst, full_size):
    imgs, _, want = full_size
    ex = kst.KStrongest(400, 3360)
    tg, cn = ex.extract_batch(imgs, return_counts=True)
    for i in range(len(imgs)):
        assert cn[i] == len(want[i]) and np.array_equal(tg[i], want[i]), i
        assert 1000 < len(want[i]) <= 400 * 12


def _device_batch(kst, ex, imgs, az, max_targets, **kw):
    import torch
    from navtech_radar_slam_amd import _rsx
    n = imgs.shape[0]
    d_img = torch.from_numpy(np.ascontiguousarray(imgs)).cuda()
    d_az = torch.from_numpy(np.ascontiguousarray(az, dtype=np.float32)).cuda()
    d_tg = torch.zeros((n, max_targets, 2), dtype=torch.int32, device="cuda")
    d_xy = torch.zeros((n, max_targets, 2), dtype=torch.float32, device="cuda")
    d_cn = torch.zeros(n, dtype=torch.int32, device="cuda")
    p = kst.params(**kw)
    s = torch.cuda.current_stream()
    _rsx.check(ex._L.rsx_kstrongest_extract_batch_device(ex._h, d_img.data_ptr(), n, imgs.strides[0], imgs.shape[2], 11, C.byref(p),
                                                          d_az.data_ptr(), 1 if az.ndim == 2 else 0, synth.RADAR_RESOLUTION, d_tg.data_ptr(),
                                                          d_xy.data_ptr(), max_targets, d_cn.data_ptr(), C.c_void_p(s.cuda_stream)))
    torch.cuda.synchronize()
    cn = d_cn.cpu().numpy()
    k = np.minimum(cn, max_targets)
    tg, xy = d_tg.cpu().numpy(), d_xy.cpu().numpy()
    return [tg[i, :k[i]] for i in range(n)], [xy[i, :k[i]] for i in range(n)], cn


def test_batch_equals_single_and_device_with_per_image_azimuths(kst, full_size, oracle):
    imgs, az, want = full_size
    imgs, want = imgs[:5], want[:5]
    az = np.stack([az[i] + np.float32(0.01 * i) for i in range(5)]).astype(np.float32)
    ex = kst.KStrongest(400, 3360)
    tg, xy = ex.extract_batch(imgs, azimuths=az, resolution=synth.RADAR_RESOLUTION)
    dtg, dxy, _ = _device_batch(kst, ex, imgs, az, 20000)
    for i in range(len(imgs)):
        one, one_xy = ex.extract(imgs[i], azimuths=az[i], resolution=synth.RADAR_RESOLUTION)
        assert np.array_equal(tg[i], want[i])
        assert np.array_equal(one, tg[i]) and np.array_equal(one_xy, xy[i])
        assert np.array_equal(dtg[i], tg[i]) and np.array_equal(dxy[i], xy[i])
        wxy = oracle.cen2019_to_cartesian(tg[i], az[i], synth.RADAR_RESOLUTION)
        assert np.allclose(xy[i], wxy, rtol=1e-5, atol=1e-4)


def test_batch_larger_than_a_sub_batch(kst):
    """300 images of 9 x 500 (> 128, the internal sub-batch), every one against the restatement; a strided batch"""
    rng = np.random.default_rng(77)
    nb, rows, cols = 300, 9, 500
    big = rng.gamma(2.0, 20.0, size=(nb, rows + 1, cols)).clip(0, 255).astype(np.uint8)
    imgs = big[:, :rows]  # image stride = (rows + 1) * cols
    ex = kst.KStrongest(rows, cols)
    tg, cn = ex.extract_batch(imgs, col_offset=0, k=5, z_min=70, min_range=3, min_separation=2, return_counts=True)
    for i in range(nb):
        want = ksn.extract(imgs[i], col_offset=0, k=5, z_min=70, min_range=3, min_separation=2)
        assert cn[i] == len(want) and np.array_equal(tg[i], want), i


def test_max_targets_truncation(kst, full_size):
    imgs, az, want = full_size
    img, full = imgs[0], want[0]
    ex = kst.KStrongest(400, 3360)
    for mt in (1, len(full) - 1, len(full), len(full) + 10):
        got, n = ex.extract(img, max_targets=mt, return_count=True)
        assert n == len(full) and np.array_equal(got, full[:mt]), mt
    tg, cn = ex.extract_batch(imgs[:2], max_targets=500, return_counts=True)
    assert cn[0] == len(full) and np.array_equal(tg[0], full[:500]) and np.array_equal(tg[1], want[1][:500])
    dtg, _, dcn = _device_batch(kst, ex, imgs[:2], az[:2], 500)
    assert np.array_equal(dcn, cn) and np.array_equal(dtg[0], full[:500]) and np.array_equal(dtg[1], tg[1])


def test_bad_arguments(kst):
    from navtech_radar_slam_amd import _rsx
    L = _rsx.lib()
    h = C.c_void_p()
    for rows, cols in ((0, 100), (10, 0), (5000, 10), (10, 9000)):
        h.value = 1
        assert L.rsx_kstrongest_create(0, rows, cols, C.byref(h)) == -1 and not h.value
    ex = kst.KStrongest(8, 64)
    img = np.zeros((8, 64), dtype=np.uint8)
    out = np.zeros((10, 2), dtype=np.int32)
    n = C.c_int32()
    # (k, z_min, min_range, max_range, min_separation)
    for bad in ((0, 60, 0, 0, 5), (-1, 60, 0, 0, 5), (129, 60, 0, 0, 5), (12, -1, 0, 0, 5), (12, 256, 0, 0, 5), (12, 60, -1, 0, 5),
                (12, 60, 0, -1, 5), (12, 60, 0, 0, -1), (12, 60, 0, 0, 33)):
        p = _rsx.KStrongestParams(*bad, 0)
        assert L.rsx_kstrongest_extract(ex._h, img.ctypes.data, 64, 0, C.byref(p), None, 0.05, out.ctypes.data, None, 10, C.byref(n)) == -1, bad
        assert L.rsx_kstrongest_extract_batch_device(ex._h, img.ctypes.data, 0, 512, 64, 0, C.byref(p), None, 0, 0.05, out.ctypes.data, None, 10,
                                                     None, None) == -1, bad
    p = _rsx.KStrongestParams(12, 60, 0, 0, 5, 0)
    assert L.rsx_kstrongest_extract(ex._h, img.ctypes.data, 63, 0, C.byref(p), None, 0.05, out.ctypes.data, None, 10, C.byref(n)) == -1  # stride
    assert L.rsx_kstrongest_extract(ex._h, img.ctypes.data, 64, 0, C.byref(p), None, 0.05, out.ctypes.data, out.ctypes.data, 10, C.byref(n)) == -1  # xy, no az
    assert L.rsx_kstrongest_extract(None, img.ctypes.data, 64, 0, C.byref(p), None, 0.05, out.ctypes.data, None, 10, C.byref(n)) == -1
    assert L.rsx_kstrongest_extract(ex._h, img.ctypes.data, 64, 0, C.byref(p), None, 0.05, out.ctypes.data, None, 10, C.byref(n)) == 0
    d = kst.default_params()
    assert (d.k, d.z_min, d.min_range, d.max_range, d.min_separation, d.reserved) == (12, 60, 58, 0, 5, 0)


def _stream_calls(kst, pool, az, serial):
    """nine rsx_kstrongest_extract_batch_device calls on a FRESH handle, consecutive calls with different images and batch sizes
    and every call with its own sentinel-filled outputs: rotating over three streams with no host synchronisation in between
    (serial=False), or on one stream with a synchronise after every call"""
    import torch
    from navtech_radar_slam_amd import _rsx
    ex = kst.KStrongest(400, 3360)
    d_az = torch.from_numpy(az).cuda()
    streams = [torch.cuda.Stream() for _ in range(1 if serial else 3)]
    p = kst.default_params()
    calls = []
    for nb, first in ((4, 0), (2, 3), (3, 1), (1, 4), (4, 1), (2, 0), (5, 2), (1, 3), (3, 4)):
        which = [(first + i) % len(pool) for i in range(nb)]
        imgs = np.ascontiguousarray(pool[which])
        calls.append((which, imgs, torch.from_numpy(imgs).cuda(), torch.full((nb, 6000, 2), -1, dtype=torch.int32, device="cuda"),
                      torch.full((nb,), -1, dtype=torch.int32, device="cuda")))
    torch.cuda.synchronize()
    for r, (which, imgs, d_img, tg, cn) in enumerate(calls):
        s = streams[r % len(streams)]
        _rsx.check(ex._L.rsx_kstrongest_extract_batch_device(ex._h, d_img.data_ptr(), len(which), imgs.strides[0], imgs.shape[2], 11, C.byref(p),
                                                              d_az.data_ptr(), 0, synth.RADAR_RESOLUTION, tg.data_ptr(), None, 6000,
                                                              cn.data_ptr(), C.c_void_p(s.cuda_stream)))
        if serial:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    out = [(which, tg.cpu().numpy(), cn.cpu().numpy()) for which, _, _, tg, cn in calls]
    ex.close()
    return out


def test_one_handle_two_streams(kst, full_size):
    """the same handle used from several streams back to back: each call ordered behind the other's work.  Nine calls rotate over
    three streams; consecutive calls carry different images and batch sizes (a workspace clobbered by an IDENTICAL call would
    go unseen), every call has its own sentinel-filled outputs, and there is no host synchronisation between the calls.  Byte
    for byte what the same calls give one at a time on a fresh handle, and the host entry's keypoints for every image."""
    imgs, azs, _ = full_size
    pool, az = imgs[:5], azs[0]
    ex = kst.KStrongest(400, 3360)
    want, _ = ex.extract_batch(pool, azimuths=az, resolution=synth.RADAR_RESOLUTION)
    serial = _stream_calls(kst, pool, az, True)
    got = _stream_calls(kst, pool, az, False)
    for (which, t, c), (_, st, sc) in zip(got, serial):
        assert t.tobytes() == st.tobytes() and c.tobytes() == sc.tobytes()
        for i, w in enumerate(which):
            assert c[i] == len(want[w]) and np.array_equal(t[i, :c[i]], want[w])
            assert (t[i, c[i]:] == -1).all()


def test_create_use_destroy_leaves_device_memory_as_it_was(kst, full_size):
    import torch
    imgs, az, _ = full_size

    def use():
        c = kst.KStrongest()
        c.extract(imgs[0], azimuths=az[0])
        c.extract_batch(imgs[:3], azimuths=az[:3])
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
