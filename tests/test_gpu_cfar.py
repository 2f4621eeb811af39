"""GPU parity of CA-CFAR / BFAR keypoint extraction (csrc/cfar.hip through the C-ABI) against the restatement of its arithmetic
contract (tests/cfar_np.py).  The rule is integer arithmetic: every comparison is bit equality.  The contract the extractors
share (tests/test_gpu_keypoints_contract.py) is restated for this extractor at the end."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from navtech_radar_slam_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cfar_np as cfn  # noqa: E402
from test_gpu_kstrongest import _padded, _tie_rows  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cf():
    from navtech_radar_slam_amd import cfar
    return cfar


SHAPES = [(1, 1), (7, 2), (5, 3), (5, 4), (7, 30), (5, 43), (5, 44), (5, 45), (5, 67), (401, 30), (1, 4000), (3, 8192)]
# every (t, g) of {(1, 0), (64, 16), (20, 2)}, every mode, A of {0, 255, 256, 1024, 65535}, B of {0, 40, 255}, s of {0, 1, 5, 32},
# k of {1, 12, 128}; None: the defaults (min_range = 58), the others look at the whole row
PARAM_SETS = [None] + [dict(train=t, guard=g, scale_q8=A, offset=B, mode=m, min_separation=s, k=k, min_range=0, max_range=xr)
                       for t, g, A, B, m, s, k, xr in (
    (1, 0, 256, 0, 0, 0, 128, 0), (1, 0, 1024, 0, 1, 32, 12, 0), (1, 0, 255, 40, 2, 1, 1, 0), (1, 0, 0, 0, 0, 5, 12, 0),
    (64, 16, 255, 0, 0, 1, 12, 0), (64, 16, 256, 0, 1, 0, 128, 0), (64, 16, 1024, 40, 2, 5, 12, 0), (64, 16, 65535, 255, 2, 32, 128, 0),
    (64, 16, 65535, 0, 0, 0, 128, 0), (20, 2, 1024, 0, 1, 5, 12, 0), (20, 2, 1024, 40, 2, 5, 1, 0), (20, 2, 0, 40, 0, 0, 12, 0),
    (20, 2, 0, 255, 1, 1, 12, 0), (20, 2, 256, 0, 2, 0, 128, 0), (20, 2, 255, 0, 0, 32, 128, 0), (20, 2, 768, 20, 1, 5, 12, 40),
    (20, 2, 256, 255, 0, 5, 12, 0), (20, 2, 1024, 0, 0, 1, 128, 0), (20, 2, 256, 40, 1, 1, 1, 0), (64, 16, 0, 0, 2, 32, 1, 0))]


def planted(rng, img, cols, reach):
    """strong bins within `reach` (= g + t) of both ends of every row, right beside the 255 bytes outside it"""
    im = img.copy()
    for a in range(im.shape[0]):
        for j in rng.integers(0, reach + 1, size=2):
            im[a, 5 + min(int(j), cols - 1)] = rng.integers(200, 255)
            im[a, 5 + max(cols - 1 - int(j), 0)] = rng.integers(200, 255)
    return im


def odd_shape_cases(rows, cols):
    """-> [(params, image)] of one shape: the padded image with strong bins planted for every parameter set"""
    rng = np.random.default_rng(rows * 10007 + cols)
    img = _padded(rng, rows, cols)
    out = []
    for ps in PARAM_SETS:
        p = dict(ps) if ps else {}
        out.append((p, planted(rng, img, cols, p.get("train", 20) + p.get("guard", 2))))
    return out


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_odd_shapes_row_stride_and_row_ends(cf, rows, cols):
    ex = cf.Cfar(rows, cols)
    most = 0
    for p, im in odd_shape_cases(rows, cols):
        want = cfn.extract(im, col_offset=5, cols=cols, **p)
        got, n = ex.extract(im, col_offset=5, return_count=True, **p)
        assert n == len(want) and np.array_equal(got, want), p
        most = max(most, len(want))
    if cols > 1:
        assert most > 0


def threshold_cases(cols=531):
    """-> [(params, row, tie bins, bins one power level above the threshold)]: 256 n v == A S + 256 B n exactly at the tie bins"""
    base = dict(train=20, guard=2, min_range=0, min_separation=0, k=128)
    special = [63, 64, 65, cols - 1]
    cases = []
    for A, B in ((256, 0), (128, 50), (0, 100)):  # a flat row of 100: a Z + b = 100 everywhere
        for mode in (0, 1, 2):
            flat = np.full(cols, 100, dtype=np.uint8)
            cases.append((dict(base, scale_q8=A, offset=B, mode=mode), flat, special + [0, 1, 30, 300], []))
            up = flat.copy()
            up[special] = 101  # (63, 64, 65 lie inside each other's guard cells: their own noise estimate stays 100)
            cases.append((dict(base, scale_q8=A, offset=B, mode=mode), up, [0, 1, 30, 300], special))
    # two levels, 40 below bin 200 and 120 from it on; the bin under test sits at the edge with 20 cells of each level around it:
    # cell averaging Z = 80, greatest-of Z = 120, smallest-of Z = 40
    for mode, z in ((0, 80), (1, 120), (2, 40)):
        for j in (63, 64, 65):
            for over in (0, 1):
                v = np.full(cols, 40, dtype=np.uint8)
                v[j + 1:] = 120
                v[j] = z + over
                cases.append((dict(base, scale_q8=256, offset=0, mode=mode), v, [] if over else [j], [j] if over else []))
        for over in (0, 1):  # the last bin: no right side at all, every mode falls back on the left one
            v = np.full(cols, 40, dtype=np.uint8)
            v[cols - 1] = 40 + over
            cases.append((dict(base, scale_q8=256, offset=0, mode=mode), v, [] if over else [cols - 1], [cols - 1] if over else []))
    return cases


def check_threshold_case(p, v, ties, overs):
    """the case is what it claims to be (CPU, from the side sums)"""
    SL, nL, SR, nR = cfn.side_sums(v, p["train"], p["guard"])
    for j in ties + overs:
        if p["mode"] == 0 or nL[j] == 0 or nR[j] == 0:
            S, n = SL[j] + SR[j], nL[j] + nR[j]
        else:
            left = (SL[j] * nR[j] >= SR[j] * nL[j]) == (p["mode"] == 1)
            S, n = (SL[j], nL[j]) if left else (SR[j], nR[j])
        lhs, rhs = 256 * n * int(v[j]), p["scale_q8"] * S + 256 * p["offset"] * n
        assert lhs - rhs == (0 if j in ties else 256 * n), (p, j, lhs, rhs)
    det = cfn.detections(v, p["train"], p["guard"], p["scale_q8"], p["offset"], p["mode"])
    assert not det[np.array(ties, dtype=np.int64)].any() and det[np.array(overs, dtype=np.int64)].all()


def test_threshold_ties(cf):
    cases = threshold_cases()
    cols = len(cases[0][1])
    ex = cf.Cfar(1, cols)
    for p, v, ties, overs in cases:
        check_threshold_case(p, v, ties, overs)
        img = np.full((1, 5 + cols + 9), 255, dtype=np.uint8)
        img[0, 5:5 + cols] = v
        want = cfn.extract(img, col_offset=5, cols=cols, **p)
        got = ex.extract(img, col_offset=5, **p)
        assert np.array_equal(got, want), (p, ties, overs)
        assert set(overs) <= set(want[:, 1].tolist()) and not set(ties) & set(want[:, 1].tolist())


@pytest.mark.parametrize("s", [0, 1, 5])
def test_kstrongest_tie_rows_at_scale_zero(cf, s):
    cols = 531
    body = _tie_rows(cols)
    img = np.full((len(body), 5 + cols + 9), 255, dtype=np.uint8)
    img[:, 5:5 + cols] = body
    ex = cf.Cfar(len(body), cols)
    for k in (1, 2, 3, 4, 5, 12, 64, 128):
        for B in (0, 59):
            p = dict(k=k, scale_q8=0, offset=B, min_range=0, min_separation=s)
            want = cfn.extract(img, col_offset=5, cols=cols, **p)
            got = ex.extract(img, col_offset=5, **p)
            assert np.array_equal(got, want), (k, B)


@pytest.fixture(scope="module")
def full_size():
    """(images, azimuths (2, 400), the restatement's keypoints with the defaults and with greatest-of) of two 400 x 3360 scans"""
    one = synth.polar_image(1)
    seq, az, _, _ = synth.polar_sequence(11, 2)
    imgs = np.stack([one[0], seq[0]])
    azs = np.stack([one[1], az[0] if az.ndim == 2 else az]).astype(np.float32)
    return imgs, azs, [cfn.extract(im) for im in imgs], [cfn.extract(im, mode=1) for im in imgs]


def test_full_size_against_restatement(cf, full_size):
    imgs, _, want, want_go = full_size
    ex = cf.Cfar(400, 3360)
    for w, kw in ((want, {}), (want_go, dict(mode=1))):
        tg, cn = ex.extract_batch(imgs, return_counts=True, **kw)
        for i in range(len(imgs)):
            assert cn[i] == len(w[i]) and np.array_equal(tg[i], w[i]), (i, kw)
            assert 0 < len(w[i]) <= 400 * 12


def _device_batch(cf, ex, imgs, az, max_targets, **kw):
    import torch
    from navtech_radar_slam_amd import _rsx
    n = imgs.shape[0]
    d_img = torch.from_numpy(np.ascontiguousarray(imgs)).cuda()
    d_az = torch.from_numpy(np.ascontiguousarray(az, dtype=np.float32)).cuda()
    d_tg = torch.zeros((n, max_targets, 2), dtype=torch.int32, device="cuda")
    d_xy = torch.zeros((n, max_targets, 2), dtype=torch.float32, device="cuda")
    d_cn = torch.zeros(n, dtype=torch.int32, device="cuda")
    p = cf.params(**kw)
    s = torch.cuda.current_stream()
    _rsx.check(ex._L.rsx_cfar_extract_batch_device(ex._h, d_img.data_ptr(), n, imgs.strides[0], imgs.shape[2], 11, C.byref(p), d_az.data_ptr(),
                                                    1 if az.ndim == 2 else 0, synth.RADAR_RESOLUTION, d_tg.data_ptr(), d_xy.data_ptr(), max_targets,
                                                    d_cn.data_ptr(), C.c_void_p(s.cuda_stream)))
    torch.cuda.synchronize()
    cn = d_cn.cpu().numpy()
    k = np.minimum(cn, max_targets)
    tg, xy = d_tg.cpu().numpy(), d_xy.cpu().numpy()
    return [tg[i, :k[i]] for i in range(n)], [xy[i, :k[i]] for i in range(n)], cn


def test_batch_equals_single_and_device_with_per_image_azimuths(cf, full_size, oracle):
    imgs, az, want, _ = full_size
    az = np.stack([az[i] + np.float32(0.01 * i) for i in range(2)]).astype(np.float32)
    ex = cf.Cfar(400, 3360)
    tg, xy = ex.extract_batch(imgs, azimuths=az, resolution=synth.RADAR_RESOLUTION)
    dtg, dxy, _ = _device_batch(cf, ex, imgs, az, 20000)
    for i in range(len(imgs)):
        one, one_xy = ex.extract(imgs[i], azimuths=az[i], resolution=synth.RADAR_RESOLUTION)
        assert np.array_equal(tg[i], want[i])
        assert np.array_equal(one, tg[i]) and np.array_equal(one_xy, xy[i])
        assert np.array_equal(dtg[i], tg[i]) and np.array_equal(dxy[i], xy[i])
        wxy = oracle.cen2019_to_cartesian(tg[i], az[i], synth.RADAR_RESOLUTION)
        assert np.allclose(xy[i], wxy, rtol=1e-5, atol=1e-4)


def test_batch_larger_than_a_sub_batch(cf):
    """300 images of 9 x 500 (> 128, the internal sub-batch), every one against the restatement; a strided batch"""
    rng = np.random.default_rng(77)
    nb, rows, cols = 300, 9, 500
    big = rng.gamma(2.0, 20.0, size=(nb, rows + 1, cols)).clip(0, 255).astype(np.uint8)
    imgs = big[:, :rows]  # image stride = (rows + 1) * cols
    ex = cf.Cfar(rows, cols)
    p = dict(k=5, train=8, guard=1, scale_q8=512, offset=10, mode=1, min_range=3, min_separation=2)
    tg, cn = ex.extract_batch(imgs, col_offset=0, return_counts=True, **p)
    total = 0
    for i in range(nb):
        want = cfn.extract(imgs[i], col_offset=0, **p)
        assert cn[i] == len(want) and np.array_equal(tg[i], want), i
        total += len(want)
    assert total > nb


def test_max_targets_truncation(cf, full_size):
    imgs, az, want, _ = full_size
    img, full = imgs[0], want[0]
    ex = cf.Cfar(400, 3360)
    for mt in (1, len(full) - 1, len(full), len(full) + 10):
        got, n = ex.extract(img, max_targets=mt, return_count=True)
        assert n == len(full) and np.array_equal(got, full[:mt]), mt
    tg, cn = ex.extract_batch(imgs, max_targets=500, return_counts=True)
    assert cn[0] == len(full) and np.array_equal(tg[0], full[:500]) and np.array_equal(tg[1], want[1][:500])
    dtg, _, dcn = _device_batch(cf, ex, imgs, az, 500)
    assert np.array_equal(dcn, cn) and np.array_equal(dtg[0], full[:500]) and np.array_equal(dtg[1], tg[1])


def _stream_calls(cf, pool, az, serial):
    """nine rsx_cfar_extract_batch_device calls on a FRESH handle, consecutive calls with different images and batch sizes and
    every call with its own sentinel-filled outputs: rotating over three streams with no host synchronisation in between
    (serial=False), or on one stream with a synchronise after every call"""
    import torch
    from navtech_radar_slam_amd import _rsx
    ex = cf.Cfar(400, 3360)
    d_az = torch.from_numpy(az).cuda()
    streams = [torch.cuda.Stream() for _ in range(1 if serial else 3)]
    p = cf.default_params()
    calls = []
    for nb, first in ((4, 0), (2, 3), (3, 1), (1, 4), (4, 1), (2, 0), (5, 2), (1, 3), (3, 4)):
        which = [(first + i) % len(pool) for i in range(nb)]
        imgs = np.ascontiguousarray(pool[which])
        calls.append((which, imgs, torch.from_numpy(imgs).cuda(), torch.full((nb, 6000, 2), -1, dtype=torch.int32, device="cuda"),
                      torch.full((nb,), -1, dtype=torch.int32, device="cuda")))
    torch.cuda.synchronize()
    for r, (which, imgs, d_img, tg, cn) in enumerate(calls):
        s = streams[r % len(streams)]
        _rsx.check(ex._L.rsx_cfar_extract_batch_device(ex._h, d_img.data_ptr(), len(which), imgs.strides[0], imgs.shape[2], 11, C.byref(p),
                                                        d_az.data_ptr(), 0, synth.RADAR_RESOLUTION, tg.data_ptr(), None, 6000, cn.data_ptr(),
                                                        C.c_void_p(s.cuda_stream)))
        if serial:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    out = [(which, tg.cpu().numpy(), cn.cpu().numpy()) for which, _, _, tg, cn in calls]
    ex.close()
    return out


def test_one_handle_three_streams(cf):
    """the nine-call pattern of test_gpu_kstrongest.test_one_handle_two_streams: byte for byte the serial run's result, and the
    host entry's keypoints for every image"""
    seq, az, _, _ = synth.polar_sequence(11, 5)
    pool, az = seq, (az[0] if az.ndim == 2 else az).astype(np.float32)
    ex = cf.Cfar(400, 3360)
    want, _ = ex.extract_batch(pool, azimuths=az, resolution=synth.RADAR_RESOLUTION)
    serial = _stream_calls(cf, pool, az, True)
    got = _stream_calls(cf, pool, az, False)
    for (which, t, c), (_, st, sc) in zip(got, serial):
        assert t.tobytes() == st.tobytes() and c.tobytes() == sc.tobytes()
        for i, w in enumerate(which):
            assert 0 < c[i] == len(want[w]) and np.array_equal(t[i, :c[i]], want[w])
            assert (t[i, c[i]:] == -1).all()


def test_create_use_destroy_leaves_device_memory_as_it_was(cf, full_size):
    import torch
    imgs, az, _, _ = full_size

    def use():
        c = cf.Cfar()
        c.extract(imgs[0], azimuths=az[0])
        c.extract_batch(imgs, azimuths=az)
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


# ---- the shared contract of the extractors, restated for this one ----

ROWS, COLS, RES = 8, 64, 0.05
SENTINEL, BAD_ARG = -7, -1
GOOD = dict(k=3, train=4, guard=1, scale_q8=512, offset=30, mode=0, min_range=2, max_range=0, min_separation=2)  # (on the CPU: 14 and 15 keypoints)
# one value outside its limits per parameter (include/rsx.h)
BAD = [dict(k=0), dict(k=129), dict(train=0), dict(train=65), dict(guard=-1), dict(guard=17), dict(scale_q8=-1), dict(scale_q8=65536),
       dict(offset=-1), dict(offset=256), dict(mode=-1), dict(mode=3), dict(min_range=-1), dict(max_range=-1), dict(min_separation=-1),
       dict(min_separation=33), dict(reserved=1)]


def contract_images():
    return np.random.default_rng(1).gamma(2.0, 20.0, size=(2, ROWS, COLS)).clip(0, 255).astype(np.uint8)


def contract_counts():
    return [len(cfn.extract(im, col_offset=0, **GOOD)) for im in contract_images()]


class _Ctx:
    """one 8 x 64 handle, host and device copies of the images and of an azimuth grid, sentinel-filled outputs"""

    def __init__(self, cf):
        import torch
        from navtech_radar_slam_amd import _rsx
        self.L, self.torch = _rsx.lib(), torch
        self.ex = cf.Cfar(ROWS, COLS)
        self.h = self.ex._h
        self.good = cf.params(**GOOD)
        self.p = C.byref(self.good)
        self.imgs = contract_images()
        self.az = np.linspace(0.0, 2.0 * np.pi, ROWS, endpoint=False).astype(np.float32)
        self.tg = np.full((2, 16, 2), SENTINEL, dtype=np.int32)
        self.xy = np.full((2, 16, 2), SENTINEL, dtype=np.float32)
        self.cn = np.full(2, SENTINEL, dtype=np.int32)
        self.d_imgs = torch.from_numpy(self.imgs).cuda()
        self.d_az = torch.from_numpy(self.az).cuda()
        self.d_tg = torch.full((2, 16, 2), SENTINEL, dtype=torch.int32, device="cuda")
        self.d_xy = torch.full((2, 16, 2), SENTINEL, dtype=torch.float32, device="cuda")
        self.d_cn = torch.full((2,), SENTINEL, dtype=torch.int32, device="cuda")

    def _host(self):
        return dict(h=self.h, img=self.imgs.ctypes.data, p=self.p, tg=self.tg.ctypes.data, cn=self.cn.ctypes.data, xy=self.xy.ctypes.data,
                    az=self.az.ctypes.data)

    def single(self, h="h", img="img", row_stride=COLS, p="p", az=None, tg="tg", xy=None, mt=16, cn="cn"):
        a = self._host()
        g = lambda v: a[v] if isinstance(v, str) else v  # noqa: E731
        return self.L.rsx_cfar_extract(g(h), g(img), row_stride, 0, g(p), g(az), RES, g(tg), g(xy), mt, C.cast(g(cn), C.POINTER(C.c_int32)))

    def batch(self, h="h", img="img", n=2, image_stride=ROWS * COLS, row_stride=COLS, p="p", az=None, tg="tg", xy=None, mt=16, cn="cn"):
        a = self._host()
        g = lambda v: a[v] if isinstance(v, str) else v  # noqa: E731
        return self.L.rsx_cfar_extract_batch(g(h), g(img), n, image_stride, row_stride, 0, g(p), g(az), 0, RES, g(tg), g(xy), mt, g(cn))

    def device(self, h="h", img="img", n=2, image_stride=ROWS * COLS, row_stride=COLS, p="p", az=None, tg="tg", xy=None, mt=16, cn="cn"):
        a = dict(h=self.h, img=self.d_imgs.data_ptr(), p=self.p, tg=self.d_tg.data_ptr(), cn=self.d_cn.data_ptr(), xy=self.d_xy.data_ptr(),
                 az=self.d_az.data_ptr())
        g = lambda v: a[v] if isinstance(v, str) else v  # noqa: E731
        st = self.L.rsx_cfar_extract_batch_device(g(h), g(img), n, image_stride, row_stride, 0, g(p), g(az), 0, RES, g(tg), g(xy), mt, g(cn), None)
        self.torch.cuda.synchronize()
        return st

    def untouched(self, targets_only=False):
        host = (self.tg == SENTINEL).all() and (self.xy == SENTINEL).all()
        dev = bool((self.d_tg == SENTINEL).all()) and bool((self.d_xy == SENTINEL).all())
        if not targets_only:
            host = host and (self.cn == SENTINEL).all()
            dev = dev and bool((self.d_cn == SENTINEL).all())
        return bool(host) and dev

    def refill(self):
        for buf in (self.tg, self.cn):
            buf.fill(SENTINEL)
        for buf in (self.d_tg, self.d_cn):
            buf.fill_(SENTINEL)


@pytest.fixture(scope="module")
def ctx(cf):
    c = _Ctx(cf)
    yield c
    c.ex.close()


def test_refused_arguments_write_nothing(ctx):
    x = ctx
    refused = {
        "null handle": (x.single(h=None), x.batch(h=None), x.device(h=None)),
        "null images": (x.single(img=None), x.batch(img=None), x.device(img=None)),
        "null targets": (x.single(tg=None), x.batch(tg=None), x.device(tg=None)),
        "null counts (host)": (x.single(cn=None), x.batch(cn=None)),
        "n_images < 0": (x.batch(n=-1), x.device(n=-1)),
        "row_stride 63": (x.single(row_stride=63), x.batch(row_stride=63), x.device(row_stride=63)),
        "image stride < image": (x.batch(image_stride=ROWS * COLS - 1), x.device(image_stride=ROWS * COLS - 1)),
        "xy without azimuths": (x.single(xy="xy"), x.batch(xy="xy"), x.device(xy="xy")),
        "max_targets 0 (device)": (x.device(mt=0),),
        "max_targets -1 (host)": (x.single(mt=-1), x.batch(mt=-1)),
    }
    for what, statuses in refused.items():
        assert all(st == BAD_ARG for st in statuses), (what, statuses)
    assert x.untouched()
    assert (x.single(), x.batch(), x.device()) == (0, 0, 0)
    assert not x.untouched()
    x.refill()


def test_one_bad_value_per_parameter(ctx, cf):
    from navtech_radar_slam_amd import _rsx
    x = ctx
    for bad in BAD:
        p = cf.params(**GOOD)
        for name, value in bad.items():
            setattr(p, name, value)
        assert x.single(p=C.byref(p)) == BAD_ARG, bad
        assert x.device(n=0, p=C.byref(p)) == BAD_ARG and x.batch(n=0, p=C.byref(p)) == BAD_ARG, bad
        assert isinstance(p, _rsx.CfarParams)
    assert x.untouched()
    # the limits themselves are accepted
    for ok in (dict(k=1), dict(k=128), dict(train=1), dict(train=64), dict(guard=0), dict(guard=16), dict(scale_q8=0), dict(scale_q8=65535),
               dict(offset=0), dict(offset=255), dict(mode=2), dict(min_separation=0), dict(min_separation=32)):
        p = cf.params(**dict(GOOD, **ok))
        assert x.device(n=0, p=C.byref(p)) == 0, ok
    assert x.untouched()


def test_create_refuses_unsupported_shapes(ctx):
    h = C.c_void_p()
    for rows, cols in ((0, COLS), (ROWS, 0), (4097, COLS), (ROWS, 8193)):
        h.value = 1
        assert ctx.L.rsx_cfar_create(0, rows, cols, C.byref(h)) == BAD_ARG and not h.value, (rows, cols)
    assert ctx.L.rsx_cfar_create(0, ROWS, COLS, None) == BAD_ARG


def test_empty_batch(ctx):
    x = ctx
    assert x.batch(n=0) == 0 and x.device(n=0) == 0
    assert x.batch(n=0, az="az", xy="xy") == 0 and x.device(n=0, az="az", xy="xy") == 0
    assert x.untouched()


def test_max_targets_zero_counts_only(ctx):
    x = ctx
    w = contract_counts()
    assert min(w) > 0 and w[0] != w[1]
    for az, xy in ((None, None), ("az", "xy")):
        x.cn.fill(SENTINEL)
        assert x.single(mt=0, az=az, xy=xy) == 0
        assert x.cn[0] == w[0] and x.cn[1] == SENTINEL
        for n in (1, 2):
            x.cn.fill(SENTINEL)
            assert x.batch(n=n, mt=0, az=az, xy=xy) == 0
            assert x.cn[:n].tolist() == w[:n] and (x.cn[n:] == SENTINEL).all(), (n, x.cn, w)
    assert x.untouched(targets_only=True)
    x.cn.fill(SENTINEL)
