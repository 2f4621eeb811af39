"""The contract the three keypoint extractors share (the scaffold of csrc/keypoints_host.h behind rsx_cen2018_*, rsx_cen2019_* and
rsx_kstrongest_*): which arguments are refused -- with nothing written --, what an empty batch does, and max_targets = 0 on the
host entries (counts only).  Expected statuses are the contract of include/rsx.h; expected counts come from the CPU restatements
(tests/cen2018_np.py, tests/kstrongest_np.py, the oracle's cen2019), never from another entry of the library."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cen2018_np as c18  # noqa: E402
import kstrongest_np as ksn  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS, COLS, RES = 8, 64, 0.05
SEED = 1        # (checked on the CPU: cen2018_np.fragile_rows is empty for both images; the counts are 15 12, 31 24 and 20 23)
SENTINEL = -7   # what the output buffers hold before a call
BAD_ARG = -1    # RSX_ERR_BAD_ARG
NAMES = ("cen2018", "cen2019", "kstrongest")
C18 = dict(zq=2.0, sigma_gauss=3, min_range=2)
C19 = dict(max_points=40, min_range=2)
KST = dict(k=3, z_min=90, min_range=2, max_range=0, min_separation=2)
# shapes no extractor takes, and one past each extractor's own limits (cen2019: rows <= 1024, 2 <= cols <= 16384; the others: 4096 x 8192)
BAD_SHAPES = {"cen2018": ((0, COLS), (ROWS, 0), (4097, COLS), (ROWS, 8193)), "cen2019": ((0, COLS), (ROWS, 1), (1025, COLS), (ROWS, 16385)),
              "kstrongest": ((0, COLS), (ROWS, 0), (4097, COLS), (ROWS, 8193))}


def images():
    """two ROWS x COLS images without metadata bytes (col_offset = 0), contiguous"""
    rng = np.random.default_rng(SEED)
    return rng.gamma(2.0, 20.0, size=(2, ROWS, COLS)).clip(0, 255).astype(np.uint8)


def expected_counts(name, imgs, oracle):
    """keypoints of every image by the extractor's CPU restatement (cen2018: also that no decision hangs on the last bit of an exp)"""
    if name == "cen2018":
        out = []
        for im in imgs:
            tg, dbg = c18.extract(im, col_offset=0, debug=True, **C18)
            assert len(c18.fragile_rows(dbg, C18["min_range"])) == 0
            out.append(len(tg))
        return out
    if name == "kstrongest":
        return [len(ksn.extract(im, col_offset=0, **KST)) for im in imgs]
    return [len(oracle.cen2019_extract(im, col_offset=0, **C19)) for im in imgs]


def good_params(name):
    from navtech_radar_slam_amd import _rsx
    return {"cen2018": lambda: _rsx.Cen2018Params(C18["zq"], C18["sigma_gauss"], C18["min_range"], 0),
            "cen2019": lambda: _rsx.Cen2019Params(C19["max_points"], C19["min_range"]),
            "kstrongest": lambda: _rsx.KStrongestParams(KST["k"], KST["z_min"], KST["min_range"], KST["max_range"], KST["min_separation"], 0)}[name]()


def bad_params(name):
    """values outside what include/rsx.h allows (cen2019 documents no limits and checks none)"""
    from navtech_radar_slam_amd import _rsx
    return {"cen2018": lambda: _rsx.Cen2018Params(2.0, 4, 2, 0), "cen2019": lambda: _rsx.Cen2019Params(-1, -1),
            "kstrongest": lambda: _rsx.KStrongestParams(0, 90, 2, 0, 2, 0)}[name]()


@pytest.fixture(scope="module")
def want(oracle):
    imgs = images()
    return {name: expected_counts(name, imgs, oracle) for name in NAMES}


class _Ctx:
    """one 8 x 64 handle of an extractor, host and device copies of the images and of an azimuth grid, sentinel-filled outputs"""

    def __init__(self, name):
        import torch
        from navtech_radar_slam_amd import _rsx, cen2018, cen2019, kstrongest
        self.name, self.L = name, _rsx.lib()
        self.ex = {"cen2018": cen2018.Cen2018, "cen2019": cen2019.Cen2019, "kstrongest": kstrongest.KStrongest}[name](ROWS, COLS)
        self.h = self.ex._h
        self.p = C.byref(good_params(name))
        self.bad_p = C.byref(bad_params(name))
        self.imgs = images()
        self.az = np.linspace(0.0, 2.0 * np.pi, ROWS, endpoint=False).astype(np.float32)
        self.tg = np.full((2, 16, 2), SENTINEL, dtype=np.int32)
        self.xy = np.full((2, 16, 2), SENTINEL, dtype=np.float32)
        self.cn = np.full(2, SENTINEL, dtype=np.int32)
        self.d_imgs = torch.from_numpy(self.imgs).cuda()
        self.d_az = torch.from_numpy(self.az).cuda()
        self.d_tg = torch.full((2, 16, 2), SENTINEL, dtype=torch.int32, device="cuda")
        self.d_xy = torch.full((2, 16, 2), SENTINEL, dtype=torch.float32, device="cuda")
        self.d_cn = torch.full((2,), SENTINEL, dtype=torch.int32, device="cuda")
        self.torch = torch

    def fn(self, entry):
        return getattr(self.L, "rsx_%s_%s" % (self.name, entry))

    # the three entries with every argument valid unless replaced (max_targets 16, 2 images, no xy)
    def single(self, h="h", img="img", row_stride=COLS, p="p", az=None, tg="tg", xy=None, mt=16, cn="cn"):
        a = dict(h=self.h, img=self.imgs.ctypes.data, p=self.p, tg=self.tg.ctypes.data, cn=self.cn.ctypes.data, xy=self.xy.ctypes.data, az=self.az.ctypes.data)
        g = lambda v: a[v] if isinstance(v, str) else v  # noqa: E731
        return self.fn("extract")(g(h), g(img), row_stride, 0, g(p), g(az), RES, g(tg), g(xy), mt, C.cast(g(cn), C.POINTER(C.c_int32)))

    def batch(self, h="h", img="img", n=2, image_stride=ROWS * COLS, row_stride=COLS, p="p", az=None, tg="tg", xy=None, mt=16, cn="cn"):
        a = dict(h=self.h, img=self.imgs.ctypes.data, p=self.p, bad_p=self.bad_p, tg=self.tg.ctypes.data, cn=self.cn.ctypes.data, xy=self.xy.ctypes.data,
                 az=self.az.ctypes.data)
        g = lambda v: a[v] if isinstance(v, str) else v  # noqa: E731
        return self.fn("extract_batch")(g(h), g(img), n, image_stride, row_stride, 0, g(p), g(az), 0, RES, g(tg), g(xy), mt, g(cn))

    def device(self, h="h", img="img", n=2, image_stride=ROWS * COLS, row_stride=COLS, p="p", az=None, tg="tg", xy=None, mt=16, cn="cn"):
        a = dict(h=self.h, img=self.d_imgs.data_ptr(), p=self.p, bad_p=self.bad_p, tg=self.d_tg.data_ptr(), cn=self.d_cn.data_ptr(), xy=self.d_xy.data_ptr(),
                 az=self.d_az.data_ptr())
        g = lambda v: a[v] if isinstance(v, str) else v  # noqa: E731
        st = self.fn("extract_batch_device")(g(h), g(img), n, image_stride, row_stride, 0, g(p), g(az), 0, RES, g(tg), g(xy), mt, g(cn), None)
        self.torch.cuda.synchronize()
        return st

    def untouched(self, targets_only=False):
        host = (self.tg == SENTINEL).all() and (self.xy == SENTINEL).all()
        dev = bool((self.d_tg == SENTINEL).all()) and bool((self.d_xy == SENTINEL).all())
        if not targets_only:
            host = host and (self.cn == SENTINEL).all()
            dev = dev and bool((self.d_cn == SENTINEL).all())
        return bool(host) and dev


@pytest.fixture(scope="module", params=NAMES)
def ctx(request):
    c = _Ctx(request.param)
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
    # every argument valid: the same calls succeed (the refusals above are about the one argument replaced)
    assert (x.single(), x.batch(), x.device()) == (0, 0, 0)
    assert not x.untouched()
    for buf in (x.tg, x.cn):
        buf.fill(SENTINEL)
    for buf in (x.d_tg, x.d_cn):
        buf.fill_(SENTINEL)


def test_create_refuses_unsupported_shapes(ctx):
    h = C.c_void_p()
    for rows, cols in BAD_SHAPES[ctx.name]:
        h.value = 1
        assert ctx.fn("create")(0, rows, cols, C.byref(h)) == BAD_ARG and not h.value, (rows, cols)
    assert ctx.fn("create")(0, ROWS, COLS, None) == BAD_ARG


def test_empty_batch(ctx):
    x = ctx
    assert x.batch(n=0) == 0 and x.device(n=0) == 0
    assert x.batch(n=0, az="az", xy="xy") == 0 and x.device(n=0, az="az", xy="xy") == 0
    # parameters are checked before the batch size: cen2018 and k-strongest refuse theirs, cen2019 has none to refuse
    bad = 0 if x.name == "cen2019" else BAD_ARG
    assert x.batch(n=0, p="bad_p") == bad and x.device(n=0, p="bad_p") == bad
    assert x.untouched()


def test_max_targets_zero_counts_only(ctx, want):
    x = ctx
    w = want[x.name]
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
