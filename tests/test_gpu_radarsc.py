"""GPU tests of the radar scan-context builder (csrc/radarsc.hip, rsx_radarsc_*) against its restatement tests/radarsc_np.py
(PARITY with MulRan's own builder UNPINNED).  The sums are integers, so the contract is BIT IDENTITY: every comparison below
is on the bytes of the descriptors.  Shapes are the smallest at which the kernel can go wrong: rows that start at every
alignment (row_stride 315, col_offset 11), rings narrower and wider than a 16-byte piece, rings that end inside the row or
lie beyond it, sectors with no row and with more rows than one staging pass holds, image pointers at every offset mod 4 and
batches of more work items than the grid has workgroups."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import radarsc_np as rc  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS, COLS, OFF, STRIDE = 37, 301, 11, 313 + 2
SMALL = dict(resolution=0.25, max_radius=80.0, min_range=5)   # 320 bins to 80 m: ring 18 is cut by the image, ring 19 lies beyond it


@pytest.fixture(scope="module")
def mod():
    from navtech_radar_slam_amd import _rsx, radar_context
    assert _rsx.device_count() >= 1, "no HIP device: GPU tests must run on the MI355X box"
    return radar_context


def images(seed, n, rows=ROWS, stride=STRIDE):
    return np.random.default_rng(seed).integers(0, 256, (n, rows, stride), dtype=np.uint8)


def grids(rows=ROWS):
    """name -> (rows,) float32: the kinds of grid the rule must take"""
    step = 2 * np.pi / rows
    a = np.arange(rows)
    g = {
        "plain": a * step,
        "wraps": 5.9 + a * step,                        # starts at 5.9 rad and passes 2 pi
        "negative": -3.0 + a * step,
        "far": 40.0 + a * (3 * step),                   # > 2 pi, three turns
        "shuffled": np.random.default_rng(1).permutation(a) * step,   # non-monotone
        "one_sector": 1.0 + a * 1e-4,                   # every row in one sector: several staging passes
    }
    g = {k: v.astype(np.float32) for k, v in g.items()}
    nan = g["plain"].copy()
    nan[[0, 5, rows - 1]] = [np.nan, np.inf, -np.inf]   # rows without a sector
    g["nan"] = nan
    return g


def want_batch(imgs, az, cols=COLS, off=OFF, **kw):
    return rc.build_batch(imgs, az, col_offset=off, cols=cols, **kw)


def device_build(ctx, imgs, az, off=OFF, base_offset=0, stream=0, guard=64):
    """imgs (n, rows, stride) uint8 -> descriptors through rsx_radarsc_build_batch_device.  The images sit base_offset bytes
    into a larger allocation (its other bytes 0xff), the output is pre-filled with a sentinel and followed by a guard."""
    import torch
    n = imgs.shape[0]
    az = np.ascontiguousarray(az, dtype=np.float32)
    buf = torch.full((imgs.size + 32,), 255, dtype=torch.uint8, device="cuda")
    if n:
        buf[base_offset:base_offset + imgs.size] = torch.from_numpy(np.ascontiguousarray(imgs).reshape(-1)).cuda()
    daz = torch.from_numpy(az).cuda()
    out = torch.full((n * 1200 + guard,), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.build_batch_device(buf.data_ptr() + base_offset, n, imgs.shape[1] * imgs.shape[2], imgs.shape[2], daz.data_ptr(), out.data_ptr(),
                           col_offset=off, azimuths_per_image=az.ndim == 2, stream=stream)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.all(got[n * 1200:] == -7.0), "wrote past the last descriptor"
    return got[:n * 1200].reshape(n, 1200)


def same(got, want):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (bad[:8], got.reshape(-1)[bad[:8]], want.reshape(-1)[bad[:8]])


@pytest.mark.parametrize("stat", [rc.MEAN, rc.MAX])
@pytest.mark.parametrize("floor", [0, 40, 255])
def test_every_grid_kind_per_image_grids(mod, stat, floor):
    g = grids()
    imgs = images(1, len(g))
    az = np.stack(list(g.values()))
    kw = dict(SMALL, power_floor=floor, stat=stat)
    ctx = mod.RadarContext(ROWS, COLS, **kw)
    want = want_batch(imgs, az, **kw)
    if floor < 255:
        assert np.count_nonzero(want) > 1000
    same(device_build(ctx, imgs, az), want)
    same(ctx.build_batch(imgs, az, col_offset=OFF), want)              # the host entry
    for name, grid in g.items():                                      # one shared grid for the whole batch
        same(device_build(ctx, imgs[:2], grid), want_batch(imgs[:2], grid, **kw))


@pytest.mark.parametrize("base_offset", [0, 1, 2, 3])
def test_image_pointer_at_every_offset(mod, base_offset):
    """The first and the last 16-byte piece of an image may stick out of it: only the bytes inside are read.  min_range 0 and
    col_offset 0 put ring bins on the image's first bytes, a row_stride of exactly cols on its last."""
    kw = dict(resolution=0.25, max_radius=80.0, min_range=0)
    imgs = images(2, 3, stride=COLS)
    az = grids()["wraps"]
    ctx = mod.RadarContext(ROWS, COLS, **kw)
    same(device_build(ctx, imgs, az, off=0, base_offset=base_offset), want_batch(imgs, az, off=0, **kw))
    imgs = images(3, 2)
    ctx2 = mod.RadarContext(ROWS, COLS, **SMALL)
    same(device_build(ctx2, imgs, az, base_offset=base_offset), want_batch(imgs, az, **SMALL))


@pytest.mark.parametrize("n", [0, 1, 3, 65])
def test_batch_sizes(mod, n):
    """65 images = 3900 (image, sector) items on a grid of 2048 workgroups: the grid-stride loop"""
    imgs = images(4, n)
    az = np.stack([grids()["wraps"] + np.float32(0.01 * i) for i in range(n)]) if n else np.zeros((0, ROWS), np.float32)
    ctx = mod.RadarContext(ROWS, COLS, **SMALL)
    want = want_batch(imgs, az, **SMALL)
    assert want.shape == (n, 1200)
    same(device_build(ctx, imgs, az), want)
    same(ctx.build_batch(imgs, az, col_offset=OFF), want)


def test_host_entry_sub_batches_and_image_stride(mod):
    """130 images (two staging sub-batches) taken from every second image of a larger array"""
    big = images(5, 260, rows=7, stride=40)
    imgs = big[::2]
    az = grids(7)["wraps"]
    kw = dict(resolution=1.0, max_radius=20.0, min_range=2)
    ctx = mod.RadarContext(7, 29, **kw)
    same(ctx.build_batch(imgs, az, col_offset=OFF), want_batch(np.ascontiguousarray(imgs), az, cols=29, **kw))


@pytest.mark.parametrize("stat", [rc.MEAN, rc.MAX])
def test_seven_rows_most_sectors_empty(mod, stat):
    imgs = images(6, 3, rows=7)
    az = grids(7)["wraps"]
    kw = dict(SMALL, stat=stat)
    want = want_batch(imgs, az, **kw)
    assert np.count_nonzero(want.reshape(3, 60, 20).any(axis=2)) == 3 * 7
    same(device_build(mod.RadarContext(7, COLS, **kw), imgs, az), want)


@pytest.mark.parametrize("stat", [rc.MEAN, rc.MAX])
@pytest.mark.parametrize("kw", [dict(resolution=0.25, max_radius=20.0, min_range=5),      # rings end mid-row (bin 80), 4 bins wide
                                dict(resolution=0.25, max_radius=500.0, min_range=5),     # rings 4 .. 19 lie beyond the image: 0
                                dict(resolution=0.25, max_radius=2.0, min_range=0),       # 8 bins in all: rings without a bin
                                dict(resolution=0.0595, max_radius=80.0, min_range=COLS),   # min_range >= cols: nothing
                                dict(resolution=0.0595, max_radius=80.0, min_range=COLS + 9)])
def test_ring_limits(mod, kw, stat):
    imgs = images(7, 2)
    az = grids()["plain"]
    kw = dict(kw, stat=stat, power_floor=3)
    want = want_batch(imgs, az, **kw)
    if kw["max_radius"] == 500.0:
        w = want.reshape(2, 60, 20)[:, np.unique(rc.sector_of_rows(az))]    # the sectors that have a row
        assert want.reshape(2, 60, 20)[:, :, 4:].max() == 0 and w[:, :, :4].min() > 0
    if kw["min_range"] >= COLS:
        assert not want.any()
    same(device_build(mod.RadarContext(ROWS, COLS, **kw), imgs, az), want)


@pytest.mark.parametrize("stat", [rc.MEAN, rc.MAX])
@pytest.mark.parametrize("grid", ["one_sector", "thirds", "plain"])
def test_one_ring_bin_per_row(mod, stat, grid):
    """min_range = cols - 1 leaves ONE bin with a ring: one 16-byte piece per row, where the row / piece split of the staging
    loop is a division by one.  Every row in one sector (several passes), three rows per sector and one row per sector; and the
    one-column image."""
    az = grids()[grid] if grid != "thirds" else ((np.arange(ROWS) // 3) * (2 * np.pi / 13) + 0.01).astype(np.float32)
    if grid == "thirds":
        assert np.bincount(rc.sector_of_rows(az)).max() == 3
    imgs = images(9, 3)
    kw = dict(resolution=0.25, max_radius=80.0, min_range=COLS - 1, stat=stat, power_floor=2)
    want = want_batch(imgs, az, **kw)
    assert np.count_nonzero(want.reshape(3, 60, 20).any(axis=1)) == 3          # one ring only
    same(device_build(mod.RadarContext(ROWS, COLS, **kw), imgs, az), want)
    one = images(10, 2, stride=1)
    kw1 = dict(resolution=0.25, max_radius=80.0, min_range=0, stat=stat)
    same(device_build(mod.RadarContext(ROWS, 1, **kw1), one, az, off=0), want_batch(one, az, cols=1, off=0, **kw1))


@pytest.mark.parametrize("stat", [rc.MEAN, rc.MAX])
@pytest.mark.parametrize("floor", [0, 40, 255])
def test_constant_images(mod, stat, floor):
    imgs = np.stack([np.zeros((ROWS, STRIDE), np.uint8), np.full((ROWS, STRIDE), 255, np.uint8)])
    az = grids()["plain"]
    kw = dict(SMALL, power_floor=floor, stat=stat)
    want = want_batch(imgs, az, **kw)
    assert not want[0].any() and set(np.unique(want[1])) <= {0.0, float(255 - floor)}
    same(device_build(mod.RadarContext(ROWS, COLS, **kw), imgs, az), want)


@pytest.mark.parametrize("stat", [rc.MEAN, rc.MAX])
def test_mulran_shape_once(mod, stat):
    """400 x 3360 scans in Oxford form (rows 3371 bytes apart, samples 11 bytes in) with the default parameters, the second
    with its own grid"""
    from navtech_radar_slam_amd import synth
    a, az, _ = synth.polar_image(100)
    b, _, _ = synth.polar_image(104, shift_rows=20, noise_seed=900)
    imgs = np.stack([a, b])
    grid = np.stack([az, (az + np.float32(5.9)).astype(np.float32)])
    kw = dict(power_floor=40 if stat == rc.MEAN else 0, stat=stat)
    want = rc.build_batch(imgs, grid, **kw)
    same(device_build(mod.RadarContext(400, 3360, **kw), imgs, grid), want)


def test_a_cell_sum_past_32_bits(mod):
    """Every row in one sector and every bin in one ring: the cell's sum is 4096 x 4400 x ~255 > 2^32"""
    rows, cols = 4096, 4400
    img = np.full((1, rows, cols), 255, np.uint8)
    img[0, ::7, ::5] = 250
    az = np.full(rows, 1.0, np.float32)
    kw = dict(resolution=0.001, max_radius=1000.0, min_range=0)   # ring 0 reaches to 50 m: 50 000 bins
    want = rc.build_batch(img, az, col_offset=0, cols=cols, **kw)
    assert np.count_nonzero(want) == 1 and 250.0 < want.max() < 255.0
    same(device_build(mod.RadarContext(rows, cols, **kw), img, az, off=0), want)


def test_bad_arguments(mod):
    from navtech_radar_slam_amd import _rsx
    L = _rsx.lib()

    def create(rows=ROWS, cols=COLS, **fields):
        p = mod.default_params()
        for k, v in fields.items():
            setattr(p, k, v)
        h = C.c_void_p(1)
        st = L.rsx_radarsc_create(0, rows, cols, C.byref(p), C.byref(h))
        if st == 0:
            L.rsx_radarsc_destroy(h)
        else:
            assert not h.value                      # a create that fails clears *out
        return st

    assert create() == 0 and create(rows=1, cols=1) == 0 and create(rows=4096, cols=8192) == 0
    for bad in (dict(rows=0), dict(rows=4097), dict(cols=0), dict(cols=8193), dict(power_floor=-1), dict(power_floor=256),
                dict(max_radius=0.0), dict(max_radius=-1.0), dict(max_radius=float("inf")), dict(max_radius=float("nan")),
                dict(resolution=0.0), dict(resolution=-0.1), dict(resolution=float("nan")), dict(min_range=-1), dict(stat=2), dict(stat=-1)):
        assert create(**bad) == -1, bad
    assert L.rsx_radarsc_create(0, ROWS, COLS, None, None) == -1
    assert L.rsx_radarsc_default_params(None) == -1
    assert L.rsx_radarsc_destroy(None) == 0
    ctx = mod.RadarContext(ROWS, COLS, **SMALL)
    imgs = images(8, 2)
    az = grids()["plain"]
    out = np.zeros((2, 1200), np.float32)
    ok = (ctx._h, imgs.ctypes.data, 2, ROWS * STRIDE, STRIDE, OFF, az.ctypes.data, 0, out.ctypes.data)

    def host(**ch):
        names = ("h", "imgs", "n", "image_stride", "row_stride", "off", "az", "per_image", "out")
        a = dict(zip(names, ok))
        a.update(ch)
        return L.rsx_radarsc_build_batch(*[a[k] for k in names])

    assert host() == 0
    for bad in (dict(h=None), dict(imgs=None), dict(az=None), dict(out=None), dict(n=-1), dict(row_stride=OFF + COLS - 1), dict(off=-1),
                dict(off=STRIDE - COLS + 1), dict(image_stride=ROWS * STRIDE - 1)):
        assert host(**bad) == -1, bad
    assert host(n=0, imgs=None, az=None, out=None) == 0
    assert L.rsx_radarsc_build_batch_device(ctx._h, None, 1, ROWS * STRIDE, STRIDE, OFF, None, 0, None, None) == -1
    assert L.rsx_radarsc_build_batch_device(None, None, 0, 0, STRIDE, OFF, None, 0, None, None) == -1
    assert L.rsx_radarsc_build_batch_device(ctx._h, None, 0, 0, STRIDE, OFF, None, 0, None, None) == 0


def test_three_streams_on_one_handle_equal_a_serial_run(mod):
    """include/rsx.h: calls on one handle that pass different streams are ordered by the library"""
    import torch
    ctx = mod.RadarContext(ROWS, COLS, **SMALL)
    az = grids()["wraps"]
    batches = [images(20 + i, 9) for i in range(6)]
    want = [want_batch(b, az, **SMALL) for b in batches]
    dev = [torch.from_numpy(b).cuda() for b in batches]
    daz = torch.from_numpy(az).cuda()
    outs = [torch.full((9, 1200), -7.0, dtype=torch.float32, device="cuda") for _ in batches]
    streams = [torch.cuda.Stream() for _ in range(3)]
    torch.cuda.synchronize()
    for i, (d, o) in enumerate(zip(dev, outs)):
        ctx.build_batch_device(d.data_ptr(), 9, ROWS * STRIDE, STRIDE, daz.data_ptr(), o.data_ptr(), col_offset=OFF,
                               stream=streams[i % 3].cuda_stream)
    torch.cuda.synchronize()
    for o, w in zip(outs, want):
        same(o.cpu().numpy(), w)
