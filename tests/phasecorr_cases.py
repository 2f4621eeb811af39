"""The cases of tests/test_phasecorr_cases.py (CPU: the cases are what they claim to be) and tests/test_gpu_phasecorr_cases.py (the kernels of
csrc/phasecorr.hip against tests/phasecorr_np.py on them).  Pure numpy.

A scene is a fixed world of point reflectors seen from a pose (x, y, yaw) in the library's frame: azimuth row a is at 2 pi a / rows, range
bin r has its centre at (r + 0.5) range_resolution, a return at azimuth phi and range rho sits at (rho cos phi, rho sin phi).  Scan 0 is at the
origin, scan i at MOTIONS[i - 1] (pixels of `resolution`, radians), so pair (i, 0) registers to pose i and pair (0, i) to its inverse.  The
shapes are the smallest at which every path of the kernels still exists: rows odd, prime or a divisor of nothing, cols no multiple of anything,
one image size per transform length; the translations are whole pixels, so the peaks of the translation surface fall on rows and columns 0
and N - 1 and in all four quadrants, and the rotations put the winning candidate on both sides of the half turn."""
import functools
import math
from collections import namedtuple

import numpy as np

import phasecorr_np as pcn

MARGIN = 1e-4      # what a peak of the restatement must lead every other sample by (tests/test_phasecorr_cases.py): over twice the device's bound
MIN_ROWS, MIN_BINS = 0.8, 1.2   # the least width (sigma) of a blob
MIN_DENOM = 5e-3   # the least |cm - 2 c0 + cp| of a parabola

# snap: the yaws of MOTIONS are rounded to whole azimuth rows.  Where a row is several angle bins wide (3.5 at s64, 9.7 at s256, 20 at s512) the
# bilinear resampling leaves a pattern that belongs to the polar grid, and it draws a rotation between two rows off its truth by up to 5 bins
# (measured on the restatement); a rotation by whole rows is its own exact roll of the samples and comes back within one bin.  s128, whose row
# is 2.8 bins, keeps the yaws as they stand: a rotation that falls between the rows stays in the set.
Shape = namedtuple("Shape", "rows cols fields seed snap", defaults=(False,))
SHAPES = {
    "s64": Shape(37, 97, dict(n=64, resolution=1.0, range_resolution=1.0, min_range_bins=0), 64, True),     # min_range_bins 0: the hole is rc < 0 alone
    "s128": Shape(90, 130, dict(n=128, resolution=0.5, range_resolution=0.5, min_range_bins=3), 128),
    "s256": Shape(53, 301, dict(n=256, resolution=1.0, range_resolution=0.9, min_range_bins=5), 256, True),
    "s512": Shape(50, 300, dict(n=512, resolution=1.0, range_resolution=1.0, min_range_bins=2), 512, True),
}
# image only (no pairs): one row, two rows, the most rows the library takes; the disc rule passes and the image is not all zero
DEGENERATE = {
    "1x3": Shape(1, 3, dict(n=64, resolution=0.05, range_resolution=1.0, min_range_bins=0), 13),
    "2x3": Shape(2, 3, dict(n=64, resolution=0.05, range_resolution=1.0, min_range_bins=0), 23),
    "4096x40": Shape(4096, 40, dict(n=64, resolution=1.0, range_resolution=1.0, min_range_bins=0), 4096),
}
MOTIONS = [(3, 0, 0.0), (-3, 2, 0.0), (0, -1, 0.0), (-1, -1, 0.3), (2, -4, -2.0), (0, 0, 2.8)]   # scan i is at MOTIONS[i - 1]
ALL_PAIRS = [(i, 0) for i in range(1, 7)] + [(0, i) for i in range(1, 7)] + [(0, 0)]
# one candidate: the pairs whose rotation lies within a quarter turn, and one that does not (its only candidate is half a turn off)
ONE_PAIRS = [(i, 0) for i in range(1, 5)] + [(0, i) for i in range(1, 5)] + [(0, 0), (6, 0)]
PAIRS_512 = [(2, 0), (0, 4), (5, 0)]   # three at most: the restatement's table loops are the slow part at N = 512

# pairs: [(src, dst)]; truth: per pair (x, y, theta) in metres and radians, None for an empty pair; ambiguous: indices of pairs without a decided peak
Case = namedtuple("Case", "name shape rows cols fields images pairs truth ambiguous empty")


def _wrap(t):
    return (t + math.pi) % (2.0 * math.pi) - math.pi


def world(shape):
    """-> [k, 3] reflectors (x, y [m], amplitude): uniform over 1.1 x the image's half-width, 60 of them at N <= 128, 200 above"""
    n, res = shape.fields["n"], shape.fields["resolution"]
    rng = np.random.default_rng(shape.seed)
    k = 60 if n <= 128 else 200
    half = 1.1 * (n // 2) * res
    return np.column_stack([rng.uniform(-half, half, k), rng.uniform(-half, half, k), rng.uniform(120.0, 250.0, k)])


def render(shape, pose, noise_seed, reflectors=None):
    """-> [rows, cols] u8: every reflector a Gaussian blob at its continuous (azimuth row, range bin) position as seen from `pose`, one pixel of
    `resolution` wide but never below 0.8 rows and 1.2 bins (a narrower blob falls between the samples), over a gamma speckle floor of mean 12"""
    rows, cols = shape.rows, shape.cols
    res, rres = shape.fields["resolution"], shape.fields["range_resolution"]
    pts = world(shape) if reflectors is None else reflectors
    x, y, yaw = pose
    c, s = math.cos(yaw), math.sin(yaw)
    px = c * (pts[:, 0] - x) + s * (pts[:, 1] - y)     # R(-yaw) (w - t)
    py = -s * (pts[:, 0] - x) + c * (pts[:, 1] - y)
    rho = np.hypot(px, py)
    a = (np.arctan2(py, px) % (2.0 * math.pi)) * rows / (2.0 * math.pi)
    b = rho / rres - 0.5
    sig_a = np.clip(res / np.maximum(rho * 2.0 * math.pi / rows, 1e-9), MIN_ROWS, max(MIN_ROWS, rows / 8.0))
    sig_b = max(MIN_BINS, res / rres)
    img = np.random.default_rng(noise_seed).gamma(2.0, 6.0, (rows, cols))
    ai, bi = np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64)
    for k in range(len(pts)):
        if b[k] > cols + 4.0 * sig_b:
            continue
        da = (ai - a[k] + rows / 2.0) % rows - rows / 2.0     # the azimuth wraps
        img += pts[k, 2] * np.outer(np.exp(-0.5 * (da / sig_a[k]) ** 2), np.exp(-0.5 * ((bi - b[k]) / sig_b) ** 2))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def poses(shape):
    res, row = shape.fields["resolution"], 2.0 * math.pi / shape.rows
    return [(0.0, 0.0, 0.0)] + [(mx * res, my * res, round(yaw / row) * row if shape.snap else yaw) for mx, my, yaw in MOTIONS]


@functools.lru_cache(maxsize=None)
def scans(name):
    """-> [7, rows, cols] u8 (read-only): scan 0 at the origin, scan i at MOTIONS[i - 1], each with a speckle seed of its own"""
    shape = SHAPES[name]
    out = np.stack([render(shape, p, 1000 * shape.seed + i) for i, p in enumerate(poses(shape))])
    out.setflags(write=False)
    return out


def pair_truth(shape, src, dst):
    """(x, y, theta) with p_dst = R(theta) p_src + (x, y)"""
    ps, pd = poses(shape)[src], poses(shape)[dst]
    th = _wrap(ps[2] - pd[2])
    c, s = math.cos(pd[2]), math.sin(pd[2])
    dx, dy = ps[0] - pd[0], ps[1] - pd[1]
    return (c * dx + s * dy, -s * dx + c * dy, th)


def pack(images, padded):
    """[n, rows, cols] u8 -> (buffer u8 [bytes], image_stride_bytes, row_stride, col_offset).  Tight: at offset 0.  Padded: col_offset 5, 3 spare
    bytes at each row's end, 17 between images, every spare byte 0xA5 -- a kernel that reads one changes the result"""
    images = np.asarray(images, dtype=np.uint8)
    n, rows, cols = images.shape
    off, tail, gap = (5, 3, 17) if padded else (0, 0, 0)
    row_stride = off + cols + tail
    image_stride = rows * row_stride + gap
    buf = np.full(n * image_stride, 0xA5, dtype=np.uint8)
    np.lib.stride_tricks.as_strided(buf[off:], (n, rows, cols), (image_stride, row_stride, 1))[...] = images
    return buf, image_stride, row_stride, off


def unpack(buf, n, rows, image_stride, row_stride):
    """the [n, rows, row_stride] view of a packed buffer that phasecorr_np.cart_image indexes with col_offset"""
    return np.lib.stride_tricks.as_strided(buf, (n, rows, row_stride), (image_stride, row_stride, 1), writeable=False)


def _case(name, shape_name, pairs, ambiguous=(), **fields):
    sh = SHAPES[shape_name]
    return Case(name, shape_name, sh.rows, sh.cols, dict(sh.fields, **fields), scans(shape_name), list(pairs),
                [pair_truth(sh, s, d) for s, d in pairs], frozenset(ambiguous), False)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case, in the order the tests run them"""
    out = [_case("s64", "s64", ALL_PAIRS), _case("s128", "s128", ALL_PAIRS), _case("s256", "s256", ALL_PAIRS), _case("s512", "s512", PAIRS_512)]
    for sn in ("s64", "s128"):
        out.append(_case(sn + "-one", sn, ONE_PAIRS, ambiguous=[ONE_PAIRS.index((6, 0))], resolve_half_turn=0))
    sh = SHAPES["s64"]
    imgs = np.stack([np.zeros((sh.rows, sh.cols), dtype=np.uint8), scans("s64")[0]])
    imgs.setflags(write=False)
    out.append(Case("s64-empty", "s64", sh.rows, sh.cols, dict(sh.fields), imgs, [(0, 0), (0, 1), (1, 0)], [None] * 3, frozenset(), True))
    return {c.name: c for c in out}


@functools.lru_cache(maxsize=None)
def expected(name):
    """the restatement's results of a case (computed once per process, shared by the test modules, never written to) -> (results, carts)"""
    c = cases()[name]
    return pcn.Restatement(c.rows, c.cols, c.fields).register_batch(c.images, c.pairs, col_offset=0)


@functools.lru_cache(maxsize=None)
def degenerate_scans(name):
    """-> [2, rows, cols] u8: two poses of a degenerate polar shape (image only)"""
    sh = DEGENERATE[name]
    res = sh.fields["resolution"]
    out = np.stack([render(sh, p, 1000 * sh.seed + i) for i, p in enumerate([(0.0, 0.0, 0.0), (2 * res, -res, 0.4)])])
    out.setflags(write=False)
    return out


def denominators(w, n):
    """|cm - 2 c0 + cp| of the three parabolas of a restatement result: the rotation curve, the surface along j, along i"""
    k0, (i0, j0), cu, s = w["rot_k0"], w["peak_ij"], w["rot_curve"], w["surface"]
    return (abs(cu[(k0 - 1) % n] - 2.0 * cu[k0] + cu[(k0 + 1) % n]), abs(s[i0, (j0 - 1) % n] - 2.0 * s[i0, j0] + s[i0, (j0 + 1) % n]),
            abs(s[(i0 - 1) % n, j0] - 2.0 * s[i0, j0] + s[(i0 + 1) % n, j0]))


def lead(a):
    """by how much the maximum of an array exceeds every other sample"""
    f = np.sort(np.asarray(a, dtype=np.float64).ravel())
    return float(f[-1] - f[-2])
