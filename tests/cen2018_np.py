"""cen2018 keypoint extraction (Cen & Newman, ICRA 2018) restated in vectorised numpy: the arithmetic contract that
csrc/cen2018.hip implements.  TEST INFRASTRUCTURE ONLY.

PARITY UNPINNED: upstream (yeti_radar_odometry `cen2018features(fft_data, zq, sigma_gauss, min_range, targets)`, through
the reference's ORORA submodule) is absent from the reference checkout, so this follows the method as recalled.  Where the
recalled loop is order dependent, this pins an order-independent or explicitly ordered definition instead:
  * mean_i = (float)((double)(sum of the row's bytes) / 255.0 / cols)   (upstream: cv::mean of the float row)
  * sigma_i from the row's 256-bin byte histogram: S = sum over b ascending with q_b < 0 of (double)c_b * (2 q_b q_b),
    sequential in fp64, sigma_i = sqrtf((float)(S / n)), 0.034 when n = 0   (upstream: a float pixel loop in range order)
  * p_j = 0.0f, then p_j += w_k * q[refl(j + k - mu)] for k ascending, every product and sum rounded to float
    (upstream: cv::filter2D, BORDER_REFLECT101, whose summation order is OpenCV's)
  * d1 = (q - p) / sigma in float; nqp = (float)exp(-0.5 * d1 * d1) in double (upstream: pow(float, 2) promotes to double);
    npp the same with d2 = p / sigma; b = nqp - npp; y = q (1 - nqp) + p b, each op rounded to float; hit: y > zq * sigma
  * the Gaussian: w_k = (float)exp(-0.5 (k - mu)^2 / sigma_gauss^2) in double (libm exp: math.exp here), s = the float sum
    ascending, w_k = w_k / s in float
  * runs of consecutive hits j >= min_range; a run's keypoint is start + len // 2
Every float32 operation below is between float32 arrays or np.float32 scalars (NEP 50: a Python float would not change
the dtype of an array, but keeping them out makes the intent checkable)."""
import math

import numpy as np

F = np.float32
SIGMA_NONE = F(0.034)


def gauss_weights(sigma_gauss):
    fsize = 3 * sigma_gauss
    mu = fsize // 2
    sig_sqr = float(F(sigma_gauss * sigma_gauss))
    w = np.array([F(math.exp(-0.5 * (k - mu) * (k - mu) / sig_sqr)) for k in range(fsize)], dtype=np.float32)
    s = F(0.0)
    for k in range(fsize):
        s = F(s + w[k])
    return (w / s).astype(np.float32)


def refl101(x, cols):
    """repeated reflect 101 of integer positions x (array) into [0, cols)"""
    x = np.asarray(x, dtype=np.int64)
    if cols == 1:
        return np.zeros_like(x)
    P = 2 * (cols - 1)
    m = np.mod(x, P)
    return np.where(m < cols, m, P - m)


def row_stats(b):
    """b: (rows, cols) uint8 -> mean (rows,) f32, qtab (rows, 256) f32, sigma (rows,) f32"""
    rows, cols = b.shape
    mean = (b.astype(np.int64).sum(axis=1).astype(np.float64) / 255.0 / cols).astype(np.float32)
    fft_b = np.arange(256, dtype=np.float32) / F(255.0)
    qtab = (fft_b[None, :] - mean[:, None]).astype(np.float32)
    hist = np.stack([np.bincount(r, minlength=256) for r in b]) if rows else np.zeros((0, 256), np.int64)
    neg = qtab < 0
    qd = qtab.astype(np.float64)
    terms = np.where(neg, hist.astype(np.float64) * (2.0 * qd * qd), 0.0)
    S = np.zeros(rows, dtype=np.float64)
    for v in range(256):  # sequential, byte values ascending
        S = S + terms[:, v]
    n = np.where(neg, hist, 0).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        sig = np.sqrt((S / np.maximum(n, 1)).astype(np.float32))
    sigma = np.where(n > 0, sig, SIGMA_NONE).astype(np.float32)
    return mean, qtab, sigma


def smooth(q, w):
    """q: (rows, cols) f32, w: taps -> p (rows, cols) f32, taps ascending, every op rounded"""
    rows, cols = q.shape
    mu = len(w) // 2
    j = np.arange(cols)
    p = np.zeros((rows, cols), dtype=np.float32)
    for k in range(len(w)):
        p = p + w[k] * q[:, refl101(j + k - mu, cols)]
    return p


def likelihoods(q, p, sigma):
    """-> nqp, npp (f32 arrays): the two Gaussian likelihoods, exp in fp64"""
    s = sigma[:, None]
    d1 = ((q - p) / s).astype(np.float32)
    d2 = (p / s).astype(np.float32)
    e1, e2 = d1.astype(np.float64), d2.astype(np.float64)
    return np.exp(-0.5 * e1 * e1).astype(np.float32), np.exp(-0.5 * e2 * e2).astype(np.float32)


def statistic(q, p, nqp, npp):
    b = (nqp - npp).astype(np.float32)
    return (q * (F(1.0) - nqp) + p * b).astype(np.float32)


def runs_to_targets(hit):
    """hit: (rows, cols) bool -> (n, 2) int32 (azimuth, median range bin) row-major"""
    rows, cols = hit.shape
    h = np.zeros((rows, cols + 2), dtype=np.int8)
    h[:, 1:-1] = hit
    d = np.diff(h, axis=1)
    sa, sr = np.nonzero(d == 1)    # run starts (bin sr)
    ea, er = np.nonzero(d == -1)   # one past the run ends
    order_s = np.lexsort((sr, sa))
    order_e = np.lexsort((er, ea))
    sa, sr, er = sa[order_s], sr[order_s], er[order_e]
    med = sr + (er - sr) // 2
    return np.stack([sa, med], axis=1).astype(np.int32).reshape(-1, 2)


def extract(img, col_offset=11, zq=3.0, sigma_gauss=17, min_range=58, cols=None, debug=False):
    """img: (rows, row_stride) uint8, power bins at [col_offset, col_offset + cols) of every row (cols = None: to the row's
    end) -> targets (n, 2) int32 [, dict of the intermediates]"""
    img = np.asarray(img)
    b = np.ascontiguousarray(img[:, col_offset:col_offset + cols if cols is not None else img.shape[1]], dtype=np.uint8)
    rows, cols = b.shape
    mean, qtab, sigma = row_stats(b)
    q = np.take_along_axis(qtab, b.astype(np.int64), axis=1)
    w = gauss_weights(sigma_gauss)
    p = smooth(q, w)
    nqp, npp = likelihoods(q, p, sigma)
    y = statistic(q, p, nqp, npp)
    thres = (F(zq) * sigma).astype(np.float32)
    hit = y > thres[:, None]
    hit[:, :min(min_range, cols)] = False
    tg = runs_to_targets(hit)
    if debug:
        return tg, {"mean": mean, "sigma": sigma, "q": q, "p": p, "y": y, "nqp": nqp, "npp": npp, "thres": thres, "hit": hit, "w": w}
    return tg


def fragile_rows(dbg, min_range):
    """rows holding a pixel whose decision flips when nqp or npp moves by one float ulp (either way): there a device exp and
    a host exp that differ in the last bit may legitimately decide differently"""
    q, p, nqp, npp, thres = dbg["q"], dbg["p"], dbg["nqp"], dbg["npp"], dbg["thres"][:, None]
    base = dbg["hit"]
    flip = np.zeros_like(base)
    for a in (np.inf, -np.inf):
        for which in (0, 1):
            n1 = np.nextafter(nqp, F(a)).astype(np.float32) if which == 0 else nqp
            n2 = np.nextafter(npp, F(a)).astype(np.float32) if which == 1 else npp
            flip |= (statistic(q, p, n1, n2) > thres) != base
    flip[:, :min(min_range, q.shape[1])] = False
    return np.nonzero(flip.any(axis=1))[0]


def to_cartesian(targets, azimuths, resolution):
    from oracle import pyoracle as po
    return po.cen2019_to_cartesian(targets, azimuths, resolution)
