"""k-strongest keypoint extraction restated as a plain per-row loop: the arithmetic contract that csrc/kstrongest.hip
implements (include/rsx.h, rsx_kstrongest_*).  TEST INFRASTRUCTURE ONLY.  Integers only, so the GPU must match bit for bit.

Per azimuth row, v[j] = the power byte of range bin j, 0 <= j < cols, s = min_separation:
  1. key[j] = (v[j] << 16) | (0xFFFF - j)   (unique in a row; higher = stronger, on equal power the nearer bin wins)
  2. win[j] = max key[i] over max(0, j - s) <= i <= min(cols - 1, j + s)   (cut at the row's ends, raw power)
  3. candidate: key[j] == win[j], v[j] >= z_min, min_range <= j < hi; hi = cols when max_range == 0, else min(max_range, cols)
  4. the row's keypoints: the min(k, #candidates) candidates of highest key, in ascending j
  5. the image's keypoints: the rows' keypoints in row-major order, (azimuth idx, range idx) int32
The kernel selects with a histogram of powers; this file deliberately does not: the window maximum is 2 s shifted
comparisons of the key array, and the k highest keys are taken one maximum at a time."""
import numpy as np


def row_keys(v):
    v = np.asarray(v, dtype=np.int64)
    return (v << 16) | (0xFFFF - np.arange(len(v), dtype=np.int64))


def extract_row(v, k=12, z_min=60, min_range=58, max_range=0, min_separation=5):
    """v: (cols,) uint8 -> the row's keypoints: ascending range bins, int64"""
    v = np.asarray(v, dtype=np.int64)
    cols = len(v)
    hi = cols if max_range == 0 else min(max_range, cols)
    key = row_keys(v)
    win = key.copy()
    for d in range(1, min(min_separation, cols - 1) + 1):
        win[d:] = np.maximum(win[d:], key[:-d])   # bin j - d
        win[:-d] = np.maximum(win[:-d], key[d:])  # bin j + d
    j = np.arange(cols)
    cand = np.nonzero((key == win) & (v >= z_min) & (j >= min_range) & (j < hi))[0]
    left = key[cand].copy()
    kept = []
    for _ in range(min(k, len(cand))):
        i = int(np.argmax(left))
        kept.append(int(cand[i]))
        left[i] = -1
    return np.array(sorted(kept), dtype=np.int64)


def extract(img, col_offset=11, cols=None, **params):
    """img: (rows, row_stride) uint8 -> targets (n, 2) int32, row-major"""
    img = np.asarray(img, dtype=np.uint8)
    if cols is None:
        cols = img.shape[1] - col_offset
    out = []
    for a in range(img.shape[0]):
        for r in extract_row(img[a, col_offset:col_offset + cols], **params):
            out.append((a, r))
    return np.array(out, dtype=np.int32).reshape(-1, 2)


def to_cartesian(targets, azimuths, resolution):
    from oracle import pyoracle as po
    return po.cen2019_to_cartesian(targets, azimuths, resolution)
