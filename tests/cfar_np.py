"""CA-CFAR / BFAR keypoint extraction restated with plain shifted additions: the arithmetic contract that csrc/cfar.hip
implements (include/rsx.h, rsx_cfar_*).  TEST INFRASTRUCTURE ONLY.  Integers only, so the GPU must match bit for bit.

Per azimuth row, v[j] = the power byte of range bin j, 0 <= j < cols; t = train, g = guard, A = scale_q8, B = offset,
s = min_separation:
  1. key[j], win[j]: steps 1 and 2 of k-strongest (kstrongest_np.row_keys; raw power, the window cut at the row's ends)
  2. training cells of bin j: left j - g - t <= i <= j - g - 1, i >= 0; right j + g + 1 <= i <= j + g + t, i <= cols - 1;
     their sums and counts S_L, n_L, S_R, n_R (cut at the row's ends, raw power)
  3. noise (S, n): mode 0 both sides; mode 1 the side of the larger mean (left iff S_L n_R >= S_R n_L); mode 2 the side of
     the smaller mean; an empty side gives way to the other
  4. detection: 256 n v[j] > A S + 256 B n when n > 0, v[j] > B when n = 0
  5. candidate: key[j] == win[j], a detection, min_range <= j < hi; hi = cols when max_range == 0, else min(max_range, cols)
  6. the row's keypoints: the min(k, #candidates) candidates of highest key, in ascending j; the image's in row-major order
The kernel screens first and sums the training bytes of the survivors only; this file deliberately does neither: S and n
of every bin are 2 t shifted additions of the row and of a row of ones, and there are no prefix sums."""
import numpy as np

from kstrongest_np import row_keys

CA, GO, SO = 0, 1, 2


def side_sums(v, train, guard):
    """v: (cols,) -> S_L, n_L, S_R, n_R, each (cols,) int64"""
    v = np.asarray(v, dtype=np.int64)
    cols = len(v)
    ones = np.ones(cols, dtype=np.int64)
    SL, nL, SR, nR = (np.zeros(cols, dtype=np.int64) for _ in range(4))
    for d in range(guard + 1, guard + train + 1):
        if d >= cols:
            break
        SL[d:] += v[:-d]   # bin j - d
        nL[d:] += ones[:-d]
        SR[:-d] += v[d:]   # bin j + d
        nR[:-d] += ones[d:]
    return SL, nL, SR, nR


def detections(v, train=20, guard=2, scale_q8=768, offset=20, mode=CA):
    """v: (cols,) uint8 -> (cols,) bool, step 4"""
    v = np.asarray(v, dtype=np.int64)
    SL, nL, SR, nR = side_sums(v, train, guard)
    if mode == CA:
        S, n = SL + SR, nL + nR
    else:
        left_ge = SL * nR >= SR * nL
        left = left_ge if mode == GO else ~left_ge
        left = np.where(nL == 0, False, np.where(nR == 0, True, left))
        S, n = np.where(left, SL, SR), np.where(left, nL, nR)
    rhs = scale_q8 * S + 256 * offset * n
    return np.where(n > 0, 256 * n * v > rhs, v > offset)


def extract_row(v, k=12, train=20, guard=2, scale_q8=768, offset=20, mode=CA, min_range=58, max_range=0, min_separation=5):
    """v: (cols,) uint8 -> the row's keypoints: ascending range bins, int64"""
    v = np.asarray(v, dtype=np.int64)
    cols = len(v)
    hi = cols if max_range == 0 else min(max_range, cols)
    key = row_keys(v)
    win = key.copy()
    for d in range(1, min(min_separation, cols - 1) + 1):
        win[d:] = np.maximum(win[d:], key[:-d])
        win[:-d] = np.maximum(win[:-d], key[d:])
    j = np.arange(cols)
    det = detections(v, train, guard, scale_q8, offset, mode)
    cand = np.nonzero((key == win) & det & (j >= min_range) & (j < hi))[0]
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
