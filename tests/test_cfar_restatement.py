"""The CFAR restatement (tests/cfar_np.py: shifted additions) against a bin-by-bin double loop written straight from the rule in
include/rsx.h, and the properties the rule promises: A = 0 is k-strongest with z_min = B + 1, the comparison is strict, the three
noise estimates differ at a clutter edge, and the arithmetic stays below 2^31 at the parameter maxima.  CPU only."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cfar_np as cfn  # noqa: E402
import kstrongest_np as ksn  # noqa: E402


def loop_row(v, k, train, guard, scale_q8, offset, mode, min_range, max_range, min_separation):
    """the rule of include/rsx.h, one bin and one training cell at a time"""
    v = [int(x) for x in v]
    cols = len(v)
    hi = cols if max_range == 0 else min(max_range, cols)
    cand = []
    for j in range(cols):
        key = (v[j] << 16) | (0xFFFF - j)
        win = max((v[i] << 16) | (0xFFFF - i) for i in range(max(0, j - min_separation), min(cols - 1, j + min_separation) + 1))
        SL = nL = SR = nR = 0
        for i in range(j - guard - train, j - guard):
            if i >= 0:
                SL, nL = SL + v[i], nL + 1
        for i in range(j + guard + 1, j + guard + train + 1):
            if i <= cols - 1:
                SR, nR = SR + v[i], nR + 1
        if mode == 0:
            S, n = SL + SR, nL + nR
        elif nL == 0 or nR == 0:
            S, n = (SR, nR) if nL == 0 else (SL, nL)
        else:
            left_greater = SL * nR >= SR * nL
            S, n = (SL, nL) if left_greater == (mode == 1) else (SR, nR)
        det = 256 * n * v[j] > scale_q8 * S + 256 * offset * n if n > 0 else v[j] > offset
        if key == win and det and min_range <= j < hi:
            cand.append((key, j))
    cand.sort(reverse=True)
    return sorted(j for _, j in cand[:k])


T, G = 6, 3
SHAPES = [(1, 1), (3, 2), (3, G + 1), (3, G + 2), (3, 2 * (G + T)), (3, 2 * (G + T) + 1), (2, 300)]


@pytest.mark.parametrize("rows,cols", SHAPES)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_restatement_equals_double_loop(rows, cols, mode):
    rng = np.random.default_rng(1000 * rows + cols)
    some = 0
    for trial in range(4):
        img = rng.gamma(2.0, 25.0, size=(rows, cols)).clip(0, 255).astype(np.uint8)
        for t, g, A, B, s, k, mr, xr in ((T, G, 300, 0, 0, 128, 0, 0), (T, G, 256, 5, 1, 3, 0, 0), (T, G, 0, 30, 2, 12, 1, cols - 1),
                                       (1, 0, 400, 0, 0, 128, 0, 0), (64, 16, 200, 10, 5, 12, 0, 0), (20, 2, 512, 0, 3, 2, 0, cols + 3)):
            p = dict(k=k, train=t, guard=g, scale_q8=A, offset=B, mode=mode, min_range=mr, max_range=xr, min_separation=s)
            for a in range(rows):
                want = loop_row(img[a], **p)
                got = cfn.extract_row(img[a], **p)
                assert got.tolist() == want, (p, a)
                some += len(want)
    assert some > 0


def test_side_sums_have_empty_sides():
    """(3, g + 1): no bin has a training cell; (3, g + 2): the first bin has one on the right only, the last on the left only"""
    v = np.arange(1, G + 2)
    SL, nL, SR, nR = cfn.side_sums(v, T, G)
    assert not nL.any() and not nR.any() and not SL.any() and not SR.any()
    v = np.arange(1, G + 3)
    SL, nL, SR, nR = cfn.side_sums(v, T, G)
    assert nR.tolist() == [1] + [0] * (G + 1) and nL.tolist() == [0] * (G + 1) + [1]
    assert SR[0] == v[-1] and SL[-1] == v[0]


@pytest.mark.parametrize("B", [0, 59, 254])
@pytest.mark.parametrize("s", [0, 5])
def test_scale_zero_is_kstrongest(B, s):
    from navtech_radar_slam_amd import synth
    img, _, _ = synth.polar_image(41, rows=6, n_targets=100)
    if B == 254:
        img = img.copy()
        img[:, 200:3000:97] = 255
    total = 0
    for mode in (0, 1, 2):
        got = cfn.extract(img, scale_q8=0, offset=B, mode=mode, min_separation=s)
        want = ksn.extract(img, z_min=B + 1, min_separation=s)
        assert np.array_equal(got, want)
        total += len(want)
    assert total > 0


def test_flat_rows_across_the_strict_threshold():
    v = np.full(100, 100, dtype=np.uint8)
    for mode in (0, 1, 2):
        assert len(cfn.extract_row(v, k=128, scale_q8=256, offset=0, mode=mode, min_range=0, min_separation=0)) == 0
        assert cfn.extract_row(v, k=128, scale_q8=255, offset=0, mode=mode, min_range=0, min_separation=0).tolist() == list(range(100))
        assert not cfn.detections(v, scale_q8=256, offset=0, mode=mode).any()
        assert cfn.detections(v, scale_q8=255, offset=0, mode=mode).all()


def test_modes_differ_at_a_clutter_edge():
    """noise 20 below bin 150, 80 from it on, a spike of 140 at bins 150 and 151.  At a = 3 (A = 768), t = 20, g = 2: the left mean
    is 20 and the right 80, so cell averaging sets T = 3 x 50 = 150 > 140 (no detection), greatest-of T = 240 (none), smallest-of
    T = 60 (both); at a = 2.5 (A = 640) cell averaging T = 125 detects while greatest-of (200) still does not."""
    v = np.full(300, 20, dtype=np.uint8)
    v[150:] = 80
    v[150:152] = 140
    verdicts = {}
    for mode in (0, 1, 2):
        d = cfn.detections(v, train=20, guard=2, scale_q8=640, offset=0, mode=mode)
        verdicts[mode] = d
    assert verdicts[0][150] and verdicts[0][151]
    assert not verdicts[1][150] and not verdicts[1][151]
    assert verdicts[2][150] and verdicts[2][151]
    # all three differ as whole-row verdicts: smallest-of also fires on the 80 plateau next to the edge, cell averaging does not
    assert not np.array_equal(verdicts[0], verdicts[1]) and not np.array_equal(verdicts[0], verdicts[2]) and not np.array_equal(verdicts[1], verdicts[2])
    kp = {mode: cfn.extract_row(v, k=128, train=20, guard=2, scale_q8=640, offset=0, mode=mode, min_range=0, min_separation=0).tolist()
          for mode in (0, 1, 2)}
    assert kp[0] != kp[1] and kp[0] != kp[2] and kp[1] != kp[2]
    assert 150 in kp[0] and 150 not in kp[1] and 150 in kp[2]


def test_bound_holds_at_the_parameter_maxima():
    v = np.full(400, 255, dtype=np.uint8)
    SL, nL, SR, nR = cfn.side_sums(v, 64, 16)
    S, n = SL + SR, nL + nR
    assert S.max() == 128 * 255 == 32640 and n.max() == 128
    rhs = 65535 * S + 256 * 255 * n
    assert rhs.max() == 2147418240 < 2 ** 31
    assert (256 * n * 255).max() < 2 ** 31
    assert (SL * nR).max() <= 64 * 255 * 64 < 2 ** 31
    # and the verdict there: a = 255.996 > 1 on a flat row detects nothing
    assert not cfn.detections(v, train=64, guard=16, scale_q8=65535, offset=255, mode=0).any()
