"""CPU checks of the cen2018 restatement (tests/cen2018_np.py), the contract csrc/cen2018.hip is tested against: the
vectorised form equals a literal per-pixel transcription of the recalled upstream loop under the pinned definitions, and
hand-built rows give the runs and medians the method defines."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cen2018_np as c18  # noqa: E402

F = np.float32


def scalar_reference(b, zq, sigma_gauss, min_range):
    """the recalled loop, pixel by pixel, with the pinned definitions (numpy float32 / float64 scalars, math.exp for the
    weights, the per-pixel exps in np.float64 like the restatement)"""
    rows, cols = b.shape
    fsize = 3 * sigma_gauss
    mu = fsize // 2
    sig_sqr = float(F(sigma_gauss * sigma_gauss))
    w = [F(math.exp(-0.5 * (k - mu) * (k - mu) / sig_sqr)) for k in range(fsize)]
    s = F(0.0)
    for x in w:
        s = F(s + x)
    w = [F(x / s) for x in w]

    def refl(x):
        if cols == 1:
            return 0
        P = 2 * (cols - 1)
        m = x % P
        return m if m < cols else P - m

    out = []
    for i in range(rows):
        row = [int(v) for v in b[i]]
        mean = F(sum(row) / 255.0 / cols)
        q = [F(F(v) / F(255.0)) - mean for v in row]
        S, n = 0.0, 0
        for v in range(256):
            qb = F(F(v) / F(255.0)) - mean
            c = row.count(v)
            if qb < 0:
                S = S + float(c) * (2.0 * float(qb) * float(qb))
                n += c
        sigma = F(math.sqrt(F(S / n))) if n else F(0.034)
        assert sigma == np.sqrt(F(S / n)) if n else True  # (sqrt of a float32 is the float32 sqrt)
        thres = F(F(zq) * sigma)
        run = []
        for j in range(cols):
            pj = F(0.0)
            for k in range(fsize):
                pj = F(pj + F(w[k] * q[refl(j + k - mu)]))
            hit = False
            if j >= min_range:
                d1 = F((q[j] - pj) / sigma)
                d2 = F(pj / sigma)
                nqp = F(np.exp(np.float64(-0.5) * np.float64(d1) * np.float64(d1)))
                npp = F(np.exp(np.float64(-0.5) * np.float64(d2) * np.float64(d2)))
                bb = F(nqp - npp)
                y = F(F(q[j] * F(F(1.0) - nqp)) + F(pj * bb))
                hit = bool(y > thres)
            if hit:
                run.append(j)
            if run and (not hit or j == cols - 1):
                out.append((i, run[len(run) // 2]))
                run = []
    return np.array(out, dtype=np.int32).reshape(-1, 2)


@pytest.mark.parametrize("seed,rows,cols,sg,zq,mr", [(1, 6, 90, 3, 3.0, 5), (2, 4, 64, 1, 1.5, 0), (3, 3, 40, 5, 2.0, 10),
                                                     (4, 2, 7, 5, 1.0, 0), (5, 5, 130, 17, 3.0, 58)])
def test_vectorised_equals_scalar_loop(seed, rows, cols, sg, zq, mr):
    rng = np.random.default_rng(seed)
    b = rng.gamma(2.0, 15.0, size=(rows, cols)).clip(0, 255).astype(np.uint8)
    for _ in range(rows * 2):
        a, r = int(rng.integers(0, rows)), int(rng.integers(0, cols))
        b[a, r:r + int(rng.integers(1, 6))] = rng.integers(120, 255)
    want = scalar_reference(b, zq, sg, mr)
    got = c18.extract(b, col_offset=0, zq=zq, sigma_gauss=sg, min_range=mr)
    assert np.array_equal(got, want), (got, want)
    assert len(want) > 0


def _row_with_runs(cols, runs, lo=20, hi=250):
    r = np.full(cols, lo, dtype=np.uint8)
    for s, e in runs:
        r[s:e + 1] = hi
    return r


def test_run_medians_odd_even_last_column_and_min_range():
    cols = 200
    runs = [(30, 32), (60, 63), (100, 100), (150, 155), (196, 199)]  # odd, even, single, even, reaching the last column
    b = np.stack([_row_with_runs(cols, runs), _row_with_runs(cols, [(45, 52)])])
    tg, dbg = c18.extract(b, col_offset=0, zq=3.0, sigma_gauss=1, min_range=0, debug=True)
    want = [(0, 31), (0, 62), (0, 100), (0, 153), (0, 198), (1, 49)]
    assert [tuple(t) for t in tg] == want
    # a run straddling min_range starts at min_range: (48 .. 52) -> 50
    tg = c18.extract(b, col_offset=0, zq=3.0, sigma_gauss=1, min_range=48)
    assert [tuple(t) for t in tg] == [(0, 62), (0, 100), (0, 153), (0, 198), (1, 50)]
    # min_range past the row: nothing
    assert len(c18.extract(b, col_offset=0, sigma_gauss=1, min_range=cols)) == 0


def test_constant_rows_and_zero_image_use_the_fallback_sigma():
    b = np.full((3, 50), 77, dtype=np.uint8)
    tg, dbg = c18.extract(b, col_offset=0, sigma_gauss=3, min_range=0, debug=True)
    assert len(tg) == 0 and np.all(dbg["sigma"] == F(0.034))
    z = np.zeros((2, 40), dtype=np.uint8)
    tg, dbg = c18.extract(z, col_offset=0, sigma_gauss=3, min_range=0, debug=True)
    assert len(tg) == 0 and np.all(dbg["sigma"] == F(0.034)) and np.all(dbg["mean"] == 0)


def test_three_taps_and_rows_shorter_than_the_filter():
    rng = np.random.default_rng(9)
    for cols, sg in ((3, 1), (5, 9), (2, 17), (1, 3), (11, 33)):
        b = rng.integers(0, 255, size=(4, cols)).astype(np.uint8)
        want = scalar_reference(b, 1.0, sg, 0)
        got = c18.extract(b, col_offset=0, zq=1.0, sigma_gauss=sg, min_range=0)
        assert np.array_equal(got, want), (cols, sg)
    # reflect 101, repeated: period 2 (cols - 1)
    assert c18.refl101(np.arange(-7, 12), 4).tolist() == [1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1]
    assert c18.refl101(np.arange(-3, 4), 1).tolist() == [0] * 7


@pytest.mark.parametrize("sg", [1, 3, 17, 33, 85])
def test_weights_symmetric_and_normalised(sg):
    w = c18.gauss_weights(sg)
    assert w.dtype == np.float32 and len(w) == 3 * sg
    assert np.array_equal(w, w[::-1])
    s = F(0.0)
    for x in w:
        s = F(s + x)
    assert abs(float(s) - 1.0) < 1e-5


def test_library_weights_equal_the_restatement():
    """rsx_cen2018_gauss_weights is host code (no device): the taps the kernels use, bit for bit, and its argument checks"""
    import ctypes as C
    import __graft_entry__ as ge
    from navtech_radar_slam_amd import _rsx
    if not os.path.exists(_rsx.LIB_PATH):
        ge.build()
    from navtech_radar_slam_amd import cen2018
    for sg in (1, 3, 17, 33, 85):
        assert np.array_equal(cen2018.gauss_weights(sg), c18.gauss_weights(sg)), sg
    L = _rsx.lib()
    buf = np.zeros(300, dtype=np.float32)
    for sg, mx in ((0, 300), (2, 300), (-3, 300), (87, 300), (17, 50)):
        assert L.rsx_cen2018_gauss_weights(sg, buf.ctypes.data, mx) == -1, (sg, mx)
    assert L.rsx_cen2018_gauss_weights(17, None, 51) == -1
    p = _rsx.Cen2018Params()
    assert L.rsx_cen2018_default_params(C.byref(p)) == 0
    assert (p.zq, p.sigma_gauss, p.min_range, p.reserved) == (3.0, 17, 58, 0)
