"""The kernels of csrc/phasecorr.hip through the C-ABI against tests/phasecorr_np.py on the cases of tests/phasecorr_cases.py: N = 128, one
candidate (resolve_half_turn 0), translation peaks on the first and last row and column and in all four quadrants, polar shapes from 1 x 3 to
4096 x 40, padded strides, empty images and one handle over calls of different sizes.  tests/test_phasecorr_cases.py shows on the CPU that the
cases are what they claim to be, and that every integer decision compared here is taken with a margin of MARGIN."""
import ctypes as C
import math

import numpy as np
import pytest

import phasecorr_cases as pcc
import phasecorr_np as pcn
from phasecorr_cases import MARGIN

pytestmark = pytest.mark.gpu

# Measured on an MI355X over every pair of every case of this file (test_cases_against_the_restatement prints them): the largest absolute
# difference between the device's fp32 curves / surfaces / peaks and the restatement's fp64 ones (both normalised: a perfect match is 1), and
# between the sub-bin estimates.  The bounds are 8 x the measurement: the order of every sum is fixed, so only fp32 round-off varies with
# the data.  Conditions, not measurements: 2 SURFACE_BOUND < MARGIN (a device peak cannot fall behind a sample the restatement's peak leads
# by MARGIN), SHIFT_BOUND < 0.01 pixel, ANGLE_BOUND < 0.01 angle bin.
# They are some 20 x those of test_gpu_phasecorr.py, and not by the kernels' doing.  Most pairs differ by 4e-8 .. 5e-7 as they do there; five
# differ by 0.6 .. 1.9e-6 in the surface (s64 (5, 0) and (6, 0), s128 (3, 0) and (0, 3), s256 (5, 0)).  In each of them the device's theta, 1e-6
# bins off the fp64 one, falls on the other side of a rounding step of the azimuth shift s, which the contract rounds to fp32 ONCE: with 37 to
# 90 rows a step of s (4e-6 to 8e-6 rows) turns the source image by far more of an angle than with 400, and the phase-normalised cross-power
# passes that on in full.  Moving the restatement's own theta across that step changes its surface by 1.46e-6, 1.76e-6 and 6.06e-7 for s64
# (6, 0), s128 (3, 0) and s256 (5, 0): the device's differences there are 1.47e-6, 1.77e-6 and 6.09e-7.
SURFACE_MEASURED, SHIFT_MEASURED, ANGLE_MEASURED = 1.884e-6, 3.850e-6, 6.560e-6   # surfaces (of 1), pixels, angle bins
SURFACE_BOUND, SHIFT_BOUND, ANGLE_BOUND = 8 * SURFACE_MEASURED, 8 * SHIFT_MEASURED, 8 * ANGLE_MEASURED   # 1.51e-5, 3.08e-5 px, 5.25e-5 bins
RESULT_BYTES = 56


@pytest.fixture(scope="module")
def pc():
    import os
    import __graft_entry__ as ge
    from navtech_radar_slam_amd import _rsx, phasecorr
    if not os.path.exists(_rsx.LIB_PATH):
        ge.build()
    return phasecorr


def _handle(pc, rows, cols, fields):
    return pc.Phasecorr(rows, cols, pc.params(**fields))


def _host(pc, h, packed, n_images, pairs, cart=False):
    """the C entry with the strides of a packaging (the Python wrapper's ascontiguousarray would hide them)"""
    from navtech_radar_slam_amd import _rsx
    buf, istride, rstride, off = packed
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    n = h.params.n
    res = np.zeros(len(pairs), dtype=_rsx.PHASECORR_RESULT_DTYPE)
    img = np.full((n_images, n, n), np.nan, dtype=np.float32) if cart else None
    _rsx.check(_rsx.lib().rsx_phasecorr_register_batch(h.handle, buf.ctypes.data, n_images, istride, rstride, off, pairs.ctypes.data, len(pairs),
                                                       res.ctypes.data, img.ctypes.data if cart else None))
    return (res, img) if cart else res


def _device(h, packed, n_images, pairs, cart=False):
    import torch
    from navtech_radar_slam_amd import _rsx
    buf, istride, rstride, off = packed
    n = h.params.n
    d_imgs = torch.from_numpy(buf).cuda()
    d_pairs = torch.tensor(pairs, dtype=torch.int32, device="cuda").reshape(-1, 2)
    d_res = torch.full((len(pairs) * RESULT_BYTES,), 99, dtype=torch.uint8, device="cuda")
    d_cart = torch.full((n_images, n, n), float("nan"), dtype=torch.float32, device="cuda") if cart else None
    torch.cuda.synchronize()
    h.register_batch_device(d_imgs.data_ptr(), n_images, istride, rstride, off, d_pairs.data_ptr(), len(pairs), d_res.data_ptr(),
                            d_cart=d_cart.data_ptr() if cart else None)
    torch.cuda.synchronize()
    res = np.frombuffer(d_res.cpu().numpy().tobytes(), dtype=_rsx.PHASECORR_RESULT_DTYPE)
    return (res, d_cart.cpu().numpy()) if cart else res


@pytest.fixture(scope="module")
def runs(pc):
    """name -> (results, [(curve, surface)] per pair) of the host entry on the tight packaging; computed once"""
    out = {}
    for name, c in pcc.cases().items():
        h = _handle(pc, c.rows, c.cols, c.fields)
        res = _host(pc, h, pcc.pack(c.images, padded=False), len(c.images), c.pairs)
        out[name] = (res, [h.correlation(i) for i in range(len(c.pairs))])
        h.close()
    return out


def _same_bits(got, want):
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("name", list(pcc.SHAPES) + list(pcc.DEGENERATE))
def test_cartesian_images_bit_identical(pc, name):
    """every shape, the one-row, two-row and 4096-row scans included: the azimuth wrap of cart_pixel and the range fences"""
    degenerate = name in pcc.DEGENERATE
    sh = pcc.DEGENERATE[name] if degenerate else pcc.SHAPES[name]
    imgs = pcc.degenerate_scans(name) if degenerate else pcc.scans(name)[:3]
    h = _handle(pc, sh.rows, sh.cols, sh.fields)
    res, got = _host(pc, h, pcc.pack(imgs, padded=False), len(imgs), np.zeros((0, 2), dtype=np.int32), cart=True)
    h.close()
    tab = pcn.Tables(dict(pcn.default_params(), **sh.fields), sh.rows, sh.cols)
    n = sh.fields["n"]
    assert len(res) == 0 and got.shape == (len(imgs), n, n)
    for i in range(len(imgs)):
        want = pcn.cart_image(imgs[i], 0, tab)
        assert want.any() and _same_bits(got[i], want), (name, i, np.abs(got[i] - want).max())


def test_cases_against_the_restatement(runs):
    from test_phasecorr_restatement import wrap
    worst = dict(surface=0.0, shift=0.0, angle=0.0)
    for name, c in pcc.cases().items():
        if c.empty:
            continue
        res, corr = runs[name]
        want = pcc.expected(name)[0]
        n, pix = c.fields["n"], c.fields["resolution"]
        for i, (w, (curve, surf)) in enumerate(zip(want, corr)):
            ambiguous = i in c.ambiguous
            ds, dc = np.abs(surf - w["surface"]).max(), np.abs(curve - w["rot_curve"]).max()
            dt = abs(wrap(res["theta"][i] - w["theta"])) / (math.pi / n)
            worst["surface"] = max(worst["surface"], ds, dc, abs(res["rot_peak"][i] - w["rot_peak"]))
            worst["angle"] = max(worst["angle"], dt)
            assert res["half_turn"][i] == w["half_turn"] and res["status"][i] == w["status"] == 0, (name, i)
            if ambiguous:   # no decided peak: the curve, the surface, theta, the one candidate and the status only
                assert res["half_turn"][i] == 0
                print(f"{name} pair {c.pairs[i]} (ambiguous): surface {ds:.3e} curve {dc:.3e} theta {dt:.3e} bins")
                continue
            dx, dy = abs(res["x"][i] - w["x"]) / pix, abs(res["y"][i] - w["y"]) / pix
            dp = abs(res["peak"][i] - w["peak"])
            print(f"{name} pair {c.pairs[i]}: surface {ds:.3e} curve {dc:.3e} peak {dp:.3e} | x {dx:.3e} y {dy:.3e} px theta {dt:.3e} bins | "
                  f"at {w['peak_ij']} k0 {w['rot_k0']} half_turn {w['half_turn']} peak {res['peak'][i]:.4f} ratio {res['peak_ratio'][i]:.4f}")
            worst["surface"] = max(worst["surface"], dp)
            worst["shift"] = max(worst["shift"], dx, dy)
            # the integer peaks are the restatement's
            assert int(np.argmax(curve)) == w["rot_k0"], (name, i)
            assert divmod(int(np.argmax(surf)), n) == w["peak_ij"], (name, i)
            assert abs(res["peak_ratio"][i] - w["peak_ratio"]) <= 2 * SURFACE_BOUND / w["peak"] + 1e-12, (name, i)
    print("measured:", worst)
    assert 2 * SURFACE_BOUND < MARGIN and SHIFT_BOUND < 0.01 and ANGLE_BOUND < 0.01
    assert worst["surface"] <= SURFACE_BOUND and worst["shift"] <= SHIFT_BOUND and worst["angle"] <= ANGLE_BOUND, worst


def test_empty_images(pc, runs):
    """the zero-denominator branches: an all-zero record byte for byte, all-zero surfaces, no NaN"""
    from navtech_radar_slam_amd import _rsx
    c = pcc.cases()["s64-empty"]
    res, corr = runs["s64-empty"]
    zero = np.zeros(len(c.pairs), dtype=_rsx.PHASECORR_RESULT_DTYPE)
    assert res.tobytes() == zero.tobytes() and (res["status"] == 0).all()
    for curve, surf in corr:
        assert not np.isnan(curve).any() and not np.isnan(surf).any()
        assert (curve == 0.0).all() and (surf == 0.0).all()
    h = _handle(pc, c.rows, c.cols, c.fields)
    dev = _device(h, pcc.pack(c.images, padded=False), len(c.images), c.pairs)
    h.close()
    assert dev.tobytes() == zero.tobytes()


@pytest.mark.parametrize("name", ["s64", "s128"])
def test_packaging_does_not_matter(pc, runs, name):
    """col_offset 5, padded rows, padded images, 0xA5 in every spare byte: the bytes of the tight call, through both entries"""
    c = pcc.cases()[name]
    k = len(c.images)
    h = _handle(pc, c.rows, c.cols, c.fields)
    tight, padded = pcc.pack(c.images, padded=False), pcc.pack(c.images, padded=True)
    assert padded[1] > c.rows * padded[2] > c.rows * c.cols and padded[3] == 5 and tight[1:] == (c.rows * c.cols, c.cols, 0)
    want_res, want_cart = _host(pc, h, tight, k, c.pairs, cart=True)
    assert want_res.tobytes() == runs[name][0].tobytes() and not np.isnan(want_cart).any()
    for entry in (lambda p: _host(pc, h, p, k, c.pairs, cart=True), lambda p: _device(h, p, k, c.pairs, cart=True)):
        for p in (padded, tight):
            res, cart = entry(p)
            assert res.tobytes() == want_res.tobytes() and _same_bits(cart, want_cart), name
    h.close()


def _call(pc, h, packed, n_images, pairs):
    res = _host(pc, h, packed, n_images, pairs)
    curve, surf = h.correlation(0)
    return res.tobytes(), curve.tobytes(), surf.tobytes()


def test_one_handle_different_sizes(pc, runs):
    """the workspace layout follows n_images and n_pairs: 7 images and 13 pairs, then 2 and 1, then 7 and 13 again on one handle; each call's
    results and correlation(0) are those of a fresh handle given that call alone"""
    from navtech_radar_slam_amd import _rsx
    c = pcc.cases()["s128"]
    big = (pcc.pack(c.images, padded=False), len(c.images), c.pairs)
    small = (pcc.pack(c.images[[3, 5]], padded=False), 2, [(1, 0)])
    one = _handle(pc, c.rows, c.cols, c.fields)
    got = []
    for step, call in enumerate((big, small, big)):
        got.append(_call(pc, one, *call))
        if step == 1:
            with pytest.raises(_rsx.RsxError):
                one.correlation(1)
        else:
            one.correlation(len(c.pairs) - 1)
    one.close()
    for step, call in enumerate((big, small, big)):
        fresh = _handle(pc, c.rows, c.cols, c.fields)
        assert got[step] == _call(pc, fresh, *call), step
        fresh.close()
    assert got[0] == got[2] and got[0][0] == runs["s128"][0].tobytes()
    # the small call is pair (3, 5) of the seven scans
    h = _handle(pc, c.rows, c.cols, c.fields)
    assert got[1][0] == _host(pc, h, big[0], big[1], [(5, 3)]).tobytes()
    h.close()


@pytest.mark.parametrize("name", ["s128", "s128-one", "s64-one"])
def test_a_pair_alone(pc, runs, name):
    """a pair's bytes do not depend on its place in a batch: at N = 128, and with one candidate (every odd job returns at once)"""
    c = pcc.cases()[name]
    full = runs[name][0]
    h = _handle(pc, c.rows, c.cols, c.fields)
    packed = pcc.pack(c.images, padded=False)
    for i in (1, 3, len(c.pairs) - 1):
        one = _host(pc, h, packed, len(c.images), [c.pairs[i]])
        assert one.tobytes() == full[i:i + 1].tobytes(), (name, i)
    h.close()
