"""The odometry's phase-correlation switch at the C-ABI without a GPU: the header's declarations, the struct's size, the documented
defaults, the Python argument types, and the Odometry constructor's rules, which fire before any handle is made."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rsx():
    import __graft_entry__ as ge
    from navtech_radar_slam_amd import _rsx
    if not os.path.exists(_rsx.LIB_PATH):
        ge.build()
    return _rsx


def test_header_declares_the_switch(rsx):
    with open(os.path.join(ROOT, "include", "rsx.h")) as f:
        h = f.read()
    assert re.search(r"int\s+rsx_odometry_default_phasecorr_params\s*\(\s*rsx_odometry_phasecorr_params\s*\*\s*p\s*\)\s*;", h)
    assert re.search(r"int\s+rsx_odometry_set_phasecorr\s*\(\s*rsx_odometry\s*\*\s*h\s*,\s*const\s+rsx_odometry_phasecorr_params\s*\*\s*params\s*\)\s*;", h)
    for name, value in (("RSX_ESTIMATOR_PHASECORR", 4), ("RSX_ODOMETRY_PHASECORR_ESTIMATE", 0), ("RSX_ODOMETRY_PHASECORR_FALLBACK", 1),
                        ("RSX_ODOMETRY_STATUS_PHASECORR", 16)):
        m = re.search(r"#define\s+" + name + r"\s+(\d+)\b", h)
        assert m and int(m.group(1)) == value, name
    assert (rsx.ESTIMATOR_PHASECORR, rsx.ODOMETRY_PHASECORR_ESTIMATE, rsx.ODOMETRY_PHASECORR_FALLBACK, rsx.ODOMETRY_STATUS_PHASECORR) == (4, 0, 1, 16)
    for name in ("rsx_odometry_default_phasecorr_params", "rsx_odometry_set_phasecorr"):
        assert name in rsx.SYMBOLS


def test_struct_and_argument_types(rsx):
    L = rsx.lib()
    P = C.POINTER(rsx.OdometryPhasecorrParams)
    assert C.sizeof(rsx.OdometryPhasecorrParams) == 64 and C.sizeof(rsx.PhasecorrParams) == 40
    assert [(n, getattr(rsx.OdometryPhasecorrParams, n).offset) for n, _ in rsx.OdometryPhasecorrParams._fields_] == [
        ("pc", 0), ("max_peak_ratio", 40), ("min_peak", 48), ("mode", 56), ("reserved", 60)]
    assert L.rsx_odometry_default_phasecorr_params.argtypes == [P]
    assert L.rsx_odometry_set_phasecorr.argtypes == [C.c_void_p, P]


def test_default_params_need_no_device(rsx):
    L = rsx.lib()
    p = rsx.OdometryPhasecorrParams()
    C.memset(C.byref(p), 0xFF, C.sizeof(p))
    assert L.rsx_odometry_default_phasecorr_params(C.byref(p)) == 0
    d = rsx.PhasecorrParams()
    assert L.rsx_phasecorr_default_params(C.byref(d)) == 0
    assert bytes(p.pc) == bytes(d) and (d.n, d.resolution, d.min_range_bins, d.max_rotation, d.resolve_half_turn) == (256, 0.5, 58, 0.0, 1)
    assert (p.max_peak_ratio, p.min_peak, p.mode, p.reserved) == (0.0, 0.0, rsx.ODOMETRY_PHASECORR_ESTIMATE, 0)
    assert L.rsx_odometry_default_phasecorr_params(None) == -1
    assert L.rsx_odometry_set_phasecorr(None, C.byref(p)) == -1   # a null handle, not a crash
    from navtech_radar_slam_amd import odometry
    assert bytes(odometry.default_phasecorr_params()) == bytes(p)
    q = odometry.phasecorr_params(dict(n=64, resolution=0.9, max_peak_ratio=0.2), mode=rsx.ODOMETRY_PHASECORR_FALLBACK)
    assert (q.pc.n, q.pc.resolution, q.pc.min_range_bins, q.max_peak_ratio, q.min_peak, q.mode) == (64, 0.9, 58, 0.2, 0.0, 1)
    assert bytes(odometry.phasecorr_params(q)) == bytes(q)
    with pytest.raises(TypeError):
        odometry.phasecorr_params(dict(radius=3.0))


def test_constructor_rules_fire_before_a_handle_is_made(rsx, monkeypatch):
    from navtech_radar_slam_amd import odometry

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(odometry, "lib", no_library)
    with pytest.raises(ValueError, match="not both"):
        odometry.Odometry(64, 512, estimator="phasecorr", fallback="phasecorr")
    with pytest.raises(ValueError, match="fallback"):
        odometry.Odometry(64, 512, fallback="cfear")
    with pytest.raises(ValueError, match="estimator"):
        odometry.Odometry(64, 512, estimator="fourier")
    with pytest.raises(ValueError, match="phasecorr parameters"):
        odometry.Odometry(64, 512, phasecorr=dict(n=64))
    with pytest.raises(AssertionError, match="the library was reached"):   # (a valid combination goes on to the library)
        odometry.Odometry(64, 512, estimator="phasecorr")
