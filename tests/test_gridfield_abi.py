"""CPU-side checks of the likelihood-field entries (include/rsx.h, rsx_gridmap_field_* and rsx_gridmap_likelihood_field): the layout of
the struct against navtech_radar_slam_amd._rsx and the restatement, the defaults, the parameter rules, which are judged before the
handle or the device is looked at and so need no device, and the host-only Gaussian table against tests/gridfield_np.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gridfield_np as gf  # noqa: E402


@pytest.fixture(scope="module")
def rsx():
    import __graft_entry__ as ge
    from navtech_radar_slam_amd import _rsx
    if not os.path.exists(_rsx.LIB_PATH):
        ge.build()
    return _rsx


def test_struct_size_and_defaults(rsx):
    from navtech_radar_slam_amd import gridmap
    names = ("threshold", "radius", "reserved0", "reserved1")
    offsets = [0, 4, 8, 12]
    assert C.sizeof(rsx.GridmapFieldParams) == 16 == gf.PARAMS.itemsize
    assert [getattr(rsx.GridmapFieldParams, f).offset for f in names] == offsets
    assert gf.PARAMS.names == names and [gf.PARAMS.fields[f][1] for f in names] == offsets
    p = gridmap.default_field_params()
    assert (p.threshold, p.radius, p.reserved0, p.reserved1) == (50, 12, 0, 0)
    assert gf.DEFAULTS == dict(threshold=50, radius=12) and (gf.DEFAULT_SIGMA, gf.DEFAULT_PEAK) == (3.0, 255)
    assert rsx.GRIDMAP_FIELD_MAX_RADIUS == 64 == gf.MAX_RADIUS
    assert rsx.lib().rsx_gridmap_field_default_params(None) == -1
    assert gridmap.field_params(radius=7).radius == 7
    with pytest.raises(TypeError):
        gridmap.field_params(sigma=3.0)


BAD_PARAMS = [({"threshold": 0}, b"threshold"), ({"threshold": 256}, b"threshold"), ({"threshold": -5}, b"threshold"), ({"radius": 0}, b"radius"),
              ({"radius": 65}, b"radius"), ({"radius": -1}, b"radius"), ({"reserved0": 1}, b"reserved"), ({"reserved1": -1}, b"reserved")]
GOOD_PARAMS = [{"threshold": 1, "radius": 1}, {"threshold": 255, "radius": 64}, {}]


def check_parameter_rules(rsx, handle):
    """every rule of rsx_gridmap_field_params, with and without a table; shared with tests/test_gpu_gridfield.py, which passes a handle
    (with handle None every call ends at "null handle" at the latest: nothing is launched)"""
    from navtech_radar_slam_amd import gridmap
    L = rsx.lib()
    table = np.zeros(64 * 64 + 1, dtype=np.uint8)
    for tp in (None, table.ctypes.data):
        for fields, word in BAD_PARAMS:
            assert L.rsx_gridmap_likelihood_field(handle, C.byref(gridmap.field_params(**fields)), tp, None) == -1, fields
            assert word in L.rsx_last_error_string(), (fields, L.rsx_last_error_string())


def test_parameter_rules_need_no_device(rsx):
    from navtech_radar_slam_amd import gridmap
    L = rsx.lib()
    check_parameter_rules(rsx, None)
    # with every rule kept, what is left to refuse is the handle
    table = np.zeros(64 * 64 + 1, dtype=np.uint8)
    calls = [L.rsx_gridmap_likelihood_field(None, None, None, None), L.rsx_gridmap_likelihood_field(None, None, table.ctypes.data, None)]
    calls += [L.rsx_gridmap_likelihood_field(None, C.byref(gridmap.field_params(**fields)), table.ctypes.data, None) for fields in GOOD_PARAMS]
    for st in calls:
        assert st == -1 and b"null handle" in L.rsx_last_error_string()


NAN, INF = float("nan"), float("inf")


def test_gaussian_table_refusals(rsx):
    from navtech_radar_slam_amd import gridmap
    L = rsx.lib()
    out = np.full(64 * 64 + 1, 0xAB, dtype=np.uint8)
    bad = [((0.0, 255, 12), b"sigma"), ((-1.0, 255, 12), b"sigma"), ((NAN, 255, 12), b"sigma"), ((INF, 255, 12), b"sigma"),
           ((3.0, 0, 12), b"peak"), ((3.0, 256, 12), b"peak"), ((3.0, 255, 0), b"radius"), ((3.0, 255, 65), b"radius")]
    for (sigma, peak, radius), word in bad:
        assert L.rsx_gridmap_field_gaussian_table(sigma, peak, radius, out.ctypes.data) == -1, (sigma, peak, radius)
        assert word in L.rsx_last_error_string(), (sigma, peak, radius, L.rsx_last_error_string())
    assert L.rsx_gridmap_field_gaussian_table(3.0, 255, 12, None) == -1 and b"null out" in L.rsx_last_error_string()
    assert (out == 0xAB).all()
    for args in ((0.0, 12), (NAN, 12), (3.0, 12, 0), (3.0, 12, 256), (3.0, 0), (3.0, 65)):
        with pytest.raises(rsx.RsxError):
            gridmap.gaussian_table(*args)
    # and exactly radius^2 + 1 bytes are written
    assert L.rsx_gridmap_field_gaussian_table(1e-3, 1, 1, out.ctypes.data) == 0
    assert out[:3].tolist() == [1, 0, 0xAB] and (out[2:] == 0xAB).all()


@pytest.mark.parametrize("sigma,radius", [(1.5, 6), (3.0, 12), (20.0, 64)])
@pytest.mark.parametrize("peak", [255, 100, 1])
def test_gaussian_table_equals_the_restatement(rsx, sigma, radius, peak):
    """the two exponentials may differ in their last bit, which the rounding hides unless an unrounded entry sits on a half: none of
    these (sigma, radius, peak) comes within 1e-9 of one (asserted first; the closest, at sigma 20, is 6.8e-5 away)"""
    from navtech_radar_slam_amd import gridmap
    raw = gf.gaussian_unrounded(sigma, radius, peak)
    to_half = np.abs(raw - np.floor(raw) - 0.5)
    assert to_half.min() > 1e-9, (to_half.min(), int(to_half.argmin()))
    want = gf.gaussian_table(sigma, radius, peak)
    got = gridmap.gaussian_table(sigma, radius, peak)
    assert got.dtype == np.uint8 and got.shape == (radius * radius + 1,) and got.tobytes() == want.tobytes()
    assert got[0] == peak and (np.diff(got.astype(np.int32)) <= 0).all()
    assert got[-1] == int(np.floor(peak * np.exp(-radius * radius / (2.0 * sigma * sigma)) + 0.5))
