"""CPU-side checks of the rsx_coral entries (include/rsx.h): the defaults, the parameter and offset rules (judged before the handle
is looked at, so they need no device) and the no-device behaviour of the create."""
import ctypes as C
import os

import numpy as np
import pytest


@pytest.fixture(scope="module")
def rsx():
    import __graft_entry__ as ge
    from navtech_radar_slam_amd import _rsx
    if not os.path.exists(_rsx.LIB_PATH):
        ge.build()
    return _rsx


def test_create_needs_a_device(rsx):
    L = rsx.lib()
    h = C.c_void_p(1)
    st = L.rsx_coral_create(0, C.byref(h))
    if rsx.device_count() > 0:
        assert st == 0 and h.value
        assert L.rsx_coral_destroy(h) == 0
    else:  # never computed on the CPU: RSX_ERR_NO_DEVICE, and *out cleared
        assert st == -2 and not h.value
        assert b"no HIP device" in L.rsx_last_error_string()
        from navtech_radar_slam_amd import coral
        with pytest.raises(rsx.RsxError):
            coral.Coral()
    assert L.rsx_coral_create(0, None) == -1
    assert L.rsx_coral_destroy(None) == 0


def test_defaults_and_layouts(rsx):
    from navtech_radar_slam_amd import coral
    p = coral.default_params()
    assert (p.radius, p.min_points, p.min_other, p.det_min) == (3.5, 6, 1, 1e-6)
    assert rsx.lib().rsx_coral_default_params(None) == -1
    assert C.sizeof(rsx.CoralParams) == 24 and C.sizeof(rsx.CoralResult) == 40
    assert rsx.CORAL_RESULT_DTYPE.itemsize == 40 and rsx.CORAL_POINT_DTYPE.itemsize == 24
    assert [rsx.CORAL_RESULT_DTYPE.fields[f][1] for f in ("quality", "h_joint", "h_separate", "n_scored", "n_scored_a", "n_valid", "status")] == \
        [0, 8, 16, 24, 28, 32, 36]
    assert coral.params(radius=2.0, min_other=0).radius == 2.0
    with pytest.raises(TypeError):
        coral.params(max_condition=3.0)
    m = coral.pose_matrices([(1.0, 2.0, 0.0), (0.0, 0.0, np.pi / 2)])
    assert m[0].tolist() == [1.0, -0.0, 1.0, 0.0, 1.0, 2.0] and m[1, 1] == -1.0 and m[1, 3] == 1.0


BAD_PARAMS = [({"radius": 0.0}, b"radius"), ({"radius": -1.0}, b"radius"), ({"radius": float("nan")}, b"radius"), ({"radius": float("inf")}, b"radius"),
              ({"min_points": 1}, b"min_points"), ({"min_points": -3}, b"min_points"), ({"min_other": -1}, b"min_other"),
              ({"det_min": 0.0}, b"det_min"), ({"det_min": -1e-6}, b"det_min"), ({"det_min": float("nan")}, b"det_min"),
              ({"det_min": float("inf")}, b"det_min")]


def _call(rsx, handle, a_off, b_off, params=None, n_jobs=None, device=False, stride=2, res=True):
    """the host (or device) entry on dummy buffers: only the argument rules are exercised"""
    L = rsx.lib()
    a_off, b_off = np.asarray(a_off, dtype=np.int64), np.asarray(b_off, dtype=np.int64)
    n = len(a_off) - 1 if n_jobs is None else n_jobs
    xy = np.zeros((max(int(a_off.max()), int(b_off.max()), 1), 2), dtype=np.float32)
    out = np.zeros(max(n, 1), dtype=rsx.CORAL_RESULT_DTYPE)
    pp = C.byref(params) if params is not None else None
    if device:
        return L.rsx_coral_quality_batch_device(handle, xy.ctypes.data, a_off.ctypes.data, xy.ctypes.data, b_off.ctypes.data, stride, n, None, pp,
                                                out.ctypes.data if res else None, None, None)
    return L.rsx_coral_quality_batch(handle, xy.ctypes.data, a_off.ctypes.data, xy.ctypes.data, b_off.ctypes.data, n, None, pp,
                                     out.ctypes.data if res else None, None)


def check_argument_rules(rsx, handle):
    """every violated rule is RSX_ERR_BAD_ARG (-1) with its own message; shared with tests/test_gpu_coral.py, which passes a handle"""
    from navtech_radar_slam_amd import coral
    L = rsx.lib()
    for fields, word in BAD_PARAMS:
        for device in (False, True):
            assert _call(rsx, handle, [0, 4], [0, 4], coral.params(**fields), device=device) == -1, fields
            assert word in L.rsx_last_error_string(), (fields, L.rsx_last_error_string())
    r = rsx.CoralResult()
    assert L.rsx_kfstore_alignment_quality(None, handle, 0, 0, None, C.byref(coral.params(radius=0.0)), C.byref(r)) == -1
    assert b"radius" in L.rsx_last_error_string()
    assert L.rsx_kfstore_alignment_quality(None, handle, 0, 0, None, None, None) == -1
    for a_off, b_off, word in (([1, 4], [0, 4], b"start at 0"), ([0, 4], [2, 4], b"start at 0"), ([0, 4, 3], [0, 1, 2], b"not decrease"),
                               ([0, 1, 2], [0, 5, 4], b"not decrease"), ([0, -1], [0, 1], b"not decrease"),
                               ([0, rsx.CORAL_MAX_POINTS + 1], [0, 4], b"more than 8192"), ([0, 4, 8], [0, 4, 4 + rsx.CORAL_MAX_POINTS + 1], b"more than 8192")):
        assert _call(rsx, handle, a_off, b_off) == -1, (a_off, b_off)
        assert word in L.rsx_last_error_string(), (a_off, b_off, L.rsx_last_error_string())
    assert _call(rsx, handle, [0, 4], [0, 4], n_jobs=-1) == -1
    assert _call(rsx, handle, [0, 4], [0, 4], res=False) == -1
    assert _call(rsx, handle, [0, 4], [0, 4], device=True, res=False) == -1
    for stride in (1, 0, -4):
        assert _call(rsx, handle, [0, 4], [0, 4], device=True, stride=stride) == -1
        assert b"point_stride" in L.rsx_last_error_string()


def test_argument_rules_need_no_device(rsx):
    check_argument_rules(rsx, None)
    # with every rule kept, what is left to refuse is the handle
    assert _call(rsx, None, [0, 4], [0, 4]) == -1 and b"null handle" in rsx.lib().rsx_last_error_string()
    assert _call(rsx, None, [0, rsx.CORAL_MAX_POINTS], [0, rsx.CORAL_MAX_POINTS]) == -1 and b"null handle" in rsx.lib().rsx_last_error_string()
    assert _call(rsx, None, [0, 4], [0, 4], device=True) == -1 and b"null handle" in rsx.lib().rsx_last_error_string()
