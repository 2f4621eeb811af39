"""The CFAR entries at the C-ABI without a GPU: the documented defaults, no CPU fall-back, and the Python argument types."""
import ctypes as C
import os

import pytest

NO_DEVICE = -2  # RSX_ERR_NO_DEVICE


@pytest.fixture(scope="module")
def rsx():
    import __graft_entry__ as ge
    from navtech_radar_slam_amd import _rsx
    if not os.path.exists(_rsx.LIB_PATH):
        ge.build()
    return _rsx


def test_default_params(rsx):
    p = rsx.CfarParams(*([-1] * 10))
    assert rsx.lib().rsx_cfar_default_params(C.byref(p)) == 0
    # k, train, guard, mode, min_range, max_range, min_separation are fixed by the rule's description; scale_q8 and offset by the
    # defaults study of include/rsx.h (a = 3, b = 20)
    assert (p.k, p.train, p.guard, p.mode, p.min_range, p.max_range, p.min_separation, p.reserved) == (12, 20, 2, 0, 58, 0, 5, 0)
    assert (p.scale_q8, p.offset) == (768, 20)
    assert rsx.lib().rsx_cfar_default_params(None) == -1
    from navtech_radar_slam_amd import cfar
    d = cfar.default_params()
    assert bytes(d) == bytes(p)
    q = cfar.params(scale_q8=0, offset=59, mode=cfar.CFAR_GO)
    assert (q.scale_q8, q.offset, q.mode, q.k, q.train) == (0, 59, 1, 12, 20)
    with pytest.raises(TypeError):
        cfar.params(z_min=3)


def test_no_cpu_fallback(rsx):
    if rsx.device_count() > 0:
        pytest.skip("a GPU is visible here")
    h = C.c_void_p(1)
    assert rsx.lib().rsx_cfar_create(0, 400, 3360, C.byref(h)) == NO_DEVICE
    assert not h.value


def test_argument_types_are_set(rsx):
    L = rsx.lib()
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    P = C.POINTER(rsx.CfarParams)
    assert L.rsx_cfar_extract.argtypes == [vp, vp, i32, i32, P, vp, C.c_float, vp, vp, i32, C.POINTER(i32)]
    assert L.rsx_cfar_extract_batch.argtypes == [vp, vp, i32, i64, i32, i32, P, vp, i32, C.c_float, vp, vp, i32, vp]
    assert L.rsx_cfar_extract_batch_device.argtypes == [vp, vp, i32, i64, i32, i32, P, vp, i32, C.c_float, vp, vp, i32, vp, vp]
    assert L.rsx_odometry_set_cfar.argtypes == [vp, P]
    assert L.rsx_cfar_create.argtypes == [C.c_int, i32, i32, C.POINTER(vp)] and L.rsx_cfar_destroy.argtypes == [vp]
    assert C.sizeof(rsx.CfarParams) == 40
    for name in ("rsx_cfar_default_params", "rsx_cfar_create", "rsx_cfar_destroy", "rsx_cfar_extract", "rsx_cfar_extract_batch",
                 "rsx_cfar_extract_batch_device", "rsx_odometry_set_cfar"):
        assert name in rsx.SYMBOLS
