"""CPU-side checks of the rsx_gridmap entries (include/rsx.h): the defaults and the layout of the parameter struct, the parameter, pointer
and window rules (judged before the handle or the device is looked at, so they need no device) and the no-device behaviour of the
create."""
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
    st = L.rsx_gridmap_create(0, 400, 3360, None, C.byref(h))
    if rsx.device_count() > 0:
        assert st == 0 and h.value
        assert L.rsx_gridmap_destroy(h) == 0
    else:  # never computed on the CPU: RSX_ERR_NO_DEVICE, and *out cleared
        assert st == -2 and not h.value
        assert b"no HIP device" in L.rsx_last_error_string()
        from navtech_radar_slam_amd import gridmap
        with pytest.raises(rsx.RsxError):
            gridmap.GridMap(400, 3360)
    assert L.rsx_gridmap_create(0, 400, 3360, None, None) == -1
    assert L.rsx_gridmap_destroy(None) == 0


def test_defaults_and_layout(rsx):
    from navtech_radar_slam_amd import gridmap
    p = gridmap.default_params()
    assert (p.width, p.height, p.resolution, p.origin_x, p.origin_y) == (1024, 1024, 0.5, -256.0, -256.0)
    assert (p.range_resolution, p.min_range_bins, p.range_halfwidth, p.hit_threshold, p.max_range, p.reserved) == (0.0595, 58, 4, 120, 0.0, 0)
    assert p.range_halfwidth == int(p.resolution / (2 * p.range_resolution))
    assert rsx.lib().rsx_gridmap_default_params(None) == -1
    assert C.sizeof(rsx.GridmapParams) == 64
    assert [getattr(rsx.GridmapParams, f).offset for f in ("width", "height", "resolution", "origin_x", "origin_y", "range_resolution", "max_range",
                                                            "min_range_bins", "range_halfwidth", "hit_threshold", "reserved")] == \
        [0, 4, 8, 16, 24, 32, 40, 48, 52, 56, 60]
    assert (rsx.GRIDMAP_MEAN, rsx.GRIDMAP_HITS, rsx.GRIDMAP_STATUS_TRANSFORM) == (0, 1, 1)
    assert gridmap.params(width=128, max_range=50.0).max_range == 50.0
    with pytest.raises(TypeError):
        gridmap.params(cell_size=1.0)
    # the restatement's defaults are the library's
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import gridmap_np
    assert gridmap_np.DEFAULTS == {k: getattr(p, k) for k in gridmap_np.DEFAULTS}


NAN, INF = float("nan"), float("inf")
BAD_PARAMS = [({"width": 0}, b"width"), ({"width": 32}, b"width"), ({"width": 100}, b"width"), ({"width": 8256}, b"width"), ({"width": -64}, b"width"),
              ({"height": 0}, b"height"), ({"height": 96}, b"height"), ({"height": 16384}, b"height"),
              ({"resolution": 0.0}, b"resolution"), ({"resolution": -0.5}, b"resolution"), ({"resolution": NAN}, b"resolution"),
              ({"resolution": INF}, b"resolution"), ({"origin_x": NAN}, b"origin"), ({"origin_y": INF}, b"origin"),
              ({"range_resolution": 0.0}, b"range_resolution"), ({"range_resolution": -1.0}, b"range_resolution"),
              ({"range_resolution": NAN}, b"range_resolution"), ({"range_resolution": INF}, b"range_resolution"),
              ({"min_range_bins": -1}, b"min_range_bins"), ({"range_halfwidth": -1}, b"range_halfwidth"), ({"range_halfwidth": 8193}, b"range_halfwidth"),
              ({"hit_threshold": -1}, b"hit_threshold"), ({"hit_threshold": 256}, b"hit_threshold"),
              ({"max_range": -1.0}, b"max_range"), ({"max_range": NAN}, b"max_range"), ({"max_range": INF}, b"max_range")]


def test_parameter_rules_need_no_device(rsx):
    """every violated rule is RSX_ERR_BAD_ARG (-1) with its own message, whatever the device"""
    from navtech_radar_slam_amd import gridmap
    L = rsx.lib()
    for fields, word in BAD_PARAMS:
        for device in (0, 9999):
            h = C.c_void_p(1)
            assert L.rsx_gridmap_create(device, 400, 3360, C.byref(gridmap.params(**fields)), C.byref(h)) == -1, fields
            assert word in L.rsx_last_error_string(), (fields, L.rsx_last_error_string())
            assert not h.value
    for rows, cols in ((0, 3360), (4097, 3360), (400, 1), (400, 8193), (-1, -1)):
        h = C.c_void_p(1)
        assert L.rsx_gridmap_create(0, rows, cols, None, C.byref(h)) == -1 and not h.value
        assert b"image shape" in L.rsx_last_error_string()
    # the smallest and the largest legal values pass the rules: what is left to refuse is the device
    if rsx.device_count() == 0:
        for fields in ({"width": 64, "height": 8192}, {"hit_threshold": 0}, {"hit_threshold": 255}, {"min_range_bins": 0, "range_halfwidth": 0},
                       {"range_halfwidth": 8192}, {"max_range": 1e-3}):
            h = C.c_void_p(1)
            assert L.rsx_gridmap_create(0, 1, 2, C.byref(gridmap.params(**fields)), C.byref(h)) == -2, fields


def check_argument_rules(rsx, handle, rows=400, cols=3360, width=1024, height=1024):
    """the NULL-pointer, batch and window rules on dummy host buffers; shared with tests/test_gpu_gridmap.py, which passes a handle
    (with handle None every call ends at "null handle" at the latest: nothing is launched)"""
    L = rsx.lib()
    img = np.zeros((1, rows, cols + 11), dtype=np.uint8)
    tf = np.array([[1.0, 0.0, 0.0, 0.0, 1.0, 0.0]])
    ip, tp, stride = img.ctypes.data, tf.ctypes.data, cols + 11
    for entry, tail in ((L.rsx_gridmap_add_batch, ()), (L.rsx_gridmap_add_batch_device, (None, None))):
        assert entry(handle, None, 1, img.strides[0], stride, 11, tp, *tail) == -1
        assert entry(handle, ip, 1, img.strides[0], stride, 11, None, *tail) == -1
        assert entry(handle, ip, -1, img.strides[0], stride, 11, tp, *tail) == -1
        if handle is not None:
            assert entry(handle, ip, 1, img.strides[0], cols + 10, 11, tp, *tail) == -1 and b"row_stride" in L.rsx_last_error_string()
            assert entry(handle, ip, 1, img.strides[0], stride, -1, tp, *tail) == -1 and b"row_stride" in L.rsx_last_error_string()
            assert entry(handle, ip, 2, img.strides[0] - 1, stride, 11, np.tile(tf, (2, 1)).ctypes.data, *tail) == -1
            assert b"image_stride_bytes" in L.rsx_last_error_string()
            assert entry(handle, None, 0, 0, stride, 11, None, *tail) == 0          # an empty batch is no error
    for k in range(6):   # the host entry refuses a non-finite transform before it looks at the handle
        for bad in (NAN, INF, -INF):
            t = tf.copy()
            t[0, k] = bad
            assert L.rsx_gridmap_add_batch(handle, ip, 1, img.strides[0], stride, 11, t.ctypes.data) == -1
            assert b"not finite" in L.rsx_last_error_string()
    out = np.zeros((height, width), dtype=np.uint32)
    op = out.ctypes.data
    for mode, mo, word in ((2, 1, b"render mode"), (-1, 1, b"render mode"), (0, 0, b"min_observations"), (1, -3, b"min_observations")):
        assert L.rsx_gridmap_render(handle, mode, mo, 0, 0, 1, 1, op) == -1 and word in L.rsx_last_error_string()
        assert L.rsx_gridmap_render_device(handle, mode, mo, 0, 0, 1, 1, op, None) == -1 and word in L.rsx_last_error_string()
    assert L.rsx_gridmap_render(handle, 0, 1, 0, 0, 1, 1, None) == -1
    assert L.rsx_gridmap_render_device(handle, 0, 1, 0, 0, 1, 1, None, None) == -1
    if handle is not None:
        for x, y, w, h in ((-1, 0, 1, 1), (0, -1, 1, 1), (0, 0, 0, 1), (0, 0, 1, 0), (0, 0, width + 1, 1), (0, 0, 1, height + 1), (width, 0, 1, 1),
                           (0, height, 1, 1), (width - 1, 0, 2, 1), (0, height - 1, 1, 2), (1, 0, 2**31 - 1, 1), (0, 1, 1, 2**31 - 1)):
            assert L.rsx_gridmap_read(handle, x, y, w, h, op, None, None) == -1 and b"window" in L.rsx_last_error_string(), (x, y, w, h)
            assert L.rsx_gridmap_render(handle, 0, 1, x, y, w, h, op) == -1 and b"window" in L.rsx_last_error_string(), (x, y, w, h)
            assert L.rsx_gridmap_render_device(handle, 1, 1, x, y, w, h, op, None) == -1 and b"window" in L.rsx_last_error_string(), (x, y, w, h)


def test_argument_rules_need_no_device(rsx):
    L = rsx.lib()
    check_argument_rules(rsx, None)
    # with every rule kept, what is left to refuse is the handle
    img = np.zeros((1, 400, 3371), dtype=np.uint8)
    tf = np.array([[1.0, 0.0, 0.0, 0.0, 1.0, 0.0]])
    out = np.zeros(4, dtype=np.uint32)
    p = [C.c_void_p() for _ in range(3)]
    for st in (L.rsx_gridmap_add_batch(None, img.ctypes.data, 1, img.strides[0], 3371, 11, tf.ctypes.data),
               L.rsx_gridmap_add_batch_device(None, img.ctypes.data, 1, img.strides[0], 3371, 11, tf.ctypes.data, None, None),
               L.rsx_gridmap_clear(None, None), L.rsx_gridmap_read(None, 0, 0, 1, 1, out.ctypes.data, None, None),
               L.rsx_gridmap_planes_device(None, C.byref(p[0]), C.byref(p[1]), C.byref(p[2]), None),
               L.rsx_gridmap_render(None, 0, 1, 0, 0, 1, 1, out.ctypes.data), L.rsx_gridmap_render_device(None, 1, 3, 0, 0, 1, 1, out.ctypes.data, None)):
        assert st == -1 and b"null handle" in L.rsx_last_error_string()
