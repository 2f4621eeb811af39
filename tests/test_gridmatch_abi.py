"""CPU-side checks of the rsx_gridmap_match_* and rsx_gridmap_likelihood_* entries (include/rsx.h): the layout of the structs against
navtech_radar_slam_amd._rsx, the defaults, and the parameter and argument rules, which are judged before the handle or the device is
looked at and so need no device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gridmatch_np as gx  # noqa: E402


@pytest.fixture(scope="module")
def rsx():
    import __graft_entry__ as ge
    from navtech_radar_slam_amd import _rsx
    if not os.path.exists(_rsx.LIB_PATH):
        ge.build()
    return _rsx


def test_struct_sizes_and_defaults(rsx):
    from navtech_radar_slam_amd import gridmap
    assert C.sizeof(rsx.GridmapMatchParams) == 24
    assert [getattr(rsx.GridmapMatchParams, f).offset for f in ("angle_step", "angle_steps", "x_cells", "y_cells", "reserved")] == [0, 8, 12, 16, 20]
    assert C.sizeof(rsx.GridmapMatchResult) == 88 == rsx.GRIDMAP_MATCH_RESULT_DTYPE.itemsize == gx.RESULT.itemsize
    names = ("transform", "k", "u", "v", "score", "score_prior", "score_runner_up", "n_points", "n_inside", "status", "reserved")
    offsets = [0, 48, 52, 56, 60, 64, 68, 72, 76, 80, 84]
    assert [getattr(rsx.GridmapMatchResult, f).offset for f in names] == offsets
    for dt in (rsx.GRIDMAP_MATCH_RESULT_DTYPE, gx.RESULT):
        assert dt.names == names and [dt.fields[f][1] for f in names] == offsets
    assert (rsx.GRIDMAP_MATCH_MAX_POINTS, gx.MAX_POINTS) == (8192, 8192)
    assert (rsx.GRIDMAP_MATCH_STATUS_TRANSFORM, rsx.GRIDMAP_MATCH_STATUS_POINTS, rsx.GRIDMAP_MATCH_STATUS_EMPTY) == (1, 2, 4)
    assert (gx.STATUS_TRANSFORM, gx.STATUS_POINTS, gx.STATUS_EMPTY) == (1, 2, 4)
    p = gridmap.default_match_params()
    assert gx.DEFAULTS == {k: getattr(p, k) for k in gx.DEFAULTS} and p.reserved == 0
    assert rsx.lib().rsx_gridmap_match_default_params(None) == -1
    assert gridmap.match_params(x_cells=3).x_cells == 3
    with pytest.raises(TypeError):
        gridmap.match_params(cells=3)


NAN, INF = float("nan"), float("inf")
BAD_PARAMS = [({"angle_steps": -1}, b"angle_steps"), ({"angle_steps": 65}, b"angle_steps"), ({"angle_step": 0.0}, b"angle_step"),
              ({"angle_step": -0.01}, b"angle_step"), ({"angle_step": NAN}, b"angle_step"), ({"angle_step": INF}, b"angle_step"),
              ({"x_cells": -1}, b"x_cells"), ({"x_cells": 33}, b"x_cells"), ({"y_cells": -1}, b"y_cells"), ({"y_cells": 33}, b"y_cells"),
              ({"reserved": 1}, b"reserved")]
GOOD_PARAMS = [{"angle_steps": 0, "angle_step": 0.0}, {"angle_steps": 0, "angle_step": NAN}, {"angle_steps": 64, "x_cells": 32, "y_cells": 32},
               {"x_cells": 0, "y_cells": 0}]


def _buffers(n_points=5):
    xy = np.zeros((n_points, 2), dtype=np.float32)
    off = np.array([0, n_points], dtype=np.int64)
    tf = np.array([[1.0, 0.0, 0.0, 0.0, 1.0, 0.0]])
    res = np.zeros(1, dtype=gx.RESULT)
    return xy, off, tf, res


def check_argument_rules(rsx, handle):
    """every rule of the two match entries on dummy host buffers; shared with tests/test_gpu_gridmatch.py, which passes a handle (with
    handle None every call ends at "null handle" at the latest: nothing is launched)"""
    from navtech_radar_slam_amd import gridmap
    L = rsx.lib()
    xy, off, tf, res = _buffers()
    ptrs = (xy.ctypes.data, off.ctypes.data, tf.ctypes.data, res.ctypes.data)

    def host(p, xyp=ptrs[0], offp=ptrs[1], n=1, tfp=ptrs[2], resp=ptrs[3]):
        return L.rsx_gridmap_match_batch(handle, xyp, offp, n, tfp, p, resp, None)

    def device(p, xyp=ptrs[0], offp=ptrs[1], stride=2, n=1, tfp=ptrs[2], resp=ptrs[3]):
        return L.rsx_gridmap_match_batch_device(handle, xyp, offp, stride, n, tfp, p, resp, None, None)

    for entry in (host, device):
        for fields, word in BAD_PARAMS:
            assert entry(C.byref(gridmap.match_params(**fields))) == -1, fields
            assert word in L.rsx_last_error_string(), (fields, L.rsx_last_error_string())
        for kw in ({"xyp": None}, {"offp": None}, {"tfp": None}, {"resp": None}, {"n": -1}):
            assert entry(None, **kw) == -1, kw
    for stride in (1, 0, -2):
        assert device(None, stride=stride) == -1 and b"point_stride" in L.rsx_last_error_string()
    assert device(C.byref(gridmap.match_params(angle_steps=64)), n=2**31 - 1) == -1 and b"2^31" in L.rsx_last_error_string()
    # the host entry looks at the offsets and at the size of every job
    for bad in ([1, 5], [0, -1]):
        o = np.array(bad, dtype=np.int64)
        assert host(None, offp=o.ctypes.data) == -1 and b"offsets" in L.rsx_last_error_string()
    big = np.zeros((gx.MAX_POINTS + 1, 2), dtype=np.float32)
    o = np.array([0, 3, gx.MAX_POINTS + 4], dtype=np.int64)
    t2, r2 = np.tile(tf, (2, 1)), np.zeros(2, dtype=gx.RESULT)
    assert host(None, xyp=big.ctypes.data, offp=o.ctypes.data, n=2, tfp=t2.ctypes.data, resp=r2.ctypes.data) == -1
    assert b"job 1 has 8193 points" in L.rsx_last_error_string()
    # the likelihood entries
    for mode, mo, word in ((2, 1, b"render mode"), (-1, 1, b"render mode"), (0, 0, b"min_observations"), (1, -3, b"min_observations")):
        assert L.rsx_gridmap_likelihood_update(handle, mode, mo, None) == -1 and word in L.rsx_last_error_string()
    assert L.rsx_gridmap_likelihood_set(handle, None) == -1
    assert L.rsx_gridmap_likelihood_read(handle, 0, 0, 1, 1, None) == -1
    return host, device


def test_argument_rules_need_no_device(rsx):
    from navtech_radar_slam_amd import gridmap
    L = rsx.lib()
    host, device = check_argument_rules(rsx, None)
    # with every rule kept, what is left to refuse is the handle
    out = np.zeros(4, dtype=np.uint8)
    d, pitch = C.c_void_p(), C.c_int64()
    calls = [host(None), device(None), device(None, stride=4), L.rsx_gridmap_likelihood_update(None, 0, 1, None), L.rsx_gridmap_likelihood_update(None, 1, 3, None),
             L.rsx_gridmap_likelihood_set(None, out.ctypes.data), L.rsx_gridmap_likelihood_read(None, 0, 0, 1, 1, out.ctypes.data),
             L.rsx_gridmap_likelihood_device(None, C.byref(d), C.byref(pitch))]
    calls += [entry(C.byref(gridmap.match_params(**fields))) for entry in (host, device) for fields in GOOD_PARAMS]
    xy, off, tf, res = _buffers(gx.MAX_POINTS)      # a job AT the cap is no error
    calls.append(L.rsx_gridmap_match_batch(None, xy.ctypes.data, off.ctypes.data, 1, tf.ctypes.data, None, res.ctypes.data, None))
    tf[0, 2] = NAN                                   # nor is a non-finite prior: the job is skipped with a status
    calls.append(L.rsx_gridmap_match_batch(None, xy.ctypes.data, off.ctypes.data, 1, tf.ctypes.data, None, res.ctypes.data, None))
    for st in calls:
        assert st == -1 and b"null handle" in L.rsx_last_error_string()


def test_match_before_a_likelihood_is_refused(rsx):
    """a handle that has had no likelihood_update and no likelihood_set refuses to match and to read, and writes nothing.  A handle
    needs a device: without one the create is refused (RSX_ERR_NO_DEVICE), which is all that can be seen here; with one the refusal
    is checked here as in tests/test_gpu_gridmatch.py"""
    from navtech_radar_slam_amd import gridmap
    if rsx.device_count() == 0:
        with pytest.raises(rsx.RsxError):
            gridmap.GridMap(64, 96, gridmap.params(width=64, height=64))
        return
    check_refused_before_a_likelihood(rsx)


def check_refused_before_a_likelihood(rsx):
    from navtech_radar_slam_amd import gridmap
    L = rsx.lib()
    m = gridmap.GridMap(64, 96, gridmap.params(width=64, height=64))
    xy, off, tf, res = _buffers()
    res.view(np.uint8)[:] = 0xAB
    vol = np.full(17 * 17 * 17, 0xABABABAB, dtype=np.uint32)
    for st in (L.rsx_gridmap_match_batch(m.handle, xy.ctypes.data, off.ctypes.data, 1, tf.ctypes.data, None, res.ctypes.data, vol.ctypes.data),
               L.rsx_gridmap_match_batch_device(m.handle, xy.ctypes.data, off.ctypes.data, 2, 1, tf.ctypes.data, None, res.ctypes.data, vol.ctypes.data, None),
               L.rsx_gridmap_likelihood_read(m.handle, 0, 0, 1, 1, vol.ctypes.data)):
        assert st == -1 and b"no likelihood" in L.rsx_last_error_string()
    assert (res.view(np.uint8) == 0xAB).all() and (vol == 0xABABABAB).all()
    with pytest.raises(rsx.RsxError):
        m.match([xy], tf)
    m.set_likelihood(np.zeros((64, 64), dtype=np.uint8))
    assert m.match([xy], tf)[0]["status"] == gx.STATUS_EMPTY
    m.close()
