"""CPU-side checks of the rsx_gridmap_search_* entries (include/rsx.h): the layout of the structs against
navtech_radar_slam_amd._rsx and tests/gridsearch_np.py, the defaults, and the parameter and argument rules, which are judged before the
handle or the device is looked at and so need no device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gridsearch_np as gs  # noqa: E402


@pytest.fixture(scope="module")
def rsx():
    import __graft_entry__ as ge
    from navtech_radar_slam_amd import _rsx
    if not os.path.exists(_rsx.LIB_PATH):
        ge.build()
    return _rsx


def test_struct_sizes_and_defaults(rsx):
    from navtech_radar_slam_amd import gridmap
    assert C.sizeof(rsx.GridmapSearchParams) == 24
    assert [getattr(rsx.GridmapSearchParams, f).offset for f in ("angle_step", "angle_steps", "x_cells", "y_cells", "min_score")] == [0, 8, 12, 16, 20]
    assert C.sizeof(rsx.GridmapSearchResult) == 96 == rsx.GRIDMAP_SEARCH_RESULT_DTYPE.itemsize == gs.RESULT.itemsize
    names = ("transform", "k", "u", "v", "score", "score_prior", "bound_runner_up", "n_points", "n_inside", "status", "n_blocks", "n_refined", "reserved")
    offsets = [0, 48, 52, 56, 60, 64, 68, 72, 76, 80, 84, 88, 92]
    assert [getattr(rsx.GridmapSearchResult, f).offset for f in names] == offsets
    for dt in (rsx.GRIDMAP_SEARCH_RESULT_DTYPE, gs.RESULT):
        assert dt.names == names and [dt.fields[f][1] for f in names] == offsets
    # the fields shared with rsx_gridmap_match_result lie where they lie there
    for f in gs.SHARED:
        assert getattr(rsx.GridmapSearchResult, f).offset == getattr(rsx.GridmapMatchResult, f).offset
    assert (rsx.GRIDMAP_SEARCH_STATUS_BELOW, gs.STATUS_BELOW) == (8, 8)
    assert (rsx.GRIDMAP_SEARCH_MAX_CELLS, rsx.GRIDMAP_SEARCH_MAX_ANGLE_STEPS) == (gs.MAX_CELLS, gs.MAX_ANGLE_STEPS) == (256, 180)
    p = gridmap.default_search_params()
    assert gs.DEFAULTS == {k: getattr(p, k) for k in gs.DEFAULTS} == dict(angle_step=0.01, angle_steps=32, x_cells=64, y_cells=64, min_score=0)
    assert rsx.lib().rsx_gridmap_search_default_params(None) == -1
    assert gridmap.search_params(x_cells=3, min_score=7).min_score == 7
    with pytest.raises(TypeError):
        gridmap.search_params(cells=3)
    assert gridmap.search_blocks(gridmap.search_params(angle_steps=2, x_cells=4, y_cells=3)) == (5, 1, 2)
    assert gridmap.search_blocks(gridmap.search_params(angle_steps=180, x_cells=256, y_cells=0)) == (361, 1, 65)


NAN, INF = float("nan"), float("inf")
BAD_PARAMS = [({"angle_steps": -1}, b"angle_steps"), ({"angle_steps": 181}, b"angle_steps"), ({"angle_step": 0.0}, b"angle_step"),
              ({"angle_step": -0.01}, b"angle_step"), ({"angle_step": NAN}, b"angle_step"), ({"angle_step": INF}, b"angle_step"),
              ({"x_cells": -1}, b"x_cells"), ({"x_cells": 257}, b"x_cells"), ({"y_cells": -1}, b"y_cells"), ({"y_cells": 257}, b"y_cells")]
GOOD_PARAMS = [{"angle_steps": 0, "angle_step": 0.0}, {"angle_steps": 0, "angle_step": NAN}, {"angle_steps": 180, "x_cells": 256, "y_cells": 256},
               {"x_cells": 0, "y_cells": 0}, {"min_score": 2**32 - 1}]


def _buffers(n_points=5):
    xy = np.zeros((n_points, 2), dtype=np.float32)
    off = np.array([0, n_points], dtype=np.int64)
    tf = np.array([[1.0, 0.0, 0.0, 0.0, 1.0, 0.0]])
    res = np.zeros(1, dtype=gs.RESULT)
    return xy, off, tf, res


def check_argument_rules(rsx, handle):
    """every rule of the search entries on dummy host buffers; shared with tests/test_gpu_gridsearch.py, which passes a handle (with
    handle None every call ends at "null handle" at the latest: nothing is launched)"""
    from navtech_radar_slam_amd import gridmap
    L = rsx.lib()
    xy, off, tf, res = _buffers()
    ptrs = (xy.ctypes.data, off.ctypes.data, tf.ctypes.data, res.ctypes.data)

    def host(p, xyp=ptrs[0], offp=ptrs[1], n=1, tfp=ptrs[2], resp=ptrs[3]):
        return L.rsx_gridmap_search_batch(handle, xyp, offp, n, tfp, p, resp, None)

    def device(p, xyp=ptrs[0], offp=ptrs[1], stride=2, n=1, tfp=ptrs[2], resp=ptrs[3]):
        return L.rsx_gridmap_search_batch_device(handle, xyp, offp, stride, n, tfp, p, resp, None, None)

    for entry in (host, device):
        for fields, word in BAD_PARAMS:
            assert entry(C.byref(gridmap.search_params(**fields))) == -1, fields
            assert word in L.rsx_last_error_string(), (fields, L.rsx_last_error_string())
        for kw in ({"xyp": None}, {"offp": None}, {"tfp": None}, {"resp": None}, {"n": -1}):
            assert entry(None, **kw) == -1, kw
    for stride in (1, 0, -2):
        assert device(None, stride=stride) == -1 and b"point_stride" in L.rsx_last_error_string()
    assert device(C.byref(gridmap.search_params(angle_steps=180)), n=2**31 - 1) == -1 and b"2^31" in L.rsx_last_error_string()
    # the host entry looks at the offsets and at the size of every job
    for bad in ([1, 5], [0, -1]):
        o = np.array(bad, dtype=np.int64)
        assert host(None, offp=o.ctypes.data) == -1 and b"offsets" in L.rsx_last_error_string()
    big = np.zeros((gs.MAX_POINTS + 1, 2), dtype=np.float32)
    o = np.array([0, 3, gs.MAX_POINTS + 4], dtype=np.int64)
    t2, r2 = np.tile(tf, (2, 1)), np.zeros(2, dtype=gs.RESULT)
    assert host(None, xyp=big.ctypes.data, offp=o.ctypes.data, n=2, tfp=t2.ctypes.data, resp=r2.ctypes.data) == -1
    assert b"job 1 has 8193 points" in L.rsx_last_error_string()
    # prepare
    for cells in (-1, 257):
        assert L.rsx_gridmap_search_prepare(handle, cells, None) == -1 and b"max_cells" in L.rsx_last_error_string()
    return host, device


def test_argument_rules_need_no_device(rsx):
    from navtech_radar_slam_amd import gridmap
    L = rsx.lib()
    host, device = check_argument_rules(rsx, None)
    # with every rule kept, what is left to refuse is the handle
    calls = [host(None), device(None), device(None, stride=4), L.rsx_gridmap_search_prepare(None, 0, None), L.rsx_gridmap_search_prepare(None, 256, None)]
    calls += [entry(C.byref(gridmap.search_params(**fields))) for entry in (host, device) for fields in GOOD_PARAMS]
    xy, off, tf, res = _buffers(gs.MAX_POINTS)      # a job AT the cap is no error
    calls.append(L.rsx_gridmap_search_batch(None, xy.ctypes.data, off.ctypes.data, 1, tf.ctypes.data, None, res.ctypes.data, None))
    tf[0, 2] = NAN                                   # nor is a non-finite prior: the job is skipped with a status
    calls.append(L.rsx_gridmap_search_batch(None, xy.ctypes.data, off.ctypes.data, 1, tf.ctypes.data, None, res.ctypes.data, None))
    for st in calls:
        assert st == -1 and b"null handle" in L.rsx_last_error_string()


def test_search_before_a_prepare_is_refused(rsx):
    """a handle refuses to prepare before it has a likelihood, and to search before a prepare or beyond the prepared max_cells, and
    writes nothing.  A handle needs a device: without one the create is refused (RSX_ERR_NO_DEVICE), which is all that can be seen
    here; with one the refusals are checked here as in tests/test_gpu_gridsearch.py"""
    from navtech_radar_slam_amd import gridmap
    if rsx.device_count() == 0:
        with pytest.raises(rsx.RsxError):
            gridmap.GridMap(64, 96, gridmap.params(width=64, height=64))
        return
    check_refused_before_a_prepare(rsx)


def check_refused_before_a_prepare(rsx):
    from navtech_radar_slam_amd import gridmap
    L = rsx.lib()
    m = gridmap.GridMap(64, 96, gridmap.params(width=64, height=64))
    xy, off, tf, res = _buffers()
    res.view(np.uint8)[:] = 0xAB
    bnd = np.full(65 * 17 * 17, 0xABABABAB, dtype=np.uint32)

    def both(p):
        return (L.rsx_gridmap_search_batch(m.handle, xy.ctypes.data, off.ctypes.data, 1, tf.ctypes.data, p, res.ctypes.data, bnd.ctypes.data),
                L.rsx_gridmap_search_batch_device(m.handle, xy.ctypes.data, off.ctypes.data, 2, 1, tf.ctypes.data, p, res.ctypes.data, bnd.ctypes.data, None))

    assert L.rsx_gridmap_search_prepare(m.handle, 64, None) == -1 and b"no likelihood" in L.rsx_last_error_string()
    m.set_likelihood(np.zeros((64, 64), dtype=np.uint8))
    for st in both(None):
        assert st == -1 and b"rsx_gridmap_search_prepare first" in L.rsx_last_error_string()
    with pytest.raises(rsx.RsxError):
        m.search([xy], tf)
    m.prepare_search(40)
    for fields in ({"x_cells": 41, "y_cells": 40}, {"x_cells": 3, "y_cells": 41}, {}):      # (the defaults are 64)
        for st in both(C.byref(gridmap.search_params(**fields))):
            assert st == -1 and b"above the prepared max_cells 40" in L.rsx_last_error_string()
    assert (res.view(np.uint8) == 0xAB).all() and (bnd == 0xABABABAB).all()
    assert m.search([xy], tf, x_cells=40, y_cells=40, angle_steps=1)[0]["status"] == gs.STATUS_EMPTY
    m.close()
