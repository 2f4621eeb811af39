"""CPU-side checks of the rsx_gridmap_refine_* entries (include/rsx.h): the layout of the structs against navtech_radar_slam_amd._rsx and
the restatement, the defaults, and the parameter and argument rules, which are judged before the handle or the device is looked at and
so need no device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gridrefine_np as gr  # noqa: E402


@pytest.fixture(scope="module")
def rsx():
    import __graft_entry__ as ge
    from navtech_radar_slam_amd import _rsx
    if not os.path.exists(_rsx.LIB_PATH):
        ge.build()
    return _rsx


def test_struct_sizes_and_defaults(rsx):
    from navtech_radar_slam_amd import gridmap
    names = ("damping", "max_shift_step", "max_rotation_step", "shift_tolerance", "rotation_tolerance", "max_evaluations", "reserved")
    offsets = [0, 8, 16, 24, 32, 40, 44]
    assert C.sizeof(rsx.GridmapRefineParams) == 48 == gr.PARAMS.itemsize
    assert [getattr(rsx.GridmapRefineParams, f).offset for f in names] == offsets
    assert gr.PARAMS.names == names and [gr.PARAMS.fields[f][1] for f in names] == offsets
    assert C.sizeof(rsx.GridmapRefineResult) == 152 == rsx.GRIDMAP_REFINE_RESULT_DTYPE.itemsize == gr.RESULT.itemsize
    names = ("transform", "hessian", "cost_initial", "cost", "score_initial", "score", "evaluations", "accepted", "n_points", "n_inside", "status",
             "reserved")
    offsets = [0, 48, 96, 104, 112, 120, 128, 132, 136, 140, 144, 148]
    assert [getattr(rsx.GridmapRefineResult, f).offset for f in names] == offsets
    for dt in (rsx.GRIDMAP_REFINE_RESULT_DTYPE, gr.RESULT):
        assert dt.names == names and [dt.fields[f][1] for f in names] == offsets
        assert [dt.fields[f][0].base for f in names] == [np.dtype("<f8")] * 6 + [np.dtype("<i4")] * 6
    assert (rsx.GRIDMAP_REFINE_STATUS_SINGULAR, rsx.GRIDMAP_REFINE_STATUS_MAX) == (16, 32) == (gr.STATUS_SINGULAR, gr.STATUS_MAX)
    assert (gr.STATUS_TRANSFORM, gr.STATUS_POINTS, gr.STATUS_EMPTY) == (rsx.GRIDMAP_MATCH_STATUS_TRANSFORM, rsx.GRIDMAP_MATCH_STATUS_POINTS,
                                                                       rsx.GRIDMAP_MATCH_STATUS_EMPTY)
    assert gr.MAX_POINTS == rsx.GRIDMAP_MATCH_MAX_POINTS
    p = gridmap.default_refine_params()
    assert gr.DEFAULTS == {k: getattr(p, k) for k in gr.DEFAULTS} and p.reserved == 0
    assert gr.DEFAULTS == dict(damping=1e-3, max_shift_step=1.0, max_rotation_step=0.02, shift_tolerance=1e-3, rotation_tolerance=1e-5, max_evaluations=32)
    assert rsx.lib().rsx_gridmap_refine_default_params(None) == -1
    assert gridmap.refine_params(max_evaluations=7).max_evaluations == 7
    with pytest.raises(TypeError):
        gridmap.refine_params(evaluations=3)


NAN, INF = float("nan"), float("inf")
BAD_PARAMS = [({"damping": 0.0}, b"damping"), ({"damping": -1e-3}, b"damping"), ({"damping": NAN}, b"damping"), ({"damping": INF}, b"damping"),
              ({"max_shift_step": 0.0}, b"max_shift_step"), ({"max_shift_step": 8.5}, b"max_shift_step"), ({"max_shift_step": NAN}, b"max_shift_step"),
              ({"max_shift_step": -1.0}, b"max_shift_step"), ({"max_rotation_step": 0.0}, b"max_rotation_step"),
              ({"max_rotation_step": 0.51}, b"max_rotation_step"), ({"max_rotation_step": NAN}, b"max_rotation_step"),
              ({"max_rotation_step": INF}, b"max_rotation_step"), ({"shift_tolerance": -1e-9}, b"shift_tolerance"),
              ({"shift_tolerance": NAN}, b"shift_tolerance"), ({"shift_tolerance": INF}, b"shift_tolerance"),
              ({"rotation_tolerance": -1e-9}, b"rotation_tolerance"), ({"rotation_tolerance": NAN}, b"rotation_tolerance"),
              ({"rotation_tolerance": INF}, b"rotation_tolerance"), ({"max_evaluations": 0}, b"max_evaluations"),
              ({"max_evaluations": 65}, b"max_evaluations"), ({"max_evaluations": -4}, b"max_evaluations"), ({"reserved": 1}, b"reserved")]
GOOD_PARAMS = [{"max_shift_step": 8.0, "max_rotation_step": 0.5, "max_evaluations": 64}, {"shift_tolerance": 0.0, "rotation_tolerance": 0.0, "max_evaluations": 1},
               {"damping": 1e-300}, {"damping": 1e300, "max_shift_step": 1e-300}]


def _buffers(n_points=5):
    xy = np.zeros((n_points, 2), dtype=np.float32)
    off = np.array([0, n_points], dtype=np.int64)
    tf = np.array([[1.0, 0.0, 0.0, 0.0, 1.0, 0.0]])
    res = np.zeros(1, dtype=gr.RESULT)
    return xy, off, tf, res


def check_argument_rules(rsx, handle):
    """every rule of the two refine entries on dummy host buffers; shared with tests/test_gpu_gridrefine.py, which passes a handle (with
    handle None every call ends at "null handle" at the latest: nothing is launched)"""
    from navtech_radar_slam_amd import gridmap
    L = rsx.lib()
    xy, off, tf, res = _buffers()
    ptrs = (xy.ctypes.data, off.ctypes.data, tf.ctypes.data, res.ctypes.data)

    def host(p, xyp=ptrs[0], offp=ptrs[1], n=1, tfp=ptrs[2], resp=ptrs[3]):
        return L.rsx_gridmap_refine_batch(handle, xyp, offp, n, tfp, p, resp)

    def device(p, xyp=ptrs[0], offp=ptrs[1], stride=2, n=1, tfp=ptrs[2], resp=ptrs[3]):
        return L.rsx_gridmap_refine_batch_device(handle, xyp, offp, stride, n, tfp, p, resp, None)

    for entry in (host, device):
        for fields, word in BAD_PARAMS:
            assert entry(C.byref(gridmap.refine_params(**fields))) == -1, fields
            assert word in L.rsx_last_error_string(), (fields, L.rsx_last_error_string())
        for kw in ({"xyp": None}, {"offp": None}, {"tfp": None}, {"resp": None}, {"n": -1}):
            assert entry(None, **kw) == -1, kw
    for stride in (1, 0, -2):
        assert device(None, stride=stride) == -1 and b"point_stride" in L.rsx_last_error_string()
    # the host entry looks at the offsets and at the size of every job
    for bad in ([1, 5], [0, -1]):
        o = np.array(bad, dtype=np.int64)
        assert host(None, offp=o.ctypes.data) == -1 and b"offsets" in L.rsx_last_error_string()
    big = np.zeros((gr.MAX_POINTS + 1, 2), dtype=np.float32)
    o = np.array([0, 3, gr.MAX_POINTS + 4], dtype=np.int64)
    t2, r2 = np.tile(tf, (2, 1)), np.zeros(2, dtype=gr.RESULT)
    assert host(None, xyp=big.ctypes.data, offp=o.ctypes.data, n=2, tfp=t2.ctypes.data, resp=r2.ctypes.data) == -1
    assert b"job 1 has 8193 points" in L.rsx_last_error_string()
    return host, device


def test_argument_rules_need_no_device(rsx):
    from navtech_radar_slam_amd import gridmap
    L = rsx.lib()
    host, device = check_argument_rules(rsx, None)
    # with every rule kept, what is left to refuse is the handle
    calls = [host(None), device(None), device(None, stride=4)]
    calls += [entry(C.byref(gridmap.refine_params(**fields))) for entry in (host, device) for fields in GOOD_PARAMS]
    xy, off, tf, res = _buffers(gr.MAX_POINTS)      # a job AT the cap is no error
    calls.append(L.rsx_gridmap_refine_batch(None, xy.ctypes.data, off.ctypes.data, 1, tf.ctypes.data, None, res.ctypes.data))
    tf[0, 2] = NAN                                   # nor is a non-finite prior: the job is skipped with a status
    calls.append(L.rsx_gridmap_refine_batch(None, xy.ctypes.data, off.ctypes.data, 1, tf.ctypes.data, None, res.ctypes.data))
    for st in calls:
        assert st == -1 and b"null handle" in L.rsx_last_error_string()


def test_priors_may_be_records(rsx):
    """refine takes an (n, 6) array or the record array of match or search, whose `transform` it reads"""
    from navtech_radar_slam_amd import gridmap
    t = np.arange(12, dtype=np.float64).reshape(2, 6)
    for dt in (rsx.GRIDMAP_MATCH_RESULT_DTYPE, rsx.GRIDMAP_SEARCH_RESULT_DTYPE):
        rec = np.zeros(2, dtype=dt)
        rec["transform"] = t
        got = gridmap.prior_transforms(rec, 2)
        assert got.dtype == np.float64 and got.flags.c_contiguous and got.tobytes() == t.tobytes()
    assert gridmap.prior_transforms(t.reshape(-1), 2).tobytes() == t.tobytes()
    assert gridmap.prior_transforms(t.tolist(), 2).shape == (2, 6)


def test_refine_before_a_likelihood_is_refused(rsx):
    """a handle that has had no likelihood_update and no likelihood_set refuses to refine and writes nothing.  A handle needs a device:
    without one the create is refused (RSX_ERR_NO_DEVICE), which is all that can be seen here; with one the refusal is checked here as in
    tests/test_gpu_gridrefine.py"""
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
    for st in (L.rsx_gridmap_refine_batch(m.handle, xy.ctypes.data, off.ctypes.data, 1, tf.ctypes.data, None, res.ctypes.data),
               L.rsx_gridmap_refine_batch_device(m.handle, xy.ctypes.data, off.ctypes.data, 2, 1, tf.ctypes.data, None, res.ctypes.data, None)):
        assert st == -1 and b"no likelihood" in L.rsx_last_error_string()
    assert (res.view(np.uint8) == 0xAB).all()
    with pytest.raises(rsx.RsxError):
        m.refine([xy], tf)
    m.set_likelihood(np.zeros((64, 64), dtype=np.uint8))
    assert m.refine([xy], tf)[0]["status"] == gr.STATUS_EMPTY
    m.close()
