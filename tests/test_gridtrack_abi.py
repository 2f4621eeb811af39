"""The grid-map tracker's boundary without a GPU (include/rsx.h, rsx_gridmap_tracker_*): the layouts of the two structs, the defaults, the
argument rules that are judged before the handle or the device is looked at, and -- as a reading of the sources -- that the tracker's
kernel runs the pick and the refinement loop of the stand-alone kernels, not copies of them."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gridtrack_np as gt  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "navtech-radar-slam_amd", "csrc")
BAD_ARG = -1


@pytest.fixture(scope="module")
def rsx():
    import __graft_entry__ as ge
    from navtech_radar_slam_amd import _rsx
    if not os.path.exists(_rsx.LIB_PATH):
        ge.build()
    return _rsx


def test_layouts_and_defaults(rsx):
    from navtech_radar_slam_amd import gridmap
    assert C.sizeof(rsx.GridmapTrackParams) == 88 and C.sizeof(rsx.GridmapTrackResult) == 344
    assert rsx.GRIDMAP_TRACK_RESULT_DTYPE.itemsize == 344 == gt.RESULT.itemsize
    for name in gt.RESULT.names:
        assert rsx.GRIDMAP_TRACK_RESULT_DTYPE.fields[name][1] == gt.RESULT.fields[name][1] == getattr(rsx.GridmapTrackResult, name).offset, name
    p = gridmap.default_track_params()
    d = gt.params()
    assert (p.match.angle_steps, p.match.x_cells, p.match.y_cells, p.match.angle_step, p.match.reserved) == (2, 2, 2, 0.01, 0)
    assert {k: getattr(p.match, k) for k in d["match"]} == d["match"] and {k: getattr(p.refine, k) for k in d["refine"]} == d["refine"]
    assert (p.min_score, p.predict, list(p.reserved)) == (0, 1, [0, 0]) and (d["min_score"], d["predict"]) == (0, 1)
    assert rsx.lib().rsx_gridmap_track_default_params(None) == BAD_ARG
    q = gridmap.track_params(angle_steps=1, max_evaluations=7, min_score=5, predict=0)
    assert (q.match.angle_steps, q.refine.max_evaluations, q.min_score, q.predict) == (1, 7, 5, 0)
    with pytest.raises(TypeError):
        gridmap.track_params(no_such_field=1)


def test_the_rules_are_judged_before_the_handle(rsx):
    """with no handle at all, a push names the violated rule, not the handle; with every rule kept it names the handle"""
    from navtech_radar_slam_amd import gridmap
    L = rsx.lib()
    xy, off, n = np.zeros((1, 2), dtype=np.float32), np.zeros(2, dtype=np.int64), np.ones(1, dtype=np.int32)
    out = np.zeros(1, dtype=gt.RESULT)

    def message(p, device):
        ref = C.byref(p) if p is not None else None
        st = (L.rsx_gridmap_tracker_push_device(None, xy.ctypes.data, off.ctypes.data, 2, n.ctypes.data, 1, ref, out.ctypes.data, None) if device
              else L.rsx_gridmap_tracker_push(None, xy.ctypes.data, off.ctypes.data, n.ctypes.data, ref, out.ctypes.data))
        assert st == BAD_ARG
        return L.rsx_last_error_string().decode()

    broken = {"angle_steps": gridmap.track_params(angle_steps=9), "x_cells": gridmap.track_params(x_cells=9), "y_cells": gridmap.track_params(y_cells=-1),
              "angle_step": gridmap.track_params(angle_step=0.0), "predict": gridmap.track_params(predict=-1),
              "max_evaluations": gridmap.track_params(max_evaluations=65), "max_shift_step": gridmap.track_params(max_shift_step=9.0)}
    for k in range(2):
        broken["reserved words %d" % k] = gridmap.default_track_params()
        broken["reserved words %d" % k].reserved[k] = -1
    broken["match.reserved"] = gridmap.default_track_params()
    broken["match.reserved"].match.reserved = 1
    broken["reserved must be 0"] = gridmap.default_track_params()
    broken["reserved must be 0"].refine.reserved = 1
    for device in (False, True):
        for word, p in broken.items():
            assert word.rstrip(" 01") in message(p, device), (word, device)
        assert "null handle" in message(None, device) and "null handle" in message(gridmap.track_params(angle_steps=8, x_cells=8, y_cells=8), device)
    assert L.rsx_gridmap_tracker_push_device(None, xy.ctypes.data, off.ctypes.data, 1, n.ctypes.data, 1, None, out.ctypes.data, None) == BAD_ARG
    assert "point_stride" in L.rsx_last_error_string().decode()
    assert L.rsx_gridmap_tracker_push_device(None, xy.ctypes.data, off.ctypes.data, 2, n.ctypes.data, -1, None, out.ctypes.data, None) == BAD_ARG
    h = C.c_void_p(1)
    assert L.rsx_gridmap_tracker_create(None, 1, C.byref(h)) == BAD_ARG and not h.value
    assert L.rsx_gridmap_tracker_create(None, 1, None) == BAD_ARG
    assert L.rsx_gridmap_tracker_destroy(None) == 0
    for call in (lambda: L.rsx_gridmap_tracker_reset(None, out.ctypes.data), lambda: L.rsx_gridmap_tracker_set_pose(None, 0, out.ctypes.data),
                 lambda: L.rsx_gridmap_tracker_state(None, None, None, None)):
        assert call() == BAD_ARG


def _code(name):
    txt = open(os.path.join(CSRC, name)).read()
    return re.sub(r"//[^\n]*", "", txt)


def test_the_kernel_runs_the_shared_device_code():
    """the pick and the refinement loop live in gridmatch_dev.h and gridrefine_dev.h once; gmm_pick, gmr_refine and gmt_track call them;
    the tracker has one launch, no atomics, no cooperative launch"""
    match_dev, refine_dev = _code("gridmatch_dev.h"), _code("gridrefine_dev.h")
    assert len(re.findall(r"rsx_gridmap_match_result pick_record\(", match_dev)) == 1 and "block_max(key" in match_dev
    assert len(re.findall(r"rsx_gridmap_refine_result refine_record\(", refine_dev)) == 1 and "LAMBDA_MAX" in refine_dev
    match, refine, track = _code("gridmatch.hip"), _code("gridrefine.hip"), _code("gridtrack.hip")
    for src, fn in ((match, "pick_record("), (refine, "refine_record("), (track, "pick_record("), (track, "refine_record("), (track, "slot_sums("),
                    (match, "slot_sums("), (track, "fill_cells("), (match, "fill_cells(")):
        assert src.count(fn) == 1, fn
    for src in (match, refine, track):
        assert not re.search(r"\bblock_max\(|\bsolve\(|LAMBDA", src)
    assert track.count("hipLaunchKernelGGL(") == 1 and "atomic" not in track.lower() and "Cooperative" not in track
    assert "#pragma STDC FP_CONTRACT OFF" in track
