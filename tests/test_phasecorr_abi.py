"""CPU-side checks of the rsx_phasecorr entries (include/rsx.h): the struct sizes and defaults match the header, the new exports are
declared there, and the parameter rules -- judged before the device is looked at -- reject what the header says they reject, as the
restatement's do."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import phasecorr_np as pcn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = [({"n": 100}, b"n 100"), ({"n": 1024}, b"n 1024"), ({"n": 32}, b"n 32"), ({"n": 0}, b"n 0"), ({"resolution": 0.0}, b"resolution"),
       ({"resolution": float("nan")}, b"resolution"), ({"resolution": float("inf")}, b"resolution"), ({"range_resolution": -1.0}, b"range_resolution"),
       ({"min_range_bins": -1}, b"min_range_bins"), ({"max_rotation": -0.1}, b"max_rotation"), ({"max_rotation": float("nan")}, b"max_rotation"),
       ({"n": 512, "resolution": 1.0}, b"does not fit"), ({"resolution": 1.6}, b"does not fit")]


@pytest.fixture(scope="module")
def rsx():
    import __graft_entry__ as ge
    from navtech_radar_slam_amd import _rsx
    if not os.path.exists(_rsx.LIB_PATH):
        ge.build()
    return _rsx


def test_defaults_and_layouts(rsx):
    from navtech_radar_slam_amd import phasecorr
    p = phasecorr.default_params()
    assert (p.n, p.resolution, p.range_resolution, p.min_range_bins, p.resolve_half_turn, p.max_rotation, p.reserved) == (256, 0.5, 0.0595, 58, 1, 0.0, 0)
    d = pcn.default_params()
    assert all(getattr(p, k) == v for k, v in d.items())
    assert rsx.lib().rsx_phasecorr_default_params(None) == -1
    assert C.sizeof(rsx.PhasecorrParams) == 40 and rsx.PHASECORR_RESULT_DTYPE.itemsize == 56
    assert [rsx.PHASECORR_RESULT_DTYPE.fields[f][1] for f in ("x", "y", "theta", "peak", "peak_ratio", "rot_peak", "half_turn", "status")] == \
        [0, 8, 16, 24, 32, 40, 48, 52]
    assert (rsx.PHASECORR_STATUS_ROTATION, pcn.STATUS_ROTATION, rsx.PHASECORR_STATUS_INDEX) == (1, 1, 2)
    assert phasecorr.params(n=64, resolution=2.0).n == 64
    with pytest.raises(TypeError):
        phasecorr.params(radius=3.0)


def test_header_states_what_the_library_has(rsx):
    main = open(os.path.join(ROOT, "include", "rsx.h")).read()
    diag = open(os.path.join(ROOT, "include", "rsx_diag.h")).read()
    code = re.sub(r"/\*.*?\*/", "", main, flags=re.S)
    for name in ("rsx_phasecorr_default_params", "rsx_phasecorr_create", "rsx_phasecorr_destroy", "rsx_phasecorr_register_batch",
                 "rsx_phasecorr_register_batch_device"):
        assert name + "(" in code and name in rsx.SYMBOLS, name
        getattr(rsx.lib(), name)
    assert "rsx_phasecorr_correlation(" not in code and "rsx_phasecorr_correlation(" in diag   # a diagnostic entry
    assert "} rsx_phasecorr_params;      /* 40 bytes */" in main and "} rsx_phasecorr_result; /* 56 bytes */" in main
    assert "#define RSX_PHASECORR_STATUS_ROTATION 1" in main and "#define RSX_PHASECORR_STATUS_INDEX 2" in main
    assert "n_images (12 N^2 - 32 N) + n_pairs (40 N^2 + 2048 + 4 N) + 64 bytes" in main   # the workspace, as csrc/phasecorr.hip lays it out


def test_parameter_rules_need_no_device(rsx):
    from navtech_radar_slam_amd import phasecorr
    L = rsx.lib()
    h = C.c_void_p(1)
    for fields, word in BAD:
        assert pcn.check_params(dict(pcn.default_params(), **fields), 400, 3360) is not None, fields
        h.value = 1
        assert L.rsx_phasecorr_create(0, 400, 3360, C.byref(phasecorr.params(**fields)), C.byref(h)) == -1 and not h.value, fields
        assert word in L.rsx_last_error_string(), (fields, L.rsx_last_error_string())
    for rows, cols, word in ((0, 3360, b"shape"), (5000, 3360, b"shape"), (400, 1, b"shape"), (400, 9000, b"shape"), (400, 1000, b"does not fit")):
        assert pcn.check_params(pcn.default_params(), rows, cols) is not None
        assert L.rsx_phasecorr_create(0, rows, cols, None, C.byref(h)) == -1 and word in L.rsx_last_error_string(), (rows, cols)
    assert L.rsx_phasecorr_create(0, 400, 3360, None, None) == -1
    st = L.rsx_phasecorr_create(0, 400, 3360, C.byref(phasecorr.params(n=512)), C.byref(h))   # 128 m fit in 3360 bins of 0.0595 m
    if rsx.device_count() > 0:
        assert st == 0 and h.value and L.rsx_phasecorr_destroy(h) == 0
    else:  # never computed on the CPU: RSX_ERR_NO_DEVICE, and *out cleared
        assert st == -2 and not h.value and b"no HIP device" in L.rsx_last_error_string()
        with pytest.raises(rsx.RsxError):
            phasecorr.Phasecorr(400, 3360)
    assert L.rsx_phasecorr_destroy(None) == 0
    img, pairs, res = np.zeros((400, 3360), dtype=np.uint8), np.zeros(2, dtype=np.int32), np.zeros(1, dtype=rsx.PHASECORR_RESULT_DTYPE)
    assert L.rsx_phasecorr_register_batch(None, img.ctypes.data, 1, 0, 3360, 0, pairs.ctypes.data, 1, res.ctypes.data, None) == -1
    assert L.rsx_phasecorr_register_batch_device(None, img.ctypes.data, 1, 0, 3360, 0, pairs.ctypes.data, 1, res.ctypes.data, None, None) == -1
    assert L.rsx_phasecorr_correlation(None, 0, None, None) == -1
