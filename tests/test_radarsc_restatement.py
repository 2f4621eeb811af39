"""CPU checks of the radar scan-context contract (tests/radarsc_np.py; PARITY with MulRan's own builder UNPINNED): the
vectorised restatement against a naive triple loop, the place-recognition property on the project's synthetic scans through
the oracle's pair function, and the no-GPU behaviour of the new create."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import radarsc_cases as cases  # noqa: E402
import radarsc_np as rc  # noqa: E402


@pytest.mark.parametrize("stat", [rc.MEAN, rc.MAX])
@pytest.mark.parametrize("floor", [0, 40])
def test_restatement_equals_naive_loop(stat, floor):
    rng = np.random.default_rng(5)
    rows, cols, off = 23, 97, 3
    img = rng.integers(0, 256, (rows, off + cols + 2), dtype=np.uint8)
    az = (5.9 + np.arange(rows) * 0.31).astype(np.float32)   # wraps, several rows per sector and empty sectors
    az[7] = np.nan
    az[11] = -0.2
    az[12] = 40.0
    # resolution 1.0, max_radius 60: rings end inside the row (bins 60 .. 96 have none), ring width 3 bins
    kw = dict(col_offset=off, cols=cols, resolution=1.0, max_radius=60.0, min_range=5, power_floor=floor, stat=stat)
    got = rc.build(img, az, **kw)
    want = rc.build_naive(img, az, **kw)
    assert got.dtype == np.float32 and got.shape == (1200,)
    assert got.tobytes() == want.tobytes()
    assert np.count_nonzero(got) > 200 and np.count_nonzero(got == 0) > 200


def test_ring_and_sector_rules():
    ring = rc.ring_of_bins(3360)
    assert ring[57] == -1 and ring[58] == 0 and ring[1344] == 19 and ring[1345] == -1   # the last bin inside 80 m
    assert np.all(np.diff(ring[58:1345]) >= 0) and set(ring[58:1345]) == set(range(20))
    sec = rc.sector_of_rows(np.array([0.0, 1e-6, np.pi, 2 * np.pi - 1e-4, -1e-4, 7.0, np.inf, np.nan], dtype=np.float32))
    assert sec.tolist() == [0, 0, 29 if np.float64(np.float32(np.pi)) * 57.29577951308232 <= 180.0 else 30, 59, 59, 6, -1, -1]


def test_rotated_revisits_rank_first(oracle):
    """40 scans, four revisits rolled by 20 / 200 / 387 / 7 rows: the revisited scan comes back first, at the shift the roll
    predicts, strictly closer than the runner-up."""
    db, q, az = cases.scans()
    m = oracle.Manager()
    m.add_descriptors(rc.build_batch(db, az).astype(np.float64))
    qd = rc.build_batch(q, az).astype(np.float64)
    hits = [m.exhaustive(qd[j], k=2) for j in range(len(q))]
    print([(h[0]["index"], h[0]["shift"], float(h[0]["dist"]), float(h[1]["dist"])) for h in hits])
    cases.check_ranking(hits)


def test_create_fails_without_a_device():
    import ctypes as C
    import __graft_entry__ as ge
    from navtech_radar_slam_amd import _rsx
    if not os.path.exists(_rsx.LIB_PATH):
        ge.build()
    L = _rsx.lib()
    p = _rsx.RadarScParams()
    assert L.rsx_radarsc_default_params(C.byref(p)) == 0
    assert (p.max_radius, p.min_range, p.power_floor, p.stat) == (80.0, 58, 0, _rsx.RADARSC_MEAN) and abs(p.resolution - 0.0595) < 1e-7
    if _rsx.device_count() > 0:
        pytest.skip("a GPU is visible here (tests/test_gpu_radarsc.py covers the create on a GPU)")
    h = C.c_void_p(1)
    assert L.rsx_radarsc_create(0, 400, 3360, None, C.byref(h)) == -2 and not h.value   # RSX_ERR_NO_DEVICE, *out cleared
    assert b"no HIP device" in L.rsx_last_error_string()
    from navtech_radar_slam_amd import radar_context
    with pytest.raises(_rsx.RsxError):
        radar_context.RadarContext()
