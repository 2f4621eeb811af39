"""The derivable truths of tests/phasecorr_np.py alone (no GPU, no library): pure rotations come back as rotations, the synthetic drive comes
back as its known motion with an unambiguous peak, a scan's image does not depend on its place in a batch, and the parameter rules
reject what include/rsx.h says they reject.  One angle bin (pi / N) and one pixel are the method's quantisation: a larger miss is a
wrong peak."""
import math

import numpy as np
import pytest

import phasecorr_np as pc
from navtech_radar_slam_amd import synth

ROWS, COLS, OFF = 400, 3360, synth.OXFORD_META
SHIFTS = (0, 1, 100, 200, 333)


def wrap(t):
    return (t + math.pi) % (2.0 * math.pi) - math.pi


def rotation_scans():
    """scan 0 unrolled, then one scan per shift with its own speckle: [6, rows, 11 + cols]"""
    return np.stack([synth.polar_image(5, shift_rows=0)[0]] + [synth.polar_image(5, shift_rows=k, noise_seed=100 + k)[0] for k in SHIFTS])


@pytest.fixture(scope="module")
def rot_scans():
    return rotation_scans()


@pytest.mark.parametrize("n", [64, 256])
def test_pure_rotations(rot_scans, n):
    """src = the scan rolled by +k rows, dst = the unrolled one: every return of src sits k rows further round, so
    p_dst = R(-k 2 pi / rows) p_src: theta = -k 2 pi / 400 (wrapped), x = y = 0"""
    # N = 64 covers the same 64 m half-width as the default, at 2 m per pixel
    r = pc.Restatement(ROWS, COLS, dict(n=n, resolution=128.0 / n))
    res, _ = r.register_batch(rot_scans, [(1 + i, 0) for i in range(len(SHIFTS))], col_offset=OFF)
    for k, got in zip(SHIFTS, res):
        want = wrap(-k * 2.0 * math.pi / ROWS)
        err = abs(wrap(got["theta"] - want))
        print(f"N={n} k={k}: theta {got['theta']:+.5f} want {want:+.5f} err {err:.5f} (bin {math.pi / n:.5f}) x {got['x']:+.4f} y {got['y']:+.4f} "
              f"peak {got['peak']:.3f} ratio {got['peak_ratio']:.3f} half_turn {got['half_turn']}")
        assert err <= math.pi / n, (n, k, got["theta"], want)
        assert abs(got["x"]) < r.p["resolution"] and abs(got["y"]) < r.p["resolution"], (n, k, got["x"], got["y"])
        if abs(abs(want) - math.pi / 2) > math.pi / n:   # (at a quarter turn exactly either branch is right)
            assert got["half_turn"] == (1 if abs(want) > math.pi / 2 else 0), (n, k)
        assert got["status"] == 0


def test_synthetic_drive():
    imgs, _, poses, _ = synth.polar_sequence(3, 6)
    r = pc.Restatement(ROWS, COLS)
    res, _ = r.register_batch(imgs, [(i + 1, i) for i in range(5)], col_offset=OFF)
    for i, got in enumerate(res):
        want = synth.relative_pose(poses[i], poses[i + 1])
        ex, ey, et = got["x"] - want[0], got["y"] - want[1], wrap(got["theta"] - want[2])
        print(f"pair {i}: err x {ex:+.4f} m y {ey:+.4f} m theta {et:+.5f} rad, peak {got['peak']:.3f} ratio {got['peak_ratio']:.3f} rot_peak {got['rot_peak']:.3f}")
        assert got["peak_ratio"] <= 0.5
        assert abs(ex) <= 0.5 and abs(ey) <= 0.5 and abs(et) <= math.pi / 256, (i, ex, ey, et)
        assert got["half_turn"] == 0 and got["status"] == 0


def test_image_does_not_depend_on_batch_position():
    imgs = synth.polar_sequence(3, 3)[0]
    r = pc.Restatement(ROWS, COLS, dict(n=64, resolution=2.0))
    _, a = r.register_batch(imgs, [(1, 0)], col_offset=OFF)
    _, b = r.register_batch(imgs[::-1], [(1, 2)], col_offset=OFF)
    for i in range(3):
        assert np.array_equal(a[i], b[2 - i])
    assert a[0].dtype == np.float32 and a[0].max() > 0 and a[0][32, 32] == 0 and a[0][0, 0] == 0


def test_tables():
    t = pc.Tables(dict(pc.default_params(), n=64, resolution=2.0), ROWS, COLS)
    E = t.E
    for k in range(1, 64):
        assert E[64 - k, 0] == E[k, 0] and E[64 - k, 1] == -E[k, 1]
    assert E[0].tolist() == [1.0, 0.0] and E[16].tolist() == [0.0, 1.0] and E[32].tolist() == [-1.0, 0.0]
    assert np.abs(E[:, 0] - np.cos(2 * np.pi * np.arange(64) / 64)).max() < 1e-7
    # forward is azimuth 0: the pixel ahead of the centre reads row 0, the one to the left (+y) row rows / 4
    assert t.map_a[32, 60] == 0.0 and t.map_a[60, 32] == 100.0
    assert t.map_r[32, 60] == np.float32(28 * 2.0 / 0.0595 - 0.5)
    assert t.map_r[32, 32] == -1 and t.map_r[32, 33] == -1 and t.map_r[0, 0] == -1   # centre, below min_range, outside the disc
    assert t.map_r[32, 63] == np.float32(31 * 2.0 / 0.0595 - 0.5) and t.map_r[32, 0] == -1   # radius N / 2 - 1 is the last one inside


def test_parameter_rules():
    d = pc.default_params()
    assert pc.check_params(d, ROWS, COLS) is None
    for fields, word in (({"n": 100}, "n"), ({"n": 1024}, "n"), ({"n": 32}, "n"), ({"resolution": 0.0}, "resolution"),
                         ({"resolution": float("nan")}, "resolution"), ({"range_resolution": -1.0}, "range_resolution"),
                         ({"min_range_bins": -1}, "min_range_bins"), ({"max_rotation": -0.1}, "max_rotation"),
                         ({"n": 512, "resolution": 1.0}, "disc"), ({"resolution": 1.6}, "disc")):
        assert pc.check_params(dict(d, **fields), ROWS, COLS) == word, fields
    assert pc.check_params(d, ROWS, 1000) == "disc" and pc.check_params(d, 0, COLS) == "shape"
    assert pc.check_params(dict(d, n=512), ROWS, COLS) is None   # 128 m fit in 3360 bins of 0.0595 m
    with pytest.raises(ValueError):
        pc.Restatement(ROWS, COLS, dict(n=100))
    imgs = np.zeros((2, ROWS, COLS), dtype=np.uint8)
    with pytest.raises(ValueError):
        pc.Restatement(ROWS, COLS, dict(n=64, resolution=2.0)).register_batch(imgs, [(0, 2)])
