"""The grid map's restatement (tests/gridmap_np.py) against geometry worked out by hand: which cell a return lands in, for every
quadrant and both signs of yaw; independence of the scan order and of the batch cut; the range parameters; the render formulas; and
the property the map is built for -- it is sharpest at the true poses.  No GPU, no library."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gridmap_cases as gc  # noqa: E402
import gridmap_np as gm  # noqa: E402

ROWS, COLS = 64, 96


def _one_byte(a, j, value=255):
    img = np.zeros((1, ROWS, gc.META + COLS), dtype=np.uint8)
    img[0, a, gc.META + j] = value
    return img


def _planes(imgs, poses, p):
    return gm.add_batch(gm.zeros(p), imgs, gc.matrices(poses), p, col_offset=gc.META)


@pytest.mark.parametrize("yaw", [0.0, 0.6, -0.6, 2.5, -2.5])
@pytest.mark.parametrize("a", [5, 21, 37, 53])          # one beam in each quadrant of the sensor frame
def test_a_return_lands_in_the_cell_that_holds_it(a, yaw):
    """one saturated byte at (row a, bin j): the cell that contains R (rho cos phi, rho sin phi) + t, rho = (j + 0.5) rr,
    phi = 2 pi a / rows, gets it.  The pose is not symmetric (tx != ty, yaw != 0), so a transposed matrix, a swapped axis or a
    mirrored azimuth moves the return to another cell."""
    p = gc.small_params(192, 128, range_halfwidth=2)       # a cell's centre is within 0.36 m = 1.5 bins of any point of the cell
    j, (tx, ty) = 70, (p["origin_x"] + 41.3, p["origin_y"] + 29.9)
    rho, phi = (j + 0.5) * p["range_resolution"], 2 * math.pi * a / ROWS
    wx = math.cos(yaw) * rho * math.cos(phi) - math.sin(yaw) * rho * math.sin(phi) + tx
    wy = math.sin(yaw) * rho * math.cos(phi) + math.cos(yaw) * rho * math.sin(phi) + ty
    ix, iy = int(math.floor((wx - p["origin_x"]) / p["resolution"])), int(math.floor((wy - p["origin_y"]) / p["resolution"]))
    psum, pcnt, phit = _planes(_one_byte(a, j), [(tx, ty, yaw)], p)
    assert 0 <= ix < 192 and 0 <= iy < 128
    assert psum[iy, ix] == 255 and phit[iy, ix] == 1 and pcnt[iy, ix] == 1
    # nothing else is lit but cells around that one (five bins are 1.25 m deep and, at 17.6 m, a beam is 1.7 m wide)
    lit = np.argwhere(psum > 0)
    assert len(lit) >= 1 and np.abs(lit - (iy, ix)).max() <= 4
    assert (psum[pcnt == 0] == 0).all() and psum.sum() == 255 * len(lit) and phit.sum() == len(lit)


def test_width_and_height_are_not_swapped():
    p = gc.small_params(192, 128)
    planes = _planes(gc.images(np.random.default_rng(1), 1, ROWS, COLS), [(p["origin_x"] + 70.0, p["origin_y"] + 30.0, 0.3)], p)
    assert planes[0].shape == (128, 192)
    iy, ix = np.nonzero(planes[1])
    assert ix.max() > 128 and abs(ix.mean() - 140) < 1 and abs(iy.mean() - 60) < 1     # x = 70 m is column 140, y = 30 m is row 60


def test_order_and_batch_cut_do_not_matter():
    imgs, T, p = gc.random_case(3, ROWS, COLS, 192, 128, 5)
    want = gm.add_batch(gm.zeros(p), imgs, T, p, col_offset=gc.META)
    order = [3, 0, 4, 2, 1]
    got = gm.add_batch(gm.zeros(p), imgs[order], T[order], p, col_offset=gc.META)
    cut = gm.zeros(p)
    for lo, hi in ((0, 2), (2, 3), (3, 5)):
        gm.add_batch(cut, imgs[lo:hi], T[lo:hi], p, col_offset=gc.META)
    for k in range(3):
        assert want[k].tobytes() == got[k].tobytes() == cut[k].tobytes()
    assert want[1].max() >= 3


def test_a_scan_outside_the_map_changes_nothing():
    for name, imgs, T, p in gc.border_cases(ROWS, COLS):
        planes = gm.add_batch(gm.zeros(p), imgs, T, p, col_offset=gc.META)
        assert planes[1].any() == (name != "far"), name
        if name == "far":
            assert not planes[0].any() and not planes[2].any()


def _along_x(p, poses=((0.0, 0.0, 0.0),), img=None):
    """the cells on the +x axis of a sensor on a cell centre at yaw 0: row 0 of the image, cell k at 0.5 k metres = bin 2 k"""
    img = _one_byte(0, 0, 0) if img is None else img
    planes = _planes(img, poses, p)
    iy = int((0.0 - p["origin_y"]) / p["resolution"])
    ix0 = int((0.0 - p["origin_x"]) / p["resolution"])
    return [q[iy, ix0:] for q in planes]


def test_range_parameters_on_one_row():
    base = dict(width=64, height=64, resolution=0.5, origin_x=-0.25, origin_y=-16.25, range_resolution=0.25, min_range_bins=0, range_halfwidth=0)
    img = _one_byte(0, 0, 0)
    img[0, 0, gc.META:] = np.arange(COLS) + 100            # bin j reads 100 + j
    # cell k of the axis sits at 0.5 k m, exactly on the lower edge of bin 2 k: bin 2 k (the edge belongs to the bin above it)
    psum, pcnt, phit = _along_x(gm.params(**base), img=img)
    assert pcnt[:48].tolist() == [1] * 48 and pcnt[48:].tolist() == [0] * 16          # bins 0 .. 94 of 96; 0.5 * 48 = bin 96: outside
    assert psum[:48].tolist() == [100 + 2 * k for k in range(48)]
    # min_range_bins: the first bin used
    psum, pcnt, _ = _along_x(gm.params(**dict(base, min_range_bins=7)), img=img)
    assert pcnt[:48].tolist() == [0] * 4 + [1] * 44 and psum[4] == 108                # cell 3 is bin 6, cell 4 is bin 8
    # max_range: d2 > max_range^2 is out, d2 == max_range^2 is in
    psum, pcnt, _ = _along_x(gm.params(**dict(base, max_range=10.0)), img=img)
    assert pcnt[:22].tolist() == [1] * 21 + [0] and psum[20] == 140
    # range_halfwidth: the maximum over j - hw .. j + hw, clipped to [min_range_bins, cols - 1]
    psum, pcnt, _ = _along_x(gm.params(**dict(base, range_halfwidth=3)), img=img)
    assert psum[:48].tolist() == [min(100 + 2 * k + 3, 195) for k in range(48)]
    dec = img.copy()
    dec[0, 0, gc.META:] = 250 - np.arange(COLS)            # decreasing: the maximum is at the lowest bin of the span
    psum, pcnt, _ = _along_x(gm.params(**dict(base, range_halfwidth=3, min_range_bins=7)), img=dec)
    assert psum[4:48].tolist() == [250 - max(2 * k - 3, 7) for k in range(4, 48)]
    # hit_threshold: v >= threshold
    _, pcnt, phit = _along_x(gm.params(**dict(base, hit_threshold=140)), img=img)
    assert phit[:48].tolist() == [0] * 20 + [1] * 28


def test_exact_tie_cases_hold_what_they_are_for():
    """what tests/test_gpu_gridmap.py::test_exact_ties_and_boundaries relies on, checked without a GPU"""
    counts = {(rows, corner): gc.exact_ties(gc.tie_case(rows, corner)[1][0], gc.tie_case(rows, corner)[2], rows, 96)
              for rows in (4, 8) for corner in (True, False)}
    assert counts[(8, True)] == (0, 0)                       # a cell corner: d2 = 0.0625 (odd^2 + odd^2), never the square of an edge
    assert counts[(4, True)][0] == 0 and counts[(4, True)][1] >= 20
    assert counts[(4, False)][0] >= 100 and counts[(4, False)][1] >= 20
    assert counts[(8, False)][0] >= 100 and counts[(8, False)][1] >= 1
    # a tie goes to the smallest row: on the diagonal px = py > 0 of four rows, row 0 and not row 1
    imgs, T, p = gc.tie_case(4, False)
    g = gm.geometry(T[0], p, 4, 96)
    # (only where the two sums are equal to the last bit: fp32 cos(pi / 2) = 6e-17 is absorbed next to py = px up to about 15 m;
    # the other three diagonals meet cos(3 pi / 2) = -1.8e-16 or sin(pi) = 1.2e-16, which are not)
    tie = g["best"] == g["second"]
    diag = tie & (g["px"] == g["py"]) & (g["px"] > 0)
    assert diag.sum() >= 20 and (g["a"][diag] == 0).all()
    assert (g["a"][(g["px"] == g["py"]) & (g["px"] > 0) & ~tie] == 1).all()


def test_render_formulas():
    s = np.array([[0, 0, 10, 11, 12, 255 * 7, 3, 1]], dtype=np.uint32)
    c = np.array([[0, 2, 4, 4, 4, 7, 2, 3]], dtype=np.uint32)
    h = np.array([[0, 0, 1, 2, 3, 7, 1, 1]], dtype=np.uint32)
    # mean: (2 s + c) / (2 c): 10/4 = 2.5 -> 3, 11/4 = 2.75 -> 3, 12/4 -> 3, 3/2 = 1.5 -> 2, 1/3 -> 0
    assert gm.render_mean((s, c, h), 1).tolist() == [[0, 0, 3, 3, 3, 255, 2, 0]]
    assert gm.render_mean((s, c, h), 3).tolist() == [[0, 0, 3, 3, 3, 255, 0, 0]]          # cnt = min_observations - 1 = 2 -> 0
    assert gm.render_mean((s, c, h), 4).tolist() == [[0, 0, 3, 3, 3, 255, 0, 0]]
    # hits: (200 h + c) / (2 c): 1/4 -> 25, 2/4 -> 50, 3/4 -> 75, 7/7 -> 100, 1/2 -> 50, 1/3 = 33.33 -> 33
    assert gm.render_hits((s, c, h), 1).tolist() == [[-1, 0, 25, 50, 75, 100, 50, 33]]
    assert gm.render_hits((s, c, h), 3).tolist() == [[-1, -1, 25, 50, 75, 100, -1, 33]]
    assert gm.render_hits((s, c, h), 1).dtype == np.int8 and gm.render_mean((s, c, h), 1).dtype == np.uint8
    # values that round: 1/8 = 12.5 % -> 13, 5/8 = 62.5 % -> 63; a mean of 0.5 -> 1
    c8 = np.full((1, 2), 8, dtype=np.uint32)
    assert gm.render_hits((c8, c8, np.array([[1, 5]], dtype=np.uint32)), 1).tolist() == [[13, 63]]
    assert gm.render_mean((np.array([[4, 3]], dtype=np.uint32), c8, c8), 1).tolist() == [[1, 0]]


def test_tables_are_rounded_once():
    c, s = gm.tables(400)
    assert c.dtype == np.float32 and s.dtype == np.float32 and c[0] == 1.0 and s[0] == 0.0
    assert c[100] == np.float32(math.cos(2.0 * math.pi * 100.0 / 400.0)) and c[100] != 0.0 and s[100] == 1.0
    assert np.abs(c.astype(np.float64) ** 2 + s.astype(np.float64) ** 2 - 1.0).max() < 2e-7


def test_the_map_is_sharpest_at_the_true_poses():
    """synth.polar_sequence(11, 6) into a 128 x 128 map of 2 m cells (range_halfwidth 16 = floor(2 / (2 * 0.0595))): the sum, over the
    cells seen by all six scans, of (mean power)^2 is strictly larger at the true poses than with scans 1, 3, 5 moved by
    (0, 0, +0.02 rad), (0, 0, -0.02 rad) or (1 m, 0, 0) in their own frames, and than with every yaw negated.  Measured with this
    restatement (16363 cells seen by all six):
        true poses                3.3586e8
        scans 1, 3, 5 perturbed   3.2530e8   3.2256e8   3.2772e8
        every yaw negated         2.7851e8
    (at 1024 x 1024 cells of 0.5 m, range_halfwidth 4, the issue's prototype gave 6.497e9 / 6.134e9, 6.134e9, 6.061e9 / 4.977e9 at
    10 s per build; 2 m cells keep every inequality at 0.4 s per build)"""
    from navtech_radar_slam_amd import synth
    imgs, _, poses, _ = synth.polar_sequence(11, 6)
    p = gm.params(width=128, height=128, resolution=2.0, origin_x=-128.0, origin_y=-128.0, range_halfwidth=16)

    def energy(P):
        psum, pcnt, _ = gm.add_batch(gm.zeros(p), imgs, gc.matrices(P), p, col_offset=synth.OXFORD_META)
        every = pcnt == len(imgs)
        assert every.sum() > 10000
        return float(((psum[every].astype(np.float64) / len(imgs)) ** 2).sum())

    true = energy(poses)
    others = []
    for d in ((0.0, 0.0, 0.02), (0.0, 0.0, -0.02), (1.0, 0.0, 0.0)):
        P = poses.copy()
        for i in (1, 3, 5):
            P[i] = synth.compose_pose(poses[i], d)
        others.append(energy(P))
    mirrored = poses.copy()
    mirrored[:, 2] = -mirrored[:, 2]
    others.append(energy(mirrored))
    print("energy: true %.4e, perturbed %.4e %.4e %.4e, yaw negated %.4e" % (true, *others))
    assert all(true > e for e in others), (true, others)
