"""rsx_phasecorr_* through the C-ABI against tests/phasecorr_np.py: the windowed Cartesian images bit for bit, the rotation curve and the
translation surface (rsx_phasecorr_correlation) and the sub-bin estimates within the bounds below, the integer peaks, half_turn and
status equal; the host and the device entry give the same bytes, and a pair's bytes do not depend on its place in a batch."""
import math

import numpy as np
import pytest

import phasecorr_np as pcn
from test_phasecorr_restatement import COLS, OFF, ROWS, SHIFTS, rotation_scans, wrap

pytestmark = pytest.mark.gpu

# Measured on an MI355X over every pair of `cases` (the first GPU run of the arithmetic as it stands; test_surfaces_and_results prints the values): the
# largest absolute difference between the device's fp32 surfaces and the restatement's fp64 ones (both normalised: a perfect match is 1),
# and between the sub-bin estimates.  The bounds are 8 x the measurement: the order of every sum is fixed, so what varies is fp32
# round-off with the data.  Conditions, not measurements: SURFACE_BOUND < 1e-3 (1/40 of the smallest runner-up of a right peak:
# above it the comparison could hide a swapped peak), SHIFT_BOUND < 0.01 pixel, ANGLE_BOUND < 0.01 angle bin.
SURFACE_MEASURED, SHIFT_MEASURED, ANGLE_MEASURED = 1.10e-7, 8.8e-9, 5.25e-7   # surfaces (of 1), pixels, angle bins
SURFACE_BOUND, SHIFT_BOUND, ANGLE_BOUND = 8 * SURFACE_MEASURED, 8 * SHIFT_MEASURED, 8 * ANGLE_MEASURED   # 8.8e-7, 7.0e-8 px, 4.2e-6 bins
SEVEN = [(1, 0), (2, 1), (3, 2), (4, 3), (5, 4), (2, 0), (0, 0)]   # scan 2 is src of two pairs and dst of a third; the last is a scan with itself


@pytest.fixture(scope="module")
def pc():
    import os
    import __graft_entry__ as ge
    from navtech_radar_slam_amd import _rsx, phasecorr
    if not os.path.exists(_rsx.LIB_PATH):
        ge.build()
    return phasecorr


@pytest.fixture(scope="module")
def drive():
    from navtech_radar_slam_amd import synth
    return synth.polar_sequence(3, 6)


@pytest.fixture(scope="module")
def cases(drive):
    """name -> (params, images, pairs, the restatement's results); computed once, never written to"""
    rot = rotation_scans()
    rot_pairs = [(1 + i, 0) for i in range(len(SHIFTS))]
    spec = {"drive256": ({}, drive[0], SEVEN), "rot256": ({}, rot, rot_pairs), "rot64": (dict(n=64, resolution=2.0), rot, rot_pairs),
            "one512": (dict(n=512, resolution=0.25), drive[0][:2], [(1, 0)])}
    out = {}
    for name, (fields, imgs, pairs) in spec.items():
        want, _ = pcn.Restatement(ROWS, COLS, fields).register_batch(imgs, pairs, col_offset=OFF)
        out[name] = (fields, imgs, pairs, want)
    return out


@pytest.fixture(scope="module")
def runs(pc, cases):
    """name -> (results, [(curve, surface)] per pair) of the host entry"""
    out = {}
    for name, (fields, imgs, pairs, _) in cases.items():
        h = pc.Phasecorr(ROWS, COLS, pc.params(**fields))
        res = h.register_batch(imgs, pairs, col_offset=OFF)
        out[name] = (res, [h.correlation(i) for i in range(len(pairs))])
        h.close()
    return out


@pytest.mark.parametrize("n,res", [(64, 2.0), (256, 0.5), (512, 0.25)])
def test_cartesian_images_bit_identical(pc, n, res):
    from navtech_radar_slam_amd import synth
    imgs = synth.polar_sequence(3, 4)[0]   # rows = 400, the samples behind 11 bytes of row header
    h = pc.Phasecorr(ROWS, COLS, pc.params(n=n, resolution=res))
    got_res, got = h.register_batch(imgs, np.zeros((0, 2), dtype=np.int32), col_offset=OFF, cart=True)
    tab = pcn.Tables(dict(pcn.default_params(), n=n, resolution=res), ROWS, COLS)
    assert len(got_res) == 0 and got.shape == (4, n, n)
    for i in range(4):
        want = pcn.cart_image(imgs[i], OFF, tab)
        assert want.max() > 50 and np.array_equal(got[i].view(np.uint32), want.view(np.uint32)), (n, i, np.abs(got[i] - want).max())
    h.close()


def test_surfaces_and_results(cases, runs):
    worst = dict(surface=0.0, shift=0.0, angle=0.0)
    for name, (fields, imgs, pairs, want) in cases.items():
        res, corr = runs[name]
        n = fields.get("n", 256)
        pix = fields.get("resolution", 0.5)
        for i, (w, (curve, surf)) in enumerate(zip(want, corr)):
            ds, dc = np.abs(surf - w["surface"]).max(), np.abs(curve - w["rot_curve"]).max()
            dx, dy = abs(res["x"][i] - w["x"]) / pix, abs(res["y"][i] - w["y"]) / pix
            dt = abs(wrap(res["theta"][i] - w["theta"])) / (math.pi / n)
            dp = max(abs(res["peak"][i] - w["peak"]), abs(res["rot_peak"][i] - w["rot_peak"]))
            print(f"{name} pair {pairs[i]}: surface {ds:.3e} curve {dc:.3e} peaks {dp:.3e} | x {dx:.3e} y {dy:.3e} px theta {dt:.3e} bins | "
                  f"peak {res['peak'][i]:.4f} ratio {res['peak_ratio'][i]:.4f} rot_peak {res['rot_peak'][i]:.4f}")
            worst["surface"] = max(worst["surface"], ds, dc, dp)
            worst["shift"] = max(worst["shift"], dx, dy)
            worst["angle"] = max(worst["angle"], dt)
            # the integer peaks, the branch and the status are the restatement's
            assert int(np.argmax(curve)) == w["rot_k0"], (name, i)
            assert divmod(int(np.argmax(surf)), n) == w["peak_ij"], (name, i)
            assert res["half_turn"][i] == w["half_turn"] and res["status"][i] == w["status"] == 0, (name, i)
            assert abs(res["peak_ratio"][i] - w["peak_ratio"]) <= 2 * SURFACE_BOUND / w["peak"] + 1e-12, (name, i)
    print("measured:", worst)
    assert SURFACE_BOUND < 1e-3 and SHIFT_BOUND < 0.01 and ANGLE_BOUND < 0.01
    assert worst["surface"] <= SURFACE_BOUND and worst["shift"] <= SHIFT_BOUND and worst["angle"] <= ANGLE_BOUND, worst


def test_a_scan_with_itself(cases, runs):
    res, corr = runs["drive256"]
    i = SEVEN.index((0, 0))
    assert res["x"][i] == 0.0 and res["y"][i] == 0.0 and res["theta"][i] == 0.0 and res["half_turn"][i] == 0 and res["status"][i] == 0
    assert abs(res["peak"][i] - 1.0) <= SURFACE_BOUND and abs(res["rot_peak"][i] - 1.0) <= SURFACE_BOUND
    assert abs(corr[i][1][0, 0] - 1.0) <= SURFACE_BOUND and abs(corr[i][0][0] - 1.0) <= SURFACE_BOUND


def test_rotations_and_drive_come_back(cases, runs, drive):
    """the library's own estimates meet what tests/test_phasecorr_restatement.py asks of the restatement"""
    from navtech_radar_slam_amd import synth
    for name, n, pix in (("rot256", 256, 0.5), ("rot64", 64, 2.0)):
        res = runs[name][0]
        for k, r in zip(SHIFTS, res):
            want = wrap(-k * 2.0 * math.pi / ROWS)
            assert abs(wrap(r["theta"] - want)) <= math.pi / n and abs(r["x"]) < pix and abs(r["y"]) < pix, (name, k, r)
            if abs(abs(want) - math.pi / 2) > math.pi / n:
                assert r["half_turn"] == (1 if abs(want) > math.pi / 2 else 0), (name, k)
    res, poses = runs["drive256"][0], drive[2]
    for i in range(5):
        want = synth.relative_pose(poses[i], poses[i + 1])
        assert abs(res["x"][i] - want[0]) <= 0.5 and abs(res["y"][i] - want[1]) <= 0.5 and abs(wrap(res["theta"][i] - want[2])) <= math.pi / 256
        assert res["peak_ratio"][i] <= 0.5


def test_entries_agree_and_batches_do_not_matter(pc, cases, runs):
    import torch
    _, imgs, pairs, _ = cases["drive256"]
    res7 = runs["drive256"][0]
    h = pc.Phasecorr(ROWS, COLS)
    n = h.params.n
    # the device entry, on a stream of the caller's
    d_imgs = torch.from_numpy(np.ascontiguousarray(imgs)).cuda()
    d_pairs = torch.tensor(pairs, dtype=torch.int32, device="cuda")
    d_res = torch.full((len(pairs) * 56,), 99, dtype=torch.uint8, device="cuda")
    d_cart = torch.full((len(imgs), n, n), 99.0, dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    h.register_batch_device(d_imgs.data_ptr(), len(imgs), imgs.strides[0], imgs.strides[1], OFF, d_pairs.data_ptr(), len(pairs), d_res.data_ptr(),
                            d_cart=d_cart.data_ptr(), stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert d_res.cpu().numpy().tobytes() == res7.tobytes()
    host_res, host_cart = h.register_batch(imgs, pairs, col_offset=OFF, cart=True)
    assert host_res.tobytes() == res7.tobytes() and np.array_equal(d_cart.cpu().numpy().view(np.uint32), host_cart.view(np.uint32))
    # 1 against 7, and the seven in another order
    for i in (2, 5, 6):
        one = h.register_batch(imgs, [pairs[i]], col_offset=OFF)
        assert one.tobytes() == res7[i:i + 1].tobytes(), i
    back = h.register_batch(imgs, pairs[::-1], col_offset=OFF)
    assert back[::-1].tobytes() == res7.tobytes()
    # the same scans at other indices of the batch
    perm = [3, 0, 5, 1, 4, 2]   # new index i holds old scan perm[i]
    inv = {old: new for new, old in enumerate(perm)}
    moved = h.register_batch(imgs[perm], [(inv[a], inv[b]) for a, b in pairs], col_offset=OFF)
    assert moved.tobytes() == res7.tobytes()
    # a pair outside the batch: the device entry marks it and computes the others
    d_pairs2 = torch.tensor([(1, 0), (6, 0), (0, -1)], dtype=torch.int32, device="cuda")
    d_res2 = torch.full((3 * 56,), 99, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    h.register_batch_device(d_imgs.data_ptr(), len(imgs), imgs.strides[0], imgs.strides[1], OFF, d_pairs2.data_ptr(), 3, d_res2.data_ptr())
    torch.cuda.synchronize()
    from navtech_radar_slam_amd import _rsx
    got = np.frombuffer(d_res2.cpu().numpy().tobytes(), dtype=_rsx.PHASECORR_RESULT_DTYPE)
    assert got[0:1].tobytes() == res7[0:1].tobytes()
    assert got["status"][1] == got["status"][2] == _rsx.PHASECORR_STATUS_INDEX and got["peak"][1] == 0.0
    with pytest.raises(_rsx.RsxError):
        h.correlation(1)
    h.close()


def test_error_paths(pc, cases):
    from navtech_radar_slam_amd import _rsx
    _, imgs, _, want = cases["rot256"]
    for fields in (dict(n=100), dict(n=1024), dict(n=512, resolution=1.0)):   # a bad N; a disc larger than the image
        with pytest.raises(_rsx.RsxError) as e:
            pc.Phasecorr(ROWS, COLS, pc.params(**fields))
        assert e.value.status == -1
    h = pc.Phasecorr(ROWS, COLS)
    for pairs in ([(0, 6)], [(-1, 0)], [(1, 0), (6, 6)]):
        with pytest.raises(_rsx.RsxError) as e:
            h.register_batch(imgs, pairs, col_offset=OFF)
        assert e.value.status == -1 and "outside the batch" in str(e.value)
    with pytest.raises(_rsx.RsxError):
        h.register_batch(imgs, [(1, 0)], col_offset=OFF + 1)   # the samples would run past the row
    with pytest.raises(_rsx.RsxError):
        h.correlation(0)   # no call yet
    h.close()
    # a limit below the truth: the pair is reported as found, and marked (k = 100 rows: a quarter turn)
    h = pc.Phasecorr(ROWS, COLS, pc.params(max_rotation=0.5))
    res = h.register_batch(imgs, [(3, 0), (1, 0)], col_offset=OFF)
    lim, _ = pcn.Restatement(ROWS, COLS, dict(max_rotation=0.5)).register_batch(imgs, [(3, 0), (1, 0)], col_offset=OFF)
    assert res["status"].tolist() == [_rsx.PHASECORR_STATUS_ROTATION, 0] == [w["status"] for w in lim]
    assert abs(wrap(res["theta"][0] - want[2]["theta"])) < 1e-3
    h.close()
