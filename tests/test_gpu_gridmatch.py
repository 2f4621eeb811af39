"""Correlative scan-to-map matching on the GPU (csrc/gridmatch.hip through navtech_radar_slam_amd.gridmap) against its restatement
(tests/gridmatch_np.py): the likelihood plane, the whole score volume and every result record byte for byte, no tolerance."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gridmap_cases as gc  # noqa: E402
import gridmap_np as gm  # noqa: E402
import gridmatch_cases as gxc  # noqa: E402
import gridmatch_np as gx  # noqa: E402
import kstrongest_np as ks  # noqa: E402
import test_gridmatch_abi as abi  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rsx():
    import __graft_entry__ as ge
    from navtech_radar_slam_amd import _rsx
    if not os.path.exists(_rsx.LIB_PATH):
        ge.build()
    return _rsx


def _map(p, rows=64, cols=96):
    from navtech_radar_slam_amd import gridmap
    return gridmap.GridMap(rows, cols, gridmap.params(**p))


def _same(got, want, what=""):
    """results and volumes of a batch, byte for byte"""
    (res, vol), (wres, wvol) = got, want
    assert vol.dtype == np.uint32 and vol.shape == wvol.shape, what
    bad = np.argwhere(vol != wvol)
    assert vol.tobytes() == wvol.tobytes(), (what, len(bad), "scores differ, the first at", bad[:1].tolist())
    assert res.dtype.itemsize == wres.dtype.itemsize == 88 and len(res) == len(wres)
    for i in range(len(res)):
        assert res[i].tobytes() == wres[i].tobytes(), (what, "job", i, res[i], wres[i])


@pytest.mark.parametrize("K,U,V", gxc.WINDOWS)
@pytest.mark.parametrize("width,height", gxc.SIZES)
def test_volume_and_records_equal_the_restatement(rsx, width, height, K, U, V):
    """a random likelihood; one job for every N of 0, 1, 63, 64, 65, 300, 8192 at every prior in, on and outside every border"""
    L, clouds, priors, p, mp = gxc.volume_case(width + 7 * K + U + V, width, height, K, U, V)
    m = _map(p)
    m.set_likelihood(L)
    assert m.likelihood().tobytes() == L.tobytes()
    got = m.match(clouds, priors, return_scores=True, **mp)
    want = gxc.reference(L, clouds, priors, p, mp)
    assert want[1].any() and len({int(s) for s in want[0]["status"]}) == 2          # (jobs that score, and EMPTY ones)
    _same(got, want, (width, height, K, U, V))
    # the records alone (the volume then stays in the handle's workspace) are the same records
    assert m.match(clouds, priors, **mp).tobytes() == want[0].tobytes()
    m.close()


@pytest.mark.parametrize("min_observations", [1, 3])
@pytest.mark.parametrize("mode", [0, 1])
def test_likelihood_update_equals_the_restated_render(rsx, mode, min_observations):
    imgs, T, p = gc.random_case(77, 64, 96, 192, 128, 6)
    m = _map(p)
    m.add(imgs, T)
    planes = gm.add_batch(gm.zeros(p), imgs, T, p, col_offset=gc.META)
    want = gx.likelihood(planes, mode, min_observations)
    assert want.any() and (planes[1] < min_observations).any() and (planes[1] >= 3).any()
    m.update_likelihood(mode, min_observations)
    got = m.likelihood()
    assert got.dtype == np.uint8 and got.tobytes() == want.tobytes()
    assert m.likelihood((5, 9, 100, 40)).tobytes() == want[9:49, 5:105].tobytes()
    if mode == 0:
        assert got.tobytes() == m.mean(min_observations).tobytes()
    else:
        assert got.tobytes() == np.maximum(m.hits(min_observations), 0).astype(np.uint8).tobytes()
    # a snapshot: the planes go on, the likelihood stays until the next update; and a match reads it
    m.add(imgs[:2], T[:2])
    assert m.likelihood().tobytes() == want.tobytes()
    rng = np.random.default_rng(4)
    clouds = [gxc.cloud(rng, 500, p)]
    _, priors = gxc.border_priors(p)
    mp = gxc.window(2, 5, 3)
    _same(m.match(clouds, priors[:1], return_scores=True, **mp), gxc.reference(want, clouds, priors[:1], p, mp), (mode, min_observations))
    m.close()


def test_ragged_batch_and_its_cuts(rsx):
    """an empty job in the middle; a job's bytes alone, first, last, and with the batch cut in two"""
    p = gc.small_params(192, 128)
    rng = np.random.default_rng(11)
    L = gxc.plane(12, p)
    _, pri = gxc.border_priors(p)
    sizes = [300, 65, 0, 1000, 64]
    clouds = [gxc.cloud(rng, n, p) for n in sizes]
    priors = pri[[0, 1, 2, 4, 0]]
    mp = gxc.window(3, 6, 2)
    m = _map(p)
    m.set_likelihood(L)
    want = gxc.reference(L, clouds, priors, p, mp)
    assert want[0]["status"].tolist() == [0, 0, gx.STATUS_EMPTY, 0, 0]
    _same(m.match(clouds, priors, return_scores=True, **mp), want, "whole")
    for i in range(5):
        res, vol = m.match(clouds[i:i + 1], priors[i:i + 1], return_scores=True, **mp)
        assert res[0].tobytes() == want[0][i].tobytes() and vol[0].tobytes() == want[1][i].tobytes(), ("alone", i)
    order = [3, 2, 1, 0, 4]          # job 3 first, job 0 neither first nor last
    res, vol = m.match([clouds[i] for i in order], priors[order], return_scores=True, **mp)
    assert res.tobytes() == want[0][order].tobytes() and vol.tobytes() == want[1][order].tobytes()
    for cut in (1, 2, 3):
        a = m.match(clouds[:cut], priors[:cut], return_scores=True, **mp)
        b = m.match(clouds[cut:], priors[cut:], return_scores=True, **mp)
        _same((np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])), want, ("cut", cut))
    m.close()


def test_device_entry_reads_a_packed_cloud_in_place(rsx):
    """point_stride 4 and a cloud whose base address is 4 modulo 16: the bytes of the host entry; with and without a score buffer"""
    import torch
    p = gc.small_params(192, 128)
    rng = np.random.default_rng(13)
    L = gxc.plane(14, p)
    _, pri = gxc.border_priors(p)
    clouds = [gxc.cloud(rng, n, p) for n in (300, 0, 65, 2000)]
    priors = pri[[1, 0, 3, 0]]
    mp = gxc.window(2, 7, 4)
    xy, off = gxc.ragged(clouds)
    m = _map(p)
    m.set_likelihood(L)
    want = m.match(clouds, priors, return_scores=True, **mp)
    _same(want, gxc.reference(L, clouds, priors, p, mp), "host")
    packed = rng.random((len(xy), 4)).astype(np.float32)          # z and w: anything
    packed[:, :2] = xy
    raw = torch.zeros(4 * len(xy) + 8, dtype=torch.float32, device="cuda")
    shift = (4 - (raw.data_ptr() % 16) // 4 + 1) % 4               # floats to skip for an address of 4 modulo 16
    d_xy = raw[shift:shift + 4 * len(xy)].view(len(xy), 4)
    d_xy.copy_(torch.from_numpy(packed))
    assert d_xy.data_ptr() % 16 == 4 and d_xy.stride(0) == 4
    d_off, d_pri = torch.from_numpy(off).cuda(), torch.from_numpy(np.ascontiguousarray(priors)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    for with_scores in (True, False):
        d_res = torch.full((len(clouds) * 88,), 0xAB, dtype=torch.uint8, device="cuda")
        d_vol = torch.full((want[1].size,), -1, dtype=torch.int32, device="cuda") if with_scores else None
        torch.cuda.synchronize()      # (the buffers are filled before a stream of the handle's own choosing writes them)
        m.match_device(d_xy, d_off, d_pri, d_res, scores=d_vol, stream=stream, **mp)
        torch.cuda.synchronize()
        assert d_res.cpu().numpy().tobytes() == want[0].tobytes()
        if with_scores:
            assert d_vol.cpu().numpy().tobytes() == want[1].tobytes()
    m.close()


def test_status(rsx):
    """a non-finite prior is skipped and its neighbours are untouched; 8193 points get POINTS from the device entry and a refusal
    from the host entry; NaN and inf points are skipped without a status"""
    import torch
    p = gc.small_params(64, 64)
    rng = np.random.default_rng(15)
    L = gxc.plane(16, p)
    _, pri = gxc.border_priors(p)
    mp = gxc.window(1, 3, 2)
    m = _map(p)
    m.set_likelihood(L)
    clouds = [gxc.cloud(rng, 200, p) for _ in range(5)]
    for k, bad in enumerate((np.nan, np.inf, -np.inf)):
        for entry in range(6):
            priors = pri[[0, 1, 0, 2, 0]].copy()
            priors[1 + k, entry] = bad
            got, want = m.match(clouds, priors, return_scores=True, **mp), gxc.reference(L, clouds, priors, p, mp)
            assert want[0]["status"].tolist().count(gx.STATUS_TRANSFORM) == 1 and not want[1][1 + k].any()
            _same(got, want, (bad, entry))
    # points that are not finite: skipped, no status, not counted
    pts = gxc.cloud(rng, 300, p)
    pts[[0, 17, 64, 299]] = [(np.nan, 0.0), (1.0, np.inf), (-np.inf, np.nan), (np.nan, np.nan)]
    want = gxc.reference(L, [pts], pri[:1], p, mp)
    assert want[0][0]["status"] == 0 and want[0][0]["n_points"] == 296
    _same(m.match([pts], pri[:1], return_scores=True, **mp), want, "non-finite points")
    # above the cap
    big = [clouds[0], gxc.cloud(rng, gx.MAX_POINTS + 1, p), clouds[1]]
    with pytest.raises(rsx.RsxError):
        m.match(big, pri[:3], **mp)
    xy, off = gxc.ragged(big)
    d_res = torch.full((3 * 88,), 0xAB, dtype=torch.uint8, device="cuda")
    d_vol = torch.full((3 * 3 * 5 * 7,), -1, dtype=torch.int32, device="cuda")
    d_xy, d_off, d_pri = torch.from_numpy(xy).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(np.ascontiguousarray(pri[:3])).cuda()
    torch.cuda.synchronize()          # (the buffers are filled before a stream of the handle's own choosing writes them)
    m.match_device(d_xy, d_off, d_pri, d_res, scores=d_vol, stream=torch.cuda.current_stream().cuda_stream, **mp)
    torch.cuda.synchronize()
    want = gxc.reference(L, big, pri[:3], p, mp, device_entry=True)
    assert want[0]["status"].tolist() == [0, gx.STATUS_POINTS, 0]
    _same((d_res.cpu().numpy().view(gx.RESULT), d_vol.cpu().numpy().view(np.uint32).reshape(want[1].shape)), want, "cap")
    m.close()


@pytest.mark.parametrize("name", sorted(gxc.TIES))
def test_tie_order(rsx, name):
    build, winner = gxc.TIES[name]
    L, clouds, priors, p, mp = build()
    m = _map(p)
    m.set_likelihood(L)
    got, want = m.match(clouds, priors, return_scores=True, **mp), gxc.reference(L, clouds, priors, p, mp)
    assert (int(want[0][0]["k"]), int(want[0][0]["u"]), int(want[0][0]["v"])) == winner
    _same(got, want, name)
    m.close()


def test_rules_and_refusals_with_a_handle(rsx):
    """the argument rules of tests/test_gridmatch_abi.py hold with a handle too, and a handle without a likelihood refuses to match"""
    from navtech_radar_slam_amd import gridmap
    m = gridmap.GridMap(64, 96, gridmap.params(width=64, height=64))
    abi.check_argument_rules(rsx, m.handle)
    m.close()
    abi.check_refused_before_a_likelihood(rsx)


def test_score_and_likelihood_device(rsx):
    """score() is match with no window; the device pointer of the likelihood plane is cell (0, 0) at its pitch"""
    p = gc.small_params(192, 128)
    rng = np.random.default_rng(17)
    L = gxc.plane(18, p)
    names, pri = gxc.border_priors(p)
    clouds = [gxc.cloud(rng, 400, p) for _ in pri]
    m = _map(p)
    m.set_likelihood(L)
    want = gxc.reference(L, clouds, pri, p, gxc.window(0, 0, 0))[0]
    assert m.score(clouds, pri).tobytes() == want.tobytes()
    assert (want["score"] == want["score_prior"]).all() and not want["score_runner_up"].any()
    d, pitch = m.likelihood_device()
    assert pitch == 192 + 256
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    row = np.zeros(192, dtype=np.uint8)
    for y in (0, 77, 127):
        assert hip.hipMemcpy(row.ctypes.data, d + y * pitch, 192, 2) == 0 and row.tobytes() == L[y].tobytes()      # (2: device to host)
    # a caller that writes the plane itself: one row, in place
    L2 = L.copy()
    L2[77] = 255 - L[77]
    assert hip.hipMemcpy(d + 77 * pitch, L2[77].ctypes.data, 192, 1) == 0                                             # (1: host to device)
    assert m.likelihood().tobytes() == L2.tobytes()
    assert m.score(clouds, pri).tobytes() == gxc.reference(L2, clouds, pri, p, gxc.window(0, 0, 0))[0].tobytes()
    m.close()


@pytest.fixture(scope="module")
def drive():
    synth = importlib.import_module("navtech_radar_slam_amd.synth")
    imgs, T, p, pts, priors = gxc.end_to_end(synth, ks.extract)
    planes = gm.add_batch(gm.zeros(p), imgs[gxc.E2E_SCANS], T[gxc.E2E_SCANS], p, col_offset=gc.META)
    return imgs, T, p, pts, priors, planes


@pytest.mark.parametrize("mode", [0, 1])
def test_end_to_end_equals_the_restatement(rsx, drive, mode):
    """scan 3 of the synthetic drive against the map of scans 0, 1, 2, 4, 5, K = U = V = 8: map, likelihood, volume and records are
    the restatement's (which recovers the three prior errors exactly: tests/test_gridmatch_restatement.py)"""
    imgs, T, p, pts, priors, planes = drive
    m = _map(p, 400, 3360)
    m.add(imgs[gxc.E2E_SCANS], T[gxc.E2E_SCANS])
    m.update_likelihood(mode)
    L = gx.likelihood(planes, mode)
    assert m.likelihood().tobytes() == L.tobytes()
    want = gxc.reference(L, [pts] * 3, priors, p, gx.params(**gxc.E2E_WINDOW))
    got = m.match([pts] * 3, priors, return_scores=True, **gxc.E2E_WINDOW)
    _same(got, want, mode)
    assert [(int(r["k"]), int(r["u"]), int(r["v"])) for r in got[0]] == gxc.E2E_WINNERS
    assert int(got[0][0]["score"]) == (1144127, 469444)[mode]
    m.close()
