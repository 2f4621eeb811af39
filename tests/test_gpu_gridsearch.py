"""The wide-window correlative search on the GPU (csrc/gridsearch.hip through navtech_radar_slam_amd.gridmap) against its restatement
(tests/gridsearch_np.py): the whole bounds volume and every result record byte for byte, no tolerance; and against the exhaustive
kernel (csrc/gridmatch.hip) on the same handle where the windows overlap."""
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
import gridsearch_cases as gsc  # noqa: E402
import gridsearch_np as gs  # noqa: E402
import kstrongest_np as ks  # noqa: E402
import test_gridsearch_abi as abi  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rsx():
    import __graft_entry__ as ge
    from navtech_radar_slam_amd import _rsx
    if not os.path.exists(_rsx.LIB_PATH):
        ge.build()
    return _rsx


def _map(p, L=None, max_cells=None, rows=64, cols=96):
    from navtech_radar_slam_amd import gridmap
    m = gridmap.GridMap(rows, cols, gridmap.params(**p))
    if L is not None:
        m.set_likelihood(L)
        m.prepare_search(max_cells)
    return m


def _same(got, want, what=""):
    """results and bounds of a batch, byte for byte"""
    (res, bnd), (wres, wbnd) = got, want
    assert bnd.dtype == np.uint32 and bnd.shape == wbnd.shape, what
    bad = np.argwhere(bnd != wbnd)
    assert bnd.tobytes() == wbnd.tobytes(), (what, len(bad), "bounds differ, the first at", bad[:1].tolist())
    assert res.dtype.itemsize == wres.dtype.itemsize == 96 and len(res) == len(wres)
    for i in range(len(res)):
        assert res[i].tobytes() == wres[i].tobytes(), (what, "job", i, res[i], wres[i])


def _check_case(L, clouds, priors, p, mp, what, max_cells=None):
    m = _map(p, L, max(mp["x_cells"], mp["y_cells"]) if max_cells is None else max_cells)
    got = m.search(clouds, priors, return_bounds=True, **mp)
    want = gsc.reference(L, clouds, priors, p, mp)
    _same(got, want, what)
    # the records alone (the bounds then stay in the handle's workspace) are the same records
    assert m.search(clouds, priors, **mp).tobytes() == want[0].tobytes()
    m.close()
    return want


@pytest.mark.parametrize("K,U,V", gsc.WINDOWS)
@pytest.mark.parametrize("width,height", gsc.SIZES)
def test_bounds_and_records_equal_the_restatement(rsx, width, height, K, U, V):
    """a random likelihood; one job for every N of 0, 1, 63, 64, 65, 300, 8192 at every prior in, on and outside every border"""
    L, clouds, priors, p, mp = gsc.volume_case(width + 7 * K + U + V, width, height, K, U, V)
    want = _check_case(L, clouds, priors, p, mp, (width, height, K, U, V))
    assert want[1].any() and {int(s) for s in want[0]["status"]} == {0, gs.STATUS_EMPTY}          # (jobs that score, and EMPTY ones)


def test_the_widest_shifts(rsx):
    """U = V = 256 on 64 x 64 with 300 points: 65 x 65 blocks, a placement margin of 256 cells, the largest frame"""
    K, U, V = gsc.WIDE
    L, clouds, priors, p, mp = gsc.volume_case(31, 64, 64, K, U, V, sizes=[300])
    want = _check_case(L, clouds, priors, p, mp, "wide")
    assert (want[0]["status"] == 0).all() and (want[0]["n_blocks"] == 65 * 65).all()
    assert (want[0]["n_points"] == 300).all()      # with PL = 256 every point of every prior is placed; with 64 some would not be


def test_long_refine_lists(rsx):
    """a random plane under 11 x 7 blocks a rotation: the bounds prune little, so the lists of blocks to refine are long -- the kernel
    takes them sixteen at a time and the rest one at a time, and skips what an exact score found meanwhile rules out"""
    K, U, V = gsc.DENSE
    L, clouds, priors, p, mp = gsc.volume_case(33, 192, 128, K, U, V, sizes=[65, 8192])
    want = _check_case(L, clouds, priors, p, mp, "dense")
    per_k = want[0]["n_refined"] / 3.0
    assert (per_k > 16).sum() >= 6 and (want[0]["n_refined"] % 16 != 0).any()


def test_the_most_rotations(rsx):
    """K = 180 on 64 x 64: tables of 361 entries, one block per rotation"""
    K, U, V = gsc.TURNS
    L, clouds, priors, p, mp = gsc.volume_case(32, 64, 64, K, U, V)
    want = _check_case(L, clouds, priors, p, mp, "turns", max_cells=7)
    assert (want[0]["n_blocks"] == 361).all() and np.abs(want[0]["k"]).max() > 64


@pytest.mark.parametrize("name", sorted(gxc.TIES))
def test_tie_order(rsx, name):
    build, winner = gxc.TIES[name]
    L, clouds, priors, p, mm = build()
    mp = gsc.window(mm["angle_steps"], mm["x_cells"], mm["y_cells"], mm["angle_step"])
    want = _check_case(L, clouds, priors, p, mp, name)
    r = want[0][0]
    assert (int(r["k"]), int(r["u"]), int(r["v"])) == winner
    if name == "zero":
        assert r["status"] == gs.STATUS_EMPTY and r["n_refined"] == 0
    if name == "constant":
        assert r["n_refined"] == r["n_blocks"] and (want[1] == r["score"]).all()      # every bound == T0: pruning is strict


def test_min_score(rsx):
    """one above the peak: BELOW with the prior returned; equal to the peak: the peak"""
    L, clouds, priors, p, mp = gsc.peaked()
    m = _map(p, L, 16)
    for floor, status, kuv in ((0, 0, (0, 5, -3)), (200, 0, (0, 5, -3)), (201, gs.STATUS_BELOW, (0, 0, 0))):
        mq = dict(mp, min_score=floor)
        got, want = m.search(clouds, priors, return_bounds=True, **mq), gsc.reference(L, clouds, priors, p, mq)
        _same(got, want, floor)
        r = got[0][0]
        assert (int(r["k"]), int(r["u"]), int(r["v"])) == kuv and r["status"] == status and r["score"] == (0 if status else 200)
    assert r["transform"].tobytes() == priors[0].tobytes() and r["n_refined"] == 0 and r["n_blocks"] == 18
    m.close()


def test_status(rsx):
    """a non-finite prior is skipped and its neighbours are untouched; 8193 points get POINTS from the device entry and a refusal from
    the host entry; points that are not finite are skipped without a status"""
    import torch
    p = gc.small_params(64, 64)
    rng = np.random.default_rng(15)
    L = gxc.plane(16, p)
    _, pri = gxc.border_priors(p)
    mp = gsc.window(1, 9, 2)
    m = _map(p, L, 9)
    clouds = [gxc.cloud(rng, 200, p) for _ in range(5)]
    clouds[4][[0, 17, 64, 199]] = [(np.nan, 0.0), (1.0, np.inf), (-np.inf, np.nan), (np.nan, np.nan)]
    for k, bad in enumerate((np.nan, np.inf, -np.inf)):
        for entry in (0, 2, 5):
            priors = pri[[0, 1, 0, 2, 0]].copy()
            priors[1 + k, entry] = bad
            got, want = m.search(clouds, priors, return_bounds=True, **mp), gsc.reference(L, clouds, priors, p, mp)
            assert want[0]["status"].tolist().count(gs.STATUS_TRANSFORM) == 1 and not want[1][1 + k].any() and want[0][4]["n_points"] == 196
            _same(got, want, (bad, entry))
    # above the cap
    big = [clouds[0], gxc.cloud(rng, gs.MAX_POINTS + 1, p), clouds[1]]
    with pytest.raises(rsx.RsxError):
        m.search(big, pri[:3], **mp)
    xy, off = gxc.ragged(big)
    want = gsc.reference(L, big, pri[:3], p, mp, device_entry=True)
    assert want[0]["status"].tolist() == [0, gs.STATUS_POINTS, 0]
    d_res = torch.full((3 * 96,), 0xAB, dtype=torch.uint8, device="cuda")
    d_bnd = torch.full((want[1].size,), -1, dtype=torch.int32, device="cuda")
    d_xy, d_off, d_pri = torch.from_numpy(xy).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(np.ascontiguousarray(pri[:3])).cuda()
    torch.cuda.synchronize()          # (the buffers are filled before a stream of the handle's own choosing writes them)
    m.search_device(d_xy, d_off, d_pri, d_res, bounds=d_bnd, stream=torch.cuda.current_stream().cuda_stream, **mp)
    torch.cuda.synchronize()
    _same((d_res.cpu().numpy().view(gs.RESULT), d_bnd.cpu().numpy().view(np.uint32).reshape(want[1].shape)), want, "cap")
    m.close()


def test_device_entry_reads_a_packed_cloud_in_place(rsx):
    """point_stride 4 and a cloud whose base address is 4 modulo 16: the bytes of the host entry; with and without a bounds buffer"""
    import torch
    p = gc.small_params(192, 128)
    rng = np.random.default_rng(13)
    L = gxc.plane(14, p)
    _, pri = gxc.border_priors(p)
    clouds = [gxc.cloud(rng, n, p) for n in (300, 0, 65, 2000)]
    priors = pri[[1, 0, 3, 0]]
    mp = gsc.window(2, 11, 4)
    xy, off = gxc.ragged(clouds)
    m = _map(p, L, 16)
    want = m.search(clouds, priors, return_bounds=True, **mp)
    _same(want, gsc.reference(L, clouds, priors, p, mp), "host")
    packed = rng.random((len(xy), 4)).astype(np.float32)          # z and w: anything
    packed[:, :2] = xy
    raw = torch.zeros(4 * len(xy) + 8, dtype=torch.float32, device="cuda")
    shift = (4 - (raw.data_ptr() % 16) // 4 + 1) % 4               # floats to skip for an address of 4 modulo 16
    d_xy = raw[shift:shift + 4 * len(xy)].view(len(xy), 4)
    d_xy.copy_(torch.from_numpy(packed))
    assert d_xy.data_ptr() % 16 == 4 and d_xy.stride(0) == 4
    d_off, d_pri = torch.from_numpy(off).cuda(), torch.from_numpy(np.ascontiguousarray(priors)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    for with_bounds in (True, False):
        d_res = torch.full((len(clouds) * 96,), 0xAB, dtype=torch.uint8, device="cuda")
        d_bnd = torch.full((want[1].size,), -1, dtype=torch.int32, device="cuda") if with_bounds else None
        torch.cuda.synchronize()      # (the buffers are filled before a stream of the handle's own choosing writes them)
        m.search_device(d_xy, d_off, d_pri, d_res, bounds=d_bnd, stream=stream, **mp)
        torch.cuda.synchronize()
        assert d_res.cpu().numpy().tobytes() == want[0].tobytes()
        if with_bounds:
            assert d_bnd.cpu().numpy().tobytes() == want[1].tobytes()
    m.close()


def test_a_jobs_bytes_do_not_depend_on_the_cut(rsx):
    """a job alone, in a batch, in another order; and through the host entry's sub-batches: at K = 180, U = V = 256 a job's bounds are
    6.1 MB, so the host entry cuts 12 jobs into 10 and 2 where the device entry takes them whole.  A plane with a few lit cells, so
    that few blocks are refined"""
    import torch
    p = gc.small_params(64, 64)
    rng = np.random.default_rng(41)
    L = np.zeros((64, 64), dtype=np.uint8)
    L[rng.integers(0, 64, 12), rng.integers(0, 64, 12)] = rng.integers(100, 256, 12)
    _, pri = gxc.border_priors(p)
    m = _map(p, L, 256)
    # a small window against the restatement
    sizes = [300, 65, 0, 1000, 64]
    clouds = [gxc.cloud(rng, n, p) for n in sizes]
    priors = pri[[0, 1, 2, 4, 0]]
    mp = gsc.window(3, 12, 5)
    want = gsc.reference(L, clouds, priors, p, mp)
    assert want[0]["status"].tolist() == [0, 0, gs.STATUS_EMPTY, 0, 0]
    _same(m.search(clouds, priors, return_bounds=True, **mp), want, "whole")
    for i in range(5):
        res, bnd = m.search(clouds[i:i + 1], priors[i:i + 1], return_bounds=True, **mp)
        assert res[0].tobytes() == want[0][i].tobytes() and bnd[0].tobytes() == want[1][i].tobytes(), ("alone", i)
    order = [3, 2, 1, 0, 4]
    res, bnd = m.search([clouds[i] for i in order], priors[order], return_bounds=True, **mp)
    assert res.tobytes() == want[0][order].tobytes() and bnd.tobytes() == want[1][order].tobytes()
    # the largest window: the device entry (no cut) against the host entry (10 + 2) and against single jobs
    mp = gsc.window(180, 256, 256, angle_step=0.017)
    clouds = [gxc.cloud(rng, 20 + i, p) for i in range(12)]
    priors = pri[[i % 9 for i in range(12)]]
    xy, off = gxc.ragged(clouds)
    host_res, host_bnd = m.search(clouds, priors, return_bounds=True, **mp)
    assert host_bnd.nbytes > 64 << 20 and host_bnd[0].nbytes * 10 <= 64 << 20 < host_bnd[0].nbytes * 11
    d_res = torch.zeros(12 * 96, dtype=torch.uint8, device="cuda")
    d_bnd = torch.zeros(host_bnd.size, dtype=torch.int32, device="cuda")
    d_xy, d_off, d_pri = torch.from_numpy(xy).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(np.ascontiguousarray(priors)).cuda()
    torch.cuda.synchronize()
    m.search_device(d_xy, d_off, d_pri, d_res, bounds=d_bnd, stream=torch.cuda.current_stream().cuda_stream, **mp)
    torch.cuda.synchronize()
    assert d_res.cpu().numpy().tobytes() == host_res.tobytes() and d_bnd.cpu().numpy().tobytes() == host_bnd.tobytes()
    assert (host_res["status"] == 0).sum() >= 8 and (host_res["n_blocks"] == 361 * 65 * 65).all()
    for i in (0, 9, 10, 11):
        res, bnd = m.search(clouds[i:i + 1], priors[i:i + 1], return_bounds=True, **mp)
        assert res[0].tobytes() == host_res[i].tobytes() and bnd[0].tobytes() == host_bnd[i].tobytes(), ("alone", i)
    m.close()


@pytest.mark.parametrize("K,U,V", [(8, 8, 8), (2, 32, 32)])
def test_shared_fields_equal_the_exhaustive_kernel(rsx, K, U, V):
    """within match's caps and without a min_score, search and match on the same handle agree byte for byte on the fields they share"""
    L, clouds, priors, p, mp = gsc.volume_case(50 + K, 192, 128, K, U, V)
    m = _map(p, L, 32)
    got = m.search(clouds, priors, **mp)
    want = m.match(clouds, priors, **gsc.as_match(mp))
    assert {int(s) for s in want["status"]} == {0, gx.STATUS_EMPTY}
    for f in gs.SHARED:
        assert got[f].tobytes() == want[f].tobytes(), f
    m.close()


def test_rules_and_refusals_with_a_handle(rsx):
    """the argument rules of tests/test_gridsearch_abi.py hold with a handle too; no prepare before a likelihood, no search before a
    prepare or beyond the prepared max_cells"""
    from navtech_radar_slam_amd import gridmap
    m = gridmap.GridMap(64, 96, gridmap.params(width=64, height=64))
    abi.check_argument_rules(rsx, m.handle)
    m.close()
    abi.check_refused_before_a_prepare(rsx)


def test_prepare_is_a_snapshot(rsx):
    """after set_likelihood without a new prepare the old snapshot answers (match, which reads the plane itself, sees the new one);
    after a new prepare the new one does; a prepare with another max_cells re-frames the same plane"""
    p = gc.small_params(192, 128)
    rng = np.random.default_rng(19)
    L1, L2 = gxc.plane(20, p), gxc.plane(21, p)
    _, pri = gxc.border_priors(p)
    clouds = [gxc.cloud(rng, 400, p) for _ in pri]
    mp = gsc.window(1, 10, 6)
    want1, want2 = gsc.reference(L1, clouds, pri, p, mp), gsc.reference(L2, clouds, pri, p, mp)
    assert want1[0].tobytes() != want2[0].tobytes()
    m = _map(p, L1, 10)
    _same(m.search(clouds, pri, return_bounds=True, **mp), want1, "first")
    m.set_likelihood(L2)
    _same(m.search(clouds, pri, return_bounds=True, **mp), want1, "stale")
    assert m.match(clouds, pri, **gsc.as_match(mp))["score"].tobytes() == want2[0]["score"].tobytes()
    m.prepare_search(10)
    _same(m.search(clouds, pri, return_bounds=True, **mp), want2, "fresh")
    for cells in (256, 11):
        m.prepare_search(cells)
        _same(m.search(clouds, pri, return_bounds=True, **mp), want2, cells)
    m.close()


@pytest.fixture(scope="module")
def drive():
    synth = importlib.import_module("navtech_radar_slam_amd.synth")
    imgs, T, p, pts, priors = gxc.end_to_end(synth, ks.extract)
    planes = gm.add_batch(gm.zeros(p), imgs[gxc.E2E_SCANS], T[gxc.E2E_SCANS], p, col_offset=gc.META)
    return imgs, T, p, pts, priors, planes


@pytest.mark.parametrize("mode", [0, 1])
def test_end_to_end_equals_the_restatement(rsx, drive, mode):
    """scan 3 of the synthetic drive against the map of scans 0, 1, 2, 4, 5, the prior 20 m and 15 m off, K = 8, U = V = 32: bounds and
    record are the restatement's, which finds the scan again (tests/test_gridsearch_restatement.py)"""
    imgs, T, p, pts, priors, planes = drive
    case = gsc.E2E_NEAR
    mp = gsc.e2e_params(case)
    prior = gsc.moved(priors[case["prior"]], *case["move"])[None]
    m = _map(p, rows=400, cols=3360)
    m.add(imgs[gxc.E2E_SCANS], T[gxc.E2E_SCANS])
    m.update_likelihood(mode)
    m.prepare_search(32)
    L = gx.likelihood(planes, mode)
    want = gsc.reference(L, [pts], prior, p, mp)
    got = m.search([pts], prior, return_bounds=True, **mp)
    _same(got, want, mode)
    r = got[0][0]
    assert (int(r["k"]), int(r["u"]), int(r["v"])) == case["winner"] and int(r["score"]) == case["scores"][mode]
    assert 1 <= r["n_refined"] <= case["share"] * r["n_blocks"]
    m.close()
