"""Sub-cell refinement of a pose in the grid map on the GPU (csrc/gridrefine.hip through navtech_radar_slam_amd.gridmap) against its
restatement (tests/gridrefine_np.py): every result record byte for byte, no tolerance -- the order of every sum is part of the rule, so a
difference is a bug."""
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
import gridrefine_cases as grc  # noqa: E402
import gridrefine_np as gr  # noqa: E402
import kstrongest_np as ks  # noqa: E402
import test_gridrefine_abi as abi  # noqa: E402

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
    assert got.dtype.itemsize == want.dtype.itemsize == 152 and len(got) == len(want), what
    for i in range(len(got)):
        assert got[i].tobytes() == want[i].tobytes(), (what, "job", i, got[i], want[i])


@pytest.mark.parametrize("width,height", grc.SIZES)
def test_random_plane_equals_the_restatement(rsx, width, height):
    """a random likelihood: one job for every N of 0, 1, 63, 64, 65, 255, 256, 257, 300, 8192 at every prior in, on and outside every
    border; the reject path, lambda growth, MAX.  The batch whole, reversed and one job at a time, and twice: the same bytes"""
    L, clouds, priors, p = grc.random_case(width, height)
    want = grc.random_reference(width, height)
    assert (want["evaluations"] > want["accepted"] + 1).any() and (want["status"] == gr.STATUS_MAX).any() and (want["accepted"] >= 3).any()
    assert {gr.STATUS_EMPTY, 0} <= set(want["status"].tolist()) and (want["n_inside"] < want["n_points"]).any()
    m = _map(p)
    m.set_likelihood(L)
    got = m.refine(clouds, priors)
    _same(got, want, (width, height))
    assert m.refine(clouds, priors).tobytes() == got.tobytes()
    assert m.refine(clouds[::-1], priors[::-1]).tobytes() == want[::-1].tobytes()
    for i in range(len(clouds)):
        assert m.refine(clouds[i:i + 1], priors[i:i + 1])[0].tobytes() == want[i].tobytes(), ("alone", i)
    m.close()


@pytest.mark.parametrize("max_evaluations", [1, 64])
def test_the_budget(rsx, max_evaluations):
    L, clouds, priors, p = grc.random_case(64, 64)
    want = grc.random_reference(64, 64, max_evaluations)
    assert want["evaluations"].max() == max_evaluations or max_evaluations == 64
    if max_evaluations == 64:
        assert want["evaluations"].max() > 32
    m = _map(p)
    m.set_likelihood(L)
    _same(m.refine(clouds, priors, max_evaluations=max_evaluations), want, max_evaluations)
    m.close()


@pytest.mark.parametrize("width,height", grc.SIZES)
def test_smooth_plane_equals_the_restatement(rsx, width, height):
    """the accept path: a cloud stamped into the plane with a cone of 3 cells around every point, priors off by sub-cell amounts"""
    L, clouds, priors, p, _ = grc.smooth_case(width, height)
    want = grc.smooth_reference(width, height)
    assert (want["accepted"] >= 3).any() and (want["status"] == 0).any() and (want["cost"] < want["cost_initial"]).any()
    m = _map(p)
    m.set_likelihood(L)
    _same(m.refine(clouds, priors), want, (width, height))
    m.close()


@pytest.mark.parametrize("kind", ["zero", "constant"])
def test_edges(rsx, kind):
    """an all-zero plane: EMPTY; a constant plane: SINGULAR after one evaluation; the prior comes back bit for bit"""
    L, clouds, priors, p = grc.edge_case(kind)
    want = grc.reference(L, clouds, priors, p, gr.params())
    assert want[0]["status"] == (gr.STATUS_EMPTY if kind == "zero" else gr.STATUS_SINGULAR) and want[0]["evaluations"] == 1
    m = _map(p)
    m.set_likelihood(L)
    got = m.refine(clouds, priors)
    _same(got, want, kind)
    assert got[0]["transform"].tobytes() == priors[0].tobytes()
    m.close()


def test_status(rsx):
    """a non-finite prior is skipped and its neighbours are untouched; NaN and inf points are skipped without a status; 8193 points get
    POINTS from the device entry and a refusal from the host entry"""
    import torch
    L, clouds, priors, p = grc.random_case(64, 64)
    ref = grc.random_reference(64, 64)
    pick = [72, 45, 73, 63, 36]
    sub_c = [clouds[i] for i in pick]
    m = _map(p)
    m.set_likelihood(L)
    for k, bad in enumerate((np.nan, np.inf, -np.inf)):
        for entry in range(6):
            sub_p = priors[pick].copy()
            sub_p[1 + k, entry] = bad
            want = ref[pick].copy()
            want[1 + k] = np.zeros((), dtype=gr.RESULT)
            want[1 + k]["status"] = gr.STATUS_TRANSFORM
            _same(m.refine(sub_c, sub_p), want, (bad, entry))
    pts = clouds[72].copy()
    pts[[0, 17, 64, 299]] = [(np.nan, 0.0), (1.0, np.inf), (-np.inf, np.nan), (np.nan, np.nan)]
    want = grc.reference(L, [pts], priors[72:73], p, gr.params())
    assert want[0]["n_points"] == 296
    _same(m.refine([pts], priors[72:73]), want, "non-finite points")
    # above the cap
    rng = np.random.default_rng(15)
    big = [clouds[72], gxc.cloud(rng, gr.MAX_POINTS + 1, p), clouds[45]]
    pri = priors[[72, 0, 45]]
    with pytest.raises(rsx.RsxError):
        m.refine(big, pri)
    xy, off = grc.ragged(big)
    d_res = torch.full((3 * 152,), 0xAB, dtype=torch.uint8, device="cuda")
    d_xy, d_off, d_pri = torch.from_numpy(xy).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(np.ascontiguousarray(pri)).cuda()
    torch.cuda.synchronize()          # (the buffers are filled before a stream of the handle's own choosing writes them)
    m.refine_device(d_xy, d_off, d_pri, d_res, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    want = grc.reference(L, big, pri, p, gr.params(), device_entry=True)
    assert want["status"].tolist()[1] == gr.STATUS_POINTS and want[0].tobytes() == ref[72].tobytes()
    _same(d_res.cpu().numpy().view(gr.RESULT), want, "cap")
    m.close()


def test_device_entry_reads_a_packed_cloud_in_place(rsx):
    """point_stride 4 and a cloud whose base address is 4 modulo 16: the bytes of the host entry"""
    import torch
    L, clouds, priors, p = grc.random_case(192, 128)
    ref = grc.random_reference(192, 128)
    pick = [72, 0, 36, 81, 50]
    sub_c, sub_p = [clouds[i] for i in pick], np.ascontiguousarray(priors[pick])
    xy, off = grc.ragged(sub_c)
    m = _map(p)
    m.set_likelihood(L)
    rng = np.random.default_rng(13)
    packed = rng.random((len(xy), 4)).astype(np.float32)          # z and w: anything
    packed[:, :2] = xy
    raw = torch.zeros(4 * len(xy) + 8, dtype=torch.float32, device="cuda")
    shift = (4 - (raw.data_ptr() % 16) // 4 + 1) % 4               # floats to skip for an address of 4 modulo 16
    d_xy = raw[shift:shift + 4 * len(xy)].view(len(xy), 4)
    d_xy.copy_(torch.from_numpy(packed))
    assert d_xy.data_ptr() % 16 == 4 and d_xy.stride(0) == 4
    d_off, d_pri = torch.from_numpy(off).cuda(), torch.from_numpy(sub_p).cuda()
    d_res = torch.full((len(pick) * 152,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()      # (the buffers are filled before a stream of the handle's own choosing writes them)
    m.refine_device(d_xy, d_off, d_pri, d_res, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _same(d_res.cpu().numpy().view(gr.RESULT), ref[pick], "packed")
    m.close()


def test_host_entries_share_one_handle(rsx):
    """refine, match and search stage their points, offsets, priors and records through one set of buffers of the handle: the host
    entries in turn on one handle, with batches that grow and shrink (a buffer left by a larger call serves a smaller one and the other
    way round), each return what a fresh handle returns for that call alone -- records, volumes and bounds byte for byte"""
    L, clouds, priors, p = grc.random_case(64, 64)
    mid = len(clouds) // 2
    calls = [("refine", slice(None), {}),
             ("match", slice(len(clouds) - 2, None), dict(return_scores=True)),            # two jobs of 8192 points
             ("search", slice(mid, mid + 3), dict(return_bounds=True, x_cells=8, y_cells=8)),
             ("refine", slice(mid + 3, mid + 4), {}),
             ("match", slice(None), {})]

    def run(m, name, jobs, options):
        if name == "search":
            m.prepare_search(8)
        out = getattr(m, name)(clouds[jobs], priors[jobs], **options)
        return [a.tobytes() for a in (out if isinstance(out, tuple) else (out,))]

    shared = _map(p)
    shared.set_likelihood(L)
    for step, call in enumerate(calls):
        fresh = _map(p)
        fresh.set_likelihood(L)
        want = run(fresh, *call)
        fresh.close()
        assert len(want[0]) > 0 and run(shared, *call) == want, (step, call[0])
    shared.close()


def test_rules_and_refusals_with_a_handle(rsx):
    """the argument rules of tests/test_gridrefine_abi.py hold with a handle too, and a handle without a likelihood refuses to refine
    and leaves the output buffer untouched"""
    from navtech_radar_slam_amd import gridmap
    m = gridmap.GridMap(64, 96, gridmap.params(width=64, height=64))
    abi.check_argument_rules(rsx, m.handle)
    m.close()
    abi.check_refused_before_a_likelihood(rsx)


def test_end_to_end_equals_the_restatement(rsx):
    """one job from the drive scene: scan 3 against the map of scans 0, 1, 2, 4, 5 with its mean as likelihood, the start (0.9, -0.8) m
    and 0.008 rad off.  Held to equality with the restatement; it recovers the pose because the restatement does
    (tests/test_gridrefine_restatement.py).  The priors are handed over as the records of a match with no window"""
    synth = importlib.import_module("navtech_radar_slam_amd.synth")
    imgs, T, p, pts, priors = gxc.end_to_end(synth, ks.extract)
    planes = gm.add_batch(gm.zeros(p), imgs[gxc.E2E_SCANS], T[gxc.E2E_SCANS], p, col_offset=gc.META)
    L = gx.likelihood(planes, 0)
    truth = grc.e2e_truth(priors)
    start = grc.e2e_starts(truth, [grc.E2E_STARTS[4]])
    m = _map(p, 400, 3360)
    m.add(imgs[gxc.E2E_SCANS], T[gxc.E2E_SCANS])
    m.update_likelihood(0)
    assert m.likelihood().tobytes() == L.tobytes()
    want = grc.reference(L, [pts], start, p, gr.params())
    got = m.refine([pts], m.score([pts], start))
    _same(got, want, "drive")
    dist, dyaw = grc.pose_error(got[0]["transform"], truth)
    assert dist < grc.E2E_LIMIT_M and dyaw < grc.E2E_LIMIT_RAD and got[0]["status"] == 0
    m.close()
