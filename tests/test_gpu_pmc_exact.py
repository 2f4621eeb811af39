"""GPU parity of the EXACT mode of the max-clique inlier selection (RSX_ORORA_PMC_EXACT: pmc_exact_kernel in csrc/pmc.hip,
through the C-ABI) against its restatement (tests/pmc_exact_np.py): integer work -- membership, size and flags are compared
EXACTLY -- and against the oracle's independent exact solver; the solver and the odometry pipeline behind it within the pose
tolerances of tests/test_gpu_pmc.py and tests/test_gpu_odometry.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pmc_exact_np as ex  # noqa: E402
from navtech_radar_slam_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
TAU = 1.5
SOLVER_NODE_CAP = 10_000  # of the oracle's own exact solver (pmcref_exact_size), per pair


@pytest.fixture(scope="module")
def reg():
    from navtech_radar_slam_amd import orora, _rsx
    assert _rsx.device_count() >= 1
    return orora.Orora()


def _same(got_m, got_i, want_m, want_i):
    for f in ("size", "max_core", "seeds", "flags"):
        assert np.array_equal(got_i[f], want_i[f]), (f, np.flatnonzero(got_i[f] != want_i[f])[:5], got_i[got_i[f] != want_i[f]][:5], want_i[got_i[f] != want_i[f]][:5])
    assert np.array_equal(got_m, want_m)


DATA = {"bench": lambda: synth.orora_pairs(777, 40),
        "high_outlier": lambda: synth.orora_high_outlier_pairs(6, 30),
        "bench_slice": lambda: synth.orora_pairs(777, 200)}


@pytest.mark.parametrize("name", list(DATA))
def test_exact_selection_equals_restatement(reg, oracle, name):
    src, dst, off, _ = DATA[name]()
    assert reg.clique_node_budget() == ex.DEFAULT_BUDGET
    m, info = reg.max_clique_batch(src, dst, off, exact=True)
    gm, ginfo = oracle.pmc_select_batch(src, dst, off, TAU, nthreads=8)
    wm, winfo, nodes = ex.exact_batch(oracle, src, dst, off, TAU)
    grew = info["size"] > ginfo["size"]
    print(name, "pairs", len(info), "grew", int(grew.sum()), "entered the search", int((nodes > 0).sum()), "largest node count", int(nodes.max()))
    _same(m, info, wm, winfo)
    assert not (info["flags"] & ex.BUDGET).any() and (info["flags"] & ex.MAXIMUM).all()
    assert grew.any()
    if name == "high_outlier":
        assert sorted(zip(ginfo["size"][grew].tolist(), info["size"][grew].tolist())) == [(3, 8), (4, 12), (4, 15)]
    # the independent solver, on the pairs that grew and as many that did not: it must finish within its cap, and agree
    sub = np.concatenate([np.flatnonzero(grew)[:12], np.flatnonzero(~grew)[:12]])
    for i in sub:
        adj = oracle.pmc_adjacency(src[off[i]:off[i + 1]], dst[off[i]:off[i + 1]], TAU)
        omega = oracle.pmc_exact_size(adj, lb=int(ginfo["size"][i]) - 1, max_nodes=SOLVER_NODE_CAP)
        assert omega > 0, (i, "the independent solver did not finish")
        assert info["size"][i] == omega, (i, info[i], omega)


def test_flag_off_is_byte_identical(reg, oracle):
    from navtech_radar_slam_amd import orora, _rsx
    src, dst, off, _ = synth.orora_pairs(777, 40)
    fresh = orora.Orora()                      # never saw the flag
    m0, i0 = fresh.max_clique_batch(src, dst, off)
    reg.max_clique_batch(src, dst, off, exact=True)
    p = orora.default_params()
    p.flags |= _rsx.ORORA_PMC
    m1, i1 = reg.max_clique_batch(src, dst, off, p)   # the same handle after an exact call
    wm, winfo = oracle.pmc_select_batch(src, dst, off, TAU, nthreads=8)
    assert m0.tobytes() == m1.tobytes() == wm.tobytes() and i0.tobytes() == i1.tobytes() == winfo.tobytes()
    r0 = fresh.register_batch(src, dst, off, p)
    r1 = reg.register_batch(src, dst, off, p)
    assert r0.tobytes() == r1.tobytes()
    fresh.close()


def test_edge_cases(reg, oracle):
    """K = 0, 1 (pass-through), 2, 3, 65, 2048 (the largest pruned pair), 2049 (pass-through); identical points; no edge at all;
    two cliques; a sparse graph of 2048 vertices"""
    rng = np.random.default_rng(11)
    src, dst, off = [], [], [0]

    def add(s, d):
        src.append(np.asarray(s, dtype=np.float32).reshape(-1, 2))
        dst.append(np.asarray(d, dtype=np.float32).reshape(-1, 2))
        off.append(off[-1] + len(src[-1]))

    for k in (0, 1, 2, 3, 65, 2048, 2049):
        s = rng.uniform(-100, 100, (k, 2))
        d = s + [1.0, -2.0] + rng.normal(0, 0.2, (k, 2))
        if k > 8:
            d[::3] = rng.uniform(-100, 100, (len(d[::3]), 2))
        add(s, d)
    add(np.zeros((40, 2)), np.zeros((40, 2)))
    add([[0, 0], [10, 0], [20, 0], [30, 0]], [[0, 0], [50, 0], [150, 0], [300, 0]])
    s = rng.uniform(-60, 60, (85, 2)); d = s.copy(); d[:50] += [3, 0]; d[50:] += [0, -40]
    add(s, d)
    s = rng.uniform(-40, 40, (2048, 2))
    add(s, rng.uniform(-40, 40, (2048, 2)))
    src = np.concatenate(src); dst = np.concatenate(dst); off = np.array(off, dtype=np.int64)
    m, info = reg.max_clique_batch(src, dst, off, exact=True)
    wm, winfo, nodes = ex.exact_batch(oracle, src, dst, off, TAU)
    print("node counts", nodes.tolist(), "sizes", info["size"].tolist(), "flags", info["flags"].tolist())
    _same(m, info, wm, winfo)
    assert info["flags"][[0, 1, 6]].tolist() == [2, 2, 2] and info["size"][6] == 2049
    assert info["size"][7] == 40 and info["flags"][7] == ex.PROVEN | ex.MAXIMUM
    assert info["size"][8] == 1 and info["flags"][8] == ex.PROVEN | ex.MAXIMUM
    assert info["size"][9] == 50


def test_device_entry_with_too_small_a_reservation(oracle):
    import torch
    from navtech_radar_slam_amd import orora, _rsx
    src, dst, off, _ = synth.orora_high_outlier_pairs(6, 30)
    fresh = orora.Orora()
    p = orora.default_params()
    p.flags |= _rsx.ORORA_PMC | _rsx.ORORA_PMC_EXACT
    n = len(off) - 1
    d_src, d_dst, d_off = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda(), torch.from_numpy(off).cuda()
    d_res = torch.zeros((n, 5), dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    with pytest.raises(_rsx.RsxError):
        fresh.register_batch_device(d_src.data_ptr(), d_dst.data_ptr(), d_off.data_ptr(), n, d_res.data_ptr(), p, stream=st)
    fresh.reserve(int(off[n // 2]))
    fresh.register_batch_device(d_src.data_ptr(), d_dst.data_ptr(), d_off.data_ptr(), n, d_res.data_ptr(), p, stream=st)
    torch.cuda.synchronize()
    info = fresh.last_pmc_info(n)
    _, winfo, _ = ex.exact_batch(oracle, src, dst, off, TAU)
    late = info["flags"] & 4 != 0
    assert late[-1] and not late[:n // 2].any()
    assert (info["flags"][late] & 2 != 0).all() and (info["size"][late] == np.diff(off)[late]).all()
    assert np.array_equal(info[~late], winfo[~late])
    res = d_res.cpu().numpy().view(_rsx.ORORA_RESULT_DTYPE).reshape(n)
    assert (res["status"] == 0).all()
    fresh.close()


def test_budget(reg, oracle):
    from navtech_radar_slam_amd import orora, _rsx
    h = orora.Orora()
    for bad in (0, -5):
        with pytest.raises(_rsx.RsxError):
            h.set_clique_node_budget(bad)
    p = orora.default_params()
    p.flags |= _rsx.ORORA_PMC_EXACT          # without ORORA_PMC
    src, dst, off, _ = synth.orora_high_outlier_pairs(6, 30)
    with pytest.raises(_rsx.RsxError):
        h.max_clique_batch(src, dst, off, p)
    with pytest.raises(_rsx.RsxError):
        h.register_batch(src, dst, off, p)
    h.set_clique_node_budget(1)
    assert h.clique_node_budget() == 1
    for name in ("high_outlier", "bench"):
        src, dst, off, _ = DATA[name]()
        m, info = h.max_clique_batch(src, dst, off, exact=True)
        wm, winfo, nodes = ex.exact_batch(oracle, src, dst, off, TAU, budget=1)
        _same(m, info, wm, winfo)
        assert (info["flags"] & ex.BUDGET).any()
        gm, _ = oracle.pmc_select_batch(src, dst, off, TAU, nthreads=8)
        cut = np.repeat(info["flags"] & ex.BUDGET != 0, np.diff(off))
        assert np.array_equal(m[cut], gm[cut])
    h.close()


def test_solver_behind_the_exact_selection(reg, oracle):
    """RSX_ORORA_PMC | RSX_ORORA_PMC_EXACT on the registration entry = the restatement's selection followed by the oracle's
    solver on the selected matches (tolerances of tests/test_gpu_pmc.py::test_solver_behind_the_selection)"""
    from navtech_radar_slam_amd import orora, _rsx
    a = synth.orora_pairs(778, 60)
    b = synth.orora_high_outlier_pairs(6, 30)
    src = np.concatenate([a[0], b[0]]); dst = np.concatenate([a[1], b[1]])
    off = np.concatenate([a[2], a[2][-1] + b[2][1:]])
    p = orora.default_params()
    p.flags |= _rsx.ORORA_PMC | _rsx.ORORA_PMC_EXACT
    got = reg.register_batch(src, dst, off, p)
    info = reg.last_pmc_info(len(off) - 1)
    wm, winfo, _ = ex.exact_batch(oracle, src, dst, off, TAU)
    for f in ("size", "max_core", "seeds", "flags"):
        assert np.array_equal(info[f], winfo[f]), f
    s2, d2, o2 = oracle.pmc_compact(src, dst, off, wm)
    want = oracle.orora_register_batch(s2, d2, o2, nthreads=8)
    assert np.array_equal(got["status"], want["status"])
    for f in ("x", "y", "yaw"):
        assert np.abs(got[f] - want[f]).max() < 1e-4, f
    assert np.array_equal(got["iterations"], want["iterations"]) and np.array_equal(got["rot_inliers"], want["rot_inliers"])


def test_odometry_with_exact_clique(oracle):
    """the moving-sensor drive of tests/test_gpu_odometry.py with exact_clique=True against the CPU chain (oracle/odometry_chain.py's
    steps) fed the restatement's selection; the pose error against truth is printed, not asserted (nobody has measured it)"""
    from navtech_radar_slam_amd import odometry
    po = oracle
    n_scans = 22
    imgs, az, poses, _ = synth.polar_sequence(11, n_scans)
    with pytest.raises(ValueError):
        q = odometry.default_params()
        q.orora.flags &= ~4
        odometry.Odometry(400, 3360, params=q, exact_clique=True)
    od = odometry.Odometry(400, 3360, exact_clique=True)
    res = od.push(imgs, az)
    plain = odometry.Odometry(400, 3360).push(imgs, az)
    fe = po.FrontendRef(rows=400, cols=3360)
    prev, worst_t, worst_y, changed = None, 0.0, 0.0, 0
    for i in range(n_scans):
        tg = po.cen2019_extract(imgs[i], col_offset=11, max_points=10000, min_range=58)[:16384]
        xy = po.cen2019_to_cartesian(tg, az, synth.RADAR_RESOLUTION)
        fe.cartesian(imgs[i], az, synth.RADAR_RESOLUTION, col_offset=11)
        desc, valid = fe.describe(xy)
        if prev is not None:
            fwd, _, _ = fe.match(prev[1], prev[2], desc, valid, ratio=0.8)
            bwd, _, _ = fe.match(desc, valid, prev[1], prev[2], ratio=0.8)
            ii = np.nonzero(fwd >= 0)[0]
            ii = ii[bwd[fwd[ii]] == ii]
            src, dst = xy[fwd[ii]], prev[0][ii]
            o = np.array([0, len(ii)], dtype=np.int64)
            gm, _ = po.pmc_select_batch(src, dst, o, TAU)
            member, info, _ = ex.exact_batch(po, src, dst, o, TAU)
            changed += int(not np.array_equal(gm, member))
            keep = member.astype(bool)
            w = po.orora_register_batch(src[keep], dst[keep], np.array([0, keep.sum()], dtype=np.int64))[0]
            assert res["n_matches"][i] == len(ii)
            assert abs(res["x"][i] - w["x"]) < 1e-4 and abs(res["y"][i] - w["y"]) < 1e-4 and abs(res["yaw"][i] - w["yaw"]) < 1e-4, (i, res[i], w)
            assert res["iterations"][i] == w["iterations"] and res["rot_inliers"][i] == w["rot_inliers"] and res["trans_inliers"][i] == w["trans_inliers"]
            truth = synth.relative_pose(poses[i - 1], poses[i])
            worst_t = max(worst_t, float(np.hypot(res["x"][i] - truth[0], res["y"][i] - truth[1])))
            worst_y = max(worst_y, abs(float(res["yaw"][i] - truth[2])))
        prev = (xy, desc, valid)
    pt = max(float(np.hypot(plain["x"][i] - synth.relative_pose(poses[i - 1], poses[i])[0], plain["y"][i] - synth.relative_pose(poses[i - 1], poses[i])[1])) for i in range(1, n_scans))
    print(f"exact clique: worst pair vs truth {worst_t:.3f} m {worst_y:.2e} rad (greedy: {pt:.3f} m); the selection changed on {changed} of {n_scans - 1} pairs")
