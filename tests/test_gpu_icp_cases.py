"""The ICP kernel (icp.hip through the C-ABI) against the oracle on the cases of tests/icp_cases.py: every convergence
criterion, a correspondence filter that binds, a guess with a rotation, both sides of every size at which the kernel changes
its way, exactly tied neighbours, covariances of rank 1 and 0, non-finite points -- and strides, refused arguments and one
handle over many clouds.  tests/test_icp_cases.py shows on the CPU that the cases are what they claim to be.

The tolerances are those of test_gpu_icp.py against the oracle adding in the device's order: the same state, verdict and
iteration count, the pose to 1e-6, the fitness to 1e-6 relative."""
import ctypes as C

import numpy as np
import pytest

import icp_cases
from icp_cases import DBL_MAX, EXPECTED, oracle_answer

pytestmark = pytest.mark.gpu
BAD_ARG, ERR_RANGE = -1, -6          # RSX_ERR_BAD_ARG, RSX_ERR_RANGE (include/rsx.h)
_max_pose_diff = [0.0]


@pytest.fixture(scope="module")
def icpmod():
    from navtech_radar_slam_amd import _rsx, icp
    assert _rsx.device_count() >= 1
    return icp


def _align(ic, src, tgt, params=None, guess=None):
    for f, v in {**icp_cases.DEFAULTS, **(params or {})}.items():
        setattr(ic.params, f, v)
    return ic.align(src, tgt, guess=guess)


def _same_bytes(a, b):
    return (a["transform"].tobytes() == b["transform"].tobytes() and a["fitness"] == b["fitness"] and a["iterations"] == b["iterations"]
            and a["state"] == b["state"] and a["converged"] == b["converged"])


def _check(name, got, want):
    d = float(np.abs(got["transform"] - want["transform"]).max())
    _max_pose_diff[0] = max(_max_pose_diff[0], d)
    print(f"[icp parity] {name}: state {got['state']}, {got['iterations']} iterations, largest pose difference {d:.3e} "
          f"(largest so far {_max_pose_diff[0]:.3e}), fitness {got['fitness']:.6e} against {want['fitness']:.6e}")
    assert got["state"] == want["state"] and got["converged"] == want["converged"] and got["iterations"] == want["iterations"]
    if name in EXPECTED:
        assert (got["state"], got["iterations"]) == EXPECTED[name]
    assert d < 1e-6
    if want["fitness"] == DBL_MAX:
        assert got["fitness"] == DBL_MAX
    else:
        assert abs(got["fitness"] - want["fitness"]) < 1e-6 * max(1.0, want["fitness"])


def _run_case(icpmod, oracle, case):
    ic = icpmod.Icp()
    try:
        got = _align(ic, case.src, case.tgt, case.params, case.guess)
    finally:
        ic.close()
    _check(case.name, got, oracle_answer(oracle, case))
    return got


@pytest.mark.parametrize("case", icp_cases.param_cases(), ids=lambda c: c.name)
def test_parameters(icpmod, oracle, case):
    """transformation_epsilon, euclidean_fitness_epsilon and max_corr_dist off their defaults: the states ITERATIONS,
    TRANSFORM, ABS_MSE, REL_MSE and no-correspondences, and filters that keep 3 to 76 % of the first correspondences, with the
    correspondences kept in registers (300 source points) and streamed (2500)"""
    _run_case(icpmod, oracle, case)


@pytest.mark.parametrize("case", icp_cases.guess_cases(), ids=lambda c: c.name)
def test_guess_with_a_rotation(icpmod, oracle, case):
    """on the oracle the one-iteration pose moves by 0.148 when the rotation block of the guess is transposed"""
    _run_case(icpmod, oracle, case)


@pytest.mark.parametrize("case", icp_cases.shape_cases(), ids=lambda c: c.name)
def test_size_edges(icpmod, oracle, case):
    """ns = 128 (one source block), 1024 (tree_sum's partial sums wrap), 2048 (correspondences kept or streamed), 128 G (one
    block per workgroup, points in registers, or several, re-read), nt = 2048 Gt (the slice stays in LDS or is reloaded),
    nt < Gt (slices without points), each from both sides.  The last two edges are placed for the G = 256 workgroups of an
    unpartitioned MI355X; on a partitioned device the grid is smaller and they sit elsewhere -- the comparison with the oracle
    holds whatever the grid is."""
    _run_case(icpmod, oracle, case)


@pytest.mark.parametrize("case", icp_cases.tie_cases(), ids=lambda c: c.name)
def test_tied_neighbours(icpmod, oracle, case):
    """four exactly tied nearest neighbours per source point, met across workgroups (100 source points: slices of 16 targets)
    and inside sub-slices (8192), and every target point twice: the lower index wins as in a sequential scan"""
    got = _run_case(icpmod, oracle, case)
    if case.name == "every target point twice":
        ic = icpmod.Icp()
        assert _same_bytes(got, _align(ic, case.src, case.tgt[:len(case.tgt) // 2]))


@pytest.mark.parametrize("case", icp_cases.degenerate_cases(), ids=lambda c: c.name)
def test_degenerate_covariance(icpmod, oracle, case):
    """collinear clouds whose covariance is of rank 1 exactly (the completion of the basis is the oracle's, a quarter turn
    about the z axis included) and a target of one point (H = 0)"""
    _run_case(icpmod, oracle, case)


@pytest.mark.parametrize("case", icp_cases.nonfinite_cases(), ids=lambda c: c.name)
def test_non_finite_points(icpmod, oracle, case):
    """NaN and Inf coordinates: such a point is nobody's neighbour and has none, in the moments and in the fitness count"""
    got = _run_case(icpmod, oracle, case)
    assert np.isfinite(got["transform"]).all()


def _strided(pts, stride):
    out = np.full((len(pts), stride // 4), np.nan, np.float32)          # every padding float is a NaN
    out[:, :3] = pts
    return out


@pytest.mark.parametrize("ns,nt", [icp_cases.SMALL, icp_cases.BIG])
def test_strides(icpmod, ns, nt):
    """source and target at 12, 16 and 32 bytes per point with NaN in the padding: the bytes of the packed call"""
    src, tgt = icp_cases.pair(1, ns, nt, 0.02)
    ic = icpmod.Icp()
    want = _align(ic, src, tgt)
    assert want["state"] == 2 and np.isfinite(want["transform"]).all()
    for ss, ts in ((12, 32), (32, 32), (16, 12), (32, 16), (16, 16), (12, 16)):
        assert _same_bytes(_align(ic, _strided(src, ss), _strided(tgt, ts)), want), (ss, ts)


def test_refused_arguments(icpmod, oracle):
    """rsx_icp_align refuses null arguments, strides that are no multiple of 4 or below 12, max_iterations < 1, max_corr_dist
    <= 0 or NaN (RSX_ERR_BAD_ARG) and clouds beyond the 32-bit indices of the records (RSX_ERR_RANGE, before anything is
    allocated or copied), leaves the result alone, and the handle answers like the oracle afterwards"""
    from navtech_radar_slam_amd import _rsx
    case = next(c for c in icp_cases.param_cases() if c.name == "defaults ns=300")
    src, tgt = np.ascontiguousarray(case.src), np.ascontiguousarray(case.tgt)
    ic = icpmod.Icp()
    L = ic._L
    res = _rsx.IcpResult()
    C.memset(C.byref(res), 0xA5, C.sizeof(res))
    sentinel = bytes(res)

    def call(h=ic._h, s=src.ctypes.data, ns=len(src), ss=12, t=tgt.ctypes.data, nt=len(tgt), ts=12, p=None, out=C.byref(res)):
        return L.rsx_icp_align(h, s, ns, ss, t, nt, ts, C.byref(p) if p is not None else None, None, out)

    refused = [call(h=None), call(out=None), call(s=None), call(t=None)]
    for stride in (8, 14, 0):
        refused += [call(ss=stride), call(ts=stride)]
    for f, v in (("max_iterations", 0), ("max_iterations", -3), ("max_corr_dist", 0.0), ("max_corr_dist", -1.0), ("max_corr_dist", float("nan"))):
        p = _rsx.IcpParams()
        assert L.rsx_icp_default_params(C.byref(p)) == 0
        setattr(p, f, v)
        refused.append(call(p=p))
    assert refused == [BAD_ARG] * len(refused)
    assert call(ns=2 ** 31) == ERR_RANGE and call(nt=2 ** 32 - 1) == ERR_RANGE
    assert bytes(res) == sentinel
    assert call(s=None, ns=0) == 0 and res.state == 5                  # (null with no points is an empty cloud)
    _check("after the refusals", _align(ic, src, tgt), oracle_answer(oracle, case))


def test_one_handle_many_clouds(icpmod):
    """clouds that shrink and grow, with and without a guess, an empty one in between: every answer of the one handle is, byte
    for byte, that of a fresh handle -- no record, current point or guess of an earlier call is seen by a later one"""
    big, small, edge = icp_cases.shape_pair(40000, 3000), icp_cases.shape_pair(129, 40), icp_cases.shape_pair(2049, 6000)
    gsrc, gtgt = icp_cases.pair(2, 300, 1500, 0.02)
    six = dict(max_iterations=6)
    calls = [(*big, six, None), (*small, six, None), (gsrc, gtgt, {}, icp_cases.guess_matrix()), (gsrc, gtgt, {}, None),
             (gsrc[:0], gtgt, {}, None), (*edge, six, None), (*big, six, None)]
    one = icpmod.Icp()
    got = [_align(one, *c) for c in calls]
    for i, c in enumerate(calls):
        fresh = icpmod.Icp()
        assert _same_bytes(got[i], _align(fresh, *c)), i
        fresh.close()
    assert _same_bytes(got[0], got[-1])
    assert got[2]["iterations"] == 3 and got[3]["iterations"] == 6 and not _same_bytes(got[2], got[3])
    assert got[4]["state"] == 5 and got[4]["fitness"] == DBL_MAX
