"""The pair entries rsx_cfear_register_batch[_device] against bytes RECORDED from the parent build.

Since the pair entries run the joint kernel (csrc/cfear_track.hip) with one keyframe per job at the identity pose, the K = 1
test of tests/test_gpu_cfear_track.py compares a build with itself for search 0.  The pin therefore comes from
tests/golden/cfear_pairs_parent.npz: the raw 48-byte rsx_cfear_result records that the last build WITH a pair kernel of its
own (commit a46f554) returned for the 13 pairs of cfear_track_cases.pair_cases(), recorded once on an MI355X by
tools/make_cfear_pairs_golden.py.  Both entries must return those bytes.  The fixture's input bytes are hashed and compared
first, so that a moved fixture is not mistaken for a moved kernel.

The joint kernel strides jobs over at most 256 workgroups, which the pair kernel (one workgroup per pair) never did: a batch
of 257 pairs makes workgroup 0 take jobs 0 and 256, and every result must be the bytes of the same pair registered alone."""
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cfear_track_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cfear_pairs_parent.npz")
MAX_JOINT_BLOCKS = 256  # csrc/cfear_track.hip


def input_hash():
    """SHA-256 over every group's parameter overrides, src and dst record bytes and inits, in pair_groups() order"""
    h = hashlib.sha256()
    for key, cs, init in cases.pair_groups():
        h.update(repr(key).encode())
        for c in cs:
            h.update(np.ascontiguousarray(c[1]).tobytes())
            h.update(np.ascontiguousarray(c[2]).tobytes())
        h.update(np.ascontiguousarray(init, dtype=np.float64).tobytes())
    return h.hexdigest()


def measure(handle):
    """-> per parameter group of pair_groups() the (n,) result records of the host entry Cfear.register"""
    from navtech_radar_slam_amd import cfear
    return [handle.register([c[1] for c in cs], [c[2] for c in cs], init, cfear.params(**dict(key))) for key, cs, init in cases.pair_groups()]


@pytest.fixture(scope="module")
def handle():
    from navtech_radar_slam_amd import cfear
    h = cfear.Cfear()
    yield h
    h.close()


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_the_fixture_is_the_recorded_one(golden):
    assert str(golden["input_sha256"]) == input_hash()
    assert int(golden["n_groups"]) == len(cases.pair_groups()) and sum(len(cs) for _, cs, _ in cases.pair_groups()) == 13


def test_host_and_device_entries_return_the_parent_bytes(handle, golden):
    import torch
    from navtech_radar_slam_amd import _rsx, cfear
    assert str(golden["input_sha256"]) == input_hash()
    got = measure(handle)
    stream = torch.cuda.Stream()
    for g, (key, cs, init) in enumerate(cases.pair_groups()):
        want = golden[f"results_{g}"].tobytes()
        assert len(want) == 48 * len(cs)
        assert [int(r["status"]) for r in got[g]] == [c[5] for c in cs]
        for c, r, w in zip(cs, got[g], np.frombuffer(want, dtype=_rsx.CFEAR_RESULT_DTYPE)):
            assert r.tobytes() == w.tobytes(), ("host entry", c[0], r, w)
        s, so = cfear.ragged([c[1] for c in cs], _rsx.CFEAR_SURFACE_POINT_DTYPE)
        d, do = cfear.ragged([c[2] for c in cs], _rsx.CFEAR_SURFACE_POINT_DTYPE)
        dev = [torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a).cuda() for a in (s, so, d, do, init)]
        out = torch.zeros(len(cs) * 48, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        handle.register_device(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), len(cs), out.data_ptr(),
                               d_init=dev[4].data_ptr(), params=cfear.params(**dict(key)), stream=stream.cuda_stream)
        stream.synchronize()
        assert out.cpu().numpy().tobytes() == want, ("device entry", key)


def test_a_workgroup_that_takes_two_jobs(handle, golden):
    """257 pairs: workgroup 0 registers drive pair 1 (about 650 records a side), then, 256 jobs later, the pair 100 m apart
    (status 4); a cell table or a descriptor left over from job 0 would show in job 256"""
    by_name = {c[0]: c for c in cases.pair_cases()}
    jobs = [by_name["drive pair 1"]] + [by_name["room moved"]] * (MAX_JOINT_BLOCKS - 1) + [by_name["100 m apart"]]
    assert len(jobs) == MAX_JOINT_BLOCKS + 1 and len(jobs[0][1]) > 500 and len(jobs[1][1]) == 54
    init = np.array([c[3] if c[3] is not None else (0.0, 0.0, 0.0) for c in jobs])
    got = handle.register([c[1] for c in jobs], [c[2] for c in jobs], init)
    alone = {n: handle.register([by_name[n][1]], [by_name[n][2]], init[i:i + 1]) for n, i in (("drive pair 1", 0), ("room moved", 1), ("100 m apart", 256))}
    for i, (c, g) in enumerate(zip(jobs, got)):
        assert g.tobytes() == alone[c[0]].tobytes(), (i, c[0], g, alone[c[0]])
    assert [int(got[i]["status"]) for i in (0, 1, 256)] == [0, 0, 4]
    # ... which are the parent's bytes as well (the default-parameter group of the golden file)
    key, cs, _ = cases.pair_groups()[0]
    assert key == ()
    want = {c[0]: golden["results_0"][48 * i:48 * (i + 1)].tobytes() for i, c in enumerate(cs)}
    for n, a in alone.items():
        assert a.tobytes() == want[n], n
