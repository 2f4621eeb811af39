"""The window kernel builds its query images itself (csrc/sc_window.hip, the prologue of sc_window_kernel): the fp16 image of
the direct filter and the hi / lo sector-key image go from the query's descriptor, column norms and sector key straight into
LDS, where two kernels used to write them to global memory for the window kernel to copy back.  Nothing of that may change a
record: every case compares with the oracle's exhaustive top-k AND with the exact-all path (filter off), bit for bit.

Shapes: databases of 100 and 400 entries (short lists at or under the 128 positions of the head, and over them: pass 2 and the
second use of the staging area's arrays), batches of 1, 3, 5 and 64 queries (one workgroup per query; 1, 3, 5 are no multiple
of the four queries the kernels in front of it take per workgroup).  Query families: binary descriptors of a synthetic drive,
continuous ones, empty columns, an all-zero query, a NaN and an inf element, sector keys of 1e+-30 (the adversarial family of
test_gpu_sc_window.py), and nothing eligible.  Callers: every entry that launches the window kernel."""
import importlib.util
import os

import numpy as np
import pytest

from navtech_radar_slam_amd import synth

pytestmark = pytest.mark.gpu

FORCE, OFF = 2, 1
K = 10
NQ = 64


@pytest.fixture(scope="module")
def sc():
    from navtech_radar_slam_amd import _rsx, scancontext
    assert _rsx.device_count() >= 1, "no HIP device: GPU tests must run on the MI355X box"
    return scancontext


def families(oracle, seed, n):
    """n descriptors, the families interleaved (entry i: family i % 8), so that every prefix and every window of a few
    entries mixes them: 0 binary drive, 1 continuous, 2 rotated copy of an earlier entry, 3 empty columns, 4 magnitudes over
    six decades with mixed signs, 5 sector keys of 1e30, 6 sector keys of 1e-30, 7 binary random"""
    rng = np.random.default_rng(seed)
    nd = (n + 7) // 8
    pts, off, _, _, _ = synth.trajectory_keyframes(seed, nd, seed + 1, 1, binary_z=True)
    drive = np.stack([oracle.make_scancontext(pts[off[i]:off[i + 1]]) for i in range(nd)]).astype(np.float32)
    cont = synth.random_descriptors(seed + 2, n, binary=False)
    binr = synth.random_descriptors(seed + 3, n, binary=True)
    d = cont.copy()
    for i in range(n):
        f = i % 8
        if f == 0:
            d[i] = drive[i // 8]
        elif f == 2 and i > 8:
            d[i] = synth.rotate_descriptor(d[int(rng.integers(0, i))], int(rng.integers(0, 60)))
        elif f == 3:
            d[i].reshape(60, 20)[rng.uniform(size=60) < rng.uniform(0.05, 0.9)] = 0
        elif f == 4:
            d[i] = (cont[i] * 10.0 ** rng.uniform(-3, 3, 1200) * np.where(rng.uniform(size=1200) < 0.5, -1.0, 1.0)).astype(np.float32)
        elif f == 5:
            d[i] = cont[i] * np.float32(1e30)
        elif f == 6:
            d[i] = cont[i] * np.float32(1e-30)
        elif f == 7:
            d[i] = binr[i]
    return np.ascontiguousarray(d, dtype=np.float32)


def make_case(oracle, n):
    descs = families(oracle, 300 + n, n)
    descs[9] = 0                      # an all-zero entry
    descs[17, 20 * 3 + 4] = np.nan    # non-finite entries
    descs[25, 20 * 59 + 19] = np.inf
    rng = np.random.default_rng(n)
    fresh = families(oracle, 700 + n, NQ)
    queries = fresh.copy()
    for i in range(0, NQ, 2):   # every other query: a rotated database entry of the same family (near-zero distances)
        e = (8 * int(rng.integers(1, n // 8)) + i % 8) % n
        queries[i] = synth.rotate_descriptor(descs[e], int(rng.integers(0, 60)))
    queries[1].reshape(60, 20)[:59] = 0     # one column left
    queries[4] = 0                          # all-zero
    queries[7, 333] = np.nan
    queries[10, 0] = np.inf
    queries[13, 1199] = -np.inf
    queries[3] = descs[9]
    return descs, np.ascontiguousarray(queries, dtype=np.float32)


class Case:
    def __init__(self, sc, oracle, n):
        self.sc, self.n = sc, n
        self.descs, self.queries = make_case(oracle, n)
        self.f = sc.SCManager(filter_mode=FORCE)
        self.x = sc.SCManager(filter_mode=OFF)
        self.f.add_descriptors_f32(self.descs)
        self.x.add_descriptors_f32(self.descs)
        self.o = oracle.Manager()
        self.o.add_descriptors(self.descs.astype(np.float64))
        self._want = {}

    def want(self, n_elig):
        """the oracle's records of all 64 queries, computed once per eligibility limit and only read afterwards"""
        if n_elig not in self._want:
            ne = self.n if n_elig < 0 else n_elig
            w = self.o.exhaustive_batch(self.queries.astype(np.float64), n_eligible=ne, k=K, nthreads=8)
            w.setflags(write=False)
            self._want[n_elig] = w
        return self._want[n_elig]

    def close(self):
        self.f.close()
        self.x.close()


@pytest.fixture(scope="module", params=[100, 400])
def case(request, sc, oracle):
    c = Case(sc, oracle, request.param)
    yield c
    c.close()


def hits(sc, tensor, nq):
    return tensor.cpu().numpy().view(sc.HIT_DTYPE).reshape(nq, K)


@pytest.mark.parametrize("n_elig", [-1, 70, 0])
@pytest.mark.parametrize("nq", [1, 3, 5, 64])
def test_device_entry(sc, case, nq, n_elig):
    """batches of nq queries starting at every multiple of nq: every family passes through every batch size"""
    import torch
    want = case.want(n_elig)
    dq = torch.from_numpy(case.queries).cuda()
    st = torch.cuda.current_stream().cuda_stream
    for m, name in ((case.f, "filtered"), (case.x, "exact-all")):
        got = torch.zeros((NQ, K, 2), dtype=torch.float64, device="cuda")
        for s in range(0, NQ - nq + 1, nq):
            m.query_device(dq[s].data_ptr(), nq, K, got[s].data_ptr(), n_eligible=n_elig, stream=st)
        torch.cuda.synchronize()
        top = NQ // nq * nq
        assert np.array_equal(hits(sc, got, NQ)[:top], want[:top]), name
    assert n_elig == 0 or case.f.profiled_kernel_name() == "sc_spec2_filter_kernel"
    if n_elig == 0:
        assert np.all(want["dist"] == 1e7)


def test_host_buffer_entry_in_pieces(sc, case):
    """2049 queries from a host buffer go up in two pieces (2048 + 1); the window kernel runs once over the whole batch"""
    reps = 2049 // NQ + 1
    q = np.tile(case.queries, (reps, 1))[:2049]
    want = np.tile(case.want(-1), (reps, 1))[:2049]
    assert np.array_equal(case.f.query(q, k=K), want)
    assert np.array_equal(case.x.query(q[:NQ + 1], k=K), want[:NQ + 1])
    for nq in (1, 3, 5):
        assert np.array_equal(case.f.query(case.queries[:nq], k=K), case.want(-1)[:nq])
        assert np.array_equal(case.f.query(case.queries[:nq], k=K, n_eligible=0), case.want(0)[:nq])


def test_self_queries(sc, case):
    """query_self_device: entry i as a query against entries [0, i - exclude_recent): every family of the database as a query,
    lists of every length from 0 up in one launch"""
    import torch
    n, excl = case.n, 6
    st = torch.cuda.current_stream().cuda_stream
    got = torch.zeros((n, K, 2), dtype=torch.float64, device="cuda")
    ref = torch.zeros((n, K, 2), dtype=torch.float64, device="cuda")
    case.f.query_self_device(0, n, K, got.data_ptr(), exclude_recent=excl, stream=st)
    case.x.query_self_device(0, n, K, ref.data_ptr(), exclude_recent=excl, stream=st)
    torch.cuda.synchronize()
    got, ref = hits(sc, got, n), hits(sc, ref, n)
    for i in range(n):
        want = case.o.exhaustive(case.descs[i].astype(np.float64), n_eligible=max(0, i - excl), k=K, nthreads=4)
        assert np.array_equal(got[i], want), f"filtered, query {i}"
        assert np.array_equal(ref[i], want), f"exact-all, query {i}"


@pytest.mark.parametrize("nq", [1, 3, 5, 64])
def test_two_stages_at_world_1(sc, case, nq):
    import torch
    n_el = case.n - 10
    want = case.want(n_el)[:nq]
    s = sc.SCManager(shard_rank=0, shard_world=1, filter_mode=FORCE)
    s.add_descriptors_f32(case.descs)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    try:
        st = stream.cuda_stream
        dq = torch.from_numpy(case.queries[:nq]).cuda()
        part = torch.zeros((1, nq, K, 2), dtype=torch.float64, device="cuda")
        glob = torch.zeros((nq, K, 2), dtype=torch.float64, device="cuda")
        out = torch.zeros((nq, K, 2), dtype=torch.float64, device="cuda")
        s.query_stage1_device(dq.data_ptr(), nq, K, part[0].data_ptr(), n_eligible=n_el, stream=st)
        s.merge_device(part.data_ptr(), 1, nq, K, glob.data_ptr(), stream=st)
        s.query_stage2_device(nq, K, glob.data_ptr(), out.data_ptr(), stream=st)
        torch.cuda.synchronize()
    finally:
        torch.cuda.set_stream(torch.cuda.default_stream())
        got = hits(sc, out, nq)
        s.close()
    assert np.array_equal(got, want)
    assert np.array_equal(case.x.query(case.queries[:nq], k=K, n_eligible=n_el), want)


@pytest.mark.parametrize("n_elig", [-1, 0])
@pytest.mark.parametrize("nq", [1, 3, 5, 64])
def test_bounds_path(sc, case, nq, n_elig):
    """the bounds come in as a column block (the filter-shard path); selection + window + re-scoring run behind them"""
    import torch
    n = case.n
    want = case.want(n_elig)[:nq]
    ld = (n + 31) // 32 * 32
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    try:
        st = stream.cuda_stream
        dq = torch.from_numpy(case.queries[:nq]).cuda()
        block = torch.full((1, nq, ld), float("nan"), dtype=torch.float16, device="cuda")
        got = torch.zeros((nq, K, 2), dtype=torch.float64, device="cuda")
        case.f.filter_range_device(dq.data_ptr(), nq, 0, n, block[0].data_ptr(), ld, stream=st)
        case.f.query_bounds_device(dq.data_ptr(), nq, K, got.data_ptr(), block.data_ptr(), 1, ld, nq * ld, n_eligible=n_elig, stream=st)
        torch.cuda.synchronize()
    finally:
        torch.cuda.set_stream(torch.cuda.default_stream())
    assert np.array_equal(hits(sc, got, nq), want)
    assert np.array_equal(case.x.query(case.queries[:nq], k=K, n_eligible=n_elig), want)


@pytest.fixture(scope="module")
def preview_rule():
    """check_previews of test_gpu_sc_window.py: every record against the oracle's pair function"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_sc_window.py")
    spec = importlib.util.spec_from_file_location("sc_window_rule", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.check_previews


@pytest.mark.parametrize("nq", [1, 3, 5, 64])
def test_previews_entry(sc, oracle, case, preview_rule, nq):
    """rsx_sc_window_previews hands out the kernel's records themselves: every one of them against the oracle's pair function.
    (The share of pairs with a unique alignment is a property of the data, which these families are not chosen for: the
    rule's per-pair checks are what counts here, so no minimum share is asked.)"""
    served, total = preview_rule(sc, oracle, case.descs, case.queries[:nq], 0.0, k=K)
    assert total > 0
    # and the entry leaves the production path as it was: the records of the same handle afterwards
    assert np.array_equal(case.f.query(case.queries[:nq], k=K), case.want(-1)[:nq])
