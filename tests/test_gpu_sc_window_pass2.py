"""Pass 2 of the window kernel (csrc/sc_window.hip): which list positions behind the head get a record, and what the records
say.  The kernel keeps the list's {bound, slot} records in LDS from its prologue on, takes the head's k-th smallest upper
bound with the ranking shared by its four waves, and runs the lean epilogue of sc_window_dev.h; none of that may change a
record: every case compares with the oracle's exhaustive top-k AND with the exact-all path (filter off), bit for bit, and
checks every preview against the oracle's pair function by the rule of test_gpu_sc_window.py.

* Exact control of n2 (the number of positions pass 2 admits): descriptors of 60 identical columns, each entry and each query
  with its own 20-vector.  Every shift of such a pair is the same pair, so no alignment is unique (k* = -1), the head yields no
  upper bound (tau_ub = +inf) and pass 2 admits every position up to min(sl_cnt, 320): databases of 128 + m entries give
  n2 = min(m, 192) -- groups of 1, 31, a full one, one past a full one, two to six groups, and the WINDOW_P clamp.
* Unique alignments in pass 2: the interleaved families of test_gpu_sc_window_prologue.py (400 entries), and a database of two
  clusters of near-duplicates (in the manner of test_gpu_sc_select_head.py) of 300 and 140 entries: a rotated copy of the first
  base admits all 192 positions behind the head, one of the second about a dozen, all with k* >= 0.
* Callers: every entry that launches the window kernel, with eligibility limits that cut the head and the tail."""
import importlib.util
import os

import numpy as np
import pytest

from navtech_radar_slam_amd import synth

pytestmark = pytest.mark.gpu

FORCE, OFF = 2, 1
K = 10
NQ = 64
HEAD, P = 128, 320


@pytest.fixture(scope="module")
def sc():
    from navtech_radar_slam_amd import _rsx, scancontext
    assert _rsx.device_count() >= 1, "no HIP device: GPU tests must run on the MI355X box"
    assert scancontext.WINDOW_P == P
    return scancontext


def _load(name):
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), name)
    spec = importlib.util.spec_from_file_location(name[:-3] + "_shared", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def preview_rule():
    """check_previews of test_gpu_sc_window.py: every record against the oracle's pair function"""
    return _load("test_gpu_sc_window.py").check_previews


def hits(sc, tensor, nq):
    return tensor.cpu().numpy().view(sc.HIT_DTYPE).reshape(nq, K)


class Case:
    """a database on a filtered and an exact-all handle, the oracle beside them; oracle records computed once per limit"""

    def __init__(self, sc, oracle, descs, queries):
        self.sc, self.n = sc, len(descs)
        self.descs = np.ascontiguousarray(descs, dtype=np.float32)
        self.queries = np.ascontiguousarray(queries, dtype=np.float32)
        self.f = sc.SCManager(filter_mode=FORCE)
        self.x = sc.SCManager(filter_mode=OFF)
        self.f.add_descriptors_f32(self.descs)
        self.x.add_descriptors_f32(self.descs)
        self.o = oracle.Manager()
        self.o.add_descriptors(self.descs.astype(np.float64))
        self._want = {}

    def want(self, n_elig=-1):
        if n_elig not in self._want:
            ne = self.n if n_elig < 0 else n_elig
            w = self.o.exhaustive_batch(self.queries.astype(np.float64), n_eligible=ne, k=K, nthreads=8)
            w.setflags(write=False)
            self._want[n_elig] = w
        return self._want[n_elig]

    def n2(self, nq):
        """positions behind the head with a record, per query, from the kernel's own records"""
        slots, pv, ks, sm, cnt = self.f.window_previews(self.queries[:nq], k=K)
        pos = np.arange(P)[None, :]
        rec = (pos >= HEAD) & (pos < np.asarray(cnt)[:, None]) & (np.asarray(ks) != -2)
        unique = rec & (np.asarray(ks) >= 0)
        return rec.sum(axis=1), unique.sum(axis=1), np.asarray(cnt)

    def close(self):
        self.f.close()
        self.x.close()


# ---------------------------------------------------------------------------------------------------------------------------
# exact control of n2
# ---------------------------------------------------------------------------------------------------------------------------
def constant_columns(seed, n):
    """n descriptors of 60 identical columns: one positive 20-vector each, no two alike"""
    v = np.random.default_rng(seed).uniform(0.05, 1.0, (n, 1, 20)).astype(np.float32)
    return np.ascontiguousarray(np.broadcast_to(v, (n, 60, 20)).reshape(n, 1200))


@pytest.fixture(scope="module", params=[1, 31, 32, 33, 64, 65, 191, 192, 250])
def flat_case(request, sc, oracle):
    m = request.param
    c = Case(sc, oracle, constant_columns(1000 + m, HEAD + m), constant_columns(2000 + m, NQ))
    c.m = m
    yield c
    c.close()


@pytest.mark.parametrize("nq", [1, 3, 64])
def test_every_position_behind_the_head_is_admitted(sc, oracle, flat_case, preview_rule, nq):
    c = flat_case
    n2, unique, cnt = c.n2(nq)
    assert np.all(cnt == min(c.n, P)), cnt
    assert np.all(n2 == min(c.m, P - HEAD)), (c.m, n2)
    assert np.all(unique == 0)  # declined alignments throughout
    preview_rule(sc, oracle, c.descs, c.queries[:nq], 0.0, k=K)
    want = c.want()[:nq]
    assert np.array_equal(c.f.query(c.queries[:nq], k=K), want)
    assert np.array_equal(c.x.query(c.queries[:nq], k=K), want)


# ---------------------------------------------------------------------------------------------------------------------------
# unique alignments in pass 2
# ---------------------------------------------------------------------------------------------------------------------------
def near_duplicates(seed, n, base, max_drop=3):
    """n rotated copies of `base`, each with 0..max_drop of its occupied cells set to zero (as test_gpu_sc_select_head.py)"""
    rng = np.random.default_rng(seed)
    occ = np.flatnonzero(base)
    out = np.empty((n, 1200), dtype=np.float32)
    for i in range(n):
        d = base.copy()
        d[rng.choice(occ, int(rng.integers(0, max_drop + 1)), replace=False)] = 0
        out[i] = synth.rotate_descriptor(d, int(rng.integers(0, 60)))
    return out


@pytest.fixture(scope="module")
def dup_case(sc, oracle):
    bases = synth.random_descriptors(80, 2, binary=False, fill=0.6)
    rand = synth.random_descriptors(81, 60 + NQ, binary=False)
    db = np.concatenate([rand[:30], near_duplicates(82, 300, bases[0]), near_duplicates(83, 140, bases[1]), rand[30:60]])
    db = db[np.random.default_rng(84).permutation(len(db))]
    rng = np.random.default_rng(85)
    queries = rand[60:].copy()
    for i in range(0, NQ, 2):   # even: the large cluster (pass 2 full), every fourth: the small one (a dozen positions)
        queries[i] = synth.rotate_descriptor(bases[(i // 2) % 2], int(rng.integers(0, 60)))
    queries[5] = 0
    queries[7, 100] = np.nan
    c = Case(sc, oracle, db, queries)
    yield c
    c.close()


@pytest.fixture(scope="module")
def family_case(sc, oracle):
    descs, queries = _load("test_gpu_sc_window_prologue.py").make_case(oracle, 400)
    c = Case(sc, oracle, descs, queries)
    yield c
    c.close()


@pytest.mark.parametrize("nq", [3, 64])
def test_unique_alignments_in_pass_2(sc, oracle, dup_case, family_case, preview_rule, nq):
    n2_all, uniq_all = [], []
    for c in (dup_case, family_case):
        n2, unique, _ = c.n2(nq)
        print("n2 per query:", n2.tolist(), "with k* >= 0:", unique.tolist())
        n2_all += n2.tolist()
        uniq_all += unique.tolist()
        preview_rule(sc, oracle, c.descs, c.queries[:nq], 0.0, k=K)
        want = c.want()[:nq]
        assert np.array_equal(c.f.query(c.queries[:nq], k=K), want)
        assert np.array_equal(c.x.query(c.queries[:nq], k=K), want)
    assert any(v >= 33 for v in n2_all) and any(1 <= v <= 31 for v in n2_all), n2_all
    assert max(uniq_all) >= 33, uniq_all  # more than one group of positions with a unique alignment


# ---------------------------------------------------------------------------------------------------------------------------
# every caller of launch_window, with limits that cut the head (100 < 128) and the tail (128 < 200 < 320)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["flat", "dup"])
def caller_case(request, sc, oracle, dup_case):
    if request.param == "dup":
        yield dup_case
        return
    c = Case(sc, oracle, constant_columns(3000, HEAD + 250), constant_columns(3001, NQ))
    yield c
    c.close()


@pytest.mark.parametrize("n_elig", [-1, 200, 100])
@pytest.mark.parametrize("nq", [3, 64])
def test_device_entry_and_host_entry(sc, caller_case, nq, n_elig):
    import torch
    c = caller_case
    want = c.want(n_elig)[:nq]
    dq = torch.from_numpy(c.queries[:nq]).cuda()
    st = torch.cuda.current_stream().cuda_stream
    for m in (c.f, c.x):
        got = torch.zeros((nq, K, 2), dtype=torch.float64, device="cuda")
        m.query_device(dq.data_ptr(), nq, K, got.data_ptr(), n_eligible=n_elig, stream=st)
        torch.cuda.synchronize()
        assert np.array_equal(hits(sc, got, nq), want)
    assert np.array_equal(c.f.query(c.queries[:nq], k=K, n_eligible=n_elig), want)


def test_host_buffer_entry_in_pieces(sc, caller_case):
    c = caller_case
    reps = 2049 // NQ + 1
    q = np.tile(c.queries, (reps, 1))[:2049]
    assert np.array_equal(c.f.query(q, k=K), np.tile(c.want(), (reps, 1))[:2049])


def test_self_queries(sc, caller_case):
    """entries 300 .. 377 as queries against everything older than 6 entries before them: lists of 294 .. 371 positions"""
    import torch
    c = caller_case
    first, count, excl = 300, 78, 6
    st = torch.cuda.current_stream().cuda_stream
    got = torch.zeros((count, K, 2), dtype=torch.float64, device="cuda")
    ref = torch.zeros((count, K, 2), dtype=torch.float64, device="cuda")
    c.f.query_self_device(first, count, K, got.data_ptr(), exclude_recent=excl, stream=st)
    c.x.query_self_device(first, count, K, ref.data_ptr(), exclude_recent=excl, stream=st)
    torch.cuda.synchronize()
    got, ref = hits(sc, got, count), hits(sc, ref, count)
    for i in range(count):
        want = c.o.exhaustive(c.descs[first + i].astype(np.float64), n_eligible=first + i - excl, k=K, nthreads=4)
        assert np.array_equal(got[i], want), f"filtered, query {first + i}"
        assert np.array_equal(ref[i], want), f"exact-all, query {first + i}"


@pytest.mark.parametrize("n_elig", [-1, 200, 100])
def test_two_stages_and_bounds_path_at_world_1(sc, caller_case, n_elig):
    import torch
    c, nq = caller_case, NQ
    want = c.want(n_elig)
    s = sc.SCManager(shard_rank=0, shard_world=1, filter_mode=FORCE)
    s.add_descriptors_f32(c.descs)
    ld = (c.n + 31) // 32 * 32
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    try:
        st = stream.cuda_stream
        dq = torch.from_numpy(c.queries).cuda()
        part = torch.zeros((1, nq, K, 2), dtype=torch.float64, device="cuda")
        glob = torch.zeros((nq, K, 2), dtype=torch.float64, device="cuda")
        out = torch.zeros((nq, K, 2), dtype=torch.float64, device="cuda")
        s.query_stage1_device(dq.data_ptr(), nq, K, part[0].data_ptr(), n_eligible=n_elig, stream=st)
        s.merge_device(part.data_ptr(), 1, nq, K, glob.data_ptr(), stream=st)
        s.query_stage2_device(nq, K, glob.data_ptr(), out.data_ptr(), stream=st)
        block = torch.full((1, nq, ld), float("nan"), dtype=torch.float16, device="cuda")
        got = torch.zeros((nq, K, 2), dtype=torch.float64, device="cuda")
        c.f.filter_range_device(dq.data_ptr(), nq, 0, c.n, block[0].data_ptr(), ld, stream=st)
        c.f.query_bounds_device(dq.data_ptr(), nq, K, got.data_ptr(), block.data_ptr(), 1, ld, nq * ld, n_eligible=n_elig, stream=st)
        torch.cuda.synchronize()
    finally:
        torch.cuda.set_stream(torch.cuda.default_stream())
        two, bounds = hits(sc, out, nq), hits(sc, got, nq)
        s.close()
    assert np.array_equal(two, want)
    assert np.array_equal(bounds, want)
