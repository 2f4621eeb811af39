"""The hand-over between the window kernel and the re-scoring wave (csrc/sc_window.hip -> csrc/sc_kernels.hip): the window
kernel computes the bound tau_ub_w (the k-th smallest preview upper bound over all its records of a query) and writes, per
query, a header and the dense list of the positions that can still reach the top-k; the re-scoring wave trusts that bound and
evaluates only what is listed.  Nothing of this may change a record: every case compares with the oracle's exhaustive top-k
AND with the exact-all path (filter off), bit for bit, at the smallest shapes at which each path of the two kernels exists --
lists shorter than the head (the window kernel's early return still writes a list), lists that reach pass 2, lists longer
than the records, empty lists, more than 64 survivors (a second round of the wave), alignments the window kernel declines,
non-finite data, and every caller of the two launches."""
import numpy as np
import pytest

from navtech_radar_slam_amd import synth

pytestmark = pytest.mark.gpu

FORCE, OFF = 2, 1


@pytest.fixture(scope="module")
def sc():
    from navtech_radar_slam_amd import _rsx, scancontext
    assert _rsx.device_count() >= 1, "no HIP device: GPU tests must run on the MI355X box"
    return scancontext


def make_db(seed, n):
    descs = synth.random_descriptors(seed, n, binary=False)
    rng = np.random.default_rng(seed + 1)
    for i in range(0, n, 7):  # rotated (and partly corrupted) copies: near-zero distances and exact ties
        j = int(rng.integers(0, n))
        descs[i] = synth.rotate_descriptor(descs[j], int(rng.integers(0, 60)))
        if i % 3 == 0:
            descs[i][rng.integers(0, 1200, 50)] = 0
    descs[5] = 0
    descs[6][20 * 7:20 * 9] = 0
    return descs


class Trio:
    """one database behind the filtered path, the exact-all path and the oracle"""

    def __init__(self, sc, oracle, descs):
        self.sc, self.descs = sc, descs
        self.f = sc.SCManager(filter_mode=FORCE)
        self.x = sc.SCManager(filter_mode=OFF)
        self.f.add_descriptors_f32(descs)
        self.x.add_descriptors_f32(descs)
        self.o = oracle.Manager()
        self.o.add_descriptors(descs.astype(np.float64))

    def want(self, queries, k, n_elig):
        ne = len(self.descs) if n_elig < 0 else n_elig
        return np.stack([self.o.exhaustive(q.astype(np.float64), n_eligible=ne, k=k, nthreads=4) for q in queries])

    def check(self, queries, k, n_elig):
        want = self.want(queries, k, n_elig)
        got = self.f.query(queries, k=k, n_eligible=n_elig)
        assert n_elig == 0 or self.f.profiled_kernel_name() != "sc_pair_kernel"   # (nothing eligible: nothing to filter)
        assert np.array_equal(got, want), "filtered path against the oracle"
        assert np.array_equal(self.x.query(queries, k=k, n_eligible=n_elig), want), "exact-all path against the oracle"
        return want

    def close(self):
        self.f.close()
        self.x.close()


@pytest.fixture(scope="module")
def edges(sc, oracle):
    n = 730
    descs = make_db(41, n)
    rng = np.random.default_rng(42)
    queries = np.stack([synth.rotate_descriptor(descs[int(rng.integers(0, 90))], int(rng.integers(0, 60))) for _ in range(9)])
    queries[::2, rng.integers(0, 1200, 40)] = 0
    queries[3] = descs[6]
    t = Trio(sc, oracle, descs)
    yield t, queries
    t.close()


@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("n_elig", [100, 200, 700, 3, 0])
def test_list_length_edges(edges, n_elig, k):
    """eligible entries = length of the short list here (every bound fits): 100 < WINDOW_HEAD (the window kernel returns early
    and must still leave a list), 128 < 200 < WINDOW_P (pass 2), 700 > WINDOW_P (the records end, the walk behind them goes
    on), 3 < k, and 0 (headers of empty lists); 1, 5 and 9 queries: no multiple of the four queries a launch group takes"""
    t, queries = edges
    for nq in (1, 5, 9):
        want = t.check(queries[:nq], k, n_elig)
        if n_elig == 0:
            assert np.all(want["dist"] == 1e7)
        if n_elig == 3 and k == 10:
            assert np.all(want["dist"][:, 3:] == 1e7)


@pytest.mark.parametrize("k", [1, 10])
def test_more_than_64_survivors(sc, oracle, k):
    """110 exact copies of one descriptor among 300 entries: all of them tie for the best distance, so all of them lie at or
    below the k-th best and none can be excluded -- the wave's second round of 64 survivors runs (all 300 have records)"""
    n = 300
    descs = synth.random_descriptors(51, n, binary=False)
    copies = np.arange(20, 240, 2)
    assert len(copies) == 110
    descs[copies] = descs[7]
    query = descs[7][None].copy()
    t = Trio(sc, oracle, descs)
    try:
        dist, _ = t.o.pair_distances(query[0].astype(np.float64), nthreads=4)
        want = t.check(query, k, n)
        kth = want["dist"][0, k - 1]
        assert n <= sc.WINDOW_P and int(np.sum(dist[:n] <= kth)) > 64, int(np.sum(dist[:n] <= kth))
        assert np.array_equal(want["index"][0], np.sort(np.concatenate([[7], copies]))[:k])   # ties: ascending index
    finally:
        t.close()


def adversarial_db():
    """the adversarial family of test_gpu_sc_window.py (magnitudes over six decades, mixed signs, single-ring and mostly-empty
    descriptors, sector keys of 1e+-30, NaN / inf) plus descriptors that repeat every 20 sectors: their sector keys match at
    three shifts exactly, so the window kernel must decline the alignment (k* = -1)"""
    rng = np.random.default_rng(23)
    n = 640
    base = synth.random_descriptors(50, n, binary=False).reshape(n, 60, 20)
    d = (base * 10.0 ** rng.uniform(-3, 3, (n, 60, 20))).astype(np.float32)
    d[100:200] *= np.where(rng.uniform(size=(100, 60, 20)) < 0.5, -1.0, 1.0).astype(np.float32)
    d[200:260, :, 1:] = 0
    d[260:320][rng.uniform(size=(60, 60)) < 0.8] = 0
    d[320:340] *= np.float32(1e30)
    d[340:360] *= np.float32(1e-30)
    d[360] = np.nan
    d[361, 3, 4] = np.inf
    period = base[400, :20].copy()
    for j, i in enumerate(range(400, 424)):   # periodic in the sectors, rotated, a little noise that keeps the period
        p = period * (1.0 + 0.01 * j * rng.uniform(-1, 1, period.shape)).astype(np.float32)
        d[i] = np.roll(np.tile(p, (3, 1)), j, axis=0)
    return np.ascontiguousarray(d.reshape(n, 1200))


def test_declined_alignments_and_bad_data(sc, oracle):
    descs = adversarial_db()
    queries = np.stack([descs[5], synth.rotate_descriptor(descs[150], 17), descs[230], descs[300], descs[330], descs[350],
                        synth.rotate_descriptor(descs[40], 59), descs[361], descs[400], synth.rotate_descriptor(descs[411], 7)])
    k = 10
    t = Trio(sc, oracle, descs)
    try:
        want = t.check(queries, k, -1)
        slots, pv, ks, sm, cnt = t.f.window_previews(queries, k=k)
        declined = nan_prev = 0
        for qi in range(len(queries)):
            best = set(int(h["index"]) for h in want[qi] if h["dist"] < 1e7)
            for i in range(int(cnt[qi])):
                # an entry of the final top-k is listed whatever the bounds are; a NaN preview is listed by definition
                declined += int(ks[qi, i]) == -1 and not np.isnan(pv[qi, i]) and int(slots[qi, i]) in best
                nan_prev += int(ks[qi, i]) != -2 and bool(np.isnan(pv[qi, i]))
        assert declined >= 1 and nan_prev >= 1, (declined, nan_prev)
        assert np.array_equal(t.f.query(queries, k=1), want[:, :1])
    finally:
        t.close()


@pytest.fixture(scope="module")
def callers(sc, oracle):
    n = 700
    descs = make_db(61, n)
    queries = np.stack([synth.rotate_descriptor(descs[(i * 37) % n], (7 * i) % 60) for i in range(9)])
    queries[4].reshape(60, 20)[:25] = 0
    t = Trio(sc, oracle, descs)
    yield t, queries
    t.close()


def hits(sc, tensor, nq, k):
    return tensor.cpu().numpy().view(sc.HIT_DTYPE).reshape(nq, k)


def test_self_queries_with_per_query_limits(sc, callers):
    """query_self_device: query i sees entries [0, i - exclude_recent) -- lists of every length from 0 up in one launch"""
    import torch
    t, _ = callers
    n, k, excl = 400, 10, 30
    st = torch.cuda.current_stream().cuda_stream
    got = torch.zeros((n, k, 2), dtype=torch.float64, device="cuda")
    ref = torch.zeros((n, k, 2), dtype=torch.float64, device="cuda")
    t.f.query_self_device(0, n, k, got.data_ptr(), exclude_recent=excl, stream=st)
    t.x.query_self_device(0, n, k, ref.data_ptr(), exclude_recent=excl, stream=st)
    torch.cuda.synchronize()
    got, ref = hits(sc, got, n, k), hits(sc, ref, n, k)
    assert np.array_equal(got, ref)
    for i in (0, 29, 30, 31, 40, 133, 160, 161, 399):
        want = t.o.exhaustive(t.descs[i].astype(np.float64), n_eligible=max(0, i - excl), k=k, nthreads=4)
        assert np.array_equal(got[i], want), f"query {i}"


def test_two_stages_of_one_shard(sc, callers):
    """stage 1 (the first rounds of the list), the merge, then stage 2 with the stage-1 hits as seed and the merged k-th
    distance as bound: the window kernel's bound is used by both launches"""
    import torch
    t, queries = callers
    nq, k, n_el = len(queries), 10, 670
    want = t.want(queries, k, n_el)
    s = sc.SCManager(shard_rank=0, shard_world=1, filter_mode=FORCE)
    s.add_descriptors_f32(t.descs)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    try:
        st = stream.cuda_stream
        dq = torch.from_numpy(queries).cuda()
        part = torch.zeros((1, nq, k, 2), dtype=torch.float64, device="cuda")
        glob = torch.zeros((nq, k, 2), dtype=torch.float64, device="cuda")
        out = torch.zeros((nq, k, 2), dtype=torch.float64, device="cuda")
        s.query_stage1_device(dq.data_ptr(), nq, k, part[0].data_ptr(), n_eligible=n_el, stream=st)
        s.merge_device(part.data_ptr(), 1, nq, k, glob.data_ptr(), stream=st)
        s.query_stage2_device(nq, k, glob.data_ptr(), out.data_ptr(), stream=st)
        torch.cuda.synchronize()
    finally:
        torch.cuda.set_stream(torch.cuda.default_stream())
    assert np.array_equal(hits(sc, out, nq, k), want)
    assert np.array_equal(t.x.query(queries, k=k, n_eligible=n_el), want)
    s.close()


def test_bounds_from_a_filter_shard(sc, callers):
    """the filter-shard path: the bounds come in as a column block, selection + window + re-scoring run behind them"""
    import torch
    t, queries = callers
    nq, k, n_el, n = len(queries), 10, 670, len(t.descs)
    want = t.want(queries, k, n_el)
    ld = (n + 31) // 32 * 32
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    try:
        st = stream.cuda_stream
        dq = torch.from_numpy(queries).cuda()
        block = torch.full((1, nq, ld), float("nan"), dtype=torch.float16, device="cuda")
        got = torch.zeros((nq, k, 2), dtype=torch.float64, device="cuda")
        t.f.filter_range_device(dq.data_ptr(), nq, 0, n, block[0].data_ptr(), ld, stream=st)
        t.f.query_bounds_device(dq.data_ptr(), nq, k, got.data_ptr(), block.data_ptr(), 1, ld, nq * ld, n_eligible=n_el, stream=st)
        torch.cuda.synchronize()
    finally:
        torch.cuda.set_stream(torch.cuda.default_stream())
    assert np.array_equal(hits(sc, got, nq, k), want)
    assert np.array_equal(t.x.query(queries, k=k, n_eligible=n_el), want)


def test_host_buffer_entry_in_pieces(sc, oracle, callers):
    """2049 queries from a host buffer go up in two pieces; the stages behind the filter run once over the whole batch"""
    t, queries = callers
    nq, k, n_el = 2049, 10, 330
    q = synth.random_descriptors(62, nq, binary=False)
    q[::5] = t.descs[np.arange(len(q[::5])) % n_el]
    q[:9] = queries
    want = t.o.exhaustive_batch(q.astype(np.float64), n_eligible=n_el, k=k, nthreads=8)
    assert np.array_equal(t.f.query(q, k=k, n_eligible=n_el), want)
    assert np.array_equal(t.x.query(q, k=k, n_eligible=n_el), want)
