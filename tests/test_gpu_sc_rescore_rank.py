"""The order in which sc_rescore_wave_kernel (csrc/sc_kernels.hip) evaluates the survivors of a round: every survivor lane
ranks itself once under (lo, lane), smallest first, and the wave walks the ranks.  The order is the one a repeated wave-wide
minimum gave before, so no record and no counter may move: every case compares the hits with the oracle's exhaustive top-k
AND with the exact-all path (filter off), bit for bit, and two fixed-seed fixtures hold rsx_sc_rescoring_stats to what the
build before the ranking counted (tests/golden/sc_rescore_rank_stats.npz, tools/make_rescore_rank_golden.py).  The cases are
the ones a ranking can get wrong: equal lower bounds (the lane breaks the tie), more than 64 survivors (a second round of
ranks), lower bounds of -inf (NaN previews rank first), fewer survivors than k, a position range that cuts the list (stage 2
of a shard), and the callers with per-query limits and host buffers.  Databases of 200-400 entries, batches of 1, 3, 5, 64."""
import os

import numpy as np
import pytest

from navtech_radar_slam_amd import synth

pytestmark = pytest.mark.gpu

FORCE, OFF = 2, 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sc_rescore_rank_stats.npz")
STAT_FIELDS = ("candidates", "exact_evals", "queries_rescored", "window_previews", "valu_previews", "exact_window_shifts",
               "tail_evals", "tail_queries")


@pytest.fixture(scope="module")
def sc():
    from navtech_radar_slam_amd import _rsx, scancontext
    assert _rsx.device_count() >= 1, "no HIP device: GPU tests must run on the MI355X box"
    return scancontext


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

    def check(self, queries, k, n_elig, want=None):
        if want is None:
            want = self.want(queries, k, n_elig)
        got = self.f.query(queries, k=k, n_eligible=n_elig)
        assert self.f.profiled_kernel_name() != "sc_pair_kernel"
        assert np.array_equal(got, want), "filtered path against the oracle"
        assert np.array_equal(self.x.query(queries, k=k, n_eligible=n_elig), want), "exact-all path against the oracle"
        return want

    def close(self):
        self.f.close()
        self.x.close()


def noisy_copy(rng, desc, shift, n_zero):
    q = synth.rotate_descriptor(desc, shift)
    q[rng.integers(0, 1200, n_zero)] = 0
    return q


# ---- equal lower bounds ----

def tie_db():
    """200 entries: 15 exact copies of entry 3 (equal previews, so equal lo: the lane decides), 20 rotated copies of it
    (equal exact distances under other alignments) and 12 copies of entry 150"""
    descs = synth.random_descriptors(81, 200, binary=False)
    descs[10:40:2] = descs[3]
    for j, i in enumerate(range(50, 70)):
        descs[i] = synth.rotate_descriptor(descs[3], 3 * j + 1)
    descs[100:124:2] = descs[150]
    return descs


@pytest.fixture(scope="module")
def ties(sc, oracle):
    descs = tie_db()
    rng = np.random.default_rng(82)
    heads = [descs[3], synth.rotate_descriptor(descs[3], 13), noisy_copy(rng, descs[3], 41, 30), descs[150],
             noisy_copy(rng, descs[150], 7, 60)]
    rest = [noisy_copy(rng, descs[int(rng.integers(0, 200))], int(rng.integers(0, 60)), 40) for _ in range(59)]
    queries = np.stack(heads + rest)
    t = Trio(sc, oracle, descs)
    wants = {(k, ne): t.want(queries, k, ne) for k in (1, 10) for ne in (-1, 33)}
    yield t, queries, wants
    t.close()


@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("nq", [1, 3, 5, 64])
def test_equal_lower_bounds(ties, nq, k):
    """several copies of one scan: survivors with the same lo, evaluated in lane order; among equal distances the smaller index
    wins, which the oracle's records state"""
    t, queries, wants = ties
    want = t.check(queries[:nq], k, -1, wants[(k, -1)][:nq])
    if k == 10:
        assert np.all(want["dist"][0] == want["dist"][0, 0]), "the fixture has no ten-fold tie at the top"
        assert np.array_equal(want["index"][0], np.sort(want["index"][0]))


@pytest.mark.parametrize("k", [1, 10])
def test_too_few_survivors(ties, k):
    """33 eligible entries of which a query may reach fewer than k by its bound; 3 eligible entries: fewer records than k, so
    no k-th upper bound exists and the list is everything there is"""
    t, queries, wants = ties
    t.check(queries[:5], k, 33, wants[(k, 33)][:5])
    want = t.check(queries[:3], k, 3)
    if k == 10:
        assert np.all(want["dist"][:, 3:] == 1e7)
    want = t.check(queries[:64], k, 7)
    if k == 10:
        assert np.all(want["dist"][:, 7:] == 1e7)


# ---- more than 64 survivors ----

@pytest.mark.parametrize("k", [1, 10])
def test_second_round_of_ranks(sc, oracle, k):
    """110 exact copies of one descriptor among 300 entries: all of them tie for the best distance, none can be excluded, and
    the wave ranks and walks a second round of 64 survivors; a rotated and a damaged copy of it as further queries"""
    n = 300
    descs = synth.random_descriptors(91, n, binary=False)
    copies = np.arange(20, 240, 2)
    descs[copies] = descs[7]
    rng = np.random.default_rng(92)
    queries = np.stack([descs[7], synth.rotate_descriptor(descs[7], 29), noisy_copy(rng, descs[7], 5, 25)])
    t = Trio(sc, oracle, descs)
    try:
        dist, _ = t.o.pair_distances(queries[0].astype(np.float64), nthreads=4)
        want = t.check(queries, k, n)
        kth = want["dist"][0, k - 1]
        assert n <= sc.WINDOW_P and int(np.sum(dist[:n] <= kth)) > 64, int(np.sum(dist[:n] <= kth))
        assert np.array_equal(want["index"][0], np.sort(np.concatenate([[7], copies]))[:k])   # ties: ascending index
        t.check(queries[:1], k, n, want[:1])
    finally:
        t.close()


# ---- declined alignments, NaN previews ----

def bad_data_db():
    """magnitudes over six decades, mixed signs, single-ring descriptors, sector keys of 1e+-30, NaN / inf, and descriptors
    that repeat every 20 sectors: their sector keys match at three shifts exactly, so the window kernel declines the alignment"""
    rng = np.random.default_rng(23)
    n = 300
    base = synth.random_descriptors(50, n, binary=False).reshape(n, 60, 20)
    d = (base * 10.0 ** rng.uniform(-3, 3, (n, 60, 20))).astype(np.float32)
    d[0:60] *= np.where(rng.uniform(size=(60, 60, 20)) < 0.5, -1.0, 1.0).astype(np.float32)
    d[60:100, :, 1:] = 0
    d[100:120] *= np.float32(1e30)
    d[120:140] *= np.float32(1e-30)
    d[140] = np.nan
    d[141, 3, 4] = np.inf
    d[142, 17, 2] = np.nan
    d[143, 40, 19] = np.nan
    period = base[200, :20].copy()
    for j, i in enumerate(range(200, 224)):   # periodic in the sectors, rotated, a little noise that keeps the period
        p = period * (1.0 + 0.01 * j * rng.uniform(-1, 1, period.shape)).astype(np.float32)
        d[i] = np.roll(np.tile(p, (3, 1)), j, axis=0)
    return np.ascontiguousarray(d.reshape(n, 1200))


def test_nan_previews_rank_first(sc, oracle):
    """a NaN preview is listed with lo = -inf and k* = -1: it ranks in front of every finite bound (several of them: in lane
    order) and gets the exact alignment; a declined alignment has a finite lo and k* = -1"""
    descs = bad_data_db()
    queries = np.stack([descs[5], synth.rotate_descriptor(descs[70], 17), descs[110], descs[130], descs[141],
                        synth.rotate_descriptor(descs[40], 59), descs[200], synth.rotate_descriptor(descs[211], 7)])
    k = 10
    t = Trio(sc, oracle, descs)
    try:
        want = t.check(queries, k, -1)
        slots, pv, ks, sm, cnt = t.f.window_previews(queries, k=k)
        declined = nan_prev = 0
        for qi in range(len(queries)):
            best = set(int(h["index"]) for h in want[qi] if h["dist"] < 1e7)
            for i in range(int(cnt[qi])):
                declined += int(ks[qi, i]) == -1 and not np.isnan(pv[qi, i]) and int(slots[qi, i]) in best
                nan_prev += int(ks[qi, i]) != -2 and bool(np.isnan(pv[qi, i]))
        assert declined >= 1 and nan_prev >= 2 * len(queries), (declined, nan_prev)
        for nq in (1, 3, 5):
            t.check(queries[:nq], 1, -1, want[:nq, :1])
    finally:
        t.close()


# ---- position ranges, other callers ----

def hits(sc, tensor, nq, k):
    return tensor.cpu().numpy().view(sc.HIT_DTYPE).reshape(nq, k)


@pytest.mark.parametrize("nq", [5, 64])
def test_position_range_cuts_the_list(sc, ties, nq):
    """the two stages of one shard at world 1: stage 1 walks the first rounds of the list, stage 2 starts at round_begin > 0
    with the stage-1 hits as seed and the merged k-th distance as bound (tau_src) -- the survivors outside [i0, pw) are not
    ranked in either launch"""
    import torch
    t, queries, wants = ties
    k, n_el = 10, 190
    q = queries[:nq]
    want = t.want(q, k, n_el)
    s = sc.SCManager(shard_rank=0, shard_world=1, filter_mode=FORCE)
    s.add_descriptors_f32(t.descs)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    try:
        st = stream.cuda_stream
        dq = torch.from_numpy(q).cuda()
        part = torch.zeros((1, nq, k, 2), dtype=torch.float64, device="cuda")
        glob = torch.zeros((nq, k, 2), dtype=torch.float64, device="cuda")
        out = torch.zeros((nq, k, 2), dtype=torch.float64, device="cuda")
        s.query_stage1_device(dq.data_ptr(), nq, k, part[0].data_ptr(), n_eligible=n_el, stream=st)
        s.merge_device(part.data_ptr(), 1, nq, k, glob.data_ptr(), stream=st)
        s.query_stage2_device(nq, k, glob.data_ptr(), out.data_ptr(), stream=st)
        torch.cuda.synchronize()
    finally:
        torch.cuda.set_stream(torch.cuda.default_stream())
        s_hits = hits(sc, out, nq, k)
        s.close()
    assert np.array_equal(s_hits, want)
    assert np.array_equal(t.x.query(q, k=k, n_eligible=n_el), want)


def test_self_queries_with_per_query_limits(sc, ties):
    """query_self_device: query i sees entries [0, i - exclude_recent) -- lists of every length from 0 up in one launch, the
    copies of entry 3 among them"""
    import torch
    t, _, _ = ties
    n, k, excl = 200, 10, 5
    st = torch.cuda.current_stream().cuda_stream
    got = torch.zeros((n, k, 2), dtype=torch.float64, device="cuda")
    ref = torch.zeros((n, k, 2), dtype=torch.float64, device="cuda")
    t.f.query_self_device(0, n, k, got.data_ptr(), exclude_recent=excl, stream=st)
    t.x.query_self_device(0, n, k, ref.data_ptr(), exclude_recent=excl, stream=st)
    torch.cuda.synchronize()
    got, ref = hits(sc, got, n, k), hits(sc, ref, n, k)
    assert np.array_equal(got, ref)
    for i in (0, 5, 6, 12, 38, 69, 122, 199):
        want = t.o.exhaustive(t.descs[i].astype(np.float64), n_eligible=max(0, i - excl), k=k, nthreads=4)
        assert np.array_equal(got[i], want), f"query {i}"


def test_device_and_host_buffer_entries_agree(sc, ties):
    """the host-buffer entry (rsx_sc_query) and the device entry (rsx_sc_query_device) run the same re-scoring launch"""
    import torch
    t, queries, wants = ties
    nq, k = 64, 10
    want = wants[(k, -1)]
    assert np.array_equal(t.f.query(queries, k=k), want)
    dq = torch.from_numpy(queries).cuda()
    out = torch.zeros((nq, k, 2), dtype=torch.float64, device="cuda")
    t.f.query_device(dq.data_ptr(), nq, k, out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(hits(sc, out, nq, k), want)


# ---- the counters ----

def pin_fixture(which):
    """-> (descs, queries, k, n_eligible).  No two entries are copies of each other: with equal lower bounds the order of the
    evaluations follows the order of the short list inside a bin, which the selection does not fix from run to run."""
    if which == 0:
        descs = synth.random_descriptors(101, 400, binary=False)
        rng = np.random.default_rng(102)
        queries = np.stack([noisy_copy(rng, descs[int(rng.integers(0, 64))], int(rng.integers(0, 60)), 20 * (i + 1)) for i in range(5)])
        return descs, queries, 10, 64   # 64 eligible entries: at most 64 records, so at most 64 survivors, whatever the bounds
    descs = synth.random_descriptors(111, 200, binary=True)
    rng = np.random.default_rng(112)
    queries = np.stack([noisy_copy(rng, descs[int(rng.integers(0, 200))], int(rng.integers(0, 60)), int(rng.integers(0, 200)))
                        for _ in range(64)])
    return descs, queries, 5, 180


def rescoring_stats(manager, queries, k, n_elig):
    """rsx_sc_rescoring_stats of the whole batch and of every query on its own: int64 [1 + nq][8], rows in STAT_FIELDS order"""
    manager.profile_enable(True)
    rows = []
    try:
        for q in [queries] + [queries[i:i + 1] for i in range(len(queries))]:
            manager.profile_read_rescoring_tail()
            manager.query(q, k=k, n_eligible=n_elig)
            rows.append(manager.profile_read_rescoring_tail())
    finally:
        manager.profile_enable(False)
    return np.array(rows, dtype=np.int64)


@pytest.mark.parametrize("which", [0, 1])
def test_counters_are_what_the_unranked_kernel_counted(sc, which):
    """candidates >= the survivors of a query (the header's n_cand counts what the window kernel's bound admits before the
    preview's own lower bound is applied), so a query alone with candidates <= 64 had one round of at most 64 survivors"""
    descs, queries, k, n_elig = pin_fixture(which)
    gold = np.load(GOLDEN)["stats_%d" % which]
    m = sc.SCManager(filter_mode=FORCE)
    try:
        m.add_descriptors_f32(descs)
        got = rescoring_stats(m, queries, k, n_elig)
    finally:
        m.close()
    assert got.shape == gold.shape == (1 + len(queries), len(STAT_FIELDS))
    one_round = gold[1:, 0] <= 64
    assert one_round.sum() >= len(queries) // 2, "the fixture no longer has queries with at most 64 survivors"
    for j, name in enumerate(STAT_FIELDS):
        print(name, "batch", got[0, j], gold[0, j])
        assert np.array_equal(got[1:, j][one_round], gold[1:, j][one_round]), name
        if one_round.all():
            assert got[0, j] == gold[0, j], name
