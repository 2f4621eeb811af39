"""The packed form of sc_rescore_wave_kernel (csrc/sc_kernels.hip, csrc/sc_exact_dev.h PackedRegs): on a database whose
entries are all packable (column-constant, tests/test_sc_packed_columns.py) the wave reads 16-byte columns instead of the fp32
descriptor, and the sector key only where it aligns.  It must give what the generic form gives: the same records bit for bit
and the same rsx_sc_rescoring_stats field by field -- the generic form forced on a second handle over the same database
(rsx_sc_rescore_force_generic) -- and both must equal the oracle's exhaustive top-k and the exact-all path (filter off).
The fixtures are those of tests/test_gpu_sc_rescore_rank.py made packable (binary and column-constant entries), plus queries
with NaN / inf elements, declined alignments (k* = -1), per-query limits, every caller of the re-scoring launch at world 1, the
four summation orders, and the rule that picks the form.  Databases of 200-400 entries (3000 where the walk has to leave the
head of the list), batches of 1, 3, 5, 64."""
import numpy as np
import pytest

from navtech_radar_slam_amd import synth

pytestmark = pytest.mark.gpu

FORCE, OFF = 2, 1
STAT_FIELDS = ("candidates", "exact_evals", "queries_rescored", "window_previews", "valu_previews", "exact_window_shifts",
               "tail_evals", "tail_queries")


@pytest.fixture(scope="module")
def sc():
    from navtech_radar_slam_amd import _rsx, scancontext
    assert _rsx.device_count() >= 1, "no HIP device: GPU tests must run on the MI355X box"
    return scancontext


def hits(sc, tensor, nq, k):
    return tensor.cpu().numpy().view(sc.HIT_DTYPE).reshape(nq, k)


def column_values(seed, descs):
    """binary descriptors -> the same occupancy with one value per column"""
    n = len(descs)
    vals = np.random.default_rng(seed).uniform(0.5, 9.0, (n, 60, 1)).astype(np.float32)
    d = np.where(descs.reshape(n, 60, 20) != 0, vals, np.float32(0.0))
    return np.ascontiguousarray(d.reshape(n, 1200), dtype=np.float32)


def noisy_copy(rng, desc, shift, n_zero):
    q = synth.rotate_descriptor(desc, shift)
    q[rng.integers(0, 1200, n_zero)] = 0
    return q


class Forms:
    """one all-packable database behind the packed form, the generic form (forced), the exact-all path and the oracle"""

    def __init__(self, sc, oracle, descs, sum_order=0):
        self.sc, self.descs = sc, descs
        n = len(descs)
        self.p = sc.SCManager(filter_mode=FORCE, sum_order=sum_order, capacity_hint=n)
        self.g = sc.SCManager(filter_mode=FORCE, sum_order=sum_order, capacity_hint=n)
        self.x = sc.SCManager(filter_mode=OFF, sum_order=sum_order, capacity_hint=n)
        self.g.rescore_force_generic(True)
        for m in (self.p, self.g, self.x):
            m.add_descriptors_f32(descs)
        assert self.p.rescore_form() == (1, 0), "the fixture is not all packable"
        assert self.g.rescore_form() == (0, 0)
        self.o = oracle.Manager()
        self.o.add_descriptors(descs.astype(np.float64))

    def want(self, queries, k, n_elig=-1):
        ne = len(self.descs) if n_elig < 0 else n_elig
        return np.stack([self.o.exhaustive(q.astype(np.float64), n_eligible=ne, k=k, nthreads=4) for q in queries])

    def run(self, m, queries, k, n_elig):
        m.profile_enable(True)
        try:
            m.profile_read_rescoring_tail()
            got = m.query(queries, k=k, n_eligible=n_elig)
            return got, m.profile_read_rescoring_tail()
        finally:
            m.profile_enable(False)

    def check(self, queries, k, n_elig=-1, want=None, stats=True):
        """stats=False: a query of the fixture has more than 64 survivors.  A round takes 64 of them in the order of the short
        list inside a bin, which the selection does not fix from run to run, and how far tau has come down when the second round
        starts depends on who was in the first: the counters of two launches of ONE form differ there already"""
        if want is None:
            want = self.want(queries, k, n_elig)
        got_p, st_p = self.run(self.p, queries, k, n_elig)
        assert self.p.profiled_kernel_name() != "sc_pair_kernel"
        got_g, st_g = self.run(self.g, queries, k, n_elig)
        assert np.array_equal(got_p, got_g), "packed form against generic form"
        for name, a, b in zip(STAT_FIELDS, st_p, st_g):
            print(name, a, b)
            assert a == b or not stats, (name, a, b)
        assert np.array_equal(got_p, want), "packed form against the oracle"
        assert np.array_equal(self.x.query(queries, k=k, n_eligible=n_elig), want), "exact-all path against the oracle"
        assert self.p.rescore_form()[0] == 1 and self.g.rescore_form()[0] == 0
        return want, st_p

    def close(self):
        for m in (self.p, self.g, self.x):
            m.close()


# ---- equal lower bounds, too few survivors ----

def tie_db():
    """200 packable entries (one half binary, one half with a value per column): 15 exact copies of entry 3, 20 rotated copies
    of it and 12 copies of entry 150"""
    descs = synth.random_descriptors(81, 200, binary=True)
    descs[100:] = column_values(83, descs[100:])
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
    t = Forms(sc, oracle, descs)
    wants = {(k, ne): t.want(queries, k, ne) for k in (1, 10) for ne in (-1, 33)}
    yield t, queries, wants
    t.close()


@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("nq", [1, 3, 5, 64])
def test_equal_lower_bounds(ties, nq, k):
    t, queries, wants = ties
    want, _ = t.check(queries[:nq], k, -1, wants[(k, -1)][:nq])
    if k == 10:
        assert np.all(want["dist"][0] == want["dist"][0, 0]), "the fixture has no ten-fold tie at the top"
        assert np.array_equal(want["index"][0], np.sort(want["index"][0]))


@pytest.mark.parametrize("k", [1, 10])
def test_too_few_survivors(ties, k):
    t, queries, wants = ties
    t.check(queries[:5], k, 33, wants[(k, 33)][:5])
    want, _ = t.check(queries[:3], k, 3)
    if k == 10:
        assert np.all(want["dist"][:, 3:] == 1e7)
    want, _ = t.check(queries[:64], k, 7)
    if k == 10:
        assert np.all(want["dist"][:, 7:] == 1e7)


# ---- more than 64 survivors ----

@pytest.mark.parametrize("k", [1, 10])
def test_second_round_of_ranks(sc, oracle, k):
    """110 exact copies of one descriptor among 300 entries: a second round of 64 survivors, i.e. more touches behind the first
    survivor's record than the wait counter can hold apart (> 60)"""
    n = 300
    descs = column_values(93, synth.random_descriptors(91, n, binary=True))
    copies = np.arange(20, 240, 2)
    descs[copies] = descs[7]
    rng = np.random.default_rng(92)
    queries = np.stack([descs[7], synth.rotate_descriptor(descs[7], 29), noisy_copy(rng, descs[7], 5, 25)])
    t = Forms(sc, oracle, descs)
    try:
        dist, _ = t.o.pair_distances(queries[0].astype(np.float64), nthreads=4)
        want, _ = t.check(queries, k, n, stats=False)
        kth = want["dist"][0, k - 1]
        assert n <= sc.WINDOW_P and int(np.sum(dist[:n] <= kth)) > 64, int(np.sum(dist[:n] <= kth))
        assert np.array_equal(want["index"][0], np.sort(np.concatenate([[7], copies]))[:k])
        t.check(queries[:1], k, n, want[:1], stats=False)
    finally:
        t.close()


# ---- the walk behind the head of the list ----

def near_duplicates(seed, n, base, min_drop=0, max_drop=3):
    rng = np.random.default_rng(seed)
    occ = np.flatnonzero(base)
    out = np.empty((n, 1200), dtype=np.float32)
    for i in range(n):
        d = base.copy()
        d[rng.choice(occ, int(rng.integers(min_drop, max_drop + 1)), replace=False)] = 0
        out[i] = synth.rotate_descriptor(d, int(rng.integers(0, 60)))
    return out


def test_near_duplicates_walk_behind_the_head(sc, oracle):
    """the fixture of tests/test_gpu_sc_select_head.py (binary): 2400 near-duplicates of the query among 600 others put hundreds
    of bounds into the bins behind the stored head, where entries have no record: found in the row of bounds, aligned exactly
    (the packed form asks for their sector key) and scored"""
    base = synth.random_descriptors(71, 1, binary=True, fill=0.6)[0]
    rand = synth.random_descriptors(73, 600, binary=True)
    common = near_duplicates(75, 1, base, 6, 6)[0]
    dup = near_duplicates(77, 2400, common, 0, 3)
    db = np.concatenate([rand[:300], dup, rand[300:]])
    rng = np.random.default_rng(5)
    queries = np.stack([synth.rotate_descriptor(base, int(r)) for r in rng.integers(0, 60, 3)] + [db[7], np.zeros(1200, np.float32)])
    t = Forms(sc, oracle, db)
    try:
        o = t.o
        want = o.exhaustive_batch(queries.astype(np.float64), k=10, nthreads=8)
        _, st = t.check(queries, 10, -1, want, stats=False)
        assert st[6] > 0 and st[7] > 0, "the walk never left the head: this test proves nothing"
    finally:
        t.close()


# ---- non-finite queries, declined alignments, per-query limits ----

def periodic_db():
    """300 packable entries; 24 of them repeat every 20 sectors: their sector keys match at three shifts exactly, so the window
    kernel declines the alignment (k* = -1) and the wave aligns them itself"""
    n = 300
    descs = column_values(25, synth.random_descriptors(24, n, binary=True))
    d = descs.reshape(n, 60, 20)
    rng = np.random.default_rng(26)
    period = d[200, :20].copy()
    for j, i in enumerate(range(200, 224)):
        p = period.copy()
        p[rng.integers(0, 20), rng.integers(0, 20)] = 0   # damage that keeps the period
        d[i] = np.roll(np.tile(p, (3, 1)), j, axis=0)
    return np.ascontiguousarray(d.reshape(n, 1200))


@pytest.fixture(scope="module")
def periodic(sc, oracle):
    t = Forms(sc, oracle, periodic_db())
    yield t
    t.close()


def test_declined_alignments(periodic):
    t = periodic
    descs = t.descs
    queries = np.stack([descs[200], synth.rotate_descriptor(descs[211], 7), descs[5], synth.rotate_descriptor(descs[223], 31),
                        synth.rotate_descriptor(descs[70], 17)])
    k = 10
    want, st = t.check(queries, k)
    slots, pv, ks, sm, cnt = t.p.window_previews(queries, k=k)
    declined = 0
    for qi in range(len(queries)):
        best = set(int(h["index"]) for h in want[qi] if h["dist"] < 1e7)
        for i in range(int(cnt[qi])):
            declined += int(ks[qi, i]) == -1 and not np.isnan(pv[qi, i]) and int(slots[qi, i]) in best
    assert declined >= 1, "no declined alignment among the hits: the k* = -1 path was not needed"
    assert st[4] > 0, "no exact alignment was counted"
    for nq in (1, 3):
        t.check(queries[:nq], 1, -1, want[:nq, :1])


def test_non_finite_queries(periodic):
    """a NaN or an inf in the query against packable entries: the product with an empty ring's 0.0 is formed as with the full
    column (NaN), so the records stay what the oracle says"""
    t = periodic
    descs = t.descs
    q = np.stack([descs[5], descs[40], descs[100], descs[210], descs[17]]).reshape(5, 60, 20).copy()
    q[0, 3, 4] = np.inf
    q[1, 17, 2] = np.nan
    q[2] = np.nan
    q[3, 0, 0] = -np.inf
    q[4, 59, 19] = np.nan
    queries = q.reshape(5, 1200)
    t.check(queries, 10)
    t.check(queries[:1], 1)
    t.check(queries[:3], 5, 150)


def test_self_queries_with_per_query_limits(sc, ties):
    import torch
    t, _, _ = ties
    n, k, excl = 200, 10, 5
    st = torch.cuda.current_stream().cuda_stream
    outs = []
    for m in (t.p, t.g, t.x):
        out = torch.zeros((n, k, 2), dtype=torch.float64, device="cuda")
        m.query_self_device(0, n, k, out.data_ptr(), exclude_recent=excl, stream=st)
        torch.cuda.synchronize()
        outs.append(hits(sc, out, n, k))
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
    for i in (0, 5, 6, 12, 38, 69, 122, 199):
        want = t.o.exhaustive(t.descs[i].astype(np.float64), n_eligible=max(0, i - excl), k=k, nthreads=4)
        assert np.array_equal(outs[0][i], want), f"query {i}"
    assert t.p.rescore_form()[0] == 1


# ---- every caller of the re-scoring launch at world 1 ----

def test_device_and_host_buffer_entries(sc, ties):
    import torch
    t, queries, wants = ties
    nq, k = 64, 10
    want = wants[(k, -1)]
    assert np.array_equal(t.p.query(queries, k=k), want)
    dq = torch.from_numpy(queries).cuda()
    out = torch.zeros((nq, k, 2), dtype=torch.float64, device="cuda")
    t.p.query_device(dq.data_ptr(), nq, k, out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(hits(sc, out, nq, k), want)
    assert t.p.rescore_form()[0] == 1


def test_host_buffer_entry_in_pieces(sc, oracle, ties):
    """2049 queries from a host buffer go up in two pieces; the stages behind the filter run once over the whole batch"""
    t, _, _ = ties
    nq, k, n_el = 2049, 10, 190
    rng = np.random.default_rng(62)
    q = np.stack([noisy_copy(rng, t.descs[int(rng.integers(0, 200))], int(rng.integers(0, 60)), 50) for _ in range(nq)])
    got = t.p.query(q, k=k, n_eligible=n_el)
    assert np.array_equal(got, t.g.query(q, k=k, n_eligible=n_el))
    assert np.array_equal(got, t.x.query(q, k=k, n_eligible=n_el))
    for i in (0, 1, 1023, 1024, 2047, 2048):
        assert np.array_equal(got[i], t.o.exhaustive(q[i].astype(np.float64), n_eligible=n_el, k=k, nthreads=4)), i


@pytest.mark.parametrize("nq", [5, 64])
def test_both_stages_of_the_sharded_search(sc, ties, nq):
    import torch
    t, queries, wants = ties
    k, n_el = 10, 190
    q = queries[:nq]
    want = t.want(q, k, n_el)
    s = sc.SCManager(shard_rank=0, shard_world=1, filter_mode=FORCE)
    s.add_descriptors_f32(t.descs)
    assert s.rescore_form() == (1, 0)
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


def test_bounds_from_a_filter_shard(sc, ties):
    import torch
    t, queries, wants = ties
    nq, k, n_el, n = len(queries), 10, 170, len(t.descs)
    want = t.want(queries, k, n_el)
    ld = (n + 31) // 32 * 32
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    try:
        st = stream.cuda_stream
        dq = torch.from_numpy(queries).cuda()
        block = torch.full((1, nq, ld), float("nan"), dtype=torch.float16, device="cuda")
        got = torch.zeros((nq, k, 2), dtype=torch.float64, device="cuda")
        t.p.filter_range_device(dq.data_ptr(), nq, 0, n, block[0].data_ptr(), ld, stream=st)
        t.p.query_bounds_device(dq.data_ptr(), nq, k, got.data_ptr(), block.data_ptr(), 1, ld, nq * ld, n_eligible=n_el, stream=st)
        torch.cuda.synchronize()
    finally:
        torch.cuda.set_stream(torch.cuda.default_stream())
    assert np.array_equal(hits(sc, got, nq, k), want)
    assert t.p.rescore_form()[0] == 1


# ---- the four summation orders ----

ORDERS = {"sse2": (0, 1), "seq": (1, 0), "avx_fma": (2, 2), "avx34_fma": (3, 3)}   # product constant, oracle constant


@pytest.mark.parametrize("name", list(ORDERS))
def test_sum_orders(sc, oracle, name):
    so, oo = ORDERS[name]
    before = oracle.get_sum_order()
    oracle.set_sum_order(oo)
    try:
        descs = column_values(45 + so, synth.random_descriptors(44, 250, binary=True))
        descs[30:60:3] = descs[9]
        rng = np.random.default_rng(46)
        queries = np.stack([descs[9], synth.rotate_descriptor(descs[9], 23)]
                           + [noisy_copy(rng, descs[int(rng.integers(0, 250))], int(rng.integers(0, 60)), 60) for _ in range(3)])
        t = Forms(sc, oracle, descs, sum_order=so)
        try:
            t.check(queries, 10, 240)
        finally:
            t.close()
    finally:
        oracle.set_sum_order(before)


# ---- which form a launch takes ----

def test_one_unpackable_entry_means_the_generic_form(sc, oracle):
    descs = tie_db()
    descs[137, 5 * 20 + 2], descs[137, 5 * 20 + 3] = np.float32(3.0), np.float32(3.5)   # two values in one column
    rng = np.random.default_rng(7)
    queries = np.stack([descs[137], descs[3]] + [noisy_copy(rng, descs[int(rng.integers(0, 200))], 9, 30) for _ in range(3)])
    m = sc.SCManager(filter_mode=FORCE)
    o = oracle.Manager()
    o.add_descriptors(descs.astype(np.float64))
    try:
        m.add_descriptors_f32(descs[:100])
        assert m.rescore_form() == (1, 0)
        m.add_descriptors_f32(descs[100:])
        assert m.rescore_form() == (0, 1)
        got = m.query(queries, k=10)
        assert m.profiled_kernel_name() != "sc_pair_kernel"
        want = np.stack([o.exhaustive(q.astype(np.float64), n_eligible=200, k=10, nthreads=4) for q in queries])
        assert np.array_equal(got, want)
        assert m.rescore_form() == (0, 1)
    finally:
        m.close()


def test_inserts_that_do_not_synchronise_leave_the_form_unknown(sc, oracle):
    import torch
    clouds, _ = synth.keyframe_clouds(331, 40, binary_z=True, loop_frac=0.2, min_gap=10, n_points=400)
    m = sc.SCManager(filter_mode=FORCE)
    o = oracle.Manager()
    try:
        for c in clouds[:39]:
            m.makeAndSaveScancontextAndKeys(c)
            o.add_points(c)
        assert m.rescore_form() == (0, -1), "rsx_sc_add_points does not wait: the count is unknown"
        queries = np.stack([o.descriptor(i) for i in (38, 20, 3)]).astype(np.float32)
        want = np.stack([o.exhaustive(o.descriptor(i), n_eligible=39, k=5) for i in (38, 20, 3)])
        # a device entry neither waits nor learns: generic form, same records
        dq = torch.from_numpy(queries).cuda()
        out = torch.zeros((3, 5, 2), dtype=torch.float64, device="cuda")
        m.query_device(dq.data_ptr(), 3, 5, out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert np.array_equal(hits(sc, out, 3, 5), want)
        assert m.rescore_form() == (0, -1)
        # the host-buffer entry synchronises anyway and reads the counter in front of that: this call still ran generic ...
        assert np.array_equal(m.query(queries, k=5), want)
        assert m.rescore_form() == (1, 0)
        # ... and the next one is packed
        assert np.array_equal(m.query(queries, k=5), want)
        m.makeAndSaveScancontextAndKeys(clouds[39])
        assert m.rescore_form() == (0, -1)
    finally:
        m.close()
