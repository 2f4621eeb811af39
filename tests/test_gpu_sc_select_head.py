"""GPU tests of the head-only short list (csrc/sc_filter.hip sc_select_kernel, csrc/sc_kernels.hip sc_rescore_wave_kernel).

The selection stores the records of the HEAD of a query's short list only (whole bins, >= RESCORE_HEAD = 512 positions unless
the list is shorter); the re-scoring kernel finds the list positions behind the head in the query's row of bounds.  Whatever
the walk does, the records a query returns are the oracle's, byte for byte: np.array_equal on HIT_DTYPE, every query.
"""
import os

import numpy as np
import pytest

from navtech_radar_slam_amd import synth

pytestmark = pytest.mark.gpu

FORCE, OFF = 2, 1
HEAD, CAP = 512, 2048  # RESCORE_HEAD, RESCORE_SHORTLIST_CAP (csrc/sc_kernels.h)
NTHREADS = min(16, os.cpu_count() or 8)


@pytest.fixture(scope="module")
def sc():
    from navtech_radar_slam_amd import _rsx, scancontext
    assert _rsx.device_count() >= 1, "no HIP device: GPU tests must run on the MI355X box"
    return scancontext


def oracle_of(oracle, descs):
    o = oracle.Manager()
    o.add_descriptors(descs.astype(np.float64))
    return o


def want_per_query(o, queries, limits, k):
    """oracle records of queries whose eligibility limits differ"""
    return np.stack([o.exhaustive(q.astype(np.float64), n_eligible=int(lim), k=k, nthreads=4) for q, lim in zip(queries, limits)])


def rotated_queries(seed, descs, nq, blank=24):
    rng = np.random.default_rng(seed)
    n = len(descs)
    q = np.stack([synth.rotate_descriptor(descs[int(rng.integers(0, n))], int(rng.integers(0, 60))) for _ in range(nq)])
    np.put_along_axis(q, rng.integers(0, 1200, (nq, blank)), 0.0, axis=1)
    return q


def near_duplicates(seed, n, base, min_drop=0, max_drop=3):
    """n rotated copies of `base`, each with min_drop..max_drop of its occupied cells set to zero"""
    rng = np.random.default_rng(seed)
    occ = np.flatnonzero(base)
    out = np.empty((n, 1200), dtype=np.float32)
    for i in range(n):
        d = base.copy()
        d[rng.choice(occ, int(rng.integers(min_drop, max_drop + 1)), replace=False)] = 0
        out[i] = synth.rotate_descriptor(d, int(rng.integers(0, 60)))
    return out


def tail_db(binary):
    """Near-duplicates of one descriptor among unrelated entries: 2400 rotated copies of `common` with 0-3 cells dropped, where
    `common` is the (densely occupied) query descriptor `base` less 6 cells.  The ~600 exact copies of `common` lie at one
    distance D from `base` and share one bin, which is where the head ends (>= RESCORE_HEAD positions) and where tau sits for
    every k the tests use.  A dropped cell adds 5e-5 .. 2e-3 (a column holds ~12 cells), so hundreds of bounds lie in the next bins,
    whose lower edge tau + eps (eps = 2.56 bins) does not exclude: the walk has to leave the head."""
    base = synth.random_descriptors(70 + binary, 1, binary=binary, fill=0.6)[0]
    rand = synth.random_descriptors(72 + binary, 600, binary=binary)
    common = near_duplicates(74 + binary, 1, base, 6, 6)[0]
    dup = near_duplicates(76 + binary, 2400, common, 0, 3)
    return base, np.concatenate([rand[:300], dup, rand[300:]])


@pytest.mark.parametrize("binary", [True, False])
@pytest.mark.parametrize("n", [300, 700, 2500, 10300])
def test_row_sizes_against_oracle(sc, oracle, n, binary):
    """300: the whole row is shorter than the head; 700: head < row < cap; 2500 and 10 300: the row exceeds the cap, and 10 300
    entries also leave the one-piece row read of the selection (10 240)."""
    nq, k = 24, 10
    descs = synth.random_descriptors(500 + n + binary, n, binary=binary)
    queries = rotated_queries(n, descs, nq)
    queries[3] = 0
    g = sc.SCManager(filter_mode=FORCE, capacity_hint=n)
    g.add_descriptors_f32(descs)
    e = sc.SCManager(filter_mode=OFF, capacity_hint=n)
    e.add_descriptors_f32(descs)
    got = g.query(queries, k=k, n_eligible=n - 30)
    assert g.profiled_kernel_name() == "sc_spec2_filter_kernel"
    want = oracle_of(oracle, descs).exhaustive_batch(queries.astype(np.float64), n_eligible=n - 30, k=k, nthreads=NTHREADS)
    assert np.array_equal(got, want)
    assert np.array_equal(e.query(queries, k=k, n_eligible=n - 30), want)  # the exact-all path, the second reference
    g.close()
    e.close()


@pytest.fixture(scope="module")
def tail_case(sc, oracle):
    out = {}
    for binary in (True, False):
        base, db = tail_db(binary)
        g = sc.SCManager(filter_mode=FORCE, capacity_hint=len(db))
        g.add_descriptors_f32(db)
        out[binary] = (base, db, g, oracle_of(oracle, db))
    yield out
    for _, _, g, _ in out.values():
        g.close()


@pytest.mark.parametrize("binary", [True, False])
def test_near_duplicates_walk_behind_the_head(sc, oracle, tail_case, binary):
    base, db, g, o = tail_case[binary]
    rng = np.random.default_rng(5)
    queries = np.stack([synth.rotate_descriptor(base, int(r)) for r in rng.integers(0, 60, 20)] + [db[7], db[1000], np.zeros(1200, np.float32)])
    g.profile_enable(True)
    g.profile_read_rescoring_tail()
    tail_evals = tail_queries = 0
    for k in (10, 32):
        got = g.query(queries, k=k)
        st = g.profile_read_rescoring_tail()
        tail_evals += st[6]
        tail_queries += st[7]
        want = o.exhaustive_batch(queries.astype(np.float64), k=k, nthreads=NTHREADS)
        assert np.array_equal(got, want), f"k={k}"
    g.profile_enable(False)
    print(f"binary={binary}: {tail_evals} exact evaluations behind the head, {tail_queries} queries walked there")
    assert tail_evals > 0 and tail_queries > 0, "the walk never left the head: this test proves nothing"


@pytest.mark.parametrize("binary", [True, False])
def test_eligibility_cuts_head_and_tail(sc, oracle, tail_case, binary):
    """per-query limits (q_elig) through the two-stage protocol at world 1 (stage 1 = round 0, stage 2 = the rest of the walk):
    a limit inside the head, limits inside what lies behind it, fewer eligible entries than k, none at all"""
    from navtech_radar_slam_amd import sharded
    base, db, _, o = tail_case[binary]
    n, k = len(db), 10
    limits = np.array([0, 3, 9, 10, 330, 450, 700, 811, 1200, 1500, 2000, 2100, 2399, 2700, n, n, 640], dtype=np.int64)
    rng = np.random.default_rng(6)
    queries = np.stack([synth.rotate_descriptor(base, int(r)) for r in rng.integers(0, 60, len(limits))])
    queries[-2] = db[5]
    s = sharded.ShardedScanContext(filter_mode=FORCE, capacity_hint=n)
    s.add_descriptors_f32(db)
    s.backend.profile_enable(True)
    s.backend.profile_read_rescoring_tail()
    for ne in (-1, 1000, 4):
        got = s.query(queries, k=k, n_eligible=ne, q_elig=limits)
        lim = np.minimum(limits, n if ne < 0 else ne)
        assert np.array_equal(got, want_per_query(o, queries, lim, k)), f"n_eligible={ne}"
        mono = np.sort(limits)
        got = s.query(queries, k=k, n_eligible=ne, q_elig=mono)  # non-decreasing limits: the filter runs on its triangular plan
        assert np.array_equal(got, want_per_query(o, queries, np.minimum(mono, n if ne < 0 else ne), k)), f"n_eligible={ne} (monotone)"
    assert s.backend.profile_read_rescoring_tail()[6] > 0, "no limit cut the part of a list behind its head"
    s.close()


def test_one_bin_exceeds_head_and_cap(sc, oracle):
    """identical descriptors share one bound, so one histogram bin alone exceeds the head (700 copies) or the whole short list
    (3000 copies); the oracle's index order decides the ties"""
    rng = np.random.default_rng(17)
    base = synth.random_descriptors(40, 2, binary=False)
    rand = synth.random_descriptors(41, 400, binary=False)
    for copies in (HEAD + 188, CAP + 952):
        q = base[1].copy()
        near = []
        for i in range(5):  # five strictly better entries in front of the copies
            d = q.copy()
            d[rng.choice(np.flatnonzero(q), 3 + i, replace=False)] = 0
            near.append(d)
        far = q.copy()
        far[rng.choice(np.flatnonzero(q), 150, replace=False)] = 0
        db = np.concatenate([rand[:100], np.tile(far, (copies, 1)), np.stack(near), rand[100:]])
        g = sc.SCManager(filter_mode=FORCE, capacity_hint=len(db))
        g.add_descriptors_f32(db)
        o = oracle_of(oracle, db)
        queries = np.stack([q, synth.rotate_descriptor(q, 11), far, rand[3], np.zeros(1200, np.float32)])
        for k, ne in ((1, -1), (10, -1), (32, -1), (10, 100 + copies // 2)):
            got = g.query(queries, k=k, n_eligible=ne)
            want = o.exhaustive_batch(queries.astype(np.float64), n_eligible=(len(db) if ne < 0 else ne), k=k, nthreads=NTHREADS)
            assert np.array_equal(got, want), f"copies={copies} k={k} ne={ne}"
        g.close()


def test_rows_with_infinite_bounds(sc, oracle):
    """entries and queries without a non-empty column have the bound +inf against everything: in no bin, never a hit"""
    base = synth.random_descriptors(90, 1, binary=False)[0]
    db = np.concatenate([near_duplicates(91, 900, base), synth.random_descriptors(92, 300, binary=False)])
    db[::3] = 0  # every third entry is empty
    o = oracle_of(oracle, db)
    g = sc.SCManager(filter_mode=FORCE, capacity_hint=len(db))
    g.add_descriptors_f32(db)
    queries = np.stack([base, synth.rotate_descriptor(base, 17), np.zeros(1200, np.float32), db[1], db[1001]])
    for k, ne in ((10, -1), (32, -1), (10, 7), (10, 2)):
        got = g.query(queries, k=k, n_eligible=ne)
        want = o.exhaustive_batch(queries.astype(np.float64), n_eligible=(len(db) if ne < 0 else ne), k=k, nthreads=NTHREADS)
        assert np.array_equal(got, want), f"k={k} ne={ne}"
    assert np.all(got[2]["dist"] == 1e7)  # the empty query: padding only
    g.close()


def test_filter_shards_of_a_replicated_db_world_1(sc, oracle, tail_case):
    """the replicated-database layout (filter shards -> gathered bounds -> selection, window, re-scoring) with one rank"""
    from navtech_radar_slam_amd import sharded
    base, db, _, o = tail_case[False]
    rng = np.random.default_rng(8)
    queries = np.stack([synth.rotate_descriptor(base, int(r)) for r in rng.integers(0, 60, 12)] + [db[2], db[900]])
    s = sharded.FilterShardedScanContext(filter_mode=FORCE, capacity_hint=len(db))
    s.add_descriptors_f32(db)
    for k, ne in ((10, -1), (32, 1700)):
        got = s.query(queries, k=k, n_eligible=ne)
        want = o.exhaustive_batch(queries.astype(np.float64), n_eligible=(len(db) if ne < 0 else ne), k=k, nthreads=NTHREADS)
        assert np.array_equal(got, want), f"k={k} ne={ne}"
    s.close()


def test_query_self_1500(sc, oracle):
    """every keyframe against the keyframes older than itself (growing per-query limits, the filter's triangular plan)"""
    import torch
    n, k, excl = 1500, 10, 30
    base = synth.random_descriptors(60, 1, binary=True)[0]
    db = np.concatenate([synth.random_descriptors(61, 500, binary=True), near_duplicates(62, 1000, base)])
    db = db[np.random.default_rng(63).permutation(n)]
    g = sc.SCManager(filter_mode=FORCE, capacity_hint=n)
    g.add_descriptors_f32(db)
    out = torch.zeros((n, k, 2), dtype=torch.float64, device="cuda")
    g.query_self_device(0, n, k, out.data_ptr(), exclude_recent=excl, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(sc.HIT_DTYPE).reshape(n, k)
    o = oracle_of(oracle, db)
    which = list(range(0, 60)) + list(range(60, n, 9)) + [n - 1]
    want = want_per_query(o, db[which], [max(0, i - excl) for i in which], k)
    assert np.array_equal(got[which], want)
    g.close()
