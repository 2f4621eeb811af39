"""Spectral form of the lower-bound filter (csrc/sc_spec.hip) on a real MI355X: its bounds are valid lower
bounds of the fp64 all-shift minimum and close to it, and every query path gives the oracle's results
with filter_kind = spectral exactly as with the direct filter."""
import hashlib
import os
import zlib

import numpy as np
import pytest

from test_gpu_sc_filter import all_shift_bound, make_db

pytestmark = pytest.mark.gpu

ONE_WAVE_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sc_spec_onewave_bounds.npz")
ONE_WAVE_COLS = np.r_[0:128, 4096:4096 + 77]      # the first tile-block and the ragged end, kept in full


@pytest.fixture(scope="module")
def sc():
    from navtech_radar_slam_amd import scancontext
    return scancontext


@pytest.fixture(scope="module")
def rsx():
    from navtech_radar_slam_amd import _rsx
    return _rsx


@pytest.fixture(scope="module")
def synth():
    from navtech_radar_slam_amd import synth
    return synth


@pytest.fixture(scope="module")
def oracle():
    from oracle import pyoracle
    return pyoracle


@pytest.fixture(params=["spectral2"])
def spec_kind(request, rsx):
    """the spectral filter, sc_spec2_filter_kernel (KIND_SPECTRAL names the same kernel:
    test_both_spectral_kinds_run_the_two_wave_kernel)"""
    return rsx.KIND_SPECTRAL2


def n_cols(d):
    return (np.sqrt((d.reshape(-1, 60, 20).astype(np.float64) ** 2).sum(2)) > 0).sum(1)


@pytest.mark.parametrize("binary", [True, False])
def test_spectral_bounds(sc, rsx, synth, binary, spec_kind):
    n, nq = 1000 + 13, 24                                # ragged last tile, 6 query tiles
    descs = make_db(100 + binary, n, binary)
    rng = np.random.default_rng(9)
    queries = np.stack([synth.rotate_descriptor(descs[int(rng.integers(0, n))], int(rng.integers(0, 60))) for _ in range(nq)])
    queries[::2, rng.integers(0, 1200, 20)] = 0
    queries[1] = 0                                       # empty query
    queries[3].reshape(60, 20)[7:31] = 0                 # 24 empty sectors: wide [n_lo, n_hi]
    g = sc.SCManager(filter_kind=spec_kind)
    g.add_descriptors_f32(descs)
    eps = g.filter_eps()
    lb = g.filter_bounds(queries)
    ne = n_cols(descs)
    worst_tight = 0.0
    for qi in range(nq):
        want = all_shift_bound(queries[qi], descs)
        fin = np.isfinite(want)
        assert np.all(lb[qi][~fin] == np.inf), "no effective column at any shift -> +inf"
        if not fin.any():
            continue
        assert (lb[qi][fin] - eps - want[fin]).max() <= 0.0, f"q={qi}: not a lower bound"
        # tightness where S >= 0 (negative heights are clamped to S = 0: valid, looser): within the spectral
        # error budget 2.05e-3 sqrt(nq ne) / n_lo plus the reciprocal bound's excess
        nq_c = int(n_cols(queries[qi])[0])
        nlo = np.maximum(nq_c + ne - 60, 1)
        nhi = np.maximum(np.minimum(nq_c, ne), nlo)
        slack = 2.05e-3 * np.sqrt(nq_c * ne) / nlo + eps + (nhi - nlo) ** 3 / (4.0 * nlo * nhi ** 2) + 1e-5
        ok = fin & (want <= 1.0)
        gap = want[ok] - (lb[qi][ok] - eps) - 2.0 ** -10 * np.abs(want[ok])   # the stored bound is fp16, rounded toward zero
        assert np.all(gap <= slack[ok] + eps), f"q={qi}: bound looser than the budget"
        if nq_c >= 50:
            worst_tight = max(worst_tight, float(np.max(gap - 2.05e-3 * np.sqrt(nq_c * ne[ok]) / nlo[ok])))
    assert worst_tight < 2e-3      # observed error is far inside the budget


@pytest.mark.parametrize("k", [1, 10, 32])
def test_spectral_query_matches_oracle(sc, rsx, synth, oracle, k, spec_kind):
    n, nq = 2500 + 5, 41
    descs = make_db(7, n, True)
    rng = np.random.default_rng(3)
    queries = np.stack([synth.rotate_descriptor(descs[int(rng.integers(0, n))], int(rng.integers(0, 60))) for _ in range(nq)])
    queries[::3, rng.integers(0, 1200, 40)] = 0
    queries[5] = 0
    g = sc.SCManager(filter_mode=rsx.FILTER_FORCE, filter_kind=spec_kind)
    g.add_descriptors_f32(descs)
    got = g.query(queries, k=k, n_eligible=n - 30)
    o = oracle.Manager()
    o.add_descriptors(descs.astype(np.float64))
    for qi in range(nq):
        assert np.array_equal(got[qi], o.exhaustive(queries[qi].astype(np.float64), n_eligible=n - 30, k=k, nthreads=4)), qi


def test_spectral_equals_direct_10k(sc, rsx, synth):
    n, nq, k = 10_000, 300, 10
    descs = synth.random_descriptors(42, n, binary=True)
    rng = np.random.default_rng(43)
    queries = np.stack([synth.rotate_descriptor(descs[int(rng.integers(0, n))], int(rng.integers(0, 60))) for _ in range(nq)])
    queries[::4, rng.integers(0, 1200, 60)] = 0
    res = []
    for kind in (rsx.KIND_DIRECT, rsx.KIND_SPECTRAL, rsx.KIND_SPECTRAL2):
        g = sc.SCManager(filter_mode=rsx.FILTER_FORCE, filter_kind=kind, capacity_hint=n)
        g.add_descriptors_f32(descs)
        res.append(g.query(queries, k=k))
    off = sc.SCManager(filter_mode=rsx.FILTER_OFF, capacity_hint=n)
    off.add_descriptors_f32(descs)
    want = off.query(queries, k=k)
    assert np.array_equal(res[0], want)
    assert np.array_equal(res[1], want)
    assert np.array_equal(res[2], want)


def test_spectral_self_queries_and_shards(sc, rsx, synth, spec_kind):
    """triangular plan in query-tile units + the staged protocol over 3 shard handles"""
    import torch
    n, k, excl = 3017, 10, 30
    descs = make_db(55, n, True)
    off = sc.SCManager(filter_mode=rsx.FILTER_OFF)
    off.add_descriptors_f32(descs)
    tstream = torch.cuda.Stream()
    torch.cuda.set_stream(tstream)
    st = tstream.cuda_stream
    want_d = torch.zeros((n, k, 2), dtype=torch.float64, device="cuda")
    off.query_self_device(0, n, k, want_d.data_ptr(), exclude_recent=excl, stream=st)
    torch.cuda.synchronize()
    want = want_d.cpu().numpy().view(sc.HIT_DTYPE).reshape(n, k)
    g = sc.SCManager(filter_mode=rsx.FILTER_FORCE, filter_kind=spec_kind)
    g.add_descriptors_f32(descs)
    out = torch.zeros((n, k, 2), dtype=torch.float64, device="cuda")
    for first, cnt in ((0, n), (1001, 777)):
        out.zero_()
        g.query_self_device(first, cnt, k, out.data_ptr(), exclude_recent=excl, stream=st)
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(sc.HIT_DTYPE).reshape(n, k)[:cnt]
        assert np.array_equal(got, want[first:first + cnt]), (first, cnt)
    world = 3
    shards = [sc.SCManager(shard_rank=r, shard_world=world, filter_mode=rsx.FILTER_FORCE, filter_kind=spec_kind)
              for r in range(world)]
    for s in shards:
        s.add_descriptors_f32(descs)
    dq = torch.from_numpy(descs).cuda()
    lim = torch.clamp(torch.arange(n, dtype=torch.int64, device="cuda") - excl, min=0)
    parts = torch.zeros((world, n, k, 2), dtype=torch.float64, device="cuda")
    glob = torch.zeros((n, k, 2), dtype=torch.float64, device="cuda")
    finals = torch.zeros((world, n, k, 2), dtype=torch.float64, device="cuda")
    for r, s in enumerate(shards):
        s.query_stage1_device(dq.data_ptr(), n, k, parts[r].data_ptr(), stream=st, q_elig_ptr=lim.data_ptr(), elig_monotone=True)
    shards[0].merge_device(parts.data_ptr(), world, n, k, glob.data_ptr(), stream=st)
    for r, s in enumerate(shards):
        s.query_stage2_device(n, k, glob.data_ptr(), finals[r].data_ptr(), stream=st)
    shards[0].merge_device(finals.data_ptr(), world, n, k, out.data_ptr(), stream=st)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(sc.HIT_DTYPE).reshape(n, k), want)
    torch.cuda.set_stream(torch.cuda.default_stream())


def one_wave_fixture(synth, binary):
    """(descs [4173][1200], queries [203][1200]) of the pin below and of tools/make_spec_onewave_golden.py, from fixed
    seeds: ragged entry tiles, partial query tiles, queries with and without empty columns, empty and non-finite
    descriptors"""
    n, nq = 4096 + 77, 203
    descs = make_db(300 + binary, n, binary)
    rng = np.random.default_rng(17)
    queries = np.stack([synth.rotate_descriptor(descs[int(rng.integers(0, n))], int(rng.integers(0, 60))) for _ in range(nq)])
    queries[::2, rng.integers(0, 1200, 20)] = 0
    queries[1] = 0
    queries[3].reshape(60, 20)[7:31] = 0
    queries[8:40] = synth.random_descriptors(5, 32, binary=False) + np.float32(0.5)   # no empty column: the short tail path
    queries[11, 5] = np.nan
    descs[12, 100] = np.inf
    return descs, queries


def bound_digest(lb):
    """what the golden file keeps of a float32 bound matrix [nq][n]: (SHA-256 of its uint32 view, one CRC32 per query
    row [nq] uint32, the bit patterns of ONE_WAVE_COLS [nq][205] uint32)"""
    bits = np.ascontiguousarray(lb).view(np.uint32)
    crc = np.array([zlib.crc32(row.tobytes()) for row in bits], dtype=np.uint32)
    return hashlib.sha256(bits.tobytes()).hexdigest(), crc, bits[:, ONE_WAVE_COLS].copy()


@pytest.mark.parametrize("binary", [True, False])
def test_two_wave_mapping_gives_the_same_bounds(sc, rsx, synth, binary):
    """sc_spec2_filter_kernel splits the entry tile by frequency over two waves; every accumulator still sees its K-steps
    in the same order as in the retired one-wave-per-SIMD kernel, so its bounds equal that kernel's BIT FOR BIT.  The
    one-wave kernel's bounds of this fixture were recorded before it was deleted (tools/make_spec_onewave_golden.py):
    a hash of the whole matrix, a CRC per query row, and the first tile-block and the ragged end in full"""
    descs, queries = one_wave_fixture(synth, binary)
    b = sc.SCManager(filter_kind=rsx.KIND_SPECTRAL2, capacity_hint=len(descs))
    b.add_descriptors_f32(descs)
    lb2 = b.filter_bounds(queries)
    assert b.profiled_kernel_name() == "sc_spec2_filter_kernel"
    assert lb2.shape == (len(queries), len(descs)) and lb2.dtype == np.float32
    gold = np.load(ONE_WAVE_GOLDEN)
    tag = "binary" if binary else "continuous"
    sha, crc, cols = bound_digest(lb2)
    rows = np.flatnonzero(crc != gold["crc32_" + tag])
    diff = np.argwhere(cols != gold["cols_" + tag])
    first = (int(diff[0, 0]), int(ONE_WAVE_COLS[diff[0, 1]])) if len(diff) else None
    assert sha == str(gold["sha256_" + tag]) and len(rows) == 0, \
        f"{len(rows)} query rows differ from the one-wave kernel's bounds: {rows[:16].tolist()}; " \
        f"first differing (query, entry) inside the stored columns: {first}"
    assert np.array_equal(cols, gold["cols_" + tag]), first


def test_both_spectral_kinds_run_the_two_wave_kernel(sc, rsx, synth):
    """KIND_SPECTRAL is kept as a synonym of KIND_SPECTRAL2: a ragged entry tile and a partial query tile"""
    n, nq = 96 + 13, 9
    descs = make_db(21, n, False)
    queries = np.stack([synth.rotate_descriptor(descs[(11 * i) % n], (7 * i) % 60) for i in range(nq)])
    queries[1] = 0
    queries[::2, 40:60] = 0
    bits = []
    for kind in (rsx.KIND_SPECTRAL, rsx.KIND_SPECTRAL2):
        g = sc.SCManager(filter_kind=kind)
        g.add_descriptors_f32(descs)
        bits.append(g.filter_bounds(queries).view(np.uint32))
        assert g.profiled_kernel_name() == "sc_spec2_filter_kernel"
    assert bits[0].shape == (nq, n) and np.array_equal(bits[0], bits[1])


def test_default_kind_is_spectral(sc, rsx, synth):
    n = 2000
    holes = synth.random_descriptors(5, n, binary=True)
    g = sc.SCManager(filter_mode=rsx.FILTER_FORCE)
    g.add_descriptors_f32(holes)
    g.query(holes[:16], k=3)
    assert g.profiled_kernel_name() == "sc_spec2_filter_kernel"      # the spectral form, two waves per SIMD
    g1 = sc.SCManager(filter_mode=rsx.FILTER_FORCE, filter_kind=rsx.KIND_SPECTRAL)
    g1.add_descriptors_f32(holes)
    g1.query(holes[:16], k=3)
    assert g1.profiled_kernel_name() == "sc_spec2_filter_kernel"     # the synonym
    g2 = sc.SCManager(filter_mode=rsx.FILTER_FORCE, filter_kind=rsx.KIND_DIRECT)
    g2.add_descriptors_f32(holes)
    g2.query(holes[:16], k=3)
    assert g2.profiled_kernel_name() == "sc_filter_kernel"


def test_spectral_random_shapes(sc, rsx, synth, spec_kind):
    """ragged sizes: 1..70 queries (partial query tiles), 1..1500 entries (partial 32-entry tiles and 128-entry
    tile-blocks, workgroups that straddle tile-blocks), k in {1, 3, 10}, eligibility prefixes -- spectral filter ==
    exact path, record for record"""
    rng = np.random.default_rng(2024)
    for trial in range(14):
        n = int(rng.integers(1, 1500))
        nq = int(rng.integers(1, 70))
        k = int(rng.choice([1, 3, 10]))
        binary = bool(trial & 1)
        descs = synth.random_descriptors(900 + trial, n, binary=binary)
        q = np.stack([synth.rotate_descriptor(descs[int(rng.integers(0, n))], int(rng.integers(0, 60))) for _ in range(nq)])
        q[::3, rng.integers(0, 1200, 30)] = 0
        n_elig = int(rng.integers(0, n + 1)) if trial % 3 == 0 else -1
        f = sc.SCManager(filter_mode=rsx.FILTER_FORCE, filter_kind=spec_kind)
        o = sc.SCManager(filter_mode=rsx.FILTER_OFF)
        f.add_descriptors_f32(descs)
        o.add_descriptors_f32(descs)
        got, want = f.query(q, k=k, n_eligible=n_elig), o.query(q, k=k, n_eligible=n_elig)
        assert np.array_equal(got, want), (trial, n, nq, k, n_elig)
