"""Every cloud of tests/voxelgrid_cases.py is in the regime its name claims -- checked with the oracle
(oracle/voxelgrid_ref.c) and numpy alone, no GPU: the overflow flag, the grid's volume and with it the width of the sort key
and the number of radix passes, shared voxels, the sizes of the crowded voxels, the non-finite rows at the tile ends.
tests/test_gpu_voxelgrid_paths.py runs the same clouds through the kernels."""
import numpy as np
import pytest

import voxelgrid_cases as vc


def _shared_voxels(oracle, p, leaf):
    """(overflow, output points, finite input points): the oracle's count against numpy's voxel indices"""
    out, ov = oracle.voxelgrid_filter(p, leaf)
    idx = vc.voxel_index(p, leaf)
    assert len(out) == len(np.unique(idx[idx >= 0]))           # numpy's voxel indices are the oracle's
    return ov, len(out), int((idx >= 0).sum())


def _nonfinite_rows(p):
    return np.flatnonzero(~np.isfinite(p[:, :3]).all(1))


@pytest.mark.parametrize("n", vc.KEY_SIZES)
@pytest.mark.parametrize("div_b", list(vc.LATTICE))
def test_lattice_cases_have_their_key_width(oracle, div_b, n):
    p, leaf = vc.lattice_cloud(div_b, n)
    vol, nbits, passes = vc.LATTICE[div_b]
    f = vc.grid_facts(p, leaf)
    assert len(p) == n and leaf == 1.0 and np.float32(1.0) / np.float32(leaf) == 1.0
    assert f["div_b"] == div_b and (f["min_b"] == 0).all()
    assert (f["vol"], f["nbits"], f["passes"]) == (vol, nbits, passes) and f["d_prod"] == vol
    assert vol == div_b[0] * div_b[1] * div_b[2] and 2 ** nbits >= vol and (nbits == 0 or 2 ** (nbits - 1) < vol)
    ov, m, nfin = _shared_voxels(oracle, p, leaf)
    assert not ov and not f["overflow"] and m < nfin           # at least one voxel holds two points or more
    idx = vc.voxel_index(p, leaf)
    assert idx[1] == 0 and idx[n - 2] == vol - 1               # the smallest and the largest key are present
    bad = _nonfinite_rows(p)
    assert len(bad) * 100 >= n and {0, n - 1, 63, 64, 65, 1023, 1024, 1025} <= set(bad.tolist())
    v0 = np.flatnonzero(idx == 0)                              # voxel 0 has points on both sides of non-finite rows
    assert set(vc.VOXEL0_ROWS) <= set(v0.tolist())
    assert sum(((bad > a) & (bad < b)).any() for a, b in zip(v0[:-1], v0[1:])) >= 4 and bad[0] < v0[0]
    frac = p[idx >= 0, :3] - np.floor(p[idx >= 0, :3])
    assert frac.min() >= 0.25 and frac.max() <= 0.75           # no coordinate near a voxel face: the facts are exact


def test_lattice_table_is_the_issue_s():
    """the passes follow from nbits, and the table holds each side of the 8-, 16- and 24-bit edges"""
    assert sorted(v[1] for v in vc.LATTICE.values()) == [7, 8, 9, 15, 16, 23, 24]
    for vol, nbits, passes in vc.LATTICE.values():
        assert passes == (nbits + 8) // 8


@pytest.mark.parametrize("n", vc.KEY_SIZES)
def test_wide_case_has_31_bits(oracle, n):
    p, leaf = vc.wide_cloud(n)
    f = vc.grid_facts(p, leaf)
    assert (f["vol"], f["nbits"], f["passes"]) == vc.WIDE_FACTS and f["div_b"] == (1291, 1291, 1001)
    assert 2 ** 30 < f["vol"] < 2 ** 31 and f["d_prod"] == f["vol"] and not f["overflow"]
    ov, m, nfin = _shared_voxels(oracle, p, leaf)
    assert not ov and m < nfin
    idx = vc.voxel_index(p, leaf)
    assert idx[1] == 0 and idx[n - 2] == f["vol"] - 1 and idx.max() > 2 ** 30
    bad = _nonfinite_rows(p)
    assert len(bad) * 100 >= n and {0, n - 1, 63, 64, 65, 1023, 1024, 1025} <= set(bad.tolist())


@pytest.mark.parametrize("n", sorted(set(vc.LARGE_SIZES)))
def test_large_clouds(oracle, n):
    p, a, b = vc.large_cloud(n % 97, n)
    c = vc.crowd_size(n)
    assert len(p) == n and len(a) == len(b) == c and c == (20000 if n > 5000 else 500)
    ov, m, nfin = _shared_voxels(oracle, p, vc.LARGE_LEAF)
    assert not ov and m < nfin
    bad = _nonfinite_rows(p)
    assert 0.03 * n <= len(bad) <= 0.04 * n
    want = {0, n - 1} | {k + s for k in range(2304, n - 1, 2304) for s in (-1, 0, 1)}
    assert want <= set(bad.tolist())
    idx = vc.voxel_index(p, vc.LARGE_LEAF)
    assert len(set(idx[a].tolist())) == 1 and len(set(idx[b].tolist())) == 1 and idx[a[0]] != idx[b[0]] and idx[a[0]] >= 0 and idx[b[0]] >= 0
    assert (idx == idx[a[0]]).sum() == c and (idx == idx[b[0]]).sum() == c      # the crowded voxels: exactly c points each
    tile = 2560 if n == 300000 else 2304                                         # a workgroup's tile with 128 workgroups
    if n > 5000:
        assert a[-1] - a[0] > 7 * tile                                           # consecutive (but for non-finite rows), several tiles
        assert a[-1] - a[0] < 1.2 * c and b[0] < tile and b[-1] > n - tile and np.diff(b).max() < 2 * n // c
    # the share of a wavefront: past CO_CH * 64 = 512 points from 262 145 points on, whatever the number of workgroups (<= 128)
    share = (n + 127) // 128                  # points per workgroup ...
    per = (share + 255) // 256 * 256          # ... rounded up to its tile, a multiple of 256; a wavefront walks a quarter
    assert (per // 4 > 512) == (n > 262144)


def test_large_overflow_and_small_sizes(oracle):
    p, leaf = vc.overflow_cloud(6, 300000)
    got, ov = oracle.voxelgrid_filter(p, leaf)
    assert ov and vc.grid_facts(p, leaf)["overflow"] and np.array_equal(got, p)
    for n in (3000, 6000):
        p, leaf = vc.overflow_cloud(6, n)
        assert oracle.voxelgrid_filter(p, leaf)[1] and vc.grid_facts(p, leaf)["overflow"]
    for n in vc.SMALL_SIZES:
        p = vc.small_cloud(n)
        assert len(p) == n and not np.isfinite(p[0, 0]) and not np.isfinite(p[n - 1, 2])
        if n <= 2:
            assert len(oracle.voxelgrid_filter(p, vc.SMALL_LEAF)[0]) == 0
            continue
        ov, m, nfin = _shared_voxels(oracle, p, vc.SMALL_LEAF)
        assert not ov and nfin == n - 2 and m < nfin
    p, leaf = vc.one_voxel_cloud()
    ov, m, nfin = _shared_voxels(oracle, p, leaf)
    assert not ov and (m, nfin) == (1, 4096)
    p, leaf = vc.own_voxel_cloud()
    ov, m, nfin = _shared_voxels(oracle, p, leaf)
    assert not ov and (m, nfin) == (4096, 4096)


@pytest.mark.parametrize("n", (3000, 6000))
def test_truncation_and_layout_clouds(oracle, n):
    p, leaf = vc.truncation_cloud(n)
    ov, m, nfin = _shared_voxels(oracle, p, leaf)
    assert not ov and 64 < m < nfin < n                        # max_out = 1 and m - 1 really cut the output
    assert not (oracle.voxelgrid_filter(p, leaf)[0].view(np.uint32) == vc.SENTINEL).any()
    for stride, ioff in vc.LAYOUTS:
        a = vc.layout_cloud(p, stride, ioff)
        assert a.shape == (n, stride // 4) and a.strides[0] == stride
        got, _ = oracle.voxelgrid_filter(a, leaf, intensity_col=ioff // 4 if ioff >= 0 else None)
        want, _ = oracle.voxelgrid_filter(p if ioff >= 0 else p[:, :3], leaf)
        assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
