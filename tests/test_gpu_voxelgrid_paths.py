"""GPU parity of the VoxelGrid kernels (csrc/voxelgrid.hip through the C-ABI) against oracle/voxelgrid_ref.c, bit for bit,
in the regimes tests/test_gpu_voxelgrid.py does not reach: every edge of the sort key's width (7 | 8, 15 | 16, 23 | 24 bits and
31), wavefront shares too large for the cooperative kernel's registers (more than CO_MAX_W x 4 x CO_CH x 64 = 262 144 points),
the one-workgroup kernel at its padding edges and full, point layouts on the cooperative kernel, and max_out below the
output count.  The clouds come from tests/voxelgrid_cases.py; tests/test_voxelgrid_cases.py shows on the CPU that each is in
the regime it is named after."""
import ctypes as C

import numpy as np
import pytest

import voxelgrid_cases as vc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vgmod():
    from navtech_radar_slam_amd import _rsx, voxelgrid
    assert _rsx.device_count() >= 1
    return voxelgrid


def same(a, b):
    """two (m, 4) clouds hold the same points in the same order, bit for bit"""
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def raw_filter(vg, a, ioff, max_out, null_out=False):
    """rsx_voxelgrid_filter on the rows of a (stride = a row), into a host buffer of max(max_out, 1) + 64 rows pre-filled with
    the sentinel -> (out_count, the whole buffer as uint32)"""
    from navtech_radar_slam_amd._rsx import check
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = np.full((max(max_out, 1) + 64, 4), vc.SENTINEL, dtype=np.uint32)
    cnt = C.c_int64(-7)
    check(vg._L.rsx_voxelgrid_filter(vg._h, a.ctypes.data, a.shape[0], a.shape[1] * 4, ioff, vg.leaf, None if null_out else buf.ctypes.data,
                                     max_out, C.byref(cnt)))
    return cnt.value, buf


# ---- key widths ----
@pytest.mark.parametrize("n", vc.KEY_SIZES)
@pytest.mark.parametrize("div_b", list(vc.LATTICE) + ["wide"])
def test_key_widths(vgmod, oracle, div_b, n):
    """7, 8, 9, 15, 16, 23, 24 and 31 key bits: one to four radix passes, the last of them for the bit of the non-finite points
    alone at 8, 16 and 24; an even number of passes leaves the result in the sort's second buffer"""
    p, leaf = vc.wide_cloud(n) if div_b == "wide" else vc.lattice_cloud(div_b, n)
    want, ov = oracle.voxelgrid_filter(p, leaf)
    vg = vgmod.VoxelGrid(leaf=leaf)
    got = vg.filter(p)
    assert not ov and same(got, want)
    assert same(vg.filter(p), got)                                  # same handle, same bytes


# ---- large shares ----
@pytest.fixture(scope="module")
def large_refs(oracle):
    """n -> (cloud, oracle output), computed once"""
    refs = {}
    for n in sorted(set(vc.LARGE_SIZES)):
        p = vc.large_cloud(n % 97, n)[0]
        want, ov = oracle.voxelgrid_filter(p, vc.LARGE_LEAF)
        assert not ov
        refs[n] = (p, want)
    return refs


def test_large_shares_one_handle(vgmod, large_refs):
    """262 144 points (the last size whose shares fit the registers with 128 workgroups), 262 145 and 300 000 (chunk by chunk,
    one thread per voxel), 5000 (five workgroups) and 300 000 again, all on one handle"""
    vg = vgmod.VoxelGrid(leaf=vc.LARGE_LEAF)
    for n in vc.LARGE_SIZES:
        p, want = large_refs[n]
        assert same(vg.filter(p), want), n


def test_large_overflow_and_all_nan(vgmod, oracle, large_refs):
    """the cooperative kernel's two early exits at 300 000 points, each followed by an ordinary call on the same handle, of the
    same and of another grid size"""
    far, tiny = vc.overflow_cloud(6, 300000)
    want_far, ov = oracle.voxelgrid_filter(far, tiny)
    assert ov
    vg = vgmod.VoxelGrid(leaf=vc.LARGE_LEAF)
    assert len(vg.filter(np.full((300000, 4), np.nan, dtype=np.float32))) == 0
    assert same(vg.filter(large_refs[300000][0]), large_refs[300000][1])
    vg.leaf = tiny
    assert same(vg.filter(far), want_far)                           # overflow guard: input unchanged
    vg.leaf = vc.LARGE_LEAF
    for n in (5000, 300000):
        p, want = large_refs[n]
        assert same(vg.filter(p), want), n


# ---- the one-workgroup kernel ----
def test_one_workgroup_sizes(vgmod, oracle):
    """n at the power-of-two padding edges and at 4096 exactly (no padding, four positions per thread all in use), then 4097
    (the cooperative kernel) on the same handle"""
    vg = vgmod.VoxelGrid(leaf=vc.SMALL_LEAF)
    for n in vc.SMALL_SIZES:
        p = vc.small_cloud(n)
        want, ov = oracle.voxelgrid_filter(p, vc.SMALL_LEAF)
        assert not ov and same(vg.filter(p), want), n
    for p, leaf in (vc.one_voxel_cloud(), vc.own_voxel_cloud()):
        want, ov = oracle.voxelgrid_filter(p, leaf)
        assert not ov and len(want) in (1, 4096) and same(vgmod.VoxelGrid(leaf=leaf).filter(p), want), leaf


# ---- layouts on the cooperative kernel ----
@pytest.mark.parametrize("stride,ioff", vc.LAYOUTS)
def test_layouts_on_the_cooperative_kernel(vgmod, oracle, stride, ioff):
    p, leaf = vc.truncation_cloud(6000)
    a = vc.layout_cloud(p, stride, ioff)
    want, ov = oracle.voxelgrid_filter(a, leaf, intensity_col=ioff // 4 if ioff >= 0 else None)
    vg = vgmod.VoxelGrid(leaf=leaf)
    cnt, buf = raw_filter(vg, a, ioff, len(a))
    assert not ov and cnt == len(want) and same(buf[:cnt], want) and (buf[cnt:] == vc.SENTINEL).all()
    assert np.isfinite(want).all() and (ioff >= 0 or not want[:, 3].any())


# ---- truncation ----
@pytest.mark.parametrize("n", (3000, 6000))
@pytest.mark.parametrize("kind", ("grid", "overflow"))
def test_max_out_below_the_output_count(vgmod, oracle, kind, n):
    """out_count is the full count whatever max_out; the first min(count, max_out) rows are the oracle's and nothing is written
    past them; and after a call whose device buffer was reserved for one point, a full-size call on the handle is exact"""
    p, leaf = vc.truncation_cloud(n) if kind == "grid" else vc.overflow_cloud(6, n)
    want, ov = oracle.voxelgrid_filter(p, leaf)
    m = len(want)
    assert ov == (kind == "overflow") and (m == n if ov else 64 < m < n)
    vg = vgmod.VoxelGrid(leaf=leaf)
    for max_out in (0, 1, m - 1, m, m + 1):
        cnt, buf = raw_filter(vg, p, 12, max_out, null_out=(max_out == 0))
        w = min(m, max_out)
        assert cnt == m, max_out
        assert same(buf[:w], want[:w]), max_out
        assert (buf[w:] == vc.SENTINEL).all(), max_out
        if max_out == 1:
            assert same(vg.filter(p), want)
    small = vgmod.VoxelGrid(leaf=leaf)                             # a fresh handle: its first device buffer is the one-point one
    cnt, buf = raw_filter(small, p, 12, 1)
    assert cnt == m and same(buf[:1], want[:1]) and (buf[1:] == vc.SENTINEL).all()
    assert same(small.filter(p), want)
