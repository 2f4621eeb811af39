"""The packed column image of the ScanContext database (csrc/sc_kernels.h PackedCol, csrc/sc_entry_dev.h pack_entry): 60
records of 16 bytes per entry, { u32 bits (bit r = ring r occupied), f32 val, f64 norm }.  An entry is packable when every
element of every column is +0.0 (all bits zero) or bit-equal to ONE finite value of that column; a -0.0, a NaN, an inf or two
different non-zero values in a column make it unpackable.  The rule and the layout are written down once more here, as a numpy
packer; the packer is checked on the CPU, and rsx_sc_packed_export must equal it byte for byte for every packable entry --
behind both kernels that fill the image (the batched image build and the one-launch insert) and across a capacity doubling."""
import numpy as np
import pytest

from navtech_radar_slam_amd import synth

PACKED = np.dtype([("bits", np.uint32), ("val", np.float32), ("norm", np.float64)])


def column_norms(descs):
    """Eigen's norm() of every column as the default reference build takes it (2-double packets): the square of element r goes
    to accumulator r % 4, result sqrt((a0 + a2) + (a1 + a3)).  -> (n, 60) float64"""
    x = descs.reshape(-1, 60, 20).astype(np.float64)
    acc = np.zeros(x.shape[:2] + (4,))
    with np.errstate(all="ignore"):
        for i in range(5):
            acc = acc + x[:, :, 4 * i:4 * i + 4] * x[:, :, 4 * i:4 * i + 4]   # (squares of fp32 values are exact in fp64)
        return np.sqrt((acc[..., 0] + acc[..., 2]) + (acc[..., 1] + acc[..., 3]))


def pack(descs):
    """-> (records (n, 60) of PACKED, packable (n,) bool)"""
    descs = np.ascontiguousarray(descs, dtype=np.float32).reshape(-1, 1200)
    u = descs.view(np.uint32).reshape(-1, 60, 20)
    occ = u != 0                                              # everything but +0.0
    bits = (occ.astype(np.uint32) << np.arange(20, dtype=np.uint32)).sum(axis=2, dtype=np.uint32)
    first = np.argmax(occ, axis=2)
    val = np.take_along_axis(u, first[..., None], axis=2)[..., 0]
    val = np.where(occ.any(axis=2), val, np.uint32(0))
    same = ((u == val[..., None]) | ~occ).all(axis=2)
    finite = (val & np.uint32(0x7f800000)) != np.uint32(0x7f800000)
    col_ok = same & finite & (val != np.uint32(0x80000000))
    rec = np.zeros(u.shape[:2], dtype=PACKED)
    rec["bits"] = bits
    rec["val"] = val.view(np.float32)
    rec["norm"] = column_norms(descs)
    return rec, col_ok.all(axis=1)


def unpack(rec):
    """the descriptors a set of records stands for -> (n, 1200) float32"""
    on = (rec["bits"][..., None] >> np.arange(20, dtype=np.uint32)) & np.uint32(1)
    return np.where(on != 0, rec["val"][..., None], np.float32(0.0)).astype(np.float32).reshape(len(rec), 1200)


def column_constant(seed, n):
    """packable entries whose columns hold different values (and empty columns: random_descriptors blanks an arc)"""
    d = synth.random_descriptors(seed, n, binary=True).reshape(n, 60, 20)
    vals = np.random.default_rng(seed + 1).uniform(0.5, 9.0, (n, 60, 1)).astype(np.float32)
    return np.ascontiguousarray(np.where(d != 0, vals, np.float32(0.0)).reshape(n, 1200), dtype=np.float32)


def packable_fixture():
    binary = synth.random_descriptors(301, 40, binary=True)
    cols = column_constant(302, 40)
    sparse = synth.random_descriptors(303, 8, binary=True, fill=0.02)   # many empty columns
    sparse[3] = 0                                                       # an entry with nothing in it
    return np.concatenate([binary, cols, sparse])


def unpackable_fixture():
    """one entry each: two values in a column that differ in the last bit, a -0.0, a NaN, an inf"""
    d = column_constant(305, 4).reshape(4, 60, 20)
    d[:, 11, :] = np.float32(3.0)
    d[0, 11, 7] = np.nextafter(np.float32(3.0), np.float32(4.0))
    d[1, 11, 0] = np.float32(-0.0)
    d[2, 11, 19] = np.nan
    d[3, 11, 4] = np.inf
    return d.reshape(4, 1200)


# ---- the packer and the predicate themselves: no GPU ----

def test_packer_round_trip_and_layout():
    assert PACKED.itemsize == 16 and PACKED.fields["val"][1] == 4 and PACKED.fields["norm"][1] == 8
    descs = packable_fixture()
    rec, ok = pack(descs)
    assert ok.all()
    assert np.array_equal(unpack(rec).view(np.uint32), descs.view(np.uint32)), "a packable entry is its records"
    empty = ~(descs.reshape(-1, 60, 20) != 0).any(axis=2)
    assert empty.any() and empty[40 + 40 + 3].all()
    assert np.all(rec["bits"][empty] == 0) and np.all(rec["val"][empty].view(np.uint32) == 0) and np.all(rec["norm"][empty] == 0.0)
    full = rec["bits"] == 0xfffff
    cnt = np.array([bin(int(b)).count("1") for b in rec["bits"].ravel()]).reshape(rec.shape)
    assert rec["bits"].max() < (1 << 20) and not full.all()
    # binary entries: every occupied ring holds 2.0, the norm is 2 sqrt(rings) exactly where that is a double
    assert np.all(rec["val"][:40][rec["bits"][:40] != 0] == np.float32(2.0))
    four = cnt[:40] == 4
    assert four.any() and np.all(rec["norm"][:40][four] == 4.0)


def test_predicate():
    rec, ok = pack(unpackable_fixture())
    assert not ok.any()
    d = column_constant(306, 6).reshape(6, 60, 20)
    d[:, 5, :] = 0
    d[0, 5, 3] = np.float32(-0.0)          # a lone -0.0 in an otherwise empty column
    d[1, 5, :] = np.float32(-1.5)          # negative values are values
    d[2, 5, 3] = np.float32(1e-45)         # the smallest subnormal
    d[3, 5, 3], d[3, 5, 4] = np.float32(1.0), np.float32(-1.0)
    d[4, 5, :] = -np.inf
    d[5, 5, 3] = np.float32(np.nan)
    _, ok = pack(d.reshape(6, 1200))
    assert ok.tolist() == [False, True, True, False, False, False]
    nan_a = np.array([0x7fc00000], dtype=np.uint32).view(np.float32)[0]
    e = column_constant(307, 1).reshape(1, 60, 20)
    e[0, 0, :] = nan_a                     # bit-equal NaNs are still not a finite value
    assert not pack(e.reshape(1, 1200))[1][0]


def test_norms_follow_the_accumulator_order():
    rng = np.random.default_rng(9)
    d = rng.uniform(0.1, 9.0, (50, 1200)).astype(np.float32)
    got = column_norms(d)
    x = d.reshape(50, 60, 20).astype(np.float64)
    want = np.empty((50, 60))
    for e in range(50):
        for c in range(60):
            a = [0.0, 0.0, 0.0, 0.0]
            for r in range(20):
                a[r % 4] = a[r % 4] + x[e, c, r] * x[e, c, r]
            want[e, c] = np.sqrt((a[0] + a[2]) + (a[1] + a[3]))
    assert np.array_equal(got, want)


# ---- the device's image ----

@pytest.fixture(scope="module")
def sc():
    from navtech_radar_slam_amd import _rsx, scancontext
    assert _rsx.device_count() >= 1, "no HIP device: GPU tests must run on the MI355X box"
    assert _rsx.PACKED_COL_DTYPE == PACKED
    return scancontext


def same_bytes(a, b):
    return np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.gpu
def test_export_equals_the_packer(sc):
    good, bad = packable_fixture(), unpackable_fixture()
    descs = np.concatenate([good[:50], bad[:2], good[50:], bad[2:]])
    rec, ok = pack(descs)
    assert int((~ok).sum()) == 4
    g = sc.SCManager()
    try:
        g.add_descriptors_f32(good[:7])
        assert g.rescore_form() == (1, 0)
        assert same_bytes(g.packed_export(), rec[:7])
        g.add_descriptors_f32(descs[7:])
        got = g.packed_export()
        assert got.shape == rec.shape and same_bytes(got[ok], rec[ok])
        assert g.rescore_form() == (0, 4), "the planted unpackable entries, and the generic form because of them"
        assert same_bytes(g.packed_export(50, 3)[2:], rec[52:53])
    finally:
        g.close()


@pytest.mark.gpu
def test_growth_keeps_the_image(sc):
    """1024 -> 2048 entries: the array grows with the other images, with a copy"""
    descs = np.concatenate([synth.random_descriptors(311, 600, binary=True), column_constant(312, 500)])
    rec, ok = pack(descs)
    assert ok.all()
    g = sc.SCManager(capacity_hint=1024)
    try:
        g.add_descriptors_f32(descs[:1000])
        assert same_bytes(g.packed_export(), rec[:1000])
        g.add_descriptors_f32(descs[1000:])      # past the capacity
        assert g.local_size == 1100
        assert same_bytes(g.packed_export(), rec)
        assert g.rescore_form() == (1, 0)
    finally:
        g.close()


@pytest.mark.gpu
def test_insert_kernel_fills_the_image(sc):
    """the one-launch insert (rsx_sc_add_points): z = 0 clouds give column-constant descriptors; a cloud with heights does not"""
    clouds, _ = synth.keyframe_clouds(321, 12, binary_z=True, loop_frac=0.0, n_points=400)
    tall, _ = synth.keyframe_clouds(322, 1, binary_z=False, loop_frac=0.0, n_points=400)
    g = sc.SCManager()
    try:
        for c in clouds:
            g.makeAndSaveScancontextAndKeys(c)
        descs = g.export_descriptors_f32()
        rec, ok = pack(descs)
        assert ok.all() and (rec["bits"] != 0).any()
        assert same_bytes(g.packed_export(), rec)
        g.makeAndSaveScancontextAndKeys(tall[0])
        rec1, ok1 = pack(g.export_descriptors_f32(12, 1))
        assert not ok1[0], "the fixture's cloud with heights came out column-constant"
        assert same_bytes(g.packed_export(0, 12), rec)
        g.query(descs[:1], k=1)                  # a host-buffer entry: it synchronises and reads the counter back
        assert g.rescore_form() == (0, 1)
    finally:
        g.close()
