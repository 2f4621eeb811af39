"""csrc/rsx_wave_dev.h, primitive by primitive, against numpy restatements of its documented orders -- bit for bit.

rsx_selftest_wave (include/rsx_diag.h) runs every primitive of the header on caller-given lane values in one launch of one
wavefront and returns what each lane ends with.  The restatements below are written from the header's comments, not from its
code: the row tree is lane l with l ^ 1, then l ^ 2, then its half's mirror, then its row's mirror; the float sums are
spelled out addition by addition in the order their name says (never np.sum).  A lane's 64-bit pattern is seen as u64, as f64
(its bits), as u32 / i32 (the low word) and as f32 (the bits of the HIGH word); no view of any case holds a NaN, an infinity
or an f32 denormal, because the primitives document that they assume no NaN."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NPRIM = 20
L = np.arange(64)
EDGES = (0, 15, 16, 31, 32, 47, 48, 63)  # the row edges, where the DPP steps and the readlanes meet


# ---- the views ----
def f64_of(u):
    return u.view(np.float64)


def lo_of(u):
    return (u & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def f32_of(u):
    return (u >> np.uint64(32)).astype(np.uint32).view(np.float32)


def bits64(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def bits32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)


# ---- the header's orders, restated ----
def row_tree(x, op):
    """every lane: op over its row of 16 -- with lane ^ 1, lane ^ 2, the mirror of its half of 8, the mirror of its row"""
    for partner in (L ^ 1, L ^ 2, (L & ~7) | (7 - (L & 7)), (L & ~15) | (15 - (L & 15))):
        x = op(x, x[partner])
    return x


def rows_seq(x, op):
    return op(op(op(x[0], x[16]), x[32]), x[48])


def rows_pair(x, op):
    return op(op(x[0], x[16]), op(x[32], x[48]))


def butterfly(x, op):
    for off in (32, 16, 8, 4, 2, 1):
        x = op(x, x[L ^ off])
    return x


def add(a, b):
    return a + b  # one IEEE addition per element (numpy does not fuse or reassociate)


def min_f32(a, b):
    """v_min_f32: -0.0 is below +0.0"""
    a, b = np.float32(a), np.float32(b)
    if a == b:
        return a if np.signbit(a) else b
    return a if a < b else b


def sum_f32_bcast(f):
    r = row_tree(f, add)
    r0, r1, r2, r3 = r[0], r[16], r[32], r[48]
    return (r3 + r2) + (r1 + r0)  # lane 63: row 3 += row 2 (row_bcast:15), then += the last lane of row 1 = r1 + r0


def expected(u):
    """[NPRIM][64] uint64: what rsx_selftest_wave documents for one case"""
    d, lo, f = f64_of(u), lo_of(u), f32_of(u)
    i32 = lo.view(np.int32)
    e = np.zeros((NPRIM, 64), dtype=np.uint64)
    e[0] = lo[L ^ 1]
    e[1] = np.concatenate([[np.uint64(0)], u[:63]])
    e[2] = np.concatenate([u[1:], [np.uint64(0)]])
    bc = np.zeros(64, dtype=np.uint64)
    hi = u >> np.uint64(32)
    bc[16:32] = hi[15]
    bc[48:64] = hi[47]
    e[3] = bc
    e[4] = u[37]
    e[5] = np.uint64(int(i32.astype(np.int64).sum()) & 0xFFFFFFFF)
    e[6] = np.uint64(int(i32.max()) & 0xFFFFFFFF)
    e[7] = lo.max()
    e[8] = u.min()
    e[9] = u.max()
    mn = f[0]
    for x in f[1:]:
        mn = min_f32(mn, x)  # (a minimum under a total order: any tree gives the same)
    e[10] = bits32(mn)[()]
    e[11] = bits64(rows_seq(row_tree(d, add), add))[()]
    e[12] = bits64(rows_pair(row_tree(d, add), add))[()]
    e[13] = bits32(sum_f32_bcast(f))[()]
    e[14] = bits64(butterfly(d, add))
    e[15] = u.max()
    e[16] = np.cumsum(lo.astype(np.uint64)) & np.uint64(0xFFFFFFFF)
    e[17] = np.maximum.accumulate(lo)
    e[18] = bits64(np.maximum.accumulate(np.abs(d)))
    e[19] = bits64(np.maximum.accumulate(np.abs(d)[::-1])[::-1])
    return e


# ---- the cases ----
def from_f64(values):
    return bits64(np.asarray(values, dtype=np.float64)).copy()


def packed(f32_values, u32_values):
    """f32 view = f32_values, u32 / i32 view = u32_values"""
    hi = bits32(np.asarray(f32_values, dtype=np.float32))
    return (hi << np.uint64(32)) | np.asarray(u32_values, dtype=np.uint64)


def order_cases():
    """rows whose sums are 1e16, 1, -1e16, 1 in some arrangement: ((r0 + r1) + r2) + r3, (r0 + r1) + (r2 + r3) and the xor
    ladder (which adds row 0 to row 2 and row 1 to row 3 first) give three different doubles"""
    out = []
    for lanes in ((0, 16, 32, 48), (5, 21, 37, 53), (15, 31, 47, 63), (3, 30, 33, 60)):
        v = np.zeros(64)
        v[list(lanes)] = (1e16, 1.0, -1e16, 1.0)
        out.append(from_f64(v))
    return out


def make_cases():
    rng = np.random.default_rng(20261019)
    cases = []
    # all lanes equal
    cases += [from_f64(np.full(64, 3.0)), from_f64(np.zeros(64)), packed(np.full(64, -2.5), np.full(64, 0x80000007))]
    # one extreme at a row edge: a maximum among doubles, a minimum in the packed views
    for edge in EDGES:
        v = np.full(64, 1.0) + L * 2.0 ** -20
        v[edge] = 1.0e6
        cases.append(from_f64(v))
    for edge in EDGES:
        fv, iv = np.full(64, 4.0, dtype=np.float32) + L.astype(np.float32), (1000 + L).astype(np.uint64)
        fv[edge], iv[edge] = -1.0e6, 0x80000000  # the smallest f32, the smallest i32 (and the largest u32)
        cases.append(packed(fv, iv))
    # alternating signs, lane by lane and row by row
    cases.append(from_f64(np.where(L % 2 == 0, 1.0, -1.0) * (1.0 + L / 7.0)))
    cases.append(packed(np.where((L // 16) % 2 == 0, 1.5, -1.5) * (1.0 + L), np.where(L % 2 == 0, 5 + L, 0xFFFFFFF0 - L)))
    cases += order_cases()
    # ties for the u64 minimum and maximum, in several rows
    t = from_f64(2.0 + L)
    t[[3, 19, 62]] = from_f64([1.0])[0]
    t[[0, 31, 32]] = from_f64([-1.0])[0]  # (sign bit: the largest patterns)
    cases.append(t)
    cases.append(packed(np.where(L % 5 == 0, 9.0, 1.0), np.where(L % 3 == 0, 77, 11)))
    # -0.0 against +0.0 for min_f32 (all other lanes positive)
    for neg in ((0,), (63,), (16, 40)):
        fv = np.where(L % 4 == 1, 0.0, 1.0 + L).astype(np.float32)
        fv[list(neg)] = -0.0
        cases.append(packed(fv, L))
    # scans: monotone, reversed, one spike
    cases.append(packed(1.0 + L, 3 + 1000003 * L))
    cases.append(packed(64.0 - L, 3 + 1000003 * (63 - L)))
    for spike in (0, 17, 63):
        fv, iv = np.full(64, 1.0, dtype=np.float32), np.full(64, 2, dtype=np.uint64)
        fv[spike], iv[spike] = 1.0e5, 0xFFFFFFF0  # (the running sum wraps past 2^32)
        cases.append(packed(fv, iv))
    # seeded noise in every view
    for _ in range(5):
        cases.append(packed(rng.uniform(-1e3, 1e3, 64), rng.integers(0, 1 << 32, 64, dtype=np.uint64)))
    cases = np.stack(cases)
    d, f = f64_of(cases.reshape(-1)), f32_of(cases.reshape(-1))
    assert np.all(np.abs(d) < 1e300) and np.all(np.abs(f) < 1e30), "a NaN, an infinity, or a sum that could overflow"
    assert np.all((f == 0) | (np.abs(f) >= np.finfo(np.float32).tiny)), "an f32 denormal"
    return cases


@pytest.fixture(scope="module")
def cases():
    return make_cases()


def test_the_three_f64_sum_orders_are_told_apart():
    """on the order cases the three restatements disagree pairwise, so a primitive that took another's order would fail below"""
    for u in order_cases():
        d = f64_of(u)
        seq, pair, bfly = rows_seq(row_tree(d, add), add), rows_pair(row_tree(d, add), add), butterfly(d, add)[0]
        assert len({float(seq), float(pair), float(bfly)}) == 3, (seq, pair, bfly)


def test_every_primitive_matches_its_documented_order(cases):
    from navtech_radar_slam_amd import _rsx
    assert _rsx.device_count() >= 1, "no HIP device: GPU tests must run on the MI355X box"
    assert 35 <= len(cases) <= 45
    out = np.zeros((len(cases), NPRIM, 64), dtype=np.uint64)
    st = _rsx.lib().rsx_selftest_wave(0, C.c_void_p(cases.ctypes.data), C.c_int32(len(cases)), C.c_void_p(out.ctypes.data))
    assert st == 0, _rsx.lib().rsx_last_error_string()
    bad = []
    for c, u in enumerate(cases):
        want = expected(u)
        for p in range(NPRIM):
            if not np.array_equal(out[c, p], want[p]):
                lane = int(np.flatnonzero(out[c, p] != want[p])[0])
                bad.append((c, p, lane, hex(int(out[c, p, lane])), hex(int(want[p, lane]))))
    assert not bad, "(case, primitive, first lane, got, want): " + str(bad[:12]) + f" ... {len(bad)} in all"
