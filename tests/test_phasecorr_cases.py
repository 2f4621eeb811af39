"""tests/phasecorr_cases.py is what it claims to be, shown on tests/phasecorr_np.py alone (no GPU, no library): the cases reach the edges of
the peak arithmetic, the restatement recovers the pose truth on them, every decision the GPU comparison rests on (the two integer peaks, the
winning candidate, the three parabolas) is taken with a margin far above the device's round-off, and empty images give exact zeros."""
import math

import numpy as np
import pytest

import phasecorr_cases as pcc
import phasecorr_np as pcn
from phasecorr_cases import MARGIN, MIN_DENOM

DECIDED = [name for name, c in pcc.cases().items() if not c.empty]


def _decided_pairs():
    """(case, index, pair, restatement result, truth) of every pair that is neither empty nor marked ambiguous"""
    for name in DECIDED:
        c = pcc.cases()[name]
        for i, w in enumerate(pcc.expected(name)[0]):
            if i not in c.ambiguous:
                yield c, i, c.pairs[i], w, c.truth[i]


def test_the_case_list():
    cs = pcc.cases()
    assert list(cs) == ["s64", "s128", "s256", "s512", "s64-one", "s128-one", "s64-empty"]
    for name in ("s64", "s128", "s256"):
        assert cs[name].pairs == [(i, 0) for i in range(1, 7)] + [(0, i) for i in range(1, 7)] + [(0, 0)] and not cs[name].ambiguous
    assert len(cs["s512"].pairs) <= 3
    for c in cs.values():
        assert pcn.check_params(dict(pcn.default_params(), **c.fields), c.rows, c.cols) is None
        assert c.images.dtype == np.uint8 and c.images.shape[1:] == (c.rows, c.cols) and len(c.truth) == len(c.pairs)
    for name in ("s64-one", "s128-one"):
        c = cs[name]
        assert c.fields["resolve_half_turn"] == 0 and len(c.ambiguous) == 1
        for i, (tr, w) in enumerate(zip(c.truth, pcc.expected(name)[0])):
            assert (abs(tr[2]) > math.pi / 2) == (i in c.ambiguous) and w["other_peak"] is None and w["half_turn"] == 0
        (i,) = c.ambiguous
        assert abs(abs(c.truth[i][2]) - 2.8) < math.pi / c.rows
    # the motions the scans were drawn at are those of the list, the yaws at most half an azimuth row off
    for name, sh in pcc.SHAPES.items():
        for (x, y, yaw), (mx, my, myaw) in zip(pcc.poses(sh)[1:], pcc.MOTIONS):
            assert (x, y) == (mx * sh.fields["resolution"], my * sh.fields["resolution"]) and abs(yaw - myaw) <= (math.pi / sh.rows if sh.snap else 0.0)


def test_scans_and_packagings():
    for name, sh in pcc.SHAPES.items():
        s = pcc.scans(name)
        assert s.shape == (7, sh.rows, sh.cols) and s.max() == 255 and 8 < np.median(s) < 16     # blobs over a floor of mean 12
        assert not np.array_equal(s[0], s[1])
    imgs = pcc.scans("s64")[:3]
    buf, istride, rstride, off = pcc.pack(imgs, padded=False)
    assert (istride, rstride, off) == (37 * 97, 97, 0) and np.array_equal(buf.reshape(3, 37, 97), imgs)
    buf, istride, rstride, off = pcc.pack(imgs, padded=True)
    assert (istride, rstride, off) == (37 * (5 + 97 + 3) + 17, 5 + 97 + 3, 5) and len(buf) == 3 * istride
    view = pcc.unpack(buf, 3, 37, istride, rstride)
    assert np.array_equal(view[:, :, off:off + 97], imgs)
    assert (view[:, :, :off] == 0xA5).all() and (view[:, :, off + 97:] == 0xA5).all() and (buf.reshape(3, istride)[:, -17:] == 0xA5).all()
    assert int((buf == 0xA5).sum()) >= 3 * (37 * 8 + 17)
    # the restatement reads the same image through either packaging
    tab = pcn.Tables(dict(pcn.default_params(), **pcc.SHAPES["s64"].fields), 37, 97)
    assert np.array_equal(pcn.cart_image(view[1], off, tab), pcn.cart_image(imgs[1], 0, tab))


@pytest.mark.parametrize("name", list(pcc.DEGENERATE))
def test_degenerate_shapes_give_an_image(name):
    sh = pcc.DEGENERATE[name]
    p = dict(pcn.default_params(), **sh.fields)
    assert pcn.check_params(p, sh.rows, sh.cols) is None
    tab = pcn.Tables(p, sh.rows, sh.cols)
    for img in pcc.degenerate_scans(name):
        cart = pcn.cart_image(img, 0, tab)
        assert cart.max() > 0.0 and np.isfinite(cart).all()


def test_edges_are_reached():
    """the union of the cases: the integer translation peak on the first and last row and column, both signs of both shifts, both
    candidates winning, the rotation peak on both sides of N / 2"""
    seen = set()
    for c, i, pair, w, _ in _decided_pairs():
        n = c.fields["n"]
        i0, j0 = w["peak_ij"]
        seen |= {("i0", {0: "0", n - 1: "N-1"}.get(i0)), ("j0", {0: "0", n - 1: "N-1"}.get(j0))}
        seen |= {("is", "-" if i0 >= n // 2 else "+" if i0 else "0"), ("js", "-" if j0 >= n // 2 else "+" if j0 else "0")}
        seen |= {("both signs", (i0 >= n // 2) != (j0 >= n // 2) and i0 != 0 and j0 != 0), ("half_turn", w["half_turn"]), ("k0 low", 0 < w["rot_k0"] < n // 2),
                 ("k0 high", w["rot_k0"] >= n // 2), ("n", n)}
    for want in [("i0", "0"), ("i0", "N-1"), ("j0", "0"), ("j0", "N-1"), ("is", "-"), ("is", "+"), ("js", "-"), ("js", "+"), ("both signs", True),
                 ("half_turn", 0), ("half_turn", 1), ("k0 low", True), ("k0 high", True), ("n", 64), ("n", 128), ("n", 256), ("n", 512)]:
        assert want in seen, want
    # and per transform length below 512: all four quadrants and all four borders
    for name in ("s64", "s128", "s256"):
        n = pcc.cases()[name].fields["n"]
        ij = [w["peak_ij"] for w in pcc.expected(name)[0]]
        assert {(i >= n // 2, j >= n // 2) for i, j in ij if i or j} == {(False, False), (False, True), (True, False), (True, True)}, name
        assert {0, n - 1} <= {i for i, _ in ij} and {0, n - 1} <= {j for _, j in ij}, name
        assert {w["half_turn"] for w in pcc.expected(name)[0]} == {0, 1}, name


def test_truth_is_recovered():
    """within one pixel and one angle bin (pi / N): the method's quantisation"""
    for c, i, pair, w, tr in _decided_pairs():
        n, pix = c.fields["n"], c.fields["resolution"]
        ex, ey, et = (w["x"] - tr[0]) / pix, (w["y"] - tr[1]) / pix, pcc._wrap(w["theta"] - tr[2]) / (math.pi / n)
        print(f"{c.name} {pair}: peak {w['peak_ij']} k0 {w['rot_k0']} half_turn {w['half_turn']}: {ex:+.3f} {ey:+.3f} px {et:+.3f} bins")
        assert abs(ex) <= 1.0 and abs(ey) <= 1.0 and abs(et) <= 1.0 and w["status"] == 0, (c.name, pair, ex, ey, et)


def test_margins():
    """no comparison with the device rests on a coin toss: a condition, not a measurement"""
    least = dict(surface=np.inf, curve=np.inf, candidate=np.inf, denominator=np.inf)
    for c, i, pair, w, _ in _decided_pairs():
        n = c.fields["n"]
        i0, j0 = w["peak_ij"]
        assert w["surface"][i0, j0] == w["surface"].max() and w["rot_curve"][w["rot_k0"]] == w["rot_curve"].max()
        ls, lc, dn = pcc.lead(w["surface"]), pcc.lead(w["rot_curve"]), min(pcc.denominators(w, n))
        least.update(surface=min(least["surface"], ls), curve=min(least["curve"], lc), denominator=min(least["denominator"], dn))
        assert ls >= MARGIN and lc >= MARGIN and dn >= MIN_DENOM, (c.name, pair, ls, lc, dn)
        if c.fields.get("resolve_half_turn", 1):
            lo = w["peak"] - w["other_peak"]
            least["candidate"] = min(least["candidate"], lo)
            assert lo >= MARGIN, (c.name, pair, lo)
    print("least margins:", least)
    # the pair marked ambiguous is: its only candidate is half a turn off and nothing stands out of its surface
    for name in ("s64-one", "s128-one"):
        (i,) = pcc.cases()[name].ambiguous
        assert pcc.expected(name)[0][i]["peak_ratio"] > 0.8


def test_empties():
    c = pcc.cases()["s64-empty"]
    assert c.empty and not c.images[0].any() and c.images[1].any()
    want, carts = pcc.expected("s64-empty")
    assert not carts[0].any() and carts[1].any()
    for w in want:
        assert all(w[f] == 0 for f in ("x", "y", "theta", "peak", "peak_ratio", "rot_peak", "half_turn", "status")), w
        assert w["peak_ij"] == (0, 0) and w["rot_k0"] == 0 and w["other_peak"] == 0.0
        assert not np.isnan(w["surface"]).any() and not np.isnan(w["rot_curve"]).any()
        assert not w["surface"].any() and not w["rot_curve"].any()
