"""The restatement of k-strongest keypoint extraction (tests/kstrongest_np.py, the contract of csrc/kstrongest.hip) against
the rule taken literally, one bin at a time in plain Python (sort every candidate key of the row, take k), and the
properties that follow from the rule.  CPU only."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kstrongest_np as ks  # noqa: E402


def brute_row(v, k, z_min, min_range, max_range, s):
    """-> (the row's keypoints ascending, every candidate bin)"""
    v = [int(x) for x in v]
    cols = len(v)
    hi = cols if max_range == 0 else min(max_range, cols)
    key = [(v[j] << 16) | (0xFFFF - j) for j in range(cols)]
    cand = []
    for j in range(cols):
        win = max(key[i] for i in range(max(0, j - s), min(cols - 1, j + s) + 1))
        if key[j] == win and v[j] >= z_min and min_range <= j < hi:
            cand.append(j)
    best = sorted(cand, key=lambda j: key[j], reverse=True)[:k]
    return sorted(best), cand


def adversarial_rows(rng):
    rows = []
    for cols in (1, 2, 3, 30, 67, 130, 257):
        rows.append(np.zeros(cols, dtype=np.uint8))
        rows.append(np.full(cols, 200, dtype=np.uint8))
        rows.append(np.full(cols, 255, dtype=np.uint8))
        rows.append(rng.integers(0, 256, size=cols).astype(np.uint8))
        rows.append(rng.choice(np.array([59, 60], dtype=np.uint8), size=cols))          # two levels around the floor
        rows.append(rng.choice(np.array([90, 180], dtype=np.uint8), size=cols, p=[0.3, 0.7]))  # far more than k at the top level
        rows.append((np.arange(cols) % 256).astype(np.uint8))                            # ascending: every bin beaten from the right
        rows.append((255 - np.arange(cols) % 256).astype(np.uint8))                      # descending
        plateau = rng.gamma(2.0, 14.0, size=cols).clip(0, 255).astype(np.uint8)
        plateau[cols // 3:cols // 3 + 9] = 220                                           # a run of equal strong bins
        plateau[-1] = 255
        plateau[0] = 255
        rows.append(plateau)
    return rows


PARAMS = [(k, z, mr, xr, s) for k in (1, 3, 12, 128) for z in (0, 60, 255) for mr, xr in ((0, 0), (2, 0), (5, 20), (300, 0)) for s in (0, 1, 5, 32)]


def test_restatement_equals_the_rule_taken_literally():
    rng = np.random.default_rng(5)
    rows = adversarial_rows(rng)
    for i, v in enumerate(rows):
        for k, z, mr, xr, s in PARAMS[i % 3::3]:
            want, _ = brute_row(v, k, z, mr, xr, s)
            got = ks.extract_row(v, k=k, z_min=z, min_range=mr, max_range=xr, min_separation=s)
            assert got.tolist() == want, (i, len(v), k, z, mr, xr, s)


def test_properties_on_random_rows():
    rng = np.random.default_rng(6)
    for trial in range(60):
        cols = int(rng.integers(1, 400))
        v = rng.gamma(2.0, 20.0, size=cols).clip(0, 255).astype(np.uint8)
        if trial % 3 == 0:
            v = (v // 32 * 32).astype(np.uint8)  # few levels: ties everywhere
        k, z, mr, xr, s = PARAMS[int(rng.integers(0, len(PARAMS)))]
        got = ks.extract_row(v, k=k, z_min=z, min_range=mr, max_range=xr, min_separation=s).tolist()
        want, cand = brute_row(v, k, z, mr, xr, s)
        assert got == want
        assert len(got) == min(k, len(cand)) <= k
        assert all(b > a for a, b in zip(got, got[1:]))              # strictly ascending
        assert all(b - a > s for a, b in zip(got, got[1:]))          # more than s bins apart
        assert set(got) <= set(cand)
        key = ks.row_keys(v)
        rest = [j for j in cand if j not in set(got)]
        if rest and got:
            assert max(int(key[j]) for j in rest) < min(int(key[j]) for j in got)


def test_image_layout_and_defaults():
    rng = np.random.default_rng(7)
    img = rng.gamma(2.0, 25.0, size=(5, 11 + 300)).clip(0, 255).astype(np.uint8)
    img[:, :11] = 255  # metadata: never seen
    tg = ks.extract(img)
    assert tg.dtype == np.int32 and tg.shape[1] == 2
    flat = [(int(a), int(r)) for a, r in tg]
    assert flat == sorted(flat)  # row-major
    for a in range(5):
        want, _ = brute_row(img[a, 11:], 12, 60, 58, 0, 5)
        assert tg[tg[:, 0] == a][:, 1].tolist() == want
    assert len(ks.extract(np.zeros((3, 50), dtype=np.uint8), col_offset=0)) == 0


@pytest.mark.parametrize("s", [0, 1, 5])
def test_plain_rule_picks_adjacent_bins_and_separation_does_not(s):
    v = np.full(200, 10, dtype=np.uint8)
    v[100:112] = 230  # one strong reflector, 12 bins wide
    got = ks.extract_row(v, k=12, z_min=60, min_range=0, min_separation=s).tolist()
    assert got == (list(range(100, 112)) if s == 0 else [100])
