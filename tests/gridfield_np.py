"""numpy restatement of the likelihood field of the grid map (include/rsx.h, rsx_gridmap_likelihood_field and
rsx_gridmap_field_gaussian_table): the arithmetic contract of csrc/gridfield.hip.  None of this is in the reference checkout -- parity
unpinned.  An exact Euclidean distance transform truncated at a radius, from the cells at or above a threshold, and a table from the
squared distance to the byte.  Integers throughout: the device's plane equals field() byte for byte.

The plane L is uint8 [height][width] (row = y); the parameters are a dict (threshold, radius); the table is uint8 [radius^2 + 1]."""
import numpy as np

DEFAULTS = dict(threshold=50, radius=12)
DEFAULT_SIGMA, DEFAULT_PEAK = 3.0, 255          # of the table that the entry makes when it is given none
MAX_RADIUS = 64
PARAMS = np.dtype([("threshold", np.int32), ("radius", np.int32), ("reserved0", np.int32), ("reserved1", np.int32)])   # rsx_gridmap_field_params, 16 bytes


def params(**kw):
    p = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in p:
            raise TypeError("no parameter " + k)
        p[k] = v
    return p


def gaussian_unrounded(sigma, radius, peak=255):
    """float64 [radius^2 + 1]: peak exp(-q / (2 sigma^2)), the exponent formed as -q / ((2.0 sigma) sigma)"""
    q = np.arange(radius * radius + 1, dtype=np.float64)
    sigma = np.float64(sigma)
    return np.float64(peak) * np.exp(-q / ((np.float64(2.0) * sigma) * sigma))


def gaussian_table(sigma, radius, peak=255):
    """uint8 [radius^2 + 1]: floor(peak exp(-q / (2 sigma^2)) + 0.5)"""
    return np.floor(gaussian_unrounded(sigma, radius, peak) + 0.5).astype(np.uint8)


def nearest(L, fp):
    """-> (q int32 [height][width], found bool [height][width]): the smallest dx dx + dy dy over the seeds (bytes >= threshold) with
    dx dx + dy dy <= radius^2, and whether there is one (q is 0 where there is none).  Separable: first the distance to the nearest
    seed along the row, then the minimum over the rows of dy dy plus its square"""
    L = np.asarray(L, dtype=np.uint8)
    H, W = L.shape
    R = int(fp["radius"])
    big = np.int32(1 << 20)
    seeds = np.zeros((H + 2 * R, W + 2 * R), dtype=bool)          # (nothing outside the map is a seed)
    seeds[R:R + H, R:R + W] = L >= fp["threshold"]
    along = np.full((H + 2 * R, W), big, dtype=np.int32)          # squared distance along the row, rows of the halo included
    for dx in range(R, -1, -1):
        hit = seeds[:, R + dx:R + dx + W] | seeds[:, R - dx:R - dx + W]
        along[hit] = dx * dx
    q = np.full((H, W), big, dtype=np.int32)
    for dy in range(-R, R + 1):
        np.minimum(q, along[R + dy:R + dy + H] + np.int32(dy * dy), out=q)
    found = q <= R * R
    return np.where(found, q, 0).astype(np.int32), found


def field(L, table, fp):
    """the transformed plane, uint8 [height][width]: table[q] where a seed lies within the radius, 0 elsewhere"""
    table = np.asarray(table, dtype=np.uint8)
    assert table.shape == (int(fp["radius"]) ** 2 + 1,)
    q, found = nearest(L, fp)
    return np.where(found, table[q], 0).astype(np.uint8)


def nearest_brute(L, fp):
    """the same by the rule as it is written: for every cell the minimum over every seed within the disc"""
    L = np.asarray(L, dtype=np.uint8)
    H, W = L.shape
    r2 = int(fp["radius"]) ** 2
    sy, sx = np.nonzero(L >= fp["threshold"])
    q, found = np.zeros((H, W), dtype=np.int32), np.zeros((H, W), dtype=bool)
    for y in range(H):
        for x in range(W):
            d2 = (sx - x) ** 2 + (sy - y) ** 2
            d2 = d2[d2 <= r2]
            if len(d2):
                q[y, x], found[y, x] = d2.min(), True
    return q, found
