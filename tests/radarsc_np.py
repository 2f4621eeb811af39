"""numpy restatement of the radar scan-context builder (csrc/radarsc.hip, include/rsx.h rsx_radarsc_*): the ARITHMETIC CONTRACT
of the kernel.  The descriptor is the "radar scan context" of the MulRan paper (Kim et al., ICRA 2020): the 20 x 60 polar grid
of Scancontext.cpp:151-195 filled with received power from the polar image.  MulRan's own builder is not part of the reference
checkout, so PARITY WITH IT IS UNPINNED; what is pinned here is the rule:

  ring of range bin j (SC.cpp:175,178, fp64)   r = (j + 0.5) * (double)resolution; none if j < min_range or r > max_radius,
                                               else max(min(20, (int)ceil(r / max_radius * 20)), 1) - 1
  sector of azimuth row a (SC.cpp:179, fp64)   th = (double)az[a] * 57.29577951308232, t = th / 360 - floor(th / 360),
                                               max(min(60, (int)ceil(t * 60)), 1) - 1; none if az[a] is not finite
  sample                                       v = max(p - power_floor, 0), integers
  cell                                         MEAN: (float)((double)sum / (double)count), 0 when empty; MAX: (float)max, 0 when empty

Sums are integers, so a cell does not depend on the order of its samples: the kernel must match bit for bit.
Output: float32 [n][60][20] (sector-major: element (ring r, sector s) at [s * 20 + r])."""
import numpy as np

MEAN, MAX = 0, 1
NUM_RING, NUM_SECTOR = 20, 60
DEFAULTS = dict(resolution=0.0595, max_radius=80.0, min_range=58, power_floor=0, stat=MEAN)


def ring_of_bins(cols, resolution=0.0595, max_radius=80.0, min_range=58):
    """-> int64 [cols]: the ring of every range bin, -1 where there is none."""
    j = np.arange(cols, dtype=np.float64)
    r = (j + 0.5) * np.float64(np.float32(resolution))
    with np.errstate(over="ignore", invalid="ignore"):
        ring = np.maximum(np.minimum(20, np.ceil(r / np.float64(max_radius) * 20.0)), 1).astype(np.int64) - 1
    ring[(np.arange(cols) < min_range) | (r > np.float64(max_radius))] = -1
    return ring


def sector_of_rows(az):
    """-> int64 [rows]: the sector of every azimuth row, -1 where the azimuth is not finite."""
    az = np.asarray(az, dtype=np.float32)
    ok = np.isfinite(az)
    th = np.where(ok, az, np.float32(0)).astype(np.float64) * 57.29577951308232
    q = th / 360.0
    t = q - np.floor(q)
    sec = np.maximum(np.minimum(60, np.ceil(t * 60.0)), 1).astype(np.int64) - 1
    sec[~ok] = -1
    return sec


def build(img, az, col_offset=11, cols=None, resolution=0.0595, max_radius=80.0, min_range=58, power_floor=0, stat=MEAN):
    """img: (rows, row_stride) uint8 with the samples at [col_offset, col_offset + cols); az: (rows,) float32 rad.
    -> (1200,) float32."""
    img = np.asarray(img, dtype=np.uint8)
    if cols is None:
        cols = img.shape[1] - col_offset
    v = np.maximum(img[:, col_offset:col_offset + cols].astype(np.int64) - int(power_floor), 0)
    ring = ring_of_bins(cols, resolution, max_radius, min_range)
    sec = sector_of_rows(az)
    cell = sec[:, None] * NUM_RING + ring[None, :]
    use = (sec[:, None] >= 0) & (ring[None, :] >= 0)
    flat, vals = cell[use], v[use]
    count = np.bincount(flat, minlength=NUM_RING * NUM_SECTOR)
    if stat == MAX:
        out = np.zeros(NUM_RING * NUM_SECTOR, dtype=np.int64)
        np.maximum.at(out, flat, vals)
        return out.astype(np.float32)
    total = np.zeros(NUM_RING * NUM_SECTOR, dtype=np.int64)
    np.add.at(total, flat, vals)
    out = np.zeros(NUM_RING * NUM_SECTOR, dtype=np.float32)
    nz = count > 0
    out[nz] = (total[nz].astype(np.float64) / count[nz].astype(np.float64)).astype(np.float32)
    return out


def build_batch(imgs, az, **kw):
    """imgs: (n, rows, row_stride); az: (rows,) shared or (n, rows).  -> (n, 1200) float32."""
    az = np.asarray(az, dtype=np.float32)
    return np.stack([build(im, az[i] if az.ndim == 2 else az, **kw) for i, im in enumerate(imgs)]) if len(imgs) else \
        np.zeros((0, NUM_RING * NUM_SECTOR), dtype=np.float32)


def build_naive(img, az, col_offset, cols, resolution, max_radius, min_range, power_floor, stat):
    """The same rule as a deliberately naive triple loop in Python scalars (what tests/test_radarsc_restatement.py compares
    build() with)."""
    import math
    total = [[0] * NUM_RING for _ in range(NUM_SECTOR)]
    count = [[0] * NUM_RING for _ in range(NUM_SECTOR)]
    peak = [[0] * NUM_RING for _ in range(NUM_SECTOR)]
    res = float(np.float32(resolution))
    for a in range(img.shape[0]):
        azf = float(np.float32(az[a]))
        if not math.isfinite(azf):
            continue
        th = azf * 57.29577951308232
        t = th / 360 - math.floor(th / 360)
        s = max(min(60, int(math.ceil(t * 60))), 1) - 1
        for j in range(cols):
            r = (j + 0.5) * res
            if j < min_range or r > max_radius:
                continue
            k = max(min(20, int(math.ceil(r / max_radius * 20))), 1) - 1
            v = max(int(img[a, col_offset + j]) - power_floor, 0)
            total[s][k] += v
            count[s][k] += 1
            peak[s][k] = max(peak[s][k], v)
    out = np.zeros((NUM_SECTOR, NUM_RING), dtype=np.float32)
    for s in range(NUM_SECTOR):
        for k in range(NUM_RING):
            if stat == MAX:
                out[s, k] = np.float32(peak[s][k])
            elif count[s][k]:
                out[s, k] = np.float32(float(total[s][k]) / float(count[s][k]))
    return out.reshape(-1)
