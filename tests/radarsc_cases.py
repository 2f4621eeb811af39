"""The place-recognition case the radar scan-context tests share (tests/test_radarsc_restatement.py on the CPU,
tests/test_gpu_sc_polar.py on the GPU): a database of 40 synthetic scans and four revisits, each one a database scan rolled in
azimuth (a pure sensor rotation) under a fresh speckle realisation.  A roll of s rows of the 400-row, 0.9 degree grid is s * 0.9
degrees = s * 0.15 sectors; the pair function searches whole sectors, so the expected shift is that rounded: 3, 30, 58, 1."""
import functools

import numpy as np

from navtech_radar_slam_amd import synth

N_DB = 40
REVISITS = ((4, 20, 3), (17, 200, 30), (33, 387, 58), (9, 7, 1))   # (database scan, rows rolled, expected shift)


@functools.lru_cache(maxsize=1)
def scans():
    """-> (db images (40, 400, 3371) uint8, query images (4, 400, 3371) uint8, azimuths (400,) float32); read-only."""
    db, az = [], None
    for i in range(N_DB):
        img, az, _ = synth.polar_image(100 + i)
        db.append(img)
    q = [synth.polar_image(100 + idx, shift_rows=s, noise_seed=900 + j)[0] for j, (idx, s, _) in enumerate(REVISITS)]
    db, q = np.stack(db), np.stack(q)
    db.setflags(write=False)
    q.setflags(write=False)
    az.setflags(write=False)
    return db, q, az


def check_ranking(hits):
    """hits: (4, k >= 2) records of the four revisits against the database: hit 0 is the revisited scan at the expected shift,
    strictly closer than hit 1."""
    for j, (idx, _, shift) in enumerate(REVISITS):
        assert hits[j][0]["index"] == idx and hits[j][0]["shift"] == shift, (j, hits[j])
        assert hits[j][0]["dist"] < hits[j][1]["dist"], (j, hits[j])
