#!/usr/bin/env python3
"""Time the radar grid map (rsx_gridmap_add_batch_device): 64 scans per call, the scans being consecutive 400 x 3360 scans of the
synthetic drive at their true poses, all resident in HBM, into the default map (1024 x 1024 cells of 0.5 m, centred on the drive).
128 distinct scans (172 MB of polar images) so that a sweep does not live in the Infinity Cache.  Prints microseconds per scan, cell
observations per second and the bytes of the planes a call moves against the HBM peak.  No earlier GPU form exists to compare with.

usage: bench_gridmap.py [n_scans=128] [reps=7]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from navtech_radar_slam_amd import coral, gridmap, synth  # noqa: E402

n_scans = int(sys.argv[1]) if len(sys.argv) > 1 else 128
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
batch = 64
n_calls = n_scans // batch
assert n_calls >= 2, "at least 128 scans: two calls of 64"
HBM_PEAK = 8.0e12  # bytes / s, MI355X

import torch  # noqa: E402

imgs, _, poses, _ = synth.polar_sequence(11, n_scans)
centre = poses[:n_calls * batch, :2].mean(axis=0)
p = gridmap.default_params()
p.origin_x, p.origin_y = float(centre[0]) - 0.5 * p.width * p.resolution, float(centre[1]) - 0.5 * p.height * p.resolution
h = gridmap.GridMap(400, 3360, p)
T = coral.pose_matrices(poses)
calls = [dict(imgs=torch.from_numpy(np.ascontiguousarray(imgs[c * batch:(c + 1) * batch])).cuda(),
              tf=torch.from_numpy(np.ascontiguousarray(T[c * batch:(c + 1) * batch])).cuda()) for c in range(n_calls)]
stream = torch.cuda.current_stream().cuda_stream
print(f"{n_calls * batch} distinct scans, {n_calls} calls of {batch}, map {p.width} x {p.height} cells of {p.resolution} m, range_halfwidth {p.range_halfwidth}")


def sweep():
    t0 = time.perf_counter()
    for c in calls:
        h.add_device(c["imgs"], c["tf"], stream=stream)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


sweep()  # warm-up
h.clear(stream)
sweep()
_, cnt, _ = h.read()
observations = int(cnt.astype(np.int64).sum())   # (scan, cell) pairs of one sweep
touched = int(np.count_nonzero(cnt.reshape(p.height // 32, 32, p.width // 32, 32).sum(axis=(1, 3))))
ts = [sweep() for _ in range(reps)]
dt = float(np.median(ts))
scans = n_calls * batch
# a tile that meets a scan reads and writes its three planes once per call (a thread whose cells saw nothing skips its 16 bytes: an upper bound)
plane_bytes = touched * 32 * 32 * 4 * 3 * 2 * n_calls
print(f"gridmap add_batch_device ({batch} scans per call, {scans} distinct scans): {dt / scans * 1e6:.1f} us per scan "
      f"(median of {reps} sweeps; fastest {min(ts) / scans * 1e6:.1f}, slowest {max(ts) / scans * 1e6:.1f}), "
      f"{observations / dt / 1e9:.2f} G cell observations/s ({observations / scans:.0f} per scan)")
print(f"planes: {touched} of {p.width * p.height // 1024} tiles touched, {plane_bytes / n_calls / 1e6:.1f} MB read + written per call = "
      f"{plane_bytes / dt / 1e9:.1f} GB/s, {100.0 * plane_bytes / dt / HBM_PEAK:.2f} % of the {HBM_PEAK / 1e12:.0f} TB/s HBM peak; "
      f"polar images {scans * 400 * 3371 / dt / 1e9:.1f} GB/s if every byte were read once")
h.close()
