#!/usr/bin/env python3
"""Time the correlative scan-to-map matching (rsx_gridmap_match_batch_device): 64 jobs per call, the clouds being the default
k-strongest clouds (4800 points) of consecutive 400 x 3360 scans of the synthetic drive, the map the default map (1024 x 1024 cells of
0.5 m, centred on the drive) built from the same scans at their true poses, its mean as the likelihood; K = U = V = 8 (4913 candidates
per job), angle_step 0.01; the priors are the true poses moved by up to 2 m and 0.04 rad, in four different ways that the 64 calls of a
sweep take in turn.  Everything is resident in HBM; the volume stays in the handle's workspace.  Prints microseconds per job and byte gathers per
second.  No earlier GPU form exists to compare with.

usage: bench_gridmatch.py [n_scans=64] [reps=7] [jobs_per_call=64]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from navtech_radar_slam_amd import coral, gridmap, kstrongest, synth  # noqa: E402
from navtech_radar_slam_amd._rsx import GRIDMAP_MATCH_RESULT_DTYPE  # noqa: E402

n_scans = int(sys.argv[1]) if len(sys.argv) > 1 else 64
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
batch, n_calls = int(sys.argv[3]) if len(sys.argv) > 3 else 64, 64
assert n_scans >= batch, "a job per scan: at least jobs_per_call scans"
K = U = V = 8

import torch  # noqa: E402

imgs, _, poses, _ = synth.polar_sequence(11, n_scans)
centre = poses[:, :2].mean(axis=0)
p = gridmap.default_params()
p.origin_x, p.origin_y = float(centre[0]) - 0.5 * p.width * p.resolution, float(centre[1]) - 0.5 * p.height * p.resolution
h = gridmap.GridMap(400, 3360, p)
for b0 in range(0, n_scans, batch):
    h.add(imgs[b0:b0 + batch], coral.pose_matrices(poses[b0:b0 + batch]))
h.update_likelihood()
lit = int(np.count_nonzero(h.likelihood()))

targets = kstrongest.KStrongest(400, 3360).extract_batch(imgs[:batch])
clouds = []
for tg in targets:   # (bin + 0.5) 0.0595 along 2 pi row / 400, fp64, rounded once
    rho, phi = (tg[:, 1].astype(np.float64) + 0.5) * synth.RADAR_RESOLUTION, tg[:, 0].astype(np.float64) * 2.0 * np.pi / 400.0
    clouds.append(np.stack([rho * np.cos(phi), rho * np.sin(phi)], axis=1).astype(np.float32))
offsets = np.zeros(batch + 1, dtype=np.int64)
offsets[1:] = np.cumsum([len(c) for c in clouds])
rng = np.random.default_rng(1)
d_xy, d_off = torch.from_numpy(np.concatenate(clouds)).cuda(), torch.from_numpy(offsets).cuda()
errors = [np.concatenate([rng.uniform(-2.0, 2.0, (batch, 2)), rng.uniform(-0.04, 0.04, (batch, 1))], axis=1) for _ in range(4)]
d_priors = [torch.from_numpy(coral.pose_matrices(poses[:batch] + e)).cuda() for e in errors]
d_res = [torch.zeros(batch * GRIDMAP_MATCH_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda") for _ in range(4)]
mp = gridmap.match_params(angle_steps=K, x_cells=U, y_cells=V, angle_step=0.01)
stream = torch.cuda.current_stream().cuda_stream
points = int(offsets[-1])
print(f"{batch} jobs per call, {n_calls} calls per sweep, {points / batch:.0f} points per job, K = U = V = {K}, map {p.width} x {p.height} cells of "
      f"{p.resolution} m from {n_scans} scans ({lit} cells lit)")


def sweep():
    t0 = time.perf_counter()
    for c in range(n_calls):
        h.match_device(d_xy, d_off, d_priors[c % 4], d_res[c % 4], params=mp, stream=stream)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


sweep()  # warm-up (grows the workspace)
sweep()
ts = [sweep() for _ in range(reps)]
dt = float(np.median(ts))
jobs = n_calls * batch
gathers = (2 * K + 1) * (2 * V + 1) * (2 * U + 1) * points * n_calls   # bytes of the plane that enter a score, per sweep
res = np.concatenate([r.cpu().numpy().view(GRIDMAP_MATCH_RESULT_DTYPE) for r in d_res])
err = np.concatenate(errors)
# how many jobs came back to within a cell and a step of the truth (the priors are off by whole metres, the window is 4 m and 0.08 rad wide)
back = int(np.count_nonzero((np.abs(res["u"] * p.resolution + err[:, 0]) <= p.resolution) & (np.abs(res["v"] * p.resolution + err[:, 1]) <= p.resolution)
                            & (np.abs(res["k"] * 0.01 + err[:, 2]) <= 0.01)))
jobs_seen = 4 * batch
print(f"gridmap match_batch_device ({batch} jobs per call): {dt / jobs * 1e6:.1f} us per job (median of {reps} sweeps; fastest "
      f"{min(ts) / jobs * 1e6:.1f}, slowest {max(ts) / jobs * 1e6:.1f}), {gathers / dt / 1e9:.1f} G byte gathers/s "
      f"({gathers / jobs / 1e6:.1f} M per job); {back} of {jobs_seen} distinct jobs within a cell and a step of the true pose, "
      f"status bits seen {int(np.bitwise_or.reduce(res['status']))}")
h.close()
