#!/usr/bin/env python3
"""Time the sub-cell refinement of a pose in the grid map (rsx_gridmap_refine_batch_device): 64 jobs per call, the clouds being the
default k-strongest clouds (4800 points) of consecutive 400 x 3360 scans of the synthetic drive, the map the default map (1024 x 1024
cells of 0.5 m, centred on the drive) built from the same scans at their true poses, its mean as the likelihood; the default parameters;
the priors are the true poses moved by up to half a cell (0.25 m) along x and y and half an angle step (0.005 rad), which is what
rsx_gridmap_match_* leaves, in four different ways that the 64 calls of a sweep take in turn.  Everything is resident in HBM.  Prints
microseconds per job, the mean evaluations per job and the median pose error before and after; and, timed in the same session as the
figure to read it against, rsx_gridmap_match_batch_device at its defaults on the same clouds.  With more jobs per call than scans, job i
takes the cloud and the pose of scan i % n_scans.  No earlier GPU form exists to compare with.

usage: bench_gridrefine.py [n_scans=64] [reps=7] [jobs_per_call=64]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from navtech_radar_slam_amd import coral, gridmap, kstrongest, synth  # noqa: E402
from navtech_radar_slam_amd._rsx import GRIDMAP_MATCH_RESULT_DTYPE, GRIDMAP_REFINE_RESULT_DTYPE  # noqa: E402

n_scans = int(sys.argv[1]) if len(sys.argv) > 1 else 64
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
batch, n_calls = int(sys.argv[3]) if len(sys.argv) > 3 else 64, 64
n_clouds = min(n_scans, batch)   # with more jobs per call than scans, job i takes the cloud and the pose of scan i % n_scans

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

targets = kstrongest.KStrongest(400, 3360).extract_batch(imgs[:n_clouds])
clouds = []
for tg in targets:   # (bin + 0.5) 0.0595 along 2 pi row / 400, fp64, rounded once
    rho, phi = (tg[:, 1].astype(np.float64) + 0.5) * synth.RADAR_RESOLUTION, tg[:, 0].astype(np.float64) * 2.0 * np.pi / 400.0
    clouds.append(np.stack([rho * np.cos(phi), rho * np.sin(phi)], axis=1).astype(np.float32))
clouds = [clouds[i % n_clouds] for i in range(batch)]
job_poses = poses[np.arange(batch) % n_clouds]
offsets = np.zeros(batch + 1, dtype=np.int64)
offsets[1:] = np.cumsum([len(c) for c in clouds])
rng = np.random.default_rng(1)
d_xy, d_off = torch.from_numpy(np.concatenate(clouds)).cuda(), torch.from_numpy(offsets).cuda()
mp = gridmap.default_match_params()
half_cell, half_step = 0.5 * p.resolution, 0.5 * mp.angle_step
errors = [np.concatenate([rng.uniform(-half_cell, half_cell, (batch, 2)), rng.uniform(-half_step, half_step, (batch, 1))], axis=1) for _ in range(4)]
d_priors = [torch.from_numpy(coral.pose_matrices(job_poses + e)).cuda() for e in errors]
d_res = [torch.zeros(batch * GRIDMAP_REFINE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda") for _ in range(4)]
d_mres = [torch.zeros(batch * GRIDMAP_MATCH_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda") for _ in range(4)]
rp = gridmap.default_refine_params()
stream = torch.cuda.current_stream().cuda_stream
points = int(offsets[-1])
print(f"{batch} jobs per call, {n_calls} calls per sweep, {points / batch:.0f} points per job, map {p.width} x {p.height} cells of "
      f"{p.resolution} m from {n_scans} scans ({lit} cells lit), priors within {half_cell} m and {half_step} rad of the truth")


def sweep(refine):
    t0 = time.perf_counter()
    for c in range(n_calls):
        if refine:
            h.refine_device(d_xy, d_off, d_priors[c % 4], d_res[c % 4], params=rp, stream=stream)
        else:
            h.match_device(d_xy, d_off, d_priors[c % 4], d_mres[c % 4], params=mp, stream=stream)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


jobs = n_calls * batch
timed = {}
for refine in (True, False):
    sweep(refine)  # warm-up (grows the workspace)
    sweep(refine)
    ts = [sweep(refine) for _ in range(reps)]
    timed[refine] = (float(np.median(ts)), min(ts), max(ts))
res = np.concatenate([r.cpu().numpy().view(GRIDMAP_REFINE_RESULT_DTYPE) for r in d_res])
err = np.concatenate(errors)
truth = np.tile(job_poses, (4, 1))
after_xy = np.hypot(res["transform"][:, 2] - truth[:, 0], res["transform"][:, 5] - truth[:, 1])
dyaw = np.arctan2(res["transform"][:, 3], res["transform"][:, 0]) - truth[:, 2]
after_yaw = np.abs((dyaw + np.pi) % (2.0 * np.pi) - np.pi)
before_xy, before_yaw = np.hypot(err[:, 0], err[:, 1]), np.abs(err[:, 2])
dt, lo, hi = timed[True]
evals = float(res["evaluations"].mean())
print(f"gridmap refine_batch_device ({batch} jobs per call): {dt / jobs * 1e6:.2f} us per job (median of {reps} sweeps; fastest "
      f"{lo / jobs * 1e6:.2f}, slowest {hi / jobs * 1e6:.2f}), {evals:.1f} evaluations per job on average ({dt / jobs / evals * 1e6:.2f} us per "
      f"evaluation), {float(res['accepted'].mean()):.1f} accepted; median pose error {np.median(before_xy):.4f} m, {np.median(before_yaw):.5f} rad "
      f"before, {np.median(after_xy):.4f} m, {np.median(after_yaw):.5f} rad after (worst after: {after_xy.max():.4f} m, {after_yaw.max():.5f} rad); "
      f"status bits seen {int(np.bitwise_or.reduce(res['status']))}, cost lower in {int(np.count_nonzero(res['cost'] < res['cost_initial']))} of {len(res)}")
dt, lo, hi = timed[False]
print(f"gridmap match_batch_device at its defaults, same session ({batch} jobs per call): {dt / jobs * 1e6:.2f} us per job (median of {reps} sweeps; "
      f"fastest {lo / jobs * 1e6:.2f}, slowest {hi / jobs * 1e6:.2f})")
h.close()
