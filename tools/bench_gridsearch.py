#!/usr/bin/env python3
"""Time the wide-window correlative search (rsx_gridmap_search_batch_device) beside the exhaustive matcher
(rsx_gridmap_match_batch_device) in one session: 64 jobs per call, the clouds being the default k-strongest clouds (4800 points) of
consecutive 400 x 3360 scans of the synthetic drive, the map the default map (1024 x 1024 cells of 0.5 m, centred on the drive) built
from the same scans at their true poses, its mean as the likelihood; K = 8, angle_step 0.01.  The priors are the true poses moved by up
to 0.04 rad and by up to 0.8 of the window in x and y, in four different ways that the 64 calls of a sweep take in turn.  Rows:
match and search at U = V = 32 (match is the yardstick), search at U = V = 128 and 256, and search at U = V = 32 with priors 60 m off,
so that the peak is outside the window, without a min_score and with one of 0.5 and of 0.9 of the median winning score of the first
search row.
Everything is resident in HBM; bounds and volumes stay in the handle's workspace.  Prints microseconds per job and the share of blocks
refined.

usage: bench_gridsearch.py [n_scans=64] [reps=7] [jobs_per_call=64]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from navtech_radar_slam_amd import coral, gridmap, kstrongest, synth  # noqa: E402
from navtech_radar_slam_amd._rsx import GRIDMAP_MATCH_RESULT_DTYPE, GRIDMAP_SEARCH_RESULT_DTYPE  # noqa: E402

n_scans = int(sys.argv[1]) if len(sys.argv) > 1 else 64
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
batch, n_calls = int(sys.argv[3]) if len(sys.argv) > 3 else 64, 64
assert n_scans >= batch, "a job per scan: at least jobs_per_call scans"
K, STEP = 8, 0.01

import torch  # noqa: E402

imgs, _, poses, _ = synth.polar_sequence(11, n_scans)
centre = poses[:, :2].mean(axis=0)
p = gridmap.default_params()
p.origin_x, p.origin_y = float(centre[0]) - 0.5 * p.width * p.resolution, float(centre[1]) - 0.5 * p.height * p.resolution
h = gridmap.GridMap(400, 3360, p)
for b0 in range(0, n_scans, batch):
    h.add(imgs[b0:b0 + batch], coral.pose_matrices(poses[b0:b0 + batch]))
h.update_likelihood()
h.prepare_search(256)

targets = kstrongest.KStrongest(400, 3360).extract_batch(imgs[:batch])
clouds = []
for tg in targets:   # (bin + 0.5) 0.0595 along 2 pi row / 400, fp64, rounded once
    rho, phi = (tg[:, 1].astype(np.float64) + 0.5) * synth.RADAR_RESOLUTION, tg[:, 0].astype(np.float64) * 2.0 * np.pi / 400.0
    clouds.append(np.stack([rho * np.cos(phi), rho * np.sin(phi)], axis=1).astype(np.float32))
offsets = np.zeros(batch + 1, dtype=np.int64)
offsets[1:] = np.cumsum([len(c) for c in clouds])
d_xy, d_off = torch.from_numpy(np.concatenate(clouds)).cuda(), torch.from_numpy(offsets).cuda()
stream = torch.cuda.current_stream().cuda_stream
print(f"{batch} jobs per call, {n_calls} calls per sweep, {int(offsets[-1]) / batch:.0f} points per job, K = {K}, map {p.width} x {p.height} cells of "
      f"{p.resolution} m from {n_scans} scans", flush=True)


def run(name, cells, search, away=0.0, min_score=0):
    """one row: the priors off by up to 0.8 cells * resolution in x and y (plus `away` metres in x), 64 calls a sweep, median of reps"""
    rng = np.random.default_rng(1)
    reach = 0.8 * cells * p.resolution
    errors = [np.concatenate([rng.uniform(-reach, reach, (batch, 2)), rng.uniform(-0.04, 0.04, (batch, 1))], axis=1) for _ in range(4)]
    for e in errors:
        e[:, 0] += away
    d_priors = [torch.from_numpy(coral.pose_matrices(poses[:batch] + e)).cuda() for e in errors]
    dtype = GRIDMAP_SEARCH_RESULT_DTYPE if search else GRIDMAP_MATCH_RESULT_DTYPE
    d_res = [torch.zeros(batch * dtype.itemsize, dtype=torch.uint8, device="cuda") for _ in range(4)]
    if search:
        mp = gridmap.search_params(angle_steps=K, x_cells=cells, y_cells=cells, angle_step=STEP, min_score=min_score)
        call = h.search_device
    else:
        mp = gridmap.match_params(angle_steps=K, x_cells=cells, y_cells=cells, angle_step=STEP)
        call = h.match_device

    def sweep():
        t0 = time.perf_counter()
        for c in range(n_calls):
            call(d_xy, d_off, d_priors[c % 4], d_res[c % 4], params=mp, stream=stream)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    sweep()  # warm-up (grows the workspace)
    sweep()
    ts = [sweep() for _ in range(reps)]
    dt, jobs = float(np.median(ts)), n_calls * batch
    res = np.concatenate([r.cpu().numpy().view(dtype) for r in d_res])
    err = np.concatenate(errors)
    back = int(np.count_nonzero((np.abs(res["u"] * p.resolution + err[:, 0]) <= p.resolution) & (np.abs(res["v"] * p.resolution + err[:, 1]) <= p.resolution)
                                & (np.abs(res["k"] * STEP + err[:, 2]) <= STEP) & (res["status"] == 0)))
    share = f", {100.0 * res['n_refined'].sum() / res['n_blocks'].sum():.2f} % of {int(res['n_blocks'][0])} blocks refined" if search else ""
    print(f"{name}: {dt / jobs * 1e6:.1f} us per job (median of {reps} sweeps; fastest {min(ts) / jobs * 1e6:.1f}, slowest {max(ts) / jobs * 1e6:.1f})"
          f"{share}; {back} of {4 * batch} distinct jobs within a cell and a step of the true pose, status bits seen "
          f"{int(np.bitwise_or.reduce(res['status']))}", flush=True)
    return res


run("match  U = V = 32", 32, False)
near = run("search U = V = 32", 32, True)
run("search U = V = 128", 128, True)
run("search U = V = 256", 256, True)
typical = int(np.median(near["score"]))
run("search U = V = 32, the peak 60 m outside the window, no min_score", 32, True, away=60.0)
for share in (0.5, 0.9):
    run(f"search U = V = 32, the peak 60 m outside the window, min_score {int(share * typical)} ({share} of the median winning score {typical})", 32, True,
        away=60.0, min_score=int(share * typical))
h.close()
