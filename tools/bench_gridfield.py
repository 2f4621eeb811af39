#!/usr/bin/env python3
"""Time the likelihood field of the grid map (rsx_gridmap_likelihood_field): the default map (1024 x 1024 cells of 0.5 m, centred on the
drive) built from consecutive 400 x 3360 scans of the synthetic drive at their true poses, its hits as the likelihood, the default
threshold (50) and the Gaussian table of sigma 3 cells, at radius 4, 12 and 64.  Everything is resident in HBM.  Prints microseconds per
call three ways, each the median of `reps` sweeps of 256 calls with the fastest and the slowest sweep beside it: the field alone (a field
of the field before it: the launches branch on no byte of the plane, so their cost does not depend on what it holds); the pair that a
map update is, rsx_gridmap_likelihood_update and the field behind it; and, timed in the same session as the figure to read both against,
rsx_gridmap_likelihood_update alone.  Beside them the bytes that a call must move -- the plane read once and written once, 2 bytes per
cell, and the bits of the seeds written once and read once, a quarter of a byte per cell -- and the share of the HBM peak (8 TB/s) that
they amount to in the time of the field alone.  Then the chain that the field is there for: the default k-strongest clouds of the scans
from priors within 3 m and 0.03 rad and within 6 m and 0.06 rad of the truth, refined on the field (radius 12, max_evaluations 64), and
refined again on the mean at the default parameters; the same priors refined on the mean alone for comparison.  No earlier GPU form
exists to compare with.

usage: bench_gridfield.py [n_scans=64] [reps=7]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from navtech_radar_slam_amd import coral, gridmap, kstrongest, synth  # noqa: E402
from navtech_radar_slam_amd._rsx import GRIDMAP_HITS, GRIDMAP_MEAN, GRIDMAP_REFINE_RESULT_DTYPE  # noqa: E402

n_scans = int(sys.argv[1]) if len(sys.argv) > 1 else 64
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
n_calls, batch = 256, 64
HBM_PEAK = 8e12   # bytes per second

import torch  # noqa: E402

imgs, _, poses, _ = synth.polar_sequence(11, n_scans)
centre = poses[:, :2].mean(axis=0)
p = gridmap.default_params()
p.origin_x, p.origin_y = float(centre[0]) - 0.5 * p.width * p.resolution, float(centre[1]) - 0.5 * p.height * p.resolution
h = gridmap.GridMap(400, 3360, p)
for b0 in range(0, n_scans, batch):
    h.add(imgs[b0:b0 + batch], coral.pose_matrices(poses[b0:b0 + batch]))
h.update_likelihood(GRIDMAP_HITS)
fp = gridmap.default_field_params()
seeds = int(np.count_nonzero(h.likelihood() >= fp.threshold))
stream = torch.cuda.current_stream().cuda_stream
cells = p.width * p.height
must_move = 2 * cells + 2 * (cells // 8)
print(f"map {p.width} x {p.height} cells of {p.resolution} m from {n_scans} scans, hits as the likelihood: {seeds} cells at or above {fp.threshold}; "
      f"{n_calls} calls per sweep; a call must move {must_move} bytes ({must_move / HBM_PEAK * 1e6:.2f} us at the HBM peak of {HBM_PEAK / 1e12:.0f} TB/s)")


def sweep(update, field, table, params):
    t0 = time.perf_counter()
    for _ in range(n_calls):
        if update:
            h.update_likelihood(GRIDMAP_HITS, stream=stream)
        if field:
            h.likelihood_field(table, params=params, stream=stream)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def timed(*what):
    sweep(*what)  # warm-up (allocates the workspace, uploads the table)
    sweep(*what)
    ts = [sweep(*what) / n_calls * 1e6 for _ in range(reps)]
    return float(np.median(ts)), min(ts), max(ts)


def say(name, t):
    return f"{name} {t[0]:.2f} us per call (median of {reps} sweeps; fastest {t[1]:.2f}, slowest {t[2]:.2f})"


for radius in (4, 12, 64):
    params = gridmap.field_params(radius=radius)
    table = gridmap.gaussian_table(3.0, radius)
    h.update_likelihood(GRIDMAP_HITS, stream=stream)
    alone = timed(False, True, table, params)
    pair = timed(True, True, table, params)
    print(f"gridmap likelihood_field radius {radius}: " + say("the field alone", alone) + f", {must_move / HBM_PEAK * 1e6 / alone[0] * 100:.1f} % of the HBM peak; "
          + say("likelihood_update and the field", pair))
print("gridmap likelihood_update, same session: " + say("alone", timed(True, False, None, None)))

# ---- the chain: refine on the field, then on the mean ----
n_clouds = min(n_scans, batch)
targets = kstrongest.KStrongest(400, 3360).extract_batch(imgs[:n_clouds])
clouds = []
for tg in targets:   # (bin + 0.5) 0.0595 along 2 pi row / 400, fp64, rounded once
    rho, phi = (tg[:, 1].astype(np.float64) + 0.5) * synth.RADAR_RESOLUTION, tg[:, 0].astype(np.float64) * 2.0 * np.pi / 400.0
    clouds.append(np.stack([rho * np.cos(phi), rho * np.sin(phi)], axis=1).astype(np.float32))
clouds = [clouds[i % n_clouds] for i in range(batch)]
truth = poses[np.arange(batch) % n_clouds]
offsets = np.zeros(batch + 1, dtype=np.int64)
offsets[1:] = np.cumsum([len(c) for c in clouds])
d_xy, d_off = torch.from_numpy(np.concatenate(clouds)).cuda(), torch.from_numpy(offsets).cuda()
d_res = [torch.zeros(batch * GRIDMAP_REFINE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda") for _ in range(3)]
far, near = gridmap.refine_params(max_evaluations=64), gridmap.default_refine_params()


def chain(d_prior):
    """-> seconds for the refinement on the field alone (the plane is prepared before the clock starts)"""
    h.update_likelihood(GRIDMAP_HITS, stream=stream)
    h.likelihood_field(stream=stream)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    h.refine_device(d_xy, d_off, d_prior, d_res[0], params=far, stream=stream)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    h.update_likelihood(GRIDMAP_MEAN, stream=stream)
    h.refine_device(d_xy, d_off, d_res[0].view(torch.float64).view(batch, -1)[:, :6].contiguous(), d_res[1], params=near, stream=stream)
    h.refine_device(d_xy, d_off, d_prior, d_res[2], params=far, stream=stream)
    torch.cuda.synchronize()
    return dt


def spread(name, t):
    res = t.cpu().numpy().view(GRIDMAP_REFINE_RESULT_DTYPE)
    dist = np.hypot(res["transform"][:, 2] - truth[:, 0], res["transform"][:, 5] - truth[:, 1])
    dyaw = np.arctan2(res["transform"][:, 3], res["transform"][:, 0]) - truth[:, 2]
    dyaw = np.abs((dyaw + np.pi) % (2.0 * np.pi) - np.pi)
    return (f"  {name}: median {np.median(dist):.4f} m and {np.median(dyaw):.5f} rad, worst {dist.max():.4f} m and {dyaw.max():.5f} rad, "
            f"{int(np.count_nonzero(dist < 0.05))} of {batch} within 0.05 m, {float(res['evaluations'].mean()):.1f} evaluations per job")


rng = np.random.default_rng(1)
for off_m, off_rad in ((3.0, 0.03), (6.0, 0.06)):   # the field's radius is 12 cells: 6 m
    errors = np.concatenate([rng.uniform(-off_m, off_m, (batch, 2)), rng.uniform(-off_rad, off_rad, (batch, 1))], axis=1)
    d_prior = torch.from_numpy(coral.pose_matrices(truth + errors)).cuda()
    chain(d_prior)
    ts = [chain(d_prior) / batch * 1e6 for _ in range(reps)]
    before = np.hypot(errors[:, 0], errors[:, 1])
    print(f"gridmap refine on the field (radius {fp.radius}, {batch} jobs per call, {int(offsets[-1]) // batch} points per job, max_evaluations 64), priors "
          f"within {off_m} m along x and y and {off_rad} rad of the truth (median {np.median(before):.2f} m, worst {before.max():.2f} m off): "
          f"{float(np.median(ts)):.2f} us per job (median of {reps} calls; fastest {min(ts):.2f}, slowest {max(ts):.2f})")
    print(spread("after the field", d_res[0]))
    print(spread("then on the mean (default parameters)", d_res[1]))
    print(spread("the same priors on the mean alone (max_evaluations 64)", d_res[2]))
h.close()
