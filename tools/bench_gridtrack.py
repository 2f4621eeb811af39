#!/usr/bin/env python3
"""Time the grid-map tracker (rsx_gridmap_tracker_push_device): 1, 16, 64 and 256 sequences side by side, 64 scans per sequence per push,
the clouds being the default k-strongest clouds (4800 points) of 64 consecutive 400 x 3360 scans of the synthetic drive, the map the
default map (1024 x 1024 cells of 0.5 m, centred on the drive) built from the same scans at their true poses, its mean as the likelihood;
the default window (K = U = V = 2 of 0.01 rad) and the refinement's defaults.  Every sequence follows the same drive from scan 0's true
pose moved by a fraction of a cell of its own, so that no two sequences do the same arithmetic.  Everything is resident in HBM.

Timed in the same session, alternating with the tracker sweep by sweep, the yardstick: the host loop over the stand-alone device
entries that the tracker replaces, batched over the same sequences -- per scan the prediction on the host (numpy, all sequences at once),
the priors up, match_batch_device, the winners' transforms out of their records on the device, refine_batch_device, both records down,
ONE synchronise, the lost rule and the motion on the host.  Its poses are checked against the tracker's, byte for byte.

A sweep is `rounds` pushes (tracker) or `rounds` drives of the loop (yardstick), rounds = max(1, 64 / sequences), so that every timed
window is a fair fraction of a second.  Prints scans per second and microseconds per scan for both, the median of the sweeps with the
fastest and the slowest, and one JSON line per sequence count.

usage: bench_gridtrack.py [reps=7] [sequence counts=1,16,64,256] [scans=64]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from navtech_radar_slam_amd import coral, gridmap, kstrongest, synth  # noqa: E402
from navtech_radar_slam_amd._rsx import GRIDMAP_TRACK_LOST, GRIDMAP_TRACK_RESULT_DTYPE  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
counts = [int(v) for v in (sys.argv[2] if len(sys.argv) > 2 else "1,16,64,256").split(",")]
n_scans = int(sys.argv[3]) if len(sys.argv) > 3 else 64

import torch  # noqa: E402

imgs, _, poses, _ = synth.polar_sequence(11, n_scans)
centre = poses[:, :2].mean(axis=0)
p = gridmap.default_params()
p.origin_x, p.origin_y = float(centre[0]) - 0.5 * p.width * p.resolution, float(centre[1]) - 0.5 * p.height * p.resolution
h = gridmap.GridMap(400, 3360, p)
h.add(imgs, coral.pose_matrices(poses))
h.update_likelihood()

targets = kstrongest.KStrongest(400, 3360).extract_batch(imgs)
clouds = []
for tg in targets:   # (bin + 0.5) 0.0595 along 2 pi row / 400, fp64, rounded once
    rho, phi = (tg[:, 1].astype(np.float64) + 0.5) * synth.RADAR_RESOLUTION, tg[:, 0].astype(np.float64) * 2.0 * np.pi / 400.0
    clouds.append(np.stack([rho * np.cos(phi), rho * np.sin(phi)], axis=1).astype(np.float32))
n_points = len(clouds[0])
assert all(len(c) == n_points for c in clouds)
d_drive = torch.from_numpy(np.stack(clouds)).cuda()      # [scan][point][2]
tp = gridmap.default_track_params()
torch.cuda.set_stream(torch.cuda.Stream())      # torch's copies between the library's calls run on the stream the calls are given
stream = torch.cuda.current_stream().cuda_stream
assert stream != 0
print(f"{n_scans} scans of {n_points} points per sequence per push, map {p.width} x {p.height} cells of {p.resolution} m, window K = "
      f"{tp.match.angle_steps}, U = {tp.match.x_cells}, V = {tp.match.y_cells}, at most {tp.refine.max_evaluations} evaluations")


# ---- the glue of include/rsx.h on (S, 6) arrays: fp64 on plain operations in the order written ----

def mul(A, B):
    return np.stack([A[:, 0] * B[:, 0] + A[:, 1] * B[:, 3], A[:, 0] * B[:, 1] + A[:, 1] * B[:, 4], (A[:, 0] * B[:, 2] + A[:, 1] * B[:, 5]) + A[:, 2],
                     A[:, 3] * B[:, 0] + A[:, 4] * B[:, 3], A[:, 3] * B[:, 1] + A[:, 4] * B[:, 4], (A[:, 3] * B[:, 2] + A[:, 4] * B[:, 5]) + A[:, 5]], axis=1)


def inv(A):
    return np.stack([A[:, 0], A[:, 3], -(A[:, 0] * A[:, 2] + A[:, 3] * A[:, 5]), A[:, 1], A[:, 4], -(A[:, 1] * A[:, 2] + A[:, 4] * A[:, 5])], axis=1)


def renorm(T):
    f = 1.5 - 0.5 * (T[:, 0] * T[:, 0] + T[:, 3] * T[:, 3])
    c, s = T[:, 0] * f, T[:, 3] * f
    return np.stack([c, -s, T[:, 2], s, c, T[:, 5]], axis=1)


for S in counts:
    rounds = max(1, 64 // S)
    rng = np.random.default_rng(S)
    starts = coral.pose_matrices(poses[:1] + np.concatenate([rng.uniform(-0.2, 0.2, (S, 2)), rng.uniform(-0.004, 0.004, (S, 1))], axis=1))
    # the tracker's layout: sequence after sequence; the loop's: scan after scan, the sequences of one scan side by side
    d_by_sequence = d_drive.unsqueeze(0).expand(S, n_scans, n_points, 2).reshape(-1, 2).contiguous()
    d_by_scan = d_drive.unsqueeze(1).expand(n_scans, S, n_points, 2).reshape(-1, 2).contiguous()
    d_off_all = torch.arange(S * n_scans + 1, dtype=torch.int64, device="cuda") * n_points
    d_off_scan = [d_off_all[j * S:(j + 1) * S + 1] - j * S * n_points for j in range(n_scans)]
    d_off_scan = [o.contiguous() for o in d_off_scan]
    d_xy_scan = [d_by_scan[j * S * n_points:(j + 1) * S * n_points] for j in range(n_scans)]
    d_n = torch.full((S,), n_scans, dtype=torch.int32, device="cuda")
    d_out = torch.zeros(S * n_scans * GRIDMAP_TRACK_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_prior = torch.zeros((S, 6), dtype=torch.float64, device="cuda")
    d_prior2 = torch.zeros((S, 6), dtype=torch.float64, device="cuda")
    d_match = torch.zeros((S, 11), dtype=torch.float64, device="cuda")       # 88 bytes a record, the transform first
    d_refine = torch.zeros((S, 19), dtype=torch.float64, device="cuda")      # 152 bytes a record, the transform first
    h_match = torch.zeros((S, 11), dtype=torch.float64).pin_memory()
    h_refine = torch.zeros((S, 19), dtype=torch.float64).pin_memory()
    h_prior = torch.zeros((S, 6), dtype=torch.float64).pin_memory()
    t = h.tracker(S)
    torch.cuda.synchronize()

    def track():
        """-> seconds for `rounds` pushes (the resets between them are not timed)"""
        total = 0.0
        for _ in range(rounds):
            t.reset(starts)
            t0 = time.perf_counter()
            t.push_device(d_by_sequence, d_off_all, d_n, d_out, params=tp, stream=stream)
            torch.cuda.synchronize()
            total += time.perf_counter() - t0
        return total

    def loop():
        """-> (seconds for `rounds` drives of the host loop, the poses after the last one)"""
        total = 0.0
        for _ in range(rounds):
            P, M = starts.copy(), np.tile(np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0]), (S, 1))
            t0 = time.perf_counter()
            for j in range(n_scans):
                start = P if j == 0 or not tp.predict else renorm(mul(P, M))
                h_prior.numpy()[:] = start
                d_prior.copy_(h_prior, non_blocking=True)
                h.match_device(d_xy_scan[j], d_off_scan[j], d_prior, d_match.view(torch.uint8).view(-1), params=tp.match, stream=stream)
                d_prior2.copy_(d_match[:, :6])
                h.refine_device(d_xy_scan[j], d_off_scan[j], d_prior2, d_refine.view(torch.uint8).view(-1), params=tp.refine, stream=stream)
                h_match.copy_(d_match, non_blocking=True)
                h_refine.copy_(d_refine, non_blocking=True)
                torch.cuda.synchronize()
                m = h_match.numpy().view(np.uint8).reshape(S, 88)
                score, status = m[:, 60:64].copy().view(np.uint32)[:, 0], m[:, 80:84].copy().view(np.int32)[:, 0]
                lost = (status != 0) | (score < tp.min_score)
                new = renorm(h_refine.numpy()[:, :6])
                if j > 0:
                    M = np.where(lost[:, None], M, mul(inv(P), new))
                P = np.where(lost[:, None], start, new)
            total += time.perf_counter() - t0
        return total, P

    for _ in range(2):          # warm-up: code objects, the map's workspaces, the pinned copies
        track()
        loop()
    times = {"tracker": [], "loop": []}
    for _ in range(reps):       # alternating, so that a drift of the machine falls on both
        times["tracker"].append(track())
        dt, P_loop = loop()
        times["loop"].append(dt)
    rec = d_out.cpu().numpy().view(GRIDMAP_TRACK_RESULT_DTYPE).reshape(S, n_scans)
    same = rec["transform"][:, -1].tobytes() == np.ascontiguousarray(P_loop).tobytes()
    lost = int(np.count_nonzero(rec["flags"] & GRIDMAP_TRACK_LOST))
    every = np.hypot(rec["transform"][:, :, 2] - poses[None, :, 0], rec["transform"][:, :, 5] - poses[None, :, 1])    # [sequence][scan], metres
    err = every[:, -1]
    held = (every < 0.5).all(axis=0)
    first_off = int(np.argmin(held)) if not held.all() else n_scans      # the first scan at which some sequence is a cell or more off
    k_at_the_edge = float(np.mean(np.abs(rec["match"]["k"]) == tp.match.angle_steps))
    scans = rounds * S * n_scans
    line = {"sequences": S, "scans_per_sweep": scans, "same_poses_as_the_loop": bool(same), "lost_scans": lost,
            "worst_final_error_m": float(err.max()), "median_error_m": float(np.median(every)), "scans_before_a_cell_off": first_off,
            "share_of_winners_at_the_last_rotation": k_at_the_edge, "mean_evaluations": float(rec["refine"]["evaluations"].mean())}
    for name, ts in times.items():
        med, lo, hi = float(np.median(ts)), min(ts), max(ts)
        line[name] = {"scans_per_s": scans / med, "us_per_scan": med / scans * 1e6, "fastest_us": lo / scans * 1e6, "slowest_us": hi / scans * 1e6}
        print(f"{S:4d} sequences, {name:7s}: {scans / med:10.0f} scans/s, {med / scans * 1e6:8.2f} us per scan (median of {reps} sweeps of {scans} scans; "
              f"fastest {lo / scans * 1e6:.2f}, slowest {hi / scans * 1e6:.2f})")
    line["tracker_over_loop"] = line["loop"]["us_per_scan"] / line["tracker"]["us_per_scan"]
    print(f"{S:4d} sequences: the tracker is {line['tracker_over_loop']:.2f} times the loop's rate; same final poses: {same}; {lost} scans lost; "
          f"worst final error {err.max():.4f} m, median error over all scans {np.median(every):.4f} m, {first_off} scans before some sequence is 0.5 m off, "
          f"{k_at_the_edge:.2f} of the winners at |k| = K")
    print(json.dumps(line))
    t.close()
    del d_by_sequence, d_by_scan, d_xy_scan
h.close()
