#!/usr/bin/env python3
"""Time the CorAl alignment quality (rsx_coral_quality_batch_device): 64 jobs per call, the jobs being distinct pairs of scans of
the 400 x 3360 synthetic drive (k-strongest clouds, k = 12, z_min = 60, min_separation = 0: about 4800 points a side) at their
true relative poses, all resident in HBM.  Prints microseconds per job and neighbour visits per second (a visit = one point of a
3 x 3 block looked at by one walk; every valid point walks once, every scored point twice -- counted on the host from the device's
own per-point records and the cells).  There is no earlier GPU form of this measure to compare with.

usage: bench_coral.py [n_scans=72] [reps=7]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from navtech_radar_slam_amd import _rsx, coral, kstrongest, synth  # noqa: E402
from navtech_radar_slam_amd.cfear import ragged  # noqa: E402
import coral_np as co  # noqa: E402

n_scans = int(sys.argv[1]) if len(sys.argv) > 1 else 72
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
batch = 64
assert n_scans >= 66

import torch  # noqa: E402

imgs, az, poses, _ = synth.polar_sequence(11, n_scans)
ks = kstrongest.KStrongest(400, 3360)
clouds = []
for lo in range(0, n_scans, 8):
    _, xy = ks.extract_batch(imgs[lo:lo + 8], k=12, z_min=60, min_separation=0, azimuths=az)
    clouds += [np.ascontiguousarray(c, dtype=np.float32) for c in xy]
ks.close()
# the pairs: every scan against the next one and the one after that -- 2 (n_scans - 2) >= 128 distinct pairs
pairs = [(i, i + g) for g in (1, 2) for i in range(n_scans - 2)]
n_calls = len(pairs) // batch
pairs = pairs[:n_calls * batch]
print(f"{len(set(pairs))} distinct pairs of {n_scans} scans, {np.mean([len(c) for c in clouds]):.0f} points a side, {n_calls} calls of {batch} jobs")

h = coral.Coral()
calls = []
for c in range(n_calls):
    ps = pairs[c * batch:(c + 1) * batch]
    a, a_off = ragged([clouds[i] for i, _ in ps], np.float32, 2)
    b, b_off = ragged([clouds[j] for _, j in ps], np.float32, 2)
    T = coral.pose_matrices([synth.relative_pose(poses[i], poses[j]) for i, j in ps])
    calls.append(dict(ps=ps, a_off=a_off, b_off=b_off, n=len(a) + len(b),
                      dev=[torch.from_numpy(v).cuda() for v in (a, a_off, b, b_off, T)],
                      res=torch.zeros(batch * 40, dtype=torch.uint8, device="cuda")))
stream = torch.cuda.current_stream().cuda_stream


def sweep(points=None):
    t0 = time.perf_counter()
    for c in calls:
        d = c["dev"]
        h.quality_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), batch, c["res"].data_ptr(), d_transforms=d[4].data_ptr(),
                         d_points=points.data_ptr() if points is not None else None, stream=stream)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


# warm-up with the records of the first call: they give the visits (the block populations come from the cells of the joint cloud)
pts = torch.zeros(max(c["n"] for c in calls) * 24, dtype=torch.uint8, device="cuda")
visits = 0
for c in calls:
    d = c["dev"]
    h.quality_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), batch, c["res"].data_ptr(), d_transforms=d[4].data_ptr(),
                     d_points=pts.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    rec = pts.cpu().numpy()[:c["n"] * 24].view(_rsx.CORAL_POINT_DTYPE)
    T = d[4].cpu().numpy()
    first = c["a_off"] + c["b_off"]
    for k, (i, j) in enumerate(c["ps"]):
        xy = co.joint_cloud(clouds[i], clouds[j], T[k])
        cell, valid = co.cells_of(xy, 3.5)
        pop = np.bincount(cell[valid], minlength=128 * 128).reshape(128, 128)
        padded = np.pad(pop, 1)
        block = sum(padded[1 + dy:129 + dy, 1 + dx:129 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)).reshape(-1)
        r = rec[first[k]:first[k + 1]]
        scored = (r["m_separate"] >= 6) & (r["m_joint"] - r["m_separate"] >= 1)
        visits += int(block[cell[valid]].sum()) + int(block[cell[valid & scored]].sum())
res = np.concatenate([c["res"].cpu().numpy().view(_rsx.CORAL_RESULT_DTYPE) for c in calls])
print(f"Q at the true poses: median {np.median(res['quality']):.4f}, max {res['quality'].max():.4f}; scored {res['n_scored'].mean():.0f} of "
      f"{res['n_valid'].mean():.0f} points per job; {visits / len(pairs):.3g} neighbour visits per job")
ts = [sweep() for _ in range(reps)]
dt = float(np.median(ts))
print(f"coral quality_batch_device ({batch} jobs per call, {len(pairs)} distinct pairs): {dt / len(pairs) * 1e6:.1f} us per job "
      f"(median of {reps} sweeps; fastest {min(ts) / len(pairs) * 1e6:.1f}, slowest {max(ts) / len(pairs) * 1e6:.1f}), "
      f"{visits / dt / 1e9:.2f} G neighbour visits/s")
ts = [sweep(pts) for _ in range(reps)]
print(f"  with the per-point records written: {float(np.median(ts)) / len(pairs) * 1e6:.1f} us per job")
h.close()
