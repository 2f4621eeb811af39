#!/usr/bin/env python3
"""Time CFEAR's surface-point build and point-to-line registration, and the odometry pipeline with them, in one session.

The inputs are the k-strongest clouds (k = 12, z_min = 60, min_separation = 0) of >= 256 distinct consecutive scans of the
synthetic drive synth.polar_sequence(11, n), MulRan shape (400 x 3360).  Measured, each through its device entry on resident
buffers, 64 scans / pairs per call cycling through all of them: the surface-point build (rsx_cfear_surface_points_batch_device)
and the registration of consecutive scans (rsx_cfear_register_batch_device, identity start).  Then the windowed odometry
(rsx_odometry_push, host images) on the same scans with k-strongest(min_separation 0) + CFEAR beside k-strongest(min_separation
5) + ORORA, alternating.  Prints microseconds per call and scans/s; every timed window ends in a device synchronise.

usage: bench_cfear.py [n_scans=256] [reps=5] [odometry_reps=3]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from navtech_radar_slam_amd import _rsx, cfear, kstrongest, odometry, synth  # noqa: E402

n_scans = int(sys.argv[1]) if len(sys.argv) > 1 else 256
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
odo_reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
batch = 64
assert n_scans % batch == 0 and n_scans >= 256

import torch  # noqa: E402

t0 = time.perf_counter()
imgs, az, poses, _ = synth.polar_sequence(11, n_scans)
print(f"{n_scans} consecutive scans generated in {time.perf_counter() - t0:.0f} s, {imgs.nbytes / 2**20:.0f} MiB", flush=True)
ks = kstrongest.KStrongest(400, 3360)
clouds = []
for b in range(0, n_scans, batch):
    _, xy = ks.extract_batch(imgs[b:b + batch], min_separation=0, azimuths=az if np.ndim(az) == 1 else az[b:b + batch])
    clouds += xy
print(f"k-strongest clouds: {np.mean([len(c) for c in clouds]):.0f} points per scan")

h = cfear.Cfear()
M = _rsx.CFEAR_MAX_SURFACE_POINTS
stream = torch.cuda.current_stream().cuda_stream
nb = n_scans // batch
d_xy, d_off = [], []
for b in range(nb):
    xy, off = cfear.ragged(clouds[b * batch:(b + 1) * batch], np.float32, 2)
    d_xy.append(torch.from_numpy(xy).cuda())
    d_off.append(torch.from_numpy(off).cuda())
d_rec = [torch.zeros(batch * M * 32, dtype=torch.uint8, device="cuda") for _ in range(nb)]
d_cnt = [torch.zeros(batch, dtype=torch.int32, device="cuda") for _ in range(nb)]


def sweep_surface():
    t0 = time.perf_counter()
    for b in range(nb):
        h.surface_points_device(d_xy[b].data_ptr(), d_off[b].data_ptr(), batch, d_rec[b].data_ptr(), M, d_cnt[b].data_ptr(), stream=stream)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


# the registration's inputs: the records of consecutive scans as two ragged layouts (src = scan i + 1, dst = scan i)
sweep_surface()
records = []
for b in range(nb):
    rec = d_rec[b].cpu().numpy().view(_rsx.CFEAR_SURFACE_POINT_DTYPE).reshape(batch, M)
    cnt = d_cnt[b].cpu().numpy()
    records += [rec[i, :min(int(cnt[i]), M)].copy() for i in range(batch)]
print(f"surface points: {np.mean([len(r) for r in records]):.0f} per scan (min {min(len(r) for r in records)}, max {max(len(r) for r in records)})")
pairs = [(records[(i + 1) % n_scans], records[i]) for i in range(n_scans)]  # (the last pair wraps round: far apart, status 4 at once)
d_pairs = []
for b in range(nb):
    s, so = cfear.ragged([p[0] for p in pairs[b * batch:(b + 1) * batch]], _rsx.CFEAR_SURFACE_POINT_DTYPE)
    d, do = cfear.ragged([p[1] for p in pairs[b * batch:(b + 1) * batch]], _rsx.CFEAR_SURFACE_POINT_DTYPE)
    d_pairs.append([torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a).cuda() for a in (s, so, d, do)])
d_res = [torch.zeros(batch * 48, dtype=torch.uint8, device="cuda") for _ in range(nb)]


def sweep_register():
    t0 = time.perf_counter()
    for b in range(nb):
        s, so, d, do = d_pairs[b]
        h.register_device(s.data_ptr(), so.data_ptr(), d.data_ptr(), do.data_ptr(), batch, d_res[b].data_ptr(), stream=stream)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


sweeps = {"surface_points_batch_device": sweep_surface, "register_batch_device": sweep_register}
for f in sweeps.values():
    f()  # warm-up
times = {k: [] for k in sweeps}
for r in range(reps):
    for k, f in sweeps.items():
        times[k].append(f())
for k, ts in times.items():
    per_call = float(np.median(ts)) / nb
    print(f"{k}: {per_call * 1e6:.0f} us per {batch} (median of {reps} sweeps of {nb} calls; fastest {min(ts) / nb * 1e6:.0f}, "
          f"slowest {max(ts) / nb * 1e6:.0f}) = {batch / per_call:.0f} per s")
res = np.concatenate([r.cpu().numpy().view(_rsx.CFEAR_RESULT_DTYPE) for r in d_res])[:n_scans - 1]
print(f"registration: status counts {dict((int(k), int(v)) for k, v in zip(*np.unique(res['status'], return_counts=True)))}, iterations mean {res['iterations'].mean():.1f} "
      f"max {res['iterations'].max()}, correspondences mean {res['correspondences'].mean():.0f}")

pipelines = {
    "kstrongest(sep 0) + cfear": dict(keypoints="kstrongest", kstrongest=kstrongest.params(min_separation=0), estimator="cfear"),
    "kstrongest(sep 5) + orora": dict(keypoints="kstrongest", kstrongest=kstrongest.params(min_separation=5)),
}
ods = {k: odometry.Odometry(400, 3360, **kw) for k, kw in pipelines.items()} if odo_reps > 0 else {}
out, best = {}, {}
for k, od in ods.items():
    out[k] = od.push(imgs, az)  # warm-up: workspaces
for r in range(odo_reps):
    for k, od in ods.items():  # alternating, so that both see the same machine
        od.reset()
        t0 = time.perf_counter()
        out[k] = od.push(imgs, az)
        best.setdefault(k, []).append(time.perf_counter() - t0)
for k, ts in best.items():
    o = out[k]
    err = [float(np.hypot(o["x"][i] - t[0], o["y"][i] - t[1])) for i in range(1, n_scans) for t in [synth.relative_pose(poses[i - 1], poses[i])]]
    print(f"odometry pipeline, {k}: {n_scans / float(np.median(ts)):.0f} scans/s over {n_scans} scans (median of {odo_reps}; fastest "
          f"{n_scans / min(ts):.0f}, slowest {n_scans / max(ts):.0f}); {np.mean(o['n_matches'][1:]):.0f} matches per scan, "
          f"{int(np.sum(o['status'][1:] != 0))} pairs with status != 0, translation error median {np.median(err):.3f} m max {np.max(err):.3f} m")
