#!/usr/bin/env python3
"""Time CA-CFAR / BFAR keypoint extraction against k-strongest in one session: each through its batched device entry on 64-scan
batches that cycle through >= 256 distinct MulRan-shape scans resident in HBM (400 x 3371 bytes each: > 256 MiB in all, past
the Infinity Cache), the extractors alternating; CFAR with its defaults (cell averaging) and with greatest-of.  Then the
windowed odometry pipeline (rsx_odometry_push) with k-strongest and with CFAR.  Prints scans/s.

usage: bench_cfar.py [n_distinct=256] [reps=5] [odometry_scans=64]"""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from navtech_radar_slam_amd import _rsx, cfar, kstrongest, odometry, synth  # noqa: E402

n_distinct = int(sys.argv[1]) if len(sys.argv) > 1 else 256
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
n_odo = int(sys.argv[3]) if len(sys.argv) > 3 else 64
batch = 64
assert n_distinct % batch == 0 and n_distinct >= 256

import torch  # noqa: E402

# distinct scans: 16 synthetic worlds, each rolled in azimuth and sprinkled with its own noise (as tools/bench_kstrongest.py)
rng = np.random.default_rng(2018)
base = [synth.polar_image(300 + i, n_targets=1200)[0] for i in range(16)]
scans = np.empty((n_distinct,) + base[0].shape, dtype=np.uint8)
for i in range(n_distinct):
    s = np.roll(base[i % 16], 7 * (i // 16), axis=0).copy()
    idx = rng.integers(0, s.size, 4000)
    s.flat[idx] = rng.integers(0, 120, idx.size).astype(np.uint8)
    scans[i] = s
print(f"{n_distinct} distinct scans, {scans.nbytes / 2**20:.0f} MiB resident")
d = torch.from_numpy(scans).cuda()
mt = 20000
tg = torch.zeros((batch, mt, 2), dtype=torch.int32, device="cuda")
cnt = torch.zeros(batch, dtype=torch.int32, device="cuda")
stream = torch.cuda.current_stream().cuda_stream
L = _rsx.lib()
extractors = {
    "kstrongest": (kstrongest.KStrongest(400, 3360), L.rsx_kstrongest_extract_batch_device, kstrongest.default_params()),
    "cfar": (cfar.Cfar(400, 3360), L.rsx_cfar_extract_batch_device, cfar.default_params()),
    "cfar greatest-of": (cfar.Cfar(400, 3360), L.rsx_cfar_extract_batch_device, cfar.params(mode=cfar.CFAR_GO)),
}
nb = n_distinct // batch


def sweep(name):
    """every distinct scan once through the device entry of `name`, 64 per call -> seconds, keypoints (ends in a device synchronise)"""
    ex, entry, p = extractors[name]
    t0 = time.perf_counter()
    for b in range(nb):
        _rsx.check(entry(ex._h, d.data_ptr() + b * batch * scans.strides[0], batch, scans.strides[0], scans.shape[2], 11, C.byref(p), None, 0,
                         0.0595, tg.data_ptr(), None, mt, cnt.data_ptr(), C.c_void_p(stream)))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    total = int(cnt.sum().item())  # (of the last batch)
    return dt, total


best, kps = {}, {}
for name in extractors:
    kps[name] = sweep(name)[1] / batch  # warm-up: code objects, workspaces
for r in range(reps):
    for name in extractors:  # alternating, so that all see the same machine
        best.setdefault(name, []).append(sweep(name)[0])
for name, ts in best.items():
    dt = float(np.median(ts)) / n_distinct
    print(f"{name} extract_batch_device ({batch} resident scans per call, {n_distinct} distinct): {dt * 1e6:.2f} us per scan "
          f"({1 / dt:.0f} scans/s; median of {reps} sweeps, fastest {n_distinct / min(ts):.0f}, slowest {n_distinct / max(ts):.0f}), "
          f"{scans[0].size / dt / 1e9:.1f} GB/s of image bytes, {kps[name]:.0f} keypoints per scan")

imgs, az, _, _ = synth.polar_sequence(11, n_odo) if n_odo > 0 else (None, None, None, None)
for kp in ("kstrongest", "cfar") if n_odo > 0 else ():
    od = odometry.Odometry(400, 3360, keypoints=kp)
    res = od.push(imgs, az)
    best_t = 1e9
    for r in range(3):
        od.reset()
        t0 = time.perf_counter()
        res = od.push(imgs, az)
        best_t = min(best_t, time.perf_counter() - t0)
    print(f"odometry pipeline, {kp} keypoints: {n_odo / best_t:.0f} scans/s over {n_odo} scans "
          f"(mean {np.mean(res['n_keypoints']):.0f} keypoints, {np.mean(res['n_matches'][1:]):.0f} matches per scan)")
    od.close()
