#!/usr/bin/env python3
"""Time the radar scan-context builder (rsx_radarsc_*): the batched device entry on 64-scan batches that cycle through >= 256
distinct MulRan-shape scans resident in HBM (400 x 3371 bytes each: > 256 MiB in all, past the Infinity Cache), the latency of
a single scan, build + insert (rsx_sc_add_polar_batch_device), the batched host entry, and -- for comparison -- the existing
route to a descriptor for the same scans: rsx_cen2019_extract_batch_device, then rsx_sc_add_points per scan.  Prints scans/s and
the share of the HBM peak on the bytes the rule needs (rows x ring-covered bins + the descriptors).

usage: bench_radarsc.py [n_distinct=256] [reps=20] [kernel_only=0]   (kernel_only=1: the device entry alone, for a profiler run)"""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from navtech_radar_slam_amd import _rsx, cen2019, radar_context, scancontext, synth  # noqa: E402

n_distinct = int(sys.argv[1]) if len(sys.argv) > 1 else 256
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
kernel_only = len(sys.argv) > 3 and sys.argv[3] == "1"
batch = 64
HBM_PEAK = 8.0e12   # bytes/s, MI355X HBM3E specification (a float4 copy measures 6.29e12)
assert n_distinct % batch == 0 and n_distinct >= 256

import torch  # noqa: E402

# distinct scans: 16 synthetic worlds, each rolled in azimuth and sprinkled with its own noise
rng = np.random.default_rng(2020)
base = [synth.polar_image(300 + i, n_targets=1200) for i in range(16)]
az = base[0][1]
scans = np.empty((n_distinct,) + base[0][0].shape, dtype=np.uint8)
for i in range(n_distinct):
    s = np.roll(base[i % 16][0], 7 * (i // 16), axis=0).copy()
    idx = rng.integers(0, s.size, 4000)
    s.flat[idx] = rng.integers(0, 120, idx.size).astype(np.uint8)
    scans[i] = s
rows, stride = scans.shape[1], scans.shape[2]
cols = stride - 11
p = radar_context.default_params()
ring_bins = int(np.floor(p.max_radius / np.float64(np.float32(p.resolution)) - 0.5)) + 1 - p.min_range   # bins min_range .. last inside max_radius
need = rows * ring_bins + 4800
print(f"{n_distinct} distinct scans, {scans.nbytes / 2**20:.0f} MiB resident; the rule needs {need} B per scan ({ring_bins} bins x {rows} rows + 4800)")
ctx = radar_context.RadarContext(rows, cols)
d = torch.from_numpy(scans).cuda()
daz = torch.from_numpy(az).cuda()
out = torch.zeros((batch, 1200), dtype=torch.float32, device="cuda")
s = torch.cuda.current_stream().cuda_stream
nb = n_distinct // batch


def run(b, n=batch):
    ctx.build_batch_device(d.data_ptr() + b * batch * scans.strides[0], n, scans.strides[0], stride, daz.data_ptr(), out.data_ptr(), stream=s)


def timed(fn, count, reps=reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (reps * count)


dt = timed(lambda: [run(b) for b in range(nb)], n_distinct)
print(f"radarsc build_batch_device ({batch} resident scans per call, {n_distinct} distinct): {dt * 1e6:.3f} us per scan ({1 / dt:.0f} scans/s), "
      f"{need / dt / 1e12:.3f} TB/s of needed bytes = {100 * need / dt / HBM_PEAK:.1f} % of the {HBM_PEAK / 1e12:.0f} TB/s HBM peak")
if kernel_only:
    sys.exit(0)
single = []
for i in range(50):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run((i * 37) % nb, 1)
    torch.cuda.synchronize()
    single.append(time.perf_counter() - t0)
print(f"radarsc single scan, call to synchronised (distinct scans): median {np.median(single) * 1e6:.1f} us, best {min(single) * 1e6:.1f} us")
g = scancontext.SCManager(capacity_hint=n_distinct * 4)
dt = timed(lambda: [g.add_polar_batch_device(ctx, d.data_ptr() + b * batch * scans.strides[0], batch, scans.strides[0], stride, daz.data_ptr(), stream=s)
                    for b in range(nb)], n_distinct, reps=3)
print(f"radarsc build + insert (rsx_sc_add_polar_batch_device, {batch} scans per call): {dt * 1e6:.2f} us per scan ({1 / dt:.0f} scans/s), "
      f"{len(g)} keyframes")
host = scans[:batch]
dt = timed(lambda: ctx.build_batch(host, az), batch, reps=3)
print(f"radarsc build_batch (host buffers, {batch} scans per call): {dt * 1e3:.4f} ms per scan ({1 / dt:.0f} scans/s)")

# ---- the existing route to a descriptor for the same scans: cen2019 keypoints on the device, then rsx_sc_add_points per scan ----
c = cen2019.Cen2019(rows, cols)
L = _rsx.lib()
mt = 20000
tg = torch.zeros((batch, mt, 2), dtype=torch.int32, device="cuda")
xy = torch.zeros((batch, mt, 2), dtype=torch.float32, device="cuda")
cnt = torch.zeros(batch, dtype=torch.int32, device="cuda")
cp = cen2019.default_params()


def extract(b):
    _rsx.check(L.rsx_cen2019_extract_batch_device(c._h, d.data_ptr() + b * batch * scans.strides[0], batch, scans.strides[0], stride, 11, C.byref(cp),
                                                  daz.data_ptr(), 0, 0.0595, tg.data_ptr(), xy.data_ptr(), mt, cnt.data_ptr(), C.c_void_p(s)))


dt_x = timed(lambda: [extract(b) for b in range(nb)], n_distinct, reps=3)
counts = cnt.cpu().numpy()
pts = xy.cpu().numpy()
clouds = [np.concatenate([pts[i, :min(counts[i], mt)], np.zeros((min(counts[i], mt), 1), np.float32)], axis=1) for i in range(batch)]
g2 = scancontext.SCManager(capacity_hint=4096)
t0 = time.perf_counter()
for cl in clouds:
    g2.makeAndSaveScancontextAndKeys(cl)
len(g2)
g2.export_descriptors_f32(0, 1)   # synchronises the inserts
dt_a = (time.perf_counter() - t0) / batch
print(f"existing route: cen2019 extract_batch_device {dt_x * 1e6:.2f} us per scan + rsx_sc_add_points {dt_a * 1e6:.2f} us per scan "
      f"(mean {counts.mean():.0f} keypoints) = {(dt_x + dt_a) * 1e6:.2f} us per scan ({1 / (dt_x + dt_a):.0f} scans/s)")
