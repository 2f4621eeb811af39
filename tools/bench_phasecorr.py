#!/usr/bin/env python3
"""Time the phase-correlation registration (rsx_phasecorr_register_batch_device): 64 pairs per call, the pairs being consecutive scans
of the 400 x 3360 synthetic drive, all resident in HBM; a call transforms its 65 scans once and registers the 64 pairs (both
half-turn candidates).  130 distinct scans (175 MB of polar images, beside 49 MB of scan slots and 160 MB of pair workspace per call at
N = 256) so that a sweep does not live in the Infinity Cache.  Prints microseconds per pair and the errors against the drive's known
motion.  No earlier GPU form exists to compare with.

usage: bench_phasecorr.py [n=256] [resolution=128/n] [n_scans=130] [reps=7]"""
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from navtech_radar_slam_amd import _rsx, phasecorr, synth  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
resolution = float(sys.argv[2]) if len(sys.argv) > 2 else 128.0 / n
n_scans = int(sys.argv[3]) if len(sys.argv) > 3 else 130
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 7
batch = 64
n_calls = n_scans // (batch + 1)
assert n_calls >= 2, "at least 130 scans: two calls of 64 pairs over 65 scans each"

import torch  # noqa: E402

imgs, _, poses, _ = synth.polar_sequence(11, n_scans)
h = phasecorr.Phasecorr(400, 3360, phasecorr.params(n=n, resolution=resolution))
d_pairs = torch.tensor([(i + 1, i) for i in range(batch)], dtype=torch.int32, device="cuda")
calls = []
for c in range(n_calls):
    lo = c * (batch + 1)
    calls.append(dict(lo=lo, imgs=torch.from_numpy(np.ascontiguousarray(imgs[lo:lo + batch + 1])).cuda(),
                      res=torch.zeros(batch * 56, dtype=torch.uint8, device="cuda")))
stream = torch.cuda.current_stream().cuda_stream
stride, row_stride = imgs.strides[0], imgs.strides[1]
print(f"{n_calls * batch} distinct pairs of {n_calls * (batch + 1)} scans, N = {n} at {resolution} m per pixel, {n_calls} calls of {batch} pairs")


def sweep():
    t0 = time.perf_counter()
    for c in calls:
        h.register_batch_device(c["imgs"].data_ptr(), batch + 1, stride, row_stride, synth.OXFORD_META, d_pairs.data_ptr(), batch, c["res"].data_ptr(),
                                stream=stream)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


sweep()  # warm-up: the workspace grows here
ex, et = [], []
for c in calls:
    res = np.frombuffer(c["res"].cpu().numpy().tobytes(), dtype=_rsx.PHASECORR_RESULT_DTYPE)
    for i in range(batch):
        want = synth.relative_pose(poses[c["lo"] + i], poses[c["lo"] + i + 1])
        ex.append(math.hypot(res["x"][i] - want[0], res["y"][i] - want[1]))
        et.append(abs((res["theta"][i] - want[2] + math.pi) % (2 * math.pi) - math.pi))
    assert not res["status"].any()
print(f"against the drive: translation error median {np.median(ex):.3f} m, max {max(ex):.3f} m; rotation error median {np.median(et):.4f} rad, "
      f"max {max(et):.4f} rad (a pixel is {resolution} m, an angle bin {math.pi / n:.4f} rad)")
ts = [sweep() for _ in range(reps)]
dt = float(np.median(ts))
pairs = n_calls * batch
print(f"phasecorr register_batch_device ({batch} pairs and {batch + 1} scans per call, {pairs} distinct pairs): {dt / pairs * 1e6:.1f} us per pair "
      f"(median of {reps} sweeps; fastest {min(ts) / pairs * 1e6:.1f}, slowest {max(ts) / pairs * 1e6:.1f}), {pairs / dt:.0f} pairs/s")
h.close()
