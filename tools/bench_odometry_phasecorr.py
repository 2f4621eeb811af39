#!/usr/bin/env python3
"""Time the windowed odometry with and without phase correlation (rsx_odometry_set_phasecorr): one session, 256 distinct scans of the
400 x 3360 synthetic drive resident in HBM (344 MB: a sweep does not live in the Infinity Cache), pushed 64 scans at a time through
rsx_odometry_push_device; a sweep is `passes` runs over the 256 scans (reset before each), the figure the median of 7 sweeps with the
fastest and the slowest.  Configurations:
  (a) the default handle (cen2019 + ORORA) -- and, with --parent-tree DIR (a checkout of the parent commit with its librsx.so built),
      the same from that tree's package and library, in child processes before and after this build's, so that both are measured in
      one session;
  (b) phase correlation as the estimator at N = 256, beside the stand-alone rsx_phasecorr_register_batch_device on 64 pairs of 65 scans;
  (c) k-strongest + ORORA with the fallback off and on, on the clean drive: the cost of the spectra nobody ends up reading;
  (d) (c) with every eighth scan dimmed below the extractor's floor: two failed pairs in eight go to phase correlation.

usage: bench_odometry_phasecorr.py [--parent-tree DIR] [--scans 256] [--passes 8] [--reps 7] [--only a,b,c,d]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv:  # (internal) the tree whose package and library are timed
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)
PUSH = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree")
    ap.add_argument("--root", help="(internal)")
    ap.add_argument("--scans", type=int, default=256)
    ap.add_argument("--passes", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default="a,b,c,d")
    ap.add_argument("--images", help="(internal) a .npz of images and azimuths made by the parent process")
    ap.add_argument("--label", default="this build")
    args = ap.parse_args()
    only = set(args.only.split(","))
    assert args.scans % PUSH == 0 and args.scans >= 2 * PUSH

    from navtech_radar_slam_amd import synth
    if args.images:
        with np.load(args.images) as z:
            imgs, az = z["imgs"], z["az"]
    else:
        imgs, az, _, _ = synth.polar_sequence(11, args.scans)
        if args.parent_tree:  # the children time the same bytes
            tmp = tempfile.NamedTemporaryFile(suffix=".npz", delete=False)
            tmp.close()
            np.savez(tmp.name, imgs=imgs, az=az)

    def child(tree, label):
        env = {k: v for k, v in os.environ.items() if k != "RSX_LIB_PATH"}
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", tree, "--images", tmp.name, "--only", "a", "--label", label, "--scans", str(args.scans),
                            "--passes", str(args.passes), "--reps", str(args.reps)], env=env, capture_output=True, text=True, timeout=900)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:
            raise RuntimeError(label + " failed:\n" + r.stderr)

    if args.parent_tree and "a" in only:
        child(os.path.abspath(args.parent_tree), "parent build, before")

    import torch
    from navtech_radar_slam_amd import _rsx, odometry, phasecorr
    if _rsx.device_count() < 1:
        raise RuntimeError("needs a GPU: librsx has no CPU fallback")
    n = args.scans
    d_clean = torch.from_numpy(np.ascontiguousarray(imgs)).cuda()
    stride, off = imgs.strides[0], synth.OXFORD_META

    def run(label, d_imgs, **kw):
        od = odometry.Odometry(400, 3360, **kw)

        def one_pass():
            od.reset()
            return np.concatenate([od.push(imgs[lo:lo + PUSH], az, device_ptr=d_imgs.data_ptr() + lo * stride) for lo in range(0, n, PUSH)])

        def sweep():
            t0 = time.perf_counter()
            for _ in range(args.passes):
                one_pass()  # (rsx_odometry_push_device is synchronous: it returns with the window's records)
            return time.perf_counter() - t0

        res = one_pass()  # warm-up: the buffers are reserved here
        sweep()
        ts = np.array([sweep() for _ in range(args.reps)]) / (args.passes * n)
        od.close()
        rec = dict(config=label, build=args.label, scans_per_s=round(1.0 / float(np.median(ts))), fastest=round(1.0 / float(ts.min())),
                   slowest=round(1.0 / float(ts.max())), us_per_scan=round(float(np.median(ts)) * 1e6, 2), failed=int((res["status"][1:] != 0).sum()),
                   phasecorr_records=int((res["iterations"][1:] < 0).sum()), scans=n, passes=args.passes, reps=args.reps)
        print(json.dumps(rec), flush=True)
        return rec

    if "a" in only:
        run("a default (cen2019 + ORORA)", d_clean)
    if "b" in only:
        run("b estimator=phasecorr N=256", d_clean, estimator="phasecorr")
        # the stand-alone entry on the same scans: 64 pairs of 65 scans per call, as tools/bench_phasecorr.py
        h = phasecorr.Phasecorr(400, 3360)
        calls = [lo for lo in range(0, n - PUSH, PUSH + 1)]
        d_pairs = torch.tensor([(i + 1, i) for i in range(PUSH)], dtype=torch.int32, device="cuda")
        d_res = torch.zeros(PUSH * 56, dtype=torch.uint8, device="cuda")
        s = torch.cuda.current_stream().cuda_stream

        def sweep():
            t0 = time.perf_counter()
            for _ in range(args.passes):
                for lo in calls:
                    h.register_batch_device(d_clean.data_ptr() + lo * stride, PUSH + 1, stride, imgs.strides[1], off, d_pairs.data_ptr(), PUSH, d_res.data_ptr(),
                                            stream=s)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        sweep()
        ts = np.array([sweep() for _ in range(args.reps)]) / (args.passes * len(calls) * PUSH)
        h.close()
        print(json.dumps(dict(config="b stand-alone register_batch_device, 64 pairs of 65 scans per call", build=args.label,
                              pairs_per_s=round(1.0 / float(np.median(ts))), fastest=round(1.0 / float(ts.min())), slowest=round(1.0 / float(ts.max())),
                              us_per_pair=round(float(np.median(ts)) * 1e6, 2), calls=len(calls), passes=args.passes, reps=args.reps)), flush=True)
    if "c" in only:
        run("c kstrongest + ORORA, fallback off, clean", d_clean, keypoints="kstrongest")
        run("c kstrongest + ORORA, fallback on, clean", d_clean, keypoints="kstrongest", fallback="phasecorr")
    if "d" in only:
        dim = imgs.copy()
        for i in range(4, n, 8):  # below z_min = 60: the extractor finds nothing, the pairs (i, i - 1) and (i + 1, i) fail
            p = dim[i, :, off:].astype(np.float64)
            dim[i, :, off:] = np.floor(p * (59.0 / p.max())).astype(np.uint8)
        d_dim = torch.from_numpy(dim).cuda()
        run("d kstrongest + ORORA, fallback off, every eighth scan dimmed", d_dim, keypoints="kstrongest")
        run("d kstrongest + ORORA, fallback on, every eighth scan dimmed", d_dim, keypoints="kstrongest", fallback="phasecorr")
    if args.parent_tree and "a" in only:
        child(os.path.abspath(args.parent_tree), "parent build, after")
        os.unlink(tmp.name)


if __name__ == "__main__":
    main()
