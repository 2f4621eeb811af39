"""Scan pairs per second of rigid RANSAC and motion-compensated RANSAC (csrc/ransac.hip, device entry) beside ORORA and
ORORA + max-clique selection on the same pairs in the same process: synth.orora_pairs(777, 3500), one dt for every match
in the MC leg (the pairs are rigid).  `--odometry [n_unique n_scans]` adds the windowed odometry's scans/s with each estimator
(images resident in HBM, as tools/bench_odometry.py).  Every timed leg runs under its own time limit (LEG_TIMEOUT seconds,
default 120): a leg that overruns ends the process with status 124 and nothing more is started."""
import os
import sys
import threading
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from navtech_radar_slam_amd import _rsx, odometry, orora, ransac, synth  # noqa: E402

LEG_TIMEOUT = float(os.environ.get("LEG_TIMEOUT", 120))


def leg(name, fn):
    """fn() -> text, under the time limit"""
    box = {}

    def run():
        try:
            box["out"] = fn()
        except BaseException as e:  # noqa: BLE001 -- reported below, the process ends
            box["err"] = repr(e)

    t = threading.Thread(target=run, daemon=True)
    t.start()
    t.join(LEG_TIMEOUT)
    if t.is_alive():
        print(f"{name}: no result within {LEG_TIMEOUT:.0f} s", flush=True)
        os._exit(124)
    if "err" in box:
        print(f"{name}: failed: {box['err']}", flush=True)
        os._exit(1)
    print(f"{name}: {box['out']}", flush=True)


def timed(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def main():
    n_pairs = int(os.environ.get("PAIRS", 3500))
    src, dst, off, truth = synth.orora_pairs(777, n_pairs)
    dt = np.full(len(src), 0.25, dtype=np.float32)
    reg, est = orora.Orora(), ransac.Ransac()
    reg.reserve(int(off[-1]))
    d_src, d_dst, d_dt, d_off = (torch.from_numpy(a).cuda() for a in (src, dst, dt, off))
    d_res = torch.zeros(n_pairs * _rsx.RANSAC_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    print(f"pairs {n_pairs}  matches {int(off[-1])}")

    def orora_leg(params):
        t = timed(lambda: reg.register_batch_device(d_src.data_ptr(), d_dst.data_ptr(), d_off.data_ptr(), n_pairs, d_res.data_ptr(), params, stream=st))
        return f"{t * 1e3:.3f} ms  {n_pairs / t:.0f} pairs/s"

    def ransac_leg(mc):
        prm = ransac.default_params(mc=mc)
        t = timed(lambda: est.estimate_batch_device(d_src.data_ptr(), d_dst.data_ptr(), d_dt.data_ptr() if mc else None, d_off.data_ptr(), n_pairs,
                                                    d_res.data_ptr(), None, prm, stream=st))
        res = d_res.cpu().numpy().view(_rsx.RANSAC_RESULT_DTYPE)
        err = np.hypot(res["x"] - truth[:, 0], res["y"] - truth[:, 1])
        return (f"{t * 1e3:.3f} ms  {n_pairs / t:.0f} pairs/s  (status 0: {np.mean(res['status'] == 0):.3f}, median error {np.median(err):.4f} m "
                f"{np.median(np.abs(res['yaw'] - truth[:, 2])):.2e} rad, hypotheses {res['hypotheses'].mean():.1f})")

    p_pmc = orora.default_params()
    p_pmc.flags |= _rsx.ORORA_PMC
    leg("ORORA", lambda: orora_leg(None))
    leg("ORORA + max-clique selection", lambda: orora_leg(p_pmc))
    leg("RANSAC", lambda: ransac_leg(False))
    leg("MC-RANSAC", lambda: ransac_leg(True))
    if "--odometry" in sys.argv:
        a = sys.argv[sys.argv.index("--odometry") + 1:]
        n_unique, n_scans = (int(a[0]), int(a[1])) if len(a) >= 2 else (8, 256)
        imgs, az, _, _ = synth.polar_sequence(11, n_unique)
        order = [abs((i + n_unique - 1) % (2 * n_unique - 2) - (n_unique - 1)) for i in range(n_scans)] if n_unique > 1 else [0] * n_scans
        seq = np.ascontiguousarray(imgs[np.asarray(order)])
        d = torch.from_numpy(seq).cuda()
        od = odometry.Odometry(400, 3360)
        od.push(seq[:200], az)

        def odo_leg(name):
            od.reset()
            od.set_estimator(name)
            od.push(seq[:64], az, device_ptr=d.data_ptr())
            best = []
            for _ in range(9):
                od.reset()
                t0 = time.perf_counter()
                res = od.push(seq, az, device_ptr=d.data_ptr())
                best.append(n_scans / (time.perf_counter() - t0))
            return f"{np.median(best):.0f} scans/s (median of 9; min {min(best):.0f}, max {max(best):.0f}), status 0 on {np.mean(res['status'][1:] == 0):.3f} of the pairs"

        for name in ("orora", "ransac", "mcransac"):
            leg(f"odometry, {n_scans} resident scans, estimator {name}", lambda name=name: odo_leg(name))


if __name__ == "__main__":
    main()
