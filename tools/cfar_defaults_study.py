#!/usr/bin/env python3
"""The defaults study of rsx_cfar_* (include/rsx.h): scale_q8 x offset through the CPU chain -- restatement (tests/cfar_np.py) ->
oracle front end -> cross-checked ratio matches -> max-clique selection -> ORORA -- on synth.polar_sequence(11, 5), with
k-strongest's defaults as the row to compare with.  CPU only; one process per setting.

  python tools/cfar_defaults_study.py [--jobs 13]"""
import argparse
import multiprocessing as mp
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SCALES = (512, 768, 1024, 1536)
OFFSETS = (0, 20, 40)


def one(setting):
    import cfar_np
    import keypoint_chain
    import kstrongest_np
    from navtech_radar_slam_amd import synth
    imgs, az, poses, _ = synth.polar_sequence(11, 5)
    if setting is None:
        name, extract = "k-strongest z_min=60", lambda img: kstrongest_np.extract(img)
    else:
        name, extract = "A=%d B=%d" % setting, lambda img: cfar_np.extract(img, scale_q8=setting[0], offset=setting[1])
    out = keypoint_chain.run(extract, imgs, az)
    status, wt, wy = keypoint_chain.pair_errors(out, poses)
    kp = [c["n_keypoints"] for c in out]
    nm = [c["n_matches"] for c in out[1:]]
    return name, min(kp), max(kp), min(nm), max(nm), status, wt, wy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=13)
    args = ap.parse_args()
    from oracle import pyoracle
    pyoracle.build()
    settings = [None] + [(a, b) for a in SCALES for b in OFFSETS]
    with mp.get_context("spawn").Pool(args.jobs) as pool:
        rows = pool.map(one, settings)
    print("%-22s %-13s %-11s %-10s %s" % ("setting", "keypoints", "matches", "statuses", "worst pair error"))
    for name, k0, k1, m0, m1, status, wt, wy in rows:
        print("%-22s %5d - %-5d %4d - %-4d %-10s %.3f m / %.1e rad" % (name, k0, k1, m0, m1, "".join(map(str, status)), wt, wy))


if __name__ == "__main__":
    main()
