#!/usr/bin/env python3
"""Defaults study of the CorAl alignment quality, on the CPU and on the restatement only (tests/coral_np.py): over the synthetic
drive of tests/cfear_track_cases.drive() (400 x 3360 scans, about 4800 k-strongest points each) and its small sequence (64 x 512,
768 points each), Q at the true relative pose for scan gaps 1, 2 and 4, and at that pose displaced by 0.25, 0.5 and 1 m (along x
and along y of the earlier scan's frame) and by 1, 2 and 5 degrees.  Prints the table of DESIGN.md 4.6l and the threshold X that
best separates "true" from "0.5 m or more off" (fewest misses + false alarms), a suggestion for pgo_replay --max-quality.
NO REAL RADAR DATA IS USED: the numbers describe the synthetic scenes of navtech_radar_slam_amd/synth.py.

usage: coral_study.py"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import coral_cases as cc  # noqa: E402
import coral_np as co  # noqa: E402

GAPS = (1, 2, 4)
SHIFTS = [("true", (0.0, 0.0, 0.0))]
for d in (0.25, 0.5, 1.0):
    SHIFTS += [(f"{d:g} m", (d, 0.0, 0.0)), (f"{d:g} m", (0.0, d, 0.0))]
for deg in (1, 2, 5):
    SHIFTS += [(f"{deg} deg", (0.0, 0.0, math.radians(deg)))]
COLUMNS = ["true", "0.25 m", "0.5 m", "1 m", "1 deg", "2 deg", "5 deg"]

samples = {}   # (sequence, gap, column) -> [Q]
scored = {}    # (sequence, gap) -> [scored / valid at the true pose]
for name, (clouds, poses) in (("drive", cc.drive_clouds()), ("small", cc.small_clouds())):
    for gap in GAPS:
        for i in range(len(clouds) - gap):
            p = cc.true_pose(poses, i, i + gap)
            for col, s in SHIFTS:
                res, _ = co.quality(clouds[i], clouds[i + gap], co.pose_matrix(p + np.array(s)))
                samples.setdefault((name, gap, col), []).append(float(res["quality"]))
                if col == "true":
                    scored.setdefault((name, gap), []).append(res["n_scored"] / max(int(res["n_valid"]), 1))

print("| sequence | gap | pairs | scored | " + " | ".join(COLUMNS) + " |")
print("|---|---|---|---|" + "---|" * len(COLUMNS))
for name in ("drive", "small"):
    for gap in GAPS:
        cells = []
        for col in COLUMNS:
            q = samples[(name, gap, col)]
            cells.append(f"{np.median(q):.3f} [{min(q):.3f}, {max(q):.3f}]")
        print(f"| {name} | {gap} | {len(samples[(name, gap, 'true')])} | {100 * min(scored[(name, gap)]):.1f} % | " + " | ".join(cells) + " |")



def pick(which):
    """the Q of the true poses and of the poses 0.5 m or more off, over the sequences in `which`"""
    true = np.array([q for (n, g, c), qs in samples.items() if c == "true" and n in which for q in qs])
    off = np.array([q for (n, g, c), qs in samples.items() if c in ("0.5 m", "1 m") and n in which for q in qs])
    return true, off


print()
for which in (("drive", "small"), ("drive",), ("small",)):
    true, off = pick(which)
    best = None
    for x in np.unique(np.concatenate([true, off])):
        miss, alarm = int((off <= x).sum()), int((true > x).sum())
        if best is None or miss + alarm < best[1] + best[2]:
            best = (float(x), miss, alarm)
    # any X between the best cut and the next sample above it separates equally well: report the middle of that gap
    above = np.concatenate([true, off])
    above = above[above > best[0]]
    x = (best[0] + float(above.min())) / 2 if len(above) else best[0]
    print(f"{' + '.join(which)}: {len(true)} true poses (Q max {true.max():.3f}), {len(off)} poses 0.5 m or more off (Q min {off.min():.3f}): X = {x:.3f} "
          f"misses {best[1]} of the displaced ones (Q <= X) and raises {best[2]} false alarms on the true ones (Q > X)")
print("no real radar data was used")
