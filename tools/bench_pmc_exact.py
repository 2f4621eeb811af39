"""The max-clique inlier selection alone, greedy (RSX_ORORA_PMC) against exact (| RSX_ORORA_PMC_EXACT), alternated in one
session: ms per batch on the bench batch (3 500 pairs of 300-1500 matches) and on the high-outlier family, the share of pairs
whose clique grew / was left to the search, and the flags.  `--restate N` also counts the search nodes of the first N pairs
of each batch on the CPU (tests/pmc_exact_np.py).  One JSON line per batch."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from navtech_radar_slam_amd import _rsx, orora, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=3500)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--restate", type=int, default=0)
args = ap.parse_args()

reg = orora.Orora()
st = torch.cuda.current_stream().cuda_stream


def leg(name, data):
    src, dst, off, _ = data
    n = len(off) - 1
    d_src, d_dst, d_off = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda(), torch.from_numpy(off).cuda()
    d_m = torch.zeros(len(src), dtype=torch.uint8, device="cuda")
    d_i = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    p = {}
    for k, fl in (("greedy", _rsx.ORORA_PMC), ("exact", _rsx.ORORA_PMC | _rsx.ORORA_PMC_EXACT)):
        p[k] = orora.default_params()
        p[k].flags |= fl

    def run(k):
        check = reg._L.rsx_orora_max_clique_batch_device(reg._h, d_src.data_ptr(), d_dst.data_ptr(), d_off.data_ptr(), n, p[k], d_m.data_ptr(), d_i.data_ptr(), st)
        assert check == 0
        torch.cuda.synchronize()

    times = {"greedy": [], "exact": []}
    infos = {}
    for rep in range(args.reps + 1):          # the first round warms up; then greedy / exact alternate
        for k in ("greedy", "exact"):
            t = time.perf_counter()
            run(k)
            if rep:
                times[k].append((time.perf_counter() - t) * 1e3)
            infos[k] = d_i.cpu().numpy().copy()
    g, e = infos["greedy"], infos["exact"]
    out = {"batch": name, "pairs": n, "matches": int(off[-1]),
           "greedy_ms": [round(t, 3) for t in times["greedy"]], "exact_ms": [round(t, 3) for t in times["exact"]],
           "greedy_ms_median": round(float(np.median(times["greedy"])), 3), "exact_ms_median": round(float(np.median(times["exact"])), 3),
           "pairs_grown": int((e[:, 0] > g[:, 0]).sum()), "largest_growth": int((e[:, 0] - g[:, 0]).max()),
           "pairs_proven_by_core_bound": int((g[:, 3] & 1 != 0).sum()),
           "pairs_maximum": int((e[:, 3] & 8 != 0).sum()), "pairs_budget": int((e[:, 3] & 16 != 0).sum())}
    if args.restate:
        import pmc_exact_np as ex
        from oracle import pyoracle as po
        po.build()
        k = min(args.restate, n)
        _, winfo, nodes = ex.exact_batch(po, src[:off[k]], dst[:off[k]], off[:k + 1], p["exact"].tim_noise_bound)
        out["restated_pairs"] = k
        out["restated_pairs_in_search"] = int((nodes > 0).sum())
        out["restated_largest_node_count"] = int(nodes.max())
        out["restated_sizes_equal"] = bool(np.array_equal(winfo["size"], e[:k, 0]))
    print(json.dumps(out), flush=True)


leg("bench", synth.orora_pairs(777, args.pairs))
leg("high_outlier", synth.orora_high_outlier_pairs(6, args.pairs))
