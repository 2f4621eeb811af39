#!/usr/bin/env python3
"""Time CFEAR's registration (pairs and scan-to-keyframes) and keyframe tracker (csrc/cfear_track.hip), and reproduce the accuracy
table of the tracking rules, in one session.

The inputs are the surface points of the k-strongest clouds (k = 12, z_min = 60, min_separation = 0) of >= 256 consecutive scans
of the synthetic drive synth.polar_sequence(11, n), MulRan shape (400 x 3360).  Through the device entries on resident buffers,
64 jobs per call cycling through all scans, alternating the variants sweep by sweep:
  (a) the 64 consecutive pairs with rsx_cfear_register_batch_device (the pair entry's own time: the same kernel as K = 1,
      search 0) and as K = 1 jobs at the identity pose with rsx_cfear_register_keyframes_batch_device, search 0 (cell index) and
      search 1 (brute force)
  (b) K = 3 jobs (scan i + 3 against scans i, i + 1, i + 2 at their tracked poses, started at scan i + 2's), both searches
  (c) the tracker: one sequence of all scans in one push, and 16 sequences at once
  (d) the windowed odometry (rsx_odometry_push, host images) with k-strongest + CFEAR, tracking on and off
  (e) accuracy against the true poses: consecutive pairs from the identity, 3 keyframes started at the previous pose, 3 keyframes
      started at the constant-velocity prediction
  (f) the timed tracker (rsx_cfear_tracker_push_timed_device, the records' times from rsx_cfear_surface_points_timed_batch) with
      compensate = 0 and compensate = 1, alternating with the untimed tracker of (c), one sequence and 16; and the odometry of (d)
      with compensation on.  The synthetic images are not distorted by the motion, so (f) measures cost, not accuracy
  (g) the objectives (rsx_cfear_params.cost x loss x weights, 18 combinations; the first row is the default's, measured in the same
      run): the pairs of (a) through rsx_cfear_register_batch_device, the combinations alternating sweep by sweep, and the
      3-keyframe tracker of (c); per combination the time per 64 jobs, mean iterations, status 8, pairs more than 0.7 m off, the
      median pair error and the end-of-trajectory error, as a table.  Reported, not gated.  objectives = 0 leaves (g) out (a
      library from before the objectives ignores the three words)
Prints microseconds per call and scans/s; every timed window ends in a device synchronise.

usage: bench_cfear_track.py [n_scans=256] [reps=5] [odometry_reps=3] [objectives=1]"""
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from navtech_radar_slam_amd import _rsx, cfear, kstrongest, odometry, synth  # noqa: E402

n_scans = int(sys.argv[1]) if len(sys.argv) > 1 else 256
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
odo_reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
objectives = int(sys.argv[4]) if len(sys.argv) > 4 else 1
batch = 64
assert n_scans % batch == 0 and n_scans >= 2 * batch

import torch  # noqa: E402

SP = _rsx.CFEAR_SURFACE_POINT_DTYPE
t0 = time.perf_counter()
imgs, az, poses, _ = synth.polar_sequence(11, n_scans)
print(f"{n_scans} consecutive scans generated in {time.perf_counter() - t0:.0f} s", flush=True)
ks = kstrongest.KStrongest(400, 3360)
h = cfear.Cfear()
records, taus = [], []
for b in range(0, n_scans, batch):
    tg, xy = ks.extract_batch(imgs[b:b + batch], min_separation=0, azimuths=az if np.ndim(az) == 1 else az[b:b + batch])
    records += h.surface_points(xy)[0]
    timed_rec, tau, _, _ = h.surface_points_timed(xy, [np.ascontiguousarray(t[:, 0]) for t in tg], 400)
    assert all(a.tobytes() == b_.tobytes() for a, b_ in zip(timed_rec, records[b:]))
    taus += tau
print(f"surface points: {np.mean([len(r) for r in records]):.0f} per scan (min {min(len(r) for r in records)}, max {max(len(r) for r in records)})", flush=True)
stream = torch.cuda.current_stream().cuda_stream
nb = n_scans // batch


def dev(a):
    return torch.from_numpy(a.view(np.uint8) if a.dtype.fields else np.ascontiguousarray(a)).cuda()


def compose(a, b):
    c, s = math.cos(a[2]), math.sin(a[2])
    return (a[0] + (c * b[0] - s * b[1]), a[1] + (s * b[0] + c * b[1]), a[2] + b[2])


def between(a, b):
    c, s = math.cos(a[2]), math.sin(a[2])
    dx, dy = b[0] - a[0], b[1] - a[1]
    return (c * dx + s * dy, c * dy - s * dx, b[2] - a[2])


# ---- (c) first: the tracked poses are (b)'s keyframe poses ----
def run_tracker(n_seq, tp, rounds, prm=None):
    t = cfear.Tracker(n_seq, params=prm, track=tp)
    rec, off = cfear.ragged(records * n_seq, SP)
    d = [dev(rec), dev(off), dev(np.full(n_seq, n_scans, dtype=np.int32))]
    d_out = torch.zeros(n_seq * n_scans * 80, dtype=torch.uint8, device="cuda")
    ts = []
    for r in range(rounds + 1):  # (the first is the warm-up)
        t.reset(params=prm, track=tp)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t.push_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d_out.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    out = d_out.cpu().numpy().view(_rsx.CFEAR_TRACK_RESULT_DTYPE).reshape(n_seq, n_scans)
    t.close()
    return out, ts[1:]


track_out = {}
for s in (0, 1):
    for n_seq in (1, 16):
        out, ts = run_tracker(n_seq, cfear.track_params(search=s), reps)
        assert all(out[q].tobytes() == out[0].tobytes() for q in range(n_seq))
        track_out[s] = out[0]
        print(f"(c) tracker, search {s}, {n_seq} sequence(s) of {n_scans} scans in one push: {np.median(ts) * 1e3:.1f} ms (fastest {min(ts) * 1e3:.1f}, slowest "
              f"{max(ts) * 1e3:.1f}; median of {reps}) = {n_seq * n_scans / np.median(ts):.0f} scans/s, {np.median(ts) / n_scans * 1e6:.0f} us per scan of a sequence",
              flush=True)
assert track_out[0].tobytes() == track_out[1].tobytes()
tracked = track_out[0]
pose = [(float(r["x"]), float(r["y"]), float(r["yaw"])) for r in tracked]



# ---- (f) the timed tracker, compensation off and on, against the untimed one: alternating ----
def make_leg(n_seq, tp, timed_push):
    t = cfear.Tracker(n_seq, track=tp)
    rec, off = cfear.ragged(records * n_seq, SP)
    d = [dev(rec), dev(off), dev(np.full(n_seq, n_scans, dtype=np.int32)), dev(np.concatenate(taus * n_seq))]
    d_out = torch.zeros(n_seq * n_scans * 80, dtype=torch.uint8, device="cuda")

    def run():
        t.reset(track=tp)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if timed_push:
            t.push_timed_device(d[0].data_ptr(), d[3].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d_out.data_ptr(), stream=stream)
        else:
            t.push_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d_out.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    return run, d_out, t


for n_seq in (1, 16):
    legs = {"untimed push": make_leg(n_seq, cfear.track_params(), False), "timed push, compensate 0": make_leg(n_seq, cfear.track_params(), True),
            "timed push, compensate 1": make_leg(n_seq, cfear.track_params(compensate=1), True)}
    for run, _, _ in legs.values():
        run()  # warm-up
    ts = {k: [] for k in legs}
    for r in range(reps):
        for k, (run, _, _) in legs.items():  # alternating
            ts[k].append(run())
    base = float(np.median(ts["untimed push"]))
    res = {k: v[1].cpu().numpy().view(_rsx.CFEAR_TRACK_RESULT_DTYPE).reshape(n_seq, n_scans)[0] for k, v in legs.items()}
    assert res["timed push, compensate 0"].tobytes() == res["untimed push"].tobytes() == tracked.tobytes()
    for k, v in ts.items():
        m = float(np.median(v))
        print(f"(f) tracker, {k}, {n_seq} sequence(s) of {n_scans} scans: {m * 1e3:.1f} ms (fastest {min(v) * 1e3:.1f}, slowest {max(v) * 1e3:.1f}; "
              f"median of {reps}) = {m / n_scans * 1e6:.0f} us per scan of a sequence, {m / base:.2f} x the untimed push", flush=True)
    o = res["timed push, compensate 1"]
    print(f"    compensate 1: iterations mean {o['reg']['reserved'][1:].mean():.1f} (pass 1) + {o['reg']['iterations'][1:].mean():.1f} (pass 2) against "
          f"{tracked['reg']['iterations'][1:].mean():.1f} without; status != 0: {int(np.sum(o['reg']['status'][1:] != 0))}, keyframes "
          f"{int(np.sum(o['keyframe'] == 1))}, re-anchored {int(np.sum(o['keyframe'] == 2))}", flush=True)
    for _, _, t in legs.values():
        t.close()

# ---- (a) and (b): batches of 64 jobs ----
pairs = [(records[(i + 1) % n_scans], records[i]) for i in range(n_scans)]  # (the last pair wraps round: far apart, status 4 at once)
d_pairs, d_k1, d_k3 = [], [], []
for b in range(nb):
    sl = range(b * batch, (b + 1) * batch)
    s, so = cfear.ragged([pairs[i][0] for i in sl], SP)
    d, do = cfear.ragged([pairs[i][1] for i in sl], SP)
    d_pairs.append([dev(a) for a in (s, so, d, do)])
    d_k1.append([dev(np.arange(batch + 1, dtype=np.int64)), dev(np.zeros((batch, 3)))])
    src3 = [records[(i + 3) % n_scans] for i in sl]
    kf3 = [records[(i + j) % n_scans] for i in sl for j in range(3)]
    kp3 = np.array([pose[(i + j) % n_scans] for i in sl for j in range(3)])
    init3 = np.array([pose[(i + 2) % n_scans] for i in sl])
    s3, so3 = cfear.ragged(src3, SP)
    k3, ko3 = cfear.ragged(kf3, SP)
    d_k3.append([dev(a) for a in (s3, so3, k3, ko3, np.arange(0, 3 * batch + 1, 3, dtype=np.int64), kp3, init3)])
d_res = {k: [torch.zeros(batch * 48, dtype=torch.uint8, device="cuda") for _ in range(nb)] for k in ("pair", "k1s0", "k1s1", "k3s0", "k3s1")}
tps = [cfear.track_params(search=0), cfear.track_params(search=1)]


def sweep_pair():
    for b in range(nb):
        s, so, d, do = d_pairs[b]
        h.register_device(s.data_ptr(), so.data_ptr(), d.data_ptr(), do.data_ptr(), batch, d_res["pair"][b].data_ptr(), stream=stream)


def sweep_k1(search):
    def f():
        for b in range(nb):
            s, so, d, do = d_pairs[b]
            jo, kp = d_k1[b]
            h.register_keyframes_device(s.data_ptr(), so.data_ptr(), d.data_ptr(), do.data_ptr(), jo.data_ptr(), kp.data_ptr(), batch,
                                        d_res[f"k1s{search}"][b].data_ptr(), track=tps[search], stream=stream)
    return f


def sweep_k3(search):
    def f():
        for b in range(nb):
            s, so, k, ko, jo, kp, init = d_k3[b]
            h.register_keyframes_device(s.data_ptr(), so.data_ptr(), k.data_ptr(), ko.data_ptr(), jo.data_ptr(), kp.data_ptr(), batch,
                                        d_res[f"k3s{search}"][b].data_ptr(), d_init=init.data_ptr(), track=tps[search], stream=stream)
    return f


sweeps = {"(a) register_batch_device, 64 pairs": sweep_pair, "(a) register_keyframes_batch_device, K = 1, search 0": sweep_k1(0),
          "(a) register_keyframes_batch_device, K = 1, search 1": sweep_k1(1), "(b) register_keyframes_batch_device, K = 3, search 0": sweep_k3(0),
          "(b) register_keyframes_batch_device, K = 3, search 1": sweep_k3(1)}


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


for f in sweeps.values():
    timed(f)  # warm-up
times = {k: [] for k in sweeps}
for r in range(reps):
    for k, f in sweeps.items():  # alternating
        times[k].append(timed(f))
for k, ts in times.items():
    per_call = float(np.median(ts)) / nb
    print(f"{k}: {per_call * 1e6:.0f} us per {batch} (median of {reps} sweeps of {nb} calls; fastest {min(ts) / nb * 1e6:.0f}, "
          f"slowest {max(ts) / nb * 1e6:.0f}) = {batch / per_call:.0f} per s", flush=True)
host = {k: np.concatenate([r.cpu().numpy().view(_rsx.CFEAR_RESULT_DTYPE) for r in v]) for k, v in d_res.items()}
assert host["k1s0"].tobytes() == host["pair"].tobytes() and host["k1s1"].tobytes() == host["pair"].tobytes(), "K = 1 is not the pair entry's bytes"
assert host["k3s0"].tobytes() == host["k3s1"].tobytes(), "the two searches differ"
for k in ("pair", "k3s0"):
    r = host[k][:n_scans - 3]
    print(f"{k}: status counts {dict((int(a), int(c)) for a, c in zip(*np.unique(r['status'], return_counts=True)))}, iterations mean "
          f"{r['iterations'].mean():.1f} max {r['iterations'].max()}, correspondences mean {r['correspondences'].mean():.0f}")


# ---- (e) accuracy ----
def report(name, rel, status, iterations, absolute):
    err = np.array([math.hypot(rel[i][0] - t[0], rel[i][1] - t[1]) for i in range(1, n_scans) for t in [synth.relative_pose(poses[i - 1], poses[i])]])
    end = synth.relative_pose(poses[0], poses[n_scans - 1])
    print(f"(e) {name}: median pair error {np.median(err):.3f} m, max {err.max():.2f} m, status 8: {int(np.sum(status[1:] == 8))}, other status != 0: "
          f"{int(np.sum((status[1:] != 0) & (status[1:] != 8)))}, scans > 0.7 m off: {int(np.sum(err > 0.7))} of {n_scans - 1}, mean iterations "
          f"{iterations[1:].mean():.1f}, end of trajectory {math.hypot(absolute[0] - end[0], absolute[1] - end[1]):.1f} m off")


p = host["pair"]
rel = [(0.0, 0.0, 0.0)] + [(float(p["x"][i]), float(p["y"][i]), float(p["yaw"][i])) for i in range(n_scans - 1)]
absolute = (0.0, 0.0, 0.0)
for r_ in rel[1:]:
    absolute = compose(absolute, r_)
report("pairs, identity start", rel, np.concatenate([[0], p["status"][:n_scans - 1]]), np.concatenate([[0], p["iterations"][:n_scans - 1]]), absolute)
for name, tp in (("3 keyframes, start at the previous pose", cfear.track_params(predict=0)), ("3 keyframes, constant-velocity start", cfear.track_params())):
    out, _ = run_tracker(1, tp, 0)
    o = out[0]
    ps = [(float(r["x"]), float(r["y"]), float(r["yaw"])) for r in o]
    report(name, [(0.0, 0.0, 0.0)] + [between(ps[i - 1], ps[i]) for i in range(1, n_scans)], o["reg"]["status"], o["reg"]["iterations"], ps[-1])
    print(f"    keyframes {int(np.sum(o['keyframe'] == 1))}, re-anchored {int(np.sum(o['keyframe'] == 2))}, correspondences mean {o['reg']['correspondences'][1:].mean():.0f}")


# ---- (g) the objectives ----
def errors(rel):
    return np.array([math.hypot(rel[i][0] - t[0], rel[i][1] - t[1]) for i in range(1, n_scans) for t in [synth.relative_pose(poses[i - 1], poses[i])]])


if objectives:
    COSTS, LOSSES = ("p2l", "p2p", "p2d"), ("huber", "cauchy", "none")
    combos = [(c, l, w) for c in range(3) for l in range(3) for w in range(2)]
    prms = {k: cfear.params(cost=k[0], loss=k[1], weights=k[2]) for k in combos}
    g_res = {k: [torch.zeros(batch * 48, dtype=torch.uint8, device="cuda") for _ in range(nb)] for k in combos}

    def sweep_objective(k):
        def f():
            for b in range(nb):
                s, so, d, do = d_pairs[b]
                h.register_device(s.data_ptr(), so.data_ptr(), d.data_ptr(), do.data_ptr(), batch, g_res[k][b].data_ptr(), params=prms[k], stream=stream)
        return f

    g_sweeps = {k: sweep_objective(k) for k in combos}
    for f in g_sweeps.values():
        timed(f)  # warm-up
    g_times = {k: [] for k in combos}
    for r in range(reps):
        for k, f in g_sweeps.items():  # alternating
            g_times[k].append(timed(f))
    end_truth = synth.relative_pose(poses[0], poses[n_scans - 1])
    print(f"(g) objectives, {n_scans - 1} consecutive pairs from the identity (us per {batch} pairs: median of {reps} sweeps of {nb} calls) and the 3-keyframe "
          f"tracker, constant-velocity start (ms per push of {n_scans} scans, us per {batch} scans: median of {reps})")
    print("| cost | loss | weights | pairs: us per 64 | mean it. | status 8 | other != 0 | > 0.7 m off | median error [m] | end of trajectory [m] "
          "| tracker: ms per push | us per 64 | mean it. | status 8 | other != 0 | > 0.7 m off | median error [m] | end of trajectory [m] |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for k in combos:
        p = np.concatenate([r.cpu().numpy().view(_rsx.CFEAR_RESULT_DTYPE) for r in g_res[k]])[:n_scans - 1]
        if k == (0, 0, 0):
            assert p.tobytes() == host["pair"][:n_scans - 1].tobytes(), "the default objective is not (a)'s bytes"
        rel = [(0.0, 0.0, 0.0)] + [(float(v["x"]), float(v["y"]), float(v["yaw"])) for v in p]
        absolute = (0.0, 0.0, 0.0)
        for r_ in rel[1:]:
            absolute = compose(absolute, r_)
        err = errors(rel)
        row = [COSTS[k[0]], LOSSES[k[1]], "yes" if k[2] else "no", f"{float(np.median(g_times[k])) / nb * 1e6:.0f}", f"{p['iterations'].mean():.1f}",
               str(int(np.sum(p["status"] == 8))), str(int(np.sum((p["status"] != 0) & (p["status"] != 8)))), str(int(np.sum(err > 0.7))),
               f"{np.median(err):.3f}", f"{math.hypot(absolute[0] - end_truth[0], absolute[1] - end_truth[1]):.1f}"]
        out, ts = run_tracker(1, cfear.track_params(), reps, prms[k])
        o = out[0]
        ps = [(float(r["x"]), float(r["y"]), float(r["yaw"])) for r in o]
        err = errors([(0.0, 0.0, 0.0)] + [between(ps[i - 1], ps[i]) for i in range(1, n_scans)])
        st = o["reg"]["status"][1:]
        row += [f"{np.median(ts) * 1e3:.1f}", f"{np.median(ts) / n_scans * batch * 1e6:.0f}", f"{o['reg']['iterations'][1:].mean():.1f}", str(int(np.sum(st == 8))),
                str(int(np.sum((st != 0) & (st != 8)))), str(int(np.sum(err > 0.7))), f"{np.median(err):.3f}",
                f"{math.hypot(ps[-1][0] - end_truth[0], ps[-1][1] - end_truth[1]):.1f}"]
        print("| " + " | ".join(row) + " |", flush=True)

# ---- (d) the odometry ----
kw = dict(keypoints="kstrongest", kstrongest=kstrongest.params(min_separation=0), estimator="cfear")
ods = {"tracking off (pairs)": odometry.Odometry(400, 3360, **kw), "tracking on": odometry.Odometry(400, 3360, cfear_track=True, **kw),
       "tracking on, compensation on": odometry.Odometry(400, 3360, cfear_track=True, cfear_compensate=True, **kw)} if odo_reps > 0 else {}
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
    print(f"(d) odometry pipeline, k-strongest(sep 0) + cfear, {k}: {n_scans / float(np.median(ts)):.0f} scans/s over {n_scans} scans (median of {odo_reps}; "
          f"fastest {n_scans / min(ts):.0f}, slowest {n_scans / max(ts):.0f}); {np.mean(o['n_matches'][1:]):.0f} matches per scan, "
          f"{int(np.sum(o['status'][1:] != 0))} scans with status != 0, translation error median {np.median(err):.3f} m max {np.max(err):.3f} m")
