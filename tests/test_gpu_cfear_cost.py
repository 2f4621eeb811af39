"""rsx_cfear_params.cost / loss / weights (csrc/cfear_track.hip, the GENERAL instances) through every entry that takes the struct,
against the arithmetic contract tests/cfear_cost_np.py.

Status, iterations and correspondences equal the restatement's; x, y, yaw and cost within 1e-4 (the project's tolerance: the kernel
sums in another order and uses the device's sincos, log and sqrt).  A case may be left out of that comparison only when the
restatement reports a decision margin below 1e-9, at most 1 % of a test's cases -- and none is: every margin is asserted to be at
least 1e-9 (tests/test_cfear_cost_restatement.py asserts the same without a GPU).  Where two GPU results are compared (the cell
index against brute force, a batch against its parts, one push against several, a sequence alone against sixteen side by side)
the BYTES are equal.  The shapes are the existing small ones: thirteen pairs of 54 to about 650 records (and the cap), the joint
jobs of up to three keyframes, the 8 scans of the small sequence (64 x 512 images).
PARITY UNPINNED w.r.t. CFEAR's own code, which is not in the reference checkout."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cfear_cost_cases as ccases  # noqa: E402
import cfear_cost_np as cc  # noqa: E402
import cfear_mocomp_cases as mcases  # noqa: E402
import cfear_track_cases as cases  # noqa: E402
import cfear_track_np as ct  # noqa: E402

pytestmark = pytest.mark.gpu
ID = ccases.ID
HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "navtech-radar-slam_amd", "host")


@pytest.fixture(scope="module")
def handle():
    from navtech_radar_slam_amd import cfear
    h = cfear.Cfear()
    yield h
    h.close()


def _params(combo, **over):
    from navtech_radar_slam_amd import cfear
    return cfear.params(**ccases.as_kw(combo), **over)


def _search(s):
    from navtech_radar_slam_amd import cfear
    return cfear.track_params(search=s)


def _compare(name, got, want, left_out):
    d = max(abs(got["x"] - want["x"]), abs(got["y"] - want["y"]), abs(got["yaw"] - want["yaw"]), abs(got["cost"] - want["cost"]))
    print(f"{name}: status {got['status']}, {got['iterations']} iterations, {got['correspondences']} correspondences, "
          f"|GPU - restatement| {d:.2e}, margin {want['margin']:.1e}")
    if want["margin"] < 1e-9:
        left_out.append(name)
        return
    assert (got["status"], got["iterations"], got["correspondences"]) == (want["status"], want["iterations"], want["correspondences"]), (name, got, want)
    assert d < 1e-4, (name, got, want)


def _job_args(jobs):
    return [j[1] for j in jobs], [list(j[2]) for j in jobs], [list(j[3]) for j in jobs], np.array([j[4] for j in jobs])


@pytest.mark.parametrize("combo", ccases.OTHERS, ids=[cc.name_of(c) for c in ccases.OTHERS])
def test_pairs_and_joint_jobs_equal_the_restatement(handle, combo):
    """2a: every combination but today's through rsx_cfear_register_batch and rsx_cfear_register_keyframes_batch, both searches"""
    want = {c[0]: w for c, w in zip(cases.pair_cases(), ccases.pair_wants(combo))}
    left_out, n = [], 0
    for key, cs, init in cases.pair_groups():
        prm = _params(combo, **dict(key))
        pair = handle.register([c[1] for c in cs], [c[2] for c in cs], init, prm)
        for s in (0, 1):
            got = handle.register_keyframes([c[1] for c in cs], [[c[2]] for c in cs], [[ID] for _ in cs], init, prm, _search(s))
            assert got.tobytes() == pair.tobytes(), (key, s)
        for c, g in zip(cs, pair):
            assert want[c[0]]["margin"] >= 1e-9, (c[0], want[c[0]])  # the restatement alone leaves out none
            _compare(c[0], g, want[c[0]], left_out)
            n += 1
    jobs = ccases.joint_jobs(combo)
    cells, brute = (handle.register_keyframes(*_job_args(jobs), params=_params(combo), track=_search(s)) for s in (0, 1))
    assert cells.tobytes() == brute.tobytes()
    for j, g, w in zip(jobs, cells, ccases.joint_wants(combo)):
        assert w["margin"] >= 1e-9, (j[0], w)
        _compare(j[0], g, w, left_out)
        n += 1
    assert len(left_out) <= n // 100, left_out
    # the words act: not the default's bytes on a pair that registers
    c = cases.pair_cases()[0]
    assert handle.register([c[1]], [c[2]], None, _params(combo)).tobytes() != handle.register([c[1]], [c[2]]).tobytes()


def test_a_batch_of_257_jobs(handle):
    """2b: more jobs than workgroups (256): a workgroup takes two jobs; a job's bytes do not depend on the batch"""
    key, cs, init = cases.pair_groups()[0]
    cs = [c for c in cs if len(c[1]) <= 700 and len(c[2]) <= 700]  # (the sides at the cap are in 2a)
    init = np.array([c[3] if c[3] is not None else ID for c in cs])
    for combo in ccases.TRACKED:
        prm = _params(combo)
        few = handle.register([c[1] for c in cs], [c[2] for c in cs], init, prm)
        pick = [i % len(cs) for i in range(257)]
        many = handle.register([cs[i][1] for i in pick], [cs[i][2] for i in pick], init[pick], prm)
        assert many.tobytes() == few[pick].tobytes()
        many = handle.register_keyframes([cs[i][1] for i in pick], [[cs[i][2]] for i in pick], [[ID] for _ in pick], init[pick], prm, _search(1))
        assert many.tobytes() == few[pick].tobytes()


def _check_track(name, got, want, left_out):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert w["margin"] >= 1e-9, (name, i, w)
        assert (g["keyframe"], g["n_keyframes"], g["reg"]["reserved"]) == (w["keyframe"], w["n_keyframes"], w["reg"]["reserved"]), (name, i, g, w)
        _compare(f"{name} scan {i}", g["reg"], w["reg"], left_out)
        assert max(abs(g[f] - w[f]) for f in ("x", "y", "yaw")) < 1e-4, (name, i, g, w)


@pytest.mark.parametrize("compensate", (0, 1), ids=("untimed push", "timed push, compensate 1"))
@pytest.mark.parametrize("combo", ccases.TRACKED, ids=[cc.name_of(c) for c in ccases.TRACKED])
def test_tracker_equals_the_restatement(combo, compensate):
    """2b: one sequence and sixteen, whole and cut into pushes (between scan 0 and scan 1 included), both searches"""
    from navtech_radar_slam_amd import cfear
    recs, taus = mcases.small_timed()
    room, room_taus, _ = mcases.drive("constant")
    prm = _params(combo)

    def tp(**kw):
        return cfear.track_params(compensate=compensate, **cases.SMALL_TRACK, **kw)

    def push(t, scans, times):
        return t.push_timed(scans, times) if compensate else t.push(scans)

    t = cfear.Tracker(params=prm, track=tp())
    whole = push(t, recs, taus)
    left_out = []
    _check_track(f"{cc.name_of(combo)}, compensate {compensate}", whole, ccases.small_track(combo, compensate), left_out)
    assert not left_out
    assert whole["n_keyframes"].max() == 3 and all(int(v) in (0, 8) for v in whole["reg"]["status"][1:])
    for cuts in (((0, 1), (1, 3), (3, 8)), ((0, 4), (4, 5), (5, 8))):
        t.reset(params=prm, track=tp())
        parts = np.concatenate([push(t, recs[a:b], taus[a:b]) for a, b in cuts])
        assert parts.tobytes() == whole.tobytes(), cuts
    t.reset(params=prm, track=tp())
    other = push(t, list(room), list(room_taus))
    t.reset(params=prm, track=tp(search=1))
    assert push(t, recs, taus).tobytes() == whole.tobytes()
    # not the default objective's track
    t.reset(params=None, track=tp())
    assert push(t, recs, taus).tobytes() != whole.tobytes()
    t.close()
    # sixteen sequences side by side: the bytes of each alone, whatever its neighbours do
    seqs = [(list(recs), list(taus)), (list(room), list(room_taus))]
    alone = [whole, other]
    many = cfear.Tracker(16, params=prm, track=tp())
    got = push(many, [seqs[q % 2][0] for q in range(16)], [seqs[q % 2][1] for q in range(16)])
    for q in range(16):
        assert got[q].tobytes() == alone[q % 2].tobytes(), q
    many.reset(params=prm, track=tp())
    cut = [1 + q % 4 for q in range(16)]  # (1: between scan 0 and scan 1)
    a = push(many, [seqs[q % 2][0][:cut[q]] for q in range(16)], [seqs[q % 2][1][:cut[q]] for q in range(16)])
    b = push(many, [[] if q == 5 else seqs[q % 2][0][cut[q]:] for q in range(16)], [[] if q == 5 else seqs[q % 2][1][cut[q]:] for q in range(16)])
    c = push(many, [seqs[1][0][cut[5]:] if q == 5 else [] for q in range(16)], [seqs[1][1][cut[5]:] if q == 5 else [] for q in range(16)])
    for q in range(16):
        assert np.concatenate([a[q], b[q], c[q]]).tobytes() == alone[q % 2].tobytes(), q
    many.close()


def test_records_that_are_not_valid(handle):
    """2c: dst (and, with weights, src) records whose lambda_min is 0, negative or NaN are skipped and counted out; the objectives
    that do not read the eigenvalues give the bytes they give without them"""
    c = cases.pair_cases()[0]  # drive pair 1
    src, dst = c[1], c[2]
    bad_dst, bad_src = ccases.poisoned(dst), ccases.poisoned(src)
    left_out = []
    for combo, s, d in (((cc.COST_P2D, 0, 0), src, bad_dst), ((cc.COST_P2D, cc.LOSS_CAUCHY, 1), src, bad_dst), ((0, 0, 1), src, bad_dst),
                        ((0, 0, 1), bad_src, dst), ((cc.COST_P2P, cc.LOSS_NONE, 1), bad_src, bad_dst)):
        want = cc.register(s, d, **ccases.as_kw(combo))
        clean = ccases.pair_wants(combo)[0]
        cells = handle.register([s, src], [d, dst], None, _params(combo))
        brute = handle.register_keyframes([s, src], [[d], [dst]], [[ID], [ID]], None, _params(combo), _search(1))
        assert cells.tobytes() == brute.tobytes()
        assert want["margin"] >= 1e-9 and want["correspondences"] < clean["correspondences"], (combo, want, clean)
        _compare(f"{cc.name_of(combo)}, records not valid", cells[0], want, left_out)
        _compare(f"{cc.name_of(combo)}, clean", cells[1], clean, left_out)
        assert all(math.isfinite(cells[0][f]) for f in ("x", "y", "yaw", "cost")), cells[0]
    assert not left_out
    # every dst record refused: no correspondence, status 4, the start pose
    none = dst.copy()
    none["lambda_min"] = np.nan
    g = handle.register([src], [none], None, _params((cc.COST_P2D, 0, 0)))[0]
    assert (g["status"], g["correspondences"], g["x"], g["y"], g["yaw"]) == (4, 0, 0.0, 0.0, 0.0)
    # point-to-line without weights never reads them: the default instance, and the general one under another loss
    for combo in ((0, 0, 0), (0, cc.LOSS_CAUCHY, 0), (cc.COST_P2P, cc.LOSS_NONE, 0)):
        got = handle.register([src, bad_src, src], [bad_dst, dst, dst], None, _params(combo))
        assert got[0].tobytes() == got[2].tobytes() and got[1].tobytes() == got[2].tobytes(), combo


def _pose(r):
    return (float(r["x"]), float(r["y"]), float(r["yaw"]))


def _odometry(**kw):
    from navtech_radar_slam_amd import kstrongest, odometry
    return odometry.Odometry(mcases.SMALL_ROWS, mcases.SMALL_COLS, keypoints="kstrongest", kstrongest=kstrongest.params(k=12, min_separation=0),
                             estimator="cfear", **kw)


def test_odometry_runs_the_chosen_objective(handle, tmp_path):
    """2d: the odometry on the small sequence's images gives what the tracker and pair entries give on the same records, and
    host/odometry's switches select the same"""
    from navtech_radar_slam_amd import cfear
    from navtech_radar_slam_amd import kstrongest
    _, imgs, az = mcases.small_keypoints()
    # the records the odometry makes inside: the device's k-strongest keypoints through the device's surface points
    ks = kstrongest.KStrongest(mcases.SMALL_ROWS, mcases.SMALL_COLS)
    tg, xy = ks.extract_batch(imgs, k=12, min_separation=0, azimuths=az)
    recs, taus, _, _ = handle.surface_points_timed(xy, [np.ascontiguousarray(t[:, 0]) for t in tg], mcases.SMALL_ROWS)
    print("records equal the CPU chain's:", [a.tobytes() == b.tobytes() for a, b in zip(recs, mcases.small_timed()[0])])
    combo = ccases.TRACKED[0]
    prm = _params(combo)
    results = {}
    for compensate in (0, 1):
        tp = cfear.track_params(compensate=compensate, **cases.SMALL_TRACK)
        od = _odometry(cfear=prm, cfear_track=tp)
        res = od.push(imgs, az)
        t = cfear.Tracker(params=prm, track=tp)
        want = t.push_timed(recs, taus) if compensate else t.push(recs)
        t.close()
        assert res["n_matches"][1:].tolist() == want["reg"]["correspondences"][1:].tolist()
        assert res["iterations"][1:].tolist() == want["reg"]["iterations"][1:].tolist()
        for i in range(1, 8):
            rel = ct.between(_pose(want[i - 1]), _pose(want[i]))
            assert max(abs(res[f][i] - v) for f, v in zip(("x", "y", "yaw"), rel)) < 1e-9, (compensate, i, res[i], rel)
        assert od.push(imgs, az).tobytes() != _odometry(cfear_track=tp).push(imgs, az).tobytes()  # (not the default's)
        results[compensate] = res
    # tracking off: the pair entry's results
    res = _odometry(cfear=prm).push(imgs, az)
    pairs = handle.register(recs[1:], recs[:-1], None, prm)
    for i in range(1, 8):
        assert (res["x"][i], res["y"][i], res["yaw"][i], res["n_matches"][i]) == (pairs["x"][i - 1], pairs["y"][i - 1], pairs["yaw"][i - 1],
                                                                                 pairs["correspondences"][i - 1]), i
    # the C++ entry: its switches select the same objective
    from PIL import Image
    from navtech_radar_slam_amd import synth
    from oracle import odometry_chain
    stamps = synth.polar_sequence(3, 8, rows=mcases.SMALL_ROWS, cols=mcases.SMALL_COLS, n_buildings=120, n_poles=200, world_radius=40.0)[3]
    d = tmp_path / "seq" / "polar_oxford_form"
    d.mkdir(parents=True)
    for img, st in zip(imgs, stamps):
        Image.fromarray(img, mode="L").save(str(d / f"{int(st)}.png"))
    base = [os.path.join(HOST, "odometry"), f"seq_dir:={tmp_path / 'seq'}", "--keypoints", "kstrongest", "--k", "12", "--min-separation", "0",
            "--estimator", "cfear"]
    r = subprocess.run(base + ["--cfear-cost", "p2p", "--cfear-loss", "cauchy", "--cfear-weights", "--cfear-keyframes", "3",
                               "--cfear-keyframe-distance", "0.5"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.array([[float(v) for v in line.split()[1:]] for line in r.stdout.strip().splitlines()])
    res = results[0]
    pose, lib_pose = np.zeros(3), [np.zeros(3)]
    for i in range(1, 8):
        pose = odometry_chain.compose(pose, (res["x"][i], res["y"][i], res["yaw"][i]))
        lib_pose.append(pose.copy())
    assert got.shape == (8, 5) and np.allclose(got[:, 0:3], np.stack(lib_pose), atol=2e-6), np.abs(got[:, 0:3] - np.stack(lib_pose)).max()
    assert np.array_equal(got[:, 4], res["n_matches"])
    for flag, value in (("--cfear-cost", "p2x"), ("--cfear-loss", "l2")):
        bad = subprocess.run(base + [flag, value], capture_output=True, text=True, timeout=120)
        assert bad.returncode != 0 and flag in bad.stdout + bad.stderr


def test_bad_values_are_refused_by_every_entry(handle):
    """2d: cost = 3, loss = -1 and weights = 2, with the field's name in the message"""
    import torch
    from navtech_radar_slam_amd import _rsx, cfear
    room = cases.as_records(cases.room64())
    tau = np.full(len(room), 0.5, dtype=np.float32)
    xy = np.stack([room["x"], room["y"]], axis=1)
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    assert (_rsx.CFEAR_COST_P2L, _rsx.CFEAR_COST_P2P, _rsx.CFEAR_COST_P2D) == (0, 1, 2)
    assert (_rsx.CFEAR_LOSS_HUBER, _rsx.CFEAR_LOSS_CAUCHY, _rsx.CFEAR_LOSS_NONE) == (0, 1, 2)
    d = cfear.default_params()
    assert (d.cost, d.loss, d.weights) == (0, 0, 0) and not hasattr(d, "reserved")
    for bad, word in ((dict(cost=3), "cost"), (dict(loss=-1), "loss"), (dict(weights=2), "weights")):
        prm = cfear.params(**bad)
        t = cfear.Tracker(params=prm)
        tt = cfear.Tracker(params=prm, track=cfear.track_params(compensate=1))
        entries = (
            lambda: handle.surface_points([xy], prm),
            lambda: handle.surface_points_timed([xy], [np.zeros(len(xy), dtype=np.int32)], 400, prm),
            lambda: handle.surface_points_device(p, p, 1, p, 16, p, params=prm),
            lambda: handle.register([room], [room], None, prm),
            lambda: handle.register_device(p, p, p, p, 1, p, params=prm),
            lambda: handle.register_keyframes([room], [[room]], [[ID]], None, prm),
            lambda: handle.register_keyframes_device(p, p, p, p, p, p, 1, p, params=prm),
            lambda: t.push([room]),
            lambda: t.push_device(p, p, p, p),
            lambda: tt.push_timed([room], [tau]),
            lambda: tt.push_timed_device(p, p, p, p, p),
            lambda: _odometry(cfear=prm),
        )
        for k, entry in enumerate(entries):
            with pytest.raises(_rsx.RsxError, match=word) as e:
                entry()
            assert e.value.status == -1, (word, k)
        t.close()
        tt.close()
