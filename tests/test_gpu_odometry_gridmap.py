"""host/odometry --grid-map FILE.pgm: every window handed to rsx_odometry_push also goes through rsx_gridmap_add_batch at the poses the
tool composes (or at those of --grid-poses), and the renders are written as binary PGM at the end.  With poses whose yaw is exactly 0
(cos = 1, sin = 0 in any libm) the files must hold the restatement's renders (tests/gridmap_np.py) byte for byte; the odometry lines
must not change."""
import os
import subprocess
import sys

import numpy as np
import pytest

from navtech_radar_slam_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gridmap_cases as gc  # noqa: E402
import gridmap_np as gm  # noqa: E402

pytestmark = pytest.mark.gpu
HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "navtech-radar-slam_amd", "host")
SIZE, RES = 256, 0.5


def _run(seq_dir, *flags):
    exe = os.path.join(HOST, "odometry")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    r = subprocess.run([exe, f"seq_dir:={seq_dir}", "do_slam:=true", *flags], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def _pgm(path):
    raw = open(path, "rb").read()
    head = b"P5\n%d %d\n255\n" % (SIZE, SIZE)
    assert raw[:len(head)] == head and len(raw) == len(head) + SIZE * SIZE
    return np.frombuffer(raw[len(head):], dtype=np.uint8).reshape(SIZE, SIZE)


def _hits_pgm(planes):
    h = gm.render_hits(planes).astype(np.int16)
    return np.where(h < 0, 255, 254 - 2 * h).astype(np.uint8)


@pytest.fixture(scope="module")
def sequence(tmp_path_factory):
    from PIL import Image
    imgs, _, poses, stamps = synth.polar_sequence(11, 6)
    root = tmp_path_factory.mktemp("gridseq")
    d = root / "seq" / "polar_oxford_form"
    d.mkdir(parents=True)
    for img, st in zip(imgs, stamps):
        Image.fromarray(img, mode="L").save(str(d / f"{int(st)}.png"))
    return root, imgs, poses


def test_grid_map_files(sequence):
    root, imgs, poses = sequence
    seq, size = root / "seq", ("--grid-size", str(SIZE), str(SIZE))
    plain = _run(seq, "--window", "4")
    # ---- poses from a file, yaw exactly 0, the first pose not at the origin: both files are the restatement's renders ----
    given = np.stack([poses[:, 0] + 3.5, poses[:, 1] - 2.25, np.zeros(6)], axis=1)
    with open(root / "poses.txt", "w") as f:
        for x, y, yaw in given:
            f.write("%s %s %s\n" % (repr(float(x)), repr(float(y)), repr(float(yaw))))
    out = _run(seq, "--window", "4", "--grid-map", str(root / "mean.pgm"), "--grid-hits", str(root / "hits.pgm"), *size, "--grid-hit-threshold", "90",
               "--grid-poses", str(root / "poses.txt"))   # windows of 4 + 2
    assert out == plain
    p = gm.params(width=SIZE, height=SIZE, hit_threshold=90, origin_x=given[0, 0] - 0.5 * SIZE * RES, origin_y=given[0, 1] - 0.5 * SIZE * RES)
    want = gm.add_batch(gm.zeros(p), imgs, gc.matrices(given), p, col_offset=synth.OXFORD_META)
    assert want[1].max() == 6 and want[2].any()
    assert _pgm(root / "mean.pgm").tobytes() == gm.render_mean(want).tobytes()
    assert _pgm(root / "hits.pgm").tobytes() == _hits_pgm(want).tobytes()
    # ---- the tool's own poses: the files against GridMap.add at the poses it printed ----
    out = _run(seq, "--window", "4", "--grid-map", str(root / "own.pgm"), "--grid-hits", str(root / "own_hits.pgm"), *size)
    assert out == plain
    printed = np.array([[float(v) for v in line.split()[1:4]] for line in out.strip().split("\n")])
    assert printed.shape == (6, 3) and np.abs(printed[1:] - poses[1:]).max() < 1.0
    from navtech_radar_slam_amd import coral, gridmap
    T = coral.pose_matrices(printed)
    p = gm.params(width=SIZE, height=SIZE, origin_x=-0.5 * SIZE * RES, origin_y=-0.5 * SIZE * RES)     # centred on the first pose, (0, 0)
    m = gridmap.GridMap(400, 3360, gridmap.params(**p))
    m.add(imgs, T)
    planes = m.read()
    m.close()
    # a printed pose is within 5e-7 m and 5e-7 rad of the composed one: a cell centre moves by less than 5e-7 * (sqrt 2 + 200) =
    # 1.01e-4 m against a scan, a fifth of the margin of 1e-3 of a cell.  Cells farther than that margin from the edges that decide
    # whether a scan observes them have the same count in both maps; those farther than it from EVERY bin edge and beam bisector,
    # for all six scans, the same bins and rows, hence the same sum and hits as well
    margin = 1e-3 * RES
    marg = [gc.cell_margins(t, p, 400, 3360) for t in T]
    observed = planes[1] > 0
    same_count = np.all([s > margin for _, s, _ in marg], axis=0)
    same_sample = np.all([(a > margin) & (b > margin) for a, _, b in marg], axis=0) & same_count
    share_count, share_sample = same_count[observed].mean(), same_sample[observed].mean()
    # six scans, each cell within the margin of a bin edge with probability 2 margin / range_resolution = 1.7 %: 0.983^6 = 0.90, less
    # about 1 % for the bisectors (a beam is 0.5 m wide at 30 m)
    print("cells with the count decided by a margin: %.4f of the observed; with every bin and row decided: %.4f" % (share_count, share_sample))
    assert share_count >= 0.99 and share_sample >= 0.85
    mean, hits = _pgm(root / "own.pgm"), _pgm(root / "own_hits.pgm")
    assert np.array_equal((hits != 255)[same_count], observed[same_count])
    assert np.array_equal(mean[same_sample], gm.render_mean(planes)[same_sample])
    assert np.array_equal(hits[same_sample], _hits_pgm(planes)[same_sample])
    assert (mean != gm.render_mean(planes)).mean() < 0.05      # (and the rest is close: a few samples taken one bin over)


def test_grid_map_flag_rules(sequence):
    root, _, _ = sequence
    exe = os.path.join(HOST, "odometry")
    bad = subprocess.run([exe, f"seq_dir:={root / 'seq'}", "--grid-map", str(root / "x.pgm"), "--per-scan"], capture_output=True, text=True, timeout=300)
    assert bad.returncode == 1 and "windowed path only" in bad.stderr
    bad = subprocess.run([exe, f"seq_dir:={root / 'seq'}", "--grid-hits", str(root / "x.pgm")], capture_output=True, text=True, timeout=300)
    assert bad.returncode == 1 and "need --grid-map" in bad.stderr
    bad = subprocess.run([exe, f"seq_dir:={root / 'seq'}", "--grid-map", str(root / "x.pgm"), "--grid-size", "100", "64"], capture_output=True,
                         text=True, timeout=300)
    assert bad.returncode == 1 and "width" in bad.stderr
    assert not (root / "x.pgm").exists()
