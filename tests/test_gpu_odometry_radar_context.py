"""host/odometry --radar-context FILE: every window handed to rsx_odometry_push also goes through rsx_radarsc_build_batch into
a ScanContext database that is written to FILE at the end.  The loaded file must hold the restatement's descriptors
(tests/radarsc_np.py) of the sequence's scans, with the grids the tool reads out of the rows' metadata, and the odometry lines
must not change."""
import os
import subprocess
import sys

import numpy as np
import pytest

from navtech_radar_slam_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import radarsc_np as rc  # noqa: E402

pytestmark = pytest.mark.gpu
HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "navtech-radar-slam_amd", "host")


def _run(seq_dir, *flags):
    exe = os.path.join(HOST, "odometry")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    r = subprocess.run([exe, f"seq_dir:={seq_dir}", "do_slam:=true", *flags], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_radar_context_file(tmp_path):
    from PIL import Image
    from navtech_radar_slam_amd import scancontext
    imgs, az, poses, stamps = synth.polar_sequence(11, 6)
    d = tmp_path / "seq" / "polar_oxford_form"
    d.mkdir(parents=True)
    for img, st in zip(imgs, stamps):
        Image.fromarray(img, mode="L").save(str(d / f"{int(st)}.png"))
    # the grid as the tool derives it: the encoder counts at bytes 8-9 of every row
    counts = imgs[:, :, 8:10].copy().view("<u2")[:, :, 0]
    grids = (counts.astype(np.float64) * 2.0 * np.pi / 5600.0).astype(np.float32)
    plain = _run(tmp_path / "seq", "--window", "4")
    for flags, kw in (((), {}), (("--rc-floor", "40", "--rc-stat", "max", "--rc-max-radius", "60"), dict(power_floor=40, stat=rc.MAX, max_radius=60.0))):
        path = tmp_path / ("rc%d.scdb" % len(flags))
        out = _run(tmp_path / "seq", "--window", "4", "--radar-context", str(path), *flags)   # windows of 4 + 2
        assert out == plain
        g = scancontext.SCManager()
        assert g.load(str(path)) == 6
        want = rc.build_batch(imgs, grids, **kw)
        assert g.export_descriptors_f32().tobytes() == want.tobytes()
    bad = subprocess.run([os.path.join(HOST, "odometry"), f"seq_dir:={tmp_path / 'seq'}", "--radar-context", str(tmp_path / "x"), "--per-scan"],
                         capture_output=True, text=True, timeout=300)
    assert bad.returncode == 1 and "windowed path only" in bad.stderr
