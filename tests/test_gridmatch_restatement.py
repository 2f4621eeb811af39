"""The correlative matching's restatement (tests/gridmatch_np.py): its vectorised volume against the rule written as a loop, the tie
order, the property the matcher is built for -- a scan is found again in a map built from its neighbours -- and the PGM round trip that
brings a saved mosaic back as a likelihood plane.  No GPU."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gridmap_cases as gc  # noqa: E402
import gridmap_np as gm  # noqa: E402
import gridmatch_cases as gxc  # noqa: E402
import gridmatch_np as gx  # noqa: E402
import kstrongest_np as ks  # noqa: E402


@pytest.mark.parametrize("K,U,V", [(0, 0, 0), (1, 3, 0), (2, 1, 4), (1, 32, 32)])
def test_vectorised_volume_equals_the_loop(K, U, V):
    """64 x 64 random planes, a cloud at every prior of border_priors (in the map, on and outside every border), non-finite points in it"""
    p = gc.small_params(64, 64)
    rng = np.random.default_rng(100 + K + U + V)
    L = gxc.plane(7, p)
    names, priors = gxc.border_priors(p)
    mp = gxc.window(K, U, V, angle_step=0.07)
    n = 12 if U == 32 else 40
    partly = 0
    for name, t in zip(names, priors):
        pts = gxc.cloud(rng, n, p)
        pts[3] = (np.nan, 1.0)
        pts[5] = (2.0, np.inf)
        fast, slow = gx.volume(L, pts, t, p, mp), gx.volume_naive(L, pts, t, p, mp)
        assert fast.dtype == np.uint32 and fast.tobytes() == slow.tobytes(), name
        assert fast.any() or name.startswith("out")
        partly += len(np.unique(fast)) > 1
    assert partly >= 5 or (K, U, V) == (0, 0, 0)


def test_points_leave_the_map_on_every_side():
    """the priors of the cases do what they are there for: under the largest window some candidate has every placed point in the map
    and another has not (in), points outside the map at the prior itself (on_*), and points that only a shift brings in (out_*)"""
    p = gc.small_params(64, 64)
    rng = np.random.default_rng(3)
    names, priors = gxc.border_priors(p)
    L = np.ones((64, 64), dtype=np.uint8)      # a score is then the number of points inside the map
    mp = gxc.window(0, 32, 32)
    for name, t in zip(names, priors):
        pts = gxc.cloud(rng, 2000, p)
        vol = gx.volume(L, pts, t, p, mp)[0]
        placed = len(gx.cells(pts, t, 1.0, 0.0, p)[0])
        if name == "in":
            assert vol[32, 32] == placed == 2000 and vol.min() < placed
        elif name.startswith("on"):
            assert 0.3 * placed < vol[32, 32] < 0.7 * placed and vol.max() > vol[32, 32] > vol.min()
        else:
            assert vol[32, 32] == 0 and vol.max() > 0 and placed < 2000


@pytest.mark.parametrize("name", sorted(gxc.TIES))
def test_tie_order(name):
    build, want = gxc.TIES[name]
    L, clouds, priors, p, mp = build()
    res, vols = gxc.reference(L, clouds, priors, p, mp)
    r = res[0]
    assert (int(r["k"]), int(r["u"]), int(r["v"])) == want
    top = vols[0] == vols[0].max()
    if name == "zero":
        assert not vols.any() and r["status"] == gx.STATUS_EMPTY and r["score"] == 0 and r["score_runner_up"] == 0
        assert r["transform"].tobytes() == priors[0].tobytes()
    elif name == "constant":
        assert top.all() and r["status"] == 0 and r["score"] == 7 * len(clouds[0]) == r["score_runner_up"] == r["score_prior"]
        assert r["n_points"] == r["n_inside"] == len(clouds[0])
    else:
        assert vols[0].reshape(-1).tolist() == [200, 0, 200] and r["score"] == 200 and r["score_prior"] == 0
        assert r["score_runner_up"] == 200          # k = +1 is 2 steps from the winner
        c, s = gx.tables(mp)
        assert r["transform"].tolist() == [float(c[0]), -float(s[0]), 10.25, float(s[0]), float(c[0]), 10.25]


def test_status_and_batch_cut():
    """a non-finite prior is skipped and leaves its neighbours alone; a job above the cap is refused by the host entry's restatement
    and skipped by the device entry's; a job's bytes do not depend on its place in the batch"""
    L, clouds, priors, p, mp = gxc.volume_case(5, 64, 64, 1, 3, 0)
    clouds, priors = clouds[40:46], priors[40:46].copy()
    alone = [gxc.reference(L, [c], t[None], p, mp) for c, t in zip(clouds, priors)]
    priors[2, 4] = np.nan
    res, vols = gxc.reference(L, clouds, priors, p, mp)
    for i in range(6):
        if i == 2:
            assert res[i]["status"] == gx.STATUS_TRANSFORM and not vols[i].any() and res[i].tobytes().count(b"\0") == 87
        else:
            assert res[i].tobytes() == alone[i][0][0].tobytes() and vols[i].tobytes() == alone[i][1][0].tobytes()
    big = [np.zeros((gx.MAX_POINTS + 1, 2), dtype=np.float32)]
    with pytest.raises(ValueError):
        gxc.reference(L, big, priors[:1], p, mp)
    res, vols = gxc.reference(L, big, priors[:1], p, mp, device_entry=True)
    assert res[0]["status"] == gx.STATUS_POINTS and not vols.any()


@pytest.fixture(scope="module")
def drive():
    synth = importlib.import_module("navtech_radar_slam_amd.synth")
    imgs, T, p, pts, priors = gxc.end_to_end(synth, ks.extract)
    planes = gm.add_batch(gm.zeros(p), imgs[gxc.E2E_SCANS], T[gxc.E2E_SCANS], p, col_offset=gc.META)
    return planes, p, pts, priors


@pytest.mark.parametrize("mode,best,neighbour", [(0, 1144127, 1076750), (1, 469444, 450499)])
def test_a_scan_is_found_again_in_a_map_of_its_neighbours(drive, mode, best, neighbour):
    """scan 3 of the synthetic drive against the map of scans 0, 1, 2, 4, 5: priors off by (3, -2) m and 0.03 rad, (-5, 4) m and
    -0.05 rad, and not at all -> exactly the window's candidate that undoes the error.  The figures are the restatement's own."""
    planes, p, pts, priors = drive
    assert len(pts) == 4800
    mp = gx.params(**gxc.E2E_WINDOW)
    res, vols = gxc.reference(gx.likelihood(planes, mode), [pts] * 3, priors, p, mp)
    for r, want in zip(res, gxc.E2E_WINNERS):
        assert (int(r["k"]), int(r["u"]), int(r["v"])) == want and r["status"] == 0
        assert r["score"] > r["score_runner_up"] > 0 and (r["score"] > r["score_prior"]) == (want != (0, 0, 0))
    for v in vols:
        assert np.count_nonzero(v == v.max()) == 1          # no tie at the top
    assert int(res[0]["score"]) == best
    top2 = np.sort(vols[0].reshape(-1))[-2]
    assert int(top2) == neighbour
    # the recovered pose is the true one to within the window's grid: half a cell and half a step of rotation
    truth = priors[2]
    for r in res:
        assert abs(r["transform"][2] - truth[2]) < 1e-9 and abs(r["transform"][5] - truth[5]) < 1e-9
        assert np.abs(r["transform"][[0, 1, 3, 4]] - truth[[0, 1, 3, 4]]).max() < 1e-6


def test_pgm_round_trip(tmp_path):
    """gridmap.load_pgm reads back what GridMap.save_pgm writes for the mean (write_pgm is its writer), comments in the header and all"""
    from navtech_radar_slam_amd import gridmap
    px = np.random.default_rng(9).integers(0, 256, size=(64, 128), dtype=np.uint8)
    px[0, :4] = (10, 32, 9, 13)       # bytes that are white space in a header, first in the raster
    f = str(tmp_path / "mosaic.pgm")
    gridmap.write_pgm(f, px)
    with open(f, "rb") as fh:
        raw = fh.read()
    assert raw.startswith(b"P5\n128 64\n255\n") and len(raw) == 14 + 64 * 128
    back = gridmap.load_pgm(f)
    assert back.dtype == np.uint8 and back.shape == (64, 128) and back.tobytes() == px.tobytes()
    with open(f, "wb") as fh:
        fh.write(b"P5\n# a comment\n128\t64\n# another\n255\n" + px.tobytes())
    assert gridmap.load_pgm(f).tobytes() == px.tobytes()
    with open(f, "wb") as fh:
        fh.write(b"P5\n128 64\n255\n" + px.tobytes()[:-1])
    with pytest.raises(ValueError):
        gridmap.load_pgm(f)
    with open(f, "wb") as fh:
        fh.write(b"P2\n1 1\n255\n0\n")
    with pytest.raises(ValueError):
        gridmap.load_pgm(f)
