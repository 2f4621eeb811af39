"""Setter sequences on one odometry handle against the restated switch rules (tests/odometry_switch_np.py): every sequence of up to
three of the twelve actions is accepted and refused call by call as the model says, a handle walked into a configuration the long way
(refusals included) computes the bytes of a handle brought there the short way, and a refused call changes nothing.

64 x 512 scans, k-strongest keypoints and phase correlation at N = 64, 0.9 m per pixel: the case of tests/test_gpu_odometry_phasecorr.py,
the smallest at which every estimator returns status 0."""
import os
import sys

import numpy as np
import pytest

from navtech_radar_slam_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import odometry_switch_np as sw  # noqa: E402

pytestmark = pytest.mark.gpu
SMALL = dict(n=64, resolution=0.9)


def _handle():
    from navtech_radar_slam_amd import odometry
    return odometry.Odometry(64, 512, keypoints="kstrongest")


def _do(od, action):
    """one action of the model on handle `od` -> accepted (a refusal is RSX_ERR_BAD_ARG)"""
    from navtech_radar_slam_amd import _rsx
    setter, arg = action
    try:
        if setter == "set_estimator":
            od.set_estimator(arg)
        elif setter == "set_cfear":
            od.set_cfear(off=not arg)
        elif setter == "set_cfear_tracking":
            od.set_cfear_tracking(off=not arg)
        elif setter == "set_compensation":
            od.set_compensation("both" if arg else None)
        elif arg == "off":
            od.set_phasecorr(off=True)
        else:
            od.set_phasecorr(dict(SMALL, mode=("estimate", "fallback").index(arg)))
    except _rsx.RsxError as e:
        assert e.status == -1, (action, e)
        return False
    return True


def _fresh_again(od):
    od.reset()
    assert all(_do(od, a) for a in sw.OFF)


@pytest.fixture(scope="module")
def scans():
    imgs, az, _, _ = synth.polar_sequence(3, 6, rows=64, cols=512, n_buildings=120, n_poles=200, world_radius=40.0)
    return imgs[:3], az


@pytest.fixture(scope="module")
def walked():
    od = _handle()
    yield od
    od.close()


def test_every_sequence_of_up_to_three_actions_is_answered_as_the_model_answers(walked):
    seqs = sw.sequences(3)
    assert len(seqs) == 1884
    for seq in seqs:
        want, _ = sw.walk(seq)
        got = [_do(walked, a) for a in seq]
        assert got == want, (seq, got, want)
        _fresh_again(walked)


def test_a_configuration_computes_the_same_however_it_was_reached(walked, scans):
    imgs, az = scans
    routes = sw.routes(3)
    assert len(routes) == 15
    seen = {}
    for state, (short, long_) in sorted(routes.items()):
        assert [_do(walked, a) for a in long_] == sw.walk(long_)[0]
        got = walked.push(imgs, az)
        _fresh_again(walked)
        direct = _handle()
        assert all(_do(direct, a) for a in short), (state, short)
        want = direct.push(imgs, az)
        direct.close()
        print(state, "by", long_, "status", got["status"].tolist(), "n_matches", got["n_matches"].tolist())
        assert got.tobytes() == want.tobytes(), (state, long_, short, got, want)
        assert got["status"][0] == 3 and got["n_keypoints"].min() > 0
        seen[state] = got.tobytes()
    # the comparison can tell configurations apart: pair stages and estimators differ in their records
    est = {s[0]: b for s, b in seen.items() if s[1:] == (False, False, "off")}
    assert len(set(est.values())) == 4, "orora, ransac, mcransac and cfear give the same bytes"
    assert seen[("orora", False, False, "estimate")] not in est.values()
    assert seen[("cfear", True, False, "off")] != est["cfear"]


def test_a_refused_set_estimator_leaves_the_tracker_on(scans):
    """rsx_odometry_set_estimator with parameters rsx::ransac_check_params rejects, on a handle with the CFEAR tracker on"""
    from navtech_radar_slam_amd import _rsx, ransac
    imgs, az = scans
    od, ref, pairs = _handle(), _handle(), _handle()
    for h in (od, ref):
        h.set_cfear()
        h.set_cfear_tracking()
    pairs.set_cfear()
    with pytest.raises(_rsx.RsxError, match="tolerance") as e:
        od.set_estimator("ransac", ransac.default_params(tolerance=-1.0))
    assert e.value.status == -1
    got, want, other = od.push(imgs, az), ref.push(imgs, az), pairs.push(imgs, az)
    for h in (od, ref, pairs):
        h.close()
    assert other.tobytes() != want.tobytes()  # (tracker and pair registration differ here: the comparison below can fail)
    assert got.tobytes() == want.tobytes(), (got, want)
