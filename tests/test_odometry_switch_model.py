"""The restated switch rules (tests/odometry_switch_np.py) keep their invariants on every sequence of up to three actions from a fresh
handle.  No GPU: tests/test_gpu_odometry_switching.py holds the library to the same model."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import odometry_switch_np as sw  # noqa: E402


def test_twelve_actions():
    assert len(sw.ACTIONS) == len(set(sw.ACTIONS)) == 12


def test_invariants_on_all_sequences_of_up_to_three_actions():
    seqs = sw.sequences(3)
    assert len(seqs) == 12 + 12 ** 2 + 12 ** 3
    for seq in seqs:
        state = sw.FRESH
        for action in seq:
            accepted, after = sw.apply(state, action)
            est, track, comp, pc = after
            assert est in sw.ESTIMATORS + ("cfear",) and pc in sw.PC_MODES
            assert not track or est == "cfear", (seq, after)
            assert not comp or (est not in ("mcransac", "cfear") and pc == "off"), (seq, after)
            assert not track or pc == "off", (seq, after)
            if accepted:
                assert after == sw.candidate(state, action)
            else:
                assert after == state and sw.broken_rule(sw.candidate(state, action)), (seq, action)
            if action[1] in (False, "off"):
                assert accepted, (seq, action)  # a NULL form is never refused
            state = after
        assert sw.walk(sw.OFF, state) == ([True] * 5, sw.FRESH), seq


def test_every_valid_state_is_reached_and_routed():
    valid = {(e, t, c, p) for e in sw.ESTIMATORS + ("cfear",) for t in (False, True) for c in (False, True) for p in sw.PC_MODES
             if sw.broken_rule((e, t, c, p)) is None}
    routes = sw.routes(3)
    assert set(routes) == valid and len(valid) == 15
    for state, (short, long_) in routes.items():
        assert sw.walk(short)[1] == state == sw.walk(long_)[1]
        assert len(short) <= 2 and len(long_) == 3
    assert routes[sw.FRESH][0] == ()
    # selecting an estimator leaves ESTIMATE, not the fallback; NULL restores the selected estimator
    assert sw.walk([("set_phasecorr", "estimate"), ("set_estimator", "ransac")])[1] == ("ransac", False, False, "off")
    assert sw.walk([("set_phasecorr", "fallback"), ("set_estimator", "ransac")])[1] == ("ransac", False, False, "fallback")
    assert sw.walk([("set_cfear", True), ("set_phasecorr", "estimate"), ("set_phasecorr", "off")])[1] == ("cfear", False, False, "off")
