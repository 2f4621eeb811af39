"""The switch rules of the windowed odometry's estimator side restated in plain Python: which of rsx_odometry_set_estimator,
rsx_odometry_set_cfear, rsx_odometry_set_cfear_tracking, rsx_odometry_set_compensation and rsx_odometry_set_phasecorr a handle that
holds no scan accepts, and the configuration it is in afterwards (include/rsx.h; csrc/odometry.hip: OdoConfig, check_config).
TEST INFRASTRUCTURE ONLY.

State: (estimator, tracker, compensation, phasecorr) with estimator in ESTIMATORS + ("cfear",) -- the SELECTED estimator, which
phase correlation as the estimator stands in for but does not replace --, tracker and compensation booleans, phasecorr in PC_MODES.
Action: (setter, argument); `False` / "off" is the setter's NULL form.  apply(state, action) -> (accepted, next state).

What an accepted action changes:
  set_estimator(e)       estimator = e, tracker off; ESTIMATE off (selecting an estimator leaves it)
  set_cfear(on)          estimator = cfear; ESTIMATE off            set_cfear(off): estimator = orora, tracker off; ESTIMATE off
  set_cfear_tracking     tracker                                    set_compensation: compensation
  set_phasecorr(m)       phasecorr = m ("off": the state before, i.e. the selected estimator alone)
An action is rejected when the configuration it would give breaks a rule (broken_rule), and then changes nothing:
  the tracker needs CFEAR; compensation excludes mcransac, cfear and any phase correlation; the tracker excludes any phase correlation."""
import itertools

ESTIMATORS = ("orora", "ransac", "mcransac")
PC_MODES = ("off", "estimate", "fallback")
FRESH = ("orora", False, False, "off")
ACTIONS = tuple([("set_estimator", e) for e in ESTIMATORS] + [(s, on) for s in ("set_cfear", "set_cfear_tracking", "set_compensation") for on in (True, False)]
                + [("set_phasecorr", m) for m in ("estimate", "fallback", "off")])
OFF = (("set_phasecorr", "off"), ("set_compensation", False), ("set_cfear_tracking", False), ("set_cfear", False), ("set_estimator", "orora"))


def broken_rule(state):
    """the first rule `state` breaks, or None"""
    est, track, comp, pc = state
    if track and est != "cfear":
        return "the tracker needs CFEAR"
    if comp and est == "mcransac":
        return "compensation excludes MC-RANSAC"
    if comp and est == "cfear":
        return "compensation excludes CFEAR"
    if comp and pc != "off":
        return "compensation excludes phase correlation"
    if track and pc != "off":
        return "the tracker excludes phase correlation"
    return None


def candidate(state, action):
    est, track, comp, pc = state
    setter, arg = action
    if setter in ("set_estimator", "set_cfear") and pc == "estimate":
        pc = "off"
    if setter == "set_estimator":
        est, track = arg, False
    elif setter == "set_cfear":
        est, track = ("cfear", track) if arg else ("orora", False)
    elif setter == "set_cfear_tracking":
        track = bool(arg)
    elif setter == "set_compensation":
        comp = bool(arg)
    elif setter == "set_phasecorr":
        pc = arg
    else:
        raise ValueError(setter)
    return (est, track, comp, pc)


def apply(state, action):
    c = candidate(state, action)
    return (True, c) if broken_rule(c) is None else (False, state)


def walk(actions, state=FRESH):
    """-> ([accepted per action], final state)"""
    accepted = []
    for a in actions:
        ok, state = apply(state, a)
        accepted.append(ok)
    return accepted, state


def sequences(max_len=3):
    """every sequence of 1 .. max_len actions"""
    return [s for n in range(1, max_len + 1) for s in itertools.product(ACTIONS, repeat=n)]


def routes(max_len=3):
    """{state reachable from FRESH: (shortest, longest)} over sequences(max_len) ending in it; among the longest the one with the most
    rejected actions, so that a route walks through refusals where one exists"""
    best = {FRESH: ((), ())}
    for s in sequences(max_len):
        accepted, state = walk(s)
        short, long_ = best.get(state, (s, s))
        if len(s) < len(short):
            short = s
        if (len(s), accepted.count(False)) > (len(long_), walk(long_)[0].count(False)):
            long_ = s
        best[state] = (short, long_)
    return best
