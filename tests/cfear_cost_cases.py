"""Inputs and expected results shared by the tests of CFEAR's costs, losses and weights (tests/test_cfear_cost_restatement.py,
tests/test_gpu_cfear_cost.py): the restatement tests/cfear_cost_np.py on the pairs and the joint jobs of tests/cfear_track_cases.py
and on the small sequence, per combination (cost, loss, weights).  Everything is computed once per process
(functools.lru_cache) and must be left unchanged by its users."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cfear_cost_np as cc  # noqa: E402
import cfear_mocomp_cases as mcases  # noqa: E402
import cfear_track_cases as cases  # noqa: E402

ID = (0.0, 0.0, 0.0)
COMBINATIONS = cc.COMBINATIONS
OTHERS = COMBINATIONS[1:]  # the 17 that are not today's
TRACKED = ((cc.COST_P2P, cc.LOSS_CAUCHY, 1), (cc.COST_P2D, cc.LOSS_HUBER, 0))  # the combinations the tracker is tested under


def as_kw(combo):
    return dict(cost=combo[0], loss=combo[1], weights=combo[2])


@functools.lru_cache(maxsize=None)
def pair_wants(combo):
    """the restatement on cases.pair_cases(), in their order"""
    return tuple(cc.register(c[1], c[2], init=c[3] if c[3] is not None else ID, **c[4], **as_kw(combo)) for c in cases.pair_cases())


# A case whose restatement decides something less than 1e-9 from its threshold gets another input here, for that combination alone
# (the bar stays, the case stays).  Under P2L / Huber / weights "drive K = 3" has a margin of 9.8e-10 from the start pose of
# cases.joint_jobs(); started 5 cm and 3 mrad beside it the smallest margin is 2.7e-8 and the job ends where it ended
MOVED_STARTS = {((cc.COST_P2L, cc.LOSS_HUBER, 1), "drive K = 3"): (0.05, -0.02, 0.003)}


@functools.lru_cache(maxsize=None)
def joint_jobs(combo):
    """cases.joint_jobs() (groups of up to three keyframes) as this combination is tested on them"""
    out = []
    for j in cases.joint_jobs():
        d = MOVED_STARTS.get((combo, j[0]))
        out.append(j if d is None else j[:4] + (tuple(v + w for v, w in zip(j[4], d)),) + j[5:])
    return tuple(out)


@functools.lru_cache(maxsize=None)
def joint_wants(combo):
    """the restatement on joint_jobs(combo), in their order"""
    return tuple(cc.register_keyframes(j[1], list(j[2]), list(j[3]), init=j[4], **as_kw(combo)) for j in joint_jobs(combo))


@functools.lru_cache(maxsize=None)
def small_track(combo, compensate):
    """the restatement's track of the small sequence (keyframe_distance 0.5: the ring fills and evicts), untimed or compensated"""
    recs, taus = mcases.small_timed()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(recs, cases.small()[0]))
    return tuple(cc.track(recs, taus if compensate else None, compensate=compensate, **cases.SMALL_TRACK, **as_kw(combo)))


def poisoned(rec, field="lambda_min"):
    """rec with that field of every fifth record made 0, -1 or NaN in turn: records the validity test refuses"""
    out = rec.copy()
    bad = np.array([0.0, -1.0, np.nan], dtype=np.float32)
    idx = np.arange(2, len(out), 5)
    out[field][idx] = bad[np.arange(len(idx)) % 3]
    return out
