"""numpy restatement of the grid-map tracker (include/rsx.h, rsx_gridmap_tracker_*): the arithmetic contract of csrc/gridtrack.hip.  None
of this is in the reference checkout -- parity unpinned.  Per scan: a correlative match on the grid (tests/gridmatch_np.py) around a
constant-velocity prediction, the refinement below the cell (tests/gridrefine_np.py), and the composition of the motion.  The glue is
fp64 on plain operations, nothing fused, every expression formed in the order written; no square root, sine or cosine.

Poses are six doubles r00 r01 tx r10 r11 ty.  A sequence's state: the pose P, the motion M (the identity after a reset) and n, the scans
seen since the reset."""
import numpy as np

import gridmatch_np as gx
import gridrefine_np as gr

LOST = 1
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)

RESULT = np.dtype([("transform", np.float64, 6), ("start", np.float64, 6), ("match", gx.RESULT), ("refine", gr.RESULT), ("flags", np.int32),
                   ("reserved", np.int32)])   # rsx_gridmap_track_result, 344 bytes
assert RESULT.itemsize == 344


def params(min_score=0, predict=1, **kw):
    """-> dict(match=, refine=, min_score=, predict=): the window K = U = V = 2 of 0.01 rad and the refinement's defaults, with the
    given fields of either part replaced by name"""
    match = {k: kw.pop(k) for k in list(kw) if k in gx.DEFAULTS}
    return dict(match=gx.params(**dict(dict(angle_steps=2, x_cells=2, y_cells=2, angle_step=0.01), **match)), refine=gr.params(**kw),
                min_score=min_score, predict=predict)


def mul(A, B):
    A, B = [np.float64(v) for v in A], [np.float64(v) for v in B]
    return [A[0] * B[0] + A[1] * B[3], A[0] * B[1] + A[1] * B[4], (A[0] * B[2] + A[1] * B[5]) + A[2],
            A[3] * B[0] + A[4] * B[3], A[3] * B[1] + A[4] * B[4], (A[3] * B[2] + A[4] * B[5]) + A[5]]


def inv(A):
    A = [np.float64(v) for v in A]
    return [A[0], A[3], -(A[0] * A[2] + A[3] * A[5]), A[1], A[4], -(A[1] * A[2] + A[4] * A[5])]


def renorm(T):
    """one Newton step towards a unit first column; the second column is rebuilt from the first"""
    T = [np.float64(v) for v in T]
    n2 = T[0] * T[0] + T[3] * T[3]
    f = np.float64(1.5) - np.float64(0.5) * n2
    c, s = T[0] * f, T[3] * f
    return [c, -s, T[2], s, c, T[5]]


class State:
    """one sequence: P, M (lists of six float64) and n"""

    def __init__(self, pose=IDENTITY):
        self.P, self.M, self.n = [np.float64(v) for v in pose], [np.float64(v) for v in IDENTITY], 0

    def copy(self):
        s = State(self.P)
        s.M, s.n = list(self.M), self.n
        return s


def step(L, xy, st, p, tp, device_entry=False, renormalise=renorm, match_fn=None, refine_fn=None):
    """one scan: st is updated in place -> a RESULT scalar.  renormalise: tests replace it to show what the rule would be without it;
    match_fn(xy, prior), refine_fn(xy, prior) -> the record of one job: tests chain the library's stand-alone entries through them"""
    xy = np.asarray(xy, dtype=np.float32).reshape(-1, 2)
    off = np.array([0, len(xy)], dtype=np.int64)
    with np.errstate(all="ignore"):
        start = list(st.P) if st.n == 0 or tp["predict"] == 0 else renormalise(mul(st.P, st.M))
        rec = np.zeros((), dtype=RESULT)
        rec["start"] = start
        m = match_fn(xy, start) if match_fn else gx.match_batch(L, xy, off, [start], p, tp["match"], device_entry=device_entry)[0][0]
        rec["match"] = m
        if m["status"] != 0 or m["score"] < tp["min_score"]:
            st.P = start
            rec["flags"] = LOST
        else:
            r = refine_fn(xy, m["transform"]) if refine_fn else gr.refine_batch(L, xy, off, [m["transform"]], p, tp["refine"], device_entry=device_entry)[0]
            rec["refine"] = r
            new = renormalise(r["transform"])
            if st.n > 0:
                st.M = mul(inv(st.P), new)
            st.P = new
        st.n += 1
        rec["transform"] = st.P
    return rec


def push(L, clouds_per_sequence, states, p, tp, device_entry=False, **hooks):
    """clouds_per_sequence[q]: the next scans of sequence q; states[q] is updated in place -> records [total scans] of RESULT, sequence
    after sequence.  hooks: step's"""
    out = [step(L, xy, st, p, tp, device_entry=device_entry, **hooks) for seq, st in zip(clouds_per_sequence, states) for xy in seq]
    return np.array(out, dtype=RESULT) if out else np.zeros(0, dtype=RESULT)


def det(T):
    return float(T[0]) * float(T[4]) - float(T[1]) * float(T[3])
