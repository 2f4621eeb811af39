"""Host-side wrapper of the CFEAR entry points of librsx.so (include/rsx.h, rsx_cfear_*): keypoint clouds in, oriented surface
points out; pairs of surface-point sets in, the point-to-line registration of each pair out; a scan and its keyframes in, the
joint registration out; sequences of surface-point sets in, their keyframe-tracked poses out."""
import ctypes as C

import numpy as np

from ._rsx import (CFEAR_MAX_SURFACE_POINTS, CFEAR_RESULT_DTYPE, CFEAR_SURFACE_POINT_DTYPE, CFEAR_TRACK_RESULT_DTYPE, CfearParams,
                   CfearTrackParams, check, lib)


def default_params():
    """radius 3.5 m, min_points 6, max_condition 1e5, cos_max_normal_angle cos 30 deg, huber_delta 0.1 m, step_epsilon 1e-6,
    max_iterations 50, min_correspondences 6; cost 0 (CFEAR_COST_P2L), loss 0 (CFEAR_LOSS_HUBER), weights 0: the objective of the
    registration, chosen among CFEAR_COST_* x CFEAR_LOSS_* x weights 0 / 1 (include/rsx.h)."""
    p = CfearParams()
    check(lib().rsx_cfear_default_params(C.byref(p)))
    return p


def params(**fields):
    """default_params() with the given fields replaced."""
    p = default_params()
    for name, value in fields.items():
        if not hasattr(p, name):
            raise TypeError("rsx_cfear_params has no field " + name)
        setattr(p, name, value)
    return p


def default_track_params():
    """n_keyframes 3, keyframe_distance 1.5 m, keyframe_rotation 5 deg, predict 1, search 0 (the cell index), compensate 0."""
    p = CfearTrackParams()
    check(lib().rsx_cfear_default_track_params(C.byref(p)))
    return p


def track_params(**fields):
    """default_track_params() with the given fields replaced."""
    p = default_track_params()
    for name, value in fields.items():
        if not hasattr(p, name):
            raise TypeError("rsx_cfear_track_params has no field " + name)
        setattr(p, name, value)
    return p


def _ref(p):
    return C.byref(p) if p is not None else None


def ragged(parts, dtype, width=None):
    """list of arrays -> (concatenation, offsets int64 [n + 1])"""
    parts = [np.ascontiguousarray(a, dtype=dtype).reshape((-1,) + ((width,) if width else ())) for a in parts]
    offsets = np.zeros(len(parts) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(a) for a in parts])
    flat = np.concatenate(parts) if parts else np.zeros((0,) + ((width,) if width else ()), dtype=dtype)
    return np.ascontiguousarray(flat), offsets


class Cfear:
    def __init__(self, device=0):
        self._L = lib()
        self._h = C.c_void_p()
        check(self._L.rsx_cfear_create(device, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.rsx_cfear_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def surface_points(self, clouds, params=None, max_records=CFEAR_MAX_SURFACE_POINTS, raw=False):
        """clouds: list of (n_i, 2) float32 -> (list of records (k_i,) CFEAR_SURFACE_POINT_DTYPE, counts, status words).
        raw: the whole (n, max_records) record buffer in place of the list."""
        xy, offsets = ragged(clouds, np.float32, 2)
        n = len(clouds)
        rec = np.zeros((n, max_records), dtype=CFEAR_SURFACE_POINT_DTYPE)
        counts, status = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        check(self._L.rsx_cfear_surface_points_batch(self._h, xy.ctypes.data, offsets.ctypes.data, n, C.byref(params) if params is not None else None,
                                                     rec.ctypes.data, max_records, counts.ctypes.data, status.ctypes.data))
        if raw:
            return rec, counts, status
        return [rec[i, :min(int(counts[i]), max_records)].copy() for i in range(n)], counts, status

    def surface_points_timed(self, clouds, rows, n_rows, params=None, max_records=CFEAR_MAX_SURFACE_POINTS):
        """surface_points with the azimuth row of every point (rows: list of (n_i,) int32 in [0, n_rows))
        -> (list of records, list of times (k_i,) float32, counts, status words)"""
        xy, offsets = ragged(clouds, np.float32, 2)
        a, _ = ragged(rows, np.int32)
        assert len(a) == len(xy)
        n = len(clouds)
        rec = np.zeros((n, max_records), dtype=CFEAR_SURFACE_POINT_DTYPE)
        tau = np.zeros((n, max_records), dtype=np.float32)
        counts, status = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        check(self._L.rsx_cfear_surface_points_timed_batch(self._h, xy.ctypes.data, a.ctypes.data, n_rows, offsets.ctypes.data, n, _ref(params),
                                                           rec.ctypes.data, tau.ctypes.data, max_records, counts.ctypes.data, status.ctypes.data))
        keep = [min(int(c), max_records) for c in counts]
        return [rec[i, :k].copy() for i, k in enumerate(keep)], [tau[i, :k].copy() for i, k in enumerate(keep)], counts, status

    def compensate(self, records, taus, motions):
        """scan i's records (measured at taus[i], fractions of the scan period) compensated with motions[i] = (x, y, yaw), the
        sensor's motion over one scan period -> (list of records, status words: 1 = left as measured)"""
        rec, offsets = ragged(records, CFEAR_SURFACE_POINT_DTYPE)
        tau, _ = ragged(taus, np.float32)
        assert len(tau) == len(rec)
        n = len(records)
        motions = np.ascontiguousarray(motions, dtype=np.float64).reshape(n, 3)
        out, status = np.zeros_like(rec), np.zeros(n, dtype=np.int32)
        check(self._L.rsx_cfear_compensate_batch(self._h, rec.ctypes.data, tau.ctypes.data, offsets.ctypes.data, n, motions.ctypes.data,
                                                 out.ctypes.data, status.ctypes.data))
        return [out[offsets[i]:offsets[i + 1]] for i in range(n)], status

    def register(self, src, dst, init=None, params=None):
        """src, dst: lists of record arrays (pair i registers src[i] to dst[i]); init: (n, 3) float64 or None
        -> (n,) CFEAR_RESULT_DTYPE"""
        s, so = ragged(src, CFEAR_SURFACE_POINT_DTYPE)
        d, do = ragged(dst, CFEAR_SURFACE_POINT_DTYPE)
        n = len(src)
        assert len(dst) == n
        out = np.zeros(n, dtype=CFEAR_RESULT_DTYPE)
        if init is not None:
            init = np.ascontiguousarray(init, dtype=np.float64).reshape(n, 3)
        check(self._L.rsx_cfear_register_batch(self._h, s.ctypes.data, so.ctypes.data, d.ctypes.data, do.ctypes.data, n,
                                               init.ctypes.data if init is not None else None, C.byref(params) if params is not None else None,
                                               out.ctypes.data))
        return out

    def register_keyframes(self, src, keyframes, poses, init=None, params=None, track=None):
        """job i registers src[i] jointly to the record arrays keyframes[i] (a list of 1 .. 4) at poses[i] ((K_i, 3): x, y, yaw
        in the map frame); init: (n, 3) start poses in the map frame or None; track: only its `search` acts
        -> (n,) CFEAR_RESULT_DTYPE, the scans' poses in the map frame"""
        n = len(src)
        assert len(keyframes) == n and len(poses) == n
        s, so = ragged(src, CFEAR_SURFACE_POINT_DTYPE)
        k, ko = ragged([a for job in keyframes for a in job], CFEAR_SURFACE_POINT_DTYPE)
        jo = np.zeros(n + 1, dtype=np.int64)
        jo[1:] = np.cumsum([len(job) for job in keyframes])
        kp = np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.float64).reshape(-1, 3) for p in poses]) if n else np.zeros((0, 3)))
        assert len(kp) == jo[-1]
        out = np.zeros(n, dtype=CFEAR_RESULT_DTYPE)
        if init is not None:
            init = np.ascontiguousarray(init, dtype=np.float64).reshape(n, 3)
        check(self._L.rsx_cfear_register_keyframes_batch(self._h, s.ctypes.data, so.ctypes.data, k.ctypes.data, ko.ctypes.data, jo.ctypes.data,
                                                         kp.ctypes.data, n, init.ctypes.data if init is not None else None, _ref(params),
                                                         _ref(track), out.ctypes.data))
        return out

    # device entries: raw HBM addresses, asynchronous on `stream` (None: the handle's own)
    def register_keyframes_device(self, d_src, d_src_offsets, d_kf, d_kf_offsets, d_kf_job_offsets, d_kf_poses, n_jobs, d_out, d_init=None,
                                  params=None, track=None, stream=None):
        check(self._L.rsx_cfear_register_keyframes_batch_device(self._h, d_src, d_src_offsets, d_kf, d_kf_offsets, d_kf_job_offsets, d_kf_poses,
                                                                n_jobs, d_init, _ref(params), _ref(track), d_out, stream))

    def surface_points_device(self, d_xy, d_offsets, n_scans, d_records, max_records, d_counts, d_status=None, params=None, stream=None):
        check(self._L.rsx_cfear_surface_points_batch_device(self._h, d_xy, d_offsets, n_scans, C.byref(params) if params is not None else None,
                                                            d_records, max_records, d_counts, d_status, stream))

    def surface_points_timed_device(self, d_xy, d_rows, n_rows, d_offsets, n_scans, d_records, d_tau, max_records, d_counts, d_status=None,
                                    params=None, stream=None):
        check(self._L.rsx_cfear_surface_points_timed_batch_device(self._h, d_xy, d_rows, n_rows, d_offsets, n_scans, _ref(params), d_records, d_tau,
                                                                  max_records, d_counts, d_status, stream))

    def compensate_device(self, d_records, d_tau, d_offsets, n_scans, d_motion, d_out, d_status=None, stream=None):
        check(self._L.rsx_cfear_compensate_batch_device(self._h, d_records, d_tau, d_offsets, n_scans, d_motion, d_out, d_status, stream))

    def register_device(self, d_src, d_src_offsets, d_dst, d_dst_offsets, n_pairs, d_out, d_init=None, params=None, stream=None):
        check(self._L.rsx_cfear_register_batch_device(self._h, d_src, d_src_offsets, d_dst, d_dst_offsets, n_pairs, d_init,
                                                      C.byref(params) if params is not None else None, d_out, stream))


class Tracker:
    """n_sequences sequences tracked side by side against their keyframes (rsx_cfear_tracker); the state stays on the device."""

    def __init__(self, n_sequences=1, params=None, track=None, device=0):
        self._L = lib()
        self._h = C.c_void_p()
        self.n_sequences, self.params, self.track = n_sequences, params, track
        check(self._L.rsx_cfear_tracker_create(device, n_sequences, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.rsx_cfear_tracker_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, params=None, track=None):
        """every sequence starts again; the parameters of the pushes that follow"""
        check(self._L.rsx_cfear_tracker_reset(self._h))
        self.params, self.track = params, track

    def push(self, scans):
        """scans: per sequence the list of record arrays it continues with (one sequence: the list itself)
        -> per sequence a (n_scans,) CFEAR_TRACK_RESULT_DTYPE array (one sequence: the array)"""
        single = self.n_sequences == 1 and (len(scans) == 0 or isinstance(scans[0], np.ndarray))
        seqs = [scans] if single else scans
        assert len(seqs) == self.n_sequences
        rec, off = ragged([s for q in seqs for s in q], CFEAR_SURFACE_POINT_DTYPE)
        n_scans = np.array([len(q) for q in seqs], dtype=np.int32)
        out = np.zeros(int(n_scans.sum()), dtype=CFEAR_TRACK_RESULT_DTYPE)
        check(self._L.rsx_cfear_tracker_push(self._h, rec.ctypes.data, off.ctypes.data, n_scans.ctypes.data, _ref(self.params), _ref(self.track),
                                             out.ctypes.data))
        ends = np.cumsum(n_scans)
        parts = [out[e - m:e] for e, m in zip(ends, n_scans)]
        return parts[0] if single else parts

    def push_timed(self, scans, taus):
        """push with the records' times (taus: laid out like scans, (k,) float32 per scan); what track.compensate = 1 needs"""
        single = self.n_sequences == 1 and (len(scans) == 0 or isinstance(scans[0], np.ndarray))
        seqs, tseqs = ([scans], [taus]) if single else (scans, taus)
        assert len(seqs) == self.n_sequences and len(tseqs) == self.n_sequences
        rec, off = ragged([s for q in seqs for s in q], CFEAR_SURFACE_POINT_DTYPE)
        tau, _ = ragged([u for q in tseqs for u in q], np.float32)
        assert len(tau) == len(rec)
        n_scans = np.array([len(q) for q in seqs], dtype=np.int32)
        out = np.zeros(int(n_scans.sum()), dtype=CFEAR_TRACK_RESULT_DTYPE)
        check(self._L.rsx_cfear_tracker_push_timed(self._h, rec.ctypes.data, tau.ctypes.data, off.ctypes.data, n_scans.ctypes.data,
                                                   _ref(self.params), _ref(self.track), out.ctypes.data))
        ends = np.cumsum(n_scans)
        parts = [out[e - m:e] for e, m in zip(ends, n_scans)]
        return parts[0] if single else parts

    def push_timed_device(self, d_records, d_tau, d_offsets, d_n_scans, d_out, stream=None):
        check(self._L.rsx_cfear_tracker_push_timed_device(self._h, d_records, d_tau, d_offsets, d_n_scans, _ref(self.params), _ref(self.track),
                                                          d_out, stream))

    def push_device(self, d_records, d_offsets, d_n_scans, d_out, stream=None):
        """raw HBM addresses, asynchronous on `stream` (None: the handle's own)"""
        check(self._L.rsx_cfear_tracker_push_device(self._h, d_records, d_offsets, d_n_scans, _ref(self.params), _ref(self.track), d_out, stream))


def surface_points(clouds, params=None, device=0):
    """one-shot Cfear(device).surface_points(clouds, params)"""
    h = Cfear(device)
    try:
        return h.surface_points(clouds, params)
    finally:
        h.close()


def register(src, dst, init=None, params=None, device=0):
    """one-shot Cfear(device).register(src, dst, init, params)"""
    h = Cfear(device)
    try:
        return h.register(src, dst, init, params)
    finally:
        h.close()
