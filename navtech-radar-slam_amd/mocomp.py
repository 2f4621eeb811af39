"""Host-side wrapper of the motion / Doppler compensation entry points of librsx.so (include/rsx.h: rsx_mocomp_*): radar
keypoints (or the matched keypoints of scan pairs) and a velocity (a pose) per scan (pair) in, the keypoints expressed in the
sensor frame at their scan's start out.  Computation happens in mocomp.hip on the GPU."""
import ctypes as C

import numpy as np

from ._rsx import MOCOMP_DESKEW, MOCOMP_DOPPLER, MOCOMP_STATUS_ANGLE, MocompParams, check, lib  # noqa: F401


def default_params(**kw):
    """the library's defaults (both corrections), fields overridden by keyword"""
    p = MocompParams()
    check(lib().rsx_mocomp_default_params(C.byref(p)))
    for k, v in kw.items():
        if k not in dict(MocompParams._fields_):
            raise TypeError(k)
        setattr(p, k, v)
    return p


class Mocomp:
    def __init__(self, device=0):
        self._L = lib()
        self._h = C.c_void_p()
        check(self._L.rsx_mocomp_create(device, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.rsx_mocomp_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def points_batch(self, xy, rows, offsets, w, params=None):
        """xy (M,2) float32, rows (M,) int32, offsets (n_scans+1,) int64, w (n_scans,3) float64 -> xy (M,2) float32, status (n_scans,) int32"""
        xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        w = np.ascontiguousarray(w, dtype=np.float64).reshape(-1, 3)
        n = off.size - 1
        out = np.zeros((max(len(xy), 1), 2), dtype=np.float32)
        status = np.zeros(max(n, 1), dtype=np.int32)
        pp = C.byref(params) if params is not None else None
        check(self._L.rsx_mocomp_points_batch(self._h, xy.ctypes.data, rows.ctypes.data, off.ctypes.data, n, w.ctypes.data, pp, out.ctypes.data,
                                              status.ctypes.data))
        return out[:len(xy)], status[:n]

    def matches_batch(self, src_xy, dst_xy, a_cur, a_prev, offsets, pose, params=None):
        """src_xy, dst_xy (M,2) float32, a_cur, a_prev (M,) int32, offsets (n_pairs+1,) int64, pose (n_pairs,3) float64 (x, y, yaw)
        -> src (M,2), dst (M,2) float32, status (n_pairs,) int32"""
        src = np.ascontiguousarray(src_xy, dtype=np.float32).reshape(-1, 2)
        dst = np.ascontiguousarray(dst_xy, dtype=np.float32).reshape(-1, 2)
        ac = np.ascontiguousarray(a_cur, dtype=np.int32)
        ap = np.ascontiguousarray(a_prev, dtype=np.int32)
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        pose = np.ascontiguousarray(pose, dtype=np.float64).reshape(-1, 3)
        n = off.size - 1
        osrc = np.zeros((max(len(src), 1), 2), dtype=np.float32)
        odst = np.zeros((max(len(src), 1), 2), dtype=np.float32)
        status = np.zeros(max(n, 1), dtype=np.int32)
        pp = C.byref(params) if params is not None else None
        check(self._L.rsx_mocomp_matches_batch(self._h, src.ctypes.data, dst.ctypes.data, ac.ctypes.data, ap.ctypes.data, off.ctypes.data, n,
                                               pose.ctypes.data, pp, osrc.ctypes.data, odst.ctypes.data, status.ctypes.data))
        return osrc[:len(src)], odst[:len(src)], status[:n]

    def points_batch_device(self, xy_ptr, rows_ptr, off_ptr, n_scans, w_ptr, out_ptr, status_ptr=None, params=None, stream=0):
        pp = C.byref(params) if params is not None else None
        check(self._L.rsx_mocomp_points_batch_device(self._h, xy_ptr, rows_ptr, off_ptr, n_scans, w_ptr, pp, out_ptr, status_ptr, stream))

    def matches_batch_device(self, src_ptr, dst_ptr, a_cur_ptr, a_prev_ptr, off_ptr, n_pairs, pose_ptr, out_src_ptr, out_dst_ptr, status_ptr=None,
                             params=None, stream=0):
        pp = C.byref(params) if params is not None else None
        check(self._L.rsx_mocomp_matches_batch_device(self._h, src_ptr, dst_ptr, a_cur_ptr, a_prev_ptr, off_ptr, n_pairs, pose_ptr, pp, out_src_ptr,
                                                      out_dst_ptr, status_ptr, stream))
