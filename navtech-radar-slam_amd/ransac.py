"""Host-side wrapper of the RANSAC / motion-compensated RANSAC entry points of librsx.so (include/rsx.h: rsx_ransac_*):
matched 2-D feature points of two consecutive radar scans in, SE(2) pose (and, motion compensated, the body velocity) out.
Computation happens in ransac.hip on the GPU."""
import ctypes as C

import numpy as np

from ._rsx import RANSAC_MOTION_COMPENSATED, RANSAC_RESULT_DTYPE, RansacParams, check, lib  # noqa: F401


def default_params(mc=False, **kw):
    """the library's defaults, RSX_RANSAC_MOTION_COMPENSATED set with mc, fields overridden by keyword"""
    p = RansacParams()
    check(lib().rsx_ransac_default_params(C.byref(p)))
    if mc:
        p.flags |= RANSAC_MOTION_COMPENSATED
    for k, v in kw.items():
        if k not in dict(RansacParams._fields_):
            raise TypeError(k)
        setattr(p, k, v)
    return p


class Ransac:
    def __init__(self, device=0):
        self._L = lib()
        self._h = C.c_void_p()
        check(self._L.rsx_ransac_create(device, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.rsx_ransac_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def estimate_batch(self, src_xy, dst_xy, offsets, dt=None, params=None, want_mask=True):
        """src_xy, dst_xy: (M,2) float32; dt: (M,) float32 (motion compensated only); offsets: (n_pairs+1,) int64
        -> (n_pairs,) RANSAC_RESULT_DTYPE [, inlier mask (M,) bool]."""
        src = np.ascontiguousarray(src_xy, dtype=np.float32)
        dst = np.ascontiguousarray(dst_xy, dtype=np.float32)
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        tm = np.ascontiguousarray(dt, dtype=np.float32) if dt is not None else None
        n = off.size - 1
        out = np.zeros(n, dtype=RANSAC_RESULT_DTYPE)
        m = int(off[-1]) if off.size else 0
        mask = np.zeros(max(m, 1), dtype=np.uint8) if want_mask else None
        pp = C.byref(params) if params is not None else None
        check(self._L.rsx_ransac_estimate_batch(self._h, src.ctypes.data, dst.ctypes.data, tm.ctypes.data if tm is not None else None,
                                                off.ctypes.data, n, pp, out.ctypes.data, mask.ctypes.data if want_mask else None))
        if want_mask:
            return out, mask[:max(m, 0)].astype(bool)
        return out

    def estimate(self, src_xy, dst_xy, dt=None, params=None):
        src = np.ascontiguousarray(src_xy, dtype=np.float32).reshape(-1, 2)
        out, mask = self.estimate_batch(src, dst_xy, np.array([0, src.shape[0]], dtype=np.int64), dt, params)
        return out[0], mask

    def estimate_batch_device(self, src_ptr, dst_ptr, dt_ptr, off_ptr, n_pairs, out_ptr, inlier_ptr=None, params=None, stream=0):
        pp = C.byref(params) if params is not None else None
        check(self._L.rsx_ransac_estimate_batch_device(self._h, src_ptr, dst_ptr, dt_ptr, off_ptr, n_pairs, pp, out_ptr, inlier_ptr, stream))
