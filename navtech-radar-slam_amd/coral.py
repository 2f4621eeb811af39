"""Host-side wrapper of the CorAl entry points of librsx.so (include/rsx.h, rsx_coral_*): pairs of clouds and the transform between
them in, the alignment quality of each pair out (mean joint minus mean separate differential entropy: about 0 when aligned)."""
import ctypes as C
import math

import numpy as np

from ._rsx import CORAL_POINT_DTYPE, CORAL_RESULT_DTYPE, CoralParams, check, lib
from .cfear import ragged


def default_params():
    """radius 3.5 m, min_points 6, min_other 1, det_min 1e-6 m^4."""
    p = CoralParams()
    check(lib().rsx_coral_default_params(C.byref(p)))
    return p


def params(**fields):
    """default_params() with the given fields replaced."""
    p = default_params()
    for name, value in fields.items():
        if not hasattr(p, name):
            raise TypeError("rsx_coral_params has no field " + name)
        setattr(p, name, value)
    return p


def pose_matrices(poses):
    """(n, 3) x, y, yaw -> (n, 6) float64 r00, r01, tx, r10, r11, ty: B into A's frame, cosine and sine taken here on the host"""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    out = np.zeros((len(poses), 6), dtype=np.float64)
    for i, (x, y, yaw) in enumerate(poses):
        c, s = math.cos(float(yaw)), math.sin(float(yaw))
        out[i] = (c, -s, x, s, c, y)
    return out


def _ref(p):
    return C.byref(p) if p is not None else None


class Coral:
    def __init__(self, device=0):
        self._L = lib()
        self._h = C.c_void_p()
        check(self._L.rsx_coral_create(device, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.rsx_coral_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def quality(self, clouds_a, clouds_b, poses=None, transforms=None, params=None, points=False):
        """clouds_a, clouds_b: lists of (n_i, 2) float32 (job i judges clouds_b[i] against clouds_a[i]); poses: (n, 3) x, y, yaw
        taking B into A's frame, or transforms: (n, 6) float64 (r00, r01, tx, r10, r11, ty); neither: the identity
        -> results (n,) CORAL_RESULT_DTYPE, and with points=True also the list of per-point records (n_a + n_b,) CORAL_POINT_DTYPE"""
        if poses is not None and transforms is not None:
            raise TypeError("give poses or transforms, not both")
        a, a_off = ragged(clouds_a, np.float32, 2)
        b, b_off = ragged(clouds_b, np.float32, 2)
        n = len(clouds_a)
        assert len(clouds_b) == n
        if poses is not None:
            transforms = pose_matrices(poses)
        if transforms is not None:
            transforms = np.ascontiguousarray(transforms, dtype=np.float64).reshape(n, 6)
        res = np.zeros(n, dtype=CORAL_RESULT_DTYPE)
        pts = np.zeros(len(a) + len(b), dtype=CORAL_POINT_DTYPE) if points else None
        check(self._L.rsx_coral_quality_batch(self._h, a.ctypes.data, a_off.ctypes.data, b.ctypes.data, b_off.ctypes.data, n,
                                              transforms.ctypes.data if transforms is not None else None, _ref(params), res.ctypes.data,
                                              pts.ctypes.data if points else None))
        if not points:
            return res
        first = a_off + b_off
        return res, [pts[first[i]:first[i + 1]].copy() for i in range(n)]

    def quality_device(self, d_a, d_a_offsets, d_b, d_b_offsets, n_jobs, d_results, d_transforms=None, d_points=None, point_stride=2,
                       params=None, stream=None):
        """device pointers (ints); asynchronous on `stream` (an int, None = the handle's own stream)"""
        check(self._L.rsx_coral_quality_batch_device(self._h, d_a, d_a_offsets, d_b, d_b_offsets, point_stride, n_jobs, d_transforms, _ref(params),
                                                     d_results, d_points, stream))
