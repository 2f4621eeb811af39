"""What the host-side wrappers of the keypoint extractors (cen2018.Cen2018, cen2019.Cen2019, kstrongest.KStrongest, cfar.Cfar) share: the handle, the
calls of rsx_<name>_extract / rsx_<name>_extract_batch with their output arrays, and how the results are returned."""
import ctypes as C

import numpy as np

from ._rsx import check, lib


class _Extractor:
    _name = None  # "cen2018": the entry points are rsx_cen2018_*

    def __init__(self, rows=400, cols=3360, device=0):
        self._L = lib()
        self.rows, self.cols = rows, cols
        self._h = C.c_void_p()
        check(self._fn("create")(device, rows, cols, C.byref(self._h)))

    def _fn(self, entry):
        return getattr(self._L, "rsx_%s_%s" % (self._name, entry))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._fn("destroy")(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _result(targets, xy, counts, want_counts):
        """-> targets [, xy if there is one] [, counts if wanted]: a tuple, or targets alone."""
        res = (targets,) + ((xy,) if xy is not None else ()) + ((counts,) if want_counts else ())
        return res if len(res) > 1 else res[0]

    def _extract(self, img, p, col_offset, azimuths, resolution, max_targets, return_count=False):
        """img: (rows, row_stride) uint8, p: the params struct.  -> targets (k, 2) int32 [, xy (k, 2) float32 if azimuths] [, the full count]."""
        img = np.ascontiguousarray(img, dtype=np.uint8)
        assert img.shape[0] == self.rows
        out = np.zeros((max(max_targets, 1), 2), dtype=np.int32)
        xy = np.zeros((max(max_targets, 1), 2), dtype=np.float32) if azimuths is not None else None
        az = np.ascontiguousarray(azimuths, dtype=np.float32) if azimuths is not None else None
        n = C.c_int32()
        check(self._fn("extract")(self._h, img.ctypes.data, img.shape[1], col_offset, C.byref(p),
                                  az.ctypes.data if az is not None else None, resolution, out.ctypes.data,
                                  xy.ctypes.data if xy is not None else None, max_targets, C.byref(n)))
        k = min(n.value, max_targets)
        return self._result(out[:k].copy(), xy[:k].copy() if xy is not None else None, n.value, return_count)

    def _extract_batch(self, imgs, p, col_offset, azimuths, resolution, max_targets, return_counts=False):
        """imgs: (n, rows, row_stride) uint8 (any image stride; copied when a row or a bin is strided).  -> list of targets
        (k_i, 2) int32 [, list of xy (k_i, 2) float32 if azimuths] [, counts (n,) int32]."""
        imgs = np.asarray(imgs, dtype=np.uint8)
        if imgs.strides[1:] != (imgs.shape[2], 1):
            imgs = np.ascontiguousarray(imgs)
        n = imgs.shape[0]
        assert imgs.shape[1] == self.rows
        mt = max(max_targets, 1)
        out = np.zeros((n, mt, 2), dtype=np.int32)
        az = np.ascontiguousarray(azimuths, dtype=np.float32) if azimuths is not None else None
        xy = np.zeros((n, mt, 2), dtype=np.float32) if az is not None else None
        counts = np.zeros(n, dtype=np.int32)
        check(self._fn("extract_batch")(self._h, imgs.ctypes.data, n, imgs.strides[0], imgs.shape[2], col_offset, C.byref(p),
                                        az.ctypes.data if az is not None else None,
                                        1 if (az is not None and az.ndim == 2) else 0, resolution, out.ctypes.data,
                                        xy.ctypes.data if xy is not None else None, max_targets, counts.ctypes.data))
        ks = np.minimum(counts, max_targets)
        return self._result([out[i, :ks[i]].copy() for i in range(n)],
                            [xy[i, :ks[i]].copy() for i in range(n)] if xy is not None else None, counts, return_counts)
