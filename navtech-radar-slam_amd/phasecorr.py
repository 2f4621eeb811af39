"""Host-side wrapper of the phase-correlation entry points of librsx.so (include/rsx.h, rsx_phasecorr_*): polar scans and (src, dst)
index pairs in, the planar transform taking src into dst's frame out -- dense, correspondence-free, no start value."""
import ctypes as C

import numpy as np

from ._rsx import PHASECORR_RESULT_DTYPE, PhasecorrParams, check, lib


def default_params():
    """N 256 at 0.5 m per pixel, 0.0595 m per range bin, min_range_bins 58, resolve_half_turn 1, max_rotation 0 (unlimited)."""
    p = PhasecorrParams()
    check(lib().rsx_phasecorr_default_params(C.byref(p)))
    return p


def params(**fields):
    """default_params() with the given fields replaced."""
    p = default_params()
    for name, value in fields.items():
        if not hasattr(p, name):
            raise TypeError("rsx_phasecorr_params has no field " + name)
        setattr(p, name, value)
    return p


class Phasecorr:
    """one handle per image shape and parameter set (the resampling map and the windows are made at creation)"""

    def __init__(self, rows, cols, params=None, device=0):
        self._L = lib()
        self._h = C.c_void_p()
        self.rows, self.cols = rows, cols
        self.params = params if params is not None else default_params()
        check(self._L.rsx_phasecorr_create(device, rows, cols, C.byref(self.params), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.rsx_phasecorr_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def register_batch(self, images, pairs, col_offset=0, cart=False):
        """images: [n_images, rows, row_stride] uint8 (power samples at [col_offset, col_offset + cols) of a row); pairs: [n_pairs, 2]
        (src, dst) image indices -> results (n_pairs,) PHASECORR_RESULT_DTYPE, and with cart=True also the psi = 0 images
        [n_images, N, N] float32"""
        images = np.ascontiguousarray(images, dtype=np.uint8)
        assert images.ndim == 3 and images.shape[1] == self.rows
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        n = self.params.n
        res = np.zeros(len(pairs), dtype=PHASECORR_RESULT_DTYPE)
        img = np.zeros((len(images), n, n), dtype=np.float32) if cart else None
        check(self._L.rsx_phasecorr_register_batch(self._h, images.ctypes.data, len(images), images.strides[0], images.strides[1], col_offset,
                                                   pairs.ctypes.data, len(pairs), res.ctypes.data, img.ctypes.data if cart else None))
        return (res, img) if cart else res

    def register_batch_device(self, d_images, n_images, image_stride_bytes, row_stride, col_offset, d_pairs, n_pairs, d_results, d_cart=None,
                              stream=None):
        """device pointers (ints); asynchronous on `stream` (an int, None = the handle's own stream)"""
        check(self._L.rsx_phasecorr_register_batch_device(self._h, d_images, n_images, image_stride_bytes, row_stride, col_offset, d_pairs, n_pairs,
                                                          d_results, d_cart, stream))

    def correlation(self, pair):
        """the rotation curve (N,) and the winning translation surface (N, N) of pair `pair` of the last call, float32"""
        n = self.params.n
        curve, surf = np.zeros(n, dtype=np.float32), np.zeros((n, n), dtype=np.float32)
        check(self._L.rsx_phasecorr_correlation(self._h, pair, curve.ctypes.data, surf.ctypes.data))
        return curve, surf
