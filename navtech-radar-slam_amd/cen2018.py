"""Host-side wrapper of the cen2018 keypoint extraction entry points of librsx.so (include/rsx.h, rsx_cen2018_*): polar
radar power image in, keypoints (azimuth idx, range idx) and Cartesian points out.  Same shapes as cen2019.Cen2019."""
import ctypes as C

import numpy as np

from ._keypoints import _Extractor
from ._rsx import Cen2018Params, check, lib


def default_params():
    """zq = 3.0, sigma_gauss = 17, min_range = 58 (yeti_radar_odometry's cen2018 defaults)."""
    p = Cen2018Params()
    check(lib().rsx_cen2018_default_params(C.byref(p)))
    return p


def params(zq=None, sigma_gauss=None, min_range=None):
    """default_params() with the given fields replaced."""
    p = default_params()
    if zq is not None:
        p.zq = zq
    if sigma_gauss is not None:
        p.sigma_gauss = sigma_gauss
    if min_range is not None:
        p.min_range = min_range
    return p


def gauss_weights(sigma_gauss):
    """The 3 * sigma_gauss normalised filter taps the extraction uses (float32)."""
    w = np.zeros(max(3 * sigma_gauss, 1), dtype=np.float32)
    check(lib().rsx_cen2018_gauss_weights(sigma_gauss, w.ctypes.data, w.size))
    return w


class Cen2018(_Extractor):
    _name = "cen2018"

    @staticmethod
    def default_params():
        return default_params()

    def extract(self, img, col_offset=11, zq=3.0, sigma_gauss=17, min_range=58, azimuths=None, resolution=0.0595,
                max_targets=200000, return_count=False):
        """img: (rows, row_stride) uint8.  -> targets (n,2) int32 [, xy (n,2) float32 if azimuths] [, the full count]."""
        return self._extract(img, Cen2018Params(zq, sigma_gauss, min_range, 0), col_offset, azimuths, resolution, max_targets, return_count)

    def extract_batch(self, imgs, col_offset=11, zq=3.0, sigma_gauss=17, min_range=58, azimuths=None, resolution=0.0595,
                      max_targets=20000, return_counts=False):
        """imgs: (n, rows, row_stride) uint8 (any image stride) -> list of targets (k_i, 2) int32 [, list of xy (k_i, 2)
        float32] [, counts]; one chain of launches for the whole batch (rsx_cen2018_extract_batch).  azimuths: (rows,)
        shared or (n, rows)."""
        return self._extract_batch(imgs, Cen2018Params(zq, sigma_gauss, min_range, 0), col_offset, azimuths, resolution, max_targets,
                                   return_counts)

    def debug_image(self, img, col_offset=11, zq=3.0, sigma_gauss=17, min_range=58):
        """rsx_cen2018_debug_image: -> dict(mean (rows,), sigma (rows,), p (rows, cols), y (rows, cols)) of one image."""
        img = np.ascontiguousarray(img, dtype=np.uint8)
        p = Cen2018Params(zq, sigma_gauss, min_range, 0)
        mean = np.zeros(self.rows, dtype=np.float32)
        sigma = np.zeros(self.rows, dtype=np.float32)
        pim = np.zeros((self.rows, self.cols), dtype=np.float32)
        yim = np.zeros((self.rows, self.cols), dtype=np.float32)
        check(self._L.rsx_cen2018_debug_image(self._h, img.ctypes.data, img.shape[1], col_offset, C.byref(p), mean.ctypes.data,
                                              sigma.ctypes.data, pim.ctypes.data, yim.ctypes.data))
        return {"mean": mean, "sigma": sigma, "p": pim, "y": yim}
