"""Host-side wrapper of the cen2019 keypoint extraction entry points of librsx.so (include/rsx.h):
polar radar power image in, keypoints (azimuth idx, range idx) and Cartesian points out."""
import ctypes as C

import numpy as np

from ._keypoints import _Extractor
from ._rsx import Cen2019Params, check, lib


def default_params():
    p = Cen2019Params()
    check(lib().rsx_cen2019_default_params(C.byref(p)))
    return p


class Cen2019(_Extractor):
    _name = "cen2019"

    def extract(self, img, col_offset=11, max_points=10000, min_range=58, azimuths=None, resolution=0.0595,
                max_targets=200000):
        """img: (rows, row_stride) uint8.  -> targets (n,2) int32 [, xy (n,2) float32 if azimuths]."""
        return self._extract(img, Cen2019Params(max_points, min_range), col_offset, azimuths, resolution, max_targets)

    def extract_batch(self, imgs, col_offset=11, max_points=10000, min_range=58, azimuths=None, resolution=0.0595,
                      max_targets=20000):
        """imgs: (n, rows, row_stride) uint8 -> list of targets (k_i, 2) int32 [, list of xy (k_i, 2) float32]; one chain
        of launches for the whole batch (rsx_cen2019_extract_batch).  azimuths: (rows,) shared or (n, rows)."""
        return self._extract_batch(np.ascontiguousarray(imgs, dtype=np.uint8), Cen2019Params(max_points, min_range), col_offset, azimuths,
                                   resolution, max_targets)
