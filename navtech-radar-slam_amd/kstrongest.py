"""Host-side wrapper of the k-strongest keypoint extraction entry points of librsx.so (include/rsx.h, rsx_kstrongest_*): polar
radar power image in, on every azimuth the k strongest returns above a power floor (azimuth idx, range idx) and their
Cartesian points out.  Same shapes as cen2018.Cen2018 and cen2019.Cen2019."""
import ctypes as C

from ._keypoints import _Extractor
from ._rsx import KStrongestParams, check, lib


def default_params():
    """k = 12, z_min = 60 (CFEAR radar odometry), min_range = 58, max_range = 0 (the whole row), min_separation = 5."""
    p = KStrongestParams()
    check(lib().rsx_kstrongest_default_params(C.byref(p)))
    return p


def params(k=None, z_min=None, min_range=None, max_range=None, min_separation=None):
    """default_params() with the given fields replaced."""
    p = default_params()
    for name, value in (("k", k), ("z_min", z_min), ("min_range", min_range), ("max_range", max_range), ("min_separation", min_separation)):
        if value is not None:
            setattr(p, name, value)
    return p


class KStrongest(_Extractor):
    _name = "kstrongest"

    @staticmethod
    def default_params():
        return default_params()

    def extract(self, img, col_offset=11, k=12, z_min=60, min_range=58, max_range=0, min_separation=5, azimuths=None, resolution=0.0595,
                max_targets=200000, return_count=False):
        """img: (rows, row_stride) uint8.  -> targets (n,2) int32 [, xy (n,2) float32 if azimuths] [, the full count]."""
        return self._extract(img, KStrongestParams(k, z_min, min_range, max_range, min_separation, 0), col_offset, azimuths, resolution,
                             max_targets, return_count)

    def extract_batch(self, imgs, col_offset=11, k=12, z_min=60, min_range=58, max_range=0, min_separation=5, azimuths=None,
                      resolution=0.0595, max_targets=20000, return_counts=False):
        """imgs: (n, rows, row_stride) uint8 (any image stride) -> list of targets (k_i, 2) int32 [, list of xy (k_i, 2)
        float32] [, counts]; one chain of launches for the whole batch (rsx_kstrongest_extract_batch).  azimuths: (rows,)
        shared or (n, rows)."""
        return self._extract_batch(imgs, KStrongestParams(k, z_min, min_range, max_range, min_separation, 0), col_offset, azimuths,
                                   resolution, max_targets, return_counts)
