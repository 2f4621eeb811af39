"""Host-side wrapper of the CA-CFAR / BFAR keypoint extraction entry points of librsx.so (include/rsx.h, rsx_cfar_*): polar radar
power image in, on every azimuth the k strongest returns above a x (the mean of the training cells around them) + b
(azimuth idx, range idx) and their Cartesian points out.  Same shapes as kstrongest.KStrongest."""
import ctypes as C

from ._keypoints import _Extractor
from ._rsx import CFAR_CA, CFAR_GO, CFAR_SO, CfarParams, check, lib  # noqa: F401

_FIELDS = ("k", "train", "guard", "scale_q8", "offset", "mode", "min_range", "max_range", "min_separation")


def default_params():
    """k = 12, train = 20, guard = 2, scale_q8 = 768 (a = 3), offset = 20, mode = CFAR_CA, min_range = 58, max_range = 0 (the whole
    row), min_separation = 5."""
    p = CfarParams()
    check(lib().rsx_cfar_default_params(C.byref(p)))
    return p


def params(**fields):
    """default_params() with the given fields (k, train, guard, scale_q8, offset, mode, min_range, max_range, min_separation) replaced."""
    p = default_params()
    for name, value in fields.items():
        if name not in _FIELDS:
            raise TypeError("unknown CFAR parameter %r" % name)
        if value is not None:
            setattr(p, name, value)
    return p


class Cfar(_Extractor):
    _name = "cfar"

    @staticmethod
    def default_params():
        return default_params()

    def extract(self, img, col_offset=11, azimuths=None, resolution=0.0595, max_targets=200000, return_count=False, **fields):
        """img: (rows, row_stride) uint8; fields: as params().  -> targets (n,2) int32 [, xy (n,2) float32 if azimuths] [, the full count]."""
        return self._extract(img, params(**fields), col_offset, azimuths, resolution, max_targets, return_count)

    def extract_batch(self, imgs, col_offset=11, azimuths=None, resolution=0.0595, max_targets=20000, return_counts=False, **fields):
        """imgs: (n, rows, row_stride) uint8 (any image stride) -> list of targets (k_i, 2) int32 [, list of xy (k_i, 2)
        float32] [, counts]; one chain of launches for the whole batch (rsx_cfar_extract_batch).  azimuths: (rows,)
        shared or (n, rows)."""
        return self._extract_batch(imgs, params(**fields), col_offset, azimuths, resolution, max_targets, return_counts)
