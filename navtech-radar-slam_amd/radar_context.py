"""Host-side wrapper of the radar scan-context builder of librsx.so (include/rsx.h, rsx_radarsc_*): polar radar power images
in, 20 x 60 descriptors of received power (f32 sector-major, 1200 floats per scan) out -- what SCManager.add_descriptors_f32 /
query take.  The rule is restated in tests/radarsc_np.py (parity with MulRan's own builder unpinned)."""
import ctypes as C

import numpy as np

from ._rsx import RADARSC_MAX, RADARSC_MEAN, RadarScParams, check, lib

STATS = {"mean": RADARSC_MEAN, "max": RADARSC_MAX}


def default_params():
    """resolution 0.0595 m, max_radius 80 m, min_range 58, power_floor 0, the mean."""
    p = RadarScParams()
    check(lib().rsx_radarsc_default_params(C.byref(p)))
    return p


class RadarContext:
    def __init__(self, rows=400, cols=3360, device=0, resolution=None, max_radius=None, min_range=None, power_floor=None, stat=None):
        """One handle per image shape and parameter set; stat: "mean" / "max" or the RADARSC_* value."""
        self._L = lib()
        self.rows, self.cols = rows, cols
        p = default_params()
        if resolution is not None:
            p.resolution = resolution
        if max_radius is not None:
            p.max_radius = max_radius
        if min_range is not None:
            p.min_range = min_range
        if power_floor is not None:
            p.power_floor = power_floor
        if stat is not None:
            p.stat = STATS.get(stat, stat)
        self.params = p
        self._h = C.c_void_p()
        check(self._L.rsx_radarsc_create(device, rows, cols, C.byref(p), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.rsx_radarsc_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def build_batch(self, imgs, azimuths, col_offset=11):
        """imgs: (n, rows, row_stride) uint8 (any image stride); azimuths: (rows,) shared or (n, rows) float32 rad.
        -> (n, 1200) float32 (rsx_radarsc_build_batch)."""
        imgs = np.asarray(imgs, dtype=np.uint8)
        if imgs.ndim == 2:
            imgs = imgs[None]
        if imgs.strides[1:] != (imgs.shape[2], 1):
            imgs = np.ascontiguousarray(imgs)
        assert imgs.shape[1] == self.rows
        az = np.ascontiguousarray(azimuths, dtype=np.float32)
        assert az.shape in ((self.rows,), (imgs.shape[0], self.rows))
        out = np.zeros((imgs.shape[0], 1200), dtype=np.float32)
        check(self._L.rsx_radarsc_build_batch(self._h, imgs.ctypes.data, imgs.shape[0], imgs.strides[0], imgs.shape[2], col_offset,
                                              az.ctypes.data, 1 if az.ndim == 2 else 0, out.ctypes.data))
        return out

    def build(self, img, azimuths, col_offset=11):
        """One image (rows, row_stride) -> (1200,) float32."""
        return self.build_batch(np.asarray(img)[None], azimuths, col_offset)[0]

    def build_batch_device(self, imgs_ptr, n, image_stride_bytes, row_stride, az_ptr, descs_ptr, col_offset=11, azimuths_per_image=False,
                           stream=0):
        """Device pointers in and out, asynchronous on `stream` (rsx_radarsc_build_batch_device): one launch."""
        check(self._L.rsx_radarsc_build_batch_device(self._h, imgs_ptr, n, image_stride_bytes, row_stride, col_offset, az_ptr,
                                                     1 if azimuths_per_image else 0, descs_ptr, stream))
