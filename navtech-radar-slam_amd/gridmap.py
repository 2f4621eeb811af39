"""Host-side wrapper of the radar grid map entry points of librsx.so (include/rsx.h, rsx_gridmap_*): polar scans and their poses in, the
radar mosaic (mean power per world cell) and the hit counts out."""
import ctypes as C

import numpy as np

from . import synth
from ._rsx import GRIDMAP_HITS, GRIDMAP_MEAN, GridmapParams, check, lib


def default_params():
    """1024 x 1024 cells of 0.5 m with the corner at (-256, -256), 0.0595 m per range bin, min_range_bins 58, range_halfwidth 4,
    hit_threshold 120, max_range 0 (to the last bin)."""
    p = GridmapParams()
    check(lib().rsx_gridmap_default_params(C.byref(p)))
    return p


def params(**fields):
    """default_params() with the given fields replaced."""
    p = default_params()
    for name, value in fields.items():
        if not hasattr(p, name):
            raise TypeError("rsx_gridmap_params has no field " + name)
        setattr(p, name, value)
    return p


class GridMap:
    """one handle per image shape and parameter set; it owns the three planes"""

    def __init__(self, rows, cols, params=None, device=0):
        self._L = lib()
        self._h = C.c_void_p()
        self.rows, self.cols = rows, cols
        self.params = params if params is not None else default_params()
        check(self._L.rsx_gridmap_create(device, rows, cols, C.byref(self.params), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.rsx_gridmap_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def add(self, imgs, transforms, col_offset=synth.OXFORD_META):
        """imgs: [n, rows, row_stride] uint8 (power samples at [col_offset, col_offset + cols) of a row); transforms: (n, 6) float64
        r00, r01, tx, r10, r11, ty taking the sensor frame into the map frame (coral.pose_matrices makes them from x, y, yaw)"""
        imgs = np.ascontiguousarray(imgs, dtype=np.uint8)
        assert imgs.ndim == 3 and imgs.shape[1] == self.rows
        transforms = np.ascontiguousarray(transforms, dtype=np.float64).reshape(len(imgs), 6)
        check(self._L.rsx_gridmap_add_batch(self._h, imgs.ctypes.data, len(imgs), imgs.strides[0], imgs.strides[1], col_offset,
                                            transforms.ctypes.data))

    def add_device(self, imgs, transforms, col_offset=synth.OXFORD_META, status=None, stream=None):
        """the same on torch tensors of the handle's device: imgs uint8 [n, rows, row_stride] (any strides with a unit last one),
        transforms float64 (n, 6) contiguous, status (optional) int32 (n,): 0, or GRIDMAP_STATUS_TRANSFORM for a skipped scan.
        Asynchronous on `stream` (an int, None = the handle's own stream)"""
        assert imgs.dim() == 3 and imgs.shape[1] == self.rows and imgs.stride(2) == 1 and transforms.is_contiguous()
        assert transforms.numel() == 6 * imgs.shape[0]
        check(self._L.rsx_gridmap_add_batch_device(self._h, imgs.data_ptr(), imgs.shape[0], imgs.stride(0), imgs.stride(1), col_offset,
                                                   transforms.data_ptr(), status.data_ptr() if status is not None else None, stream))

    def clear(self, stream=None):
        check(self._L.rsx_gridmap_clear(self._h, stream))

    def _window(self, window):
        return (0, 0, self.params.width, self.params.height) if window is None else tuple(int(v) for v in window)

    def read(self, window=None):
        """window: (x, y, w, h) in cells, None = the whole map -> (sum, cnt, hit), uint32 [h, w] each"""
        x, y, w, h = self._window(window)
        out = [np.zeros((max(h, 0), max(w, 0)), dtype=np.uint32) for _ in range(3)]
        check(self._L.rsx_gridmap_read(self._h, x, y, w, h, *(o.ctypes.data for o in out)))
        return tuple(out)

    def _render(self, mode, min_observations, window, dtype):
        x, y, w, h = self._window(window)
        out = np.zeros((max(h, 0), max(w, 0)), dtype=dtype)
        check(self._L.rsx_gridmap_render(self._h, mode, min_observations, x, y, w, h, out.ctypes.data))
        return out

    def mean(self, min_observations=1, window=None):
        """uint8 [h, w]: the mean sample of a cell, rounded; 0 where it was observed fewer than min_observations times"""
        return self._render(GRIDMAP_MEAN, min_observations, window, np.uint8)

    def hits(self, min_observations=1, window=None):
        """int8 [h, w], nav_msgs/OccupancyGrid: -1 unknown, else the percentage of the observations that were hits"""
        return self._render(GRIDMAP_HITS, min_observations, window, np.int8)

    def render_device(self, mode, out, min_observations=1, window=None, stream=None):
        """out: a torch uint8 / int8 tensor of h * w elements on the handle's device"""
        x, y, w, h = self._window(window)
        assert out.is_contiguous() and out.numel() == w * h and out.element_size() == 1
        check(self._L.rsx_gridmap_render_device(self._h, mode, min_observations, x, y, w, h, out.data_ptr(), stream))

    def planes_device(self):
        """-> (d_sum, d_cnt, d_hit, pitch_bytes): device addresses of the planes"""
        p = [C.c_void_p() for _ in range(3)]
        pitch = C.c_int64()
        check(self._L.rsx_gridmap_planes_device(self._h, C.byref(p[0]), C.byref(p[1]), C.byref(p[2]), C.byref(pitch)))
        return p[0].value, p[1].value, p[2].value, pitch.value

    def save_pgm(self, path, mode=GRIDMAP_MEAN, min_observations=1):
        """binary PGM (P5), row 0 = y 0: the mean as is; the hits as 255 for unknown and 254 - 2 value otherwise (what host/odometry
        --grid-map / --grid-hits write)"""
        if mode == GRIDMAP_MEAN:
            px = self.mean(min_observations)
        else:
            h = self.hits(min_observations).astype(np.int16)
            px = np.where(h < 0, 255, 254 - 2 * h).astype(np.uint8)
        with open(path, "wb") as f:
            f.write(b"P5\n%d %d\n255\n" % (px.shape[1], px.shape[0]))
            f.write(px.tobytes())
