"""Host-side wrapper of the radar grid map entry points of librsx.so (include/rsx.h, rsx_gridmap_*): polar scans and their poses in, the
radar mosaic (mean power per world cell) and the hit counts out."""
import ctypes as C
import weakref

import numpy as np

from . import synth
from ._rsx import (GRIDMAP_HITS, GRIDMAP_MATCH_RESULT_DTYPE, GRIDMAP_MEAN, GRIDMAP_REFINE_RESULT_DTYPE, GRIDMAP_SEARCH_RESULT_DTYPE,
                   GRIDMAP_TRACK_RESULT_DTYPE, GridmapFieldParams, GridmapMatchParams, GridmapParams, GridmapRefineParams, GridmapSearchParams,
                   GridmapTrackParams, check, lib)
from .cfear import ragged


def _with_fields(p, struct, fields):
    for name, value in fields.items():
        if not hasattr(p, name):
            raise TypeError(struct + " has no field " + name)
        setattr(p, name, value)
    return p


def default_params():
    """1024 x 1024 cells of 0.5 m with the corner at (-256, -256), 0.0595 m per range bin, min_range_bins 58, range_halfwidth 4,
    hit_threshold 120, max_range 0 (to the last bin)."""
    p = GridmapParams()
    check(lib().rsx_gridmap_default_params(C.byref(p)))
    return p


def params(**fields):
    """default_params() with the given fields replaced."""
    return _with_fields(default_params(), "rsx_gridmap_params", fields)


def default_match_params():
    """rotations -8 .. 8 of 0.01 rad, shifts -8 .. 8 cells along x and y."""
    p = GridmapMatchParams()
    check(lib().rsx_gridmap_match_default_params(C.byref(p)))
    return p


def match_params(**fields):
    """default_match_params() with the given fields replaced."""
    return _with_fields(default_match_params(), "rsx_gridmap_match_params", fields)


def default_search_params():
    """rotations -32 .. 32 of 0.01 rad, shifts -64 .. 64 cells along x and y, no min_score."""
    p = GridmapSearchParams()
    check(lib().rsx_gridmap_search_default_params(C.byref(p)))
    return p


def search_params(**fields):
    """default_search_params() with the given fields replaced."""
    return _with_fields(default_search_params(), "rsx_gridmap_search_params", fields)


def search_blocks(p):
    """-> (2K + 1, nbv, nbu): the shape of a job's bounds under the parameters p"""
    return 2 * max(p.angle_steps, 0) + 1, (2 * max(p.y_cells, 0) + 8) // 8, (2 * max(p.x_cells, 0) + 8) // 8


def default_refine_params():
    """damping 1e-3, steps of at most 1 cell and 0.02 rad, tolerances 1e-3 cells and 1e-5 rad, at most 32 evaluations."""
    p = GridmapRefineParams()
    check(lib().rsx_gridmap_refine_default_params(C.byref(p)))
    return p


def refine_params(**fields):
    """default_refine_params() with the given fields replaced."""
    return _with_fields(default_refine_params(), "rsx_gridmap_refine_params", fields)


def default_field_params():
    """seeds at bytes >= 50, radius 12 cells: a prototype's values on the hits plane of the synthetic drive; no real radar data backs them."""
    p = GridmapFieldParams()
    check(lib().rsx_gridmap_field_default_params(C.byref(p)))
    return p


def field_params(**fields):
    """default_field_params() with the given fields replaced."""
    return _with_fields(default_field_params(), "rsx_gridmap_field_params", fields)


def default_track_params():
    """a window of rotations -2 .. 2 of 0.01 rad and shifts -2 .. 2 cells, the refinement's defaults, no min_score, predict 1."""
    p = GridmapTrackParams()
    check(lib().rsx_gridmap_track_default_params(C.byref(p)))
    return p


def track_params(**fields):
    """default_track_params() with the given fields replaced: min_score, predict, match or refine (whole structs), or a field of the
    match part (angle_steps, angle_step, x_cells, y_cells) or of the refine part (damping, ..., max_evaluations) by its own name"""
    p = default_track_params()
    for name, value in fields.items():
        part = next((q for q in (p.match, p.refine) if name != "reserved" and hasattr(q, name)), p)
        _with_fields(part, "rsx_gridmap_track_params", {name: value})
    return p


def gaussian_table(sigma, radius, peak=255):
    """uint8 [radius^2 + 1]: floor(peak exp(-q / (2 sigma^2)) + 0.5) at the squared distance q [cells^2], made on the host in fp64"""
    out = np.zeros(max(int(radius), 0) ** 2 + 1, dtype=np.uint8)
    check(lib().rsx_gridmap_field_gaussian_table(float(sigma), int(peak), int(radius), out.ctypes.data))
    return out


def prior_transforms(priors, n):
    """(n, 6) float64 from an (n, 6) array, or from the record array of match or search, whose `transform` is taken"""
    priors = np.asarray(priors)
    if priors.dtype.names and "transform" in priors.dtype.names:
        priors = priors["transform"]
    return np.ascontiguousarray(priors, dtype=np.float64).reshape(n, 6)


def _choose(params, fields, maker):
    """the params struct of a call that may give it whole or as fields by name"""
    if params is not None and fields:
        raise TypeError("give params or its fields, not both")
    return params if params is not None else maker(**fields)


def _jobs(clouds, priors, dtype, records=False):
    """-> xy, offsets, n, priors (n, 6) float64 and zeroed results (n,) of `dtype` for a host entry; records: priors may also be what
    prior_transforms takes"""
    xy, off = ragged(clouds, np.float32, 2)
    n = len(clouds)
    priors = prior_transforms(priors, n) if records else np.ascontiguousarray(priors, dtype=np.float64).reshape(n, 6)
    return xy, off, n, priors, np.zeros(n, dtype=dtype)


def _device_jobs(xy, offsets, priors, results, dtype):
    """the layout that a device entry asks of its tensors -> n; dtype: of a result record"""
    n = offsets.numel() - 1
    assert xy.dim() == 2 and xy.stride(1) == 1 and xy.element_size() == 4 and offsets.is_contiguous() and priors.is_contiguous()
    assert priors.numel() == 6 * n and results.is_contiguous() and results.numel() * results.element_size() == n * dtype.itemsize
    return n


def write_pgm(path, px):
    """uint8 [h, w] -> binary PGM (P5), row 0 first"""
    px = np.ascontiguousarray(px, dtype=np.uint8)
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (px.shape[1], px.shape[0]))
        f.write(px.tobytes())


def load_pgm(path):
    """a binary PGM (P5, maxval 255; comments allowed in the header) -> uint8 [h, w]: the inverse of save_pgm for the mean, so that
    set_likelihood(load_pgm(f)) localises in a mosaic saved earlier"""
    with open(path, "rb") as f:
        data = f.read()
    fields, at = [], 0
    while len(fields) < 4:
        while at < len(data) and data[at:at + 1].isspace():
            at += 1
        if data[at:at + 1] == b"#":
            at = data.index(b"\n", at) + 1
            continue
        end = at
        while end < len(data) and not data[end:end + 1].isspace():
            end += 1
        if end == at:
            raise ValueError(path + ": truncated PGM header")
        fields.append(data[at:end])
        at = end
    if fields[0] != b"P5" or int(fields[3]) != 255:
        raise ValueError(path + ": not a binary PGM with maxval 255")
    w, h = int(fields[1]), int(fields[2])
    if len(data) < at + 1 + w * h:
        raise ValueError(path + ": truncated PGM")
    return np.frombuffer(data, dtype=np.uint8, count=w * h, offset=at + 1).reshape(h, w).copy()


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
            for t in list(getattr(self, "_trackers", ())):   # (a tracker reads this map: it goes first)
                t.close()
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
        write_pgm(path, px)

    # ---- localising clouds in the map: the likelihood plane and the correlative matching (include/rsx.h, rsx_gridmap_match_*) ----

    def update_likelihood(self, mode=GRIDMAP_MEAN, min_observations=1, stream=None):
        """the likelihood plane (a frozen uint8 snapshot that matching reads) from the planes as they stand: the mean, or the hit
        percentage with unknown as 0.  Asynchronous on `stream`"""
        check(self._L.rsx_gridmap_likelihood_update(self._h, mode, min_observations, stream))

    def set_likelihood(self, img):
        """the likelihood plane from a uint8 [height, width] image (load_pgm of a saved mosaic, for one)"""
        img = np.ascontiguousarray(img, dtype=np.uint8)
        assert img.shape == (self.params.height, self.params.width)
        check(self._L.rsx_gridmap_likelihood_set(self._h, img.ctypes.data))

    def likelihood(self, window=None):
        """window: (x, y, w, h) in cells, None = the whole map -> uint8 [h, w]"""
        x, y, w, h = self._window(window)
        out = np.zeros((max(h, 0), max(w, 0)), dtype=np.uint8)
        check(self._L.rsx_gridmap_likelihood_read(self._h, x, y, w, h, out.ctypes.data))
        return out

    def likelihood_device(self):
        """-> (address of cell (0, 0) of the likelihood plane in device memory, pitch_bytes)"""
        d, pitch = C.c_void_p(), C.c_int64()
        check(self._L.rsx_gridmap_likelihood_device(self._h, C.byref(d), C.byref(pitch)))
        return d.value, pitch.value

    def likelihood_field(self, table=None, sigma=3.0, peak=255, params=None, stream=None, **fields):
        """turn the likelihood plane, in place, into a likelihood field (include/rsx.h, rsx_gridmap_likelihood_field): the cells at or
        above `threshold` are seeds, a cell within `radius` cells of a seed gets table[q] at the squared distance q to the nearest one,
        every other cell 0.  table: uint8 [radius^2 + 1], None = gaussian_table(sigma, radius, peak); params: a GridmapFieldParams, or
        its fields by name (threshold, radius).  Asynchronous on `stream`; a search in the field needs a prepare_search after it"""
        p = _choose(params, fields, field_params)
        if table is None and (float(sigma), int(peak)) != (3.0, 255):
            table = gaussian_table(sigma, p.radius, peak)
        if table is not None:
            table = np.ascontiguousarray(table, dtype=np.uint8)
            assert table.shape == (p.radius * p.radius + 1,)
        check(self._L.rsx_gridmap_likelihood_field(self._h, C.byref(p), table.ctypes.data if table is not None else None, stream))

    def match(self, clouds, priors, return_scores=False, params=None, **fields):
        """clouds: list of (n_i, 2) float32 in the sensor frame; priors: (n, 6) float64 r00, r01, tx, r10, r11, ty (coral.pose_matrices
        makes them from x, y, yaw); params: a GridmapMatchParams, or its fields by name (angle_steps, angle_step, x_cells, y_cells)
        -> results (n,) GRIDMAP_MATCH_RESULT_DTYPE, and with return_scores=True also the volumes uint32 [n, 2K + 1, 2V + 1, 2U + 1]"""
        p = _choose(params, fields, match_params)
        xy, off, n, priors, res = _jobs(clouds, priors, GRIDMAP_MATCH_RESULT_DTYPE)
        vol = np.zeros((n, 2 * max(p.angle_steps, 0) + 1, 2 * max(p.y_cells, 0) + 1, 2 * max(p.x_cells, 0) + 1), dtype=np.uint32) if return_scores else None
        check(self._L.rsx_gridmap_match_batch(self._h, xy.ctypes.data, off.ctypes.data, n, priors.ctypes.data, C.byref(p), res.ctypes.data,
                                              vol.ctypes.data if return_scores else None))
        return (res, vol) if return_scores else res

    def match_device(self, xy, offsets, priors, results, scores=None, params=None, stream=None, **fields):
        """the same on torch tensors of the handle's device: xy float32 [m, point_stride] (rows point_stride floats apart, x and y
        first), offsets int64 (n + 1,), priors float64 (n, 6) contiguous, results uint8 of n * 88 bytes (view it as
        GRIDMAP_MATCH_RESULT_DTYPE on the host), scores (optional) uint32 / int32 of n (2K + 1)(2V + 1)(2U + 1) elements.  Asynchronous on
        `stream` (an int, None = the handle's own stream); a job above the cap gets GRIDMAP_MATCH_STATUS_POINTS"""
        p = _choose(params, fields, match_params)
        n = _device_jobs(xy, offsets, priors, results, GRIDMAP_MATCH_RESULT_DTYPE)
        if scores is not None:
            assert scores.is_contiguous() and scores.element_size() == 4
            assert scores.numel() == n * (2 * p.angle_steps + 1) * (2 * p.y_cells + 1) * (2 * p.x_cells + 1)
        check(self._L.rsx_gridmap_match_batch_device(self._h, xy.data_ptr(), offsets.data_ptr(), xy.stride(0), n, priors.data_ptr(), C.byref(p),
                                                     results.data_ptr(), scores.data_ptr() if scores is not None else None, stream))

    def score(self, clouds, poses):
        """how well clouds fit the map at poses (n, 6): match with no window (K = U = V = 0) -> results; `score` is the sum of the
        likelihood bytes under the cloud, n_inside the points it was taken over"""
        return self.match(clouds, poses, angle_steps=0, x_cells=0, y_cells=0)

    # ---- the same over a wide window, pruned by bounds (include/rsx.h, rsx_gridmap_search_*) ----

    def prepare_search(self, max_cells=64, stream=None):
        """snapshot the likelihood plane as it stands for searches with x_cells, y_cells <= max_cells (0 .. 256): a framed copy and the
        8 x 8 pooled plane.  Later likelihood changes are not seen until the next prepare_search.  Asynchronous on `stream`"""
        check(self._L.rsx_gridmap_search_prepare(self._h, max_cells, stream))

    def search(self, clouds, priors, return_bounds=False, params=None, **fields):
        """match over a window of up to 180 rotations and 256 cells either way, with the same winner as the exhaustive rule; clouds
        and priors as for match; params: a GridmapSearchParams, or its fields by name (angle_steps, angle_step, x_cells, y_cells,
        min_score) -> results (n,) GRIDMAP_SEARCH_RESULT_DTYPE, and with return_bounds=True also the bounds uint32 [n, 2K + 1, nbv, nbu]"""
        p = _choose(params, fields, search_params)
        xy, off, n, priors, res = _jobs(clouds, priors, GRIDMAP_SEARCH_RESULT_DTYPE)
        bounds = np.zeros((n,) + search_blocks(p), dtype=np.uint32) if return_bounds else None
        check(self._L.rsx_gridmap_search_batch(self._h, xy.ctypes.data, off.ctypes.data, n, priors.ctypes.data, C.byref(p), res.ctypes.data,
                                               bounds.ctypes.data if return_bounds else None))
        return (res, bounds) if return_bounds else res

    def search_device(self, xy, offsets, priors, results, bounds=None, params=None, stream=None, **fields):
        """the same on torch tensors of the handle's device, as match_device: results uint8 of n * 96 bytes (view it as
        GRIDMAP_SEARCH_RESULT_DTYPE on the host), bounds (optional) uint32 / int32 of n (2K + 1) nbv nbu elements.  Asynchronous on
        `stream`; a job above the cap gets GRIDMAP_MATCH_STATUS_POINTS"""
        p = _choose(params, fields, search_params)
        n = _device_jobs(xy, offsets, priors, results, GRIDMAP_SEARCH_RESULT_DTYPE)
        if bounds is not None:
            nk, nbv, nbu = search_blocks(p)
            assert bounds.is_contiguous() and bounds.element_size() == 4 and bounds.numel() == n * nk * nbv * nbu
        check(self._L.rsx_gridmap_search_batch_device(self._h, xy.data_ptr(), offsets.data_ptr(), xy.stride(0), n, priors.data_ptr(), C.byref(p),
                                                      results.data_ptr(), bounds.data_ptr() if bounds is not None else None, stream))

    # ---- the pose below the cell: Levenberg-Marquardt on the interpolated likelihood plane (include/rsx.h, rsx_gridmap_refine_*) ----

    def refine(self, clouds, priors, params=None, **fields):
        """clouds as for match; priors: (n, 6) float64, or the records that match or search returned (their `transform` is taken, so
        gm.refine(clouds, gm.match(clouds, priors)) is the whole chain); params: a GridmapRefineParams, or its fields by name (damping,
        max_shift_step, max_rotation_step, shift_tolerance, rotation_tolerance, max_evaluations)
        -> results (n,) GRIDMAP_REFINE_RESULT_DTYPE: the refined transform, the Hessian at it, cost and score before and after"""
        p = _choose(params, fields, refine_params)
        xy, off, n, priors, res = _jobs(clouds, priors, GRIDMAP_REFINE_RESULT_DTYPE, records=True)
        check(self._L.rsx_gridmap_refine_batch(self._h, xy.ctypes.data, off.ctypes.data, n, priors.ctypes.data, C.byref(p), res.ctypes.data))
        return res

    def refine_device(self, xy, offsets, priors, results, params=None, stream=None, **fields):
        """the same on torch tensors of the handle's device, as match_device: priors float64 (n, 6) contiguous, results uint8 of
        n * 152 bytes (view it as GRIDMAP_REFINE_RESULT_DTYPE on the host).  One launch, asynchronous on `stream`; a job above the cap
        gets GRIDMAP_MATCH_STATUS_POINTS"""
        p = _choose(params, fields, refine_params)
        n = _device_jobs(xy, offsets, priors, results, GRIDMAP_REFINE_RESULT_DTYPE)
        check(self._L.rsx_gridmap_refine_batch_device(self._h, xy.data_ptr(), offsets.data_ptr(), xy.stride(0), n, priors.data_ptr(), C.byref(p),
                                                      results.data_ptr(), stream))

    # ---- following a sensor through the map: match, refine and compose in one launch per push (include/rsx.h, rsx_gridmap_tracker_*) ----

    def tracker(self, n_sequences):
        """a GridTracker of n_sequences sequences in this map, every one at the identity pose; the map must stay open while it is used"""
        return GridTracker(self, n_sequences)


class GridTracker:
    """n_sequences sensors followed through one GridMap scan after scan (include/rsx.h, rsx_gridmap_tracker_*): per scan a match on the grid
    around a constant-velocity prediction, the refinement below the cell, and the composed motion; the state stays on the device"""

    def __init__(self, gridmap, n_sequences):
        self._L = lib()
        self._h = C.c_void_p()
        self.map = gridmap          # (kept alive: the tracker reads its plane)
        self.n_sequences = int(n_sequences)
        check(self._L.rsx_gridmap_tracker_create(gridmap.handle, self.n_sequences, C.byref(self._h)))
        if not hasattr(gridmap, "_trackers"):
            gridmap._trackers = weakref.WeakSet()
        gridmap._trackers.add(self)   # (GridMap.close closes its trackers first)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.rsx_gridmap_tracker_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def reset(self, poses):
        """poses: (n_sequences, 6) float64 r00, r01, tx, r10, r11, ty -> every sequence starts again at its pose (no motion, no scan seen)"""
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(self.n_sequences, 6)
        check(self._L.rsx_gridmap_tracker_reset(self._h, poses.ctypes.data))

    def set_pose(self, q, pose):
        """sequence q starts again at pose (6,): what follows a search after a lost scan"""
        pose = np.ascontiguousarray(pose, dtype=np.float64).reshape(6)
        check(self._L.rsx_gridmap_tracker_set_pose(self._h, int(q), pose.ctypes.data))

    def state(self):
        """-> poses (n_sequences, 6) float64, motions (n_sequences, 6) float64, counts (n_sequences,) int32"""
        poses, motions = np.zeros((self.n_sequences, 6)), np.zeros((self.n_sequences, 6))
        counts = np.zeros(self.n_sequences, dtype=np.int32)
        check(self._L.rsx_gridmap_tracker_state(self._h, poses.ctypes.data, motions.ctypes.data, counts.ctypes.data))
        return poses, motions, counts

    def push(self, clouds_per_sequence, params=None, **fields):
        """clouds_per_sequence: for every sequence the list of its next scans, each (n_i, 2) float32 in the sensor frame (an empty list: no
        scan for that sequence in this push); params: a GridmapTrackParams, or what track_params takes
        -> records (total scans,) GRIDMAP_TRACK_RESULT_DTYPE, sequence after sequence in the order given"""
        assert len(clouds_per_sequence) == self.n_sequences
        p = _choose(params, fields, track_params)
        clouds = [c for seq in clouds_per_sequence for c in seq]
        xy, off = ragged(clouds, np.float32, 2)
        n_scans = np.array([len(seq) for seq in clouds_per_sequence], dtype=np.int32)
        res = np.zeros(len(clouds), dtype=GRIDMAP_TRACK_RESULT_DTYPE)
        check(self._L.rsx_gridmap_tracker_push(self._h, xy.ctypes.data, off.ctypes.data, n_scans.ctypes.data, C.byref(p), res.ctypes.data))
        return res

    def push_device(self, xy, offsets, n_scans, results, params=None, stream=None, **fields):
        """the same on torch tensors of the map's device: xy float32 [m, point_stride], offsets int64 (total scans + 1,), n_scans int32
        (n_sequences,), results uint8 of total scans * 344 bytes (view it as GRIDMAP_TRACK_RESULT_DTYPE on the host).  One launch,
        asynchronous on `stream` (an int, None = the map's own stream); a scan above the cap is lost with GRIDMAP_MATCH_STATUS_POINTS"""
        p = _choose(params, fields, track_params)
        total = offsets.numel() - 1
        assert xy.dim() == 2 and xy.stride(1) == 1 and xy.element_size() == 4 and offsets.is_contiguous() and offsets.element_size() == 8
        assert n_scans.is_contiguous() and n_scans.element_size() == 4 and n_scans.numel() == self.n_sequences
        assert results.is_contiguous() and results.numel() * results.element_size() == total * GRIDMAP_TRACK_RESULT_DTYPE.itemsize
        check(self._L.rsx_gridmap_tracker_push_device(self._h, xy.data_ptr(), offsets.data_ptr(), xy.stride(0), n_scans.data_ptr(), total, C.byref(p),
                                                      results.data_ptr(), stream))
