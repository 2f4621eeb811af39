"""Host-side wrapper of the file-based odometry pipeline of librsx.so (include/rsx.h: rsx_odometry_*): windows of
consecutive polar scans in, one relative motion per scan out.  Test / bench harness; the product entry is host/odometry.cpp."""
import ctypes as C

import numpy as np

from ._rsx import (MOCOMP_DESKEW, MOCOMP_DOPPLER, ODOMETRY_PHASECORR_ESTIMATE, ODOMETRY_PHASECORR_FALLBACK, ORORA_PMC, ORORA_PMC_EXACT, ODOMETRY_SCAN_DTYPE, Cen2018Params,
                   CfarParams, CfearParams, CfearTrackParams, KStrongestParams, MocompParams, OdometryParams, OdometryPhasecorrParams, PhasecorrParams, RansacParams, check,
                   lib)

ESTIMATORS = {"orora": 0, "ransac": 1, "mcransac": 2}  # RSX_ESTIMATOR_* ("cfear" and "phasecorr", RSX_ESTIMATOR_CFEAR and _PHASECORR, have setters of their own)
COMPENSATIONS = {"motion": MOCOMP_DESKEW, "doppler": MOCOMP_DOPPLER, "both": MOCOMP_DESKEW | MOCOMP_DOPPLER}  # rsx_mocomp_params.flags


def default_params():
    p = OdometryParams()
    check(lib().rsx_odometry_default_params(C.byref(p)))
    return p


def default_phasecorr_params():
    """rsx_phasecorr_default_params in .pc, both gates 0 (off), mode ESTIMATE; needs no device"""
    p = OdometryPhasecorrParams()
    check(lib().rsx_odometry_default_phasecorr_params(C.byref(p)))
    return p


def phasecorr_params(fields=None, mode=None):
    """fields: None (the defaults), an OdometryPhasecorrParams (copied) or a dict: max_peak_ratio, min_peak and mode by name, any other
    name a field of rsx_phasecorr_params (n, resolution, min_range_bins, max_rotation, resolve_half_turn).  mode, when given, wins."""
    p = default_phasecorr_params()
    if isinstance(fields, OdometryPhasecorrParams):
        C.memmove(C.byref(p), C.byref(fields), C.sizeof(p))
    elif fields is not None:
        own = [name for name, _ in OdometryPhasecorrParams._fields_ if name != "pc"]
        inner = [name for name, _ in PhasecorrParams._fields_]
        for name, value in dict(fields).items():
            if name in own:
                setattr(p, name, value)
            elif name in inner:
                setattr(p.pc, name, value)
            else:
                raise TypeError("rsx_odometry_phasecorr_params has no field " + name)
    if mode is not None:
        p.mode = mode
    return p


class Odometry:
    """keypoints: "cen2019" (default), "cen2018", "kstrongest" or "cfar"; cen2018: its Cen2018Params (None: cen2018.default_params());
    kstrongest: its KStrongestParams (None: kstrongest.default_params()); cfar: its CfarParams (None: cfar.default_params()).
    estimator: "orora" (default), "ransac", "mcransac" or "cfear"; ransac: the RANSAC estimators' RansacParams (None:
    ransac.default_params()); cfear: CfearParams (None: cfear.default_params()): CFEAR's surface points and point-to-line
    registration in place of descriptors, matcher and estimator (rsx_odometry_set_cfear; pair it with keypoints="kstrongest",
    min_separation = 0; not with compensate).  cfear_track: True (the defaults) or a CfearTrackParams: CFEAR's keyframe tracker --
    joint registration against the last keyframes from a constant-velocity prediction -- in place of the registration of
    consecutive pairs (rsx_odometry_set_cfear_tracking; only with estimator="cfear").  cfear_compensate: True switches on the
    tracker's motion compensation (CfearTrackParams.compensate = 1: surface points with times, every scan registered twice; the
    published cloud stays as measured); it implies cfear_track.
    exact_clique: the max-clique inlier selection returns a maximum clique (params.orora.flags |= ORORA_PMC_EXACT).
    compensate: None (default), "motion", "doppler" or "both": every pair is estimated, its matches compensated with that
    estimate, and estimated again (rsx_odometry_set_compensation; not with "mcransac"); beta, dt_scan: the Doppler factor and
    the scan period of the model (None: the library's defaults).
    estimator="phasecorr": phase correlation of the power images in place of descriptors, matcher and estimator
    (rsx_odometry_set_phasecorr, mode ESTIMATE; the keypoint extractor still runs); fallback="phasecorr": beside any other estimator,
    for exactly the pairs it failed on (mode FALLBACK); not both.  phasecorr: an OdometryPhasecorrParams, a dict of fields (see
    phasecorr_params) or None for the defaults; not with compensate or the CFEAR tracker.  A record of phase correlation has
    iterations = -1 - half_turn, rot_inliers = rint(peak * 1e6), trans_inliers = rint(peak_ratio * 1e6), status 0 or 16 | 1 | 2."""

    def __init__(self, rows=400, cols=3360, params=None, device=0, keypoints="cen2019", cen2018=None, estimator="orora", ransac=None,
                 exact_clique=False, compensate=None, beta=None, dt_scan=None, kstrongest=None, cfear=None, cfear_track=None,
                 cfear_compensate=False, cfar=None, phasecorr=None, fallback=None):
        if keypoints not in ("cen2019", "cen2018", "kstrongest", "cfar"):
            raise ValueError("keypoints must be cen2019, cen2018, kstrongest or cfar")
        if estimator not in ESTIMATORS and estimator not in ("cfear", "phasecorr"):
            raise ValueError("estimator must be orora, ransac, mcransac, cfear or phasecorr")
        if fallback not in (None, "phasecorr"):
            raise ValueError("fallback must be None or phasecorr")
        if estimator == "phasecorr" and fallback == "phasecorr":
            raise ValueError("phasecorr is the estimator or the fallback, not both")
        if phasecorr is not None and estimator != "phasecorr" and fallback is None:
            raise ValueError("phasecorr parameters need estimator=\"phasecorr\" or fallback=\"phasecorr\"")
        if compensate is not None and compensate not in COMPENSATIONS:
            raise ValueError("compensate must be None, motion, doppler or both")
        self._L = lib()
        self.rows, self.cols = rows, cols
        self.params = params if params is not None else default_params()
        self.params.device = device
        if exact_clique:
            if not self.params.orora.flags & ORORA_PMC:
                raise ValueError("exact_clique needs the max-clique selection (ORORA_PMC) on")
            self.params.orora.flags |= ORORA_PMC_EXACT
        self._h = C.c_void_p()
        check(self._L.rsx_odometry_create(C.byref(self.params), rows, cols, C.byref(self._h)))
        if keypoints == "cen2018":
            self.set_cen2018(cen2018)
        if keypoints == "kstrongest":
            self.set_kstrongest(kstrongest)
        if keypoints == "cfar":
            self.set_cfar(cfar)
        if cfear_compensate and estimator != "cfear":
            raise ValueError("cfear_compensate needs estimator=\"cfear\"")
        if estimator == "cfear":
            self.set_cfear(cfear)
            if cfear_compensate:
                track = CfearTrackParams()
                if cfear_track is None or cfear_track is True or cfear_track is False:
                    check(self._L.rsx_cfear_default_track_params(C.byref(track)))
                else:
                    C.memmove(C.byref(track), C.byref(cfear_track), C.sizeof(track))
                track.compensate = 1
                cfear_track = track
            if cfear_track is not None and cfear_track is not False:
                self.set_cfear_tracking(None if cfear_track is True else cfear_track)
        elif estimator == "phasecorr":
            self.set_phasecorr(phasecorr_params(phasecorr, mode=ODOMETRY_PHASECORR_ESTIMATE))
        elif estimator != "orora":
            self.set_estimator(estimator, ransac)
        if fallback == "phasecorr":
            self.set_phasecorr(phasecorr_params(phasecorr, mode=ODOMETRY_PHASECORR_FALLBACK))
        if compensate is not None:
            self.set_compensation(compensate, beta=beta, dt_scan=dt_scan)

    def set_compensation(self, compensate, beta=None, dt_scan=None):
        """Switch the compensation of keypoints on ("motion", "doppler", "both", or a MocompParams) or off (None).  Only while the
        handle holds no scan, and not with the "mcransac" estimator."""
        if compensate is None:
            check(self._L.rsx_odometry_set_compensation(self._h, None))
            return
        p = compensate
        if not isinstance(p, MocompParams):
            p = MocompParams()
            check(self._L.rsx_mocomp_default_params(C.byref(p)))
            p.flags = COMPENSATIONS[compensate]
            if beta is not None:
                p.beta = beta
            if dt_scan is not None:
                p.dt_scan = dt_scan
        check(self._L.rsx_odometry_set_compensation(self._h, C.byref(p)))

    def set_estimator(self, estimator, ransac=None):
        """Switch the motion estimator (ransac: RansacParams or None for the defaults).  Only while the handle holds no scan."""
        if ransac is not None and not isinstance(ransac, RansacParams):
            raise TypeError("ransac must be RansacParams")
        check(self._L.rsx_odometry_set_estimator(self._h, ESTIMATORS[estimator], C.byref(ransac) if ransac is not None else None))

    def _set(self, setter, default_params, params_type, params, off):
        """One extractor / CFEAR setter of the library: off -> its NULL form; params None -> the library's defaults."""
        if off:
            check(setter(self._h, None))
            return
        p = params
        if p is None:
            p = params_type()
            check(default_params(C.byref(p)))
        check(setter(self._h, C.byref(p)))

    def set_cfear(self, cfear=None, off=False):
        """Switch to CFEAR surface points and point-to-line registration (cfear: CfearParams or None for the defaults), or back to
        ORORA with off=True.  Only while the handle holds no scan, and not while compensation is on."""
        self._set(self._L.rsx_odometry_set_cfear, self._L.rsx_cfear_default_params, CfearParams, cfear, off)

    def set_cfear_tracking(self, track=None, off=False):
        """Switch CFEAR to its keyframe tracker (track: CfearTrackParams or None for the defaults), or back to consecutive pairs with
        off=True.  Only while CFEAR is selected and the handle holds no scan."""
        self._set(self._L.rsx_odometry_set_cfear_tracking, self._L.rsx_cfear_default_track_params, CfearTrackParams, track, off)

    def set_phasecorr(self, params=None, off=False):
        """Switch phase correlation on (params: an OdometryPhasecorrParams whose mode picks ESTIMATE or FALLBACK, a dict of fields, or None
        for the defaults: ESTIMATE at N = 256), or off with off=True (the selected estimator alone again).  Only while the handle holds no scan, and not
        while compensation or the CFEAR tracker is on."""
        if params is not None and not isinstance(params, OdometryPhasecorrParams):
            params = phasecorr_params(params)
        self._set(self._L.rsx_odometry_set_phasecorr, self._L.rsx_odometry_default_phasecorr_params, OdometryPhasecorrParams, params, off)

    def set_cen2018(self, cen2018=None, off=False):
        """Switch to cen2018 keypoints (cen2018: Cen2018Params or None for the defaults), or back to cen2019 with off=True.
        Only while the handle holds no scan (fresh, or after reset())."""
        self._set(self._L.rsx_odometry_set_cen2018, self._L.rsx_cen2018_default_params, Cen2018Params, cen2018, off)

    def set_kstrongest(self, kstrongest=None, off=False):
        """Switch to k-strongest keypoints (kstrongest: KStrongestParams or None for the defaults) in place of whichever extractor
        was selected, or back to cen2019 with off=True.  Only while the handle holds no scan (fresh, or after reset())."""
        self._set(self._L.rsx_odometry_set_kstrongest, self._L.rsx_kstrongest_default_params, KStrongestParams, kstrongest, off)

    def set_cfar(self, cfar=None, off=False):
        """Switch to CA-CFAR / BFAR keypoints (cfar: CfarParams or None for the defaults) in place of whichever extractor was
        selected, or back to cen2019 with off=True.  Only while the handle holds no scan (fresh, or after reset())."""
        self._set(self._L.rsx_odometry_set_cfar, self._L.rsx_cfar_default_params, CfarParams, cfar, off)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.rsx_odometry_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        check(self._L.rsx_odometry_reset(self._h))

    def push(self, imgs, azimuths, want_xy=False, max_xy=None, device_ptr=None):
        """imgs: (n, rows, row_stride) uint8 host array (or, with device_ptr, only its shape / strides are used and the
        bytes are read from that HBM address).  -> structured array (n,) of ODOMETRY_SCAN_DTYPE [, list of xy (k_i, 2)]."""
        n, rows, row_stride = imgs.shape
        assert rows == self.rows
        az = np.ascontiguousarray(azimuths, dtype=np.float32)
        out = np.zeros(n, dtype=ODOMETRY_SCAN_DTYPE)
        mx = (max_xy or self.params.max_keypoints) if want_xy else 0
        xy = np.zeros((n, mx, 2), dtype=np.float32) if want_xy else None
        if device_ptr is None:
            imgs = np.ascontiguousarray(imgs, dtype=np.uint8)
            fn, src = self._L.rsx_odometry_push, imgs.ctypes.data
        else:
            fn, src = self._L.rsx_odometry_push_device, device_ptr
        check(fn(self._h, src, n, imgs.strides[0], row_stride, az.ctypes.data, 1 if az.ndim == 2 else 0, out.ctypes.data,
                 xy.ctypes.data if xy is not None else None, mx))
        if want_xy:
            k = np.minimum(np.minimum(out["n_keypoints"], self.params.max_keypoints), mx)
            return out, [xy[i, :k[i]].copy() for i in range(n)]
        return out
