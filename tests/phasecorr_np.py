"""numpy restatement of the rsx_phasecorr entries (include/rsx.h, csrc/phasecorr.hip): the arithmetic contract of the phase-correlation
(Fourier-Mellin at scale 1) registration of two polar scans.  PARITY UNPINNED: the reference has no such code.

What is bit-exact and what is not:
  * the tables (resampling map, Hann window, the table of cos / sin) are fp64 on the host, rounded ONCE to fp32: bit-exact
  * the windowed Cartesian image is fp32 in the operation order of cart_image(): bit-exact
  * everything behind it (FFTs, cross-powers, surfaces) is fp32 on the device in a fixed order and fp64 here: compared within the
    bound tests/test_gpu_phasecorr.py states; the integer peak positions, half_turn and status are equal

Frames (synth.polar_sequence, rsx_cfear_result): azimuth 0 is +x (forward), a return at azimuth phi and range rho sits at
(rho cos phi, rho sin phi); image column j is x = (j - N/2) resolution, image row i is y = (i - N/2) resolution.  The result of a pair
(src, dst) is (x, y, theta) with p_dst = R(theta) p_src + (x, y): synth.relative_pose(dst_pose, src_pose).  So a scan whose rows were
rolled by +k (every return k rows further round) registers against the unrolled one with theta = -k 2 pi / rows."""
import math

import numpy as np

SIZES = (64, 128, 256, 512)
R_MIN = 4          # innermost radius of the polar-resampled magnitude spectrum
EPS = 1e-9         # C / (|C| + EPS max|C|)
STATUS_ROTATION = 1
F32 = np.float32


def default_params():
    return dict(n=256, resolution=0.5, range_resolution=0.0595, min_range_bins=58, resolve_half_turn=1, max_rotation=0.0)


def check_params(p, rows, cols):
    """the rules of rsx_phasecorr_params; -> None or the word of the violated rule"""
    if p["n"] not in SIZES:
        return "n"
    if not (p["resolution"] > 0.0 and math.isfinite(p["resolution"])):
        return "resolution"
    if not (p["range_resolution"] > 0.0 and math.isfinite(p["range_resolution"])):
        return "range_resolution"
    if p["min_range_bins"] < 0:
        return "min_range_bins"
    if not (p["max_rotation"] >= 0.0 and math.isfinite(p["max_rotation"])):
        return "max_rotation"
    if not (1 <= rows <= 4096 and 2 <= cols <= 8192):
        return "shape"
    if (p["n"] // 2) * p["resolution"] > (cols - 1) * p["range_resolution"]:
        return "disc"
    return None


def cos_sin_table(n):
    """E[k] = (cos, sin)(2 pi k / n), k < n, fp32, mirror-symmetric BY CONSTRUCTION (one libm cosine per k <= n / 4, the rest copied):
    cos[n - k] == cos[k], sin[n - k] == -sin[k] bit for bit, which is what makes a pair of a scan with itself come out at exactly 0"""
    q = [F32(math.cos(2.0 * math.pi * k / n)) for k in range(n // 4 + 1)]
    q[n // 4] = F32(0.0)

    def c(k):
        k %= n
        if k > n // 2:
            k = n - k
        return -q[n // 2 - k] if k > n // 4 else q[k]

    out = np.zeros((n, 2), dtype=F32)
    for k in range(n):
        out[k, 0] = c(k)
        out[k, 1] = c(k - n // 4)
    return out


class Tables:
    def __init__(self, p, rows, cols):
        bad = check_params(p, rows, cols)
        if bad:
            raise ValueError(bad)
        n = self.n = p["n"]
        self.rows, self.cols, self.p = rows, cols, dict(p)
        res, rres = float(p["resolution"]), float(p["range_resolution"])
        rho_max = (n // 2 - 1) * res
        mr = np.full((n, n), -1.0, dtype=F32)   # range-bin coordinate, -1 = outside (zero pixel)
        ma = np.zeros((n, n), dtype=F32)        # azimuth-row coordinate in [0, rows)
        for i in range(n):
            y = (i - n // 2) * res
            for j in range(n):
                x = (j - n // 2) * res
                rho = math.sqrt(x * x + y * y)
                rc = rho / rres - 0.5           # bin r covers [r, r + 1) range_resolution: its centre is at r + 0.5
                if rho > rho_max or rc < 0.0 or rc < p["min_range_bins"] or rc > cols - 1:
                    continue
                phi = math.atan2(y, x)
                if phi < 0.0:
                    phi += 2.0 * math.pi
                a = F32(phi * rows / (2.0 * math.pi))   # rows evenly spaced: row a is at 2 pi a / rows
                mr[i, j] = F32(rc)
                ma[i, j] = a if a < F32(rows) else F32(0.0)
        self.map_r, self.map_a = mr, ma
        self.hann = np.array([F32(0.5 - 0.5 * math.cos(2.0 * math.pi * k / n)) for k in range(n)], dtype=F32)
        self.E = cos_sin_table(n)
        self.dirs = np.array([[F32(math.cos(math.pi * k / n)), F32(math.sin(math.pi * k / n))] for k in range(n)], dtype=F32)
        self.hp = np.array([F32(math.cos(math.pi * (u - n // 2) / n)) for u in range(n)], dtype=F32)


def cart_image(img, col_offset, tab, psi=0.0):
    """windowed Cartesian image at rotation psi, fp32, THE operation order:
      s = (float)fmod(psi rows / (2 pi), rows) (+ rows if negative; fp64, one rounding);  a = map_a + s;  if a >= rows: a -= rows
      a0 = floor(a), fa = a - a0, a1 = a0 + 1 (0 at rows);  r0 = floor(map_r), fr = map_r - r0, r1 = min(r0 + 1, cols - 1)
      v = (((1 - fa)(1 - fr)) p00 + ((1 - fa) fr) p01) + (fa (1 - fr)) p10) + (fa fr) p11;   out = (v hann[i]) hann[j]"""
    n, rows, cols = tab.n, tab.rows, tab.cols
    s = math.fmod(psi * rows / (2.0 * math.pi), rows)
    if s < 0.0:
        s += rows
    s = F32(s)
    if s >= F32(rows):
        s = F32(0.0)
    a = tab.map_a + s
    a = np.where(a >= F32(rows), a - F32(rows), a).astype(F32)
    a0 = np.floor(a)
    fa = (a - a0).astype(F32)
    a0 = a0.astype(np.int64)
    a0 = np.where(a0 >= rows, rows - 1, a0)
    a1 = np.where(a0 + 1 >= rows, 0, a0 + 1)
    inside = tab.map_r >= 0
    mr = np.where(inside, tab.map_r, F32(0.0)).astype(F32)
    r0f = np.floor(mr)
    fr = (mr - r0f).astype(F32)
    r0 = r0f.astype(np.int64)
    r1 = np.minimum(r0 + 1, cols - 1)
    pw = np.asarray(img)[:, col_offset:col_offset + cols]
    p00, p01 = pw[a0, r0].astype(F32), pw[a0, r1].astype(F32)
    p10, p11 = pw[a1, r0].astype(F32), pw[a1, r1].astype(F32)
    one = F32(1.0)
    ga, gr = (one - fa).astype(F32), (one - fr).astype(F32)
    v = (((ga * gr) * p00 + (ga * fr) * p01) + (fa * gr) * p10) + (fa * fr) * p11
    v = np.where(inside, v, F32(0.0)).astype(F32)
    out = (v * tab.hann[:, None]) * tab.hann[None, :]
    assert out.dtype == F32
    return out


def scan_spectra(cart, tab):
    """-> F [n, n] the 2-D spectrum, A [n / 2 - R_MIN, n] the angle spectrum of the high-passed, polar-resampled magnitude"""
    n = tab.n
    F = np.fft.fft2(cart.astype(np.float64))
    M = np.fft.fftshift(np.abs(F))
    X = tab.hp.astype(np.float64)[:, None] * tab.hp.astype(np.float64)[None, :]
    M = M * ((1.0 - X) * (2.0 - X))
    rad = np.arange(R_MIN, n // 2, dtype=np.float64).astype(F32)
    u = (F32(n // 2) + rad[:, None] * tab.dirs[None, :, 0]).astype(F32)   # [radius, angle], fp32 coordinates as the device forms them
    v = (F32(n // 2) + rad[:, None] * tab.dirs[None, :, 1]).astype(F32)
    u0, v0 = np.floor(u), np.floor(v)
    fu, fv = (u - u0).astype(np.float64), (v - v0).astype(np.float64)
    u0, v0 = u0.astype(np.int64), v0.astype(np.int64)
    u1, v1 = np.minimum(u0 + 1, n - 1), np.minimum(v0 + 1, n - 1)
    P = (((1 - fv) * (1 - fu)) * M[v0, u0] + ((1 - fv) * fu) * M[v0, u1]) + ((fv * (1 - fu)) * M[v1, u0] + (fv * fu) * M[v1, u1])
    return F, np.fft.fft(P, axis=1)


def _parabola(cm, c0, cp):
    den = cm - 2.0 * c0 + cp
    return 0.0 if den == 0.0 else 0.5 * (cm - cp) / den


def rotation(A_src, A_dst, n):
    """-> curve [n] (1 at a perfect match), k0, theta0 in [-pi / 2, pi / 2), rot_peak.  Radius r contributes its angular frequencies
    |f| <= r only: the half circle of radius r crosses about pi r cells of the spectrum, above that frequency the resampled ring holds
    the kinks of the bilinear interpolant, which belong to the grid and do not turn with the scene (they vote for a rotation of 0)"""
    C = A_dst * np.conj(A_src)
    mag = np.abs(C)
    den = mag + EPS * mag.max()
    Cn = np.where(den > 0, C / np.where(den > 0, den, 1.0), 0.0)
    f = np.minimum(np.arange(n), n - np.arange(n))
    S = np.zeros(n, dtype=np.complex128)
    total = 0.0                    # the sum of the terms' magnitudes (each about 1): the curve is 1 at a perfect match whatever EPS removes
    for r in range(Cn.shape[0]):   # the radii in ascending order
        S = S + np.where(f <= r + R_MIN, Cn[r], 0.0)
        total += float(np.where(f <= r + R_MIN, np.abs(Cn[r]), 0.0).sum())
    curve = np.real(np.fft.ifft(S)) * (n / total if total > 0.0 else 0.0)
    k0 = int(np.argmax(curve))     # ties: the lowest index
    d = _parabola(curve[(k0 - 1) % n], curve[k0], curve[(k0 + 1) % n])
    ks = k0 - n if k0 >= n // 2 else k0
    return curve, k0, (ks + d) * math.pi / n, float(curve[k0])


def translation(F_dst, cart_src, n):
    """-> surface [n, n], (i0, j0), dx, dy [pixels], peak, peak_ratio"""
    G = np.fft.fft2(cart_src.astype(np.float64))
    C = F_dst * np.conj(G)
    mag = np.abs(C)
    den = mag + EPS * mag.max()
    Cn = np.where(den > 0, C / np.where(den > 0, den, 1.0), 0.0)
    total = float(np.abs(Cn).sum())   # (each term about 1) the surface is 1 at a perfect match whatever EPS removes
    s = np.real(np.fft.ifft2(Cn)) * (n * n / total if total > 0.0 else 0.0)
    flat = int(np.argmax(s))       # ties: the lowest row-major index
    i0, j0 = divmod(flat, n)
    dj = _parabola(s[i0, (j0 - 1) % n], s[i0, j0], s[i0, (j0 + 1) % n])
    di = _parabola(s[(i0 - 1) % n, j0], s[i0, j0], s[(i0 + 1) % n, j0])
    t = s.copy()
    for a in (-1, 0, 1):
        for b in (-1, 0, 1):
            t[(i0 + a) % n, (j0 + b) % n] = -np.inf
    peak = float(s[i0, j0])
    js, is_ = (j0 - n if j0 >= n // 2 else j0), (i0 - n if i0 >= n // 2 else i0)
    return s, (i0, j0), js + dj, is_ + di, peak, (float(t.max()) / peak if peak != 0.0 else 0.0)


def wrap_pi(t):
    return t - 2.0 * math.pi if t > math.pi else t


class Restatement:
    """every scan of a batch is transformed once; a pair reads two slots"""

    def __init__(self, rows, cols, params=None):
        self.p = default_params()
        if params:
            self.p.update(params)
        self.tab = Tables(self.p, rows, cols)

    def register_batch(self, images, pairs, col_offset=0):
        """images: [n_images, rows, row_stride] u8; pairs: [(src, dst)] -> list of dicts (the fields of rsx_phasecorr_result + the
        surfaces rsx_phasecorr_correlation copies out), and the theta = 0 images"""
        tab, n, p = self.tab, self.tab.n, self.p
        for s, d in pairs:
            if not (0 <= s < len(images) and 0 <= d < len(images)):
                raise ValueError("pair index")
        carts = [cart_image(im, col_offset, tab) for im in images]
        spectra = [scan_spectra(c, tab) for c in carts]
        out = []
        for s, d in pairs:
            curve, k0, th0, rot_peak = rotation(spectra[s][1], spectra[d][1], n)
            best, peaks = None, []
            for c in range(2 if p["resolve_half_turn"] else 1):
                th = th0 if c == 0 else wrap_pi(th0 + math.pi)
                surf, ij, dx, dy, peak, ratio = translation(spectra[d][0], cart_image(images[s], col_offset, tab, psi=-th), n)
                peaks.append(peak)
                if best is None or peak > best["peak"]:
                    best = dict(x=dx * p["resolution"], y=dy * p["resolution"], theta=th, peak=peak, peak_ratio=ratio, rot_peak=rot_peak,
                                half_turn=c, status=0, rot_k0=k0, rot_curve=curve, surface=surf, peak_ij=ij)
            best["other_peak"] = peaks[1 - best["half_turn"]] if len(peaks) == 2 else None   # the losing candidate's peak
            if p["max_rotation"] > 0.0 and abs(best["theta"]) > p["max_rotation"]:
                best["status"] |= STATUS_ROTATION
            out.append(best)
        return out, carts
