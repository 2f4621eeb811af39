"""Inputs of the ORORA solver parity tests beyond the defaults, built ONCE so that the GPU test (tests/test_gpu_orora.py) and
the CPU knife-edge test (tests/test_oracle_orora_np.py) see the same data.

Iteration count and inlier counts are decided at thresholds, and the GPU adds in another order than the oracle.  So every
pair of at most KNIFE_EDGE_MAX_K matches in here must be one on which the two CPU restatements (oracle/orora_ref.c and
oracle/orora_np.py, which also add in different orders) agree EXACTLY on iterations and both inlier counts:
test_oracle_orora_np.py::test_gpu_parity_cases_are_not_knife_edge asserts that for all of them; the seeds below were picked
until it held.  Larger pairs follow the rule of test_gpu_orora._check: counts equal on the given data."""
import numpy as np

from navtech_radar_slam_amd import synth

KNIFE_EDGE_MAX_K = 400
PARAM_SEED, BIG_SEED = 4101, 4102
DEFAULTS = dict(tim_noise_bound=1.5, noise_bound_radial=0.3536, noise_bound_tangential=1.8 * np.pi / 180.0, gnc_factor=1.4,
                cost_threshold=1e-6, max_iterations=100)


def _batch(pairs):
    src = np.concatenate([p[0] for p in pairs]).astype(np.float32)
    dst = np.concatenate([p[1] for p in pairs]).astype(np.float32)
    off = np.zeros(len(pairs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(p[0]) for p in pairs])
    return np.ascontiguousarray(src), np.ascontiguousarray(dst), off


def _split(src, dst, off):
    return [(src[off[i]:off[i + 1]], dst[off[i]:off[i + 1]]) for i in range(len(off) - 1)]


def _rot(yaw):
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([[c, s], [-s, c]])       # row vectors: d = s @ _rot(yaw) + t


def param_cases():
    """[(name, {field: value}, src, dst, off)]: one numeric field of rsx_orora_params off its default at a time, on six pairs of
    40 to 400 matches plus one pair of 2 300 (the HBM-workspace kernel)."""
    small = synth.orora_pairs(PARAM_SEED, 6, k_range=(40, 400))
    big = synth.orora_pairs(BIG_SEED, 1, k_range=(2300, 2300))
    src, dst, off = _batch(_split(*small[:3]) + _split(*big[:3]))
    out = []
    for v in (0.3, 1.5, 6.0, 0.0):           # 0.0: c2 < 1e-16 -> 1e-2, the replacement kernel and oracle share
        out.append((f"tim_noise_bound={v}", {"tim_noise_bound": v}, src, dst, off))
    for f in ("noise_bound_radial", "noise_bound_tangential"):
        for m in (0.25, 4.0):
            out.append((f"{f}x{m}", {f: DEFAULTS[f] * m}, src, dst, off))
    for m in (0.25, 4.0):
        out.append((f"noise_bounds_both_x{m}", {"noise_bound_radial": DEFAULTS["noise_bound_radial"] * m,
                                                "noise_bound_tangential": DEFAULTS["noise_bound_tangential"] * m}, src, dst, off))
    for v in (1.05, 1.4, 3.0):
        out.append((f"gnc_factor={v}", {"gnc_factor": v}, src, dst, off))
    for v in (1e-12, 1e-2):
        out.append((f"cost_threshold={v}", {"cost_threshold": v}, src, dst, off))
    for v in (1, 3, 100):
        out.append((f"max_iterations={v}", {"max_iterations": v}, src, dst, off))
    return out


def _lattice_pair(rng, k):
    """coordinates on a 0.25 m lattice, a pure lattice translation, a third of the matches replaced by other lattice points:
    exactly tied residuals and interval endpoints in large numbers"""
    s = rng.integers(-320, 321, (k, 2)) * 0.25
    d = s + np.array([0.5, -0.25])
    n_out = k // 3
    d[rng.choice(k, n_out, replace=False)] = rng.integers(-320, 321, (n_out, 2)) * 0.25
    return s, d


def geometry_cases():
    """[(name, {}, src, dst, off)]: geometry synth.orora_pairs never produces"""
    out = []
    for name, yaw, seed in (("yaw=+3.1", 3.1, 4201), ("yaw=-3.1", -3.1, 4202), ("yaw=+pi/2", np.pi / 2, 4203), ("yaw=-pi/2", -np.pi / 2, 4204)):
        s = synth.orora_pairs(seed, 4, k_range=(40, 400), yaw_range=(yaw, yaw))
        b = synth.orora_pairs(seed + 50, 1, k_range=(2100, 2100), yaw_range=(yaw, yaw))
        out.append((name, {}, *_batch(_split(*s[:3]) + _split(*b[:3]))))

    rng = np.random.default_rng(4301)
    # the origin and points on the axes, in src AND (identity motion, these matches noise-free) in dst: aniso_bound with rho == 0,
    # c == 0 or s == 0; then the same src under a general motion
    special = np.array([[0.0, 0.0], [30.0, 0.0], [0.0, 30.0], [-12.5, 0.0], [0.0, -12.5], [0.0, 0.0]])
    pairs = []
    for yaw, t in ((0.0, (0.0, 0.0)), (0.1, (1.0, -0.5))):
        s = np.concatenate([special, rng.uniform(-60, 60, (70, 2))])
        d = s @ _rot(yaw) + np.array(t)
        d[len(special):] += rng.normal(0, 0.05, (70, 2))
        d[len(special) + 5:len(special) + 25] = rng.uniform(-60, 60, (20, 2))
        perm = rng.permutation(len(s))
        pairs.append((s[perm], d[perm]))
    out.append(("origin_and_axes", {}, *_batch(pairs)))

    # every match twice, one after the other: zero-length TIMs on the ring, every interval endpoint tied with its twin's
    s = synth.orora_pairs(4401, 3, k_range=(40, 200))
    out.append(("duplicated_matches", {}, *_batch([(np.repeat(a, 2, axis=0), np.repeat(b, 2, axis=0)) for a, b in _split(*s[:3])])))

    # all source points identical: every TIM has a = 0, C = S = 0, the identity-rotation branch
    rng = np.random.default_rng(4501)
    pairs = []
    for k in (2, 9, 120):
        s = np.tile(np.array([[7.25, -3.5]]), (k, 1))
        pairs.append((s, s + np.array([0.75, 0.5]) + rng.normal(0, 0.05, (k, 2))))
    out.append(("identical_sources", {}, *_batch(pairs)))

    rng = np.random.default_rng(4601)
    pairs = []
    for k in (2, 3, 2, 3):
        s = rng.uniform(-40, 40, (k, 2))
        pairs.append((s, s @ _rot(0.07) + np.array([0.4, -0.3]) + rng.normal(0, 0.03, (k, 2))))
    out.append(("K=2_and_K=3", {}, *_batch(pairs)))

    # every bitonic_sort_regs<E> instantiation and the plain network: 2 K endpoints at each sort size
    rng = np.random.default_rng(4701)
    out.append(("lattice_ties", {}, *_batch([_lattice_pair(rng, k) for k in (64, 127, 128, 129, 256, 400, 512, 1024, 2047, 2048, 2049, 3000)])))
    return out


def all_cases():
    return param_cases() + geometry_cases()


def np_register(s, d, fields, flags=0):
    from oracle import orora_np
    kw = dict(DEFAULTS)
    kw.update(fields)
    return orora_np.register(s, d, complete=bool(flags & 1), teaser_cost=bool(flags & 2), **kw)
