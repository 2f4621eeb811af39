"""Case builders shared by the refinement tests (tests/test_gridrefine_restatement.py, tests/test_gpu_gridrefine.py): likelihood planes,
clouds, priors and the parameters as dicts of tests/gridmap_np.py and tests/gridrefine_np.py.  The maps, clouds and border priors are
those of tests/gridmatch_cases.py; a reference is computed once per case and shared (functools.lru_cache): nobody writes into it."""
import functools
import math

import numpy as np

import gridmap_cases as gc
import gridmatch_cases as gxc
import gridrefine_np as gr

SIZES = gxc.SIZES
N_POINTS = [0, 1, 63, 64, 65, 255, 256, 257, 300, 8192]
ragged = gxc.ragged


def reference(L, clouds, priors, p, rp, device_entry=False, evaluate_fn=None):
    xy, off = ragged(clouds)
    return gr.refine_batch(L, xy, off, priors, p, rp, device_entry=device_entry, evaluate_fn=evaluate_fn)


# ---- a random plane: the reject path, lambda growth, MAX ----

@functools.lru_cache(maxsize=None)
def random_case(width, height):
    """every N of N_POINTS at every prior of border_priors (in the map, on every border, outside every border beyond the placement
    margin), one job each, on a random plane -> L, clouds (list), priors (n, 6), p"""
    rng = np.random.default_rng(1000 + width)
    p = gc.small_params(width, height)
    _, priors = gxc.border_priors(p)
    clouds, pri = [], []
    for n in N_POINTS:
        for t in priors:
            clouds.append(gxc.cloud(rng, n, p))
            pri.append(t)
    return gxc.plane(2000 + width, p), clouds, np.array(pri), p


@functools.lru_cache(maxsize=None)
def random_reference(width, height, max_evaluations=32):
    L, clouds, priors, p = random_case(width, height)
    return reference(L, clouds, priors, p, gr.params(max_evaluations=max_evaluations))


# ---- a smooth plane: the accept path ----

TENT_PEAK, TENT_RADIUS = 250.0, 3.0     # a cone of 3 cells around every stamped point
SMOOTH_TRUTH_YAW = 0.4
SMOOTH_OFFSETS = [(0.0, 0.0, 0.0), (0.2, -0.15, 0.002), (-0.24, 0.1, -0.004), (0.1, 0.22, 0.0), (0.45, -0.4, 0.006), (-0.3, -0.3, -0.003),
                  (0.05, 0.0, 0.01), (0.7, 0.6, -0.008)]      # prior minus truth: x, y [m] (cells of 0.5 m), yaw [rad]
SMOOTH_SIZES = [40, 33, 7, 1]             # a job takes the first n points of the stamped cloud


def tent_plane(pts, pose, p):
    """uint8 [height][width]: the largest of the cones TENT_PEAK (1 - d / TENT_RADIUS) around the points at the pose (x, y, yaw), d the
    distance in cells from the point to a cell's centre"""
    T = gc.matrices([pose])[0]
    x, y = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
    fx = (T[0] * x + T[1] * y + T[2] - p["origin_x"]) / p["resolution"]
    fy = (T[3] * x + T[4] * y + T[5] - p["origin_y"]) / p["resolution"]
    cx, cy = np.meshgrid(np.arange(p["width"]) + 0.5, np.arange(p["height"]) + 0.5)
    best = np.zeros((p["height"], p["width"]))
    for a, b in zip(fx, fy):
        best = np.maximum(best, TENT_PEAK * (1.0 - np.hypot(cx - a, cy - b) / TENT_RADIUS))
    return np.rint(np.maximum(best, 0.0)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def smooth_case(width, height):
    """40 points in a disc of 0.4 times the map's smaller side, stamped with the sensor at the middle of the map; jobs: the first n points
    for n of SMOOTH_SIZES at every offset of SMOOTH_OFFSETS -> L, clouds, priors, p, truth (x, y, yaw)"""
    rng = np.random.default_rng(3000 + width)
    p = gc.small_params(width, height)
    shrink = np.float32(0.4 * min(width, height) / (0.45 * width))
    pts = (gxc.cloud(rng, max(SMOOTH_SIZES), p) * shrink).astype(np.float32)
    truth = (p["origin_x"] + 0.5 * width * p["resolution"] + 0.13, p["origin_y"] + 0.5 * height * p["resolution"] - 0.21, SMOOTH_TRUTH_YAW)
    L = tent_plane(pts, truth, p)
    clouds, poses = [], []
    for n in SMOOTH_SIZES:
        for ex, ey, eth in SMOOTH_OFFSETS:
            clouds.append(pts[:n])
            poses.append((truth[0] + ex, truth[1] + ey, truth[2] + eth))
    return L, clouds, gc.matrices(poses), p, truth


@functools.lru_cache(maxsize=None)
def smooth_reference(width, height):
    L, clouds, priors, p, _ = smooth_case(width, height)
    return reference(L, clouds, priors, p, gr.params())


# ---- ties and edges ----

def edge_case(kind):
    """'zero': an all-zero plane; 'constant': a constant plane and a cloud so small that every point reads the constant (a zero
    gradient: the first pivot fails) -> L, clouds, priors, p"""
    p = gc.small_params(64, 64)
    rng = np.random.default_rng(21)
    _, priors = gxc.border_priors(p)
    if kind == "zero":
        return np.zeros((64, 64), dtype=np.uint8), [gxc.cloud(rng, 200, p)], priors[:1], p
    pts = (gxc.cloud(rng, 100, p) * np.float32(0.25)).astype(np.float32)
    return np.full((64, 64), 7, dtype=np.uint8), [pts], priors[:1], p


def pose_error(transform, truth):
    """-> (distance [m], |yaw difference| [rad]) of a six-double pose from (x, y, yaw)"""
    dyaw = math.atan2(transform[3], transform[0]) - truth[2]
    dyaw = (dyaw + math.pi) % (2.0 * math.pi) - math.pi
    return math.hypot(transform[2] - truth[0], transform[5] - truth[1]), abs(dyaw)


# ---- end to end: the drive of tests/gridmatch_cases.end_to_end ----

E2E_STARTS = [(0.0, 0.0, 0.0), (0.4, -0.3, 0.004), (-0.5, 0.5, -0.005), (0.45, 0.45, 0.0), (0.9, -0.8, 0.008), (1.5, 1.2, -0.01)]   # prior minus truth
E2E_LIMIT_M, E2E_LIMIT_RAD, E2E_EVALUATIONS = 0.05, 0.002, 32
CHAIN_ERROR = (3.4, -2.3, 0.034)


def e2e_truth(priors):
    """(x, y, yaw) of the query scan from end_to_end's third prior, which is the true pose"""
    t = priors[2]
    return float(t[2]), float(t[5]), math.atan2(float(t[3]), float(t[0]))


def e2e_starts(truth, errors=E2E_STARTS):
    return gc.matrices([(truth[0] + ex, truth[1] + ey, truth[2] + eth) for ex, ey, eth in errors])
