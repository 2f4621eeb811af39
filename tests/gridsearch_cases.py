"""Case builders shared by the wide-window search tests (tests/test_gridsearch_restatement.py, tests/test_gpu_gridsearch.py): the planes,
clouds and priors of tests/gridmatch_cases.py under the windows that the search adds, and the parameters as dicts of
tests/gridsearch_np.py."""
import numpy as np

import gridmap_cases as gc
import gridmatch_cases as gxc
import gridsearch_np as gs

SIZES = gxc.SIZES
N_POINTS = gxc.N_POINTS
# (K, U, V): the empty window; one partial block; 9 wide, a full and a partial block; past match's cap with U != V
WINDOWS = [(0, 0, 0), (1, 3, 0), (2, 4, 3), (1, 33, 5)]
WIDE = (0, 256, 256)       # on 64 x 64 with 300 points: the widest shifts, 65 x 65 blocks
TURNS = (180, 1, 1)        # on 64 x 64: the most rotations
DENSE = (1, 40, 24)        # on 192 x 128 with a random plane: 11 x 7 blocks a rotation, most of them refined, sixteen at a time
RESTATED = WINDOWS + [(0, 40, 40), (1, 256, 256)]   # what the restatement is checked on, 40 points on 64 x 64


def window(K, U, V, angle_step=0.013, min_score=0):
    return gs.params(angle_steps=K, x_cells=U, y_cells=V, angle_step=angle_step, min_score=min_score)


def as_match(mp):
    """the same window as parameters of tests/gridmatch_np.py (for windows within match's caps)"""
    return gxc.gx.params(angle_steps=mp["angle_steps"], x_cells=mp["x_cells"], y_cells=mp["y_cells"], angle_step=mp["angle_step"])


def volume_case(seed, width, height, K, U, V, sizes=N_POINTS, angle_step=0.013):
    """every N of sizes at every prior of border_priors, one job each: -> L, clouds (list), priors (n, 6), p, mp"""
    rng = np.random.default_rng(seed)
    p = gc.small_params(width, height)
    _, priors = gxc.border_priors(p)
    clouds, pri = [], []
    for n in sizes:
        for t in priors:
            clouds.append(gxc.cloud(rng, n, p))
            pri.append(t)
    return gxc.plane(seed + 1, p), clouds, np.array(pri), p, window(K, U, V, angle_step)


def reference(L, clouds, priors, p, mp, device_entry=False):
    xy, off = gxc.ragged(clouds)
    return gs.search_batch(L, xy, off, priors, p, mp, device_entry=device_entry)


def peaked():
    """a 64 x 64 plane that is 0 but for one cell of 200, and a cloud of one point that the candidate (k, u, v) = (0, 5, -3) puts
    there: the peak is 200 and it is alone -> L, clouds, priors, p, mp (K = 1, U = 9, V = 6)"""
    p = gc.gm.params(width=64, height=64, resolution=0.5, origin_x=0.0, origin_y=0.0)
    mp = window(1, 9, 6, angle_step=0.2)
    pts = np.array([[4.0, 0.0]], dtype=np.float32)
    prior = gc.matrices([(10.25, 10.25, 0.0)])
    c, s = gxc.gx.tables(mp)
    ix, iy = gs.cells(pts, prior[0], c[1], s[1], p, gs.margin(mp))
    L = np.zeros((64, 64), dtype=np.uint8)
    L[iy[0] - 3, ix[0] + 5] = 200
    return L, [pts], prior, p, mp


def moved(prior, dx, dy):
    """a prior (6,) moved by (dx, dy) metres in the map frame"""
    t = np.array(prior, dtype=np.float64)
    t[2] += dx
    t[5] += dy
    return t


# ---- end to end: the scene of gridmatch_cases.end_to_end, the prior off by tens of metres ----

E2E_NEAR = dict(prior=0, move=(17.0, -13.0), window=(8, 32, 32), winner=(-3, -20, 15), scores=(1144127, 469444), share=0.05)
E2E_FAR = dict(prior=2, move=(71.0, -52.0), window=(8, 128, 128), winner=(0, -71, 52), share=0.01)


def e2e_params(case):
    K, U, V = case["window"]
    return window(K, U, V, angle_step=0.01)
