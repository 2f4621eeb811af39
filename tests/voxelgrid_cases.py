"""The clouds of tests/test_gpu_voxelgrid_paths.py, and the facts that put each of them into the regime of
csrc/voxelgrid.hip its name claims.  tests/test_voxelgrid_cases.py checks those facts on the CPU (the oracle and numpy
alone), so that a cloud which has drifted out of its regime fails there, where it is cheap, and not by passing silently on
the GPU.

grid_facts restates steps 1-3 of the header of oracle/voxelgrid_ref.c (float32 arithmetic, PCL's int64 / int casts); it
is NOT derived from the kernel.  From the grid's volume follow the width of the sort key the cooperative kernel uses:
nbits = the smallest b with 2^b >= vol (at most 31), a non-finite point's key is 1 << nbits, and the LSD radix sort takes
passes = (nbits + 8) // 8 passes of 8 bits -- at nbits = 8, 16, 24 the last pass exists for that one bit only."""
import numpy as np

from test_oracle_voxelgrid import _cloud

SENTINEL = np.uint32(0xDEADBEEF)  # pre-fill of host output buffers: no centroid of these clouds has this bit pattern


def grid_facts(p, leaf):
    """-> dict: d_prod (step 2's product), overflow (d_prod > INT32_MAX), min_b, div_b, vol, nbits, passes, n_finite"""
    p = np.asarray(p, dtype=np.float32)
    q = p[np.isfinite(p[:, :3]).all(1), :3]
    inv = np.float32(1.0) / np.float32(leaf)
    mn, mx = q.min(0), q.max(0)
    d = ((mx - mn) * inv).astype(np.int64) + 1
    d_prod = int(d[0]) * int(d[1]) * int(d[2])
    min_b = np.floor(mn * inv).astype(np.int32)
    div_b = np.floor(mx * inv).astype(np.int32) - min_b + 1
    vol = int(div_b[0]) * int(div_b[1]) * int(div_b[2])
    nbits = 0
    while nbits < 31 and (1 << nbits) < vol:
        nbits += 1
    return {"d_prod": d_prod, "overflow": d_prod > 2**31 - 1, "min_b": min_b, "div_b": tuple(int(v) for v in div_b), "vol": vol,
            "nbits": nbits, "passes": (nbits + 8) // 8, "n_finite": len(q)}


def voxel_index(p, leaf):
    """step 4 of voxelgrid_ref.c: the voxel index of every row, -1 for a non-finite one (int64)"""
    p = np.asarray(p, dtype=np.float32)
    f = grid_facts(p, leaf)
    fin = np.isfinite(p[:, :3]).all(1)
    inv = np.float32(1.0) / np.float32(leaf)
    mul = np.array([1, f["div_b"][0], f["div_b"][0] * f["div_b"][1]], dtype=np.int64)
    idx = np.full(len(p), -1, dtype=np.int64)
    ijk = (np.floor(p[fin, :3] * inv) - f["min_b"].astype(np.float32)).astype(np.int32)
    idx[fin] = (ijk.astype(np.int64) * mul).sum(1)
    return idx


def poison(p, rows, rng):
    """rows of p made non-finite: NaN, +inf or -inf in x, y or z, in turn"""
    bad = np.float32([np.nan, np.inf, -np.inf])
    rows = np.unique(np.asarray(rows, dtype=np.int64))
    rows = rows[(rows >= 0) & (rows < len(p))]
    p[rows, rng.integers(0, 3, len(rows))] = bad[np.arange(len(rows)) % 3]
    return rows


def _edge_rows(n, multiples):
    """row 0, the last row, and the rows on both sides of every multiple of each of `multiples`"""
    rows = [0, n - 1]
    for m in multiples:
        for k in range(m, n, m):
            rows += [k - 1, k, k + 1]
    return [r for r in rows if 0 <= r < n]


# ---- key widths: div_b -> (vol, nbits, passes) ----
LATTICE = {
    (16, 8, 1): (128, 7, 1),
    (16, 16, 1): (256, 8, 2),
    (257, 1, 1): (257, 9, 2),
    (256, 128, 1): (1 << 15, 15, 2),
    (256, 256, 1): (1 << 16, 16, 3),
    (256, 256, 128): (1 << 23, 23, 3),
    (256, 256, 256): (1 << 24, 24, 4),
}
KEY_SIZES = (3000, 6000)  # the one-workgroup kernel; the cooperative kernel with six workgroups of 1024 points
# Rows of voxel 0, with non-finite rows between them.  The low bits of a non-finite point's key are those of voxel 0, so a
# sort that stops one pass early (or hands on the buffer of the pass before) leaves them BETWEEN the points of voxel 0, in
# input order -- which shows only if voxel 0 has points on both sides of them.  (With the corner point alone in voxel 0 a
# swapped final buffer passed the 16- and 24-bit cases.)
VOXEL0_ROWS = (1, 62, 66, 254, 258, 1022, 1026, 2046)
WIDE_FACTS = (1668347681, 31, 4)  # lattice-free case below: vol, nbits, passes
WIDE_LEAF = 0.4


def _key_poison(p, keep, rng):
    """at least 1 % of the rows non-finite: row 0, the last row, both sides of every multiple of 64 ... 1024 (chunk, share
    and tile ends of the cooperative kernel at these sizes) and random ones; `keep` (the corner points) stay finite"""
    n = len(p)
    rows = set(_edge_rows(n, (1024,))) | {63, 64, 65, 255, 256, 257} | set(rng.choice(n, n // 100 + 1, replace=False).tolist())
    return poison(p, sorted(rows - set(keep)), rng)


def lattice_cloud(div_b, n):
    """leaf 1.0 (inv exactly 1): coordinates k + 0.25 .. k + 0.75 with integer k in [0, div_b), drawn from n // 2 cells so that
    voxels are shared; corner points (0.5, 0.5, 0.5) and div_b - 0.5 at rows 1 and n - 2 pin min_b = 0 and div_b, and carry the
    smallest and the largest voxel index (0 and vol - 1)"""
    rng = np.random.default_rng([n, *div_b])
    cells = np.stack([rng.integers(0, d, n // 2) for d in div_b], 1)
    pick = rng.integers(0, len(cells), n)
    p = np.zeros((n, 4), dtype=np.float32)
    p[:, :3] = cells[pick] + rng.uniform(0.25, 0.75, (n, 3))
    p[:, 3] = rng.uniform(0, 255, n)
    p[list(VOXEL0_ROWS), :3] = rng.uniform(0.25, 0.75, (len(VOXEL0_ROWS), 3))   # voxel 0, around the non-finite rows
    p[1, :3] = 0.5
    p[n - 2, :3] = np.float32(div_b) - np.float32(0.5)
    _key_poison(p, VOXEL0_ROWS + (n - 2,), rng)
    return p, 1.0


def wide_cloud(n):
    """nbits = 31: x, y uniform in [0.2, 516.2], z in [0.2, 400.2], leaf 0.4, corner points at both ends -- a grid of
    1291 x 1291 x 1001 voxels, between 2^30 and 2^31, so a non-finite point's key is 1u << 31.  Half the rows are a
    neighbour (within 0.05) of another row, so voxels are shared"""
    rng = np.random.default_rng([n, 31])
    lo, hi = np.float32([0.2, 0.2, 0.2]), np.float32([516.2, 516.2, 400.2])
    p = np.zeros((n, 4), dtype=np.float32)
    h = n // 2
    p[:h, :3] = rng.uniform(lo, hi, (h, 3))
    p[h:, :3] = np.clip(p[rng.integers(0, h, n - h), :3] + rng.uniform(-0.05, 0.05, (n - h, 3)).astype(np.float32), lo, hi)
    p[:] = p[rng.permutation(n)]
    p[:, 3] = rng.uniform(0, 255, n)
    p[1, :3] = lo
    p[n - 2, :3] = hi
    _key_poison(p, (1, n - 2), rng)
    return p, WIDE_LEAF


# ---- large shares: clouds of the cooperative kernel whose wavefront shares do not fit its registers ----
# (at most CO_MAX_W = 128 workgroups of four wavefronts, CO_CH = 8 chunks of 64 points in registers: 128 x 4 x 8 x 64 =
# 262 144 points; a device that keeps fewer workgroups resident switches earlier, never later)
LARGE_SIZES = (262144, 262145, 300000, 5000, 300000)  # in this order on ONE handle
LARGE_LEAF = 0.4
CROWD_A = np.float32([10.05, -3.15, 5.25])   # + [0, 0.3): inside ONE 0.4 m voxel, above every other point (z <= 3)
CROWD_B = np.float32([-20.35, 14.05, 5.25])


def crowd_size(n):
    return 20000 if n >= 200000 else n // 10


def large_cloud(seed, n):
    """_cloud(seed, n) with 3 % of the rows non-finite (row 0, row n - 1, multiples of 2304 and of 2560 +- 1: the workgroup
    tiles at 262 145 and at 300 000 points, and random ones), one voxel of crowd_size(n) points spread evenly over the whole
    cloud and one of as many points at consecutive indices (but for the non-finite rows and those of the other crowd between
    them: it spans several workgroup tiles).
    -> (cloud, rows of the consecutive crowd, rows of the spread one)"""
    rng = np.random.default_rng([seed, n])
    p = _cloud(seed, n)
    rows = set(_edge_rows(n, (2304, 2560))) | set(rng.choice(n, n * 3 // 100, replace=False).tolist())
    poison(p, sorted(rows), rng)
    fin = np.flatnonzero(np.isfinite(p[:, :3]).all(1))
    c = crowd_size(n)
    b = fin[np.linspace(0, len(fin) - 1, c).astype(np.int64)]
    rest = np.setdiff1d(fin, b)
    a = rest[rest >= n // 7][:c]
    p[a, :3] = CROWD_A + rng.uniform(0, 0.3, (c, 3)).astype(np.float32)
    p[b, :3] = CROWD_B + rng.uniform(0, 0.3, (c, 3)).astype(np.float32)
    return p, a, b


def overflow_cloud(seed, n):
    """with leaf 0.01 and one far point the grid would need more than 2^31 voxels: the filter returns its input"""
    p = _cloud(seed, n)
    p[17, :3] = [3e4, 3e4, 3e3]
    return p, 0.01


# ---- the one-workgroup kernel: n <= 4096, keys padded to a power of two, four sorted positions per thread ----
SMALL_SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097)  # (4097: back to the cooperative kernel)
SMALL_LEAF = 0.4


def small_cloud(n):
    """_cloud(n, n) with NaN rows at 0 and n - 1 (n <= 2: nothing finite is left); from four points on, row 2 sits on row 1,
    so at least one voxel holds two points"""
    p = _cloud(n, n)
    if n >= 4:
        p[2, :3] = p[1, :3]
    p[0, 0] = np.nan
    p[n - 1, 2] = np.nan
    return p


def one_voxel_cloud(n=4096):
    rng = np.random.default_rng(n)
    p = np.zeros((n, 4), dtype=np.float32)
    p[:, :3] = CROWD_A + rng.uniform(0, 0.3, (n, 3)).astype(np.float32)
    p[:, 3] = rng.uniform(0, 255, n)
    return p, 0.4


def own_voxel_cloud():
    """4096 points, each alone in its voxel: a 16 x 16 x 16 lattice of pitch 0.01 under a leaf of 0.001, rows shuffled"""
    rng = np.random.default_rng(4096)
    g = np.stack(np.meshgrid(*[np.arange(16)] * 3, indexing="ij"), -1).reshape(-1, 3)
    p = np.zeros((4096, 4), dtype=np.float32)
    p[:, :3] = (g[rng.permutation(4096)] + 0.5) * 0.01
    p[:, 3] = rng.uniform(0, 255, 4096)
    return p, 0.001


# ---- point layouts: (stride in bytes, byte offset of the intensity or -1) ----
LAYOUTS = ((32, 16), (32, 28), (20, -1))  # pcl::PointXYZI; intensity in the last word; no intensity, two words of padding


def layout_cloud(p, stride, ioff):
    """the (n, 4) cloud p laid out with `stride` bytes per point; every word that is neither x, y, z nor the intensity is NaN,
    so a read at a wrong offset shows"""
    a = np.full((len(p), stride // 4), np.nan, dtype=np.float32)
    a[:, :3] = p[:, :3]
    if ioff >= 0:
        a[:, ioff // 4] = p[:, 3]
    return a


def truncation_cloud(n):
    """a cloud of n points (3000: one workgroup; 6000: cooperative) with non-finite rows, for max_out below the output count"""
    rng = np.random.default_rng(n)
    p = _cloud(100 + n, n)
    poison(p, [0, n - 1] + rng.choice(n, n // 50, replace=False).tolist(), rng)
    return p, 0.4
