"""The likelihood field of the grid map on the GPU (csrc/gridfield.hip through navtech_radar_slam_amd.gridmap) against its restatement
(tests/gridfield_np.py): every byte of every plane, no tolerance -- the rule is integers throughout, so a difference is a bug.  And the
three localisers on the device's field against their restatements on the restated field, byte for byte."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gridfield_np as gf  # noqa: E402
import gridmap_cases as gc  # noqa: E402
import gridmap_np as gm  # noqa: E402
import gridmatch_cases as gxc  # noqa: E402
import gridmatch_np as gx  # noqa: E402
import gridrefine_cases as grc  # noqa: E402
import gridrefine_np as gr  # noqa: E402
import gridsearch_cases as gsc  # noqa: E402
import test_gridfield_abi as abi  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(64, 64), (192, 128), (64, 192)]          # (width, height): one tile wide and two high; 3 x 4 tiles; 1 x 6 tiles
RADII = [1, 2, 12, 64]
THRESHOLDS = [1, 50, 255]
DENSITIES = [0.01, 0.3]
EDGE = [0, 31, 32, 63]                             # modulo 64: the borders of a wavefront's word, of a tile and of its two halves


@pytest.fixture(scope="module")
def rsx():
    import __graft_entry__ as ge
    from navtech_radar_slam_amd import _rsx
    if not os.path.exists(_rsx.LIB_PATH):
        ge.build()
    return _rsx


def _map(width, height, L=None, rows=64, cols=96):
    from navtech_radar_slam_amd import gridmap
    m = gridmap.GridMap(rows, cols, gridmap.params(**gc.small_params(width, height)))
    if L is not None:
        m.set_likelihood(L)
    return m


def _same(got, want, what=""):
    assert got.dtype == np.uint8 and got.shape == want.shape, what
    bad = np.argwhere(got != want)
    assert got.tobytes() == want.tobytes(), (what, len(bad), "cells differ, the first (y, x) at", bad[:3].tolist(),
                                             [(int(got[y, x]), int(want[y, x])) for y, x in bad[:3]])


def _random_plane(rng, width, height, density, threshold):
    """about `density` of the cells at or above the threshold, the rest below it"""
    seeds = rng.random((height, width)) < density
    return np.where(seeds, rng.integers(threshold, 256, (height, width)), rng.integers(0, threshold, (height, width))).astype(np.uint8)


def _framed(m, width, height):
    """the whole buffer of the likelihood plane, the frame of 128 cells included, through likelihood_device and the pitch"""
    d, pitch = m.likelihood_device()
    assert pitch == width + 256
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.zeros((height + 256, pitch), dtype=np.uint8)
    assert hip.hipMemcpy(out.ctypes.data, d - 128 * pitch - 128, out.size, 2) == 0      # (2: device to host)
    return out


@pytest.mark.parametrize("width,height", SIZES)
def test_random_planes_equal_the_restatement(rsx, width, height):
    """about 1 % and 30 % of the cells seeds, radii 1, 2, 12, 64, thresholds 1, 50, 255, a random table (so that a wrong q shows): every
    byte; and the same plane through the same handle a second time: the same bytes"""
    rng = np.random.default_rng(width + 3 * height)
    m = _map(width, height)
    for radius in RADII:
        table = rng.integers(0, 256, radius * radius + 1, dtype=np.uint8)
        for threshold in THRESHOLDS:
            for density in DENSITIES:
                L = _random_plane(rng, width, height, density, threshold)
                fp = gf.params(threshold=threshold, radius=radius)
                want = gf.field(L, table, fp)
                assert want.any() and (L >= threshold).any() and not (L >= threshold).all()
                m.set_likelihood(L)
                m.likelihood_field(table, **fp)
                got = m.likelihood()
                _same(got, want, (width, height, radius, threshold, density))
                m.set_likelihood(L)
                m.likelihood_field(table, **fp)
                assert m.likelihood().tobytes() == got.tobytes()
    m.close()


@pytest.mark.parametrize("width,height", SIZES)
def test_q_itself(rsx, width, height):
    """three tables, q & 255, q >> 8 and 1: q and "a seed within the radius" for every cell, rebuilt from the three planes, against the
    restatement's -- the transform apart from the table"""
    rng = np.random.default_rng(7 * width + height)
    m = _map(width, height)
    for radius in RADII:
        q_all = np.arange(radius * radius + 1)
        tables = [(q_all & 255).astype(np.uint8), (q_all >> 8).astype(np.uint8), np.ones(len(q_all), dtype=np.uint8)]
        for density in DENSITIES + [0.0]:
            L = _random_plane(rng, width, height, density, 50)
            if density == 0.0:          # three seeds: q goes beyond 255, the high byte is used
                L[5, 3], L[height // 2, width - 2], L[height - 1, width // 3] = 50, 255, 77
            fp = gf.params(threshold=50, radius=radius)
            planes = []
            for t in tables:
                m.set_likelihood(L)
                m.likelihood_field(t, **fp)
                planes.append(m.likelihood().astype(np.int32))
            q, found = planes[0] + 256 * planes[1], planes[2] == 1
            want_q, want_found = gf.nearest(L, fp)
            assert set(np.unique(planes[2]).tolist()) <= {0, 1} and found.tobytes() == want_found.tobytes(), (radius, density)
            bad = np.argwhere(q != want_q)
            assert not len(bad), (radius, density, len(bad), bad[:3].tolist())
            assert want_found.any() and want_q.max() >= (256 if density == 0.0 and radius == 64 else 1)
    m.close()


@pytest.mark.parametrize("width,height", SIZES)
def test_edges(rsx, width, height):
    table = (np.arange(64 * 64 + 1) % 251 + 1).astype(np.uint8)          # no zero in it: "none within the radius" stands apart
    fp = gf.params(threshold=1, radius=64)
    m = _map(width, height)
    # no seed at all: zero everywhere; every cell a seed: table[0] everywhere
    m.set_likelihood(np.zeros((height, width), dtype=np.uint8))
    m.likelihood_field(table, **fp)
    assert not m.likelihood().any()
    m.set_likelihood(np.full((height, width), 49, dtype=np.uint8))
    m.likelihood_field(table, threshold=50, radius=64)
    assert not m.likelihood().any()
    m.set_likelihood(np.full((height, width), 49, dtype=np.uint8))
    m.likelihood_field(table, threshold=49, radius=64)
    assert (m.likelihood() == table[0]).all()
    # one seed in each corner and at the middle of each border, radius 64: the closed disc cut by the map, nothing wraps round a row
    # or a tile, nothing comes back from the frame
    yy, xx = np.mgrid[0:height, 0:width]
    spots = [(0, 0), (width - 1, 0), (0, height - 1), (width - 1, height - 1), (width // 2, 0), (width // 2, height - 1), (0, height // 2),
             (width - 1, height // 2)]
    for x, y in spots:
        L = np.zeros((height, width), dtype=np.uint8)
        L[y, x] = 1
        d2 = (xx - x) ** 2 + (yy - y) ** 2
        want = np.where(d2 <= 64 * 64, table[np.minimum(d2, 64 * 64)], 0).astype(np.uint8)
        assert want.tobytes() == gf.field(L, table, fp).tobytes()
        m.set_likelihood(L)
        m.likelihood_field(table, **fp)
        _same(m.likelihood(), want, ("one seed", x, y))
    whole = _framed(m, width, height)
    whole[128:128 + height, 128:128 + width] = 0
    assert not whole.any()
    # seeds at every x and y that is 0, 31, 32 or 63 modulo 64
    L = (np.isin(xx % 64, EDGE) & np.isin(yy % 64, EDGE)).astype(np.uint8) * 200
    for radius in RADII:
        fp = gf.params(threshold=200, radius=radius)
        m.set_likelihood(L)
        m.likelihood_field(table[:radius * radius + 1], **fp)
        _same(m.likelihood(), gf.field(L, table[:radius * radius + 1], fp), ("lattice", radius))
    # a row of seeds at the last row only, and a column at the last column only
    for L in (np.where(yy == height - 1, 255, 0).astype(np.uint8), np.where(xx == width - 1, 255, 0).astype(np.uint8)):
        for radius in (2, 64):
            fp = gf.params(threshold=255, radius=radius)
            want = gf.field(L, table[:radius * radius + 1], fp)
            m.set_likelihood(L)
            m.likelihood_field(table[:radius * radius + 1], **fp)
            _same(m.likelihood(), want, ("last row / column", radius))
            assert np.count_nonzero(want) == (min(radius + 1, height) * width if L[height - 1, 0] else min(radius + 1, width) * height)
    m.close()


@pytest.mark.parametrize("width,height", SIZES)
def test_the_frame_stays_zero(rsx, width, height):
    """dense seeds, on the borders too, at radius 64 with a table without a zero: every cell of the map is lit, and the whole buffer,
    read through likelihood_device and the pitch, is zero outside the map"""
    rng = np.random.default_rng(width)
    table = rng.integers(1, 256, 64 * 64 + 1, dtype=np.uint8)
    L = _random_plane(rng, width, height, 0.3, 50)
    L[0, :], L[-1, :], L[:, 0], L[:, -1] = 255, 255, 255, 255
    fp = gf.params(threshold=50, radius=64)
    m = _map(width, height, L)
    m.likelihood_field(table, **fp)
    whole = _framed(m, width, height)
    want = gf.field(L, table, fp)
    assert want.all()
    _same(np.ascontiguousarray(whole[128:128 + height, 128:128 + width]), want, "inside")
    whole[128:128 + height, 128:128 + width] = 0
    assert not whole.any()
    m.close()


def test_the_default_table_and_the_wrapper(rsx):
    """table NULL is the Gaussian of sigma 3 and peak 255 at the radius of params, params NULL the defaults; the wrapper's sigma and
    peak make the table that gaussian_table makes"""
    from navtech_radar_slam_amd import gridmap
    rng = np.random.default_rng(3)
    L = _random_plane(rng, 192, 128, 0.01, 50)
    m = _map(192, 128, L)
    assert rsx.lib().rsx_gridmap_likelihood_field(m.handle, None, None, None) == 0
    want = gf.field(L, gf.gaussian_table(3.0, 12), gf.params())
    _same(m.likelihood(), want, "all defaults")
    for kw, table, fp in (({}, gf.gaussian_table(3.0, 12), gf.params()), ({"radius": 5}, gf.gaussian_table(3.0, 5), gf.params(radius=5)),
                          ({"sigma": 1.5, "peak": 100, "radius": 6}, gf.gaussian_table(1.5, 6, 100), gf.params(radius=6)),
                          ({"params": gridmap.field_params(threshold=200, radius=2)}, gf.gaussian_table(3.0, 2), gf.params(threshold=200, radius=2))):
        m.set_likelihood(L)
        m.likelihood_field(**kw)
        _same(m.likelihood(), gf.field(L, table, fp), kw)
    with pytest.raises(TypeError):
        m.likelihood_field(params=gridmap.default_field_params(), radius=3)
    # the caller may free (here: overwrite) its table on return
    table = gf.gaussian_table(2.0, 7)
    mine = table.copy()
    m.set_likelihood(L)
    m.likelihood_field(mine, radius=7)
    mine[:] = 0
    _same(m.likelihood(), gf.field(L, table, gf.params(radius=7)), "the table is the handle's copy")
    m.close()


def test_ordering(rsx):
    """update_likelihood and then the field on one stream of the caller's; set_likelihood and then the field on the handle's own; and a
    field of a field, which is the restatement applied twice"""
    import torch
    imgs, T, p = gc.random_case(77, 64, 96, 192, 128, 6)
    planes = gm.add_batch(gm.zeros(p), imgs, T, p, col_offset=gc.META)
    hits = gx.likelihood(planes, 1)
    fp = gf.params(threshold=20, radius=9)
    table = gf.gaussian_table(2.5, 9)
    want = gf.field(hits, table, fp)
    assert want.any() and not want.all() and 0 < np.count_nonzero(hits >= 20) < hits.size
    m = _map(192, 128)
    m.add(imgs, T)
    stream = torch.cuda.Stream()
    for _ in range(2):
        m.update_likelihood(1, 1, stream=stream.cuda_stream)
        m.likelihood_field(table, stream=stream.cuda_stream, **fp)
        _same(m.likelihood(), want, "update, field on a caller's stream")          # (read on the handle's own stream: ordered by the library)
    m.set_likelihood(hits)
    m.likelihood_field(table, **fp)
    _same(m.likelihood(), want, "set, field on the handle's stream")
    fp2 = gf.params(threshold=150, radius=3)
    t2 = gf.gaussian_table(1.0, 3, 200)
    m.likelihood_field(t2, stream=stream.cuda_stream, **fp2)
    twice = gf.field(want, t2, fp2)
    assert twice.any() and twice.tobytes() != want.tobytes()
    _same(m.likelihood(), twice, "a field of a field")
    stream.synchronize()
    m.close()


def test_before_any_likelihood(rsx):
    """the call is refused, the wrapper raises, and nothing was marked as filled: likelihood_read still fails.  With the parameter
    rules of tests/test_gridfield_abi.py, which hold with a handle too and come first"""
    L = rsx.lib()
    m = _map(64, 64)
    abi.check_parameter_rules(rsx, m.handle)
    table = gf.gaussian_table(3.0, 12)
    for tp in (None, table.ctypes.data):
        assert L.rsx_gridmap_likelihood_field(m.handle, None, tp, None) == -1 and b"no likelihood" in L.rsx_last_error_string()
    with pytest.raises(rsx.RsxError):
        m.likelihood_field()
    with pytest.raises(rsx.RsxError):
        m.likelihood()
    m.set_likelihood(np.full((64, 64), 60, dtype=np.uint8))
    m.likelihood_field()
    assert (m.likelihood() == 255).all()
    abi.check_parameter_rules(rsx, m.handle)
    assert (m.likelihood() == 255).all()          # (a refused call touches nothing)
    m.close()


# ---- the chain: the localisers read the field like any plane ----

CHAIN_FIELD = dict(threshold=245, radius=6)      # on the uniformly random planes of tests/gridmatch_cases.py: about 4 % of the cells are seeds
PICK = [72, 45, 0, 63, 73, 36]                    # jobs of tests/gridrefine_cases.random_case: 300 and 257 points, in, on and outside the map


@functools.lru_cache(maxsize=None)
def _chain_field(seed):
    p = gc.small_params(64, 64)
    L = gxc.plane(seed, p)
    F = gf.field(L, gf.gaussian_table(2.0, CHAIN_FIELD["radius"]), gf.params(**CHAIN_FIELD))
    assert 0 < np.count_nonzero(F) < F.size and len(np.unique(F)) > 10
    return L, F


def _field_map(L):
    m = _map(64, 64, L)
    m.likelihood_field(sigma=2.0, **CHAIN_FIELD)
    return m


def test_match_on_the_field(rsx):
    _, clouds, priors, p, mp = gxc.volume_case(91, 64, 64, 1, 3, 2)
    L, F = _chain_field(92)
    m = _field_map(L)
    res, vol = m.match(clouds, priors, return_scores=True, **mp)
    wres, wvol = gxc.reference(F, clouds, priors, p, mp)
    assert wvol.any() and vol.tobytes() == wvol.tobytes() and res.tobytes() == wres.tobytes()
    m.close()


def test_search_on_the_field(rsx):
    _, clouds, priors, p, mp = gsc.volume_case(93, 64, 64, 2, 4, 3)
    L, F = _chain_field(94)
    m = _map(64, 64, L)
    m.prepare_search(4)
    m.likelihood_field(sigma=2.0, **CHAIN_FIELD)
    # the search reads its snapshot: before a new prepare that is still the raw plane
    stale = m.search(clouds, priors, **mp)
    assert stale.tobytes() == gsc.reference(L, clouds, priors, p, mp)[0].tobytes()
    m.prepare_search(4)
    res, bnd = m.search(clouds, priors, return_bounds=True, **mp)
    wres, wbnd = gsc.reference(F, clouds, priors, p, mp)
    assert wbnd.any() and bnd.tobytes() == wbnd.tobytes() and res.tobytes() == wres.tobytes() and res.tobytes() != stale.tobytes()
    m.close()


def test_refine_on_the_field(rsx):
    _, clouds, priors, p = grc.random_case(64, 64)
    clouds, priors = [clouds[i] for i in PICK], priors[PICK]
    L, F = _chain_field(95)
    m = _field_map(L)
    got = m.refine(clouds, priors)
    want = grc.reference(F, clouds, priors, p, gr.params())
    assert (want["accepted"] >= 1).any()
    for i in range(len(PICK)):
        assert got[i].tobytes() == want[i].tobytes(), (i, got[i], want[i])
    m.close()


def test_one_handle_through_the_chain(rsx):
    """match, search and refine in turn with field calls between them on one handle (the workspaces of all four live side by side):
    each equals its restatement on the plane as the restatement has transformed it so far"""
    _, clouds, priors, p = grc.random_case(64, 64)
    clouds, priors = [clouds[i] for i in PICK], priors[PICK]
    L, F1 = _chain_field(96)
    mp, sp = gxc.window(1, 3, 2), gsc.window(2, 4, 3)
    m = _field_map(L)
    assert m.match(clouds, priors, **mp).tobytes() == gxc.reference(F1, clouds, priors, p, mp)[0].tobytes()
    fp2, t2 = gf.params(threshold=150, radius=3), gf.gaussian_table(1.5, 3, 200)
    F2 = gf.field(F1, t2, fp2)
    m.likelihood_field(t2, **fp2)
    m.prepare_search(4)
    assert m.search(clouds, priors, **sp).tobytes() == gsc.reference(F2, clouds, priors, p, sp)[0].tobytes()
    fp3, t3 = gf.params(threshold=100, radius=64), gf.gaussian_table(20.0, 64)
    F3 = gf.field(F2, t3, fp3)
    m.likelihood_field(t3, **fp3)
    _same(m.likelihood(), F3, "the third field")
    assert len({F1.tobytes(), F2.tobytes(), F3.tobytes()}) == 3
    assert m.refine(clouds, priors).tobytes() == grc.reference(F3, clouds, priors, p, gr.params()).tobytes()
    assert m.match(clouds, priors, **mp).tobytes() == gxc.reference(F3, clouds, priors, p, mp)[0].tobytes()
    m.close()
