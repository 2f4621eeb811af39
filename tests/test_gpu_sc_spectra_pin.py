"""The spectral filter's images, pinned bit for bit (csrc/sc_spec.hip spectra_of: sc_spec_query_kernel for the queries,
sc_spec_db_kernel for the database).  The oracle comparison of the other files forgives a bound that moves by an ulp as long
as the records stay right; this one does not: tests/golden/sc_spec_bounds_parent.npz holds the filter's fp16 bound matrix
(every query against every entry, from the diagnostic bounds entry) and the records of one fixed fixture, recorded on the GPU
from the build of the commit named in tools/make_spec_bounds_golden.py, and the build under test must give the same bits.
The fp64 spectra are rounded to fp16 and pass through two MFMA stages before they become a bound, so a one-ulp change of a
twiddle factor or of a normalised element shows wherever it crosses an fp16 rounding boundary in the 64 x 96 x 1216 spectrum
values; the fixture's empty columns and non-finite elements pin the mask and the flags."""
import os

import numpy as np
import pytest

from navtech_radar_slam_amd import synth

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sc_spec_bounds_parent.npz")
NQ, NDB, K, FORCE = 64, 96, 10, 2


def make_fixture():
    """(descs [96][1200], queries [64][1200]) float32 from fixed seeds: continuous and binary descriptors, rotated copies,
    empty columns on both sides, an all-zero entry and query, NaN / inf elements on both sides"""
    descs = synth.random_descriptors(901, NDB, binary=False)
    descs[48:72] = synth.random_descriptors(902, 24, binary=True)
    rng = np.random.default_rng(903)
    for i in range(0, NDB, 6):
        descs[i] = synth.rotate_descriptor(descs[int(rng.integers(0, NDB))], int(rng.integers(0, 60)))
    descs[5] = 0
    descs[6].reshape(60, 20)[7:9] = 0
    descs[17].reshape(60, 20)[rng.uniform(size=60) < 0.5] = 0
    descs[90, 123] = np.nan
    descs[91, 777] = np.inf
    queries = synth.random_descriptors(904, NQ, binary=False)
    for i in range(0, NQ, 2):
        queries[i] = synth.rotate_descriptor(descs[int(rng.integers(0, NDB))], int(rng.integers(0, 60)))
    queries[3].reshape(60, 20)[11] = 0
    queries[8].reshape(60, 20)[rng.uniform(size=60) < 0.3] = 0
    queries[9].reshape(60, 20)[:59] = 0
    queries[20] = 0
    queries[33, 5] = np.nan
    queries[34, 1199] = np.inf
    queries[35, 400] = -np.inf
    return np.ascontiguousarray(descs, dtype=np.float32), np.ascontiguousarray(queries, dtype=np.float32)


def measure(sc):
    """(bounds as fp16 bit patterns [64][96] uint16, records [64][10]) of the fixture through the spectral filter"""
    descs, queries = make_fixture()
    g = sc.SCManager(filter_mode=FORCE)
    try:
        g.add_descriptors_f32(descs)
        lb = g.filter_bounds(queries)
        assert g.profiled_kernel_name() == "sc_spec2_filter_kernel", g.profiled_kernel_name()
        rec = g.query(queries, k=K)
    finally:
        g.close()
    assert lb.shape == (NQ, NDB) and lb.dtype == np.float32
    h = lb.astype(np.float16)
    same = (h.astype(np.float32) == lb) | (np.isnan(lb) & np.isnan(h))
    assert same.all(), "the bounds entry hands out fp16 values"
    return h.view(np.uint16).copy(), rec


def test_bounds_and_records_are_the_parents(oracle):
    from navtech_radar_slam_amd import _rsx, scancontext as sc
    assert _rsx.device_count() >= 1, "no HIP device: GPU tests must run on the MI355X box"
    gold = np.load(GOLDEN)
    bits, rec = measure(sc)
    nan = np.isnan(bits.view(np.float16))
    assert np.array_equal(nan, np.isnan(gold["bound_bits"].view(np.float16)))
    diff = np.argwhere((bits != gold["bound_bits"]) & ~nan)
    assert len(diff) == 0, f"{len(diff)} bounds differ from the recorded build, first (query, entry) {diff[:4].tolist()}"
    assert np.array_equal(bits, gold["bound_bits"])
    for f in ("dist", "index", "shift"):
        assert np.array_equal(rec[f], gold[f]), f
    # and the records are right, not only unchanged
    descs, queries = make_fixture()
    o = oracle.Manager()
    o.add_descriptors(descs.astype(np.float64))
    want = o.exhaustive_batch(queries.astype(np.float64), n_eligible=NDB, k=K, nthreads=4)
    assert np.array_equal(rec, want)
