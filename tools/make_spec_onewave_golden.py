"""Records tests/golden/sc_spec_onewave_bounds.npz: the bounds of the one-wave-per-SIMD mapping of the spectral
filter, on the fixture of tests/test_gpu_sc_spec.py test_two_wave_mapping_gives_the_same_bounds (4096 + 77 entries,
203 queries, binary and continuous descriptors, fixed seeds).

Recorded ONCE, on an MI355X, from the build of commit 8bd21ee ("Add CA-CFAR / BFAR keypoint extraction and select it in the
odometry") -- the last commit that has the one-wave kernel.  The commit after it deletes that kernel, and the test holds
sc_spec2_filter_kernel to this recording bit for bit.  It cannot be re-recorded from a later build: there filter_kind =
KIND_SPECTRAL selects the two-wave kernel and the kernel-name assertion below fails.  To record again, check out 8bd21ee,
build it, and run this file from the later tree against that build.

Per variant the file keeps the SHA-256 of the uint32 view of the float32 bound matrix [203][4173], one CRC32 per query row,
and the bit patterns of entry columns [0, 128) and [4096, 4173) (the first tile-block and the ragged end).

Run on the GPU machine, from the repository root, with that commit's librsx.so:
    python tools/make_spec_onewave_golden.py [output.npz]
"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
RECORDED_FROM = "8bd21ee"


def main():
    from navtech_radar_slam_amd import _rsx, scancontext as sc, synth
    spec = importlib.util.spec_from_file_location("sc_spec_tests", os.path.join(ROOT, "tests", "test_gpu_sc_spec.py"))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    out = {"recorded_from": np.array(RECORDED_FROM), "cols": t.ONE_WAVE_COLS.astype(np.int32)}
    for binary in (True, False):
        descs, queries = t.one_wave_fixture(synth, binary)
        a = sc.SCManager(filter_kind=_rsx.KIND_SPECTRAL, capacity_hint=len(descs))
        b = sc.SCManager(filter_kind=_rsx.KIND_SPECTRAL2, capacity_hint=len(descs))
        try:
            a.add_descriptors_f32(descs)
            b.add_descriptors_f32(descs)
            la = a.filter_bounds(queries)
            assert a.profiled_kernel_name() == "sc_spec_filter_kernel", a.profiled_kernel_name()
            assert np.array_equal(la.view(np.uint32), a.filter_bounds(queries).view(np.uint32)), "the build does not repeat itself"
            lb2 = b.filter_bounds(queries)
            assert b.profiled_kernel_name() == "sc_spec2_filter_kernel", b.profiled_kernel_name()
            assert np.array_equal(la.view(np.uint32), lb2.view(np.uint32)), "the two mappings differ at this commit"
        finally:
            a.close()
            b.close()
        assert la.shape == (len(queries), len(descs)) and la.dtype == np.float32
        tag = "binary" if binary else "continuous"
        sha, crc, cols = t.bound_digest(la)
        out["sha256_" + tag], out["crc32_" + tag], out["cols_" + tag] = np.array(sha), crc, cols
        print(tag, la.shape, "sha256", sha, int(np.isinf(la).sum()), "inf,", int(np.isnan(la).sum()), "NaN,",
              len(np.unique(la.view(np.uint32))), "distinct values")
    path = sys.argv[1] if len(sys.argv) > 1 else t.ONE_WAVE_GOLDEN
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
