"""Records tests/golden/sc_rescore_rank_stats.npz: rsx_sc_rescoring_stats of the two fixed-seed fixtures of
tests/test_gpu_sc_rescore_rank.py (pin_fixture), for the whole batch and for every query on its own.

Recorded ONCE, on an MI355X, from the build of commit bbb4c13 ("Add CorAl alignment quality for cloud pairs; report it in
pgo_replay") -- the last commit whose sc_rescore_wave_kernel finds the next survivor of a round with a wave-wide minimum.  The
commit after it ranks the survivors once; the order of the evaluations is meant to be the same, and the test holds the
counters of the later builds to this recording field by field.  To record again, check out bbb4c13, build it, and run this
file from the later tree against that build (RSX_LIB_PATH names the library).

Run on the GPU machine, from the repository root:
    python tools/make_rescore_rank_golden.py [output.npz]
"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
RECORDED_FROM = "bbb4c13"


def main():
    from navtech_radar_slam_amd import scancontext as sc
    spec = importlib.util.spec_from_file_location("sc_rescore_rank_tests", os.path.join(ROOT, "tests", "test_gpu_sc_rescore_rank.py"))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    out = {"recorded_from": np.array(RECORDED_FROM), "fields": np.array(t.STAT_FIELDS)}
    for which in (0, 1):
        descs, queries, k, n_elig = t.pin_fixture(which)
        m = sc.SCManager(filter_mode=t.FORCE)
        try:
            m.add_descriptors_f32(descs)
            st = t.rescoring_stats(m, queries, k, n_elig)
            for _ in range(3):
                assert np.array_equal(st, t.rescoring_stats(m, queries, k, n_elig)), "the build does not repeat itself"
        finally:
            m.close()
        out["stats_%d" % which] = st
        print("fixture", which, descs.shape, queries.shape, "k", k, "n_eligible", n_elig)
        print("  batch", dict(zip(t.STAT_FIELDS, st[0].tolist())))
        print("  candidates per query", st[1:, 0].tolist())
        print("  exact evaluations per query", st[1:, 1].tolist())
    path = sys.argv[1] if len(sys.argv) > 1 else t.GOLDEN
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
