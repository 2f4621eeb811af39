"""Records tests/golden/cfear_pairs_parent.npz: the raw rsx_cfear_result records of rsx_cfear_register_batch for the 13 pairs
of tests/cfear_track_cases.pair_cases(), per parameter group, with a SHA-256 of the inputs.

Recorded ONCE, on an MI355X, from the build of commit a46f554 ("Build window-stage query images in the window kernel, slim the
spectra") -- the last commit whose pair entries run a kernel of their own (cfear_register_kernel: brute-force search, one
workgroup per pair).  Later builds register pairs through the joint kernel and must reproduce these bytes (that is
tests/test_gpu_cfear_pair_pin.py); re-recording from a later build would make the test compare a build with itself, so do that
only when a change is MEANT to move the registration's bytes, and name the new commit here.

Run on the GPU machine, from the repository root, with that commit's librsx.so:
    python tools/make_cfear_pairs_golden.py [output.npz]
"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RECORDED_FROM = "a46f554"


def main():
    from navtech_radar_slam_amd import cfear
    spec = importlib.util.spec_from_file_location("cfear_pair_pin", os.path.join(ROOT, "tests", "test_gpu_cfear_pair_pin.py"))
    pin = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pin)
    h = cfear.Cfear()
    first, again = pin.measure(h), pin.measure(h)
    h.close()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again)), "the build does not repeat itself"
    groups = pin.cases.pair_groups()
    for (key, cs, _), r in zip(groups, first):
        assert [int(x["status"]) for x in r] == [c[5] for c in cs], (key, r)
    path = sys.argv[1] if len(sys.argv) > 1 else pin.GOLDEN
    np.savez_compressed(path, n_groups=np.array(len(groups)), input_sha256=np.array(pin.input_hash()), recorded_from=np.array(RECORDED_FROM),
                        **{f"results_{g}": np.frombuffer(r.tobytes(), dtype=np.uint8) for g, r in enumerate(first)})
    print("wrote", path, os.path.getsize(path), "bytes;", sum(len(r) for r in first), "results in", len(groups), "groups; inputs", pin.input_hash())


if __name__ == "__main__":
    main()
