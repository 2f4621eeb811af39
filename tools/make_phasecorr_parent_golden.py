"""Records tests/golden/phasecorr_parent.npz: the raw rsx_phasecorr_result records of rsx_phasecorr_register_batch for the SEVEN
pairs of synth.polar_sequence(3, 6) at N = 64 / 2.0 m and at N = 256 / 0.5 m, with a SHA-256 of the inputs.

Recorded ONCE, on an MI355X, from the build of commit 4976d40 ("Add phase-correlation (Fourier-Mellin) registration of polar
scans") -- the last commit whose run() owned all nine launches on the handle's own workspace.  Later builds run the two stages
through rsx::phasecorr::launch_spectra / launch_pairs on caller-given buffers and must reproduce these bytes (that is
tests/test_gpu_phasecorr_parent_pin.py); re-recording from a later build would make the test compare a build with itself, so do
that only when a change is MEANT to move the registration's bytes, and name the new commit here.

Run on the GPU machine, from the repository root, with that commit's librsx.so:
    python tools/make_phasecorr_parent_golden.py [output.npz]
"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RECORDED_FROM = "4976d40"


def main():
    spec = importlib.util.spec_from_file_location("phasecorr_parent_pin", os.path.join(ROOT, "tests", "test_gpu_phasecorr_parent_pin.py"))
    pin = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pin)
    imgs, off = pin.scans()
    first, again = pin.measure(imgs, off), pin.measure(imgs, off)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again)), "the build does not repeat itself"
    for r in first:
        assert not r["status"].any() and len({x.tobytes() for x in r}) == len(pin.SEVEN), r
    path = sys.argv[1] if len(sys.argv) > 1 else pin.GOLDEN
    np.savez_compressed(path, n_groups=np.array(len(first)), input_sha256=np.array(pin.input_hash(imgs)), recorded_from=np.array(RECORDED_FROM),
                        **{f"results_{g}": np.frombuffer(r.tobytes(), dtype=np.uint8) for g, r in enumerate(first)})
    print("wrote", path, os.path.getsize(path), "bytes;", sum(len(r) for r in first), "results in", len(first), "groups; inputs", pin.input_hash(imgs))
    for fields, r in zip(pin.GROUPS, first):
        print(fields, r)


if __name__ == "__main__":
    main()
