"""Records tests/golden/sc_spec_bounds_parent.npz: the spectral filter's fp16 bound matrix and the records of the fixture of
tests/test_gpu_sc_spectra_pin.py (64 queries x 96 entries, fixed seeds).

Recorded ONCE, on an MI355X, from the build of commit 0d1e445 ("Add CFEAR scan-to-keyframes registration and a device-side
tracker") -- the last commit whose spectra_of evaluates the 15 twiddle factors in every wavefront and stages the normalised
image as doubles in LDS.  Later builds must reproduce both arrays bit for bit (that is the test); re-recording from a later
build would make the test compare a build with itself, so do that only when a change is MEANT to move the bounds, and name
the new commit here.

Run on the GPU machine, from the repository root, with that commit's librsx.so:
    python tools/make_spec_bounds_golden.py [output.npz]
"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RECORDED_FROM = "0d1e445"


def main():
    from navtech_radar_slam_amd import scancontext as sc
    spec = importlib.util.spec_from_file_location("spectra_pin", os.path.join(ROOT, "tests", "test_gpu_sc_spectra_pin.py"))
    pin = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pin)
    bits, rec = pin.measure(sc)
    again, rec2 = pin.measure(sc)
    assert np.array_equal(bits, again) and np.array_equal(rec, rec2), "the build does not repeat itself"
    path = sys.argv[1] if len(sys.argv) > 1 else pin.GOLDEN
    np.savez_compressed(path, bound_bits=bits, dist=rec["dist"], index=rec["index"], shift=rec["shift"],
                        recorded_from=np.array(RECORDED_FROM))
    h = bits.view(np.float16)
    print("wrote", path, os.path.getsize(path), "bytes;", int(np.isnan(h).sum()), "NaN bounds,", len(np.unique(bits)), "distinct values")


if __name__ == "__main__":
    main()
