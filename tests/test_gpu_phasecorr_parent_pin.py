"""The stand-alone entries rsx_phasecorr_register_batch[_device] against bytes RECORDED from the parent build.

Since the odometry switch, the two stages of a batch (spectra of the scans, registration of the pairs) are internal launch
functions on caller-owned buffers, which the windowed pipeline calls on its own sets, and the stand-alone entries are those two
calls in a row on the handle's workspace.  The pin is tests/golden/phasecorr_parent.npz: the raw 56-byte rsx_phasecorr_result
records that the last build whose run() owned all nine launches (commit 4976d40) returned for the SEVEN pairs of
synth.polar_sequence(3, 6) at N = 64 / 2.0 m and at N = 256 / 0.5 m, recorded once on an MI355X by
tools/make_phasecorr_parent_golden.py.  Both entries must return those bytes.  The scans' bytes are hashed and compared first, so
that a moved generator is not mistaken for a moved kernel."""
import hashlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "phasecorr_parent.npz")
ROWS, COLS = 400, 3360
SEVEN = [(1, 0), (2, 1), (3, 2), (4, 3), (5, 4), (2, 0), (0, 0)]   # the pairs of tests/test_gpu_phasecorr.py
GROUPS = (dict(n=64, resolution=2.0), dict(n=256, resolution=0.5))


def scans():
    from navtech_radar_slam_amd import synth
    return np.ascontiguousarray(synth.polar_sequence(3, 6)[0]), synth.OXFORD_META


def input_hash(imgs):
    h = hashlib.sha256()
    h.update(repr((imgs.shape, SEVEN, [sorted(g.items()) for g in GROUPS])).encode())
    h.update(imgs.tobytes())
    return h.hexdigest()


def measure(imgs, off):
    """-> per group of GROUPS the (7,) result records of the host entry"""
    from navtech_radar_slam_amd import phasecorr
    out = []
    for fields in GROUPS:
        h = phasecorr.Phasecorr(ROWS, COLS, phasecorr.params(**fields))
        out.append(h.register_batch(imgs, SEVEN, col_offset=off))
        h.close()
    return out


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_host_and_device_entries_return_the_parent_bytes(golden):
    import torch
    from navtech_radar_slam_amd import _rsx, phasecorr
    imgs, off = scans()
    assert str(golden["input_sha256"]) == input_hash(imgs)
    assert int(golden["n_groups"]) == len(GROUPS)
    got = measure(imgs, off)
    d_imgs = torch.from_numpy(imgs).cuda()
    d_pairs = torch.tensor(SEVEN, dtype=torch.int32, device="cuda")
    for g, fields in enumerate(GROUPS):
        want = golden[f"results_{g}"].tobytes()
        assert len(want) == 56 * len(SEVEN)
        rec = np.frombuffer(want, dtype=_rsx.PHASECORR_RESULT_DTYPE)
        assert not rec["status"].any() and len({r.tobytes() for r in rec}) == len(SEVEN)   # the file holds seven distinct results
        for p, r, w in zip(SEVEN, got[g], rec):
            assert r.tobytes() == w.tobytes(), ("host entry", fields, p, r, w)
        h = phasecorr.Phasecorr(ROWS, COLS, phasecorr.params(**fields))
        d_res = torch.full((len(SEVEN) * 56,), 99, dtype=torch.uint8, device="cuda")
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        h.register_batch_device(d_imgs.data_ptr(), len(imgs), imgs.strides[0], imgs.strides[1], off, d_pairs.data_ptr(), len(SEVEN),
                                d_res.data_ptr(), stream=s.cuda_stream)
        torch.cuda.synchronize()
        assert d_res.cpu().numpy().tobytes() == want, ("device entry", fields)
        h.close()
