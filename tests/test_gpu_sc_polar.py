"""Radar scan contexts as a place-recognition database on the GPU: rsx_sc_add_polar_batch_device / rsx_sc_add_polar build the
descriptors of polar scans (csrc/radarsc.hip) and insert them without a host hop; the stored descriptors equal the restatement
(tests/radarsc_np.py, PARITY with MulRan's builder UNPINNED) bit for bit, and the rotated revisits of tests/radarsc_cases.py,
queried through rsx_sc_query_device, give the records of the oracle's exhaustive search on the restatement's descriptors."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import radarsc_cases as cases  # noqa: E402
import radarsc_np as rc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    from navtech_radar_slam_amd import _rsx, radar_context, scancontext
    assert _rsx.device_count() >= 1, "no HIP device: GPU tests must run on the MI355X box"
    db, q, az = cases.scans()
    allscans = np.concatenate([db, q])
    e = dict(sc=scancontext, ctx=radar_context.RadarContext(400, 3360), imgs=allscans, az=az, want=rc.build_batch(allscans, az),
             d_imgs=torch.from_numpy(allscans).cuda(), d_az=torch.from_numpy(np.array(az)).cuda())
    torch.cuda.synchronize()
    return e


def add_all(env, manager, stream=0):
    imgs = env["imgs"]
    manager.add_polar_batch_device(env["ctx"], env["d_imgs"].data_ptr(), len(imgs), imgs.shape[1] * imgs.shape[2], imgs.shape[2],
                                   env["d_az"].data_ptr(), stream=stream)


def test_database_equals_restatement(env):
    import torch
    g = env["sc"].SCManager()
    add_all(env, g, stream=torch.cuda.current_stream().cuda_stream)
    assert len(g) == cases.N_DB + 4 and g.local_size == cases.N_DB + 4
    assert g.export_descriptors_f32().tobytes() == env["want"].tobytes()
    # the host single-scan form appends the same descriptor
    idx = g.add_polar(env["ctx"], env["imgs"][7], env["az"])
    assert idx == cases.N_DB + 4 and g.export_descriptors_f32(idx, 1).tobytes() == env["want"][7].tobytes()


@pytest.mark.parametrize("filter_mode", [0, 1, 2, 3])
def test_revisits_through_query_device(env, oracle, filter_mode):
    import torch
    g = env["sc"].SCManager(filter_mode=filter_mode)
    add_all(env, g)
    k, nq, n = 3, 4, cases.N_DB
    m = oracle.Manager()
    m.add_descriptors(env["want"].astype(np.float64))
    want = m.exhaustive_batch(env["want"][n:].astype(np.float64), n_eligible=n, k=k)
    # the queries are the descriptors the database itself holds for the revisits: nothing leaves the GPU before the records
    dq = torch.from_numpy(g.export_descriptors_f32(n, nq)).cuda()
    out = torch.zeros((nq, k, 2), dtype=torch.float64, device="cuda")
    g.query_device(dq.data_ptr(), nq, k, out.data_ptr(), n_eligible=n, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(env["sc"].HIT_DTYPE).reshape(nq, k)
    assert got.tobytes() == want.astype(env["sc"].HIT_DTYPE).tobytes(), (got, want)
    cases.check_ranking(got)


def test_sharded_pair_keeps_residue_classes(env):
    shards = [env["sc"].SCManager(shard_rank=r, shard_world=2) for r in range(2)]
    for r, s in enumerate(shards):
        add_all(env, s)
        assert len(s) == cases.N_DB + 4 and s.local_size == (cases.N_DB + 4) // 2
        assert s.export_descriptors_f32().tobytes() == env["want"][r::2].tobytes()
        assert s.add_polar(env["ctx"], env["imgs"][3], env["az"]) == cases.N_DB + 4    # index 44 belongs to rank 0
        assert s.local_size == (cases.N_DB + 4) // 2 + (1 if r == 0 else 0)
    assert shards[0].export_descriptors_f32(22, 1).tobytes() == env["want"][3].tobytes()


def test_save_load_round_trip(env, tmp_path):
    g = env["sc"].SCManager()
    add_all(env, g)
    path = str(tmp_path / "radar_context.scdb")
    g.save(path)
    h = env["sc"].SCManager()
    assert h.load(path) == cases.N_DB + 4
    assert h.export_descriptors_f32().tobytes() == env["want"].tobytes()
    q = env["want"][cases.N_DB:]
    assert h.query(q, k=3, n_eligible=cases.N_DB).tobytes() == g.query(q, k=3, n_eligible=cases.N_DB).tobytes()


def test_handles_and_arguments(env):
    from navtech_radar_slam_amd import _rsx
    L = _rsx.lib()
    g = env["sc"].SCManager()
    imgs = env["imgs"]
    args = (env["d_imgs"].data_ptr(), 2, imgs.shape[1] * imgs.shape[2], imgs.shape[2], 11, env["d_az"].data_ptr(), 0, None)
    assert L.rsx_sc_add_polar_batch_device(g._h, None, *args) == -1
    assert L.rsx_sc_add_polar_batch_device(None, env["ctx"]._h, *args) == -1
    assert L.rsx_sc_add_polar_batch_device(g._h, env["ctx"]._h, None, *args[1:]) == -1
    assert L.rsx_sc_add_polar_batch_device(g._h, env["ctx"]._h, args[0], 2, args[2], 3360, *args[4:]) == -1   # row_stride < 11 + cols
    assert L.rsx_sc_add_polar(g._h, env["ctx"]._h, None, imgs.shape[2], 11, env["az"].ctypes.data, None) == -1
    assert len(g) == 0
    assert L.rsx_sc_add_polar_batch_device(g._h, env["ctx"]._h, args[0], 0, *args[2:]) == 0 and len(g) == 0
