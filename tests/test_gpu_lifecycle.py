"""Handle lifecycles on the device: every handle type created, used until its buffers have grown and destroyed, over and
over.  Each handle owns its device memory, pinned memory, streams and events through the owning types of rsx_common.h;
if one of them leaked, the device's free memory would fall cycle after cycle.  Also: a create on a device past the last
one fails with RSX_ERR_NO_DEVICE and leaves the handle null."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CYCLES = 20
# Device memory that may come and go between the first and the last cycle without a leak on our side.  Measured on the parent
# commit (after the warm-up below): 0 bytes for every handle type.  Without the warm-up the free memory drops once by 40 MiB
# during the second ScanContext cycle of the process and stays flat afterwards (the runtime's own, the same on the parent).
TOLERANCE = 4 << 20


@pytest.fixture(scope="module")
def inputs():
    from navtech_radar_slam_amd import _rsx, synth
    assert _rsx.device_count() >= 1
    clouds, _ = synth.keyframe_clouds(21, 40, binary_z=False, n_points=600)
    descs = synth.random_descriptors(22, 1500, binary=True)
    imgs, az, _, _ = synth.polar_sequence(23, 5)
    src, dst, off, _ = synth.orora_pairs(24, 6, k_range=(200, 2600))
    return {"clouds": clouds, "descs": descs, "imgs": imgs, "az": az, "src": src, "dst": dst, "off": off}


def use_sc(d):
    from navtech_radar_slam_amd import scancontext
    g = scancontext.SCManager(capacity_hint=64)
    g.profile_enable(True)                      # the profiler's events
    for c in d["clouds"][:12]:                   # the insert slots' pinned staging and events
        g.makeAndSaveScancontextAndKeys(c)
        g.detectLoopClosureID()
    g.add_descriptors_f32(d["descs"])            # the database grows past its capacity hint
    g.query(d["descs"][:1], k=5)                 # pinned results
    g.query(np.concatenate([d["descs"], d["descs"]])[:2048], k=10)  # in pieces: the upload stream, the second lane, their events
    g.close()


def use_scs(d):
    from navtech_radar_slam_amd import scancontext
    s = scancontext.ShardedSet([0], capacity_hint=64)
    s.add_descriptors_f32(d["descs"])
    s.query(d["descs"][:64], k=10)
    s.close()


def use_cen2019(d):
    from navtech_radar_slam_amd import cen2019
    c = cen2019.Cen2019()
    c.extract(d["imgs"][0], azimuths=d["az"][0])       # single-scan entry: pinned read-back
    c.extract(d["imgs"][1], azimuths=d["az"][1], max_targets=400000)
    c.extract_batch(d["imgs"])
    c.close()


def use_frontend(d):
    from navtech_radar_slam_amd import frontend, synth
    f = frontend.Frontend()
    f.cartesian(d["imgs"][0], d["az"][0], synth.RADAR_RESOLUTION)
    rng = np.random.default_rng(0)
    descs = [f.describe(rng.uniform(-100, 100, (n, 2)).astype(np.float32)) for n in (300, 1200)]
    f.match(descs[0][0], descs[0][1], descs[1][0], descs[1][1], 0.8)
    f.close()


def use_orora(d):
    from navtech_radar_slam_amd import orora
    o = orora.Orora()
    o.register_batch(d["src"], d["dst"], d["off"])      # pairs above 2048 matches: the big-pair workspaces
    o.max_clique_batch(d["src"], d["dst"], d["off"])    # the selection's workspaces
    o.close()


def use_voxelgrid(d):
    from navtech_radar_slam_amd import voxelgrid
    v = voxelgrid.VoxelGrid()
    for n in (1, 5, 40):
        v.filter(np.concatenate(d["clouds"][:n]))
    v.close()


def use_icp(d):
    from navtech_radar_slam_amd import icp
    i = icp.Icp()
    i.align(d["clouds"][0][:, :3], d["clouds"][0][:, :3])
    i.align(np.concatenate(d["clouds"][:4])[:, :3], np.concatenate(d["clouds"][1:5])[:, :3])
    i.close()


def use_kfstore(d):
    from navtech_radar_slam_amd import loopverify
    k = loopverify.KeyframeStore()
    for c in d["clouds"]:
        k.add(c)
    k.submap(20, 5, np.zeros(6))
    k.verify(2, 30, np.zeros(6))
    k.close()


def use_odometry(d):
    from navtech_radar_slam_amd import odometry
    o = odometry.Odometry(400, 3360)
    o.push(d["imgs"][:2], d["az"][:2])
    o.push(d["imgs"][2:], d["az"][2:])
    o.close()


USES = {"sc": use_sc, "scs": use_scs, "cen2019": use_cen2019, "frontend": use_frontend, "orora": use_orora,
        "voxelgrid": use_voxelgrid, "icp": use_icp, "kfstore": use_kfstore, "odometry": use_odometry}


def test_create_use_destroy_leaves_device_memory_as_it_was(inputs):
    import torch
    for use in USES.values():  # warm-up: the runtime's one-time allocations
        use(inputs)
        use(inputs)
    drift = {}
    for name, use in USES.items():
        for cycle in range(CYCLES):
            use(inputs)
            torch.cuda.synchronize()
            free, _ = torch.cuda.mem_get_info(0)
            if cycle == 0:
                first = free
        drift[name] = first - free  # > 0: less free memory after the last cycle than after the first
    print("device memory lost between cycle 1 and cycle %d (bytes):" % CYCLES, drift)
    assert all(abs(v) <= TOLERANCE for v in drift.values()), drift


def test_create_on_a_device_past_the_last_fails(inputs):
    from navtech_radar_slam_amd import _rsx
    L = _rsx.lib()
    n = _rsx.device_count()
    h = C.c_void_p()
    sp = _rsx.ScParams()
    L.rsx_sc_default_params(C.byref(sp))
    sp.device = n
    op = _rsx.OdometryParams()
    L.rsx_odometry_default_params(C.byref(op))
    op.device = n
    devs = (C.c_int32 * 1)(n)
    for name, create in (("sc", lambda: L.rsx_sc_create(C.byref(sp), C.byref(h))),
                         ("scs", lambda: L.rsx_scs_create(None, devs, 1, C.byref(h))),
                         ("orora", lambda: L.rsx_orora_create(n, C.byref(h))),
                         ("cen2019", lambda: L.rsx_cen2019_create(n, 400, 3360, C.byref(h))),
                         ("frontend", lambda: L.rsx_frontend_create(n, 400, 3360, None, C.byref(h))),
                         ("voxelgrid", lambda: L.rsx_voxelgrid_create(n, C.byref(h))),
                         ("icp", lambda: L.rsx_icp_create(n, C.byref(h))),
                         ("kfstore", lambda: L.rsx_kfstore_create(n, C.byref(h))),
                         ("odometry", lambda: L.rsx_odometry_create(C.byref(op), 400, 3360, C.byref(h)))):
        h.value = 1
        assert create() == -2 and not h.value, name
        assert b"out of range" in L.rsx_last_error_string(), name
