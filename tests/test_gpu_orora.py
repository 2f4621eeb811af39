"""GPU parity of ORORA registration (orora.hip through the C-ABI) against the CPU oracle.
Tolerance (north_star): pose within 1e-4 of the oracle (reductions run in a different order on the
GPU, so this is a tolerance test, not a bit-exact one)."""
import numpy as np
import pytest

from navtech_radar_slam_amd import synth

pytestmark = pytest.mark.gpu
POSE_TOL = 1e-4


@pytest.fixture(scope="module")
def reg():
    from navtech_radar_slam_amd import orora, _rsx
    assert _rsx.device_count() >= 1
    return orora.Orora()


def _check(got, want):
    assert np.array_equal(got["status"], want["status"])
    ok = want["status"] == 0
    for f in ("x", "y", "yaw"):
        assert np.abs(got[f][ok] - want[f][ok]).max() < POSE_TOL, f
    assert np.array_equal(got["iterations"], want["iterations"])
    # inlier counts are thresholded quantities (TIM weight >= 0.5; |v - t| <= beta): the GPU sums in another order, poses agree
    # to ~4e-15, so a count could only differ for a weight / residual within ~1e-14 of its threshold.  The kernels' reduction
    # orders are fixed, so the outcome on given data is deterministic: on these data sets the counts are EQUAL (rounds 1-2
    # allowed +-1 here without saying why)
    assert np.array_equal(got["rot_inliers"], want["rot_inliers"])
    assert np.array_equal(got["trans_inliers"], want["trans_inliers"])


def test_batch_matches_oracle(reg, oracle):
    src, dst, off, truth = synth.orora_pairs(777, 300)
    got = reg.register_batch(src, dst, off)
    want = oracle.orora_register_batch(src, dst, off, nthreads=8)
    _check(got, want)
    assert np.abs(got["x"] - truth[:, 0]).max() < 0.05 and np.abs(got["yaw"] - truth[:, 2]).max() < 2e-3


def test_edge_sizes(reg, oracle):
    from navtech_radar_slam_amd import orora
    maxk = orora.max_correspondences()
    assert maxk == 16384
    # <= 2048 matches: on-chip kernel; 2049 .. 16384 (cen2019 can emit 10 000 keypoints): the HBM-workspace kernel
    sizes = [0, 1, 2, 3, 5, 255, 256, 257, 511, 512, 1024, 2048, 2049, 3000, 10000, maxk, maxk + 1]
    rng = np.random.default_rng(5)
    src, dst, off = [], [], [0]
    for k in sizes:
        s = rng.uniform(-80, 80, (k, 2))
        d = s @ np.array([[np.cos(0.05), np.sin(0.05)], [-np.sin(0.05), np.cos(0.05)]]) + [0.5, 0.25]
        d += rng.normal(0, 0.03, d.shape)
        if k > 10:
            d[: k // 3] = rng.uniform(-80, 80, (k // 3, 2))
        src.append(s); dst.append(d); off.append(off[-1] + k)
    src = np.concatenate(src).astype(np.float32)
    dst = np.concatenate(dst).astype(np.float32)
    off = np.array(off, dtype=np.int64)
    got = reg.register_batch(src, dst, off)
    want = oracle.orora_register_batch(src, dst, off)
    assert list(got["status"][:2]) == [1, 1] and got["status"][-1] == 2   # too few / too many matches
    want["status"][-1] = 2                                                  # the oracle has no size cap
    for f in ("x", "y", "yaw", "iterations", "rot_inliers", "trans_inliers"):
        want[f][-1] = 0
    _check(got, want)


def test_clean_and_all_outlier_pairs(reg, oracle):
    rng = np.random.default_rng(9)
    s = rng.uniform(-50, 50, (400, 2)).astype(np.float32)
    c, sn = np.cos(-0.15), np.sin(-0.15)
    clean = (s.astype(np.float64) @ np.array([[c, sn], [-sn, c]]) + [-1.5, 2.0]).astype(np.float32)
    junk = rng.uniform(-50, 50, (400, 2)).astype(np.float32)
    src = np.concatenate([s, s]); dst = np.concatenate([clean, junk]); off = np.array([0, 400, 800])
    got = reg.register_batch(src, dst, off)
    want = oracle.orora_register_batch(src, dst, off)
    assert got["iterations"][0] == 1 and abs(got["yaw"][0] + 0.15) < 1e-5
    assert got["status"][1] == 0                                            # garbage in, finite pose out
    _check(got[:1], want[:1])
    assert np.all(np.isfinite([got["x"][1], got["y"][1], got["yaw"][1]]))


@pytest.mark.parametrize("flags", [1, 2, 3])
def test_modelling_switches_match_oracle(reg, oracle, flags):
    """The two unpinned modelling choices as parameters: TIMs on the complete graph (flag 1) and TEASER++'s form of the
    scalar TLS cost (flag 2); GPU == oracle within the pose tolerance for every combination, small and large pairs."""
    from navtech_radar_slam_amd import orora
    src, dst, off, truth = synth.orora_pairs(91, 24, k_range=(40, 400))
    big = synth.orora_pairs(92, 1, k_range=(2300, 2300))
    src = np.concatenate([src, big[0]]); dst = np.concatenate([dst, big[1]])
    off = np.concatenate([off, [off[-1] + 2300]]); truth = np.concatenate([truth, big[3]])
    gp, op = orora.default_params(), oracle.orora_default_params()
    gp.flags = flags
    op.flags = flags
    got = reg.register_batch(src, dst, off, gp)
    want = oracle.orora_register_batch(src, dst, off, op, nthreads=8)
    _check(got, want)
    assert np.abs(got["yaw"] - truth[:, 2]).max() < 3e-3 and np.abs(got["x"] - truth[:, 0]).max() < 0.08


# ---------------------------------------------------------------------------------------------------------------------
# the device entry (what bench.py and the odometry pipeline call), solver parity beyond the defaults, bad arguments,
# and the one-handle, many-streams contract of include/rsx.h
# ---------------------------------------------------------------------------------------------------------------------
import ctypes as C  # noqa: E402
import os  # noqa: E402
import sys  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import orora_cases  # noqa: E402

SENTINEL = 0xA5
_max_pose_diff = [0.0]


def _note_pose_diff(name, got, want):
    ok = want["status"] == 0
    d = max(float(np.abs(got[f][ok] - want[f][ok]).max()) for f in ("x", "y", "yaw")) if ok.any() else 0.0
    _max_pose_diff[0] = max(_max_pose_diff[0], d)
    print(f"[orora parity] {name}: largest pose difference {d:.3e} (largest so far {_max_pose_diff[0]:.3e})")


def _concat(parts):
    """[(src, dst, off, ...)] -> one batch"""
    src = np.concatenate([p[0] for p in parts]).astype(np.float32)
    dst = np.concatenate([p[1] for p in parts]).astype(np.float32)
    ks = np.concatenate([np.diff(p[2]) for p in parts])
    off = np.zeros(len(ks) + 1, dtype=np.int64)
    off[1:] = np.cumsum(ks)
    return src, dst, off


def _take(src, dst, off, idx):
    return _concat([(src[off[i]:off[i + 1]], dst[off[i]:off[i + 1]], np.array([0, off[i + 1] - off[i]])) for i in idx])


class _DeviceBatch:
    """a batch in device memory with its own result buffers, pre-filled with a sentinel"""

    def __init__(self, src, dst, off, pmc_arrays=False):
        import torch
        self.src, self.dst, self.off, self.n = src, dst, off, len(off) - 1
        self.d_src = torch.from_numpy(np.ascontiguousarray(src)).cuda()
        self.d_dst = torch.from_numpy(np.ascontiguousarray(dst)).cuda()
        self.d_off = torch.from_numpy(np.ascontiguousarray(off)).cuda()
        self.d_out = torch.full((self.n, 40), SENTINEL, dtype=torch.uint8, device="cuda")
        if pmc_arrays:
            self.d_member = torch.full((max(int(off[-1]), 1),), SENTINEL, dtype=torch.uint8, device="cuda")
            self.d_info = torch.full((self.n, 16), SENTINEL, dtype=torch.uint8, device="cuda")

    def register(self, reg, params, stream):
        reg.register_batch_device(self.d_src.data_ptr(), self.d_dst.data_ptr(), self.d_off.data_ptr(), self.n, self.d_out.data_ptr(), params,
                                  stream=stream.cuda_stream)

    def max_clique(self, reg, params, stream):
        from navtech_radar_slam_amd import _rsx
        _rsx.check(reg._L.rsx_orora_max_clique_batch_device(reg._h, self.d_src.data_ptr(), self.d_dst.data_ptr(), self.d_off.data_ptr(), self.n,
                                                            C.byref(params), self.d_member.data_ptr(), self.d_info.data_ptr(), stream.cuda_stream))

    def result(self):
        from navtech_radar_slam_amd import _rsx
        return self.d_out.cpu().numpy().view(_rsx.ORORA_RESULT_DTYPE).reshape(self.n)


def _mixed_batch():
    small = synth.orora_pairs(31, 10, k_range=(40, 900))
    b1, b2 = synth.orora_pairs(32, 1, k_range=(2300, 2300)), synth.orora_pairs(33, 1, k_range=(5000, 5000))
    src, dst, off = _concat([small, b1, b2])
    return _take(src, dst, off, [0, 1, 10, 2, 3, 4, 11, 5, 6, 7, 8, 9])     # the large pairs in the middle


def test_device_entry_equals_host_entry(reg, oracle):
    """rsx_orora_register_batch_device on a caller's stream writes the host entry's bytes; a permuted batch gives the permuted
    results; a pair alone gives its batch result (a pair's result does not depend on its place in the batch, nor on whether
    the on-chip or the HBM-workspace kernel scores its neighbours)."""
    import torch
    src, dst, off = _mixed_batch()
    host = reg.register_batch(src, dst, off)
    want = oracle.orora_register_batch(src, dst, off, nthreads=8)
    _check(host, want)
    _note_pose_diff("mixed batch", host, want)
    st = torch.cuda.Stream()
    b = _DeviceBatch(src, dst, off)
    torch.cuda.synchronize()
    b.register(reg, None, st)
    torch.cuda.synchronize()
    assert b.result().tobytes() == host.tobytes()
    perm = np.random.default_rng(1).permutation(len(off) - 1)
    pb = _DeviceBatch(*_take(src, dst, off, perm))
    torch.cuda.synchronize()
    pb.register(reg, None, st)
    torch.cuda.synchronize()
    assert pb.result().tobytes() == host[perm].tobytes()
    assert reg.register_batch(*_take(src, dst, off, perm)).tobytes() == host[perm].tobytes()
    for i in range(len(off) - 1):
        one = _DeviceBatch(*_take(src, dst, off, [i]))
        torch.cuda.synchronize()
        one.register(reg, None, st)
        torch.cuda.synchronize()
        assert one.result().tobytes() == host[i:i + 1].tobytes(), i


def _params_pair(oracle, fields, flags=0):
    from navtech_radar_slam_amd import orora
    gp, op = orora.default_params(), oracle.orora_default_params()
    for f, v in fields.items():
        setattr(gp, f, v)
        setattr(op, f, v)
    gp.flags = op.flags = flags
    return gp, op


@pytest.mark.parametrize("case", orora_cases.param_cases(), ids=lambda c: c[0])
def test_numeric_parameters_match_oracle(reg, oracle, case):
    """every numeric field of rsx_orora_params off its default, GPU == oracle through _check (tests/orora_cases.py; the pairs
    of at most 400 matches are shown not to sit on a threshold by test_oracle_orora_np.py)"""
    name, fields, src, dst, off = case
    gp, op = _params_pair(oracle, fields)
    got = reg.register_batch(src, dst, off, gp)
    want = oracle.orora_register_batch(src, dst, off, op, nthreads=8)
    _note_pose_diff(name, got, want)
    _check(got, want)
    if fields.get("max_iterations") in (1, 3):
        assert (got["iterations"] == fields["max_iterations"]).any()    # the cap binds
        assert (got["iterations"] <= fields["max_iterations"]).all()


@pytest.mark.parametrize("case", orora_cases.geometry_cases(), ids=lambda c: c[0])
def test_geometry_the_generator_never_produces(reg, oracle, case):
    """yaw near +-pi and +-pi/2; the origin and points on the axes; every match duplicated; identical source points (C = S = 0);
    K = 2 and 3; lattice coordinates with exactly tied interval endpoints at every sort size -- GPU == oracle through _check"""
    name, fields, src, dst, off = case
    gp, op = _params_pair(oracle, fields)
    got = reg.register_batch(src, dst, off, gp)
    want = oracle.orora_register_batch(src, dst, off, op, nthreads=8)
    ok = want["status"] == 0
    assert np.array_equal(got["status"], want["status"])
    if name.startswith("yaw="):     # +pi and -pi are the same rotation: compare on the circle before _check's plain difference
        d = np.abs(got["yaw"] - want["yaw"])
        assert np.minimum(d, 2 * np.pi - d)[ok].max() < POSE_TOL
    _note_pose_diff(name, got, want)
    _check(got, want)


def test_bad_arguments(reg, oracle):
    """Refused with RSX_ERR_BAD_ARG by the host entry and the device entry: max_iterations = 0, gnc_factor 1.0 / 0.5 / NaN,
    RSX_ORORA_PMC_EXACT without RSX_ORORA_PMC, null pointers, n_pairs = -1; offsets that do not start at 0 by the host entry;
    n_pairs = 0 is a no-op; the handle works afterwards."""
    import torch
    from navtech_radar_slam_amd import orora, _rsx
    L = reg._L
    src, dst, off, _ = synth.orora_pairs(12, 3, k_range=(40, 80))
    n = 3
    out = np.full(n, 7, dtype=_rsx.ORORA_RESULT_DTYPE)
    b = _DeviceBatch(src, dst, off)
    torch.cuda.synchronize()

    def host(p, s=src.ctypes.data, d=dst.ctypes.data, o=off.ctypes.data, npairs=n, res=out.ctypes.data, h=reg._h):
        return L.rsx_orora_register_batch(h, s, d, o, npairs, C.byref(p) if p is not None else None, res)

    def dev(p, s=None, d=None, o=None, npairs=n, res=None, h=reg._h):
        return L.rsx_orora_register_batch_device(h, b.d_src.data_ptr() if s is None else s, b.d_dst.data_ptr() if d is None else d,
                                                 b.d_off.data_ptr() if o is None else o, npairs, C.byref(p) if p is not None else None,
                                                 b.d_out.data_ptr() if res is None else res, None)

    bad = []
    for f, v in (("max_iterations", 0), ("max_iterations", -3), ("gnc_factor", 1.0), ("gnc_factor", 0.5), ("gnc_factor", float("nan"))):
        p = orora.default_params()
        setattr(p, f, v)
        bad.append(p)
    p = orora.default_params()
    p.flags = _rsx.ORORA_PMC_EXACT
    bad.append(p)
    for p in bad:
        assert host(p) == -1 and dev(p) == -1
    ok = orora.default_params()
    assert host(ok, s=None) == -1 and host(ok, d=None) == -1 and host(ok, o=None) == -1 and host(ok, res=None) == -1 and host(ok, h=None) == -1
    assert dev(ok, s=0) == -1 and dev(ok, d=0) == -1 and dev(ok, o=0) == -1 and dev(ok, res=0) == -1 and dev(ok, h=None) == -1
    assert host(ok, npairs=-1) == -1 and dev(ok, npairs=-1) == -1
    assert host(ok, npairs=0) == 0 and dev(ok, npairs=0) == 0
    shifted = off + 5
    assert host(ok, o=shifted.ctypes.data) == -1
    # offsets that decrease in the middle, or go negative: refused by both host entries (the selection on its own included)
    m = int(off[-1])
    member = np.full(m, SENTINEL, dtype=np.uint8)
    info = np.full(n, 7, dtype=_rsx.PMC_INFO_DTYPE)

    def clique(o):
        return L.rsx_orora_max_clique_batch(reg._h, src.ctypes.data, dst.ctypes.data, o.ctypes.data, n, None, member.ctypes.data, info.ctypes.data)

    assert clique(shifted) == -1
    for bad_off in ([0, 60, 40, m], [0, -1, 40, m], [0, 40, 60, -1]):
        bad_off = np.array(bad_off, dtype=np.int64)
        assert host(ok, o=bad_off.ctypes.data) == -1 and b"offsets" in L.rsx_last_error_string(), bad_off
        assert clique(bad_off) == -1 and b"offsets" in L.rsx_last_error_string(), bad_off
    torch.cuda.synchronize()
    assert (out.view(np.uint8) == np.full(n, 7, dtype=_rsx.ORORA_RESULT_DTYPE).view(np.uint8)).all()     # nothing was written
    assert (b.d_out.cpu().numpy() == SENTINEL).all()
    assert (member == SENTINEL).all() and (info.view(np.uint8) == np.full(n, 7, dtype=_rsx.PMC_INFO_DTYPE).view(np.uint8)).all()
    want = oracle.orora_register_batch(src, dst, off)
    assert host(ok) == 0 and dev(None) == 0
    torch.cuda.synchronize()
    _check(out, want)
    assert b.result().tobytes() == out.tobytes()
    wm, winfo = oracle.pmc_select_batch(src, dst, off, ok.tim_noise_bound)
    assert clique(off) == 0 and np.array_equal(member, wm)
    for f in ("size", "max_core", "seeds", "flags"):
        assert np.array_equal(info[f], winfo[f]), f


def test_one_nan_match_leaves_the_other_pairs_alone(reg):
    """One match of one pair has a NaN coordinate: the call returns, and every OTHER pair of the batch is byte-identical to the
    batch without that pair (host and device entry).

    What the kernel does with the NaN pair itself is not asserted (the oracle is not specified there).  Observed on an MI355X
    with this data (the test prints it, "[orora nan] ..."): status 0 and max_iterations (100) iterations for both; the on-chip
    pair of 464 matches (NaN in src) came back with x = 335.5, y = -8.5, yaw = 0, 1 rotation inlier, 0 translation inliers; the
    pair of 5 000 matches (NaN in dst) with x = y = yaw = 0, 2 628 and 2 051 inliers.  Finite, but meaningless."""
    import torch
    src, dst, off = _mixed_batch()
    n = len(off) - 1
    for victim, where in ((3, "src"), (6, "dst")):      # an on-chip pair, then the 5 000-match pair of the HBM-workspace kernel
        s2, d2 = src.copy(), dst.copy()
        (s2 if where == "src" else d2)[off[victim] + 17, 1] = np.nan
        rest = [i for i in range(n) if i != victim]
        without = reg.register_batch(*_take(src, dst, off, rest))
        got = reg.register_batch(s2, d2, off)
        assert got[rest].tobytes() == without.tobytes()
        b = _DeviceBatch(s2, d2, off)
        torch.cuda.synchronize()
        b.register(reg, None, torch.cuda.current_stream())
        torch.cuda.synchronize()
        assert b.result()[rest].tobytes() == without.tobytes()
        print(f"[orora nan] pair of {off[victim + 1] - off[victim]} matches, NaN in {where}: {got[victim]}")


# ---- one handle, two threads ----

def _common_offsets(a, b):
    """two batches of as many pairs, cut to ONE offsets array: pair i keeps the first min(K_a, K_b) matches of each"""
    k = np.minimum(np.diff(a[2]), np.diff(b[2]))

    def cut(s):
        return _concat([(s[0][s[2][i]:s[2][i] + k[i]], s[1][s[2][i]:s[2][i] + k[i]], np.array([0, k[i]])) for i in range(len(k))])
    return cut(a), cut(b)


def test_two_threads_on_one_handle(reg):
    """include/rsx.h: "every entry point holds the handle's mutex for its whole duration, so any number of threads may call
    concurrently".  Two threads share one handle and call a host-buffer entry 200 times each (ctypes releases the GIL), each
    with its own batch: the batches differ in every coordinate but share one offsets array, so a call that read the other
    thread's staged input, or downloaded the other thread's result, returns wrong bytes with status 0 -- never wrong sizes.
    Every call returns, byte for byte, what its batch gave alone before the threads started: rsx_orora_register_batch against
    itself, rsx_orora_max_clique_batch against itself (member bytes and info records), and one against the other with
    RSX_ORORA_PMC on the registration (they share the selection's workspace)."""
    import threading
    from navtech_radar_slam_amd import orora, _rsx
    L = _rsx.lib()
    a, b = _common_offsets(synth.orora_pairs(41, 3, k_range=(40, 80)), synth.orora_pairs(42, 3, k_range=(40, 80)))
    assert np.array_equal(a[2], b[2]) and not np.array_equal(a[0], b[0])
    n, m = 3, int(a[2][-1])
    plain, pmc = orora.default_params(), orora.default_params()
    pmc.flags |= _rsx.ORORA_PMC

    def register(batch, p):
        out = np.full(n, 7, dtype=_rsx.ORORA_RESULT_DTYPE)
        st = L.rsx_orora_register_batch(reg._h, batch[0].ctypes.data, batch[1].ctypes.data, batch[2].ctypes.data, n, C.byref(p), out.ctypes.data)
        return st, out.tobytes()

    def clique(batch, p):
        member = np.full(m, SENTINEL, dtype=np.uint8)
        info = np.full(n, 7, dtype=_rsx.PMC_INFO_DTYPE)
        st = L.rsx_orora_max_clique_batch(reg._h, batch[0].ctypes.data, batch[1].ctypes.data, batch[2].ctypes.data, n, C.byref(p), member.ctypes.data,
                                          info.ctypes.data)
        return st, member.tobytes() + info.tobytes()

    def race(jobs):
        want = [call(batch, p) for call, batch, p in jobs]      # alone, before the threads start
        assert all(w[0] == 0 for w in want)
        wrong = [[] for _ in jobs]
        start = threading.Barrier(len(jobs))

        def run(i):
            call, batch, p = jobs[i]
            try:
                start.wait()
                for c in range(200):
                    if call(batch, p) != want[i]:
                        wrong[i].append(c)
            except Exception as e:  # noqa: BLE001
                wrong[i].append(repr(e))
        threads = [threading.Thread(target=run, args=(i,)) for i in range(len(jobs))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert wrong == [[] for _ in jobs], [w[:5] for w in wrong]
        return want

    want = race([(register, a, plain), (register, b, plain)])
    assert want[0] != want[1]                                   # a mix-up would show
    want = race([(clique, a, plain), (clique, b, plain)])
    assert want[0] != want[1]
    race([(register, a, pmc), (clique, b, plain)])


# ---- one handle, three streams ----

def _stream_batches():
    """nine batches, no two neighbours alike in input or n_pairs: (a) several pairs of 2 049 .. 16 384 matches mixed with small
    pairs -- the large-pair list and workspace, and the large pairs take long -- alternating with (b) a short batch of small
    pairs with one large pair"""
    out = []
    for c in range(9):
        if c % 2 == 0:
            small = synth.orora_pairs(600 + c, 4 + c % 3, k_range=(40, 700))
            bigs = [synth.orora_pairs(700 + 10 * c + j, 1, k_range=(k, k)) for j, k in enumerate((2049 + 300 * c, 16384 if c == 4 else 6000 + 500 * c, 3000 + 100 * c))]
            src, dst, off = _concat([small] + bigs)
            n = len(off) - 1
            order = np.random.default_rng(c).permutation(n)
        else:
            small = synth.orora_pairs(600 + c, 2 + c // 2, k_range=(40, 500))
            big = synth.orora_pairs(800 + c, 1, k_range=(2100 + 50 * c, 2100 + 50 * c))
            src, dst, off = _concat([small, big])
            order = np.arange(len(off) - 1)
        out.append(_take(src, dst, off, order))
    sizes = [len(b[2]) - 1 for b in out]
    assert all(sizes[i] != sizes[i + 1] for i in range(8)), sizes
    return out


def _run_stream_calls(pmc, serial, batches, host_at):
    """the nine calls on a FRESH handle: rotating over three streams without any host synchronisation in between (serial=False),
    or on one stream with a synchronise after every call (serial=True) -> what every call wrote"""
    import torch
    from navtech_radar_slam_amd import orora, _rsx
    reg = orora.Orora()
    p = orora.default_params()
    if pmc:
        p.flags |= _rsx.ORORA_PMC
        reg.reserve(max(int(b[2][-1]) for b in batches))
    streams = [torch.cuda.Stream() for _ in range(1 if serial else 3)]
    dev = [_DeviceBatch(*b, pmc_arrays=pmc) for b in batches]
    host = {}
    torch.cuda.synchronize()
    for c, b in enumerate(dev):
        if c in host_at:
            host[c] = reg.register_batch(b.src, b.dst, b.off, p)      # host buffers, the handle's own stream, between device calls
        else:
            b.register(reg, p, streams[c % len(streams)])
        if pmc:     # the selection on its own, for the batch before this one, on the NEXT stream: shares pmc_ws with the call above
            prev = dev[c - 1]
            prev.max_clique(reg, p, streams[(c + 1) % len(streams)])
        if serial:
            torch.cuda.synchronize()
    info = reg.last_pmc_info(dev[-1].n) if pmc else None   # waits for the last call only
    torch.cuda.synchronize()
    res = [host[c] if c in host else b.result() for c, b in enumerate(dev)]
    sel = [(b.d_member.cpu().numpy(), b.d_info.cpu().numpy().view(_rsx.PMC_INFO_DTYPE).reshape(b.n)) for b in dev] if pmc else None
    reg.close()
    return res, sel, info


@pytest.mark.parametrize("pmc", [False, True], ids=["plain", "pmc"])
def test_one_handle_three_streams(oracle, pmc):
    """include/rsx.h: calls on ONE handle that pass different streams are ordered by the library.  Nine calls rotate over three
    streams with no host synchronisation in between; every call has its own input, batch size and (sentinel-filled) outputs;
    a host-buffer call sits between the device calls.  Byte for byte what the same calls give one at a time, and the oracle's
    result for every input.  With RSX_ORORA_PMC the selection buffers, rsx_orora_max_clique_batch_device's member and info
    arrays and rsx_orora_last_pmc_info are covered too."""
    from navtech_radar_slam_amd import _rsx
    batches = _stream_batches()
    host_at = {4, 7}
    want, want_sel, want_info = _run_stream_calls(pmc, True, batches, host_at)
    got, got_sel, got_info = _run_stream_calls(pmc, False, batches, host_at)
    for c, (src, dst, off) in enumerate(batches):
        assert got[c].tobytes() == want[c].tobytes(), c
        assert not (got[c].view(np.uint8) == SENTINEL).all()
        if pmc:
            wm, winfo = oracle.pmc_select_batch(src, dst, off, 1.5, nthreads=8)
            s2, d2, o2 = oracle.pmc_compact(src, dst, off, wm)
            ref = oracle.orora_register_batch(s2, d2, o2, nthreads=8)
            assert np.array_equal(got_sel[c][0], want_sel[c][0]) and got_sel[c][1].tobytes() == want_sel[c][1].tobytes(), c
            assert np.array_equal(got_sel[c][0][:int(off[-1])], wm), c
            for f in ("size", "max_core", "seeds", "flags"):
                assert np.array_equal(got_sel[c][1][f], winfo[f]), (c, f)
        else:
            ref = oracle.orora_register_batch(src, dst, off, nthreads=8)
        _note_pose_diff(f"three streams, call {c}", got[c], ref)
        _check(got[c], ref)
    if pmc:
        assert got_info.tobytes() == want_info.tobytes()
        winfo = oracle.pmc_select_batch(*batches[-1], 1.5, nthreads=8)[1]
        for f in ("size", "max_core", "seeds", "flags"):
            assert np.array_equal(got_info[f], winfo[f]), f
