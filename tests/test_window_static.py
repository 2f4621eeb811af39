"""Compile-time guard of the window kernel's occupancy (no GPU needed: hipcc cross-compiles).

sc_window_kernel is laid out for four 4-wave workgroups per CU: 128 VGPRs per wave (tests/test_filter_static.py pins the
registers and the spills) and a quarter of the CU's 160 KB of LDS per workgroup.  The LDS of a workgroup is what the compiler
reports for the kernel's static arrays plus the dynamic part launch_window asks for (W_LDS = the query's fp16 image and its key
image, sc_kernels.h)."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "navtech-radar-slam_amd", "csrc")
LDS_PER_CU = 160 * 1024


def _constant(name):
    text = open(os.path.join(CSRC, "sc_kernels.h")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


def test_four_window_workgroups_fit_a_cu():
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "sc_window.s")
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
               "-fhip-fp32-correctly-rounded-divide-sqrt", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-x", "hip",
               "--cuda-device-only", "-S", os.path.join(CSRC, "sc_window.hip"), "-o", out]
        subprocess.run(cmd, check=True, capture_output=True, timeout=900)
        text = open(out).read()
    # the kernel's metadata block: .group_segment_fixed_size stands in front of its .name, .vgpr_count behind it
    name = re.search(r"\.name:\s+\S*sc_window_kernel\S*\n", text)
    assert name, "no resource report for sc_window_kernel"
    lds = re.findall(r"\.group_segment_fixed_size:\s+(\d+)\n", text[:name.start()])
    vg = re.search(r"\.vgpr_count:\s+(\d+)\n", text[name.end():])
    assert lds and vg
    static_lds, vgprs = int(lds[-1]), int(vg.group(1))
    assert static_lds > 0
    dynamic_lds = _constant("FILTER_QIMG_BYTES") + _constant("WINDOW_QK_BYTES")
    # the launch's dynamic size is W_LDS of sc_window_dev.h: the sum of the same two constants
    dev = open(os.path.join(CSRC, "sc_window_dev.h")).read()
    assert re.search(r"W_LDS = FILTER_QIMG_BYTES \+ WINDOW_QK_BYTES;", dev)
    total = static_lds + dynamic_lds
    print(f"sc_window_kernel: {static_lds} B static + {dynamic_lds} B dynamic = {total} B of LDS per workgroup, {vgprs} VGPRs")
    assert 4 * total <= LDS_PER_CU, (static_lds, dynamic_lds)
    assert 4 * vgprs <= 512, vgprs  # four waves per SIMD
    # no instrumentation in the product build: the region timers are behind RSX_WINDOW_PROF
    assert "s_memtime" not in text
