// wave_selftest.hip -- rsx_selftest_wave (include/rsx_diag.h): every primitive of rsx_wave_dev.h on caller-given lane
// values, lane by lane, so that tests/test_gpu_wave.py can hold the header to its documented orders bit for bit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rsx_common.h"
#include "rsx_wave_dev.h"

namespace {

namespace wave = rsx::wave;
constexpr int NPRIM = RSX_SELFTEST_WAVE_PRIMS;

// One wavefront; all cases in one launch.  Views of a lane's 64-bit pattern: u64 = the pattern, f64 = its bits, u32 / i32 = the
// low word, f32 = the HIGH word's bits (a finite double below 2^1017 then has a finite f32 view and the other way round).
__global__ __launch_bounds__(64) void wave_selftest_kernel(const unsigned long long *__restrict__ in, int n_cases, unsigned long long *__restrict__ out) {
  const int lane = threadIdx.x;
  auto f64bits = [](double d) { return (unsigned long long)__double_as_longlong(d); };
  auto f32bits = [](float f) { return (unsigned long long)__float_as_uint(f); };
  for (int c = 0; c < n_cases; c++) {
    const unsigned long long u = in[(size_t)c * 64 + lane];
    const unsigned lo = (unsigned)u;
    const double d = __longlong_as_double((long long)u);
    const float f = __uint_as_float((unsigned)(u >> 32));
    unsigned long long r[NPRIM];
    r[0] = wave::dpp<0xB1>(lo);           // quad_perm [1,0,3,2]
    r[1] = wave::dpp<0x138>(u);           // wave_shr:1
    r[2] = f64bits(wave::dpp<0x130>(d));  // wave_shl:1
    r[3] = f32bits(wave::dpp<0x142, 0xa>(f));  // row_bcast:15 into rows 1, 3
    r[4] = wave::readlane(u, 37);
    r[5] = (unsigned)wave::sum_i32((int)lo);
    r[6] = (unsigned)wave::max_i32((int)lo);
    r[7] = wave::max_u32(lo);
    r[8] = wave::minmax_u64<false>(u);
    r[9] = wave::minmax_u64<true>(u);
    r[10] = f32bits(wave::min_f32(f));
    r[11] = f64bits(wave::sum_f64_rows_seq(d));
    r[12] = f64bits(wave::sum_f64_rows_pair(d));
    r[13] = f32bits(wave::sum_f32_bcast(f));
    r[14] = f64bits(wave::butterfly(d, wave::Add{}));
    r[15] = wave::butterfly_u64(u, [](unsigned long long a, unsigned long long b) { return b > a ? b : a; });
    r[16] = wave::incl_add_u32(lo);
    r[17] = wave::incl_max_u32(lo);
    auto mx = [](double a, double b) { return fmax(a, b); };
    r[18] = f64bits(wave::incl_max_f64<false>(fabs(d), lane, mx));
    r[19] = f64bits(wave::incl_max_f64<true>(fabs(d), lane, mx));
#pragma unroll
    for (int p = 0; p < NPRIM; p++) out[((size_t)c * NPRIM + p) * 64 + lane] = r[p];
  }
}

}  // namespace

int rsx_selftest_wave(int device, const uint64_t *lanes, int32_t n_cases, uint64_t *out) try {
  if (!lanes || !out || n_cases < 1 || n_cases > 4096) return rsx::fail(RSX_ERR_BAD_ARG, "bad arg");
  RSX_TRY(rsx::check_device(device));
  RSX_HIP(hipSetDevice(device));
  const size_t in_bytes = (size_t)n_cases * 64 * sizeof(uint64_t), out_bytes = in_bytes * NPRIM;
  rsx::DevBuf buf;
  RSX_TRY(buf.reserve(in_bytes + out_bytes, nullptr, false));
  unsigned long long *d_in = buf.as<unsigned long long>(), *d_out = d_in + (size_t)n_cases * 64;
  RSX_HIP(hipMemcpy(d_in, lanes, in_bytes, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(wave_selftest_kernel, dim3(1), dim3(64), 0, nullptr, d_in, (int)n_cases, d_out);
  RSX_HIP(hipGetLastError());
  RSX_HIP(hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost));
  return RSX_OK;
} RSX_CATCH_ALL
