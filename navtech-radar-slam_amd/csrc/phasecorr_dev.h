// phasecorr_dev.h -- device code the kernels of csrc/phasecorr.hip share: the LDS transform of a block of lines, the cross-power of two
// spectrum samples, one pixel of the windowed Cartesian image, and the workgroup reductions (built on rsx_wave_dev.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rsx_wave_dev.h"

#pragma STDC FP_CONTRACT OFF

namespace rsx {
namespace phasecorr {

constexpr int NT = 256, NW = NT / 64;
constexpr int R_MIN = 4;      // innermost radius of the polar-resampled magnitude spectrum
constexpr int MAX_BLOCKS = 64;  // workgroups a pass over one N x N image takes, at most (N = 512: 8 lines each)
constexpr float EPS = 1e-9f;  // C / (|C| + EPS max|C|)

struct Dims {
  int n, logn;      // image size and its logarithm
  int lines, llog;  // lines of n samples a workgroup transforms at once: min(4096 / n, 16)
  int nb;           // n / lines workgroups per image and pass
  int rows, cols;   // the polar scan
  int nr;           // n / 2 - R_MIN radii
};

// what a pair keeps in device memory between the launches
struct PairRec {
  float pmax[2][MAX_BLOCKS];   // per candidate: the column pass's partial maxima of |F_dst conj(G)|
  double psum[2][MAX_BLOCKS];  // per candidate: the inverse column pass's partial sums of the normalised cross-power's magnitudes
  double theta[2];             // theta0 and theta0 + pi
  double rot_peak;
  int32_t winner, reserved;
  unsigned char pad[2048 - 2 * MAX_BLOCKS * 12 - 32];
};
static_assert(sizeof(PairRec) == 2048, "include/rsx.h states the workspace per pair");

// ---- radix-2 Stockham transform of `lines` lines of n complex samples in LDS (line l at x + l (n + 1): the odd pitch keeps the
// column tiles' transposed stores off one bank), n / 2 butterflies per line and stage spread over the NT threads.  Every stage reads
// x[b] and x[b + n / 2] -- a wavefront's 8-byte reads are contiguous, conflict-free -- and writes y[q + 2 s p], y[q + 2 s p + s]
// (stride 2 in the first stage: twice the cycles of a contiguous store), then the buffers swap: natural order in, natural order
// out, no bit reversal.  E[k] = (cos, sin)(2 pi k / n) in LDS.  The caller has synchronised after filling x; the result is in
// the returned buffer, visible to the whole workgroup.  Unscaled in both directions.
template <bool INV>
__device__ __forceinline__ float2 *fft_lines(float2 *x, float2 *y, const float2 *E, int n, int logn, int lines, int t) {
  const int P = n + 1, half = n >> 1, total = lines * half;
  for (int st = 0; st < logn; st++) {
    const int s = 1 << st;
    for (int idx = t; idx < total; idx += NT) {
      const int line = idx >> (logn - 1), b = idx & (half - 1);
      const int p = b >> st, q = b & (s - 1);
      float2 w = E[p << st];
      if (!INV) w.y = -w.y;
      const float2 a = x[line * P + b], c = x[line * P + b + half];
      float2 *o = y + line * P + q + ((2 * p) << st);
      o[0] = make_float2(a.x + c.x, a.y + c.y);
      const float dx = a.x - c.x, dy = a.y - c.y;
      o[s] = make_float2(dx * w.x - dy * w.y, dx * w.y + dy * w.x);
    }
    __syncthreads();
    float2 *tmp = x;
    x = y;
    y = tmp;
  }
  return x;
}

// C = f conj(g) and |C|; for f == g the imaginary part is exactly 0 (the two products commute)
__device__ __forceinline__ float2 xpower(float2 f, float2 g, float &mag) {
  const float2 c = make_float2(f.x * g.x + f.y * g.y, f.y * g.x - f.x * g.y);
  mag = sqrtf(c.x * c.x + c.y * c.y);
  return c;
}
// C / (|C| + EPS mx) and its magnitude w = |C| / (|C| + EPS mx); 0 where the denominator is 0 (two empty images)
__device__ __forceinline__ float2 xnorm(float2 f, float2 g, float mx, float &w) {
  float mag;
  const float2 c = xpower(f, g, mag);
  const float den = mag + EPS * mx;
  w = den > 0.0f ? mag / den : 0.0f;
  return den > 0.0f ? make_float2(c.x / den, c.y / den) : make_float2(0.0f, 0.0f);
}
__device__ __forceinline__ float2 xnorm(float2 f, float2 g, float mx) {
  float w;
  return xnorm(f, g, mx, w);
}

// the azimuth shift of an image at rotation psi, in rows, in [0, rows): fp64, one rounding (tests/phasecorr_np.py cart_image)
__device__ __forceinline__ float azimuth_shift(double psi, int rows) {
  double s = fmod(psi * (double)rows / (2.0 * 3.14159265358979323846), (double)rows);
  if (s < 0.0) s += (double)rows;
  const float sf = (float)s;
  return sf >= (float)rows ? 0.0f : sf;
}

// one pixel of the windowed Cartesian image, in the operation order of the restatement; m = the map's (range, azimuth) coordinates,
// pw = the first power sample of the image
__device__ __forceinline__ float cart_pixel(float2 m, float s, int rows, int cols, const uint8_t *__restrict__ pw, int row_stride, float hi, float hj) {
  if (m.x < 0.0f) return 0.0f;
  float a = m.y + s;
  if (a >= (float)rows) a = a - (float)rows;
  const float a0f = floorf(a), fa = a - a0f;
  int a0 = (int)a0f;
  if (a0 >= rows) a0 = rows - 1;
  const int a1 = a0 + 1 >= rows ? 0 : a0 + 1;
  const float r0f = floorf(m.x), fr = m.x - r0f;
  int r0 = (int)r0f;
  if (r0 > cols - 1) r0 = cols - 1;  // (the map holds no such pixel: a second fence in front of the loads)
  const int r1 = r0 + 1 < cols ? r0 + 1 : cols - 1;
  const uint8_t *ra = pw + (int64_t)a0 * row_stride, *rb = pw + (int64_t)a1 * row_stride;
  const float p00 = (float)ra[r0], p01 = (float)ra[r1], p10 = (float)rb[r0], p11 = (float)rb[r1];
  const float ga = 1.0f - fa, gr = 1.0f - fr;
  const float v = (((ga * gr) * p00 + (ga * fr) * p01) + (fa * gr) * p10) + (fa * fr) * p11;
  return (v * hi) * hj;
}

// ---- workgroup reductions (every thread calls; the result in every thread); red: NW 64-bit words of LDS ----
__device__ __forceinline__ unsigned long long block_max_u64(unsigned long long v, unsigned long long *red, int t) {
  v = rsx::wave::minmax_u64<true>(v);
  __syncthreads();  // (red is free: the last reduction has been read)
  if ((t & 63) == 0) red[t >> 6] = v;
  __syncthreads();
  unsigned long long m = red[0];
  for (int w = 1; w < NW; w++) m = red[w] > m ? red[w] : m;
  return m;
}
// the maximum of floats that are all >= 0 (their bit patterns order as unsigned integers)
__device__ __forceinline__ float block_max_nonneg(float v, unsigned long long *red, int t) {
  return __uint_as_float((unsigned)block_max_u64((unsigned long long)__float_as_uint(v), red, t));
}
// the sum of one double per thread in a fixed order: the wavefront by the row tree, the wavefronts in ascending order
__device__ __forceinline__ double block_sum_f64(double v, unsigned long long *red, int t) {
  v = rsx::wave::sum_f64_rows_pair(v);
  __syncthreads();
  if ((t & 63) == 0) red[t >> 6] = (unsigned long long)__double_as_longlong(v);
  __syncthreads();
  double acc = 0.0;
  for (int w = 0; w < NW; w++) acc = acc + __longlong_as_double((long long)red[w]);
  return acc;
}
// key of (value, index): a larger value wins, then the LOWER index
__device__ __forceinline__ unsigned long long peak_key(float v, unsigned idx) {
  const unsigned b = __float_as_uint(v);
  return ((unsigned long long)(b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u)) << 32) | (unsigned long long)(0xffffffffu - idx);
}
__device__ __forceinline__ unsigned key_index(unsigned long long key) { return 0xffffffffu - (unsigned)key; }

}  // namespace phasecorr
}  // namespace rsx
