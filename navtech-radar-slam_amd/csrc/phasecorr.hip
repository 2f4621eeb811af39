// phasecorr.hip -- phase-correlation (Fourier-Mellin at scale 1) registration of pairs of polar scans: dense, correspondence-free, the
// one estimator of the library that reads the power image itself.  None of it is in the reference checkout, so this implements the
// rules written in include/rsx.h as restated in tests/phasecorr_np.py (PARITY UNPINNED); that file is the arithmetic contract.  The
// windowed Cartesian image is bit-identical to the restatement; the transforms are fp32 in a fixed order (no atomics, every maximum
// breaks ties by index), so a pair's result does not depend on its place in a batch.
//
// One batch = nine launches, whatever its size, no host round trip (the angles stay in the pairs' records), in two stages on
// caller-given buffers (phasecorr.h: launch_spectra for the scans, launch_pairs for the pairs; they take the tables and the shape and
// touch no handle).  The stand-alone entries run both in a row on the handle's workspace; the windowed odometry (csrc/odometry.hip) runs
// the first in a window's extraction stage and the second in its matching stage, on slots of its own sets:
//   scans   1. pc_rows_fwd    image at psi = 0 (resampled from the polar scan while the rows are filled) -> row transforms -> F
//           2. pc_cols<0>     column transforms of F, in place
//           3. pc_polar       |F| fftshifted, high-passed, resampled on N angles x N/2 - 4 radii -> transform along the angle -> A
//   pairs   4. pc_rotation    one workgroup per pair: cross-power of A_dst and A_src, sum over the radii, inverse transform, peak,
//                             parabola -> theta0, theta0 + pi
//           5. pc_rows_fwd    image of src at psi = -theta for both candidates -> row transforms -> G
//           6. pc_cols<1>     column transforms of G, in place; partial maxima of |F_dst conj(G)| per workgroup
//           7. pc_cols<2>     the normalised cross-power is formed while a column tile is loaded -> inverse column transforms -> W
//           8. pc_rows_inv    inverse row transforms of W -> the surface (real part / the sum of the cross-power's magnitudes)
//           9. pc_peak        one workgroup per pair: peak of each candidate's surface, the winner, the runner-up, the five direct
//                             sums under the parabolas -> the result
// A workgroup of 256 threads transforms min(4096 / N, 16) lines at once in LDS (phasecorr_dev.h: fft_lines); a column pass loads a tile
// of that many adjacent columns (128-byte runs at N <= 256, 64-byte at N = 512) through L2.  LDS: 2 x lines x (N + 1) + N complex
// samples, 66 - 70 KiB: two workgroups per CU.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "phasecorr.h"
#include "phasecorr_dev.h"
#include "ragged_host.h"

#pragma STDC FP_CONTRACT OFF

using rsx::fail;

namespace {

using namespace rsx::phasecorr;
constexpr int MAX_IMAGES = 4096, MAX_PAIRS = 16384;
static_assert(sizeof(rsx_phasecorr_params) == 40 && sizeof(rsx_phasecorr_result) == 56, "record layouts of include/rsx.h");

// the handle's tables, all in one buffer
struct Tables {
  const float2 *map;   // [n][n] range-bin and azimuth-row coordinate; range < 0: the pixel reads 0
  const float2 *E;     // [n] (cos, sin)(2 pi k / n)
  const float2 *dirs;  // [n] (cos, sin)(pi k / n)
  const float *hann;   // [n]
  const float *hp;     // [n] cos(pi (u - n / 2) / n)
};

// the scans of a call: a pair's src is spectrum slot `src` and image `src + image_offset` (the stand-alone entries: 0; the odometry's
// window: -1, slot 0 being the scan carried from the window before, whose image is not needed -- only src is re-sampled)
struct Scans {
  const uint8_t *imgs;
  int64_t image_stride;
  int n_images, n_slots, row_stride, col_offset, image_offset;
};

// where the pieces of the workspace lie (the sum is the size include/rsx.h states)
struct Layout {
  size_t F, A, G, W, surf, rec, curve, total;
  Layout(const Dims &d, int n_images, int n_pairs) {
    const size_t n2 = (size_t)d.n * d.n, ni = (size_t)n_images, np = (size_t)n_pairs;
    F = 0;
    A = F + ni * n2 * 8;
    G = A + ni * (size_t)d.nr * d.n * 8;
    W = G + np * 2 * n2 * 8;
    surf = W + np * 2 * n2 * 8;
    rec = surf + np * 2 * n2 * 4;
    curve = rec + np * sizeof(PairRec);
    total = curve + np * (size_t)d.n * 4 + 64;
  }
};

__device__ __forceinline__ bool pair_ok(const int32_t *__restrict__ pairs, int pair, int n_images, int &src, int &dst) {
  src = pairs[2 * pair];
  dst = pairs[2 * pair + 1];
  return src >= 0 && src < n_images && dst >= 0 && dst < n_images;
}

__device__ __forceinline__ void load_table(float2 *E, const float2 *__restrict__ g, int n, int t) {
  for (int k = t; k < n; k += NT) E[k] = g[k];
}

// 1. and 5.: rows [blockIdx.x lines, + lines) of the image of job blockIdx.y, made in LDS, transformed, stored.  pairs == nullptr:
// job = scan, psi = 0; else job = 2 pair + candidate, the scan is the pair's src, psi = -theta[candidate]
__global__ __launch_bounds__(NT) void pc_rows_fwd(Dims d, Tables tb, Scans sc, const int32_t *__restrict__ pairs, const PairRec *__restrict__ rec,
                                                  int n_cand, float2 *__restrict__ out, float *__restrict__ out_cart) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pc_lds[];
  const int t = threadIdx.x, n = d.n, P = n + 1, job = blockIdx.y;
  float2 *x = reinterpret_cast<float2 *>(pc_lds), *y = x + d.lines * P, *E = y + d.lines * P;
  int image = job;
  float s = 0.0f;
  if (pairs) {
    int src, dst;
    if ((job & 1) >= n_cand || !pair_ok(pairs, job >> 1, sc.n_slots, src, dst)) return;  // (uniform)
    image = src + sc.image_offset;
    if (image < 0 || image >= sc.n_images) return;  // (uniform; no caller builds such a pair: a fence in front of the loads)
    s = azimuth_shift(-rec[job >> 1].theta[job & 1], d.rows);
  }
  load_table(E, tb.E, n, t);
  const uint8_t *pw = sc.imgs + (int64_t)image * sc.image_stride + sc.col_offset;
  const int row0 = blockIdx.x * d.lines;
  for (int idx = t; idx < d.lines * n; idx += NT) {
    const int line = idx >> d.logn, j = idx & (n - 1), i = row0 + line;
    const float v = cart_pixel(tb.map[(size_t)i * n + j], s, d.rows, d.cols, pw, sc.row_stride, tb.hann[i], tb.hann[j]);
    if (out_cart) out_cart[((size_t)image * n + i) * n + j] = v;
    x[line * P + j] = make_float2(v, 0.0f);
  }
  __syncthreads();
  const float2 *r = fft_lines<false>(x, y, E, n, d.logn, d.lines, t);
  float2 *o = out + (size_t)job * n * n;
  for (int idx = t; idx < d.lines * n; idx += NT) {
    const int line = idx >> d.logn, k = idx & (n - 1);
    o[(size_t)(row0 + line) * n + k] = r[line * P + k];
  }
}

// 2., 6. and 7.: columns [blockIdx.x lines, + lines) of the image of job blockIdx.y.  MODE 0: forward, in place (job = scan).
// MODE 1: forward, in place, and this workgroup's maximum of |F_dst conj(G)| (job = 2 pair + candidate).  MODE 2: the normalised
// cross-power of F_dst and G is formed on load, inverse transform, stored to W
template <int MODE>
__global__ __launch_bounds__(NT) void pc_cols(Dims d, Tables tb, float2 *__restrict__ data, const float2 *__restrict__ F, const int32_t *__restrict__ pairs,
                                              int n_images, PairRec *__restrict__ rec, int n_cand, float2 *__restrict__ Wout) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pc_lds[];
  __shared__ unsigned long long red[NW];
  const int t = threadIdx.x, n = d.n, P = n + 1, job = blockIdx.y;
  float2 *x = reinterpret_cast<float2 *>(pc_lds), *y = x + d.lines * P, *E = y + d.lines * P;
  const float2 *Fd = nullptr;
  if (MODE != 0) {
    int src, dst;
    if ((job & 1) >= n_cand || !pair_ok(pairs, job >> 1, n_images, src, dst)) return;  // (uniform)
    Fd = F + (size_t)dst * n * n;
  }
  load_table(E, tb.E, n, t);
  float2 *g = data + (size_t)job * n * n;
  const int c0 = blockIdx.x * d.lines;
  float mx = 0.0f, wsum = 0.0f;
  if (MODE == 2) {
    const float *pm = rec[job >> 1].pmax[job & 1];
    for (int b = 0; b < d.nb; b++) mx = fmaxf(mx, pm[b]);
  }
  for (int idx = t; idx < d.lines * n; idx += NT) {
    const int row = idx >> d.llog, cl = idx & (d.lines - 1);
    const size_t at = (size_t)row * n + c0 + cl;
    float w = 0.0f;
    x[cl * P + row] = MODE == 2 ? xnorm(Fd[at], g[at], mx, w) : g[at];
    wsum = wsum + w;
  }
  if (MODE == 2) {  // (a thread its own samples in ascending order, then the fixed order of block_sum_f64)
    const double tot = block_sum_f64((double)wsum, red, t);
    if (t == 0) rec[job >> 1].psum[job & 1][blockIdx.x] = tot;
  }
  __syncthreads();
  const float2 *r = MODE == 2 ? fft_lines<true>(x, y, E, n, d.logn, d.lines, t) : fft_lines<false>(x, y, E, n, d.logn, d.lines, t);
  float2 *o = MODE == 2 ? Wout + (size_t)job * n * n : g;
  float m = 0.0f;
  for (int idx = t; idx < d.lines * n; idx += NT) {
    const int row = idx >> d.llog, cl = idx & (d.lines - 1);
    const size_t at = (size_t)row * n + c0 + cl;
    const float2 v = r[cl * P + row];
    o[at] = v;
    if (MODE == 1) {
      float mag;
      (void)xpower(Fd[at], v, mag);
      m = fmaxf(m, mag);
    }
  }
  if (MODE == 1) {
    m = block_max_nonneg(m, red, t);
    if (t == 0) rec[job >> 1].pmax[job & 1][blockIdx.x] = m;
  }
}

// 8.: inverse row transforms of W; the surface is the real part over the sum of the cross-power's magnitudes (1 at a perfect match)
__global__ __launch_bounds__(NT) void pc_rows_inv(Dims d, Tables tb, const float2 *__restrict__ W, const int32_t *__restrict__ pairs, int n_images, int n_cand,
                                                  const PairRec *__restrict__ rec, float *__restrict__ surf) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pc_lds[];
  const int t = threadIdx.x, n = d.n, P = n + 1, job = blockIdx.y;
  float2 *x = reinterpret_cast<float2 *>(pc_lds), *y = x + d.lines * P, *E = y + d.lines * P;
  int src, dst;
  if ((job & 1) >= n_cand || !pair_ok(pairs, job >> 1, n_images, src, dst)) return;  // (uniform)
  load_table(E, tb.E, n, t);
  const float2 *w = W + (size_t)job * n * n;
  const int row0 = blockIdx.x * d.lines;
  for (int idx = t; idx < d.lines * n; idx += NT) {
    const int line = idx >> d.logn, k = idx & (n - 1);
    x[line * P + k] = w[(size_t)(row0 + line) * n + k];
  }
  __syncthreads();
  const float2 *r = fft_lines<true>(x, y, E, n, d.logn, d.lines, t);
  double total = 0.0;  // the sum of the cross-power's magnitudes, the column pass's partial sums in ascending order
  for (int b = 0; b < d.nb; b++) total = total + rec[job >> 1].psum[job & 1][b];
  const float scale = total > 0.0 ? (float)(1.0 / total) : 0.0f;
  float *o = surf + (size_t)job * n * n;
  for (int idx = t; idx < d.lines * n; idx += NT) {
    const int line = idx >> d.logn, j = idx & (n - 1);
    o[(size_t)(row0 + line) * n + j] = r[line * P + j].x * scale;
  }
}

// 3.: radii [R_MIN + blockIdx.x lines, + lines) of scan blockIdx.y: the high-passed magnitude spectrum resampled along N angles over
// [0, pi), then the transform along the angle
__global__ __launch_bounds__(NT) void pc_polar(Dims d, Tables tb, const float2 *__restrict__ F, float2 *__restrict__ A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pc_lds[];
  const int t = threadIdx.x, n = d.n, P = n + 1, h = n >> 1, mask = n - 1;
  float2 *x = reinterpret_cast<float2 *>(pc_lds), *y = x + d.lines * P, *E = y + d.lines * P;
  load_table(E, tb.E, n, t);
  const float2 *f = F + (size_t)blockIdx.y * n * n;
  const int r0 = R_MIN + blockIdx.x * d.lines;
  auto sample = [&](int vv, int uu) {  // fftshifted (vv, uu) is frequency (vv - n / 2, uu - n / 2)
    const float2 c = f[(size_t)((vv + h) & mask) * n + ((uu + h) & mask)];
    const float X = tb.hp[uu] * tb.hp[vv];
    return sqrtf(c.x * c.x + c.y * c.y) * ((1.0f - X) * (2.0f - X));
  };
  for (int idx = t; idx < d.lines * n; idx += NT) {
    const int line = idx >> d.logn, k = idx & mask, r = r0 + line;
    float p = 0.0f;
    if (r < h) {
      const float2 dir = tb.dirs[k];
      const float u = (float)h + (float)r * dir.x, v = (float)h + (float)r * dir.y;
      const float u0f = floorf(u), v0f = floorf(v), fu = u - u0f, fv = v - v0f;
      int u0 = (int)u0f, v0 = (int)v0f;
      u0 = u0 < 0 ? 0 : (u0 > mask ? mask : u0);  // (1 <= u, v <= n - 1 by construction: a second fence in front of the loads)
      v0 = v0 < 0 ? 0 : (v0 > mask ? mask : v0);
      const int u1 = u0 + 1 < n ? u0 + 1 : mask, v1 = v0 + 1 < n ? v0 + 1 : mask;
      p = (((1.0f - fv) * (1.0f - fu)) * sample(v0, u0) + ((1.0f - fv) * fu) * sample(v0, u1)) +
          ((fv * (1.0f - fu)) * sample(v1, u0) + (fv * fu) * sample(v1, u1));
    }
    x[line * P + k] = make_float2(p, 0.0f);
  }
  __syncthreads();
  const float2 *r = fft_lines<false>(x, y, E, n, d.logn, d.lines, t);
  float2 *a = A + (size_t)blockIdx.y * d.nr * n;
  for (int idx = t; idx < d.lines * n; idx += NT) {
    const int line = idx >> d.logn, k = idx & mask, rr = r0 + line;
    if (rr < h) a[(size_t)(rr - R_MIN) * n + k] = r[line * P + k];
  }
}

// three-point parabola through (-1, cm), (0, c0), (1, cp): the abscissa of its vertex
__device__ __forceinline__ double parabola(double cm, double c0, double cp) {
  const double den = cm - 2.0 * c0 + cp;
  return den == 0.0 ? 0.0 : 0.5 * (cm - cp) / den;
}

// 4.: one workgroup per pair
__global__ __launch_bounds__(NT) void pc_rotation(Dims d, Tables tb, const float2 *__restrict__ A, const int32_t *__restrict__ pairs, int n_images,
                                                  PairRec *__restrict__ rec, float *__restrict__ curve) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pc_lds[];
  __shared__ unsigned long long red[NW];
  __shared__ double three[3];
  const int t = threadIdx.x, n = d.n, P = n + 1, mask = n - 1, pair = blockIdx.x;
  float2 *x = reinterpret_cast<float2 *>(pc_lds), *y = x + d.lines * P, *E = y + d.lines * P;
  float2 *S0 = y + P;  // (the second line of y: fft_lines touches one line here) the summed cross-power, kept for the direct sums
  int src, dst;
  if (!pair_ok(pairs, pair, n_images, src, dst)) return;  // (uniform) pc_peak writes the pair's result
  load_table(E, tb.E, n, t);
  const float2 *As = A + (size_t)src * d.nr * n, *Ad = A + (size_t)dst * d.nr * n;
  float mx = 0.0f;
  for (int i = t; i < d.nr * n; i += NT) {
    float mag;
    (void)xpower(Ad[i], As[i], mag);
    mx = fmaxf(mx, mag);
  }
  mx = block_max_nonneg(mx, red, t);
  float wsum = 0.0f;
  for (int f = t; f < n; f += NT) {
    const int fm = f < n - f ? f : n - f;
    float2 acc = make_float2(0.0f, 0.0f);
    for (int r = 0; r < d.nr; r++) {  // the radii in ascending order
      if (fm > r + R_MIN) continue;
      float w;
      const float2 c = xnorm(Ad[(size_t)r * n + f], As[(size_t)r * n + f], mx, w);
      acc.x = acc.x + c.x;
      acc.y = acc.y + c.y;
      wsum = wsum + w;
    }
    x[f] = acc;
    S0[f] = acc;
  }
  // the sum of the terms' magnitudes: a thread its own frequencies in ascending order, then the fixed order of block_sum_f64
  const double total = block_sum_f64((double)wsum, red, t), inv_count = total > 0.0 ? 1.0 / total : 0.0;
  const float2 *r = fft_lines<true>(x, y, E, n, d.logn, 1, t);
  unsigned long long key = 0;
  for (int k = t; k < n; k += NT) {
    const float c = (float)((double)r[k].x * inv_count);
    curve[(size_t)pair * n + k] = c;
    const unsigned long long kk = peak_key(c, (unsigned)k);
    key = kk > key ? kk : key;
  }
  key = block_max_u64(key, red, t);
  const int k0 = (int)(key_index(key) & (unsigned)mask);
  if (t < 3) {  // the curve at k0 - 1, k0, k0 + 1 as direct sums, fp64, ascending f
    const int k = (k0 - 1 + t) & mask;
    double sum = 0.0;
    for (int f = 0; f < n; f++) {
      const float2 e = E[(f * k) & mask], sv = S0[f];
      sum = sum + ((double)sv.x * (double)e.x - (double)sv.y * (double)e.y);
    }
    three[t] = sum * inv_count;
  }
  __syncthreads();
  if (t == 0) {
    const double delta = parabola(three[0], three[1], three[2]);
    const int ks = k0 >= n / 2 ? k0 - n : k0;
    const double pi = 3.14159265358979323846, th0 = ((double)ks + delta) * pi / (double)n, th1 = th0 + pi;
    rec[pair].theta[0] = th0;
    rec[pair].theta[1] = th1 > pi ? th1 - 2.0 * pi : th1;
    rec[pair].rot_peak = three[1];
  }
}

// 9.: one workgroup per pair
__global__ __launch_bounds__(NT) void pc_peak(Dims d, Tables tb, const float2 *__restrict__ F, const float2 *__restrict__ G, const float *__restrict__ surf,
                                              const int32_t *__restrict__ pairs, int n_images, int n_cand, double resolution, double max_rotation,
                                              PairRec *__restrict__ rec, rsx_phasecorr_result *__restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pc_lds[];
  __shared__ unsigned long long red[NW];
  __shared__ double part[NW][5];
  const int t = threadIdx.x, n = d.n, mask = n - 1, n2 = n * n, pair = blockIdx.x;
  float2 *E = reinterpret_cast<float2 *>(pc_lds);
  int src, dst;
  if (!pair_ok(pairs, pair, n_images, src, dst)) {  // (uniform)
    if (t == 0) {
      out[pair] = rsx_phasecorr_result{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0, RSX_PHASECORR_STATUS_INDEX};
      rec[pair].winner = -1;
    }
    return;
  }
  load_table(E, tb.E, n, t);
  int win = 0, at = 0;
  float best = 0.0f;
  for (int c = 0; c < n_cand; c++) {
    const float *s = surf + ((size_t)pair * 2 + c) * n2;
    unsigned long long key = 0;
    for (int i = t; i < n2; i += NT) {
      const unsigned long long kk = peak_key(s[i], (unsigned)i);
      key = kk > key ? kk : key;
    }
    key = block_max_u64(key, red, t);
    const int idx = (int)(key_index(key) & (unsigned)(n2 - 1));  // (n2 is a power of two: a fence in front of the load)
    const float v = s[idx];
    if (c == 0 || v > best) {  // (a tie: theta0)
      win = c;
      at = idx;
      best = v;
    }
  }
  const int i0 = at >> d.logn, j0 = at & mask;
  const float *s = surf + ((size_t)pair * 2 + win) * n2;
  unsigned long long key = 0;
  for (int i = t; i < n2; i += NT) {
    const int di = ((i >> d.logn) - i0) & mask, dj = ((i & mask) - j0) & mask;
    if ((di <= 1 || di == mask) && (dj <= 1 || dj == mask)) continue;
    const unsigned long long kk = peak_key(s[i], (unsigned)i);
    key = kk > key ? kk : key;
  }
  key = block_max_u64(key, red, t);
  const float runner = s[key_index(key) & (unsigned)(n2 - 1)];

  // the surface at the peak and its four neighbours as direct sums of the inverse transform: fp64 over the fp32 cross-power, a thread
  // its own samples in ascending order, the wavefront by the row tree, the four wavefronts in order
  const float2 *Fd = F + (size_t)dst * n2, *g = G + ((size_t)pair * 2 + win) * n2;
  float mx = 0.0f;
  for (int b = 0; b < d.nb; b++) mx = fmaxf(mx, rec[pair].pmax[win][b]);
  double a0 = 0.0, ajp = 0.0, ajm = 0.0, aip = 0.0, aim = 0.0;
  for (int i = t; i < n2; i += NT) {
    const int v = i >> d.logn, u = i & mask;
    const float2 c = xnorm(Fd[i], g[i], mx);
    const int base = (u * j0 + v * i0) & mask;
    auto term = [&](int k) {
      const float2 e = E[k & mask];
      return (double)c.x * (double)e.x - (double)c.y * (double)e.y;
    };
    a0 = a0 + term(base);
    ajp = ajp + term(base + u);
    ajm = ajm + term(base - u);
    aip = aip + term(base + v);
    aim = aim + term(base - v);
  }
  double five[5] = {a0, ajp, ajm, aip, aim};
#pragma unroll
  for (int q = 0; q < 5; q++) five[q] = rsx::wave::sum_f64_rows_pair(five[q]);
  if ((t & 63) == 0)
    for (int q = 0; q < 5; q++) part[t >> 6][q] = five[q];
  __syncthreads();
  if (t == 0) {
    double sum[5], total = 0.0;
    for (int b = 0; b < d.nb; b++) total = total + rec[pair].psum[win][b];
    for (int q = 0; q < 5; q++) {
      double acc = 0.0;
      for (int w = 0; w < NW; w++) acc = acc + part[w][q];
      sum[q] = total > 0.0 ? acc / total : 0.0;
    }
    const double dj = parabola(sum[2], sum[0], sum[1]), di = parabola(sum[4], sum[0], sum[3]);
    const int js = j0 >= n / 2 ? j0 - n : j0, is = i0 >= n / 2 ? i0 - n : i0;
    rsx_phasecorr_result r;
    r.x = ((double)js + dj) * resolution;
    r.y = ((double)is + di) * resolution;
    r.theta = rec[pair].theta[win];
    r.peak = sum[0];
    r.peak_ratio = best != 0.0f ? (double)runner / (double)best : 0.0;
    r.rot_peak = rec[pair].rot_peak;
    r.half_turn = win;
    r.status = max_rotation > 0.0 && fabs(r.theta) > max_rotation ? RSX_PHASECORR_STATUS_ROTATION : 0;
    out[pair] = r;
    rec[pair].winner = win;
  }
}

// ---------------------------------------------------------------- host ----------------------------------------------------------------

}  // namespace

int rsx::phasecorr::check_params(const rsx_phasecorr_params &p, int rows, int cols) {
  if (p.n != 64 && p.n != 128 && p.n != 256 && p.n != 512) return fail(RSX_ERR_BAD_ARG, "n %d is not 64, 128, 256 or 512", p.n);
  if (!(p.resolution > 0.0) || !std::isfinite(p.resolution)) return fail(RSX_ERR_BAD_ARG, "resolution must be positive");
  if (!(p.range_resolution > 0.0) || !std::isfinite(p.range_resolution)) return fail(RSX_ERR_BAD_ARG, "range_resolution must be positive");
  if (p.min_range_bins < 0) return fail(RSX_ERR_BAD_ARG, "min_range_bins %d below 0", p.min_range_bins);
  if (!(p.max_rotation >= 0.0) || !std::isfinite(p.max_rotation)) return fail(RSX_ERR_BAD_ARG, "max_rotation must not be negative");
  if (rows < 1 || rows > 4096 || cols < 2 || cols > 8192) return fail(RSX_ERR_BAD_ARG, "image shape %d x %d out of range", rows, cols);
  if ((double)(p.n / 2) * p.resolution > (double)(cols - 1) * p.range_resolution)
    return fail(RSX_ERR_BAD_ARG, "the disc of %d pixels of %g m does not fit in %d range bins of %g m", p.n / 2, p.resolution, cols, p.range_resolution);
  return RSX_OK;
}

namespace {

Dims dims_of(const rsx_phasecorr_params &p, int rows, int cols) {
  Dims d;
  d.n = p.n;
  d.logn = 0;
  while ((1 << d.logn) < d.n) d.logn++;
  d.lines = 4096 / d.n < 16 ? 4096 / d.n : 16;
  d.llog = 0;
  while ((1 << d.llog) < d.lines) d.llog++;
  d.nb = d.n / d.lines;
  d.rows = rows;
  d.cols = cols;
  d.nr = d.n / 2 - R_MIN;
  return d;
}

size_t lds_bytes(const Dims &d) { return ((size_t)2 * d.lines * (d.n + 1) + d.n) * sizeof(float2); }
constexpr size_t MAX_LDS = ((size_t)2 * 8 * 513 + 512) * 8;  // N = 512; N = 256 takes 67840, the smaller sizes less

// byte offsets of the tables in h->tables
struct TableLayout {
  size_t map, E, dirs, hann, hp, total;
  explicit TableLayout(int n) {
    map = 0;
    E = map + (size_t)n * n * 8;
    dirs = E + (size_t)n * 8;
    hann = dirs + (size_t)n * 8;
    hp = hann + (size_t)n * 4;
    total = hp + (size_t)n * 4;
  }
};

Tables tables_of(const void *d_tables, int n) {
  const TableLayout L(n);
  const unsigned char *b = static_cast<const unsigned char *>(d_tables);
  return Tables{reinterpret_cast<const float2 *>(b + L.map), reinterpret_cast<const float2 *>(b + L.E), reinterpret_cast<const float2 *>(b + L.dirs),
                reinterpret_cast<const float *>(b + L.hann), reinterpret_cast<const float *>(b + L.hp)};
}

// the tables of tests/phasecorr_np.py (Tables, cos_sin_table): fp64, the same expressions in the same order, one rounding to fp32
void fill_tables(const rsx_phasecorr_params &p, int rows, int cols, std::vector<unsigned char> &buf) {
  const int n = p.n, h = n / 2;
  const TableLayout L(n);
  buf.assign(L.total, 0);
  float *map = reinterpret_cast<float *>(buf.data() + L.map), *E = reinterpret_cast<float *>(buf.data() + L.E);
  float *dirs = reinterpret_cast<float *>(buf.data() + L.dirs), *hann = reinterpret_cast<float *>(buf.data() + L.hann);
  float *hp = reinterpret_cast<float *>(buf.data() + L.hp);
  const double pi = 3.14159265358979323846, res = p.resolution, rres = p.range_resolution, rho_max = (double)(h - 1) * res;
  for (int i = 0; i < n; i++) {
    const double y = (double)(i - h) * res;
    for (int j = 0; j < n; j++) {
      const double x = (double)(j - h) * res, rho = std::sqrt(x * x + y * y), rc = rho / rres - 0.5;
      float *m = map + ((size_t)i * n + j) * 2;
      m[0] = -1.0f;
      m[1] = 0.0f;
      if (rho > rho_max || rc < 0.0 || rc < (double)p.min_range_bins || rc > (double)(cols - 1)) continue;
      double phi = std::atan2(y, x);
      if (phi < 0.0) phi += 2.0 * pi;
      const float a = (float)(phi * (double)rows / (2.0 * pi));
      m[0] = (float)rc;
      m[1] = a < (float)rows ? a : 0.0f;
    }
  }
  std::vector<float> q((size_t)n / 4 + 1);
  for (int k = 0; k <= n / 4; k++) q[k] = (float)std::cos(2.0 * pi * (double)k / (double)n);
  q[n / 4] = 0.0f;
  auto c = [&](int k) {
    k = ((k % n) + n) % n;
    if (k > n / 2) k = n - k;
    return k > n / 4 ? -q[n / 2 - k] : q[k];
  };
  for (int k = 0; k < n; k++) {
    E[2 * k] = c(k);
    E[2 * k + 1] = c(k - n / 4);
    dirs[2 * k] = (float)std::cos(pi * (double)k / (double)n);
    dirs[2 * k + 1] = (float)std::sin(pi * (double)k / (double)n);
    hann[k] = (float)(0.5 - 0.5 * std::cos(2.0 * pi * (double)k / (double)n));
    hp[k] = (float)std::cos(pi * (double)(k - h) / (double)n);
  }
}

int check_batch(const rsx_phasecorr *h, int32_t n_images, int64_t image_stride, int32_t row_stride, int32_t col_offset, int32_t n_pairs) {
  if (n_images < 1 || n_images > MAX_IMAGES) return fail(RSX_ERR_BAD_ARG, "n_images %d outside 1 .. %d", n_images, MAX_IMAGES);
  if (n_pairs < 0 || n_pairs > MAX_PAIRS) return fail(RSX_ERR_BAD_ARG, "n_pairs %d outside 0 .. %d", n_pairs, MAX_PAIRS);
  if (col_offset < 0 || (int64_t)row_stride < (int64_t)col_offset + h->cols)
    return fail(RSX_ERR_BAD_ARG, "row_stride %d does not hold %d samples behind col_offset %d", row_stride, h->cols, col_offset);
  if (n_images > 1 && image_stride < (int64_t)h->rows * row_stride) return fail(RSX_ERR_BAD_ARG, "image_stride_bytes %lld below rows x row_stride", (long long)image_stride);
  return RSX_OK;
}

}  // namespace

namespace rsx {
namespace phasecorr {

void workspace_bytes(int n, size_t *per_scan_F, size_t *per_scan_A, size_t *per_pair) {
  const size_t n2 = (size_t)n * n;
  if (per_scan_F) *per_scan_F = n2 * 8;
  if (per_scan_A) *per_scan_A = (size_t)(n / 2 - R_MIN) * n * 8;
  if (per_pair) *per_pair = 40 * n2 + sizeof(PairRec) + (size_t)n * 4;
}

int make_tables(const rsx_phasecorr_params &p, int rows, int cols, rsx::DevBuf &tables, hipStream_t s) {
  std::vector<unsigned char> buf;
  fill_tables(p, rows, cols, buf);
  RSX_TRY(tables.reserve(buf.size(), s, false));
  RSX_HIP(hipMemcpy(tables.p, buf.data(), buf.size(), hipMemcpyHostToDevice));
  const int lds = (int)MAX_LDS;  // (the attribute belongs to the kernel, not to the handle: the largest any handle launches with)
  RSX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&pc_rows_fwd), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  RSX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&pc_cols<0>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  RSX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&pc_cols<1>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  RSX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&pc_cols<2>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  RSX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&pc_rows_inv), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  RSX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&pc_polar), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  RSX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&pc_rotation), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  return RSX_OK;
}

// launches 1 - 3
int launch_spectra(const rsx_phasecorr_params &p, int rows, int cols, const void *d_tables, const Images &im, int32_t n_scans, float2 *d_F, float2 *d_A,
                   float *d_cart, hipStream_t s) {
  if (n_scans <= 0) return RSX_OK;
  const Dims d = dims_of(p, rows, cols);
  const Tables tb = tables_of(d_tables, d.n);
  const Scans sc{im.d_imgs, im.image_stride, n_scans, n_scans, im.row_stride, im.col_offset, 0};
  const size_t lds = lds_bytes(d);
  const dim3 blk(NT), per_scan((unsigned)d.nb, (unsigned)n_scans);
  hipLaunchKernelGGL(pc_rows_fwd, per_scan, blk, lds, s, d, tb, sc, (const int32_t *)nullptr, (const PairRec *)nullptr, 1, d_F, d_cart);
  hipLaunchKernelGGL(pc_cols<0>, per_scan, blk, lds, s, d, tb, d_F, (const float2 *)nullptr, (const int32_t *)nullptr, n_scans, (PairRec *)nullptr, 1,
                     (float2 *)nullptr);
  hipLaunchKernelGGL(pc_polar, dim3((unsigned)((d.nr + d.lines - 1) / d.lines), (unsigned)n_scans), blk, lds, s, d, tb, d_F, d_A);
  RSX_HIP(hipGetLastError());
  return RSX_OK;
}

// launches 4 - 9
int launch_pairs(const rsx_phasecorr_params &p, int rows, int cols, const void *d_tables, const Images &im, int32_t n_images, int32_t image_offset,
                 const float2 *d_F, const float2 *d_A, int32_t n_slots, const int32_t *d_pairs, int32_t n_pairs, void *d_pair_work,
                 rsx_phasecorr_result *d_results, hipStream_t s) {
  if (n_pairs <= 0) return RSX_OK;
  const Dims d = dims_of(p, rows, cols);
  const Layout L(d, 0, n_pairs);  // (no scans: the offsets of the pairs' pieces from the first of them)
  unsigned char *b = static_cast<unsigned char *>(d_pair_work);
  float2 *G = reinterpret_cast<float2 *>(b + L.G), *W = reinterpret_cast<float2 *>(b + L.W);
  float *surf = reinterpret_cast<float *>(b + L.surf), *curve = reinterpret_cast<float *>(b + L.curve);
  PairRec *rec = reinterpret_cast<PairRec *>(b + L.rec);
  const Tables tb = tables_of(d_tables, d.n);
  const Scans sc{im.d_imgs, im.image_stride, n_images, n_slots, im.row_stride, im.col_offset, image_offset};
  const size_t lds = lds_bytes(d);
  const int n_cand = p.resolve_half_turn ? 2 : 1;
  const dim3 blk(NT), per_cand((unsigned)d.nb, (unsigned)(2 * n_pairs));
  hipLaunchKernelGGL(pc_rotation, dim3((unsigned)n_pairs), blk, lds, s, d, tb, d_A, d_pairs, n_slots, rec, curve);
  hipLaunchKernelGGL(pc_rows_fwd, per_cand, blk, lds, s, d, tb, sc, d_pairs, rec, n_cand, G, (float *)nullptr);
  hipLaunchKernelGGL(pc_cols<1>, per_cand, blk, lds, s, d, tb, G, d_F, d_pairs, n_slots, rec, n_cand, (float2 *)nullptr);
  hipLaunchKernelGGL(pc_cols<2>, per_cand, blk, lds, s, d, tb, G, d_F, d_pairs, n_slots, rec, n_cand, W);
  hipLaunchKernelGGL(pc_rows_inv, per_cand, blk, lds, s, d, tb, W, d_pairs, n_slots, n_cand, rec, surf);
  hipLaunchKernelGGL(pc_peak, dim3((unsigned)n_pairs), blk, (size_t)d.n * sizeof(float2), s, d, tb, d_F, G, surf, d_pairs, n_slots, n_cand, p.resolution,
                     p.max_rotation, rec, d_results);
  RSX_HIP(hipGetLastError());
  return RSX_OK;
}

}  // namespace phasecorr
}  // namespace rsx

namespace {

// both stand-alone entries: the two stages in a row on the handle's own workspace, which grows here (the caller holds h->mu and has
// entered s)
int run(rsx_phasecorr *h, const uint8_t *d_imgs, int32_t n_images, int64_t image_stride, int32_t row_stride, int32_t col_offset, const int32_t *d_pairs,
        int32_t n_pairs, rsx_phasecorr_result *d_results, float *d_cart, hipStream_t s) {
  const Dims d = dims_of(h->p, h->rows, h->cols);
  const Layout L(d, n_images, n_pairs);
  RSX_TRY(h->work.reserve(L.total, s, false));
  h->last_images = n_images;
  h->last_pairs = n_pairs;
  unsigned char *b = h->work.as<unsigned char>();
  float2 *F = reinterpret_cast<float2 *>(b + L.F), *A = reinterpret_cast<float2 *>(b + L.A);
  const Images im{d_imgs, image_stride, row_stride, col_offset};
  RSX_TRY(launch_spectra(h->p, h->rows, h->cols, h->tables.p, im, n_images, F, A, d_cart, s));
  return launch_pairs(h->p, h->rows, h->cols, h->tables.p, im, n_images, 0, F, A, n_images, d_pairs, n_pairs, b + L.G, d_results, s);
}

}  // namespace

extern "C" {

int rsx_phasecorr_default_params(rsx_phasecorr_params *p) try {
  if (!p) return fail(RSX_ERR_BAD_ARG, "null params");
  p->n = 256;
  p->min_range_bins = 58;
  p->resolution = 0.5;
  p->range_resolution = 0.0595;
  p->max_rotation = 0.0;
  p->resolve_half_turn = 1;
  p->reserved = 0;
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_phasecorr_create(int device, int32_t rows, int32_t cols, const rsx_phasecorr_params *params, rsx_phasecorr **out) try {
  if (!out) return fail(RSX_ERR_BAD_ARG, "null out");
  *out = nullptr;
  rsx_phasecorr_params dp;
  rsx_phasecorr_default_params(&dp);
  if (params) dp = *params;
  RSX_TRY(check_params(dp, rows, cols));  // (judged before the device is looked at: the rules need none)
  RSX_TRY(rsx::check_device(device));
  std::unique_ptr<rsx_phasecorr> h(new (std::nothrow) rsx_phasecorr());
  if (!h) return fail(RSX_ERR_OOM, "host alloc");
  h->device = device;
  h->p = dp;
  h->rows = rows;
  h->cols = cols;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = h->stream.create();
  if (e != hipSuccess) return fail(RSX_ERR_HIP, "create: %s", hipGetErrorString(e));
  RSX_TRY(make_tables(dp, rows, cols, h->tables, h->stream));
  *out = h.release();
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_phasecorr_destroy(rsx_phasecorr *h) try {
  if (!h) return RSX_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  delete h;
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_phasecorr_register_batch_device(rsx_phasecorr *h, const uint8_t *d_imgs, int32_t n_images, int64_t image_stride_bytes, int32_t row_stride,
                                        int32_t col_offset, const int32_t *d_pairs, int32_t n_pairs, rsx_phasecorr_result *d_results, float *d_cart,
                                        void *stream) try {
  if (!h) return fail(RSX_ERR_BAD_ARG, "null handle");
  if (!d_imgs || (n_pairs > 0 && (!d_pairs || !d_results))) return fail(RSX_ERR_BAD_ARG, "null arg");
  RSX_TRY(check_batch(h, n_images, image_stride_bytes, row_stride, col_offset, n_pairs));
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
  RSX_TRY(h->order.enter(s));
  return run(h, d_imgs, n_images, image_stride_bytes, row_stride, col_offset, d_pairs, n_pairs, d_results, d_cart, s);
} RSX_CATCH_ALL

int rsx_phasecorr_register_batch(rsx_phasecorr *h, const uint8_t *imgs, int32_t n_images, int64_t image_stride_bytes, int32_t row_stride,
                                 int32_t col_offset, const int32_t *pairs, int32_t n_pairs, rsx_phasecorr_result *out_results, float *out_cart) try {
  if (!h) return fail(RSX_ERR_BAD_ARG, "null handle");
  if (!imgs || (n_pairs > 0 && (!pairs || !out_results))) return fail(RSX_ERR_BAD_ARG, "null arg");
  RSX_TRY(check_batch(h, n_images, image_stride_bytes, row_stride, col_offset, n_pairs));
  for (int32_t i = 0; i < 2 * n_pairs; i++)
    if (pairs[i] < 0 || pairs[i] >= n_images)
      return fail(RSX_ERR_BAD_ARG, "pair %d names image %d outside the batch of %d", i / 2, pairs[i], n_images);
  const size_t ib = (size_t)(n_images - 1) * (size_t)image_stride_bytes + (size_t)h->rows * (size_t)row_stride;
  const size_t pb = (size_t)n_pairs * 8, rb = (size_t)n_pairs * sizeof(rsx_phasecorr_result), cb = (size_t)n_images * h->p.n * h->p.n * 4;
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  RSX_TRY(h->order.enter(s));
  RSX_TRY(rsx::stage_up(h->imgs, imgs, ib, s));
  RSX_TRY(rsx::stage_up(h->pairs, pairs, pb, s));
  RSX_TRY(rsx::stage_room(h->res, rb, s));
  if (out_cart) RSX_TRY(rsx::stage_room(h->cart, cb, s));
  RSX_TRY(run(h, h->imgs.as<uint8_t>(), n_images, image_stride_bytes, row_stride, col_offset, h->pairs.as<int32_t>(), n_pairs,
              h->res.as<rsx_phasecorr_result>(), out_cart ? h->cart.as<float>() : nullptr, s));
  RSX_TRY(rsx::stage_down(out_results, h->res, rb, s));
  if (out_cart) RSX_TRY(rsx::stage_down(out_cart, h->cart, cb, s));
  RSX_HIP(hipStreamSynchronize(s));
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_phasecorr_correlation(rsx_phasecorr *h, int32_t pair, float *out_rot_curve, float *out_surface) try {
  if (!h) return fail(RSX_ERR_BAD_ARG, "null handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (pair < 0 || pair >= h->last_pairs) return fail(RSX_ERR_BAD_ARG, "pair %d outside the %d pairs of the last call", pair, h->last_pairs < 0 ? 0 : h->last_pairs);
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  RSX_TRY(h->order.enter(s));
  const Dims d = dims_of(h->p, h->rows, h->cols);
  const Layout L(d, h->last_images, h->last_pairs);
  const unsigned char *b = h->work.as<unsigned char>();
  PairRec rec;
  RSX_HIP(hipMemcpyAsync(&rec, b + L.rec + (size_t)pair * sizeof(PairRec), sizeof(PairRec), hipMemcpyDeviceToHost, s));
  RSX_HIP(hipStreamSynchronize(s));
  if (rec.winner < 0 || rec.winner > 1) return fail(RSX_ERR_BAD_ARG, "pair %d was not computed (an index outside the batch)", pair);
  const size_t n2 = (size_t)d.n * d.n;
  if (out_rot_curve) RSX_HIP(hipMemcpyAsync(out_rot_curve, b + L.curve + (size_t)pair * d.n * 4, (size_t)d.n * 4, hipMemcpyDeviceToHost, s));
  if (out_surface) RSX_HIP(hipMemcpyAsync(out_surface, b + L.surf + ((size_t)pair * 2 + rec.winner) * n2 * 4, n2 * 4, hipMemcpyDeviceToHost, s));
  RSX_HIP(hipStreamSynchronize(s));
  return RSX_OK;
} RSX_CATCH_ALL

}  // extern "C"
