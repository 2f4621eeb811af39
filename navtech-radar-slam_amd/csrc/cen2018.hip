// cen2018.hip -- cen2018 radar keypoint extraction (Cen & Newman, ICRA 2018) on gfx950, batched.
//
// The second keypoint extractor of the upstream file-based odometry entry (yeti_radar_odometry through ORORA; its
// `keypoint_extraction` = 0 and yeti's own default).  The upstream source is absent from the reference checkout (empty
// ORORA submodule), so this follows the method as recalled and pinned in tests/cen2018_np.py (PARITY UNPINNED):
// per azimuth row, q = fft - mean, p = q smoothed along range by a 1 x 3 sigma_gauss Gaussian (reflect 101), the noise
// sigma from the negative q, y = q (1 - nqp) + p (nqp - npp) with nqp / npp Gaussian likelihoods of q - p and p, and one
// keypoint at the median of every run of consecutive range bins (>= min_range) with y > zq * sigma.
//
// Launch chain of a batch (no host synchronisation, two launches per sub-batch of <= 128 images):
//   c18_rows   one WAVEFRONT per (azimuth, image): the row's bytes once into LDS (+ 256-bin histogram, byte sum),
//              mean, q per byte value, sigma from the histogram (fp64, bins ascending), q of the reflect-101-extended row
//              into LDS, the smoothing (each lane two range bins 64 apart per step, packed fp32), the screen and the
//              threshold, per-chunk ballots of the decisions -> runs and their medians (scalar bit scans) -> per-row
//              keypoints + per-row count
//   kp_pack    (keypoints_host.h, shared with cen2019) one wavefront per (azimuth, image): row-major packing of the rows'
//              keypoints + polar -> Cartesian
// Arithmetic: every fp32 operation separately rounded (-ffp-contract=off, explicit __f*_rn), the smoothing in ascending
// tap order, sigma's sum sequential in fp64 over the byte values ascending: bit-identical to the restatement up to the
// two fp64 exp per pixel (a device exp and a host exp may differ by an ulp; see tests/test_gpu_cen2018.py).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <new>

#include "cen2018.h"
#include "keypoints_host.h"
#include "rsx_wave_dev.h"

namespace {

constexpr int MAX_TAPS = 255;       // fsize = 3 sigma_gauss: sigma_gauss <= 85
constexpr int MAX_COLS = 8192;      // LDS of c18_rows: 4 (cols + 128 + 255) + cols + 2048 bytes <= 43 KB
constexpr int MAX_ROWS = 4096;
constexpr float SIGMA_NONE = 0.034f;  // sigma of a row without a negative q (upstream's fallback)

struct Taps {  // passed by value: every lane reads w[k] at the same k, a uniform load from the kernel arguments
  float w[MAX_TAPS + 1];
};

typedef float c18_f2 __attribute__((ext_vector_type(2)));

// repeated reflect 101 (period 2 (cols - 1)); cols == 1: 0
__device__ __forceinline__ int refl101(int x, int cols) {
  if (x >= 0 && x < cols) return x;
  if (cols == 1) return 0;
  const int P = 2 * (cols - 1);
  int m = x % P;
  if (m < 0) m += P;
  return m < cols ? m : P - m;
}

// correctly rounded sqrt of a positive normal float: __fsqrt_rn compiles to v_sqrt_f32 here (1 ulp), so the hardware estimate
// is corrected like the compiler's own IEEE expansion -- one step down if (s - ulp) s >= x, one step up if (s + ulp) s < x,
// both residuals exact by fma
__device__ __forceinline__ float sqrt_rn(float x) {
  float s = __builtin_amdgcn_sqrtf(x);
  const float dn = __uint_as_float(__float_as_uint(s) - 1u), up = __uint_as_float(__float_as_uint(s) + 1u);
  const float rdn = __fmaf_rn(-dn, s, x), rup = __fmaf_rn(-up, s, x);
  s = rdn <= 0.0f ? dn : s;
  s = rup > 0.0f ? up : s;
  return s;
}

// y of one pixel (pinned: every op rounded on its own, the two exp in fp64)
__device__ __forceinline__ float c18_y(float q, float p, float sigma) {
  const float d1 = __fdiv_rn(__fsub_rn(q, p), sigma), d2 = __fdiv_rn(p, sigma);
  const double e1 = (double)d1, e2 = (double)d2;
  const float nqp = (float)exp(-0.5 * e1 * e1), npp = (float)exp(-0.5 * e2 * e2);
  const float b = __fsub_rn(nqp, npp);
  return __fadd_rn(__fmul_rn(q, __fsub_rn(1.0f, nqp)), __fmul_rn(p, b));
}

// the decision of one pixel.  Screen: (1 - nqp) and b lie in [-1, 1] and rounding is monotone, so |y| <= RN(|q| + |p|);
// when that is <= thres, y > thres is false and both exp are skipped (not a single decision changes)
template <bool DIAG>
__device__ __forceinline__ bool c18_hit(float q, float p, float sigma, float thres, bool in_range, float &y) {
  y = 0.0f;
  if (DIAG) {
    y = c18_y(q, p, sigma);
    return in_range && y > thres;
  }
  if (!in_range || !(__fadd_rn(fabsf(q), fabsf(p)) > thres)) return false;
  y = c18_y(q, p, sigma);
  return y > thres;
}

// LDS of one wavefront (dynamic): hist[256] u32 | qtab[256] f32 | qx[nx] f32 | bytes[cols]
__host__ __device__ inline int c18_nx(int cols, int fsize) { return 128 * (((cols + 63) / 64 + 1) / 2) + fsize - 1; }
__host__ __device__ inline size_t c18_lds_bytes(int cols, int fsize) { return 2048 + 4 * (size_t)c18_nx(cols, fsize) + (size_t)((cols + 3) & ~3); }

// one wavefront per (azimuth blockIdx.x, image blockIdx.y).  DIAG (rsx_cen2018_debug_image): the same steps, y for every
// pixel (no screen) and mean / sigma / p / y stored
template <bool DIAG>
__global__ __launch_bounds__(64) void c18_rows(const uint8_t *__restrict__ imgs, int64_t img_stride, int rows, int cols, int stride, int off,
                                               Taps taps, int fsize, float zq, int min_range, int row_cap, uint16_t *__restrict__ row_kp,
                                               unsigned *__restrict__ row_n, float *__restrict__ d_mean, float *__restrict__ d_sigma,
                                               float *__restrict__ d_p, float *__restrict__ d_y) {
  extern __shared__ __attribute__((aligned(16))) unsigned char c18_lds[];
  unsigned *hist = reinterpret_cast<unsigned *>(c18_lds);
  float *qtab = reinterpret_cast<float *>(c18_lds + 1024);
  float *qx = reinterpret_cast<float *>(c18_lds + 2048);
  const int nx = c18_nx(cols, fsize);
  uint8_t *bytes = c18_lds + 2048 + 4 * (size_t)nx;
  const int lane = threadIdx.x, a = blockIdx.x, img = blockIdx.y;
  const uint8_t *row = imgs + (int64_t)img * img_stride + (int64_t)a * stride + off;

  // ---- the row's bytes (once), their histogram and sum ----
#pragma unroll
  for (int b = lane; b < 256; b += 64) hist[b] = 0u;
  __syncthreads();
  unsigned sum = 0;
  for (int x = lane; x < cols; x += 64) {
    const unsigned b = row[x];
    bytes[x] = (uint8_t)b;
    atomicAdd(&hist[b], 1u);
    sum += b;
  }
  sum = rsx::wave::butterfly(sum, rsx::wave::Add{});  // (measured: the DPP sum_i32 here was 0.3 % slower per scan, so the shuffles stay)
  const float mean = (float)((double)sum / 255.0 / (double)cols);
  // q depends on the byte value only; q_b is non-decreasing in b, so q_b < 0 exactly for b < T
  unsigned T = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int b = lane + 64 * i;
    const float q = __fsub_rn(__fdiv_rn((float)b, 255.0f), mean);
    qtab[b] = q;
    T += (unsigned)__popcll(__ballot(q < 0.0f));
  }
  __syncthreads();
  // ---- sigma: S = sum over b < T ascending of c_b (2 q_b^2), sequential in fp64 (every lane the same, uniform reads) ----
  double S = 0.0;
  unsigned n = 0;
  for (unsigned b = 0; b < T; b++) {
    const unsigned c = hist[b];
    const double qd = (double)qtab[b];
    S = S + (double)c * (2.0 * qd * qd);
    n += c;
  }
  const float sigma = n ? sqrt_rn((float)(S / (double)n)) : SIGMA_NONE;  // (S / n: a normal float)
  const float thres = __fmul_rn(zq, sigma);
  // ---- q of the reflect-101-extended row: qx[x + mu] = q[refl(x)]; past cols - 1 + mu: padding for the lanes past the row ----
  const int mu = fsize / 2;
  for (int xx = lane; xx < nx; xx += 64) {
    const int x = xx - mu;
    qx[xx] = x < cols + mu ? qtab[bytes[refl101(x, cols)]] : 0.0f;
  }
  __syncthreads();
  // ---- smoothing, decisions, runs: lane l takes range bins 128 c + l and 128 c + 64 + l, so that a ballot is 64 consecutive bins ----
  const int npair = ((cols + 63) / 64 + 1) / 2;
  uint16_t *kp = row_kp + ((int64_t)img * rows + a) * row_cap;
  int open = -1;  // first bin of the run still open (-1: none)
  unsigned nk = 0;
  auto emit = [&](int s, int e) {
    const int med = s + (e - s + 1) / 2;
    if (nk < (unsigned)row_cap && lane == 0) kp[nk] = (uint16_t)med;
    nk++;
  };
  auto scan = [&](unsigned long long m, int base) {  // (wave-uniform) the runs of one chunk's decisions
    int pos = 0;
    while (pos < 64) {
      if (open < 0) {
        const unsigned long long rest = m >> pos;
        if (!rest) return;
        pos += __builtin_ctzll(rest);
        open = base + pos;
      }
      const unsigned long long zeros = ~m >> pos;  // (pos < 64 here)
      if (!zeros) return;                          // the run goes on into the next chunk
      pos += __builtin_ctzll(zeros);
      emit(open, base + pos - 1);
      open = -1;
    }
  };
  for (int c = 0; c < npair; c++) {
    const int j0 = 128 * c + lane, j1 = j0 + 64;
    const float *qa = qx + j0;
    c18_f2 acc = {0.0f, 0.0f};
#pragma unroll 4
    for (int k = 0; k < fsize; k++) {
      const c18_f2 wv = {taps.w[k], taps.w[k]};
      const c18_f2 xv = {qa[k], qa[k + 64]};
      acc = acc + wv * xv;  // v_pk_mul_f32 + v_pk_add_f32: each element rounded on its own
    }
    const float q0 = qx[j0 + mu], q1 = qx[j1 + mu];
    float y0, y1;
    const bool h0 = c18_hit<DIAG>(q0, acc.x, sigma, thres, j0 >= min_range && j0 < cols, y0);
    const bool h1 = c18_hit<DIAG>(q1, acc.y, sigma, thres, j1 >= min_range && j1 < cols, y1);
    if (DIAG) {
      const int64_t o = (int64_t)a * cols;
      if (j0 < cols) {
        d_p[o + j0] = acc.x;
        d_y[o + j0] = y0;
      }
      if (j1 < cols) {
        d_p[o + j1] = acc.y;
        d_y[o + j1] = y1;
      }
    }
    const unsigned long long m0 = __ballot(h0), m1 = __ballot(h1);
    scan(m0, 128 * c);
    scan(m1, 128 * c + 64);
  }
  if (open >= 0) emit(open, cols - 1);  // a run that reaches the last bin
  if (lane == 0) {
    row_n[(int64_t)img * rows + a] = nk;
    if (DIAG) {
      d_mean[a] = mean;
      d_sigma[a] = sigma;
    }
  }
}

// the Gaussian of step 2 on the host: libm exp in double, float sum ascending, float division
void gauss_weights(int sigma_gauss, float *w) {
  const int fsize = 3 * sigma_gauss, mu = fsize / 2;
  const float sig_sqr = (float)(sigma_gauss * sigma_gauss);
  float s = 0.0f;
  for (int k = 0; k < fsize; k++) {
    w[k] = (float)std::exp(-0.5 * (double)(k - mu) * (double)(k - mu) / (double)sig_sqr);
    s = s + w[k];
  }
  for (int k = 0; k < fsize; k++) w[k] = w[k] / s;
}

}  // namespace

struct rsx_cen2018 : rsx::KeypointHandle {
  rsx::DevBuf row_kp, row_n, dbg;
};

using rsx::fail;

int rsx::cen2018_check_params(const rsx_cen2018_params &p) {
  if (p.sigma_gauss < 1 || p.sigma_gauss % 2 == 0 || 3 * p.sigma_gauss > MAX_TAPS)
    return fail(RSX_ERR_BAD_ARG, "sigma_gauss %d: must be odd, in [1, %d]", p.sigma_gauss, MAX_TAPS / 3);
  if (p.min_range < 0) return fail(RSX_ERR_BAD_ARG, "min_range %d < 0", p.min_range);
  if (!std::isfinite(p.zq)) return fail(RSX_ERR_BAD_ARG, "zq is not finite");
  return RSX_OK;
}

namespace {

// the resolve step of the scaffold (keypoints_host.h): the defaults, *params over them, the check
int get_params(const rsx_cen2018_params *params, rsx_cen2018_params *p) {
  rsx_cen2018_default_params(p);
  if (params) *p = *params;
  return rsx::cen2018_check_params(*p);
}

Taps make_taps(const rsx_cen2018_params &p) {
  Taps t{};
  gauss_weights(p.sigma_gauss, t.w);
  return t;
}

// d_imgs: nb device images img_stride bytes apart -> d_targets [nb][max_targets][2], d_xy (optional, needs d_az), d_counts
// (optional).  Two launches per sub-batch (rsx::rows_then_pack), nothing read on the host.
int extract_device(rsx_cen2018 *h, const uint8_t *d_imgs, int64_t img_stride, int nb, int32_t stride, int32_t off, const rsx_cen2018_params &p,
                   const float *d_az, int64_t az_stride, float resolution, int32_t max_targets, int *d_targets, float *d_xy, int *d_counts,
                   hipStream_t s) {
  const int rows = h->rows, cols = h->cols;
  const int row_cap = cols / 2 + 1;  // a row of `cols` bins holds at most ceil(cols / 2) runs
  const Taps taps = make_taps(p);
  const int fsize = 3 * p.sigma_gauss;
  const size_t lds = c18_lds_bytes(cols, fsize);
  return rsx::rows_then_pack(h, row_cap, nb, d_az, az_stride, resolution, max_targets, d_targets, d_xy, d_counts, s, [&](int b0, int n) {
    hipLaunchKernelGGL(c18_rows<false>, dim3((unsigned)rows, (unsigned)n), dim3(64), lds, s, d_imgs + (int64_t)b0 * img_stride, img_stride, rows, cols,
                       stride, off, taps, fsize, p.zq, p.min_range, row_cap, h->row_kp.as<uint16_t>(), h->row_n.as<unsigned>(), nullptr, nullptr,
                       nullptr, nullptr);
  });
}

}  // namespace

extern "C" {

int rsx_cen2018_default_params(rsx_cen2018_params *p) try {
  if (!p) return fail(RSX_ERR_BAD_ARG, "null params");
  p->zq = 3.0f;  // yeti_radar_odometry defaults for cen2018 (recollection)
  p->sigma_gauss = 17;
  p->min_range = 58;
  p->reserved = 0;
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_cen2018_create(int device, int32_t rows, int32_t cols, rsx_cen2018 **out) try {
  return rsx::keypoints_create(rows >= 1 && rows <= MAX_ROWS && cols >= 1 && cols <= MAX_COLS, device, rows, cols, out);
} RSX_CATCH_ALL

int rsx_cen2018_destroy(rsx_cen2018 *h) try {
  return rsx::keypoints_destroy(h);
} RSX_CATCH_ALL

int rsx_cen2018_extract_batch_device(rsx_cen2018 *h, const uint8_t *d_imgs, int32_t n_images, int64_t image_stride_bytes, int32_t row_stride,
                                     int32_t col_offset, const rsx_cen2018_params *params, const float *d_azimuths,
                                     int32_t azimuths_per_image, float resolution, int32_t *d_targets, float *d_xy, int32_t max_targets,
                                     int32_t *d_counts, void *stream) try {
  return rsx::keypoints_extract_batch_device(h, get_params, extract_device, d_imgs, n_images, image_stride_bytes, row_stride, col_offset, params,
                                             d_azimuths, azimuths_per_image, resolution, d_targets, d_xy, max_targets, d_counts, stream);
} RSX_CATCH_ALL

int rsx_cen2018_extract_batch(rsx_cen2018 *h, const uint8_t *imgs, int32_t n_images, int64_t image_stride_bytes, int32_t row_stride,
                              int32_t col_offset, const rsx_cen2018_params *params, const float *azimuths, int32_t azimuths_per_image,
                              float resolution, int32_t *out_targets, float *out_xy, int32_t max_targets, int32_t *out_counts) try {
  return rsx::keypoints_extract_batch(h, get_params, extract_device, imgs, n_images, image_stride_bytes, row_stride, col_offset, params, azimuths,
                                      azimuths_per_image, resolution, out_targets, out_xy, max_targets, out_counts);
} RSX_CATCH_ALL

int rsx_cen2018_extract(rsx_cen2018 *h, const uint8_t *img, int32_t row_stride, int32_t col_offset, const rsx_cen2018_params *params,
                        const float *azimuths, float resolution, int32_t *out_targets, float *out_xy, int32_t max_targets,
                        int32_t *out_count) try {
  return rsx::keypoints_extract(h, get_params, extract_device, img, row_stride, col_offset, params, azimuths, resolution, out_targets, out_xy,
                                max_targets, out_count);
} RSX_CATCH_ALL

int rsx_cen2018_gauss_weights(int32_t sigma_gauss, float *out, int32_t max) try {
  rsx_cen2018_params p;
  rsx_cen2018_default_params(&p);
  p.sigma_gauss = sigma_gauss;
  RSX_TRY(rsx::cen2018_check_params(p));
  if (!out || max < 3 * sigma_gauss) return fail(RSX_ERR_BAD_ARG, "out holds %d of %d taps", max, 3 * sigma_gauss);
  gauss_weights(sigma_gauss, out);
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_cen2018_debug_image(rsx_cen2018 *h, const uint8_t *img, int32_t row_stride, int32_t col_offset, const rsx_cen2018_params *params,
                            float *out_mean, float *out_sigma, float *out_p, float *out_y) try {
  if (!h || !img || !out_mean || !out_sigma || !out_p || !out_y) return fail(RSX_ERR_BAD_ARG, "bad arg");
  RSX_TRY(rsx::check_polar_layout(h->rows, h->cols, 1, 0, row_stride, col_offset));
  rsx_cen2018_params p;
  RSX_TRY(get_params(params, &p));
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  RSX_TRY(h->order.enter(s));
  const int rows = h->rows, cols = h->cols, row_cap = cols / 2 + 1, fsize = 3 * p.sigma_gauss;
  const size_t ibytes = (size_t)rows * row_stride, px = (size_t)rows * cols * 4;
  RSX_TRY(h->stage.img.reserve(ibytes, s, false));
  RSX_TRY(h->row_kp.reserve((size_t)rows * row_cap * 2, s, false));
  RSX_TRY(h->row_n.reserve((size_t)rows * 4, s, false));
  RSX_TRY(h->dbg.reserve(2 * px + (size_t)rows * 8, s, false));
  RSX_HIP(hipMemcpyAsync(h->stage.img.p, img, ibytes, hipMemcpyHostToDevice, s));
  float *dp = h->dbg.as<float>(), *dy = dp + (size_t)rows * cols, *dm = dy + (size_t)rows * cols, *ds = dm + rows;
  hipLaunchKernelGGL(c18_rows<true>, dim3((unsigned)rows, 1u), dim3(64), c18_lds_bytes(cols, fsize), s, h->stage.img.as<uint8_t>(), (int64_t)ibytes, rows, cols,
                     row_stride, col_offset, make_taps(p), fsize, p.zq, p.min_range, row_cap, h->row_kp.as<uint16_t>(), h->row_n.as<unsigned>(), dm, ds,
                     dp, dy);
  RSX_HIP(hipGetLastError());
  RSX_HIP(hipMemcpyAsync(out_p, dp, px, hipMemcpyDeviceToHost, s));
  RSX_HIP(hipMemcpyAsync(out_y, dy, px, hipMemcpyDeviceToHost, s));
  RSX_HIP(hipMemcpyAsync(out_mean, dm, (size_t)rows * 4, hipMemcpyDeviceToHost, s));
  RSX_HIP(hipMemcpyAsync(out_sigma, ds, (size_t)rows * 4, hipMemcpyDeviceToHost, s));
  RSX_HIP(hipStreamSynchronize(s));
  return RSX_OK;
} RSX_CATCH_ALL

}  // extern "C"
