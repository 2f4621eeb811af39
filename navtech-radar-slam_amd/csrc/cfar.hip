// cfar.hip -- CA-CFAR / BFAR radar keypoint extraction on gfx950, batched: per azimuth row the k strongest returns that exceed
// an affine function of the noise AROUND them, T = a Z + b (BFAR; b = 0 is cell-averaging CFAR, a = 0 the fixed floor of
// k-strongest), with the greatest-of and smallest-of variants of the noise estimate.
//
// The rule is integer arithmetic only (include/rsx.h, restated in tests/cfar_np.py).  t = train, g = guard, A = scale_q8, B = offset:
//   training cells of bin j: the bins j - g - t .. j - g - 1 (left) and j + g + 1 .. j + g + t (right), cut at the row's ends;
//   (S, n) = their sum and count: both sides (mode 0), the side of the larger mean (1) or of the smaller (2), an empty side giving way;
//   detection: 256 n v[j] > A S + 256 B n (n = 0: v[j] > B);   candidate: a detection with key[j] == win[j] and min_range <= j < hi;
//   keypoints: the min(k, #candidates) candidates of highest key, in ascending j -- key, win, hi and the select as k-strongest.
//
// Launch chain of a batch (no host synchronisation, two launches per sub-batch of <= 128 images):
//   cfar_rows  one WAVEFRONT per (azimuth, image): the row body of k-strongest (kstrongest_dev.h: the row once into LDS, the
//              screen, the separation window, the histogram select) with the detection below in place of the fixed floor.
//              The screen takes what every detection needs -- the range limits, v > B (the threshold is never below B) and,
//              for separation >= 1, the two adjacent bins -- and only its survivors (a few per cent of a radar row), one per
//              lane, sum their <= 2 x 64 training bytes out of the row in LDS: aligned dwords, the bytes outside the cells
//              masked off the first and the last, one v_sad_u8 per dword.  No prefix sums, nothing per bin.
//   kp_pack    (keypoints_host.h) row-major packing of the rows' keypoints + polar -> Cartesian
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <mutex>
#include <new>

#include "cfar.h"
#include "keypoints_host.h"
#include "kstrongest_dev.h"

namespace {

using rsx::ks::MAX_COLS;
using rsx::ks::MAX_K;
using rsx::ks::MAX_ROWS;
using rsx::ks::MAX_SEP;
constexpr int MAX_TRAIN = 64;
constexpr int MAX_GUARD = 16;

// sum of the bytes raw[p0 .. p1) of LDS (raw: 4-byte aligned, 0 <= p0; nothing when p0 >= p1): whole dwords, only the bytes asked for count
__device__ __forceinline__ unsigned lds_byte_sum(const unsigned char *raw, int p0, int p1) {
  if (p0 >= p1) return 0u;
  const unsigned *rd = reinterpret_cast<const unsigned *>(raw);
  const int d0 = p0 >> 2, d1 = (p1 - 1) >> 2;
  const unsigned first = 0xFFFFFFFFu << (8 * (p0 & 3)), last = 0xFFFFFFFFu >> (8 * (3 - ((p1 - 1) & 3)));
  if (d0 == d1) return __builtin_amdgcn_sad_u8(rd[d0] & first & last, 0u, 0u);
  unsigned s = __builtin_amdgcn_sad_u8(rd[d0] & first, 0u, 0u);
  for (int d = d0 + 1; d < d1; d++) s = __builtin_amdgcn_sad_u8(rd[d], 0u, s);
  return __builtin_amdgcn_sad_u8(rd[d1] & last, 0u, s);
}

// the detection of rsx::ks::row: T = (A / 256) (S / n) + B over the training cells of the bin
struct CfarDetect {
  static constexpr bool kLocal = true;
  int train, guard, scale_q8, offset, mode;
  __device__ __forceinline__ int floor() const { return offset + 1; }  // A S >= 0: no detection at or below B
  // bin i of the row at raw[m + i]
  __device__ __forceinline__ bool detect(const unsigned char *raw, int m, int j, int cols) const {
    // the cells, cut at the row's ends: [l0, l1) on the left, [r0, r1) on the right
    const int l0 = max(j - guard - train, 0), l1 = max(j - guard, 0);
    const int r0 = min(j + guard + 1, cols), r1 = min(j + guard + train + 1, cols);
    const unsigned SL = lds_byte_sum(raw, m + l0, m + l1), nL = (unsigned)(l1 - l0);
    const unsigned SR = lds_byte_sum(raw, m + r0, m + r1), nR = (unsigned)(r1 - r0);
    unsigned S = SL + SR, n = nL + nR;
    if (mode != 0 && nL && nR) {                // (an empty side gives way: S, n are the other side's already)
      const bool left_ge = SL * nR >= SR * nL;  // mean_L >= mean_R; <= 64 x 255 x 64
      const bool left = mode == 1 ? left_ge : !left_ge;
      S = left ? SL : SR;
      n = left ? nL : nR;
    }
    const unsigned v = raw[m + j];
    if (n == 0) return v > (unsigned)offset;
    // both sides below 2^31 within the parameter limits: the left <= 256 x 128 x 255, the right <= 65535 x 32640 + 256 x 255 x 128
    // = 2 147 418 240 (S <= 128 x 255 = 32640)
    return 256u * n * v > (unsigned)scale_q8 * S + 256u * (unsigned)offset * n;
  }
};

// one wavefront per (azimuth blockIdx.x, image blockIdx.y); dynamic LDS: rsx::ks::lds_bytes(cols, sep)
__global__ __launch_bounds__(64) void cfar_rows(const uint8_t *__restrict__ imgs, int64_t img_stride, int rows, int cols, int stride, int off, int k,
                                                CfarDetect det, int lo_bin, int hi_bin, int sep, uint16_t *__restrict__ row_kp,
                                                unsigned *__restrict__ row_n) {
  rsx::ks::row(imgs, img_stride, rows, cols, stride, off, k, det, lo_bin, hi_bin, sep, row_kp, row_n);
}

}  // namespace

struct rsx_cfar : rsx::KeypointHandle {
  rsx::DevBuf row_kp, row_n;
};

using rsx::fail;

int rsx::cfar_check_params(const rsx_cfar_params &p) {
  if (p.k < 1 || p.k > MAX_K) return fail(RSX_ERR_BAD_ARG, "k %d outside [1, %d]", p.k, MAX_K);
  if (p.train < 1 || p.train > MAX_TRAIN) return fail(RSX_ERR_BAD_ARG, "train %d outside [1, %d]", p.train, MAX_TRAIN);
  if (p.guard < 0 || p.guard > MAX_GUARD) return fail(RSX_ERR_BAD_ARG, "guard %d outside [0, %d]", p.guard, MAX_GUARD);
  if (p.scale_q8 < 0 || p.scale_q8 > 65535) return fail(RSX_ERR_BAD_ARG, "scale_q8 %d outside [0, 65535]", p.scale_q8);
  if (p.offset < 0 || p.offset > 255) return fail(RSX_ERR_BAD_ARG, "offset %d outside [0, 255]", p.offset);
  if (p.mode < 0 || p.mode > 2) return fail(RSX_ERR_BAD_ARG, "mode %d outside [0, 2]", p.mode);
  if (p.min_range < 0) return fail(RSX_ERR_BAD_ARG, "min_range %d < 0", p.min_range);
  if (p.max_range < 0) return fail(RSX_ERR_BAD_ARG, "max_range %d < 0", p.max_range);
  if (p.min_separation < 0 || p.min_separation > MAX_SEP) return fail(RSX_ERR_BAD_ARG, "min_separation %d outside [0, %d]", p.min_separation, MAX_SEP);
  if (p.reserved != 0) return fail(RSX_ERR_BAD_ARG, "reserved %d != 0", p.reserved);
  return RSX_OK;
}

namespace {

// the resolve step of the scaffold (keypoints_host.h): the defaults, *params over them, the check
int get_params(const rsx_cfar_params *params, rsx_cfar_params *p) {
  rsx_cfar_default_params(p);
  if (params) *p = *params;
  return rsx::cfar_check_params(*p);
}

// d_imgs: nb device images img_stride bytes apart -> d_targets [nb][max_targets][2], d_xy (optional, needs d_az), d_counts
// (optional).  Two launches per sub-batch (rsx::rows_then_pack; row_cap = k), nothing read on the host.
int extract_device(rsx_cfar *h, const uint8_t *d_imgs, int64_t img_stride, int nb, int32_t stride, int32_t off, const rsx_cfar_params &p,
                   const float *d_az, int64_t az_stride, float resolution, int32_t max_targets, int *d_targets, float *d_xy, int *d_counts,
                   hipStream_t s) {
  const int rows = h->rows, cols = h->cols;
  const int lo = p.min_range < cols ? p.min_range : cols, hi = p.max_range == 0 || p.max_range > cols ? cols : p.max_range;
  const size_t lds = rsx::ks::lds_bytes(cols, p.min_separation);
  const CfarDetect det{p.train, p.guard, p.scale_q8, p.offset, p.mode};
  return rsx::rows_then_pack(h, p.k, nb, d_az, az_stride, resolution, max_targets, d_targets, d_xy, d_counts, s, [&](int b0, int n) {
    hipLaunchKernelGGL(cfar_rows, dim3((unsigned)rows, (unsigned)n), dim3(64), lds, s, d_imgs + (int64_t)b0 * img_stride, img_stride, rows, cols, stride,
                       off, p.k, det, lo, hi, p.min_separation, h->row_kp.as<uint16_t>(), h->row_n.as<unsigned>());
  });
}

}  // namespace

extern "C" {

int rsx_cfar_default_params(rsx_cfar_params *p) try {
  if (!p) return fail(RSX_ERR_BAD_ARG, "null params");
  p->k = 12;  // as k-strongest
  p->train = 20;
  p->guard = 2;
  p->scale_q8 = 768;  // a = 3, b = 20: include/rsx.h, the defaults study
  p->offset = 20;
  p->mode = RSX_CFAR_CA;
  p->min_range = 58;  // as the other extractors
  p->max_range = 0;
  p->min_separation = 5;
  p->reserved = 0;
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_cfar_create(int device, int32_t rows, int32_t cols, rsx_cfar **out) try {
  return rsx::keypoints_create(rows >= 1 && rows <= MAX_ROWS && cols >= 1 && cols <= MAX_COLS, device, rows, cols, out);
} RSX_CATCH_ALL

int rsx_cfar_destroy(rsx_cfar *h) try {
  return rsx::keypoints_destroy(h);
} RSX_CATCH_ALL

int rsx_cfar_extract_batch_device(rsx_cfar *h, const uint8_t *d_imgs, int32_t n_images, int64_t image_stride_bytes, int32_t row_stride,
                                  int32_t col_offset, const rsx_cfar_params *params, const float *d_azimuths, int32_t azimuths_per_image,
                                  float resolution, int32_t *d_targets, float *d_xy, int32_t max_targets, int32_t *d_counts, void *stream) try {
  return rsx::keypoints_extract_batch_device(h, get_params, extract_device, d_imgs, n_images, image_stride_bytes, row_stride, col_offset, params,
                                             d_azimuths, azimuths_per_image, resolution, d_targets, d_xy, max_targets, d_counts, stream);
} RSX_CATCH_ALL

int rsx_cfar_extract_batch(rsx_cfar *h, const uint8_t *imgs, int32_t n_images, int64_t image_stride_bytes, int32_t row_stride, int32_t col_offset,
                           const rsx_cfar_params *params, const float *azimuths, int32_t azimuths_per_image, float resolution,
                           int32_t *out_targets, float *out_xy, int32_t max_targets, int32_t *out_counts) try {
  return rsx::keypoints_extract_batch(h, get_params, extract_device, imgs, n_images, image_stride_bytes, row_stride, col_offset, params, azimuths,
                                      azimuths_per_image, resolution, out_targets, out_xy, max_targets, out_counts);
} RSX_CATCH_ALL

int rsx_cfar_extract(rsx_cfar *h, const uint8_t *img, int32_t row_stride, int32_t col_offset, const rsx_cfar_params *params,
                     const float *azimuths, float resolution, int32_t *out_targets, float *out_xy, int32_t max_targets, int32_t *out_count) try {
  return rsx::keypoints_extract(h, get_params, extract_device, img, row_stride, col_offset, params, azimuths, resolution, out_targets, out_xy,
                                max_targets, out_count);
} RSX_CATCH_ALL

}  // extern "C"
