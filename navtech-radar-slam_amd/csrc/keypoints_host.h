// keypoints_host.h -- what the keypoint extractors (cen2018.hip, cen2019.hip, kstrongest.hip) and the odometry share: the check of a polar image
// layout, the image upload, the kernel that packs the per-row keypoints, and the host path of rsx_cen201x_extract_batch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rsx_common.h"

namespace rsx {

constexpr int MAX_SUB_BATCH = 128;  // images per internal launch chain of an extractor (bounds its workspaces and the staging below)

// n_images polar images of rows x cols bins, image_stride_bytes apart, col_offset bytes in front of every row of row_stride bytes
inline int check_polar_layout(int rows, int cols, int32_t n_images, int64_t image_stride_bytes, int32_t row_stride, int32_t col_offset) {
  if (col_offset < 0 || row_stride < col_offset + cols)
    return fail(RSX_ERR_BAD_ARG, "row_stride %d too small for offset %d + %d columns", row_stride, col_offset, cols);
  if (n_images > 1 && image_stride_bytes < (int64_t)rows * row_stride) return fail(RSX_ERR_BAD_ARG, "image_stride_bytes smaller than an image");
  return RSX_OK;
}

// n host images of image_bytes, image_stride_bytes apart -> dst, contiguous
inline int upload_images(void *dst, const uint8_t *src, int n, size_t image_bytes, int64_t image_stride_bytes, hipStream_t s) {
  if (n == 1 || image_stride_bytes == (int64_t)image_bytes) {
    RSX_HIP(hipMemcpyAsync(dst, src, image_bytes * n, hipMemcpyHostToDevice, s));
  } else {
    RSX_HIP(hipMemcpy2DAsync(dst, image_bytes, src, (size_t)image_stride_bytes, image_bytes, (size_t)n, hipMemcpyHostToDevice, s));
  }
  return RSX_OK;
}

// one wavefront per (azimuth, image): row-major packing of the rows' keypoints (row_kp: row_cap range bins per row, row_n of
// them set), polar -> Cartesian.  n_targets (optional): the image's count also goes to n_targets + img * n_targets_stride bytes
constexpr int PACK_WAVES = 4;  // azimuths per workgroup
template <typename Rec>
__global__ __launch_bounds__(64 * PACK_WAVES) void kp_pack(int rows, int row_cap, const Rec *__restrict__ row_kp, const unsigned *__restrict__ row_n,
                                                           const float *__restrict__ az, int64_t az_stride, float resolution, int max_targets,
                                                           int *__restrict__ targets, float *__restrict__ xy, int *__restrict__ counts,
                                                           unsigned *__restrict__ n_targets, int64_t n_targets_stride) {
  const int a = (int)blockIdx.x * PACK_WAVES + (int)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), img = blockIdx.y, lane = threadIdx.x & 63;
  if (a >= rows) return;  // (wave-uniform; no barrier in this kernel)
  const unsigned *rn = row_n + (int64_t)img * rows;
  unsigned before = 0;
  for (int r = lane; r < a; r += 64) before += rn[r];
  for (int o = 32; o >= 1; o >>= 1) before += __shfl_xor(before, o);
  const unsigned n = rn[a];
  int *tg = targets + (int64_t)img * max_targets * 2;
  float *pxy = xy ? xy + (int64_t)img * max_targets * 2 : nullptr;
  const float *azi = az ? az + (int64_t)img * az_stride : nullptr;
  const Rec *kp = row_kp + ((int64_t)img * rows + a) * row_cap;
  for (unsigned i = lane; i < n; i += 64) {
    const unsigned d = before + i;
    if (d >= (unsigned)max_targets) break;
    const int r = kp[i];
    tg[2 * d] = a;
    tg[2 * d + 1] = r;
    if (pxy && azi) {
      const float range = __fmul_rn(__fadd_rn((float)r, 0.5f), resolution);
      pxy[2 * d] = __fmul_rn(range, cosf(azi[a]));
      pxy[2 * d + 1] = __fmul_rn(range, sinf(azi[a]));
    }
  }
  if (a == rows - 1 && lane == 0) {
    if (n_targets) *reinterpret_cast<unsigned *>(reinterpret_cast<char *>(n_targets) + (int64_t)img * n_targets_stride) = before + n;
    if (counts) counts[img] = (int)(before + n);
  }
}

// device staging of the host-buffer entries (rsx_cen201x_extract_batch): images and azimuth grids up, keypoints down
struct KeypointStaging {
  DevBuf img, targets, xy, az, counts;

  // n_images host images through `extract`, int(const uint8_t *d_imgs, int n, const float *d_az, int *d_targets, float *d_xy,
  // int *d_counts, hipStream_t): n <= MAX_SUB_BATCH contiguous device images, max(max_targets, 1) keypoint slots per image.
  // Sub-batches bound the staging memory; each one is a single upload, one launch chain, one download
  template <typename Extract>
  int extract_batch(int rows, const uint8_t *imgs, int32_t n_images, int64_t image_stride_bytes, int32_t row_stride, const float *azimuths,
                    int32_t azimuths_per_image, int32_t *out_targets, float *out_xy, int32_t max_targets, int32_t *out_counts, hipStream_t s,
                    Extract &&extract) {
    const size_t ibytes = (size_t)rows * row_stride;
    const int mt = max_targets > 0 ? max_targets : 1;
    for (int b0 = 0; b0 < n_images; b0 += MAX_SUB_BATCH) {
      const int n = n_images - b0 < MAX_SUB_BATCH ? n_images - b0 : MAX_SUB_BATCH;
      RSX_TRY(img.reserve(ibytes * n, s, false));
      RSX_TRY(targets.reserve((size_t)n * mt * 8, s, false));
      RSX_TRY(xy.reserve((size_t)n * mt * 8, s, false));
      RSX_TRY(counts.reserve((size_t)n * 4, s, false));
      RSX_TRY(upload_images(img.p, imgs + (int64_t)b0 * image_stride_bytes, n, ibytes, image_stride_bytes, s));
      const float *d_az = nullptr;
      if (azimuths) {
        const size_t na = (size_t)rows * (azimuths_per_image ? n : 1);
        RSX_TRY(az.reserve(na * 4, s, false));
        RSX_HIP(hipMemcpyAsync(az.p, azimuths + (azimuths_per_image ? (size_t)b0 * rows : 0), na * 4, hipMemcpyHostToDevice, s));
        d_az = az.as<float>();
      }
      RSX_TRY(extract(img.as<uint8_t>(), n, d_az, targets.as<int>(), d_az ? xy.as<float>() : nullptr, counts.as<int>(), s));
      RSX_HIP(hipMemcpyAsync(out_counts + b0, counts.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
      RSX_HIP(hipStreamSynchronize(s));
      for (int i = 0; i < n; i++) {
        const unsigned cnt = (unsigned)out_counts[b0 + i];
        const unsigned w = cnt < (unsigned)max_targets ? cnt : (unsigned)max_targets;
        if (!w) continue;
        RSX_HIP(hipMemcpyAsync(out_targets + (int64_t)(b0 + i) * max_targets * 2, targets.as<int>() + (int64_t)i * mt * 2, (size_t)w * 8,
                               hipMemcpyDeviceToHost, s));
        if (out_xy)
          RSX_HIP(hipMemcpyAsync(out_xy + (int64_t)(b0 + i) * max_targets * 2, xy.as<float>() + (int64_t)i * mt * 2, (size_t)w * 8,
                                 hipMemcpyDeviceToHost, s));
      }
      RSX_HIP(hipStreamSynchronize(s));
    }
    return RSX_OK;
  }
};

}  // namespace rsx
