// keypoints_host.h -- what the keypoint extractors (cen2018.hip, cen2019.hip, kstrongest.hip, cfar.hip) and the odometry share: the check of a polar image
// layout, the image upload, the kernel that packs the per-row keypoints, the staging of the host-buffer entries, and the host
// scaffold of an extractor (its handle and the bodies of its create / destroy / extract entries, written once: "the scaffold" below).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <mutex>
#include <new>
#include <type_traits>

#include "rsx_common.h"
#include "rsx_wave_dev.h"

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
  before = rsx::wave::butterfly(before, rsx::wave::Add{});
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

// device staging of the host-buffer entries (rsx_<extractor>_extract_batch): images and azimuth grids up, keypoints down
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

// ---- the scaffold: the host side that the extractors have in common ----
// An extractor's own file keeps its kernels, its workspaces and three things the templates below are handed:
//   its parameter type P (deduced from the entry's `params`);
//   resolve: int(const P *params, P *p) -- the defaults, then *params over them when given, then the check of the result
//            (RSX_ERR_BAD_ARG with the message set; cen2019 has nothing to check);
//   extract: int(H *h, const uint8_t *d_imgs, int64_t img_stride, int nb, int32_t stride, int32_t off, const P &p, const float *d_az,
//            int64_t az_stride, float resolution, int32_t max_targets, int *d_targets, float *d_xy, int *d_counts, hipStream_t s)
//            -- the launch chain over nb device images, nothing read on the host.
// Every extern "C" entry stays a function-try-block in the extractor's file and forwards here in one statement.  The argument
// contract (include/rsx.h) and the one-handle, many-streams contract -- the lock, the device, StreamOrder::enter before anything
// is enqueued or reserved -- are written here and nowhere else.

// what every extractor handle holds; rsx_cen2018, rsx_cen2019, rsx_kstrongest and rsx_cfar add their workspaces
struct KeypointHandle {
  int device = 0, rows = 0, cols = 0;
  std::mutex mu;
  Stream stream;
  KeypointStaging stage;
  StreamOrder order;
};

// rsx_<extractor>_create; shape_ok: the extractor's verdict on rows x cols
template <typename H>
int keypoints_create(bool shape_ok, int device, int32_t rows, int32_t cols, H **out) {
  if (!out) return fail(RSX_ERR_BAD_ARG, "null out");
  *out = nullptr;
  if (!shape_ok) return fail(RSX_ERR_BAD_ARG, "image shape %d x %d unsupported", rows, cols);
  RSX_TRY(check_device(device));
  std::unique_ptr<H> h(new (std::nothrow) H());
  if (!h) return fail(RSX_ERR_OOM, "host alloc");
  h->device = device;
  h->rows = rows;
  h->cols = cols;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = h->stream.create();
  if (e != hipSuccess) return fail(RSX_ERR_HIP, "create: %s", hipGetErrorString(e));
  *out = h.release();
  return RSX_OK;
}

// rsx_<extractor>_destroy
template <typename H>
int keypoints_destroy(H *h) {
  if (!h) return RSX_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  delete h;
  return RSX_OK;
}

// rsx_<extractor>_extract_batch_device: images and results on the device, on the caller's stream (NULL: the handle's)
template <typename H, typename P, typename Resolve, typename Extract>
int keypoints_extract_batch_device(H *h, Resolve resolve, Extract extract, const uint8_t *d_imgs, int32_t n_images, int64_t image_stride_bytes,
                                   int32_t row_stride, int32_t col_offset, const P *params, const float *d_azimuths, int32_t azimuths_per_image,
                                   float resolution, int32_t *d_targets, float *d_xy, int32_t max_targets, int32_t *d_counts, void *stream) {
  if (!h || !d_imgs || !d_targets || n_images < 0 || max_targets < 1) return fail(RSX_ERR_BAD_ARG, "bad arg");
  RSX_TRY(check_polar_layout(h->rows, h->cols, n_images, image_stride_bytes, row_stride, col_offset));
  if (d_xy && !d_azimuths) return fail(RSX_ERR_BAD_ARG, "d_xy needs d_azimuths");
  P p;
  RSX_TRY(resolve(params, &p));  // (before the empty batch: bad parameters are refused whatever n_images)
  if (n_images == 0) return RSX_OK;
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
  RSX_TRY(h->order.enter(s));
  return extract(h, d_imgs, image_stride_bytes, n_images, row_stride, col_offset, p, d_azimuths, azimuths_per_image ? h->rows : 0, resolution,
                 max_targets, d_targets, d_xy, d_counts, s);
}

// an extractor may give the host entry a path of its own for a single image: a member
//   int single_scan(const uint8_t *img, int32_t row_stride, int32_t col_offset, const P &p, const float *azimuths, float resolution,
//                   int32_t *out_targets, float *out_xy, int32_t max_targets, int32_t *out_count, hipStream_t s)
// of its handle, called under the handle's lock with s entered, in place of the staging below (cen2019 has one)
template <typename H, typename = void>
struct has_single_scan : std::false_type {};
template <typename H>
struct has_single_scan<H, std::void_t<decltype(&H::single_scan)>> : std::true_type {};

// rsx_<extractor>_extract_batch: images and results in host memory, on the handle's stream; max_targets = 0 counts only
template <typename H, typename P, typename Resolve, typename Extract>
int keypoints_extract_batch(H *h, Resolve resolve, Extract extract, const uint8_t *imgs, int32_t n_images, int64_t image_stride_bytes,
                            int32_t row_stride, int32_t col_offset, const P *params, const float *azimuths, int32_t azimuths_per_image,
                            float resolution, int32_t *out_targets, float *out_xy, int32_t max_targets, int32_t *out_counts) {
  if (!h || !imgs || !out_targets || !out_counts || n_images < 0 || max_targets < 0) return fail(RSX_ERR_BAD_ARG, "bad arg");
  RSX_TRY(check_polar_layout(h->rows, h->cols, n_images, image_stride_bytes, row_stride, col_offset));
  if (out_xy && !azimuths) return fail(RSX_ERR_BAD_ARG, "out_xy needs azimuths");
  P p;
  RSX_TRY(resolve(params, &p));
  if (n_images == 0) return RSX_OK;
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  RSX_TRY(h->order.enter(s));
  if constexpr (has_single_scan<H>::value) {
    if (n_images == 1) return h->single_scan(imgs, row_stride, col_offset, p, azimuths, resolution, out_targets, out_xy, max_targets, out_counts, s);
  }
  const int mt = max_targets > 0 ? max_targets : 1;  // (the launch chain wants a slot; KeypointStaging copies none of it back)
  auto staged = [&](const uint8_t *d_imgs, int n, const float *d_az, int *d_targets, float *d_xy, int *d_counts, hipStream_t st) {
    return extract(h, d_imgs, (int64_t)h->rows * row_stride, n, row_stride, col_offset, p, d_az, azimuths_per_image ? h->rows : 0, resolution, mt,
                   d_targets, d_xy, d_counts, st);
  };
  return h->stage.extract_batch(h->rows, imgs, n_images, image_stride_bytes, row_stride, azimuths, azimuths_per_image, out_targets, out_xy, max_targets,
                                out_counts, s, staged);
}

// rsx_<extractor>_extract: one image through the host entry
template <typename H, typename P, typename Resolve, typename Extract>
int keypoints_extract(H *h, Resolve resolve, Extract extract, const uint8_t *img, int32_t row_stride, int32_t col_offset, const P *params,
                      const float *azimuths, float resolution, int32_t *out_targets, float *out_xy, int32_t max_targets, int32_t *out_count) {
  if (!h || !img || !out_targets || !out_count || max_targets < 0) return fail(RSX_ERR_BAD_ARG, "bad arg");
  return keypoints_extract_batch(h, resolve, extract, img, 1, (int64_t)h->rows * row_stride, row_stride, col_offset, params, azimuths, 0, resolution,
                                 out_targets, out_xy, max_targets, out_count);
}

// the launch chain of an extractor whose row kernel leaves up to row_cap uint16 range bins per row in h->row_kp and their number in
// h->row_n (cen2018, k-strongest, CFAR): per sub-batch launch_rows(b0, n) -- the row kernel over images b0 .. b0 + n -- then kp_pack
template <typename H, typename LaunchRows>
int rows_then_pack(H *h, int row_cap, int nb, const float *d_az, int64_t az_stride, float resolution, int32_t max_targets, int *d_targets,
                   float *d_xy, int *d_counts, hipStream_t s, LaunchRows &&launch_rows) {
  const int rows = h->rows;
  for (int b0 = 0; b0 < nb; b0 += MAX_SUB_BATCH) {
    const int n = nb - b0 < MAX_SUB_BATCH ? nb - b0 : MAX_SUB_BATCH;
    RSX_TRY(h->row_kp.reserve((size_t)n * rows * row_cap * 2, s, false));
    RSX_TRY(h->row_n.reserve((size_t)n * rows * 4, s, false));
    launch_rows(b0, n);
    hipLaunchKernelGGL(kp_pack<uint16_t>, dim3((unsigned)((rows + PACK_WAVES - 1) / PACK_WAVES), (unsigned)n), dim3(64 * PACK_WAVES), 0, s, rows, row_cap,
                       h->row_kp.template as<uint16_t>(), h->row_n.template as<unsigned>(), d_az ? d_az + (int64_t)b0 * az_stride : nullptr, az_stride,
                       resolution, max_targets, d_targets + (int64_t)b0 * max_targets * 2, d_xy ? d_xy + (int64_t)b0 * max_targets * 2 : nullptr,
                       d_counts ? d_counts + b0 : nullptr, nullptr, 0);
    RSX_HIP(hipGetLastError());
  }
  return RSX_OK;
}

}  // namespace rsx
