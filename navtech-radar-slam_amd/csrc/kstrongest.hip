// kstrongest.hip -- k-strongest radar keypoint extraction (the detector of CFEAR radar odometry, with a separation rule) on
// gfx950, batched.
//
// Per azimuth row the k strongest returns above a fixed power floor; no noise model, a hard budget of rows x k keypoints
// per scan.  The rule is integer arithmetic only (include/rsx.h, restated in tests/kstrongest_np.py):
//   key[j] = (v[j] << 16) | (0xFFFF - j);   win[j] = max key over the bins within min_separation of j (cut at the row's ends);
//   candidate: key[j] == win[j], v[j] >= z_min, min_range <= j < hi;   keypoints: the min(k, #candidates) candidates of
//   highest key, in ascending j.
// On powers alone: key[j] == win[j] iff v[j] > v[i] for every bin i < j of the window and v[j] >= v[i] for every bin i > j.
//
// Launch chain of a batch (no host synchronisation, two launches per sub-batch of <= 128 images):
//   ks_rows    one WAVEFRONT per (azimuth, image); its body is kstrongest_dev.h (shared with cfar.hip), the detection the fixed floor:
//              1. the row's bytes once into LDS, in the aligned 16-byte pieces that hold them (a piece that sticks out of the
//                 image: only its bytes inside)
//              2. screen, four consecutive bins per lane from three LDS dwords: floor, range limits and the two ADJACENT bins
//                 (separation >= 1) -- the survivors (no two adjacent; a few per cent of a radar row) go, in ascending
//                 bin order (ballots), into a list in LDS
//              3. separation >= 2: one survivor per lane against the rest of its window, the list compacted in place
//              4. more candidates than k: a 256-bin histogram of their powers (LDS atomics), a wave suffix scan over it
//                 from the strongest power down -> the threshold power and how many candidates AT the threshold are kept;
//                 everything above the threshold and the nearest of the ties survive, ranked by ballots so that they land in
//                 ascending bin order in row_kp (row_cap = k) + per-row count
//   kp_pack    (keypoints_host.h, shared with cen2018 and cen2019) row-major packing of the rows' keypoints + polar -> Cartesian
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <mutex>
#include <new>

#include "keypoints_host.h"
#include "kstrongest.h"
#include "kstrongest_dev.h"

namespace {

using rsx::ks::MAX_COLS;
using rsx::ks::MAX_K;
using rsx::ks::MAX_ROWS;
using rsx::ks::MAX_SEP;

// one wavefront per (azimuth blockIdx.x, image blockIdx.y): the shared row body (kstrongest_dev.h) with the fixed floor as its detection
__global__ __launch_bounds__(64) void ks_rows(const uint8_t *__restrict__ imgs, int64_t img_stride, int rows, int cols, int stride, int off, int k,
                                              int z_min, int lo_bin, int hi_bin, int sep, uint16_t *__restrict__ row_kp,
                                              unsigned *__restrict__ row_n) {
  rsx::ks::row(imgs, img_stride, rows, cols, stride, off, k, rsx::ks::Floor{z_min}, lo_bin, hi_bin, sep, row_kp, row_n);
}

}  // namespace

struct rsx_kstrongest : rsx::KeypointHandle {
  rsx::DevBuf row_kp, row_n;
};

using rsx::fail;

int rsx::kstrongest_check_params(const rsx_kstrongest_params &p) {
  if (p.k < 1 || p.k > MAX_K) return fail(RSX_ERR_BAD_ARG, "k %d outside [1, %d]", p.k, MAX_K);
  if (p.z_min < 0 || p.z_min > 255) return fail(RSX_ERR_BAD_ARG, "z_min %d outside [0, 255]", p.z_min);
  if (p.min_range < 0) return fail(RSX_ERR_BAD_ARG, "min_range %d < 0", p.min_range);
  if (p.max_range < 0) return fail(RSX_ERR_BAD_ARG, "max_range %d < 0", p.max_range);
  if (p.min_separation < 0 || p.min_separation > MAX_SEP) return fail(RSX_ERR_BAD_ARG, "min_separation %d outside [0, %d]", p.min_separation, MAX_SEP);
  return RSX_OK;
}

namespace {

// the resolve step of the scaffold (keypoints_host.h): the defaults, *params over them, the check
int get_params(const rsx_kstrongest_params *params, rsx_kstrongest_params *p) {
  rsx_kstrongest_default_params(p);
  if (params) *p = *params;
  return rsx::kstrongest_check_params(*p);
}

// d_imgs: nb device images img_stride bytes apart -> d_targets [nb][max_targets][2], d_xy (optional, needs d_az), d_counts
// (optional).  Two launches per sub-batch (rsx::rows_then_pack; row_cap = k), nothing read on the host.
int extract_device(rsx_kstrongest *h, const uint8_t *d_imgs, int64_t img_stride, int nb, int32_t stride, int32_t off, const rsx_kstrongest_params &p,
                   const float *d_az, int64_t az_stride, float resolution, int32_t max_targets, int *d_targets, float *d_xy, int *d_counts,
                   hipStream_t s) {
  const int rows = h->rows, cols = h->cols;
  const int lo = p.min_range < cols ? p.min_range : cols, hi = p.max_range == 0 || p.max_range > cols ? cols : p.max_range;
  const size_t lds = rsx::ks::lds_bytes(cols, p.min_separation);
  return rsx::rows_then_pack(h, p.k, nb, d_az, az_stride, resolution, max_targets, d_targets, d_xy, d_counts, s, [&](int b0, int n) {
    hipLaunchKernelGGL(ks_rows, dim3((unsigned)rows, (unsigned)n), dim3(64), lds, s, d_imgs + (int64_t)b0 * img_stride, img_stride, rows, cols, stride, off,
                       p.k, p.z_min, lo, hi, p.min_separation, h->row_kp.as<uint16_t>(), h->row_n.as<unsigned>());
  });
}

}  // namespace

extern "C" {

int rsx_kstrongest_default_params(rsx_kstrongest_params *p) try {
  if (!p) return fail(RSX_ERR_BAD_ARG, "null params");
  p->k = 12;  // CFEAR radar odometry: k = 12, z_min = 60
  p->z_min = 60;
  p->min_range = 58;  // as the other extractors
  p->max_range = 0;
  p->min_separation = 5;  // include/rsx.h: why not CFEAR's plain rule
  p->reserved = 0;
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_kstrongest_create(int device, int32_t rows, int32_t cols, rsx_kstrongest **out) try {
  return rsx::keypoints_create(rows >= 1 && rows <= MAX_ROWS && cols >= 1 && cols <= MAX_COLS, device, rows, cols, out);
} RSX_CATCH_ALL

int rsx_kstrongest_destroy(rsx_kstrongest *h) try {
  return rsx::keypoints_destroy(h);
} RSX_CATCH_ALL

int rsx_kstrongest_extract_batch_device(rsx_kstrongest *h, const uint8_t *d_imgs, int32_t n_images, int64_t image_stride_bytes, int32_t row_stride,
                                        int32_t col_offset, const rsx_kstrongest_params *params, const float *d_azimuths,
                                        int32_t azimuths_per_image, float resolution, int32_t *d_targets, float *d_xy, int32_t max_targets,
                                        int32_t *d_counts, void *stream) try {
  return rsx::keypoints_extract_batch_device(h, get_params, extract_device, d_imgs, n_images, image_stride_bytes, row_stride, col_offset, params,
                                             d_azimuths, azimuths_per_image, resolution, d_targets, d_xy, max_targets, d_counts, stream);
} RSX_CATCH_ALL

int rsx_kstrongest_extract_batch(rsx_kstrongest *h, const uint8_t *imgs, int32_t n_images, int64_t image_stride_bytes, int32_t row_stride,
                                 int32_t col_offset, const rsx_kstrongest_params *params, const float *azimuths, int32_t azimuths_per_image,
                                 float resolution, int32_t *out_targets, float *out_xy, int32_t max_targets, int32_t *out_counts) try {
  return rsx::keypoints_extract_batch(h, get_params, extract_device, imgs, n_images, image_stride_bytes, row_stride, col_offset, params, azimuths,
                                      azimuths_per_image, resolution, out_targets, out_xy, max_targets, out_counts);
} RSX_CATCH_ALL

int rsx_kstrongest_extract(rsx_kstrongest *h, const uint8_t *img, int32_t row_stride, int32_t col_offset, const rsx_kstrongest_params *params,
                           const float *azimuths, float resolution, int32_t *out_targets, float *out_xy, int32_t max_targets,
                           int32_t *out_count) try {
  return rsx::keypoints_extract(h, get_params, extract_device, img, row_stride, col_offset, params, azimuths, resolution, out_targets, out_xy,
                                max_targets, out_count);
} RSX_CATCH_ALL

}  // extern "C"
