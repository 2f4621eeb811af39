// phasecorr.h -- the handle of the rsx_phasecorr entries (csrc/phasecorr.hip), and the two launch stages csrc/odometry.hip shares with them.
#pragma once
#include <mutex>

#include "rsx_common.h"

struct rsx_phasecorr {
  int device = 0;
  std::mutex mu;
  rsx::Stream stream;
  rsx::StreamOrder order;  // the workspace and the staging buffers are shared by every call
  rsx_phasecorr_params p{};
  int rows = 0, cols = 0;
  rsx::DevBuf tables;      // map | cos / sin | directions | Hann | high-pass cosines, made by rsx_phasecorr_create
  rsx::DevBuf work;        // the slots of the scans and the pairs of the call in flight (include/rsx.h states its size)
  int last_images = 0, last_pairs = -1;  // the layout of `work` as the last call left it (rsx_phasecorr_correlation)
  rsx::DevBuf imgs, pairs, res, cart;    // staging of the host-buffer entry
};

namespace rsx {
namespace phasecorr {

// the parameter rules of the rsx_phasecorr entries, judged against the scans' shape (RSX_ERR_BAD_ARG + message, or RSX_OK)
int check_params(const rsx_phasecorr_params &p, int rows, int cols);
// the tables of (p, rows, cols) into `tables` (a blocking upload) and the kernels' LDS limit raised: once per parameter set.  The
// launches below only read them, so one set serves any number of streams
int make_tables(const rsx_phasecorr_params &p, int rows, int cols, rsx::DevBuf &tables, hipStream_t s);
// the bytes include/rsx.h states: per scan F (8 N^2) and the angle spectrum A (4 N^2 - 32 N), per pair 40 N^2 + 2048 + 4 N
void workspace_bytes(int n, size_t *per_scan_F, size_t *per_scan_A, size_t *per_pair);

// where the scans lie: image i at d_imgs + i * image_stride, power samples at [col_offset, col_offset + cols) of a row
struct Images {
  const uint8_t *d_imgs;
  int64_t image_stride;
  int32_t row_stride, col_offset;
};

// The two stages behind the device entry; they take the tables and the shape only and touch no handle.
// launches 1 - 3: the spectra of scans 0 .. n_scans - 1 of `im` into slots 0 .. n_scans - 1 of d_F ([slot][N][N]) and d_A
// ([slot][N / 2 - 4][N]); d_cart (may be null): their psi = 0 images
int launch_spectra(const rsx_phasecorr_params &p, int rows, int cols, const void *d_tables, const Images &im, int32_t n_scans, float2 *d_F, float2 *d_A,
                   float *d_cart, hipStream_t s);
// launches 4 - 9: pair i = (src, dst) = d_pairs[2 i], d_pairs[2 i + 1] names SLOTS of d_F / d_A (n_slots of them; a pair outside
// gets RSX_PHASECORR_STATUS_INDEX and costs nothing); src's image is image src + image_offset of the n_images of `im` (dst needs
// none: only src is sampled again).  d_pair_work: n_pairs x the per-pair bytes + 64
int launch_pairs(const rsx_phasecorr_params &p, int rows, int cols, const void *d_tables, const Images &im, int32_t n_images, int32_t image_offset,
                 const float2 *d_F, const float2 *d_A, int32_t n_slots, const int32_t *d_pairs, int32_t n_pairs, void *d_pair_work,
                 rsx_phasecorr_result *d_results, hipStream_t s);

}  // namespace phasecorr
}  // namespace rsx
