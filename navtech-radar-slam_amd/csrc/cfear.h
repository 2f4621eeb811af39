// cfear.h -- what csrc/odometry.hip shares with csrc/cfear.hip beside the public entries of include/rsx.h.
#pragma once
#include "rsx_common.h"

namespace rsx {
namespace cfear {

// the parameter rules of the rsx_cfear entries (RSX_ERR_BAD_ARG + message, or RSX_OK)
int check_params(const rsx_cfear_params &p);

// The launches behind the device entries; they touch no handle.  Group i owns elements [d_begin[i], d_end[i]) of its array:
// a ragged batch passes (offsets, offsets + 1), the odometry the ranges of its slots.
// scan i's records to d_out + i * max_records, d_counts[i] every record found, d_status[i] (may be null) the status word
int launch_surface(const float *d_xy, const int64_t *d_begin, const int64_t *d_end, int32_t n_scans, const rsx_cfear_params &p,
                   rsx_cfear_surface_point *d_out, int32_t max_records, int32_t *d_counts, int32_t *d_status, hipStream_t s);
// d_init: [n_pairs][3] doubles or null (identity)
int launch_register(const rsx_cfear_surface_point *d_src, const int64_t *d_src_begin, const int64_t *d_src_end,
                    const rsx_cfear_surface_point *d_dst, const int64_t *d_dst_begin, const int64_t *d_dst_end, int32_t n_pairs,
                    const double *d_init, const rsx_cfear_params &p, rsx_cfear_result *d_out, hipStream_t s);

}  // namespace cfear
}  // namespace rsx
