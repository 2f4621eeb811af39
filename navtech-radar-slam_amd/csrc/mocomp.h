// mocomp.h -- what csrc/odometry.hip shares with csrc/mocomp.hip beside the public entries of include/rsx.h.
#pragma once
#include "rsx_common.h"

namespace rsx {
namespace mocomp {

// the parameter rules of the rsx_mocomp entries (RSX_ERR_BAD_ARG + message, or RSX_OK)
int check_params(const rsx_mocomp_params &p);

// The launches behind the device entries; they touch no handle.  A pair's / scan's pose is read from a record `pose_stride`
// bytes long that starts with the doubles x, y, yaw (an array of double[3], or of rsx_orora_result); status_off >= 0: the
// record carries an int32 status at that byte offset, and a pair / scan whose status != 0 is copied through as measured.
int launch_matches(const float *d_src, const float *d_dst, const int32_t *d_a_cur, const int32_t *d_a_prev, const int64_t *d_offsets,
                   int32_t n_pairs, const void *d_pose, int64_t pose_stride, int32_t status_off, const rsx_mocomp_params &p, float *d_out_src,
                   float *d_out_dst, int32_t *d_out_status, hipStream_t s);
// keypoints in the slot layout of the odometry: scan i owns min(d_counts[i], stride) points at d_xy + i * stride * 2, their
// azimuth rows at d_targets[(i * stride + k) * 2]; it is compensated with the velocity of the pose record i - first (copied
// through as measured when i < first) into d_out_xy, laid out like d_xy
int launch_slots(const float *d_xy, const int32_t *d_targets, const int32_t *d_counts, int32_t stride, int32_t n_scans, int32_t first,
                 const void *d_pose, int64_t pose_stride, int32_t status_off, const rsx_mocomp_params &p, float *d_out_xy, hipStream_t s);

}  // namespace mocomp
}  // namespace rsx
