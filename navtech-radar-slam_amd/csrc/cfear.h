// cfear.h -- what csrc/cfear.hip, csrc/cfear_track.hip and csrc/odometry.hip share beside the public entries of include/rsx.h.
#pragma once
#include <mutex>

#include "rsx_common.h"

// the handle of the rsx_cfear entries (csrc/cfear.hip; the registration entries of csrc/cfear_track.hip work on it too)
struct rsx_cfear {
  int device = 0;
  std::mutex mu;
  rsx::Stream stream;
  rsx::StreamOrder order;  // the staging buffers are shared by every host-buffer call
  rsx::DevBuf in0, in1, off0, off1, init, out, cnt, st, tau;  // staging of the host-buffer entries
  rsx::DevBuf job_off, poses, index;  // registration: the jobs' keyframe ranges and poses (staging), the cell-index workspace
};

namespace rsx {
namespace cfear {

// the parameter rules of the rsx_cfear entries (RSX_ERR_BAD_ARG + message, or RSX_OK)
int check_params(const rsx_cfear_params &p);
// dp = *params or the defaults, checked; with dt, *dt = *track or the defaults, checked as well
int resolve(const rsx_cfear_params *params, const rsx_cfear_track_params *track, rsx_cfear_params &dp, rsx_cfear_track_params *dt);

// The launches behind the device entries; they touch no handle.  Group i owns elements [d_begin[i], d_end[i]) of its array:
// a ragged batch passes (offsets, offsets + 1), the odometry the ranges of its slots.
// scan i's records to d_out + i * max_records, d_counts[i] every record found, d_status[i] (may be null) the status word
int launch_surface(const float *d_xy, const int64_t *d_begin, const int64_t *d_end, int32_t n_scans, const rsx_cfear_params &p,
                   rsx_cfear_surface_point *d_out, int32_t max_records, int32_t *d_counts, int32_t *d_status, hipStream_t s);
// the same with the records' times: point j of group i was measured on azimuth row d_rows[(d_begin[i] + j) * row_stride] of n_rows
// (1 .. 65536, checked); scan i's times to d_out_tau + i * max_records.  The records are launch_surface's bytes
int launch_surface_timed(const float *d_xy, const int32_t *d_rows, int32_t row_stride, int32_t n_rows, const int64_t *d_begin,
                         const int64_t *d_end, int32_t n_scans, const rsx_cfear_params &p, rsx_cfear_surface_point *d_out, float *d_out_tau,
                         int32_t max_records, int32_t *d_counts, int32_t *d_status, hipStream_t s);

// ---- csrc/cfear_track.hip: registration, and the tracker ----
int check_track_params(const rsx_cfear_track_params &p);
// bytes of cell-index workspace (d_index) a registration launch wants for n_jobs jobs
size_t keyframe_index_bytes(int32_t n_jobs);
// job i registers src group i jointly to the keyframes [d_kf_job_offsets[i], d_kf_job_offsets[i + 1]) -- null: keyframe i alone --
// where keyframe g owns records [d_kf_begin[g], d_kf_end[g]) of d_kf and pose d_kf_poses[3 g ..] (null: every keyframe at the
// identity); d_init: [n_jobs][3] doubles or null (identity)
int launch_register_keyframes(const rsx_cfear_surface_point *d_src, const int64_t *d_src_begin, const int64_t *d_src_end,
                              const rsx_cfear_surface_point *d_kf, const int64_t *d_kf_begin, const int64_t *d_kf_end,
                              const int64_t *d_kf_job_offsets, const double *d_kf_poses, int32_t n_jobs, const double *d_init,
                              const rsx_cfear_params &p, const rsx_cfear_track_params &tp, void *d_index, rsx_cfear_result *d_out, hipStream_t s);
// pair i registers src group i to dst group i: the launch above with one keyframe per job at the identity, through the cell index
int launch_register(const rsx_cfear_surface_point *d_src, const int64_t *d_src_begin, const int64_t *d_src_end,
                    const rsx_cfear_surface_point *d_dst, const int64_t *d_dst_begin, const int64_t *d_dst_end, int32_t n_pairs,
                    const double *d_init, const rsx_cfear_params &p, void *d_index, rsx_cfear_result *d_out, hipStream_t s);
// bytes of tracker state of one sequence (zero = a sequence that has seen no scan)
size_t track_state_bytes();
// sequence q (one workgroup) runs its d_n_scans[q] scans -- group sum(d_n_scans[0 .. q)) + i of (d_records, d_begin, d_end) is its
// scan i -- through the tracker and writes one rsx_cfear_track_result per scan at the same index of d_out.  d_tau: the records'
// times, element for element beside d_records; read only with tp.compensate (null without)
int launch_track(const rsx_cfear_surface_point *d_records, const float *d_tau, const int64_t *d_begin, const int64_t *d_end, const int32_t *d_n_scans,
                 int32_t n_sequences, const rsx_cfear_params &p, const rsx_cfear_track_params &tp, void *d_state,
                 rsx_cfear_track_result *d_out, hipStream_t s);

}  // namespace cfear
}  // namespace rsx
