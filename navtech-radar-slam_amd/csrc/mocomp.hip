// mocomp.hip -- motion (deskewing) and Doppler compensation of radar keypoints: the corrections the upstream odometry
// switches on with ORORA's deskewing / Doppler options and yeti_radar_odometry's --doppler configuration.  Their sources are
// an empty directory in the reference checkout, so this implements the model written in include/rsx.h as restated in
// tests/mocomp_np.py (PARITY UNPINNED); that file is the arithmetic contract: every product and sum below stands where it
// stands there, and nothing is fused (the library is built with -ffp-contract=off, and this file switches contraction off
// itself as well).
//
// One thread per point (or per match: both of its points), fp64 arithmetic on fp32 float2 loads and stores; the velocity of
// a scan / the pose of a pair is read through a wave-uniform address (scalar loads) once per workgroup.  No LDS, no barrier,
// no atomics: the status bit is a plain store of the same value by every thread that finds a reason.
//
// The polynomials sn, cs, A, B and the velocity of a pose are csrc/mocomp_dev.h's (shared with the CFEAR record compensation);
// their truncation bound is proved there.
// sqrt and / are correctly rounded in fp64 on gfx950, fp64 -> fp32 rounds to nearest even on both sides.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <new>

#include "mocomp.h"
#include "mocomp_dev.h"
#include "ragged_host.h"

#pragma STDC FP_CONTRACT OFF

namespace {

constexpr int NT = 256;
constexpr int CHUNKS = 16;  // workgroups per scan / pair: 4096 points per sweep, more by a grid-stride loop
using rsx::mocomp::Poly;
using rsx::mocomp::poly;
using rsx::mocomp::TH_MAX;
using rsx::mocomp::velocity_of;

struct Consts {
  double dt_scan, beta, rows;
  int flags;
};

// one point measured on azimuth row a under the velocity (vx, vy, wz); true: left as measured (not |th| <= 1/2)
__device__ __forceinline__ bool compensate(float2 p, int a, double vx, double vy, double wz, const Consts &k, float2 &out) {
  double x = p.x, y = p.y;
  const double tau = (((double)a + 0.5) / k.rows) * k.dt_scan;
  const double th = wz * tau;
  if ((k.flags & RSX_MOCOMP_DESKEW) && !(fabs(th) <= TH_MAX)) {
    out = p;
    return true;
  }
  if (k.flags & RSX_MOCOMP_DOPPLER) {
    const double r = sqrt(x * x + y * y);
    if (r != 0.0) {
      const double cx = x / r, sy = y / r;
      const double rc = r + k.beta * (vx * cx + vy * sy);
      x = rc * cx;
      y = rc * sy;
    }
  }
  if (k.flags & RSX_MOCOMP_DESKEW) {
    const Poly f = poly(th);
    const double x0 = (f.cs * x - f.sn * y) + (f.A * vx - f.B * vy) * tau;
    const double y0 = (f.sn * x + f.cs * y) + (f.B * vx + f.A * vy) * tau;
    x = x0;
    y = y0;
  }
  out = make_float2((float)x, (float)y);
  return false;
}

// a pose record: doubles x, y, yaw at its start, optionally an int32 status at status_off.  -> 0 compensate with (vx, vy, wz),
// 1 copy through (status != 0), 2 copy through and flag (no velocity)
__device__ __forceinline__ int record_velocity(const char *__restrict__ pose, int64_t stride, int status_off, int64_t i, double dt_scan,
                                               double &vx, double &vy, double &wz) {
  const char *rec = pose + i * stride;
  const double *d = reinterpret_cast<const double *>(rec);
  const double x = d[0], y = d[1], yaw = d[2];
  vx = vy = wz = 0.0;
  if (status_off >= 0 && *reinterpret_cast<const int32_t *>(rec + status_off) != 0) return 1;
  return velocity_of(x, y, yaw, dt_scan, vx, vy, wz) ? 0 : 2;
}

__global__ __launch_bounds__(NT) void mocomp_points_kernel(const float2 *__restrict__ xy, const int32_t *__restrict__ rows,
                                                           const int64_t *__restrict__ offsets, const double *__restrict__ w, Consts k,
                                                           float2 *__restrict__ out, int32_t *__restrict__ status) {
  const int scan = blockIdx.x / CHUNKS, chunk = blockIdx.x % CHUNKS;
  const int64_t o = offsets[scan], n = offsets[scan + 1] - o;
  const double vx = w[3 * (int64_t)scan], vy = w[3 * (int64_t)scan + 1], wz = w[3 * (int64_t)scan + 2];
  for (int64_t i = (int64_t)chunk * NT + threadIdx.x; i < n; i += (int64_t)CHUNKS * NT) {
    float2 r;
    const bool bad = compensate(xy[o + i], rows[o + i], vx, vy, wz, k, r);
    out[o + i] = r;
    if (bad && status) status[scan] = RSX_MOCOMP_STATUS_ANGLE;
  }
}

__global__ __launch_bounds__(NT) void mocomp_matches_kernel(const float2 *__restrict__ src, const float2 *__restrict__ dst,
                                                            const int32_t *__restrict__ a_cur, const int32_t *__restrict__ a_prev,
                                                            const int64_t *__restrict__ offsets, const char *__restrict__ pose, int64_t pose_stride,
                                                            int status_off, Consts k, float2 *__restrict__ out_src, float2 *__restrict__ out_dst,
                                                            int32_t *__restrict__ status) {
  const int pair = blockIdx.x / CHUNKS, chunk = blockIdx.x % CHUNKS;
  const int64_t o = offsets[pair], n = offsets[pair + 1] - o;
  double vx, vy, wz;
  const int how = record_velocity(pose, pose_stride, status_off, pair, k.dt_scan, vx, vy, wz);
  if (how == 2 && status && chunk == 0 && threadIdx.x == 0) status[pair] = RSX_MOCOMP_STATUS_ANGLE;
  for (int64_t i = (int64_t)chunk * NT + threadIdx.x; i < n; i += (int64_t)CHUNKS * NT) {
    const float2 ps = src[o + i], pd = dst[o + i];
    float2 rs = ps, rd = pd;
    if (how == 0) {
      const bool b1 = compensate(ps, a_cur[o + i], vx, vy, wz, k, rs);
      const bool b2 = compensate(pd, a_prev[o + i], vx, vy, wz, k, rd);
      if ((b1 || b2) && status) status[pair] = RSX_MOCOMP_STATUS_ANGLE;
    }
    out_src[o + i] = rs;
    out_dst[o + i] = rd;
  }
}

__global__ __launch_bounds__(NT) void mocomp_slots_kernel(const float2 *__restrict__ xy, const int32_t *__restrict__ targets,
                                                          const int32_t *__restrict__ counts, int stride, int first, const char *__restrict__ pose,
                                                          int64_t pose_stride, int status_off, Consts k, float2 *__restrict__ out) {
  const int scan = blockIdx.x / CHUNKS, chunk = blockIdx.x % CHUNKS;
  const int n = counts[scan] < stride ? counts[scan] : stride;
  const int64_t o = (int64_t)scan * stride;
  double vx = 0.0, vy = 0.0, wz = 0.0;
  const int how = scan < first ? 1 : record_velocity(pose, pose_stride, status_off, scan - first, k.dt_scan, vx, vy, wz);
  for (int i = chunk * NT + threadIdx.x; i < n; i += CHUNKS * NT) {
    const float2 p = xy[o + i];
    float2 r = p;
    if (how == 0) (void)compensate(p, targets[(o + i) * 2], vx, vy, wz, k, r);
    out[o + i] = r;
  }
}

Consts consts_of(const rsx_mocomp_params &p) {
  Consts k;
  k.dt_scan = p.dt_scan;
  k.beta = p.beta;
  k.rows = (double)p.rows;
  k.flags = p.flags;
  return k;
}

constexpr int32_t MAX_GROUPS = 0x7fffffff / CHUNKS;  // scans / pairs per call: the grid is groups x CHUNKS workgroups

int launch_points(const float *d_xy, const int32_t *d_rows, const int64_t *d_off, int32_t n_scans, const double *d_w, const rsx_mocomp_params &p,
                  float *d_out, int32_t *d_status, hipStream_t s) {
  if (d_status) RSX_HIP(hipMemsetAsync(d_status, 0, (size_t)n_scans * 4, s));
  hipLaunchKernelGGL(mocomp_points_kernel, dim3((unsigned)n_scans * CHUNKS), dim3(NT), 0, s, reinterpret_cast<const float2 *>(d_xy), d_rows, d_off,
                     d_w, consts_of(p), reinterpret_cast<float2 *>(d_out), d_status);
  RSX_HIP(hipGetLastError());
  return RSX_OK;
}

}  // namespace

using rsx::fail;

int rsx::mocomp::check_params(const rsx_mocomp_params &p) {
  if (!(p.flags & (RSX_MOCOMP_DESKEW | RSX_MOCOMP_DOPPLER))) return fail(RSX_ERR_BAD_ARG, "neither RSX_MOCOMP_DESKEW nor RSX_MOCOMP_DOPPLER is set");
  if (p.flags & ~(RSX_MOCOMP_DESKEW | RSX_MOCOMP_DOPPLER)) return fail(RSX_ERR_BAD_ARG, "unknown flags");
  if (!(p.dt_scan > 0.0) || !std::isfinite(p.dt_scan)) return fail(RSX_ERR_BAD_ARG, "dt_scan must be positive");
  if (!std::isfinite(p.beta)) return fail(RSX_ERR_BAD_ARG, "beta must be finite");
  if (p.rows < 1) return fail(RSX_ERR_BAD_ARG, "rows must be positive");
  return RSX_OK;
}

int rsx::mocomp::launch_matches(const float *d_src, const float *d_dst, const int32_t *d_a_cur, const int32_t *d_a_prev, const int64_t *d_offsets,
                                int32_t n_pairs, const void *d_pose, int64_t pose_stride, int32_t status_off, const rsx_mocomp_params &p,
                                float *d_out_src, float *d_out_dst, int32_t *d_out_status, hipStream_t s) {
  if (n_pairs < 1 || n_pairs > MAX_GROUPS) return fail(RSX_ERR_BAD_ARG, "n_pairs %d outside [1, %d]", n_pairs, MAX_GROUPS);
  if (d_out_status) RSX_HIP(hipMemsetAsync(d_out_status, 0, (size_t)n_pairs * 4, s));
  hipLaunchKernelGGL(mocomp_matches_kernel, dim3((unsigned)n_pairs * CHUNKS), dim3(NT), 0, s, reinterpret_cast<const float2 *>(d_src),
                     reinterpret_cast<const float2 *>(d_dst), d_a_cur, d_a_prev, d_offsets, static_cast<const char *>(d_pose), pose_stride,
                     (int)status_off, consts_of(p), reinterpret_cast<float2 *>(d_out_src), reinterpret_cast<float2 *>(d_out_dst), d_out_status);
  RSX_HIP(hipGetLastError());
  return RSX_OK;
}

int rsx::mocomp::launch_slots(const float *d_xy, const int32_t *d_targets, const int32_t *d_counts, int32_t stride, int32_t n_scans, int32_t first,
                              const void *d_pose, int64_t pose_stride, int32_t status_off, const rsx_mocomp_params &p, float *d_out_xy,
                              hipStream_t s) {
  if (n_scans < 1 || n_scans > MAX_GROUPS) return fail(RSX_ERR_BAD_ARG, "n_scans %d outside [1, %d]", n_scans, MAX_GROUPS);
  hipLaunchKernelGGL(mocomp_slots_kernel, dim3((unsigned)n_scans * CHUNKS), dim3(NT), 0, s, reinterpret_cast<const float2 *>(d_xy), d_targets,
                     d_counts, (int)stride, (int)first, static_cast<const char *>(d_pose), pose_stride, (int)status_off, consts_of(p),
                     reinterpret_cast<float2 *>(d_out_xy));
  RSX_HIP(hipGetLastError());
  return RSX_OK;
}

struct rsx_mocomp {
  int device = 0;
  std::mutex mu;
  rsx::Stream stream;
  rsx::StreamOrder order;  // the staging buffers are shared by every host-buffer call
  rsx::DevBuf in0, in1, a0, a1, off, vel, out0, out1, st;  // staging of the host-buffer entries
};

namespace {

int resolve_params(const rsx_mocomp_params *params, rsx_mocomp_params &dp) {
  rsx_mocomp_default_params(&dp);
  if (params) dp = *params;
  return rsx::mocomp::check_params(dp);
}

}  // namespace

extern "C" {

int rsx_mocomp_default_params(rsx_mocomp_params *p) try {
  if (!p) return fail(RSX_ERR_BAD_ARG, "null params");
  p->dt_scan = 0.25;
  p->beta = 0.049;
  p->rows = 400;
  p->flags = RSX_MOCOMP_DESKEW | RSX_MOCOMP_DOPPLER;
  p->reserved[0] = p->reserved[1] = 0;
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_mocomp_create(int device, rsx_mocomp **out) try {
  if (!out) return fail(RSX_ERR_BAD_ARG, "null out");
  *out = nullptr;
  RSX_TRY(rsx::check_device(device));
  std::unique_ptr<rsx_mocomp> h(new (std::nothrow) rsx_mocomp());
  if (!h) return fail(RSX_ERR_OOM, "host alloc");
  h->device = device;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = h->stream.create();
  if (e != hipSuccess) return fail(RSX_ERR_HIP, "create: %s", hipGetErrorString(e));
  *out = h.release();
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_mocomp_destroy(rsx_mocomp *h) try {
  if (!h) return RSX_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  delete h;
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_mocomp_points_batch_device(rsx_mocomp *h, const float *d_xy, const int32_t *d_rows, const int64_t *d_offsets, int32_t n_scans,
                                   const double *d_w, const rsx_mocomp_params *params, float *d_out_xy, int32_t *d_out_status, void *stream) try {
  if (!h || !d_xy || !d_rows || !d_offsets || !d_w || !d_out_xy || n_scans < 0) return fail(RSX_ERR_BAD_ARG, "bad arg");
  if (d_out_xy == d_xy) return fail(RSX_ERR_BAD_ARG, "out_xy must not be xy");
  rsx_mocomp_params dp;
  RSX_TRY(resolve_params(params, dp));
  if (n_scans == 0) return RSX_OK;
  if (n_scans > MAX_GROUPS) return fail(RSX_ERR_BAD_ARG, "n_scans above %d", MAX_GROUPS);
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
  RSX_TRY(h->order.enter(s));
  return launch_points(d_xy, d_rows, d_offsets, n_scans, d_w, dp, d_out_xy, d_out_status, s);
} RSX_CATCH_ALL

int rsx_mocomp_points_batch(rsx_mocomp *h, const float *xy, const int32_t *rows, const int64_t *offsets, int32_t n_scans, const double *w,
                            const rsx_mocomp_params *params, float *out_xy, int32_t *out_status) try {
  if (!h || !xy || !rows || !offsets || !w || !out_xy || n_scans < 0) return fail(RSX_ERR_BAD_ARG, "bad arg");
  rsx_mocomp_params dp;
  RSX_TRY(resolve_params(params, dp));
  if (n_scans == 0) return RSX_OK;
  if (n_scans > MAX_GROUPS) return fail(RSX_ERR_BAD_ARG, "n_scans above %d", MAX_GROUPS);
  RSX_TRY(rsx::check_offsets(offsets, n_scans, "rsx_mocomp_points_batch"));
  const size_t m = (size_t)offsets[n_scans], n = (size_t)n_scans;
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  RSX_TRY(h->order.enter(s));
  RSX_TRY(rsx::stage_up(h->in0, xy, m * 8, s));
  RSX_TRY(rsx::stage_up(h->a0, rows, m * 4, s));
  RSX_TRY(rsx::stage_up(h->off, offsets, (n + 1) * 8, s));
  RSX_TRY(rsx::stage_up(h->vel, w, n * 24, s));
  RSX_TRY(rsx::stage_room(h->out0, m * 8, s));
  RSX_TRY(rsx::stage_room(h->st, n * 4, s));
  RSX_TRY(launch_points(h->in0.as<float>(), h->a0.as<int32_t>(), h->off.as<int64_t>(), n_scans, h->vel.as<double>(), dp, h->out0.as<float>(),
                        h->st.as<int32_t>(), s));
  RSX_TRY(rsx::stage_down(out_xy, h->out0, m * 8, s));
  RSX_TRY(rsx::stage_down(out_status, h->st, n * 4, s));
  RSX_HIP(hipStreamSynchronize(s));
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_mocomp_matches_batch_device(rsx_mocomp *h, const float *d_src_xy, const float *d_dst_xy, const int32_t *d_a_cur, const int32_t *d_a_prev,
                                    const int64_t *d_offsets, int32_t n_pairs, const double *d_pose, const rsx_mocomp_params *params,
                                    float *d_out_src_xy, float *d_out_dst_xy, int32_t *d_out_status, void *stream) try {
  if (!h || !d_src_xy || !d_dst_xy || !d_a_cur || !d_a_prev || !d_offsets || !d_pose || !d_out_src_xy || !d_out_dst_xy || n_pairs < 0)
    return fail(RSX_ERR_BAD_ARG, "bad arg");
  if (d_out_src_xy == d_src_xy || d_out_dst_xy == d_dst_xy || d_out_src_xy == d_out_dst_xy)
    return fail(RSX_ERR_BAD_ARG, "the outputs must be buffers of their own");
  rsx_mocomp_params dp;
  RSX_TRY(resolve_params(params, dp));
  if (n_pairs == 0) return RSX_OK;
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
  RSX_TRY(h->order.enter(s));
  return rsx::mocomp::launch_matches(d_src_xy, d_dst_xy, d_a_cur, d_a_prev, d_offsets, n_pairs, d_pose, 24, -1, dp, d_out_src_xy, d_out_dst_xy,
                                     d_out_status, s);
} RSX_CATCH_ALL

int rsx_mocomp_matches_batch(rsx_mocomp *h, const float *src_xy, const float *dst_xy, const int32_t *a_cur, const int32_t *a_prev,
                             const int64_t *offsets, int32_t n_pairs, const double *pose, const rsx_mocomp_params *params, float *out_src_xy,
                             float *out_dst_xy, int32_t *out_status) try {
  if (!h || !src_xy || !dst_xy || !a_cur || !a_prev || !offsets || !pose || !out_src_xy || !out_dst_xy || n_pairs < 0)
    return fail(RSX_ERR_BAD_ARG, "bad arg");
  rsx_mocomp_params dp;
  RSX_TRY(resolve_params(params, dp));
  if (n_pairs == 0) return RSX_OK;
  RSX_TRY(rsx::check_offsets(offsets, n_pairs, "rsx_mocomp_matches_batch"));
  const size_t m = (size_t)offsets[n_pairs], n = (size_t)n_pairs;
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  RSX_TRY(h->order.enter(s));
  RSX_TRY(rsx::stage_up(h->in0, src_xy, m * 8, s));
  RSX_TRY(rsx::stage_up(h->in1, dst_xy, m * 8, s));
  RSX_TRY(rsx::stage_up(h->a0, a_cur, m * 4, s));
  RSX_TRY(rsx::stage_up(h->a1, a_prev, m * 4, s));
  RSX_TRY(rsx::stage_up(h->off, offsets, (n + 1) * 8, s));
  RSX_TRY(rsx::stage_up(h->vel, pose, n * 24, s));
  RSX_TRY(rsx::stage_room(h->out0, m * 8, s));
  RSX_TRY(rsx::stage_room(h->out1, m * 8, s));
  RSX_TRY(rsx::stage_room(h->st, n * 4, s));
  RSX_TRY(rsx::mocomp::launch_matches(h->in0.as<float>(), h->in1.as<float>(), h->a0.as<int32_t>(), h->a1.as<int32_t>(), h->off.as<int64_t>(), n_pairs,
                                      h->vel.p, 24, -1, dp, h->out0.as<float>(), h->out1.as<float>(), h->st.as<int32_t>(), s));
  RSX_TRY(rsx::stage_down(out_src_xy, h->out0, m * 8, s));
  RSX_TRY(rsx::stage_down(out_dst_xy, h->out1, m * 8, s));
  RSX_TRY(rsx::stage_down(out_status, h->st, n * 4, s));
  RSX_HIP(hipStreamSynchronize(s));
  return RSX_OK;
} RSX_CATCH_ALL

}  // extern "C"
