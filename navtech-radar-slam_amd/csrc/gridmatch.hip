// gridmatch.hip -- localising a point cloud in the radar grid map on gfx950: the likelihood plane of the rsx_gridmap handle and the
// exhaustive correlative matching of clouds against it (rotations -K .. K, whole-cell shifts -V .. V and -U .. U around a prior pose).
// None of this is in the reference checkout: the rule is the one stated in include/rsx.h and restated in tests/gridmatch_np.py
// (PARITY UNPINNED): fp64 on plain operations up to the cell of a point, integers from there on, so the scores are the restatement's
// byte for byte whatever the order of the sums.
//
// The plane lies in a zeroed frame of GRIDMAP_LIKE_MARGIN cells (gridmap.h): a placed point's cell is at most 64 cells outside the
// map, a shift at most 32, a read four bytes wide, so every read is a byte of the buffer, a cell outside the map reads 0 and the inner
// loop tests no bound.  A point that is not placed is given the cell (-64, -64), from which no candidate reaches the map.
// Two launches per call whatever the batch, no atomics on device memory:
//   gmm_score  one workgroup per (job, k).  Every thread takes points t, t + 256, ... through steps 1 - 5 of the rule and leaves
//              their byte offsets into the framed plane in LDS (32 KB at the cap).  Then a thread owns a SLOT, four neighbouring u
//              of one v; with S = (2V + 1) ceil((2U + 1) / 4) slots and P = max(1, 256 / S), the points are dealt to P parts and
//              thread part S + slot walks its part: the offset comes from LDS (a broadcast within a part), the four bytes from one
//              unaligned 32-bit read (neighbouring slots read neighbouring bytes; the plane is served by L2), and they are added as
//              two pairs of 16-bit sums that are flushed every 256 points, before they can overflow; eight reads are in flight
//              per thread (the trip count is known before the loop: an exit test inside it costs a wait per read).  The parts are added
//              through LDS; with S above 256 a thread walks several slots in turn (slot_sums of gridmatch_dev.h, which the
//              search's gms_bound shares).
//   gmm_pick   one workgroup per job: pick_record of gridmatch_dev.h -- the winner by a 64-bit key that carries the tie order and the
//              linear index, then the runner-up and, from steps 1 - 5 again at the winner's k, the counts; thread 0 writes the record.
// The two batch entries are the scaffold of gridloc_host.h behind their own rules; the rules that gridmap.hip judges too are in gridmap.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>

#include "gridloc_host.h"
#include "gridmap.h"
#include "gridmatch_dev.h"

#pragma STDC FP_CONTRACT OFF

namespace {

using rsx::check_render;  // (gridmap.h)
using rsx::fail;
using rsx::no_likelihood;
using rsx::GRIDMAP_LIKE_MARGIN;
using namespace rsx::gridmatch_dev;  // NT, PLACE, MatchGeo, Rotations, place, job_points, skip_status, fill_cells, slot_sums, pick_record
namespace gridloc = rsx::gridloc;

constexpr int MAX_POINTS = RSX_GRIDMAP_MATCH_MAX_POINTS;
constexpr int MAX_K = 64, MAX_UV = 32;
static_assert(PLACE + MAX_UV + 3 < GRIDMAP_LIKE_MARGIN, "a shifted read must stay in the frame");
static_assert((MAX_POINTS & (MAX_POINTS - 1)) == 0, "");

using Tables = Rotations<MAX_K>;

__global__ __launch_bounds__(NT) void gmm_score(const float *__restrict__ xy, int64_t stride, const int64_t *__restrict__ offsets,
                                                const double *__restrict__ priors, Tables tab, MatchGeo g,
                                                const uint8_t *__restrict__ plane, unsigned *__restrict__ volume) {
  __shared__ unsigned cell[MAX_POINTS];  // byte offset of the point's cell in the framed plane
  __shared__ unsigned red[NT * 4];
  const int tid = threadIdx.x;
  const int nk = 2 * g.K + 1, nv = 2 * g.V + 1, nu = 2 * g.U + 1;
  const int job = (int)(blockIdx.x / (unsigned)nk), kk = (int)(blockIdx.x % (unsigned)nk);
  unsigned *out = volume + ((int64_t)job * nk + kk) * nv * nu;
  const double *t = priors + 6 * (int64_t)job;
  int64_t first;
  const int64_t n64 = job_points(offsets, job, &first);
  if (skip_status(t, n64)) {  // (workgroup-uniform) a skipped job: its scores are 0
    for (int i = tid; i < nv * nu; i += NT) out[i] = 0u;
    return;
  }
  const double c = (double)tab.c[kk], s = (double)tab.s[kk];
  const double t6[6] = {t[0], t[1], t[2], t[3], t[4], t[5]};
  const int n = (int)n64;
  fill_cells(g, GRIDMAP_LIKE_MARGIN, xy, stride, first, n, t6, c, s, cell);
  __syncthreads();
  slot_sums(
      plane, cell, red, n, nv, nu, [&](int vi, int gi) { return (unsigned)((vi - g.V) * (int)g.pitch + (4 * gi - g.U)); },
      [&](int vi, int ui, unsigned sum) { out[vi * nu + ui] = sum; });
}

__global__ __launch_bounds__(NT) void gmm_pick(const float *__restrict__ xy, int64_t stride, const int64_t *__restrict__ offsets,
                                               const double *__restrict__ priors, Tables tab, MatchGeo g,
                                               const unsigned *__restrict__ volume, rsx_gridmap_match_result *__restrict__ results) {
  __shared__ PickLds lds;
  const int job = blockIdx.x;
  const int total = (2 * g.K + 1) * (2 * g.V + 1) * (2 * g.U + 1);
  int64_t first;
  const int64_t n64 = job_points(offsets, job, &first);
  const rsx_gridmap_match_result r = pick_record(xy, stride, first, n64, priors + 6 * (int64_t)job, tab, g, volume + (int64_t)job * total, &lds);
  if (threadIdx.x == 0) results[job] = r;
}

// one thread per cell: the byte of the likelihood plane from the planes -- render's rule (gm_render of gridmap.hip; include/rsx.h),
// the hit ratio with "unknown" as 0
__global__ __launch_bounds__(NT) void gmm_likelihood(const unsigned *__restrict__ p_sum, const unsigned *__restrict__ p_cnt,
                                                     const unsigned *__restrict__ p_hit, int W, int H, int mode, unsigned min_obs,
                                                     uint8_t *__restrict__ origin, int64_t pitch) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= (int64_t)W * H) return;
  const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
  const unsigned long long cnt = p_cnt[i];
  unsigned long long v = 0ull;
  if (cnt >= min_obs) {
    if (mode == RSX_GRIDMAP_MEAN) {
      v = (2ull * p_sum[i] + cnt) / (2ull * cnt);
      v = v < 255ull ? v : 255ull;
    } else {
      v = (200ull * p_hit[i] + cnt) / (2ull * cnt);
    }
  }
  origin[(int64_t)y * pitch + x] = (uint8_t)v;
}

int check_params(const rsx_gridmap_match_params &p) {
  RSX_TRY(gridloc::check_window_params(p, MAX_K, MAX_UV));
  if (p.reserved != 0) return fail(RSX_ERR_BAD_ARG, "reserved must be 0");
  return RSX_OK;
}

int resolve(const rsx_gridmap_match_params *params, rsx_gridmap_match_params &dp) {
  rsx_gridmap_match_default_params(&dp);
  if (params) dp = *params;
  return check_params(dp);
}

size_t candidates(const rsx_gridmap_match_params &p) { return (size_t)(2 * p.angle_steps + 1) * (2 * p.y_cells + 1) * (2 * p.x_cells + 1); }

// the framed plane, allocated and zeroed at the first call that needs it (the caller holds h->mu and has entered s)
int need_plane(rsx_gridmap *h, hipStream_t s) {
  if (h->like.p) return RSX_OK;
  RSX_TRY(h->like.reserve(h->like_bytes(), s, false));
  RSX_HIP(hipMemsetAsync(h->like.p, 0, h->like.bytes, s));
  return RSX_OK;
}

// the call as gridloc_host.h's scaffold takes it: a score volume of (2K + 1)(2V + 1)(2U + 1) words per job, in h->volume unless the
// caller gave room, and the two launches
gridloc::LocCall describe(const rsx_gridmap_match_params &p) {
  return {gridloc::have_likelihood, candidates(p), &rsx_gridmap::volume, sizeof(rsx_gridmap_match_result),
          [&p](rsx_gridmap *h, const gridloc::LocJobs &j, void *d_results, uint32_t *d_volume, hipStream_t s) -> int {
            const Tables tab(p.angle_steps, p.angle_step);
            const MatchGeo g = gridloc::match_geo(h, p.angle_steps, p.x_cells, p.y_cells, (unsigned)h->like_pitch());
            const unsigned nk = (unsigned)(2 * p.angle_steps + 1);
            hipLaunchKernelGGL(gmm_score, dim3((unsigned)j.n * nk), dim3(NT), 0, s, j.xy, j.stride, j.off, j.priors, tab, g, h->like.as<uint8_t>(), d_volume);
            RSX_HIP(hipGetLastError());
            hipLaunchKernelGGL(gmm_pick, dim3((unsigned)j.n), dim3(NT), 0, s, j.xy, j.stride, j.off, j.priors, tab, g, d_volume,
                               static_cast<rsx_gridmap_match_result *>(d_results));
            RSX_HIP(hipGetLastError());
            return RSX_OK;
          }};
}

}  // namespace

extern "C" {

int rsx_gridmap_match_default_params(rsx_gridmap_match_params *p) try {
  if (!p) return fail(RSX_ERR_BAD_ARG, "null params");
  p->angle_step = 0.01;
  p->angle_steps = 8;
  p->x_cells = 8;
  p->y_cells = 8;
  p->reserved = 0;
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_gridmap_likelihood_update(rsx_gridmap *h, int32_t mode, int32_t min_observations, void *stream) try {
  RSX_TRY(check_render(mode, min_observations));
  if (!h) return fail(RSX_ERR_BAD_ARG, "null handle");
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
  RSX_TRY(h->order.enter(s));
  RSX_TRY(need_plane(h, s));
  const int64_t n = (int64_t)h->p.width * h->p.height;
  hipLaunchKernelGGL(gmm_likelihood, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, s, h->plane(0), h->plane(1), h->plane(2), h->p.width, h->p.height,
                     mode, (unsigned)min_observations, h->like_origin(), h->like_pitch());
  RSX_HIP(hipGetLastError());
  h->have_like = true;
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_gridmap_likelihood_set(rsx_gridmap *h, const uint8_t *img) try {
  if (!img) return fail(RSX_ERR_BAD_ARG, "null image");
  if (!h) return fail(RSX_ERR_BAD_ARG, "null handle");
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  RSX_TRY(h->order.enter(s));
  RSX_TRY(need_plane(h, s));
  RSX_HIP(hipMemcpy2DAsync(h->like_origin(), (size_t)h->like_pitch(), img, (size_t)h->p.width, (size_t)h->p.width, (size_t)h->p.height,
                           hipMemcpyHostToDevice, s));
  RSX_HIP(hipStreamSynchronize(s));
  h->have_like = true;
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_gridmap_likelihood_device(rsx_gridmap *h, uint8_t **d_likelihood, int64_t *pitch_bytes) try {
  if (!h) return fail(RSX_ERR_BAD_ARG, "null handle");
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  RSX_TRY(h->order.enter(s));
  RSX_TRY(need_plane(h, s));
  RSX_HIP(hipStreamSynchronize(s));  // (the frame is zero before the caller can write)
  h->have_like = true;
  if (d_likelihood) *d_likelihood = h->like_origin();
  if (pitch_bytes) *pitch_bytes = h->like_pitch();
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_gridmap_likelihood_read(rsx_gridmap *h, int32_t x, int32_t y, int32_t w, int32_t hgt, uint8_t *out) try {
  if (!out) return fail(RSX_ERR_BAD_ARG, "null out");
  if (!h) return fail(RSX_ERR_BAD_ARG, "null handle");
  RSX_TRY(rsx::check_window(h, x, y, w, hgt));
  std::lock_guard<std::mutex> lk(h->mu);
  if (!h->have_like) return no_likelihood();
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  RSX_TRY(h->order.enter(s));
  RSX_HIP(hipMemcpy2DAsync(out, (size_t)w, h->like_origin() + (size_t)y * h->like_pitch() + x, (size_t)h->like_pitch(), (size_t)w, (size_t)hgt,
                           hipMemcpyDeviceToHost, s));
  RSX_HIP(hipStreamSynchronize(s));
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_gridmap_match_batch_device(rsx_gridmap *h, const float *d_xy, const int64_t *d_offsets, int32_t point_stride, int32_t n_jobs,
                                   const double *d_priors, const rsx_gridmap_match_params *params, rsx_gridmap_match_result *d_results,
                                   uint32_t *d_scores, void *stream) try {
  RSX_TRY(gridloc::check_args(d_xy, d_offsets, d_priors, d_results, n_jobs, point_stride));
  rsx_gridmap_match_params dp;
  RSX_TRY(resolve(params, dp));
  if ((int64_t)n_jobs * (2 * dp.angle_steps + 1) > 0x7fffffffll) return fail(RSX_ERR_BAD_ARG, "n_jobs %d times %d rotations is 2^31 or more", n_jobs, 2 * dp.angle_steps + 1);
  return gridloc::run_device(h, describe(dp), {d_xy, d_offsets, point_stride, n_jobs, d_priors}, d_results, d_scores, stream);
} RSX_CATCH_ALL

int rsx_gridmap_match_batch(rsx_gridmap *h, const float *xy, const int64_t *offsets, int32_t n_jobs, const double *priors,
                            const rsx_gridmap_match_params *params, rsx_gridmap_match_result *out_results, uint32_t *out_scores) try {
  RSX_TRY(gridloc::check_args(xy, offsets, priors, out_results, n_jobs, 2));
  rsx_gridmap_match_params dp;
  RSX_TRY(resolve(params, dp));
  return gridloc::run_host(h, describe(dp), "rsx_gridmap_match_batch", xy, offsets, n_jobs, priors, out_results, out_scores);
} RSX_CATCH_ALL

}  // extern "C"
