// gridrefine.hip -- refining a pose in the radar grid map below the cell on gfx950: Levenberg-Marquardt with an accept test on the
// bilinearly interpolated likelihood plane of the rsx_gridmap handle (Hector SLAM's matcher; the stage that Olson's and Cartographer's
// matchers put behind the correlative one).  None of this is in the reference checkout: the rule is the one stated in include/rsx.h
// and restated in tests/gridrefine_np.py (PARITY UNPINNED): fp64 on plain operations, nothing fused, and every sum in a stated order,
// so the records are the restatement's byte for byte.
//
// One launch per call whatever the batch, no atomics, no host round trip: gmr_refine runs one workgroup of 256 threads per job and the
// whole iteration in it (refine_record of gridrefine_dev.h, which the tracker of gridtrack.hip runs too).
//   an evaluation  thread t takes points t, t + 256, ... in that order, four at a time: the four points are read (the cloud is
//                  re-read from global memory at every evaluation -- 38 KB at 4800 points, served by L2; LDS holds nothing but the
//                  reduction's words, so what bounds the workgroups of a CU is registers), their four pairs of 16-bit reads of the
//                  plane are issued together, and the eleven terms of each are added to the thread's partial sums in the points'
//                  order.  A slot past the end of the job adds +0.0, which changes no partial (none is ever -0.0).  The reads are
//                  the framed plane's own (gridmap.h): a placed point's four bytes lie at most 65 cells outside the map, inside the
//                  128-cell frame, so nothing tests a bound; a point that is not placed reads cell (0, 0) and its terms are replaced.
//   the sums       rsx::wave::sum_f64_rows_pair in each of the four wavefronts, lane 0 leaves the wavefront's word in LDS, every
//                  thread adds (w0 + w1) + (w2 + w3): the balanced adjacent tree over the 256 partials.
//   the step       the 3 x 3 solve, the clamp, the pose update and the accept test are computed by every thread from the same sums:
//                  the same bits in every thread, every branch on them workgroup-uniform, no broadcast.
// The two batch entries are the scaffold of gridloc_host.h behind their own rules: a call with no side output, so one cut of the batch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>

#include "gridloc_host.h"
#include "gridmap.h"
#include "gridmatch_dev.h"
#include "gridrefine_dev.h"

#pragma STDC FP_CONTRACT OFF

namespace {

using rsx::fail;
using rsx::GRIDMAP_LIKE_MARGIN;
using rsx::gridmatch_dev::job_points;
using rsx::gridmatch_dev::NT;
using rsx::gridmatch_dev::PLACE;
using rsx::gridrefine_dev::refine_record;
using rsx::gridrefine_dev::RefineGeo;
using rsx::gridrefine_dev::RefineLds;
namespace gridloc = rsx::gridloc;

static_assert(PLACE + 2 < GRIDMAP_LIKE_MARGIN, "the four bytes of a placed point must stay in the frame");

__global__ __launch_bounds__(NT) void gmr_refine(const float *__restrict__ xy, int64_t stride, const int64_t *__restrict__ offsets,
                                                 const double *__restrict__ priors, RefineGeo g, rsx_gridmap_refine_params prm,
                                                 const uint8_t *__restrict__ origin, rsx_gridmap_refine_result *__restrict__ results) {
  __shared__ RefineLds lds;
  const int job = blockIdx.x;
  int64_t first;
  const int64_t n64 = job_points(offsets, job, &first);
  const rsx_gridmap_refine_result r = refine_record(xy + first * stride, stride, n64, priors + 6 * (int64_t)job, g, prm, origin, &lds);
  if (threadIdx.x == 0) results[job] = r;
}

int resolve(const rsx_gridmap_refine_params *params, rsx_gridmap_refine_params &dp) {
  rsx_gridmap_refine_default_params(&dp);
  if (params) dp = *params;
  return gridloc::check_refine_params(dp);
}

// the call as gridloc_host.h's scaffold takes it: no side output, and the one launch
gridloc::LocCall describe(const rsx_gridmap_refine_params &p) {
  return {gridloc::have_likelihood, 0, nullptr, sizeof(rsx_gridmap_refine_result),
          [&p](rsx_gridmap *h, const gridloc::LocJobs &j, void *d_results, uint32_t *, hipStream_t s) -> int {
            const RefineGeo g = gridloc::refine_geo(h);
            hipLaunchKernelGGL(gmr_refine, dim3((unsigned)j.n), dim3(NT), 0, s, j.xy, j.stride, j.off, j.priors, g, p, (const uint8_t *)h->like_origin(),
                               static_cast<rsx_gridmap_refine_result *>(d_results));
            RSX_HIP(hipGetLastError());
            return RSX_OK;
          }};
}

}  // namespace

extern "C" {

int rsx_gridmap_refine_default_params(rsx_gridmap_refine_params *p) try {
  if (!p) return fail(RSX_ERR_BAD_ARG, "null params");
  p->damping = 1e-3;
  p->max_shift_step = 1.0;
  p->max_rotation_step = 0.02;
  p->shift_tolerance = 1e-3;
  p->rotation_tolerance = 1e-5;
  p->max_evaluations = 32;
  p->reserved = 0;
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_gridmap_refine_batch_device(rsx_gridmap *h, const float *d_xy, const int64_t *d_offsets, int32_t point_stride, int32_t n_jobs,
                                    const double *d_priors, const rsx_gridmap_refine_params *params, rsx_gridmap_refine_result *d_results,
                                    void *stream) try {
  RSX_TRY(gridloc::check_args(d_xy, d_offsets, d_priors, d_results, n_jobs, point_stride));
  rsx_gridmap_refine_params dp;
  RSX_TRY(resolve(params, dp));
  return gridloc::run_device(h, describe(dp), {d_xy, d_offsets, point_stride, n_jobs, d_priors}, d_results, nullptr, stream);
} RSX_CATCH_ALL

int rsx_gridmap_refine_batch(rsx_gridmap *h, const float *xy, const int64_t *offsets, int32_t n_jobs, const double *priors,
                             const rsx_gridmap_refine_params *params, rsx_gridmap_refine_result *out_results) try {
  RSX_TRY(gridloc::check_args(xy, offsets, priors, out_results, n_jobs, 2));
  rsx_gridmap_refine_params dp;
  RSX_TRY(resolve(params, dp));
  return gridloc::run_host(h, describe(dp), "rsx_gridmap_refine_batch", xy, offsets, n_jobs, priors, out_results, nullptr);
} RSX_CATCH_ALL

}  // extern "C"
