// gridrefine.hip -- refining a pose in the radar grid map below the cell on gfx950: Levenberg-Marquardt with an accept test on the
// bilinearly interpolated likelihood plane of the rsx_gridmap handle (Hector SLAM's matcher; the stage that Olson's and Cartographer's
// matchers put behind the correlative one).  None of this is in the reference checkout: the rule is the one stated in include/rsx.h
// and restated in tests/gridrefine_np.py (PARITY UNPINNED): fp64 on plain operations, nothing fused, and every sum in a stated order,
// so the records are the restatement's byte for byte.
//
// One launch per call whatever the batch, no atomics, no host round trip: gmr_refine runs one workgroup of 256 threads per job and the
// whole iteration in it.
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
#include "mocomp_dev.h"
#include "rsx_wave_dev.h"

#pragma STDC FP_CONTRACT OFF

namespace {

using rsx::fail;
using rsx::GRIDMAP_LIKE_MARGIN;
using rsx::gridmatch_dev::job_points;
using rsx::gridmatch_dev::NT;
using rsx::gridmatch_dev::PLACE;
using rsx::gridmatch_dev::skip_status;
namespace gridloc = rsx::gridloc;

constexpr int NS = 11;      // cost, score, g0 g1 g2, H00 H01 H02 H11 H12 H22
constexpr int DEPTH = 4;    // points of a thread whose reads are in flight together
constexpr double LAMBDA_MIN = 1e-9, LAMBDA_MAX = 1e6;
static_assert(PLACE + 2 < GRIDMAP_LIKE_MARGIN, "the four bytes of a placed point must stay in the frame");
static_assert(sizeof(rsx_gridmap_refine_params) == 48 && sizeof(rsx_gridmap_refine_result) == 152, "");

struct RefineGeo {
  double ox, oy, inv_res, res;
  double x_hi, y_hi;  // width + 64, height + 64
  double w, h;        // width, height
  int64_t pitch;      // of the framed plane
};

struct Sums {
  double s[NS];
  int placed, inside;
};

__device__ __forceinline__ bool finite1(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// one evaluation at pose t (r00 r01 tx r10 r11 ty): every thread returns the same sums.  red, cnt: the LDS words of the reduction
__device__ __forceinline__ Sums evaluate(const float *__restrict__ xy, int64_t stride, int n, const double *t, const RefineGeo &g,
                                         const uint8_t *__restrict__ origin, double (*red)[NS], int (*cnt)[2]) {
  const int tid = threadIdx.x;
  double acc[NS];
#pragma unroll
  for (int q = 0; q < NS; q++) acc[q] = 0.0;
  int placed_n = 0, inside_n = 0;
  for (int base = 0; base < n; base += DEPTH * NT) {  // (workgroup-uniform trip count)
    float x[DEPTH], y[DEPTH];
    bool live[DEPTH];
#pragma unroll
    for (int e = 0; e < DEPTH; e++) {
      const int i = base + e * NT + tid;
      live[e] = i < n;
      const float *p = xy + (int64_t)(live[e] ? i : 0) * stride;  // (n > 0 here: point 0 exists)
      x[e] = p[0], y[e] = p[1];
    }
    double rx[DEPTH], ry[DEPTH], a[DEPTH], b[DEPTH];
    bool fin[DEPTH], ok[DEPTH];
    unsigned short w0[DEPTH], w1[DEPTH];
#pragma unroll
    for (int e = 0; e < DEPTH; e++) {
      const double xd = (double)x[e], yd = (double)y[e];
      fin[e] = live[e] && finite1(x[e]) && finite1(y[e]);
      rx[e] = t[0] * xd + t[1] * yd;
      ry[e] = t[3] * xd + t[4] * yd;
      const double fx = ((rx[e] + t[2]) - g.ox) * g.inv_res, fy = ((ry[e] + t[5]) - g.oy) * g.inv_res;
      ok[e] = fin[e] && fx >= -(double)PLACE && fx < g.x_hi && fy >= -(double)PLACE && fy < g.y_hi;  // (a NaN fails)
      placed_n += ok[e] ? 1 : 0;
      inside_n += (ok[e] && fx >= 0.0 && fx < g.w && fy >= 0.0 && fy < g.h) ? 1 : 0;  // floor(fx) in [0, width): the same test
      const double px = (ok[e] ? fx : 0.5) - 0.5, py = (ok[e] ? fy : 0.5) - 0.5;
      const double fi = floor(px), fj = floor(py);
      a[e] = px - fi, b[e] = py - fj;
      const uint8_t *q = origin + ((int64_t)fj * g.pitch + (int64_t)fi);  // fi in [-65, width + 63], fj likewise: inside the frame
      __builtin_memcpy(&w0[e], q, 2);
      __builtin_memcpy(&w1[e], q + g.pitch, 2);
    }
#pragma unroll
    for (int e = 0; e < DEPTH; e++) {
      const double l00 = (double)(w0[e] & 0xffu), l01 = (double)(w0[e] >> 8), l10 = (double)(w1[e] & 0xffu), l11 = (double)(w1[e] >> 8);
      const double na = 1.0 - a[e], nb = 1.0 - b[e];
      const double top = na * l00 + a[e] * l01, bot = na * l10 + a[e] * l11;
      double M = nb * top + b[e] * bot;
      double gx = nb * (l01 - l00) + b[e] * (l11 - l10);
      double gy = na * (l10 - l00) + a[e] * (l11 - l01);
      double jt = (gy * rx[e] - gx * ry[e]) * g.inv_res;
      M = ok[e] ? M : 0.0, gx = ok[e] ? gx : 0.0, gy = ok[e] ? gy : 0.0, jt = ok[e] ? jt : 0.0;
      const double r = ok[e] ? 255.0 - M : (fin[e] ? 255.0 : 0.0);
      acc[0] = acc[0] + r * r;
      acc[1] = acc[1] + M;
      acc[2] = acc[2] + gx * r;
      acc[3] = acc[3] + gy * r;
      acc[4] = acc[4] + jt * r;
      acc[5] = acc[5] + gx * gx;
      acc[6] = acc[6] + gx * gy;
      acc[7] = acc[7] + gx * jt;
      acc[8] = acc[8] + gy * gy;
      acc[9] = acc[9] + gy * jt;
      acc[10] = acc[10] + jt * jt;
    }
  }
  // (the whole workgroup is here: the loop's trip count is uniform)
  const int wv = tid >> 6, lane = tid & 63;
#pragma unroll
  for (int q = 0; q < NS; q++) {
    const double s = rsx::wave::sum_f64_rows_pair(acc[q]);
    if (lane == 0) red[wv][q] = s;
  }
  const int pn = rsx::wave::sum_i32(placed_n), in = rsx::wave::sum_i32(inside_n);
  if (lane == 0) cnt[wv][0] = pn, cnt[wv][1] = in;
  __syncthreads();
  Sums out;
#pragma unroll
  for (int q = 0; q < NS; q++) out.s[q] = (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]);
  out.placed = cnt[0][0] + cnt[1][0] + cnt[2][0] + cnt[3][0];
  out.inside = cnt[0][1] + cnt[1][1] + cnt[2][1] + cnt[3][1];
  __syncthreads();  // (the next evaluation writes the words again)
  return out;
}

// (H + lam diag H) d = g by LDL^T written out; false when a pivot is not > 0 (a NaN fails)
__device__ __forceinline__ bool solve(const double *s, double lam, double *d) {
  const double damp = 1.0 + lam;
  const double a00 = s[5] * damp, a11 = s[8] * damp, a22 = s[10] * damp, a01 = s[6], a02 = s[7], a12 = s[9];
  const double d0 = a00;
  if (!(d0 > 0.0)) return false;
  const double l10 = a01 / d0, l20 = a02 / d0;
  const double d1 = a11 - l10 * a01;
  if (!(d1 > 0.0)) return false;
  const double e = a12 - l20 * a01;
  const double l21 = e / d1;
  const double d2 = (a22 - l20 * a02) - l21 * e;
  if (!(d2 > 0.0)) return false;
  const double z0 = s[2];
  const double z1 = s[3] - l10 * z0;
  const double z2 = (s[4] - l20 * z0) - l21 * z1;
  const double w0 = z0 / d0, w1 = z1 / d1, w2 = z2 / d2;
  d[2] = w2;
  d[1] = w1 - l21 * d[2];
  d[0] = (w0 - l10 * d[1]) - l20 * d[2];
  return true;
}

__device__ __forceinline__ double clamp(double v, double m) {  // two comparisons: a NaN passes through
  v = v > m ? m : v;
  return v < -m ? -m : v;
}

__global__ __launch_bounds__(NT) void gmr_refine(const float *__restrict__ xy, int64_t stride, const int64_t *__restrict__ offsets,
                                                 const double *__restrict__ priors, RefineGeo g, rsx_gridmap_refine_params prm,
                                                 const uint8_t *__restrict__ origin, rsx_gridmap_refine_result *__restrict__ results) {
  __shared__ double red[4][NS];
  __shared__ int cnt[4][2];
  const int tid = threadIdx.x, job = blockIdx.x;
  const double *t = priors + 6 * (int64_t)job;
  int64_t first;
  const int64_t n64 = job_points(offsets, job, &first);
  rsx_gridmap_refine_result r;
  memset(&r, 0, sizeof(r));
  const int skipped = skip_status(t, n64);
  if (skipped) {  // (workgroup-uniform)
    r.status = skipped;
    if (tid == 0) results[job] = r;
    return;
  }
  const int n = (int)n64;
  const float *pts = xy + first * stride;
  double pose[6] = {t[0], t[1], t[2], t[3], t[4], t[5]};
  Sums cur = evaluate(pts, stride, n, pose, g, origin, red, cnt);
  const double cost_initial = cur.s[0], score_initial = cur.s[1];
  int evaluations = 1, accepted = 0, status = RSX_GRIDMAP_REFINE_STATUS_MAX;
  double lam = prm.damping;
  if (score_initial == 0.0) {
    status = RSX_GRIDMAP_MATCH_STATUS_EMPTY;
  } else {
    while (evaluations < prm.max_evaluations) {  // (everything below is the same in every thread)
      double d[3];
      if (!solve(cur.s, lam, d)) {
        status = RSX_GRIDMAP_REFINE_STATUS_SINGULAR;
        break;
      }
      d[0] = clamp(d[0], prm.max_shift_step), d[1] = clamp(d[1], prm.max_shift_step), d[2] = clamp(d[2], prm.max_rotation_step);
      const rsx::mocomp::Poly f = rsx::mocomp::poly(d[2]);
      const double trial[6] = {f.cs * pose[0] - f.sn * pose[3], f.cs * pose[1] - f.sn * pose[4], pose[2] + d[0] * g.res,
                               f.sn * pose[0] + f.cs * pose[3], f.sn * pose[1] + f.cs * pose[4], pose[5] + d[1] * g.res};
      const Sums nxt = evaluate(pts, stride, n, trial, g, origin, red, cnt);
      evaluations++;
      if (nxt.s[0] < cur.s[0]) {
        cur = nxt;
#pragma unroll
        for (int q = 0; q < 6; q++) pose[q] = trial[q];
        accepted++;
        const double tenth = lam / 10.0;
        lam = tenth > LAMBDA_MIN ? tenth : LAMBDA_MIN;
        const double sh = fabs(d[0]) > fabs(d[1]) ? fabs(d[0]) : fabs(d[1]);
        if (sh < prm.shift_tolerance && fabs(d[2]) < prm.rotation_tolerance) {
          status = 0;
          break;
        }
      } else {
        lam = 10.0 * lam;
        if (lam > LAMBDA_MAX) {
          status = 0;
          break;
        }
      }
    }
  }
  if (tid != 0) return;
#pragma unroll
  for (int q = 0; q < 6; q++) r.transform[q] = pose[q], r.hessian[q] = cur.s[5 + q];
  r.cost_initial = cost_initial, r.cost = cur.s[0];
  r.score_initial = score_initial, r.score = cur.s[1];
  r.evaluations = evaluations, r.accepted = accepted;
  r.n_points = cur.placed, r.n_inside = cur.inside;
  r.status = status;
  results[job] = r;
}

int check_params(const rsx_gridmap_refine_params &p) {
  if (!(p.damping > 0.0) || !std::isfinite(p.damping)) return fail(RSX_ERR_BAD_ARG, "damping must be positive and finite");
  if (!(p.max_shift_step > 0.0 && p.max_shift_step <= 8.0)) return fail(RSX_ERR_BAD_ARG, "max_shift_step outside (0, 8]");
  if (!(p.max_rotation_step > 0.0 && p.max_rotation_step <= rsx::mocomp::TH_MAX)) return fail(RSX_ERR_BAD_ARG, "max_rotation_step outside (0, 0.5]");
  if (!(p.shift_tolerance >= 0.0) || !std::isfinite(p.shift_tolerance)) return fail(RSX_ERR_BAD_ARG, "shift_tolerance must be finite and not negative");
  if (!(p.rotation_tolerance >= 0.0) || !std::isfinite(p.rotation_tolerance))
    return fail(RSX_ERR_BAD_ARG, "rotation_tolerance must be finite and not negative");
  if (p.max_evaluations < 1 || p.max_evaluations > 64) return fail(RSX_ERR_BAD_ARG, "max_evaluations %d outside 1 .. 64", p.max_evaluations);
  if (p.reserved != 0) return fail(RSX_ERR_BAD_ARG, "reserved must be 0");
  return RSX_OK;
}

int resolve(const rsx_gridmap_refine_params *params, rsx_gridmap_refine_params &dp) {
  rsx_gridmap_refine_default_params(&dp);
  if (params) dp = *params;
  return check_params(dp);
}

// the call as gridloc_host.h's scaffold takes it: no side output, and the one launch
gridloc::LocCall describe(const rsx_gridmap_refine_params &p) {
  return {gridloc::have_likelihood, 0, nullptr, sizeof(rsx_gridmap_refine_result),
          [&p](rsx_gridmap *h, const gridloc::LocJobs &j, void *d_results, uint32_t *, hipStream_t s) -> int {
            RefineGeo g{};
            g.ox = h->p.origin_x, g.oy = h->p.origin_y, g.res = h->p.resolution, g.inv_res = 1.0 / h->p.resolution;
            g.w = (double)h->p.width, g.h = (double)h->p.height;
            g.x_hi = (double)(h->p.width + PLACE), g.y_hi = (double)(h->p.height + PLACE);
            g.pitch = h->like_pitch();
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
