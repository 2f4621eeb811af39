// gridrefine_dev.h -- the device code of the sub-cell refinement that gridrefine.hip (a batch of jobs) and gridtrack.hip (the one-launch
// tracker) share: one evaluation of the rule of include/rsx.h (rsx_gridmap_refine_*) by a workgroup of 256 threads, the 3 x 3 solve, and
// the whole Levenberg-Marquardt loop of a job as refine_record.  fp64 on plain operations, every sum in the stated order: no
// expression here may be fused or re-associated (the Makefile's -ffp-contract=off covers a header too).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "gridmatch_dev.h"
#include "mocomp_dev.h"
#include "rsx.h"
#include "rsx_wave_dev.h"

namespace rsx {
namespace gridrefine_dev {

using gridmatch_dev::NT;
using gridmatch_dev::PLACE;
using gridmatch_dev::skip_status;

constexpr int NS = 11;      // cost, score, g0 g1 g2, H00 H01 H02 H11 H12 H22
constexpr int DEPTH = 4;    // points of a thread whose reads are in flight together
constexpr double LAMBDA_MIN = 1e-9, LAMBDA_MAX = 1e6;
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

// the LDS words of an evaluation's reduction
struct RefineLds {
  double red[4][NS];
  int cnt[4][2];
};

// The record of one job: the n64 points at pts (rows `stride` floats apart) from the prior t.  A skipped job (skip_status) gives a
// zero record but for the status and reads nothing.  Called by the whole workgroup; every thread returns the same record
__device__ __forceinline__ rsx_gridmap_refine_result refine_record(const float *__restrict__ pts, int64_t stride, int64_t n64, const double *t,
                                                                   const RefineGeo &g, const rsx_gridmap_refine_params &prm,
                                                                   const uint8_t *__restrict__ origin, RefineLds *lds) {
  double(*red)[NS] = lds->red;
  int(*cnt)[2] = lds->cnt;
  rsx_gridmap_refine_result r;
  memset(&r, 0, sizeof(r));
  const int skipped = skip_status(t, n64);
  if (skipped) {  // (workgroup-uniform)
    r.status = skipped;
    return r;
  }
  const int n = (int)n64;
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
#pragma unroll
  for (int q = 0; q < 6; q++) r.transform[q] = pose[q], r.hessian[q] = cur.s[5 + q];
  r.cost_initial = cost_initial, r.cost = cur.s[0];
  r.score_initial = score_initial, r.score = cur.s[1];
  r.evaluations = evaluations, r.accepted = accepted;
  r.n_points = cur.placed, r.n_inside = cur.inside;
  r.status = status;
  return r;
}

}  // namespace gridrefine_dev
}  // namespace rsx
