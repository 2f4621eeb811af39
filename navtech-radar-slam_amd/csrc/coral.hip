// coral.hip -- CorAl alignment quality of a pair of clouds (Adolfsson et al., "CorAl: Introspection for robust radar and lidar
// perception in diverse environments using differential entropy"): merging two aligned clouds does not blur the scene, so the
// differential entropy of a point's neighbourhood in the merged cloud (joint) is about the one in its own cloud (separate);
// quality = mean joint - mean separate entropy, ~0 aligned, growing with misalignment.  It reads no solver's residual, so it
// judges every estimator of the library alike.  CorAl's own code is not part of the reference checkout, so this implements the
// rules written in include/rsx.h as restated in tests/coral_np.py (PARITY UNPINNED); that file is the arithmetic contract.  fp64
// throughout, nothing fused (the library is built with -ffp-contract=off, and this file switches contraction off itself as well).
//
// coral_kernel: one workgroup of 1024 threads per job (min(n_jobs, 256) workgroups, each takes jobs blockIdx.x, + gridDim.x, ...),
// LDS = 64 KiB of keys + 32 KiB cell table + 448 bytes of partial sums.  The neighbour search is cfear_surface_kernel's
// (csrc/cfear_dev.h):
//   1. joint point i (A's point i, or B's point i - n_a moved by T and rounded to float) is written ONCE to the workgroup's
//      128 KiB slot of the handle's workspace; key[i] = cell << 14 | i inside the 128 x 128 grid (i < 16384 = 2 x
//      RSX_CORAL_MAX_POINTS), all ones otherwise -- such a point gets its all-zero record here; padded to a power of two
//   2. bitonic sort of the keys in LDS, then the 16-bit cell table
//   3. lanes take the points in SORTED order, so the lanes of a wavefront sit in the same or adjacent cells and walk nearly the
//      same lists (a cell's points are read through one address by every lane that visits it).  Each lane walks its 3 x 3 block
//      twice in the contract's order: counts and coordinate sums of the joint and the separate set, then -- if scored -- the two
//      covariances.  The points are read from the workspace through the sorted indices: 16384 float2 do not fit beside the keys
//      and the table (128 KiB + 96 KiB > 160 KiB), and one job's slot stays in cache
//   4. the entropies: a lane sums its own points' terms in order, the 64 lanes of a wavefront by the row tree
//      (rsx_wave_dev.h: sum_f64_rows_pair), the 16 wavefronts in order -- fixed, so a job's result does not depend on its place
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <new>

#include "cfear_dev.h"
#include "coral.h"
#include "loopverify.h"
#include "ragged_host.h"
#include "rsx_wave_dev.h"

#pragma STDC FP_CONTRACT OFF

using rsx::fail;

namespace {

constexpr int NT = 1024, NW = NT / 64, MAX_GROUPS = 256;
using namespace rsx::cfear;  // the grid, the keys, the sort and the block walk of cfear_dev.h
constexpr unsigned IDX_BITS = 14;
constexpr int MAX_JOINT = 2 * RSX_CORAL_MAX_POINTS;
static_assert(MAX_JOINT == (1 << IDX_BITS) && NCELL == (1 << IDX_BITS), "a key is cell << 14 | joint index");
static_assert(sizeof(rsx_coral_point) == 24 && sizeof(rsx_coral_result) == 40, "record layouts of include/rsx.h");
constexpr size_t CO_LDS = (size_t)MAX_JOINT * 4 + (size_t)NCELL * 2 + (size_t)NW * 2 * 8 + (size_t)NW * 3 * 4;
constexpr double H_CONST = 2.8378770664093453;  // 1 + log(2 pi), rounded to fp64

struct CoConsts {
  double r, r2, det_min;
  int min_points, min_other;
};

struct CoTransform {
  double r00, r01, tx, r10, r11, ty;
};

// joint point i of a job: A's point i, or B's point i - na through T (one rounding to float per coordinate)
__device__ __forceinline__ float2 joint_point(const float *__restrict__ a, const float *__restrict__ b, int64_t stride, unsigned na, unsigned i,
                                              const CoTransform &T) {
  if (i < na) return make_float2(a[(int64_t)i * stride], a[(int64_t)i * stride + 1]);
  const double bx = (double)b[(int64_t)(i - na) * stride], by = (double)b[(int64_t)(i - na) * stride + 1];
  return make_float2((float)((T.r00 * bx + T.r01 * by) + T.tx), (float)((T.r10 * bx + T.r11 * by) + T.ty));
}

__global__ __launch_bounds__(NT) void coral_kernel(const float *__restrict__ a_xy, const int64_t *__restrict__ a_off, const float *__restrict__ b_xy,
                                                   const int64_t *__restrict__ b_off, int64_t stride, int n_jobs,
                                                   const double *__restrict__ transforms, CoConsts k, float2 *work,
                                                   rsx_coral_result *__restrict__ out, rsx_coral_point *__restrict__ out_points) {
  extern __shared__ __attribute__((aligned(16))) unsigned char co_lds[];
  unsigned *keys = reinterpret_cast<unsigned *>(co_lds);                                     // [<= 16384]
  unsigned short *start = reinterpret_cast<unsigned short *>(co_lds + (size_t)MAX_JOINT * 4);  // [16384]
  double *s_d = reinterpret_cast<double *>(co_lds + (size_t)MAX_JOINT * 4 + (size_t)NCELL * 2);  // [2 NW]
  int *s_i = reinterpret_cast<int *>(s_d + 2 * NW);                                          // [3 NW]
  const int t = threadIdx.x;
  const unsigned lane = t & 63, w = t >> 6;
  float2 *J = work + (size_t)blockIdx.x * MAX_JOINT;  // this workgroup's joint cloud, in joint-index order

  for (int job = blockIdx.x; job < n_jobs; job += gridDim.x) {
    const int64_t ab = a_off[job], na64 = a_off[job + 1] - ab, bb = b_off[job], nb64 = b_off[job + 1] - bb;
    rsx_coral_point *op = out_points ? out_points + (ab + bb) : nullptr;
    if (na64 > RSX_CORAL_MAX_POINTS || nb64 > RSX_CORAL_MAX_POINTS) {  // (uniform) nothing is computed
      if (op)
        for (int64_t i = t; i < (na64 > 0 ? na64 : 0) + (nb64 > 0 ? nb64 : 0); i += NT) op[i] = rsx_coral_point{0.0, 0.0, 0, 0};
      if (t == 0) out[job] = rsx_coral_result{0.0, 0.0, 0.0, 0, 0, 0, RSX_CORAL_STATUS_POINTS};
      continue;
    }
    const unsigned na = na64 > 0 ? (unsigned)na64 : 0u, nb = nb64 > 0 ? (unsigned)nb64 : 0u, n = na + nb;
    unsigned n2 = NT;
    while (n2 < n) n2 <<= 1;
    const float *a = a_xy + ab * stride, *b = b_xy + bb * stride;
    CoTransform T = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0};
    if (transforms) {
      const double *tf = transforms + 6 * (int64_t)job;
      T = CoTransform{tf[0], tf[1], tf[2], tf[3], tf[4], tf[5]};
    }

    int bad = 0, n_valid = 0;
    for (unsigned i = t; i < n2; i += NT) {
      unsigned key = NO_KEY;
      if (i < n) {
        const float2 q = joint_point(a, b, stride, na, i, T);
        J[i] = q;
        const double fx = floor((double)q.x / k.r), fy = floor((double)q.y / k.r);
        if (fx >= -(double)HALF && fx < (double)HALF && fy >= -(double)HALF && fy < (double)HALF) {
          key = ((unsigned)(((int)fy + HALF) * GRID + ((int)fx + HALF)) << IDX_BITS) | i;
          n_valid++;
        } else {
          bad = 1;
          if (op) op[i] = rsx_coral_point{0.0, 0.0, 0, 0};
        }
      }
      keys[i] = key;
    }
    for (int c = t; c < NCELL; c += NT) start[c] = NO_CELL;
    bad = __syncthreads_or(bad);  // (the joint cloud in J is visible to the workgroup from here on)

    bitonic_sort_lds<NT>(keys, n2, t);
    fill_cell_table<NT, IDX_BITS, true>(keys, (int)n, start, t);  // (points outside the grid have no cell)
    __syncthreads();

    double hj = 0.0, hs = 0.0;
    int n_scored = 0, n_scored_a = 0;
    for (unsigned i = t; i < n; i += NT) {
      const unsigned key = keys[i];
      if (key == NO_KEY) continue;
      const unsigned cell = key >> IDX_BITS, me = key & ((1u << IDX_BITS) - 1u);
      const int ix = (int)(cell % GRID), iy = (int)(cell / GRID);
      const bool in_b = me >= na;
      const float2 pf = J[me];
      const double px = (double)pf.x, py = (double)pf.y;
      int mj = 0, ms = 0;
      double jx = 0.0, jy = 0.0, sx = 0.0, sy = 0.0;
      for_block<IDX_BITS>(keys, start, n, ix, iy, [&](unsigned idx) {
        const float2 q = J[idx];
        const double ex = (double)q.x - px, ey = (double)q.y - py;
        if (ex * ex + ey * ey <= k.r2) {
          jx = jx + (double)q.x;
          jy = jy + (double)q.y;
          mj++;
          if ((idx >= na) == in_b) {
            sx = sx + (double)q.x;
            sy = sy + (double)q.y;
            ms++;
          }
        }
      });
      rsx_coral_point rec = {0.0, 0.0, ms, mj};
      if (ms >= k.min_points && mj - ms >= k.min_other) {
        const double mjx = jx / (double)mj, mjy = jy / (double)mj, msx = sx / (double)ms, msy = sy / (double)ms;
        double jxx = 0.0, jyy = 0.0, jxy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
        for_block<IDX_BITS>(keys, start, n, ix, iy, [&](unsigned idx) {
          const float2 q = J[idx];
          const double ex = (double)q.x - px, ey = (double)q.y - py;
          if (ex * ex + ey * ey <= k.r2) {
            const double ux = (double)q.x - mjx, uy = (double)q.y - mjy;
            jxx = jxx + ux * ux;
            jyy = jyy + uy * uy;
            jxy = jxy + ux * uy;
            if ((idx >= na) == in_b) {
              const double vx = (double)q.x - msx, vy = (double)q.y - msy;
              sxx = sxx + vx * vx;
              syy = syy + vy * vy;
              sxy = sxy + vx * vy;
            }
          }
        });
        const double j1 = (double)(mj - 1), s1 = (double)(ms - 1);
        jxx = jxx / j1;
        jyy = jyy / j1;
        jxy = jxy / j1;
        sxx = sxx / s1;
        syy = syy / s1;
        sxy = sxy / s1;
        rec.det_joint = jxx * jyy - jxy * jxy;
        rec.det_separate = sxx * syy - sxy * sxy;
        hj = hj + (0.5 * log(fmax(rec.det_joint, k.det_min)) + H_CONST);
        hs = hs + (0.5 * log(fmax(rec.det_separate, k.det_min)) + H_CONST);
        n_scored++;
        n_scored_a += in_b ? 0 : 1;
      }
      if (op) op[me] = rec;
    }

    // (the whole workgroup is here: the loop above holds no barrier)
    hj = rsx::wave::sum_f64_rows_pair(hj);
    hs = rsx::wave::sum_f64_rows_pair(hs);
    n_valid = rsx::wave::sum_i32(n_valid);
    n_scored = rsx::wave::sum_i32(n_scored);
    n_scored_a = rsx::wave::sum_i32(n_scored_a);
    if (lane == 0) {
      s_d[2 * w] = hj;
      s_d[2 * w + 1] = hs;
      s_i[3 * w] = n_valid;
      s_i[3 * w + 1] = n_scored;
      s_i[3 * w + 2] = n_scored_a;
    }
    __syncthreads();
    if (t == 0) {
      double tj = 0.0, ts = 0.0;
      int v = 0, sc = 0, sa = 0;
      for (int ww = 0; ww < NW; ww++) {
        tj = tj + s_d[2 * ww];
        ts = ts + s_d[2 * ww + 1];
        v += s_i[3 * ww];
        sc += s_i[3 * ww + 1];
        sa += s_i[3 * ww + 2];
      }
      rsx_coral_result r = {0.0, 0.0, 0.0, sc, sa, v, bad ? RSX_CORAL_STATUS_RANGE : 0};
      if (sc == 0) {
        r.status |= RSX_CORAL_STATUS_EMPTY;
      } else {
        r.h_joint = tj / (double)sc;
        r.h_separate = ts / (double)sc;
        r.quality = r.h_joint - r.h_separate;
      }
      out[job] = r;
    }
    __syncthreads();  // (the keys, the table, the partial sums and J are free for the next job)
  }
}

int check_params(const rsx_coral_params &p) {
  if (!(p.radius > 0.0) || !std::isfinite(p.radius)) return fail(RSX_ERR_BAD_ARG, "radius must be positive");
  if (!(p.det_min > 0.0) || !std::isfinite(p.det_min)) return fail(RSX_ERR_BAD_ARG, "det_min must be positive");
  if (p.min_points < 2) return fail(RSX_ERR_BAD_ARG, "min_points %d below 2", p.min_points);
  if (p.min_other < 0) return fail(RSX_ERR_BAD_ARG, "min_other %d below 0", p.min_other);
  return RSX_OK;
}

int resolve(const rsx_coral_params *params, rsx_coral_params &dp) {
  rsx_coral_default_params(&dp);
  if (params) dp = *params;
  return check_params(dp);
}

// the one launch behind every entry (the caller holds h->mu and has entered s); grows the workspace to min(n_jobs, 256) x 128 KiB
int launch(rsx_coral *h, const float *d_a, const int64_t *d_a_off, const float *d_b, const int64_t *d_b_off, int32_t stride, int32_t n_jobs,
           const double *d_transforms, const rsx_coral_params &p, rsx_coral_result *d_out, rsx_coral_point *d_points, hipStream_t s) {
  const int groups = n_jobs < MAX_GROUPS ? n_jobs : MAX_GROUPS;
  RSX_TRY(h->work.reserve((size_t)groups * MAX_JOINT * sizeof(float2), s, false));
  RSX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&coral_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)CO_LDS));
  CoConsts k;
  k.r = p.radius;
  k.r2 = p.radius * p.radius;
  k.det_min = p.det_min;
  k.min_points = p.min_points;
  k.min_other = p.min_other;
  hipLaunchKernelGGL(coral_kernel, dim3((unsigned)groups), dim3(NT), CO_LDS, s, d_a, d_a_off, d_b, d_b_off, (int64_t)stride, (int)n_jobs, d_transforms,
                     k, h->work.as<float2>(), d_out, d_points);
  RSX_HIP(hipGetLastError());
  return RSX_OK;
}

int check_clouds(const int64_t *offsets, int32_t n_jobs, const char *which) {
  for (int32_t i = 0; i < n_jobs; i++)
    if (offsets[i + 1] - offsets[i] > RSX_CORAL_MAX_POINTS)
      return fail(RSX_ERR_BAD_ARG, "cloud %s of job %d has %lld points, more than %d", which, i, (long long)(offsets[i + 1] - offsets[i]),
                  RSX_CORAL_MAX_POINTS);
  return RSX_OK;
}

}  // namespace

extern "C" {

int rsx_coral_default_params(rsx_coral_params *p) try {
  if (!p) return fail(RSX_ERR_BAD_ARG, "null params");
  p->radius = 3.5;
  p->det_min = 1e-6;
  p->min_points = 6;
  p->min_other = 1;
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_coral_create(int device, rsx_coral **out) try {
  if (!out) return fail(RSX_ERR_BAD_ARG, "null out");
  *out = nullptr;
  RSX_TRY(rsx::check_device(device));
  std::unique_ptr<rsx_coral> h(new (std::nothrow) rsx_coral());
  if (!h) return fail(RSX_ERR_OOM, "host alloc");
  h->device = device;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = h->stream.create();
  if (e != hipSuccess) return fail(RSX_ERR_HIP, "create: %s", hipGetErrorString(e));
  *out = h.release();
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_coral_destroy(rsx_coral *h) try {
  if (!h) return RSX_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  delete h;
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_coral_quality_batch_device(rsx_coral *h, const float *d_a, const int64_t *d_a_offsets, const float *d_b, const int64_t *d_b_offsets,
                                   int32_t point_stride, int32_t n_jobs, const double *d_transforms, const rsx_coral_params *params,
                                   rsx_coral_result *d_results, rsx_coral_point *d_points, void *stream) try {
  // (the arguments are judged before the handle is looked at: their rules need no device)
  if (!d_a || !d_a_offsets || !d_b || !d_b_offsets || !d_results || n_jobs < 0) return fail(RSX_ERR_BAD_ARG, "bad arg");
  if (point_stride < 2) return fail(RSX_ERR_BAD_ARG, "point_stride %d below 2", point_stride);
  rsx_coral_params dp;
  RSX_TRY(resolve(params, dp));
  if (!h) return fail(RSX_ERR_BAD_ARG, "null handle");
  if (n_jobs == 0) return RSX_OK;
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
  RSX_TRY(h->order.enter(s));
  return launch(h, d_a, d_a_offsets, d_b, d_b_offsets, point_stride, n_jobs, d_transforms, dp, d_results, d_points, s);
} RSX_CATCH_ALL

int rsx_coral_quality_batch(rsx_coral *h, const float *a_xy, const int64_t *a_offsets, const float *b_xy, const int64_t *b_offsets, int32_t n_jobs,
                            const double *transforms, const rsx_coral_params *params, rsx_coral_result *out_results,
                            rsx_coral_point *out_points) try {
  // (the arguments are judged before the handle is looked at: their rules need no device)
  if (!a_xy || !a_offsets || !b_xy || !b_offsets || !out_results || n_jobs < 0) return fail(RSX_ERR_BAD_ARG, "bad arg");
  rsx_coral_params dp;
  RSX_TRY(resolve(params, dp));
  if (n_jobs > 0) {
    RSX_TRY(rsx::check_offsets(a_offsets, n_jobs, "rsx_coral_quality_batch (a)"));
    RSX_TRY(rsx::check_offsets(b_offsets, n_jobs, "rsx_coral_quality_batch (b)"));
    RSX_TRY(check_clouds(a_offsets, n_jobs, "a"));
    RSX_TRY(check_clouds(b_offsets, n_jobs, "b"));
  }
  if (!h) return fail(RSX_ERR_BAD_ARG, "null handle");
  if (n_jobs == 0) return RSX_OK;
  const size_t ma = (size_t)a_offsets[n_jobs], mb = (size_t)b_offsets[n_jobs], n = (size_t)n_jobs;
  const size_t rb = n * sizeof(rsx_coral_result), pb = (ma + mb) * sizeof(rsx_coral_point);
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  RSX_TRY(h->order.enter(s));
  RSX_TRY(rsx::stage_up(h->a, a_xy, ma * 8, s));
  RSX_TRY(rsx::stage_up(h->a_off, a_offsets, (n + 1) * 8, s));
  RSX_TRY(rsx::stage_up(h->b, b_xy, mb * 8, s));
  RSX_TRY(rsx::stage_up(h->b_off, b_offsets, (n + 1) * 8, s));
  if (transforms) RSX_TRY(rsx::stage_up(h->tf, transforms, n * 48, s));
  RSX_TRY(rsx::stage_room(h->res, rb, s));
  if (out_points) RSX_TRY(rsx::stage_room(h->pts, pb, s));
  RSX_TRY(launch(h, h->a.as<float>(), h->a_off.as<int64_t>(), h->b.as<float>(), h->b_off.as<int64_t>(), 2, n_jobs,
                 transforms ? h->tf.as<double>() : nullptr, dp, h->res.as<rsx_coral_result>(), out_points ? h->pts.as<rsx_coral_point>() : nullptr, s));
  RSX_TRY(rsx::stage_down(out_results, h->res, rb, s));
  if (out_points) RSX_TRY(rsx::stage_down(out_points, h->pts, pb, s));
  RSX_HIP(hipStreamSynchronize(s));
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_kfstore_alignment_quality(rsx_kfstore *kf, rsx_coral *h, int32_t idx_a, int32_t idx_b, const double *transform,
                                  const rsx_coral_params *params, rsx_coral_result *out_result) try {
  if (!out_result) return fail(RSX_ERR_BAD_ARG, "null arg");
  std::memset(out_result, 0, sizeof(*out_result));
  rsx_coral_params dp;
  RSX_TRY(resolve(params, dp));
  if (!kf || !h) return fail(RSX_ERR_BAD_ARG, "null handle");
  if (rsx::kf::device_of(kf) != h->device) return fail(RSX_ERR_BAD_ARG, "the keyframe store and the rsx_coral handle are on different devices");
  std::lock_guard<std::mutex> lkf(rsx::kf::mutex_of(kf));
  const float *d_a = nullptr, *d_b = nullptr;
  int64_t na = 0, nb = 0;
  RSX_TRY(rsx::kf::keyframe_device_locked(kf, idx_a, &d_a, &na));
  RSX_TRY(rsx::kf::keyframe_device_locked(kf, idx_b, &d_b, &nb));
  const int64_t offs[4] = {0, na, 0, nb};
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  RSX_TRY(h->order.enter(s));
  RSX_TRY(rsx::stage_up(h->a_off, offs, sizeof(offs), s));
  if (transform) RSX_TRY(rsx::stage_up(h->tf, transform, 48, s));
  RSX_TRY(rsx::stage_room(h->res, sizeof(rsx_coral_result), s));
  // the clouds are read where the store keeps them: packed float4, x and y first (a keyframe above the cap gets RSX_CORAL_STATUS_POINTS)
  RSX_TRY(launch(h, d_a, h->a_off.as<int64_t>(), d_b, h->a_off.as<int64_t>() + 2, 4, 1, transform ? h->tf.as<double>() : nullptr, dp,
                 h->res.as<rsx_coral_result>(), nullptr, s));
  RSX_TRY(rsx::stage_down(out_result, h->res, sizeof(rsx_coral_result), s));
  RSX_HIP(hipStreamSynchronize(s));
  return RSX_OK;
} RSX_CATCH_ALL

}  // extern "C"
