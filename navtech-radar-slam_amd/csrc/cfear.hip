// cfear.hip -- CFEAR oriented surface points and point-to-line scan registration (Adolfsson et al., CFEAR radar odometry):
// what the k-strongest detector (csrc/kstrongest.hip) feeds.  CFEAR's own code is not part of the reference checkout, so this
// implements the rules written in include/rsx.h as restated in tests/cfear_np.py (PARITY UNPINNED); that file is the arithmetic
// contract.  fp64 throughout, nothing fused (the library is built with -ffp-contract=off, and this file switches contraction
// off itself as well); fp64 add, multiply, divide and sqrt are IEEE on gfx950.
//
// cfear_surface_kernel: one workgroup of 1024 threads per scan, LDS = 64 KiB of keys + 32 KiB cell table.
//   1. key[i] = cell << 14 | i for a point inside the 128 x 128 grid (i < 16384 = RSX_CFEAR_MAX_POINTS, cell < 16384), all ones
//      otherwise; the array is padded to a power of two
//   2. bitonic sort of the keys in LDS: points ordered by cell, inside a cell by input index.  A sort, not atomic counters and a
//      per-cell reorder: its cost is the same for every cloud (all 16384 points in one cell included) and the order needs no
//      second step
//   3. start[cell] = the first sorted position of the cell (16-bit, 0xFFFF = empty): the cell table
//   4. one lane per sorted position that starts a cell -- these are the occupied cells in ascending (iy, ix) -- walks the 3 x 3
//      block twice (count and mean, then the covariance) in the contract's order; the points themselves are read from HBM
//      through the sorted indices (the whole cloud is at most 128 KiB: it stays in cache, and it would not fit beside the keys)
//   5. per 1024 positions the kept cells are compacted in cell order: a ballot per wavefront, the wavefronts' counts scanned
// cfear_register_kernel: one workgroup of 512 threads per pair, LDS = the dst records' x, y, nx, ny (64 KiB at the cap).  The
// src records are strided over the threads (at most 8 each, re-read from cache every iteration).  The correspondence search is
// BRUTE FORCE over the dst records: every lane of a wavefront reads the same LDS address (a broadcast), a tie goes to the
// lowest j by the order of the loop alone, and at the sizes measured so far (600 - 709 records a side) a src record costs 650
// distance tests an iteration.  A search through the dst grid was not built (a record's mean need not lie in the cell that
// produced it: the records would have to be binned again per pair) and neither was measured against the other.  Sums: per
// thread in ascending record index, a butterfly over the lanes of a wavefront, then the 8 wavefront sums in ascending order,
// all fp64; every thread holds the same 3 x 3 system and solves it itself, so the loop needs no host and the branch is uniform.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <new>

#include "cfear.h"
#include "ragged_host.h"

#pragma STDC FP_CONTRACT OFF

namespace {

constexpr int NT = 1024, NW = NT / 64;
constexpr int GRID = 128, HALF = 64, NCELL = GRID * GRID;
constexpr unsigned NO_KEY = 0xFFFFFFFFu, IDX_BITS = 14, IDX_MASK = (1u << IDX_BITS) - 1u;
constexpr unsigned short NO_CELL = 0xFFFF;
static_assert(RSX_CFEAR_MAX_POINTS == (1 << IDX_BITS) && NCELL == (1 << IDX_BITS), "a key is cell << 14 | index");
static_assert(sizeof(rsx_cfear_surface_point) == 32 && sizeof(rsx_cfear_result) == 48, "record layouts of include/rsx.h");
constexpr size_t SP_LDS = (size_t)RSX_CFEAR_MAX_POINTS * 4 + (size_t)NCELL * 2 + NW * 4;
constexpr int N_SUMS = 11;  // H00 H10 H11 H20 H21 H22 g0 g1 g2 cost count
constexpr int RG_NT = 512, RG_NW = RG_NT / 64;  // (the registration kernel: 256 VGPRs a thread, which the fp64 sincos wants)
constexpr size_t RG_LDS = (size_t)RSX_CFEAR_MAX_SURFACE_POINTS * 16 + (size_t)RG_NW * N_SUMS * 8;

struct SpConsts {
  double r, r2, max_condition;
  int min_points, max_records;
};

// f(input index) for every point of the 3 x 3 block of cells around (ix, iy): dy outer, dx inner, ascending index inside a cell
template <typename F>
__device__ __forceinline__ void for_block(const unsigned *keys, const unsigned short *start, unsigned n, int ix, int iy, F &&f) {
  for (int dy = -1; dy <= 1; dy++)
    for (int dx = -1; dx <= 1; dx++) {
      const int jx = ix + dx, jy = iy + dy;
      if (jx < 0 || jx >= GRID || jy < 0 || jy >= GRID) continue;
      const unsigned cc = (unsigned)(jy * GRID + jx);
      unsigned k = start[cc];
      if (k == NO_CELL) continue;
      for (; k < n && (keys[k] >> IDX_BITS) == cc; k++) f(keys[k] & IDX_MASK);
    }
}

__global__ __launch_bounds__(NT) void cfear_surface_kernel(const float2 *__restrict__ xy, const int64_t *__restrict__ begin,
                                                           const int64_t *__restrict__ end, SpConsts k,
                                                           rsx_cfear_surface_point *__restrict__ out, int32_t *__restrict__ counts,
                                                           int32_t *__restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) unsigned char cf_lds[];
  unsigned *keys = reinterpret_cast<unsigned *>(cf_lds);                                             // [<= 16384]
  unsigned short *start = reinterpret_cast<unsigned short *>(cf_lds + (size_t)RSX_CFEAR_MAX_POINTS * 4);  // [16384]
  unsigned *s_w = reinterpret_cast<unsigned *>(cf_lds + (size_t)RSX_CFEAR_MAX_POINTS * 4 + (size_t)NCELL * 2);  // [NW]
  const int scan = blockIdx.x, t = threadIdx.x;
  const int64_t b = begin[scan], n64 = end[scan] - b;
  if (n64 > RSX_CFEAR_MAX_POINTS) {  // (uniform)
    if (t == 0) {
      counts[scan] = 0;
      if (status) status[scan] = RSX_CFEAR_STATUS_POINTS;
    }
    return;
  }
  const unsigned n = n64 > 0 ? (unsigned)n64 : 0u;
  unsigned n2 = NT;
  while (n2 < n) n2 <<= 1;
  const float2 *p = xy + b;
  rsx_cfear_surface_point *o = out + (int64_t)scan * k.max_records;

  int bad = 0;
  for (unsigned i = t; i < n2; i += NT) {
    unsigned key = NO_KEY;
    if (i < n) {
      const float2 q = p[i];
      const double fx = floor((double)q.x / k.r), fy = floor((double)q.y / k.r);
      if (fx >= -(double)HALF && fx < (double)HALF && fy >= -(double)HALF && fy < (double)HALF)
        key = ((unsigned)(((int)fy + HALF) * GRID + ((int)fx + HALF)) << IDX_BITS) | i;
      else
        bad = 1;
    }
    keys[i] = key;
  }
  for (int c = t; c < NCELL; c += NT) start[c] = NO_CELL;
  bad = __syncthreads_or(bad);

  for (unsigned kk = 2; kk <= n2; kk <<= 1)
    for (unsigned j = kk >> 1; j > 0; j >>= 1) {
      for (unsigned i = t; i < n2; i += NT) {
        const unsigned l = i ^ j;
        if (l > i) {
          const unsigned a = keys[i], c = keys[l];
          if ((a > c) == ((i & kk) == 0)) {
            keys[i] = c;
            keys[l] = a;
          }
        }
      }
      __syncthreads();
    }

  for (unsigned i = t; i < n; i += NT) {
    const unsigned key = keys[i];
    if (key != NO_KEY && (i == 0 || (keys[i - 1] >> IDX_BITS) != (key >> IDX_BITS))) start[key >> IDX_BITS] = (unsigned short)i;
  }
  __syncthreads();

  unsigned run = 0;
  const unsigned lane = t & 63, w = t >> 6;
  for (unsigned base = 0; base < n; base += NT) {
    const unsigned i = base + t;
    bool keep = false;
    rsx_cfear_surface_point rec;
    if (i < n) {
      const unsigned key = keys[i];
      if (key != NO_KEY && (i == 0 || (keys[i - 1] >> IDX_BITS) != (key >> IDX_BITS))) {
        const unsigned cell = key >> IDX_BITS;
        const int ix = (int)(cell % GRID), iy = (int)(cell / GRID);
        double sx = 0.0, sy = 0.0;
        unsigned own = 0;
        for (unsigned j = i; j < n && (keys[j] >> IDX_BITS) == cell; j++) {
          const float2 q = p[keys[j] & IDX_MASK];
          sx = sx + (double)q.x;
          sy = sy + (double)q.y;
          own++;
        }
        const double cx = sx / (double)own, cy = sy / (double)own;
        int m = 0;
        sx = sy = 0.0;
        for_block(keys, start, n, ix, iy, [&](unsigned idx) {
          const float2 q = p[idx];
          const double ex = (double)q.x - cx, ey = (double)q.y - cy;
          if (ex * ex + ey * ey <= k.r2) {
            sx = sx + (double)q.x;
            sy = sy + (double)q.y;
            m++;
          }
        });
        if (m >= k.min_points) {
          const double mx = sx / (double)m, my = sy / (double)m;
          double sxx = 0.0, syy = 0.0, sxy = 0.0;
          for_block(keys, start, n, ix, iy, [&](unsigned idx) {
            const float2 q = p[idx];
            const double ex = (double)q.x - cx, ey = (double)q.y - cy;
            if (ex * ex + ey * ey <= k.r2) {
              const double ux = (double)q.x - mx, uy = (double)q.y - my;
              sxx = sxx + ux * ux;
              syy = syy + uy * uy;
              sxy = sxy + ux * uy;
            }
          });
          const double m1 = (double)(m - 1);
          sxx = sxx / m1;
          syy = syy / m1;
          sxy = sxy / m1;
          const double h = (sxx + syy) / 2.0, d = (sxx - syy) / 2.0;
          const double s = sqrt(d * d + sxy * sxy);
          const double lmax = h + s, lmin = h - s;
          if (lmin > 0.0 && lmax <= k.max_condition * lmin) {
            const double a = sxx - lmin, bb = syy - lmin;
            double vx, vy;
            if (a >= bb) {
              vx = sxy;
              vy = -a;
            } else {
              vx = -bb;
              vy = sxy;
            }
            if (vx == 0.0 && vy == 0.0) {
              vx = 1.0;
              vy = 0.0;
            }
            const double nn = sqrt(vx * vx + vy * vy);
            double nx = vx / nn, ny = vy / nn;
            if (nx * mx + ny * my > 0.0) {
              nx = -nx;
              ny = -ny;
            }
            rec.x = (float)mx;
            rec.y = (float)my;
            rec.nx = (float)nx;
            rec.ny = (float)ny;
            rec.lambda_max = (float)lmax;
            rec.lambda_min = (float)lmin;
            rec.n_points = m;
            rec.cell = (int32_t)cell;
            keep = true;
          }
        }
      }
    }
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) s_w[w] = (unsigned)__popcll(bal);
    __syncthreads();
    unsigned before = run, total = 0;
    for (unsigned ww = 0; ww < (unsigned)NW; ww++) {
      if (ww < w) before += s_w[ww];
      total += s_w[ww];
    }
    if (keep) {
      const unsigned pos = before + (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
      if (pos < (unsigned)k.max_records) o[pos] = rec;
    }
    run += total;
    __syncthreads();
  }
  if (t == 0) {
    counts[scan] = (int32_t)run;
    if (status) status[scan] = bad ? RSX_CFEAR_STATUS_RANGE : 0;
  }
}

struct RgConsts {
  double r2, cos_max, delta, step_epsilon;
  int max_iterations, min_correspondences;
};

__global__ __launch_bounds__(RG_NT) void cfear_register_kernel(const rsx_cfear_surface_point *__restrict__ src, const int64_t *__restrict__ src_begin,
                                                            const int64_t *__restrict__ src_end, const rsx_cfear_surface_point *__restrict__ dst,
                                                            const int64_t *__restrict__ dst_begin, const int64_t *__restrict__ dst_end,
                                                            const double *__restrict__ init, RgConsts k, rsx_cfear_result *__restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char cf_lds[];
  float4 *s_dst = reinterpret_cast<float4 *>(cf_lds);                                                          // [<= 4096]
  double *s_red = reinterpret_cast<double *>(cf_lds + (size_t)RSX_CFEAR_MAX_SURFACE_POINTS * 16);  // [RG_NW][N_SUMS]
  const int pair = blockIdx.x, t = threadIdx.x;
  const int64_t sb = src_begin[pair], ns64 = src_end[pair] - sb, db = dst_begin[pair], nd64 = dst_end[pair] - db;
  double x = 0.0, y = 0.0, yaw = 0.0;
  if (init) {
    x = init[3 * (int64_t)pair];
    y = init[3 * (int64_t)pair + 1];
    yaw = init[3 * (int64_t)pair + 2];
  }
  rsx_cfear_result res;
  res.x = x;
  res.y = y;
  res.yaw = yaw;
  res.cost = 0.0;
  res.iterations = res.correspondences = res.status = res.reserved = 0;
  if (ns64 <= 0 || nd64 <= 0 || ns64 > RSX_CFEAR_MAX_SURFACE_POINTS || nd64 > RSX_CFEAR_MAX_SURFACE_POINTS) {  // (uniform)
    res.status = (ns64 <= 0 || nd64 <= 0) ? 1 : 2;
    if (t == 0) out[pair] = res;
    return;
  }
  const int ns = (int)ns64, nd = (int)nd64;
  for (int j = t; j < nd; j += RG_NT) {
    const rsx_cfear_surface_point r = dst[db + j];
    s_dst[j] = make_float4(r.x, r.y, r.nx, r.ny);
  }
  const float4 *sp = reinterpret_cast<const float4 *>(src + sb);  // x, y, nx, ny: the first 16 bytes of a record (2 float4 apart)
  __syncthreads();

  const unsigned lane = t & 63, w = t >> 6;
  int it = 0, status = 0;
  for (;;) {
    double sn, cs;
    sincos(yaw, &sn, &cs);
    double acc[N_SUMS];
#pragma unroll
    for (int a = 0; a < N_SUMS; a++) acc[a] = 0.0;
#pragma unroll 1
    for (int i = t; i < ns; i += RG_NT) {
      const float4 sr = sp[2 * i];
      const double px = (double)sr.x, py = (double)sr.y, pnx = (double)sr.z, pny = (double)sr.w;
      const double qx = (cs * px - sn * py) + x, qy = (sn * px + cs * py) + y;
      const double mx = cs * pnx - sn * pny, my = sn * pnx + cs * pny;
      int best = -1;
      double best_d2 = INFINITY;
#pragma unroll 8
      for (int j = 0; j < nd; j++) {  // (unrolled: the LDS reads of eight records are in flight together; the order of j stays)
        const float4 d = s_dst[j];
        const double ex = qx - (double)d.x, ey = qy - (double)d.y;
        const double d2 = ex * ex + ey * ey;
        const bool ok = (d2 <= k.r2) & (d2 < best_d2) & (mx * (double)d.z + my * (double)d.w >= k.cos_max);
        best = ok ? j : best;
        best_d2 = ok ? d2 : best_d2;
      }
      if (best < 0) continue;
      const float4 d = s_dst[best];
      const double nx = (double)d.z, ny = (double)d.w;
      const double e = nx * (qx - (double)d.x) + ny * (qy - (double)d.y);
      const double ae = fabs(e);
      const double wt = ae <= k.delta ? 1.0 : k.delta / ae;
      const double j0 = nx, j1 = ny, j2 = nx * (-sn * px - cs * py) + ny * (cs * px - sn * py);
      acc[0] += wt * j0 * j0;
      acc[1] += wt * j1 * j0;
      acc[2] += wt * j1 * j1;
      acc[3] += wt * j2 * j0;
      acc[4] += wt * j2 * j1;
      acc[5] += wt * j2 * j2;
      acc[6] += wt * j0 * e;
      acc[7] += wt * j1 * e;
      acc[8] += wt * j2 * e;
      acc[9] += ae <= k.delta ? 0.5 * e * e : k.delta * (ae - 0.5 * k.delta);
      acc[10] += 1.0;
    }
#pragma unroll
    for (int a = 0; a < N_SUMS; a++) {
      double v = acc[a];
      for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
      acc[a] = v;
    }
    if (lane == 0) {
#pragma unroll
      for (int a = 0; a < N_SUMS; a++) s_red[w * N_SUMS + a] = acc[a];
    }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < N_SUMS; a++) {
      double v = 0.0;
      for (int ww = 0; ww < RG_NW; ww++) v += s_red[ww * N_SUMS + a];
      acc[a] = v;
    }
    __syncthreads();  // (s_red is written again in the next iteration)
    // from here on every thread holds the same numbers
    res.cost = acc[9];
    res.correspondences = (int32_t)acc[10];
    if (res.correspondences < k.min_correspondences) {
      status = 4;
      break;
    }
    const double h00 = acc[0], h10 = acc[1], h11 = acc[2], h20 = acc[3], h21 = acc[4], h22 = acc[5];
    const double d0 = h00;
    if (!(d0 > 1e-12 * h00)) {
      status = 5;
      break;
    }
    const double l10 = h10 / d0, l20 = h20 / d0;
    const double d1 = h11 - l10 * h10;
    if (!(d1 > 1e-12 * h11)) {
      status = 5;
      break;
    }
    const double l21 = (h21 - l20 * h10) / d1;
    const double d2 = (h22 - l20 * h20) - l21 * l21 * d1;
    if (!(d2 > 1e-12 * h22)) {
      status = 5;
      break;
    }
    const double z0 = -acc[6];
    const double z1 = -acc[7] - l10 * z0;
    const double z2 = (-acc[8] - l20 * z0) - l21 * z1;
    const double t2 = z2 / d2;
    const double t1 = z1 / d1 - l21 * t2;
    const double t0 = (z0 / d0 - l10 * t1) - l20 * t2;
    x += t0;
    y += t1;
    yaw += t2;
    it++;
    if (sqrt((t0 * t0 + t1 * t1) + t2 * t2) < k.step_epsilon) break;
    if (it >= k.max_iterations) {
      status = 8;
      break;
    }
  }
  if (t == 0) {
    res.x = x;
    res.y = y;
    res.yaw = yaw;
    res.iterations = it;
    res.status = status;
    out[pair] = res;
  }
}

}  // namespace

using rsx::fail;

int rsx::cfear::check_params(const rsx_cfear_params &p) {
  if (!(p.radius > 0.0) || !std::isfinite(p.radius)) return fail(RSX_ERR_BAD_ARG, "radius must be positive");
  if (!(p.max_condition >= 1.0)) return fail(RSX_ERR_BAD_ARG, "max_condition must be at least 1");
  if (!(p.cos_max_normal_angle >= -1.0 && p.cos_max_normal_angle <= 1.0)) return fail(RSX_ERR_BAD_ARG, "cos_max_normal_angle outside [-1, 1]");
  if (!(p.huber_delta > 0.0) || !std::isfinite(p.huber_delta)) return fail(RSX_ERR_BAD_ARG, "huber_delta must be positive");
  if (!(p.step_epsilon >= 0.0) || !std::isfinite(p.step_epsilon)) return fail(RSX_ERR_BAD_ARG, "step_epsilon must not be negative");
  if (p.min_points < 2) return fail(RSX_ERR_BAD_ARG, "min_points %d below 2", p.min_points);
  if (p.max_iterations < 1 || p.max_iterations > 200) return fail(RSX_ERR_BAD_ARG, "max_iterations %d outside [1, 200]", p.max_iterations);
  if (p.min_correspondences < 1) return fail(RSX_ERR_BAD_ARG, "min_correspondences %d below 1", p.min_correspondences);
  return RSX_OK;
}

int rsx::cfear::launch_surface(const float *d_xy, const int64_t *d_begin, const int64_t *d_end, int32_t n_scans, const rsx_cfear_params &p,
                               rsx_cfear_surface_point *d_out, int32_t max_records, int32_t *d_counts, int32_t *d_status, hipStream_t s) {
  if (n_scans < 1) return fail(RSX_ERR_BAD_ARG, "n_scans %d below 1", n_scans);
  if (max_records < 1 || max_records > RSX_CFEAR_MAX_SURFACE_POINTS)
    return fail(RSX_ERR_BAD_ARG, "max_records %d outside [1, %d]", max_records, RSX_CFEAR_MAX_SURFACE_POINTS);
  RSX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&cfear_surface_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)SP_LDS));
  SpConsts k;
  k.r = p.radius;
  k.r2 = p.radius * p.radius;
  k.max_condition = p.max_condition;
  k.min_points = p.min_points;
  k.max_records = max_records;
  hipLaunchKernelGGL(cfear_surface_kernel, dim3((unsigned)n_scans), dim3(NT), SP_LDS, s, reinterpret_cast<const float2 *>(d_xy), d_begin, d_end, k,
                     d_out, d_counts, d_status);
  RSX_HIP(hipGetLastError());
  return RSX_OK;
}

int rsx::cfear::launch_register(const rsx_cfear_surface_point *d_src, const int64_t *d_src_begin, const int64_t *d_src_end,
                                const rsx_cfear_surface_point *d_dst, const int64_t *d_dst_begin, const int64_t *d_dst_end, int32_t n_pairs,
                                const double *d_init, const rsx_cfear_params &p, rsx_cfear_result *d_out, hipStream_t s) {
  if (n_pairs < 1) return fail(RSX_ERR_BAD_ARG, "n_pairs %d below 1", n_pairs);
  RSX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&cfear_register_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)RG_LDS));
  RgConsts k;
  k.r2 = p.radius * p.radius;
  k.cos_max = p.cos_max_normal_angle;
  k.delta = p.huber_delta;
  k.step_epsilon = p.step_epsilon;
  k.max_iterations = p.max_iterations;
  k.min_correspondences = p.min_correspondences;
  hipLaunchKernelGGL(cfear_register_kernel, dim3((unsigned)n_pairs), dim3(RG_NT), RG_LDS, s, d_src, d_src_begin, d_src_end, d_dst, d_dst_begin,
                     d_dst_end, d_init, k, d_out);
  RSX_HIP(hipGetLastError());
  return RSX_OK;
}

namespace {

int resolve_params(const rsx_cfear_params *params, rsx_cfear_params &dp) {
  rsx_cfear_default_params(&dp);
  if (params) dp = *params;
  return rsx::cfear::check_params(dp);
}

}  // namespace

extern "C" {

int rsx_cfear_default_params(rsx_cfear_params *p) try {
  if (!p) return fail(RSX_ERR_BAD_ARG, "null params");
  p->radius = 3.5;
  p->max_condition = 1e5;
  p->cos_max_normal_angle = 0.8660254037844387;  // cos 30 deg
  p->huber_delta = 0.1;
  p->step_epsilon = 1e-6;
  p->min_points = 6;
  p->max_iterations = 50;
  p->min_correspondences = 6;
  p->reserved[0] = p->reserved[1] = p->reserved[2] = 0;
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_cfear_create(int device, rsx_cfear **out) try {
  if (!out) return fail(RSX_ERR_BAD_ARG, "null out");
  *out = nullptr;
  RSX_TRY(rsx::check_device(device));
  std::unique_ptr<rsx_cfear> h(new (std::nothrow) rsx_cfear());
  if (!h) return fail(RSX_ERR_OOM, "host alloc");
  h->device = device;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = h->stream.create();
  if (e != hipSuccess) return fail(RSX_ERR_HIP, "create: %s", hipGetErrorString(e));
  *out = h.release();
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_cfear_destroy(rsx_cfear *h) try {
  if (!h) return RSX_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  delete h;
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_cfear_surface_points_batch_device(rsx_cfear *h, const float *d_xy, const int64_t *d_offsets, int32_t n_scans,
                                          const rsx_cfear_params *params, rsx_cfear_surface_point *d_records, int32_t max_records,
                                          int32_t *d_counts, int32_t *d_status, void *stream) try {
  if (!h || !d_xy || !d_offsets || !d_records || !d_counts || n_scans < 0) return fail(RSX_ERR_BAD_ARG, "bad arg");
  rsx_cfear_params dp;
  RSX_TRY(resolve_params(params, dp));
  if (max_records < 1 || max_records > RSX_CFEAR_MAX_SURFACE_POINTS)
    return fail(RSX_ERR_BAD_ARG, "max_records %d outside [1, %d]", max_records, RSX_CFEAR_MAX_SURFACE_POINTS);
  if (n_scans == 0) return RSX_OK;
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
  RSX_TRY(h->order.enter(s));
  return rsx::cfear::launch_surface(d_xy, d_offsets, d_offsets + 1, n_scans, dp, d_records, max_records, d_counts, d_status, s);
} RSX_CATCH_ALL

int rsx_cfear_surface_points_batch(rsx_cfear *h, const float *xy, const int64_t *offsets, int32_t n_scans, const rsx_cfear_params *params,
                                   rsx_cfear_surface_point *out_records, int32_t max_records, int32_t *out_counts, int32_t *out_status) try {
  if (!h || !xy || !offsets || !out_records || n_scans < 0) return fail(RSX_ERR_BAD_ARG, "bad arg");
  rsx_cfear_params dp;
  RSX_TRY(resolve_params(params, dp));
  if (max_records < 1 || max_records > RSX_CFEAR_MAX_SURFACE_POINTS)
    return fail(RSX_ERR_BAD_ARG, "max_records %d outside [1, %d]", max_records, RSX_CFEAR_MAX_SURFACE_POINTS);
  if (n_scans == 0) return RSX_OK;
  RSX_TRY(rsx::check_offsets(offsets, n_scans, "rsx_cfear_surface_points_batch"));
  for (int32_t i = 0; i < n_scans; i++)
    if (offsets[i + 1] - offsets[i] > RSX_CFEAR_MAX_POINTS)
      return fail(RSX_ERR_BAD_ARG, "scan %d has %lld points, more than %d", i, (long long)(offsets[i + 1] - offsets[i]), RSX_CFEAR_MAX_POINTS);
  const size_t m = (size_t)offsets[n_scans], n = (size_t)n_scans, ob = n * (size_t)max_records * sizeof(rsx_cfear_surface_point);
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  RSX_TRY(h->order.enter(s));
  RSX_TRY(rsx::stage_up(h->in0, xy, m * 8, s));
  RSX_TRY(rsx::stage_up(h->off0, offsets, (n + 1) * 8, s));
  RSX_TRY(rsx::stage_room(h->out, ob, s));
  RSX_TRY(rsx::stage_room(h->cnt, n * 4, s));
  RSX_TRY(rsx::stage_room(h->st, n * 4, s));
  RSX_HIP(hipMemsetAsync(h->out.p, 0, ob, s));  // (the slots past a scan's count come back as zeros)
  RSX_TRY(rsx::cfear::launch_surface(h->in0.as<float>(), h->off0.as<int64_t>(), h->off0.as<int64_t>() + 1, n_scans, dp,
                                     h->out.as<rsx_cfear_surface_point>(), max_records, h->cnt.as<int32_t>(), h->st.as<int32_t>(), s));
  RSX_TRY(rsx::stage_down(out_records, h->out, ob, s));
  RSX_TRY(rsx::stage_down(out_counts, h->cnt, n * 4, s));
  RSX_TRY(rsx::stage_down(out_status, h->st, n * 4, s));
  RSX_HIP(hipStreamSynchronize(s));
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_cfear_register_batch_device(rsx_cfear *h, const rsx_cfear_surface_point *d_src, const int64_t *d_src_offsets,
                                    const rsx_cfear_surface_point *d_dst, const int64_t *d_dst_offsets, int32_t n_pairs,
                                    const double *d_init, const rsx_cfear_params *params, rsx_cfear_result *d_out, void *stream) try {
  if (!h || !d_src || !d_src_offsets || !d_dst || !d_dst_offsets || !d_out || n_pairs < 0) return fail(RSX_ERR_BAD_ARG, "bad arg");
  rsx_cfear_params dp;
  RSX_TRY(resolve_params(params, dp));
  if (n_pairs == 0) return RSX_OK;
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
  RSX_TRY(h->order.enter(s));
  return rsx::cfear::launch_register(d_src, d_src_offsets, d_src_offsets + 1, d_dst, d_dst_offsets, d_dst_offsets + 1, n_pairs, d_init, dp, d_out,
                                     s);
} RSX_CATCH_ALL

int rsx_cfear_register_batch(rsx_cfear *h, const rsx_cfear_surface_point *src, const int64_t *src_offsets,
                             const rsx_cfear_surface_point *dst, const int64_t *dst_offsets, int32_t n_pairs, const double *init,
                             const rsx_cfear_params *params, rsx_cfear_result *out) try {
  if (!h || !src || !src_offsets || !dst || !dst_offsets || !out || n_pairs < 0) return fail(RSX_ERR_BAD_ARG, "bad arg");
  rsx_cfear_params dp;
  RSX_TRY(resolve_params(params, dp));
  if (n_pairs == 0) return RSX_OK;
  RSX_TRY(rsx::check_offsets(src_offsets, n_pairs, "rsx_cfear_register_batch (src)"));
  RSX_TRY(rsx::check_offsets(dst_offsets, n_pairs, "rsx_cfear_register_batch (dst)"));
  const size_t ms = (size_t)src_offsets[n_pairs], md = (size_t)dst_offsets[n_pairs], n = (size_t)n_pairs;
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  RSX_TRY(h->order.enter(s));
  RSX_TRY(rsx::stage_up(h->in0, src, ms * sizeof(rsx_cfear_surface_point), s));
  RSX_TRY(rsx::stage_up(h->in1, dst, md * sizeof(rsx_cfear_surface_point), s));
  RSX_TRY(rsx::stage_up(h->off0, src_offsets, (n + 1) * 8, s));
  RSX_TRY(rsx::stage_up(h->off1, dst_offsets, (n + 1) * 8, s));
  if (init) RSX_TRY(rsx::stage_up(h->init, init, n * 24, s));
  RSX_TRY(rsx::stage_room(h->out, n * sizeof(rsx_cfear_result), s));
  RSX_TRY(rsx::cfear::launch_register(h->in0.as<rsx_cfear_surface_point>(), h->off0.as<int64_t>(), h->off0.as<int64_t>() + 1,
                                      h->in1.as<rsx_cfear_surface_point>(), h->off1.as<int64_t>(), h->off1.as<int64_t>() + 1, n_pairs,
                                      init ? h->init.as<double>() : nullptr, dp, h->out.as<rsx_cfear_result>(), s));
  RSX_TRY(rsx::stage_down(out, h->out, n * sizeof(rsx_cfear_result), s));
  RSX_HIP(hipStreamSynchronize(s));
  return RSX_OK;
} RSX_CATCH_ALL

}  // extern "C"
