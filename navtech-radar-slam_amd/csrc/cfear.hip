// cfear.hip -- CFEAR oriented surface points (Adolfsson et al., CFEAR radar odometry): what the k-strongest detector
// (csrc/kstrongest.hip) feeds, and what the point-to-line registration of csrc/cfear_track.hip reads.  CFEAR's own code is not
// part of the reference checkout, so this implements the rules written in include/rsx.h as restated in tests/cfear_np.py
// (PARITY UNPINNED); that file is the arithmetic contract.  fp64 throughout, nothing fused (the library is built with -ffp-contract=off, and this file switches contraction
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
// cfear_surface_kernel<true> (rsx_cfear_surface_points_timed_batch) also gives every record the time it was measured: the owner
//   lane reads the neighbours' azimuth rows in its second walk and takes their circular mean.  cfear_compensate_kernel deskews
//   records with the motion of their scan (csrc/cfear_dev.h: comp_record, on csrc/mocomp_dev.h's polynomials); the contract of both
//   is tests/cfear_mocomp_np.py.
// The registration of surface-point sets is csrc/cfear_track.hip's, the pair entries included; this file keeps the handle and the
// parameter rules they share.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <new>

#include "cfear.h"
#include "cfear_dev.h"
#include "ragged_host.h"

#pragma STDC FP_CONTRACT OFF

using rsx::fail;

namespace {

constexpr int NT = 1024, NW = NT / 64;
using namespace rsx::cfear;  // the grid, the keys and the sort of cfear_dev.h
constexpr unsigned IDX_BITS = 14, IDX_MASK = (1u << IDX_BITS) - 1u;
static_assert(RSX_CFEAR_MAX_POINTS == (1 << IDX_BITS) && NCELL == (1 << IDX_BITS), "a key is cell << 14 | index");
static_assert(sizeof(rsx_cfear_surface_point) == 32 && sizeof(rsx_cfear_result) == 48, "record layouts of include/rsx.h");
constexpr size_t SP_LDS = (size_t)RSX_CFEAR_MAX_POINTS * 4 + (size_t)NCELL * 2 + NW * 4;

struct SpConsts {
  double r, r2, max_condition;
  int min_points, max_records;
};

// TIMED: point i of the scan was measured on azimuth row rows[(begin + i) * row_stride] of n_rows; a record's time, the circular
// mean of its neighbours' rows as a fraction of the revolution, goes to out_tau (laid out like out).  Untimed, the kernel is the
// code it was: everything timed sits behind if constexpr
template <bool TIMED>
__global__ __launch_bounds__(NT) void cfear_surface_kernel(const float2 *__restrict__ xy, const int64_t *__restrict__ begin,
                                                           const int64_t *__restrict__ end, SpConsts k,
                                                           rsx_cfear_surface_point *__restrict__ out, int32_t *__restrict__ counts,
                                                           int32_t *__restrict__ status, const int32_t *__restrict__ rows, int row_stride,
                                                           int n_rows, float *__restrict__ out_tau) {
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

  bitonic_sort_lds<NT>(keys, n2, t);
  fill_cell_table<NT, IDX_BITS, true>(keys, (int)n, start, t);  // (points outside the grid have no cell)
  __syncthreads();

  unsigned run = 0;
  const unsigned lane = t & 63, w = t >> 6;
  for (unsigned base = 0; base < n; base += NT) {
    const unsigned i = base + t;
    bool keep = false;
    rsx_cfear_surface_point rec;
    float tau = 0.f;
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
        for_block<IDX_BITS>(keys, start, n, ix, iy, [&](unsigned idx) {
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
          int a1 = -1, dsum = 0;  // the first neighbour's row; the sum of the others' signed row distances from it (|d| <= 32768,
                                  // m <= 16384: an int holds it)
          for_block<IDX_BITS>(keys, start, n, ix, iy, [&](unsigned idx) {
            const float2 q = p[idx];
            const double ex = (double)q.x - cx, ey = (double)q.y - cy;
            if (ex * ex + ey * ey <= k.r2) {
              const double ux = (double)q.x - mx, uy = (double)q.y - my;
              sxx = sxx + ux * ux;
              syy = syy + uy * uy;
              sxy = sxy + ux * uy;
              if constexpr (TIMED) {
                const int a = rows[(b + (int64_t)idx) * row_stride], half = n_rows / 2;
                if (a1 < 0) a1 = a;
                int d = (a - a1 + half) % n_rows;
                d = d < 0 ? d + n_rows : d;
                dsum += d - half;
              }
            }
          });
          if constexpr (TIMED) {
            double u = ((double)a1 + (double)dsum / (double)m) + 0.5;
            if (u < 0.0)
              u = u + (double)n_rows;
            else if (u >= (double)n_rows)
              u = u - (double)n_rows;
            tau = (float)(u / (double)n_rows);
          }
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
      if (pos < (unsigned)k.max_records) {
        o[pos] = rec;
        if constexpr (TIMED) out_tau[(int64_t)scan * k.max_records + pos] = tau;
      }
    }
    run += total;
    __syncthreads();
  }
  if (t == 0) {
    counts[scan] = (int32_t)run;
    if (status) status[scan] = bad ? RSX_CFEAR_STATUS_RANGE : 0;
  }
}

}  // namespace

int rsx::cfear::check_params(const rsx_cfear_params &p) {
  if (!(p.radius > 0.0) || !std::isfinite(p.radius)) return fail(RSX_ERR_BAD_ARG, "radius must be positive");
  if (!(p.max_condition >= 1.0)) return fail(RSX_ERR_BAD_ARG, "max_condition must be at least 1");
  if (!(p.cos_max_normal_angle >= -1.0 && p.cos_max_normal_angle <= 1.0)) return fail(RSX_ERR_BAD_ARG, "cos_max_normal_angle outside [-1, 1]");
  if (!(p.huber_delta > 0.0) || !std::isfinite(p.huber_delta)) return fail(RSX_ERR_BAD_ARG, "huber_delta must be positive");
  if (!(p.step_epsilon >= 0.0) || !std::isfinite(p.step_epsilon)) return fail(RSX_ERR_BAD_ARG, "step_epsilon must not be negative");
  if (p.min_points < 2) return fail(RSX_ERR_BAD_ARG, "min_points %d below 2", p.min_points);
  if (p.max_iterations < 1 || p.max_iterations > 200) return fail(RSX_ERR_BAD_ARG, "max_iterations %d outside [1, 200]", p.max_iterations);
  if (p.min_correspondences < 1) return fail(RSX_ERR_BAD_ARG, "min_correspondences %d below 1", p.min_correspondences);
  if (p.cost < RSX_CFEAR_COST_P2L || p.cost > RSX_CFEAR_COST_P2D) return fail(RSX_ERR_BAD_ARG, "cost %d is none of RSX_CFEAR_COST_*", p.cost);
  if (p.loss < RSX_CFEAR_LOSS_HUBER || p.loss > RSX_CFEAR_LOSS_NONE) return fail(RSX_ERR_BAD_ARG, "loss %d is none of RSX_CFEAR_LOSS_*", p.loss);
  if (p.weights != 0 && p.weights != 1) return fail(RSX_ERR_BAD_ARG, "weights %d is neither 0 nor 1", p.weights);
  return RSX_OK;
}

namespace {

template <bool TIMED>
int launch_surface_t(const float *d_xy, const int64_t *d_begin, const int64_t *d_end, int32_t n_scans, const rsx_cfear_params &p,
                     rsx_cfear_surface_point *d_out, int32_t max_records, int32_t *d_counts, int32_t *d_status, const int32_t *d_rows,
                     int32_t row_stride, int32_t n_rows, float *d_out_tau, hipStream_t s) {
  if (n_scans < 1) return fail(RSX_ERR_BAD_ARG, "n_scans %d below 1", n_scans);
  if (max_records < 1 || max_records > RSX_CFEAR_MAX_SURFACE_POINTS)
    return fail(RSX_ERR_BAD_ARG, "max_records %d outside [1, %d]", max_records, RSX_CFEAR_MAX_SURFACE_POINTS);
  RSX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&cfear_surface_kernel<TIMED>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)SP_LDS));
  SpConsts k;
  k.r = p.radius;
  k.r2 = p.radius * p.radius;
  k.max_condition = p.max_condition;
  k.min_points = p.min_points;
  k.max_records = max_records;
  hipLaunchKernelGGL(cfear_surface_kernel<TIMED>, dim3((unsigned)n_scans), dim3(NT), SP_LDS, s, reinterpret_cast<const float2 *>(d_xy), d_begin,
                     d_end, k, d_out, d_counts, d_status, d_rows, (int)row_stride, (int)n_rows, d_out_tau);
  RSX_HIP(hipGetLastError());
  return RSX_OK;
}

// cfear_compensate_kernel: one thread per record, CHUNKS workgroups per scan (4096 records a sweep); the scan's motion is read
// through a wave-uniform address.  A record is two 16-byte halves: (x, y, nx, ny), which compensation rewrites, and the rest,
// copied.  No LDS, no barrier; the status word is written by one thread.  out may be the input
constexpr int CNT = 256, CHUNKS = 16;
constexpr int32_t MAX_COMP_SCANS = 0x7fffffff / CHUNKS;

__global__ __launch_bounds__(CNT) void cfear_compensate_kernel(const float4 *rec, const float *__restrict__ tau, const int64_t *__restrict__ offsets,
                                                               const double *__restrict__ motion, float4 *out, int32_t *__restrict__ status) {
  const int scan = blockIdx.x / CHUNKS, chunk = blockIdx.x % CHUNKS;
  const int64_t o = offsets[scan], n = offsets[scan + 1] - o;
  const CompMotion m = comp_motion(motion[3 * (int64_t)scan], motion[3 * (int64_t)scan + 1], motion[3 * (int64_t)scan + 2]);
  if (status && chunk == 0 && threadIdx.x == 0) status[scan] = m.how == 2 ? 1 : 0;
  for (int64_t i = (int64_t)chunk * CNT + threadIdx.x; i < n; i += (int64_t)CHUNKS * CNT) {
    const float4 q = rec[2 * (o + i)], rest = rec[2 * (o + i) + 1];
    out[2 * (o + i)] = m.how == 0 ? comp_record(q, tau[o + i], m) : q;
    out[2 * (o + i) + 1] = rest;
  }
}

int launch_compensate(const rsx_cfear_surface_point *d_rec, const float *d_tau, const int64_t *d_offsets, int32_t n_scans, const double *d_motion,
                      rsx_cfear_surface_point *d_out, int32_t *d_status, hipStream_t s) {
  if (n_scans < 1 || n_scans > MAX_COMP_SCANS) return fail(RSX_ERR_BAD_ARG, "n_scans %d outside [1, %d]", n_scans, MAX_COMP_SCANS);
  hipLaunchKernelGGL(cfear_compensate_kernel, dim3((unsigned)n_scans * CHUNKS), dim3(CNT), 0, s, reinterpret_cast<const float4 *>(d_rec), d_tau,
                     d_offsets, d_motion, reinterpret_cast<float4 *>(d_out), d_status);
  RSX_HIP(hipGetLastError());
  return RSX_OK;
}

int check_n_rows(int32_t n_rows) {
  if (n_rows < 1 || n_rows > 65536) return fail(RSX_ERR_BAD_ARG, "n_rows %d outside [1, 65536]", n_rows);
  return RSX_OK;
}

}  // namespace

int rsx::cfear::launch_surface(const float *d_xy, const int64_t *d_begin, const int64_t *d_end, int32_t n_scans, const rsx_cfear_params &p,
                               rsx_cfear_surface_point *d_out, int32_t max_records, int32_t *d_counts, int32_t *d_status, hipStream_t s) {
  return launch_surface_t<false>(d_xy, d_begin, d_end, n_scans, p, d_out, max_records, d_counts, d_status, nullptr, 1, 1, nullptr, s);
}

int rsx::cfear::launch_surface_timed(const float *d_xy, const int32_t *d_rows, int32_t row_stride, int32_t n_rows, const int64_t *d_begin,
                                     const int64_t *d_end, int32_t n_scans, const rsx_cfear_params &p, rsx_cfear_surface_point *d_out,
                                     float *d_out_tau, int32_t max_records, int32_t *d_counts, int32_t *d_status, hipStream_t s) {
  RSX_TRY(check_n_rows(n_rows));
  return launch_surface_t<true>(d_xy, d_begin, d_end, n_scans, p, d_out, max_records, d_counts, d_status, d_rows, row_stride, n_rows, d_out_tau, s);
}

int rsx::cfear::resolve(const rsx_cfear_params *params, const rsx_cfear_track_params *track, rsx_cfear_params &dp, rsx_cfear_track_params *dt) {
  rsx_cfear_default_params(&dp);
  if (params) dp = *params;
  RSX_TRY(check_params(dp));
  if (!dt) return RSX_OK;
  rsx_cfear_default_track_params(dt);
  if (track) *dt = *track;
  return check_track_params(*dt);
}

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
  p->cost = RSX_CFEAR_COST_P2L;
  p->loss = RSX_CFEAR_LOSS_HUBER;
  p->weights = 0;
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
  RSX_TRY(rsx::cfear::resolve(params, nullptr, dp, nullptr));
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
  RSX_TRY(rsx::cfear::resolve(params, nullptr, dp, nullptr));
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

int rsx_cfear_surface_points_timed_batch_device(rsx_cfear *h, const float *d_xy, const int32_t *d_rows, int32_t n_rows, const int64_t *d_offsets,
                                                int32_t n_scans, const rsx_cfear_params *params, rsx_cfear_surface_point *d_records,
                                                float *d_tau, int32_t max_records, int32_t *d_counts, int32_t *d_status, void *stream) try {
  if (!h || !d_xy || !d_rows || !d_offsets || !d_records || !d_tau || !d_counts || n_scans < 0) return fail(RSX_ERR_BAD_ARG, "bad arg");
  rsx_cfear_params dp;
  RSX_TRY(rsx::cfear::resolve(params, nullptr, dp, nullptr));
  RSX_TRY(check_n_rows(n_rows));
  if (max_records < 1 || max_records > RSX_CFEAR_MAX_SURFACE_POINTS)
    return fail(RSX_ERR_BAD_ARG, "max_records %d outside [1, %d]", max_records, RSX_CFEAR_MAX_SURFACE_POINTS);
  if (n_scans == 0) return RSX_OK;
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
  RSX_TRY(h->order.enter(s));
  return rsx::cfear::launch_surface_timed(d_xy, d_rows, 1, n_rows, d_offsets, d_offsets + 1, n_scans, dp, d_records, d_tau, max_records, d_counts,
                                          d_status, s);
} RSX_CATCH_ALL

int rsx_cfear_surface_points_timed_batch(rsx_cfear *h, const float *xy, const int32_t *rows, int32_t n_rows, const int64_t *offsets, int32_t n_scans,
                                         const rsx_cfear_params *params, rsx_cfear_surface_point *out_records, float *out_tau,
                                         int32_t max_records, int32_t *out_counts, int32_t *out_status) try {
  if (!h || !xy || !rows || !offsets || !out_records || !out_tau || n_scans < 0) return fail(RSX_ERR_BAD_ARG, "bad arg");
  rsx_cfear_params dp;
  RSX_TRY(rsx::cfear::resolve(params, nullptr, dp, nullptr));
  RSX_TRY(check_n_rows(n_rows));
  if (max_records < 1 || max_records > RSX_CFEAR_MAX_SURFACE_POINTS)
    return fail(RSX_ERR_BAD_ARG, "max_records %d outside [1, %d]", max_records, RSX_CFEAR_MAX_SURFACE_POINTS);
  if (n_scans == 0) return RSX_OK;
  RSX_TRY(rsx::check_offsets(offsets, n_scans, "rsx_cfear_surface_points_timed_batch"));
  for (int32_t i = 0; i < n_scans; i++)
    if (offsets[i + 1] - offsets[i] > RSX_CFEAR_MAX_POINTS)
      return fail(RSX_ERR_BAD_ARG, "scan %d has %lld points, more than %d", i, (long long)(offsets[i + 1] - offsets[i]), RSX_CFEAR_MAX_POINTS);
  const size_t m = (size_t)offsets[n_scans], n = (size_t)n_scans, slots = n * (size_t)max_records, ob = slots * sizeof(rsx_cfear_surface_point);
  for (size_t i = 0; i < m; i++)
    if (rows[i] < 0 || rows[i] >= n_rows) return fail(RSX_ERR_BAD_ARG, "rows[%lld] = %d outside [0, %d)", (long long)i, rows[i], n_rows);
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  RSX_TRY(h->order.enter(s));
  RSX_TRY(rsx::stage_up(h->in0, xy, m * 8, s));
  RSX_TRY(rsx::stage_up(h->in1, rows, m * 4, s));
  RSX_TRY(rsx::stage_up(h->off0, offsets, (n + 1) * 8, s));
  RSX_TRY(rsx::stage_room(h->out, ob, s));
  RSX_TRY(rsx::stage_room(h->tau, slots * 4, s));
  RSX_TRY(rsx::stage_room(h->cnt, n * 4, s));
  RSX_TRY(rsx::stage_room(h->st, n * 4, s));
  RSX_HIP(hipMemsetAsync(h->out.p, 0, ob, s));  // (the slots past a scan's count come back as zeros)
  RSX_HIP(hipMemsetAsync(h->tau.p, 0, slots * 4, s));
  RSX_TRY(rsx::cfear::launch_surface_timed(h->in0.as<float>(), h->in1.as<int32_t>(), 1, n_rows, h->off0.as<int64_t>(), h->off0.as<int64_t>() + 1,
                                           n_scans, dp, h->out.as<rsx_cfear_surface_point>(), h->tau.as<float>(), max_records, h->cnt.as<int32_t>(),
                                           h->st.as<int32_t>(), s));
  RSX_TRY(rsx::stage_down(out_records, h->out, ob, s));
  RSX_TRY(rsx::stage_down(out_tau, h->tau, slots * 4, s));
  RSX_TRY(rsx::stage_down(out_counts, h->cnt, n * 4, s));
  RSX_TRY(rsx::stage_down(out_status, h->st, n * 4, s));
  RSX_HIP(hipStreamSynchronize(s));
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_cfear_compensate_batch_device(rsx_cfear *h, const rsx_cfear_surface_point *d_records, const float *d_tau, const int64_t *d_offsets,
                                      int32_t n_scans, const double *d_motion, rsx_cfear_surface_point *d_out_records, int32_t *d_out_status,
                                      void *stream) try {
  if (!h || !d_records || !d_tau || !d_offsets || !d_motion || !d_out_records || n_scans < 0) return fail(RSX_ERR_BAD_ARG, "bad arg");
  if (n_scans == 0) return RSX_OK;
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
  RSX_TRY(h->order.enter(s));
  return launch_compensate(d_records, d_tau, d_offsets, n_scans, d_motion, d_out_records, d_out_status, s);
} RSX_CATCH_ALL

int rsx_cfear_compensate_batch(rsx_cfear *h, const rsx_cfear_surface_point *records, const float *tau, const int64_t *offsets, int32_t n_scans,
                               const double *motion, rsx_cfear_surface_point *out_records, int32_t *out_status) try {
  if (!h || !records || !tau || !offsets || !motion || !out_records || n_scans < 0) return fail(RSX_ERR_BAD_ARG, "bad arg");
  if (n_scans == 0) return RSX_OK;
  RSX_TRY(rsx::check_offsets(offsets, n_scans, "rsx_cfear_compensate_batch"));
  const size_t m = (size_t)offsets[n_scans], n = (size_t)n_scans, rb = m * sizeof(rsx_cfear_surface_point);
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  RSX_TRY(h->order.enter(s));
  RSX_TRY(rsx::stage_up(h->in0, records, rb, s));
  RSX_TRY(rsx::stage_up(h->in1, tau, m * 4, s));
  RSX_TRY(rsx::stage_up(h->off0, offsets, (n + 1) * 8, s));
  RSX_TRY(rsx::stage_up(h->init, motion, n * 24, s));
  RSX_TRY(rsx::stage_room(h->out, rb, s));
  RSX_TRY(rsx::stage_room(h->st, n * 4, s));
  RSX_TRY(launch_compensate(h->in0.as<rsx_cfear_surface_point>(), h->in1.as<float>(), h->off0.as<int64_t>(), n_scans, h->init.as<double>(),
                            h->out.as<rsx_cfear_surface_point>(), h->st.as<int32_t>(), s));
  RSX_TRY(rsx::stage_down(out_records, h->out, rb, s));
  RSX_TRY(rsx::stage_down(out_status, h->st, n * 4, s));
  RSX_HIP(hipStreamSynchronize(s));
  return RSX_OK;
} RSX_CATCH_ALL

}  // extern "C"
