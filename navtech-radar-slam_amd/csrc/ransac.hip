// ransac.hip -- rigid RANSAC and motion-compensated RANSAC (Burnett et al. 2021) on the 2-D matches of a scan pair, the two
// other estimators of the upstream file-based odometry.cpp entry beside ORORA (csrc/orora.hip).  One 256-thread workgroup
// per pair; the matches are streamed from HBM (no limit below rsx_orora_max_correspondences(), nothing in LDS grows with
// K), the H <= 1024 hypotheses' models and their inlier counters live in LDS (36 KB: four workgroups per CU).
//
// The upstream sources (yeti_radar_odometry's Ransac / MotionDistortedRansac, through the reference's ORORA submodule) are
// an empty directory in the reference checkout, so this implements the published methods as restated in
// tests/ransac_np.py (PARITY UNPINNED); that file is the arithmetic contract: every product and sum below stands where it
// stands there (the library is built with -ffp-contract=off), and sums over matches run in the order of its block_sum.
//
//   phase 1   one lane per hypothesis: two sampled matches (counter-based sampler) -> rigid fit, or Gauss-Newton on the
//             body velocity in registers
//   phase 2   each thread holds one match of a 256-match chunk and walks all H models (LDS broadcasts); per hypothesis a
//             wave ballot + popcount goes to its LDS counter
//   phase 3   h_stop (first hypothesis above the inlier ratio) and the winner, two workgroup reductions
//   phase 4   the winner's inlier mask (one bit per match in a 64-bit register: thread t owns matches t, t + 256, ..) and the
//             refit over it: two passes (centroids, cross-covariance) or <= max_gn_iterations passes of 9 sums
// Everything is fp64 VALU work on K x 20 B of input per pair; there is no matrix-shaped part.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <mutex>
#include <new>

#include "ragged_host.h"
#include "ransac.h"
#include "rsx_wave_dev.h"

namespace {

constexpr int NT = 256, NW = NT / 64;
constexpr int MAX_H = 1024;    // hypotheses (rsx_ransac_params.max_iterations)
constexpr int MAX_K = 16384;   // = rsx_orora_max_correspondences(): 64 matches per thread, one mask bit each
constexpr double SERIES_BELOW = 1e-3, SINGULAR_REL = 1e-12;

struct Params {
  double tol2, ratio, gn_eps, dt_scan;
  int H, max_gn;
  uint64_t seed;
};

// splitmix64's output function at state z
__device__ __forceinline__ uint64_t mix(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

struct alignas(32) Model {  // rigid: c, s, tx, ty; MC: vx, vy, wz, void (0 / 1)
  double a, b, c, d;
};

// A = sin th / th, B = (1 - cos th) / th and their derivatives
__device__ __forceinline__ void v_coeffs(double th, double s, double c, double &A, double &B, double &Ap, double &Bp) {
  const double th2 = th * th;
  if (fabs(th) < SERIES_BELOW) {
    A = 1.0 - th2 / 6.0 + th2 * th2 / 120.0;
    B = th / 2.0 - th2 * th / 24.0 + th2 * th2 * th / 720.0;
    Ap = -th / 3.0 + th2 * th / 30.0;
    Bp = 0.5 - th2 / 8.0 + th2 * th2 / 144.0;
  } else {
    A = s / th;
    B = (1.0 - c) / th;
    Ap = (c - A) / th;
    Bp = (s - B) / th;
  }
}

__device__ __forceinline__ double rigid_r2(double px, double py, double qx, double qy, const Model &m) {
  const double ex = qx - ((m.a * px - m.b * py) + m.c);
  const double ey = qy - ((m.b * px + m.a * py) + m.d);
  return ex * ex + ey * ey;
}

__device__ __forceinline__ double mc_r2(double px, double py, double qx, double qy, double dt, double vx, double vy, double wz) {
  const double th = wz * dt;
  double s, c, A, B, Ap, Bp;
  sincos(th, &s, &c);
  v_coeffs(th, s, c, A, B, Ap, Bp);
  const double rx = c * px - s * py, ry = s * px + c * py;
  const double ex = qx - (rx + (A * vx - B * vy) * dt);
  const double ey = qy - (ry + (B * vx + A * vy) * dt);
  return ex * ex + ey * ey;
}

// the 9 terms of one match of the normal equations: a00 a01 a02 a11 a12 a22 g0 g1 g2
__device__ __forceinline__ void mc_normal_terms(double px, double py, double qx, double qy, double dt, double vx, double vy, double wz,
                                                double (&t)[9]) {
  const double th = wz * dt;
  double s, c, A, B, Ap, Bp;
  sincos(th, &s, &c);
  v_coeffs(th, s, c, A, B, Ap, Bp);
  const double rx = c * px - s * py, ry = s * px + c * py;
  const double ex = qx - (rx + (A * vx - B * vy) * dt);
  const double ey = qy - (ry + (B * vx + A * vy) * dt);
  const double j0x = A * dt, j0y = B * dt;
  const double j1x = -B * dt, j1y = A * dt;
  const double j2x = dt * ((-s * px - c * py) + (Ap * vx - Bp * vy) * dt);
  const double j2y = dt * (rx + (Bp * vx + Ap * vy) * dt);
  t[0] = j0x * j0x + j0y * j0y;
  t[1] = j0x * j1x + j0y * j1y;
  t[2] = j0x * j2x + j0y * j2y;
  t[3] = j1x * j1x + j1y * j1y;
  t[4] = j1x * j2x + j1y * j2y;
  t[5] = j2x * j2x + j2y * j2y;
  t[6] = j0x * ex + j0y * ey;
  t[7] = j1x * ex + j1y * ey;
  t[8] = j2x * ex + j2y * ey;
}

// one Gauss-Newton step by Cramer's rule; false: singular system or a step that is not finite
__device__ __forceinline__ bool gn_step(const double (&q)[9], double &d0, double &d1, double &d2) {
  const double a00 = q[0], a01 = q[1], a02 = q[2], a11 = q[3], a12 = q[4], a22 = q[5], g0 = q[6], g1 = q[7], g2 = q[8];
  const double c00 = a11 * a22 - a12 * a12;
  const double c01 = a02 * a12 - a01 * a22;
  const double c02 = a01 * a12 - a02 * a11;
  const double det = a00 * c00 + a01 * c01 + a02 * c02;
  const bool ok = det > SINGULAR_REL * (a00 * a11 * a22);
  const double c11 = a00 * a22 - a02 * a02;
  const double c12 = a01 * a02 - a00 * a12;
  const double c22 = a00 * a11 - a01 * a01;
  d0 = (c00 * g0 + c01 * g1 + c02 * g2) / det;
  d1 = (c01 * g0 + c11 * g1 + c12 * g2) / det;
  d2 = (c02 * g0 + c12 * g1 + c22 * g2) / det;
  return ok && isfinite(d0) && isfinite(d1) && isfinite(d2);
}

// workgroup sums in a fixed order: xor butterfly inside a wave, the waves added in ascending order (buf: N * NW doubles)
template <int N>
__device__ __forceinline__ void block_sum(double (&v)[N], double *buf) {
#pragma unroll
  for (int k = 0; k < N; k++) v[k] = rsx::wave::butterfly(v[k], rsx::wave::Add{});
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < N; k++) buf[k * NW + (threadIdx.x >> 6)] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; k++) {
    double r = buf[k * NW];
#pragma unroll
    for (int w = 1; w < NW; w++) r += buf[k * NW + w];
    v[k] = r;
  }
}

template <bool MAX>
__device__ __forceinline__ int block_minmax(int v, int *buf) {
  v = rsx::wave::butterfly(v, [](int x, int o) { return MAX ? (o > x ? o : x) : (o < x ? o : x); });
  __syncthreads();
  if ((threadIdx.x & 63) == 0) buf[threadIdx.x >> 6] = v;
  __syncthreads();
  int r = buf[0];
#pragma unroll
  for (int w = 1; w < NW; w++) r = MAX ? (buf[w] > r ? buf[w] : r) : (buf[w] < r ? buf[w] : r);
  return r;
}

template <bool MC>
__device__ __forceinline__ void estimate_pair(const float2 *__restrict__ src, const float2 *__restrict__ dst, const float *__restrict__ dt,
                                              const int64_t *__restrict__ offsets, int n_pairs, const Params &p,
                                              rsx_ransac_result *__restrict__ out, uint8_t *__restrict__ out_inlier) {
  __shared__ Model s_model[MAX_H];
  __shared__ int s_cnt[MAX_H];
  __shared__ double s_red[9 * NW];
  __shared__ int s_sel[NW];
  const int pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  if (pair >= n_pairs) return;
  const int64_t o = offsets[pair], K64 = offsets[pair + 1] - o;
  rsx_ransac_result r;
  r.x = r.y = r.yaw = r.vx = r.vy = r.wz = 0.0;
  r.inliers = r.hypotheses = r.gn_iterations = 0;
  r.status = 0;
  if (K64 < 2 || K64 > MAX_K) {
    if (out_inlier)
      for (int64_t i = tid; i < K64; i += NT) out_inlier[o + i] = 0;
    r.status = K64 < 2 ? 1 : 2;
    if (tid == 0) out[pair] = r;
    return;
  }
  const int K = (int)K64, H = p.H;
  const float2 *ps = src + o, *pd = dst + o;
  const float *pt = MC ? dt + o : nullptr;

  // ---- phase 1: the hypotheses' models ----
  for (int h = tid; h < H; h += NT) {
    s_cnt[h] = 0;
    const uint64_t ia = mix(p.seed ^ mix(2ull * (uint64_t)h)) % (uint64_t)K;
    uint64_t ib = mix(p.seed ^ mix(2ull * (uint64_t)h + 1ull)) % (uint64_t)(K - 1);
    ib += ib >= ia ? 1 : 0;
    const double pxa = ps[ia].x, pya = ps[ia].y, qxa = pd[ia].x, qya = pd[ia].y;
    const double pxb = ps[ib].x, pyb = ps[ib].y, qxb = pd[ib].x, qyb = pd[ib].y;
    Model m;
    if constexpr (!MC) {
      const double pbx = (pxa + pxb) / 2.0, pby = (pya + pyb) / 2.0, qbx = (qxa + qxb) / 2.0, qby = (qya + qyb) / 2.0;
      const double axa = pxa - pbx, aya = pya - pby, bxa = qxa - qbx, bya = qya - qby;
      const double axb = pxb - pbx, ayb = pyb - pby, bxb = qxb - qbx, byb = qyb - qby;
      const double C = (axa * bxa + aya * bya) + (axb * bxb + ayb * byb);
      const double S = (axa * bya - aya * bxa) + (axb * byb - ayb * bxb);
      const double nrm = sqrt(C * C + S * S);
      m.a = nrm > 0.0 ? C / nrm : 1.0;
      m.b = nrm > 0.0 ? S / nrm : 0.0;
      m.c = qbx - (m.a * pbx - m.b * pby);
      m.d = qby - (m.b * pbx + m.a * pby);
    } else {
      const double dta = pt[ia], dtb = pt[ib];
      double vx = 0.0, vy = 0.0, wz = 0.0, is_void = 0.0;
      for (int it = 0; it < p.max_gn; it++) {
        double ta[9], tb[9], d0, d1, d2;
        mc_normal_terms(pxa, pya, qxa, qya, dta, vx, vy, wz, ta);
        mc_normal_terms(pxb, pyb, qxb, qyb, dtb, vx, vy, wz, tb);
#pragma unroll
        for (int k = 0; k < 9; k++) ta[k] += tb[k];
        if (!gn_step(ta, d0, d1, d2)) {
          is_void = 1.0;
          break;
        }
        vx += d0;
        vy += d1;
        wz += d2;
        if (sqrt(d0 * d0 + d1 * d1 + d2 * d2) < p.gn_eps) break;
      }
      m.a = vx;
      m.b = vy;
      m.c = wz;
      m.d = is_void;
    }
    s_model[h] = m;
  }
  __syncthreads();

  // ---- phase 2: inlier counts, one match per thread and chunk ----
  for (int base = 0; base < K; base += NT) {
    const int i = base + tid;
    const bool have = i < K;
    double px = 0.0, py = 0.0, qx = 0.0, qy = 0.0, dti = 0.0;
    if (have) {
      px = ps[i].x; py = ps[i].y; qx = pd[i].x; qy = pd[i].y;
      if constexpr (MC) dti = pt[i];
    }
    for (int h = 0; h < H; h++) {
      const Model m = s_model[h];
      bool inl;
      if constexpr (MC) inl = m.d == 0.0 && have && mc_r2(px, py, qx, qy, dti, m.a, m.b, m.c) < p.tol2;
      else inl = have && rigid_r2(px, py, qx, qy, m) < p.tol2;
      const unsigned long long bal = __ballot(inl);
      if (lane == 0 && bal) atomicAdd(&s_cnt[h], (int)__popcll(bal));
    }
  }
  __syncthreads();

  // ---- phase 3: h_stop and the winner (most inliers among h <= h_stop, the lowest h on a tie) ----
  int first = H - 1;
  for (int h = tid; h < H; h += NT)
    if ((double)s_cnt[h] > p.ratio * (double)K && h < first) first = h;
  const int h_stop = block_minmax<false>(first, s_sel);
  int key = -1;
  for (int h = tid; h <= h_stop; h += NT) {
    const int k = (s_cnt[h] << 10) | (MAX_H - 1 - h);
    key = k > key ? k : key;
  }
  key = block_minmax<true>(key, s_sel);
  const int win = MAX_H - 1 - (key & (MAX_H - 1)), wcnt = key >> 10;
  r.hypotheses = h_stop + 1;
  if (wcnt < 2) {
    if (out_inlier)
      for (int i = tid; i < K; i += NT) out_inlier[o + i] = 0;
    r.status = 4;
    if (tid == 0) out[pair] = r;
    return;
  }
  r.inliers = wcnt;

  // ---- phase 4: the winner's inliers (bit j: match tid + j * 256) and the refit over them ----
  const Model wm = s_model[win];
  unsigned long long mask = 0;
  for (int i = tid, j = 0; i < K; i += NT, j++) {
    const double px = ps[i].x, py = ps[i].y, qx = pd[i].x, qy = pd[i].y;
    bool inl;
    if constexpr (MC) inl = mc_r2(px, py, qx, qy, (double)pt[i], wm.a, wm.b, wm.c) < p.tol2;
    else inl = rigid_r2(px, py, qx, qy, wm) < p.tol2;
    if (inl) mask |= 1ull << j;
    if (out_inlier) out_inlier[o + i] = inl ? 1 : 0;
  }
  if constexpr (!MC) {
    const double n = (double)wcnt;
    double sm[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = tid, j = 0; i < K; i += NT, j++)
      if ((mask >> j) & 1ull) {
        sm[0] += (double)ps[i].x; sm[1] += (double)ps[i].y; sm[2] += (double)pd[i].x; sm[3] += (double)pd[i].y;
      }
    block_sum<4>(sm, s_red);
    const double pbx = sm[0] / n, pby = sm[1] / n, qbx = sm[2] / n, qby = sm[3] / n;
    double cs[2] = {0.0, 0.0};
    for (int i = tid, j = 0; i < K; i += NT, j++)
      if ((mask >> j) & 1ull) {
        const double ax = (double)ps[i].x - pbx, ay = (double)ps[i].y - pby, bx = (double)pd[i].x - qbx, by = (double)pd[i].y - qby;
        cs[0] += ax * bx + ay * by;
        cs[1] += ax * by - ay * bx;
      }
    block_sum<2>(cs, s_red);
    const double nrm = sqrt(cs[0] * cs[0] + cs[1] * cs[1]);
    const double c = nrm > 0.0 ? cs[0] / nrm : 1.0, s = nrm > 0.0 ? cs[1] / nrm : 0.0;
    r.x = qbx - (c * pbx - s * pby);
    r.y = qby - (s * pbx + c * pby);
    r.yaw = atan2(s, c);
  } else {
    double vx = wm.a, vy = wm.b, wz = wm.c;
    int it = 0;
    while (it < p.max_gn) {
      double q[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, d0, d1, d2;
      for (int i = tid, j = 0; i < K; i += NT, j++)
        if ((mask >> j) & 1ull) {
          double t[9];
          mc_normal_terms(ps[i].x, ps[i].y, pd[i].x, pd[i].y, (double)pt[i], vx, vy, wz, t);
#pragma unroll
          for (int k = 0; k < 9; k++) q[k] += t[k];
        }
      block_sum<9>(q, s_red);
      if (!gn_step(q, d0, d1, d2)) {  // (workgroup-uniform: every thread holds the same sums) back to the winner's model
        vx = wm.a; vy = wm.b; wz = wm.c;
        it = 0;
        break;
      }
      vx += d0;
      vy += d1;
      wz += d2;
      it++;
      if (sqrt(d0 * d0 + d1 * d1 + d2 * d2) < p.gn_eps) break;
    }
    const double th = wz * p.dt_scan;
    double s, c, A, B, Ap, Bp;
    sincos(th, &s, &c);
    v_coeffs(th, s, c, A, B, Ap, Bp);
    r.x = (A * vx - B * vy) * p.dt_scan;
    r.y = (B * vx + A * vy) * p.dt_scan;
    r.yaw = th;
    r.vx = vx; r.vy = vy; r.wz = wz;
    r.gn_iterations = it;
  }
  if (tid == 0) out[pair] = r;
}

__global__ __launch_bounds__(NT) void ransac_rigid_kernel(const float2 *__restrict__ src, const float2 *__restrict__ dst,
                                                          const int64_t *__restrict__ offsets, int n_pairs, Params p,
                                                          rsx_ransac_result *__restrict__ out, uint8_t *__restrict__ out_inlier) {
  estimate_pair<false>(src, dst, nullptr, offsets, n_pairs, p, out, out_inlier);
}

__global__ __launch_bounds__(NT) void ransac_mc_kernel(const float2 *__restrict__ src, const float2 *__restrict__ dst, const float *__restrict__ dt,
                                                       const int64_t *__restrict__ offsets, int n_pairs, Params p,
                                                       rsx_ransac_result *__restrict__ out, uint8_t *__restrict__ out_inlier) {
  estimate_pair<true>(src, dst, dt, offsets, n_pairs, p, out, out_inlier);
}

// validated arguments -> the launch; touches no state of a handle (the kernels need no workspace)
int launch(const float *d_src, const float *d_dst, const float *d_dt, const int64_t *d_off, int32_t n_pairs, const rsx_ransac_params &dp,
           rsx_ransac_result *d_out, uint8_t *d_inl, hipStream_t s) {
  Params kp;
  kp.tol2 = dp.tolerance * dp.tolerance;
  kp.ratio = dp.inlier_ratio;
  kp.gn_eps = dp.gn_epsilon;
  kp.dt_scan = dp.dt_scan;
  kp.H = dp.max_iterations;
  kp.max_gn = dp.max_gn_iterations;
  kp.seed = dp.seed;
  if (dp.flags & RSX_RANSAC_MOTION_COMPENSATED)
    hipLaunchKernelGGL(ransac_mc_kernel, dim3((unsigned)n_pairs), dim3(NT), 0, s, reinterpret_cast<const float2 *>(d_src),
                       reinterpret_cast<const float2 *>(d_dst), d_dt, d_off, n_pairs, kp, d_out, d_inl);
  else
    hipLaunchKernelGGL(ransac_rigid_kernel, dim3((unsigned)n_pairs), dim3(NT), 0, s, reinterpret_cast<const float2 *>(d_src),
                       reinterpret_cast<const float2 *>(d_dst), d_off, n_pairs, kp, d_out, d_inl);
  RSX_HIP(hipGetLastError());
  return RSX_OK;
}

}  // namespace

static_assert(MAX_H == RSX_RANSAC_MAX_ITERATIONS, "rsx.h");

struct rsx_ransac {
  int device = 0;
  std::mutex mu;
  rsx::Stream stream;
  rsx::DevBuf src, dst, dt, off, res, inl;  // staging of the host-buffer entry
};

using rsx::fail;

int rsx::ransac_check_params(const rsx_ransac_params &p) {
  if (!(p.tolerance > 0.0) || !std::isfinite(p.tolerance)) return fail(RSX_ERR_BAD_ARG, "tolerance must be positive");
  if (!(p.inlier_ratio > 0.0 && p.inlier_ratio <= 1.0)) return fail(RSX_ERR_BAD_ARG, "inlier_ratio outside (0, 1]");
  if (p.max_iterations < 1 || p.max_iterations > RSX_RANSAC_MAX_ITERATIONS)
    return fail(RSX_ERR_BAD_ARG, "max_iterations outside [1, %d]", RSX_RANSAC_MAX_ITERATIONS);
  if (p.flags & ~RSX_RANSAC_MOTION_COMPENSATED) return fail(RSX_ERR_BAD_ARG, "unknown flags");
  if (p.flags & RSX_RANSAC_MOTION_COMPENSATED) {
    if (p.max_gn_iterations < 1 || p.max_gn_iterations > 100) return fail(RSX_ERR_BAD_ARG, "max_gn_iterations outside [1, 100]");
    if (!(p.gn_epsilon >= 0.0)) return fail(RSX_ERR_BAD_ARG, "gn_epsilon must not be negative");
    if (!(p.dt_scan > 0.0) || !std::isfinite(p.dt_scan)) return fail(RSX_ERR_BAD_ARG, "dt_scan must be positive");
  }
  return RSX_OK;
}

namespace {

// the defaults, then the caller's, checked; dt: the per-match times of the call (the motion-compensated estimator needs them)
int resolve_params(const rsx_ransac_params *params, const float *dt, rsx_ransac_params &dp) {
  rsx_ransac_default_params(&dp);
  if (params) dp = *params;
  RSX_TRY(rsx::ransac_check_params(dp));
  if ((dp.flags & RSX_RANSAC_MOTION_COMPENSATED) && !dt) return fail(RSX_ERR_BAD_ARG, "RSX_RANSAC_MOTION_COMPENSATED needs dt");
  return RSX_OK;
}

}  // namespace

extern "C" {

int rsx_ransac_default_params(rsx_ransac_params *p) try {
  if (!p) return fail(RSX_ERR_BAD_ARG, "null params");
  p->tolerance = 0.35;
  p->inlier_ratio = 0.90;
  p->gn_epsilon = 1e-5;
  p->dt_scan = 0.25;
  p->max_iterations = 100;
  p->max_gn_iterations = 10;
  p->seed = 0;
  p->flags = 0;
  p->reserved = 0;
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_ransac_create(int device, rsx_ransac **out) try {
  if (!out) return fail(RSX_ERR_BAD_ARG, "null out");
  *out = nullptr;
  RSX_TRY(rsx::check_device(device));
  std::unique_ptr<rsx_ransac> h(new (std::nothrow) rsx_ransac());
  if (!h) return fail(RSX_ERR_OOM, "host alloc");
  h->device = device;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = h->stream.create();
  if (e != hipSuccess) return fail(RSX_ERR_HIP, "create: %s", hipGetErrorString(e));
  *out = h.release();
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_ransac_destroy(rsx_ransac *h) try {
  if (!h) return RSX_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  delete h;
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_ransac_estimate_batch_device(rsx_ransac *h, const float *d_src_xy, const float *d_dst_xy, const float *d_dt, const int64_t *d_offsets,
                                     int32_t n_pairs, const rsx_ransac_params *params, rsx_ransac_result *d_out, uint8_t *d_out_inlier,
                                     void *stream) try {
  if (!h || !d_src_xy || !d_dst_xy || !d_offsets || !d_out || n_pairs < 0) return fail(RSX_ERR_BAD_ARG, "bad arg");
  rsx_ransac_params dp;
  RSX_TRY(resolve_params(params, d_dt, dp));
  if (n_pairs == 0) return RSX_OK;
  // No rsx::StreamOrder and no lock: the launch reads and writes the caller's buffers only -- the handle has no workspace that
  // calls on different streams could share, so there is nothing to order and they may run side by side
  RSX_HIP(hipSetDevice(h->device));
  return launch(d_src_xy, d_dst_xy, d_dt, d_offsets, n_pairs, dp, d_out, d_out_inlier, stream ? static_cast<hipStream_t>(stream) : h->stream);
} RSX_CATCH_ALL

int rsx_ransac_estimate_batch(rsx_ransac *h, const float *src_xy, const float *dst_xy, const float *dt, const int64_t *offsets, int32_t n_pairs,
                              const rsx_ransac_params *params, rsx_ransac_result *out, uint8_t *out_inlier) try {
  if (!h || !src_xy || !dst_xy || !offsets || !out || n_pairs < 0) return fail(RSX_ERR_BAD_ARG, "bad arg");
  rsx_ransac_params dp;
  RSX_TRY(resolve_params(params, dt, dp));
  if (n_pairs == 0) return RSX_OK;
  RSX_TRY(rsx::check_offsets(offsets, n_pairs, "rsx_ransac_estimate_batch"));
  const bool mc = (dp.flags & RSX_RANSAC_MOTION_COMPENSATED) != 0;
  const size_t m = (size_t)offsets[n_pairs], res_bytes = (size_t)n_pairs * sizeof(rsx_ransac_result);
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  RSX_TRY(rsx::stage_up(h->src, src_xy, m * 8, s));
  RSX_TRY(rsx::stage_up(h->dst, dst_xy, m * 8, s));
  if (mc) RSX_TRY(rsx::stage_up(h->dt, dt, m * 4, s));
  RSX_TRY(rsx::stage_up(h->off, offsets, (size_t)(n_pairs + 1) * 8, s));
  RSX_TRY(rsx::stage_room(h->res, res_bytes, s));
  if (out_inlier) RSX_TRY(rsx::stage_room(h->inl, m, s));
  RSX_TRY(launch(h->src.as<float>(), h->dst.as<float>(), mc ? h->dt.as<float>() : nullptr, h->off.as<int64_t>(), n_pairs, dp,
                 h->res.as<rsx_ransac_result>(), out_inlier ? h->inl.as<uint8_t>() : nullptr, s));
  RSX_TRY(rsx::stage_down(out, h->res, res_bytes, s));
  RSX_TRY(rsx::stage_down(out_inlier, h->inl, m, s));
  RSX_HIP(hipStreamSynchronize(s));
  return RSX_OK;
} RSX_CATCH_ALL

}  // extern "C"
