// gridmap.hip -- the radar grid map on gfx950: polar scans at known poses accumulated into three integer planes (sum of the
// samples, observations, hits) of a fixed, georeferenced cell grid; rendered as the radar mosaic (mean power) or as an
// occupancy-style hit ratio.  None of this is in the reference checkout: the rule is the one stated in include/rsx.h and restated in
// tests/gridmap_np.py (PARITY UNPINNED), fp64 on plain operations and integers in the planes, so the map is the restatement's byte
// for byte and does not depend on the order of the scans or on how a sequence is cut into batches.
//
// Owner-computes, no atomics, ONE launch per call whatever the batch size: the map is cut into 32 x 32 tiles, one workgroup per
// tile, thread t owns cells 4 (t % 8) .. 4 (t % 8) + 3 of row t / 8 of its tile and keeps their twelve accumulators in registers
// over the whole batch.
//   head   per 1024 scans of the batch: thread t tests scans t, t + 256, ... against the tile (circle against the box of the
//          tile's cell centres, fp64, with a relative margin of 1e-6 on the squared radii: conservative) and lists the ones that
//          meet it in LDS; a scan with a non-finite transform is never listed (workgroup 0 writes the per-scan status words)
//   body   per listed scan (workgroup-uniform: the transform comes through scalar loads), per owned cell: the cell centre into the
//          sensor frame, the range bin from an fp32 square root corrected by stepping until (j rr)^2 <= d2 < ((j + 1) rr)^2 holds,
//          the azimuth row from a polynomial fp32 arc tangent corrected by stepping to a neighbour while one has the larger dot product (the
//          direction table sits in LDS as the fp32 values it was rounded to and is widened where used; a tie goes to the smallest
//          row, as np.argmax); then, for the four cells together so that their loads are in flight at once, the maximum of the
//          2 halfwidth + 1 bytes around (row, bin): neighbouring cells read neighbouring bytes, the gather is served by L2
//   tail   a tile that met a scan reads, adds to and writes its planes once, 16 bytes per thread and plane
// The guesses never show in the result: both are confirmed by the comparisons of the rule.  Where the stepping could be misled
// (d2 below 1e-200: the dot products underflow) every row is compared.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <mutex>
#include <new>
#include <vector>

#include "gridmap.h"
#include "keypoints_host.h"

#pragma STDC FP_CONTRACT OFF

namespace {

constexpr int MAX_COLS = 8192, MAX_ROWS = 4096, MAX_SIDE = 8192;
constexpr int TILE = 32, THREADS = 256, CELLS = 4;  // 32 x 32 cells, 8 threads x 4 cells across, 32 rows
constexpr int LIST = 1024;                          // scans tested and listed at a time
constexpr int GATHER = 9;                           // bytes of a sample loaded without a loop: range_halfwidth 4, the default
constexpr int MAX_IMAGES = 1 << 24;

using Geometry = rsx::GridmapGeometry;

__device__ __forceinline__ bool finite6(const double *t) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 6; k++) ok = ok && ((__double_as_longlong(t[k]) & 0x7ff0000000000000ll) != 0x7ff0000000000000ll);
  return ok;
}

__device__ __forceinline__ double dot_row(const float2 *dir, int a, double px, double py) {
  const float2 t = dir[a];
  return (double)t.x * px + (double)t.y * py;
}

// atan2(y, x) within 1e-3 rad, in (-pi, pi]: an odd polynomial on min / max of |x|, |y|.  Only ever a guess
__device__ __forceinline__ float guess_angle(float x, float y) {
  const float ax = fabsf(x), ay = fabsf(y);
  const float hi = fmaxf(ax, ay), lo = fminf(ax, ay);
  if (!(hi > 0.0f) || !(hi < 3.0e38f)) return 0.0f;  // (0 / 0, inf / inf)
  const float q = lo * __builtin_amdgcn_rcpf(hi), s = q * q;
  float r = ((-0.0464964749f * s + 0.15931422f) * s - 0.327622764f) * s * q + q;
  r = ay > ax ? 1.57079637f - r : r;
  r = x < 0.0f ? 3.14159274f - r : r;
  return y < 0.0f ? -r : r;
}

// steps 4 - 6 of the rule for one cell: false when the cell is not observed, else its range bin and azimuth row.  The guesses
// (fp32 square root and arc tangent) are confirmed by the rule's own comparisons
__device__ __forceinline__ bool locate(const float2 *dir, const Geometry &g, double px, double py, int *bin, int *row) {
  const int rows = g.rows, cols = g.cols;
  const double d2 = px * px + py * py;
  if (!(d2 < g.e_hi) || d2 > g.max2) return false;  // (a NaN observes nothing)
  // ---- the range bin: (j rr)^2 <= d2 < ((j + 1) rr)^2 ----
  int j = (int)fminf(__builtin_amdgcn_sqrtf((float)d2) * g.inv_rr, (float)(cols - 1));  // (a guess: the approximate instruction will do)
  for (;;) {
    const double e = (double)j * g.rr;
    if (j > 0 && e * e > d2) j--;
    else break;
  }
  for (;;) {  // (d2 < e_hi: stops at cols - 1 at the latest)
    const double e = (double)(j + 1) * g.rr;
    if (j + 1 < cols && e * e <= d2) j++;
    else break;
  }
  if (j < g.lo_bin) return false;
  // ---- the azimuth row: the largest c[a] px + s[a] py, the smallest a among equals ----
  int a = 0;
  if (d2 < 1e-200) {
    double f = dot_row(dir, 0, px, py);
    for (int b = 1; b < rows; b++) {
      const double fb = dot_row(dir, b, px, py);
      if (fb > f) f = fb, a = b;
    }
  } else {
    a = (int)rintf(guess_angle((float)px, (float)py) * g.rows_per_rad);
    a = a < 0 ? a + rows : a;
    a = a >= rows ? a - rows : a;
    a = a < 0 ? 0 : (a >= rows ? rows - 1 : a);
    double f = dot_row(dir, a, px, py);
    for (;;) {
      const int an = a + 1 == rows ? 0 : a + 1, ap = a == 0 ? rows - 1 : a - 1;
      const double fn = dot_row(dir, an, px, py), fp = dot_row(dir, ap, px, py);
      if (fn > f && fn >= fp) {
        a = an, f = fn;
      } else if (fp > f) {
        a = ap, f = fp;
      } else {
        int best = a;
        if (fn == f && an < best) best = an;
        if (fp == f && ap < best) best = ap;
        a = best;
        break;
      }
    }
  }
  *bin = j;
  *row = a;
  return true;
}

__global__ __launch_bounds__(THREADS) void gm_add(const uint8_t *__restrict__ imgs, int64_t img_stride, int n_images, int stride, int off,
                                                  const double *__restrict__ transforms, const float2 *__restrict__ table, Geometry g,
                                                  unsigned *__restrict__ p_sum, unsigned *__restrict__ p_cnt, unsigned *__restrict__ p_hit,
                                                  int *__restrict__ status) {
  extern __shared__ float2 dir[];  // [rows]: cos, sin of 2 pi a / rows
  __shared__ uint16_t list[LIST];
  __shared__ unsigned n_list;
  const int tid = threadIdx.x;
  for (int a = tid; a < g.rows; a += THREADS) dir[a] = table[a];
  if (status && blockIdx.x == 0 && blockIdx.y == 0)
    for (int s = tid; s < n_images; s += THREADS) status[s] = finite6(transforms + 6 * (int64_t)s) ? 0 : RSX_GRIDMAP_STATUS_TRANSFORM;
  const int cx0 = (int)blockIdx.x * TILE, cy0 = (int)blockIdx.y * TILE;
  // the box of the tile's cell centres
  const double bx0 = g.ox + ((double)cx0 + 0.5) * g.res, bx1 = g.ox + ((double)(cx0 + TILE - 1) + 0.5) * g.res;
  const double by0 = g.oy + ((double)cy0 + 0.5) * g.res, by1 = g.oy + ((double)(cy0 + TILE - 1) + 0.5) * g.res;
  const int ix0 = cx0 + (tid & 7) * CELLS, iy = cy0 + (tid >> 3);
  double mx[CELLS];
#pragma unroll
  for (int c = 0; c < CELLS; c++) mx[c] = g.ox + ((double)(ix0 + c) + 0.5) * g.res;
  const double my = g.oy + ((double)iy + 0.5) * g.res;
  unsigned a_sum[CELLS] = {0u, 0u, 0u, 0u}, a_cnt[CELLS] = {0u, 0u, 0u, 0u}, a_hit[CELLS] = {0u, 0u, 0u, 0u};
  const int cols = g.cols;

  for (int base = 0; base < n_images; base += LIST) {
    __syncthreads();  // (the table; the previous list has been read)
    if (tid == 0) n_list = 0u;
    __syncthreads();
    const int end = n_images - base < LIST ? n_images : base + LIST;
    for (int s = base + tid; s < end; s += THREADS) {
      const double *t = transforms + 6 * (int64_t)s;
      if (!finite6(t)) continue;
      const double tx = t[2], ty = t[5];
      const double nx = fmax(fmax(bx0 - tx, tx - bx1), 0.0), ny = fmax(fmax(by0 - ty, ty - by1), 0.0);
      const double fx = fmax(fabs(tx - bx0), fabs(tx - bx1)), fy = fmax(fabs(ty - by0), fabs(ty - by1));
      if (nx * nx + ny * ny <= g.reach2 && fx * fx + fy * fy >= g.hole2) list[atomicAdd(&n_list, 1u)] = (uint16_t)(s - base);
    }
    __syncthreads();
    const int nl = (int)n_list;
    for (int k = 0; k < nl; k++) {
      const int s = base + __builtin_amdgcn_readfirstlane((int)list[k]);
      const double *t = transforms + 6 * (int64_t)s;
      const double r00 = t[0], r01 = t[1], tx = t[2], r10 = t[3], r11 = t[4], ty = t[5];
      const uint8_t *img = imgs + (int64_t)s * img_stride + off;
      const double dy = my - ty;
      // ---- where every owned cell falls: bin and row, or not observed ----
      const uint8_t *row[CELLS];
      int b0[CELLS], b1[CELLS];
      bool seen[CELLS];
#pragma unroll
      for (int c = 0; c < CELLS; c++) {
        const double dx = mx[c] - tx;
        const double px = r00 * dx + r10 * dy;
        const double py = r01 * dx + r11 * dy;
        int jj = 0, aa = 0;
        seen[c] = locate(dir, g, px, py, &jj, &aa);
        // the sample's bins j - hw .. j + hw inside [lo_bin, cols - 1]; a cell that is not observed reads the image's first sample
        row[c] = img + (seen[c] ? (int64_t)aa * stride : 0);
        b0[c] = seen[c] ? (jj - g.hw > g.lo_bin ? jj - g.hw : g.lo_bin) : 0;
        b1[c] = seen[c] ? (jj + g.hw < cols - 1 ? jj + g.hw : cols - 1) : 0;
      }
      // ---- the samples: GATHER bytes of every cell in flight at once (a bin past the last repeats the last: the maximum is the same) ----
      unsigned v[CELLS];
#pragma unroll
      for (int c = 0; c < CELLS; c++) {
        unsigned q[GATHER];
#pragma unroll
        for (int u = 0; u < GATHER; u++) q[u] = row[c][b0[c] + u < b1[c] ? b0[c] + u : b1[c]];
        v[c] = q[0];
#pragma unroll
        for (int u = 1; u < GATHER; u++) v[c] = q[u] > v[c] ? q[u] : v[c];
      }
#pragma unroll
      for (int c = 0; c < CELLS; c++) {
        for (int b = b0[c] + GATHER; b <= b1[c]; b++) {  // (range_halfwidth above 4)
          const unsigned q = row[c][b];
          v[c] = q > v[c] ? q : v[c];
        }
        a_cnt[c] += seen[c] ? 1u : 0u;
        a_sum[c] += seen[c] ? v[c] : 0u;
        a_hit[c] += seen[c] && v[c] >= (unsigned)g.thr ? 1u : 0u;
      }
    }
  }
  // ---- the tile's planes: read, add, write, once ----
  if (a_cnt[0] | a_cnt[1] | a_cnt[2] | a_cnt[3]) {
    const int64_t at = (int64_t)iy * g.W + ix0;
    uint4 *qs = reinterpret_cast<uint4 *>(p_sum + at), *qc = reinterpret_cast<uint4 *>(p_cnt + at), *qh = reinterpret_cast<uint4 *>(p_hit + at);
    uint4 vs = *qs, vc = *qc, vh = *qh;
    vs.x += a_sum[0], vs.y += a_sum[1], vs.z += a_sum[2], vs.w += a_sum[3];
    vc.x += a_cnt[0], vc.y += a_cnt[1], vc.z += a_cnt[2], vc.w += a_cnt[3];
    vh.x += a_hit[0], vh.y += a_hit[1], vh.z += a_hit[2], vh.w += a_hit[3];
    *qs = vs, *qc = vc, *qh = vh;
  }
}

// one thread per cell of the window [x, x + w) x [y, y + hgt) -> out [hgt][w] bytes
__global__ __launch_bounds__(THREADS) void gm_render(const unsigned *__restrict__ p_sum, const unsigned *__restrict__ p_cnt,
                                                     const unsigned *__restrict__ p_hit, int W, int mode, unsigned min_obs, int x, int y, int w,
                                                     int hgt, uint8_t *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (i >= (int64_t)w * hgt) return;
  const int r = (int)(i / w), c = (int)(i - (int64_t)r * w);
  const int64_t at = (int64_t)(y + r) * W + (x + c);
  const unsigned long long cnt = p_cnt[at];
  uint8_t v;
  if (mode == RSX_GRIDMAP_MEAN) {
    const unsigned long long m = cnt >= min_obs ? (2ull * p_sum[at] + cnt) / (2ull * cnt) : 0ull;
    v = (uint8_t)(m < 255ull ? m : 255ull);
  } else {
    v = cnt >= min_obs ? (uint8_t)((200ull * p_hit[at] + cnt) / (2ull * cnt)) : (uint8_t)0xff;  // (int8 -1)
  }
  out[i] = v;
}

}  // namespace

using rsx::check_render;  // (gridmap.h)
using rsx::check_window;
using rsx::fail;

namespace {

bool pos_finite(double v) { return v > 0.0 && std::isfinite(v); }

int check_params(const rsx_gridmap_params &p) {
  if (p.width < 64 || p.width > MAX_SIDE || p.width % 64) return fail(RSX_ERR_BAD_ARG, "width %d: 64 .. %d and a multiple of 64", p.width, MAX_SIDE);
  if (p.height < 64 || p.height > MAX_SIDE || p.height % 64)
    return fail(RSX_ERR_BAD_ARG, "height %d: 64 .. %d and a multiple of 64", p.height, MAX_SIDE);
  if (!pos_finite(p.resolution)) return fail(RSX_ERR_BAD_ARG, "resolution must be positive and finite");
  if (!std::isfinite(p.origin_x) || !std::isfinite(p.origin_y)) return fail(RSX_ERR_BAD_ARG, "origin must be finite");
  if (!pos_finite(p.range_resolution)) return fail(RSX_ERR_BAD_ARG, "range_resolution must be positive and finite");
  if (p.min_range_bins < 0) return fail(RSX_ERR_BAD_ARG, "min_range_bins %d < 0", p.min_range_bins);
  if (p.range_halfwidth < 0 || p.range_halfwidth > MAX_COLS) return fail(RSX_ERR_BAD_ARG, "range_halfwidth %d outside 0 .. %d", p.range_halfwidth, MAX_COLS);
  if (p.hit_threshold < 0 || p.hit_threshold > 255) return fail(RSX_ERR_BAD_ARG, "hit_threshold %d outside 0 .. 255", p.hit_threshold);
  if (!(p.max_range >= 0.0) || !std::isfinite(p.max_range)) return fail(RSX_ERR_BAD_ARG, "max_range must be finite and not negative");
  return RSX_OK;
}

Geometry geometry_of(const rsx_gridmap_params &p, int rows, int cols) {
  Geometry g{};
  g.res = p.resolution, g.ox = p.origin_x, g.oy = p.origin_y, g.rr = p.range_resolution;
  const double e = (double)cols * g.rr;
  g.e_hi = e * e;
  g.max2 = p.max_range > 0.0 ? p.max_range * p.max_range : std::numeric_limits<double>::infinity();
  // the tile test compares distances in the map frame with bounds taken in the sensor frame: the margin covers the rounding of
  // both and a matrix within 1e-7 of a rotation
  const double reach2 = g.e_hi < g.max2 ? g.e_hi : g.max2, lo = (double)p.min_range_bins * g.rr;
  g.reach2 = reach2 * (1.0 + 1e-6);
  g.hole2 = lo * lo * (1.0 - 1e-6);
  g.inv_rr = (float)(1.0 / g.rr);
  g.rows_per_rad = (float)((double)rows / (2.0 * M_PI));
  g.W = p.width, g.H = p.height, g.rows = rows, g.cols = cols;
  g.lo_bin = p.min_range_bins, g.hw = p.range_halfwidth, g.thr = p.hit_threshold;
  return g;
}

int check_batch(const rsx_gridmap *h, int32_t n_images, int64_t image_stride_bytes, int32_t row_stride, int32_t col_offset) {
  if (n_images < 0 || n_images > MAX_IMAGES) return fail(RSX_ERR_BAD_ARG, "n_images %d outside 0 .. %d", n_images, MAX_IMAGES);
  return rsx::check_polar_layout(h->rows, h->cols, n_images, image_stride_bytes, row_stride, col_offset);
}

// n device images at their transforms into the planes: one launch, nothing read on the host
int add_device(rsx_gridmap *h, const uint8_t *d_imgs, int64_t img_stride, int n, int32_t stride, int32_t off, const double *d_tf, int *d_status,
               hipStream_t s) {
  const dim3 grid((unsigned)(h->p.width / TILE), (unsigned)(h->p.height / TILE));
  hipLaunchKernelGGL(gm_add, grid, dim3(THREADS), (size_t)h->rows * sizeof(float2), s, d_imgs, img_stride, n, stride, off, d_tf, h->table.as<float2>(),
                     h->g, h->plane(0), h->plane(1), h->plane(2), d_status);
  RSX_HIP(hipGetLastError());
  return RSX_OK;
}

int render_device(rsx_gridmap *h, int32_t mode, int32_t min_observations, int32_t x, int32_t y, int32_t w, int32_t hgt, void *d_out, hipStream_t s) {
  const int64_t n = (int64_t)w * hgt;
  hipLaunchKernelGGL(gm_render, dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, h->plane(0), h->plane(1), h->plane(2), h->p.width,
                     mode, (unsigned)min_observations, x, y, w, hgt, static_cast<uint8_t *>(d_out));
  RSX_HIP(hipGetLastError());
  return RSX_OK;
}

}  // namespace

extern "C" {

int rsx_gridmap_default_params(rsx_gridmap_params *p) try {
  if (!p) return fail(RSX_ERR_BAD_ARG, "null params");
  p->width = 1024;
  p->height = 1024;
  p->resolution = 0.5;
  p->origin_x = -256.0;
  p->origin_y = -256.0;
  p->range_resolution = 0.0595;  // Navtech CIR204-H / MulRan
  p->max_range = 0.0;
  p->min_range_bins = 58;
  p->range_halfwidth = 4;        // floor(resolution / (2 range_resolution))
  p->hit_threshold = 120;
  p->reserved = 0;
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_gridmap_create(int device, int32_t rows, int32_t cols, const rsx_gridmap_params *params, rsx_gridmap **out) try {
  if (!out) return fail(RSX_ERR_BAD_ARG, "null out");
  *out = nullptr;
  if (rows < 1 || rows > MAX_ROWS || cols < 2 || cols > MAX_COLS) return fail(RSX_ERR_BAD_ARG, "image shape %d x %d unsupported", rows, cols);
  rsx_gridmap_params p;
  rsx_gridmap_default_params(&p);
  if (params) p = *params;
  RSX_TRY(check_params(p));
  RSX_TRY(rsx::check_device(device));
  std::unique_ptr<rsx_gridmap> h(new (std::nothrow) rsx_gridmap());
  if (!h) return fail(RSX_ERR_OOM, "host alloc");
  h->device = device;
  h->rows = rows;
  h->cols = cols;
  h->p = p;
  h->g = geometry_of(p, rows, cols);
  std::vector<float> tab((size_t)rows * 2);  // fp64, rounded once
  for (int a = 0; a < rows; a++) {
    const double ang = 2.0 * M_PI * (double)a / (double)rows;
    tab[2 * a] = (float)std::cos(ang);
    tab[2 * a + 1] = (float)std::sin(ang);
  }
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = h->stream.create();
  if (e != hipSuccess) return fail(RSX_ERR_HIP, "create: %s", hipGetErrorString(e));
  RSX_TRY(h->planes.reserve(3 * h->plane_bytes(), h->stream, false));
  RSX_TRY(h->table.reserve(tab.size() * sizeof(float), h->stream, false));
  RSX_HIP(hipMemsetAsync(h->planes.p, 0, 3 * h->plane_bytes(), h->stream));
  RSX_HIP(hipMemcpyAsync(h->table.p, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
  RSX_HIP(hipStreamSynchronize(h->stream));
  *out = h.release();
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_gridmap_destroy(rsx_gridmap *h) try {
  if (!h) return RSX_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  delete h;
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_gridmap_clear(rsx_gridmap *h, void *stream) try {
  if (!h) return fail(RSX_ERR_BAD_ARG, "null handle");
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
  RSX_TRY(h->order.enter(s));
  RSX_HIP(hipMemsetAsync(h->planes.p, 0, 3 * h->plane_bytes(), s));
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_gridmap_add_batch_device(rsx_gridmap *h, const uint8_t *d_imgs, int32_t n_images, int64_t image_stride_bytes, int32_t row_stride,
                                 int32_t col_offset, const double *d_transforms, int32_t *d_status, void *stream) try {
  if (n_images < 0 || (n_images && (!d_imgs || !d_transforms))) return fail(RSX_ERR_BAD_ARG, "bad arg");
  if (!h) return fail(RSX_ERR_BAD_ARG, "null handle");
  RSX_TRY(check_batch(h, n_images, image_stride_bytes, row_stride, col_offset));
  if (n_images == 0) return RSX_OK;
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
  RSX_TRY(h->order.enter(s));
  return add_device(h, d_imgs, image_stride_bytes, n_images, row_stride, col_offset, d_transforms, d_status, s);
} RSX_CATCH_ALL

int rsx_gridmap_add_batch(rsx_gridmap *h, const uint8_t *imgs, int32_t n_images, int64_t image_stride_bytes, int32_t row_stride,
                          int32_t col_offset, const double *transforms) try {
  if (n_images < 0 || (n_images && (!imgs || !transforms))) return fail(RSX_ERR_BAD_ARG, "bad arg");
  for (int64_t i = 0; i < (int64_t)n_images * 6; i++)
    if (!std::isfinite(transforms[i])) return fail(RSX_ERR_BAD_ARG, "transform %d is not finite", (int)(i / 6));
  if (!h) return fail(RSX_ERR_BAD_ARG, "null handle");
  RSX_TRY(check_batch(h, n_images, image_stride_bytes, row_stride, col_offset));
  if (n_images == 0) return RSX_OK;
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  RSX_TRY(h->order.enter(s));
  const size_t ibytes = (size_t)h->rows * row_stride;
  for (int b0 = 0; b0 < n_images; b0 += rsx::MAX_SUB_BATCH) {  // sub-batches bound the staging memory
    const int n = n_images - b0 < rsx::MAX_SUB_BATCH ? n_images - b0 : rsx::MAX_SUB_BATCH;
    RSX_TRY(h->img.reserve(ibytes * n, s, false));
    RSX_TRY(h->tf.reserve((size_t)n * 6 * sizeof(double), s, false));
    RSX_TRY(rsx::upload_images(h->img.p, imgs + (int64_t)b0 * image_stride_bytes, n, ibytes, image_stride_bytes, s));
    RSX_HIP(hipMemcpyAsync(h->tf.p, transforms + (size_t)b0 * 6, (size_t)n * 6 * sizeof(double), hipMemcpyHostToDevice, s));
    RSX_TRY(add_device(h, h->img.as<uint8_t>(), (int64_t)ibytes, n, row_stride, col_offset, h->tf.as<double>(), nullptr, s));
    RSX_HIP(hipStreamSynchronize(s));
  }
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_gridmap_read(rsx_gridmap *h, int32_t x, int32_t y, int32_t w, int32_t hgt, uint32_t *out_sum, uint32_t *out_cnt, uint32_t *out_hit) try {
  if (!h) return fail(RSX_ERR_BAD_ARG, "null handle");
  RSX_TRY(check_window(h, x, y, w, hgt));
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  RSX_TRY(h->order.enter(s));
  uint32_t *outs[3] = {out_sum, out_cnt, out_hit};
  for (int k = 0; k < 3; k++)
    if (outs[k])
      RSX_HIP(hipMemcpy2DAsync(outs[k], (size_t)w * 4, h->plane(k) + (size_t)y * h->p.width + x, (size_t)h->p.width * 4, (size_t)w * 4, (size_t)hgt,
                               hipMemcpyDeviceToHost, s));
  RSX_HIP(hipStreamSynchronize(s));
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_gridmap_planes_device(rsx_gridmap *h, uint32_t **d_sum, uint32_t **d_cnt, uint32_t **d_hit, int64_t *pitch_bytes) try {
  if (!h) return fail(RSX_ERR_BAD_ARG, "null handle");
  if (d_sum) *d_sum = h->plane(0);
  if (d_cnt) *d_cnt = h->plane(1);
  if (d_hit) *d_hit = h->plane(2);
  if (pitch_bytes) *pitch_bytes = (int64_t)h->p.width * 4;
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_gridmap_render_device(rsx_gridmap *h, int32_t mode, int32_t min_observations, int32_t x, int32_t y, int32_t w, int32_t hgt, void *d_out,
                              void *stream) try {
  RSX_TRY(check_render(mode, min_observations));
  if (!d_out) return fail(RSX_ERR_BAD_ARG, "null out");
  if (!h) return fail(RSX_ERR_BAD_ARG, "null handle");
  RSX_TRY(check_window(h, x, y, w, hgt));
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
  RSX_TRY(h->order.enter(s));
  return render_device(h, mode, min_observations, x, y, w, hgt, d_out, s);
} RSX_CATCH_ALL

int rsx_gridmap_render(rsx_gridmap *h, int32_t mode, int32_t min_observations, int32_t x, int32_t y, int32_t w, int32_t hgt, void *out) try {
  RSX_TRY(check_render(mode, min_observations));
  if (!out) return fail(RSX_ERR_BAD_ARG, "null out");
  if (!h) return fail(RSX_ERR_BAD_ARG, "null handle");
  RSX_TRY(check_window(h, x, y, w, hgt));
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  RSX_TRY(h->order.enter(s));
  RSX_TRY(h->out.reserve((size_t)w * hgt, s, false));
  RSX_TRY(render_device(h, mode, min_observations, x, y, w, hgt, h->out.p, s));
  RSX_HIP(hipMemcpyAsync(out, h->out.p, (size_t)w * hgt, hipMemcpyDeviceToHost, s));
  RSX_HIP(hipStreamSynchronize(s));
  return RSX_OK;
} RSX_CATCH_ALL

}  // extern "C"
