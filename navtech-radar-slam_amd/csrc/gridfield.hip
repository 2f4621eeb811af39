// gridfield.hip -- a likelihood field in the likelihood plane of the rsx_gridmap handle on gfx950: an exact Euclidean distance transform,
// truncated at a radius, from the cells at or above a threshold, and a table that turns the squared distance into the byte that
// match, search and refine read.  None of this is in the reference checkout: the rule is the one stated in include/rsx.h and restated
// in tests/gridfield_np.py (PARITY UNPINNED): integers throughout, so the plane is the restatement's byte for byte.
//
// The transform is in place, so it must not read a cell that another workgroup overwrites.  Two launches whatever the map, no atomics:
//   gf_seeds  one thread per map cell: the byte against the threshold, one 64-bit ballot per wavefront (a map row is a multiple of 64
//             cells: a wavefront never straddles two rows), lane 0 stores the word.  width height / 8 bytes.
//   gf_field  one workgroup per tile of 64 x 32 cells; it reads the bits and the table, never the plane.
//             1. the bit rows of the tile and of `radius` rows above and below it, three words each (the tile's and its neighbours';
//                rows and words outside the map are 0), and the table go into LDS
//             2. a thread per (row, column): the distance to the nearest seed along the row, from the count of trailing zeros of the
//                64 cells to the right and of leading zeros of the 64 cells to the left, each a window shifted out of two words; the
//                cell at 64 exactly is one more bit.  No loop over dx.  A byte per cell, 255 for "none within the radius"
//             3. a thread per four neighbouring cells of a row and of the row 16 below it: q = min over |dy| <= radius of dy dy + g g,
//                the four g of a row from one 32-bit LDS read; 255 squared is above any radius squared, so "none" needs no test;
//                the table gives the byte, four of them are stored as one word (the plane's pitch is a multiple of 64)
//             17.8 KB of static LDS: 3840 of bits, 10240 of row distances, 4100 of table.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <vector>

#include "gridmap.h"

namespace {

using rsx::fail;
using rsx::no_likelihood;

constexpr int NT = 256;
constexpr int MAX_R = RSX_GRIDMAP_FIELD_MAX_RADIUS;
constexpr int TX = 64, TY = 32;                    // a tile: one word of bits wide
constexpr int ROWS = TY + 2 * MAX_R;               // bit rows of a tile with its halo at the largest radius
constexpr int TABLE = MAX_R * MAX_R + 1;           // entries of the largest table
constexpr int TABLE_WORDS = (TABLE + 3) / 4;
constexpr unsigned NONE = 255u;                    // no seed within the radius along the row
static_assert(MAX_R <= 64, "a row distance is found in one 64-bit window a side and one more bit");
static_assert(MAX_R <= rsx::GRIDMAP_LIKE_MARGIN, "");
static_assert(NONE * NONE > (unsigned)(MAX_R * MAX_R) && NONE > (unsigned)MAX_R, "");
static_assert(NT == 16 * (TY / 2) && TX == 16 * 4, "step 3: a thread owns 4 cells of row y and of row y + TY / 2");

__global__ __launch_bounds__(NT) void gf_seeds(const uint8_t *__restrict__ origin, int64_t pitch, int W, int H, unsigned threshold,
                                               unsigned long long *__restrict__ bits) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;  // (W H is a multiple of NT: no thread is beyond the map)
  const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
  const unsigned long long word = __ballot(origin[(int64_t)y * pitch + x] >= threshold);
  if ((threadIdx.x & 63) == 0) bits[i >> 6] = word;
}

// the distance from bit b of w1 to the nearest set bit of the row w0 w1 w2 (64 cells each, w1 in the middle), 0 .. 64, or more than
// 64 when there is none that near
__device__ inline unsigned row_distance(unsigned long long w0, unsigned long long w1, unsigned long long w2, int b) {
  // to the right, the cell itself first: bit k is the cell k to the right, k = 0 .. 63; the cell 64 to the right is bit b of w2
  const unsigned long long right = (w1 >> b) | (b ? w2 << (64 - b) : 0ull);
  // to the left, the cell itself first: bit 63 - k is the cell k to the left; the cell 64 to the left is bit b of w0
  const unsigned long long left = (w1 << (63 - b)) | (b < 63 ? w0 >> (b + 1) : 0ull);
  const unsigned dr = right ? (unsigned)__builtin_ctzll(right) : ((w2 >> b) & 1ull ? 64u : NONE);
  const unsigned dl = left ? (unsigned)__builtin_clzll(left) : ((w0 >> b) & 1ull ? 64u : NONE);
  return dl < dr ? dl : dr;
}

__global__ __launch_bounds__(NT) void gf_field(const unsigned long long *__restrict__ bits, const unsigned *__restrict__ table, int W, int H, int R,
                                               uint8_t *__restrict__ origin, int64_t pitch) {
  __shared__ unsigned long long rows[ROWS][3];
  __shared__ __attribute__((aligned(4))) uint8_t dist[ROWS][TX];
  __shared__ unsigned tab[TABLE_WORDS];
  const int tid = threadIdx.x;
  const int bx = blockIdx.x, y0 = (int)blockIdx.y * TY;
  const int words = W / 64, n_rows = TY + 2 * R;
  // ---- 1. the bits of the tile and its halo, the table ----
  for (int i = tid; i < n_rows * 3; i += NT) {
    const int r = i / 3, j = i - 3 * r;
    const int y = y0 - R + r, wx = bx - 1 + j;
    rows[r][j] = y >= 0 && y < H && wx >= 0 && wx < words ? bits[(int64_t)y * words + wx] : 0ull;
  }
  for (int i = tid; i < (R * R + 4) / 4; i += NT) tab[i] = table[i];  // (the buffer holds TABLE_WORDS words whatever the radius)
  __syncthreads();
  // ---- 2. the distance to the nearest seed along the row, a wavefront per row ----
  for (int i = tid; i < n_rows * TX; i += NT) {
    const int r = i >> 6, b = i & 63;
    const unsigned g = row_distance(rows[r][0], rows[r][1], rows[r][2], b);
    dist[r][b] = (uint8_t)(g <= (unsigned)R ? g : NONE);
  }
  __syncthreads();
  // ---- 3. q = min over dy of dy dy + g g; the byte from the table ----
  const int xq = (tid & 15) * 4, ya = tid >> 4, yb = ya + TY / 2;
  unsigned best[8];
#pragma unroll
  for (int k = 0; k < 8; k++) best[k] = ~0u;
  for (int dy = -R; dy <= R; dy++) {
    const unsigned d2 = (unsigned)(dy * dy);
    const unsigned va = *reinterpret_cast<const unsigned *>(&dist[ya + R + dy][xq]);
    const unsigned vb = *reinterpret_cast<const unsigned *>(&dist[yb + R + dy][xq]);
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const unsigned ga = (va >> (8 * k)) & 255u, gb = (vb >> (8 * k)) & 255u;
      const unsigned qa = d2 + ga * ga, qb = d2 + gb * gb;
      best[k] = qa < best[k] ? qa : best[k];
      best[4 + k] = qb < best[4 + k] ? qb : best[4 + k];
    }
  }
  const uint8_t *tab8 = reinterpret_cast<const uint8_t *>(tab);
  const unsigned r2 = (unsigned)(R * R);
  unsigned out[2] = {0u, 0u};
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const unsigned q = best[k] <= r2 ? best[k] : 0u;  // (an index in the table either way)
    const unsigned v = best[k] <= r2 ? (unsigned)tab8[q] : 0u;
    out[k >> 2] |= v << (8 * (k & 3));
  }
  uint8_t *cell = origin + (int64_t)(y0 + ya) * pitch + (int64_t)bx * TX + xq;
  *reinterpret_cast<unsigned *>(cell) = out[0];
  *reinterpret_cast<unsigned *>(cell + (int64_t)(TY / 2) * pitch) = out[1];
}

int check_params(const rsx_gridmap_field_params &p) {
  if (p.threshold < 1 || p.threshold > 255) return fail(RSX_ERR_BAD_ARG, "threshold %d outside 1 .. 255", p.threshold);
  if (p.radius < 1 || p.radius > MAX_R) return fail(RSX_ERR_BAD_ARG, "radius %d outside 1 .. %d", p.radius, MAX_R);
  if (p.reserved0 != 0 || p.reserved1 != 0) return fail(RSX_ERR_BAD_ARG, "reserved must be 0");
  return RSX_OK;
}

int check_table(double sigma, int32_t peak, int32_t radius) {
  if (!(sigma > 0.0) || !std::isfinite(sigma)) return fail(RSX_ERR_BAD_ARG, "sigma_cells must be positive and finite");
  if (peak < 1 || peak > 255) return fail(RSX_ERR_BAD_ARG, "peak %d outside 1 .. 255", peak);
  if (radius < 1 || radius > MAX_R) return fail(RSX_ERR_BAD_ARG, "radius %d outside 1 .. %d", radius, MAX_R);
  return RSX_OK;
}

void gaussian_table(double sigma, int32_t peak, int32_t radius, uint8_t *out) {
  const double two_var = (2.0 * sigma) * sigma;
  for (int q = 0; q <= radius * radius; q++) out[q] = (uint8_t)std::floor((double)peak * std::exp(-(double)q / two_var) + 0.5);
}

}  // namespace

extern "C" {

int rsx_gridmap_field_default_params(rsx_gridmap_field_params *p) try {
  if (!p) return fail(RSX_ERR_BAD_ARG, "null params");
  p->threshold = 50;
  p->radius = 12;
  p->reserved0 = 0;
  p->reserved1 = 0;
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_gridmap_field_gaussian_table(double sigma_cells, int32_t peak, int32_t radius, uint8_t *out) try {
  RSX_TRY(check_table(sigma_cells, peak, radius));
  if (!out) return fail(RSX_ERR_BAD_ARG, "null out");
  gaussian_table(sigma_cells, peak, radius, out);
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_gridmap_likelihood_field(rsx_gridmap *h, const rsx_gridmap_field_params *params, const uint8_t *table, void *stream) try {
  rsx_gridmap_field_params p;
  rsx_gridmap_field_default_params(&p);
  if (params) p = *params;
  RSX_TRY(check_params(p));
  if (!h) return fail(RSX_ERR_BAD_ARG, "null handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (!h->have_like) return no_likelihood();
  const size_t n = (size_t)p.radius * p.radius + 1;
  std::vector<uint8_t> made;
  if (!table) {
    made.resize(n);
    gaussian_table(3.0, 255, p.radius, made.data());
    table = made.data();
  }
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
  RSX_TRY(h->order.enter(s));
  const int W = h->p.width, H = h->p.height;  // multiples of 64 (rsx_gridmap_create): of the tile, of a wavefront, of a stored word
  RSX_TRY(h->f_bits.reserve((size_t)W * H / 8, s, false));
  RSX_TRY(h->f_table.reserve((size_t)TABLE_WORDS * 4, s, false));
  if (h->f_table_host.size() != n || memcmp(h->f_table_host.data(), table, n) != 0) {
    // behind everything the handle has in flight that reads the old table; the caller's memory is free again on return
    h->f_table_host.clear();
    RSX_HIP(hipMemcpyAsync(h->f_table.p, table, n, hipMemcpyHostToDevice, s));
    RSX_HIP(hipStreamSynchronize(s));
    h->f_table_host.assign(table, table + n);
  }
  hipLaunchKernelGGL(gf_seeds, dim3((unsigned)((size_t)W * H / NT)), dim3(NT), 0, s, h->like_origin(), h->like_pitch(), W, H, (unsigned)p.threshold,
                     h->f_bits.as<unsigned long long>());
  RSX_HIP(hipGetLastError());
  hipLaunchKernelGGL(gf_field, dim3((unsigned)(W / TX), (unsigned)(H / TY)), dim3(NT), 0, s, h->f_bits.as<unsigned long long>(), h->f_table.as<unsigned>(),
                     W, H, p.radius, h->like_origin(), h->like_pitch());
  RSX_HIP(hipGetLastError());
  return RSX_OK;
} RSX_CATCH_ALL

}  // extern "C"
