// radarsc.hip -- radar scan-context descriptors straight from the polar image on gfx950, batched.
//
// The "radar scan context" the reference's README names (Kim et al., MulRan, ICRA 2020): the 20 x 60 polar grid of
// Scancontext.cpp:151-195 filled with received power instead of point heights.  MulRan's own builder is not part of the
// reference checkout, so the rule is the one pinned in tests/radarsc_np.py (PARITY UNPINNED): the ring of a range bin and the
// sector of an azimuth row by the index formulas of SC.cpp:175-179 in fp64, a cell = the mean (integer sum / count, one fp64
// division) or the maximum of max(p - power_floor, 0) over its samples.  Integer sums: the result does not depend on the
// order of the reduction, the contract is bit identity.
//
// One launch per batch, one workgroup per (image, sector) item (grid-strided over at most 2048 workgroups):
//   1. every thread decides the sector of its azimuth rows (fp64, the device reads the grid: per-image grids cost nothing)
//      and the rows of this sector are listed in LDS;
//   2. as many listed rows at a time as the 10 KB staging buffer holds (7 of a 400 x 3360 scan's, at most 12), the bytes
//      between the first and the last ring bin go into LDS by aligned 16-byte
//      loads (the workgroup's only HBM reads: nothing in front of min_range, nothing behind the last ring but the tail of
//      the last 16 bytes; a 16-byte piece that is not wholly inside the image -- possible only at its two ends -- is read
//      byte by byte);
//   3. one thread per (row, ring) sums its ~67 bytes out of LDS four to a register (v_sad_u8; the floor by two
//      v_pk_max_u16 in front of it) and adds the sum to the ring's LDS word;
//   4. 20 threads divide and write the sector's 80 bytes.
// Ring limits are a function of the handle's parameters only: the host works them out once, at create.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <new>

#include "keypoints_host.h"
#include "radarsc.h"

namespace {

constexpr int NR = RSX_SC_NUM_RING, NS = RSX_SC_NUM_SECTOR, DS = RSX_SC_DESC_SIZE;
constexpr int MAX_COLS = 8192, MAX_ROWS = 4096;
constexpr int THREADS = 256;
constexpr int STAGE_BYTES = 10240;           // >= one row's pieces at MAX_COLS (8224 B); with the row list 18.6 KB of LDS: 8 workgroups per CU
constexpr int MAX_PASS_ROWS = THREADS / NR;  // one thread per (row, ring) of a pass
constexpr int MAX_GRID = 2048;               // memory-bound kernel: 256 CUs x 8 workgroups, grid-stride the rest
constexpr int MAX_IMAGES = 1 << 24;

struct Geometry {
  int lo, hi;           // range bins [lo, hi) belong to a ring
  int chunks;           // 16-byte pieces staged per row: ceil((hi - lo + 15) / 16), at least 2
  unsigned inv_chunks;  // floor(2^32 / chunks) + 1 (chunks >= 2, so it fits): i / chunks = umulhi(i, inv_chunks) for i < 2^32 / chunks
  int pass_rows;        // rows staged at a time
  int floor, stat;
};

// SC.cpp:179 on the row's azimuth, fp64; -1: not finite
__device__ __forceinline__ int sector_of(float az) {
  if ((__float_as_uint(az) & 0x7f800000u) == 0x7f800000u) return -1;
  const double th = (double)az * 57.29577951308232;
  const double q = th / 360.0;
  const double t = q - floor(q);
  int s = (int)ceil(t * 60.0);
  s = s < NS ? s : NS;
  s = s > 1 ? s : 1;
  return s - 1;
}

typedef unsigned short rc_us2 __attribute__((ext_vector_type(2)));

// acc + sum over the four bytes b of v of max(b - f, 0); f2 = f in both halves, f4 = f in all four bytes
__device__ __forceinline__ unsigned sum_above_floor(unsigned v, unsigned f2, unsigned f4, unsigned acc) {
  const rc_us2 F = __builtin_bit_cast(rc_us2, f2);
  const rc_us2 e = __builtin_elementwise_max(__builtin_bit_cast(rc_us2, v & 0x00ff00ffu), F);
  const rc_us2 o = __builtin_elementwise_max(__builtin_bit_cast(rc_us2, (v >> 8) & 0x00ff00ffu), F);
  const unsigned c = __builtin_bit_cast(unsigned, e) | (__builtin_bit_cast(unsigned, o) << 8);
  return __builtin_amdgcn_sad_u8(c, f4, acc);
}

__device__ __forceinline__ unsigned max_byte(unsigned v, unsigned m) {
  const unsigned a = v & 0xffu, b = (v >> 8) & 0xffu, c = (v >> 16) & 0xffu, d = v >> 24;
  const unsigned ab = a > b ? a : b, cd = c > d ? c : d, x = ab > cd ? ab : cd;
  return x > m ? x : m;
}

__global__ __launch_bounds__(THREADS) void rc_build(const uint8_t *__restrict__ imgs, int64_t img_stride, int n_images, int rows, int stride, int off,
                                                    const float *__restrict__ az, int64_t az_stride, const int *__restrict__ edges, Geometry g,
                                                    float *__restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[STAGE_BYTES];
  __shared__ uint16_t list[MAX_ROWS];
  __shared__ int edge[NR + 1];
  __shared__ unsigned long long acc[NR];  // (64 bits: 4096 rows x 8192 bins of one ring x 255 does not fit 32)
  __shared__ unsigned n_list;
  const int tid = threadIdx.x;
  if (tid <= NR) edge[tid] = edges[tid];
  const int len = g.hi - g.lo;
  const unsigned f1 = (unsigned)g.floor, f2 = f1 | (f1 << 16), f4 = f2 | (f2 << 8);
  for (int w = blockIdx.x; w < n_images * NS; w += gridDim.x) {
    const int img = w / NS, sec = w - img * NS;
    if (tid < NR) acc[tid] = 0ull;
    if (tid == 0) n_list = 0u;
    __syncthreads();
    // ---- 1. the rows of this sector ----
    const float *azi = az + (int64_t)img * az_stride;
    if (len > 0)
      for (int a = tid; a < rows; a += THREADS)
        if (sector_of(azi[a]) == sec) list[atomicAdd(&n_list, 1u)] = (uint16_t)a;
    __syncthreads();
    const int nrow = (int)n_list;
    // (offsets from imgs, so that the loads stay global loads; base16: the alignment of imgs itself)
    const int64_t ilo = (int64_t)img * img_stride, ihi = ilo + (int64_t)rows * stride;
    const int64_t base16 = (int64_t)(reinterpret_cast<uintptr_t>(imgs) & 15u);
    for (int p0 = 0; p0 < nrow; p0 += g.pass_rows) {
      const int np = nrow - p0 < g.pass_rows ? nrow - p0 : g.pass_rows;
      // ---- 2. bytes [lo, hi) of np rows -> LDS, in the aligned 16-byte pieces that hold them ----
      for (int i = tid; i < np * g.chunks; i += THREADS) {
        const int r = (int)__umulhi((unsigned)i, g.inv_chunks), c = i - r * g.chunks;
        const int64_t A = ilo + (int64_t)list[p0 + r] * stride + off + g.lo;  // the row's bin lo
        const int64_t ch = A - ((A + base16) & 15) + 16 * c;                  // an aligned 16-byte piece
        if (ch >= A + len) continue;                                          // behind the last ring bin
        uint4 v;
        if (ch >= ilo && ch + 16 <= ihi) {
          v = *reinterpret_cast<const uint4 *>(imgs + ch);
        } else {  // the piece sticks out of the image (its first or last bytes): only the bytes inside
          unsigned d[4] = {0u, 0u, 0u, 0u};
#pragma unroll
          for (int b = 0; b < 16; b++) {
            const int64_t p = ch + b;
            if (p >= ilo && p < ihi) d[b >> 2] |= (unsigned)imgs[p] << (8 * (b & 3));
          }
          v = make_uint4(d[0], d[1], d[2], d[3]);
        }
        *reinterpret_cast<uint4 *>(stage + 16 * i) = v;
      }
      __syncthreads();
      // ---- 3. one thread per (row, ring) ----
      if (tid < np * NR) {
        const int r = tid / NR, k = tid - r * NR;
        const int64_t A = ilo + (int64_t)list[p0 + r] * stride + off + g.lo;
        const int m = (int)((A + base16) & 15);
        const int b0 = m + edge[k] - g.lo, b1 = m + edge[k + 1] - g.lo;  // the ring's bytes in the row's pieces
        if (b1 > b0) {
          const unsigned *sw = reinterpret_cast<const unsigned *>(stage + 16 * r * g.chunks);
          unsigned s = 0u;
          for (int d = b0 >> 2; d <= (b1 - 1) >> 2; d++) {
            const int first = b0 - 4 * d > 0 ? b0 - 4 * d : 0, last = b1 - 4 * d < 4 ? b1 - 4 * d : 4;
            const unsigned mask = (0xffffffffu << (8 * first)) & (0xffffffffu >> (8 * (4 - last)));
            const unsigned v = sw[d] & mask;
            s = g.stat == RSX_RADARSC_MAX ? max_byte(v, s) : sum_above_floor(v, f2, f4, s);
          }
          if (g.stat == RSX_RADARSC_MAX) atomicMax(&acc[k], (unsigned long long)s);
          else atomicAdd(&acc[k], (unsigned long long)s);
        }
      }
      __syncthreads();
    }
    // ---- 4. the sector's 20 cells ----
    if (tid < NR) {
      const unsigned long long a = acc[tid];
      const unsigned cnt = (unsigned)nrow * (unsigned)(edge[tid + 1] - edge[tid]);
      float v;
      if (g.stat == RSX_RADARSC_MAX) v = (float)(a > f1 ? (unsigned)a - f1 : 0u);
      else v = cnt ? (float)((double)a / (double)cnt) : 0.0f;
      out[(int64_t)w * NR + tid] = v;
    }
    __syncthreads();
  }
}

}  // namespace

struct rsx_radarsc {
  int device = 0, rows = 0, cols = 0;
  rsx_radarsc_params p{};
  Geometry g{};
  std::mutex mu;
  rsx::Stream stream;
  rsx::DevBuf edges;            // int[21]: first range bin of every ring, then the end of the last one
  rsx::DevBuf img, az, descs;   // staging of the host entries; descs also the scratch of rsx_sc_add_polar*
  rsx::StreamOrder order;
};

using rsx::fail;

namespace {

int check_params(const rsx_radarsc_params &p) {
  if (!(p.resolution > 0.0f) || !std::isfinite(p.resolution)) return fail(RSX_ERR_BAD_ARG, "resolution must be positive");
  if (!(p.max_radius > 0.0) || !std::isfinite(p.max_radius)) return fail(RSX_ERR_BAD_ARG, "max_radius must be positive and finite");
  if (p.min_range < 0) return fail(RSX_ERR_BAD_ARG, "min_range %d < 0", p.min_range);
  if (p.power_floor < 0 || p.power_floor > 255) return fail(RSX_ERR_BAD_ARG, "power_floor %d outside 0 .. 255", p.power_floor);
  if (p.stat != RSX_RADARSC_MEAN && p.stat != RSX_RADARSC_MAX) return fail(RSX_ERR_BAD_ARG, "unknown stat %d", p.stat);
  return RSX_OK;
}

// the ring of every range bin (SC.cpp:175,178 in fp64) -> edge[0 .. 20] and the kernel's geometry
void ring_edges(const rsx_radarsc_params &p, int cols, int *edge, Geometry *g) {
  const double res = (double)p.resolution;
  int lo = p.min_range < cols ? p.min_range : cols, hi = lo;
  for (int k = 0; k <= NR; k++) edge[k] = -1;
  for (int j = lo; j < cols; j++) {
    const double r = ((double)j + 0.5) * res;
    if (r > p.max_radius) break;
    int ring = (int)std::ceil(r / p.max_radius * 20.0);
    ring = (ring < NR ? ring : NR);
    ring = (ring > 1 ? ring : 1) - 1;
    for (int k = 0; k <= ring; k++)
      if (edge[k] < 0) edge[k] = j;
    hi = j + 1;
  }
  for (int k = 0; k <= NR; k++)
    if (edge[k] < 0) edge[k] = hi;
  g->lo = lo;
  g->hi = hi;
  g->chunks = (hi - lo + 15 + 15) / 16;
  if (g->chunks < 2) g->chunks = 2;  // one piece per row would need the multiplier 2^32 + 1; the second piece is never loaded
  g->inv_chunks = (unsigned)((1ull << 32) / (unsigned)g->chunks) + 1u;
  const int fit = STAGE_BYTES / (16 * g->chunks);
  g->pass_rows = fit < MAX_PASS_ROWS ? fit : MAX_PASS_ROWS;
  g->floor = p.power_floor;
  g->stat = p.stat;
}

int check_batch(const rsx_radarsc *h, int32_t n_images, int64_t image_stride_bytes, int32_t row_stride, int32_t col_offset) {
  if (n_images < 0 || n_images > MAX_IMAGES) return fail(RSX_ERR_BAD_ARG, "n_images %d outside 0 .. %d", n_images, MAX_IMAGES);
  return rsx::check_polar_layout(h->rows, h->cols, n_images, image_stride_bytes, row_stride, col_offset);
}

// nb device images -> d_descs [nb][1200]: one launch, nothing read on the host
int build_device(rsx_radarsc *h, const uint8_t *d_imgs, int64_t img_stride, int nb, int32_t stride, int32_t off, const float *d_az, int64_t az_stride,
                 float *d_descs, hipStream_t s) {
  const int64_t items = (int64_t)nb * NS;
  const unsigned grid = (unsigned)(items < MAX_GRID ? items : MAX_GRID);
  hipLaunchKernelGGL(rc_build, dim3(grid), dim3(THREADS), 0, s, d_imgs, img_stride, nb, h->rows, stride, off, d_az, az_stride, h->edges.as<int>(), h->g,
                     d_descs);
  RSX_HIP(hipGetLastError());
  return RSX_OK;
}

}  // namespace

std::mutex &rsx::rc::mutex_of(rsx_radarsc *h) { return h->mu; }
int rsx::rc::device_of(rsx_radarsc *h) { return h->device; }

int rsx::rc::build_scratch_device(rsx_radarsc *h, const uint8_t *d_imgs, int32_t n_images, int64_t image_stride_bytes, int32_t row_stride,
                                  int32_t col_offset, const float *d_azimuths, int32_t azimuths_per_image, hipStream_t s, const float **d_descs) {
  RSX_TRY(check_batch(h, n_images, image_stride_bytes, row_stride, col_offset));
  RSX_TRY(h->order.enter(s));
  RSX_TRY(h->descs.reserve((size_t)n_images * DS * sizeof(float), s, false));
  *d_descs = h->descs.as<float>();
  return build_device(h, d_imgs, image_stride_bytes, n_images, row_stride, col_offset, d_azimuths, azimuths_per_image ? h->rows : 0, h->descs.as<float>(),
                      s);
}

int rsx::rc::upload_and_build(rsx_radarsc *h, const uint8_t *img, int32_t row_stride, int32_t col_offset, const float *azimuths, hipStream_t s,
                              const float **d_descs) {
  RSX_TRY(check_batch(h, 1, 0, row_stride, col_offset));
  RSX_TRY(h->order.enter(s));
  const size_t ibytes = (size_t)h->rows * row_stride;
  RSX_TRY(h->img.reserve(ibytes, s, false));
  RSX_TRY(h->az.reserve((size_t)h->rows * 4, s, false));
  RSX_TRY(h->descs.reserve((size_t)DS * sizeof(float), s, false));
  RSX_HIP(hipMemcpyAsync(h->img.p, img, ibytes, hipMemcpyHostToDevice, s));
  RSX_HIP(hipMemcpyAsync(h->az.p, azimuths, (size_t)h->rows * 4, hipMemcpyHostToDevice, s));
  *d_descs = h->descs.as<float>();
  return build_device(h, h->img.as<uint8_t>(), (int64_t)ibytes, 1, row_stride, col_offset, h->az.as<float>(), 0, h->descs.as<float>(), s);
}

extern "C" {

int rsx_radarsc_default_params(rsx_radarsc_params *p) try {
  if (!p) return fail(RSX_ERR_BAD_ARG, "null params");
  p->max_radius = 80.0;     // SC.h:87 PC_MAX_RADIUS
  p->resolution = 0.0595f;  // Navtech CIR204-H / MulRan
  p->min_range = 58;
  p->power_floor = 0;
  p->stat = RSX_RADARSC_MEAN;
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_radarsc_create(int device, int32_t rows, int32_t cols, const rsx_radarsc_params *params, rsx_radarsc **out) try {
  if (!out) return fail(RSX_ERR_BAD_ARG, "null out");
  *out = nullptr;
  if (rows < 1 || rows > MAX_ROWS || cols < 1 || cols > MAX_COLS) return fail(RSX_ERR_BAD_ARG, "image shape %d x %d unsupported", rows, cols);
  rsx_radarsc_params p;
  rsx_radarsc_default_params(&p);
  if (params) p = *params;
  RSX_TRY(check_params(p));
  RSX_TRY(rsx::check_device(device));
  std::unique_ptr<rsx_radarsc> h(new (std::nothrow) rsx_radarsc());
  if (!h) return fail(RSX_ERR_OOM, "host alloc");
  h->device = device;
  h->rows = rows;
  h->cols = cols;
  h->p = p;
  int edge[NR + 1];
  ring_edges(p, cols, edge, &h->g);
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = h->stream.create();
  if (e != hipSuccess) return fail(RSX_ERR_HIP, "create: %s", hipGetErrorString(e));
  RSX_TRY(h->edges.reserve(sizeof(edge), h->stream, false));
  RSX_HIP(hipMemcpyAsync(h->edges.p, edge, sizeof(edge), hipMemcpyHostToDevice, h->stream));
  RSX_HIP(hipStreamSynchronize(h->stream));
  *out = h.release();
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_radarsc_destroy(rsx_radarsc *h) try {
  if (!h) return RSX_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  delete h;
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_radarsc_build_batch_device(rsx_radarsc *h, const uint8_t *d_imgs, int32_t n_images, int64_t image_stride_bytes, int32_t row_stride,
                                   int32_t col_offset, const float *d_azimuths, int32_t azimuths_per_image, float *d_descs, void *stream) try {
  if (!h || n_images < 0 || (n_images && (!d_imgs || !d_azimuths || !d_descs))) return fail(RSX_ERR_BAD_ARG, "bad arg");
  RSX_TRY(check_batch(h, n_images, image_stride_bytes, row_stride, col_offset));
  if (n_images == 0) return RSX_OK;
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
  RSX_TRY(h->order.enter(s));
  return build_device(h, d_imgs, image_stride_bytes, n_images, row_stride, col_offset, d_azimuths, azimuths_per_image ? h->rows : 0, d_descs, s);
} RSX_CATCH_ALL

int rsx_radarsc_build_batch(rsx_radarsc *h, const uint8_t *imgs, int32_t n_images, int64_t image_stride_bytes, int32_t row_stride,
                            int32_t col_offset, const float *azimuths, int32_t azimuths_per_image, float *out_descs) try {
  if (!h || n_images < 0 || (n_images && (!imgs || !azimuths || !out_descs))) return fail(RSX_ERR_BAD_ARG, "bad arg");
  RSX_TRY(check_batch(h, n_images, image_stride_bytes, row_stride, col_offset));
  if (n_images == 0) return RSX_OK;
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  RSX_TRY(h->order.enter(s));
  const size_t ibytes = (size_t)h->rows * row_stride;
  for (int b0 = 0; b0 < n_images; b0 += rsx::MAX_SUB_BATCH) {  // sub-batches bound the staging memory
    const int n = n_images - b0 < rsx::MAX_SUB_BATCH ? n_images - b0 : rsx::MAX_SUB_BATCH;
    const size_t na = (size_t)h->rows * (azimuths_per_image ? n : 1);
    RSX_TRY(h->img.reserve(ibytes * n, s, false));
    RSX_TRY(h->az.reserve(na * 4, s, false));
    RSX_TRY(h->descs.reserve((size_t)n * DS * sizeof(float), s, false));
    RSX_TRY(rsx::upload_images(h->img.p, imgs + (int64_t)b0 * image_stride_bytes, n, ibytes, image_stride_bytes, s));
    RSX_HIP(hipMemcpyAsync(h->az.p, azimuths + (azimuths_per_image ? (size_t)b0 * h->rows : 0), na * 4, hipMemcpyHostToDevice, s));
    RSX_TRY(build_device(h, h->img.as<uint8_t>(), (int64_t)ibytes, n, row_stride, col_offset, h->az.as<float>(), azimuths_per_image ? h->rows : 0,
                         h->descs.as<float>(), s));
    RSX_HIP(hipMemcpyAsync(out_descs + (int64_t)b0 * DS, h->descs.p, (size_t)n * DS * sizeof(float), hipMemcpyDeviceToHost, s));
    RSX_HIP(hipStreamSynchronize(s));
  }
  return RSX_OK;
} RSX_CATCH_ALL

}  // extern "C"
