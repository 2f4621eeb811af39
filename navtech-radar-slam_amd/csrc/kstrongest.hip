// kstrongest.hip -- k-strongest radar keypoint extraction (the detector of CFEAR radar odometry, with a separation rule) on
// gfx950, batched.
//
// Per azimuth row the k strongest returns above a fixed power floor; no noise model, a hard budget of rows x k keypoints
// per scan.  The rule is integer arithmetic only (include/rsx.h, restated in tests/kstrongest_np.py):
//   key[j] = (v[j] << 16) | (0xFFFF - j);   win[j] = max key over the bins within min_separation of j (cut at the row's ends);
//   candidate: key[j] == win[j], v[j] >= z_min, min_range <= j < hi;   keypoints: the min(k, #candidates) candidates of
//   highest key, in ascending j.
// On powers alone: key[j] == win[j] iff v[j] > v[i] for every bin i < j of the window and v[j] >= v[i] for every bin i > j.
//
// Launch chain of a batch (no host synchronisation, two launches per sub-batch of <= 128 images):
//   ks_rows    one WAVEFRONT per (azimuth, image):
//              1. the row's bytes once into LDS, in the aligned 16-byte pieces that hold them (a piece that sticks out of the
//                 image: only its bytes inside)
//              2. screen, four consecutive bins per lane from three LDS dwords: floor, range limits and the two ADJACENT bins
//                 (separation >= 1) -- the survivors (no two adjacent; a few per cent of a radar row) go, in ascending
//                 bin order (ballots), into a list in LDS
//              3. separation >= 2: one survivor per lane against the rest of its window, the list compacted in place
//              4. more candidates than k: a 256-bin histogram of their powers (LDS atomics), a wave suffix scan over it
//                 from the strongest power down -> the threshold power and how many candidates AT the threshold are kept;
//                 everything above the threshold and the nearest of the ties survive, ranked by ballots so that they land in
//                 ascending bin order in row_kp (row_cap = k) + per-row count
//   kp_pack    (keypoints_host.h, shared with cen2018 and cen2019) row-major packing of the rows' keypoints + polar -> Cartesian
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <mutex>
#include <new>

#include "keypoints_host.h"
#include "kstrongest.h"

namespace {

constexpr int MAX_COLS = 8192;  // LDS of ks_rows: 1024 + 32 + 16 ((cols + 30) / 16) + 2 cols <= 26 KB
constexpr int MAX_ROWS = 4096;
constexpr int MAX_K = 128;
constexpr int MAX_SEP = 32;
constexpr int LOADS = 4;  // 16-byte loads per lane in flight: a 3360-bin row is one round of them

// LDS of one wavefront (dynamic): hist[256] u32 | 16 bytes | the row's 16-byte pieces | 16 bytes | list[cap] u16
__host__ __device__ inline int ks_pieces(int cols) { return (cols + 30) / 16; }  // a row that starts 15 bytes into its first piece
__host__ __device__ inline int ks_list_cap(int cols, int sep) { return sep > 0 ? (cols + 1) / 2 : cols; }  // (no two adjacent survivors)
__host__ __device__ inline size_t ks_lds_bytes(int cols, int sep) {
  return 1024 + 32 + 16 * (size_t)ks_pieces(cols) + 2 * (size_t)((ks_list_cap(cols, sep) + 7) & ~7);
}

__device__ __forceinline__ unsigned lanes_below(unsigned long long m) {  // set bits of m in the lanes below this one
  return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// one wavefront per (azimuth blockIdx.x, image blockIdx.y)
__global__ __launch_bounds__(64) void ks_rows(const uint8_t *__restrict__ imgs, int64_t img_stride, int rows, int cols, int stride, int off, int k,
                                              int z_min, int lo_bin, int hi_bin, int sep, uint16_t *__restrict__ row_kp,
                                              unsigned *__restrict__ row_n) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ks_lds[];
  unsigned *hist = reinterpret_cast<unsigned *>(ks_lds);
  unsigned char *raw = ks_lds + 1024 + 16;  // piece c of the row at raw + 16 c; 16 spare bytes in front and behind
  const int npieces_max = ks_pieces(cols);
  uint16_t *list = reinterpret_cast<uint16_t *>(raw + 16 * (size_t)npieces_max + 16);
  const int lane = threadIdx.x, a = blockIdx.x, img = blockIdx.y;

  // ---- 1. the row's bytes (once): bin j at raw[m + j] ----
  // (offsets from imgs, so that the loads stay global loads; m: where the row starts in its first piece, the alignment of imgs counted)
  const int64_t ilo = (int64_t)img * img_stride, ihi = ilo + (int64_t)rows * stride;
  const int64_t A = ilo + (int64_t)a * stride + off;  // the row's bin 0
  const int m = (int)((A + (int64_t)(reinterpret_cast<uintptr_t>(imgs) & 15u)) & 15);
  const int npieces = (m + cols + 15) / 16;  // <= npieces_max
  // every piece lies inside the image, except perhaps the first piece of its first row and the last piece of its last row.
  // LOADS loads per lane are in flight before the first of them is written to LDS
  auto inside = [&](int c) { return A - m + 16 * (int64_t)c >= ilo && A - m + 16 * (int64_t)c + 16 <= ihi; };
  uint4 *raw16 = reinterpret_cast<uint4 *>(raw);
  for (int c0 = 0; c0 < npieces; c0 += 64 * LOADS) {
    uint4 v[LOADS];
#pragma unroll
    for (int u = 0; u < LOADS; u++) {
      const int c = c0 + 64 * u + lane;
      v[u] = make_uint4(0u, 0u, 0u, 0u);
      if (c < npieces && inside(c)) v[u] = *reinterpret_cast<const uint4 *>(imgs + (A - m + 16 * (int64_t)c));
    }
#pragma unroll
    for (int u = 0; u < LOADS; u++) {
      const int c = c0 + 64 * u + lane;
      if (c < npieces && inside(c)) raw16[c] = v[u];
    }
  }
  if (lane < (npieces > 1 ? 2 : 1)) {  // a piece that sticks out of the image (its first or last bytes): only the bytes inside
    const int c = lane ? npieces - 1 : 0;
    if (!inside(c)) {
      const int64_t ch = A - m + 16 * (int64_t)c;
      unsigned d[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int b = 0; b < 16; b++) {
        const int64_t p = ch + b;
        if (p >= ilo && p < ihi) d[b >> 2] |= (unsigned)imgs[p] << (8 * (b & 3));
      }
      raw16[c] = make_uint4(d[0], d[1], d[2], d[3]);
    }
  }
  __syncthreads();

  // ---- 2. screen: lane l of step t takes dword 64 t + l of the pieces, bins 4 (64 t + l) - m .. + 3 ----
  const unsigned *rawd = reinterpret_cast<const unsigned *>(raw);
  const int ndw = (m + cols + 3) / 4;
  unsigned n_list = 0;  // (wave-uniform)
  for (int d0 = 0; d0 < ndw; d0 += 64) {
    const int d = d0 + lane;
    unsigned mask = 0;
    if (d < ndw) {
      // (dword -1 and dword ndw are the spare bytes: read, never used -- the row's first bin has no left neighbour, its last no right)
      const unsigned wl = rawd[d - 1], w = rawd[d], wr = rawd[d + 1];
#pragma unroll
      for (int b = 0; b < 4; b++) {
        const int j = 4 * d + b - m;
        const int v = (int)((w >> (8 * b)) & 255u);
        const int vp = (int)(b ? (w >> (8 * (b - 1))) & 255u : wl >> 24);
        const int vn = (int)(b < 3 ? (w >> (8 * (b + 1))) & 255u : wr & 255u);
        bool ok = j >= lo_bin && j < hi_bin && v >= z_min;  // (0 <= lo_bin, hi_bin <= cols: a bin of the row)
        if (sep > 0) ok = ok && (j == 0 || v > vp) && (j == cols - 1 || v >= vn);
        mask |= (unsigned)ok << b;
      }
    }
    // ascending bins = lanes ascending, bytes ascending inside a lane
    unsigned before = 0, total = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) {
      const unsigned long long bal = __ballot((mask >> b) & 1u);
      before += lanes_below(bal);
      total += (unsigned)__popcll(bal);
    }
    unsigned pos = n_list + before;
#pragma unroll
    for (int b = 0; b < 4; b++)
      if ((mask >> b) & 1u) list[pos++] = (uint16_t)(4 * d + b - m);
    n_list += total;
  }
  __syncthreads();

  // ---- 3. the rest of the window (bins 2 .. sep away), the list compacted in place ----
  // (round r reads entries 64 r .. 64 r + 63 before its ballot and writes below 64 r + 64: no entry is overwritten unread)
  const unsigned char *bin = raw + m;
  if (sep > 1) {
    unsigned n_keep = 0;
    for (unsigned i0 = 0; i0 < n_list; i0 += 64) {
      const unsigned i = i0 + lane;
      bool ok = i < n_list;
      int j = 0;
      if (ok) {
        j = list[i];
        const int v = bin[j];
        const int nl = j < sep ? j : sep, nr = cols - 1 - j < sep ? cols - 1 - j : sep;
        int left = -1, right = -1;
        for (int e = 2; e <= nl; e++) left = max(left, (int)bin[j - e]);
        for (int e = 2; e <= nr; e++) right = max(right, (int)bin[j + e]);
        ok = v > left && v >= right;
      }
      const unsigned long long bal = __ballot(ok);
      if (ok) list[n_keep + lanes_below(bal)] = (uint16_t)j;
      n_keep += (unsigned)__popcll(bal);
    }
    n_list = n_keep;
    __syncthreads();
  }

  // ---- 4. the k strongest candidates ----
  uint16_t *kp = row_kp + ((int64_t)img * rows + a) * k;
  int t = -1;           // threshold power: everything above it is kept
  unsigned n_ties = 0;  // ... and the nearest n_ties candidates AT it
  if (n_list > (unsigned)k) {
#pragma unroll
    for (int b = lane; b < 256; b += 64) hist[b] = 0u;
    __syncthreads();
    for (unsigned i = lane; i < n_list; i += 64) atomicAdd(&hist[bin[list[i]]], 1u);
    __syncthreads();
    // lane l: powers 4 l .. 4 l + 3; G(p) = candidates of power >= p; t = the largest p with G(p) >= k
    const uint4 h = reinterpret_cast<const uint4 *>(hist)[lane];
    const unsigned own = h.x + h.y + h.z + h.w;
    unsigned incl = own;  // own + the lanes above
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned up = (unsigned)__shfl_down((int)incl, o);
      if (lane + o < 64) incl += up;
    }
    const unsigned above_lane = incl - own;
    const bool here = above_lane < (unsigned)k && incl >= (unsigned)k;  // exactly one lane: G(0) = n_list > k >= 1
    int tl = 0;
    unsigned al = 0;
    if (here) {
      const unsigned hv[4] = {h.x, h.y, h.z, h.w};
      unsigned g = above_lane;
#pragma unroll
      for (int b = 3; b >= 0; b--) {
        if (g < (unsigned)k && g + hv[b] >= (unsigned)k) {
          tl = 4 * lane + b;
          al = g;
        }
        g += hv[b];
      }
    }
    const int src = __builtin_ctzll(__ballot(here));
    t = __shfl(tl, src);
    n_ties = (unsigned)k - (unsigned)__shfl((int)al, src);
  }
  unsigned n_out = 0, ties_seen = 0;
  for (unsigned i0 = 0; i0 < n_list; i0 += 64) {
    const unsigned i = i0 + lane;
    int j = 0, v = -2;
    if (i < n_list) {
      j = list[i];
      v = bin[j];
    }
    const unsigned long long tie_bal = __ballot(v == t);
    const bool keep = v > t || (v == t && ties_seen + lanes_below(tie_bal) < n_ties);
    const unsigned long long bal = __ballot(keep);
    if (keep) kp[n_out + lanes_below(bal)] = (uint16_t)j;  // (n_out + ... < min(n_list, k))
    n_out += (unsigned)__popcll(bal);
    ties_seen += (unsigned)__popcll(tie_bal);
  }
  if (lane == 0) row_n[(int64_t)img * rows + a] = n_out;
}

}  // namespace

struct rsx_kstrongest : rsx::KeypointHandle {
  rsx::DevBuf row_kp, row_n;
};

using rsx::fail;

int rsx::kstrongest_check_params(const rsx_kstrongest_params &p) {
  if (p.k < 1 || p.k > MAX_K) return fail(RSX_ERR_BAD_ARG, "k %d outside [1, %d]", p.k, MAX_K);
  if (p.z_min < 0 || p.z_min > 255) return fail(RSX_ERR_BAD_ARG, "z_min %d outside [0, 255]", p.z_min);
  if (p.min_range < 0) return fail(RSX_ERR_BAD_ARG, "min_range %d < 0", p.min_range);
  if (p.max_range < 0) return fail(RSX_ERR_BAD_ARG, "max_range %d < 0", p.max_range);
  if (p.min_separation < 0 || p.min_separation > MAX_SEP) return fail(RSX_ERR_BAD_ARG, "min_separation %d outside [0, %d]", p.min_separation, MAX_SEP);
  return RSX_OK;
}

namespace {

// the resolve step of the scaffold (keypoints_host.h): the defaults, *params over them, the check
int get_params(const rsx_kstrongest_params *params, rsx_kstrongest_params *p) {
  rsx_kstrongest_default_params(p);
  if (params) *p = *params;
  return rsx::kstrongest_check_params(*p);
}

// d_imgs: nb device images img_stride bytes apart -> d_targets [nb][max_targets][2], d_xy (optional, needs d_az), d_counts
// (optional).  Two launches per sub-batch (rsx::rows_then_pack; row_cap = k), nothing read on the host.
int extract_device(rsx_kstrongest *h, const uint8_t *d_imgs, int64_t img_stride, int nb, int32_t stride, int32_t off, const rsx_kstrongest_params &p,
                   const float *d_az, int64_t az_stride, float resolution, int32_t max_targets, int *d_targets, float *d_xy, int *d_counts,
                   hipStream_t s) {
  const int rows = h->rows, cols = h->cols;
  const int lo = p.min_range < cols ? p.min_range : cols, hi = p.max_range == 0 || p.max_range > cols ? cols : p.max_range;
  const size_t lds = ks_lds_bytes(cols, p.min_separation);
  return rsx::rows_then_pack(h, p.k, nb, d_az, az_stride, resolution, max_targets, d_targets, d_xy, d_counts, s, [&](int b0, int n) {
    hipLaunchKernelGGL(ks_rows, dim3((unsigned)rows, (unsigned)n), dim3(64), lds, s, d_imgs + (int64_t)b0 * img_stride, img_stride, rows, cols, stride, off,
                       p.k, p.z_min, lo, hi, p.min_separation, h->row_kp.as<uint16_t>(), h->row_n.as<unsigned>());
  });
}

}  // namespace

extern "C" {

int rsx_kstrongest_default_params(rsx_kstrongest_params *p) try {
  if (!p) return fail(RSX_ERR_BAD_ARG, "null params");
  p->k = 12;  // CFEAR radar odometry: k = 12, z_min = 60
  p->z_min = 60;
  p->min_range = 58;  // as the other extractors
  p->max_range = 0;
  p->min_separation = 5;  // include/rsx.h: why not CFEAR's plain rule
  p->reserved = 0;
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_kstrongest_create(int device, int32_t rows, int32_t cols, rsx_kstrongest **out) try {
  return rsx::keypoints_create(rows >= 1 && rows <= MAX_ROWS && cols >= 1 && cols <= MAX_COLS, device, rows, cols, out);
} RSX_CATCH_ALL

int rsx_kstrongest_destroy(rsx_kstrongest *h) try {
  return rsx::keypoints_destroy(h);
} RSX_CATCH_ALL

int rsx_kstrongest_extract_batch_device(rsx_kstrongest *h, const uint8_t *d_imgs, int32_t n_images, int64_t image_stride_bytes, int32_t row_stride,
                                        int32_t col_offset, const rsx_kstrongest_params *params, const float *d_azimuths,
                                        int32_t azimuths_per_image, float resolution, int32_t *d_targets, float *d_xy, int32_t max_targets,
                                        int32_t *d_counts, void *stream) try {
  return rsx::keypoints_extract_batch_device(h, get_params, extract_device, d_imgs, n_images, image_stride_bytes, row_stride, col_offset, params,
                                             d_azimuths, azimuths_per_image, resolution, d_targets, d_xy, max_targets, d_counts, stream);
} RSX_CATCH_ALL

int rsx_kstrongest_extract_batch(rsx_kstrongest *h, const uint8_t *imgs, int32_t n_images, int64_t image_stride_bytes, int32_t row_stride,
                                 int32_t col_offset, const rsx_kstrongest_params *params, const float *azimuths, int32_t azimuths_per_image,
                                 float resolution, int32_t *out_targets, float *out_xy, int32_t max_targets, int32_t *out_counts) try {
  return rsx::keypoints_extract_batch(h, get_params, extract_device, imgs, n_images, image_stride_bytes, row_stride, col_offset, params, azimuths,
                                      azimuths_per_image, resolution, out_targets, out_xy, max_targets, out_counts);
} RSX_CATCH_ALL

int rsx_kstrongest_extract(rsx_kstrongest *h, const uint8_t *img, int32_t row_stride, int32_t col_offset, const rsx_kstrongest_params *params,
                           const float *azimuths, float resolution, int32_t *out_targets, float *out_xy, int32_t max_targets,
                           int32_t *out_count) try {
  return rsx::keypoints_extract(h, get_params, extract_device, img, row_stride, col_offset, params, azimuths, resolution, out_targets, out_xy,
                                max_targets, out_count);
} RSX_CATCH_ALL

}  // extern "C"
