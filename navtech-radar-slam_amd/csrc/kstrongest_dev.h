// kstrongest_dev.h -- the row kernel body that k-strongest (kstrongest.hip) and CFAR (cfar.hip) share: the row's bytes into LDS,
// the screen, the separation window and the histogram select of the k strongest candidates.  The two extractors differ in one
// thing, the DETECTION of a bin, which is a compile-time policy `Det`:
//   Det::floor()            the least power a detection can have (wave-uniform): part of the screen of every bin
//   Det::kLocal             false: the floor is the whole detection (k-strongest) and step 2b below is not compiled;
//                           true: every survivor of the screen, one per lane, is also asked
//   Det::detect(raw, m, j, cols)   bin j's own verdict from the row in LDS (bin i at raw[m + i], 0 <= i < cols; the bytes of
//                           the row's 16-byte pieces outside the row are NOT the row's and must not count)
//                           before the rest of the separation window and the select run.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rsx {
namespace ks {

constexpr int MAX_COLS = 8192;  // LDS of a row: 1024 + 32 + 16 ((cols + 30) / 16) + 2 cols <= 26 KB
constexpr int MAX_ROWS = 4096;
constexpr int MAX_K = 128;
constexpr int MAX_SEP = 32;
constexpr int LOADS = 4;  // 16-byte loads per lane in flight: a 3360-bin row is one round of them

// LDS of one wavefront (dynamic): hist[256] u32 | 16 bytes | the row's 16-byte pieces | 16 bytes | list[cap] u16
__host__ __device__ inline int pieces(int cols) { return (cols + 30) / 16; }  // a row that starts 15 bytes into its first piece
__host__ __device__ inline int list_cap(int cols, int sep) { return sep > 0 ? (cols + 1) / 2 : cols; }  // (no two adjacent survivors)
__host__ __device__ inline size_t lds_bytes(int cols, int sep) {
  return 1024 + 32 + 16 * (size_t)pieces(cols) + 2 * (size_t)((list_cap(cols, sep) + 7) & ~7);
}

__device__ __forceinline__ unsigned lanes_below(unsigned long long m) {  // set bits of m in the lanes below this one
  return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// k-strongest's detection: the fixed power floor and nothing else
struct Floor {
  static constexpr bool kLocal = false;
  int z_min;
  __device__ __forceinline__ int floor() const { return z_min; }
};

// one wavefront per (azimuth blockIdx.x, image blockIdx.y); the kernel's dynamic LDS: lds_bytes(cols, sep)
template <class Det>
__device__ __forceinline__ void row(const uint8_t *__restrict__ imgs, int64_t img_stride, int rows, int cols, int stride, int off,
                                    int k, const Det &det, int lo_bin, int hi_bin, int sep, uint16_t *__restrict__ row_kp,
                                    unsigned *__restrict__ row_n) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ks_lds[];
  unsigned *hist = reinterpret_cast<unsigned *>(ks_lds);
  unsigned char *raw = ks_lds + 1024 + 16;  // piece c of the row at raw + 16 c; 16 spare bytes in front and behind
  const int npieces_max = pieces(cols);
  uint16_t *list = reinterpret_cast<uint16_t *>(raw + 16 * (size_t)npieces_max + 16);
  const int lane = threadIdx.x, a = blockIdx.x, img = blockIdx.y;
  const int z_min = det.floor();

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

  // ---- 2b. a detection that looks around the bin: one survivor per lane, the list compacted in place (as in step 3) ----
  if constexpr (Det::kLocal) {
    unsigned n_keep = 0;
    for (unsigned i0 = 0; i0 < n_list; i0 += 64) {
      const unsigned i = i0 + lane;
      bool ok = i < n_list;
      int j = 0;
      if (ok) {
        j = list[i];
        ok = det.detect(raw, m, j, cols);
      }
      const unsigned long long bal = __ballot(ok);
      if (ok) list[n_keep + lanes_below(bal)] = (uint16_t)j;
      n_keep += (unsigned)__popcll(bal);
    }
    n_list = n_keep;
    __syncthreads();
  }

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

}  // namespace ks
}  // namespace rsx
