// gridmatch_dev.h -- the device code that gridmatch.hip (exhaustive correlative matching) and gridsearch.hip (the wide-window search
// pruned by bounds) share: steps 1 - 5 of the rule of include/rsx.h for one point, the ragged job convention, the slot walk over a
// framed byte plane and the workgroup maximum.  Everything here is integers from the cell on.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rsx {
namespace gridmatch_dev {

constexpr int NT = 256;
constexpr int FLUSH = 256;  // 256 * 255 < 2^16: points between two flushes of the 16-bit sums
constexpr int DEPTH = 8;    // reads of the plane a thread keeps in flight
static_assert(FLUSH * 255 < 65536, "");

struct MatchGeo {
  double ox, oy, inv_res, res;
  int W, H, K, U, V;
  unsigned pitch;  // of the framed plane
};

__device__ __forceinline__ bool finite6(const double *t) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 6; k++) ok = ok && ((__double_as_longlong(t[k]) & 0x7ff0000000000000ll) != 0x7ff0000000000000ll);
  return ok;
}

// steps 1 - 5 of the rule for one point: false when it is not placed (margin: how far outside the map a point is still placed, cells)
__device__ __forceinline__ bool place(const MatchGeo &g, int margin, const double *t, double c, double s, double x, double y, int *ix, int *iy) {
  const double rx = c * x - s * y, ry = s * x + c * y;
  const double mx = t[0] * rx + t[1] * ry + t[2], my = t[3] * rx + t[4] * ry + t[5];
  const double fx = (mx - g.ox) * g.inv_res, fy = (my - g.oy) * g.inv_res;
  if (!(fx >= -(double)margin && fx < (double)(g.W + margin) && fy >= -(double)margin && fy < (double)(g.H + margin))) return false;
  *ix = (int)floor(fx);
  *iy = (int)floor(fy);
  return true;
}

// the points of a job; n < 0 (offsets that decrease: the device entry trusts them, the kernel reads nothing through them) is 0
__device__ __forceinline__ int64_t job_points(const int64_t *offsets, int job, int64_t *first) {
  const int64_t a = offsets[job], n = offsets[job + 1] - a;
  *first = a;
  return n < 0 ? 0 : n;
}

// thread-owned slot (four neighbouring bytes from `shift`): walks points part, part + parts, ... of cell[0 .. n) and adds the four
// bytes of each to sum
__device__ __forceinline__ void walk(const uint8_t *__restrict__ plane, const unsigned *cell, int n, int part, int parts, unsigned shift,
                                     unsigned sum[4]) {
  const int mine = part < n ? (n - part + parts - 1) / parts : 0;  // points of this part
  for (int done = 0; done < mine; done += FLUSH) {
    const int m = mine - done < FLUSH ? mine - done : FLUSH;
    const unsigned *c = cell + part + done * parts;
    unsigned lo = 0u, hi = 0u;  // bytes 0 and 2, bytes 1 and 3, as two 16-bit sums each
    int q = 0;
    for (; q + DEPTH <= m; q += DEPTH) {  // DEPTH reads in flight: nothing in the loop depends on a read but the sums
      unsigned w[DEPTH];
#pragma unroll
      for (int e = 0; e < DEPTH; e++) __builtin_memcpy(&w[e], plane + (c[(q + e) * parts] + shift), 4);
#pragma unroll
      for (int e = 0; e < DEPTH; e++) lo += w[e] & 0x00ff00ffu, hi += (w[e] >> 8) & 0x00ff00ffu;
    }
    for (; q < m; q++) {
      unsigned w;
      __builtin_memcpy(&w, plane + (c[q * parts] + shift), 4);
      lo += w & 0x00ff00ffu, hi += (w >> 8) & 0x00ff00ffu;
    }
    sum[0] += lo & 0xffffu, sum[1] += hi & 0xffffu, sum[2] += lo >> 16, sum[3] += hi >> 16;
  }
}

// the maximum of v over the workgroup (every thread gets it); scratch: NT entries
template <typename T>
__device__ __forceinline__ T block_max(T v, T *scratch) {
  const int tid = threadIdx.x;
  __syncthreads();  // (the scratch may still be read from the call before)
  scratch[tid] = v;
  __syncthreads();
  for (int h = NT / 2; h > 0; h >>= 1) {
    if (tid < h) scratch[tid] = scratch[tid] > scratch[tid + h] ? scratch[tid] : scratch[tid + h];
    __syncthreads();
  }
  return scratch[0];
}

}  // namespace gridmatch_dev
}  // namespace rsx
