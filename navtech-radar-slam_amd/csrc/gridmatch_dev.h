// gridmatch_dev.h -- the device code that gridmatch.hip (exhaustive correlative matching) and gridsearch.hip (the wide-window search
// pruned by bounds) share: steps 1 - 5 of the rule of include/rsx.h for one point, the slot walk over a framed byte plane, the slot
// and part scheme that deals it to a workgroup, the workgroup maximum, and the counts and the transform of a record's winner; and,
// with gridrefine.hip as well, the ragged job convention and the status of a skipped job.  Everything here is integers from the
// cell on.  No fp64 expression here may be fused or re-associated (the Makefile's -ffp-contract=off covers a header too).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rsx.h"

namespace rsx {
namespace gridmatch_dev {

constexpr int NT = 256;
constexpr int FLUSH = 256;  // 256 * 255 < 2^16: points between two flushes of the 16-bit sums
constexpr int DEPTH = 8;    // reads of the plane a thread keeps in flight
constexpr int PLACE = 64;   // how far outside the map a point is still placed (cells)
static_assert(FLUSH * 255 < 65536, "");

// cos and sin of the rotations -K .. K of `step` rad (filled on the host, handed to a kernel by value)
template <int MAX_K>
struct Rotations {
  float c[2 * MAX_K + 1], s[2 * MAX_K + 1];  // [k + K]
  Rotations(int K, double step) : c{}, s{} {
    for (int k = -K; k <= K; k++) c[k + K] = (float)std::cos((double)k * step), s[k + K] = (float)std::sin((double)k * step);  // fp64, rounded once
  }
};

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

// the status bits of a job that is skipped (0: it is not): priors t that are not finite, more than the cap of points
__device__ __forceinline__ int skip_status(const double *t, int64_t n64) {
  return (finite6(t) ? 0 : RSX_GRIDMAP_MATCH_STATUS_TRANSFORM) | (n64 > RSX_GRIDMAP_MATCH_MAX_POINTS ? RSX_GRIDMAP_MATCH_STATUS_POINTS : 0);
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

// The slot and part scheme: the sums over the n cells of every slot of `rows` rows of `cols` columns, a slot being four neighbouring
// columns of a row whose bytes lie at shift(row, group) from a point's cell; emit(row, column, sum) is called once per column, by
// the thread that owns its slot.  With S slots and P = max(1, 256 / S), the points are dealt to P parts and thread part S + slot
// walks its part; the parts are added through red (4 NT words); with S above 256 a thread walks several slots in turn.
// (workgroup-uniform: every thread calls it; the cells are in LDS and a barrier has passed)
template <typename Shift, typename Emit>
__device__ __forceinline__ void slot_sums(const uint8_t *__restrict__ plane, const unsigned *cell, unsigned *red, int n, int rows, int cols, Shift shift,
                                          Emit emit) {
  const int tid = threadIdx.x;
  const int groups = (cols + 3) >> 2, slots = rows * groups;
  const int parts = slots < NT ? NT / slots : 1;
  if (parts > 1) {  // (workgroup-uniform) every slot has a thread in each part
    unsigned sum[4] = {0u, 0u, 0u, 0u};
    const int part = tid / slots, slot = tid - part * slots;
    const int row = slot / groups, gi = slot - row * groups;
    if (part < parts) walk(plane, cell, n, part, parts, shift(row, gi), sum);
#pragma unroll
    for (int j = 0; j < 4; j++) red[4 * tid + j] = sum[j];
    __syncthreads();
    if (tid < slots) {
      for (int q = 1; q < parts; q++)
#pragma unroll
        for (int j = 0; j < 4; j++) sum[j] += red[4 * (tid + q * slots) + j];
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (4 * gi + j < cols) emit(row, 4 * gi + j, sum[j]);
    }
  } else {
    for (int slot = tid; slot < slots; slot += NT) {
      unsigned sum[4] = {0u, 0u, 0u, 0u};
      const int row = slot / groups, gi = slot - row * groups;
      walk(plane, cell, n, 0, 1, shift(row, gi), sum);
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (4 * gi + j < cols) emit(row, 4 * gi + j, sum[j]);
    }
  }
}

// the counts of a record at rotation (c, s) and shift (bu, bv): the points of the job that are placed, and those of them whose
// shifted cell is in the map, added to the LDS words n_placed and n_inside (zeroed, and a barrier passed, before)
__device__ __forceinline__ void count_at(const MatchGeo &g, int margin, const float *__restrict__ xy, int64_t stride, int64_t first, int n, const double *t6,
                                         double c, double s, int bu, int bv, unsigned *n_placed, unsigned *n_inside) {
  unsigned placed = 0u, inside = 0u;
  for (int i = threadIdx.x; i < n; i += NT) {
    const float *p = xy + (first + i) * stride;
    int ix, iy;
    if (place(g, margin, t6, c, s, (double)p[0], (double)p[1], &ix, &iy)) {
      placed++;
      inside += (ix + bu >= 0 && ix + bu < g.W && iy + bv >= 0 && iy + bv < g.H) ? 1u : 0u;
    }
  }
  atomicAdd(n_placed, placed);  // (LDS)
  atomicAdd(n_inside, inside);
}

// the transform of a record: the prior t6 behind the rotation (c, s), shifted by (bu, bv) cells; the prior itself when nothing was found
__device__ __forceinline__ void winner_transform(double *out, bool found, const double *t6, double c, double s, int bu, int bv, double res) {
  if (!found) {
    for (int q = 0; q < 6; q++) out[q] = t6[q];
  } else {
    out[0] = t6[0] * c + t6[1] * s;
    out[1] = t6[1] * c - t6[0] * s;
    out[2] = t6[2] + (double)bu * res;
    out[3] = t6[3] * c + t6[4] * s;
    out[4] = t6[4] * c - t6[3] * s;
    out[5] = t6[5] + (double)bv * res;
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
