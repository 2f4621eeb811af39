// gridmatch_dev.h -- the device code that gridmatch.hip (exhaustive correlative matching) and gridsearch.hip (the wide-window search
// pruned by bounds) share: steps 1 - 5 of the rule of include/rsx.h for one point, the slot walk over a framed byte plane, the slot
// and part scheme that deals it to a workgroup, the workgroup maximum, and the pick of a record from its score volume (which
// gridtrack.hip, the one-launch tracker, runs on a volume in LDS); and, with gridrefine_dev.h as well, the ragged job convention and
// the status of a skipped job.  Everything here is integers from the cell on.  No fp64 expression here may be fused or re-associated (the Makefile's -ffp-contract=off covers a header too).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

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

// the LDS words of pick_record
struct PickLds {
  unsigned long long keys[NT];
  unsigned seconds[NT];
  unsigned n_placed, n_inside;
};

// The record of one job from its score volume vol[(2K + 1)(2V + 1)(2U + 1)] (global memory or LDS, written before a barrier that
// the caller has passed): the winner by a 64-bit key that carries the tie order and the linear index, the runner-up and, from steps
// 1 - 5 again at the winner's k, the counts.  A skipped job (skip_status) gives a zero record but for the status and reads nothing.
// Called by the whole workgroup; every thread returns the same record.  Tab: a Rotations<>
template <typename Tab>
__device__ __forceinline__ rsx_gridmap_match_result pick_record(const float *__restrict__ xy, int64_t stride, int64_t first, int64_t n64, const double *t,
                                                                const Tab &tab, const MatchGeo &g, const unsigned *vol, PickLds *lds) {
  const int tid = threadIdx.x;
  const int nk = 2 * g.K + 1, nv = 2 * g.V + 1, nu = 2 * g.U + 1, total = nk * nv * nu;
  rsx_gridmap_match_result r;
  memset(&r, 0, sizeof(r));
  const int skipped = skip_status(t, n64);
  if (skipped) {  // (workgroup-uniform)
    r.status = skipped;
    return r;
  }
  // ---- the winner: score, then the smallest |k|, then the smallest u u + v v, then the smallest linear index ----
  // score < 2^21 | 127 - |k| < 2^7 | 4095 - (u u + v v) < 2^12 | 2^20 - 1 - index < 2^20
  unsigned long long key = 0ull;
  for (int i = tid; i < total; i += NT) {
    const int ui = i % nu, vi = (i / nu) % nv, ki = i / (nu * nv);
    const int k = ki - g.K, v = vi - g.V, u = ui - g.U;
    const unsigned long long cand = ((unsigned long long)vol[i] << 39) | ((unsigned long long)(127 - (k < 0 ? -k : k)) << 32) |
                                    ((unsigned long long)(4095 - (u * u + v * v)) << 20) | (unsigned long long)(0xfffff - i);
    key = cand > key ? cand : key;
  }
  key = block_max(key, lds->keys);
  const int best = 0xfffff - (int)(key & 0xfffffull);
  const int bu = best % nu - g.U, bv = (best / nu) % nv - g.V, bk = best / (nu * nv) - g.K;
  // ---- the runner-up: the best score farther than 1 from the winner in k, u or v ----
  unsigned second = 0u;
  for (int i = tid; i < total; i += NT) {
    const int du = i % nu - g.U - bu, dv = (i / nu) % nv - g.V - bv, dk = i / (nu * nv) - g.K - bk;
    const bool far = du > 1 || du < -1 || dv > 1 || dv < -1 || dk > 1 || dk < -1;
    second = far && vol[i] > second ? vol[i] : second;
  }
  second = block_max(second, lds->seconds);
  // ---- the counts at the winner ----
  if (tid == 0) lds->n_placed = 0u, lds->n_inside = 0u;
  __syncthreads();
  const double c = (double)tab.c[bk + g.K], s = (double)tab.s[bk + g.K];
  const double t6[6] = {t[0], t[1], t[2], t[3], t[4], t[5]};
  count_at(g, PLACE, xy, stride, first, (int)n64, t6, c, s, bu, bv, &lds->n_placed, &lds->n_inside);
  __syncthreads();
  r.score = (unsigned)(key >> 39);
  r.score_prior = vol[(g.K * nv + g.V) * nu + g.U];
  r.score_runner_up = second;
  r.k = bk, r.u = bu, r.v = bv;
  r.n_points = (int)lds->n_placed, r.n_inside = (int)lds->n_inside;
  if (r.score == 0u) r.status = RSX_GRIDMAP_MATCH_STATUS_EMPTY;
  winner_transform(r.transform, r.score != 0u, t6, c, s, bu, bv, g.res);
  return r;
}

// the cells of one rotation (c, s) of a job's n points into LDS: the byte offset of a placed point's cell in the framed plane (frame:
// its margin in cells), cell (-PLACE, -PLACE) for a point that is not placed, from which no candidate reaches the map.  The caller
// passes a barrier before it reads them
__device__ __forceinline__ void fill_cells(const MatchGeo &g, int frame, const float *__restrict__ xy, int64_t stride, int64_t first, int n, const double *t6,
                                           double c, double s, unsigned *cell) {
  const unsigned nowhere = (unsigned)(frame - PLACE) * g.pitch + (unsigned)(frame - PLACE);
  for (int i = threadIdx.x; i < n; i += NT) {
    const float *p = xy + (first + i) * stride;
    int ix, iy;
    cell[i] = place(g, PLACE, t6, c, s, (double)p[0], (double)p[1], &ix, &iy) ? (unsigned)(iy + frame) * g.pitch + (unsigned)(ix + frame) : nowhere;
  }
}

}  // namespace gridmatch_dev
}  // namespace rsx
