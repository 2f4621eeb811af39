// gridsearch.hip -- localising a point cloud in the radar grid map over a WIDE window on gfx950 (rotations -K .. K <= 180, whole-cell
// shifts up to 256 cells): the exhaustive rule of gridmatch.hip, pruned by bounds in two levels, exact.  None of this is in the
// reference checkout: the rule is the one stated in include/rsx.h and restated in tests/gridsearch_np.py (PARITY UNPINNED): fp64 on
// plain operations up to the cell of a point, integers from there on, so bounds and records are the restatement's byte for byte
// whatever the order of the sums.
//
// rsx_gridmap_search_prepare snapshots the likelihood plane into two buffers of the search's own, both over the same frame of M
// cells (a multiple of 8) around the map: F, the plane itself in zeros, and Pd, the 8 x 8 pooled plane P[y][x] = max L[y .. y + 7][x .. x + 7]
// de-interleaved by phase, Pd[y mod 8][x mod 8][y / 8][x / 8] (frame coordinates), so that the blocks bu, bu + 1, ... of one point
// are neighbouring bytes and walk's one unaligned 32-bit read serves four of them.  M >= max(64, max_cells) + max_cells + 32: a
// placed point's cell is at most PL outside the map, a shift at most max_cells + 7 (a block is scored whole, its candidates outside
// the window are dropped afterwards), a read four bytes wide -- no read leaves a buffer and no inner loop tests a bound.  A point that
// is not placed is given the cell (-(max_cells + 32), ...), from which no candidate and no block reaches a byte that is not 0.
// Three launches per call whatever the batch, no atomics on device memory:
//   gms_bound   one workgroup per (job, k).  Cells of the rotated cloud into LDS as offsets into Pd; bounds of every block with the
//               slot and part scheme of gmm_score (slot_sums); the best block by an index-carrying maximum; cells again as offsets into F; that
//               block's <= 64 candidates exactly (8 v x 2 groups of four u = 16 slots x 16 parts of points): seed(k).  The
//               workgroup of k = 0 also writes score(0, 0, 0).
//   gms_refine  one workgroup per (job, k).  T0 from the 2K + 1 seeds; cells; a pass over its bounds that lists the blocks reaching
//               max(T0, 1), in ascending order; each listed block exactly, unless an exact score found meanwhile already exceeds its bound (it is still
//               counted: n_refined is the rule's): sixteen blocks at a time with a thread per slot while the list is long (bounds that
//               do not prune then cost what gmm_score costs), a block at a time with 16 parts per slot for the rest; its best key by
//               the tie order and its count.
//   gms_pick    one workgroup per job: the winner over the 2K + 1 keys by a two-word comparison that carries the whole tie order,
//               bound_runner_up from the bounds, the counts at the winner's k; thread 0 writes the record.
// The two batch entries are the scaffold of gridloc_host.h behind their own rules.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>

#include "gridloc_host.h"
#include "gridmap.h"
#include "gridmatch_dev.h"

#pragma STDC FP_CONTRACT OFF

namespace {

using rsx::fail;
using namespace rsx::gridmatch_dev;  // NT, MatchGeo, Rotations, place, job_points, skip_status, walk, slot_sums, count_at, winner_transform, block_max
namespace gridloc = rsx::gridloc;

constexpr int MAX_POINTS = RSX_GRIDMAP_MATCH_MAX_POINTS;
constexpr int MAX_K = RSX_GRIDMAP_SEARCH_MAX_ANGLE_STEPS, MAX_UV = RSX_GRIDMAP_SEARCH_MAX_CELLS;
constexpr int MAX_BLOCKS = ((2 * MAX_UV + 1 + 7) / 8) * ((2 * MAX_UV + 1 + 7) / 8);  // of one k: 65 x 65
constexpr int TILE = 32;                                                             // gms_prepare: cells of a tile's side
static_assert(MAX_BLOCKS <= 65536, "the refine list holds block indices in 16 bits");

using Tables = Rotations<MAX_K>;
static_assert(sizeof(Tables) == 2888, "");

struct SearchGeo {
  MatchGeo g;   // g.pitch: of F, 8 cw
  int M;        // the frame: cells on every side of the map
  int cw, ch;   // coarse columns and rows of the frame
  int PL;       // max(64, U, V): how far outside the map a point is still placed
  int nbu, nbv;
  int nowhere;  // the coordinate (x and y) of a point that is not placed
  unsigned min_score;
};

// key of a candidate within one k: score < 2^21 | 2^18 - 1 - (u u + v v) | 2^19 - 1 - ((v + V)(2U + 1) + u + U)
__device__ __forceinline__ unsigned long long key_of(unsigned score, int u, int v, int local) {
  return ((unsigned long long)score << 37) | ((unsigned long long)(0x3ffff - (u * u + v * v)) << 19) | (unsigned long long)(0x7ffff - local);
}

// the tie order across k: score, then the smallest |k|, then the smallest u u + v v, then the smallest linear index
struct WideKey {
  unsigned long long hi, lo;  // score << 8 | 255 - |k| ; 2^18 - 1 - r2 << 27 | 2^27 - 1 - index
};

// b replaces a when it is later in the order (plain words: a select between two structs would go through scratch memory)
__device__ __forceinline__ void wide_max(unsigned long long &a_hi, unsigned long long &a_lo, unsigned long long b_hi, unsigned long long b_lo) {
  const bool later = b_hi > a_hi || (b_hi == a_hi && b_lo > a_lo);
  a_hi = later ? b_hi : a_hi;
  a_lo = later ? b_lo : a_lo;
}

// block_max for a WideKey; scratch: two arrays of NT entries
__device__ __forceinline__ WideKey block_wide_max(unsigned long long v_hi, unsigned long long v_lo, unsigned long long *hi, unsigned long long *lo) {
  const int tid = threadIdx.x;
  __syncthreads();
  hi[tid] = v_hi, lo[tid] = v_lo;
  __syncthreads();
  for (int h = NT / 2; h > 0; h >>= 1) {
    if (tid < h) {
      wide_max(v_hi, v_lo, hi[tid + h], lo[tid + h]);
      hi[tid] = v_hi, lo[tid] = v_lo;
    }
    __syncthreads();
  }
  return WideKey{hi[0], lo[0]};
}

// cells of the rotated cloud into LDS: offsets into Pd of the block (0, 0) of each point (pooled), or into F of its cell
template <bool POOLED>
__device__ __forceinline__ void fill_cells(unsigned *cell, const float *__restrict__ xy, int64_t stride, int64_t first, int n, const SearchGeo &sg,
                                           const double *t6, double c, double s) {
  for (int i = threadIdx.x; i < n; i += NT) {
    const float *p = xy + (first + i) * stride;
    int ix, iy;
    if (!place(sg.g, sg.PL, t6, c, s, (double)p[0], (double)p[1], &ix, &iy)) ix = iy = sg.nowhere;
    if (POOLED) {
      const unsigned x0 = (unsigned)(ix - sg.g.U + sg.M), y0 = (unsigned)(iy - sg.g.V + sg.M);
      cell[i] = (((y0 & 7u) * 8u + (x0 & 7u)) * (unsigned)sg.ch + (y0 >> 3)) * (unsigned)sg.cw + (x0 >> 3);
    } else {
      cell[i] = (unsigned)(iy + sg.M) * sg.g.pitch + (unsigned)(ix + sg.M);
    }
  }
}

// the 64 candidates of block (bv, bu) exactly: thread tid < 16 leaves with the scores of v = -V + 8 bv + tid / 2 and the four u from
// -U + 8 bu + 4 (tid & 1) in sum (candidates outside the window included: the caller drops them)
__device__ __forceinline__ void score_block(const uint8_t *__restrict__ F, const unsigned *cell, int n, const MatchGeo &g, int bv, int bu, unsigned *red,
                                            unsigned sum[4]) {
  const int tid = threadIdx.x, part = tid >> 4, slot = tid & 15;
  const int v = -g.V + 8 * bv + (slot >> 1), u = -g.U + 8 * bu + 4 * (slot & 1);
  sum[0] = sum[1] = sum[2] = sum[3] = 0u;
  walk(F, cell, n, part, 16, (unsigned)(v * (int)g.pitch + u), sum);
  __syncthreads();  // (red may still be read from the block before)
#pragma unroll
  for (int j = 0; j < 4; j++) red[4 * tid + j] = sum[j];
  __syncthreads();
  if (tid < 16)
    for (int q = 1; q < 16; q++)
#pragma unroll
      for (int j = 0; j < 4; j++) sum[j] += red[4 * (tid + 16 * q) + j];
}

__global__ __launch_bounds__(NT) void gms_bound(const float *__restrict__ xy, int64_t stride, const int64_t *__restrict__ offsets,
                                                const double *__restrict__ priors, Tables tab, SearchGeo sg, const uint8_t *__restrict__ F,
                                                const uint8_t *__restrict__ Pd, unsigned *__restrict__ bounds, unsigned *__restrict__ seeds,
                                                unsigned *__restrict__ prior_scores) {
  __shared__ unsigned cell[MAX_POINTS];
  __shared__ unsigned red[NT * 4];
  __shared__ unsigned long long keys[NT];
  __shared__ unsigned small[16];
  __shared__ unsigned prior_sum;
  const MatchGeo &g = sg.g;
  const int tid = threadIdx.x;
  const int nk = 2 * g.K + 1, nb = sg.nbv * sg.nbu;
  const int job = (int)(blockIdx.x / (unsigned)nk), kk = (int)(blockIdx.x % (unsigned)nk);
  unsigned *out = bounds + ((int64_t)job * nk + kk) * nb;
  const double *t = priors + 6 * (int64_t)job;
  int64_t first;
  const int64_t n64 = job_points(offsets, job, &first);
  if (skip_status(t, n64)) {  // (workgroup-uniform) a skipped job: its bounds are 0
    for (int i = tid; i < nb; i += NT) out[i] = 0u;
    if (tid == 0) {
      seeds[(int64_t)job * nk + kk] = 0u;
      if (kk == g.K) prior_scores[job] = 0u;
    }
    return;
  }
  const int n = (int)n64;
  const double c = (double)tab.c[kk], s = (double)tab.s[kk];
  const double t6[6] = {t[0], t[1], t[2], t[3], t[4], t[5]};
  fill_cells<true>(cell, xy, stride, first, n, sg, t6, c, s);
  if (tid == 0) prior_sum = 0u;
  __syncthreads();
  // ---- the bounds of every block, and the best of them (bound << 32 | ~index: the highest bound, then the smallest index) ----
  unsigned long long best = 0ull;
  slot_sums(
      Pd, cell, red, n, sg.nbv, sg.nbu, [&](int bv, int gi) { return (unsigned)(bv * sg.cw + 4 * gi); },
      [&](int bv, int bu, unsigned sum) {
        const int idx = bv * sg.nbu + bu;
        out[idx] = sum;
        const unsigned long long cand = ((unsigned long long)sum << 32) | (unsigned long long)(0xffffffffu - (unsigned)idx);
        best = cand > best ? cand : best;
      });
  best = block_max(best, keys);  // (its barriers: every walk over the pooled cells has ended)
  const int bi = (int)(0xffffffffu - (unsigned)(best & 0xffffffffull));
  const int bv = bi / sg.nbu, bu = bi - bv * sg.nbu;
  // ---- the seed: that block's candidates exactly ----
  fill_cells<false>(cell, xy, stride, first, n, sg, t6, c, s);
  __syncthreads();
  unsigned sum[4];
  score_block(F, cell, n, g, bv, bu, red, sum);
  if (tid < 16) {
    const int v = -g.V + 8 * bv + (tid >> 1), u = -g.U + 8 * bu + 4 * (tid & 1);
    unsigned m = 0u;
#pragma unroll
    for (int j = 0; j < 4; j++) m = (v <= g.V && u + j <= g.U && sum[j] > m) ? sum[j] : m;
    small[tid] = m;
  }
  if (kk == g.K) {  // (workgroup-uniform) score(0, 0, 0)
    unsigned mine = 0u;
    for (int i = tid; i < n; i += NT) mine += F[cell[i]];
    atomicAdd(&prior_sum, mine);  // (LDS)
  }
  __syncthreads();
  if (tid == 0) {
    unsigned m = 0u;
    for (int q = 0; q < 16; q++) m = small[q] > m ? small[q] : m;
    seeds[(int64_t)job * nk + kk] = m;
    if (kk == g.K) prior_scores[job] = prior_sum;
  }
}

__global__ __launch_bounds__(NT) void gms_refine(const float *__restrict__ xy, int64_t stride, const int64_t *__restrict__ offsets,
                                                 const double *__restrict__ priors, Tables tab, SearchGeo sg, const uint8_t *__restrict__ F,
                                                 const unsigned *__restrict__ bounds, const unsigned *__restrict__ seeds,
                                                 const unsigned *__restrict__ prior_scores, unsigned long long *__restrict__ out_keys,
                                                 int *__restrict__ out_counts) {
  __shared__ unsigned cell[MAX_POINTS];
  __shared__ unsigned red[NT * 4];
  __shared__ unsigned long long keys[NT];
  __shared__ unsigned thr[NT];
  __shared__ unsigned short list[MAX_BLOCKS];
  __shared__ unsigned t_cur;
  const MatchGeo &g = sg.g;
  const int tid = threadIdx.x;
  const int nk = 2 * g.K + 1, nb = sg.nbv * sg.nbu, nu = 2 * g.U + 1;
  const int job = (int)(blockIdx.x / (unsigned)nk), kk = (int)(blockIdx.x % (unsigned)nk);
  const unsigned *bnd = bounds + ((int64_t)job * nk + kk) * nb;
  const double *t = priors + 6 * (int64_t)job;
  int64_t first;
  const int64_t n64 = job_points(offsets, job, &first);
  if (skip_status(t, n64)) {  // (workgroup-uniform) a skipped job
    if (tid == 0) out_keys[(int64_t)job * nk + kk] = 0ull, out_counts[(int64_t)job * nk + kk] = 0;
    return;
  }
  const int n = (int)n64;
  // ---- T0 = max(min_score, score(0, 0, 0), the seeds); a block is refined iff its bound >= max(T0, 1) ----
  unsigned t0 = sg.min_score > prior_scores[job] ? sg.min_score : prior_scores[job];
  for (int i = tid; i < nk; i += NT) {
    const unsigned sd = seeds[(int64_t)job * nk + i];
    t0 = sd > t0 ? sd : t0;
  }
  t0 = block_max(t0, thr);
  t0 = t0 > 1u ? t0 : 1u;
  const unsigned floor_score = sg.min_score > 1u ? sg.min_score : 1u;  // what a winner must reach
  if (tid == 0) t_cur = t0;
  __syncthreads();  // (thr is free again)
  // the list in ascending block order, so that neighbours in the list are neighbours in the plane: every thread counts the blocks of
  // its stretch that reach t0, an inclusive scan over the workgroup, then it writes them
  const int per = (nb + NT - 1) / NT, lo = tid * per, hi = lo + per < nb ? lo + per : nb;
  unsigned mine = 0u;
  for (int i = lo; i < hi; i++) mine += bnd[i] >= t0 ? 1u : 0u;
  thr[tid] = mine;
  __syncthreads();
  for (int d = 1; d < NT; d <<= 1) {
    const unsigned add = tid >= d ? thr[tid - d] : 0u;
    __syncthreads();
    thr[tid] += add;
    __syncthreads();
  }
  unsigned at = thr[tid] - mine;
  for (int i = lo; i < hi; i++)
    if (bnd[i] >= t0) list[at++] = (unsigned short)i;
  const double c = (double)tab.c[kk], s = (double)tab.s[kk];
  const double t6[6] = {t[0], t[1], t[2], t[3], t[4], t[5]};
  fill_cells<false>(cell, xy, stride, first, n, sg, t6, c, s);
  __syncthreads();
  const int count = (int)thr[NT - 1];
  unsigned long long best = 0ull;
  // the candidates of one slot (v, four u from u) that are in the window and reach the floor: into best; the highest score of them
  auto take = [&](const unsigned sum[4], int v, int u) {
    unsigned m = 0u;
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (v <= g.V && u + j <= g.U && sum[j] >= floor_score) {
        const unsigned long long cand = key_of(sum[j], u + j, v, (v + g.V) * nu + u + j + g.U);
        best = cand > best ? cand : best;
        m = sum[j] > m ? sum[j] : m;
      }
    return m;
  };
  // sixteen listed blocks at a time while there are as many: a thread owns one slot of one block and walks every point, as in
  // gmm_score -- the reads per thread of the part scheme without its sums through LDS.  A wavefront takes two rows of the sixteen
  // blocks: where the blocks are neighbours (bounds that do not prune), 128 neighbouring bytes a row
  int e = 0;
  for (; e + 16 <= count; e += 16) {
    __syncthreads();  // (t_cur of the blocks before has settled for the part scheme below; here a late value only skips less)
    const int bi = (int)list[e + ((tid & 31) >> 1)];
    if (bnd[bi] < t_cur) continue;  // an exact score above this bound is already known
    const int bv = bi / sg.nbu, bu = bi - bv * sg.nbu;
    const int v = -g.V + 8 * bv + (tid >> 5), u = -g.U + 8 * bu + 4 * (tid & 1);
    unsigned sum[4] = {0u, 0u, 0u, 0u};
    walk(F, cell, n, 0, 1, (unsigned)(v * (int)g.pitch + u), sum);
    const unsigned m = take(sum, v, u);
    if (m > t0) atomicMax(&t_cur, m);  // (LDS)
  }
  // the rest, fewer than sixteen (all there is once the bounds prune): a block at a time, its points dealt to 16 parts
  for (; e < count; e++) {
    __syncthreads();  // (t_cur of the block before has settled)
    const int bi = (int)list[e];
    if (bnd[bi] < t_cur) continue;  // (workgroup-uniform)
    const int bv = bi / sg.nbu, bu = bi - bv * sg.nbu;
    unsigned sum[4];
    score_block(F, cell, n, g, bv, bu, red, sum);
    if (tid < 16) {
      const unsigned m = take(sum, -g.V + 8 * bv + (tid >> 1), -g.U + 8 * bu + 4 * (tid & 1));
      if (m > t0) atomicMax(&t_cur, m);  // (LDS)
    }
  }
  best = block_max(best, keys);
  if (tid == 0) out_keys[(int64_t)job * nk + kk] = best, out_counts[(int64_t)job * nk + kk] = count;
}

__global__ __launch_bounds__(NT) void gms_pick(const float *__restrict__ xy, int64_t stride, const int64_t *__restrict__ offsets,
                                               const double *__restrict__ priors, Tables tab, SearchGeo sg, const unsigned *__restrict__ bounds,
                                               const unsigned *__restrict__ prior_scores, const unsigned long long *__restrict__ in_keys,
                                               const int *__restrict__ in_counts, rsx_gridmap_search_result *__restrict__ results) {
  __shared__ unsigned long long wide_hi[NT], wide_lo[NT];
  __shared__ unsigned seconds[NT];
  __shared__ unsigned n_placed, n_inside, n_refined;
  const MatchGeo &g = sg.g;
  const int tid = threadIdx.x, job = blockIdx.x;
  const int nk = 2 * g.K + 1, nv = 2 * g.V + 1, nu = 2 * g.U + 1, nb = sg.nbv * sg.nbu;
  const double *t = priors + 6 * (int64_t)job;
  int64_t first;
  const int64_t n64 = job_points(offsets, job, &first);
  const int skipped = skip_status(t, n64);
  if (skipped) {  // (workgroup-uniform) a zero record but for the status
    if (tid == 0) {
      rsx_gridmap_search_result r;
      memset(&r, 0, sizeof(r));
      r.status = skipped;
      results[job] = r;
    }
    return;
  }
  if (tid == 0) n_placed = 0u, n_inside = 0u, n_refined = 0u;
  __syncthreads();
  // ---- the winner over the keys of the 2K + 1 rotations, by the whole tie order ----
  unsigned long long key_hi = 0ull, key_lo = 0ull;
  unsigned refined = 0u;
  for (int i = tid; i < nk; i += NT) {
    const unsigned long long k64 = in_keys[(int64_t)job * nk + i];
    refined += (unsigned)in_counts[(int64_t)job * nk + i];
    if (k64 == 0ull) continue;
    const int k = i - g.K, local = 0x7ffff - (int)(k64 & 0x7ffffull);
    wide_max(key_hi, key_lo, ((k64 >> 37) << 8) | (unsigned long long)(255 - (k < 0 ? -k : k)),
             (((k64 >> 19) & 0x3ffffull) << 27) | (unsigned long long)(0x7ffffff - (i * nv * nu + local)));
  }
  atomicAdd(&n_refined, refined);  // (LDS)
  const WideKey key = block_wide_max(key_hi, key_lo, wide_hi, wide_lo);
  const bool found = key.hi != 0ull;
  const int index = found ? 0x7ffffff - (int)(key.lo & 0x7ffffffull) : (g.K * nv + g.V) * nu + g.U;
  const int ui = index % nu, vi = (index / nu) % nv, ki = index / (nu * nv);
  const int bu = ui - g.U, bv = vi - g.V, bk = ki - g.K;
  // ---- bound_runner_up: the largest bound among the blocks farther than 1 from the winner's block in k, bv or bu ----
  unsigned second = 0u;
  if (found) {  // (workgroup-uniform)
    const unsigned *bnd = bounds + (int64_t)job * nk * nb;
    const int wbv = vi >> 3, wbu = ui >> 3;
    for (int i = tid; i < nk * nb; i += NT) {
      const int rest = i % nb;
      const int dk = i / nb - ki, dv = rest / sg.nbu - wbv, du = rest % sg.nbu - wbu;
      const bool far = du > 1 || du < -1 || dv > 1 || dv < -1 || dk > 1 || dk < -1;
      second = far && bnd[i] > second ? bnd[i] : second;
    }
  }
  second = block_max(second, seconds);
  // ---- the counts at the winner (at k = 0 without one) ----
  const double c = (double)tab.c[ki], s = (double)tab.s[ki];
  const double t6[6] = {t[0], t[1], t[2], t[3], t[4], t[5]};
  count_at(g, sg.PL, xy, stride, first, (int)n64, t6, c, s, bu, bv, &n_placed, &n_inside);
  __syncthreads();
  if (tid != 0) return;
  rsx_gridmap_search_result r;
  memset(&r, 0, sizeof(r));
  r.score = found ? (unsigned)(key.hi >> 8) : 0u;
  r.score_prior = prior_scores[job];
  r.bound_runner_up = second;
  r.k = bk, r.u = bu, r.v = bv;
  r.n_points = (int)n_placed, r.n_inside = (int)n_inside;
  r.n_blocks = nk * nb, r.n_refined = (int)n_refined;
  if (!found) r.status = sg.min_score == 0u ? RSX_GRIDMAP_MATCH_STATUS_EMPTY : RSX_GRIDMAP_SEARCH_STATUS_BELOW;
  winner_transform(r.transform, found, t6, c, s, bu, bv, g.res);
  results[job] = r;
}

// one workgroup per tile of 32 x 32 cells of the frame: the likelihood bytes of the tile and of 7 more columns and rows into LDS
// (0 outside the map), the 8-wide sliding maximum along the rows, then along the columns; every cell of F and of Pd is written
__global__ __launch_bounds__(NT) void gms_prepare(const uint8_t *__restrict__ like, int64_t like_pitch, int W, int H, int M, int cw, int ch,
                                                  uint8_t *__restrict__ F, uint8_t *__restrict__ Pd) {
  __shared__ uint8_t in[TILE + 7][TILE + 8];
  __shared__ uint8_t rowmax[TILE + 7][TILE];
  const int tid = threadIdx.x, X0 = TILE * (int)blockIdx.x, Y0 = TILE * (int)blockIdx.y;
  for (int i = tid; i < (TILE + 7) * (TILE + 7); i += NT) {
    const int r = i / (TILE + 7), q = i - r * (TILE + 7);
    const int y = Y0 + r - M, x = X0 + q - M;
    in[r][q] = (x >= 0 && x < W && y >= 0 && y < H) ? like[(int64_t)y * like_pitch + x] : (uint8_t)0;
  }
  __syncthreads();
  for (int i = tid; i < (TILE + 7) * TILE; i += NT) {
    const int r = i / TILE, q = i - r * TILE;
    uint8_t m = in[r][q];
#pragma unroll
    for (int b = 1; b < 8; b++) m = in[r][q + b] > m ? in[r][q + b] : m;
    rowmax[r][q] = m;
  }
  __syncthreads();
  for (int i = tid; i < TILE * TILE; i += NT) {
    const int r = i / TILE, q = i - r * TILE;
    const int fy = Y0 + r, fx = X0 + q;
    if (fy >= 8 * ch || fx >= 8 * cw) continue;
    uint8_t m = rowmax[r][q];
#pragma unroll
    for (int a = 1; a < 8; a++) m = rowmax[r + a][q] > m ? rowmax[r + a][q] : m;
    F[(size_t)fy * (size_t)(8 * cw) + fx] = in[r][q];
    Pd[((size_t)((fy & 7) * 8 + (fx & 7)) * ch + (fy >> 3)) * cw + (fx >> 3)] = m;
  }
}

int resolve(const rsx_gridmap_search_params *params, rsx_gridmap_search_params &dp) {
  rsx_gridmap_search_default_params(&dp);
  if (params) dp = *params;
  return gridloc::check_window_params(dp, MAX_K, MAX_UV);
}

int blocks_of(int cells) { return (2 * cells + 1 + 7) / 8; }
size_t blocks(const rsx_gridmap_search_params &p) { return (size_t)(2 * p.angle_steps + 1) * blocks_of(p.y_cells) * blocks_of(p.x_cells); }

// what only a prepared handle can judge (the caller holds h->mu)
int check_prepared(const rsx_gridmap *h, const rsx_gridmap_search_params &p) {
  if (h->s_cells < 0) return fail(RSX_ERR_BAD_ARG, "no search snapshot yet: rsx_gridmap_search_prepare first");
  if (p.x_cells > h->s_cells || p.y_cells > h->s_cells)
    return fail(RSX_ERR_BAD_ARG, "x_cells %d or y_cells %d above the prepared max_cells %d", p.x_cells, p.y_cells, h->s_cells);
  return RSX_OK;
}

// the call as gridloc_host.h's scaffold takes it: the bounds of (2K + 1) nbv nbu words per job, in h->s_bounds unless the caller
// gave room, and the three launches
gridloc::LocCall describe(const rsx_gridmap_search_params &p) {
  return {[&p](const rsx_gridmap *h) { return check_prepared(h, p); }, blocks(p), &rsx_gridmap::s_bounds, sizeof(rsx_gridmap_search_result),
          [&p](rsx_gridmap *h, const gridloc::LocJobs &j, void *d_results, uint32_t *d_bounds, hipStream_t s) -> int {
            const Tables tab(p.angle_steps, p.angle_step);
            SearchGeo sg{};
            sg.g = gridloc::match_geo(h, p.angle_steps, p.x_cells, p.y_cells, (unsigned)(8 * h->s_cw));
            sg.M = h->s_margin, sg.cw = h->s_cw, sg.ch = h->s_ch;
            sg.PL = std::max(64, std::max(p.x_cells, p.y_cells));
            sg.nbu = blocks_of(p.x_cells), sg.nbv = blocks_of(p.y_cells);
            sg.nowhere = -(h->s_cells + 32);
            sg.min_score = p.min_score;
            const size_t nk = (size_t)(2 * p.angle_steps + 1), per_k = (size_t)j.n * nk;
            RSX_TRY(h->s_aux.reserve(16 * per_k + 4 * (size_t)j.n, s, false));
            unsigned long long *keys = h->s_aux.as<unsigned long long>();
            unsigned *seeds = reinterpret_cast<unsigned *>(keys + per_k);
            int *counts = reinterpret_cast<int *>(seeds + per_k);
            unsigned *prior_scores = reinterpret_cast<unsigned *>(counts + per_k);
            const uint8_t *F = h->s_frame.as<uint8_t>(), *Pd = h->s_pool.as<uint8_t>();
            hipLaunchKernelGGL(gms_bound, dim3((unsigned)per_k), dim3(NT), 0, s, j.xy, j.stride, j.off, j.priors, tab, sg, F, Pd, d_bounds, seeds, prior_scores);
            RSX_HIP(hipGetLastError());
            hipLaunchKernelGGL(gms_refine, dim3((unsigned)per_k), dim3(NT), 0, s, j.xy, j.stride, j.off, j.priors, tab, sg, F, d_bounds, seeds, prior_scores,
                               keys, counts);
            RSX_HIP(hipGetLastError());
            hipLaunchKernelGGL(gms_pick, dim3((unsigned)j.n), dim3(NT), 0, s, j.xy, j.stride, j.off, j.priors, tab, sg, d_bounds, prior_scores, keys, counts,
                               static_cast<rsx_gridmap_search_result *>(d_results));
            RSX_HIP(hipGetLastError());
            return RSX_OK;
          }};
}

}  // namespace

extern "C" {

int rsx_gridmap_search_default_params(rsx_gridmap_search_params *p) try {
  if (!p) return fail(RSX_ERR_BAD_ARG, "null params");
  p->angle_step = 0.01;
  p->angle_steps = 32;
  p->x_cells = 64;
  p->y_cells = 64;
  p->min_score = 0u;
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_gridmap_search_prepare(rsx_gridmap *h, int32_t max_cells, void *stream) try {
  if (max_cells < 0 || max_cells > MAX_UV) return fail(RSX_ERR_BAD_ARG, "max_cells %d outside 0 .. %d", max_cells, MAX_UV);
  if (!h) return fail(RSX_ERR_BAD_ARG, "null handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (!h->have_like) return rsx::no_likelihood();
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
  RSX_TRY(h->order.enter(s));
  const int M = (std::max(64, (int)max_cells) + max_cells + 32 + 7) & ~7;
  const int cw = (h->p.width + 2 * M + 7) / 8, ch = (h->p.height + 2 * M + 7) / 8;
  const size_t bytes = (size_t)64 * cw * ch;
  if (bytes >= ((size_t)1 << 32)) return fail(RSX_ERR_BAD_ARG, "a frame of %d x %d cells is 4 GB or more", 8 * cw, 8 * ch);
  h->s_cells = -1;  // (nothing is prepared should an allocation fail)
  const bool fresh = bytes > h->s_frame.bytes || bytes > h->s_pool.bytes;
  RSX_TRY(h->s_frame.reserve(bytes, s, false));
  RSX_TRY(h->s_pool.reserve(bytes, s, false));
  if (fresh) {  // (the kernel writes every byte a search reads; what a grown buffer holds beyond them is zeroed once)
    RSX_HIP(hipMemsetAsync(h->s_frame.p, 0, h->s_frame.bytes, s));
    RSX_HIP(hipMemsetAsync(h->s_pool.p, 0, h->s_pool.bytes, s));
  }
  hipLaunchKernelGGL(gms_prepare, dim3((unsigned)((8 * cw + TILE - 1) / TILE), (unsigned)((8 * ch + TILE - 1) / TILE)), dim3(NT), 0, s, h->like_origin(),
                     h->like_pitch(), h->p.width, h->p.height, M, cw, ch, h->s_frame.as<uint8_t>(), h->s_pool.as<uint8_t>());
  RSX_HIP(hipGetLastError());
  h->s_margin = M, h->s_cw = cw, h->s_ch = ch, h->s_cells = max_cells;
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_gridmap_search_batch_device(rsx_gridmap *h, const float *d_xy, const int64_t *d_offsets, int32_t point_stride, int32_t n_jobs,
                                    const double *d_priors, const rsx_gridmap_search_params *params, rsx_gridmap_search_result *d_results,
                                    uint32_t *d_bounds, void *stream) try {
  RSX_TRY(gridloc::check_args(d_xy, d_offsets, d_priors, d_results, n_jobs, point_stride));
  rsx_gridmap_search_params dp;
  RSX_TRY(resolve(params, dp));
  if ((int64_t)n_jobs * (2 * dp.angle_steps + 1) > 0x7fffffffll) return fail(RSX_ERR_BAD_ARG, "n_jobs %d times %d rotations is 2^31 or more", n_jobs, 2 * dp.angle_steps + 1);
  return gridloc::run_device(h, describe(dp), {d_xy, d_offsets, point_stride, n_jobs, d_priors}, d_results, d_bounds, stream);
} RSX_CATCH_ALL

int rsx_gridmap_search_batch(rsx_gridmap *h, const float *xy, const int64_t *offsets, int32_t n_jobs, const double *priors,
                             const rsx_gridmap_search_params *params, rsx_gridmap_search_result *out_results, uint32_t *out_bounds) try {
  RSX_TRY(gridloc::check_args(xy, offsets, priors, out_results, n_jobs, 2));
  rsx_gridmap_search_params dp;
  RSX_TRY(resolve(params, dp));
  return gridloc::run_host(h, describe(dp), "rsx_gridmap_search_batch", xy, offsets, n_jobs, priors, out_results, out_bounds);
} RSX_CATCH_ALL

}  // extern "C"
