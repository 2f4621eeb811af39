// cfear_track.hip -- CFEAR point-to-line registration and the keyframe tracker (Adolfsson et al., CFEAR radar odometry): a scan is
// registered JOINTLY against the last few keyframes, from a constant-velocity prediction, and becomes a keyframe itself only
// after enough motion; the registration of a PAIR of scans (rsx_cfear_register_batch, the odometry without tracking) is the same
// with one keyframe at the identity pose.  The rules are written in include/rsx.h and restated in tests/cfear_np.py (pairs) and
// tests/cfear_track_np.py (PARITY UNPINNED); those files are the arithmetic contract.  fp64 throughout, nothing fused, as in
// csrc/cfear.hip, which makes the surface points.
//
// joint_register: the one Gauss-Newton loop of the library, the device function both kernels call.  512 threads (the fp64 sincos wants the 256 VGPRs of two waves per
//   SIMD).  Per Gauss-Newton iteration: threads 0 .. K-1 take the scan's pose in their keyframe's frame (one sincos each) and
//   leave it in LDS; the items (record i, keyframe c) are strided over the threads as item = i * K + c (so a thread's items ascend
//   in i and, inside, in ring order, and with K = 1 a thread has records t, t + 512, ...); a thread finds the correspondence of
//   each of its items and adds its term; the sums are taken per thread in ascending item, then by a butterfly over the lanes of
//   a wavefront, then over the 8 wavefront sums in ascending order; every thread holds the same 3 x 3 system and solves it
//   itself, so the loop needs no host and its branches are uniform.  With K = 1 at the identity pose every expression reduces
//   to the pair rule's of tests/cfear_np.py (tests/golden/cfear_pairs_parent.npz pins the bytes).
//   The correspondence of (record, keyframe) comes from one of two searches that give the same record, hence the same bytes:
//   search 0  the keyframe's CELL INDEX: its records binned by floor(mu / radius), clamped into the 128 x 128 grid (a clamp is
//             monotone and 1-Lipschitz: two records within the radius stay in adjacent cells, and a query far outside finds only
//             records the d2 <= r^2 test rejects), sorted by (cell, record index) with a bitonic sort in LDS as the surface kernel
//             sorts its points; a 16-bit table start[cell] stays in LDS (32 KiB per keyframe, four of them), the sorted keys and
//             the records in sorted order lie in HBM and are read through L2.  The 3 x 3 block's candidates are compared
//             lexicographically by (d2, record index): the brute-force rule's choice in any visiting order.  The first record of
//             each of the nine cells is read in one batch of independent loads, further records of a cell are walked.  All 4096
//             records in one cell make the walk a brute-force one, nothing else
//   search 1  brute force: one keyframe at a time staged in LDS, every lane reads the same address; the chosen index per (record,
//             keyframe) is parked in LDS (16 bit) so that the sums run in the one order above
// cfear_joint_kernel: a workgroup takes jobs blockIdx.x, blockIdx.x + gridDim.x, ...; it bins the job's keyframes into its
//   own slice of the index workspace, then registers.  Without job offsets job i has keyframe i alone, without poses every
//   keyframe is at the identity: the pair entries.  cfear_track_kernel: one workgroup per sequence loops over the sequence's
//   scans with no host round trip; the ring (records, poses, sorted keys and records) lives in the sequence's state in HBM, the
//   header is read at the start and written back at the end, the LDS tables are rebuilt from the sorted keys at the start.  A
//   workgroup reads back what it wrote to HBM only behind __threadfence_block() + __syncthreads(); no workgroup reads another's.
//   cfear_track_kernel<COMP = true> (rsx_cfear_track_params.compensate, tests/cfear_mocomp_np.py): the scan is compensated for the sensor's
//   motion into a copy in the state before each of two registrations -- with the motion before it, then with the motion the first
//   registration found -- and the first keyframe once the first motion is known; joint_register itself knows nothing of it.
// GENERAL (joint_register and both kernels; the host takes it when rsx_cfear_params.cost | loss | weights != 0): the term a
//   correspondence adds is chosen among point-to-line / point-to-point / point-to-distribution, Huber / Cauchy / none, weighted or
//   not (include/rsx.h, tests/cfear_cost_np.py) by uniform branches on three integers of the kernel's constants (RgGeneral) -- one instance for all
//   seventeen combinations.  Two rows add into the same eleven sums.  What the other objectives read beside x, y, nx, ny -- the
//   second 16 bytes of the CHOSEN record and of the src record -- is fetched by record index after the search; the searches, the
//   index and the staged keyframes stay at 16 bytes per candidate.  The instances without GENERAL are the code they were.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <new>
#include <type_traits>

#include "cfear.h"
#include "cfear_dev.h"
#include "rsx_wave_dev.h"
#include "ragged_host.h"

#pragma STDC FP_CONTRACT OFF

namespace {

constexpr int NT = 512, NW = NT / 64;
using namespace rsx::cfear;  // the grid, the keys and the sort of cfear_dev.h
constexpr int CAP = RSX_CFEAR_MAX_SURFACE_POINTS, MAXK = RSX_CFEAR_MAX_KEYFRAMES;
constexpr unsigned IDX_BITS = 12, IDX_MASK = (1u << IDX_BITS) - 1u;
constexpr unsigned short NO_BEST = 0xFFFF;
constexpr int N_SUMS = 11;  // H00 H10 H11 H20 H21 H22 g0 g1 g2 cost count
static_assert(CAP == (1 << IDX_BITS) && NCELL == (1 << 14), "a key is cell << 12 | record index");
static_assert(sizeof(rsx_cfear_surface_point) == 32 && sizeof(rsx_cfear_result) == 48 && sizeof(rsx_cfear_track_result) == 80 &&
                  sizeof(rsx_cfear_params) == 64 && sizeof(rsx_cfear_track_params) == 40,
              "record layouts of include/rsx.h");
// dynamic LDS: [0, 128 KiB) the four cell tables (search 0), or one staged keyframe (64 KiB) and the parked choices (32 KiB)
// (search 1); then the sort buffer of the index build
constexpr size_t LDS_TABLES = (size_t)MAXK * NCELL * 2, LDS_STAGE = (size_t)CAP * 16;
constexpr size_t LDS_BYTES = LDS_TABLES + (size_t)CAP * 4;
static_assert(LDS_STAGE + (size_t)MAXK * CAP * 2 <= LDS_TABLES, "search 1 fits where the tables are");
// the index of one keyframe in HBM: records in sorted order, then their keys; a workgroup's workspace / a sequence's ring holds MAXK
constexpr size_t WS_SORTED = (size_t)MAXK * CAP * 16, WS_KEYS = (size_t)MAXK * CAP * 4, WS_BYTES = WS_SORTED + WS_KEYS;
constexpr int MAX_JOINT_BLOCKS = 256;  // one per CU; more jobs are strided over them

struct RgConsts {
  double r, r2, cos_max, delta, step_epsilon;
  int max_iterations, min_correspondences;
};
// ... of the GENERAL instances: with rsx_cfear_params' cost, loss and weights.  A type of its own, so that the kernel arguments of
// the instances without GENERAL keep their layout, and with it the code the compiler makes of them
struct RgGeneral : RgConsts {
  int cost, loss, weights;
};
template <bool GENERAL>
using Rg = std::conditional_t<GENERAL, RgGeneral, RgConsts>;

struct TrConsts {
  double keyframe_distance, keyframe_rotation;
  int n_keyframes, predict, search;
};

struct KfDesc {
  const float4 *orig;    // record j's x, y, nx, ny at orig[j * stride]
  const float4 *sorted;  // search 0: the same in (cell, j) order ...
  const unsigned *keys;  // ... and cell << 12 | j of each
  double x, y, yaw, c, s;  // the keyframe's pose in the map frame, cos and sin of its yaw
  int stride, n, slot;   // slot: which LDS table
};

struct KfFrame {  // the scan's pose in a keyframe's frame, this iteration
  double cs, sn, tx, ty;
};

// a sequence's state in HBM; all zero = no scan seen
struct TrackHeader {
  double P[3], M[3];
  double kf_pose[MAXK][3];
  int32_t kf_n[MAXK];  // records of the slot's keyframe (RSX_CFEAR_MAX_SURFACE_POINTS + 1: more, none stored)
  int32_t head, n_ring, started;
  int32_t first;  // compensation: the ring's only keyframe is the sequence's first scan, still as measured (its times: ST_TAU0)
};
// ... then, for compensation: the times of the first scan's records, and the current scan compensated (x, y, nx, ny per record);
// then, for the GENERAL instances: the second halves (lambda_max, lambda_min, n_points, cell) of the ring's records, slot by slot as
// ST_ORIG holds the first halves; written where a keyframe is inserted and never by compensation (a rigid motion leaves them)
constexpr size_t ST_HEADER = 256, ST_ORIG = ST_HEADER, ST_INDEX = ST_ORIG + (size_t)MAXK * CAP * 16, ST_TAU0 = ST_INDEX + WS_BYTES,
                 ST_COMP = ST_TAU0 + (size_t)CAP * 4, ST_EXTRA = ST_COMP + (size_t)CAP * 16, ST_BYTES = ST_EXTRA + (size_t)MAXK * CAP * 16;
static_assert(sizeof(TrackHeader) <= ST_HEADER, "header room");
static_assert(ST_ORIG % 16 == 0 && ST_EXTRA % 16 == 0 && ST_BYTES % 16 == 0, "float4 regions");

// the second half of a surface-point record as the GENERAL instances read it
struct SpExtra {
  double lmax, lmin, n;
  bool valid;  // include/rsx.h: lambda_min > 0, lambda_max >= lambda_min, both finite
};
__device__ __forceinline__ SpExtra sp_extra(const float4 &h) {
  SpExtra e;
  e.lmax = (double)h.x;
  e.lmin = (double)h.y;
  e.n = (double)__float_as_int(h.z);
  e.valid = h.y > 0.f && h.x >= h.y && fabsf(h.x) < INFINITY && fabsf(h.y) < INFINITY;
  return e;
}

__device__ __forceinline__ int cell_coord(double v, double r) {
  const double f = floor(v / r);
  return !(f >= -(double)HALF) ? 0 : (f >= (double)HALF ? GRID - 1 : (int)f + HALF);  // (a NaN lands in cell 0 and is never matched)
}

// the cell index of one keyframe of 1 <= n <= CAP records: table in LDS, sorted keys and records to HBM; ends behind a barrier
__device__ void build_index(const float4 *orig, int stride, int n, unsigned *keys_out, float4 *sorted_out, unsigned short *table,
                            unsigned *sortbuf, double r, int t) {
  unsigned n2 = NT;
  while (n2 < (unsigned)n) n2 <<= 1;
  for (unsigned i = t; i < n2; i += NT) {
    unsigned key = NO_KEY;
    if (i < (unsigned)n) {
      const float4 q = orig[(size_t)i * stride];
      key = ((unsigned)(cell_coord((double)q.y, r) * GRID + cell_coord((double)q.x, r)) << IDX_BITS) | i;
    }
    sortbuf[i] = key;
  }
  for (int c = t; c < NCELL; c += NT) table[c] = NO_CELL;
  __syncthreads();
  bitonic_sort_lds<NT>(sortbuf, n2, t);
  fill_cell_table<NT, IDX_BITS, false>(sortbuf, n, table, t);  // (every record has a cell: cell_coord clamps)
  for (int i = t; i < n; i += NT) {
    const unsigned key = sortbuf[i];
    keys_out[i] = key;
    sorted_out[i] = orig[(size_t)(key & IDX_MASK) * stride];
  }
  __threadfence_block();  // the workgroup reads keys_out and sorted_out again
  __syncthreads();
}

// The joint registration of one scan (ns64 records at sp[i * sstride]) against kf[0 .. K) (LDS, ring order; K <= MAXK; search 0:
// every keyframe of 1 .. CAP records has its index built) from (x, y, yaw).  Called by all threads behind a barrier; every thread
// returns the same result.  s_red: [NW][N_SUMS], s_fr: [MAXK]
// GENERAL: the objective is chosen by k.cost, k.loss and k.weights (include/rsx.h; tests/cfear_cost_np.py) with workgroup-uniform
// branches; without it the code is the point-to-line / Huber / unweighted one it was, and sx, sxstride and kf_xoff are not read.
// The second half of src record i is sx[i * sxstride] (the input record's, also when sp is a compensated copy), that of record j of
// keyframe c is kf[c].orig[j * kf[c].stride + kf_xoff]; only the chosen record's is fetched, the searches read what they read
template <bool GENERAL>
__device__ void joint_register(const float4 *sp, int sstride, const float4 *sx, int sxstride, int64_t ns64, int K, const KfDesc *kf,
                               ptrdiff_t kf_xoff, int search, unsigned char *lds, double *s_red, KfFrame *s_fr, const Rg<GENERAL> &k, double x,
                               double y, double yaw, rsx_cfear_result &res) {
  const int t = threadIdx.x;
  res.x = x;
  res.y = y;
  res.yaw = yaw;
  res.cost = 0.0;
  res.iterations = res.correspondences = res.status = res.reserved = 0;
  bool any = false, over = ns64 > CAP;
  for (int c = 0; c < K; c++) {
    any |= kf[c].n > 0;
    over |= kf[c].n > CAP;
  }
  if (ns64 <= 0 || !any) {  // (uniform)
    res.status = 1;
    return;
  }
  if (over) {
    res.status = 2;
    return;
  }
  const int ns = (int)ns64;
  const unsigned short *tables = reinterpret_cast<const unsigned short *>(lds);
  float4 *stage = reinterpret_cast<float4 *>(lds);
  unsigned short *parked = reinterpret_cast<unsigned short *>(lds + LDS_STAGE);  // [ns * K <= MAXK * CAP], by item
  const unsigned lane = t & 63, w = t >> 6;
  int it = 0, status = 0;
  for (;;) {
    if (t < K) {
      const KfDesc &f = kf[t];
      KfFrame fr;
      sincos(yaw - f.yaw, &fr.sn, &fr.cs);
      const double ux = x - f.x, uy = y - f.y;
      fr.tx = f.c * ux + f.s * uy;
      fr.ty = f.c * uy - f.s * ux;
      s_fr[t] = fr;
    }
    __syncthreads();
    // the items (record i, keyframe c), item = i * K + c, are strided over the threads: a thread's items ascend in i, then in c
    const int n_items = ns * K;
    if (search == RSX_CFEAR_SEARCH_BRUTE) {
      for (int c = 0; c < K; c++) {
        const int nd = kf[c].n;
        if (nd == 0) continue;  // (uniform)
        const float4 *orig = kf[c].orig;
        const int stride = kf[c].stride;
        for (int j = t; j < nd; j += NT) stage[j] = orig[(size_t)j * stride];
        __syncthreads();
        const KfFrame fr = s_fr[c];
#pragma unroll 1
        for (int item = t; item < n_items; item += NT) {
          const int i = item / K;
          if (item - i * K != c) continue;
          const float4 sr = sp[(size_t)i * sstride];
          const double px = (double)sr.x, py = (double)sr.y, pnx = (double)sr.z, pny = (double)sr.w;
          const double qx = (fr.cs * px - fr.sn * py) + fr.tx, qy = (fr.sn * px + fr.cs * py) + fr.ty;
          const double mx = fr.cs * pnx - fr.sn * pny, my = fr.sn * pnx + fr.cs * pny;
          int best = -1;
          double best_d2 = INFINITY;
#pragma unroll 8
          for (int j = 0; j < nd; j++) {  // (ascending j and a strict <: the lowest j wins a tie)
            const float4 d = stage[j];
            const double ex = qx - (double)d.x, ey = qy - (double)d.y;
            const double d2 = ex * ex + ey * ey;
            const bool ok = (d2 <= k.r2) & (d2 < best_d2) & (mx * (double)d.z + my * (double)d.w >= k.cos_max);
            best = ok ? j : best;
            best_d2 = ok ? d2 : best_d2;
          }
          parked[item] = best < 0 ? NO_BEST : (unsigned short)best;  // (a thread reads back its own entries only)
        }
        __syncthreads();  // (the stage is filled again)
      }
    }
    double acc[N_SUMS];
#pragma unroll
    for (int a = 0; a < N_SUMS; a++) acc[a] = 0.0;
#pragma unroll 1
    for (int item = t; item < n_items; item += NT) {
      const int i = item / K, c = item - i * K;
      const int nd = kf[c].n;
      if (nd == 0) continue;
      const float4 sr = sp[(size_t)i * sstride];
      const double px = (double)sr.x, py = (double)sr.y, pnx = (double)sr.z, pny = (double)sr.w;
      const KfFrame fr = s_fr[c];
      const double qx = (fr.cs * px - fr.sn * py) + fr.tx, qy = (fr.sn * px + fr.cs * py) + fr.ty;
      float4 d;
      unsigned jsel = 0;  // (GENERAL) the chosen record's index
      if (search == RSX_CFEAR_SEARCH_BRUTE) {
        const unsigned short j = parked[item];
        if (j == NO_BEST) continue;
        d = kf[c].orig[(size_t)j * kf[c].stride];
        if constexpr (GENERAL) jsel = j;
      } else {
        const double mx = fr.cs * pnx - fr.sn * pny, my = fr.sn * pnx + fr.cs * pny;
        const unsigned short *table = tables + (size_t)kf[c].slot * NCELL;
        const unsigned *keys = kf[c].keys;
        const float4 *sorted = kf[c].sorted;
        const int ix = cell_coord(qx, k.r), iy = cell_coord(qy, k.r);
        bool found = false;
        unsigned best_j = 0;
        double best_d2 = INFINITY;
        auto consider = [&](unsigned key, const float4 &e4) {
          const double ex = qx - (double)e4.x, ey = qy - (double)e4.y;
          const double d2 = ex * ex + ey * ey;
          const unsigned j = key & IDX_MASK;
          const bool ok = (d2 <= k.r2) & ((d2 < best_d2) | ((d2 == best_d2) & (j < best_j))) & (mx * (double)e4.z + my * (double)e4.w >= k.cos_max);
          found |= ok;
          best_j = ok ? j : best_j;
          best_d2 = ok ? d2 : best_d2;
          d.x = ok ? e4.x : d.x;
          d.y = ok ? e4.y : d.y;
          d.z = ok ? e4.z : d.z;
          d.w = ok ? e4.w : d.w;
        };
        // the first record of each of the nine cells and the key behind it are loaded at once (independent reads: one trip to
        // L2 for the whole block); a cell that holds more than one record -- rare: a surface point per occupied cell -- is walked
        int p0[9];
        unsigned key0[9], key1[9];
        float4 rec0[9];
#pragma unroll
        for (int b = 0; b < 9; b++) {
          const int jx = ix + b % 3 - 1, jy = iy + b / 3 - 1;
          const bool in = jx >= 0 && jx < GRID && jy >= 0 && jy < GRID;
          const int p = in ? (int)table[in ? jy * GRID + jx : 0] : (int)NO_CELL;
          p0[b] = p == NO_CELL ? -1 : p;
        }
#pragma unroll
        for (int b = 0; b < 9; b++) {
          const int p = p0[b] < 0 ? 0 : p0[b];  // (position 0 exists: nd >= 1)
          key0[b] = keys[p];
          rec0[b] = sorted[p];
          key1[b] = keys[p + 1 < nd ? p + 1 : p];
        }
        d = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int b = 0; b < 9; b++) {
          if (p0[b] < 0) continue;
          consider(key0[b], rec0[b]);
          const unsigned cc = key0[b] >> IDX_BITS;
          if (p0[b] + 1 < nd && (key1[b] >> IDX_BITS) == cc)
            for (int p = p0[b] + 1; p < nd; p++) {
              const unsigned key = keys[p];
              if ((key >> IDX_BITS) != cc) break;
              consider(key, sorted[p]);
            }
        }
        if (!found) continue;
        if constexpr (GENERAL) jsel = best_j;
      }
      const double nx = (double)d.z, ny = (double)d.w;
      if constexpr (GENERAL) {
        double sc0 = 1.0, sc1 = 1.0, v = 1.0;
        if (k.cost == RSX_CFEAR_COST_P2D || k.weights) {  // (uniform)
          const SpExtra dj = sp_extra(kf[c].orig[(size_t)jsel * kf[c].stride + kf_xoff]);
          if (!dj.valid) continue;
          if (k.cost == RSX_CFEAR_COST_P2D) {
            sc0 = 1.0 / sqrt(dj.lmin);
            sc1 = 1.0 / sqrt(dj.lmax);
          }
          if (k.weights) {
            const SpExtra si = sp_extra(sx[(size_t)i * sxstride]);
            if (!si.valid) continue;
            const double mx = fr.cs * pnx - fr.sn * pny, my = fr.sn * pnx + fr.cs * pny;
            const double w_dir = fmax(mx * nx + my * ny, 0.0);
            const double p_i = log(1.0 + si.lmax / si.lmin), p_j = log(1.0 + dj.lmax / dj.lmin);
            const double w_plan = (2.0 * fmin(p_i, p_j)) / (p_i + p_j), w_num = (2.0 * fmin(si.n, dj.n)) / (si.n + dj.n);
            v = (w_dir * w_plan) * w_num;
          }
        }
        const double ex = qx - (double)d.x, ey = qy - (double)d.y;
        const double ppx = -fr.sn * px - fr.cs * py, ppy = fr.cs * px - fr.sn * py;  // R'(yaw_r) mu_i
        const double kc = kf[c].c, ks = kf[c].s;
        const double e0 = sc0 * (nx * ex + ny * ey);
        const double a0 = sc0 * (kc * nx - ks * ny), a1 = sc0 * (ks * nx + kc * ny), a2 = sc0 * (nx * ppx + ny * ppy);
        const bool two = k.cost != RSX_CFEAR_COST_P2L;  // (uniform) the second row, along t_j = (-n_jy, n_jx)
        const double ux = -ny, uy = nx;
        const double e1 = sc1 * (ux * ex + uy * ey);
        const double b0 = sc1 * (kc * ux - ks * uy), b1 = sc1 * (ks * ux + kc * uy), b2 = sc1 * (ux * ppx + uy * ppy);
        double s2, a, half;
        if (two) {
          s2 = e0 * e0 + e1 * e1;
          a = sqrt(s2);
          half = 0.5 * s2;
        } else {
          s2 = e0 * e0;
          a = fabs(e0);
          half = 0.5 * e0 * e0;
        }
        double wt, rho;
        if (k.loss == RSX_CFEAR_LOSS_HUBER) {
          wt = a <= k.delta ? 1.0 : k.delta / a;
          rho = a <= k.delta ? half : k.delta * (a - 0.5 * k.delta);
        } else if (k.loss == RSX_CFEAR_LOSS_CAUCHY) {
          const double dd = k.delta * k.delta, z = 1.0 + s2 / dd;
          wt = 1.0 / z;
          rho = (0.5 * dd) * log(z);
        } else {
          wt = 1.0;
          rho = half;
        }
        const double vw = v * wt;
        acc[0] += vw * a0 * a0;
        acc[1] += vw * a1 * a0;
        acc[2] += vw * a1 * a1;
        acc[3] += vw * a2 * a0;
        acc[4] += vw * a2 * a1;
        acc[5] += vw * a2 * a2;
        acc[6] += vw * a0 * e0;
        acc[7] += vw * a1 * e0;
        acc[8] += vw * a2 * e0;
        if (two) {
          acc[0] += vw * b0 * b0;
          acc[1] += vw * b1 * b0;
          acc[2] += vw * b1 * b1;
          acc[3] += vw * b2 * b0;
          acc[4] += vw * b2 * b1;
          acc[5] += vw * b2 * b2;
          acc[6] += vw * b0 * e1;
          acc[7] += vw * b1 * e1;
          acc[8] += vw * b2 * e1;
        }
        acc[9] += v * rho;
        acc[10] += 1.0;
        continue;
      }
      const double e = nx * (qx - (double)d.x) + ny * (qy - (double)d.y);
      const double ae = fabs(e);
      const double wt = ae <= k.delta ? 1.0 : k.delta / ae;
      const double kc = kf[c].c, ks = kf[c].s;
      const double j0 = kc * nx - ks * ny, j1 = ks * nx + kc * ny, j2 = nx * (-fr.sn * px - fr.cs * py) + ny * (fr.cs * px - fr.sn * py);
      acc[0] += wt * j0 * j0;
      acc[1] += wt * j1 * j0;
      acc[2] += wt * j1 * j1;
      acc[3] += wt * j2 * j0;
      acc[4] += wt * j2 * j1;
      acc[5] += wt * j2 * j2;
      acc[6] += wt * j0 * e;
      acc[7] += wt * j1 * e;
      acc[8] += wt * j2 * e;
      acc[9] += ae <= k.delta ? 0.5 * e * e : k.delta * (ae - 0.5 * k.delta);
      acc[10] += 1.0;
    }
#pragma unroll
    for (int a = 0; a < N_SUMS; a++) acc[a] = rsx::wave::butterfly(acc[a], rsx::wave::Add{});  // (fp64: this order is the result)
    if (lane == 0) {
#pragma unroll
      for (int a = 0; a < N_SUMS; a++) s_red[w * N_SUMS + a] = acc[a];
    }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < N_SUMS; a++) {
      double v = 0.0;
      for (int ww = 0; ww < NW; ww++) v += s_red[ww * N_SUMS + a];
      acc[a] = v;
    }
    __syncthreads();  // (s_red and s_fr are written again in the next iteration)
    // from here on every thread holds the same numbers
    res.cost = acc[9];
    res.correspondences = (int32_t)acc[10];
    if (res.correspondences < k.min_correspondences) {
      status = 4;
      break;
    }
    const double h00 = acc[0], h10 = acc[1], h11 = acc[2], h20 = acc[3], h21 = acc[4], h22 = acc[5];
    const double d0 = h00;
    if (!(d0 > 1e-12 * h00)) {
      status = 5;
      break;
    }
    const double l10 = h10 / d0, l20 = h20 / d0;
    const double d1 = h11 - l10 * h10;
    if (!(d1 > 1e-12 * h11)) {
      status = 5;
      break;
    }
    const double l21 = (h21 - l20 * h10) / d1;
    const double d2 = (h22 - l20 * h20) - l21 * l21 * d1;
    if (!(d2 > 1e-12 * h22)) {
      status = 5;
      break;
    }
    const double z0 = -acc[6];
    const double z1 = -acc[7] - l10 * z0;
    const double z2 = (-acc[8] - l20 * z0) - l21 * z1;
    const double t2 = z2 / d2;
    const double t1 = z1 / d1 - l21 * t2;
    const double t0 = (z0 / d0 - l10 * t1) - l20 * t2;
    x += t0;
    y += t1;
    yaw += t2;
    it++;
    if (sqrt((t0 * t0 + t1 * t1) + t2 * t2) < k.step_epsilon) break;
    if (it >= k.max_iterations) {
      status = 8;
      break;
    }
  }
  res.x = x;
  res.y = y;
  res.yaw = yaw;
  res.iterations = it;
  res.status = status;
}

__device__ __forceinline__ int clamp_count(int64_t n) { return n <= 0 ? 0 : (n > CAP ? CAP + 1 : (int)n); }

// kf_job_off null: job i has keyframe i alone; poses null: every keyframe at the identity
// GENERAL: joint_register's; the second halves are the second float4 of the 32-byte input records
template <bool GENERAL>
__global__ __launch_bounds__(NT) void cfear_joint_kernel(const rsx_cfear_surface_point *__restrict__ src, const int64_t *__restrict__ src_begin,
                                                         const int64_t *__restrict__ src_end, const rsx_cfear_surface_point *__restrict__ kfrec,
                                                         const int64_t *__restrict__ kf_begin, const int64_t *__restrict__ kf_end,
                                                         const int64_t *__restrict__ kf_job_off, const double *__restrict__ poses,
                                                         const double *__restrict__ init, int n_jobs, Rg<GENERAL> k, int search,
                                                         unsigned char *index, rsx_cfear_result *__restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ct_lds[];
  __shared__ double s_red[NW * N_SUMS];
  __shared__ KfFrame s_fr[MAXK];
  __shared__ KfDesc s_kf[MAXK];
  unsigned short *tables = reinterpret_cast<unsigned short *>(ct_lds);
  unsigned *sortbuf = reinterpret_cast<unsigned *>(ct_lds + LDS_TABLES);
  float4 *ws_sorted = reinterpret_cast<float4 *>(index + (size_t)blockIdx.x * WS_BYTES);
  unsigned *ws_keys = reinterpret_cast<unsigned *>(index + (size_t)blockIdx.x * WS_BYTES + WS_SORTED);
  const int t = threadIdx.x;
  for (int job = blockIdx.x; job < n_jobs; job += gridDim.x) {
    int64_t g0 = job, k64 = 1;
    if (kf_job_off) {
      g0 = kf_job_off[job];
      k64 = kf_job_off[job + 1] - g0;
    }
    const int64_t sb = src_begin[job], ns64 = src_end[job] - sb;
    double x = 0.0, y = 0.0, yaw = 0.0;
    if (init) {
      x = init[3 * (int64_t)job];
      y = init[3 * (int64_t)job + 1];
      yaw = init[3 * (int64_t)job + 2];
    }
    rsx_cfear_result res;
    if (k64 > MAXK) {  // (uniform; the host entry refuses such a job)
      res.x = x;
      res.y = y;
      res.yaw = yaw;
      res.cost = 0.0;
      res.iterations = res.correspondences = res.reserved = 0;
      res.status = 2;
      if (t == 0) out[job] = res;
      continue;
    }
    const int K = k64 < 0 ? 0 : (int)k64;
    __syncthreads();  // (the previous job's descriptors and tables are done with)
    if (t < K) {
      const int64_t g = g0 + t, b = kf_begin[g];
      KfDesc f;
      f.orig = reinterpret_cast<const float4 *>(kfrec + b);
      f.stride = 2;  // x, y, nx, ny: the first 16 bytes of a 32-byte record
      f.n = clamp_count(kf_end[g] - b);
      f.sorted = ws_sorted + (size_t)t * CAP;
      f.keys = ws_keys + (size_t)t * CAP;
      f.x = f.y = f.yaw = f.s = 0.0;
      f.c = 1.0;
      if (poses) {
        f.x = poses[3 * g];
        f.y = poses[3 * g + 1];
        f.yaw = poses[3 * g + 2];
        sincos(f.yaw, &f.s, &f.c);
      }
      f.slot = t;
      s_kf[t] = f;
    }
    __syncthreads();
    if (search == RSX_CFEAR_SEARCH_CELLS && ns64 > 0 && ns64 <= CAP)
      for (int c = 0; c < K; c++) {
        const int n = s_kf[c].n;
        if (n >= 1 && n <= CAP)
          build_index(s_kf[c].orig, 2, n, ws_keys + (size_t)c * CAP, ws_sorted + (size_t)c * CAP, tables + (size_t)c * NCELL, sortbuf, k.r, t);
      }
    joint_register<GENERAL>(reinterpret_cast<const float4 *>(src + sb), 2, reinterpret_cast<const float4 *>(src + sb) + 1, 2, ns64, K, s_kf, 1, search,
                            ct_lds, s_red, s_fr, k, x, y, yaw, res);
    if (t == 0) out[job] = res;
  }
}

// COMP: rsx_cfear_track_params.compensate as a template parameter: without it the kernel is the code it was (everything about compensation sits behind
// if constexpr), with it a scan is compensated into the state's copy before each of its two registrations
// GENERAL: joint_register's; the ring keeps its records' second halves at ST_EXTRA, written by these instances alone
template <bool COMP, bool GENERAL>
__global__ __launch_bounds__(NT) void cfear_track_kernel(const rsx_cfear_surface_point *__restrict__ rec, const float *__restrict__ tau,
                                                         const int64_t *__restrict__ begin, const int64_t *__restrict__ end,
                                                         const int32_t *__restrict__ n_scans, Rg<GENERAL> k,
                                                         TrConsts tc, unsigned char *state, rsx_cfear_track_result *__restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ct_lds[];
  __shared__ double s_red[NW * N_SUMS];
  __shared__ KfFrame s_fr[MAXK];
  __shared__ KfDesc s_kf[MAXK];
  unsigned short *tables = reinterpret_cast<unsigned short *>(ct_lds);
  unsigned *sortbuf = reinterpret_cast<unsigned *>(ct_lds + LDS_TABLES);
  const int seq = blockIdx.x, t = threadIdx.x;
  const int n = n_scans[seq];
  if (n <= 0) return;  // (uniform)
  int64_t first = 0;
  for (int q = 0; q < seq; q++) first += n_scans[q] > 0 ? n_scans[q] : 0;
  unsigned char *st = state + (size_t)seq * ST_BYTES;
  TrackHeader *hdr = reinterpret_cast<TrackHeader *>(st);
  float4 *orig = reinterpret_cast<float4 *>(st + ST_ORIG);
  float4 *sorted = reinterpret_cast<float4 *>(st + ST_INDEX);
  unsigned *keys = reinterpret_cast<unsigned *>(st + ST_INDEX + WS_SORTED);
  float *tau0 = reinterpret_cast<float *>(st + ST_TAU0);
  float4 *cbuf = reinterpret_cast<float4 *>(st + ST_COMP);
  float4 *extra = reinterpret_cast<float4 *>(st + ST_EXTRA);
  const int NK = tc.n_keyframes;
  double P[3], M[3];
  for (int a = 0; a < 3; a++) {
    P[a] = hdr->P[a];
    M[a] = hdr->M[a];
  }
  int head = hdr->head, n_ring = hdr->n_ring, started = hdr->started, first_kf = COMP ? hdr->first : 0;
  if (tc.search == RSX_CFEAR_SEARCH_CELLS && started) {  // the tables of the ring this launch continues with
    for (int c = t; c < MAXK * NCELL; c += NT) tables[c] = NO_CELL;
    __syncthreads();
    for (int c = 0; c < n_ring; c++) {
      const int slot = (head + c) % NK, cnt = hdr->kf_n[slot];
      if (cnt >= 1 && cnt <= CAP) fill_cell_table<NT, IDX_BITS, false>(keys + (size_t)slot * CAP, cnt, tables + (size_t)slot * NCELL, t);
    }
  }
  for (int s = 0; s < n; s++) {
    const int64_t scan = first + s, b = begin[scan], ns64 = end[scan] - b;
    const float4 *sp = reinterpret_cast<const float4 *>(rec + b);
    rsx_cfear_track_result r;
    r.reg.x = r.reg.y = r.reg.yaw = r.reg.cost = 0.0;
    r.reg.iterations = r.reg.correspondences = r.reg.status = r.reg.reserved = 0;
    r.keyframe = 0;
    r.n_keyframes = 0;
    bool insert = false;
    const float4 *cur = sp;  // the records the scan is registered with and, as a keyframe, stored as: sp, or its compensated copy
    int cstride = 2;         // x, y, nx, ny: the first 16 bytes of a 32-byte record
    if (!started) {
      started = 1;
      for (int a = 0; a < 3; a++) P[a] = M[a] = 0.0;
      head = n_ring = 0;
      r.keyframe = 1;
      insert = true;
      if constexpr (COMP) {  // the first keyframe stays as measured until the first motion is known
        first_kf = 1;
        if (ns64 <= CAP)
          for (int j = t; j < (int)ns64; j += NT) tau0[j] = tau[b + j];
      }
    } else {
      double start[3] = {P[0], P[1], P[2]};
      if (tc.predict) {
        double sn, cs;
        sincos(P[2], &sn, &cs);
        start[0] = P[0] + (cs * M[0] - sn * M[1]);
        start[1] = P[1] + (sn * M[0] + cs * M[1]);
        start[2] = P[2] + M[2];
      }
      __syncthreads();  // (the previous scan's descriptors are done with; what it wrote to the header is visible: see below)
      if (t < n_ring) {
        const int slot = (head + t) % NK;
        KfDesc f;
        f.orig = orig + (size_t)slot * CAP;
        f.stride = 1;
        f.n = hdr->kf_n[slot];
        f.sorted = sorted + (size_t)slot * CAP;
        f.keys = keys + (size_t)slot * CAP;
        f.x = hdr->kf_pose[slot][0];
        f.y = hdr->kf_pose[slot][1];
        f.yaw = hdr->kf_pose[slot][2];
        sincos(f.yaw, &f.s, &f.c);
        f.slot = slot;
        s_kf[t] = f;
      }
      __syncthreads();
      // Compensation (pass = 0, 1 are include/rsx.h's pass 1 and pass 2): pass 0 registers the scan compensated with the motion before it, from `start`.  After a pass 0 that succeeded M
      // becomes the motion it found and `start` the pose it found, and pass 1 registers the scan compensated with that M from that
      // `start`: a pass 1 that fails then leaves exactly them behind, by the failure rule below.  Without compensation there is pass 0
      // alone, on sp
      const bool comp = COMP && ns64 >= 1 && ns64 <= CAP;  // (otherwise pass 0 ends with status 1 or 2 and reads no record)
      int pass = 0, it0 = 0;
      bool ok;
      for (;; pass++) {
        if (COMP && comp) {
          const CompMotion m = comp_motion(M[0], M[1], M[2]);
          for (int j = t; j < (int)ns64; j += NT) {
            const float4 q = sp[2 * (size_t)j];
            cbuf[j] = m.how == 0 ? comp_record(q, tau[b + j], m) : q;
          }
          __threadfence_block();  // the workgroup reads the copy
          __syncthreads();
          cur = cbuf;
          cstride = 1;
        }
        joint_register<GENERAL>(cur, cstride, sp + 1, 2, ns64, n_ring, s_kf, (ptrdiff_t)((ST_EXTRA - ST_ORIG) / 16), tc.search, ct_lds, s_red, s_fr, k,
                                start[0], start[1], start[2], r.reg);
        ok = r.reg.status == 0 || r.reg.status == 8;
        if (!COMP || !ok || pass == 1) break;  // (uniform)
        it0 = r.reg.iterations;
        {
          double sn, cs;
          sincos(P[2], &sn, &cs);
          const double dx = r.reg.x - P[0], dy = r.reg.y - P[1];
          M[0] = cs * dx + sn * dy;
          M[1] = cs * dy - sn * dx;
          M[2] = r.reg.yaw - P[2];
          start[0] = r.reg.x;
          start[1] = r.reg.y;
          start[2] = r.reg.yaw;
        }
        if (first_kf) {  // the ring's only keyframe is the first scan as measured: compensated now, at its pose, and binned again
          const int slot = s_kf[0].slot, cnt = s_kf[0].n;
          if (cnt >= 1 && cnt <= CAP) {
            const CompMotion m = comp_motion(M[0], M[1], M[2]);
            if (m.how == 0)
              for (int j = t; j < cnt; j += NT) orig[(size_t)slot * CAP + j] = comp_record(orig[(size_t)slot * CAP + j], tau0[j], m);
            __threadfence_block();
            __syncthreads();
            if (tc.search == RSX_CFEAR_SEARCH_CELLS)
              build_index(orig + (size_t)slot * CAP, 1, cnt, keys + (size_t)slot * CAP, sorted + (size_t)slot * CAP,
                          tables + (size_t)slot * NCELL, sortbuf, k.r, t);
          }
          first_kf = 0;
        }
      }
      first_kf = 0;
      r.n_keyframes = n_ring;
      if (pass == 1) r.reg.reserved = it0;
      if (ok) {
        double sn, cs;
        sincos(P[2], &sn, &cs);
        const double dx = r.reg.x - P[0], dy = r.reg.y - P[1];
        M[0] = cs * dx + sn * dy;
        M[1] = cs * dy - sn * dx;
        M[2] = r.reg.yaw - P[2];
        P[0] = r.reg.x;
        P[1] = r.reg.y;
        P[2] = r.reg.yaw;
        const KfDesc &nw = s_kf[n_ring - 1];  // the newest keyframe
        const double dist = hypot(P[0] - nw.x, P[1] - nw.y), rot = fabs(remainder(P[2] - nw.yaw, 6.283185307179586));
        if (dist > tc.keyframe_distance || rot > tc.keyframe_rotation) {
          r.keyframe = 1;
          insert = true;
        }
      } else {
        for (int a = 0; a < 3; a++) P[a] = start[a];
        if (ns64 >= 1 && ns64 <= CAP) {
          r.keyframe = 2;
          head = n_ring = 0;
          insert = true;
        }
      }
    }
    if (insert) {  // (uniform) this scan at P joins the ring, in the oldest keyframe's slot when the ring is full
      int slot;
      if (n_ring < NK) {
        slot = (head + n_ring) % NK;
        n_ring++;
      } else {
        slot = head;
        head = (head + 1) % NK;
      }
      const int cnt = clamp_count(ns64);
      __syncthreads();  // (s_kf, read above, names the slot that is overwritten now)
      if (t == 0) {
        for (int a = 0; a < 3; a++) hdr->kf_pose[slot][a] = P[a];
        hdr->kf_n[slot] = cnt;
      }
      if (cnt <= CAP)
        for (int j = t; j < cnt; j += NT) {
          orig[(size_t)slot * CAP + j] = cur[(size_t)cstride * j];
          if constexpr (GENERAL) extra[(size_t)slot * CAP + j] = sp[2 * (size_t)j + 1];  // (the input record's, also of a compensated copy)
        }
      __threadfence_block();  // the workgroup reads the header and the records again
      __syncthreads();
      if (tc.search == RSX_CFEAR_SEARCH_CELLS && cnt >= 1 && cnt <= CAP)
        build_index(orig + (size_t)slot * CAP, 1, cnt, keys + (size_t)slot * CAP, sorted + (size_t)slot * CAP, tables + (size_t)slot * NCELL,
                    sortbuf, k.r, t);
    }
    if (t == 0) {
      r.x = P[0];
      r.y = P[1];
      r.yaw = P[2];
      out[scan] = r;
    }
  }
  if (t == 0) {
    for (int a = 0; a < 3; a++) {
      hdr->P[a] = P[a];
      hdr->M[a] = M[a];
    }
    hdr->head = head;
    hdr->n_ring = n_ring;
    hdr->started = started;
    hdr->first = first_kf;  // (without COMP: 0, the pad it was)
  }
}

template <bool GENERAL>
Rg<GENERAL> rg_consts(const rsx_cfear_params &p) {
  Rg<GENERAL> k;
  k.r = p.radius;
  k.r2 = p.radius * p.radius;
  k.cos_max = p.cos_max_normal_angle;
  k.delta = p.huber_delta;
  k.step_epsilon = p.step_epsilon;
  k.max_iterations = p.max_iterations;
  k.min_correspondences = p.min_correspondences;
  if constexpr (GENERAL) {
    k.cost = p.cost;
    k.loss = p.loss;
    k.weights = p.weights;
  }
  return k;
}

// the default objective runs the instances that know no other
bool general(const rsx_cfear_params &p) { return (p.cost | p.loss | p.weights) != 0; }

}  // namespace

using rsx::fail;

int rsx::cfear::check_track_params(const rsx_cfear_track_params &p) {
  if (p.n_keyframes < 1 || p.n_keyframes > RSX_CFEAR_MAX_KEYFRAMES)
    return fail(RSX_ERR_BAD_ARG, "n_keyframes %d outside [1, %d]", p.n_keyframes, RSX_CFEAR_MAX_KEYFRAMES);
  if (!(p.keyframe_distance >= 0.0) || !std::isfinite(p.keyframe_distance)) return fail(RSX_ERR_BAD_ARG, "keyframe_distance must not be negative");
  if (!(p.keyframe_rotation >= 0.0) || !std::isfinite(p.keyframe_rotation)) return fail(RSX_ERR_BAD_ARG, "keyframe_rotation must not be negative");
  if (p.predict != 0 && p.predict != 1) return fail(RSX_ERR_BAD_ARG, "predict %d is neither 0 nor 1", p.predict);
  if (p.search != RSX_CFEAR_SEARCH_CELLS && p.search != RSX_CFEAR_SEARCH_BRUTE) return fail(RSX_ERR_BAD_ARG, "search %d is neither 0 nor 1", p.search);
  if (p.reserved[0] || p.reserved[1]) return fail(RSX_ERR_BAD_ARG, "reserved words of rsx_cfear_track_params must be 0");
  if (p.compensate != 0 && p.compensate != 1) return fail(RSX_ERR_BAD_ARG, "compensate %d is neither 0 nor 1", p.compensate);
  return RSX_OK;
}

size_t rsx::cfear::keyframe_index_bytes(int32_t n_jobs) { return (size_t)(n_jobs < MAX_JOINT_BLOCKS ? n_jobs : MAX_JOINT_BLOCKS) * WS_BYTES; }

size_t rsx::cfear::track_state_bytes() { return ST_BYTES; }

int rsx::cfear::launch_register_keyframes(const rsx_cfear_surface_point *d_src, const int64_t *d_src_begin, const int64_t *d_src_end,
                                          const rsx_cfear_surface_point *d_kf, const int64_t *d_kf_begin, const int64_t *d_kf_end,
                                          const int64_t *d_kf_job_offsets, const double *d_kf_poses, int32_t n_jobs, const double *d_init,
                                          const rsx_cfear_params &p, const rsx_cfear_track_params &tp, void *d_index, rsx_cfear_result *d_out,
                                          hipStream_t s) {
  if (n_jobs < 1) return fail(RSX_ERR_BAD_ARG, "n_jobs %d below 1", n_jobs);
  const int blocks = n_jobs < MAX_JOINT_BLOCKS ? n_jobs : MAX_JOINT_BLOCKS;
  auto launch = [&](auto gen) {
    constexpr bool G = decltype(gen)::value;
    RSX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&cfear_joint_kernel<G>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES));
    hipLaunchKernelGGL(cfear_joint_kernel<G>, dim3((unsigned)blocks), dim3(NT), LDS_BYTES, s, d_src, d_src_begin, d_src_end, d_kf, d_kf_begin, d_kf_end,
                       d_kf_job_offsets, d_kf_poses, d_init, (int)n_jobs, rg_consts<G>(p), (int)tp.search, static_cast<unsigned char *>(d_index), d_out);
    RSX_HIP(hipGetLastError());
    return (int)RSX_OK;
  };
  return general(p) ? launch(std::true_type()) : launch(std::false_type());
}

int rsx::cfear::launch_register(const rsx_cfear_surface_point *d_src, const int64_t *d_src_begin, const int64_t *d_src_end,
                                const rsx_cfear_surface_point *d_dst, const int64_t *d_dst_begin, const int64_t *d_dst_end, int32_t n_pairs,
                                const double *d_init, const rsx_cfear_params &p, void *d_index, rsx_cfear_result *d_out, hipStream_t s) {
  if (n_pairs < 1) return fail(RSX_ERR_BAD_ARG, "n_pairs %d below 1", n_pairs);
  rsx_cfear_track_params tp;
  rsx_cfear_default_track_params(&tp);  // (only `search` acts: RSX_CFEAR_SEARCH_CELLS)
  return launch_register_keyframes(d_src, d_src_begin, d_src_end, d_dst, d_dst_begin, d_dst_end, nullptr, nullptr, n_pairs, d_init, p, tp, d_index,
                                   d_out, s);
}

int rsx::cfear::launch_track(const rsx_cfear_surface_point *d_records, const float *d_tau, const int64_t *d_begin, const int64_t *d_end,
                             const int32_t *d_n_scans,
                             int32_t n_sequences, const rsx_cfear_params &p, const rsx_cfear_track_params &tp, void *d_state,
                             rsx_cfear_track_result *d_out, hipStream_t s) {
  if (n_sequences < 1) return fail(RSX_ERR_BAD_ARG, "n_sequences %d below 1", n_sequences);
  if (tp.compensate && !d_tau) return fail(RSX_ERR_BAD_ARG, "compensate = 1 needs the records' times");
  TrConsts tc;
  tc.keyframe_distance = tp.keyframe_distance;
  tc.keyframe_rotation = tp.keyframe_rotation;
  tc.n_keyframes = tp.n_keyframes;
  tc.predict = tp.predict;
  tc.search = tp.search;
  auto launch = [&](auto comp, auto gen) {
    constexpr bool C = decltype(comp)::value, G = decltype(gen)::value;
    RSX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&cfear_track_kernel<C, G>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES));
    hipLaunchKernelGGL((cfear_track_kernel<C, G>), dim3((unsigned)n_sequences), dim3(NT), LDS_BYTES, s, d_records, d_tau, d_begin, d_end, d_n_scans,
                       rg_consts<G>(p), tc, static_cast<unsigned char *>(d_state), d_out);
    RSX_HIP(hipGetLastError());
    return (int)RSX_OK;
  };
  if (general(p)) return tp.compensate ? launch(std::true_type(), std::true_type()) : launch(std::false_type(), std::true_type());
  return tp.compensate ? launch(std::true_type(), std::false_type()) : launch(std::false_type(), std::false_type());
}

struct rsx_cfear_tracker {
  int device = 0;
  int32_t n_sequences = 0;
  std::mutex mu;
  rsx::Stream stream;
  rsx::StreamOrder order;  // the state and the staging buffers are shared by every call
  rsx::DevBuf state;       // [n_sequences][track_state_bytes()]
  rsx::DevBuf in, in_tau, off, nsc, out;  // staging of the host-buffer entries
  bool have_params = false;  // since create / reset
  rsx_cfear_params prm{};
  rsx_cfear_track_params tprm{};
};

namespace {

// A batch of registration jobs as the launch takes it, in host or in device memory; job_off and poses null: the pair entries
struct RegJobs {
  const rsx_cfear_surface_point *src, *kf;
  const int64_t *src_off, *kf_off, *job_off;
  const double *poses, *init;
  int32_t n, n_kf;  // jobs, keyframes in all
  rsx_cfear_result *out;
};

// the host-buffer forms: j's arrays into the handle's staging buffers; j names those afterwards
int stage_jobs(rsx_cfear *h, RegJobs &j, hipStream_t s) {
  const size_t n = (size_t)j.n, nk = (size_t)j.n_kf;
  RSX_TRY(rsx::stage_up(h->in0, j.src, (size_t)j.src_off[j.n] * sizeof(rsx_cfear_surface_point), s));
  RSX_TRY(rsx::stage_up(h->in1, j.kf, (size_t)j.kf_off[j.n_kf] * sizeof(rsx_cfear_surface_point), s));
  RSX_TRY(rsx::stage_up(h->off0, j.src_off, (n + 1) * 8, s));
  RSX_TRY(rsx::stage_up(h->off1, j.kf_off, (nk + 1) * 8, s));
  if (j.job_off) RSX_TRY(rsx::stage_up(h->job_off, j.job_off, (n + 1) * 8, s));
  if (j.poses) RSX_TRY(rsx::stage_up(h->poses, j.poses, nk * 24, s));
  if (j.init) RSX_TRY(rsx::stage_up(h->init, j.init, n * 24, s));
  RSX_TRY(rsx::stage_room(h->out, n * sizeof(rsx_cfear_result), s));
  j.src = h->in0.as<rsx_cfear_surface_point>();
  j.kf = h->in1.as<rsx_cfear_surface_point>();
  j.src_off = h->off0.as<int64_t>();
  j.kf_off = h->off1.as<int64_t>();
  if (j.job_off) j.job_off = h->job_off.as<int64_t>();
  if (j.poses) j.poses = h->poses.as<double>();
  if (j.init) j.init = h->init.as<double>();
  j.out = h->out.as<rsx_cfear_result>();
  return RSX_OK;
}

// The one path of the four registration entries: lock, device, stream order, (staging,) the index workspace, the launch.
// host: j is in host memory, the call goes through the handle's stream and returns with the results; otherwise j is in device
// memory and the call is asynchronous on `stream` (null: the handle's)
int register_jobs(rsx_cfear *h, RegJobs j, bool host, void *stream, const rsx_cfear_params &dp, const rsx_cfear_track_params &dt) {
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
  RSX_TRY(h->order.enter(s));
  rsx_cfear_result *host_out = j.out;
  if (host) RSX_TRY(stage_jobs(h, j, s));
  RSX_TRY(h->index.reserve(rsx::cfear::keyframe_index_bytes(j.n), s, false));
  RSX_TRY(rsx::cfear::launch_register_keyframes(j.src, j.src_off, j.src_off + 1, j.kf, j.kf_off, j.kf_off + 1, j.job_off, j.poses, j.n, j.init, dp, dt,
                                                h->index.p, j.out, s));
  if (!host) return RSX_OK;
  RSX_TRY(rsx::stage_down(host_out, h->out, (size_t)j.n * sizeof(rsx_cfear_result), s));
  RSX_HIP(hipStreamSynchronize(s));
  return RSX_OK;
}

// the parameters of a sequence stay: the first push since create / reset sets them
int same_params(rsx_cfear_tracker *h, const rsx_cfear_params &dp, const rsx_cfear_track_params &dt) {
  if (h->have_params && (std::memcmp(&h->prm, &dp, sizeof(dp)) != 0 || std::memcmp(&h->tprm, &dt, sizeof(dt)) != 0))
    return fail(RSX_ERR_BAD_ARG, "the parameters differ from the previous push's (rsx_cfear_tracker_reset first)");
  h->prm = dp;
  h->tprm = dt;
  h->have_params = true;
  return RSX_OK;
}

// the untimed entries pass tau = null and refuse compensation: they have no times to compensate with
int untimed_ok(const float *tau, const rsx_cfear_track_params &dt) {
  if (!tau && dt.compensate) return fail(RSX_ERR_BAD_ARG, "compensate = 1 needs the records' times (rsx_cfear_tracker_push_timed)");
  return RSX_OK;
}

int push_device(rsx_cfear_tracker *h, const rsx_cfear_surface_point *d_records, const float *d_tau, const int64_t *d_offsets,
                const int32_t *d_n_scans, const rsx_cfear_params *params, const rsx_cfear_track_params *track, rsx_cfear_track_result *d_out,
                void *stream) {
  if (!h || !d_records || !d_offsets || !d_n_scans || !d_out) return fail(RSX_ERR_BAD_ARG, "bad arg");
  rsx_cfear_params dp;
  rsx_cfear_track_params dt;
  RSX_TRY(rsx::cfear::resolve(params, track, dp, &dt));
  RSX_TRY(untimed_ok(d_tau, dt));
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_TRY(same_params(h, dp, dt));
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
  RSX_TRY(h->order.enter(s));
  return rsx::cfear::launch_track(d_records, d_tau, d_offsets, d_offsets + 1, d_n_scans, h->n_sequences, dp, dt, h->state.p, d_out, s);
}

int push_host(rsx_cfear_tracker *h, const rsx_cfear_surface_point *records, const float *tau, const int64_t *offsets, const int32_t *n_scans,
              const rsx_cfear_params *params, const rsx_cfear_track_params *track, rsx_cfear_track_result *out, const char *what) {
  if (!h || !records || !offsets || !n_scans || !out) return fail(RSX_ERR_BAD_ARG, "bad arg");
  rsx_cfear_params dp;
  rsx_cfear_track_params dt;
  RSX_TRY(rsx::cfear::resolve(params, track, dp, &dt));
  RSX_TRY(untimed_ok(tau, dt));
  int64_t total = 0;
  for (int32_t q = 0; q < h->n_sequences; q++) {
    if (n_scans[q] < 0) return fail(RSX_ERR_BAD_ARG, "n_scans[%d] = %d is negative", q, n_scans[q]);
    total += n_scans[q];
  }
  if (total > INT32_MAX) return fail(RSX_ERR_BAD_ARG, "too many scans");
  if (total > 0) RSX_TRY(rsx::check_offsets(offsets, (int32_t)total, what));
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_TRY(same_params(h, dp, dt));
  if (total == 0) return RSX_OK;
  const size_t n = (size_t)total, m = (size_t)offsets[total];
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  RSX_TRY(h->order.enter(s));
  RSX_TRY(rsx::stage_up(h->in, records, m * sizeof(rsx_cfear_surface_point), s));
  if (tau) RSX_TRY(rsx::stage_up(h->in_tau, tau, m * 4, s));
  RSX_TRY(rsx::stage_up(h->off, offsets, (n + 1) * 8, s));
  RSX_TRY(rsx::stage_up(h->nsc, n_scans, (size_t)h->n_sequences * 4, s));
  RSX_TRY(rsx::stage_room(h->out, n * sizeof(rsx_cfear_track_result), s));
  RSX_TRY(rsx::cfear::launch_track(h->in.as<rsx_cfear_surface_point>(), tau ? h->in_tau.as<float>() : nullptr, h->off.as<int64_t>(),
                                   h->off.as<int64_t>() + 1, h->nsc.as<int32_t>(), h->n_sequences, dp, dt, h->state.p,
                                   h->out.as<rsx_cfear_track_result>(), s));
  RSX_TRY(rsx::stage_down(out, h->out, n * sizeof(rsx_cfear_track_result), s));
  RSX_HIP(hipStreamSynchronize(s));
  return RSX_OK;
}

}  // namespace

extern "C" {

int rsx_cfear_default_track_params(rsx_cfear_track_params *p) try {
  if (!p) return fail(RSX_ERR_BAD_ARG, "null params");
  p->keyframe_distance = 1.5;
  p->keyframe_rotation = 0.08726646259971647;  // 5 deg
  p->n_keyframes = 3;
  p->predict = 1;
  p->search = RSX_CFEAR_SEARCH_CELLS;
  p->reserved[0] = p->reserved[1] = 0;
  p->compensate = 0;
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_cfear_register_batch_device(rsx_cfear *h, const rsx_cfear_surface_point *d_src, const int64_t *d_src_offsets,
                                    const rsx_cfear_surface_point *d_dst, const int64_t *d_dst_offsets, int32_t n_pairs,
                                    const double *d_init, const rsx_cfear_params *params, rsx_cfear_result *d_out, void *stream) try {
  if (!h || !d_src || !d_src_offsets || !d_dst || !d_dst_offsets || !d_out || n_pairs < 0) return fail(RSX_ERR_BAD_ARG, "bad arg");
  rsx_cfear_params dp;
  rsx_cfear_track_params dt;
  RSX_TRY(resolve(params, nullptr, dp, &dt));
  if (n_pairs == 0) return RSX_OK;
  return register_jobs(h, {d_src, d_dst, d_src_offsets, d_dst_offsets, nullptr, nullptr, d_init, n_pairs, n_pairs, d_out}, false, stream, dp, dt);
} RSX_CATCH_ALL

int rsx_cfear_register_batch(rsx_cfear *h, const rsx_cfear_surface_point *src, const int64_t *src_offsets,
                             const rsx_cfear_surface_point *dst, const int64_t *dst_offsets, int32_t n_pairs, const double *init,
                             const rsx_cfear_params *params, rsx_cfear_result *out) try {
  if (!h || !src || !src_offsets || !dst || !dst_offsets || !out || n_pairs < 0) return fail(RSX_ERR_BAD_ARG, "bad arg");
  rsx_cfear_params dp;
  rsx_cfear_track_params dt;
  RSX_TRY(resolve(params, nullptr, dp, &dt));
  if (n_pairs == 0) return RSX_OK;
  RSX_TRY(rsx::check_offsets(src_offsets, n_pairs, "rsx_cfear_register_batch (src)"));
  RSX_TRY(rsx::check_offsets(dst_offsets, n_pairs, "rsx_cfear_register_batch (dst)"));
  return register_jobs(h, {src, dst, src_offsets, dst_offsets, nullptr, nullptr, init, n_pairs, n_pairs, out}, true, nullptr, dp, dt);
} RSX_CATCH_ALL

int rsx_cfear_register_keyframes_batch_device(rsx_cfear *h, const rsx_cfear_surface_point *d_src, const int64_t *d_src_offsets,
                                              const rsx_cfear_surface_point *d_kf, const int64_t *d_kf_offsets,
                                              const int64_t *d_kf_job_offsets, const double *d_kf_poses, int32_t n_jobs,
                                              const double *d_init, const rsx_cfear_params *params,
                                              const rsx_cfear_track_params *track, rsx_cfear_result *d_out, void *stream) try {
  if (!h || !d_src || !d_src_offsets || !d_kf || !d_kf_offsets || !d_kf_job_offsets || !d_kf_poses || !d_out || n_jobs < 0)
    return fail(RSX_ERR_BAD_ARG, "bad arg");
  rsx_cfear_params dp;
  rsx_cfear_track_params dt;
  RSX_TRY(resolve(params, track, dp, &dt));
  if (n_jobs == 0) return RSX_OK;
  return register_jobs(h, {d_src, d_kf, d_src_offsets, d_kf_offsets, d_kf_job_offsets, d_kf_poses, d_init, n_jobs, 0, d_out}, false, stream, dp, dt);
} RSX_CATCH_ALL

int rsx_cfear_register_keyframes_batch(rsx_cfear *h, const rsx_cfear_surface_point *src, const int64_t *src_offsets,
                                       const rsx_cfear_surface_point *kf, const int64_t *kf_offsets, const int64_t *kf_job_offsets,
                                       const double *kf_poses, int32_t n_jobs, const double *init, const rsx_cfear_params *params,
                                       const rsx_cfear_track_params *track, rsx_cfear_result *out) try {
  if (!h || !src || !src_offsets || !kf || !kf_offsets || !kf_job_offsets || !kf_poses || !out || n_jobs < 0) return fail(RSX_ERR_BAD_ARG, "bad arg");
  rsx_cfear_params dp;
  rsx_cfear_track_params dt;
  RSX_TRY(resolve(params, track, dp, &dt));
  if (n_jobs == 0) return RSX_OK;
  RSX_TRY(rsx::check_offsets(src_offsets, n_jobs, "rsx_cfear_register_keyframes_batch (src)"));
  RSX_TRY(rsx::check_offsets(kf_job_offsets, n_jobs, "rsx_cfear_register_keyframes_batch (jobs)"));
  for (int32_t i = 0; i < n_jobs; i++) {
    const int64_t nk = kf_job_offsets[i + 1] - kf_job_offsets[i];
    if (nk < 1 || nk > RSX_CFEAR_MAX_KEYFRAMES)
      return fail(RSX_ERR_BAD_ARG, "job %d has %lld keyframes, outside [1, %d]", i, (long long)nk, RSX_CFEAR_MAX_KEYFRAMES);
  }
  if (kf_job_offsets[n_jobs] > INT32_MAX) return fail(RSX_ERR_BAD_ARG, "too many keyframes");
  const int32_t n_kf = (int32_t)kf_job_offsets[n_jobs];
  RSX_TRY(rsx::check_offsets(kf_offsets, n_kf, "rsx_cfear_register_keyframes_batch (keyframes)"));
  return register_jobs(h, {src, kf, src_offsets, kf_offsets, kf_job_offsets, kf_poses, init, n_jobs, n_kf, out}, true, nullptr, dp, dt);
} RSX_CATCH_ALL

int rsx_cfear_tracker_create(int device, int32_t n_sequences, rsx_cfear_tracker **out) try {
  if (!out) return fail(RSX_ERR_BAD_ARG, "null out");
  *out = nullptr;
  if (n_sequences < 1 || n_sequences > 4096) return fail(RSX_ERR_BAD_ARG, "n_sequences %d outside [1, 4096]", n_sequences);
  RSX_TRY(rsx::check_device(device));
  std::unique_ptr<rsx_cfear_tracker> h(new (std::nothrow) rsx_cfear_tracker());
  if (!h) return fail(RSX_ERR_OOM, "host alloc");
  h->device = device;
  h->n_sequences = n_sequences;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = h->stream.create();
  if (e != hipSuccess) return fail(RSX_ERR_HIP, "create: %s", hipGetErrorString(e));
  const size_t bytes = (size_t)n_sequences * rsx::cfear::track_state_bytes();
  RSX_TRY(h->state.reserve(bytes, h->stream, false));
  RSX_HIP(hipMemsetAsync(h->state.p, 0, bytes, h->stream));
  RSX_HIP(hipStreamSynchronize(h->stream));
  *out = h.release();
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_cfear_tracker_destroy(rsx_cfear_tracker *h) try {
  if (!h) return RSX_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  delete h;
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_cfear_tracker_reset(rsx_cfear_tracker *h) try {
  if (!h) return fail(RSX_ERR_BAD_ARG, "null handle");
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  RSX_TRY(h->order.enter(s));
  // (the headers alone decide: a sequence whose header is zero has seen no scan)
  RSX_HIP(hipMemsetAsync(h->state.p, 0, (size_t)h->n_sequences * rsx::cfear::track_state_bytes(), s));
  RSX_HIP(hipStreamSynchronize(s));
  h->have_params = false;
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_cfear_tracker_push_device(rsx_cfear_tracker *h, const rsx_cfear_surface_point *d_records, const int64_t *d_offsets,
                                  const int32_t *d_n_scans, const rsx_cfear_params *params, const rsx_cfear_track_params *track,
                                  rsx_cfear_track_result *d_out, void *stream) try {
  return push_device(h, d_records, nullptr, d_offsets, d_n_scans, params, track, d_out, stream);
} RSX_CATCH_ALL

int rsx_cfear_tracker_push(rsx_cfear_tracker *h, const rsx_cfear_surface_point *records, const int64_t *offsets, const int32_t *n_scans,
                           const rsx_cfear_params *params, const rsx_cfear_track_params *track, rsx_cfear_track_result *out) try {
  return push_host(h, records, nullptr, offsets, n_scans, params, track, out, "rsx_cfear_tracker_push");
} RSX_CATCH_ALL

int rsx_cfear_tracker_push_timed_device(rsx_cfear_tracker *h, const rsx_cfear_surface_point *d_records, const float *d_tau,
                                        const int64_t *d_offsets, const int32_t *d_n_scans, const rsx_cfear_params *params,
                                        const rsx_cfear_track_params *track, rsx_cfear_track_result *d_out, void *stream) try {
  if (!d_tau) return fail(RSX_ERR_BAD_ARG, "bad arg");
  return push_device(h, d_records, d_tau, d_offsets, d_n_scans, params, track, d_out, stream);
} RSX_CATCH_ALL

int rsx_cfear_tracker_push_timed(rsx_cfear_tracker *h, const rsx_cfear_surface_point *records, const float *tau, const int64_t *offsets,
                                 const int32_t *n_scans, const rsx_cfear_params *params, const rsx_cfear_track_params *track,
                                 rsx_cfear_track_result *out) try {
  if (!tau) return fail(RSX_ERR_BAD_ARG, "bad arg");
  return push_host(h, records, tau, offsets, n_scans, params, track, out, "rsx_cfear_tracker_push_timed");
} RSX_CATCH_ALL

}  // extern "C"
