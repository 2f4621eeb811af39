// cfear_dev.h -- the device code csrc/cfear.hip (surface points), csrc/cfear_track.hip (registration) and csrc/coral.hip
// (alignment quality) need: the 128 x 128 grid of cells of one radius, points / records sorted by cell in LDS, the walk of a
// 3 x 3 block of cells, and the motion compensation of a record.  A key is cell << IDX_BITS | index, all
// ones for an element outside the grid; sorted keys order the elements by cell and, inside a cell, by index.  Everything is
// __forceinline__: a kernel keeps the instruction sequence it had with the code written out in place.
#pragma once
#include <hip/hip_runtime.h>

#include "mocomp_dev.h"

namespace rsx {
namespace cfear {

constexpr int GRID = 128, HALF = 64, NCELL = GRID * GRID;
constexpr unsigned NO_KEY = 0xFFFFFFFFu;
constexpr unsigned short NO_CELL = 0xFFFF;

// bitonic sort of keys[0 .. n2) in LDS, ascending, by a workgroup of NT threads (thread t); n2 a power of two >= NT.  Called
// behind a barrier, ends behind one
template <int NT>
__device__ __forceinline__ void bitonic_sort_lds(unsigned *keys, unsigned n2, int t) {
  for (unsigned kk = 2; kk <= n2; kk <<= 1)
    for (unsigned j = kk >> 1; j > 0; j >>= 1) {
      for (unsigned i = t; i < n2; i += NT) {
        const unsigned l = i ^ j;
        if (l > i) {
          const unsigned a = keys[i], c = keys[l];
          if ((a > c) == ((i & kk) == 0)) {
            keys[i] = c;
            keys[l] = a;
          }
        }
      }
      __syncthreads();
    }
}

// table[cell] = the first sorted position of the cell, from the sorted keys[0 .. n) (LDS or HBM); the other entries of the
// table (NO_CELL: an empty cell) stay.  OUTSIDE: some of the n keys may be NO_KEY (they sort to the end and have no cell).  No barrier
template <int NT, unsigned IDX_BITS, bool OUTSIDE>
__device__ __forceinline__ void fill_cell_table(const unsigned *keys, int n, unsigned short *table, int t) {
  for (int i = t; i < n; i += NT) {
    const unsigned key = keys[i];
    if (OUTSIDE && key == NO_KEY) continue;
    if (i == 0 || (keys[i - 1] >> IDX_BITS) != (key >> IDX_BITS)) table[key >> IDX_BITS] = (unsigned short)i;
  }
}

// f(index) for every element of the 3 x 3 block of cells around (ix, iy), from the sorted keys[0 .. n) and their cell table:
// dy outer, dx inner, ascending index inside a cell; cells off the grid are skipped
template <unsigned IDX_BITS, typename F>
__device__ __forceinline__ void for_block(const unsigned *keys, const unsigned short *start, unsigned n, int ix, int iy, F &&f) {
  for (int dy = -1; dy <= 1; dy++)
    for (int dx = -1; dx <= 1; dx++) {
      const int jx = ix + dx, jy = iy + dy;
      if (jx < 0 || jx >= GRID || jy < 0 || jy >= GRID) continue;
      const unsigned cc = (unsigned)(jy * GRID + jx);
      unsigned k = start[cc];
      if (k == NO_CELL) continue;
      for (; k < n && (keys[k] >> IDX_BITS) == cc; k++) f(keys[k] & ((1u << IDX_BITS) - 1u));
    }
}

// Motion compensation of surface-point records (include/rsx.h, rsx_cfear_compensate_batch; tests/cfear_mocomp_np.py): the
// deskewing of csrc/mocomp.hip with dt_scan = 1 and no Doppler term, on a record's mean and normal.
struct CompMotion {
  double vx, vy, wz;
  int how;  // 0 compensate; 1 copy (the motion is exactly zero); 2 copy and flag (not |yaw| <= 1/2, or not finite)
};

__device__ __forceinline__ CompMotion comp_motion(double x, double y, double yaw) {
  CompMotion m;
  m.how = rsx::mocomp::velocity_of(x, y, yaw, 1.0, m.vx, m.vy, m.wz) ? 0 : 2;
  if (x == 0.0 && y == 0.0 && yaw == 0.0) m.how = 1;
  return m;
}

// q = (x, y, nx, ny) measured at tau (a fraction of the scan period) under m (how == 0)
__device__ __forceinline__ float4 comp_record(float4 q, float tau_f, const CompMotion &m) {
  const double x = (double)q.x, y = (double)q.y, nx = (double)q.z, ny = (double)q.w, tau = (double)tau_f;
  const rsx::mocomp::Poly f = rsx::mocomp::poly(m.wz * tau);
  const double x0 = (f.cs * x - f.sn * y) + (f.A * m.vx - f.B * m.vy) * tau;
  const double y0 = (f.sn * x + f.cs * y) + (f.B * m.vx + f.A * m.vy) * tau;
  return make_float4((float)x0, (float)y0, (float)(f.cs * nx - f.sn * ny), (float)(f.sn * nx + f.cs * ny));
}

}  // namespace cfear
}  // namespace rsx
