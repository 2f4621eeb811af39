// rsx_wave_dev.h -- the 64-lane building blocks every kernel here shares: DPP moves, v_readlane, reductions, scans and the
// LDS fence of one wavefront.  Device-only, header-only, a flat list.
//
// WHY DPP: a __shfl_xor / __shfl_up step is a ds_bpermute round trip through the LDS crossbar (two for a 64-bit value), and
// the steps of a reduction depend on each other: ~1.2 k cycles for one 64-bit butterfly, and the wavefronts of a workgroup
// queue on the LDS pipe.  A DPP step is an operand modifier of a VALU instruction inside a row of 16 lanes; the four rows
// meet through v_readlane (or the two row broadcasts).  Use the DPP forms in anything hot; `butterfly` is for cold code and
// for the sites whose ORDER OF ADDITIONS is the xor ladder's.
//
// ORDER IS PART OF THE CONTRACT.  The project's results are bit-identical to its oracles, so a floating-point sum must keep
// the order its oracle restates.  Three orders exist, each under its own name; never swap one for another:
//   sum_f64_rows_seq   rows by the tree below, then ((r0 + r1) + r2) + r3
//   sum_f64_rows_pair  rows by the tree below, then (r0 + r1) + (r2 + r3)
//   butterfly(v, +)    xor ladder 32, 16, 8, 4, 2, 1
// (sum_f32_bcast is a fourth, fp32 only.)  Integer sums, minima and maxima have no order; the float minima and maxima assume
// that no lane holds a NaN.
//
// THE ROW TREE (row_reduce): lane l of a row of 16 combines, in this order, with lane l ^ 1 (quad_perm [1,0,3,2]), l ^ 2
// (quad_perm [2,3,0,1]), 7 - l inside its half (row_half_mirror) and 15 - l (row_mirror).  After step k every lane holds the
// combination of an aligned group of 2^k lanes, so for a commutative op the row's result is the balanced tree
// ((x0 . x1) . (x2 . x3)) . ((x4 . x5) . (x6 . x7))  .  the same of x8..x15, in every lane of the row.
#pragma once
#include <hip/hip_runtime.h>

namespace rsx {
namespace wave {

// DPP move of a 32- or 64-bit value (int, unsigned, float, unsigned long long, double): lane l reads x of the lane CTRL
// names.  One operand form: old = 0, bank_mask = 0xf, bound_ctrl exactly when every row is enabled -- so a lane without a
// source, and every lane of a row outside ROWS, reads 0, with no register to preset in front of the move.
// The caller guarantees:
//  * the WHOLE wavefront is active at the call (no lane-dependent branch around it, no early return of part of the wave):
//    a lane whose source lane is inactive reads 0 with bound_ctrl and keeps `old` without it, never x;
//  * for shift and broadcast controls, 0 is the identity or lower bound it wants in the lanes without a source.
template <int CTRL, int ROWS = 0xf, class T>
__device__ __forceinline__ T dpp(T x) {
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "a 32- or 64-bit value");
  if constexpr (sizeof(T) == 4) {
    return __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, ROWS, 0xf, ROWS == 0xf));
  } else {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, x);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)u, CTRL, ROWS, 0xf, ROWS == 0xf);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(u >> 32), CTRL, ROWS, 0xf, ROWS == 0xf);
    return __builtin_bit_cast(T, ((unsigned long long)hi << 32) | lo);
  }
}
// (uniform) x of lane l, l wave-uniform: one v_readlane per 32 bits
template <class T>
__device__ __forceinline__ T readlane(T x, int l) {
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "a 32- or 64-bit value");
  if constexpr (sizeof(T) == 4) {
    return __builtin_bit_cast(T, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), l));
  } else {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, x);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, l), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), l);
    return __builtin_bit_cast(T, ((unsigned long long)hi << 32) | lo);
  }
}

struct Add {  // a + b as an op for the reductions below (with -ffp-contract=off: one rounding)
  template <class T>
  __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};

// every lane: op over its row of 16 lanes, in the order of THE ROW TREE above
template <class T, class Op>
__device__ __forceinline__ T row_reduce(T x, Op op) {
  x = op(x, dpp<0xB1>(x));   // quad_perm [1,0,3,2]
  x = op(x, dpp<0x4E>(x));   // quad_perm [2,3,0,1]
  x = op(x, dpp<0x141>(x));  // row_half_mirror
  x = op(x, dpp<0x140>(x));  // row_mirror: every lane = its row's result
  return x;
}
// (uniform) the four rows' results, rows 0 and 1 first, then rows 2 and 3: (r0 . r1) . (r2 . r3)
template <class T, class Op>
__device__ __forceinline__ T rows_pair(T x, Op op) {
  return op(op(readlane(x, 0), readlane(x, 16)), op(readlane(x, 32), readlane(x, 48)));
}

// ---- reductions over the 64 lanes, (uniform) result: row tree, then lanes 0, 16, 32, 48 ----
__device__ __forceinline__ int sum_i32(int x) {
  x = row_reduce(x, Add{});
  return readlane(x, 0) + readlane(x, 16) + readlane(x, 32) + readlane(x, 48);
}
__device__ __forceinline__ int max_i32(int x) {
  auto mx = [](int a, int b) { return a > b ? a : b; };
  return rows_pair(row_reduce(x, mx), mx);
}
__device__ __forceinline__ unsigned max_u32(unsigned x) {
  auto mx = [](unsigned a, unsigned b) { return a > b ? a : b; };
  return rows_pair(row_reduce(x, mx), mx);
}
template <bool MAX>
__device__ __forceinline__ unsigned long long minmax_u64(unsigned long long x) {
  auto pick = [](unsigned long long a, unsigned long long b) { return MAX ? (a > b ? a : b) : (a < b ? a : b); };
  return rows_pair(row_reduce(x, pick), pick);
}
__device__ __forceinline__ float min_f32(float x) {  // no NaN; -0.0 counts as below +0.0 (v_min_f32)
  auto mn = [](float a, float b) { return fminf(a, b); };
  return rows_pair(row_reduce(x, mn), mn);
}
// fp64 sums: the rows by the row tree, then the four rows' sums in the order the name says
__device__ __forceinline__ double sum_f64_rows_seq(double x) {  // ((r0 + r1) + r2) + r3
  x = row_reduce(x, Add{});
  return ((readlane(x, 0) + readlane(x, 16)) + readlane(x, 32)) + readlane(x, 48);
}
__device__ __forceinline__ double sum_f64_rows_pair(double x) {  // (r0 + r1) + (r2 + r3)
  return rows_pair(row_reduce(x, Add{}), Add{});
}
// fp32 sum, rows by the row tree, then the two row broadcasts: row 1 += r0, row 3 += r2 (row_bcast:15), then rows 2 and 3
// += the last lane of row 1 (row_bcast:31); the result is lane 63's, (r2 + r3) + (r0 + r1)
__device__ __forceinline__ float sum_f32_bcast(float x) {
  x = row_reduce(x, Add{});
  x += dpp<0x142, 0xa>(x);  // row_bcast:15 into rows 1, 3
  x += dpp<0x143, 0xc>(x);  // row_bcast:31 into rows 2, 3
  return readlane(x, 63);
}

// ---- xor butterfly: every lane ends with v = op(v, v of lane ^ 32), then ^ 16, 8, 4, 2, 1, in THIS order -- for a
// floating-point sum the order of additions is the result.  Any type __shfl_xor takes; twelve dependent ds_bpermute for a
// 64-bit one, so for cold code and for the sums that are defined by this order ----
template <class T, class Op>
__device__ __forceinline__ T butterfly(T v, Op op) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = op(v, __shfl_xor(v, off));
  return v;
}
// the same for an unsigned 64-bit value, moved as two 32-bit words
template <class Op>
__device__ __forceinline__ unsigned long long butterfly_u64(unsigned long long v, Op op) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned long long x = ((unsigned long long)(unsigned)__shfl_xor((int)(unsigned)(v >> 32), off) << 32) | (unsigned long long)(unsigned)__shfl_xor((int)(unsigned)v, off);
    v = op(v, x);
  }
  return v;
}

// ---- inclusive scans over the 64 lanes: Hillis-Steele inside each row of 16 by DPP shifts (a lane without a source reads 0:
// the identity of + and the lower bound of the unsigned and key maxima); across the rows forward by the two row broadcasts of
// the ISA (row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3), backward -- there is no broadcast of a row's
// FIRST lane -- by three v_readlane ----
__device__ __forceinline__ unsigned incl_add_u32(unsigned x) {
  x += dpp<0x111>(x);  // row_shr:1
  x += dpp<0x112>(x);  // row_shr:2
  x += dpp<0x114>(x);  // row_shr:4
  x += dpp<0x118>(x);  // row_shr:8
  x += dpp<0x142, 0xa>(x);  // row_bcast:15
  x += dpp<0x143, 0xc>(x);  // row_bcast:31
  return x;
}
__device__ __forceinline__ unsigned incl_max_u32(unsigned x) {
  auto mx = [](unsigned a, unsigned b) { return a > b ? a : b; };
  x = mx(x, dpp<0x111>(x));
  x = mx(x, dpp<0x112>(x));
  x = mx(x, dpp<0x114>(x));
  x = mx(x, dpp<0x118>(x));
  x = mx(x, dpp<0x142, 0xa>(x));
  x = mx(x, dpp<0x143, 0xc>(x));
  return x;
}
// max-scan of doubles that are all >= 0.0 (REV: from lane 63 down); mx(a, b) is the caller's maximum of two such values
template <bool REV, class Max>
__device__ __forceinline__ double incl_max_f64(double x, int lane, Max mx) {
  if constexpr (!REV) {
    x = mx(x, dpp<0x111>(x));  // row_shr:1
    x = mx(x, dpp<0x112>(x));  // row_shr:2
    x = mx(x, dpp<0x114>(x));  // row_shr:4
    x = mx(x, dpp<0x118>(x));  // row_shr:8
    x = mx(x, dpp<0x142, 0xa>(x));  // row_bcast:15
    x = mx(x, dpp<0x143, 0xc>(x));  // row_bcast:31
    return x;
  } else {
    x = mx(x, dpp<0x101>(x));  // row_shl:1
    x = mx(x, dpp<0x102>(x));
    x = mx(x, dpp<0x104>(x));
    x = mx(x, dpp<0x108>(x));
    const double t3 = readlane(x, 48), t2 = mx(t3, readlane(x, 32)), t1 = mx(t2, readlane(x, 16));
    const double suf = lane >= 48 ? 0.0 : (lane >= 32 ? t3 : (lane >= 16 ? t2 : t1));
    return mx(x, suf);
  }
}

__device__ __forceinline__ void lds_fence() {
  // LDS operations of one wave execute in order; this only stops the compiler from moving LDS
  // accesses across the point where lanes exchange data through LDS.
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

}  // namespace wave
}  // namespace rsx
