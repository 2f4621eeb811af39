// mocomp_dev.h -- the device code csrc/mocomp.hip (keypoints and matches) and the CFEAR record compensation (csrc/cfear_dev.h:
// csrc/cfear.hip, csrc/cfear_track.hip) both need: the fixed polynomials of the deskewing model and the velocity of a pose.  One
// copy, __forceinline__: a kernel keeps the instruction sequence it had with the code written out in place.  A file that includes
// this switches contraction off (#pragma STDC FP_CONTRACT OFF; the library is built with -ffp-contract=off as well).
//
// The polynomials.  With u = th^2 and Horner sums over k >= 1
//     q_S = sum_{k=1..6} (-1)^k u^k / (2k+1)!      sin th = th + th q_S        A = sin th / th       = 1 + q_S
//     q_C = sum_{k=1..7} (-1)^k u^k / (2k)!        cos th = 1 + q_C
//     q_D = sum_{k=1..6} (-1)^k u^k / (2k+2)!      B = (1 - cos th) / th = th / 2 + th q_D
// Truncation bound for |th| <= 1/2, i.e. u <= 1/4.  Each is the Taylor series of its function cut after the term shown; the
// series alternate and their terms decrease in magnitude (ratio of consecutive terms <= u / 6 < 1), so the error is smaller
// than the first omitted term:
//     sin, A:  u^7 / 15!  relative to  sin th / th >= sin(1/2) / (1/2) = 0.9588..:  4^-7 / 15! / 0.9588 = 4.87e-17
//     cos:     u^8 / 16!  relative to  cos th >= cos(1/2) = 0.8775..:               4^-8 / 16! / 0.8775 = 8.31e-19
//     B:       u^7 / 16!  relative to  B / th >= (1 - cos(1/2)) / (1/4) = 0.4896..: 4^-7 / 16! / 0.4896 = 5.96e-18
// all below 2^-53 = 1.11e-16.  (One term fewer would not do: 4^-6 / 13! / 0.9588 = 4.1e-14 for sin, 4^-7 / 14! / 0.8775 =
// 8.0e-16 for cos, 4^-6 / 14! / 0.4896 = 5.7e-15 for B.)  The "1 + small" forms keep the rounding error of the evaluation
// near half an ulp: tests/test_mocomp_restatement.py checks <= 1 ulp against a 50-digit evaluation on a dense grid.
#pragma once
#include <hip/hip_runtime.h>

namespace rsx {
namespace mocomp {

constexpr double TH_MAX = 0.5;

constexpr double S1 = -1.0 / 6.0, S2 = 1.0 / 120.0, S3 = -1.0 / 5040.0, S4 = 1.0 / 362880.0, S5 = -1.0 / 39916800.0, S6 = 1.0 / 6227020800.0;
constexpr double C1 = -1.0 / 2.0, C2 = 1.0 / 24.0, C3 = -1.0 / 720.0, C4 = 1.0 / 40320.0, C5 = -1.0 / 3628800.0, C6 = 1.0 / 479001600.0,
                 C7 = -1.0 / 87178291200.0;
constexpr double D1 = -1.0 / 24.0, D2 = 1.0 / 720.0, D3 = -1.0 / 40320.0, D4 = 1.0 / 3628800.0, D5 = -1.0 / 479001600.0,
                 D6 = 1.0 / 87178291200.0;

struct Poly {
  double sn, cs, A, B;
};

__device__ __forceinline__ Poly poly(double th) {
  const double u = th * th;
  double s = S6;
  s = S5 + u * s;
  s = S4 + u * s;
  s = S3 + u * s;
  s = S2 + u * s;
  s = S1 + u * s;
  const double qs = u * s;
  double c = C7;
  c = C6 + u * c;
  c = C5 + u * c;
  c = C4 + u * c;
  c = C3 + u * c;
  c = C2 + u * c;
  c = C1 + u * c;
  double d = D6;
  d = D5 + u * d;
  d = D4 + u * d;
  d = D3 + u * d;
  d = D2 + u * d;
  d = D1 + u * d;
  Poly f;
  f.A = 1.0 + qs;
  f.sn = th + th * qs;
  f.cs = 1.0 + u * c;
  f.B = 0.5 * th + th * (u * d);
  return f;
}

// log(pose) / dt_scan; false: the pose has no velocity here (not |yaw| <= 1/2, or x, y not finite)
__device__ __forceinline__ bool velocity_of(double x, double y, double yaw, double dt_scan, double &vx, double &vy, double &wz) {
  vx = vy = wz = 0.0;
  if (!(fabs(yaw) <= TH_MAX) || !(fabs(x) < INFINITY) || !(fabs(y) < INFINITY)) return false;
  const Poly f = poly(yaw);
  const double d = f.A * f.A + f.B * f.B;
  vx = ((f.A * x + f.B * y) / d) / dt_scan;
  vy = ((f.A * y - f.B * x) / d) / dt_scan;
  wz = yaw / dt_scan;
  return true;
}

}  // namespace mocomp
}  // namespace rsx
