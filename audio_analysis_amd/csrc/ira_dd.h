// Double-double arithmetic (~32 significant digits) on the device: a value is hi + lo with |lo| <= ulp(hi) / 2.
// Used by the double-double normal equations of ira_ar.hip (ar_lag_dd_kernel, ar_solve_dd_kernel).
#pragma once

#include <cmath>

#include "ira_common.h"

struct dd { double hi, lo; };
// `#pragma clang fp contract(off)` in every routine: ira_ar.hip is compiled with fused multiply-add contraction on, and a
// product that gets fused into the addition of an error-free transformation (s = a + b*c computed as ONE fma while the error
// term assumes s = fl(a + fl(b*c))) silently turns double-double into plain float64 -- seen as a 6e-8 instead of 1e-15
// agreement with an exact rational solve.
__device__ __forceinline__ dd dd_two_sum(double a, double b) {
#pragma clang fp contract(off)
  const double s = a + b, bb = s - a;
  return {s, (a - (s - bb)) + (b - bb)};
}
__device__ __forceinline__ dd dd_fast_two_sum(double a, double b) {      // |a| >= |b|
#pragma clang fp contract(off)
  const double s = a + b;
  return {s, b - (s - a)};
}
__device__ __forceinline__ dd dd_two_prod(double a, double b) {
#pragma clang fp contract(off)
  const double p = a * b;
  return {p, fma(a, b, -p)};
}
__device__ __forceinline__ dd dd_add(dd x, dd y) {
#pragma clang fp contract(off)
  const dd s = dd_two_sum(x.hi, y.hi);
  const dd t = dd_two_sum(x.lo, y.lo);
  const dd u = dd_fast_two_sum(s.hi, s.lo + t.hi);
  return dd_fast_two_sum(u.hi, u.lo + t.lo);
}
__device__ __forceinline__ dd dd_neg(dd x) { return {-x.hi, -x.lo}; }
__device__ __forceinline__ dd dd_mul(dd x, dd y) {
#pragma clang fp contract(off)
  dd p = dd_two_prod(x.hi, y.hi);
  p.lo += x.hi * y.lo + x.lo * y.hi;
  return dd_fast_two_sum(p.hi, p.lo);
}
__device__ __forceinline__ dd dd_div(dd x, dd y) {
#pragma clang fp contract(off)
  const double q1 = x.hi / y.hi;
  dd r = dd_add(x, dd_neg(dd_mul(y, dd{q1, 0.0})));
  const double q2 = r.hi / y.hi;
  r = dd_add(r, dd_neg(dd_mul(y, dd{q2, 0.0})));
  const double q3 = r.hi / y.hi;
  const dd q = dd_fast_two_sum(q1, q2);
  return dd_add(q, dd{q3, 0.0});
}
__device__ __forceinline__ dd dd_sqrt(dd x) {                            // x > 0
#pragma clang fp contract(off)
  const double s = sqrt(x.hi);
  const dd r = dd_add(x, dd_neg(dd_two_prod(s, s)));
  return dd_fast_two_sum(s, r.hi / (2.0 * s));
}
