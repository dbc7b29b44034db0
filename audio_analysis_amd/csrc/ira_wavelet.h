// The wavelet term g(k) = w(k) e^{-2 pi i k rho}, k = -H .. H, of a point (H, rho, window) and the checks of a grid of such
// points, once: ira_fdw.hip sums the terms where it forms them, ira_burstdecay.hip stores them as a table, and include/ira.h
// promises the same bits of both.  For files compiled with -ffp-contract=off: the reduction of the turn count needs the
// PRODUCT k rho rounded (t_hi) and its error (t_lo) apart -- a contraction of `k * rho - rint(t_hi)` into one fma would
// count t_lo twice.
#pragma once
#include "ira_common.h"

namespace ira {

// Term k: sincospi of the turn count k rho, reduced exactly, into *sn and *cs; returns the weight, for hann (window 0)
// sinpi((H + 1 - |k|) / (2 H + 2))^2, else 1.  recip() gives 1.0 / (double)(2 * h + 2), always that quotient; the CALLER
// says where it is formed (once per point in front of ira_fdw.hip's rounds, at the term in the table kernel), which is
// all that told the two kernels' code apart and keeps each what it was.
template <typename Recip>
__device__ __forceinline__ double wavelet_term(int k, int h, double rho, int window, Recip recip, double* sn, double* cs) {
  const double kd = (double)k;
  const double t_hi = kd * rho;
  const double t_lo = fma(kd, rho, -t_hi);
  const double turn = (t_hi - rint(t_hi)) + t_lo;
  sincospi(2.0 * turn, sn, cs);
  double w = 1.0;
  if (window == 0) {
    const double sp = sinpi((double)(h + 1 - (k < 0 ? -k : k)) * recip());
    w = sp * sp;
  }
  return w;
}

// half_dev[j] clamped to its range: no access depends on the device table holding the host's values
__device__ __forceinline__ int wavelet_half(const int32_t* half_dev, int j) {
  const int h = half_dev[j];
  return h < 1 ? 1 : (h > IRA_FDW_MAX_HALF ? IRA_FDW_MAX_HALF : h);
}

// a centre sample clamped to +-2^62: |p| beyond this is as far outside every channel as this, and p +- H cannot overflow
__device__ __forceinline__ int64_t wavelet_centre(int64_t p) {
  constexpr int64_t limit = (int64_t)1 << 62;
  return p > limit ? limit : (p < -limit ? -limit : p);
}

// The host's check of a point grid: IRA_E_SIZE for npts outside 0 .. IRA_FDW_MAX_POINTS, a window other than hann (0) or
// rect (1), a rho[j] not finite or outside (0, 0.5] (rho == nullptr: a call that takes none) or a half[j] outside
// 1 .. IRA_FDW_MAX_HALF; IRA_E_NULL for points without a half table.
inline int32_t wavelet_points_check(const double* rho, const int32_t* half, int32_t npts, int32_t window) {
  if (npts < 0 || npts > IRA_FDW_MAX_POINTS) return IRA_E_SIZE;
  if (npts > 0) IRA_CHECK_PTR(half);
  if (window != 0 && window != 1) return IRA_E_SIZE;
  for (int32_t j = 0; rho != nullptr && j < npts; ++j)
    if (!(isfinite(rho[j]) && rho[j] > 0.0 && rho[j] <= 0.5)) return IRA_E_SIZE;
  for (int32_t j = 0; j < npts; ++j)
    if (half[j] < 1 || half[j] > IRA_FDW_MAX_HALF) return IRA_E_SIZE;
  return IRA_OK;
}

}  // namespace ira
