// a19-a21: what follows the z-plane AR fit of ira_ar.hip (reference analyse/zplane.py:123-158).
//   poly_roots_kernel     all roots of the monic polynomial by Aberth-Ehrlich iteration in float64
//                         (numpy.roots uses companion-matrix eigenvalues; root ORDER is unspecified there, so
//                         parity is on the sorted set and on the radius statistics).
//   fir_numerator_kernel  b[n] = sum_k a[k] h[n-k], n <= Q   (zplane.py:123-142, --zeros option).
#include <cmath>

#include "ira_common.h"

namespace {

// ------------------------------------------------------------------------------------------------------------
// Aberth-Ehrlich: all roots of c[0] z^n + ... + c[n] (descending powers), float64 complex.
// One workgroup per polynomial, one thread per root (n <= 1024).  Jacobi-style sweeps (all corrections from
// the previous iterate) keep it deterministic.  Leading/trailing handling follows the reference: trailing
// |c| < trail_eps coefficients are dropped first (zplane.py:153-155), then numpy.roots semantics (leading
// zeros stripped; exact trailing zeros become roots at 0).
// ------------------------------------------------------------------------------------------------------------
constexpr int RT_MAX_DEG = 1024;
constexpr int RT_MAX_ITERS = 200;
constexpr double RT_ZERO_TOL = 2.0 * 1.1102230246251565e-16;   // 2 u, u = 2^-53

struct cdbl { double re, im; };
__device__ __forceinline__ cdbl c_mul(cdbl a, cdbl b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ cdbl c_div(cdbl a, cdbl b) {
  // Smith's algorithm
  if (fabs(b.re) >= fabs(b.im)) {
    const double r = b.im / b.re, d = b.re + b.im * r;
    return {(a.re + a.im * r) / d, (a.im - a.re * r) / d};
  }
  const double r = b.re / b.im, d = b.re * r + b.im;
  return {(a.re * r + a.im) / d, (a.im * r - a.re) / d};
}

// LPR lanes per root (round 4): the sum over the other roots, 1 / (z_k - z_j) -- a float64 reciprocal per pair, four fifths
// of an iteration -- is dealt to LPR neighbouring lanes and combined with two DPP shuffles; the Horner chain (serial by
// nature) is evaluated by every lane of the group.  One lane per root kept a 64-root polynomial on ONE wave for ~20
// iterations of ~14 k cycles each: 0.15-0.18 ms per 256 polynomials at a quarter of the SIMDs.
template <int LPR>
__global__ void poly_roots_kernel(const double* __restrict__ coeffs, int stride, int ncoef, double trail_eps,
                                  double* __restrict__ roots, int32_t* __restrict__ nroots_out) {
  __shared__ double c[RT_MAX_DEG + 1];
  __shared__ cdbl z[2][RT_MAX_DEG];
  __shared__ int sh_lo, sh_hi, sh_changed;
  const int e = blockIdx.x, nt = blockDim.x / LPR;
  const int tid = threadIdx.x / LPR, part = threadIdx.x % LPR;     // root slot and the lane's share of the pair sum
  const double* ce = coeffs + (long long)e * stride;
  double* re = roots + (long long)e * 2 * (ncoef - 1);
  if (threadIdx.x == 0) {
    int hi = ncoef;   // exclusive end after trimming tiny trailing coefficients
    while (hi > 1 && fabs(ce[hi - 1]) < trail_eps) --hi;
    int lo = 0;       // strip leading exact zeros (numpy.roots)
    while (lo < hi && ce[lo] == 0.0) ++lo;
    sh_lo = lo; sh_hi = hi;
  }
  __syncthreads();
  int lo = sh_lo, hi = sh_hi;
  if (hi - lo <= 1 || hi <= 1) {
    if (threadIdx.x == 0) nroots_out[e] = 0;
    return;
  }
  // exact trailing zeros -> roots at the origin
  int tz = 0;
  while (hi - 1 - tz > lo && ce[hi - 1 - tz] == 0.0) ++tz;
  const int n = hi - lo - 1 - tz;   // degree of the deflated polynomial
  const double lead = ce[lo];
  for (int k = threadIdx.x; k <= n; k += blockDim.x) c[k] = ce[lo + k] / lead;   // monic
  __syncthreads();
  if (n >= 1) {
    // initial radius: geometric mean of the root moduli, |c_n|^(1/n), kept in a sane range
    double r0 = pow(fabs(c[n]), 1.0 / (double)n);
    if (!(r0 > 1e-3)) r0 = 1e-3;
    if (r0 > 1e3) r0 = 1e3;
    for (int k = threadIdx.x; k < n; k += blockDim.x) {
      double s, co;
      sincos(2.0 * 3.14159265358979323846 * (double)k / (double)n + 0.4, &s, &co);
      z[0][k] = {r0 * co, r0 * s};
    }
    __syncthreads();
    int cur = 0;
    for (int it = 0; it < RT_MAX_ITERS; ++it) {
      if (threadIdx.x == 0) sh_changed = 0;
      __syncthreads();
      int changed = 0;
      // (every lane of a group runs the same trip count: the shuffles below need the whole group)
      for (int k0 = tid; k0 < ((n + nt - 1) / nt) * nt; k0 += nt) {
        const bool live = k0 < n;
        const int k = live ? k0 : n - 1;
        const cdbl zk = z[cur][k];
        // Newton ratio p / p' and "p(zk) != 0".  The lanes of a group share zk: every branch here is uniform across them.
        // p counts as zero, and the iterate stays where it is, once |p| is within RT_ZERO_TOL (two units roundoff) of
        // sv = sum_k |c_k| |zk|^(n-k): Horner's own rounding error is of that size, a correction computed from such a p is noise.
        // At an m-fold root every sweep is noise once the iterates are within u^(1/m) of it; this test is what ends them there.
        // Outside the unit circle |zk|^n overflows long before the iterate is unreasonable (|zk| > 2 at n = 1024), and one NaN
        // iterate enters every other root's pair sum.  There, with y = 1 / zk and q(y) = 1 + c_1 y + ... + c_n y^n,
        // p(z) = z^n q(y) and p / p' = 1 / (y (n - y q'(y) / q(y))), every power at most 1 in modulus: the same Horner
        // recurrence on the coefficients in reverse order at y (one loop for both, so that a wave with iterates on both
        // sides of the circle does not run two).
        const bool outside = zk.re * zk.re + zk.im * zk.im > 1.0;
        const cdbl x = outside ? c_div(cdbl{1.0, 0.0}, zk) : zk;
        const double ax = sqrt(x.re * x.re + x.im * x.im);
        const int step = outside ? -1 : 1;
        int idx = outside ? n : 0;
        cdbl pv = {c[idx], 0.0}, dv = {0.0, 0.0};           // p and p' at zk, or q and q' at y
        double sv = fabs(c[idx]);
        for (int m = 1; m <= n; ++m) {
          idx += step;
          const double cm = c[idx];
          dv = c_mul(dv, x); dv.re += pv.re; dv.im += pv.im;
          pv = c_mul(pv, x); pv.re += cm;
          sv = sv * ax + fabs(cm);
        }
        const bool nonzero = fabs(pv.re) + fabs(pv.im) > RT_ZERO_TOL * sv;
        cdbl ratio;
        if (outside) {
          const cdbl t = c_mul(x, c_div(dv, pv));
          ratio = c_div(cdbl{1.0, 0.0}, c_mul(x, cdbl{(double)n - t.re, -t.im}));
        } else {
          ratio = c_div(pv, dv);
        }
        cdbl w = {0.0, 0.0};
        if (nonzero) {
          cdbl sum = {0.0, 0.0};
          for (int j = part; j < n; j += LPR) {
            if (j == k) continue;
            const cdbl zj = z[cur][j];
            const double dr = zk.re - zj.re, di = zk.im - zj.im;
            const double d2 = dr * dr + di * di;
            // 1/(zk - zj) = conj(d)/|d|^2; coincident iterates (a multiple root) add nothing instead of 0 * inf
            const double inv = d2 != 0.0 ? 1.0 / d2 : 0.0;
            sum.re += dr * inv; sum.im -= di * inv;
          }
          if (LPR > 1) {
#pragma unroll
            for (int o = 1; o < LPR; o <<= 1) {                // the group's lanes are neighbours: xor 1, xor 2
              sum.re += __shfl_xor(sum.re, o, 64);
              sum.im += __shfl_xor(sum.im, o, 64);
            }
          }
          const cdbl rs = c_mul(ratio, sum);
          w = c_div(ratio, cdbl{1.0 - rs.re, -rs.im});
        }
        if (live && part == 0) z[cur ^ 1][k] = {zk.re - w.re, zk.im - w.im};
        const double wm = fabs(w.re) + fabs(w.im), zm = fabs(zk.re) + fabs(zk.im);
        if (live && wm > 2e-13 * zm) changed = 1;
      }
      if (changed) sh_changed = 1;   // benign race: every writer stores 1
      __syncthreads();
      cur ^= 1;
      const int any = sh_changed;
      __syncthreads();
      if (!any) break;
    }
    for (int k = threadIdx.x; k < n; k += blockDim.x) { re[2 * k] = z[cur][k].re; re[2 * k + 1] = z[cur][k].im; }
  }
  for (int k = n + threadIdx.x; k < n + tz; k += blockDim.x) { re[2 * k] = 0.0; re[2 * k + 1] = 0.0; }
  if (threadIdx.x == 0) nroots_out[e] = n + tz;
}

// b[n] = sum_{k=0..p} a[k] h[n-k], 0 <= n-k < N; h = x / divisor (float64)
__global__ void fir_numerator_kernel(const double* __restrict__ coeffs, int p, const float* __restrict__ x,
                                     const int64_t* __restrict__ xoff, const int32_t* __restrict__ nlen,
                                     const double* __restrict__ divisor, int q, double* __restrict__ b) {
  const int e = blockIdx.x;
  const double* a = coeffs + (long long)e * (p + 1);
  const float* xs = x + xoff[e];
  const double div = divisor ? divisor[e] : 1.0;
  const long long N = nlen[e];
  for (int n = threadIdx.x; n <= q; n += blockDim.x) {
    double acc = 0.0;
    for (int k = 0; k <= p; ++k) {
      const long long m = (long long)n - k;
      if (m < 0 || m >= N) continue;
      acc += a[k] * ((double)xs[m] / div);
    }
    b[(long long)e * (q + 1) + n] = acc;
  }
}

}  // namespace

extern "C" int32_t ira_poly_roots(const double* coeffs_dev, int32_t npoly, int32_t ncoef, double trail_eps,
                                  double* roots_dev, int32_t* nroots_dev, void* stream) {
  IRA_CHECK_PTR(coeffs_dev); IRA_CHECK_PTR(roots_dev); IRA_CHECK_PTR(nroots_dev);
  if (npoly <= 0) return npoly == 0 ? IRA_OK : IRA_E_SIZE;
  if (ncoef < 2 || ncoef - 1 > RT_MAX_DEG) return IRA_E_SIZE;
  int threads = 64;
  while (threads < ncoef - 1 && threads < 1024) threads <<= 1;
  if (threads <= 256) {                                      // four lanes per root while a workgroup can hold them
    poly_roots_kernel<4><<<npoly, 4 * threads, 0, (hipStream_t)stream>>>(coeffs_dev, ncoef, ncoef, trail_eps, roots_dev,
                                                                        nroots_dev);
    IRA_RETURN_LAUNCH();
  }
  poly_roots_kernel<1><<<npoly, threads, 0, (hipStream_t)stream>>>(coeffs_dev, ncoef, ncoef, trail_eps, roots_dev,
                                                               nroots_dev);
  IRA_RETURN_LAUNCH();
}

extern "C" int32_t ira_fir_numerator(const double* coeffs_dev, int32_t order, const float* x_dev,
                                     const int64_t* xoff_dev, const int32_t* len_dev, const double* divisor_dev,
                                     int32_t nb, int32_t zero_order, double* b_dev, void* stream) {
  IRA_CHECK_PTR(coeffs_dev); IRA_CHECK_PTR(x_dev); IRA_CHECK_PTR(xoff_dev); IRA_CHECK_PTR(len_dev);
  IRA_CHECK_PTR(b_dev);
  if (nb <= 0) return nb == 0 ? IRA_OK : IRA_E_SIZE;
  if (order < 0 || zero_order < 0) return IRA_E_SIZE;
  fir_numerator_kernel<<<nb, 128, 0, (hipStream_t)stream>>>(coeffs_dev, order, x_dev, xoff_dev, len_dev,
                                                            divisor_dev, zero_order, b_dev);
  IRA_RETURN_LAUNCH();
}
