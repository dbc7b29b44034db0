// In-register building blocks shared by the register-resident STFT (ira_stft2.hip) and the radix-16 passes of the
// in-LDS FFT (ira_fft_lds.h): constant twiddles, R-point decimation-in-frequency DFTs on register arrays, and a
// shallow power tree for per-butterfly twiddles; and the per-bin split of a complex transform that carried two real signals
// (ira_fftlong.hip, ira_fftsmooth.hip, ira_spectrum.hip).
#pragma once
#include "ira_common.h"

namespace ira {

template <typename T>
struct Wc {  // constants in the working precision
  static constexpr T c1 = (T)0.92387953251128675612818318939679;
  static constexpr T s1 = (T)0.38268343236508977172845998403040;
  static constexpr T h = (T)0.70710678118654752440084436210485;
};

// v * W16^j  (W16 = exp(-2 pi i / 16)), j compile-time after unrolling.
// NOT recursive on purpose: a self-recursive helper cannot be inlined and every twiddle became an s_swappc call.
template <typename T>
__device__ __forceinline__ cplx<T> mul_w16(cplx<T> v, int j) {
  const T c1 = Wc<T>::c1, s1 = Wc<T>::s1, h = Wc<T>::h;
  cplx<T> t;
  switch (j & 7) {
    case 0: t = v; break;
    case 1: t = {v.re * c1 + v.im * s1, v.im * c1 - v.re * s1}; break;
    case 2: t = {(v.re + v.im) * h, (v.im - v.re) * h}; break;
    case 3: t = {v.re * s1 + v.im * c1, v.im * s1 - v.re * c1}; break;
    case 4: t = {v.im, -v.re}; break;
    case 5: t = {v.im * c1 - v.re * s1, -v.re * c1 - v.im * s1}; break;
    case 6: t = {(v.im - v.re) * h, -(v.re + v.im) * h}; break;
    default: t = {v.im * s1 - v.re * c1, -v.re * s1 - v.im * c1}; break;
  }
  if (j & 8) t = {-t.re, -t.im};   // W16^(j+8) = -W16^j
  return t;
}

__host__ __device__ constexpr int brev_bits(int k, int bits) {
  int r = 0;
  for (int b = 0; b < bits; ++b) r |= ((k >> b) & 1) << (bits - 1 - b);
  return r;
}

// In-register R-point DFT, decimation in frequency; result X[k] is left at v[brev(k)].
template <typename T, int R>
__device__ __forceinline__ void dft_dif(cplx<T> (&v)[R]) {
  constexpr int LOG = (R == 16) ? 4 : 3;
#pragma unroll
  for (int s = 0; s < LOG; ++s) {
    const int span = R >> s, half = span >> 1;
#pragma unroll
    for (int b = 0; b < R; b += span) {
#pragma unroll
      for (int j = 0; j < half; ++j) {
        const cplx<T> a = v[b + j], c = v[b + j + half];
        v[b + j] = {a.re + c.re, a.im + c.im};
        const cplx<T> d = {a.re - c.re, a.im - c.im};
        v[b + j + half] = mul_w16<T>(d, j * (16 / span));   // W_span^j = W16^(j*16/span)
      }
    }
  }
}

// w^k for k = 0..15 from w (tree of depth <= 4 multiplications to limit rounding growth)
template <typename T>
__device__ __forceinline__ void powers16(cplx<T> w, cplx<T> (&p)[16]) {
  p[0] = {(T)1, (T)0};
  p[1] = w;
  p[2] = ira::cmul(w, w);
  p[3] = ira::cmul(p[2], w);
  p[4] = ira::cmul(p[2], p[2]);
  p[5] = ira::cmul(p[4], w);
  p[6] = ira::cmul(p[4], p[2]);
  p[7] = ira::cmul(p[4], p[3]);
  p[8] = ira::cmul(p[4], p[4]);
#pragma unroll
  for (int k = 9; k < 16; ++k) p[k] = ira::cmul(p[8], p[k - 8]);
}

// v[idx(k)] *= w^k for k = 1..15, idx = bit reversal (BREV: v[i] holds index brev4(i), the order dft_dif leaves) or
// identity.  Same products as powers16, but only w^1..w^7 and w^8 are ever live together: 36 registers of
// twiddles instead of 64 beside the 64 of v in float64, which is what keeps the radix-16 LDS passes at 4 waves/SIMD.
template <typename T, bool BREV>
__device__ __forceinline__ void twiddle16(cplx<T> (&v)[16], cplx<T> w) {
  cplx<T> p[8];
  p[1] = w;
  p[2] = ira::cmul(w, w);
  p[3] = ira::cmul(p[2], w);
  p[4] = ira::cmul(p[2], p[2]);
  p[5] = ira::cmul(p[4], w);
  p[6] = ira::cmul(p[4], p[2]);
  p[7] = ira::cmul(p[4], p[3]);
#pragma unroll
  for (int k = 1; k < 8; ++k) {
    const int i = BREV ? brev_bits(k, 4) : k;
    v[i] = ira::cmul(v[i], p[k]);
  }
  const cplx<T> w8 = ira::cmul(p[4], p[4]);
  {
    const int i = BREV ? brev_bits(8, 4) : 8;
    v[i] = ira::cmul(v[i], w8);
  }
#pragma unroll
  for (int k = 1; k < 8; ++k) {
    const int i = BREV ? brev_bits(8 + k, 4) : 8 + k;
    v[i] = ira::cmul(v[i], ira::cmul(w8, p[k]));
  }
}

// The same for 8-point butterflies: v[idx(k)] *= w^k, k = 1..7, idx = 3-bit reversal or identity.
template <typename T, bool BREV>
__device__ __forceinline__ void twiddle8(cplx<T> (&v)[8], cplx<T> w) {
  const cplx<T> w2 = ira::cmul(w, w);
  const cplx<T> w3 = ira::cmul(w2, w);
  const cplx<T> w4 = ira::cmul(w2, w2);
  const cplx<T> p[8] = {{(T)1, (T)0}, w, w2, w3, w4, ira::cmul(w4, w), ira::cmul(w4, w2), ira::cmul(w4, w3)};
#pragma unroll
  for (int k = 1; k < 8; ++k) {
    const int i = BREV ? brev_bits(k, 3) : k;
    v[i] = ira::cmul(v[i], p[k]);
  }
}

// radix selected by its log2 (3 or 4)
template <typename T, int LR, bool BREV>
__device__ __forceinline__ void twiddle_r(cplx<T> (&v)[1 << LR], cplx<T> w) {
  if constexpr (LR == 4) twiddle16<T, BREV>(v, w);
  else twiddle8<T, BREV>(v, w);
}

// ---- two real signals in one complex transform ----------------------------------------------------------------------------
// With Z = DFT_L(x1 + i x2) and zl = Z[(L - k) mod L]:
//   X1[k] = (Z[k] + conj zl) / 2,   X2[k] = (Z[k] - conj zl) / (2i).
template <typename T>
struct cplx2 {
  cplx<T> x1, x2;
};
template <typename T>
__device__ __forceinline__ cplx2<T> hermitian_parts(cplx<T> zk, cplx<T> zl) {
  const T h = (T)0.5;
  return {{h * (zk.re + zl.re), h * (zk.im - zl.im)}, {h * (zk.im + zl.im), h * (zl.re - zk.re)}};
}

// Bin k = 0 .. L/2 of the two half spectra.  k = 0 and k = L/2 pair a bin with itself, so their imaginary parts come out
// exactly zero like numpy's rfft.  The caller reads its job's offsets BEFORE this (the stores may alias the job tables).
__device__ __forceinline__ void pair_split_bin(const cplx<double>* z, long long L, long long k, cplx<double>* x1,
                                               cplx<double>* x2) {
  const cplx2<double> x = hermitian_parts(z[k], z[k == 0 ? 0 : L - k]);
  *x1 = x.x1;
  *x2 = x.x2;
}

// Interleaved signal: z[m] = x[2m] + i x[2m+1], Z = DFT_L(z); bin k = 0 .. L of the real signal's spectrum of length 2L is
//   X[k] = E[k] + W_2L^k O[k],  (E, O) = hermitian_parts(Z[k], Z[L-k])   (Z index mod L)
// Returned, not stored: of the two kernels that use it one reads its output offset before the arithmetic and one after it, and
// each keeps its order.
__device__ __forceinline__ cplx<double> half_split_bin(const cplx<double>* z, long long L, long long k) {
  const auto [ev, od] = hermitian_parts(z[k == L ? 0 : k], z[(k == 0 || k == L) ? 0 : L - k]);
  double sn, cs;
  sincospi(-(double)k / (double)L, &sn, &cs);                 // W_2L^k = exp(-i pi k / L)
  cplx<double> x = {ev.re + (cs * od.re - sn * od.im), ev.im + (cs * od.im + sn * od.re)};
  if (k == 0 || k == L) x.im = 0.0;                            // DC / Nyquist of a real signal
  return x;
}

}  // namespace ira
