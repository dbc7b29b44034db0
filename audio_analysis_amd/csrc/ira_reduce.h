// The loads, wave reductions, wave scans and chunk-record fold that the measure kernels share (gfx950; wave = 64 lanes).
// Everything is inline, so a function rounds the way its includer's -ffp-contract setting says.
#pragma once

#include "ira_common.h"

namespace ira {

// ---- 16-byte accesses at the alignment of their element ---------------------------------------------------------------------
// A sample row starts anywhere (peak-trimmed offsets, onsets).  With the alignment declared as 4 (8) bytes the compiler still
// issues one 16-byte access, at any address: which thread holds which sample never depends on the address, so neither does
// the order of the sums.  That is what makes a row's result bit-identical whatever the batch and its place in it.
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
typedef double d2u __attribute__((ext_vector_type(2), aligned(8)));

// ---- tile loads --------------------------------------------------------------------------------------------------------------
// A contiguous run per thread: x = src[PER tid .. PER tid + PER), zeros where first + PER tid + r >= end (first = the index
// of src[0] on the axis `end` is counted on).
template <int PER, typename N>
__device__ __forceinline__ void load_run(const float* __restrict__ src, N first, N end, float x[PER]) {
  const int i0 = PER * threadIdx.x;
  const N m0 = first + i0;
  if (m0 + PER <= end) {
#pragma unroll
    for (int j = 0; j < PER / 4; ++j) {
      const f4u v = *reinterpret_cast<const f4u*>(src + i0 + 4 * j);
      x[4 * j] = v.x; x[4 * j + 1] = v.y; x[4 * j + 2] = v.z; x[4 * j + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int r = 0; r < PER; ++r) x[r] = (m0 + r < end) ? src[i0 + r] : 0.0f;
  }
}

// Strided quads of a chunk of cnt valid samples: a[u] = q[4 (tid + THREADS u) .. + 3], zeros past cnt; all loads in flight
// together.  FULL: cnt is the whole chunk, no test.
template <int THREADS, int QUADS, bool FULL>
__device__ __forceinline__ void load_quads(const float* __restrict__ q, int cnt, f4u a[QUADS]) {
#pragma unroll
  for (int u = 0; u < QUADS; ++u) {
    const int b = 4 * (threadIdx.x + THREADS * u);
    if (FULL || b + 4 <= cnt) {
      a[u] = *reinterpret_cast<const f4u*>(q + b);
    } else {
      a[u] = f4u{0.0f, 0.0f, 0.0f, 0.0f};
      if (b < cnt) a[u].x = q[b];
      if (b + 1 < cnt) a[u].y = q[b + 1];
      if (b + 2 < cnt) a[u].z = q[b + 2];
    }
  }
}

// ---- wave reductions: total orders, so the shape of the tree does not matter ------------------------------------------------
template <typename T>
__device__ __forceinline__ T wave_min(T v) {                  // integers
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const T other = __shfl_xor(v, o, 64);
    v = other < v ? other : v;
  }
  return v;
}
template <typename T>
__device__ __forceinline__ T wave_max_int(T v) {              // integers (and bit patterns ordered as such)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const T other = __shfl_xor(v, o, 64);
    v = other > v ? other : v;
  }
  return v;
}
__device__ __forceinline__ double wave_max(double v) {        // fmax: a NaN is dropped
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}
// (greatest value, then smallest index); no NaN among the values
template <typename V, typename I>
__device__ __forceinline__ void wave_argmax(V& v, I& idx) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const V ov = __shfl_xor(v, o, 64);
    const I oi = __shfl_xor(idx, o, 64);
    if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
  }
}

// ---- wave scans (Hillis-Steele, distances 1, 2, .. 32: the association the callers' sums are compared bit for bit in) ----------
// Inclusive sum over the lanes up to and including this one; excl = the sum over the lanes in front of it.
template <typename T>
__device__ __forceinline__ T wave_prefix(T v, int lane, T& excl) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T dn = __shfl_up(v, o, 64);
    if (lane >= o) v += dn;
  }
  excl = __shfl_up(v, 1, 64);
  if (lane == 0) excl = 0;
  return v;
}
// The mirror image: this lane and the lanes after it; excl = the lanes after it.
template <typename T>
__device__ __forceinline__ T wave_suffix(T v, int lane, T& excl) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T up = __shfl_down(v, o, 64);
    if (lane + o < 64) v += up;
  }
  excl = __shfl_down(v, 1, 64);
  if (lane == 63) excl = 0;
  return v;
}

// numpy.maximum: a NaN operand gives NaN (fmax would drop it)
__device__ __forceinline__ double np_max(double a, double b) { return (a != a) ? a : fmax(a, b); }
// the quiet NaN numpy.nan is
__device__ __forceinline__ double qnan() { return __longlong_as_double(0x7ff8000000000000ll); }

// float32 <-> a key whose unsigned order is the float order (no value maps to key 0)
__device__ __forceinline__ uint32_t float_key(float f) {
  const uint32_t b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float float_unkey(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// ---- the fold of a row's chunk records, for a one-wave workgroup ------------------------------------------------------------
// Row `row` of n samples owns chunk_stride records of nrec doubles in scratch, one per `chunk` samples.  Lane l adds records
// l, l + 64, ... in ascending order, then wave_sum -> out[row * nrec ..].  A row longer than the max_len the stride was sized
// for: never read past its records.
__device__ __forceinline__ void fold_records(const double* scratch, int row, int64_t n, int chunk, int64_t chunk_stride,
                                             int nrec, double* out) {
  int64_t nch = n > 0 ? (n + chunk - 1) / chunk : 0;
  if (nch > chunk_stride) nch = chunk_stride;
  const double* rec = scratch + (int64_t)row * chunk_stride * nrec;
  const int lane = threadIdx.x;
  for (int r = 0; r < nrec; ++r) {
    double v = 0.0;
    for (int64_t c = lane; c < nch; c += IRA_WAVE) v += rec[c * nrec + r];
    v = wave_sum(v);
    if (lane == 0) out[(int64_t)row * nrec + r] = v;
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

}  // namespace ira
