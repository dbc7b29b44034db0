// Equalisation filter design: fractional-octave smoothing of the power spectrum on every bin, the regularised inversion,
// the gather of the grid points and the taper (include/ira_equalise.h and audio_analysis_amd/analyse/equalise.py state the
// definition).  Nothing in the reference computes it.
//
// The transforms of the chain are the library's long FFTs and the cepstral steps ira_minphase.hip's; this file holds what
// sits between them, for rows of one transform size N (n0 = N/2 + 1 bins):
//   ira_eq_power    level 0 of every row's pyramid: the members' |X|^2 summed in ascending order and divided by their
//                   count, optionally times |F|^2 of the row's second spectrum
//   ira_eq_pyramid  the upper levels, pairwise sums; EQ_TILE_LOG2 levels a pass out of one LDS tile
//   ira_eq_smooth   the window sum W(lo, hi) over the pyramid and S = W / (hi - lo + 1), one bin a lane
//   ira_eq_invert   c = (a t + beta) / (s + beta), clamped, as the complex (c, 0), and the clamped count per row
//   ira_eq_gather   doubles at the grid bins with a stride
//   ira_eq_taper    f = float32((double)g v)
// The window sum is the sum of at most 2 log2(N) pyramid entries, every one non-negative (no cancellation, unlike a
// difference of prefix sums), added in an order that (lo, hi) alone fixes: the NumPy restatement gives the same bits.
// Neighbouring lanes read neighbouring entries of every level, so the walk is served from the caches.  The only reduction
// is the clamped count, an integer sum combined by integer atomics.  No atomic touches a double and nothing depends on the
// launch shape.
//
// Compiled with -ffp-contract=off: re * re + im * im, the pairwise sums and the quotients round one operation at a time,
// like NumPy's.
//
// Every index is formed from the call's own N (checked: a power of two 32 .. 2^21), and every table value (members, row
// starts, window edges, grid bins) is masked into range before it indexes anything.
#include <math.h>

#include "ira_common.h"
#include "../../include/ira_equalise.h"

namespace {

constexpr int EQ_THREADS = 256;
constexpr int EQ_MIN_N = 32, EQ_MAX_N = 1 << IRA_MINPHASE_MAX_LOG2;
typedef unsigned long long u64;

// THE geometry of a row's pyramid, host and device: level j of a row of n0 = N/2 + 1 bins has len entries at off doubles
// from the row's start.  eq_levels: the count of levels (the last one has one entry); eq_row_doubles: a row's doubles.
struct EqLevel { int off, len; };

__host__ __device__ __forceinline__ EqLevel eq_level(int n0, int j) {
  EqLevel v;
  v.off = 0;
  v.len = n0;
  for (int i = 0; i < j; ++i) {
    v.off += v.len;
    v.len = (v.len + 1) >> 1;
  }
  return v;
}

__host__ __device__ __forceinline__ int eq_levels(int n0) {
  int levels = 1;
  for (int n = n0; n > 1; n = (n + 1) >> 1) ++levels;
  return levels;
}

__host__ __device__ __forceinline__ long long eq_row_doubles(int n0) {
  const EqLevel top = eq_level(n0, eq_levels(n0) - 1);
  return (long long)top.off + top.len;
}

__device__ __forceinline__ int eq_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(EQ_THREADS) void eq_power_kernel(const double2* __restrict__ spec, const int64_t* __restrict__ spec_off,
                                                              int nspec, const int32_t* __restrict__ member, int nmember,
                                                              const int32_t* __restrict__ row_first,
                                                              const double2* __restrict__ spec2,
                                                              const int64_t* __restrict__ spec2_off, int n0, long long row_doubles,
                                                              double* __restrict__ pyr) {
  const int row = blockIdx.y;
  const int k = blockIdx.x * EQ_THREADS + threadIdx.x;
  if (k >= n0) return;
  const int first = eq_clamp(ira::uniform(row_first[row]), 0, nmember);
  int count = eq_clamp(ira::uniform(row_first[row + 1]) - first, 0, IRA_EQ_MAX_MEMBERS);
  count = count > nmember - first ? nmember - first : count;
  double p = 0.0;
  for (int m = 0; m < count; ++m) {
    const int s = eq_clamp(ira::uniform(member[first + m]), 0, nspec - 1);
    const double2 v = spec[ira::uniform(spec_off[s]) + k];
    p = p + (v.x * v.x + v.y * v.y);
  }
  if (count > 0) p = p / (double)count;
  if (spec2 != nullptr) {
    const double2 f = spec2[ira::uniform(spec2_off[row]) + k];
    p = p * (f.x * f.x + f.y * f.y);
  }
  pyr[(long long)row * row_doubles + k] = p;
}

// One pass: the workgroup (tile, row) stages the up to EQ_TILE entries of level `base` from tile * EQ_TILE on and writes
// its share of the `up` levels above (up <= EQ_TILE_LOG2): a tile starts at a multiple of 2^up, so its pairs are the
// level's pairs, and only the last tile of a level is short -- its odd entry out is the level's.
__global__ __launch_bounds__(EQ_THREADS) void eq_pyramid_kernel(double* __restrict__ pyr, int n0, long long row_doubles, int base,
                                                                int up) {
  __shared__ double buf[2][IRA_EQ_TILE];
  const EqLevel lv = eq_level(n0, base);
  double* row = pyr + (long long)blockIdx.y * row_doubles;
  int start = blockIdx.x * IRA_EQ_TILE;
  int cnt = lv.len - start;
  cnt = cnt > IRA_EQ_TILE ? IRA_EQ_TILE : cnt;
  if (cnt <= 0) return;                                                   // (uniform: the whole workgroup leaves)
  for (int i = threadIdx.x; i < cnt; i += EQ_THREADS) buf[0][i] = row[lv.off + start + i];
  __syncthreads();
  int off = lv.off, len = lv.len, cur = 0;
  for (int m = 0; m < up; ++m) {
    off += len;
    len = (len + 1) >> 1;
    start >>= 1;
    const int half = (cnt + 1) >> 1;
    for (int i = threadIdx.x; i < half; i += EQ_THREADS) {
      double v = buf[cur][2 * i];
      if (2 * i + 1 < cnt) v = v + buf[cur][2 * i + 1];
      buf[cur ^ 1][i] = v;
      if (start + i < len) row[off + start + i] = v;                       // (always true; the level's own length bounds the store)
    }
    __syncthreads();
    cur ^= 1;
    cnt = half;
  }
}

// W(lo, hi) over the pyramid at `row`: 0 <= lo <= hi < n0.  l < r <= n_j holds at every level, so every read lies in its level.
__device__ __forceinline__ double eq_window(const double* __restrict__ row, int n0, int lo, int hi) {
  int l = lo, r = hi + 1, n = n0;
  double left = 0.0, right = 0.0;
  const double* lev = row;
  while (l < r) {
    if (l & 1) left = left + lev[l++];
    if (r & 1) right = right + lev[--r];
    l >>= 1;
    r >>= 1;
    lev += n;
    n = (n + 1) >> 1;
  }
  return left + right;
}

__global__ __launch_bounds__(EQ_THREADS) void eq_smooth_kernel(const double* __restrict__ pyr, const int32_t* __restrict__ lo_tab,
                                                               const int32_t* __restrict__ hi_tab, int n0, long long row_doubles,
                                                               double* __restrict__ s_out) {
  const int k = blockIdx.x * EQ_THREADS + threadIdx.x;
  if (k >= n0) return;
  const int lo = eq_clamp(lo_tab[k], 0, n0 - 1);
  const int hi = eq_clamp(hi_tab[k], lo, n0 - 1);
  const double w = eq_window(pyr + (long long)blockIdx.y * row_doubles, n0, lo, hi);
  s_out[(long long)blockIdx.y * n0 + k] = w / (double)(hi - lo + 1);
}

__global__ __launch_bounds__(EQ_THREADS) void eq_invert_kernel(const double* __restrict__ s_in, const double* __restrict__ ref,
                                                               const double* __restrict__ target, const double* __restrict__ beta,
                                                               double max_gain, const int64_t* __restrict__ c_off, int n0,
                                                               double2* __restrict__ c_out, u64* __restrict__ clamped) {
  __shared__ unsigned part[EQ_THREADS / IRA_WAVE];
  const int row = blockIdx.y;
  const double rf = ira::uniform(ref[row]);
  const bool valid = rf > 0.0 && rf < __builtin_inf();
  const double* s_row = s_in + (long long)row * n0;
  double2* out = c_out + ira::uniform(c_off[row]);
  unsigned over = 0;
  for (int k = blockIdx.x * EQ_THREADS + threadIdx.x; k < n0; k += gridDim.x * EQ_THREADS) {
    double2 v;
    v.x = 1.0;                                                            // a row without values: the unit filter
    v.y = 0.0;
    if (valid) {
      const double s = s_row[k] / rf;
      const double a = sqrt(s);
      const double b = beta[k];
      double c = (a * target[k] + b) / (s + b);
      if (c > max_gain) {
        c = max_gain;
        ++over;
      }
      v.x = c;
    }
    out[k] = v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) over += __shfl_xor(over, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = over;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < EQ_THREADS / IRA_WAVE; ++w) over += part[w];
    if (over) atomicAdd(clamped + row, (u64)over);
  }
}

__global__ __launch_bounds__(EQ_THREADS) void eq_gather_kernel(const double* __restrict__ src, const int64_t* __restrict__ src_off,
                                                               int stride, const int32_t* __restrict__ bins, int npts, int n0,
                                                               double* __restrict__ out) {
  const int j = blockIdx.x * EQ_THREADS + threadIdx.x;
  if (j >= npts) return;
  const int k = eq_clamp(bins[j], 0, n0 - 1);
  out[(long long)blockIdx.y * npts + j] = src[ira::uniform(src_off[blockIdx.y]) + (long long)stride * k];
}

__global__ __launch_bounds__(EQ_THREADS) void eq_taper_kernel(const float* __restrict__ g, const int64_t* __restrict__ g_off,
                                                              const double* __restrict__ taper, int taps, float* __restrict__ f) {
  const int n = blockIdx.x * EQ_THREADS + threadIdx.x;
  if (n >= taps) return;
  f[(long long)blockIdx.y * taps + n] = (float)((double)g[ira::uniform(g_off[blockIdx.y]) + n] * taper[n]);
}

bool eq_sizes_ok(int32_t nrows, int32_t nfft) {
  return nrows >= 0 && nrows <= 65535 && nfft >= EQ_MIN_N && nfft <= EQ_MAX_N && (nfft & (nfft - 1)) == 0;
}

unsigned eq_blocks(int count) { return (unsigned)((count + EQ_THREADS - 1) / EQ_THREADS); }

}  // namespace

extern "C" int32_t ira_eq_power(const double* spec_dev, const int64_t* spec_off_dev, int32_t nspec, const int32_t* member_dev,
                                int32_t nmember, const int32_t* row_first_dev, int32_t nrows, const double* spec2_dev,
                                const int64_t* spec2_off_dev, int32_t nfft, double* pyr_dev, void* stream) {
  IRA_CHECK_PTR(spec_dev); IRA_CHECK_PTR(spec_off_dev); IRA_CHECK_PTR(member_dev); IRA_CHECK_PTR(row_first_dev);
  IRA_CHECK_PTR(pyr_dev);
  if (spec2_dev != nullptr) IRA_CHECK_PTR(spec2_off_dev);
  if (!eq_sizes_ok(nrows, nfft)) return IRA_E_SIZE;
  if (nspec < 1 || nspec > IRA_EQ_MAX_TABLE || nmember < 1 || nmember > IRA_EQ_MAX_TABLE) return IRA_E_SIZE;
  if (nrows == 0) return IRA_OK;
  const int n0 = nfft / 2 + 1;
  const dim3 grid(eq_blocks(n0), (unsigned)nrows);
  eq_power_kernel<<<grid, EQ_THREADS, 0, (hipStream_t)stream>>>(
      reinterpret_cast<const double2*>(spec_dev), spec_off_dev, nspec, member_dev, nmember, row_first_dev,
      reinterpret_cast<const double2*>(spec2_dev), spec2_off_dev, n0, eq_row_doubles(n0), pyr_dev);
  IRA_RETURN_LAUNCH();
}

extern "C" int32_t ira_eq_pyramid(double* pyr_dev, int32_t nrows, int32_t nfft, void* stream) {
  IRA_CHECK_PTR(pyr_dev);
  if (!eq_sizes_ok(nrows, nfft)) return IRA_E_SIZE;
  if (nrows == 0) return IRA_OK;
  const int n0 = nfft / 2 + 1;
  const int levels = eq_levels(n0);
  const long long row_doubles = eq_row_doubles(n0);
  for (int base = 0; base < levels - 1; base += IRA_EQ_TILE_LOG2) {
    const int up = levels - 1 - base < IRA_EQ_TILE_LOG2 ? levels - 1 - base : IRA_EQ_TILE_LOG2;
    const int len = eq_level(n0, base).len;
    const dim3 grid((unsigned)((len + IRA_EQ_TILE - 1) / IRA_EQ_TILE), (unsigned)nrows);
    eq_pyramid_kernel<<<grid, EQ_THREADS, 0, (hipStream_t)stream>>>(pyr_dev, n0, row_doubles, base, up);
  }
  IRA_RETURN_LAUNCH();
}

extern "C" int32_t ira_eq_smooth(const double* pyr_dev, const int32_t* lo_dev, const int32_t* hi_dev, int32_t nrows,
                                 int32_t nfft, double* s_dev, void* stream) {
  IRA_CHECK_PTR(pyr_dev); IRA_CHECK_PTR(lo_dev); IRA_CHECK_PTR(hi_dev); IRA_CHECK_PTR(s_dev);
  if (!eq_sizes_ok(nrows, nfft)) return IRA_E_SIZE;
  if (nrows == 0) return IRA_OK;
  const int n0 = nfft / 2 + 1;
  const dim3 grid(eq_blocks(n0), (unsigned)nrows);
  eq_smooth_kernel<<<grid, EQ_THREADS, 0, (hipStream_t)stream>>>(pyr_dev, lo_dev, hi_dev, n0, eq_row_doubles(n0), s_dev);
  IRA_RETURN_LAUNCH();
}

extern "C" int32_t ira_eq_invert(const double* s_dev, const double* ref_dev, const double* target_dev, const double* beta_dev,
                                 double max_gain, const int64_t* c_off_dev, int32_t nrows, int32_t nfft, double* c_dev,
                                 int64_t* clamped_dev, void* stream) {
  IRA_CHECK_PTR(s_dev); IRA_CHECK_PTR(ref_dev); IRA_CHECK_PTR(target_dev); IRA_CHECK_PTR(beta_dev); IRA_CHECK_PTR(c_off_dev);
  IRA_CHECK_PTR(c_dev); IRA_CHECK_PTR(clamped_dev);
  if (!eq_sizes_ok(nrows, nfft)) return IRA_E_SIZE;
  if (!(max_gain > 0.0 && max_gain < (double)INFINITY)) return IRA_E_SIZE;                  // (a NaN fails both)
  if (nrows == 0) return IRA_OK;
  hipStream_t st = (hipStream_t)stream;
  IRA_TRY_HIP(hipMemsetAsync(clamped_dev, 0, sizeof(int64_t) * (size_t)nrows, st));
  const int n0 = nfft / 2 + 1;
  // 8 bins a thread, at most 1024 workgroups along a row (the rest by the grid stride)
  unsigned blocks = (unsigned)((n0 + EQ_THREADS * 8 - 1) / (EQ_THREADS * 8));
  blocks = blocks > 1024u ? 1024u : blocks;
  const dim3 grid(blocks, (unsigned)nrows);
  eq_invert_kernel<<<grid, EQ_THREADS, 0, st>>>(s_dev, ref_dev, target_dev, beta_dev, max_gain, c_off_dev, n0,
                                                reinterpret_cast<double2*>(c_dev), reinterpret_cast<u64*>(clamped_dev));
  IRA_RETURN_LAUNCH();
}

extern "C" int32_t ira_eq_gather(const double* src_dev, const int64_t* src_off_dev, int32_t stride, const int32_t* bins_dev,
                                 int32_t nrows, int32_t npts, int32_t nfft, double* out_dev, void* stream) {
  IRA_CHECK_PTR(src_dev); IRA_CHECK_PTR(src_off_dev); IRA_CHECK_PTR(bins_dev); IRA_CHECK_PTR(out_dev);
  if (!eq_sizes_ok(nrows, nfft)) return IRA_E_SIZE;
  if (stride < 1 || stride > 2 || npts < 0 || npts > IRA_FDW_MAX_POINTS) return IRA_E_SIZE;
  if (nrows == 0 || npts == 0) return IRA_OK;
  const dim3 grid(eq_blocks(npts), (unsigned)nrows);
  eq_gather_kernel<<<grid, EQ_THREADS, 0, (hipStream_t)stream>>>(src_dev, src_off_dev, stride, bins_dev, npts, nfft / 2 + 1,
                                                                 out_dev);
  IRA_RETURN_LAUNCH();
}

extern "C" int32_t ira_eq_taper(const float* g_dev, const int64_t* g_off_dev, const double* taper_dev, int32_t nrows,
                                int32_t taps, int32_t nfft, float* f_dev, void* stream) {
  IRA_CHECK_PTR(g_dev); IRA_CHECK_PTR(g_off_dev); IRA_CHECK_PTR(taper_dev); IRA_CHECK_PTR(f_dev);
  if (!eq_sizes_ok(nrows, nfft)) return IRA_E_SIZE;
  if (taps < 1 || taps > nfft / 2) return IRA_E_SIZE;
  if (nrows == 0) return IRA_OK;
  const dim3 grid(eq_blocks(taps), (unsigned)nrows);
  eq_taper_kernel<<<grid, EQ_THREADS, 0, (hipStream_t)stream>>>(g_dev, g_off_dev, taper_dev, taps, f_dev);
  IRA_RETURN_LAUNCH();
}
