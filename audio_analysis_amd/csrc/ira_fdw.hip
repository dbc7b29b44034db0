// Frequency-dependent-window (FDW) response: per channel and frequency point one windowed Fourier sum around a centre
// sample, the window a fixed number of cycles long, so its length falls with frequency (include/ira.h and
// audio_analysis_amd/analyse/fdw.py state the definition).  Nothing in the reference computes it.
//
// Compiled with -ffp-contract=off for the reduction of the turn count (ira_wavelet.h, which holds the term's weight and
// phasor); the sums call fma themselves.
//
//   fdw_plan_kernel     one workgroup.  From half_dev: first[j] = the first chunk of point j (a narrow point has none),
//                       first[npts] = T, job_point[b] = the point of chunk b, narrow_point[m] = the m-th narrow point.
//                       Thread t owns the points 16 t .. 16 t + 15; a wave scan and four wave totals give its offsets.
//   fdw_narrow_kernel   grid (ceil(M / 4), channels), 256 threads: ONE WAVEFRONT PER NARROW POINT (2 H + 1 <= 255 terms).
//                       Lane l takes the terms l, l + 64, l + 128, l + 192; the top four octaves of a 15-cycle grid at
//                       48 kHz are all of this kind and would leave three quarters and more of a workgroup idle each.
//   fdw_wide_kernel     grid (T, channels), 256 threads: one chunk of IRA_FDW_CHUNK consecutive terms of one wide point;
//                       thread t takes the terms t, t + 256, ..: the loads of a round are 256 consecutive floats.  Its
//                       five sums go to scratch with plain stores.
//   fdw_finish_kernel   one thread per (channel, wide point): adds the point's chunks in ascending order, writes the six
//                       fields.
// Per term: two float64 multiplies and an fma for the turn count, rint, two adds, sincospi; for hann one multiply, sinpi
// and a square; five multiplies, four fmas and an add for the sums.  Every table entry read on the device is clamped to
// its range, so no store leaves out_dev or scratch_dev even if half_dev does not hold the values of half.
#include <math.h>

#include "ira_common.h"
#include "ira_reduce.h"
#include "ira_wavelet.h"

namespace {

constexpr int FDW_THREADS = 256;
constexpr int FDW_WAVES = FDW_THREADS / IRA_WAVE;
constexpr int FDW_ROUNDS = IRA_FDW_CHUNK / FDW_THREADS;                  // terms per thread of a wide chunk
constexpr int FDW_NARROW_ROUNDS = (2 * IRA_FDW_NARROW_HALF + 1 + IRA_WAVE - 1) / IRA_WAVE;
constexpr int FDW_PLAN_PER_THREAD = IRA_FDW_MAX_POINTS / FDW_THREADS;
static_assert(IRA_FDW_CHUNK % FDW_THREADS == 0, "whole rounds");
static_assert(FDW_NARROW_ROUNDS == 4 && 2 * IRA_FDW_NARROW_HALF + 1 <= FDW_NARROW_ROUNDS * IRA_WAVE, "a narrow point fits a wave's rounds");
static_assert(FDW_PLAN_PER_THREAD * FDW_THREADS == IRA_FDW_MAX_POINTS, "the plan's workgroup covers every point");

__host__ __device__ inline int64_t fdw_chunks(int h) {
  return h <= IRA_FDW_NARROW_HALF ? 0 : (2 * (int64_t)h + 1 + IRA_FDW_CHUNK - 1) / IRA_FDW_CHUNK;
}

struct FdwChannel {
  const float* x;
  int64_t len, p;
};

__device__ __forceinline__ FdwChannel fdw_channel(const float* x, const int64_t* off, const int64_t* len,
                                                  const int64_t* centre, int c) {
  FdwChannel ch;
  ch.x = x + ira::uniform(off[c]);
  ch.len = ira::uniform(len[c]);
  ch.len = ch.len > 0 ? ch.len : 0;
  ch.p = ira::wavelet_centre(ira::uniform(centre[c]));
  return ch;
}

// the number of terms of the window p - H .. p + H inside [0, len)
__device__ __forceinline__ int64_t fdw_inside(const FdwChannel& ch, int h) {
  const int64_t lo = ch.p - h > 0 ? ch.p - h : 0;
  const int64_t hi = ch.p + h < ch.len - 1 ? ch.p + h : ch.len - 1;
  return hi >= lo ? hi - lo + 1 : 0;
}

struct FdwSums {
  double v[IRA_FDW_SUMS];                                                // Re S0, Im S0, Re S1, Im S1, A
};

// R terms u0 + stride r of the window (term u is k = u - H), the loads of all of them in flight before the arithmetic
template <int R>
__device__ __forceinline__ FdwSums fdw_terms(const FdwChannel& ch, int h, double rho, int window, int u0, int stride) {
  float xv[R];
  bool in[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int u = u0 + stride * r;
    const int64_t i = ch.p + (u - h);
    in[r] = u >= 0 && u <= 2 * h && i >= 0 && i < ch.len;
    xv[r] = in[r] ? ch.x[i] : 0.0f;
  }
  const double inv = 1.0 / (double)(2 * h + 2);
  FdwSums s;
#pragma unroll
  for (int q = 0; q < IRA_FDW_SUMS; ++q) s.v[q] = 0.0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (!in[r]) continue;
    const int k = u0 + stride * r - h;
    double sn, cs;
    const double v = ira::wavelet_term(k, h, rho, window, [inv] { return inv; }, &sn, &cs) * (double)xv[r];
    const double kv = (double)k * v;
    s.v[0] = fma(v, cs, s.v[0]);
    s.v[1] = fma(-v, sn, s.v[1]);
    s.v[2] = fma(kv, cs, s.v[2]);
    s.v[3] = fma(-kv, sn, s.v[3]);
    s.v[4] += fabs(v);
  }
  return s;
}

__global__ __launch_bounds__(FDW_THREADS) void fdw_plan_kernel(const int32_t* __restrict__ half_dev, int npts, int total,
                                                               int n_narrow, int32_t* __restrict__ first,
                                                               int32_t* __restrict__ job_point,
                                                               int32_t* __restrict__ narrow_point) {
  __shared__ int s_wide[FDW_WAVES], s_narrow[FDW_WAVES];
  const int t = threadIdx.x, lane = t & (IRA_WAVE - 1), wv = t / IRA_WAVE;
  const int j0 = t * FDW_PLAN_PER_THREAD;
  int cnt[FDW_PLAN_PER_THREAD], wide = 0, narrow = 0;
#pragma unroll
  for (int q = 0; q < FDW_PLAN_PER_THREAD; ++q) {
    const int j = j0 + q;
    cnt[q] = j < npts ? (int)fdw_chunks(ira::wavelet_half(half_dev, j)) : -1;     // -1: no such point
    wide += cnt[q] > 0 ? cnt[q] : 0;
    narrow += cnt[q] == 0;
  }
  int wide_before, narrow_before;
  const int wide_incl = ira::wave_prefix(wide, lane, wide_before);
  const int narrow_incl = ira::wave_prefix(narrow, lane, narrow_before);
  if (lane == IRA_WAVE - 1) { s_wide[wv] = wide_incl; s_narrow[wv] = narrow_incl; }
  __syncthreads();
  for (int w = 0; w < wv; ++w) { wide_before += s_wide[w]; narrow_before += s_narrow[w]; }
#pragma unroll
  for (int q = 0; q < FDW_PLAN_PER_THREAD; ++q) {
    const int j = j0 + q;
    if (cnt[q] < 0) continue;
    first[j] = wide_before;
    if (cnt[q] == 0) {
      if (narrow_before < n_narrow) narrow_point[narrow_before] = j;
      ++narrow_before;
    }
    for (int b = 0; b < cnt[q]; ++b)
      if (wide_before + b < total) job_point[wide_before + b] = j;
    wide_before += cnt[q];
    if (j == npts - 1) first[npts] = wide_before;
  }
}

__global__ __launch_bounds__(FDW_THREADS) void fdw_narrow_kernel(const float* __restrict__ x, const int64_t* __restrict__ off,
                                                                 const int64_t* __restrict__ len,
                                                                 const int64_t* __restrict__ centre,
                                                                 const double* __restrict__ rho_dev,
                                                                 const int32_t* __restrict__ half_dev,
                                                                 const int32_t* __restrict__ narrow_point, int n_narrow,
                                                                 int npts, int window, double* __restrict__ out) {
  const int lane = threadIdx.x & (IRA_WAVE - 1);
  const int m = blockIdx.x * FDW_WAVES + threadIdx.x / IRA_WAVE;
  if (m >= n_narrow) return;                                             // the whole wave
  const int c = blockIdx.y;
  int j = ira::uniform(narrow_point[m]);
  j = j < 0 ? 0 : (j >= npts ? npts - 1 : j);
  int h = ira::uniform(ira::wavelet_half(half_dev, j));
  h = h > IRA_FDW_NARROW_HALF ? IRA_FDW_NARROW_HALF : h;
  const double rho = ira::uniform(rho_dev[j]);
  const FdwChannel ch = fdw_channel(x, off, len, centre, c);
  FdwSums s = fdw_terms<FDW_NARROW_ROUNDS>(ch, h, rho, window, lane, IRA_WAVE);
#pragma unroll
  for (int q = 0; q < IRA_FDW_SUMS; ++q) s.v[q] = ira::wave_sum(s.v[q]);
  if (lane == 0) {
    double* o = out + ((int64_t)c * npts + j) * IRA_FDW_FIELDS;
#pragma unroll
    for (int q = 0; q < IRA_FDW_SUMS; ++q) o[q] = s.v[q];
    o[IRA_FDW_SUMS] = (double)fdw_inside(ch, h);
  }
}

__global__ __launch_bounds__(FDW_THREADS) void fdw_wide_kernel(const float* __restrict__ x, const int64_t* __restrict__ off,
                                                               const int64_t* __restrict__ len,
                                                               const int64_t* __restrict__ centre,
                                                               const double* __restrict__ rho_dev,
                                                               const int32_t* __restrict__ half_dev,
                                                               const int32_t* __restrict__ first,
                                                               const int32_t* __restrict__ job_point, int npts, int window,
                                                               double* __restrict__ partial) {
  __shared__ double s_part[FDW_WAVES][IRA_FDW_SUMS];
  const int t = threadIdx.x, lane = t & (IRA_WAVE - 1), wv = t / IRA_WAVE;
  const int b = blockIdx.x, c = blockIdx.y;
  int j = ira::uniform(job_point[b]);
  j = j < 0 ? 0 : (j >= npts ? npts - 1 : j);
  const int h = ira::uniform(ira::wavelet_half(half_dev, j));
  const double rho = ira::uniform(rho_dev[j]);
  int chunk = b - ira::uniform(first[j]);
  chunk = chunk < 0 || chunk >= fdw_chunks(h) ? -1 : chunk;              // a chunk the point does not have: no term
  const FdwChannel ch = fdw_channel(x, off, len, centre, c);
  FdwSums s;
  if (chunk >= 0) {
    s = fdw_terms<FDW_ROUNDS>(ch, h, rho, window, chunk * IRA_FDW_CHUNK + t, FDW_THREADS);
  } else {
#pragma unroll
    for (int q = 0; q < IRA_FDW_SUMS; ++q) s.v[q] = 0.0;
  }
#pragma unroll
  for (int q = 0; q < IRA_FDW_SUMS; ++q) {
    s.v[q] = ira::wave_sum(s.v[q]);
    if (lane == 0) s_part[wv][q] = s.v[q];
  }
  __syncthreads();
  if (t < IRA_FDW_SUMS) {
    double v = s_part[0][t];
    for (int w = 1; w < FDW_WAVES; ++w) v += s_part[w][t];
    partial[((int64_t)c * gridDim.x + b) * IRA_FDW_SUMS + t] = v;
  }
}

__global__ __launch_bounds__(FDW_THREADS) void fdw_finish_kernel(const int64_t* __restrict__ len,
                                                                 const int64_t* __restrict__ centre,
                                                                 const int32_t* __restrict__ half_dev,
                                                                 const int32_t* __restrict__ first, int npts, int total,
                                                                 const double* __restrict__ partial,
                                                                 double* __restrict__ out) {
  const int j = blockIdx.x * FDW_THREADS + threadIdx.x, c = blockIdx.y;
  if (j >= npts) return;
  int b0 = first[j], b1 = first[j + 1];
  b0 = b0 < 0 ? 0 : b0;
  b1 = b1 > total ? total : b1;
  if (b1 <= b0) return;                                                  // a narrow point: written by its own launch
  const double* p = partial + ((int64_t)c * total + b0) * IRA_FDW_SUMS;
  double v[IRA_FDW_SUMS];
#pragma unroll
  for (int q = 0; q < IRA_FDW_SUMS; ++q) v[q] = p[q];
  for (int b = 1; b < b1 - b0; ++b) {
#pragma unroll
    for (int q = 0; q < IRA_FDW_SUMS; ++q) v[q] += p[(int64_t)b * IRA_FDW_SUMS + q];
  }
  FdwChannel ch;
  ch.x = nullptr;
  ch.len = len[c] > 0 ? len[c] : 0;
  ch.p = ira::wavelet_centre(centre[c]);
  double* o = out + ((int64_t)c * npts + j) * IRA_FDW_FIELDS;
#pragma unroll
  for (int q = 0; q < IRA_FDW_SUMS; ++q) o[q] = v[q];
  o[IRA_FDW_SUMS] = (double)fdw_inside(ch, ira::wavelet_half(half_dev, j));
}

// T = the chunks of the wide points, M = the number of narrow points, of a checked grid
void fdw_counts(const int32_t* half, int32_t npts, int64_t* total, int64_t* narrow) {
  *total = *narrow = 0;
  for (int32_t j = 0; j < npts; ++j) {
    const int64_t n = fdw_chunks(half[j]);
    *total += n;
    *narrow += n == 0;
  }
}

int64_t fdw_table_doubles(int32_t npts, int64_t total, int64_t narrow) { return (npts + 1 + total + narrow + 1) / 2; }

}  // namespace

extern "C" int64_t ira_fdw_scratch_doubles(int32_t nch, const int32_t* half, int32_t npts) {
  if (nch < 0 || nch > 65535) return IRA_E_SIZE;
  const int32_t rc = ira::wavelet_points_check(nullptr, half, npts, 0);
  if (rc != IRA_OK) return rc;
  int64_t total, narrow;
  fdw_counts(half, npts, &total, &narrow);
  return (int64_t)nch * total * IRA_FDW_SUMS + fdw_table_doubles(npts, total, narrow);
}

extern "C" int32_t ira_fdw_response(const float* x_dev, const int64_t* off_dev, const int64_t* len_dev,
                                    const int64_t* centre_dev, int32_t nch, const double* rho, const int32_t* half,
                                    const double* rho_dev, const int32_t* half_dev, int32_t npts, int32_t window,
                                    double* scratch_dev, int64_t scratch_doubles, double* out_dev, void* stream) {
  IRA_CHECK_PTR(x_dev); IRA_CHECK_PTR(off_dev); IRA_CHECK_PTR(len_dev); IRA_CHECK_PTR(centre_dev); IRA_CHECK_PTR(rho);
  IRA_CHECK_PTR(half); IRA_CHECK_PTR(rho_dev); IRA_CHECK_PTR(half_dev); IRA_CHECK_PTR(scratch_dev); IRA_CHECK_PTR(out_dev);
  if (nch < 0 || nch > 65535) return IRA_E_SIZE;
  const int32_t rc = ira::wavelet_points_check(rho, half, npts, window);
  if (rc != IRA_OK) return rc;
  int64_t total, narrow;
  fdw_counts(half, npts, &total, &narrow);
  const int64_t sums = (int64_t)nch * total * IRA_FDW_SUMS;
  if (scratch_doubles < sums + fdw_table_doubles(npts, total, narrow)) return IRA_E_SIZE;
  if (nch == 0 || npts == 0) return IRA_OK;
  hipStream_t st = (hipStream_t)stream;
  int32_t* first = reinterpret_cast<int32_t*>(scratch_dev + sums);
  int32_t* job_point = first + npts + 1;
  int32_t* narrow_point = job_point + total;
  fdw_plan_kernel<<<1, FDW_THREADS, 0, st>>>(half_dev, npts, (int)total, (int)narrow, first, job_point, narrow_point);
  if (narrow > 0)
    fdw_narrow_kernel<<<dim3((unsigned)ira::ceil_div(narrow, FDW_WAVES), nch), FDW_THREADS, 0, st>>>(
        x_dev, off_dev, len_dev, centre_dev, rho_dev, half_dev, narrow_point, (int)narrow, npts, window, out_dev);
  if (total > 0) {
    fdw_wide_kernel<<<dim3((unsigned)total, nch), FDW_THREADS, 0, st>>>(x_dev, off_dev, len_dev, centre_dev, rho_dev,
                                                                        half_dev, first, job_point, npts, window,
                                                                        scratch_dev);
    fdw_finish_kernel<<<dim3((unsigned)ira::ceil_div(npts, FDW_THREADS), nch), FDW_THREADS, 0, st>>>(
        len_dev, centre_dev, half_dev, first, npts, (int)total, scratch_dev, out_dev);
  }
  IRA_RETURN_LAUNCH();
}
