// Energy decay relief (Jot): the Schroeder backward integration at every frequency row of a short-time transform.  Nothing in
// the reference computes it; include/ira_edr.h pins the definitions (the order of a row's sum, the order of the backward sum,
// the record) and the host side is audio_analysis_amd/analyse/edr.py.
//
//   edr_power_kernel (chunks x segments)  a workgroup walks the EDR_FRAMES frames of its chunk two at a time.  Per pair:
//       z[i] = w[i] x[m hop + i] + i w[i] x[(m + 1) hop + i] as float64 in LDS  ->  ONE n_fft-point complex lds_fft_dif
//       ->  unpacked as xspec_accumulate_kernel unpacks its two channels (a thread owns POSITIONS of the bit-reversed output,
//       not bins: consecutive lanes read consecutive even positions and their partners descend consecutively)  ->  the
//       bin powers of both frames into registers, and after a barrier into the transform's own LDS in BIN order (swizzled:
//       bin k < n/2 lies at k ^ (k >> (log2 n - 7)), so that the 64 bins a wave writes, which differ in their top six bits,
//       spread over the banks, and the consecutive bins a row sum reads stay a permutation of consecutive words)
//       ->  row sums (the order ira_edr.h states) into stage[row][frame of the chunk].
//     The staged (row, sf) block leaves as runs of sf doubles, plain stores: sf = EDR_FRAMES (128 bytes) wherever the LDS
//     holds the transform and nrows * EDR_FRAMES sums, half of it (64 bytes) at 8192 points with more than 254 rows.
//   edr_integrate_kernel (rows x segments, one wavefront each)  the noise level from a raw scan of the last blocks, the scan
//       of the (subtracted) powers for S(0), the record and the optional S, and the same scan again for the float32 curve.
// The frames of a chunk, the chunk boundaries and each thread's share are functions of n_fft, hop and the row table alone,
// and a workgroup reads and writes nothing of another segment: a segment's bytes are the same whatever else is in the batch.
// Built with -ffp-contract=off: the sums and the subtraction round one operation at a time (the transform calls fma itself).
#include <math.h>

#include "ira_edc_tile.h"
#include "ira_fft_lds.h"
#include "../../include/ira_edr.h"

namespace {

using ira::cplx;

constexpr int EDR_THREADS = 256;
constexpr int EDR_FRAMES = IRA_EDR_FRAMES;
constexpr int EDR_BLOCK = IRA_EDR_BLOCK;
constexpr int EDR_MIN_FFT = 256, EDR_MAX_FFT = 8192;
constexpr size_t EDR_CU_LDS = 160 * 1024, EDR_STATIC_LDS = 256;
static_assert(EDR_FRAMES == 16 && EDR_BLOCK == IRA_WAVE, "a store run is 16 doubles, a block of the backward sum one wavefront");

__device__ __forceinline__ int64_t edr_frames(int64_t len, int n, int hop) { return len >= n ? 1 + (len - n) / hop : 0; }
__host__ __device__ __forceinline__ int64_t edr_pad(int64_t T) { return (T + EDR_FRAMES - 1) / EDR_FRAMES * EDR_FRAMES; }
__device__ __forceinline__ bool edr_finite(double v) { return fabs(v) < __longlong_as_double(0x7ff0000000000000ll); }

// where bin k <= n/2 of a frame's powers lies in LDS (see the head of the file); sh = log2 n - 7 >= 1
__device__ __forceinline__ unsigned edr_slot(unsigned k, unsigned half, int sh) { return k < half ? k ^ (k >> sh) : half; }

// NB: positions per thread, n_fft / 512 + 1 (the + 1: position 1, the Nyquist bin, is slot n_fft / 2)
template <int NB>
__global__ __launch_bounds__(EDR_THREADS) void edr_power_kernel(
    const float* __restrict__ x, const int64_t* __restrict__ x_off, const int64_t* __restrict__ n_of,
    const int64_t* __restrict__ p_off, int log2n, int hop, const double* __restrict__ window,
    const cplx<double>* __restrict__ tw, const int32_t* __restrict__ row_first, const int32_t* __restrict__ row_count,
    int nrows, int sf, double* __restrict__ p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  cplx<double>* buf = reinterpret_cast<cplx<double>*>(smem_raw);
  double* pw = reinterpret_cast<double*>(smem_raw);                      // the pair's bin powers: 2 (n/2 + 1) <= 2 n doubles
  double* stage = reinterpret_cast<double*>(smem_raw + (sizeof(cplx<double>) << log2n));   // [nrows][sf]
  const int seg = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
  const int n = 1 << log2n, half = n >> 1, nbins = half + 1, sh = log2n - 7;
  const int64_t T = edr_frames(ira::uniform(n_of[seg]), n, hop);
  const int64_t f0 = (int64_t)chunk * EDR_FRAMES;
  if (f0 >= T) return;                                                   // T <= Tpad < f0 + EDR_FRAMES: no padding of its own
  const int64_t f1 = f0 + EDR_FRAMES < T ? f0 + EDR_FRAMES : T;
  const float* xs = x + ira::uniform(x_off[seg]);
  const double qnan = ira::qnan();
  const int64_t Tpad = edr_pad(T);
  double* dst = p + ira::uniform(p_off[seg]) + f0;

  for (int i = tid; i < nrows * sf; i += EDR_THREADS) stage[i] = 0.0;    // published by the transform's barriers

  // every pair of the chunk, the ones past the last frame too: their columns are the zero padding this chunk owns
  for (int col = 0; col < EDR_FRAMES; col += 2) {
    const int64_t m = f0 + col;
    if (m < f1) {
    const bool two = m + 1 < f1;                                         // a last unpaired frame rides with zeros
    const float* fa = xs + m * hop;
    const float* fb = fa + hop;
    int nza = 0, nzb = 0, nfa = 0, nfb = 0;
    for (int i = tid; i < n; i += EDR_THREADS) {
      const double w = window[i];
      const double a = (double)fa[i] * w, b = two ? (double)fb[i] * w : 0.0;
      nza |= a != 0.0;
      nzb |= b != 0.0;
      nfa |= !edr_finite(a);
      nfb |= !edr_finite(b);
      buf[i] = {a, b};
    }
    // A frame that holds a non-finite windowed sample has NaN in every bin; it rides as zeros, so that its partner, which
    // need not cover that sample, keeps its own spectrum.
    const bool bad_a = __syncthreads_or(nfa) != 0;
    const bool bad_b = __syncthreads_or(nfb) != 0;
    if (bad_a || bad_b) {
      for (int i = tid; i < n; i += EDR_THREADS) {                       // the elements this thread wrote itself
        const cplx<double> z = buf[i];
        buf[i] = {bad_a ? 0.0 : z.re, bad_b ? 0.0 : z.im};
      }
    }
    // A frame whose windowed samples are all zero has the spectrum 0, exactly: unpacked from the joint transform it would
    // carry its partner's rounding error instead (synthetic tails end in digital silence).
    const bool live_a = __syncthreads_or(nza) != 0 && !bad_a;
    const bool live_b = __syncthreads_or(nzb) != 0 && !bad_b;
    ira::lds_fft_dif<double>(buf, log2n, tw, 1u, tid, EDR_THREADS);      // ends with a barrier
    double pa[NB], pb[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int s = tid + EDR_THREADS * j;
      pa[j] = pb[j] = 0.0;
      if (s <= half) {
        const unsigned a = s < half ? 2u * (unsigned)s : 1u;
        const unsigned q = a < 2u ? a : a ^ ((1u << (31 - __clz((int)a))) - 1u);
        const cplx<double> zk = buf[a], zp = buf[q];
        const double ar = 0.5 * (zk.re + zp.re), ai = 0.5 * (zk.im - zp.im);
        const double br = 0.5 * (zk.im + zp.im), bi = -0.5 * (zk.re - zp.re);
        pa[j] = bad_a ? qnan : (live_a ? ar * ar + ai * ai : 0.0);
        pb[j] = bad_b ? qnan : (live_b ? br * br + bi * bi : 0.0);
      }
    }
    __syncthreads();                                                     // every position is read: the powers take the buffer
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int s = tid + EDR_THREADS * j;
      if (s <= half) {
        const unsigned k = s < half ? ira::lds_brev(2u * (unsigned)s, log2n) : (unsigned)half;
        const unsigned o = edr_slot(k, (unsigned)half, sh);
        pw[o] = pa[j];
        pw[nbins + o] = pb[j];
      }
    }
    __syncthreads();
    const int sc = col & (sf - 1);
    // rows of up to IRA_EDR_SERIAL bins: one thread per (row, frame), ascending from 0.0
    for (int t = tid; t < 2 * nrows; t += EDR_THREADS) {
      const int row = t >> 1, h = t & 1;
      int first = row_first[row], count = row_count[row];
      first = first < 0 ? 0 : (first > nbins ? nbins : first);
      count = count < 0 ? 0 : (count > nbins - first ? nbins - first : count);
      if (count <= IRA_EDR_SERIAL) {
        const double* src = pw + h * nbins;
        double v = 0.0;
        for (int k = first; k < first + count; ++k) v += src[edr_slot((unsigned)k, (unsigned)half, sh)];
        stage[row * sf + sc + h] = v;
      }
    }
    // wider rows: half a wavefront per (row, frame), 32 strided partial sums and a butterfly
    {
      const int wave = tid >> 6, lane = tid & 63, h = lane >> 5, l = lane & 31;
      for (int row = wave; row < nrows; row += EDR_THREADS / IRA_WAVE) {
        int first = ira::uniform(row_first[row]), count = ira::uniform(row_count[row]);
        first = first < 0 ? 0 : (first > nbins ? nbins : first);
        count = count < 0 ? 0 : (count > nbins - first ? nbins - first : count);
        if (count <= IRA_EDR_SERIAL) continue;
        const double* src = pw + h * nbins;
        double v = 0.0;
        for (int k = first + l; k < first + count; k += 32) v += src[edr_slot((unsigned)k, (unsigned)half, sh)];
#pragma unroll
        for (int d = 16; d > 0; d >>= 1) v = v + __shfl_xor(v, d, 64);
        if (l == 0) stage[row * sf + sc + h] = v;
      }
    }
    __syncthreads();                                                     // the next pair overwrites the powers
    }
    if (((col + 2) & (sf - 1)) == 0) {                                   // sf staged frames leave: sf lanes a run of 8 sf bytes
      __syncthreads();
      for (int i = tid; i < nrows * sf; i += EDR_THREADS) {
        dst[(int64_t)(i / sf) * Tpad + (col + 2 - sf) + (i & (sf - 1))] = stage[i];
        stage[i] = 0.0;                                                  // its own entry; published by the barriers that follow
      }
    }
  }
}

// ---- the backward sum -------------------------------------------------------------------------------------------------------
// (value, index) of numpy.max / numpy.argmax: a NaN beats a number, the smaller index wins a tie; index -1 is "none yet"
__device__ __forceinline__ bool edr_beats(double v2, int i2, double v1, int i1) {
  if (i2 < 0) return false;
  if (i1 < 0) return true;
  const bool n1 = v1 != v1, n2 = v2 != v2;
  if (n1 || n2) return (n1 && n2) ? i2 < i1 : n2;
  return v2 > v1 || (v2 == v1 && i2 < i1);
}

__global__ __launch_bounds__(IRA_WAVE) void edr_integrate_kernel(
    const double* __restrict__ p, const int64_t* __restrict__ p_off, const int32_t* __restrict__ T_of,
    const int32_t* __restrict__ q_of, const int64_t* __restrict__ c_off, int nrows, double eps, double floor_db,
    float* __restrict__ curve, double* __restrict__ rec, double* __restrict__ s_out) {
  __shared__ ira::LogTabEntry ltab[ira::LOGTAB_N];
  const int seg = blockIdx.y, row = blockIdx.x, lane = threadIdx.x;
  ira::build_log_table(ltab, lane);
  ira::build_log_table(ltab, lane + IRA_WAVE);
  __syncthreads();
  const int T = ira::uniform(T_of[seg]);
  double* r = rec + ((int64_t)seg * nrows + row) * IRA_EDR_DOUBLES;
  if (T <= 0) {
    if (lane == 0) { r[0] = 0.0; r[1] = 0.0; r[2] = ira::qnan(); r[3] = -1.0; }
    return;
  }
  int q = ira::uniform(q_of[seg]);
  q = q < 0 ? 0 : (q > T ? T : q);
  const int64_t Tpad = edr_pad(T);
  const int64_t base = ira::uniform(p_off[seg]) + (int64_t)row * Tpad;
  const double* P = p + base;
  const int nblk = (T + EDR_BLOCK - 1) / EDR_BLOCK;
  double excl;

  // the noise level: the raw backward sum up to the block that holds frame T - q
  double noise = 0.0;
  if (q >= 1) {
    const int bq = (q - 1) / EDR_BLOCK;
    double carry = 0.0, at = 0.0;
    for (int b = 0; b <= bq; ++b) {
      const int idx = T - EDR_BLOCK * (b + 1) + lane;
      const double out = ira::wave_suffix(idx >= 0 ? P[idx] : 0.0, lane, excl) + carry;
      carry = __shfl(out, 0, 64);
      if (b == bq) at = __shfl(out, T - q - (T - EDR_BLOCK * (bq + 1)), 64);
    }
    noise = at / (double)q;
  }

  // S, its first value, the maximum of P
  double best = 0.0, s0 = 0.0;
  int best_at = -1;
  {
    double carry = 0.0;
    for (int b = 0; b < nblk; ++b) {
      const int idx = T - EDR_BLOCK * (b + 1) + lane;
      const double pv = idx >= 0 ? P[idx] : 0.0;
      const double a = (idx >= 0 && q >= 1) ? pv - noise : pv;
      const double out = ira::wave_suffix(a, lane, excl) + carry;
      carry = __shfl(out, 0, 64);
      if (idx >= 0) {
        if (edr_beats(pv, idx, best, best_at)) { best = pv; best_at = idx; }
        if (s_out) s_out[base + idx] = out;
      }
      if (b == nblk - 1) s0 = __shfl(out, EDR_BLOCK * nblk - T, 64);     // the lane of frame 0
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(best_at, o, 64);
    if (edr_beats(ov, oi, best, best_at)) { best = ov; best_at = oi; }
  }
  if (lane == 0) { r[0] = s0; r[1] = noise; r[2] = best; r[3] = (double)best_at; }
  if (s_out)
    for (int64_t i = T + lane; i < Tpad; i += IRA_WAVE) s_out[base + i] = 0.0;

  // the curve
  const bool silent = edr_finite(s0) && s0 <= eps;
  const ira::EdcDb D(s0, eps, floor_db, ltab);
  float* y = curve + ira::uniform(c_off[seg]) + (int64_t)row * T;
  double carry = 0.0;
  for (int b = 0; b < nblk; ++b) {
    const int idx = T - EDR_BLOCK * (b + 1) + lane;
    const double pv = idx >= 0 ? P[idx] : 0.0;
    const double a = (idx >= 0 && q >= 1) ? pv - noise : pv;
    const double out = ira::wave_suffix(a, lane, excl) + carry;
    carry = __shfl(out, 0, 64);
    if (idx >= 0) y[idx] = silent ? (float)floor_db : D.db32(out);
  }
}

inline int32_t edr_check(int32_t nseg, int32_t nrows) {
  if (nseg < 0 || nseg > 65535 || nrows < 1 || nrows > IRA_EDR_MAX_ROWS) return IRA_E_SIZE;
  return IRA_OK;
}

template <int NB>
int32_t edr_launch(const float* x, const int64_t* x_off, const int64_t* n_of, const int64_t* p_off, int32_t nseg, int chunks,
                   int log2n, int32_t hop, const double* window, const double* tw, const int32_t* row_first,
                   const int32_t* row_count, int32_t nrows, double* p, hipStream_t st) {
  // 128 KiB + 32 KiB at 8192 points and 256 rows are the CU's 160 KiB, and the block-wide votes take EDR_STATIC_LDS bytes
  // of their own (the compiler's resource report): from 255 rows on at 8192 points half a chunk is staged per store
  const size_t fft = sizeof(cplx<double>) << log2n;
  const int sf = fft + sizeof(double) * EDR_FRAMES * (size_t)nrows + EDR_STATIC_LDS <= EDR_CU_LDS ? EDR_FRAMES : EDR_FRAMES / 2;
  const size_t lds = fft + sizeof(double) * (size_t)sf * (size_t)nrows;
  IRA_TRY_HIP(allow_lds(edr_power_kernel<NB>, lds));
  edr_power_kernel<NB><<<dim3((unsigned)chunks, (unsigned)nseg), EDR_THREADS, lds, st>>>(
      x, x_off, n_of, p_off, log2n, hop, window, reinterpret_cast<const cplx<double>*>(tw), row_first, row_count, nrows, sf,
      p);
  IRA_RETURN_LAUNCH();
}

}  // namespace

extern "C" int32_t ira_edr_power(const float* x_dev, const int64_t* x_off_dev, const int64_t* n_dev, const int64_t* p_off_dev,
                                 int32_t nseg, int32_t max_frames, int32_t n_fft, int32_t hop, const double* window_dev,
                                 const double* twiddle_dev, const int32_t* row_first_dev, const int32_t* row_count_dev,
                                 int32_t nrows, double* p_dev, void* stream) {
  IRA_CHECK_PTR(x_dev); IRA_CHECK_PTR(x_off_dev); IRA_CHECK_PTR(n_dev); IRA_CHECK_PTR(p_off_dev);
  IRA_CHECK_PTR(window_dev); IRA_CHECK_PTR(twiddle_dev); IRA_CHECK_PTR(row_first_dev); IRA_CHECK_PTR(row_count_dev);
  IRA_CHECK_PTR(p_dev);
  const int32_t rc = edr_check(nseg, nrows);
  if (rc != IRA_OK) return rc;
  if (n_fft < EDR_MIN_FFT || n_fft > EDR_MAX_FFT || (n_fft & (n_fft - 1)) != 0) return IRA_E_SIZE;
  if (hop < 1 || hop > n_fft || max_frames < 0) return IRA_E_SIZE;
  if (nseg == 0 || max_frames == 0) return IRA_OK;
  int log2n = 0;
  while ((1 << log2n) < n_fft) ++log2n;
  hipStream_t st = (hipStream_t)stream;
  const int chunks = (int)(((int64_t)max_frames + EDR_FRAMES - 1) / EDR_FRAMES);
  if (n_fft <= 2048)
    return edr_launch<2048 / 512 + 1>(x_dev, x_off_dev, n_dev, p_off_dev, nseg, chunks, log2n, hop, window_dev, twiddle_dev,
                                      row_first_dev, row_count_dev, nrows, p_dev, st);
  if (n_fft == 4096)
    return edr_launch<4096 / 512 + 1>(x_dev, x_off_dev, n_dev, p_off_dev, nseg, chunks, log2n, hop, window_dev, twiddle_dev,
                                      row_first_dev, row_count_dev, nrows, p_dev, st);
  return edr_launch<8192 / 512 + 1>(x_dev, x_off_dev, n_dev, p_off_dev, nseg, chunks, log2n, hop, window_dev, twiddle_dev,
                                    row_first_dev, row_count_dev, nrows, p_dev, st);
}

extern "C" int32_t ira_edr_integrate(const double* p_dev, const int64_t* p_off_dev, const int32_t* T_dev, const int32_t* q_dev,
                                     const int64_t* c_off_dev, int32_t nseg, int32_t nrows, double eps, double floor_db,
                                     float* curve_dev, double* rec_dev, double* s_out_dev, void* stream) {
  IRA_CHECK_PTR(p_dev); IRA_CHECK_PTR(p_off_dev); IRA_CHECK_PTR(T_dev); IRA_CHECK_PTR(q_dev); IRA_CHECK_PTR(c_off_dev);
  IRA_CHECK_PTR(curve_dev); IRA_CHECK_PTR(rec_dev);
  const int32_t rc = edr_check(nseg, nrows);
  if (rc != IRA_OK) return rc;
  if (!(eps >= 0.0) || !isfinite(eps) || !isfinite(floor_db)) return IRA_E_SIZE;
  if (nseg == 0) return IRA_OK;
  edr_integrate_kernel<<<dim3((unsigned)nrows, (unsigned)nseg), IRA_WAVE, 0, (hipStream_t)stream>>>(
      p_dev, p_off_dev, T_dev, q_dev, c_off_dev, nrows, eps, floor_db, curve_dev, rec_dev, s_out_dev);
  IRA_RETURN_LAUNCH();
}
