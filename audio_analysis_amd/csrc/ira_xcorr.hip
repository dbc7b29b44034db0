// ISO 3382-1 Annex B inter-channel cross-correlation (IACC_E / IACC_L / IACC_A): float64 lag sums between the two channels
// of a stereo pair, partitioned in time.  Nothing in the reference computes these; the host side is
// audio_analysis_amd/analyse/iacc.py.
// Compiled with -ffp-contract=off.  The lag products are written as fma() on purpose: the product of two float32 samples is
// exact in float64 (48 significant bits), so fma(l, r, acc) and acc + l * r round identically, bit for bit.
#include "ira_common.h"
#include "ira_reduce.h"

namespace {

// ------------------------------------------------------------------------------------------------
// Segment j is one signal row of a pair (the broadband signals, or one band of both channels): left channel at l_off[j],
// right channel at r_off[j], both len[j] samples.  o = min(onset[lchan[j]], onset[rchan[j]]), L = len - o, n counted from o.
// With the segment's limits N_1 <= ... <= N_K (clamped to L) the partitions are [0, N_1), ..., [N_K, L), and for each of them
//   C(tau) = sum_n l[o + n] r[o + n + tau]  (-T <= tau <= T; r = 0 outside the file, never wrapped),
//   El = sum_n l[o + n]^2,  Er = sum_n r[o + n]^2.
//   xcorr_partial_kernel (chunks x segments, 512 threads)  one record of 2T + 3 doubles per (chunk, partition it overlaps)
//   xcorr_fold_kernel    (segments x partitions, 1 wave)   the records of a partition added in ascending chunk order -> out
//
// Tiling (after ar_lag_kernel in ira_ar.hip, whose comment records that LDS data return, not the FMAs, bounds this shape of
// kernel).  A workgroup stages rows [c0, c0 + XC_CHUNK) of l in LDS as float64, and r from T samples before to W - 1 - T
// samples after them (W = LPT * ngroups >= 2T + 1 lag slots).  A thread owns LPT consecutive lags and a sub-range of the
// rows and slides an LPT-value register window over r: a row costs TWO LDS reads for LPT FMAs.  The window advances
// under compile-time renaming (an LPT-row unrolled body, no moves).  LPT is ODD (ira_diffusion.hip, LG): neighbouring
// lanes read r LPT doubles apart, and an even count folds a half wave onto a few bank pairs.  Sub-range lengths are odd
// for the same reason (lanes of different sub-ranges read l that far apart).
//
// Every chunk boundary, every thread's share of a chunk and every reduction order is a function of the segment's own
// length, onset and limits (and of T): a pair's sums are bit-identical alone, in a ragged batch, at any place in it and at any
// 4-byte alignment (the staging loads are scalar float loads).  No atomics.
// A chunk that a limit cuts (one or two per limit and segment) is processed once per partition it overlaps, staging its
// samples again each time: the sample area of LDS doubles as the area of the sub-range partials.
// Record r of a segment: chunk c and partition j share record c + j, which is unique because chunks and partitions both ascend
// (stride = chunks of the longest segment + nlim records).
// ------------------------------------------------------------------------------------------------
constexpr int XC_CHUNK = 4096;
constexpr int XC_THREADS = 512;
constexpr int XC_WAVES = XC_THREADS / IRA_WAVE;
constexpr int XC_MAX_LIMITS = 4;
constexpr int XC_STAGE = 8;                                   // staging loads in flight per thread
constexpr int64_t XC_MAX_LEN = (int64_t)1 << 31;
static_assert(IRA_XCORR_MAX_LAG == 128, "the lags-per-thread candidates below are sized for 257 lags");

// lags per thread: the odd candidate that wastes the fewest lag slots (ties: the wider one)
inline int xc_lags_per_thread(int nlag) {
  int best = 9, best_waste = 1 << 30;
  for (int c : {13, 11, 9}) {
    const int waste = (nlag + c - 1) / c * c - nlag;
    if (waste < best_waste) { best_waste = waste; best = c; }
  }
  return best;
}
inline bool xc_shape_ok(int32_t nseg, int64_t max_len) { return nseg <= 65535 && max_len >= 0 && max_len <= XC_MAX_LEN; }
// LDS doubles: l rows | r rows + W; the partials ([nsub][W] <= 512 * 13 doubles, then El / Er per wave) reuse the space
inline size_t xc_lds_doubles(int w) { return (size_t)2 * XC_CHUNK + w; }

// cnt samples of src from file index first on (zeros outside [0, n_file)) -> dst as float64
__device__ __forceinline__ void xc_stage(const float* __restrict__ src, int64_t first, int64_t n_file, int cnt,
                                         double* __restrict__ dst) {
  for (int m0 = threadIdx.x; m0 < cnt; m0 += XC_STAGE * XC_THREADS) {
    float v[XC_STAGE];
#pragma unroll
    for (int u = 0; u < XC_STAGE; ++u) {                      // index clamped, value dropped afterwards (ar_lag_kernel)
      int64_t idx = first + m0 + u * XC_THREADS;
      idx = idx < 0 ? 0 : (idx < n_file ? idx : n_file - 1);
      v[u] = src[idx];
    }
#pragma unroll
    for (int u = 0; u < XC_STAGE; ++u) {
      const int m = m0 + u * XC_THREADS;
      const int64_t idx = first + m;
      if (m < cnt) dst[m] = (idx >= 0 && idx < n_file) ? (double)v[u] : 0.0;
    }
  }
}

template <int LPT>
__global__ __launch_bounds__(XC_THREADS) void xcorr_partial_kernel(
    const float* __restrict__ x, const int64_t* __restrict__ l_off, const int64_t* __restrict__ r_off,
    const int64_t* __restrict__ len, const int32_t* __restrict__ lchan, const int32_t* __restrict__ rchan,
    const int64_t* __restrict__ onset, const int64_t* __restrict__ limits, int nlim, int T, int64_t rec_stride,
    double* __restrict__ scratch) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int seg = blockIdx.y;
  const int64_t ol = ira::uniform(onset[ira::uniform(lchan[seg])]);
  const int64_t orr = ira::uniform(onset[ira::uniform(rchan[seg])]);
  const int64_t o = ol < orr ? ol : orr;
  const int64_t N = ira::uniform(len[seg]);
  const int64_t L = N - o;
  const int64_t c0 = (int64_t)blockIdx.x * XC_CHUNK;
  if (o < 0 || c0 >= L) return;                               // the fold reads only the chunks of the segment's length
  const int cnt = (int)(L - c0 < XC_CHUNK ? L - c0 : XC_CHUNK);
  const int nlag = 2 * T + 1, ngroups = (nlag + LPT - 1) / LPT, W = LPT * ngroups;
  const int nrec = nlag + 2;
  const int nsub = XC_THREADS / ngroups;                      // ngroups <= 29
  const float* xl = x + ira::uniform(l_off[seg]);
  const float* xr = x + ira::uniform(r_off[seg]);
  double* lds_l = reinterpret_cast<double*>(smem_raw);        // l[o + c0 + m], m < cnt
  double* lds_r = lds_l + XC_CHUNK;                           // r[o + c0 - T + m], m < cnt + W
  double* part = lds_l;                                       // [nsub][W] after the rows are done with
  double* wsum = lds_l + (size_t)XC_THREADS * 13;             // [XC_WAVES][2]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool active = tid < ngroups * nsub;
  const int g = active ? tid % ngroups : 0, sub = active ? tid / ngroups : 0;
  const int b0 = LPT * g;

  bool staged = false;
  for (int j = 0; j <= nlim; ++j) {                           // every bound below is workgroup-uniform
    int64_t a = j == 0 ? 0 : ira::uniform(limits[(int64_t)seg * nlim + j - 1]);
    int64_t b = j == nlim ? L : ira::uniform(limits[(int64_t)seg * nlim + j]);
    a = a < 0 ? 0 : (a < L ? a : L);
    b = b < a ? a : (b < L ? b : L);
    const int64_t lo = a > c0 ? a : c0, hi = b < c0 + cnt ? b : c0 + cnt;
    if (lo >= hi) continue;
    const int ra = (int)(lo - c0), rb = (int)(hi - c0), rows = rb - ra;
    if (staged) __syncthreads();                              // the previous partition's reduction has read the partials
    xc_stage(xl, o + c0, N, cnt, lds_l);
    xc_stage(xr, o + c0 - T, N, cnt + W, lds_r);
    staged = true;
    __syncthreads();

    const int sub_len = ((rows + nsub - 1) / nsub) | 1;
    double acc[LPT];
#pragma unroll
    for (int q = 0; q < LPT; ++q) acc[q] = 0.0;
    if (active) {
      const int r_begin = ra + sub * sub_len;
      const int r_end = r_begin + sub_len < rb ? r_begin + sub_len : rb;
      if (r_begin < r_end) {
        const double* cur = lds_l + r_begin;                  // l of the first row
        const double* nw = lds_r + r_begin + b0;              // r at the thread's first lag of that row
        double w[LPT];                                        // at unrolled step u, slot (q + u) mod LPT holds lag b0 + q
#pragma unroll
        for (int q = 0; q < LPT - 1; ++q) w[q] = nw[q];
        w[LPT - 1] = 0.0;
        nw += LPT - 1;                                        // the value that enters the window at the next row
        int r = r_begin;
        for (; r + LPT <= r_end; r += LPT) {
#pragma unroll
          for (int u = 0; u < LPT; ++u) {
            const double ln = cur[u];
            w[(LPT - 1 + u) % LPT] = nw[u];                   // the newest value takes the slot of the oldest
#pragma unroll
            for (int q = 0; q < LPT; ++q) acc[q] = fma(ln, w[(q + u) % LPT], acc[q]);
          }
          cur += LPT; nw += LPT;
        }
        for (; r < r_end; ++r) {                              // fewer than LPT rows left: one at a time, the window moved
          const double ln = *cur++;
          w[LPT - 1] = *nw++;
#pragma unroll
          for (int q = 0; q < LPT; ++q) acc[q] = fma(ln, w[q], acc[q]);
#pragma unroll
          for (int q = 0; q < LPT - 1; ++q) w[q] = w[q + 1];
        }
      }
    }
    double el = 0.0, er = 0.0;                                // rows ra + tid, + 512, ...: the same unshifted rows for both
    for (int r = ra + tid; r < rb; r += XC_THREADS) {
      const double dl = lds_l[r], dr = lds_r[r + T];
      el = fma(dl, dl, el);
      er = fma(dr, dr, er);
    }
    el = ira::wave_sum(el);
    er = ira::wave_sum(er);
    __syncthreads();                                          // every thread is done with the samples
    if (active) {
      double* dst = part + (size_t)sub * W + b0;
#pragma unroll
      for (int q = 0; q < LPT; ++q) dst[q] = acc[q];
    }
    if (lane == 0) { wsum[2 * wave] = el; wsum[2 * wave + 1] = er; }
    __syncthreads();
    double* rec = scratch + ((int64_t)seg * rec_stride + blockIdx.x + j) * nrec;
    for (int q = tid; q < nlag; q += XC_THREADS) {            // sub-ranges in eights, eights in eights: a short fixed tree
      double sum = 0.0;
      for (int s2 = 0; s2 < nsub; s2 += 64) {
        double sum2 = 0.0;
        for (int s1 = s2; s1 < nsub && s1 < s2 + 64; s1 += 8) {
          double sum1 = 0.0;
          for (int sb = s1; sb < nsub && sb < s1 + 8; ++sb) sum1 += part[(size_t)sb * W + q];
          sum2 += sum1;
        }
        sum += sum2;
      }
      rec[q] = sum;
    }
    if (tid < 2) {
      double sum = wsum[tid];
      for (int wv = 1; wv < XC_WAVES; ++wv) sum += wsum[2 * wv + tid];
      rec[nlag + tid] = sum;
    }
  }
}

// One wave per (segment, partition): lane q owns entries q, q + 64, ... of the record and adds the partition's chunks in
// ascending order (coalesced reads, no cross-lane step).  A partition without samples gives zeros.  Not ira::fold_records:
// a lane owns entries, not chunks, and the chunk range comes from the partition's limits.  Like ira::fold_records it never
// reads past its records: the range stops at the rec_stride - nlim chunks pass 1 was launched over, so a segment longer than
// the max_len the caller stated comes out cut at that many chunks instead of reading its neighbour's records, and an onset
// past the end of the file (L < 0) gives the empty segment it gives in pass 1, not a chunk range that starts below zero.
__global__ __launch_bounds__(IRA_WAVE) void xcorr_fold_kernel(
    const int64_t* __restrict__ len, const int32_t* __restrict__ lchan, const int32_t* __restrict__ rchan,
    const int64_t* __restrict__ onset, const int64_t* __restrict__ limits, int nlim, int T, int64_t rec_stride,
    const double* __restrict__ scratch, double* __restrict__ out) {
  const int seg = blockIdx.x, j = blockIdx.y;
  const int64_t ol = onset[lchan[seg]], orr = onset[rchan[seg]];
  const int64_t o = ol < orr ? ol : orr;
  const int64_t L = o < 0 || o > len[seg] ? 0 : len[seg] - o;
  int64_t a = j == 0 ? 0 : limits[(int64_t)seg * nlim + j - 1];
  int64_t b = j == nlim ? L : limits[(int64_t)seg * nlim + j];
  a = a < 0 ? 0 : (a < L ? a : L);
  b = b < a ? a : (b < L ? b : L);
  const int nrec = 2 * T + 3;
  const double* rec = scratch + (int64_t)seg * rec_stride * nrec;
  double* dst = out + ((int64_t)seg * (nlim + 1) + j) * nrec;
  const int64_t chunks = rec_stride - nlim;
  const int64_t c_lo = a / XC_CHUNK, c_last = a < b ? (b - 1) / XC_CHUNK : -1;
  const int64_t c_hi = c_last < chunks ? c_last : chunks - 1;
  for (int q = threadIdx.x; q < nrec; q += IRA_WAVE) {
    double v = 0.0;
    for (int64_t c = c_lo; c <= c_hi; ++c) v += rec[(c + j) * nrec + q];
    dst[q] = v;
  }
}

}  // namespace

extern "C" int64_t ira_xcorr_scratch_doubles(int32_t nseg, int64_t max_len, int32_t nlim, int32_t max_lag) {
  if (nseg < 0 || !xc_shape_ok(nseg, max_len) || nlim < 1 || nlim > XC_MAX_LIMITS || max_lag < 1 ||
      max_lag > IRA_XCORR_MAX_LAG)
    return IRA_E_SIZE;
  return (int64_t)nseg * (ira::ceil_div(max_len, XC_CHUNK) + nlim) * (2 * max_lag + 3);
}

extern "C" int32_t ira_xcorr_windows(const float* x_dev, const int64_t* l_off_dev, const int64_t* r_off_dev,
                                     const int64_t* len_dev, const int32_t* lchan_of_seg_dev,
                                     const int32_t* rchan_of_seg_dev, const int64_t* onset_dev, int32_t nseg,
                                     int64_t max_len, const int64_t* limits_dev, int32_t nlim, int32_t max_lag,
                                     double* scratch_dev, double* out_dev, void* stream) {
  IRA_CHECK_PTR(x_dev); IRA_CHECK_PTR(l_off_dev); IRA_CHECK_PTR(r_off_dev); IRA_CHECK_PTR(len_dev);
  IRA_CHECK_PTR(lchan_of_seg_dev); IRA_CHECK_PTR(rchan_of_seg_dev); IRA_CHECK_PTR(onset_dev); IRA_CHECK_PTR(limits_dev);
  IRA_CHECK_PTR(scratch_dev); IRA_CHECK_PTR(out_dev);
  if (nlim < 1 || nlim > XC_MAX_LIMITS) return IRA_E_SIZE;
  if (max_lag < 1 || max_lag > IRA_XCORR_MAX_LAG) return IRA_E_SIZE;
  if (nseg <= 0) return nseg == 0 ? IRA_OK : IRA_E_SIZE;
  if (!xc_shape_ok(nseg, max_len)) return IRA_E_SIZE;
  hipStream_t st = (hipStream_t)stream;
  const int64_t chunks = ira::ceil_div(max_len, XC_CHUNK);
  const int64_t rec_stride = chunks + nlim;
  const int nlag = 2 * max_lag + 1;
  const int lpt = xc_lags_per_thread(nlag);
  const int w = (nlag + lpt - 1) / lpt * lpt;
  const size_t lds = sizeof(double) * xc_lds_doubles(w);
  if (chunks > 0) {
    auto launch = [&](auto kernel) -> hipError_t {
      const hipError_t e = allow_lds(kernel, lds);
      if (e != hipSuccess) return e;
      kernel<<<dim3((unsigned)chunks, nseg), XC_THREADS, lds, st>>>(x_dev, l_off_dev, r_off_dev, len_dev, lchan_of_seg_dev,
                                                                  rchan_of_seg_dev, onset_dev, limits_dev, nlim, max_lag,
                                                                  rec_stride, scratch_dev);
      return hipSuccess;
    };
    switch (lpt) {
      case 13: IRA_TRY_HIP(launch(&xcorr_partial_kernel<13>)); break;
      case 11: IRA_TRY_HIP(launch(&xcorr_partial_kernel<11>)); break;
      default: IRA_TRY_HIP(launch(&xcorr_partial_kernel<9>)); break;
    }
  }
  xcorr_fold_kernel<<<dim3(nseg, nlim + 1), IRA_WAVE, 0, st>>>(len_dev, lchan_of_seg_dev, rchan_of_seg_dev, onset_dev,
                                                             limits_dev, nlim, max_lag, rec_stride, scratch_dev, out_dev);
  IRA_RETURN_LAUNCH();
}
