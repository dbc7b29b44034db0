// Harmonic distortion from a deconvolved logarithmic sweep: the windowed segments in front of the linear peak that hold
// the harmonic impulses (ira_harmonic_windows) and the mean band powers of their spectra (ira_harmonic_band_powers).
// Nothing in the reference computes these; the host side, with the definitions, is audio_analysis_amd/analyse/harmonics.py.
// Contraction is off (build.py): a segment sample is one float64 product rounded once to float32, like NumPy's.
#include "ira_common.h"
#include "ira_reduce.h"

namespace {

constexpr int HW_THREADS = 256;
constexpr int HW_PER_THREAD = 4;                              // one 16-byte access per thread
constexpr int HW_TILE = HW_THREADS * HW_PER_THREAD;           // 1024 samples of a row per workgroup
constexpr int HARM_MAX_SEG = 1 << 21;                         // the longest response the deconvolution makes
constexpr int HARM_MAX_BANDS = 4096;
constexpr int HARM_MAX_BINS = (1 << 20) + 1;

// ------------------------------------------------------------------------------------------------
// harm_windows_kernel (tiles x rows): row r = c * nharm + k of out is
//   out[r * seg + i] = float32(float64(h_c[(p_c - d_k - guard + i) mod n_c]) * w[i]),  i < seg.
// A circular gather and a multiply, bound by memory.  Thread t of a tile holds samples 4 t .. 4 t + 3, so a wave reads 1 KiB
// of h and stores 1 KiB of the row in one piece; the wrap point of the circular buffer splits a row into at most two such
// runs, and only the one quad that straddles it (and the last quad of a row whose seg is no multiple of 4) goes sample by
// sample.  The start index is reduced once per workgroup (uniform), a thread only subtracts n.  Whatever the tables hold, an
// index is reduced into [0, n) before it is used, and a row of a channel without samples is written as zeros.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HW_THREADS) void harm_windows_kernel(const float* __restrict__ h,
                                                                  const int64_t* __restrict__ h_off,
                                                                  const int32_t* __restrict__ nfft,
                                                                  const int64_t* __restrict__ peak,
                                                                  const int64_t* __restrict__ lag,
                                                                  const double* __restrict__ win, int nharm, int guard,
                                                                  int seg, float* __restrict__ out) {
  const int row = blockIdx.y;
  const int c = row / nharm, k = row - c * nharm;
  const int64_t n = ira::uniform((int64_t)nfft[c]);
  const int i0 = blockIdx.x * HW_TILE + HW_PER_THREAD * threadIdx.x;
  if (i0 >= seg) return;
  float* dst = out + (int64_t)row * seg + i0;
  const int left = seg - i0;
  if (n <= 0) {
    for (int r = 0; r < HW_PER_THREAD && r < left; ++r) dst[r] = 0.0f;
    return;
  }
  int64_t start = (ira::uniform(peak[c]) - ira::uniform(lag[k]) - (int64_t)guard) % n;      // uniform: once per workgroup
  if (start < 0) start += n;
  const float* src = h + ira::uniform(h_off[c]);
  int64_t j = start + i0;
  if (j >= n) {
    j -= n;
    if (j >= n) j %= n;                                       // a row longer than its channel's buffer
  }
  if (left >= HW_PER_THREAD && j + HW_PER_THREAD <= n) {
    const ira::f4u a = *reinterpret_cast<const ira::f4u*>(src + j);
    const ira::d2u w0 = *reinterpret_cast<const ira::d2u*>(win + i0);
    const ira::d2u w1 = *reinterpret_cast<const ira::d2u*>(win + i0 + 2);
    ira::f4u v;
    v.x = (float)((double)a.x * w0.x);
    v.y = (float)((double)a.y * w0.y);
    v.z = (float)((double)a.z * w1.x);
    v.w = (float)((double)a.w * w1.y);
    *reinterpret_cast<ira::f4u*>(dst) = v;
  } else {
    for (int r = 0; r < HW_PER_THREAD && r < left; ++r) {
      dst[r] = (float)((double)src[j] * win[i0 + r]);
      if (++j >= n) j = 0;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// harm_band_powers_kernel (bands / 4 x rows): one wave per (row, band).  Lane l adds re^2 + im^2 of the bins lo + l + 64 m
// in ascending m, four independent accumulators (m mod 4) combined as (a0 + a1) + (a2 + a3), then the butterfly of
// wave_sum, then one division by the count.  The order is a function of the band's own lo and cnt: a row's result does not
// depend on the batch or on the row's place in it (the rule ira_mtf.hip states).  No atomics.  A lane's bin is a 16-byte
// complex value, so a wave reads 1 KiB in one piece per step.
// ------------------------------------------------------------------------------------------------
constexpr int BP_WAVES = 4;
constexpr int BP_THREADS = BP_WAVES * IRA_WAVE;

__global__ __launch_bounds__(BP_THREADS) void harm_band_powers_kernel(const double* __restrict__ spec,
                                                                      const int64_t* __restrict__ spec_off,
                                                                      const int32_t* __restrict__ lo_tab,
                                                                      const int32_t* __restrict__ cnt_tab, int nharm,
                                                                      int nband, int nbins, double* __restrict__ out) {
  const int row = blockIdx.y;
  const int band = blockIdx.x * BP_WAVES + (threadIdx.x >> 6);
  if (band >= nband) return;                                  // whole waves leave: no barrier follows
  const int lane = threadIdx.x & 63;
  const int k = row % nharm;
  const int lo = ira::uniform(lo_tab[k * nband + band]);
  const int cnt = ira::uniform(cnt_tab[k * nband + band]);
  double* dst = out + (int64_t)row * nband + band;
  if (cnt <= 0) {
    if (lane == 0) *dst = 0.0;
    return;
  }
  if (lo < 0 || (int64_t)lo + cnt > nbins) {                  // a table that leaves the spectrum: never read, and visibly wrong
    if (lane == 0) *dst = __builtin_nan("");
    return;
  }
  const ira::d2u* z = reinterpret_cast<const ira::d2u*>(spec) + ira::uniform(spec_off[row]) + lo;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int b = lane;
  for (; b + 3 * IRA_WAVE < cnt; b += 4 * IRA_WAVE) {
    const ira::d2u v0 = z[b], v1 = z[b + IRA_WAVE], v2 = z[b + 2 * IRA_WAVE], v3 = z[b + 3 * IRA_WAVE];
    a0 += v0.x * v0.x + v0.y * v0.y;
    a1 += v1.x * v1.x + v1.y * v1.y;
    a2 += v2.x * v2.x + v2.y * v2.y;
    a3 += v3.x * v3.x + v3.y * v3.y;
  }
  if (b < cnt) { const ira::d2u v = z[b]; a0 += v.x * v.x + v.y * v.y; b += IRA_WAVE; }
  if (b < cnt) { const ira::d2u v = z[b]; a1 += v.x * v.x + v.y * v.y; b += IRA_WAVE; }
  if (b < cnt) { const ira::d2u v = z[b]; a2 += v.x * v.x + v.y * v.y; }
  const double s = ira::wave_sum((a0 + a1) + (a2 + a3));
  if (lane == 0) *dst = s / (double)cnt;
}

}  // namespace

extern "C" int32_t ira_harmonic_windows(const float* h_dev, const int64_t* h_off_dev, const int32_t* nfft_dev,
                                        const int64_t* peak_dev, const int64_t* lag_dev, const double* window_dev,
                                        int32_t nch, int32_t nharm, int32_t guard, int32_t seg, float* out_dev,
                                        void* stream) {
  IRA_CHECK_PTR(h_dev); IRA_CHECK_PTR(h_off_dev); IRA_CHECK_PTR(nfft_dev); IRA_CHECK_PTR(peak_dev);
  IRA_CHECK_PTR(lag_dev); IRA_CHECK_PTR(window_dev); IRA_CHECK_PTR(out_dev);
  if (nharm < 1 || nharm > IRA_HARMONIC_MAX) return IRA_E_SIZE;
  if (guard < 1 || seg <= guard || seg > HARM_MAX_SEG) return IRA_E_SIZE;
  if (nch <= 0) return nch == 0 ? IRA_OK : IRA_E_SIZE;
  if ((int64_t)nch * nharm > 65535) return IRA_E_SIZE;
  const unsigned tiles = (unsigned)((seg + HW_TILE - 1) / HW_TILE);
  harm_windows_kernel<<<dim3(tiles, (unsigned)(nch * nharm)), HW_THREADS, 0, (hipStream_t)stream>>>(
      h_dev, h_off_dev, nfft_dev, peak_dev, lag_dev, window_dev, nharm, guard, seg, out_dev);
  IRA_RETURN_LAUNCH();
}

extern "C" int32_t ira_harmonic_band_powers(const double* spec_dev, const int64_t* spec_off_dev, const int32_t* lo_dev,
                                            const int32_t* cnt_dev, int32_t nrow, int32_t nharm, int32_t nband,
                                            int32_t nbins, double* out_dev, void* stream) {
  IRA_CHECK_PTR(spec_dev); IRA_CHECK_PTR(spec_off_dev); IRA_CHECK_PTR(lo_dev); IRA_CHECK_PTR(cnt_dev);
  IRA_CHECK_PTR(out_dev);
  if (nharm < 1 || nharm > IRA_HARMONIC_MAX) return IRA_E_SIZE;
  if (nband < 1 || nband > HARM_MAX_BANDS || nbins < 1 || nbins > HARM_MAX_BINS) return IRA_E_SIZE;
  if (nrow <= 0) return nrow == 0 ? IRA_OK : IRA_E_SIZE;
  if (nrow > 65535 || nrow % nharm != 0) return IRA_E_SIZE;
  harm_band_powers_kernel<<<dim3((unsigned)((nband + BP_WAVES - 1) / BP_WAVES), (unsigned)nrow), BP_THREADS, 0,
                            (hipStream_t)stream>>>(spec_dev, spec_off_dev, lo_dev, cnt_dev, nharm, nband, nbins, out_dev);
  IRA_RETURN_LAUNCH();
}
