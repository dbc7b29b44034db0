// Dual-channel spectral sums (Welch): auto- and cross-spectra of a (reference, measurement) pair averaged over
// overlapping frames, and the H1 / H2 transfer-function estimates, coherence, level and phase formed from them.  Nothing
// in the reference computes them; the host side is audio_analysis_amd/analyse/transfer.py, which states the definitions.
//
// Pair p: reference samples x' = x + x_off[p], measurement y' = x + y_off[p] (the pair's delay is already in the two
// offsets), n[p] samples of each, K = 1 + (n[p] - n_fft) / hop frames (0 when n[p] < n_fft), frame f at f * hop.
//   xspec_accumulate_kernel (chunks x pairs)  a workgroup walks the XS_FRAMES frames of its chunk.  Per frame:
//       z[i] = w[i] x'[i] + i w[i] y'[i] as float64 in LDS  ->  ONE n_fft-point complex lds_fft_dif (both channels ride it)
//       ->  its bit-reversed output read in place: X[k] = (Z[k] + conj(Z[n-k])) / 2, Y[k] = (Z[k] - conj(Z[n-k])) / 2i
//       ->  |X|^2, |Y|^2, Re / Im conj(X) Y added to the thread's own registers.  (A channel whose windowed frame is all
//       zeros contributes the spectrum 0 exactly.)
//     A thread owns POSITIONS of the transform's output, not bins: position a holds bin brev(a), and the position of bin
//     n - k is a ^ (2^floor(log2 a) - 1) (the bits below a's highest set bit, complemented; 0 and 1 -- bins 0 and n/2 --
//     are their own partners).  Bins 0 .. n/2 - 1 are the even positions, so consecutive lanes read consecutive even
//     positions and their partners descend consecutively: the natural-bin order (buf[brev(k)] for consecutive k) would
//     put every lane of a wave on one bank.  At the end of the chunk the sums pass through LDS once to leave in bin
//     order: partial[pair][chunk][4][nbins], plain stores, no atomics.
//   xspec_finish_kernel (one thread per pair and bin)  adds the chunks in ascending order and forms the derived values.
// The frames of a chunk, the chunk boundaries and each thread's share are functions of n_fft and hop alone, and a
// workgroup reads and writes nothing of another pair: a pair's sums are the same bytes whatever else is in the batch.
// A chunk wholly past a pair's K returns before it touches memory, and the finish pass reads only the chunks below
// ceil(K / XS_FRAMES); the last frame ends at (K - 1) hop + n_fft <= n[p], so nothing past a row's n[p] samples is read.
#include <math.h>

#include "ira_fft_lds.h"

namespace {

using ira::cplx;

constexpr int XS_THREADS = 256;
constexpr int XS_FRAMES = IRA_XSPEC_FRAMES;
constexpr int XS_MIN_FFT = 256, XS_MAX_FFT = 8192;

__device__ __forceinline__ int64_t xs_frames(int64_t len, int n, int hop) {
  return len >= n ? 1 + (len - n) / hop : 0;
}

// NB: positions per thread, n_fft / 512 + 1 (the + 1: position 1, the Nyquist bin, is slot n_fft / 2)
template <int NB>
__global__ __launch_bounds__(XS_THREADS) void xspec_accumulate_kernel(
    const float* __restrict__ x, const int64_t* __restrict__ x_off, const int64_t* __restrict__ y_off,
    const int64_t* __restrict__ n_of, int log2n, int hop, const double* __restrict__ window,
    const cplx<double>* __restrict__ tw, double* __restrict__ partial, int chunks) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  cplx<double>* buf = reinterpret_cast<cplx<double>*>(smem_raw);
  const int pair = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
  const int n = 1 << log2n, half = n >> 1, nbins = half + 1;
  const int64_t nframes = xs_frames(ira::uniform(n_of[pair]), n, hop);
  const int64_t f0 = (int64_t)chunk * XS_FRAMES;
  if (f0 >= nframes) return;
  const int64_t f1 = f0 + XS_FRAMES < nframes ? f0 + XS_FRAMES : nframes;
  const float* xs = x + ira::uniform(x_off[pair]);
  const float* ys = x + ira::uniform(y_off[pair]);

  double sxx[NB], syy[NB], sre[NB], sim[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) sxx[j] = syy[j] = sre[j] = sim[j] = 0.0;

  for (int64_t f = f0; f < f1; ++f) {
    const float* fx = xs + f * hop;
    const float* fy = ys + f * hop;
    int nzx = 0, nzy = 0;
    for (int i = tid; i < n; i += XS_THREADS) {
      const double w = window[i];
      const double a = (double)fx[i] * w, b = (double)fy[i] * w;
      nzx |= a != 0.0;                                                   // a NaN counts
      nzy |= b != 0.0;
      buf[i] = {a, b};
    }
    // A channel whose windowed frame is all zeros has the spectrum 0, exactly: unpacked from the joint transform it would
    // carry the other channel's rounding error instead (a muted reference must give Sxx = 0, not 1e-30 of Syy).
    const bool live_x = __syncthreads_or(nzx) != 0;
    const bool live_y = __syncthreads_or(nzy) != 0;
    ira::lds_fft_dif<double>(buf, log2n, tw, 1u, tid, XS_THREADS);      // ends with a barrier
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int m = tid + XS_THREADS * j;
      if (m <= half) {
        const unsigned a = m < half ? 2u * (unsigned)m : 1u;
        const unsigned p = a < 2u ? a : a ^ ((1u << (31 - __clz((int)a))) - 1u);
        const cplx<double> zk = buf[a], zp = buf[p];
        const double xr = live_x ? 0.5 * (zk.re + zp.re) : 0.0, xi = live_x ? 0.5 * (zk.im - zp.im) : 0.0;
        const double yr = live_y ? 0.5 * (zk.im + zp.im) : 0.0, yi = live_y ? -0.5 * (zk.re - zp.re) : 0.0;
        sxx[j] += xr * xr + xi * xi;
        syy[j] += yr * yr + yi * yi;
        sre[j] += xr * yr + xi * yi;                                     // conj(X) Y
        sim[j] += xr * yi - xi * yr;
      }
    }
    __syncthreads();                                                     // the next frame overwrites buf
  }

  // the four sums, one after the other, through LDS into bin order
  double* stage = reinterpret_cast<double*>(smem_raw);
  double* dst = partial + ((int64_t)pair * chunks + chunk) * 4 * nbins;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int m = tid + XS_THREADS * j;
      if (m <= half) {
        const unsigned k = m < half ? ira::lds_brev(2u * (unsigned)m, log2n) : (unsigned)half;
        stage[k] = s == 0 ? sxx[j] : (s == 1 ? syy[j] : (s == 2 ? sre[j] : sim[j]));
      }
    }
    __syncthreads();
    for (int k = tid; k < nbins; k += XS_THREADS) dst[(int64_t)s * nbins + k] = stage[k];
    __syncthreads();
  }
}

__global__ __launch_bounds__(XS_THREADS) void xspec_finish_kernel(const double* __restrict__ partial,
                                                                  const int64_t* __restrict__ n_of, int n_fft, int hop,
                                                                  int chunks, double* __restrict__ out) {
  // one operation, one rounding: the host restatement of these quotients is held to a few ulp
#pragma clang fp contract(off)
  const int pair = blockIdx.y, nbins = n_fft / 2 + 1;
  const int k = blockIdx.x * XS_THREADS + threadIdx.x;
  if (k >= nbins) return;
  const int64_t nframes = xs_frames(n_of[pair], n_fft, hop);
  int64_t nch = (nframes + XS_FRAMES - 1) / XS_FRAMES;
  nch = nch < chunks ? nch : chunks;
  const double* p = partial + (int64_t)pair * chunks * 4 * nbins + k;
  double sxx = 0.0, syy = 0.0, sre = 0.0, sim = 0.0;
  for (int64_t c = 0; c < nch; ++c) {
    sxx += p[0];
    syy += p[nbins];
    sre += p[2 * (int64_t)nbins];
    sim += p[3 * (int64_t)nbins];
    p += 4 * (int64_t)nbins;
  }
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  const double h1r = sxx == 0.0 ? qnan : sre / sxx, h1i = sxx == 0.0 ? qnan : sim / sxx;
  const double m2 = sre * sre + sim * sim;                               // |Sxy|^2
  const double h2r = m2 == 0.0 ? qnan : syy * sre / m2, h2i = m2 == 0.0 ? qnan : syy * sim / m2;   // Syy / conj(Sxy)
  const double den = sxx * syy;
  const double q = den == 0.0 ? qnan : m2 / den;
  double* o = out + (int64_t)pair * IRA_XSPEC_ROWS * nbins + k;
  o[0] = sxx;
  o[nbins] = syy;
  o[2 * (int64_t)nbins] = sre;
  o[3 * (int64_t)nbins] = sim;
  o[4 * (int64_t)nbins] = h1r;
  o[5 * (int64_t)nbins] = h1i;
  o[6 * (int64_t)nbins] = h2r;
  o[7 * (int64_t)nbins] = h2i;
  o[8 * (int64_t)nbins] = q > 1.0 ? 1.0 : q;                             // a NaN stays
  o[9 * (int64_t)nbins] = 10.0 * log10(h1r * h1r + h1i * h1i);           // 20 log10 |H1|
  o[10 * (int64_t)nbins] = atan2(sim, sre);
}

inline int32_t xs_check(int32_t npairs, int32_t max_frames, int32_t n_fft, int32_t hop) {
  if (n_fft < XS_MIN_FFT || n_fft > XS_MAX_FFT || (n_fft & (n_fft - 1)) != 0) return IRA_E_SIZE;
  if (hop < 1 || hop > n_fft) return IRA_E_SIZE;
  if (npairs < 0 || npairs > 65535 || max_frames < 0) return IRA_E_SIZE;
  return IRA_OK;
}

inline int xs_chunks(int32_t max_frames) { return (int)(((int64_t)max_frames + XS_FRAMES - 1) / XS_FRAMES); }

template <int NB>
int32_t xs_launch(const float* x, const int64_t* x_off, const int64_t* y_off, const int64_t* n_of, int32_t npairs,
                  int chunks, int log2n, int32_t hop, const double* window, const double* tw, double* partial,
                  hipStream_t st) {
  const size_t lds = sizeof(cplx<double>) << log2n;                      // 128 KiB at 8192 points: one workgroup per CU
  IRA_TRY_HIP(allow_lds(xspec_accumulate_kernel<NB>, lds));
  xspec_accumulate_kernel<NB><<<dim3((unsigned)chunks, (unsigned)npairs), XS_THREADS, lds, st>>>(
      x, x_off, y_off, n_of, log2n, hop, window, reinterpret_cast<const cplx<double>*>(tw), partial, chunks);
  IRA_RETURN_LAUNCH();
}

}  // namespace

extern "C" int32_t ira_xspec_accumulate(const float* x_dev, const int64_t* x_off_dev, const int64_t* y_off_dev,
                                        const int64_t* n_dev, int32_t npairs, int32_t max_frames, int32_t n_fft,
                                        int32_t hop, const double* window_dev, const double* twiddle_dev,
                                        double* partial_dev, void* stream) {
  IRA_CHECK_PTR(x_dev); IRA_CHECK_PTR(x_off_dev); IRA_CHECK_PTR(y_off_dev); IRA_CHECK_PTR(n_dev);
  IRA_CHECK_PTR(window_dev); IRA_CHECK_PTR(twiddle_dev); IRA_CHECK_PTR(partial_dev);
  const int32_t rc = xs_check(npairs, max_frames, n_fft, hop);
  if (rc != IRA_OK) return rc;
  if (npairs == 0 || max_frames == 0) return IRA_OK;
  int log2n = 0;
  while ((1 << log2n) < n_fft) ++log2n;
  hipStream_t st = (hipStream_t)stream;
  const int chunks = xs_chunks(max_frames);
  if (n_fft <= 2048)
    return xs_launch<2048 / 512 + 1>(x_dev, x_off_dev, y_off_dev, n_dev, npairs, chunks, log2n, hop, window_dev,
                                     twiddle_dev, partial_dev, st);
  if (n_fft == 4096)
    return xs_launch<4096 / 512 + 1>(x_dev, x_off_dev, y_off_dev, n_dev, npairs, chunks, log2n, hop, window_dev,
                                     twiddle_dev, partial_dev, st);
  return xs_launch<8192 / 512 + 1>(x_dev, x_off_dev, y_off_dev, n_dev, npairs, chunks, log2n, hop, window_dev,
                                   twiddle_dev, partial_dev, st);
}

extern "C" int32_t ira_xspec_finish(const double* partial_dev, const int64_t* n_dev, int32_t npairs, int32_t max_frames,
                                    int32_t n_fft, int32_t hop, double* out_dev, void* stream) {
  IRA_CHECK_PTR(partial_dev); IRA_CHECK_PTR(n_dev); IRA_CHECK_PTR(out_dev);
  const int32_t rc = xs_check(npairs, max_frames, n_fft, hop);
  if (rc != IRA_OK) return rc;
  if (npairs == 0) return IRA_OK;
  const int nbins = n_fft / 2 + 1;
  xspec_finish_kernel<<<dim3((unsigned)((nbins + XS_THREADS - 1) / XS_THREADS), (unsigned)npairs), XS_THREADS, 0,
                        (hipStream_t)stream>>>(partial_dev, n_dev, n_fft, hop, xs_chunks(max_frames), out_dev);
  IRA_RETURN_LAUNCH();
}
