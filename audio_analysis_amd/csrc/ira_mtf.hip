// Modulation transfer sums for the speech transmission index (IEC 60268-16, Schroeder's indirect method): per row the
// float64 energy E = sum e[n] and, per modulation frequency, A = sum e[n] cos(2 pi frac(w n)), B = sum e[n] sin(2 pi frac(w n)),
// e = float64(x)^2.  Nothing in the reference computes these; the host side is audio_analysis_amd/analyse/sti.py.
// Contraction stays on: nothing here is compared bit for bit with NumPy, only with itself.
#include "ira_common.h"
#include "ira_reduce.h"

namespace {

// ------------------------------------------------------------------------------------------------
//   mtf_partial_kernel (chunks x rows)  one MT_CHUNK-sample chunk per workgroup -> one record of 2 nf + 1 doubles
//   mtf_fold_kernel    (1 wave / row)   the records folded in a fixed order -> out
// Thread tid of a chunk that starts at sample c0 holds quads u < MT_QUADS: samples n = c0 + 4 tid + 1024 u + r, r < 4 (the
// layout of ira_energy.hip: ira::load_quads, so the order of the sums never changes with the address).
// The phasor of sample n is the product of three unit phasors, each evaluated directly from a phase reduced to a fraction
// of a turn (mt_cis), never by a recurrence:
//   cis(w n) = base(c0 + 4 tid) * stride(1024 u) * quad(r)
// base is one sincospi per thread, frequency and chunk; stride and quad are 20 phasors per frequency that the workgroup
// puts in LDS once.  The sums are linear in the phasors, so a thread forms S_r = sum_u e[u][r] stride(u) (two FMAs per
// sample and frequency) and multiplies by quad(r) and base once per frequency:
//   A + iB = base * sum_r quad(r) * S_r.
// The squares stay in registers as float64 (128 VGPRs): squaring float32 samples again for each of the 14 frequencies
// would double the float64 instructions per sample.  The frequency loop is not unrolled: eight accumulators are live.
// Every chunk boundary, every thread's share and every reduction tree is a function of the row's own length only: a
// row's result does not depend on the batch, its place in it or the alignment of its first sample.  No atomics.
// ------------------------------------------------------------------------------------------------
constexpr int MT_THREADS = 256;
constexpr int MT_QUADS = 16;                                  // 16-byte loads per thread per chunk, all in flight together
constexpr int MT_CHUNK = MT_THREADS * 4 * MT_QUADS;           // 16384 samples
constexpr int MT_WAVES = MT_THREADS / IRA_WAVE;
constexpr int MT_TAB = MT_QUADS + 4;                          // per frequency: stride(0 .. 15), quad(0 .. 3)
constexpr int MT_MAX_REC = 2 * IRA_MTF_MAX_FREQS + 1;         // E, A_0, B_0, ...
constexpr int64_t MT_MAX_LEN = (int64_t)1 << 31;
static_assert(MT_CHUNK == IRA_MTF_CHUNK, "include/ira.h states the chunk size");

// cis(2 pi frac(w n)), n an integer below 2^32 held exactly in float64.  p + lo is w n exactly (the FMA recovers what the
// product rounded away); the whole turns leave p before anything is evaluated, so the phase error is that of one rounding
// of a number below 1, whatever n.
__device__ __forceinline__ void mt_cis(double w, double n, double& c, double& s) {
  const double p = w * n;
  const double lo = __builtin_fma(w, n, -p);
  const double f = (p - rint(p)) + lo;
  sincospi(2.0 * f, &s, &c);
}

__global__ __launch_bounds__(MT_THREADS) void mtf_partial_kernel(const float* __restrict__ x,
                                                                 const int64_t* __restrict__ off,
                                                                 const int64_t* __restrict__ len,
                                                                 const double* __restrict__ w, int nf,
                                                                 int64_t chunk_stride, double* __restrict__ scratch) {
  __shared__ double tab_c[IRA_MTF_MAX_FREQS][MT_TAB], tab_s[IRA_MTF_MAX_FREQS][MT_TAB];
  __shared__ double wsum[MT_WAVES][MT_MAX_REC];
  const int seg = blockIdx.y;
  const int64_t n = ira::uniform(len[seg]);
  const int64_t c0 = (int64_t)blockIdx.x * MT_CHUNK;
  if (c0 >= n) return;                                        // the fold reads only the chunks of the row's length
  const int cnt = (int)(n - c0 < MT_CHUNK ? n - c0 : MT_CHUNK);
  const float* q = x + ira::uniform(off[seg]) + c0;
  const double* ws = w + (int64_t)seg * nf;
  const int tid = threadIdx.x;

  for (int k = tid; k < nf * MT_TAB; k += MT_THREADS) {
    const int i = k / MT_TAB, j = k % MT_TAB;
    const double step = j < MT_QUADS ? (double)(4 * MT_THREADS * j) : (double)(j - MT_QUADS);
    double c, s;
    mt_cis(ws[i], step, c, s);
    tab_c[i][j] = c;
    tab_s[i][j] = s;
  }

  double e[MT_QUADS][4];
  {
    ira::f4u a[MT_QUADS];
    ira::load_quads<MT_THREADS, MT_QUADS, false>(q, cnt, a);
#pragma unroll
    for (int u = 0; u < MT_QUADS; ++u) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double d = (double)a[u][r];
        e[u][r] = d * d;
      }
    }
  }
  const int lane = tid & 63, wave = tid >> 6;
  {
    double tot = 0.0;
#pragma unroll
    for (int u = 0; u < MT_QUADS; ++u) tot += (e[u][0] + e[u][1]) + (e[u][2] + e[u][3]);
    tot = ira::wave_sum(tot);
    if (lane == 0) wsum[wave][0] = tot;
  }
  __syncthreads();                                            // the tables

  const double nbase = (double)(c0 + 4 * tid);
#pragma unroll 1
  for (int i = 0; i < nf; ++i) {
    double bc, bs;
    mt_cis(ira::uniform(ws[i]), nbase, bc, bs);
    double sc[4] = {0.0, 0.0, 0.0, 0.0}, ss[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int u = 0; u < MT_QUADS; ++u) {
      const double tc = tab_c[i][u], ts = tab_s[i][u];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        sc[r] = __builtin_fma(e[u][r], tc, sc[r]);
        ss[r] = __builtin_fma(e[u][r], ts, ss[r]);
      }
    }
    double tc = sc[0], ts = ss[0];                            // quad(0) = 1
#pragma unroll
    for (int r = 1; r < 4; ++r) {
      const double qc = tab_c[i][MT_QUADS + r], qs = tab_s[i][MT_QUADS + r];
      tc += qc * sc[r] - qs * ss[r];
      ts += qc * ss[r] + qs * sc[r];
    }
    const double a = ira::wave_sum(bc * tc - bs * ts);
    const double b = ira::wave_sum(bc * ts + bs * tc);
    if (lane == 0) {
      wsum[wave][1 + 2 * i] = a;
      wsum[wave][2 + 2 * i] = b;
    }
  }
  __syncthreads();
  const int nrec = 2 * nf + 1;
  if (tid < nrec) {
    double v = wsum[0][tid];
    for (int k = 1; k < MT_WAVES; ++k) v += wsum[k][tid];
    scratch[((int64_t)seg * chunk_stride + blockIdx.x) * nrec + tid] = v;
  }
}

// One wave per row: ira::fold_records over the row's records.
__global__ __launch_bounds__(IRA_WAVE) void mtf_fold_kernel(const int64_t* __restrict__ len, int nseg, int nf,
                                                            int64_t chunk_stride, const double* __restrict__ scratch,
                                                            double* __restrict__ out) {
  const int seg = blockIdx.x;
  if (seg >= nseg) return;
  ira::fold_records(scratch, seg, len[seg], MT_CHUNK, chunk_stride, 2 * nf + 1, out);
}

inline bool mt_shape_ok(int32_t nseg, int64_t max_len) { return nseg <= 65535 && max_len >= 0 && max_len <= MT_MAX_LEN; }

}  // namespace

extern "C" int64_t ira_mtf_scratch_doubles(int32_t nseg, int64_t max_len, int32_t nf) {
  if (nseg < 0 || !mt_shape_ok(nseg, max_len) || nf < 1 || nf > IRA_MTF_MAX_FREQS) return IRA_E_SIZE;
  return (int64_t)nseg * ira::ceil_div(max_len, MT_CHUNK) * (2 * nf + 1);
}

extern "C" int32_t ira_mtf_sums(const float* x_dev, const int64_t* off_dev, const int64_t* len_dev, const double* w_dev,
                                int32_t nseg, int64_t max_len, int32_t nf, double* scratch_dev, double* out_dev,
                                void* stream) {
  IRA_CHECK_PTR(x_dev); IRA_CHECK_PTR(off_dev); IRA_CHECK_PTR(len_dev); IRA_CHECK_PTR(w_dev);
  IRA_CHECK_PTR(scratch_dev); IRA_CHECK_PTR(out_dev);
  if (nf < 1 || nf > IRA_MTF_MAX_FREQS) return IRA_E_SIZE;
  if (nseg <= 0) return nseg == 0 ? IRA_OK : IRA_E_SIZE;
  if (!mt_shape_ok(nseg, max_len)) return IRA_E_SIZE;
  hipStream_t st = (hipStream_t)stream;
  const int64_t chunks = ira::ceil_div(max_len, MT_CHUNK);
  if (chunks > 0)
    mtf_partial_kernel<<<dim3((unsigned)chunks, nseg), MT_THREADS, 0, st>>>(x_dev, off_dev, len_dev, w_dev, nf, chunks,
                                                                           scratch_dev);
  mtf_fold_kernel<<<nseg, IRA_WAVE, 0, st>>>(len_dev, nseg, nf, chunks, scratch_dev, out_dev);
  IRA_RETURN_LAUNCH();
}
