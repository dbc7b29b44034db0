// Dietsch-Kraak echo criterion EK: running float64 centre time of |p|^n, lagged difference, maximum, first crossings
// and a decimated curve.  Nothing in the reference computes it; the host side is audio_analysis_amd/analyse/echo.py,
// which states the definition.  Compiled with -ffp-contract=off: the float64 products and sums round one operation at a
// time, like NumPy's.
//
// Segment j is one (channel, criterion) row: samples base_off[j] + o .. of x, o = onset[chan_of_seg[j]], m counted from
// o, L = base_len[j] - o, and a parameter set p = param_of_seg[j] (exponent n, D, G, Mmax, S, two thresholds, fs).
//   s[m] = |y[o + m]|^n,  W[m] = sum_{j<=m} s[j],  V[m] = sum_{j<=m} j s[j],  ts[m] = V[m] / (fs W[m]) (0 where W = 0)
//   EK[m] = (ts[m] - ts[m - D]) / (D / fs),  m < M = min(L - G, Mmax),  ts = 0 in front of the onset.
// The sums are causal, so nothing at or after M is read.  The scan of ira_edc.hip, run forwards, in chunks of EC_CHUNK
// samples counted from the ONSET:
//   echo_init_kernel                          crossing slots = none, curve keys = empty
//   echo_partial_kernel (chunks x segments)   chunk totals of s and m s (and, with a stash, s itself as float64)
//   echo_carry_kernel   (1 wave / segment)    exclusive scan of the chunk totals in ascending order
//   echo_emit_kernel    (chunks x segments)   scans the chunk in front of its own (the halo: ts[m - D] for the first D
//                                             samples, D <= EC_HALO) and its own with the SAME scan code, forms ts and
//                                             EK; the chunk's (max, first index at the max) record; first crossings by
//                                             atomicMin on the index; curve maxima by atomicMax on an ordered key
//   echo_fold_kernel    (1 wave / segment)    greatest chunk maximum, smallest index on a tie -> the 8-double record;
//                                             curve keys -> float32 (untouched keys -> NaN)
// Every chunk boundary, every thread's share of a chunk and every reduction tree is a function of the segment's own
// onset, length and parameters; the two atomics merge with min / max, which do not depend on arrival order; loads are
// ira::load_run (16 bytes at 4-byte alignment).  So a segment's record and curve are bit-identical whatever the batch, the
// segment's place in it or the alignment of its first sample.
#include <math.h>

#include "ira_common.h"
#include "ira_reduce.h"

namespace {

constexpr int EC_THREADS = 256;
constexpr int EC_PER_THREAD = 16;
constexpr int EC_CHUNK = EC_THREADS * EC_PER_THREAD;
constexpr int EC_WAVES = EC_THREADS / IRA_WAVE;
constexpr int EC_HALO = IRA_ECHO_MAX_LAG;                    // samples of ts kept from the chunk in front
constexpr int EC_HDR = 8;                                    // per segment: slot10, slot50, ts_end, W_end, V_end, 3 spare
constexpr int EC_PER_CHUNK = 6;                              // totW, totV, carryW, carryV, chunk max, its index
constexpr int64_t EC_MAX_LEN = (int64_t)1 << 31;
constexpr unsigned long long EC_NONE = ~0ull;
static_assert(EC_CHUNK == IRA_ECHO_CHUNK, "the host sizes the stash and its tests with this chunk");
static_assert(EC_HALO <= EC_CHUNK && EC_HALO % EC_PER_THREAD == 0, "the halo is a whole number of thread shares of one chunk");
static_assert(EC_HALO >= 1344, "14 ms at 96 kHz");

// ts in LDS: halo then the chunk, one double of padding per thread share (a share is 16 doubles = 128 bytes: without
// it every lane of a wave would hit the same two banks)
__device__ __forceinline__ int ts_slot(int i) { return i + (i >> 4); }
constexpr int EC_TS_SLOTS = (EC_HALO + EC_CHUNK) + ((EC_HALO + EC_CHUNK) >> 4);

struct EchoParamTable {
  double v[IRA_ECHO_MAX_PARAMS][IRA_ECHO_PARAM_DOUBLES];
};

struct EchoTables {
  const float* x;
  const int64_t* base_off;
  const int64_t* base_len;
  const int32_t* chan_of_seg;
  const int32_t* param_of_seg;
  const int64_t* onset;
  int nparam;
  int64_t chunk_stride;                                      // chunks of the longest segment: strides of the scratch
};

struct EchoShared {
  double wtot[2][2][EC_WAVES];                               // [parity][W | V][wave]
};

// The wave-uniform values of one segment.
struct EchoSeg {
  const float* q;                                            // sample m = 0
  int64_t m_raw, m;                                          // M as defined, and max(M, 0)
  int64_t step;                                              // S
  int lag;                                                   // D
  int mode;                                                  // 0 fabs, 1 product, 2 sqrt, 3 pow
  double n, thr10, thr50, fs;
};

__device__ __forceinline__ EchoSeg echo_seg(const EchoTables& T, const EchoParamTable& P, int seg) {
  EchoSeg g;
  int p = ira::uniform(T.param_of_seg[seg]);
  p = p < 0 ? 0 : (p >= T.nparam ? T.nparam - 1 : p);
  int64_t o = ira::uniform(T.onset[ira::uniform(T.chan_of_seg[seg])]);
  o = o > 0 ? o : 0;
  const int64_t len = ira::uniform(T.base_len[seg]) - o;
  g.n = P.v[p][0];
  g.lag = (int)P.v[p][1];
  const int64_t guard = (int64_t)P.v[p][2], mmax = (int64_t)P.v[p][3];
  g.step = (int64_t)P.v[p][4];
  g.thr10 = P.v[p][5];
  g.thr50 = P.v[p][6];
  g.fs = P.v[p][7];
  g.m_raw = len - guard < mmax ? len - guard : mmax;
  g.m = g.m_raw > 0 ? g.m_raw : 0;
  const int64_t room = T.chunk_stride * EC_CHUNK;           // max_len >= M is the caller's; never leave the scratch
  g.m = g.m < room ? g.m : room;
  g.mode = g.n == 1.0 ? 0 : (g.n == 2.0 ? 1 : (g.n == 0.5 ? 2 : 3));
  g.q = T.x + ira::uniform(T.base_off[seg]) + o;
  return g;
}

__device__ __forceinline__ double echo_power(float x, double n, int mode) {
  const double a = fabs((double)x);
  if (mode == 0) return a;
  if (mode == 1) return a * a;
  if (mode == 2) return sqrt(a);
  return a == 0.0 ? 0.0 : pow(a, n);
}

// s at the thread's 16 positions c0 + 16 t .. + 15 of the chunk that starts at c0 (zeros at and after M): from the
// samples, or from the stash the partial pass wrote (stash_chunk = that chunk's EC_CHUNK doubles).
__device__ __forceinline__ void echo_chunk_s(const EchoSeg& g, int64_t c0, const double* __restrict__ stash_chunk,
                                             double s[EC_PER_THREAD]) {
  const int i0 = EC_PER_THREAD * threadIdx.x;
  if (stash_chunk != nullptr) {
#pragma unroll
    for (int r = 0; r < EC_PER_THREAD; r += 2) {
      const ira::d2u v = *reinterpret_cast<const ira::d2u*>(stash_chunk + i0 + r);
      s[r] = v.x; s[r + 1] = v.y;
    }
    return;
  }
  float xv[EC_PER_THREAD];
  ira::load_run<EC_PER_THREAD>(g.q + c0, c0, g.m, xv);
#pragma unroll
  for (int r = 0; r < EC_PER_THREAD; ++r) s[r] = echo_power(xv[r], g.n, g.mode);      // a zero sample gives 0
}

// Inclusive prefix sums inside the chunk of s (w) and of m s (v) at the thread's 16 positions; parity selects the LDS
// buffer (one barrier per call).  w[15], v[15] of the last thread are the chunk totals.
__device__ __forceinline__ void echo_chunk_scan(const double s[EC_PER_THREAD], int64_t c0, EchoShared& sh, int parity,
                                                double w[EC_PER_THREAD], double v[EC_PER_THREAD]) {
  const int t = threadIdx.x;
  const double m0 = (double)(c0 + EC_PER_THREAD * t);        // exact: m < 2^31
  w[0] = s[0];
  v[0] = m0 * s[0];
#pragma unroll
  for (int r = 1; r < EC_PER_THREAD; ++r) {
    w[r] = w[r - 1] + s[r];
    v[r] = v[r - 1] + (m0 + (double)r) * s[r];
  }
  const int lane = t & 63, wave = t >> 6;
  double ew, ev;                                             // sums over the lanes in front of this one
  const double iw = ira::wave_prefix(w[EC_PER_THREAD - 1], lane, ew), iv = ira::wave_prefix(v[EC_PER_THREAD - 1], lane, ev);
  if (lane == 63) { sh.wtot[parity][0][wave] = iw; sh.wtot[parity][1][wave] = iv; }
  __syncthreads();
  double pw = 0.0, pv = 0.0;
#pragma unroll
  for (int k = 0; k < EC_WAVES - 1; ++k)
    if (k < wave) { pw += sh.wtot[parity][0][k]; pv += sh.wtot[parity][1][k]; }
  ew = pw + ew;
  ev = pv + ev;
#pragma unroll
  for (int r = 0; r < EC_PER_THREAD; ++r) { w[r] += ew; v[r] += ev; }
}

__device__ __forceinline__ double echo_ts(double w, double v, double fs) { return w == 0.0 ? 0.0 : v / (fs * w); }

// a curve key is ira::float_key; 0 is below every key a value can take: "empty", read back as NaN
__device__ __forceinline__ float echo_unkey(uint32_t k) {
  return k == 0u ? __uint_as_float(0x7fc00000u) : ira::float_unkey(k);
}

__device__ __forceinline__ double* echo_scratch(double* scratch, const EchoTables& T, int seg) {
  return scratch + (int64_t)seg * (EC_HDR + EC_PER_CHUNK * T.chunk_stride);
}

__global__ __launch_bounds__(256) void echo_init_kernel(EchoTables T, int nseg, double* __restrict__ scratch,
                                                        uint32_t* __restrict__ curve, int64_t ncurve) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t s = i0; s < nseg; s += stride) {
    unsigned long long* slot = reinterpret_cast<unsigned long long*>(echo_scratch(scratch, T, (int)s));
    slot[0] = EC_NONE;
    slot[1] = EC_NONE;
  }
  if (curve != nullptr)
    for (int64_t i = i0; i < (int64_t)nseg * ncurve; i += stride) curve[i] = 0u;
}

__global__ __launch_bounds__(EC_THREADS) void echo_partial_kernel(EchoTables T, EchoParamTable P,
                                                                  double* __restrict__ scratch,
                                                                  double* __restrict__ stash) {
  __shared__ EchoShared sh;
  const int seg = blockIdx.y;
  const EchoSeg g = echo_seg(T, P, seg);
  const int64_t c = blockIdx.x, c0 = c * EC_CHUNK;
  if (c0 >= g.m) return;
  double s[EC_PER_THREAD], w[EC_PER_THREAD], v[EC_PER_THREAD];
  echo_chunk_s(g, c0, nullptr, s);
  if (stash != nullptr) {
    double* dst = stash + ((int64_t)seg * T.chunk_stride + c) * EC_CHUNK + EC_PER_THREAD * threadIdx.x;
#pragma unroll
    for (int r = 0; r < EC_PER_THREAD; r += 2) *reinterpret_cast<ira::d2u*>(dst + r) = ira::d2u{s[r], s[r + 1]};
  }
  echo_chunk_scan(s, c0, sh, 0, w, v);
  if (threadIdx.x == EC_THREADS - 1) {
    double* sc = echo_scratch(scratch, T, seg) + EC_HDR;
    sc[c] = w[EC_PER_THREAD - 1];
    sc[T.chunk_stride + c] = v[EC_PER_THREAD - 1];
  }
}

// One wave per segment: exclusive prefix sums of the chunk totals, in blocks of 64 with a shuffle scan (any fixed
// association will do: the emit pass reads THESE carries).
__global__ __launch_bounds__(IRA_WAVE) void echo_carry_kernel(EchoTables T, EchoParamTable P, int nseg,
                                                              double* __restrict__ scratch) {
  const int seg = blockIdx.x;
  if (seg >= nseg) return;
  const EchoSeg g = echo_seg(T, P, seg);
  const int64_t nch = (g.m + EC_CHUNK - 1) / EC_CHUNK;
  double* sc = echo_scratch(scratch, T, seg) + EC_HDR;
  const int64_t cs = T.chunk_stride;
  const int lane = threadIdx.x;
  double bw = 0.0, bv = 0.0;
  for (int64_t j0 = 0; j0 < nch; j0 += IRA_WAVE) {
    const int64_t j = j0 + lane;
    double ew, ev;
    const double iw = ira::wave_prefix(j < nch ? sc[j] : 0.0, lane, ew);
    const double iv = ira::wave_prefix(j < nch ? sc[cs + j] : 0.0, lane, ev);
    if (j < nch) {
      sc[2 * cs + j] = bw + ew;
      sc[3 * cs + j] = bv + ev;
    }
    bw = bw + __shfl(iw, 63, 64);
    bv = bv + __shfl(iv, 63, 64);
  }
}

__global__ __launch_bounds__(EC_THREADS) void echo_emit_kernel(EchoTables T, EchoParamTable P,
                                                               double* __restrict__ scratch,
                                                               const double* __restrict__ stash,
                                                               uint32_t* __restrict__ curve, int64_t ncurve) {
  __shared__ EchoShared sh;
  __shared__ double ts_lds[EC_TS_SLOTS];
  __shared__ double wave_best[EC_WAVES];
  __shared__ long long wave_idx[EC_WAVES];
  const int seg = blockIdx.y;
  const EchoSeg g = echo_seg(T, P, seg);
  const int64_t c = blockIdx.x, c0 = c * EC_CHUNK;
  if (c0 >= g.m) return;
  double* hdr = echo_scratch(scratch, T, seg);
  double* sc = hdr + EC_HDR;
  const int64_t cs = T.chunk_stride;
  const int tid = threadIdx.x, i0 = EC_PER_THREAD * tid;
  const double* stash_seg = stash != nullptr ? stash + (int64_t)seg * cs * EC_CHUNK : nullptr;
  double s[EC_PER_THREAD], w[EC_PER_THREAD], v[EC_PER_THREAD];
  if (c > 0) {                                               // the chunk in front: every sample of it lies below M
    echo_chunk_s(g, c0 - EC_CHUNK, stash_seg ? stash_seg + (c - 1) * EC_CHUNK : nullptr, s);
    echo_chunk_scan(s, c0 - EC_CHUNK, sh, 0, w, v);
    const double cw = sc[2 * cs + c - 1], cv = sc[3 * cs + c - 1];
    if (i0 >= EC_CHUNK - EC_HALO) {
#pragma unroll
      for (int r = 0; r < EC_PER_THREAD; ++r)
        ts_lds[ts_slot(i0 + r - (EC_CHUNK - EC_HALO))] = echo_ts(w[r] + cw, v[r] + cv, g.fs);
    }
  }
  echo_chunk_s(g, c0, stash_seg ? stash_seg + c * EC_CHUNK : nullptr, s);
  echo_chunk_scan(s, c0, sh, 1, w, v);
  const double cw = sc[2 * cs + c], cv = sc[3 * cs + c];
  double ts[EC_PER_THREAD];
#pragma unroll
  for (int r = 0; r < EC_PER_THREAD; ++r) {
    const double wm = w[r] + cw, vm = v[r] + cv;
    ts[r] = echo_ts(wm, vm, g.fs);
    ts_lds[ts_slot(EC_HALO + i0 + r)] = ts[r];
    if (c0 + i0 + r == g.m - 1) { hdr[2] = ts[r]; hdr[3] = wm; hdr[4] = vm; }
  }
  __syncthreads();
  const double dof = (double)g.lag / g.fs;                   // D / fs seconds
  double best = -INFINITY;
  long long best_i = -1, f10 = INT64_MAX, f50 = INT64_MAX;
  const bool want_curve = curve != nullptr && g.step > 0;
  int64_t k = want_curve ? (c0 + i0) / g.step : 0;           // the curve step of the thread's first sample ...
  int64_t rem = want_curve ? (c0 + i0) - k * g.step : 0;     // ... and the sample's place in it
  double run = -INFINITY;
  bool have = false;
  uint32_t* crow = want_curve ? curve + (int64_t)seg * ncurve : nullptr;
#pragma unroll
  for (int r = 0; r < EC_PER_THREAD; ++r) {
    const long long m = c0 + i0 + r;
    if (m < g.m) {
      // index >= 0: D <= EC_HALO; below EC_HALO only when c > 0 (m - D >= 0 in chunk 0 means i0 + r >= D)
      const double tl = m < g.lag ? 0.0 : ts_lds[ts_slot(EC_HALO + i0 + r - g.lag)];
      const double ek = (ts[r] - tl) / dof;
      if (ek > best) { best = ek; best_i = m; }
      if (ek >= g.thr10 && m < f10) f10 = m;
      if (ek >= g.thr50 && m < f50) f50 = m;
      if (want_curve) {
        if (!have || ek > run || ek != ek) run = ek;         // a NaN stays: the row is non-finite
        have = true;
      }
    }
    if (want_curve) {
      if (++rem == g.step || r == EC_PER_THREAD - 1) {
        if (have && k < ncurve) atomicMax(&crow[k], ira::float_key((float)run));
        have = false;
        run = -INFINITY;
        if (rem == g.step) { rem = 0; ++k; }
      }
    }
  }
  // first crossings: rare events, wave-uniform test first
  if (__any(f10 != INT64_MAX)) {
    f10 = ira::wave_min(f10);
    if ((tid & 63) == 0) atomicMin(reinterpret_cast<unsigned long long*>(hdr), (unsigned long long)f10);
  }
  if (__any(f50 != INT64_MAX)) {
    f50 = ira::wave_min(f50);
    if ((tid & 63) == 0) atomicMin(reinterpret_cast<unsigned long long*>(hdr) + 1, (unsigned long long)f50);
  }
  // the chunk's maximum, the smallest index on a tie: (greater value, then smaller index) is a total order
  ira::wave_argmax(best, best_i);
  if ((tid & 63) == 0) { wave_best[tid >> 6] = best; wave_idx[tid >> 6] = best_i; }
  __syncthreads();
  if (tid == 0) {
    for (int wv = 1; wv < EC_WAVES; ++wv)
      if (wave_best[wv] > best || (wave_best[wv] == best && wave_idx[wv] < best_i)) { best = wave_best[wv]; best_i = wave_idx[wv]; }
    sc[4 * cs + c] = best;
    sc[5 * cs + c] = (double)best_i;
  }
}

__global__ __launch_bounds__(IRA_WAVE) void echo_fold_kernel(EchoTables T, EchoParamTable P, int nseg,
                                                             const double* __restrict__ scratch,
                                                             double* __restrict__ rec, uint32_t* __restrict__ curve,
                                                             int64_t ncurve) {
  const int seg = blockIdx.x;
  if (seg >= nseg) return;
  const EchoSeg g = echo_seg(T, P, seg);
  const int64_t nch = (g.m + EC_CHUNK - 1) / EC_CHUNK;
  const double* hdr = scratch + (int64_t)seg * (EC_HDR + EC_PER_CHUNK * T.chunk_stride);
  const double* sc = hdr + EC_HDR;
  const int64_t cs = T.chunk_stride;
  const int lane = threadIdx.x;
  double best = -INFINITY, best_i = -1.0;
  for (int64_t c = lane; c < nch; c += IRA_WAVE) {
    const double b = sc[4 * cs + c], bi = sc[5 * cs + c];
    if (b > best || (b == best && bi < best_i)) { best = b; best_i = bi; }
  }
  ira::wave_argmax(best, best_i);
  if (lane == 0) {
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    const unsigned long long* slot = reinterpret_cast<const unsigned long long*>(hdr);
    double* o = rec + (int64_t)seg * IRA_ECHO_DOUBLES;
    const bool any = g.m > 0;
    o[0] = any && best_i >= 0.0 ? best : qnan;
    o[1] = any ? best_i : -1.0;
    o[2] = any && slot[0] != EC_NONE ? (double)slot[0] : -1.0;
    o[3] = any && slot[1] != EC_NONE ? (double)slot[1] : -1.0;
    o[4] = any ? hdr[2] : qnan;
    o[5] = any ? hdr[3] : 0.0;
    o[6] = (double)g.m_raw;
    o[7] = any ? hdr[4] : 0.0;
  }
  if (curve != nullptr) {
    uint32_t* row = curve + (int64_t)seg * ncurve;
    for (int64_t k = lane; k < ncurve; k += IRA_WAVE) reinterpret_cast<float*>(row)[k] = echo_unkey(row[k]);
  }
}

inline bool ec_shape_ok(int32_t nseg, int64_t max_len) {
  return nseg >= 0 && nseg <= 65535 && max_len >= 0 && max_len <= EC_MAX_LEN;
}

// An integer-valued double in [lo, hi] (NaN fails).
inline bool ec_whole(double v, double lo, double hi) { return v >= lo && v <= hi && v == floor(v); }

}  // namespace

extern "C" int64_t ira_echo_scratch_doubles(int32_t nseg, int64_t max_len) {
  if (!ec_shape_ok(nseg, max_len)) return IRA_E_SIZE;
  return (int64_t)nseg * (EC_HDR + EC_PER_CHUNK * ira::ceil_div(max_len, EC_CHUNK));
}

extern "C" int32_t ira_echo_criterion(const float* x_dev, const int64_t* base_off_dev, const int64_t* base_len_dev,
                                      const int32_t* chan_of_seg_dev, const int32_t* param_of_seg_dev,
                                      const int64_t* onset_dev, int32_t nseg, int64_t max_len, const double* params,
                                      int32_t nparam, int64_t ncurve, double* scratch_dev, double* stash_dev,
                                      double* rec_dev, float* curve_dev, void* stream) {
  IRA_CHECK_PTR(x_dev); IRA_CHECK_PTR(base_off_dev); IRA_CHECK_PTR(base_len_dev); IRA_CHECK_PTR(chan_of_seg_dev);
  IRA_CHECK_PTR(param_of_seg_dev); IRA_CHECK_PTR(onset_dev); IRA_CHECK_PTR(params); IRA_CHECK_PTR(scratch_dev);
  IRA_CHECK_PTR(rec_dev);
  if (ncurve > 0) IRA_CHECK_PTR(curve_dev);
  if (nparam < 1 || nparam > IRA_ECHO_MAX_PARAMS) return IRA_E_SIZE;
  if (!ec_shape_ok(nseg, max_len)) return IRA_E_SIZE;
  if (ncurve < 0 || ncurve > EC_MAX_LEN) return IRA_E_SIZE;
  EchoParamTable P;
  for (int p = 0; p < IRA_ECHO_MAX_PARAMS; ++p) {
    for (int k = 0; k < IRA_ECHO_PARAM_DOUBLES; ++k) P.v[p][k] = p < nparam ? params[p * IRA_ECHO_PARAM_DOUBLES + k] : 0.0;
    if (p >= nparam) continue;
    const double* v = P.v[p];
    if (!(isfinite(v[0]) && v[0] > 0.0)) return IRA_E_SIZE;                       // exponent n
    if (!ec_whole(v[1], 1.0, (double)IRA_ECHO_MAX_LAG)) return IRA_E_SIZE;        // D
    if (!ec_whole(v[2], 0.0, (double)EC_MAX_LEN)) return IRA_E_SIZE;              // G
    if (!ec_whole(v[3], 0.0, (double)EC_MAX_LEN)) return IRA_E_SIZE;              // Mmax
    if (!ec_whole(v[4], 0.0, (double)EC_MAX_LEN)) return IRA_E_SIZE;              // S (0: no curve)
    if (!(isfinite(v[5]) && isfinite(v[6]))) return IRA_E_SIZE;                   // thresholds
    if (!(isfinite(v[7]) && v[7] > 0.0)) return IRA_E_SIZE;                       // fs
  }
  if (nseg == 0) return IRA_OK;
  hipStream_t st = (hipStream_t)stream;
  const int64_t chunks = ira::ceil_div(max_len, EC_CHUNK);
  const EchoTables T{x_dev, base_off_dev, base_len_dev, chan_of_seg_dev, param_of_seg_dev, onset_dev, nparam, chunks};
  uint32_t* keys = ncurve > 0 ? reinterpret_cast<uint32_t*>(curve_dev) : nullptr;
  {
    const int64_t items = (int64_t)nseg * (ncurve > 0 ? ncurve : 1);
    const int64_t blocks = (items + 255) / 256;
    echo_init_kernel<<<(unsigned)(blocks < 2048 ? blocks : 2048), 256, 0, st>>>(T, nseg, scratch_dev, keys, ncurve);
  }
  if (chunks > 0) {
    echo_partial_kernel<<<dim3((unsigned)chunks, nseg), EC_THREADS, 0, st>>>(T, P, scratch_dev, stash_dev);
    echo_carry_kernel<<<nseg, IRA_WAVE, 0, st>>>(T, P, nseg, scratch_dev);
    echo_emit_kernel<<<dim3((unsigned)chunks, nseg), EC_THREADS, 0, st>>>(T, P, scratch_dev, stash_dev, keys, ncurve);
  }
  echo_fold_kernel<<<nseg, IRA_WAVE, 0, st>>>(T, P, nseg, scratch_dev, rec_dev, keys, ncurve);
  IRA_RETURN_LAUNCH();
}
