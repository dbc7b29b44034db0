// Lundeby noise-floor truncation of the Schroeder integration (ISO 3382-1, 5.3.3 and 6): block energies, the iterative
// cross-point estimate and the truncated, compensated energy-decay curve.  Nothing in the reference estimates a noise
// floor; the algorithm is pinned in the docstring of audio_analysis_amd/analyse/lundeby.py (the host side).
// Compiled with -ffp-contract=off: float64 products and sums round one operation at a time.
//
// A row is one signal (a channel's broadband signal or one of its band signals) from its start index s on:
// s = start[chan_of_seg[row]] is read on the device, L = base_len[row] - s, and the host's per-row block size B and block
// count nb must satisfy nb == L / B (a row whose tables do not is treated as having no blocks: status "too short").
//   block_energy_kernel      (chunks x rows)  E[j] = sum of float64(y)^2 over block j, j < nb, and the partial tail as E[nb]
//   lundeby_estimate_kernel  (1 wg / row)     steps 2 to 6 on E in LDS -> record, curve length, per-block suffix energies
//   edc_truncated_kernel     (chunks x rows)  in-block reverse sums + the block's suffix (+ C) -> dB -> float32
// Both sample passes stage a chunk of G = 4096 / B whole blocks in LDS with 16-byte loads from the first 16-byte aligned
// address of the chunk on (scalar loads in front of it and behind the last whole quad), then sum FROM LDS: which thread adds
// which sample in which order is a function of B (and, for the partial tail block, of its length) alone, never of the
// address.  No atomics; every reduction tree is fixed.
#include "ira_common.h"
#include "ira_edc_tile.h"
#include "ira_lundeby_rows.h"
#include "ira_reduce.h"

namespace {

constexpr int LB_THREADS = 256;
constexpr int LB_WAVES = LB_THREADS / IRA_WAVE;
constexpr int LB_MIN_BLOCKS = 32;
constexpr int LB_MAX_ROUNDS = 5;
constexpr double LB_TINY = 1e-300;

typedef float lb_f4 __attribute__((ext_vector_type(4)));

// cnt samples from q into LDS: scalar loads up to the first 16-byte aligned address, 16-byte loads, scalar tail.
__device__ __forceinline__ void lb_stage_load(const float* q, int cnt, float* lds) {
  const int tid = threadIdx.x;
  int head = (int)(((16u - (unsigned)((uintptr_t)q & 15u)) & 15u) >> 2);
  if (head > cnt) head = cnt;
  const int nq = (cnt - head) >> 2;
  if (tid < head) lds[tid] = q[tid];
  const lb_f4* q4 = reinterpret_cast<const lb_f4*>(q + head);
#pragma unroll 4
  for (int i = tid; i < nq; i += LB_THREADS) {
    const lb_f4 v = q4[i];
    float* d = lds + head + 4 * i;
    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
  }
  const int t0 = head + 4 * nq + tid;
  if (t0 < cnt) lds[t0] = q[t0];
}

// The mirror image: cnt floats from LDS to dst.
__device__ __forceinline__ void lb_stage_store(float* dst, int cnt, const float* lds) {
  const int tid = threadIdx.x;
  int head = (int)(((16u - (unsigned)((uintptr_t)dst & 15u)) & 15u) >> 2);
  if (head > cnt) head = cnt;
  const int nq = (cnt - head) >> 2;
  if (tid < head) dst[tid] = lds[tid];
  lb_f4* d4 = reinterpret_cast<lb_f4*>(dst + head);
#pragma unroll 4
  for (int i = tid; i < nq; i += LB_THREADS) {
    const float* s = lds + head + 4 * i;
    d4[i] = lb_f4{s[0], s[1], s[2], s[3]};
  }
  const int t0 = head + 4 * nq + tid;
  if (t0 < cnt) dst[t0] = lds[t0];
}

// ------------------------------------------------------------------------------------------------
// Pass 1: block energies.  Wave w of a workgroup sums blocks w, w + 4, ... of its chunk: lane l adds the block's samples
// l, l + 64, ... in ascending order, the lanes meet in the fixed butterfly of wave_sum.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LB_THREADS) void block_energy_kernel(
    const float* __restrict__ x, const int64_t* __restrict__ base_off, const int64_t* __restrict__ base_len,
    const int32_t* __restrict__ chan_of_seg, const int64_t* __restrict__ start, const int32_t* __restrict__ blk_size,
    const int32_t* __restrict__ nblk, const int64_t* __restrict__ blk_off, double* __restrict__ blk) {
  __shared__ float stage[LB_STAGE];
  const int row = blockIdx.y;
  const LbRow r = lb_row(row, base_len, chan_of_seg, start, blk_size, nblk);
  double* E = blk + ira::uniform(blk_off[row]);
  const int64_t whole = (int64_t)r.nb * r.B;
  if (blockIdx.x == 0 && threadIdx.x == 0 && r.L == whole) E[r.nb] = 0.0;     // no partial tail block
  const int nbt = r.nb + (r.L > whole ? 1 : 0);
  const int G = LB_STAGE / r.B;
  const int j0 = blockIdx.x * G;
  if (j0 >= nbt) return;
  const int nj = nbt - j0 < G ? nbt - j0 : G;
  const int64_t c0 = (int64_t)j0 * r.B;
  const int64_t left = r.L - c0;
  const int cnt = (int)(left < (int64_t)nj * r.B ? left : (int64_t)nj * r.B);
  lb_stage_load(x + ira::uniform(base_off[row]) + r.s + c0, cnt, stage);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int jl = wave; jl < nj; jl += LB_WAVES) {
    const int b0 = jl * r.B;
    const int blen = cnt - b0 < r.B ? cnt - b0 : r.B;
    double acc = 0.0;
    for (int i = lane; i < blen; i += IRA_WAVE) {
      const double d = (double)stage[b0 + i];
      acc += d * d;
    }
    acc = ira::wave_sum(acc);
    if (lane == 0) E[j0 + jl] = acc;
  }
}

// ------------------------------------------------------------------------------------------------
// The estimate.  One workgroup per row; E lives in LDS, the interval means M of m >= 2 blocks beside it (at most 2048 of
// them; for m == 1 an interval IS a block and M[k] = E[k] / B is formed where it is used).  Every sum over intervals is: a
// thread adds its intervals k = tid, tid + 256, ... in ascending order, the wave's butterfly, the four waves in order.
// ------------------------------------------------------------------------------------------------
struct LbShared {
  double E[LB_MAX_BLOCKS + 1];
  double M[LB_MAX_BLOCKS / 2];
  double tot[LB_THREADS];
  double w[LB_WAVES];
  long long wi[LB_WAVES];
};

__device__ __forceinline__ double lb_sum(double v, LbShared& sh) {
  v = ira::wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh.w[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = sh.w[0];
#pragma unroll
  for (int i = 1; i < LB_WAVES; ++i) r += sh.w[i];
  return r;
}

__device__ __forceinline__ long long lb_min(long long v, LbShared& sh) {
  v = ira::wave_min(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh.wi[threadIdx.x >> 6] = v;
  __syncthreads();
  long long r = sh.wi[0];
#pragma unroll
  for (int i = 1; i < LB_WAVES; ++i) r = sh.wi[i] < r ? sh.wi[i] : r;
  return r;
}

// (largest value, its first index); values are finite
__device__ __forceinline__ void lb_argmax(double& v, long long& idx, LbShared& sh) {
  ira::wave_argmax(v, idx);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { sh.w[threadIdx.x >> 6] = v; sh.wi[threadIdx.x >> 6] = idx; }
  __syncthreads();
  v = sh.w[0]; idx = sh.wi[0];
#pragma unroll
  for (int i = 1; i < LB_WAVES; ++i)
    if (sh.w[i] > v || (sh.w[i] == v && sh.wi[i] < idx)) { v = sh.w[i]; idx = sh.wi[i]; }
}

struct LbMeans {
  int m, K, B;
  double mmax;
  int kmax;
  __device__ __forceinline__ double at(int k, const LbShared& sh) const {
    return m == 1 ? sh.E[k] / (double)B : sh.M[k];
  }
  __device__ __forceinline__ double db_of(double mean) const { return 10.0 * log10(fmax(mean, LB_TINY) / mmax); }
  __device__ __forceinline__ double D(int k, const LbShared& sh) const { return db_of(at(k, sh)); }
};

// Step 2: interval means of m blocks, their maximum and its first index.
__device__ __forceinline__ LbMeans lb_means(int m, int nb, int B, LbShared& sh) {
  LbMeans a;
  a.m = m; a.B = B; a.K = nb / m;
  __syncthreads();
  if (m > 1) {
    const double div = (double)((long long)m * B);
    for (int k = threadIdx.x; k < a.K; k += LB_THREADS) {
      double s = 0.0;
      for (int i = 0; i < m; ++i) s += sh.E[k * m + i];
      sh.M[k] = s / div;
    }
  }
  __syncthreads();
  double v = -1.0;
  long long idx = 0x7fffffff;
  for (int k = threadIdx.x; k < a.K; k += LB_THREADS) {
    const double mk = a.at(k, sh);
    if (mk > v) { v = mk; idx = k; }
  }
  lb_argmax(v, idx, sh);
  a.mmax = v; a.kmax = (int)idx;
  return a;
}

// mean of M[ka .. K)
__device__ __forceinline__ double lb_tail_mean(const LbMeans& a, int ka, LbShared& sh) {
  double s = 0.0;
  for (int k = ka + threadIdx.x; k < a.K; k += LB_THREADS) s += a.at(k, sh);
  return lb_sum(s, sh) / (double)(a.K - ka);
}

// first k in [ka, kb) with D[k] < thr (strict) or D[k] <= thr; kb if there is none
__device__ __forceinline__ int lb_first(const LbMeans& a, int ka, int kb, double thr, bool strict, LbShared& sh) {
  long long f = kb;
  for (int k = ka + threadIdx.x; k < kb; k += LB_THREADS) {
    const double d = a.D(k, sh);
    if ((strict ? d < thr : d <= thr) && k < f) f = k;
  }
  return (int)lb_min(f, sh);
}

// Least-squares line D ~ slope * t + c over the intervals [ka, kb), t = (k + 0.5) m B samples.  With u = k - ka and
// ubar = (n - 1) / 2: slope per interval = sum (u - ubar) D / sum (u - ubar)^2, the denominator in closed form
// n (n^2 - 1) / 12 (exact in float64 for n <= 4096).
__device__ __forceinline__ void lb_line(const LbMeans& a, int ka, int kb, double& slope, double& c, LbShared& sh) {
  const double n = (double)(kb - ka), ubar = 0.5 * (n - 1.0);
  double sd = 0.0, sxd = 0.0;
  for (int k = ka + threadIdx.x; k < kb; k += LB_THREADS) {
    const double d = a.D(k, sh);
    sd += d;
    sxd += ((double)(k - ka) - ubar) * d;
  }
  sd = lb_sum(sd, sh);
  sxd = lb_sum(sxd, sh);
  const double per_interval = sxd / (n * (n * n - 1.0) / 12.0);
  slope = per_interval / (double)((long long)a.m * a.B);
  c = sd / n - per_interval * (ubar + (double)ka + 0.5);
}

__global__ __launch_bounds__(LB_THREADS) void lundeby_estimate_kernel(
    const int64_t* __restrict__ base_len, const int32_t* __restrict__ chan_of_seg, const int64_t* __restrict__ start,
    const int32_t* __restrict__ blk_size, const int32_t* __restrict__ nblk, const int32_t* __restrict__ first_m,
    const int64_t* __restrict__ blk_off, const double* __restrict__ blk, int compensate, double* __restrict__ rec_out,
    int64_t* __restrict__ len_out, double* __restrict__ suffix) {
  __shared__ LbShared sh;
  const int row = blockIdx.x, tid = threadIdx.x;
  const LbRow r = lb_row(row, base_len, chan_of_seg, start, blk_size, nblk);
  const int nb = r.nb, B = r.B;
  const int64_t off = ira::uniform(blk_off[row]);
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  double* rec = rec_out + (int64_t)row * IRA_LUNDEBY_DOUBLES;
  int status = 0;
  double Ln = qnan, slope = qnan, c = qnan, C = 0.0, tx = qnan, tx0 = qnan;
  int rounds = 0, m1 = 0, k0 = 0, k1 = 0;
  LbMeans a{};
  int64_t t1 = 0, curve_len = 0;

  if (nb < LB_MIN_BLOCKS) status = IRA_LUNDEBY_TOO_SHORT;
  if (!status) {
    double emax = 0.0;
    int bad = 0;
    for (int j = tid; j <= nb; j += LB_THREADS) {
      const double e = blk[off + j];
      sh.E[j] = e;
      if (!(e <= 1.7976931348623157e308)) bad = 1;         // NaN or infinite
      if (j < nb) emax = fmax(emax, e);
    }
    bad = lb_sum((double)bad, sh) != 0.0;
    long long none = 0;
    lb_argmax(emax, none, sh);
    if (bad) status = IRA_LUNDEBY_NON_FINITE;
    else if (emax == 0.0) status = IRA_LUNDEBY_SILENT;
  }
  // ---- step 3: preliminary pass ---------------------------------------------------------------------------------------
  if (!status) {
    int m0 = ira::uniform(first_m[row]);
    if (m0 < 1) m0 = 1;
    if (m0 > nb) m0 = nb;
    a = lb_means(m0, nb, B, sh);
    const int ntail = a.K / 10 > 1 ? a.K / 10 : 1;
    Ln = a.db_of(lb_tail_mean(a, a.K - ntail, sh));
    const int kend = lb_first(a, a.kmax + 1, a.K, Ln + 10.0, true, sh);
    if (kend >= a.K || kend - a.kmax < 3) status = IRA_LUNDEBY_NO_RANGE;
    if (!status) {
      lb_line(a, a.kmax, kend, slope, c, sh);
      if (!(slope < 0.0)) status = IRA_LUNDEBY_SLOPE;
    }
  }
  // ---- steps 4 and 5: re-averaging, iteration --------------------------------------------------------------------------
  if (!status) {
    tx0 = tx = (Ln - c) / slope;
    const double hi = (double)(nb / 16 > 1 ? nb / 16 : 1);
    double want = floor((-10.0 / slope) / 5.0 / (double)B + 0.5);
    if (!(want >= 1.0)) want = 1.0;
    if (want > hi) want = hi;
    m1 = (int)want;
    a = lb_means(m1, nb, B, sh);
    const double mb = (double)((long long)m1 * B);
    for (int it = 0; it < LB_MAX_ROUNDS && !status; ++it) {
      rounds = it + 1;
      const double from = fmin(tx + (-10.0 / slope), 0.9 * (double)((long long)nb * B));
      double before = 0.0;
      for (int k = tid; k < a.K; k += LB_THREADS) before += (((double)k + 0.5) * mb < from) ? 1.0 : 0.0;
      int kn = (int)lb_sum(before, sh);
      if (kn > a.K - 1) kn = a.K - 1;
      Ln = a.db_of(lb_tail_mean(a, kn, sh));
      k1 = lb_first(a, a.kmax + 1, a.K, Ln + 10.0, true, sh);
      if (k1 >= a.K) { status = IRA_LUNDEBY_NO_RANGE; break; }
      k0 = lb_first(a, a.kmax, k1, Ln + 30.0, false, sh);
      if (k0 > k1 - 3) k0 = k1 - 3;
      if (k0 < a.kmax) { status = IRA_LUNDEBY_NO_RANGE; break; }
      lb_line(a, k0, k1, slope, c, sh);
      if (!(slope < 0.0)) { status = IRA_LUNDEBY_SLOPE; break; }
      const double next = (Ln - c) / slope;
      const double moved = fabs(next - tx);
      tx = next;
      if (moved < mb) break;
    }
  }
  // ---- step 6 ----------------------------------------------------------------------------------------------------------
  int ncurve = 0;            // blocks the curve covers (the partial tail block included when there is no floor in the file)
  if (!status) {
    const double whole = (double)((long long)nb * B);
    if (tx >= whole) {
      status = IRA_LUNDEBY_NO_FLOOR;
      t1 = (int64_t)nb * B;
      curve_len = r.L;
      ncurve = nb + (r.L > t1 ? 1 : 0);
      C = 0.0;
    } else {
      double cut = floor(tx / (double)B) * (double)B;
      if (!(cut >= (double)B)) cut = (double)B;
      if (cut > whole) cut = whole;
      t1 = (int64_t)cut;
      curve_len = t1;
      ncurve = (int)(t1 / B);
      const double lev = a.mmax * pow(10.0, (c + slope * cut) / 10.0);
      C = compensate ? lev * 10.0 / (-slope * 2.302585092994046) : 0.0;
    }
    const double chk = Ln + slope + c + C + tx;
    if (!(fabs(chk) <= 1.7976931348623157e308)) status = IRA_LUNDEBY_NON_FINITE;
  }
  if (status & ~IRA_LUNDEBY_NO_FLOOR) {
    if (tid == 0) {
      rec[0] = (double)status;
      for (int i = 1; i < IRA_LUNDEBY_DOUBLES; ++i) rec[i] = qnan;
      len_out[row] = 0;
    }
    return;
  }
  // ---- suffix energies: base[j] = (energy of the blocks behind j, inside the curve) + C ---------------------------------
  // thread t owns the blocks [17 t, 17 t + 17); its totals meet in one serial sweep from the last thread down.
  constexpr int OWN = (LB_MAX_BLOCKS + LB_THREADS) / LB_THREADS;
  const int lo = OWN * tid, hi = lo + OWN < ncurve ? lo + OWN : ncurve;
  {
    double acc = 0.0;
    for (int j = hi - 1; j >= lo; --j) acc += sh.E[j];
    __syncthreads();
    sh.tot[tid] = acc;
    __syncthreads();
    if (tid == 0) {
      double run = 0.0;
      for (int t = LB_THREADS - 1; t >= 0; --t) {
        const double v = sh.tot[t];
        sh.tot[t] = run;
        run += v;
      }
    }
    __syncthreads();
    double* base = suffix + off;
    acc = 0.0;
    const double behind = sh.tot[tid];
    for (int j = hi - 1; j >= lo; --j) {
      const double b = (behind + acc) + C;
      base[j] = b;
      if (j == 0) sh.w[0] = sh.E[0] + b;          // edc[0]; the curve kernel writes exactly this value at index 0
      acc += sh.E[j];
    }
  }
  __syncthreads();
  if (tid == 0) {
    rec[0] = (double)status; rec[1] = Ln; rec[2] = (double)t1; rec[3] = slope; rec[4] = c; rec[5] = C;
    rec[6] = (double)rounds; rec[7] = (double)m1; rec[8] = (double)a.kmax; rec[9] = (double)k0; rec[10] = (double)k1;
    rec[11] = tx0; rec[12] = tx; rec[13] = a.mmax; rec[14] = sh.w[0]; rec[15] = (double)ncurve;
    len_out[row] = curve_len;
  }
}

// ------------------------------------------------------------------------------------------------
// Pass 2: the curve.  A wave takes a block of its chunk: lane l owns the block's samples [l per, (l + 1) per),
// per = ceil(B / 64), and forms their suffix sums from its last sample down; the lanes' totals meet in a suffix scan towards
// the higher lanes.  edc[i] = (suffix inside the block) + base[j]; then the dB chain of ira_edc_db (ira::EdcDb):
// max(., eps) / max(edc[0], eps) -> 10 log10 -> max(., floor_db) -> float32.  The float32 values replace the samples in LDS
// and leave with 16-byte stores.  A band row may be written over the signal it is read from: a workgroup has read its chunk
// before it writes it, and no other workgroup touches that chunk.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LB_THREADS) void edc_truncated_kernel(
    const float* x, const int64_t* __restrict__ base_off, const int64_t* __restrict__ base_len,
    const int32_t* __restrict__ chan_of_seg, const int64_t* __restrict__ start, const int32_t* __restrict__ blk_size,
    const int32_t* __restrict__ nblk, const int64_t* __restrict__ blk_off, const double* __restrict__ rec_in,
    const int64_t* __restrict__ curve_len, const double* __restrict__ suffix, double eps, double floor_db,
    float* out, const int64_t* __restrict__ out_off) {      // x and out may be the same memory: no __restrict__
  __shared__ float stage[LB_STAGE];
  __shared__ ira::LogTabEntry ltab[ira::LOGTAB_N];
  const int row = blockIdx.y;
  const LbRow r = lb_row(row, base_len, chan_of_seg, start, blk_size, nblk);
  int64_t n = ira::uniform(curve_len[row]);
  if (n > r.L) n = r.L;
  const int G = LB_STAGE / r.B;
  const int j0 = blockIdx.x * G;
  const int64_t c0 = (int64_t)j0 * r.B;
  if (c0 >= n) return;
  const int64_t left = n - c0;
  const int cnt = (int)(left < (int64_t)G * r.B ? left : (int64_t)G * r.B);
  const int nj = (cnt + r.B - 1) / r.B;
  lb_stage_load(x + ira::uniform(base_off[row]) + r.s + c0, cnt, stage);
  ira::build_log_table(ltab, threadIdx.x);
  __syncthreads();
  const double* base = suffix + ira::uniform(blk_off[row]);
  const double first = ira::uniform(rec_in[(int64_t)row * IRA_LUNDEBY_DOUBLES + 14]);
  const ira::EdcDb D(ira::np_max(first, eps), eps, floor_db, ltab);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int per = (r.B + IRA_WAVE - 1) / IRA_WAVE;
  for (int jl = wave; jl < nj; jl += LB_WAVES) {
    const int b0 = jl * r.B;
    const int blen = cnt - b0 < r.B ? cnt - b0 : r.B;
    const int lo = lane * per < blen ? lane * per : blen;
    const int hi = lo + per < blen ? lo + per : blen;
    double acc = 0.0;
    for (int i = hi - 1; i >= lo; --i) {
      const double d = (double)stage[b0 + i];
      acc = d * d + acc;
    }
    double run;                                       // the lanes after this one
    ira::wave_suffix(acc, lane, run);
    const double bj = base[j0 + jl];
    for (int i = hi - 1; i >= lo; --i) {
      const double d = (double)stage[b0 + i];
      run = d * d + run;
      // edc[0] sums the same energies in another order (the estimate's E[0] + base[0]): a later sample may come out one
      // float64 rounding above it, and is held to it, so that no sample of the curve lies above 0 dB
      stage[b0 + i] = D.db32((c0 + b0 + i == 0) ? first : fmin(run + bj, first));
    }
  }
  __syncthreads();
  lb_stage_store(out + ira::uniform(out_off[row]) + c0, cnt, stage);
}

static inline bool lb_bad_count(int32_t nseg, int32_t max_chunks) {
  return nseg > 65535 || max_chunks < 1 || max_chunks > LB_MAX_BLOCKS + 1;
}

}  // namespace

extern "C" int64_t ira_lundeby_scratch_doubles(int32_t nseg, int32_t max_nblk) {
  if (nseg < 0 || nseg > 65535 || max_nblk < 0 || max_nblk > LB_MAX_BLOCKS) return IRA_E_SIZE;
  return (int64_t)nseg * (max_nblk + 1);
}

extern "C" int32_t ira_block_energy(const float* x_dev, const int64_t* base_off_dev, const int64_t* base_len_dev,
                                    const int32_t* chan_of_seg_dev, const int64_t* start_dev, const int32_t* blk_size_dev,
                                    const int32_t* nblk_dev, const int64_t* blk_off_dev, int32_t nseg, int32_t max_chunks,
                                    double* blk_dev, void* stream) {
  IRA_CHECK_PTR(x_dev); IRA_CHECK_PTR(base_off_dev); IRA_CHECK_PTR(base_len_dev); IRA_CHECK_PTR(chan_of_seg_dev);
  IRA_CHECK_PTR(start_dev); IRA_CHECK_PTR(blk_size_dev); IRA_CHECK_PTR(nblk_dev); IRA_CHECK_PTR(blk_off_dev);
  IRA_CHECK_PTR(blk_dev);
  if (nseg <= 0) return nseg == 0 ? IRA_OK : IRA_E_SIZE;
  if (lb_bad_count(nseg, max_chunks)) return IRA_E_SIZE;
  block_energy_kernel<<<dim3((unsigned)max_chunks, nseg), LB_THREADS, 0, (hipStream_t)stream>>>(
      x_dev, base_off_dev, base_len_dev, chan_of_seg_dev, start_dev, blk_size_dev, nblk_dev, blk_off_dev, blk_dev);
  IRA_RETURN_LAUNCH();
}

extern "C" int32_t ira_lundeby_estimate(const int64_t* base_len_dev, const int32_t* chan_of_seg_dev,
                                        const int64_t* start_dev, const int32_t* blk_size_dev, const int32_t* nblk_dev,
                                        const int32_t* first_m_dev, const int64_t* blk_off_dev, int32_t nseg,
                                        const double* blk_dev, int32_t compensate, double* rec_dev, int64_t* len_out_dev,
                                        double* suffix_dev, void* stream) {
  IRA_CHECK_PTR(base_len_dev); IRA_CHECK_PTR(chan_of_seg_dev); IRA_CHECK_PTR(start_dev); IRA_CHECK_PTR(blk_size_dev);
  IRA_CHECK_PTR(nblk_dev); IRA_CHECK_PTR(first_m_dev); IRA_CHECK_PTR(blk_off_dev); IRA_CHECK_PTR(blk_dev);
  IRA_CHECK_PTR(rec_dev); IRA_CHECK_PTR(len_out_dev); IRA_CHECK_PTR(suffix_dev);
  if (compensate != 0 && compensate != 1) return IRA_E_SIZE;
  if (nseg <= 0) return nseg == 0 ? IRA_OK : IRA_E_SIZE;
  if (nseg > 65535) return IRA_E_SIZE;
  lundeby_estimate_kernel<<<nseg, LB_THREADS, 0, (hipStream_t)stream>>>(
      base_len_dev, chan_of_seg_dev, start_dev, blk_size_dev, nblk_dev, first_m_dev, blk_off_dev, blk_dev, compensate,
      rec_dev, len_out_dev, suffix_dev);
  IRA_RETURN_LAUNCH();
}

extern "C" int32_t ira_edc_truncated(const float* x_dev, const int64_t* base_off_dev, const int64_t* base_len_dev,
                                     const int32_t* chan_of_seg_dev, const int64_t* start_dev, const int32_t* blk_size_dev,
                                     const int32_t* nblk_dev, const int64_t* blk_off_dev, int32_t nseg, int32_t max_chunks,
                                     const double* rec_dev, const int64_t* len_dev, const double* suffix_dev, double eps,
                                     double floor_db, float* edc_dev, const int64_t* edc_off_dev, void* stream) {
  IRA_CHECK_PTR(x_dev); IRA_CHECK_PTR(base_off_dev); IRA_CHECK_PTR(base_len_dev); IRA_CHECK_PTR(chan_of_seg_dev);
  IRA_CHECK_PTR(start_dev); IRA_CHECK_PTR(blk_size_dev); IRA_CHECK_PTR(nblk_dev); IRA_CHECK_PTR(blk_off_dev);
  IRA_CHECK_PTR(rec_dev); IRA_CHECK_PTR(len_dev); IRA_CHECK_PTR(suffix_dev); IRA_CHECK_PTR(edc_dev);
  IRA_CHECK_PTR(edc_off_dev);
  if (!(eps >= 0.0) || floor_db != floor_db) return IRA_E_SIZE;
  if (nseg <= 0) return nseg == 0 ? IRA_OK : IRA_E_SIZE;
  if (lb_bad_count(nseg, max_chunks)) return IRA_E_SIZE;
  edc_truncated_kernel<<<dim3((unsigned)max_chunks, nseg), LB_THREADS, 0, (hipStream_t)stream>>>(
      x_dev, base_off_dev, base_len_dev, chan_of_seg_dev, start_dev, blk_size_dev, nblk_dev, blk_off_dev, rec_dev, len_dev,
      suffix_dev, eps, floor_db, edc_dev, edc_off_dev);
  IRA_RETURN_LAUNCH();
}
