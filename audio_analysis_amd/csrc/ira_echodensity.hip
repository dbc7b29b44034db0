// Normalized echo density (Abel & Huang 2006) per channel: for every position of a sliding window the weighted fraction
// of samples that lie outside the window's own standard deviation, over the value a Gaussian signal gives, and the
// 8-double record reduced from the profile as stored.  Nothing in the reference computes it; the host side is
// audio_analysis_amd/analyse/echodensity.py, which states the definition.  Compiled with -ffp-contract=off: the float64
// products and sums round one operation at a time.
//
// Channel c: L = len[c] float32 samples at x + off[c], o = max(onset[c], 0), W = 2 delta + 1 weights w (float64, built on
// the host), S = step.  K = 0 if L <= o, else min((L - 1 - o) / S + 1, kmax); position j < K has its centre at c_j =
// o + j S and the window i = c_j - delta .. c_j + delta clipped to [0, L), k = i - (c_j - delta):
//   h2[i] = float64(x[i])^2,  A = sum w[k],  B = sum w[k] h2[i],  C = sum of w[k] where h2[i] A > B (1 + 2^-32),
//   each over the clipped window with k ascending;  eta = (C / A) / erfc(1 / sqrt 2);  profile[j] = float32(eta),
//   a NaN with payload IRA_NED_NAN_SILENT where B == 0 and IRA_NED_NAN_NONFINITE where B is not finite.
// The O(N W) work cannot be folded into prefix sums: the indicator depends on the position's own B.
//
//   ned_profile_kernel   grid (G, channels), 256 threads.  A workgroup walks the channel's tiles of T consecutive
//                        positions (tile = blockIdx.x, + G, ..).  Per tile it stages h2 of the tile's span (T - 1) S + W
//                        as float64 in LDS (the square is formed once per sample, not once per window), the weights are
//                        staged once per workgroup.  ONE THREAD PER POSITION, up to 4 positions per thread (p = t, t +
//                        256, ..): a thread reads w[k] once (an LDS broadcast) for its positions, and the lanes of a wave
//                        read consecutive LDS doubles (ds_read_b64, 64 banks: conflict-free).  For S > 1 the span is
//                        stored de-interleaved, sample u at slot (u mod S) P + u / S, so that position p reads slot
//                        (k mod S) P + k / S + p: consecutive lanes still read consecutive doubles; the tap loop is
//                        nested over k / S and k mod S.  P is odd, so the staging stores (stride P) spread over the
//                        banks too.  Waves without a position (a tile of a large step is short) skip the tile.
//                        Where the de-interleaved span of one position does not fit (S and W both in the thousands) the
//                        span is stored as it is and lanes read with stride S.
//                        At S = 1 a full tile takes 4 CONSECUTIVE positions per thread instead (ned_tile_slide): their
//                        windows share all but one sample per tap, so 4 taps cost two 16-byte reads of new squares
//                        where the mapping above reads 16 values, and the loop is bound by float64 issue, not LDS.
//                        A tile whose windows are all whole takes the loop without range tests and forms A once per
//                        thread; a tile with clipped windows selects w or 0 per (position, k).  x + 0 == x for the
//                        non-negative sums here, so both loops give the bits of "sum over the clipped window, k ascending".
//   ned_record_kernel    one workgroup per channel: counts of the two NaN kinds, the maximum of the other values with
//                        its first index, the first index at or above each threshold, by (value, index) orders that do
//                        not depend on the reduction tree.
// A position's three sums are a function of its own window and run in one fixed order, whatever the tile, the grid or
// the batch: a channel's profile and record are bit-identical wherever the channel lies.  No atomics, no scratch.
#include <math.h>

#include "ira_common.h"

namespace {

constexpr int NED_THREADS = 256;
constexpr int NED_ROUNDS = IRA_NED_TILE / NED_THREADS;       // positions per thread in a full tile
constexpr int NED_WAVES = NED_THREADS / IRA_WAVE;
constexpr int NED_W_MAX = 2 * IRA_NED_MAX_DELTA + 1;
// float64 slots of h2 a workgroup stages: 40 KiB, with the 32 KiB of the longest weights 72 KiB of the CU's 160 KiB, so
// two workgroups fit whatever the window; the launch asks only for what its own span and W need (47 KiB at the default
// 1 ms step and 20 ms window at 48 kHz, 23 KiB at one sample per step)
constexpr int NED_SLOTS = 5120;
constexpr int NED_SLIDE_PAD = 8;
constexpr int NED_STAGE = 8;
constexpr int NED_MAX_GRID_X = 2048;
constexpr int64_t NED_MAX_COUNT = (int64_t)1 << 31;
static_assert(IRA_NED_TILE % NED_THREADS == 0 && NED_ROUNDS == 4, "ned_tile is instantiated for 1 and 4 rounds");
static_assert(NED_SLOTS >= NED_W_MAX, "one position of the longest window fits");
static_assert(NED_SLOTS >= IRA_NED_TILE - 1 + 3841, "a full tile at step 1 up to 20 ms at 192 kHz");

struct NedGeom {
  int delta, w, step;
  int tile;                                                  // T: positions per tile
  int sl, p;                                                 // layout: sample u of the span at slot (u % sl) * p + u / sl
  int pstride;                                               // slot distance of neighbouring positions: step / sl
  int64_t kmax;
};

struct NedThresholds {
  double v[IRA_NED_MAX_THRESHOLDS];
};

struct NedChannel {
  const float* x;
  int64_t len, onset, count, room;                           // K, and the K of onset 0: what the row holds
};

__device__ __forceinline__ int64_t ned_count(int64_t len, int64_t onset, int64_t step, int64_t kmax) {
  if (len <= onset) return 0;
  const int64_t k = (len - 1 - onset) / step + 1;
  return k < kmax ? k : kmax;
}

__device__ __forceinline__ NedChannel ned_channel(const float* x, const int64_t* off, const int64_t* len,
                                                  const int64_t* onset, int ch, int64_t step, int64_t kmax) {
  NedChannel c;
  c.x = x + ira::uniform(off[ch]);
  c.len = ira::uniform(len[ch]);
  c.len = c.len > 0 ? c.len : 0;
  c.onset = ira::uniform(onset[ch]);
  c.onset = c.onset > 0 ? c.onset : 0;
  c.count = ned_count(c.len, c.onset, step, kmax);
  c.room = ned_count(c.len, 0, step, kmax);
  return c;
}

__device__ __forceinline__ float ned_nan(uint32_t bits) { return __uint_as_float(bits); }

// The positions p = t + 256 r, r < R, of one tile: npos of them exist; centre of position 0 at sample c0.
template <int R, bool EDGE, bool UNIT>
__device__ __forceinline__ void ned_tile(const double* __restrict__ h2, const double* __restrict__ wl, const NedGeom& g,
                                         int npos, int64_t c0, int64_t len, float* __restrict__ out) {
  const int t = threadIdx.x;
  if ((t & ~(IRA_WAVE - 1)) >= npos) return;                 // a wave without a position (tiles of large steps are short)
  int base[R], klo[R], khi[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int p = t + NED_THREADS * r;
    const int pc = p < npos ? p : 0;                         // a thread without a position repeats position 0, stores nothing
    base[r] = pc * g.pstride;
    const int64_t first = c0 + (int64_t)pc * g.step - g.delta;          // sample of k = 0
    const int64_t lo = -first, hi = len - 1 - first;
    klo[r] = lo > 0 ? (int)lo : 0;
    khi[r] = hi < g.w - 1 ? (int)hi : g.w - 1;
  }
  double a[R], b[R], c[R], bg[R];
#pragma unroll
  for (int r = 0; r < R; ++r) a[r] = b[r] = c[r] = bg[r] = 0.0;
  // tap k of pass 1 (A and B) or 2 (C), its square at slot base + f
  auto tap = [&](int pass, int k, int f) {
    const double w = wl[k];
    if (pass == 1 && !EDGE) a[0] += w;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const double h = h2[base[r] + f];
      const bool inside = !EDGE || (k >= klo[r] && k <= khi[r]);
      if (pass == 1) {
        if (EDGE) {
          const double ws = inside ? w : 0.0;
          a[r] += ws;
          b[r] += ws * h;
        } else {
          b[r] += w * h;
        }
      } else {
        c[r] += (inside && h * a[r] > bg[r]) ? w : 0.0;
      }
    }
  };
#pragma unroll
  for (int pass = 1; pass <= 2; ++pass) {
    if (UNIT) {
#pragma unroll 4
      for (int k = 0; k < g.w; ++k) tap(pass, k, k);
    } else {
      // k = kq sl + kr ascending, slot kr P + kq: the inner loop is a plain counted one (stride P), which the compiler
      // unrolls with the reads of several taps in flight; counters updated tap by tap kept one read in flight
      for (int k0 = 0, kq = 0; k0 < g.w; k0 += g.sl, ++kq) {
        const int nr = g.w - k0 < g.sl ? g.w - k0 : g.sl;
#pragma unroll 4
        for (int kr = 0; kr < nr; ++kr) tap(pass, k0 + kr, kr * g.p + kq);
      }
    }
    if (pass == 1) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (!EDGE) a[r] = a[0];
        bg[r] = b[r] * (1.0 + 0x1p-32);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int p = t + NED_THREADS * r;
    if (p >= npos) continue;
    float v;
    if (!(fabs(b[r]) <= 1.7976931348623157e308)) v = ned_nan(IRA_NED_NAN_NONFINITE);
    else if (b[r] == 0.0) v = ned_nan(IRA_NED_NAN_SILENT);
    else v = (float)((c[r] / a[r]) / 0.31731050786291415);
    out[p] = v;
  }
}

typedef double ned_d2 __attribute__((ext_vector_type(2)));

// One block of up to 4 window taps k = kb .. kb + taps - 1 for the thread's 4 consecutive positions: v[0 .. 6] are the
// squares at (position 0, tap kb) .. (position 3, tap kb + 3), wv the 4 weights.  PASS 1 adds to A and B, PASS 2 to C.
template <bool EDGE, int PASS>
__device__ __forceinline__ void ned_slide_block(const double v[8], const double wv[4], int kb, int taps, const int klo[4],
                                                const int khi[4], double a[4], double b[4], const double bg[4],
                                                double c[4]) {
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    if (m >= taps) break;
    const int k = kb + m;
    const double w = wv[m];
    if (PASS == 1 && !EDGE) a[0] += w;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double h = v[r + m];
      const bool inside = !EDGE || (k >= klo[r] && k <= khi[r]);
      if (PASS == 1) {
        if (EDGE) {
          const double ws = inside ? w : 0.0;
          a[r] += ws;
          b[r] += ws * h;
        } else {
          b[r] += w * h;
        }
      } else {
        c[r] += (inside && h * a[r] > bg[r]) ? w : 0.0;
      }
    }
  }
}

// One sample per step, a tile of more than 256 positions: thread t takes the 4 CONSECUTIVE positions 4 t .. 4 t + 3.
// Their windows at tap k are the samples 4 t + k .. 4 t + k + 3, so a step of 4 taps needs 4 new squares per thread (two
// 16-byte LDS reads at a 32-byte-aligned address) instead of 16: the kernel leaves the LDS bound for the float64 one.
// The sums of a position run over k ascending exactly as in ned_tile: the same bits.
template <bool EDGE>
__device__ __forceinline__ void ned_tile_slide(const double* __restrict__ h2, const double* __restrict__ wl,
                                               const NedGeom& g, int npos, int64_t c0, int64_t len,
                                               float* __restrict__ out) {
  const int p0 = 4 * threadIdx.x;
  int klo[4], khi[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t first = c0 + p0 + r - g.delta;             // sample of k = 0
    const int64_t lo = -first, hi = len - 1 - first;
    klo[r] = lo > 0 ? (int)lo : 0;
    khi[r] = hi < g.w - 1 ? (int)(hi < -1 ? -1 : hi) : g.w - 1;         // a position past the tile's last: nothing kept
  }
  double a[4], b[4], c[4], bg[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) a[r] = b[r] = c[r] = bg[r] = 0.0;
  const double* hp = h2 + p0;
  const int whole = g.w & ~3;
#pragma unroll
  for (int pass = 1; pass <= 2; ++pass) {
    double v[8], wv[4];
    {
      const ned_d2 x0 = *reinterpret_cast<const ned_d2*>(hp), x1 = *reinterpret_cast<const ned_d2*>(hp + 2);
      v[0] = x0.x; v[1] = x0.y; v[2] = x1.x; v[3] = x1.y;
    }
    for (int kb = 0; kb <= whole; kb += 4) {                  // the last block holds the W mod 4 taps that remain (W is odd)
      const ned_d2 x0 = *reinterpret_cast<const ned_d2*>(hp + kb + 4), x1 = *reinterpret_cast<const ned_d2*>(hp + kb + 6);
      const ned_d2 w0 = *reinterpret_cast<const ned_d2*>(wl + kb), w1 = *reinterpret_cast<const ned_d2*>(wl + kb + 2);
      v[4] = x0.x; v[5] = x0.y; v[6] = x1.x; v[7] = x1.y;
      wv[0] = w0.x; wv[1] = w0.y; wv[2] = w1.x; wv[3] = w1.y;
      if (kb < whole) {
        if (pass == 1) ned_slide_block<EDGE, 1>(v, wv, kb, 4, klo, khi, a, b, bg, c);
        else ned_slide_block<EDGE, 2>(v, wv, kb, 4, klo, khi, a, b, bg, c);
      } else {
        if (pass == 1) ned_slide_block<EDGE, 1>(v, wv, kb, g.w - whole, klo, khi, a, b, bg, c);
        else ned_slide_block<EDGE, 2>(v, wv, kb, g.w - whole, klo, khi, a, b, bg, c);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = v[4 + r];
    }
    if (pass == 1) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (!EDGE) a[r] = a[0];
        bg[r] = b[r] * (1.0 + 0x1p-32);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (p0 + r >= npos) continue;
    float val;
    if (!(fabs(b[r]) <= 1.7976931348623157e308)) val = ned_nan(IRA_NED_NAN_NONFINITE);
    else if (b[r] == 0.0) val = ned_nan(IRA_NED_NAN_SILENT);
    else val = (float)((c[r] / a[r]) / 0.31731050786291415);
    out[p0 + r] = val;
  }
}

template <bool UNIT>
__device__ __forceinline__ void ned_walk(const NedChannel& ch, const NedGeom& g, double* h2, const double* wl,
                                         float* __restrict__ row) {
  const int t = threadIdx.x;
  const int64_t tiles = (ch.room + g.tile - 1) / g.tile;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t j0 = tile * g.tile;
    const int64_t left = ch.count - j0, room = ch.room - j0;
    const int npos = left <= 0 ? 0 : (left < g.tile ? (int)left : g.tile);
    const int nrow = room < g.tile ? (int)room : g.tile;
    for (int p = npos + t; p < nrow; p += NED_THREADS) row[j0 + p] = ned_nan(IRA_NED_NAN_SILENT);    // past K: NaN
    if (npos == 0) continue;
    const int64_t c0 = ch.onset + j0 * g.step;
    const int64_t i0 = c0 - g.delta;
    const int span = (npos - 1) * g.step + g.w;
    __syncthreads();                                         // the tile before has been read
    for (int u0 = t; u0 < span; u0 += NED_STAGE * NED_THREADS) {          // NED_STAGE loads in flight per thread
      float xv[NED_STAGE];
#pragma unroll
      for (int q = 0; q < NED_STAGE; ++q) {
        const int u = u0 + q * NED_THREADS;
        const int64_t i = i0 + u;
        xv[q] = (u < span && i >= 0 && i < ch.len) ? ch.x[i] : 0.0f;
      }
#pragma unroll
      for (int q = 0; q < NED_STAGE; ++q) {
        const int u = u0 + q * NED_THREADS;
        const double d = (double)xv[q];
        if (u < span) h2[UNIT ? u : (u % g.sl) * g.p + u / g.sl] = d * d;
      }
    }
    __syncthreads();
    const bool edge = i0 < 0 || i0 + span > ch.len;
    float* out = row + j0;
    if (npos <= NED_THREADS) {
      if (edge) ned_tile<1, true, UNIT>(h2, wl, g, npos, c0, ch.len, out);
      else ned_tile<1, false, UNIT>(h2, wl, g, npos, c0, ch.len, out);
    } else if (UNIT && g.step == 1) {
      if (edge) ned_tile_slide<true>(h2, wl, g, npos, c0, ch.len, out);
      else ned_tile_slide<false>(h2, wl, g, npos, c0, ch.len, out);
    } else {
      if (edge) ned_tile<NED_ROUNDS, true, UNIT>(h2, wl, g, npos, c0, ch.len, out);
      else ned_tile<NED_ROUNDS, false, UNIT>(h2, wl, g, npos, c0, ch.len, out);
    }
  }
}

__global__ __launch_bounds__(NED_THREADS) void ned_profile_kernel(const float* __restrict__ x,
                                                                  const int64_t* __restrict__ off,
                                                                  const int64_t* __restrict__ len,
                                                                  const int64_t* __restrict__ onset,
                                                                  const double* __restrict__ w, NedGeom g, int slots,
                                                                  float* __restrict__ prof,
                                                                  const int64_t* __restrict__ prof_off) {
  extern __shared__ __attribute__((aligned(16))) double ned_lds[];
  double* h2 = ned_lds;
  double* wl = ned_lds + slots;
  const int c = blockIdx.y;
  const NedChannel ch = ned_channel(x, off, len, onset, c, g.step, g.kmax);
  if ((int64_t)blockIdx.x * g.tile >= ch.room) return;       // the whole workgroup: no tile is its own
  for (int k = threadIdx.x; k < g.w; k += NED_THREADS) wl[k] = w[k];
  float* row = prof + ira::uniform(prof_off[c]);
  if (g.sl == 1) ned_walk<true>(ch, g, h2, wl, row);
  else ned_walk<false>(ch, g, h2, wl, row);
}

// (greater value, then smaller index) and (smaller index) are total orders: the tree's shape does not matter
__global__ __launch_bounds__(NED_THREADS) void ned_record_kernel(const int64_t* __restrict__ len,
                                                                 const int64_t* __restrict__ onset, int64_t step,
                                                                 int64_t kmax, NedThresholds thr, int nthr,
                                                                 const float* __restrict__ prof,
                                                                 const int64_t* __restrict__ prof_off,
                                                                 double* __restrict__ rec) {
  __shared__ float s_best[NED_WAVES];
  __shared__ long long s_idx[NED_WAVES], s_first[IRA_NED_MAX_THRESHOLDS][NED_WAVES], s_cnt[2][NED_WAVES];
  const int c = blockIdx.x, t = threadIdx.x;
  int64_t n = ira::uniform(len[c]), o = ira::uniform(onset[c]);
  n = n > 0 ? n : 0;
  o = o > 0 ? o : 0;
  const int64_t count = ned_count(n, o, step, kmax);
  const float* row = prof + ira::uniform(prof_off[c]);
  const long long none = INT64_MAX;
  float best = -INFINITY;
  long long idx = none, first[IRA_NED_MAX_THRESHOLDS], silent = 0, nonfinite = 0;
#pragma unroll
  for (int q = 0; q < IRA_NED_MAX_THRESHOLDS; ++q) first[q] = none;
  for (int64_t j = t; j < count; j += NED_THREADS) {
    const float v = row[j];
    if (v != v) {
      if (__float_as_uint(v) == IRA_NED_NAN_NONFINITE) ++nonfinite; else ++silent;
      continue;
    }
    if (idx == none || v > best) { best = v; idx = j; }      // j ascends: the first index of the thread's maximum
#pragma unroll
    for (int q = 0; q < IRA_NED_MAX_THRESHOLDS; ++q)
      if (q < nthr && first[q] == none && (double)v >= thr.v[q]) first[q] = j;
  }
  // not ira::wave_argmax: a lane that saw no finite value carries idx == none and must lose whatever its `best`
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    const float ob = __shfl_xor(best, s, 64);
    const long long oi = __shfl_xor(idx, s, 64);
    if (oi != none && (idx == none || ob > best || (ob == best && oi < idx))) { best = ob; idx = oi; }
#pragma unroll
    for (int q = 0; q < IRA_NED_MAX_THRESHOLDS; ++q) {
      const long long of = __shfl_xor(first[q], s, 64);
      first[q] = of < first[q] ? of : first[q];
    }
    silent += __shfl_xor(silent, s, 64);
    nonfinite += __shfl_xor(nonfinite, s, 64);
  }
  if ((t & 63) == 0) {
    const int wv = t >> 6;
    s_best[wv] = best; s_idx[wv] = idx; s_cnt[0][wv] = silent; s_cnt[1][wv] = nonfinite;
#pragma unroll
    for (int q = 0; q < IRA_NED_MAX_THRESHOLDS; ++q) s_first[q][wv] = first[q];
  }
  __syncthreads();
  if (t == 0) {
    for (int wv = 1; wv < NED_WAVES; ++wv) {
      const float ob = s_best[wv];
      const long long oi = s_idx[wv];
      if (oi != none && (idx == none || ob > best || (ob == best && oi < idx))) { best = ob; idx = oi; }
      silent += s_cnt[0][wv];
      nonfinite += s_cnt[1][wv];
#pragma unroll
      for (int q = 0; q < IRA_NED_MAX_THRESHOLDS; ++q) first[q] = s_first[q][wv] < first[q] ? s_first[q][wv] : first[q];
    }
    double* r = rec + (int64_t)c * IRA_NED_DOUBLES;
    r[0] = (double)count;
    r[1] = (double)silent;
    r[2] = (double)nonfinite;
    r[3] = idx != none ? (double)best : __longlong_as_double(0x7ff8000000000000ll);
    r[4] = idx != none ? (double)idx : -1.0;
#pragma unroll
    for (int q = 0; q < IRA_NED_MAX_THRESHOLDS; ++q) r[5 + q] = (q < nthr && first[q] != none) ? (double)first[q] : -1.0;
  }
}

// Positions per tile and the layout of the staged span for (W, S): de-interleaved by S when at least one position fits
// that way, as it is otherwise.
NedGeom ned_geometry(int delta, int step, int64_t kmax) {
  NedGeom g;
  g.delta = delta;
  g.w = 2 * delta + 1;
  g.step = step;
  g.kmax = kmax;
  g.sl = 1;
  if (step > 1 && step <= NED_SLOTS) {
    const int wq = (g.w + step - 1) / step;                  // P = (T - 1 + ceil(W / S)) made odd, S P <= NED_SLOTS
    int t = NED_SLOTS / step - wq + 1;
    t = t < IRA_NED_TILE ? t : IRA_NED_TILE;
    while (t >= 1 && (int64_t)step * ((t - 1 + wq) | 1) > NED_SLOTS) --t;
    if (t >= 1) {
      g.sl = step;
      g.tile = t;
      g.p = (t - 1 + wq) | 1;
      g.pstride = 1;
      return g;
    }
  }
  const int64_t t = (NED_SLOTS - g.w) / (int64_t)step + 1;   // (T - 1) S + W <= NED_SLOTS
  g.tile = (int)(t < IRA_NED_TILE ? t : IRA_NED_TILE);
  g.p = 0;
  g.pstride = step;
  return g;
}

}  // namespace

extern "C" int32_t ira_echo_density(const float* x_dev, const int64_t* off_dev, const int64_t* len_dev,
                                    const int64_t* onset_dev, int32_t nch, const double* w_dev, int32_t delta,
                                    int32_t step, int64_t kmax, const double* thresholds, int32_t nthr, float* prof_dev,
                                    const int64_t* prof_off_dev, double* rec_dev, void* stream) {
  IRA_CHECK_PTR(x_dev); IRA_CHECK_PTR(off_dev); IRA_CHECK_PTR(len_dev); IRA_CHECK_PTR(onset_dev); IRA_CHECK_PTR(w_dev);
  IRA_CHECK_PTR(prof_dev); IRA_CHECK_PTR(prof_off_dev); IRA_CHECK_PTR(rec_dev);
  if (delta < 1 || delta > IRA_NED_MAX_DELTA || step < 1) return IRA_E_SIZE;
  if (kmax < 0 || kmax > NED_MAX_COUNT) return IRA_E_SIZE;
  if (nthr < 0 || nthr > IRA_NED_MAX_THRESHOLDS) return IRA_E_SIZE;
  if (nthr > 0) IRA_CHECK_PTR(thresholds);
  NedThresholds thr;
  for (int q = 0; q < IRA_NED_MAX_THRESHOLDS; ++q) {
    thr.v[q] = q < nthr ? thresholds[q] : 0.0;
    if (!isfinite(thr.v[q])) return IRA_E_SIZE;
  }
  if (nch < 0 || nch > 65535) return IRA_E_SIZE;
  if (nch == 0) return IRA_OK;
  hipStream_t st = (hipStream_t)stream;
  const NedGeom g = ned_geometry(delta, step, kmax);
  // the squares, then the weights at a 16-byte boundary; ned_tile_slide reads (and drops) up to 8 squares and 3 weights
  // past the ones it uses
  const int slots = ((g.sl == 1 ? (g.tile - 1) * step + g.w : g.sl * g.p) + NED_SLIDE_PAD + 1) & ~1;
  const size_t lds = (size_t)(slots + g.w + 4) * sizeof(double);
  IRA_TRY_HIP(allow_lds(ned_profile_kernel, lds));
  // enough workgroups to fill the device whatever the batch; a channel's tiles are dealt over its blockIdx.x
  int64_t gx = (kmax + g.tile - 1) / g.tile;
  const int64_t want = (4096 + nch - 1) / nch;
  gx = gx < want ? gx : want;
  gx = gx < 1 ? 1 : (gx > NED_MAX_GRID_X ? NED_MAX_GRID_X : gx);
  ned_profile_kernel<<<dim3((unsigned)gx, nch), NED_THREADS, lds, st>>>(x_dev, off_dev, len_dev, onset_dev, w_dev, g,
                                                                         slots, prof_dev, prof_off_dev);
  ned_record_kernel<<<nch, NED_THREADS, 0, st>>>(len_dev, onset_dev, step, kmax, thr, nthr, prof_dev, prof_off_dev,
                                                 rec_dev);
  IRA_RETURN_LAUNCH();
}
