// stft5_kernel: the float64 / n_fft = 8192 STFT (the reference's modal-cloud default, modalcloud.py:121-158) with ONE FRAME
// ON FOUR WAVES (256 lanes, 16 complex values per lane), KF5 consecutive frames of a segment per workgroup: frame-major
// (T, F) dB output, or (ira_stft_logbin) the modal cloud's log-bin aggregation fused in.
// Transform: packed real FFT, z[n] = xw[2n] + i xw[2n+1], M = 4096 = 16 * 16 * 16, DIF, n = n1*256 + n2*16 + n3,
// k = k1 + 16 k2 + 256 k3:
//   step 1  lane m = q: 16-point DFT over n1 from global memory, twiddle W_M^(k1 m)
//   E1      lanes 0..127 write [16 k1][128 m'] (stride 129), all lanes read n2 = 0..7 at (k1 = q & 15, n3 = q >> 4);
//           then lanes 128..255 write and all read n2 = 8..15
//   step 2  16-point DFT over n2, twiddle W_M^(16 k2 n3)
//   E2      lanes with n3 < 8 (q < 128) write k1 + 16 k2 + 256 n3, lane r = q = k1 + 16 k2 reads n3 = 0..7; then n3 >= 8
//   step 3  16-point DFT over n3 -> lane r holds Z[r + 256 k3]
//   E3      the mirror partners Z[M - k] of the lane's bins k = q + 256 i, i < 8
//   post    (Z[k], Z[M-k]) -> |X[k]|, |X[M-k]| in dB (table log2, ira_log.h), stored at out[t*F + k]; or linear magnitudes
//           -> log-bin means
// QUIET FRAMES skip the transform.  While step 1 forms the windowed samples it also sums their squares; |X[k]|^2 <= N sum(xw)^2
// for every bin, so a frame with 4 N sum(xw)^2 <= floor^2 is floored on every row: it stores the floor (dB mode) or hands
// the aggregation the floored linear value (log-bin mode) -- the very bytes the full path would have produced, for the
// price of the loads, one reduction and one barrier.  The decaying tails of impulse responses are such frames.
// QUIET CHUNKS skip even that.  Without a frame selection a workgroup's frames are consecutive, and sum (x w)^2 over any of
// them is at most max(w^2) times sum x^2 over the chunk's whole sample span: one pass over the span (11 776 samples for
// eight frames at hop 512, against 8 x 8192 samples and as many window values) certifies all of them at once, and the
// workgroup stores its floored values without a frame loop.  In log-bin mode the value a floored frame leaves in a log bin
// depends on the bin alone: a quiet frame of an uncertified chunk takes it from a table the workgroup's first quiet frame
// builds (quiet_val) instead of summing the same constant again.
// QUIET SUFFIXES skip the pass as well.  What is quiet in an impulse response is a suffix of it: a launch that is given the
// suffix energies of ira_tail_energy (ira_tailenergy.hip) tests a chunk with ONE load -- 4 N max(w^2) S[j] <= floor^2, j the
// 512-sample block its first frame starts in -- before it builds anything, and copies a floored row that
// stft5_consts_kernel formed once for the launch; a chunk the table does not certify goes to the frame loop without a span
// pass.  Without the table the kernel is what it was.
// 16-byte LDS accesses are served a quarter wave at a time: in every exchange the 16 lanes of a quarter differ in k1
// (or in consecutive m), which the strides 129 and 1 map to distinct 16-byte bank groups: conflict free.
// Why four waves per frame (profiles/r02_stft4_counters.txt): with two waves per frame (32 values per lane, 228 VGPRs, two
// waves per SIMD) the SIMDs' float64 pipes were busy 60 % of the time.  The frame's LDS budget (one half-size exchange
// buffer, 33 KB) does not depend on how many lanes share it, the register budget does: 16 values per lane fit ~128 VGPRs,
// so four frames per CU bring 16 waves and a wave that waits at a barrier has three others on its SIMD to cover for it.
#include <cmath>
#include <cstdlib>

#include "ira_fft_reg.h"
#include "ira_log.h"
#include "ira_stft.h"

namespace {

using ira::brev_bits;
using ira::cplx;
using ira::dft_dif;
using ira::powers16;

typedef cplx<double> cdd;

constexpr int M4 = 4096, F4 = M4 + 1, TL4 = 128;   // TL4: the lanes that fill one half-size E1 / E2 buffer
constexpr int ROW4 = 129;                 // E1 half: row stride (complex)
constexpr int E2N4 = 256;                 // E2 half: n3' stride (complex)
constexpr int EXC4 = 16 * ROW4;           // complex slots per workgroup: max(16*129, 8*256, 4096 doubles / 2)
static_assert(EXC4 >= 8 * E2N4 && EXC4 * 2 >= M4, "exchange buffer too small");

__device__ __forceinline__ float db_of4(double re, double im, double floor_pow, float floor_db,
                                        const ira::LogTabEntry* tab) {
  // |X| <= 8192 * max|x| < 3e42 for float32 samples, so p < 1e85 is always a normal double unless the frame holds an
  // infinity or a NaN -- and those frames are flagged as a whole (bad_frame) and never reach this value.  (Round 2 carried
  // a hypot + log10 path for p >= 1e300 here: dead for this kernel's inputs, and 40 % of its code size.)
  const double p = fma(re, re, im * im);
  if (!(p > floor_pow)) return floor_db;                                       // also catches NaN
  return (float)(3.0102999566398120 * ira::log2_table<4>(p, tab));
}

// Linear magnitude the reference's aggregation starts from: 10^(float32(dB)/20) with dB = 20 log10 max(|X|, floor)
// (modalcloud.py:186-190 applied to the float32 STFT of :150-156).  With dB = 10 log10 p in float64 and d = float32(dB) - dB
// (|d| <= 4e-6 dB) this is sqrt(p) * 10^(d/20) = sqrt(p) (1 + t + t^2/2), t = d ln(10)/20 <= 5e-7 (next term 2e-20):
// a square root and two fused multiply-adds instead of a float64 exp10 (~50 instructions), same value to ~1e-15.
__device__ __forceinline__ double lin_of4(double re, double im, double floor_pow, float floor_db, double floor_lin32,
                                          const ira::LogTabEntry* tab) {
  const double p = fma(re, re, im * im);
  if (!(p > floor_pow)) return floor_lin32;                                    // also catches NaN, like db_of4
  const double db = 3.0102999566398120 * ira::log2_table<4>(p, tab);           // (p < 1e85: see db_of4)
  const double t = ((double)(float)db - db) * 0.11512925464970228;
  // sqrt(p) for a normal p (floor_pow < p < 1e85: no scaling needed): hardware reciprocal square root (~26 bits) and ONE
  // coupled Newton step (Goldschmidt form): relative error 1.5 e0^2 ~ 3e-16 -- the mean of these values is rounded to a
  // float32 dB value, 1e-12 would do (round 2 ran two steps).  6 instructions instead of the ~25 of the library sqrt.
  const double y0 = __builtin_amdgcn_rsq(p);
  double g = p * y0;
  const double h = 0.5 * y0;
  const double r = fma(-h, g, 0.5);
  g = fma(g, r, g);
  return g * fma(t, fma(t, 0.5, 1.0), 1.0);
}

// Log bin -> float32 dB: the mean of the bin's c rows r[0 .. c), added in ascending order, -> 20 log10(max(., 1e-30)).
// CONST: every row holds the value cst (a floored frame), r is not read.  Both forms perform the same additions in the
// same order -- the sum of c copies of cst is formed by c - 1 additions, not by a product -- so a floored frame gets the
// bits the sum over the exchange buffer would have given it.
template <bool CONST>
__device__ __forceinline__ float logbin_mean_db(const double* r, double cst, int c, const ira::LogTabEntry* tab) {
  double acc = CONST ? cst : r[0];
  for (int k0 = 1; k0 < c; k0 += 8) {
    double v8[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v8[u] = (k0 + u < c) ? (CONST ? cst : r[k0 + u]) : 0.0;
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (k0 + u < c) acc += v8[u];
  }
  // 20 log10 m through the table log2 (series to r^6: a few 1e-16 relative, invisible after the float32 rounding) --
  // the library log10 was ~130 of the ~1800 instructions of every wave although only 240 lanes of a frame use it
  return (float)(6.0205999132796239 * ira::log2_table<6>(fmax(acc / (double)c, 1e-30), tab));
}

constexpr int TL5 = 256;
// Frames per workgroup (tuning build: IRA_STFT5_K).  Measured on the report step and on the kernel alone at 2, 4, 8, 16
// (profiles/stft5_chunks_ab.txt): 8 is the fastest on both.  It amortises 7/8 of the per-workgroup set-up; at 16 the
// coarser tail of the launch (14.5 rounds of the 1024 resident workgroups) costs more than the last sixteenth saves.
constexpr int KF5 = 8;

// Two neighbouring samples / window values in one load.  A frame starts at any sample (segment offset + peak index +
// frame * hop), so a sample pair is 4-byte aligned only; the window table is only known to be a double array.
struct __attribute__((aligned(4))) fpair5 { float a, b; };
struct __attribute__((aligned(8))) dpair5 { double a, b; };
typedef float fquad5 __attribute__((ext_vector_type(4), aligned(4)));   // four samples of a span that starts at any sample
// The chunk test is made where the chunk's sample span is at most this many samples: twice n_fft, hop <= 1170 at eight
// frames.  The bound holds at any hop, but the longer the span the less of it each frame holds: the pass over it costs a
// loud chunk more and certifies fewer quiet ones (from hop = n_fft on it reads the gaps between the frames as well).
constexpr int64_t SPAN5_MAX = 2 * (2 * M4);

// What a launch with a suffix-energy table needs of its window table and its log bins, worked out ONCE per launch by
// stft5_consts_kernel instead of by every certified workgroup: the greatest w^2 and the log-bin row of a floored frame.
// Layout of the caller's scratch (IRA_STFT_CONSTS_DOUBLES): the double, then lb_nbins floats.
struct Stft5Consts {
  double wmax2;
  float row[1];                                    // lb_nbins values (none in dB mode)
};

// The greatest w^2 of the window table, taken over the bit patterns of |w^2|, which order like the values and put every
// NaN above infinity: a NaN in the table comes out as a NaN (and certifies nothing).  A maximum: whatever order the lanes
// visit the table in, the bits are the same.  wmax (one slot per wave) is LDS; ends behind a barrier.
__device__ __forceinline__ double window_max_sq5(const double* __restrict__ window, int q, unsigned long long* wmax) {
  unsigned long long wb = 0;
#pragma unroll
  for (int j = 0; j < 2 * M4 / (2 * TL5); ++j) {
    const dpair5 w = *reinterpret_cast<const dpair5*>(window + 2 * (j * TL5 + q));
    const unsigned long long ba = (unsigned long long)__double_as_longlong(w.a * w.a) & 0x7fffffffffffffffull;
    const unsigned long long bb = (unsigned long long)__double_as_longlong(w.b * w.b) & 0x7fffffffffffffffull;
    wb = ba > wb ? ba : wb;
    wb = bb > wb ? bb : wb;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(wb, o, 64);
    wb = other > wb ? other : wb;
  }
  if ((q & 63) == 0) wmax[q >> 6] = wb;
  __syncthreads();
  unsigned long long wm = wmax[0];
#pragma unroll
  for (int i = 1; i < TL5 / 64; ++i) wm = wmax[i] > wm ? wmax[i] : wm;
  return ira::uniform(__longlong_as_double((long long)wm));
}

// One workgroup per launch.  row[bb] is what stft5_kernel's quiet_bin gives log bin bb of a floored frame: the same
// function of the same float floor_db on the same table, so the same bytes.
__global__ __launch_bounds__(TL5) void stft5_consts_kernel(const double* __restrict__ window, float floor_db, int lb_nbins,
                                                           const int32_t* __restrict__ lb_count, Stft5Consts* __restrict__ cst) {
  __shared__ unsigned long long wmax[TL5 / 64];
  __shared__ ira::LogTabEntry ltab[ira::LOGTAB_N];
  const int q = threadIdx.x;
  ira::build_log_table(ltab, q);
  const double wmax2 = window_max_sq5(window, q, wmax);          // its barrier also publishes ltab
  if (q == 0) cst->wmax2 = wmax2;
  const double floor_lin32 = ira::uniform(exp10((double)floor_db * 0.05));
  for (int bb = q; bb < lb_nbins; bb += TL5) {
    const int c = lb_count[bb];
    cst->row[bb] = c > 0 ? logbin_mean_db<true>(nullptr, floor_lin32, c, ltab) : __uint_as_float(0x7fc00000u);
  }
}

// One workgroup transforms kfr CONSECUTIVE frames of one segment, one after the other.  Everything that does not depend on
// the frame is done once, before the frame loop: the XCD remap and (segment, chunk) decode, the segment's job values (as
// scalars), the log2 table in LDS, the hull of the log bins and 10^(floor/20).  Only scalar state lives across the loop:
// the frame's twiddle factors are reloaded per frame (they hit the caches), the frame alone needs 122 of the 128 VGPRs.
// The loop body is the frame as described at the top of the file, barrier for barrier, behind one more barrier at which
// the waves agree whether the frame is quiet; its trip count and that decision are workgroup-uniform, so every wave of
// the workgroup meets the same barriers.  Before the loop the workgroup tests its whole chunk once ("quiet chunk?"): where
// that certifies all of its frames there is no loop.  The results do not depend on kfr: a frame's arithmetic reads nothing
// of its neighbours, and a frame the chunk test certifies gets the bytes its own arithmetic would have produced.
__global__ __launch_bounds__(TL5) __attribute__((amdgpu_waves_per_eu(4, 4))) void stft5_kernel(
    const float* __restrict__ x, const int64_t* __restrict__ off, const int32_t* __restrict__ nframes, int hop,
    const double* __restrict__ window, const cdd* __restrict__ tw, double floor_lin, float floor_db,
    float* __restrict__ out, const int64_t* __restrict__ out_off, const int32_t* __restrict__ frame_sel,
    const int64_t* __restrict__ sel_off, int lb_nbins, int lb_kbase, const int32_t* __restrict__ lb_first,
    const int32_t* __restrict__ lb_count, int kfr, int ablate, const double* __restrict__ tail,
    const int64_t* __restrict__ tail_off, const Stft5Consts* __restrict__ cst) {
  // ablate (IRA_STFT5_ABLATE, tuning build, timing only): 1 no window loads, 2 no sample loads, 4 no dB -> linear conversion;
  // results unchanged (tests and A/B): 256 every frame takes the full path -- the quiet-frame rule, the chunk test (table
  // test included) and the quiet table are all off; 512 the chunk test (table test included) alone is off; 1024 the quiet
  // table alone is off (a quiet frame fills the exchange buffer with the floored value and sums it like a loud one)
  __shared__ __attribute__((aligned(16))) cdd ex[EXC4];
  __shared__ double wave_energy[2][TL5 / 64];      // per-wave sums of (xw)^2, one slot per frame parity
  __shared__ double chunk_energy[TL5 / 64];        // per-wave sums of x^2 over the chunk's span (written once, before the loop)
  __shared__ unsigned long long chunk_wmax[TL5 / 64];   // per-wave max of w^2, as bit patterns
  __shared__ float quiet_val[TL5];                 // log bin q of a floored frame, kept by lane q for lane q (no barrier)
  __shared__ ira::LogTabEntry ltab[ira::LOGTAB_N];
  __shared__ int lb_range[2];
  __shared__ int frame_bad;
  // XCD-aware remap: the workgroups of one XCD take a contiguous run of chunks, so that neighbouring chunks, whose frames
  // overlap, share an L2
  unsigned bx, by;
  ira::xcd_remap(bx, by);
  const int seg = (int)by;
  const int col0 = (int)bx * kfr;
  const int T_out = ira::uniform(nframes[seg]);
  if (col0 >= T_out) return;                       // the whole workgroup, before its first barrier
  const int col1 = T_out - col0 < kfr ? T_out : col0 + kfr;
  int q = threadIdx.x;
  float* os = out + ira::uniform(out_off[seg]);
  const double floor_pow = floor_lin * floor_lin;

  // ---- quiet suffix? (a launch with a suffix-energy table and no frame selection) -------------------------------------
  // The table's S[j] is the sum of x^2 from block j (512 samples) of THIS segment to the end of its channel (ira_tail_energy;
  // the caller's contract: the table's segments start where these do, and no frame reads past the channel's end).  The
  // chunk's first frame starts at sample col0 hop, inside block j = col0 hop / 512, and frames are consecutive: every
  // sample the chunk reads is one of those S[j] sums, so for each of its frames
  //   sum (x w)^2 <= wmax2 sum x^2 <= wmax2 S_exact[j].
  // S[j] is a float64 sum of at most a few million non-negative terms (480 000 for ten seconds) in trees no deeper than a
  // few dozen additions: S_exact <= S[j] (1 + 1e-13), far inside the factor 4 the per-frame rule below keeps over the
  // transform's own rounding.  So 4 N wmax2 S[j] <= floor^2 puts every frame of the chunk under that rule, as the span
  // pass further down does -- for ONE load, before the log table, the hull and any barrier; the frames get the floor (dB
  // mode) or the floored log-bin row stft5_consts_kernel formed with quiet_bin's arithmetic, the bytes the frame loop
  // gives a floored frame.  A suffix holds more than the chunk's span, so the test certifies a little later in a decay
  // than the span pass; what it misses the per-frame rule still finds.  A NaN or an infinity from the chunk on makes
  // S[j] non-finite, a NaN in the window makes wmax2 one: the comparison is false.  Workgroup-uniform (launch arguments
  // and values read through ira::uniform): either every wave leaves here or none.
  // A chunk the table does not certify goes straight to the frame loop: it does not pay the span pass as well.
  const bool use_tail = tail != nullptr && frame_sel == nullptr && !IRA_ABL(ablate & (256 | 512));
  if (use_tail) {
    const int64_t j = ((int64_t)col0 * hop) / IRA_TAIL_BLOCK;
    const double S = ira::uniform(tail[ira::uniform(tail_off[seg]) + j]);
    const double wmax2 = ira::uniform(cst->wmax2);
    if (S * (4.0 * (2 * M4)) * wmax2 <= floor_pow) {
      const int nfr = col1 - col0;
      if (lb_nbins <= 0) {
        float* fo = os + (int64_t)col0 * F4;
        for (int i = q; i < nfr * F4; i += TL5) fo[i] = floor_db;
      } else {
        for (int bb = q; bb < lb_nbins; bb += TL5) {
          const float val = cst->row[bb];
          float* o = os + (int64_t)bb * T_out + col0;
          for (int jf = 0; jf < nfr; ++jf) o[jf] = val;
        }
      }
      return;
    }
  }

  double* exd = reinterpret_cast<double*>(ex);
  ira::build_log_table(ltab, q);
  if (q < 2) lb_range[q] = q == 0 ? F4 : 0;

  const float* xs = x + ira::uniform(off[seg]);
  const int32_t* fsel = frame_sel ? frame_sel + ira::uniform(sel_off[seg]) : nullptr;
  const float qnan32 = __uint_as_float(0x7fc00000u);
  // Log-bin mode: the hull [k_lo, k_hi) of the rows some log bin reads, and the linear value of a floored row.  Only the
  // hull's rows are converted: 20 Hz .. 20 kHz is rows 4 .. 3413 of 4097, a sixth of the conversions (the costliest part
  // of the frame) is skipped.
  int k_lo = 0, k_hi = 0;
  double floor_lin32 = 0.0;
  __syncthreads();                                 // lb_range initialised
  if (lb_nbins > 0) {
    int lo = F4, hi = 0;
    for (int bb = q; bb < lb_nbins; bb += TL5) {
      const int c = lb_count[bb];
      if (c > 0) {
        const int f0 = lb_kbase + lb_first[bb];
        lo = f0 < lo ? f0 : lo;
        hi = f0 + c > hi ? f0 + c : hi;
      }
    }
    atomicMin(&lb_range[0], lo);
    atomicMax(&lb_range[1], hi);
    __syncthreads();
    k_lo = ira::uniform(lb_range[0]);
    k_hi = ira::uniform(lb_range[1]);
    floor_lin32 = ira::uniform(exp10((double)floor_db * 0.05));
  }
  // Log bin bb of a frame that is floored on every row: what the sums at the loop's tail make of the floored linear value
  // (the same additions, see logbin_mean_db), or the NaN of an empty bin.
  auto quiet_bin = [&](int bb, double fl) -> float {
    const int c = lb_count[bb];
    return c > 0 ? logbin_mean_db<true>(nullptr, fl, c, ltab) : qnan32;
  };

  // ---- quiet chunk? ------------------------------------------------------------------------------------------------
  // Without a frame selection the chunk's frames are consecutive and read the samples [col0 hop, (col1 - 1) hop + N) of the
  // segment and nothing else.  For each of them sum (x w)^2 <= max(w^2) sum x^2 <= wmax2 S, S the sum of x^2 over that
  // span, so 4 N wmax2 S <= floor^2 puts every frame of the chunk under the per-frame rule of the loop below ("quiet
  // frame?"; the float64 rounding of S, ~1e-13 relative, disappears in that rule's factor 4).  Their output is known: the
  // floor on every row, or the floored value's log-bin means.  The pass reads exactly the span -- the last segment of a batch
  // may end where the buffer ends -- in 16-byte pieces that are 4-byte aligned, like the frames' own pairs.
  // wmax2 is the maximum over the window table this call was given (a table scaled above 1 must not certify more), and only
  // chunks whose S passes a 16 times wider pre-test pay for it: a loud chunk pays the pass over the span, one reduction and
  // one barrier.  A NaN or an infinity in the span makes S non-finite and both comparisons false; the chunk then takes the
  // frame loop, which finds the frames that hold it.  The maximum is taken over the bit patterns of |w^2|, which order like
  // the values and put every NaN above infinity: a NaN in the table comes out as a NaN and certifies nothing either.
  // Every branch here is workgroup-uniform (launch arguments, values read back through ira::uniform from LDS that all lanes
  // read alike), so all four waves meet the same barriers; a certified chunk leaves behind its last one.
  // The decision may differ from K to K, the bytes do not: a certified frame gets what the loop would have given it.
  // A launch with a suffix-energy table has made its test above and does not pass over the span.
  if (!use_tail && !IRA_ABL(ablate & (256 | 512)) && fsel == nullptr && (int64_t)(col1 - col0 - 1) * hop + 2 * M4 <= SPAN5_MAX) {
    const int nfr = col1 - col0;
    const int span = (nfr - 1) * hop + 2 * M4;
    const float* cx = xs + (int64_t)col0 * hop;
    const int n4 = span >> 2;
    double s = 0.0;
    for (int i0 = 0; i0 < n4; i0 += 4 * TL5) {
      fquad5 p[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + u * TL5 + q;
        p[u] = i < n4 ? *reinterpret_cast<const fquad5*>(cx + 4 * i) : fquad5{0.0f, 0.0f, 0.0f, 0.0f};
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        s = fma((double)p[u].x, (double)p[u].x, s);
        s = fma((double)p[u].y, (double)p[u].y, s);
        s = fma((double)p[u].z, (double)p[u].z, s);
        s = fma((double)p[u].w, (double)p[u].w, s);
      }
    }
    if (q < (span & 3)) {                          // the span's last one to three samples
      const double t = (double)cx[4 * n4 + q];
      s = fma(t, t, s);
    }
    {
      const double wsum = ira::wave_sum(s);
      if ((q & 63) == 0) chunk_energy[q >> 6] = wsum;
    }
    __syncthreads();
    const double scaled = ira::uniform((chunk_energy[0] + chunk_energy[1]) + (chunk_energy[2] + chunk_energy[3])) * (4.0 * (2 * M4));
    if (scaled <= 16.0 * floor_pow) {
      const double wmax2 = window_max_sq5(window, q, chunk_wmax);
      if (scaled * wmax2 <= floor_pow) {
        if (lb_nbins <= 0) {
          // dB mode: the chunk's frames are one run of nfr * 4097 floats of the frame-major matrix
          float* fo = os + (int64_t)col0 * F4;
          for (int i = q; i < nfr * F4; i += TL5) fo[i] = floor_db;
        } else {
          // log-bin mode: lane bb writes its bin's run of nfr consecutive frames
          for (int bb = q; bb < lb_nbins; bb += TL5) {
            const float val = quiet_bin(bb, floor_lin32);
            float* o = os + (int64_t)bb * T_out + col0;
            for (int j = 0; j < nfr; ++j) o[j] = val;
          }
        }
        return;
      }
    }
  }
  bool quiet_built = false;                        // workgroup-uniform: quiet_val holds this workgroup's table

  for (int col = col0; col < col1; ++col) {
    // The lane index passes through an empty asm statement in every frame, so that the compiler derives the lane's
    // addresses, twiddle factors and masks inside the frame, as a one-frame kernel does.  Hoisted out of the loop they
    // stay live across it, and the frame (122 of the 128 VGPRs that four waves per SIMD allow) has no room for them.
    asm volatile("" : "+v"(q));
    const int k1l = q & 15, n3l = q >> 4;          // step-2 role: (k1, n3)
    const bool lower = q < TL4;                    // lanes whose step-1 / step-2 results go through the buffer first
    const int64_t frame = fsel ? (int64_t)ira::uniform(fsel[col]) : (int64_t)col;
    const float* fx = xs + frame * hop;
    // The eight wave-uniform factors W_N^(256 i) of the post step, requested HERE: they compile to scalar loads, and placed
    // at their use each one stalled its wave for a scalar-cache round trip (s_waitcnt lgkmcnt(0), which also drains the LDS
    // queue) in the middle of the conversion loop.  Loaded per frame (their index passes through an empty asm statement):
    // 32 scalar registers held across the loop would spill.
    int u0 = 0;
    asm volatile("" : "+s"(u0));
    cdd wuni[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) wuni[i] = tw[TL5 * i + u0];

    // ---- step 1 -----------------------------------------------------------------------------------------------
    cdd v[16];
    double energy = 0.0;                           // the lane's share of sum (xw[n])^2, added where the products are made
    {
      float xa[16], xb[16];
      double wa[16], wb[16];
#pragma unroll
      for (int n1 = 0; n1 < 16; ++n1) {
        const int n = n1 * 256 + q;
        if (IRA_ABL(ablate & 2)) { xa[n1] = (float)(n & 7) * 0.125f; xb[n1] = (float)(q & 3); }
        else { const fpair5 p = *reinterpret_cast<const fpair5*>(fx + 2 * n); xa[n1] = p.a; xb[n1] = p.b; }
        if (IRA_ABL(ablate & 1)) { wa[n1] = 0.5 + 1e-4 * n1; wb[n1] = 0.25; }
        else { const dpair5 w = *reinterpret_cast<const dpair5*>(window + 2 * n); wa[n1] = w.a; wb[n1] = w.b; }
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int n1 = 0; n1 < 16; ++n1) {
        v[n1] = {(double)xa[n1] * wa[n1], (double)xb[n1] * wb[n1]};
        energy = fma(v[n1].re, v[n1].re, energy);
        energy = fma(v[n1].im, v[n1].im, energy);
      }
    }

    // ---- quiet frame? ---------------------------------------------------------------------------------------------
    // Every bin obeys |X[k]|^2 <= N sum (xw[n])^2 (triangle inequality, then Cauchy-Schwarz; N = 8192).  When four times
    // that bound (6 dB over the transform's float64 rounding, ~1e-13 of the bound) is at or under the floor, db_of4 and
    // lin_of4 would take their floored branch on every row: the frame's output is known here, before any butterfly.  The
    // bound is over the windowed values themselves and assumes nothing about the window table.  A NaN or an infinity makes
    // the sum non-finite and the comparison false: such a frame takes the full path and its bad_frame handling.
    // The waves' sums meet in wave_energy[frame parity]; every lane reads back the same four doubles and adds them in the
    // same order, so the decision is the same in all four waves and they meet the same barriers.  Two slots because the
    // quiet path (either mode) has no barrier behind it: a fast wave writes the NEXT frame's slot while a slow one still reads
    // this one's.  The barrier below orders a slot's writes before its reads in this frame, and its reads in this frame
    // before its next writes two frames on (the next frame's barrier lies between them).
    double* we = wave_energy[col & 1];
    {
      const double wsum = ira::wave_sum(energy);
      if ((q & 63) == 0) we[q >> 6] = wsum;
    }
    __syncthreads();
    const double frame_energy = ira::uniform((we[0] + we[1]) + (we[2] + we[3]));
    const bool quiet = !IRA_ABL(ablate & 256) && frame_energy * (4.0 * (2 * M4)) <= floor_pow;

    bool bad_frame = false;                        // a quiet frame holds finite samples only
    if (quiet) {
      if (lb_nbins <= 0) {
        // dB mode: the floor on all 4097 rows, with the lane mapping of the loud frame's stores.  No LDS access here.
        float* fo = os + (int64_t)col * F4;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int k = q + TL5 * i;
          fo[k] = floor_db;
          fo[M4 - k] = floor_db;                                                   // k = 0 -> bin M
        }
        if (q == 0) fo[M4 / 2] = floor_db;
        continue;
      }
      // log-bin mode.  Every row of the frame holds the value lin_of4 gives a floored row, so log bin bb is a function of
      // lb_count[bb] alone: the workgroup's first quiet frame works it out (quiet_bin: the additions of the sums at the
      // loop's tail, over the constant) and lane q keeps bin q in quiet_val[q]; every later quiet frame stores from there.
      // No barrier: a slot of quiet_val is written and read by the same lane, in program order, and no other.  No LDS
      // access to the exchange buffer, so no barrier at the tail either, as in dB mode: what the previous loud frame's
      // sums read of it is fenced by that frame's own tail barrier, and wave_energy by its two slots (above).  Bins from
      // TL5 on (no caller has more than 240) are worked out frame by frame.
      // The value passes through an empty asm statement as a scalar: taken as a vector register pair it is held across
      // the frame loop for this path alone, and the loud frame has no pair to spare (the pair was spilled to scratch).
      double fl = floor_lin32;
      asm volatile("" : "+s"(fl));
      if (!IRA_ABL(ablate & 1024)) {
        if (!quiet_built) {
          if (q < lb_nbins) quiet_val[q] = quiet_bin(q, fl);
          quiet_built = true;
        }
        for (int bb = q; bb < lb_nbins; bb += TL5) os[(int64_t)bb * T_out + col] = bb < TL5 ? quiet_val[bb] : quiet_bin(bb, fl);
        continue;
      }
      // tuning build, bit 1024: the slots the post step fills, with the floored value; then the sums at the loop's tail
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int k = q + TL5 * i;
        if (k >= k_lo && k < k_hi) exd[k] = fl;
        if ((M4 - k) >= k_lo && (M4 - k) < k_hi) exd[M4 - k] = fl;
      }
      if (q == 0 && M4 / 2 >= k_lo && M4 / 2 < k_hi) exd[M4 / 2] = fl;
    } else {
      dft_dif<double, 16>(v);
      ira::twiddle16<double, true>(v, tw[2 * q]);                 // W_M^(k1 q) = W_N^(2 q k1), k1 at v[brev(k1)]

      // ---- E1: half-size exchange, lower lanes first --------------------------------------------------------------
      cdd b[16];
      if (lower) {
#pragma unroll
        for (int k1 = 0; k1 < 16; ++k1) ex[k1 * ROW4 + q] = v[brev_bits(k1, 4)];
      }
      __syncthreads();
#pragma unroll
      for (int n2 = 0; n2 < 8; ++n2) b[n2] = ex[k1l * ROW4 + n2 * 16 + n3l];
      __syncthreads();
      if (!lower) {
#pragma unroll
        for (int k1 = 0; k1 < 16; ++k1) ex[k1 * ROW4 + (q - TL4)] = v[brev_bits(k1, 4)];
      }
      __syncthreads();
#pragma unroll
      for (int n2 = 0; n2 < 8; ++n2) b[8 + n2] = ex[k1l * ROW4 + n2 * 16 + n3l];
      __syncthreads();

      // ---- step 2 and E2 -------------------------------------------------------------------------------------------
      dft_dif<double, 16>(b);
      ira::twiddle16<double, true>(b, tw[32 * n3l]);              // W_M^(16 k2 n3) = W_N^(32 n3 k2)
      if (lower) {                                                 // n3 < 8
#pragma unroll
        for (int k2 = 0; k2 < 16; ++k2) ex[k1l + 16 * k2 + E2N4 * n3l] = b[brev_bits(k2, 4)];
      }
      __syncthreads();
#pragma unroll
      for (int n3 = 0; n3 < 8; ++n3) v[n3] = ex[q + E2N4 * n3];
      __syncthreads();
      if (!lower) {
#pragma unroll
        for (int k2 = 0; k2 < 16; ++k2) ex[k1l + 16 * k2 + E2N4 * (n3l - 8)] = b[brev_bits(k2, 4)];
      }
      __syncthreads();
#pragma unroll
      for (int n3 = 0; n3 < 8; ++n3) v[8 + n3] = ex[q + E2N4 * n3];
      __syncthreads();

      // ---- step 3: lane r = q holds Z[r + 256 k3] at v[brev(k3)] --------------------------------------------------------
      dft_dif<double, 16>(v);

      // ---- E3: the mirror partners only.  The post step pairs Z[k] with Z[M - k]; lane q keeps k = q + 256 i, i < 8, which
      // it already holds (v[brev(i)]), and M - k = (256 - q) + 256 (15 - i) is entry k3 = 15 - i >= 8 of lane 256 - q: every
      // lane publishes its upper eight values and reads eight of its partner's -- 256 bytes per lane through LDS and one
      // barrier pair instead of the 512 bytes and two of the round-2 natural-order exchange (real parts, then imaginary
      // parts, own values included).  Lane 0 pairs with itself: M - 256 i = 256 (16 - i), its own entry 16 - i; i = 0 pairs
      // Z[0] with Z[0].
      double zkr[8], zpr[8], zki[8], zpi[8], midr, midi;
#pragma unroll
      for (int j = 0; j < 8; ++j) ex[j * TL5 + q] = v[brev_bits(8 + j, 4)];       // k3 = 8 + j
      __syncthreads();
      {
        const int partner = (TL5 - q) & (TL5 - 1);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          // partner entry k3 = 15 - i (slot 7 - i); lane 0: k3 = 16 - i (slot 8 - i), i = 0 -> Z[0] itself
          const int slot = q == 0 ? 8 - i : 7 - i;
          cdd zp = v[0];                                                             // Z[0] (lane 0, i = 0)
          if (!(q == 0 && i == 0)) zp = ex[slot * TL5 + partner];
          zkr[i] = v[brev_bits(i, 4)].re; zki[i] = v[brev_bits(i, 4)].im;
          zpr[i] = zp.re; zpi[i] = zp.im;
        }
      }
      {
        const cdd mid = ex[0];                                                       // Z[2048]: lane 0, k3 = 8
        midr = mid.re; midi = mid.im;
      }
      // A NaN (or infinite) sample anywhere in the frame makes every bin of numpy's rfft NaN (modalcloud.py:150): it shows
      // in Z[0] = sum of the packed inputs (lane 0, first pair; 0 * NaN at the Hann end points is NaN too).  One check per
      // frame, written by lane 0 for EVERY frame: the flag of a bad frame does not outlive it.
      if (q == 0) frame_bad = !((zkr[0] - zkr[0]) + (zki[0] - zki[0]) == 0.0) ? 1 : 0;
      __syncthreads();                                            // E3 fully read; frame_bad visible
      bad_frame = frame_bad != 0;

      // ---- post -------------------------------------------------------------------------------------------------
      const cdd wlane = tw[q];
      if (lb_nbins <= 0) {
        // no barrier at the loop's tail here: the next frame's first write to ex (E1; frame_bad is written later still)
        // follows the barrier above and the next frame's energy barrier, behind which this frame reads only the table;
        // wave_energy is ordered by its own barrier and its two slots (see "quiet frame?")
        float* fo = os + (int64_t)col * F4;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int k = q + TL5 * i;
          const cdd e = {0.5 * (zkr[i] + zpr[i]), 0.5 * (zki[i] - zpi[i])};
          const cdd d = {0.5 * (zkr[i] - zpr[i]), 0.5 * (zki[i] + zpi[i])};
          const cdd o = {d.im, -d.re};
          const cdd wk = ira::cmul(wlane, wuni[i]);              // W_N^k = W_N^q W_N^(256 i); second factor wave-uniform
          const cdd pp = ira::cmul(wk, o);
          fo[k] = bad_frame ? qnan32 : db_of4(e.re + pp.re, e.im + pp.im, floor_pow, floor_db, ltab);
          fo[M4 - k] = bad_frame ? qnan32 : db_of4(e.re - pp.re, e.im - pp.im, floor_pow, floor_db, ltab);   // k = 0 -> bin M
        }
        if (q == 0) fo[M4 / 2] = bad_frame ? qnan32 : db_of4(midr, midi, floor_pow, floor_db, ltab);
        continue;
      }
      // ---- fused modal-cloud aggregation (reference modalcloud.py:176-207): the frame's dB values never leave the CU.
      // float32 dB (the reference's STFT output type) -> linear magnitude 10^(dB/20) in float64 -> LDS; then log bin b is
      // the mean of its rows, added in ascending order, -> 20 log10(max(., 1e-30)) -> float32 at out[b * T + frame].
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int k = q + TL5 * i;
        const bool need_a = k >= k_lo && k < k_hi, need_b = (M4 - k) >= k_lo && (M4 - k) < k_hi;
        if (!need_a && !need_b) continue;
        const cdd e = {0.5 * (zkr[i] + zpr[i]), 0.5 * (zki[i] - zpi[i])};
        const cdd d = {0.5 * (zkr[i] - zpr[i]), 0.5 * (zki[i] + zpi[i])};
        const cdd o = {d.im, -d.re};
        const cdd wk = ira::cmul(wlane, wuni[i]);
        const cdd pp = ira::cmul(wk, o);
        if (IRA_ABL(ablate & 4)) {
          if (need_a) exd[k] = e.re + pp.re;
          if (need_b) exd[M4 - k] = e.im - pp.im;
          continue;
        }
        if (need_a) exd[k] = lin_of4(e.re + pp.re, e.im + pp.im, floor_pow, floor_db, floor_lin32, ltab);
        if (need_b) exd[M4 - k] = lin_of4(e.re - pp.re, e.im - pp.im, floor_pow, floor_db, floor_lin32, ltab);
      }
      if (q == 0 && M4 / 2 >= k_lo && M4 / 2 < k_hi) exd[M4 / 2] = lin_of4(midr, midi, floor_pow, floor_db, floor_lin32, ltab);
    }
    __syncthreads();
    for (int bb = q; bb < lb_nbins; bb += TL5) {
      const int c = lb_count[bb];
      float val = qnan32;
      if (c > 0) val = logbin_mean_db<false>(exd + lb_kbase + lb_first[bb], 0.0, c, ltab);
      os[(int64_t)bb * T_out + col] = (bad_frame && c > 0) ? qnan32 : val;
    }
    __syncthreads();                               // the sums have read the buffer the next frame's E1 (or quiet path) writes
  }
}

}  // namespace

int32_t ira_stft5_launch(const float* x, const int64_t* off, const int32_t* nframes, int32_t nseg, int32_t max_frames,
                         int32_t hop, const void* window, const void* tw, double floor_db, float* out,
                         const int64_t* out_off, const int32_t* frame_sel, const int64_t* sel_off, int32_t lb_nbins,
                         int32_t lb_kbase, const int32_t* lb_first, const int32_t* lb_count, const double* tail,
                         const int64_t* tail_off, void* consts, hipStream_t st) {
  const double floor_lin = std::pow(10.0, floor_db / 20.0);
  int kfr = ira_tune_int("IRA_STFT5_K", KF5);
  if (kfr < 1) kfr = 1;
  if (frame_sel != nullptr) tail = nullptr;        // selected frames are not consecutive: the table says nothing about them
  if (tail != nullptr) {
    if (tail_off == nullptr || consts == nullptr) return IRA_E_NULL;
    stft5_consts_kernel<<<1, TL5, 0, st>>>(static_cast<const double*>(window), (float)floor_db, lb_nbins > 0 ? lb_nbins : 0,
                                           lb_count, static_cast<Stft5Consts*>(consts));
    IRA_TRY_HIP(hipGetLastError());
  }
  dim3 grid((max_frames + kfr - 1) / kfr, nseg);
  stft5_kernel<<<grid, TL5, (size_t)ira_tune_int("IRA_STFT5_LDS_PAD", 0), st>>>(x, off, nframes, hop, static_cast<const double*>(window),
                                     static_cast<const cdd*>(tw), floor_lin, (float)floor_db, out, out_off, frame_sel,
                                     sel_off, lb_nbins, lb_kbase, lb_first, lb_count, kfr, ira_tune_int("IRA_STFT5_ABLATE", 0),
                                     tail, tail_off, static_cast<const Stft5Consts*>(consts));
  IRA_RETURN_LAUNCH();
}
