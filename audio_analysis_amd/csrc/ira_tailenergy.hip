// ira_tail_energy: float64 SUFFIX energies of sample segments, in blocks of IRA_TAIL_BLOCK = 512 samples.
//   S[j] = sum of x[n]^2 over n in [start + 512 j, end),  j < nblk = ceil((end - start) / 512);  S[nblk] = 0.
// What is quiet in an impulse response is a suffix of it: a reader that starts in block j of a segment and never reads past
// `end` sees only samples S[j] bounds, so one scalar load replaces a pass over those samples (the quiet-chunk test of
// stft5_kernel, ira_stft4.hip).  Nothing in the reference computes this table.
//   tail_block_kernel  (chunks x segments)  E[j] = the energy of block j alone, written where S[j] will stand
//   tail_scan_kernel   (1 wave / segment)   S[j] = E[j] + E[j + 1] + ... in place, from the end; S[nblk] = 0
// Bit-reproducible: a sample's square is exact in float64 (24-bit significands), lane l of a wave adds the samples
// 4 l .. 4 l + 3 and 256 + 4 l .. 256 + 4 l + 3 of its block in ascending order (fma on the exact square = one rounded
// addition), the lanes meet in the fixed butterfly of wave_sum, and the scan is a fixed Hillis-Steele tree per run of 64
// blocks with the runs chained from the end.  Which lane holds which sample never depends on the address: the 16-byte loads
// are declared 4-byte aligned (ira_reduce.h), a segment starts at any sample.  No atomics.
// A NaN or an infinity in block j makes E[j], and with it every S[i], i <= j, non-finite (squares are >= 0: no infinity
// meets its opposite); entries behind it sum only blocks behind it and stay what they were.  The last block is read up to
// `end` and no further: the last segment of a buffer may end where the buffer ends.
#include "ira_common.h"
#include "ira_reduce.h"

namespace {

using ira::f4u;

constexpr int TE_B = IRA_TAIL_BLOCK;
constexpr int TE_THREADS = 256;
constexpr int TE_WAVES = TE_THREADS / IRA_WAVE;
constexpr int TE_BPW = 4;                          // consecutive blocks per wave: eight 16-byte loads per lane in flight
constexpr int TE_CHUNK = TE_WAVES * TE_BPW;        // blocks per workgroup
constexpr int TE_RUNS = 8;                         // runs of 64 blocks the scan loads ahead of its serial part
static_assert(TE_B == 8 * IRA_WAVE, "a lane takes two quads of its block");

__device__ __forceinline__ int64_t tail_blocks(int64_t len) { return len > 0 ? (len + TE_B - 1) / TE_B : 0; }

__global__ __launch_bounds__(TE_THREADS) void tail_block_kernel(const float* __restrict__ x, const int64_t* __restrict__ start,
                                                                const int64_t* __restrict__ end,
                                                                const int64_t* __restrict__ tab_off, double* __restrict__ tab) {
  const int seg = blockIdx.y;
  const int64_t s0 = ira::uniform(start[seg]);
  const int64_t len = ira::uniform(end[seg]) - s0;
  const int64_t nblk = tail_blocks(len);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t j0 = ((int64_t)blockIdx.x * TE_WAVES + wave) * TE_BPW;
  if (j0 >= nblk) return;                          // a whole wave; the kernel has no barrier
  double* S = tab + ira::uniform(tab_off[seg]);
  const float* p = x + s0 + j0 * TE_B;
  const int64_t left = len - j0 * TE_B;            // samples from the wave's first block to the end: > 0
  f4u a[TE_BPW][2];
  if (left >= TE_BPW * TE_B) {
#pragma unroll
    for (int u = 0; u < TE_BPW; ++u)
#pragma unroll
      for (int h = 0; h < 2; ++h) a[u][h] = *reinterpret_cast<const f4u*>(p + u * TE_B + 4 * (lane + 64 * h));
  } else {
    // the segment's last blocks: zeros from `end` on (adding the square of a zero changes no sum), nothing read there
#pragma unroll
    for (int u = 0; u < TE_BPW; ++u)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int b = u * TE_B + 4 * (lane + 64 * h);
        if (b + 4 <= left) {
          a[u][h] = *reinterpret_cast<const f4u*>(p + b);
        } else {
          a[u][h] = f4u{0.0f, 0.0f, 0.0f, 0.0f};
          if (b < left) a[u][h].x = p[b];
          if (b + 1 < left) a[u][h].y = p[b + 1];
          if (b + 2 < left) a[u][h].z = p[b + 2];
        }
      }
  }
#pragma unroll
  for (int u = 0; u < TE_BPW; ++u) {
    double acc = 0.0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      acc = fma((double)a[u][h].x, (double)a[u][h].x, acc);
      acc = fma((double)a[u][h].y, (double)a[u][h].y, acc);
      acc = fma((double)a[u][h].z, (double)a[u][h].z, acc);
      acc = fma((double)a[u][h].w, (double)a[u][h].w, acc);
    }
    acc = ira::wave_sum(acc);
    if (lane == 0 && j0 + u < nblk) S[j0 + u] = acc;
  }
}

// One wave per segment folds the block energies into suffix sums, in place.  Runs of 64 blocks from the end: within a run the
// fixed tree of wave_suffix, between runs one carried double.  TE_RUNS runs are loaded before their scans, which are serial.
__global__ __launch_bounds__(IRA_WAVE) void tail_scan_kernel(const int64_t* __restrict__ start, const int64_t* __restrict__ end,
                                                             const int64_t* __restrict__ tab_off, double* __restrict__ tab) {
  const int seg = blockIdx.x;
  const int64_t nblk = tail_blocks(ira::uniform(end[seg]) - ira::uniform(start[seg]));
  double* S = tab + ira::uniform(tab_off[seg]);
  const int lane = threadIdx.x;
  if (lane == 0) S[nblk] = 0.0;
  double carry = 0.0;                              // wave-uniform: the sum of every run behind the current one
  for (int64_t r1 = (nblk + IRA_WAVE - 1) / IRA_WAVE; r1 > 0; r1 -= TE_RUNS) {
    double v[TE_RUNS];
#pragma unroll
    for (int u = 0; u < TE_RUNS; ++u) {
      const int64_t j = (r1 - 1 - u) * IRA_WAVE + lane;
      v[u] = (r1 - 1 - u >= 0 && j < nblk) ? S[j] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < TE_RUNS; ++u) {
      if (r1 - 1 - u < 0) break;                   // wave-uniform
      const int64_t j = (r1 - 1 - u) * IRA_WAVE + lane;
      double excl;
      const double incl = ira::wave_suffix(v[u], lane, excl);
      if (j < nblk) S[j] = incl + carry;
      carry = ira::uniform(__shfl(incl, 0, 64)) + carry;
    }
  }
}

}  // namespace

extern "C" int32_t ira_tail_energy(const float* x_dev, const int64_t* start_dev, const int64_t* end_dev,
                                   const int64_t* tab_off_dev, int32_t nseg, int32_t max_nblk, double* tab_dev,
                                   void* stream) {
  IRA_CHECK_PTR(x_dev); IRA_CHECK_PTR(start_dev); IRA_CHECK_PTR(end_dev); IRA_CHECK_PTR(tab_off_dev); IRA_CHECK_PTR(tab_dev);
  if (nseg < 0 || nseg > 65535 || max_nblk < 0) return IRA_E_SIZE;
  if (nseg == 0) return IRA_OK;
  hipStream_t st = (hipStream_t)stream;
  if (max_nblk > 0) {
    tail_block_kernel<<<dim3((unsigned)((max_nblk + TE_CHUNK - 1) / TE_CHUNK), nseg), TE_THREADS, 0, st>>>(
        x_dev, start_dev, end_dev, tab_off_dev, tab_dev);
    IRA_TRY_HIP(hipGetLastError());
  }
  tail_scan_kernel<<<nseg, IRA_WAVE, 0, st>>>(start_dev, end_dev, tab_off_dev, tab_dev);
  IRA_RETURN_LAUNCH();
}
