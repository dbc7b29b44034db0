// Burst decay: per channel a map of windowed Fourier sums over (frequency point, step), every point seen through a window
// a fixed number of cycles long and moved along the channel in steps (include/ira.h and
// audio_analysis_amd/analyse/burstdecay.py state the definition).  Nothing in the reference computes it.
//
// ira_fdw_response makes weight and phasor of every term where it uses them.  A map uses the wavelet g_j of a point for
// every step and every channel, so it is made ONCE (burst_table_kernel, from the same ira::wavelet_term of ira_wavelet.h)
// and the map is a real-by-complex correlation against that table: two fmas and a conversion per term.
//
// Compiled with -ffp-contract=off for the reduction of the turn count (ira_wavelet.h); the sums call fma themselves.
//
//   burst_table_kernel  grid (ceil((2 max H + 1) / 256), points), 256 threads: one thread per table entry.
//   burst_decay_kernel  grid (points * ceil(steps / IRA_BURST_STEPS), ceil(channels / IRA_BURST_CHANNELS)), a wave per
//                       (channel, point, tile of IRA_BURST_STEPS steps).  Lane l owns the terms u = l, l + 64, .. of EVERY
//                       cell of the tile: per round one 16-byte load of g_j(u) and, per step, one load of 64 consecutive
//                       floats through a base address held in scalar registers.  The tile's 16 sums of a lane go to LDS
//                       and 16 lanes add the 64 lane sums of one value each in ascending lane order.  Workgroups are
//                       remapped so that an XCD takes consecutive (point, tile) of the same channels.
// Every table entry read on the device is clamped to its range and every sample index is tested against the channel, so no
// access leaves the channels, table_dev or out_dev even if the device tables do not hold the host's values.
#include <math.h>

#include "ira_common.h"
#include "ira_wavelet.h"

namespace {

constexpr int BD_THREADS = IRA_BURST_CHANNELS * IRA_WAVE;
constexpr int BD_TABLE_THREADS = 256;
constexpr int BD_VALUES = 2 * IRA_BURST_STEPS;                           // Re, Im of every step of a tile
constexpr int BD_PITCH = IRA_BURST_LANES + 1;                            // doubles: the 16 summing lanes on 16 banks
static_assert(IRA_BURST_LANES == IRA_WAVE, "a round is one term a lane");
static_assert(BD_VALUES <= IRA_WAVE, "a lane per value in the final sums");
static_assert(IRA_BURST_MAX_STEPS >= 1024 && IRA_BURST_MAX_DELTA >= 72000, "the default axes fit");

__global__ __launch_bounds__(BD_TABLE_THREADS) void burst_table_kernel(const double* __restrict__ rho_dev,
                                                                       const int32_t* __restrict__ half_dev,
                                                                       const int64_t* __restrict__ tab_off_dev, int window,
                                                                       int64_t entries, double* __restrict__ table) {
  const int j = blockIdx.y;
  const int h = ira::uniform(ira::wavelet_half(half_dev, j));
  const int64_t n = 2 * (int64_t)h + 1;
  const int64_t u = (int64_t)blockIdx.x * BD_TABLE_THREADS + threadIdx.x;
  const int64_t first = ira::uniform(tab_off_dev[j]);
  if (u >= n || first < 0 || first > entries - n) return;                // a point that would leave the table: not written
  const double rho = ira::uniform(rho_dev[j]);
  double sn, cs;
  const double w = ira::wavelet_term((int)(u - h), h, rho, window, [h] { return 1.0 / (double)(2 * h + 2); }, &sn, &cs);
  double2 g;
  g.x = w * cs;
  g.y = -(w * sn);
  reinterpret_cast<double2*>(table)[first + u] = g;
}

struct BdTile {
  const float* x[IRA_BURST_STEPS];                                       // the sample of term u = 0 of each step
  int first[IRA_BURST_STEPS], last[IRA_BURST_STEPS];                     // terms inside the channel: first .. last (none: 1, 0)
};

// One round: lane's term u of every step.  CHECKED rounds test u against the window and each step's terms inside.
// u < 2^22, so its byte offsets fit 32 bits: every load takes its base from scalar registers and a 32-bit offset from the
// lane, and a round computes two offsets, not a 64-bit address per load.
template <typename T>
__device__ __forceinline__ T bd_load(const T* base, unsigned bytes) {
  return *reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + bytes);
}

template <bool CHECKED>
__device__ __forceinline__ void bd_round(const BdTile& t, const double2* __restrict__ g, unsigned n, unsigned u,
                                         double (&acc)[BD_VALUES]) {
  const unsigned xb = u * (unsigned)sizeof(float), gb = u * (unsigned)sizeof(double2);
  float xv[IRA_BURST_STEPS];
#pragma unroll
  for (int s = 0; s < IRA_BURST_STEPS; ++s) {
    if (CHECKED)
      xv[s] = (int)u >= t.first[s] && (int)u <= t.last[s] ? bd_load(t.x[s], xb) : 0.0f;
    else
      xv[s] = bd_load(t.x[s], xb);
  }
  double2 gv;
  if (CHECKED) {
    gv.x = gv.y = 0.0;
    if (u < n) gv = bd_load(g, gb);
  } else {
    gv = bd_load(g, gb);
  }
#pragma unroll
  for (int s = 0; s < IRA_BURST_STEPS; ++s) {
    const double v = (double)xv[s];
    acc[2 * s] = fma(gv.x, v, acc[2 * s]);
    acc[2 * s + 1] = fma(gv.y, v, acc[2 * s + 1]);
  }
}

__global__ __launch_bounds__(BD_THREADS) void burst_decay_kernel(const float* __restrict__ x, const int64_t* __restrict__ off,
                                                                 const int64_t* __restrict__ len,
                                                                 const int64_t* __restrict__ centre, int nch,
                                                                 const int32_t* __restrict__ half_dev,
                                                                 const int64_t* __restrict__ tab_off_dev,
                                                                 const double* __restrict__ table, int64_t entries,
                                                                 const int32_t* __restrict__ delta_dev, int npts, int nsteps,
                                                                 int tiles, double* __restrict__ out) {
  __shared__ double s_sum[IRA_BURST_CHANNELS][BD_VALUES * BD_PITCH];
  const int lane = threadIdx.x & (IRA_WAVE - 1), wv = threadIdx.x / IRA_WAVE;
  // The tiles of a point share most of their samples and neighbouring points a part: the remap gives each XCD a run of
  // consecutive (point, tile) of the same channels, so that they meet in one L2 (speed only: 4.6 -> 3.1 ms at the defaults).
  unsigned bx = blockIdx.x, by = blockIdx.y;
  ira::xcd_remap(bx, by);
  const int c = (int)by * IRA_BURST_CHANNELS + wv;
  if (c >= nch) return;                                                  // the whole wave; the waves of a workgroup never meet
  const int j = (int)bx / tiles, m0 = ((int)bx % tiles) * IRA_BURST_STEPS;
  const int h = ira::uniform(ira::wavelet_half(half_dev, j));
  const int n = 2 * h + 1;
  const int64_t first = ira::uniform(tab_off_dev[j]);
  const bool table_ok = first >= 0 && first <= entries - n;
  const float* xc = x + ira::uniform(off[c]);
  int64_t length = ira::uniform(len[c]);
  length = length > 0 ? length : 0;
  const int64_t p = ira::wavelet_centre(ira::uniform(centre[c]));

  // per step: the terms inside the channel; over the tile: the rounds that hold any, and those that hold nothing else
  BdTile t;
  int any_first = n, any_last = -1, all_first = 0, all_last = n - 1;
#pragma unroll
  for (int s = 0; s < IRA_BURST_STEPS; ++s) {
    const int m = m0 + s < nsteps ? m0 + s : nsteps - 1;                 // a step past the end repeats the last; not stored
    int d = ira::uniform(delta_dev[(int64_t)j * nsteps + m]);
    d = d > IRA_BURST_MAX_DELTA ? IRA_BURST_MAX_DELTA : (d < -IRA_BURST_MAX_DELTA ? -IRA_BURST_MAX_DELTA : d);
    const int64_t lo = p + d - h;                                        // the sample index of term u = 0
    const int64_t a = lo < 0 ? -lo : 0, b = length - 1 - lo;             // terms a .. b are inside
    if (a < n && b >= 0 && a <= b) {
      t.first[s] = (int)a;
      t.last[s] = b < n - 1 ? (int)b : n - 1;
      t.x[s] = xc + lo;                                                  // read only at first .. last
    } else {
      t.first[s] = 1;
      t.last[s] = 0;
      t.x[s] = xc;
    }
    if (t.first[s] <= t.last[s]) {
      any_first = t.first[s] < any_first ? t.first[s] : any_first;
      any_last = t.last[s] > any_last ? t.last[s] : any_last;
    }
    all_first = t.first[s] > all_first ? t.first[s] : all_first;
    all_last = t.last[s] < all_last ? t.last[s] : all_last;
  }
  double acc[BD_VALUES];
#pragma unroll
  for (int q = 0; q < BD_VALUES; ++q) acc[q] = 0.0;
  if (table_ok && any_last >= any_first) {
    const double2* g = reinterpret_cast<const double2*>(table) + first;
    const int r_begin = any_first / IRA_BURST_LANES, r_end = any_last / IRA_BURST_LANES + 1;
    // rounds r_all .. r_all_end - 1: every lane's term is inside the channel for every step (an empty step: none)
    int r_all = (all_first + IRA_BURST_LANES - 1) / IRA_BURST_LANES, r_all_end = (all_last + 1) / IRA_BURST_LANES;
    r_all = r_all < r_begin ? r_begin : (r_all > r_end ? r_end : r_all);
    r_all_end = r_all_end < r_all ? r_all : (r_all_end > r_end ? r_end : r_all_end);
    const unsigned un = (unsigned)n, ul = (unsigned)lane;
    for (int r = r_begin; r < r_all; ++r) bd_round<true>(t, g, un, (unsigned)r * IRA_BURST_LANES + ul, acc);
#pragma unroll 4
    for (int r = r_all; r < r_all_end; ++r) bd_round<false>(t, g, un, (unsigned)r * IRA_BURST_LANES + ul, acc);
    for (int r = r_all_end; r < r_end; ++r) bd_round<true>(t, g, un, (unsigned)r * IRA_BURST_LANES + ul, acc);
  }
  // the 64 lane sums of each value, added in ascending lane order by one lane
  double* sums = s_sum[wv];
#pragma unroll
  for (int q = 0; q < BD_VALUES; ++q) sums[q * BD_PITCH + lane] = acc[q];
  ira::wave_sync();
  if (lane < BD_VALUES && m0 + lane / 2 < nsteps) {
    const double* row = sums + lane * BD_PITCH;
    double v = row[0];
    for (int l = 1; l < IRA_BURST_LANES; ++l) v += row[l];
    if (!table_ok) v = __builtin_nan("");
    out[(((int64_t)c * npts + j) * nsteps + m0) * 2 + lane] = v;
  }
}

// the entries of the table of a checked grid
int64_t bd_entries(const int32_t* half, int32_t npts) {
  int64_t total = 0;
  for (int32_t j = 0; j < npts; ++j) total += 2 * (int64_t)half[j] + 1;
  return total;
}

}  // namespace

extern "C" int64_t ira_burst_table_doubles(const int32_t* half, int32_t npts) {
  const int32_t rc = ira::wavelet_points_check(nullptr, half, npts, 0);
  return rc != IRA_OK ? rc : 2 * bd_entries(half, npts);
}

extern "C" int32_t ira_burst_table(const double* rho, const int32_t* half, const double* rho_dev, const int32_t* half_dev,
                                   const int64_t* tab_off_dev, int32_t npts, int32_t window, double* table_dev,
                                   int64_t table_doubles, void* stream) {
  IRA_CHECK_PTR(rho); IRA_CHECK_PTR(half); IRA_CHECK_PTR(rho_dev); IRA_CHECK_PTR(half_dev); IRA_CHECK_PTR(tab_off_dev);
  IRA_CHECK_PTR(table_dev);
  const int32_t rc = ira::wavelet_points_check(rho, half, npts, window);
  if (rc != IRA_OK) return rc;
  if (table_doubles < 2 * bd_entries(half, npts)) return IRA_E_SIZE;
  if (npts == 0) return IRA_OK;
  int32_t widest = 1;
  for (int32_t j = 0; j < npts; ++j) widest = half[j] > widest ? half[j] : widest;
  const unsigned blocks = (unsigned)((2 * (int64_t)widest + 1 + BD_TABLE_THREADS - 1) / BD_TABLE_THREADS);
  burst_table_kernel<<<dim3(blocks, (unsigned)npts), BD_TABLE_THREADS, 0, (hipStream_t)stream>>>(
      rho_dev, half_dev, tab_off_dev, window, table_doubles / 2, table_dev);
  IRA_RETURN_LAUNCH();
}

extern "C" int32_t ira_burst_decay(const float* x_dev, const int64_t* off_dev, const int64_t* len_dev,
                                   const int64_t* centre_dev, int32_t nch, const int32_t* half, const int32_t* half_dev,
                                   const int64_t* tab_off_dev, const double* table_dev, int64_t table_doubles,
                                   const int32_t* delta, const int32_t* delta_dev, int32_t npts, int32_t nsteps,
                                   double* out_dev, void* stream) {
  IRA_CHECK_PTR(x_dev); IRA_CHECK_PTR(off_dev); IRA_CHECK_PTR(len_dev); IRA_CHECK_PTR(centre_dev); IRA_CHECK_PTR(half);
  IRA_CHECK_PTR(half_dev); IRA_CHECK_PTR(tab_off_dev); IRA_CHECK_PTR(table_dev); IRA_CHECK_PTR(delta);
  IRA_CHECK_PTR(delta_dev); IRA_CHECK_PTR(out_dev);
  if (nch < 0 || nch > 65535 || nsteps < 0 || nsteps > IRA_BURST_MAX_STEPS) return IRA_E_SIZE;
  const int32_t rc = ira::wavelet_points_check(nullptr, half, npts, 0);
  if (rc != IRA_OK) return rc;
  if (table_doubles < 2 * bd_entries(half, npts)) return IRA_E_SIZE;
  for (int32_t j = 0; j < npts; ++j) {
    const int32_t* d = delta + (int64_t)j * nsteps;
    for (int32_t m = 0; m < nsteps; ++m) {
      if (d[m] > IRA_BURST_MAX_DELTA || d[m] < -IRA_BURST_MAX_DELTA) return IRA_E_SIZE;
      if (m > 0 && d[m] < d[m - 1]) return IRA_E_SIZE;
    }
  }
  if (nch == 0 || npts == 0 || nsteps == 0) return IRA_OK;
  const int tiles = (nsteps + IRA_BURST_STEPS - 1) / IRA_BURST_STEPS;
  const dim3 grid((unsigned)npts * (unsigned)tiles, (unsigned)((nch + IRA_BURST_CHANNELS - 1) / IRA_BURST_CHANNELS));
  burst_decay_kernel<<<grid, BD_THREADS, 0, (hipStream_t)stream>>>(x_dev, off_dev, len_dev, centre_dev, nch, half_dev,
                                                                   tab_off_dev, table_dev, table_doubles / 2, delta_dev, npts,
                                                                   nsteps, tiles, out_dev);
  IRA_RETURN_LAUNCH();
}
