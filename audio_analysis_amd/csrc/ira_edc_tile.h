// The Schroeder-EDC conventions that more than one kernel file depends on: how a signal is cut into tiles, and how a
// suffix energy becomes a dB value.  Everything is inline, so it rounds the way its includer's -ffp-contract setting says.
#pragma once

#include "ira_common.h"
#include "ira_log.h"
#include "ira_reduce.h"

namespace ira {

// ---- tiles ----------------------------------------------------------------------------------------------------------------------
// A signal of n samples is cut into tiles of EDC_TILE samples counted from its END (the direction numpy.cumsum(e[::-1])
// accumulates in): tile j covers [max(n - (j + 1) EDC_TILE, 0), n - j EDC_TILE), so only the tile that holds the first sample
// can be short.  One EDC_THREADS-thread workgroup takes a tile, EDC_PER_THREAD consecutive samples per thread.
constexpr int EDC_THREADS = 256;
constexpr int EDC_PER_THREAD = 16;
constexpr int EDC_TILE = EDC_THREADS * EDC_PER_THREAD;
static_assert(EDC_TILE == 4096, "the host sizes its checks with 4096-sample tiles");

__host__ __device__ __forceinline__ long long edc_tile_count(long long n) { return (n + EDC_TILE - 1) / EDC_TILE; }

struct EdcSpan {
  long long lo, hi;                          // the tile's samples: [lo, hi)
  __host__ __device__ __forceinline__ int len() const { return (int)(hi - lo); }
};
__host__ __device__ __forceinline__ EdcSpan edc_tile_span(long long n, long long j) {
  const long long hi = n - j * EDC_TILE;
  return {hi > EDC_TILE ? hi - EDC_TILE : 0, hi};
}

// ---- the dB chain ---------------------------------------------------------------------------------------------------------------
// 10 log10(max(sum, eps) / norm) through the table log2 (ira_log.h): ~30 instructions per sample instead of ~110 for an f64
// divide + log10, same value to ~1e-14 dB; sum == norm gives exactly 0 dB.  Then the floor and the float32 cast.  np_max keeps
// a NaN: a NaN sample makes the reference's whole curve NaN (decay.py:151-166), an infinite one NaN before it and the floor
// after it.  Every kernel that forms a curve value goes through here, so a kernel that re-derives a value (the fused fits)
// sees the float32 curve the emit pass writes bit for bit.  Built once per workgroup, after the barrier that publishes ltab.
struct EdcDb {
  double eps, floor_db, norm, lnorm;
  bool fast;                                 // norm in the table's range; else the library path for every value
  const LogTabEntry* ltab;

  __device__ __forceinline__ EdcDb(double norm_, double eps_, double floor_db_, const LogTabEntry* ltab_)
      : eps(eps_), floor_db(floor_db_), norm(norm_), fast(norm_ > 1e-300 && norm_ < 1e300), ltab(ltab_) {
    lnorm = fast ? log2_table(norm, ltab) : 0.0;
  }
  // unfloored float64 (optional dB smoothing, decay.py:161-164)
  __device__ __forceinline__ double db64(double sum) const {
    const double v = np_max(sum, eps);
    if (fast && v > 1e-300 && v < 1e300) return 3.0102999566398120 * (log2_table(v, ltab) - lnorm);
    return 10.0 * log10(v / norm);
  }
  __device__ __forceinline__ float floored(double db) const { return (float)np_max(db, floor_db); }
  __device__ __forceinline__ float db32(double sum) const { return floored(db64(sum)); }
};

}  // namespace ira
