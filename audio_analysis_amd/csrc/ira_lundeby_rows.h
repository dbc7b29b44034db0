// The row of the block-energy tables (ira_block_energy) as the kernels that read them see it: shared by ira_lundeby.hip and
// ira_multislope.hip.
#pragma once

#include "ira_common.h"

namespace {

constexpr int LB_STAGE = 4096;                           // samples staged per workgroup; also the largest block size
constexpr int LB_MAX_BLOCKS = IRA_LUNDEBY_MAX_BLOCKS;
constexpr int64_t LB_MAX_LEN = (int64_t)2047 * 4096;     // the longest curve ira_curve_fits' callers produce (ira_edc_db)

struct LbRow {
  int64_t s, L;      // start index inside the signal, samples from it on
  int B, nb;         // block size, whole blocks (0 when the tables are inconsistent)
};

__device__ __forceinline__ LbRow lb_row(int row, const int64_t* __restrict__ base_len, const int32_t* __restrict__ chan_of_seg,
                                        const int64_t* __restrict__ start, const int32_t* __restrict__ blk_size,
                                        const int32_t* __restrict__ nblk) {
  LbRow r;
  const int64_t len = ira::uniform(base_len[row]);
  int64_t s = ira::uniform(start[ira::uniform(chan_of_seg[row])]);
  if (s < 0) s = 0;
  if (s > len) s = len;
  r.s = s;
  r.L = len - s;
  r.B = ira::uniform(blk_size[row]);
  r.nb = ira::uniform(nblk[row]);
  const bool ok = r.B >= 1 && r.B <= LB_STAGE && r.nb >= 0 && r.nb <= LB_MAX_BLOCKS && r.L <= LB_MAX_LEN &&
                  (int64_t)r.nb == r.L / r.B;
  if (!ok) { r.B = 1; r.nb = 0; r.L = 0; }
  return r;
}

}  // namespace
